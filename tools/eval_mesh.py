#!/usr/bin/env python
"""Geometric evaluation of a mesh against a ground-truth point set on the GPU (gs2mesh_amd.evaluation):

    python tools/eval_mesh.py mesh.ply gt_points.ply [--dtu-dir D --scan N] [--density 0.2] [--max-dist 20]
                              [--thresholds 0.0025,0.005]

prints one JSON object: the DTU evaluation's keys (mean_d2s, mean_s2d, overall; evaluation/DTU/eval_code/eval.py) and,
with --thresholds, MobileBrick's (pred_gt, gt_pred, chamfer and per threshold accuracy, recall, F1) under "fscore".
--dtu-dir / --scan read D/ObsMask/ObsMask<N>_10.mat and D/ObsMask/Plane<N>.mat as the reference does (scipy.io.loadmat).
The mesh is this package's own PLY; the ground truth is any vertex PLY (binary little-endian or ASCII)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("gt_points")
    ap.add_argument("--dtu-dir", default=None)
    ap.add_argument("--scan", type=int, default=None)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--patch", type=float, default=60.0)
    ap.add_argument("--thresholds", default="", help="comma-separated distances for accuracy / recall / F1")
    args = ap.parse_args(argv)

    from gs2mesh_amd import evaluation
    from gs2mesh_amd.mesh import read_point_cloud, read_triangle_mesh

    kw = {}
    if args.dtu_dir is not None:
        if args.scan is None:
            ap.error("--dtu-dir needs --scan")
        from scipy.io import loadmat            # only the DTU files need it
        obs = loadmat(os.path.join(args.dtu_dir, "ObsMask", f"ObsMask{args.scan}_10.mat"))
        kw.update(obs_mask=obs["ObsMask"], bb=obs["BB"], res=obs["Res"],
                  plane=loadmat(os.path.join(args.dtu_dir, "ObsMask", f"Plane{args.scan}.mat"))["P"])
    thresholds = [float(t) for t in args.thresholds.split(",") if t.strip()]
    out = evaluation.evaluate_mesh(read_triangle_mesh(args.mesh), read_point_cloud(args.gt_points), density=args.density,
                                   max_dist=args.max_dist, thresholds=thresholds, patch=args.patch, **kw)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
