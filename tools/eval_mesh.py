#!/usr/bin/env python
"""Geometric evaluation of a mesh against a ground-truth point set on the GPU (gs2mesh_amd.evaluation):

    python tools/eval_mesh.py mesh.ply gt_points.ply [--dtu-dir D --scan N] [--density 0.2] [--max-dist 20]
                              [--thresholds 0.0025,0.005] [--cull-dir scanN [--cull-radius 24] [--save-culled culled.ply]]
                              [--icp-gt-mesh gt_mesh.ply] [--tnt-dir SCENE_DIR --tnt-init trans.txt --tau X]

prints one JSON object: the DTU evaluation's keys (mean_d2s, mean_s2d, overall; evaluation/DTU/eval_code/eval.py) and,
with --thresholds, MobileBrick's (pred_gt, gt_pred, chamfer and per threshold accuracy, recall, F1) under "fscore".
--dtu-dir / --scan read D/ObsMask/ObsMask<N>_10.mat and D/ObsMask/Plane<N>.mat as the reference does (scipy.io.loadmat).
--cull-dir first culls the mesh as the reference's cull_scan does (evaluation.dtu_cull): it reads scanN/cameras.npz and the
sorted scanN/mask/*.png, and the result gains "n_vertices_culled"; --save-culled writes the culled mesh (DTU world frame).
--icp-gt-mesh first aligns the mesh as MobileBrick's evaluation does (evaluation.mobilebrick_align: ICP from the GT mesh's
vertices to the mesh's, the inverse applied when the fitness is above 0.99); the result gains "icp" = {fitness, inlier_rmse,
n_iterations, applied}.  --tnt-dir runs TNT's flow instead (evaluation.tnt_evaluate) on the mesh's vertices against gt_points:
SCENE_DIR/<name of SCENE_DIR>.json is the crop volume, --tnt-init the 4 x 4 initial alignment (the reference gets it from its
trajectory registration, which is not part of this package), --tau the scene's distance; it prints {precision, recall, fscore,
transformation, n_source, n_target}.
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
    ap.add_argument("--cull-dir", default=None, help="DTU scan directory with cameras.npz and mask/*.png")
    ap.add_argument("--cull-radius", type=int, default=24, help="radius of the disk the masks are dilated with (the reference: 24)")
    ap.add_argument("--save-culled", default=None, help="write the culled mesh to this PLY (needs --cull-dir)")
    ap.add_argument("--icp-gt-mesh", default=None, help="GT mesh PLY: MobileBrick's ICP alignment before scoring")
    ap.add_argument("--tnt-dir", default=None, help="TNT scene directory holding <scene>.json (the crop volume)")
    ap.add_argument("--tnt-init", default=None, help="text file of the 4x4 initial alignment (needs --tnt-dir)")
    ap.add_argument("--tau", type=float, default=None, help="TNT's distance threshold of the scene (needs --tnt-dir)")
    args = ap.parse_args(argv)

    from gs2mesh_amd import evaluation
    from gs2mesh_amd.mesh import read_point_cloud, read_triangle_mesh, write_triangle_mesh

    kw = {}
    if args.dtu_dir is not None:
        if args.scan is None:
            ap.error("--dtu-dir needs --scan")
        from scipy.io import loadmat            # only the DTU files need it
        obs = loadmat(os.path.join(args.dtu_dir, "ObsMask", f"ObsMask{args.scan}_10.mat"))
        kw.update(obs_mask=obs["ObsMask"], bb=obs["BB"], res=obs["Res"],
                  plane=loadmat(os.path.join(args.dtu_dir, "ObsMask", f"Plane{args.scan}.mat"))["P"])
    thresholds = [float(t) for t in args.thresholds.split(",") if t.strip()]
    mesh = read_triangle_mesh(args.mesh)
    if args.tnt_dir is not None:
        if args.tnt_init is None or args.tau is None:
            ap.error("--tnt-dir needs --tnt-init and --tau")
        import numpy as np
        scene = os.path.basename(os.path.normpath(args.tnt_dir))
        out = evaluation.tnt_evaluate(mesh.vertices, read_point_cloud(args.gt_points), np.loadtxt(args.tnt_init).reshape(4, 4),
                                      evaluation.read_crop_volume(os.path.join(args.tnt_dir, scene + ".json")), args.tau)
        out["transformation"] = out["transformation"].tolist()
        print(json.dumps(out))
        return out
    icp = None
    if args.icp_gt_mesh is not None:
        mesh, r = evaluation.mobilebrick_align(mesh, read_triangle_mesh(args.icp_gt_mesh))
        icp = {"fitness": r.fitness, "inlier_rmse": r.inlier_rmse, "n_iterations": r.n_iterations, "applied": bool(r.fitness > 0.99)}
    if args.save_culled is not None and args.cull_dir is None:
        ap.error("--save-culled needs --cull-dir")
    if args.cull_dir is not None:
        import glob
        kw.update(cull=dict(cameras=os.path.join(args.cull_dir, "cameras.npz"),
                            masks=sorted(glob.glob(os.path.join(args.cull_dir, "mask", "*.png"))), radius=args.cull_radius))
        if args.save_culled is not None:
            write_triangle_mesh(args.save_culled, evaluation.dtu_cull(mesh, **kw["cull"]))
    out = evaluation.evaluate_mesh(mesh, read_point_cloud(args.gt_points), density=args.density,
                                   max_dist=args.max_dist, thresholds=thresholds, patch=args.patch, **kw)
    if icp is not None:
        out["icp"] = icp
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
