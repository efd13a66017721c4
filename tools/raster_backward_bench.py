"""Operator-level cost of the rasteriser's backward pass on the C2 model (300 k Gaussians), one 1600 x 1200 view.

  python tools/raster_backward_bench.py [--reps 20] [--kernel-stats] [--out profiles/raster_backward_bench.json]

  * forward alone and forward + backward, timed with hipEvents around `reps` repetitions after a warm-up;
  * N (instances of the view), the instance rows and the row-buffer bytes of the backward;
  * whether two backward calls on the same state give bit-identical gradients;
  * with --kernel-stats: the split per kernel from ONE `rocprofv3 --kernel-trace --stats` run of a child process that only runs
    forward + backward, and from it the achieved store bandwidth of the compositing backward (the 36 stored bytes of every row / its time,
    a lower bound: the kernel also computes) and the gather bandwidth of the per-Gaussian pass (row bytes read / its time).
Prints one JSON object.  No speed gate: the figure of interest is the backward / forward ratio and what bounds each kernel.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 48   # GS2M_BW_ROW floats per instance row (gs2mesh_amd/csrc/raster_common.h)


def setup(config):
    import numpy as np
    import torch
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.rasterizer import Rasterizer
    cfg = synthetic.CONFIGS[config]
    g = synthetic.synth_v1(cfg.P, cfg.seed, cfg.log_s_mu)
    pose = synthetic.ring_poses(cfg.n_pairs, cfg.ring_radius)[0]
    cam, _ = synthetic.stereo_cameras(pose, cfg.width, cfg.height, cfg.focal, cfg.focal, cfg.baseline)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    xyz = t(g["xyz"])
    scales = torch.exp(t(g["scaling"]))
    rots = torch.nn.functional.normalize(t(g["rotation"]))
    opac = torch.sigmoid(t(g["opacity"])).reshape(-1).contiguous()
    shs = t(np.concatenate([g["features_dc"], g["features_rest"]], axis=1))
    W, H = cfg.width, cfg.height
    common = (t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
              torch.tensor([0.1, 0.2, 0.3], device=dev), W, H, cam.tanfovx, cam.tanfovy)
    kw = dict(shs=shs, scales=scales, rotations=rots, sh_degree=3)
    dL = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (3, H, W)).astype(np.float32)).to(dev)
    r = Rasterizer(0)
    fwd = lambda sync=False: r.forward(xyz, opac, *common, sync=sync, **kw)
    bwd = lambda: r.backward(dL, xyz, *common, **kw)
    return r, fwd, bwd


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_stats(config, reps):
    """one rocprofv3 --kernel-trace --stats run of a child that only runs forward + backward -> {kernel: average us}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--config", config, "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=400)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0].replace("void ", "")
                out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) only run forward + backward, for the profiler")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    r, fwd, bwd = setup(a.config)
    fwd(sync=True)   # sizes the instance arena
    if a.child:
        for _ in range(a.reps):
            fwd()
            bwd()
        torch.cuda.synchronize()
        return
    for _ in range(3):
        fwd()
        bwd()
    g1 = bwd()
    g2 = bwd()
    torch.cuda.synchronize()
    same = all(torch.equal(g1[k], g2[k]) for k in g1 if g1[k] is not None)
    fwd(sync=True)
    n = int(r.last_num_rendered)
    t_f = timed(fwd, a.reps)
    t_fb = timed(lambda: (fwd(), bwd()), a.reps)
    rows, arena = r.backward_rows()
    res = dict(config=a.config, reps=a.reps, instances=n, rows=rows, row_bytes=rows * ROW_BYTES, row_arena_bytes=arena,
               forward_ms=round(t_f, 4), forward_backward_ms=round(t_fb, 4), backward_ms=round(t_fb - t_f, 4),
               backward_over_forward=round((t_fb - t_f) / t_f, 2), gradients_bit_identical=bool(same))
    if a.kernel_stats:
        ks = kernel_stats(a.config, a.reps)
        res["kernels"] = ks
        # 36 of a row's 48 bytes are stored (upper bound: rows nobody contributed to are not written); all 48 are read back
        for key, name, nbytes in (("store_GBps", "k_blend_backward<4", 36), ("gather_GBps", "k_gaussian_backward", ROW_BYTES)):
            hit = [k for k in ks if k.startswith(name)]
            if hit and ks[hit[0]]["avg_us"] > 0:
                res[key] = round(rows * nbytes / (ks[hit[0]]["avg_us"] * 1e-6) / 1e9, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
