"""The depth stage on a C2-shaped scene (1600 x 1200, focal 2900, a textured sphere seen from a ring): one JSON line.

  * stream time of gs2m_stereo_sgm (LR + RL) for D = 128 and 256 (torch events around repeated calls, the median of
    `--repeats` after `--warmup`), the bytes of the traffic model in gs2mesh_amd/csrc/sgm_kernels.h (8 N bytes per direction,
    N = H W D: two u8 planes written, read back with one u16 plane written, that plane read) and the fraction of the
    measured 6.29 TB/s copy rate that the time amounts to;
  * with --kernel-stats: the split per kernel from one `rocprofv3 --kernel-trace --stats` run of a child process that only
    matches (this tool started with --child-match);
  * wall views/s of Stereo.run with files and of the in-memory chain Stereo.run(keep_on_device, no files) + TSDF.run(batch),
    next to the render time per pair of the same scene.

Files go to --root (a tmpfs by default).  Usage:  python tools/stereo_bench.py [--views 8] [--kernel-stats]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs2mesh_amd import stereo_utils, synthetic  # noqa: E402
from gs2mesh_amd.gaussian_model import write_gaussian_ply  # noqa: E402

W, H, FOCAL, BASELINE, RING, RADIUS = 1600, 1200, 2900.0, 0.245, 3.5, 0.6
COPY_RATE = 6.29e12        # measured copy rate of the MI355X, bytes / s


def make_args(**kw):
    from argparse import Namespace
    a = dict(colmap_name="scene", dataset_name="custom", GS_white_background=False, GS_iterations=30000,
             renderer_baseline_absolute=BASELINE, renderer_baseline_percentage=7.0, renderer_scene_360=True,
             renderer_save_json=False, renderer_sort_cameras=False, png_encoder="device", stereo_model="SGM",
             stereo_max_disparity=256, stereo_occlusion_threshold=3, stereo_warm=False, TSDF_scale=1.0, TSDF_dilate=1,
             TSDF_valid=None, TSDF_skip=None, TSDF_use_occlusion_mask=True, TSDF_use_mask=False, TSDF_invert_mask=False,
             TSDF_erode_mask=True, TSDF_erosion_kernel_size=10, TSDF_closing_kernel_size=10, TSDF_voxel=2,
             TSDF_sdf_trunc=0.04, TSDF_min_depth_baselines=4, TSDF_max_depth_baselines=20, TSDF_cleaning_threshold=1000)
    a.update(kw)
    return Namespace(**a)


def write_scene(base, n_views, P, sigma, seed):
    from scipy.spatial.transform import Rotation
    g = synthetic.textured_sphere(P, seed, RADIUS, sigma)
    ply = os.path.join(base, "splatting_output", "custom", "scene", "point_cloud", "iteration_30000")
    os.makedirs(ply)
    write_gaussian_ply(os.path.join(ply, "point_cloud.ply"), g["xyz"], g["features_dc"], g["features_rest"], g["opacity"],
                       g["scaling"], g["rotation"])
    sp = os.path.join(base, "colmap", "sparse", "0")
    os.makedirs(sp)
    with open(os.path.join(sp, "cameras.txt"), "w") as f:
        f.write(f"1 PINHOLE {W} {H} {FOCAL} {FOCAL} {W / 2} {H / 2}\n")
    with open(os.path.join(sp, "images.txt"), "w") as f:
        for i, p in enumerate(synthetic.ring_poses(n_views, RING)):
            q = Rotation.from_matrix(p[:, :3]).as_quat()
            vals = [q[3], q[0], q[1], q[2], p[0, 3], p[1, 3], p[2, 3]]
            f.write(f"{i + 1} " + " ".join(repr(float(v)) for v in vals) + f" 1 img{i:03}.png\n\n")


def stream_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def match_only(rgb8, warmup, repeats):
    res = {}
    for D in (128, 256):
        ms = stream_ms(lambda: stereo_utils.sgm_disparity(rgb8[0], rgb8[1], D), warmup, repeats)
        nbytes = 2 * 8 * W * H * D
        med = statistics.median(ms)
        res[f"D{D}"] = dict(stream_ms_median=round(med, 4), stream_ms_min=round(min(ms), 4), stream_ms_max=round(max(ms), 4),
                            model_bytes=nbytes, model_ms_at_copy_rate=round(nbytes / COPY_RATE * 1e3, 4),
                            fraction_of_copy_rate=round(nbytes / (med * 1e-3) / COPY_RATE, 4))
    return res


def kernel_stats(argv, out_dir):
    """one rocprofv3 --kernel-trace --stats run of a child that only matches -> {D: {kernel: average ms per call}}"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable,
           os.path.abspath(__file__), "--child-match"] + argv
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    if r.returncode != 0:
        return dict(error=r.stdout.decode(errors="replace")[-400:])
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_sgm" in row["Name"]:
                name = row["Name"].split("(")[0].replace("void ", "")
                rows[name] = dict(calls=int(row["Calls"]), average_ms=round(float(row["AverageNs"]) * 1e-6, 4))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--splats", type=int, default=300_000)
    ap.add_argument("--sigma", type=float, default=0.006)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--root", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child-match", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    from gs2mesh_amd.renderer_utils import Renderer
    from gs2mesh_amd.stereo_utils import Stereo
    from gs2mesh_amd.tsdf_utils import TSDF
    base = tempfile.mkdtemp(prefix="stereo_bench_", dir=a.root)
    try:
        write_scene(base, a.views, a.splats, a.sigma, 7)
        args = make_args()
        ren = Renderer(base, os.path.join(base, "colmap"), os.path.join(base, "out"), args)
        ren.prepare_renderer()
        rgb8 = ren.render_pair_device(1)["rgb8"].clone()
        if a.child_match:
            match_only(rgb8, 2, 10)
            return None
        res = dict(tool="stereo_bench", width=W, height=H, focal=FOCAL, views=a.views, splats=a.splats, copy_rate=COPY_RATE)
        res["match"] = match_only(rgb8, a.warmup, a.repeats)
        res["render_pair_ms"] = round(statistics.median(stream_ms(lambda: ren.render_pair_device(1), a.warmup, a.repeats)), 4)
        if a.kernel_stats:
            res["kernels"] = kernel_stats(["--views", "2", "--splats", str(a.splats), "--sigma", str(a.sigma)] +
                                          (["--root", a.root] if a.root else []), os.path.join(base, "rocprof"))
        # wall: files, then the in-memory chain (first of three runs each is the warm-up; the median of the others)
        stereo = Stereo(base, ren, args)
        walls, chain, timings = [], [], None
        for rep in range(3):
            t0 = time.perf_counter()
            stereo.run()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            timings = {k: round(v, 4) for k, v in stereo.timings.items()}
            t0 = time.perf_counter()
            stereo.run(keep_on_device=True, write_files=False)
            t = TSDF(ren, stereo, args, "bench", frame_source=stereo.frame_source, fuse="batch")
            t.run()
            torch.cuda.synchronize()
            chain.append(time.perf_counter() - t0)
        res["stereo_run_files_views_per_s"] = round(a.views / statistics.median(walls[1:]), 3)
        res["stereo_run_files_timings_s"] = timings
        res["memory_chain_views_per_s"] = round(a.views / statistics.median(chain[1:]), 3)
        res["memory_chain_triangles"] = int(np.asarray(t.mesh.triangles).shape[0])
        print(json.dumps(res))
        return res
    finally:
        shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
