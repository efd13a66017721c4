"""Cost of depth without a matcher on a C2-shaped job (300 k Gaussians, 1600 x 1200).

  python tools/depth_bench.py [--reps 50] [--repeats 5] [--views 16] [--out profiles/raster_depth_bench.json]
                              [--parent-lib PATH] [--skip-pipeline] [--splat synth_v1|trained_like] [--skip-backward]
                              [--surfel-mesh] [--kernel-stats]

  * the depth pass (gs2m_rasterize_depth: all three maps of one view), in us per view, and gs2m_rasterize_forward as a whole:
    stream events around `reps` calls after a warm-up, `repeats` times (median and range: the spread comes with the figure);
  * RenderedDepth.run(keep_on_device=True, write_files=False) + TSDF.run(fuse="batch") over `views` ring cameras, in views/s:
    a host clock around work that ends in the mesh download, after one warm-up pass of the same shapes.
  * the backward pass, in us per view, each call with its one stream synchronisation: gs2m_rasterize_backward (colour only)
    gs2m_rasterize_backward_depth with all three map gradients and gs2m_rasterize_backward_depth_ray with the same three (on
    the ray maps; with --parent-lib also against the parent's gs2m_rasterize_backward_depth); with --parent-lib (a libgs2mesh_amd.so built from the
    parent commit) also the parent's gs2m_rasterize_backward on the same inputs, the three ALTERNATING inside every repeat
    (this, parent, depth, parent, this, ...) so that drift of the shared machine hits them alike.  `backward_same_code_spread`
    is the spread of this commit's colour backward against itself (its even repeats over its odd ones): a
    difference to the parent inside it is code placement, not a cost.
  * the ray depth call (gs2m_rasterize_depth_ray: record pass + walk, all three maps) next to the centre call on the same
    forward, the two ALTERNATING inside every repeat; with --parent-lib also the parent's centre call (the walk template is
    shared: `depth_pass_over_parent` beyond `depth_pass_same_code_spread` would be a defect).  With --kernel-stats the ray
    call's two kernels (k_ray_records, k_blend_depth<4, true>) are told apart by ONE `rocprofv3 --kernel-trace --stats` run of a
    child process that only runs the forward once and then the centre and the ray call.
  * --surfel-mesh: `synthetic.surfel_sphere` (flat discs on the test sphere) on 12 ring views at 320 x 240, fused from
    kind="median" and from kind="ray_median": mean | |v| - R | over the mesh vertices.
Prints one JSON object.  No speed gate: nothing of this had been measured before.
"""
import argparse
import csv
import glob
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tsdf_args():
    return Namespace(TSDF_scale=1.0, TSDF_dilate=1, TSDF_valid=None, TSDF_skip=None, TSDF_use_occlusion_mask=True,
                     TSDF_use_mask=False, TSDF_invert_mask=False, TSDF_erode_mask=True, TSDF_erosion_kernel_size=10,
                     TSDF_closing_kernel_size=10, TSDF_voxel=2, TSDF_sdf_trunc=0.04, TSDF_min_depth_baselines=4,
                     TSDF_max_depth_baselines=20, TSDF_cleaning_threshold=100000)


def make_scene(cfg, views, root, device, splat="synth_v1"):
    """the part of Renderer that RenderedDepth and TSDF read, for the config's synthetic splat on `views` ring cameras"""
    import torch
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.gaussian_model import GaussianModel
    poses = synthetic.ring_poses(views, cfg.ring_radius)
    baseline = cfg.ring_radius * cfg.baseline_pct / 100.0
    scene = synthetic.DiskScene(root, poses, cfg.width, cfg.height, cfg.focal, baseline)
    if splat == "trained_like":
        g = synthetic.trained_like(cfg.P, cfg.seed, cfg.log_s_mu, focal=cfg.focal, ring_radius=cfg.ring_radius)
    else:
        g = synthetic.synth_v1(cfg.P, cfg.seed, cfg.log_s_mu)
    model = GaussianModel(3, device=device)
    model.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    background = torch.zeros(3, device=device)
    cams = [synthetic.stereo_cameras(p, cfg.width, cfg.height, cfg.focal, cfg.focal, baseline)[0] for p in poses]
    scene.left_view = lambda i: (cams[i], model, background)
    return scene, model, cams


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


def surfel_mesh(torch, root):
    """mean | |v| - R | of the meshes fused from the centre and from the ray median depth of a flat-disc sphere"""
    import numpy as np
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.depth_utils import RenderedDepth
    from gs2mesh_amd.gaussian_model import GaussianModel
    from gs2mesh_amd.tsdf_utils import TSDF
    R, ring, W, H, focal, views, P = 0.6, 3.5, 320, 240, 600.0, 12, 6000
    poses = synthetic.ring_poses(views, ring)
    scene = synthetic.DiskScene(os.path.join(root, "surfel"), poses, W, H, focal, 0.245)
    g = synthetic.surfel_sphere(P, 7, R, 0.03)
    model = GaussianModel(3, device="cuda:0")
    model.load_arrays(g["xyz"], g["features_dc"], g["features_rest"], g["scaling"], g["rotation"], g["opacity"])
    bg = torch.zeros(3, device="cuda:0")
    cams = [synthetic.stereo_cameras(p, W, H, focal, focal, 0.245)[0] for p in poses]
    scene.left_view = lambda i: (cams[i], model, bg)
    args = tsdf_args()
    args.TSDF_voxel, args.TSDF_sdf_trunc = 8, 0.1       # 1/64 voxels
    out = dict(P=P, views=views, width=W, height=H, sigma=0.03, radius=R, voxel=1 / 64)
    for kind in ("median", "ray_median"):
        rd = RenderedDepth(scene.output_dir_root, scene, args, kind=kind)
        rd.run(keep_on_device=True, write_files=False)
        fuse = TSDF(scene, rd, args, kind, frame_source=rd.frame_source, fuse="batch")
        fuse.run()
        v = np.asarray(fuse.mesh.vertices, np.float64)
        d = np.abs(np.linalg.norm(v, axis=1) - R)
        out[kind] = dict(vertices=int(v.shape[0]), mean_abs_radius_error=round(float(d.mean()), 6),
                         median=round(float(np.median(d)), 6), q95=round(float(np.quantile(d, 0.95)), 6))
    return out


def kernel_stats(a):
    """one rocprofv3 --kernel-trace --stats run of a child that only runs the two depth calls -> {kernel: calls, average us}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--config", a.config, "--splat", a.splat, "--reps", str(a.reps)]
        # its own process group: at the limit the profiler AND the child it started are killed, so nothing keeps the GPU open
        proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, start_new_session=True)
        try:
            _, err = proc.communicate(timeout=400)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            _, err = proc.communicate()
            raise RuntimeError("depth_bench: the kernel trace ran past 400 s and was killed:\n" + err.decode(errors="replace")[-2000:])
        if proc.returncode != 0:
            raise RuntimeError(f"depth_bench: the kernel trace failed (exit {proc.returncode}):\n" + err.decode(errors="replace")[-2000:])
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"].split("(")[0].replace("void ", "")
                if "k_blend_depth" in name or "k_ray_records" in name:
                    out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
    return out


def spread(xs, digits):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--max-blocks", type=int, default=131072, help="block pool of the fused volume (16^3 voxels, 64 KiB each)")
    ap.add_argument("--parent-lib", default=None, help="libgs2mesh_amd.so of the parent commit: its colour backward is timed too")
    ap.add_argument("--skip-pipeline", action="store_true", help="operator-level figures only")
    ap.add_argument("--splat", default="synth_v1", choices=("synth_v1", "trained_like"))
    ap.add_argument("--skip-backward", action="store_true", help="no backward figures")
    ap.add_argument("--surfel-mesh", action="store_true", help="fuse a flat-disc sphere from the centre and the ray median depth")
    ap.add_argument("--kernel-stats", action="store_true", help="per-kernel averages of the two depth calls from a profiler run")
    ap.add_argument("--child", action="store_true", help="(internal) only run the two depth calls, for the profiler")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_bench: no HIP device (there is no CPU path)")
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.depth_utils import RenderedDepth
    from gs2mesh_amd.rasterizer import Rasterizer
    from gs2mesh_amd.tsdf_utils import TSDF
    cfg = synthetic.CONFIGS[a.config]
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="depth_bench_")
    scene, model, cams = make_scene(cfg, a.views, root, "cuda:0", a.splat)
    W, H = cfg.width, cfg.height
    # ---- operator level: one view
    t = lambda x: torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    cam = cams[0]
    common = (t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center), torch.zeros(3, device=dev), W, H,
              cam.tanfovx, cam.tanfovy)
    with torch.no_grad():
        xyz, opac = model.get_xyz.contiguous(), model.get_opacity.reshape(-1).contiguous()
        kw = dict(shs=model.get_features.contiguous(), scales=model.get_scaling.contiguous(),
                  rotations=model.get_rotation.contiguous(), sh_degree=3)
    r = Rasterizer(0)
    fwd = lambda sync=False: r.forward(xyz, opac, *common, sync=sync, **kw)
    depth = lambda: r.depth_maps(W, H, like=xyz)
    fwd(sync=True)      # sizes the instance arena
    instances = int(r.last_num_rendered)
    for _ in range(3):
        fwd()
        depth()
    m = depth()
    torch.cuda.synchronize()
    covered = float((m["alpha"] >= 0.5).float().mean())
    if a.child:
        for _ in range(a.reps):
            depth()
            r.depth_maps_ray(xyz, kw["scales"], kw["rotations"], common[0], W, H, cam.tanfovx, cam.tanfovy, like=xyz)
        torch.cuda.synchronize()
        return
    t_fwd = [timed(fwd, a.reps) * 1e3 for _ in range(a.repeats)]
    t_depth = [timed(depth, a.reps) * 1e3 for _ in range(a.repeats)]
    t_one = [timed(lambda: r.depth_maps(W, H, want=("median",), like=xyz), a.reps) * 1e3 for _ in range(a.repeats)]
    # ---- the ray call next to the centre call on the same forward (and the parent's centre call on its own)
    ray = lambda: r.depth_maps_ray(xyz, kw["scales"], kw["rotations"], common[0], W, H, cam.tanfovx, cam.tanfovy, like=xyz)
    pairs = [("depth_pass_alt_us", depth), ("depth_ray_us", ray)]
    if a.parent_lib:
        import ctypes
        from gs2mesh_amd import _lib
        rp = Rasterizer(0, lib=_lib.bind(ctypes.CDLL(os.path.abspath(a.parent_lib)), require_all=False))
        rp.forward(xyz, opac, *common, sync=True, **kw)
        pairs.append(("depth_pass_parent_us", lambda: rp.depth_maps(W, H, like=xyz)))
        depth_same = all(torch.equal(x, y) for x, y in zip(depth().values(), rp.depth_maps(W, H, like=xyz).values()))
    mr = ray()
    ray_alpha_equal = bool(torch.equal(mr["alpha"], m["alpha"]))
    for _, fn in pairs:
        fn()
    t_ray = {name: [] for name, _ in pairs}
    for _ in range(2 * a.repeats):
        for name, fn in pairs:
            t_ray[name].append(timed(fn, a.reps) * 1e3)
    # ---- the backward pass: colour only (this commit, and the parent's library if given) and with the three map gradients
    gen = torch.Generator(device="cpu").manual_seed(0)
    g_pix = torch.rand((3, H, W), generator=gen).to(dev) - 0.5
    g_maps = [(torch.rand((H, W), generator=gen).to(dev) - 0.5) for _ in range(3)]
    bw = lambda rr: rr.backward(g_pix, xyz, *common, **kw)
    bw_depth = lambda rr=r, **more: rr.backward(g_pix, xyz, *common, grad_depth=g_maps[0], grad_median=g_maps[1],
                                                grad_alpha=g_maps[2], **more, **kw)
    runners = [("backward_us", lambda: bw(r)), ("backward_depth_us", bw_depth),
               ("backward_depth_ray_us", lambda: bw_depth(ray_depth=True))]
    if a.skip_backward:
        runners = []
    elif a.parent_lib:
        same = all(torch.equal(x, y) for x, y in zip(bw(r).values(), bw(rp).values()) if x is not None)
        runners.insert(1, ("backward_parent_us", lambda: bw(rp)))
        runners.insert(3, ("backward_parent_us", lambda: bw(rp)))    # this, parent, depth, parent, ray, parent's depth
        runners.append(("backward_depth_parent_us", lambda: bw_depth(rp)))
    fwd()
    for _, fn in runners:
        fn()
    t_bw = {name: [] for name, _ in runners}
    for _ in range(2 * a.repeats):
        for name, fn in runners:
            t_bw[name].append(timed(fn, max(a.reps // 5, 5)) * 1e3)
    rows, arena = r.backward_rows()
    res_ray = {name: spread(v, 1) for name, v in t_ray.items()}
    alt = t_ray["depth_pass_alt_us"]
    res_ray["depth_pass_same_code_spread"] = round(statistics.median(alt[::2]) / statistics.median(alt[1::2]), 4)
    res_ray["depth_ray_over_depth_pass"] = round(statistics.median(t_ray["depth_ray_us"]) / statistics.median(alt), 3)
    res_ray["ray_alpha_bits_equal"] = ray_alpha_equal
    if a.parent_lib:
        res_ray["depth_pass_over_parent"] = round(statistics.median(alt) / statistics.median(t_ray["depth_pass_parent_us"]), 4)
        res_ray["depth_pass_bits_equal_parent"] = bool(depth_same)
    # ---- pipeline level: RenderedDepth -> TSDF over the ring
    args = tsdf_args()

    def job():
        rd = RenderedDepth(root, scene, args)
        t0 = time.perf_counter()
        rd.run(keep_on_device=True, write_files=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        fuse = TSDF(scene, rd, args, "out", frame_source=rd.frame_source, max_blocks=a.max_blocks, fuse="batch")
        fuse.run()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, int(fuse.mesh.triangles.shape[0]), int(fuse.volume.num_blocks)

    res = dict(config=a.config, splat=a.splat, P=cfg.P, width=W, height=H, instances=instances, pixels_with_median=round(covered, 4),
               reps=a.reps, repeats=a.repeats, forward_us=spread(t_fwd, 1), depth_pass_us=spread(t_depth, 1),
               depth_pass_median_only_us=spread(t_one, 1),
               depth_over_forward=round(statistics.median(t_depth) / statistics.median(t_fwd), 3), views=a.views,
               backward_rows=rows, backward_arena_bytes=arena)
    res.update(res_ray)
    res.update({name: spread(v, 1) for name, v in t_bw.items()})
    if not a.skip_backward:
        half = t_bw["backward_us"]
        res["backward_same_code_spread"] = round(statistics.median(half[::2]) / statistics.median(half[1::2]), 4)
        res["backward_depth_over_backward"] = round(statistics.median(t_bw["backward_depth_us"]) / statistics.median(half), 3)
        res["backward_depth_ray_over_backward_depth"] = round(
            statistics.median(t_bw["backward_depth_ray_us"]) / statistics.median(t_bw["backward_depth_us"]), 3)
    if a.parent_lib and not a.skip_backward:
        res["backward_over_parent"] = round(statistics.median(half) / statistics.median(t_bw["backward_parent_us"]), 4)
        res["backward_bits_equal_parent"] = bool(same)
        res["backward_depth_over_parent"] = round(
            statistics.median(t_bw["backward_depth_us"]) / statistics.median(t_bw["backward_depth_parent_us"]), 4)
        res["backward_depth_ray_over_parent_backward_depth"] = round(
            statistics.median(t_bw["backward_depth_ray_us"]) / statistics.median(t_bw["backward_depth_parent_us"]), 3)
    try:
        if a.skip_pipeline:
            raise RuntimeError("skipped (--skip-pipeline)")
        job()           # warm-up: every shape of the timed window
        runs = [job() for _ in range(max(a.repeats, 1))]
        res.update(render_views_per_s=spread([a.views / x[0] for x in runs], 1),
                   fuse_views_per_s=spread([a.views / x[1] for x in runs], 1),
                   render_and_fuse_views_per_s=spread([a.views / (x[0] + x[1]) for x in runs], 1), triangles=runs[-1][2],
                   blocks=runs[-1][3], max_blocks=a.max_blocks)
    except RuntimeError as e:       # a volume overflow (raise --max-blocks) must not lose the operator-level figures
        res["pipeline_error"] = str(e)
    if a.kernel_stats:
        res["kernel_stats"] = kernel_stats(a)
    if a.surfel_mesh:
        res["surfel_sphere"] = surfel_mesh(torch, root)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
