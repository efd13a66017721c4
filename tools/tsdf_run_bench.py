"""TSDF.run on a C2-sized on-disk scene (1600 x 1200, `synthetic.write_tsdf_scene`, on tmpfs): fuse="frame" (the per-frame
loop) against fuse="batch" (prefetching loader, device masks, integrate_batch sweeps, device normals), alternating, and one
JSON line:

  frames_per_s            wall frames/s of each path's frame loop (selection, loading, masks, integration, up to status())
  batch_split_ms          batch path, per run: loader wait, mask call and integrate_batch call (host wall), extraction, normals
  per_frame_us            per frame: mask_kernels = stream time (hipEvents) of gs2m_mask_preprocess on one sweep of all views with
                          every buffer already on the device (the C call alone: its eight launches, no allocation), averaged
                          over back-to-back calls; sweep = the same for integrate_batch on the frames already on the device;
                          mask_call = the whole mask_preprocess wrapper (output allocation, launches) on device inputs;
                          upload = host -> device copy of one frame (image, depth, both masks)
  normals_ms              host numpy vs gs2m_mesh_vertex_normals on the extracted mesh (wall, incl. transfers)
  identical               volume (every block, every voxel) and mesh (canonical order: the vertex order follows the block
                          slots, which atomics hand out) of the two paths are equal; vertex normals to max_normal_diff

    python tools/tsdf_run_bench.py [--views 20|49] [--reps 3] [--tmp /dev/shm]   (the scene goes to a new directory there)
"""
import argparse
import copy
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from gs2mesh_amd import _lib, synthetic
from gs2mesh_amd.integration import Image, RGBDImage
from gs2mesh_amd.tsdf_utils import TSDF, mask_preprocess


def tsdf_args():
    return Namespace(stereo_model="DLNR_Middlebury", TSDF_scale=1.0, TSDF_dilate=1, TSDF_valid=None, TSDF_skip=None,
                     TSDF_use_occlusion_mask=True, TSDF_use_mask=True, TSDF_invert_mask=False, TSDF_erode_mask=True,
                     TSDF_erosion_kernel_size=10, TSDF_closing_kernel_size=10, TSDF_voxel=2, TSDF_sdf_trunc=0.04,
                     TSDF_min_depth_baselines=4, TSDF_max_depth_baselines=20, TSDF_cleaning_threshold=100000)


def canonical(m):
    order = np.argsort(m.edge_index.view([("", np.int32)] * 4).reshape(-1))
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    tri = rank[m.triangles]
    t_order = np.lexsort(tri.T[::-1])
    return [m.vertices[order], m.vertex_colors[order], m.edge_index[order], tri[t_order], m.triangle_normals[t_order]], \
        m.vertex_normals[order]


def same(a, b):
    ka, *va = a.volume.download()
    kb, *vb = b.volume.download()
    oa, ob = np.lexsort(ka.T[::-1]), np.lexsort(kb.T[::-1])
    ok = np.array_equal(ka[oa], kb[ob]) and all(np.array_equal(x[oa], y[ob]) for x, y in zip(va, vb))
    (ca, na), (cb, nb) = canonical(a.mesh), canonical(b.mesh)
    ok = ok and all(np.array_equal(x, y) for x, y in zip(ca, cb))
    return bool(ok), float(np.abs(na - nb).max()) if na.shape == nb.shape and na.size else None


def stream_us(fn, calls=10, reps=5, setup=None):
    """stream time of one fn() (hipEvents around `calls` back-to-back calls, median of reps), microseconds"""
    fn()
    ts = []
    for _ in range(reps):
        if setup is not None:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / calls)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the scene's own new directory is made (tmpfs by default)")
    a = ap.parse_args()
    cfg = synthetic.CONFIGS["C2"]
    out = tempfile.mkdtemp(prefix="tsdf_run_bench_", dir=a.tmp)      # removed afterwards: only what this run made
    stereo = Namespace(model_name="DLNR_Middlebury")
    args = tsdf_args()
    fps = {"frame": [], "batch": []}
    split = {k: [] for k in ("load_wait", "mask", "integrate", "extract", "normals")}
    last = {}
    try:
        scene = synthetic.write_tsdf_scene(out, a.views, cfg.width, cfg.height, cfg.focal, seed=a.seed)
        for _ in range(a.reps):
            for fuse in ("frame", "batch"):
                last.pop(fuse, None)
                t = TSDF(scene, stereo, args, "out", max_blocks=16384, fuse=fuse)
                t.run()
                fps[fuse].append(a.views / t.timings["fuse"])
                if fuse == "batch":
                    for k in split:
                        split[k].append(t.timings[k] * 1000.0)
                last[fuse] = t
        identical, max_normal_diff = same(last["frame"], last["batch"])

        # stream time of the two calls of one sweep of every view (buffers on the device), and the upload of one frame
        frames = [last["batch"]._load_frame(i) for i in range(a.views)]
        objs = [torch.from_numpy(f["mask"].view(np.uint8)).cuda() for f in frames]
        occs = [torch.from_numpy(f["occlusion"].view(np.uint8)).cuda() for f in frames]
        n, Wd, Hd = a.views, cfg.width, cfg.height
        outs = torch.empty((n, Hd, Wd), dtype=torch.uint8, device="cuda")
        scratch = torch.empty((2 * n * Hd * ((Wd + 63) // 64),), dtype=torch.int64, device="cuda")
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        obj_p, occ_p, out_p = arr(objs), arr(occs), arr([outs[i] for i in range(n)])
        lib = _lib.get()
        st = _lib.MEMORY.current_stream(0)
        call = lambda: _lib.check(lib.gs2m_mask_preprocess(n, Wd, Hd, obj_p, occ_p, 0, 1, 10, 10, out_p, C.c_void_p(scratch.data_ptr()),
                                                           st), lib)
        mask_kernels_us = stream_us(call) / n
        mask_call_us = stream_us(lambda: mask_preprocess(objs, occs, False, True, 10, 10)) / n
        masks = mask_preprocess(objs, occs, False, True, 10, 10)
        assert torch.equal(torch.stack(masks), outs)
        tb = last["batch"]
        imgs = [RGBDImage.create_from_color_and_depth(Image(torch.from_numpy(f["image"]).cuda()), Image(torch.from_numpy(f["depth"]).cuda()),
                                                      depth_scale=1.0, depth_trunc=scene.baseline * 20, convert_rgb_to_intensity=False)
                for f in frames]
        exts = [tb._world_to_camera(i) for i in range(a.views)]
        intr = tb._intrinsic(0)
        vol_args = dict(voxel_length=args.TSDF_voxel / 512, sdf_trunc=args.TSDF_sdf_trunc, max_blocks=16384)
        from gs2mesh_amd.integration import ScalableTSDFVolume

        vol = ScalableTSDFVolume(**vol_args)
        sweep_us = stream_us(lambda: vol.integrate_batch(imgs, intr, exts, masks=masks, min_depth=4 * scene.baseline), calls=1,
                             setup=lambda: (vol.reset(), torch.cuda.synchronize())) / n
        up = []
        for f in frames[:5]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for key, dt in (("image", torch.uint8), ("depth", torch.float32), ("mask", torch.uint8), ("occlusion", torch.uint8)):
                x = f[key].view(np.uint8) if f[key].dtype == np.bool_ else f[key]
                _lib.MEMORY.upload(x, dt, 0)
            torch.cuda.synchronize()
            up.append((time.perf_counter() - t0) * 1e6)

        m = last["batch"].mesh
        host_ms, dev_ms = [], []
        for _ in range(3):
            h = copy.deepcopy(m)
            t0 = time.perf_counter()
            h.compute_vertex_normals()
            host_ms.append((time.perf_counter() - t0) * 1000.0)
            t0 = time.perf_counter()
            m.compute_vertex_normals(on_device=True)
            dev_ms.append((time.perf_counter() - t0) * 1000.0)
        normals_equal = bool(np.array_equal(h.vertex_normals, m.vertex_normals) and np.array_equal(h.triangle_normals, m.triangle_normals))
    finally:
        shutil.rmtree(out, ignore_errors=True)

    med = lambda x: round(statistics.median(x), 3)
    spread = lambda x: [round(min(x), 3), round(max(x), 3)]
    print(json.dumps(dict(
        tool="tsdf_run_bench", views=a.views, width=cfg.width, height=cfg.height, reps=a.reps,
        loader_threads=min(TSDF.LOADER_THREADS, len(os.sched_getaffinity(0))), max_sweep=TSDF.MAX_SWEEP,
        frames_per_s={k: med(v) for k, v in fps.items()}, frames_per_s_range={k: spread(v) for k, v in fps.items()},
        speedup=round(statistics.median(fps["batch"]) / statistics.median(fps["frame"]), 2),
        batch_split_ms={k: med(v) for k, v in split.items()},
        per_frame_us=dict(mask_kernels=round(mask_kernels_us, 2), sweep=round(sweep_us, 2), mask_call=round(mask_call_us, 2),
                          upload=round(statistics.median(up), 1)),
        mesh=dict(vertices=int(m.vertices.shape[0]), triangles=int(m.triangles.shape[0])),
        normals_ms=dict(host=med(host_ms), device=med(dev_ms), host_range=spread(host_ms), device_range=spread(dev_ms),
                        speedup=round(statistics.median(host_ms) / statistics.median(dev_ms), 1), equal_host=normals_equal),
        identical=identical, max_normal_diff=max_normal_diff)))


if __name__ == "__main__":
    main()
