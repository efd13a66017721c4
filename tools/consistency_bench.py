"""Stream time of gs2m_depth_consistency on a C2 shape next to the sweep it feeds, in the same run.

  * 49 ring views of 1600 x 1200 (synthetic.CONFIGS["C2"]), depths from sphere_depth_torch on the device, K = 4 sources per
    view from select_sources.  The C entry point is called with prebuilt descriptor arrays (what depth_utils.consistency_votes
    passes), so the timed window holds the call's 25 launches and nothing of Python's.  Torch (hip) events around single calls:
    median [min, max] of --repeats calls after --warmup, per call and per reference view.
  * Achieved bytes/s against the traffic model of the kernel: per VALID reference pixel 4 bytes of its own depth, 4 bytes
    gathered from each of its K_used sources and the bytes of the outputs asked for (keep alone: 1; keep and the three counts:
    4).  Invalid pixels (here: the background, 0) cost their own read and write and are left out of the model, which therefore
    understates the traffic a little.  The share is against the 6.29 TB/s copy rate of BASELINE.md.
  * integrate_batch over the same 49 depth maps (bench.py's sweeps: 25 + 24 frames, RGB8 volume), events around the sweeps,
    per frame: what one view of the stage costs next to one view of the fusion.
One JSON line; --out also writes text.

Usage:  python tools/consistency_bench.py [--repeats 20] [--warmup 3] [--out profiles/depth_consistency.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs2mesh_amd import _lib, synthetic  # noqa: E402
from gs2mesh_amd.depth_utils import pair_matrices, select_sources  # noqa: E402
from gs2mesh_amd.integration import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume  # noqa: E402

COPY_RATE = 6.29e12
K = 4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def repeat(fn, warmup, repeats):
    t = [timed(fn) for _ in range(warmup + repeats)][warmup:]
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench needs a GPU: a CPU run gives no timing")
    if a.repeats < 20 or a.warmup < 3:
        raise SystemExit("at least 3 warm-up and 20 timed calls")
    cfg = synthetic.CONFIGS[a.config]
    W, H, n = cfg.width, cfg.height, cfg.n_pairs
    dev = torch.device("cuda:0")
    lib = _lib.get()
    stream = torch.cuda.current_stream().cuda_stream
    poses = synthetic.ring_poses(n, cfg.ring_radius)
    depths = [synthetic.sphere_depth_torch(p, W, H, cfg.focal, cfg.focal, W / 2, H / 2, cfg.sphere_radius, dev) for p in poses]
    w2c = []
    for p in poses:
        E = np.eye(4)
        E[:3] = p
        w2c.append(E)
    c2w = np.stack([np.linalg.inv(E) for E in w2c])
    sources = select_sources(c2w, K)
    pair = pair_matrices(c2w, sources)
    k_used = (sources >= 0).sum(axis=1)
    min_depth, max_depth = cfg.baseline * 4, cfg.baseline * 20
    valid = [int(((d > 0) & (d >= min_depth) & (d < max_depth)).sum().item()) for d in depths]
    views = (_lib.DepthView * n)(*[_lib.DepthView(d.data_ptr(), None, W, H, cfg.focal, cfg.focal, W / 2, H / 2) for d in depths])
    out = {name: torch.empty((n, H, W), dtype=torch.uint8, device=dev) for name in ("keep", "support", "violation", "occluded")}
    arr = {name: (C.c_void_p * n)(*[t.data_ptr() + i * H * W for i in range(n)]) for name, t in out.items()}
    src_p, pair_p = sources.ctypes.data_as(C.POINTER(C.c_int32)), pair.ctypes.data_as(C.POINTER(C.c_float))

    def call(counts):
        _lib.check(lib.gs2m_depth_consistency(n, views, K, src_p, pair_p, 0.01, min_depth, max_depth, 2, 1, arr["keep"],
                                              arr["support"] if counts else None, arr["violation"] if counts else None,
                                              arr["occluded"] if counts else None, stream), lib)

    res = {"device": torch.cuda.get_device_name(0), "config": a.config, "views": n, "size": [W, H], "K": K,
           "k_used_mean": float(k_used.mean()), "valid_pixels_per_view": sum(valid) / n, "repeats": a.repeats, "warmup": a.warmup,
           "consistency": {}}
    for label, counts, out_bytes in (("keep", False, 1), ("keep_and_counts", True, 4)):
        row = repeat(lambda: call(counts), a.warmup, a.repeats)
        traffic = sum(v * (4 + 4 * int(k) + out_bytes) for v, k in zip(valid, k_used))
        row.update(per_view_us=1e3 * row["median_ms"] / n, traffic_bytes=traffic,
                   achieved_bytes_per_s=traffic / (row["median_ms"] * 1e-3))
        row["share_of_copy_rate"] = row["achieved_bytes_per_s"] / COPY_RATE
        res["consistency"][label] = row
    kept = int(out["keep"].sum().item())
    res["kept_of_valid"] = kept / max(sum(valid), 1)

    # ---- the sweep it feeds ----------------------------------------------------------------------------------------------
    col = torch.from_numpy(synthetic.color_pattern(W, H)).to(dev)
    vol = ScalableTSDFVolume(cfg.voxel_length, cfg.sdf_trunc, max_blocks=(cfg.tsdf_n // 16) ** 3)
    intr = PinholeCameraIntrinsic(W, H, cfg.focal, cfg.focal, W / 2, H / 2)
    size = -(-n // -(-n // 32))
    sweeps = [list(range(i, min(n, i + size))) for i in range(0, n, size)]

    def fuse():
        for idx in sweeps:
            vol.integrate_batch([RGBDImage(col, depths[k], depth_scale=1.0, depth_trunc=max_depth) for k in idx], intr,
                                [w2c[k] for k in idx], min_depth=min_depth)

    t = []
    for rnd in range(1 + 5):
        ms = timed(fuse)
        vol.status()
        vol.reset()
        if rnd >= 1:
            t.append(ms)
    res["integrate_batch"] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                              "per_frame_us": 1e3 * statistics.median(t) / n, "sweeps": [len(s) for s in sweeps], "runs": len(t)}
    print(json.dumps(res))
    if a.out:
        fmt = lambda r: f"{r['median_ms']:9.3f}  [{r['min_ms']:.3f}, {r['max_ms']:.3f}]"
        lines = [f"gs2m_depth_consistency, {res['device']}: stream time per call in ms, median [min, max] of {a.repeats} calls after "
                 f"{a.warmup} warm-ups (tools/consistency_bench.py)", "",
                 f"{a.config}: {n} ring views of {W} x {H}, K = {K} (sources used per view: {res['k_used_mean']:.2f}), "
                 f"{res['valid_pixels_per_view']:,.0f} valid pixels per view, kept {res['kept_of_valid']:.4f} of them"]
        for label, text in (("keep", "keep alone"), ("keep_and_counts", "keep + 3 counts")):
            r = res["consistency"][label]
            lines.append(f"  {text:16s} {fmt(r)}   {r['per_view_us']:.1f} us per reference view;  traffic model {r['traffic_bytes'] / 1e6:.1f} MB -> "
                         f"{r['achieved_bytes_per_s'] / 1e12:.3f} TB/s = {r['share_of_copy_rate']:.3f} of the 6.29 TB/s copy rate")
        ib = res["integrate_batch"]
        lines += ["", f"integrate_batch on the same {n} depth maps (sweeps of {ib['sweeps']}, RGB8), events around the sweeps, {ib['runs']} runs "
                  f"after 1 warm-up: {fmt(ib)}   {ib['per_frame_us']:.1f} us per frame", ""]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
