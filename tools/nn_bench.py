"""Stream time of gs2m_nn_dist2 (the nearest neighbour of every query in another point set: the hot path of the DTU,
MobileBrick and TNT mesh metrics) next to the host baseline the reference's evaluators use, on the same points in the same run.

  * points: two independent samples of a noisy sphere shell (radius 1, radial noise 0.002) -- surface-like, as the sets a mesh
    evaluation compares; Q = R = 1 M and 4 M;
  * kernel with the Morton orders of both sides (`rasterizer.morton_order`, prepared outside the timed window, reported);
  * kernel with order = NULL on both sides (no box can cull: the brute force), up to --unsorted-max;
  * scipy.spatial.cKDTree(refs).query(queries, workers=16): the query alone, the build reported next to it;
  * gs2m_mesh_sample_count + _emit (evaluation.sample_mesh, with its one synchronisation) on a mesh of about 1 M triangles.
Torch events around single calls after `--warmup` rounds, `--repeats` rounds with the kernel variants of one size interleaved;
the host query is timed with perf_counter `--host-repeats` times between them.  Median [min, max] of every variant.  The
kernel's output is checked, untimed, against the tree's.  One JSON line; --out also writes the table as text.

Usage:  python tools/nn_bench.py [--repeats 5] [--warmup 1] [--out profiles/nn.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs2mesh_amd import _lib, evaluation  # noqa: E402
from gs2mesh_amd._lib import _ptr  # noqa: E402
from gs2mesh_amd.rasterizer import morton_order  # noqa: E402


def shell(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (1 + rng.normal(0, 0.002, (n, 1)))).astype(np.float32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 4_000_000])
    ap.add_argument("--unsorted-max", type=int, default=4_000_000, help="largest Q = R the unsorted kernel runs at")
    ap.add_argument("--mesh-side", type=int, default=708, help="the sampled mesh is a side x side grid: 2 (side - 1)^2 triangles")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_bench needs a GPU: a CPU run gives no timing")
    from scipy.spatial import cKDTree
    lib = _lib.get()
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "host_repeats": a.host_repeats,
           "host_workers": 16, "sizes": {}}
    for n in a.sizes:
        hq, hr = shell(n, 1), shell(n, 2)
        q, r = torch.from_numpy(hq).cuda(), torch.from_numpy(hr).cuda()
        timed(lambda: (morton_order(q), morton_order(r)))
        t_prep, (qo, ro) = timed(lambda: (morton_order(q), morton_order(r)))      # the second call: code loaded
        scratch = torch.empty((int(lib.gs2m_nn_scratch_bytes(n, n)) // 8 + 2,), dtype=torch.int64, device="cuda")
        d2, idx = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def kernel(o1, o2):
            _lib.check(lib.gs2m_nn_dist2(n, _ptr(q), _ptr(o1), n, _ptr(r), _ptr(o2), _ptr(scratch), scratch.shape[0] * 8, _ptr(d2),
                                         _ptr(idx), stream), lib)
            return d2.clone(), idx.clone()
        variants = {"kernel_morton": lambda: kernel(qo, ro)}
        if n <= a.unsorted_max:
            variants["kernel_unsorted"] = lambda: kernel(None, None)
        t0 = time.perf_counter()
        tree = cKDTree(hr.astype(np.float64))
        t_build = (time.perf_counter() - t0) * 1e3
        hq64 = hq.astype(np.float64)
        times = {k: [] for k in variants}
        host, outs, kd = [], {}, None
        for rnd in range(a.warmup + a.repeats):
            for k, fn in variants.items():                       # interleaved: every round runs every variant once
                ms, outs[k] = timed(fn)
                if rnd >= a.warmup:
                    times[k].append(ms)
            if len(host) < a.host_repeats:
                t0 = time.perf_counter()
                kd = tree.query(hq64, workers=16)
                host.append((time.perf_counter() - t0) * 1e3)
        row = {"morton_order_ms": t_prep, "ckdtree_build_ms": t_build, "ckdtree_query_workers16": stats(host)}
        for k, t in times.items():
            row[k] = stats(t)
        got = outs["kernel_morton"][0].cpu().numpy().astype(np.float64)
        row["max_rel_diff_to_ckdtree_d2"] = float(np.max(np.abs(got - kd[0] ** 2) / np.maximum(kd[0] ** 2, 1e-30)))
        row["index_differs_from_ckdtree"] = int(np.count_nonzero(outs["kernel_morton"][1].cpu().numpy() != kd[1]))
        if "kernel_unsorted" in outs:
            row["unsorted_equals_morton_bitwise"] = bool(torch.equal(outs["kernel_unsorted"][0], outs["kernel_morton"][0]) and
                                                         torch.equal(outs["kernel_unsorted"][1], outs["kernel_morton"][1]))
        res["sizes"][str(n)] = row
        del tree, kd, q, r, scratch

    s = a.mesh_side
    x, y = np.meshgrid(np.arange(s, dtype=np.float64), np.arange(s, dtype=np.float64), indexing="ij")
    verts = np.stack([x, y, np.sin(x / 9) + np.cos(y / 11)], -1).reshape(-1, 3)
    i = (np.arange(s - 1)[:, None] * s + np.arange(s - 1)[None, :]).reshape(-1)
    tris = np.concatenate([np.stack([i, i + s, i + s + 1], 1), np.stack([i, i + s + 1, i + 1], 1)]).astype(np.int32)
    dv, dt = torch.from_numpy(verts).cuda(), torch.from_numpy(tris).cuda()
    t = []
    for rnd in range(a.warmup + a.repeats):
        ms, pts = timed(lambda: evaluation.sample_mesh((dv, dt), 0.2))
        if rnd >= a.warmup:
            t.append(ms)
    res["sampler"] = {"triangles": int(tris.shape[0]), "vertices": int(verts.shape[0]), "density": 0.2, "points": int(pts.shape[0]),
                      "count_emit": stats(t)}
    print(json.dumps(res))
    if a.out:
        fmt = lambda t: f"{t['median_ms']:12.3f}  [{t['min_ms']:.3f}, {t['max_ms']:.3f}]"
        lines = [f"gs2m_nn_dist2 on two samples of a noisy sphere shell, {res['device']}: stream time per call in ms, median [min, max] of "
                 f"{a.repeats} interleaved rounds after {a.warmup} warm-up round(s); the host query: wall time of {a.host_repeats} calls in "
                 f"the same run (tools/nn_bench.py)", ""]
        for n, row in res["sizes"].items():
            lines.append(f"Q = R = {int(n):,}   (morton_order of both sides, torch, outside the timed call: {row['morton_order_ms']:.2f} ms; "
                         f"cKDTree build, outside the timed call: {row['ckdtree_build_ms']:.0f} ms)")
            for k in ("kernel_morton", "kernel_unsorted", "ckdtree_query_workers16"):
                if k in row:
                    lines.append(f"  {k:24s} {fmt(row[k])}")
            if "unsorted_equals_morton_bitwise" in row:
                lines.append(f"  unsorted == morton bit for bit, distance and index: {row['unsorted_equals_morton_bitwise']}")
            lines.append(f"  kernel d2 (f32 arithmetic) vs cKDTree distance^2 (f64): max relative difference {row['max_rel_diff_to_ckdtree_d2']:.2e}; "
                         f"indices that differ: {row['index_differs_from_ckdtree']}")
            lines.append("")
        sm = res["sampler"]
        lines.append(f"gs2m_mesh_sample_count + _emit (evaluation.sample_mesh, one synchronisation inside): {sm['triangles']:,} triangles, "
                     f"{sm['vertices']:,} vertices, density {sm['density']} -> {sm['points']:,} points")
        lines.append(f"  {'count_emit':24s} {fmt(sm['count_emit'])}")
        lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
