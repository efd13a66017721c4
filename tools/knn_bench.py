"""Stream time of gs2m_knn_mean_dist2 (simple-knn's distCUDA2) on `synth_v1` centres, next to the only baseline that exists
on the same GPU: a chunked torch brute force (cdist + topk).

  * kernel, order = Morton (`rasterizer.morton_order`, prepared outside the timed window), P = 100 k and 1 M;
  * kernel, order = NULL (the points as they come: no box can cull), P = 100 k;
  * torch brute force, P = 100 k;
  * the Morton preparation itself, once per size, for scale.
Torch events around single calls after `--warmup` calls, `--repeats` rounds with the variants of one size interleaved; the
median and the range of every variant.  The kernel's output at the timed size is checked, untimed, against explicit f32
coordinate differences + topk; the difference to the cdist baseline is reported too.  One JSON line; --out also writes the table as text.

Usage:  python tools/knn_bench.py [--repeats 7] [--warmup 2] [--out profiles/knn.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gs2mesh_amd import synthetic  # noqa: E402
from gs2mesh_amd.rasterizer import morton_order  # noqa: E402
from gs2mesh_amd.simple_knn._C import knn_mean_dist2  # noqa: E402


def brute_force(x, chunk=4096):
    """mean of the three smallest squared distances to the other points, [chunk, P] distances at a time"""
    out = torch.empty(x.shape[0], device=x.device)
    for i0 in range(0, x.shape[0], chunk):
        d = torch.cdist(x[i0:i0 + chunk], x, compute_mode="donot_use_mm_for_euclid_dist")
        d = d * d
        idx = torch.arange(i0, min(i0 + chunk, x.shape[0]), device=x.device)
        d[idx - i0, idx] = float("inf")
        out[i0:i0 + chunk] = torch.topk(d, 3, dim=1, largest=False).values.sum(dim=1) / 3.0
    return out


def direct_differences(x, chunk=1024):
    """the same quantity from explicit coordinate differences, (dx*dx + dy*dy) + dz*dz in f32: the untimed check of the
    kernel's output at the sizes that are timed (cdist's own arithmetic is too coarse for near neighbours to serve as one)"""
    out = torch.empty(x.shape[0], device=x.device)
    for i0 in range(0, x.shape[0], chunk):
        q = x[i0:i0 + chunk]
        dx, dy, dz = (x[None, :, a] - q[:, None, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        idx = torch.arange(i0, i0 + q.shape[0], device=x.device)
        d[idx - i0, idx] = float("inf")
        b = torch.topk(d, 3, dim=1, largest=False, sorted=True).values
        out[i0:i0 + chunk] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / 3.0
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--brute-max", type=int, default=100_000, help="largest P the unsorted kernel and the brute force run at")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU: a CPU run gives no timing")
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "sizes": {}}
    for P in a.sizes:
        x = torch.from_numpy(synthetic.synth_v1(P, 1, -4.0)["xyz"]).cuda().contiguous()
        t_prep, order = timed(lambda: morton_order(x))
        t_prep, order = timed(lambda: morton_order(x))           # the second call: code loaded
        variants = {"kernel_morton": lambda: knn_mean_dist2(x, order)}
        if P <= a.brute_max:
            variants["kernel_unsorted"] = lambda: knn_mean_dist2(x, None)
            variants["torch_cdist_topk"] = lambda: brute_force(x)
        times = {k: [] for k in variants}
        outs = {}
        for r in range(a.warmup + a.repeats):
            for k, fn in variants.items():                       # interleaved: every round runs every variant once
                ms, outs[k] = timed(fn)
                if r >= a.warmup:
                    times[k].append(ms)
        row = {"morton_order_ms": t_prep}
        for k, t in times.items():
            row[k] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
        if "kernel_unsorted" in outs:
            row["unsorted_equals_morton_bitwise"] = bool(torch.equal(outs["kernel_unsorted"], outs["kernel_morton"]))
            rel = lambda t: float(((t - outs["kernel_morton"]).abs() / outs["kernel_morton"].clamp_min(1e-30)).max())
            row["torch_max_rel_diff"] = rel(outs["torch_cdist_topk"])
            direct = direct_differences(x)
            row["direct_max_rel_diff"] = rel(direct)
            row["direct_equal_bitwise"] = bool(torch.equal(direct, outs["kernel_morton"]))
        res["sizes"][str(P)] = row
    print(json.dumps(res))
    if a.out:
        lines = [f"gs2m_knn_mean_dist2 on synth_v1 centres, {res['device']}: stream time per call in ms, median [min, max] of "
                 f"{a.repeats} interleaved rounds after {a.warmup} warm-up rounds (tools/knn_bench.py)", ""]
        for P, row in res["sizes"].items():
            lines.append(f"P = {int(P):,}   (morton_order preparation, torch, outside the timed call: {row['morton_order_ms']:.2f} ms)")
            for k in ("kernel_morton", "kernel_unsorted", "torch_cdist_topk"):
                if k in row:
                    t = row[k]
                    lines.append(f"  {k:18s} {t['median_ms']:10.3f}  [{t['min_ms']:.3f}, {t['max_ms']:.3f}]")
            if "torch_max_rel_diff" in row:
                lines.append(f"  unsorted == morton bit for bit: {row['unsorted_equals_morton_bitwise']}")
                lines.append(f"  kernel vs explicit f32 coordinate differences + topk (untimed check): bit for bit "
                             f"{row['direct_equal_bitwise']}, max relative difference {row['direct_max_rel_diff']:.2e}")
                lines.append(f"  kernel vs the timed cdist + topk baseline: max relative difference {row['torch_max_rel_diff']:.2e} "
                             f"(cdist's distance arithmetic, not the kernel's)")
            lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
