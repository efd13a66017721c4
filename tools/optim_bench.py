"""Time the Adam step alone on the six tensors of a Gaussian model: optim.FusedAdam.step (one launch of gs2m_adam_step),
torch.optim.Adam.step, and the row-sparse step at 10 % and 30 % visible rows (rows chosen at random, and in contiguous
runs of 256 rows as a Morton-ordered model sees them).

    python tools/optim_bench.py [--sizes 100000 1000000 2000000] [--calls 30] [--warmup 10]

Stream time between torch events, median [min, max] over the calls after the warm-up calls, next to the traffic bound of a
dense step -- p, g, m, v read and p, m, v written: 28 B x 59 parameters x P (x the visible fraction for the sparse step) --
at the 6.29 TB/s copy rate BASELINE.md uses.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gs2mesh_amd.optim import FusedAdam  # noqa: E402

SHAPES = (("xyz", (3,), 0.00016), ("f_dc", (1, 3), 0.0025), ("f_rest", (15, 3), 0.000125), ("opacity", (1,), 0.05),
          ("scaling", (3,), 0.005), ("rotation", (4,), 0.001))
COPY_RATE = 6.29e12     # bytes / s
BYTES_PER_ROW = 28 * 59


def groups(P, gen):
    out = []
    for name, tail, lr in SHAPES:
        p = torch.nn.Parameter(torch.randn((P,) + tail, generator=gen, device="cuda"))
        p.grad = torch.randn((P,) + tail, generator=gen, device="cuda") * 1e-3
        out.append({"params": [p], "lr": lr, "name": name})
    return out


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def mask(P, fraction, contiguous, gen):
    if contiguous:
        runs = (P + 255) // 256
        pick = torch.rand(runs, generator=gen, device="cuda") < fraction
        return pick.repeat_interleave(256)[:P].to(torch.int32).contiguous()
    return (torch.rand(P, generator=gen, device="cuda") < fraction).to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000, 2_000_000])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a GPU")
    for P in a.sizes:
        gen = torch.Generator(device="cuda").manual_seed(P)
        fused = FusedAdam(groups(P, gen), lr=0.0, eps=1e-15)
        cases = [("fused", 1.0, fused.step)]
        for fraction in (0.1, 0.3):
            for contiguous in (False, True):
                vis = mask(P, fraction, contiguous, gen)
                seen = float(vis.sum()) / P
                cases.append((f"sparse {int(100 * fraction)} % {'contiguous' if contiguous else 'random'}", seen,
                              lambda vis=vis: fused.step(visible=vis)))
        for name, seen, fn in cases:
            med, lo, hi = timed(fn, a.calls, a.warmup)
            bound = 1e3 * BYTES_PER_ROW * P * seen / COPY_RATE
            print(json.dumps({"P": P, "step": name, "visible_fraction": round(seen, 4), "ms_median": round(med, 4),
                              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "traffic_bound_ms": round(bound, 4),
                              "fraction_of_bound": round(bound / med, 3)}), flush=True)
        del fused, cases
        torch.cuda.empty_cache()
        plain = torch.optim.Adam(groups(P, gen), lr=0.0, eps=1e-15)
        med, lo, hi = timed(plain.step, a.calls, a.warmup)
        bound = 1e3 * BYTES_PER_ROW * P / COPY_RATE
        print(json.dumps({"P": P, "step": "torch.optim.Adam", "visible_fraction": 1.0, "ms_median": round(med, 4),
                          "ms_min": round(lo, 4), "ms_max": round(hi, 4), "traffic_bound_ms": round(bound, 4),
                          "fraction_of_bound": round(bound / med, 3)}), flush=True)
        del plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
