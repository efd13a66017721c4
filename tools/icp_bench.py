"""Time of one ICP iteration and of a whole registration (gs2mesh_amd.evaluation.registration_icp on gs2m_icp_prepare /
gs2m_icp_step) next to a host restatement on scipy's cKDTree, on the same points in the same run, at two sizes:

  * "mobilebrick": 200 k x 200 k points, rigid, threshold 0.02, 10 iterations (evaluate.py:82-93 on mesh vertices);
  * "tnt": 4 M x 4 M points, with scaling, threshold 2 tau = 0.006, 20 iterations (the last stage of run.py:98-102).
Points: two independent samples of a noisy sphere shell (radius 1, radial noise 0.002), the source moved by a small similarity.

Per size, stream time by torch events, median [min, max] of --repeats rounds after --warmup, the variants interleaved:
  * prepare             gs2m_icp_prepare (once per registration);
  * icp_step            one gs2m_icp_step with both Morton orders (prepared outside, reported);
  * nn_plus_torch_sums  the same iteration from separate pieces: the transform in torch, evaluation.nearest_neighbors (which
                        builds the target's structure again, as every call of it does) and torch gathers / sums of the moments.
Wall time (perf_counter, the call ends in a device-to-host copy): registration_icp as a whole, and its iterations.
Host: cKDTree build, one iteration (query with workers=16, f64 moments, Umeyama) --host-iterations times, and -- at sizes up to
--host-full-max -- the whole loop.  The two results are compared, untimed.
Also gs2m_voxel_mean inside evaluation.voxel_down_sample at 4 M points: the kernel alone by events next to the whole call.
One JSON line; --out also writes the table as text.

Usage:  python tools/icp_bench.py [--repeats 5] [--warmup 1] [--out profiles/icp.txt]
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

SIZES = {"mobilebrick": dict(n=200_000, threshold=0.02, scaling=False, iterations=10),
         "tnt": dict(n=4_000_000, threshold=0.006, scaling=True, iterations=20)}


def shell(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (1 + rng.normal(0, 0.002, (n, 1)))


def perturbation(scaling):
    a = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = (1.001 if scaling else 1.0) * (np.eye(3) + np.sin(0.002) * K + (1 - np.cos(0.002)) * (K @ K))
    T[:3, 3] = [0.001, -0.002, 0.0015]
    return T


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def host_iteration(tree, s, t, T, max_dist, scaling):
    p = s @ T[:3, :3].T + T[:3, 3]
    d, j = tree.query(p, workers=16)
    k = d < max_dist
    n = int(k.sum())
    return evaluation.umeyama(p[k], t[j[k]], scaling) @ T, n / len(s), float(np.sqrt((d[k] ** 2).mean())) if n else 0.0


def host_registration(tree, s, t, max_dist, scaling, iterations):
    """the loop of evaluation.icp_loop on the tree: an evaluation costs a query, an update the moments"""
    T = np.eye(4)
    p = s.copy()
    d, j = tree.query(p, workers=16)
    k = d < max_dist
    fit, rmse, done = k.mean(), float(np.sqrt((d[k] ** 2).mean())) if k.any() else 0.0, 0
    for _ in range(iterations):
        T = evaluation.umeyama(p[k], t[j[k]], scaling) @ T
        p = s @ T[:3, :3].T + T[:3, 3]
        done += 1
        before = (fit, rmse)
        d, j = tree.query(p, workers=16)
        k = d < max_dist
        fit, rmse = k.mean(), float(np.sqrt((d[k] ** 2).mean())) if k.any() else 0.0
        if abs(before[0] - fit) < 1e-6 and abs(before[1] - rmse) < 1e-6:
            break
    return T, done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-iterations", type=int, default=2)
    ap.add_argument("--host-full-max", type=int, default=200_000, help="largest size the whole host loop runs at")
    ap.add_argument("--sizes", nargs="*", default=list(SIZES))
    ap.add_argument("--voxel-points", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench needs a GPU: a CPU run gives no timing")
    from scipy.spatial import cKDTree
    lib = _lib.get()
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "host_workers": 16, "sizes": {}}
    for name in a.sizes:
        cfg = SIZES[name]
        n, thr, scaling = cfg["n"], cfg["threshold"], cfg["scaling"]
        P = perturbation(scaling)
        ht = shell(n, 2)
        hs = shell(n, 1)
        Pi = np.linalg.inv(P)
        hs = hs @ Pi[:3, :3].T + Pi[:3, 3]                            # P moves the source back onto the target's shell
        s, t = torch.from_numpy(hs).cuda(), torch.from_numpy(ht).cuda()
        o_t = (t.amin(dim=0) + t.amax(dim=0)) / 2
        o = np.ascontiguousarray(o_t.cpu().numpy())
        timed(lambda: (morton_order((s - o_t).float()), morton_order((t - o_t).float())))
        t_orders, (qo, ro) = timed(lambda: (morton_order((s - o_t).float()), morton_order((t - o_t).float())))
        need = int(lib.gs2m_icp_scratch_bytes(n, n))
        scratch = torch.empty((need // 8 + 2,), dtype=torch.int64, device="cuda")
        sums = torch.zeros(_lib.ICP_SUMS, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        T0 = np.eye(4)
        o_ptr, T_ptr = o.ctypes.data_as(_lib.vp), T0.ctypes.data_as(_lib.vp)

        def prepare():
            _lib.check(lib.gs2m_icp_prepare(n, _ptr(t), o_ptr, _ptr(ro), _ptr(scratch), scratch.shape[0] * 8, stream), lib)

        def step():
            _lib.check(lib.gs2m_icp_step(n, _ptr(s), _ptr(qo), T_ptr, n, _ptr(t), o_ptr, thr, _ptr(scratch), scratch.shape[0] * 8,
                                         _ptr(sums), None, None, stream), lib)
            return sums.clone()

        M = torch.from_numpy(T0).cuda()

        def pieces():
            p = s @ M[:3, :3].T + M[:3, 3]
            d2f, idx = evaluation.nearest_neighbors((p - o_t).float(), (t - o_t).float(), sort=True)
            q = t[idx.long()]
            d2 = ((p - q) ** 2).sum(dim=1)
            k = d2 < thr * thr
            a_, b_ = (p - o_t)[k], (q - o_t)[k]
            return k.sum(), d2[k].sum(), a_.sum(dim=0), b_.sum(dim=0), a_.T @ b_, (a_ * a_).sum()

        variants = {"prepare": prepare, "icp_step": step, "nn_plus_torch_sums": pieces}
        times = {k: [] for k in variants}
        outs = {}
        for rnd in range(a.warmup + a.repeats):
            for k, fn in variants.items():                            # interleaved: every round runs every variant once
                ms, outs[k] = timed(fn)
                if rnd >= a.warmup:
                    times[k].append(ms)
        row = {"N": n, "R": n, "threshold": thr, "with_scaling": scaling, "morton_orders_ms": t_orders}
        for k, tt in times.items():
            row[k] = stats(tt)
        kept = int(outs["icp_step"][0].item())
        row["pairs_kept_at_identity"] = kept
        row["pairs_kept_by_the_pieces"] = int(outs["nn_plus_torch_sums"][0].item())

        reg = []
        for rnd in range(a.warmup + min(a.repeats, 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = evaluation.registration_icp(s, t, thr, with_scaling=scaling, max_iteration=cfg["iterations"])
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                reg.append((time.perf_counter() - t0) * 1e3)
        row["registration_icp_wall"] = stats(reg)
        row["registration_icp_iterations"] = r.n_iterations
        row["registration_icp_fitness"] = r.fitness
        row["registration_icp_rmse"] = r.inlier_rmse

        t0 = time.perf_counter()
        tree = cKDTree(ht)
        row["ckdtree_build_ms"] = (time.perf_counter() - t0) * 1e3
        host = []
        for _ in range(a.host_iterations):
            t0 = time.perf_counter()
            host_iteration(tree, hs, ht, T0, thr, scaling)
            host.append((time.perf_counter() - t0) * 1e3)
        row["host_iteration_workers16"] = stats(host)
        if n <= a.host_full_max:
            t0 = time.perf_counter()
            Th, done = host_registration(tree, hs, ht, thr, scaling, cfg["iterations"])
            row["host_registration_wall_ms"] = (time.perf_counter() - t0) * 1e3
            row["host_registration_iterations"] = done
            row["max_abs_diff_to_host_T"] = float(np.abs(r.transformation - Th).max())
        row["max_abs_diff_to_perturbation"] = float(np.abs(r.transformation - P).max())
        res["sizes"][name] = row
        del tree, s, t, scratch

    n = a.voxel_points
    pts = torch.from_numpy(shell(n, 3)).cuda()
    voxel = 0.004
    whole, kern = [], []
    real = lib.gs2m_voxel_mean
    for rnd in range(a.warmup + a.repeats):
        box = {}

        class Timed:                                                  # the library with the one call wrapped in events
            def __getattr__(self, k):
                return getattr(lib, k)

            def gs2m_voxel_mean(self, *args):
                box["ms"], rc = timed(lambda: real(*args))
                return rc
        ms, out = timed(lambda: evaluation.voxel_down_sample(pts, voxel, lib=Timed()))
        if rnd >= a.warmup:
            whole.append(ms)
            kern.append(box["ms"])
    S = int(out.shape[0])
    res["voxel"] = {"points": n, "voxel_size": voxel, "voxels": S, "voxel_down_sample": stats(whole), "gs2m_voxel_mean": stats(kern),
                    "kernel_bytes": n * 28 + S * 28}
    res["voxel"]["kernel_GBps"] = res["voxel"]["kernel_bytes"] / (res["voxel"]["gs2m_voxel_mean"]["median_ms"] * 1e-3) / 1e9
    print(json.dumps(res))
    if a.out:
        fmt = lambda t: f"{t['median_ms']:12.3f}  [{t['min_ms']:.3f}, {t['max_ms']:.3f}]"
        lines = [f"ICP on two samples of a noisy sphere shell, {res['device']}: stream time per call in ms, median [min, max] of {a.repeats} "
                 f"interleaved rounds after {a.warmup} warm-up round(s); wall times by perf_counter in the same run (tools/icp_bench.py)", ""]
        for name, row in res["sizes"].items():
            lines.append(f"{name}: N = R = {row['N']:,}, threshold {row['threshold']}, with_scaling {row['with_scaling']}   (Morton orders of both "
                         f"sides, torch, outside the timed calls: {row['morton_orders_ms']:.2f} ms; cKDTree build: {row['ckdtree_build_ms']:.0f} ms)")
            for k in ("prepare", "icp_step", "nn_plus_torch_sums", "host_iteration_workers16", "registration_icp_wall"):
                lines.append(f"  {k:26s} {fmt(row[k])}")
            lines.append(f"  registration_icp: {row['registration_icp_iterations']} iterations, fitness {row['registration_icp_fitness']:.6f}, rmse "
                         f"{row['registration_icp_rmse']:.3e}, max|T - perturbation| {row['max_abs_diff_to_perturbation']:.3e}")
            lines.append(f"  pairs kept at the identity: {row['pairs_kept_at_identity']:,} (kernel), {row['pairs_kept_by_the_pieces']:,} (pieces)")
            if "host_registration_wall_ms" in row:
                lines.append(f"  host registration: {row['host_registration_wall_ms']:.0f} ms wall, {row['host_registration_iterations']} iterations, "
                             f"max|T - T_host| {row['max_abs_diff_to_host_T']:.3e}")
            else:
                lines.append("  host registration: not run at this size")
            lines.append("")
        v = res["voxel"]
        lines.append(f"voxel_down_sample of {v['points']:,} points at {v['voxel_size']} -> {v['voxels']:,} voxels")
        lines.append(f"  {'voxel_down_sample (whole)':26s} {fmt(v['voxel_down_sample'])}")
        lines.append(f"  {'gs2m_voxel_mean (inside)':26s} {fmt(v['gs2m_voxel_mean'])}   {v['kernel_GBps']:.0f} GB/s of the {v['kernel_bytes']:,} bytes it must move")
        lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
