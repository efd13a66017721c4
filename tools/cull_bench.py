"""Stream time of the two kernels of the DTU cull (evaluation.dtu_cull, the reference's cull_scan) next to the host arithmetic
the reference runs, on the same data in the same run.

  * gs2m_mask_dilate_disk: 49 and 64 masks of 1600 x 1200 (the sizes of a DTU scan) at r = 24, bitmaps only.  Yardstick:
    scipy.ndimage.binary_dilation with disk(24) -- what the reference's skimage call resolves to -- timed on the first 4 masks
    and scaled to the scan; the kernel's bits of those 4 are checked, untimed, against scipy's.  Also the share of the traffic
    bound it reaches: the masks read once plus the bitmaps written once at the 6.29 TB/s copy rate of BASELINE.md.
  * gs2m_points_cull_views: 1 M and 5 M points against the 64 dilated views; 70 % of them lie on the object and walk every
    view, 30 % are background and leave at the first view that fails.  Yardstick: the same projection and torch's
    F.grid_sample(mode='nearest') on the host (torch CPU, f32), all views, timed once at 1 M points; the keep-masks are compared.
  * evaluation.dtu_cull on a synthetic scan (an object sphere inside a background sphere, about 1 M vertices, 64 masks as
    host arrays): wall time with a synchronise, uploads and the mesh filter included.
Torch events around single calls: median [min, max] of --repeats calls after --warmup.  One JSON line; --out also writes text.

Usage:  python tools/cull_bench.py [--repeats 30] [--warmup 10] [--out profiles/cull.txt]
"""
import argparse
import ctypes as C
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
from gs2mesh_amd.mesh import TriangleMesh  # noqa: E402

W, H, RADIUS, COPY_RATE = 1600, 1200, 24, 6.29e12


def scan(n):
    """n cameras on a ring around the origin as world_mat_i / scale_mat_i, and the silhouettes of a unit ball as masks"""
    cams = {}
    masks = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        a = 2 * np.pi * i / n
        eye = np.array([np.cos(a), np.sin(a), 0.3 + 0.4 * np.sin(3 * a)]) * 3.5
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0, 0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        K = np.array([[1400.0, 0, (W - 1) / 2], [0, 1400.0, (H - 1) / 2], [0, 0, 1]])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = K @ R, -K @ R @ eye
        cams[f"world_mat_{i}"], cams[f"scale_mat_{i}"] = P, np.eye(4)
        r_px = 1400.0 / np.sqrt(np.dot(eye, eye) - 1)             # the ball's outline, about 420 px
        masks[i] = (((xx - (W - 1) / 2) ** 2 + (yy - (H - 1) / 2) ** 2) <= (1.05 * r_px) ** 2) * 255
    return cams, masks


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def repeat(fn, warmup, repeats):
    t = []
    for rnd in range(warmup + repeats):
        ms, _ = timed(fn)
        if rnd >= warmup:
            t.append(ms)
    return stats(t)


def shell_points(n, seed):
    """70 % on a noisy shell of the unit ball (inside every mask: they walk all views), 30 % background in a cube of +-3"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (1 + rng.normal(0, 0.01, (n, 1)))
    far = rng.random(n) < 0.3
    p[far] = rng.uniform(-3, 3, (int(far.sum()), 3))
    return p.astype(np.float32)


def sphere(n_lat, radius):
    th = np.linspace(0, np.pi, n_lat + 2)[1:-1]
    ph = np.linspace(0, 2 * np.pi, 2 * n_lat, endpoint=False)
    T, Pp = np.meshgrid(th, ph, indexing="ij")
    verts = np.stack([np.sin(T) * np.cos(Pp), np.sin(T) * np.sin(Pp), np.cos(T)], -1).reshape(-1, 3) * radius
    r, c = np.meshgrid(np.arange(n_lat - 1), np.arange(2 * n_lat), indexing="ij")
    i00, i01 = (r * 2 * n_lat + c).reshape(-1), (r * 2 * n_lat + (c + 1) % (2 * n_lat)).reshape(-1)
    tris = np.concatenate([np.stack([i00, i00 + 2 * n_lat, i01 + 2 * n_lat], 1), np.stack([i00, i01 + 2 * n_lat, i01], 1)])
    return verts, tris.astype(np.int32)


def host_cull(points, proj, dilated):
    """the reference's loop on the host in torch f32: projection, validity, nearest grid_sample, all views"""
    import torch.nn.functional as F
    p = torch.from_numpy(points)
    hom = torch.cat([p, torch.ones(len(p), 1)], 1).T.contiguous()
    keep = torch.ones(len(p), dtype=torch.bool)
    for m, mask in zip(torch.from_numpy(proj), dilated):
        c = m @ hom
        pix = (c[:2] / (c[2][None] + 1e-6)).T.contiguous()
        pix[:, 0] /= W - 1
        pix[:, 1] /= H - 1
        g = (pix - 0.5) * 2
        inside = ((g > -1) & (g < 1)).all(dim=1).float()
        s = F.grid_sample(mask[None, None], g[None, None], mode="nearest", padding_mode="zeros", align_corners=True)[0, 0, 0]
        keep &= (s + (1 - inside)) > 0
    return keep.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--views", type=int, nargs="*", default=[49, 64])
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--host-masks", type=int, default=4, help="masks the host dilation is timed on (scaled to the scan)")
    ap.add_argument("--host-points", type=int, default=1_000_000, help="points the host cull is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cull_bench needs a GPU: a CPU run gives no timing")
    from scipy import ndimage
    lib = _lib.get()
    stream = torch.cuda.current_stream().cuda_stream
    nw = (W + 63) // 64
    n_max = max(a.views)
    cams, masks = scan(n_max)
    proj, _ = evaluation.dtu_projections(cams)
    dm = torch.from_numpy(masks).cuda()
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "mask_size": [W, H], "radius": RADIUS,
           "dilate": {}, "cull": {}}

    # ---- dilation ------------------------------------------------------------------------------------------------------------
    L = np.arange(-RADIUS, RADIUS + 1)
    disk = (L[:, None] ** 2 + L[None, :] ** 2) <= RADIUS ** 2
    t0 = time.perf_counter()
    host_dil = [ndimage.binary_dilation(masks[i] != 0, structure=disk) for i in range(a.host_masks)]
    host_ms = (time.perf_counter() - t0) * 1e3
    bits_all = None
    for n in a.views:
        bits = torch.empty((n, H, nw), dtype=torch.int64, device="cuda")
        need = int(lib.gs2m_mask_dilate_disk_scratch_bytes(n, W, H))
        scratch = torch.empty((need // 8,), dtype=torch.int64, device="cuda")
        ptrs = (C.c_void_p * n)(*[dm.data_ptr() + i * H * W for i in range(n)])
        call = lambda: _lib.check(lib.gs2m_mask_dilate_disk(n, W, H, ptrs, RADIUS, _ptr(bits), None, _ptr(scratch), need, stream), lib)
        row = repeat(call, a.warmup, a.repeats)
        traffic = n * H * W + n * H * nw * 8
        row.update(traffic_bytes=traffic, bound_ms=traffic / COPY_RATE * 1e3, host_scipy_ms_scaled=host_ms / a.host_masks * n)
        row["share_of_traffic_bound"] = row["bound_ms"] / row["median_ms"]
        res["dilate"][str(n)] = row
        if n == n_max:
            bits_all = bits
    res["dilate"]["host_scipy_ms_per_mask"] = host_ms / a.host_masks
    got = bits_all[:a.host_masks].cpu().numpy().view(np.uint64)
    want = np.packbits(np.pad(np.stack(host_dil), ((0, 0), (0, 0), (0, nw * 64 - W))).reshape(a.host_masks, H, nw, 64), axis=-1,
                       bitorder="little").view("<u8").reshape(a.host_masks, H, nw)
    res["dilate"]["equals_scipy_on_host_masks"] = bool(np.array_equal(got, want))

    # ---- cull ----------------------------------------------------------------------------------------------------------------
    dproj = torch.from_numpy(proj).cuda().reshape(-1, 12).contiguous()
    for V in a.points:
        pts = torch.from_numpy(shell_points(V, V)).cuda()
        keep = torch.empty(V, dtype=torch.uint8, device="cuda")
        call = lambda: _lib.check(lib.gs2m_points_cull_views(V, _ptr(pts), n_max, _ptr(dproj), _ptr(bits_all), W, H, float(W), float(H),
                                                             _ptr(keep), stream), lib)
        row = repeat(call, a.warmup, a.repeats)
        row.update(views=n_max, kept=int(keep.sum().item()))
        res["cull"][str(V)] = row
    hp = shell_points(a.host_points, a.host_points)
    bytes_all = torch.empty((n_max, H, W), dtype=torch.uint8, device="cuda")
    scratch = torch.empty((int(lib.gs2m_mask_dilate_disk_scratch_bytes(n_max, W, H)) // 8,), dtype=torch.int64, device="cuda")
    ptrs = (C.c_void_p * n_max)(*[dm.data_ptr() + i * H * W for i in range(n_max)])
    _lib.check(lib.gs2m_mask_dilate_disk(n_max, W, H, ptrs, RADIUS, _ptr(bits_all), _ptr(bytes_all), _ptr(scratch), scratch.shape[0] * 8,
                                         stream), lib)
    dilated = bytes_all.cpu().float()
    t0 = time.perf_counter()
    host_keep = host_cull(hp, proj, dilated)
    host_cull_ms = (time.perf_counter() - t0) * 1e3
    dev_keep = evaluation.cull_points(torch.from_numpy(hp).cuda(), proj, bits_all, (W, H), (W, H)).cpu().numpy()
    res["cull"]["host_torch_cpu"] = {"points": a.host_points, "views": n_max, "ms": host_cull_ms, "threads": torch.get_num_threads(),
                                     "keep_bits_that_differ": int(np.count_nonzero(dev_keep != host_keep))}

    # ---- the whole step ------------------------------------------------------------------------------------------------------
    (v1, t1), (v2, t2) = sphere(600, 1.0), sphere(380, 2.2)           # the object, and a background shell the masks cull
    verts, tris = np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)])
    mesh = TriangleMesh(verts, tris)
    mask_list = [m for m in masks]
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluation.dtu_cull(mesh, cams, mask_list, radius=RADIUS, norm_size=(W, H))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["dtu_cull"] = {"vertices": int(verts.shape[0]), "triangles": int(tris.shape[0]), "views": n_max, "kept_vertices": int(out.vertices.shape[0]),
                       "wall_ms": wall}
    print(json.dumps(res))
    if a.out:
        fmt = lambda t: f"{t['median_ms']:10.3f}  [{t['min_ms']:.3f}, {t['max_ms']:.3f}]"
        lines = [f"The DTU cull's kernels, {res['device']}: stream time per call in ms, median [min, max] of {a.repeats} calls after "
                 f"{a.warmup} warm-ups (tools/cull_bench.py)", "",
                 f"gs2m_mask_dilate_disk, masks of {W} x {H}, r = {RADIUS}, bitmaps only"]
        for n in a.views:
            row = res["dilate"][str(n)]
            lines.append(f"  {n} masks {fmt(row)}   traffic bound (masks read + bitmaps written, {row['traffic_bytes'] / 1e6:.1f} MB at "
                         f"6.29 TB/s) {row['bound_ms']:.4f} ms = {row['share_of_traffic_bound']:.3f} of the call;  scipy binary_dilation on "
                         f"the host, scaled from {a.host_masks} masks: {row['host_scipy_ms_scaled']:.0f} ms")
        lines.append(f"  scipy per mask: {res['dilate']['host_scipy_ms_per_mask']:.0f} ms; kernel bits == scipy on those masks: "
                     f"{res['dilate']['equals_scipy_on_host_masks']}")
        lines += ["", f"gs2m_points_cull_views, {n_max} views, 70 % of the points on the object, 30 % background"]
        for V in a.points:
            row = res["cull"][str(V)]
            lines.append(f"  {V:,} points {fmt(row)}   kept {row['kept']:,}")
        hc = res["cull"]["host_torch_cpu"]
        lines.append(f"  torch CPU (f32 matmul + grid_sample nearest, {hc['threads']} threads), {hc['points']:,} points x {hc['views']} views, "
                     f"one run: {hc['ms']:.0f} ms; keep-bits that differ from the kernel's: {hc['keep_bits_that_differ']}")
        dc = res["dtu_cull"]
        lines += ["", f"evaluation.dtu_cull, wall time with a synchronise (mask upload and the host mesh filter included): {dc['vertices']:,} "
                  f"vertices, {dc['triangles']:,} triangles, {dc['views']} masks -> {dc['kept_vertices']:,} vertices kept",
                  "  " + ", ".join(f"{w:.0f} ms" for w in dc["wall_ms"]), ""]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
