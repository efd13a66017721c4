"""Census of the batch sweep's frame passes: how many of them update no voxel, and how many of those the max-depth test of
k_tsdf_integrate_batch (tsdf_kernels.h, ``tsdf_pass_live``) proves dead without probing.  CPU only, numpy, the seeded synthetic
configs of gs2mesh_amd.synthetic with the benchmark's own ring of poses and depth conversion.

    python tools/tsdf_dead_pass_census.py --config C2 --frames 20
    python tools/tsdf_dead_pass_census.py --config C4 --frames 12

The touch rule is Open3D's (f64 back-projection of every ``stride``-th pixel, every block the +-sdf_trunc box of the point
overlaps), the voxel update is the f32 projection of the sweep, and the cull test is the kernel's restated in f64 with the
kernel's margins.  A pass is (micro-column of 4 x 4 x 16 voxels, frame that touched its block): what one wave of the sweep runs
per frame; a probe is (micro-block of 4^3 voxels, frame): what one gather instruction of it covers.

The functions are also what tests/test_tsdf_dead_pass_cull.py checks its scenes with.
"""
import argparse
import os
import sys

import numpy as np

TILE = 8                      # GS2M_TSDF_TILE
MAX_TILES = 48                # GS2M_TSDF_CULL_MAX_TILES: a footprint over more tiles is not tested (live)
F32 = np.float32


def convert_depth(depth, mask=None, min_depth=0.0, depth_scale=1.0, depth_trunc=float("inf")):
    """the depth as the integrator sees it (tsdf_read_depth + tsdf_convert_depth), f32; invalid samples may come out NaN"""
    d = np.asarray(depth, np.float32).copy()
    with np.errstate(invalid="ignore"):
        if mask is not None:
            d = d * (np.asarray(mask) != 0).astype(np.float32)
        if min_depth > 0:
            d = np.where(d < F32(min_depth), F32(0), d)
        if F32(depth_scale) != F32(1):
            d = d / F32(depth_scale)
        d = np.where(d.astype(np.float64) >= depth_trunc, F32(0), d)
    return d.astype(np.float32)


def tile_map(conv):
    """max of the valid (> 0) converted depths per 8 x 8 tile, 0 where a tile has none: k_tsdf_depth_tiles"""
    H, W = conv.shape
    ty, tx = -(-H // TILE), -(-W // TILE)
    with np.errstate(invalid="ignore"):
        v = np.where(conv > 0, conv, F32(0)).astype(np.float32)
    pad = np.zeros((ty * TILE, tx * TILE), np.float32)
    pad[:H, :W] = v
    return pad.reshape(ty, TILE, tx, TILE).max(axis=(1, 3))


def touched_blocks(conv, K, E, voxel, trunc, stride):
    """the blocks a frame touches, sorted [n, 3] (ScalableTSDFVolume::Integrate, step i)"""
    W, H, fx, fy, cx, cy = K
    ii, jj = np.arange(0, H, stride), np.arange(0, W, stride)
    z = conv[np.ix_(ii, jj)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = z > 0
    if not valid.any():
        return np.zeros((0, 3), np.int64)
    x = ((jj[None, :] - cx) * np.where(valid, z, 1.0) / fx)[valid]
    y = ((ii[:, None] - cy) * np.where(valid, z, 1.0) / fy)[valid]
    z = z[valid]
    pose = np.linalg.inv(np.asarray(E, np.float64))
    L = voxel * 16
    lo, hi = [], []
    for r in range(3):
        pw = pose[r, 0] * x + pose[r, 1] * y + pose[r, 2] * z + pose[r, 3] * 1.0
        lo.append(np.floor((pw - trunc) / L).astype(np.int64))
        hi.append(np.floor((pw + trunc) / L).astype(np.int64))
    lo, hi = np.stack(lo, 1), np.stack(hi, 1)
    boxes = np.unique(np.hstack([lo, hi]), axis=0)                  # neighbouring pixels mostly share their box
    lo, hi = boxes[:, :3], boxes[:, 3:]
    ext = (hi - lo).max(0) + 1
    out = []
    for ox in range(ext[0]):
        for oy in range(ext[1]):
            for oz in range(ext[2]):
                b = lo + np.array([ox, oy, oz])
                out.append(b[np.all(b <= hi, 1)])
    return np.unique(np.vstack(out), axis=0)


def voxel_updates(keys, conv, K, E, voxel, trunc):
    """upd [n, 16, 16, 16] (x, y, z): does the frame update the voxel?  The sweep's f32 projection, z chain included."""
    W, H, fx, fy, cx, cy = K
    E = np.asarray(E, np.float64).astype(np.float32)
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    vl = F32(voxel)
    half = vl * F32(0.5)
    L = voxel * 16
    lin = half + vl * np.arange(16, dtype=np.float32)
    org = keys.astype(np.float64) * L
    p0 = (lin[None, :].astype(np.float64) + org[:, 0:1]).astype(np.float32)[:, :, None]
    p1 = (lin[None, :].astype(np.float64) + org[:, 1:2]).astype(np.float32)[:, None, :]
    p2 = (np.float64(half) + org[:, 2]).astype(np.float32)[:, None, None]
    pc = [E[r, 0] * p0 + E[r, 1] * p1 + E[r, 2] * p2 + E[r, 3] * F32(1.0) for r in range(3)]
    step = [E[r, 2] * vl for r in range(3)]
    chain = [[], [], []]
    for _ in range(16):
        for r in range(3):
            chain[r].append(pc[r])
            pc[r] = pc[r] + step[r]
    pc0, pc1, pc2 = (np.stack(c, -1) for c in chain)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u_f = pc0 * F32(fx) / pc2 + F32(cx) + F32(0.5)
        v_f = pc1 * F32(fy) / pc2 + F32(cy) + F32(0.5)
        acc = (pc2 > 0) & (u_f >= F32(0.0001)) & (u_f < F32(W - F32(0.0001))) & (v_f >= F32(0.0001)) & (v_f < F32(H - F32(0.0001)))
        u = np.where(acc, u_f, 0).astype(np.int64)
        v = np.where(acc, v_f, 0).astype(np.int64)
        d = conv[v, u]
        xx, yy = (u.astype(np.float32) - F32(cx)) * (F32(1.0) / F32(fx)), (v.astype(np.float32) - F32(cy)) * (F32(1.0) / F32(fy))
        mult = np.sqrt(xx * xx + yy * yy + F32(1.0))
        sdf = (d - pc2) * mult
        return acc & (d > 0) & (sdf > -F32(trunc))


def proven_dead(keys, tiles, K, E, voxel, trunc, per_micro_block=False):
    """The kernel's cull test (tsdf_pass_live, negated) in f64: dead [n, 4 (xq), 4 (yq)] per micro-column, or with
    ``per_micro_block`` [n, 4 (j), 4, 4] for the 4 voxel layers z = 4 j .. 4 j + 3 of each.  Also returned: why, as a small
    integer per entry -- 0 live, 1 footprint off the image, 2 no depth sample in the footprint, 3 behind the band; and the number
    of tiles the test read (0 where it read none)."""
    W, H, fx, fy, cx, cy = K
    E = np.asarray(E, np.float64).astype(np.float32).astype(np.float64)
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    n = len(keys)
    vl = float(F32(voxel))
    L = voxel * 16
    lin = vl * 0.5 + vl * np.arange(16)
    org = keys.astype(np.float64) * L
    q = np.arange(4)
    xs = np.stack([lin[4 * q][None, :] + org[:, 0:1], lin[4 * q + 3][None, :] + org[:, 0:1]], -1)     # [n, 4, 2]
    ys = np.stack([lin[4 * q][None, :] + org[:, 1:2], lin[4 * q + 3][None, :] + org[:, 1:2]], -1)
    z0 = vl * 0.5 + org[:, 2]
    zr = [(0, 15)] if not per_micro_block else [(4 * j, 4 * j + 3) for j in range(4)]
    dead_all, why_all, nt_all = [], [], []
    for za, zb in zr:
        zs = np.stack([z0 + za * vl, z0 + zb * vl], -1)                                               # [n, 2]
        # corners [n, xq, yq, cx, cy, cz]
        X = xs[:, :, None, :, None, None]
        Y = ys[:, None, :, None, :, None]
        Z = zs[:, None, None, None, None, :]
        pc = [E[r, 0] * X + E[r, 1] * Y + E[r, 2] * Z + E[r, 3] for r in range(3)]
        S = max(float((abs(E[r, 0]) * np.abs(X) + abs(E[r, 1]) * np.abs(Y) + abs(E[r, 2]) * (np.abs(z0).max() + 16 * vl) + abs(E[r, 3])).max())
                for r in range(3))
        eps = S * 2.0 ** -18
        flat = [p.reshape(n, 4, 4, 8) for p in np.broadcast_arrays(*pc)]
        zmin = flat[2].min(-1)
        front = zmin - eps > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            zz = np.where(front[..., None], flat[2], 1.0)
            u = flat[0] * fx / zz + cx
            v = flat[1] * fy / zz + cy
            zl = np.where(front, zmin - eps, 1.0)
        umin, umax, vmin, vmax = u.min(-1), u.max(-1), v.min(-1), v.max(-1)
        au, av = np.maximum(np.abs(umin - cx), np.abs(umax - cx)), np.maximum(np.abs(vmin - cy), np.abs(vmax - cy))
        mu = 1.0 + eps / zl * (abs(fx) + au) + 2.0 ** -20 * (au + abs(cx) + 1.0)
        mv = 1.0 + eps / zl * (abs(fy) + av) + 2.0 ** -20 * (av + abs(cy) + 1.0)
        x0, x1 = np.maximum(np.floor(umin - mu), 0), np.minimum(np.ceil(umax + mu), W - 1)
        y0, y1 = np.maximum(np.floor(vmin - mv), 0), np.minimum(np.ceil(vmax + mv), H - 1)
        empty = front & ((x0 > x1) | (y0 > y1))
        test = front & ~empty
        tx0, tx1 = (np.where(test, x0, 0).astype(np.int64) // TILE, np.where(test, x1, 0).astype(np.int64) // TILE)
        ty0, ty1 = (np.where(test, y0, 0).astype(np.int64) // TILE, np.where(test, y1, 0).astype(np.int64) // TILE)
        many = (tx1 - tx0 + 1) * (ty1 - ty0 + 1) > MAX_TILES
        test &= ~many
        dmax = np.zeros(test.shape)
        for i in zip(*np.nonzero(test)):
            dmax[i] = tiles[ty0[i]:ty1[i] + 1, tx0[i]:tx1[i] + 1].max()
        zlow = zmin - eps - vl
        nodepth = test & (dmax == 0)
        behind = test & (dmax > 0) & (dmax - zlow <= -float(F32(trunc)))
        why = np.zeros(test.shape, np.int8)
        why[empty], why[nodepth], why[behind] = 1, 2, 3
        dead_all.append(why > 0)
        why_all.append(why)
        nt_all.append(np.where(test, (tx1 - tx0 + 1) * (ty1 - ty0 + 1), 0))
    if not per_micro_block:
        return dead_all[0], why_all[0], nt_all[0]
    return np.stack(dead_all, 1), np.stack(why_all, 1), np.stack(nt_all, 1)


def column_updates(upd):
    """upd [n, 16, 16, 16] -> does the pass of micro-column (xq, yq) update a voxel [n, 4, 4]; per micro-block [n, 4 (j), 4, 4]"""
    n = len(upd)
    u = upd.reshape(n, 4, 4, 4, 4, 4, 4)             # x = (xq, lx), y = (yq, ly), z = (j, lz)
    return u.any(axis=(2, 4, 5, 6)), u.any(axis=(2, 4, 6)).transpose(0, 3, 1, 2)


def census(frames, K, voxel, trunc, stride=4, log=None):
    """frames: [(converted depth [H, W] f32, E 4 x 4)] -> the table's figures as a dict"""
    per_block = {}                                                   # key -> list over its frames of (col_upd, col_dead) [4, 4]
    n_pass = n_pass_idle = n_pass_dead = n_probe = n_probe_idle = n_probe_dead = 0
    blocks_per_frame = []
    for k, (conv, E) in enumerate(frames):
        keys = touched_blocks(conv, K, E, voxel, trunc, stride)
        blocks_per_frame.append(len(keys))
        if not len(keys):
            continue
        tiles = tile_map(conv)
        col_dead = np.zeros((len(keys), 4, 4), bool)
        mb_dead = np.zeros((len(keys), 4, 4, 4), bool)
        col_upd = np.zeros((len(keys), 4, 4), bool)
        mb_upd = np.zeros((len(keys), 4, 4, 4), bool)
        for a in range(0, len(keys), 256):
            sl = slice(a, a + 256)
            col_upd[sl], mb_upd[sl] = column_updates(voxel_updates(keys[sl], conv, K, E, voxel, trunc))
            col_dead[sl] = proven_dead(keys[sl], tiles, K, E, voxel, trunc)[0]
            mb_dead[sl] = proven_dead(keys[sl], tiles, K, E, voxel, trunc, per_micro_block=True)[0]
        assert not (col_dead & col_upd).any() and not (mb_dead & mb_upd).any(), "the test culled a pass that updates a voxel"
        n_pass += col_upd.size
        n_pass_idle += int((~col_upd).sum())
        n_pass_dead += int(col_dead.sum())
        n_probe += mb_upd.size
        n_probe_idle += int((~mb_upd).sum())
        n_probe_dead += int(mb_dead.sum())
        for i, key in enumerate(map(tuple, keys.tolist())):
            per_block.setdefault(key, []).append(~col_dead[i])
        if log:
            log(f"frame {k}: {len(keys)} blocks, passes idle {100 * (~col_upd).mean():.1f} %, proven dead {100 * col_dead.mean():.1f} %")
    today, slowest, mean, empty_items, items = 0.0, 0.0, 0.0, 0, 0
    for lst in per_block.values():
        cnt = np.stack(lst).sum(0)                                   # live frame passes per wave [xq, yq]
        nfr = len(lst)
        for xq in range(4):
            items += 1
            today += nfr
            slowest += cnt[xq].max()
            mean += cnt[xq].mean()
            empty_items += int(cnt[xq].max() == 0)
    pct = lambda a, b: 100.0 * a / max(b, 1)
    return dict(frames=len(frames), blocks=len(per_block), blocks_per_frame=float(np.mean(blocks_per_frame)),
                passes_idle_pct=pct(n_pass_idle, n_pass), passes_proven_dead_pct=pct(n_pass_dead, n_pass),
                probes_idle_pct=pct(n_probe_idle, n_probe), probes_proven_dead_pct=pct(n_probe_dead, n_probe),
                passes_per_item_today=today / max(items, 1), passes_per_item_slowest_wave=slowest / max(items, 1),
                passes_per_item_mean_wave=mean / max(items, 1), items_without_live_pass_pct=pct(empty_items, items))


def synthetic_frames(cname, n_frames, ring_total=None):
    """the benchmark's TSDF job of a config: n_frames views spread over the whole ring (bench.py; ``ring_total`` views per turn
    otherwise), analytic sphere depth, the driver's depth conversion"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gs2mesh_amd import synthetic
    cfg = synthetic.CONFIGS[cname]
    W, H = cfg.width, cfg.height
    K = (W, H, cfg.focal, cfg.focal, W / 2, H / 2)
    frames = []
    for p in synthetic.ring_poses(n_frames, cfg.ring_radius, 0, ring_total or n_frames):
        E = np.eye(4)
        E[:3] = p
        d = synthetic.sphere_depth(p, W, H, cfg.focal, cfg.focal, W / 2, H / 2, cfg.sphere_radius)
        frames.append((convert_depth(d, None, cfg.baseline * 4, 1.0, cfg.baseline * 20), E))
    return frames, K, cfg.voxel_length, cfg.sdf_trunc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="C2")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--ring-total", type=int, default=None, help="views per turn of the ring (default: --frames, as bench.py spreads its job)")
    a = ap.parse_args()
    frames, K, voxel, trunc = synthetic_frames(a.config, a.frames, a.ring_total)
    r = census(frames, K, voxel, trunc, a.stride, log=lambda s: print(s, file=sys.stderr, flush=True))
    print(f"{a.config}, {r['frames']} frames: {r['blocks']} blocks, {r['blocks_per_frame']:.1f} blocks per frame")
    for label, key, unit in (("wave passes (micro-column x frame) that update no voxel", "passes_idle_pct", " %"),
                             ("... of which the max-depth test proves dead, of all passes", "passes_proven_dead_pct", " %"),
                             ("micro-block probes (4^3 voxels x frame) that update no voxel", "probes_idle_pct", " %"),
                             ("... proven dead by the test per micro-block, of all probes", "probes_proven_dead_pct", " %"),
                             ("frame passes per work item today", "passes_per_item_today", ""),
                             ("after the cull: slowest wave of the workgroup", "passes_per_item_slowest_wave", ""),
                             ("after the cull: mean wave", "passes_per_item_mean_wave", ""),
                             ("work items with no live pass at all", "items_without_live_pass_pct", " %")):
        print(f"  {label:<66s} {r[key]:6.2f}{unit}")


if __name__ == "__main__":
    main()
