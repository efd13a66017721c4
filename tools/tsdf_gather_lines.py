"""Distinct cache lines per 64-lane gather instruction of the TSDF sweep, counted on the CPU from addresses alone (no GPU, no
timing): the voxel centres of the blocks a frame touches on the camera side of the benchmark's sphere are projected as
``tsdf_project`` does (fp32, the incremental z chain), and for each way of laying 64 lanes over a block the depth (4 B per
pixel) and colour (3 B per pixel, read as one unaligned 4-B word) addresses of one instruction are reduced to their 64-B and
128-B lines.

    python tools/tsdf_gather_lines.py --config C2 --poses 3
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, json
import numpy as np
from gs2mesh_amd import synthetic

F32 = np.float32
ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C2")
ap.add_argument("--poses", type=int, default=3)
a = ap.parse_args()
cfg = synthetic.CONFIGS[a.config]
W, H, fx = cfg.width, cfg.height, F32(cfg.focal)
cx, cy = F32(W / 2), F32(H / 2)
vl, R, trunc = cfg.voxel_length, cfg.sphere_radius, cfg.sdf_trunc
L = 16 * vl


def touched_blocks(E, stride=4):
    """the touch pass in numpy: every `stride`-th valid depth pixel back-projected (f64), the blocks its +-trunc cube overlaps"""
    z = synthetic.sphere_depth(E[:3], W, H, cfg.focal, cfg.focal, W / 2, H / 2, R)[::stride, ::stride].astype(np.float64)
    ii, jj = np.arange(0, H, stride)[:, None], np.arange(0, W, stride)[None, :]
    ok = z > 0
    x, y = ((jj - W / 2) * z / cfg.focal)[ok], ((ii - H / 2) * z / cfg.focal)[ok]
    pw = (np.linalg.inv(E) @ np.stack([x, y, z[ok], np.ones_like(x)]))[:3].T
    lo, hi = np.floor((pw - trunc) / L).astype(np.int64), np.floor((pw + trunc) / L).astype(np.int64)
    out = []
    for d in np.ndindex(*(int((hi - lo).max()) + 1,) * 3):
        b = lo + np.array(d)
        out.append(b[np.all(b <= hi, axis=1)])
    return np.unique(np.concatenate(out), axis=0)


def pixels(E, key):
    """tsdf_block_centres + tsdf_cam_point + tsdf_z_step + tsdf_project for the voxels [x, y, z] of block `key`: pixel index or -1"""
    E = E.astype(np.float32)
    lin = F32(vl) * F32(0.5) + F32(vl) * np.arange(16, dtype=np.float32)
    org = key.astype(np.float64) * L
    p0 = (lin.astype(np.float64) + org[0]).astype(np.float32)[:, None]
    p1 = (lin.astype(np.float64) + org[1]).astype(np.float32)[None, :]
    p2 = F32(np.float64(F32(vl) * F32(0.5)) + org[2])
    pc = [E[r, 0] * p0 + E[r, 1] * p1 + E[r, 2] * p2 + E[r, 3] * F32(1.0) for r in range(3)]
    step = [E[r, 2] * F32(vl) for r in range(3)]
    out = []
    for z in range(16):
        with np.errstate(divide="ignore", invalid="ignore"):
            u_f = pc[0] * fx / pc[2] + cx + F32(0.5)
            v_f = pc[1] * fx / pc[2] + cy + F32(0.5)
        ok = (pc[2] > 0) & (u_f >= F32(0.0001)) & (u_f < F32(W - F32(0.0001))) & (v_f >= F32(0.0001)) & (v_f < F32(H - F32(0.0001)))
        out.append(np.where(ok, np.where(ok, v_f, 0).astype(np.int64) * W + np.where(ok, u_f, 0).astype(np.int64), -1))
        pc = [pc[r] + step[r] for r in range(3)]
    return np.stack(out, -1)                                                   # [x, y, z]


def lines_per_instruction(pix, line):
    """pix [groups, 64] -> mean over the groups with a valid lane of the distinct `line`-byte lines of the depth and the colour gather"""
    valid = pix >= 0
    big = np.int64(1) << 60
    d = np.where(valid, (4 * pix) // line, big)
    c = np.concatenate([np.where(valid, (3 * pix) // line, big), np.where(valid, (3 * pix + 3) // line, big)], 1)
    def distinct(x):
        x = np.sort(x, 1)
        return (np.diff(x, axis=1) != 0).sum(1) + 1 - (x[:, -1] == big)         # the sentinel is one extra value where present
    keep = valid.any(1)
    return distinct(d)[keep].mean(), distinct(c)[keep].mean()


LAYOUTS = {
    # lanes of one instruction: [x, y, z] of a block -> [groups, 64]
    "4 x * 16 y, one z": lambda p: p.reshape(4, 4, 16, 16).transpose(0, 3, 1, 2).reshape(-1, 64),
    "8 x * 8 y, one z": lambda p: p.reshape(2, 8, 2, 8, 16).transpose(0, 2, 4, 1, 3).reshape(-1, 64),
    "one 4x4x4 micro-block": lambda p: p.reshape(4, 4, 4, 4, 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 64),
}

groups = {k: [] for k in LAYOUTS}
n_blocks = 0
for pose in synthetic.ring_poses(a.poses, cfg.ring_radius, 0, a.poses):
    E = np.eye(4)
    E[:3] = pose
    for key in touched_blocks(E):
        p = pixels(E, key)
        n_blocks += 1
        for k, f in LAYOUTS.items():
            groups[k].append(f(p))
print(json.dumps(dict(config=a.config, poses=a.poses, blocks=n_blocks, px_per_voxel=round(float(fx) * vl / (cfg.ring_radius - R), 2))))
for k in LAYOUTS:
    g = np.concatenate(groups[k])
    d64, c64 = lines_per_instruction(g, 64)
    d128, c128 = lines_per_instruction(g, 128)
    print(json.dumps({"lanes": k, "depth_64B": round(d64, 1), "depth_128B": round(d128, 1), "colour_64B": round(c64, 1),
                      "colour_128B": round(c128, 1)}))
