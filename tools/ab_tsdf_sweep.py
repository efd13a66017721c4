"""Development A/B of builds of the TSDF batch sweep: several builds of libgs2mesh_amd.so in ONE process, order-interleaved
(the order is rotated every round), per-frame stage times from the library's own stage timers, + a check that every
build leaves the same volume bit for bit as the first one.

    python tools/ab_tsdf_sweep.py --libs gs2mesh_amd/libgs2mesh_amd.so,/path/to/other/libgs2mesh_amd.so --configs C2,C4 --rounds 5
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, ctypes, json
import numpy as np, torch
from gs2mesh_amd import _lib, synthetic
from gs2mesh_amd.integration import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume, TSDFVolumeColorType

ap = argparse.ArgumentParser()
ap.add_argument("--libs", required=True, help="comma-separated builds of libgs2mesh_amd.so; the first one is the reference")
ap.add_argument("--configs", default="C2")
ap.add_argument("--frames", type=int, default=20, help="frames of the job (bench.py: 20 steps)")
ap.add_argument("--batch", type=int, default=20, help="frames per sweep")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--color", type=int, default=1)
a = ap.parse_args()
paths = [p for p in a.libs.split(",") if p]
libs = [_lib.bind(ctypes.CDLL(os.path.abspath(p))) for p in paths]
names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
dev = torch.device("cuda:0")

for cname in a.configs.split(","):
    cfg = synthetic.CONFIGS[cname]
    W, H = cfg.width, cfg.height
    poses = synthetic.ring_poses(a.frames, cfg.ring_radius, 0, cfg.n_pairs)
    deps = [synthetic.sphere_depth_torch(p, W, H, cfg.focal, cfg.focal, W / 2, H / 2, cfg.sphere_radius, dev) for p in poses]
    Es = []
    for p in poses:
        E = np.eye(4)
        E[:3] = p
        Es.append(E)
    col = torch.from_numpy(synthetic.color_pattern(W, H)).to(dev)
    intr = PinholeCameraIntrinsic(W, H, cfg.focal, cfg.focal, W / 2, H / 2)
    vols = [ScalableTSDFVolume(cfg.voxel_length, cfg.sdf_trunc, TSDFVolumeColorType.RGB8 if a.color else TSDFVolumeColorType.NoColor,
                               max_blocks=(cfg.tsdf_n // 16) ** 3, lib=lib) for lib in libs]

    def run(vol):
        for i0 in range(0, a.frames, a.batch):
            idx = range(i0, min(a.frames, i0 + a.batch))
            vol.integrate_batch([RGBDImage(col, deps[k], depth_scale=1.0, depth_trunc=cfg.baseline * 20) for k in idx], intr,
                                [Es[k] for k in idx], min_depth=cfg.baseline * 4)

    ref, same = None, []
    for vol in vols:                                      # warm-up + the result of every build against the first one's
        run(vol)
        k, *arrs = vol.download()
        o = np.lexsort(k.T[::-1])
        got = [k[o]] + [x[o] for x in arrs] + [np.asarray(vol.status()[:2])]
        ref = ref or got
        same.append(all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(got, ref)))
        vol.reset()
    runs = {n: dict(tsdf_integrate=[], tsdf_touch=[]) for n in names}
    for rnd in range(a.rounds):
        for i in [(j + rnd) % len(vols) for j in range(len(vols))]:
            vol = vols[i]
            vol.set_stage_timing(True)
            run(vol)
            st = vol.stage_times()
            vol.set_stage_timing(False)
            vol.reset()
            for s in runs[names[i]]:
                ms, c = st[s]
                runs[names[i]][s].append(round(1e3 * ms / max(c, 1), 2))
    for n, ok in zip(names, same):
        r = runs[n]
        print(json.dumps(dict(config=cname, lib=n, frames=a.frames, batch=a.batch, bit_identical_to_first=ok,
                              integrate_us_per_frame=r["tsdf_integrate"], integrate_median=float(np.median(r["tsdf_integrate"])),
                              touch_us_per_frame=r["tsdf_touch"], touch_median=float(np.median(r["tsdf_touch"])))), flush=True)
    for vol in vols:
        vol.close()
