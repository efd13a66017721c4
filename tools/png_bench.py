"""Device PNG encoder on the drop-in Renderer: one JSON line per scene (C2 `synth_v1` and `trained_like`, 300 k Gaussians,
1600 x 1200), files on tmpfs.

  encode_us_per_pair      GPU time of gs2m_png_encode (hipEvents) per stereo pair: one pair per call, and 4 pairs per call
  render_image_pair       wall pairs/s of N x Renderer.render_image_pair with png_encoder="pil" and "device"
  render_image_pairs      wall pairs/s of one Renderer.render_image_pairs(range(N))
  bytes                   file sizes of the first pair against PIL compress_level 1 (cv2's default) and 6 (PIL's default)

    python tools/png_bench.py [--pairs 20] [--out /dev/shm/png_bench]
"""
import argparse
import io
import json
import os
import shutil
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from PIL import Image
from scipy.spatial.transform import Rotation

from gs2mesh_amd import synthetic
from gs2mesh_amd.gaussian_model import write_gaussian_ply
from gs2mesh_amd.png import PngEncoder
from gs2mesh_amd.renderer_utils import Renderer


def write_scene(root, g, cfg, n):
    ply_dir = os.path.join(root, "splatting_output", "custom", "scene", "point_cloud", "iteration_30000")
    os.makedirs(ply_dir, exist_ok=True)
    write_gaussian_ply(os.path.join(ply_dir, "point_cloud.ply"), g["xyz"], g["features_dc"], g["features_rest"], g["opacity"],
                       g["scaling"], g["rotation"])
    sp = os.path.join(root, "colmap", "sparse", "0")
    os.makedirs(sp, exist_ok=True)
    with open(os.path.join(sp, "cameras.txt"), "w") as f:
        f.write(f"1 PINHOLE {cfg.width} {cfg.height} {cfg.focal} {cfg.focal} {cfg.width / 2} {cfg.height / 2}\n")
    with open(os.path.join(sp, "images.txt"), "w") as f:
        for i, p in enumerate(synthetic.ring_poses(n, cfg.ring_radius, 0, cfg.n_pairs)):
            q = Rotation.from_matrix(p[:, :3]).as_quat()
            vals = [q[3], q[0], q[1], q[2], p[0, 3], p[1, 3], p[2, 3]]
            f.write(f"{i + 1} " + " ".join(repr(float(v)) for v in vals) + f" 1 img{i:03}.png\n\n")


def args_for(cfg):
    return Namespace(colmap_name="scene", dataset_name="custom", GS_white_background=False, GS_iterations=30000,
                     renderer_baseline_absolute=cfg.baseline, renderer_baseline_percentage=7.0, renderer_scene_360=True,
                     renderer_save_json=False, renderer_sort_cameras=False)


def encode_us(enc, rgb8, reps=20):
    """GPU time of one gs2m_png_encode of rgb8, microseconds (median of reps)."""
    enc.encode(rgb8)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        enc.encode_device(rgb8)
        b.record()
        b.synchronize()
        ts.append(1e3 * a.elapsed_time(b))
    return float(np.median(ts))


def wall(fn, pairs):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return pairs / (time.perf_counter() - t)


def run(scene, n, out_root):
    cfg = synthetic.CONFIGS["C2"]
    g = (synthetic.synth_v1(cfg.P, cfg.seed, cfg.log_s_mu) if scene == "synth_v1" else
         synthetic.trained_like(cfg.P, cfg.seed, cfg.log_s_mu, focal=cfg.focal, ring_radius=cfg.ring_radius))
    root = os.path.join(out_root, scene)
    shutil.rmtree(root, ignore_errors=True)
    write_scene(root, g, cfg, n)
    col = os.path.join(root, "colmap")
    r = {}
    for mode in ("pil", "device"):
        ren = Renderer(root, col, os.path.join(root, "out_" + mode), args_for(cfg), png_encoder=mode)
        ren.prepare_renderer()
        ren.render_image_pair(0)                                           # warm-up: arenas, code objects
        r[mode] = wall(lambda: [ren.render_image_pair(i) for i in range(n)], n)
        if mode == "device":
            rgb8 = ren.render_pair_device(0)["rgb8"]
            enc = ren._encoder()
            one = encode_us(enc, rgb8)
            four = torch.cat([ren.render_pair_device(i)["rgb8"] for i in range(4)])
            batch = encode_us(enc, four) / 4
            ren.render_image_pairs(range(min(n, 4)))                       # warm-up of the 8-view launch + writer
            batched = wall(lambda: ren.render_image_pairs(range(n)), n)
            files = enc.encode(rgb8)
            host = rgb8.cpu().numpy()
    sizes = dict(device=[len(f) for f in files], pil_level1=[], pil_level6=[])
    for k in range(2):
        for lvl in (1, 6):
            buf = io.BytesIO()
            Image.fromarray(host[k], mode="RGB").save(buf, format="PNG", compress_level=lvl)
            sizes[f"pil_level{lvl}"].append(buf.tell())
    shutil.rmtree(root, ignore_errors=True)
    return dict(tool="png_bench", scene=scene, config="C2", P=cfg.P, width=cfg.width, height=cfg.height, pairs=n,
                encode_us_per_pair=dict(one_pair_per_call=round(one, 1), four_pairs_per_call=round(batch, 1)),
                render_image_pair_pairs_per_s=dict(pil=round(r["pil"], 2), device=round(r["device"], 1)),
                render_image_pairs_pairs_per_s=round(batched, 1),
                bytes=sizes,
                size_vs_pil_level1=round(sum(sizes["device"]) / sum(sizes["pil_level1"]), 4),
                size_vs_pil_level6=round(sum(sizes["device"]) / sum(sizes["pil_level6"]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--out", default="/dev/shm/png_bench")
    ap.add_argument("--scenes", default="synth_v1,trained_like")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a GPU")
    for scene in a.scenes.split(","):
        print(json.dumps(run(scene, a.pairs, a.out)), flush=True)


if __name__ == "__main__":
    main()
