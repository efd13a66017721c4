"""Train a Gaussian splat on one GPU: point cloud + posed images -> point_cloud/iteration_N/point_cloud.ply.

    python tools/train_splat.py <colmap_dir> <out_dir> [--iterations N] [--resolution-scale s] [--loss {torch,fused}]
                                [--optimizer {default,fused,sparse_adam}] [--depth-priors DIR --lambda-depth X [--depth-kind {centre,ray}]]
    python tools/train_splat.py --synthetic <out_dir> [--iterations N] [--loss {torch,fused}] [--optimizer ...]

<colmap_dir> holds a COLMAP text model (sparse/0/cameras.txt, images.txt, points3D.txt; PINHOLE or SIMPLE_PINHOLE cameras)
and images/.  <out_dir>/point_cloud/iteration_N/point_cloud.ply is where `Renderer` and `GaussianModel.load_ply` look.
--synthetic trains against renders of `synthetic.textured_sphere` instead (no dataset needed).  Prints the wall time per
iteration and its split into render forward, loss, backward and optimiser + densification (stream time between events).
--loss fused computes L1 + D-SSIM and its gradient with the HIP kernels (training.fused_loss) instead of torch ops.
--optimizer fused takes the Adam step and the densification statistics with the HIP kernels (optim.FusedAdam) instead of
torch.optim.Adam and boolean-mask indexing; --optimizer sparse_adam steps only the Gaussians the view saw.
--depth-priors DIR --lambda-depth X adds X * training.depth_l1_loss against one depth map per camera, read from
DIR/<NNN>/out_<model>/depth.npy (NNN = the camera's position in the list, the layout `Stereo` and `RenderedDepth` write;
--depth-model names <model>, default the only out_* folder); 0, NaN and inf in a map mean "no depth".  --depth-kind ray compares the priors with
the ray-Gaussian intersection depth instead of the z of the centres: its gradient also turns and flattens the Gaussians.
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

from gs2mesh_amd import colmap_io, training  # noqa: E402
from gs2mesh_amd.gaussian_model import GaussianModel  # noqa: E402
from gs2mesh_amd.graphics import BasicPointCloud, Camera, focal2fov  # noqa: E402


def load_colmap(root, scale, device):
    from PIL import Image
    sparse = os.path.join(root, "sparse", "0")
    cams = colmap_io.read_cameras_text(os.path.join(sparse, "cameras.txt"))
    cam_of = {}
    with open(os.path.join(sparse, "images.txt")) as f:
        rows = [ln.split() for ln in f if ln.strip() and not ln.startswith("#")]
    for e in rows[::2]:                                      # every second line lists the 2-D points
        cam_of[int(e[0])] = int(e[8])
    ids, poses, names = colmap_io.read_image_poses_text(os.path.join(sparse, "images.txt"))
    cameras, images = [], []
    for k, (i, p, name) in enumerate(zip(ids, poses, names)):
        c = cams[cam_of[i]]
        if c.model == "SIMPLE_PINHOLE":
            fx = fy = c.params[0]
        elif c.model == "PINHOLE":
            fx, fy = c.params[0], c.params[1]
        else:
            raise SystemExit(f"camera model {c.model}: undistort to PINHOLE first")
        im = Image.open(os.path.join(root, "images", name)).convert("RGB")
        W, H = round(c.width * scale), round(c.height * scale)
        if (W, H) != im.size:
            im = im.resize((W, H), Image.LANCZOS)
        images.append(torch.from_numpy(np.asarray(im, np.float32) / 255.0).permute(2, 0, 1).contiguous().to(device))
        cameras.append(Camera(i, p[:, :3].T, p[:, 3], focal2fov(fx, c.width), focal2fov(fy, c.height), W, H, image_name=name, uid=k))
    xyz, rgb, _ = colmap_io.read_points3D_text(os.path.join(sparse, "points3D.txt"))
    return cameras, images, BasicPointCloud(xyz.astype(np.float32), rgb.astype(np.float32) / 255.0, np.zeros_like(xyz, np.float32))


def load_depth_priors(root, cameras, model, device):
    """one [H,W] f32 map per camera from <root>/<NNN>/out_<model>/depth.npy; non-finite -> 0 (invalid)"""
    priors = []
    for k, cam in enumerate(cameras):
        view = os.path.join(root, f"{k:03d}")
        name = model
        if name is None:
            outs = sorted(d for d in os.listdir(view) if d.startswith("out_"))
            if len(outs) != 1:
                raise SystemExit(f"{view}: {len(outs)} out_* folders, name one with --depth-model")
            name = outs[0][4:]
        d = np.nan_to_num(np.load(os.path.join(view, f"out_{name}", "depth.npy")).astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
        if d.shape != (cam.image_height, cam.image_width):
            raise SystemExit(f"{view}: depth.npy is {d.shape}, the camera {cam.image_height} x {cam.image_width}")
        priors.append(torch.from_numpy(np.ascontiguousarray(d)).to(device))
    return priors


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("paths", nargs="+", help="<colmap_dir> <out_dir>, or <out_dir> with --synthetic")
    ap.add_argument("--iterations", type=int, default=30_000)
    ap.add_argument("--resolution-scale", type=float, default=1.0)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--white-background", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--loss", choices=("torch", "fused"), default="torch", help="torch ops (default) or the fused HIP kernels")
    ap.add_argument("--optimizer", choices=("default", "fused", "sparse_adam"), default="default",
                    help="torch.optim.Adam (default), the fused HIP step, or the fused step on the visible rows only")
    ap.add_argument("--synthetic-size", type=int, nargs=4, default=[20000, 4000, 800, 600], metavar=("P_TRUE", "P_INIT", "W", "H"))
    ap.add_argument("--depth-priors", metavar="DIR", help="folder of <NNN>/out_<model>/depth.npy, one per camera")
    ap.add_argument("--depth-model", default=None, help="<model> of out_<model> under --depth-priors")
    ap.add_argument("--lambda-depth", type=float, default=0.0, help="weight of the depth L1 term (needs --depth-priors)")
    ap.add_argument("--depth-kind", choices=["centre", "ray"], default="centre",
                    help="the rendered depth the depth term compares: z of the centres, or the ray-Gaussian intersection depth")
    a = ap.parse_args()
    if (a.lambda_depth > 0) != bool(a.depth_priors):
        ap.error("--depth-priors and a positive --lambda-depth go together")
    if not torch.cuda.is_available():
        raise SystemExit("train_splat needs a GPU")
    device = "cuda"
    if a.synthetic:
        if len(a.paths) != 1:
            ap.error("--synthetic takes <out_dir> only")
        out_dir = a.paths[0]
        n_true, n_init, W, H = a.synthetic_size
        cameras, images, pcd, _, _ = training.synthetic_scene(device, n_true=n_true, n_init=n_init, n_views=24, width=W, height=H,
                                                             focal=1.7 * W, seed=a.seed)
    else:
        if len(a.paths) != 2:
            ap.error("<colmap_dir> <out_dir>")
        out_dir = a.paths[1]
        cameras, images, pcd = load_colmap(a.paths[0], a.resolution_scale, device)
    # schedules written in iterations scale with a short run the way the reference's defaults sit in 30 000
    opt = training.OptimizationParams(iterations=a.iterations, position_lr_max_steps=a.iterations, optimizer_type=a.optimizer,
                                      lambda_depth=a.lambda_depth, depth_kind=a.depth_kind)
    priors = load_depth_priors(a.depth_priors, cameras, a.depth_model, device) if a.depth_priors else None
    if a.iterations < 30_000:
        f = a.iterations / 30_000
        opt.densify_from_iter = max(1, int(500 * f))
        opt.densify_until_iter = int(15_000 * f)
        opt.densification_interval = max(1, int(100 * f)) if a.iterations < 3000 else 100
        opt.opacity_reset_interval = max(opt.densification_interval, int(3000 * f))
    extent = training.cameras_extent(cameras)
    bg = torch.tensor([1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0], device=device)
    torch.manual_seed(a.seed)
    g = GaussianModel(3, device=device)
    g.create_from_pcd(pcd, extent)
    g.training_setup(opt)
    P0 = g.get_xyz.shape[0]
    timing = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = training.train(g, cameras, images, opt, extent=extent, bg=bg, white_background=a.white_background, seed=a.seed,
                            timing=timing, loss=a.loss, depth_priors=priors)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ply_dir = os.path.join(out_dir, "point_cloud", f"iteration_{a.iterations}")
    os.makedirs(ply_dir, exist_ok=True)
    ply = os.path.join(ply_dir, "point_cloud.ply")
    g.save_ply(ply)
    check = GaussianModel(3, device=device)
    check.load_ply(ply)
    assert check.get_xyz.shape[0] == g.get_xyz.shape[0]
    k = max(1, len(losses) // 10)
    split = {name: statistics.fmean(v) for name, v in timing.items()}
    print(json.dumps({
        "ply": ply, "views": len(cameras), "width": cameras[0].image_width, "height": cameras[0].image_height,
        "iterations": a.iterations, "loss_path": a.loss, "optimizer": a.optimizer, "lambda_depth": a.lambda_depth, "depth_kind": a.depth_kind, "gaussians_start": P0, "gaussians_end": int(g.get_xyz.shape[0]),
        "loss_first_tenth": statistics.fmean(losses[:k]), "loss_last_tenth": statistics.fmean(losses[-k:]),
        "wall_ms_per_iteration": 1e3 * wall / max(1, a.iterations),
        "stream_ms_per_iteration": {"render_forward": split["render"], "loss": split["loss"], "backward": split["backward"],
                                    "optimiser_and_densification": split["update"]}}))


if __name__ == "__main__":
    main()
