"""Device PNG encoder on the MI355X: byte identity with the CPU-emulator build of the same kernel source, full-size renders
against PIL, and the Renderer's device paths (``png_encoder="device"``, ``render_image_pairs``, the writer thread)."""
import io
import os

import numpy as np
import pytest

from test_png_encode import KINDS, SHAPES, check_file, content, emu_lib
from test_pipeline_classes import make_args, write_colmap

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from backends import use_host_memory
    use_host_memory(False)
    return torch


def _emu_encode(imgs, S, filt=4):
    from gs2mesh_amd import _lib
    from gs2mesh_amd.png import PngEncoder
    from backends import HostMemory
    old = _lib.MEMORY
    _lib.MEMORY = HostMemory()
    try:
        e = PngEncoder(0, lib=emu_lib(), rows_per_segment=S, filter=filt)
        files = e.encode(imgs)
        e.close()
        return files
    finally:
        _lib.MEMORY = old


@pytest.mark.parametrize("W,H", SHAPES)
def test_gpu_bytes_equal_emulator_bytes(W, H):
    torch = _torch()
    from gs2mesh_amd.png import PngEncoder
    imgs = np.stack([content(k, H, W) for k in KINDS])
    dev = torch.from_numpy(imgs).cuda()
    for S in sorted({1, 16, H}):
        enc = PngEncoder(0, rows_per_segment=S)
        got = enc.encode(dev)
        ref = _emu_encode(imgs, S)
        assert got == ref
        for k in range(len(KINDS)):
            check_file(got[k], imgs[k], 4)
            assert enc.encode(dev[k])[0] == got[k]          # batch size does not change the bytes
    enc0 = PngEncoder(0, rows_per_segment=16, filter=0)
    assert enc0.encode(dev) == _emu_encode(imgs, 16, filt=0)


def _render_pair(g, cfg, torch):
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.rasterizer import Rasterizer, camera_from
    gd = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    gd["raw"] = True
    pose = synthetic.ring_poses(1, cfg.ring_radius, 3, cfg.n_pairs)[0]
    left, right = synthetic.stereo_cameras(pose, cfg.width, cfg.height, cfg.focal, cfg.focal, cfg.baseline)
    return Rasterizer(0).render_views(gd, [camera_from(left), camera_from(right)], want_color=False, want_rgb8=True)["rgb8"]


@pytest.mark.parametrize("scene", ["synth_v1", "trained_like"])
def test_full_size_c2_pair_decodes_and_beats_pil_level_1(scene):
    torch = _torch()
    from PIL import Image
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.png import PngEncoder
    cfg = synthetic.CONFIGS["C2"]
    g = (synthetic.synth_v1(cfg.P, cfg.seed, cfg.log_s_mu) if scene == "synth_v1" else
         synthetic.trained_like(cfg.P, cfg.seed, cfg.log_s_mu, focal=cfg.focal, ring_radius=cfg.ring_radius))
    rgb8 = _render_pair(g, cfg, torch)
    files = PngEncoder(0).encode(rgb8)
    host = rgb8.cpu().numpy()
    for k in range(2):
        check_file(files[k], host[k], 4)
        buf = io.BytesIO()
        Image.fromarray(host[k], mode="RGB").save(buf, format="PNG", compress_level=1)
        assert len(files[k]) <= 0.95 * buf.tell(), (len(files[k]), buf.tell())


def _scene(tmp_path, n_views=6):
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.gaussian_model import write_gaussian_ply
    cfg = synthetic.CONFIGS["C1"]
    g = synthetic.synth_v1(cfg.P, cfg.seed, cfg.log_s_mu)
    ply_dir = tmp_path / "splatting_output" / "custom" / "scene" / "point_cloud" / "iteration_30000"
    os.makedirs(ply_dir)
    write_gaussian_ply(str(ply_dir / "point_cloud.ply"), g["xyz"], g["features_dc"], g["features_rest"], g["opacity"],
                       g["scaling"], g["rotation"])
    write_colmap(str(tmp_path / "colmap"), synthetic.ring_poses(n_views, cfg.ring_radius), cfg.width, cfg.height, cfg.focal,
                 cfg.focal, cfg.width / 2, cfg.height / 2)
    return cfg


def _renderer(tmp_path, cfg, out, **kw):
    from gs2mesh_amd.renderer_utils import Renderer
    r = Renderer(str(tmp_path), str(tmp_path / "colmap"), str(tmp_path / out),
                 make_args(renderer_baseline_absolute=cfg.baseline, renderer_save_json=False), **kw)
    r.prepare_renderer()
    return r


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_renderer_device_path_writes_the_pil_paths_pixels(tmp_path):
    _torch()
    from PIL import Image
    cfg = _scene(tmp_path)
    dev = _renderer(tmp_path, cfg, "dev", png_encoder="device")
    pil = _renderer(tmp_path, cfg, "pil")
    assert pil.png_encoder == "pil" and dev.png_encoder == "device"
    dev.render_image_pair(1)
    pil.render_image_pair(1)
    for name in ("left", "right"):
        a = np.asarray(Image.open(os.path.join(dev.render_folder_name(1), f"{name}.png")))
        b = np.asarray(Image.open(os.path.join(pil.render_folder_name(1), f"{name}.png")))
        assert a.shape == (cfg.height, cfg.width, 3) and np.array_equal(a, b)
    from argparse import Namespace
    args = make_args(renderer_baseline_absolute=cfg.baseline, renderer_save_json=False, png_encoder="device")
    from gs2mesh_amd.renderer_utils import Renderer
    assert Renderer(str(tmp_path), str(tmp_path / "colmap"), str(tmp_path / "x"), args).png_encoder == "device"
    with pytest.raises(ValueError):
        Renderer(str(tmp_path), str(tmp_path / "colmap"), str(tmp_path / "x"), Namespace(**vars(args)), png_encoder="jpeg")


def test_render_image_pairs_equals_the_per_pair_device_files(tmp_path):
    _torch()
    cfg = _scene(tmp_path)
    one = _renderer(tmp_path, cfg, "one", png_encoder="device")
    many = _renderer(tmp_path, cfg, "many")
    for i in range(5):
        one.render_image_pair(i)
    many.render_image_pairs(range(5))                 # one launch of 4 pairs + a partial launch of 1
    for i in range(5):
        for name in ("left", "right"):
            assert _read(os.path.join(one.render_folder_name(i), f"{name}.png")) == \
                _read(os.path.join(many.render_folder_name(i), f"{name}.png"))
    lazy = _renderer(tmp_path, cfg, "lazy")
    lazy.render_image_pairs(range(5), wait=False)
    lazy.flush()
    for i in range(5):
        d = lazy.render_folder_name(i)
        assert sorted(os.listdir(d)) == ["left.png", "right.png"]     # no .tmp left behind
        assert _read(os.path.join(d, "left.png")) == _read(os.path.join(one.render_folder_name(i), "left.png"))


def test_writer_reports_a_path_it_cannot_create(tmp_path):
    torch = _torch()
    from gs2mesh_amd.png import PngEncoder, PngWriter
    blocker = tmp_path / "a_file"
    blocker.write_bytes(b"x")
    w = PngWriter(PngEncoder(0), max_pending=2)
    img = torch.from_numpy(content("gradient", 16, 17)).cuda()
    w.submit([str(tmp_path / "ok.png")], img)
    w.submit([str(blocker / "left.png")], img)      # parent is a regular file
    with pytest.raises(OSError):
        w.flush()
    with pytest.raises(RuntimeError):
        w.submit([str(tmp_path / "later.png")], img)
    check_file(_read(tmp_path / "ok.png"), content("gradient", 16, 17), 4)
    w.close()
