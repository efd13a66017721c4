"""Depth without a matcher, above the C ABI (no GPU, no HIP library): ``render(..., return_depth=)``,
``GaussianRasterizer.depth_maps`` and ``RenderedDepth``'s on-disk layout, with a stub renderer and the CPU emulator build of the
kernels behind the operator module's handle."""
import os

import numpy as np
import pytest
import torch
from PIL import Image as PILImage

from rendered_depth_scene import SplatScene, np_of, sphere_hit, tsdf_args

W, H, F, P, VIEWS = 96, 72, 180.0, 1200, 3
OLD_KEYS = {"render", "viewspace_points", "visibility_filter", "radii"}


@pytest.fixture()
def emu(monkeypatch):
    """the operator module's per-device handle -> one Rasterizer on the emulator library; host memory policy"""
    from backends import make
    from gs2mesh_amd import _lib
    from gs2mesh_amd import diff_gaussian_rasterization as dgr
    from gs2mesh_amd.rasterizer import Rasterizer
    old = _lib.MEMORY
    be = make("emu")
    h = Rasterizer(0, lib=be.lib)
    monkeypatch.setattr(dgr, "_handle", lambda device: h)
    yield h
    _lib.MEMORY = old


@pytest.fixture()
def scene(tmp_path):
    return SplatScene(tmp_path, VIEWS, W, H, F, P, "cpu", bg=(0.1, 0.2, 0.3))


def test_render_without_return_depth_has_exactly_the_old_keys(emu, scene):
    from gs2mesh_amd.gaussian_renderer import render
    cam, pc, bg = scene.left_view(0)
    with torch.no_grad():
        plain = render(cam, pc, None, bg)
        plain_kw = render(cam, pc, None, bg, return_depth=False)
        deep = render(cam, pc, None, bg, return_depth=True)
    assert set(plain) == set(plain_kw) == OLD_KEYS
    assert set(deep) == OLD_KEYS | {"depth", "median_depth", "alpha"}
    assert torch.equal(deep["render"], plain["render"]) and torch.equal(deep["radii"], plain["radii"])
    for k in ("depth", "median_depth", "alpha"):
        assert deep[k].shape == (H, W) and deep[k].dtype == torch.float32 and not deep[k].requires_grad
    hit = sphere_hit(scene, 0)
    alpha, med, exp = (np_of(deep[k]) for k in ("alpha", "median_depth", "depth"))
    assert ((med > 0) == (alpha >= 0.5)).all()
    inner = hit & (alpha >= 0.5)
    assert inner.sum() > 0.5 * hit.sum(), "the splat covers most of the sphere's silhouette"
    # the sphere spans z = 2.9 .. 4.1 from a camera on the ring of radius 3.5; its front half, 2.9 .. 3.5, is what most pixels see
    # (a few look through a gap between the front splats at the back ones)
    for d in (med, exp):
        assert d[inner].min() > 2.8 and d[inner].max() < 4.2 and np.median(d[inner]) < 3.5
    assert not alpha[0, 0] and not med[0, 0] and not exp[0, 0], "nothing in the corner"


def test_depth_maps_replays_its_own_forward(emu, scene):
    """forward A, forward B on the same handle, then A.depth_maps(): A's maps"""
    import math
    from gs2mesh_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    pc = scene.gaussians

    def rasterizer(i):
        cam = scene.camera(i)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous()
        return GaussianRasterizer(GaussianRasterizationSettings(
            H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), scene.background, 1.0, t(cam.world_view_transform),
            t(cam.full_proj_transform), 3, t(cam.camera_center), False, False))

    def run(r):
        return r(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), opacities=pc.get_opacity, shs=pc.get_features,
                 scales=pc.get_scaling, rotations=pc.get_rotation)

    ra, rb = rasterizer(0), rasterizer(1)
    with pytest.raises(RuntimeError, match="has not run a forward"):
        ra.depth_maps()
    with torch.no_grad():
        out = run(ra)
        assert isinstance(out, tuple) and len(out) == 2, "(color, radii), as the reference returns"
        first = ra.depth_maps()
        run(rb)
        calls = emu.state_calls
        again = ra.depth_maps()
        assert emu.state_calls == calls + 1, "the forward was replayed"
        other = rb.depth_maps(want=("alpha",))
    assert set(first) == {"expected", "median", "alpha"} and set(other) == {"alpha"}
    for k in first:
        assert torch.equal(first[k], again[k]), k
    assert not torch.equal(other["alpha"], first["alpha"])


def test_rendered_depth_is_named_render():
    from gs2mesh_amd.depth_utils import RenderedDepth
    assert RenderedDepth.model_name == "RENDER"
    rd = RenderedDepth("base", None, None)
    assert rd.model_name == "RENDER" and rd.kind == "median" and rd.alpha_min == 0.5
    with pytest.raises(ValueError, match="kind"):
        RenderedDepth("base", None, None, kind="mean")
    with pytest.raises(RuntimeError, match="was not kept"):
        rd.frame_source(0)


@pytest.mark.parametrize("kind,alpha_min", [("median", 0.5), ("expected", 0.8)])
def test_rendered_depth_writes_the_layout_tsdf_reads(emu, scene, kind, alpha_min):
    from gs2mesh_amd.depth_utils import RenderedDepth
    from gs2mesh_amd.gaussian_renderer import render
    from gs2mesh_amd.tsdf_utils import TSDF
    args = tsdf_args()
    rd = RenderedDepth(scene.output_dir_root, scene, args, device="cpu", kind=kind, alpha_min=alpha_min)
    calls = emu.state_calls
    rd.run(start=1, keep_on_device=True, write_files=True)
    rd.close()
    assert emu.state_calls == calls + (VIEWS - 1), "ONE forward per left camera"
    assert sorted(rd.frames) == [1, 2] and not os.path.exists(scene.render_folder_name(0))
    tsdf = TSDF(scene, rd, args, "mesh")
    assert tsdf.model_name == "RENDER"
    for i in (1, 2):
        d = scene.render_folder_name(i)
        assert sorted(os.listdir(d)) == ["left.png", "out_RENDER"]
        assert sorted(os.listdir(os.path.join(d, "out_RENDER"))) == ["depth.npy", "occlusion_mask.npy"]
        cam, pc, bg = scene.left_view(i)
        with torch.no_grad():
            ref = render(cam, pc, None, bg, return_depth=True)
        depth = np.load(os.path.join(d, "out_RENDER", "depth.npy"))
        occ = np.load(os.path.join(d, "out_RENDER", "occlusion_mask.npy"))
        png = np.array(PILImage.open(os.path.join(d, "left.png")))
        assert depth.dtype == np.float32 and depth.shape == (H, W) and occ.dtype == np.bool_ and png.shape == (H, W, 3)
        assert np.array_equal(depth, np_of(ref["median_depth" if kind == "median" else "depth"]))
        assert np.array_equal(occ, np_of(ref["alpha"]) >= np.float32(alpha_min)) and occ.any() and not occ.all()
        want = np.floor(np.clip(np_of(ref["render"]).transpose(1, 2, 0), 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
        assert np.array_equal(png, want)
        fr = rd.frame_source(i)                 # the in-memory frame is the written one
        assert np.array_equal(np_of(fr["image"]), png) and np.array_equal(np_of(fr["depth"]), depth)
        assert np.array_equal(np_of(fr["occlusion"]).astype(bool), occ)
        disk = tsdf._load_frame(i)              # and TSDF reads it back
        assert np.array_equal(disk["image"], png) and np.array_equal(disk["depth"], depth) and np.array_equal(disk["occlusion"], occ)
    rd2 = RenderedDepth(scene.output_dir_root, scene, args, device="cpu")
    rd2.run(start=2, keep_on_device=True, write_files=False)
    assert sorted(rd2.frames) == [2] and rd2._writer is None


def test_renderer_left_view_is_the_left_camera_of_the_pair(tmp_path):
    """the accessor RenderedDepth reads: the 3DGS camera ``_pair`` builds for the left eye, the model and the background"""
    from gs2mesh_amd import synthetic
    from gs2mesh_amd.rasterizer import camera_from
    from gs2mesh_amd.renderer_utils import Renderer
    from test_pipeline_classes import make_args, write_colmap
    write_colmap(str(tmp_path / "colmap"), synthetic.ring_poses(4, 3.5), 64, 48, 60, 60, 32, 24)
    r = Renderer(str(tmp_path), str(tmp_path / "colmap"), str(tmp_path / "out"), make_args(renderer_save_json=False))
    with pytest.raises(RuntimeError, match="prepare_renderer"):
        r.left_view(0)
    r._raster, r.gaussians, r.background = object(), "model", "background"      # what prepare_renderer sets, without a device
    for i in range(len(r)):
        cam, model, bg = r.left_view(i)
        assert model == "model" and bg == "background"
        got, want = camera_from(cam), r._pair(i)[0]
        assert bytes(got) == bytes(want)
