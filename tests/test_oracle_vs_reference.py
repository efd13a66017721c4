"""The restated oracle (oracle/raster_oracle.c) against the REFERENCE'S OWN KERNELS.

oracle/_ref = cuda_rasterizer/forward.cu + checkFrustum / duplicateWithKeys / identifyTileRanges of
rasterizer_impl.cu, compiled for the CPU from the sources where they lie (oracle/build_ref.py, oracle/ref_shim/),
driven in the order of CudaRasterizer::Rasterizer::forward (rasterizer_impl.cu:198-336).  Both sides are built
-ffp-contract=off, so the bar is BIT-EXACT on every output: radii, means2D, depths, cov3D, rgb, conic/opacity,
tiles_touched, the sorted instance list, the tile ranges and the image.

 * `test_oracle_equals_reference_golden`: against tests/golden/ref_forward.npz (made by tests/golden/make_golden.py
   from the reference build) -- runs everywhere, also where /root/reference does not exist;
 * the other tests: more scenes (SH degrees, precomputed inputs, ragged / crowded tiles) built here from seeds; the
   reference's inputs and outputs are pinned by SHA-256 digests in tests/golden/ref_scenes.json (same script, `--ref-scenes`)
   -- also self-contained, and just as bit-exact."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import oracle
from gs2mesh_amd import synthetic
from gs2mesh_amd.graphics import Camera

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_forward.npz")
SCENES = os.path.join(os.path.dirname(__file__), "golden", "ref_scenes.json")


def _oracle_all(xyz, o, cam_args, W, H, bg, **kw):
    vm, pm, cp, tx, ty = cam_args
    img, radii, n = oracle.rasterize_forward(xyz, o, vm, pm, cp, W, H, tx, ty, bg, **kw)
    kw2 = dict(kw)
    geom = oracle.preprocess(xyz, kw2.pop("scales", None), kw2.pop("rotations", None), o, kw2.pop("shs", None), vm, pm, cp,
                             W, H, tx, ty, **kw2)
    pl, ranges = oracle.bin_instances(geom, W, H)
    return img, radii, n, geom, pl, ranges


def _assert_same(ref, img, radii, n, geom, pl, ranges, cov3d=True):
    assert ref["num_rendered"] == n
    np.testing.assert_array_equal(ref["radii"], radii)
    vis = radii > 0
    keys = ["means2D", "depths", "rgb", "conic_opacity"] + (["cov3D"] if cov3d else [])
    for k in keys:
        np.testing.assert_array_equal(ref[k][vis], geom[k][vis], err_msg=k)
    np.testing.assert_array_equal(ref["tiles_touched"], geom["tiles_touched"])
    np.testing.assert_array_equal(ref["point_list"], pl)
    np.testing.assert_array_equal(ref["ranges"], ranges)
    np.testing.assert_array_equal(ref["color"], img)


def test_oracle_equals_reference_golden():
    z = np.load(GOLD)
    W, H = int(z["W"]), int(z["H"])
    cam = (z["viewmatrix"], z["projmatrix"], z["campos"], float(z["tanfovx"]), float(z["tanfovy"]))
    img, radii, n, geom, pl, ranges = _oracle_all(z["xyz"], z["opacity"], cam, W, H, z["bg"], shs=z["shs"],
                                                  scales=z["scales"], rotations=z["rotations"])
    ref = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    ref["num_rendered"] = int(ref["num_rendered"])
    assert ref["num_rendered"] > 5000 and (ref["radii"] > 0).sum() > 1000
    _assert_same(ref, img, radii, n, geom, pl, ranges)


COMPARED = ("means2D", "depths", "rgb", "conic_opacity", "cov3D")        # compared over the visible Gaussians


def _digest(a):
    a = np.ascontiguousarray(a)
    return [a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]


def output_digests(out):
    """Digest (dtype, shape, SHA-256 of the bytes) of every output the bit-exact comparison covers."""
    vis = out["radii"] > 0
    d = {k: _digest(out[k]) for k in ("color", "radii", "tiles_touched", "point_list", "ranges")}
    d.update({k: _digest(out[k][vis]) for k in COMPARED})
    d["num_rendered"] = int(out["num_rendered"])
    if "mark_visible" in out:
        d["mark_visible"] = _digest(out["mark_visible"])
    return d


def input_digests(sc):
    d = {k: _digest(np.asarray(sc[k], np.float32)) for k in ("xyz", "opacity", "bg")}
    d.update({f"cam{i}": _digest(np.asarray(c, np.float32)) for i, c in enumerate(sc["cam"][:3])})
    d.update(W=int(sc["W"]), H=int(sc["H"]), tanfovx=float(sc["cam"][3]), tanfovy=float(sc["cam"][4]))
    d.update({"kw_" + k: (_digest(np.asarray(v, np.float32)) if isinstance(v, np.ndarray) else v) for k, v in sc["kw"].items()})
    return d


def _ring_scene(P, seed, W, H, f, log_s=math.log(0.03), az=0.3, ring=3.5):
    g = synthetic.synth_v1(P, seed, log_s)
    s, q, o = oracle.activate(g["scaling"], g["rotation"], g["opacity"])
    shs = np.ascontiguousarray(np.concatenate([g["features_dc"], g["features_rest"]], axis=1))
    pose = synthetic.ring_pose(az, ring)
    pose = np.concatenate([pose[0], pose[1][:, None]], axis=1)
    cam, _ = synthetic.stereo_cameras(pose, W, H, f, f, 0.245)
    return g["xyz"], s, q, o, shs, _cam(cam)


def _cam(cam):
    return (cam.world_view_transform, cam.full_proj_transform, cam.camera_center, cam.tanfovx, cam.tanfovy)


def scenes():
    """name -> the inputs of one ref_forward call (``kw`` = its keyword arguments).  "precomputed_cov3d" takes the cov3D that
    "precomputed" produced (None here: filled in by the caller)."""
    out = {}
    W, H = 96, 80
    for deg, M in [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)]:
        xyz, s, q, o, shs, cam = _ring_scene(800, 5, W, H, 90.0)
        out[f"sh_{deg}_{M}"] = dict(xyz=xyz, opacity=o, W=W, H=H, bg=[0, 0, 0], cam=cam,
                                    kw=dict(shs=np.ascontiguousarray(shs[:, :M]), scales=s, rotations=q, sh_degree=deg))
    xyz, s, q, o, shs, cam = _ring_scene(800, 6, W, H, 90.0)
    cols = np.random.default_rng(0).uniform(0, 1, (800, 3)).astype(np.float32)
    out["precomputed"] = dict(xyz=xyz, opacity=o, W=W, H=H, bg=[1, 1, 1], cam=cam,
                              kw=dict(colors_precomp=cols, scales=s, rotations=q, scale_modifier=0.7))
    out["precomputed_cov3d"] = dict(xyz=xyz, opacity=o, W=W, H=H, bg=[1, 1, 1], cam=cam, kw=dict(colors_precomp=cols, cov3D_precomp=None))

    # 1..hundreds of tiles per splat, Gaussians behind / close to the camera (0.2 near cull), ragged tiles
    W, H = 184, 120
    rng = np.random.default_rng(9)
    P = 1500
    xyz = rng.uniform(-1.5, 1.5, (P, 3)).astype(np.float32)
    xyz[:200, 2] = rng.uniform(3.2, 4.5, 200)       # around and behind the camera at z = 4
    s = np.exp(rng.normal(math.log(0.03), 1.2, (P, 3))).astype(np.float32)
    s[:20] *= 30.0                                   # screen-filling splats
    q = rng.normal(0, 1, (P, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    o = rng.uniform(0.005, 1.0, P).astype(np.float32)
    shs = rng.normal(0, 0.4, (P, 16, 3)).astype(np.float32)
    cam = Camera(0, np.eye(3), np.array([0, 0, 4.0]), 2 * math.atan2(W, 2 * 150.0), 2 * math.atan2(H, 2 * 150.0), W, H)
    out["ragged"] = dict(xyz=xyz, opacity=o, W=W, H=H, bg=[0.2, 0.1, 0.0], cam=_cam(cam), kw=dict(shs=shs, scales=s, rotations=q))

    # thousands of instances per tile: early termination (T < 1e-4), > 256-instance batches
    W, H = 48, 32
    P = 6000
    rng = np.random.default_rng(3)
    xyz = rng.normal(0, 0.02, (P, 3)).astype(np.float32)
    xyz[:, 2] = rng.uniform(-1, 1, P)
    cam = Camera(0, np.eye(3), np.array([0, 0, 4.0]), 2 * math.atan2(W, 2 * 60.0), 2 * math.atan2(H, 2 * 60.0), W, H)
    o = rng.uniform(0.02, 0.4, P).astype(np.float32)
    cols = rng.uniform(0, 1, (P, 3)).astype(np.float32)
    s = np.full((P, 3), 0.05, np.float32)
    q = np.tile([1, 0, 0, 0], (P, 1)).astype(np.float32)
    out["crowded"] = dict(xyz=xyz, opacity=o, W=W, H=H, bg=[0, 0, 0], cam=_cam(cam), kw=dict(colors_precomp=cols, scales=s, rotations=q))
    return out


def _check(name, sc, skip=()):
    """The oracle on scene `name` against the reference's kernels (tests/golden/ref_scenes.json, made by
    tests/golden/make_golden.py --ref-scenes from the reference build): inputs and every output bit for bit."""
    gold = json.load(open(SCENES))[name]
    assert input_digests(sc) == gold["inputs"], f"{name}: the scene's inputs changed -- regenerate the digests with the reference build"
    img, radii, n, geom, pl, ranges = _oracle_all(sc["xyz"], sc["opacity"], sc["cam"], sc["W"], sc["H"], sc["bg"], **sc["kw"])
    out = dict(geom, color=img, radii=radii, num_rendered=n, point_list=pl, ranges=ranges)
    got = output_digests(out)
    bad = [k for k in gold["outputs"] if k not in skip and k != "mark_visible" and got[k] != gold["outputs"][k]]
    assert not bad, f"{name}: differs from the reference's kernels in {bad}"
    return out, gold["outputs"]


@pytest.mark.parametrize("deg,M", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)])
def test_sh_degrees(deg, M):
    _check(f"sh_{deg}_{M}", scenes()[f"sh_{deg}_{M}"])


def test_precomputed_inputs_and_scale_modifier():
    sc = scenes()
    # colours are an input here: the reference leaves rgb untouched
    out, _ = _check("precomputed", sc["precomputed"], skip=("rgb",))
    sc2 = sc["precomputed_cov3d"]
    sc2["kw"]["cov3D_precomp"] = out["cov3D"]        # = the reference's cov3D, bit for bit (checked above)
    out2, _ = _check("precomputed_cov3d", sc2, skip=("rgb", "cov3D"))     # cov3D is an input here
    np.testing.assert_array_equal(out2["color"], out["color"])


def test_ragged_image_huge_and_tiny_splats_near_plane():
    """1..hundreds of tiles per splat, Gaussians behind / close to the camera (0.2 near cull), ragged tiles."""
    sc = scenes()["ragged"]
    out, gold = _check("ragged", sc)
    assert 0 < (out["radii"] > 0).sum() < sc["xyz"].shape[0] and out["tiles_touched"].max() > 60
    assert _digest(oracle.mark_visible(sc["xyz"], sc["cam"][0], sc["cam"][1])) == gold["mark_visible"]


def test_crowded_saturating_tiles():
    """Thousands of instances per tile: early termination (T < 1e-4), > 256-instance batches."""
    _check("crowded", scenes()["crowded"], skip=("rgb",))
