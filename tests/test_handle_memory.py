"""The native handles' device memory (gs2mesh_amd/csrc/device_memory.h as raster_api.hip, tsdf_api.hip and png_encode.hip use
it), on both back-ends: a handle whose buffers have grown, shrunk in use and been reused computes bit for bit what a fresh
handle computes, and handles can be created and destroyed in any number.

Every comparison is exact: growth must change where the data lives and nothing else."""
import functools

import numpy as np
import pytest

from backends import BACKENDS, make
from gs2mesh_amd.mesh import TriangleMesh
from gs2mesh_amd.png import PngEncoder
from gs2mesh_amd.rasterizer import Rasterizer, camera_from
from test_mesh_edges import VL, make_volume, upload
from test_mesh_extract import scipy_clusters
from test_png_encode import check_file, content, emu_lib
from test_raster_parity import scene


@pytest.fixture(params=BACKENDS)
def be(request):
    return make(request.param)


# ---- rasteriser --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raster_case():
    """~2 000 Gaussians; the small camera (176 x 112) and four views of the large one (320 x 208)"""
    g, s, q, o, shs, small, _ = scene(2000, 31, 176, 112, 160.0)
    big = []
    for az in (0.1, 0.9):
        big += list(scene(2000, 31, 320, 208, 290.0, az=az)[5:7])
    w = np.random.default_rng(5).uniform(-1.0, 1.0, (3, 112, 176)).astype(np.float32)
    return dict(g=g, s=s, q=q, o=o, shs=shs, small=small, big=big, w=w)


def render(be, r, c, cams):
    g = c["g"]
    gd = dict(xyz=be.dev(g["xyz"]), scaling=be.dev(g["scaling"]), rotation=be.dev(g["rotation"]), opacity=be.dev(g["opacity"]),
              features_dc=be.dev(g["features_dc"]), features_rest=be.dev(g["features_rest"]), raw=True, sh_degree=3)
    res = r.render_views(gd, [camera_from(cam) for cam in cams], bg=(0.1, 0.2, 0.3), want_radii=True)
    return be.host(res["color"]).copy(), be.host(res["radii"]).copy(), list(res["num_rendered"])


def forward_backward(be, r, c):
    d, cam = be.dev, c["small"]
    common = (d(cam.world_view_transform), d(cam.full_proj_transform), d(cam.camera_center), d(np.array([0.1, 0.2, 0.3], np.float32)),
              176, 112, cam.tanfovx, cam.tanfovy)
    xyz, kw = d(c["g"]["xyz"]), dict(shs=d(c["shs"]), scales=d(c["s"]), rotations=d(c["q"]))
    img, radii = r.forward(xyz, d(c["o"].reshape(-1)), *common, **kw)
    g = r.backward(d(c["w"]), xyz, *common, want_conic=True, **kw)
    be.sync()
    return be.host(img).copy(), be.host(radii).copy(), {k: be.host(v).copy() for k, v in g.items()}, r.backward_rows()


def assert_same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y)
        elif isinstance(x, dict):
            assert x.keys() == y.keys()
            for k in x:
                np.testing.assert_array_equal(x[k], y[k], err_msg=k)
        else:
            assert x == y


def test_raster_handle_regrown_equals_fresh(be):
    c = raster_case()
    r = Rasterizer(0, lib=be.lib)
    first = render(be, r, c, [c["small"]])
    assert first[2][0] > 2000 and (first[1] > 0).sum() > 500
    # two views per pass and a larger image: records, masks, histograms, tile arrays and class lists all outgrow what one small view
    # left (more than its 1/8 headroom); the instance count does the same for the key arrays
    r.reserve(2000, 4, 320, 208, 400_000)
    big = render(be, r, c, c["big"])
    assert big[0].shape == (4, 3, 208, 320) and min(big[2]) > 2000
    again = render(be, r, c, [c["small"]])
    fresh_r = Rasterizer(0, lib=be.lib)
    fresh = render(be, fresh_r, c, [c["small"]])
    assert_same(again, first)
    assert_same(again, fresh)
    grown = forward_backward(be, r, c)
    new = forward_backward(be, Rasterizer(0, lib=be.lib), c)
    assert grown[3][0] > 0 and grown[3][1] >= grown[3][0] * 4 and any(v.any() for v in grown[2].values())
    assert_same(grown, new)


# ---- handle churn ------------------------------------------------------------------------------------------------------------
def plane_field(keys, z0=0.37, ax=0.3, ay=-0.2):
    """a tilted plane through the blocks `keys`, weight 1, colours from the position -> (tsdf, w, col) in (x, y, z) index order"""
    x, y, z = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    tsdf, col = [], []
    for k in np.asarray(keys):
        px, py, pz = ((k[0] * 16 + x + 0.5) * VL, (k[1] * 16 + y + 0.5) * VL, (k[2] * 16 + z + 0.5) * VL)
        f = np.clip((pz + ax * px + ay * py - z0) / (4 * VL), -1, 1)
        tsdf.append(np.round(f * 256).reshape(-1) / 256)       # multiples of 1 / 256: exact in the sum form
        col.append(np.stack([(k[0] * 16 + x) % 256, (k[1] * 16 + y) % 256, (k[2] * 16 + z) % 256], -1).reshape(-1, 3))
    tsdf = np.asarray(tsdf, np.float32)
    return tsdf, np.ones_like(tsdf), np.asarray(col)


SMALL_KEYS = np.array([[0, 0, 0], [1, 0, 0]], np.int32)
LARGE_KEYS = np.array([[bx, by, bz] for bx in range(4) for by in range(4) for bz in range(2)], np.int32)   # 32 blocks


def extract(be, vol, keys):
    vol.reset()
    tsdf, w, col = plane_field(keys)
    for b in range(len(keys)):      # one block per call: the pool hands its slots out in this order, whichever workgroup runs first
        upload(be, vol, keys[b:b + 1], tsdf[b:b + 1], w[b:b + 1], col[b:b + 1])
    m = vol.extract_triangle_mesh()
    return m.vertices.copy(), m.triangles.copy(), m.vertex_colors.copy(), m.edge_index.copy()


def png_lib(be):
    """the library with the PNG encoder on this back-end: the emulator builds png_encode.hip into a library of its own"""
    return be.lib if be.name == "gpu" else emu_lib()


def png_files(be, enc, imgs):
    return enc.encode(be.dev(imgs))


def test_handles_created_and_destroyed_repeatedly(be):
    c = raster_case()
    img = content("blobs", 24, 40)[None]
    results = []
    for i in range(9):
        r = Rasterizer(0, lib=be.lib)
        vol = make_volume(be, max_blocks=64)
        enc = PngEncoder(0, lib=png_lib(be))
        if i in (0, 8):
            results.append((render(be, r, c, [c["small"]]), extract(be, vol, SMALL_KEYS), png_files(be, enc, img)))
        r.close()
        vol.close()
        enc.close()
    (ras0, mesh0, png0), (ras8, mesh8, png8) = results
    assert_same(ras8, ras0)
    assert_same(mesh8, mesh0)
    assert png8 == png0 and len(png0) == 1
    check_file(png0[0], img[0], 4)
    assert mesh0[1].shape[0] > 500 and ras0[2][0] > 2000


# ---- TSDF mesh cache and the per-device scratch ---------------------------------------------------------------------------------
def test_mesh_buffers_regrown_equal_first_use(be):
    vol = make_volume(be, max_blocks=64)
    small = extract(be, vol, SMALL_KEYS)
    large = extract(be, vol, LARGE_KEYS)
    assert large[1].shape[0] > 2 * small[1].shape[0] > 2000      # well past the 1 / 8 headroom of the small mesh's buffers
    assert_same(extract(be, vol, SMALL_KEYS), small)
    assert_same(extract(be, vol, LARGE_KEYS), large)
    assert_same(extract(be, make_volume(be, max_blocks=64), SMALL_KEYS), small)
    # clustering and normals share one arena per device: alternate them on the large, the small and the large mesh
    for v, t, _, _ in (large, small, large):
        m = TriangleMesh(v, t)
        labels, counts, _ = m.cluster_connected_triangles(lib=be.lib)
        ref_labels, ref_counts = scipy_clusters(m)
        np.testing.assert_array_equal(labels, ref_labels)
        np.testing.assert_array_equal(counts, ref_counts)
        h = TriangleMesh(v, t).compute_vertex_normals()
        d = TriangleMesh(v, t).compute_vertex_normals(on_device=True, lib=be.lib)
        np.testing.assert_array_equal(d.triangle_normals, h.triangle_normals)
        np.testing.assert_array_equal(d.vertex_normals, h.vertex_normals)


# ---- PNG scratch ---------------------------------------------------------------------------------------------------------------
def test_png_scratch_regrown_equals_first_use(be):
    small = content("blobs", 48, 64)[None]
    big = np.stack([content(k, 192, 256) for k in ("blobs", "gradient", "noise", "blobs")])
    enc = PngEncoder(0, lib=png_lib(be))
    first = png_files(be, enc, small)
    many = png_files(be, enc, big)
    again = png_files(be, enc, small)
    assert again == first and len(first) == 1 and len(many) == 4
    check_file(first[0], small[0], 4)
    for k in range(4):
        check_file(many[k], big[k], 4)
    assert png_files(be, PngEncoder(0, lib=png_lib(be)), small) == first
