"""The mesh stage at its edges, on both back-ends: marching cubes over the block-sparse volume (tsdf_extract.h), the device weld,
scan, clustering and vertex normals (mesh_kernels.h) and their host entry points (tsdf_api.hip).

References: the restated Open3D volume (oracle.ScalableTSDFVolume.import_state -> extract_triangle_mesh) for the extraction, the
host weld (TriangleMesh.from_triangle_soup), scipy connected components (scipy_clusters), the numpy compute_vertex_normals, and
closed forms.  Device state is injected with unpack_sum (sum form [n, 5, 4096], device voxel layout); voxel length 1 / 32,
truncation 4 / 32.

Comparison bar of the extraction (the one test_exact_zero_tsdf_values_keep_open3ds_vertices_apart uses): numbering-independent form
with the vertices ordered by their edge key on both sides; vertices float64 bit for bit, triangles exactly, colours to 1e-12
absolute (the oracle divides Open3D's double running mean by 255, the device the integer colour sum by the weight first).

Thresholds pinned here: 1024 blocks (k_mc_scan: blocks per thread 1 -> 2), the 4096-item scan tile and the 4096 x 1024 items
after which k_scan_sums carries between iterations (gs2m_launch_scan_u32, shared by weld, clustering and normals), 1 048 576 items
(grid_for caps at 4096 workgroups: second grid-stride round) and the 2^20-voxel span of the 62-bit weld key."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

from gs2mesh_amd import _lib
from gs2mesh_amd.integration import ScalableTSDFVolume, TSDFVolumeColorType
from gs2mesh_amd.mesh import TriangleMesh
from gs2mesh_amd.rasterizer import _ptr, _stream_of
from test_mesh_extract import canonical_mesh, extract_soup, scipy_clusters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VL = 1.0 / 32
_x, _y, _z = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
# device position of voxel (x, y, z), listed in the (x, y, z) index order x * 256 + y * 16 + z of Open3D's IndexOf
VIDX = (((_z >> 2) * 16 + (_x >> 2) * 4 + (_y >> 2)) * 64 + (_z & 3) * 16 + (_x & 3) * 4 + (_y & 3)).reshape(-1)
L_KEYS = np.array([[-2, -1, -1], [-1, -1, -1], [-1, 0, -1], [-1, -1, 0], [0, 0, 0], [-2, -1, 0]], np.int32)   # six blocks in an L
L_HALO = (1, 3)                                                                                              # case 2: uploaded halo=True


def mc_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mc_classic_table
    return mc_classic_table


def make_volume(be, max_blocks=64, color_type=TSDFVolumeColorType.RGB8):
    return ScalableTSDFVolume(VL, 4 * VL, color_type, max_blocks=max_blocks, lib=be.lib)


def upload(be, vol, keys, tsdf, w, col, halo=False):
    """keys [n, 3]; tsdf / w [n, 4096] f32 and col [n, 4096, 3] (0..255) in (x, y, z) index order -> the volume's blocks"""
    n = len(keys)
    buf = np.zeros((n, 5, 4096), np.float32)
    buf[:, 0, VIDX] = tsdf * w                  # exact for the fields below (k / 256 times an integer <= 8; w == 1 elsewhere)
    buf[:, 1, VIDX] = w
    for c in range(3):
        buf[:, 2 + c, VIDX] = col[:, :, c].astype(np.float32) * w
    vol.unpack_sum(be.dev(np.ascontiguousarray(keys, np.int32)), be.dev(buf), halo=halo)


def oracle_mesh(keys, tsdf, w, col, color_type=1):
    import oracle
    ref = oracle.ScalableTSDFVolume(VL, 4 * VL, color_type)
    ref.import_state(keys, tsdf, w, col.astype(np.float64))
    return ref.extract_triangle_mesh(mc_table().T)


def assert_full_bar(mesh, om, colors=True):
    """the comparison bar of the module docstring, and the vertex keys themselves"""
    assert mesh.vertices.shape == om["vertices"].shape and mesh.triangles.shape == om["triangles"].shape
    assert om["triangles"].shape[0] > 0
    ov, oc, ot = canonical_mesh(om["vertices"], om["colors"], om["triangles"], vertex_key=om["edge_index"])
    v, c, t = canonical_mesh(mesh.vertices, mesh.vertex_colors if colors else None, mesh.triangles, vertex_key=mesh.edge_index)
    np.testing.assert_array_equal(v, ov)
    np.testing.assert_array_equal(t, ot)
    if colors:
        np.testing.assert_allclose(c, oc, rtol=0, atol=1e-12)
    order = lambda e: e[np.lexsort((e[:, 3], e[:, 2], e[:, 1], e[:, 0]))]
    np.testing.assert_array_equal(order(mesh.edge_index), order(om["edge_index"]))


def cube_cases(keys, tsdf, w):
    """From the field alone: the case index of the cube based at every voxel [n, 16, 16, 16] (corner i at the voxel +
    CORNER[i], bit i set where tsdf < 0), -1 where one of its eight corners is absent or has weight 0."""
    corner = mc_table().CORNER.astype(int)
    slot = {tuple(k): i for i, k in enumerate(np.asarray(keys).tolist())}
    out = np.full((len(keys), 16, 16, 16), -1, np.int32)
    for b, k in enumerate(np.asarray(keys).tolist()):
        f17, w17 = np.zeros((17, 17, 17), np.float32), np.zeros((17, 17, 17), np.float32)
        for d in itertools.product((0, 1), repeat=3):
            j = slot.get((k[0] + d[0], k[1] + d[1], k[2] + d[2]))
            if j is None:
                continue
            dst = tuple(slice(16, 17) if a else slice(0, 16) for a in d)
            src = tuple(slice(0, 1) if a else slice(0, 16) for a in d)
            f17[dst] = tsdf[j].reshape(16, 16, 16)[src]
            w17[dst] = w[j].reshape(16, 16, 16)[src]
        ok = np.ones((16, 16, 16), bool)
        ci = np.zeros((16, 16, 16), np.int32)
        for i, (sx, sy, sz) in enumerate(corner):
            ok &= w17[sx:sx + 16, sy:sy + 16, sz:sz + 16] > 0
            ci |= (f17[sx:sx + 16, sy:sy + 16, sz:sz + 16] < 0).astype(np.int32) << i
        out[b] = np.where(ok, ci, -1)
    return out


@functools.lru_cache(maxsize=None)
def holed_field():
    """Case 1's field (shared, never written to): random sign times k / 256, k in 1..254; weight 0 with probability 0.03, else
    an integer 1..8; random colours; with it the cube cases and the oracle's meshes with and without colour."""
    rng = np.random.default_rng(1)
    n = len(L_KEYS)
    k = rng.integers(1, 255, (n, 4096))
    sign = rng.choice(np.array([-1.0, 1.0]), (n, 4096))
    tsdf = (sign * k / 256.0).astype(np.float32)
    w = np.where(rng.random((n, 4096)) < 0.03, 0, rng.integers(1, 9, (n, 4096))).astype(np.float32)
    col = rng.integers(0, 256, (n, 4096, 3))
    return dict(keys=L_KEYS, tsdf=tsdf, w=w, col=col, cases=cube_cases(L_KEYS, tsdf, w),
                om={ct: oracle_mesh(L_KEYS, tsdf, w, col, ct) for ct in (0, 1)})


def holed_volume(be, color_type=TSDFVolumeColorType.RGB8, halo=()):
    F = holed_field()
    vol = make_volume(be, color_type=color_type)
    own = [b for b in range(len(L_KEYS)) if b not in halo]
    upload(be, vol, F["keys"][own], F["tsdf"][own], F["w"][own], F["col"][own])
    if halo:
        h = list(halo)
        upload(be, vol, F["keys"][h], F["tsdf"][h], F["w"][h], F["col"][h], halo=True)
    return vol


# ---- A. extraction against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_type", [TSDFVolumeColorType.RGB8, TSDFVolumeColorType.NoColor])
def test_every_cube_case_with_holes_absent_neighbours_and_negative_keys(backend, color_type):
    """Case 1.  Random signs visit all 254 surface rows of the table (saddles included); the holes and the open sides of the L
    take the `slot < 0` / `w == 0` exits of mc_cube_case and the absent-neighbour and negative-key lookups of
    mc_neighbour_slots.  Without colour: the same geometry, and the colours the device mesh holds are all zero."""
    F = holed_field()
    cases = F["cases"]
    hist = np.bincount(cases[cases >= 0], minlength=256)
    print("least visited surface case:", int(hist[1:255].min()), "| cubes skipped:", float((cases < 0).mean()))
    assert hist[1:255].min() >= 20                      # every surface case at least 20 times
    assert (cases < 0).mean() <= 0.40                   # at most 40 % of the cubes skipped
    ntri = np.array([len(r) // 3 for r in mc_table().T])
    om = F["om"][int(color_type)]
    assert om["triangles"].shape[0] == int(ntri[cases[cases >= 0]].sum())
    vol = holed_volume(backend, color_type)
    mesh = vol.extract_triangle_mesh()
    assert mesh.vertices.shape[0] == om["vertices"].shape[0] and mesh.triangles.shape[0] == om["triangles"].shape[0]
    if color_type == TSDFVolumeColorType.RGB8:
        assert_full_bar(mesh, om)
        return
    assert_full_bar(mesh, om, colors=False)
    assert not om["colors"].any() and mesh.vertex_colors.shape == (0, 3)
    cols = np.full((mesh.vertices.shape[0], 3), -7.5)
    st = _lib.MEMORY.current_stream(vol.device)
    _lib.check(vol._lib.gs2m_tsdf_mesh_copy(vol._h, st, None, C.c_void_p(cols.ctypes.data), None, None), vol._lib)
    assert not cols.any()


def keyed_triangles(edge_index, triangles):
    """triangles as rows of their three vertex keys [nt, 12], rotated so that the smallest key comes first (winding kept)"""
    k = np.asarray(edge_index, np.int64)[np.asarray(triangles, np.int64)]                     # [nt, 3, 4]
    s = ((k[:, :, 0] * 4096 + k[:, :, 1]) * 4096 + k[:, :, 2]) * 4 + k[:, :, 3]               # |voxel index| < 2048 here
    first = s.argmin(axis=1)
    rows = np.arange(len(k))
    return np.concatenate([k[rows, (first + j) % 3] for j in range(3)], axis=1)


def test_halo_blocks_supply_corners_and_start_no_cube(backend):
    """Case 2.  Blocks 1 and 3 of case 1's field are uploaded halo=True.  Expected: the oracle's full mesh restricted to the
    triangles whose base cube lies in a non-halo block.  The base block comes from the reference side alone: the oracle walks the
    blocks in import order and the cubes of a block in (x, y, z) order, so the per-cube triangle counts (case index from the
    field -> table row length) cut its triangle list into blocks."""
    F = holed_field()
    om, cases = F["om"][1], F["cases"]
    ntri = np.array([len(r) // 3 for r in mc_table().T])
    per_block = np.where(cases >= 0, ntri[np.maximum(cases, 0)], 0).reshape(len(L_KEYS), -1).sum(axis=1)
    assert per_block.sum() == om["triangles"].shape[0] and (per_block[list(L_HALO)] > 100).all()
    base_block = np.repeat(np.arange(len(L_KEYS)), per_block)
    in_halo = np.isin(base_block, L_HALO)
    full = keyed_triangles(om["edge_index"], om["triangles"])
    assert len(np.unique(full, axis=0)) == len(full)            # a triangle names its base cube: no two cubes emit the same one
    used = np.unique(om["triangles"][~in_halo])
    remap = np.full(om["vertices"].shape[0], -1, np.int64)
    remap[used] = np.arange(len(used))
    expect = dict(vertices=om["vertices"][used], colors=om["colors"][used], edge_index=om["edge_index"][used],
                  triangles=remap[om["triangles"][~in_halo]].astype(np.int32))
    # a halo block's own corners are still read: triangles of non-halo cubes reach into blocks 1 and 3
    lo = np.asarray(expect["edge_index"][:, :3]) >> 4
    assert any((lo == L_KEYS[h]).all(axis=1).any() for h in L_HALO)

    mesh = holed_volume(backend, halo=L_HALO).extract_triangle_mesh()
    assert mesh.triangles.shape[0] == int((~in_halo).sum())
    got = set(map(bytes, keyed_triangles(mesh.edge_index, mesh.triangles)))
    assert got <= set(map(bytes, full))
    assert not got & set(map(bytes, full[in_halo]))
    assert_full_bar(mesh, expect)


@functools.lru_cache(maxsize=None)
def scattered_field():
    """Case 3: 1100 blocks scattered along a line, weight 1, tsdf +0.5 with one random voxel per block at -0.25"""
    rng = np.random.default_rng(3)
    i = np.arange(1100)
    keys = np.stack([i - 550, (7 * i) % 13 - 6, (3 * i) % 5], axis=1).astype(np.int32)
    tsdf = np.full((1100, 4096), 0.5, np.float32)
    tsdf[i, rng.integers(0, 4096, 1100)] = -0.25
    return keys, tsdf, np.ones((1100, 4096), np.float32), rng.integers(0, 256, (1100, 4096, 3)).astype(np.uint8)


@pytest.mark.parametrize("n_blocks", [1024, 1025, 1100])
def test_more_than_1024_blocks(backend, n_blocks):
    """Case 3.  k_mc_scan is one workgroup of 1024 threads: up to 1024 blocks each thread owns one, from 1025 on two."""
    keys, tsdf, w, col = (a[:n_blocks] for a in scattered_field())
    vol = make_volume(backend, max_blocks=2048)
    upload(backend, vol, keys, tsdf, w, col)
    assert vol.num_blocks == n_blocks
    assert_full_bar(vol.extract_triangle_mesh(), oracle_mesh(keys, tsdf, w, col))


F_CANARY, I_CANARY = -12345.678, -7777777


def raw_extract(be, vol, max_tris, rows, colors=True, edge_index=True, indexed=True):
    """gs2m_tsdf_extract[_indexed] into canary-filled buffers of `rows` triangles -> (count, vertices, colours, edge_index)"""
    v = be.dev(np.full((rows, 3, 3), F_CANARY))
    c = be.dev(np.full((rows, 3, 3), F_CANARY)) if colors else None
    e = be.dev(np.full((rows, 3, 4), I_CANARY, np.int32)) if edge_index else None
    got = C.c_int64(-1)
    if indexed:
        rc = vol._lib.gs2m_tsdf_extract_indexed(vol._h, _stream_of(v, None), int(max_tris), _ptr(v), _ptr(c), _ptr(e), C.byref(got))
    else:
        rc = vol._lib.gs2m_tsdf_extract(vol._h, _stream_of(v, None), int(max_tris), _ptr(v), _ptr(c), C.byref(got))
    _lib.check(rc, vol._lib)
    vol.status()
    return int(got.value), be.host(v), be.host(c), be.host(e)


def test_truncated_and_optional_outputs_of_the_c_abi(backend):
    """Case 4.  max_triangles below, at and above the count (the `out >= max_tris` guard of k_mc_emit): the count is always the
    full one, the emitted prefix is the prefix of the full soup, every row behind it is untouched.  colors == NULL,
    edge_index == NULL and gs2m_tsdf_extract give the same vertices; a volume without colour writes zero colours."""
    be = backend
    vol = holed_volume(be)
    sv, sc, se = extract_soup(vol)
    n = sv.shape[0]
    assert n == holed_field()["om"][1]["triangles"].shape[0]
    for mx in (0, 1, n // 2, n - 1, n, n + 5):
        got, v, c, e = raw_extract(be, vol, mx, n + 5)
        k = min(mx, n)
        assert got == n
        np.testing.assert_array_equal(v[:k], sv[:k])
        np.testing.assert_array_equal(c[:k], sc[:k])
        np.testing.assert_array_equal(e[:k], se[:k])
        assert (v[k:] == F_CANARY).all() and (c[k:] == F_CANARY).all() and (e[k:] == I_CANARY).all()
    for kw in (dict(colors=False), dict(edge_index=False), dict(colors=False, edge_index=False), dict(indexed=False),
               dict(indexed=False, colors=False)):
        got, v, c, e = raw_extract(be, vol, n, n + 5, **kw)
        assert got == n
        np.testing.assert_array_equal(v[:n], sv)
        assert (v[n:] == F_CANARY).all()
        if c is not None:
            np.testing.assert_array_equal(c[:n], sc)
            assert (c[n:] == F_CANARY).all()
        if e is not None:
            if kw.get("indexed", True):
                np.testing.assert_array_equal(e[:n], se)
            else:
                assert (e == I_CANARY).all()         # gs2m_tsdf_extract has no edge_index: the buffer was never handed over
    # colourless volume: same triangles (block slots may be numbered differently: compared as sorted rows), zero colours
    plain = holed_volume(be, TSDFVolumeColorType.NoColor)
    got, v, c, e = raw_extract(be, plain, n - 1, n + 5)
    assert got == n and not c[:n - 1].any() and (c[n - 1:] == F_CANARY).all() and (v[n - 1:] == F_CANARY).all()
    got, v, c, e = raw_extract(be, plain, n, n + 5)
    rows = lambda a: a[np.lexsort(a.reshape(len(a), -1).T[::-1])]
    np.testing.assert_array_equal(rows(v[:n]), rows(sv))
    np.testing.assert_array_equal(rows(e[:n]), rows(se))


def test_exact_zeros_and_negative_zero(backend):
    """Case 5.  -0.0f is not < 0: it counts as outside like +0.0.  Corners at either zero next to negative ones put the vertex
    on the corner (offset 0 or the whole edge); the oracle keeps such vertices apart by edge key, and so must the device."""
    rng = np.random.default_rng(5)
    keys = np.array([[bx, by, bz] for bx in (-1, 0) for by in (-1, 0) for bz in (-1, 0)], np.int32)
    n = len(keys)
    values = np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5], np.float32)
    tsdf = values[rng.integers(0, len(values), (n, 4096))]
    assert (np.signbit(tsdf) & (tsdf == 0)).sum() > 1000 and (~np.signbit(tsdf) & (tsdf == 0)).sum() > 1000
    w = np.ones((n, 4096), np.float32)
    col = rng.integers(0, 256, (n, 4096, 3))
    om = oracle_mesh(keys, tsdf, w, col)
    assert om["zero_offset_vertices"] > 0
    vol = make_volume(backend)
    upload(backend, vol, keys, tsdf, w, col)
    dk, dt, _, _ = vol.download()
    order = {tuple(k): i for i, k in enumerate(dk.tolist())}
    dt = dt[[order[tuple(k)] for k in keys.tolist()]]
    np.testing.assert_array_equal(np.signbit(dt), np.signbit(tsdf))       # the injected field kept its negative zeros
    assert_full_bar(vol.extract_triangle_mesh(), om)


# ---- B. weld -----------------------------------------------------------------------------------------------------------------
def test_device_weld_equals_host_weld_in_negative_voxel_space(backend):
    """Case 6.  gs2m_tsdf_extract_mesh == TriangleMesh.from_triangle_soup(gs2m_tsdf_extract_indexed) on case 1's field: dense in
    distinct keys, voxel indices down to -32 (the weld keys are relative to the per-axis minimum).  Same order, same arrays;
    and the extraction repeats itself exactly."""
    vol = holed_volume(backend)
    mesh = vol.extract_triangle_mesh()
    v, c, e = extract_soup(vol)
    assert e[..., :3].min() == -32 and e[..., :3].max() >= 15
    ref = TriangleMesh.from_triangle_soup(v, c, edge_index=e)
    assert mesh.triangles.shape[0] == v.shape[0] > 10000
    np.testing.assert_array_equal(mesh.triangles, ref.triangles)
    np.testing.assert_array_equal(mesh.vertices, ref.vertices)
    np.testing.assert_array_equal(mesh.vertex_colors, ref.vertex_colors)
    np.testing.assert_array_equal(mesh.edge_index, ref.edge_index)
    again = vol.extract_triangle_mesh()
    for name in ("triangles", "vertices", "vertex_colors", "edge_index"):
        np.testing.assert_array_equal(getattr(again, name), getattr(mesh, name))


@pytest.mark.parametrize("x0", [0, -32768])
def test_weld_key_span_on_either_side_of_2_pow_20_voxels(backend, x0):
    """Case 7.  Two blocks `gap` blocks apart along x, one negative voxel each at the same in-block position: the soup spans
    16 * gap voxels (+ 1 inside the key range).  gap 65534 and 65535 weld; 65536 = 2^20 voxels raises, and the handle then serves
    a small volume as before."""
    rng = np.random.default_rng(7)
    tsdf = np.full((2, 4096), 0.5, np.float32)
    tsdf[:, 5 * 256 + 6 * 16 + 7] = -0.25
    w = np.ones((2, 4096), np.float32)
    col = rng.integers(0, 256, (2, 4096, 3))
    vol = make_volume(backend)
    for gap in (65534, 65535, 65536):
        keys = np.array([[x0, 0, 0], [x0 + gap, 0, 0]], np.int32)
        vol.reset()
        upload(backend, vol, keys, tsdf, w, col)
        if gap < 65536:
            assert_full_bar(vol.extract_triangle_mesh(), oracle_mesh(keys, tsdf, w, col))
        else:
            with pytest.raises(RuntimeError, match=r"2\^20 voxels"):
                vol.extract_triangle_mesh()
    vol.reset()
    keys = np.array([[x0, 0, 0], [x0 + 1, 0, 0]], np.int32)
    upload(backend, vol, keys, tsdf, w, col)
    assert vol.num_blocks == 2
    assert_full_bar(vol.extract_triangle_mesh(), oracle_mesh(keys, tsdf, w, col))


def random_triangles(rng, nv, nt):
    t = rng.integers(0, nv, (nt, 3)).astype(np.int32)
    t[t[:, 1] == t[:, 0], 1] = (t[t[:, 1] == t[:, 0], 0] + 1) % nv
    return t


def assert_device_normals_equal_host(be, v, t):
    h = TriangleMesh(v, t).compute_vertex_normals()
    d = TriangleMesh(v, t).compute_vertex_normals(on_device=True, lib=be.lib)
    assert np.array_equal(h.triangle_normals, d.triangle_normals)
    assert np.array_equal(h.vertex_normals, d.vertex_normals)
    return h


@pytest.mark.parametrize("nv", [4095, 4096, 4097, 8191, 8192, 8193])
def test_scan_tile_boundaries(backend, nv):
    """Case 8, through the normals: a soup of exactly 4095 or 4096 items needs 1365 triangles, or a third of a triangle more,
    and a cropped plane only gives even counts -- so the 4096-item tile of gs2m_launch_scan_u32 is pinned where the item count is
    free: the scan of the vertex degrees (the same launch the weld and the clustering make).  A wrong offset at a tile boundary
    moves the bucket of every later vertex."""
    rng = np.random.default_rng(nv)
    t = random_triangles(rng, nv, 2 * nv)
    t[:4] = [[nv - 1, 0, 1], [4094 % nv, nv - 1, 2], [3, 4095 % nv, nv - 2], [nv - 1, nv - 2, 4096 % nv]]
    h = assert_device_normals_equal_host(backend, rng.random((nv, 3)), t)
    assert np.linalg.norm(h.vertex_normals[nv - 1]) > 0.5


# ---- C. clustering against scipy_clusters ------------------------------------------------------------------------------------
def awkward_triangles():
    tri = [[0, 1, 2], [0, 1, 3], [1, 0, 4], [0, 1, 5],                      # four triangles on the edge (0, 1)
           [6, 7, 8], [6, 7, 8], [8, 7, 6],                                 # one triangle twice, and once reversed
           [9, 9, 10], [9, 10, 11],                                         # (a, a, b) shares the edge (a, b) with a proper triangle
           [12, 12, 12],                                                    # (a, a, a)
           [13, 14, 15], [15, 16, 17]]                                      # a bow tie: one shared vertex does not connect
    tri += [[20 + k, 21 + k, 22 + k] for k in range(700)]                   # a strip, fed in shuffled order below
    tri = np.array(tri, np.int32)
    rng = np.random.default_rng(9)
    rot = rng.integers(0, 3, len(tri))                                      # a shared edge sits in any of the three edge slots
    tri = np.stack([tri[np.arange(len(tri)), (rot + j) % 3] for j in range(3)], axis=1)
    return tri[rng.permutation(len(tri))]


def interleaved_triangles():
    """64 mutually disjoint strips of 5 triangles, triangle j of strip c at row 64 * j + c: every wave of 64 consecutive
    triangles carries 64 different labels, and every cluster's count is collected from five waves"""
    j, c = np.divmod(np.arange(320), 64)
    return (np.stack([j + (c + k) % 3 for k in range(3)], axis=1) + 7 * c[:, None]).astype(np.int32)      # corners rotated by c


@pytest.mark.parametrize("n_tri", [1, 63, 64, 65, 255, 256, 257, None])
@pytest.mark.parametrize("which", ["awkward", "interleaved"])
def test_clustering_of_awkward_connectivity(backend, which, n_tri):
    """Case 9.  Non-manifold edge, duplicate and reversed triangles, repeated vertices, a bow tie and a shuffled strip (deep
    parent chains, CAS retries) in one mesh; 64 labels in one wave in the other; both cropped to the sizes around one wave and
    one workgroup.  Labels, counts and the number of clusters are scipy's."""
    tri = (awkward_triangles() if which == "awkward" else interleaved_triangles())[:n_tri]
    m = TriangleMesh(np.random.default_rng(1).random((int(tri.max()) + 1, 3)), tri)
    labels, counts, areas = m.cluster_connected_triangles(lib=backend.lib)
    ref_labels, ref_counts = scipy_clusters(m)
    if n_tri is None:
        assert len(ref_counts) == (7 if which == "awkward" else 64)
    assert len(counts) == len(ref_counts) == len(areas)
    np.testing.assert_array_equal(labels, ref_labels)
    np.testing.assert_array_equal(counts, ref_counts)


def test_clustering_second_grid_stride_round(backend):
    """Case 10.  1 048 576 + 300 triangles: grid_for caps at 4096 workgroups of 256, so every kernel of the clustering takes a
    second grid-stride round, and the wave ballots of k_mesh_uf_labels run with lanes that hold no triangle.  One strip broken
    every 1000 triangles and shuffled; the answer in closed form: 1049 clusters, numbered by first appearance."""
    n = 1048576 + 300
    k = np.random.default_rng(10).permutation(n)
    group = k // 1000
    tri = (k[:, None] + np.arange(3)[None, :] + 5 * group[:, None]).astype(np.int32)
    first = np.full(1049, n, np.int64)
    np.minimum.at(first, group, np.arange(n))
    rank = np.empty(1049, np.int64)
    rank[np.argsort(first)] = np.arange(1049)
    m = TriangleMesh(np.zeros((int(tri.max()) + 1, 3)), tri)
    labels, counts, _ = m.cluster_connected_triangles(lib=backend.lib)
    assert len(counts) == 1049
    np.testing.assert_array_equal(labels, rank[group])
    np.testing.assert_array_equal(counts, np.bincount(rank[group]))
    assert sorted(counts.tolist()) == sorted(np.bincount(np.arange(n) // 1000).tolist())


# ---- D. normals against the numpy statement ------------------------------------------------------------------------------------
def test_normals_across_the_scan_carry(backend):
    """Case 11.  4096 * 1024 + 4096 + 7 vertices are 1026 scan tiles: k_scan_sums (one workgroup, 1024 tile sums per iteration)
    loops twice and carries the running total over.  Triangles sit on both sides of the carry.  gs2m_launch_scan_u32 is the
    scan of the weld and of the clustering as well, so this case stands for their carry loop too: a soup or a triangle list of
    more than four million items would test the same code at forty times the memory."""
    rng = np.random.default_rng(11)
    nv = 4096 * 1024 + 4096 + 7
    v = rng.random((nv, 3))
    t = random_triangles(rng, nv, 5000)
    t[:50] = np.stack([np.roll([nv - 3, nv - 2, nv - 1], i) for i in range(50)])
    t[50:100, 0] = 4096 * 1024
    t[100:110, 1] = 4096 * 1024 - 1
    h = assert_device_normals_equal_host(backend, v, t)
    assert (np.linalg.norm(h.vertex_normals[[nv - 1, 4096 * 1024, 4096 * 1024 - 1]], axis=1) > 0.5).all()


def test_normals_of_high_non_power_of_two_degrees(backend):
    """Case 12.  Fans of 1000, 1023, 1024 and 1025 triangles around one vertex each, the centre in all three corners (the bucket
    merge runs ceil(log2(degree)) passes and its last run is short), next to vertices of degree 1, 2 and 3."""
    tri, nv = [], 0
    for d in (1000, 1023, 1024, 1025):
        ring = nv + 1 + np.arange(d + 1)
        tri += [np.roll([nv, ring[i], ring[i + 1]], i % 3) for i in range(d)]
        nv += d + 2
    tri += [[nv, nv + 1, nv + 2],                                                        # degree 1
            [nv + 3, nv + 4, nv + 5], [nv + 4, nv + 3, nv + 6],                          # an edge of degree 2
            [nv + 7, nv + 8, nv + 9], [nv + 9, nv + 7, nv + 10], [nv + 10, nv + 11, nv + 7]]   # a vertex of degree 3
    nv += 12
    t = np.array(tri, np.int32)
    t = t[np.random.default_rng(12).permutation(len(t))]
    assert (3 * len(t)) % 256 != 0
    deg = np.bincount(t.reshape(-1), minlength=nv)
    assert set([1, 2, 3, 1000, 1023, 1024, 1025]) <= set(deg.tolist())
    assert_device_normals_equal_host(backend, np.random.default_rng(13).random((nv, 3)), t)
