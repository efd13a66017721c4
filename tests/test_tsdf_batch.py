"""TSDF.run(fuse="batch") and its two kernels against the host statements they replace: gs2m_mask_preprocess against
preprocess_object_mask & occlusion, gs2m_mesh_vertex_normals against TriangleMesh.compute_vertex_normals, and the batch run
against the default per-frame loop (same volume bit for bit, same mesh in canonical vertex order).  Emulator build (CPU) and the HIP library (-m gpu)."""
import copy
import ctypes as C
import os
import threading

import numpy as np
import pytest
from PIL import Image as PILImage

from gs2mesh_amd import synthetic
from gs2mesh_amd.mesh import TriangleMesh
from gs2mesh_amd.tsdf_utils import TSDF, mask_preprocess, preprocess_object_mask
from test_pipeline_classes import FakeRenderer, make_args

KS = (1, 2, 3, 9, 10, 11, 64, 65, 130)


def patterns(W, H, rng):
    """random, all 0, all 1 and single pixels at the borders / corners"""
    out = [rng.uniform(size=(H, W)) > 0.55, rng.uniform(size=(H, W)) > 0.95, np.zeros((H, W), bool), np.ones((H, W), bool)]
    for y, x in ((0, 0), (H - 1, W - 1), (0, W - 1), (H // 2, 0), (H - 1, W // 2)):
        m = np.zeros((H, W), bool)
        m[y, x] = True
        out += [m, ~m]
    return out


@pytest.mark.parametrize("W", [1, 63, 64, 65, 160, 1000])
@pytest.mark.parametrize("H", [1, 2, 9, 120])
def test_mask_kernel_equals_host(backend, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    objs = patterns(W, H, rng)
    occ = rng.uniform(size=(H, W)) > 0.1
    # every pattern without and with the occlusion mask, all in one call
    occs = [None] * len(objs) + [occ] * len(objs)
    objs = objs + objs
    for i, k in enumerate(KS):
        k2 = KS[(i + 4) % len(KS)]
        for invert in (False, True):
            for erode in (False, True):
                got = mask_preprocess(objs, occs, invert, erode, k, k2, lib=backend.lib)
                backend.sync()
                for o, c, g in zip(objs, occs, got):
                    ref = preprocess_object_mask(o, invert, erode, k, k2)
                    if c is not None:
                        ref = ref & c
                    g = backend.host(g)
                    assert g.dtype == np.uint8 and g.shape == (H, W)
                    assert np.array_equal(g, ref.astype(np.uint8)), (W, H, k, k2, invert, erode, c is not None)
                got = mask_preprocess(None, [occ], invert, erode, k, k2, lib=backend.lib)     # occlusion only: no morphology
                assert np.array_equal(backend.host(got[0]), occ.astype(np.uint8))


def test_mask_batch_equals_single_calls(backend):
    """37 frames (two launches of at most 32), absent masks mixed in, non-bool inputs (non-zero = true)"""
    W, H, n = 70, 23, 37
    rng = np.random.default_rng(5)
    objs = [(rng.uniform(size=(H, W)) > 0.4).astype(np.float32) * rng.uniform(0.5, 2.0) if i % 5 else None for i in range(n)]
    occs = [rng.integers(0, 3, size=(H, W)).astype(np.uint8) if i % 3 else None for i in range(n)]
    batch = mask_preprocess(objs, occs, True, True, 6, 3, lib=backend.lib)
    backend.sync()
    for i in range(n):
        one = mask_preprocess([objs[i]], [occs[i]], True, True, 6, 3, lib=backend.lib)[0]
        if objs[i] is None and occs[i] is None:
            assert batch[i] is None and one is None
            continue
        ref = np.ones((H, W), bool) if objs[i] is None else preprocess_object_mask(objs[i], True, True, 6, 3)
        if occs[i] is not None:
            ref = ref & (occs[i] != 0)
        assert np.array_equal(backend.host(batch[i]), backend.host(one))
        assert np.array_equal(backend.host(batch[i]), ref.astype(np.uint8)), i


def test_mask_kernel_rejects_k_below_1(backend):
    m = np.ones((8, 8), bool)
    for k1, k2 in ((0, 10), (10, 0), (-3, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            mask_preprocess([m], None, False, True, k1, k2, lib=backend.lib)
    # the C ABI itself refuses it
    from gs2mesh_amd import _lib
    src = _lib.MEMORY.upload(m.view(np.uint8), __import__("torch").uint8, 0)
    out = _lib.MEMORY.zeros((8, 8), np.uint8, 0)
    scratch = _lib.MEMORY.zeros((2 * 8,), np.int64, 0)
    arr = lambda x: (C.c_void_p * 1)(_lib.MEMORY.ptr(x))
    rc = backend.lib.gs2m_mask_preprocess(1, 8, 8, arr(src), None, 0, 1, 0, 10, arr(out), _lib.MEMORY.ptr(scratch),
                                          _lib.MEMORY.current_stream(0))
    assert rc != 0 and b">= 1" in backend.lib.gs2m_last_error()


# ---- TSDF.run(fuse="batch") == TSDF.run() ---------------------------------------------------------------------------------
def write_views(root, n, W, H, f, rng, baseline=0.245):
    poses = synthetic.ring_poses(n, 3.5, 0, 16)
    ren = FakeRenderer(str(root), poses, W, H, f, baseline)
    for i, p in enumerate(poses):
        d = ren.render_folder_name(i)
        os.makedirs(os.path.join(d, "out_DLNR_Middlebury"), exist_ok=True)
        dep = synthetic.sphere_depth(p, W, H, f, f, W / 2.0, H / 2.0, 0.6)
        dep = dep + np.where(dep > 0, rng.normal(0, 2e-3, dep.shape), 0).astype(np.float32)
        msk = (dep > 0) & (rng.uniform(size=(H, W)) > 0.01)
        PILImage.fromarray(np.roll(synthetic.color_pattern(W, H), 5 * i, axis=0)).save(os.path.join(d, "left.png"))
        np.save(os.path.join(d, "out_DLNR_Middlebury", "depth.npy"), dep.astype(np.float32))
        np.save(os.path.join(d, "out_DLNR_Middlebury", "occlusion_mask.npy"), rng.uniform(size=(H, W)) > 0.05)
        np.save(os.path.join(d, "left_mask.npy"), msk)
    # two intrinsic groups, the first one coming back after the second: cameras 6..10 see with another focal length / centre
    for i in range(6, min(11, n)):
        ren.left_cameras[i].update(fx=f * 1.05, fy=f * 1.05, cx=W / 2.0 + 3.0)
    return ren


def canonical(m):
    """the mesh with its vertices in the order of their cut-edge key (Open3D's vertex identity) and its triangles sorted"""
    order = np.argsort(m.edge_index.view([("", np.int32)] * 4).reshape(-1))
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    tri = rank[m.triangles]
    t_order = np.lexsort(tri.T[::-1])
    return dict(vertices=m.vertices[order], vertex_colors=m.vertex_colors[order], edge_index=m.edge_index[order],
                vertex_normals=m.vertex_normals[order], triangles=tri[t_order], triangle_normals=m.triangle_normals[t_order])


def assert_same_volume_and_mesh(a, b):
    """Same blocks with the same voxels, and the same mesh.  Block slots are handed out by atomics in either path, and the
    extraction walks the blocks in slot order, so the vertex / triangle ORDER of the mesh is not a property of the volume
    (two runs of one path differ in it too): the meshes are compared in canonical order.  The vertex normals follow the
    triangle order they are summed in; each mesh's normals are checked bit for bit against the host statement on that mesh."""
    ka, *va = a.volume.download()
    kb, *vb = b.volume.download()
    oa, ob = np.lexsort(ka.T[::-1]), np.lexsort(kb.T[::-1])
    assert len(ka) > 20 and np.array_equal(ka[oa], kb[ob])
    for x, y in zip(va, vb):
        assert np.array_equal(x[oa], y[ob])
    assert a.mesh.triangles.shape[0] > 100
    ca, cb = canonical(a.mesh), canonical(b.mesh)
    for name in ("vertices", "vertex_colors", "edge_index", "triangles", "triangle_normals"):
        assert np.array_equal(ca[name], cb[name]), name
    np.testing.assert_allclose(ca["vertex_normals"], cb["vertex_normals"], rtol=0, atol=1e-12)
    for m in (a.mesh, b.mesh):
        h = copy.deepcopy(m).compute_vertex_normals()
        assert np.array_equal(h.vertex_normals, m.vertex_normals) and np.array_equal(h.triangle_normals, m.triangle_normals)


@pytest.mark.parametrize("dilate,valid,skip,use_mask,invert", [(1, "all-but-4", [2, 9], True, False),
                                                               (2, None, [6], True, True),
                                                               (1, None, None, False, False)])
def test_tsdf_run_batch_equals_frame(backend, tmp_path, dilate, valid, skip, use_mask, invert):
    from argparse import Namespace
    W, H, f, n = 128, 96, 140.0, 13
    ren = write_views(tmp_path, n, W, H, f, np.random.default_rng(3))
    args = make_args(TSDF_use_mask=use_mask, TSDF_invert_mask=invert, TSDF_scale=0.5, TSDF_voxel=8, TSDF_sdf_trunc=0.1,
                     TSDF_dilate=dilate, TSDF_valid=[i for i in range(n) if i != 4] if valid else None, TSDF_skip=skip,
                     TSDF_min_depth_baselines=4, TSDF_max_depth_baselines=15)
    stereo = Namespace(model_name="DLNR_Middlebury")
    ref = TSDF(ren, stereo, args, "out", max_blocks=4096, lib=backend.lib)
    ref.run()
    bat = TSDF(ren, stereo, args, "out", max_blocks=4096, lib=backend.lib, fuse="batch")
    bat.MAX_SWEEP = 3
    sweeps = bat._sweeps(bat._selected())
    assert len(sweeps) >= 3 and max(map(len, sweeps)) <= 3 and len({ren.left_cameras[s[0]]["fx"] for s in sweeps}) == 2
    assert sum(sweeps, []) == ref._selected()
    bat.run()
    assert_same_volume_and_mesh(ref, bat)
    # args.TSDF_fuse selects the same path
    via_args = TSDF(ren, stereo, Namespace(**vars(args), TSDF_fuse="batch"), "out", max_blocks=4096, lib=backend.lib)
    assert via_args.fuse == "batch"


def test_sweeps_are_equal_and_at_most_max_sweep(tmp_path):
    ren = FakeRenderer(str(tmp_path), synthetic.ring_poses(75, 3.5), 32, 24, 30.0, 0.2)
    t = TSDF(ren, None, make_args(), "out", fuse="batch")
    assert [len(s) for s in t._sweeps(list(range(75)))] == [25, 25, 25]
    assert [len(s) for s in t._sweeps(list(range(33)))] == [17, 16]
    t.MAX_SWEEP = 4
    assert [len(s) for s in t._sweeps(list(range(10)))] == [4, 4, 2]
    with pytest.raises(ValueError):
        TSDF(ren, None, make_args(), "out", fuse="sweep")


def test_tsdf_run_batch_frame_source(backend, tmp_path):
    """in-memory frames (host arrays; masks of other dtypes) take the same path"""
    from argparse import Namespace
    W, H, f, n = 96, 72, 100.0, 7
    ren = write_views(tmp_path, n, W, H, f, np.random.default_rng(4))
    args = make_args(TSDF_use_mask=True, TSDF_voxel=8, TSDF_sdf_trunc=0.1, TSDF_min_depth_baselines=4,
                     TSDF_max_depth_baselines=15, TSDF_closing_kernel_size=5, TSDF_erosion_kernel_size=3)
    stereo = Namespace(model_name="DLNR_Middlebury")
    disk = TSDF(ren, stereo, args, "out", lib=backend.lib)
    frames = {i: disk._load_frame(i) for i in range(n)}
    for i in range(n):
        frames[i]["mask"] = frames[i]["mask"].astype(np.float32) * 3.0
        if i == 3:
            del frames[i]["occlusion"]
    ref = TSDF(ren, stereo, args, "out", frame_source=lambda i: frames[i], max_blocks=2048, lib=backend.lib)
    ref.run()
    bat = TSDF(ren, stereo, args, "out", frame_source=lambda i: frames[i], max_blocks=2048, lib=backend.lib, fuse="batch")
    bat.MAX_SWEEP = 2
    bat.run()
    assert_same_volume_and_mesh(ref, bat)


def test_tsdf_run_batch_missing_file_raises(backend, tmp_path):
    from argparse import Namespace
    W, H, f, n = 64, 48, 70.0, 9
    ren = write_views(tmp_path, n, W, H, f, np.random.default_rng(6))
    os.remove(os.path.join(ren.render_folder_name(5), "out_DLNR_Middlebury", "depth.npy"))
    args = make_args(TSDF_use_mask=True, TSDF_voxel=8, TSDF_sdf_trunc=0.1)
    stereo = Namespace(model_name="DLNR_Middlebury")
    with pytest.raises(FileNotFoundError):
        TSDF(ren, stereo, args, "out", max_blocks=2048, lib=backend.lib).run()
    bat = TSDF(ren, stereo, args, "out", max_blocks=2048, lib=backend.lib, fuse="batch")
    bat.MAX_SWEEP = 2
    with pytest.raises(FileNotFoundError):
        bat.run()
    assert not [t for t in threading.enumerate() if t.name.startswith("tsdf-load")]
    # a frame of the wrong shape: the loop's error type
    np.save(os.path.join(ren.render_folder_name(5), "out_DLNR_Middlebury", "depth.npy"), np.zeros((H, W + 1), np.float32))
    with pytest.raises(RuntimeError):
        TSDF(ren, stereo, args, "out", max_blocks=2048, lib=backend.lib).run()
    with pytest.raises(RuntimeError):
        bat.run()
    assert not [t for t in threading.enumerate() if t.name.startswith("tsdf-load")]


# ---- device vertex normals ------------------------------------------------------------------------------------------------
def random_mesh(rng, nv, nt, unref=20):
    v = rng.normal(size=(nv, 3)) * rng.uniform(0.1, 10.0)
    t = rng.integers(0, nv - unref, size=(nt, 3)).astype(np.int32)
    t[: nt // 5, rng.integers(0, 3)] = 11                         # a vertex of degree > nt / 5
    t[nt // 5: nt // 5 + 40, 2] = 5                               # and another one, in every corner
    t[nt // 5 + 40: nt // 5 + 80, 0] = 5
    t[nt // 5 + 80: nt // 5 + 90, 1] = t[nt // 5 + 80: nt // 5 + 90, 0]      # degenerate: two equal corners
    t[nt // 5 + 90: nt // 5 + 95] = 3                              # degenerate: one point
    v[t[nt // 5 + 95, 1]] = v[t[nt // 5 + 95, 0]] + 0.5 * (v[t[nt // 5 + 95, 2]] - v[t[nt // 5 + 95, 0]])   # collinear
    return TriangleMesh(v, t)


@pytest.mark.parametrize("seed,nv,nt", [(0, 60, 200), (1, 500, 3000), (2, 3000, 20000)])
def test_device_normals_equal_host_random_meshes(backend, seed, nv, nt):
    m = random_mesh(np.random.default_rng(seed), nv, nt)
    h = copy.deepcopy(m).compute_vertex_normals()
    d = m.compute_vertex_normals(on_device=True, lib=backend.lib)
    assert d is m
    assert np.array_equal(h.triangle_normals, m.triangle_normals)
    assert np.array_equal(h.vertex_normals, m.vertex_normals)
    assert np.all(m.vertex_normals[nv - 20:] == 0.0)               # unreferenced
    assert np.count_nonzero(np.linalg.norm(m.triangle_normals, axis=1) == 0) >= 15


def test_device_normals_edge_cases(backend):
    m = TriangleMesh(np.zeros((4, 3)), np.zeros((0, 3), np.int32))
    m.compute_vertex_normals(on_device=True, lib=backend.lib)
    assert m.vertex_normals.shape == (4, 3) and not m.vertex_normals.any() and m.triangle_normals.shape == (0, 3)
    e = TriangleMesh().compute_vertex_normals(on_device=True, lib=backend.lib)
    assert e.vertex_normals.shape == (0, 3)
    bad = TriangleMesh(np.zeros((3, 3)), np.array([[0, 1, 3]], np.int32))
    with pytest.raises(RuntimeError, match="outside"):
        bad.compute_vertex_normals(on_device=True, lib=backend.lib)


def test_device_normals_on_extracted_mesh(backend, tmp_path):
    """the extraction's device triangles are used as they are (and the answer is the host one)"""
    from argparse import Namespace
    ren = write_views(tmp_path, 5, 128, 96, 140.0, np.random.default_rng(7))
    t = TSDF(ren, Namespace(model_name="DLNR_Middlebury"), make_args(TSDF_voxel=8, TSDF_sdf_trunc=0.1), "out",
             max_blocks=2048, lib=backend.lib)
    t.run()
    m = t.mesh
    assert getattr(m, "_dev", None) is not None and m._dev[3] is m.triangles and m.triangles.shape[0] > 1000
    h = copy.deepcopy(m).compute_vertex_normals()
    m.vertex_normals = m.triangle_normals = None
    m.compute_vertex_normals(on_device=True, lib=backend.lib)
    assert np.array_equal(h.triangle_normals, m.triangle_normals)
    assert np.array_equal(h.vertex_normals, m.vertex_normals)
