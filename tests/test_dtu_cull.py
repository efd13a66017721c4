"""The Python side of the DTU cull (gs2mesh_amd.evaluation: dtu_projections, dtu_cull, visibility_cull, evaluate_mesh's
``cull``; TriangleMesh.remove_vertices_by_mask; tools/eval_mesh.py --cull-dir).  The parts that need no kernel run as they are;
the others run on the emulator build here and on the GPU under -m gpu."""
import json
import os
import sys

import numpy as np
import pytest

import cull_scene
import cull_statement
import dilate_statement
from gs2mesh_amd import _lib, evaluation
from gs2mesh_amd.mesh import TriangleMesh, read_triangle_mesh, write_triangle_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MASK, NORM, RADIUS = (130, 70), (1600, 1200), 2


@pytest.fixture
def env(backend, monkeypatch):
    """the back-end's library and memory policy behind _lib.get(), which is what dtu_cull and the tool call"""
    monkeypatch.setattr(_lib, "MEMORY", _lib.MEMORY)          # put back afterwards what the back-end installed
    monkeypatch.setattr(_lib, "_LIB", backend.lib)
    return backend


# ---- no kernel ------------------------------------------------------------------------------------------------------------------

def test_dtu_projections_rebuild_the_normalised_camera():
    cams, parts = cull_scene.cameras(4, NORM)
    proj, scale0 = evaluation.dtu_projections(cams)
    assert proj.dtype == np.float32 and proj.shape == (4, 3, 4) and scale0.dtype == np.float32
    np.testing.assert_array_equal(scale0, cams["scale_mat_0"].astype(np.float32))
    for i, (K, R, C) in enumerate(parts):
        want = (K / K[2, 2]) @ np.concatenate([R, (-R @ C)[:, None]], axis=1) @ cams[f"scale_mat_{i}"]
        # the reference's w2c is in the frame the scale matrix maps from; its third row there has the length of the scale
        want = want / np.linalg.norm(want[2, :3])
        assert np.abs(proj[i] - want).max() <= 1e-5 * np.abs(want).max()
        assert abs(np.linalg.norm(proj[i][2, :3].astype(np.float64)) - 1) < 1e-6
    # the .npz of the dataset reads the same
    import io
    buf = io.BytesIO()
    np.savez(buf, **cams)
    buf.seek(0)
    np.testing.assert_array_equal(evaluation.dtu_projections(np.load(buf))[0], proj)
    assert evaluation.dtu_projections({})[0].shape == (0, 3, 4)


def test_dtu_projections_refuse_a_mirrored_camera():
    cams, _ = cull_scene.cameras(2, NORM)
    cams["world_mat_1"] = cams["world_mat_1"].copy()
    cams["world_mat_1"][:3] *= -1                              # the same projection, det(P[:, :3]) < 0
    with pytest.raises(ValueError, match="camera 1"):
        evaluation.dtu_projections(cams)
    cams["world_mat_1"][:3, :3] = 0
    with pytest.raises(ValueError, match="det"):
        evaluation.dtu_projections(cams)


def six_vertex_mesh():
    v = np.arange(18, dtype=np.float64).reshape(6, 3)
    t = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 5], [5, 0, 2]], np.int32)
    m = TriangleMesh(v, t, vertex_colors=v / 20)
    m.vertex_normals = -v
    m.triangle_normals = np.arange(12, dtype=np.float64).reshape(4, 3)
    return m


def test_remove_vertices_by_mask_against_a_hand_written_expectation():
    m = six_vertex_mesh()
    ret = m.remove_vertices_by_mask([False, False, False, True, False, False])           # vertex 3 goes
    assert ret is m
    # triangles 1 and 2 used vertex 3; vertex 4 is used by nothing any more and stays; 4 -> 3, 5 -> 4
    np.testing.assert_array_equal(m.vertices, np.arange(18, dtype=np.float64).reshape(6, 3)[[0, 1, 2, 4, 5]])
    np.testing.assert_array_equal(m.triangles, [[0, 1, 2], [4, 0, 2]])
    assert m.triangles.dtype == np.int32
    np.testing.assert_array_equal(m.vertex_colors, m.vertices / 20)
    np.testing.assert_array_equal(m.vertex_normals, -m.vertices)
    np.testing.assert_array_equal(m.triangle_normals, [[0, 1, 2], [9, 10, 11]])

    none = six_vertex_mesh().remove_vertices_by_mask(np.ones(6, bool))
    assert none.vertices.shape == (0, 3) and none.triangles.shape == (0, 3) and none.vertex_colors.shape == (0, 3)
    same = six_vertex_mesh().remove_vertices_by_mask(np.zeros(6, bool))
    np.testing.assert_array_equal(same.vertices, six_vertex_mesh().vertices)
    np.testing.assert_array_equal(same.triangles, six_vertex_mesh().triangles)
    with pytest.raises(ValueError, match="mask of 5"):
        six_vertex_mesh().remove_vertices_by_mask(np.zeros(5, bool))


# ---- on a back-end ----------------------------------------------------------------------------------------------------------------

def test_visibility_cull_against_the_reference_lines(env):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    volume = (rng.random((5, 4, 3)) < 0.6).astype(np.float64) * rng.integers(1, 5, (5, 4, 3))
    res = np.array([5, 4, 3])
    min_pts, voxel = np.array([-0.2, 0.1, 0.3]), 0.05
    centres = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    halves = centres[::3] + rng.choice([-0.5, 0.5], (len(centres[::3]), 3))               # ties, and half a voxel outside
    outside = np.array([[-0.51, 1, 1], [4.51, 1, 1], [2, -0.6, 1], [2, 3.6, 1], [2, 1, -0.7], [2, 1, 2.7], [-3, -3, -3], [9, 9, 9]])
    near = centres + rng.uniform(-0.49, 0.49, centres.shape)
    verts = np.concatenate([centres, halves, outside, near]) * voxel + min_pts
    tris = np.stack([np.arange(len(verts) - 2), np.arange(1, len(verts) - 1), np.arange(2, len(verts))], 1).astype(np.int32)
    # evaluation/MobileBrick/eval_code/evaluate.py:35-42 restated: numpy f64 up to the grid, torch f32 for the look-up
    g = (verts - min_pts) / voxel
    g = g / (res - 1) * 2 - 1
    grid = torch.from_numpy(np.ascontiguousarray(g[:, ::-1])).float()
    seen = F.grid_sample(torch.from_numpy(volume).float()[None, None], grid[None, None, None], mode="nearest", padding_mode="zeros",
                         align_corners=True)[0, 0, 0, 0].numpy() > 0
    assert seen[:60].tolist() == (volume.reshape(-1) > 0).tolist()                         # voxel centres read their voxel
    assert not seen[60 + len(halves):60 + len(halves) + 8].any()                           # outside reads 0
    want = TriangleMesh(verts, tris).remove_vertices_by_mask(~seen)

    mesh = TriangleMesh(verts, tris)
    got = evaluation.visibility_cull(mesh, volume, min_pts, res, voxel)
    assert got is not mesh and mesh.vertices.shape[0] == len(verts)                        # a new mesh
    np.testing.assert_array_equal(got.vertices, want.vertices)
    np.testing.assert_array_equal(got.triangles, want.triangles)
    assert 0 < got.vertices.shape[0] < len(verts)
    np.testing.assert_array_equal(got.vertex_normals, want.compute_vertex_normals().vertex_normals)


def scan(tmp_path):
    """a sphere in the normalised frame, three cameras for 1600 x 1200 images, 130 x 70 disc masks as PNG files (one grey, two
    RGB with the mask in the blue channel only, which is channel 0 of cv2.imread), DTU's directory layout"""
    from PIL import Image
    cams, _ = cull_scene.cameras(3, NORM)
    masks = cull_scene.disc_masks(3, MASK)
    d = tmp_path / "scan7"
    os.makedirs(d / "mask")
    np.savez(str(d / "cameras.npz"), **cams)
    rng = np.random.default_rng(5)
    paths = []
    for i, m in enumerate(masks):
        paths.append(str(d / "mask" / f"{i:03d}.png"))
        if i == 0:
            Image.fromarray(m, "L").save(paths[-1])
        else:
            rgb = np.stack([rng.integers(0, 256, m.shape).astype(np.uint8), 255 - m, m], -1)     # red noise, green inverted
            Image.fromarray(rgb, "RGB").save(paths[-1])
    verts, tris = cull_scene.sphere_mesh()
    return str(d), cams, masks, paths, verts, tris


def composition_of_the_statements(cams, masks, verts, tris):
    proj, scale0 = evaluation.dtu_projections(cams)
    dilated = np.stack([dilate_statement.dilate(m, RADIUS) for m in masks]).astype(np.uint8)
    keep = cull_statement.keep_a(verts.astype(np.float32), proj, dilated, NORM)
    new_index = np.cumsum(keep) - 1
    faces = tris[keep[tris].all(axis=1)]
    world = verts[keep] * np.float64(scale0[0, 0]) + scale0[:3, 3].astype(np.float64)[None]
    return keep, world, new_index[faces].astype(np.int32)


def test_dtu_cull_end_to_end_and_the_tool(env, tmp_path, capsys):
    d, cams, masks, paths, verts, tris = scan(tmp_path)
    keep, world, faces = composition_of_the_statements(cams, masks, verts, tris)
    V = len(verts)
    assert 0 < keep.sum() < V

    mesh = TriangleMesh(verts, tris)
    for given in (paths, list(masks), [np.stack([m, 0 * m, 0 * m], -1) for m in masks]):       # files, [H,W], [H,W,C]: channel 0
        got = evaluation.dtu_cull(mesh, cams, given, radius=RADIUS)
        assert got is not mesh and mesh.vertices.shape[0] == V
        np.testing.assert_array_equal(got.vertices, world)
        np.testing.assert_array_equal(got.triangles, faces)
    assert 0 < got.vertices.shape[0] < V
    np.testing.assert_array_equal(evaluation.dtu_cull((verts, tris), os.path.join(d, "cameras.npz"), paths, radius=RADIUS).vertices, world)
    with pytest.raises(ValueError, match="2 masks for 3 cameras"):
        evaluation.dtu_cull(mesh, cams, paths[:2])

    # evaluate_mesh: the cull first, and only then the keys change
    gt = verts * 1.3 + cull_scene.CENTRE
    plain = evaluation.evaluate_mesh(mesh, verts, density=0.05)
    assert set(plain) == {"mean_d2s", "mean_s2d", "overall", "n_sampled", "n_thinned", "n_observed", "n_gt"}
    culled = evaluation.evaluate_mesh(mesh, gt, density=0.05, cull=dict(cameras=cams, masks=paths, radius=RADIUS))
    assert set(culled) == set(plain) | {"n_vertices_culled"} and culled["n_vertices_culled"] == V - int(keep.sum())
    assert culled == dict(evaluation.evaluate_mesh(TriangleMesh(world, faces), gt, density=0.05), n_vertices_culled=V - int(keep.sum()))

    # the tool: scanN/cameras.npz and the sorted scanN/mask/*.png
    import eval_mesh
    mesh_path, gt_path, out_path = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply"), str(tmp_path / "culled.ply")
    write_triangle_mesh(mesh_path, mesh)
    write_triangle_mesh(gt_path, TriangleMesh(gt))                   # a vertex PLY
    capsys.readouterr()
    eval_mesh.main([mesh_path, gt_path, "--density", "0.05", "--cull-dir", d, "--cull-radius", str(RADIUS), "--save-culled", out_path])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out == culled
    saved = read_triangle_mesh(out_path)
    np.testing.assert_array_equal(saved.vertices, world)
    np.testing.assert_array_equal(saved.triangles, faces)
    # the default is the reference's disk(24), which on these small masks covers the whole sphere
    eval_mesh.main([mesh_path, gt_path, "--density", "0.05", "--cull-dir", d])
    assert json.loads(capsys.readouterr().out.strip())["n_vertices_culled"] == 0
    eval_mesh.main([mesh_path, gt_path, "--density", "0.05"])
    assert "n_vertices_culled" not in json.loads(capsys.readouterr().out.strip())
