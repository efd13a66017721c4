"""tools/eval_mesh.py --icp-gt-mesh and --tnt-dir, on the CPU under the emulator's memory policy: the tool aligns as
``evaluation.mobilebrick_align`` / ``evaluation.tnt_evaluate`` do, and without the new options its output has no new key."""
import json
import os
import sys

import numpy as np
import pytest

from gs2mesh_amd import _lib
from gs2mesh_amd.mesh import TriangleMesh, write_triangle_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture
def emu(monkeypatch):
    """the emulator build and its memory policy behind _lib.get(), which is what the tool calls"""
    from backends import EmuBackend
    monkeypatch.setattr(_lib, "MEMORY", _lib.MEMORY)          # put back afterwards: EmuBackend() installs the host policy
    b = EmuBackend()
    monkeypatch.setattr(_lib, "_LIB", b.lib)
    return b


def sheet(n, h):
    g = np.arange(-n, n + 1) * h
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    verts = np.stack([x, y, 0.3 * np.sin(2 * x + 0.5) * np.cos(3 * y) + 0.1 * x * y], 1)
    m = 2 * n + 1
    i = (np.arange(m - 1)[:, None] * m + np.arange(m - 1)[None, :]).reshape(-1)
    tris = np.concatenate([np.stack([i, i + m, i + m + 1], 1), np.stack([i, i + m + 1, i + 1], 1)]).astype(np.int32)
    return verts, tris


def similarity(scale):
    a = np.array([0.3, -1.0, 2.0]) / np.linalg.norm([0.3, -1.0, 2.0])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    S = np.eye(4)
    S[:3, :3] = scale * (np.eye(3) + np.sin(0.004) * K + (1 - np.cos(0.004)) * (K @ K))
    S[:3, 3] = [0.003, -0.002, 0.001]
    return S


def test_icp_gt_mesh_aligns_before_scoring(tmp_path, emu, capsys):
    import eval_mesh
    verts, tris = sheet(20, 0.05)                                     # pitch 0.05 > the 0.02 threshold > the displacement
    S = similarity(1.0)
    moved = verts @ S[:3, :3].T + S[:3, 3]
    mesh_path, gt_path = str(tmp_path / "mesh.ply"), str(tmp_path / "gt_mesh.ply")
    write_triangle_mesh(mesh_path, TriangleMesh(moved, tris))
    write_triangle_mesh(gt_path, TriangleMesh(verts, tris))
    common = [mesh_path, gt_path, "--density", "0.02", "--max-dist", "1"]
    plain = eval_mesh.main(common)
    aligned = eval_mesh.main(common + ["--icp-gt-mesh", gt_path])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and json.loads(lines[1]) == aligned
    assert "icp" not in plain and set(aligned) == set(plain) | {"icp"}
    assert aligned["icp"]["applied"] is True and aligned["icp"]["fitness"] == 1.0 and 1 <= aligned["icp"]["n_iterations"] <= 10
    assert aligned["mean_s2d"] < 1e-6 < plain["mean_s2d"]             # the GT vertices lie on the aligned mesh's vertices (f32 search)


def test_tnt_dir_runs_the_tnt_flow(tmp_path, emu, capsys):
    import eval_mesh
    h = 0.05
    gt, tris = sheet(20, h)
    S = similarity(1.002)
    Si = np.linalg.inv(S)
    mesh_path, gt_path = str(tmp_path / "mesh.ply"), str(tmp_path / "Barn.ply")
    write_triangle_mesh(mesh_path, TriangleMesh(gt @ Si[:3, :3].T + Si[:3, 3], tris))
    write_triangle_mesh(gt_path, TriangleMesh(gt, tris))
    os.makedirs(tmp_path / "Barn")
    c = 17.5 * h
    (tmp_path / "Barn" / "Barn.json").write_text(json.dumps({
        "axis_max": 1.0, "axis_min": -1.0, "bounding_polygon": [[-c, -c, 0], [c, -c, 0], [c, c, 0], [-c, c, 0]],
        "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "version_major": 1, "version_minor": 0}))
    np.savetxt(str(tmp_path / "init.txt"), np.eye(4))
    out = eval_mesh.main([mesh_path, gt_path, "--tnt-dir", str(tmp_path / "Barn"), "--tnt-init", str(tmp_path / "init.txt"), "--tau", "0.03"])
    printed = json.loads(capsys.readouterr().out.strip())
    assert printed == out and set(out) == {"precision", "recall", "fscore", "transformation", "n_source", "n_target"}
    assert out["precision"] == out["recall"] == out["fscore"] == 1.0 and out["n_source"] == out["n_target"] == 35 * 35
    assert np.abs(np.array(out["transformation"]) - S).max() < 1e-9
    with pytest.raises(SystemExit):
        eval_mesh.main([mesh_path, gt_path, "--tnt-dir", str(tmp_path / "Barn")])
