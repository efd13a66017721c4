"""tools/eval_mesh.py and the vertex PLY reader, on the CPU under the emulator's memory policy: the tool prints what the
module computes, with the reference's keys, from files of the kinds the DTU evaluation reads."""
import json
import os
import sys

import numpy as np
import pytest

from gs2mesh_amd import _lib, evaluation
from gs2mesh_amd.mesh import TriangleMesh, read_point_cloud, read_triangle_mesh, write_triangle_mesh

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


def write_ply(path, pts, fmt, dtype, extra=False):
    name = {"f4": "float", "f8": "double"}[dtype]
    hdr = ["ply", f"format {fmt} 1.0", "comment a ground-truth scan", f"element vertex {len(pts)}"]
    hdr += [f"property {name} {a}" for a in "xyz"]
    if extra:
        hdr += ["property uchar red", "property uchar green", "property uchar blue"]
    hdr += ["element face 0", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode())
        if fmt == "ascii":
            for p in pts:
                row = [repr(float(np.dtype(dtype).type(x))) for x in p] + (["255", "0", "7"] if extra else [])
                fh.write((" ".join(row) + "\n").encode())
        else:
            fields = [(a, "<" + dtype) for a in "xyz"] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if extra else [])
            v = np.zeros(len(pts), dtype=fields)
            v["x"], v["y"], v["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
            fh.write(v.tobytes())


def test_ascii_and_binary_vertex_plys_read_alike(tmp_path):
    pts = np.random.default_rng(0).normal(0, 100, (257, 3))
    for dtype in ("f4", "f8"):
        want = pts.astype(dtype).astype(np.float64)
        for fmt in ("ascii", "binary_little_endian"):
            for extra in (False, True):
                path = str(tmp_path / f"{fmt}_{dtype}_{extra}.ply")
                write_ply(path, pts, fmt, dtype, extra)
                got = read_point_cloud(path)
                assert got.dtype == np.float64 and got.shape == (257, 3)
                np.testing.assert_array_equal(got, want)
    write_ply(str(tmp_path / "none.ply"), pts[:0], "ascii", "f4")
    assert read_point_cloud(str(tmp_path / "none.ply")).shape == (0, 3)
    # this package's own mesh files: the vertices, as read_triangle_mesh gives them (whose behaviour is unchanged)
    m = TriangleMesh(pts[:4], np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    write_triangle_mesh(str(tmp_path / "mesh.ply"), m)
    np.testing.assert_array_equal(read_point_cloud(str(tmp_path / "mesh.ply")), pts[:4])
    back = read_triangle_mesh(str(tmp_path / "mesh.ply"))
    np.testing.assert_array_equal(back.vertices, pts[:4])
    np.testing.assert_array_equal(back.triangles, m.triangles)
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\n"
                                       b"property float z\nend_header\n" + bytes(12))
    with pytest.raises(ValueError, match="binary_little_endian or ascii"):
        read_point_cloud(str(tmp_path / "bad.ply"))


def scene(tmp_path):
    """a bumpy 40 x 40 sheet of 1 mm pitch as the mesh, a shifted, noisy, finer sheet as the scan, DTU-style .mat files"""
    from scipy.io import savemat
    rng = np.random.default_rng(1)
    n = 40
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    verts = np.stack([x, y, 0.5 * np.sin(x / 5) + 0.3 * np.cos(y / 7)], -1).reshape(-1, 3)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    tris = np.concatenate([np.stack([i, i + n, i + n + 1], 1), np.stack([i, i + n + 1, i + 1], 1)]).astype(np.int32)
    gx, gy = np.meshgrid(np.arange(0, n - 1, 0.5), np.arange(0, n - 1, 0.5), indexing="ij")
    gt = np.stack([gx, gy, 0.5 * np.sin(gx / 5) + 0.3 * np.cos(gy / 7) + 0.2], -1).reshape(-1, 3) + rng.normal(0, 0.02, (gx.size, 3))
    gt = np.concatenate([gt, rng.uniform(0, n, (200, 3)) * [1, 1, 0] - [0, 0, 30.0]])      # clutter under the ground plane
    mesh_path, gt_path = str(tmp_path / "mesh.ply"), str(tmp_path / "stl.ply")
    write_triangle_mesh(mesh_path, TriangleMesh(verts, tris))
    write_ply(gt_path, gt, "binary_little_endian", "f4")
    os.makedirs(tmp_path / "dtu" / "ObsMask")
    obs = np.ones((12, 12, 8), np.uint8)
    obs[:3] = 0                                                                            # x < 2.5 + BB: unobserved
    bb = np.array([[-2.0, -2.0, -10.0], [42.0, 42.0, 10.0]])
    savemat(str(tmp_path / "dtu" / "ObsMask" / "ObsMask7_10.mat"), {"ObsMask": obs, "BB": bb, "Res": np.array([[4.0]])})
    savemat(str(tmp_path / "dtu" / "ObsMask" / "Plane7.mat"), {"P": np.array([[0.0], [0.0], [1.0], [5.0]])})
    return mesh_path, gt_path, str(tmp_path / "dtu"), obs, bb


def test_the_tool_prints_what_the_module_computes(tmp_path, emu, capsys):
    import eval_mesh
    mesh_path, gt_path, dtu, obs, bb = scene(tmp_path)
    eval_mesh.main([mesh_path, gt_path, "--dtu-dir", dtu, "--scan", "7", "--density", "0.4", "--max-dist", "5", "--patch", "1",
                    "--thresholds", "0.1,0.5"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    want = evaluation.evaluate_mesh(read_triangle_mesh(mesh_path), read_point_cloud(gt_path), density=0.4, max_dist=5.0,
                                    thresholds=[0.1, 0.5], obs_mask=obs, bb=bb, res=np.array([[4.0]]), plane=np.array([0, 0, 1.0, 5.0]),
                                    patch=1.0)
    assert out == want
    assert {"mean_d2s", "mean_s2d", "overall"} <= set(out)                                 # eval.py:160-166
    f = out["fscore"]
    assert {"pred_gt", "gt_pred", "chamfer"} <= set(f) and set(f["thresholds"]) == {"0.1", "0.5"}      # evaluate.py:62
    assert all(set(v) == {"accuracy", "recall", "F1"} for v in f["thresholds"].values())
    # the sheet lies 0.2 under the scan: both means are near it, the filters removed something, the clutter is gone
    assert 0.15 < out["mean_d2s"] < 0.3 and 0.15 < out["mean_s2d"] < 0.45
    assert 0 < out["n_observed"] < out["n_thinned"] < out["n_sampled"] and out["n_gt"] == 78 * 78
    assert f["thresholds"]["0.1"]["accuracy"] < 0.05 and f["thresholds"]["0.5"]["accuracy"] > 0.95

    # without the DTU files and with a max_dist beyond it, the clutter counts
    eval_mesh.main([mesh_path, gt_path, "--density", "0.4", "--max-dist", "100"])
    plain = json.loads(capsys.readouterr().out.strip())
    assert plain["n_observed"] == plain["n_thinned"] and plain["n_gt"] == 78 * 78 + 200 and "fscore" not in plain
    assert plain["mean_s2d"] > out["mean_s2d"]
