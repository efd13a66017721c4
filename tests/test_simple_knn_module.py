"""gs2mesh_amd.simple_knn: the drop-in for the reference's ``simple_knn._C.distCUDA2`` (GPU), and the promise that the
training modules import without the library (no GPU)."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_statement


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for P in (1000, 5000):
        pts = np.random.default_rng(P).uniform(-1, 1, (P, 3)).astype(np.float32)
        out[P] = (pts, knn_statement.mean_dist2(pts))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1000, 5000])      # 5000 takes the Morton path
def test_distCUDA2_equals_the_statement(cases, P):
    from backends import use_host_memory
    from gs2mesh_amd.simple_knn import _C
    use_host_memory(False)
    assert (P >= _C.MORTON_MIN_P) == (P == 5000)
    pts, ref = cases[P]
    x = torch.from_numpy(pts).cuda()
    out = _C.distCUDA2(x)
    assert out.dtype == torch.float32 and out.shape == (P,) and out.device == x.device
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref))
    # a non-contiguous view of the same numbers, and a float64 copy of them
    wide = torch.zeros((P, 5), device="cuda")
    wide[:, 1:4] = x
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    np.testing.assert_array_equal(bits(_C.distCUDA2(view).cpu().numpy()), bits(ref))
    np.testing.assert_array_equal(bits(_C.distCUDA2(x.double()).cpu().numpy()), bits(ref))
    assert _C.distCUDA2(x[:0]).shape == (0,)


@pytest.mark.gpu
def test_distCUDA2_with_a_nan_row_equals_the_statement():
    """1500 points take the Morton path, and morton_order sees a NaN bounding box: whatever permutation comes out of it, the
    NaN row gets +inf and no other row changes (the contract of include/gs2mesh_amd.h)"""
    from backends import use_host_memory
    from gs2mesh_amd.simple_knn import _C
    use_host_memory(False)
    pts = np.random.default_rng(1500).uniform(-1, 1, (1500, 3)).astype(np.float32)
    pts[700, 1] = np.nan
    assert len(pts) >= _C.MORTON_MIN_P
    ref = knn_statement.mean_dist2(pts)
    keep = np.arange(1500) != 700
    np.testing.assert_array_equal(bits(ref[keep]), bits(knn_statement.mean_dist2(pts[keep])))
    out = _C.distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()
    assert np.isposinf(out[700]) and np.all(np.isfinite(out[keep]))
    np.testing.assert_array_equal(bits(out), bits(ref))


@pytest.mark.gpu
def test_a_cpu_tensor_is_an_error():
    from backends import use_host_memory
    from gs2mesh_amd.simple_knn import _C
    use_host_memory(False)
    with pytest.raises(RuntimeError, match="HIP device"):
        _C.distCUDA2(torch.zeros(10, 3))
    with pytest.raises(RuntimeError):
        _C.distCUDA2(np.zeros((10, 3), np.float32))


@pytest.mark.gpu
def test_sys_modules_alias_serves_the_reference_import(monkeypatch):
    import gs2mesh_amd.simple_knn
    monkeypatch.setitem(sys.modules, "simple_knn", gs2mesh_amd.simple_knn)
    monkeypatch.setitem(sys.modules, "simple_knn._C", gs2mesh_amd.simple_knn._C)
    from simple_knn._C import distCUDA2         # scene/gaussian_model.py:20
    assert distCUDA2 is gs2mesh_amd.simple_knn._C.distCUDA2
    x = torch.rand(64, 3, device="cuda")
    np.testing.assert_array_equal(bits(distCUDA2(x).cpu().numpy()), bits(knn_statement.mean_dist2(x.cpu().numpy())))


def test_training_modules_import_without_the_library():
    code = ("import gs2mesh_amd._lib as L\n"
            "L.LIB_PATH = '/nonexistent/libgs2mesh_amd.so'\n"
            "import sys, gs2mesh_amd.gaussian_model as gm, gs2mesh_amd.training as tr\n"
            "assert L._LIB is None\n"
            "m = gm.GaussianModel(3, device='cpu')\n"
            "assert hasattr(m, 'create_from_pcd') and hasattr(tr, 'train') and tr.OptimizationParams().iterations == 30000\n"
            "try:\n"
            "    L.get()\n"
            "    raise SystemExit('the library loaded')\n"
            "except RuntimeError:\n"
            "    pass\n"
            "print('ok')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
