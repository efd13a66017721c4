"""gs2m_densify_stats (gs2mesh_amd/csrc/optim_kernels.h) against the numpy statement (tests/adam_statement.py) bit for bit
on both back-ends, and the statement against the torch ops of the training loop on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import adam_statement as st
from gs2mesh_amd import optim

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs2mesh_amd.h")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def inputs(P, seed):
    rng = np.random.default_rng(seed)
    radii = np.array([0, 3, 0, 12, 1, -1], np.int32)[rng.integers(0, 6, P)]
    grad = (rng.normal(0, 1, (P, 3)) * 10.0 ** rng.uniform(-8, 0, (P, 1))).astype(F32)
    grad[radii <= 0] = np.nan                                   # an unseen row is not read
    grad[:, 2] = np.nan                                         # the third column never is
    max_radii = rng.integers(0, 8, P).astype(F32)               # below, equal to and above the new radius
    accum = rng.uniform(0, 1, (P, 1)).astype(F32)
    denom = rng.integers(0, 50, (P, 1)).astype(F32)
    return radii, grad, max_radii, accum, denom


def run(backend, radii, grad, max_radii, accum, denom):
    d = [backend.dev(a.copy()) for a in (radii, grad, max_radii, accum, denom)]
    optim.densify_stats(*d, lib=backend.lib)
    backend.sync()
    return tuple(backend.host(a) for a in d[2:])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 300])
def test_kernel_equals_the_statement_and_leaves_unseen_rows(backend, P):
    radii, grad, max_radii, accum, denom = inputs(P, P)
    if P == 1:
        radii[0], grad[0, :2] = 5, (3e-4, -4e-4)
    got = run(backend, radii, grad, max_radii, accum, denom)
    ref = st.densify_stats(radii, grad, max_radii, accum, denom)
    unseen = radii <= 0
    for name, g, r, before in zip(("max_radii2D", "grad_accum", "denom"), got, ref, (max_radii, accum, denom)):
        assert g.shape == before.shape and not np.isnan(g).any(), name
        np.testing.assert_array_equal(bits(g), bits(r), err_msg=name)
        np.testing.assert_array_equal(bits(g[unseen]), bits(before[unseen]), err_msg=name)
    assert np.all(got[2][~unseen] == denom[~unseen] + 1)


def test_visible_row_with_zero_gradient_adds_zero_and_one(backend):
    radii = np.array([4, 0, 9], np.int32)
    grad = np.zeros((3, 3), F32)
    grad[:, 2] = 7.0
    accum, denom = np.array([[0.25], [0.5], [0.0]], F32), np.array([[2.0], [3.0], [0.0]], F32)
    mr, acc, den = run(backend, radii, grad, np.zeros(3, F32), accum, denom)
    np.testing.assert_array_equal(bits(acc), bits(accum))
    np.testing.assert_array_equal(den, np.array([[3.0], [3.0], [1.0]], F32))
    np.testing.assert_array_equal(mr, np.array([4.0, 0.0, 9.0], F32))


def test_max_radii_keeps_the_larger_value_in_both_orders(backend):
    grad = np.zeros((2, 3), F32)
    z = lambda: np.zeros((2, 1), F32)
    mr, _, _ = run(backend, np.array([5, 11], np.int32), grad, np.array([9.0, 2.0], F32), z(), z())
    np.testing.assert_array_equal(mr, np.array([9.0, 11.0], F32))
    mr, _, _ = run(backend, np.array([9, 2], np.int32), grad, np.array([5.0, 11.0], F32), z(), z())
    np.testing.assert_array_equal(mr, np.array([9.0, 11.0], F32))


def test_bad_arguments_are_refused(backend):
    from gs2mesh_amd.rasterizer import _ptr
    a = backend.dev(np.zeros(4, F32))
    rc = backend.lib.gs2m_densify_stats(4, None, _ptr(a), _ptr(a), _ptr(a), _ptr(a), C.c_void_p(0))
    assert rc != 0 and "NULL radii" in backend.lib.gs2m_last_error().decode()
    rc = backend.lib.gs2m_densify_stats(-1, None, None, None, None, None, C.c_void_p(0))
    assert rc != 0 and "P = -1" in backend.lib.gs2m_last_error().decode()
    assert backend.lib.gs2m_densify_stats(0, None, None, None, None, None, C.c_void_p(0)) == 0


def test_statement_against_the_torch_ops_of_the_loop():
    """training.train's ``max_radii2D[visible] = torch.max(...)`` and ``GaussianModel.add_densification_stats`` on CPU tensors"""
    P = 100_000
    radii, grad, max_radii, accum, denom = inputs(P, 7)
    grad = np.nan_to_num(grad, nan=0.5)
    mr, acc, den = st.densify_stats(radii, grad, max_radii, accum, denom)
    t_radii, t_grad = torch.from_numpy(radii), torch.from_numpy(grad)
    t_mr, t_acc, t_den = (torch.from_numpy(a.copy()) for a in (max_radii, accum, denom))
    visible = t_radii > 0
    t_mr[visible] = torch.max(t_mr[visible], t_radii[visible].to(t_mr.dtype))
    t_acc[visible] += torch.norm(t_grad[visible, :2], dim=-1, keepdim=True)
    t_den[visible] += 1
    np.testing.assert_array_equal(mr, t_mr.numpy())
    np.testing.assert_array_equal(den, t_den.numpy())
    want = t_acc.numpy()
    ulp = np.nextafter(np.abs(want), F32(np.inf)) - np.abs(want)
    worst = float((np.abs(acc.astype(np.float64) - want) / ulp).max())
    tol = float(re.search(r"#define GS2M_DENSIFY_ACCUM_TOL_ULP\s+([0-9.]+)", open(HEADER).read()).group(1))
    print("grad_accum: largest difference", worst, "ulp of", tol)
    assert worst <= tol
