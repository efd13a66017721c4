"""gs2m_stereo_sgm (the built-in matcher of Stereo, gs2mesh_amd/csrc/sgm_kernels.h) against the plain numpy statement of
its arithmetic (tests/sgm_statement.py) on both back-ends: bit-exact summed cost and disparities, a known answer, an
accuracy floor on a stereogram with a known disparity, the reference's RL protocol, argument checking, determinism."""
import ctypes as C

import numpy as np
import pytest

import sgm_statement
from gs2mesh_amd import stereo_utils, synthetic
from gs2mesh_amd.rasterizer import _ptr

_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def matched(backend, W, H, D, p1=10, p2=120):
    """(left, right, truth, disp_lr, disp_rl, S) of the stereogram, matched once per back-end"""
    key = (backend.name, W, H, D, p1, p2)
    if key not in _CACHE:
        left, right, truth = synthetic.random_dot_stereogram(W, H, 0)
        lr, rl, S = stereo_utils.sgm_disparity(backend.dev(left), backend.dev(right), D, p1, p2, tap=True, lib=backend.lib)
        backend.sync()
        _CACHE[key] = (left, right, truth, backend.host(lr), backend.host(rl), backend.host(S).view(np.uint16))
    return _CACHE[key]


@pytest.mark.parametrize("W,H,D,p1,p2", [(176, 120, 64, 10, 120), (200, 104, 128, 10, 120), (176, 120, 64, 3, 190)])
def test_cost_and_disparities_equal_the_statement(backend, W, H, D, p1, p2):
    left, right, _, lr, rl, S = matched(backend, W, H, D, p1, p2)
    ref_lr, ref_rl, ref_S = sgm_statement.sgm(left, right, D, p1, p2)
    assert ref_S.max() <= 4 * (62 + p2) and S.shape == (H, W, D) and lr.dtype == rl.dtype == np.float32
    np.testing.assert_array_equal(S, ref_S.astype(np.uint16))
    np.testing.assert_array_equal(bits(lr), bits(ref_lr))
    np.testing.assert_array_equal(bits(rl), bits(ref_rl))
    assert (lr != np.floor(lr)).mean() > 0.3                  # the sub-pixel step is exercised


def test_known_answer_of_a_shifted_image(backend):
    W, H, D, shift = 176, 64, 64, 9
    left = synthetic.random_dot_stereogram(W, H, 3)[0]
    right = np.ascontiguousarray(np.roll(left, -shift, axis=1))
    lr, _ = stereo_utils.sgm_disparity(backend.dev(left), backend.dev(right), D, want_rl=False, lib=backend.lib)
    lr = backend.host(lr)
    # x >= D: every candidate is inside the image; the last columns of `right` hold the wrapped-around left edge, and the
    # census windows (4 px to each side) of the pixels matching there see it
    sel = lr[:, D:W - 4 - 1]
    assert np.all(np.rint(sel) == shift)
    assert np.all(np.abs(sel - shift) < 0.5)


def test_accuracy_floor_on_the_stereogram(backend):
    W, H, D = 176, 120, 64
    _, _, truth, lr, rl, _ = matched(backend, W, H, D)
    sel = np.zeros((H, W), bool)
    sel[4:H - 4, D:W - 8] = True
    good = (np.abs(lr - truth) <= 1)[sel].mean()
    visible = backend.host(stereo_utils.get_occlusion_mask(backend.dev(lr), backend.dev(rl), 3, lib=backend.lib)).astype(bool)
    print(f"within 1 px: {good:.4f}, visible: {visible[sel].mean():.4f}")
    assert good >= 0.95
    assert visible[sel].mean() >= 0.95


def test_rl_is_the_reference_protocol(backend):
    """stereo_utils.py:112-119: the matcher on (flip(right), flip(left)), flipped back"""
    W, H, D = 176, 120, 64
    left, right, _, _, rl, _ = matched(backend, W, H, D)
    fl, fr = np.ascontiguousarray(left[:, ::-1]), np.ascontiguousarray(right[:, ::-1])
    prot, _ = stereo_utils.sgm_disparity(backend.dev(fr), backend.dev(fl), D, want_rl=False, lib=backend.lib)
    np.testing.assert_array_equal(bits(rl), bits(backend.host(prot)[:, ::-1]))


def test_arguments_and_determinism(backend):
    lib = backend.lib
    W, H, D = 80, 24, 64
    left, right, _ = synthetic.random_dot_stereogram(W, H, 5)
    dl, dr = backend.dev(left), backend.dev(right)
    need = lib.gs2m_stereo_sgm_scratch_bytes(W, H, D)
    assert need > 4 * W * H * D
    assert lib.gs2m_stereo_sgm_scratch_bytes(W, H, 96) == -1 and lib.gs2m_stereo_sgm_scratch_bytes(W, H, 1088) == -1
    scratch = backend.dev(np.zeros(need // 8 + 1, np.int64))
    out = backend.dev(np.zeros((H, W), np.float32))
    st = C.c_void_p(0)

    def call(l=dl, r=dr, d=D, p1=10, p2=120, lr=out, rl=None, sc=scratch, nbytes=need):
        return lib.gs2m_stereo_sgm(_ptr(l), _ptr(r), W, H, d, p1, p2, _ptr(lr), _ptr(rl), _ptr(sc), nbytes, None, st)

    for bad, word in ((dict(d=96), "multiple of 64"), (dict(d=1088), "multiple of 64"), (dict(p2=191), "p2"),
                      (dict(p1=121), "p1"), (dict(p1=0), "p1"), (dict(nbytes=need - 1), "scratch"), (dict(sc=None), "scratch"),
                      (dict(l=None), "NULL image"), (dict(r=None), "NULL image")):
        assert call(**bad) == 1, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    before = backend.host(out).copy()
    assert call(lr=None, rl=None) == 0                        # nothing asked for: nothing done
    backend.sync()
    np.testing.assert_array_equal(backend.host(out), before)
    with pytest.raises(ValueError, match="multiple of 64"):
        stereo_utils.sgm_disparity(dl, dr, 100, lib=lib)
    a = stereo_utils.sgm_disparity(dl, dr, D, lib=lib)
    b = stereo_utils.sgm_disparity(dl, dr, D, lib=lib)
    backend.sync()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(backend.host(x)), bits(backend.host(y)))
    assert backend.host(a[0]).min() >= 0 and backend.host(a[0]).max() <= D - 1
