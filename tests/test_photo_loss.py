"""gs2m_photo_loss_forward / _backward (gs2mesh_amd/csrc/loss_kernels.h) against the plain numpy statement of their
arithmetic (tests/loss_statement.py) on both back-ends.  The SSIM map, the three derivative planes and the gradient are
compared bit for bit; the three scalars against the fp64 sum of the statement's terms, within the bound that the length of
the kernels' addition chain gives."""
import ctypes as C
import math

import numpy as np
import pytest

import loss_statement
from gs2mesh_amd import training
from gs2mesh_amd.rasterizer import _ptr

LAMBDA = 0.2
TW, TH = loss_statement.TILE_W, loss_statement.TILE_H
_REF = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(shape, seed, lo=0.0, hi=1.0):
    r = np.random.default_rng(seed)
    return r.uniform(lo, hi, shape).astype(np.float32), r.uniform(lo, hi, shape).astype(np.float32)


def statement(key, make, lam=LAMBDA, grad_loss=1.0):
    """(x, y, forward planes, gradient), computed once per input and shared between the back-ends; never modified"""
    if key not in _REF:
        x, y = make()
        fw = loss_statement.forward(x.reshape(-1, *x.shape[-2:]), y.reshape(-1, *y.shape[-2:]))
        grad = loss_statement.backward(x.reshape(-1, *x.shape[-2:]), y.reshape(-1, *y.shape[-2:]), fw, lam, grad_loss)
        for a in list(fw.values()) + [grad]:                 # the inputs only ever go to backend.dev
            a.setflags(write=False)
        _REF[key] = (x, y, fw, grad)
    return _REF[key]


def run(backend, x, y, lam=LAMBDA, grad_loss=1.0, want_partials=True):
    dx, dy = backend.dev(x), backend.dev(y)
    out, partials, tap = training.photo_loss_forward(dx, dy, lam, want_partials=want_partials, want_map=True, lib=backend.lib)
    grad = None
    if want_partials:
        grad = training.photo_loss_backward(dx, dy, partials, lam, backend.dev(np.array([grad_loss], np.float32)), lib=backend.lib)
    backend.sync()
    return backend.host(out), backend.host(partials), backend.host(tap), backend.host(grad)


def assert_same(got, ref, what, nan_ok=False):
    """bit for bit; with ``nan_ok`` the NaN masks are equal and every other value is equal in bits"""
    got, ref = np.asarray(got).reshape(ref.shape), np.asarray(ref)
    gn, rn = np.isnan(got), np.isnan(ref)
    if not nan_ok:
        assert not rn.any() and not gn.any(), what
    np.testing.assert_array_equal(gn, rn, err_msg=what + ": NaN mask")
    np.testing.assert_array_equal(bits(got)[~rn], bits(ref)[~rn], err_msg=what)


def check_scalars(out, fw, lam, planes, H, W):
    value, absum = loss_statement.scalars64(fw, lam)
    chain = loss_statement.chain(planes, H, W)
    for k, name in enumerate(("loss", "l1_mean", "ssim_mean")):
        bound = chain * 2.0 ** -24 * absum[k]
        assert abs(float(out[k]) - value[k]) <= bound, (name, float(out[k]), value[k], bound)


def check(backend, key, make, lam=LAMBDA, grad_loss=1.0, nan_ok=False):
    x, y, fw, grad = statement(key, make, lam, grad_loss)
    out, partials, tap, got_grad = run(backend, x, y, lam, grad_loss)
    assert tap.shape == x.shape and partials.shape == (3,) + x.shape and got_grad.shape == x.shape and out.shape == (3,)
    assert_same(tap, fw["map"], "map", nan_ok)
    for k in range(3):
        assert_same(partials[k], fw[f"p{k}"], f"partials[{k}]", nan_ok)
    assert_same(got_grad, grad, "grad_image", nan_ok)
    if not nan_ok:
        planes = int(np.prod(x.shape[:-2]))
        check_scalars(out, fw, lam, planes, x.shape[-2], x.shape[-1])
    return x, y, fw, grad, out, tap, got_grad


EDGE = [(1, 1), (1, 12), (12, 1), (5, 6), (11, 11), (2, 10), (6, 5), (10, 2)]


@pytest.mark.parametrize("H,W", EDGE)
def test_images_around_the_window_radius_and_width(backend, H, W):
    check(backend, ("edge", H, W), lambda: noise((1, H, W), 100 * H + W))


@pytest.mark.parametrize("H", [TH - 1, TH, TH + 1, 2 * TH + 3])
@pytest.mark.parametrize("W", [TW - 1, TW, TW + 1, 2 * TW + 3])
def test_tile_boundaries_in_both_directions(backend, H, W):
    check(backend, ("tile", H, W), lambda: noise((1, H, W), 100 * H + W))


def test_odd_non_square_image(backend):
    check(backend, "odd", lambda: noise((3, 37, 53), 7))


@pytest.mark.parametrize("shape", [(1, 19, 35), (3, 19, 35), (4, 19, 35), (2, 3, 19, 35)])
def test_planes_and_the_batched_form(backend, shape):
    x, y, fw, grad, out, tap, got = check(backend, ("planes", shape), lambda: noise(shape, len(shape) * 10 + shape[0]))
    if len(shape) == 4:
        # planes are independent: the batched call is the per-image calls side by side
        for b in range(shape[0]):
            _, _, tap_b, _ = run(backend, x[b], y[b])
            np.testing.assert_array_equal(bits(tap_b), bits(tap[b]))


def test_values_outside_zero_one(backend):
    check(backend, "wide", lambda: noise((3, 21, 40), 11, -0.5, 1.5), lam=0.35, grad_loss=-2.5)


def test_constant_images_have_zero_variance(backend):
    def make():
        return np.full((2, 18, 34), 0.25, np.float32), np.full((2, 18, 34), 0.75, np.float32)
    x, y, fw, *_ = check(backend, "constant", make)
    c = (slice(None), slice(6, 12), slice(6, 28))             # the full window lies inside: sigma is exactly 0
    assert np.all(fw["map"][c] == fw["map"][0, 8, 8]) and 0 < fw["map"][0, 8, 8] < 1


def test_identical_images(backend):
    def make():
        x, _ = noise((3, 20, 37), 5)
        return x, x.copy()
    x, y, fw, grad, out, tap, got = check(backend, "identical", make)
    assert np.all(tap == np.float32(1.0)) and out[1] == 0.0
    assert abs(float(out[2]) - 1.0) <= loss_statement.chain(3, 20, 37) * 2.0 ** -24


def test_sign_zero_next_to_plus_and_minus_one(backend):
    def make():
        x, y = noise((3, 20, 37), 6)
        x = x.copy()
        x[:, :, ::2] = y[:, :, ::2]
        return x, y
    x, y, fw, grad, *_ = check(backend, "half", make, lam=0.0, grad_loss=1.0)
    ka = loss_statement.factors(0.0, x.size)[0]
    # lambda = 0: only the L1 term is left, up to the signed zeros of the SSIM terms
    assert set(np.unique(grad).tolist()) == {float(-ka), 0.0, float(ka)} and not grad[:, :, ::2].any()
    check(backend, "half_dssim", make)


def test_one_nan_pixel_spreads_as_far_as_the_statement_says(backend):
    def make():
        x, y = noise((3, 24, 40), 8)
        x = x.copy()
        x[1, 12, 20] = np.nan
        return x, y
    x, y, fw, grad, out, tap, got = check(backend, "nan", make, nan_ok=True)
    hit_map, hit_grad = np.isnan(tap), np.isnan(got)
    assert not hit_map[0].any() and not hit_map[2].any() and not hit_grad[0].any() and not hit_grad[2].any()
    rows, cols = np.nonzero(hit_map[1])
    assert len(rows) == 121 and np.abs(rows - 12).max() == 5 and np.abs(cols - 20).max() == 5
    rows, cols = np.nonzero(hit_grad[1])
    assert len(rows) == 441 and np.abs(rows - 12).max() == 10 and np.abs(cols - 20).max() == 10
    assert math.isnan(float(out[0])) and math.isnan(float(out[2])) and math.isnan(float(out[1]))


def test_the_scalars_are_the_same_bits_on_every_call(backend):
    x, y, fw, _ = statement("odd", lambda: noise((3, 37, 53), 7))
    a = run(backend, x, y)[0]
    b = run(backend, x, y)[0]
    c = run(backend, x, y, want_partials=False)[0]              # partials = NULL gives the same out
    np.testing.assert_array_equal(bits(a), bits(b))
    np.testing.assert_array_equal(bits(a), bits(c))
    check_scalars(a, fw, LAMBDA, 3, 37, 53)


def test_the_wrapper_on_the_backend_arrays(backend):
    """fused_loss / fused_ssim on what the back-end calls device memory: out[0] and out[2] of the same kernels"""
    x, y, fw, _ = statement("odd", lambda: noise((3, 37, 53), 7))
    out = run(backend, x, y)[0]
    dx, dy = backend.dev(x), backend.dev(y)
    loss = training.fused_loss(dx, dy, LAMBDA, lib=backend.lib)
    ssim = training.fused_ssim(dx, dy, lib=backend.lib)
    backend.sync()
    assert np.shape(loss) == () and bits(backend.host(loss)) == bits(out[0])
    assert bits(backend.host(ssim)) == bits(out[2])


def test_arguments_and_no_state_between_calls(backend):
    lib = backend.lib
    P, H, W = 3, 37, 53
    x, y, fw, grad = statement("odd", lambda: noise((3, 37, 53), 7))
    need = lib.gs2m_photo_loss_scratch_bytes(P, H, W)
    assert need >= 8 * P * 3 * 2 and need % 16 == 0
    assert lib.gs2m_photo_loss_scratch_bytes(0, H, W) == 0 and lib.gs2m_photo_loss_scratch_bytes(P, 0, W) == 0
    big = 3 * ((30000 + TH - 1) // TH) * ((30000 + TW - 1) // TW)                # 2.7e9 pixels: sizes are 64-bit
    assert lib.gs2m_photo_loss_scratch_bytes(3, 30000, 30000) == 16 * ((big + 1) // 2)
    for huge in ((3, 2 ** 31 - 1, 2 ** 31 - 1), (1, 2 ** 31 - 1, 1), (1, 1, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 1),
                 (2 ** 31 - 1, 16, 32)):
        assert lib.gs2m_photo_loss_scratch_bytes(*huge) == -1, huge             # refused, not wrapped around
    scratch = backend.dev(np.zeros(need // 8 + 2, np.int64))
    dx, dy = backend.dev(x), backend.dev(y)
    out = backend.dev(np.full(3, 7.0, np.float32))
    partials = backend.dev(np.full((3, P, H, W), 7.0, np.float32))
    tap = backend.dev(np.full((P, H, W), 7.0, np.float32))
    gimg = backend.dev(np.full((P, H, W), 7.0, np.float32))
    one = backend.dev(np.ones(1, np.float32))
    st = C.c_void_p(0)

    def fwd(p=P, h=H, w=W, a=dx, b=dy, sc=_ptr(scratch), nbytes=need, o=out, pa=partials, tp=tap):
        return lib.gs2m_photo_loss_forward(p, h, w, _ptr(a), _ptr(b), LAMBDA, sc, nbytes, _ptr(o), _ptr(pa), _ptr(tp), st)

    def bwd(p=P, h=H, w=W, a=dx, b=dy, pa=partials, gl=one, g=gimg):
        return lib.gs2m_photo_loss_backward(p, h, w, _ptr(a), _ptr(b), _ptr(pa), LAMBDA, _ptr(gl), _ptr(g), st)

    misaligned = C.c_void_p(_ptr(scratch).value + 8)
    for bad, word in ((dict(a=None), "image"), (dict(b=None), "target"), (dict(o=None), "out"), (dict(sc=None), "scratch"),
                      (dict(nbytes=need - 1), "scratch"), (dict(sc=misaligned), "aligned"), (dict(p=-1), "planes"),
                      (dict(h=-1), "height"), (dict(w=-1), "width")):
        assert fwd(**bad) == 1, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    for bad, word in ((dict(a=None), "image"), (dict(b=None), "target"), (dict(pa=None), "partials"),
                      (dict(gl=None), "grad_loss"), (dict(g=None), "grad_image"), (dict(p=-1), "planes"),
                      (dict(h=-1), "height"), (dict(w=-1), "width")):
        assert bwd(**bad) == 1, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert fwd(p=1, h=2 ** 31 - 1, w=1) == 1 and "tiles" in lib.gs2m_last_error().decode()
    assert bwd(p=1, h=2 ** 31 - 1, w=1) == 1 and "tiles" in lib.gs2m_last_error().decode()
    # size 0 does nothing, whatever else is passed
    for zero in (dict(p=0), dict(h=0), dict(w=0)):
        assert fwd(**zero) == 0 and bwd(**zero) == 0
        assert fwd(a=None, b=None, sc=None, nbytes=0, o=None, pa=None, tp=None, **zero) == 0
    backend.sync()
    for buf in (out, partials, tap, gimg):
        assert np.all(backend.host(buf) == 7.0)                                 # every refused or empty call: outputs untouched

    def whole(shape_key, make, p, h, w, o):
        xs, ys, fws, grads = statement(shape_key, make)
        a, b = backend.dev(xs), backend.dev(ys)
        pa, tp, g = (backend.dev(np.zeros(s, np.float32)) for s in ((3, p, h, w), (p, h, w), (p, h, w)))
        assert fwd(p, h, w, a, b, o=o, pa=pa, tp=tp) == 0 and bwd(p, h, w, a, b, pa=pa, g=g) == 0
        backend.sync()
        assert_same(backend.host(tp), fws["map"], "map")
        assert_same(backend.host(g), grads, "grad_image")
        return bits(backend.host(o)).copy()

    # one scratch buffer, another shape, then the first again: every call its own result
    first = whole("odd", None, P, H, W, out)
    out2 = backend.dev(np.zeros(3, np.float32))
    second = whole(("tile", TH + 1, TW + 1), lambda: noise((1, TH + 1, TW + 1), 100 * (TH + 1) + TW + 1), 1, TH + 1, TW + 1, out2)
    assert not np.array_equal(first, second)
    np.testing.assert_array_equal(whole("odd", None, P, H, W, out), first)
