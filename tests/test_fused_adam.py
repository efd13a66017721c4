"""gs2m_adam_step (gs2mesh_amd/csrc/optim_kernels.h) against the plain numpy statement of its arithmetic
(tests/adam_statement.py) on both back-ends, bit for bit (equal NaN positions, equal bits elsewhere); and the statement
against its two yardsticks, Adam evaluated in double and torch.optim.Adam(foreach=False) on CPU tensors, within the
tolerances include/gs2mesh_amd.h states."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import adam_statement as st
from gs2mesh_amd import _lib, optim
from gs2mesh_amd.rasterizer import _ptr

F32 = np.float32
WG = st.WG_ELEMS
WIDTHS = (3, 3, 45, 1, 3, 4)                      # xyz, f_dc, f_rest, opacity, scaling, rotation
LRS = (0.00016, 0.0025, 0.000125, 0.05, 0.005, 0.001)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs2mesh_amd.h")


def header_number(name):
    return float(re.search(rf"#define {name}\s+([0-9.]+)", open(HEADER).read()).group(1))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, ref, what):
    got, ref = np.asarray(got).reshape(np.shape(ref)), np.asarray(ref)
    gn, rn = np.isnan(got), np.isnan(ref)
    np.testing.assert_array_equal(gn, rn, err_msg=what + ": NaN positions")
    np.testing.assert_array_equal(bits(got)[~rn], bits(ref)[~rn], err_msg=what)


def decades(rng, shape):
    """normal x 10^U(-8, 0)"""
    return (rng.normal(0, 1, shape) * 10.0 ** rng.uniform(-8, 0, shape)).astype(F32)


def segment(rng, shape, step=1, lr=0.0025, betas=(0.9, 0.999), eps=1e-15, grad=None, fresh=False):
    """one tensor with state as after some steps (``fresh``: zero moments)"""
    return dict(param=rng.normal(0, 1, shape).astype(F32), grad=decades(rng, shape) if grad is None else grad,
                exp_avg=np.zeros(shape, F32) if fresh else decades(rng, shape),
                exp_avg_sq=np.zeros(shape, F32) if fresh else decades(rng, shape) ** 2,
                step=step, lr=lr, betas=betas, eps=eps)


def model_segments(rng, P, steps=(3,) * 6):
    """the six tensors of a GaussianModel of P rows, each with its own learning rate, betas and step"""
    shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4))
    return [segment(rng, sh, step=t, lr=lr, betas=(0.9 - 0.01 * k, 0.999 - 0.001 * k))
            for k, (sh, lr, t) in enumerate(zip(shapes, LRS, steps))]


def reference(segs, row_visible=None):
    return [st.adam(s["param"], s["grad"], s["exp_avg"], s["exp_avg_sq"], s["lr"], s["betas"], s["eps"], s["step"], row_visible)
            for s in segs]


def run(backend, segs, row_visible=None, offset=0):
    """the kernel on copies of the arrays -> [(p', m', v')] on the host.  ``offset``: elements by which every buffer is
    moved off its 16-byte alignment"""
    def dev(a):
        flat = np.concatenate([np.zeros(offset, F32), np.ravel(a)]) if offset else a.copy()   # the emulator's device is the host
        d = backend.dev(flat)
        return d[offset:].reshape(a.shape) if offset else d
    d = [dict(s, **{k: dev(s[k]) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}) for s in segs]
    optim.adam_step(d, row_visible=None if row_visible is None else backend.dev(np.asarray(row_visible, np.int32)), lib=backend.lib)
    backend.sync()
    return [tuple(backend.host(s[k]) for k in ("param", "exp_avg", "exp_avg_sq")) for s in d]


def check(backend, segs, row_visible=None, offset=0):
    got, ref = run(backend, segs, row_visible, offset), reference(segs, row_visible)
    for i, (g, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), g, r):
            assert_same(a, b, f"segment {i} {name}")
    return got, ref


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025])
def test_single_segment_around_the_vector_tail_and_the_workgroup(backend, count):
    check(backend, [segment(np.random.default_rng(count), (count,), step=7)])


@pytest.mark.parametrize("count", [5, 1025])
def test_buffers_off_the_16_byte_alignment_take_the_scalar_path(backend, count):
    check(backend, [segment(np.random.default_rng(count), (count,), step=7)], offset=1)


@pytest.mark.parametrize("P", [1, 5, 64, 85, 257])
def test_the_models_six_tensors_with_their_own_scalars(backend, P):
    check(backend, model_segments(np.random.default_rng(P), P, steps=(1, 2, 3, 1000, 100000, 17)))


def test_eight_segments_in_one_call(backend):
    rng = np.random.default_rng(8)
    counts = (1, WG, WG + 1, 7, 300, 2 * WG + 3, 4, 1000)
    check(backend, [segment(rng, (c,), step=k + 1, lr=0.001 * (k + 1)) for k, c in enumerate(counts)])


def test_zero_count_segment_between_two_others(backend):
    rng = np.random.default_rng(9)
    got, _ = check(backend, [segment(rng, (WG + 5,)), segment(rng, (0,)), segment(rng, (37, 3), lr=0.01)])
    assert got[1][0].size == 0


def test_every_count_zero_launches_nothing(backend):
    rng = np.random.default_rng(10)
    run(backend, [segment(rng, (0,)), segment(rng, (0, 3))])


@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
def test_steps_up_to_the_underflow_of_the_bias_correction(backend, t):
    if t == 100000:
        assert 1.0 - 0.999 ** t == 1.0 and 1.0 - 0.9 ** t == 1.0
    check(backend, [segment(np.random.default_rng(t), (WG + 77,), step=t, fresh=(t == 1))])


# ---- gradient content -----------------------------------------------------------------------------------------------------
def content(kind, n, rng):
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == "zeros":
        return np.zeros(n, F32)
    if kind == "tiny":
        return (sign * 1e-20).astype(F32)
    if kind == "huge":
        return (sign * 1e20).astype(F32)
    if kind == "overflow":
        return (sign * 1e25).astype(F32)
    assert kind == "nonfinite"
    g = decades(rng, n)
    g[0::4], g[1::4], g[2::4] = np.nan, np.inf, -np.inf
    return g


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("kind", ["zeros", "tiny", "huge", "overflow", "nonfinite"])
def test_gradient_content_at_the_edges_of_f32(backend, kind, fresh):
    rng = np.random.default_rng(len(kind) + fresh)
    n = WG + 13
    seg = segment(rng, (n,), step=1 if fresh else 5, grad=content(kind, n, rng), fresh=fresh)
    got, ref = check(backend, [seg])
    p2, m2, v2 = ref[0]
    if kind == "zeros" and fresh:
        assert_same(p2, seg["param"], "0 / eps leaves the parameter")
        assert not m2.any() and not v2.any()
    if kind == "tiny":
        sq = (st.scalars(seg["lr"], seg["betas"], seg["eps"], seg["step"])["omb2"] * seg["grad"]) * seg["grad"]
        assert np.all(sq > 0) and np.all(sq < np.finfo(F32).tiny)              # (omb2 * g) * g is a subnormal, not 0
        assert np.all(seg["grad"] * seg["grad"] < np.finfo(F32).tiny)
        if fresh:
            assert_same(v2, sq, "the subnormal is kept")
    if kind == "huge":
        # g * g overflows; the form never takes that product: (omb2 * g) * g = 1e37 is finite and the step is an ordinary one
        with np.errstate(over="ignore"):
            assert np.all(np.isposinf(seg["grad"] * seg["grad"]))
        assert np.all(np.isfinite(v2)) and np.all(v2 > 9e36) and np.all(np.isfinite(p2))
        nxt = dict(seg, param=p2, exp_avg=m2, exp_avg_sq=v2, grad=decades(rng, n), step=seg["step"] + 1)
        check(backend, [nxt])
    if kind == "overflow":
        assert np.all(np.isposinf(v2)) and np.all(np.isfinite(m2))
        assert_same(p2, seg["param"], "an infinite second moment gives a zero update")
        # the following step runs from that state
        nxt = dict(seg, param=p2, exp_avg=m2, exp_avg_sq=v2, grad=decades(rng, n), step=seg["step"] + 1)
        _, ref2 = check(backend, [nxt])
        assert_same(ref2[0][0], p2, "and stays there")
        assert np.all(np.isposinf(ref2[0][2]))
    if kind == "nonfinite":
        assert np.isnan(p2[0::4]).all() and np.isnan(p2[1::4]).all() and np.isnan(p2[2::4]).all()
        assert np.isfinite(p2[3::4]).all()


def test_decades_of_gradient_on_zero_and_non_zero_state_with_exact_zeros(backend):
    rng = np.random.default_rng(21)
    for fresh in (True, False):
        g = decades(rng, (2 * WG + 1,))
        g[::3] = 0.0
        check(backend, [segment(rng, g.shape, step=1 if fresh else 9, grad=g, fresh=fresh)])


# ---- runs -----------------------------------------------------------------------------------------------------------------
def test_three_consecutive_steps_carry_the_state(backend):
    rng = np.random.default_rng(30)
    segs = model_segments(rng, 85, steps=(1,) * 6)
    for s in segs:
        s["exp_avg"], s["exp_avg_sq"] = np.zeros_like(s["param"]), np.zeros_like(s["param"])
    for t in (1, 2, 3):
        got, _ = check(backend, segs)
        segs = [dict(s, param=g[0], exp_avg=g[1], exp_avg_sq=g[2], grad=decades(rng, s["param"].shape), step=t + 1)
                for s, g in zip(segs, got)]


def test_two_runs_from_equal_inputs_give_equal_bits(backend):
    segs = model_segments(np.random.default_rng(31), 257)
    a, b = run(backend, segs), run(backend, segs)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(bits(u), bits(v))


# ---- row-sparse -----------------------------------------------------------------------------------------------------------
def pattern(kind, P):
    rng = np.random.default_rng(P)
    vals = np.array([0, 1, 7], np.int32)
    if kind == "alternating":
        return vals[np.arange(P) % 3]
    if kind == "blocked":
        return vals[(np.arange(P) // 19) % 3]
    if kind == "random":
        return vals[rng.integers(0, 3, P)]
    if kind == "none":
        return np.zeros(P, np.int32)
    assert kind == "all"
    return vals[1 + np.arange(P) % 2]


@pytest.mark.parametrize("P", [5, 85, 257])
@pytest.mark.parametrize("kind", ["alternating", "blocked", "random", "none", "all"])
def test_row_sparse_updates_the_visible_rows_only(backend, kind, P):
    rng = np.random.default_rng(40 + P)
    vis = pattern(kind, P)
    segs = model_segments(rng, P)
    dense = reference(segs) if kind == "all" else None
    for s in segs:                                             # the gradient of an unseen row is never read
        s["grad"] = s["grad"].copy()
        s["grad"][vis <= 0] = np.nan
    got, _ = check(backend, segs, row_visible=vis)
    for s, g in zip(segs, got):
        for name, a in zip(("param", "exp_avg", "exp_avg_sq"), g):
            np.testing.assert_array_equal(bits(a[vis <= 0]), bits(s[name][vis <= 0]), err_msg=name)
            assert not np.isnan(a).any()
    if kind == "all":
        plain = run(backend, segs)
        for a, b, c in zip(got, plain, dense):
            for x, y, z in zip(a, b, c):
                np.testing.assert_array_equal(bits(x), bits(y))
                np.testing.assert_array_equal(bits(x), bits(z))
    if kind == "none":
        for s, g in zip(segs, got):
            np.testing.assert_array_equal(bits(g[0]), bits(s["param"]))


# ---- errors ---------------------------------------------------------------------------------------------------------------
def raw_call(backend, arrays, n=None, row_visible=None, rows=0):
    """the C entry itself; ``arrays``: dicts of device buffers (or None) with count / row_width / step"""
    table = (_lib.AdamSegment * max(len(arrays), 1))()
    for s, a in zip(table, arrays):
        s.param, s.grad, s.exp_avg, s.exp_avg_sq = (_ptr(a[k]) for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
        s.count, s.step, s.row_width = a["count"], a.get("step", 1), a.get("row_width", 1)
        s.lr, s.beta1, s.beta2, s.eps = 0.01, 0.9, 0.999, 1e-15
    rc = backend.lib.gs2m_adam_step(len(arrays) if n is None else n, table, _ptr(row_visible), rows, C.c_void_p(0))
    backend.sync()
    return rc, backend.lib.gs2m_last_error().decode()


ERRORS = {
    "no segments": (dict(n=0), "n_segments"),
    "nine segments": (dict(n=9), "n_segments"),
    "NULL pointer": (dict(null="exp_avg_sq"), "NULL exp_avg_sq"),
    "row_width 0": (dict(row_width=0), "row_width"),
    "count not rows x row_width": (dict(rows=3), "rows x row_width"),
    "param overlaps exp_avg": (dict(overlap=True), "overlaps"),
}


@pytest.mark.parametrize("case", list(ERRORS))
def test_bad_arguments_are_refused_with_a_message_and_nothing_is_written(backend, case):
    how, message = ERRORS[case]
    rng = np.random.default_rng(50)
    n = 12
    host = {k: rng.normal(0, 1, n).astype(F32) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
    host["exp_avg_sq"] = host["exp_avg_sq"] ** 2
    good = {k: backend.dev(v.copy()) for k, v in host.items()}
    bad = {k: backend.dev(v.copy()) for k, v in host.items()}
    bad.update(count=n, row_width=how.get("row_width", 3))
    good.update(count=n, row_width=3)
    if "null" in how:
        bad[how["null"]] = None
    if "overlap" in how:
        big = backend.dev(np.concatenate([host["param"], host["exp_avg"]]))
        bad["param"], bad["exp_avg"] = big[:n], big[n - 1:2 * n - 1]
    vis = backend.dev(np.ones(how["rows"], np.int32)) if "rows" in how else None
    rc, msg = raw_call(backend, [good, bad], n=how.get("n"), row_visible=vis, rows=how.get("rows", 0))
    assert rc != 0 and message in msg and msg.startswith("gs2m_adam_step"), (rc, msg)
    for k, v in host.items():                                  # the good segment before the bad one was not stepped either
        np.testing.assert_array_equal(bits(backend.host(good[k])), bits(v))
        if bad[k] is not None and "overlap" not in how:
            np.testing.assert_array_equal(bits(backend.host(bad[k])), bits(v))
    rc, msg = raw_call(backend, [good])                        # and the same buffers are accepted on their own
    assert rc == 0, msg
    assert not np.array_equal(bits(backend.host(good["param"])), bits(host["param"]))


def test_a_grid_past_the_launch_limit_is_refused_before_anything_is_touched():
    """more than 2^31 - 1 workgroups of 1024 elements: refused on the count alone (the pointers are never followed, so the
    emulator back-end is enough; no such tensor can be allocated)"""
    from backends import make
    lib = make("emu").lib
    table = (_lib.AdamSegment * 2)()
    for k, s in enumerate(table):
        base = (1 + 4 * k) << 44
        s.param, s.grad, s.exp_avg, s.exp_avg_sq = base, base + (1 << 44), base + (2 << 44), base + (3 << 44)
        s.count, s.step, s.row_width = (1 << 30) * WG, 1, 1       # 2^30 workgroups each: only the sum is past the limit
        s.lr, s.beta1, s.beta2, s.eps = 0.01, 0.9, 0.999, 1e-15
    assert lib.gs2m_adam_step(2, table, None, 0, C.c_void_p(0)) != 0
    assert "2^31 - 1 workgroups" in lib.gs2m_last_error().decode()
    table[0].count = (1 << 31) * WG
    assert lib.gs2m_adam_step(1, table, None, 0, C.c_void_p(0)) != 0
    assert "segment 0" in lib.gs2m_last_error().decode() and "2^31 - 1 workgroups" in lib.gs2m_last_error().decode()


def test_the_wrapper_refuses_a_mask_of_another_length(backend):
    rng = np.random.default_rng(51)
    with pytest.raises(ValueError, match="rows"):
        run(backend, [segment(rng, (6, 3))], row_visible=np.ones(5, np.int32))


# ---- the statement against its two yardsticks (CPU only; never the kernel) ---------------------------------------------------
def ulp(x):
    x = np.abs(np.asarray(x, F32))
    return (np.nextafter(x, F32(np.inf)) - x).astype(np.float64)


@pytest.fixture(scope="module")
def fifty_steps():
    """the issue's run: 200 000 elements, gradients over eight decades, lr 0.0025, eps 1e-15; the statement, Adam in double and
    torch.optim.Adam(foreach=False) side by side -> the largest error of a single step from identical state (in u(1)), and
    the errors after 50 carried steps (in u(50)), u(T) = ulp(p) + T * lr * 2^-23"""
    lr, eps, betas, n = 0.0025, 1e-15, (0.9, 0.999), 200_000
    rng = np.random.default_rng(0)
    p0 = rng.normal(0, 1, n).astype(F32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, eps=eps, betas=betas, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, F32), np.zeros(n, F32)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    out = dict(step64=0.0, lr=lr)
    for t in range(1, 51):
        g = decades(rng, n)
        if t % 7 == 0:
            g[::3] = 0
        q64, _, _ = st.adam64(p, g, m, v, lr, betas, eps, t)                       # one step in double from the f32 state
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p64, m64, v64 = st.adam64(p64, g, m64, v64, lr, betas, eps, t)
        p, m, v = st.adam(p, g, m, v, lr, betas, eps, t)
        out["step64"] = max(out["step64"], float((np.abs(p - q64) / (ulp(q64) + lr * 2.0 ** -23)).max()))
        if t == 1:
            tt = tp.detach().numpy().copy()
            out["step_torch"] = float((np.abs(p.astype(np.float64) - tt) / (ulp(tt) + lr * 2.0 ** -23)).max())
    tt = tp.detach().numpy()
    out["carried64"] = float((np.abs(p - p64) / (ulp(p64) + 50 * lr * 2.0 ** -23)).max())
    out["carried_torch"] = float((np.abs(p.astype(np.float64) - tt) / (ulp(tt) + 50 * lr * 2.0 ** -23)).max())
    st_m, st_v = opt.state[tp]["exp_avg"].numpy(), opt.state[tp]["exp_avg_sq"].numpy()
    out["moments"] = (float(np.abs(m - st_m).max()), float(np.abs(v - st_v).max()))
    return out


@pytest.mark.parametrize("which,define", [("step64", "GS2M_ADAM_TOL_FP64_STEP"), ("step_torch", "GS2M_ADAM_TOL_TORCH_STEP"),
                                          ("carried64", "GS2M_ADAM_TOL_FP64_50"), ("carried_torch", "GS2M_ADAM_TOL_TORCH_50")])
def test_statement_against_fp64_and_torch_adam(fifty_steps, which, define):
    print(which, fifty_steps[which], "of", header_number(define), "| moments", fifty_steps["moments"])
    assert fifty_steps[which] <= header_number(define)
