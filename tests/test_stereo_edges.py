"""The stereo stage at its edges, on both back-ends and without tolerances: gs2m_stereo_sgm (gs2mesh_amd/csrc/sgm_kernels.h)
at every disparity width K = D / 64 = 1..16, at image sizes around the 64-step chunk of the horizontal kernel and below the
census window, on content with ties, saturated path costs and winners at d* = D-1, with every selection of its outputs and a
dirty scratch; and gs2m_stereo_depth_occlusion (stereo_kernels.hip) at truncation, clipping and non-finite disparities.

The matcher's reference is the numpy statement (tests/sgm_statement.py): S (tap), disp_lr and disp_rl are compared bit for
bit.  A statement result is computed once per case and shared between the back-ends (``_REF``); it is never modified.  What a
case is there for (ties, the largest path cost, the sub-pixel step, the last disparity) is asserted on the statement's result
first, so a case cannot pass without reaching its edge; the measured figures are printed (``-s``; profiles/stereo_edges.txt).
"""
import ctypes as C
import os
import platform

import numpy as np
import pytest

import sgm_statement
from gs2mesh_amd import stereo_utils, synthetic
from gs2mesh_amd.rasterizer import _ptr

_REF = {}
SENTINEL_F32 = np.float32(-7.0)
SENTINEL_U16 = 0xABCD


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- content ------------------------------------------------------------------------------------------------------------
def noise(W, H, D):
    """two independent noise images with independent channels: the 77 / 150 / 29 grey weights matter"""
    rng = np.random.default_rng(1000 * W + 10 * H + D)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def dots(W, H, D):
    left, right, _ = synthetic.random_dot_stereogram(W, H, W + H)
    return left, right


def flat(W, H, D):
    a = np.full((H, W, 3), 255, np.uint8)
    return a, a.copy()


def steps(W, H, D):
    """two grey plateaus split at W/2, the lower half of the image 40 brighter; right = left rolled by -3"""
    g = np.full((H, W), 60, np.uint8)
    g[:, W // 2:] = 150
    g[H // 2:] += 40
    left = np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
    return left, np.ascontiguousarray(np.roll(left, -3, axis=1))


def last_disparity(W, H, D):
    """the known answer d* = D-1 for every pixel whose match is inside the image"""
    left = noise(W, H, D)[0]
    return left, np.ascontiguousarray(np.roll(left, -(D - 1), axis=1))


CONTENT = {"noise": noise, "dots": dots, "flat": flat, "steps": steps, "last": last_disparity}


class Case:
    """one input and everything the statement says about it"""

    def __init__(self, kind, W, H, D, p1, p2):
        self.kind, self.W, self.H, self.D, self.p1, self.p2 = kind, W, H, D, p1, p2
        self.left, self.right = CONTENT[kind](W, H, D)
        assert self.left.shape == self.right.shape == (H, W, 3) and self.left.dtype == self.right.dtype == np.uint8
        self.lr, self.rl, self.S = sgm_statement.sgm(self.left, self.right, D, p1, p2)
        assert 0 <= self.S.min() and self.S.max() <= 4 * (62 + p2) <= 0xFFFF
        for a in (self.left, self.right, self.lr, self.rl, self.S):
            a.setflags(write=False)

    def right_pass_cost(self):
        """S of the right-based pass in the right image's coordinates (d is the same number in both)"""
        gl, gr = sgm_statement.grey(self.left), sgm_statement.grey(self.right)
        return sgm_statement.sgm_grey(gr[:, ::-1], gl[:, ::-1], self.D, self.p1, self.p2)[1][:, ::-1]

    def path_maxima(self):
        """the largest cost of each of the four paths of the left-based pass"""
        Cv = sgm_statement.cost_volume(sgm_statement.census(sgm_statement.grey(self.left)),
                                       sgm_statement.census(sgm_statement.grey(self.right)), self.D)
        return [int(sgm_statement.aggregate(Cv, dy, dx, self.p1, self.p2).max()) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0))]


def case(kind, W, H, D, p1=10, p2=120):
    key = (kind, W, H, D, p1, p2)
    if key not in _REF:
        _REF[key] = Case(*key)
    return _REF[key]


def tied_fraction(S):
    """fraction of the pixels whose two lowest values of S are equal"""
    two = np.partition(S, 1, axis=-1)[..., :2]
    return float((two[..., 0] == two[..., 1]).mean())


def fractional(disp):
    return float((disp != np.floor(disp)).mean())


def match(backend, c):
    """(disp_lr, disp_rl, S) of the back-end through the package's own entry point"""
    lr, rl, S = stereo_utils.sgm_disparity(backend.dev(c.left.copy()), backend.dev(c.right.copy()), c.D, c.p1, c.p2, tap=True, lib=backend.lib)
    backend.sync()
    return backend.host(lr), backend.host(rl), backend.host(S).view(np.uint16)


def check(backend, c):
    """S, disp_lr and disp_rl of the back-end equal the statement bit for bit"""
    if c.kind in ("noise", "dots") and c.W >= 64:           # the sub-pixel step is exercised
        f = fractional(c.lr), fractional(c.rl)
        print(f"{c.kind} {c.W}x{c.H} D={c.D} p=({c.p1},{c.p2}): fractional lr {f[0]:.3f} rl {f[1]:.3f}")
        assert f[0] >= 0.3
    lr, rl, S = match(backend, c)
    assert S.shape == (c.H, c.W, c.D) and lr.shape == rl.shape == (c.H, c.W) and lr.dtype == rl.dtype == np.float32
    np.testing.assert_array_equal(S, c.S.astype(np.uint16))
    np.testing.assert_array_equal(bits(lr), bits(c.lr))
    np.testing.assert_array_equal(bits(rl), bits(c.rl))


# ---- 1. every width -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p1,p2", [(10, 120), (120, 190)])
@pytest.mark.parametrize("k", range(1, 17))
def test_every_width(backend, k, p1, p2):
    """D = 64 k on 72 x 10 noise: most candidates of most pixels are outside the image (W < D from k = 2 on)"""
    check(backend, case("noise", 72, 10, 64 * k, p1, p2))


@pytest.mark.parametrize("p1,p2", [(10, 120), (120, 190)])
@pytest.mark.parametrize("k", [3, 12, 16])
def test_widths_with_every_candidate_inside(backend, k, p1, p2):
    """W = D + 5: the last five columns have all D candidates inside the image (3-byte, 24-byte and the widest packs)"""
    D = 64 * k
    check(backend, case("noise", D + 5, 3, D, p1, p2))


# ---- 2. image edges -----------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(1, 1), (8, 2), (63, 6), (64, 7), (65, 1), (127, 3), (128, 9), (129, 3), (200, 8)]


@pytest.mark.parametrize("kind", ["dots", "noise", "flat", "steps"])
@pytest.mark.parametrize("W,H", EDGE_SHAPES)
@pytest.mark.parametrize("D", [64, 128])
def test_image_edges(backend, D, W, H, kind):
    """one pixel, one partial chunk, exact multiples of the 64-step chunk and one past them, rows inside the census window,
    a single row (no vertical step)"""
    p1, p2 = (1, 1) if kind == "flat" else (10, 120)
    c = case(kind, W, H, D, p1, p2)
    if kind == "flat":                                      # every cost inside the image is 0 and leaving d = 0 costs p1
        assert np.all(c.lr == 0) and np.all(c.rl == 0)
    check(backend, c)


# ---- 3. content ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D", [(72, 10, 192), (64, 8, 64), (200, 8, 128)])
def test_ties_take_the_lowest_disparity(backend, W, H, D):
    """plateaus: at least a quarter of the pixels have two equal lowest S in both passes and at least 100 win at d* = 0, so
    the (S << 10) | d key decides.  Measured on the statement: tied 0.79 to 0.93 (left-based), 0.45 to 0.49 (right-based)."""
    c = case("steps", W, H, D)
    tl, tr = tied_fraction(c.S), tied_fraction(c.right_pass_cost())
    zero = int((c.S.argmin(-1) == 0).sum())
    print(f"steps {W}x{H} D={D}: tied lr {tl:.3f} rl {tr:.3f}, winners at d*=0: {zero}")
    assert tl >= 0.25 and tr >= 0.25
    assert zero >= 100
    check(backend, c)


def test_largest_path_cost(backend):
    """noise with p2 = 190: every one of the four paths reaches 62 + p2 = 252, the most a u8 plane has to hold, and S
    reaches 1000 of the 1008 a u16 sum can get (measured: 1008)"""
    c = case("noise", 72, 10, 192, 120, 190)
    maxima = c.path_maxima()
    print(f"noise 72x10 D=192 p=(120,190): path maxima {maxima}, S.max {int(c.S.max())}")
    assert maxima == [62 + 190] * 4
    assert c.S.max() >= 1000
    check(backend, c)


@pytest.mark.parametrize("D", [64, 192])
def test_last_disparity(backend, D):
    """right = roll(left, -(D-1)): at least 100 pixels win at d* = D-1, where there is no sub-pixel step"""
    W, H = D + 40, 8
    c = case("last", W, H, D)
    last = c.S.argmin(-1) == D - 1
    print(f"last {W}x{H} D={D}: winners at d*=D-1: {int(last.sum())}")
    assert last.sum() >= 100
    assert np.all(c.lr[last] == np.float32(D - 1))
    lr, rl, S = match(backend, c)
    np.testing.assert_array_equal(bits(lr[last]), bits(c.lr[last]))
    np.testing.assert_array_equal(S, c.S.astype(np.uint16))
    np.testing.assert_array_equal(bits(lr), bits(c.lr))
    np.testing.assert_array_equal(bits(rl), bits(c.rl))


# ---- 4. pass selection and scratch --------------------------------------------------------------------------------------
def aligned(nbytes, byte):
    """nbytes of `byte` at a 64-byte aligned host address (the C ABI asks for 16 of scratch and tap)"""
    raw = np.empty(nbytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + nbytes]
    a[:] = byte
    return a


class Direct:
    """gs2m_stereo_sgm through the C ABI with sentinel-filled outputs and a scratch of the caller's making"""

    def __init__(self, backend, c):
        self.b, self.c, self.lib = backend, c, backend.lib
        self.need = int(self.lib.gs2m_stereo_sgm_scratch_bytes(c.W, c.H, c.D))
        assert self.need > 0
        self.nbytes = self.need
        self.left, self.right = backend.dev(c.left.copy()), backend.dev(c.right.copy())
        self.scratch = None
        self.fill_scratch(0)

    def fill_scratch(self, byte):
        self.scratch = self.b.dev(aligned(self.nbytes, byte))

    def __call__(self, lr=False, rl=False, tap=False, c=None):
        """-> (disp_lr, disp_rl, S) on the host; outputs that were not asked for come back None after their buffers were
        checked to still hold the sentinel"""
        c = c or self.c
        left, right = (self.left, self.right) if c is self.c else (self.b.dev(c.left.copy()), self.b.dev(c.right.copy()))
        out_lr = self.b.dev(np.full((c.H, c.W), SENTINEL_F32, np.float32))
        out_rl = self.b.dev(np.full((c.H, c.W), SENTINEL_F32, np.float32))
        n = c.H * c.W * c.D
        tap_fill = aligned(2 * n, 0).view(np.uint16)
        tap_fill[:] = SENTINEL_U16
        out_tap = self.b.dev(tap_fill.view(np.int16))
        rc = self.lib.gs2m_stereo_sgm(_ptr(left), _ptr(right), c.W, c.H, c.D, c.p1, c.p2, _ptr(out_lr) if lr else None,
                                      _ptr(out_rl) if rl else None, _ptr(self.scratch), self.nbytes,
                                      _ptr(out_tap) if tap else None, C.c_void_p(0))
        assert rc == 0, self.lib.gs2m_last_error()
        self.b.sync()
        h_lr, h_rl = self.b.host(out_lr), self.b.host(out_rl)
        h_tap = self.b.host(out_tap).view(np.uint16).reshape(c.H, c.W, c.D)
        if not lr:
            assert np.all(bits(h_lr) == bits(SENTINEL_F32)), "disp_lr was written without being asked for"
        if not rl:
            assert np.all(bits(h_rl) == bits(SENTINEL_F32)), "disp_rl was written without being asked for"
        if not tap:
            assert np.all(h_tap == SENTINEL_U16), "the tap was written without being asked for"
        return (h_lr if lr else None), (h_rl if rl else None), (h_tap if tap else None)

    def equal(self, got, c=None):
        c = c or self.c
        lr, rl, S = got
        if lr is not None:
            np.testing.assert_array_equal(bits(lr), bits(c.lr))
        if rl is not None:
            np.testing.assert_array_equal(bits(rl), bits(c.rl))
        if S is not None:
            np.testing.assert_array_equal(S, c.S.astype(np.uint16))


SELECTIONS = {"rl": dict(rl=True), "lr": dict(lr=True), "tap": dict(tap=True), "tap+rl": dict(tap=True, rl=True)}


@pytest.mark.parametrize("sel", sorted(SELECTIONS))
def test_a_selection_is_its_part_of_the_full_call(backend, sel):
    c = case("noise", 129, 3, 128)
    call = Direct(backend, c)
    full = call(lr=True, rl=True, tap=True)
    call.equal(full)
    part = call(**SELECTIONS[sel])
    assert [x is not None for x in part] == [SELECTIONS[sel].get(k, False) for k in ("lr", "rl", "tap")]
    call.equal(part)
    for a, b in zip(part, full):
        if a is not None:
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_scratch_need_not_be_clean(backend):
    c = case("noise", 129, 3, 128)
    call = Direct(backend, c)
    results = []
    for byte in (0xFF, 0x00):
        call.fill_scratch(byte)
        results.append(call(lr=True, rl=True, tap=True))
        call.equal(results[-1])
    for a, b in zip(*results):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_narrow_call_after_the_widest_in_one_scratch(backend):
    wide, narrow = case("noise", 129, 3, 1024), case("noise", 129, 3, 64)
    call = Direct(backend, wide)
    assert call.need >= int(backend.lib.gs2m_stereo_sgm_scratch_bytes(narrow.W, narrow.H, narrow.D))
    call.equal(call(lr=True, rl=True, tap=True))
    call.equal(call(lr=True, rl=True, tap=True, c=narrow), narrow)


# ---- 5. gs2m_stereo_depth_occlusion -------------------------------------------------------------------------------------
FB = 2892.33 * 0.245


def ordinary_disparities(W, H):
    """(disp_lr, disp_rl) in half pixels, so that |x - xr| meets the thresholds 0, 0.5 and 3 exactly as well as from
    either side; then, in two of five entries: x - l in (-1, 0) and in (W-1, W) (truncation toward zero against the xp < 0
    and xp >= W tests), zero and negative disparities, and disp_rl that carries xr past either clip"""
    rng = np.random.default_rng(100 * W + H)
    q = lambda lo, hi: (rng.integers(2 * lo, 2 * hi + 1, (H, W)) / 2.0).astype(np.float32)
    L, R = np.float32(2.0) + q(-2, 2), np.float32(2.0) + q(-2, 2)
    x = np.broadcast_to(np.arange(W, dtype=np.float32), (H, W))
    pick = rng.integers(0, 24, (H, W))
    special = [x + np.float32(0.5), x + np.float32(0.75), x + np.float32(1.0), x - np.float32(W - 0.5), x - np.float32(W - 1),
               x - np.float32(W), np.zeros_like(x), -np.zeros_like(x), -q(0, 3), x + q(0, 3)]
    for i, s in enumerate(special):
        L = np.where(pick == i, s.astype(np.float32), L)
    pick = rng.integers(0, 12, (H, W))
    R = np.where(pick == 0, np.float32(W + 5), np.where(pick == 1, np.float32(-W - 5), np.where(pick == 2, -R, R)))
    return np.ascontiguousarray(L, np.float32), np.ascontiguousarray(R, np.float32)


def depth_equal(got, L):
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.float32(FB) / L
    assert got.dtype == np.float32
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(ref)[~nan])
    return ref


def statement_mask(L, R, thr):
    with np.errstate(invalid="ignore"):
        return sgm_statement.occlusion(L, R, thr).astype(np.uint8)


@pytest.mark.parametrize("thr", [0, 0.5, 3])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", [1, 255, 256, 257])
def test_depth_and_occlusion_at_the_edges(backend, W, H, thr):
    L, R = ordinary_disparities(W, H)
    ref = statement_mask(L, R, thr)
    if W > 1:
        xg = np.arange(W)
        assert np.any((xg - L > -1) & (xg - L < 0)) and np.any((xg - L > W - 1) & (xg - L < W))
        assert np.any(L == 0) and np.any(L < 0) and 0.02 < ref.mean() < 0.98
    dL, dR = backend.dev(L), backend.dev(R)
    depth, mask = stereo_utils.depth_and_occlusion(dL, dR, 2892.33, 0.245, thr, lib=backend.lib)
    backend.sync()
    d = depth_equal(backend.host(depth), L)
    assert np.all(np.isinf(d[L == 0]))
    assert backend.host(mask).dtype == np.uint8
    np.testing.assert_array_equal(backend.host(mask), ref)
    # mask only; depth only, without disp_rl
    none, mask = stereo_utils.depth_and_occlusion(dL, dR, 2892.33, 0.245, thr, want_depth=False, lib=backend.lib)
    assert none is None
    np.testing.assert_array_equal(backend.host(mask), ref)
    out = backend.dev(np.zeros((H, W), np.float32))
    assert backend.lib.gs2m_stereo_depth_occlusion(_ptr(dL), None, W, H, FB, float(thr), _ptr(out), None, C.c_void_p(0)) == 0
    backend.sync()
    depth_equal(backend.host(out), L)
    assert backend.lib.gs2m_stereo_depth_occlusion(_ptr(dL), None, W, H, FB, float(thr), None, _ptr(out), C.c_void_p(0)) == 1


NONFINITE_LR = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e20": 1e20, "-1e20": -1e20, "3e9": 3e9, "-3e9": -3e9}
NONFINITE_RL = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
NONFINITE_THR = 3
# where the value goes.  disp_lr: in every row a column within the threshold of disp_rl[y][0] = 5 (the pixels that a NaN
# converted to 0 would call visible) and one far from it.  disp_rl: column 100, which the pixels x = 102 (disp_lr = 2) read.
NONFINITE_LR_AT = [(0, 5), (1, 3), (2, 8), (1, 200)]
NONFINITE_RL_AT, NONFINITE_RL_READER = [(0, 100), (1, 100), (2, 100)], [(0, 102), (1, 102), (2, 102)]


def nonfinite_case(golden, side, name):
    """(disp_lr, disp_rl, expected mask, the pixels the value decides) from tests/golden/stereo_nonfinite.npz"""
    L, R = golden["L2R"].copy(), golden["R2L"].copy()
    at = NONFINITE_LR_AT if side == "lr" else NONFINITE_RL_AT
    for y, x in at:
        (L if side == "lr" else R)[y, x] = np.float32((NONFINITE_LR if side == "lr" else NONFINITE_RL)[name])
    ys, xs = zip(*(at if side == "lr" else NONFINITE_RL_READER))
    return L, R, golden[f"mask_{side}_{name}"], (np.array(ys), np.array(xs))


@pytest.fixture(scope="module")
def nonfinite_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "stereo_nonfinite.npz")))


def run_nonfinite(backend, L, R, expected):
    if platform.machine() in ("x86_64", "AMD64"):           # the fixture is what the statement gives on x86-64 numpy
        np.testing.assert_array_equal(statement_mask(L, R, NONFINITE_THR), expected)
    depth, mask = stereo_utils.depth_and_occlusion(backend.dev(L), backend.dev(R), 2892.33, 0.245, NONFINITE_THR, lib=backend.lib)
    backend.sync()
    depth_equal(backend.host(depth), L)
    got = backend.host(mask)
    print("mask at the expected-occluded / visible pixels:", got[expected == 0].mean(), got[expected == 1].mean())
    return got


@pytest.mark.parametrize("name", sorted(NONFINITE_LR))
def test_nonfinite_disp_lr_is_occluded(backend, nonfinite_golden, name):
    """a pixel whose x - disp_lr is NaN or outside int32 is occluded"""
    L, R, expected, where = nonfinite_case(nonfinite_golden, "lr", name)
    assert np.all(R[:, 0] == 5) and np.all(expected[where] == 0)
    got = run_nonfinite(backend, L, R, expected)
    assert np.all(got[where] == 0), got[where]
    np.testing.assert_array_equal(got, expected)


@pytest.mark.parametrize("name", sorted(NONFINITE_RL))
def test_nonfinite_disp_rl(backend, nonfinite_golden, name):
    """NaN in disp_rl compares false with every threshold (visible); +-inf clip to an end of the row (occluded)"""
    L, R, expected, where = nonfinite_case(nonfinite_golden, "rl", name)
    assert np.all(L[where] == 2) and np.all(expected[where] == (1 if name == "nan" else 0))
    got = run_nonfinite(backend, L, R, expected)
    np.testing.assert_array_equal(got, expected)
