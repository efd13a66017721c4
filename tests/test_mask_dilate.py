"""gs2m_mask_dilate_disk (gs2mesh_amd/csrc/mask_disk_kernels.h) against scipy's binary_dilation with skimage's disk
(tests/dilate_statement.py) on both back-ends.  Every comparison is exact: the packed bitmap word for word, the bytes byte
for byte."""
import ctypes as C

import numpy as np
import pytest

import dilate_statement
from gs2mesh_amd import evaluation
from gs2mesh_amd.rasterizer import _ptr

RADII = [0, 1, 7, 24, 64]
GUARD = 5
_REF = {}


def masks_of(W, H, merged=False):
    """the masks of one shape: empty, full, one set pixel at each corner, at x = 63 / 64 and at the mid-edges, random at
    density 0.001 and 0.3, set bytes other than 1.  ``merged``: the single pixels and the sparse random ones share one mask and the
    empty one is left out (scipy walks the whole 129 x 129 footprint for every pixel a sparse mask leaves unset: 1.3 s per such mask of
    193 x 70 at r = 64)"""
    rng = np.random.default_rng(1000 * W + H)
    out = [np.ones((H, W), np.uint8)] if merged else [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (H // 2, W - 1), (0, W // 2), (H - 1, W // 2),
             (H // 2, min(63, W - 1)), (H // 2, min(64, W - 1))]
    if merged:
        m = np.zeros((H, W), np.uint8)
        for y, x in spots:
            m[y, x] = 1
        out.append(m | (rng.random((H, W)) < 0.001))
    else:
        for y, x in sorted(set(spots)):
            m = np.zeros((H, W), np.uint8)
            m[y, x] = 1
            out.append(m)
    if not merged:
        out.append((rng.random((H, W)) < 0.001).astype(np.uint8))
    out.append((rng.random((H, W)) < 0.3).astype(np.uint8) * 255)
    out.append((rng.random((H, W)) < 0.3).astype(np.uint8) * 2)
    return np.stack(out)


def statement(key, masks, r):
    """([n,H,W] bool, [n,H,nw] uint64), computed once per case and shared between the back-ends; never modified"""
    k = (key, r)
    if k not in _REF:
        d = np.stack([dilate_statement.dilate(m, r) for m in masks])
        _REF[k] = (d, dilate_statement.pack(d))
    return _REF[k]


def addr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run(backend, masks, r, want_bytes=True):
    """-> (bits [n,H,nw] uint64, bytes [n,H,W] u8 or None); the guard words / bytes behind both outputs are checked here"""
    lib = backend.lib
    n, H, W = masks.shape
    nw = (W + 63) // 64
    dm = backend.dev(masks)
    ptrs = (C.c_void_p * max(n, 1))(*[addr(dm) + i * H * W for i in range(n)])
    need = lib.gs2m_mask_dilate_disk_scratch_bytes(n, W, H)
    assert need == min(n, 32) * H * nw * 8
    scratch = backend.dev(np.zeros(need // 8 + 1, np.int64))
    bits = backend.dev(np.full(n * H * nw + GUARD, 0x5a5a5a5a5a5a5a5a, np.int64))
    out = backend.dev(np.full(n * H * W + GUARD, 77, np.uint8)) if want_bytes else None
    rc = lib.gs2m_mask_dilate_disk(n, W, H, ptrs, r, _ptr(bits), _ptr(out), _ptr(scratch), need, C.c_void_p(0))
    assert rc == 0, lib.gs2m_last_error()
    backend.sync()
    hb = backend.host(bits)
    assert np.all(hb[n * H * nw:] == 0x5a5a5a5a5a5a5a5a)
    hb = np.ascontiguousarray(hb[:n * H * nw]).view(np.uint64).reshape(n, H, nw)
    ho = None
    if want_bytes:
        ho = backend.host(out)
        assert np.all(ho[n * H * W:] == 77)
        ho = ho[:n * H * W].reshape(n, H, W)
    return hb, ho


def check(backend, key, masks, r):
    want, want_bits = statement(key, masks, r)
    bits, out = run(backend, masks, r)
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_array_equal(out, want.astype(np.uint8))
    W = masks.shape[2]
    if W & 63:                                                      # bits at x >= W are 0
        assert np.all(bits[:, :, -1] >> np.uint64(W & 63) == 0)


# H = 5 < r: the disk leaves the image on both sides.  W = 64 takes the 16-pixel packing, the others the ballot
@pytest.mark.parametrize("H", [1, 5, 70])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 130, 193])
def test_every_radius_equals_scipy_on_edge_pixels_and_random_masks(backend, W, H):
    masks = masks_of(W, H)
    for r in RADII:
        if r == 64 and H == 70:
            check(backend, ("merged", W, H), masks_of(W, H, merged=True), r)
        else:
            check(backend, ("shape", W, H), masks, r)
    # r = 0 is the identity
    np.testing.assert_array_equal(statement(("shape", W, H), masks, 0)[0], masks != 0)


@pytest.mark.parametrize("n", [1, 3, 33])                            # 33 crosses the batch of 32
@pytest.mark.parametrize("W,H,r", [(65, 5, 7), (130, 70, 24)])
def test_any_number_of_masks(backend, n, W, H, r):
    rng = np.random.default_rng(n)
    masks = (rng.random((n, H, W)) < 0.002).astype(np.uint8)
    masks[-1, H - 1, W - 1] = 9                                      # the last mask of the last chunk is not empty
    check(backend, ("n", n, W, H), masks, r)


def test_the_bytes_are_optional_and_two_runs_agree(backend):
    masks = masks_of(130, 70)
    want, want_bits = statement(("shape", 130, 70), masks, 24)
    a, none = run(backend, masks, 24, want_bytes=False)
    b, _ = run(backend, masks, 24)
    assert none is None
    np.testing.assert_array_equal(a, want_bits)
    np.testing.assert_array_equal(a, b)


def test_no_masks_does_nothing(backend):
    lib = backend.lib
    assert lib.gs2m_mask_dilate_disk_scratch_bytes(0, 10, 10) == 0
    assert lib.gs2m_mask_dilate_disk(0, 10, 10, None, 3, None, None, None, 0, C.c_void_p(0)) == 0


def test_bad_arguments_are_refused_with_a_message(backend):
    lib = backend.lib
    W, H, n = 65, 5, 2
    masks = masks_of(W, H)[:n]
    dm = backend.dev(masks)
    ptrs = (C.c_void_p * n)(*[addr(dm) + i * H * W for i in range(n)])
    null_entry = (C.c_void_p * n)(addr(dm), None)
    need = lib.gs2m_mask_dilate_disk_scratch_bytes(n, W, H)
    scratch = backend.dev(np.zeros(need // 8 + 2, np.int64))
    bits = backend.dev(np.full(n * H * 2, 7, np.int64))
    st = C.c_void_p(0)

    def call(nn=n, w=W, h=H, p=ptrs, r=3, ob=_ptr(bits), sc=_ptr(scratch), nbytes=need):
        return lib.gs2m_mask_dilate_disk(nn, w, h, p, r, ob, None, sc, nbytes, st)

    misaligned = C.c_void_p(addr(scratch) + 4)
    for bad, word in ((dict(r=65), "radius = 65"), (dict(r=-1), "radius = -1"), (dict(nn=-1), "n = -1"), (dict(w=0), "n = 2 masks of 0 x 5"),
                      (dict(h=0), "65 x 0"), (dict(p=null_entry), "mask 1 is NULL"), (dict(p=None), "NULL masks"),
                      (dict(ob=None), "NULL masks or out_bits"), (dict(nbytes=need - 1), "scratch"), (dict(sc=None), "scratch"),
                      (dict(sc=misaligned), "8-byte aligned")):
        assert call(**bad) == 1, bad
        assert word in lib.gs2m_last_error().decode(), (bad, lib.gs2m_last_error())
    assert lib.gs2m_mask_dilate_disk_scratch_bytes(-1, W, H) == -1 and lib.gs2m_mask_dilate_disk_scratch_bytes(1, 0, H) == -1
    backend.sync()
    assert np.all(backend.host(bits) == 7)                           # a refused call writes nothing
    assert call() == 0
    backend.sync()
    np.testing.assert_array_equal(np.ascontiguousarray(backend.host(bits)).view(np.uint64).reshape(n, H, 2),
                                  statement(("bad", W, H), masks, 3)[1])


def test_dilate_masks_returns_bits_and_bytes(backend):
    masks = masks_of(130, 70)
    want, want_bits = statement(("shape", 130, 70), masks, 7)
    bits, out = evaluation.dilate_masks(backend.dev(masks), 7, want_bytes=True, lib=backend.lib)
    backend.sync()
    host = lambda t: t.detach().cpu().numpy()
    np.testing.assert_array_equal(host(bits).view(np.uint64), want_bits)
    np.testing.assert_array_equal(host(out), want.astype(np.uint8))
    only = evaluation.dilate_masks([m for m in masks], 7, lib=backend.lib)          # a sequence of host arrays
    backend.sync()
    np.testing.assert_array_equal(host(only).view(np.uint64), want_bits)
    with pytest.raises(RuntimeError, match="radius = 65"):
        evaluation.dilate_masks(backend.dev(masks), 65, lib=backend.lib)
