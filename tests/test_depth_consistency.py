"""gs2m_depth_consistency against the numpy statement of its vote (tests/consistency_statement.py), bit for bit for keep and
the three counts: the ring scene, odd sizes and source tables, every decision at its edge, non-finite and masked input, the
thresholds, the refused arguments and determinism.  Emulator build (CPU) and the HIP library (-m gpu)."""
import ctypes as C
import functools

import numpy as np
import pytest

import consistency_statement as cs
from gs2mesh_amd import _lib
from gs2mesh_amd.depth_utils import ConsistencyParams, consistency_votes, depth_consistency

NAMES = ("keep", "support", "violation", "occluded")
FILL = 0xAB                                     # what an output holds before the call: a pixel still FILL was not written
ID = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def call(backend, depths, intr, sources, pair, rel_tol=0.01, min_depth=0.0, max_depth=100.0, min_support=2, max_violation=1,
         masks=None, outputs=None, null_depth=None):
    """the C entry point itself.  ``outputs``: name -> None (NULL array) or a list of bools (False = NULL entry); default: all.
    Returns (rc, name -> list of host arrays / None)."""
    n = len(depths)
    mem = _lib.MEMORY
    outputs = {name: [True] * n for name in NAMES} if outputs is None else outputs
    sources = np.ascontiguousarray(np.asarray(sources, np.int32).reshape(n, -1)) if n else np.zeros((0, 0), np.int32)
    K = sources.shape[1] if np.ndim(sources) == 2 else 0
    pair = np.ascontiguousarray(np.asarray(pair, np.float32).reshape(n, K, 12)) if n else np.zeros((0, 0, 12), np.float32)
    views = (_lib.DepthView * max(n, 1))()
    held = []
    for i in range(n):
        d = backend.dev(np.asarray(depths[i], np.float32))
        m = backend.dev(np.asarray(masks[i], np.uint8)) if masks is not None and masks[i] is not None else None
        held += [d, m]
        H, W = depths[i].shape
        views[i] = _lib.DepthView(None if null_depth == i else mem.ptr(d), mem.ptr(m), W, H, *[float(v) for v in intr[i]])
    bufs, arrays = {}, {}
    for name in NAMES:
        want = outputs.get(name)
        if want is None:
            bufs[name], arrays[name] = None, None
            continue
        bufs[name] = [backend.dev(np.full(depths[i].shape, FILL, np.uint8)) if want[i] else None for i in range(n)]
        arrays[name] = (C.c_void_p * max(n, 1))(*[mem.ptr(b) for b in bufs[name]])
    rc = backend.lib.gs2m_depth_consistency(
        n, views, K, sources.ctypes.data_as(C.POINTER(C.c_int32)), pair.ctypes.data_as(C.POINTER(C.c_float)), rel_tol, min_depth,
        max_depth, min_support, max_violation, arrays["keep"], arrays["support"], arrays["violation"], arrays["occluded"],
        mem.current_stream(0))
    backend.sync()
    return rc, {name: None if b is None else [backend.host(x) for x in b] for name, b in bufs.items()}


def assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.01, min_depth=0.0, max_depth=100.0, min_support=2,
                            max_violation=1, masks=None, ref=None):
    ref = ref or cs.consistency(depths, intr, sources, pair, rel_tol, min_depth, max_depth, min_support, max_violation, masks)
    for name, want in zip(NAMES, ref):
        if got[name] is None:
            continue
        for i, w in enumerate(want):
            if got[name][i] is not None:
                assert got[name][i].dtype == np.uint8 and np.array_equal(got[name][i], w), (name, i)
    return ref


@functools.lru_cache(maxsize=None)
def ring():
    s = cs.ring_scene()
    g = cs.RING
    s["votes"] = cs.votes(s["depths"], s["intrinsics"], s["sources"], s["pair"], g["rel_tol"], g["min_depth"], g["max_depth"])
    return s


def ring_ref(min_support, max_violation):
    valid, sup, vio, occ = ring()["votes"]
    return cs.keep_maps(valid, sup, vio, min_support, max_violation), sup, vio, occ


# ---- 1. the ring scene ----------------------------------------------------------------------------------------------------------
def test_ring_scene(backend):
    s = ring()
    rc, got = call(backend, s["depths"], s["intrinsics"], s["sources"], s["pair"])
    assert rc == 0
    keep, sup, vio, occ = assert_equals_statement(got, None, None, None, None, ref=ring_ref(2, 1))
    # the scene exercises every outcome
    assert sum(int(k.sum()) for k in keep) > 20000 and all(sum(int((c > 0).sum()) for c in cnt) > 500 for cnt in (sup, vio, occ))
    # the wrappers: the explicit table, and select_sources' own (the same views in another order: the same counts)
    dev = [backend.dev(d) for d in s["depths"]]
    out = consistency_votes(dev, s["intrinsics"], s["sources"], s["pair"], 0.01, 2, 1, max_depth=100.0, want=NAMES,
                            lib=backend.lib)
    backend.sync()
    for name, want in zip(NAMES, (keep, sup, vio, occ)):
        assert all(np.array_equal(backend.host(a), w) for a, w in zip(out[name], want)), name
    high = depth_consistency(dev, s["intrinsics"][0], s["camera_to_world"], ConsistencyParams(), max_depth=100.0,
                             want_counts=True, lib=backend.lib)
    backend.sync()
    for name, a, want in zip(NAMES, high, (keep, sup, vio, occ)):
        assert all(np.array_equal(backend.host(x), w) for x, w in zip(a, want)), name
    only_keep = depth_consistency(dev, s["intrinsics"], s["camera_to_world"], dict(sources=s["sources"]), max_depth=100.0,
                                  lib=backend.lib)
    backend.sync()
    assert all(np.array_equal(backend.host(x), w) for x, w in zip(only_keep, keep))


# ---- 2. sizes and tables --------------------------------------------------------------------------------------------------------
def random_scene(rng, sizes, K, minus_one=0.0):
    """views of the given (W, H) looking roughly the same way from nearby, depths in [1.5, 3] with holes; every view has
    its own intrinsics.  Sources are random other views, -1 with probability ``minus_one``."""
    n = len(sizes)
    depths, intr = [], []
    for W, H in sizes:
        d = rng.uniform(1.5, 3.0, (H, W)).astype(np.float32)
        d[rng.random((H, W)) < 0.1] = 0.0
        depths.append(d)
        intr.append((W * rng.uniform(0.9, 1.3), H * rng.uniform(0.9, 1.3) + 1.0, W / 2.0 + rng.uniform(-0.5, 0.5),
                     H / 2.0 + rng.uniform(-0.5, 0.5)))
    sources = np.full((n, K), -1, np.int32)
    pair = np.zeros((n, K, 12), np.float32)
    for i in range(n):
        for k in range(K):
            if n > 1 and rng.random() >= minus_one:
                sources[i, k] = rng.choice([j for j in range(n) if j != i])
            a = rng.normal(0.0, 0.05, 3)                                     # a small rotation, a small step
            Rm = np.eye(3) + np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            pair[i, k] = np.concatenate([Rm, rng.normal(0.0, 0.1, (3, 1))], axis=1).reshape(12).astype(np.float32)
    return depths, intr, sources, pair


SIZES = [(1, 1), (17, 9), (70, 33)]


@pytest.mark.parametrize("n_views", [1, 2, _lib.CONSISTENCY_BATCH + 1])
@pytest.mark.parametrize("K", [0, 1, 16])
def test_sizes_and_tables(backend, n_views, K):
    rng = np.random.default_rng(100 * n_views + K)
    sizes = [SIZES[(i + n_views) % 3] for i in range(n_views)]
    depths, intr, sources, pair = random_scene(rng, sizes, K, minus_one=0.2)
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.2, min_support=1)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.2, min_support=1)
    if K == 0 or n_views == 1:                   # no source at all: nothing is supported, so min_support 1 keeps nothing
        assert all(not k.any() for k in got["keep"]) and all(not c.any() for c in got["support"])


def test_three_sizes_in_one_call_and_minus_one_anywhere(backend):
    rng = np.random.default_rng(11)
    depths, intr, sources, pair = random_scene(rng, SIZES + [(33, 70), (16, 16)], 5)
    sources[0, 0] = -1                                                      # at the start,
    sources[1, 2] = -1                                                      # in the middle
    sources[2, 4] = -1                                                      # and at the end of a row,
    sources[3] = -1                                                         # a whole row,
    sources[4] = [-1, 2, -1, 2, -1]                                         # and one source twice, under one transform
    pair[4, 3] = pair[4, 1]
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.2, min_support=1)
    assert rc == 0
    _, sup, vio, occ = assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.2, min_support=1)
    assert sum(int(c.sum()) for c in sup) > 100 and sum(int(c.sum()) for c in vio) > 100 and sum(int(c.sum()) for c in occ) > 100
    assert not got["support"][3].any() and not got["keep"][3].any()
    assert not (got["support"][4] % 2).any()                                # the doubled source votes twice


def test_null_output_arrays_and_entries(backend):
    rng = np.random.default_rng(12)
    depths, intr, sources, pair = random_scene(rng, [(70, 33), (17, 9), (70, 33), (1, 1), (17, 9)], 3)
    outputs = dict(keep=[True, False, True, False, False], support=None, violation=[False, False, True, False, True],
                   occluded=[False] * 5)                                    # view 1 and view 3 ask for nothing at all
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.2, min_support=1, outputs=outputs)
    assert rc == 0 and got["support"] is None
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.2, min_support=1)
    for name in ("keep", "violation"):
        assert [x is not None for x in got[name]] == outputs[name]
    rc, got = call(backend, depths, intr, sources, pair, outputs=dict(keep=None, support=None, violation=None, occluded=None))
    assert rc == 0


# ---- 3. decisions at their edges ------------------------------------------------------------------------------------------------
def edge_views(src_row):
    """two 4 x 1 views with fx = fy = 1, cx = cy = 0: pixel u of the reference at depth 2 is the point (2 u, 0, 2)"""
    ref = np.full((1, 4), 2.0, np.float32)
    return [ref, np.asarray(src_row, np.float32).reshape(1, 4)], [(1.0, 1.0, 0.0, 0.0)] * 2


def test_vote_classes_at_their_edges(backend):
    f = np.float32
    row = [f(2.5), np.nextafter(f(2.5), f(3)), f(1.5), np.nextafter(f(1.5), f(1))]
    depths, intr = edge_views(row)
    sources, pair = [[1], [-1]], np.stack([ID, ID]).reshape(2, 1, 12)
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.25, min_support=1, max_violation=0)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.25, min_support=1, max_violation=0)
    assert got["support"][0].tolist() == [[1, 0, 1, 0]]                     # |diff| == tol on both sides is support
    assert got["violation"][0].tolist() == [[0, 1, 0, 0]]                   # one ulp past it: the source sees past the point
    assert got["occluded"][0].tolist() == [[0, 0, 0, 1]]                    # one ulp short of it: something in front
    assert got["keep"][0].tolist() == [[1, 0, 1, 0]]


@pytest.mark.parametrize("shift,expect", [(-1.0, [1, 1, 1, 1]), (1.0, [1, 1, 1, 0]), (-1.0000001, [0, 1, 1, 1])])
def test_image_bounds_are_half_open(backend, shift, expect):
    """pu = u + shift / 2 + 0.5: a half-pixel translation puts pixel 0 at pu = 0 exactly (inside) and pixel 3 at pu = W_j
    exactly (outside); one ulp further left pixel 0 is outside too"""
    depths, intr = edge_views([2.0] * 4)
    M = ID.copy()
    M[3] = shift
    sources, pair = [[1], [-1]], np.stack([M, ID]).reshape(2, 1, 12)
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.25, min_support=1)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.25, min_support=1)
    assert got["support"][0].tolist() == [expect]
    # the same along v: 1 x 4 views
    depths = [d.T.copy() for d in depths]
    M = ID.copy()
    M[7] = shift
    pair = np.stack([M, ID]).reshape(2, 1, 12)
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.25, min_support=1)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.25, min_support=1)
    assert got["support"][0].T.tolist() == [expect]


@pytest.mark.parametrize("row2", [[0, 0, 1, -2], [0, 0, 1, -3], [0, 0, -1, 0], [0, 0, 0, 0]])
def test_points_not_in_front_of_the_source_do_not_vote(backend, row2):
    depths, intr = edge_views([2.0] * 4)
    M = ID.copy()
    M[8:] = row2                                                            # q_2 = 0, -1, -2, 0
    sources, pair = [[1], [-1]], np.stack([M, ID]).reshape(2, 1, 12)
    rc, got = call(backend, depths, intr, sources, pair, rel_tol=0.25, min_support=0)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, rel_tol=0.25, min_support=0)
    assert not any(got[name][0].any() for name in ("support", "violation", "occluded"))
    assert got["keep"][0].all()                                             # min_support 0: valid and nothing against it


def test_identity_pair_on_a_copy_supports_every_valid_pixel(backend):
    s = ring()
    d = s["depths"][3]
    depths, intr = [d, d.copy()], s["intrinsics"][:2]
    sources, pair = [[1], [0]], np.stack([ID, ID]).reshape(2, 1, 12)
    rc, got = call(backend, depths, intr, sources, pair, min_support=1, max_violation=0)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, min_support=1, max_violation=0)
    valid = (d > 0).astype(np.uint8)
    assert valid.sum() > 1000
    for i in range(2):
        assert np.array_equal(got["support"][i], valid) and np.array_equal(got["keep"][i], valid)
        assert not got["violation"][i].any() and not got["occluded"][i].any()


# ---- 4. non-finite and invalid input --------------------------------------------------------------------------------------------
VALUES = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 0.25, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, 1.0,
                   1.004, 2.0, 1e30], np.float32)


def grid_views():
    """reference pixel (y, x) holds VALUES[x], the source's (y, x) holds VALUES[y], and the identity pair sends a pixel to
    itself: every value meets every value"""
    n = len(VALUES)
    ref = np.tile(VALUES[None, :], (n, 1))
    src = np.tile(VALUES[:, None], (1, n))
    intr = [(20.0, 20.0, n / 2.0, n / 2.0)] * 2
    return [ref, src], intr, [[1], [0]], np.stack([ID, ID]).reshape(2, 1, 12)


@pytest.mark.parametrize("max_depth", [np.inf, 1.5])
def test_non_finite_and_out_of_range_depths(backend, max_depth):
    depths, intr, sources, pair = grid_views()
    kw = dict(rel_tol=0.01, min_depth=0.5, max_depth=max_depth, min_support=1, max_violation=0)
    rc, got = call(backend, depths, intr, sources, pair, **kw)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, **kw)
    ok = np.array([v > 0 and v >= 0.5 and v < max_depth for v in VALUES])   # NaN compares false
    assert ok.sum() == (5 if max_depth == np.inf else 3)
    votes = got["support"][0].astype(int) + got["violation"][0] + got["occluded"][0]
    assert np.array_equal(votes, (ok[None, :] & ok[:, None]).astype(int))   # a vote needs both ends valid
    assert not got["keep"][0][:, ~ok].any() and not got["keep"][0][~ok, :].any()
    i1, i2 = list(VALUES).index(1.0), list(VALUES).index(np.float32(1.004))
    assert got["support"][0][i1, i2] == 1 and got["support"][0][i2, i1] == 1 and got["keep"][0][i1, i1] == 1
    if max_depth == np.inf:
        big = len(VALUES) - 1
        assert got["violation"][0][big, i1] == 1 and got["occluded"][0][i1, big] == 1


def test_masks(backend):
    s = ring()
    rng = np.random.default_rng(5)
    n = 5
    depths, intr = s["depths"][:n], s["intrinsics"][:n]
    sources = np.array([[(i - 1) % n, (i + 1) % n, (i + 2) % n] for i in range(n)], np.int32)
    sources[0, 0] = -1                                                      # 0 and 4 are no neighbours on the ring of 12
    sources[n - 1, 1:] = -1
    sources[n - 2, 2] = -1
    from gs2mesh_amd.depth_utils import pair_matrices
    pair = pair_matrices(s["camera_to_world"][:n], sources)
    masks = [(rng.random(d.shape) < 0.7).astype(np.uint8) * rng.integers(1, 255, d.shape).astype(np.uint8) for d in depths]
    masks[2] = None
    rc, got = call(backend, depths, intr, sources, pair, min_support=1, masks=masks)
    assert rc == 0
    assert_equals_statement(got, depths, intr, sources, pair, min_support=1, masks=masks)
    dead = masks[1] == 0
    for name in NAMES:                                                      # a masked reference pixel: keep 0, zero counts
        assert not got[name][1][dead].any()
    # a masked source pixel does not vote: masking view 1 alone can only lower the counts view 2 gets from it
    rc, free = call(backend, depths, intr, sources, pair, min_support=1, masks=[None] * n)
    assert rc == 0
    only1 = [None, masks[1], None, None, None]
    rc, part = call(backend, depths, intr, sources, pair, min_support=1, masks=only1)
    assert rc == 0
    assert_equals_statement(part, depths, intr, sources, pair, min_support=1, masks=only1)
    total = lambda g, i: g["support"][i].astype(int) + g["violation"][i] + g["occluded"][i]
    assert (total(part, 2) <= total(free, 2)).all() and (total(part, 2) < total(free, 2)).sum() > 100
    assert np.array_equal(total(part, 3), total(free, 3))                   # view 3 does not look at view 1


# ---- 5. thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_support,max_violation", [(0, 4), (4, 4), (2, 0), (0, 0), (4, 0)])
def test_thresholds(backend, min_support, max_violation):
    s = ring()
    rc, got = call(backend, s["depths"], s["intrinsics"], s["sources"], s["pair"], min_support=min_support,
                   max_violation=max_violation, outputs=dict(keep=[True] * 12))
    assert rc == 0
    keep, *_ = assert_equals_statement(got, None, None, None, None, ref=ring_ref(min_support, max_violation))
    valid = ring()["votes"][0]
    if (min_support, max_violation) == (0, 4):                              # nothing can fail: keep is `valid`
        assert all(np.array_equal(k, v.astype(np.uint8)) for k, v in zip(got["keep"], valid))
    else:
        assert all(0 < int(k.sum()) < int(v.sum()) for k, v in zip(keep, valid))


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def small_scene():
    return random_scene(np.random.default_rng(1), [(17, 9), (17, 9), (17, 9)], 2)


def refused(backend, rc, got, *words):
    assert rc == 1
    msg = backend.lib.gs2m_last_error().decode()
    assert msg.startswith("gs2m_depth_consistency") and all(w in msg for w in words), msg
    for bufs in got.values():
        assert all((b == FILL).all() for b in bufs)                         # nothing was written


def test_errors(backend):
    depths, intr, sources, pair = small_scene()
    bad = sources.copy()
    bad[2, 1] = 2
    refused(backend, *call(backend, depths, intr, bad, pair), "sources[2][1] = 2")           # a view as its own source
    bad[2, 1] = 3
    refused(backend, *call(backend, depths, intr, bad, pair), "sources[2][1] = 3")           # past the last view
    bad[2, 1] = -2
    refused(backend, *call(backend, depths, intr, bad, pair), "sources[2][1] = -2")
    refused(backend, *call(backend, depths, intr, np.full((3, 17), -1), np.zeros((3, 17, 12))), "max_sources = 17")
    for tol in (0.0, 1.0, -0.5, float("nan")):
        refused(backend, *call(backend, depths, intr, sources, pair, rel_tol=tol), "rel_tol")
    refused(backend, *call(backend, depths, intr, sources, pair, null_depth=1), "view 1", "NULL depth")
    # a view of non-positive size (the descriptor says so; the buffers are what they were)
    mem = _lib.MEMORY
    d = backend.dev(depths[0])
    out = backend.dev(np.full(depths[0].shape, FILL, np.uint8))
    for W, H in ((0, 9), (17, 0), (-1, 9), (65537, 9)):
        views = (_lib.DepthView * 1)(_lib.DepthView(mem.ptr(d), None, W, H, 1.0, 1.0, 0.0, 0.0))
        rc = backend.lib.gs2m_depth_consistency(1, views, 0, None, None, 0.01, 0.0, 1.0, 0, 0, (C.c_void_p * 1)(mem.ptr(out)),
                                                None, None, None, mem.current_stream(0))
        backend.sync()
        assert rc == 1 and f"{W} x {H}" in backend.lib.gs2m_last_error().decode()
        assert (backend.host(out) == FILL).all()
    # the wrapper raises with the library's message
    with pytest.raises(RuntimeError, match="rel_tol"):
        consistency_votes([backend.dev(x) for x in depths], intr, sources, pair, 1.5, 2, 1, lib=backend.lib)


def test_no_views_is_not_an_error(backend):
    rc, _ = call(backend, [], [], [], [])
    assert rc == 0
    assert depth_consistency([], [], np.zeros((0, 4, 4)), lib=backend.lib) == []


@pytest.mark.gpu
def test_host_inputs_on_an_explicit_stream():
    """host arrays are uploaded on torch's current stream and the kernels run on the caller's: the wrapper orders the two and
    keeps its temporaries until the kernels have run"""
    import torch
    from backends import make
    backend = make("gpu")
    s = ring()
    side = torch.cuda.Stream()
    masks = [(d > 0).astype(np.float32) * 2.0 for d in s["depths"]]            # converted on the device before the call
    out = consistency_votes(s["depths"], s["intrinsics"], s["sources"], s["pair"], 0.01, 2, 1, masks=masks, max_depth=100.0,
                            want=NAMES, lib=backend.lib, stream=side.cuda_stream)
    junk = [torch.full((64, 96), 7.0, device="cuda") for _ in range(48)]     # what would reuse temporaries freed too early
    side.synchronize()
    for name, want in zip(NAMES, ring_ref(2, 1)):
        assert all(np.array_equal(backend.host(a), w) for a, w in zip(out[name], want)), name
    del junk


# ---- 7. determinism -------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(backend):
    s = ring()
    _, a = call(backend, s["depths"], s["intrinsics"], s["sources"], s["pair"])
    _, b = call(backend, s["depths"], s["intrinsics"], s["sources"], s["pair"])
    for name in NAMES:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[name], b[name])), name
