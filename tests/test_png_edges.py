"""The device PNG encoder (gs2mesh_amd/csrc/png_encode.hip) at the boundaries of its own code: the scan rounds of
k_png_assemble (more than 256 segments), the chunk counts at which k_png_crc_finish changes shape (255 / 256 / 257 / > 512 and
IDAT lengths at exact 16 KiB multiples), the 7-bit limit of the code-length code, every branch of the tree header's run-length
coder, the smallest and the fullest literal code, segment lengths at the 4096-byte round of k_png_encode with segment starts at
every address residue, stored segments at the 65535-byte block limit, misaligned output through the C ABI, and handle reuse.

Both back-ends run every case: "emu" is the kernel source compiled against the CPU fiber emulator (test_png_encode.emu_lib),
"gpu" the product library on an MI355X.  Every case goes through ``check``: PIL, the chunk CRCs and ``zlib.decompress``
(test_png_encode.check_file), the structure of the stream (png_stream.check_stream), on the GPU byte equality with the
emulator's file, and a second encode that must repeat the first.  Every comparison is exact.  Each test asserts on the reader's
report that its input sits where it claims (token list, code lengths, block kinds and lengths, segment count, chunk count)
before the pass is trusted.

Not pinned here: the dynamic-versus-stored choice at equal size (``dyn_bytes < stored``).  That needs a second implementation
of the exact size computation; ``check_stream`` asserts the implication that can be seen from outside (a dynamic segment is
strictly smaller than its stored form)."""
import contextlib
import ctypes as C
import hashlib

import numpy as np
import pytest

from png_stream import StreamError, check_stream, inflate, inflate_zlib
from test_png_encode import _huffman_max_depth, check_file, content, emu_lib, filtered_scanlines, parse_png

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
CRC_CHUNK = 16384


# ---- back-ends ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _memory(name):
    from gs2mesh_amd import _lib
    from backends import HostMemory
    old = _lib.MEMORY
    _lib.MEMORY = HostMemory() if name == "emu" else _lib.DeviceMemory()
    try:
        yield
    finally:
        _lib.MEMORY = old


def make_encoder(name, S, filt):
    from gs2mesh_amd.png import PngEncoder
    if name == "emu":
        return PngEncoder(0, lib=emu_lib(), rows_per_segment=S, filter=filt)
    return PngEncoder(0, rows_per_segment=S, filter=filt)


def run(name, enc, img):
    """the files of ``img`` ([H,W,3] or [n,H,W,3] u8 numpy) from encoder ``enc`` of back-end ``name``"""
    with _memory(name):
        if name == "emu":
            return enc.encode(img)
        import torch
        return enc.encode(torch.from_numpy(img).cuda())


_EMU_FILES = {}     # the emulator's file of an input, made once and shared by the two back-ends' tests


def _key(img, S, filt):
    return hashlib.sha1(img.tobytes()).hexdigest(), img.shape, S, filt


def emu_file(img, S, filt):
    """the emulator's file from a FRESH handle"""
    k = _key(img, S, filt)
    if k not in _EMU_FILES:
        enc = make_encoder("emu", S, filt)
        try:
            _EMU_FILES[k] = run("emu", enc, img)[0]
        finally:
            enc.close()
    return _EMU_FILES[k]


def same_bytes(got, want, what):
    if got != want:     # not `assert got == want`: the difference of two 8 MB strings is not worth rendering
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}")


def verify(name, data, img, S, filt):
    """one file against everything that can be known about it from outside; returns check_stream's segment reports"""
    H, W, _ = img.shape
    check_file(data, img, filt)
    segs = check_stream(parse_png(data)[2], W, H, S, filt, filtered_scanlines(img, filt))
    if name == "gpu":
        same_bytes(data, emu_file(img, S, filt), "GPU file against the emulator's")
    return segs


def check(name, img, S, filt):
    enc = make_encoder(name, S, filt)
    try:
        data = run(name, enc, img)[0]
        again = run(name, enc, img)[0]
    finally:
        enc.close()
    if name == "emu":
        _EMU_FILES.setdefault(_key(img, S, filt), data)
    segs = verify(name, data, img, S, filt)
    same_bytes(again, data, "second encode of the same input")
    return data, segs


def crc_chunks(data):
    """number of 16 KiB chunks that the CRC kernels cut "IDAT" + payload into"""
    return -(-(len(parse_png(data)[2]) + 4) // CRC_CHUNK)


def kinds(segs):
    return [s["kind"] for s in segs]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make(kind, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W])
    if kind == "noise128":          # uniform over 128 values: about 7 bits per byte, so Huffman coding pays
        return rng.integers(0, 128, (H, W, 3), dtype=np.uint8)
    if kind == "alternating":       # even rows noise, odd rows one value: stored and dynamic one-row segments interleave
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[1::2] = rng.integers(0, 256, (H, 1, 1), dtype=np.uint8)[1::2]
        return img
    return content(kind, H, W, seed)


def image_of_counts(counts, W, H, seed):
    """[H,W,3] image whose filter-0 scanlines hold byte v exactly counts[v] times (H of the zeros are the filter bytes)"""
    counts = list(counts)
    assert counts[0] >= H and sum(counts) == H * (3 * W + 1), (counts[0], sum(counts))
    counts[0] -= H
    flat = np.repeat(np.arange(256, dtype=np.uint8), counts)
    img = np.random.default_rng(seed).permutation(flat).reshape(H, W, 3)
    assert np.bincount(np.frombuffer(filtered_scanlines(img, 0), np.uint8), minlength=256).tolist()[0] == counts[0] + H
    return img


# ---- the reader itself ---------------------------------------------------------------------------------------------------
def _zlib_streams(raw):
    import zlib
    yield "level 0", zlib.compress(raw, 0)
    yield "level 1", zlib.compress(raw, 1)
    yield "level 9", zlib.compress(raw, 9)
    for name, strategy in (("huffman only", zlib.Z_HUFFMAN_ONLY), ("fixed", zlib.Z_FIXED)):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
        yield name, c.compress(raw) + c.flush()


def test_reader_decodes_what_zlib_decodes():
    """The reader on streams that are not ours: stored, fixed and dynamic blocks, with matches (overlapping ones in the
    flat Paeth residuals of the gradient) and without, from zlib itself."""
    import zlib
    seen = set()
    for kind, W, H, filt in (("blobs", 97, 61, 4), ("gradient", 64, 40, 4), ("noise128", 33, 20, 0)):
        raw = filtered_scanlines(make(kind, H, W, seed=1), filt)
        for name, stream in _zlib_streams(raw):
            blocks = inflate_zlib(stream)
            assert b"".join(b.data for b in blocks) == zlib.decompress(stream) == raw, (kind, name)
            assert blocks[-1].bfinal and not any(b.bfinal for b in blocks[:-1])
            assert blocks[0].start == 0 and all(a.end == b.start for a, b in zip(blocks, blocks[1:]))
            seen |= {(b.btype, b.n_matches > 0) for b in blocks}
    assert {(0, False), (1, True), (1, False), (2, True), (2, False)} <= seen


def _bits(*fields):
    """LSB-first packing of (value, width) fields, padded to the byte"""
    acc = n = 0
    for v, w in fields:
        acc |= v << n
        n += w
    return acc.to_bytes((n + 7) // 8, "little")


def _dynamic_header(cl_lens, codes, hlit=257):
    """BFINAL 1, dynamic, HLIT, HDIST 1, all 19 code-length lengths, then ``codes``: (code, width) already bit-reversed"""
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    return _bits((1, 1), (2, 2), (hlit - 257, 5), (0, 5), (15, 4), *[(cl_lens.get(s, 0), 3) for s in order], *codes)


def test_reader_rejects_malformed_streams():
    good = _bits((1, 1), (0, 2)) + b"\x02\x00\xfd\xffab"
    assert inflate(good)[0].data == b"ab"
    cases = {
        "LEN": _bits((1, 1), (0, 2)) + b"\x02\x00\xfc\xffab",
        "left over": good + b"\x00",
        "block type 3": _bits((1, 1), (3, 2)),
        "end of input": good[:-1],
        "over-subscribed": _dynamic_header({0: 1, 1: 1, 2: 1}, []),
        "incomplete": _dynamic_header({0: 1, 1: 2}, []),
        # code-length code {1: '0', 16: '10', 18: '11'}: a repeat before any length
        "no previous length": _dynamic_header({1: 1, 16: 2, 18: 2}, [(0b01, 2), (0, 2)]),
        # 18(+127), 18(+127) = 276 zeros > 258
        "run past": _dynamic_header({1: 1, 16: 2, 18: 2}, [(0b11, 2), (127, 7), (0b11, 2), (127, 7)]),
        # fixed block: literal/length symbol 286 is the 8-bit code 11000110, sent MSB first
        "undefined literal/length code 286": _bits((1, 1), (1, 2), (0b01100011, 8)),
        # fixed block: length symbol 257 (0000001), then distance 1 with nothing before it
        "before the start": _bits((1, 1), (1, 2), (0b1000000, 7), (0, 5)),
    }
    for text, stream in cases.items():
        with pytest.raises(StreamError, match=text):
            inflate(stream)
    # HLIT 258: lengths 256 -> 1, 257 -> 1, every other and the one distance code 0; code-length code {0: '0', 1: '10',
    # 18: '11'}; tokens 18(+127) 18(+107) (256 zeros), 1, 1, 0; then length symbol 257 ('1'): there is no distance code
    toks = [(0b11, 2), (127, 7), (0b11, 2), (107, 7), (0b01, 2), (0b01, 2), (0, 1), (1, 1)]
    with pytest.raises(StreamError, match="undefined distance code"):
        inflate(_dynamic_header({0: 1, 1: 2, 18: 2}, toks, hlit=258))
    assert inflate(_dynamic_header({0: 1, 1: 2, 18: 2}, toks[:-1] + [(0, 1)], hlit=258))[0].data == b""


# ---- a. the run-length coder of the tree header --------------------------------------------------------------------------
# What k_png_codes emits for a maximal run of n equal lengths (its greedy rule, written out by hand for the n that select
# between the codes): zeros first as 18 (11..138), then 17 (3..10), then single 0s; a non-zero v once, then 16 (3..6), then vs.
ZERO_PIECES = {
    1: [(0, 0)], 2: [(0, 0), (0, 0)], 3: [(17, 0)], 10: [(17, 7)], 11: [(18, 0)], 12: [(18, 1)], 138: [(18, 127)],
    139: [(18, 127), (0, 0)], 140: [(18, 127), (0, 0), (0, 0)], 148: [(18, 127), (17, 7)], 149: [(18, 127), (18, 0)],
    255: [(18, 127), (18, 106)],
}
V = "v"
NONZERO_PIECES = {
    1: [V], 2: [V, V], 3: [V, V, V], 4: [V, (16, 0)], 7: [V, (16, 3)], 8: [V, (16, 3), V], 9: [V, (16, 3), V, V],
    10: [V, (16, 3), (16, 0)],
}


def header_runs(block):
    """[(length value, run length, tokens that code the run)] for the maximal runs of the 258 code lengths of ``block``"""
    lens = block.lit_lens + block.dist_lens
    at, starts = 0, []
    for s, extra in block.tokens:
        starts.append(at)
        at += 1 if s < 16 else (3 if s < 18 else 11) + extra
    assert at == len(lens) == 258
    starts.append(at)
    runs, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        assert i in starts and j in starts, "a token crosses the end of a run"
        runs.append((lens[i], j - i, block.tokens[starts.index(i):starts.index(j)]))
        i = j
    return runs


def check_header_runs(block, pins):
    """every run whose length is in the tables is coded as the tables say; ``pins`` [(zero?, n)] must each occur"""
    seen = set()
    for v, n, toks in header_runs(block):
        want = ZERO_PIECES.get(n) if v == 0 else [(v, 0) if p == V else p for p in NONZERO_PIECES.get(n, [])] or None
        if want is not None:
            assert toks == want, (v, n, toks)
            seen.add((v == 0, n))
    assert set(pins) <= seen, (sorted(set(pins) - seen), [(v, n) for v, n, _ in header_runs(block)])


def layout_image(layout, seed, c=8):
    """A 21 x 8 image (filter 0, 512 stream bytes) whose PRESENT byte values are the 'P' stretches of ``layout``
    [('P' | 'G', n), ...] over the values 0..255: 63 present values.  All but the first (0) and the last occur c = 8 times, the
    last c - 1 = 7 times and 0 (with the 8 filter bytes) 17 times.  With end-of-block (once) that is 64 leaves of weights
    1, 7, 8 x 61, 17: Huffman pairs 1 + 7, then the 62 weights of 8 into 31 of 16, and the 32 nodes 16 x 31, 17 balance: byte
    0 gets 5 bits, the 61 equal values 6 bits each, the last value and end-of-block 7.  So every 'P' stretch between two gaps
    is one run of equal lengths."""
    present, v = [], 0
    for what, n in layout:
        if what == "P":
            present += range(v, v + n)
        v += n
    assert v == 256 and len(present) == 63 and present[0] == 0
    counts = [0] * 256
    for p in present[1:-1]:
        counts[p] = c
    counts[present[-1]] = c - 1
    counts[0] = 8 * 64 - sum(counts)
    return image_of_counts(counts, 21, 8, seed)


P, G = "P", "G"
HEADER_CASES = {
    # gaps 138, 1, 2, 3, 10, 11, 12 and runs of 3, 4, 7, 8, 9, 10 equal non-zero lengths in one header
    "small": ([(P, 1), (G, 138), (P, 3), (G, 1), (P, 4), (G, 2), (P, 7), (G, 3), (P, 8), (G, 10), (P, 9), (G, 11), (P, 10),
               (G, 12), (P, 20), (G, 16), (P, 1)],
              [(True, n) for n in (138, 1, 2, 3, 10, 11, 12)] + [(False, n) for n in (3, 4, 7, 8, 9, 10)]),
    "139": ([(P, 1), (G, 139), (P, 31), (G, 54), (P, 31)], [(True, 139)]),
    "140": ([(P, 1), (G, 140), (P, 31), (G, 53), (P, 31)], [(True, 140)]),
    "148": ([(P, 1), (G, 148), (P, 31), (G, 45), (P, 31)], [(True, 148)]),
    "149": ([(P, 1), (G, 149), (P, 31), (G, 44), (P, 31)], [(True, 149)]),
}


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("case", HEADER_CASES)
def test_tree_header_run_lengths(name, case):
    layout, pins = HEADER_CASES[case]
    img = layout_image(layout, seed=11)
    _, segs = check(name, img, 8, 0)
    assert kinds(segs) == ["dynamic"]
    blk = segs[0]["blocks"][0]
    lens = blk.lit_lens
    assert [l != 0 for l in lens[:256]] == [w == P for w, n in layout for _ in range(n)], "the gaps are where the layout puts them"
    assert lens[0] == 5 and lens[256] == 7 and sorted(set(lens[1:255])) == [0, 6], "layout_image's argument"
    check_header_runs(blk, pins)


# ---- b. the smallest and the fullest code ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
def test_one_literal_and_end_of_block(name):
    """An all-zero image under filter 0: the literal code has two symbols (n == 2 in png_mk_lengths), one bit each, and the
    255 absent literals between them are one gap."""
    img = np.zeros((4, 5, 3), np.uint8)
    _, segs = check(name, img, 4, 0)
    assert kinds(segs) == ["dynamic"]
    blk = segs[0]["blocks"][0]
    assert blk.lit_lens == [1] + [0] * 255 + [1]
    assert blk.tokens == [(1, 0), (18, 127), (18, 106), (1, 0), (0, 0)]
    check_header_runs(blk, [(True, 255)])
    assert (blk.end - blk.start) == 17 + 3 * blk.hclen + sum(blk.cl_lens[s] + (7 if s == 18 else 0) for s, _ in blk.tokens) + 64 + 1


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("filt", [0, 4])
def test_one_pixel(name, filt):
    for px in ((0, 0, 0), (255, 255, 255), (1, 2, 3), (4, 4, 4)):
        img = np.array(px, np.uint8).reshape(1, 1, 3)
        for S in (1, 16):
            _, segs = check(name, img, S, filt)
            assert len(segs) == 1 and segs[0]["L"] == 4


@pytest.mark.parametrize("name", BACKENDS)
def test_all_256_literals_present(name):
    """No zero length in the literal code: the header's only zero is the distance code's.  Equal counts of all 256 values
    cost 8 bits a byte or more and the segment is stored; with half the pixels one value the dynamic form wins."""
    uniform = [12] * 256
    uniform[0] += 4
    _, segs = check(name, image_of_counts(uniform, 256, 4, seed=2), 4, 0)
    assert kinds(segs) == ["stored"]
    big = [192] * 256
    big[0] += 64
    _, segs = check(name, image_of_counts(big, 256, 64, seed=3), 64, 0)
    assert kinds(segs) == ["stored"] and [b.len for b in segs[0]["blocks"]] == [49216]
    skewed = [6] * 256
    skewed[0] += 4
    skewed[7] += 1536
    _, segs = check(name, image_of_counts(skewed, 256, 4, seed=4), 4, 0)
    assert kinds(segs) == ["dynamic"]
    blk = segs[0]["blocks"][0]
    assert min(blk.lit_lens) > 0 and blk.dist_lens == [0]
    assert [t for t in blk.tokens if t[0] in (17, 18)] == [] and blk.tokens[-1] == (0, 0)
    assert sum(1 for t in blk.tokens if t[0] == 0) == 1


# ---- c. the 7-bit limit of the code-length code ---------------------------------------------------------------------------
def dyadic_image(classes, M, W, H, absent, seed):
    """An image (filter 0, one segment of 2^M - 1 bytes) whose literal code is known in advance: ``classes`` {length: number
    of symbols, end-of-block included}, with Kraft sum 1.  A literal of length l occurs 2^(M - l) times, end-of-block once
    (length M), so every probability is a power of two and the Huffman lengths are exactly these.  Byte 0 (which holds the H
    filter bytes) takes the shortest class; the values ``absent`` do not occur; the other values get their classes so that no
    four neighbours share one, which keeps token 16 out of the header.  Returns (image, the 257 expected lengths)."""
    assert sum(n << (M - l) for l, n in classes.items()) == 1 << M and H * (3 * W + 1) == (1 << M) - 1
    left = dict(classes)
    left[M] -= 1                                   # end-of-block
    lens = [0] * 257
    lens[256] = M
    lens[0] = min(classes)
    left[lens[0]] -= 1
    values = [v for v in range(1, 256) if v not in absent]
    assert sum(left.values()) == len(values)
    for v in values:
        free = [l for l in left if left[l]]
        big = max(free, key=lambda l: (left[l], l))
        if left[big] > sum(left.values()) - left[big] + 1 and not lens[v - 1] == lens[v - 2] == big:
            lens[v] = big           # more of this class than gaps between the others: spend the surplus in pairs
        else:
            lens[v] = max(free, key=lambda l: (lens[v - 1] != l, left[l], l))    # the fullest class other than the neighbour's
        left[lens[v]] -= 1
    assert not any(lens[i] and len(set(lens[i:i + 4])) == 1 for i in range(254))
    counts = [(1 << (M - l)) if l else 0 for l in lens[:256]]
    return image_of_counts(counts, W, H, seed), lens


def token_histogram(block):
    h = [0] * 19
    for s, _ in block.tokens:
        h[s] += 1
    return h


SEVEN_BIT_CASES = {
    # the issue's construction: 1023 bytes; tokens {10: 128, 9: 64, 8: 32, 7: 16, 6: 8, 5: 4, 0: 2, 2: 1, 17: 1}
    "depth8": dict(W=10, H=33, M=10, classes={2: 1, 5: 4, 6: 8, 7: 16, 8: 32, 9: 64, 10: 128}, absent=(5, 100, 101, 102),
                   tokens={10: 128, 9: 64, 8: 32, 7: 16, 6: 8, 5: 4, 0: 2, 2: 1, 17: 1}, depth=8),
    # Fibonacci counts of the classes: tokens {0: 1, 18: 1, 11: 2, 5: 3, 4: 5, 12: 8, 10: 13, 8: 21, 9: 34, 7: 55}
    "depth9": dict(W=30, H=45, M=12, classes={4: 5, 5: 3, 7: 55, 8: 21, 9: 34, 10: 13, 11: 2, 12: 8}, absent=range(60, 176),
                   tokens={0: 1, 18: 1, 11: 2, 5: 3, 4: 5, 12: 8, 10: 13, 8: 21, 9: 34, 7: 55}, depth=9),
    # one class more: tokens {0: 1, 18: 1, 6: 2, 5: 3, 4: 5, 12: 8, 7: 13, 9: 21, 11: 34, 10: 55, 8: 89}
    "depth10": dict(W=30, H=45, M=12, classes={4: 5, 5: 3, 6: 2, 7: 13, 8: 89, 9: 21, 10: 55, 11: 34, 12: 8},
                    absent=range(200, 227), tokens={0: 1, 18: 1, 6: 2, 5: 3, 4: 5, 12: 8, 7: 13, 9: 21, 11: 34, 10: 55, 8: 89},
                    depth=10),
}


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("case", SEVEN_BIT_CASES)
def test_code_length_code_is_limited_to_7_bits(name, case):
    """Token histograms whose unlimited Huffman code is 8, 9 and 10 deep; the header can say 7.  The histogram of the header's
    tokens is a chain (each count at least the sum of all smaller ones), as the Fibonacci test of test_png_encode.py is for the
    literals.  Depth 10 is the deepest there is: a Huffman tree d deep weighs at least Fibonacci(d + 2), which is 233 for
    d = 10 and 377 for d = 11, and a header has at most 258 tokens.  That the reader accepts the header proves the limited
    code complete (Kraft sum 1); the decoded lengths prove it is the right one."""
    c = SEVEN_BIT_CASES[case]
    img, lens = dyadic_image(c["classes"], c["M"], c["W"], c["H"], set(c["absent"]), seed=7)
    _, segs = check(name, img, c["H"], 0)
    assert kinds(segs) == ["dynamic"]
    blk = segs[0]["blocks"][0]
    assert blk.lit_lens == lens
    hist = token_histogram(blk)
    assert {s: n for s, n in enumerate(hist) if n} == c["tokens"]
    assert _huffman_max_depth(hist) == c["depth"] > 7
    assert max(blk.cl_lens) == 7 and sum(2.0 ** -l for l in blk.cl_lens if l) == 1.0
    if case == "depth8":
        assert blk.cl_lens == [7, 0, 7, 0, 0, 7, 5, 4, 3, 2, 1, 0, 0, 0, 0, 0, 0, 7, 0]


# ---- d. the 4096-byte round of k_png_encode and the words shared between segments --------------------------------------
ROUND_SHAPES = [(4095, 30, 45), (4096, 341, 4), (4096, 1365, 1), (4097, 80, 17), (8191, 2730, 1), (8192, 341, 8), (8193, 910, 3)]


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("kind,filt", [("gradient", 4), ("noise128", 0)])
def test_segments_at_the_encode_round(name, kind, filt):
    """Dynamic segments of L = 4096 k and one byte either side, three of them and a shorter fourth, so that each has
    neighbours.  Every segment of the stated length L must be dynamic, and every gradient segment.  The one-row last segment
    of the two narrowest noise128 images (W = 30 and 80: 91 and 241 bytes of 7-bit noise) cannot pay for a tree header and is
    stored, which puts a stored neighbour behind a dynamic segment as well."""
    residues = set()
    for L, W, S in ROUND_SHAPES:
        H = 3 * S + 1
        assert S * (3 * W + 1) == L
        _, segs = check(name, make(kind, H, W, seed=L), S, filt)
        assert [s["L"] for s in segs] == [L, L, L, 3 * W + 1]
        assert kinds(segs)[:3] == ["dynamic"] * 3, (L, kinds(segs))
        if kind == "gradient":
            assert kinds(segs)[3] == "dynamic"
        residues |= {s["offset"] % 4 for s in segs if s["kind"] == "dynamic"}
    assert residues == {0, 1, 2, 3}


# ---- e. stored segments at the 65535-byte block -----------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("L,W,S,nseg", [(65534, 72, 302, 1), (65535, 1456, 15, 1), (65536, 341, 64, 1), (65536, 341, 64, 2),
                                        (131070, 1456, 30, 1), (131071, 43690, 1, 1), (131071, 43690, 1, 2)])
def test_stored_segments_at_the_block_limit(name, L, W, S, nseg):
    assert S * (3 * W + 1) == L
    _, segs = check(name, make("noise", nseg * S, W, seed=L), S, 0)
    assert kinds(segs) == ["stored"] * nseg
    want = [65535] * (L // 65535) + ([L % 65535] if L % 65535 else [])
    for s in segs:
        assert [b.len for b in s["blocks"]] == want and s["nbytes"] == L + 5 * len(want)


# ---- f. more segments than one round of k_png_assemble's scan ---------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("H", [255, 256, 257, 513, 1025])
@pytest.mark.parametrize("kind,filt", [("gradient", 4), ("noise", 0), ("alternating", 0)])
def test_segment_counts_around_the_scan_round(name, kind, filt, H):
    _, segs = check(name, make(kind, H, 40, seed=H), 1, filt)
    assert len(segs) == H
    if kind == "gradient":
        assert set(kinds(segs)) == {"dynamic"}
    elif kind == "noise":
        assert set(kinds(segs)) == {"stored"}
    else:
        assert kinds(segs) == ["stored", "dynamic"] * (H // 2) + ["stored"] * (H % 2)


# ---- g. the chunks of the IDAT CRC --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("N,W,H,S", [(16383, 779, 7, 7), (16384, 67, 81, 41), (16385, 165, 33, 33), (32768, 404, 27, 27)])
def test_crc_at_exact_chunk_multiples(name, N, W, H, S):
    """"IDAT" + payload of N = 16 KiB - 1, 16 KiB, 16 KiB + 1 and 32 KiB bytes: the virtual leading padding of the first
    chunk is 1, 0, 16383 and 0 bytes.  N is exact because every segment is stored: N = 12 + H (3 W + 1) + 5 per segment.
    (Narrow images cannot be used for this: at W = 2, 4 or 5 the filter byte is 1/7 to 1/16 of the stream, byte 0 is that
    much more frequent than the rest, and the dynamic form wins: test_crc_of_long_dynamic_segments.)"""
    data, segs = check(name, make("noise", H, W, seed=N), S, 0)
    assert set(kinds(segs)) == {"stored"}
    assert len(parse_png(data)[2]) + 4 == N == 12 + H * (3 * W + 1) + 5 * len(segs)
    assert crc_chunks(data) == -(-N // CRC_CHUNK)


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("W,H", [(2, 2338), (4, 1259), (5, 1023)])
def test_crc_of_long_dynamic_segments(name, W, H):
    """One segment of 16 KiB of narrow noise rows (four rounds of k_png_encode): dynamic, because of the filter bytes."""
    data, segs = check(name, make("noise", H, W, seed=W), H, 0)
    assert kinds(segs) == ["dynamic"] and crc_chunks(data) == 1


@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("H,chunks", [(1016, 255), (1020, 256), (1024, 257)])
def test_crc_chunk_counts_around_256(name, H, chunks):
    """k_png_crc_finish gives each lane one chunk up to 256 chunks and two from 257 (lk = 1, 255 virtual leading chunks)."""
    data, segs = check(name, big_noise(H), 16, 0)
    assert set(kinds(segs)) == {"stored"} and [b.len for b in segs[0]["blocks"]] == [65535, 1]
    assert crc_chunks(data) == chunks


@pytest.mark.parametrize("name", BACKENDS)
def test_crc_of_more_than_512_chunks(name):
    """lk = 2: four chunks per lane."""
    data, segs = check(name, make("noise", 1650, 1700, seed=5), 16, 0)
    assert set(kinds(segs)) == {"stored"}
    assert crc_chunks(data) == 514 > 512


_BIG = {}


def big_noise(H):
    if H not in _BIG:
        _BIG[H] = make("noise", 1024, 1365, seed=9)[:H].copy()
    return _BIG[H]


# ---- h. strides and alignment through the C ABI -----------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
@pytest.mark.parametrize("filt", [0, 4])
def test_misaligned_output_and_strides(name, filt):
    """A batch of three through gs2m_png_encode itself: image_stride with 7 bytes between the images, out_stride and the base
    of ``out`` at every residue mod 4.  k_png_encode stores whole words where it can: nothing outside the files may change."""
    from gs2mesh_amd import _lib
    W, H, S, n, lead = 17, 33, 5, 3, 64
    imgs = np.stack([make(k, H, W, seed=6) for k in ("gradient", "blobs", "noise")])
    istride = 3 * W * H + 7
    packed = np.full(n * istride, 0x55, np.uint8)
    for k in range(n):
        packed[k * istride:k * istride + 3 * W * H] = imgs[k].reshape(-1)
    enc = make_encoder(name, S, filt)
    lib = enc._lib
    bound = enc.max_bytes(W, H)
    if name == "gpu":
        import torch
        src = torch.from_numpy(packed).cuda()
        src_ptr = src.data_ptr()
    else:
        src_ptr = packed.ctypes.data
    found = set()
    try:
        for extra in range(4):
            for off in range(4):
                ostride = bound + extra
                size = lead + off + n * ostride + 64
                if name == "gpu":
                    buf = torch.full((size,), 0xAA, dtype=torch.uint8, device="cuda")
                    nb = torch.zeros(n, dtype=torch.int64, device="cuda")
                    out_ptr, nb_ptr = buf[lead + off:].data_ptr(), nb.data_ptr()
                    assert out_ptr % 4 == off
                    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                else:
                    raw = np.full(size + 4, 0xAA, np.uint8)
                    buf = raw[-raw.ctypes.data % 4:][:size]          # 4-aligned, so that `off` is the residue of the base
                    nb = np.zeros(n, np.int64)
                    out_ptr, nb_ptr = buf.ctypes.data + lead + off, nb.ctypes.data
                    assert out_ptr % 4 == off
                    stream = None
                _lib.check(lib.gs2m_png_encode(enc._h, n, W, H, src_ptr, istride, out_ptr, ostride, nb_ptr, filt, S, stream), lib)
                if name == "gpu":
                    torch.cuda.synchronize()
                    host, sizes = buf.cpu().numpy(), nb.cpu().numpy()
                else:
                    host, sizes = buf, nb
                keep = np.ones(size, bool)
                for k in range(n):
                    at = lead + off + k * ostride
                    assert 65 <= sizes[k] <= bound
                    keep[at:at + sizes[k]] = False
                    data = host[at:at + sizes[k]].tobytes()
                    segs = verify(name, data, imgs[k], S, filt)
                    found |= {((at + s["offset"]) % 4, s["kind"]) for s in segs}
                    same_bytes(data, emu_file(imgs[k], S, filt), f"image {k} at base + {off}, out_stride + {extra}")
                assert (host[keep] == 0xAA).all(), f"bytes outside the files changed (base + {off}, out_stride + {extra})"
    finally:
        enc.close()
    assert {r for r, kind in found if kind == "dynamic"} == {0, 1, 2, 3}


# ---- i. one handle, a large call and then small ones -----------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKENDS)
def test_handle_reuse_after_a_large_call(name):
    """The scratch arena only grows: after the 4 MB call the small ones run in a corner of it, and the large one again."""
    other = make("blobs", 33, 17, seed=8)
    calls = [(big_noise(1024), 16, 0), (make("gradient", 1, 3), 16, 0), (other, 5, 4), (other, 33, 0), (big_noise(1024), 16, 0)]
    enc = make_encoder(name, 16, 0)
    try:
        for i, (img, S, filt) in enumerate(calls):
            enc.rows_per_segment, enc.filter = S, filt
            data = run(name, enc, img)[0]
            verify(name, data, img, S, filt)
            same_bytes(data, emu_file(img, S, filt), f"call {i} on the reused handle against a fresh handle")
    finally:
        enc.close()
