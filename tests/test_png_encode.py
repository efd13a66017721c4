"""Device PNG encoder (gs2mesh_amd/csrc/png_encode.hip) on the CPU emulator: the kernel SOURCE compiled with g++ against
tests/emu/platform.h into a library of its own, driven through ``gs2mesh_amd.png.PngEncoder(lib=...)``.  Every file is checked
by PIL and, independently, by a parse of the stream here: signature, IHDR fields, chunk CRCs against ``zlib.crc32``, IEND, and
``zlib.decompress(IDAT)`` (which checks the Adler-32) against the filtered scanlines computed in numpy."""
import ctypes as C
import heapq
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
OUT = os.path.join(EMU, "_build")
LIB = os.path.join(OUT, "libgs2mesh_png_emu.so")
SRC = os.path.join(ROOT, "gs2mesh_amd", "csrc", "png_encode.hip")

# the product library's error plumbing lives in raster_api.hip; this build needs only these two functions
_ERRORS_CPP = r"""
#include <stdarg.h>
#include <stdio.h>
static thread_local char g_err[1024];
void gs2m_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* gs2m_last_error(void) { return g_err; }
"""


def build_png_emu():
    """tests/emu/_build/libgs2mesh_png_emu.so: png_encode.hip + the fiber emulator (rebuilt when a source is newer)."""
    os.makedirs(OUT, exist_ok=True)
    deps = [SRC, os.path.join(os.path.dirname(SRC), "device_memory.h"), os.path.join(EMU, "platform.h"),
            os.path.join(EMU, "emu_runtime.cpp"), os.path.abspath(__file__), os.path.join(ROOT, "include", "gs2mesh_amd.h")]
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
        return LIB
    err = os.path.join(OUT, "png_emu_errors.cpp")
    with open(err, "w") as f:
        f.write(_ERRORS_CPP)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-Wall", "-Wno-unknown-pragmas",
           "-Wno-unused-function", "-I", EMU, "-I", os.path.join(ROOT, "gs2mesh_amd", "csrc"),
           "-x", "c++", SRC, "-x", "none", os.path.join(EMU, "emu_runtime.cpp"), err, "-o", LIB + ".tmp"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("g++ failed:\n" + r.stdout.decode(errors="replace"))
    os.replace(LIB + ".tmp", LIB)
    return LIB


_EMU_LIB = None


def emu_lib():
    global _EMU_LIB
    if _EMU_LIB is None:
        from gs2mesh_amd import _lib
        _EMU_LIB = _lib.bind(C.CDLL(build_png_emu()), require_all=False)
    return _EMU_LIB


@pytest.fixture
def emu_encoder():
    """factory of PngEncoder(lib=<emulator build>) with the emulator's host-pointer memory policy"""
    from gs2mesh_amd import _lib
    from gs2mesh_amd.png import PngEncoder
    from backends import HostMemory
    old = _lib.MEMORY
    _lib.MEMORY = HostMemory()
    made = []

    def make(rows_per_segment=16, filter=4):
        e = PngEncoder(0, lib=emu_lib(), rows_per_segment=rows_per_segment, filter=filter)
        made.append(e)
        return e
    try:
        yield make
    finally:
        for e in made:
            e.close()
        _lib.MEMORY = old


# ---- reference computations ---------------------------------------------------------------------------------------------
def filtered_scanlines(img, filt):
    """The bytes the zlib stream must hold: per row the filter-type byte, then the filtered 3W bytes (PNG spec 9.2)."""
    H, W, _ = img.shape
    x = img.reshape(H, W * 3).astype(np.int32)
    if filt == 0:
        f = x
    else:
        a = np.zeros_like(x)
        a[:, 3:] = x[:, :-3]
        b = np.zeros_like(x)
        b[1:] = x[:-1]
        c = np.zeros_like(x)
        c[1:, 3:] = x[:-1, :-3]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        f = (x - pred) & 255
    return np.concatenate([np.full((H, 1), filt), f], axis=1).astype(np.uint8).tobytes()


def parse_png(data):
    """(W, H, IDAT payload) after checking the container byte by byte."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        ln, = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        crc, = struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])
        assert len(body) == ln and crc == zlib.crc32(typ + body), typ
        chunks.append((typ, body))
        pos += 12 + ln
    assert pos == len(data)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, inter) == (8, 2, 0, 0, 0)
    assert chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01"
    return W, H, idat


def check_file(data, img, filt):
    from PIL import Image
    H, W, _ = img.shape
    w, h, idat = parse_png(data)
    assert (w, h) == (W, H)
    assert zlib.decompress(idat) == filtered_scanlines(img, filt)
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGB" and im.size == (W, H)
    assert np.array_equal(np.asarray(im), img)


def content(kind, H, W, seed=0):
    rng = np.random.default_rng(seed + 7 * H + W)
    if kind == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(x * 3 + y) % 256, (y * 5) % 256, (x + 2 * y) % 256], -1).astype(np.uint8)
    if kind == "blobs":        # a rendered-looking field: soft Gaussian blobs on a dark background
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        img = np.zeros((H, W, 3))
        for _ in range(12):
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            s = rng.uniform(1.0, max(2.0, 0.3 * max(W, H)))
            img += rng.uniform(0, 1, 3) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))[..., None]
        return np.clip(np.rint(255 * img / max(img.max(), 1e-9)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    raise ValueError(kind)


SHAPES = [(W, H) for W in (1, 2, 3, 17, 1601) for H in (1, 15, 16, 17, 33)]
KINDS = ("zeros", "ones", "gradient", "blobs", "noise")


# ---- tests ---------------------------------------------------------------------------------------------------------------
def test_max_bytes_is_the_stored_bound():
    lib = emu_lib()

    def bound(W, H, S):
        S = min(S, H)
        R = 3 * W + 1
        stored = lambda L: L + 5 * -(-L // 65535)
        return 65 + (H // S) * stored(S * R) + (stored((H % S) * R) if H % S else 0)
    for W, H, S in ((1, 1, 1), (1600, 1200, 16), (1601, 33, 1), (17, 33, 100), (20000, 7, 3)):
        assert lib.gs2m_png_max_bytes(W, H, S) == bound(W, H, S)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 5, 16)):
        assert lib.gs2m_png_max_bytes(*bad) == -1


@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes_and_contents_decode(emu_encoder, W, H):
    encs = {S: emu_encoder(rows_per_segment=S) for S in sorted({1, 16, H})}
    for kind in KINDS:
        img = content(kind, H, W)
        for S, enc in encs.items():
            data = enc.encode(img)[0]
            check_file(data, img, 4)
            bound = enc.max_bytes(W, H)
            assert len(data) <= bound
            if kind == "noise" and W == 1601:
                assert len(data) == bound, "uniform noise must take the stored fallback in every segment"
            if kind in ("zeros", "ones") and W == 1601:
                assert len(data) < bound // 4


def test_filter_none_and_partial_last_segment(emu_encoder):
    for W, H, S in ((17, 33, 16), (5, 7, 3), (1601, 17, 16)):
        img = content("blobs", H, W, seed=3)
        check_file(emu_encoder(rows_per_segment=S, filter=0).encode(img)[0], img, 0)


def _huffman_max_depth(freqs):
    heap = [(f, i, 0) for i, f in enumerate(freqs) if f]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        f1, _, d1 = heapq.heappop(heap)
        f2, _, d2 = heapq.heappop(heap)
        heapq.heappush(heap, (f1 + f2, k, max(d1, d2) + 1))
        k += 1
    return heap[0][2]


def test_code_lengths_are_limited_to_15_bits(emu_encoder):
    """A segment whose byte histogram is Fibonacci-shaped: the unlimited Huffman code is deeper than 15 bits, which a
    dynamic block header cannot express -- a correct decode proves the limit (and the Kraft repair) works."""
    fib = [1, 2]            # with end-of-block (count 1) the counts 1, 1, 2, 3, 5, ...: a Huffman tree that is one chain
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    W = 64
    sym = np.concatenate([np.full(f, 1 + i, np.uint8) for i, f in enumerate(fib)])
    H = -(-len(sym) // (3 * W))
    flat = np.concatenate([sym, np.full(H * 3 * W - len(sym), len(fib), np.uint8)])   # pad with the most frequent byte
    img = np.random.default_rng(5).permutation(flat).reshape(H, W, 3)
    hist = np.bincount(np.frombuffer(filtered_scanlines(img, 0), np.uint8), minlength=256).tolist() + [1]
    assert _huffman_max_depth(hist) > 15
    enc = emu_encoder(rows_per_segment=H, filter=0)
    data = enc.encode(img)[0]
    check_file(data, img, 0)
    assert len(data) < enc.max_bytes(W, H), "the segment must be Huffman coded, not stored"


def test_a_batch_of_eight_equals_eight_single_calls(emu_encoder):
    W, H = 17, 33
    imgs = np.stack([content(k, H, W, seed=s) for s in range(2) for k in ("zeros", "gradient", "blobs", "noise")])
    enc = emu_encoder()
    batch = enc.encode(imgs)
    assert len(batch) == 8
    for k in range(8):
        assert batch[k] == enc.encode(imgs[k])[0]
        check_file(batch[k], imgs[k], 4)


def test_bad_arguments_are_reported(emu_encoder):
    lib = emu_lib()
    enc = emu_encoder()
    img = content("gradient", 4, 4)
    out = np.zeros((1, 10), np.uint8)
    nb = np.zeros(1, np.int64)
    rc = lib.gs2m_png_encode(enc._h, 1, 4, 4, img.ctypes.data, 48, out.ctypes.data, 10, nb.ctypes.data, 4, 16, None)
    assert rc != 0 and b"out_stride" in lib.gs2m_last_error()
    rc = lib.gs2m_png_encode(enc._h, 1, 4, 4, img.ctypes.data, 48, out.ctypes.data, 10**6, nb.ctypes.data, 2, 16, None)
    assert rc != 0
    with pytest.raises(ValueError):
        enc.encode(np.zeros((4, 4, 4), np.uint8))
