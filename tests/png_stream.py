"""A plain deflate reader (RFC 1951: stored, fixed and dynamic blocks, lengths and distances) that reports the STRUCTURE of a
stream next to its bytes, and ``check_stream``, which holds a file of the device PNG encoder to the grammar that the header
comment of ``gs2mesh_amd/csrc/png_encode.hip`` promises.  Pure Python, no zlib in the inflate (``check_stream`` takes the
Adler-32 from ``zlib.adler32``); complete, so that it is validated on streams of zlib's own making (tests/test_png_edges.py)
before its report on ours is trusted.

It is stricter than zlib where the RFC is: a Huffman code must be complete (Kraft sum of the non-zero lengths exactly 1), the
two exceptions being those of RFC 1951 3.2.7 for the distance code (no distance code at all: every length 0; or a single
distance code of length 1)."""
import zlib
from dataclasses import dataclass, field

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
STORED_MAX = 65535


class StreamError(ValueError):
    pass


@dataclass
class Block:
    start: int                      # bit offset of BFINAL
    end: int = 0                    # bit offset one past the block's last bit
    bfinal: int = 0
    btype: int = 0
    # stored
    pad_count: int = 0              # bits skipped to the byte boundary, and their value
    pad_value: int = 0
    len: int = 0
    nlen: int = 0
    # dynamic
    hlit: int = 0
    hdist: int = 0
    hclen: int = 0
    cl_lens: list = field(default_factory=list)     # the 19 code-length code lengths, by symbol (not in HCLEN order)
    tokens: list = field(default_factory=list)      # (symbol of the code-length code, extra bits value) in order
    lit_lens: list = field(default_factory=list)
    dist_lens: list = field(default_factory=list)
    # contents
    data: bytes = b""
    n_literals: int = 0
    n_matches: int = 0


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def make_table(lens, what, allow_single=False):
    """(table, bits): ``table[next `bits` bits of the stream]`` = ``symbol << 4 | length`` or None (undefined code).
    Raises unless the code is complete; ``allow_single``: the distance code may also be empty or one code of length 1."""
    maxl = max(lens) if lens else 0
    used = [l for l in lens if l]
    if allow_single and (not used or used == [1]):
        tab = [None, None]
        for s, l in enumerate(lens):
            if l:
                tab[0] = s << 4 | 1
        return tab, 1
    if not used:
        raise StreamError(f"{what} code: no symbol has a length")
    kraft = sum(1 << (maxl - l) for l in used)
    if kraft > 1 << maxl:
        raise StreamError(f"{what} code is over-subscribed: lengths {sorted(used)}")
    if kraft < 1 << maxl:
        raise StreamError(f"{what} code is incomplete: lengths {sorted(used)}")
    count = [0] * (maxl + 2)
    for l in used:
        count[l] += 1
    code, nxt = 0, [0] * (maxl + 2)
    for l in range(1, maxl + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    tab = [None] * (1 << maxl)
    for s, l in enumerate(lens):
        if l:
            tab[_reverse(nxt[l], l)::1 << l] = [s << 4 | l] * (1 << (maxl - l))
            nxt[l] += 1
    return tab, maxl


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (make_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "fixed literal"), make_table([5] * 32, "fixed distance"))
    return _FIXED


class _Reader:
    def __init__(self, data):
        self.data, self.n = data, len(data)
        self.acc = self.cnt = self.at = 0        # bit buffer (LSB = next bit), its fill, next byte to load

    def pos(self):
        return 8 * self.at - self.cnt

    def fill(self):
        chunk = self.data[self.at:self.at + 8]
        self.acc |= int.from_bytes(chunk, "little") << self.cnt
        self.cnt += 8 * len(chunk)
        self.at += len(chunk)

    def bits(self, n):
        if self.cnt < n:
            self.fill()
            if self.cnt < n:
                raise StreamError("unexpected end of input")
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.cnt -= n
        return v

    def symbol(self, table, what):
        tab, nb = table
        if self.cnt < nb:
            self.fill()
        e = tab[self.acc & ((1 << nb) - 1)]
        if e is None:
            raise StreamError(f"undefined {what} code")
        if (e & 15) > self.cnt:
            raise StreamError("unexpected end of input")
        self.acc >>= e & 15
        self.cnt -= e & 15
        return e >> 4


def _stored(r, blk, out):
    blk.pad_count = -r.pos() % 8
    blk.pad_value = r.bits(blk.pad_count)
    blk.len, blk.nlen = r.bits(16), r.bits(16)
    if blk.len != (~blk.nlen & 0xffff):
        raise StreamError(f"stored block: LEN {blk.len:#06x} is not the complement of NLEN {blk.nlen:#06x}")
    p = r.pos() // 8
    if p + blk.len > r.n:
        raise StreamError("unexpected end of input in a stored block")
    out += r.data[p:p + blk.len]
    r.acc = r.cnt = 0
    r.at = p + blk.len
    blk.n_literals = blk.len


def _dynamic_header(r, blk):
    blk.hlit, blk.hdist, blk.hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    if blk.hlit > 286 or blk.hdist > 30:
        raise StreamError(f"HLIT {blk.hlit} / HDIST {blk.hdist} out of range")
    blk.cl_lens = [0] * 19
    for i in range(blk.hclen):
        blk.cl_lens[CL_ORDER[i]] = r.bits(3)
    cl = make_table(blk.cl_lens, "code-length")
    lens, total = [], blk.hlit + blk.hdist
    while len(lens) < total:
        s = r.symbol(cl, "code-length")
        if s < 16:
            blk.tokens.append((s, 0))
            lens.append(s)
            continue
        extra = r.bits((2, 3, 7)[s - 16])
        blk.tokens.append((s, extra))
        if s == 16:
            if not lens:
                raise StreamError("token 16 (repeat the previous length) with no previous length")
            rep, v = 3 + extra, lens[-1]
        else:
            rep, v = (3 if s == 17 else 11) + extra, 0
        if len(lens) + rep > total:
            raise StreamError(f"code lengths run past HLIT + HDIST = {total}")
        lens += [v] * rep
    blk.lit_lens, blk.dist_lens = lens[:blk.hlit], lens[blk.hlit:]
    if blk.lit_lens[256] == 0:
        raise StreamError("the literal/length code has no end-of-block")
    return make_table(blk.lit_lens, "literal/length"), make_table(blk.dist_lens, "distance", allow_single=True)


def _coded(r, blk, lit, dist, out):
    ltab, lbits = lit
    lmask = (1 << lbits) - 1
    data, n = r.data, r.n
    acc, cnt, at = r.acc, r.cnt, r.at
    append = out.append
    while True:
        if cnt < 48:                                  # a length / distance pair is at most 15 + 5 + 15 + 13 bits
            chunk = data[at:at + 8]
            acc |= int.from_bytes(chunk, "little") << cnt
            cnt += 8 * len(chunk)
            at += len(chunk)
        e = ltab[acc & lmask]
        if e is None:
            raise StreamError("undefined literal/length code")
        l = e & 15
        if l > cnt:
            raise StreamError("unexpected end of input")
        acc >>= l
        cnt -= l
        s = e >> 4
        if s < 256:
            append(s)
            blk.n_literals += 1
            continue
        if s == 256:
            break
        if s > 285:
            raise StreamError(f"undefined literal/length code {s}")
        r.acc, r.cnt, r.at = acc, cnt, at
        length = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
        d = r.symbol(dist, "distance")
        if d > 29:
            raise StreamError(f"undefined distance code {d}")
        d = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
        if d > len(out):
            raise StreamError("distance reaches before the start of the output")
        for _ in range(length):                       # byte by byte: the copy may overlap its own output
            append(out[-d])
        blk.n_matches += 1
        acc, cnt, at = r.acc, r.cnt, r.at
    r.acc, r.cnt, r.at = acc, cnt, at


def inflate(data):
    """The blocks of the raw deflate stream ``data`` (which must end with its final block, padded to the byte)."""
    r, out, blocks = _Reader(bytes(data)), bytearray(), []
    while True:
        blk = Block(start=r.pos())
        blk.bfinal, blk.btype = r.bits(1), r.bits(2)
        first = len(out)
        if blk.btype == 0:
            _stored(r, blk, out)
        elif blk.btype == 1:
            _coded(r, blk, *_fixed_tables(), out)
        elif blk.btype == 2:
            _coded(r, blk, *_dynamic_header(r, blk), out)
        else:
            raise StreamError("block type 3")
        blk.end = r.pos()
        blk.data = bytes(out[first:])
        blocks.append(blk)
        if blk.bfinal:
            break
    if (r.pos() + 7) // 8 != r.n:
        raise StreamError(f"{r.n - (r.pos() + 7) // 8} bytes of input left over after the final block")
    return blocks


def inflate_zlib(stream):
    """The blocks of a zlib stream (RFC 1950 without a dictionary); the Adler-32 is the caller's to check."""
    if len(stream) < 6 or stream[0] & 15 != 8 or (stream[0] << 8 | stream[1]) % 31 or stream[1] & 32:
        raise StreamError("not a zlib header")
    return inflate(stream[2:-4])


def stored_bound(L):
    return L + 5 * -(-L // STORED_MAX)


def check_stream(idat, W, H, S, filt, scan):
    """Assert that the IDAT payload ``idat`` of a W x H image cut into segments of S rows is what png_encode.hip's header
    comment says, and holds ``scan`` (the filtered scanlines).  Returns one dict per segment: ``kind`` ("dynamic" or
    "stored"), ``offset`` (bytes from the start of the PNG FILE: IDAT data starts at 41), ``nbytes``, ``L``, ``blocks``."""
    S = min(S, H)
    R = 3 * W + 1
    assert len(scan) == H * R and all(scan[r * R] == filt for r in range(H))
    assert idat[:2] == b"\x78\x01"
    blocks = inflate_zlib(idat)
    segs, i, done = [], 0, 0
    for r0 in range(0, H, S):
        L = min(S, H - r0) * R
        assert i < len(blocks), f"segment at row {r0}: the stream has ended"
        b = blocks[i]
        assert b.start % 8 == 0, f"segment at row {r0} starts at bit {b.start}"
        if b.btype == 2:
            assert i + 1 < len(blocks)
            sync = blocks[i + 1]
            assert not b.bfinal and (b.hlit, b.hdist, b.dist_lens) == (257, 1, [0])
            assert b.n_matches == 0 and b.n_literals == L
            assert max(b.lit_lens) <= 15 and max(b.cl_lens) <= 7
            assert (sync.btype, sync.bfinal, sync.len, sync.nlen, sync.pad_value) == (0, 0, 0, 0xffff, 0)
            assert sync.end % 8 == 0 and sync.end - sync.start == 3 + sync.pad_count + 32
            used, kind = [b, sync], "dynamic"
            nbytes = (sync.end - b.start) // 8
            assert nbytes < stored_bound(L), f"dynamic segment at row {r0}: {nbytes} bytes, stored {stored_bound(L)}"
        else:
            nblk = -(-L // STORED_MAX)
            used, kind = blocks[i:i + nblk], "stored"
            assert len(used) == nblk
            for j, s in enumerate(used):
                assert (s.btype, s.bfinal, s.pad_count) == (0, 0, 5), f"segment at row {r0}, block {j}"
                assert s.pad_value == 0 and s.len == min(STORED_MAX, L - j * STORED_MAX)
            nbytes = (used[-1].end - b.start) // 8
            assert nbytes == stored_bound(L)
        assert b"".join(u.data for u in used) == scan[done:done + L], f"segment at row {r0} decodes to other bytes"
        segs.append(dict(kind=kind, offset=41 + 2 + b.start // 8, nbytes=nbytes, L=L, blocks=used))
        done += L
        i += len(used)
    assert i == len(blocks) - 1, f"{len(blocks) - 1 - i} blocks between the last segment and the final block"
    last = blocks[i]
    assert (last.btype, last.bfinal, last.data, last.start % 8) == (1, 1, b"", 0)
    assert idat[-6:-4] == b"\x03\x00" and last.end - last.start == 10
    assert int.from_bytes(idat[-4:], "big") == zlib.adler32(scan)
    return segs
