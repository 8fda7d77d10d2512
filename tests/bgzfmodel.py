"""The rule of the BGZF input side of libtgsf_text (include/tgsf_text.h, tgsf_text_bgzf_*), restated in Python over zlib: the
member walk (bgzf_peek of tgsfilter_amd/host/bam.cpp, plus the bound usize <= 65536), the verdict on a member (zlib's raw
inflate reaches the end of a final block with exactly usize bytes), and writers for what the tests feed both with -- a
bit-level DEFLATE writer for hand-made streams (stored, fixed, dynamic from chosen code lengths) and a member writer that can
lie about BC and ISIZE and add extra subfields."""
from __future__ import annotations

import struct
import zlib

END, IRREGULAR, CAPACITY = 0, 1, 2
NONE = 0xFFFFFFFF
MAX_USIZE = 65536
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


# ---- the rule ----------------------------------------------------------------------------------------------------------
def peek(gz, at):
    """The member at byte `at`: (payload, clen, usize, bsize); "cut" when the bytes left are the front of one as far as they
    go; None when they are not a member."""
    n = len(gz)
    left = n - at
    if gz[at:at + 4] != b"\x1f\x8b\x08\x04"[:min(left, 4)]:
        return None
    if left < 18:
        return "cut"
    xlen = gz[at + 10] | gz[at + 11] << 8
    if left < 12 + xlen:
        return "cut"
    bsize, x = 0, at + 12
    while x + 4 <= at + 12 + xlen:
        slen = gz[x + 2] | gz[x + 3] << 8
        if gz[x:x + 2] == b"BC" and slen == 2 and x + 6 <= at + 12 + xlen:
            bsize = (gz[x + 4] | gz[x + 5] << 8) + 1
        x += 4 + slen
    if bsize < 12 + xlen + 8:
        return None
    if bsize > left:
        return "cut"
    usize = struct.unpack_from("<I", gz, at + bsize - 4)[0]
    if usize > MAX_USIZE:
        return None
    return at + 12 + xlen, bsize - 12 - xlen - 8, usize, bsize


def walk(gz, final=True, max_blocks=1 << 30, max_out=1 << 62):
    """(blocks as (payload, clen, usize, out), stop, consumed, out_bytes)."""
    at, out, blocks, stop = 0, 0, [], END
    while at < len(gz):
        m = peek(gz, at)
        if m is None:
            stop = IRREGULAR
            break
        if m == "cut":
            stop = IRREGULAR if final else END
            break
        payload, clen, usize, bsize = m
        if len(blocks) == max_blocks or usize > max_out - out:
            stop = CAPACITY
            break
        blocks.append((payload, clen, usize, out))
        out += usize
        at += bsize
    return blocks, stop, at, out


def inflate(payload, usize):
    """The member's bytes when it is GOOD, else None."""
    if usize == 0 and len(payload) <= 2:
        return b""
    d = zlib.decompressobj(-15)
    try:
        o = d.decompress(bytes(payload), usize + 1)
    except zlib.error:
        return None
    return o if d.eof and len(o) == usize else None


def rule(gz, final=True, max_blocks=1 << 30, max_out=1 << 62):
    blocks, stop, consumed, out_bytes = walk(gz, final, max_blocks, max_out)
    data = [inflate(gz[p:p + c], u) for p, c, u, _ in blocks]
    bad = next((i for i, d in enumerate(data) if d is None), NONE)
    return {"blocks": blocks, "n_blocks": len(blocks), "stop": stop, "consumed": consumed, "out_bytes": out_bytes, "bad_block": bad, "data": data}


# ---- the member writer ---------------------------------------------------------------------------------------------------
def member(payload, usize, pre=b"", post=b"", bc=None, crc=0, flg=4, magic=b"\x1f\x8b\x08", with_bc=True):
    """One member around a DEFLATE stream; usize is what ISIZE says, bc what BC says (None: the truth); pre / post are whole
    extra subfields in front of and behind BC."""
    extra = pre + ((b"BC" + struct.pack("<HH", 2, 0)) if with_bc else b"") + post
    total = 12 + len(extra) + len(payload) + 8
    if with_bc:
        extra = pre + b"BC" + struct.pack("<HH", 2, (total - 1 if bc is None else bc) & 0xFFFF) + post
    return magic + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + bytes(payload) + struct.pack("<II", crc, usize & 0xFFFFFFFF)


def subfield(tag, data):
    return tag + struct.pack("<H", len(data)) + data


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return co.compress(data) + co.flush()


def zmember(data, **kw):
    return member(deflate(data, **kw), len(data), crc=zlib.crc32(data))


EOF_MEMBER = member(b"\x03\x00", 0)


# ---- the bit-level DEFLATE writer ---------------------------------------------------------------------------------------
def canonical(lengths):
    """sym -> (code, length) of the canonical Huffman code with these lengths (0: no code)."""
    code, out = 0, {}
    for l in range(1, 16):
        for s, x in enumerate(lengths):
            if x == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def complete_lengths(n_total, used):
    """Lengths of a complete code over the symbols `used` (two or more), 0 for the others."""
    m = len(used)
    k = m.bit_length() - 1
    longer = 2 * (m - (1 << k))
    lens = [0] * n_total
    for i, s in enumerate(sorted(used)):
        lens[s] = k if i < m - longer else k + 1
    return lens


def len_symbol(length):
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        """nbits of value, least significant first."""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        return self

    def code(self, pair):
        """A Huffman code, first bit first."""
        c, l = pair
        return self.put(int(format(c, "0%db" % l)[::-1], 2), l)

    def align(self):
        return self.put(0, -self.n % 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")

    # -- blocks --
    def stored(self, data, final, nlen=None, length=None):
        self.put(final, 1).put(0, 2).align()
        length = len(data) if length is None else length
        self.put(length, 16).put(length ^ 0xFFFF if nlen is None else nlen, 16)
        for b in data:
            self.put(b, 8)
        return self

    def tokens(self, toks, lit, dist):
        """toks: a literal byte; ("m", length, distance); ("s", lit/len symbol) alone; ("r", length symbol, extra value,
        distance symbol, extra value) as they are."""
        for t in toks:
            if isinstance(t, int):
                self.code(lit[t])
            elif t[0] == "s":
                self.code(lit[t[1]])
            else:
                if t[0] == "m":
                    ls, lx, lv = len_symbol(t[1])
                    ds, dx, dv = dist_symbol(t[2])
                else:
                    _, ls, lv, ds, dv = t
                    lx, dx = LEN_EXTRA[ls - 257] if ls < 286 else 0, DIST_EXTRA[ds] if ds < 30 else 0
                self.code(lit[ls]).put(lv, lx).code(dist[ds]).put(dv, dx)
        return self

    def fixed(self, toks, final, end=True):
        self.put(final, 1).put(1, 2)
        return self.tokens(list(toks) + ([("s", 256)] if end else []), canonical(FIXED_LIT), canonical(FIXED_DIST))

    def dynamic(self, toks, final, lit_lens, dist_lens, cl_lens=None, hclen=19, cl_seq=None, hlit=None, hdist=None, end=True):
        """A dynamic block from chosen code lengths.  cl_seq: the header's code-length symbols as (symbol, extra value) pairs
        (None: one symbol per length, no repeats); cl_lens: the code-length code's own lengths (None: a complete code over
        all 19); hlit / hdist: the counts the header states (None: len(lit_lens), len(dist_lens))."""
        cl_lens = [4] * 13 + [5] * 6 if cl_lens is None else cl_lens
        hlit, hdist = len(lit_lens) if hlit is None else hlit, len(dist_lens) if hdist is None else hdist
        self.put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
        for i in range(hclen):
            self.put(cl_lens[CL_ORDER[i]], 3)
        cl = canonical(cl_lens)
        for s, x in ([(l, 0) for l in list(lit_lens) + list(dist_lens)] if cl_seq is None else cl_seq):
            self.code(cl[s]).put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        return self.tokens(list(toks) + ([("s", 256)] if end else []), canonical(lit_lens), canonical(dist_lens))
