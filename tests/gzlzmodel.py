"""What the tests of the match search (level 1 of the BGZF output side, include/tgsf_text.h, tgsf_text_bgzf_out_level) need beside
tests/gzoutmodel.py: the texts in which matches are where the gain is, a bit-level DEFLATE reader that returns the tokens of a
payload -- the model of gzoutmodel.py says whether an output is right, this one says what it is made of -- and zlib's size
for the same cuts at a level."""
from __future__ import annotations

import struct
import zlib

import numpy as np

from tests import gzoutmodel as zm

MEMBER, FRAME = zm.MEMBER, zm.FRAME

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def hifi_like(rng, n):
    """n bytes of HiFi-like FASTQ: names with a long common prefix, qualities in runs."""
    parts, size, i = [], 0, 0
    while size < n:
        l = int(rng.integers(800, 4000)); k = l // 6 + 1
        q = np.repeat(rng.choice(np.frombuffer(b"~~~~~~~~~~~~nbZK?5", np.uint8), k), rng.integers(1, 12, k))[:l]
        l = len(q)
        rec = (b"@m64011_190830_220126/%d/ccs np=%d rq=0.99%d\n" % (4194370 + i * 67, 5 + i % 20, i % 10)
               + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), l)) + b"\n+\n" + q.tobytes() + b"\n")
        parts.append(rec); size += len(rec); i += 1
    return b"".join(parts)[:n]


def three_copies(rng, block=20000, values=64):
    """A block of uniformly random bytes over `values` values, written three times: the second and third cost match tokens alone."""
    return bytes(rng.integers(0, values, block).astype(np.uint8)) * 3


def uniform(rng, n):
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def noise(rng, n):
    """n bytes over all 256 byte values, the value v with a weight of 1 / (v + 4): a prefix code gains on them (so a dynamic
    block is written, whose tokens can be read), and four bytes in a row hardly ever repeat by chance."""
    w = 1.0 / (np.arange(256) + 4.0)
    return bytes(rng.choice(256, n, p=w / w.sum()).astype(np.uint8))


def copy_text(rng, before, length, dist, after=0):
    """`before` noise bytes (>= dist), then `length` bytes each of which repeats the byte `dist` back, then `after` noise bytes.
    dist < length: the copy overlaps itself, a pattern of period dist."""
    assert before >= dist >= 1
    t = bytearray(noise(rng, before))
    if dist > 1 and t[-1] == t[-dist]:                                  # (the byte in front of the copy does not belong to it)
        t[-dist] ^= 0x55
    for _ in range(length):
        t.append(t[-dist])
    tail = bytearray(noise(rng, after))
    if after and tail[0] == t[-dist]:                                   # (nor the byte behind it)
        tail[0] ^= 0xAA
    return bytes(t + tail)


def copies_text(rng, length, dist, place, reps):
    """copy_text `reps` times over, each with fresh noise in front of it and as much of it as puts the copy's first byte at
    `place` modulo 1024 (of the whole text: of its member, as long as the text is one)."""
    t = bytearray()
    for _ in range(reps):
        b = max(dist, 8)
        t += copy_text(rng, b + (place - len(t) - b) % 1024, length, dist)
    return bytes(t)


# ---- the tokens of a payload ---------------------------------------------------------------------------------------------------
class _Bits:
    """The bits of `data`, the lowest of each byte first, through a small window (shifting one long integer costs its length)."""

    def __init__(self, data):
        self.data, self.n = data, 8 * len(data)
        self.at = 0                                                      # bits consumed
        self.next, self.acc, self.have = 0, 0, 0

    def peek(self, k):
        """The next k bits, zeros behind the end."""
        while self.have < k:
            if self.next < len(self.data):
                self.acc |= self.data[self.next] << self.have
            self.next += 1
            self.have += 8
        return self.acc & ((1 << k) - 1)

    def skip(self, k):
        assert self.at + k <= self.n, "the payload ends inside a block"
        self.peek(k)
        self.acc >>= k
        self.have -= k
        self.at += k

    def get(self, k):
        x = self.peek(k)
        self.skip(k)
        return x

    def to_byte(self):
        self.skip(-self.at % 8)


def _decoder(lengths):
    """The canonical code over `lengths` as a table: the next 15 bits of the stream -> (symbol, its length); None where no code
    begins."""
    table, code = [None] * (1 << 15), 0
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                assert code < 1 << l, "an over-subscribed code"
                rev = int(format(code, "0%db" % l)[::-1], 2)            # the stream has a code's first bit lowest
                for hi in range(0, 1 << 15, 1 << l):
                    table[hi | rev] = (s, l)
                code += 1
        code <<= 1
    return table


def _symbol(b, table):
    e = table[b.peek(15)]
    assert e is not None, "no code of 15 bits or less"
    b.skip(e[1])
    return e[0]


_FIXED_LIT = _decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _decoder([5] * 30)


def tokens(payload):
    """The blocks of a raw DEFLATE stream: per block a list of tokens, an int for a literal, (length, distance) for a match.
    A stored block's bytes are its literals."""
    b, blocks = _Bits(bytes(payload)), []
    while True:
        final, kind = b.get(1), b.get(2)
        toks = []
        if kind == 0:
            b.to_byte()
            n, nn = b.get(16), b.get(16)
            assert n == nn ^ 0xFFFF, "LEN and NLEN"
            toks = [b.get(8) for _ in range(n)]
        else:
            assert kind in (1, 2), "BTYPE 3"
            lit, dist = _FIXED_LIT, _FIXED_DIST
            if kind == 2:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = b.get(3)
                clt, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(b, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    else:
                        lens += [0] * (3 + b.get(3) if s == 17 else 11 + b.get(7))
                assert len(lens) == hlit + hdist, "a run of code lengths passes the end"
                lit, dist = _decoder(lens[:hlit]), _decoder(lens[hlit:])
            while True:
                s = _symbol(b, lit)
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    assert s < 286, "length symbol 286 or 287"
                    length = LEN_BASE[s - 257] + b.get(LEN_EXTRA[s - 257])
                    d = _symbol(b, dist)
                    toks.append((length, DIST_BASE[d] + b.get(DIST_EXTRA[d])))
        blocks.append(toks)
        if final:
            assert b.n - b.at < 8, "bytes behind the final block"
            return blocks


def expand(blocks, limit=None):
    """The bytes the tokens stand for; a distance that reaches in front of the first byte is an error."""
    out = bytearray()
    for toks in blocks:
        for t in toks:
            if isinstance(t, tuple):
                length, d = t
                assert 3 <= length <= 258 and 1 <= d <= 32768 and d <= len(out), ("a match out of range", t, len(out))
                for _ in range(length):
                    out.append(out[-d])
            else:
                out.append(t)
    return bytes(out)


def member_payloads(gz, n_data_members):
    """The DEFLATE payloads of the first n_data_members members of a BGZF stream."""
    at, out = 0, []
    for _ in range(n_data_members):
        bsize = struct.unpack_from("<H", gz, at + 16)[0] + 1
        out.append(gz[at + 18:at + bsize - 8])
        at += bsize
    return out


def member_tokens(text, gz):
    """Per data member of `gz` (the output for `text`): its tokens as one list, having checked that they expand to its input."""
    cuts, out = zm.cuts(len(text)), []
    for (lo, hi), payload in zip(cuts, member_payloads(gz, len(cuts))):
        blocks = tokens(payload)
        assert expand(blocks) == text[lo:hi], ("the tokens of the member at", lo, "do not expand to its input")
        out.append([t for toks in blocks for t in toks])
    return out


def member_sizes(ends):
    return [e - b for b, e in zip(zm.starts(ends), [int(x) for x in ends])]


def zlib_size(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """What zlib writes for the same cuts at `level`, 26 bytes of framing a member."""
    total = 0
    for lo, hi in zm.cuts(len(text)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(co.compress(bytes(text[lo:hi])) + co.flush()) + FRAME
    return total


def length_extra_bits(length):
    return LEN_EXTRA[max(i for i, b in enumerate(LEN_BASE) if b <= length)] if length < 258 else 0


def distance_extra_bits(d):
    return DIST_EXTRA[max(i for i, b in enumerate(DIST_BASE) if b <= d)]
