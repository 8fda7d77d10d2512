"""The rule of the BGZF output side of libtgsf_text (include/tgsf_text.h, tgsf_text_bgzf_deflate*), restated in Python over
zlib and gzip: the member cuts, the framing and the bound; per member zlib's raw inflate, which must end a final block in the
payload's last byte having produced exactly the member's input; CRC32 and ISIZE; and the texts the tests feed it with.  The
compressed bytes themselves are not specified, so nothing here produces them: the model judges an output, whoever wrote it."""
from __future__ import annotations

import gzip
import heapq
import struct
import zlib

import numpy as np

from tests import bgzfmodel as gm

MEMBER = 0xFF00
FRAME = 26
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
EOF_MEMBER = gm.EOF_MEMBER
END, CAPACITY = 0, 2
assert len(EOF_MEMBER) == 28 and EOF_MEMBER[:16] == HEAD


def cuts(n):
    """(begin, end) of every member's input."""
    return [(at, min(at + MEMBER, n)) for at in range(0, n, MEMBER)]


def bound(n, eof):
    return n + 31 * ((n + MEMBER - 1) // MEMBER) + (28 if eof else 0)


def check(text, gz, eof, member_end=None, summary=None, what=""):
    """Everything the rule says about `gz` as the output for `text`.  Returns the number of stored members."""
    text, gz = bytes(text), bytes(gz)
    n = len(text)
    assert len(gz) <= bound(n, eof), (what, "over the bound", len(gz), bound(n, eof))
    at, ends, stored = 0, [], 0
    for lo, hi in cuts(n):
        usize = hi - lo
        assert gz[at:at + 16] == HEAD, (what, "header of the member at", at)
        bsize = struct.unpack_from("<H", gz, at + 16)[0] + 1
        assert FRAME < bsize <= usize + 5 + FRAME and at + bsize <= len(gz), (what, "BSIZE", bsize, usize)
        payload = gz[at + 18:at + bsize - 8]
        d = zlib.decompressobj(-15)
        got = d.decompress(payload, usize + 1)
        assert d.eof and got == text[lo:hi], (what, "member at", at, "does not inflate to its input", d.eof, len(got), usize)
        assert d.unused_data == b"" and d.unconsumed_tail == b"", (what, "bytes behind the final block", len(d.unused_data))
        # a stored member: one final stored block and nothing else; whatever else a build writes is smaller than that
        if payload[0] & 7 == 1 and len(payload) == usize + 5:
            stored += 1
        else:
            assert len(payload) < usize + 5, (what, "a member that one stored block beats", len(payload), usize)
        crc, isize = struct.unpack_from("<II", gz, at + bsize - 8)
        assert crc == zlib.crc32(text[lo:hi]) and isize == usize, (what, "trailer of the member at", at, hex(crc), isize)
        at += bsize
        ends.append(at)
    if eof:
        assert gz[at:at + 28] == EOF_MEMBER, (what, "the EOF member")
        at += 28
        ends.append(at)
    assert at == len(gz), (what, "bytes behind the last member", at, len(gz))
    assert gzip.decompress(gz) == text if gz else text == b"", (what, "gzip.decompress")
    if member_end is not None:
        assert [int(x) for x in member_end] == ends, (what, "member_end", list(member_end)[:4], ends[:4])
    if summary is not None:
        want = {"in_bytes": n, "n_bytes": len(gz), "n_members": len(ends), "stored": stored, "stop": END, "reserved": 0}
        assert {k: summary[k] for k in want} == want and summary["device_ms"] >= 0.0, (what, summary, want)
    return stored


def starts(member_end):
    return [0] + [int(x) for x in member_end[:-1]]


def huffman_only_size(text):
    """What zlib writes for the same cuts with Z_HUFFMAN_ONLY, 26 bytes of framing a member."""
    total = 0
    for lo, hi in cuts(len(text)):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        total += len(co.compress(bytes(text[lo:hi])) + co.flush()) + FRAME
    return total


def huffman_depth(freqs, shallow=True):
    """The longest code of a Huffman tree over `freqs` (two or more, positive) without any limit; among nodes of equal weight
    the tree merges the shallowest first (shallow: the least depth an optimal code can have) or the deepest first."""
    heap = [(f, 0, i) for i, f in enumerate(freqs)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        h = max(abs(a[1]), abs(b[1])) + 1
        heapq.heappush(heap, (a[0] + b[0], h if shallow else -h, k))
        k += 1
    return abs(heap[0][1])


def member_freqs(text):
    """Per member: the counts of the bytes that occur, and 1 for the end of the block."""
    return [[int(c) for c in np.bincount(np.frombuffer(bytes(text[lo:hi]), np.uint8), minlength=256) if c] + [1] for lo, hi in cuts(len(text))]


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def fastq_like(rng, n):
    """n bytes of FASTQ-like text: names, bases, '+', qualities around 30."""
    parts, size, i = [], 0, 0
    while size < n:
        l = int(rng.integers(40, 2500))
        rec = b"@read_%d/%d ch=%d\n" % (i, l, i % 512) + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), l)) + b"\n+\n" + \
            bytes((rng.normal(30, 7, l).clip(2, 60).astype(np.uint8) + 33)) + b"\n"
        parts.append(rec)
        size += len(rec)
        i += 1
    return b"".join(parts)[:n]


def from_freqs(rng, symbols, freqs):
    """A text in which symbols[i] occurs freqs[i] times, shuffled."""
    a = np.repeat(np.asarray(symbols, np.uint8), freqs)
    rng.shuffle(a)
    return a.tobytes()


def fibonacci(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def steeper_than_fibonacci(k):
    """f[i] = f[i-1] + f[i-2] + 1: the two lightest nodes always weigh less than the next leaf, so every Huffman tree over
    these (and one more symbol of weight 1) is a chain."""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2] + 1)
    return f[:k]
