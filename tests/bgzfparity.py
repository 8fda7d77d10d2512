"""Shared checks of the BGZF input side of libtgsf_text (include/tgsf_text.h, tgsf_text_bgzf_*): a backend (the HIP build on
the GPU box, the serial emulation of the same kernels elsewhere) against tests/bgzfmodel.py -- the walk word for word, the
verdict on every member, every byte of every good member, canaries around the output -- after every input has been asserted
on the model first.  tests/test_bgzf_emul.py and tests/test_bgzf_gpu.py run them."""
from __future__ import annotations

import ctypes as C
import gzip
import os
import threading
import zlib

import numpy as np

from tests import bamparity as bp, bgzfmodel as gm, textmodel, textoutparity as top
from tgsfilter_amd import text as tgtext

END, IRREGULAR, CAPACITY, NONE = gm.END, gm.IRREGULAR, gm.CAPACITY, gm.NONE
HostMem, TorchMem = bp.HostMem, bp.TorchMem
_refused = top._refused
FRONT = 17                                                             # the output begins at an odd address


def same_walk(got, m, what=""):
    blocks, stop, consumed, out_bytes = got
    assert [tuple(int(x) for x in b) for b in blocks] == m["blocks"], (what, "blocks")
    assert (stop, consumed, out_bytes) == (m["stop"], m["consumed"], m["out_bytes"]), (what, stop, consumed, out_bytes, m["stop"], m["consumed"], m["out_bytes"])


def same_summary(s, m, what=""):
    for k in ("n_blocks", "stop", "consumed", "out_bytes", "bad_block"):
        assert s[k] == m[k], (what, k, s, {x: m[x] for x in m if x not in ("data", "blocks")})
    assert s["reserved"] == 0 and s["device_ms"] >= 0.0, (what, s)


def same_bytes(got, m, what=""):
    """got: out_bytes bytes; every good member's bytes are right (a bad member's are unspecified)."""
    for (_, _, usize, out), d in zip(m["blocks"], m["data"]):
        if d is not None and bytes(got[out:out + usize]) != d:
            g = bytes(got[out:out + usize])
            at = next(i for i in range(usize) if g[i] != d[i])
            raise AssertionError((what, "member at", out, "differs at byte", at, g[max(0, at - 16):at + 16], d[max(0, at - 16):at + 16]))


class Inflater:
    """One TextIndexer reserved for BGZF; run() inflates a chunk by the device form, into a caller's buffer between canaries,
    and compares everything with the model."""

    def __init__(self, text_lib, dev, max_gz=1 << 20, max_blocks=64, max_bytes=1 << 20):
        self.dev, self.lib = dev, text_lib
        self.tx = tgtext.TextIndexer(0, max_bytes, 16, text_lib)
        self.tx.reserve_bgzf(max_gz, max_blocks)

    def run(self, gz, final=True, expect=None, what="", payloads=None):
        """expect = (stop, n_blocks, bad_block): asserted on the model first.  Returns the model's result.  payloads: (payload,
        usize) pairs instead of gz, for streams longer than a BC field can state: the chunk is the bare payloads, eight bytes
        between them, and the table is made here, not walked."""
        if payloads is None:
            gz = bytes(gz)
            m = gm.rule(gz, final, self.tx.max_blocks)
            walked = tgtext.bgzf_walk(gz, self.tx.max_blocks, final=final, lib_path=self.lib)
            same_walk(walked, m, what)
        else:
            gz, blocks, out = b"\xa5" * 16, [], 0
            for p, u in payloads:
                blocks.append((len(gz), len(p), u, out))
                gz += bytes(p) + b"\xa5" * 8
                out += u
            data = [gm.inflate(p, u) for p, u in payloads]
            m = {"blocks": blocks, "n_blocks": len(blocks), "stop": END, "consumed": len(gz), "out_bytes": out, "data": data,
                 "bad_block": next((i for i, d in enumerate(data) if d is None), NONE)}
            walked = (np.array(blocks, dtype=tgtext.BGZF_BLOCK_DTYPE), END)
        if expect is not None:
            assert (m["stop"], m["n_blocks"], m["bad_block"]) == tuple(expect), (what, "the model", m["stop"], m["n_blocks"], m["bad_block"], expect)
        dev, n = self.dev, m["out_bytes"]
        d_gz = dev.put(np.frombuffer(gz + b"\xa5" * (-len(gz) % 16 + 16), np.uint8))       # (what lies behind n_bytes does not count)
        d_out = dev.full(FRONT + n + 64, 0xA5)
        d_sum = dev.full(16 + 40 + 16, 0xA5)
        dev.sync()
        self.tx.inflate_device(len(gz), walked[0], walked[1], dev.ptr(d_out) + FRONT, n, d_gz=dev.ptr(d_gz), d_summary=dev.ptr(d_sum) + 16, stream=dev.stream)
        dev.sync()
        raw = dev.get(d_sum)
        assert (raw[:16] == 0xA5).all() and (raw[56:] == 0xA5).all(), (what, "the summary's canaries")
        same_summary(tgtext.BgzfSummary.from_buffer_copy(raw[16:56].tobytes()).as_dict(), m, what)
        got = dev.get(d_out)
        assert (got[:FRONT] == 0xA5).all() and (got[FRONT + n:] == 0xA5).all(), (what, "written outside the output")
        same_bytes(got[FRONT:FRONT + n], m, what)
        return m

    def each(self, cases, what=""):
        """cases: (payload, usize) pairs.  Those the model calls good go through in one chunk; every other one sits between two
        good members, which must stay right.  Returns (good, bad) counts."""
        guard = gm.zmember(bytes(range(7, 200)) * 3)
        verdict = [gm.inflate(p, u) is not None for p, u in cases]
        long = [c for c in cases if len(c[0]) + 26 > 65536]
        if long:
            assert all(gm.inflate(p, u) is not None for p, u in long)
            self.run(None, True, (END, len(long), NONE), (what, "longer than a member"), payloads=long)
        good = [gm.member(p, u) for (p, u), v in zip(cases, verdict) if v and len(p) + 26 <= 65536]
        for lo in range(0, len(good), self.tx.max_blocks):
            self.run(b"".join(good[lo:lo + self.tx.max_blocks]), True, (END, len(good[lo:lo + self.tx.max_blocks]), NONE), (what, "the good ones"))
        for i, ((p, u), v) in enumerate(zip(cases, verdict)):
            if not v:
                self.run(guard + gm.member(p, u) + guard, True, (END, 3, 1), (what, "bad case", i))
        return sum(verdict), len(verdict) - sum(verdict)

    def close(self):
        self.tx.close()


B = gm.Bits


# ---- 1: stored blocks ------------------------------------------------------------------------------------------------------
def stored(text_lib, dev):
    rng = np.random.default_rng(201)
    data = bytes(rng.integers(0, 256, 65536).astype(np.uint8))
    good = [(B().stored(data[:n], 1).bytes(), n) for n in (0, 1, 2, 65535)]
    good.append((B().stored(data[:65535], 0).stored(data[65535:], 1).bytes(), 65536))
    good.append((B().stored(data[:40000], 0).stored(data[40000:], 1).bytes(), 65536))
    ends = set()
    for k in range(8):                                                 # behind a fixed block that ends on each of the 8 bit positions
        w = B().fixed(list(data[:3]) + [200] * k, 0)                   # (literal 200 has nine bits)
        ends.add(w.n % 8)
        good.append((w.stored(data[9:100], 1).bytes(), 3 + k + 91))
    assert len(ends) == 8
    good.append((B().stored(b"", 0).stored(b"", 0).stored(data[:77], 1).bytes(), 77))          # empty non-final blocks first
    bad = [(B().stored(data[:10], 1, nlen=(10 ^ 0xFFFF) ^ 0x100).bytes(), 10), (B().put(1, 1).put(3, 2).put(0, 29).bytes(), 0),
           (B().stored(data[:10], 1).bytes()[:-1], 10), (B().stored(data[:10], 0).bytes(), 10)]
    D = Inflater(text_lib, dev, max_gz=1 << 20, max_bytes=1 << 20)
    try:
        assert D.each(good, "stored") == (len(good), 0)
        assert D.each(bad, "stored, bad") == (0, len(bad))
    finally:
        D.close()


# ---- 2: the fixed code -----------------------------------------------------------------------------------------------------
def fixed_code(text_lib, dev):
    good = [(B().fixed(list(range(256)), 1).bytes(), 256)]
    toks, n = list(range(40, 45)), 5
    for ls in range(257, 286):
        for lv in {0, (1 << gm.LEN_EXTRA[ls - 257]) - 1}:
            toks.append(("r", ls, lv, 2, 0))                               # distance 3
            n += 258 if ls == 285 else gm.LEN_BASE[ls - 257] + lv
    good.append((B().fixed(toks, 1).bytes(), n))
    toks, n = [ord("a") + i % 7 for i in range(300)], 300
    for ds in range(30):
        for dv in sorted({0, (1 << gm.DIST_EXTRA[ds]) - 1}):
            d = gm.DIST_BASE[ds] + dv
            while n < d:                                               # enough bytes in front to be legal
                toks.append(("m", 258, 7))
                n += 258
            toks.append(("r", 257 + (ds % 8), 0, ds, dv))
            n += 3 + ds % 8
    assert n <= 65536
    good.append((B().fixed(toks, 1).bytes(), n))
    pre = [1, 2, 3, 4]
    bad = [(B().fixed(pre + [("s", 286)], 1).bytes(), 4), (B().fixed(pre + [("s", 287)], 1).bytes(), 4),
           (B().fixed(pre + [("r", 257, 0, 30, 0)], 1).bytes(), 7), (B().fixed(pre + [("r", 257, 0, 31, 0)], 1).bytes(), 7)]
    D = Inflater(text_lib, dev)
    try:
        assert D.each(good, "fixed") == (len(good), 0)
        assert D.each(bad, "fixed, bad") == (0, len(bad))
    finally:
        D.close()


# ---- 3: copies on the seams of 64 lanes ------------------------------------------------------------------------------------------
def copies(text_lib, dev):
    rng = np.random.default_rng(203)
    lits = [int(x) for x in rng.integers(0, 256, 70)]
    cases = []
    for d in (1, 2, 3, 63, 64, 65):
        for l in (3, 63, 64, 65, 258):
            cases.append((B().fixed(lits[:d] + [("m", l, d)] + lits[:5] + [("m", l, d)], 1).bytes(), d + 2 * l + 5))
    toks, n = [lits[0], lits[1], lits[2]], 3
    for i in range(130):                                               # a match that begins in one batch's literals
        if i % 2:
            toks.append(("m", 3 + i % 9, 1 + i % 3))
            n += 3 + i % 9
        else:
            toks.append(lits[i % 70])
            n += 1
    cases.append((B().fixed(toks, 1).bytes(), n))
    cases.append((B().fixed(lits[:40] + [("m", 10, 40)], 1).bytes(), 50))                  # as far back as there are bytes
    cases.append((B().fixed(lits[:40] + [("m", 10, 41)], 1).bytes(), 50))                  # ... and one more: bad
    cases.append((B().fixed(lits[:3] + [("m", 10, 3)], 1).bytes(), 12))                    # a byte beyond usize: bad
    w, n = B().stored(bytes(rng.integers(0, 256, 32770).astype(np.uint8)), 0), 32770
    toks = [("m", 258, 32768)] * ((65536 - n) // 258)
    assert n + 258 * len(toks) == 65536
    cases.append((w.fixed(toks, 1).bytes(), 65536))                    # distance 32768 in a member of 65536 bytes
    D = Inflater(text_lib, dev)
    try:
        assert D.each(cases, "copies") == (len(cases) - 2, 2)
    finally:
        D.close()


# ---- 4: dynamic headers ------------------------------------------------------------------------------------------------------
def _lens(total, used):
    return gm.complete_lengths(total, used)


def dynamic_headers(text_lib, dev):
    cases, expect = [], []

    def add(w, usize, good):
        cases.append((w.bytes(), usize))
        expect.append(good)

    lit2 = lambda n: _lens(n, [65, 66, 256, 257])                      # noqa: E731
    c2 = gm.canonical(lit2(258))
    msg = [65, 66, 65, ("m", 3, 2), 66]
    # HLIT 257 and HDIST 1; HLIT 286 and HDIST 30; HCLEN 19 (all of these) and 4 (four code-length symbols, 16, 17, 18 and 0,
    # cannot state a length but 0: there is no symbol 256)
    add(B().dynamic([65, 66, 65], 1, _lens(257, [65, 66, 256]), [0]), 3, True)
    add(B().dynamic(msg, 1, lit2(286), _lens(30, [0, 1, 29])), 7, True)
    add(B().dynamic([], 1, [0] * 257, [0], cl_lens=[2] + [0] * 15 + [2, 2, 2], hclen=4, cl_seq=[(18, 127), (18, 109)], end=False), 0, False)
    # codes of length 15 in both alphabets
    l15 = list(range(1, 16)) + [15]
    lit15 = [0] * 286
    for sym, l in zip([256, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 257, 258, 285], l15):
        lit15[sym] = l
    add(B().dynamic([65, 76, 75, ("r", 258, 0, 0, 0), ("r", 285, 0, 0, 0), ("r", 257, 0, 15, 0), ("r", 257, 0, 14, 0), 74], 1, lit15, l15 + [0] * 14),
        3 + 4 + 258 + 3 + 3 + 1, True)
    # 16, 17 and 18 with their lowest and highest counts
    seq = [(8, 0), (16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127), (18, 73), (1, 0), (2, 0), (3, 0), (4, 0), (6, 0), (7, 0), (1, 0), (1, 0)]
    lits = [8] * 10 + [0] * (3 + 10 + 11 + 138 + 84) + [1, 2, 3, 4, 6, 7]
    assert len(lits) == 262
    add(B().dynamic([0, 9, 5, ("r", 257, 0, 0, 0), ("r", 261, 0, 1, 0)], 1, lits, [1, 1], cl_seq=seq), 3 + 3 + 7, True)
    # a repeat that crosses from the literal lengths into the distance lengths: 285 and the four distance codes repeat 284's
    litx = _lens(286, [65, 256, 284, 285])
    add(B().dynamic([65] * 4 + [("r", 284, 0, 3, 0)], 1, litx, [2] * 4, cl_seq=[(l, 0) for l in litx[:285]] + [(16, 2)]), 4 + 227, True)
    # a single distance code of length 1 (good), and its unused code used (bad)
    add(B().dynamic([65, 66, ("m", 3, 1)], 1, lit2(258), [1]), 5, True)
    add(B().dynamic([65, 66], 1, lit2(258), [1], end=False).code(c2[257]).put(1, 1).code(c2[256]), 5, False)
    # no distance code: literals only (good), then a length symbol (bad)
    add(B().dynamic([65, 66], 1, lit2(258), [0]), 2, True)
    add(B().dynamic([65, 66], 1, lit2(258), [0], end=False).code(c2[257]).put(0, 1).code(c2[256]), 5, False)
    # bad headers
    ok = lit2(258)
    add(B().dynamic([65], 1, ok, [1], cl_seq=[(16, 0)] + [(l, 0) for l in ok[3:]] + [(1, 0)]), 1, False)                  # 16 first
    add(B().dynamic([65], 1, ok, [1], cl_seq=[(l, 0) for l in ok[:257]] + [(17, 0)]), 1, False)                          # a repeat one past HLIT + HDIST
    add(B().dynamic([65], 1, _lens(258, [65, 66, 257, 0]), [1], end=False), 1, False)                                    # no symbol 256
    over = ok[:]
    over[67] = 1
    add(B().dynamic([65], 1, over, [1]), 1, False)                                                                     # over-subscribed
    inc = ok[:]
    inc[66] = 0
    add(B().dynamic([65], 1, inc, [1]), 1, False)                                                                      # incomplete
    add(B().dynamic([65], 1, lit2(286) + [0], [1], hlit=287), 1, False)                                                 # HLIT 287
    add(B().dynamic([65], 1, ok, [1] + [0] * 30, hdist=31), 1, False)                                                   # HDIST 31
    for i, ((p, u), e) in enumerate(zip(cases, expect)):
        assert (gm.inflate(p, u) is not None) == e, ("the model", i, e)
    D = Inflater(text_lib, dev)
    try:
        assert D.each(cases, "dynamic headers") == (sum(expect), len(expect) - sum(expect))
    finally:
        D.close()


# ---- 5: what zlib writes ----------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 65280, 65535, 65536)


def zlib_data(rng, kind, n):
    if kind == "zeros":
        return bytes(n)
    if kind == "8mer":
        return (b"ACGTTGCA" * (n // 8 + 1))[:n]
    if kind == "bam":
        recs, have = [], 0
        while have < n:
            recs.append(bp.rnd_record(rng, 12, int(rng.integers(200, 3000)), aux=9, qmax=60))
            have += len(recs[-1])
        return b"".join(recs)[:n]
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def zlib_streams(text_lib, dev, sizes=SIZES):
    rng = np.random.default_rng(205)
    strategies = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)
    D = Inflater(text_lib, dev, max_gz=5 << 20, max_blocks=64)
    try:
        for kind in ("zeros", "8mer", "bam", "random"):
            cases, k = [], 0
            for n in sizes:
                if kind == "random" and n > 65280:
                    continue
                data = zlib_data(rng, kind, n)
                level, strat = (0, 1, 6, 9)[k % 4], strategies[(k // 4 + k) % 4]
                k += 1
                cases.append((gm.deflate(data, level=level, strategy=strat), n))
                cases.append((gm.deflate(data, level=6, mem_level=1), n))                  # several dynamic blocks in one member
                cases.append((gm.deflate(data, level=(1, 9)[k % 2], strategy=strategies[k % 4]), n))
            assert D.each(cases, ("zlib", kind)) == (len(cases), 0)
    finally:
        D.close()


# ---- 6: several members -------------------------------------------------------------------------------------------------------
def several_members(text_lib, dev):
    rng = np.random.default_rng(206)
    sizes = (1, 0, 17, 4097, 0, 33)
    datas = [zlib_data(rng, "bam", n) for n in sizes]
    members = [gm.zmember(d) for d in datas]
    members[4] = gm.EOF_MEMBER
    D = Inflater(text_lib, dev)
    try:
        m = D.run(b"".join(members), True, (END, 6, NONE), "several members")
        assert [b[3] for b in m["blocks"]] == [0, 1, 1, 18, 4115, 4115] and m["out_bytes"] == 4148
        # the host form: the bytes come down
        out, s = D.tx.inflate(b"".join(members))
        same_summary(s, m)
        assert out == b"".join(datas)
        bad1 = gm.member(gm.deflate(datas[3])[:-3], 4097)
        bad2 = gm.member(gm.deflate(datas[2]), 16)
        chunk = [members[0], members[2], bad1, members[3], bad2, members[5]]
        m = D.run(b"".join(chunk), True, (END, 6, 2), "two bad members among four good ones")
        try:
            D.tx.inflate(b"".join(chunk))
            raise AssertionError("accepted")
        except tgtext.TgsfError as e:
            assert e.code == -6 and "member 2" in str(e), str(e)
            same_summary(e.summary, m, "the refused call's summary")
        out, s = D.tx.inflate(b"".join(members))                       # a good call straight afterwards
        assert out == b"".join(datas) and s["bad_block"] == NONE
    finally:
        D.close()


# ---- 7: damage ---------------------------------------------------------------------------------------------------------------------
def damage(text_lib, dev):
    rng = np.random.default_rng(207)
    data = zlib_data(rng, "bam", 700)
    z = gm.deflate(data, level=9)
    while len(z) + 26 > 200:
        data = data[:-10]
        z = gm.deflate(data, level=9)
    cases = [(z[:cut], len(data)) for cut in range(len(z))]            # the member cut at every byte: clen shortened, BC rewritten
    cases += [(z, len(data) - 1), (z, len(data) + 1)]                  # ISIZE one less and one more than the truth
    cases.append((gm.deflate(data + b"more"), len(data)))              # the stream goes on after usize bytes
    cases.append((z + b"\x00\xff garbage behind the final block", len(data)))
    D = Inflater(text_lib, dev, max_blocks=256)
    try:
        good, bad = D.each(cases, "damage")
        assert good >= 1 and bad >= len(z) - 8, (good, bad)
    finally:
        D.close()


# ---- 8: the host walk -----------------------------------------------------------------------------------------------------------
def host_walk(text_lib):
    rng = np.random.default_rng(208)
    datas = [zlib_data(rng, "bam", n) for n in (100, 0, 300)]
    members = [gm.zmember(datas[0]), gm.EOF_MEMBER, gm.member(gm.deflate(datas[2]), 300, pre=gm.subfield(b"XY", b"abc"), post=gm.subfield(b"ZZ", b""))]
    gz = b"".join(members)
    ends = np.cumsum([0] + [len(m) for m in members])

    def check(g, final=True, max_blocks=16, max_out=1 << 40, expect=None, what=""):
        m = gm.rule(g, final, max_blocks, max_out)
        if expect is not None:
            assert (m["stop"], m["n_blocks"], m["consumed"]) == tuple(expect), (what, "the model", m["stop"], m["n_blocks"], m["consumed"], expect)
        same_walk(tgtext.bgzf_walk(g, max_blocks, max_out, final, text_lib), m, what)
        return m

    for cut in range(len(gz) + 1):
        k = int(np.searchsorted(ends, cut, side="right")) - 1
        whole = cut == ends[k]
        check(gz[:cut], False, expect=(END, k, int(ends[k])), what=("cut", cut))
        check(gz[:cut], True, expect=(END if whole else IRREGULAR, k, int(ends[k])), what=("final cut", cut))
    a, z = members[0], gm.deflate(datas[2])
    for final in (True, False):
        check(a + gm.member(z, 300, magic=b"\x1f\x8b\x09"), final, expect=(IRREGULAR, 1, len(a)), what="wrong magic")
        check(a + gm.member(z, 300, flg=0), final, expect=(IRREGULAR, 1, len(a)), what="FLG without FEXTRA")
        check(a + gm.member(z, 300, with_bc=False, pre=gm.subfield(b"XY", b"abcdef")), final, expect=(IRREGULAR, 1, len(a)), what="no BC")
        check(a + gm.member(z, 300, bc=12 + 6 + 8 - 2) + a, final, expect=(IRREGULAR, 1, len(a)), what="bsize one below 12 + xlen + 8")
        check(a + gm.member(z, 65537) + a, final, expect=(IRREGULAR, 1, len(a)), what="usize 65537")
    full = gm.zmember(bytes(65536))
    check(a + full + a, True, expect=(END, 3, 2 * len(a) + len(full)), what="usize 65536")
    for mb, exp in ((2, (CAPACITY, 2, int(ends[2]))), (3, (END, 3, len(gz))), (4, (END, 3, len(gz)))):
        check(gz, True, max_blocks=mb, expect=exp, what=("max_blocks", mb))
    for mo, exp in ((399, (CAPACITY, 2, int(ends[2]))), (400, (END, 3, len(gz))), (401, (END, 3, len(gz))), (99, (CAPACITY, 0, 0))):
        check(gz, True, max_out=mo, expect=exp, what=("max_out_bytes", mo))
    at, out, calls = 0, b"", 0                                         # resuming at `consumed`
    while True:
        m = check(gz[at:], True, max_blocks=1)
        out += b"".join(m["data"])
        at += m["consumed"]
        calls += 1
        if m["stop"] != CAPACITY:
            break
    assert out == b"".join(datas) and at == len(gz) and calls == 3


# ---- 9: seeded fuzz ---------------------------------------------------------------------------------------------------------------
def fuzz(text_lib, dev, seed, count, max_size=3000):
    """Members from zlib with drawn parameters and sizes; in half of the chunks one bit of one payload is flipped.  Verdict and
    bytes against the model, either way the model answers.  Returns (flips that made a bad member, flips that left it good)."""
    rng = np.random.default_rng(seed)
    strategies = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED)
    D = Inflater(text_lib, dev)
    broke = kept = 0
    try:
        for i in range(count):
            n = int(rng.integers(1, 7))
            members = []
            for _ in range(n):
                data = zlib_data(rng, ("zeros", "8mer", "bam", "random")[int(rng.integers(0, 4))], int(rng.integers(0, max_size)))
                members.append(gm.zmember(data, level=int(rng.integers(0, 10)), strategy=strategies[int(rng.integers(0, 5))], mem_level=int(rng.integers(1, 10))))
            flip = i % 2 == 1
            if flip:
                k = int(rng.integers(0, n))
                mb = bytearray(members[k])
                clen = len(mb) - 26
                # (bits behind the end of the final block do not count: garbage there leaves the member good)
                tail = b"" if i % 8 != 1 else bytes(rng.integers(0, 256, 3).astype(np.uint8))
                if tail:
                    mb = bytearray(gm.member(bytes(mb[18:18 + clen]) + tail, int.from_bytes(mb[-4:], "little")))
                    at = 18 + clen + int(rng.integers(0, 3))
                else:
                    at = 18 + int(rng.integers(0, clen))
                mb[at] ^= 1 << int(rng.integers(0, 8))
                members[k] = bytes(mb)
            m = D.run(b"".join(members), True, None, (seed, i))
            assert m["stop"] == END and m["n_blocks"] == n
            if flip:
                broke += m["bad_block"] != NONE
                kept += m["bad_block"] == NONE
            else:
                assert m["bad_block"] == NONE
    finally:
        D.close()
    return broke, kept


# ---- 10: the device walk ------------------------------------------------------------------------------------------------------------
def chunks_of(check):
    """The (chunk, final) pairs that a check of tests/bamparity.py feeds its Decoder, taken by running it on a recorder: the
    inputs are that file's own and cannot drift from it."""
    got = []

    class Recorder:
        def __init__(self, *a, **kw):
            pass

        def check(self, bam, final=True, expect=None, what=""):
            got.append((bytes(bam), bool(final)))

        def close(self):
            pass

    real, bp.Decoder = bp.Decoder, Recorder
    try:
        check(None, None)
    finally:
        bp.Decoder = real
    return got


def device_walk(text_lib, dev):
    """bam_walk_device equals tgsf_text_bam_walk word for word: every chunk of bamparity.cut_everywhere and irregular_records,
    `start` on every offset of the first record (the host walk on bam[start:], shifted), max_records on its seam."""
    recs, ends = bp.three()
    bam = b"".join(recs)
    cuts, irregular = chunks_of(bp.cut_everywhere), chunks_of(bp.irregular_records)
    assert len(cuts) == 2 * (len(bam) + 1) and len(irregular) >= 14 and (b"", True) in irregular and max(len(c) for c, _ in cuts + irregular) <= 1024
    chunks = cuts + irregular
    tx = tgtext.TextIndexer(0, 4096, 8, text_lib)
    small = [tgtext.TextIndexer(0, 4096, k, text_lib) for k in (2, 3, 4)]
    try:
        for t in [tx] + small:
            t.reserve_bam(1024)
        _refused(-1, tx.bam_walk_device, 10, start=11, d_bam=dev.ptr(dev.full(16)))
        for chunk, final in chunks:
            d = dev.put(np.frombuffer(chunk + b"\xa5" * 16, np.uint8))
            dev.sync()
            off, stop, consumed = tx.bam_walk_device(len(chunk), 0, final, dev.ptr(d))
            eoff, estop, econs = tgtext.bam_walk(chunk, 8, final, text_lib)
            assert np.array_equal(off, eoff) and (stop, consumed) == (estop, econs), (len(chunk), final, off, eoff, stop, estop)
        d = dev.put(np.frombuffer(bam + b"\xa5" * 16, np.uint8))
        dev.sync()
        for start in range(len(recs[0]) + 1):
            for final in (False, True):
                off, stop, consumed = tx.bam_walk_device(len(bam), start, final, dev.ptr(d))
                eoff, estop, econs = tgtext.bam_walk(bam[start:], 8, final, text_lib)
                assert np.array_equal(off, eoff + np.uint64(start)) and (stop, consumed) == (estop, econs + start), (start, final)
        for t, k in zip(small, (2, 3, 4)):
            off, stop, consumed = t.bam_walk_device(len(bam), 0, True, dev.ptr(d))
            eoff, estop, econs = tgtext.bam_walk(bam, k, True, text_lib)
            assert np.array_equal(off, eoff) and (stop, consumed) == (estop, econs) and stop == (CAPACITY if k == 2 else END)
    finally:
        for t in [tx] + small:
            t.close()


# ---- 11: compressed BAM in, clean text out -----------------------------------------------------------------------------------------
def _same_bam(s, m, what=""):
    bp.same_summary(s["bam"], m, what)


def golden_compressed(lib, text_lib, dev, golden_dir, name):
    """tests/golden/<name>.in.bam as it is on disk through bgzf_bam_start and bgzf_bam_filter: the reference's own output file,
    records, fragments and tallies against the oracle, index and text as bam_decode's on zlib-inflated bytes; once in one
    call, once resumed by (next_gz, next_skip) with buffers small enough to need several calls."""
    from oracle import orc
    from tests import textparity
    from tgsfilter_amd import capi
    case, at, chunk, m = bp.golden_model(golden_dir, name)
    gz = open(os.path.join(golden_dir, name + ".in.bam"), "rb").read()
    n = m["n_records"]
    whole = gm.rule(gz)
    assert whole["stop"] == END and whole["bad_block"] == NONE and b"".join(whole["data"]) == case.bam
    D = bp.Decoder(text_lib, dev, len(case.bam), n)
    D.tx.reserve_bgzf(len(gz), whole["n_blocks"])
    p = bp.golden_params(case, m)
    ctx = capi.Context(p, 0, lib)
    try:
        goff, skip = D.tx.bgzf_bam_start(gz)
        b0 = max(i for i, b in enumerate(whole["blocks"]) if b[3] <= at and (b[2] or b[3] < at))
        assert skip == at - whole["blocks"][b0][3] and gz[goff:goff + 4] == b"\x1f\x8b\x08\x04"
        shift = whole["blocks"][b0][3]                                 # inflated bytes in front of that member
        dev.fill(D.text_ptr, D.room, 0xA5)
        idx, s = D.tx.bgzf_bam_decode(gz[goff:], skip)
        mm = dict(m, consumed=m["consumed"] + at - shift)
        _same_bam(s, mm, name)
        bp.same_index(idx, m, name)
        bp.same_text(dev.peek(D.text_ptr, D.room), m, name)
        assert (s["gz"]["stop"], s["gz"]["consumed"], s["gz"]["bad_block"], s["next_gz"], s["next_skip"]) == (END, len(gz) - goff, NONE, len(gz) - goff, 0)
        host = np.frombuffer(m["text"] + b"\0" * 64, dtype=np.uint8)
        er, ef, ec = orc.filter_batch(p, host, host, m["index"]["seq_off"], m["index"]["len"], n_bins=ctx.n_bins, qual_offsets=m["index"]["qual_off"])
        idx, s, r1, f1 = D.tx.bgzf_bam_submit(ctx, gz[goff:], skip)
        _same_bam(s, mm, name)
        bp.same_index(idx, m, name)
        textparity.same_results((r1, f1, ctx.counters()), (er, ef, ec))
        fr = top.frag_room(m["text_bytes"], n)
        D.tx.reserve_output(fr, top.out_room(m["text_bytes"], fr))
        out, rec_end, so, si = D.tx.bgzf_bam_filter(ctx, gz[goff:], skip)
        assert out == case.ref_out and len(out) > 1000, name
        top.same_output((out, rec_end, so), top.expected(m["text"], m["index"], er, ef, True), name)
    finally:
        ctx.close()
        D.close()
    # several calls: room for a few members and a part of the records a call
    longest = int(max(np.diff(np.concatenate([bm_offsets(chunk), [len(chunk)]]))))
    D = bp.Decoder(text_lib, dev, 2 * 65536 + longest, max(n // 5, 2))
    D.tx.reserve_bgzf(len(gz), 3)
    fr = top.frag_room(D.tx.max_bytes, D.tx.max_records)
    D.tx.reserve_output(fr, top.out_room(D.tx.max_bytes, fr))
    ctx = capi.Context(p, 0, lib)
    try:
        out, calls, records = b"", 0, 0
        while True:
            part, _, so, si = D.tx.bgzf_bam_filter(ctx, gz[goff:], skip)
            out += part
            records += si["bam"]["n_records"]
            calls += 1
            assert si["bam"]["n_records"] >= 1 or si["next_gz"] > 0 or si["bam"]["stop"] == END, si
            goff, skip = goff + si["next_gz"], si["next_skip"]
            if goff == len(gz) or calls > 400:
                break
        assert out == case.ref_out and records == n and calls >= 3, (calls, records, n)
    finally:
        ctx.close()
        D.close()


def bm_offsets(chunk):
    from tests import bammodel
    return np.array(bammodel.walk(chunk, True, 1 << 30)[0][:-1], dtype=np.int64)


def compressed_seams(lib, text_lib, dev):
    """Members of 1, 31, 100 and 0xFF00 bytes under records that span several of them; skip on every offset of a small first
    member; a record larger than the object; a bad member; a quality byte of 233 through the compressed path."""
    from tests import bamio, bammodel, textparity
    from tgsfilter_amd import capi
    rng = np.random.default_rng(211)
    recs = [bp.rnd_record(rng, 5, 40, aux=3, qmax=60), bp.rnd_record(rng, 7, 300, aux=9, qmax=60), bp.rnd_record(rng, 0, 1, qmax=60), bp.rnd_record(rng, 9, 77, qmax=60)]
    bam = b"".join(recs)
    D = bp.Decoder(text_lib, dev, 4096, 8)
    D.tx.reserve_bgzf(1 << 16, 1024)
    p = textparity.params_for("hifi", bammodel.reads_of(bam), bp.text_room(len(bam)), min_q=0.0, min_len=1)
    p.max_batch_reads = 8
    ctx = capi.Context(p, 0, lib)
    try:
        m = D.model(bam)
        assert (m["stop"], m["n_records"]) == (END, 4)
        for block in (1, 31, 100, 0xFF00):
            gz = bamio.bgzf(bam, block)
            assert gm.rule(gz)["n_blocks"] == -(-len(bam) // block) + 1
            dev.fill(D.text_ptr, D.room, 0xA5)
            idx, s = D.tx.bgzf_bam_decode(gz)
            _same_bam(s, m, ("block", block))
            bp.same_index(idx, m, ("block", block))
            bp.same_text(dev.peek(D.text_ptr, D.room), m, ("block", block))
            assert (s["next_gz"], s["next_skip"], s["gz"]["stop"]) == (len(gz), 0, END)
        for skip in range(41):                                         # junk in front of the records, in a first member of 40 bytes
            inflated = b"\xee" * skip + bam
            gz = gm.zmember(inflated[:40]) + gm.zmember(inflated[40:]) + gm.EOF_MEMBER
            idx, s = D.tx.bgzf_bam_decode(gz, skip)
            _same_bam(s, dict(m, consumed=m["consumed"] + skip), ("skip", skip))
            bp.same_index(idx, m, ("skip", skip))
        assert "skip" in _refused(-1, D.tx.bgzf_bam_decode, gm.zmember(bam), len(bam) + 1)
        # not final: the last record is cut; the next call begins at the member that holds its first byte
        gz = bamio.bgzf(bam[:-5], 100)[:-28]
        idx, s = D.tx.bgzf_bam_decode(gz, 0, final=False)
        cut = len(bam) - len(recs[3])
        assert (s["bam"]["n_records"], s["bam"]["stop"], s["bam"]["consumed"]) == (3, END, cut)
        assert (s["next_gz"], s["next_skip"]) == (gm.rule(gz, False)["blocks"][cut // 100][0] - 18, cut % 100)
        assert gm.rule(gz[s["next_gz"]:], False)["data"][0][s["next_skip"]:s["next_skip"] + 4] == recs[3][:4]
        # a record larger than the object
        big = bp.Decoder(text_lib, dev, 4096, 8, max_bytes=500)
        big.tx.reserve_bgzf(1 << 16, 16)
        try:
            idx, s = big.tx.bgzf_bam_decode(gm.zmember(recs[1] + recs[0]))
            assert (s["bam"]["stop"], s["bam"]["n_records"], s["bam"]["consumed"], s["next_gz"], s["next_skip"]) == (CAPACITY, 0, 0, 0, 0)
        finally:
            big.close()
        # members cut short by max_bam_bytes that hold no whole record: the call says CAPACITY, not "to be continued"
        tiny = bp.Decoder(text_lib, dev, 64, 8)
        tiny.tx.reserve_bgzf(1 << 16, 16)
        try:
            idx, s = tiny.tx.bgzf_bam_decode(gm.zmember(bam[:64]) + gm.zmember(bam[64:]) + gm.EOF_MEMBER)
            assert (s["gz"]["stop"], s["gz"]["n_blocks"], s["gz"]["out_bytes"]) == (CAPACITY, 1, 64) and len(recs[0]) > 64
            assert (s["bam"]["stop"], s["bam"]["n_records"], s["bam"]["consumed"], s["next_gz"], s["next_skip"]) == (CAPACITY, 0, 0, 0, 0)
        finally:
            tiny.close()
        # a bad member: the call names it, the filter has not run, a good call follows
        good = gm.zmember(bam[:100]) + gm.zmember(bam[100:])
        bad = gm.zmember(bam[:100]) + gm.member(gm.deflate(bam[100:])[:-4], len(bam) - 100)
        D.tx.reserve_output(64, 1 << 16)
        before = ctx.counters().copy()
        try:
            D.tx.bgzf_bam_filter(ctx, bad)
            raise AssertionError("accepted")
        except tgtext.TgsfError as e:
            assert e.code == -6 and "member 1" in str(e), str(e)
            assert e.in_summary["gz"]["bad_block"] == 1 and e.in_summary["gz"]["n_blocks"] == 2 and e.in_summary["bam"]["n_records"] == 0 and e.summary["n_bytes"] == 0
        assert np.array_equal(ctx.counters(), before)
        out = D.tx.bgzf_bam_filter(ctx, good)
        want = D.tx.bam_filter(ctx, bam)
        assert out[0] == want[0] and len(out[0]) > 500 and out[3]["bam"]["n_records"] == 4, (len(out[0]), len(want[0]))
        # a quality byte of 233 through the compressed path
        q = bp.record(b"first_bad\0", np.arange(9) % 16, b"\1\2\xe9\3\4\5\6\7\x08")
        msg = _refused(-6, D.tx.bgzf_bam_filter, ctx, gm.zmember(recs[0] + q[:20]) + gm.zmember(q[20:] + recs[3]))
        assert "first_bad" in msg and "quality" in msg
        out = D.tx.bgzf_bam_filter(ctx, good)
        assert out[0] == want[0]
    finally:
        ctx.close()
        D.close()


# ---- 12: chaining into the text index --------------------------------------------------------------------------------------------
def into_the_text_index(text_lib, dev, golden_dir, name="hifi_auto"):
    """A bgzip'ed copy of a FASTQ golden: the host form inflates into the object's text buffer; inflate_device aimed at the
    same buffer, then tgsf_text_index_device: the index equals the plain text's."""
    text = gzip.open(os.path.join(golden_dir, name + ".in.fq.gz"), "rb").read()[:300_000]
    text = text[:text.rfind(b"\n@") + 1]
    gz = b"".join(gm.zmember(text[i:i + 0xFF00]) for i in range(0, len(text), 0xFF00)) + gm.EOF_MEMBER
    recs, consumed, stop = textmodel.rule(text, False, True)
    want = textmodel.expected_index(recs)
    assert stop == tgtext.END and consumed == len(text) and len(recs) > 5
    tx = tgtext.TextIndexer(0, len(text), len(recs), text_lib)
    try:
        tx.reserve_bgzf(len(gz), 16)
        plain_idx, plain_s = tx.index(text)
        blocks, wstop, consumed, out_bytes = tgtext.bgzf_walk(gz, 16, lib_path=text_lib)
        assert (wstop, consumed, out_bytes) == (END, len(gz), len(text))
        b = tx.buffers()
        dev.fill(b.text, bp.buffer_bytes(len(text)), 0xA5)
        d_gz = dev.put(np.frombuffer(gz + bytes(-len(gz) % 16), np.uint8))
        dev.sync()
        tx.inflate_device(len(gz), blocks, wstop, b.text, len(text), d_gz=dev.ptr(d_gz))
        tx.index_device(len(text))
        idx, s = tx.fetch()
        assert s == dict(plain_s, device_ms=s["device_ms"]) and s["n_records"] == len(recs)
        for f in ("seq_off", "qual_off", "len", "name_off", "name_len"):
            assert np.array_equal(getattr(idx, f), want[f]) and np.array_equal(getattr(idx, f), getattr(plain_idx, f)), f
        assert dev.peek(b.text, len(text)).tobytes() == text
        out, gs = tx.inflate(gz)                                       # the host form leaves the same bytes there
        assert out == text and gs["n_blocks"] == len(blocks) and gs["consumed"] == len(gz)
    finally:
        tx.close()


# ---- 13: refusals, row by row -------------------------------------------------------------------------------------------------------
def refusals(text_lib, dev):
    rng = np.random.default_rng(213)
    datas = [zlib_data(rng, "bam", n) for n in (500, 900, 0, 77)]
    gz = b"".join(gm.zmember(d) for d in datas)
    whole = b"".join(datas)
    tx = tgtext.TextIndexer(0, 4096, 8, text_lib)
    L = tgtext.load(text_lib)
    blocks, stop, consumed, out_bytes = tgtext.bgzf_walk(gz, 8, lib_path=text_lib)
    d_out = dev.full(len(whole) + 32, 0xA5)
    d_gz = dev.put(np.frombuffer(gz + bytes(-len(gz) % 16 + 16), np.uint8))

    def good():
        out, s = tx.inflate(gz)
        assert out == whole and (s["n_blocks"], s["stop"], s["consumed"], s["out_bytes"], s["bad_block"]) == (4, END, len(gz), len(whole), NONE)
        dev.sync()
        tx.inflate_device(len(gz), blocks, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz), stream=dev.stream)
        dev.sync()
        tx.fetch(want_index=False)
        assert dev.get(d_out)[:len(whole)].tobytes() == whole

    try:
        assert "reserve" in _refused(-1, tx.inflate, gz)                                               # before reserve
        assert "reserve" in _refused(-1, tx.inflate_device, len(gz), blocks, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz))
        _refused(-1, tx.reserve_bgzf, 0, 4)
        tx.reserve_bgzf(len(gz), 4)
        tx.index(b"@r\nACGT\n+\nIIII\n")
        good()
        assert "already" in _refused(-1, tx.reserve_bgzf, len(gz), 4)                                  # a second reserve
        good()
        assert "reserved for" in _refused(-4, tx.inflate, gz + gm.EOF_MEMBER)                          # n_bytes over the reservation
        good()
        more = np.concatenate([blocks, blocks[-1:]])                                                    # n_blocks over max_blocks
        assert "reserved for 4" in _refused(-4, tx.inflate_device, len(gz), more, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz))
        good()
        s = tgtext.BgzfSummary()                                                                        # null arguments
        g = np.frombuffer(gz, np.uint8)
        assert L.tgsf_text_bgzf_inflate(tx.h, None, 10, 1, None, 0, C.byref(s)) == -1
        assert L.tgsf_text_bgzf_inflate(tx.h, g.ctypes.data, len(gz), 1, None, 0, None) == -1
        assert L.tgsf_text_bgzf_inflate_device(tx.h, dev.ptr(d_gz), len(gz), None, 4, 0, dev.ptr(d_out), len(whole), None, None) == -1
        assert L.tgsf_text_bgzf_inflate_device(tx.h, dev.ptr(d_gz), len(gz), blocks.ctypes.data, 4, 0, None, len(whole), None, None) == -1
        assert L.tgsf_text_bgzf_walk(None, 10, 1, 4, 100, None, None, None, None, None) == -1
        assert len(L.tgsf_text_last_error(tx.h)) > 10
        good()
        assert "final" in _refused(-1, tx.inflate, gz, final=2)                                        # final of 2
        _refused(-1, tgtext.bgzf_walk, gz, 8, final=2, lib_path=text_lib)
        good()
        assert "room for" in _refused(-4, tx.inflate_device, len(gz), blocks, stop, dev.ptr(d_out), len(whole) - 1, d_gz=dev.ptr(d_gz))   # out_capacity below out_bytes
        good()
        assert "16-byte" in _refused(-1, tx.inflate_device, len(gz), blocks, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz) + 4)
        lie = blocks.copy()
        lie["clen"][3] = 60000                                                                          # a table that is not the walk's
        assert "member 3" in _refused(-1, tx.inflate_device, len(gz), lie, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz))
        wide = tgtext.TextIndexer(0, 4096, 8, text_lib)                                                  # a stream longer than the device form takes
        try:
            wide.reserve_bgzf(1 << 18, 2)
            table = np.array([(16, 131073, 10, 0)], dtype=tgtext.BGZF_BLOCK_DTYPE)
            assert "member 0" in _refused(-1, wide.inflate_device, 1 << 18, table, END, dev.ptr(d_out), 10, d_gz=dev.ptr(d_gz))
        finally:
            wide.close()
        lie = blocks.copy()
        lie["out"][2] += 1
        assert "member 2" in _refused(-1, tx.inflate_device, len(gz), lie, stop, dev.ptr(d_out), len(whole), d_gz=dev.ptr(d_gz))
        good()
        out, s = tx.inflate(gz, out_capacity=1400)                                                      # the host form stops where the room ends
        assert (s["stop"], s["n_blocks"], s["out_bytes"]) == (CAPACITY, 3, 1400) and out == whole[:1400]
        assert "does not fit" in _refused(-4, tx.inflate, gz, out_capacity=499)
        good()
    finally:
        tx.close()


# ---- 14: the device form on a caller's stream, two objects on two threads ----------------------------------------------------------
def two_threads(text_lib, make_dev):
    errors = []

    def work(k):
        try:
            b, g = fuzz(text_lib, make_dev(), 1400 + k, 40)
            assert b + g == 20
        except BaseException as e:              # noqa: BLE001 -- reported by the asserting thread
            errors.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
