"""Shared checks of the BGZF output side of libtgsf_text (include/tgsf_text.h, tgsf_text_bgzf_deflate*, _crc_device, _verify,
*_filter_bgzf): a backend (the HIP build on the GPU box, the serial emulation of the same kernels elsewhere) against
tests/gzoutmodel.py, which asks zlib and gzip.  Every output is checked every way: gzip.decompress, the model's per-member
check, member_end and the summary word for word, the stricter host walk, two calls with identical bytes, canaries around the
output, and the project's own inflate and CRC check on the way back.  tests/test_gzout_emul.py and tests/test_gzout_gpu.py
run them."""
from __future__ import annotations

import ctypes as C
import gzip
import os
import threading
import zlib

import numpy as np

from tests import bamparity as bp, bgzfmodel as gm, gzoutmodel as zm, hostmodel, textoutparity as top, textparity
from tgsfilter_amd import capi, synth, text as tgtext

END, CAPACITY, NONE = zm.END, zm.CAPACITY, gm.NONE
HostMem, TorchMem = bp.HostMem, bp.TorchMem
_refused = top._refused
MEMBER = zm.MEMBER
FRONT = 16                                                             # canary in front of the output (which is 16-byte aligned)
GOLDEN_TEXTS = ("ont_auto", "hifi_auto", "hifi_bam", "ont_fasta", "hifi_zoo", "odd_bytes", "hifi_phred64_auto")


def golden_text(golden_dir, name):
    return gzip.open(os.path.join(golden_dir, name + ".out.fq.gz"), "rb").read()


class Deflater:
    """One TextIndexer reserved for both BGZF sides; run() deflates a text by the device form into a caller's buffer between
    canaries, twice, and checks the output every way."""

    def __init__(self, text_lib, dev, max_in=1 << 20):
        self.dev, self.lib = dev, text_lib
        self.max_in = max_in
        self.room = zm.bound(max_in, True)
        self.tx = tgtext.TextIndexer(0, max(max_in, 64), 16, text_lib)
        self.tx.reserve_bgzf_out(max_in, self.room)
        self.tx.reserve_bgzf(self.room, max_in // MEMBER + 2)

    def run(self, text, eof=True, what="", capacity=None):
        text = bytes(text)
        dev, n, tx = self.dev, len(text), self.tx
        assert zm.cuts(n) == [(i * MEMBER, min((i + 1) * MEMBER, n)) for i in range((n + MEMBER - 1) // MEMBER)]
        cap = zm.bound(n, eof) if capacity is None else capacity
        d_in = dev.put(np.frombuffer(text, np.uint8)) if n else dev.full(16, 0xA5)
        n_ends = (n + MEMBER - 1) // MEMBER + 1
        outs = []
        for _ in range(2):                                             # two calls: identical bytes
            d_out = dev.full(FRONT + cap + 64, 0xA5)
            d_end = dev.full(8 * (n_ends + 2), 0xA5)
            d_sum = dev.full(16 + 40 + 16, 0xA5)
            dev.sync()
            tx.deflate_device(n, eof, d_in=dev.ptr(d_in), d_out=dev.ptr(d_out) + FRONT, out_capacity=cap, d_member_end=dev.ptr(d_end),
                              d_summary=dev.ptr(d_sum) + 16, stream=dev.stream)
            dev.sync()
            raw = dev.get(d_sum)
            assert (raw[:16] == 0xA5).all() and (raw[56:] == 0xA5).all(), (what, "the summary's canaries")
            s = tgtext.GzOutSummary.from_buffer_copy(raw[16:56].tobytes()).as_dict()
            assert s["stop"] == END and s["n_bytes"] <= cap, (what, s)
            got = dev.get(d_out)
            k = s["n_bytes"]
            assert (got[:FRONT] == 0xA5).all() and (got[FRONT + k:] == 0xA5).all(), (what, "written outside the output")
            ends = dev.get(d_end).view(np.uint64)
            assert (ends[s["n_members"]:] == 0xA5A5A5A5A5A5A5A5).all(), (what, "written behind member_end")
            outs.append((got[FRONT:FRONT + k].tobytes(), ends[:s["n_members"]].copy(), s, d_out))
        gz, ends, s, d_out = outs[-1]
        assert outs[0][0] == gz, (what, "two calls, two outputs")
        stored = zm.check(text, gz, eof, ends, s, what)
        # the stricter host walk accepts every member
        blocks, stop, consumed, out_bytes = tgtext.bgzf_walk(gz, len(ends) + 1, lib_path=self.lib)
        assert (len(blocks), stop, consumed, out_bytes) == (len(ends), END, len(gz), n), (what, "the walk", len(blocks), stop, consumed, out_bytes)
        # the round trip: the project's own inflate, and its CRC check, on the bytes where they are
        d_back = dev.full(n + 32, 0xA5)
        d_bad = dev.full(16, 0xA5)
        dev.sync()
        tx.inflate_device(len(gz), blocks, stop, dev.ptr(d_back), n, d_gz=dev.ptr(d_out) + FRONT, stream=dev.stream)
        tx.crc_device(blocks, dev.ptr(d_bad), d_gz=dev.ptr(d_out) + FRONT, d_inflated=dev.ptr(d_back), stream=dev.stream)
        dev.sync()
        back = dev.get(d_back)
        assert back[:n].tobytes() == text and (back[n:] == 0xA5).all(), (what, "the round trip")
        bad = dev.get(d_bad)
        assert bad[:4].view(np.uint32)[0] == NONE and (bad[4:] == 0xA5).all(), (what, "the CRC check", bad[:4])
        return gz, ends, s, stored

    def close(self):
        self.tx.close()


# ---- 1: lengths --------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER, 2 * MEMBER + 1)


def lengths(text_lib, dev):
    rng = np.random.default_rng(301)
    fq = zm.fastq_like(rng, 2 * MEMBER + 1)
    D = Deflater(text_lib, dev, 1 << 18)
    try:
        for eof in (False, True):
            gz, ends, s, _ = D.run(b"", eof, ("empty", eof))
            assert gz == (zm.EOF_MEMBER if eof else b"") and s["n_members"] == int(eof)
        for n in LENGTHS[1:]:
            for text in (fq[:n], b"G" * n):
                gz, ends, s, _ = D.run(text, n % 2 == 0, ("length", n, text[:1]))
                assert s["n_members"] == (n + MEMBER - 1) // MEMBER + (n % 2 == 0)
    finally:
        D.close()


# ---- 2: code shapes ------------------------------------------------------------------------------------------------------------
def code_shapes(text_lib, dev):
    rng = np.random.default_rng(302)
    D = Deflater(text_lib, dev, 1 << 18)
    try:
        gz, _, s, stored = D.run(b"\n" * MEMBER, True, "one distinct byte")
        assert stored == 0 and len(gz) < MEMBER // 7                   # one bit a byte
        D.run(zm.from_freqs(rng, [65, 67], [40000, 9]), True, "two distinct bytes")
        D.run(zm.from_freqs(rng, [0, 255], [1, 1]), False, "two bytes")
        # Fibonacci frequencies over 24 symbols: a Huffman tree over them is as deep as its symbols are many (ties broken the
        # deep way); one step steeper and every Huffman tree is: the code of 15 bits at most is not the Huffman code
        fib = zm.fibonacci(24)
        for syms, freqs, shallow, what in ((range(40, 64), fib[:22], False, "fibonacci, 22 of 24 in one member"),
                                           (range(100, 120), zm.steeper_than_fibonacci(20), True, "steeper than fibonacci")):
            text = zm.from_freqs(rng, list(syms)[:len(freqs)], freqs)
            assert len(text) <= MEMBER and zm.huffman_depth(zm.member_freqs(text)[0], shallow) > 15, what
            _, _, _, stored = D.run(text, True, what)
            assert stored == 0
        text = zm.from_freqs(rng, list(range(40, 64)), fib)            # all 24: two members
        assert max(zm.huffman_depth(f, False) for f in zm.member_freqs(text)) > 15
        D.run(text, True, "fibonacci over 24 symbols")
        # all 256 byte values uniformly: nothing to gain, the member is stored
        text = zm.from_freqs(rng, list(range(256)), [MEMBER // 256] * 256)
        gz, ends, s, stored = D.run(text, False, "uniform")
        assert len(text) == MEMBER and stored == 1 == s["stored"] and len(gz) == MEMBER + 5 + zm.FRAME
        # either side of the break-even: 128 byte values uniformly, from a text no dynamic block can describe in less than
        # itself (every byte value once: 128 code lengths and 7 bits a byte) to one where 7 bits a byte win by hundreds of bytes
        kinds = set()
        for reps in (1, 2, 4, 6, 8, 9, 10, 12, 16, 32):
            text = zm.from_freqs(rng, list(range(64, 192)), [reps] * 128)
            _, _, _, stored = D.run(text, True, ("break-even", reps))
            kinds.add(stored)
            assert (reps != 1 or stored == 1) and (reps != 32 or stored == 0), (reps, stored)
        assert kinds == {0, 1}
        D.run(bytes(rng.integers(128, 256, 3000).astype(np.uint8)), True, "bytes of 128 and above")
        D.run(zm.from_freqs(rng, [128, 255, 200], [5000, 3, 70]), True, "skewed bytes of 128 and above")
    finally:
        D.close()


# ---- 3: bit seams ---------------------------------------------------------------------------------------------------------------
def bit_seams(text_lib, dev, positions=tuple(range(201))):
    rng = np.random.default_rng(303)
    D = Deflater(text_lib, dev, 1 << 16)
    try:
        n = 1500
        for p in list(positions) + [n - 1]:                            # the rare byte has the longest code: on every lane piece and dword seam
            t = bytearray(b"A" * n)
            t[p] = ord("#")
            D.run(bytes(t), p % 2 == 0, ("rare byte at", p))
        alphabets = (zm.fastq_like(rng, 2200), zm.from_freqs(rng, [65, 67], [2000, 200]),
                     zm.from_freqs(rng, list(range(33, 49)), [5 * (1 << (i // 2)) for i in range(16)]))
        for a, text in enumerate(alphabets):
            assert len(text) >= 2064, (a, len(text))
            for n in range(2000, 2064):                                # the block ends on varied bit positions
                D.run(text[:n], False, ("alphabet", a, "length", n))
    finally:
        D.close()


# ---- 4: address seams, capacity, canaries -----------------------------------------------------------------------------------------
def address_seams(text_lib, dev):
    rng = np.random.default_rng(304)
    text = zm.fastq_like(rng, 17 * MEMBER + 4321)
    D = Deflater(text_lib, dev, len(text))
    try:
        gz, ends, s, _ = D.run(text, True, "18 members")
        res = {b % 16 for b in zm.starts(ends)}
        assert s["n_members"] == 19 and len(res) >= 8 and any(r % 2 for r in res), ("the members' starts do not cover the residues", sorted(res))
        D.run(text, True, "capacity exactly n_bytes", capacity=len(gz))
        # one byte short: CAPACITY, the size that is needed, and not a byte written anywhere
        dev_, tx = D.dev, D.tx
        d_in = dev_.put(np.frombuffer(text, np.uint8))
        d_out = dev_.full(FRONT + len(gz) + 64, 0xA5)
        d_end = dev_.full(8 * 32, 0xA5)
        d_sum = dev_.full(40, 0xA5)
        dev_.sync()
        tx.deflate_device(len(text), True, d_in=dev_.ptr(d_in), d_out=dev_.ptr(d_out) + FRONT, out_capacity=len(gz) - 1, d_member_end=dev_.ptr(d_end),
                          d_summary=dev_.ptr(d_sum), stream=dev_.stream)
        dev_.sync()
        sc = tgtext.GzOutSummary.from_buffer_copy(dev_.get(d_sum).tobytes()).as_dict()
        assert (sc["stop"], sc["n_bytes"], sc["in_bytes"], sc["n_members"], sc["stored"]) == (CAPACITY, len(gz), len(text), 19, 0), sc
        assert (dev_.get(d_out) == 0xA5).all() and (dev_.get(d_end) == 0xA5).all(), "CAPACITY, and something was written"
        # the host form: the same bytes; CAPACITY comes down as TGSF_E_CAPACITY with the summary alone
        hgz, hends, hs = tx.deflate(text)
        assert hgz == gz and np.array_equal(hends, ends) and {k: hs[k] for k in hs if k != "device_ms"} == {k: s[k] for k in s if k != "device_ms"}
        out = np.full(len(gz) + 16, 0xA5, np.uint8)
        try:
            tx.deflate(text, out=out, out_capacity=len(gz) - 1)
            raise AssertionError("accepted")
        except capi.TgsfError as e:
            assert e.code == -4 and "room for" in str(e) and e.summary["stop"] == CAPACITY and e.summary["n_bytes"] == len(gz), (e.code, str(e), e.summary)
        assert (out == 0xA5).all()
        hgz, _, _ = tx.deflate(text, out=out, out_capacity=len(gz))
        assert hgz == gz and (out[len(gz):] == 0xA5).all()
    finally:
        D.close()


# ---- 5: the size, on the goldens' output texts -------------------------------------------------------------------------------------
def golden_size(text_lib, dev, golden_dir, name):
    """At most 1.05 times what zlib writes for the same cuts with Z_HUFFMAN_ONLY, 26 bytes of framing a member."""
    text = golden_text(golden_dir, name)
    assert len(text) > 2 * MEMBER, name
    D = Deflater(text_lib, dev, len(text))
    try:
        gz, ends, s, stored = D.run(text, False, name)
        ref = zm.huffman_only_size(text)
        print("size %s: %d bytes of text, %d compressed, zlib Z_HUFFMAN_ONLY %d, ratio %.4f, share %.4f, stored %d" % (
            name, len(text), len(gz), ref, len(gz) / ref, len(gz) / len(text), stored))
        assert len(gz) <= 1.05 * ref, (name, len(gz), ref, len(gz) / ref)
    finally:
        D.close()


# ---- 6: a seeded fuzz over length, alphabet size and skew --------------------------------------------------------------------------
def fuzz(text_lib, dev, seed, count, max_size=3 * MEMBER):
    rng = np.random.default_rng(seed)
    D = Deflater(text_lib, dev, max_size)
    stored = 0
    try:
        for i in range(count):
            n = int(rng.integers(1, max_size + 1)) if i % 4 else int(rng.integers(1, 300))
            k = int(rng.integers(1, 257))
            skew = float(rng.choice([0.0, 0.3, 1.0, 2.5]))
            w = 1.0 / np.arange(1, k + 1) ** skew
            syms = rng.permutation(256)[:k].astype(np.uint8)
            text = syms[rng.choice(k, n, p=w / w.sum())].tobytes()
            stored += D.run(text, bool(i % 2), ("fuzz", seed, i, n, k, skew))[3]
    finally:
        D.close()
    return stored


# ---- 7: the goldens through the composed calls --------------------------------------------------------------------------------------
def _gz_agrees(text, gz, sg, so, eof, what):
    assert gzip.decompress(gz) == text if gz else text == b"", (what, "gunzip")
    zm.check(text, gz, eof, None, sg, what)
    assert so["n_bytes"] == len(text) and so["stop"] == END, (what, so)


def golden_filter_bgzf(lib, text_lib, golden_dir, name):
    """A text golden through filter_bgzf: the gunzipped output is the reference's output file, byte for byte."""
    case = hostmodel.GoldenCase(golden_dir, name)
    text = textparity.fastq_of(case.reads)
    p = case.params()
    p.max_batch_reads = len(case.reads)
    p.max_batch_bases = 2 * len(text) + 64 * len(case.reads) + 4096
    p.max_read_len = max(len(r[1]) for r in case.reads)
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(text), len(case.reads), text_lib)
    try:
        fr = top.frag_room(len(text), len(case.reads))
        tx.reserve_output(fr, top.out_room(len(text), fr))
        tx.reserve_bgzf_out(top.out_room(len(text), fr))
        for eof in (True, False):
            gz, sg, so, si = tx.filter_bgzf(ctx, text, eof=eof)
            assert si["n_records"] == len(case.reads) and si["stop"] == END
            _gz_agrees(case.ref_out, gz, sg, so, eof, (name, eof))
        plain = tx.filter(ctx, text)
        assert plain[0] == case.ref_out and {k: v for k, v in plain[2].items() if k != "device_ms"} == {k: v for k, v in so.items() if k != "device_ms"}
        # a null gz_summary: the bytes are the same
        whole = tx.filter_bgzf(ctx, text, eof=False, want_gz_summary=False)
        assert whole[1] is None and whole[0][:len(gz)] == gz
    finally:
        tx.close()
        ctx.close()


def golden_bam_bgzf(lib, text_lib, dev, golden_dir, name):
    """tests/golden/<name>.in.bam, inflated and as it is on disk, through bam_filter_bgzf and bgzf_bam_filter_bgzf."""
    case, at, chunk, m = bp.golden_model(golden_dir, name)
    on_disk = open(os.path.join(golden_dir, name + ".in.bam"), "rb").read()
    n = m["n_records"]
    D = bp.Decoder(text_lib, dev, len(case.bam), n)
    D.tx.reserve_bgzf(len(on_disk), len(gm.walk(on_disk)[0]))
    fr = top.frag_room(m["text_bytes"], n)
    D.tx.reserve_output(fr, top.out_room(m["text_bytes"], fr))
    D.tx.reserve_bgzf_out(top.out_room(m["text_bytes"], fr))
    ctx = capi.Context(bp.golden_params(case, m), 0, lib)
    try:
        gz, sg, so, si = D.tx.bam_filter_bgzf(ctx, chunk)
        bp.same_summary(si, m, name)
        _gz_agrees(case.ref_out, gz, sg, so, True, (name, "bam"))
        assert len(case.ref_out) > 1000
        goff, skip = D.tx.bgzf_bam_start(on_disk)
        gz2, sg2, so2, si2 = D.tx.bgzf_bam_filter_bgzf(ctx, on_disk[goff:], skip)
        assert gz2 == gz and si2["bam"]["n_records"] == n and si2["gz"]["bad_block"] == NONE, (name, "as it is on disk")
        _gz_agrees(case.ref_out, gz2, sg2, so2, True, (name, "bgzf bam"))
        gz3 = D.tx.bgzf_bam_filter_bgzf(ctx, on_disk[goff:], skip, eof=False, fastq_out=False)
        fa = D.tx.bgzf_bam_filter(ctx, on_disk[goff:], skip, fastq_out=False)[0]
        _gz_agrees(fa, gz3[0], gz3[1], gz3[2], False, (name, "FASTA out"))
    finally:
        ctx.close()
        D.close()


# ---- 8: refusals row by row, and a good call straight afterwards -------------------------------------------------------------------
def refusals(lib, text_lib, dev):
    rng = np.random.default_rng(308)
    text = zm.fastq_like(rng, 70000)
    L = tgtext.load(text_lib)
    tx = tgtext.TextIndexer(0, len(text), 64, text_lib)
    d_in = dev.put(np.frombuffer(text, np.uint8))
    d_out = dev.full(zm.bound(len(text), True) + 16, 0xA5)
    out = np.zeros(zm.bound(len(text), True), np.uint8)

    def good():
        gz, ends, s = tx.deflate(text)
        zm.check(text, gz, True, ends, s, "a good call")
        dev.sync()
        tx.deflate_device(len(text), True, d_in=dev.ptr(d_in), d_out=dev.ptr(d_out), out_capacity=len(gz), stream=dev.stream)
        dev.sync()
        tx.fetch(want_index=False)
        assert dev.get(d_out)[:len(gz)].tobytes() == gz

    try:
        assert L.tgsf_text_bgzf_bound(0, 0) == 0 and L.tgsf_text_bgzf_bound(0, 1) == 28 and L.tgsf_text_bgzf_bound(MEMBER + 1, 1) == MEMBER + 1 + 62 + 28
        assert L.tgsf_text_bgzf_bound((1 << 64) - 5, 1) == (1 << 64) - 1
        for n in (1, MEMBER - 1, MEMBER, 5 * MEMBER + 7):
            assert tgtext.bgzf_bound(n, True, text_lib) == zm.bound(n, True) and tgtext.bgzf_bound(n, False, text_lib) == zm.bound(n, False)
        assert "reserve" in _refused(-1, tx.deflate, text)                                              # before the reserve
        assert "reserve" in _refused(-1, tx.deflate_device, len(text), True, d_in=dev.ptr(d_in), d_out=dev.ptr(d_out), out_capacity=len(out))
        _refused(-1, tx.reserve_bgzf_out, 0, 100)
        _refused(-1, tx.reserve_bgzf_out, 100, 0)
        tx.reserve_bgzf_out(len(text))
        good()
        assert "already" in _refused(-1, tx.reserve_bgzf_out, len(text))                                # a second reserve
        good()
        assert "reserved for" in _refused(-4, tx.deflate, text + b"A")                                  # above the reserved size
        assert "reserved for" in _refused(-4, tx.deflate_device, len(text) + 1, True, d_in=dev.ptr(d_in), d_out=dev.ptr(d_out), out_capacity=len(out))
        good()
        s = tgtext.GzOutSummary()                                                                       # null arguments
        t = np.frombuffer(text, np.uint8)
        assert L.tgsf_text_bgzf_deflate(tx.h, None, 10, 1, out.ctypes.data, out.size, None, C.byref(s)) == -1
        assert L.tgsf_text_bgzf_deflate(tx.h, t.ctypes.data, t.size, 1, None, out.size, None, C.byref(s)) == -1
        assert L.tgsf_text_bgzf_deflate(tx.h, t.ctypes.data, t.size, 1, out.ctypes.data, out.size, None, None) == -1
        assert len(L.tgsf_text_last_error(tx.h)) > 10
        assert L.tgsf_text_bgzf_deflate(None, t.ctypes.data, t.size, 1, out.ctypes.data, out.size, None, C.byref(s)) == -1
        good()
        assert "eof" in _refused(-1, tx.deflate, text, eof=2)                                           # eof of 2
        good()
        assert "16-byte" in _refused(-1, tx.deflate_device, len(text) - 4, True, d_in=dev.ptr(d_in) + 4, d_out=dev.ptr(d_out), out_capacity=len(out))
        assert "16-byte" in _refused(-1, tx.deflate_device, len(text), True, d_in=dev.ptr(d_in), d_out=dev.ptr(d_out) + 8, out_capacity=len(out))
        assert "null" in _refused(-1, tx.deflate_device, len(text), True, d_out=dev.ptr(d_out), out_capacity=len(out))   # the object's output buffer: none yet
        good()
        assert "room for" in _refused(-4, tx.deflate, text, out_capacity=100)                           # the output does not fit
        good()
        # the CRC check's own refusals
        gz = tx.deflate(text)[0]
        blocks, stop, _, _ = tgtext.bgzf_walk(gz, 8, lib_path=text_lib)
        d_bad = dev.full(16, 0xA5)
        assert "reserve" in _refused(-1, tx.crc_device, blocks, dev.ptr(d_bad), d_gz=dev.ptr(d_out), d_inflated=dev.ptr(d_in))
        assert "reserve" in _refused(-1, tx.verify, gz)
        tx.reserve_bgzf(len(gz), 3)
        assert tx.verify(gz) == (NONE, NONE)
        assert "reserved for 3" in _refused(-4, tx.crc_device, np.concatenate([blocks, blocks[-1:], blocks[-1:]]), dev.ptr(d_bad), d_gz=dev.ptr(d_out), d_inflated=dev.ptr(d_in))
        lie = blocks.copy()
        lie["out"][1] += 1
        assert "member 1" in _refused(-1, tx.crc_device, lie, dev.ptr(d_bad), d_gz=dev.ptr(d_out), d_inflated=dev.ptr(d_in))
        assert L.tgsf_text_bgzf_crc_device(tx.h, dev.ptr(d_out), blocks.ctypes.data, len(blocks), dev.ptr(d_in), None, None) == -1
        assert L.tgsf_text_bgzf_crc_device(tx.h, dev.ptr(d_out), None, 2, dev.ptr(d_in), dev.ptr(d_bad), None) == -1
        g = np.frombuffer(gz, np.uint8)
        bb = C.c_uint32()
        assert L.tgsf_text_bgzf_verify(tx.h, g.ctypes.data, g.size, 1, None, C.byref(bb)) == -1
        assert L.tgsf_text_bgzf_verify(tx.h, g.ctypes.data, g.size, 1, C.byref(bb), None) == -1
        assert L.tgsf_text_bgzf_verify(tx.h, None, g.size, 1, C.byref(bb), C.byref(bb)) == -1
        assert "final" in _refused(-1, tx.verify, gz, final=2)
        assert "reserved for" in _refused(-4, tx.verify, gz + zm.EOF_MEMBER)
        assert tx.verify(gz) == (NONE, NONE)
        good()
    finally:
        tx.close()
    # the composed calls: what their counterparts refuse, and the output side's own rows
    reads = synth.make_reads(23, 12, "ont", mean_len=1500, zoo=False)
    ftext = textparity.fastq_of(reads)
    p = textparity.params_for("ont", reads, len(ftext), min_q=9.0)
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(ftext), 32, text_lib)
    try:
        assert "tgsf_text_out_reserve" in _refused(-1, tx.filter_bgzf, ctx, ftext, out=out)
        tx.reserve_output(64, 2 * len(ftext))
        assert "tgsf_text_bgzf_out_reserve" in _refused(-1, tx.filter_bgzf, ctx, ftext, out=out)
        tx.reserve_bgzf_out(4 * len(ftext))
        clean = tx.filter(ctx, ftext)[0]

        def good_filter():
            gz, sg, so, si = tx.filter_bgzf(ctx, ftext)
            _gz_agrees(clean, gz, sg, so, True, "a good filter")

        good_filter()
        assert "eof" in _refused(-1, tx.filter_bgzf, ctx, ftext, eof=3)
        assert "created for" in _refused(-4, tx.filter_bgzf, ctx, ftext + ftext)                        # the counterpart's refusal, unchanged
        assert "qualities" in _refused(-1, tx.filter_bgzf, ctx, ftext, fasta=True, fastq_out=True)
        good_filter()
        assert "room for" in _refused(-4, tx.filter_bgzf, ctx, ftext, out_capacity=64)                  # the compressed bytes do not fit
        good_filter()
        assert "reserve" in _refused(-1, tx.bam_filter_bgzf, ctx, b"")                                  # no tgsf_text_bam_reserve
        so, si = tgtext.OutSummary(), tgtext.Summary()
        t = np.frombuffer(ftext, np.uint8)
        assert L.tgsf_text_filter_bgzf(tx.h, ctx.h, t.ctypes.data, t.size, 0, 1, 1, out.ctypes.data, out.size, None, C.byref(si), None, None, 1, None) == -1
        assert L.tgsf_text_filter_bgzf(tx.h, None, t.ctypes.data, t.size, 0, 1, 1, out.ctypes.data, out.size, C.byref(so), C.byref(si), None, None, 1, None) == -1
        good_filter()
        # no record: an empty output, or the EOF member alone
        for eof in (True, False):
            gz, sg, so_, si_ = tx.filter_bgzf(ctx, b"", eof=eof)
            assert gz == (zm.EOF_MEMBER if eof else b"") and sg["n_members"] == int(eof) and so_["n_bytes"] == 0 and si_["n_records"] == 0
        # the object's own buffers, device form: the last format's text deflated where it lies
        tx.filter(ctx, ftext)
        d_sum = dev.full(40, 0)
        dev.sync()
        tx.deflate_device(len(clean), True, d_out=dev.ptr(d_out), out_capacity=len(out), d_summary=dev.ptr(d_sum))
        tx.fetch(want_index=False)
        s = tgtext.GzOutSummary.from_buffer_copy(dev.get(d_sum).tobytes()).as_dict()
        zm.check(clean, dev.get(d_out)[:s["n_bytes"]].tobytes(), True, None, s, "the object's output buffer")
        assert "output buffer has" in _refused(-4, tx.deflate_device, 2 * len(ftext) + 1, True, d_out=dev.ptr(d_out), out_capacity=len(out))
        good_filter()
    finally:
        tx.close()
        ctx.close()


# ---- 9: the CRC32 kernel against zlib.crc32 ---------------------------------------------------------------------------------------
CRC_SIZES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536)


def crc_against_zlib(text_lib, dev):
    """Members of every size and three fills, their inflated bytes packed one behind the other (so at odd addresses), through
    crc_device with trailers that are right, then with one bit of a CRC off in every fifth member in turn, then in three at once."""
    rng = np.random.default_rng(309)
    datas = []
    for n in CRC_SIZES:
        datas += [bytes(n), b"\xff" * n, bytes(rng.integers(0, 256, n).astype(np.uint8))]
    rng.shuffle(datas)
    assert len({sum(len(d) for d in datas[:i]) % 16 for i in range(len(datas))}) >= 8
    # the kernel reads the table, the inflated bytes and four bytes behind each payload: the chunk is hand-made, a payload of a
    # few arbitrary bytes and a trailer a member, so that members of 65535 and 65536 random bytes have a place in it
    gz, table, out = b"", [], 0
    for i, d in enumerate(datas):
        table.append((len(gz), i % 7, len(d), out))
        gz += bytes([0xA5] * (i % 7)) + zlib.crc32(d).to_bytes(4, "little") + len(d).to_bytes(4, "little")
        out += len(d)
    blocks = np.array(table, dtype=tgtext.BGZF_BLOCK_DTYPE)
    whole = b"".join(datas)
    tx = tgtext.TextIndexer(0, 4096, 16, text_lib)
    try:
        tx.reserve_bgzf(4096, len(datas))
        d_inf = dev.put(np.frombuffer(b"\xa5" + whole + b"\xa5" * 16, np.uint8))
        d_bad = dev.full(16, 0xA5)

        def check(g, want, what):
            d_gz = dev.put(np.frombuffer(g + bytes(16), np.uint8))
            dev.sync()
            tx.crc_device(blocks, dev.ptr(d_bad), d_gz=dev.ptr(d_gz), d_inflated=dev.ptr(d_inf) + 1, stream=dev.stream)
            dev.sync()
            bad = dev.get(d_bad)
            assert bad[:4].view(np.uint32)[0] == want and (bad[4:] == 0xA5).all(), (what, bad[:4].view(np.uint32)[0], want)

        check(gz, NONE, "every CRC is right")
        for b in range(0, len(datas), 5):
            g = bytearray(gz)
            at = int(blocks["payload"][b] + blocks["clen"][b]) + int(rng.integers(0, 4))
            g[at] ^= 1 << int(rng.integers(0, 8))
            check(bytes(g), b, ("one CRC off", b))
        g = bytearray(gz)
        for b in (40, 7, 55):
            g[int(blocks["payload"][b] + blocks["clen"][b])] ^= 0x10
        check(bytes(g), 7, "the lowest of three")
    finally:
        tx.close()


def verify(text_lib, dev):
    """verify() on good streams, with one CRC byte flipped in members 0, k and last, and with a bad DEFLATE member."""
    rng = np.random.default_rng(310)
    text = zm.fastq_like(rng, 5 * MEMBER + 99)
    tx = tgtext.TextIndexer(0, len(text), 16, text_lib)
    try:
        tx.reserve_bgzf_out(len(text))
        gz, ends, s = tx.deflate(text)
        tx.reserve_bgzf(len(gz), 8)
        assert s["n_members"] == 7 and tx.verify(gz) == (NONE, NONE) and tx.verify(gz[:int(ends[2])], final=False) == (NONE, NONE)
        zl = b"".join(gm.zmember(text[lo:hi]) for lo, hi in zm.cuts(len(text))) + zm.EOF_MEMBER
        assert tx.verify(zl) == (NONE, NONE)                            # what zlib writes
        begins = zm.starts(ends)

        def flipped(members):
            g = bytearray(gz)
            for b in members:
                g[int(ends[b]) - 8 + b % 4] ^= 0x40
            return bytes(g)

        for members, want in (((0,), 0), ((3,), 3), ((5,), 5), ((4, 2, 5), 2), ((6,), 6)):   # (member 6 is the EOF member: its CRC counts too)
            try:
                tx.verify(flipped(members))
                raise AssertionError("accepted")
            except capi.TgsfError as e:
                assert e.code == -6 and (e.bad_block, e.bad_crc) == (NONE, want) and ("member %d" % want) in str(e) and "CRC32" in str(e), (members, e.bad_block, e.bad_crc, str(e))
            assert tx.inflate(flipped(members))[0] == text              # the inflate itself does not look at the CRC, as ever
        g = bytearray(flipped((1,)))                                    # a bad DEFLATE member: reported as today, whatever the CRCs say
        g[begins[3] + 18] |= 6                                          # BTYPE 3
        assert gm.rule(bytes(g))["bad_block"] == 3
        try:
            tx.verify(bytes(g))
            raise AssertionError("accepted")
        except capi.TgsfError as e:
            assert e.code == -6 and e.bad_block == 3 and e.bad_crc == 1 and "member 3" in str(e) and "inflate" in str(e), (e.bad_block, e.bad_crc, str(e))
        assert tx.verify(gz) == (NONE, NONE)

        # what the walk leaves over refuses the check: TGSF_OK says that every byte was looked at
        def refused(code, g, words, final=True, t=tx):
            assert gm.rule(g, final, t.max_blocks, t.max_bytes)["stop"] == (CAPACITY if code == -4 else gm.IRREGULAR), ("the model", words)
            try:
                t.verify(g, final=final)
                raise AssertionError(("accepted", words))
            except capi.TgsfError as e:
                assert e.code == code and (e.bad_block, e.bad_crc) == (NONE, NONE) and all(w in str(e) for w in words), (e.code, str(e), words)

        cut1 = begins[1] + 3000                                         # inside member 1
        refused(-6, gz[:-40], ("byte %d" % begins[5], "member 5"))      # truncated: the last data member is cut short
        refused(-6, gz[:cut1], ("byte %d" % begins[1], "member 1"))
        refused(-6, gz[:-1], ("byte %d" % begins[6], "member 6"))       # the EOF member cut short
        refused(-6, gz[:begins[2]] + b"garbage behind member 1", ("byte %d" % begins[2], "member 2"))
        refused(-6, gz[:begins[2]] + b"garbage", ("byte %d" % begins[2],), final=False)
        g = bytearray(gz)
        g[begins[1]] ^= 0xFF                                            # member 1's magic
        refused(-6, bytes(g), ("byte %d" % begins[1], "member 1"))
        g = bytearray(gz)
        g[begins[4] + 16] ^= 0x55                                       # member 4's BSIZE: the next header is not where it says
        assert gm.rule(bytes(g))["stop"] in (gm.IRREGULAR,)
        refused(-6, bytes(g), ("member",))
        assert tx.verify(gz[:cut1], final=False) == (NONE, NONE)        # not final: a last member that is cut short is the next call's
        assert tx.verify(gz[:-40], final=False) == (NONE, NONE)
        assert tx.verify(gz) == (NONE, NONE)
        few = tgtext.TextIndexer(0, len(text), 16, text_lib)            # more members than max_blocks
        small = tgtext.TextIndexer(0, 2 * MEMBER + 5, 16, text_lib)     # more inflated bytes than the text buffer
        try:
            few.reserve_bgzf(len(gz), 3)
            refused(-4, gz, ("3 members", "byte %d" % begins[3]), t=few)
            refused(-4, gz, ("3 members", "byte %d" % begins[3]), final=False, t=few)
            assert few.verify(gz[:begins[3]], final=False) == (NONE, NONE)
            small.reserve_bgzf(len(gz), 8)
            refused(-4, gz, ("2 members", "byte %d" % begins[2]), t=small)
            assert small.verify(gz[:begins[2]]) == (NONE, NONE)
        finally:
            few.close()
            small.close()
    finally:
        tx.close()


# ---- 10: two objects on two threads --------------------------------------------------------------------------------------------------
def two_threads(text_lib, make_dev):
    errors = []

    def work(k):
        try:
            fuzz(text_lib, make_dev(), 1500 + k, 12, max_size=2 * MEMBER)
        except BaseException as e:              # noqa: BLE001 -- reported by the asserting thread
            errors.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
