"""Shared checks of the BAM input side of libtgsf_text (include/tgsf_text.h, tgsf_text_bam_*): a backend (the HIP build on the
GPU box, the serial emulation of the same kernels elsewhere) against tests/bammodel.py, word for word -- text bytes, pad,
the five index arrays, every summary word -- after every input has been asserted on the model's result first.
tests/test_bam_emul.py and tests/test_bam_gpu.py run them."""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import struct
import threading

import numpy as np

from oracle import orc
from tests import bammodel as bm, hostmodel, textoutparity as top, textparity
from tgsfilter_amd import capi, text as tgtext

END, IRREGULAR, CAPACITY = bm.END, bm.IRREGULAR, bm.CAPACITY
NONE = bm.NO_BAD_QUAL
PIECE = 4096
_refused = top._refused


# ---- inputs ------------------------------------------------------------------------------------------------------------
def record(name_field, codes, quals, n_cigar=0, aux=b"", l_seq=None, block_size=None, low_fill=0):
    """One BAM record from its parts: name_field is the l_read_name bytes as they lie in the record (NULs included), codes
    the 4-bit base codes, quals the raw qualities; l_seq / block_size overwrite the fields; low_fill is the unused low nibble
    of the last packed byte of an odd l_seq."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.size
    c = np.concatenate([codes, np.full(n & 1, low_fill, np.uint8)])
    packed = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
    core = struct.pack("<iiBBHHHIiii", -1, -1, len(name_field), 255, 4680, n_cigar, 4, n if l_seq is None else l_seq, -1, -1, 0)
    body = core + bytes(name_field) + bytes(range(1, 4 * n_cigar + 1)) + packed + bytes(quals) + bytes(aux)
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def rnd_record(rng, name_len, l_seq, aux=0, n_cigar=0, low_fill=0, qmax=100, name=None):
    nm = bytes(rng.integers(33, 127, name_len).astype(np.uint8)) if name is None else name
    return record(nm + b"\0", rng.integers(0, 16, l_seq), bytes(rng.integers(0, qmax, l_seq).astype(np.uint8)), n_cigar=n_cigar,
                  aux=bytes(rng.integers(0, 256, aux).astype(np.uint8)), low_fill=low_fill)


def text_room(bam_bytes):
    """Room for the decoded text: under 2 bytes of text per byte of BAM, but for six bytes a record (of 36 bytes or more)."""
    return 2 * bam_bytes + 64


# ---- device memory: host memory for the emulation, HBM through torch on the GPU ------------------------------------------
class HostMem(top.HostDev):
    def peek(self, ptr, n):
        return np.frombuffer(C.string_at(ptr, n), dtype=np.uint8) if n else np.zeros(0, np.uint8)

    def fill(self, ptr, n, v):
        C.memset(ptr, v, n)


class _Raw:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class TorchMem(top.TorchDev):
    def _view(self, ptr, n):
        return self.torch.as_tensor(_Raw(ptr, n), device=self.dev)

    def peek(self, ptr, n):
        self.sync()
        return self._view(ptr, n).cpu().numpy() if n else np.zeros(0, np.uint8)

    def fill(self, ptr, n, v):
        self.sync()
        self._view(ptr, n).fill_(v)
        self.sync()


def buffer_bytes(max_bytes):
    return ((max_bytes + 15) & ~15) + tgtext.PAD


# ---- the one comparison ---------------------------------------------------------------------------------------------------
def same_summary(s, m, what=""):
    for k in ("n_records", "stop", "consumed", "text_bytes", "bases", "longest", "bad_qual"):
        assert s[k] == m[k], (what, k, s, {x: m[x] for x in m if x not in ("text", "index")})
    assert s["reserved"] == 0 and s["device_ms"] >= 0.0, (what, s)


def same_index(idx, m, what=""):
    for f in bm.FIELDS:
        g, e = getattr(idx, f) if not isinstance(idx, dict) else idx[f], m["index"][f]
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, f, g[:8], e[:8])


def same_text(got, m, what=""):
    """got: the object's whole text buffer after the decode, filled with 0xA5 before it: the text, TGSF_TEXT_PAD zeros, and
    not a byte behind them."""
    n = m["text_bytes"]
    if got[:n].tobytes() != m["text"]:
        g, e = got[:n].tobytes(), m["text"]
        at = next(i for i in range(n + 1) if g[i:i + 1] != e[i:i + 1])
        raise AssertionError((what, "text differs at byte", at, g[max(0, at - 24):at + 24], e[max(0, at - 24):at + 24]))
    assert not got[n:n + tgtext.PAD].any(), (what, "pad", got[n:n + tgtext.PAD])
    assert (got[n + tgtext.PAD:] == 0xA5).all(), (what, "written behind the pad", n, np.nonzero(got[n + tgtext.PAD:] != 0xA5)[0][:8])


class Decoder:
    """One TextIndexer reserved for BAM; check() decodes a chunk and compares everything with the model."""

    def __init__(self, text_lib, dev, max_bam, max_records, max_bytes=None):
        self.dev = dev
        self.tx = tgtext.TextIndexer(0, text_room(max_bam) if max_bytes is None else max_bytes, max_records, text_lib)
        self.tx.reserve_bam(max_bam)
        self.room = buffer_bytes(self.tx.max_bytes)
        self.text_ptr = self.tx.buffers().text

    def model(self, bam, final=True):
        return bm.rule(bam, final, self.tx.max_records, self.tx.max_bytes)

    def check(self, bam, final=True, expect=None, what=""):
        """expect = (stop, n_records, consumed): asserted on the model first.  Returns the model's result."""
        m = self.model(bam, final)
        if expect is not None:
            assert (m["stop"], m["n_records"], m["consumed"]) == tuple(expect), (what, "the model", m["stop"], m["n_records"], m["consumed"], expect)
        self.dev.fill(self.text_ptr, self.room, 0xA5)
        idx, s = self.tx.bam_decode(bam, final=final)
        same_summary(s, m, what)
        same_index(idx, m, what)
        same_text(self.dev.peek(self.text_ptr, self.room), m, what)
        return m

    def close(self):
        self.tx.close()


# ---- 1: the model and the library pinned to the reference ----------------------------------------------------------------
class BamGolden(hostmodel.GoldenCase):
    """tests/golden/<name>.in.bam and what the reference made of it; the parameters as GoldenCase resolves them."""

    def __init__(self, golden_dir, name):
        self.name = name
        self.cmd = json.load(open(os.path.join(golden_dir, name + ".cmd.json")))
        self.bam = gzip.decompress(open(os.path.join(golden_dir, name + ".in.bam"), "rb").read())       # BGZF: gzip members
        self.ref_out = gzip.open(os.path.join(golden_dir, name + ".out.fq.gz"), "rb").read()
        self.stderr = open(os.path.join(golden_dir, name + ".stderr.txt")).read()
        self.info = hostmodel.parse_stderr(self.stderr)
        self.flags = hostmodel.parse_flags(self.cmd["flags"])


GOLDEN = {"hifi_bam": 60, "hifi_bam_auto": 700}


def golden_params(case, m):
    p = case.params()
    p.max_batch_reads = m["n_records"]
    p.max_batch_bases = 2 * m["text_bytes"] + 64 * m["n_records"] + 4096
    p.max_read_len = m["longest"]
    return p


def golden_model(golden_dir, name):
    """Without the library: the file inflates to a header and a clean chain of the stated number of records, nothing left over."""
    case = BamGolden(golden_dir, name)
    at = bm.header(case.bam)
    assert at is not None and at > 12
    chunk = case.bam[at:]
    m = bm.rule(chunk, True, 1 << 20, 1 << 40)
    assert (m["stop"], m["n_records"], m["consumed"], m["bad_qual"]) == (END, GOLDEN[name], len(chunk), NONE)
    return case, at, chunk, m


def golden(lib, text_lib, dev, golden_dir, name):
    case, at, chunk, m = golden_model(golden_dir, name)
    assert tgtext.bam_header(case.bam, text_lib) == at
    n = m["n_records"]
    D = Decoder(text_lib, dev, len(chunk), n)
    p = golden_params(case, m)
    try:
        D.check(chunk, True, (END, n, len(chunk)), name)
        # the decoded text through the text index: the same five arrays
        idx, s = D.tx.index(m["text"])
        assert s["n_records"] == n and s["stop"] == tgtext.END and s["consumed"] == len(m["text"])
        same_index(idx, m, "the text index on the decoded text")
        # records, fragments and every tally word: the oracle on the decoded reads
        ctx = capi.Context(p, 0, lib)
        try:
            host = np.frombuffer(m["text"] + b"\0" * 64, dtype=np.uint8)
            er, ef, ec = orc.filter_batch(p, host, host, m["index"]["seq_off"], m["index"]["len"], n_bins=ctx.n_bins, qual_offsets=m["index"]["qual_off"])
            idx, s, r1, f1 = D.tx.bam_submit(ctx, chunk)
            same_summary(s, m, name)
            same_index(idx, m, name)
            textparity.same_results((r1, f1, ctx.counters()), (er, ef, ec))
        finally:
            ctx.close()
        # BAM in, clean text out: the reference's own output file
        fr = top.frag_room(m["text_bytes"], n)
        D.tx.reserve_output(fr, top.out_room(m["text_bytes"], fr))
        ctx = capi.Context(p, 0, lib)
        try:
            out, rec_end, so, si = D.tx.bam_filter(ctx, chunk)
            assert out == case.ref_out and len(out) > 1000, name
            same_summary(si, m, name)
            top.same_output((out, rec_end, so), top.expected(m["text"], m["index"], er, ef, True), name)
            fa = D.tx.bam_filter(ctx, chunk, fastq_out=False)
            top.same_output(fa[:3], top.expected(m["text"], m["index"], er, ef, False), (name, "FASTA out"))
        finally:
            ctx.close()
    finally:
        D.close()


def bamio_against_reference(lib, text_lib, dev, ref_bin, tmp_path):
    """The reference binary on a tests/bamio.py file with auxiliary fields on every second record, against bam_filter.  Absent
    qualities (0xFF, which bamio writes for qual None) are not in this file: the reference binary itself dies of a segmentation
    fault on the first such record (a mean quality of -1 indexes its tables out of bounds), so there is nothing to compare
    with; that they decode to spaces, as in the host, is pinned by names_codes_qualities against the model."""
    import subprocess
    from tests import bamio
    from tgsfilter_amd import synth
    reads = synth.make_reads(27, 40, "hifi", mean_len=2500, zoo=False)
    path = os.path.join(str(tmp_path), "in.bam")
    bamio.write_bam(path, reads, aux_every=2)
    out, fa, flags = os.path.join(str(tmp_path), "ref_out.fq"), os.path.join(str(tmp_path), "adapters.fa"), "-x hifi -l 500 -q 15 -5 0 -3 0"
    with open(fa, "wb") as f:
        f.write(b">a0\n" + synth.PACBIO_BLUNT + b"\n")
    r = subprocess.run([ref_bin, "-i", path, "-t", "1"] + flags.split() + ["-o", out, "-a", fa], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and os.path.exists(out), r.stderr[-2000:]

    class Case(hostmodel.GoldenCase):
        def __init__(self):
            self.info, self.flags = hostmodel.parse_stderr(r.stderr), hostmodel.parse_flags(flags)

    bam = gzip.decompress(open(path, "rb").read())
    chunk = bam[bm.header(bam):]
    D = Decoder(text_lib, dev, len(chunk), len(reads))
    m = D.check(chunk, True, (END, len(reads), len(chunk)), "bamio")
    fr = top.frag_room(m["text_bytes"], len(reads))
    D.tx.reserve_output(fr, top.out_room(m["text_bytes"], fr))
    ctx = capi.Context(golden_params(Case(), m), 0, lib)
    try:
        got = D.tx.bam_filter(ctx, chunk)[0]
        assert got == open(out, "rb").read() and len(got) > 1000
    finally:
        ctx.close()
        D.close()


# ---- 2: seams ---------------------------------------------------------------------------------------------------------------
def seam_chunk(low_fill):
    """Name lengths 0..17 x l_seq 1..40 (the base stretch on every offset of a 16-byte chunk, both nibble parities), auxiliary
    tails of 0..16 bytes (record starts on every alignment), n_cigar_op of 0, 1, 3."""
    rng = np.random.default_rng(101)
    recs, k = [], 0
    for nl in range(18):
        for L in range(1, 41):
            recs.append(rnd_record(rng, nl, L, aux=k % 17, n_cigar=(0, 1, 3)[k % 3], low_fill=low_fill))
            k += 1
    return b"".join(recs), k


def seams(text_lib, dev):
    a, n = seam_chunk(0xF)
    b, _ = seam_chunk(0)
    assert a != b and len(a) == len(b)
    D = Decoder(text_lib, dev, len(a), n)
    try:
        ma = D.check(a, True, (END, n, len(a)), "seams, low nibble 0xF")
        mb = D.check(b, True, (END, n, len(b)), "seams, low nibble 0")
        assert ma["text"] == mb["text"] and np.unique(ma["index"]["seq_off"] % 16).size == 16
        starts = np.cumsum([0] + [len(x) for x in [a]])                # (one chunk; the starts' alignments are the model's walk)
        offs, _ = bm.walk(a, True, n)
        assert np.unique(np.array(offs[:-1]) % 16).size == 16 and starts[0] == 0
    finally:
        D.close()


def piece_seams(text_lib, dev, n_short=6):
    """l_seq around a piece, and one record of 300 000 bases among short ones."""
    rng = np.random.default_rng(102)
    recs = [rnd_record(rng, 5 + i % 7, L, aux=i % 5) for i, L in enumerate(range(PIECE - 17, PIECE + 18))]
    recs += [rnd_record(rng, 4, int(rng.integers(1, 90))) for _ in range(n_short)]
    recs.insert(len(recs) - n_short // 2, rnd_record(rng, 4, 300_000, aux=3, name=b"long"))
    bam = b"".join(recs)
    D = Decoder(text_lib, dev, len(bam), len(recs))
    try:
        m = D.check(bam, True, (END, len(recs), len(bam)), "piece seams")
        assert m["longest"] == 300_000
    finally:
        D.close()


def names_codes_qualities(lib, text_lib, dev):
    """l_read_name of 1 (an empty name) and 255, a NUL in the middle of the name field, all 16 base codes, every quality byte;
    233 in three records: bad_qual is the lowest, bam_submit refuses, and the next good call on the object succeeds."""
    rng = np.random.default_rng(103)
    allq = bytes(range(256))
    q_ok = bytes(x for x in range(256) if x != 233)
    codes = lambda n: np.arange(n) % 16                                # noqa: E731
    recs = [
        record(b"\0", codes(33), q_ok[:33]),
        record(b"n" * 254 + b"\0", codes(255), q_ok, n_cigar=3),
        record(b"n" * 255, codes(7), q_ok[200:207]),                   # no NUL within l_read_name: strnlen gives all 255
        record(b"ab\0cd\0", codes(16), q_ok[100:116], aux=b"xy"),
        record(b"absent\0", codes(50), b"\xff" * 50),
        record(b"q\0", codes(255), q_ok),
    ]
    good = b"".join(recs)
    bad = good + record(b"first_bad\0", codes(256), allq) + rnd_record(rng, 3, 20) + record(b"bad2\0", codes(5), b"\1\2\xe9\3\4") + record(b"bad3\0", codes(1), b"\xe9")
    D = Decoder(text_lib, dev, len(bad), 16)
    p = textparity.params_for("hifi", [(b"", b"A" * 256, b"")], text_room(len(bad)), min_q=0.0, min_len=1)
    p.max_batch_reads = 16
    ctx = capi.Context(p, 0, lib)
    try:
        m = D.check(good, True, (END, 6, len(good)), "names")
        assert m["bad_qual"] == NONE and set(b"\0ACGTN") <= set(m["text"]) and m["text"].count(b"\0") >= 10 * 33 // 16
        assert [int(x) for x in m["index"]["name_len"]] == [0, 254, 255, 2, 6, 1] and b"@\n" in m["text"] and b"@ab\n" in m["text"] and b" " * 50 in m["text"]
        assert len(set(m["text"])) >= 255
        m = D.check(bad, True, (END, 10, len(bad)), "every quality byte")
        assert m["bad_qual"] == 6 and m["text"].count(b"\n") == 4 * 10 + 3
        msg = _refused(-6, D.tx.bam_submit, ctx, bad)
        assert "first_bad" in msg and "quality" in msg
        try:
            D.tx.bam_submit(ctx, bad)
        except capi.TgsfError as e:
            same_summary(e.summary, m, "the refused call's summary")
        plain = b"".join(rnd_record(rng, 4, 200, aux=i, qmax=60) for i in range(5))      # (means within what libtgsf takes)
        idx, s, r, f = D.tx.bam_submit(ctx, plain)
        same_summary(s, D.model(plain), "after the refusal")
        same_index(idx, D.model(plain), "after the refusal")
        assert len(r) == 5
        assert "mean quality" in _refused(-6, D.tx.bam_submit, ctx, good)             # libtgsf's own refusal, handed through
        D.check(good, True, (END, 6, len(good)), "after the refusal")
    finally:
        ctx.close()
        D.close()


# ---- 3: stops -----------------------------------------------------------------------------------------------------------------
def three(rng=None):
    rng = rng or np.random.default_rng(104)
    recs = [rnd_record(rng, 3, 21, aux=2), rnd_record(rng, 0, 40, n_cigar=1), rnd_record(rng, 9, 5, aux=7)]
    return recs, np.cumsum([0] + [len(r) for r in recs])


def cut_everywhere(text_lib, dev):
    """One three-record chunk cut at every byte, final and not final."""
    recs, ends = three()
    bam = b"".join(recs)
    D = Decoder(text_lib, dev, len(bam), 8)
    try:
        for cut in range(len(bam) + 1):
            k = int(np.searchsorted(ends, cut, side="right")) - 1
            whole = cut == ends[k]
            D.check(bam[:cut], False, (END, k, int(ends[k])), ("cut", cut))
            D.check(bam[:cut], True, (END if whole else IRREGULAR, k, int(ends[k])), ("final cut", cut))
    finally:
        D.close()


def irregular_records(text_lib, dev):
    """block_size of 0, 31, 32; the field overrun by one byte and exactly fitting; l_seq == 0 as the first, a middle, the last record."""
    rng = np.random.default_rng(105)
    recs, ends = three(rng)
    a, b1 = recs[0], int(ends[1])
    exact = record(b"fits\0", rng.integers(0, 16, 9), bytes(9))        # block_size == o_qual + l_seq
    D = Decoder(text_lib, dev, 1024, 8)
    try:
        for bs in (0, 31, 32):
            tail = struct.pack("<I", bs) + bytes(bs) + recs[1]
            for final in (True, False):
                D.check(a + tail, final, (IRREGULAR, 1, b1), ("block_size", bs, final))
        D.check(a + exact + recs[2], True, (END, 3, b1 + len(exact) + len(recs[2])), "exactly fitting")
        over = struct.pack("<I", len(exact) - 5) + exact[4:]           # the qualities overrun the block by one byte
        D.check(a + over, True, (IRREGULAR, 1, b1), "overrun by one, final")
        D.check(a + over + recs[2], False, (IRREGULAR, 1, b1), "overrun by one")
        zero = record(b"z\0", [], b"", aux=b"abcdef")
        for at in (0, 1, 3):
            seq = recs[:at] + [zero] + recs[at:]
            D.check(b"".join(seq), True, (IRREGULAR, at, int(ends[at])), ("l_seq == 0 at", at))
        D.check(b"", True, (END, 0, 0), "empty")
        D.check(b"", False, (END, 0, 0), "empty, not final")
    finally:
        D.close()


def capacities(text_lib, dev):
    """max_records one below, at and one above the count; max_bytes one below, at and one above the decoded size and below the
    first record's; then resuming at `consumed` reproduces the whole file's text."""
    rng = np.random.default_rng(106)
    recs = [rnd_record(rng, int(rng.integers(0, 12)), int(rng.integers(1, 300)), aux=int(rng.integers(0, 9))) for _ in range(9)]
    bam = b"".join(recs)
    ends = np.cumsum([0] + [len(r) for r in recs])
    whole = bm.rule(bam, True, 100, 1 << 30)
    size, first = whole["text_bytes"], int(whole["index"]["name_off"][1]) - 1
    for mr, exp in ((8, (CAPACITY, 8, int(ends[8]))), (9, (END, 9, len(bam))), (10, (END, 9, len(bam)))):
        D = Decoder(text_lib, dev, len(bam), mr)
        try:
            D.check(bam, True, exp, ("max_records", mr))
        finally:
            D.close()
    for mb, exp in ((size - 1, (CAPACITY, 8, int(ends[8]))), (size, (END, 9, len(bam))), (size + 1, (END, 9, len(bam))), (first - 1, (CAPACITY, 0, 0)),
                    (first, (CAPACITY, 1, int(ends[1])))):
        D = Decoder(text_lib, dev, len(bam), 16, max_bytes=mb)
        try:
            D.check(bam, True, exp, ("max_bytes", mb))
        finally:
            D.close()
    D = Decoder(text_lib, dev, len(bam), 2, max_bytes=int(max(np.diff(np.concatenate([[0], whole["index"]["name_off"][1:] - 1, [size]])))) + 40)
    try:
        at, text, calls = 0, b"", 0
        while True:
            m = D.check(bam[at:], True, None, ("resume", at))
            assert m["n_records"] >= 1 or m["stop"] == END
            text += m["text"]
            at += m["consumed"]
            calls += 1
            if m["stop"] != CAPACITY:
                break
        assert text == whole["text"] and at == len(bam) and m["stop"] == END and calls >= 5
    finally:
        D.close()


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------
def refusals(lib, text_lib, dev):
    rng = np.random.default_rng(107)
    recs = [rnd_record(rng, 6, int(rng.integers(1200, 2500)), aux=4, qmax=60) for _ in range(12)]
    bam = b"".join(recs)
    m = bm.rule(bam, True, 32, text_room(len(bam)))
    assert (m["stop"], m["n_records"]) == (END, 12)
    reads = bm.reads_of(bam)
    tx = tgtext.TextIndexer(0, text_room(len(bam)), 32, text_lib)
    lib_c = tgtext.load(text_lib)
    p = textparity.params_for("hifi", reads, m["text_bytes"], min_q=5.0)
    ctx = capi.Context(p, 0, lib)

    def good():
        idx, s = tx.bam_decode(bam)
        same_summary(s, m)
        same_index(idx, m)
        got = tx.bam_filter(ctx, bam)
        ix, er, ef = top.oracle_on_text(p, m["text"])
        top.same_output(got[:3], top.expected(m["text"], ix, er, ef, True))

    try:
        assert "reserve" in _refused(-1, tx.bam_decode, bam)                                        # before reserve
        off, stop, consumed = tgtext.bam_walk(bam, 32, True, text_lib)
        assert "reserve" in _refused(-1, tx.bam_decode_device, len(bam), off, stop)
        tx.reserve_bam(len(bam))
        tx.reserve_output(256, 4 * len(bam))
        good()
        assert "already" in _refused(-1, tx.reserve_bam, len(bam))                                  # a second reserve
        good()
        assert "reserved for" in _refused(-4, tx.bam_decode, bam + recs[0])                         # n_bytes over the reserve
        assert "reserved for" in _refused(-4, tx.bam_filter, ctx, bam + recs[0])
        good()
        s = tgtext.BamSummary()                                                                     # null arguments
        assert lib_c.tgsf_text_bam_decode(tx.h, None, 10, 1, None, C.byref(s)) == -1
        assert lib_c.tgsf_text_bam_decode(tx.h, np.frombuffer(bam, np.uint8).ctypes.data, len(bam), 1, None, None) == -1
        assert lib_c.tgsf_text_bam_decode_device(tx.h, None, len(bam), 1, None, 0, 0, None, None, None) == -1
        assert lib_c.tgsf_text_bam_submit(tx.h, None, np.frombuffer(bam, np.uint8).ctypes.data, len(bam), 1, None, C.byref(s), None) == -1
        assert lib_c.tgsf_text_bam_header(None, 10, None) == -1 and lib_c.tgsf_text_bam_walk(None, 10, 1, 4, None, None, None, None) == -1
        assert len(lib_c.tgsf_text_last_error(tx.h)) > 10
        good()
        assert "fragment" in _refused(-4, tx.bam_filter, ctx, bam, want_results=True, frag_capacity=3)   # libtgsf's refusals, handed through
        good()
        ctx.close()
        p2 = textparity.params_for("hifi", reads, m["text_bytes"], min_q=5.0)
        p2.max_read_len = min(len(r[1]) for r in reads)
        ctx = capi.Context(p2, 0, lib)
        assert "max_read_len" in _refused(-6, tx.bam_filter, ctx, bam)
        assert "max_read_len" in _refused(-6, tx.bam_submit, ctx, bam)
        ctx.close()
        ctx = capi.Context(p, 0, lib)
        good()
        # the header: a wrong magic, and every cut of a header with two references
        hdr = b"BAM\1" + struct.pack("<I", 5) + b"@HD\t\n" + struct.pack("<I", 2) + struct.pack("<I", 3) + b"c1\0" + struct.pack("<I", 1000) + struct.pack("<I", 2) + b"x\0" + struct.pack("<I", 7)
        assert tgtext.bam_header(hdr + bam, text_lib) == len(hdr) == bm.header(hdr + bam)
        assert tgtext.bam_header(hdr, text_lib) == len(hdr)
        assert "magic" in _refused(-6, tgtext.bam_header, b"BAM\2" + hdr[4:], text_lib)
        for cut in range(len(hdr)):
            assert bm.header(hdr[:cut]) is None
            _refused(-6, tgtext.bam_header, hdr[:cut], text_lib)
    finally:
        ctx.close()
        tx.close()


# ---- 5: the device form -----------------------------------------------------------------------------------------------------------
def summary_of(dev, d_sum):
    return tgtext.BamSummary.from_buffer_copy(dev.get(d_sum).tobytes()).as_dict()


def device_form(text_lib, dev, seed=108, n=40, rounds=1):
    """The walk on the host, then bam_decode_device on a caller's stream with a caller's BAM buffer (of exactly n_bytes), index
    arrays (0xA5 around them) and summary."""
    rng = np.random.default_rng(seed)
    recs = [rnd_record(rng, int(rng.integers(0, 20)), int(rng.integers(1, 6000)), aux=int(rng.integers(0, 17)), n_cigar=int(rng.integers(0, 3))) for _ in range(n)]
    cases = [(b"".join(recs), True), (b"".join(recs)[:-7], False), (b"".join(recs[:n // 2]) + record(b"z\0", [], b"") + recs[0], True)]
    D = Decoder(text_lib, dev, max(len(c[0]) for c in cases), n + 2)
    mr = D.tx.max_records
    try:
        for _ in range(rounds):
            for bam, final in cases:
                m = D.model(bam, final)
                off, stop, consumed = tgtext.bam_walk(bam, mr, final, text_lib)
                assert [int(x) for x in off] == bm.walk(bam, final, mr)[0] and stop == bm.walk(bam, final, mr)[1] and consumed == int(off[-1])
                d_bam = dev.put(np.frombuffer(bam, np.uint8))
                arr = {f: dev.full((mr + 4) * (4 if f in ("len", "name_len") else 8), 0xA5) for f in bm.FIELDS}
                w = {f: 4 if f in ("len", "name_len") else 8 for f in bm.FIELDS}
                ia = tgtext.IndexArrays(*[dev.ptr(arr[f]) + 2 * w[f] for f in bm.FIELDS])
                d_sum = dev.full(48 + 32, 0xA5)
                D.dev.fill(D.text_ptr, D.room, 0xA5)
                dev.sync()
                D.tx.bam_decode_device(len(bam), off, stop, final=final, d_bam=dev.ptr(d_bam), d_index=ia, d_summary=dev.ptr(d_sum) + 16, stream=dev.stream)
                dev.sync()
                raw = dev.get(d_sum)
                assert (raw[:16] == 0xA5).all() and (raw[64:] == 0xA5).all()
                s = tgtext.BamSummary.from_buffer_copy(raw[16:64].tobytes()).as_dict()
                same_summary(s, m, "device form")
                k = m["n_records"]
                got = {}
                for f in bm.FIELDS:
                    a = dev.get(arr[f])
                    assert (a[:2 * w[f]] == 0xA5).all() and (a[(2 + mr) * w[f]:] == 0xA5).all(), ("canary of", f)
                    got[f] = a[2 * w[f]:(2 + k) * w[f]].view(np.uint32 if w[f] == 4 else np.uint64)
                same_index(got, m, "device form")
                same_text(D.dev.peek(D.text_ptr, D.room), m, "device form")
    finally:
        D.close()


def two_threads(text_lib, make_dev):
    errors = []

    def work(k):
        try:
            device_form(text_lib, make_dev(), seed=120 + k, n=30, rounds=3)
        except BaseException as e:              # noqa: BLE001 -- reported by the asserting thread
            errors.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


KINDS = ("END", "IRREGULAR", "CAPACITY", "BAD_QUAL")


def fuzz(text_lib, dev, seed, count, max_len=120):
    """A seeded stream of chunks; the stop kind and the cut are drawn explicitly, so that no kind's share is left to chance.
    Returns how many cases of each kind were run (each checked against the model, whose stop is asserted to be the kind drawn)."""
    rng = np.random.default_rng(seed)
    MR, MB = 12, 2 * max_len * 12
    D = Decoder(text_lib, dev, 1 << 16, MR, max_bytes=MB)
    ran = dict.fromkeys(KINDS, 0)
    try:
        for i in range(count):
            kind = KINDS[i % 4] if i < 8 else KINDS[int(rng.integers(0, 4))]
            n = int(rng.integers(1, MR + 1))
            recs = [rnd_record(rng, int(rng.integers(0, 24)), int(rng.integers(1, max_len + 1)), aux=int(rng.integers(0, 17)), n_cigar=int(rng.integers(0, 3)),
                               low_fill=int(rng.integers(0, 16)), qmax=200) for _ in range(n)]
            final, want_bad = True, NONE
            if kind == "END":
                final = bool(rng.integers(0, 2))
                bam = b"".join(recs)
                if not final:
                    bam = bam[:int(rng.integers(0, len(bam) + 1))]
                want = END
            elif kind == "IRREGULAR":
                how = int(rng.integers(0, 4))
                at = int(rng.integers(0, n))
                if how == 0:
                    recs[at] = record(b"zero\0", [], b"", aux=bytes(int(rng.integers(0, 9))))
                elif how == 1:
                    recs[at] = struct.pack("<I", int(rng.integers(0, 32))) + recs[at][4:]
                elif how == 2:
                    r = recs[at]
                    recs[at] = r[:20] + struct.pack("<I", struct.unpack_from("<I", r, 20)[0] + int(rng.integers(17, 400))) + r[24:]     # l_seq overruns the block (more than an auxiliary tail of 16 bytes can take)
                bam = b"".join(recs)
                if how == 3:
                    ends = np.cumsum([len(r) for r in recs])
                    cut = int(rng.integers(1, len(bam)))
                    bam = bam[:cut if cut not in ends else cut - 1]                     # a final chunk that ends inside a record
                want = IRREGULAR
            elif kind == "CAPACITY":
                if rng.integers(0, 2):
                    recs += [rnd_record(rng, 2, int(rng.integers(1, 30))) for _ in range(MR + 1 - n)]                               # one record too many
                else:
                    recs.insert(int(rng.integers(0, n + 1)), rnd_record(rng, 5, MB // 2 - int(rng.integers(0, 4))))                # its text alone has MB + 5 + .. bytes
                bam = b"".join(recs)
                want = CAPACITY
            else:
                at = int(rng.integers(0, n))
                r = bytearray(recs[at])
                l_seq, o = struct.unpack_from("<I", r, 20)[0], 4 + 32 + r[12] + 4 * struct.unpack_from("<H", r, 16)[0]
                r[o + (l_seq + 1) // 2 + int(rng.integers(0, l_seq))] = 233
                recs[at] = bytes(r)
                if at + 1 < n and rng.integers(0, 2):
                    r2 = bytearray(recs[n - 1])
                    l2, o2 = struct.unpack_from("<I", r2, 20)[0], 4 + 32 + r2[12] + 4 * struct.unpack_from("<H", r2, 16)[0]
                    r2[o2 + (l2 + 1) // 2 + l2 - 1] = 233
                    recs[n - 1] = bytes(r2)
                bam = b"".join(recs)
                want, want_bad = END, at
            m = D.check(bam, final, None, (seed, i, kind))
            assert m["stop"] == want and m["bad_qual"] == want_bad, (seed, i, kind, m["stop"], m["bad_qual"], want_bad)
            ran[kind] += 1
    finally:
        D.close()
    return ran
