"""Shared checks of the output side of libtgsf_text (include/tgsf_text.h, tgsf_text_format* / tgsf_text_filter): a backend
(the HIP build on the GPU box, the serial emulation of the same kernels elsewhere) against format_records below, which
is written from the rule of the header and pinned against tests/hostmodel.py and the reference's own output files.
tests/test_textout_emul.py and tests/test_textout_gpu.py run them."""
from __future__ import annotations

import threading

import numpy as np

from oracle import orc
from tests import hostmodel, textmodel, textparity
from tgsfilter_amd import abi, capi, synth, text as tgtext

ISSPACE = b" \t\n\v\f\r"
PIECE = 4096

# the three sets of the one-call checks: (seed, kind, reads, mean_len, pmid, filter parameters)
SYNTH_SETS = {
    31: ("ont", 300, 3000, 0.1, dict(min_q=9.0, head_trim=5, tail_trim=3)),
    32: ("hifi", 200, 5000, 0.3, dict(min_q=20.0)),
    35: ("ont", 200, 600, 0.5, dict(min_q=7.0, min_len=50)),
}
MODES = ("fastq_fastq", "fastq_fasta", "fasta_fasta")


# ---- the model ---------------------------------------------------------------------------------------------------
def _col(index, f):
    return index[f] if isinstance(index, dict) else getattr(index, f)


def format_records(text, index, reads, frags, fastq_out):
    """The rule of include/tgsf_text.h: (the output text, the byte behind each record).  `reads` is not needed by the rule
    (pass_num counts a read's PASS fragments in table order); it is taken to keep the call like the library's."""
    seq_off, qual_off, name_off, name_len = (_col(index, f) for f in ("seq_off", "qual_off", "name_off", "name_len"))
    out, ends, pos, seen = [], [], 0, {}
    for f in frags:
        if not int(f["flags"]) & abi.FF_PASS:
            continue
        r, s, l = int(f["read"]), int(f["start"]), int(f["len"])
        k = seen[r] = seen.get(r, 0) + 1
        name = bytes(text[int(name_off[r]):int(name_off[r]) + int(name_len[r])])
        if k >= 2:
            at = next((i for i, c in enumerate(name) if c in ISSPACE), len(name))
            name = name[:at] + b":" + str(k).encode() + name[at:]
        rec = (b"@" if fastq_out else b">") + name + b"\n" + bytes(text[int(seq_off[r]) + s:int(seq_off[r]) + s + l])
        if fastq_out:
            rec += b"\n+\n" + bytes(text[int(qual_off[r]) + s:int(qual_off[r]) + s + l])
        rec += b"\n"
        out.append(rec)
        pos += len(rec)
        ends.append(pos)
    return b"".join(out), np.array(ends, dtype=np.uint64)


def index_of(text, fasta=False):
    recs, consumed, stop = textmodel.rule(text, fasta, True)
    return textmodel.expected_index(recs)


def oracle_on_text(p, text, fasta=False):
    """(index, per-read records, fragments) of the oracle reading the text in place."""
    ix = index_of(text, fasta)
    host = np.frombuffer(text + b"\0" * 64, dtype=np.uint8)
    r, f, _ = orc.filter_batch(p, host, host, ix["seq_off"], ix["len"], qual_offsets=ix["qual_off"])
    return ix, r, f


def reads_with_two_pass(frags):
    passed = frags["read"][(frags["flags"] & abi.FF_PASS) != 0]
    return int((np.bincount(passed.astype(np.int64)) >= 2).sum()) if passed.size else 0


def synth_case(seed, mode, eol=b"\n"):
    """(kind, reads, text, fasta, fastq_out, params) of one synthetic one-call case."""
    kind, n, mean_len, pmid, kw = SYNTH_SETS[seed]
    reads = synth.make_reads(seed, n, kind, mean_len=mean_len, zoo=True, pmid=pmid)
    fasta = mode == "fasta_fasta"
    text = textparity.fasta_of(reads, eol) if fasta else textparity.fastq_of(reads, eol)
    kw = dict(kw, no_qual=True) if fasta else dict(kw)
    return kind, reads, text, fasta, mode == "fastq_fastq", textparity.params_for(kind, reads, len(text), **kw)


def frag_room(text_bytes, n_reads):
    return text_bytes // 100 + n_reads + 16


def out_room(text_bytes, n_frags_room):
    """Room for the output: a record is no longer than its read's, but for ":<n>" and a name repeated per fragment."""
    return 2 * text_bytes + 64 * n_frags_room + 4096


def same_output(got, exp, what=""):
    text, rec_end, s = got
    etext, eends, ebases = exp
    assert s["n_bytes"] == len(etext) and s["n_records"] == len(eends) and s["bases"] == ebases and s["stop"] == tgtext.END, (what, s, len(etext), len(eends), ebases)
    if text != etext:
        at = next(i for i in range(min(len(text), len(etext)) + 1) if text[i:i + 1] != etext[i:i + 1])
        raise AssertionError((what, "output differs at byte", at, text[max(0, at - 20):at + 20], etext[max(0, at - 20):at + 20]))
    assert rec_end.dtype == np.uint64 and np.array_equal(rec_end, eends), (what, rec_end[:8], eends[:8])


def expected(text, ix, reads, frags, fastq_out):
    etext, eends = format_records(text, ix, reads, frags, fastq_out)
    bases = int(frags["len"][(frags["flags"] & abi.FF_PASS) != 0].astype(np.int64).sum())
    return etext, eends, bases


# ---- 1, 2: the one-call form -------------------------------------------------------------------------------------------
def one_call(lib, text_lib, p, text, n_reads, fasta, fastq_out, exp, tables=None, what=""):
    """tx.filter(ctx, text) against exp = (text, record ends, bases); with tables = (records, fragments) the filter's results
    come down in a second call and equal them.  Returns the output."""
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(text), n_reads, text_lib)
    try:
        fr = frag_room(len(text), n_reads)
        tx.reserve_output(fr, out_room(len(text), fr))
        got = tx.filter(ctx, text, fasta=fasta, fastq_out=fastq_out)
        assert got[3]["n_records"] == n_reads and got[3]["stop"] == tgtext.END and got[3]["consumed"] == len(text), (what, got[3])
        same_output(got[:3], exp, what)
        if tables is not None:
            again = tx.filter(ctx, text, fasta=fasta, fastq_out=fastq_out, want_results=True)
            assert again[0] == got[0] and np.array_equal(again[4], tables[0]) and np.array_equal(again[5], tables[1]), what
    finally:
        tx.close()
        ctx.close()
    return got[0]


def golden(lib, text_lib, golden_dir, name):
    """The reference binary's own output file, byte for byte.  Its size, records, bases and record ends are read off the file:
    they are the oracle's and the model's (tests/test_textout_emul.py::test_model_equals_reference_output, on the CPU)."""
    case = hostmodel.GoldenCase(golden_dir, name)
    text = textparity.fastq_of(case.reads)
    p = case.params()
    p.max_batch_reads = len(case.reads)
    p.max_batch_bases = 2 * len(text) + 64 * len(case.reads) + 4096
    p.max_read_len = max(len(r[1]) for r in case.reads)
    lines = case.ref_out.split(b"\n")[:-1]
    assert len(lines) % 4 == 0
    sizes = [sum(len(x) + 1 for x in lines[i:i + 4]) for i in range(0, len(lines), 4)]
    exp = (case.ref_out, np.cumsum(sizes, dtype=np.uint64), sum(len(x) for x in lines[1::4]))
    out = one_call(lib, text_lib, p, text, len(case.reads), False, True, exp, None, name)
    assert out == case.ref_out and (name == "qc_only") == (out == b""), name


def synthetic(lib, text_lib, seed, mode):
    for eol in (b"\n", b"\r\n"):
        kind, reads, text, fasta, fastq_out, p = synth_case(seed, mode, eol)
        ix, er, ef = oracle_on_text(p, text, fasta)
        assert reads_with_two_pass(ef) >= 10, (seed, mode, reads_with_two_pass(ef))      # a condition of the test: ":<n>" is exercised
        out = one_call(lib, text_lib, p, text, len(reads), fasta, fastq_out, expected(text, ix, er, ef, fastq_out), (er, ef), (seed, mode, eol))
        assert b"\r" not in out


# ---- 3: hand-made fragment tables through format ---------------------------------------------------------------------
def tables(n_reads, frag_list):
    """Per-read records and the fragment table of [(read, start, len, flags)] (in read order)."""
    frags = np.zeros(len(frag_list), dtype=abi.FRAGMENT_DTYPE)
    reads = np.zeros(n_reads, dtype=abi.READ_RESULT_DTYPE)
    last = -1
    for i, (r, s, l, fl) in enumerate(frag_list):
        assert r >= last
        last = r
        frags[i] = (0, r, s, l, fl)
    cnt = np.bincount(frags["read"].astype(np.int64), minlength=n_reads) if len(frag_list) else np.zeros(n_reads, np.int64)
    reads["n_frags"] = cnt
    reads["frag_begin"] = np.concatenate(([0], np.cumsum(cnt)[:-1])) if n_reads else []
    return reads, frags


class Formatter:
    """One TextIndexer with a text and its index in it; check() formats a table and compares with the model."""

    def __init__(self, text_lib, text, fasta=False, max_frags=4096, max_out=None):
        self.text, self.fasta = text, fasta
        self.ix = index_of(text, fasta)
        self.n = len(self.ix["len"])
        self.tx = tgtext.TextIndexer(0, max(len(text), 1), max(self.n, 1), text_lib)
        self.tx.reserve_output(max_frags, max_out or out_room(len(text), max_frags))
        _, s = self.tx.index(text, fasta=fasta)
        assert s["n_records"] == self.n and s["stop"] == tgtext.END, s

    def check(self, frag_list, fastq_out, what=""):
        reads, frags = tables(self.n, frag_list)
        got = self.tx.format(self.n, reads, frags, fastq_out=fastq_out, fasta=self.fasta)
        exp = expected(self.text, self.ix, reads, frags, fastq_out)
        same_output(got, exp, what)
        return got[0]

    def close(self):
        self.tx.close()


def _seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]), bytes((rng.integers(3, 40, n) + 33).astype(np.uint8))


def many_fragments_of_one_read(text_lib):
    """400 bases cut into 120 PASS fragments of 1..5 bases, others interleaved: pass_num crosses 9 -> 10 and 99 -> 100."""
    rng = np.random.default_rng(5)
    reads = [(b"first x", *_seq(rng, 50)), (b"cut_up\tby adapters", *_seq(rng, 400)), (b"last", *_seq(rng, 60))]
    fl, at = [(0, 0, 50, abi.FF_PASS)], 0
    for k in range(120):
        if k % 3 == 1:
            fl.append((1, at, 1, abi.FF_REPEAT if k % 2 else 0))
            at += 1
        fl.append((1, at, 1 + k % 5, abi.FF_PASS))
        at += 1 + k % 5
    assert at <= 400
    fl += [(2, 3, 40, 0), (2, 3, 40, abi.FF_PASS), (2, 50, 10, abi.FF_PASS)]
    F = Formatter(text_lib, textparity.fastq_of(reads))
    try:
        for fastq_out in (True, False):
            out = F.check(fl, fastq_out, "120 fragments")
            assert b"up:9\tby" in out and b"up:10\tby" in out and b"up:99\tby" in out and b"up:100\tby" in out and b"up:120\tby" in out
            assert b"last:2\n" in out and b"first x\n" in out
    finally:
        F.close()
    F = Formatter(text_lib, textparity.fasta_of(reads), fasta=True)
    try:
        F.check(fl, False, "120 fragments, FASTA")
    finally:
        F.close()


NAMES = [b"", b"a", b"n" * 15, b"n" * 16, b"n" * 17, b"no_white_space_in_this_name", b"sp ace", b"ta\tb", b"vt\vx", b"ff\fx", b"cr\rx y", b" first", b"\tfirst", b"x  y"]


def names(text_lib):
    """Every kind of name, three records of each read (":2", ":3") and of 1..40 bases only: every chunk is a seam chunk."""
    rng = np.random.default_rng(6)
    reads = [(nm, *_seq(rng, 90)) for nm in NAMES]
    fl = []
    for r in range(len(reads)):
        a, b, c = (int(x) for x in rng.integers(1, 41, 3))
        fl += [(r, 0, a, abi.FF_PASS), (r, a, 2, 0), (r, a, b, abi.FF_PASS), (r, 90 - c, c, abi.FF_PASS)]
    for eol in (b"\n", b"\r\n"):
        F = Formatter(text_lib, textparity.fastq_of(reads, eol))
        try:
            for fastq_out in (True, False):
                out = F.check(fl, fastq_out, ("names", eol))
                for want in (b"@\n", b"@:2\n", b"@:3\n", b"@a:2\n", b"@" + b"n" * 16 + b":3\n", b"@sp:2 ace\n", b"@ta:2\tb\n", b"@vt:3\vx\n", b"@ff:2\fx\n",
                             b"@cr:2\rx y\n", b"@:2 first\n", b"@:3\tfirst\n", b"@x:2  y\n", b"@no_white_space_in_this_name:2\n"):
                    assert want.replace(b"@", b"@" if fastq_out else b">", 1) in out, want
        finally:
            F.close()
    # lengths 1..40, every one of them, one record each
    reads = [(b"r%d" % i, *_seq(rng, i)) for i in range(1, 41)]
    F = Formatter(text_lib, textparity.fastq_of(reads))
    try:
        for fastq_out in (True, False):
            F.check([(i, 0, i + 1, abi.FF_PASS) for i in range(40)], fastq_out, "1..40")
    finally:
        F.close()


def long_read_among_short(text_lib, n_short=30):
    reads = textparity.long_line_text(n_short=n_short)
    big = n_short // 2
    fl = []
    for r, (n, s, q) in enumerate(reads):
        if r == big:
            fl += [(r, 7, 100_001, abi.FF_PASS), (r, 100_100, 50, abi.FF_REPEAT), (r, 100_200, 150_003, abi.FF_PASS), (r, 299_000, 1000, abi.FF_PASS)]
        elif r % 4:
            fl.append((r, 0, len(s), abi.FF_PASS))
    for fasta in (False, True):
        text = textparity.fasta_of(reads) if fasta else textparity.fastq_of(reads)
        F = Formatter(text_lib, text, fasta=fasta)
        try:
            out = F.check(fl, not fasta, "long read")
            assert b"long:3\n" in out
            if not fasta:
                F.check(fl, False, "long read, FASTA out")
        finally:
            F.close()


def seam_sweep(text_lib, fastq_out, lengths=range(1, PIECE + 17 + 1)):
    """A leading record of every length up to a piece and a chunk more pushes the records behind it over every offset of a
    16-byte chunk and over both sides of the 4096-byte seam."""
    rng = np.random.default_rng(7)
    reads = [(b"lead", *_seq(rng, PIECE + 40)), (b"a b", *_seq(rng, 33)), (b"", *_seq(rng, 5)), (b"tail", *_seq(rng, 64))]
    F = Formatter(text_lib, textparity.fastq_of(reads), max_frags=16)
    try:
        for L in lengths:
            F.check([(0, 3, L, abi.FF_PASS), (1, 0, 33, abi.FF_PASS), (1, 1, 17, abi.FF_PASS), (2, 0, 5, 0), (2, 0, 5, abi.FF_PASS), (3, 0, 64, abi.FF_PASS),
                     (3, 10, 1, abi.FF_PASS)], fastq_out, ("sweep", L))
    finally:
        F.close()


def nothing_to_write(text_lib):
    rng = np.random.default_rng(8)
    reads = [(b"r%d" % i, *_seq(rng, 20)) for i in range(3)]
    F = Formatter(text_lib, textparity.fastq_of(reads))
    try:
        for fl in ([], [(0, 0, 20, 0), (1, 0, 5, abi.FF_REPEAT), (2, 1, 2, 0)]):
            for fastq_out in (True, False):
                assert F.check(fl, fastq_out, "nothing") == b""
        F.check([(1, 0, 20, abi.FF_PASS)], True, "and then something")
    finally:
        F.close()


# ---- 4: identity -------------------------------------------------------------------------------------------------------
def identity(text_lib, n=60):
    reads = synth.make_reads(44, n, "ont", mean_len=2500, zoo=False)
    for fasta in (False, True):
        text = textparity.fasta_of(reads) if fasta else textparity.fastq_of(reads)
        F = Formatter(text_lib, text, fasta=fasta, max_frags=n, max_out=len(text))
        try:
            assert F.check([(r, 0, len(rd[1]), abi.FF_PASS) for r, rd in enumerate(reads)], not fasta, "identity") == text
        finally:
            F.close()


# ---- device memory: host memory for the emulation, torch tensors on the GPU --------------------------------------------
class HostDev:
    stream = None

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        raw = np.empty(a.size + 16, np.uint8)
        at = (-raw.ctypes.data) % 16
        buf = raw[at:at + a.size]
        buf[:] = a
        return buf

    def full(self, n, v=0):
        return self.put(np.full(n, v, np.uint8))

    def ptr(self, x):
        return x.ctypes.data

    def get(self, x):
        return x.copy()

    def sync(self):
        pass


class TorchDev:
    def __init__(self, own_stream=True):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self._st = torch.cuda.Stream(device=self.dev) if own_stream else None
        self.stream = self._st.cuda_stream if own_stream else None

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def full(self, n, v=0):
        return self.torch.full((n,), v, dtype=self.torch.uint8, device=self.dev)

    def ptr(self, x):
        return x.data_ptr()

    def get(self, x):
        return x.cpu().numpy()

    def sync(self):
        if self._st is not None:
            self._st.synchronize()
        self.torch.cuda.synchronize()


def summary_of(dev, d_sum):
    return tgtext.OutSummary.from_buffer_copy(dev.get(d_sum).tobytes()).as_dict()


# ---- 5: capacity and canaries, on the device buffer itself ------------------------------------------------------------
def capacity_and_canaries(text_lib, dev):
    rng = np.random.default_rng(9)
    reads = [(b"r%d x" % i, *_seq(rng, int(rng.integers(1, 700)))) for i in range(40)]
    text = textparity.fastq_of(reads)
    fl = [(r, 0, len(rd[1]), abi.FF_PASS) for r, rd in enumerate(reads)] + [(39, 1, len(reads[39][1]) - 1, abi.FF_PASS)]
    F = Formatter(text_lib, text, max_frags=64)
    try:
        rd, fr = tables(F.n, fl)
        etext, eends, ebases = expected(text, F.ix, rd, fr, True)
        need = len(etext)
        assert need % 16 != 0                                          # the output ends in a partial chunk
        d_reads, d_frags = dev.put(rd), dev.put(fr)
        d_sum, d_ends = dev.full(32), dev.full(8 * 64)
        for cap in (need - 1, 0, need, need + 40):
            d_out = dev.full(cap + 64, 0xA5)
            dev.sync()
            F.tx.format_device(F.n, dev.ptr(d_reads), dev.ptr(d_frags), len(fr), d_out=dev.ptr(d_out), out_capacity=cap, d_rec_end=dev.ptr(d_ends),
                               d_summary=dev.ptr(d_sum), stream=dev.stream)
            dev.sync()
            s, out = summary_of(dev, d_sum), dev.get(d_out)
            assert s["n_bytes"] == need and s["n_records"] == len(eends) and s["bases"] == ebases, (cap, s)
            if cap < need:
                assert s["stop"] == tgtext.CAPACITY and (out == 0xA5).all(), (cap, s)     # the need is told, no byte changed
            else:
                assert s["stop"] == tgtext.END and out[:need].tobytes() == etext and (out[need:] == 0xA5).all(), (cap, s)
                assert np.array_equal(dev.get(d_ends).view(np.uint64)[:len(eends)], eends)
        # the host form: TGSF_E_CAPACITY with the need in the summary, the buffer untouched, then the same call with room
        for cap in (need - 1, 0):
            out = np.full(need + 64, 0xA5, np.uint8)
            try:
                F.tx.format(F.n, rd, fr, out=out, out_capacity=cap)
                raise AssertionError("accepted")
            except capi.TgsfError as e:
                assert e.code == -4 and e.summary["n_bytes"] == need and e.summary["stop"] == tgtext.CAPACITY and len(str(e)) > 20
            assert (out == 0xA5).all()
        out = np.full(need + 64, 0xA5, np.uint8)
        same_output(F.tx.format(F.n, rd, fr, out=out, out_capacity=need), (etext, eends, ebases), "with room")
        assert (out[need:] == 0xA5).all()
    finally:
        F.close()


# ---- 6: refusals and recovery -------------------------------------------------------------------------------------------
def _refused(code, call, *a, **kw):
    try:
        call(*a, **kw)
    except capi.TgsfError as e:
        assert e.code == code and len(str(e)) > 20, (e.code, str(e))
        return str(e)
    raise AssertionError("accepted")


def refusals(lib, text_lib, dev):
    """Each refusal returns its code with a message, and the same object then formats a good text correctly."""
    reads = synth.make_reads(22, 12, "ont", mean_len=1500, zoo=False)
    text = textparity.fastq_of(reads)
    ix = index_of(text)
    whole = [(r, 0, len(rd[1]), abi.FF_PASS) for r, rd in enumerate(reads)]
    rd, fr = tables(len(reads), whole)
    tx = tgtext.TextIndexer(0, len(text), 32, text_lib)

    def good_format():
        _, s = tx.index(text)
        assert s["n_records"] == len(reads)
        got = tx.format(len(reads), rd, fr)
        assert got[0] == text
        same_output(got, expected(text, ix, rd, fr, True))

    def good_filter(ctx, p):
        _, er, ef = oracle_on_text(p, text)
        same_output(tx.filter(ctx, text)[:3], expected(text, ix, er, ef, True))

    try:
        p = textparity.params_for("ont", reads, len(text), min_q=9.0)
        ctx = capi.Context(p, 0, lib)
        tx.index(text)
        assert "reserve" in _refused(-1, tx.format, len(reads), rd, fr, out=np.zeros(len(text), np.uint8))       # before reserve
        assert "reserve" in _refused(-1, tx.filter, ctx, text, out=np.zeros(len(text), np.uint8))
        tx.reserve_output(64, 2 * len(text))
        good_format()
        assert "reserved for 64" in _refused(-4, tx.format, len(reads), *tables(len(reads), sorted(whole * 6)))            # n_frags > max_frags
        good_format()
        _, s = tx.index(textparity.fasta_of(reads), fasta=True)
        assert "qualities" in _refused(-1, tx.format, len(reads), rd, fr, fastq_out=True, fasta=True)               # FASTQ from a FASTA index
        assert tx.format(len(reads), rd, fr, fastq_out=False, fasta=True)[0] == textparity.fasta_of(reads)
        good_format()
        d_reads, d_frags, d_out = dev.put(rd), dev.put(fr), dev.full(2 * len(text) + 32, 0xA5)
        dev.sync()
        assert "aligned" in _refused(-1, tx.format_device, len(reads), dev.ptr(d_reads), dev.ptr(d_frags), len(fr), d_out=dev.ptr(d_out) + 1,
                                     out_capacity=2 * len(text))                                                     # a misaligned caller's d_out
        dev.sync()
        assert (dev.get(d_out) == 0xA5).all()
        good_format()
        assert "already" in _refused(-1, tx.reserve_output, 64, 2 * len(text))
        good_format()
        # what tgsf_text_submit refuses, through filter: the same codes and words (tests/textparity.refusals)
        assert "created for" in _refused(-4, tx.filter, ctx, text + textparity.fastq_of(reads[:1]))
        good_filter(ctx, p)
        assert "fragment" in _refused(-4, tx.filter, ctx, text, want_results=True, frag_capacity=3)
        good_filter(ctx, p)
        ctx.close()
        p = textparity.params_for("ont", reads, len(text), min_q=9.0)
        p.max_batch_reads = 5
        ctx = capi.Context(p, 0, lib)
        assert "sized for 5" in _refused(-4, tx.filter, ctx, text)
        ctx.close()
        p = textparity.params_for("ont", reads, len(text), min_q=9.0)
        p.max_read_len = min(len(r[1]) for r in reads)
        ctx = capi.Context(p, 0, lib)
        assert "max_read_len" in _refused(-6, tx.filter, ctx, text)
        ctx.close()
        p = textparity.params_for("ont", reads, len(text), min_q=9.0)
        ctx = capi.Context(p, 0, lib)
        good_filter(ctx, p)
        good_format()
        # nothing regular: nothing runs, an empty output, no error
        got = tx.filter(ctx, b"garbage\n" + textparity.fastq_of(reads[:3]))
        assert got[0] == b"" and got[2]["n_bytes"] == 0 and got[2]["n_records"] == 0 and got[3]["n_records"] == 0 and got[3]["stop"] == tgtext.IRREGULAR
        good_filter(ctx, p)
        ctx.close()
    finally:
        tx.close()


# ---- 7: the device form -----------------------------------------------------------------------------------------------
def device_form(lib, text_lib, dev, seed=41, n=300, rounds=1):
    """index -> tgsf_submit_device -> tgsf_wait -> format_device with a caller's output, record ends and summary on the
    caller's stream: no table ever on the host (n_frags is the one host value).  Against the model after one synchronise."""
    reads = synth.make_reads(seed, n, "ont", mean_len=3000, zoo=True, pmid=0.1)
    text = textparity.fastq_of(reads)
    p = textparity.params_for("ont", reads, len(text), min_q=9.0)
    ix, er, ef = oracle_on_text(p, text)
    exp = expected(text, ix, er, ef, True)
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(text), n, text_lib)
    try:
        fcap = frag_room(len(text), n)
        cap = out_room(len(text), fcap)
        tx.reserve_output(fcap, 16)
        d_reads, d_frags, d_nf = dev.full(n * 32), dev.full(fcap * 24), dev.full(16)
        d_ends, d_sum = dev.full(fcap * 8), dev.full(32)
        for _ in range(rounds):
            d_out = dev.full(cap + 64, 0xA5)
            assert tx.upload(text) == len(text)
            tx.index_device(len(text))
            _, s = tx.fetch(want_index=False)
            assert s["n_records"] == n and s["stop"] == tgtext.END
            b = tx.buffers()
            dev.sync()
            ctx.submit_device(b.text, b.text, b.index.seq_off, b.index.len, n, len(text), dev.ptr(d_reads), dev.ptr(d_frags), fcap, dev.ptr(d_nf), None,
                              d_qual_offsets=b.index.qual_off)
            ctx.wait()
            nf = int(dev.get(d_nf).view(np.uint32)[0])
            assert nf == len(ef)
            tx.format_device(n, dev.ptr(d_reads), dev.ptr(d_frags), nf, d_out=dev.ptr(d_out), out_capacity=cap, d_rec_end=dev.ptr(d_ends),
                             d_summary=dev.ptr(d_sum), stream=dev.stream)
            dev.sync()
            out, s = dev.get(d_out), summary_of(dev, d_sum)
            same_output((out[:s["n_bytes"]].tobytes(), dev.get(d_ends).view(np.uint64)[:s["n_records"]], s), exp, "device form")
            assert (out[s["n_bytes"]:] == 0xA5).all()
    finally:
        tx.close()
        ctx.close()


def two_threads(lib, text_lib, make_dev):
    errors = []

    def work(k):
        try:
            device_form(lib, text_lib, make_dev(), seed=51 + k, n=120, rounds=4)
        except BaseException as e:              # noqa: BLE001 -- reported by the asserting thread
            errors.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


# ---- 8: seeded fuzz -----------------------------------------------------------------------------------------------------
def fuzz(text_lib, seed, count, max_len=60):
    """Small texts (LF and CRLF) with random fragment tables that obey the contract and a random output format; returns the
    number of output records checked."""
    rng = np.random.default_rng(seed)
    tx = tgtext.TextIndexer(0, 1 << 16, 64, text_lib)
    tx.reserve_output(512, 1 << 18)
    records = 0
    try:
        for i in range(count):
            fasta = bool(rng.random() < 0.4)
            text = textmodel.make_text(rng, fasta, damage="crlf" if rng.random() < 0.4 else "none", max_len=max_len)
            ix = index_of(text, fasta)
            n = len(ix["len"])
            fl = []
            for r in range(n):
                L = int(ix["len"][r])
                for _ in range(int(rng.integers(0, 5)) if rng.random() < 0.8 else int(rng.integers(5, 14))):
                    s = int(rng.integers(0, L))
                    fl.append((r, s, int(rng.integers(1, L - s + 1)), int(rng.integers(0, 4))))
            rd, fr = tables(n, fl)
            fastq_out = bool(not fasta and rng.random() < 0.6)
            _, s = tx.index(text, fasta=fasta)
            assert s["n_records"] == n, (seed, i, s)
            got = tx.format(n, rd, fr, fastq_out=fastq_out, fasta=fasta)
            same_output(got, expected(text, ix, rd, fr, fastq_out), (seed, i, text, fl, fastq_out))
            records += got[2]["n_records"]
    finally:
        tx.close()
    return records
