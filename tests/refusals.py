"""Shared checks of what libtgsf REFUSES and of what a context is worth afterwards (include/tgsf.h: the status codes, the
tally contract on tgsf_submit / tgsf_wait).  Every check takes `lib_path` -- the serial emulation's path on a GPU-less box,
None for the HIP build on the GPU -- so one body serves both builds, in the style of tests/parity.py."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import orc
from tests import parity
from tgsfilter_amd import abi, capi, synth

ADS = [synth.ONT_RAPID, synth.ONT_RAPID_RC]
HEAD, TAIL = 5, 3
LONGEST = 12801          # two 6 400-base tiles and one byte


def last_error(ctx):
    return ctx.lib.tgsf_last_error(ctx.h).decode()


def refused(ctx, rc, code, *words):
    """A call was refused with `code`, and its message holds every one of `words`."""
    assert rc == code, (rc, code, last_error(ctx))
    msg = last_error(ctx)
    for w in words:
        assert w in msg, (w, msg)


def raises(fn, code, *words, any_of=()):
    try:
        fn()
    except capi.TgsfError as e:
        assert e.code == code, (e.code, code, str(e))
        for w in words:
            assert w in str(e), (w, str(e))
        assert not any_of or any(w in str(e) for w in any_of), (any_of, str(e))
        return str(e)
    raise AssertionError("the call was accepted")


class Dev:
    """'Device' memory for tgsf_submit_device: host arrays on the emulation (its device memory is host memory), torch
    tensors on the GPU.  A handle is (pointer, whatever keeps the memory alive)."""

    def __init__(self, lib_path):
        self.torch = None
        if lib_path is None:
            import torch
            self.torch = torch
            self.dev = torch.device("cuda", 0)

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.torch is None:
            a = a.copy()
            return a.ctypes.data, a
        t = self.torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(self.dev)
        return t.data_ptr(), t

    def zeros(self, nbytes):
        return self.put(np.zeros(max(int(nbytes), 16), dtype=np.uint8))

    def sync(self):
        if self.torch is not None:
            self.torch.cuda.synchronize()

    def get(self, handle, dtype, count=None):
        a = handle[1].cpu().numpy() if self.torch is not None else handle[1]
        a = a.reshape(-1).view(np.uint8)
        if count is not None:
            a = a[:count * np.dtype(dtype).itemsize]
        return a.view(dtype).copy()


class DeviceBatch:
    """One batch in 'device' memory with output buffers of its own, and the oracle's answer to it."""

    def __init__(self, dev, p, n_bins, reads, exp_ctr=None, frag_room=16):
        seq, qual, off, ln = synth.pack(reads)
        self.exp_r, self.exp_f, self.exp_ctr = orc.filter_batch(p, seq, qual, off, ln, n_bins=n_bins, ctr=exp_ctr)
        self.n, self.n_bytes, self.dev = len(reads), seq.size, dev
        self.fcap = len(self.exp_f) + frag_room
        self.seq, self.qual = dev.put(seq), dev.put(qual)
        self.off, self.len = dev.put(off[:-1].astype(np.uint64)), dev.put(ln.astype(np.uint32))
        self.o_r = dev.zeros(self.n * abi.READ_RESULT_DTYPE.itemsize)
        self.o_f = dev.zeros(self.fcap * abi.FRAGMENT_DTYPE.itemsize)
        self.o_n = dev.zeros(16)

    def structs(self, fcap=None):
        bi = abi.BatchIn(self.seq[0], self.qual[0], self.off[0], self.len[0], self.n, 0, self.n_bytes, None)
        bo = abi.BatchOut(self.o_r[0], self.o_f[0], self.fcap if fcap is None else fcap, 0)
        return bi, bo

    def submit(self, ctx, fcap=None):
        bi, bo = self.structs(fcap)
        return ctx.lib.tgsf_submit_device(ctx.h, C.byref(bi), C.byref(bo), self.o_n[0], None)

    def check(self):
        got_r = self.dev.get(self.o_r, abi.READ_RESULT_DTYPE, self.n)
        nf = int(self.dev.get(self.o_n, np.uint32)[0])
        assert nf == len(self.exp_f), (nf, len(self.exp_f))
        got_f = self.dev.get(self.o_f, abi.FRAGMENT_DTYPE, nf)
        assert np.array_equal(got_r, self.exp_r) and np.array_equal(got_f, self.exp_f)


def assert_tallies(ctx, exp, what=""):
    got = ctx.counters()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: tally words differ at {bad[:12]}: got {got[bad[:12]]} exp {exp[bad[:12]]}"


def records_equal(got_r, got_f, exp_r, exp_f, what=""):
    assert np.array_equal(got_r, exp_r), what
    assert len(got_f) == len(exp_f) and np.array_equal(got_f, exp_f), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. refusals decided on the host: nothing is enqueued, the tallies do not move, the context goes on
# ---------------------------------------------------------------------------------------------------------------------
def host_refusals(lib_path):
    """check_batch, the output, span and pending-batch checks of tgsf_submit_async, the span and pointer checks of
    tgsf_submit_device, the buffer checks of tgsf_counters / tgsf_counters_used, tgsf_counters_merge and
    tgsf_align_windows, on a context that
    already holds tallies: each refusal has the code include/tgsf.h names and a message that says what was wrong, leaves
    tgsf_counters() bit-identical, and the context then passes compare_batch without a reset."""
    L, I, CAP = None, abi.E_INVALID, abi.E_CAPACITY
    good = synth.make_reads(91, 24, "ont", mean_len=1500, max_len=5000, zoo=True, pmid=0.2)
    p = parity.sized(abi.make_params("ont", adapters=ADS, min_q=7.0, min_len=100, head_trim=HEAD, tail_trim=TAIL), good)
    ctx = capi.Context(p, 0, lib_path)
    others = []
    try:
        L = ctx.lib
        _, _, before = parity.compare_batch(ctx, p, good)
        assert before.any()
        seq, qual, off, ln = synth.pack(good)
        n, off_n = len(good), off[:-1].copy()
        cap_reads, cap_bases = int(p.max_batch_reads), int(p.max_batch_bases)
        o_r = np.zeros(n, dtype=abi.READ_RESULT_DTYPE)
        o_f = np.zeros(int(ln.sum()) // 100 + n + 16, dtype=abi.FRAGMENT_DTYPE)
        far = off_n.copy()
        far[-1] = 1 << 40                              # (never read through: the span check comes first)
        far1 = off.copy()
        far1[-1] = 1 << 40

        def bi(**kw):
            d = dict(seq=seq.ctypes.data, qual=qual.ctypes.data, offsets=off_n.ctypes.data, lengths=ln.ctypes.data, n_reads=n,
                     n_bytes=seq.size, qual_offsets=None)
            d.update(kw)
            return abi.BatchIn(d["seq"], d["qual"], d["offsets"], d["lengths"], d["n_reads"], 0, d["n_bytes"], d["qual_offsets"])

        def bo(**kw):
            d = dict(reads=o_r.ctypes.data, frags=o_f.ctypes.data, cap=len(o_f))
            d.update(kw)
            return abi.BatchOut(d["reads"], d["frags"], d["cap"], 0)

        def unchanged(what):
            assert_tallies(ctx, before, what)

        batch_cases = [
            ("seq NULL", bi(seq=None), bo(), I, ["null batch pointer"]),
            ("offsets NULL", bi(offsets=None), bo(), I, ["null batch pointer"]),
            ("qual NULL without no_qual", bi(qual=None), bo(), I, ["null batch pointer"]),
            ("n_reads 0", bi(n_reads=0), bo(), I, ["empty batch"]),
            ("n_reads cap + 1", bi(n_reads=cap_reads + 1), bo(), CAP, ["%u reads" % (cap_reads + 1), "sized for %u" % cap_reads]),
            ("qual_offsets without lengths", bi(lengths=None, offsets=off.ctypes.data, qual_offsets=off_n.ctypes.data), bo(), I, ["qual_offsets", "lengths"]),
            ("span above the capacity", bi(n_bytes=cap_bases + 16 * cap_reads + 1), bo(), CAP, ["spans %u bytes" % (cap_bases + 16 * cap_reads + 1), "sized for %u bases" % cap_bases]),
        ]
        host_only = [
            ("span from offsets and lengths", bi(n_bytes=0, offsets=far.ctypes.data), bo(), CAP, ["spans"]),
            ("span from the last offset", bi(n_bytes=0, offsets=far1.ctypes.data, lengths=None), bo(), CAP, ["spans"]),
            ("out->reads NULL", bi(), bo(reads=None), I, ["null output"]),
        ]
        for fn in (L.tgsf_submit, L.tgsf_submit_async):
            refused(ctx, fn(ctx.h, None, C.byref(bo())), I, "null batch pointer")
            unchanged("in NULL")
            refused(ctx, fn(ctx.h, C.byref(bi()), None), I, "null output")
            unchanged("out NULL")
            for what, i_, o_, code, words in batch_cases + host_only:
                refused(ctx, fn(ctx.h, C.byref(i_), C.byref(o_)), code, *words)
                unchanged(what)
        # the largest span a context takes is not refused: cap_bases + 16 * cap_reads is what 16-byte padded reads may need
        assert cap_bases + 16 * cap_reads >= seq.size

        # tgsf_submit_device: the same batch checks, then its own
        dev = Dev(lib_path)
        db = DeviceBatch(dev, p, ctx.n_bins, good)
        dev.sync()
        assert db.seq[0] % 16 == 0 and db.qual[0] % 16 == 0
        d_i, d_o = db.structs()
        for what, i_, o_, code, words in batch_cases:
            j = abi.BatchIn(d_i.seq if i_.seq else None, d_i.qual if i_.qual else None, d_i.offsets if i_.offsets else None,
                            d_i.lengths if i_.lengths else None, i_.n_reads, 0, i_.n_bytes, d_i.offsets if i_.qual_offsets else None)
            refused(ctx, L.tgsf_submit_device(ctx.h, C.byref(j), C.byref(d_o), db.o_n[0], None), code, *words)
            unchanged("device: " + what)
        # a device batch states its span: the offsets are on the device, the host cannot derive it from them
        j = abi.BatchIn(d_i.seq, d_i.qual, d_i.offsets, d_i.lengths, d_i.n_reads, 0, 0, None)
        refused(ctx, L.tgsf_submit_device(ctx.h, C.byref(j), C.byref(d_o), db.o_n[0], None), I, "n_bytes is 0")
        unchanged("device: n_bytes 0")
        refused(ctx, L.tgsf_submit_device(ctx.h, C.byref(d_i), None, db.o_n[0], None), I, "null output")
        refused(ctx, L.tgsf_submit_device(ctx.h, C.byref(d_i), C.byref(abi.BatchOut(None, d_o.frags, d_o.frag_capacity, 0)), db.o_n[0], None), I, "null output")
        for seq_at, qual_at in ((1, 0), (8, 0), (0, 4), (0, 15)):
            j = abi.BatchIn(d_i.seq + seq_at, d_i.qual + qual_at, d_i.offsets, d_i.lengths, d_i.n_reads, 0, d_i.n_bytes - 16, None)
            refused(ctx, L.tgsf_submit_device(ctx.h, C.byref(j), C.byref(d_o), db.o_n[0], None), I, "16-byte aligned")
            unchanged("misaligned device pointers")
        refused(ctx, L.tgsf_wait(ctx.h), abi.OK)          # nothing was enqueued

        # a batch already pending: the second one is refused, writes nothing and adds nothing; the first completes as if alone
        ctx.submit_async(seq, qual, off_n, ln)
        for fn in (L.tgsf_submit_async, L.tgsf_submit):
            refused(ctx, fn(ctx.h, C.byref(bi()), C.byref(bo())), I, "a batch is already pending", "tgsf_wait")
        got_r, got_f = ctx.wait_result()
        exp_r, exp_f, before = orc.filter_batch(p, seq, qual, off, ln, n_bins=ctx.n_bins, ctr=before.copy())
        records_equal(got_r, got_f, exp_r, exp_f, "the pending batch")
        assert not o_r.view(np.uint8).any() and not o_f.view(np.uint8).any()
        unchanged("a second batch while one is pending")

        # fetching the tallies into too small a buffer
        buf = np.full(ctx.ctr_words, 0xA5A5A5A5, dtype=np.uint64)
        rows = (C.c_uint64 * 2)(7, 7)
        refused(ctx, L.tgsf_counters(ctx.h, buf.ctypes.data, ctx.ctr_words - 1), CAP, "counter buffer too small")
        refused(ctx, L.tgsf_counters_used(ctx.h, buf.ctypes.data, ctx.ctr_words - 1, rows), CAP, "counter buffer too small")
        assert (buf == 0xA5A5A5A5).all() and tuple(rows) == (7, 7)
        assert L.tgsf_counters(ctx.h, None, ctx.ctr_words) == I and L.tgsf_counters_used(ctx.h, None, ctx.ctr_words, rows) == I
        unchanged("tgsf_counters refusals")

        # merging: with itself, with another table geometry (more rows; more end-table positions; both at once such that
        # the two vectors are equally LONG: 40 words per position, 20 per row)
        assert L.tgsf_counters_merge(ctx.h, ctx.h) == I
        assert L.tgsf_counters_merge(ctx.h, None) == I and L.tgsf_counters_merge(None, ctx.h) == I
        for d_len, d_bc in ((200, 0), (0, 1), (-200, 1)):
            q = parity.sized(abi.make_params("ont", adapters=ADS, min_q=7.0, min_len=100, head_trim=HEAD, tail_trim=TAIL, bc_len=150 + d_bc), good)
            q.max_read_len = p.max_read_len + d_len
            o = capi.Context(q, 0, lib_path)
            others.append(o)
            assert (o.ctr_words == ctx.ctr_words) == (d_len < 0)
            refused(ctx, L.tgsf_counters_merge(ctx.h, o.h), I, "tgsf_counters_merge", "tally layout")
            refused(o, L.tgsf_counters_merge(o.h, ctx.h), I, "tgsf_counters_merge", "tally layout")
            unchanged("refused merge")
            assert not o.counters().any()

        # tgsf_align_windows
        rng = np.random.default_rng(3)
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 400)].copy()
        text[100:150] = np.frombuffer(synth.ONT_RAPID, dtype=np.uint8)
        Q = len(ADS[0])

        def align(n_=3, w_off=(0, 90, 300), w_len=(100, 80, 100), aid=(0, 0, 1), k=(10, 10, 10), null=None):
            a = [np.ascontiguousarray(w_off, np.uint64), np.ascontiguousarray(w_len, np.uint32), np.ascontiguousarray(aid, np.uint8),
                 np.ascontiguousarray(k, np.int32), np.zeros((n_, 4), np.int32), np.zeros((n_, 2), np.int32)]
            ptr = [x.ctypes.data for x in a]
            if null is not None:
                ptr[null] = None
            rc = L.tgsf_align_windows(ctx.h, text.ctypes.data, text.size, ptr[0], ptr[1], ptr[2], ptr[3], n_, ptr[4], ptr[5])
            return rc, a[4], a[5]
        refused(ctx, align(aid=(0, 2, 1))[0], I, "problem 1", "adapter id")
        refused(ctx, align(w_len=(100, 80, 0))[0], I, "problem 2", "window outside")
        refused(ctx, align(w_off=(301, 90, 300))[0], I, "problem 0", "window outside")
        refused(ctx, align(k=(10, -1, 10))[0], I, "problem 1", "k < 0")
        refused(ctx, align(k=(10, 10, Q))[0], CAP, "problem 2", "k larger")
        many = 2 * cap_reads * len(ADS) + 1
        refused(ctx, align(many, [0] * many, [50] * many, [0] * many, [5] * many)[0], CAP, "more alignment problems")
        for k_ in range(6):
            assert align(null=k_)[0] == I
        unchanged("tgsf_align_windows refusals")
        rc, res, ends = align()
        refused(ctx, rc, abi.OK)
        ed, n_loc, starts, ends_, alen = orc.align_hw(synth.ONT_RAPID, text[90:170].tobytes(), 10)
        assert (int(res[1, 0]), int(res[1, 1]), int(res[1, 2]), int(res[1, 3]), int(ends[1, 0])) == (ed, n_loc, alen, starts[0], ends_[0]) == (0, 1, 50, 10, 59)

        # ... and the context goes on where it was: a good batch on top of the tallies it held, one through tgsf_submit_device
        _, _, now = parity.compare_batch(ctx, p, good, align=1, explicit_lengths=False, base=before)
        db2 = DeviceBatch(dev, p, ctx.n_bins, good, exp_ctr=now.copy())
        dev.sync()
        refused(ctx, db2.submit(ctx), abi.OK)
        ctx.wait()
        db2.check()
        assert_tallies(ctx, db2.exp_ctr, "after the refusals")
    finally:
        for o in others:
            o.close()
        ctx.close()


def text_over_capacity(lib_path, text_lib_path):
    """tgsf_text_submit hands its text's size to tgsf_submit_device as the batch's span: an object that holds more text
    than the context takes (max_batch_bases + 16 * max_batch_reads) gets TGSF_E_CAPACITY through the text object, nothing
    of the batch is enqueued or tallied, and the object and the context both go on -- the context with a text that fits,
    the object with a context that takes the large one."""
    from tests import textparity
    from tgsfilter_amd import text as tgtext
    reads = synth.make_reads(23, 40, "ont", mean_len=1500, max_len=5000, zoo=True, pmid=0.1)
    small = reads[:8]
    padded, off, qoff, ln = parity.fastq_text_layout(reads)
    text = padded[:-64].tobytes()
    s_padded, s_off, s_qoff, s_ln = parity.fastq_text_layout(small)
    s_text = s_padded[:-64].tobytes()
    p = abi.make_params("ont", adapters=ADS, min_q=7.0, min_len=100, head_trim=HEAD, tail_trim=TAIL)
    p.max_batch_reads, p.max_read_len = len(reads), max(len(r[1]) for r in reads)
    p.max_batch_bases = len(text) - 16 * len(reads) - 1               # one byte short of the whole text
    assert p.max_batch_bases + 16 * p.max_batch_reads >= len(s_text)
    big = abi.make_params("ont", adapters=ADS, min_q=7.0, min_len=100, head_trim=HEAD, tail_trim=TAIL)
    big.max_batch_reads, big.max_read_len, big.max_batch_bases = p.max_batch_reads, p.max_read_len, len(text)
    ctx = capi.Context(p, 0, lib_path)
    ctx_big = capi.Context(big, 0, lib_path)
    tx = tgtext.TextIndexer(0, len(text), len(reads), text_lib_path)
    try:
        idx, s, r, f = tx.submit(ctx, s_text)
        exp_r, exp_f, before = orc.filter_batch(p, s_padded, s_padded, s_off, s_ln, n_bins=ctx.n_bins, qual_offsets=s_qoff)
        records_equal(r, f, exp_r, exp_f, "a text that fits")
        assert_tallies(ctx, before, "a text that fits")
        raises(lambda: tx.submit(ctx, text), abi.E_CAPACITY, "spans %u bytes" % len(text), "sized for %u bases" % p.max_batch_bases)
        refused(ctx, ctx.lib.tgsf_wait(ctx.h), abi.OK)                 # nothing was enqueued
        assert_tallies(ctx, before, "after the refused text")
        idx, s, r, f = tx.submit(ctx, s_text)                          # the same object, the same context
        exp_r, exp_f, now = orc.filter_batch(p, s_padded, s_padded, s_off, s_ln, n_bins=ctx.n_bins, qual_offsets=s_qoff, ctr=before.copy())
        assert s["n_records"] == len(small) and s["stop"] == tgtext.END
        records_equal(r, f, exp_r, exp_f, "the context after the refusal")
        assert_tallies(ctx, now, "the context after the refusal")
        idx, s, r, f = tx.submit(ctx_big, text)                        # the object still holds and indexes the large text
        exp_r, exp_f, exp = orc.filter_batch(big, padded, padded, off, ln, n_bins=ctx_big.n_bins, qual_offsets=qoff)
        assert s["n_records"] == len(reads) and np.array_equal(idx.seq_off, off) and np.array_equal(idx.qual_off, qoff)
        records_equal(r, f, exp_r, exp_f, "the text object after the refusal")
        assert_tallies(ctx_big, exp, "the text object after the refusal")
    finally:
        tx.close()
        ctx.close()
        ctx_big.close()


def min_len_below_zero(lib_path, text_lib_path):
    """tgsf_params.min_len < 0: tgsf_create refuses it in front of the device (with a negative min_len k_prepare would
    speculate on reads shorter than their trims), so no context exists for tgsf_text_filter to take either -- it answers a
    NULL context with TGSF_E_INVALID and runs nothing.  min_len = 0 is the domain's edge: the one-call form then gives the
    oracle's records and fragments, reads shorter than the trims among them."""
    from tests import textoutparity as top
    from tests import textparity
    from tgsfilter_amd import text as tgtext
    rng = np.random.default_rng(29)
    reads = synth.make_reads(29, 24, "ont", mean_len=1500, max_len=5000, zoo=True, pmid=0.1)
    for L in (3, 2000, 4, 1500, 7, 12, 13, HEAD + TAIL, HEAD + TAIL + 1):
        reads.insert(int(rng.integers(0, len(reads))), (b"short%d" % L, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes(),
                                                        (rng.integers(25, 40, L) + 33).astype(np.uint8).tobytes()))
    text = textparity.fastq_of(reads)
    p = seam_params(reads)
    for bad in (-1, -(1 << 31)):
        p.min_len = bad
        raises(lambda: capi.Context(p, 0, lib_path), abi.E_INVALID, "min_len")

    class NoContext:
        h = None
    fr = top.frag_room(len(text), len(reads))
    tx = tgtext.TextIndexer(0, len(text), len(reads), text_lib_path)
    try:
        tx.reserve_output(fr, top.out_room(len(text), fr))
        raises(lambda: tx.filter(NoContext(), text), abi.E_INVALID, "null argument")
    finally:
        tx.close()
    p.min_len = 0
    ix, er, ef = top.oracle_on_text(p, text)
    assert (ef["len"][(ef["flags"] & abi.FF_PASS) != 0] < 100).any()
    top.one_call(lib_path, text_lib_path, p, text, len(reads), False, True, top.expected(text, ix, er, ef, True), (er, ef), "min_len 0")


SEARCH_BOUND = 1 << 28          # the most end_len (-E) and extra_len (-T) may be: the cap on max_read_len


def end_len_and_extra_len_above_their_bound(lib_path):
    """tgsf_params.end_len / extra_len above 2^28: tgsf_create refuses them in front of the device, whether or not adapters are
    searched for (k_gate_reads forms L - 2 * end_len, k_mid_resolve pos + end_len + 1 + extra_len in 32 signed bits: with
    end_len = 1 500 000 000 a read got a middle window far outside itself).  tgsf_create only: no batch is submitted with
    such a value.  The bound itself is taken, and a context that was created next to a refused one works."""
    reads = synth.make_reads(28, 12, "ont", mean_len=1200, max_len=4000, zoo=True, pmid=0.2)
    for field, flag in (("end_len", "-E"), ("extra_len", "-T")):
        for bad in (SEARCH_BOUND + 1, 1_500_000_000, 2147483647):
            for kw in ({}, {"filter": False}, {"adapters": []}):
                p = seam_params(reads, **kw)
                setattr(p, field, bad)
                raises(lambda: capi.Context(p, 0, lib_path), abi.E_INVALID, "%s (%s) %d" % (field, flag, bad), "2^28")
    p = seam_params(reads)
    p.end_len = p.extra_len = SEARCH_BOUND
    ctx = capi.Context(p, 0, lib_path)
    try:
        parity.compare_batch(ctx, p, reads)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. refusals decided on the device
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_reads(seed=71, n=300):
    """300 short reads of 200..700 bp (k_prepare's read loop spans more than one 256-lane block; a few shorter ones from
    the zoo) and reads on the seams of the 6 400-base tiles.  The longest one comes last."""
    rng = np.random.default_rng(seed)
    reads = synth.make_reads(seed, n, "ont", mean_len=420, max_len=700, zoo=True)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for L in (6399, 6400, 6401, LONGEST):
        s = bytearray(acgt[rng.integers(0, 4, L)].tobytes())
        a = synth.mutate(rng, synth.ONT_RAPID_RC, 0.04)
        s[L // 2:L // 2 + len(a)] = a
        q = (np.clip(np.rint(rng.normal(16, 4, L)), 2, 40) + 33).astype(np.uint8).tobytes()
        reads.insert(len(reads) if L == LONGEST else int(rng.integers(0, len(reads))), (b"seam%d" % L, bytes(s[:L]), q))
    assert max(len(r[1]) for r in reads[:-1]) < LONGEST == len(reads[-1][1])
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def good_batches():
    return tuple(tuple(synth.make_reads(81 + k, n, "ont", mean_len=m, max_len=6000, zoo=True, pmid=0.2)) for k, (n, m) in enumerate(((40, 1500), (32, 2500), (24, 2000))))


def seam_params(reads, max_read_len=None, **kw):
    kw = dict(dict(adapters=ADS, min_q=7.0, min_len=100, head_trim=HEAD, tail_trim=TAIL), **kw)
    p = abi.make_params("ont", **kw)
    p.max_batch_reads = len(reads)
    p.max_batch_bases = 2 * sum(len(r[1]) for r in reads) + 64 * len(reads) + 4096      # (room for a batch as FASTQ text)
    p.max_read_len = max_read_len or max(len(r[1]) for r in reads)
    return p


def set_mode(monkeypatch, mode):
    monkeypatch.setenv("TGSF_CLEAN_TABLES", mode) if mode else monkeypatch.delenv("TGSF_CLEAN_TABLES", raising=False)


def recover(ctx, p, known=None):
    """What a context is worth after a refusal.  Without a reset the next batch's records and fragments are the oracle's
    (and its tallies too where the refusal left `known` ones).  After tgsf_reset_counters the context is as new: three
    batches, 16-byte padded / packed with implicit lengths / FASTQ text in place, the tallies accumulating."""
    g = good_batches()
    seq, qual, off, ln = synth.pack(g[0])
    got_r, got_f = ctx.submit(seq, qual, off[:-1].copy(), ln)
    exp_r, exp_f, exp = orc.filter_batch(p, seq, qual, off, ln, n_bins=ctx.n_bins, ctr=None if known is None else known.copy())
    records_equal(got_r, got_f, exp_r, exp_f, "first batch after the refusal, no reset")
    if known is not None:
        assert_tallies(ctx, exp, "first batch after the refusal, no reset")
    ctx.reset_counters()
    assert not ctx.counters().any()
    _, _, base = parity.compare_batch(ctx, p, g[0], align=16)
    _, _, base = parity.compare_batch(ctx, p, g[1], align=1, explicit_lengths=False, base=base)
    _, _, base = parity.compare_batch_in_place(ctx, p, g[2], base=base)
    return base


def bad_length_batch(kind, at):
    """A batch of seam_reads() with ONE read of unsupported length at index `at` (negative: from the end).
    kind "len0": length 0 in explicit `lengths`; "offsets": two equal offsets, lengths == NULL, no padding; "over": the
    longest read, one base above the context's max_read_len.  Returns (submit arguments, index, the other reads, max_read_len)."""
    reads = list(seam_reads())
    n = len(reads)
    idx = at if at >= 0 else n + at
    if kind == "over":
        batch = reads[:-1][:idx] + [reads[-1]] + reads[:-1][idx:]
        seq, qual, off, ln = synth.pack(batch)
        return (seq, qual, off[:-1].copy(), ln), idx, batch[:idx] + batch[idx + 1:], LONGEST - 1
    others = reads[:idx] + reads[idx + 1:]
    if kind == "len0":
        seq, qual, off, ln = synth.pack(reads)
        ln[idx] = 0
        return (seq, qual, off[:-1].copy(), ln), idx, others, LONGEST
    assert kind == "offsets"
    seq, qual, off, ln = synth.pack(others, align=1)
    off = np.insert(off, idx, off[idx])
    assert len(off) == n + 1 and off[idx] == off[idx + 1]
    return (seq, qual, off, None), idx, others, LONGEST


def oracle_tallies(p, n_bins, reads, base=None):
    seq, qual, off, ln = synth.pack(reads)
    return orc.filter_batch(p, seq, qual, off, ln, n_bins=n_bins, ctr=None if base is None else base.copy())[2]


def bad_length(lib_path, kind, at, mode, monkeypatch):
    """DS_BAD_LEN in k_prepare: TGSF_E_DATA, the message names the read.  Every later kernel of the pipeline runs over
    that read with a length of 0.  The tally contract (include/tgsf.h, tgsf_wait): that read is left out, the batch's
    other reads are tallied exactly as the oracle tallies them alone; the next batch adds to that without a reset, and
    after a reset the context is as new: recover()."""
    set_mode(monkeypatch, mode)
    args, idx, others, max_read_len = bad_length_batch(kind, at)
    p = seam_params(seam_reads(), max_read_len=max_read_len)
    ctx = capi.Context(p, 0, lib_path)
    try:
        raises(lambda: ctx.submit(*args), abi.E_DATA, "read %d:" % idx, "length 0 or above max_read_len %d" % max_read_len)
        left = oracle_tallies(p, ctx.n_bins, others)
        assert_tallies(ctx, left, "the other reads of a batch refused for one read's length")
        recover(ctx, p, left)
    finally:
        ctx.close()


def two_bad_lengths(lib_path, monkeypatch, mode=None):
    """Two reads of length 0 in one batch: either may be the one named; both are left out of the tallies."""
    set_mode(monkeypatch, mode)
    reads = list(seam_reads())
    seq, qual, off, ln = synth.pack(reads)
    ln[3] = ln[200] = 0
    p = seam_params(reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "length 0", any_of=("read 3:", "read 200:"))
        left = oracle_tallies(p, ctx.n_bins, [r for k, r in enumerate(reads) if k not in (3, 200)])
        assert_tallies(ctx, left, "the other reads of a batch refused for two reads' lengths")
        recover(ctx, p, left)
    finally:
        ctx.close()


def bad_mean_quality(lib_path, at, mode, monkeypatch):
    """A read whose raw mean of `qual - qType` is below 0 (every byte 200: -89): TGSF_E_DATA, the message names the read.
    The raw pass has tallied it by then: the tallies hold an unspecified part of the batch until tgsf_reset_counters."""
    set_mode(monkeypatch, mode)
    reads = list(seam_reads())
    idx = at if at >= 0 else len(reads) + at
    name, s, q = reads[idx]
    reads[idx] = (name, s, bytes([200]) * len(q))
    p = seam_params(reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        seq, qual, off, ln = synth.pack(reads)
        raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "read %d:" % idx, "mean quality outside [0,256)")
        recover(ctx, p)
    finally:
        ctx.close()


def negative_kept_mean_reads():
    """One read of 1 000 bases whose raw mean is 2 -- inside the tables -- while what -5 500 keeps of it has a mean of
    -89: with the filter on, the quality gate drops that fragment before its mean is taken as a table index
    (src/TGSFilter.cpp:1995-2002), in the library as in the oracle.  Beside ordinary reads."""
    rng = np.random.default_rng(5)
    reads = synth.make_reads(85, 30, "ont", mean_len=2500, max_len=9000, zoo=True, pmid=0.1)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1000)].tobytes()
    reads.insert(11, (b"kept_mean_below_0", s, bytes([126]) * 500 + bytes([200]) * 500))
    p = parity.sized(abi.make_params("ont", adapters=ADS, min_q=1.0, min_len=100, head_trim=500), reads)
    return reads, p, 11


def negative_kept_mean_oracle():
    """The case with the oracle alone: raw mean 2, accepted, its one fragment dropped by the quality gate."""
    reads, p, at = negative_kept_mean_reads()
    seq, qual, off, ln = synth.pack(reads)
    r, f, ctr = orc.filter_batch(p, seq, qual, off, ln)
    assert int(r["sum_q"][at]) == 500 * (126 - 33) + 500 * (200 - 256 - 33) == 2000 and 2000 / 1000 == 2.0
    assert not r["flags"][at] & abi.RF_LOWQ and r["n_frags"][at] == 1
    fr = f[r["frag_begin"][at]]
    assert (int(fr["start"]), int(fr["len"]), int(fr["flags"])) == (500, 500, 0)
    assert int(np.array(fr["sum_q"]).astype(np.int64)) == 500 * (200 - 256 - 33)
    assert ctr[abi.CTR_DROPINFO + 13] >= 1


def negative_kept_mean(lib_path, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    reads, p, at = negative_kept_mean_reads()
    for align in (16, 1):
        ctx = capi.Context(p, 0, lib_path)
        try:
            r, f, _ = parity.compare_batch(ctx, p, reads, align=align, explicit_lengths=align > 1)
            assert r["n_frags"][at] == 1 and f["flags"][r["frag_begin"][at]] == 0
        finally:
            ctx.close()


def kept_mean_outside_the_tables(lib_path, mode, monkeypatch):
    """The same reads with no upper bound on the mean quality.  The negative sum of the kept part stands as an unsigned
    one, a mean of about 3.7e16, which only max_q kept from the clean pass's table index: now the clean pass finds it
    outside [0,256) itself -- TGSF_E_DATA, the message names the read.  (With the filter off nothing is trimmed, so the
    kept part is the whole read and the raw pass has judged the same mean first.)"""
    set_mode(monkeypatch, mode)
    reads, p, at = negative_kept_mean_reads()
    p.max_q = 1e30
    ctx = capi.Context(p, 0, lib_path)
    try:
        seq, qual, off, ln = synth.pack(reads)
        raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "read %d:" % at, "mean quality outside [0,256)")
        ctx.reset_counters()
        parity.compare_batch(ctx, p, reads[:at] + reads[at + 1:], align=1)
    finally:
        ctx.close()


def fragment_capacity(lib_path, mode, monkeypatch):
    """tgsf_batch_out.frag_capacity: exactly the oracle's count is enough; one less, or no fragment buffer at all, is
    TGSF_E_CAPACITY from tgsf_wait with out->n_frags the count needed and out->reads complete; through tgsf_submit_device
    the device finds it.  Such a batch HAS been tallied in full (include/tgsf.h, tgsf_wait): retrying it counts it twice."""
    set_mode(monkeypatch, mode)
    reads = list(seam_reads())
    p = seam_params(reads)
    seq, qual, off, ln = synth.pack(reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        exp_r, exp_f, tally = orc.filter_batch(p, seq, qual, off, ln, n_bins=ctx.n_bins)
        nf = len(exp_f)
        assert nf > 64
        got_r, got_f = ctx.submit(seq, qual, off[:-1].copy(), ln, frag_capacity=nf)
        records_equal(got_r, got_f, exp_r, exp_f, "frag_capacity == n_frags")
        assert_tallies(ctx, tally, "frag_capacity == n_frags")
        off_n = off[:-1].copy()
        for cap, null in ((nf - 1, False), (nf, True), (0, False)):
            o_r = np.zeros(len(reads), dtype=abi.READ_RESULT_DTYPE)
            o_f = np.zeros(nf, dtype=abi.FRAGMENT_DTYPE)
            bi = abi.BatchIn(seq.ctypes.data, qual.ctypes.data, off_n.ctypes.data, ln.ctypes.data, len(reads), 0, seq.size, None)
            bo = abi.BatchOut(o_r.ctypes.data, None if null else o_f.ctypes.data, cap, 0)
            refused(ctx, ctx.lib.tgsf_submit(ctx.h, C.byref(bi), C.byref(bo)), abi.E_CAPACITY, "produced %d fragments" % nf, "room for %d" % cap)
            assert bo.n_frags == nf and np.array_equal(o_r, exp_r) and not o_f.view(np.uint8).any()
            tally = oracle_tallies(p, ctx.n_bins, reads, base=tally)
            assert_tallies(ctx, tally, "a batch refused for frag_capacity alone is tallied in full")
        dev = Dev(lib_path)
        db = DeviceBatch(dev, p, ctx.n_bins, reads, exp_ctr=tally.copy(), frag_room=0)
        dev.sync()
        refused(ctx, db.submit(ctx, fcap=nf - 1), abi.OK)
        refused(ctx, ctx.lib.tgsf_wait(ctx.h), abi.E_CAPACITY, "fragment capacity exceeded (%d)" % nf)
        assert_tallies(ctx, db.exp_ctr, "tgsf_submit_device, frag_capacity one too small")
        refused(ctx, db.submit(ctx), abi.OK)                      # the same buffers with room for all: the batch completes
        ctx.wait()
        db.check()
        tally = oracle_tallies(p, ctx.n_bins, reads, base=db.exp_ctr)
        assert_tallies(ctx, tally, "the batch once more, accepted")
        recover(ctx, p, tally)
    finally:
        ctx.close()


def refused_between_good(lib_path, what, mode, monkeypatch):
    """A refused batch between two good ones of by_product_run's shape: the device decides per batch whether the next one
    speculates (bp_state), also while it runs a batch that ends refused.  Whatever speculation state it left, the third
    and fourth batches' records and fragments are the oracle's.  tgsf_reset_counters comes between the refused batch and
    the third, so that their tallies can be compared too (a bad mean leaves an unspecified part of its batch); the next
    batch WITHOUT a reset is recover()'s first step, after every device-side refusal."""
    set_mode(monkeypatch, mode)
    sets = [synth.make_reads(300 + 7 * b + HEAD, 40, "ont", mean_len=3000 + 2500 * b, zoo=(b == 1), pmid=0.05 if b else 0.0, p5=0.8) for b in range(2)]
    p = seam_params(sets[0] + sets[1])
    ctx = capi.Context(p, 0, lib_path)
    try:
        _, _, base = parity.compare_batch(ctx, p, sets[0])
        bad = list(sets[1])
        seq, qual, off, ln = synth.pack(bad)
        if what == "length":
            ln[5] = 0
            raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "read 5:", "length 0")
        else:
            bad[5] = (bad[5][0], bad[5][1], bytes([200]) * len(bad[5][2]))
            seq, qual, off, ln = synth.pack(bad)
            raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "read 5:", "mean quality")
        ctx.reset_counters()
        _, _, base = parity.compare_batch(ctx, p, sets[1], align=1)
        parity.compare_batch(ctx, p, sets[0], base=base)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the enqueue limit of tgsf_submit_device
# ---------------------------------------------------------------------------------------------------------------------
def enqueue_limit(lib_path):
    """TGSF_MAX_ENQUEUED + 1 batches of 8 reads through tgsf_submit_device without a tgsf_wait: the last call closes the
    books of the first 64 itself.  After tgsf_wait all 65 record and fragment sets and the summed tallies are the oracle's."""
    n_batches = abi.MAX_ENQUEUED + 1
    sets = [synth.make_reads(500 + b, 8, "ont", mean_len=500, max_len=3000, zoo=True, p5=0.5) for b in range(n_batches)]
    p = seam_params([r for s in sets for r in s][:8], max_read_len=3000)
    p.max_batch_bases = 8 * 3000 + 64
    ctx = capi.Context(p, 0, lib_path)
    try:
        dev = Dev(lib_path)
        exp, batches = None, []
        for s in sets:
            batches.append(DeviceBatch(dev, p, ctx.n_bins, s, exp_ctr=exp))
            exp = batches[-1].exp_ctr.copy()
        dev.sync()
        for b in batches:
            refused(ctx, b.submit(ctx), abi.OK)
        ctx.wait()
        for b in batches:
            b.check()
        assert_tallies(ctx, exp, "65 batches, one wait")
    finally:
        ctx.close()


def enqueue_limit_needs_wait(lib_path, monkeypatch):
    """The same with a pool of one candidate slot and a homopolymer read against homopolymer adapters in an early batch:
    that batch has to be run again from its inputs, which only tgsf_wait does -- the 65th call is TGSF_E_INVALID and says
    so.  After tgsf_wait and tgsf_reset_counters the context passes compare_batch."""
    monkeypatch.setenv("TGSF_POOL_CAP", "1")
    n_batches = abi.MAX_ENQUEUED + 1
    sets = [synth.make_reads(600 + b, 8, "ont", mean_len=500, max_len=3000, zoo=False, pmid=0.0, p5=0.0) for b in range(n_batches)]
    sets[2][4] = (b"polyA", b"A" * 2000, bytes([33 + 20]) * 2000)
    p = seam_params(sets[0], max_read_len=3000, adapters=[b"A" * 50, b"T" * 50])
    p.max_batch_bases = 8 * 3000 + 64
    ctx = capi.Context(p, 0, lib_path)
    try:
        dev = Dev(lib_path)
        batches = [DeviceBatch(dev, p, ctx.n_bins, s) for s in sets]
        dev.sync()
        for b in batches[:-1]:
            refused(ctx, b.submit(ctx), abi.OK)
        refused(ctx, batches[-1].submit(ctx), abi.E_INVALID, "call tgsf_wait", "has to be run again")
        ctx.wait()
        ctx.reset_counters()
        assert not ctx.counters().any()
        _, _, base = parity.compare_batch(ctx, p, sets[2])
        parity.compare_batch(ctx, p, sets[0], align=1, explicit_lengths=False, base=base)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. fetching and merging the tallies
# ---------------------------------------------------------------------------------------------------------------------
class _DevicePointer:
    """A device address as torch.as_tensor takes it (the CUDA array interface), int64 words."""

    def __init__(self, ptr, n_words):
        self.__cuda_array_interface__ = {"shape": (int(n_words),), "typestr": "<i8", "data": (int(ptr), False), "version": 2, "strides": None}


def read_device_words(lib_path, ptr, n_words):
    if lib_path is not None:                           # the emulation's device memory is host memory
        return np.frombuffer(C.string_at(ptr, n_words * 8), dtype=np.uint64).copy()
    import torch
    return torch.as_tensor(_DevicePointer(ptr, n_words), device=torch.device("cuda", 0)).cpu().numpy().view(np.uint64).copy()


def fetch_and_merge(lib_path):
    """tgsf_counters_used, tgsf_counters_merge, tgsf_counters_device and tgsf_reset_counters against the oracle, on
    contexts with far more rows (2 501) than their reads use."""
    SENT = np.uint64(0x5EA75EA75EA75EA7)
    ra = synth.make_reads(701, 30, "ont", mean_len=6000, max_len=19000, zoo=True, pmid=0.2)
    ra.append((b"long", np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, 19950)].tobytes(), bytes([33 + 20]) * 19950))
    rb = synth.make_reads(702, 40, "ont", mean_len=1200, max_len=3000, zoo=True, pmid=0.2)
    p = seam_params(ra + rb, max_read_len=250_000)
    a, b = capi.Context(p, 0, lib_path), capi.Context(p, 0, lib_path)
    try:
        assert a.n_bins == 2501
        _, _, ea = parity.compare_batch(a, p, ra)
        _, _, eb = parity.compare_batch(b, p, rb, align=1)
        rows = abi.CTR_ROWS
        assert ea[rows] == 200 and eb[rows] <= 31 and ea[rows + 1] > eb[rows + 1] > 0

        def check_used(ctx, full):
            for with_rows in (True, False):
                buf = np.full(ctx.ctr_words, SENT, dtype=np.uint64)
                out, used = ctx.counters_used(buf, with_rows=with_rows)
                assert out is buf
                if with_rows:
                    assert used == (int(full[rows]), int(full[rows + 1]))
                head = abi.ctr_bin_table(0, ctx.bc_len, ctx.n_bins)
                assert np.array_equal(buf[:head], full[:head])
                for t in range(4):
                    at, r = abi.ctr_bin_table(t, ctx.bc_len, ctx.n_bins), int(full[rows + (t >> 1)])
                    assert np.array_equal(buf[at:at + 5 * r], full[at:at + 5 * r])
                    assert (buf[at + 5 * r:at + 5 * ctx.n_bins] == SENT).all()
                    assert not full[at + 5 * r:at + 5 * ctx.n_bins].any()
        check_used(a, ea)
        check_used(b, eb)

        both = oracle_tallies(p, a.n_bins, rb, base=ea)                     # the oracle over both batches into one vector
        a.merge_from(b)
        assert_tallies(a, both, "merge")
        assert_tallies(b, eb, "the source of a merge keeps its own")
        assert all(both[rows + k] == max(ea[rows + k], eb[rows + k]) for k in range(4))
        check_used(a, both)
        a.merge_from(b)
        twice = both + eb
        twice[rows:rows + 4] = both[rows:rows + 4]                         # sums double, the four maxima stay
        assert_tallies(a, twice, "merge, again")
        assert_tallies(b, eb, "the source of a merge keeps its own")

        ptr, n_words = a.counters_device_ptr()
        assert n_words == a.ctr_words
        a.wait()
        assert np.array_equal(read_device_words(lib_path, ptr, n_words), twice)

        b.merge_from(a)                                                    # the other direction: the larger rows arrive
        eb2 = eb + twice
        eb2[rows:rows + 4] = np.maximum(eb[rows:rows + 4], twice[rows:rows + 4])
        assert_tallies(b, eb2, "merge into the context with fewer rows in use")
        check_used(b, eb2)

        a.reset_counters()
        buf = np.full(a.ctr_words, SENT, dtype=np.uint64)
        _, used = a.counters_used(buf)
        head = abi.ctr_bin_table(0, a.bc_len, a.n_bins)
        assert used == (0, 0) and not buf[:head].any() and (buf[head:] == SENT).all()
        assert not read_device_words(lib_path, ptr, n_words).any()
        parity.compare_batch(a, p, rb)                                     # ... and counts from zero again
    finally:
        a.close()
        b.close()


def refusal_through_other_calls(lib_path):
    """tgsf_counters, tgsf_counters_used and tgsf_counters_merge wait for the context (for both contexts), so a batch
    still pending is refused through THEM, with tgsf_wait's code and message -- a merge puts the source's message on the
    destination and adds nothing."""
    good = synth.make_reads(93, 24, "ont", mean_len=1200, max_len=4000, zoo=True)
    p = seam_params(good)
    seq, qual, off, ln = synth.pack(good)
    bad = ln.copy()
    bad[2] = 0
    a, b = capi.Context(p, 0, lib_path), capi.Context(p, 0, lib_path)
    try:
        _, _, ea = parity.compare_batch(a, p, good)
        b.submit_async(seq, qual, off[:-1].copy(), bad)
        raises(lambda: a.merge_from(b), abi.E_DATA, "read 2:", "length 0")
        assert_tallies(a, ea, "a merge refused for the source's pending batch")
        b.submit_async(seq, qual, off[:-1].copy(), bad)
        raises(b.counters, abi.E_DATA, "read 2:", "length 0")
        b.submit_async(seq, qual, off[:-1].copy(), bad)
        raises(b.counters_used, abi.E_DATA, "read 2:", "length 0")
        b.reset_counters()
        parity.compare_batch(b, p, good, align=1)
    finally:
        a.close()
        b.close()


def device_out_of_range(lib_path):
    """tgsf_create on a device index that does not exist: TGSF_E_NO_DEVICE, and the message says how many there are."""
    p = abi.make_params("ont", adapters=ADS, max_batch_bases=1000, max_batch_reads=4, max_read_len=500)
    for device in (-1, 4096):
        raises(lambda: capi.Context(p, device, lib_path), abi.E_NO_DEVICE, "device %d out of range" % device)
