"""Sizing and layout independence: the sizing hints of tgsf_params (max_batch_bases, max_batch_reads, max_read_len) select
code paths in libtgsf, not only buffer sizes -- the LDS or the global tile histogram, k_tail_fix's memory path, the
capacities every per-chunk buffer and the flat schedule's grid come from -- and the command line never creates a context
cut to fit its batch (tgsfilter_amd/host/run_contexts.cpp, run_second_pass.cpp).  Here small workloads go through contexts
sized as the product sizes them, in the layouts the product submits, and every record, fragment and tally word is the
oracle's at the context's own n_bins.  No tolerance anywhere.  Every check takes `lib_path` -- the emulation's path on a
GPU-less box, None for the HIP build -- in the style of tests/parity.py (tests/test_sizing_emul.py, tests/test_sizing_gpu.py)."""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import re

import numpy as np

from oracle import orc
from tests import parity, refusals
from tgsfilter_amd import abi, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tgsfilter_amd", "csrc")

ONT = [synth.ONT_RAPID, synth.ONT_RAPID_RC]
HIFI = [synth.PACBIO_BLUNT, synth.PACBIO_BLUNT_RC]
LIGATION_28 = b"AATGTACTTCGTTCAGTTACGTATTGCT"        # src/TGSFilter.cpp:2974-2977
LIGATION_22 = [b"GCAATACGTAACTGAACGAAGT", b"ACTTCGTTCAGTTACGTATTGC"]
KNOBS = ("TGSF_CLEAN_TABLES", "TGSF_REP_MAX_PLOG", "TGSF_POOL_CAP", "TGSF_MID_FLAT")


def _constant(header, name):
    """An integer `constexpr` of the kernel sources (a literal, or a product of other such constants)."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, (header, name)
    val = 1
    for f in m.group(1).split("*"):
        f = f.strip().rstrip("uU")
        val *= int(f) if f.isdigit() else _constant(header, f)
    return val


TILE_BASES = _constant("tgsf_core.h", "kTileBases")            # 6 400
HIST_LDS = _constant("tgsf_kernels.h", "kHistLds")             # 4 096 buckets of a block's LDS histogram
BATCH_READS = 1 << 16                                          # run_contexts.cpp: batch_reads
STREAMED_READ_LEN = 1 << 26                                    # run_contexts.cpp: max_read_len of every streamed input
STREAMED_CHUNK = 64 << 20                                      # run.h: chunk_bytes, a streamed input's batch_text

# max_read_len on either side of the histogram's switch: one segment (the raw pass without the by-product), and the two
# segments of the clean pass and of the by-product's raw pass
SEAMS = {"seam1_lds": (26_201_600, 1), "seam1_mem": (26_201_601, 1), "seam2_lds": (13_094_400, 2), "seam2_mem": (13_094_401, 2)}
BASIC = ("exact", "indexed", "streamed")
ALL = BASIC + tuple(SEAMS) + ("second_pass",)


def buckets(max_read_len, segments):
    """nbuck of k_prepare / k_frag_prepare / k_tile_scatter: (max_tiles + 2) x segments."""
    return ((max_read_len + TILE_BASES - 1) // TILE_BASES + 2) * segments


def seams_sit_on_the_switch():
    """A later change of kTileBases or kHistLds fails here instead of moving the seam sizings off the seam: the last count
    the LDS holds, and the first one past it (4 097 with one segment, 4 098 with two: the count is a multiple of them)."""
    for name, (max_read_len, segments) in SEAMS.items():
        assert buckets(max_read_len, segments) == HIST_LDS + (segments if name.endswith("_mem") else 0), (name, buckets(max_read_len, segments))
    assert buckets(STREAMED_READ_LEN, 1) > 2 * HIST_LDS


def text_bytes(reads):
    return sum(len(n) + 2 * len(s) + 6 for n, s, _ in reads)


def product_batch_reads(p):
    """run_contexts.cpp: 65 536 reads a batch, fewer where the traceback scratch of the adapters would pass 4 GB."""
    cols, words = 0, 1
    for a in range(p.n_adapters):
        q = p.adapter_len[a]
        kmax = max(0, min(q - 1, max(q - p.end_match_len + 1, q - p.mid_match_len + 1)))
        cols = max(cols, q + kmax + 2)
        words = max(words, (q + 63) // 64 if q > 256 else 4 if q > 128 else 2 if q > 64 else 1)
    per_read = cols * 2 * words * 8
    if words > 4:
        per_read = min(per_read, (1 << 20) + 16 * words) + 32 * words + 512
    per_read *= 3 * max(p.n_adapters, 1)
    return min(BATCH_READS, max(256, (4 << 30) // per_read)) if per_read else BATCH_READS


def size(p, reads, name):
    """The sizing hints `name` stands for, for a batch of `reads`."""
    if name == "exact":
        return parity.sized(p, reads)
    longest = max(len(r[1]) for r in reads)
    batch_text = min(256 << 20, max(text_bytes(reads) // 8 + 4096, 1 << 16))
    p.max_batch_reads = product_batch_reads(p)
    if name == "indexed":
        p.max_read_len = max(longest, 1024)
    elif name == "streamed":
        p.max_read_len, batch_text = STREAMED_READ_LEN, STREAMED_CHUNK
    elif name in SEAMS:
        p.max_read_len = SEAMS[name][0]
    else:
        assert name == "second_pass", name
        p.max_read_len, p.max_batch_reads, p.max_batch_bases = max(longest, 1024), BATCH_READS, 1 << 30
        return p
    p.max_batch_bases = max(batch_text, 2 * p.max_read_len + (1 << 16)) + (1 << 20)
    return p


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# workloads: small, because the code under test is selected by the hints
# ---------------------------------------------------------------------------------------------------------------------
def _random_read(rng, name, L):
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
    return (name, s, (rng.integers(5, 40, L) + 33).astype(np.uint8).tobytes())


@functools.lru_cache(maxsize=None)
def reads_of(what):
    if what == "ont":
        return synth.make_reads(211, 60, "ont", mean_len=3000, zoo=True, pmid=0.1)
    if what == "hifi":
        return synth.make_reads(212, 48, "hifi", mean_len=4000, zoo=True, pmid=0.3)
    if what == "ligation":
        return synth.make_reads(213, 50, "ont", mean_len=2500, zoo=True, pmid=0.3, adapter=LIGATION_28)
    if what == "repeat":
        return parity.repeat_reads(seed=214, n=40)
    if what == "soft_masked":
        rng = np.random.default_rng(215)
        out = []
        for i, (name, s, q) in enumerate(synth.make_reads(215, 50, "ont", mean_len=2500, zoo=True, pmid=0.1)):
            b = np.frombuffer(s, dtype=np.uint8).copy()
            if i % 2 == 0:                             # lower case over both ends and the middle: the reference's quirks at the read ends
                for lo in (0, max(len(b) - 40, 0), len(b) // 2):
                    m = rng.random(len(b[lo:lo + 40])) < 0.7
                    b[lo:lo + 40][m] |= 0x20
            out.append((name, b.tobytes(), q))
        return out
    if what == "edge":
        from tests.test_gpu_parity import _edge_reads
        return _edge_reads() + [long_read()]
    if what == "high_bytes":
        return parity.high_quality_byte_reads(seed=217, n=40, kind="ont")
    if what == "adapter150":
        from tests import fuzz
        return synth.make_reads(218, 40, "ont", mean_len=2500, zoo=True, pmid=0.3, adapter=fuzz.LIB_ADAPTERS[8])
    raise KeyError(what)


@functools.lru_cache(maxsize=None)
def long_read(L=300_000):
    rng = np.random.default_rng(216)
    name, s, q = _random_read(rng, b"long300k", L)
    s = bytearray(s)
    for frac in (0.3, 0.7):
        a = synth.mutate(rng, synth.ONT_RAPID_RC, 0.04)
        s[int(L * frac):int(L * frac) + len(a)] = a
    return (name, bytes(s), q)


def _adapter150():
    from tests import fuzz
    return [fuzz.LIB_ADAPTERS[8]]


# name: (kind, reads, environment, parameters)
WORKLOADS = {
    "1_ont_trims_byproduct": ("ont", "ont", {"TGSF_CLEAN_TABLES": "byproduct"}, dict(adapters=ONT, head_trim=79, tail_trim=13, min_q=9.0)),
    "1_ont_trims": ("ont", "ont", {}, dict(adapters=ONT, head_trim=79, tail_trim=13, min_q=9.0)),
    "2_hifi": ("hifi", "hifi", {}, dict(adapters=HIFI, min_q=20.0)),
    "2_hifi_direct": ("hifi", "hifi", {"TGSF_CLEAN_TABLES": "direct"}, dict(adapters=HIFI, min_q=20.0)),
    "3_ligation_M14": ("ont", "ligation", {}, dict(adapters=[LIGATION_22[0], LIGATION_28], mid_match_len=14, min_q=8.0)),
    "4_repeat_k11": ("ont", "repeat", {}, dict(adapters=ONT, min_q=10.0, min_repeat=60, kmer=11)),
    "4_repeat_k15": ("ont", "repeat", {}, dict(adapters=ONT, min_q=10.0, min_repeat=60, kmer=15)),
    "4_repeat_k31_in_memory": ("ont", "repeat", {"TGSF_REP_MAX_PLOG": "0"}, dict(adapters=ONT, min_q=10.0, min_repeat=60, kmer=31)),
    "5_no_qual": ("ont", "soft_masked", {}, dict(adapters=ONT, min_q=10.0, head_trim=3, no_qual=True)),
    "6_filter_off": ("hifi", "hifi", {}, dict(adapters=HIFI, filter=False)),
    "6_only_qc": ("ont", "ont", {}, dict(adapters=ONT, only_qc=True)),
    "7_edge_lengths": ("ont", "edge", {}, dict(adapters=ONT, min_q=7.0, min_len=100, head_trim=3, tail_trim=2)),
    "8_high_quality_bytes": ("ont", "high_bytes", {}, dict(adapters=ONT, min_q=7.0, head_trim=13, tail_trim=4)),
    "9_adapter_150bp": ("ont", "adapter150", {}, dict(adapters=None, min_q=8.0, mid_match_len=100)),
}
EVERYWHERE = ("1_ont_trims_byproduct", "1_ont_trims", "2_hifi", "2_hifi_direct", "4_repeat_k11", "4_repeat_k15", "4_repeat_k31_in_memory", "7_edge_lengths")
CASES = [(w, s) for w in WORKLOADS for s in (ALL if w in EVERYWHERE else BASIC)]


def workload(name):
    kind, what, env, kw = WORKLOADS[name]
    kw = dict(kw)
    if kw["adapters"] is None:
        kw["adapters"] = _adapter150()
    return kind, reads_of(what), env, kw


_first = {}


def same_as_at_other_sizings(key, got_r, got_f, sizing):
    """Records and fragments of one workload are byte-identical whatever the context was sized for."""
    first = _first.setdefault(key, (sizing, got_r.tobytes(), got_f.tobytes()))
    assert first[1] == got_r.tobytes() and first[2] == got_f.tobytes(), f"{key}: records at {sizing} differ from those at {first[0]}"


def check_geometry(ctx, p, sizing):
    assert ctx.n_bins == abi.n_bins(p.max_read_len)
    if sizing == "streamed":
        assert ctx.n_bins == 671_089 and p.max_batch_bases > (8 << 20)     # k_tail_fix's memory path, the pinned staging path
    if sizing in SEAMS:
        assert p.max_read_len == SEAMS[sizing][0] and ctx.n_bins > 1024


def workload_at(lib_path, wname, sizing, monkeypatch):
    seams_sit_on_the_switch()
    kind, reads, env, kw = workload(wname)
    set_env(monkeypatch, env)
    p = size(abi.make_params(kind, **kw), reads, sizing)
    ctx = capi.Context(p, 0, lib_path)
    try:
        check_geometry(ctx, p, sizing)
        got_r, got_f, _ = parity.compare_batch(ctx, p, reads)
    finally:
        ctx.close()
    same_as_at_other_sizings((lib_path, wname), got_r, got_f, sizing)


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
class LaidOut(refusals.DeviceBatch):
    """A batch in any layout in 'device' memory (refusals.Dev), and the oracle's answer to it on that layout."""

    def __init__(self, dev, p, n_bins, seq, qual, off, ln, exp_ctr=None, frag_room=16):
        self.exp_r, self.exp_f, self.exp_ctr = orc.filter_batch(p, seq, qual, off, ln, n_bins=n_bins, ctr=exp_ctr)
        self.n, self.n_bytes, self.dev = len(ln), seq.size, dev
        self.fcap = len(self.exp_f) + frag_room
        self.seq, self.qual = dev.put(seq), dev.put(qual)
        self.off, self.len = dev.put(off[:self.n].astype(np.uint64)), dev.put(ln.astype(np.uint32))
        self.o_r = dev.zeros(self.n * abi.READ_RESULT_DTYPE.itemsize)
        self.o_f = dev.zeros(self.fcap * abi.FRAGMENT_DTYPE.itemsize)
        self.o_n = dev.zeros(16)

    def submit(self, ctx, fcap=None, stream=None):
        bi, bo = self.structs(fcap)
        return ctx.lib.tgsf_submit_device(ctx.h, C.byref(bi), C.byref(bo), self.o_n[0], stream)


def caller_stream(dev):
    """A stream of the caller's own (the emulation has none: NULL)."""
    if dev.torch is None:
        return None, None
    st = dev.torch.cuda.Stream(device=dev.dev)
    return st, st.cuda_stream


@functools.lru_cache(maxsize=1)
def _other_bases(nbytes=96 << 20):
    rng = np.random.default_rng(4)
    return (np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, nbytes, dtype=np.uint8)],
            rng.integers(33 + 2, 33 + 41, nbytes, dtype=np.uint8))


def scatter(reads, seed=5):
    """The reads at random offsets of a 96-MiB buffer of other bases, out of address order, every other one on 16 bytes."""
    seq, qual = (a.copy() for a in _other_bases())
    n = len(reads)
    rng = np.random.default_rng(seed)
    slot, place = seq.size // n, rng.permutation(n)
    off = np.zeros(n, dtype=np.uint64)
    ln = np.array([len(r[1]) for r in reads], dtype=np.uint32)
    for i, (_, s, q) in enumerate(reads):
        L = len(s)
        assert L + 64 < slot
        at = (int(place[i]) * slot + int(rng.integers(16, slot - L - 32))) & ~15
        if i % 2:
            at += int(rng.integers(1, 16))
        seq[at:at + L] = np.frombuffer(s, dtype=np.uint8)
        qual[at:at + L] = np.frombuffer(q, dtype=np.uint8)
        off[i] = at
    assert (np.diff(off.astype(np.int64)) < 0).sum() > n // 4 and (off % 16 == 0).sum() == (n + 1) // 2
    return seq, qual, off, ln


def host_batch(ctx, p, seq, qual, off, ln, base):
    got_r, got_f = ctx.submit(seq, qual, off, ln)
    exp_r, exp_f, exp = orc.filter_batch(p, seq, qual, off, ln, n_bins=ctx.n_bins, ctr=base.copy())
    refusals.records_equal(got_r, got_f, exp_r, exp_f, "host batch")
    refusals.assert_tallies(ctx, exp, "host batch")
    return got_r, got_f, exp


def layouts_at_streamed(lib_path, wname, monkeypatch):
    """Scattered reads (n_bytes the whole buffer) through tgsf_submit and tgsf_submit_device, then the same reads as
    FASTQ text in place -- one context sized as for a streamed input, the tallies running."""
    kind, reads, env, kw = workload(wname)
    set_env(monkeypatch, env)
    p = size(abi.make_params(kind, **kw), reads, "streamed")
    seq, qual, off, ln = scatter(reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        assert seq.size > p.max_batch_bases // 2 and seq.size <= p.max_batch_bases + 16 * p.max_batch_reads
        got_r, got_f, tally = host_batch(ctx, p, seq, qual, off, ln, np.zeros(ctx.ctr_words, dtype=np.uint64))
        same_as_at_other_sizings((lib_path, wname), got_r, got_f, "streamed, scattered")
        dev = refusals.Dev(lib_path)
        db = LaidOut(dev, p, ctx.n_bins, seq, qual, off, ln, exp_ctr=tally.copy())
        dev.sync()
        assert db.seq[0] % 16 == 0 and db.qual[0] % 16 == 0
        refusals.refused(ctx, db.submit(ctx), abi.OK)
        ctx.wait()
        db.check()
        refusals.assert_tallies(ctx, db.exp_ctr, "scattered, tgsf_submit_device")
        got_r, got_f, _ = parity.compare_batch_in_place(ctx, p, reads, base=db.exp_ctr)
        same_as_at_other_sizings((lib_path, wname), got_r, got_f, "streamed, FASTQ text in place")
    finally:
        ctx.close()


def largest_batch(seed=7, n=2048, cap_bases=2048 * 40, adapters=tuple(LIGATION_22)):
    """n unaligned reads of 33..81 bases packed end to end, cap_bases + 16 n bytes in all and every byte a base: the
    largest span a context of (cap_bases, n) accepts, with the most chunks per base a batch can have."""
    total = cap_bases + 16 * n
    rng = np.random.default_rng(seed)
    # lengths of 16 m + 1 bases: one base in the last chunk of every window, (n_bytes + 15 n) / 16 chunks in all -- no batch
    # of this span and this many reads has more
    assert (n, cap_bases) == (2048, 2048 * 40)
    lens = rng.permutation(np.repeat([33, 49, 65, 81], [256, 896, 640, 256]))
    assert lens.sum() == total and ((lens + 15) // 16).sum() == (total + 15 * n) // 16
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total)].copy()
    for i in range(0, n, 3):                               # an adapter, some with a difference, in a third of the reads
        a = np.frombuffer(adapters[(i // 3) % len(adapters)], dtype=np.uint8).copy()
        if i % 2:
            a[int(rng.integers(0, a.size))] = ord("A")
        at = int(off[i]) + int(rng.integers(0, lens[i] - a.size + 1))
        seq[at:at + a.size] = a
    qual = (rng.integers(8, 40, total) + 33).astype(np.uint8)
    assert seq.size == total == int(off[-1]) and (off[:-1] % 16 != 0).sum() > n // 2
    return seq, qual, off, lens.astype(np.uint32)


# four adapters of 33 bp, the shortest the 32-row filter of k_mid_flat takes (and no longer than the batch's shortest read):
# one filtering pass of four, the chunk marks of the fourth last in their buffer
FOUR_33 = [a[:33] for a in HIFI + ONT]


def largest_accepted_batch(lib_path, mid_flat, monkeypatch, adapters=None, mid_match_len=14):
    """The batch the capacity bound of tgsf_submit_device has to be safe for, through both entry points."""
    set_env(monkeypatch, {} if mid_flat is None else {"TGSF_MID_FLAT": mid_flat})
    n, cap_bases = 2048, 2048 * 40
    adapters = adapters or LIGATION_22
    p = abi.make_params("ont", adapters=adapters, mid_match_len=mid_match_len, end_len=0, min_q=7.0, min_len=100,
                        max_batch_reads=n, max_batch_bases=cap_bases, max_read_len=4096)
    seq, qual, off, ln = largest_batch(n=n, cap_bases=cap_bases, adapters=tuple(adapters))
    assert seq.size == p.max_batch_bases + 16 * p.max_batch_reads
    ctx = capi.Context(p, 0, lib_path)
    try:
        got_r, got_f = ctx.submit(seq, qual, off, None)                  # implicit lengths: packed end to end
        exp_r, exp_f, tally = orc.filter_batch(p, seq, qual, off, None, n_bins=ctx.n_bins)
        refusals.records_equal(got_r, got_f, exp_r, exp_f, "the largest accepted batch")
        refusals.assert_tallies(ctx, tally, "the largest accepted batch")
        assert (exp_r["flags"] & abi.RF_ADMID).sum() > n // 8               # the middle scan found what was planted
        dev = refusals.Dev(lib_path)
        db = LaidOut(dev, p, ctx.n_bins, seq, qual, off, ln, exp_ctr=tally.copy())
        dev.sync()
        refusals.refused(ctx, db.submit(ctx), abi.OK)
        ctx.wait()
        db.check()
        refusals.assert_tallies(ctx, db.exp_ctr, "the largest accepted batch, tgsf_submit_device")
        # one byte more is refused, nothing enqueued
        bi, bo = db.structs()
        bi.n_bytes += 1
        refusals.refused(ctx, ctx.lib.tgsf_submit_device(ctx.h, C.byref(bi), C.byref(bo), db.o_n[0], None), abi.E_CAPACITY, "spans %u bytes" % (seq.size + 1))
        refusals.refused(ctx, ctx.lib.tgsf_wait(ctx.h), abi.OK)
        refusals.assert_tallies(ctx, db.exp_ctr, "after the refusal")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# a long-lived context
# ---------------------------------------------------------------------------------------------------------------------
HOMOPOLYMER = [b"A" * 50, b"T" * 50]


def long_lived_batches(kind, overflow):
    """What one streamed context takes without a reset.  kind 1: ONT with trims (the by-product's state goes from batch to
    batch); kind 2: HiFi.  overflow: with the batch whose candidate pool overflows (None in its place otherwise)."""
    from tests.test_gpu_parity import _edge_reads
    if kind == 1:
        w = reads_of("ont")
        rng = np.random.default_rng(77)
        busy = [(b"polyA", b"A" * 200_000, bytes((rng.integers(15, 35, 200_000) + 33).astype(np.uint8)))] + list(w[:3])
    else:
        w = reads_of("hifi")
        # (the pool has grown to the first batch's candidates and a thousand by then: a read studded with 1 500 adapters)
        rng = np.random.default_rng(78)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        s = b"".join(HIFI[i & 1] + acgt[rng.integers(0, 4, 15)].tobytes() for i in range(1500))
        busy = [(b"studded", s, bytes((rng.integers(25, 40, len(s)) + 33).astype(np.uint8)))] + list(w[:3])
    return [w, w[:3], [long_read()], w, busy if overflow else None, w, _edge_reads()]


def long_lived_params(kind, overflow, monkeypatch):
    """kind 1's pool of a streamed context holds millions of candidates, more than a 200-kb homopolymer read has tied
    columns: a pool of 65 536 slots (a small context's) makes that read outgrow it; kind 2: three slots."""
    set_env(monkeypatch, {"TGSF_POOL_CAP": "65536" if kind == 1 else "3"} if overflow else {})
    monkeypatch.setenv("TGSF_TRACE_POOL", "1")
    if kind == 1:
        return abi.make_params("ont", adapters=ONT + HOMOPOLYMER, head_trim=79, tail_trim=13, min_q=9.0, min_len=100)
    return abi.make_params("hifi", adapters=HIFI, min_q=20.0, min_len=100)


def long_lived_host(lib_path, kind, monkeypatch, capfd):
    """Seven batches, a tgsf_wait after each: every batch's records and fragments and the running tallies are the oracle's."""
    p = long_lived_params(kind, True, monkeypatch)
    sets = long_lived_batches(kind, True)
    size(p, sets[0], "streamed")
    ctx = capi.Context(p, 0, lib_path)
    try:
        base = None
        for k, reads in enumerate(sets):
            if k == 4:
                capfd.readouterr()
            _, _, base = parity.compare_batch(ctx, p, reads, align=16 if k % 2 == 0 else 1, explicit_lengths=k % 2 == 0, base=base)
            if k == 4:
                err = capfd.readouterr().err
                assert "candidate pool overflow" in err and "(grown)" in err, err[-400:]
    finally:
        ctx.close()


def long_lived_enqueued(lib_path, kind, overflow, monkeypatch):
    """The same batches back to back through tgsf_submit_device on one caller stream, one tgsf_wait at the end: the
    by-product's state (bp_state, bp_ring) goes from batch to batch on the device alone; with `overflow`, tgsf_wait runs
    one batch again after its successors have run."""
    p = long_lived_params(kind, overflow, monkeypatch)
    sets = [s for s in long_lived_batches(kind, overflow) if s is not None]
    size(p, sets[0], "streamed")
    ctx = capi.Context(p, 0, lib_path)
    try:
        dev = refusals.Dev(lib_path)
        exp, batches = None, []
        for k, reads in enumerate(sets):
            seq, qual, off, ln = synth.pack(reads, align=16 if k % 2 == 0 else 1)
            batches.append(LaidOut(dev, p, ctx.n_bins, seq, qual, off, ln, exp_ctr=exp))
            exp = batches[-1].exp_ctr.copy()
        dev.sync()
        keep, st = caller_stream(dev)
        for b in batches:
            refusals.refused(ctx, b.submit(ctx, stream=st), abi.OK)
        ctx.wait()
        dev.sync()
        for b in batches:
            b.check()
        refusals.assert_tallies(ctx, exp, "%d batches enqueued together" % len(batches))
        del keep
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# stage timing
# ---------------------------------------------------------------------------------------------------------------------
def stage_timing(lib_path, n_batches=70):
    """tgsf_profile / tgsf_stage_times over more batches than the ring of event sets holds (kProfRing = 64: the harvest
    inside run_pipeline runs): results as with profiling off, every batch counted, times finite; switched off, further
    batches leave the counts alone.  No thresholds on the times themselves."""
    sets = [synth.make_reads(500 + b, 8, "ont", mean_len=500, max_len=3000, zoo=True, p5=0.5, pmid=0.3) for b in range(n_batches)]
    p = refusals.seam_params(sets[0], max_read_len=3000)
    p.max_batch_bases = 8 * 3000 + 64
    out = []
    for profiled in (False, True):
        ctx = capi.Context(p, 0, lib_path)
        try:
            if profiled:
                ctx.profile(True)
            res = []
            for s in sets:
                seq, qual, off, ln = synth.pack(s)
                r, f = ctx.submit(seq, qual, off[:-1].copy(), ln)
                res.append((r.tobytes(), f.tobytes()))
            out.append((res, ctx.counters()))
            if profiled:
                times, n = ctx.stage_times()
                assert n == n_batches and len(times) == abi.N_STAGES, (n, times)
                assert all(math.isfinite(v) and v >= 0.0 for v in times.values()), times
                assert times["stats_raw"] > 0.0 and times["mid_scan"] > 0.0, times
                ctx.profile(False)
                assert ctx.stage_times() == (dict.fromkeys(times, 0.0), 0)
                for s in sets[:3]:
                    seq, qual, off, ln = synth.pack(s)
                    ctx.submit(seq, qual, off[:-1].copy(), ln)
                assert ctx.stage_times() == (dict.fromkeys(times, 0.0), 0)
        finally:
            ctx.close()
    assert out[0][0] == out[1][0], "records or fragments differ with profiling on"
    assert np.array_equal(out[0][1], out[1][1]), "tallies differ with profiling on"
    exp = None
    for k, reads in enumerate(sets[:4]):                    # (and they are the oracle's)
        seq, qual, off, ln = synth.pack(reads)
        exp_r, exp_f, exp = orc.filter_batch(p, seq, qual, off, ln, n_bins=abi.n_bins(p.max_read_len), ctr=exp)
        assert out[1][0][k] == (exp_r.tobytes(), exp_f.tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------------------------------
def fuzz_under_sizings(lib_path, seeds, n_reads, monkeypatch):
    from tests import fuzz
    for k in ("TGSF_FUZZ_WIDE", "TGSF_FUZZ_TRIMS", "TGSF_FUZZ_SIZING"):
        monkeypatch.setenv(k, "1")
    drawn = set()
    for seed in seeds:
        drawn.add(fuzz.random_case(seed, 1)[2]["_sizing"])
        fuzz.run_case(lib_path, seed, n_reads)
    assert {"exact", "indexed", "streamed"} <= drawn and drawn & set(SEAMS), drawn
