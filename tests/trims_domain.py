"""The trim domain: fixed 5' and 3' trims (-5 / -3) across their range and at the scale of a product batch.

With a fixed trim the clean tables come as a by-product of the raw pass: k_prepare speculates that a read is kept as
[head_trim, L - tail_trim), k_stats<raw, BP> tallies that range into the clean tables with its split bins while it holds the
bytes, k_tail_fix tallies the tail_trim bytes behind it, the work list has two segments, and k_clean_plan_next decides
whether the next batch speculates.  It is the path of the product's own workload -- and the rest of the suite runs it with
trims of at most 250 / 120 and batches of at most 600 reads, where k_tail_fix is one block and its grid never wraps.  Here:

  B1  pairs of trims on the seams of bins (100) and tiles (6 400), tails of several rows and of more than a tile, tables
      longer than k_tail_fix's LDS, Phred+64, records without qualities, quality bytes of 128 and above in the head and
      tail pieces, an upper length bound: seam_case();
  B2  minimum lengths of 0, 1, 5 and 99 (tgsf_params.min_len >= 0; below that tgsf_create refuses): the same with reads
      of 1..20 bp;
  B3  the adaptive switch: a designed sequence of batches, the number that speculated read off the TGSF_TRACE_BP line;
  B4  136 000 reads in one batch (k_tail_fix's grid is 131 072 lanes): every wave's sums, every block's LDS tallies and
      flush, many blocks adding to one table row.  GPU only: tests/test_trims_gpu.py.

Every comparison is against orc.filter_batch: all record fields, all fragment fields, every tally word
(parity.compare_batch).  Each input comes with assertions on the input itself, made on the oracle's result before anything
runs.  tests/test_trims_emul.py runs B1-B3 on the serial emulation, tests/test_trims_gpu.py runs all four on the HIP build."""
from __future__ import annotations

import concurrent.futures
import os
import re

import numpy as np

from oracle import orc
from tests import parity
from tgsfilter_amd import abi, capi, synth

ADS = [synth.ONT_RAPID, synth.ONT_RAPID_RC]
MODES = ["byproduct", None]          # TGSF_CLEAN_TABLES: always speculate | the context decides (its first batch speculates)
MIN_Q = 8.0
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_AD_FLAGS = abi.RF_AD5P | abi.RF_AD3P | abi.RF_ADMID

HEADS = (1, 3, 4, 99, 100, 101, 137, 6399, 6400, 6401, 12850)
TAILS = (1, 8, 99, 100, 101, 250, 700, 6400, 6401, 6500, 13000)
# 21 of the 144 pairs (0: that end is not trimmed): every value of either list at least once, both trims of a tile and more in three
PAIRS = [(1, 8), (3, 6400), (4, 1), (99, 100), (100, 99), (101, 101), (137, 6500), (6399, 101), (6400, 0), (6401, 8), (12850, 250),
         (0, 250), (0, 700), (0, 6401), (0, 13000), (6400, 6401), (6399, 6500), (79, 700), (12850, 6400), (100, 1), (79, 13)]
assert all(any(h == v for h, _ in PAIRS) for v in HEADS) and all(any(t == v for _, t in PAIRS) for v in TAILS)
assert sum(h >= 6399 and t >= 6400 for h, t in PAIRS) >= 2

# a case: (head, tail, variant, min_len)
VARIANTS = {
    "qtype64": [(4, 1), (137, 6500), (6400, 6401)],
    "no_qual": [(99, 100), (6401, 8), (0, 6401)],
    "high_q": [(137, 6500), (6399, 101), (79, 700)],                # (a head that splits a bin, and a tail)
    "long_tables": [(79, 700), (0, 6401), (6400, 6401)],            # max_read_len 250 000: k_tail_fix goes straight to memory
    "max_len": [(1, 8), (101, 101), (12850, 250)],
}
SEAM_CASES = [(h, t, None, 100) for h, t in PAIRS] + [(h, t, v, 100) for v, pairs in VARIANTS.items() for h, t in pairs]
MIN_LENS = (0, 1, 5, 99)
MIN_LEN_CASES = [(h, t, None, m) for h, t in ((4, 1), (99, 100), (137, 6500), (6400, 6401)) for m in MIN_LENS]
assert all(pair in PAIRS for pairs in VARIANTS.values() for pair in pairs) and all((h, t) in PAIRS for h, t, _, _ in MIN_LEN_CASES)


def case_id(case):
    h, t, v, m = case
    return "%d-%d" % (h, t) + ("-%s" % v if v else "") + ("-l%d" % m if m != 100 else "")


# ---------------------------------------------------------------------------
# B1, B2: the inputs
# ---------------------------------------------------------------------------
# lengths beyond head + tail + min_len of further hand-made reads: whatever the trims, a dozen reads of a case are long enough
# to be kept as [head, L - tail) (the 30 synthetic reads of about 9 kb are not, under trims of 19 kb), ten of them also under
# the "max_len" variant's bound
_BEYOND = (7, 50, 99, 100, 101, 250, 999, 1000, 1001, 6300, 6400, 6401, 12801)


def hand_lengths(h, t, m):
    ls = [t, t + 1, h, h + 1, h + t - 1, h + t, h + t + 1, h + t + m - 1, h + t + m, h + t + m + 1, 6400, 6400 + t, 6400 + h,
          12800 + t, 6399 + h + t, 99 + t, 100 + t, 101 + t]
    ls += [h + t + m + d for d in _BEYOND]
    return [L for L in ls if L >= 1]


def _with_high_bytes(rng, q, h, t, L):
    """Qualities of 120..126 with bytes of 128 and above (which stand for their value - 256, src/TGSFilter.cpp:1455-1457)
    at a quarter of the places of the last t bytes -- k_tail_fix's -- and of the first h % 100 bytes of every bin -- the
    head pieces of the split bins.  The mean of the read and of any run of bins stays above 0."""
    q[:] = rng.integers(120, 127, L)
    at = np.arange(L)
    where = ((at >= L - t) | (at % 100 < h % 100)) & (rng.random(L) < 0.25)
    q[where] = rng.integers(128, 256, int(where.sum()))
    return q


def case_reads(case):
    """The reads of a case: 30 ONT reads of about 9 kb with the zoo's edge cases, adapters at the 5' end of a third and in
    the middle of a few; hand-made clean reads on the seams of the trims, min_len, bins and tiles (hand_lengths); with a
    min_len below 100 also reads of 1..20 bp."""
    h, t, variant, m = case
    qtype = 64 if variant == "qtype64" else 33
    rng = np.random.default_rng(100003 * h + 17 * t + m)
    reads = synth.make_reads(9000 + 7 * h + t, 30, "ont", mean_len=9000, zoo=True, pmid=0.05, p5=0.3)
    lens = hand_lengths(h, t, m) + (list(range(1, 21)) if m != 100 else [])
    for k, L in enumerate(lens):
        q = (rng.integers(25, 40, L) + 33).astype(np.uint8)
        if variant == "high_q" and L >= h + t + m:
            q = _with_high_bytes(rng, q, h, t, L)
        reads.insert(int(rng.integers(0, len(reads) + 1)), (b"hand%d_%d" % (k, L), _ACGT[rng.integers(0, 4, L)].tobytes(), q.tobytes()))
    if qtype == 64:
        reads = [(name, s, bytes(min(c + 31, 126) for c in q)) for name, s, q in reads]
    return reads


def case_params(case, reads):
    h, t, variant, m = case
    p = parity.sized(abi.make_params("ont", adapters=ADS, min_q=MIN_Q, head_trim=h, tail_trim=t, qtype=64 if variant == "qtype64" else 33,
                                     no_qual=variant == "no_qual"), reads)
    p.min_len = m                                                     # (make_params clamps it to 100 as the reference's command line does)
    if variant == "long_tables":
        p.max_read_len = 250_000
    if variant == "max_len":
        p.max_len = h + t + m + 1000
    return p


_EXPECTED = {}


def expected(case):
    """(reads, parameters, the oracle's (records, fragments, tallies) after one batch and after the same batch again) of a
    case, computed once for all the tests that run it, with the case's assertions on its input."""
    if case not in _EXPECTED:
        h, t, variant, m = case
        reads = case_reads(case)
        p = case_params(case, reads)
        seq, qual, offsets, lengths = synth.pack(reads)
        r, f, ctr = orc.filter_batch(p, seq, qual, offsets, lengths)
        L = lengths.astype(np.int64)
        one = r["n_frags"] == 1
        first = f[np.minimum(r["frag_begin"], max(len(f) - 1, 0))] if len(f) else None
        as_speculated = one & (first["start"] == h) & (first["len"] == L - h - t) & ((first["flags"] & abi.FF_PASS) != 0)
        assert as_speculated.sum() >= 10, (case, int(as_speculated.sum()))
        assert (((r["flags"] & _AD_FLAGS) != 0) | (r["n_frags"] > 1)).sum() >= 5, case
        assert variant == "no_qual" or ((r["flags"] & abi.RF_LOWQ) != 0).sum() >= 2, case       # (records without qualities: no gate)
        assert (L <= h).any() or h == 0, case
        assert (L <= t).any() or t == 0, case
        assert (L - h - t == m).any(), case
        if variant == "high_q":
            kept = np.nonzero(as_speculated)[0]
            tails = b"".join(reads[i][2][-t:] for i in kept)
            heads = b"".join(reads[i][2][100 * k:100 * k + h % 100] for i in kept for k in range(len(reads[i][2]) // 100))
            assert max(tails) >= 128 and max(heads) >= 128, case
        if variant == "max_len":
            assert (L - h - t > p.max_len).any() and (as_speculated & (L - h - t > m + 900)).any(), case
        if m != 100:
            assert (L <= 20).sum() >= 20, case
        # the same batch once more on the same tallies: every sum doubles, the four rows-in-use words are maxima
        twice = ctr * np.uint64(2)
        twice[abi.CTR_ROWS:abi.CTR_ROWS + 4] = ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4]
        _EXPECTED[case] = (reads, p, (r, f, ctr), (r, f, twice))
    return _EXPECTED[case]


def prefetch(cases):
    """The oracle over all `cases` at once (it holds no state and ctypes releases the interpreter for the call)."""
    todo = [c for c in cases if c not in _EXPECTED]
    if todo:
        with concurrent.futures.ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
            list(pool.map(expected, todo))


def second_batch_doubles(case):
    """What expected() derives for the second batch is what the oracle gives when it adds the batch to the first's tallies."""
    reads, p, (r, f, ctr), (_, _, twice) = expected(case)
    seq, qual, offsets, lengths = synth.pack(reads, align=1)
    r2, f2, ctr2 = orc.filter_batch(p, seq, qual, offsets, lengths, ctr=ctr.copy())
    assert np.array_equal(r2, r) and np.array_equal(f2, f) and np.array_equal(ctr2, twice)


def set_mode(monkeypatch, mode):
    monkeypatch.setenv("TGSF_CLEAN_TABLES", mode) if mode else monkeypatch.delenv("TGSF_CLEAN_TABLES", raising=False)
    for k in ("TGSF_POOL_CAP", "TGSF_TRACE_BP"):
        monkeypatch.delenv(k, raising=False)


def run_case(lib_path, case, mode, monkeypatch):
    """One case under one strategy: the batch 16-byte padded, then packed back to back (reads start anywhere) through the
    same context, whose tallies then hold both."""
    reads, p, first, second = expected(case)
    set_mode(monkeypatch, mode)
    ctx = capi.Context(p, 0, lib_path)
    try:
        assert ctx.n_bins == abi.n_bins(p.max_read_len) and (case[2] != "long_tables" or ctx.n_bins > 1024)
        parity.compare_batch(ctx, p, reads, align=16, expected=first)
        parity.compare_batch(ctx, p, reads, align=1, expected=second)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# B3: the switch
# ---------------------------------------------------------------------------
SWITCH_TRIMS = (79, 13)
SWITCH_CLEAN_FIRST, SWITCH_CLEAN_AFTER = 3, 70
_TRACE = re.compile(r"tgsf: clean tables as a by-product of the raw pass: (\d+) batches speculated; the next would( not)?;")


def _clean_reads(rng, n, tag, lo=600, hi=3000):
    """Reads of lo..hi bp without an adapter, every quality well above MIN_Q."""
    out = []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        out.append((b"%s_%d" % (tag, i), _ACGT[rng.integers(0, 4, L)].tobytes(), (rng.integers(25, 40, L) + 33).astype(np.uint8).tobytes()))
    return out


def switch_batches():
    """The designed sequence: three clean batches; one whose every read carries an exact copy of an adapter inside its 5' end
    window behind the head trim; 70 clean batches of 8 reads of 300..1 000 bp."""
    rng = np.random.default_rng(793)
    batches = [_clean_reads(rng, 24, b"first%d" % b) for b in range(SWITCH_CLEAN_FIRST)]
    bad = []
    for i, (name, s, q) in enumerate(_clean_reads(rng, 24, b"adapter")):
        at = SWITCH_TRIMS[0] + 5 + i
        bad.append((name, s[:at] + ADS[i & 1] + s[at + len(ADS[i & 1]):], q))
    batches.append(bad)
    batches += [_clean_reads(rng, 8, b"after%d" % b, 300, 1000) for b in range(SWITCH_CLEAN_AFTER)]
    return batches


def switch(lib_path, mode, monkeypatch, capfd):
    """k_clean_plan_next over the sequence, every batch's records, fragments and tallies against the oracle; returns
    (batches that speculated, batches submitted, would the next).

    What the sequence is designed to give under the context's own decisions: the first batch speculates (tgsf_create), a
    clean batch keeps every read as speculated and leaves the switch on, so the adapter batch -- the fourth -- speculates
    too.  Every read of it turns out otherwise: the second looks cost more than twice a direct pass, the switch goes off.
    64 batches go by without speculation, the 64th turns it on again, and the six that follow speculate: 4 + 6 of 74."""
    set_mode(monkeypatch, mode)
    monkeypatch.setenv("TGSF_TRACE_BP", "1")
    batches = switch_batches()
    h, t = SWITCH_TRIMS
    # (-m 20: with the default of 4 a random read now and then has an "adapter" at an end; here a read has one by design or not at all)
    p = parity.sized(abi.make_params("ont", adapters=ADS, min_q=MIN_Q, min_len=100, head_trim=h, tail_trim=t, end_match_len=20), max(batches, key=lambda b: sum(len(r[1]) for r in b)))
    p.max_batch_reads = max(len(b) for b in batches)
    p.max_read_len = 3000
    ctx = capi.Context(p, 0, lib_path)
    try:
        capfd.readouterr()
        base = None
        for k, reads in enumerate(batches):
            res, frags, base = parity.compare_batch(ctx, p, reads, align=16 if k % 2 == 0 else 1, base=base)
            first = frags[np.minimum(res["frag_begin"], len(frags) - 1)]
            as_speculated = (res["n_frags"] == 1) & (first["start"] == h) & (first["len"] == np.array([len(r[1]) for r in reads]) - h - t)
            if k == SWITCH_CLEAN_FIRST:
                assert ((res["flags"] & abi.RF_AD5P) != 0).all() and not as_speculated.any()
            else:
                assert as_speculated.sum() >= len(reads) - 1, (k, as_speculated)      # (one read of eight looked at twice: a quarter of a direct pass)
    finally:
        ctx.close()
    m = _TRACE.search(capfd.readouterr().err)
    assert m, "no TGSF_TRACE_BP line"
    return int(m.group(1)), len(batches), m.group(2) is None


def switch_adaptive(lib_path, monkeypatch, capfd):
    speculated, submitted, next_would = switch(lib_path, None, monkeypatch, capfd)
    assert 2 < speculated < submitted and next_would, (speculated, submitted, next_would)
    assert speculated == SWITCH_CLEAN_FIRST + 1 + (SWITCH_CLEAN_AFTER - 64), (speculated, submitted)


def switch_forced(lib_path, monkeypatch, capfd):
    speculated, submitted, next_would = switch(lib_path, "byproduct", monkeypatch, capfd)
    assert speculated == submitted and next_would, (speculated, submitted, next_would)


# ---------------------------------------------------------------------------
# B4: scale
# ---------------------------------------------------------------------------
SCALE_N = 136_000
TAIL_FIX_GRID = 128 * 1024           # k_tail_fix: at most 128 blocks of 1 024 lanes
SCALE_MIN_Q = 12.0


class ScaleInput:
    """136 000 reads built with numpy in one go: most of 320..450 bp, 200 of 6..30 kb (several tiles); a per-read mean quality
    uniform in [min_q - 4, min_q + 8] with normal noise of sd 6 per base, clipped to 0..60.  Every read starts at a multiple of
    16; the bytes between two reads are bases and qualities like any others (a caller's buffer may hold anything there).
    adapters: ONT_RAPID or its reverse complement, 5 % of its bases substituted, within 30 bases of either end of 30 % of the
    reads, in the middle of 2 % of the reads of 420 bp and more, and in the middle of every fourth long read."""

    def __init__(self, adapters=False, seed=136):
        rng = np.random.default_rng(seed)
        n = SCALE_N
        L = rng.integers(320, 451, n).astype(np.int64)
        long_at = rng.choice(n, 200, replace=False)
        L[long_at] = rng.integers(6000, 30001, 200)
        L[long_at[:4]] = (6400, 6401, 12800 + 13, 6399 + 79 + 13)
        slots = (L + 15) // 16 * 16
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(slots, out=off[1:])
        total = int(off[-1])
        self.n, self.lengths, self.offsets = n, L.astype(np.uint32), off.astype(np.uint64)
        self.seq = np.zeros(total + 64, dtype=np.uint8)
        self.seq[:total] = _ACGT[rng.integers(0, 4, total, dtype=np.uint8)]
        q = rng.standard_normal(total, dtype=np.float32)
        q *= 6.0
        q += np.repeat(rng.uniform(SCALE_MIN_Q - 4, SCALE_MIN_Q + 8, n).astype(np.float32), slots)
        np.rint(q, out=q)
        np.clip(q, 0, 60, out=q)
        q += 33
        self.qual = np.zeros(total + 64, dtype=np.uint8)
        self.qual[:total] = q.astype(np.uint8)
        del q
        self.planted_end = self.planted_mid = 0
        if adapters:
            ad = np.stack([np.frombuffer(a, dtype=np.uint8) for a in ADS])
            A = ad.shape[1]

            def plant(reads, at):
                copies = ad[rng.integers(0, 2, reads.size)].copy()
                hit = rng.random(copies.shape) < 0.05
                copies[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
                self.seq[(off[reads] + at)[:, None] + np.arange(A)[None, :]] = copies
            ends = np.nonzero(rng.random(n) < 0.30)[0]
            pre = rng.integers(0, 31, ends.size)
            five = rng.random(ends.size) < 0.6
            plant(ends[five], pre[five])
            plant(ends[~five], (L[ends] - A - pre)[~five])
            mids = np.nonzero((rng.random(n) < 0.02) & (L >= 420))[0]
            plant(mids, rng.integers(180, L[mids] - 180 - A + 1))
            plant(long_at[::4], L[long_at[::4]] // 2)                  # (a short read's pieces beside a middle adapter are mostly below min_len: these split)
            self.planted_end, self.planted_mid, self.planted_split = int(ends.size), int(mids.size), int(long_at[::4].size)

    def qual64(self):
        return self.qual + np.uint8(31)

    def sample_passes(self):
        """k_prepare's guess of the mean quality in numpy: 16 bytes at ((L - 16) * k) / 3 for k = 0..3."""
        L = self.lengths.astype(np.int64)
        at = ((L - 16)[:, None] * np.arange(4)[None, :]) // 3
        idx = (self.offsets[:-1].astype(np.int64)[:, None, None] + at[:, :, None] + np.arange(16)[None, None, :]).reshape(self.n, 64)
        guess = self.qual[idx].astype(np.float64).mean(axis=1) - 33.0
        return guess >= SCALE_MIN_Q

    def full_passes(self):
        o = self.offsets[:-1].astype(np.int64)
        bounds = np.stack([o, o + self.lengths.astype(np.int64)], axis=1).reshape(-1)
        sums = np.add.reduceat(self.qual, bounds, dtype=np.int64)[::2]
        return sums / self.lengths - 33.0 >= SCALE_MIN_Q

    def check(self):
        """The mix the input is there for: reads whose 64 sampled bytes pass the gate while the read fails it (speculated, then
        taken back out) and the other way round, a thousand and more of each, and a thousand speculated reads beyond
        k_tail_fix's grid."""
        assert self.n > TAIL_FIX_GRID + 4000
        s, f = self.sample_passes(), self.full_passes()
        counts = (int(s.sum()), int((s & ~f).sum()), int((~s & f).sum()), int(s[TAIL_FIX_GRID:].sum()))
        assert counts[1] >= 1000 and counts[2] >= 1000 and counts[3] >= 1000, counts
        assert ((self.lengths > 6400).sum() >= 150) and (self.lengths > 12800).sum() >= 100
        return counts

    def params(self, head, tail, adapters, qtype=33, max_read_len=None):
        p = abi.make_params("ont", adapters=adapters, min_q=SCALE_MIN_Q, min_len=100, head_trim=head, tail_trim=tail, qtype=qtype)
        p.max_batch_reads = self.n
        p.max_batch_bases = int(self.lengths.sum()) + 64
        p.max_read_len = max_read_len or int(self.lengths.max())
        return p

    def oracle(self, p, qual=None, workers=1):
        """The oracle over the batch, in `workers` runs of consecutive reads at once: records and fragments put back in
        order, the tallies summed, the four rows-in-use words by maximum."""
        qual = self.qual if qual is None else qual
        n_bins = abi.n_bins(p.max_read_len)
        cuts = np.linspace(0, self.n, workers + 1).astype(int)

        def part(k):
            a, b = cuts[k], cuts[k + 1]
            return orc.filter_batch(p, self.seq, qual, self.offsets[a:b + 1], self.lengths[a:b], n_bins=n_bins)
        if workers == 1:
            return part(0)
        with concurrent.futures.ThreadPoolExecutor(min(workers, 16)) as pool:
            parts = list(pool.map(part, range(workers)))
        ctr = np.zeros_like(parts[0][2])
        rs, fs, nf = [], [], 0
        for k, (r, f, c) in enumerate(parts):
            r, f = r.copy(), f.copy()
            r["frag_begin"] += np.uint32(nf)
            f["read"] += np.uint32(cuts[k])
            nf += len(f)
            rs.append(r)
            fs.append(f)
            rows = np.maximum(ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4], c[abi.CTR_ROWS:abi.CTR_ROWS + 4])
            ctr += c
            ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4] = rows
        return np.concatenate(rs), np.concatenate(fs), ctr

    def run(self, lib_path, p, exp, mode, monkeypatch, capfd, qual=None):
        """The batch through a new context under one strategy against exp = the oracle's (records, fragments, tallies);
        returns the number of batches that speculated (of one)."""
        set_mode(monkeypatch, mode)
        monkeypatch.setenv("TGSF_TRACE_BP", "1")
        ctx = capi.Context(p, 0, lib_path)
        try:
            assert ctx.n_bins == abi.n_bins(p.max_read_len)
            capfd.readouterr()
            got_r, got_f = ctx.submit(self.seq, self.qual if qual is None else qual, self.offsets[:-1].copy(), self.lengths)
            ctr = ctx.counters()
        finally:
            ctx.close()
        m = _TRACE.search(capfd.readouterr().err)
        exp_r, exp_f, exp_ctr = exp
        for name in ("sum_q", "flags", "n_frags", "frag_begin", "trimmed"):
            bad = np.nonzero(got_r[name] != exp_r[name])[0]
            assert bad.size == 0, f"read field {name} differs at {bad.size} reads, first {bad[:8]}: got {got_r[name][bad[:8]]} exp {exp_r[name][bad[:8]]}"
        assert len(got_f) == len(exp_f), (len(got_f), len(exp_f))
        for name in ("sum_q", "read", "start", "len", "flags"):
            bad = np.nonzero(got_f[name] != exp_f[name])[0]
            assert bad.size == 0, f"fragment field {name} differs at {bad.size} fragments, first {bad[:8]}"
        bad = np.nonzero(ctr != exp_ctr)[0]
        assert bad.size == 0, f"{bad.size} tally words differ, first {bad[:12]}: got {ctr[bad[:12]]} exp {exp_ctr[bad[:12]]}"
        return int(m.group(1)) if m else 0
