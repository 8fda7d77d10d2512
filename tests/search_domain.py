"""The adapter search across its parameters and adapter sets: k_end_windows, the k_mid_* family, k_mid_resolve* and k_regions.

The rest of the suite draws end_len from {0, 7, 60, 150, 300}, extra_len from {0, 10, 50} and three similarities each, and no
batch of it has more than 9 adapters.  Here:

  S1  window seams: end_len from 0 to 2^28 against a set of adapters of different lengths (28, 45, 150 bp); clean reads with
      L - 2E one below, at and one above each adapter's length (the middle scan is on for the shorter adapters and off for the
      longer ones of the same read), reads of 1..8 bp and around each 5' window's width, copies starting at 0, ending on a
      window's last column and one beyond, starting at E - 1, E, E + 1, and the mirror images: seam_case();
  S2  margins and merging: extra_len from 0 to 2^28; two middle copies whose margins touch, leave one base between and overlap
      by one, an end clip and a margin the same three ways, kept pieces of min_len - 1, min_len, max_len, max_len + 1, reads
      dropped as one region (dl == L); discard, filter = 0, only_qc: margin_case();
  S3  gates: similarities on the float32 value m / Q and its two neighbours against copies with Q - m substitutions, one more
      and one fewer; match lengths of 1, Q - 1, Q, Q + 1 and INT_MAX; similarities of 1.0, 1.5, 1e-30 and +inf: gate_case();
  S4  adapter sets of 0, 1, 5, 8, 9, 17 and 32 members, ordered so that the middle scan's passes have 1 to 4 members of each
      word class and start at many a0, up to 28..31; the 32-sets also with a candidate pool of 3 slots (the replay), the
      segment scan and every TGSF_MID_FILTER: set_case();
  S5  fuzzing over the same dimensions: tests/fuzz.py, TGSF_FUZZ_SEARCH=1.

Every comparison is parity.compare_batch against orc.filter_batch: all record fields, all fragment fields, every tally word,
the batch 16-byte padded and then packed back to back through the same context.  Each input comes with assertions on the
oracle's result, made before the library runs, that it holds what it is there for.  tests/test_search_emul.py runs all of it
on the serial emulation, tests/test_search_gpu.py on the HIP build.  No tolerance anywhere: everything is an integer."""
from __future__ import annotations

import concurrent.futures
import os

import numpy as np

from oracle import orc
from tests import parity
from tgsfilter_amd import abi, capi, synth

INT_MAX = 2147483647
BOUND = 1 << 28                       # the most end_len and extra_len may be (include/tgsf.h)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_OTHER = {65: 67, 67: 65, 71: 84, 84: 71}          # a base that is not the one given
_AD = abi.RF_AD5P | abi.RF_AD3P | abi.RF_ADMID
_KIND = (abi.RF_AD5P, abi.RF_AD3P, abi.RF_ADMID)        # what a copy near the 5' end, near the 3' end, in the middle sets
KNOBS = ("TGSF_POOL_CAP", "TGSF_MID_FLAT", "TGSF_MID_FILTER", "TGSF_CLEAN_TABLES", "TGSF_TRACE_BP", "TGSF_NO_HOT32", "TGSF_SEG_COLS")

AD22 = b"GCAATACGTAACTGAACGAAGT"
AD28 = synth.ONT_RAPID[:28]
AD45 = b"CTTGCGGGCGGCGGACTCTCCTCTGAAGATAGAGCGACAGGCAAG"
AD150 = bytes(_ACGT[np.random.default_rng(150).integers(0, 4, 150)])


def bases(rng, L):
    return _ACGT[rng.integers(0, 4, L)].tobytes()


def read_of(rng, name, seq):
    """A record whose every quality is well above any gate used here."""
    return (name, bytes(seq), (rng.integers(25, 40, len(seq)) + 33).astype(np.uint8).tobytes())


def substituted(rng, ad, n):
    """`ad` with exactly n bases replaced by another base, no two of them adjacent where that is possible."""
    a = bytearray(ad)
    if n > 0:
        step = max(1, len(a) // n)
        start = int(rng.integers(0, max(1, min(step, len(a) - step * (n - 1)))))
        for x in range(n):
            at = (start + x * step) % len(a)
            a[at] = _OTHER[a[at]]
    return bytes(a)


def planted(rng, L, copies):
    """A random read of L bases with each (start, bytes) of `copies` written over it; a copy reaching outside is cut."""
    s = bytearray(bases(rng, L))
    for at, c in copies:
        if at < 0:
            c, at = c[-at:], 0
        c = c[:max(0, L - at)]
        s[at:at + len(c)] = c
    return s


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def oracle(p, reads):
    seq, qual, offsets, lengths = synth.pack(reads)
    return orc.filter_batch(p, seq, qual, offsets, lengths)


def twice(ctr):
    """The tallies after the same batch once more: every sum doubles, the four rows-in-use words are maxima."""
    t = ctr * np.uint64(2)
    t[abi.CTR_ROWS:abi.CTR_ROWS + 4] = ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4]
    return t


def run(lib_path, p, reads, exp, env, monkeypatch):
    """One input under one set of knobs: 16-byte padded, then back to back (windows at every alignment) on the same tallies."""
    set_env(monkeypatch, env)
    r, f, ctr = exp
    ctx = capi.Context(p, 0, lib_path)
    try:
        parity.compare_batch(ctx, p, reads, align=16, expected=exp)
        parity.compare_batch(ctx, p, reads, align=1, expected=(r, f, twice(ctr)))
    finally:
        ctx.close()


def flagged(r, flag):
    return int(((r["flags"] & flag) != 0).sum())


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def prefetch(jobs):
    """The oracle over several inputs at once (it holds no state and ctypes releases the interpreter for the call)."""
    with concurrent.futures.ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda j: j[0](*j[1:]), jobs))


# ---------------------------------------------------------------------------
# S1: window seams
# ---------------------------------------------------------------------------
SEAM_ADS = [AD28, AD45, AD150]
SEAM_E = (0, 1, 4, 5, 27, 28, 150, 1000, 100_000, BOUND)
SEAM_ENVS = {"flat": {}, "segments": {"TGSF_MID_FLAT": "0"}}
SEAM_END_SIM = 0.75


def seam_w5(E, Q):
    return E + int(np.float32(Q) / np.float32(SEAM_END_SIM))


def seam_reads(E):
    """(reads, what each designed read is: name -> (kind, adapter index)).  Beyond E = 1000 no read has a middle window and
    every end window is the read: the positions are those of E = 150, so that the copies lie anywhere in those windows."""
    rng = np.random.default_rng(1000 + E % 9973)
    reads = []
    Ep = E if E <= 1000 else 150                         # where the copies go
    for a, ad in enumerate(SEAM_ADS):
        Q = len(ad)
        for d in (-1, 0, 1):                             # clean reads: the middle window one below, at, one above the adapter
            L = 2 * E + Q + d
            if 1 <= L <= 3300:
                reads.append(read_of(rng, b"mid_a%d_%+d" % (a, d), bases(rng, L)))
            # ... and the same three with the adapter itself as the middle window [E, E + Q): found there only while L - 2E >= Q
            if 1 <= L <= 3300 and E <= 1000:
                reads.append(read_of(rng, b"midcopy_a%d_%+d" % (a, d), planted(rng, L, [(E, ad)])))
        w5 = seam_w5(E, Q)
        for L in (w5 - 1, w5, w5 + 1):                   # the 5' / 3' window is the read, or one base short of it
            if 1 <= L <= 3300:
                reads.append(read_of(rng, b"w5_a%d_%d" % (a, L), planted(rng, L, [(max(0, L - Q), ad)])))
    for L in range(1, 9):                                # the `< 5` rule, windows clamped to tiny reads
        reads.append(read_of(rng, b"tiny%d" % L, (AD28 * 2)[3:3 + L] if L & 1 else bases(rng, L)))
    k = 0
    for a, ad in enumerate(SEAM_ADS):
        Q = len(ad)
        L = 2 * Ep + 2 * Q + 400 + 37 * a
        W5 = min(seam_w5(Ep, Q), L)
        starts = {"at0": 0, "w5_last": W5 - Q, "w5_beyond": W5 - Q + 1, "E-1": Ep - 1, "E": Ep, "E+1": Ep + 1,
                  "atL": L - Q, "w3_first": L - W5, "w3_before": L - W5 - 1, "LE-1": L - Ep - Q - 1, "LE": L - Ep - Q, "LE+1": L - Ep - Q + 1,
                  "middle": L // 2}
        for what, at in starts.items():
            if at < 0:
                continue
            copy = ad if k % 2 == 0 else substituted(rng, ad, 1 + k % 2 + (Q > 100))     # exact, or lightly mutated
            reads.append(read_of(rng, b"copy_a%d_%s" % (a, what.encode()), planted(rng, L, [(at, copy)])))
            k += 1
    order = np.random.default_rng(E % 9973).permutation(len(reads))
    return [reads[i] for i in order]


def seam_params(E, reads):
    p = parity.sized(abi.make_params("ont", adapters=SEAM_ADS, min_q=7.0, end_len=E, end_match_len=8, mid_match_len=20, extra_len=50), reads)
    p.min_len = 1
    p.end_sim = SEAM_END_SIM
    return p


def seam_case(E):
    def make():
        reads = seam_reads(E)
        assert len(reads) <= 150 and max(len(r[1]) for r in reads) <= 3300, (E, len(reads))
        p = seam_params(E, reads)
        r, f, ctr = exp = oracle(p, reads)
        L = np.array([len(x[1]) for x in reads], dtype=np.int64)
        ML = L - 2 * E
        has_mid = E <= 1000
        assert flagged(r, abi.RF_AD5P) >= 3 and flagged(r, abi.RF_AD3P) >= 3, (E, flagged(r, abi.RF_AD5P), flagged(r, abi.RF_AD3P))
        if has_mid:
            assert flagged(r, abi.RF_ADMID) >= 3, (E, flagged(r, abi.RF_ADMID))
            # a read where one adapter of the set has a middle window and another has not: between two lengths of the set
            assert ((ML >= 28) & (ML < 45)).any() and ((ML >= 45) & (ML < 150)).any() and (ML == 150).any() and (ML == 27).any(), E
            # ... and one copy found by the 5' search and the middle search alike (the 5' window reaches beyond E)
            assert (((r["flags"] & abi.RF_AD5P) != 0) & ((r["flags"] & abi.RF_ADMID) != 0)).any(), E
        else:
            assert (ML < 1).all() and flagged(r, abi.RF_ADMID) == 0, E
        names = [x[0] for x in reads]
        if has_mid:                                        # the middle window that is exactly the adapter: a middle hit at L - 2E = Q, none one below
            for a in range(len(SEAM_ADS)):
                at = [int(r["flags"][names.index(b"midcopy_a%d_%+d" % (a, d))] & abi.RF_ADMID) != 0 for d in (-1, 0, 1)]
                assert at == [False, True, True], (E, a, at)
        for L_tiny in range(1, 5):                         # windows below 5 columns are not searched: such a read is kept whole
            i = names.index(b"tiny%d" % L_tiny)
            assert (r["flags"][i] & _AD) == 0 and r["n_frags"][i] == 1, (E, L_tiny)
        return reads, p, exp
    return cached(("seam", E), make)


# ---------------------------------------------------------------------------
# S2: margins and merging
# ---------------------------------------------------------------------------
MARGIN_ADS = [synth.ONT_RAPID, synth.ONT_RAPID_RC]
MARGIN_T = (0, 1, 50, 1000, BOUND)
MARGIN_E, MARGIN_MIN, MARGIN_MAX = 150, 50, 700
MARGIN_VARIANTS = (None, "discard", "no_filter", "only_qc", "ends_only")
_MQ = 50                                                # both adapters
_MW5 = MARGIN_E + int(np.float32(_MQ) / np.float32(0.75))


def margin_reads(T):
    """Designed reads first (their names say what they are), then ordinary ones with adapters at ends and in the middle."""
    rng = np.random.default_rng(2000 + T % 9973)
    ad, rc = MARGIN_ADS
    Tp = min(T, 1000)                                   # positions of the two-copy reads: beyond a read's length T is any T
    reads = []
    # two middle copies: the first one's interval ends where the second one's begins (d = 0), one base before it, one base after
    lead, tail = (300, 300) if Tp < 1000 else (60, 230)     # (the pieces outside the two intervals; the 3' window is 216 wide)
    for d in (-1, 0, 1):
        s1 = Tp + lead
        s2 = s1 + _MQ + 2 * Tp + d
        L = s2 + _MQ + Tp + tail
        reads.append(read_of(rng, b"pair%+d" % d, planted(rng, L, [(s1, ad), (s2, rc)])))
    # an end clip [0, 166) and a middle copy whose margin begins there, one base before, one base after (the 5' copy has 16 of
    # its bases in the middle window: no middle hit of its own)
    if Tp >= 50:
        for d in (-1, 0, 1):
            s = 166 + Tp + d
            reads.append(read_of(rng, b"clip%+d" % d, planted(rng, s + _MQ + Tp + 320, [(116, ad), (s, rc)])))
    # margins clipped at 0 and at L: copies just inside the middle window at either end
    for at in (MARGIN_E, MARGIN_E + 30, _MW5 + 5):
        L = 900
        reads.append(read_of(rng, b"near5_%d" % at, planted(rng, L, [(at, ad)])))
        reads.append(read_of(rng, b"near3_%d" % at, planted(rng, L, [(L - at - _MQ, rc)])))
    # kept pieces on the seams of max_len: an exact copy at 0 is clipped as [0, 50), one at the other end as [L - 50, L)
    for kept in (MARGIN_MAX, MARGIN_MAX + 1):
        reads.append(read_of(rng, b"keep%d" % kept, planted(rng, _MQ + kept, [(0, ad)])))
        reads.append(read_of(rng, b"keep3_%d" % kept, planted(rng, _MQ + kept, [(kept, rc)])))
    # ... and of min_len: the piece between two middle copies' intervals.  (A read short enough for such a piece beside an end
    # clip lies inside its own end windows, where the 3' search drops everything behind a copy: with a margin beyond the reads'
    # lengths, where a middle hit drops the whole read, no kept piece that short can be designed.)
    for kept in (MARGIN_MIN - 1, MARGIN_MIN):
        s1 = Tp + lead
        s2 = s1 + _MQ + 2 * Tp + kept
        reads.append(read_of(rng, b"gap%d" % kept, planted(rng, s2 + _MQ + Tp + tail, [(s1, ad), (s2, rc)])))
    # the whole read one dropped region: two copies and nothing else; one copy and nothing else
    reads.append(read_of(rng, b"whole2", ad + rc))
    reads.append(read_of(rng, b"whole1", ad))
    # ... and by margins alone: a middle copy in a read shorter than the margin (T >= 1000)
    reads.append(read_of(rng, b"whole_mid", planted(rng, 700, [(330, ad)])))
    # ... and by two end clips that touch, [0, 216) and [216, 432): one region only where touching regions are joined (the variant
    # "ends_only" switches the middle search off, which would find both copies); one base between them, and overlapping by one
    for d in (-1, 0, 1):
        reads.append(read_of(rng, b"ends%+d" % d, planted(rng, 2 * _MW5 + d, [(_MW5 - _MQ, ad), (_MW5 + d, rc)])))
        # (... and with the adapters the other way round: the second adapter's 5' clip then meets the first one's 3' clip from the left)
        reads.append(read_of(rng, b"sdne%+d" % d, planted(rng, 2 * _MW5 + d, [(_MW5 - _MQ, rc), (_MW5 + d, ad)])))
    designed = len(reads)
    for i, (name, s, q) in enumerate(synth.make_reads(2100, 40, "ont", mean_len=1500, max_len=3000, zoo=True, pmid=0.4, p5=0.4)):
        reads.append((name, s, q))
    return reads, designed


def margin_params(T, variant, reads):
    p = parity.sized(abi.make_params("ont", adapters=MARGIN_ADS, min_q=7.0, end_len=MARGIN_E, end_match_len=15, mid_match_len=_MQ + 1 if variant == "ends_only" else 35, extra_len=T,
                                     max_len=MARGIN_MAX, discard=variant == "discard", filter=variant != "no_filter", only_qc=variant == "only_qc"), reads)
    p.min_len = MARGIN_MIN
    return p


def margin_ends(tag, T, variant, reads, names, L, r):
    """The three reads of two end clips each (overlapping by one, touching, a base between) as the oracle sees them."""
    tallies = []
    for d in (-1, 0, 1):
        i = names.index(tag + b"%+d" % d)
        assert r["n_frags"][i] == 0 and r["trimmed"][i] == L[names[i]] - max(d, 0), (T, tag, d, r[i])
        c1 = oracle(parity.sized(margin_params(T, variant, reads[i:i + 1]), reads[i:i + 1]), reads[i:i + 1])[2]
        tallies.append((int(c1[abi.CTR_DROPINFO + 11]), int(c1[abi.CTR_DROPINFO + 12])))
    # overlapping and touching: ONE region that is the read (dl == L); a base between: two regions, and the base too short to keep
    assert tallies == [(1, 0), (1, 0), (1, 1)], (T, tag, tallies)


def margin_case(T, variant=None):
    def make():
        reads, designed = margin_reads(T)
        assert len(reads) <= 150 and max(len(r[1]) for r in reads) <= 4500
        p = margin_params(T, variant, reads)
        r, f, ctr = exp = oracle(p, reads)
        if variant in ("no_filter", "only_qc"):            # adapters are set and not searched for: every read comes back whole
            assert flagged(r, _AD) == 0 and (r["trimmed"] == 0).all(), (T, variant)
            assert variant == "only_qc" or ((r["n_frags"] == 1).all() and (f["len"] == [len(x[1]) for x in reads]).all()), (T, variant)
            return reads, p, exp
        names = [x[0] for x in reads]
        L = {x[0]: len(x[1]) for x in reads}
        if variant == "ends_only":
            assert flagged(r, abi.RF_AD5P) >= 5 and flagged(r, abi.RF_AD3P) >= 5 and flagged(r, abi.RF_ADMID) == 0, T
            for tag in (b"ends", b"sdne"):
                margin_ends(tag, T, variant, reads, names, L, r)
            return reads, p, exp
        assert flagged(r, abi.RF_AD5P) >= 5 and flagged(r, abi.RF_AD3P) >= 5 and flagged(r, abi.RF_ADMID) >= 5, (T, variant)
        if variant == "discard":
            assert flagged(r, abi.RF_DISCARDED) == flagged(r, abi.RF_ADMID), T
            return reads, p, exp

        def kept(name):
            i = names.index(name)
            return [(int(x["start"]), int(x["len"])) for x in f[r["frag_begin"][i]:r["frag_begin"][i] + r["n_frags"][i]]], int(r["trimmed"][i])
        if T <= 1000:
            # the pair whose margins touch is ONE region, as the pair that overlaps by a base; with a base between there are two,
            # and the base (shorter than min_len) is dropped: the same fragments but for the shift, another sum of dropped bases
            lead, tail = (300, 300) if T < 1000 else (60, 230)
            for d in (-1, 0, 1):
                fr, trimmed = kept(b"pair%+d" % d)
                s2 = T + lead + _MQ + 2 * T + d
                assert fr == [(0, lead), (s2 + _MQ + T, tail)], (T, d, fr)
                assert trimmed == 2 * _MQ + 4 * T + min(d, 0), (T, d, trimmed)
        else:
            assert all(kept(b"pair%+d" % d) == ([], L[b"pair%+d" % d]) for d in (-1, 0, 1)), T
        # one kept piece at each of the four seams of the lengths: two are kept, two are not
        for side in (b"keep", b"keep3_"):
            got = [kept(side + b"%d" % k)[0] for k in (MARGIN_MAX, MARGIN_MAX + 1)]
            assert [len(g) for g in got] == [1, 0] and got[0][0][1] == MARGIN_MAX, (T, side, got)
        if T <= 1000:
            got = [kept(b"gap%d" % k)[0] for k in (MARGIN_MIN - 1, MARGIN_MIN)]
            assert [len(g) for g in got] == [2, 3] and got[1][1][1] == MARGIN_MIN, (T, got)
        # dl == L: the read alone through the oracle leaves one count in DropInfo[11] and no base in DropInfo[12]
        for name in (b"whole2", b"whole1") + ((b"whole_mid",) if T >= 1000 else ()):
            i = names.index(name)
            _, _, c1 = oracle(parity.sized(margin_params(T, variant, reads[i:i + 1]), reads[i:i + 1]), reads[i:i + 1])
            assert kept(name) == ([], L[name]) and c1[abi.CTR_DROPINFO + 11] == 1 and c1[abi.CTR_DROPINFO + 12] == 0, (T, name, c1[:17])
        return reads, p, exp
    return cached(("margin", T, variant), make)


MARGIN_CASES = [(T, None) for T in MARGIN_T] + [(T, "discard") for T in (0, 50, BOUND)] + [(50, "no_filter"), (50, "only_qc"), (50, "ends_only")]


# ---------------------------------------------------------------------------
# S3: gates
# ---------------------------------------------------------------------------
GATE_ADS = [AD22, AD28, AD45]
GATE_QM = [(22, 16), (22, 20), (28, 20), (28, 25), (45, 36), (45, 41)]     # (the designed reads hold for these: sim_case asserts it)
GATE_MATCH = (1, 27, 28, 29, INT_MAX)                   # around the 28-bp member of the set
GATE_SIMS = (1.0, 1.5, 1e-30, float("inf"))


def sim_values(Q, m):
    """The float32 value m / Q as the reference's float division gives it, the float32 below it and the one above it."""
    s = np.float32(m) / np.float32(Q)
    return float(np.nextafter(s, np.float32(0))), float(s), float(np.nextafter(s, np.float32(2)))


def gate_reads(ads_subs):
    """For every (adapter, substitutions): one read with the copy near the 5' end, one near the 3' end, one in the middle;
    returns (reads, {(adapter index, substitutions): indices of its three reads})."""
    rng = np.random.default_rng(3000 + 7 * len(ads_subs) + sum(n for _, n in ads_subs))
    reads, where = [], {}
    for a, n in ads_subs:
        ad = GATE_ADS[a]
        where[(a, n)] = []
        for at_kind in range(3):
            L = 700 + 13 * a + at_kind
            at = (6, L - len(ad) - 9, L // 2)[at_kind]
            where[(a, n)].append(len(reads))
            reads.append(read_of(rng, b"a%d_s%d_%d" % (a, n, at_kind), planted(rng, L, [(at, substituted(rng, ad, n))])))
    for i in range(4):
        reads.append(read_of(rng, b"clean%d" % i, bases(rng, 500 + 100 * i)))
    return reads, where


def gate_params(reads, end_sim, mid_sim, end_match_len=1, mid_match_len=1):
    p = parity.sized(abi.make_params("ont", adapters=GATE_ADS, min_q=7.0, end_len=100, end_match_len=end_match_len, mid_match_len=mid_match_len, extra_len=10), reads)
    p.min_len = 50
    p.end_sim, p.mid_sim = end_sim, mid_sim             # (make_params clamps them as the reference's command line does)
    return p


def sim_case(Q, m, which):
    """Similarity gates at exactly m / Q (which = 1) and its neighbours (0: below, 2: above), match lengths of 1: copies of the
    Q-bp adapter with Q - m substitutions, one more and one fewer."""
    def make():
        a = [len(x) for x in GATE_ADS].index(Q)
        subs = [(a, Q - m - 1), (a, Q - m), (a, Q - m + 1)]
        reads, where = gate_reads(subs)
        outcomes = []
        for w in range(3):
            s = sim_values(Q, m)[w]
            p = gate_params(reads, s, s)
            exp = oracle(p, reads)
            outcomes.append(tuple(int(exp[0]["flags"][i] & _KIND[k]) for k, i in enumerate(where[(a, Q - m)])))
            if w == which:
                mine = (reads, p, exp)
        # the copy with exactly Q - m substitutions passes at m / Q and below it and fails above it, at either end and in the middle
        assert outcomes[0] == outcomes[1] == _KIND and outcomes[2] == (0, 0, 0), (Q, m, outcomes)
        return mine
    return cached(("sim", Q, m, which), make)


def _match_inputs():
    return gate_reads([(1, 0), (1, 1), (2, 0), (2, 1), (0, 0)])


def match_case(end_m, mid_m):
    """Match lengths around the 28-bp member's length in a set of 22, 28 and 45 bp: at 29 that member alone is switched off
    (k_end[a] < 0, k_mid[a] < 0), and the 22-bp one has been off since 23."""
    def make():
        reads, where = _match_inputs()
        p = gate_params(reads, 0.75, 0.9, end_m, mid_m)
        r, f, ctr = exp = oracle(p, reads)
        hit = {k: tuple(int(r["flags"][i] & _KIND[kind]) != 0 for kind, i in enumerate(v)) for k, v in where.items()}
        ends, mid = (0, 1), 2
        for m_len, at in ((end_m, ends), (mid_m, (mid,))):
            for k in at:
                assert hit[(1, 0)][k] == (m_len <= 28) and hit[(1, 1)][k] == (m_len <= 27), (end_m, mid_m, k, hit)
                assert hit[(2, 0)][k] == (m_len <= 45) and hit[(2, 1)][k] == (m_len <= 44), (end_m, mid_m, k, hit)
                assert hit[(0, 0)][k] == (m_len <= 22), (end_m, mid_m, k, hit)
        return reads, p, exp
    return cached(("match", end_m, mid_m), make)


MATCH_CASES = [(m, m) for m in GATE_MATCH] + [(1, 29), (29, 1), (INT_MAX, 28)]


def loose_case(sim):
    """Similarities nobody would ask for: 1.0 (exact copies only), 1.5 and +inf (nothing passes; the 5' window of +inf is E
    wide), 1e-30 (every window is the read and every alignment within the match lengths passes)."""
    def make():
        reads, where = _match_inputs()
        p = gate_params(reads, sim, sim, 15, 20)
        r, f, ctr = exp = oracle(p, reads)
        hit = {k: all(int(r["flags"][i] & _AD) != 0 for i in v) for k, v in where.items()}
        if sim == 1.0:
            assert hit[(1, 0)] and hit[(2, 0)] and hit[(0, 0)] and not hit[(1, 1)] and not hit[(2, 1)], hit
        elif sim > 1.0:
            assert flagged(r, _AD) == 0, sim
        else:
            assert all(hit.values()) and flagged(r, _AD) >= len(reads) - 4, hit
        return reads, p, exp
    return cached(("loose", sim), make)


TINY_ADS = [b"GATTC", b"CCATGA", AD22]


def tiny_case():
    """End windows of 4, 5 and 6 columns against adapters of 5 and 6 bp (-m 4): a window of fewer than 5 columns is not searched
    (the reference's `checkLen >= 5`), one of exactly 5 is."""
    def make():
        rng = np.random.default_rng(3500)
        reads = [read_of(rng, b"w%d_%d" % (len(s), i), s) for i, s in enumerate((b"GATT", b"GATTC", b"GATTCA", b"CCATG", b"CCATGA", b"TGATTCA", b"ACGTA", b"GAT", b"G"))]
        reads += [read_of(rng, b"long%d" % i, planted(rng, 300 + i, [(at, ad)])) for i, (at, ad) in enumerate(((0, TINY_ADS[0]), (294, TINY_ADS[1]), (150, TINY_ADS[0]), (2, AD22)))]
        p = parity.sized(abi.make_params("ont", adapters=TINY_ADS, min_q=7.0, end_len=2, end_match_len=4, mid_match_len=5, extra_len=0), reads)
        p.min_len = 1
        p.end_sim, p.mid_sim = 0.75, 0.9
        r, f, ctr = exp = oracle(p, reads)
        hit = [int(x & _AD) != 0 for x in r["flags"][:9]]
        assert hit[:3] == [False, True, True] and hit[3] and hit[4] and not hit[7] and not hit[8], hit
        return reads, p, exp
    return cached(("tiny",), make)


# ---------------------------------------------------------------------------
# S4: adapter sets
# ---------------------------------------------------------------------------
def _random_ads(seed, lengths):
    rng = np.random.default_rng(seed)
    return [bases(rng, int(L)) for L in lengths]


def _interleave(xs, ys):
    out = []
    for x, y in zip(xs, ys):
        out += [x, y]
    return out


_LIB9 = [synth.PACBIO_BLUNT, AD28, synth.PACBIO_BLUNT_RC, synth.ONT_RAPID, AD45, AD22, synth.ONT_RAPID_RC, AD150, synth.revcomp(AD45)]
_SHORT = _random_ads(41, [20 + (7 * i) % 13 for i in range(32)])                      # 20..32 bp: one dword a column, two a pass
_QWORD = _random_ads(42, [33 + (11 * i) % 32 for i in range(32)])                     # 33..64 bp
_NEAR = _random_ads(43, [36 + i % 11 for i in range(16)])                             # 36..46 bp: within kSuffixMaxK differences at -M 35
_FAR = _random_ads(44, [47 + i % 18 for i in range(16)])                              # 47..64 bp: beyond
# runs of 1, 2, 3 and 4 members of the qword class (one pass each) between runs of 1, 2 and 3 of the dword class (passes of 1, 2, 2 + 1)
_RUNS = "Q S QQ SS QQQ SSS QQQQ S QQ SSS Q SS QQQQ S QQ".replace(" ", "")
assert len(_RUNS) == 32


def _runs_set():
    s, q = iter(_SHORT), iter(_QWORD)
    return [next(s) if c == "S" else next(q) for c in _RUNS]


def _wide_set():
    out = list(_SHORT[:28])
    for at, L in ((3, 100), (12, 150), (21, 230), (29, 300)):
        out.insert(at, _random_ads(45 + L, [L])[0])
    return out


SETS = {
    "none": ([], 35),
    "one": ([synth.ONT_RAPID], 35),
    "five": (_LIB9[:5], 20),
    "same5": ([synth.ONT_RAPID] * 5, 35),
    "eight": (_LIB9[:8], 20),
    "nine": (_LIB9, 20),
    "nested": ([synth.ONT_RAPID, synth.ONT_RAPID[10:40], AD45, synth.revcomp(AD45), synth.ONT_RAPID_RC, synth.ONT_RAPID[:28]], 20),
    "seventeen": (_LIB9 + _SHORT[:4] + _QWORD[:4], 20),
    "short32": (_SHORT, 18),
    "qword32": (_QWORD, 30),
    "alternating32": (_interleave(_SHORT[:16], _QWORD[:16]), 20),
    "runs32": (_runs_set(), 20),
    "suffix32": (_interleave(_NEAR, _FAR), 35),            # the filtered and the unfiltered class of the flat scan, one by one
    "wide32": (_wide_set(), 18),                           # one each of 65..128, 129..192, 193..256 and 257+ bp among short ones, the last at index 29
    "lengths32": (_random_ads(46, [1, 2, 4, 5, 31, 32, 33, 63, 64, 65, 128, 129, 192, 193, 256, 24, 48, 40, 30, 36, 22, 60, 28, 50, 26, 44, 34, 27, 25, 37, 29, 52]), 20),
}
assert all(len(s) <= 32 for s, _ in SETS.values()) and sum(len(s) == 32 for s, _ in SETS.values()) == 7
SET_ENVS = {"default": {}, "pool3": {"TGSF_POOL_CAP": "3"}, "segments": {"TGSF_MID_FLAT": "0"}, "segments_pool3": {"TGSF_MID_FLAT": "0", "TGSF_POOL_CAP": "3"},
            "filter0": {"TGSF_MID_FILTER": "0"}, "filter1": {"TGSF_MID_FILTER": "1"}, "filter2": {"TGSF_MID_FILTER": "2"}}
SET_CASES = [(name, "default") for name in SETS] + [(name, env) for name in ("runs32", "lengths32", "suffix32") for env in SET_ENVS if env != "default"]
SET_CASES.append(("wide32", "pool3"))     # the wide column through the count-and-rescan path and the per-slot resolve
SET_READS = 96


def set_reads(name):
    """The fixed 96 backbones (the same generator state for every set), read i carrying a lightly mutated copy of member i % A
    near its 5' end, near its 3' end or in its middle ((i // A + i) % 3)."""
    ads, _ = SETS[name]
    rng = np.random.default_rng(4000)
    lens = rng.integers(400, 1300, SET_READS)
    backs = [bases(rng, int(L)) for L in lens]
    rng = np.random.default_rng(4001)
    reads = []
    for i, s in enumerate(backs):
        s = bytearray(s)
        if ads:
            a = i % len(ads)
            Q = len(ads[a])
            copy = substituted(rng, ads[a], Q // 25 if i % 2 else 0)
            L = len(s)
            if Q + 20 > L // 2:
                s = bytearray(bases(rng, 4 * Q + 400))
                L = len(s)
            at = (4, L - Q - 5, L // 2)[(i // len(ads) + i) % 3]
            s[at:at + Q] = copy
        reads.append(read_of(rng, b"set%d" % i, s))
    return reads


def set_params(name, reads):
    ads, mid_m = SETS[name]
    p = parity.sized(abi.make_params("ont", adapters=ads, min_q=7.0, end_len=150, end_match_len=15, mid_match_len=mid_m, extra_len=50, head_trim=3, tail_trim=2), reads)
    p.min_len = 50
    return p


def set_case(name):
    def make():
        ads, _ = SETS[name]
        reads = set_reads(name)
        p = set_params(name, reads)
        r, f, ctr = exp = oracle(p, reads)
        A = len(ads)
        if A == 0:
            assert flagged(r, _AD) == 0 and (r["n_frags"] == 1).all()
            return reads, p, exp
        assert flagged(r, abi.RF_AD5P) >= 5 and flagged(r, abi.RF_AD3P) >= 5 and flagged(r, abi.RF_ADMID) >= 5, name
        # which members produce a hit: each one alone through the oracle
        alone = []
        for a in range(A):
            pa = parity.sized(abi.make_params("ont", adapters=[ads[a]], min_q=7.0, end_len=150, end_match_len=15, mid_match_len=SETS[name][1], extra_len=50), reads)
            pa.min_len = 50
            alone.append(flagged(oracle(pa, reads)[0], _AD) > 0)
        assert sum(alone) >= (A + 1) // 2, (name, sum(alone))
        if A == 32:
            assert any(alone[28:]), name
        if name == "same5":                                # every copy of the adapter counts and the regions coincide: the fragments of one copy
            p1 = set_params(name, reads)
            p1.n_adapters = 1
            r1, f1, _ = oracle(p1, reads)
            assert np.array_equal(r1, r) and np.array_equal(f1, f)
        return reads, p, exp
    return cached(("set", name), make)


def device_batch(name):
    """GPU only: the set's batch through tgsf_submit_device and tgsf_wait with a candidate pool of 3 slots -- the first run
    overflows, says so in the fragment count, and the batch is run again from its inputs in position order."""
    import torch
    reads, p, (exp_r, exp_f, exp_ctr) = set_case(name)
    seq, qual, offsets, lengths = synth.pack(reads)
    ctx = capi.Context(p, 0)
    try:
        dev = torch.device("cuda", 0)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("seq", seq), ("qual", qual), ("off", offsets[:-1].astype(np.int64)), ("len", lengths.astype(np.int32)))}
        n, fcap = len(reads), len(exp_f) + 64
        d_reads = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_frags = torch.zeros(fcap * 24, dtype=torch.uint8, device=dev)
        d_nf = torch.zeros(4, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        ctx.submit_device(d["seq"].data_ptr(), d["qual"].data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(), n, seq.size,
                          d_reads.data_ptr(), d_frags.data_ptr(), fcap, d_nf.data_ptr(), st.cuda_stream)
        st.synchronize()
        first = int(d_nf[0].item()) & 0xFFFFFFFF
        ctx.wait()
        st.synchronize()
        got_r = d_reads.cpu().numpy().view(abi.READ_RESULT_DTYPE)
        got_f = d_frags.cpu().numpy().view(abi.FRAGMENT_DTYPE)[:int(d_nf[0].item())]
        for field in ("sum_q", "flags", "n_frags", "frag_begin", "trimmed"):
            assert np.array_equal(got_r[field], exp_r[field]), field
        assert np.array_equal(got_f, exp_f) and np.array_equal(ctx.counters(), exp_ctr)
        return first
    finally:
        ctx.close()
