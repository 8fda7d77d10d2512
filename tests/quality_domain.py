"""The quality gates and the QC tallies across their domain: q_fail / mean_q (tgsf_core.h) as k_gate_reads, k_gate_frags and
k_prepare use them, the two DiffQual histograms, and k_end_tables on the seams of its slots and slabs.

The rest of the suite gates random qualities on integer thresholds: no mean lies on a threshold, none is an integer.  Here
every read is built by construction -- a length, a sum of `qual - qType`, then the bytes (lay_out):

  Q1  the raw gate: for thresholds 0, 7, 7.5, 12.25, 9.9f, 20.3f, 60.1f and 94, as min_q and as max_q, reads whose double mean
      is the largest sum / L below the threshold, equal to it where an integer sum gives it, and the smallest above it, run at
      the threshold and its two float32 neighbours; the same sums through bytes of 128 and above (negative after `- qType`)
      and under qType 64: raw_gate_case().  min_q == max_q, min_q > max_q, -1, -0.0, NaN and the infinities: special_case();
  Q2  one long read per threshold that is not a double of few bits, on which a mean held in float32 (or formed as
      (float)sum / (float)L) gives the other answer -- the shortest such read: long_case(), float_disagreement(); the first
      power of two bases with that property, where the threshold itself is a mean as well: mega_case();
  Q3  sum 0 (bin 0) and sum -1 (TGSF_E_DATA, the read named): zero_sum_case(), negative_sum();
  Q4  the histograms' index: means of k, k - 1/L and k + 1/L for k in 0, 1, 2, 63, 93, 94 with filter = 1, filter = 0 and
      only_qc, and the four rows-in-use words: hist_case();
  Q5  the gate after the split: reads whose raw mean passes and whose kept part lies on, one sum below and one above the
      threshold -- kept by a fixed -5 / -3, by an end adapter's clip, and as the two pieces beside a middle adapter, one on
      either side of the threshold -- under every clean-table strategy: post_case();
  Q6  k_prepare's guess: 64 sampled bytes that say pass on a read that fails by 1 / L, the reverse, and a guess equal to the
      threshold, with the by-product forced: guess_case();
  Q7  nothing counted twice: the seam reads beside one read that overflows the candidate pool, through tgsf_submit (run twice
      inside tgsf_wait) and through tgsf_submit_device: replay_case(), replay_device();
  E1  bc_len 0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4096 against reads of 1, bc - 1, bc, bc + 1, 2 bc - 1, 2 bc and
      2 bc + 1 bases, with qualities, without, and under fixed trims; a lower-case g and t on the first and last counted
      position, a quality byte of 128 and above on position bc - 1 from either end: end_case().  bc_len 2^20 with a read of
      2^20 + 1 bases: widest_case().

Every comparison is parity.compare_batch against orc.filter_batch: all record fields, all fragment fields, every tally word.
No tolerance anywhere.  Each input is asserted on the oracle's result alone first, against expectations stated in numpy
float64 / float32 (gate_fails): a case that stops meaning what it says fails without the library.
tests/test_quality_emul.py runs all of it on the serial emulation, tests/test_quality_gpu.py on the HIP build."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from oracle import orc
from tests import parity, refusals
from tests.search_domain import MARGIN_ADS, cached, prefetch, set_env  # noqa: F401  (prefetch: for the runners)
from tests.search_domain import run as search_run
from tgsfilter_amd import abi, capi, synth

F32 = np.float32
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
THRESHOLDS = {"0": 0.0, "7": 7.0, "7.5": 7.5, "12.25": 12.25, "9.9f": float(F32(9.9)), "20.3f": float(F32(20.3)), "60.1f": float(F32(60.1)), "94": 94.0}
NOT_FEW_BITS = ("9.9f", "20.3f", "60.1f")           # float32 values whose double needs all 24 bits: no small L reaches them
CLEAN_MODES = ("direct", "difference", "byproduct", None)


def oracle(p, reads):
    seq, qual, offsets, lengths = synth.pack(reads)
    return orc.filter_batch(p, seq, qual, offsets, lengths)


def lowq(r):
    return (r["flags"] & abi.RF_LOWQ) != 0


def neighbours(t):
    """The float32 below t, t, and the float32 above t."""
    t = F32(t)
    return float(np.nextafter(t, F32(-np.inf))), float(t), float(np.nextafter(t, F32(np.inf)))


def seam_sums(t, L):
    """In exact arithmetic: (the largest integer sum with sum / L < t, the sum with sum / L == t or None, the smallest with
    sum / L > t)."""
    x = Fraction(t) * L
    fl = x.numerator // x.denominator
    at = fl if x.denominator == 1 else None
    return (fl - 1 if at is not None else fl), at, fl + 1


def gate_fails(total, L, min_q, max_q):
    """The reference's gate restated: the double quotient of the sum, compared with the float32 thresholds as doubles."""
    mean = np.float64(total) / np.float64(L)
    return bool(mean < np.float64(F32(min_q)) or mean > np.float64(F32(max_q)))


def bases(rng, L):
    return _ACGT[rng.integers(0, 4, L)].tobytes()


def lay_out(rng, L, total, qtype=33, high=0):
    """L quality bytes whose values -- byte - qtype, a byte of 128 and above standing for byte - 256 -- sum to `total`:
    `high` of them are bytes of 128 and above, the others are as equal as the sum allows, of values 0 .. 127 - qtype, in a
    drawn order.  None where no such bytes exist."""
    hi_bytes = rng.integers(128, 256, high)
    rest, n = int(total) - int((hi_bytes - 256 - qtype).sum()), L - high
    if n < 0 or (n == 0 and rest != 0):
        return None
    q = np.empty(L, dtype=np.int64)
    q[:high] = hi_bytes
    if n:
        base, rem = divmod(rest, n)
        if base < 0 or base + (rem > 0) > 127 - qtype:
            return None
        q[high:] = base + qtype
        q[high:high + rem] += 1
    q = q[rng.permutation(L)].astype(np.uint8)
    value = np.where(q >= 128, q.astype(np.int64) - 256, q.astype(np.int64)) - qtype
    assert int(value.sum()) == total and (q >= 128).sum() == high
    return q.tobytes()


def params(reads, min_q, max_q, *, adapters=(), min_len=1, **kw):
    p = parity.sized(abi.make_params("ont", adapters=adapters, **kw), reads)
    p.min_len = min_len                               # (make_params clamps it to 100 and the similarities as the command line does)
    p.min_q, p.max_q = min_q, max_q                   # any float at all: tgsf_create refuses none
    return p


def run(lib_path, case, env, monkeypatch):
    """search_domain.run over a case = (reads, parameters, the oracle's result)."""
    reads, p, exp = case
    search_run(lib_path, p, reads, exp, env, monkeypatch)


def mode_env(mode):
    return {"TGSF_CLEAN_TABLES": mode} if mode else {}


# ---------------------------------------------------------------------------
# Q1: the raw gate on its thresholds
# ---------------------------------------------------------------------------
GATE_L = (1, 2, 3, 4, 99, 100, 101, 12800)
GATE_CASES = [(name, side, w, 33) for name in THRESHOLDS for side in ("min", "max") for w in range(3)] + \
             [(name, side, 1, 64) for name in THRESHOLDS if name != "94" for side in ("min", "max")]       # (qType 64: values of 0 .. 63)


def gate_reads(t, qtype=33, seed=0):
    """(reads, what each is: (L, sum, "below" | "at" | "above", bytes of 128 and above)).  A sum no bytes give (a mean above
    127 - qtype; bytes of 128 and above that nothing beside them makes up for) has no read; a sum below 0 is negative_sum()'s."""
    rng = np.random.default_rng(5000 + seed + int(t * 1000))
    reads, what = [], []
    for L in GATE_L:
        for kind, total in zip(("below", "at", "above"), seam_sums(t, L)):
            if total is None or total < 0:
                continue
            for high in (0, 1 + L // 40):
                q = lay_out(rng, L, total, qtype, high) if high < L else None
                if q is not None:
                    reads.append((b"%s_L%d_h%d" % (kind.encode(), L, high), bases(rng, L), q))
                    what.append((L, total, kind, high))
    return reads, what


def _gate_triple(name, side, qtype):
    """The reads of one threshold under it and its two float32 neighbours: [(reads, p, exp)] * 3, asserted on the oracle."""
    def make():
        t = THRESHOLDS[name]
        reads, what = gate_reads(t, qtype)
        out, flags = [], []
        for v in neighbours(t):
            p = params(reads, v if side == "min" else 0.0, 255.0 if side == "min" else v, qtype=qtype)
            exp = oracle(p, reads)
            assert lowq(exp[0]).tolist() == [gate_fails(s, L, p.min_q, p.max_q) for L, s, _, _ in what], (name, side, v)
            assert (exp[0]["sum_q"] == [s for _, s, _, _ in what]).all()
            out.append((reads, p, exp))
            flags.append(lowq(exp[0]))
        kinds = [k for _, _, k, _ in what]
        # at the threshold itself: one sum below it fails a min_q and passes a max_q, one sum above it the other way round
        assert all(flags[1][i] == (side == "min") for i, k in enumerate(kinds) if k == "below"), (name, side)
        assert all(flags[1][i] == (side == "max") for i, k in enumerate(kinds) if k == "above"), (name, side)
        assert "below" in kinds or t == 0.0
        assert "above" in kinds or t == 127 - qtype
        # a read exactly on it is kept at the threshold (the comparisons are strict) and dropped at the neighbour inside
        at = [i for i, k in enumerate(kinds) if k == "at"]
        assert bool(at) == (name not in NOT_FEW_BITS), (name, len(at))
        for i in at:
            got = tuple(bool(fl[i]) for fl in flags)
            assert got == ((False, False, True) if side == "min" else (True, False, False)), (name, side, what[i], got)
        if t not in (0.0, 94.0) and (qtype == 33 or t < 30):
            assert any(h for _, _, _, h in what), name        # the same seams through bytes of 128 and above
        return out
    return cached(("gate", name, side, qtype), make)


def raw_gate_case(name, side, w, qtype=33):
    return _gate_triple(name, side, qtype)[w]


SPECIAL = {"equal": (7.5, 7.5), "crossed": (12.25, 7.5), "min_-1": (-1.0, 255.0), "min_-0.0": (-0.0, 255.0), "max_-0.0": (0.0, -0.0), "max_-1": (0.0, -1.0),
           "min_nan": (float("nan"), 255.0), "max_nan": (0.0, float("nan")), "both_nan": (float("nan"), float("nan")),
           "min_+inf": (float("inf"), 255.0), "min_-inf": (float("-inf"), 255.0), "max_+inf": (0.0, float("inf")), "max_-inf": (0.0, float("-inf"))}


def special_case(name):
    """Thresholds the ABI does not refuse, over the seam reads of 7.5 and of 0 (sums of 0 among them)."""
    def make():
        min_q, max_q = SPECIAL[name]
        reads, what = gate_reads(7.5)
        more, what0 = gate_reads(0.0, seed=1)
        reads, what = reads + more, what + [(L, s, "zero" if s == 0 else "one", h) for L, s, _, h in what0]
        p = params(reads, min_q, max_q)
        exp = oracle(p, reads)
        fails = lowq(exp[0])
        assert fails.tolist() == [gate_fails(s, L, min_q, max_q) for L, s, _, _ in what], name
        kinds = np.array([k for _, _, k, _ in what])
        if name == "equal":                                  # the reads exactly on it are kept, and nothing else
            assert (fails == (kinds != "at")).all() and (kinds == "at").sum() >= 3
        elif name in ("crossed", "min_+inf", "max_-inf", "max_-1"):
            assert fails.all(), name
        elif name in ("min_-1", "min_-0.0", "min_nan", "max_nan", "both_nan", "min_-inf", "max_+inf"):
            assert not fails.any(), name                     # (a comparison with NaN is false: nothing fails)
        else:                                                # a mean of 0 is not above -0.0
            assert name == "max_-0.0" and (fails == (kinds != "zero")).all() and (kinds == "zero").sum() >= 3
        return reads, p, exp
    return cached(("special", name), make)


# ---------------------------------------------------------------------------
# Q2: one long read on which a float mean gives the other answer
# ---------------------------------------------------------------------------
LONG_SEARCH = (1 << 22) + 1
# What float_disagreement() finds: the smallest L at which BOTH restatements below give the other answer than the double
# gate -- on the largest sum / L below the threshold as a min_q, on the smallest above it as a max_q (long_case asserts them).
LONG_L = {("9.9f", "min"): 116509, ("9.9f", "max"): 10, ("20.3f", "min"): 58257, ("20.3f", "max"): 10, ("60.1f", "min"): 29131, ("60.1f", "max"): 10}
# ... and the smallest power of two with the same property as a min_q: there the threshold itself is a mean (mega_case)
MEGA_L = {"9.9f": 1 << 21, "20.3f": 1 << 20, "60.1f": 1 << 19}


def float_gates(total, L, t, side):
    """For arrays of sums and lengths against the float32 threshold t: (the double gate, a mean held in float32, a mean formed
    as (float)sum / (float)L) -- True where the read fails."""
    t32, td = F32(t), np.float64(F32(t))
    mean = total.astype(np.float64) / L.astype(np.float64)
    in_float = mean.astype(F32)
    from_floats = total.astype(F32) / L.astype(F32)
    if side == "min":
        return mean < td, in_float < t32, from_floats.astype(np.float64) < td
    return mean > td, in_float > t32, from_floats.astype(np.float64) > td


def float_disagreement(name, side):
    """(L, sum): the smallest L <= 2^22 whose seam read -- the largest sum / L below the threshold for a min_q, the smallest
    above it for a max_q -- is judged the other way by both float restatements."""
    def make():
        t = Fraction(THRESHOLDS[name])
        L = np.arange(1, LONG_SEARCH, dtype=np.int64)
        x = L * t.numerator                                   # (below 2^24 * 2^23)
        fl, frac = x // t.denominator, x % t.denominator
        total = np.where(frac == 0, fl - 1, fl) if side == "min" else fl + 1
        dbl, a, b = float_gates(total, L, THRESHOLDS[name], side)
        at = np.nonzero((a != dbl) & (b != dbl) & dbl)[0]
        assert at.size, (name, side)
        return int(L[at[0]]), int(total[at[0]])
    return cached(("disagree", name, side), make)


def long_case(name, side):
    """The smallest L found, per threshold and side (float_disagreement: every L from 1 to 2^22 in numpy, the gate in float64
    and float32 as float_gates states it):
        9.9f   min_q: L = 116 509 (sum 1 153 439)    max_q: L = 10 (sum  99)
        20.3f  min_q: L =  58 257 (sum 1 182 617)    max_q: L = 10 (sum 203)
        60.1f  min_q: L =  29 131 (sum 1 750 773)    max_q: L = 10 (sum 601)
    The three float32 values lie just below 9.9, 20.3 and 60.1: ten bytes that sum to 99 have a double mean above 9.9f whose
    float32 image is 9.9f, not above it.  From below, L * threshold has to fall within half a float32 step times L above an
    integer: the first such L are the ones listed.  The read has no adapter set to search for: the middle scan costs nothing."""
    def make():
        L, total = float_disagreement(name, side)
        assert L == LONG_L[(name, side)], (name, side, L)
        t = THRESHOLDS[name]
        one = (np.array([total]), np.array([L]))
        dbl, in_float, from_floats = (bool(x[0]) for x in float_gates(*one, t, side))
        assert dbl and not in_float and not from_floats, (name, side, L, total)
        rng = np.random.default_rng(L)
        reads = [(b"long_%s_%s" % (name.encode(), side.encode()), bases(rng, L), lay_out(rng, L, total))]
        p = params(reads, t if side == "min" else 0.0, 255.0 if side == "min" else t, bc_len=64)
        exp = oracle(p, reads)
        assert lowq(exp[0]).all() and int(exp[0]["sum_q"][0]) == total and exp[2][abi.CTR_DROPINFO + 1] == L
        return reads, p, exp
    return cached(("long", name, side), make)


def mega_case(name):
    """Three reads of a power of two bases -- 2^19 for 60.1f, 2^20 for 20.3f, 2^21 for 9.9f: the smallest at which the largest
    sum / L below the threshold has the threshold as its float32 image (asserted here for this L, and for half of it that
    both float restatements still agree with the double gate); the threshold itself is a mean there.  One sum below the
    threshold, the one on it and one above it, gated as a min_q: one batch of three such reads a test (7 Mbases at
    the most, no adapter to search for), built for that test and not kept."""
    def make():
        L, t = MEGA_L[name], THRESHOLDS[name]
        sums = seam_sums(t, L)
        assert sums[1] is not None
        dbl, in_float, from_floats = float_gates(np.array(sums), np.array([L] * 3), t, "min")
        assert dbl.tolist() == [True, False, False] and not in_float.any() and not from_floats.any(), (name, dbl, in_float, from_floats)
        half = seam_sums(t, L // 2)[0]
        assert all(x[0] for x in float_gates(np.array([half]), np.array([L // 2]), t, "min")), name
        rng = np.random.default_rng(L)
        reads = [(b"mega_%s_%d" % (name.encode(), k), bases(rng, L), lay_out(rng, L, total)) for k, total in enumerate(sums)]
        p = params(reads, t, 255.0, bc_len=64)
        exp = oracle(p, reads)
        assert lowq(exp[0]).tolist() == [True, False, False]
        return reads, p, exp
    return make()                                     # (not kept: three reads of up to 2^21 bases; one test on either build runs each)


# ---------------------------------------------------------------------------
# Q3: sums of 0 and of -1
# ---------------------------------------------------------------------------
def zero_sum_case():
    def make():
        rng = np.random.default_rng(33)
        reads = [(b"zero%d" % L, bases(rng, L), b"!" * L) for L in (1, 2, 99, 100, 101, 6400, 6401)]
        p = params(reads, 0.0, 0.0)
        r, f, ctr = exp = oracle(p, reads)
        total = sum(len(x[1]) for x in reads)
        assert not lowq(r).any() and (r["n_frags"] == 1).all() and (r["sum_q"] == 0).all()
        for table in (abi.CTR_RAW_DIFFQ, abi.CTR_CLEAN_DIFFQ):
            assert ctr[table] == total and not ctr[table + 1:table + 256].any()
        return reads, p, exp
    return cached(("zero",), make)


def negative_sum(lib_path, at, monkeypatch):
    """One byte of 32 among `!`: a sum of -1, a mean outside [0, 256) -- the reference indexes its histogram out of bounds,
    the oracle answers TGSF_E_DATA and so does the library, naming the read."""
    set_env(monkeypatch, {})
    reads, p, _ = zero_sum_case()
    reads = list(reads)
    name, s, q = reads[at]
    reads[at] = (name, s, q[:len(q) // 2] + b" " + q[len(q) // 2 + 1:])
    seq, qual, off, ln = synth.pack(reads)
    try:
        orc.filter_batch(p, seq, qual, off, ln)
        raise AssertionError("the oracle accepted a sum of -1")
    except RuntimeError as e:
        assert str(abi.E_DATA) in str(e)
    ctx = capi.Context(p, 0, lib_path)
    try:
        refusals.raises(lambda: ctx.submit(seq, qual, off[:-1].copy(), ln), abi.E_DATA, "read %d:" % at, "mean quality outside [0,256)")
        ctx.reset_counters()
        parity.compare_batch(ctx, p, zero_sum_case()[0], expected=zero_sum_case()[2])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# Q4: the histograms' index
# ---------------------------------------------------------------------------
HIST_K = (0, 1, 2, 63, 93, 94)
HIST_L = (1, 2, 99, 100, 101, 12800)
HIST_MODES = ("filter", "no_filter", "only_qc")


def hist_case(mode):
    def make():
        rng = np.random.default_rng(44)
        reads, what = [], []
        for k in HIST_K:
            for L in HIST_L:
                for d in (-1, 0, 1):
                    q = lay_out(rng, L, k * L + d) if k * L + d >= 0 else None      # (no bytes give a mean above 94 under qType 33)
                    if q is not None:
                        reads.append((b"k%d_L%d_%+d" % (k, L, d), bases(rng, L), q))
                        what.append((L, k * L + d))
        assert len(reads) >= 3 * len(HIST_K) * len(HIST_L) - 2 * len(HIST_L)
        p = params(reads, 0.0, 255.0, filter=mode != "no_filter", only_qc=mode == "only_qc")
        r, f, ctr = exp = oracle(p, reads)
        hist = np.zeros(256, dtype=np.uint64)
        for L, total in what:
            hist[int(np.float64(total) / np.float64(L))] += np.uint64(L)        # truncated, not rounded: k - 1/L lies in bin k - 1
        assert sorted(np.nonzero(hist)[0]) == [0, 1, 2, 3, 62, 63, 64, 92, 93, 94]
        assert np.array_equal(ctr[abi.CTR_RAW_DIFFQ:abi.CTR_RAW_DIFFQ + 256], hist)
        assert np.array_equal(ctr[abi.CTR_CLEAN_DIFFQ:abi.CTR_CLEAN_DIFFQ + 256], hist * np.uint64(mode != "only_qc"))
        rows = [12800 // 100 + 1, 0 if mode == "only_qc" else 12800 // 100 + 1, 150, 0 if mode == "only_qc" else 150]
        assert ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4].tolist() == rows, ctr[abi.CTR_ROWS:abi.CTR_ROWS + 4]
        assert not lowq(r).any()
        return reads, p, exp
    return cached(("hist", mode), make)


# ---------------------------------------------------------------------------
# Q5: the gate after the split
# ---------------------------------------------------------------------------
POST_T = 12.25
POST_MIN_LEN = 50
POST_HEAD, POST_TAIL = 10, 7
POST_WAYS = ("trim", "adapter")
_Q = len(MARGIN_ADS[0])
_T = 50                                               # extra_len


def post_reads(side):
    """{way: (reads, [the fragments each read is designed to give: (start, len, sum)])}.  Whatever is not kept -- the trimmed
    ends, the adapter, its margins -- has qualities of 93 against a min_q and of 0 against a max_q: the raw mean passes."""
    rng = np.random.default_rng(55 + (side == "max"))
    fill = 93 if side == "min" else 0
    out = {"trim": ([], []), "adapter": ([], [])}

    def piece(K, kind):
        total = dict(zip(("below", "at", "above"), seam_sums(POST_T, K)))[kind]
        return lay_out(rng, K, total), total

    def filler(n):
        return bytes([fill + 33]) * n
    for K in (52, 100, 104, 6400):
        for kind in ("below", "at", "above"):
            q, total = piece(K, kind)
            reads, frags = out["trim"]
            reads.append((b"trim_%s_%d" % (kind.encode(), K), bases(rng, POST_HEAD + K + POST_TAIL), filler(POST_HEAD) + q + filler(POST_TAIL)))
            frags.append([(POST_HEAD, K, total)])
    ad, rc = MARGIN_ADS
    for K in (300, 304, 700):                         # (beyond the other end's window of 216 bases, which would find the same copy)
        for kind in ("below", "at", "above"):
            reads, frags = out["adapter"]
            q, total = piece(K, kind)
            reads.append((b"clip5_%s_%d" % (kind.encode(), K), ad + bases(rng, K), filler(_Q) + q))
            frags.append([(_Q, K, total)])
            q, total = piece(K, kind)
            reads.append((b"clip3_%s_%d" % (kind.encode(), K), bases(rng, K) + rc, q + filler(_Q)))
            frags.append([(0, K, total)])
    for k1, k2 in (("below", "above"), ("above", "below"), ("at", "below"), ("below", "at"), ("above", "at"), ("below", "below"), ("above", "above")):
        for K1, K2 in ((300, 304), (404, 6400)):
            reads, frags = out["adapter"]
            (q1, s1), (q2, s2) = piece(K1, k1), piece(K2, k2)
            mid = 2 * _T + _Q
            s = bytearray(bases(rng, K1 + mid + K2))
            s[K1 + _T:K1 + _T + _Q] = ad if K1 == 300 else rc
            reads.append((b"split_%s_%s_%d" % (k1.encode(), k2.encode(), K1), bytes(s), q1 + filler(mid) + q2))
            frags.append([(0, K1, s1), (K1 + mid, K2, s2)])
    return out


def post_params(side, way, reads):
    gate = (POST_T, 255.0) if side == "min" else (0.0, POST_T)
    if way == "trim":
        return params(reads, *gate, min_len=POST_MIN_LEN, head_trim=POST_HEAD, tail_trim=POST_TAIL)
    return params(reads, *gate, adapters=MARGIN_ADS, min_len=POST_MIN_LEN, end_len=150, end_match_len=15, mid_match_len=35, extra_len=_T)


def post_case(side, way):
    def make():
        reads, designed = post_reads(side)[way]
        p = post_params(side, way, reads)
        r, f, ctr = exp = oracle(p, reads)
        assert not lowq(r).any(), (side, way)                  # the raw mean of every read passes
        n_fail = b_fail = b_all = b_pass = n_pass = 0
        for i, want in enumerate(designed):
            got = f[r["frag_begin"][i]:r["frag_begin"][i] + r["n_frags"][i]]
            assert [(int(x["start"]), int(x["len"]), int(x["sum_q"])) for x in got] == want, (side, way, reads[i][0], got, want)
            for x, (_, K, total) in zip(got, want):
                fails = gate_fails(total, K, p.min_q, p.max_q)
                assert bool(x["flags"] & abi.FF_PASS) != fails, (side, way, reads[i][0])
                n_fail, b_fail, b_all = n_fail + fails, b_fail + K * fails, b_all + K
                n_pass, b_pass = n_pass + (not fails), b_pass + K * (not fails)
        assert n_fail >= len(designed) // 3 and n_pass >= len(designed) // 2, (side, way, n_fail, n_pass)
        assert (ctr[abi.CTR_DROPINFO + 13], ctr[abi.CTR_DROPINFO + 14]) == (n_fail, b_fail), (side, way)
        # the failing fragments are in the clean bin tables (tallied before the gate) and neither in the clean histogram nor
        # in the clean 5' / 3' tables (tallied after it)
        n_bins = abi.n_bins(p.max_read_len)
        cnt = ctr[abi.ctr_bin_table(abi.B_CLEAN_CNT, p.bc_len, n_bins):abi.ctr_bin_table(abi.B_CLEAN_CNT + 1, p.bc_len, n_bins)].reshape(-1, 5)
        assert int(cnt[:, 4].sum()) == b_all and b_all > b_pass
        assert int(ctr[abi.CTR_CLEAN_DIFFQ:abi.CTR_CLEAN_DIFFQ + 256].sum()) == b_pass
        for t in (abi.T_CLEAN5P_CNT, abi.T_CLEAN3P_CNT):
            assert int(ctr[abi.ctr_end_table(t, p.bc_len) + 4]) == n_pass and int(ctr[abi.ctr_end_table(t, p.bc_len) + 5 * 51 + 4]) == n_pass
        return reads, p, exp
    return cached(("post", side, way), make)


# ---------------------------------------------------------------------------
# Q6: k_prepare's guess
# ---------------------------------------------------------------------------
GUESS_T = 12.25
GUESS_L = (64, 100, 101, 1000, 6400)
GUESS_SAMPLES = {"pass": [13] * 64, "fail": [12] * 64, "equal": [12] * 48 + [13] * 16}      # means of 13, 12 and 12.25


def sampled(L):
    """The 64 positions k_prepare's guess reads: 16 bytes at ((L - 16) * k) / 3 for k = 0 .. 3 (disjoint from L = 64 on)."""
    return np.concatenate([np.arange(16) + ((L - 16) * k) // 3 for k in range(4)])


def guess_case():
    def make():
        rng = np.random.default_rng(66)
        reads, what = [], []
        for L in GUESS_L:
            at = sampled(L)
            assert np.unique(at).size == 64 and at.max() < L
            for sample, values in GUESS_SAMPLES.items():
                for kind, total in zip(("below", "at", "above"), seam_sums(GUESS_T, L)):
                    if total is None:
                        continue
                    q = np.zeros(L, dtype=np.uint8)
                    q[at] = rng.permutation(values) + 33
                    rest = np.setdiff1d(np.arange(L), at)
                    if rest.size:
                        other = lay_out(rng, rest.size, total - sum(values))
                        q[rest] = np.frombuffer(other, dtype=np.uint8)
                    elif total != sum(values):
                        continue
                    guess = q[at].astype(np.float64).mean() - 33.0
                    assert (guess < GUESS_T, guess == GUESS_T, guess > GUESS_T) == (sample == "fail", sample == "equal", sample == "pass")
                    reads.append((b"guess_%s_read_%s_%d" % (sample.encode(), kind.encode(), L), bases(rng, L), q.tobytes()))
                    what.append((sample, kind, L, total))
        p = params(reads, GUESS_T, 255.0, min_len=POST_MIN_LEN, head_trim=3, tail_trim=2)
        r, f, ctr = exp = oracle(p, reads)
        fails = lowq(r)
        assert fails.tolist() == [kind == "below" for _, kind, _, _ in what]
        # the guess says pass and the read fails by 1 / L; the guess says fail, or sits on the threshold, and the read passes
        for sample, kind in (("pass", "below"), ("fail", "above"), ("fail", "at"), ("equal", "below"), ("equal", "at"), ("equal", "above")):
            assert sum(w[0] == sample and w[1] == kind for w in what) >= 3, (sample, kind)
        return reads, p, exp
    return cached(("guess",), make)


# ---------------------------------------------------------------------------
# Q7: nothing counted twice
# ---------------------------------------------------------------------------
REPLAY_ENV = {"TGSF_POOL_CAP": "3"}


def replay_case():
    """The seam reads of 12.25 and the histogram reads beside one read with eight middle adapters: with a candidate pool of
    three slots the batch's first run overflows and tgsf_wait runs it again."""
    def make():
        rng = np.random.default_rng(77)
        reads = list(gate_reads(12.25)[0]) + list(hist_case("filter")[0])
        ad, rc = MARGIN_ADS
        s = bytearray(bases(rng, 3400))
        for k in range(8):
            s[400 + 330 * k:400 + 330 * k + _Q] = rc if k & 1 else ad
        reads.insert(len(reads) // 2, (b"eight_adapters", bytes(s), bytes([33 + 40]) * len(s)))
        p = params(reads, 12.25, 255.0, adapters=MARGIN_ADS, min_len=POST_MIN_LEN, end_len=150, end_match_len=15, mid_match_len=35, extra_len=_T)
        r, f, ctr = exp = oracle(p, reads)
        i = [x[0] for x in reads].index(b"eight_adapters")
        assert r["flags"][i] & abi.RF_ADMID and r["n_frags"][i] == 9
        assert 10 <= ctr[abi.CTR_DROPINFO] == lowq(r).sum() < len(reads) - 10
        return reads, p, exp
    return cached(("replay",), make)


def replay_device(lib_path, monkeypatch):
    """The batch through tgsf_submit_device and tgsf_wait; returns what the fragment count said after the first run."""
    set_env(monkeypatch, REPLAY_ENV)
    reads, p, (exp_r, exp_f, exp_ctr) = replay_case()
    dev = refusals.Dev(lib_path)
    ctx = capi.Context(p, 0, lib_path)
    try:
        b = refusals.DeviceBatch(dev, p, ctx.n_bins, reads, frag_room=64)
        assert np.array_equal(b.exp_ctr, exp_ctr)
        assert b.submit(ctx) == abi.OK, refusals.last_error(ctx)
        dev.sync()
        first = int(dev.get(b.o_n, np.uint32)[0])
        ctx.wait()
        dev.sync()
        b.check()
        refusals.assert_tallies(ctx, exp_ctr, "after the replay")
        return first
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# E1: bc_len on the seams of k_end_tables' slots (64 positions) and slabs (512)
# ---------------------------------------------------------------------------
END_BC = (0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4096)
END_VARIANTS = ("qual", "no_qual", "trims")
END_TRIMS = (3, 2)
WIDEST = 1 << 20


def end_lengths(bc):
    return sorted({L for L in (1, bc - 1, bc, bc + 1, 2 * bc - 1, 2 * bc, 2 * bc + 1) if L >= 1})


def end_reads(bc, lengths=None, shift=(0, 0)):
    """Per length a plain read and a marked one: lower-case g and t on the first and the last position either table counts,
    a quality byte of 128 and above on position bc - 1 from either end (ordinary qualities of 90 and more beside it: the
    mean stays above 0).  shift: what fixed trims cut off in front and behind -- the marks then sit in the kept part."""
    rng = np.random.default_rng(8000 + bc % 9973)
    reads = []
    h, t = shift
    for L in lengths or end_lengths(bc):
        reads.append((b"plain%d" % L, bases(rng, L), (rng.integers(20, 60, L) + 33).astype(np.uint8).tobytes()))
        s, q = bytearray(bases(rng, L)), (rng.integers(90, 94, L) + 33).astype(np.uint8)
        K = L - h - t
        if K >= 1:
            last = min(bc, K) - 1
            for n, at in enumerate((h, L - 1 - t, h + last, L - 1 - t - last) if bc else ()):
                s[at] = b"gt"[n & 1] if s[at] not in b"gt" else s[at]
            if 0 <= bc - 1 < K and K >= 8:
                q[h + bc - 1] = 128 + int(rng.integers(0, 128))
                q[L - 1 - t - (bc - 1)] = 128 + int(rng.integers(0, 128))
        reads.append((b"marked%d" % L, bytes(s), q.tobytes()))
    return reads


def end_params(bc, variant, reads):
    h, t = END_TRIMS if variant == "trims" else (0, 0)
    return params(reads, 0.0, 255.0, bc_len=bc, no_qual=variant == "no_qual", head_trim=h, tail_trim=t)


def end_case(bc, variant):
    def make():
        shift = END_TRIMS if variant == "trims" else (0, 0)        # (under trims: the same lengths also for the kept parts)
        reads = end_reads(bc, sorted(set(end_lengths(bc)) | {L + sum(shift) for L in end_lengths(bc)}), shift)
        p = end_params(bc, variant, reads)
        r, f, ctr = exp = oracle(p, reads)
        L = np.array([len(x[1]) for x in reads])
        assert not lowq(r).any()
        # rows in use: the longest read's share of the table, not the table's length
        assert ctr[abi.CTR_ROWS + 2] == min(bc, L.max()) and (bc <= 1 or ctr[abi.CTR_ROWS + 2] < 2 * bc + 1)
        for t_cnt in (abi.T_RAW5P_CNT, abi.T_RAW3P_CNT):
            cnt = ctr[abi.ctr_end_table(t_cnt, bc):abi.ctr_end_table(t_cnt + 1, bc)].reshape(bc, 5)
            assert np.array_equal(cnt[:, 4], [(L > pos).sum() for pos in range(bc)]), (bc, variant)       # position pos: every read longer than it
        if bc:
            # a lower-case g at the 5' end and a lower-case t at the 3' end count as G and T with qualities and as neither without
            g5 = sum(x[1][0] in b"Gg" for x in reads) if variant != "no_qual" else sum(x[1][0] in b"G" for x in reads)
            t3 = sum(x[1][-1] in b"Tt" for x in reads) if variant != "no_qual" else sum(x[1][-1] in b"T" for x in reads)
            assert ctr[abi.ctr_end_table(abi.T_RAW5P_CNT, bc) + 2] == g5 and ctr[abi.ctr_end_table(abi.T_RAW3P_CNT, bc) + 1] == t3, (bc, variant)
            h, t = END_TRIMS if variant == "trims" else (0, 0)       # (under trims the marks are on the kept part's ends: the clean tables')
            assert any(x[1][h:h + 1] == b"g" for x in reads) and any(x[1][len(x[1]) - 1 - t:len(x[1]) - t] == b"t" for x in reads)
        if bc >= 63 and variant != "no_qual":
            assert any(max(x[2]) >= 128 for x in reads)
        return reads, p, exp
    return cached(("end", bc, variant), make)


def short_end_case():
    """bc_len 4096 over reads of at most 700 bases: the rows-in-use word is the longest read's length."""
    def make():
        reads = end_reads(4096, lengths=(1, 63, 64, 65, 511, 512, 513, 700))
        p = end_params(4096, "qual", reads)
        exp = oracle(p, reads)
        assert exp[2][abi.CTR_ROWS + 2] == 700 and exp[2][abi.CTR_ROWS + 3] == 700
        return reads, p, exp
    return cached(("short_end",), make)


def widest_case():
    """The largest bc_len tgsf_create accepts, 2^20 (2 048 slabs), with a read of 2^20 + 1 bases and one of 513."""
    def make():
        reads = end_reads(WIDEST, lengths=(513, WIDEST + 1))
        p = end_params(WIDEST, "qual", reads)
        exp = oracle(p, reads)
        assert exp[2][abi.CTR_ROWS + 2] == WIDEST and exp[2][abi.ctr_end_table(abi.T_RAW3P_CNT, WIDEST) + 5 * (WIDEST - 1) + 4] == 2
        return reads, p, exp
    return make()                                     # (not kept: the tallies are a third of a gigabyte)


def run_once(lib_path, case, monkeypatch):
    """One batch, once (the widest tables are a third of a gigabyte)."""
    reads, p, exp = case
    set_env(monkeypatch, {})
    ctx = capi.Context(p, 0, lib_path)
    try:
        parity.compare_batch(ctx, p, reads, align=16, expected=exp)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# the command line against the reference on the same seams (tests/test_cli_live.py, tests/golden/make_golden.py)
# ---------------------------------------------------------------------------
CLI_THRESHOLDS = {"7.5": "7.5", "9.9": "9.9f", "12.25": "12.25", "20.3": "20.3f"}


CLI_HEAD, CLI_TAIL, CLI_MIN_LEN = 10, 7, 100
# (the flag's value, which gate it sets, the read type): every value as -q and as -Q, under -x ont and -x hifi in turn
CLI_CORNERS = [(v, side, ("ont", "hifi")[(i + j) % 2]) for i, v in enumerate(CLI_THRESHOLDS) for j, side in enumerate(("min", "max"))]


def cli_designed(flag_value, side):
    """(FASTQ records, the pieces each is designed to be kept as under -5 10 -3 7 -l 100 if its raw mean passes: [(start, len)])
    for -q (side "min") or -Q (side "max") of 7.5, 9.9, 12.25 or 20.3: the raw gate's seam reads of that threshold from 100 bases
    on (the command line's least -l), reads whose part kept by the fixed trims, by an end adapter's clip (that part longer than
    the other end's window of 216 bases, which would find the same copy) and by a middle split lies on the seams of the same
    threshold, and -- first -- one read of quality 60 throughout, since the reference refuses a -q at or above the largest
    quality it sampled; with a -Q that read is dropped, which is as it should be."""
    t = THRESHOLDS[CLI_THRESHOLDS[flag_value]]
    rng = np.random.default_rng(9000 + int(t * 100) + (side == "max"))
    fill = bytes([(93 if side == "min" else 0) + 33])
    h, tl = CLI_HEAD, CLI_TAIL
    reads, pieces = [(b"high_quality", bases(rng, 400), bytes([33 + 60]) * 400)], [[(h, 400 - h - tl)]]
    for L in (100, 101, 104, 400, 12800):
        for kind, total in zip(("below", "at", "above"), seam_sums(t, L)):
            if total is not None:
                reads.append((b"raw_%s_%d" % (kind.encode(), L), bases(rng, L), lay_out(rng, L, total)))
                pieces.append([(h, L - h - tl)])
    ad = synth.ONT_RAPID
    for K in (100, 104, 300):
        for kind, total in zip(("below", "at", "above"), seam_sums(t, K)):
            if total is not None:
                reads.append((b"trim_%s_%d" % (kind.encode(), K), bases(rng, h + K + tl), fill * h + lay_out(rng, K, total) + fill * tl))
                pieces.append([(h, K)])
    for K in (300, 304, 700):
        for kind, total in zip(("below", "at", "above"), seam_sums(t, K)):
            if total is not None:
                reads.append((b"clip_%s_%d" % (kind.encode(), K), bases(rng, h) + ad + bases(rng, K + tl), fill * (h + len(ad)) + lay_out(rng, K, total) + fill * tl))
                pieces.append([(h + len(ad), K)])
    for k1, k2 in ((0, 2), (2, 0), (0, 0)):
        K1, K2 = 400, 404
        mid = 2 * _T + len(ad)
        s = bytearray(bases(rng, h + K1 + mid + K2 + tl))
        s[h + K1 + _T:h + K1 + _T + len(ad)] = ad
        q = fill * h + lay_out(rng, K1, seam_sums(t, K1)[k1]) + fill * mid + lay_out(rng, K2, seam_sums(t, K2)[k2]) + fill * tl
        reads.append((b"split_%d_%d" % (k1, k2), bytes(s), q))
        pieces.append([(h, K1), (h + K1 + mid, K2)])
    return reads, pieces


def cli_reads(flag_value, side):
    return cli_designed(flag_value, side)[0]


def cli_case(flag_value, side, kind):
    """The reads of a command-line corner, asserted on the oracle under the parameters the command line resolves the flags
    `-x kind -l 100 -5 10 -3 7 -q / -Q value -a ONT_RAPID` to: every read is kept as the pieces it is designed for, and the
    reads and pieces the gate drops -- before the split and after it -- are those the numpy restatement drops."""
    def make():
        reads, pieces = cli_designed(flag_value, side)
        v = float(flag_value)
        p = params(reads, v if side == "min" else 0.0, 255.0 if side == "min" else v, adapters=[synth.ONT_RAPID, synth.ONT_RAPID_RC],
                   min_len=CLI_MIN_LEN, head_trim=CLI_HEAD, tail_trim=CLI_TAIL)
        p.end_sim, p.mid_sim = {"ont": (0.75, 0.9), "hifi": (0.9, 0.95)}[kind]
        r, f, ctr = oracle(p, reads)
        n_raw = n_post = clipped = split = 0
        for i, ((name, _, q), want) in enumerate(zip(reads, pieces)):
            value = np.frombuffer(q, dtype=np.uint8).astype(np.int64) - 33
            got = [(int(x["start"]), int(x["len"]), int(x["sum_q"]), bool(x["flags"] & abi.FF_PASS)) for x in f[r["frag_begin"][i]:r["frag_begin"][i] + r["n_frags"][i]]]
            if gate_fails(int(value.sum()), len(q), p.min_q, p.max_q):
                assert lowq(r)[i] and not got, (flag_value, side, kind, name)
                n_raw += 1
                continue
            exp = [(s, n, int(value[s:s + n].sum())) for s, n in want if n >= CLI_MIN_LEN]
            exp = [(s, n, total, not gate_fails(total, n, p.min_q, p.max_q)) for s, n, total in exp]
            assert not lowq(r)[i] and got == exp, (flag_value, side, kind, name, got, exp)
            n_post += sum(not x[3] for x in exp)
            clipped += name.startswith(b"clip_") and bool(r["flags"][i] & abi.RF_AD5P) and not r["flags"][i] & (abi.RF_AD3P | abi.RF_ADMID)
            split += name.startswith(b"split_") and len(got) == 2
        assert (ctr[abi.CTR_DROPINFO], ctr[abi.CTR_DROPINFO + 13]) == (n_raw, n_post), (flag_value, side, kind, n_raw, n_post)
        assert n_raw >= 5 and n_post >= 8 and clipped >= 6 and split == 3, (flag_value, side, kind, n_raw, n_post, clipped, split)
        return reads
    return cached(("cli", flag_value, side, kind), make)
