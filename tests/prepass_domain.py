"""The pre-pass across its domain (tgsfilter_amd/host/prepass.cpp, the pre-pass part of host/run_contexts.cpp): what the filter is
configured with before the first batch -- the quality encoding and the automatic -q, the automatic -5 / -3 trims, and which of
the 22 library adapters the run trims.  tests/test_prepass_emul.py runs everything here on the emulation build,
tests/test_prepass_gpu.py a part of it on the HIP build.

1. tgsf_align_windows AS THE PRE-PASS CALLS IT against edlib (tests/parity.py, edlib_truth): all 22 library entries against the
   same window, read-major, k = int((1 - min_sim) * Q) + 1 in float32, on a context made with adapter_search's own parameters.
2. A model of the identification (adapterSearch, reference :1148-1209, and the 5x rule of host/run_contexts.cpp) on top of
   that truth; every case is asserted to do what it is built for ON THE MODEL, the model is asserted against the reference's
   own INFO lines, and only then is the command line compared with the reference binary (tests/cli_check.py, compare_live).
3. Get_qType (reference :1042-1077) and 4. CheckBaseContent (reference :1079-1146) the same way, from restatements here.

Every comparison is exact: integers, bytes and printed lines."""
from __future__ import annotations

import functools
import gzip
import json
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import cli_check, parity
from tgsfilter_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "tgsfilter_ref")
EMUL_CLI = os.path.join(ROOT, "tests", "emul", "tgsfilter_emul")
GPU_CLI = os.path.join(ROOT, "tgsfilter_amd", "bin", "tgsfilter")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def adapter_lib():
    """kAdapterLib as host/prepass.cpp holds it: there is no second copy of the table."""
    text = open(os.path.join(ROOT, "tgsfilter_amd", "host", "prepass.cpp")).read()
    m = re.search(r"kAdapterLib\[22\]\s*=\s*\{(.*?)\};", text, flags=re.S)
    lib = [s.encode() for s in re.findall(r'"([ACGT]+)"', m.group(1))]
    assert len(lib) == 22
    return lib


LIB = adapter_lib()
SIMS = (0.9, 0.93, 0.95, 0.99, 1.0)
WINDOW_LENS = (100, 101, 140, 257)       # the check lengths -E / -e can make: the least, one more, below -e's default, past 256
PER_CALL = 4096                          # read ends per library call (host/prepass.cpp, adapter_search)
# siblings: an entry inside another one (4 > 7, 5 > 6), inside it but for one base (13 > 10, 12 > 11), and the 14 .. 19 family
# that shares its core with 4 .. 7
SIBLINGS = [(4, 7), (5, 6), (13, 10), (12, 11)] + [(a, b) for a in range(14, 20) for b in range(4, 8)]


def k_of(min_sim):
    """k[a] = (int)((1 - min_sim) * Q) + 1 with min_sim a float and Q an int: float32 all the way (:1161)."""
    ms = np.float32(min_sim)
    return [int(np.float32(np.float32(1) - ms) * np.float32(len(a))) + 1 for a in LIB]


def context_params():
    """EXACTLY what adapter_search (host/prepass.cpp) creates its context with: the two places must move together."""
    return abi.make_params("ont", adapters=LIB, min_len=100, max_len=2147483647, min_q=0, max_q=255, bc_len=0, head_trim=0, tail_trim=0,
                           end_len=0, extra_len=0, end_sim=0.75, mid_sim=0.9, discard=False, filter=True, only_qc=False, qtype=33,
                           min_repeat=0, kmer=0, end_match_len=2, mid_match_len=64,
                           max_batch_reads=PER_CALL * 22 // (22 * 2) + 64, max_batch_bases=1 << 20, max_read_len=1 << 16)


# ---- truth ----------------------------------------------------------------------------------------------------------------------
_TRUTH = {}


@functools.lru_cache(maxsize=None)
def _edlib():
    return parity.edlib_truth()


def truth(a, t, k):
    """(distance, locations, alignment length, first start, first end, last end) of library entry a in window t within k."""
    key = (a, t, k)
    r = _TRUTH.get(key)
    if r is None:
        r = _TRUTH[key] = _edlib()(LIB[a], t, k)
    return r


# ---- part 1: windows ------------------------------------------------------------------------------------------------------------
_OTHER = {65: 67, 67: 65, 71: 84, 84: 71}


def edited(rng, q, e, kind):
    """q with e substitutions, inserted bases or deleted bases, away from its first and last two bases."""
    q = bytearray(q)
    for x in sorted((int(v) for v in rng.choice(np.arange(2, len(q) - 2), size=e, replace=False)), reverse=True):
        if kind == "sub":
            q[x] = _OTHER[q[x]]
        elif kind == "ins":
            q[x:x] = bytes([_OTHER[q[x]]])
        else:
            del q[x]
    return bytes(q)


def placed(rng, m, T, how):
    bg = bytearray(_ACGT[rng.integers(0, 4, T)].tobytes())
    if how == "first":
        bg[:len(m)] = m
    elif how == "middle":
        at = (T - len(m)) // 2
        bg[at:at + len(m)] = m
    elif how == "last":
        bg[T - len(m):] = m
    elif how == "over_start":
        bg[:len(m) - 2] = m[2:]
    else:
        bg[T - (len(m) - 2):] = m[:-2]
    assert len(bg) == T
    return bytes(bg)


PLACES = ("first", "middle", "last", "over_start", "over_end")
UNITS = (b"A", b"T", b"C", b"G", b"CT", b"TC", b"AG", b"GA", b"GGA", b"TCC", b"GTT", b"AAC", b"N", b"a")


@functools.lru_cache(maxsize=None)
def windows():
    """[(window, the entry planted in it or -1, the number of edits of the copy)]"""
    rng = np.random.default_rng(2201)
    k0 = k_of(0.9)
    out, i = [], 0
    for a, q in enumerate(LIB):
        for e in range(k0[a] + 3):
            for kind in ("sub", "ins", "del"):
                if e == 0 and kind != "sub":
                    continue
                for how in PLACES:
                    out.append((placed(rng, edited(rng, q, e, kind), WINDOW_LENS[i % 4], how), a, e))
                    i += 1
    for unit in UNITS:
        foreign = next(bytes([c]) for c in b"ACGT" if bytes([c]) not in unit.upper())
        for T in WINDOW_LENS:
            t = (unit * T)[:T]
            out.append((t, -1, 0))
            out.append((t[:T // 2] + foreign + t[T // 2 + 1:], -1, 0))
    for a, q in enumerate(LIB):
        for T in WINDOW_LENS:
            out.append(((q * (T // len(q) + 1))[:T], -1, 0))                           # a tandem that fills the window
        out.append((placed(rng, q.lower(), WINDOW_LENS[a % 4], "middle"), -1, 0))      # edlib matches bytes: not found
        out.append((placed(rng, rev_comp(q), WINDOW_LENS[(a + 1) % 4], "middle"), -1, 0))
    for a, b in SIBLINGS:
        t = bytearray(_ACGT[rng.integers(0, 4, 257)].tobytes())
        t[10:10 + len(LIB[a])] = LIB[a]
        t[130:130 + len(LIB[b])] = LIB[b]
        out.append((bytes(t), -1, 0))
    return out


def lower_case_windows():
    return [(a, w[0]) for a in range(22) for w in windows() if LIB[a].lower() in w[0]]


def expected(wins, ks):
    """The truth of every window against all 22 entries, read-major: an (n * 22, 6) array."""
    return np.array([truth(a, t, ks[a]) for t in wins for a in range(22)], dtype=np.int32)


def align_call(ctx, wins, ks):
    """One tgsf_align_windows call laid out as adapter_search lays it out: the 22 problems of a window share win_off."""
    n = len(wins)
    ln = np.array([len(t) for t in wins], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    res, ends = ctx.align_windows(b"".join(wins), np.repeat(off, 22), np.repeat(ln, 22).astype(np.uint32),
                                  np.tile(np.arange(22, dtype=np.uint8), n), np.tile(np.array(ks, dtype=np.int32), n))
    return np.concatenate([res, ends], axis=1)


def assert_equal_words(got, exp, wins, ks):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%d of %d alignments differ, first: entry %d, k %d, window %r: got %s, edlib %s"
                             % (bad.size, len(exp), i % 22, ks[i % 22], wins[i // 22], got[i].tolist(), exp[i].tolist()))


def check_windows(lib_path, min_sim):
    """All windows against all 22 entries at the k of min_sim, all six words per problem."""
    ks = k_of(min_sim)
    wins = [w[0] for w in windows()]
    exp = expected(wins, ks)
    ctx = capi.Context(context_params(), 0, lib_path)
    try:
        for b in range(0, len(wins), PER_CALL):
            part = wins[b:b + PER_CALL]
            assert_equal_words(align_call(ctx, part, ks), exp[b * 22:(b + len(part)) * 22], part, ks)
    finally:
        ctx.close()
    return len(exp)


def check_product_sized_call(lib_path):
    """4 096 windows x 22 = 90 112 problems in ONE call: the command line's per_call, the most the context is sized for."""
    ks = k_of(0.9)
    ws = [w[0] for w in windows()]
    wins = [ws[i % len(ws)] for i in range(PER_CALL)]
    exp = expected(wins, ks)
    assert len(exp) == 90112
    ctx = capi.Context(context_params(), 0, lib_path)
    try:
        assert_equal_words(align_call(ctx, wins, ks), exp, wins, ks)
    finally:
        ctx.close()


def check_conditions():
    """Conditions on the case list, on the truth alone: what part 1 claims to reach, it reaches."""
    ws = windows()
    several = set()
    at_start = set()
    at_end = set()
    odd_len = 0
    for sim in SIMS:
        ks = k_of(sim)
        on_k, past_k = set(), set()
        for t, planted, _ in ws:
            for a in range(22):
                d, n, alen, s0, e0, _e1 = truth(a, t, ks[a])
                if n > 0 and d == ks[a]:
                    on_k.add(a)
                if sim == SIMS[0] and n > 0:
                    if n > 1:
                        several.add(a)
                    if s0 == 0:
                        at_start.add(a)
                    if e0 == len(t) - 1:
                        at_end.add(a)
                    odd_len += alen != len(LIB[a])
                if n == 0 and a == planted and truth(a, t, ks[a] + 1)[1] > 0:
                    past_k.add(a)
        assert on_k == set(range(22)), (sim, "no window at distance k for", sorted(set(range(22)) - on_k))
        assert past_k == set(range(22)), (sim, "no window found at k + 1 only for", sorted(set(range(22)) - past_k))
    assert several == set(range(22)) and at_start == set(range(22)) and at_end == set(range(22)), (several, at_start, at_end)
    assert odd_len >= 200, odd_len
    ks = k_of(0.9)
    for a, t in lower_case_windows():
        assert truth(a, t, ks[a])[1] == 0


# ---- part 2: the model ----------------------------------------------------------------------------------------------------------
_COMP = bytearray(b"N" * 256)
for _a, _b in zip(b"AGCTagctMRWSYKmrwsyk", b"TCGAtcgaKYWSRMkywsrm"):
    _COMP[_a] = _b
_COMP = bytes(_COMP)


def rev_comp(s):
    return bytes(s).translate(_COMP)[::-1]


class Opts:
    """The flags the pre-pass looks at, with the command line's defaults."""
    def __init__(self, x="ont", l=100, E=150, e=150, N=100000, n=100000, S=None, b=None, q=None, trim5="0", trim3="0", only_adapters=True):
        self.x, self.l, self.E, self.e, self.N, self.n, self.S, self.b, self.q = x, l, E, e, N, n, S, b, q
        self.trim5, self.trim3, self.only_adapters = trim5, trim3, only_adapters

    def flags(self):
        f = ["-x", self.x, "-l", str(self.l)]
        for name, v, default in (("-E", self.E, 150), ("-e", self.e, 150), ("-N", self.N, 100000), ("-n", self.n, 100000),
                                 ("-S", self.S, None), ("-b", self.b, None), ("-q", self.q, None), ("-5", self.trim5, None), ("-3", self.trim3, None)):
            if v != default:
                f += [name, str(v)]
        return f + (["-A"] if self.only_adapters else [])

    @property
    def check_len(self):
        return max(self.E, self.e, 100)

    @property
    def min_sim(self):
        return np.float32(0.95 if self.x == "hifi" else 0.9) if self.S is None else np.float32(max(float(self.S), 0.8))


def sampled(reads, o):
    """The reads the pre-pass looks at: L >= max(-l, 2 * check_len), the first max(-N, -n) of them."""
    min_len, cap = max(max(o.l, 100), 2 * o.check_len), max(o.N, o.n)
    return [r for r in reads if len(r[1]) >= min_len][:cap]


def read_ends(reads, o):
    c = o.check_len
    sm = sampled(reads, o)
    return [bytes(r[1][:c]) for r in sm], [rev_comp(r[1][len(r[1]) - c:]) for r in sm]


def clamped_sim(S):
    """-S below 0.9 counts as 0.9 in the identification (:1151-1154): the float against the double 0.9."""
    ms = np.float32(S)
    return np.float32(0.9) if float(ms) < 0.9 else ms


def search(ends, min_sim):
    """adapterSearch over one side: (entry or -1, its total, depth as float32; 0 where the winner is not accepted)."""
    ms = clamped_sim(min_sim)
    ks = k_of(ms)
    totals, found = [0] * 22, [False] * 22
    for t in ends:
        for a in range(22):
            d, n, alen = truth(a, t, ks[a])[:3]
            if n > 0:
                totals[a] += alen - d
                found[a] = True
    if not any(found):
        return -1, 0, np.float32(0)
    best = max(totals[a] for a in range(22) if found[a])
    winners = [a for a in range(22) if found[a] and totals[a] == best]
    assert len(winners) == 1, "an exact tie between entries %s at %d: it falls by the container's order (DESIGN 7)" % (winners, best)
    a = winners[0]
    depth = np.float32(best) / np.float32(len(LIB[a]))
    if depth >= np.float32(2) * ms:
        return a, best, depth
    return -1, best, np.float32(0)


def identify(reads, o):
    """What the run prints: (5' adapter, 3' adapter, 5' depth, 3' depth) after the 5x rule; and the two totals."""
    e5, e3 = read_ends(reads, o)
    a5, t5, d5 = search(e5, o.min_sim)
    a3, t3, d3 = search(e3, o.min_sim)
    if d5 > np.float32(5) * d3:
        a3, d3 = -1, np.float32(0)
    elif d3 > np.float32(5) * d5:
        a5, d5 = -1, np.float32(0)
    return (a5, a3, d5, d3), (t5, t3)


def adapter_lines(model):
    a5, a3, d5, d3 = model
    return ["INFO: 5' adapter: " + (LIB[a5].decode() if a5 >= 0 else ""), "INFO: 3' adapter: " + (LIB[a3].decode() if a3 >= 0 else ""),
            "INFO: mean depth of 5' adapter: %g" % float(d5), "INFO: mean depth of 3' adapter: %g" % float(d3)]


def lines_with(err, *starts):
    return [l for l in err.splitlines() if l.startswith(starts)]


# ---- reads ----------------------------------------------------------------------------------------------------------------------
def plain_reads(seed, n=30, L=400, prefix=b"r"):
    """Random reads with Phred+33 qualities of 2 .. 30 (both reached in the first read's first bases: the encoding reads as 33)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        q = bytearray((rng.integers(2, 31, L) + 33).astype(np.uint8).tobytes())
        if i == 0:
            q[0], q[1] = 35, 63
        out.append([prefix + b"%d" % i, bytearray(_ACGT[rng.integers(0, 4, L)].tobytes()), bytes(q)])
    return out


def plant(read, m, end, off=5):
    s = read[1]
    if end == 5:
        s[off:off + len(m)] = m
    else:
        s[len(s) - off - len(m):len(s) - off] = m


def done(reads):
    return [(bytes(n), bytes(s), bytes(q)) for n, s, q in reads]


class Case:
    def __init__(self, reads, opts, in_fmt="fq", want=None):
        self.reads, self.opts, self.in_fmt = done(reads), opts, in_fmt
        self.model, self.totals = identify(self.reads, opts)
        if want is not None:                   # what the case is built for, on the model
            want(self)

    def names(self, a5, a3):
        assert self.model[:2] == (a5, a3), (self.model, a5, a3)

    def among(self, ok5, ok3):
        assert self.model[0] in ok5 and self.model[1] in ok3, (self.model, ok5, ok3)


CARRIERS = {1: (4,), 2: (4, 17), 3: (0, 13, 29), 11: tuple(range(1, 30, 2))[:11]}
# the entries that hold entry a, or all of it but its first or last base: copies of a count for them too, with whatever of
# their own bases the read happens to hold beside the copy -- and the winner is the largest TOTAL, not the largest depth
SUPERS = {a: [b for b in range(22) if b != a and LIB[a][1:-1] in LIB[b]] for a in range(22)}
assert SUPERS[10] == [13] and SUPERS[11] == [12] and SUPERS[7] == [4, 14, 17] and SUPERS[6] == [5, 15, 16]


def family(a, or_none=False):
    """What planted copies of a may be identified as: a or an entry that holds it; with no more than two copies also nothing at all
    (an entry that holds it can win the total and still miss the depth)."""
    return {a, *SUPERS[a]} | ({-1} if or_none and SUPERS[a] else set())


@functools.lru_cache(maxsize=None)
def five_case(a, copies):
    reads = plain_reads(1000 + a)
    for i in CARRIERS[copies]:
        plant(reads[i], LIB[a], 5)
    ok = {-1} if copies == 1 else family(a, or_none=copies == 2)
    return Case(reads, Opts(), want=lambda c: c.among(ok, {-1}))


@functools.lru_cache(maxsize=None)
def three_case(a):
    """Entry a at the 3' end: the 3' end is read as its reverse complement, the winner is a's partner."""
    reads = plain_reads(1100 + a)
    for i in CARRIERS[3]:
        plant(reads[i], LIB[a], 3)
    assert rev_comp(LIB[a]) == LIB[a ^ 1]
    return Case(reads, Opts(), want=lambda c: c.among({-1}, family(a ^ 1)))


@functools.lru_cache(maxsize=None)
def both_case(a):
    b = (a + 7) % 22
    reads = plain_reads(1200 + a)
    for i in CARRIERS[3]:
        plant(reads[i], LIB[a], 5)
        plant(reads[i], LIB[b], 3)
    return Case(reads, Opts(), want=lambda c: c.among(family(a), family(b ^ 1)))


# what the reference answers where an entry's sibling is in the library: (planted at the 5' end in two reads) -> (winner, depth)
SIBLING_PINS = {10: (13, "1.89062"), 11: (12, "1.875"), 12: (12, "2"), 13: (13, "2"),      # 13 holds 10 but for its last base, 12 holds 11 likewise
                4: (4, "2"), 5: (5, "2"), 7: (7, "2"), 6: (-1, "0"),          # 6: entry 16 holds it and wins the total with 47, a depth of 1.74
                14: (14, "2"), 15: (15, "2"), 16: (16, "2"), 17: (17, "2"), 18: (16, "1.81481"), 19: (19, "2")}


@functools.lru_cache(maxsize=None)
def sibling_case(a):
    reads = plain_reads(1300 + a)
    for i in CARRIERS[2]:
        plant(reads[i], LIB[a], 5)
    w, depth = SIBLING_PINS[a]

    def want(c):
        c.names(w, -1)
        assert "%g" % float(c.model[2]) == depth, c.model
    return Case(reads, Opts(), want=want)


DEPTH_ENTRIES = (18, 20, 8, 12)          # 22, 45, 50 and 64 bp
DEPTH_SIMS = (0.8, 0.9, 0.95)


def seam_total(Q, min_sim):
    """The smallest total T with float32(T) / float32(Q) >= 2 * min_sim in float32."""
    ms = clamped_sim(min_sim)
    T = 0
    while not np.float32(T) / np.float32(Q) >= np.float32(2) * ms:
        T += 1
    return T


def copies_for(a, total, k, seed):
    """Two copies of entry a with substitutions within k that add up to `total` matched bases."""
    Q = len(LIB[a])
    deficit = 2 * Q - total
    e1 = min(k, (deficit + 1) // 2)
    e2 = deficit - e1
    assert 0 <= e2 <= k and 0 <= e1, (a, total, k)
    rng = np.random.default_rng(seed)
    return [edited(rng, LIB[a], e1, "sub"), edited(rng, LIB[a], e2, "sub")]


@functools.lru_cache(maxsize=None)
def depth_case(a, S, below):
    assert len(LIB[a]) in (22, 45, 50, 64)
    o = Opts(S=S)
    T = seam_total(len(LIB[a]), S) - (1 if below else 0)
    # (where the substitutions fall decides what else edlib can make of the copy: the first placing that gives T is taken)
    for seed in range(20):
        reads = plain_reads(1400 + a)
        for i, m in zip(CARRIERS[2], copies_for(a, T, k_of(clamped_sim(S))[a], 100 * T + seed)):
            plant(reads[i], m, 5)
        try:
            if search(read_ends(done(reads), o)[0], o.min_sim)[1] == T:
                break
        except AssertionError:
            pass

    def want(c):
        assert c.totals[0] == T, (c.totals, T)
        c.names(-1 if below else a, -1)
    return Case(reads, o, want=want)


@functools.lru_cache(maxsize=None)
def five_times_case(strong, mirrored):
    """d = 2 on one side against `strong` (10: kept, 11: the weak side is dropped) on the other."""
    reads = plain_reads(1500 + strong)
    big, small = (3, 5) if mirrored else (5, 3)
    for i in range(strong):
        plant(reads[2 * i], LIB[8] if big == 5 else LIB[9], big)
    for i in (25, 27):
        plant(reads[i], LIB[20] if small == 5 else LIB[21], small)

    def want(c):
        e5, e3 = read_ends(c.reads, c.opts)
        d = {5: search(e5, 0.9)[2], 3: search(e3, 0.9)[2]}
        assert float(d[big]) == strong and float(d[small]) == 2.0, d
        weak = 20 if strong == 10 else -1
        c.names(*((8, weak) if big == 5 else (weak, 8)))
    return Case(reads, Opts(), want=want)


def _sampling(name):
    """Which reads, and how much of them, the identification looks at: two carriers of entry 8 that are seen, or are not."""
    o, carriers, L, L_others, off, named = Opts(), (4, 17), 400, 400, 5, True
    if name in ("len299", "len300"):     # 2 * check_len - 1 and 2 * check_len bases
        L, named = int(name[3:]), name == "len300"
    elif name in ("l500", "l100"):       # -l above and below 2 * check_len
        o, L_others, named = Opts(l=int(name[1:])), 600, name == "l100"
    elif name in ("E100", "E200"):       # the adapter at offset 110: beyond a check length of 100, within one of 200
        o, off, named = Opts(e=100, E=int(name[1:])), 110, name == "E200"
    elif name == "N10":                  # -N alone caps nothing: the cap is max(-N, -n) and -n stays 100 000
        o, carriers = Opts(N=10), (9, 10)
    elif name == "n10N5_9_10":
        o, carriers, named = Opts(n=10, N=5), (9, 10), False
    elif name == "n10N5_8_9":
        o, carriers = Opts(n=10, N=5), (8, 9)
    reads = plain_reads(1600, L=L_others)
    for i in carriers:
        reads[i] = plain_reads(1601 + i, n=1, L=L, prefix=b"c%d_" % i)[0]
        plant(reads[i], LIB[8], 5, off)
    return Case(reads, o, want=lambda c: c.names(8 if named else -1, -1))


SAMPLING = ("len299", "len300", "l500", "l100", "E100", "E200", "N10", "n10N5_9_10", "n10N5_8_9")
sampling_case = functools.lru_cache(maxsize=None)(_sampling)
CALL_SEAMS = ((4094, 4095), (4095, 4096), (4096, 4097), (8191, 8192))


@functools.lru_cache(maxsize=None)
def call_seam_case(i, j):
    """8 200 reads of 200 bases, two carriers of entry 10 on the two sides of a 4 096-ends call: 16 different reads over and
    over (what the model aligns once, and what keeps a committed copy of the input small), the carriers apart."""
    base = plain_reads(1700, n=16, L=200)
    reads = [[b"s%d" % r, base[r % 16][1], base[r % 16][2]] for r in range(8200)]
    for r in (i, j):
        reads[r] = [b"s%d" % r, bytearray(base[r % 16][1]), base[r % 16][2]]
        plant(reads[r], LIB[10], 5)
    return Case(reads, Opts(e=100, E=100, N=9000), want=lambda c: c.names(13, -1))


def _bytes_case(name):
    reads = plain_reads(1800)
    if name == "lower":                  # lower-case copies are not found: edlib matches bytes
        for i in CARRIERS[3]:
            plant(reads[i], LIB[8].lower(), 5)
        return Case(reads, Opts(), want=lambda c: c.names(-1, -1))
    if name == "with_N":                 # an N is one difference
        m = bytearray(LIB[8])
        m[20] = ord("N")
        for i in CARRIERS[3]:
            plant(reads[i], bytes(m), 5)

        def want(c):
            c.names(8, -1)
            assert c.totals[0] == 3 * 49
        return Case(reads, Opts(), want=want)
    # IUPAC letters and other bytes in the 3' end: complemented through the 20-letter table, every other byte becomes N
    m = bytearray(LIB[9])
    for x, ch in zip((7, 19, 31, 43), b"MRyk"):
        m[x] = ch
    for i in CARRIERS[3]:
        plant(reads[i], bytes(m), 3)
        reads[i][1][-3:] = b"SWx"
        reads[i][1][-120:-114] = b"u-.*Bd"

    def want(c):
        c.names(-1, 8)
        assert c.totals[1] == 3 * 46
        assert read_ends(c.reads, c.opts)[1][CARRIERS[3][0]][:3] == b"NWS"
    return Case(reads, Opts(), want=want)


BYTES = ("lower", "with_N", "iupac3")
bytes_case = functools.lru_cache(maxsize=None)(_bytes_case)
FORMATS = ("fa", "fq.gz", "sam", "bam")


@functools.lru_cache(maxsize=None)
def format_case(fmt):
    reads = plain_reads(1900)
    for i in CARRIERS[3]:
        plant(reads[i], LIB[8], 5)
        plant(reads[i], LIB[21], 3)
    return Case(reads, Opts(), in_fmt=fmt, want=lambda c: c.names(8, 20))


@functools.lru_cache(maxsize=None)
def fallback_case(x):
    """No adapter in the reads and none by -a: the run trims entries 8 / 9 (ont) or 0 / 1 (hifi, clr), and says so."""
    return Case(plain_reads(2000), Opts(x=x, q=7, only_adapters=False), want=lambda c: c.names(-1, -1))


def adapter_check(case):
    """The model's adapters and depths are the reference's own four lines (a case whose reads were never sampled fails here)."""
    def check(rc, err):
        assert rc == 0, err
        assert lines_with(err, "INFO: 5' adapter", "INFO: 3' adapter", "INFO: mean depth") == adapter_lines(case.model), (err, case.model)
    return check


def live(binary, case, ref_check, refused=False):
    """The command line against the reference binary on the case's input; returns what compare_live returns."""
    got = cli_check.compare_live(binary, REF, case.reads, case.opts.flags(), None, in_fmt=case.in_fmt, ref_check=ref_check)
    assert (got == "both failed") == refused, got
    return got


# ---- part 3: the quality encoding and the automatic -q -------------------------------------------------------------------------
def q_type(lo, hi):
    if 33 <= lo <= 78 and 33 <= hi <= 127:
        return 33
    if 64 <= lo <= 108 and 64 <= hi <= 127:
        return 64
    return 33 if lo < 55 else 64


def q_branch(lo, hi):
    return 1 if 33 <= lo <= 78 and 33 <= hi <= 127 else 2 if 64 <= lo <= 108 and 64 <= hi <= 127 else 3


def quality_seen(reads, o):
    """The smallest and the largest quality byte among the first check_len qualities of the sampled reads."""
    qs = b"".join(r[2][:o.check_len] for r in sampled(reads, o))
    return min(qs), max(qs)


def auto_q(maxq, x):
    return 10 if maxq > 10 and x in ("clr", "ont") else 20 if maxq > 20 and x == "hifi" else 0


def quality_reads(seed, lo, hi, n=30, L=400):
    """Random reads whose qualities are drawn from lo + 1 .. hi, with lo and hi themselves in the first read's first bases."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        q = bytearray(rng.integers(lo + 1, hi + 1, L).astype(np.uint8).tobytes())
        if i == 0:
            q[0], q[1] = lo, hi
        out.append([b"q%d" % i, bytearray(_ACGT[rng.integers(0, 4, L)].tobytes()), q])
    return out


class QualityCase:
    def __init__(self, reads, opts, in_fmt="fq", qtype=None, branch=None, min_q=None):
        self.reads, self.opts, self.in_fmt = done(reads), opts, in_fmt
        lo, hi = quality_seen(self.reads, opts)
        self.qtype, self.maxq = q_type(lo, hi), hi - q_type(lo, hi)
        self.min_q = auto_q(self.maxq, opts.x) if opts.q is None else opts.q
        if qtype is not None:
            assert self.qtype == qtype, (lo, hi, self.qtype)
        if branch is not None:
            assert q_branch(lo, hi) == branch, (lo, hi)
        if min_q is not None:
            assert self.min_q == min_q


ENCODING_LOW = ((32, 33, 3), (33, 33, 1), (54, 33, 1), (55, 33, 1), (78, 33, 1), (79, 64, 2), (108, 64, 2), (109, 64, 3))


@functools.lru_cache(maxsize=None)
def encoding_case(lo):
    qtype, branch = next((t, b) for l, t, b in ENCODING_LOW if l == lo)
    return QualityCase(quality_reads(2100 + lo, lo, 126), Opts(), qtype=qtype, branch=branch)


ODD_PLACES = (("inside", 33), ("past_check_len", 64), ("short_read", 64), ("after_cap", 64))


@functools.lru_cache(maxsize=None)
def odd_byte_case(place):
    """Qualities of 80 .. 126 read as Phred+64; one byte of 50 makes them Phred+33 -- where the pre-pass looks at it."""
    reads = quality_reads(2200, 80, 126)
    o = Opts()
    qtype = dict(ODD_PLACES)[place]
    if place == "inside":
        reads[7][2][o.check_len - 1] = 50
    elif place == "past_check_len":
        reads[7][2][o.check_len] = 50
    elif place == "short_read":
        reads[0] = [reads[0][0], reads[0][1][:2 * o.check_len - 1], reads[0][2][:2 * o.check_len - 1]]
        reads[0][2][3] = 50
        reads[1][2][0], reads[1][2][1] = 80, 126
    else:
        o = Opts(n=10, N=5)
        reads[10][2][0] = 50
    return QualityCase(reads, o, qtype=qtype)


AUTO_Q = (("ont", 10, 0), ("ont", 11, 10), ("clr", 10, 0), ("clr", 11, 10), ("hifi", 20, 0), ("hifi", 21, 20))


@functools.lru_cache(maxsize=None)
def auto_q_case(x, maxq):
    want = next(w for xx, m, w in AUTO_Q if (xx, m) == (x, maxq))
    c = QualityCase(quality_reads(2300 + maxq, 35, 33 + maxq), Opts(x=x), qtype=33, min_q=want)
    assert c.maxq == maxq
    return c


@functools.lru_cache(maxsize=None)
def fixed_q_case(q):
    """-q at the largest quality seen (30): refused; one below it: runs."""
    c = QualityCase(plain_reads(2400), Opts(q=q), qtype=33)
    assert c.maxq == 30
    return c


def quality_check(case, fasta=False, refused=False):
    def check(rc, err):
        enc = lines_with(err, "INFO: base quality scoring")
        if fasta:
            assert rc == 0 and enc == [] and lines_with(err, "INFO: min Phred average") == [], err
            return
        assert enc == ["INFO: base quality scoring: Phred%d" % case.qtype], (err, case.qtype)
        if refused:
            assert rc != 0 and lines_with(err, "Warning: max base quality") == ["Warning: max base quality score was: %d" % case.maxq], err
        else:
            assert rc == 0 and lines_with(err, "INFO: min Phred average") == ["INFO: min Phred average quality score: %d" % case.min_q], err
    return check


# ---- part 4: the automatic trims ------------------------------------------------------------------------------------------------
def base_content(ends, check_len, seq_num, bias):
    """CheckBaseContent: the last column that differs from one of its five neighbours on EITHER side by more than max_diff, + 1."""
    col = {65: 0, 97: 0, 84: 1, 116: 1, 71: 2, 103: 2, 67: 3, 99: 3}
    cnt = np.zeros((check_len, 4), dtype=np.int64)
    for s in ends:
        for i, c in enumerate(s[:check_len]):
            if c in col:
                cnt[i, col[c]] += 1
    max_diff = int(np.float32(seq_num) * np.float32(bias) / np.float32(100))
    trim = 0
    for i in range(1, check_len - 1):
        left = any(abs(cnt[i] - cnt[i - x]).max() > max_diff for x in range(1, min(i, 5) + 1))
        right = any(abs(cnt[i + x] - cnt[i]).max() > max_diff for x in range(1, min(check_len - i - 1, 5) + 1))
        if left and right:
            trim = i + 1
    return trim


def auto_trims(reads, o):
    """(trim 5', trim 3') as printed: an automatic 5' trim is clamped to -e where the 3' trim is automatic too."""
    e5, e3 = read_ends(reads, o)
    n, bias = len(e5), 1.0 if o.b is None else o.b
    t5 = base_content(e5, o.check_len, n, bias) if o.trim5 is None else int(o.trim5)
    t3 = base_content(e3, o.check_len, n, bias) if o.trim3 is None else int(o.trim3)
    if o.trim5 is None and o.trim3 is None and t5 > o.e:
        t5 = o.e
    return t5, t3


def even_reads(n, L=400, extra=0):
    """Reads whose every column holds each base n / 4 times (n a multiple of 4; beyond it reads of A alone, which add the same to
    every column): no column differs from another until a case makes it."""
    out = []
    for i in range(n + extra):
        s = bytearray(b"A" * L) if i >= n - n % 4 and i < n else bytearray(b"ACGT"[(i + j) % 4] for j in range(L))
        out.append([b"t%d" % i, s, bytes([35, 63] + [50] * (L - 2))])
    return out


class TrimCase:
    def __init__(self, reads, opts, want):
        self.reads, self.opts, self.in_fmt = done(reads), opts, "fq"
        self.trims = auto_trims(self.reads, opts)
        assert self.trims == want, (self.trims, want)


BARCODE = b"ACGT" * 40
PREFIX_T = (1, 2, 5, 6, 50, 148)


@functools.lru_cache(maxsize=None)
def prefix_case(t, end, kind):
    """The first (last) t positions the same in all reads.  kind "barcode": neighbouring positions hold different bases, every one
    of the t columns differs from both sides and the trim is t (from 2 on: column 0 is never looked at).  kind "same": one base;
    no column differs from BOTH its sides and nothing is trimmed."""
    reads = even_reads(100)
    fixed = BARCODE[:t] if kind == "barcode" else b"A" * t
    for r in reads:
        if end == 5:
            r[1][:t] = fixed
        else:
            r[1][len(r[1]) - t:] = rev_comp(fixed)
    got = t if kind == "barcode" and t >= 2 else 0
    return TrimCase(reads, Opts(trim5=None, trim3=None), (got, 0) if end == 5 else (0, got))


BIAS_SEAMS = [(b, n) for b in (1, 2, 8) for n in (100, 101)]


@functools.lru_cache(maxsize=None)
def bias_case(b, n, over):
    """Column 40 differs from its neighbours by int(seq_num * b / 100) (no trim) or by one more (trim 41); -n caps the sample."""
    reads = even_reads(n, extra=6)
    d = int(np.float32(n) * np.float32(b) / np.float32(100)) + over
    moved = [r for i, r in enumerate(reads[:100]) if (i + 40) % 4 == 0][:d]
    assert len(moved) == d
    for r in moved:
        r[1][40] = ord("C")
    for r in reads[n:]:                    # behind the cap: would change every column were they counted
        r[1][:] = b"G" * len(r[1])
    return TrimCase(reads, Opts(trim5=None, trim3=None, b=b, n=n, N=n), (41 if over else 0, 0))


CLAMPS = (("both", 5, (50, 0)), ("both", 3, (0, 80)), ("five_only", 5, (80, 0)))


@functools.lru_cache(maxsize=None)
def clamp_case(which, end):
    """-e 50 -E 50: the check length is 100, a barcode of 80 columns; the 5' trim is clamped to -e only when both are automatic."""
    reads = even_reads(100)
    for r in reads:
        if end == 5:
            r[1][:80] = BARCODE[:80]
        else:
            r[1][len(r[1]) - 80:] = rev_comp(BARCODE[:80])
    want = next(w for wh, e, w in CLAMPS if (wh, e) == (which, end))
    return TrimCase(reads, Opts(e=50, E=50, trim5=None, trim3=None if which == "both" else "0"), want)


def trim_lines(trims):
    return ["INFO: trim 5' end length: %d" % trims[0], "INFO: trim 3' end length: %d" % trims[1]]


def trim_check(case):
    def check(rc, err):
        assert rc == 0, err
        assert lines_with(err, "INFO: trim ") == trim_lines(case.trims), (err, case.trims)
    return check


def run_alone(binary, case):
    """One binary on the case's input: (return code, stderr)."""
    from tgsfilter_amd import synth
    with tempfile.TemporaryDirectory() as td:
        fin = os.path.join(td, "in.fq")
        synth.write_fastq(fin, case.reads)
        rc, _, err, _ = cli_check._run(binary, td, "run", fin, case.opts.flags(), None)
    return rc, err


def check_clamp_where_the_reference_races(binary, ref):
    """Both trims automatic and a 5' trim above -e: the reference clamps whatever its 5' thread has stored when its 3' thread
    gets there (:1135-1137), and prints 50 or 80 from run to run -- no line to compare with.  This side always clamps (the order
    seen on inputs of any size but the smallest); the reference, where it is there, must give one of the two."""
    case = clamp_case("both", 5)
    rc, err = run_alone(binary, case)
    assert rc == 0 and lines_with(err, "INFO: trim ") == trim_lines((50, 0)), err
    if ref:
        rc, err = run_alone(ref, case)
        assert rc == 0 and lines_with(err, "INFO: trim ") in (trim_lines((50, 0)), trim_lines((80, 0))), err


# ---- goldens --------------------------------------------------------------------------------------------------------------------
GOLDENS = {
    "prepass_sibling10": lambda: sibling_case(10),
    "prepass_depth_on": lambda: depth_case(12, 0.9, False),
    "prepass_depth_below": lambda: depth_case(12, 0.9, True),
    "prepass_call_seam": lambda: call_seam_case(4095, 4096),
    "prepass_three_prime": lambda: three_case(2),
    "prepass_five_times": lambda: five_times_case(11, False),
}


def write_golden(name):
    """tests/golden/make_golden.py: the input, the command and the reference's stderr."""
    from tgsfilter_amd import synth
    case = GOLDENS[name]()
    with tempfile.TemporaryDirectory() as td:
        fin = os.path.join(td, "in.fq")
        synth.write_fastq(fin, case.reads)
        p = subprocess.run([REF, "-i", fin, "-t", "1"] + case.opts.flags() + ["-o", os.path.join(td, "out.fq")], capture_output=True, cwd=td)
        err = p.stderr.decode().replace(td + "/", "")
        adapter_check(case)(p.returncode, err)
        with gzip.GzipFile(os.path.join(GOLDEN_DIR, name + ".in.fq.gz"), "wb", mtime=0) as f:
            f.write(open(fin, "rb").read())
    open(os.path.join(GOLDEN_DIR, name + ".stderr.txt"), "w").write(err)
    json.dump({"flags": " ".join(case.opts.flags()), "adapters": None, "returncode": p.returncode, "in_format": "fq"},
              open(os.path.join(GOLDEN_DIR, name + ".cmd.json"), "w"), indent=1)
    return err


def golden_reads(name):
    text = gzip.open(os.path.join(GOLDEN_DIR, name + ".in.fq.gz"), "rb").read().split(b"\n")
    return [(text[i][1:], text[i + 1], text[i + 3]) for i in range(0, len(text) - 1, 4)]


def check_golden(binary, name):
    """The committed input through `binary`: its INFO and Warning lines are the reference's; and the committed input is the case
    as it is built today, so that the model's answer is asserted against the committed lines as well."""
    cmd = json.load(open(os.path.join(GOLDEN_DIR, name + ".cmd.json")))
    ref_err = open(os.path.join(GOLDEN_DIR, name + ".stderr.txt")).read()
    case = GOLDENS[name]()
    assert golden_reads(name) == case.reads and cmd["flags"].split() == case.opts.flags()
    adapter_check(case)(cmd["returncode"], ref_err)
    with tempfile.TemporaryDirectory() as td:
        fin = os.path.join(td, "in.fq")
        open(fin, "wb").write(gzip.open(os.path.join(GOLDEN_DIR, name + ".in.fq.gz"), "rb").read())
        p = subprocess.run([binary, "-i", fin, "-t", "1"] + cmd["flags"].split() + ["-o", os.path.join(td, "out.fq")], capture_output=True, cwd=td)
        err = p.stderr.decode().replace(td + "/", "")
    assert p.returncode == cmd["returncode"], err
    keep = lambda text: [l for l in lines_with(text, "INFO:", "Warning:") if not l.startswith("Warning: reset -t")]
    assert keep(err) == keep(ref_err), "stderr differs:\n%s\n---- reference:\n%s" % (err, ref_err)
