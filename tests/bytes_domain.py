"""The byte domain: every byte value through the kernels that read bases and qualities.

tgsf_submit, tgsf_submit_device and tgsf_align_windows take any byte, and the kernels classify bytes with bit tricks that are
right only if every bit of the byte counts: the case fold and the bit-7 test of the QC columns (qc_accum4, k_tail_fix,
base_col), the validity masks of the k-mer codes (base_code, base_codes4), the 256-row Eq tables of the Myers columns, and
the signed `quality - qType` that travels through 32- and 64-bit sums into the unsigned tallies.  The rest of the suite draws
its bases from ACGT with a sprinkle of N and lower case, and its qualities from qType+1 .. qType+60 (or from 128 up): a slip
of one bit in any of those places goes unseen there.  Here the inputs hold every value, at every offset of the 4- and 16-byte
words the kernels load, on the seams of bins, tiles and end tables -- and every check compares records, fragments and every
tally word with the oracle (parity.compare_batch).  tests/test_bytes_emul.py runs the checks on the serial emulation (and
pins the oracle itself against the reference on these bytes), tests/test_bytes_gpu.py on the HIP build.

Each input comes with an assertion on the input itself (coverage of the values, the quirks present, adapters found at the
ends and in the middle): a change of a generator that empties a case fails instead of passing."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from oracle import orc
from tests import parity
from tgsfilter_amd import abi, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EDLIB = os.path.join(ROOT, "oracle", "_ref", "libedlib_ref.so")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "tgsfilter_ref")

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ADS = [synth.ONT_RAPID, synth.ONT_RAPID_RC]
MODES = [None, "direct", "difference", "byproduct"]          # TGSF_CLEAN_TABLES
TRIMS = [(0, 0), (79, 0), (7, 8), (100, 3)]                  # -5 / -3: none, a head piece of most of a bin, both, a whole bin

# the one-bit neighbours of A C G T a c g t (eight a letter: 0x40 0x43 0x45 0x49 0x51 0x61 0x01 0xC1 for A) and the bytes
# whose (c - 'A') & 31 is 0, 2, 6 or 19 -- what a validity mask indexed that way can take for a base; the letters themselves
# are among them
NEIGHBOURS = bytes(sorted({c ^ (1 << b) for c in b"ACGTacgt" for b in range(8)}
                          | {c for c in range(256) if ((c - 0x41) & 31) in (0, 2, 6, 19)}))
HIGH_BASES = bytes([0xC1, 0xE1, 0xD4, 0xF4, 0xC7, 0xE7, 0xC3, 0xE3])       # a base letter of either case with bit 7 set
NOT_NEWLINE = 0x8A                                           # stands in for "\n" where the layout is FASTQ text


def carpet(n=4096):
    """n bytes in which every value 0..255 occurs at every offset mod n / 256 (4096: mod 16, 1024: mod 4): block b of 256
    bytes holds the values in order, rotated by b."""
    i = np.arange(n)
    return ((i + i // 256) & 255).astype(np.uint8)


def covers(buf, mod, values=range(256)):
    """Does every one of `values` occur in buf at every offset mod `mod`?"""
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    seen = np.zeros((256, mod), dtype=bool)
    seen[a, np.arange(a.size) % mod] = True
    return bool(seen[list(values)].all())


def mutate256(rng, s, rate):
    """synth.mutate with the substituted and inserted bytes drawn from all 256 values."""
    out = bytearray()
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.integers(0, 256)))
            out.append(ch)
            continue
        if u < rate:
            out.append(int(rng.integers(0, 256)))
            continue
        out.append(ch)
    return bytes(out)


# ---------------------------------------------------------------------------
# 1. the inputs of the tally checks
# ---------------------------------------------------------------------------
SEQ_CARPETS = [(5003, (0,), ()), (7777, (), (7777 - 4096,)), (12345, (4352,), ()), (6161, (1237,), ()), (9037, (0,), (9037 - 4096,))]
QUAL_CARPETS = [(4501, 0), (5555, 5555 - 1024), (8011, 5900), (4807, 1237)]


@functools.lru_cache(maxsize=None)
def domain_batch(qtype=33, newline=True):
    """56 reads: ordinary zoo reads (trims, splits, low-quality drops) around
      * sequence carpets (carpet(4096), forwards at `fwd`, backwards at `bwd`) in reads of 5-12 kb: from the first base, up to
        the last one (in a last, partial bin), across the tile seam at 6 400, at an odd place, over both ends of one read;
      * quality carpets (carpet(1024)) in reads of 4.5-8 kb whose other qualities are 120..126, over bases of every class;
      * runs of quality bytes in 33..63 over a whole bin and across dwords (below the offset at qType 64);
      * reads drawn from NEIGHBOURS;
      * reads whose first 112 and last 8 bases and qualities are odd ones (the head and tail pieces of the by-product, k_tail_fix).
    qtype: what the ordinary qualities are offset by.  newline=False: no byte 10 anywhere (the in-place FASTQ-text layout)."""
    rng = np.random.default_rng(4242 + qtype)
    nl = (lambda a: a) if newline else (lambda a: np.where(a == 10, NOT_NEWLINE, a).astype(np.uint8))
    reads = []
    for name, s, q in synth.make_reads(4243, 24, "ont", mean_len=3000, zoo=True, pmid=0.1):
        reads.append((name, s, bytes(min(c + qtype - 33, 126) for c in q)))
    cp, cq = nl(carpet(4096)), nl(carpet(1024))
    for k, (L, fwd, bwd) in enumerate(SEQ_CARPETS):
        s = _ACGT[rng.integers(0, 4, L)].copy()
        for at in fwd:
            s[at:at + 4096] = cp
        for at in bwd:
            s[at:at + 4096] = cp[::-1]
        if k == 2:                                             # a split in front of the carpet: it lies in a clean fragment that starts elsewhere
            s[1500:1550] = np.frombuffer(synth.ONT_RAPID, dtype=np.uint8)
        if k == 3:                                             # a 5' adapter
            s[7:57] = np.frombuffer(synth.ONT_RAPID, dtype=np.uint8)
        reads.append((b"seqcarpet%d" % k, s.tobytes(), (rng.integers(12, 40, L) + qtype).astype(np.uint8).tobytes()))
    mixed = np.frombuffer(b"ACGT" * 6 + b"acgtN\xc1\xd4\x00", dtype=np.uint8)
    for k, (L, at) in enumerate(QUAL_CARPETS + QUAL_CARPETS):
        L += 300 * (k // 4)
        s = mixed[rng.integers(0, len(mixed), L)].copy()
        if at >= 100 and k % 2:
            s[5:55] = np.frombuffer(synth.ONT_RAPID, dtype=np.uint8)
        q = rng.integers(120, 127, L).astype(np.uint8)
        q[at:at + 1024] = cq
        reads.append((b"qualcarpet%d" % k, s.tobytes(), q.tobytes()))
    for k in range(4):
        L = 2900 + 101 * k
        q = np.full(L, 126, dtype=np.uint8)
        a = int(rng.integers(0, L - 210))
        q[a:a + 205] = np.array([33, 63, 48], dtype=np.uint8)[np.arange(a, a + 205) % 3]
        reads.append((b"lowrun%d" % k, _ACGT[rng.integers(0, 4, L)].tobytes(), q.tobytes()))
    nb = np.frombuffer(NEIGHBOURS, dtype=np.uint8)
    for k in range(6):
        L = 4000 + 7 * k
        reads.append((b"neighbours%d" % k, nb[rng.integers(0, len(nb), L)].tobytes(), (rng.integers(12, 40, L) + qtype).astype(np.uint8).tobytes()))
    odd_b = np.frombuffer(NEIGHBOURS + HIGH_BASES * 4, dtype=np.uint8)
    odd_q = np.array([128, 255, 200, 0, 32, 63, 11, 129, 64, 1, 127, 192], dtype=np.uint8)
    for k in range(8):
        L = 1500 + 113 * k
        s = _ACGT[rng.integers(0, 4, L)].copy()
        q = rng.integers(120, 127, L).astype(np.uint8)
        s[:112] = odd_b[rng.integers(0, len(odd_b), 112)]
        q[16:112] = odd_q[rng.integers(0, len(odd_q), 96)]      # (not the first 16: the by-product's guess of the mean samples them)
        s[L - 8:] = np.roll(np.frombuffer(HIGH_BASES if k % 2 == 0 else b"gtGTacAC", dtype=np.uint8), k)
        q[L - 8:] = np.roll(odd_q[:8], k)
        reads.append((b"ends%d" % k, s.tobytes(), q.tobytes()))
    assert newline or not any(10 in s or 10 in q for _, s, q in reads)
    return tuple(reads)


def inputs_cover():
    """The coverage the inputs are there for, asserted on the inputs."""
    assert covers(carpet(4096), 16) and covers(carpet(4096)[::-1], 16) and covers(carpet(1024), 4)
    assert all(c in NEIGHBOURS for c in b"ACGTacgt\x40\x43\x45\x49\x51\x61\x01\xc1")
    for qtype in (33, 64):
        for newline in (True, False):
            reads = {name: (s, q) for name, s, q in domain_batch(qtype, newline)}
            assert 32 <= len(reads) <= 64
            values = [v for v in range(256) if newline or v != 10]
            for k, (L, fwd, bwd) in enumerate(SEQ_CARPETS):
                s = reads[b"seqcarpet%d" % k][0]
                assert len(s) == L and 4000 <= L <= 16000
                for at in fwd + bwd:
                    assert covers(s[at:at + 4096], 16, values), (k, at)
            # ... across a bin seam (every one), the tile seam, into the read's last, partial bin, over the first and last bc_len bases
            assert any(at < 6400 < at + 4096 for L, f, b in SEQ_CARPETS for at in f + b)
            assert any(at + 4096 == L and L % 100 for L, f, b in SEQ_CARPETS for at in b)
            assert any(at == 0 for L, f, b in SEQ_CARPETS for at in f)
            for k, (L, at) in enumerate(QUAL_CARPETS):
                s, q = reads[b"qualcarpet%d" % k]
                assert covers(q[at:at + 1024], 4, values) and 4 * 1024 <= len(q)
                assert all(120 <= c <= 126 for c in q[:at] + q[at + 1024:])
            nbs = b"".join(reads[b"neighbours%d" % k][0] + b"\0" * (-len(reads[b"neighbours%d" % k][0]) % 16) for k in range(6))
            assert covers(nbs, 16, NEIGHBOURS)
            tails = b"".join(reads[b"ends%d" % k][0][-8:] for k in range(8))
            assert all(c in tails for c in HIGH_BASES + b"acgtACGT")
            assert any(c >= 128 for k in range(8) for c in reads[b"ends%d" % k][1][-8:])
            if qtype == 64:
                assert any(33 <= c < 64 for k in range(4) for c in reads[b"lowrun%d" % k][1])


def means_in_range(p, reads, n_bins=None):
    """From the oracle's result: nothing is refused (it answers TGSF_E_DATA -- filter_batch raises -- where the reference would
    index out of bounds) and every read's and every kept fragment's mean quality lies in [0, 256)."""
    seq, qual, offsets, lengths = synth.pack(reads)
    r, f, _ = orc.filter_batch(p, seq, qual, offsets, lengths, n_bins=n_bins)
    if p.no_qual:
        return r, f
    m = r["sum_q"].astype(np.int64) / np.maximum(lengths, 1)
    assert ((m >= 0) & (m < 256)).all(), m
    kept = f[(f["flags"] & abi.FF_PASS) != 0]
    mk = kept["sum_q"].astype(np.int64) / kept["len"]
    assert len(kept) and ((mk >= 0) & (mk < 256)).all(), mk
    return r, f


def _in_place_sized(p, reads):
    p.max_batch_reads = len(reads)
    p.max_batch_bases = 2 * sum(len(r[1]) for r in reads) + 64 * len(reads) + 4096
    p.max_read_len = max(len(r[1]) for r in reads)
    return p


def _set_mode(monkeypatch, mode, pool_cap=None):
    monkeypatch.setenv("TGSF_CLEAN_TABLES", mode) if mode else monkeypatch.delenv("TGSF_CLEAN_TABLES", raising=False)
    monkeypatch.setenv("TGSF_POOL_CAP", str(pool_cap)) if pool_cap else monkeypatch.delenv("TGSF_POOL_CAP", raising=False)


# ---------------------------------------------------------------------------
# 2. tallies
# ---------------------------------------------------------------------------
def tallies(lib_path, mode, head, tail, qtype, monkeypatch, pool_cap=None, long_tables=False):
    """domain_batch under one strategy for the clean tables and one pair of trims: packed at 16-byte alignment with -e 150,
    packed back to back (reads start anywhere) with -e 513 (two slabs of k_end_tables), and as FASTQ text in place.
    long_tables: a context whose bin tables have more rows than k_tail_fix's LDS holds (as parity.tail_fix_long_tables)."""
    _set_mode(monkeypatch, mode, pool_cap)
    kw = dict(adapters=ADS, min_q=7.0, head_trim=head, tail_trim=tail, qtype=qtype)
    reads = list(domain_batch(qtype, True))
    means_in_range(parity.sized(abi.make_params("ont", **kw), reads), reads)
    for bc_len, align in ((150, 16), (513, 1)):
        p = parity.sized(abi.make_params("ont", bc_len=bc_len, **kw), reads)
        if long_tables:
            p.max_read_len = 250_000
        ctx = capi.Context(p, 0, lib_path)
        try:
            assert not long_tables or ctx.n_bins > 1024
            res, frags, ctr = parity.compare_batch(ctx, p, reads, align=align)
            assert (res["n_frags"] > 1).any() and (res["trimmed"] > head + tail).any() and (res["flags"] & abi.RF_LOWQ).any()
        finally:
            ctx.close()
    reads = list(domain_batch(qtype, False))
    p = _in_place_sized(abi.make_params("ont", **kw), reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        parity.compare_batch_in_place(ctx, p, reads)
    finally:
        ctx.close()


def no_qual_tallies(lib_path, mode, monkeypatch):
    """Records without qualities: the count tables, with the reference's two quirks (a `g` within -e of the 5' end and a `t`
    within -e of the 3' end reach only the "all" column, src/TGSFilter.cpp:1629, :1667) present in the input -- beside a `t` at
    the 5' end and a `g` at the 3' end, which count as T and G."""
    _set_mode(monkeypatch, mode)
    reads = list(domain_batch(33, True))
    both = dict((name, s) for name, s, q in reads)[b"seqcarpet4"]
    for bc_len, align in ((150, 16), (513, 1)):
        for letters in (both[:bc_len], both[-bc_len:]):
            assert ord("g") in letters and ord("t") in letters and ord("G") in letters and ord("T") in letters
        p = parity.sized(abi.make_params("ont", adapters=ADS, head_trim=3, bc_len=bc_len, no_qual=True), reads)
        ctx = capi.Context(p, 0, lib_path)
        try:
            res, frags, ctr = parity.compare_batch(ctx, p, reads, align=align)
            assert (res["sum_q"] == 0).all() and (frags["sum_q"] == 0).all() and (res["n_frags"] > 1).any()
        finally:
            ctx.close()


# ---------------------------------------------------------------------------
# 3. the Myers columns
# ---------------------------------------------------------------------------
LIBRARY = {22: b"GCAATACGTAACTGAACGAAGT", 28: b"AATGTACTTCGTTCAGTTACGTATTGCT", 45: synth.PACBIO_BLUNT}
ALPHABETS = {"lower": b"acgt", "iupac": b"RYKMSWBDHVN=0123456789", "ctrl_high": bytes(range(0, 32)) + bytes(range(128, 256))}
# one set per class of column: lengths, parameters
MYERS_SETS = {
    "dword": ((22, 28), dict(mid_match_len=18)),            # at most 32 bp: the one-dword column
    "filter45": ((45,), dict(mid_match_len=35)),            # within 11 <= kSuffixMaxK differences: k_mid_flat as a filter + k_mid_recheck
    "beyond45": ((45,), dict(mid_match_len=30)),            # within 16: the 64-bit column
    "words": ((90, 150, 241), dict(end_match_len=24)),                     # two- and four-word columns
    "wide": ((300,), dict(mid_match_len=120, end_match_len=24)),             # beyond 256 bp: the wide column
}
MYERS_ENVS = [{}, {"TGSF_MID_FLAT": "0"}, {"TGSF_MID_FILTER": "0"}]


def odd_adapter(Q, kind):
    """An adapter of Q bytes: "lower" the library adapter of that length in lower case (a random one where the library has
    none), "iupac" over IUPAC codes, N, = and digits, "ctrl_high" over bytes 0..31 and 128..255, "many" over more than 64
    distinct values.  NUL is among them: tgsf_create takes an adapter's length from tgsf_params.adapter_len, never from a
    terminator."""
    rng = np.random.default_rng(1000 * Q + sorted(list(ALPHABETS) + ["many"]).index(kind))
    if kind == "lower" and Q in LIBRARY:
        return LIBRARY[Q].lower()
    if kind == "many":
        a = rng.permutation(256).astype(np.uint8)[np.arange(Q) % 256]
    else:
        al = np.frombuffer(ALPHABETS[kind], dtype=np.uint8)
        a = al[rng.integers(0, len(al), Q)].copy()
    if kind == "ctrl_high":
        a[Q // 3] = 0
    return a.tobytes()


def set_adapters(name):
    lens, _ = MYERS_SETS[name]
    return [(odd_adapter(Q, kind), kind) for Q in lens for kind in ("lower", "iupac", "ctrl_high", "many") if kind != "many" or Q >= 90]


@functools.lru_cache(maxsize=None)
def myers_case(name):
    """(params' keywords, reads) of one set: reads random over the symbols of the set's adapters and others (NUL among them),
    each with a copy of one adapter (mutate256: 0, 3 or 6 % of its bytes replaced, inserted or deleted, from all 256 values) at
    the 5' end, at the 3' end, in the middle or straddling -E.  The lower-case adapters sit in upper-case reads -- in every
    third one as an upper-case copy, which is no copy at all."""
    ads = set_adapters(name)
    assert all(len(set(a)) > 64 for a, kind in ads if kind == "many") and any(0 in a for a, _ in ads)
    rng = np.random.default_rng(sorted(MYERS_SETS).index(name) + 31)
    union = np.frombuffer(bytes(sorted(set(b"".join(a for a, _ in ads)) | set(b"ACGTN\x00\x7f\xff"))), dtype=np.uint8)
    n = max(64, 8 * len(ads))
    reads = []
    for i in range(n):
        a, kind = ads[i % len(ads)]
        rep = i // len(ads)
        L = int(rng.integers(900, 2000)) + len(a)
        if kind == "lower":
            s = bytearray(_ACGT[rng.integers(0, 4, L)].tobytes())
            a = a.upper() if rep % 3 == 2 else a
        else:
            s = bytearray(union[rng.integers(0, len(union), L)].tobytes())
        m = mutate256(rng, a, (0.0, 0.03, 0.06)[(i // 2) % 3])
        at = (int(rng.integers(0, 10)), L - len(m) - int(rng.integers(0, 10)), L // 2,
              150 - len(m) // 2 if rep % 2 else L - 150 - len(m) // 2)[(rep + i) % 4]
        at = max(0, min(at, L - len(m)))
        s[at:at + len(m)] = m
        if i % 5 == 0:
            s[int(rng.integers(0, L))] = 0
        reads.append((b"%s%d" % (name.encode(), i), bytes(s), bytes(rng.integers(60, 70, L, dtype=np.uint8))))
    kw = dict(adapters=[a for a, _ in ads], min_len=100, end_sim=0.7, mid_sim=0.8, **MYERS_SETS[name][1])
    return kw, tuple(reads)


def myers_found(name):
    """The oracle alone: at least 10 reads of the set trimmed at an end and at least 10 split in the middle."""
    kw, reads = myers_case(name)
    reads = list(reads)
    p = parity.sized(abi.make_params("ont", **kw), reads)
    seq, qual, offsets, lengths = synth.pack(reads)
    r, f, _ = orc.filter_batch(p, seq, qual, offsets, lengths)
    ends = int(((r["flags"] & (abi.RF_AD5P | abi.RF_AD3P)) != 0).sum())
    split = int((((r["flags"] & abi.RF_ADMID) != 0) & (r["n_frags"] >= 2)).sum())
    assert ends >= 10 and split >= 10, (name, ends, split)
    return ends, split


def myers(lib_path, name, env, monkeypatch):
    for k in ("TGSF_MID_FLAT", "TGSF_MID_FILTER", "TGSF_CLEAN_TABLES", "TGSF_POOL_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw, reads = myers_case(name)
    reads = list(reads)
    p = parity.sized(abi.make_params("ont", **kw), reads)
    ctx = capi.Context(p, 0, lib_path)
    try:
        if env:
            res, frags, ctr = parity.compare_batch(ctx, p, reads, align=1, explicit_lengths=False)
        else:
            res, frags, ctr = parity.compare_batch(ctx, p, reads)
        assert ((res["flags"] & (abi.RF_AD5P | abi.RF_AD3P)) != 0).sum() >= 10 and ((res["flags"] & abi.RF_ADMID) != 0).sum() >= 10
    finally:
        ctx.close()


ALIGN_CLASSES = {"two_words": ("dword", "filter45"), "four_words": ("words",), "wide": ("wide",)}      # k_align_windows<2 | 4 | kWideNW>: up to the column forms Bv<2>, Bv<4>, BvW


def align_windows(lib_path, cls, n):
    """The sets' adapters through tgsf_align_windows: windows over the adapters' symbols, ACGT and NUL with mutated copies,
    against the reference's edlib where it was built, else against the oracle's."""
    ads = [a for name in ALIGN_CLASSES[cls] for a, _ in set_adapters(name)]
    alphabet = bytes(sorted(set(b"".join(ads)) | set(b"ACGT\x00")))
    parity.align_windows_random(lib_path, n, seed=17 + len(ads), adapters=ads, alphabet=alphabet, mutate=mutate256)


# ---------------------------------------------------------------------------
# 4. the repeat gate
# ---------------------------------------------------------------------------
REPEAT_ALPHABETS = {
    "acgt_and_all_others": b"ACGT" * (9 * 63) + bytes(c for c in range(256) if c not in b"ACGT"),     # 90 % ACGT, 10 % the other 252 values
    "lower_case": b"acgt",                                   # every k-mer has code 0: the count is the largest there is
    "neighbours": NEIGHBOURS,
}
REPEAT_KS = [5, 11, 12, 15, 31, 32]
REPEAT_LENS = parity.REPEAT_TINY + [500, 1023, 1025, 4097]


def repeat_gate(lib_path, alphabet, k):
    al = REPEAT_ALPHABETS[alphabet]
    if alphabet == "acgt_and_all_others":
        assert len(set(al)) == 256 and al.count(b"A") * 4 * 10 == 9 * len(al)
    parity.repeat_threshold_case(lib_path, k, REPEAT_LENS, max_runs=16, alphabet=al)


def repeat_counted_in_memory(lib_path, monkeypatch, k=31, units=9000):
    """The gate's last resort, rep_distinct_in_memory (it codes its bases one by one with base_code): a fragment of thousands of
    distinct duplicated k-mers that share their first 16 bases (as tests/test_emul_parity.py's _shared_prefix_read), with
    TGSF_REP_MAX_PLOG=0 (counted in memory at the first overflow of a pass's table).  The fragment is a block and its copy; in
    the copy every fifth A is another byte of code 0 -- any of the 253 values that are not C, G or T, the neighbours of the
    letters more often than others --, so the copy repeats the block's k-mers only if each of those bytes is coded as an A is.
    The read's own count passes, one more drops it."""
    monkeypatch.setenv("TGSF_REP_MAX_PLOG", "0")
    rng = np.random.default_rng(55)
    pre = _ACGT[rng.integers(0, 4, 16)]
    block = np.concatenate([np.concatenate([pre, _ACGT[rng.integers(0, 4, k - 16)]]) for _ in range(units)])
    zero = np.frombuffer(bytes(c for c in NEIGHBOURS * 3 + bytes(range(256)) if c not in b"CGT"), dtype=np.uint8)
    copy = block.copy()
    at = np.nonzero(block == ord("A"))[0][::5]
    copy[at] = zero[rng.integers(0, len(zero), at.size)]
    assert len(set(copy[at].tolist())) == 253
    s = block.tobytes() + copy.tobytes()
    read = (b"shared_prefix_odd", s, bytes((rng.integers(15, 35, len(s)) + 33).astype(np.uint8)))
    c = parity._kmer_repeat_np(s, k)
    assert c == parity._kmer_repeat_np(block.tobytes() * 2, k) > units * (k - 1)
    for pval, kept in ((c, True), (c + 1, False)):
        p = parity.sized(abi.make_params("ont", adapters=[], min_q=7.0, min_repeat=pval, kmer=k), [read])
        ctx = capi.Context(p, 0, lib_path)
        try:
            res, frags, ctr = parity.compare_batch(ctx, p, [read])
            assert len(frags) == 1 and bool(frags["flags"][0] & abi.FF_PASS) == kept and bool(frags["flags"][0] & abi.FF_REPEAT) == (not kept)
        finally:
            ctx.close()


# ---------------------------------------------------------------------------
# 5. the oracle against the reference on these bytes
# ---------------------------------------------------------------------------
def ref_edlib():
    """edlibAlign(HW, PATH) of oracle/_ref/libedlib_ref.so as a function (q, t, k) -> (ed, n, starts, ends, alen); None where
    it was not built."""
    if not os.path.exists(REF_EDLIB):
        return None

    class Cfg(C.Structure):
        _fields_ = [("k", C.c_int), ("mode", C.c_int), ("task", C.c_int), ("eq", C.c_void_p), ("neq", C.c_int)]

    class Res(C.Structure):
        _fields_ = [("status", C.c_int), ("editDistance", C.c_int), ("endLocations", C.POINTER(C.c_int)),
                    ("startLocations", C.POINTER(C.c_int)), ("numLocations", C.c_int),
                    ("alignment", C.POINTER(C.c_ubyte)), ("alignmentLength", C.c_int), ("alphabetLength", C.c_int)]
    lib = C.CDLL(REF_EDLIB)
    lib.edlibAlign.restype = Res
    lib.edlibAlign.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, Cfg]
    lib.edlibFreeAlignResult.argtypes = [Res]

    def run(q, t, k):
        r = lib.edlibAlign(q, len(q), t, len(t), Cfg(k, 2, 2, None, 0))
        out = (r.editDistance, r.numLocations, [r.startLocations[i] for i in range(r.numLocations)],
               [r.endLocations[i] for i in range(r.numLocations)], r.alignmentLength)
        lib.edlibFreeAlignResult(r)
        return out
    return run


def oracle_edlib_all_bytes(edlib, n=2000):
    """orc.align_hw against the reference's edlib with queries and targets over all 256 values (alphabets of 2 to 256 symbols
    picked anywhere among them, NUL included)."""
    rng = np.random.default_rng(2025)
    hits, seen = 0, np.zeros(256, dtype=bool)
    for it in range(n):
        Q = int(rng.choice([5, 22, 28, 45, 50, 64, 65, 90, 128, 150, 241, 300]))
        sym = rng.permutation(256).astype(np.uint8)[:int(rng.choice([2, 4, 16, 64, 256]))]
        q = sym[rng.integers(0, len(sym), Q)].tobytes()
        T = int(rng.integers(5, 30)) if it % 5 == 0 else int(rng.integers(5, 620))
        t = bytearray(sym[rng.integers(0, len(sym), T)].tobytes())
        for _ in range(int(rng.integers(0, 3))):
            m = mutate256(rng, q, float(rng.choice([0.0, 0.03, 0.1, 0.2, 0.3])))
            if m and rng.random() < 0.3:
                m = m[:int(rng.integers(1, len(m) + 1))]
            at = int(rng.integers(0, max(1, T)))
            t[at:at + len(m)] = m
        t = bytes(t[:max(5, min(len(t), 620))])
        k = max(0, int(rng.choice([Q - 3, Q - 34, Q - 14, 3, Q // 3, Q - 1])))
        a, b = edlib(q, t, k), orc.align_hw(q, t, k)
        assert a == b, (q, t, k, a, b)
        hits += a[0] >= 0
        seen[np.frombuffer(q + t, dtype=np.uint8)] = True
    assert hits > n // 4 and seen.all()


# what the sequence and quality lines of odd_fastq() carry besides ordinary letters.  The command line's reader (tests/textmodel.py,
# Reader.line; the reference's getLine, src/TGSFilter.cpp:657-683) keeps every byte of a line but the "\n" that ends it and one
# "\r" in front of that, so every value but 10 can stand anywhere but at the end of a line, where 13 is left out as well.
ODD_TEXT_BASES = bytes(c for c in range(256) if c != 10)
ODD_TEXT_QUALS = bytes(c for c in range(256) if c != 10)


def odd_bytes_into(reads, seed):
    """`reads` with odd bytes: a tenth of the bases of every other read from all values but "\\n", the first and last 30
    bases of every fourth from NEIGHBOURS, a fifth of the quality bytes of every fourth read from all values but "\\n" beside
    qualities of 120..126 (the mean stays in [0, 256)).  No line ends in "\\r"."""
    rng = np.random.default_rng(seed)
    ob, oq = np.frombuffer(ODD_TEXT_BASES, dtype=np.uint8), np.frombuffer(ODD_TEXT_QUALS, dtype=np.uint8)
    nb = np.frombuffer(NEIGHBOURS, dtype=np.uint8)
    out = []
    for i, (name, s, q) in enumerate(reads):
        s, q = np.frombuffer(s, dtype=np.uint8).copy(), np.frombuffer(q, dtype=np.uint8).copy()
        L = len(s)
        if i % 2 == 0 and L > 300:
            at = rng.integers(0, L, L // 10)
            s[at] = ob[rng.integers(0, len(ob), len(at))]
        if i % 4 == 1 and L > 300:
            s[:30] = nb[rng.integers(0, len(nb), 30)]
            s[L - 30:] = nb[rng.integers(0, len(nb), 30)]
        if i % 4 == 2 and L > 1200:
            q[:] = rng.integers(120, 127, L)
            at = rng.integers(0, L, L // 5)
            q[at] = oq[rng.integers(0, len(oq), len(at))]
        if s[-1] == 13:
            s[-1] = 65
        if q[-1] == 13:
            q[-1] = 120
        out.append((name, s.tobytes(), q.tobytes()))
    return out


def odd_reads(seed, n=40, mean_len=2500):
    return odd_bytes_into(synth.make_reads(seed, n, "ont", mean_len=mean_len, zoo=True, pmid=0.1), seed)


def odd_fastq(seed, n=40):
    return b"".join(b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n" for name, s, q in odd_reads(seed, n))
