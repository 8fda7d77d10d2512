"""Shared checks of libtgsf_text (include/tgsf_text.h): a backend (the HIP build on the GPU box, the serial emulation of
the same kernels elsewhere) against tests/textmodel.py, and the one-call form against libtgsf with a host-made index and
against the oracle.  tests/test_text_emul.py and tests/test_text_gpu.py run them."""
from __future__ import annotations

import numpy as np

from oracle import orc
from tests import parity, textmodel
from tgsfilter_amd import abi, capi, synth, text as tgtext

FIELDS = ("seq_off", "qual_off", "len", "name_off", "name_len")


def fastq_of(reads, eol=b"\n"):
    return b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in reads)


def fasta_of(reads, eol=b"\n"):
    return b"".join(b">" + n + eol + s + eol for n, s, q in reads)


def assert_index(got, summary, text, fasta, final, max_records, what=""):
    """Index and summary of one call against the rule, word for word."""
    recs, consumed, stop = textmodel.rule(text, fasta, final, max_records)
    exp = textmodel.expected_index(recs)
    assert summary["n_records"] == len(recs), (what, summary, len(recs), consumed, stop)
    assert summary["consumed"] == consumed and summary["stop"] == stop, (what, summary, consumed, stop)
    for f in FIELDS:
        g = getattr(got, f)
        assert g.dtype == exp[f].dtype and np.array_equal(g, exp[f]), (what, f, g[:8], exp[f][:8])
    assert summary["bases"] == int(exp["len"].astype(np.uint64).sum()), (what, summary)
    assert summary["longest"] == (int(exp["len"].max()) if recs else 0), (what, summary)
    return recs, consumed, stop


def check_text(lib, text, fasta=False, final=True, max_records=None, tx=None, what=""):
    recs_all = max(1, text.count(b"\n") // 2 + 2)
    own = tx is None
    if own:
        tx = tgtext.TextIndexer(0, max(len(text), 1), max_records or recs_all, lib)
    try:
        got, s = tx.index(text, fasta=fasta, final=final)
        return assert_index(got, s, text, fasta, final, tx.max_records, what)
    finally:
        if own:
            tx.close()


def unusual_texts():
    from tests.test_cli_live import case3
    return [case3(seed, 40)[0] for seed in range(6000, 6006)]


def damaged_texts(seed=11, per_class=12):
    rng = np.random.default_rng(seed)
    out = []
    for damage in textmodel.DAMAGE:
        for i in range(per_class):
            fasta = bool(i & 1)
            out.append((damage, fasta, textmodel.make_text(rng, fasta, n_records=int(rng.integers(1, 9)), damage=damage)))
    return out


def long_line_text(seed=13, long_len=300_000, n_short=30):
    """One read of 300 kb (dozens of 4 KiB pieces without a line end) among short ones."""
    reads = synth.make_reads(seed, n_short, "ont", mean_len=800, zoo=False)
    rng = np.random.default_rng(seed)
    s = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, long_len)])
    q = bytes((rng.integers(5, 40, long_len) + 33).astype(np.uint8))
    reads.insert(n_short // 2, (b"long", s, q))
    return reads


def capacity_then_rest(lib, text, fasta, max_records):
    """CAPACITY, then calls from `consumed` complete the file: the indexes concatenated are the whole file's."""
    whole, _, stop_all = textmodel.rule(text, fasta, True)
    tx = tgtext.TextIndexer(0, len(text), max_records, lib)
    try:
        at, got, calls = 0, [], 0
        while True:
            idx, s = tx.index(text[at:], fasta=fasta, final=True)
            assert_index(idx, s, text[at:], fasta, True, max_records, ("capacity", at))
            got += [(int(idx.name_off[i]) + at, int(idx.name_len[i]), int(idx.seq_off[i]) + at, int(idx.qual_off[i]) + at, int(idx.len[i]))
                    for i in range(s["n_records"])]
            at += s["consumed"]
            calls += 1
            if s["stop"] != tgtext.CAPACITY:
                break
            assert s["n_records"] == max_records
        assert got == whole and s["stop"] == stop_all and calls >= -(-len(whole) // max_records)
    finally:
        tx.close()


def cut_everywhere(lib, text, fasta):
    """A non-final cut at every byte, then a final call from `consumed` on the rest: together the whole file's index."""
    whole, consumed_all, stop_all = textmodel.rule(text, fasta, True)
    tx = tgtext.TextIndexer(0, len(text) + 1, len(whole) + 2, lib)
    try:
        for cut in range(len(text) + 1):
            a, sa = tx.index(text[:cut], fasta=fasta, final=False)
            assert_index(a, sa, text[:cut], fasta, False, tx.max_records, ("cut", cut))
            at = sa["consumed"]
            first = [(int(a.name_off[i]), int(a.name_len[i]), int(a.seq_off[i]), int(a.qual_off[i]), int(a.len[i])) for i in range(sa["n_records"])]
            if sa["stop"] == tgtext.IRREGULAR:                     # the damaged spot itself is the sequential reader's business
                assert first == whole[:len(first)] and len(first) == len(whole) and stop_all == tgtext.IRREGULAR
                continue
            b, sb = tx.index(text[at:], fasta=fasta, final=True)
            assert_index(b, sb, text[at:], fasta, True, tx.max_records, ("rest", cut))
            rest = [(int(b.name_off[i]) + at, int(b.name_len[i]), int(b.seq_off[i]) + at, int(b.qual_off[i]) + at, int(b.len[i])) for i in range(sb["n_records"])]
            assert first + rest == whole, (cut, at)
            assert at + sb["consumed"] == consumed_all and sb["stop"] == stop_all, (cut, sa, sb)
    finally:
        tx.close()


def fuzz(lib, seed, count, max_len=60):
    """Seeded texts of every damage class, both formats, final and cut at a random byte; returns how many were indexed to the
    end according to the model alone (stop == END and every record of the sequential reader)."""
    rng = np.random.default_rng(seed)
    tx = tgtext.TextIndexer(0, 1 << 16, 64, lib)
    to_end = 0
    try:
        for i in range(count):
            fasta = bool(rng.random() < 0.4)
            damage = textmodel.DAMAGE[int(rng.integers(0, len(textmodel.DAMAGE)))] if rng.random() < 0.6 else "none"
            text = textmodel.make_text(rng, fasta, damage=damage, max_len=max_len)
            final = bool(rng.random() < 0.7)
            if not final:
                text = text[:int(rng.integers(0, len(text) + 1))]
            got, s = tx.index(text, fasta=fasta, final=final)
            recs, consumed, stop = assert_index(got, s, text, fasta, final, tx.max_records, (seed, i, damage, fasta, final, text))
            # from the model alone: the sequential reader finds no record the index lacks, and nothing but an incomplete line is left
            seq_recs, _ = textmodel.read_all(text if final else text[:consumed], not fasta)
            to_end += stop == tgtext.END and len(recs) == len(seq_recs) and (final or consumed == text.rfind(b"\n") + 1)
    finally:
        tx.close()
    return to_end


# ---- the one-call form -------------------------------------------------------------------------------------------
def params_for(kind, reads, text_bytes, **kw):
    ad = [synth.ONT_RAPID, synth.ONT_RAPID_RC] if kind == "ont" else [synth.PACBIO_BLUNT, synth.PACBIO_BLUNT_RC]
    p = abi.make_params(kind, adapters=ad, **kw)
    p.max_batch_reads = len(reads)
    p.max_batch_bases = 2 * text_bytes + 64 * len(reads) + 4096            # the text itself is the batch
    p.max_read_len = max(len(r[1]) for r in reads)
    return p


def same_results(a, b):
    (ra, fa, ca), (rb, fb, cb) = a, b
    assert np.array_equal(ra, rb), "per-read records differ"
    assert np.array_equal(fa, fb), "fragments differ"
    bad = np.nonzero(ca != cb)[0]
    assert bad.size == 0, f"tally words differ at {bad[:12]}"


def chained(lib, text_lib, kind, reads, fasta=False, garbage_in_padding=False, **kw):
    """TextIndexer.submit(ctx, text) == ctx.submit with the host-made index == the oracle on that layout."""
    if fasta:
        text = fasta_of(reads)
        off, ln, pos = [], [], 0
        for n, s, q in reads:
            pos += len(n) + 2
            off.append(pos); ln.append(len(s))
            pos += len(s) + 1
        off, qoff, ln = np.array(off, np.uint64), None, np.array(ln, np.uint32)
        kw["no_qual"] = True
    else:
        padded, off, qoff, ln = parity.fastq_text_layout(reads)
        text = padded[:-64].tobytes()
    p = params_for(kind, reads, len(text), **kw)
    host_text = np.frombuffer(text + b"\0" * 64, dtype=np.uint8)
    ctx = capi.Context(p, 0, lib)
    try:
        r0, f0 = ctx.submit(host_text, host_text, off, ln, qual_offsets=qoff if not fasta else off)
        c0 = ctx.counters()
    finally:
        ctx.close()
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(text), len(reads), text_lib)
    try:
        er, ef, ec = orc.filter_batch(p, host_text, host_text, off, ln, n_bins=ctx.n_bins, qual_offsets=qoff if not fasta else off)
        if garbage_in_padding:                                 # bytes behind n_bytes in the caller's buffer are never looked at
            buf = np.frombuffer(text + b"\n@x\nAC\n+\nII\n" + b"\xff" * 52, dtype=np.uint8)
            idx, s, r1, f1 = tx.submit(ctx, buf[:len(text)])
        else:
            idx, s, r1, f1 = tx.submit(ctx, text, fasta=fasta)
        c1 = ctx.counters()
        assert s["n_records"] == len(reads) and s["stop"] == tgtext.END and s["consumed"] == len(text)
        assert np.array_equal(idx.seq_off, off) and np.array_equal(idx.len, ln)
        assert np.array_equal(idx.qual_off, off if fasta else qoff)
        same_results((r1, f1, c1), (r0, f0, c0))
        same_results((r1, f1, c1), (er, ef, ec))
    finally:
        tx.close()
        ctx.close()


def irregular_tail(lib, text_lib):
    """A text whose tail is irregular filters exactly the regular prefix."""
    reads = synth.make_reads(21, 30, "ont", mean_len=2000, zoo=True, pmid=0.1)
    good = fastq_of(reads[:20])
    text = good + b"@broken\nACGT\n+\nII\n" + fastq_of(reads[20:])
    p = params_for("ont", reads, len(text), min_q=9.0)
    ctx = capi.Context(p, 0, lib)
    tx = tgtext.TextIndexer(0, len(text), 64, text_lib)
    try:
        idx, s, r1, f1 = tx.submit(ctx, text)
        c1 = ctx.counters()
        assert s["n_records"] == 20 and s["stop"] == tgtext.IRREGULAR and s["consumed"] == len(good)
        padded, off, qoff, ln = parity.fastq_text_layout(reads[:20])
        er, ef, ec = orc.filter_batch(p, padded, padded, off, ln, n_bins=ctx.n_bins, qual_offsets=qoff)
        same_results((r1, f1, c1), (er, ef, ec))
        # nothing regular at all: no pipeline run, empty results, no error
        idx, s, r2, f2 = tx.submit(ctx, b"garbage\n" + good)
        assert s["n_records"] == 0 and s["stop"] == tgtext.IRREGULAR and s["consumed"] == 0 and len(r2) == 0 and len(f2) == 0
        assert np.array_equal(ctx.counters(), c1)
        idx, s, r2, f2 = tx.submit(ctx, b"", want_index=False)
        assert idx is None and s["n_records"] == 0 and s["stop"] == tgtext.END
    finally:
        tx.close()
        ctx.close()


def refusals(lib, text_lib):
    """Each refusal returns its code with a message, and the same TextIndexer then indexes a good text correctly."""
    reads = synth.make_reads(22, 12, "ont", mean_len=1500, zoo=False)
    text = fastq_of(reads)
    tx = tgtext.TextIndexer(0, len(text), 32, text_lib)

    def good_again(ctx):
        idx, s, r, f = tx.submit(ctx, text)
        assert s["n_records"] == len(reads) and s["stop"] == tgtext.END and len(r) == len(reads)
        got, s = tx.index(text)
        assert_index(got, s, text, False, True, tx.max_records)

    def refused(code, ctx, t, **kw):
        try:
            tx.submit(ctx, t, **kw)
        except capi.TgsfError as e:
            assert e.code == code and len(str(e)) > 20, (e.code, str(e))
            return str(e)
        raise AssertionError("accepted")

    try:
        p = params_for("ont", reads, len(text), min_q=9.0)
        ctx = capi.Context(p, 0, lib)
        assert "created for" in refused(-4, ctx, text + fastq_of(reads[:1]))           # above max_bytes: before anything is copied
        good_again(ctx)
        assert "fragment" in refused(-4, ctx, text, frag_capacity=3)                    # too few fragment slots (from tgsf_wait)
        good_again(ctx)
        ctx.close()
        p = params_for("ont", reads, len(text), min_q=9.0)
        p.max_batch_reads = 5
        ctx = capi.Context(p, 0, lib)
        assert "sized for 5" in refused(-4, ctx, text)                                  # more records than max_batch_reads
        ctx.close()
        p = params_for("ont", reads, len(text), min_q=9.0)
        p.max_read_len = min(len(r[1]) for r in reads)
        ctx = capi.Context(p, 0, lib)
        assert "max_read_len" in refused(-6, ctx, text)                                 # a read above max_read_len (from tgsf_wait)
        ctx.close()
        p = params_for("ont", reads, len(text), min_q=9.0)
        ctx = capi.Context(p, 0, lib)
        good_again(ctx)
        ctx.close()
    finally:
        tx.close()


# ---- full size ------------------------------------------------------------------------------------------------------
def full_size_block(seed=71, n=3000, mean_len=10000):
    """A block of n well-formed FASTQ records of ONT-like lengths and its index (numpy only)."""
    rng = np.random.default_rng(seed)
    lens = np.maximum(200, rng.gamma(2.0, mean_len / 2.0, n)).astype(np.int64)
    names = [b"@read_%d runid=%08x" % (i, int(rng.integers(0, 1 << 31))) for i in range(n)]
    parts, pos = [], 0
    idx = {f: np.zeros(n, np.uint64) for f in ("seq_off", "qual_off", "name_off")}
    idx["len"], idx["name_len"] = lens.astype(np.uint32), np.array([len(x) - 1 for x in names], np.uint32)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(n):
        L = int(lens[i])
        idx["name_off"][i] = pos + 1
        idx["seq_off"][i] = pos + len(names[i]) + 1
        idx["qual_off"][i] = pos + len(names[i]) + 1 + L + 3
        parts += [np.frombuffer(names[i] + b"\n", dtype=np.uint8), acgt[rng.integers(0, 4, L)], np.frombuffer(b"\n+\n", dtype=np.uint8),
                  (rng.integers(3, 40, L) + 33).astype(np.uint8), np.frombuffer(b"\n", dtype=np.uint8)]
        pos += len(names[i]) + 1 + L + 3 + L + 1
    block = np.concatenate(parts)
    assert block.size == pos
    return block, idx
