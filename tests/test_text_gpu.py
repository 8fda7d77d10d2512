"""-m gpu: libtgsf_text.so, the HIP build, on a real MI355X -- the checks of tests/test_text_emul.py again with larger
counts, the device form end to end, two objects driven from two threads, and one text of more than 4 GiB whose index
is known in closed form."""
import threading

import numpy as np
import pytest

from oracle import orc
from tests import parity, textmodel, textparity
from tgsfilter_amd import abi, capi, synth, text as tgtext

pytestmark = pytest.mark.gpu


def test_backend_is_hip():
    assert tgtext.load().tgsf_text_backend().startswith(b"hip")


@pytest.mark.parametrize("kind", ["ont", "hifi"])
def test_gpu_well_formed(kind):
    reads = synth.make_reads(3, 400, kind, mean_len=4000, zoo=True)
    for eol in (b"\n", b"\r\n"):
        recs, _, stop = textparity.check_text(None, textparity.fastq_of(reads, eol))
        assert len(recs) == len(reads) and stop == tgtext.END
        recs, _, stop = textparity.check_text(None, textparity.fasta_of(reads, eol), fasta=True)
        assert len(recs) == len(reads) and stop == tgtext.END
    text = textparity.fastq_of(reads)
    recs, consumed, stop = textparity.check_text(None, text[:-1])
    assert len(recs) == len(reads) and consumed == len(text) - 1 and stop == tgtext.END
    recs, consumed, stop = textparity.check_text(None, text[:-1], final=False)
    assert len(recs) == len(reads) - 1 and stop == tgtext.END


def test_gpu_unusual_texts():
    for i, text in enumerate(textparity.unusual_texts()):
        textparity.check_text(None, text, what=i)


def test_gpu_every_damage_class():
    stops = set()
    for damage, fasta, text in textparity.damaged_texts(per_class=40):
        for final in (True, False):
            stops.add(textparity.check_text(None, text, fasta=fasta, final=final, what=(damage, fasta, final, text))[2])
    assert stops == {tgtext.END, tgtext.IRREGULAR}


def test_gpu_lines_longer_than_a_piece_and_a_block():
    reads = textparity.long_line_text(n_short=300)
    recs, _, stop = textparity.check_text(None, textparity.fastq_of(reads))
    assert len(recs) == len(reads) and stop == tgtext.END
    textparity.check_text(None, textparity.fasta_of(reads), fasta=True)


def test_gpu_no_newline_and_empty():
    for text in (b"", b"@", b"A" * 10000, b"\n", b"\n" * 9000, b"\r\n\r\n", b"@a\nA\n+\nI"):
        for fasta in (False, True):
            for final in (True, False):
                textparity.check_text(None, text, fasta=fasta, final=final, what=(text[:20], fasta, final))


def test_gpu_more_scan_blocks_than_one():
    reads = synth.make_reads(9, 300, "ont", mean_len=3000, zoo=False)
    block = textparity.fastq_of(reads)
    text = block * (40_000_000 // len(block) + 1)
    recs, _, stop = textparity.check_text(None, text)
    assert len(recs) == 300 * (40_000_000 // len(block) + 1) and stop == tgtext.END


def test_gpu_capacity_then_the_rest():
    reads = synth.make_reads(4, 203, "ont", mean_len=500, zoo=False)
    textparity.capacity_then_rest(None, textparity.fastq_of(reads), False, 50)
    textparity.capacity_then_rest(None, textparity.fasta_of(reads[:200]), True, 50)
    textparity.capacity_then_rest(None, textparity.fastq_of(reads) + b"@x\n\n", False, 203)


def test_gpu_cut_at_every_byte():
    rng = np.random.default_rng(17)
    textparity.cut_everywhere(None, textmodel.make_text(rng, False, n_records=5, max_len=30), False)
    textparity.cut_everywhere(None, textmodel.make_text(rng, False, n_records=4, damage="crlf", max_len=30), False)
    textparity.cut_everywhere(None, textmodel.make_text(rng, True, n_records=6, max_len=30), True)
    textparity.cut_everywhere(None, textmodel.make_text(rng, False, n_records=5, damage="no_final_newline", max_len=30), False)


def test_gpu_fuzz():
    n = 6000
    assert textparity.fuzz(None, 2001, n, max_len=400) >= n // 4


# ---- the one-call form ---------------------------------------------------------------------------------------------
def test_gpu_chained_ont():
    reads = synth.make_reads(31, 300, "ont", mean_len=3000, zoo=True, pmid=0.1)
    textparity.chained(None, None, "ont", reads, min_q=9.0, head_trim=5, tail_trim=3)


def test_gpu_chained_hifi():
    reads = synth.make_reads(32, 200, "hifi", mean_len=5000, zoo=True, pmid=0.3)
    textparity.chained(None, None, "hifi", reads, min_q=20.0)


def test_gpu_chained_fasta_no_qual():
    reads = synth.make_reads(33, 300, "ont", mean_len=3000, zoo=True, pmid=0.1)
    textparity.chained(None, None, "ont", reads, fasta=True, min_q=9.0)


def test_gpu_chained_garbage_in_the_padding():
    reads = synth.make_reads(34, 100, "ont", mean_len=2000, zoo=True, pmid=0.1)
    textparity.chained(None, None, "ont", reads, garbage_in_padding=True, min_q=9.0)


def test_gpu_chained_irregular_tail():
    textparity.irregular_tail(None, None)


def test_gpu_chained_refusals():
    textparity.refusals(None, None)


# ---- the device form -----------------------------------------------------------------------------------------------
def test_gpu_device_form_end_to_end():
    """Text up into the object's buffer, tgsf_text_index_device with d_index = NULL, tgsf_submit_device straight from the
    object's arrays: no index ever on the host.  Then the same index from a caller's buffer with garbage behind n_bytes."""
    import torch
    dev = torch.device("cuda", 0)
    reads = synth.make_reads(41, 300, "ont", mean_len=3000, zoo=True, pmid=0.1)
    padded, off, qoff, ln = parity.fastq_text_layout(reads)
    text = padded[:-64].tobytes()
    n = len(reads)
    p = textparity.params_for("ont", reads, len(text), min_q=9.0)
    ctx = capi.Context(p, 0)
    tx = tgtext.TextIndexer(0, len(text), n, None)
    try:
        assert tx.upload(text) == len(text)
        tx.index_device(len(text))
        _, s = tx.fetch(want_index=False)                        # the one small copy: n_records
        assert s["n_records"] == n and s["stop"] == tgtext.END and s["consumed"] == len(text)
        b = tx.buffers()
        assert b.text % 16 == 0 and b.max_records == n
        fcap = len(text) // 100 + n + 16
        d_reads = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_frags = torch.zeros(fcap * 24, dtype=torch.uint8, device=dev)
        d_nf = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.submit_device(b.text, b.text, b.index.seq_off, b.index.len, s["n_records"], len(text), d_reads.data_ptr(),
                          d_frags.data_ptr(), fcap, d_nf.data_ptr(), None, d_qual_offsets=b.index.qual_off)
        ctx.wait()
        got_r = d_reads.cpu().numpy().view(abi.READ_RESULT_DTYPE)
        got_f = d_frags.cpu().numpy().view(abi.FRAGMENT_DTYPE)[:int(d_nf[0].item())]
        exp_r, exp_f, exp_c = orc.filter_batch(p, padded, padded, off, ln, n_bins=ctx.n_bins, qual_offsets=qoff)
        textparity.same_results((got_r, got_f, ctx.counters()), (exp_r, exp_f, exp_c))
        # a caller's buffer, a caller's stream, a caller's index arrays; a whole record of garbage behind n_bytes
        tail = b"\n@x\nAC\n+\nII\n" + b"\xff" * 60
        d_text = torch.from_numpy(np.frombuffer(text + tail, dtype=np.uint8).copy()).to(dev)
        arrs = [torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(5)]
        d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        ia = tgtext.IndexArrays(*[a.data_ptr() for a in arrs])
        tx.index_device(len(text) - 1, d_text=d_text.data_ptr(), d_index=ia, d_summary=d_sum.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        sm = tgtext.Summary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
        assert (sm.n_records, sm.stop, sm.consumed) == (n, tgtext.END, len(text) - 1)            # the last '\n' is behind n_bytes: a tail line
        assert np.array_equal(arrs[0].cpu().numpy().view(np.uint64), off) and np.array_equal(arrs[1].cpu().numpy().view(np.uint64), qoff)
        assert np.array_equal(arrs[2].cpu().numpy().view(np.uint32)[:n], ln)
        tx.index_device(len(text) - 1, final=False, d_text=d_text.data_ptr(), d_index=ia, d_summary=d_sum.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        sm = tgtext.Summary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
        assert (sm.n_records, sm.stop) == (n - 1, tgtext.END)
    finally:
        tx.close()
        ctx.close()


def test_gpu_two_indexers_two_contexts_two_threads():
    """Two objects, two contexts, two host threads at the same time; every result against the oracle afterwards."""
    capi.load(), tgtext.load()
    sets = [synth.make_reads(51 + k, 250, "ont", mean_len=3000, zoo=True, pmid=0.1) for k in range(2)]
    texts = [textparity.fastq_of(rd) + b"@bad\n\n" for rd in sets]
    params = [textparity.params_for("ont", sets[k], len(texts[k]), min_q=9.0, head_trim=3 * k) for k in range(2)]
    results, errors = [[], []], []

    def work(k):
        try:
            ctx = capi.Context(params[k], 0)
            tx = tgtext.TextIndexer(0, len(texts[k]), len(sets[k]) + 4, None)
            for rep in range(4):
                ctx.reset_counters()
                idx, s, r, f = tx.submit(ctx, texts[k])
                results[k].append((idx, s, r, f, ctx.counters(), ctx.n_bins))
            tx.close()
            ctx.close()
        except BaseException as e:              # noqa: BLE001 -- reported by the asserting thread
            errors.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for k in range(2):
        padded, off, qoff, ln = parity.fastq_text_layout(sets[k])
        assert len(results[k]) == 4
        for idx, s, r, f, c, n_bins in results[k]:
            assert s["n_records"] == len(sets[k]) and s["stop"] == tgtext.IRREGULAR and s["consumed"] == len(texts[k]) - 6
            assert np.array_equal(idx.seq_off, off) and np.array_equal(idx.qual_off, qoff) and np.array_equal(idx.len, ln)
            textparity.same_results((r, f, c), orc.filter_batch(params[k], padded, padded, off, ln, n_bins=n_bins, qual_offsets=qoff))


# ---- full size -----------------------------------------------------------------------------------------------------
def test_gpu_text_above_4_gib():
    """5 GiB of text: a seeded block repeated (the expected index is the block's plus the period), every array, bases, longest,
    consumed, stop; then one irregular line planted behind the 4 GiB mark."""
    import torch
    dev = torch.device("cuda", 0)
    block, bidx = textparity.full_size_block()
    period = block.size
    reps = (5 << 30) // period + 1
    n_bytes, nrec = reps * period, reps * len(bidx["len"])
    assert n_bytes > 5 << 30
    d_text = torch.from_numpy(block).to(dev).repeat(reps)
    assert d_text.numel() == n_bytes and d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    tx = tgtext.TextIndexer(0, n_bytes, nrec + 8, None)
    try:
        tx.index_device(n_bytes, d_text=d_text.data_ptr())
        got, s = tx.fetch()
        shift = (np.arange(reps, dtype=np.uint64) * np.uint64(period)).repeat(len(bidx["len"]))
        assert s["n_records"] == nrec and s["stop"] == tgtext.END and s["consumed"] == n_bytes
        for f in ("seq_off", "qual_off", "name_off"):
            assert np.array_equal(getattr(got, f), np.tile(bidx[f], reps) + shift), f
        for f in ("len", "name_len"):
            assert np.array_equal(getattr(got, f), np.tile(bidx[f], reps)), f
        assert s["bases"] == int(bidx["len"].astype(np.uint64).sum()) * reps and s["longest"] == int(bidx["len"].max())
        assert int(got.seq_off[-1]) > 1 << 32
        # the '+' of one record behind the 4 GiB mark becomes '-': the index ends in front of that record
        r = int(np.searchsorted(np.tile(bidx["name_off"], reps) + shift, np.uint64((4 << 30) + 12345)))
        plus = int(got.qual_off[r]) - 2
        assert plus > 4 << 30 and int(d_text[plus].item()) == ord("+")
        d_text[plus] = ord("-")
        torch.cuda.synchronize()
        tx.index_device(n_bytes, d_text=d_text.data_ptr())
        got2, s2 = tx.fetch()
        assert s2["n_records"] == r and s2["stop"] == tgtext.IRREGULAR and s2["consumed"] == int(got.name_off[r]) - 1
        assert np.array_equal(got2.seq_off, got.seq_off[:r]) and np.array_equal(got2.len, got.len[:r])
        assert s2["bases"] == int(got.len[:r].astype(np.uint64).sum())
    finally:
        tx.close()
