"""-m gpu: the BAM input side of libtgsf_text.so, the HIP build, on a real MI355X -- the checks of tests/test_bam_emul.py
again with larger counts, the device form on a caller's stream, two objects on two threads, and a chunk of more than 4 GiB
of BAM whose text has more than 5 GiB."""

import numpy as np
import pytest

from tests import bammodel as bm, bamparity as bp
from tgsfilter_amd import text as tgtext

pytestmark = pytest.mark.gpu


def test_gpu_bam_symbols():
    lib = tgtext.load()
    assert lib.tgsf_text_backend().startswith(b"hip") and lib.tgsf_text_abi_version() == 2
    for sym in ("tgsf_text_bam_header", "tgsf_text_bam_walk", "tgsf_text_bam_reserve", "tgsf_text_bam_decode", "tgsf_text_bam_decode_device",
                "tgsf_text_bam_submit", "tgsf_text_bam_filter"):
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)


@pytest.mark.parametrize("name", sorted(bp.GOLDEN))
def test_gpu_golden(golden_dir, name):
    bp.golden(None, None, bp.TorchMem(), golden_dir, name)


def test_gpu_seams():
    bp.seams(None, bp.TorchMem())


def test_gpu_piece_seams():
    bp.piece_seams(None, bp.TorchMem(), n_short=300)


def test_gpu_names_codes_qualities():
    bp.names_codes_qualities(None, None, bp.TorchMem())


def test_gpu_cut_everywhere():
    bp.cut_everywhere(None, bp.TorchMem())


def test_gpu_irregular_records():
    bp.irregular_records(None, bp.TorchMem())


def test_gpu_capacities_and_resuming():
    bp.capacities(None, bp.TorchMem())


def test_gpu_refusals_and_recovery():
    bp.refusals(None, None, bp.TorchMem(own_stream=False))


def test_gpu_device_form_on_a_callers_stream():
    bp.device_form(None, bp.TorchMem(), n=400)


def test_gpu_two_objects_two_threads():
    tgtext.load()
    bp.two_threads(None, bp.TorchMem)


def test_gpu_fuzz():
    ran = bp.fuzz(None, bp.TorchMem(), 4002, 1200, max_len=400)
    assert sum(ran.values()) == 1200 and all(ran[k] >= 120 for k in bp.KINDS), ran


def test_gpu_offsets_above_4_gib():
    """A block of 300 records repeated in HBM to just over 4 GiB of BAM (over 5 GiB of text), the record offsets in closed
    form: the text is the block's text repeated, the index its closed form.  Then l_seq = 0 in one record behind the 4 GiB
    mark: n_records and consumed stop exactly there."""
    import torch
    mem = bp.TorchMem(own_stream=False)
    dev = mem.dev
    rng = np.random.default_rng(109)
    recs = [bp.rnd_record(rng, 10 + i % 9, int(rng.integers(8000, 22000)), aux=i % 17, qmax=94) for i in range(300)]
    block = np.frombuffer(b"".join(recs), np.uint8)
    per, period = len(recs), block.size
    bmod = bm.rule(block.tobytes(), True, per, 1 << 40)
    assert (bmod["stop"], bmod["n_records"]) == (bm.END, per)
    tperiod = bmod["text_bytes"]
    reps = (4 << 30) // period + 2
    n_bytes, nrec, text_bytes = reps * period, reps * per, reps * tperiod
    assert n_bytes > 4 << 30 and text_bytes > 5 << 30
    boff = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    rec_off = np.concatenate([np.tile(boff, reps) + (np.arange(reps, dtype=np.uint64) * np.uint64(period)).repeat(per), np.array([n_bytes], np.uint64)])
    d_bam = torch.from_numpy(block.copy()).to(dev).repeat(reps)
    d_want = torch.from_numpy(np.frombuffer(bmod["text"], np.uint8).copy()).to(dev).repeat(reps)
    tx = tgtext.TextIndexer(0, text_bytes + 100, nrec, None)
    try:
        tx.reserve_bam(n_bytes)
        b = tx.buffers()
        d_sum = torch.zeros(48, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def decode():
            tx.bam_decode_device(n_bytes, rec_off, bm.END, d_bam=d_bam.data_ptr(), d_summary=d_sum.data_ptr())
            tx.fetch(want_index=False)                                  # (waits for the object's stream)
            return tgtext.BamSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes()).as_dict()

        def index(f, k):
            w = 4 if f in ("len", "name_len") else 8
            return mem.peek(getattr(b.index, f), k * w).view(np.uint32 if w == 4 else np.uint64)

        def closed(f, k):
            a = np.tile(bmod["index"][f], reps)
            if f not in ("len", "name_len"):
                a = a + (np.arange(reps, dtype=np.uint64) * np.uint64(tperiod)).repeat(per)
            return a[:k]

        s = decode()
        assert (s["n_records"], s["stop"], s["consumed"], s["text_bytes"], s["bad_qual"]) == (nrec, bm.END, n_bytes, text_bytes, bm.NO_BAD_QUAL), s
        assert s["bases"] == bmod["bases"] * reps and s["longest"] == bmod["longest"]
        got = mem._view(b.text, text_bytes + tgtext.PAD)
        assert torch.equal(got[:text_bytes], d_want) and not bool(got[text_bytes:].any())
        for f in bm.FIELDS:
            assert np.array_equal(index(f, nrec), closed(f, nrec)), f
        # one record behind the 4 GiB mark loses its sequence
        r = int(np.searchsorted(rec_off, np.uint64((4 << 30) + 12345)))
        at = int(rec_off[r])
        assert at > 4 << 30 and r < nrec
        d_bam[at + 20:at + 24] = 0
        torch.cuda.synchronize()
        s = decode()
        cut = int(closed("name_off", r + 1)[r]) - 1
        assert (s["n_records"], s["stop"], s["consumed"], s["text_bytes"]) == (r, bm.IRREGULAR, at, cut) and cut > 5 << 30, (s, r, at, cut)
        got = mem._view(b.text, cut + tgtext.PAD)
        assert torch.equal(got[:cut], d_want[:cut]) and not bool(got[cut:].any())
        for f in bm.FIELDS:
            assert np.array_equal(index(f, r), closed(f, r)), f
    finally:
        tx.close()
