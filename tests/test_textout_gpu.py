"""-m gpu: the output side of libtgsf_text.so, the HIP build, on a real MI355X -- the checks of tests/test_textout_emul.py
again with larger counts, the device form on a caller's stream, two objects on two threads, and an output of more than
4 GiB that equals its input."""
import numpy as np
import pytest

from tests import hostmodel, textoutparity as top, textparity
from tgsfilter_amd import abi, text as tgtext

pytestmark = pytest.mark.gpu


def test_gpu_abi_and_symbols():
    lib = tgtext.load()
    assert lib.tgsf_text_backend().startswith(b"hip") and lib.tgsf_text_abi_version() == 2
    for sym in tgtext.SYMBOLS:
        getattr(lib, sym)


@pytest.mark.parametrize("name", hostmodel.GOLDEN_CASES)
def test_gpu_golden_one_call(golden_dir, name):
    top.golden(None, None, golden_dir, name)


@pytest.mark.parametrize("mode", top.MODES)
@pytest.mark.parametrize("seed", sorted(top.SYNTH_SETS))
def test_gpu_synthetic_one_call(seed, mode):
    top.synthetic(None, None, seed, mode)


def test_gpu_many_fragments_of_one_read():
    top.many_fragments_of_one_read(None)


def test_gpu_names_and_short_records():
    top.names(None)


def test_gpu_long_read_among_short():
    top.long_read_among_short(None, n_short=300)


@pytest.mark.parametrize("fastq_out", [True, False])
def test_gpu_seam_sweep(fastq_out):
    top.seam_sweep(None, fastq_out)


def test_gpu_nothing_to_write():
    top.nothing_to_write(None)


def test_gpu_identity():
    top.identity(None, n=600)


def test_gpu_capacity_and_canaries():
    top.capacity_and_canaries(None, top.TorchDev())


def test_gpu_refusals_and_recovery():
    top.refusals(None, None, top.TorchDev(own_stream=False))


def test_gpu_device_form_on_a_callers_stream():
    top.device_form(None, None, top.TorchDev())


def test_gpu_two_objects_two_contexts_two_threads():
    from tgsfilter_amd import capi
    capi.load(), tgtext.load()
    top.two_threads(None, None, top.TorchDev)


def test_gpu_fuzz():
    assert top.fuzz(None, 3002, 3000, max_len=400) >= 3000


def test_gpu_identity_above_4_gib():
    """5 GiB of well-formed FASTQ resident in HBM, one whole-read PASS fragment per read, the tables made on the device: the
    output equals the text.  Then one fragment behind the 4 GiB mark loses its PASS: the text without that record."""
    import torch
    dev = torch.device("cuda", 0)
    block, bidx = textparity.full_size_block()
    per, period = len(bidx["len"]), block.size
    reps = (5 << 30) // period + 1
    n_bytes, nrec = reps * period, reps * per
    d_text = torch.from_numpy(block).to(dev).repeat(reps)
    tx = tgtext.TextIndexer(0, n_bytes, nrec, None)
    try:
        tx.reserve_output(nrec, 16)
        tx.index_device(n_bytes, d_text=d_text.data_ptr())
        _, s = tx.fetch(want_index=False)
        assert s["n_records"] == nrec and s["stop"] == tgtext.END
        # tgsf_read_result: 8 int32 words, frag_begin the fifth, n_frags the fourth; tgsf_fragment: 6 words, read, start, len, flags behind sum_q
        ar = torch.arange(nrec, dtype=torch.int32, device=dev)
        d_reads = torch.zeros((nrec, 8), dtype=torch.int32, device=dev)
        d_reads[:, 3], d_reads[:, 4] = 1, ar
        d_frags = torch.zeros((nrec, 6), dtype=torch.int32, device=dev)
        d_frags[:, 2], d_frags[:, 4], d_frags[:, 5] = ar, torch.from_numpy(bidx["len"].astype(np.int32)).to(dev).repeat(reps), abi.FF_PASS
        d_out = torch.full((n_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
        d_ends = torch.zeros(nrec, dtype=torch.int64, device=dev)
        d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        args = dict(d_text=d_text.data_ptr(), d_out=d_out.data_ptr(), out_capacity=n_bytes, d_rec_end=d_ends.data_ptr(), d_summary=d_sum.data_ptr())
        tx.format_device(nrec, d_reads.data_ptr(), d_frags.data_ptr(), nrec, **args)
        tx.fetch(want_index=False)                                      # (waits for the object's stream)
        sm = tgtext.OutSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
        assert (sm.n_bytes, sm.n_records, sm.stop) == (n_bytes, nrec, tgtext.END) and sm.n_bytes > 1 << 32
        assert sm.bases == int(bidx["len"].astype(np.uint64).sum()) * reps
        assert torch.equal(d_out[:n_bytes], d_text) and bool((d_out[n_bytes:] == 0xA5).all())
        ends = d_ends.cpu().numpy()
        starts = np.tile(bidx["name_off"].astype(np.int64) - 1, reps) + (np.arange(reps, dtype=np.int64) * period).repeat(per)
        assert np.array_equal(ends[:-1], starts[1:]) and int(ends[-1]) == n_bytes
        # one record behind the 4 GiB mark is not kept
        r = int(np.searchsorted(starts, (4 << 30) + 12345))
        a, b = int(starts[r]), int(ends[r])
        assert a > 4 << 30
        d_frags[r, 5] = 0
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        tx.format_device(nrec, d_reads.data_ptr(), d_frags.data_ptr(), nrec, **args)
        tx.fetch(want_index=False)
        sm = tgtext.OutSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
        assert (sm.n_bytes, sm.n_records, sm.stop) == (n_bytes - (b - a), nrec - 1, tgtext.END)
        assert torch.equal(d_out[:a], d_text[:a]) and torch.equal(d_out[a:sm.n_bytes], d_text[b:]) and bool((d_out[sm.n_bytes:] == 0xA5).all())
    finally:
        tx.close()
