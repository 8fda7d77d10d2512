"""-m gpu: the BGZF output side of libtgsf_text.so, the HIP build, on a real MI355X -- the checks of tests/test_gzout_emul.py
again, where 64 lanes share a member: their slices' CRCs are combined, their codes meet in the words of the staging area, their
bit offsets come from the wave's prefix sum (none of which a wave of one does) -- on a caller's stream, with two objects on two
threads, and one chunk whose compressed output passes 4 GiB.  The steps that feed the coder hand-made distributions, and the
fuzz, each run in a child process under a time limit."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bamparity as bp, gzoutmodel as zm, gzoutparity as zp, hostmodel
from tgsfilter_amd import text as tgtext

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_gzout_symbols():
    lib = tgtext.load()
    assert lib.tgsf_text_backend().startswith(b"hip") and lib.tgsf_text_abi_version() == 2
    for sym in ("tgsf_text_bgzf_bound", "tgsf_text_bgzf_out_reserve", "tgsf_text_bgzf_deflate", "tgsf_text_bgzf_deflate_device", "tgsf_text_bgzf_crc_device",
                "tgsf_text_bgzf_verify", "tgsf_text_filter_bgzf", "tgsf_text_bam_filter_bgzf", "tgsf_text_bgzf_bam_filter_bgzf"):
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)


# Every step that feeds the kernels hand-made distributions runs in a fresh child process under a time limit of its own: a coder
# that fails to end is then a failed test, not a hung suite.  (The limit leaves room for the child's start-up.)
STEP_SECONDS = 150
STEPS = {
    "code_shapes": "zp.code_shapes(None, zp.TorchMem())",
    "bit_seams": "zp.bit_seams(None, zp.TorchMem())",
    "crc_against_zlib": "zp.crc_against_zlib(None, zp.TorchMem())",
    # (torch and then the library are brought up on the main thread first, as in a process that has run anything before its threads start)
    "two_objects_two_threads": "zp.TorchMem().sync(); tgtext.TextIndexer(0, 64, 1).close(); zp.two_threads(None, zp.TorchMem)",
}


def run_step(code):
    """`code` in a child process; its standard output."""
    prog = "from tests import gzoutparity as zp\nfrom tgsfilter_amd import text as tgtext\n" + code + "\n"
    try:
        p = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        pytest.fail("the step did not end within %d s: a coder that does not terminate" % STEP_SECONDS)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("step", sorted(STEPS))
def test_gpu_step(step):
    run_step(STEPS[step])


@pytest.mark.parametrize("seed", (6002, 6003))
def test_gpu_fuzz(seed):
    out = run_step("print('stored', zp.fuzz(None, zp.TorchMem(), %d, 60))" % seed)
    assert int(out.split("stored")[1].split()[0]) >= 3


def test_gpu_lengths_on_a_callers_stream():
    mem = zp.TorchMem()
    assert mem.stream is not None
    zp.lengths(None, mem)


def test_gpu_address_seams_and_capacity():
    zp.address_seams(None, zp.TorchMem(own_stream=False))


@pytest.mark.parametrize("name", zp.GOLDEN_TEXTS)
def test_gpu_golden_size(golden_dir, name):
    zp.golden_size(None, zp.TorchMem(own_stream=False), golden_dir, name)


@pytest.mark.parametrize("name", hostmodel.GOLDEN_CASES)
def test_gpu_golden_filter_bgzf(golden_dir, name):
    zp.golden_filter_bgzf(None, None, golden_dir, name)


@pytest.mark.parametrize("name", sorted(bp.GOLDEN))
def test_gpu_golden_bam_bgzf(golden_dir, name):
    zp.golden_bam_bgzf(None, None, zp.TorchMem(own_stream=False), golden_dir, name)


def test_gpu_refusals_and_recovery():
    zp.refusals(None, None, zp.TorchMem(own_stream=False))


def test_gpu_verify():
    zp.verify(None, zp.TorchMem(own_stream=False))


def test_gpu_output_above_4_gib():
    """One chunk of 65 800 members of random bytes made on the device: they do not compress, so every member is stored and the
    output has 31 bytes more a member than the 4.0 GiB that go in: its offsets pass 2^32.  Checked on the device: the framing
    words by their arithmetic, the bytes by the device inflate and its CRC check, canaries on both sides."""
    import torch
    mem = zp.TorchMem(own_stream=False)
    members, M = 65800, zm.MEMBER
    n = members * M - 12345                                             # (the last member is a short one)
    need = n + 31 * members + 28
    assert need > 1 << 32 and need == zm.bound(n, True)
    gen = torch.Generator(device=mem.dev)
    gen.manual_seed(64)
    d_in = torch.randint(0, 256, (n,), dtype=torch.uint8, device=mem.dev, generator=gen)
    d_out = torch.empty(16 + need + 16, dtype=torch.uint8, device=mem.dev)
    d_out[:16] = 0xA5
    d_out[-16:] = 0xA5
    d_end = torch.zeros(members + 1, dtype=torch.int64, device=mem.dev)
    d_sum = torch.zeros(40, dtype=torch.uint8, device=mem.dev)
    d_back = torch.empty(n + 16, dtype=torch.uint8, device=mem.dev)
    d_back[-16:] = 0xA5
    d_bad = torch.zeros(4, dtype=torch.int32, device=mem.dev)
    d_gsum = torch.zeros(40, dtype=torch.uint8, device=mem.dev)
    tx = tgtext.TextIndexer(0, 4096, 16, None)
    try:
        tx.reserve_bgzf_out(n, 16)
        tx.reserve_bgzf(need, members + 1)
        torch.cuda.synchronize()
        tx.deflate_device(n, True, d_in=d_in.data_ptr(), d_out=d_out.data_ptr() + 16, out_capacity=need, d_member_end=d_end.data_ptr(), d_summary=d_sum.data_ptr())
        tx.fetch(want_index=False)                                      # (waits for the object's stream)
        s = tgtext.GzOutSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes()).as_dict()
        assert (s["in_bytes"], s["n_bytes"], s["n_members"], s["stored"], s["stop"]) == (n, need, members + 1, members, zm.END), s
        ends = d_end.cpu().numpy().astype(np.uint64)
        usize = np.full(members, M, np.uint64)
        usize[-1] = n - (members - 1) * M
        assert np.array_equal(ends[:-1], np.cumsum(usize + np.uint64(31))) and ends[-1] == need
        assert bool((d_out[:16] == 0xA5).all()) and bool((d_out[-16:] == 0xA5).all())
        assert d_out[16 + need - 28:16 + need].cpu().numpy().tobytes() == zm.EOF_MEMBER
        # back through the device inflate; the table is the walk's, written down from member_end
        blocks = np.zeros(members + 1, tgtext.BGZF_BLOCK_DTYPE)
        begins = np.concatenate([[np.uint64(0)], ends[:-1]])
        blocks["payload"] = begins + np.uint64(18)
        blocks["clen"] = (ends - begins - np.uint64(26)).astype(np.uint32)
        blocks["usize"] = np.concatenate([usize, [0]]).astype(np.uint32)
        blocks["out"] = np.concatenate([[0], np.cumsum(usize)]).astype(np.uint64)
        tx.inflate_device(need, blocks, zm.END, d_back.data_ptr(), n, d_gz=d_out.data_ptr() + 16, d_summary=d_gsum.data_ptr())
        tx.crc_device(blocks, d_bad.data_ptr(), d_gz=d_out.data_ptr() + 16, d_inflated=d_back.data_ptr())
        tx.fetch(want_index=False)
        g = tgtext.BgzfSummary.from_buffer_copy(d_gsum.cpu().numpy().tobytes()).as_dict()
        assert (g["n_blocks"], g["out_bytes"], g["bad_block"]) == (members + 1, n, tgtext.NO_BAD_BLOCK), g
        assert torch.equal(d_back[:n], d_in) and bool((d_back[-16:] == 0xA5).all())
        assert int(d_bad[0].item()) == -1                               # UINT32_MAX: every CRC is right
    finally:
        tx.close()
