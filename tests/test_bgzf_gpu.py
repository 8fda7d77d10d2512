"""-m gpu: the BGZF input side of libtgsf_text.so, the HIP build, on a real MI355X -- the checks of tests/test_bgzf_emul.py
again, where 64 lanes copy side by side and a match reads what other lanes stored (the fence the emulation cannot check), with
larger counts, the device form on a caller's stream, two objects on two threads, and a chunk that inflates past 4 GiB.  The steps
that feed the decoder damaged streams each run in a child process under a time limit."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bgzfmodel as gm, bgzfparity as gp
from tgsfilter_amd import text as tgtext

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_bgzf_symbols():
    lib = tgtext.load()
    assert lib.tgsf_text_backend().startswith(b"hip") and lib.tgsf_text_abi_version() == 2
    for sym in ("tgsf_text_bgzf_walk", "tgsf_text_bgzf_reserve", "tgsf_text_bgzf_inflate", "tgsf_text_bgzf_inflate_device", "tgsf_text_bam_walk_device",
                "tgsf_text_bgzf_bam_decode", "tgsf_text_bgzf_bam_submit", "tgsf_text_bgzf_bam_filter"):
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)


# Every step that feeds the kernel damaged or hand-made streams runs in a fresh child process under a time limit of its own: a
# decoder that fails to end is then a failed test, not a hung suite.  (The limit leaves room for the child's start-up.)
STEP_SECONDS = 150
STEPS = {
    "stored_blocks": "gp.stored(None, gp.TorchMem())",
    "fixed_code": "gp.fixed_code(None, gp.TorchMem())",
    "copies": "gp.copies(None, gp.TorchMem())",
    "dynamic_headers": "gp.dynamic_headers(None, gp.TorchMem())",
    "what_zlib_writes": "gp.zlib_streams(None, gp.TorchMem())",
    "several_members": "gp.several_members(None, gp.TorchMem())",
    "damage": "gp.damage(None, gp.TorchMem())",
    "compressed_seams": "gp.compressed_seams(None, None, gp.TorchMem(own_stream=False))",
    # (torch and then the library are brought up on the main thread first, as in a process that has run anything before its threads start)
    "two_objects_two_threads": "gp.TorchMem().sync(); tgtext.TextIndexer(0, 64, 1).close(); gp.two_threads(None, gp.TorchMem)",
}


def run_step(code):
    """`code` in a child process; its standard output."""
    prog = "from tests import bgzfparity as gp\nfrom tgsfilter_amd import text as tgtext\n" + code + "\n"
    try:
        p = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        pytest.fail("the step did not end within %d s: a decoder that does not terminate" % STEP_SECONDS)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return p.stdout


@pytest.mark.parametrize("step", sorted(STEPS))
def test_gpu_step(step):
    run_step(STEPS[step])


@pytest.mark.parametrize("seed", (5002, 5003))
def test_gpu_fuzz(seed):
    out = run_step("print('flips', *gp.fuzz(None, gp.TorchMem(), %d, 200, max_size=20000))" % seed)
    broke, kept = (int(x) for x in out.split("flips")[1].split()[:2])
    assert broke + kept == 100 and broke >= 10 and kept >= 5, (broke, kept)


def test_gpu_into_the_text_index(golden_dir):
    gp.into_the_text_index(None, gp.TorchMem(own_stream=False), golden_dir)


def test_gpu_refusals_and_recovery():
    gp.refusals(None, gp.TorchMem(own_stream=False))


def test_gpu_device_walk():
    gp.device_walk(None, gp.TorchMem(own_stream=False))


@pytest.mark.parametrize("name", sorted(gp.bp.GOLDEN))
def test_gpu_golden_compressed(golden_dir, name):
    gp.golden_compressed(None, None, gp.TorchMem(own_stream=False), golden_dir, name)


def test_gpu_offsets_above_4_gib():
    """One chunk of 65 600 members of 65536 bytes, member b filled with byte (7 * b) & 255: about 5 MB in, 4.1 GiB out, so the
    output offsets pass 2^32; compared on the device."""
    import torch
    mem = gp.TorchMem(own_stream=False)
    n = 65600
    members = [gm.zmember(bytes([v]) * 65536) for v in range(256)]
    gz = b"".join(members[(7 * b) & 255] for b in range(n))
    tx = tgtext.TextIndexer(0, 4096, 16, None)
    try:
        tx.reserve_bgzf(len(gz), n)
        blocks, stop, consumed, out_bytes = tgtext.bgzf_walk(gz, n)
        assert (len(blocks), stop, consumed, out_bytes) == (n, gm.END, len(gz), n * 65536) and out_bytes > 1 << 32
        d_gz = mem.put(np.frombuffer(gz + bytes(-len(gz) % 16), np.uint8))
        d_out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=mem.dev)
        d_out[-16:] = 0xA5
        d_sum = torch.zeros(40, dtype=torch.uint8, device=mem.dev)
        torch.cuda.synchronize()
        tx.inflate_device(len(gz), blocks, stop, d_out.data_ptr(), out_bytes, d_gz=d_gz.data_ptr(), d_summary=d_sum.data_ptr())
        tx.fetch(want_index=False)                                      # (waits for the object's stream)
        s = tgtext.BgzfSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes()).as_dict()
        assert (s["n_blocks"], s["stop"], s["consumed"], s["out_bytes"], s["bad_block"]) == (n, gm.END, len(gz), out_bytes, gm.NONE), s
        want = ((torch.arange(n, device=mem.dev, dtype=torch.int64) * 7) & 255).to(torch.uint8)
        assert torch.equal(d_out[:out_bytes].view(n, 65536), want[:, None].expand(n, 65536))
        assert bool((d_out[-16:] == 0xA5).all())
    finally:
        tx.close()
