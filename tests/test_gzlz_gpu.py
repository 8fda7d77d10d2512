"""-m gpu: the match search of the BGZF output side of libtgsf_text.so (level 1, tgsf_text_bgzf_out_level), the HIP build, on a
real MI355X -- the checks of tests/test_gzlz_emul.py again, where the 64 positions of a round are the 64 lanes of a wave: they
look the table up together and insert together (two lanes may want one word), the one serial step reads their matches lane
by lane, their tokens meet in the words of the staging area (none of which a wave of one does).  Every step that feeds the
parse hand-made texts runs in a fresh child process under a time limit of its own."""

import os
import subprocess
import sys

import pytest

from tests import gzlzparity as lp, gzoutparity as zp
from tgsfilter_amd import text as tgtext

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpu_gzlz_symbols():
    lib = tgtext.load()
    assert lib.tgsf_text_backend().startswith(b"hip") and lib.tgsf_text_abi_version() == 2
    for sym in lp.NEW_SYMBOLS:
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)


# A parse that fails to end is then a failed test, not a hung suite: a child process a step, never the image of a process that
# has touched the GPU, under a limit that leaves room for the child's start-up.
STEP_SECONDS = 150
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS = {
    "interface": "lp.interface(None, zp.TorchMem(), %r)" % GOLDEN,
    "hifi_like_size": "lp.hifi_size(None, zp.TorchMem())",
    "far_matches": "lp.far_matches(None, zp.TorchMem())",
    "never_worse": "lp.never_worse(None, zp.TorchMem(), %r)" % GOLDEN,
    "match_geometry": "lp.match_geometry(None, zp.TorchMem())",
    "member_independence": "lp.independence(None, zp.TorchMem())",
    # (torch and then the library are brought up on the main thread first, as in a process that has run anything before its threads start)
    "two_levels_two_threads": "zp.TorchMem().sync(); tgtext.TextIndexer(0, 64, 1).close(); lp.two_levels_two_threads(None, zp.TorchMem)",
}


def run_step(code):
    """`code` in a child process; its standard output."""
    prog = "from tests import gzlzparity as lp, gzoutparity as zp\nfrom tgsfilter_amd import text as tgtext\n" + code + "\n"
    try:
        p = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        pytest.fail("the step did not end within %d s: a parse that does not terminate" % STEP_SECONDS)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout, end="")
    return p.stdout


@pytest.mark.parametrize("step", sorted(STEPS))
def test_gpu_step(step):
    run_step(STEPS[step])


def test_gpu_golden_filter_bgzf_at_level_1(golden_dir):
    lp.golden_filter_bgzf(None, None, golden_dir, "hifi_auto")


def test_gpu_golden_bam_bgzf_at_level_1(golden_dir):
    lp.golden_bam_bgzf(None, None, zp.TorchMem(own_stream=False), golden_dir, "hifi_bam")


def test_gpu_compressed_bytes_are_the_pinned_ones(golden_dir):
    lp.pinned_bytes(None, zp.TorchMem(own_stream=False), golden_dir)
