"""-m gpu: the pre-pass on the HIP build (tests/prepass_domain.py holds the builders, the model and the checks and says why;
tests/test_prepass_emul.py runs all of it on the emulation first).  Here: tgsf_align_windows as the pre-pass calls it -- a wave
whose lanes hold the 22 different adapter lengths, which the one-lane emulation cannot show -- with the one call of the command
line's own size, and the real binary on the committed goldens, the 22 entries at the 5' end, the 4 096-ends call seam and the
depth seams.  The live cases take the reference binary from oracle/_ref/ and skip without it."""
import os

import pytest

from tests import prepass_domain as pd

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not os.path.exists(pd.REF), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")


@pytest.mark.parametrize("min_sim", pd.SIMS)
def test_gpu_library_shaped_alignments(min_sim):
    assert pd.check_windows(None, min_sim) > 50000


def test_gpu_one_call_of_the_products_size():
    pd.check_product_sized_call(None)


@pytest.mark.parametrize("name", sorted(pd.GOLDENS))
def test_gpu_golden(name):
    pd.check_golden(pd.GPU_CLI, name)


@needs_ref
@pytest.mark.parametrize("a", range(22))
def test_gpu_entry_at_the_5p_end(a):
    case = pd.five_case(a, 3)
    pd.live(pd.GPU_CLI, case, pd.adapter_check(case))


@needs_ref
@pytest.mark.parametrize("i,j", pd.CALL_SEAMS)
def test_gpu_call_seam(i, j):
    case = pd.call_seam_case(i, j)
    pd.live(pd.GPU_CLI, case, pd.adapter_check(case))


@needs_ref
@pytest.mark.parametrize("below", (False, True), ids=("on", "below"))
@pytest.mark.parametrize("S", pd.DEPTH_SIMS)
@pytest.mark.parametrize("a", pd.DEPTH_ENTRIES)
def test_gpu_depth_seam(a, S, below):
    case = pd.depth_case(a, S, below)
    pd.live(pd.GPU_CLI, case, pd.adapter_check(case))
