"""-m gpu: what tgsf_text_submit, tgsf_text_filter, tgsf_text_bam_submit and tgsf_text_bam_filter leave in the caller's
memory, on success and on every way they end early, on the HIP build (the cases of tests/test_textcalls_emul.py)."""
import pytest

from tests import textcalls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    r = textcalls.Rig(None, None)
    yield r
    r.close()


@pytest.mark.parametrize("case,call", textcalls.LEGS)
def test_gpu_text_calls(rig, case, call):
    textcalls.run(rig, case, call)
