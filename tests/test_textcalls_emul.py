"""What tgsf_text_submit, tgsf_text_filter, tgsf_text_bam_submit and tgsf_text_bam_filter leave in the caller's memory, on
success and on every way they end early, on the serial emulation of the kernels (tests/textcalls.py holds the cases;
tests/test_textcalls_gpu.py runs them on the HIP build)."""
import os
import subprocess

import pytest

from tests import textcalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")


@pytest.fixture(scope="module")
def rig():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    r = textcalls.Rig(os.path.join(EMUL_DIR, "libtgsf_emul.so"), os.path.join(EMUL_DIR, "libtgsf_text_emul.so"))
    yield r
    r.close()


@pytest.mark.parametrize("case,call", textcalls.LEGS)
def test_emul_text_calls(rig, case, call):
    textcalls.run(rig, case, call)
