"""The output side of libtgsf_text on a GPU-less box: the kept records formatted as FASTQ / FASTA text by the serial
emulation of the kernels (tests/emul/libtgsf_text_emul.so, every lane a wave of one), against the model of
tests/textoutparity.py -- which is pinned here first, without the library, against tests/hostmodel.py and the reference
binary's own output files.  tests/test_textout_gpu.py repeats the checks on the HIP build."""
import os
import subprocess

import pytest

from tests import hostmodel, textoutparity as top, textparity
from tgsfilter_amd import text as tgtext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")


@pytest.fixture(scope="module")
def libs():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    return os.path.join(EMUL_DIR, "libtgsf_emul.so"), os.path.join(EMUL_DIR, "libtgsf_text_emul.so")


@pytest.fixture(scope="module")
def tlib(libs):
    return libs[1]


# ---- the model, without the library ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sorted(top.SYNTH_SETS))
def test_model_equals_hostmodel(seed):
    kind, reads, text, fasta, fastq_out, p = top.synth_case(seed, "fastq_fastq")
    ix, er, ef = top.oracle_on_text(p, text)
    out, ends = top.format_records(text, ix, er, ef, True)
    assert out == hostmodel.format_fastq(reads, er, ef) and len(ends) == out.count(b"\n") // 4 and int(ends[-1]) == len(out)
    assert top.reads_with_two_pass(ef) >= 10
    crlf = textparity.fastq_of(reads, b"\r\n")
    assert top.format_records(crlf, top.index_of(crlf), er, ef, True)[0] == out        # line ends are '\n' whatever the input used


@pytest.mark.parametrize("name", hostmodel.GOLDEN_CASES)
def test_model_equals_reference_output(golden_dir, name):
    case = hostmodel.GoldenCase(golden_dir, name)
    text = textparity.fastq_of(case.reads)
    p = case.params()
    p.max_read_len = max(len(r[1]) for r in case.reads)
    ix, er, ef = top.oracle_on_text(p, text)
    assert top.format_records(text, ix, er, ef, True)[0] == case.ref_out
    assert (name == "qc_only") == (case.ref_out == b"")


# ---- the library -------------------------------------------------------------------------------------------------------
def test_abi_and_symbols(tlib):
    lib = tgtext.load(tlib)
    assert lib.tgsf_text_abi_version() == tgtext.ABI_VERSION == 2
    for sym in tgtext.SYMBOLS:
        getattr(lib, sym)


@pytest.mark.parametrize("name", hostmodel.GOLDEN_CASES)
def test_golden_one_call(libs, golden_dir, name):
    top.golden(libs[0], libs[1], golden_dir, name)


@pytest.mark.parametrize("mode", top.MODES)
@pytest.mark.parametrize("seed", sorted(top.SYNTH_SETS))
def test_synthetic_one_call(libs, seed, mode):
    top.synthetic(libs[0], libs[1], seed, mode)


def test_many_fragments_of_one_read(tlib):
    top.many_fragments_of_one_read(tlib)


def test_names_and_short_records(tlib):
    top.names(tlib)


def test_long_read_among_short(tlib):
    top.long_read_among_short(tlib)


@pytest.mark.parametrize("fastq_out", [True, False])
def test_seam_sweep(tlib, fastq_out):
    top.seam_sweep(tlib, fastq_out)


def test_nothing_to_write(tlib):
    top.nothing_to_write(tlib)


def test_identity(tlib):
    top.identity(tlib)


def test_capacity_and_canaries(tlib):
    top.capacity_and_canaries(tlib, top.HostDev())


def test_refusals_and_recovery(libs):
    top.refusals(libs[0], libs[1], top.HostDev())


def test_device_form(libs):
    top.device_form(libs[0], libs[1], top.HostDev(), n=30)


def test_fuzz(tlib):
    assert top.fuzz(tlib, 3001, 300) >= 300
