"""The BAM input side of libtgsf_text on a GPU-less box: inflated unaligned BAM records decoded into FASTQ text and its index
by the serial emulation of the kernels (tests/emul/libtgsf_text_emul.so, every lane a wave of one), against the model of
tests/bammodel.py -- which is pinned here first, without the library, to the reference's own output files.
tests/test_bam_gpu.py repeats the checks on the HIP build."""
import os
import subprocess

import pytest

from tests import bammodel as bm, bamparity as bp, hostmodel, textoutparity as top, textparity
from tgsfilter_amd import text as tgtext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
REF = os.path.join(ROOT, "oracle", "_ref", "tgsfilter_ref")


@pytest.fixture(scope="module")
def libs():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    return os.path.join(EMUL_DIR, "libtgsf_emul.so"), os.path.join(EMUL_DIR, "libtgsf_text_emul.so")


@pytest.fixture(scope="module")
def tlib(libs):
    return libs[1]


# ---- the model, without the library ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bp.GOLDEN))
def test_model_equals_reference_output(golden_dir, name):
    """The model's text, filtered by the oracle and formatted by the output model, is the reference's own output file."""
    case, at, chunk, m = bp.golden_model(golden_dir, name)
    p = bp.golden_params(case, m)
    ix, er, ef = top.oracle_on_text(p, m["text"])
    for f in bm.FIELDS:
        assert (ix[f] == m["index"][f]).all(), f                                     # the text model's index of the decoded text
    assert top.format_records(m["text"], ix, er, ef, True)[0] == case.ref_out
    assert hostmodel.format_fastq(bm.reads_of(chunk), er, ef) == case.ref_out


# ---- the library -------------------------------------------------------------------------------------------------------
def test_abi_and_symbols(tlib):
    lib = tgtext.load(tlib)
    assert lib.tgsf_text_abi_version() == tgtext.ABI_VERSION == 2
    for sym in tgtext.SYMBOLS:
        getattr(lib, sym)
    assert "tgsf_text_bam_decode" in tgtext.SYMBOLS and "tgsf_text_bam_filter" in tgtext.SYMBOLS


@pytest.mark.parametrize("name", sorted(bp.GOLDEN))
def test_golden(libs, golden_dir, name):
    bp.golden(libs[0], libs[1], bp.HostMem(), golden_dir, name)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")
def test_reference_reads_a_bamio_file(libs, tmp_path):
    bp.bamio_against_reference(libs[0], libs[1], bp.HostMem(), REF, tmp_path)


def test_seams(tlib):
    bp.seams(tlib, bp.HostMem())


def test_piece_seams(tlib):
    bp.piece_seams(tlib, bp.HostMem())


def test_names_codes_qualities(libs):
    bp.names_codes_qualities(libs[0], libs[1], bp.HostMem())


def test_cut_everywhere(tlib):
    bp.cut_everywhere(tlib, bp.HostMem())


def test_irregular_records(tlib):
    bp.irregular_records(tlib, bp.HostMem())


def test_capacities_and_resuming(tlib):
    bp.capacities(tlib, bp.HostMem())


def test_refusals_and_recovery(libs):
    bp.refusals(libs[0], libs[1], bp.HostMem())


def test_device_form(tlib):
    bp.device_form(tlib, bp.HostMem(), n=12)


def test_fuzz(tlib):
    ran = bp.fuzz(tlib, bp.HostMem(), 4001, 240)
    assert sum(ran.values()) == 240 and all(ran[k] >= 24 for k in bp.KINDS), ran


def test_seams_and_cuts_under_address_sanitizer(tmp_path):
    """tests/manual/bam_asan.cpp includes the library's source built with -fsanitize=address,undefined: one stand-alone host
    program; nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    exe = os.path.join(EMUL_DIR, "bam_asan")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DTGSF_EMUL", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-x", "c++", os.path.join(ROOT, "tests", "manual", "bam_asan.cpp"), "-o", exe,
                    "-L" + EMUL_DIR, "-ltgsf_emul", "-Wl,-rpath,$ORIGIN"], check=True)
    p = subprocess.run([exe], capture_output=True, timeout=600)
    assert p.returncode == 0 and b"bam ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
