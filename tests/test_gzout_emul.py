"""The BGZF output side of libtgsf_text on a GPU-less box: text deflated into BGZF members, and the CRC32 of input members,
by the serial emulation of the kernels (tests/emul/libtgsf_text_emul.so, every lane a wave of one) against the model of
tests/gzoutmodel.py, which asks zlib and gzip.  tests/test_gzout_gpu.py repeats the checks on the HIP build, where 64 lanes
share a member's bits."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bamparity as bp, cli_check, gzoutmodel as zm, gzoutparity as zp, hostmodel
from tgsfilter_amd import text as tgtext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
REF = os.path.join(ROOT, "oracle", "_ref", "tgsfilter_ref")
NEW_SYMBOLS = ("tgsf_text_bgzf_bound", "tgsf_text_bgzf_out_reserve", "tgsf_text_bgzf_deflate", "tgsf_text_bgzf_deflate_device", "tgsf_text_bgzf_crc_device",
               "tgsf_text_bgzf_verify", "tgsf_text_filter_bgzf", "tgsf_text_bam_filter_bgzf", "tgsf_text_bgzf_bam_filter_bgzf")


@pytest.fixture(scope="module")
def libs():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    return os.path.join(EMUL_DIR, "libtgsf_emul.so"), os.path.join(EMUL_DIR, "libtgsf_text_emul.so")


@pytest.fixture(scope="module")
def tlib(libs):
    return libs[1]


def test_abi_and_symbols(tlib):
    lib = tgtext.load(tlib)
    assert lib.tgsf_text_abi_version() == tgtext.ABI_VERSION == 2
    for sym in NEW_SYMBOLS:
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)
    assert tgtext.BGZF_MEMBER == zm.MEMBER == 0xFF00


def test_model_on_what_zlib_writes():
    """The model accepts bgzip's own layout written through zlib, and refuses each thing the rule forbids.  This one pins the
    model, not the library: it is the only test of this file that passes without the feature."""
    import struct
    import zlib
    from tests import bgzfmodel as gm
    rng = np.random.default_rng(300)
    text = zm.fastq_like(rng, zm.MEMBER + 700)
    gz = b"".join(gm.zmember(text[lo:hi]) for lo, hi in zm.cuts(len(text))) + zm.EOF_MEMBER
    assert zm.check(text, gz, True) == 0
    for bad, why in ((gz[:-28], "EOF"), (gz + b"\0", "behind"), (gz[:40] + bytes([gz[40] ^ 1]) + gz[41:], "inflate")):
        with pytest.raises((AssertionError, zlib.error)):
            zm.check(text, bad, True)
    first = struct.unpack_from("<H", gz, 16)[0] + 1
    wrong_crc = gz[:first - 8] + bytes([gz[first - 8] ^ 1]) + gz[first - 7:]
    with pytest.raises(AssertionError, match="trailer"):
        zm.check(text, wrong_crc, True)
    rnd = bytes(rng.integers(0, 256, 500).astype(np.uint8))          # the fixed code on random bytes: larger than one stored block
    fixed = gm.member(gm.Bits().fixed(list(rnd), 1).bytes(), 500, crc=zlib.crc32(rnd))
    with pytest.raises(AssertionError, match="over the bound"):
        zm.check(rnd, fixed, False)


def test_lengths(tlib):
    zp.lengths(tlib, zp.HostMem())


def test_code_shapes(tlib):
    zp.code_shapes(tlib, zp.HostMem())


def test_bit_seams(tlib):
    zp.bit_seams(tlib, zp.HostMem())


def test_address_seams_and_capacity(tlib):
    zp.address_seams(tlib, zp.HostMem())


@pytest.mark.parametrize("name", zp.GOLDEN_TEXTS)
def test_golden_size(tlib, golden_dir, name):
    zp.golden_size(tlib, zp.HostMem(), golden_dir, name)


def test_fuzz(tlib):
    assert zp.fuzz(tlib, zp.HostMem(), 6001, 120) >= 5                 # (stored members among them)


@pytest.mark.parametrize("name", hostmodel.GOLDEN_CASES)
def test_golden_filter_bgzf(libs, golden_dir, name):
    zp.golden_filter_bgzf(libs[0], libs[1], golden_dir, name)


@pytest.mark.parametrize("name", sorted(bp.GOLDEN))
def test_golden_bam_bgzf(libs, golden_dir, name):
    zp.golden_bam_bgzf(libs[0], libs[1], zp.HostMem(), golden_dir, name)


def test_refusals_and_recovery(libs):
    zp.refusals(libs[0], libs[1], zp.HostMem())


def test_crc_against_zlib(tlib):
    zp.crc_against_zlib(tlib, zp.HostMem())


def test_verify(tlib):
    zp.verify(tlib, zp.HostMem())


def _cli_reads_what_the_emulation_wrote(binary, tlib, golden_dir, name="ont_auto"):
    """The golden's input text, deflated by the emulation into x.fq.gz, through a command line as -i: the golden's output."""
    case = hostmodel.GoldenCase(golden_dir, name)
    text = zp.textparity.fastq_of(case.reads)
    tx = tgtext.TextIndexer(0, 64, 1, tlib)
    try:
        tx.reserve_bgzf_out(len(text))
        gz, ends, s = tx.deflate(text)
    finally:
        tx.close()
    zm.check(text, gz, True, ends, s, name)
    with tempfile.TemporaryDirectory() as td:
        outs = {}
        for sub, fname, data in (("plain", "x.fq", text), ("gz", "x.fq.gz", gz)):
            fin = os.path.join(td, fname)
            open(fin, "wb").write(data)
            rc, out, err, _ = cli_check._run(binary, td, sub, fin, case.cmd["flags"].split(), [a.encode() for a in case.cmd["adapters"] or []])
            assert rc == 0, err
            outs[sub] = out
    assert outs["gz"] == outs["plain"] == case.ref_out and len(case.ref_out) > 1000


def test_command_line_reads_the_file(libs, golden_dir):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "host"), "emul"], check=True)
    _cli_reads_what_the_emulation_wrote(os.path.join(EMUL_DIR, "tgsfilter_emul"), libs[1], golden_dir)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")
def test_reference_reads_the_file(libs, golden_dir):
    _cli_reads_what_the_emulation_wrote(REF, libs[1], golden_dir)


def test_sweeps_under_address_sanitizer(tmp_path):
    """tests/manual/gzout_asan.cpp includes the library's source built with -fsanitize=address,undefined: one stand-alone host
    program; nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    exe = os.path.join(EMUL_DIR, "gzout_asan")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DTGSF_EMUL", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-x", "c++", os.path.join(ROOT, "tests", "manual", "gzout_asan.cpp"), "-o", exe,
                    "-L" + EMUL_DIR, "-ltgsf_emul", "-Wl,-rpath,$ORIGIN"], check=True)
    p = subprocess.run([exe], capture_output=True, timeout=600)
    assert p.returncode == 0 and b"gzout ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
