"""The match search of the BGZF output side of libtgsf_text (level 1, tgsf_text_bgzf_out_level) on a GPU-less box: the serial
emulation of the kernels (tests/emul/libtgsf_text_emul.so) through the checks of tests/gzlzparity.py -- everything
tests/gzoutparity.py asks of an output, and the sizes and tokens that only a match search has.  tests/test_gzlz_gpu.py
repeats them on the HIP build, where the 64 positions of a round are 64 lanes."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import gzlzmodel as lm, gzlzparity as lp, gzoutmodel as zm, gzoutparity as zp
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


def test_token_reader_on_what_zlib_writes():
    """The DEFLATE reader, before anything is judged by it: zlib's output at levels 1 and 9 (and stored and fixed blocks), read
    into tokens and expanded again, is the text; its matches are in range.  This one pins the model, not the library."""
    rng = np.random.default_rng(500)
    texts = (lm.hifi_like(rng, zm.MEMBER), zm.fastq_like(rng, 30000), lm.three_copies(rng, 9000), b"", b"a", b"abc" * 400, lm.uniform(rng, 70000), b"~" * 5000)
    matches = 0
    for text in texts:
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_RLE)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            blocks = lm.tokens(co.compress(text) + co.flush())
            assert lm.expand(blocks) == text, (len(text), level, strategy)
            matches += sum(isinstance(t, tuple) for toks in blocks for t in toks)
    assert matches > 1000
    assert [lm.length_extra_bits(x) for x in (3, 10, 11, 18, 19, 35, 67, 131, 257, 258)] == [0, 0, 1, 1, 2, 3, 4, 5, 5, 0]
    assert [lm.distance_extra_bits(x) for x in (1, 4, 5, 8, 9, 32, 33, 512, 513, 8193, 16385, 32768)] == [0, 0, 1, 1, 2, 3, 4, 7, 8, 12, 13, 13]
    text = lm.hifi_like(rng, 3 * zm.MEMBER)
    assert lm.zlib_size(text, 6, zlib.Z_HUFFMAN_ONLY) == zm.huffman_only_size(text) and lm.zlib_size(text, 1) < 0.8 * zm.huffman_only_size(text)
    with pytest.raises(AssertionError):                                 # a distance in front of the first byte
        lm.expand([[65, (3, 2)]])


def test_interface(tlib, golden_dir):
    lp.interface(tlib, zp.HostMem(), golden_dir)


def test_hifi_like_size(tlib):
    lp.hifi_size(tlib, zp.HostMem())


def test_far_matches(tlib):
    lp.far_matches(tlib, zp.HostMem())


def test_never_worse(tlib, golden_dir):
    lp.never_worse(tlib, zp.HostMem(), golden_dir)


def test_match_geometry(tlib):
    lp.match_geometry(tlib, zp.HostMem())


def test_member_independence(tlib):
    lp.independence(tlib, zp.HostMem())


def test_golden_filter_bgzf_at_level_1(libs, golden_dir):
    lp.golden_filter_bgzf(libs[0], libs[1], golden_dir, "hifi_auto")


def test_golden_bam_bgzf_at_level_1(libs, golden_dir):
    lp.golden_bam_bgzf(libs[0], libs[1], zp.HostMem(), golden_dir, "hifi_bam")


def test_compressed_bytes_are_the_pinned_ones(tlib, golden_dir):
    lp.pinned_bytes(tlib, zp.HostMem(), golden_dir)


def test_two_levels_two_threads(tlib):
    lp.two_levels_two_threads(tlib, zp.HostMem)


def test_the_lengths_and_seams_of_level_0_at_level_1(tlib):
    """What tests/gzoutparity.py feeds level 0 -- every length around the seams, one byte value, a rare byte on every lane piece
    -- through level 1."""
    rng = np.random.default_rng(501)
    fq = lm.hifi_like(rng, 2 * zm.MEMBER + 1)
    D = lp.Deflater(tlib, zp.HostMem(), 1 << 18)
    try:
        for n in zp.LENGTHS:
            for text in (fq[:n], b"G" * n):
                gz, ends, s, _ = D.run(text, n % 2 == 0, ("length", n, text[:1]))
                assert s["n_members"] == (n + zm.MEMBER - 1) // zm.MEMBER + (n % 2 == 0)
        for p in list(range(0, 201, 7)) + [1499]:
            t = bytearray(b"A" * 1500)
            t[p] = ord("#")
            D.run(bytes(t), p % 2 == 0, ("rare byte at", p))
    finally:
        D.close()


def test_sweeps_under_address_sanitizer(tmp_path):
    """tests/manual/gzlz_asan.cpp includes the library's source built with -fsanitize=address,undefined: one stand-alone host
    program; nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    exe = os.path.join(EMUL_DIR, "gzlz_asan")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-DTGSF_EMUL", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-x", "c++", os.path.join(ROOT, "tests", "manual", "gzlz_asan.cpp"), "-o", exe,
                    "-L" + EMUL_DIR, "-ltgsf_emul", "-Wl,-rpath,$ORIGIN"], check=True)
    p = subprocess.run([exe], capture_output=True, timeout=600)
    assert p.returncode == 0 and b"gzlz ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
