"""The BGZF input side of libtgsf_text on a GPU-less box: compressed members inflated by the serial emulation of the kernels
(tests/emul/libtgsf_text_emul.so, every lane a wave of one) against the model of tests/bgzfmodel.py, which asks zlib.
tests/test_bgzf_gpu.py repeats the checks on the HIP build, where the lanes of a wave copy side by side."""
import os
import subprocess

import pytest

from tests import bgzfparity as gp
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


def test_abi_and_symbols(tlib):
    lib = tgtext.load(tlib)
    assert lib.tgsf_text_abi_version() == tgtext.ABI_VERSION == 2
    for sym in ("tgsf_text_bgzf_walk", "tgsf_text_bgzf_reserve", "tgsf_text_bgzf_inflate", "tgsf_text_bgzf_inflate_device", "tgsf_text_bam_walk_device",
                "tgsf_text_bgzf_bam_decode", "tgsf_text_bgzf_bam_submit", "tgsf_text_bgzf_bam_filter"):
        assert sym in tgtext.SYMBOLS
        getattr(lib, sym)


def test_stored_blocks(tlib):
    gp.stored(tlib, gp.HostMem())


def test_fixed_code(tlib):
    gp.fixed_code(tlib, gp.HostMem())


def test_copies(tlib):
    gp.copies(tlib, gp.HostMem())


def test_dynamic_headers(tlib):
    gp.dynamic_headers(tlib, gp.HostMem())


def test_what_zlib_writes(tlib):
    gp.zlib_streams(tlib, gp.HostMem())


def test_several_members(tlib):
    gp.several_members(tlib, gp.HostMem())


def test_damage(tlib):
    gp.damage(tlib, gp.HostMem())


def test_host_walk(tlib):
    gp.host_walk(tlib)


def test_fuzz(tlib):
    broke, kept = gp.fuzz(tlib, gp.HostMem(), 5001, 200)
    assert broke + kept == 100 and broke >= 10 and kept >= 5, (broke, kept)


def test_into_the_text_index(tlib, golden_dir):
    gp.into_the_text_index(tlib, gp.HostMem(), golden_dir)


def test_refusals_and_recovery(tlib):
    gp.refusals(tlib, gp.HostMem())


def test_device_walk(tlib):
    gp.device_walk(tlib, gp.HostMem())


@pytest.mark.parametrize("name", sorted(gp.bp.GOLDEN))
def test_golden_compressed(libs, golden_dir, name):
    gp.golden_compressed(libs[0], libs[1], gp.HostMem(), golden_dir, name)


def test_compressed_seams(libs):
    gp.compressed_seams(libs[0], libs[1], gp.HostMem())
