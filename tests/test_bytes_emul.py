"""Every byte value through the kernels that read bases and qualities, on the serial emulation (tests/bytes_domain.py holds the
checks and says why; tests/test_bytes_gpu.py runs them on the HIP build) -- and, where oracle/_ref/ was built, the oracle itself
against the reference on these bytes: without that the rest compares the kernels with an opinion."""
import os
import subprocess

import pytest

from tests import bytes_domain as bd
from tests import cli_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    return EMUL


def test_inputs_cover_the_byte_domain():
    bd.inputs_cover()


@pytest.mark.parametrize("name", list(bd.MYERS_SETS))
def test_oracle_finds_the_odd_adapters(name):
    bd.myers_found(name)


@pytest.mark.parametrize("qtype", [33, 64])
@pytest.mark.parametrize("head,tail", bd.TRIMS)
@pytest.mark.parametrize("mode", bd.MODES)
def test_emul_tallies(emul, mode, head, tail, qtype, monkeypatch):
    bd.tallies(emul, mode, head, tail, qtype, monkeypatch)


@pytest.mark.parametrize("mode", bd.MODES)
def test_emul_no_quality_tallies(emul, mode, monkeypatch):
    bd.no_qual_tallies(emul, mode, monkeypatch)


@pytest.mark.parametrize("qtype", [33, 64])
def test_emul_tail_fix_straight_to_memory(emul, qtype, monkeypatch):
    bd.tallies(emul, "byproduct", 79, 8, qtype, monkeypatch, long_tables=True)


@pytest.mark.parametrize("qtype", [33, 64])
def test_emul_by_product_through_a_pool_overflow(emul, qtype, monkeypatch, capfd):
    monkeypatch.setenv("TGSF_TRACE_POOL", "1")
    bd.tallies(emul, "byproduct", 7, 8, qtype, monkeypatch, pool_cap=3)
    assert "candidate pool overflow" in capfd.readouterr().err


@pytest.mark.parametrize("env", bd.MYERS_ENVS, ids=["default", "mid_flat_0", "mid_filter_0"])
@pytest.mark.parametrize("name", list(bd.MYERS_SETS))
def test_emul_myers(emul, name, env, monkeypatch):
    bd.myers(emul, name, env, monkeypatch)


@pytest.mark.parametrize("cls,n", [("two_words", 600), ("four_words", 600), ("wide", 300)])
def test_emul_align_windows(emul, cls, n):
    bd.align_windows(emul, cls, n)


@pytest.mark.parametrize("k", bd.REPEAT_KS)
@pytest.mark.parametrize("alphabet", list(bd.REPEAT_ALPHABETS))
def test_emul_repeat_gate(emul, alphabet, k):
    bd.repeat_gate(emul, alphabet, k)


def test_emul_repeat_gate_counted_in_memory(emul, monkeypatch):
    bd.repeat_counted_in_memory(emul, monkeypatch)


# ---- the oracle against the reference --------------------------------------------------------------------------------------
def test_oracle_edlib_over_all_byte_values():
    edlib = bd.ref_edlib()
    if edlib is None:
        pytest.skip("oracle/_ref/libedlib_ref.so not built")
    bd.oracle_edlib_all_bytes(edlib, 2000)


@pytest.mark.skipif(not os.path.exists(bd.REF_BIN), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")
@pytest.mark.parametrize("seed,flags", [(9101, "-x ont -l 500 -q 7 -5 0 -3 0"), (9102, "-x ont -l 500 -q 7 -5 7 -3 8 -e 513"),
                                        (9103, "-x ont -l 300 -q 7 -5 100 -3 3 -p 40 -k 11")])
def test_cli_live_odd_bytes_emul(seed, flags):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "host"), "emul"], check=True)
    cli_check.compare_live(os.path.join(EMUL_DIR, "tgsfilter_emul"), bd.REF_BIN, None, flags.split(), bd.ADS[:1], raw_input=bd.odd_fastq(seed))
