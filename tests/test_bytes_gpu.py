"""-m gpu: every byte value through the kernels that read bases and qualities, on the HIP build (tests/bytes_domain.py holds the
checks and says why; tests/test_bytes_emul.py runs them on the emulation first and asserts the inputs' coverage)."""
import pytest

from tests import bytes_domain as bd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("qtype", [33, 64])
@pytest.mark.parametrize("head,tail", bd.TRIMS)
@pytest.mark.parametrize("mode", bd.MODES)
def test_gpu_tallies(mode, head, tail, qtype, monkeypatch):
    bd.tallies(None, mode, head, tail, qtype, monkeypatch)


@pytest.mark.parametrize("mode", bd.MODES)
def test_gpu_no_quality_tallies(mode, monkeypatch):
    bd.no_qual_tallies(None, mode, monkeypatch)


@pytest.mark.parametrize("qtype", [33, 64])
def test_gpu_tail_fix_straight_to_memory(qtype, monkeypatch):
    bd.tallies(None, "byproduct", 79, 8, qtype, monkeypatch, long_tables=True)


@pytest.mark.parametrize("qtype", [33, 64])
def test_gpu_by_product_through_a_pool_overflow(qtype, monkeypatch, capfd):
    monkeypatch.setenv("TGSF_TRACE_POOL", "1")
    bd.tallies(None, "byproduct", 7, 8, qtype, monkeypatch, pool_cap=3)
    assert "candidate pool overflow" in capfd.readouterr().err


@pytest.mark.parametrize("env", bd.MYERS_ENVS, ids=["default", "mid_flat_0", "mid_filter_0"])
@pytest.mark.parametrize("name", list(bd.MYERS_SETS))
def test_gpu_myers(name, env, monkeypatch):
    bd.myers(None, name, env, monkeypatch)


@pytest.mark.parametrize("cls,n", [("two_words", 1600), ("four_words", 1600), ("wide", 800)])
def test_gpu_align_windows(cls, n):
    bd.align_windows(None, cls, n)


@pytest.mark.parametrize("k", bd.REPEAT_KS)
@pytest.mark.parametrize("alphabet", list(bd.REPEAT_ALPHABETS))
def test_gpu_repeat_gate(alphabet, k):
    bd.repeat_gate(None, alphabet, k)


def test_gpu_repeat_gate_counted_in_memory(monkeypatch):
    bd.repeat_counted_in_memory(None, monkeypatch)
