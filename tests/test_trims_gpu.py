"""-m gpu: fixed trims across their domain and at the scale of a product batch, on the HIP build (tests/trims_domain.py holds
the checks and says why; tests/test_trims_emul.py runs the small ones on the emulation first and asserts the inputs'
coverage).  No parameter set with min_len < 0 reaches a kernel: tgsf_create refuses it (tests/test_abi.py,
tests/test_refusals_gpu.py)."""
import pytest

from tests import trims_domain as td

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def oracle_results():
    td.prefetch(td.SEAM_CASES + td.MIN_LEN_CASES)


@pytest.mark.parametrize("mode", td.MODES, ids=["byproduct", "default"])
@pytest.mark.parametrize("case", td.SEAM_CASES, ids=td.case_id)
def test_gpu_seam_sweep(case, mode, monkeypatch):
    td.run_case(None, case, mode, monkeypatch)


@pytest.mark.parametrize("mode", td.MODES, ids=["byproduct", "default"])
@pytest.mark.parametrize("case", td.MIN_LEN_CASES, ids=td.case_id)
def test_gpu_small_minimum_lengths(case, mode, monkeypatch):
    td.run_case(None, case, mode, monkeypatch)


def test_gpu_switch_goes_off_and_comes_back(monkeypatch, capfd):
    td.switch_adaptive(None, monkeypatch, capfd)


def test_gpu_switch_forced_on_stays_on(monkeypatch, capfd):
    td.switch_forced(None, monkeypatch, capfd)


# ---- scale: 136 000 reads in one batch ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    return td.ScaleInput(adapters=False)


@pytest.fixture(scope="module")
def with_adapters():
    """The input with adapters and the oracle's answer under trims of 79 / 13, in 16 runs side by side."""
    inp = td.ScaleInput(adapters=True)
    p = inp.params(79, 13, td.ADS)
    return inp, p, inp.oracle(p, workers=16)


def test_scale_input_mixes_right_and_wrong_guesses(plain):
    counts = plain.check()
    print("sample passes: %d; sample passes and the read fails: %d; the other way: %d; sample passes beyond the grid: %d" % counts)


@pytest.mark.parametrize("head,tail,max_read_len,qtype", [(79, 13, None, 33), (3, 250, None, 33), (79, 13, 250_000, 33), (79, 13, None, 64)],
                         ids=["79-13", "3-250", "79-13-long_tables", "79-13-qtype64"])
def test_gpu_scale_without_adapters(plain, head, tail, max_read_len, qtype, monkeypatch, capfd):
    """Leg 1: no adapter, so every read that passes the gate is kept as speculated and every wrong guess of k_prepare is one
    read taken back out or put in; k_tail_fix's grid wraps, every one of its blocks flushes into the same few rows."""
    p = plain.params(head, tail, [], qtype=qtype, max_read_len=max_read_len)
    qual = plain.qual64() if qtype == 64 else None
    exp = plain.oracle(p, qual=qual)
    kept = (exp[0]["n_frags"] == 1).sum()
    assert kept > td.SCALE_N // 4 and ((exp[0]["flags"] & 1) != 0).sum() > td.SCALE_N // 8
    assert plain.run(None, p, exp, None, monkeypatch, capfd, qual=qual) == 1


@pytest.mark.parametrize("mode", [None, "byproduct", "direct", "difference"], ids=["default", "byproduct", "direct", "difference"])
def test_gpu_scale_with_adapters(with_adapters, mode, monkeypatch, capfd):
    """Leg 2: adapters at the ends of 30 % of the reads and in the middle of 2 %: speculated reads that turn out trimmed or
    split, by the ten thousand.  Every strategy for the clean tables gives the oracle's three arrays."""
    inp, p, exp = with_adapters
    r = exp[0]
    assert ((r["flags"] & (2 | 4)) != 0).sum() > inp.planted_end // 2 and ((r["flags"] & 8) != 0).sum() > inp.planted_mid // 4
    assert (r["n_frags"] > 1).sum() > inp.planted_split // 4
    speculated = inp.run(None, p, exp, mode, monkeypatch, capfd)
    assert speculated == (1 if mode in (None, "byproduct") else 0)
