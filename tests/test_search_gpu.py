"""-m gpu: the adapter search across its parameters and adapter sets on the HIP build (tests/search_domain.py holds the inputs
and checks and says why; tests/test_search_emul.py runs them on the emulation first and asserts what the inputs hold).  No
batch here carries an end_len or extra_len above 2^28: tgsf_create refuses those (tests/test_abi.py, tests/test_refusals_gpu.py)."""
import pytest

from tests import fuzz
from tests import search_domain as sd

pytestmark = pytest.mark.gpu
SIM_CASES = [(Q, m, w) for Q, m in sd.GATE_QM for w in range(3)]


@pytest.fixture(scope="module", autouse=True)
def oracle_results():
    sd.prefetch([(sd.seam_case, E) for E in sd.SEAM_E] + [(sd.margin_case, T, v) for T, v in sd.MARGIN_CASES] + [(sd.set_case, name) for name in sd.SETS])


@pytest.mark.parametrize("scan", list(sd.SEAM_ENVS))
@pytest.mark.parametrize("E", sd.SEAM_E)
def test_gpu_window_seams(E, scan, monkeypatch):
    reads, p, exp = sd.seam_case(E)
    sd.run(None, p, reads, exp, sd.SEAM_ENVS[scan], monkeypatch)


@pytest.mark.parametrize("T,variant", sd.MARGIN_CASES)
def test_gpu_margins_and_merging(T, variant, monkeypatch):
    reads, p, exp = sd.margin_case(T, variant)
    sd.run(None, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("Q,m,which", SIM_CASES)
def test_gpu_similarity_on_a_float_seam(Q, m, which, monkeypatch):
    reads, p, exp = sd.sim_case(Q, m, which)
    sd.run(None, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("end_m,mid_m", sd.MATCH_CASES)
def test_gpu_match_lengths_around_an_adapters_length(end_m, mid_m, monkeypatch):
    reads, p, exp = sd.match_case(end_m, mid_m)
    sd.run(None, p, reads, exp, {}, monkeypatch)


def test_gpu_end_windows_of_four_five_and_six_columns(monkeypatch):
    reads, p, exp = sd.tiny_case()
    sd.run(None, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("sim", sd.GATE_SIMS)
def test_gpu_similarities_nobody_would_ask_for(sim, monkeypatch):
    reads, p, exp = sd.loose_case(sim)
    sd.run(None, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("name,env", sd.SET_CASES)
def test_gpu_adapter_sets(name, env, monkeypatch):
    reads, p, exp = sd.set_case(name)
    sd.run(None, p, reads, exp, sd.SET_ENVS[env], monkeypatch)


@pytest.mark.parametrize("name", ["runs32", "lengths32"])
def test_gpu_adapter_set_of_32_through_submit_device(name, monkeypatch):
    """tgsf_submit_device and tgsf_wait with 32 adapters and a candidate pool of 3 slots: the first run leaves the batch alone
    (the fragment count says so), tgsf_wait runs it again in position order."""
    from tgsfilter_amd import abi
    sd.set_env(monkeypatch, {"TGSF_POOL_CAP": "3"})
    assert sd.device_batch(name) == abi.NFRAGS_NOT_FINAL


@pytest.mark.parametrize("block", range(20))
def test_gpu_fuzz_search(block, monkeypatch):
    """300 seeds of the search stream (the emulation runs the first 60 of them), 15 a test."""
    monkeypatch.setenv("TGSF_FUZZ_SEARCH", "1")
    for seed in range(40000 + 15 * block, 40015 + 15 * block):
        fuzz.run_case(None, seed, 24)
