"""The adapter search across its parameters and adapter sets on the serial emulation of the kernels (tests/search_domain.py
holds the inputs and checks and says why; tests/test_search_gpu.py runs them on the HIP build), a fuzzing stream over the same
dimensions (tests/fuzz.py, TGSF_FUZZ_SEARCH), and create plus one batch over the accepted corners of the parameters under
AddressSanitizer, UBSan and -fsanitize=float-cast-overflow in a stand-alone program (tests/manual/search_asan.cpp)."""
import os
import subprocess

import pytest

from tests import fuzz
from tests import search_domain as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)
SIM_CASES = [(Q, m, w) for Q, m in sd.GATE_QM for w in range(3)]


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    return EMUL


# ---- the inputs hold what they are there for: assertions on the oracle's result alone ---------------------------------------
@pytest.mark.parametrize("E", sd.SEAM_E)
def test_seam_inputs_hold_what_they_are_there_for(E):
    sd.seam_case(E)


@pytest.mark.parametrize("T,variant", sd.MARGIN_CASES)
def test_margin_inputs_hold_what_they_are_there_for(T, variant):
    sd.margin_case(T, variant)


@pytest.mark.parametrize("Q,m", sd.GATE_QM)
def test_gate_inputs_change_their_outcome_between_the_three_similarities(Q, m):
    sd.sim_case(Q, m, 1)


@pytest.mark.parametrize("name", list(sd.SETS))
def test_set_inputs_hold_what_they_are_there_for(name):
    sd.set_case(name)


# ---- S1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", list(sd.SEAM_ENVS))
@pytest.mark.parametrize("E", sd.SEAM_E)
def test_emul_window_seams(emul, E, scan, monkeypatch):
    reads, p, exp = sd.seam_case(E)
    sd.run(emul, p, reads, exp, sd.SEAM_ENVS[scan], monkeypatch)


# ---- S2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,variant", sd.MARGIN_CASES)
def test_emul_margins_and_merging(emul, T, variant, monkeypatch):
    reads, p, exp = sd.margin_case(T, variant)
    sd.run(emul, p, reads, exp, {}, monkeypatch)


# ---- S3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,m,which", SIM_CASES)
def test_emul_similarity_on_a_float_seam(emul, Q, m, which, monkeypatch):
    reads, p, exp = sd.sim_case(Q, m, which)
    sd.run(emul, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("end_m,mid_m", sd.MATCH_CASES)
def test_emul_match_lengths_around_an_adapters_length(emul, end_m, mid_m, monkeypatch):
    reads, p, exp = sd.match_case(end_m, mid_m)
    sd.run(emul, p, reads, exp, {}, monkeypatch)


def test_emul_end_windows_of_four_five_and_six_columns(emul, monkeypatch):
    reads, p, exp = sd.tiny_case()
    sd.run(emul, p, reads, exp, {}, monkeypatch)


@pytest.mark.parametrize("sim", sd.GATE_SIMS)
def test_emul_similarities_nobody_would_ask_for(emul, sim, monkeypatch):
    reads, p, exp = sd.loose_case(sim)
    sd.run(emul, p, reads, exp, {}, monkeypatch)


# ---- S4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", sd.SET_CASES)
def test_emul_adapter_sets(emul, name, env, monkeypatch):
    reads, p, exp = sd.set_case(name)
    sd.run(emul, p, reads, exp, sd.SET_ENVS[env], monkeypatch)


# ---- S5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40000, 40060))
def test_emul_fuzz_search(emul, seed, monkeypatch):
    monkeypatch.setenv("TGSF_FUZZ_SEARCH", "1")
    fuzz.run_case(emul, seed, 24)


def test_corners_of_the_search_parameters_under_sanitizers(tmp_path):
    """The stand-alone program links the emulation sources built with -fsanitize=address,undefined,float-cast-overflow;
    nothing of it is loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "search_asan"], check=True)
    env = {k: v for k, v in os.environ.items() if k not in sd.KNOBS}
    p = subprocess.run([os.path.join(EMUL_DIR, "search_asan")], capture_output=True, env=env, timeout=600)
    assert p.returncode == 0 and b"search ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
