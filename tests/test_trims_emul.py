"""Fixed trims across their domain on the serial emulation of the kernels (tests/trims_domain.py holds the checks and says
why; tests/test_trims_gpu.py runs them on the HIP build, and a batch of 136 000 reads besides), and create plus one batch
over the corners of min_len, max_len and the trims under AddressSanitizer in a stand-alone program
(tests/manual/trims_asan.cpp)."""
import os
import subprocess

import pytest

from tests import trims_domain as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    td.prefetch(td.SEAM_CASES + td.MIN_LEN_CASES)
    return EMUL


@pytest.mark.parametrize("case", td.SEAM_CASES + td.MIN_LEN_CASES, ids=td.case_id)
def test_inputs_hold_what_they_are_there_for(case):
    td.expected(case)


@pytest.mark.parametrize("case", [td.SEAM_CASES[0], td.SEAM_CASES[-1], td.MIN_LEN_CASES[0]], ids=td.case_id)
def test_oracle_doubles_the_tallies_of_a_batch_run_twice(case):
    td.second_batch_doubles(case)


@pytest.mark.parametrize("mode", td.MODES, ids=["byproduct", "default"])
@pytest.mark.parametrize("case", td.SEAM_CASES, ids=td.case_id)
def test_emul_seam_sweep(emul, case, mode, monkeypatch):
    td.run_case(emul, case, mode, monkeypatch)


@pytest.mark.parametrize("mode", td.MODES, ids=["byproduct", "default"])
@pytest.mark.parametrize("case", td.MIN_LEN_CASES, ids=td.case_id)
def test_emul_small_minimum_lengths(emul, case, mode, monkeypatch):
    td.run_case(emul, case, mode, monkeypatch)


def test_emul_switch_goes_off_and_comes_back(emul, monkeypatch, capfd):
    td.switch_adaptive(emul, monkeypatch, capfd)


def test_emul_switch_forced_on_stays_on(emul, monkeypatch, capfd):
    td.switch_forced(emul, monkeypatch, capfd)


def test_corners_of_lengths_and_trims_under_address_sanitizer(tmp_path):
    """The stand-alone program links the emulation sources built with -fsanitize=address,undefined; nothing of it is
    loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "trims_asan"], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("TGSF_MID_FLAT", "TGSF_POOL_CAP", "TGSF_CLEAN_TABLES", "TGSF_TRACE_BP")}
    p = subprocess.run([os.path.join(EMUL_DIR, "trims_asan")], capture_output=True, env=env, timeout=600)
    assert p.returncode == 0 and b"trims ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
