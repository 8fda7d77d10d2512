"""The quality gates and the QC tallies across their domain on the serial emulation of the kernels (tests/quality_domain.py
holds the inputs and checks and says why; tests/test_quality_gpu.py runs them on the HIP build), and create plus one batch
over the corners of the thresholds and of bc_len under AddressSanitizer, UBSan and -fsanitize=float-cast-overflow in a
stand-alone program (tests/manual/quality_asan.cpp)."""
import os
import subprocess

import pytest

from tests import quality_domain as qd
from tgsfilter_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)
SIDES = ("min", "max")
END_CASES = [(bc, v) for bc in qd.END_BC for v in qd.END_VARIANTS]
POST_CASES = [(side, way, mode) for side in SIDES for way in qd.POST_WAYS for mode in qd.CLEAN_MODES]


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    return EMUL


# ---- the inputs hold what they are there for: assertions on the oracle's result alone ---------------------------------------
@pytest.mark.parametrize("name,side,qtype", [(n, s, q) for n, s, w, q in qd.GATE_CASES if w == 1])
def test_gate_inputs_change_their_outcome_on_the_threshold(name, side, qtype):
    qd.raw_gate_case(name, side, 1, qtype)


@pytest.mark.parametrize("name", list(qd.SPECIAL))
def test_special_threshold_inputs_hold_what_they_are_there_for(name):
    qd.special_case(name)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_a_float_mean_gives_the_other_answer_on_the_long_reads(name, side):
    """The smallest L whose seam read a mean held in float32 AND a mean formed as (float)sum / (float)L judge the other way
    than the double gate: below 9.9f 116 509 bases (sum 1 153 439), below 20.3f 58 257 (1 182 617), below 60.1f 29 131
    (1 750 773); above each of them 10 bases (sums 99, 203, 601: the three floats lie just below 9.9, 20.3 and 60.1).  The check
    is quality_domain.float_disagreement: every L from 1 to 2^22, sum = ceil(L t) - 1 or floor(L t) + 1 in integers, then
    float64(sum) / float64(L) < float64(t) against float32(that quotient) < t and against float32(sum) / float32(L) < t."""
    assert qd.float_disagreement(name, side)[0] == qd.LONG_L[(name, side)]
    qd.long_case(name, side)


@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_a_float_mean_gives_the_other_answer_on_the_power_of_two_reads(name):
    """The smallest power of two with the same property below the threshold: 2^21 for 9.9f, 2^20 for 20.3f, 2^19 for 60.1f (at
    half of each both float restatements still agree with the double gate: quality_domain.mega_case asserts both)."""
    qd.mega_case(name)


@pytest.mark.parametrize("mode", qd.HIST_MODES)
def test_histogram_inputs_land_in_the_bins_they_are_there_for(mode):
    qd.hist_case(mode)
    qd.zero_sum_case()


@pytest.mark.parametrize("way", qd.POST_WAYS)
@pytest.mark.parametrize("side", SIDES)
def test_post_split_inputs_fail_after_the_bin_tables_and_before_the_rest(side, way):
    qd.post_case(side, way)


@pytest.mark.parametrize("value,side,kind", qd.CLI_CORNERS)
def test_command_line_inputs_are_kept_as_the_pieces_they_are_designed_for(value, side, kind):
    """The reads of tests/test_cli_live.py's QUALITY_CORNERS and of the goldens quality_* under the parameters the command
    line resolves their flags to."""
    qd.cli_case(value, side, kind)


def test_guess_inputs_are_guessed_wrong_and_on_the_threshold():
    qd.guess_case()


@pytest.mark.parametrize("bc,variant", END_CASES)
def test_end_table_inputs_hold_what_they_are_there_for(bc, variant):
    qd.end_case(bc, variant)
    qd.short_end_case()


# ---- Q1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,side,w,qtype", qd.GATE_CASES)
def test_emul_raw_gate_on_a_threshold_and_its_float_neighbours(emul, name, side, w, qtype, monkeypatch):
    qd.run(emul, qd.raw_gate_case(name, side, w, qtype), {}, monkeypatch)


@pytest.mark.parametrize("name", list(qd.SPECIAL))
def test_emul_thresholds_the_abi_does_not_refuse(emul, name, monkeypatch):
    qd.run(emul, qd.special_case(name), {}, monkeypatch)


# ---- Q2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_emul_long_read_one_sum_from_a_threshold(emul, name, side, monkeypatch):
    qd.run_once(emul, qd.long_case(name, side), monkeypatch)


@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_emul_power_of_two_reads_around_a_threshold(emul, name, monkeypatch):
    qd.run_once(emul, qd.mega_case(name), monkeypatch)


# ---- Q3 ------------------------------------------------------------------------------------------------------------------------
def test_emul_sum_of_zero_lands_in_bin_zero(emul, monkeypatch):
    qd.run(emul, qd.zero_sum_case(), {}, monkeypatch)


@pytest.mark.parametrize("at", (0, 3, 6))
def test_emul_sum_of_minus_one_is_refused_with_the_read_named(emul, at, monkeypatch):
    qd.negative_sum(emul, at, monkeypatch)


# ---- Q4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", qd.HIST_MODES)
def test_emul_histogram_seams(emul, mode, monkeypatch):
    qd.run(emul, qd.hist_case(mode), {}, monkeypatch)


# ---- Q5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,way,mode", POST_CASES)
def test_emul_gate_after_the_split(emul, side, way, mode, monkeypatch):
    qd.run(emul, qd.post_case(side, way), qd.mode_env(mode), monkeypatch)


# ---- Q6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("byproduct", None))
def test_emul_results_do_not_depend_on_the_guess(emul, mode, monkeypatch):
    qd.run(emul, qd.guess_case(), qd.mode_env(mode), monkeypatch)


# ---- Q7 ------------------------------------------------------------------------------------------------------------------------
def test_emul_a_batch_run_again_counts_once(emul, monkeypatch):
    qd.run(emul, qd.replay_case(), qd.REPLAY_ENV, monkeypatch)


def test_emul_a_device_batch_run_again_counts_once(emul, monkeypatch):
    assert qd.replay_device(emul, monkeypatch) == abi.NFRAGS_NOT_FINAL


# ---- E1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc,variant", END_CASES)
def test_emul_bc_len_on_its_seams(emul, bc, variant, monkeypatch):
    qd.run(emul, qd.end_case(bc, variant), {}, monkeypatch)


def test_emul_bc_len_beyond_every_read(emul, monkeypatch):
    qd.run(emul, qd.short_end_case(), {}, monkeypatch)


def test_corners_of_the_thresholds_and_of_bc_len_under_sanitizers(tmp_path):
    """The stand-alone program links the emulation sources built with -fsanitize=address,undefined,float-cast-overflow;
    nothing of it is loaded into this process.  `quick`: without bc_len 2^20, whose 4 096 launches of k_end_tables take the
    serial emulation eight minutes as it is and twenty under the sanitizers (the program without an argument runs it too)."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "quality_asan"], check=True)
    from tests.search_domain import KNOBS
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    p = subprocess.run([os.path.join(EMUL_DIR, "quality_asan"), "quick"], capture_output=True, env=env, timeout=600)
    assert p.returncode == 0 and b"quality ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
