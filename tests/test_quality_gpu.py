"""-m gpu: the quality gates and the QC tallies across their domain on the HIP build (tests/quality_domain.py holds the inputs
and checks and says why; tests/test_quality_emul.py runs them on the emulation first and asserts what the inputs hold)."""
import pytest

from tests import quality_domain as qd
from tgsfilter_amd import abi

pytestmark = pytest.mark.gpu
SIDES = ("min", "max")
END_CASES = [(bc, v) for bc in qd.END_BC for v in qd.END_VARIANTS]
POST_CASES = [(side, way, mode) for side in SIDES for way in qd.POST_WAYS for mode in qd.CLEAN_MODES]


@pytest.fixture(scope="module", autouse=True)
def oracle_results():
    qd.prefetch([(qd.raw_gate_case, n, s, 1, q) for n, s, w, q in qd.GATE_CASES if w == 1] + [(qd.special_case, n) for n in qd.SPECIAL] +
                [(qd.long_case, n, s) for n in qd.NOT_FEW_BITS for s in SIDES] +
                [(qd.post_case, s, w) for s in SIDES for w in qd.POST_WAYS] + [(qd.end_case, bc, v) for bc, v in END_CASES])


@pytest.mark.parametrize("name,side,w,qtype", qd.GATE_CASES)
def test_gpu_raw_gate_on_a_threshold_and_its_float_neighbours(name, side, w, qtype, monkeypatch):
    qd.run(None, qd.raw_gate_case(name, side, w, qtype), {}, monkeypatch)


@pytest.mark.parametrize("name", list(qd.SPECIAL))
def test_gpu_thresholds_the_abi_does_not_refuse(name, monkeypatch):
    qd.run(None, qd.special_case(name), {}, monkeypatch)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_gpu_long_read_one_sum_from_a_threshold(name, side, monkeypatch):
    qd.run_once(None, qd.long_case(name, side), monkeypatch)


@pytest.mark.parametrize("name", qd.NOT_FEW_BITS)
def test_gpu_power_of_two_reads_around_a_threshold(name, monkeypatch):
    qd.run_once(None, qd.mega_case(name), monkeypatch)


def test_gpu_sum_of_zero_lands_in_bin_zero(monkeypatch):
    qd.run(None, qd.zero_sum_case(), {}, monkeypatch)


@pytest.mark.parametrize("at", (0, 3, 6))
def test_gpu_sum_of_minus_one_is_refused_with_the_read_named(at, monkeypatch):
    qd.negative_sum(None, at, monkeypatch)


@pytest.mark.parametrize("mode", qd.HIST_MODES)
def test_gpu_histogram_seams(mode, monkeypatch):
    qd.run(None, qd.hist_case(mode), {}, monkeypatch)


@pytest.mark.parametrize("side,way,mode", POST_CASES)
def test_gpu_gate_after_the_split(side, way, mode, monkeypatch):
    qd.run(None, qd.post_case(side, way), qd.mode_env(mode), monkeypatch)


@pytest.mark.parametrize("mode", ("byproduct", None))
def test_gpu_results_do_not_depend_on_the_guess(mode, monkeypatch):
    qd.run(None, qd.guess_case(), qd.mode_env(mode), monkeypatch)


def test_gpu_a_batch_run_again_counts_once(monkeypatch):
    qd.run(None, qd.replay_case(), qd.REPLAY_ENV, monkeypatch)


def test_gpu_a_device_batch_run_again_counts_once(monkeypatch):
    assert qd.replay_device(None, monkeypatch) == abi.NFRAGS_NOT_FINAL


@pytest.mark.parametrize("bc,variant", END_CASES)
def test_gpu_bc_len_on_its_seams(bc, variant, monkeypatch):
    qd.run(None, qd.end_case(bc, variant), {}, monkeypatch)


def test_gpu_bc_len_beyond_every_read(monkeypatch):
    qd.run(None, qd.short_end_case(), {}, monkeypatch)


def test_gpu_widest_bc_len(monkeypatch):
    """bc_len = 2^20, the largest tgsf_create accepts: 2 048 launches of k_end_tables per table set (the serial emulation
    takes eight minutes over them: this case runs here only)."""
    qd.run_once(None, qd.widest_case(), monkeypatch)
