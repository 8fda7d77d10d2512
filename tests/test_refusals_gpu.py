"""-m gpu: what libtgsf.so refuses, and what a context is worth afterwards, on the HIP build (tests/refusals.py holds the
checks; tests/test_refusals_emul.py runs them on the emulation first).  No batch here has offsets outside its buffers:
the library does not check them (include/tgsf.h, tgsf_batch_in)."""
import pytest

from tests import refusals

pytestmark = pytest.mark.gpu

MODES = [None, "byproduct"]


def test_gpu_host_side_refusals_leave_the_context_alone():
    refusals.host_refusals(None)


def test_gpu_text_larger_than_the_context_takes():
    refusals.text_over_capacity(None, None)


def test_gpu_min_len_below_zero_is_refused_for_the_text_filter_too():
    refusals.min_len_below_zero(None, None)


def test_gpu_end_len_and_extra_len_above_their_bound_are_refused():
    refusals.end_len_and_extra_len_above_their_bound(None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [0, 7, 256, -1])
@pytest.mark.parametrize("kind", ["len0", "offsets", "over"])
def test_gpu_read_of_unsupported_length(kind, at, mode, monkeypatch):
    refusals.bad_length(None, kind, at, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_gpu_two_reads_of_length_0(mode, monkeypatch):
    refusals.two_bad_lengths(None, monkeypatch, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [0, -1])
def test_gpu_raw_mean_quality_below_0(at, mode, monkeypatch):
    refusals.bad_mean_quality(None, at, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_gpu_kept_part_with_a_negative_mean_is_not_refused(mode, monkeypatch):
    refusals.negative_kept_mean(None, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_gpu_kept_part_with_a_mean_outside_the_tables_is_reported(mode, monkeypatch):
    refusals.kept_mean_outside_the_tables(None, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_gpu_fragment_capacity(mode, monkeypatch):
    refusals.fragment_capacity(None, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what", ["length", "mean quality"])
def test_gpu_refused_batch_between_two_good_ones(what, mode, monkeypatch):
    refusals.refused_between_good(None, what, mode, monkeypatch)


def test_gpu_enqueue_limit_drains_by_itself():
    refusals.enqueue_limit(None)


def test_gpu_enqueue_limit_with_a_batch_to_run_again(monkeypatch):
    refusals.enqueue_limit_needs_wait(None, monkeypatch)


def test_gpu_fetch_and_merge_tallies():
    refusals.fetch_and_merge(None)


def test_gpu_pending_refusal_comes_through_counters_and_merge():
    refusals.refusal_through_other_calls(None)


def test_gpu_device_index_out_of_range():
    refusals.device_out_of_range(None)
