"""What libtgsf refuses, and what a context is worth afterwards, on the serial emulation of the kernels (tests/refusals.py
holds the checks; tests/test_refusals_gpu.py runs them on the HIP build).  A read of length 0 that made a kernel read or
write out of bounds shows under tests/manual/sanitize_emul.py, which runs this file on the sanitizer build."""
import os
import subprocess

import pytest

from tests import refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)

MODES = [None, "byproduct"]


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    return EMUL


def test_emul_host_side_refusals_leave_the_context_alone(emul):
    refusals.host_refusals(emul)


def test_emul_text_larger_than_the_context_takes(emul):
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    refusals.text_over_capacity(emul, os.path.join(EMUL_DIR, "libtgsf_text_emul.so"))


def test_emul_min_len_below_zero_is_refused_for_the_text_filter_too(emul):
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    refusals.min_len_below_zero(emul, os.path.join(EMUL_DIR, "libtgsf_text_emul.so"))


def test_emul_end_len_and_extra_len_above_their_bound_are_refused(emul):
    refusals.end_len_and_extra_len_above_their_bound(emul)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [0, 7, 256, -1])
@pytest.mark.parametrize("kind", ["len0", "offsets", "over"])
def test_emul_read_of_unsupported_length(emul, kind, at, mode, monkeypatch):
    refusals.bad_length(emul, kind, at, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_emul_two_reads_of_length_0(emul, mode, monkeypatch):
    refusals.two_bad_lengths(emul, monkeypatch, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("at", [0, -1])
def test_emul_raw_mean_quality_below_0(emul, at, mode, monkeypatch):
    refusals.bad_mean_quality(emul, at, mode, monkeypatch)


def test_oracle_accepts_a_read_whose_kept_part_has_a_negative_mean():
    refusals.negative_kept_mean_oracle()


@pytest.mark.parametrize("mode", MODES)
def test_emul_kept_part_with_a_negative_mean_is_not_refused(emul, mode, monkeypatch):
    refusals.negative_kept_mean(emul, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_emul_kept_part_with_a_mean_outside_the_tables_is_reported(emul, mode, monkeypatch):
    refusals.kept_mean_outside_the_tables(emul, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_emul_fragment_capacity(emul, mode, monkeypatch):
    refusals.fragment_capacity(emul, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what", ["length", "mean quality"])
def test_emul_refused_batch_between_two_good_ones(emul, what, mode, monkeypatch):
    refusals.refused_between_good(emul, what, mode, monkeypatch)


def test_emul_enqueue_limit_drains_by_itself(emul):
    refusals.enqueue_limit(emul)


def test_emul_enqueue_limit_with_a_batch_to_run_again(emul, monkeypatch):
    refusals.enqueue_limit_needs_wait(emul, monkeypatch)


def test_emul_fetch_and_merge_tallies(emul):
    refusals.fetch_and_merge(emul)


def test_emul_pending_refusal_comes_through_counters_and_merge(emul):
    refusals.refusal_through_other_calls(emul)
