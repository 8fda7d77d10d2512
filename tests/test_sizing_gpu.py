"""-m gpu: sizing and layout independence on the HIP build (tests/sizing.py holds the checks and says why;
tests/test_sizing_emul.py runs them on the emulation first), and the stage timing that only the HIP build has."""
import pytest

from tests import sizing

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("workload,hints", sizing.CASES)
def test_gpu_workload_at_sizing(workload, hints, monkeypatch):
    sizing.workload_at(None, workload, hints, monkeypatch)


@pytest.mark.parametrize("workload", ["1_ont_trims_byproduct", "2_hifi"])
def test_gpu_layouts_at_streamed_sizing(workload, monkeypatch):
    sizing.layouts_at_streamed(None, workload, monkeypatch)


@pytest.mark.parametrize("mid_flat", [None, "0"])
def test_gpu_largest_accepted_batch(mid_flat, monkeypatch):
    sizing.largest_accepted_batch(None, mid_flat, monkeypatch)


def test_gpu_largest_accepted_batch_four_filtered_adapters(monkeypatch):
    sizing.largest_accepted_batch(None, None, monkeypatch, adapters=sizing.FOUR_33, mid_match_len=30)


@pytest.mark.parametrize("kind", [1, 2])
def test_gpu_long_lived_context(kind, monkeypatch, capfd):
    sizing.long_lived_host(None, kind, monkeypatch, capfd)


@pytest.mark.parametrize("overflow", [False, True])
@pytest.mark.parametrize("kind", [1, 2])
def test_gpu_long_lived_context_batches_enqueued_together(kind, overflow, monkeypatch):
    sizing.long_lived_enqueued(None, kind, overflow, monkeypatch)


def test_gpu_fuzz_under_product_sizings(monkeypatch):
    sizing.fuzz_under_sizings(None, range(7000, 7040), 150, monkeypatch)


def test_gpu_stage_timing_over_more_batches_than_the_event_ring():
    sizing.stage_timing(None)
