"""Sizing and layout independence on the serial emulation of the kernels (tests/sizing.py holds the checks and says why;
tests/test_sizing_gpu.py runs them on the HIP build), and the largest batch a context accepts under AddressSanitizer in a
stand-alone program (tests/manual/largest_batch_asan.cpp)."""
import os
import subprocess

import pytest

from tests import sizing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL = os.environ.get("TGSF_EMUL_LIB") or os.path.join(EMUL_DIR, "libtgsf_emul.so")     # (tests/manual/sanitize_emul.py: the sanitizer build)


@pytest.fixture(scope="module")
def emul():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    return EMUL


def test_seam_sizings_sit_on_the_histogram_switch():
    sizing.seams_sit_on_the_switch()


@pytest.mark.parametrize("workload,hints", sizing.CASES)
def test_emul_workload_at_sizing(emul, workload, hints, monkeypatch):
    sizing.workload_at(emul, workload, hints, monkeypatch)


@pytest.mark.parametrize("workload", ["1_ont_trims_byproduct", "2_hifi"])
def test_emul_layouts_at_streamed_sizing(emul, workload, monkeypatch):
    sizing.layouts_at_streamed(emul, workload, monkeypatch)


@pytest.mark.parametrize("mid_flat", [None, "0"])
def test_emul_largest_accepted_batch(emul, mid_flat, monkeypatch):
    sizing.largest_accepted_batch(emul, mid_flat, monkeypatch)


def test_emul_largest_accepted_batch_four_filtered_adapters(emul, monkeypatch):
    sizing.largest_accepted_batch(emul, None, monkeypatch, adapters=sizing.FOUR_33, mid_match_len=30)


@pytest.mark.parametrize("kind", [1, 2])
def test_emul_long_lived_context(emul, kind, monkeypatch, capfd):
    sizing.long_lived_host(emul, kind, monkeypatch, capfd)


@pytest.mark.parametrize("overflow", [False, True])
@pytest.mark.parametrize("kind", [1, 2])
def test_emul_long_lived_context_batches_enqueued_together(emul, kind, overflow, monkeypatch):
    sizing.long_lived_enqueued(emul, kind, overflow, monkeypatch)


def test_emul_fuzz_under_product_sizings(emul, monkeypatch):
    sizing.fuzz_under_sizings(emul, range(7000, 7040), 60, monkeypatch)


def test_largest_accepted_batch_under_address_sanitizer(tmp_path):
    """The stand-alone program links the emulation sources built with -fsanitize=address,undefined; nothing of it is
    loaded into this process."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "largest_batch_asan"], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("TGSF_MID_FLAT", "TGSF_POOL_CAP", "TGSF_CLEAN_TABLES")}
    p = subprocess.run([os.path.join(EMUL_DIR, "largest_batch_asan")], capture_output=True, env=env, timeout=600)
    assert p.returncode == 0 and b"largest batch ok" in p.stdout, (p.returncode, p.stdout.decode()[-1000:], p.stderr.decode()[-3000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-3000:]
