"""libtgsf_text on a GPU-less box: tests/emul/libtgsf_text_emul.so is tgsfilter_amd/csrc/tgsf_text.hip and its kernels
compiled with -DTGSF_EMUL and run lane by lane (every lane a wave of one), linked against the emulation of libtgsf.
The index equals the rule of include/tgsf_text.h as tests/textmodel.py states it, word for word; the one-call form equals
libtgsf with a host-made index and the oracle.  tests/test_text_gpu.py repeats this on the HIP build."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import textmodel, textparity
from tgsfilter_amd import synth, text as tgtext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")


@pytest.fixture(scope="module")
def libs():
    subprocess.run(["make", "-s", "-C", EMUL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", EMUL_DIR, "-f", "Makefile.text"], check=True)
    return os.path.join(EMUL_DIR, "libtgsf_emul.so"), os.path.join(EMUL_DIR, "libtgsf_text_emul.so")


@pytest.fixture(scope="module")
def tlib(libs):
    return libs[1]


def test_load_insists_on_the_hip_build(tlib, monkeypatch):
    assert tgtext.load(tlib).tgsf_text_backend() == b"emulation"
    monkeypatch.setattr(tgtext, "DEFAULT_LIB", tlib)
    with pytest.raises(RuntimeError, match="not the HIP build"):
        tgtext.load()


@pytest.mark.parametrize("kind", ["ont", "hifi"])
def test_well_formed(tlib, kind):
    reads = synth.make_reads(3, 40, kind, mean_len=3000, zoo=True)
    for eol in (b"\n", b"\r\n"):
        recs, consumed, stop = textparity.check_text(tlib, textparity.fastq_of(reads, eol))
        assert len(recs) == len(reads) and stop == tgtext.END
        recs, consumed, stop = textparity.check_text(tlib, textparity.fasta_of(reads, eol), fasta=True)
        assert len(recs) == len(reads) and stop == tgtext.END
    text = textparity.fastq_of(reads)
    recs, consumed, stop = textparity.check_text(tlib, text[:-1])                   # no final newline
    assert len(recs) == len(reads) and consumed == len(text) - 1 and stop == tgtext.END
    recs, consumed, stop = textparity.check_text(tlib, text[:-1], final=False)      # ... which in a non-final chunk is a tail
    assert len(recs) == len(reads) - 1 and stop == tgtext.END


def test_unusual_texts(tlib):
    for i, text in enumerate(textparity.unusual_texts()):
        textparity.check_text(tlib, text, what=i)


def test_every_damage_class(tlib):
    stops = set()
    for damage, fasta, text in textparity.damaged_texts():
        for final in (True, False):
            stops.add(textparity.check_text(tlib, text, fasta=fasta, final=final, what=(damage, fasta, final, text))[2])
    assert stops == {tgtext.END, tgtext.IRREGULAR}


def test_lines_longer_than_a_piece_and_a_block(tlib):
    reads = textparity.long_line_text()
    recs, _, stop = textparity.check_text(tlib, textparity.fastq_of(reads))
    assert len(recs) == len(reads) and stop == tgtext.END
    textparity.check_text(tlib, textparity.fasta_of(reads), fasta=True)


def test_no_newline_and_empty(tlib):
    for text in (b"", b"@", b"A" * 10000, b"\n", b"\n" * 9000, b"\r\n\r\n", b"@a\nA\n+\nI"):
        for fasta in (False, True):
            for final in (True, False):
                textparity.check_text(tlib, text, fasta=fasta, final=final, what=(text[:20], fasta, final))


def test_more_scan_blocks_than_one(tlib):
    """More than 4 096 pieces (16 MiB): the offsets of k_text_scan_top count."""
    reads = synth.make_reads(9, 300, "ont", mean_len=3000, zoo=False)
    block = textparity.fastq_of(reads)
    text = block * (17_500_000 // len(block) + 1)
    recs, _, stop = textparity.check_text(tlib, text)
    assert len(recs) == 300 * (17_500_000 // len(block) + 1) and stop == tgtext.END


def test_capacity_then_the_rest(tlib):
    reads = synth.make_reads(4, 23, "ont", mean_len=500, zoo=False)
    textparity.capacity_then_rest(tlib, textparity.fastq_of(reads), False, 5)
    textparity.capacity_then_rest(tlib, textparity.fasta_of(reads[:20]), True, 5)        # an exact multiple
    textparity.capacity_then_rest(tlib, textparity.fastq_of(reads) + b"@x\n\n", False, 23)


def test_cut_at_every_byte(tlib):
    rng = np.random.default_rng(17)
    textparity.cut_everywhere(tlib, textmodel.make_text(rng, False, n_records=5, max_len=30), False)
    textparity.cut_everywhere(tlib, textmodel.make_text(rng, False, n_records=4, damage="crlf", max_len=30), False)
    textparity.cut_everywhere(tlib, textmodel.make_text(rng, True, n_records=6, max_len=30), True)
    textparity.cut_everywhere(tlib, textmodel.make_text(rng, False, n_records=5, damage="no_final_newline", max_len=30), False)


def test_fuzz_forward(tlib):
    n = 2000
    assert textparity.fuzz(tlib, 1001, n) >= n // 4


def test_fuzz_reverse_lane_order(tlib):
    """TGSF_EMUL_ORDER=reverse: lanes and blocks run last to first (tgsf_emul_rt.h); in a process of its own, the order is read per launch
    but the environment belongs to the whole session."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom tests import textparity\nn = 2000\n"
            "assert textparity.fuzz(%r, 1002, n) >= n // 4\nprint('fuzz ok')\n" % (ROOT, tlib))
    env = dict(os.environ, TGSF_EMUL_ORDER="reverse")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, env=env, timeout=900)
    assert p.returncode == 0 and b"fuzz ok" in p.stdout, p.stderr.decode()[-2000:]


# ---- the one-call form: text in, filter results out -----------------------------------------------------------------
def test_chained_ont(libs):
    reads = synth.make_reads(31, 30, "ont", mean_len=2500, zoo=True, pmid=0.1)
    textparity.chained(libs[0], libs[1], "ont", reads, min_q=9.0, head_trim=5, tail_trim=3)


def test_chained_hifi(libs):
    reads = synth.make_reads(32, 24, "hifi", mean_len=4000, zoo=True, pmid=0.3)
    textparity.chained(libs[0], libs[1], "hifi", reads, min_q=20.0)


def test_chained_fasta_no_qual(libs):
    reads = synth.make_reads(33, 30, "ont", mean_len=2500, zoo=True, pmid=0.1)
    textparity.chained(libs[0], libs[1], "ont", reads, fasta=True, min_q=9.0)


def test_chained_garbage_in_the_padding(libs):
    reads = synth.make_reads(34, 20, "ont", mean_len=2000, zoo=True, pmid=0.1)
    textparity.chained(libs[0], libs[1], "ont", reads, garbage_in_padding=True, min_q=9.0)


def test_chained_irregular_tail(libs):
    textparity.irregular_tail(*libs)


def test_chained_refusals(libs):
    textparity.refusals(*libs)
