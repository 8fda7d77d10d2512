"""tests/textmodel.py pinned: its restatement of the sequential reader (FastxReader, tgsfilter_amd/host/fastx.cpp) against
the command line itself.  With -F -r <more reads than the file holds> every record read is written back unchanged and in
order, and the reader's words go to stderr (more than once: the pre-pass reads the file too; compared as a set).  Where
oracle/_ref/tgsfilter_ref exists, the reference reads the texts it can read (LF line ends, a final newline) as well.
Then the rule of include/tgsf_text.h against that reader, from the model alone."""
import os
import subprocess

import numpy as np
import pytest

from tests import textmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "tgsfilter_ref")


@pytest.fixture(scope="module")
def binary():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "host"), "emul"], check=True)
    return os.path.join(ROOT, "tests", "emul", "tgsfilter_emul")


def rendered(text, recs, fasta):
    out = []
    for name_off, name_len, seq_off, qual_off, n in recs:
        name = text[name_off:name_off + name_len]
        if fasta:
            out.append(b">" + name + b"\n" + text[seq_off:seq_off + n] + b"\n")
        else:
            out.append(b"@" + name + b"\n" + text[seq_off:seq_off + n] + b"\n+\n" + text[qual_off:qual_off + n] + b"\n")
    return b"".join(out)


def run_cli(binary, text, fasta, tmp_path, tag):
    ext = "fa" if fasta else "fq"
    fin, fout = tmp_path / f"{tag}.in.{ext}", tmp_path / f"{tag}.out.{ext}"
    fin.write_bytes(text)
    p = subprocess.run([binary, "-i", str(fin), "-o", str(fout), "-t", "1", "-F", "-r", "100000"], capture_output=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr.decode()[-1500:]
    said = {l for l in p.stderr.split(b"\n") if l.startswith((b"Error:", b"warning:"))}
    return fout.read_bytes(), said


def texts(seed, per_class):
    """Texts of every damage class whose first record is sound (a command line that reads nothing ends otherwise)."""
    rng = np.random.default_rng(seed)
    for damage in textmodel.DAMAGE:
        for i in range(per_class):
            fasta = bool(i % 3 == 2)
            while True:
                t = textmodel.make_text(rng, fasta, n_records=int(rng.integers(2, 8)), damage=damage, cli_safe=True)
                if textmodel.read_all(t, not fasta)[0]:
                    break
            yield damage, fasta, t


def test_reader_model_equals_the_command_line(binary, tmp_path):
    for k, (damage, fasta, t) in enumerate(texts(7, 3)):
        recs, msg = textmodel.read_all(t, not fasta)
        out, said = run_cli(binary, t, fasta, tmp_path, "e%d" % k)
        assert out == rendered(t, recs, fasta), (damage, fasta, t)
        assert said == ({msg} if msg else set()), (damage, fasta, t, said, msg)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/tgsfilter_ref not built (make -C oracle ref)")
def test_reader_model_equals_the_reference(tmp_path):
    rng = np.random.default_rng(3)
    good = textmodel.make_text(rng, False, n_records=6, cli_safe=True)
    good = rendered(good, textmodel.read_all(good)[0], False)              # (plain "+" lines: those are what is written)
    out, said = run_cli(REF, good, False, tmp_path, "good")
    assert out == good and out.count(b"\n+\n") == 6 and not said          # the identity on a well-formed file first
    k = 0
    for damage, fasta, t in texts(8, 2):
        if damage in ("crlf", "no_final_newline", "lone_cr", "garbage"):      # texts the reference reads out of bounds or byte-dependently
            continue
        recs, msg = textmodel.read_all(t, not fasta)
        out, said = run_cli(REF, t, fasta, tmp_path, "r%d" % k)
        k += 1
        assert out == rendered(t, recs, fasta), (damage, fasta, t)
        assert said == ({msg} if msg else set()), (damage, fasta, t, said, msg)


def test_rule_is_a_prefix_of_the_reader_and_the_reader_resumes_at_consumed():
    """The records of the rule are the first records of the sequential reader; started again at `consumed` the reader yields the
    rest and the same message -- final chunks and chunks cut at any byte."""
    rng = np.random.default_rng(5)
    to_end = 0
    n = 6000
    for i in range(n):
        fasta = bool(rng.random() < 0.4)
        damage = textmodel.DAMAGE[int(rng.integers(0, len(textmodel.DAMAGE)))] if rng.random() < 0.6 else "none"
        t = textmodel.make_text(rng, fasta, damage=damage)
        everything, msg = textmodel.read_all(t, not fasta)
        recs, consumed, stop = textmodel.rule(t, fasta, True)
        rest, msg2 = textmodel.read_all(t, not fasta, consumed)
        assert recs + rest == everything and msg == msg2, (damage, fasta, t)
        assert stop != textmodel.CAPACITY and (stop == textmodel.IRREGULAR or (not rest and consumed == len(t)))
        to_end += stop == textmodel.END
        cut = int(rng.integers(0, len(t) + 1))
        recs, consumed, stop = textmodel.rule(t[:cut], fasta, False)
        rest, msg2 = textmodel.read_all(t, not fasta, consumed)
        assert recs + rest == everything and msg == msg2, (damage, fasta, t, cut)
        recs3, consumed3, stop3 = textmodel.rule(t, fasta, True, max_records=2)
        assert recs3 == textmodel.rule(t, fasta, True)[0][:2] and (stop3 == textmodel.CAPACITY) == (len(recs3) == 2 and consumed3 < len(t))
    assert to_end >= n // 4
