"""Test infrastructure: the sequential FASTQ / FASTA reader of the command line restated in Python
(tgsfilter_amd/host/fastx.cpp, FastxReader::line / next_fastq / next_fasta; the reference's getLine / readFastq / readFasta,
src/TGSFilter.cpp:657-760), the parallel rule of include/tgsf_text.h derived from the same lines, and a generator of texts
with every kind of damage.  tests/test_text_model.py pins the reader against the command line itself."""
from __future__ import annotations

import numpy as np

END, IRREGULAR, CAPACITY = 0, 1, 2


class Reader:
    """FastxReader over text[start:] as one final input."""

    def __init__(self, text: bytes, fastq=True, start=0):
        self.t, self.p, self.fastq = text, start, fastq
        self.done = False
        self.message = None

    def line(self):
        """(offset, length) of the next line; an exhausted input gives an empty line and sets done."""
        t, p = self.t, self.p
        if p >= len(t):
            self.done = True
            return (p, 0)
        nl = t.find(b"\n", p)
        e = nl if nl >= 0 else len(t)
        n = e - p
        if n > 0 and t[e - 1] == 13:
            n -= 1
        self.p = nl + 1 if nl >= 0 else len(t)
        return (p, n)

    def _first(self, ln):
        return self.t[ln[0]] if ln[1] else -1

    def _name(self, ln):
        return self.t[ln[0] + 1:ln[0] + ln[1]]

    def next(self):
        """The next record as (name_off, name_len, seq_off, qual_off, len), or None (message holds the reader's words, if any)."""
        return self.next_fastq() if self.fastq else self.next_fasta()

    def next_fastq(self):
        name = seq = strand = (0, 0)
        for _ in range(5):
            name = self.line()
            if self._first(name) == 64:
                seq = self.line()
                strand = self.line()
                if self._first(strand) == 43 and seq[1] > 0:
                    break
        if self.done:
            return None
        if name[1] == 0:
            self.message = b"Error: input format wrong!"
            return None
        qual = self.line()
        if qual[1] == 0:
            self.message = b"Error: quality are empty:" + self._name(name)
            return None
        if qual[1] != seq[1]:
            self.message = b"warning: sequence and quality have different length:" + self._name(name)
            return None
        return (name[0] + 1, name[1] - 1, seq[0], qual[0], seq[1])

    def next_fasta(self):
        name = (0, 0)
        for _ in range(3):
            name = self.line()
            if self._first(name) == 62:
                break
        if self.done:
            return None
        if name[1] == 0:
            self.message = b"Error: input format wrong!"
            return None
        seq = self.line()
        if seq[1] == 0:
            self.message = b"Error: sequence are empty:" + self._name(name)
            return None
        return (name[0] + 1, name[1] - 1, seq[0], seq[0], seq[1])


def read_all(text: bytes, fastq=True, start=0):
    """Every record the sequential reader yields from text[start:], and its last message (None: it just ended)."""
    r = Reader(text, fastq, start)
    recs = []
    while True:
        rec = r.next()
        if rec is None:
            return recs, r.message
        recs.append(rec)


def lines_of(text: bytes, final=True):
    """(start, length without a trailing CR, start of the next line) of every line of the chunk."""
    out = []
    p = 0
    while p < len(text):
        nl = text.find(b"\n", p)
        if nl < 0:
            if not final:
                break
            e, nxt = len(text), len(text)
        else:
            e, nxt = nl, nl + 1
        n = e - p
        if n > 0 and text[e - 1] == 13:
            n -= 1
        out.append((p, n, nxt))
        p = nxt
    return out


def rule(text: bytes, fasta=False, final=True, max_records=1 << 30):
    """The rule of include/tgsf_text.h: (records, consumed, stop); records as read_all returns them."""
    G = 2 if fasta else 4
    ln = lines_of(text, final)
    groups = min(len(ln) // G, max_records)
    recs = []
    for g in range(groups):
        L = ln[G * g:G * g + G]
        ok = L[0][1] > 0 and text[L[0][0]] == (62 if fasta else 64) and L[1][1] > 0
        if not fasta:
            ok = ok and L[2][1] > 0 and text[L[2][0]] == 43 and L[3][1] > 0 and L[3][1] == L[1][1]
        if not ok:
            break
        recs.append((L[0][0] + 1, L[0][1] - 1, L[1][0], L[1][0] if fasta else L[3][0], L[1][1]))
    k = len(recs)
    left = len(ln) - G * k
    if k < groups:
        stop = IRREGULAR
    elif left == 0:
        stop = END
    elif k == max_records:
        stop = CAPACITY
    else:
        stop = IRREGULAR if final else END
    return recs, (ln[G * k - 1][2] if k else 0), stop


def expected_index(recs):
    """The five arrays of tgsf_text_index_arrays from record tuples."""
    a = np.array(recs, dtype=np.int64).reshape(-1, 5)
    return {"name_off": a[:, 0].astype(np.uint64), "name_len": a[:, 1].astype(np.uint32), "seq_off": a[:, 2].astype(np.uint64),
            "qual_off": a[:, 3].astype(np.uint64), "len": a[:, 4].astype(np.uint32)}


# ---- texts ------------------------------------------------------------------------------------------------------
DAMAGE = ("none", "blank_line", "missing_line", "unequal", "empty_qual", "bad_header", "lone_cr", "crlf", "no_final_newline", "garbage")


def make_text(rng, fasta=False, n_records=None, damage="none", max_len=60, cli_safe=False):
    """A small FASTQ / FASTA text of n_records records with one kind of damage at a random record (none: well-formed).
    cli_safe: quality and garbage bytes that the command line takes as Phred+64 qualities whatever line they end up in (its
    pre-pass sees no read this short and settles on Phred+64; a mean quality below 0 ends a run)."""
    n = int(rng.integers(0, 7)) if n_records is None else n_records
    eol = b"\r\n" if damage == "crlf" else b"\n"
    hit = int(rng.integers(0, n)) if n else -1
    out = []
    for i in range(n):
        L = int(rng.integers(1, max_len))
        name = (b">" if fasta else b"@") + b"r%d" % i + (b" x" if rng.random() < 0.3 else b"")
        seq = bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, L)])
        qual = bytes((rng.integers(0, 40, L) + (70 if cli_safe else 33)).astype(np.uint8))
        plus = b"+" + (name[1:] if rng.random() < 0.2 else b"")
        lines = [name, seq] if fasta else [name, seq, plus, qual]
        if i == hit:
            k = int(rng.integers(0, len(lines)))
            if damage == "blank_line":
                lines.insert(k, b"")
            elif damage == "missing_line":
                del lines[k]
            elif damage == "unequal":
                lines[-1] = lines[-1] + b"I" if rng.random() < 0.5 else lines[-1][:-1]
            elif damage == "empty_qual":
                lines[-1] = b""
            elif damage == "bad_header":
                lines[0] = b"r%d" % i if rng.random() < 0.5 else b"#" + lines[0]
            elif damage == "lone_cr":
                lines.insert(k, b"\r")
            elif damage == "garbage":
                lines.insert(k, bytes(rng.integers(70 if cli_safe else 1, 127 if cli_safe else 256, int(rng.integers(1, 20)), dtype=np.uint8)).replace(b"\n", b" "))
        out.append(eol.join(lines) + eol)
    text = b"".join(out)
    if damage == "no_final_newline" and text:
        text = text[:-len(eol)]
    return text
