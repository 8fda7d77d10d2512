"""The rule of the BAM input side of libtgsf_text (include/tgsf_text.h, tgsf_text_bam_*), restated in numpy / Python from the
header's words: the record chain, which records are regular, the decoded FASTQ text, its index, where the index ends and
why.  tests/bamparity.py compares the library with it word for word; tests/test_bam_emul.py pins it to the reference's own
output files first."""
from __future__ import annotations

import struct

import numpy as np

END, IRREGULAR, CAPACITY = 0, 1, 2
NO_BAD_QUAL = 0xFFFFFFFF
PAD = 64
NT16 = np.frombuffer(b"\0AC\0G\0\0\0T\0\0\0\0\0\0N", dtype=np.uint8)     # the reference's table (src/TGSFilter.cpp:31): other codes are NUL
assert NT16.size == 16
FIELDS = ("seq_off", "qual_off", "len", "name_off", "name_len")


def header(bam: bytes):
    """The offset of the first record, or None when the magic is wrong or the header is not complete."""
    if len(bam) < 8 or bam[:4] != b"BAM\1":
        return None
    at = 8 + struct.unpack_from("<I", bam, 4)[0]
    if at + 4 > len(bam):
        return None
    n_ref = struct.unpack_from("<I", bam, at)[0]
    at += 4
    for _ in range(n_ref):
        if at + 4 > len(bam):
            return None
        at += 4 + struct.unpack_from("<I", bam, at)[0] + 4
        if at > len(bam):
            return None
    return at


def walk(bam: bytes, final: bool, max_records: int):
    """tgsf_text_bam_walk: (offsets of the records walked plus the offset behind them, stop)."""
    off, at, n = [0], 0, len(bam)
    while True:
        if at == n:
            return off, END
        if len(off) - 1 == max_records:
            return off, CAPACITY
        if n - at < 4:
            return off, IRREGULAR if final else END
        block = struct.unpack_from("<I", bam, at)[0]
        if block < 32:
            return off, IRREGULAR
        if n - at - 4 < block:
            return off, IRREGULAR if final else END
        at += 4 + block
        off.append(at)


def fields(bam: bytes, at: int):
    """(regular, name, l_seq, o_seq, o_qual) of the complete record whose block_size is at `at`; offsets are from `at` + 4."""
    block = struct.unpack_from("<I", bam, at)[0]
    r = at + 4
    l_read_name, n_cigar, l_seq = bam[r + 8], struct.unpack_from("<H", bam, r + 12)[0], struct.unpack_from("<I", bam, r + 16)[0]
    o_seq = 32 + l_read_name + 4 * n_cigar
    o_qual = o_seq + (l_seq + 1) // 2
    if not (block >= 32 and o_qual + l_seq <= block and l_seq > 0):
        return False, b"", l_seq, o_seq, o_qual
    name = bam[r + 32:r + 32 + l_read_name]
    return True, name.split(b"\0", 1)[0], l_seq, o_seq, o_qual


def piece(bam: bytes, at: int, name: bytes, l_seq: int, o_seq: int, o_qual: int):
    """One record's text and whether a quality decodes to a line end."""
    r = at + 4
    packed = np.frombuffer(bam, np.uint8, (l_seq + 1) // 2, r + o_seq)
    codes = np.empty(2 * packed.size, np.uint8)
    codes[0::2], codes[1::2] = packed >> 4, packed & 15
    q = (np.frombuffer(bam, np.uint8, l_seq, r + o_qual).astype(np.uint16) + 33).astype(np.uint8)      # (uint8_t)(q + 33)
    return b"@" + name + b"\n" + NT16[codes[:l_seq]].tobytes() + b"\n+\n" + q.tobytes() + b"\n", bool((q == 10).any())


def rule(bam: bytes, final: bool, max_records: int, max_bytes: int):
    """What one decode of the chunk gives: dict of text, index (the five arrays), n_records, stop, consumed, text_bytes, bases,
    longest, bad_qual."""
    bam = bytes(bam)
    off, stop = walk(bam, final, max_records)
    parts, idx, pos, bad = [], {f: [] for f in FIELDS}, 0, NO_BAD_QUAL
    k = 0
    for k, at in enumerate(off[:-1]):
        ok, name, l_seq, o_seq, o_qual = fields(bam, at)
        if not ok:
            stop = IRREGULAR
            break
        if pos + len(name) + 2 * l_seq + 6 > max_bytes:
            stop = CAPACITY
            break
        text, newline = piece(bam, at, name, l_seq, o_seq, o_qual)
        assert len(text) == len(name) + 2 * l_seq + 6
        if newline and bad == NO_BAD_QUAL:
            bad = k
        idx["name_off"].append(pos + 1)
        idx["name_len"].append(len(name))
        idx["seq_off"].append(pos + 2 + len(name))
        idx["qual_off"].append(pos + 2 + len(name) + l_seq + 3)
        idx["len"].append(l_seq)
        parts.append(text)
        pos += len(text)
    else:
        k = len(off) - 1
    index = {f: np.array(idx[f], dtype=np.uint32 if f in ("len", "name_len") else np.uint64) for f in FIELDS}
    return {"text": b"".join(parts), "index": index, "n_records": k, "stop": stop, "consumed": off[k], "text_bytes": pos,
            "bases": int(index["len"].astype(np.uint64).sum()), "longest": int(index["len"].max()) if k else 0, "bad_qual": bad}


def reads_of(bam: bytes):
    """[(name, seq, qual)] of a whole clean chain: what the host's decode_bam hands to the FASTQ path."""
    m = rule(bam, True, 1 << 30, 1 << 62)
    assert m["stop"] == END and m["consumed"] == len(bam)
    lines = m["text"].split(b"\n")[:-1]
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines), 4)]
