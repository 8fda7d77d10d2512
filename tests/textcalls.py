"""What the four host entry points of libtgsf_text that run the filter -- tgsf_text_submit, tgsf_text_filter,
tgsf_text_bam_submit, tgsf_text_bam_filter -- leave in the caller's memory, on success and on every way a call ends early.
The calls go through TextIndexer.lib with the caller's own structs and buffers, every one of them filled with 0xA5 first, so
that each output is seen to be untouched, zeroed or filled, byte for byte.  The expectations are the library's behaviour as
tgsf_text.hip had it when this file was written; where the text calls and the BAM calls differ (the input summary of a call
that the filter refuses) the difference is pinned as it is.  tests/test_textcalls_emul.py and tests/test_textcalls_gpu.py
run the cases."""
from __future__ import annotations

import ctypes as C
import functools
import struct

import numpy as np

from tests import bammodel as bm, bamparity as bp, textmodel, textoutparity as top, textparity
from tgsfilter_amd import abi, capi, synth, text as tgtext

CALLS = ("submit", "filter", "bam_submit", "bam_filter")
FIELDS = textparity.FIELDS
WIDTH = {"seq_off": 8, "qual_off": 8, "len": 4, "name_off": 8, "name_len": 4}
MAX_RECORDS, FRAG_ROOM, MAX_FRAGS = 8, 16, 64
OK, E_INVALID, E_CAPACITY, E_DATA = abi.OK, abi.E_INVALID, abi.E_CAPACITY, abi.E_DATA
A5 = 0xA5


def is_bam(call):
    return call.startswith("bam")


def is_filter(call):
    return call.endswith("filter")


# ---- the input: six records, the third split into two kept fragments by an adapter in its middle ------------------------
@functools.lru_cache(maxsize=None)
def world():
    """The records, their text and their BAM, the parameters, and what the oracle and the output model make of them: once."""
    rng = np.random.default_rng(7)
    reads = []
    for i, L in enumerate((40, 120, 300, 77, 210, 150)):
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)])
        if L == 300:
            s = s[:120] + synth.PACBIO_BLUNT + s[120 + len(synth.PACBIO_BLUNT):]
        reads.append((b"r%d x" % i, s, bytes((rng.integers(25, 40, L) + 33).astype(np.uint8))))
    text = textparity.fastq_of(reads)
    code = {65: 1, 67: 2, 71: 4, 84: 8}
    recs = [bp.record(n + b"\0", [code[c] for c in s], bytes(c - 33 for c in q)) for n, s, q in reads]
    p = params(reads, text)
    ix, er, ef = top.oracle_on_text(p, text)
    assert len(er) == 6 and len(ef) == 7 and int(er["n_frags"][2]) == 2 and ((ef["flags"] & abi.FF_PASS) != 0).all()
    etext, eends, ebases = top.expected(text, ix, er, ef, True)
    assert len(eends) == 7 and b"@r2:2 x\n" in etext
    return dict(reads=reads, text=text, recs=recs, bam=b"".join(recs), ix=ix, er=er, ef=ef, out=etext, ends=eends, bases=ebases)


def params(reads, text, max_batch_reads=None):
    p = textparity.params_for("hifi", reads, len(text) + 64, min_q=5.0, end_len=20, extra_len=0, min_len=100)
    p.min_len = 30
    if max_batch_reads is not None:
        p.max_batch_reads = max_batch_reads
    return p


def bad_quality_bam():
    """The BAM with a quality byte of 233 (which decodes to '\\n') in record 2."""
    recs = list(world()["recs"])
    r = bytearray(recs[2])
    l_seq, o = struct.unpack_from("<I", r, 20)[0], 4 + 32 + r[12] + 4 * struct.unpack_from("<H", r, 16)[0]
    r[o + (l_seq + 1) // 2 + 100] = 233
    recs[2] = bytes(r)
    return b"".join(recs)


def chunk_of(call, kind):
    """The input of a case: "good", "empty", or "irregular" (the first group of lines / the first record is not regular)."""
    W = world()
    if kind == "good":
        return W["bam"] if is_bam(call) else W["text"]
    if kind == "empty":
        return b""
    assert kind == "irregular"
    return bp.record(b"z\0", [], b"") + W["bam"] if is_bam(call) else b"garbage\n" + W["text"]


# ---- the caller's memory --------------------------------------------------------------------------------------------------
class Outputs:
    """Every output a caller passes, filled with 0xA5."""

    def __init__(self, call, out_room):
        self.call = call
        self.in_summary = (tgtext.BamSummary if is_bam(call) else tgtext.Summary)()
        self.out_summary = tgtext.OutSummary()
        C.memset(C.byref(self.in_summary), A5, C.sizeof(self.in_summary))
        C.memset(C.byref(self.out_summary), A5, C.sizeof(self.out_summary))
        self.reads = np.full(MAX_RECORDS * 32, A5, np.uint8)
        self.frags = np.full(FRAG_ROOM * 24, A5, np.uint8)
        self.out = np.full(out_room, A5, np.uint8)
        self.rec_end = np.full(MAX_FRAGS * 8, A5, np.uint8)
        self.index = {f: np.full(MAX_RECORDS * WIDTH[f], A5, np.uint8) for f in FIELDS}
        self.ia = tgtext.IndexArrays(*[self.index[f].ctypes.data for f in FIELDS])
        self.bo = abi.BatchOut(self.reads.ctypes.data, self.frags.ctypes.data, FRAG_ROOM, 0xA5A5A5A5)

    def state(self, with_bo, with_out_summary):
        """The bytes of every output, by name."""
        s = {"in_summary": bytes(self.in_summary), "reads": self.reads.tobytes(), "frags": self.frags.tobytes()}
        for f in FIELDS:
            s[f] = self.index[f].tobytes()
        if with_bo:
            s["n_frags"] = self.bo.n_frags
            assert (self.bo.reads, self.bo.frags) == (self.reads.ctypes.data, self.frags.ctypes.data)
        if is_filter(self.call):
            s["out"], s["rec_end"] = self.out.tobytes(), self.rec_end.tobytes()
            if with_out_summary:
                s["out_summary"] = bytes(self.out_summary)
        return s


def _prefix(filled, room):
    """`filled` in front of 0xA5 up to `room` bytes."""
    filled = bytes(filled)
    assert len(filled) <= room
    return filled + bytes([A5]) * (room - len(filled))


def in_summary_bytes(call, chunk):
    """The input summary of a call on `chunk`, from the models."""
    if is_bam(call):
        m = bm.rule(chunk, True, MAX_RECORDS, 1 << 30)
        return bytes(tgtext.BamSummary(m["n_records"], m["stop"], m["consumed"], m["text_bytes"], m["bases"], m["longest"], m["bad_qual"], 0.0, 0))
    recs, consumed, stop = textmodel.rule(chunk, False, True, MAX_RECORDS)
    lens = [r[4] for r in recs]
    return bytes(tgtext.Summary(len(recs), stop, consumed, sum(lens), max(lens, default=0), 0.0))


def expected(call, stage, chunk, out_room, with_bo=True, with_out_summary=True):
    """The caller's memory after a call that got as far as `stage`:
         "args"      refused for its arguments: nothing is touched
         "refused"   the input is in the object and counted, the filter refuses it (libtgsf's refusals, the fragment room, for
                     BAM a bad quality): n_frags is 0, the filter's out_summary is zeroed, and the input summary is filled by the
                     BAM calls and left alone by the text calls
         "nothing"   no record: TGSF_OK, the input summary filled, n_frags 0, out_summary zeroed
         "filtered"  the filter has run and everything of it and the index is down; the format has not begun (max_frags)
         "sized"     ... and the format has found the output too large: out_summary tells the need
         "ok"        everything."""
    W = world()
    s = {"in_summary": _prefix(b"", 48 if is_bam(call) else 32), "reads": _prefix(b"", MAX_RECORDS * 32), "frags": _prefix(b"", FRAG_ROOM * 24)}
    for f in FIELDS:
        s[f] = _prefix(b"", MAX_RECORDS * WIDTH[f])
    if with_bo:
        s["n_frags"] = 0xA5A5A5A5
    if is_filter(call):
        s["out"], s["rec_end"] = _prefix(b"", out_room), _prefix(b"", MAX_FRAGS * 8)
        if with_out_summary:
            s["out_summary"] = _prefix(b"", 32)
    if stage == "args":
        return s
    if with_bo:
        s["n_frags"] = 0
    if is_filter(call):
        s["out_summary"] = bytes(32)
    if stage != "refused" or is_bam(call):
        s["in_summary"] = in_summary_bytes(call, chunk)
    if stage in ("refused", "nothing"):
        return s
    for f in FIELDS:
        s[f] = _prefix(W["ix"][f].tobytes(), MAX_RECORDS * WIDTH[f])
    if with_bo:
        s["n_frags"] = len(W["ef"])
        s["reads"] = _prefix(W["er"].tobytes(), MAX_RECORDS * 32)
        s["frags"] = _prefix(W["ef"].tobytes(), FRAG_ROOM * 24)
    if stage == "filtered" or not is_filter(call):
        return s
    fits = stage == "ok"
    s["out_summary"] = bytes(tgtext.OutSummary(len(W["out"]), W["bases"], len(W["ends"]), tgtext.END if fits else tgtext.CAPACITY, 0.0, 0))
    if fits:
        s["out"], s["rec_end"] = _prefix(W["out"], out_room), _prefix(W["ends"].tobytes(), MAX_FRAGS * 8)
    return s


# ---- the calls --------------------------------------------------------------------------------------------------------------
class Rig:
    """Two objects (the second with an output side reserved for three fragments only) and two contexts (the second takes three
    reads a batch)."""

    def __init__(self, lib, text_lib):
        W = world()
        self.out_room = len(W["out"]) + 64
        room_text, room_bam = len(W["text"]) + 64, len(W["bam"]) + 256
        self.tx, self.tx_small = (tgtext.TextIndexer(0, room_text, MAX_RECORDS, text_lib) for _ in range(2))
        self.ctx = self.ctx3 = None
        try:
            self.tx.reserve_output(MAX_FRAGS, 4 * room_text)
            self.tx_small.reserve_output(3, 4 * room_text)
            for t in (self.tx, self.tx_small):
                t.reserve_bam(room_bam)
            self.ctx = capi.Context(params(W["reads"], W["text"]), 0, lib)
            self.ctx3 = capi.Context(params(W["reads"], W["text"], 3), 0, lib)
        except BaseException:
            self.close()
            raise

    def close(self):
        for x in (self.ctx, self.ctx3, self.tx, self.tx_small):
            if x is not None:
                x.close()

    def call(self, call, chunk, tx=None, ctx=None, with_bo=True, with_out_summary=True, frag_capacity=FRAG_ROOM, out_capacity=None):
        """One call with fresh 0xA5 memory: (return code, the object's error text, the state of the caller's memory)."""
        tx, ctx = tx or self.tx, ctx or self.ctx
        o = Outputs(call, self.out_room)
        o.bo.frag_capacity = frag_capacity
        b = np.frombuffer(chunk, np.uint8)
        L = tx.lib
        ins, outs = C.byref(o.in_summary), C.byref(o.out_summary) if with_out_summary else None
        bo = C.byref(o.bo) if with_bo else None
        cap = self.out_room if out_capacity is None else out_capacity
        if call == "submit":
            rc = L.tgsf_text_submit(tx.h, ctx.h, b.ctypes.data, b.size, 0, 1, C.byref(o.ia), ins if with_out_summary else None, bo)
        elif call == "bam_submit":
            rc = L.tgsf_text_bam_submit(tx.h, ctx.h, b.ctypes.data, b.size, 1, C.byref(o.ia), ins if with_out_summary else None, bo)
        elif call == "filter":
            rc = L.tgsf_text_filter(tx.h, ctx.h, b.ctypes.data, b.size, 0, 1, 1, o.out.ctypes.data, cap, o.rec_end.ctypes.data, outs, ins, C.byref(o.ia), bo)
        else:
            rc = L.tgsf_text_bam_filter(tx.h, ctx.h, b.ctypes.data, b.size, 1, 1, o.out.ctypes.data, cap, o.rec_end.ctypes.data, outs, ins, C.byref(o.ia), bo)
        assert o.bo.frag_capacity == frag_capacity
        return rc, L.tgsf_text_last_error(tx.h).decode(), o.state(with_bo, with_out_summary)

    def check(self, call, stage, code, words, kind="good", chunk=None, tx=None, **kw):
        """One case: the return code, the words of the error text, every output; then the good call on the same object."""
        chunk = chunk_of(call, kind) if chunk is None else chunk
        rc, err, got = self.call(call, chunk, tx=tx, **kw)
        assert rc == code, (call, stage, rc, err)
        for w in words:
            assert w in err, (call, stage, w, err)
        exp = expected(call, stage, chunk, self.out_room, kw.get("with_bo", True), kw.get("with_out_summary", True))
        for k in exp:
            assert got[k] == exp[k], (call, stage, k, got[k][:64] if isinstance(got[k], bytes) else got[k], exp[k][:64] if isinstance(exp[k], bytes) else exp[k])
        assert set(got) == set(exp)
        if stage != "ok":
            self.good(call, tx)

    def good(self, call, tx=None):
        if tx is self.tx_small:                                        # (its output side has no room for a good filter call)
            call = call.replace("filter", "submit")
        rc, err, got = self.call(call, chunk_of(call, "good"), tx=tx)
        assert rc == OK, (call, err)
        assert got == expected(call, "ok", chunk_of(call, "good"), self.out_room), (call, "the good call afterwards")


# ---- the cases: each takes a Rig and one of CALLS ---------------------------------------------------------------------------
def success(rig, call):
    rig.check(call, "ok", OK, ())
    if is_filter(call):                                                # the same without a batch_out: nothing of the filter comes down
        rig.check(call, "ok", OK, (), with_bo=False)


def no_records(rig, call):
    for kind in ("empty", "irregular"):
        rig.check(call, "nothing", OK, (), kind=kind)
        if is_filter(call):
            rig.check(call, "nothing", OK, (), kind=kind, with_bo=False)


def refused_by_libtgsf(rig, call):
    rig.check(call, "refused", E_CAPACITY, ("libtgsf", "6 reads", "sized for 3"), ctx=rig.ctx3)


def fragment_room_of_one(rig, call):
    rig.check(call, "refused", E_CAPACITY, ("fragment",), frag_capacity=1)


def output_too_small(rig, call):
    assert is_filter(call)
    need = len(world()["out"])
    rig.check(call, "sized", E_CAPACITY, ("formatted text has %d bytes" % need, "room for %d" % (need - 16)), out_capacity=need - 16)


def more_fragments_than_reserved(rig, call):
    """With the caller's fragment room the filter runs and the call stops in front of the format; without it the object's own
    room is max_frags, and libtgsf refuses."""
    assert is_filter(call)
    rig.check(call, "filtered", E_CAPACITY, ("7 fragments", "reserved for 3"), tx=rig.tx_small)
    rig.check(call, "refused", E_CAPACITY, ("fragment",), tx=rig.tx_small, with_bo=False)


def bad_quality(rig, call):
    assert is_bam(call)
    rig.check(call, "refused", E_DATA, ("quality", "r2 x", "record 2", "has not run"), chunk=bad_quality_bam())


def null_out_summary(rig, call):
    rig.check(call, "args", E_INVALID, ("null argument",), with_out_summary=False)


CASES = {"success": (success, CALLS), "no_records": (no_records, CALLS), "refused_by_libtgsf": (refused_by_libtgsf, CALLS),
         "fragment_room_of_one": (fragment_room_of_one, CALLS), "output_too_small": (output_too_small, ("filter", "bam_filter")),
         "more_fragments_than_reserved": (more_fragments_than_reserved, ("filter", "bam_filter")),
         "bad_quality": (bad_quality, ("bam_submit", "bam_filter")), "null_out_summary": (null_out_summary, CALLS)}
LEGS = [(case, call) for case, (_, calls) in CASES.items() for call in calls]


def run(rig, case, call):
    CASES[case][0](rig, call)
