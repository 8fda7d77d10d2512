"""ctypes binding of libtgsf_text.so (include/tgsf_text.h): the record index of FASTQ / FASTA text, made on the GPU.

    tx = TextIndexer(0, max_bytes=len(text), max_records=100_000)
    idx, summary = tx.index(text)                       # five numpy arrays + the summary
    idx, summary, reads, frags = tx.submit(ctx, text)   # text in, filter results out (ctx: capi.Context)
    tx.reserve_output(max_frags, max_out_bytes)         # once; then
    clean, rec_end, out_summary, summary = tx.filter(ctx, text)   # text in, clean FASTQ / FASTA text out
    tx.reserve_bam(max_bam_bytes)                       # once; then, for inflated unaligned BAM from bam_header()'s offset on,
    idx, bam_summary = tx.bam_decode(bam)               # the records as FASTQ text in the object, and its index
    clean, rec_end, out_summary, bam_summary = tx.bam_filter(ctx, bam)   # BAM in, clean text out
    tx.reserve_bgzf(max_gz_bytes, max_blocks)           # once; then BGZF members as they are on disk:
    data, gz_summary = tx.inflate(gz)                   # inflated on the device (bgzip'ed FASTQ / FASTA lands in the text buffer)
    at, skip = tx.bgzf_bam_start(gz)                    # where a .bam file's records begin, as a BGZF virtual offset
    clean, rec_end, out_summary, s = tx.bgzf_bam_filter(ctx, gz[at:], skip)   # compressed BAM in, clean text out; s["next_gz"], s["next_skip"] resume
    tx.reserve_bgzf_out(max_in_bytes, max_gz_bytes)     # once; then text deflated on the device into BGZF members:
    gz, member_end, gz_summary = tx.deflate(text)       # gzip.decompress(gz) == text
    gz, gz_summary, out_summary, s = tx.bgzf_bam_filter_bgzf(ctx, gz[at:], skip)   # compressed BAM in, compressed clean text out
    bad_block, bad_crc = tx.verify(gz)                  # the opt-in CRC32 check of input members, on the device

There is no CPU fallback: the library found beside this file must be the HIP build.  (tests/emul builds a serial
emulation of the same kernels; only tests pass its path in.)
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import abi
from .capi import TgsfError

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libtgsf_text.so")
_LIBS = {}

ABI_VERSION = 2
END, IRREGULAR, CAPACITY = 0, 1, 2
STOP_NAMES = {END: "END", IRREGULAR: "IRREGULAR", CAPACITY: "CAPACITY"}
PAD = 64

SYMBOLS = [
    "tgsf_text_abi_version", "tgsf_text_backend", "tgsf_text_create", "tgsf_text_destroy", "tgsf_text_last_error", "tgsf_text_profile",
    "tgsf_text_buffers", "tgsf_text_index", "tgsf_text_upload", "tgsf_text_index_device", "tgsf_text_fetch", "tgsf_text_submit",
    "tgsf_text_out_reserve", "tgsf_text_format_device", "tgsf_text_format", "tgsf_text_filter", "tgsf_text_out_stage_ms",
    "tgsf_text_bam_header", "tgsf_text_bam_walk", "tgsf_text_bam_reserve", "tgsf_text_bam_decode", "tgsf_text_bam_decode_device",
    "tgsf_text_bam_submit", "tgsf_text_bam_filter",
    "tgsf_text_bgzf_walk", "tgsf_text_bgzf_reserve", "tgsf_text_bgzf_inflate", "tgsf_text_bgzf_inflate_device",
    "tgsf_text_bam_walk_device", "tgsf_text_bgzf_bam_decode", "tgsf_text_bgzf_bam_submit", "tgsf_text_bgzf_bam_filter",
    "tgsf_text_bgzf_bound", "tgsf_text_bgzf_out_reserve", "tgsf_text_bgzf_deflate", "tgsf_text_bgzf_deflate_device",
    "tgsf_text_bgzf_crc_device", "tgsf_text_bgzf_verify", "tgsf_text_filter_bgzf", "tgsf_text_bam_filter_bgzf", "tgsf_text_bgzf_bam_filter_bgzf",
    "tgsf_text_bgzf_out_level", "tgsf_text_bgzf_out_level_get",
]
BGZF_MEMBER = 0xFF00


class Summary(C.Structure):
    _fields_ = [("n_records", C.c_uint32), ("stop", C.c_uint32), ("consumed", C.c_uint64), ("bases", C.c_uint64),
                ("longest", C.c_uint32), ("device_ms", C.c_float)]

    def as_dict(self):
        return {"n_records": self.n_records, "stop": self.stop, "consumed": self.consumed, "bases": self.bases,
                "longest": self.longest, "device_ms": self.device_ms}


class IndexArrays(C.Structure):
    _fields_ = [("seq_off", C.c_void_p), ("qual_off", C.c_void_p), ("len", C.c_void_p), ("name_off", C.c_void_p), ("name_len", C.c_void_p)]


class DeviceBuffers(C.Structure):
    _fields_ = [("text", C.c_void_p), ("index", IndexArrays), ("summary", C.c_void_p), ("max_bytes", C.c_uint64),
                ("max_records", C.c_uint32), ("reserved", C.c_uint32)]


class OutSummary(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("bases", C.c_uint64), ("n_records", C.c_uint32), ("stop", C.c_uint32),
                ("device_ms", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"n_bytes": self.n_bytes, "bases": self.bases, "n_records": self.n_records, "stop": self.stop, "device_ms": self.device_ms}


class BamSummary(C.Structure):
    _fields_ = [("n_records", C.c_uint32), ("stop", C.c_uint32), ("consumed", C.c_uint64), ("text_bytes", C.c_uint64), ("bases", C.c_uint64),
                ("longest", C.c_uint32), ("bad_qual", C.c_uint32), ("device_ms", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"n_records": self.n_records, "stop": self.stop, "consumed": self.consumed, "text_bytes": self.text_bytes, "bases": self.bases,
                "longest": self.longest, "bad_qual": self.bad_qual, "device_ms": self.device_ms, "reserved": self.reserved}


class BgzfBlock(C.Structure):
    _fields_ = [("payload", C.c_uint64), ("clen", C.c_uint32), ("usize", C.c_uint32), ("out", C.c_uint64)]


BGZF_BLOCK_DTYPE = np.dtype([("payload", "<u8"), ("clen", "<u4"), ("usize", "<u4"), ("out", "<u8")])


class BgzfSummary(C.Structure):
    _fields_ = [("n_blocks", C.c_uint32), ("stop", C.c_uint32), ("consumed", C.c_uint64), ("out_bytes", C.c_uint64),
                ("bad_block", C.c_uint32), ("device_ms", C.c_float), ("reserved", C.c_uint64)]

    def as_dict(self):
        return {"n_blocks": self.n_blocks, "stop": self.stop, "consumed": self.consumed, "out_bytes": self.out_bytes,
                "bad_block": self.bad_block, "device_ms": self.device_ms, "reserved": self.reserved}


class BgzfBamSummary(C.Structure):
    _fields_ = [("gz", BgzfSummary), ("bam", BamSummary), ("next_gz", C.c_uint64), ("next_skip", C.c_uint32), ("reserved", C.c_uint32)]

    @property
    def n_records(self):
        return self.bam.n_records

    def as_dict(self):
        return {"gz": self.gz.as_dict(), "bam": self.bam.as_dict(), "next_gz": self.next_gz, "next_skip": self.next_skip, "reserved": self.reserved}


class GzOutSummary(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("n_bytes", C.c_uint64), ("n_members", C.c_uint32), ("stored", C.c_uint32), ("stop", C.c_uint32),
                ("device_ms", C.c_float), ("reserved", C.c_uint64)]

    def as_dict(self):
        return {"in_bytes": self.in_bytes, "n_bytes": self.n_bytes, "n_members": self.n_members, "stored": self.stored, "stop": self.stop,
                "device_ms": self.device_ms, "reserved": self.reserved}


NO_BAD_QUAL = NO_BAD_BLOCK = NO_BAD_CRC = 0xFFFFFFFF
assert C.sizeof(GzOutSummary) == 40
assert C.sizeof(BgzfBamSummary) == 104
assert C.sizeof(BgzfBlock) == 24 == BGZF_BLOCK_DTYPE.itemsize
assert C.sizeof(BgzfSummary) == 40
assert C.sizeof(Summary) == 32
assert C.sizeof(BamSummary) == 48
assert C.sizeof(OutSummary) == 32

Index = namedtuple("Index", "seq_off qual_off len name_off name_len")


def load(path: str | None = None):
    """`path` if given (the tests hand the emulation's in), else the in-tree HIP build, which must answer "hip..."."""
    explicit = path is not None
    path = path or DEFAULT_LIB
    if path not in _LIBS:
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(path)
        vp, u64, i = C.c_void_p, C.c_uint64, C.c_int
        L.tgsf_text_abi_version.restype = i
        L.tgsf_text_backend.restype = C.c_char_p
        L.tgsf_text_create.argtypes = [i, u64, C.c_uint32, C.POINTER(vp)]
        L.tgsf_text_destroy.argtypes = [vp]
        L.tgsf_text_destroy.restype = None
        L.tgsf_text_last_error.argtypes = [vp]
        L.tgsf_text_last_error.restype = C.c_char_p
        L.tgsf_text_profile.argtypes = [vp, i]
        L.tgsf_text_buffers.argtypes = [vp, C.POINTER(DeviceBuffers)]
        L.tgsf_text_index.argtypes = [vp, vp, u64, i, i, C.POINTER(IndexArrays), C.POINTER(Summary)]
        L.tgsf_text_upload.argtypes = [vp, vp, u64]
        L.tgsf_text_index_device.argtypes = [vp, vp, u64, i, i, C.POINTER(IndexArrays), vp, vp]
        L.tgsf_text_fetch.argtypes = [vp, C.POINTER(IndexArrays), C.POINTER(Summary)]
        L.tgsf_text_submit.argtypes = [vp, vp, vp, u64, i, i, C.POINTER(IndexArrays), C.POINTER(Summary), C.POINTER(abi.BatchOut)]
        u32 = C.c_uint32
        L.tgsf_text_out_reserve.argtypes = [vp, u32, u64]
        L.tgsf_text_format_device.argtypes = [vp, vp, C.POINTER(IndexArrays), u32, i, vp, vp, u32, i, vp, u64, vp, vp, vp]
        L.tgsf_text_format.argtypes = [vp, u32, i, vp, vp, u32, i, vp, u64, vp, C.POINTER(OutSummary)]
        L.tgsf_text_filter.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, vp, C.POINTER(OutSummary), C.POINTER(Summary),
                                       C.POINTER(IndexArrays), C.POINTER(abi.BatchOut)]
        L.tgsf_text_out_stage_ms.argtypes = [vp, C.POINTER(C.c_float * 3)]
        L.tgsf_text_bam_header.argtypes = [vp, u64, C.POINTER(u64)]
        L.tgsf_text_bam_walk.argtypes = [vp, u64, i, u32, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
        L.tgsf_text_bam_reserve.argtypes = [vp, u64]
        L.tgsf_text_bam_decode.argtypes = [vp, vp, u64, i, C.POINTER(IndexArrays), C.POINTER(BamSummary)]
        L.tgsf_text_bam_decode_device.argtypes = [vp, vp, u64, i, vp, u32, u32, C.POINTER(IndexArrays), vp, vp]
        L.tgsf_text_bam_submit.argtypes = [vp, vp, vp, u64, i, C.POINTER(IndexArrays), C.POINTER(BamSummary), C.POINTER(abi.BatchOut)]
        L.tgsf_text_bam_filter.argtypes = [vp, vp, vp, u64, i, i, vp, u64, vp, C.POINTER(OutSummary), C.POINTER(BamSummary),
                                           C.POINTER(IndexArrays), C.POINTER(abi.BatchOut)]
        L.tgsf_text_bgzf_walk.argtypes = [vp, u64, i, u32, u64, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
        L.tgsf_text_bgzf_reserve.argtypes = [vp, u64, u32]
        L.tgsf_text_bgzf_inflate.argtypes = [vp, vp, u64, i, vp, u64, C.POINTER(BgzfSummary)]
        L.tgsf_text_bgzf_inflate_device.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp]
        L.tgsf_text_bam_walk_device.argtypes = [vp, vp, u64, u64, i, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
        L.tgsf_text_bgzf_bam_decode.argtypes = [vp, vp, u64, u32, i, C.POINTER(IndexArrays), C.POINTER(BgzfBamSummary)]
        L.tgsf_text_bgzf_bam_submit.argtypes = [vp, vp, vp, u64, u32, i, C.POINTER(IndexArrays), C.POINTER(BgzfBamSummary), C.POINTER(abi.BatchOut)]
        L.tgsf_text_bgzf_bam_filter.argtypes = [vp, vp, vp, u64, u32, i, i, vp, u64, vp, C.POINTER(OutSummary), C.POINTER(BgzfBamSummary),
                                                C.POINTER(IndexArrays), C.POINTER(abi.BatchOut)]
        L.tgsf_text_bgzf_bound.argtypes = [u64, i]
        L.tgsf_text_bgzf_bound.restype = u64
        L.tgsf_text_bgzf_out_reserve.argtypes = [vp, u64, u64]
        L.tgsf_text_bgzf_out_level.argtypes = [vp, i]
        L.tgsf_text_bgzf_out_level_get.argtypes = [vp]
        L.tgsf_text_bgzf_deflate.argtypes = [vp, vp, u64, i, vp, u64, vp, C.POINTER(GzOutSummary)]
        L.tgsf_text_bgzf_deflate_device.argtypes = [vp, vp, u64, i, vp, u64, vp, vp, vp]
        L.tgsf_text_bgzf_crc_device.argtypes = [vp, vp, vp, u32, vp, vp, vp]
        L.tgsf_text_bgzf_verify.argtypes = [vp, vp, u64, i, C.POINTER(u32), C.POINTER(u32)]
        L.tgsf_text_filter_bgzf.argtypes = [vp, vp, vp, u64, i, i, i, vp, u64, C.POINTER(OutSummary), C.POINTER(Summary),
                                            C.POINTER(IndexArrays), C.POINTER(abi.BatchOut), i, C.POINTER(GzOutSummary)]
        L.tgsf_text_bam_filter_bgzf.argtypes = [vp, vp, vp, u64, i, i, vp, u64, C.POINTER(OutSummary), C.POINTER(BamSummary),
                                                C.POINTER(IndexArrays), C.POINTER(abi.BatchOut), i, C.POINTER(GzOutSummary)]
        L.tgsf_text_bgzf_bam_filter_bgzf.argtypes = [vp, vp, vp, u64, u32, i, i, vp, u64, C.POINTER(OutSummary), C.POINTER(BgzfBamSummary),
                                                     C.POINTER(IndexArrays), C.POINTER(abi.BatchOut), i, C.POINTER(GzOutSummary)]
        if L.tgsf_text_abi_version() != ABI_VERSION:
            raise RuntimeError("libtgsf_text ABI version mismatch")
        _LIBS[path] = L
    L = _LIBS[path]
    if not explicit and not L.tgsf_text_backend().startswith(b"hip"):
        raise RuntimeError(f"{path} is the {L.tgsf_text_backend().decode()!r} build of libtgsf_text, not the HIP build (there is no CPU fallback)")
    return L


def _as_u8(text):
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


def bam_header(bam, lib_path: str | None = None) -> int:
    """The offset of the first record's block_size in inflated BAM bytes that begin with the BAM header; TgsfError(-6) when
    the magic is wrong or the header is not complete yet."""
    L = load(lib_path)
    b = _as_u8(bam)
    at = C.c_uint64()
    rc = L.tgsf_text_bam_header(b.ctypes.data, b.size, C.byref(at))
    if rc != 0:
        raise TgsfError(rc, L.tgsf_text_last_error(None).decode())
    return at.value


def bam_walk(bam, max_records: int, final=True, lib_path: str | None = None):
    """The chain walk on the host: (rec_off of n + 1 entries as uint64, stop, consumed) for a chunk that begins at a record."""
    L = load(lib_path)
    b = _as_u8(bam)
    rec_off = np.zeros(int(max_records) + 1, np.uint64)
    n, stop, consumed = C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = L.tgsf_text_bam_walk(b.ctypes.data, b.size, int(final), int(max_records), rec_off.ctypes.data, C.byref(n), C.byref(stop), C.byref(consumed))
    if rc != 0:
        raise TgsfError(rc, L.tgsf_text_last_error(None).decode())
    return rec_off[:n.value + 1].copy(), stop.value, consumed.value


def bgzf_walk(gz, max_blocks: int, max_out_bytes: int = (1 << 64) - 1, final=True, lib_path: str | None = None):
    """The member walk on the host for a chunk that begins at a BGZF member: (blocks as BGZF_BLOCK_DTYPE, stop, consumed,
    out_bytes)."""
    L = load(lib_path)
    b = _as_u8(gz)
    blocks = np.zeros(max(int(max_blocks), 1), BGZF_BLOCK_DTYPE)
    n, stop, consumed, out_bytes = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = L.tgsf_text_bgzf_walk(b.ctypes.data, b.size, int(final), int(max_blocks), int(max_out_bytes), blocks.ctypes.data, C.byref(n), C.byref(stop),
                               C.byref(consumed), C.byref(out_bytes))
    if rc != 0:
        raise TgsfError(rc, L.tgsf_text_last_error(None).decode())
    return blocks[:n.value].copy(), stop.value, consumed.value, out_bytes.value


def bgzf_bound(n_bytes: int, eof=True, lib_path: str | None = None) -> int:
    """Room enough for the BGZF members of any n_bytes of text (with eof: and the EOF member)."""
    return load(lib_path).tgsf_text_bgzf_bound(int(n_bytes), int(eof))


class TextIndexer:
    """One tgsf_text object: device buffers for chunks of up to max_bytes bytes and max_records records, and a stream."""

    def __init__(self, device: int, max_bytes: int, max_records: int, lib_path: str | None = None):
        self.lib, self.lib_path = load(lib_path), lib_path
        self.max_bytes, self.max_records = int(max_bytes), int(max_records)
        h = C.c_void_p()
        rc = self.lib.tgsf_text_create(device, self.max_bytes, self.max_records, C.byref(h))
        if rc != 0:
            raise TgsfError(rc, self.lib.tgsf_text_last_error(None).decode())
        self.h = h

    def _chk(self, rc, summary=None, in_summary=None):
        """Raise what a call refused; the summaries it filled go along as the attributes `summary` and `in_summary`."""
        if rc != 0:
            e = TgsfError(rc, self.lib.tgsf_text_last_error(self.h).decode())
            if summary is not None:
                e.summary = summary.as_dict()
            if in_summary is not None:
                e.in_summary = in_summary.as_dict()
            raise e

    def close(self):
        if getattr(self, "h", None):
            self.lib.tgsf_text_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self, enable=True):
        self._chk(self.lib.tgsf_text_profile(self.h, int(enable)))

    def buffers(self) -> DeviceBuffers:
        """Device addresses of the object's text buffer, index arrays and summary."""
        b = DeviceBuffers()
        self._chk(self.lib.tgsf_text_buffers(self.h, C.byref(b)))
        return b

    def _host_index(self):
        m = self.max_records
        arrs = Index(np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint64), np.zeros(m, np.uint32))
        return arrs, IndexArrays(*[a.ctypes.data for a in arrs])

    @staticmethod
    def _clip(arrs, n):
        return Index(*[a[:n].copy() for a in arrs])

    def index(self, text, fasta=False, final=True):
        """Index a chunk held in host memory: (Index of n_records entries each, summary dict)."""
        t = _as_u8(text)
        arrs, ia = self._host_index()
        s = Summary()
        self._chk(self.lib.tgsf_text_index(self.h, t.ctypes.data, t.size, int(fasta), int(final), C.byref(ia), C.byref(s)))
        return self._clip(arrs, s.n_records), s.as_dict()

    def upload(self, text):
        """The text into the object's device buffer (zero-padded), nothing else."""
        t = _as_u8(text)
        self._chk(self.lib.tgsf_text_upload(self.h, t.ctypes.data, t.size))
        return t.size

    def index_device(self, n_bytes, fasta=False, final=True, d_text=None, d_index: IndexArrays | None = None, d_summary=None, stream=None):
        """Enqueue the index of text already in HBM (d_text None: the object's buffer, see upload) without waiting.
        d_index None: the index stays in the object's arrays (buffers().index); fetch() brings it to the host."""
        self._chk(self.lib.tgsf_text_index_device(self.h, d_text, int(n_bytes), int(fasta), int(final),
                                                  C.byref(d_index) if d_index is not None else None, d_summary, stream))

    def fetch(self, want_index=True):
        """Wait for the object's stream; the object's own index and summary as index() returns them."""
        s = Summary()
        if not want_index:
            self._chk(self.lib.tgsf_text_fetch(self.h, None, C.byref(s)))
            return None, s.as_dict()
        arrs, ia = self._host_index()
        self._chk(self.lib.tgsf_text_fetch(self.h, C.byref(ia), C.byref(s)))
        return self._clip(arrs, s.n_records), s.as_dict()

    def _results(self, frag_capacity, expected_frags):
        """Host tables for the filter's results and the tgsf_batch_out over them; frag_capacity None: room for the fragments
        expected of the chunk's size, one more per record, and 16."""
        if frag_capacity is None:
            frag_capacity = expected_frags + self.max_records + 16
        reads = np.zeros(self.max_records, dtype=abi.READ_RESULT_DTYPE)
        frags = np.zeros(frag_capacity, dtype=abi.FRAGMENT_DTYPE)
        return reads, frags, abi.BatchOut(reads.ctypes.data, frags.ctypes.data, frag_capacity, 0)

    def _submit(self, call, s, frag_capacity, expected_frags, want_index, summary_on_error):
        """submit() and bam_submit(): call(out_index, out_summary, batch_out) is the library's; s its empty summary."""
        arrs, ia = self._host_index() if want_index else (None, None)
        reads, frags, bo = self._results(frag_capacity, expected_frags)
        self._chk(call(C.byref(ia) if want_index else None, C.byref(s), C.byref(bo)), s if summary_on_error else None)
        n = s.n_records
        return (self._clip(arrs, n) if want_index else None), s.as_dict(), reads[:n].copy(), frags[:bo.n_frags].copy()

    def submit(self, ctx, text, fasta=False, final=True, frag_capacity=None, want_index=True):
        """Text in, filter results out: (Index or None, summary dict, reads, frags) for the regular prefix of `text`,
        through `ctx` (a capi.Context of the same device and the same build; no_qual for FASTA)."""
        t = _as_u8(text)
        return self._submit(lambda *a: self.lib.tgsf_text_submit(self.h, ctx.h, t.ctypes.data, t.size, int(fasta), int(final), *a),
                            Summary(), frag_capacity, t.size // 100, want_index, False)

    # ---- the output side: the kept records as clean FASTQ / FASTA text ------------------------------------------------
    def reserve_output(self, max_frags, max_out_bytes):
        """Once, before the first format: scratch for max_frags fragments a call and an output buffer of max_out_bytes."""
        self._chk(self.lib.tgsf_text_out_reserve(self.h, int(max_frags), int(max_out_bytes)))
        self.max_frags, self.max_out_bytes = int(max_frags), int(max_out_bytes)

    def _out(self, out, out_capacity):
        """The host buffer a format writes into: the caller's (a writable uint8 array) or a new one of out_capacity bytes."""
        if out is None:
            out = np.empty(getattr(self, "max_out_bytes", 0) if out_capacity is None else int(out_capacity), np.uint8)
        return out, (out.size if out_capacity is None else int(out_capacity))

    def format(self, n_records, reads, frags, fastq_out=True, fasta=False, out=None, out_capacity=None):
        """Format host tables (abi.READ_RESULT_DTYPE, abi.FRAGMENT_DTYPE) against the text and the index that are in the
        object: (the text as bytes, rec_end as uint64 array, summary dict).  TGSF_TEXT_CAPACITY raises TgsfError(-4); its
        `summary` attribute says what is needed."""
        reads = np.ascontiguousarray(reads, dtype=abi.READ_RESULT_DTYPE)
        frags = np.ascontiguousarray(frags, dtype=abi.FRAGMENT_DTYPE)
        out, cap = self._out(out, out_capacity)
        rec_end = np.zeros(max(len(frags), 1), np.uint64)
        s = OutSummary()
        rc = self.lib.tgsf_text_format(self.h, int(n_records), int(fasta), reads.ctypes.data, frags.ctypes.data, len(frags), int(fastq_out),
                                       out.ctypes.data, cap, rec_end.ctypes.data, C.byref(s))
        self._chk(rc, s)
        return out[:s.n_bytes].tobytes(), rec_end[:s.n_records].copy(), s.as_dict()

    def format_device(self, n_records, d_reads, d_frags, n_frags, fastq_out=True, fasta=False, d_text=None, d_index: IndexArrays | None = None,
                      d_out=None, out_capacity=0, d_rec_end=None, d_summary=None, stream=None):
        """Enqueue the format of tables already in HBM (device addresses) without waiting; None: the object's own text,
        index, output buffer and summary."""
        self._chk(self.lib.tgsf_text_format_device(self.h, d_text, C.byref(d_index) if d_index is not None else None, int(n_records),
                                                   int(fasta), d_reads, d_frags, int(n_frags), int(fastq_out), d_out, int(out_capacity),
                                                   d_rec_end, d_summary, stream))

    def stage_ms(self):
        """Milliseconds of the last format's stages (sizes, layout, copy) with profile() on; waits for it."""
        ms = (C.c_float * 3)()
        self._chk(self.lib.tgsf_text_out_stage_ms(self.h, C.byref(ms)))
        return {"sizes": ms[0], "layout": ms[1], "copy": ms[2]}

    def _filter(self, call, si, out, out_capacity, frag_capacity, expected_frags, want_results, in_summary_on_error):
        """filter() and bam_filter(): call(out, out_capacity, rec_end, out_summary, in_summary, out_index, batch_out) is the
        library's; si its empty input summary."""
        out, cap = self._out(out, out_capacity)
        rec_end = np.zeros(max(getattr(self, "max_frags", 0), 1), np.uint64)
        so = OutSummary()
        reads, frags, bo = self._results(frag_capacity, expected_frags) if want_results else (None, None, None)
        rc = call(out.ctypes.data, cap, rec_end.ctypes.data, C.byref(so), C.byref(si), None, C.byref(bo) if want_results else None)
        self._chk(rc, so, si if in_summary_on_error else None)
        res = (out[:so.n_bytes].tobytes(), rec_end[:so.n_records].copy(), so.as_dict(), si.as_dict())
        if want_results:
            res += (reads[:si.n_records].copy(), frags[:bo.n_frags].copy())
        return res

    def filter(self, ctx, text, fasta=False, final=True, fastq_out=None, out=None, out_capacity=None, frag_capacity=None, want_results=False):
        """Text in, clean text out: (the text as bytes, rec_end, out summary dict, in summary dict) for the regular prefix
        of `text`; with want_results also the per-read records and the fragments, as submit() returns them."""
        t = _as_u8(text)
        if fastq_out is None:
            fastq_out = not fasta
        return self._filter(lambda *a: self.lib.tgsf_text_filter(self.h, ctx.h, t.ctypes.data, t.size, int(fasta), int(final), int(fastq_out), *a),
                            Summary(), out, out_capacity, frag_capacity, t.size // 100, want_results, False)

    # ---- the BAM input side: inflated unaligned BAM records in -----------------------------------------------------------
    def reserve_bam(self, max_bam_bytes):
        """Once, before the first decode: the device buffer for chunks of up to max_bam_bytes and the per-record scratch."""
        self._chk(self.lib.tgsf_text_bam_reserve(self.h, int(max_bam_bytes)))
        self.max_bam_bytes = int(max_bam_bytes)

    def bam_decode(self, bam, final=True, want_index=True):
        """Decode a chunk of inflated BAM records held in host memory into the object's text buffer and index arrays:
        (Index or None, summary dict).  The text itself stays on the device (buffers().text, summary["text_bytes"] bytes)."""
        b = _as_u8(bam)
        arrs, ia = self._host_index() if want_index else (None, None)
        s = BamSummary()
        self._chk(self.lib.tgsf_text_bam_decode(self.h, b.ctypes.data, b.size, int(final), C.byref(ia) if want_index else None, C.byref(s)))
        return (self._clip(arrs, s.n_records) if want_index else None), s.as_dict()

    def bam_decode_device(self, n_bytes, rec_off, walk_stop, final=True, d_bam=None, d_index: IndexArrays | None = None, d_summary=None, stream=None):
        """Enqueue the decode of BAM bytes already in HBM (d_bam None: the object's buffer) without waiting; rec_off (uint64,
        n_walked + 1 entries) and walk_stop are bam_walk()'s.  fetch() does not know this summary: read d_summary, or
        buffers() after a synchronise."""
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        self._chk(self.lib.tgsf_text_bam_decode_device(self.h, d_bam, int(n_bytes), int(final), rec_off.ctypes.data, rec_off.size - 1, int(walk_stop),
                                                       C.byref(d_index) if d_index is not None else None, d_summary, stream))

    def bam_submit(self, ctx, bam, final=True, frag_capacity=None, want_index=True):
        """BAM in, filter results out: (Index or None, summary dict, reads, frags) for the indexed prefix of `bam`.  A quality
        byte of 233 raises TgsfError(-6); its `summary` attribute holds bad_qual."""
        b = _as_u8(bam)
        return self._submit(lambda *a: self.lib.tgsf_text_bam_submit(self.h, ctx.h, b.ctypes.data, b.size, int(final), *a),
                            BamSummary(), frag_capacity, b.size // 50, want_index, True)

    def bam_filter(self, ctx, bam, final=True, fastq_out=True, out=None, out_capacity=None, frag_capacity=None, want_results=False):
        """BAM in, clean text out: (the text as bytes, rec_end, out summary dict, BAM summary dict) for the indexed prefix of
        `bam`; with want_results also the per-read records and the fragments, as bam_submit() returns them."""
        b = _as_u8(bam)
        return self._filter(lambda *a: self.lib.tgsf_text_bam_filter(self.h, ctx.h, b.ctypes.data, b.size, int(final), int(fastq_out), *a),
                            BamSummary(), out, out_capacity, frag_capacity, b.size // 50, want_results, True)

    # ---- the BGZF input side: compressed members in ------------------------------------------------------------------------
    def reserve_bgzf(self, max_gz_bytes, max_blocks):
        """Once, before the first inflate: the device buffer for chunks of up to max_gz_bytes compressed bytes and the table
        of up to max_blocks members."""
        self._chk(self.lib.tgsf_text_bgzf_reserve(self.h, int(max_gz_bytes), int(max_blocks)))
        self.max_gz_bytes, self.max_blocks = int(max_gz_bytes), int(max_blocks)

    def inflate(self, gz, final=True, out_capacity=None, want_bytes=True):
        """Inflate a chunk of BGZF members held in host memory into the object's text buffer: (the inflated bytes or None,
        summary dict).  A bad member raises TgsfError(-6); its `summary` attribute holds bad_block."""
        b = _as_u8(gz)
        cap = self.max_bytes if out_capacity is None else int(out_capacity)
        out = np.empty(max(cap, 1), np.uint8) if want_bytes else None
        s = BgzfSummary()
        self._chk(self.lib.tgsf_text_bgzf_inflate(self.h, b.ctypes.data, b.size, int(final), out.ctypes.data if want_bytes else None, cap, C.byref(s)), s)
        return (out[:s.out_bytes].tobytes() if want_bytes else None), s.as_dict()

    def inflate_device(self, n_bytes, blocks, walk_stop, d_out, out_capacity, d_gz=None, d_summary=None, stream=None):
        """Enqueue the inflate of compressed bytes already in HBM (d_gz None: the object's buffer) into d_out without waiting;
        blocks (BGZF_BLOCK_DTYPE) and walk_stop are bgzf_walk()'s."""
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        self._chk(self.lib.tgsf_text_bgzf_inflate_device(self.h, d_gz, int(n_bytes), blocks.ctypes.data if blocks.size else None, blocks.size, int(walk_stop),
                                                         d_out, int(out_capacity), d_summary, stream))

    def bam_walk_device(self, n_bytes, start=0, final=True, d_bam=None):
        """The chain walk on BAM bytes in HBM (d_bam None: the object's BAM buffer) from byte `start` on: (rec_off of n + 1
        entries, stop, consumed), offsets counted from d_bam, as bam_walk() gives them on the host."""
        rec_off = np.zeros(self.max_records + 1, np.uint64)
        n, stop, consumed = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._chk(self.lib.tgsf_text_bam_walk_device(self.h, d_bam, int(start), int(n_bytes), int(final), rec_off.ctypes.data, C.byref(n), C.byref(stop),
                                                     C.byref(consumed)))
        return rec_off[:n.value + 1].copy(), stop.value, consumed.value

    # ---- compressed BAM in: chunks are (gz bytes that begin at a member, skip) ---------------------------------------------
    def bgzf_bam_start(self, gz):
        """Where the records of a .bam file begin, as a BGZF virtual offset (compressed offset of the member, skip): inflates
        members from the front until the BAM header is complete."""
        b = _as_u8(gz)
        blocks, stop, consumed, out_bytes = bgzf_walk(b, self.max_blocks, self.max_bytes, False, self.lib_path)
        ends = blocks["payload"] + blocks["clen"] + 8
        k = 1
        while True:
            k = min(k, len(blocks))
            data, _ = self.inflate(b[:int(ends[k - 1])] if k else b[:0], final=False)
            try:
                at = bam_header(data, self.lib_path)
                break
            except TgsfError:
                if k >= len(blocks):
                    raise
                k *= 2
        if at == len(data):
            return (int(ends[k - 1]) if k else 0), 0
        m = int(np.searchsorted(blocks["out"][:k], at, side="right")) - 1
        return (int(ends[m - 1]) if m else 0), at - int(blocks["out"][m])

    def bgzf_bam_decode(self, gz, skip=0, final=True, want_index=True):
        """Decode a chunk of a .bam file as it is on disk, from a member's first byte on, the first `skip` inflated bytes left
        out: (Index or None, summary dict with "gz", "bam", "next_gz", "next_skip")."""
        b = _as_u8(gz)
        arrs, ia = self._host_index() if want_index else (None, None)
        s = BgzfBamSummary()
        self._chk(self.lib.tgsf_text_bgzf_bam_decode(self.h, b.ctypes.data, b.size, int(skip), int(final), C.byref(ia) if want_index else None, C.byref(s)), s)
        return (self._clip(arrs, s.n_records) if want_index else None), s.as_dict()

    def bgzf_bam_submit(self, ctx, gz, skip=0, final=True, frag_capacity=None, want_index=True):
        """Compressed BAM in, filter results out: as bam_submit()."""
        b = _as_u8(gz)
        return self._submit(lambda *a: self.lib.tgsf_text_bgzf_bam_submit(self.h, ctx.h, b.ctypes.data, b.size, int(skip), int(final), *a),
                            BgzfBamSummary(), frag_capacity, b.size // 12, want_index, True)

    def bgzf_bam_filter(self, ctx, gz, skip=0, final=True, fastq_out=True, out=None, out_capacity=None, frag_capacity=None, want_results=False):
        """Compressed BAM in, clean text out: as bam_filter()."""
        b = _as_u8(gz)
        return self._filter(lambda *a: self.lib.tgsf_text_bgzf_bam_filter(self.h, ctx.h, b.ctypes.data, b.size, int(skip), int(final), int(fastq_out), *a),
                            BgzfBamSummary(), out, out_capacity, frag_capacity, b.size // 12, want_results, True)

    # ---- the BGZF output side: text in, compressed members out; the CRC32 of input members ----------------------------------
    def reserve_bgzf_out(self, max_in_bytes, max_gz_bytes=None):
        """Once, before the first deflate: room for texts of up to max_in_bytes and max_gz_bytes compressed bytes (None: the
        bound for max_in_bytes, which fits every text)."""
        if max_gz_bytes is None:
            max_gz_bytes = bgzf_bound(max_in_bytes, True, self.lib_path)
        self._chk(self.lib.tgsf_text_bgzf_out_reserve(self.h, int(max_in_bytes), int(max_gz_bytes)))
        self.max_gz_in, self.max_gz_out = int(max_in_bytes), int(max_gz_bytes)

    def set_bgzf_level(self, level):
        """Before reserve_bgzf_out: 0, the Huffman-only coder (the default), or 1, the match search.  Holds for every deflate of
        the object, the composed *_filter_bgzf calls included."""
        self._chk(self.lib.tgsf_text_bgzf_out_level(self.h, int(level)))

    @property
    def bgzf_level(self):
        return int(self.lib.tgsf_text_bgzf_out_level_get(self.h))

    def _gz_out(self, out, out_capacity):
        if out is None:
            out = np.empty(max(getattr(self, "max_gz_out", 0) if out_capacity is None else int(out_capacity), 1), np.uint8)
        return out, (out.size if out_capacity is None else int(out_capacity))

    def deflate(self, text, eof=True, out=None, out_capacity=None):
        """Text held in host memory as BGZF members: (the compressed bytes, member_end as uint64 array, summary dict).
        TGSF_TEXT_CAPACITY raises TgsfError(-4); its `summary` attribute says what is needed."""
        t = _as_u8(text)
        out, cap = self._gz_out(out, out_capacity)
        member_end = np.zeros(t.size // BGZF_MEMBER + 2, np.uint64)
        s = GzOutSummary()
        self._chk(self.lib.tgsf_text_bgzf_deflate(self.h, t.ctypes.data, t.size, int(eof), out.ctypes.data, cap, member_end.ctypes.data, C.byref(s)), s)
        return out[:s.n_bytes].tobytes(), member_end[:s.n_members].copy(), s.as_dict()

    def deflate_device(self, n_bytes, eof=True, d_in=None, d_out=None, out_capacity=0, d_member_end=None, d_summary=None, stream=None):
        """Enqueue the deflate of text already in HBM without waiting; None: the object's own output buffer as the last
        format left it, the object's own compressed buffer and summary."""
        self._chk(self.lib.tgsf_text_bgzf_deflate_device(self.h, d_in, int(n_bytes), int(eof), d_out, int(out_capacity), d_member_end, d_summary, stream))

    def crc_device(self, blocks, d_bad_crc, d_gz=None, d_inflated=None, stream=None):
        """Enqueue the CRC32 check of inflated members (blocks: bgzf_walk()'s table; None: the object's compressed bytes, its
        text buffer) without waiting; the lowest mismatching member goes to the device word d_bad_crc."""
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        self._chk(self.lib.tgsf_text_bgzf_crc_device(self.h, d_gz, blocks.ctypes.data if blocks.size else None, blocks.size, d_inflated, d_bad_crc, stream))

    def verify(self, gz, final=True):
        """Inflate a chunk of BGZF members into the object's text buffer and check every member's CRC32 on the device:
        (NO_BAD_BLOCK, NO_BAD_CRC) when all is well, else TgsfError(-6) with the attributes bad_block and bad_crc."""
        b = _as_u8(gz)
        bb, bc = C.c_uint32(), C.c_uint32()
        rc = self.lib.tgsf_text_bgzf_verify(self.h, b.ctypes.data, b.size, int(final), C.byref(bb), C.byref(bc))
        if rc != 0:
            e = TgsfError(rc, self.lib.tgsf_text_last_error(self.h).decode())
            e.bad_block, e.bad_crc = bb.value, bc.value
            raise e
        return bb.value, bc.value

    def _filter_bgzf(self, call, si, eof, out, out_capacity, frag_capacity, expected_frags, want_results, in_summary_on_error, want_gz_summary):
        """The three *_filter_bgzf calls: call(out, out_capacity, out_summary, in_summary, out_index, batch_out, eof, gz_summary)
        is the library's; si its empty input summary."""
        out, cap = self._gz_out(out, out_capacity)
        so, sg = OutSummary(), GzOutSummary()
        reads, frags, bo = self._results(frag_capacity, expected_frags) if want_results else (None, None, None)
        rc = call(out.ctypes.data, cap, C.byref(so), C.byref(si), None, C.byref(bo) if want_results else None, int(eof),
                  C.byref(sg) if want_gz_summary else None)
        if rc != 0:
            e = TgsfError(rc, self.lib.tgsf_text_last_error(self.h).decode())
            e.summary, e.gz_summary = so.as_dict(), sg.as_dict()
            if in_summary_on_error:
                e.in_summary = si.as_dict()
            raise e
        n = sg.n_bytes if want_gz_summary else cap
        res = (out[:n].tobytes(), sg.as_dict() if want_gz_summary else None, so.as_dict(), si.as_dict())
        if want_results:
            res += (reads[:si.n_records].copy(), frags[:bo.n_frags].copy())
        return res

    def filter_bgzf(self, ctx, text, fasta=False, final=True, fastq_out=None, eof=True, out=None, out_capacity=None, frag_capacity=None,
                    want_results=False, want_gz_summary=True):
        """Text in, compressed clean text out: (the BGZF bytes, gz summary dict, out summary dict of the text, in summary dict).
        Without want_gz_summary the library is handed a null gz_summary and the whole buffer comes back."""
        t = _as_u8(text)
        if fastq_out is None:
            fastq_out = not fasta
        return self._filter_bgzf(lambda *a: self.lib.tgsf_text_filter_bgzf(self.h, ctx.h, t.ctypes.data, t.size, int(fasta), int(final), int(fastq_out), *a),
                                 Summary(), eof, out, out_capacity, frag_capacity, t.size // 100, want_results, False, want_gz_summary)

    def bam_filter_bgzf(self, ctx, bam, final=True, fastq_out=True, eof=True, out=None, out_capacity=None, frag_capacity=None, want_results=False,
                        want_gz_summary=True):
        """BAM in, compressed clean text out: as filter_bgzf()."""
        b = _as_u8(bam)
        return self._filter_bgzf(lambda *a: self.lib.tgsf_text_bam_filter_bgzf(self.h, ctx.h, b.ctypes.data, b.size, int(final), int(fastq_out), *a),
                                 BamSummary(), eof, out, out_capacity, frag_capacity, b.size // 50, want_results, True, want_gz_summary)

    def bgzf_bam_filter_bgzf(self, ctx, gz, skip=0, final=True, fastq_out=True, eof=True, out=None, out_capacity=None, frag_capacity=None,
                             want_results=False, want_gz_summary=True):
        """Compressed BAM in, compressed clean text out: as filter_bgzf()."""
        b = _as_u8(gz)
        return self._filter_bgzf(lambda *a: self.lib.tgsf_text_bgzf_bam_filter_bgzf(self.h, ctx.h, b.ctypes.data, b.size, int(skip), int(final), int(fastq_out), *a),
                                 BgzfBamSummary(), eof, out, out_capacity, frag_capacity, b.size // 12, want_results, True, want_gz_summary)
