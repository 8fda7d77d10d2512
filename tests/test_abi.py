"""The C-ABI library loads on a GPU-less box, exports every symbol include/tgsf.h declares, and
refuses to run without a device (there is no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tgsfilter_amd import abi, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "csrc")], check=True)
    return capi.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "tgsf.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(tgsf_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s)
    assert lib.tgsf_abi_version() == abi.ABI_VERSION


def test_struct_layout_matches_header(tmp_path):
    """sizeof() of the ctypes mirrors == what the C compiler sees."""
    src = r'''
    #include <stdio.h>
    #include "tgsf.h"
    int main(void){ printf("%zu %zu %zu %zu %zu\n", sizeof(tgsf_params), sizeof(tgsf_batch_in),
        sizeof(tgsf_batch_out), sizeof(tgsf_read_result), sizeof(tgsf_fragment)); return 0; }'''
    exe = str(tmp_path / "tgsf_sizes")             # (not a fixed name in /tmp: another user's file of that name cannot be written over)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    out = subprocess.run([exe], capture_output=True, check=True).stdout.split()
    got = [int(x) for x in out]
    assert got == [C.sizeof(abi.Params), C.sizeof(abi.BatchIn), C.sizeof(abi.BatchOut),
                   abi.READ_RESULT_DTYPE.itemsize, abi.FRAGMENT_DTYPE.itemsize]


def test_constants_match_header():
    """The constants of the tgsf_submit_device contract as the Python binding states them."""
    import re
    from tgsfilter_amd import abi
    hdr = open(os.path.join(ROOT, "include", "tgsf.h")).read()
    assert int(re.search(r"#define TGSF_MAX_ENQUEUED (\d+)", hdr).group(1)) == abi.MAX_ENQUEUED
    assert int(re.search(r"#define TGSF_NFRAGS_NOT_FINAL (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == abi.NFRAGS_NOT_FINAL
    assert int(re.search(r"#define TGSF_N_STAGES (\d+)", hdr).group(1)) == abi.N_STAGES


def test_no_device_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = abi.make_params("ont", adapters=[synth.ONT_RAPID], max_batch_bases=1000, max_batch_reads=4, max_read_len=500)
    with pytest.raises(capi.TgsfError) as ei:
        capi.Context(p, 0)
    assert ei.value.code == abi.E_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


def test_parameter_validation(lib):
    p = abi.make_params("ont", adapters=[b"A" * 8193], max_batch_bases=1000, max_batch_reads=4, max_read_len=500)      # beyond TGSF_MAX_ADAPTER_LEN
    with pytest.raises(capi.TgsfError) as ei:
        capi.Context(p, 0)
    assert ei.value.code == abi.E_UNSUPPORTED


def _create_params(**kw):
    """Parameters tgsf_create accepts (two adapters, the repeat gate on), with fields overwritten AFTER make_params' own clamps."""
    p = abi.make_params("ont", adapters=[synth.ONT_RAPID, synth.ONT_RAPID_RC], min_repeat=5, kmer=11,
                        max_batch_bases=1000, max_batch_reads=4, max_read_len=500)
    for k, v in kw.items():
        if k == "adapter0":                     # (pointer, length) of the first adapter
            p.adapters[0], p.adapter_len[0] = v
        else:
            setattr(p, k, v)
    return p


_NAN = float("nan")
# one row per check of tgsf_create, in its order: (fields, the status include/tgsf.h names for that class, the field's name in
# tgsf_params as the message holds it -- the offending field's and no other's: see test_create_refuses)
CREATE_REFUSALS = [
    (dict(struct_size=C.sizeof(abi.Params) - 8), abi.E_INVALID, "struct_size"),
    (dict(struct_size=0), abi.E_INVALID, "struct_size"),
    (dict(n_adapters=-1), abi.E_INVALID, "n_adapters"),
    (dict(n_adapters=33), abi.E_INVALID, "n_adapters"),
    (dict(min_len=-1), abi.E_INVALID, "min_len"),
    (dict(end_len=(1 << 28) + 1), abi.E_INVALID, "end_len (-E)"),
    (dict(end_len=2147483647), abi.E_INVALID, "end_len (-E)"),
    (dict(extra_len=(1 << 28) + 1), abi.E_INVALID, "extra_len (-T)"),
    (dict(extra_len=2147483647), abi.E_INVALID, "extra_len (-T)"),
    (dict(end_len=1500000000, filter=0), abi.E_INVALID, "end_len (-E)"),        # (whether or not adapters are searched for)
    (dict(extra_len=2147483647, n_adapters=0), abi.E_INVALID, "extra_len (-T)"),
    (dict(kmer=0), abi.E_UNSUPPORTED, "kmer (-k) 0"),
    (dict(kmer=33), abi.E_UNSUPPORTED, "kmer (-k) 33"),
    (dict(qtype=32), abi.E_INVALID, "qtype"),
    (dict(bc_len=-1), abi.E_INVALID, "bc_len"),
    (dict(bc_len=(1 << 20) + 1), abi.E_INVALID, "bc_len"),
    (dict(end_sim=0.0), abi.E_INVALID, "end_sim"),
    (dict(end_sim=_NAN), abi.E_INVALID, "end_sim"),
    (dict(mid_sim=0.0), abi.E_INVALID, "mid_sim"),
    (dict(mid_sim=_NAN), abi.E_INVALID, "mid_sim"),
    (dict(end_len=-1), abi.E_INVALID, "end_len"),
    (dict(extra_len=-1), abi.E_INVALID, "extra_len"),
    (dict(end_match_len=0), abi.E_INVALID, "end_match_len"),
    (dict(mid_match_len=0), abi.E_INVALID, "mid_match_len"),
    (dict(adapter0=(synth.ONT_RAPID, 0)), abi.E_UNSUPPORTED, "adapter 0"),
    (dict(adapter0=(None, 50)), abi.E_UNSUPPORTED, "adapter 0"),
    (dict(max_batch_bases=0), abi.E_INVALID, "max_batch_bases"),
    (dict(max_batch_reads=0), abi.E_INVALID, "max_batch_reads"),
    (dict(max_read_len=0), abi.E_INVALID, "max_read_len"),
    (dict(max_read_len=(1 << 28) + 1), abi.E_INVALID, "max_read_len"),
]
# the accepting neighbours that are cheap (small contexts; no context with max_read_len near 2^28 is created)
CREATE_ACCEPTED = [dict(min_len=0), dict(kmer=1), dict(kmer=32), dict(kmer=0, min_repeat=0), dict(kmer=33, min_repeat=0), dict(qtype=33), dict(qtype=64),
                   dict(bc_len=0), dict(end_len=0, extra_len=0), dict(end_match_len=1, mid_match_len=1),
                   dict(end_len=1 << 28, extra_len=1 << 28), dict(end_sim=1e-30), dict(end_sim=float("inf")),
                   dict(end_match_len=2147483647, mid_match_len=2147483647)]


@pytest.mark.parametrize("fields,code,names", CREATE_REFUSALS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_create_refuses(lib, fields, code, names):
    """Every check of tgsf_create in front of the device: the status of its class, no context, and a message from
    tgsf_last_error(NULL) that names the field."""
    p = _create_params(**fields)
    h = C.c_void_p(0xDEAD)
    rc = lib.tgsf_create(C.byref(p), 0, C.byref(h))
    msg = lib.tgsf_last_error(None).decode()
    assert rc == code, (rc, msg)
    assert h.value is None                         # *out_ctx is NULL after a refusal
    assert names in msg, msg
    # ... and no other field of tgsf_params: the message tells WHICH of two similarities, lengths or sizing hints it was
    others = [f for f, _ in abi.Params._fields_ if re.search(r"\b%s\b" % f, msg) and not re.search(r"\b%s\b" % f, names)]
    assert not others, (others, msg)


def test_create_refuses_null_arguments(lib):
    h = C.c_void_p()
    assert lib.tgsf_create(None, 0, C.byref(h)) == abi.E_INVALID and "null argument" in lib.tgsf_last_error(None).decode()
    assert lib.tgsf_create(C.byref(_create_params()), 0, None) == abi.E_INVALID and "null argument" in lib.tgsf_last_error(None).decode()


@pytest.mark.parametrize("fields", CREATE_ACCEPTED, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_create_accepts_the_neighbours(lib, fields):
    """... and the values next to the refused ones pass every check: on a box without a device that shows as
    TGSF_E_NO_DEVICE (the device is looked for after the checks), with one as a context."""
    p = _create_params(**fields)
    h = C.c_void_p()
    rc = lib.tgsf_create(C.byref(p), 0, C.byref(h))
    assert rc in (abi.OK, abi.E_NO_DEVICE), (rc, lib.tgsf_last_error(None).decode())
    if rc == abi.OK:
        lib.tgsf_destroy(h)
    else:
        assert "no CPU fallback" in lib.tgsf_last_error(None).decode()


def test_rccl_library_exports():
    """libtgsf_rccl.so (include/tgsf_rccl.h, the optional tally all-reduce) loads and exports what its header declares."""
    hdr = open(os.path.join(ROOT, "include", "tgsf_rccl.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(tgsf_rccl_\w+)\s*\(", hdr, flags=re.M))
    assert declared == {"tgsf_rccl_allreduce_counters", "tgsf_rccl_last_error", "tgsf_rccl_unique_id", "tgsf_rccl_comm_init",
                        "tgsf_rccl_comm_count", "tgsf_rccl_comm_destroy"}
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "csrc")], check=True)
    from tgsfilter_amd import rccl
    lib = rccl.load()
    for s in declared:
        assert hasattr(lib, s)


def test_backend_symbol_names_what_runs_the_kernels(lib):
    """include/tgsf.h: tgsf_backend() -- "hip:gfx950" for the product library, "emulation" for the tests' serial build."""
    assert lib.tgsf_backend() == b"hip:gfx950"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True)
    emul = capi.load(os.path.join(ROOT, "tests", "emul", "libtgsf_emul.so"))          # (an explicit path: the tests' way in)
    assert emul.tgsf_backend() == b"emulation"


def test_a_stray_TGSF_LIB_never_turns_a_gpu_run_into_a_cpu_run(tmp_path):
    """TGSF_LIB says where libtgsf.so is installed; pointing it at the emulation must not make the product
    -- the command line or the Python binding -- run on the CPU, with or without the debug switch."""
    import sys
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tgsfilter_amd", "host")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True)
    emul = os.path.join(ROOT, "tests", "emul", "libtgsf_emul.so")
    fq = tmp_path / "in.fq"
    reads = synth.make_reads(5, 6, "ont", mean_len=3000)
    fq.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, q) for n, s, q in reads))
    cli = os.path.join(ROOT, "tgsfilter_amd", "bin", "tgsfilter")
    for knobs in ({}, {"TGSF_DEBUG_KNOBS": "1"}):
        env = dict(os.environ, TGSF_LIB=emul, **knobs)
        if not knobs:
            env.pop("TGSF_DEBUG_KNOBS", None)
        out = tmp_path / "out.fq"
        p = subprocess.run([cli, "-i", str(fq), "-o", str(out), "-x", "ont", "-5", "0", "-3", "0"], capture_output=True, env=env, timeout=120)
        assert p.returncode != 0 and b"emulation" in p.stderr and b"no CPU fallback" in p.stderr, p.stderr[-500:]
        assert not out.exists() or out.stat().st_size == 0
        code = "from tgsfilter_amd import capi\ntry:\n    capi.load()\nexcept RuntimeError as e:\n    assert 'not the HIP build' in str(e), e\n    raise SystemExit(7)\n"
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, env=env, cwd=ROOT, timeout=120)
        assert p.returncode == 7, p.stderr[-500:]
