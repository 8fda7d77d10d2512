#!/usr/bin/env python3
"""Times the BGZF input side of libtgsf_text on the GPU: k_bgzf_inflate on a chunk of BAM-like members, and
the device chain walk (k_bam_walk) at records of 1 kb and of 15 kb.  Each figure is the median of --reps calls, by a host
clock around a call that ends in a synchronise, after one warm-up call.  Prints one JSON line; --out writes it to a file too.

    python tools/text_bgzf_measure.py --members 4096 --reps 7 --out bgzf_measure.json
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bamparity as bp, bgzfmodel as gm  # noqa: E402
from tgsfilter_amd import text as tgtext  # noqa: E402


def records(rng, l_seq, n_bytes):
    recs, have = [], 0
    while have < n_bytes:
        recs.append(bp.rnd_record(rng, 24, l_seq, aux=40, qmax=60))
        have += len(recs[-1])
    return b"".join(recs)


def median_ms(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    res = {"members": a.members, "reps": a.reps}

    # 64 different members of 0xFF00 inflated bytes, as bgzip writes them (level 6), repeated to a.members
    pool = records(rng, 15000, 64 * 0xFF00)
    kinds = [gm.zmember(pool[i * 0xFF00:(i + 1) * 0xFF00]) for i in range(64)]
    gz = b"".join(kinds[b % 64] for b in range(a.members))
    out_bytes = a.members * 0xFF00
    tx = tgtext.TextIndexer(0, 1 << 20, 1 << 20, None)
    tx.reserve_bgzf(len(gz), a.members)
    blocks, stop, consumed, ob = tgtext.bgzf_walk(gz, a.members)
    assert (len(blocks), consumed, ob) == (a.members, len(gz), out_bytes)
    d_gz = torch.from_numpy(np.frombuffer(gz + bytes(-len(gz) % 16), np.uint8).copy()).to(dev)
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    t0 = time.perf_counter()
    tgtext.bgzf_walk(gz, a.members)
    res["host_walk_ms"] = (time.perf_counter() - t0) * 1e3

    def inflate():
        tx.inflate_device(len(gz), blocks, stop, d_out.data_ptr(), out_bytes, d_gz=d_gz.data_ptr())
        tx.fetch(want_index=False)

    med, lo, hi = median_ms(inflate, a.reps)
    want = np.frombuffer(pool[:0xFF00], np.uint8)
    assert np.array_equal(d_out[:0xFF00].cpu().numpy(), want) and np.array_equal(d_out[64 * 0xFF00:65 * 0xFF00].cpu().numpy(), want)
    res["inflate"] = {"gz_bytes": len(gz), "out_bytes": out_bytes, "ratio": out_bytes / len(gz), "ms_median": med, "ms_min": lo, "ms_max": hi,
                      "inflated_GB_per_s": out_bytes / med / 1e6, "compressed_GB_per_s": len(gz) / med / 1e6,
                      "note": "call time: table upload, k_bgzf_inflate, k_bgzf_finish, one synchronise"}
    t0 = time.perf_counter()
    for k in kinds:
        zlib.decompress(k[18:-8], -15)
    res["zlib_one_thread_GB_per_s"] = 64 * 0xFF00 / (time.perf_counter() - t0) / 1e9
    tx.close()

    # the device chain walk: 256 MiB of records of 1 kb and of 15 kb
    for l_seq in (1000, 15000):
        block = records(rng, l_seq, 1 << 20)
        reps = (256 << 20) // len(block)
        n_rec = len(bp.bm.walk(block, True, 1 << 30)[0]) - 1
        d_bam = torch.from_numpy(np.frombuffer(block, np.uint8).copy()).to(dev).repeat(reps)
        tx = tgtext.TextIndexer(0, 1 << 20, n_rec * reps + 8, None)
        tx.reserve_bam(16)
        n_bytes = len(block) * reps

        def walk():
            off, wstop, cons = tx.bam_walk_device(n_bytes, 0, True, d_bam.data_ptr())
            assert len(off) == n_rec * reps + 1 and cons == n_bytes

        med, lo, hi = median_ms(walk, a.reps)
        res["walk_%d" % l_seq] = {"records": n_rec * reps, "bytes": n_bytes, "ms_median": med, "ms_min": lo, "ms_max": hi, "ns_per_record": med * 1e6 / (n_rec * reps),
                                  "GB_per_s": n_bytes / med / 1e6, "note": "k_bam_walk, the copy of the table down, one synchronise"}
        tx.close()
        del d_bam
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
