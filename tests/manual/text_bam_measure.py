"""Measurement of the BAM input side of libtgsf_text on an MI355X (k_bam_*): a synthetic chunk of about
1 GiB of inflated unaligned BAM with HiFi-like records of about 15 kb (a block of 200 records repeated), decoded with
tgsf_text_profile on; device_ms (the eight launches of one decode, by HIP events) is the median of --reps calls after a
warm-up.  The bytes moved are the BAM bytes read plus the text written, about 3.5 bytes per base.  The yardstick, in the same
process: k_textout_copy formatting the decoded text as identity (one whole-read PASS fragment per read, the tables made on
the device), which moves 4 bytes per base with the same piece scheme.  The host's walk (tgsf_text_bam_walk) is timed on the
same bytes.  Prints one JSON line.

    python tests/manual/text_bam_measure.py [--gib 1] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import bammodel as bm, bamparity as bp       # noqa: E402
from tgsfilter_amd import abi, text as tgtext            # noqa: E402

PEAK_HBM = 8.0e12          # bytes/s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    rng = np.random.default_rng(110)
    recs = [bp.rnd_record(rng, 24, int(min(max(rng.normal(15000, 2500), 3000), 30000)), aux=20 + i % 13, qmax=94) for i in range(200)]
    block = np.frombuffer(b"".join(recs), np.uint8)
    bmod = bm.rule(block.tobytes(), True, len(recs), 1 << 40)
    reps = int(a.gib * (1 << 30)) // block.size + 1
    bam = np.tile(block, reps)
    n_bytes, nrec, text_bytes, bases = bam.size, reps * len(recs), reps * bmod["text_bytes"], reps * bmod["bases"]
    out = {"bam_bytes": n_bytes, "n_records": nrec, "text_bytes": text_bytes, "bases": bases, "mean_len": round(bases / nrec, 1)}

    # the walk on the host
    walks = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        off, stop, consumed = tgtext.bam_walk(bam, nrec)
        walks.append(time.perf_counter() - t0)
    assert off.size == nrec + 1 and stop == tgtext.END and consumed == n_bytes
    out["walk_ms"] = {"runs": [round(x * 1e3, 4) for x in walks], "median": round(float(np.median(walks)) * 1e3, 4),
                      "ns_per_record": round(float(np.median(walks)) * 1e9 / nrec, 2)}

    tx = tgtext.TextIndexer(0, text_bytes, nrec)
    tx.reserve_bam(n_bytes)
    tx.reserve_output(nrec, 16)
    tx.profile(True)

    def one():
        _, s = tx.bam_decode(bam, want_index=False)
        assert (s["n_records"], s["stop"], s["text_bytes"], s["bases"], s["bad_qual"]) == (nrec, tgtext.END, text_bytes, bases, tgtext.NO_BAD_QUAL), s
        return s["device_ms"]

    one()                                                                   # warm-up
    b = tx.buffers()
    mem = bp.TorchMem(own_stream=False)
    want = torch.from_numpy(np.frombuffer(bmod["text"], np.uint8).copy()).to(dev)
    got = mem._view(b.text, text_bytes)
    assert torch.equal(got[:want.numel()], want) and torch.equal(got[-want.numel():], want)
    ms = [one() for _ in range(a.reps)]
    med = float(np.median(ms))
    moved = n_bytes + text_bytes
    out["decode_ms"] = {"runs": [round(x, 4) for x in ms], "median": round(med, 4)}
    out["decode_bytes_moved"] = moved
    out["decode_bytes_per_base"] = round(moved / bases, 3)
    out["decode_gb_per_s"] = round(moved / (med * 1e-3) / 1e9, 1)
    out["decode_fraction_of_peak"] = round(moved / (med * 1e-3) / PEAK_HBM, 3)
    out["decode_floor_ms"] = round(moved / PEAK_HBM * 1e3, 4)

    # the yardstick: k_textout_copy on the decoded text as identity
    ar = torch.arange(nrec, dtype=torch.int32, device=dev)
    d_reads = torch.zeros((nrec, 8), dtype=torch.int32, device=dev)         # tgsf_read_result: n_frags, frag_begin are words 3, 4
    d_reads[:, 3], d_reads[:, 4] = 1, ar
    d_frags = torch.zeros((nrec, 6), dtype=torch.int32, device=dev)         # tgsf_fragment: read, start, len, flags are words 2..5
    d_frags[:, 2], d_frags[:, 4], d_frags[:, 5] = ar, torch.from_numpy(np.tile(bmod["index"]["len"].astype(np.int32), reps)).to(dev), abi.FF_PASS
    d_out = torch.empty(text_bytes, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def fmt():
        tx.format_device(nrec, d_reads.data_ptr(), d_frags.data_ptr(), nrec, d_out=d_out.data_ptr(), out_capacity=text_bytes, d_summary=d_sum.data_ptr())
        return tx.stage_ms()                                                # (waits for the format)

    fmt()
    sm = tgtext.OutSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
    assert (sm.n_bytes, sm.n_records, sm.stop) == (text_bytes, nrec, tgtext.END), sm.as_dict()
    assert torch.equal(d_out, got)
    runs = [fmt() for _ in range(a.reps)]
    cp = float(np.median([r["copy"] for r in runs]))
    out["copy_ms"] = {"runs": [round(r["copy"], 4) for r in runs], "median": round(cp, 4)}
    out["copy_bytes_moved"] = 2 * text_bytes
    out["copy_gb_per_s"] = round(2 * text_bytes / (cp * 1e-3) / 1e9, 1)
    out["copy_fraction_of_peak"] = round(2 * text_bytes / (cp * 1e-3) / PEAK_HBM, 3)
    out["decode_byte_rate_over_copy_byte_rate"] = round(out["decode_gb_per_s"] / out["copy_gb_per_s"], 3)
    tx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
