"""Measurement of the output side of libtgsf_text on an MI355X (k_textout_*): the identity workload --
one text of more than 5 GiB resident in HBM (tests/textparity.full_size_block repeated), one whole-read PASS fragment per
read, the tables made on the device -- formatted with tgsf_text_profile on; the three stages by HIP events, median of
--reps after a warm-up call.  The comparator, in the same process: a device-to-device hipMemcpyAsync of n_bytes bytes (torch's
Tensor.copy_), the same algorithmic traffic: one read and one write of the output.  Prints one JSON line.  Under
`rocprofv3 --kernel-trace --stats -- python ...` the same run gives profiles/text_format_kernel_stats.csv.

    python tests/manual/text_format_measure.py [--gib 5] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import textparity                       # noqa: E402
from tgsfilter_amd import abi, text as tgtext      # noqa: E402

PEAK_HBM = 8.0e12          # bytes/s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    block, bidx = textparity.full_size_block()
    per = len(bidx["len"])
    reps = int(a.gib * (1 << 30)) // block.size + 1
    n_bytes, nrec = reps * block.size, reps * per
    d_text = torch.from_numpy(block).to(dev).repeat(reps)
    ar = torch.arange(nrec, dtype=torch.int32, device=dev)
    d_reads = torch.zeros((nrec, 8), dtype=torch.int32, device=dev)         # tgsf_read_result: n_frags, frag_begin are words 3, 4
    d_reads[:, 3], d_reads[:, 4] = 1, ar
    d_frags = torch.zeros((nrec, 6), dtype=torch.int32, device=dev)         # tgsf_fragment: read, start, len, flags are words 2..5
    d_frags[:, 2], d_frags[:, 4], d_frags[:, 5] = ar, torch.from_numpy(bidx["len"].astype(np.int32)).to(dev).repeat(reps), abi.FF_PASS
    d_out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out = {"n_bytes": n_bytes, "n_records": nrec, "n_frags": nrec}

    tx = tgtext.TextIndexer(0, n_bytes, nrec)
    tx.reserve_output(nrec, 16)
    tx.profile(True)
    tx.index_device(n_bytes, d_text=d_text.data_ptr())
    _, s = tx.fetch(want_index=False)
    assert s["n_records"] == nrec and s["stop"] == tgtext.END, s

    def one():
        tx.format_device(nrec, d_reads.data_ptr(), d_frags.data_ptr(), nrec, d_text=d_text.data_ptr(), d_out=d_out.data_ptr(), out_capacity=n_bytes,
                         d_summary=d_sum.data_ptr())
        return tx.stage_ms()                                                # (waits for the format)

    one()                                                                   # warm-up
    sm = tgtext.OutSummary.from_buffer_copy(d_sum.cpu().numpy().tobytes())
    assert (sm.n_bytes, sm.n_records, sm.stop) == (n_bytes, nrec, tgtext.END), sm.as_dict()
    assert torch.equal(d_out, d_text)
    runs = [one() for _ in range(a.reps)]
    med = {k: float(np.median([r[k] for r in runs])) for k in ("sizes", "layout", "copy")}
    total = float(np.median([sum(r.values()) for r in runs]))
    out["format_ms"] = {"runs": [{k: round(v, 4) for k, v in r.items()} for r in runs], "median": {k: round(v, 4) for k, v in med.items()},
                        "median_total": round(total, 4)}
    out["copy_gb_per_s"] = round(2 * n_bytes / (med["copy"] * 1e-3) / 1e9, 1)
    out["floor_ms"] = round(2 * n_bytes / PEAK_HBM * 1e3, 4)

    # the comparator: hipMemcpyAsync device to device, n_bytes bytes, by HIP events on the current stream
    d_copy = torch.empty_like(d_out)
    ms = []
    for k in range(a.reps + 1):                                             # the first is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d_copy.copy_(d_text, non_blocking=True)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    out["memcpy_d2d_ms"] = {"runs": [round(x, 4) for x in ms], "median": round(float(np.median(ms)), 4)}
    out["ratio_format_to_memcpy"] = round(total / float(np.median(ms)), 3)
    out["ratio_copy_kernel_to_memcpy"] = round(med["copy"] / float(np.median(ms)), 3)
    out["bar_1p5x_met"] = bool(total <= 1.5 * float(np.median(ms)))
    tx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
