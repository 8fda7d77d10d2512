"""Measurement of libtgsf_text on an MI355X (k_text_*): one text of more than 5 GiB resident in HBM
(tests/textparity.full_size_block repeated), indexed with tgsf_text_profile on; the stats_raw stage of the unchanged filter
pipeline on the same text in the same process as the comparator; wall times of the one-call form against tgsf_submit with a
host-made index.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python ... --no-wall` the same run gives
profiles/text_index_kernel_stats.csv.

    python tests/manual/text_index_measure.py [--gib 5] [--reps 5] [--no-wall]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import textparity                                   # noqa: E402
from tgsfilter_amd import abi, capi, synth, text as tgtext     # noqa: E402

PEAK_HBM = 8.0e12          # bytes/s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-wall", action="store_true", help="skip the host-text wall-time comparison (profiling runs)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    block, bidx = textparity.full_size_block()
    per = len(bidx["len"])
    reps = int(a.gib * (1 << 30)) // block.size + 1
    n_bytes, nrec = reps * block.size, reps * per
    d_text = torch.from_numpy(block).to(dev).repeat(reps)
    torch.cuda.synchronize()
    out = {"n_bytes": n_bytes, "n_records": nrec, "bases": int(bidx["len"].astype(np.uint64).sum()) * reps}

    tx = tgtext.TextIndexer(0, n_bytes, nrec + 8)
    tx.profile(True)
    tx.index_device(n_bytes, d_text=d_text.data_ptr())
    _, s = tx.fetch(want_index=False)                          # warm-up
    assert s["n_records"] == nrec and s["stop"] == tgtext.END and s["consumed"] == n_bytes, s
    ms = []
    for _ in range(a.reps):
        tx.index_device(n_bytes, d_text=d_text.data_ptr())
        _, s = tx.fetch(want_index=False)
        ms.append(s["device_ms"])
    out["index_device_ms"] = {"runs": [round(x, 4) for x in ms], "median": round(float(np.median(ms)), 4)}
    extra = 2 * (n_bytes // 8) + 2 * 8 * 4 * nrec + 28 * nrec          # bits written + read, table written + read, index written
    out["floor"] = {"one_read_ms": round(n_bytes / PEAK_HBM * 1e3, 4), "extra_bytes": extra,
                    "with_extra_ms": round((n_bytes + extra) / PEAK_HBM * 1e3, 4)}

    # the comparator: stats_raw of the filter pipeline on the same text, read in place through the device index
    p = abi.make_params("ont", adapters=[synth.ONT_RAPID, synth.ONT_RAPID_RC], min_len=1000, min_q=10.0, head_trim=0, tail_trim=0,
                        max_batch_bases=n_bytes + 64, max_batch_reads=nrec, max_read_len=int(bidx["len"].max()))
    ctx = capi.Context(p, 0)
    b = tx.buffers()
    fcap = n_bytes // 1000 + nrec + 16
    d_reads = torch.empty(nrec * 32, dtype=torch.uint8, device=dev)
    d_frags = torch.zeros(fcap * 24, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def one_batch():
        ctx.submit_device(d_text.data_ptr(), d_text.data_ptr(), b.index.seq_off, b.index.len, nrec, n_bytes, d_reads.data_ptr(),
                          d_frags.data_ptr(), fcap, d_nf.data_ptr(), None, d_qual_offsets=b.index.qual_off)
        ctx.wait()

    one_batch()                                                # warm-up
    ctx.profile(True)
    for _ in range(a.reps):
        one_batch()
    st, nb = ctx.stage_times()
    out["pipeline_stage_ms_per_batch"] = {k: round(v / nb, 4) for k, v in st.items()}
    out["stats_raw_ms"] = round(st["stats_raw"] / nb, 4)
    out["bar_1p5x_stats_raw_ms"] = round(1.5 * st["stats_raw"] / nb, 4)
    out["bar_met"] = bool(out["index_device_ms"]["median"] <= 1.5 * st["stats_raw"] / nb)
    ctx.profile(False)

    if not a.no_wall:
        host = d_text.cpu().numpy()
        idx_host = {f: np.tile(bidx[f], reps) for f in ("len",)}
        shift = (np.arange(reps, dtype=np.uint64) * np.uint64(block.size)).repeat(per)
        off, qoff = np.tile(bidx["seq_off"], reps) + shift, np.tile(bidx["qual_off"], reps) + shift
        walls = {"text_submit_s": [], "submit_host_index_s": []}
        for k in range(2):                                     # the first of each is the warm-up
            t0 = time.perf_counter()
            _, s2, r1, f1 = tx.submit(ctx, host, frag_capacity=fcap, want_index=False)
            walls["text_submit_s"].append(round(time.perf_counter() - t0, 3))
            t0 = time.perf_counter()
            r0, f0 = ctx.submit(host, host, off, idx_host["len"], frag_capacity=fcap, qual_offsets=qoff)
            walls["submit_host_index_s"].append(round(time.perf_counter() - t0, 3))
            assert s2["n_records"] == nrec and np.array_equal(r0, r1) and np.array_equal(f0, f1)
        out["wall"] = walls
    tx.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
