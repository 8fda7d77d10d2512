#!/usr/bin/env python3
"""Times the BGZF output side of libtgsf_text on the GPU: the deflate of a chunk of FASTQ text as the format
stage leaves it in the object's output buffer (k_gz_count, the scan, k_gz_emit), beside that format's own stage times for
the same text; k_bgzf_crc on the members tools/text_bgzf_measure.py inflates; and zlib with Z_HUFFMAN_ONLY and at level 1 on
one CPU thread over the same text, all of it (--zlib-members: its first members; 0: none).  --level sets the coder (0: Huffman-only, 1: the match search; with it
zlib at level 6 is timed too), --text the text: synth, the HiFi-like reads of tgsfilter_amd/synth.py as the goldens have
them (random bases, Gaussian qualities), or hifi_like, tests/gzlzmodel.py's (qualities in runs, names with a long common
prefix).  Each GPU figure is the median of --reps calls, by a host clock around a call that ends in
a synchronise, after one warm-up call; device_ms is the kernels alone, by HIP events.  Prints one JSON line; --out writes it
to a file too.

    python tools/text_gzout_measure.py --members 4096 --reps 7 --out gzout_measure.json
    python tools/text_gzout_measure.py --members 4096 --reps 7 --level 1 --text hifi_like
"""
import argparse
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bgzfmodel as gm, gzlzmodel as lm, gzoutmodel as zm, textoutparity as top, textparity  # noqa: E402
from tgsfilter_amd import abi, synth, text as tgtext  # noqa: E402
from tools.text_bgzf_measure import median_ms, records  # noqa: E402


def zlib_rate(text, level, strategy):
    """GB/s of text in, and the compressed share, of one thread over members of 0xFF00 bytes."""
    size, t0 = 0, time.perf_counter()
    for lo, hi in zm.cuts(len(text)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        size += len(co.compress(text[lo:hi]) + co.flush()) + zm.FRAME
    return len(text) / (time.perf_counter() - t0) / 1e9, size / len(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4096, help="members of 0xFF00 bytes of text to deflate, and of BAM to check")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=0, choices=(0, 1), help="tgsf_text_bgzf_out_level")
    ap.add_argument("--text", default="synth", choices=("synth", "hifi_like"))
    ap.add_argument("--zlib-members", type=int, default=None, help="members zlib is timed on (default: all of the text; 0: none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    res = {"members": a.members, "reps": a.reps, "level": a.level, "text": a.text}

    # HiFi-like reads as the goldens have them, as many as fill the members; the format of all of them whole leaves the text
    # in the object's output buffer, which is where the deflate takes it from
    want = a.members * zm.MEMBER
    if a.text == "synth":
        reads = synth.make_reads(11, min(max(want // 30000, 4), 256), "hifi", mean_len=15000, zoo=False)
        text = textparity.fastq_of(reads)                               # (a few MB of different reads, repeated)
    else:
        text = lm.hifi_like(np.random.default_rng(1), min(want, 64 * zm.MEMBER) + 5000)
        text = text[:text.rfind(b"\n@") + 1]
    while len(text) < want:
        text += text
    text = text[:text.rfind(b"\n@", 0, want) + 1]
    tx = tgtext.TextIndexer(0, len(text), len(text) // 1500 + 16, None)
    if a.level:
        tx.set_bgzf_level(a.level)
    idx, s = tx.index(text)
    n = s["n_records"]
    assert s["stop"] == tgtext.END and s["consumed"] == len(text) and n > 0
    rd, fr = top.tables(n, [(r, 0, int(idx.len[r]), abi.FF_PASS) for r in range(n)])
    tx.reserve_output(n + 16, len(text) + 4096)
    tx.reserve_bgzf_out(len(text) + 4096)
    tx.profile(True)
    out, _, _ = tx.format(n, rd, fr)
    assert out == text
    tx.format(n, rd, fr)
    res["format_stage_ms"] = tx.stage_ms()
    res["format_stage_ms"]["sum"] = sum(res["format_stage_ms"].values())

    def deflate():
        tx.deflate_device(len(text), True, out_capacity=1 << 62)        # (the object's output buffer into its compressed buffer)
        tx.fetch(want_index=False)

    med, lo, hi = median_ms(deflate, a.reps)
    gz, _, sg = tx.deflate(text)                                        # the host form: the bytes to check, and the kernels' own time
    assert gzip.decompress(gz) == text
    res["deflate"] = {"text_bytes": len(text), "gz_bytes": len(gz), "share": len(gz) / len(text), "stored": sg["stored"], "ms_median": med, "ms_min": lo,
                      "ms_max": hi, "text_GB_per_s": len(text) / med / 1e6, "device_ms": sg["device_ms"],
                      "kernels_text_GB_per_s": len(text) / sg["device_ms"] / 1e6 if sg["device_ms"] else None,
                      "note": "call time: memset, k_gz_count, two scan launches, k_gz_emit, one synchronise; device_ms: the same by HIP events"}
    tx.close()
    ztext = text if a.zlib_members is None else text[:a.zlib_members * zm.MEMBER]
    coders = [("zlib_huffman_only_one_thread", 6, zlib.Z_HUFFMAN_ONLY), ("zlib_level_1_one_thread", 1, zlib.Z_DEFAULT_STRATEGY)]
    if a.level:
        coders.append(("zlib_level_6_one_thread", 6, zlib.Z_DEFAULT_STRATEGY))
    for key, level, strategy in coders if ztext else []:
        rate, share = zlib_rate(ztext, level, strategy)
        res[key] = {"text_GB_per_s": rate, "share": share, "text_bytes": len(ztext)}

    # the CRC check on the members of tools/text_bgzf_measure.py: 64 different members of 0xFF00 inflated bytes, repeated
    pool = records(rng, 15000, 64 * 0xFF00)
    kinds = [gm.zmember(pool[i * 0xFF00:(i + 1) * 0xFF00]) for i in range(64)]
    bam_gz = b"".join(kinds[b % 64] for b in range(a.members))
    out_bytes = a.members * 0xFF00
    tx = tgtext.TextIndexer(0, 1 << 20, 16, None)
    tx.reserve_bgzf(len(bam_gz), a.members)
    blocks, stop, consumed, ob = tgtext.bgzf_walk(bam_gz, a.members)
    assert (len(blocks), consumed, ob) == (a.members, len(bam_gz), out_bytes)
    d_gz = torch.from_numpy(np.frombuffer(bam_gz + bytes(-len(bam_gz) % 16), np.uint8).copy()).to(dev)
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    d_bad = torch.zeros(4, dtype=torch.int32, device=dev)
    tx.inflate_device(len(bam_gz), blocks, stop, d_out.data_ptr(), out_bytes, d_gz=d_gz.data_ptr())
    tx.fetch(want_index=False)

    def crc():
        tx.crc_device(blocks, d_bad.data_ptr(), d_gz=d_gz.data_ptr(), d_inflated=d_out.data_ptr())
        tx.fetch(want_index=False)

    med, lo, hi = median_ms(crc, a.reps)
    assert int(d_bad[0].item()) == -1
    res["crc"] = {"inflated_bytes": out_bytes, "ms_median": med, "ms_min": lo, "ms_max": hi, "inflated_GB_per_s": out_bytes / med / 1e6,
                  "note": "call time: table upload, memset, k_bgzf_crc, one synchronise"}
    t0 = time.perf_counter()
    for i in range(64):
        zlib.crc32(pool[i * 0xFF00:(i + 1) * 0xFF00])
    res["zlib_crc32_one_thread_GB_per_s"] = 64 * 0xFF00 / (time.perf_counter() - t0) / 1e9
    tx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
