// tgsf_text_kernels.h -- the kernels of libtgsf_text.so (include/tgsf_text.h): what its sides share, then a header a side.
//
//   tgsf_text_index.h    the record index of FASTQ / FASTA text (k_text_*)
//   tgsf_text_out.h      the kept records as clean text (k_textout_*)
//   tgsf_text_bam.h      unaligned BAM records -> text and its index (k_bam_*)
//   tgsf_text_inflate.h  BGZF members -> their inflated bytes (k_bgzf_inflate, k_bgzf_finish)
//   tgsf_text_crc.h      the CRC32 the check and the deflate need (k_bgzf_crc)
//   tgsf_text_deflate.h  text -> BGZF members, both levels (k_gz_*)
// Here: the wave primitives, the constants of the wave-per-piece kernels, and the one scan of this library --
//   k_text_scan_tiles  } exclusive prefix sums: the scheme of k_scan_tiles / k_scan_top in tgsf_kernels.h, restated here once
//   k_textout_scan_top } (k_text_scan_tiles<uint32_t> and <uint64_t>, text_scan_top; the index has a top kernel of its own,
//                        k_text_scan_top); the offset of a block of counts is added by the reader, not by a third launch
// Compiled by hipcc for gfx950 and, with -DTGSF_EMUL, by g++ for the serial emulation of tests/emul, in which every lane
// is a wave of one (kTextLanes = 1).  The wave primitives this library adds to tgsf_hip.h / tgsf_emul.h follow, each with
// its one-lane stand-in: those `#if !defined(TGSF_EMUL)` branches are the only lines the emulation does not run.
#pragma once
#include <stdint.h>
#if defined(TGSF_EMUL)
#include "tgsf_emul.h"
#else
#include "tgsf_hip.h"
#endif
#include "../../include/tgsf_text.h"

namespace tgsf {

typedef unsigned long long text_ull;

#if !defined(TGSF_EMUL)
constexpr uint32_t kTextLanes = 64;
// sum of v over the lanes below this one
TGSF_D uint32_t wave_excl_scan(uint32_t v)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64); if (lane >= o) x += y; }
    return x - v;
}
// a value every lane of the wave holds (loaded from LDS or global memory at a wave-uniform address), as a scalar: what is
// computed from it and branched on stays on the scalar side
TGSF_D uint32_t wave_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
TGSF_D uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64); v = u < v ? u : v; }
    return v;
}
// Global-memory stores of this wave's lanes, made before it, are seen by the loads any of its lanes makes behind it.  The rule
// of the memory model relied on: a workgroup-scope fence orders a wave's earlier stores before its later loads for every
// observer of the workgroup, and the waves of a workgroup share their CU's vector L1 (the build never uses threadgroup-split
// mode), so a store that has been waited for (s_waitcnt vmcnt(0), which the fence emits) is what a later load of the CU returns.
// (Kept here and not in tgsf_hip.h: that file is part of libtgsf's kernel sources, whose profiles are stamped with its hash.)
#define TGSF_WG_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)
// a value every lane of the wave holds, moved to scalar registers (loads that depend on it become scalar loads)
TGSF_D uint64_t wave_uniform64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}
#else
#define TGSF_WG_FENCE() ((void)0)             /* one lane at a time: every store has happened before the next load */
constexpr uint32_t kTextLanes = 1;
TGSF_HD uint32_t wave_excl_scan(uint32_t) { return 0; }
TGSF_HD uint32_t wave_first(uint32_t v) { return v; }
TGSF_HD uint32_t wave_min(uint32_t v) { return v; }
TGSF_HD uint64_t wave_uniform64(uint64_t v) { return v; }
#endif
// the lowest v of the wave into *lowest, by one atomic of its leader (0xFFFFFFFF in every lane: none)
TGSF_D void wave_min_into(uint32_t* lowest, uint32_t v)
{
    v = wave_min(v);
    if (wave_leader() && v != 0xFFFFFFFFu) atomicMin(lowest, v);
}

constexpr uint32_t kTextThreads = 256;                    // lanes of a workgroup of the wave-per-piece kernels
constexpr uint32_t kTextPiece = 4096;                     // bytes of text a wave marks / emits: 4 loads of 16 bytes a lane
constexpr uint32_t kTextPieceChunks = kTextPiece / 16;    // 16-byte chunks (one uint16 of bits each)
constexpr uint32_t kTextPieceWords = kTextPiece / 64;     // 64-bit words of bits
constexpr uint32_t kTextEmitPieces = 4;                   // pieces a wave of k_text_emit turns into positions (four loads under way a lane)
constexpr uint32_t kTextScanTile = 4096;                  // counts one block of k_text_scan_tiles sums
constexpr uint32_t kInfWaves = kTextThreads / 64;         // table sets of a workgroup: its waves (the emulation's lanes, waves of one
                                                          // that run one after the other, take turns on them)
static_assert(kTextPieceWords == 64, "k_text_emit: one word of bits per lane");

TGSF_D uint32_t text_lane() { return threadIdx.x % kTextLanes; }
TGSF_D uint64_t text_wave() { return (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kTextLanes; }

// little-endian fields at any alignment (BAM records, BGZF trailers)
TGSF_HD uint32_t bam_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
TGSF_HD uint32_t bam_le32(const uint8_t* p) { return bam_le16(p) | bam_le16(p + 2) << 16; }

// a[0..n) -> exclusive prefix sums within blocks of kTextScanTile entries, in place; part[b] = the block's total
template <typename T> TGSF_KERNEL k_text_scan_tiles(T* a, uint64_t n, uint64_t* part)
{
    TGSF_SHARED T sums[1024];
    const uint32_t B = blockDim.x, per = (kTextScanTile + B - 1) / B;
    const uint64_t base = blockIdx.x * (uint64_t)kTextScanTile;
    const uint64_t lo = base + threadIdx.x * per;
    uint64_t hi = lo + per;
    if (hi > base + kTextScanTile) hi = base + kTextScanTile;
    if (hi > n) hi = n;
    T s = 0;
    for (uint64_t i = lo; i < hi; i++) s += a[i];
    sums[threadIdx.x] = s;
    TGSF_BLOCK_SYNC();
    if (threadIdx.x == 0) {
        T acc = 0;
        for (uint32_t t = 0; t < B; t++) { const T x = sums[t]; sums[t] = acc; acc += x; }
        part[blockIdx.x] = acc;
    }
    TGSF_BLOCK_SYNC();
    T acc = sums[threadIdx.x];
    for (uint64_t i = lo; i < hi; i++) { const T x = a[i]; a[i] = acc; acc += x; }
}
// part[0..nb) -> exclusive prefix sums, by the one lane that calls it; returns the total (nb == 0: 0).  64-bit: a chunk of
// newlines only has more than 2^32 of them
TGSF_D uint64_t text_scan_top(uint64_t* part, uint32_t nb)
{
    uint64_t acc = 0;
    for (uint32_t b = 0; b < nb; b++) { const uint64_t x = part[b]; part[b] = acc; acc += x; }
    return acc;
}
// part[0..nb) -> exclusive prefix sums; the total (nb == 0: 0)
TGSF_KERNEL k_textout_scan_top(uint64_t* part, uint32_t nb, uint64_t* total)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *total = text_scan_top(part, nb);
}

}  // namespace tgsf

#include "tgsf_text_index.h"
#include "tgsf_text_out.h"
#include "tgsf_text_bam.h"
#include "tgsf_text_inflate.h"
#include "tgsf_text_crc.h"
#include "tgsf_text_deflate.h"
