// tgsf_text_kernels.h -- the kernels of libtgsf_text.so (include/tgsf_text.h): the record index of FASTQ / FASTA text.
//
//   k_text_mark        one streaming read of the text, 16 bytes a lane: a bit per byte ('\n' or not) and the number of
//                      line ends of every 4 KiB piece (one wave's share).  The text is not read again as a stream.
//   k_text_scan_tiles  } exclusive prefix sums of those counts: the scheme of k_scan_tiles / k_scan_top in tgsf_kernels.h,
//   k_text_scan_top    } restated here once for every scan of this library (k_text_scan_tiles<uint32_t> and <uint64_t>,
//                        text_scan_top); the offset of a block of counts is added by the reader, not by a third launch
//   k_text_emit        every wave turns the bits of four pieces into 64-bit positions, in order, at each piece's offset of
//                      the line-end table (lane prefix count, no atomics); only the first 4 * max_records are kept
//   k_text_check       a lane per group of 4 (2) lines: five table entries, the first byte of lines 0 and 2, the byte in
//                      front of each line end ('\r'); writes the record's index words, folds the first irregular group
//   k_text_fold        bases and longest over the records of the index (per wave first, then one atomic); k_text_fold<TextState>
//                      here, k_text_fold<BamState> on the BAM input side
//   k_text_finish      one lane: n_records, consumed, why the index ends
//
// Compiled by hipcc for gfx950 and, with -DTGSF_EMUL, by g++ for the serial emulation of tests/emul, in which every lane
// is a wave of one (kTextLanes = 1).  The wave primitives this file adds to tgsf_hip.h / tgsf_emul.h follow, each with
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
#else
#define TGSF_WG_FENCE() ((void)0)             /* one lane at a time: every store has happened before the next load */
constexpr uint32_t kTextLanes = 1;
TGSF_HD uint32_t wave_excl_scan(uint32_t) { return 0; }
TGSF_HD uint32_t wave_first(uint32_t v) { return v; }
TGSF_HD uint32_t wave_min(uint32_t v) { return v; }
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
static_assert(kTextPieceWords == 64, "k_text_emit: one word of bits per lane");

TGSF_D uint32_t text_lane() { return threadIdx.x % kTextLanes; }
TGSF_D uint64_t text_wave() { return (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / kTextLanes; }

// what the kernels keep between launches (device memory)
struct TextState {
    uint64_t total;        // line ends of the chunk
    uint64_t lines;        // lines: total, plus the unterminated tail of a final chunk
    uint64_t bases;
    uint32_t first_bad;    // first group that is not regular (0xFFFFFFFF: none)
    uint32_t longest;
};

// bit i = byte i of x is '\n'
TGSF_HD uint32_t newline_bits4(uint32_t x)
{
    x ^= 0x0A0A0A0Au;
    const uint32_t nz = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;          // bit 7 of a byte: the byte is not zero
    return ((((~nz & 0x80808080u) >> 7) * 0x00204081u) >> 21) & 0xFu;   // bits 0, 8, 16, 24 -> 21, 22, 23, 24 (no carries)
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_text_mark(const uint8_t* __restrict__ text, uint64_t n, uint64_t n_pieces,
                                                     uint16_t* __restrict__ bits, uint32_t* __restrict__ cnt)
{
    const uint64_t piece = text_wave();
    if (piece >= n_pieces) return;                                     // (wave-uniform)
    constexpr uint32_t per = kTextPieceChunks / kTextLanes;            // chunks a lane takes: 4, a wave's 64 lanes side by side (emulation: all 256)
    const uint64_t chunk0 = piece * kTextPieceChunks + text_lane();
    const uint64_t last = ((n - 1) / 16u) * 16u;                       // the last chunk that holds text (n > 0: there are pieces)
    uint4 v[per];
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {                               // every load under way before the first is looked at
        const uint64_t at = (chunk0 + j * kTextLanes) * 16u;
        v[j] = *reinterpret_cast<const uint4*>(text + (at < n ? at : last));   // (readable up to n rounded up to 16)
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        const uint64_t at = (chunk0 + j * kTextLanes) * 16u;
        uint32_t m = newline_bits4(v[j].x) | newline_bits4(v[j].y) << 4 | newline_bits4(v[j].z) << 8 | newline_bits4(v[j].w) << 12;
        if (at >= n) m = 0;
        else if (n - at < 16u) m &= (1u << (uint32_t)(n - at)) - 1u;   // bytes at and behind n do not count
        bits[chunk0 + j * kTextLanes] = (uint16_t)m;                   // (the whole piece is written: no stale bits)
        c += popc32(m);
    }
    c = (uint32_t)wave_sum_i32((int32_t)c);
    if (wave_leader()) cnt[piece] = c;
}

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
// ... of the line ends; resets the state
TGSF_KERNEL k_text_scan_top(uint64_t* part, uint32_t nb, TextState* S)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t acc = text_scan_top(part, nb);
    S->total = acc; S->lines = acc; S->bases = 0; S->first_bad = 0xFFFFFFFFu; S->longest = 0;
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_text_emit(const uint64_t* __restrict__ bits, const uint32_t* __restrict__ excl,
                                                     const uint64_t* __restrict__ part, uint64_t n_pieces,
                                                     uint64_t* __restrict__ table, uint64_t cap)
{
    const uint64_t p0 = text_wave() * kTextEmitPieces;
    if (p0 >= n_pieces) return;                                        // (wave-uniform, as every branch around a wave operation here)
    constexpr uint32_t per = kTextPieceWords / kTextLanes;             // words of a piece a lane holds: 1 (emulation: all 64)
    uint64_t m[kTextEmitPieces][per];
#pragma unroll
    for (uint32_t q = 0; q < kTextEmitPieces; q++)                     // all loads first: the pass is bound by latency, not by bytes
#pragma unroll
        for (uint32_t j = 0; j < per; j++)
            m[q][j] = p0 + q < n_pieces ? bits[(p0 + q) * kTextPieceWords + text_lane() * per + j] : 0ull;
#pragma unroll
    for (uint32_t q = 0; q < kTextEmitPieces; q++) {
        const uint64_t piece = p0 + q;
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < per; j++) c += popc64(m[q][j]);
        if (!wave_any(c != 0)) continue;
        uint64_t pos = part[piece / kTextScanTile] + excl[piece];
        if (pos >= cap) return;                                        // (so are all later pieces)
        pos += wave_excl_scan(c);
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {
            uint64_t w = m[q][j];
            const uint64_t byte0 = (piece * kTextPieceWords + text_lane() * per + j) * 64u;
            while (w) {
                if (pos < cap) table[pos] = byte0 + (uint32_t)__builtin_ctzll(w);
                pos++;
                w &= w - 1;
            }
        }
    }
}

// the unterminated tail of a final chunk is a line (FastxReader::line: "a last line without '\n' is still a line")
TGSF_D uint64_t text_lines(const uint64_t* table, uint64_t total, uint64_t cap, uint64_t n, int final)
{
    if (!final || total > cap) return total;                           // (beyond cap lines are left over whatever the tail is)
    const uint64_t tail = total ? table[total - 1] + 1 : 0;
    return total + (tail < n ? 1u : 0u);
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_text_check(const uint8_t* __restrict__ text, uint64_t n, int fasta, int final,
                                                      const uint64_t* __restrict__ table, uint32_t max_records, TextState* S,
                                                      tgsf_text_index_arrays I)
{
    const uint32_t G = fasta ? 2u : 4u;
    const uint64_t total = S->total;
    const uint64_t lines = text_lines(table, total, (uint64_t)G * max_records, n, final);
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    if (gid == 0) S->lines = lines;
    const uint64_t groups = lines / G < max_records ? lines / G : max_records;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t g = gid; g < groups; g += stride) {
        uint64_t s[4], len[4];
        uint64_t prev = g ? table[G * g - 1] + 1 : 0;
        for (uint32_t k = 0; k < G; k++) {
            const uint64_t li = G * g + k;
            uint64_t e = li < total ? table[li] : n;                   // (li == total: the tail line)
            s[k] = prev;
            prev = e + 1;
            if (e > s[k] && text[e - 1] == '\r') e--;
            len[k] = e - s[k];
        }
        bool ok = len[0] > 0 && len[0] <= 0xFFFFFFFFull && len[1] > 0 && len[1] <= 0xFFFFFFFFull && text[s[0]] == (fasta ? '>' : '@');
        if (!fasta) ok = ok && len[2] > 0 && text[s[2]] == '+' && len[3] == len[1];
        if (ok) {
            I.seq_off[g] = s[1];
            I.qual_off[g] = fasta ? s[1] : s[3];
            I.len[g] = (uint32_t)len[1];
            I.name_off[g] = s[0] + 1;
            I.name_len[g] = (uint32_t)(len[0] - 1);
        } else if ((uint32_t)g < bad) bad = (uint32_t)g;
    }
    wave_min_into(&S->first_bad, bad);
}

// records of the index: the regular groups of G lines in front of the first that is not, max_records at most
TGSF_D uint32_t index_records(const TextState* S, uint32_t max_records, uint32_t G)
{
    const uint64_t groups = S->lines / G < max_records ? S->lines / G : max_records;
    return S->first_bad < groups ? S->first_bad : (uint32_t)groups;
}

// State: TextState (limit: max_records; fasta: 2 lines a record, not 4) or BamState (limit: n_walked); its index_records() counts
template <typename State>
TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_text_fold(const uint32_t* __restrict__ len, uint32_t limit, int fasta, State* S)
{
    const uint32_t nrec = index_records(S, limit, fasta ? 2u : 4u);
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    uint64_t sum = 0;
    uint32_t mx = 0;
    for (uint64_t g = gid; g < nrec; g += stride) { const uint32_t l = len[g]; sum += l; mx = l > mx ? l : mx; }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if (wave_leader() && mx) {
        atomicAdd((text_ull*)&S->bases, (text_ull)sum);
        atomicMax(&S->longest, mx);
    }
}

TGSF_KERNEL k_text_finish(uint64_t n, int fasta, int final, const uint64_t* table, uint32_t max_records, const TextState* S,
                          tgsf_text_summary* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t G = fasta ? 2u : 4u;
    const uint64_t groups = S->lines / G < max_records ? S->lines / G : max_records;
    const uint32_t k = index_records(S, max_records, G);
    const uint64_t last = (uint64_t)G * k;                             // lines of the index
    const uint64_t left = S->lines - last;
    uint32_t stop;
    if (k < groups) stop = TGSF_TEXT_IRREGULAR;
    else if (left == 0) stop = TGSF_TEXT_END;
    else if (k == max_records) stop = TGSF_TEXT_CAPACITY;
    else stop = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END;           // fewer lines than a group: garbage at the end, or a record to be continued
    out->n_records = k;
    out->stop = stop;
    out->consumed = !k ? 0 : (last - 1 < S->total ? table[last - 1] + 1 : n);
    out->bases = S->bases;
    out->longest = S->longest;
    out->device_ms = 0.0f;
}

// ---- the output side: the kept records as clean FASTQ / FASTA text (tgsf_text_format*) -------------------------------
//
//   k_textout_flag     a lane per fragment: 1 for TGSF_FF_PASS, else 0
//   (k_text_scan_tiles<uint32_t> / k_textout_scan_top: exclusive prefix sums of the flags -- a fragment's pass_num is its sum minus
//    the sum at its read's frag_begin, plus one; a read may have thousands of fragments, nobody walks them)
//   k_textout_size     a lane per fragment: the record's size (0 without PASS), for pass_num >= 2 where ":<n>" goes into the name
//   (k_text_scan_tiles<uint64_t> / k_textout_scan_top: exclusive prefix sums of the sizes, 64-bit)
//   k_textout_finish   a lane per fragment: the byte behind each record (ends[]; the caller's rec_end), the summary; decides CAPACITY
//   k_textout_copy     the hot path: waves stride over 4 KiB pieces of the OUTPUT; a lane owns aligned 16-byte chunks.  A chunk
//                      inside one sequence or quality stretch is one load16u and one store; a chunk that touches a seam is put
//                      together byte by byte by out_byte(), the only place that knows the layout (host/record_out.h).
#if !defined(TGSF_EMUL)
// a value every lane of the wave holds, moved to scalar registers (loads that depend on it become scalar loads)
TGSF_D uint64_t wave_uniform64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}
// 8 bytes at any alignment (one global_load_dwordx2)
struct __attribute__((packed, aligned(1))) U2u { uint32_t x, y; };
TGSF_D uint64_t load8u(const uint8_t* p) { const U2u* q = reinterpret_cast<const U2u*>(p); return (uint64_t)q->y << 32 | q->x; }
#else
TGSF_HD uint64_t wave_uniform64(uint64_t v) { return v; }
TGSF_HD uint64_t load8u(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
#endif

// what the output kernels keep between launches (device memory)
struct TextOutState {
    uint64_t n_records;    // fragments with TGSF_FF_PASS
    uint64_t n_bytes;      // bytes of the formatted text
    uint64_t bases;
};
// per fragment: where ":<pass_num>" goes into the name (name_len: behind it), and pass_num (0: no record)
struct TextOutMeta { uint32_t sfx, pass_num; };

TGSF_HD uint32_t textout_digits(uint32_t v) { uint32_t d = 0; for (; v; v /= 10) d++; return d; }
// record_bytes() of host/record_out.h
TGSF_HD uint64_t textout_record_bytes(uint32_t name_len, uint32_t len, uint32_t pass_num, int fastq)
{
    uint64_t name = name_len;
    if (pass_num >= 2) name += 1u + textout_digits(pass_num);
    return 1 + name + 1 + (uint64_t)len + (fastq ? 3 + (uint64_t)len : 0) + 1;
}
// an exclusive sum of the two-level scans: the block's offset is added by the reader
TGSF_D uint64_t textout_sum32(const uint32_t* excl, const uint64_t* part, uint64_t i) { return part[i / kTextScanTile] + excl[i]; }

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_textout_flag(const tgsf_fragment* __restrict__ frags, uint64_t n_frags, uint32_t* __restrict__ pass,
                                                        TextOutState* S)
{
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    if (gid == 0) S->bases = 0;
    for (uint64_t f = gid; f < n_frags; f += stride) pass[f] = frags[f].flags & TGSF_FF_PASS ? 1u : 0u;
}

// part[0..nb) -> exclusive prefix sums; the total (nb == 0: 0)
TGSF_KERNEL k_textout_scan_top(uint64_t* part, uint32_t nb, uint64_t* total)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *total = text_scan_top(part, nb);
}

TGSF_HD bool textout_isspace(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }    // " \t\n\v\f\r" (newSeqName)

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_textout_size(const uint8_t* __restrict__ text, tgsf_text_index_arrays I,
                                                        const tgsf_read_result* __restrict__ reads, const tgsf_fragment* __restrict__ frags,
                                                        uint64_t n_frags, int fastq, const uint32_t* __restrict__ pass_excl,
                                                        const uint64_t* __restrict__ pass_part, uint64_t* __restrict__ size,
                                                        TextOutMeta* __restrict__ meta, TextOutState* S)
{
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    uint64_t bases = 0;
    for (uint64_t f = gid; f < n_frags; f += stride) {
        uint64_t sz = 0;
        TextOutMeta m = {0u, 0u};
        if (frags[f].flags & TGSF_FF_PASS) {
            const uint32_t r = frags[f].read, len = (uint32_t)frags[f].len, nl = I.name_len[r];
            m.pass_num = (uint32_t)(textout_sum32(pass_excl, pass_part, f) - textout_sum32(pass_excl, pass_part, reads[r].frag_begin)) + 1u;
            m.sfx = nl;
            if (m.pass_num >= 2) {                                     // only here is the name looked at
                const uint8_t* nm = text + I.name_off[r];
                for (uint32_t k = 0; k < nl; k++) if (textout_isspace(nm[k])) { m.sfx = k; break; }
            }
            sz = textout_record_bytes(nl, len, m.pass_num, fastq);
            bases += len;
        }
        size[f] = sz;
        meta[f] = m;
    }
    bases = wave_sum(bases);
    if (wave_leader() && bases) atomicAdd((text_ull*)&S->bases, (text_ull)bases);
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_textout_finish(const uint64_t* __restrict__ size_excl, const uint64_t* __restrict__ size_part,
                                                          const uint32_t* __restrict__ pass_excl, const uint64_t* __restrict__ pass_part,
                                                          const TextOutMeta* __restrict__ meta, uint64_t n_frags, uint64_t capacity,
                                                          const TextOutState* S, uint64_t* __restrict__ ends, uint64_t* __restrict__ rec_end,
                                                          tgsf_text_out_summary* out)
{
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    const uint64_t total = S->n_bytes;
    const bool fits = total <= capacity;
    if (gid == 0) {
        out->n_bytes = total;
        out->bases = S->bases;
        out->n_records = (uint32_t)S->n_records;
        out->stop = fits ? TGSF_TEXT_END : TGSF_TEXT_CAPACITY;
        out->device_ms = 0.0f;
        out->reserved = 0;
    }
    for (uint64_t f = gid; f < n_frags; f += stride) {
        const uint64_t e = f + 1 == n_frags ? total : size_part[(f + 1) / kTextScanTile] + size_excl[f + 1];
        ends[f] = e;
        if (rec_end && fits && meta[f].pass_num) rec_end[textout_sum32(pass_excl, pass_part, f)] = e;
    }
}

// one output record, as the copy needs it
struct TextOutRec {
    uint64_t begin, end;               // bytes of the output
    const uint8_t *name, *seq, *qual;  // in the text
    uint32_t name_len, len, sfx, pass_num, digits;
};
TGSF_D TextOutRec textout_rec(uint64_t f, const uint64_t* __restrict__ ends, const tgsf_fragment* __restrict__ frags,
                              const TextOutMeta* __restrict__ meta, const tgsf_text_index_arrays& I, const uint8_t* __restrict__ text)
{
    TextOutRec R;
    R.begin = f ? ends[f - 1] : 0;                                     // (fragments without a record have the end of the one before)
    R.end = ends[f];
    const uint32_t r = frags[f].read;
    const uint64_t start = (uint64_t)(uint32_t)frags[f].start;
    R.len = (uint32_t)frags[f].len;
    R.sfx = meta[f].sfx;
    R.pass_num = meta[f].pass_num;
    R.digits = R.pass_num >= 2 ? textout_digits(R.pass_num) : 0u;
    R.name = text + I.name_off[r];
    R.name_len = I.name_len[r];
    R.seq = text + I.seq_off[r] + start;
    R.qual = text + I.qual_off[r] + start;
    return R;
}
// THE LAYOUT: byte `pos` of the record.  '@' or '>', the name with ":<pass_num>" in front of its first white space from
// the read's second record on, '\n', the bases, for FASTQ "\n+\n" and the qualities, '\n'.
TGSF_D uint8_t out_byte(const TextOutRec& R, uint64_t pos, int fastq)
{
    if (pos == 0) return fastq ? '@' : '>';
    pos -= 1;
    const uint64_t name = (uint64_t)R.name_len + (R.digits ? 1u + R.digits : 0u);
    if (pos < name) {
        if (!R.digits || pos < R.sfx) return R.name[pos];
        const uint32_t k = (uint32_t)pos - R.sfx;                      // within ":<pass_num>" or behind it
        if (k == 0) return ':';
        if (k > R.digits) return R.name[pos - 1u - R.digits];
        uint32_t v = R.pass_num;
        for (uint32_t d = R.digits - k; d; d--) v /= 10;
        return (uint8_t)('0' + v % 10);
    }
    pos -= name;
    if (pos == 0) return '\n';
    pos -= 1;
    if (pos < R.len) return R.seq[pos];
    pos -= R.len;
    if (!fastq || pos == 3u + (uint64_t)R.len) return '\n';
    if (pos < 3) return pos == 1 ? '+' : '\n';
    return R.qual[pos - 3];
}
// where the 16 bytes at `pos` of the record come from when they lie within the bases or within the qualities; else NULL
TGSF_D const uint8_t* textout_plain(const TextOutRec& R, uint64_t pos, int fastq)
{
    const uint64_t s0 = 2u + (uint64_t)R.name_len + (R.digits ? 1u + R.digits : 0u);
    if (pos >= s0 && pos + 16u <= s0 + R.len) return R.seq + (pos - s0);
    const uint64_t q0 = s0 + R.len + 3u;
    if (fastq && pos >= q0 && pos + 16u <= q0 + R.len) return R.qual + (pos - q0);
    return nullptr;
}
// the first fragment in [lo, hi) whose record ends behind byte o of the output (there is one: o < ends[hi - 1])
TGSF_D uint64_t textout_find(const uint64_t* __restrict__ ends, uint64_t lo, uint64_t hi, uint64_t o)
{
    while (lo + 1 < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ends[mid - 1] > o) hi = mid; else lo = mid;
    }
    return lo;
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_textout_copy(const uint8_t* __restrict__ text, tgsf_text_index_arrays I,
                                                        const tgsf_fragment* __restrict__ frags, const TextOutMeta* __restrict__ meta,
                                                        const uint64_t* __restrict__ ends, uint64_t n_frags, int fastq,
                                                        const TextOutState* S, uint64_t capacity, uint8_t* __restrict__ out)
{
    const uint64_t total = S->n_bytes;
    if (total > capacity) return;                                      // TGSF_TEXT_CAPACITY: nothing is written
    const uint64_t n_pieces = (total + kTextPiece - 1) / kTextPiece;
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    constexpr uint32_t per = kTextPieceChunks / kTextLanes;            // chunks a lane takes: 4 (emulation: all 256)
    for (uint64_t piece = wave_uniform64(text_wave()); piece < n_pieces; piece += n_waves) {
        const uint64_t p0 = piece * kTextPiece;
        const uint64_t f0 = textout_find(ends, 0, n_frags, p0);        // wave-uniform: the first record that touches the piece
        const TextOutRec R0 = textout_rec(f0, ends, frags, meta, I, text);
        const uint8_t* src[per];
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {
            const uint64_t o = p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u;
            src[j] = nullptr;
            if (o + 16u > total) continue;                             // behind the output, or its last partial chunk
            if (o + 16u <= R0.end) src[j] = textout_plain(R0, o - R0.begin, fastq);
            else if (o >= R0.end) {
                const TextOutRec R = textout_rec(textout_find(ends, f0 + 1, n_frags, o), ends, frags, meta, I, text);
                if (o + 16u <= R.end) src[j] = textout_plain(R, o - R.begin, fastq);
            }
        }
        uint4 v[per];
#pragma unroll
        for (uint32_t j = 0; j < per; j++)                             // every load under way before the first store
            if (src[j]) v[j] = load16u(src[j]);
#pragma unroll
        for (uint32_t j = 0; j < per; j++)
            if (src[j]) *reinterpret_cast<uint4*>(out + p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u) = v[j];
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {                           // the seam chunks, byte by byte
            const uint64_t o = p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u;
            if (src[j] || o >= total) continue;
            const uint32_t nb = total - o < 16u ? (uint32_t)(total - o) : 16u;
            uint64_t f = textout_find(ends, f0, n_frags, o);
            TextOutRec R = textout_rec(f, ends, frags, meta, I, text);
            uint64_t lo = 0, hi = 0;
            for (uint32_t i = 0; i < nb; i++) {
                while (o + i >= R.end) R = textout_rec(++f, ends, frags, meta, I, text);   // (o + i < total = ends[n_frags - 1])
                const uint64_t b = out_byte(R, o + i - R.begin, fastq);
                if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u));
            }
            if (nb == 16u) {
                uint4 w;
                w.x = (uint32_t)lo; w.y = (uint32_t)(lo >> 32); w.z = (uint32_t)hi; w.w = (uint32_t)(hi >> 32);
                *reinterpret_cast<uint4*>(out + o) = w;
            } else
                for (uint32_t i = 0; i < nb; i++) out[o + i] = (uint8_t)((i < 8 ? lo >> (8u * i) : hi >> (8u * (i - 8u))) & 0xFFu);
        }
    }
}

// ---- the BAM input side: inflated unaligned BAM records -> FASTQ text and its index (tgsf_text_bam_*) -----------------
//
//   k_bam_reset        one lane: the state
//   k_bam_heads        a lane per walked record: its fields by byte loads (record starts have no alignment), regular or not,
//                      name_len (strnlen), l_seq, where the packed bases begin, the size of its piece of text (0: not regular)
//   (k_text_scan_tiles<uint64_t> / k_textout_scan_top: exclusive prefix sums of the sizes)
//   k_bam_layout       a lane per walked record: the byte behind its text (ends[]), its index words, the first one that ends
//                      behind max_bytes
//   (k_text_fold<BamState>: bases and longest over the prefix that is indexed)
//   k_bam_finish       one lane: the summary
//   k_bam_unpack       the hot path, driven by the OUTPUT as k_textout_copy is: waves stride over 4 KiB pieces of the text, a
//                      lane owns aligned 16-byte chunks.  A chunk inside a base stretch is 8 packed bytes (9 when it starts on
//                      an odd base) through the 16-entry table, held in four registers and read with v_perm_b32; a chunk
//                      inside a quality stretch is 16 bytes plus 33; a chunk on a seam is put together byte by byte by
//                      bam_text_byte(), the only place that knows the layout.  It also writes the zero pad and bad_qual.
struct BamState {
    uint64_t total;        // sum of the sizes of the walked records
    uint64_t bases;
    uint32_t first_bad;    // first walked record that is not regular (0xFFFFFFFF: none)
    uint32_t first_over;   // first walked record whose text ends behind max_bytes (0xFFFFFFFF: none)
    uint32_t longest;
    uint32_t reserved;
};

TGSF_HD uint32_t bam_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
TGSF_HD uint32_t bam_le32(const uint8_t* p) { return bam_le16(p) | bam_le16(p + 2) << 16; }
// records of the index: the walked ones in front of the first that is not regular and the first that does not fit
TGSF_D uint32_t index_records(const BamState* S, uint32_t n_walked, uint32_t = 0)
{
    const uint32_t k = S->first_bad < S->first_over ? S->first_bad : S->first_over;
    return k < n_walked ? k : n_walked;
}

TGSF_KERNEL k_bam_reset(BamState* S)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    S->total = 0; S->bases = 0; S->first_bad = 0xFFFFFFFFu; S->first_over = 0xFFFFFFFFu; S->longest = 0; S->reserved = 0;
}

// rec_off[i]: the record's block_size field; the walk has seen that block_size >= 32 and that the record is complete
TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_bam_heads(const uint8_t* __restrict__ bam, const uint64_t* __restrict__ rec_off, uint32_t n_walked,
                                                     uint64_t* __restrict__ size, uint32_t* __restrict__ oseq, tgsf_text_index_arrays I,
                                                     BamState* S)
{
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t i = gid; i < n_walked; i += stride) {
        const uint8_t* r = bam + rec_off[i];
        const uint32_t block = bam_le32(r);
        r += 4;
        const uint32_t l_read_name = r[8], n_cigar = bam_le16(r + 12), l_seq = bam_le32(r + 16);
        const uint32_t o_seq = 32u + l_read_name + 4u * n_cigar;
        const uint64_t o_qual = (uint64_t)o_seq + ((uint64_t)l_seq + 1u) / 2u;
        const bool ok = block >= 32u && o_qual + l_seq <= block && l_seq > 0;
        uint32_t nl = 0;
        if (ok) while (nl < l_read_name && r[32u + nl]) nl++;       // (the name field lies within the record: o_seq <= block)
        size[i] = ok ? (uint64_t)nl + 2ull * l_seq + 6u : 0u;
        oseq[i] = o_seq;
        I.name_len[i] = nl;
        I.len[i] = l_seq;
        if (!ok && (uint32_t)i < bad) bad = (uint32_t)i;
    }
    wave_min_into(&S->first_bad, bad);
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_bam_layout(const uint64_t* __restrict__ size_excl, const uint64_t* __restrict__ size_part,
                                                      uint32_t n_walked, uint64_t max_bytes, BamState* S, uint64_t* __restrict__ ends,
                                                      tgsf_text_index_arrays I)
{
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = gridDim.x * (uint64_t)blockDim.x;
    const uint64_t total = S->total;
    uint32_t over = 0xFFFFFFFFu;
    for (uint64_t i = gid; i < n_walked; i += stride) {
        const uint64_t begin = size_part[i / kTextScanTile] + size_excl[i];
        const uint64_t end = i + 1 == n_walked ? total : size_part[(i + 1) / kTextScanTile] + size_excl[i + 1];
        ends[i] = end;
        const uint64_t seq = begin + 2u + I.name_len[i];
        I.name_off[i] = begin + 1u;
        I.seq_off[i] = seq;
        I.qual_off[i] = seq + I.len[i] + 3u;
        if (end > max_bytes && (uint32_t)i < over) over = (uint32_t)i;
    }
    wave_min_into(&S->first_over, over);
}

TGSF_KERNEL k_bam_finish(const uint64_t* rec_off, const uint64_t* ends, uint32_t n_walked, uint32_t walk_stop, const BamState* S,
                         tgsf_text_bam_summary* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t k = index_records(S, n_walked);
    out->n_records = k;
    out->stop = k == n_walked ? walk_stop : (S->first_bad == k ? (uint32_t)TGSF_TEXT_IRREGULAR : (uint32_t)TGSF_TEXT_CAPACITY);
    out->consumed = rec_off[k];                                        // (n_walked + 1 entries)
    out->text_bytes = k ? ends[k - 1] : 0;
    out->bases = S->bases;
    out->longest = S->longest;
    out->bad_qual = 0xFFFFFFFFu;                                       // (k_bam_unpack folds into it)
    out->device_ms = 0.0f;
    out->reserved = 0;
}

// The chain walk of tgsf_text_bam_walk on BAM bytes that are in HBM (behind a device inflate), by one lane: a dependent load per
// record.  The walk covers bam[start .. n_bytes); offsets count from bam.  head: n, stop, consumed; rec_off follows it in one
// allocation, so that one copy brings everything down.
struct BamWalkHead { uint32_t n, stop; uint64_t consumed; };
TGSF_KERNEL k_bam_walk(const uint8_t* bam, uint64_t start, uint64_t n_bytes, int final, uint32_t max_records, BamWalkHead* head,
                       uint64_t* rec_off)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t at = start;
    uint32_t k = 0, why = TGSF_TEXT_END;
    for (;;) {
        rec_off[k] = at;
        if (at == n_bytes) break;                                      // nothing is left
        if (k == max_records) { why = TGSF_TEXT_CAPACITY; break; }
        if (n_bytes - at < 4) { why = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        const uint32_t block = bam_le32(bam + at);
        if (block < 32u) { why = TGSF_TEXT_IRREGULAR; break; }
        if (n_bytes - at - 4 < block) { why = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        at += 4ull + block;
        k++;
    }
    head->n = k;
    head->stop = why;
    head->consumed = at;
}

// one record, as the unpack needs it
struct BamRec {
    uint64_t begin, end;               // bytes of the text
    const uint8_t *name, *seq, *qual;  // in the BAM bytes
    uint32_t name_len, len;
};
TGSF_D BamRec bam_rec(uint64_t i, const uint64_t* __restrict__ ends, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ oseq,
                      const tgsf_text_index_arrays& I, const uint8_t* __restrict__ bam)
{
    BamRec R;
    R.begin = i ? ends[i - 1] : 0;
    R.end = ends[i];
    const uint8_t* r = bam + rec_off[i] + 4u;
    R.name_len = I.name_len[i];
    R.len = I.len[i];
    R.name = r + 32u;
    R.seq = r + oseq[i];
    R.qual = R.seq + ((uint64_t)R.len + 1u) / 2u;
    return R;
}
// the host's kBase (host/bam.cpp; the reference's table, src/TGSFilter.cpp:31): of the codes of "=ACMGRSVTWYHKDBN" only A, C, G, T
// and N have a letter, the others decode to NUL.  Four bytes a word.
constexpr uint32_t kNt16a = 0x00434100u, kNt16b = 0x00000047u, kNt16c = 0x00000054u, kNt16d = 0x4E000000u;
TGSF_HD uint8_t bam_base(uint32_t code)
{
    const uint32_t w = code < 8u ? (code < 4u ? kNt16a : kNt16b) : (code < 12u ? kNt16c : kNt16d);
    return (uint8_t)(w >> (8u * (code & 3u)));
}
// THE LAYOUT: byte `pos` of the record's text.  '@', the name, '\n', the bases, "\n+\n", the qualities plus 33, '\n'.
// *qual: the byte is a quality.
TGSF_D uint8_t bam_text_byte(const BamRec& R, uint64_t pos, bool* qual)
{
    *qual = false;
    if (pos == 0) return '@';
    pos -= 1;
    if (pos < R.name_len) return R.name[pos];
    pos -= R.name_len;
    if (pos == 0) return '\n';
    pos -= 1;
    if (pos < R.len) { const uint32_t by = R.seq[pos >> 1]; return bam_base(pos & 1u ? by & 15u : by >> 4); }
    pos -= R.len;
    if (pos < 3) return pos == 1 ? '+' : '\n';
    pos -= 3;
    if (pos < R.len) { *qual = true; return (uint8_t)(R.qual[pos] + 33u); }
    return '\n';
}
// what kind of chunk the 16 bytes at `pos` of the record are: 1 bases from an even one on, 2 from an odd one on (*src: the first
// packed byte), 3 qualities (*src: the first of them), 0 a seam
TGSF_D uint32_t bam_plain(const BamRec& R, uint64_t pos, const uint8_t** src)
{
    const uint64_t s0 = 2u + (uint64_t)R.name_len;
    if (pos >= s0 && pos + 16u <= s0 + R.len) { *src = R.seq + ((pos - s0) >> 1); return 1u + (uint32_t)((pos - s0) & 1u); }
    const uint64_t q0 = s0 + R.len + 3u;
    if (pos >= q0 && pos + 16u <= q0 + R.len) { *src = R.qual + (pos - q0); return 3u; }
    return 0u;
}
// two packed bytes (the low 16 bits of w) -> their four bases
TGSF_D uint32_t bam_bases4(uint32_t w)
{
    const uint32_t u = (w & 0xFFu) | (w & 0xFF00u) << 8;                          // bytes p0, 0, p1, 0
    const uint32_t v = ((u >> 4) & 0x000F000Fu) | (u & 0x000F000Fu) << 8;         // codes: p0 >> 4, p0 & 15, p1 >> 4, p1 & 15
    const uint32_t sel = v & 0x07070707u, hi = ((v >> 3) & 0x01010101u) * 0xFFu;  // hi: 0xFF in the bytes with codes 8..15
    return (perm_bytes(kNt16b, kNt16a, sel) & ~hi) | (perm_bytes(kNt16d, kNt16c, sel) & hi);
}
// four bytes plus 33 each (no carry between them)
TGSF_HD uint32_t bam_plus33(uint32_t x) { return ((x & 0x7F7F7F7Fu) + 0x21212121u) ^ (x & 0x80808080u); }

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_bam_unpack(const uint8_t* __restrict__ bam, const uint64_t* __restrict__ rec_off,
                                                      const uint32_t* __restrict__ oseq, tgsf_text_index_arrays I,
                                                      const uint64_t* __restrict__ ends, tgsf_text_bam_summary* sum, uint8_t* __restrict__ text)
{
    const uint64_t nrec = sum->n_records, total = sum->text_bytes, padded = total + TGSF_TEXT_PAD;   // (k_bam_finish wrote them)
    const uint64_t n_pieces = (padded + kTextPiece - 1) / kTextPiece;
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    constexpr uint32_t per = kTextPieceChunks / kTextLanes;            // chunks a lane takes: 4 (emulation: all 256)
    uint32_t bad = 0xFFFFFFFFu;                                        // the lowest record with a quality that decodes to '\n'
    for (uint64_t piece = wave_uniform64(text_wave()); piece < n_pieces; piece += n_waves) {
        const uint64_t p0 = piece * kTextPiece;
        const bool in_text = p0 < total;                               // wave-uniform: else the piece is pad only
        const uint64_t f0 = in_text ? textout_find(ends, 0, nrec, p0) : 0;   // the first record that touches the piece
        BamRec R0 = {0, 0, nullptr, nullptr, nullptr, 0, 0};
        if (in_text) R0 = bam_rec(f0, ends, rec_off, oseq, I, bam);
        const uint8_t* src[per];
        uint32_t kind[per];
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {
            const uint64_t o = p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u;
            kind[j] = 0; src[j] = nullptr;
            if (o + 16u > total) continue;                             // behind the text, or its last partial chunk
            if (o + 16u <= R0.end) kind[j] = bam_plain(R0, o - R0.begin, &src[j]);
            else if (o >= R0.end) {
                const BamRec R = bam_rec(textout_find(ends, f0 + 1, nrec, o), ends, rec_off, oseq, I, bam);
                if (o + 16u <= R.end) kind[j] = bam_plain(R, o - R.begin, &src[j]);
            }
        }
        uint4 v[per];
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {                           // every load under way before the first store
            if (kind[j] == 3u) v[j] = load16u(src[j]);
            else if (kind[j]) {
                const uint64_t p = load8u(src[j]);
                v[j].x = (uint32_t)p; v[j].y = (uint32_t)(p >> 32);
                v[j].z = kind[j] == 2u ? src[j][8] : 0u;
                v[j].w = 0;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {
            if (!kind[j]) continue;
            uint4 w;
            if (kind[j] == 3u) {
                w.x = bam_plus33(v[j].x); w.y = bam_plus33(v[j].y); w.z = bam_plus33(v[j].z); w.w = bam_plus33(v[j].w);
                if (newline_bits4(w.x) | newline_bits4(w.y) | newline_bits4(w.z) | newline_bits4(w.w)) {     // (rare: the record is looked up again)
                    const uint32_t f = (uint32_t)textout_find(ends, f0, nrec, p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u);
                    if (f < bad) bad = f;
                }
            } else {
                uint64_t p = (uint64_t)v[j].y << 32 | v[j].x;
                if (kind[j] == 2u)                                     // from the low nibble of the first byte on: a nibble down
                    p = (p & 0x0F0F0F0F0F0F0F0Full) << 4 | (((p >> 8 | (uint64_t)v[j].z << 56) >> 4) & 0x0F0F0F0F0F0F0F0Full);
                w.x = bam_bases4((uint32_t)p); w.y = bam_bases4((uint32_t)(p >> 16));
                w.z = bam_bases4((uint32_t)(p >> 32)); w.w = bam_bases4((uint32_t)(p >> 48));
            }
            *reinterpret_cast<uint4*>(text + p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u) = w;
        }
#pragma unroll
        for (uint32_t j = 0; j < per; j++) {                           // the seam chunks and the pad, byte by byte
            const uint64_t o = p0 + (uint64_t)(text_lane() + j * kTextLanes) * 16u;
            if (kind[j] || o >= padded) continue;
            const uint32_t nb = padded - o < 16u ? (uint32_t)(padded - o) : 16u;
            uint64_t lo = 0, hi = 0;
            if (o < total) {
                uint64_t f = textout_find(ends, f0, nrec, o);
                BamRec R = bam_rec(f, ends, rec_off, oseq, I, bam);
                for (uint32_t i = 0; i < nb && o + i < total; i++) {   // (behind the text: zeros)
                    while (o + i >= R.end) R = bam_rec(++f, ends, rec_off, oseq, I, bam);   // (o + i < total = ends[nrec - 1])
                    bool q;
                    const uint64_t b = bam_text_byte(R, o + i - R.begin, &q);
                    if (q && b == '\n' && (uint32_t)f < bad) bad = (uint32_t)f;
                    if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u));
                }
            }
            if (nb == 16u) {
                uint4 w;
                w.x = (uint32_t)lo; w.y = (uint32_t)(lo >> 32); w.z = (uint32_t)hi; w.w = (uint32_t)(hi >> 32);
                *reinterpret_cast<uint4*>(text + o) = w;
            } else
                for (uint32_t i = 0; i < nb; i++) text[o + i] = (uint8_t)((i < 8 ? lo >> (8u * i) : hi >> (8u * (i - 8u))) & 0xFFu);
        }
    }
    wave_min_into(&sum->bad_qual, bad);
}

// ---- the BGZF input side: compressed members -> their inflated bytes (tgsf_text_bgzf_*) -------------------------------
//
//   k_bgzf_inflate     a wave per member, the waves striding over the block table.  Everything that steers the decoder --
//                      the bit reader, the tables' lookups, the symbol loop -- is wave-uniform, and made scalar on the device by
//                      wave_first() on every value that is loaded (the loads themselves are vector loads at one address); the
//                      lanes work side by side where bytes move: literals are gathered one per lane and stored together,
//                      a match and a stored block are copied by all lanes, the Huffman tables (LDS, a set per wave) are
//                      built a code length per lane.  The window is the member's own output range in global memory.
//   k_bgzf_finish      one lane: the summary
//
// EVERY LOOP IS BOUNDED BY clen AND usize: an iteration of the symbol loop consumes at least one bit or ends the member, a
// block at least three, and a member ends as BAD as soon as a consumed bit lies behind 8 * clen or a byte behind usize.
struct BgzfState { uint32_t bad_block, bad_crc; };      // the lowest bad member; the lowest whose CRC32 differs, when asked (0xFFFFFFFF: none)

constexpr uint32_t kInfWaves = kTextThreads / 64;         // table sets of a workgroup: its waves (the emulation's lanes, waves of one
                                                          // that run one after the other, take turns on them)
constexpr uint32_t kInfLitFast = 9, kInfDistFast = 6, kInfLenFast = 7;   // bits of the first-level lookups
constexpr uint32_t kInfNone = 0xFFFFu;
// one Huffman code: lut[the next `fast` bits] = symbol << 4 | length for the codes of up to `fast` bits (0: a longer code, or
// none); for those, the canonical walk over count[] (codes per length) and sym[] (the symbols in the order of their codes)
struct InfTable { uint16_t lut[1u << kInfLitFast]; uint16_t sym[288]; uint16_t count[16]; };
struct InfWave { InfTable lit, dist; uint8_t lens[320]; };

// the order of the code-length code's lengths in a dynamic header, five bits each
constexpr uint64_t inf_order_word(int from, int n)
{
    const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t w = 0;
    for (int i = 0; i < n; i++) w |= (uint64_t)o[from + i] << (5 * i);
    return w;
}
constexpr uint64_t kInfOrderLo = inf_order_word(0, 12), kInfOrderHi = inf_order_word(12, 7);
TGSF_HD uint32_t inf_order(uint32_t i) { return (uint32_t)((i < 12u ? kInfOrderLo >> (5u * i) : kInfOrderHi >> (5u * (i - 12u))) & 31u); }

// The payload's bits, least significant first, by aligned dword loads (the chunk is 4-byte aligned and readable up to its end
// rounded up to 4: a member's dwords lie within it, its trailer follows the payload).  Dwords that begin at or behind the
// payload's end are not loaded: they read as zeros.  `used` counts the bits taken; the caller compares it with 8 * clen.
struct InfBits {
    const uint32_t* words;
    uint32_t a0, clen;       // bytes between words[0] and the payload's first byte; the payload's bytes
    uint32_t next;           // the next dword
    uint64_t buf;
    uint32_t n, used;        // bits in buf; bits taken since the payload's first
};
TGSF_D uint32_t inf_word(const InfBits& B, uint32_t w) { return 4u * w < B.a0 + B.clen ? wave_first(B.words[w]) : 0u; }
TGSF_D void inf_seek(InfBits& B, uint32_t bit)
{
    const uint32_t p = bit + 8u * B.a0;
    B.next = p / 32u;
    B.buf = inf_word(B, B.next) >> (p % 32u);
    B.n = 32u - p % 32u;
    B.next++;
    B.used = bit;
}
TGSF_D void inf_open(InfBits& B, const uint8_t* payload, uint32_t clen)
{
    B.a0 = (uint32_t)((uintptr_t)payload & 3u);
    B.words = reinterpret_cast<const uint32_t*>(payload - B.a0);
    B.clen = clen;
    inf_seek(B, 0);
}
// the next k <= 32 bits (at least 32 are in buf behind it)
TGSF_D uint32_t inf_peek(InfBits& B, uint32_t k)
{
    if (B.n < 32u) { B.buf |= (uint64_t)inf_word(B, B.next) << B.n; B.next++; B.n += 32u; }
    return (uint32_t)B.buf & (k >= 32u ? 0xFFFFFFFFu : (1u << k) - 1u);
}
TGSF_D void inf_drop(InfBits& B, uint32_t k) { B.buf >>= k; B.n -= k; B.used += k; }      // (k <= the bits peeked)
TGSF_D uint32_t inf_take(InfBits& B, uint32_t k) { const uint32_t v = inf_peek(B, k); inf_drop(B, k); return v; }

// Builds T from lens[0 .. n) (n <= 288, lengths 0..15), by the whole wave: the lookups zeroed by all lanes, then a code
// length per lane -- its count first, then its symbols in order, each with its canonical code.  Returns zlib's verdict on the
// set (inftrees.c): false when it is over-subscribed, or incomplete with a longest code of more than one bit (any_incomplete
// false: incomplete at all).  A set without any code is complete for this purpose; its lookups find nothing.
TGSF_D bool inf_build(InfTable& T, const uint8_t* lens, uint32_t n, uint32_t fast, bool any_incomplete)
{
    TGSF_WAVE_SYNC();                                                  // lens[] is written, the last lookups in T are over
    for (uint32_t i = TGSF_WCOOP_BEGIN(text_lane()); i < (1u << fast); i += TGSF_WCOOP_STRIDE) T.lut[i] = 0;
    for (uint32_t l = TGSF_WCOOP_BEGIN(text_lane()); l < 16u; l += TGSF_WCOOP_STRIDE) {
        uint32_t c = 0;
        for (uint32_t s = 0; s < n; s++) c += lens[s] == l ? 1u : 0u;
        T.count[l] = (uint16_t)c;
    }
    TGSF_WAVE_SYNC();
    int32_t left = 1;                                                  // (uniform: every lane reads the same counts)
    uint32_t longest = 0;
    for (uint32_t l = 1; l < 16u; l++) {
        const uint32_t c = wave_first(T.count[l]);
        left = 2 * left - (int32_t)c;
        if (left < 0) return false;                                    // over-subscribed
        if (c) longest = l;
    }
    if (left > 0 && longest != 0 && (!any_incomplete || longest != 1u)) return false;
    for (uint32_t l = TGSF_WCOOP_BEGIN(text_lane()); l < 16u; l += TGSF_WCOOP_STRIDE) {
        if (l == 0) continue;
        uint32_t at = 0, code = 0;                                     // where this length's symbols begin in sym[]; its first code
        for (uint32_t k = 1; k < l; k++) { at += T.count[k]; code = (code + T.count[k]) << 1; }
        for (uint32_t s = 0; s < n; s++) {
            if (lens[s] != l) continue;
            T.sym[at++] = (uint16_t)s;
            if (l <= fast) {
                uint32_t rev = 0;                                      // the stream has a code's first bit lowest
                for (uint32_t k = 0; k < l; k++) rev = rev << 1 | ((code >> k) & 1u);
                for (uint32_t i = rev; i < (1u << fast); i += 1u << l) T.lut[i] = (uint16_t)(s << 4 | l);
            }
            code++;
        }
    }
    TGSF_WAVE_SYNC();
    return true;
}
// the symbol whose code begins the 15 bits `peek`, and its length; kInfNone: no code of the set does
TGSF_D uint32_t inf_symbol(const InfTable& T, uint32_t fast, uint32_t peek, uint32_t* len)
{
    const uint32_t e = wave_first(T.lut[peek & ((1u << fast) - 1u)]);
    if (e) { *len = e & 15u; return e >> 4; }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16u; l++) {
        code |= (peek >> (l - 1u)) & 1u;
        const uint32_t c = wave_first(T.count[l]);
        if (code < first + c) { *len = l; return wave_first(T.sym[index + (code - first)]); }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    *len = 0;
    return kInfNone;
}

// One member: payload[0 .. clen) inflated to dst[0 .. usize); whether it is GOOD.  Wave-uniform but for the copies.
TGSF_D bool inf_member(const uint8_t* __restrict__ payload, uint32_t clen, uint32_t usize, uint8_t* dst, InfWave& W)
{
    if (usize == 0 && clen <= 2u) return true;                         // the EOF member
    const uint32_t lane = text_lane(), limit = 8u * clen;
    InfBits B;
    inf_open(B, payload, clen);
    uint32_t pos = 0;                                                  // bytes produced
    uint32_t clean = 0;                                                // dst[0 .. clean) has been fenced: any lane may load it
    for (;;) {
        const uint32_t head = inf_take(B, 3);
        if (B.used > limit) return false;
        const uint32_t type = head >> 1;
        if (type == 3u) return false;
        if (type == 0u) {                                              // stored: to the byte boundary, LEN, NLEN, the bytes
            inf_drop(B, (8u - (B.used & 7u)) & 7u);
            const uint32_t v = inf_take(B, 32);
            if (B.used > limit) return false;
            const uint32_t len = v & 0xFFFFu;
            if ((v >> 16) != (len ^ 0xFFFFu) || len > usize - pos || 8u * len > limit - B.used) return false;
            const uint8_t* src = payload + B.used / 8u;
            for (uint32_t i = lane; i < len; i += kTextLanes) dst[pos + i] = src[i];
            pos += len;
            inf_seek(B, B.used + 8u * len);
        } else {
            uint32_t nlen = 288, ndist = 32;
            if (type == 1u) {                                          // the fixed code, built as any other
                for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < 320u; s += TGSF_WCOOP_STRIDE)
                    W.lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < 288u ? 8u : 5u);
            } else {
                const uint32_t h = inf_take(B, 14);
                if (B.used > limit) return false;
                nlen = 257u + (h & 31u); ndist = 1u + ((h >> 5) & 31u);
                const uint32_t ncode = 4u + (h >> 10);
                if (nlen > 286u || ndist > 30u) return false;
                for (uint32_t i = 0; i < 19u; i++) W.lens[inf_order(i)] = (uint8_t)(i < ncode ? inf_take(B, 3) : 0u);   // (every lane the same byte)
                if (B.used > limit) return false;
                if (!inf_build(W.lit, W.lens, 19, kInfLenFast, false)) return false;
                bool none = true;
                for (uint32_t l = 1; l < 16u; l++) none = none && wave_first(W.lit.count[l]) == 0;
                if (none) return false;                                // (zlib reads on, a bit a length, and finds no symbol 256)
                const uint32_t total = nlen + ndist;
                for (uint32_t have = 0; have < total;) {
                    uint32_t l;
                    const uint32_t s = inf_symbol(W.lit, kInfLenFast, inf_peek(B, 15), &l);
                    if (s == kInfNone) return false;
                    inf_drop(B, l);
                    uint32_t rep = 1, val = s;
                    if (s == 16u) {
                        if (have == 0) return false;
                        val = wave_first(W.lens[have - 1u]);
                        rep = 3u + inf_take(B, 2);
                    } else if (s == 17u) { val = 0; rep = 3u + inf_take(B, 3); }
                    else if (s == 18u) { val = 0; rep = 11u + inf_take(B, 7); }
                    if (B.used > limit || have + rep > total) return false;
                    for (uint32_t i = 0; i < rep; i++) W.lens[have + i] = (uint8_t)val;
                    have += rep;
                }
                if (wave_first(W.lens[256]) == 0) return false;                    // no code for the end of the block
            }
            if (!inf_build(W.lit, W.lens, nlen, kInfLitFast, true)) return false;
            if (!inf_build(W.dist, W.lens + nlen, ndist, kInfDistFast, true)) return false;
            uint32_t nlit = 0, mine = 0;                               // literals gathered, lane k holds the k-th
            for (;;) {
                uint32_t l;
                const uint32_t s = inf_symbol(W.lit, kInfLitFast, inf_peek(B, 15), &l);
                if (s == kInfNone) return false;
                inf_drop(B, l);
                if (B.used > limit) return false;
                if (s < 256u) {
                    if (pos + nlit >= usize) return false;
                    if (lane == nlit) mine = s;
                    if (++nlit < kTextLanes) continue;
                }
                if (lane < nlit) dst[pos + lane] = (uint8_t)mine;      // before anything but a literal, and when every lane has one
                pos += nlit;
                nlit = 0;
                if (s < 256u) continue;
                if (s == 256u) break;
                if (s >= 286u) return false;
                uint32_t len = s - 254u;                               // 257..264: 3..10
                if (s == 285u) len = 258;
                else if (s >= 265u) { const uint32_t k = s - 261u, x = k >> 2; len = 3u + ((4u + (k & 3u)) << x) + inf_take(B, x); }
                const uint32_t ds = inf_symbol(W.dist, kInfDistFast, inf_peek(B, 15), &l);
                if (ds == kInfNone || ds >= 30u) return false;
                inf_drop(B, l);
                uint32_t dist = ds + 1u;
                if (ds >= 4u) { const uint32_t x = (ds >> 1) - 1u; dist = 1u + ((2u + (ds & 1u)) << x) + inf_take(B, x); }
                if (B.used > limit || dist > pos || len > usize - pos) return false;
                // byte i of the match is byte i % dist of the dist bytes in front of it: all stored before this match, whether it
                // overlaps itself (dist < len) or not, so the lanes need no order among themselves; but other lanes stored them
                if (pos - dist + (len < dist ? len : dist) > clean) { TGSF_WG_FENCE(); clean = pos; }
                const uint8_t* from = dst + (pos - dist);
                if (dist >= len) for (uint32_t i = lane; i < len; i += kTextLanes) dst[pos + i] = from[i];
                else for (uint32_t i = lane; i < len; i += kTextLanes) dst[pos + i] = from[i % dist];
                pos += len;
            }
        }
        if (head & 1u) return pos == usize;
    }
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_bgzf_inflate(const uint8_t* __restrict__ gz, const tgsf_text_bgzf_block* __restrict__ blocks,
                                                        uint32_t n_blocks, uint8_t* out, BgzfState* S)
{
    TGSF_SHARED InfWave sets[kInfWaves];
    InfWave& W = sets[(threadIdx.x / kTextLanes) % kInfWaves];
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t b = wave_uniform64(text_wave()); b < n_blocks; b += n_waves) {
        const uint64_t payload = wave_uniform64(blocks[b].payload), at = wave_uniform64(blocks[b].out);
        const uint32_t clen = (uint32_t)wave_uniform64(blocks[b].clen), usize = (uint32_t)wave_uniform64(blocks[b].usize);
        if (!inf_member(gz + payload, clen, usize, out + at, W) && (uint32_t)b < bad) bad = (uint32_t)b;
    }
    wave_min_into(&S->bad_block, bad);
}

TGSF_KERNEL k_bgzf_finish(uint32_t n_blocks, uint32_t walk_stop, uint64_t consumed, uint64_t out_bytes, const BgzfState* S,
                          tgsf_text_bgzf_summary* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out->n_blocks = n_blocks;
    out->stop = walk_stop;
    out->consumed = consumed;
    out->out_bytes = out_bytes;
    out->bad_block = S->bad_block;
    out->device_ms = 0.0f;
    out->reserved = 0;
}

// ---- the BGZF output side: text -> compressed members, and the CRC32 both ends need (tgsf_text_bgzf_deflate*, _crc_device) ------
//
//   k_gz_count         a wave per member of TGSF_TEXT_BGZF_MEMBER input bytes, the waves striding over the members.  One read of
//                      the member, a contiguous slice per lane: the histogram (LDS, a set per wave) and the slice's CRC32, the
//                      slices' CRCs combined by multiplication by x^(8 * bytes behind the slice) mod P.  Then the prefix code:
//                      the symbols ranked by frequency (a symbol per lane), the Huffman depths by the in-place method of Moffat
//                      and Katajainen (one lane: 3 passes over at most 257 words), depths over 15 clamped and the Kraft sum
//                      repaired as zlib's gen_bitlen does (a leaf one level down, a 15-bit leaf beside it, until the code is
//                      complete), canonical codes (a symbol per lane).  Per member to scratch: code | length << 16 of every
//                      symbol, the CRC, stored or not; its size in bytes, framing included, to the table that is scanned.
//   (k_text_scan_tiles<uint64_t> / k_textout_scan_top: exclusive prefix sums of the sizes -- a member's place in the output)
//   k_gz_emit          a wave per member, straight to its final place: the 18 bytes of header, the block, CRC32 and ISIZE.  A
//                      dynamic block goes through a staging area in LDS, 16 input bytes a lane and round (one aligned load, the
//                      loads of a wave side by side): a lane's codes are put together in registers, its bit offset is the wave's
//                      prefix sum of code lengths, the words it shares with its neighbours are or-ed in LDS; whole dwords then
//                      leave for the output, the bits left over open the next round.  Decides CAPACITY (nothing is written),
//                      writes the EOF member, the summary and member_end.
//   k_bgzf_crc         a wave per member of a block table: CRC32 of its inflated bytes against its trailer
//
// EVERY LOOP IS BOUNDED BY THE MEMBER'S SIZE OR BY THE ALPHABET'S: no input byte steers a loop count.
constexpr uint32_t kGzMember = TGSF_TEXT_BGZF_MEMBER;
constexpr uint32_t kGzSyms = 257;                          // the literals and the end of the block: no length symbol occurs
constexpr uint32_t kGzSymRoom = 260;
constexpr uint32_t kGzFrame = 26;                          // header 18, CRC32, ISIZE
constexpr uint32_t kGzEofBytes = 28;
// a dynamic block's header: BFINAL, BTYPE, HLIT = 257, HDIST = 2, HCLEN = 19; the code-length code (three bits each: four-bit
// codes for 0..15, none for 16, 17, 18: constant and complete); 257 + 2 code lengths of four bits
constexpr uint32_t kGzFixedHeadBits = 17 + 19 * 3;
constexpr uint32_t kGzHeadBits = kGzFixedHeadBits + 4 * (kGzSyms + 2);
constexpr uint32_t kGzRound = 16 * kTextLanes;             // input bytes of a round of k_gz_emit
// Level 1 (tgsf_text_bgzf_out_level), the match search: rounds of kLzRound positions, a position a lane.  A round looks its
// positions up in a table of the latest position of every hash of four bytes (LDS, uint16 position + 1, two to a word), then
// inserts them: what a position finds depends on the rounds before its own alone, never on the order of the lanes.
constexpr uint32_t kLzRound = 64;
constexpr uint32_t kLzHashBits = 13;
constexpr uint32_t kLzSlots = 1u << kLzHashBits;
constexpr uint32_t kLzMaxLen = 258, kLzMaxDist = 32768;
constexpr uint32_t kLzLitSyms = 286, kLzDistSyms = 30, kLzLitRoom = 288; // (the distance counts and lengths follow the literal/length ones at kLzLitRoom)
constexpr uint32_t kLzSymRoom = kLzLitRoom + 32;
constexpr uint32_t kLzTokenBits = 15 + 5 + 15 + 13;                  // a match at its longest: two codes and their extra bits
// its block's header: HLIT = 286, HDIST = 30, the same code-length code; 286 + 30 code lengths of four bits
constexpr uint32_t kLzHeadBits = kGzFixedHeadBits + 4 * (kLzLitSyms + kLzDistSyms);
constexpr uint32_t kLzThreads = 128;                                   // lanes of a workgroup of the level-1 kernels: two waves, two tables
constexpr uint32_t kLzWaves = kLzThreads / 64;
static_assert(kLzRound == 64, "a round's positions are the bits of one 64-bit mask; on the device a position a lane");
// the staging area: the bits left over (31 at most), a round's (level 0: 15 a byte at most; level 1: a token a position at most),
// and the word a put may reach into
constexpr uint32_t kGzRoundBits = 15 * kGzRound > kLzTokenBits * kLzRound ? 15 * kGzRound : kLzTokenBits * kLzRound;
constexpr uint32_t kGzStageWords = (31 + kGzRoundBits + 31) / 32 + 2 > 44 ? (31 + kGzRoundBits + 31) / 32 + 2 : 44;
static_assert(kGzStageWords * 32 >= kGzHeadBits + 64 && kGzStageWords * 32 >= kLzHeadBits + 64, "the staging area holds either block's header");
static_assert(kGzStageWords * 32 >= 31 + 15 * kGzRound + 32 && kGzStageWords * 32 >= 31 + kLzTokenBits * kLzRound + 32, "the staging area holds the bits left over and a round's");
static_assert(kGzMember % 16 == 0 && kGzMember + 5 + kGzFrame <= 65536, "members begin on 16 bytes of the input; BSIZE - 1 is 16 bits");

struct GzState { uint64_t total; uint32_t stored, reserved; };        // bytes of all members but the EOF member; stored members
struct GzMeta { uint32_t crc, stored; uint32_t lut[kGzSyms]; uint32_t reserved; };   // lut[s]: the code, its first bit lowest | length << 16
struct GzCrcTables { uint32_t t[4][256]; };                // t[k][b]: the register after byte b and k zero bytes (slicing by 4)
struct GzCountWave { uint32_t hist[kGzSymRoom], freq[kGzSymRoom]; uint16_t order[kGzSymRoom]; uint8_t lens[kGzSymRoom]; uint32_t cnt[16]; };
struct GzEmitWave { uint32_t lut[kGzSymRoom]; uint32_t stage[kGzStageWords]; };
// level 1, per member (1280 bytes): lz, whether the block of matches is the smallest of the three; its two codes as in GzMeta::lut
struct GzLzMeta { uint32_t lz; uint32_t llut[kLzLitSyms]; uint32_t dlut[kLzDistSyms]; uint32_t reserved[3]; };
static_assert(sizeof(GzLzMeta) == 1280, "include/tgsf_text.h states the scratch of a member at level 1");
// level 1, per wave: the table; a round's matches (length | (distance - 1) << 9, 0: none) and the positions that have one; sym[]:
// counts in the first pass, codes in the second; the first pass's code builder; the second pass's lengths of the level-0 code
struct GzLzWave {
    uint32_t table[kLzSlots / 2];
    uint32_t rm[kLzRound], mask[2];
    uint32_t sym[kLzSymRoom];
    uint32_t freq[kLzLitRoom], cnt[2][16];
    uint16_t order[kLzLitRoom];
    uint8_t lens[kLzSymRoom], lens0[256];
};

#if !defined(TGSF_EMUL)
TGSF_D uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
#else
TGSF_HD uint32_t wave_xor(uint32_t v) { return v; }
#endif

constexpr uint32_t kCrcPoly = 0xEDB88320u;                 // IEEE, reflected: bit 31 is x^0
// crc_tab[256 * k + b] -> LDS, by the workgroup (the host computed it: tgsf_text.hip)
TGSF_D void gz_crc_tables(GzCrcTables& T, const uint32_t* __restrict__ crc_tab)
{
    for (uint32_t i = TGSF_COOP_BEGIN; i < 1024u; i += TGSF_COOP_STRIDE) T.t[i >> 8][i & 255u] = crc_tab[i];
    TGSF_BLOCK_SYNC();
}
TGSF_D uint32_t gz_crc_byte(const GzCrcTables& T, uint32_t c, uint32_t b) { return (c >> 8) ^ T.t[0][(c ^ b) & 255u]; }
TGSF_D uint32_t gz_crc_word(const GzCrcTables& T, uint32_t c, uint32_t w)      // four bytes, the first lowest
{
    c ^= w;
    return T.t[3][c & 255u] ^ T.t[2][(c >> 8) & 255u] ^ T.t[1][(c >> 16) & 255u] ^ T.t[0][c >> 24];
}
// a * b mod P
TGSF_HD uint32_t gz_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32u; i++) {
        p ^= b & (0u - ((a >> (31u - i)) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P, n < 2^17
TGSF_HD uint32_t gz_xpow8(uint32_t n)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;            // 1; x^8
    for (uint32_t i = 0; i < 17u; i++, n >>= 1) {
        if (n & 1u) p = gz_mulmod(sq, p);
        sq = gz_mulmod(sq, sq);
    }
    return p;
}
// zlib.crc32 of p[0 .. len) by one lane, at any alignment: bytes up to the first 16-byte boundary, aligned chunks, bytes; with
// Hist every byte is counted in hist[] (LDS)
template <bool Hist>
TGSF_D uint32_t gz_crc_slice(const GzCrcTables& T, const uint8_t* __restrict__ p, uint32_t len, uint32_t* hist)
{
    uint32_t c = 0xFFFFFFFFu, i = 0;
    uint32_t head = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u;
    if (head > len) head = len;
    for (; i < head; i++) { const uint32_t b = p[i]; c = gz_crc_byte(T, c, b); if (Hist) atomicAdd(&hist[b], 1u); }
    for (; i + 16u <= len; i += 16u) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            c = gz_crc_word(T, c, w[k]);
            if (Hist) { atomicAdd(&hist[w[k] & 255u], 1u); atomicAdd(&hist[(w[k] >> 8) & 255u], 1u); atomicAdd(&hist[(w[k] >> 16) & 255u], 1u); atomicAdd(&hist[w[k] >> 24], 1u); }
        }
    }
    for (; i < len; i++) { const uint32_t b = p[i]; c = gz_crc_byte(T, c, b); if (Hist) atomicAdd(&hist[b], 1u); }
    return ~c;
}
// ... of p[0 .. n) by the wave, n <= 65536: a slice of whole 16-byte chunks per lane; crc(A B) = crc(A) x^(8 |B|) + crc(B)
template <bool Hist>
TGSF_D uint32_t gz_crc_wave(const GzCrcTables& T, const uint8_t* __restrict__ p, uint32_t n, uint32_t* hist)
{
    const uint32_t per = ((n + kTextLanes - 1u) / kTextLanes + 15u) & ~15u;
    uint32_t lo = text_lane() * per, hi = lo + per;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
    const uint32_t c = gz_crc_slice<Hist>(T, p + lo, hi - lo, hist);
    return wave_xor(hi > lo ? gz_mulmod(c, gz_xpow8(n - hi)) : 0u);
}

// freq[0 .. n), ascending, n >= 2 -> the depth of each in a Huffman tree, in place (Moffat and Katajainen 1995); one lane
TGSF_D void gz_depths(uint32_t* A, uint32_t n)
{
    A[0] += A[1];
    uint32_t root = 0, leaf = 2;
    for (uint32_t next = 1; next + 1 < n; next++) {                    // parents: A[k] of an internal node is its parent's index
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (uint32_t next = n - 2; next-- > 0;) A[next] = A[A[next]] + 1u;  // depths of the internal nodes
    uint32_t avbl = 1, used = 0, dpth = 0;
    int32_t r = (int32_t)n - 2, nx = (int32_t)n - 1;
    while (avbl > 0 && nx >= 0) {                                      // depths of the leaves, a level a turn: at most n turns
        while (r >= 0 && A[r] == dpth) { used++; r--; }
        while (avbl > used && nx >= 0) { A[nx--] = dpth; avbl--; }
        avbl = 2u * used; dpth++; used = 0;
    }
}

// The prefix code of an alphabet, by the wave: hist[0 .. nsyms) (counts below 2^23, nsyms <= 512) -> lens[s], the length of
// symbol s (0: it does not occur; zeroed by the caller), and cnt[l], the codes of l bits -- at most 15 bits, complete.  freq
// and order are nsyms words of room.  With no or one symbol in use (a distance code can be): two codes of one bit, the
// complete set zlib asks for.
TGSF_D void gz_code_lengths(const uint32_t* hist, uint32_t nsyms, uint32_t* freq, uint16_t* order, uint8_t* lens, uint32_t* cnt)
{
    [[maybe_unused]] const uint32_t lane = text_lane();               // (the emulation's loops take every turn themselves)
    // the symbols that occur, by frequency (then by value): each finds its own rank
    uint32_t mine = 0;
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < nsyms; s += TGSF_WCOOP_STRIDE) {
        const uint32_t f = hist[s];
        if (!f) continue;
        const uint32_t key = f << 9 | s;                               // (f <= kGzMember < 2^16)
        uint32_t rank = 0;
        for (uint32_t t = 0; t < nsyms; t++) { const uint32_t ft = hist[t]; rank += ft && (ft << 9 | t) < key ? 1u : 0u; }
        freq[rank] = f;
        order[rank] = (uint16_t)s;
        mine++;
    }
    const uint32_t n_used = (uint32_t)wave_sum_i32((int32_t)mine);     // (the literal/length code: two at least, a token and the end of the block)
    TGSF_WAVE_SYNC();
    if (n_used < 2u) {
        if (wave_leader()) {
            const uint32_t s = n_used ? order[0] : 0u;
            lens[s] = 1; lens[s ? 0u : 1u] = 1;
            for (uint32_t l = 0; l < 16u; l++) cnt[l] = l == 1u ? 2u : 0u;
        }
        TGSF_WAVE_SYNC();
        return;
    }
    if (wave_leader()) gz_depths(freq, n_used);
    TGSF_WAVE_SYNC();
    for (uint32_t l = TGSF_WCOOP_BEGIN(lane); l < 16u; l += TGSF_WCOOP_STRIDE) {    // codes per length, depths over 15 clamped
        uint32_t c = 0;
        for (uint32_t i = 0; i < n_used; i++) { const uint32_t d = freq[i]; c += (d < 15u ? d : 15u) == l ? 1u : 0u; }
        cnt[l] = c;
    }
    TGSF_WAVE_SYNC();
    if (wave_leader()) {
        // The clamped set is over-subscribed by a whole number of 2^-15: every step takes one away.  There is a leaf above level
        // 15 as long as the sum exceeds 1 (n_used leaves of 15 bits sum to less), and a 15-bit leaf (the clamped ones: more of
        // them than steps).
        uint32_t kraft = 0;
        for (uint32_t l = 1; l < 16u; l++) kraft += cnt[l] << (15u - l);
        for (; kraft > 32768u; kraft--) {
            uint32_t b = 14;
            while (b > 1u && !cnt[b]) b--;
            cnt[b]--; cnt[b + 1u] += 2u; cnt[15]--;
        }
    }
    TGSF_WAVE_SYNC();
    for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < n_used; i += TGSF_WCOOP_STRIDE) {  // the rarest symbols get the longest codes
        uint32_t acc = 0, bits = 1;
        for (uint32_t l = 15; l >= 1u; l--) { acc += cnt[l]; if (i < acc) { bits = l; break; } }
        lens[order[i]] = (uint8_t)bits;
    }
    TGSF_WAVE_SYNC();
}
// the canonical code of symbol s, its first bit lowest | its length << 16 (0: the symbol has none)
TGSF_D uint32_t gz_code_entry(const uint8_t* lens, const uint32_t* cnt, uint32_t s)
{
    const uint32_t l = lens[s];
    if (!l) return 0;
    uint32_t code = 0, rev = 0;
    for (uint32_t k = 1; k < l; k++) code = (code + cnt[k]) << 1;
    for (uint32_t t = 0; t < s; t++) code += lens[t] == l ? 1u : 0u;
    for (uint32_t k = 0; k < l; k++) rev = rev << 1 | ((code >> k) & 1u);
    return rev | l << 16;
}

// one member: in[0 .. usize), 1 <= usize <= kGzMember, 16-byte aligned.  Returns its payload's bytes (wave-uniform).
TGSF_D uint32_t gz_count_member(const GzCrcTables& T, const uint8_t* __restrict__ in, uint32_t usize, GzCountWave& W, GzMeta* M)
{
    [[maybe_unused]] const uint32_t lane = text_lane();               // (the emulation's loops take every turn themselves)
    TGSF_WAVE_SYNC();                                                  // the last member's reads of W are over
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kGzSymRoom; s += TGSF_WCOOP_STRIDE) { W.hist[s] = s == 256u ? 1u : 0u; W.lens[s] = 0; }
    TGSF_WAVE_SYNC();
    const uint32_t crc = gz_crc_wave<true>(T, in, usize, W.hist);
    TGSF_WAVE_SYNC();
    gz_code_lengths(W.hist, kGzSyms, W.freq, W.order, W.lens, W.cnt);
    uint64_t bits = 0;
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kGzSyms; s += TGSF_WCOOP_STRIDE) {  // canonical codes
        const uint32_t e = gz_code_entry(W.lens, W.cnt, s);
        M->lut[s] = e;
        bits += (uint64_t)W.hist[s] * (e >> 16);
    }
    const uint32_t dyn = (uint32_t)((wave_sum(bits) + kGzHeadBits + 7u) / 8u);
    const bool stored = dyn >= usize + 5u;                             // one stored block whenever the dynamic one is not smaller
    if (wave_leader()) { M->crc = crc; M->stored = stored ? 1u : 0u; M->reserved = 0; }
    return stored ? usize + 5u : dyn;
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_gz_count(const uint8_t* __restrict__ in, uint64_t n, uint32_t n_members,
                                                    const uint32_t* __restrict__ crc_tab, GzMeta* __restrict__ meta,
                                                    uint64_t* __restrict__ size, GzState* S)
{
    TGSF_SHARED GzCrcTables T;
    TGSF_SHARED GzCountWave sets[kInfWaves];
    gz_crc_tables(T, crc_tab);
    GzCountWave& W = sets[(threadIdx.x / kTextLanes) % kInfWaves];
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    uint32_t stored = 0;
    for (uint64_t m = wave_uniform64(text_wave()); m < n_members; m += n_waves) {
        const uint64_t at = m * kGzMember;
        const uint32_t usize = n - at < kGzMember ? (uint32_t)(n - at) : kGzMember;
        const uint32_t payload = wave_first(gz_count_member(T, in + at, usize, W, meta + m));
        if (wave_leader()) size[m] = (uint64_t)payload + kGzFrame;
        stored += payload == usize + 5u ? 1u : 0u;
    }
    if (wave_leader() && stored) atomicAdd(&S->stored, stored);
}

// 1f 8b 08 04 00 00 00 00 00 ff 06 00 'B' 'C' 02 00: a member's first 16 bytes; the EOF member goes on 1b 00 03 00 and 8 zeros
constexpr uint64_t kGzHeadLo = 0x0000000004088B1Full, kGzHeadHi = 0x000243420006FF00ull, kGzEofTail = 0x000000000003001Bull;
TGSF_HD uint8_t gz_head_byte(uint32_t i) { return (uint8_t)((i < 8u ? kGzHeadLo >> (8u * i) : kGzHeadHi >> (8u * (i - 8u))) & 0xFFu); }
TGSF_HD uint8_t gz_eof_byte(uint32_t i) { return i < 16u ? gz_head_byte(i) : (uint8_t)(i < 24u ? (kGzEofTail >> (8u * (i - 16u))) & 0xFFu : 0u); }

// the low nbits <= 32 bits of v (nothing above them) into the staging area at bit `pos`
TGSF_D void gz_put(uint32_t* stage, uint32_t pos, uint32_t v, uint32_t nbits)
{
    const uint32_t w = pos >> 5, sh = pos & 31u;
    atomicOr(&stage[w], v << sh);
    if (sh + nbits > 32u) atomicOr(&stage[w + 1u], v >> (32u - sh));
}
// The staging area's bits [0, pos) leave for dst: its whole dwords, the bits left over move to the front (last: every byte
// that holds a bit).  Wave-uniform but for the copy.
TGSF_D void gz_flush(uint32_t* stage, uint32_t& pos, uint8_t*& dst, bool last)
{
    TGSF_WAVE_SYNC();
    const uint32_t nw = pos >> 5, nbytes = last ? (pos + 7u) / 8u : 4u * nw;
    for (uint32_t i = text_lane(); i < nbytes; i += kTextLanes) dst[i] = (uint8_t)(stage[i >> 2] >> (8u * (i & 3u)));
    if (last) return;
    const uint32_t carry = wave_first(stage[nw]);
    TGSF_WAVE_SYNC();
    for (uint32_t w = TGSF_WCOOP_BEGIN(text_lane()); w <= nw; w += TGSF_WCOOP_STRIDE) stage[w] = w == 0 ? carry : 0u;
    TGSF_WAVE_SYNC();
    dst += 4u * nw;
    pos &= 31u;
}

// a member's 26 bytes of framing around its payload: out[0 .. 18) and out[bsize - 8 .. bsize)
TGSF_D void gz_emit_frame(uint8_t* out, uint32_t bsize, uint32_t crc, uint32_t usize)
{
    for (uint32_t i = TGSF_WCOOP_BEGIN(text_lane()); i < kGzFrame; i += TGSF_WCOOP_STRIDE) {
        if (i < 16u) out[i] = gz_head_byte(i);
        else if (i < 18u) out[i] = (uint8_t)((bsize - 1u) >> (8u * (i - 16u)));
        else if (i < 22u) out[bsize - 26u + i] = (uint8_t)(crc >> (8u * (i - 18u)));
        else out[bsize - 26u + i] = (uint8_t)(usize >> (8u * (i - 22u)));
    }
}

// one member to out[0 .. bsize): the frame, then one stored or one dynamic block of in[0 .. usize)
TGSF_D void gz_emit_member(const uint8_t* __restrict__ in, uint32_t usize, const GzMeta* __restrict__ M, uint8_t* out, uint32_t bsize, GzEmitWave& E)
{
    const uint32_t lane = text_lane();
    const bool stored = wave_first(M->stored) != 0;
    gz_emit_frame(out, bsize, wave_first(M->crc), usize);
    uint8_t* dst = out + 18;
    if (stored) {                                                     // BFINAL, BTYPE 0, to the byte boundary; LEN, NLEN; the bytes
        for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < 5u; i += TGSF_WCOOP_STRIDE)
            dst[i] = (uint8_t)(i == 0 ? 1u : ((i < 3u ? usize : ~usize) >> (8u * ((i - 1u) & 1u))));
        for (uint32_t i = lane; i < usize; i += kTextLanes) dst[5u + i] = in[i];
        return;
    }
    TGSF_WAVE_SYNC();                                                  // the last member's reads of E are over
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kGzSyms; s += TGSF_WCOOP_STRIDE) E.lut[s] = M->lut[s];
    for (uint32_t w = TGSF_WCOOP_BEGIN(lane); w < kGzStageWords; w += TGSF_WCOOP_STRIDE) E.stage[w] = 0;
    TGSF_WAVE_SYNC();
    // the block's header: entry 0 is its constant front, entry 1 + s the length of symbol s, the last two the distance code
    // (two codes of one bit, as zlib writes when no distance occurs)
    for (uint32_t j = TGSF_WCOOP_BEGIN(lane); j < kGzSyms + 3u; j += TGSF_WCOOP_STRIDE) {
        if (j == 0) {
            gz_put(E.stage, 0, 1u | 2u << 1 | 0u << 3 | 1u << 8 | 15u << 13, 17);
            for (uint32_t k = 3; k < 19u; k++) gz_put(E.stage, 17u + 3u * k, 4u, 3);      // (inf_order: 16, 17, 18 come first)
        } else {
            const uint32_t l = j - 1u < kGzSyms ? E.lut[j - 1u] >> 16 : 1u;
            gz_put(E.stage, kGzFixedHeadBits + 4u * (j - 1u), (l & 1u) << 3 | (l & 2u) << 1 | (l & 4u) >> 1 | (l & 8u) >> 3, 4);
        }
    }
    uint32_t pos = kGzHeadBits;
    gz_flush(E.stage, pos, dst, false);
    for (uint32_t r0 = 0; r0 < usize; r0 += kGzRound) {
        const uint32_t off = r0 + lane * 16u;
        const uint32_t nb = off < usize ? (usize - off < 16u ? usize - off : 16u) : 0u;
        uint64_t lo = 0, hi = 0;
        if (nb == 16u) {
            const uint4 v = *reinterpret_cast<const uint4*>(in + off);
            lo = (uint64_t)v.y << 32 | v.x; hi = (uint64_t)v.w << 32 | v.z;
        } else
            for (uint32_t i = 0; i < nb; i++) { const uint64_t b = in[off + i]; if (i < 8) lo |= b << (8u * i); else hi |= b << (8u * (i - 8u)); }
        uint32_t e[16], bits = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) {
            const uint32_t b = (uint32_t)((i < 8 ? lo >> (8u * i) : hi >> (8u * (i - 8u))) & 0xFFu);
            e[i] = i < nb ? E.lut[b] : 0u;
            bits += e[i] >> 16;
        }
        uint32_t p = pos + wave_excl_scan(bits);
        pos += (uint32_t)wave_sum_i32((int32_t)bits);
        uint64_t acc = 0;
        uint32_t na = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) {
            acc |= (uint64_t)(e[i] & 0xFFFFu) << na;
            na += e[i] >> 16;
            if (na >= 32u) { gz_put(E.stage, p, (uint32_t)acc, 32); acc >>= 32; na -= 32u; p += 32u; }
        }
        if (na) gz_put(E.stage, p, (uint32_t)acc, na);
        gz_flush(E.stage, pos, dst, false);
    }
    const uint32_t eob = wave_first(E.lut[256]);
    if (wave_leader()) gz_put(E.stage, pos, eob & 0xFFFFu, eob >> 16);
    pos += eob >> 16;
    gz_flush(E.stage, pos, dst, true);
}

// ---- level 1: the match search (tgsf_text_bgzf_out_level) ---------------------------------------------------------------------------
//
//   k_gz_count_lz      k_gz_count's work on a member -- the level-0 code is one of the three candidates, and its code lengths are
//                      what a literal costs -- then the parse, then the two codes of the block of matches by the same builder
//                      and its size.  The smallest of the three is the member's size.
//   k_gz_emit_lz       k_gz_emit; a member whose block of matches won repeats the parse (nothing of it is kept between the
//                      passes) and puts a token a lane into the staging area.
//
// The parse, lz_round(): 64 positions a round, a position a lane.  (1) Each position that no earlier match covers looks for
// its two candidates -- distance 1, and the table's entry for the hash of its four bytes, a position of an EARLIER round --
// compares byte for byte, up to min(258, the bytes left in the member), and keeps the one that saves more bits than it costs
// (the literals at their level-0 code lengths against flat guesses for a match's two codes) or none.  (2) The one serial
// step, wave-uniform: the positions with a match are a 64-bit mask, the parse is greedy, so from the first position not yet
// covered the next set bit begins a match and everything in front of it is literals: a turn a MATCH TAKEN, 22 a round at most,
// on scalar registers.  (3) All 64 positions go into the table, the halves of its words in two steps: within a step every
// contender for a word holds the same other half, so atomicMax on the word leaves the highest position, whichever lane came first.
TGSF_D uint32_t lz_load32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }    // (any alignment)
TGSF_D uint64_t lz_load64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
TGSF_HD uint32_t lz_hash(uint32_t w) { return (w * 2654435761u) >> (32u - kLzHashBits); }
TGSF_HD uint32_t lz_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
// a length 3 .. 258 -> its symbol less 257, the number of its extra bits and their value (RFC 1951, 3.2.5)
TGSF_HD uint32_t lz_len_code(uint32_t len, uint32_t* n_extra, uint32_t* extra)
{
    const uint32_t l = len - 3u;
    if (l < 8u || len == kLzMaxLen) { *n_extra = 0; *extra = 0; return len == kLzMaxLen ? 28u : l; }
    const uint32_t e = lz_log2(l) - 2u;
    *n_extra = e; *extra = l & ((1u << e) - 1u);
    return 4u * e + 4u + ((l >> e) & 3u);
}
// a distance 1 .. 32768 -> its symbol, the number of its extra bits and their value
TGSF_HD uint32_t lz_dist_code(uint32_t dist, uint32_t* n_extra, uint32_t* extra)
{
    const uint32_t d = dist - 1u;
    if (d < 4u) { *n_extra = 0; *extra = 0; return d; }
    const uint32_t e = lz_log2(d) - 1u;
    *n_extra = e; *extra = d & ((1u << e) - 1u);
    return 2u * e + 2u + ((d >> e) & 1u);
}
// the bytes a[0 ..) and b[0 ..) have in common, cap at most: eight at a time, then one at a time; a[cap] and b[cap] are not read
TGSF_D uint32_t lz_common(const uint8_t* a, const uint8_t* b, uint32_t cap)
{
    uint32_t i = 0;
    for (; i + 8u <= cap; i += 8u) {
        const uint64_t x = lz_load64(a + i) ^ lz_load64(b + i);
        if (x) return i + ((uint32_t)__builtin_ctzll(x) >> 3);
    }
    for (; i < cap && a[i] == b[i]; i++) {}
    return i;
}
// What a match of len bytes at p[0 ..) saves, in bits: its bytes as literals of the level-0 code (lens0; beyond 32 bytes a bit
// each, the least a literal costs: such a match pays whatever it costs) less a guess at its two codes and its extra bits.
constexpr uint32_t kLzLenCost = 7, kLzDistCost = 6, kLzDist1Cost = 2;
TGSF_D int32_t lz_gain(const uint8_t* p, uint32_t len, uint32_t dist, const uint8_t* lens0)
{
    uint32_t lit = len > 32u ? len - 32u : 0u, le, de, x, i = 0;
    const uint32_t k = len < 32u ? len : 32u;
    for (; i + 8u <= k; i += 8u) {                                     // (eight bytes a load: the loads are what the parse waits for)
        const uint64_t w = lz_load64(p + i);
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++) lit += lens0[(w >> (8u * b)) & 0xFFu];
    }
    if (i + 4u <= k) {
        const uint32_t w = lz_load32(p + i);
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++) lit += lens0[(w >> (8u * b)) & 0xFFu];
        i += 4u;
    }
    for (; i < k; i++) lit += lens0[p[i]];
    lz_len_code(len, &le, &x);
    lz_dist_code(dist, &de, &x);
    return (int32_t)lit - (int32_t)(kLzLenCost + le + (dist == 1u ? kLzDist1Cost : kLzDistCost + de));
}
// slots[i], which lane i of the wave holds in `mine` (i: wave-uniform)
#if !defined(TGSF_EMUL)
TGSF_D uint32_t lz_lane_value(uint32_t mine, const uint32_t*, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)mine, __builtin_amdgcn_readfirstlane((int)i)); }
#else
TGSF_HD uint32_t lz_lane_value(uint32_t, const uint32_t* slots, uint32_t i) { return slots[i]; }
#endif

// One round of the parse: positions r0 .. r0 + 64 of in[0 .. usize).  carry: how many positions at the round's front a match
// of an earlier round covers (in: this round's; out: the next one's).  taken: the positions that begin a match, L.rm[] says
// which; lit: the positions that are literals.  Wave-uniform but for L.rm[].
TGSF_D void lz_round(const uint8_t* __restrict__ in, uint32_t usize, uint32_t r0, uint32_t& carry, GzLzWave& L, const uint8_t* lens0, uint64_t& taken, uint64_t& lit)
{
    [[maybe_unused]] const uint32_t lane = text_lane();
    const uint32_t nr = usize - r0 < kLzRound ? usize - r0 : kLzRound;
    const bool search = carry < nr;                                    // else a match covers the whole round
    TGSF_WAVE_SYNC();                                                  // the last round's reads of L.rm are over
    if (search) {
        if (wave_leader()) { L.mask[0] = 0; L.mask[1] = 0; }
        TGSF_WAVE_SYNC();
        for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < kLzRound; i += TGSF_WCOOP_STRIDE) {
            uint32_t m = 0;
            if (i >= carry && i < nr) {
                const uint32_t p = r0 + i, cap = usize - p < kLzMaxLen ? usize - p : kLzMaxLen;
                int32_t best = 0;
                if (p >= 1u && cap >= 3u) {                            // a run: the table cannot see inside a round
                    const uint32_t len = lz_common(in + p, in + p - 1u, cap);
                    if (len >= 3u) { const int32_t g = lz_gain(in + p, len, 1u, lens0); if (g > best) { best = g; m = len; } }
                }
                if (cap >= 4u) {
                    const uint32_t w = lz_load32(in + p), s = lz_hash(w);
                    const uint32_t e = (L.table[s & (kLzSlots / 2u - 1u)] >> (16u * (s >> (kLzHashBits - 1u)))) & 0xFFFFu;
                    if (e) {
                        const uint32_t c = e - 1u, dist = p - c;       // (c < r0: the member's own bytes, never in front of them)
                        if (dist <= kLzMaxDist && lz_load32(in + c) == w) {
                            const uint32_t len = 4u + lz_common(in + p + 4u, in + c + 4u, cap - 4u);
                            const int32_t g = lz_gain(in + p, len, dist, lens0);
                            if (g > best) { best = g; m = len | (dist - 1u) << 9; }
                        }
                    }
                }
                if (m) atomicOr(&L.mask[i >> 5], 1u << (i & 31u));
            }
            L.rm[i] = m;
        }
        TGSF_WAVE_SYNC();
    }
    const uint64_t mask = search ? (uint64_t)wave_first(L.mask[1]) << 32 | wave_first(L.mask[0]) : 0ull;
    const uint32_t mine = search ? L.rm[lane % kLzRound] : 0u;
    uint64_t cover = carry >= kLzRound ? ~0ull : (1ull << carry) - 1ull;
    uint32_t cur = carry;
    taken = 0;
    while (cur < nr) {                                                 // a match a turn
        const uint64_t rest = mask >> cur;
        if (!rest) break;
        cur += (uint32_t)__builtin_ctzll(rest);
        const uint32_t end = cur + (lz_lane_value(mine, L.rm, cur) & 511u);
        taken |= 1ull << cur;
        cover |= (end >= kLzRound ? ~0ull : (1ull << end) - 1ull) & ~((1ull << cur) - 1ull);
        cur = end;
    }
    carry = cur > kLzRound ? cur - kLzRound : 0u;
    lit = (nr >= kLzRound ? ~0ull : (1ull << nr) - 1ull) & ~cover;
    for (uint32_t half = 0; half < 2u; half++) {                       // covered or not, every position with four bytes goes into the table
        for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < kLzRound; i += TGSF_WCOOP_STRIDE) {
            const uint32_t p = r0 + i;
            if (i >= nr || usize - p < 4u) continue;
            const uint32_t s = lz_hash(lz_load32(in + p));
            if ((s >> (kLzHashBits - 1u)) != half) continue;
            uint32_t* word = &L.table[s & (kLzSlots / 2u - 1u)];
            const uint32_t old = *word;                                // (its other half does not change in this step)
            atomicMax(word, half ? (p + 1u) << 16 | (old & 0xFFFFu) : (old & 0xFFFF0000u) | (p + 1u));
        }
        TGSF_WAVE_SYNC();
    }
}

// A member's block of matches: the parse, the two codes (to Z), its size.  payload0: what gz_count_member returned; lens0: the
// level-0 code's lengths, which it left.  Returns the payload's bytes, the smallest of the three (wave-uniform).
TGSF_D uint32_t gz_lz_count_member(const uint8_t* __restrict__ in, uint32_t usize, uint32_t payload0, const uint8_t* lens0, GzLzWave& L, GzLzMeta* Z)
{
    [[maybe_unused]] const uint32_t lane = text_lane();
    TGSF_WAVE_SYNC();                                                  // the last member's reads of L are over
    for (uint32_t w = TGSF_WCOOP_BEGIN(lane); w < kLzSlots / 2u; w += TGSF_WCOOP_STRIDE) L.table[w] = 0;
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kLzSymRoom; s += TGSF_WCOOP_STRIDE) { L.sym[s] = s == 256u ? 1u : 0u; L.lens[s] = 0; }
    uint32_t carry = 0;
    uint64_t bits = 0;
    for (uint32_t r0 = 0; r0 < usize; r0 += kLzRound) {
        uint64_t taken, lit;
        lz_round(in, usize, r0, carry, L, lens0, taken, lit);
        for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < kLzRound; i += TGSF_WCOOP_STRIDE) {
            if ((taken >> i) & 1u) {
                const uint32_t m = L.rm[i];
                uint32_t le, de, x;
                atomicAdd(&L.sym[257u + lz_len_code(m & 511u, &le, &x)], 1u);
                atomicAdd(&L.sym[kLzLitRoom + lz_dist_code((m >> 9) + 1u, &de, &x)], 1u);
                bits += le + de;
            } else if ((lit >> i) & 1u)
                atomicAdd(&L.sym[in[r0 + i]], 1u);
        }
    }
    TGSF_WAVE_SYNC();
    gz_code_lengths(L.sym, kLzLitSyms, L.freq, L.order, L.lens, L.cnt[0]);
    gz_code_lengths(L.sym + kLzLitRoom, kLzDistSyms, L.freq, L.order, L.lens + kLzLitRoom, L.cnt[1]);
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kLzLitSyms + kLzDistSyms; s += TGSF_WCOOP_STRIDE) {
        const uint32_t d = s >= kLzLitSyms ? 1u : 0u, t = d ? s - kLzLitSyms : s;
        const uint32_t e = gz_code_entry(L.lens + d * kLzLitRoom, L.cnt[d], t);
        if (d) Z->dlut[t] = e; else Z->llut[t] = e;
        bits += (uint64_t)L.sym[d * kLzLitRoom + t] * (e >> 16);
    }
    const uint32_t lz = (uint32_t)((wave_sum(bits) + kLzHeadBits + 7u) / 8u);
    const bool use = lz < payload0;
    if (wave_leader()) { Z->lz = use ? 1u : 0u; Z->reserved[0] = Z->reserved[1] = Z->reserved[2] = 0; }
    return use ? lz : payload0;
}

TGSF_KERNEL TGSF_BOUNDS(kLzThreads, 2) k_gz_count_lz(const uint8_t* __restrict__ in, uint64_t n, uint32_t n_members,
                                                     const uint32_t* __restrict__ crc_tab, GzMeta* __restrict__ meta,
                                                     GzLzMeta* __restrict__ lzmeta, uint64_t* __restrict__ size, GzState* S)
{
    TGSF_SHARED GzCrcTables T;
    TGSF_SHARED GzCountWave sets[kLzWaves];
    TGSF_SHARED GzLzWave lzs[kLzWaves];
    gz_crc_tables(T, crc_tab);
    GzCountWave& W = sets[(threadIdx.x / kTextLanes) % kLzWaves];
    GzLzWave& L = lzs[(threadIdx.x / kTextLanes) % kLzWaves];
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    uint32_t stored = 0;
    for (uint64_t m = wave_uniform64(text_wave()); m < n_members; m += n_waves) {
        const uint64_t at = m * kGzMember;
        const uint32_t usize = n - at < kGzMember ? (uint32_t)(n - at) : kGzMember;
        const uint32_t payload0 = wave_first(gz_count_member(T, in + at, usize, W, meta + m));
        const uint32_t payload = wave_first(gz_lz_count_member(in + at, usize, payload0, W.lens, L, lzmeta + m));
        if (wave_leader()) size[m] = (uint64_t)payload + kGzFrame;
        stored += payload == usize + 5u ? 1u : 0u;
    }
    if (wave_leader() && stored) atomicAdd(&S->stored, stored);
}

// one member's block of matches to out[0 .. bsize): the frame, the header with both codes, the parse again, a token a lane
TGSF_D void gz_lz_emit_member(const uint8_t* __restrict__ in, uint32_t usize, const GzMeta* __restrict__ M, const GzLzMeta* __restrict__ Z, uint8_t* out,
                              uint32_t bsize, uint32_t* stage, GzLzWave& L)
{
    [[maybe_unused]] const uint32_t lane = text_lane();
    gz_emit_frame(out, bsize, wave_first(M->crc), usize);
    uint8_t* dst = out + 18;
    TGSF_WAVE_SYNC();                                                  // the last member's reads of L and the staging area are over
    for (uint32_t w = TGSF_WCOOP_BEGIN(lane); w < kLzSlots / 2u; w += TGSF_WCOOP_STRIDE) L.table[w] = 0;
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < kLzLitSyms + kLzDistSyms; s += TGSF_WCOOP_STRIDE)
        L.sym[s < kLzLitSyms ? s : kLzLitRoom + s - kLzLitSyms] = s < kLzLitSyms ? Z->llut[s] : Z->dlut[s - kLzLitSyms];
    for (uint32_t s = TGSF_WCOOP_BEGIN(lane); s < 256u; s += TGSF_WCOOP_STRIDE) L.lens0[s] = (uint8_t)(M->lut[s] >> 16);
    for (uint32_t w = TGSF_WCOOP_BEGIN(lane); w < kGzStageWords; w += TGSF_WCOOP_STRIDE) stage[w] = 0;
    TGSF_WAVE_SYNC();
    // the block's header: entry 0 is its constant front (HLIT 286, HDIST 30), entry 1 + s the length of symbol s of either code
    for (uint32_t j = TGSF_WCOOP_BEGIN(lane); j < kLzLitSyms + kLzDistSyms + 1u; j += TGSF_WCOOP_STRIDE) {
        if (j == 0) {
            gz_put(stage, 0, 1u | 2u << 1 | (kLzLitSyms - 257u) << 3 | (kLzDistSyms - 1u) << 8 | 15u << 13, 17);
            for (uint32_t k = 3; k < 19u; k++) gz_put(stage, 17u + 3u * k, 4u, 3);
        } else {
            const uint32_t l = L.sym[j - 1u < kLzLitSyms ? j - 1u : kLzLitRoom + j - 1u - kLzLitSyms] >> 16;
            gz_put(stage, kGzFixedHeadBits + 4u * (j - 1u), (l & 1u) << 3 | (l & 2u) << 1 | (l & 4u) >> 1 | (l & 8u) >> 3, 4);
        }
    }
    uint32_t pos = kLzHeadBits, carry = 0;
    gz_flush(stage, pos, dst, false);
    for (uint32_t r0 = 0; r0 < usize; r0 += kLzRound) {
        uint64_t taken, lit;
        lz_round(in, usize, r0, carry, L, L.lens0, taken, lit);
        for (uint32_t i = TGSF_WCOOP_BEGIN(lane); i < kLzRound; i += TGSF_WCOOP_STRIDE) {
            uint64_t v = 0;
            uint32_t nb = 0;
            if ((taken >> i) & 1u) {
                const uint32_t m = L.rm[i];
                uint32_t le, lx, de, dx;
                const uint32_t el = L.sym[257u + lz_len_code(m & 511u, &le, &lx)], ed = L.sym[kLzLitRoom + lz_dist_code((m >> 9) + 1u, &de, &dx)];
                v = el & 0xFFFFu; nb = el >> 16;
                v |= (uint64_t)lx << nb; nb += le;
                v |= (uint64_t)(ed & 0xFFFFu) << nb; nb += ed >> 16;
                v |= (uint64_t)dx << nb; nb += de;
            } else if ((lit >> i) & 1u) {
                const uint32_t e = L.sym[in[r0 + i]];
                v = e & 0xFFFFu; nb = e >> 16;
            }
            const uint32_t p = pos + wave_excl_scan(nb);
            pos += (uint32_t)wave_sum_i32((int32_t)nb);
            if (nb > 32u) { gz_put(stage, p, (uint32_t)v, 32); gz_put(stage, p + 32u, (uint32_t)(v >> 32), nb - 32u); }
            else if (nb) gz_put(stage, p, (uint32_t)v, nb);
        }
        // the staging area takes rounds until the next might not fit: few tokens a round where the matches are long
        if (pos + kLzTokenBits * kLzRound + 64u > 32u * kGzStageWords) gz_flush(stage, pos, dst, false);
    }
    const uint32_t eob = wave_first(L.sym[256]);
    TGSF_WAVE_SYNC();
    if (wave_leader()) gz_put(stage, pos, eob & 0xFFFFu, eob >> 16);
    pos += eob >> 16;
    gz_flush(stage, pos, dst, true);
}
static_assert(32u * kGzStageWords >= 31u + kLzTokenBits * kLzRound + 64u, "a round of tokens fits behind what a flush leaves");

// what k_gz_emit and k_gz_emit_lz do (Lz: L and lzmeta are there, and a member may be a block of matches)
template <bool Lz>
TGSF_D void gz_emit_all(const uint8_t* __restrict__ in, uint64_t n, uint32_t n_members, int eof, const GzMeta* __restrict__ meta,
                        const GzLzMeta* __restrict__ lzmeta, const uint64_t* __restrict__ size_excl, const uint64_t* __restrict__ size_part,
                        const GzState* S, uint64_t capacity, uint8_t* out, uint64_t* __restrict__ member_end, tgsf_text_gzout_summary* sum,
                        GzEmitWave& E, GzLzWave* L)
{
    const uint64_t body = S->total, total = body + (eof ? kGzEofBytes : 0u);
    const bool fits = total <= capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sum->in_bytes = n;
        sum->n_bytes = total;
        sum->n_members = n_members + (eof ? 1u : 0u);
        sum->stored = S->stored;
        sum->stop = fits ? TGSF_TEXT_END : TGSF_TEXT_CAPACITY;
        sum->device_ms = 0.0f;
        sum->reserved = 0;
    }
    if (!fits) return;                                                 // TGSF_TEXT_CAPACITY: nothing is written
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    for (uint64_t m = wave_uniform64(text_wave()); m < n_members; m += n_waves) {
        const uint64_t at = m * kGzMember;
        const uint32_t usize = n - at < kGzMember ? (uint32_t)(n - at) : kGzMember;
        const uint64_t begin = size_part[m / kTextScanTile] + size_excl[m];       // (the same in every lane, and left in vector registers: addresses of stores)
        const uint64_t end = m + 1 == n_members ? body : size_part[(m + 1) / kTextScanTile] + size_excl[m + 1];
        if (Lz && wave_first(lzmeta[m].lz)) gz_lz_emit_member(in + at, usize, meta + m, lzmeta + m, out + begin, (uint32_t)(end - begin), E.stage, *L);
        else gz_emit_member(in + at, usize, meta + m, out + begin, (uint32_t)(end - begin), E);
        if (member_end && wave_leader()) member_end[m] = end;
    }
    if (eof && text_wave() == 0) {
        for (uint32_t i = TGSF_WCOOP_BEGIN(text_lane()); i < kGzEofBytes; i += TGSF_WCOOP_STRIDE) out[body + i] = gz_eof_byte(i);
        if (member_end && wave_leader()) member_end[n_members] = total;
    }
}

TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_gz_emit(const uint8_t* __restrict__ in, uint64_t n, uint32_t n_members, int eof,
                                                   const GzMeta* __restrict__ meta, const uint64_t* __restrict__ size_excl,
                                                   const uint64_t* __restrict__ size_part, const GzState* S, uint64_t capacity,
                                                   uint8_t* out, uint64_t* __restrict__ member_end, tgsf_text_gzout_summary* sum)
{
    TGSF_SHARED GzEmitWave sets[kInfWaves];
    gz_emit_all<false>(in, n, n_members, eof, meta, nullptr, size_excl, size_part, S, capacity, out, member_end, sum,
                       sets[(threadIdx.x / kTextLanes) % kInfWaves], nullptr);
}

TGSF_KERNEL TGSF_BOUNDS(kLzThreads, 2) k_gz_emit_lz(const uint8_t* __restrict__ in, uint64_t n, uint32_t n_members, int eof,
                                                    const GzMeta* __restrict__ meta, const GzLzMeta* __restrict__ lzmeta,
                                                    const uint64_t* __restrict__ size_excl, const uint64_t* __restrict__ size_part,
                                                    const GzState* S, uint64_t capacity, uint8_t* out, uint64_t* __restrict__ member_end,
                                                    tgsf_text_gzout_summary* sum)
{
    TGSF_SHARED GzEmitWave sets[kLzWaves];
    TGSF_SHARED GzLzWave lzs[kLzWaves];
    gz_emit_all<true>(in, n, n_members, eof, meta, lzmeta, size_excl, size_part, S, capacity, out, member_end, sum,
                      sets[(threadIdx.x / kTextLanes) % kLzWaves], &lzs[(threadIdx.x / kTextLanes) % kLzWaves]);
}

// bad_crc: the lowest member whose inflated bytes do not have the CRC32 of its trailer (0xFFFFFFFF, set by the caller: none)
TGSF_KERNEL TGSF_BOUNDS(kTextThreads, 2) k_bgzf_crc(const uint8_t* __restrict__ gz, const tgsf_text_bgzf_block* __restrict__ blocks,
                                                    uint32_t n_blocks, const uint8_t* __restrict__ inflated,
                                                    const uint32_t* __restrict__ crc_tab, uint32_t* bad_crc)
{
    TGSF_SHARED GzCrcTables T;
    gz_crc_tables(T, crc_tab);
    const uint64_t n_waves = gridDim.x * (uint64_t)blockDim.x / kTextLanes;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t b = wave_uniform64(text_wave()); b < n_blocks; b += n_waves) {
        const uint64_t trailer = wave_uniform64(blocks[b].payload) + wave_first(blocks[b].clen), at = wave_uniform64(blocks[b].out);
        const uint32_t usize = wave_first(blocks[b].usize);
        const uint32_t crc = gz_crc_wave<false>(T, inflated + at, usize, nullptr);
        if (crc != wave_first(bam_le32(gz + trailer)) && (uint32_t)b < bad) bad = (uint32_t)b;
    }
    wave_min_into(bad_crc, bad);
}

}  // namespace tgsf
