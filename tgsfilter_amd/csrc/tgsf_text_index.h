// ---- the record index of FASTQ / FASTA text (tgsf_text_index*; included by tgsf_text_kernels.h) -----------------------------
//
//   k_text_mark        one streaming read of the text, 16 bytes a lane: a bit per byte ('\n' or not) and the number of
//                      line ends of every 4 KiB piece (one wave's share).  The text is not read again as a stream.
//   k_text_scan_top    behind k_text_scan_tiles<uint32_t>: exclusive prefix sums of those counts; resets the state
//   k_text_emit        every wave turns the bits of four pieces into 64-bit positions, in order, at each piece's offset of
//                      the line-end table (lane prefix count, no atomics); only the first 4 * max_records are kept
//   k_text_check       a lane per group of 4 (2) lines: five table entries, the first byte of lines 0 and 2, the byte in
//                      front of each line end ('\r'); writes the record's index words, folds the first irregular group
//   k_text_fold        bases and longest over the records of the index (per wave first, then one atomic); k_text_fold<TextState>
//                      here, k_text_fold<BamState> on the BAM input side
//   k_text_finish      one lane: n_records, consumed, why the index ends
#pragma once
namespace tgsf {

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

// text_scan_top() of the line ends; resets the state
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
}  // namespace tgsf
