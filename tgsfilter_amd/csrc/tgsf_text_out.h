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
#pragma once
namespace tgsf {

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
}  // namespace tgsf
