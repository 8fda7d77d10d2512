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
#pragma once
namespace tgsf {

#if !defined(TGSF_EMUL)
// 8 bytes at any alignment (one global_load_dwordx2)
struct __attribute__((packed, aligned(1))) U2u { uint32_t x, y; };
TGSF_D uint64_t load8u(const uint8_t* p) { const U2u* q = reinterpret_cast<const U2u*>(p); return (uint64_t)q->y << 32 | q->x; }
#else
TGSF_HD uint64_t load8u(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
#endif

struct BamState {
    uint64_t total;        // sum of the sizes of the walked records
    uint64_t bases;
    uint32_t first_bad;    // first walked record that is not regular (0xFFFFFFFF: none)
    uint32_t first_over;   // first walked record whose text ends behind max_bytes (0xFFFFFFFF: none)
    uint32_t longest;
    uint32_t reserved;
};

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
}  // namespace tgsf
