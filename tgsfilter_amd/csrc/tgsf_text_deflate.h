// ---- the BGZF output side: text -> compressed members (tgsf_text_bgzf_deflate*; included behind tgsf_text_crc.h) ------------
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
//
// EVERY LOOP IS BOUNDED BY THE MEMBER'S SIZE OR BY THE ALPHABET'S: no input byte steers a loop count.
#pragma once
namespace tgsf {

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

// the end of a block: its code (eob_entry, wave-uniform) behind the pos bits of the staging area, and everything leaves for dst
TGSF_D void gz_finish_block(uint32_t* stage, uint32_t pos, uint8_t* dst, uint32_t eob_entry)
{
    if (wave_leader()) gz_put(stage, pos, eob_entry & 0xFFFFu, eob_entry >> 16);
    pos += eob_entry >> 16;
    gz_flush(stage, pos, dst, true);
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
    gz_finish_block(E.stage, pos, dst, wave_first(E.lut[256]));
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
    TGSF_WAVE_SYNC();                                                  // (this path alone: the last round may not have flushed)
    gz_finish_block(stage, pos, dst, eob);
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
}  // namespace tgsf
