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
#pragma once
namespace tgsf {

struct BgzfState { uint32_t bad_block, bad_crc; };      // the lowest bad member; the lowest whose CRC32 differs, when asked (0xFFFFFFFF: none)

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
}  // namespace tgsf
