// ---- the CRC32 both BGZF sides need (tgsf_text_bgzf_crc_device, _verify, the deflate; included by tgsf_text_kernels.h) --------
//   k_bgzf_crc         a wave per member of a block table: CRC32 of its inflated bytes against its trailer
//   (gz_crc_wave<true> is k_gz_count's one read of a member: tgsf_text_deflate.h)
#pragma once
namespace tgsf {

struct GzCrcTables { uint32_t t[4][256]; };                // t[k][b]: the register after byte b and k zero bytes (slicing by 4)

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
