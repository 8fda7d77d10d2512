// TEST INFRASTRUCTURE: the BGZF output side of libtgsf_text (tgsf_text_bgzf_deflate*, _verify) through the serial emulation of
// its kernels built with the host compiler's address and undefined-behaviour sanitizers.  This file includes the library's
// source, compiled with -DTGSF_EMUL, so the whole is one host program; of libtgsf it needs the emulation beside it:
//
//   make -s -C tests/emul
//   g++ -O1 -g -std=c++17 -DTGSF_EMUL -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wno-unused-function
//       -Wno-unknown-pragmas -x c++ tests/manual/gzout_asan.cpp -o tests/emul/gzout_asan -Ltests/emul -ltgsf_emul
//       -Wl,-rpath,'$ORIGIN'                                                                        (one command line)
//   tests/emul/gzout_asan
//
// The emulation's device memory is host memory, so a byte read outside the text or written outside the output is a report:
// the text and the output here are heap blocks of exactly their size (16-byte aligned), member_end has exactly n_members words.
//   - the length sweep: every length 0..300, the lengths around 1024, around the member size and around two members, FASTQ-like
//     and of one byte value, with and without the EOF member;
//   - the bit-seam sweep: a text of one byte value with a rare byte at every position 0..200 and at the last; 64 consecutive
//     lengths of three alphabets;
//   - the capacity sweep: out_capacity exactly what is needed, one byte short (nothing is written), and 0.
//   - the CRC combination (x^(8 n) mod P), which a wave of one never needs, against a bit-by-bit CRC32.
// Every output goes back through the library's own inflate and CRC check (tgsf_text_bgzf_verify, tgsf_text_bgzf_inflate:
// tests/test_bgzf_emul.py holds them to zlib) and must give the text; the device form's bytes equal the host form's.
// Exit status 0 and "gzout ok": no difference, no error code, no sanitizer report (a report ends the program).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/tgsf_text.h"
#include "../../tgsfilter_amd/csrc/tgsf_text.hip"     // (TGSF_EMUL: the kernels as serial host code)

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n)           // a fixed linear-congruential generator (Knuth's MMIX constants)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

typedef std::vector<uint8_t> Bytes;
static int g_checked = 0;

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// exactly n bytes, 16-byte aligned (n == 0: one byte nobody may touch)
static uint8_t* exact(size_t n)
{
    void* p = nullptr;
    REQUIRE(posix_memalign(&p, 16, n ? n : 1) == 0, "out of memory");
    return (uint8_t*)p;
}

static Bytes fastq_like(size_t n)
{
    Bytes t;
    while (t.size() < n) {
        const uint32_t l = 30 + rnd(400);
        t.push_back('@');
        for (uint32_t i = 0; i < 6 + rnd(20); i++) t.push_back((uint8_t)(48 + rnd(60)));
        t.push_back('\n');
        for (uint32_t i = 0; i < l; i++) t.push_back((uint8_t)"ACGT"[rnd(4)]);
        t.push_back('\n'); t.push_back('+'); t.push_back('\n');
        for (uint32_t i = 0; i < l; i++) t.push_back((uint8_t)(33 + 20 + rnd(8) + rnd(8) + rnd(8)));
        t.push_back('\n');
    }
    t.resize(n);
    return t;
}

static tgsf_text* g_tx;

// one text through the host form, the device form at exactly the room it needs, one byte short, and back
static void check(const Bytes& text, int eof, const char* what)
{
    const uint64_t n = text.size(), bound = tgsf_text_bgzf_bound(n, eof);
    const uint32_t members = (uint32_t)((n + TGSF_TEXT_BGZF_MEMBER - 1) / TGSF_TEXT_BGZF_MEMBER) + (eof ? 1u : 0u);
    Bytes host(bound + 1, 0xA5);
    std::vector<uint64_t> hend(members + 1, 0xA5A5A5A5A5A5A5A5ull);
    tgsf_text_gzout_summary hs;
    int rc = tgsf_text_bgzf_deflate(g_tx, text.data(), n, eof, host.data(), bound, hend.data(), &hs);
    REQUIRE(rc == TGSF_OK, "%s: deflate returned %d: %s", what, rc, tgsf_text_last_error(g_tx));
    REQUIRE(hs.in_bytes == n && hs.n_bytes <= bound && hs.n_members == members && hs.stop == TGSF_TEXT_END && hs.reserved == 0, "%s: summary", what);
    REQUIRE(host[hs.n_bytes] == 0xA5 && hend[members] == 0xA5A5A5A5A5A5A5A5ull, "%s: written behind the output", what);
    REQUIRE(members == 0 || hend[members - 1] == hs.n_bytes, "%s: member_end", what);
    // the device form: the text, the output and member_end in blocks of exactly their size
    uint8_t* d_in = exact(n);
    if (n) memcpy(d_in, text.data(), n);
    uint8_t* d_out = exact(hs.n_bytes);
    uint64_t* d_end = (uint64_t*)exact(8 * (size_t)members);
    tgsf_text_gzout_summary* d_sum = (tgsf_text_gzout_summary*)exact(sizeof(tgsf_text_gzout_summary));
    for (uint64_t cap : {hs.n_bytes, hs.n_bytes - 1, (uint64_t)0}) {
        if (hs.n_bytes == 0 && cap != 0) continue;
        if (hs.n_bytes) memset(d_out, 0xA5, hs.n_bytes);
        rc = tgsf_text_bgzf_deflate_device(g_tx, d_in, n, eof, d_out, cap, d_end, d_sum, nullptr);
        REQUIRE(rc == TGSF_OK, "%s: deflate_device returned %d: %s", what, rc, tgsf_text_last_error(g_tx));
        REQUIRE(d_sum->n_bytes == hs.n_bytes && d_sum->n_members == members && d_sum->stored == hs.stored, "%s: device summary", what);
        if (cap == hs.n_bytes) {
            REQUIRE(d_sum->stop == TGSF_TEXT_END && (hs.n_bytes == 0 || memcmp(d_out, host.data(), hs.n_bytes) == 0), "%s: the device form's bytes", what);
            REQUIRE(members == 0 || memcmp(d_end, hend.data(), 8 * (size_t)members) == 0, "%s: the device form's member_end", what);
        } else {
            REQUIRE(d_sum->stop == TGSF_TEXT_CAPACITY, "%s: capacity %llu of %llu accepted", what, (unsigned long long)cap, (unsigned long long)hs.n_bytes);
            for (uint64_t i = 0; i < hs.n_bytes; i++) REQUIRE(d_out[i] == 0xA5, "%s: CAPACITY, and byte %llu was written", what, (unsigned long long)i);
        }
    }
    free(d_in); free(d_out); free(d_end); free(d_sum);
    // back: the library's own inflate and CRC check
    uint32_t bad_block = 0, bad_crc = 0;
    rc = tgsf_text_bgzf_verify(g_tx, host.data(), hs.n_bytes, 1, &bad_block, &bad_crc);
    REQUIRE(rc == TGSF_OK && bad_block == 0xFFFFFFFFu && bad_crc == 0xFFFFFFFFu, "%s: verify returned %d (%u, %u): %s", what, rc, bad_block, bad_crc, tgsf_text_last_error(g_tx));
    Bytes back(n + 1, 0xA5);
    tgsf_text_bgzf_summary gs;
    rc = tgsf_text_bgzf_inflate(g_tx, host.data(), hs.n_bytes, 1, back.data(), n, &gs);
    REQUIRE(rc == TGSF_OK && gs.out_bytes == n && gs.n_blocks == members && gs.bad_block == 0xFFFFFFFFu, "%s: inflate returned %d: %s", what, rc, tgsf_text_last_error(g_tx));
    REQUIRE((n == 0 || memcmp(back.data(), text.data(), n) == 0) && back[n] == 0xA5, "%s: the round trip", what);
    g_checked++;
}

int main()
{
    const uint64_t M = TGSF_TEXT_BGZF_MEMBER, max_in = 2 * M + 64;
    int rc = tgsf_text_create(0, max_in, 16, &g_tx);
    REQUIRE(rc == TGSF_OK, "create: %s", tgsf_text_last_error(nullptr));
    REQUIRE(tgsf_text_bgzf_out_reserve(g_tx, max_in, tgsf_text_bgzf_bound(max_in, 1)) == TGSF_OK, "out_reserve: %s", tgsf_text_last_error(g_tx));
    REQUIRE(tgsf_text_bgzf_reserve(g_tx, tgsf_text_bgzf_bound(max_in, 1), 8) == TGSF_OK, "reserve: %s", tgsf_text_last_error(g_tx));
    const Bytes fq = fastq_like(max_in);
    char what[96];
    // the length sweep
    std::vector<uint64_t> lens;
    for (uint64_t n = 0; n <= 300; n++) lens.push_back(n);
    for (uint64_t c : {(uint64_t)1024, (uint64_t)4096, M, 2 * M}) for (uint64_t n = c - 2; n <= c + 2; n++) lens.push_back(n);
    for (uint64_t n : lens) {
        snprintf(what, sizeof what, "length %llu", (unsigned long long)n);
        check(Bytes(fq.begin(), fq.begin() + n), (int)(n & 1), what);
        check(Bytes(n, (uint8_t)'G'), (int)(~n & 1), what);
    }
    // the bit-seam sweep
    for (uint32_t p = 0; p <= 201; p++) {
        Bytes t(1500, (uint8_t)'A');
        t[p == 201 ? t.size() - 1 : p] = '#';
        snprintf(what, sizeof what, "rare byte %u", p);
        check(t, (int)(p & 1), what);
    }
    Bytes two(2100), sixteen(2100);
    for (size_t i = 0; i < two.size(); i++) { two[i] = rnd(10) ? 'A' : 'C'; uint32_t k = 0; while (k < 15 && rnd(2)) k++; sixteen[i] = (uint8_t)(33 + k); }
    for (uint64_t n = 2000; n < 2064; n++) {
        snprintf(what, sizeof what, "alphabets, length %llu", (unsigned long long)n);
        check(Bytes(fq.begin() + 77, fq.begin() + 77 + n), 0, what);
        check(Bytes(two.begin(), two.begin() + n), 0, what);
        check(Bytes(sixteen.begin(), sixteen.begin() + n), 1, what);
    }
    // bytes that do not compress: stored members, at the member size and around it
    Bytes noise(max_in);
    for (auto& b : noise) b = (uint8_t)rnd(256);
    for (uint64_t n : {(uint64_t)1, (uint64_t)700, M - 1, M, M + 1, 2 * M + 1}) {
        snprintf(what, sizeof what, "noise %llu", (unsigned long long)n);
        check(Bytes(noise.begin(), noise.begin() + n), 1, what);
    }
    // the arithmetic that only the 64-lane build reaches (a wave of one has no bytes behind its slice): crc(A B) =
    // crc(A) x^(8 |B|) + crc(B), against a bit-by-bit CRC32 written here
    auto crc32 = [](const uint8_t* p, size_t n) {
        uint32_t c = 0xFFFFFFFFu;
        for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
        return ~c;
    };
    REQUIRE(crc32((const uint8_t*)"123456789", 9) == 0xCBF43926u, "the check value of CRC-32");
    for (uint32_t total : {1u, 2u, 17u, 1024u, 65279u, 65280u, 65536u})
        for (uint32_t cut : {0u, 1u, 16u, total / 64u, total / 2u, total - 1u, total}) {
            if (cut > total) continue;
            const uint32_t a = crc32(noise.data(), cut), b = crc32(noise.data() + cut, total - cut);
            REQUIRE((tgsf::gz_mulmod(a, tgsf::gz_xpow8(total - cut)) ^ b) == crc32(noise.data(), total), "crc combine at %u of %u", cut, total);
        }
    tgsf_text_destroy(g_tx);
    printf("gzout ok: %d texts\n", g_checked);
    return 0;
}
