// TEST INFRASTRUCTURE: the match search of the BGZF output side of libtgsf_text (level 1, tgsf_text_bgzf_out_level) through the
// serial emulation of its kernels built with the host compiler's address and undefined-behaviour sanitizers.  This file includes
// the library's source, compiled with -DTGSF_EMUL, so the whole is one host program; of libtgsf it needs the emulation beside it:
//
//   make -s -C tests/emul
//   g++ -O1 -g -std=c++17 -DTGSF_EMUL -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wno-unused-function
//       -Wno-unknown-pragmas -x c++ tests/manual/gzlz_asan.cpp -o tests/emul/gzlz_asan -Ltests/emul -ltgsf_emul
//       -Wl,-rpath,'$ORIGIN'                                                                        (one command line)
//   tests/emul/gzlz_asan
//
//   - the code builder (gz_code_lengths, gz_code_entry), arithmetic only: Fibonacci and steeper-than-Fibonacci counts over 20 and
//     30 distance symbols and over 286 literal/length symbols, whose Huffman trees are far deeper than 15; no and one symbol in
//     use.  Every code: 15 bits at most, a Kraft sum of exactly 1, canonical and prefix-free.
//   - the geometry sweep: noise, then a copy of L bytes from D back, for the lengths and distances of tests/gzlzparity.py, the
//     copy beginning on, before and behind a multiple of 64 and of 1024, ending on the member's last byte, being a whole member;
//     a source 32769 back; one byte value; members of 1 .. 8 bytes and of MEMBER - 3 .. MEMBER.  The emulation's device memory
//     is host memory and the text a heap block of exactly its size: a match compared past the member's end, or a source in
//     front of its first byte, is a report.
// Every output goes back through the library's own inflate and CRC check and must give the text; the device form's bytes equal
// the host form's; no member is larger than at level 0.
// Exit status 0 and "gzlz ok": no difference, no error code, no sanitizer report (a report ends the program).
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
static int g_checked = 0, g_codes = 0;

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// exactly n bytes, 16-byte aligned (n == 0: one byte nobody may touch)
static uint8_t* exact(size_t n)
{
    void* p = nullptr;
    REQUIRE(posix_memalign(&p, 16, n ? n : 1) == 0, "out of memory");
    return (uint8_t*)p;
}

// ---- the code builder ----------------------------------------------------------------------------------------------------------
static void check_code(const std::vector<uint32_t>& hist, const char* what)
{
    const uint32_t n = (uint32_t)hist.size();
    std::vector<uint32_t> freq(n + 2), cnt(16, 0xA5A5A5A5u);
    std::vector<uint16_t> order(n + 2);
    std::vector<uint8_t> lens(n < 2 ? 2 : n, 0);
    tgsf::gz_code_lengths(hist.data(), n, freq.data(), order.data(), lens.data(), cnt.data());
    uint32_t used = 0, kraft = 0, deepest = 0;
    for (uint32_t s = 0; s < n; s++) used += hist[s] ? 1u : 0u;
    std::vector<uint32_t> code, bits;
    for (uint32_t s = 0; s < lens.size(); s++) {
        const uint32_t l = lens[s];
        REQUIRE(l <= 15, "%s: symbol %u has %u bits", what, s, l);
        REQUIRE(s >= n || used < 2 || (l != 0) == (hist[s] != 0), "%s: symbol %u, count %u, %u bits", what, s, s < n ? hist[s] : 0, l);
        if (!l) continue;
        kraft += 1u << (15 - l);
        deepest = l > deepest ? l : deepest;
        const uint32_t e = tgsf::gz_code_entry(lens.data(), cnt.data(), s);
        REQUIRE((e >> 16) == l, "%s: the entry's length", what);
        uint32_t c = 0;
        for (uint32_t k = 0; k < l; k++) c = c << 1 | ((e >> k) & 1u);                 // its first bit highest again
        code.push_back(c); bits.push_back(l);
    }
    REQUIRE(kraft == 32768u, "%s: the Kraft sum is %u / 32768", what, kraft);
    REQUIRE(used >= 2 || (code.size() == 2 && bits[0] == 1 && bits[1] == 1 && code[0] == 0 && code[1] == 1), "%s: two codes of one bit", what);
    for (size_t a = 0; a < code.size(); a++)
        for (size_t b = 0; b < code.size(); b++)
            REQUIRE(a == b || bits[a] > bits[b] || (code[b] >> (bits[b] - bits[a])) != code[a], "%s: code %zu is a prefix of code %zu", what, a, b);
    for (uint32_t l = 1; l < 16; l++) { uint32_t c = 0; for (uint32_t b : bits) c += b == l; REQUIRE(cnt[l] == c, "%s: cnt[%u]", what, l); }
    if (used > 16) REQUIRE(deepest == 15, "%s: the deepest code has %u bits", what, deepest);
    g_codes++;
}

static std::vector<uint32_t> fibonacci(uint32_t k, uint32_t step)       // step 0: f = f' + f''; 1: one more, every Huffman tree a chain
{
    std::vector<uint32_t> f = {1, 1};
    while (f.size() < k) f.push_back(f[f.size() - 1] + f[f.size() - 2] + step);
    f.resize(k);
    return f;
}

static void check_codes()
{
    for (uint32_t step : {0u, 1u})
        for (uint32_t k : {20u, 30u}) {
            std::vector<uint32_t> f = fibonacci(k, step);
            REQUIRE(f.back() < 1u << 23, "counts the builder's keys hold");
            check_code(f, "distance symbols, ascending");
            std::vector<uint32_t> r(f.rbegin(), f.rend());
            check_code(r, "distance symbols, descending");
            for (uint32_t i = 0; i + 1 < k; i += 3) r[i] = 0;                          // some not in use
            r.resize(30, 0);
            check_code(r, "distance symbols, some not in use");
        }
    for (uint32_t step : {0u, 1u}) {
        const std::vector<uint32_t> f = fibonacci(30, step);
        std::vector<uint32_t> h(286);
        for (uint32_t s = 0; s < 286; s++) h[s] = f[(s * 7) % 30];
        check_code(h, "286 literal/length symbols");
        for (uint32_t s = 0; s < 286; s++) h[s] = s < 256 ? (s % 5 ? 0 : f[(s / 5) % 24]) : f[s - 256];
        check_code(h, "286 literal/length symbols, the lengths the heaviest");
    }
    for (uint32_t one : {0u, 1u, 29u}) {
        std::vector<uint32_t> h(30, 0);
        check_code(h, "no distance in use");
        h[one] = 77;
        check_code(h, "one distance in use");
    }
    check_code({5, 0, 9}, "two symbols");
}

// ---- the geometry sweep --------------------------------------------------------------------------------------------------------
static tgsf_text* g_tx[2];               // level 0, level 1

static uint8_t noise_byte()              // all 256 values, the low ones often: a prefix code gains on them
{
    const uint32_t r = rnd(256), q = rnd(4);
    return (uint8_t)(q == 0 ? r : q == 1 ? r & 63 : r & 15);
}

static void add_copy(Bytes& t, size_t before, size_t length, size_t dist)
{
    REQUIRE(before >= dist && dist >= 1, "a copy from in front of the text");
    for (size_t i = 0; i < before; i++) t.push_back(noise_byte());
    if (dist > 1 && t[t.size() - 1] == t[t.size() - dist]) t[t.size() - dist] ^= 0x55;
    for (size_t i = 0; i < length; i++) t.push_back(t[t.size() - dist]);
}

// one text through both levels: the host form, the device form at exactly the room it needs and one byte short, and back
static void check(const Bytes& text, int eof, const char* what)
{
    const uint64_t n = text.size(), bound = tgsf_text_bgzf_bound(n, eof);
    const uint32_t members = (uint32_t)((n + TGSF_TEXT_BGZF_MEMBER - 1) / TGSF_TEXT_BGZF_MEMBER) + (eof ? 1u : 0u);
    std::vector<uint64_t> end0;
    for (int level = 0; level < 2; level++) {
        tgsf_text* tx = g_tx[level];
        Bytes host(bound + 1, 0xA5);
        std::vector<uint64_t> hend(members + 1, 0xA5A5A5A5A5A5A5A5ull);
        tgsf_text_gzout_summary hs;
        int rc = tgsf_text_bgzf_deflate(tx, text.data(), n, eof, host.data(), bound, hend.data(), &hs);
        REQUIRE(rc == TGSF_OK, "%s: deflate returned %d: %s", what, rc, tgsf_text_last_error(tx));
        REQUIRE(hs.in_bytes == n && hs.n_bytes <= bound && hs.n_members == members && hs.stop == TGSF_TEXT_END && hs.reserved == 0, "%s: summary", what);
        REQUIRE(host[hs.n_bytes] == 0xA5 && hend[members] == 0xA5A5A5A5A5A5A5A5ull, "%s: written behind the output", what);
        REQUIRE(members == 0 || hend[members - 1] == hs.n_bytes, "%s: member_end", what);
        if (level == 0) end0 = hend;
        else
            for (uint32_t m = 0; m < members; m++)
                REQUIRE(hend[m] - (m ? hend[m - 1] : 0) <= end0[m] - (m ? end0[m - 1] : 0), "%s: member %u is larger at level 1", what, m);
        // the device form: the text, the output and member_end in blocks of exactly their size
        uint8_t* d_in = exact(n);
        if (n) memcpy(d_in, text.data(), n);
        uint8_t* d_out = exact(hs.n_bytes);
        uint64_t* d_end = (uint64_t*)exact(8 * (size_t)members);
        tgsf_text_gzout_summary* d_sum = (tgsf_text_gzout_summary*)exact(sizeof(tgsf_text_gzout_summary));
        for (uint64_t cap : {hs.n_bytes, hs.n_bytes - 1}) {
            if (hs.n_bytes == 0 && cap != 0) continue;
            if (hs.n_bytes) memset(d_out, 0xA5, hs.n_bytes);
            rc = tgsf_text_bgzf_deflate_device(tx, d_in, n, eof, d_out, cap, d_end, d_sum, nullptr);
            REQUIRE(rc == TGSF_OK, "%s: deflate_device returned %d: %s", what, rc, tgsf_text_last_error(tx));
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
        rc = tgsf_text_bgzf_verify(tx, host.data(), hs.n_bytes, 1, &bad_block, &bad_crc);
        REQUIRE(rc == TGSF_OK && bad_block == 0xFFFFFFFFu && bad_crc == 0xFFFFFFFFu, "%s: verify returned %d (%u, %u): %s", what, rc, bad_block, bad_crc, tgsf_text_last_error(tx));
        Bytes back(n + 1, 0xA5);
        tgsf_text_bgzf_summary gs;
        rc = tgsf_text_bgzf_inflate(tx, host.data(), hs.n_bytes, 1, back.data(), n, &gs);
        REQUIRE(rc == TGSF_OK && gs.out_bytes == n && gs.n_blocks == members && gs.bad_block == 0xFFFFFFFFu, "%s: inflate returned %d: %s", what, rc, tgsf_text_last_error(tx));
        REQUIRE((n == 0 || memcmp(back.data(), text.data(), n) == 0) && back[n] == 0xA5, "%s: the round trip", what);
    }
    g_checked++;
}

int main()
{
    check_codes();
    const uint64_t M = TGSF_TEXT_BGZF_MEMBER, max_in = 2 * M + 64;
    for (int level = 0; level < 2; level++) {
        int rc = tgsf_text_create(0, max_in, 16, &g_tx[level]);
        REQUIRE(rc == TGSF_OK, "create: %s", tgsf_text_last_error(nullptr));
        REQUIRE(tgsf_text_bgzf_out_level_get(g_tx[level]) == 0, "the default level");
        REQUIRE(tgsf_text_bgzf_out_level(g_tx[level], 2) == TGSF_E_INVALID && tgsf_text_bgzf_out_level(g_tx[level], -1) == TGSF_E_INVALID, "levels -1 and 2");
        REQUIRE(tgsf_text_bgzf_out_level(g_tx[level], level) == TGSF_OK && tgsf_text_bgzf_out_level_get(g_tx[level]) == level, "out_level: %s", tgsf_text_last_error(g_tx[level]));
        REQUIRE(tgsf_text_bgzf_out_reserve(g_tx[level], max_in, tgsf_text_bgzf_bound(max_in, 1)) == TGSF_OK, "out_reserve: %s", tgsf_text_last_error(g_tx[level]));
        REQUIRE(tgsf_text_bgzf_out_level(g_tx[level], level) == TGSF_E_INVALID && tgsf_text_bgzf_out_level_get(g_tx[level]) == level, "a level after the reserve");
        REQUIRE(tgsf_text_bgzf_reserve(g_tx[level], tgsf_text_bgzf_bound(max_in, 1), 8) == TGSF_OK, "reserve: %s", tgsf_text_last_error(g_tx[level]));
    }
    REQUIRE(tgsf_text_bgzf_out_level(nullptr, 0) == TGSF_E_INVALID && tgsf_text_bgzf_out_level_get(nullptr) == TGSF_E_INVALID, "a null object");
    char what[128];
    const size_t lengths[] = {3, 4, 5, 10, 11, 12, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258, 259, 600};
    const size_t dists[] = {1, 2, 3, 4, 6, 12, 24, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1500, 4095, 4096, 4097, 12000, 32767, 32768};
    const size_t places[] = {192, 191, 193, 1024, 1023, 1025};
    int k = 0;
    for (size_t li = 0; li < sizeof lengths / sizeof *lengths; li++)
        for (size_t di = 0; di < sizeof dists / sizeof *dists; di++) {
            const size_t L = lengths[li], D = dists[di];
            if ((li + di) % 3 && L != 600 && L != 258 && D != 1 && D != 32768) continue;             // a third of the grid, and its edges whole
            Bytes t;
            const size_t reps = D <= 1024 ? 3 : 1, place = places[k++ % 6];
            for (size_t r = 0; r < reps; r++) { const size_t b = D < 8 ? 8 : D; add_copy(t, b + (place + 2048 - (t.size() + b) % 1024) % 1024, L, D); }
            for (int i = 0; i < k % 3; i++) t.push_back(noise_byte());
            snprintf(what, sizeof what, "copy of %zu from %zu back at %zu", L, D, place);
            check(t, k & 1, what);
        }
    for (size_t L : {(size_t)3, (size_t)4, (size_t)19, (size_t)131, (size_t)258, (size_t)259, (size_t)600})
        for (size_t D : {(size_t)1, (size_t)4, (size_t)64, (size_t)4097, (size_t)32768}) {
            Bytes t;
            add_copy(t, M - L, L, D);                                                             // ends on the member's last byte
            snprintf(what, sizeof what, "copy of %zu from %zu back to the member's end", L, D);
            check(t, 0, what);
            if (L != 600) continue;
            t.clear();
            add_copy(t, M, L, D);                                                                 // a whole member behind one of noise
            snprintf(what, sizeof what, "copy of %zu from %zu back as a whole member", L, D);
            check(t, 1, what);
        }
    { Bytes t; add_copy(t, 32769, 600, 32769); for (int i = 0; i < 50; i++) t.push_back(noise_byte()); check(t, 1, "the only source 32769 back"); }
    { Bytes t; add_copy(t, M, M, 64); check(t, 1, "a member of period 64 behind a member of noise"); }
    check(Bytes(M, (uint8_t)'~'), 1, "one byte value");
    check(Bytes(2 * M + 1, (uint8_t)'~'), 0, "one byte value, two members and a byte");
    Bytes period;
    for (size_t i = 0; i < 1000; i++) period.push_back(noise_byte());
    { Bytes t; while (t.size() < 2 * M + 1) t.push_back(period[t.size() % 1000]); check(t, 1, "period 1000 across two cuts"); }
    Bytes noise;
    for (size_t i = 0; i < M + 8; i++) noise.push_back(noise_byte());
    for (size_t n = 0; n <= 8; n++) {
        snprintf(what, sizeof what, "members of %zu bytes", n);
        check(Bytes(noise.begin(), noise.begin() + n), (int)(n & 1), what);
        check(Bytes(n, (uint8_t)'A'), (int)(~n & 1), what);
        check(Bytes(noise.begin(), noise.begin() + M + n), 1, what);
        if (n < 4) check(Bytes(noise.begin(), noise.begin() + M - n), 0, what);
    }
    for (int level = 0; level < 2; level++) tgsf_text_destroy(g_tx[level]);
    printf("gzlz ok: %d codes, %d texts\n", g_codes, g_checked);
    return 0;
}
