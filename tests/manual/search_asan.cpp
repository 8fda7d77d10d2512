// TEST INFRASTRUCTURE: tgsf_create plus one small batch over the accepted corners of the adapter search's parameters, and
// tgsf_create alone for the refused ones, through the serial emulation of the kernels built with the host compiler's address
// and undefined-behaviour sanitizers and -fsanitize=float-cast-overflow, which GCC's `undefined` group leaves out
// (tests/emul/Makefile, target search_asan: this file includes the library's source, compiled with -DTGSF_EMUL, so the whole
// is one host program).
//
// What the bounds of include/tgsf.h are there for: k_gate_reads forms L - 2 * end_len, k_mid_resolve pos + end_len + 1 +
// extra_len in 32 signed bits, and adapter_rules converts Q / end_sim to an int.  Accepted and run: end_len 0 and 2^28,
// extra_len 2^28, end_sim 1e-30 and +inf, match lengths of INT_MAX, a set of 32 adapters of 1..256 bp.  Refused in front of
// the device: end_len and extra_len of 2^28 + 1, 1 500 000 000 and INT_MAX.  Should a library accept one of those, its batch
// is run as well: the sanitizer then says where.
// Exit status 0 and "search ok": no error code, no sanitizer report (a report ends the program).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tgsf.h"
#include "../../tgsfilter_amd/csrc/tgsf_lib.hip"      // (TGSF_EMUL: the kernels as serial host code)

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t rnd(uint32_t n)           // a fixed linear-congruential generator (Knuth's MMIX constants)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

static std::string random_bases(uint32_t n)
{
    std::string s(n, 'A');
    for (uint32_t k = 0; k < n; k++) s[k] = "ACGT"[rnd(4)];
    return s;
}

struct Batch {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint8_t *seq = nullptr, *qual = nullptr;
    uint64_t total = 0, bases = 0;
    uint32_t longest = 0;
    // reads of the given lengths; read i carries adapter i % n at its 5' end, its 3' end or its middle (i % 3) where it fits
    Batch(const std::vector<uint32_t>& lens, const std::vector<std::string>& ads)
    {
        for (uint32_t L : lens) { off.push_back(total); len.push_back(L); total += (L + 15u) / 16u * 16u; bases += L; longest = L > longest ? L : longest; }
        // 16-byte aligned, exactly the padded span long: a byte read or written behind it is a report
        seq = (uint8_t*)aligned_alloc(16, total);
        qual = (uint8_t*)aligned_alloc(16, total);
        memset(seq, 0, total); memset(qual, 0, total);
        for (size_t i = 0; i < len.size(); i++) {
            for (uint32_t k = 0; k < len[i]; k++) { seq[off[i] + k] = (uint8_t)"ACGT"[rnd(4)]; qual[off[i] + k] = (uint8_t)(33 + 25 + rnd(15)); }
            const std::string& a = ads[i % ads.size()];
            if (a.size() + 8 > len[i]) continue;
            const uint32_t at = i % 3 == 0 ? 3 : i % 3 == 1 ? len[i] - (uint32_t)a.size() - 2 : (len[i] - (uint32_t)a.size()) / 2;
            memcpy(seq + off[i] + at, a.data(), a.size());
        }
    }
    ~Batch() { free(seq); free(qual); }
};

static tgsf_params params(const Batch& b, const std::vector<std::string>& ads)
{
    tgsf_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.min_len = 50; p.max_len = INT_MAX; p.min_q = 7.f; p.max_q = 255.f; p.bc_len = 150;
    p.end_len = 150; p.end_match_len = 4; p.mid_match_len = 35; p.extra_len = 50;
    p.end_sim = 0.75f; p.mid_sim = 0.9f; p.filter = 1; p.qtype = 33; p.kmer = 11;
    p.n_adapters = (int)ads.size();
    for (size_t a = 0; a < ads.size(); a++) { p.adapters[a] = ads[a].data(); p.adapter_len[a] = (int)ads[a].size(); }
    p.max_batch_bases = b.bases + 64; p.max_batch_reads = (uint32_t)b.len.size(); p.max_read_len = b.longest;
    return p;
}

// one batch through a context; returns the number of reads with an adapter flag, or -1
static int submit(tgsf_ctx* c, const Batch& b)
{
    const uint32_t n = (uint32_t)b.len.size();
    std::vector<tgsf_read_result> res(n);
    std::vector<tgsf_fragment> fr(4096);
    tgsf_batch_in in;
    memset(&in, 0, sizeof in);
    in.seq = b.seq; in.qual = b.qual; in.offsets = b.off.data(); in.lengths = b.len.data(); in.n_reads = n; in.n_bytes = b.total;
    tgsf_batch_out out = {res.data(), fr.data(), (uint32_t)fr.size(), 0};
    const int rc = tgsf_submit(c, &in, &out);
    if (rc != TGSF_OK) { fprintf(stderr, "tgsf_submit: status %d: %s\n", rc, tgsf_last_error(c)); return -1; }
    for (uint32_t f = 0; f < out.n_frags; f++)
        if (fr[f].start < 0 || fr[f].len < 0 || (uint32_t)fr[f].start + (uint32_t)fr[f].len > b.len[fr[f].read]) { fprintf(stderr, "fragment %u outside its read\n", f); return -1; }
    int hits = 0;
    for (uint32_t r = 0; r < n; r++) hits += (res[r].flags & (TGSF_RF_AD5P | TGSF_RF_AD3P | TGSF_RF_ADMID)) != 0;
    return hits;
}

static int run(const char* what, tgsf_params p, const Batch& b, int min_hits, int max_hits)
{
    tgsf_ctx* c = nullptr;
    if (tgsf_create(&p, 0, &c) != TGSF_OK) { fprintf(stderr, "%s: tgsf_create refused: %s\n", what, tgsf_last_error(nullptr)); return 1; }
    const int hits = submit(c, b);
    tgsf_destroy(c);
    printf("%s: %d reads with an adapter\n", what, hits);
    if (hits < min_hits || hits > max_hits) { fprintf(stderr, "%s: %d reads with an adapter, expected %d..%d\n", what, hits, min_hits, max_hits); return 1; }
    return 0;
}

int main()
{
    const std::vector<std::string> two = {"GTTTTCGCATTTATCGTGAAACGCTTTCGCGTTTTTCGTGCGCCGCTTCA", "AATGTACTTCGTTCAGTTACGTATTGCT"};
    std::vector<std::string> many;
    static const uint32_t lens32[32] = {1, 2, 4, 5, 22, 28, 31, 32, 33, 40, 45, 50, 63, 64, 65, 90, 127, 128, 129, 150, 192, 193, 230, 256, 24, 36, 48, 60, 72, 30, 34, 66};
    for (uint32_t L : lens32) many.push_back(random_bases(L));
    std::vector<uint32_t> lens = {1, 2, 4, 5, 7, 27, 28, 29, 56, 57, 99, 100, 101, 150, 299, 300, 301, 350, 600, 1000};
    for (int k = 0; k < 44; k++) lens.push_back(300 + rnd(700));
    const Batch b(lens, two), b32(lens, many);
    const int n = (int)lens.size();
    int bad = 0;
    { tgsf_params p = params(b, two); bad |= run("defaults", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.end_len = 0; bad |= run("end_len 0", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.end_len = 1 << 28; bad |= run("end_len 2^28", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.extra_len = 1 << 28; bad |= run("extra_len 2^28", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.end_len = 1 << 28; p.extra_len = 1 << 28; bad |= run("both 2^28", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.end_sim = 1e-30f; bad |= run("end_sim 1e-30", p, b, 20, n); }
    { tgsf_params p = params(b, two); p.end_sim = INFINITY; p.end_len = 0; p.mid_match_len = 20; bad |= run("end_sim inf", p, b, 1, n); }
    { tgsf_params p = params(b, two); p.end_match_len = INT_MAX; p.mid_match_len = INT_MAX; bad |= run("match lengths INT_MAX", p, b, 0, 0); }
    { tgsf_params p = params(b32, many); p.mid_match_len = 20; bad |= run("32 adapters", p, b32, 20, n); }
    for (int field = 0; field < 2; field++)
        for (int v : {(1 << 28) + 1, 1500000000, INT_MAX}) {
            tgsf_params p = params(b, two);
            (field ? p.extra_len : p.end_len) = v;
            tgsf_ctx* c = (tgsf_ctx*)0x1;
            const int rc = tgsf_create(&p, 0, &c);
            const char* name = field ? "extra_len (-T)" : "end_len (-E)";
            if (rc != TGSF_E_INVALID || c != nullptr || !strstr(tgsf_last_error(nullptr), name)) {
                fprintf(stderr, "tgsf_create(%s %d): status %d (%s), expected TGSF_E_INVALID naming the field\n", name, v, rc, rc ? tgsf_last_error(nullptr) : "accepted");
                bad = 1;
                if (rc == TGSF_OK && c) { (void)submit(c, b); tgsf_destroy(c); }
            }
        }
    if (bad) return 1;
    printf("search ok\n");
    return 0;
}
