// TEST INFRASTRUCTURE: tgsf_create plus one batch over the corners of the quality thresholds and of bc_len, through the serial
// emulation of the kernels built with the host compiler's address and undefined-behaviour sanitizers and
// -fsanitize=float-cast-overflow, which GCC's `undefined` group leaves out (tests/emul/Makefile, target quality_asan: this
// file includes the library's source, compiled with -DTGSF_EMUL, so the whole is one host program).
//
// What could go wrong: k_gate_reads and k_gate_frags index a histogram of 256 words with (int)mean, behind a gate whose
// thresholds are any float at all -- NaN, the infinities, -1, -0.0, min_q above max_q: tgsf_create refuses none --, and
// k_end_tables tallies bc_len positions in slabs of 512, 64 to a slot, into tables sized by bc_len.  Here: reads with means of
// 0, 7.5 (exactly), 93 and 94, one with quality bytes of 128 and above, reads of 1, 63, 64, 65, 511, 512, 513 and 1100 bases,
// under each threshold corner with fixed trims (the gate after the split; the by-product forced as well) and under bc_len of
// 0, 1, 63, 64, 65, 512, 513 and 2^20 (with a read of 2^20 + 1 bases), with qualities and without.  A gate that cannot fail
// keeps every read, one that cannot pass keeps none: checked.
// Exit status 0 and "quality ok": no error code, no sanitizer report (a report ends the program).
// `quality_asan quick` leaves bc_len 2^20 out: its 4 096 launches of k_end_tables take the serial emulation eight minutes
// without the sanitizers and twenty with them (the suite runs `quick`; run the whole by hand).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/tgsf.h"
#include "../../tgsfilter_amd/csrc/tgsf_lib.hip"      // (TGSF_EMUL: the kernels as serial host code)

static uint64_t g_state = 0x452821E638D01377ull;
static uint32_t rnd(uint32_t n)           // a fixed linear-congruential generator (Knuth's MMIX constants)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

struct Batch {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint8_t *seq = nullptr, *qual = nullptr;
    uint64_t total = 0, bases = 0;
    uint32_t longest = 0;
    // read i has, by i % 6, a quality value of 0 throughout, 7 and 8 in turn (a mean of 7.5 where the length is even), 93, 94,
    // 90 with every 40th byte of 128 and above, or a drawn one
    explicit Batch(const std::vector<uint32_t>& lens)
    {
        for (uint32_t L : lens) { off.push_back(total); len.push_back(L); total += (L + 15u) / 16u * 16u; bases += L; longest = L > longest ? L : longest; }
        // 16-byte aligned, exactly the padded span long: a byte read or written behind it is a report
        seq = (uint8_t*)aligned_alloc(16, total);
        qual = (uint8_t*)aligned_alloc(16, total);
        memset(seq, 0, total); memset(qual, 0, total);
        for (size_t i = 0; i < len.size(); i++)
            for (uint32_t k = 0; k < len[i]; k++) {
                seq[off[i] + k] = (uint8_t)"ACGTgt"[rnd(6)];
                uint32_t q;
                switch (i % 6) {
                case 0: q = 0; break;
                case 1: q = 7 + (k & 1u); break;
                case 2: q = 93; break;
                case 3: q = 94; break;
                case 4: q = (k % 40u == 39u) ? 95 + rnd(128) : 90; break;
                default: q = 5 + rnd(30);
                }
                qual[off[i] + k] = (uint8_t)(33 + q);
            }
    }
    ~Batch() { free(seq); free(qual); }
};

static tgsf_params params(const Batch& b, float min_q, float max_q, int bc_len, int head, int tail, int no_qual)
{
    tgsf_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.min_len = 1; p.max_len = INT_MAX; p.min_q = min_q; p.max_q = max_q; p.bc_len = bc_len;
    p.head_trim = head; p.tail_trim = tail;
    p.end_len = 150; p.end_match_len = 4; p.mid_match_len = 35; p.extra_len = 50;
    p.end_sim = 0.75f; p.mid_sim = 0.9f; p.filter = 1; p.qtype = 33; p.kmer = 11; p.no_qual = no_qual;
    p.max_batch_bases = b.bases + 64; p.max_batch_reads = (uint32_t)b.len.size(); p.max_read_len = b.longest;
    return p;
}

// create, one batch, the tallies; returns the number of reads with a kept fragment, or -1
static int run(const char* what, tgsf_params p, const Batch& b)
{
    tgsf_ctx* c = nullptr;
    if (tgsf_create(&p, 0, &c) != TGSF_OK) { fprintf(stderr, "%s: tgsf_create refused: %s\n", what, tgsf_last_error(nullptr)); return -1; }
    const uint32_t n = (uint32_t)b.len.size();
    std::vector<tgsf_read_result> res(n);
    std::vector<tgsf_fragment> fr(n + 16);
    tgsf_batch_in in;
    memset(&in, 0, sizeof in);
    in.seq = b.seq; in.qual = b.qual; in.offsets = b.off.data(); in.lengths = b.len.data(); in.n_reads = n; in.n_bytes = b.total;
    tgsf_batch_out out = {res.data(), fr.data(), (uint32_t)fr.size(), 0};
    int kept = -1;
    uint64_t nw = 0; int32_t bc = 0; uint32_t nb = 0;
    const int rc = tgsf_submit(c, &in, &out);
    if (rc != TGSF_OK) fprintf(stderr, "%s: tgsf_submit: status %d: %s\n", what, rc, tgsf_last_error(c));
    else if (tgsf_counters_len(c, &nw, &bc, &nb) != TGSF_OK || bc != p.bc_len) fprintf(stderr, "%s: tgsf_counters_len\n", what);
    else {
        std::vector<uint64_t> ctr(nw);
        if (tgsf_counters(c, ctr.data(), nw) != TGSF_OK) fprintf(stderr, "%s: tgsf_counters: %s\n", what, tgsf_last_error(c));
        else {
            kept = 0;
            for (uint32_t f = 0; f < out.n_frags; f++) kept += (fr[f].flags & TGSF_FF_PASS) != 0;
            uint64_t raw = 0, want = 0;                               // every read with qualities is in the raw histogram, once
            for (int k = 0; k < TGSF_N_QBINS; k++) raw += ctr[TGSF_CTR_RAW_DIFFQ + k];
            if (!p.no_qual) want = b.bases;
            if (raw != want) { fprintf(stderr, "%s: the raw histogram holds %llu bases of %llu\n", what, (unsigned long long)raw, (unsigned long long)want); kept = -1; }
            const uint64_t rows = ctr[TGSF_CTR_ROWS + 2], most = (uint64_t)p.bc_len < b.longest ? (uint64_t)p.bc_len : b.longest;
            if (rows != most) { fprintf(stderr, "%s: %llu rows of the end tables in use, expected %llu\n", what, (unsigned long long)rows, (unsigned long long)most); kept = -1; }
        }
    }
    tgsf_destroy(c);
    printf("%s: %d reads kept\n", what, kept);
    return kept;
}

int main(int argc, char** argv)
{
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    setenv("TGSF_DEBUG_KNOBS", "1", 1);                               // the library reads TGSF_CLEAN_TABLES only under this switch
    const Batch b({1, 2, 63, 64, 65, 100, 511, 512, 513, 1100, 1024, 1025, 700, 6400, 6401, 12, 99, 300});
    const int n = (int)b.len.size();
    struct Corner { const char* what; float min_q, max_q; int least, most; };
    const float nan = NAN, inf = INFINITY;
    const Corner corners[] = {
        {"min_q NaN", nan, 255.f, n, n}, {"max_q NaN", 0.f, nan, n, n}, {"both NaN", nan, nan, n, n},
        {"min_q -inf", -inf, 255.f, n, n}, {"max_q +inf", 0.f, inf, n, n}, {"min_q +inf", inf, 255.f, 0, 0}, {"max_q -inf", 0.f, -inf, 0, 0},
        {"min_q -1", -1.f, 255.f, n, n}, {"min_q -0.0", -0.f, 255.f, n, n}, {"max_q -1", 0.f, -1.f, 0, 0}, {"max_q -0.0", 0.f, -0.f, 1, n / 2},
        {"min_q 12.25 > max_q 7.5", 12.25f, 7.5f, 0, 0}, {"min_q 7.5 == max_q", 7.5f, 7.5f, 1, n / 2}, {"min_q 0, max_q 94", 0.f, 94.f, n, n},
    };
    int bad = 0;
    for (int strategy = 0; strategy < 2; strategy++) {
        if (strategy) setenv("TGSF_CLEAN_TABLES", "byproduct", 1); else unsetenv("TGSF_CLEAN_TABLES");
        for (const Corner& k : corners)
            for (int trims = 0; trims < 2; trims++) {
                // (under trims of 1 / 1 the reads of 1 and 2 bases keep nothing, whatever the gate; the mean of what is kept of the others is the read's)
                const int gone = trims ? 2 : 0;
                const int kept = run(k.what, params(b, k.min_q, k.max_q, 150, trims, trims, 0), b);
                const int least = k.least == n ? n - gone : k.least > gone ? k.least - gone : 0;
                if (kept < least || kept > k.most) { fprintf(stderr, "%s (trims %d, strategy %d): %d reads kept, expected %d..%d\n", k.what, trims, strategy, kept, least, k.most); bad = 1; }
            }
    }
    unsetenv("TGSF_CLEAN_TABLES");
    for (int bc : {0, 1, 63, 64, 65, 512, 513})
        for (int no_qual = 0; no_qual < 2; no_qual++) {
            char what[64];
            snprintf(what, sizeof what, "bc_len %d%s", bc, no_qual ? ", no qualities" : "");
            if (run(what, params(b, 0.f, 255.f, bc, 0, 0, no_qual), b) != n) bad = 1;
        }
    if (!quick) {
        const Batch wide({513, (1u << 20) + 1u, 64});
        if (run("bc_len 2^20", params(wide, 0.f, 255.f, 1 << 20, 0, 0, 0), wide) != 3) bad = 1;
    }
    if (bad) return 1;
    printf(quick ? "quality ok (without bc_len 2^20)\n" : "quality ok\n");
    return 0;
}
