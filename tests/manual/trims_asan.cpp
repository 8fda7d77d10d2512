// TEST INFRASTRUCTURE: tgsf_create plus one batch over the corners of min_len, max_len and the fixed trims, through the
// serial emulation of the kernels built with the host compiler's address and undefined-behaviour sanitizers
// (tests/emul/Makefile, target trims_asan: this file includes the library's source, compiled with -DTGSF_EMUL, so the whole
// is one host program).
//
// With a fixed trim k_prepare speculates that a read is kept as [head_trim, L - tail_trim) when that range has a length
// the filters accept; stats_item_len, held_range and k_tail_fix then form L - tail_trim in 32 unsigned bits.  That is sound
// only while `keep >= min_len` implies keep >= 0: tgsf_create refuses min_len < 0.  Here: reads of 3, 2000, 4, 1500, 7, 12,
// 13, 6400 and 6500 bp (shorter than a trim, than both, exactly a tile, a tile and a bin), 16-byte padded, for every
// combination of min_len in {0, 1, 100, INT32_MAX}, max_len in {-1, 0, 1, INT32_MAX}, either trim in {0, 5, 2000, INT32_MAX}
// and both strategies (the context's own decisions; TGSF_CLEAN_TABLES=byproduct) -- and the refusal of min_len = -1.  Should a
// library accept that, its batch is run as well: the sanitizer then says where.
// Exit status 0 and "trims ok": no error code, no sanitizer report (a report ends the program).
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/tgsf.h"
#include "../../tgsfilter_amd/csrc/tgsf_lib.hip"      // (TGSF_EMUL: the kernels as serial host code)

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n)           // a fixed linear-congruential generator (Knuth's MMIX constants)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

static const char kAdapter[] = "GTTTTCGCATTTATCGTGAAACGCTTTCGCGTTTTTCGTGCGCCGCTTCA";
static const std::vector<uint32_t> kSeven = {3, 2000, 4, 1500, 7, 12, 13};
static const std::vector<uint32_t> kNine = {3, 2000, 4, 1500, 7, 12, 13, 6400, 6500};

struct Batch {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint8_t *seq = nullptr, *qual = nullptr;
    uint64_t total = 0, bases = 0;
    uint32_t longest = 0;
    explicit Batch(const std::vector<uint32_t>& lens)
    {
        for (uint32_t L : lens) { off.push_back(total); len.push_back(L); total += (L + 15u) / 16u * 16u; bases += L; longest = L > longest ? L : longest; }
        // 16-byte aligned, exactly the padded span long: a byte read or written behind it is a report
        seq = (uint8_t*)aligned_alloc(16, total);
        qual = (uint8_t*)aligned_alloc(16, total);
        memset(seq, 0, total); memset(qual, 0, total);
        for (size_t i = 0; i < len.size(); i++)
            for (uint32_t k = 0; k < len[i]; k++) { seq[off[i] + k] = (uint8_t)"ACGT"[rnd(4)]; qual[off[i] + k] = (uint8_t)(33 + 25 + rnd(15)); }
    }
    ~Batch() { free(seq); free(qual); }
};

// (sized as tightly as a caller may: the batch's own bases, reads and longest read)
static tgsf_params params(const Batch& b, int min_len, int max_len, int head, int tail)
{
    tgsf_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.min_len = min_len; p.max_len = max_len; p.min_q = 7.f; p.max_q = 255.f; p.bc_len = 150;
    p.head_trim = head; p.tail_trim = tail;
    p.end_len = 150; p.end_match_len = 4; p.mid_match_len = 35; p.extra_len = 50;
    p.end_sim = 0.75f; p.mid_sim = 0.9f; p.filter = 1; p.qtype = 33; p.kmer = 11;
    p.n_adapters = 1; p.adapters[0] = kAdapter; p.adapter_len[0] = (int)strlen(kAdapter);
    p.max_batch_bases = b.bases + 64; p.max_batch_reads = (uint32_t)b.len.size(); p.max_read_len = b.longest;
    return p;
}

// one batch through a context; returns the bases kept, or -1
static long long submit(tgsf_ctx* c, const Batch& b)
{
    const uint32_t n = (uint32_t)b.len.size();
    std::vector<tgsf_read_result> res(n);
    std::vector<tgsf_fragment> fr(512);
    tgsf_batch_in in;
    memset(&in, 0, sizeof in);
    in.seq = b.seq; in.qual = b.qual; in.offsets = b.off.data(); in.lengths = b.len.data(); in.n_reads = n; in.n_bytes = b.total;
    tgsf_batch_out out = {res.data(), fr.data(), (uint32_t)fr.size(), 0};
    const int rc = tgsf_submit(c, &in, &out);
    if (rc != TGSF_OK) { fprintf(stderr, "tgsf_submit: status %d: %s\n", rc, tgsf_last_error(c)); return -1; }
    std::vector<uint64_t> ctr;
    uint64_t nw = 0; int32_t bc = 0; uint32_t nb = 0;
    if (tgsf_counters_len(c, &nw, &bc, &nb) != TGSF_OK) return -1;
    ctr.resize(nw);
    if (tgsf_counters(c, ctr.data(), nw) != TGSF_OK) { fprintf(stderr, "tgsf_counters: %s\n", tgsf_last_error(c)); return -1; }
    long long kept = 0;
    for (uint32_t f = 0; f < out.n_frags; f++) {
        if (fr[f].start < 0 || fr[f].len < 0 || (uint32_t)fr[f].start + (uint32_t)fr[f].len > b.len[fr[f].read]) { fprintf(stderr, "fragment %u outside its read\n", f); return -1; }
        if (fr[f].flags & TGSF_FF_PASS) kept += fr[f].len;
    }
    return kept;
}

int main()
{
    setenv("TGSF_DEBUG_KNOBS", "1", 1);                               // the library reads TGSF_CLEAN_TABLES only under this switch
    const Batch b(kNine), seven(kSeven);
    static const int min_lens[4] = {0, 1, 100, INT_MAX}, max_lens[4] = {-1, 0, 1, INT_MAX}, trims[4] = {0, 5, 2000, INT_MAX};
    int bad = 0, runs = 0;
    for (int strategy = 0; strategy < 2; strategy++) {
        if (strategy) setenv("TGSF_CLEAN_TABLES", "byproduct", 1); else unsetenv("TGSF_CLEAN_TABLES");
        // both strategies must keep the same bases: nothing of a result depends on a guess.  (The contexts of a strategy run side
        // by side on the host's threads -- the emulation keeps a lane's state per thread --: a batch takes a third of a second here.)
        static long long kept_default[256];
        std::atomic<int> next(0), failed(0), done(0);
        auto work = [&] {
            for (int i = next++; i < 256; i = next++) {
                const int a = i >> 6, m = (i >> 4) & 3, h = (i >> 2) & 3, t = i & 3;
                tgsf_params p = params(b, min_lens[a], max_lens[m], trims[h], trims[t]);
                tgsf_ctx* c = nullptr;
                if (tgsf_create(&p, 0, &c) != TGSF_OK) {
                    fprintf(stderr, "tgsf_create(min_len %d, max_len %d, trims %d / %d) refused\n", p.min_len, p.max_len, p.head_trim, p.tail_trim);
                    failed = 1;
                    continue;
                }
                const long long kept = submit(c, b);
                tgsf_destroy(c);
                done++;
                if (kept < 0) { fprintf(stderr, "  ... with min_len %d, max_len %d, trims %d / %d, strategy %d\n", p.min_len, p.max_len, p.head_trim, p.tail_trim, strategy); failed = 1; continue; }
                if (!strategy) kept_default[i] = kept;
                else if (kept != kept_default[i]) {
                    fprintf(stderr, "min_len %d, max_len %d, trims %d / %d: %lld bases kept by default, %lld as a by-product\n", p.min_len, p.max_len, p.head_trim, p.tail_trim, kept_default[i], kept);
                    failed = 1;
                }
                // (a fragment of more than max_len bases is not kept: below 1 that is every base)
                if (max_lens[m] < 1 && kept != 0) { fprintf(stderr, "max_len %d kept %lld bases\n", p.max_len, kept); failed = 1; }
            }
        };
        unsigned nt = std::thread::hardware_concurrency();
        nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
        std::vector<std::thread> pool;
        for (unsigned k = 1; k < nt; k++) pool.emplace_back(work);
        work();
        for (std::thread& th : pool) th.join();
        bad |= failed;
        runs += done;
        // min_len below 0: refused in front of the device, for either strategy -- the reads and parameters the out-of-bounds write was found with
        for (int min_len : {-1, -5, INT_MIN}) {
            tgsf_params p = params(seven, min_len, INT_MAX, 0, 5);
            tgsf_ctx* c = (tgsf_ctx*)0x1;
            const int rc = tgsf_create(&p, 0, &c);
            if (rc != TGSF_E_INVALID || c != nullptr || !strstr(tgsf_last_error(nullptr), "min_len")) {
                fprintf(stderr, "tgsf_create(min_len %d): status %d (%s), expected TGSF_E_INVALID naming min_len\n", min_len, rc, rc ? tgsf_last_error(nullptr) : "accepted");
                bad = 1;
                if (rc == TGSF_OK && c) { (void)submit(c, seven); tgsf_destroy(c); }
            }
        }
    }
    unsetenv("TGSF_CLEAN_TABLES");
    if (bad) return 1;
    printf("%d contexts, one batch each\ntrims ok\n", runs);
    return 0;
}
