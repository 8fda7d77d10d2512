// TEST INFRASTRUCTURE: the largest batch a context accepts, through the serial emulation of the kernels built with
// the host compiler's address and undefined-behaviour sanitizers (tests/emul/Makefile, target largest_batch_asan: this file
// includes the library's source, compiled with -DTGSF_EMUL, so the whole is one host program).
//
// tgsf_submit_device accepts a span of max_batch_bases + 16 * max_batch_reads bytes.  Every buffer of a context that is
// sized by chunks or bases must hold a batch that uses that span to the last byte: 2 048 unaligned reads of 33..81 bases
// packed end to end, every byte a base, so that every read has a middle window and the chunks per base are at their
// worst.  Through tgsf_submit and tgsf_submit_device (the emulation's device memory is host memory), with the flat scan
// and with TGSF_MID_FLAT=0, with the 22-bp ligation adapters at -M 14 (the one-dword column) and with the PacBio blunt
// adapters (the 32-row filter: its mark and recheck buffers; and with four 33-bp adapters at -M 30, four
// filtered adapters in one pass: the marks of the fourth lie last in their buffer).  One byte more must come back
// TGSF_E_CAPACITY.
// Exit status 0 and "largest batch ok": no error code, no sanitizer report (a report ends the program).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/tgsf.h"
#include "../../tgsfilter_amd/csrc/tgsf_lib.hip"      // (TGSF_EMUL: the kernels as serial host code)

static const uint64_t kSeed = 0x243F6A8885A308D3ull;
static uint64_t g_state = kSeed;
static uint32_t rnd(uint32_t n)           // a fixed linear-congruential generator (Knuth's MMIX constants)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

static const uint32_t kReads = 2048;
static const uint64_t kBases = 2048 * 40;

static int check(tgsf_ctx* c, int rc, int want, const char* what)
{
    if (rc == want) return 0;
    fprintf(stderr, "%s: status %d, expected %d: %s\n", what, rc, want, tgsf_last_error(c));
    return 1;
}

static int run(const char* const* adapters, int n_adapters, int mid_match_len, const char* mid_flat)
{
    if (mid_flat) setenv("TGSF_MID_FLAT", mid_flat, 1); else unsetenv("TGSF_MID_FLAT");
    g_state = kSeed;                                                  // every run builds the same lengths and bases
    tgsf_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    p.min_len = 100; p.max_len = 2147483647; p.min_q = 7.f; p.max_q = 255.f; p.bc_len = 150;
    p.end_len = 0; p.end_match_len = 4; p.mid_match_len = mid_match_len; p.extra_len = 50;
    p.end_sim = 0.75f; p.mid_sim = 0.9f; p.filter = 1; p.qtype = 33; p.kmer = 11;
    p.n_adapters = n_adapters;
    for (int a = 0; a < n_adapters; a++) { p.adapters[a] = adapters[a]; p.adapter_len[a] = (int)strlen(adapters[a]); }
    p.max_batch_bases = kBases; p.max_batch_reads = kReads; p.max_read_len = 4096;

    const uint64_t total = kBases + 16ull * kReads;
    // lengths of 16 m + 1 bases: one base in the last chunk of every window, (n_bytes + 15 n_reads) / 16 chunks in all --
    // no batch of this span and this many reads has more.  256 x 33, 896 x 49, 640 x 65, 256 x 81 = 114 688 bases, shuffled.
    std::vector<uint32_t> len;
    for (uint32_t i = 0; i < kReads; i++) len.push_back(i < 256 ? 33 : i < 1152 ? 49 : i < 1792 ? 65 : 81);
    for (uint32_t i = kReads - 1; i > 0; i--) { const uint32_t j = rnd(i + 1), t = len[i]; len[i] = len[j]; len[j] = t; }
    uint64_t sum = 0;
    for (uint32_t i = 0; i < kReads; i++) sum += len[i];
    if (sum != total) { fprintf(stderr, "the lengths add up to %llu\n", (unsigned long long)sum); return 1; }
    std::vector<uint64_t> off(kReads + 1, 0);
    for (uint32_t i = 0; i < kReads; i++) off[i + 1] = off[i] + len[i];
    // 16-byte aligned, exactly `total` bytes long: a byte read or written behind the span is a report
    uint8_t* seq = (uint8_t*)aligned_alloc(16, total);
    uint8_t* qual = (uint8_t*)aligned_alloc(16, total);
    for (uint64_t i = 0; i < total; i++) { seq[i] = (uint8_t)"ACGT"[rnd(4)]; qual[i] = (uint8_t)(33 + 8 + rnd(32)); }
    for (uint32_t i = 0; i < kReads; i += 3) {                        // an adapter (or its head) in a third of the reads
        const char* a = adapters[(i / 3) % n_adapters];
        const uint32_t q = (uint32_t)strlen(a), n = q < len[i] ? q : len[i];
        memcpy(seq + off[i] + rnd(len[i] - n + 1), a, n);
    }

    int bad = 0;
    tgsf_ctx* c = nullptr;
    if (tgsf_create(&p, 0, &c) != TGSF_OK) { fprintf(stderr, "tgsf_create: %s\n", tgsf_last_error(nullptr)); return 1; }
    const uint32_t fcap = 4096;
    std::vector<tgsf_read_result> r1(kReads), r2(kReads);
    std::vector<tgsf_fragment> f1(fcap), f2(fcap);
    uint32_t* nf2 = (uint32_t*)aligned_alloc(16, 16);
    tgsf_batch_in in;
    memset(&in, 0, sizeof in);
    in.seq = seq; in.qual = qual; in.offsets = off.data(); in.lengths = nullptr; in.n_reads = kReads; in.n_bytes = total;
    tgsf_batch_out o1 = {r1.data(), f1.data(), fcap, 0}, o2 = {r2.data(), f2.data(), fcap, 0};
    bad |= check(c, tgsf_submit(c, &in, &o1), TGSF_OK, "tgsf_submit");
    in.lengths = len.data();
    *nf2 = 0;
    bad |= check(c, tgsf_submit_device(c, &in, &o2, nf2, nullptr), TGSF_OK, "tgsf_submit_device");
    bad |= check(c, tgsf_wait(c), TGSF_OK, "tgsf_wait");
    if (!bad && (*nf2 != o1.n_frags || memcmp(r1.data(), r2.data(), kReads * sizeof(tgsf_read_result)) ||
                 memcmp(f1.data(), f2.data(), o1.n_frags * sizeof(tgsf_fragment)))) {
        fprintf(stderr, "tgsf_submit and tgsf_submit_device disagree\n");
        bad = 1;
    }
    uint32_t mid = 0;
    for (uint32_t i = 0; i < kReads; i++) mid += (r1[i].flags & TGSF_RF_ADMID) ? 1u : 0u;
    if (!bad && mid < kReads / 16) { fprintf(stderr, "only %u reads with a middle adapter\n", mid); bad = 1; }
    // one byte more than the context takes: refused, nothing enqueued
    in.n_bytes = total + 1;
    bad |= check(c, tgsf_submit_device(c, &in, &o2, nf2, nullptr), TGSF_E_CAPACITY, "tgsf_submit_device over capacity");
    bad |= check(c, tgsf_wait(c), TGSF_OK, "tgsf_wait after the refusal");
    in.n_bytes = 0;
    bad |= check(c, tgsf_submit_device(c, &in, &o2, nf2, nullptr), TGSF_E_INVALID, "tgsf_submit_device without a span");
    printf("%d adapters of %d bp, -M %d, TGSF_MID_FLAT=%s: %u reads with a middle adapter, %u fragments\n", n_adapters, p.adapter_len[0],
           mid_match_len, mid_flat ? mid_flat : "(unset)", mid, o1.n_frags);
    tgsf_destroy(c);
    free(seq); free(qual); free(nf2);
    return bad;
}

int main()
{
    setenv("TGSF_DEBUG_KNOBS", "1", 1);                               // the library reads TGSF_MID_FLAT only under this switch
    static const char* const ligation[2] = {"GCAATACGTAACTGAACGAAGT", "ACTTCGTTCAGTTACGTATTGC"};
    static const char* const blunt[2] = {"ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT", "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT"};
    // (33 bp: the shortest the filter takes, and no longer than the shortest read -- every read has a window for them)
    static const char* const four[4] = {"ATCTCTCTCAACAACAACAACGGAGGAGGAGGA", "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTT", "GTTTTCGCATTTATCGTGAAACGCTTTCGCGTT", "TGAAGCGGCGCACGAAAAACGCGAAAGCGTTTC"};
    int bad = 0;
    bad |= run(ligation, 2, 14, nullptr);
    bad |= run(ligation, 2, 14, "0");
    bad |= run(blunt, 2, 35, nullptr);
    bad |= run(blunt, 2, 35, "0");
    bad |= run(four, 4, 30, nullptr);
    if (bad) return 1;
    printf("largest batch ok\n");
    return 0;
}
