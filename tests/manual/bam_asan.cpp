// TEST INFRASTRUCTURE: the BAM input side of libtgsf_text (tgsf_text_bam_*) through the serial emulation of its kernels built
// with the host compiler's address and undefined-behaviour sanitizers.  This file includes the library's source, compiled
// with -DTGSF_EMUL, so the whole is one host program; of libtgsf it needs the emulation beside it:
//
//   make -s -C tests/emul
//   g++ -O1 -g -std=c++17 -DTGSF_EMUL -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wno-unused-function
//       -Wno-unknown-pragmas -x c++ tests/manual/bam_asan.cpp -o tests/emul/bam_asan -Ltests/emul -ltgsf_emul
//       -Wl,-rpath,'$ORIGIN'                                                                        (one command line)
//   tests/emul/bam_asan
//
// The emulation's device memory is host memory, so a byte read outside the BAM bytes or written outside the text buffer or the
// index arrays is a report: the BAM bytes and the caller's index arrays here are heap blocks of exactly their size, and the
// object's text buffer has exactly max_bytes rounded up to 16 plus TGSF_TEXT_PAD.
//   - the seam sweep: name lengths 0..17 x l_seq 1..40 (the base stretch on every offset of a 16-byte chunk in both nibble
//     parities), auxiliary tails of 0..16 bytes (every alignment of a record start), n_cigar_op 0, 1, 3, the unused low nibble
//     of an odd l_seq 0xF and 0 -- as one chunk, and every record alone in a block of exactly its bytes; then l_seq of
//     4096 - 17 .. 4096 + 17 (piece boundaries);
//   - the byte cuts: one three-record chunk cut at every byte, final and not final, host form and device form.
// Every result is compared with a decoder written here from the rule of include/tgsf_text.h.
// Exit status 0 and "bam ok": no difference, no error code, no sanitizer report (a report ends the program).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
static void put32(Bytes& b, uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i))); }

// one record: a random name of name_len bytes and its NUL, random codes and qualities (never 233), aux bytes behind them
static Bytes make_record(uint32_t name_len, uint32_t l_seq, uint32_t n_cigar, uint32_t aux, uint8_t low_fill)
{
    Bytes body;
    put32(body, 0xFFFFFFFFu); put32(body, 0xFFFFFFFFu);
    body.push_back((uint8_t)(name_len + 1)); body.push_back(255); body.push_back(0x48); body.push_back(0x12);
    body.push_back((uint8_t)n_cigar); body.push_back(0); body.push_back(4); body.push_back(0);
    put32(body, l_seq); put32(body, 0xFFFFFFFFu); put32(body, 0xFFFFFFFFu); put32(body, 0);
    for (uint32_t i = 0; i < name_len; i++) body.push_back((uint8_t)(33 + rnd(94)));
    body.push_back(0);
    for (uint32_t i = 0; i < 4 * n_cigar; i++) body.push_back((uint8_t)rnd(256));
    for (uint32_t i = 0; i < l_seq; i += 2) body.push_back((uint8_t)(rnd(16) << 4 | (i + 1 < l_seq ? rnd(16) : low_fill)));
    for (uint32_t i = 0; i < l_seq; i++) { uint8_t q = (uint8_t)rnd(256); body.push_back(q == 233 ? 0 : q); }
    for (uint32_t i = 0; i < aux; i++) body.push_back((uint8_t)rnd(256));
    Bytes r;
    put32(r, (uint32_t)body.size());
    r.insert(r.end(), body.begin(), body.end());
    return r;
}

struct Model {
    std::string text;
    std::vector<uint64_t> seq_off, qual_off, name_off;
    std::vector<uint32_t> len, name_len;
    uint32_t stop = 0;
    uint64_t consumed = 0, bases = 0;
    uint32_t longest = 0;
};

static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the rule of include/tgsf_text.h
static Model model(const Bytes& bam, uint64_t n, bool final, uint32_t max_records, uint64_t max_bytes)
{
    static const char T[17] = "\0AC\0G\0\0\0T\0\0\0\0\0\0N";
    Model m;
    uint64_t at = 0;
    for (;;) {
        m.consumed = at;
        if (at == n) { m.stop = TGSF_TEXT_END; break; }
        if (m.len.size() == max_records) { m.stop = TGSF_TEXT_CAPACITY; break; }
        if (n - at < 4) { m.stop = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        const uint32_t block = le32(&bam[at]);
        if (block < 32) { m.stop = TGSF_TEXT_IRREGULAR; break; }
        if (n - at - 4 < block) { m.stop = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        const uint8_t* r = &bam[at + 4];
        const uint32_t l_read_name = r[8], n_cigar = r[12] | r[13] << 8, l_seq = le32(r + 16);
        const uint64_t o_seq = 32ull + l_read_name + 4ull * n_cigar, o_qual = o_seq + (l_seq + 1ull) / 2;
        if (o_qual + l_seq > block || l_seq == 0) { m.stop = TGSF_TEXT_IRREGULAR; break; }
        const size_t nl = strnlen((const char*)r + 32, l_read_name);
        if (m.text.size() + nl + 2ull * l_seq + 6 > max_bytes) { m.stop = TGSF_TEXT_CAPACITY; break; }
        m.text += '@';
        m.name_off.push_back(m.text.size()); m.name_len.push_back((uint32_t)nl);
        m.text.append((const char*)r + 32, nl);
        m.text += '\n';
        m.seq_off.push_back(m.text.size()); m.len.push_back(l_seq);
        for (uint32_t k = 0; k < l_seq; k++) m.text += T[k & 1 ? r[o_seq + k / 2] & 15 : r[o_seq + k / 2] >> 4];
        m.text += "\n+\n";
        m.qual_off.push_back(m.text.size());
        for (uint32_t k = 0; k < l_seq; k++) m.text += (char)(uint8_t)(r[o_qual + k] + 33);
        m.text += '\n';
        m.bases += l_seq;
        if (l_seq > m.longest) m.longest = l_seq;
        at += 4ull + block;
    }
    return m;
}

template <class T>
static T* exact(const T* src, size_t count)          // a heap block of exactly count entries, 16-byte aligned
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, count * sizeof(T) > 0 ? count * sizeof(T) : 1)) abort();
    if (src && count) memcpy(p, src, count * sizeof(T)); else if (count) memset(p, 0xA5, count * sizeof(T));
    return (T*)p;
}

static uint64_t g_decodes = 0;

// one decode of bam[0 .. n) on an object made for exactly this input, device form (and the host form when asked), against the model
static int check(const Bytes& bam, uint64_t n, bool final, uint32_t max_records, const char* what, bool host_form)
{
    const Model m = model(bam, n, final, max_records, ~0ull);
    const uint64_t max_bytes = m.text.size() ? m.text.size() : 1;      // the text fits exactly
    tgsf_text* tx = nullptr;
    if (tgsf_text_create(0, max_bytes, max_records, &tx) != TGSF_OK) { fprintf(stderr, "%s: tgsf_text_create: %s\n", what, tgsf_text_last_error(nullptr)); return 1; }
    int bad = 0;
    if (tgsf_text_bam_reserve(tx, n ? n : 1) != TGSF_OK) { fprintf(stderr, "%s: reserve: %s\n", what, tgsf_text_last_error(tx)); bad = 1; }
    uint8_t* d_bam = exact(bam.data(), (size_t)n);
    std::vector<uint64_t> rec_off(max_records + 1);
    uint32_t n_walked = 0, walk_stop = 0;
    uint64_t consumed = 0;
    if (!bad && tgsf_text_bam_walk(d_bam, n, final, max_records, rec_off.data(), &n_walked, &walk_stop, &consumed) != TGSF_OK) { fprintf(stderr, "%s: the walk failed\n", what); bad = 1; }
    tgsf_text_index_arrays I = {exact<uint64_t>(nullptr, max_records), exact<uint64_t>(nullptr, max_records), exact<uint32_t>(nullptr, max_records),
                                exact<uint64_t>(nullptr, max_records), exact<uint32_t>(nullptr, max_records)};
    tgsf_text_bam_summary* s = exact<tgsf_text_bam_summary>(nullptr, 1);
    tgsf_text_device_buffers b;
    tgsf_text_buffers(tx, &b);
    for (int form = 0; form < (host_form ? 2 : 1) && !bad; form++) {
        memset(b.text, 0xA5, (size_t)(((max_bytes + 15) & ~15ull) + TGSF_TEXT_PAD));
        const int rc = form == 0 ? tgsf_text_bam_decode_device(tx, d_bam, n, final, rec_off.data(), n_walked, walk_stop, &I, s, nullptr)
                                 : tgsf_text_bam_decode(tx, d_bam, n, final, &I, s);
        g_decodes++;
        if (rc != TGSF_OK) { fprintf(stderr, "%s: decode: status %d: %s\n", what, rc, tgsf_text_last_error(tx)); bad = 1; break; }
        const size_t k = m.len.size();
        if (s->n_records != k || s->stop != m.stop || s->consumed != m.consumed || s->text_bytes != m.text.size() || s->bases != m.bases ||
            s->longest != m.longest || s->bad_qual != 0xFFFFFFFFu || s->reserved != 0) {
            fprintf(stderr, "%s (form %d): summary %u records, stop %u, consumed %llu, %llu bytes; expected %zu, %u, %llu, %zu\n", what, form, s->n_records, s->stop,
                    (unsigned long long)s->consumed, (unsigned long long)s->text_bytes, k, m.stop, (unsigned long long)m.consumed, m.text.size());
            bad = 1;
            break;
        }
        if (m.text.size() && memcmp(b.text, m.text.data(), m.text.size())) { fprintf(stderr, "%s (form %d): the text differs\n", what, form); bad = 1; }
        for (uint32_t i = 0; i < TGSF_TEXT_PAD && !bad; i++) if (b.text[m.text.size() + i]) { fprintf(stderr, "%s: pad byte %u is not zero\n", what, i); bad = 1; }
        for (uint64_t i = m.text.size() + TGSF_TEXT_PAD; i < ((max_bytes + 15) & ~15ull) + TGSF_TEXT_PAD && !bad; i++)
            if (b.text[i] != 0xA5) { fprintf(stderr, "%s: byte %llu behind the pad was written\n", what, (unsigned long long)i); bad = 1; }
        if (!bad && k && (memcmp(I.seq_off, m.seq_off.data(), k * 8) || memcmp(I.qual_off, m.qual_off.data(), k * 8) || memcmp(I.len, m.len.data(), k * 4) ||
                     memcmp(I.name_off, m.name_off.data(), k * 8) || memcmp(I.name_len, m.name_len.data(), k * 4))) { fprintf(stderr, "%s (form %d): the index differs\n", what, form); bad = 1; }
    }
    free(I.seq_off); free(I.qual_off); free(I.len); free(I.name_off); free(I.name_len); free(s); free(d_bam);
    tgsf_text_destroy(tx);
    return bad;
}

int main()
{
    int bad = 0;
    char what[96];
    // the seam sweep
    for (int fill = 0; fill < 2 && !bad; fill++) {
        Bytes chunk;
        uint32_t k = 0;
        for (uint32_t nl = 0; nl <= 17 && !bad; nl++)
            for (uint32_t L = 1; L <= 40 && !bad; L++, k++) {
                static const uint32_t cig[3] = {0, 1, 3};
                const Bytes r = make_record(nl, L, cig[k % 3], k % 17, fill ? 0 : 0xF);
                snprintf(what, sizeof what, "record alone: name %u, l_seq %u, aux %u", nl, L, k % 17);
                bad |= check(r, r.size(), true, 1, what, false);
                chunk.insert(chunk.end(), r.begin(), r.end());
            }
        if (!bad) bad |= check(chunk, chunk.size(), true, k, "the sweep as one chunk", true);
        if (!bad) bad |= check(chunk, chunk.size(), true, k - 1, "the sweep, one record too many", false);
    }
    if (!bad) {
        Bytes chunk;
        for (uint32_t L = 4096 - 17; L <= 4096 + 17; L++) { const Bytes r = make_record(L % 11, L, 0, L % 5, 0xF); chunk.insert(chunk.end(), r.begin(), r.end()); }
        bad |= check(chunk, chunk.size(), true, 35, "piece boundaries", true);
    }
    // the byte cuts
    if (!bad) {
        Bytes chunk;
        const uint32_t shape[3][4] = {{3, 21, 0, 2}, {0, 40, 1, 0}, {9, 5, 0, 7}};
        for (const auto& sh : shape) { const Bytes r = make_record(sh[0], sh[1], sh[2], sh[3], 0); chunk.insert(chunk.end(), r.begin(), r.end()); }
        for (uint64_t cut = 0; cut <= chunk.size() && !bad; cut++)
            for (int final = 0; final < 2 && !bad; final++) {
                snprintf(what, sizeof what, "cut at byte %llu, final %d", (unsigned long long)cut, final);
                bad |= check(chunk, cut, final != 0, 4, what, true);
            }
    }
    if (bad) return 1;
    printf("%llu decodes\nbam ok\n", (unsigned long long)g_decodes);
    return 0;
}
