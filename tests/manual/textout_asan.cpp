// TEST INFRASTRUCTURE: the output side of libtgsf_text (tgsf_text_format*) through the serial emulation of its kernels built
// with the host compiler's address and undefined-behaviour sanitizers.  This file includes the library's source, compiled
// with -DTGSF_EMUL, so the whole is one host program; of libtgsf it needs tgsf_backend only, from the emulation beside it:
//
//   make -s -C tests/emul
//   g++ -O1 -g -std=c++17 -DTGSF_EMUL -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wno-unused-function
//       -Wno-unknown-pragmas -x c++ tests/manual/textout_asan.cpp -o tests/emul/textout_asan -Ltests/emul -ltgsf_emul
//       -Wl,-rpath,'$ORIGIN'                                                                        (one command line)
//   tests/emul/textout_asan
//
// The emulation's device memory is host memory, so a byte read outside the text or written outside the output is a report:
// the text, the tables and the output buffers here are heap blocks of exactly their size.
//   - the seam sweep: a leading record of every length 1 .. 4096 + 17 pushes the records behind it over every offset of a
//     16-byte chunk and both sides of the 4096-byte piece seam, FASTQ and FASTA output, through tgsf_text_format_device into
//     a buffer of exactly n_bytes bytes;
//   - capacity and canaries: out_capacity of n_bytes - 1 and 0 (TGSF_TEXT_CAPACITY, no byte changed, the need is told), of
//     n_bytes (the bytes behind it keep their 0xA5), and the host form's TGSF_E_CAPACITY followed by the same call with room.
// Every output is compared with a formatter written here from the rule of include/tgsf_text.h.
// Exit status 0 and "textout ok": no difference, no error code, no sanitizer report (a report ends the program).
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

struct Read { std::string name, seq, qual; };
struct Text {
    std::string text;
    std::vector<uint64_t> name_off, seq_off, qual_off;
    std::vector<uint32_t> name_len, len;
};

static Text make_text(const std::vector<Read>& reads)
{
    Text t;
    for (const Read& r : reads) {
        t.text += '@';
        t.name_off.push_back(t.text.size()); t.name_len.push_back((uint32_t)r.name.size());
        t.text += r.name + '\n';
        t.seq_off.push_back(t.text.size()); t.len.push_back((uint32_t)r.seq.size());
        t.text += r.seq + "\n+\n";
        t.qual_off.push_back(t.text.size());
        t.text += r.qual + '\n';
    }
    return t;
}

static Read make_read(const char* name, uint32_t n)
{
    Read r;
    r.name = name;
    for (uint32_t i = 0; i < n; i++) { r.seq += "ACGT"[rnd(4)]; r.qual += (char)(33 + 3 + rnd(37)); }
    return r;
}

// the rule of include/tgsf_text.h
static std::string model(const Text& t, const std::vector<tgsf_fragment>& frags, bool fastq, std::vector<uint64_t>& ends)
{
    std::string out;
    std::vector<uint32_t> seen(t.len.size(), 0);
    ends.clear();
    for (const tgsf_fragment& f : frags) {
        if (!(f.flags & TGSF_FF_PASS)) continue;
        const uint32_t k = ++seen[f.read];
        std::string name = t.text.substr(t.name_off[f.read], t.name_len[f.read]);
        if (k >= 2) {
            size_t at = name.find_first_of(" \t\n\v\f\r");
            if (at == std::string::npos) at = name.size();
            name.insert(at, ":" + std::to_string(k));
        }
        out += fastq ? '@' : '>';
        out += name + '\n' + t.text.substr(t.seq_off[f.read] + f.start, f.len);
        if (fastq) out += "\n+\n" + t.text.substr(t.qual_off[f.read] + f.start, f.len);
        out += '\n';
        ends.push_back(out.size());
    }
    return out;
}

static void tables(uint32_t n_reads, const std::vector<tgsf_fragment>& frags, std::vector<tgsf_read_result>& reads)
{
    reads.assign(n_reads, tgsf_read_result());
    for (const tgsf_fragment& f : frags) reads[f.read].n_frags++;
    uint32_t at = 0;
    for (tgsf_read_result& r : reads) { r.frag_begin = at; at += r.n_frags; }
}

template <class T>
static T* exact(const std::vector<T>& v)          // a heap block of exactly the vector's bytes, 16-byte aligned
{
    void* p = nullptr;
    const size_t bytes = v.size() * sizeof(T);
    if (posix_memalign(&p, 16, bytes > 0 ? bytes : 1)) abort();
    if (bytes > 0) memcpy(p, v.data(), bytes);
    return (T*)p;
}

static int fails(tgsf_text* tx, const char* what, int rc, int want)
{
    if (rc == want) return 0;
    fprintf(stderr, "%s: status %d, expected %d: %s\n", what, rc, want, tgsf_text_last_error(tx));
    return 1;
}

static uint8_t* g_text;       // the text in a heap block of exactly its size: the kernels read it from there

// one format through the device form into a buffer of exactly `room` bytes of which `cap` are offered
static int format_exact(tgsf_text* tx, const Text& t, const std::vector<tgsf_fragment>& frags, bool fastq, uint64_t cap, uint64_t room,
                        const char* what)
{
    std::vector<tgsf_read_result> reads;
    tables((uint32_t)t.len.size(), frags, reads);
    std::vector<uint64_t> ends;
    const std::string want = model(t, frags, fastq, ends);
    tgsf_read_result* d_reads = exact(reads);
    tgsf_fragment* d_frags = exact(frags);
    uint8_t* d_out = exact(std::vector<uint8_t>(room, 0xA5));
    uint64_t* d_ends = exact(std::vector<uint64_t>(frags.size(), 0));
    tgsf_text_out_summary* d_sum = exact(std::vector<tgsf_text_out_summary>(1));
    int bad = fails(tx, what, tgsf_text_format_device(tx, g_text, nullptr, (uint32_t)t.len.size(), 0, d_reads, d_frags, (uint32_t)frags.size(), fastq,
                                                      d_out, cap, d_ends, d_sum, nullptr), TGSF_OK);
    if (!bad) {
        const bool fits = want.size() <= cap;
        if (d_sum->n_bytes != want.size() || d_sum->n_records != ends.size() || d_sum->stop != (fits ? TGSF_TEXT_END : TGSF_TEXT_CAPACITY)) {
            fprintf(stderr, "%s: summary %llu bytes, %u records, stop %u; expected %zu, %zu\n", what, (unsigned long long)d_sum->n_bytes,
                    d_sum->n_records, d_sum->stop, want.size(), ends.size());
            bad = 1;
        }
        const uint64_t written = fits ? want.size() : 0;
        if (!bad && (memcmp(d_out, want.data(), written) || (fits && memcmp(d_ends, ends.data(), ends.size() * 8)))) { fprintf(stderr, "%s: the output differs\n", what); bad = 1; }
        for (uint64_t i = written; !bad && i < room; i++)
            if (d_out[i] != 0xA5) { fprintf(stderr, "%s: byte %llu behind the output was written\n", what, (unsigned long long)i); bad = 1; }
    }
    free(d_reads); free(d_frags); free(d_out); free(d_ends); free(d_sum);
    return bad;
}

static tgsf_fragment frag(uint32_t read, int32_t start, int32_t len, uint32_t flags)
{
    tgsf_fragment f;
    f.sum_q = 0; f.read = read; f.start = start; f.len = len; f.flags = flags;
    return f;
}

int main()
{
    const std::vector<Read> reads = {make_read("lead", 4096 + 40), make_read("a b", 33), make_read("", 5), make_read("tail\tx", 64)};
    const Text t = make_text(reads);
    tgsf_text* tx = nullptr;
    if (tgsf_text_create(0, t.text.size(), (uint32_t)reads.size(), &tx) != TGSF_OK) { fprintf(stderr, "tgsf_text_create: %s\n", tgsf_text_last_error(nullptr)); return 1; }
    int bad = 0;
    tgsf_text_summary s;
    uint8_t* text = g_text = exact(std::vector<uint8_t>(t.text.begin(), t.text.end()));
    bad |= fails(tx, "tgsf_text_index", tgsf_text_index(tx, text, t.text.size(), 0, 1, nullptr, &s), TGSF_OK);
    if (!bad && (s.n_records != reads.size() || s.stop != TGSF_TEXT_END)) { fprintf(stderr, "the text was not indexed to its end\n"); bad = 1; }
    bad |= fails(tx, "tgsf_text_out_reserve", tgsf_text_out_reserve(tx, 16, 3 * t.text.size()), TGSF_OK);

    // the seam sweep
    uint64_t sweeps = 0;
    for (int fastq = 1; fastq >= 0 && !bad; fastq--)
        for (int32_t L = 1; L <= 4096 + 17 && !bad; L++) {
            const std::vector<tgsf_fragment> fr = {frag(0, 3, L, TGSF_FF_PASS), frag(1, 0, 33, TGSF_FF_PASS), frag(1, 1, 17, TGSF_FF_PASS), frag(2, 0, 5, 0),
                                                   frag(2, 0, 5, TGSF_FF_PASS), frag(2, 1, 1, TGSF_FF_REPEAT), frag(3, 0, 64, TGSF_FF_PASS), frag(3, 10, 1, TGSF_FF_PASS)};
            std::vector<uint64_t> ends;
            const uint64_t need = model(t, fr, fastq, ends).size();
            bad |= format_exact(tx, t, fr, fastq, need, need, "sweep");
            sweeps++;
        }

    // capacity and canaries
    const std::vector<tgsf_fragment> fr = {frag(0, 0, 4096 + 40, TGSF_FF_PASS), frag(0, 7, 500, TGSF_FF_PASS), frag(1, 0, 33, 0), frag(3, 1, 63, TGSF_FF_PASS)};
    std::vector<uint64_t> ends;
    const std::string want = model(t, fr, true, ends);
    const uint64_t need = want.size();
    if (!bad) {
        bad |= format_exact(tx, t, fr, true, need - 1, need + 64, "capacity n_bytes - 1");
        bad |= format_exact(tx, t, fr, true, 0, 64, "capacity 0");
        bad |= format_exact(tx, t, fr, true, need, need + 64, "capacity n_bytes");
        bad |= format_exact(tx, t, fr, false, need, need + 64, "FASTA output in the same room");
    }
    if (!bad) {                                                       // the host form
        std::vector<tgsf_read_result> rd;
        tables((uint32_t)reads.size(), fr, rd);
        tgsf_read_result* h_reads = exact(rd);
        tgsf_fragment* h_frags = exact(fr);
        uint8_t* out = exact(std::vector<uint8_t>(need, 0xA5));
        uint64_t* h_ends = exact(std::vector<uint64_t>(fr.size(), 0));
        tgsf_text_out_summary os;
        bad |= fails(tx, "tgsf_text_format without room", tgsf_text_format(tx, (uint32_t)reads.size(), 0, h_reads, h_frags, (uint32_t)fr.size(), 1, out, need - 1, h_ends, &os), TGSF_E_CAPACITY);
        if (!bad && (os.n_bytes != need || os.stop != TGSF_TEXT_CAPACITY || out[0] != 0xA5 || out[need - 1] != 0xA5)) { fprintf(stderr, "a refused format wrote, or did not tell the need\n"); bad = 1; }
        bad |= fails(tx, "tgsf_text_format with room", tgsf_text_format(tx, (uint32_t)reads.size(), 0, h_reads, h_frags, (uint32_t)fr.size(), 1, out, need, h_ends, &os), TGSF_OK);
        if (!bad && (os.n_bytes != need || os.n_records != ends.size() || memcmp(out, want.data(), need) || memcmp(h_ends, ends.data(), ends.size() * 8))) { fprintf(stderr, "tgsf_text_format: the output differs\n"); bad = 1; }
        bad |= fails(tx, "too many fragments", tgsf_text_format(tx, (uint32_t)reads.size(), 0, h_reads, h_frags, 17, 1, out, need, h_ends, &os), TGSF_E_CAPACITY);
        bad |= fails(tx, "FASTQ from FASTA", tgsf_text_format(tx, (uint32_t)reads.size(), 1, h_reads, h_frags, (uint32_t)fr.size(), 1, out, need, h_ends, &os), TGSF_E_INVALID);
        free(h_reads); free(h_frags); free(out); free(h_ends);
    }
    tgsf_text_destroy(tx);
    free(text);
    if (bad) return 1;
    printf("%llu sweeps, %llu bytes with canaries\ntextout ok\n", (unsigned long long)sweeps, (unsigned long long)need);
    return 0;
}
