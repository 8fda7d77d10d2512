// tgsf_text.hip -- libtgsf_text.so: the record index of FASTQ / FASTA text on the device (include/tgsf_text.h).
// Built on the public ABI of libtgsf only (tgsf_backend, tgsf_submit_device, tgsf_wait, tgsf_last_error).
//
// Built two ways from this one source, like tgsf_lib.hip:
//   hipcc --offload-arch=gfx950  -ltgsf       -> tgsfilter_amd/libtgsf_text.so      (the product)
//   g++ -x c++ -DTGSF_EMUL       -ltgsf_emul  -> tests/emul/libtgsf_text_emul.so    (serial emulation; test infrastructure)
#include <algorithm>

#include "tgsf_text_kernels.h"
constexpr size_t kErrorCap = 768;          // bytes of an error text (fail)
#include "tgsf_rt.h"                       // the runtime layer: HIP, or the serial emulation's (test infrastructure)
#if defined(TGSF_EMUL)
namespace tgsf_emul { thread_local Dim3 threadIdx, blockIdx, blockDim, gridDim; }
#endif

using namespace tgsf;

// an event pair around the launches of a call (profile): begin() and end() record on the launches' stream; ms() once that stream
// has been waited for, the milliseconds between them -- 0 when profiling is off, nothing was recorded, or it has been read
struct Span {
    rt_event e[2] = {nullptr, nullptr};
    bool recorded = false;
    void begin(rt_stream st) { (void)rt_event_record(e[0], st); }
    void end(rt_stream st) { (void)rt_event_record(e[1], st); recorded = true; }
    float ms(bool profile)
    {
        float t = 0.0f;
        if (profile && recorded && !rt_event_ms(&t, e[0], e[1])) { recorded = false; return t; }
        (void)rt_last_error();
        return 0.0f;
    }
};

struct tgsf_text : rt_ctx {                // (alloc_slack 0: the arrays are exact, the text has TGSF_TEXT_PAD)
    uint64_t max_bytes, max_pieces;
    uint32_t max_records;
    rt_stream stream;
    bool profile = false;
    // device memory
    uint8_t* d_text = nullptr;          // max_bytes rounded up to 16, + TGSF_TEXT_PAD
    uint64_t* d_bits = nullptr;         // a bit per byte, whole pieces
    uint32_t* d_cnt = nullptr;          // line ends per piece -> exclusive sums within blocks of kTextScanTile pieces
    uint64_t* d_part = nullptr;         // ... and the blocks' offsets
    uint64_t* d_table = nullptr;        // positions of the first 4 * max_records line ends
    TextState* d_state = nullptr;
    tgsf_text_index_arrays d_index = {nullptr, nullptr, nullptr, nullptr, nullptr};
    tgsf_text_summary* d_summary = nullptr;
    // results of tgsf_text_submit before they go down
    tgsf_read_result* d_reads = nullptr;
    tgsf_fragment* d_frags = nullptr;
    uint32_t frag_cap = 0;
    uint32_t* d_nfrags = nullptr;
    // the output side (tgsf_text_out_reserve): per-fragment scratch, the object's own output buffer
    bool out_reserved = false;
    uint32_t max_frags = 0;
    uint64_t max_out = 0;
    uint32_t* d_opass = nullptr;        // PASS flags -> exclusive sums within blocks of kTextScanTile fragments
    uint64_t* d_opass_part = nullptr;   // ... and the blocks' offsets
    uint64_t* d_osize = nullptr;        // record sizes -> the same, 64-bit
    uint64_t* d_osize_part = nullptr;
    uint64_t* d_oends = nullptr;        // the byte behind each fragment's record
    TextOutMeta* d_ometa = nullptr;
    TextOutState* d_ostate = nullptr;
    tgsf_fragment* d_ofrags = nullptr;  // fragment records: tgsf_text_format's table, tgsf_text_filter without batch_out
    uint64_t* d_orec_end = nullptr;
    uint8_t* d_out = nullptr;
    tgsf_text_out_summary* d_osummary = nullptr;
    // the BAM input side (tgsf_text_bam_reserve): the chunk's bytes, the walked records' offsets, per-record scratch
    bool bam_reserved = false;
    uint64_t max_bam = 0;
    uint8_t* d_bam = nullptr;           // max_bam rounded up to 16, + TGSF_TEXT_PAD
    uint64_t* d_brec_off = nullptr;     // max_records + 1
    uint64_t* d_bsize = nullptr;        // sizes of the records' text -> exclusive sums within blocks of kTextScanTile records
    uint64_t* d_bsize_part = nullptr;   // ... and the blocks' offsets
    uint64_t* d_bends = nullptr;        // the byte behind each record's text
    uint32_t* d_boseq = nullptr;        // where the packed bases begin in each record
    BamState* d_bstate = nullptr;
    tgsf_text_bam_summary* d_bsummary = nullptr;
    std::vector<uint64_t> h_rec_off;    // the walk of tgsf_text_bam_decode / _submit / _filter
    uint64_t* d_bwalk = nullptr;        // tgsf_text_bam_walk_device: BamWalkHead (16 bytes), then max_records + 1 offsets
    std::vector<uint64_t> h_bwalk;      // ... as they come down
    // the BGZF input side (tgsf_text_bgzf_reserve): the chunk's compressed bytes, the members walked
    bool gz_reserved = false;
    uint64_t max_gz = 0;
    uint32_t max_gblocks = 0;
    uint8_t* d_gz = nullptr;            // max_gz rounded up to 16, + TGSF_TEXT_PAD
    tgsf_text_bgzf_block* d_gblocks = nullptr;
    BgzfState* d_gstate = nullptr;
    tgsf_text_bgzf_summary* d_gsummary = nullptr;
    std::vector<tgsf_text_bgzf_block> h_gblocks;   // the walk of tgsf_text_bgzf_inflate
    uint32_t* d_crc_tab = nullptr;      // the CRC32 tables of k_gz_count and k_bgzf_crc (either reserve brings them up)
    // the BGZF output side (tgsf_text_bgzf_out_reserve): the host form's input, the compressed bytes, per-member scratch
    bool zout_reserved = false;
    uint64_t max_zin = 0, max_zout = 0;
    uint32_t max_zmembers = 0;
    uint8_t* d_zin = nullptr;           // max_zin rounded up to 16
    uint8_t* d_zout = nullptr;          // max_zout rounded up to 16
    int zlevel = 0;                     // tgsf_text_bgzf_out_level: 0 Huffman-only, 1 the match search
    GzMeta* d_zmeta = nullptr;          // codes, CRC32 and verdict of every member
    GzLzMeta* d_zlz = nullptr;          // level 1: whether the block of matches won, and its two codes
    uint64_t* d_zsize = nullptr;        // the members' sizes -> exclusive sums within blocks of kTextScanTile members
    uint64_t* d_zsize_part = nullptr;   // ... and the blocks' offsets
    uint64_t* d_zend = nullptr;         // the byte behind each member (the host form's member_end)
    GzState* d_zstate = nullptr;
    tgsf_text_gzout_summary* d_zsummary = nullptr;
    Span zev;
    // around the last index, and around the stages of the last format (profile)
    Span ev;
    rt_event oev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool oev_recorded = false;
};

extern "C" int tgsf_text_abi_version(void) { return TGSF_TEXT_ABI_VERSION; }
extern "C" const char* tgsf_text_backend(void) { return kTgsfEmul ? "emulation" : "hip:gfx950"; }
extern "C" const char* tgsf_text_last_error(tgsf_text* tx) { return tx ? tx->error.c_str() : g_create_error.c_str(); }

extern "C" void tgsf_text_destroy(tgsf_text* tx)
{
    if (!tx) return;
    (void)rt_set_device(tx->device);
    if (tx->stream) { (void)rt_sync(tx->stream); rt_stream_destroy(tx->stream); }
    for (rt_event e : tx->ev.e) rt_event_destroy(e);
    for (rt_event e : tx->oev) rt_event_destroy(e);
    for (rt_event e : tx->zev.e) rt_event_destroy(e);
    dev_free_all(tx);
    delete tx;
}

extern "C" int tgsf_text_create(int device, uint64_t max_bytes, uint32_t max_records, tgsf_text** out)
{
    if (!out) return fail(nullptr, TGSF_E_INVALID, "null argument");
    *out = nullptr;
    if (max_bytes == 0 || max_records == 0) return fail(nullptr, TGSF_E_INVALID, "max_bytes and max_records must be positive");
    // one build of the kernels per process: the product binds the HIP build of libtgsf, the emulation the emulation
    const char* be = tgsf_backend();
    if (strncmp(be, kTgsfEmul ? "emulation" : "hip", kTgsfEmul ? 9 : 3) != 0)
        return fail(nullptr, TGSF_E_INVALID, "libtgsf_text (%s) is linked against the '%s' build of libtgsf", tgsf_text_backend(), be);
    tgsf_text* tx = new tgsf_text;
    tx->device = device;
    tx->max_bytes = max_bytes;
    tx->max_records = max_records;
    tx->max_pieces = (max_bytes + kTextPiece - 1) / kTextPiece;
    tx->stream = nullptr;
    if (rt_set_device(device)) { delete tx; return fail(nullptr, TGSF_E_NO_DEVICE, "hipSetDevice(%d) failed: no usable HIP device (there is no CPU fallback)", device); }
    if (rt_stream_create(&tx->stream)) { delete tx; return fail(nullptr, TGSF_E_HIP, "stream creation failed"); }
    for (rt_event& e : tx->ev.e) if (rt_event_create(&e)) { tgsf_text_destroy(tx); return fail(nullptr, TGSF_E_HIP, "event creation failed"); }
    const uint64_t text_bytes = ((max_bytes + 15u) & ~15ull) + TGSF_TEXT_PAD;
    int e = 0;
    e |= dev_alloc(tx, &tx->d_text, text_bytes);
    if (!e) e |= dev_alloc(tx, &tx->d_bits, tx->max_pieces * kTextPieceWords);
    if (!e) e |= dev_alloc(tx, &tx->d_cnt, tx->max_pieces + 1);
    if (!e) e |= dev_alloc(tx, &tx->d_part, tx->max_pieces / kTextScanTile + 2);
    if (!e) e |= dev_alloc(tx, &tx->d_table, 4ull * max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_state, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_index.seq_off, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_index.qual_off, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_index.len, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_index.name_off, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_index.name_len, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_summary, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_reads, max_records);
    if (!e) e |= dev_alloc(tx, &tx->d_nfrags, 4);
    if (e) {
        tgsf_text_destroy(tx);
        return fail(nullptr, TGSF_E_HIP, "device allocation failed (%llu bytes of text, %u records)", (unsigned long long)max_bytes, max_records);
    }
    *out = tx;
    return TGSF_OK;
}

extern "C" int tgsf_text_profile(tgsf_text* tx, int enable)
{
    if (!tx) return TGSF_E_INVALID;
    tx->profile = enable != 0;
    return TGSF_OK;
}

extern "C" int tgsf_text_buffers(tgsf_text* tx, tgsf_text_device_buffers* out)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out) return fail(tx, TGSF_E_INVALID, "null argument");
    out->text = tx->d_text;
    out->index = tx->d_index;
    out->summary = tx->d_summary;
    out->max_bytes = tx->max_bytes;
    out->max_records = tx->max_records;
    out->reserved = 0;
    return TGSF_OK;
}

static unsigned blocks_for(uint64_t items, unsigned per_block) { return (unsigned)((items + per_block - 1) / per_block); }
// the grid of a kernel whose waves stride over `waves` items: a wave each, at most a few per SIMD of the device
static unsigned wave_grid(uint64_t waves, unsigned threads = kTextThreads, unsigned cap = 2048u)
{
    return grid_cap(std::min(std::max(blocks_for(waves * kTextLanes, threads), 1u), cap));
}
// what every enqueue ends with
static int launched(tgsf_text* tx) { return rt_last_error() ? fail(tx, TGSF_E_HIP, "kernel launch failed") : TGSF_OK; }
// a caller's stream (NULL: the object's own)
static rt_stream stream_of(tgsf_text* tx, void* hip_stream) { return hip_stream ? (rt_stream)hip_stream : tx->stream; }

// bytes from the device to the host on the object's stream (0: no copy), which is then waited for; wait = false: a copy
// follows on the same stream, and its wait is this one's
static int down(tgsf_text* tx, void* dst, const void* src, size_t bytes, bool wait = true)
{
    int he = bytes ? rt_d2h(dst, src, bytes, tx->stream) : 0;
    if (!he && wait) he = rt_sync(tx->stream);
    return he ? fail(tx, TGSF_E_HIP, "device to host copy failed: %s", rt_errstr(he)) : TGSF_OK;
}

// exclusive prefix sums of a[0 .. n) on st, in place and two levels deep (part: the blocks' offsets; *total: the sum)
template <typename T> static void enqueue_scan(rt_stream st, T* a, uint64_t n, uint64_t* part, uint64_t* total)
{
    const uint32_t nb = (uint32_t)((n + kTextScanTile - 1) / kTextScanTile);
    if (n) TGSF_LAUNCH_COOP(k_text_scan_tiles<T>, nb, 256, st, a, n, part);
    TGSF_LAUNCH_COOP(k_textout_scan_top, 1, 64, st, part, nb, total);
}

// the seven launches of one index, on st; nothing is waited for
static int enqueue_index(tgsf_text* tx, const uint8_t* d_text, uint64_t n, int fasta, int final,
                         const tgsf_text_index_arrays& I, tgsf_text_summary* d_summary, rt_stream st)
{
    const uint64_t pieces = (n + kTextPiece - 1) / kTextPiece;
    const uint32_t nb = (uint32_t)((pieces + kTextScanTile - 1) / kTextScanTile);
    const uint64_t cap = (fasta ? 2ull : 4ull) * tx->max_records;
    const unsigned gwave = blocks_for(pieces * kTextLanes, kTextThreads);          // a wave per piece
    const unsigned gemit = blocks_for((pieces + kTextEmitPieces - 1) / kTextEmitPieces * kTextLanes, kTextThreads);
    const unsigned gsmall = grid_cap(std::min(blocks_for(tx->max_records, kTextThreads), 2048u));
    const unsigned gfold = std::min(gsmall, 64u);                                  // every wave ends in two atomics on one word each
    if (tx->profile) tx->ev.begin(st);
    if (pieces) {
        TGSF_LAUNCH(k_text_mark, gwave, kTextThreads, st, d_text, n, pieces, (uint16_t*)tx->d_bits, tx->d_cnt);
        TGSF_LAUNCH_COOP(k_text_scan_tiles<uint32_t>, nb, 256, st, tx->d_cnt, pieces, tx->d_part);
    }
    TGSF_LAUNCH_COOP(k_text_scan_top, 1, 64, st, tx->d_part, nb, tx->d_state);
    if (pieces)
        TGSF_LAUNCH(k_text_emit, gemit, kTextThreads, st, (const uint64_t*)tx->d_bits, (const uint32_t*)tx->d_cnt,
                    (const uint64_t*)tx->d_part, pieces, tx->d_table, cap);
    TGSF_LAUNCH(k_text_check, gsmall, kTextThreads, st, d_text, n, fasta, final, (const uint64_t*)tx->d_table, tx->max_records, tx->d_state, I);
    TGSF_LAUNCH(k_text_fold<TextState>, gfold, kTextThreads, st, (const uint32_t*)I.len, tx->max_records, fasta, tx->d_state);
    TGSF_LAUNCH_COOP(k_text_finish, 1, 64, st, n, fasta, final, (const uint64_t*)tx->d_table, tx->max_records, (const TextState*)tx->d_state, d_summary);
    if (tx->profile) tx->ev.end(st);
    return launched(tx);
}

static int check_args(tgsf_text* tx, uint64_t n_bytes, int fasta, int final)
{
    if ((fasta != 0 && fasta != 1) || (final != 0 && final != 1)) return fail(tx, TGSF_E_INVALID, "fasta and final are 0 or 1");
    if (n_bytes > tx->max_bytes)
        return fail(tx, TGSF_E_CAPACITY, "text of %llu bytes, the indexer was created for %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_bytes);
    return TGSF_OK;
}

// a caller's index arrays on the device (NULL: the object's own)
static int check_index(tgsf_text* tx, const tgsf_text_index_arrays* d_index)
{
    if (d_index && (!d_index->seq_off || !d_index->qual_off || !d_index->len || !d_index->name_off || !d_index->name_len))
        return fail(tx, TGSF_E_INVALID, "a device index needs all five arrays");
    return TGSF_OK;
}

static int upload(tgsf_text* tx, const uint8_t* text, uint64_t n_bytes)
{
    int he = 0;
    if (n_bytes) he |= rt_h2d(tx->d_text, text, n_bytes, tx->stream);
    he |= rt_memset(tx->d_text + n_bytes, 0, (size_t)((((n_bytes + 15u) & ~15ull) - n_bytes) + TGSF_TEXT_PAD), tx->stream);
    return he ? fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he)) : TGSF_OK;
}

extern "C" int tgsf_text_upload(tgsf_text* tx, const uint8_t* text, uint64_t n_bytes)
{
    if (!tx) return TGSF_E_INVALID;
    if (!text && n_bytes) return fail(tx, TGSF_E_INVALID, "null text");
    int e = check_args(tx, n_bytes, 0, 0);
    if (e) return e;
    (void)rt_set_device(tx->device);
    if ((e = upload(tx, text, n_bytes))) return e;
    const int he = rt_sync(tx->stream);
    return he ? fail(tx, TGSF_E_HIP, "stream synchronize failed: %s", rt_errstr(he)) : TGSF_OK;
}

extern "C" int tgsf_text_index_device(tgsf_text* tx, const uint8_t* d_text, uint64_t n_bytes, int fasta, int final,
                                      const tgsf_text_index_arrays* d_index, tgsf_text_summary* d_summary, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    int e = check_args(tx, n_bytes, fasta, final);
    if (e) return e;
    if (!d_text) d_text = tx->d_text;
    if ((uintptr_t)d_text & 15u) return fail(tx, TGSF_E_INVALID, "the device text must be 16-byte aligned");
    if ((e = check_index(tx, d_index))) return e;
    (void)rt_set_device(tx->device);
    return enqueue_index(tx, d_text, n_bytes, fasta, final, d_index ? *d_index : tx->d_index, d_summary ? d_summary : tx->d_summary,
                         stream_of(tx, hip_stream));
}

// the first k entries of the object's own index to the host, on the object's stream, which is waited for
static int fetch_index(tgsf_text* tx, const tgsf_text_index_arrays* out_index, size_t k)
{
    if (!out_index || !k) return TGSF_OK;
    const tgsf_text_index_arrays &O = *out_index, &D = tx->d_index;   // (an array the caller does not take: 0 bytes)
    int e = down(tx, O.seq_off, D.seq_off, O.seq_off ? k * 8 : 0, false);
    if (!e) e = down(tx, O.qual_off, D.qual_off, O.qual_off ? k * 8 : 0, false);
    if (!e) e = down(tx, O.len, D.len, O.len ? k * 4 : 0, false);
    if (!e) e = down(tx, O.name_off, D.name_off, O.name_off ? k * 8 : 0, false);
    if (!e) e = down(tx, O.name_len, D.name_len, O.name_len ? k * 4 : 0);
    return e;
}

// the object's own summary and index to the host; the copies run on the object's stream, which is waited for
static int fetch(tgsf_text* tx, const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary, tgsf_text_summary* sum)
{
    int e = down(tx, sum, tx->d_summary, sizeof *sum);
    if (e) return e;
    sum->device_ms = tx->ev.ms(tx->profile);
    if ((e = fetch_index(tx, out_index, sum->n_records))) return e;
    if (out_summary) *out_summary = *sum;
    return TGSF_OK;
}

extern "C" int tgsf_text_fetch(tgsf_text* tx, const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    (void)rt_set_device(tx->device);
    tgsf_text_summary sum;
    return fetch(tx, out_index, out_summary, &sum);
}

extern "C" int tgsf_text_index(tgsf_text* tx, const uint8_t* text, uint64_t n_bytes, int fasta, int final,
                               const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out_summary || (!text && n_bytes)) return fail(tx, TGSF_E_INVALID, "null argument");
    int e = check_args(tx, n_bytes, fasta, final);
    if (e) return e;
    (void)rt_set_device(tx->device);
    if ((e = upload(tx, text, n_bytes))) return e;
    if ((e = enqueue_index(tx, tx->d_text, n_bytes, fasta, final, tx->d_index, tx->d_summary, tx->stream))) return e;
    tgsf_text_summary sum;
    return fetch(tx, out_index, out_summary, &sum);
}

// The filter on the text and the index that are in the object (n_records of them, n_bytes of text), through ctx; bo == NULL:
// nothing comes down.  The fragments go to d_fr on the device (room for fr_cap; NULL: not wanted), their number to *n_frags
// (and to bo->n_frags, which the caller has zeroed).
static int run_filter(tgsf_text* tx, tgsf_ctx* ctx, uint32_t n_records, uint64_t n_bytes, tgsf_batch_out* bo, tgsf_fragment* d_fr,
                      uint32_t fr_cap, uint32_t* n_frags)
{
    int e;
    *n_frags = 0;
    if (n_records) {
        tgsf_batch_in in;
        memset(&in, 0, sizeof in);
        in.seq = tx->d_text;
        in.qual = tx->d_text;
        in.offsets = tx->d_index.seq_off;
        in.lengths = tx->d_index.len;
        in.qual_offsets = tx->d_index.qual_off;
        in.n_reads = n_records;
        in.n_bytes = n_bytes;
        tgsf_batch_out dout;
        dout.reads = tx->d_reads;
        dout.frags = d_fr;
        dout.frag_capacity = d_fr ? fr_cap : 0u;
        dout.n_frags = 0;
        e = tgsf_submit_device(ctx, &in, &dout, tx->d_nfrags, (void*)tx->stream);
        if (!e) e = tgsf_wait(ctx);
        if (e) return fail(tx, e, "libtgsf: %s", tgsf_last_error(ctx));
        uint32_t nf = 0;
        if ((e = down(tx, &nf, tx->d_nfrags, 4, false))) return e;
        if ((e = down(tx, bo ? bo->reads : nullptr, tx->d_reads, bo ? (size_t)n_records * sizeof(tgsf_read_result) : 0))) return e;
        if (nf > dout.frag_capacity) return fail(tx, TGSF_E_CAPACITY, "batch produced %u fragments, caller provided room for %u", nf, dout.frag_capacity);
        if (nf && bo && bo->frags && (e = down(tx, bo->frags, d_fr, (size_t)nf * sizeof(tgsf_fragment)))) return e;
        if (bo) bo->n_frags = nf;
        *n_frags = nf;
    }
    return TGSF_OK;
}

// fragment records on the device for a caller who takes them: as many as the caller takes
static int grow_frags(tgsf_text* tx, const tgsf_batch_out* bo)
{
    if (bo->frags && bo->frag_capacity > tx->frag_cap) {
        tgsf_fragment* f = nullptr;
        if (dev_alloc(tx, &f, bo->frag_capacity)) return fail(tx, TGSF_E_HIP, "device allocation failed (%u fragment records)", bo->frag_capacity);
        tx->d_frags = f;                                               // (the smaller one stays allocated until destroy)
        tx->frag_cap = bo->frag_capacity;
    }
    return TGSF_OK;
}

// ---- the output side ---------------------------------------------------------------------------------------------------
extern "C" int tgsf_text_out_reserve(tgsf_text* tx, uint32_t max_frags, uint64_t max_out_bytes)
{
    if (!tx) return TGSF_E_INVALID;
    if (tx->out_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_out_reserve has been called already (%u fragments, %llu bytes)", tx->max_frags, (unsigned long long)tx->max_out);
    if (max_frags == 0 || max_out_bytes == 0) return fail(tx, TGSF_E_INVALID, "max_frags and max_out_bytes must be positive");
    (void)rt_set_device(tx->device);
    for (rt_event& ev : tx->oev) if (!ev && rt_event_create(&ev)) return fail(tx, TGSF_E_HIP, "event creation failed");
    const size_t parts = (size_t)max_frags / kTextScanTile + 2;
    int e = 0;
    e |= dev_alloc(tx, &tx->d_out, ((max_out_bytes + 15u) & ~15ull));
    if (!e) e |= dev_alloc(tx, &tx->d_opass, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_opass_part, parts);
    if (!e) e |= dev_alloc(tx, &tx->d_osize, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_osize_part, parts);
    if (!e) e |= dev_alloc(tx, &tx->d_oends, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_ometa, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_ostate, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_ofrags, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_orec_end, max_frags);
    if (!e) e |= dev_alloc(tx, &tx->d_osummary, 1);
    if (e) return fail(tx, TGSF_E_HIP, "device allocation failed (%u fragments, %llu bytes of output)", max_frags, (unsigned long long)max_out_bytes);
    tx->max_frags = max_frags;
    tx->max_out = max_out_bytes;
    tx->out_reserved = true;
    return TGSF_OK;
}

// what every format call is refused for before anything is enqueued
static int check_format(tgsf_text* tx, uint32_t n_frags, int fasta, int fastq_out)
{
    if (!tx->out_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_out_reserve has not been called on this object: no scratch to format with");
    if (n_frags > tx->max_frags) return fail(tx, TGSF_E_CAPACITY, "%u fragments, the output side was reserved for %u", n_frags, tx->max_frags);
    if ((fasta != 0 && fasta != 1) || (fastq_out != 0 && fastq_out != 1)) return fail(tx, TGSF_E_INVALID, "fasta and fastq_out are 0 or 1");
    if (fasta && fastq_out) return fail(tx, TGSF_E_INVALID, "FASTQ output from a FASTA index: the records have no qualities");
    return TGSF_OK;
}

// the launches of one format, on st; nothing is waited for
static int enqueue_format(tgsf_text* tx, const uint8_t* d_text, const tgsf_text_index_arrays& I, const tgsf_read_result* d_reads,
                          const tgsf_fragment* d_frags, uint32_t n_frags, int fastq_out, uint8_t* d_out, uint64_t capacity,
                          uint64_t* d_rec_end, tgsf_text_out_summary* d_summary, rt_stream st)
{
    const uint64_t n = n_frags;
    const unsigned gfrag = grid_cap(std::min(std::max(blocks_for(n, kTextThreads), 1u), 2048u));
    const unsigned gcopy = wave_grid((capacity + kTextPiece - 1) / kTextPiece);   // a wave per 4 KiB piece of the output, as many as the capacity has
    TextOutState* S = tx->d_ostate;
    if (tx->profile) (void)rt_event_record(tx->oev[0], st);
    TGSF_LAUNCH(k_textout_flag, gfrag, kTextThreads, st, d_frags, n, tx->d_opass, S);
    enqueue_scan(st, tx->d_opass, n, tx->d_opass_part, &S->n_records);
    if (n)
        TGSF_LAUNCH(k_textout_size, gfrag, kTextThreads, st, d_text, I, d_reads, d_frags, n, fastq_out, (const uint32_t*)tx->d_opass,
                    (const uint64_t*)tx->d_opass_part, tx->d_osize, tx->d_ometa, S);
    if (tx->profile) (void)rt_event_record(tx->oev[1], st);
    enqueue_scan(st, tx->d_osize, n, tx->d_osize_part, &S->n_bytes);
    TGSF_LAUNCH(k_textout_finish, gfrag, kTextThreads, st, (const uint64_t*)tx->d_osize, (const uint64_t*)tx->d_osize_part,
                (const uint32_t*)tx->d_opass, (const uint64_t*)tx->d_opass_part, (const TextOutMeta*)tx->d_ometa, n, capacity,
                (const TextOutState*)S, tx->d_oends, d_rec_end, d_summary);
    if (tx->profile) (void)rt_event_record(tx->oev[2], st);
    if (n)
        TGSF_LAUNCH(k_textout_copy, gcopy, kTextThreads, st, d_text, I, d_frags, (const TextOutMeta*)tx->d_ometa, (const uint64_t*)tx->d_oends,
                    n, fastq_out, (const TextOutState*)S, capacity, d_out);
    if (tx->profile) { (void)rt_event_record(tx->oev[3], st); tx->oev_recorded = true; }
    return launched(tx);
}

// milliseconds of the last format's stages; ms[3] (may be NULL); returns their sum.  The format has finished.
static float format_ms(tgsf_text* tx, float* ms)
{
    float sum = 0.0f;
    if (ms) ms[0] = ms[1] = ms[2] = 0.0f;
    if (tx->profile && tx->oev_recorded) {
        for (int k = 0; k < 3; k++) {
            float t = 0.0f;
            if (rt_event_ms(&t, tx->oev[k], tx->oev[k + 1])) { (void)rt_last_error(); return 0.0f; }
            if (ms) ms[k] = t;
            sum += t;
        }
    }
    return sum;
}

extern "C" int tgsf_text_out_stage_ms(tgsf_text* tx, float ms[3])
{
    if (!tx) return TGSF_E_INVALID;
    if (!ms) return fail(tx, TGSF_E_INVALID, "null argument");
    (void)rt_set_device(tx->device);
    if (tx->profile && tx->oev_recorded && rt_event_sync(tx->oev[3])) return fail(tx, TGSF_E_HIP, "waiting for the format failed");
    (void)format_ms(tx, ms);
    return TGSF_OK;
}

extern "C" int tgsf_text_format_device(tgsf_text* tx, const uint8_t* d_text, const tgsf_text_index_arrays* d_index, uint32_t n_records,
                                       int fasta, const tgsf_read_result* d_reads, const tgsf_fragment* d_frags, uint32_t n_frags,
                                       int fastq_out, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_rec_end,
                                       tgsf_text_out_summary* d_summary, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    int e = check_format(tx, n_frags, fasta, fastq_out);
    if (e) return e;
    if (n_frags && (!d_reads || !d_frags || !n_records)) return fail(tx, TGSF_E_INVALID, "fragments without their table or without the per-read records");
    if ((e = check_index(tx, d_index))) return e;
    if (!d_index && n_records > tx->max_records)
        return fail(tx, TGSF_E_CAPACITY, "%u records, the object's index arrays hold %u", n_records, tx->max_records);
    if ((uintptr_t)d_out & 15u) return fail(tx, TGSF_E_INVALID, "the device output buffer must be 16-byte aligned");
    if (!d_out) { d_out = tx->d_out; out_capacity = std::min(out_capacity, tx->max_out); }
    (void)rt_set_device(tx->device);
    return enqueue_format(tx, d_text ? d_text : tx->d_text, d_index ? *d_index : tx->d_index, d_reads, d_frags, n_frags, fastq_out, d_out,
                          out_capacity, d_rec_end, d_summary ? d_summary : tx->d_osummary, stream_of(tx, hip_stream));
}

// where the format calls and the filter calls have the kept records formatted to; gz: as BGZF members (out and out_capacity are
// theirs, the text stays in the object's output buffer; eof: the EOF member behind them; gz_summary may be NULL)
struct FormatTo {
    int fastq_out;
    uint8_t* out;
    uint64_t out_capacity;
    uint64_t* rec_end;
    tgsf_text_out_summary* out_summary;
    int gz, eof;
    tgsf_text_gzout_summary* gz_summary;
};
static int check_gzout(tgsf_text* tx, uint64_t n_bytes, int eof);
static int gzout_down(tgsf_text* tx, const uint8_t* d_in, uint64_t n_bytes, int eof, uint8_t* out, uint64_t out_capacity, uint64_t* member_end,
                      tgsf_text_gzout_summary* out_summary);

// format what is on the device into the object's output buffer, on its stream; summary, text and record ends come down -- or,
// with to.gz, the summary and the text's BGZF members
static int format_down(tgsf_text* tx, const tgsf_read_result* d_reads, const tgsf_fragment* d_frags, uint32_t n_frags, const FormatTo& to)
{
    uint8_t* const out = to.out;
    uint64_t* const rec_end = to.gz ? nullptr : to.rec_end;
    tgsf_text_out_summary* const out_summary = to.out_summary;
    const uint64_t out_capacity = to.gz ? tx->max_out : to.out_capacity;
    const uint64_t cap = std::min(out_capacity, tx->max_out);
    int e = enqueue_format(tx, tx->d_text, tx->d_index, d_reads, d_frags, n_frags, to.fastq_out, tx->d_out, cap, rec_end ? tx->d_orec_end : nullptr,
                           tx->d_osummary, tx->stream);
    if (e) return e;
    tgsf_text_out_summary sum;
    if ((e = down(tx, &sum, tx->d_osummary, sizeof sum))) return e;
    sum.device_ms = format_ms(tx, nullptr);
    *out_summary = sum;
    if (sum.stop == TGSF_TEXT_CAPACITY)
        return fail(tx, TGSF_E_CAPACITY, "the formatted text has %llu bytes, there is room for %llu (out_capacity %llu, reserved %llu)",
                    (unsigned long long)sum.n_bytes, (unsigned long long)cap, (unsigned long long)out_capacity, (unsigned long long)tx->max_out);
    if (to.gz) {
        if ((e = check_gzout(tx, sum.n_bytes, to.eof))) return e;
        return gzout_down(tx, tx->d_out, sum.n_bytes, to.eof, out, to.out_capacity, nullptr, to.gz_summary);
    }
    if ((e = down(tx, out, tx->d_out, (size_t)sum.n_bytes, false))) return e;
    return down(tx, rec_end, tx->d_orec_end, rec_end ? (size_t)sum.n_records * 8 : 0);
}

extern "C" int tgsf_text_format(tgsf_text* tx, uint32_t n_records, int fasta, const tgsf_read_result* reads, const tgsf_fragment* frags,
                                uint32_t n_frags, int fastq_out, uint8_t* out, uint64_t out_capacity, uint64_t* rec_end,
                                tgsf_text_out_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    int e = check_format(tx, n_frags, fasta, fastq_out);
    if (e) return e;
    if (!out_summary || (!out && out_capacity) || (n_frags && (!reads || !frags || !n_records))) return fail(tx, TGSF_E_INVALID, "null argument: summary, output buffer or tables");
    if (n_records > tx->max_records) return fail(tx, TGSF_E_CAPACITY, "%u records, the object's index arrays hold %u", n_records, tx->max_records);
    (void)rt_set_device(tx->device);
    int he = 0;
    if (n_frags) {
        he |= rt_h2d(tx->d_reads, reads, (size_t)n_records * sizeof(tgsf_read_result), tx->stream);
        he |= rt_h2d(tx->d_ofrags, frags, (size_t)n_frags * sizeof(tgsf_fragment), tx->stream);
    }
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    return format_down(tx, tx->d_reads, tx->d_ofrags, n_frags, {fastq_out, out, out_capacity, rec_end, out_summary});
}

// ---- the BAM input side --------------------------------------------------------------------------------------------------
extern "C" int tgsf_text_bam_header(const uint8_t* bam, uint64_t n_bytes, uint64_t* records_at)
{
    if (!records_at || (!bam && n_bytes)) return fail(nullptr, TGSF_E_INVALID, "null argument");
    *records_at = 0;
    uint64_t at = 4;
    auto need = [&](uint64_t k) { return at + k <= n_bytes; };
    if (n_bytes < 4) return fail(nullptr, TGSF_E_DATA, "truncated BAM header: %llu bytes", (unsigned long long)n_bytes);
    if (memcmp(bam, "BAM\1", 4) != 0) return fail(nullptr, TGSF_E_DATA, "not BAM: the magic \"BAM\\1\" is missing");
    if (!need(4)) return fail(nullptr, TGSF_E_DATA, "truncated BAM header: l_text is not complete");
    const uint32_t l_text = bam_le32(bam + at); at += 4;
    if (!need((uint64_t)l_text + 4)) return fail(nullptr, TGSF_E_DATA, "truncated BAM header: %u bytes of text are not complete", l_text);
    at += l_text;
    const uint32_t n_ref = bam_le32(bam + at); at += 4;
    for (uint32_t i = 0; i < n_ref; i++) {
        if (!need(4)) return fail(nullptr, TGSF_E_DATA, "truncated BAM reference list: entry %u of %u", i, n_ref);
        const uint32_t l_name = bam_le32(bam + at); at += 4;
        if (!need((uint64_t)l_name + 4)) return fail(nullptr, TGSF_E_DATA, "truncated BAM reference list: entry %u of %u", i, n_ref);
        at += (uint64_t)l_name + 4;
    }
    *records_at = at;
    return TGSF_OK;
}

extern "C" int tgsf_text_bam_walk(const uint8_t* bam, uint64_t n_bytes, int final, uint32_t max_records, uint64_t* rec_off, uint32_t* n,
                                  uint32_t* stop, uint64_t* consumed)
{
    if (!rec_off || !n || !stop || !consumed || (!bam && n_bytes)) return fail(nullptr, TGSF_E_INVALID, "null argument");
    if (final != 0 && final != 1) return fail(nullptr, TGSF_E_INVALID, "final is 0 or 1");
    uint64_t at = 0;
    uint32_t k = 0, why = TGSF_TEXT_END;
    for (;;) {
        rec_off[k] = at;
        if (at == n_bytes) break;                                      // nothing is left
        if (k == max_records) { why = TGSF_TEXT_CAPACITY; break; }
        if (n_bytes - at < 4) { why = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        const uint32_t block = bam_le32(bam + at);
        if (block < 32u) { why = TGSF_TEXT_IRREGULAR; break; }
        if (n_bytes - at - 4 < block) { why = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END; break; }
        at += 4ull + block;
        k++;
    }
    *n = k;
    *stop = why;
    *consumed = at;
    return TGSF_OK;
}

extern "C" int tgsf_text_bam_reserve(tgsf_text* tx, uint64_t max_bam_bytes)
{
    if (!tx) return TGSF_E_INVALID;
    if (tx->bam_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bam_reserve has been called already (%llu bytes of BAM)", (unsigned long long)tx->max_bam);
    if (max_bam_bytes == 0) return fail(tx, TGSF_E_INVALID, "max_bam_bytes must be positive");
    (void)rt_set_device(tx->device);
    const size_t m = tx->max_records;
    int e = 0;
    e |= dev_alloc(tx, &tx->d_bam, ((max_bam_bytes + 15u) & ~15ull) + TGSF_TEXT_PAD);
    if (!e) e |= dev_alloc(tx, &tx->d_brec_off, m + 1);
    if (!e) e |= dev_alloc(tx, &tx->d_bsize, m);
    if (!e) e |= dev_alloc(tx, &tx->d_bsize_part, m / kTextScanTile + 2);
    if (!e) e |= dev_alloc(tx, &tx->d_bends, m);
    if (!e) e |= dev_alloc(tx, &tx->d_boseq, m);
    if (!e) e |= dev_alloc(tx, &tx->d_bstate, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_bsummary, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_bwalk, m + 3);
    if (e) return fail(tx, TGSF_E_HIP, "device allocation failed (%llu bytes of BAM, %u records)", (unsigned long long)max_bam_bytes, tx->max_records);
    tx->h_rec_off.resize(m + 1);
    tx->h_bwalk.resize(m + 3);
    tx->max_bam = max_bam_bytes;
    tx->bam_reserved = true;
    return TGSF_OK;
}

// what every decode is refused for before anything is copied or enqueued
static int check_bam(tgsf_text* tx, uint64_t n_bytes, int final)
{
    if (!tx->bam_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bam_reserve has not been called on this object: no buffers to decode with");
    if (final != 0 && final != 1) return fail(tx, TGSF_E_INVALID, "final is 0 or 1");
    if (n_bytes > tx->max_bam)
        return fail(tx, TGSF_E_CAPACITY, "BAM chunk of %llu bytes, the object was reserved for %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_bam);
    return TGSF_OK;
}

// the offsets up and the eight launches of one decode, on st; nothing is waited for
static int enqueue_bam(tgsf_text* tx, const uint8_t* d_bam, const uint64_t* rec_off, uint32_t n_walked, uint32_t walk_stop,
                       const tgsf_text_index_arrays& I, tgsf_text_bam_summary* d_summary, rt_stream st)
{
    const uint64_t n = n_walked;
    const unsigned grec = grid_cap(std::min(std::max(blocks_for(n, kTextThreads), 1u), 2048u));
    const unsigned gfold = std::min(grec, 64u);                                    // every wave ends in two atomics on one word each
    const unsigned gtext = wave_grid((tx->max_bytes + TGSF_TEXT_PAD + kTextPiece - 1) / kTextPiece);   // a wave per 4 KiB piece of the text, as many as the object's buffer has
    const int he = rt_h2d(tx->d_brec_off, rec_off, (size_t)(n + 1) * 8, st);
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    BamState* S = tx->d_bstate;
    if (tx->profile) tx->ev.begin(st);
    TGSF_LAUNCH_COOP(k_bam_reset, 1, 64, st, S);
    if (n) {
        TGSF_LAUNCH(k_bam_heads, grec, kTextThreads, st, d_bam, (const uint64_t*)tx->d_brec_off, n_walked, tx->d_bsize, tx->d_boseq, I, S);
        enqueue_scan(st, tx->d_bsize, n, tx->d_bsize_part, &S->total);
        TGSF_LAUNCH(k_bam_layout, grec, kTextThreads, st, (const uint64_t*)tx->d_bsize, (const uint64_t*)tx->d_bsize_part, n_walked, tx->max_bytes, S,
                    tx->d_bends, I);
        TGSF_LAUNCH(k_text_fold<BamState>, gfold, kTextThreads, st, (const uint32_t*)I.len, n_walked, 0, S);
    }
    TGSF_LAUNCH_COOP(k_bam_finish, 1, 64, st, (const uint64_t*)tx->d_brec_off, (const uint64_t*)tx->d_bends, n_walked, walk_stop, (const BamState*)S, d_summary);
    TGSF_LAUNCH(k_bam_unpack, gtext, kTextThreads, st, d_bam, (const uint64_t*)tx->d_brec_off, (const uint32_t*)tx->d_boseq, I,
                (const uint64_t*)tx->d_bends, d_summary, tx->d_text);
    if (tx->profile) tx->ev.end(st);
    return launched(tx);
}

extern "C" int tgsf_text_bam_decode_device(tgsf_text* tx, const uint8_t* d_bam, uint64_t n_bytes, int final, const uint64_t* rec_off,
                                           uint32_t n_walked, uint32_t walk_stop, const tgsf_text_index_arrays* d_index,
                                           tgsf_text_bam_summary* d_summary, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    int e = check_bam(tx, n_bytes, final);
    if (e) return e;
    if (!rec_off) return fail(tx, TGSF_E_INVALID, "null argument: the record offsets of tgsf_text_bam_walk");
    if (walk_stop > TGSF_TEXT_CAPACITY) return fail(tx, TGSF_E_INVALID, "walk_stop is one of TGSF_TEXT_END, _IRREGULAR, _CAPACITY");
    if (n_walked > tx->max_records) return fail(tx, TGSF_E_CAPACITY, "%u records walked, the object was created for %u", n_walked, tx->max_records);
    if (rec_off[n_walked] > n_bytes) return fail(tx, TGSF_E_INVALID, "the record offsets end at byte %llu of %llu", (unsigned long long)rec_off[n_walked], (unsigned long long)n_bytes);
    if ((e = check_index(tx, d_index))) return e;
    (void)rt_set_device(tx->device);
    return enqueue_bam(tx, d_bam ? d_bam : tx->d_bam, rec_off, n_walked, walk_stop, d_index ? *d_index : tx->d_index,
                       d_summary ? d_summary : tx->d_bsummary, stream_of(tx, hip_stream));
}

// the chain walk on the device, on the object's stream; one copy and one wait bring n, stop, consumed and the offsets down
static int bam_walk_down(tgsf_text* tx, const uint8_t* d_bam, uint64_t start, uint64_t n_bytes, int final, uint64_t* rec_off, uint32_t* n,
                         uint32_t* stop, uint64_t* consumed)
{
    static_assert(sizeof(BamWalkHead) == 16, "the head is two of the table's words");
    TGSF_LAUNCH_COOP(k_bam_walk, 1, 64, tx->stream, d_bam, start, n_bytes, final, tx->max_records, (BamWalkHead*)tx->d_bwalk, tx->d_bwalk + 2);
    if (launched(tx)) return TGSF_E_HIP;
    // a walked record has 36 bytes or more: the head and as many offsets as the bytes can hold records, and one
    const uint64_t most = std::min<uint64_t>(tx->max_records, (n_bytes - start) / 36u);
    const int e = down(tx, tx->h_bwalk.data(), tx->d_bwalk, (size_t)(2 + most + 1) * 8);
    if (e) return e;
    BamWalkHead head;
    memcpy(&head, tx->h_bwalk.data(), sizeof head);
    memcpy(rec_off, tx->h_bwalk.data() + 2, ((size_t)head.n + 1) * 8);
    *n = head.n;
    *stop = head.stop;
    *consumed = head.consumed;
    return TGSF_OK;
}

extern "C" int tgsf_text_bam_walk_device(tgsf_text* tx, const uint8_t* d_bam, uint64_t start, uint64_t n_bytes, int final, uint64_t* rec_off,
                                         uint32_t* n, uint32_t* stop, uint64_t* consumed)
{
    if (!tx) return TGSF_E_INVALID;
    if (!rec_off || !n || !stop || !consumed) return fail(tx, TGSF_E_INVALID, "null argument");
    if (!tx->bam_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bam_reserve has not been called on this object: no table to walk into");
    if (final != 0 && final != 1) return fail(tx, TGSF_E_INVALID, "final is 0 or 1");
    if (start > n_bytes) return fail(tx, TGSF_E_INVALID, "the walk starts at byte %llu of %llu", (unsigned long long)start, (unsigned long long)n_bytes);
    if (!d_bam && n_bytes > tx->max_bam)
        return fail(tx, TGSF_E_CAPACITY, "BAM chunk of %llu bytes, the object was reserved for %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_bam);
    (void)rt_set_device(tx->device);
    return bam_walk_down(tx, d_bam ? d_bam : tx->d_bam, start, n_bytes, final, rec_off, n, stop, consumed);
}

// the decode of the records walked into h_rec_off, from the object's BAM buffer, on the object's stream; the summary comes down (a wait)
static int bam_summary_down(tgsf_text* tx, uint32_t n_walked, uint32_t walk_stop, tgsf_text_bam_summary* sum)
{
    int e = enqueue_bam(tx, tx->d_bam, tx->h_rec_off.data(), n_walked, walk_stop, tx->d_index, tx->d_bsummary, tx->stream);
    if (!e) e = down(tx, sum, tx->d_bsummary, sizeof *sum);
    if (e) return e;
    sum->device_ms = tx->ev.ms(tx->profile);
    return TGSF_OK;
}

// walk, upload, decode on the object's stream; the summary comes down (the one wait)
static int bam_decode_down(tgsf_text* tx, const uint8_t* bam, uint64_t n_bytes, int final, tgsf_text_bam_summary* sum)
{
    uint32_t n_walked = 0, walk_stop = 0;
    uint64_t consumed = 0;
    int e = tgsf_text_bam_walk(bam, n_bytes, final, tx->max_records, tx->h_rec_off.data(), &n_walked, &walk_stop, &consumed);
    if (e) return fail(tx, e, "the walk failed: %s", g_create_error.c_str());
    const int he = n_bytes ? rt_h2d(tx->d_bam, bam, n_bytes, tx->stream) : 0;
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    return bam_summary_down(tx, n_walked, walk_stop, sum);
}

extern "C" int tgsf_text_bam_decode(tgsf_text* tx, const uint8_t* bam, uint64_t n_bytes, int final, const tgsf_text_index_arrays* out_index,
                                    tgsf_text_bam_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out_summary || (!bam && n_bytes)) return fail(tx, TGSF_E_INVALID, "null argument");
    int e = check_bam(tx, n_bytes, final);
    if (e) return e;
    (void)rt_set_device(tx->device);
    tgsf_text_bam_summary sum;
    if ((e = bam_decode_down(tx, bam, n_bytes, final, &sum))) return e;
    if ((e = fetch_index(tx, out_index, sum.n_records))) return e;
    *out_summary = sum;
    return TGSF_OK;
}

// the host refuses the whole input for a quality that decodes to '\n'; here the call, naming the record as the host does
// (rec: the record's block_size field and what follows it, as far as the name reaches)
static int bad_quality(tgsf_text* tx, const uint8_t* rec, const tgsf_text_bam_summary& sum)
{
    const uint8_t* r = rec + 4;
    const char* name = reinterpret_cast<const char*>(r + 32);
    return fail(tx, TGSF_E_DATA, "unsupported quality value in %.*s (record %u of the chunk): the filter has not run", (int)strnlen(name, r[8]), name, sum.bad_qual);
}

// ---- the one path of the nine calls that run the filter: ingest, filter, format ------------------------------------------------
// How the chunk gets into the object and where its summary goes.  Text (text_summary): upload and index; the caller's summary
// is written when the call has succeeded.  BAM (bam_summary): walk, copy up, decode; the text has text_bytes bytes, the
// caller's summary is written before the filter runs, and a quality that decodes to '\n' refuses the chunk.
// Compressed BAM (gz_summary, with bam_summary = &gz_summary->bam, which filter_call sets): the members inflated into the object's BAM buffer, the
// chain walked there from byte `skip` on, then the decode as for BAM.
struct Ingest {
    const uint8_t* bytes;
    uint64_t n_bytes;
    int fasta, final;
    tgsf_text_summary* text_summary;
    tgsf_text_bam_summary* bam_summary;
    tgsf_text_bgzf_bam_summary* gz_summary;
    uint32_t skip;
};
static int bgzf_bam_decode_down(tgsf_text* tx, const Ingest& in, tgsf_text_bam_summary* bs);

// The chunk into the object, the one wait for the record count (libtgsf sizes its launches by n_reads on the host), the filter,
// the index down last (the filter does not wait for it); with `to` the kept records as text.  The arguments have been checked.
static int ingest_filter_format(tgsf_text* tx, tgsf_ctx* ctx, const Ingest& in, const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo,
                                const FormatTo* to)
{
    int e;
    (void)rt_set_device(tx->device);
    const bool takes = bo && bo->frags;                                // the caller takes the fragments: its capacity counts
    if (takes && (e = grow_frags(tx, bo))) return e;
    tgsf_fragment* d_fr = takes ? tx->d_frags : (to ? tx->d_ofrags : nullptr);
    const uint32_t fr_cap = takes ? bo->frag_capacity : (to ? tx->max_frags : 0u);
    if (to) memset(to->out_summary, 0, sizeof *to->out_summary);
    if (to && to->gz_summary) memset(to->gz_summary, 0, sizeof *to->gz_summary);
    tgsf_text_summary ts;
    tgsf_text_bam_summary bs;
    if (in.bam_summary) {
        if ((e = in.gz_summary ? bgzf_bam_decode_down(tx, in, &bs) : bam_decode_down(tx, in.bytes, in.n_bytes, in.final, &bs))) return e;
        *in.bam_summary = bs;
    } else {
        if ((e = upload(tx, in.bytes, in.n_bytes))) return e;
        if ((e = enqueue_index(tx, tx->d_text, in.n_bytes, in.fasta, in.final, tx->d_index, tx->d_summary, tx->stream))) return e;
        if ((e = fetch(tx, nullptr, nullptr, &ts))) return e;
    }
    const uint32_t n_records = in.bam_summary ? bs.n_records : ts.n_records;
    if (bo) bo->n_frags = 0;
    if (in.bam_summary && bs.bad_qual != 0xFFFFFFFFu) {
        if (!in.gz_summary) return bad_quality(tx, in.bytes + tx->h_rec_off[bs.bad_qual], bs);
        uint8_t rec[4 + 32 + 255] = {0};                               // the record's name is in HBM only
        const uint64_t at = tx->h_rec_off[bs.bad_qual];
        if ((e = down(tx, rec, tx->d_bam + at, (size_t)std::min<uint64_t>(sizeof rec, in.gz_summary->gz.out_bytes - at)))) return e;
        return bad_quality(tx, rec, bs);
    }
    uint32_t nf = 0;
    if ((e = run_filter(tx, ctx, n_records, in.bam_summary ? bs.text_bytes : in.n_bytes, bo, d_fr, fr_cap, &nf))) return e;
    if ((e = fetch_index(tx, out_index, n_records))) return e;
    if (in.text_summary) *in.text_summary = ts;
    if (!to) return TGSF_OK;
    if (!n_records)                                                    // no record: nothing ran, an empty output (or the EOF member alone), no error
        return to->gz ? gzout_down(tx, tx->d_out, 0, to->eof, to->out, to->out_capacity, nullptr, to->gz_summary) : TGSF_OK;
    if (nf > tx->max_frags) return fail(tx, TGSF_E_CAPACITY, "%u fragments, the output side was reserved for %u", nf, tx->max_frags);
    return format_down(tx, tx->d_reads, d_fr, nf, *to);
}

// The nine calls that run the filter: what they are refused for before anything is copied or enqueued -- the input's checks by
// its kind, which the summary that is there tells; to: NULL for the submit forms, whose batch_out is not optional -- then the path.
static int check_bgzf_bam(tgsf_text* tx, uint64_t n_bytes, int final);
static int filter_call(tgsf_text* tx, tgsf_ctx* ctx, Ingest in, const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo, const FormatTo* to)
{
    if (!tx) return TGSF_E_INVALID;
    const bool no_input = !ctx || !(in.text_summary || in.bam_summary || in.gz_summary) || (!in.bytes && in.n_bytes);
    const bool no_output = to ? !to->out_summary || (bo && !bo->reads) || (!to->out && to->out_capacity) : !bo || !bo->reads;
    if (no_input || no_output) return fail(tx, TGSF_E_INVALID, "null argument");
    int e = to ? check_format(tx, 0, in.fasta, to->fastq_out) : TGSF_OK;
    if (!e) e = in.gz_summary ? check_bgzf_bam(tx, in.n_bytes, in.final) : in.bam_summary ? check_bam(tx, in.n_bytes, in.final) : check_args(tx, in.n_bytes, in.fasta, in.final);
    if (!e && to && to->gz) e = check_gzout(tx, 0, to->eof);
    if (e) return e;
    if (in.gz_summary) in.bam_summary = &in.gz_summary->bam;
    return ingest_filter_format(tx, ctx, in, out_index, bo, to);
}

extern "C" int tgsf_text_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final,
                                const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary, tgsf_batch_out* bo)
{
    return filter_call(tx, ctx, {text, n_bytes, fasta, final, out_summary}, out_index, bo, nullptr);
}

extern "C" int tgsf_text_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final, int fastq_out,
                                uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                                tgsf_text_summary* in_summary,
                                const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo)
{
    const FormatTo to = {fastq_out, out, out_capacity, rec_end, out_summary};
    return filter_call(tx, ctx, {text, n_bytes, fasta, final, in_summary}, out_index, bo, &to);
}

extern "C" int tgsf_text_bam_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final,
                                    const tgsf_text_index_arrays* out_index, tgsf_text_bam_summary* out_summary, tgsf_batch_out* bo)
{
    return filter_call(tx, ctx, {bam, n_bytes, 0, final, nullptr, out_summary}, out_index, bo, nullptr);
}

extern "C" int tgsf_text_bam_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final, int fastq_out,
                                    uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                                    tgsf_text_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo)
{
    const FormatTo to = {fastq_out, out, out_capacity, rec_end, out_summary};
    return filter_call(tx, ctx, {bam, n_bytes, 0, final, nullptr, in_summary}, out_index, bo, &to);
}

// ---- the BGZF input side ---------------------------------------------------------------------------------------------------
static uint32_t gz_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

extern "C" int tgsf_text_bgzf_walk(const uint8_t* gz, uint64_t n_bytes, int final, uint32_t max_blocks, uint64_t max_out_bytes,
                                   tgsf_text_bgzf_block* blocks, uint32_t* n, uint32_t* stop, uint64_t* consumed, uint64_t* out_bytes)
{
    if (!n || !stop || !consumed || !out_bytes || (!blocks && max_blocks) || (!gz && n_bytes)) return fail(nullptr, TGSF_E_INVALID, "null argument");
    if (final != 0 && final != 1) return fail(nullptr, TGSF_E_INVALID, "final is 0 or 1");
    uint64_t at = 0, out = 0;
    uint32_t k = 0, why = TGSF_TEXT_END;
    const uint32_t cut = final ? TGSF_TEXT_IRREGULAR : TGSF_TEXT_END;  // the bytes left are the front of a member, as far as they go
    while (at < n_bytes) {
        const uint8_t* p = gz + at;
        const uint64_t left = n_bytes - at;
        const uint8_t magic[4] = {0x1f, 0x8b, 8, 4};
        if (memcmp(p, magic, (size_t)std::min<uint64_t>(left, 4)) != 0) { why = TGSF_TEXT_IRREGULAR; break; }
        if (left < 18) { why = cut; break; }
        const uint64_t xlen = gz_le16(p + 10);
        if (left < 12 + xlen) { why = cut; break; }
        uint64_t bsize = 0;
        for (uint64_t x = 12; x + 4 <= 12 + xlen;) {                   // bgzf_peek's walk of the extra field
            const uint64_t slen = gz_le16(p + x + 2);
            if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = (uint64_t)gz_le16(p + x + 4) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8) { why = TGSF_TEXT_IRREGULAR; break; }
        if (bsize > left) { why = cut; break; }
        const uint32_t usize = bam_le32(p + bsize - 4);
        if (usize > 65536u) { why = TGSF_TEXT_IRREGULAR; break; }
        if (k == max_blocks || usize > max_out_bytes - out) { why = TGSF_TEXT_CAPACITY; break; }
        blocks[k].payload = at + 12 + xlen;
        blocks[k].clen = (uint32_t)(bsize - 12 - xlen - 8);
        blocks[k].usize = usize;
        blocks[k].out = out;
        out += usize;
        at += bsize;
        k++;
    }
    *n = k;
    *stop = why;
    *consumed = at;
    *out_bytes = out;
    return TGSF_OK;
}

extern "C" int tgsf_text_bgzf_reserve(tgsf_text* tx, uint64_t max_gz_bytes, uint32_t max_blocks)
{
    if (!tx) return TGSF_E_INVALID;
    if (tx->gz_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_reserve has been called already (%llu bytes, %u members)", (unsigned long long)tx->max_gz, tx->max_gblocks);
    if (max_gz_bytes == 0 || max_blocks == 0) return fail(tx, TGSF_E_INVALID, "max_gz_bytes and max_blocks must be positive");
    (void)rt_set_device(tx->device);
    int e = 0;
    e |= dev_alloc(tx, &tx->d_gz, ((max_gz_bytes + 15u) & ~15ull) + TGSF_TEXT_PAD);
    if (!e) e |= dev_alloc(tx, &tx->d_gblocks, max_blocks);
    if (!e) e |= dev_alloc(tx, &tx->d_gstate, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_gsummary, 1);
    if (e) return fail(tx, TGSF_E_HIP, "device allocation failed (%llu compressed bytes, %u members)", (unsigned long long)max_gz_bytes, max_blocks);
    tx->h_gblocks.resize(max_blocks);
    tx->max_gz = max_gz_bytes;
    tx->max_gblocks = max_blocks;
    tx->gz_reserved = true;
    return TGSF_OK;
}

// the CRC32 tables of the kernels (GzCrcTables: entry 256 * k + b is the register after byte b and k zero bytes), once per object:
// tgsf_text_bgzf_out_reserve brings them up, or the first CRC check of an object that deflates nothing (4 KiB, one copy, one wait)
struct CrcTables {
    uint32_t t[1024];
    CrcTables()
    {
        for (uint32_t i = 0; i < 1024u; i++) {
            uint32_t c = i & 255u;
            for (uint32_t k = 0; k < 8u * (1u + (i >> 8)); k++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
            t[i] = c;
        }
    }
};
static int crc_tables_up(tgsf_text* tx)
{
    static const CrcTables host;
    if (tx->d_crc_tab) return 0;
    uint32_t* d = nullptr;
    if (dev_alloc(tx, &d, 1024)) return 1;
    int he = rt_h2d(d, host.t, sizeof host.t, tx->stream);
    if (!he) he = rt_sync(tx->stream);
    if (he) return 1;
    tx->d_crc_tab = d;
    return 0;
}

// what every inflate is refused for before anything is copied or enqueued
static int check_bgzf(tgsf_text* tx, uint64_t n_bytes)
{
    if (!tx->gz_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_reserve has not been called on this object: no buffers to inflate with");
    if (n_bytes > tx->max_gz)
        return fail(tx, TGSF_E_CAPACITY, "BGZF chunk of %llu bytes, the object was reserved for %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_gz);
    return TGSF_OK;
}

// the table up and the launches of one inflate, on st; nothing is waited for.  The table has been checked.
static int enqueue_bgzf(tgsf_text* tx, const uint8_t* d_gz, const tgsf_text_bgzf_block* blocks, uint32_t n_blocks, uint32_t walk_stop,
                        uint64_t consumed, uint64_t out_bytes, uint8_t* d_out, tgsf_text_bgzf_summary* d_summary, rt_stream st)
{
    int he = n_blocks ? rt_h2d(tx->d_gblocks, blocks, (size_t)n_blocks * sizeof *blocks, st) : 0;
    if (!he) he = rt_memset(tx->d_gstate, 0xFF, sizeof(BgzfState), st);
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    const unsigned g = wave_grid(n_blocks);                            // a wave per member
    if (tx->profile) tx->ev.begin(st);
    if (n_blocks) TGSF_LAUNCH(k_bgzf_inflate, g, kTextThreads, st, d_gz, (const tgsf_text_bgzf_block*)tx->d_gblocks, n_blocks, d_out, tx->d_gstate);
    TGSF_LAUNCH_COOP(k_bgzf_finish, 1, 64, st, n_blocks, walk_stop, consumed, out_bytes, (const BgzfState*)tx->d_gstate, d_summary);
    if (tx->profile) tx->ev.end(st);
    return launched(tx);
}

// a caller's table against the chunk's size and the rule's bounds: the kernels' bounds are these words.  *out: the inflated
// bytes; *end: the byte behind the last payload.
static int check_block_table(tgsf_text* tx, const tgsf_text_bgzf_block* blocks, uint32_t n_blocks, uint64_t n_bytes, uint64_t* out_bytes, uint64_t* last_end)
{
    uint64_t out = 0, end = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        const tgsf_text_bgzf_block& k = blocks[b];
        if (k.payload < end || k.payload > n_bytes || k.clen > n_bytes - k.payload || k.clen > TGSF_TEXT_BGZF_MAX_CLEN || k.usize > 65536u || k.out != out)
            return fail(tx, TGSF_E_INVALID, "member %u of the block table is not what tgsf_text_bgzf_walk gives for a chunk of %llu bytes", b, (unsigned long long)n_bytes);
        end = k.payload + k.clen;
        out += k.usize;
    }
    *out_bytes = out;
    *last_end = end;
    return TGSF_OK;
}

extern "C" int tgsf_text_bgzf_inflate_device(tgsf_text* tx, const uint8_t* d_gz, uint64_t n_bytes, const tgsf_text_bgzf_block* blocks,
                                             uint32_t n_blocks, uint32_t walk_stop, uint8_t* d_out, uint64_t out_capacity,
                                             tgsf_text_bgzf_summary* d_summary, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    int e = check_bgzf(tx, n_bytes);
    if (e) return e;
    if ((!blocks && n_blocks) || (!d_out && n_blocks)) return fail(tx, TGSF_E_INVALID, "null argument: the block table of tgsf_text_bgzf_walk, or the output");
    if (walk_stop > TGSF_TEXT_CAPACITY) return fail(tx, TGSF_E_INVALID, "walk_stop is one of TGSF_TEXT_END, _IRREGULAR, _CAPACITY");
    if (n_blocks > tx->max_gblocks) return fail(tx, TGSF_E_CAPACITY, "%u members, the object was reserved for %u", n_blocks, tx->max_gblocks);
    if (!d_gz) d_gz = tx->d_gz;
    if ((uintptr_t)d_gz & 15u) return fail(tx, TGSF_E_INVALID, "the compressed bytes on the device must be 16-byte aligned");
    uint64_t out = 0, end = 0;
    if ((e = check_block_table(tx, blocks, n_blocks, n_bytes, &out, &end))) return e;
    if (out > out_capacity) return fail(tx, TGSF_E_CAPACITY, "the members inflate to %llu bytes, there is room for %llu", (unsigned long long)out, (unsigned long long)out_capacity);
    (void)rt_set_device(tx->device);
    return enqueue_bgzf(tx, d_gz, blocks, n_blocks, walk_stop, n_blocks ? end + 8 : 0, out, d_out, d_summary ? d_summary : tx->d_gsummary,
                        stream_of(tx, hip_stream));
}

// What the calls that take compressed bytes from the host share.  gz_walk: the walk into h_gblocks (room: inflated bytes).
// walk_up_inflate, of tgsf_text_bgzf_inflate and tgsf_text_bgzf_verify: their checks, the walk, the refusal of a first member
// that does not fit.  up_inflate: the bytes up, the inflate into d_out enqueued on the object's stream.
struct GzWalk { uint32_t n, stop; uint64_t consumed, out_bytes; };
static int gz_walk(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint64_t room, GzWalk* w)
{
    const int e = tgsf_text_bgzf_walk(gz, n_bytes, final, tx->max_gblocks, room, tx->h_gblocks.data(), &w->n, &w->stop, &w->consumed, &w->out_bytes);
    return e ? fail(tx, e, "the walk failed: %s", g_create_error.c_str()) : TGSF_OK;
}
static int walk_up_inflate(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint64_t room, GzWalk* w)
{
    if (final != 0 && final != 1) return fail(tx, TGSF_E_INVALID, "final is 0 or 1");
    int e = check_bgzf(tx, n_bytes);
    if (!e) e = gz_walk(tx, gz, n_bytes, final, room, w);
    if (e) return e;
    if (!w->n && w->stop == TGSF_TEXT_CAPACITY)
        return fail(tx, TGSF_E_CAPACITY, "the first member does not fit: room for %llu bytes (the text buffer %llu)", (unsigned long long)room, (unsigned long long)tx->max_bytes);
    return TGSF_OK;
}
static int up_inflate(tgsf_text* tx, const uint8_t* gz, const GzWalk& w, uint8_t* d_out)
{
    (void)rt_set_device(tx->device);
    const int he = w.consumed ? rt_h2d(tx->d_gz, gz, w.consumed, tx->stream) : 0;
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    return enqueue_bgzf(tx, tx->d_gz, tx->h_gblocks.data(), w.n, w.stop, w.consumed, w.out_bytes, d_out, tx->d_gsummary, tx->stream);
}
static int bad_member(tgsf_text* tx, uint32_t b, const char* tail = "")
{
    return fail(tx, TGSF_E_DATA, "member %u of the chunk (its DEFLATE stream at byte %llu) does not inflate to its %u bytes%s", b,
                (unsigned long long)tx->h_gblocks[b].payload, tx->h_gblocks[b].usize, tail);
}

extern "C" int tgsf_text_bgzf_inflate(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint8_t* out, uint64_t out_capacity,
                                      tgsf_text_bgzf_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out_summary || (!gz && n_bytes)) return fail(tx, TGSF_E_INVALID, "null argument");
    GzWalk w;
    int e = walk_up_inflate(tx, gz, n_bytes, final, out ? std::min(out_capacity, tx->max_bytes) : tx->max_bytes, &w);
    if (!e) e = up_inflate(tx, gz, w, tx->d_text);
    if (e) return e;
    tgsf_text_bgzf_summary sum;
    if ((e = down(tx, &sum, tx->d_gsummary, sizeof sum, false))) return e;
    if ((e = down(tx, out, tx->d_text, out ? w.out_bytes : 0))) return e;
    sum.device_ms = tx->ev.ms(tx->profile);
    *out_summary = sum;
    return sum.bad_block != 0xFFFFFFFFu ? bad_member(tx, sum.bad_block) : TGSF_OK;
}

// ---- compressed BAM in: the one-call forms, resumed by a BGZF virtual offset ---------------------------------------------------
// walk, upload, inflate into the BAM buffer (the first wait: a bad member ends the call), the chain walk on the device (the
// second), the decode (the third: the record count).  *in.gz_summary is filled as far as the call gets.
static int bgzf_bam_decode_down(tgsf_text* tx, const Ingest& in, tgsf_text_bam_summary* bs)
{
    tgsf_text_bgzf_bam_summary* S = in.gz_summary;
    memset(S, 0, sizeof *S);
    S->gz.bad_block = S->bam.bad_qual = 0xFFFFFFFFu;
    GzWalk w;
    int e = gz_walk(tx, in.bytes, in.n_bytes, in.final, tx->max_bam, &w);
    if (e) return e;
    S->gz.n_blocks = w.n; S->gz.stop = w.stop; S->gz.consumed = w.consumed; S->gz.out_bytes = w.out_bytes;
    if (in.skip > w.out_bytes)
        return fail(tx, TGSF_E_INVALID, "skip is %u, the %u members of the chunk inflate to %llu bytes", in.skip, w.n, (unsigned long long)w.out_bytes);
    if ((e = up_inflate(tx, in.bytes, w, tx->d_bam))) return e;
    if ((e = down(tx, &S->gz, tx->d_gsummary, sizeof S->gz))) return e;
    S->gz.device_ms = tx->ev.ms(tx->profile);
    if (S->gz.bad_block != 0xFFFFFFFFu) return bad_member(tx, S->gz.bad_block, ": nothing was decoded");
    // the records are final only when the file ends here and every byte of the chunk was inflated
    const int rec_final = in.final && w.stop == TGSF_TEXT_END && w.consumed == in.n_bytes;
    uint32_t n_walked = 0, walk_stop = 0;
    uint64_t walked_to = 0;
    if ((e = bam_walk_down(tx, tx->d_bam, in.skip, w.out_bytes, rec_final, tx->h_rec_off.data(), &n_walked, &walk_stop, &walked_to))) return e;
    if ((e = bam_summary_down(tx, n_walked, walk_stop, bs))) return e;
    S->bam = *bs;
    // the virtual offset of the first record that is not indexed: the last member that begins at or in front of it holds it
    S->next_gz = w.consumed;
    S->next_skip = 0;
    if (bs->consumed < w.out_bytes) {
        uint32_t lo = 0, hi = w.n;                                     // the first member that begins behind it
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (tx->h_gblocks[mid].out > bs->consumed) hi = mid; else lo = mid + 1; }
        const uint32_t m = lo - 1;
        S->next_gz = m ? tx->h_gblocks[m - 1].payload + tx->h_gblocks[m - 1].clen + 8 : 0;
        S->next_skip = (uint32_t)(bs->consumed - tx->h_gblocks[m].out);
    }
    // the members of this call were cut short by the object's room and hold no whole record, and the next call would be this
    // one again: named as what it is, a record larger than the object, instead of a chunk to be continued
    if (w.stop == TGSF_TEXT_CAPACITY && bs->n_records == 0 && bs->stop == TGSF_TEXT_END && S->next_gz == 0 && S->next_skip == in.skip)
        bs->stop = S->bam.stop = TGSF_TEXT_CAPACITY;
    return TGSF_OK;
}

// what the three calls are refused for before anything is copied or enqueued
static int check_bgzf_bam(tgsf_text* tx, uint64_t n_bytes, int final)
{
    if (!tx->bam_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bam_reserve has not been called on this object: no buffer to inflate into");
    if (final != 0 && final != 1) return fail(tx, TGSF_E_INVALID, "final is 0 or 1");
    return check_bgzf(tx, n_bytes);
}

extern "C" int tgsf_text_bgzf_bam_decode(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final,
                                         const tgsf_text_index_arrays* out_index, tgsf_text_bgzf_bam_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out_summary || (!gz && n_bytes)) return fail(tx, TGSF_E_INVALID, "null argument");
    int e = check_bgzf_bam(tx, n_bytes, final);
    if (e) return e;
    (void)rt_set_device(tx->device);
    tgsf_text_bam_summary bs;
    if ((e = bgzf_bam_decode_down(tx, {gz, n_bytes, 0, final, nullptr, &out_summary->bam, out_summary, skip}, &bs))) return e;
    return fetch_index(tx, out_index, bs.n_records);
}

extern "C" int tgsf_text_bgzf_bam_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final,
                                         const tgsf_text_index_arrays* out_index, tgsf_text_bgzf_bam_summary* out_summary, tgsf_batch_out* bo)
{
    return filter_call(tx, ctx, {gz, n_bytes, 0, final, nullptr, nullptr, out_summary, skip}, out_index, bo, nullptr);
}

extern "C" int tgsf_text_bgzf_bam_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final, int fastq_out,
                                         uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                                         tgsf_text_bgzf_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo)
{
    const FormatTo to = {fastq_out, out, out_capacity, rec_end, out_summary};
    return filter_call(tx, ctx, {gz, n_bytes, 0, final, nullptr, nullptr, in_summary, skip}, out_index, bo, &to);
}

// ---- the BGZF output side: text in, compressed members out ------------------------------------------------------------------------
extern "C" uint64_t tgsf_text_bgzf_bound(uint64_t n_bytes, int eof)
{
    const uint64_t members = n_bytes / kGzMember + (n_bytes % kGzMember ? 1u : 0u);
    const uint64_t extra = (kGzFrame + 5u) * members + (eof ? kGzEofBytes : 0u);
    return n_bytes > UINT64_MAX - extra ? UINT64_MAX : n_bytes + extra;
}

extern "C" int tgsf_text_bgzf_out_level(tgsf_text* tx, int level)
{
    if (!tx) return TGSF_E_INVALID;
    if (level != 0 && level != 1) return fail(tx, TGSF_E_INVALID, "level is 0 (Huffman-only) or 1 (the match search), not %d", level);
    if (tx->zout_reserved)
        return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_out_reserve has been called already: the level (%d) sizes its scratch and is set before it", tx->zlevel);
    tx->zlevel = level;
    return TGSF_OK;
}

extern "C" int tgsf_text_bgzf_out_level_get(const tgsf_text* tx) { return tx ? tx->zlevel : TGSF_E_INVALID; }

extern "C" int tgsf_text_bgzf_out_reserve(tgsf_text* tx, uint64_t max_in_bytes, uint64_t max_gz_bytes)
{
    if (!tx) return TGSF_E_INVALID;
    if (tx->zout_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_out_reserve has been called already (%llu bytes in, %llu compressed)", (unsigned long long)tx->max_zin, (unsigned long long)tx->max_zout);
    if (max_in_bytes == 0 || max_gz_bytes == 0) return fail(tx, TGSF_E_INVALID, "max_in_bytes and max_gz_bytes must be positive");
    const uint64_t members = (max_in_bytes + kGzMember - 1) / kGzMember;
    if (members >= 0xFFFFFFFFull) return fail(tx, TGSF_E_INVALID, "max_in_bytes of %llu: more members than 32 bits count", (unsigned long long)max_in_bytes);
    (void)rt_set_device(tx->device);
    for (rt_event& ev : tx->zev.e) if (!ev && rt_event_create(&ev)) return fail(tx, TGSF_E_HIP, "event creation failed");
    int e = 0;
    e |= dev_alloc(tx, &tx->d_zin, (max_in_bytes + 15u) & ~15ull);
    if (!e) e |= dev_alloc(tx, &tx->d_zout, (max_gz_bytes + 15u) & ~15ull);
    if (!e) e |= dev_alloc(tx, &tx->d_zmeta, (size_t)members);
    if (!e && tx->zlevel) e |= dev_alloc(tx, &tx->d_zlz, (size_t)members);
    if (!e) e |= dev_alloc(tx, &tx->d_zsize, (size_t)members + 1);
    if (!e) e |= dev_alloc(tx, &tx->d_zsize_part, (size_t)members / kTextScanTile + 2);
    if (!e) e |= dev_alloc(tx, &tx->d_zend, (size_t)members + 1);
    if (!e) e |= dev_alloc(tx, &tx->d_zstate, 1);
    if (!e) e |= dev_alloc(tx, &tx->d_zsummary, 1);
    if (!e) e |= crc_tables_up(tx);
    if (e) return fail(tx, TGSF_E_HIP, "device allocation failed (%llu bytes of text, %llu compressed)", (unsigned long long)max_in_bytes, (unsigned long long)max_gz_bytes);
    tx->max_zin = max_in_bytes;
    tx->max_zout = max_gz_bytes;
    tx->max_zmembers = (uint32_t)members;
    tx->zout_reserved = true;
    return TGSF_OK;
}

// what every deflate is refused for before anything is copied or enqueued
static int check_gzout(tgsf_text* tx, uint64_t n_bytes, int eof)
{
    if (!tx->zout_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_out_reserve has not been called on this object: no scratch to deflate with");
    if (eof != 0 && eof != 1) return fail(tx, TGSF_E_INVALID, "eof is 0 or 1");
    if (n_bytes > tx->max_zin)
        return fail(tx, TGSF_E_CAPACITY, "text of %llu bytes to deflate, the object was reserved for %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_zin);
    return TGSF_OK;
}

// the launches of one deflate, on st; nothing is waited for
static int enqueue_gzout(tgsf_text* tx, const uint8_t* d_in, uint64_t n, int eof, uint8_t* d_out, uint64_t capacity, uint64_t* d_member_end,
                         tgsf_text_gzout_summary* d_summary, rt_stream st)
{
    const uint32_t members = (uint32_t)((n + kGzMember - 1) / kGzMember);
    const unsigned g = wave_grid(members);                             // a wave per member
    GzState* S = tx->d_zstate;
    const int he = rt_memset(S, 0, sizeof *S, st);
    if (he) return fail(tx, TGSF_E_HIP, "device memset failed: %s", rt_errstr(he));
    if (tx->profile) tx->zev.begin(st);
    // level 1: a wave per member as well, two waves a workgroup (a table a wave: LDS)
    const unsigned glz = wave_grid(members, kLzThreads, 4096u);
    if (members) {
        if (tx->zlevel) TGSF_LAUNCH(k_gz_count_lz, glz, kLzThreads, st, d_in, n, members, (const uint32_t*)tx->d_crc_tab, tx->d_zmeta, tx->d_zlz, tx->d_zsize, S);
        else TGSF_LAUNCH(k_gz_count, g, kTextThreads, st, d_in, n, members, (const uint32_t*)tx->d_crc_tab, tx->d_zmeta, tx->d_zsize, S);
    }
    enqueue_scan(st, tx->d_zsize, (uint64_t)members, tx->d_zsize_part, &S->total);
    if (tx->zlevel)
        TGSF_LAUNCH(k_gz_emit_lz, glz, kLzThreads, st, d_in, n, members, eof, (const GzMeta*)tx->d_zmeta, (const GzLzMeta*)tx->d_zlz, (const uint64_t*)tx->d_zsize,
                    (const uint64_t*)tx->d_zsize_part, (const GzState*)S, capacity, d_out, d_member_end, d_summary);
    else
        TGSF_LAUNCH(k_gz_emit, g, kTextThreads, st, d_in, n, members, eof, (const GzMeta*)tx->d_zmeta, (const uint64_t*)tx->d_zsize,
                    (const uint64_t*)tx->d_zsize_part, (const GzState*)S, capacity, d_out, d_member_end, d_summary);
    if (tx->profile) tx->zev.end(st);
    return launched(tx);
}

extern "C" int tgsf_text_bgzf_deflate_device(tgsf_text* tx, const uint8_t* d_in, uint64_t n_bytes, int eof, uint8_t* d_out, uint64_t out_capacity,
                                             uint64_t* d_member_end, tgsf_text_gzout_summary* d_summary, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    const int e = check_gzout(tx, n_bytes, eof);
    if (e) return e;
    if (!d_in) {
        if (!tx->out_reserved) return fail(tx, TGSF_E_INVALID, "no input: d_in is null and tgsf_text_out_reserve has not been called on this object");
        if (n_bytes > tx->max_out) return fail(tx, TGSF_E_CAPACITY, "text of %llu bytes to deflate, the object's output buffer has %llu", (unsigned long long)n_bytes, (unsigned long long)tx->max_out);
        d_in = tx->d_out;
    }
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 15u) return fail(tx, TGSF_E_INVALID, "the device input and the device output buffer must be 16-byte aligned");
    if (!d_out) { d_out = tx->d_zout; out_capacity = std::min(out_capacity, tx->max_zout); }
    (void)rt_set_device(tx->device);
    return enqueue_gzout(tx, d_in, n_bytes, eof, d_out, out_capacity, d_member_end, d_summary ? d_summary : tx->d_zsummary,
                         stream_of(tx, hip_stream));
}

// deflate what is on the device into the object's compressed buffer, on its stream; summary, bytes and member ends come down
static int gzout_down(tgsf_text* tx, const uint8_t* d_in, uint64_t n_bytes, int eof, uint8_t* out, uint64_t out_capacity, uint64_t* member_end,
                      tgsf_text_gzout_summary* out_summary)
{
    const uint64_t cap = std::min(out_capacity, tx->max_zout);
    int e = enqueue_gzout(tx, d_in, n_bytes, eof, tx->d_zout, cap, member_end ? tx->d_zend : nullptr, tx->d_zsummary, tx->stream);
    if (e) return e;
    tgsf_text_gzout_summary sum;
    if ((e = down(tx, &sum, tx->d_zsummary, sizeof sum))) return e;
    sum.device_ms = tx->zev.ms(tx->profile);
    if (out_summary) *out_summary = sum;
    if (sum.stop == TGSF_TEXT_CAPACITY)
        return fail(tx, TGSF_E_CAPACITY, "the compressed text has %llu bytes, there is room for %llu (out_capacity %llu, reserved %llu)",
                    (unsigned long long)sum.n_bytes, (unsigned long long)cap, (unsigned long long)out_capacity, (unsigned long long)tx->max_zout);
    if ((e = down(tx, out, tx->d_zout, (size_t)sum.n_bytes, false))) return e;
    return down(tx, member_end, tx->d_zend, member_end ? (size_t)sum.n_members * 8 : 0);
}

extern "C" int tgsf_text_bgzf_deflate(tgsf_text* tx, const uint8_t* in, uint64_t n_bytes, int eof, uint8_t* out, uint64_t out_capacity,
                                      uint64_t* member_end, tgsf_text_gzout_summary* out_summary)
{
    if (!tx) return TGSF_E_INVALID;
    if (!out_summary || (!in && n_bytes) || (!out && out_capacity)) return fail(tx, TGSF_E_INVALID, "null argument: summary, text or output buffer");
    const int e = check_gzout(tx, n_bytes, eof);
    if (e) return e;
    (void)rt_set_device(tx->device);
    const int he = n_bytes ? rt_h2d(tx->d_zin, in, n_bytes, tx->stream) : 0;
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    return gzout_down(tx, tx->d_zin, n_bytes, eof, out, out_capacity, member_end, out_summary);
}

// ---- the CRC32 of inflated members, for a caller who asks -------------------------------------------------------------------------
// the check of the members in the object's table against their trailers, on st; *d_bad becomes the lowest that differs
static int enqueue_crc(tgsf_text* tx, const uint8_t* d_gz, uint32_t n_blocks, const uint8_t* d_inflated, uint32_t* d_bad, rt_stream st)
{
    const int he = rt_memset(d_bad, 0xFF, 4, st);
    if (he) return fail(tx, TGSF_E_HIP, "device memset failed: %s", rt_errstr(he));
    if (n_blocks)
        TGSF_LAUNCH(k_bgzf_crc, wave_grid(n_blocks), kTextThreads, st, d_gz, (const tgsf_text_bgzf_block*)tx->d_gblocks, n_blocks, d_inflated, (const uint32_t*)tx->d_crc_tab, d_bad);
    return launched(tx);
}

extern "C" int tgsf_text_bgzf_crc_device(tgsf_text* tx, const uint8_t* d_gz, const tgsf_text_bgzf_block* blocks, uint32_t n_blocks,
                                         const uint8_t* d_inflated, uint32_t* d_bad_crc, void* hip_stream)
{
    if (!tx) return TGSF_E_INVALID;
    if (!tx->gz_reserved) return fail(tx, TGSF_E_INVALID, "tgsf_text_bgzf_reserve has not been called on this object: no table to check with");
    if (!d_bad_crc || (!blocks && n_blocks)) return fail(tx, TGSF_E_INVALID, "null argument: the block table of tgsf_text_bgzf_walk, or the result's word");
    if (n_blocks > tx->max_gblocks) return fail(tx, TGSF_E_CAPACITY, "%u members, the object was reserved for %u", n_blocks, tx->max_gblocks);
    const uint64_t room = d_gz ? UINT64_MAX : tx->max_gz;             // (a caller's buffer: the table is the caller's word for its size)
    uint64_t out = 0, end = 0;
    int e = check_block_table(tx, blocks, n_blocks, room, &out, &end);
    if (e) return e;
    if (n_blocks && room - end < 8) return fail(tx, TGSF_E_INVALID, "the last member's trailer lies behind the %llu bytes of the object's buffer", (unsigned long long)room);
    if (!d_inflated && out > tx->max_bytes) return fail(tx, TGSF_E_CAPACITY, "the members inflate to %llu bytes, the text buffer has %llu", (unsigned long long)out, (unsigned long long)tx->max_bytes);
    (void)rt_set_device(tx->device);
    if (crc_tables_up(tx)) return fail(tx, TGSF_E_HIP, "device allocation failed (the CRC32 tables)");
    rt_stream st = stream_of(tx, hip_stream);
    const int he = n_blocks ? rt_h2d(tx->d_gblocks, blocks, (size_t)n_blocks * sizeof *blocks, st) : 0;
    if (he) return fail(tx, TGSF_E_HIP, "host to device copy failed: %s", rt_errstr(he));
    return enqueue_crc(tx, d_gz ? d_gz : tx->d_gz, n_blocks, d_inflated ? d_inflated : tx->d_text, d_bad_crc, st);
}

extern "C" int tgsf_text_bgzf_verify(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint32_t* bad_block, uint32_t* bad_crc)
{
    if (!tx) return TGSF_E_INVALID;
    if (!bad_block || !bad_crc || (!gz && n_bytes)) return fail(tx, TGSF_E_INVALID, "null argument");
    *bad_block = *bad_crc = 0xFFFFFFFFu;
    GzWalk w;
    int e = walk_up_inflate(tx, gz, n_bytes, final, tx->max_bytes, &w);
    if (e) return e;
    // a check that covers a part of the bytes has no way to say so: whatever the walk leaves over refuses the call
    if (w.stop == TGSF_TEXT_IRREGULAR)
        return fail(tx, TGSF_E_DATA, "member %u of the chunk, at byte %llu of %llu, is not a BGZF member%s: nothing was checked", w.n, (unsigned long long)w.consumed,
                    (unsigned long long)n_bytes, final ? ", or is cut short" : "");
    if (w.stop == TGSF_TEXT_CAPACITY)
        return fail(tx, TGSF_E_CAPACITY, "%u members (%llu inflated bytes) fit the object (max_blocks %u, the text buffer %llu) and the chunk goes on at byte %llu: nothing was checked",
                    w.n, (unsigned long long)w.out_bytes, tx->max_gblocks, (unsigned long long)tx->max_bytes, (unsigned long long)w.consumed);
    (void)rt_set_device(tx->device);
    if (crc_tables_up(tx)) return fail(tx, TGSF_E_HIP, "device allocation failed (the CRC32 tables)");
    if ((e = up_inflate(tx, gz, w, tx->d_text))) return e;
    if ((e = enqueue_crc(tx, tx->d_gz, w.n, tx->d_text, &tx->d_gstate->bad_crc, tx->stream))) return e;
    BgzfState S;
    if ((e = down(tx, &S, tx->d_gstate, sizeof S))) return e;
    (void)tx->ev.ms(tx->profile);
    *bad_block = S.bad_block;
    *bad_crc = S.bad_crc;
    if (S.bad_block != 0xFFFFFFFFu) return bad_member(tx, S.bad_block);
    if (S.bad_crc != 0xFFFFFFFFu)
        return fail(tx, TGSF_E_DATA, "member %u of the chunk: the CRC32 of its %u inflated bytes is not the one in its trailer (byte %llu)", S.bad_crc,
                    tx->h_gblocks[S.bad_crc].usize, (unsigned long long)(tx->h_gblocks[S.bad_crc].payload + tx->h_gblocks[S.bad_crc].clen));
    return TGSF_OK;
}

// ---- compressed clean text out: the filter calls with the deflate behind the format ----------------------------------------------
extern "C" int tgsf_text_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final, int fastq_out,
                                     uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary, tgsf_text_summary* in_summary,
                                     const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo, int eof, tgsf_text_gzout_summary* gz_summary)
{
    const FormatTo to = {fastq_out, out, out_capacity, nullptr, out_summary, 1, eof, gz_summary};
    return filter_call(tx, ctx, {text, n_bytes, fasta, final, in_summary}, out_index, bo, &to);
}

extern "C" int tgsf_text_bam_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final, int fastq_out,
                                         uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary, tgsf_text_bam_summary* in_summary,
                                         const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo, int eof, tgsf_text_gzout_summary* gz_summary)
{
    const FormatTo to = {fastq_out, out, out_capacity, nullptr, out_summary, 1, eof, gz_summary};
    return filter_call(tx, ctx, {bam, n_bytes, 0, final, nullptr, in_summary}, out_index, bo, &to);
}

extern "C" int tgsf_text_bgzf_bam_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final, int fastq_out,
                                              uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary,
                                              tgsf_text_bgzf_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* bo,
                                              int eof, tgsf_text_gzout_summary* gz_summary)
{
    const FormatTo to = {fastq_out, out, out_capacity, nullptr, out_summary, 1, eof, gz_summary};
    return filter_call(tx, ctx, {gz, n_bytes, 0, final, nullptr, nullptr, in_summary, skip}, out_index, bo, &to);
}
