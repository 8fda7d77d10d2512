/*
 * tgsf_text.h -- C ABI of libtgsf_text.so: the record index of a chunk of FASTQ / FASTA text, made on the GPU.
 *
 * libtgsf reads sequence and quality lines in place from raw FASTQ text (tgsf_batch_in.qual_offsets with
 * seq == qual, include/tgsf.h); what is left to its caller is finding the line ends and checking the records.
 * This library does that on the device, which reads every byte anyway, and offers the one-call form
 * "text in, filter results out".  It is built on the public ABI of libtgsf only, as libtgsf_rccl is.
 *
 * WHAT IS INDEXED.  Truth is the sequential reader of the command line (tgsfilter_amd/host/fastx.cpp,
 * FastxReader::line / next_fastq / next_fasta: a restatement of the reference's getLine / readFastq / readFasta,
 * src/TGSFilter.cpp:657-760).  That reader resynchronises after a malformed record, line by line; the device does
 * not imitate this.  It applies a rule that every position can check on its own:
 *
 *   - A line ends at '\n'; one '\r' in front of it is not part of the line.  With `final` set, the bytes behind the
 *     last '\n' are a line too (if there are any); otherwise they are an incomplete tail that belongs to the next chunk.
 *   - Lines are grouped from the start of the chunk: four to a group for FASTQ, two for FASTA.  A FASTQ group is
 *     REGULAR when line 0 is not empty and begins with '@', line 1 is not empty, line 2 begins with '+', line 3 is
 *     not empty and as long as line 1.  A FASTA group: line 0 not empty and begins with '>', line 1 not empty.
 *     (A line of 4 GiB or more is never regular: lengths are 32-bit in tgsf_batch_in.)
 *   - The index is the LONGEST PREFIX OF REGULAR GROUPS, at most max_records of them.
 *
 * On such a prefix the sequential reader yields exactly these records, one group each, and started again at
 * `consumed` it yields the rest of its records and its message: the rule never differs from the reader, it only
 * stops early.  The chunk must begin where the reader would begin a record: the start of the input or an earlier
 * call's `consumed`.  After TGSF_TEXT_IRREGULAR the caller reads on from `consumed` with a sequential reader of its
 * own (blank lines, garbage and the reader's messages are its business) and may come back behind that spot.
 *
 * Multi-line FASTA is not read by the reference either: the rule stops there.
 *
 * Conventions as in tgsf.h: plain C, 0 or a negative tgsf_status; calls on one object are serialised by the caller,
 * different objects may be driven from different threads.  No CPU fallback.
 */
#ifndef TGSF_TEXT_H
#define TGSF_TEXT_H

#include "tgsf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TGSF_TEXT_ABI_VERSION 1
#define TGSF_TEXT_PAD 64u  /* bytes of zeros the object keeps behind the text in its own buffer */

/* why the index ends where it ends */
enum {
    TGSF_TEXT_END = 0,        /* nothing is left, or only lines that make no whole group yet (non-final chunk) */
    TGSF_TEXT_IRREGULAR = 1,  /* the group at `consumed` is not regular, or the lines left over in a final chunk make no whole group */
    TGSF_TEXT_CAPACITY = 2    /* max_records records indexed and lines are left */
};

/* 32 bytes */
typedef struct tgsf_text_summary {
    uint32_t n_records;
    uint32_t stop;         /* TGSF_TEXT_*                                                           */
    uint64_t consumed;     /* the byte behind the last indexed record's last line end (0 if none)   */
    uint64_t bases;        /* sum of len over the index                                             */
    uint32_t longest;      /* largest len                                                           */
    float    device_ms;    /* the index kernels by HIP events, when tgsf_text_profile is on and the call synchronises
                              (tgsf_text_index, tgsf_text_submit, tgsf_text_fetch); else 0          */
} tgsf_text_summary;

/*
 * The index, five arrays of n_records entries (room for max_records each).  Offsets are bytes from the start of
 * the chunk.  seq_off / qual_off / len are what tgsf_batch_in takes as offsets / qual_offsets / lengths
 * (FASTA: qual_off == seq_off); name_off is the byte behind '@' / '>', name_len excludes a trailing '\r'.
 * Entries at and behind n_records are undefined.  Host pointers for tgsf_text_index / _submit / _fetch (any of the
 * five may be NULL: not wanted), device pointers for tgsf_text_index_device (all five, 8-byte aligned).
 */
typedef struct tgsf_text_index_arrays {
    uint64_t* seq_off;
    uint64_t* qual_off;
    uint32_t* len;
    uint64_t* name_off;
    uint32_t* name_len;
} tgsf_text_index_arrays;

/* device addresses the object owns (tgsf_text_buffers): the text buffer (16-byte aligned, max_bytes + padding),
 * the index arrays (max_records entries each) and the summary. */
typedef struct tgsf_text_device_buffers {
    uint8_t* text;
    tgsf_text_index_arrays index;
    tgsf_text_summary* summary;
    uint64_t max_bytes;
    uint32_t max_records;
    uint32_t reserved;
} tgsf_text_device_buffers;

typedef struct tgsf_text tgsf_text;

int tgsf_text_abi_version(void);
/* "hip:gfx950" for the product; it refuses a libtgsf of another kind (tgsf_backend()) at tgsf_text_create. */
const char* tgsf_text_backend(void);

/*
 * An indexer on HIP device `device` for chunks of up to max_bytes bytes and up to max_records records a call.
 * It owns a device text buffer (16-byte aligned, as tgsf_submit_device demands), a line-end bit per byte,
 * per-tile counts, the line-end table (4 * max_records positions), the index arrays and a stream.
 */
int tgsf_text_create(int device, uint64_t max_bytes, uint32_t max_records, tgsf_text** out);
void tgsf_text_destroy(tgsf_text* tx);
const char* tgsf_text_last_error(tgsf_text* tx);   /* tx may be NULL: last create error */
int tgsf_text_profile(tgsf_text* tx, int enable);  /* fill tgsf_text_summary.device_ms */
int tgsf_text_buffers(tgsf_text* tx, tgsf_text_device_buffers* out);

/*
 * Index text[0 .. n_bytes) held in HOST memory: the text goes up into the object's buffer (zero-padded by
 * TGSF_TEXT_PAD bytes), is indexed there, index and summary come down.  fasta: 0 FASTQ, 1 FASTA.
 * out_index may be NULL (summary only).  n_bytes > max_bytes: TGSF_E_CAPACITY, nothing is copied.
 */
int tgsf_text_index(tgsf_text* tx, const uint8_t* text, uint64_t n_bytes, int fasta, int final,
                    const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary);

/* Only the copy of tgsf_text_index: text into the object's buffer, padded; returns when it is there. */
int tgsf_text_upload(tgsf_text* tx, const uint8_t* text, uint64_t n_bytes);

/*
 * Everything in HBM already; the kernels are enqueued on `hip_stream` (a hipStream_t; NULL: the object's own
 * stream) and nothing is waited for.  d_text (NULL: the object's buffer) must be 16-byte aligned and readable up to
 * n_bytes rounded up to 16; bytes at and behind n_bytes never influence the result.  d_index NULL: the index stays
 * in the object's own arrays (tgsf_text_buffers), ready to be put into a tgsf_batch_in for tgsf_submit_device;
 * d_summary NULL: the object's own.  One call's scratch is the object's: enqueue the next call on the same stream, or
 * after the first has finished.  n_bytes above max_bytes is refused for a caller's d_text too (the scratch is sized by it).
 */
int tgsf_text_index_device(tgsf_text* tx, const uint8_t* d_text, uint64_t n_bytes, int fasta, int final,
                           const tgsf_text_index_arrays* d_index, tgsf_text_summary* d_summary, void* hip_stream);

/* Waits for the object's stream and copies the object's own index arrays and summary to the host (after
 * tgsf_text_index_device with d_index == NULL and d_summary == NULL on the object's own stream, or on a stream the
 * caller has synchronised).  out_index may be NULL. */
int tgsf_text_fetch(tgsf_text* tx, const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary);

/*
 * Text in, filter results out: the text goes up once, is indexed on the device, ONE small copy and synchronise
 * tells the host n_records (libtgsf sizes its launches on the host: this wait is part of the design), then
 * tgsf_submit_device(ctx) runs with seq = qual = the device text and the device index, tgsf_wait(ctx), and the
 * per-read records, the fragments (batch_out->n_frags is set) and the index come down.  batch_out->reads needs room
 * for max_records entries or for the records the text holds.  ctx must live on the same device; create it with
 * no_qual for FASTA.  What libtgsf refuses -- more records than its max_batch_reads (TGSF_E_CAPACITY), a text larger
 * than the context's max_batch_bases + 16 * max_batch_reads (TGSF_E_CAPACITY: the text's n_bytes is the batch's span, the
 * filter has not run), a read above its max_read_len (TGSF_E_DATA), too few fragment slots (TGSF_E_CAPACITY) -- is handed through with its code and
 * tgsf_last_error(ctx)'s text; the object stays usable.  n_records == 0 is no error: nothing runs, n_frags = 0.
 * Only the regular prefix is filtered: look at out_summary->stop and ->consumed.
 */
int tgsf_text_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final,
                     const tgsf_text_index_arrays* out_index, tgsf_text_summary* out_summary, tgsf_batch_out* batch_out);

#ifdef __cplusplus
}
#endif
#endif /* TGSF_TEXT_H */
