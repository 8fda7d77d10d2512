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
 * THE OUTPUT SIDE (tgsf_text_format*, tgsf_text_filter, further down): the records the filter kept, formatted as clean
 * FASTQ / FASTA text on the device, from the text, the index and the filter's fragment table, all of which sit in HBM already.
 *
 * THE BAM INPUT SIDE (tgsf_text_bam_*, at the end, with its rule): inflated unaligned BAM records are decoded on the device
 * into the object's text buffer as FASTQ text, with the same index; from there everything above works unchanged.
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

#define TGSF_TEXT_ABI_VERSION 2
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

/*
 * ---- the output side: text in, clean text out -------------------------------------------------------------------------
 *
 * THE RULE (tgsfilter_amd/host/record_out.h; the reference's record formatting, src/TGSFilter.cpp:2011-2053, and newSeqName,
 * :1680-1701).  The output is the concatenation, in the order of the fragment table, of one record per fragment with
 * TGSF_FF_PASS:
 *
 *     '@' (fastq_out) or '>'   name'   '\n'   text[seq_off[read] + start .. + len)
 *                              [ "\n+\n"   text[qual_off[read] + start .. + len) ]   (fastq_out only)   '\n'
 *
 * name = text[name_off[read] .. + name_len[read]).  pass_num is 1 for the read's first fragment with TGSF_FF_PASS, 2 for
 * its second and so on (other fragments do not count); name' = name for pass_num 1, else ":" and pass_num in decimal are
 * inserted in front of the first byte of name that is one of " \t\n\v\f\r" (an interior '\r' counts), or appended
 * where there is none.  An empty name is allowed ("@:2\n").  Line ends are '\n' whatever the input used.
 *
 * THE TABLES ARE TRUSTED, as tgsf.h trusts offsets: `reads` has n_records entries whose frag_begin is the index of the
 * read's first fragment in `frags`; the fragments are in the order of their reads (what tgsf_batch_out holds); every
 * fragment has read < n_records, start >= 0 and start + len <= len[read].  This is THE CALLER'S DUTY: the library does not
 * check it, and a table that breaks it makes the kernels read outside the text.
 */

/* 32 bytes */
typedef struct tgsf_text_out_summary {
    uint64_t n_bytes;      /* bytes of the formatted text; with TGSF_TEXT_CAPACITY the size that is needed          */
    uint64_t bases;        /* sum of len over the records                                                           */
    uint32_t n_records;    /* records of the output: fragments with TGSF_FF_PASS                                    */
    uint32_t stop;         /* TGSF_TEXT_END: everything was written.  TGSF_TEXT_CAPACITY: n_bytes > out_capacity and
                              NOTHING was written to the output (nor to rec_end)                                    */
    float    device_ms;    /* the output kernels by HIP events, when tgsf_text_profile is on and the call synchronises
                              (tgsf_text_format, tgsf_text_filter); else 0                                          */
    uint32_t reserved;
} tgsf_text_out_summary;

/*
 * Once, before the first format: per-fragment scratch for up to max_frags fragments a call, the object's own output
 * buffer of max_out_bytes bytes (16-byte aligned) and fragment records on the device.  No later call allocates.
 * A format call before it is TGSF_E_INVALID, one with n_frags > max_frags TGSF_E_CAPACITY, both before anything is
 * enqueued; the object stays usable.  A second call is TGSF_E_INVALID.
 */
int tgsf_text_out_reserve(tgsf_text* tx, uint32_t max_frags, uint64_t max_out_bytes);

/*
 * Everything in HBM; the kernels are enqueued on `hip_stream` (NULL: the object's own stream) and nothing is waited for.
 * d_text / d_index NULL: the object's own buffer and arrays, as tgsf_text_index_device left them.  d_reads (n_records
 * entries) and d_frags (n_frags entries) are the filter's results on the device; n_records and n_frags are host values
 * (the caller has them after tgsf_wait).  fasta: what the index was made with; fastq_out with fasta = 1 is
 * TGSF_E_INVALID (there are no qualities: qual_off == seq_off, which the device cannot tell from a FASTQ index).
 * d_out NULL: the object's own output buffer (out_capacity above max_out_bytes is then cut to it); a caller's d_out
 * must be 16-byte aligned.  No byte at or behind n_bytes is written, none at or behind out_capacity.
 * d_rec_end (optional; room for n_frags entries): entry i becomes the byte behind output record i.
 * d_summary NULL: the object's own.  The scratch is the object's: one call at a time, or all on one stream.
 */
int tgsf_text_format_device(tgsf_text* tx, const uint8_t* d_text, const tgsf_text_index_arrays* d_index, uint32_t n_records,
                            int fasta, const tgsf_read_result* d_reads, const tgsf_fragment* d_frags, uint32_t n_frags,
                            int fastq_out, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_rec_end,
                            tgsf_text_out_summary* d_summary, void* hip_stream);

/*
 * The same with HOST tables and a HOST output buffer, for the text and the index that are in the object (after
 * tgsf_text_upload + tgsf_text_index_device, tgsf_text_index or tgsf_text_submit): the tables go up, the text is
 * formatted into the object's output buffer, the summary and n_bytes bytes come down (and n_records entries of rec_end,
 * which may be NULL).  With TGSF_TEXT_CAPACITY only the summary comes down and the call returns TGSF_E_CAPACITY;
 * out_summary->n_bytes says what is needed (of out_capacity, or of tgsf_text_out_reserve's max_out_bytes).
 */
int tgsf_text_format(tgsf_text* tx, uint32_t n_records, int fasta, const tgsf_read_result* reads, const tgsf_fragment* frags,
                     uint32_t n_frags, int fastq_out, uint8_t* out, uint64_t out_capacity, uint64_t* rec_end,
                     tgsf_text_out_summary* out_summary);

/*
 * Text in, clean text out: exactly tgsf_text_submit (its refusals are handed through unchanged), then the regular
 * prefix's kept records formatted on the device and one copy down (rec_end as for tgsf_text_format; may be NULL).  batch_out may be NULL: the per-read records and the
 * fragments then stay on the device, in the object's scratch (at most max_frags fragments); with batch_out they come
 * down too, as from tgsf_text_submit.  out_index may be NULL.  n_records == 0: nothing runs, out_summary->n_bytes = 0,
 * no error.  Only the regular prefix is filtered: look at in_summary->stop and ->consumed.
 */
int tgsf_text_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final, int fastq_out,
                     uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                     tgsf_text_summary* in_summary,
                     const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out);

/* Milliseconds of the last format's three stages -- sizes (flags, their sums, sizes), layout (the sums of the sizes, the
 * record ends), copy -- when tgsf_text_profile was on; waits for that format to finish. */
int tgsf_text_out_stage_ms(tgsf_text* tx, float ms[3]);

/*
 * ---- the BAM input side: inflated unaligned BAM records in, FASTQ text and its index out ------------------------------
 *
 * THE RULE.  Truth is decode_bam of the command line (tgsfilter_amd/host/bam.cpp, a restatement of the reference's sam_read1
 * loop).  The input is a chunk of INFLATED BAM bytes (BGZF inflation is the caller's) that begins at a record's block_size
 * field -- behind the BAM header (tgsf_text_bam_header) or at an earlier call's `consumed` -- and ends at any byte.
 *
 *   - The record at byte `at`: block_size is the little-endian u32 there, the record the block_size bytes behind it; it is
 *     COMPLETE when at + 4 + block_size <= n_bytes.  l_read_name is its byte 8, n_cigar_op the u16 at byte 12, l_seq the u32
 *     at byte 16, the name starts at byte 32; o_seq = 32 + l_read_name + 4 * n_cigar_op, o_qual = o_seq + (l_seq + 1) / 2.
 *     It is REGULAR when block_size >= 32, o_qual + l_seq <= block_size (in 64 bits) and l_seq > 0.  The name is the bytes from
 *     byte 32 to the first NUL within l_read_name (strnlen; it may be empty).  The flag word, the CIGAR and the auxiliary
 *     fields are skipped, as by the host: reads are never reverse-complemented.
 *   - The decoded text is the concatenation, in input order, of one piece per indexed record:
 *         '@' name '\n' bases '\n' '+' '\n' quals '\n'
 *     bases[k] = T[nibble k] (even k: the high nibble) with the host's and the reference's table (src/TGSFilter.cpp:31)
 *     T = {0,'A','C',0,'G',0,0,0,'T',0,0,0,0,0,0,'N'}: of the codes of "=ACMGRSVTWYHKDBN" only A, C, G, T and N keep a letter,
 *     every other code becomes a NUL byte, as in the reference's output.  quals[k] = (uint8_t)(q[k] + 33): an absent quality
 *     string (all 0xFF) becomes spaces, exactly as in the host.
 *   - The index is the five arrays of tgsf_text_index_arrays with offsets into the decoded text: name_off behind the '@',
 *     seq_off = name_off + name_len + 1, qual_off = seq_off + len + 3, len = l_seq.  After a decode the object is in exactly
 *     the state tgsf_text_index_device leaves it in on the same FASTQ text: tgsf_submit_device, tgsf_text_format* and
 *     tgsf_text_buffers work on it unchanged.
 *   - Indexed is the LONGEST PREFIX OF COMPLETE, REGULAR RECORDS of at most max_records records whose decoded text has at
 *     most max_bytes bytes.  `consumed` is the byte offset of the first record not indexed.
 *   - stop: TGSF_TEXT_END -- nothing is left, or a non-final chunk ends inside a record or inside its block_size (that tail
 *     belongs to the next chunk).  TGSF_TEXT_IRREGULAR -- the record at `consumed` is not regular, or the chunk is final and
 *     the bytes left (1 or more) make no complete record (the host ends its stream silently there, or dies on l_seq == 0:
 *     what to say is the caller's business, as with text).  TGSF_TEXT_CAPACITY -- max_records are indexed and bytes are
 *     left, or the next record's text does not fit max_bytes (n_records may then be 0: one record larger than the object).
 *   - A quality byte of 233 decodes to '\n'; the host refuses the whole input ("unsupported quality value in NAME").  Here
 *     bad_qual is the LOWEST index of an indexed record with such a byte (UINT32_MAX: none) and the text is written as the
 *     rule says; tgsf_text_bam_submit / _filter then return TGSF_E_DATA, naming the record, and the filter does not run.
 *
 * The chain of block_size fields is a dependent load per record: it is walked on the host (tgsf_text_bam_walk, O(records)).
 * Everything a position can check on its own -- the field overrun, l_seq == 0, the name's NUL, the text capacity -- and every
 * byte of the text is the device's.
 */

/* 48 bytes */
typedef struct tgsf_text_bam_summary {
    uint32_t n_records;
    uint32_t stop;         /* TGSF_TEXT_*                                                                    */
    uint64_t consumed;     /* the byte offset, in the chunk, of the first record that is not indexed          */
    uint64_t text_bytes;   /* bytes of the decoded text (TGSF_TEXT_PAD zeros follow them in the buffer)       */
    uint64_t bases;        /* sum of len over the index                                                       */
    uint32_t longest;      /* largest len                                                                     */
    uint32_t bad_qual;     /* the lowest indexed record with a quality byte of 233; UINT32_MAX: none          */
    float    device_ms;    /* the decode kernels by HIP events, when tgsf_text_profile is on and the call synchronises
                              (tgsf_text_bam_decode, _submit, _filter); else 0                                */
    uint32_t reserved;
} tgsf_text_bam_summary;

/* Host only.  bam[0 .. n_bytes) begins with the BAM header: checks the magic "BAM\1", steps over l_text, the text and the
 * reference list; *records_at becomes the offset of the first record's block_size.  TGSF_E_DATA when the magic is wrong or
 * the header is not complete within n_bytes (tgsf_text_last_error(NULL) says which). */
int tgsf_text_bam_header(const uint8_t* bam, uint64_t n_bytes, uint64_t* records_at);

/*
 * Host only: the chain walk.  It reads block_size alone.  rec_off (room for max_records + 1 entries) takes the offsets of
 * the records walked and, as entry *n, the offset behind the last of them (= *consumed).  It stops on block_size < 32
 * (TGSF_TEXT_IRREGULAR), on an incomplete record or fewer than 4 bytes (final: TGSF_TEXT_IRREGULAR, else TGSF_TEXT_END),
 * at max_records with bytes left (TGSF_TEXT_CAPACITY) or at n_bytes (TGSF_TEXT_END).
 */
int tgsf_text_bam_walk(const uint8_t* bam, uint64_t n_bytes, int final, uint32_t max_records, uint64_t* rec_off, uint32_t* n,
                       uint32_t* stop, uint64_t* consumed);

/*
 * Once, before the first decode: the device buffer for chunks of up to max_bam_bytes BAM bytes (16-byte aligned, padded), the
 * record-offset table (max_records + 1) and the per-record scratch.  No later call allocates.  A decode before it is
 * TGSF_E_INVALID, a second call is TGSF_E_INVALID, a chunk of n_bytes > max_bam_bytes TGSF_E_CAPACITY before anything is copied.
 */
int tgsf_text_bam_reserve(tgsf_text* tx, uint64_t max_bam_bytes);

/*
 * BAM bytes in HOST memory: the walk, the bytes and the offsets go up, the text is decoded into the object's own text buffer
 * (TGSF_TEXT_PAD zeros behind it) and its index arrays; the summary and, if wanted, the index come down.
 */
int tgsf_text_bam_decode(tgsf_text* tx, const uint8_t* bam, uint64_t n_bytes, int final, const tgsf_text_index_arrays* out_index,
                         tgsf_text_bam_summary* out_summary);

/*
 * The BAM bytes in HBM already (d_bam NULL: the object's buffer); rec_off[0 .. n_walked] and walk_stop are the HOST results of
 * tgsf_text_bam_walk on the same bytes (trusted, as tgsf.h trusts offsets: every walked record is complete and has
 * block_size >= 32; n_walked <= max_records).  Everything is enqueued on `hip_stream` (NULL: the object's own) and nothing is
 * waited for.  The text always goes to the object's text buffer; d_index NULL: the object's index arrays; d_summary NULL: the
 * object's own.  Bytes of d_bam at and behind n_bytes are never read.  The scratch is the object's: one call at a time, or
 * all on one stream.
 */
int tgsf_text_bam_decode_device(tgsf_text* tx, const uint8_t* d_bam, uint64_t n_bytes, int final, const uint64_t* rec_off,
                                uint32_t n_walked, uint32_t walk_stop, const tgsf_text_index_arrays* d_index,
                                tgsf_text_bam_summary* d_summary, void* hip_stream);

/*
 * tgsf_text_submit / tgsf_text_filter with the decode in place of upload plus index: fasta = 0, the batch's n_bytes is
 * text_bytes.  What libtgsf refuses is handed through unchanged; bad_qual set: TGSF_E_DATA (out_summary / in_summary are
 * filled), the filter has not run, the object stays usable.  fastq_out 0 and 1 both work.
 */
int tgsf_text_bam_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final,
                         const tgsf_text_index_arrays* out_index, tgsf_text_bam_summary* out_summary, tgsf_batch_out* batch_out);
int tgsf_text_bam_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final, int fastq_out,
                         uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                         tgsf_text_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out);

#ifdef __cplusplus
}
#endif
#endif /* TGSF_TEXT_H */
