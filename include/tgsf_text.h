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
 * THE BGZF INPUT SIDE (tgsf_text_bgzf_*, behind it, with its rule): BGZF members -- a .bam file or bgzip'ed FASTQ / FASTA as it is
 * on disk -- are inflated on the device, a wave per member; tgsf_text_bgzf_bam_* are the BAM calls with the compressed bytes.
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
 * loop).  The input is a chunk of INFLATED BAM bytes (inflated by the caller, or by the BGZF input side) that begins at a record's block_size
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

/*
 * ---- the BGZF input side: compressed members in, their inflated bytes out -----------------------------------------------
 *
 * THE RULE.  Truth is bgzf_peek / inflate_members of the command line (tgsfilter_amd/host/bam.cpp), with zlib as the arbiter
 * of what a DEFLATE stream means.  The input is a chunk of the file's bytes as they are on disk that begins at a member --
 * the start of the file or an earlier call's `consumed` -- and ends at any byte.
 *
 *   - A MEMBER at byte `at` starts with 1f 8b 08 04; xlen is the u16 at byte 10.  The extra field is walked as bgzf_peek walks
 *     it: the subfield 'B','C' with slen == 2 gives bsize = u16 + 1, other subfields in front of it or behind it are stepped
 *     over.  It is a member when 18 bytes are there, bsize >= 12 + xlen + 8 and at + bsize <= n_bytes.  payload = at + 12 + xlen,
 *     clen = bsize - 12 - xlen - 8, usize is the u32 in the member's last four bytes.
 *   - STRICTER THAN THE HOST: usize > 65536 is not BGZF and stops the walk as TGSF_TEXT_IRREGULAR.  That bounds everything the
 *     device does for a member.
 *   - The walk's stops: TGSF_TEXT_END -- nothing is left, or a non-final chunk ends inside a member or inside its header.
 *     TGSF_TEXT_IRREGULAR -- the bytes at `consumed` are not a member, or the chunk is final and the bytes left are an
 *     incomplete member.  TGSF_TEXT_CAPACITY -- max_blocks walked and bytes left, or the next member's usize does not fit
 *     max_out_bytes.
 *   - A member is GOOD iff usize == 0 and clen <= 2 (the EOF member: the host does not look at such a payload either), or
 *     zlib's raw inflate of payload[0 .. clen) reaches the end of a final block having produced exactly usize bytes, without
 *     consuming a bit at or behind 8 * clen.  Payload bytes behind the end of the final block are ignored, as by the host.
 *     THE CRC32 IS NOT CHECKED, as by the host.  Everything zlib refuses makes the member BAD: a stored block whose NLEN is
 *     not the complement of LEN; BTYPE 3; HLIT > 286 or HDIST > 30; a repeat code 16 with nothing before it or a repeat that
 *     runs over HLIT + HDIST; no code for symbol 256; an over-subscribed code; an incomplete code other than a single code of
 *     length 1; literal/length symbols 286 and 287, distance symbols 30 and 31, the unused code of an incomplete set; a
 *     distance farther back than the bytes this member has produced; running out of input; a byte beyond usize, or ending
 *     short of it.  (The repeats of the code lengths run across the literal/distance boundary: legal.  A distance alphabet
 *     without any code is legal as long as no length symbol occurs.)
 *   - The inflated bytes of member b are written at out + blocks[b].out, blocks[b].out being the sum of usize of the members
 *     before it.  A BAD member writes nothing outside [out, out + usize) of its own range, and what it leaves inside is
 *     unspecified; every other member's bytes are right.  bad_block is the LOWEST index of a bad member (UINT32_MAX: none).
 *
 * Members are found on the host (tgsf_text_bgzf_walk: headers and trailers only, O(members)); every bit of every payload is
 * the device's, a wave per member.
 */

#define TGSF_TEXT_BGZF_MAX_CLEN 131072u   /* bytes of one member's DEFLATE stream the device form takes: the walk gives less than
                                             65536; 65536 bytes in stored blocks of any size that a sane writer makes fit twice that */

/* 24 bytes */
typedef struct tgsf_text_bgzf_block {
    uint64_t payload;      /* byte offset of the DEFLATE stream in the chunk                */
    uint32_t clen;         /* its bytes                                                     */
    uint32_t usize;        /* ISIZE: the inflated bytes, at most 65536                      */
    uint64_t out;          /* sum of usize of the members before this one                   */
} tgsf_text_bgzf_block;

/* 40 bytes */
typedef struct tgsf_text_bgzf_summary {
    uint32_t n_blocks;
    uint32_t stop;         /* TGSF_TEXT_*: the walk's                                                       */
    uint64_t consumed;     /* compressed bytes: the offset of the first member that is not inflated         */
    uint64_t out_bytes;    /* sum of usize over the members                                                 */
    uint32_t bad_block;    /* the lowest bad member; UINT32_MAX: none                                       */
    float    device_ms;    /* the inflate kernels by HIP events, when tgsf_text_profile is on and the call synchronises
                              (tgsf_text_bgzf_inflate); else 0                                              */
    uint64_t reserved;
} tgsf_text_bgzf_summary;

/* Host only: the member walk, as the rule above says.  blocks has room for max_blocks entries; *n of them are filled. */
int tgsf_text_bgzf_walk(const uint8_t* gz, uint64_t n_bytes, int final, uint32_t max_blocks, uint64_t max_out_bytes,
                        tgsf_text_bgzf_block* blocks, uint32_t* n, uint32_t* stop, uint64_t* consumed, uint64_t* out_bytes);

/*
 * Once, before the first inflate: the device buffer for chunks of up to max_gz_bytes compressed bytes (16-byte aligned,
 * padded), the block table (max_blocks), the state and the summary.  No later call allocates.  An inflate before it is
 * TGSF_E_INVALID, a second call is TGSF_E_INVALID, a chunk of n_bytes > max_gz_bytes or a table of n_blocks > max_blocks
 * TGSF_E_CAPACITY before anything is copied.
 */
int tgsf_text_bgzf_reserve(tgsf_text* tx, uint64_t max_gz_bytes, uint32_t max_blocks);

/*
 * Compressed bytes in HOST memory: the walk (at most max_blocks members, at most min(out_capacity, max_bytes) inflated
 * bytes), the bytes and the table go up, the members are inflated INTO THE OBJECT'S OWN TEXT BUFFER -- the call is capped by
 * max_bytes and OVERWRITES THE TEXT AND INVALIDATES THE INDEX of the last call; in exchange bgzip'ed FASTQ / FASTA is ready for
 * tgsf_text_index_device there (tgsf_text_buffers); a caller who wants neither uses the device form --, the summary and out_bytes bytes come down (out NULL:
 * nothing but the summary comes down, and the room is max_bytes).  A walk that stops for
 * TGSF_TEXT_CAPACITY before its first member (one member larger than the room) is TGSF_E_CAPACITY before anything is
 * enqueued.  A bad member: TGSF_E_DATA naming it; the summary is filled, the other members' bytes have come down.
 */
int tgsf_text_bgzf_inflate(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint8_t* out, uint64_t out_capacity,
                           tgsf_text_bgzf_summary* out_summary);

/*
 * The compressed bytes in HBM already (d_gz NULL: the object's buffer; a caller's must be 16-byte aligned and readable up to
 * n_bytes rounded up to 16; bytes at and behind n_bytes never influence the result).  blocks[0 .. n_blocks) and walk_stop are
 * the HOST results of tgsf_text_bgzf_walk on the same bytes; the table is checked against n_bytes and the rule's bounds
 * (usize <= 65536, clen <= TGSF_TEXT_BGZF_MAX_CLEN, members in order, out the running sum: TGSF_E_INVALID), its last member's out + usize against out_capacity (TGSF_E_CAPACITY), both before anything is enqueued.
 * d_out is any device pointer with out_capacity bytes -- the object's own text buffer for one (tgsf_text_buffers), to be
 * followed by tgsf_text_index_device; d_summary NULL: the object's own.  Everything is enqueued on `hip_stream` (NULL: the
 * object's own) and nothing is waited for.  The table and the state are the object's: one call at a time, or all on one stream.
 */
int tgsf_text_bgzf_inflate_device(tgsf_text* tx, const uint8_t* d_gz, uint64_t n_bytes, const tgsf_text_bgzf_block* blocks,
                                  uint32_t n_blocks, uint32_t walk_stop, uint8_t* d_out, uint64_t out_capacity,
                                  tgsf_text_bgzf_summary* d_summary, void* hip_stream);

/*
 * The chain walk of tgsf_text_bam_walk on BAM bytes that are in HBM (behind a device inflate the block_size chain is not on
 * the host): one lane follows it, applying exactly that walk's rule to d_bam[start .. n_bytes) with the object's max_records;
 * offsets count from d_bam (NULL: the object's BAM buffer).  Runs on the object's stream; n, stop, consumed and
 * rec_off[0 .. n] (room for max_records + 1) come down in one copy and one wait.  tgsf_text_bam_decode_device takes the table
 * as it is.  After tgsf_text_bam_reserve; start > n_bytes is TGSF_E_INVALID.
 */
int tgsf_text_bam_walk_device(tgsf_text* tx, const uint8_t* d_bam, uint64_t start, uint64_t n_bytes, int final, uint64_t* rec_off,
                              uint32_t* n, uint32_t* stop, uint64_t* consumed);

/*
 * COMPRESSED BAM IN: tgsf_text_bam_decode / _submit / _filter with the bytes of the .bam file as they are on disk.  Members
 * and records do not share boundaries, so a chunk is (gz bytes that begin at a member, skip): skip is the number of inflated
 * bytes at the chunk's front that earlier calls consumed -- a BGZF virtual offset.  After tgsf_text_bam_reserve and
 * tgsf_text_bgzf_reserve (and tgsf_text_out_reserve for the filter).
 *   - The members are inflated into the object's BAM buffer: the walk's max_out_bytes is max_bam_bytes.  The record chunk is
 *     inflated[skip .. gz.out_bytes); it is final only when `final` is set and every byte of the chunk was inflated
 *     (gz.stop == TGSF_TEXT_END and gz.consumed == n_bytes).  skip > gz.out_bytes is TGSF_E_INVALID.
 *   - bam.consumed counts inflated bytes from the chunk's first member.  (next_gz, next_skip) is where the next call begins:
 *     the compressed offset, in this chunk, of the member that holds the first record not indexed, and that record's offset
 *     in that member's inflated bytes; (gz.consumed, 0) when every inflated byte was consumed.
 *   - NO PROGRESS IS NAMED: when gz.stop is TGSF_TEXT_CAPACITY (max_blocks or max_bam_bytes cut the members short) and the bytes
 *     inflated hold no whole record from `skip` on, bam.stop is TGSF_TEXT_CAPACITY with n_records == 0 -- one record larger than
 *     the object, as for inflated BAM -- and (next_gz, next_skip) is the pair the call was given: a caller must not loop on it.
 *   - A bad member: TGSF_E_DATA naming it; the summaries are filled (gz), the decode and the filter have not run, the object
 *     stays usable -- the contract of bad_qual, which holds here as it does for tgsf_text_bam_submit / _filter.
 * The BAM header is the caller's, as for inflated BAM: inflate the first members (tgsf_text_bgzf_inflate), call
 * tgsf_text_bam_header, and turn records_at into (member, skip) with the walk's table.
 */
typedef struct tgsf_text_bgzf_bam_summary {     /* 104 bytes */
    tgsf_text_bgzf_summary gz;
    tgsf_text_bam_summary bam;
    uint64_t next_gz;
    uint32_t next_skip;
    uint32_t reserved;
} tgsf_text_bgzf_bam_summary;

int tgsf_text_bgzf_bam_decode(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final,
                              const tgsf_text_index_arrays* out_index, tgsf_text_bgzf_bam_summary* out_summary);
int tgsf_text_bgzf_bam_submit(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final,
                              const tgsf_text_index_arrays* out_index, tgsf_text_bgzf_bam_summary* out_summary, tgsf_batch_out* batch_out);
int tgsf_text_bgzf_bam_filter(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final, int fastq_out,
                              uint8_t* out, uint64_t out_capacity, uint64_t* rec_end, tgsf_text_out_summary* out_summary,
                              tgsf_text_bgzf_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out);

/*
 * ---- the BGZF output side: text in, compressed members out; and the CRC32 of inflated members --------------------------------
 *
 * THE RULE.  Truth is zlib.  The input in[0 .. n_bytes) is cut into members of TGSF_TEXT_BGZF_MEMBER input bytes, bgzip's size;
 * the last member takes the rest; the cuts ignore record boundaries, as bgzip's do.  n_bytes == 0 has no member.  With eof the
 * 28-byte EOF member of the BGZF specification ends the output.
 *
 *   - A member is 1f 8b 08 04 00 00 00 00 00 ff 06 00 'B' 'C' 02 00, BSIZE - 1 (u16), the payload, CRC32 (u32), ISIZE (u32):
 *     26 bytes of framing.  A call is RIGHT iff, for every member, zlib's raw inflate of the payload ends a final block having
 *     produced exactly the member's input bytes and consumed the payload to its last byte, and the trailer holds zlib.crc32 of
 *     those bytes and their number.  gzip.decompress of the whole output then returns the input, and tgsf_text_bgzf_walk
 *     (stricter than gzip) accepts every member.
 *   - THE COMPRESSED BYTES THEMSELVES ARE NOT SPECIFIED.  They may change with the build and differ between the serial
 *     emulation and the device.  The same input through the same build twice gives the same bytes.
 *   - What this build writes: one block per member and no match search -- a dynamic block whose literal/length code is a
 *     complete prefix code of at most 15 bits over the bytes that occur and symbol 256 (two codes of one bit when one byte
 *     value occurs), whose distance code is two codes of one bit, and whose code-length code is constant; or one stored block
 *     whenever the dynamic block would not be smaller.  So no payload exceeds its input by more than 5 bytes, and
 *   - What this build writes at level 1 (tgsf_text_bgzf_out_level; level 0, the default, is the above): still one block per
 *     member, the smallest of three -- a dynamic block of literals and matches, the level-0 dynamic block, one stored block
 *     -- so no member is larger than at level 0.  The smallest match has 3 bytes at distance 1 and 4 bytes at any other
 *     distance; lengths go to 258 and distances to 32768.  A match's source lies inside the member: no distance reaches in
 *     front of the member's first byte, so every member still inflates on its own; and no byte at or behind the member's end
 *     is read for it, so none influences its bytes.  The literal/length code is a complete prefix code of at most 15 bits
 *     over up to 286 symbols, the distance code one over up to 30 (no or one distance in use: two codes of one bit), the
 *     code-length code the same constant one (the run-length symbols 16, 17, 18 are not used).  The parse is a function of
 *     the member's bytes alone, whatever the order in which the lanes of a wave arrive.
 *   - THE BOUND: tgsf_text_bgzf_bound(n_bytes, eof) = n_bytes + 31 * ceil(n_bytes / TGSF_TEXT_BGZF_MEMBER) + (eof ? 28 : 0)
 *     is room enough for every input.
 *   - Members begin at any byte address of the output.  No byte outside [out, out + summary.n_bytes) is written.  When
 *     summary.n_bytes exceeds out_capacity NOTHING is written: stop is TGSF_TEXT_CAPACITY and n_bytes the size that is needed
 *     (n_members and stored count what would have been written).
 *   - member_end[i] is the byte behind member i, the EOF member included: n_members entries, ceil(n_bytes / MEMBER) + 1 at most.
 *
 * The CRC32 is computed on the device by the whole wave that has the member.  The same kernel checks input members:
 * tgsf_text_bgzf_crc_device / tgsf_text_bgzf_verify close what THE RULE of the input side leaves open ("the CRC32 is not
 * checked, as by the host") for a caller who asks; tgsf_text_bgzf_inflate and the composed calls stay as they are.
 */
#define TGSF_TEXT_BGZF_MEMBER 0xFF00u

/* 40 bytes */
typedef struct tgsf_text_gzout_summary {
    uint64_t in_bytes;
    uint64_t n_bytes;      /* compressed bytes; with TGSF_TEXT_CAPACITY the size that is needed                   */
    uint32_t n_members;    /* members written, the EOF member included                                            */
    uint32_t stored;       /* of them stored blocks                                                               */
    uint32_t stop;         /* TGSF_TEXT_END, or TGSF_TEXT_CAPACITY: nothing was written                           */
    float    device_ms;    /* the deflate kernels by HIP events, when tgsf_text_profile is on and the call synchronises; else 0 */
    uint64_t reserved;
} tgsf_text_gzout_summary;

/* Host only.  UINT64_MAX when the sum does not fit 64 bits. */
uint64_t tgsf_text_bgzf_bound(uint64_t n_bytes, int eof);

/*
 * Once, before the first deflate: a staging buffer for inputs of up to max_in_bytes (the host form's), the object's own
 * compressed buffer of max_gz_bytes, per-member scratch (1 KiB a member; at level 1, below, 1280 bytes more).  No later call
 * allocates.  A deflate before it is TGSF_E_INVALID, a second call is TGSF_E_INVALID, an input of n_bytes > max_in_bytes
 * TGSF_E_CAPACITY before anything is copied or enqueued.
 */
int tgsf_text_bgzf_out_reserve(tgsf_text* tx, uint64_t max_in_bytes, uint64_t max_gz_bytes);

/*
 * The coder of every deflate of the object, the composed *_filter_bgzf calls included: 0, Huffman-only (the default: the
 * bytes of a build without this call), or 1, the match search of THE RULE.  Only BEFORE tgsf_text_bgzf_out_reserve, which
 * sizes the scratch: level 1 adds 1280 bytes a member (the two codes of the block of matches; the parse itself is not kept,
 * the second pass repeats it).  After the reserve, for any other level and for a null tx: TGSF_E_INVALID, and the object
 * goes on as it was.  tgsf_text_bgzf_bound and tgsf_text_gzout_summary do not depend on the level.
 */
int tgsf_text_bgzf_out_level(tgsf_text* tx, int level);
/* The level in force; TGSF_E_INVALID for a null tx. */
int tgsf_text_bgzf_out_level_get(const tgsf_text* tx);

/*
 * Everything is in HBM; the work is enqueued on `hip_stream` (NULL: the object's own) and nothing is waited for.  d_in NULL:
 * the object's own output buffer as the last format left it (after tgsf_text_out_reserve, else TGSF_E_INVALID); n_bytes is
 * the caller's value, from tgsf_text_out_summary.  d_out NULL: the object's own compressed buffer, out_capacity capped by
 * max_gz_bytes.  Both pointers must be 16-byte aligned; d_in is read up to n_bytes and not a byte further.  d_member_end
 * (device, optional) and d_summary (device; NULL: the object's own) as THE RULE says.  The scratch is the object's: one call
 * at a time, or all on one stream.
 */
int tgsf_text_bgzf_deflate_device(tgsf_text* tx, const uint8_t* d_in, uint64_t n_bytes, int eof, uint8_t* d_out, uint64_t out_capacity,
                                  uint64_t* d_member_end, tgsf_text_gzout_summary* d_summary, void* hip_stream);

/*
 * The host form: the text goes up, the summary, summary.n_bytes bytes and member_end (optional) come down.  With
 * TGSF_TEXT_CAPACITY only the summary comes down and the call returns TGSF_E_CAPACITY.
 */
int tgsf_text_bgzf_deflate(tgsf_text* tx, const uint8_t* in, uint64_t n_bytes, int eof, uint8_t* out, uint64_t out_capacity,
                           uint64_t* member_end, tgsf_text_gzout_summary* out_summary);

/*
 * The opt-in CRC check of inflated members, after tgsf_text_bgzf_reserve.  blocks[0 .. n_blocks) is the HOST table of
 * tgsf_text_bgzf_walk over the compressed bytes at d_gz (NULL: the object's buffer); d_inflated (NULL: the object's text
 * buffer) holds what tgsf_text_bgzf_inflate_device made of them.  The table is checked as there (TGSF_E_INVALID, TGSF_E_CAPACITY
 * above max_blocks) and goes up; a wave per member takes the CRC32 of its inflated bytes and compares it with the u32 in
 * front of ISIZE.  *d_bad_crc (device) becomes the lowest mismatching member, UINT32_MAX: none.  Enqueued on `hip_stream`
 * (NULL: the object's own); nothing is waited for.  The table on the device is the one the inflate uses: same stream.
 * The first CRC check of an object brings the CRC32 tables up (4 KiB, one copy and one wait on the object's stream), unless
 * tgsf_text_bgzf_out_reserve has; no later one allocates.
 */
int tgsf_text_bgzf_crc_device(tgsf_text* tx, const uint8_t* d_gz, const tgsf_text_bgzf_block* blocks, uint32_t n_blocks,
                              const uint8_t* d_inflated, uint32_t* d_bad_crc, void* hip_stream);

/*
 * The host form of the check: tgsf_text_bgzf_inflate with out == NULL (the walk, the inflate into the text buffer, which it
 * overwrites), then the CRC kernel.  *bad_block as there; *bad_crc the lowest member whose inflated bytes do not match its
 * trailer, UINT32_MAX: none; it is meaningless at or behind a bad member.  TGSF_E_DATA naming the member when either is set.
 * TGSF_OK SAYS THAT EVERY BYTE OF THE CHUNK WAS CHECKED, or, with final == 0, every byte in front of a last member that is
 * cut short.  The call has no summary to say "so far", so whatever else the walk leaves over refuses it before anything is
 * copied or enqueued (both words stay UINT32_MAX): a walk that stops as TGSF_TEXT_IRREGULAR -- bytes that are not a member
 * (a damaged header, garbage behind the last member), or with final == 1 a member that is cut short -- is TGSF_E_DATA naming
 * the member and the byte where it stopped; a walk that stops as TGSF_TEXT_CAPACITY (more members than max_blocks, or more
 * inflated bytes than the text buffer) is TGSF_E_CAPACITY saying how many members fit and where the chunk goes on: a caller
 * cuts there (tgsf_text_bgzf_walk) and checks piece by piece with final == 0.
 */
int tgsf_text_bgzf_verify(tgsf_text* tx, const uint8_t* gz, uint64_t n_bytes, int final, uint32_t* bad_block, uint32_t* bad_crc);

/*
 * COMPRESSED CLEAN TEXT OUT: tgsf_text_filter, tgsf_text_bam_filter and tgsf_text_bgzf_bam_filter with the deflate behind the
 * format.  The arguments of their counterparts without rec_end (record ends mean nothing in compressed bytes), plus eof and
 * gz_summary (may be NULL).  `out` receives the BGZF bytes, out_capacity counts them; out_summary still describes the text,
 * which stays in the object's output buffer and is bounded by max_out_bytes alone.  After tgsf_text_out_reserve and
 * tgsf_text_bgzf_out_reserve (max_in_bytes >= the text).  What the counterparts refuse is handed through unchanged.  No record:
 * an empty output, or the EOF member alone.
 */
int tgsf_text_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* text, uint64_t n_bytes, int fasta, int final, int fastq_out,
                          uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary, tgsf_text_summary* in_summary,
                          const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out, int eof, tgsf_text_gzout_summary* gz_summary);
int tgsf_text_bam_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, int final, int fastq_out,
                              uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary, tgsf_text_bam_summary* in_summary,
                              const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out, int eof, tgsf_text_gzout_summary* gz_summary);
int tgsf_text_bgzf_bam_filter_bgzf(tgsf_text* tx, tgsf_ctx* ctx, const uint8_t* gz, uint64_t n_bytes, uint32_t skip, int final, int fastq_out,
                                   uint8_t* out, uint64_t out_capacity, tgsf_text_out_summary* out_summary,
                                   tgsf_text_bgzf_bam_summary* in_summary, const tgsf_text_index_arrays* out_index, tgsf_batch_out* batch_out,
                                   int eof, tgsf_text_gzout_summary* gz_summary);

#ifdef __cplusplus
}
#endif
#endif /* TGSF_TEXT_H */
