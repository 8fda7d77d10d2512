// run_writer.cpp -- the output side of the filter pass (run.h): the ordered planner and the fill jobs; the early sink of a
// downsampling run.
#include "record_out.h"
#include "run.h"

namespace host {

bool Run::plain_file_out() const
{
    const char* w = getenv("TGSF_WRITER");                             // "writev": always the single-stream writer
    return !o.out_gz && !o.out_file.empty() && !(w && !strcmp(w, "writev"));
}

// records [lo, hi) of the batch's layout copied into the mapped output file
void Run::fill_job(const std::shared_ptr<Batch>& b, size_t lo, size_t hi)
{
    Batch& bb = *b;
    const auto at = [&](size_t i) { return i < bb.em.size() ? bb.em[i].at : bb.out_bytes; };
    fill_records(bb.dst + at(lo), bb.dst + at(hi), lo, hi, fastq_out, [&](size_t i) -> const CleanRec& { return bb.em[i].rec; });
    if (--bb.left == 0) batch_done(b);
}

// record formatting :2011-2053 + write_output :2095-2145.  The planner takes the batches in input order (= the reference's
// -t 1 order), lays the records of a batch out in the output file and hands runs of them to the fill threads (MappedSink);
// or, for the other kinds of output, gathers the pieces and writes them itself (Output).
void Run::writer_body()
{
    using Emit = Batch::Emit;
    CpuScope cpu(CPU_PLANNER);
    std::string name;
    std::map<uint64_t, std::shared_ptr<Batch>> held;               // batches that arrived ahead of their turn
    uint64_t want = 0, in_seen = 0;
    size_t open_feeders = ctxs.size();
    for (;;) {
        std::shared_ptr<Batch> b;
        auto it = held.find(want);
        if (it != held.end()) { b = std::move(it->second); held.erase(it); }
        else {
            if (open_feeders == 0) break;
            const double i0 = now_s();
            b = to_writer->get();
            t_widle += now_s() - i0;
            if (!b) { open_feeders--; continue; }
            if (b->id != want) { const uint64_t id = b->id; held[id] = std::move(b); continue; }
        }
        want++;
        const double w0 = now_s();
        const bool fill = mapped.is_open();
        uint64_t at = 0;
        for (size_t r = 0; r < b->recs.size(); r++) {
            int pass_num = 1;
            const tgsf_read_result& rr = b->res[r];
            const Rec& rec = b->recs[r];
            const std::string_view rname(rec.name, rec.name_len);
            for (uint32_t f = rr.frag_begin; f < rr.frag_begin + rr.n_frags; f++) {
                const tgsf_fragment& fr = b->frags[f];
                if (!(fr.flags & TGSF_FF_PASS)) continue;
                const CleanRec c{rname, pass_num++, rec.seq + fr.start, rec.qual + fr.start, (uint32_t)fr.len};
                clean_bases += (uint64_t)fr.len;
                clean_lens.push_back(fr.len);
                if (o.downsample) clean_recs.push_back(c);         // kept in memory instead of a tmp file (:3129-3137)
                else if (o.only_qc) continue;
                else if (fill) {
                    b->em.push_back({c, at});
                    at += record_bytes(c, fastq_out);
                } else gather_record(out, c, fastq_out, name);
            }
        }
        in_seen += b->span;
        if (fill && at) {
            // How far the file will go: what is left of the input times the share of it that was written so far
            // (plus a little).  (A streamed input's text size is estimated from the share of the file decoded so far.)
            const uint64_t end = mapped.sink.planned() + at;
            const double share = in_seen ? (double)end / (double)in_seen : 1.0;
            const double sh = stream_share.load();
            const uint64_t in_total = !streaming ? (uint64_t)text_size
                                    : (uint64_t)((double)stream_text.load() / (sh > 1e-6 ? sh : 1e-6));
            b->dst = mapped.claim(at, end + (uint64_t)(share * 1.02 * (double)(in_total - std::min<uint64_t>(in_seen, in_total))));
            b->out_bytes = at;
            const size_t n = b->em.size();
            const int parts = (int)std::min<size_t>((size_t)fill_threads, std::max<size_t>(1, at / fill_min));
            b->left = parts;
            size_t lo = 0;
            for (int k = 0; k < parts; k++) {                      // byte-balanced runs of records
                size_t hi = n;
                if (k + 1 < parts) {
                    const uint64_t target = at / (uint64_t)parts * (uint64_t)(k + 1);
                    hi = (size_t)(std::lower_bound(b->em.begin() + (long)lo, b->em.end(), target,
                                                   [](const Emit& e, uint64_t tgt) { return e.at < tgt; }) - b->em.begin());
                }
                mapped.fill([this, b, lo, hi] { fill_job(b, lo, hi); });
                lo = hi;
            }
        }
        if (!o.only_qc && !fill) out.flush_iov();                   // the batch (and its views) goes away
        if (!(fill && at)) batch_done(b);                           // written (or nothing to write)
        t_write += now_s() - w0;
    }
    if (!o.downsample) std::sort(clean_lens.begin(), clean_lens.end());   // for the statistics (:3182), beside the last fill jobs
}

// A downsampling run writes its output only after the whole filter pass (the selection needs every fragment's length,
// :2297-2344) -- but the file can be instantiated meanwhile: while the filter pass is busy with the link to the device,
// pages for what the selection may keep are reserved and mapped (a quarter of the input at most, and no more than twice
// the bases asked for with -g/-d; a surplus is cut off at the end).  Large plain outputs only.
bool Run::open_down_mapped(uint64_t capacity, uint64_t speculative)
{
    if (!plain_file_out() || !down_mapped.open(out_path, capacity)) return false;
    down_mapped.start_reserving(populate_threads, stride_bytes, speculative);
    return true;
}

}  // namespace host
