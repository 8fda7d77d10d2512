// record_out.h -- the layout of an output record (record formatting, src/TGSFilter.cpp:2011-2053), in this file only:
//   '@' or '>', the name (newSeqName: ":<n>" from a read's second fragment on), '\n', the sequence, for FASTQ "\n+\n" and the
//   qualities, '\n'.
// Both passes write a CleanRec: its size (the planners lay records out before anything is copied), its copy into the mapped
// output file (the fill jobs) and its gathered form for the single-stream writer (Output).
#pragma once
#include "pipeline.h"

namespace host {

// the size of the record, without building its name
inline uint64_t record_bytes(const CleanRec& r, bool fastq)
{
    uint64_t name = r.name.size();
    if (r.pass_num >= 2) { name += 1; for (int v = r.pass_num; v; v /= 10) name++; }
    return 1 + name + 1 + (uint64_t)r.len + (fastq ? 3 + (uint64_t)r.len : 0) + 1;
}

// the record copied to d (a mapped output file: stream_copy; fill_records fences); returns its end.  `name` is scratch.
inline char* put_record(char* d, const CleanRec& r, bool fastq, std::string& name)
{
    *d++ = fastq ? '@' : '>';
    if (r.pass_num < 2) { memcpy(d, r.name.data(), r.name.size()); d += r.name.size(); }
    else { name.clear(); append_name(name, r.name, r.pass_num); memcpy(d, name.data(), name.size()); d += name.size(); }
    *d++ = '\n';
    stream_copy(d, r.seq, r.len); d += r.len;
    if (fastq) {
        memcpy(d, "\n+\n", 3); d += 3;
        stream_copy(d, r.qual, r.len); d += r.len;
    }
    *d++ = '\n';
    return d;
}

// A fill job: records [lo, hi), rec(i) each, copied to d.  It must end exactly at `end`, where the layout put the end of its
// last record (record_bytes and put_record agree): a slip would corrupt the file at the seam to the next job without a sign.
template <class RecordAt>
void fill_records(char* d, const char* end, size_t lo, size_t hi, bool fastq, RecordAt rec)
{
    std::string name;
    for (size_t i = lo; i < hi; i++) d = put_record(d, rec(i), fastq, name);
    stream_fence();
    if (d != end) die("an output record was laid out with another size than it was written with (" + std::to_string((long long)(d - end)) + " bytes off)");
}

// the record's pieces gathered straight from the input text (Output: writev, or a gzip member per record)
inline void gather_record(Output& out, const CleanRec& r, bool fastq, std::string& name)
{
    static const std::string at("@"), gt(">"), nl("\n"), sep("\n+\n");
    out.text(fastq ? at : gt);
    if (r.pass_num < 2) out.piece(r.name.data(), r.name.size());
    else { name.clear(); append_name(name, r.name, r.pass_num); out.text(name); }
    out.text(nl);
    out.piece(r.seq, r.len);
    if (fastq) {
        out.text(sep);
        out.piece(r.qual, r.len);
    }
    out.text(nl);
    out.end_record();
}

}  // namespace host
