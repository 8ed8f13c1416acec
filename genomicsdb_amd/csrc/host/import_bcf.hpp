// import_bcf.hpp - the host's share of BCF2 input for the device importer, without HIP types (the CPU harness
// tests/hostsim_import_bcf runs the same code): the content sniff, inflating a gzip / BGZF buffer held in memory, the header with
// its dictionaries as htslib builds them (bcf_hdr_parse / bcf_hdr_sync), the per-file tables the bodies of
// core/gdb_import_bcf.hpp read, the walk of the l_shared / l_indiv chain with the cut into batches, and the text of an error
// the bodies flagged on a record.
#pragma once
#include <zlib.h>

#include <cstring>
#include <string>
#include <vector>

#include "../core/gdb_import_bcf.hpp"
#include "import_common.hpp"

namespace genomicsdb_amd {

inline bool is_bcf2(const char* p, size_t n) { return n >= 5 && memcmp(p, "BCF\2", 4) == 0 && (p[4] == 1 || p[4] == 2); }
inline bool is_gzip(const char* p, size_t n) { return n >= 2 && (uint8_t)p[0] == 0x1f && (uint8_t)p[1] == 0x8b; }

// the first bytes of a file's content, through zlib (plain, gzip and BGZF alike)
inline bool file_is_bcf2(const std::string& path) {
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) return false;       // (the caller's own open reports it)
  char head[5];
  const int n = gzread(f, head, sizeof(head));
  gzclose(f);
  return n == 5 && is_bcf2(head, 5);
}

// every member of a gzip / BGZF buffer, inflated on the host
inline std::string inflate_gzip_buffer(const char* p, size_t n, const std::string& name) {
  std::string out;
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, 15 + 16) != Z_OK) throw VCF2BinaryException("zlib inflateInit2 failed");
  zs.next_in = (Bytef*)p;
  size_t left = n;
  std::vector<char> buf(1 << 16);
  for (;;) {
    if (zs.avail_in == 0) {
      if (left == 0) break;
      const size_t take = left < ((size_t)1 << 30) ? left : ((size_t)1 << 30);
      zs.avail_in = (uInt)take; left -= take;
    }
    zs.next_out = (Bytef*)buf.data(); zs.avail_out = (uInt)buf.size();
    const int rc = inflate(&zs, Z_NO_FLUSH);
    out.append(buf.data(), buf.size() - zs.avail_out);
    if (rc == Z_STREAM_END) {
      if (zs.avail_in == 0 && left == 0) break;
      if (inflateReset(&zs) != Z_OK) { inflateEnd(&zs); throw VCF2BinaryException("zlib inflateReset failed"); }
    } else if (rc != Z_OK) { inflateEnd(&zs); throw VCF2BinaryException("invalid gzip data in " + name); }
  }
  inflateEnd(&zs);
  return out;
}

struct BcfHeaderHost {
  std::string text;                     // the header text (VCF header lines), without the terminating NULs
  size_t records_begin = 0;             // offset of the first record in the stream
  std::vector<std::string> dict;        // FILTER / INFO / FORMAT id -> name ("" : unused id)
  std::vector<std::string> contigs;     // contig id -> name
  ImportHeader samples;                 // the #CHROM line, by the text importer's rule
  // per-file tables
  std::vector<int32_t> dict_info, dict_fmt, dict_filter;
  std::vector<int64_t> contig_off;
  int32_t end_key = -1;
  gdbimp::ImpBcfTables view() const {
    gdbimp::ImpBcfTables B;
    B.dict_info = dict_info.data(); B.dict_fmt = dict_fmt.data(); B.dict_filter = dict_filter.data(); B.contig_off = contig_off.data();
    B.n_dict = (int32_t)dict.size(); B.n_contig = (int32_t)contigs.size(); B.end_key = end_key; B.n_samples = samples.n_samples;
    return B;
  }
};

namespace bcf_detail {
// ID and IDX of a structured header line's <key=value,...> body; values may be quoted
inline bool id_and_idx(const char* p, size_t n, std::string* id, long* idx) {
  *idx = -1;
  bool have_id = false;
  size_t i = 0;
  while (i < n) {
    size_t k = i;
    while (k < n && p[k] != '=' && p[k] != ',') ++k;
    const std::string key(p + i, k - i);
    if (k >= n || p[k] == ',') { i = k + 1; continue; }
    size_t v = k + 1, e;
    std::string val;
    if (v < n && p[v] == '"') {
      e = v + 1;
      while (e < n && p[e] != '"') { if (p[e] == '\\' && e + 1 < n) ++e; ++e; }
      val.assign(p + v + 1, (e < n ? e : n) - v - 1);
      e = e < n ? e + 1 : n;
    } else {
      e = v;
      while (e < n && p[e] != ',') ++e;
      val.assign(p + v, e - v);
    }
    if (key == "ID" && !have_id) { *id = val; have_id = true; }
    else if (key == "IDX") { char* end = nullptr; const long x = strtol(val.c_str(), &end, 10); if (!val.empty() && !*end && x >= 0 && x < (1 << 24)) *idx = x; }
    i = e + 1;
  }
  return have_id;
}
inline void put(std::vector<std::string>& dict, const std::string& name, long idx) {
  for (const std::string& s : dict) if (s == name) return;       // the first appearance of a name gives its id
  if (idx < 0) idx = (long)dict.size();
  if ((size_t)idx >= dict.size()) dict.resize((size_t)idx + 1);
  dict[(size_t)idx] = name;
}
}  // namespace bcf_detail

// 'BCF\2\x' + l_text + header text; the dictionaries; the tables against the vid
inline BcfHeaderHost parse_bcf_header(const char* data, size_t n, const ImportFile& file, const ImportTablesHost& H) {
  if (!is_bcf2(data, n) || n < 9) throw VCF2BinaryException(file.path + " is not a BCF2 stream");
  uint32_t l_text;
  memcpy(&l_text, data + 5, 4);
  if ((uint64_t)l_text > n - 9) throw VCF2BinaryException("the BCF2 header of " + file.path + " is longer than the input (l_text " + std::to_string(l_text) + ")");
  BcfHeaderHost h;
  h.text.assign(data + 9, l_text);
  const size_t nul = h.text.find('\0');
  if (nul != std::string::npos) h.text.resize(nul);
  h.records_begin = 9 + (size_t)l_text;
  h.dict.push_back("PASS");       // id 0 whether or not the header declares it
  size_t pos = 0;
  while (pos < h.text.size()) {
    size_t eol = h.text.find('\n', pos);
    if (eol == std::string::npos) eol = h.text.size();
    const char* lp = h.text.data() + pos;
    size_t ln = eol - pos;
    pos = eol + 1;
    if (ln && lp[ln - 1] == '\r') --ln;
    int kind = -1;
    size_t skip = 0;
    if (ln > 10 && memcmp(lp, "##FILTER=<", 10) == 0) { kind = 0; skip = 10; }
    else if (ln > 8 && memcmp(lp, "##INFO=<", 8) == 0) { kind = 0; skip = 8; }
    else if (ln > 10 && memcmp(lp, "##FORMAT=<", 10) == 0) { kind = 0; skip = 10; }
    else if (ln > 10 && memcmp(lp, "##contig=<", 10) == 0) { kind = 1; skip = 10; }
    if (kind < 0 || lp[ln - 1] != '>') continue;
    std::string id;
    long idx;
    if (!bcf_detail::id_and_idx(lp + skip, ln - skip - 1, &id, &idx)) continue;
    bcf_detail::put(kind == 0 ? h.dict : h.contigs, id, idx);
  }
  h.samples = parse_import_header(h.text, file);
  // dictionary id -> attribute / field / column offset
  auto name_is = [&](uint32_t off, uint32_t len, const std::string& s) { return s.size() == len && memcmp(H.names.data() + off, s.data(), len) == 0; };
  h.dict_info.assign(h.dict.size(), -1); h.dict_fmt.assign(h.dict.size(), -1); h.dict_filter.assign(h.dict.size(), -1);
  for (size_t d = 0; d < h.dict.size(); ++d) {
    const std::string& s = h.dict[d];
    if (s.empty()) continue;
    if (s == "END") h.end_key = (int32_t)d;
    for (size_t i = 0; i < H.info.size() && h.dict_info[d] < 0; ++i) if (name_is(H.info[i].name_off, H.info[i].name_len, s)) h.dict_info[d] = (int32_t)i;
    for (size_t i = 0; i < H.fmt.size() && h.dict_fmt[d] < 0; ++i) if (name_is(H.fmt[i].name_off, H.fmt[i].name_len, s)) h.dict_fmt[d] = (int32_t)i;
    for (size_t i = 0; i < H.fields.size() && h.dict_filter[d] < 0; ++i) if (name_is(H.fields[i].off, H.fields[i].len, s)) h.dict_filter[d] = (int32_t)H.fields[i].value;
  }
  h.contig_off.assign(h.contigs.size(), -1);
  for (size_t c = 0; c < h.contigs.size(); ++c)
    for (size_t i = 0; i < H.contigs.size() && h.contig_off[c] < 0; ++i)
      if (!h.contigs[c].empty() && name_is(H.contigs[i].off, H.contigs[i].len, h.contigs[c])) h.contig_off[c] = H.contigs[i].value;
  return h;
}

// The chain of records from `begin` to the end of the stream: offs gets the offset of every record and the end of the last.
// A broken chain names the file, the 1-based record number and the byte offset.
inline void bcf_walk_records(const char* data, size_t n, size_t begin, const std::string& path, std::vector<uint64_t>& offs) {
  offs.clear();
  size_t at = begin;
  while (at < n) {
    const std::string where = " (" + path + " record " + std::to_string(offs.size() + 1) + " at byte offset " + std::to_string(at) + ")";
    if (n - at < 8) throw VCF2BinaryException("truncated BCF2 record: " + std::to_string(n - at) + " bytes where the two record lengths belong" + where);
    uint32_t l_shared, l_indiv;
    memcpy(&l_shared, data + at, 4);
    memcpy(&l_indiv, data + at + 4, 4);
    if (l_shared < 24) throw VCF2BinaryException("BCF2 record with l_shared " + std::to_string(l_shared) + " below the 24 fixed bytes" + where);
    const uint64_t len = 8ull + l_shared + l_indiv;
    if (len > n - at) throw VCF2BinaryException("truncated BCF2 record: " + std::to_string(len) + " bytes announced, " + std::to_string(n - at) + " left" + where);
    offs.push_back(at);
    at += (size_t)len;
  }
  offs.push_back(at);
}

// records [first, last) of one batch: at most `budget` bytes, cut at record boundaries; a record larger than the budget is a batch of its own
inline size_t bcf_next_batch(const std::vector<uint64_t>& offs, size_t first, uint64_t budget) {
  size_t last = first + 1;
  while (last + 1 < offs.size() && offs[last + 1] - offs[first] <= budget) ++last;
  return last;
}

// the message of an error bit the bodies flagged on record [begin, end) of `p`; `where` = "<path> record <n>"
inline std::string describe_bcf_error(uint32_t bit, const ImportTablesHost& H, const ImportOptions& opt, const BcfHeaderHost& hdr, const uint8_t* p, uint32_t begin,
                                      uint32_t end, const std::string& where) {
  using namespace gdbimp;
  const ImpTables T = H.view(opt, hdr.samples.n_samples);
  const ImpBcfTables B = hdr.view();
  std::vector<ImpBcfField> F(H.info.size() + H.fmt.size() + 1);
  ImpBcfRec R;
  imp_bcf_index(T, B, p, begin, end, &R, F.data());
  auto dict_name = [&](int32_t id) { return id >= 0 && (size_t)id < hdr.dict.size() && !hdr.dict[(size_t)id].empty() ? hdr.dict[(size_t)id] : "#" + std::to_string(id); };
  switch (bit) {
    case IMP_ERR_CONTIG: {
      const int32_t rid = (int32_t)bcf_u32(p, begin + 8u);
      return "contig " + (rid >= 0 && (size_t)rid < hdr.contigs.size() ? hdr.contigs[(size_t)rid] : std::to_string(rid)) + " is not in the vid mapping (" + where + ")";
    }
    case IMP_ERR_FILTER:
      for (uint32_t k = 0; k < R.filter_n; ++k) {
        const int32_t id = bcf_int(p, R.filter_off + k * bcf_width(R.filter_type), R.filter_type);
        if (id >= 0 && id < B.n_dict && B.dict_filter[id] < 0) return "FILTER " + dict_name(id) + " is not in the vid mapping (" + where + ")";
      }
      break;
    case IMP_ERR_COORD_RANGE: return "a column outside what the device importer's (column, row) sort key holds (" + where + ")";
    case IMP_ERR_COUNT:
      for (size_t i = 0; i < H.info.size(); ++i) {
        const ImpAttr& a = H.info[i];
        const ImpBcfField& f = F[i];
        if (!a.fixed || a.elem > GDB_ET_FLOAT || !f.present || f.type == BCF_T_NULL || f.type == BCF_T_CHAR) continue;
        uint32_t m = 0;
        while (m < f.count && !bcf_elem_vector_end(p, f.off, m, f.type)) ++m;
        if (m == 0 || (m == 1 && bcf_elem_missing(p, f.off, 0, f.type))) continue;
        if (m != a.num_elements) return "field " + H.info_names[i] + ": " + std::to_string(m) + " values, expected " + std::to_string(a.num_elements) + " (" + where + ")";
      }
      return "a fixed-length FORMAT field with a wrong number of values (" + where + ")";
    case IMP_ERR_BCF_FIELD_TYPE:
      for (size_t i = 0; i < H.info.size() + H.fmt.size(); ++i) {
        const bool info = i < H.info.size();
        const ImpAttr& a = info ? H.info[i] : H.fmt[i - H.info.size()];
        const std::string& name = info ? H.info_names[i] : H.fmt_names[i - H.info.size()];
        const ImpBcfField& f = F[i];
        if (!f.present || f.type == BCF_T_NULL || a.elem == GDB_ET_FLAG) continue;
        const char* rec = f.type == BCF_T_CHAR ? "char" : f.type == BCF_T_FLOAT ? "float" : "integer";
        const bool bad = a.elem == GDB_ET_CHAR ? f.type != BCF_T_CHAR : (f.type == BCF_T_CHAR || (a.elem == GDB_ET_INT && f.type == BCF_T_FLOAT));
        if (bad) return std::string("field ") + name + ": the record holds " + rec + " values, the vid mapping declares " + (a.elem == GDB_ET_CHAR ? "char" : a.elem == GDB_ET_INT ? "int" : "float") + " (" + where + ")";
      }
      break;
    case IMP_ERR_BCF_TYPE_CODE: return "BCF2 typed descriptor with an unknown or misplaced type code (" + where + ")";
    case IMP_ERR_BCF_BOUNDS: return "BCF2 vector or block that runs past the end of its block (" + where + ")";
    case IMP_ERR_BCF_DICT: return "BCF2 dictionary or contig id outside the header's range (" + where + ")";
    case IMP_ERR_BCF_NSAMPLE:
      return "BCF2 record with n_sample " + std::to_string(bcf_u32(p, begin + 28u) & 0xFFFFFFu) + ", the header has " + std::to_string(hdr.samples.n_samples) + " samples (" + where + ")";
    case IMP_ERR_BCF_END: return "INFO END without one integer value (" + where + ")";
    default: break;
  }
  return "malformed record (" + where + ")";
}

}  // namespace genomicsdb_amd
