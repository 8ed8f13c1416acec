// import_common.hpp - the host's share of the device importer (kernels/gdb_import.hip), without HIP types so that the CPU
// harness of the bodies (tests/hostsim_import) runs the very same code: the small tables the bodies of core/gdb_import.hpp read,
// the refusals, the files of the callset mapping, the header / #CHROM rule of host/vcf_importer.cc, the host parse of deferred
// tokens and the text of an error found on a record line.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../core/gdb_import_csv.hpp"
#include "vcf_importer.h"

namespace genomicsdb_amd {

struct ImportTablesHost {
  std::string names;
  std::vector<gdbimp::ImpName> contigs, fields;
  std::vector<gdbimp::ImpAttr> info, fmt;
  std::vector<std::string> info_names, fmt_names;      // m_name, for messages
  bool has_id = false;
  int key_row_bits = 1;
  int64_t max_row = 0;
  uint32_t add_name(const std::string& s) { const uint32_t off = (uint32_t)names.size(); names += s; return off; }
  // the tables as the bodies take them, over host memory
  gdbimp::ImpTables view(const ImportOptions& opt, int n_samples) const {
    gdbimp::ImpTables T;
    T.names = names.data(); T.contigs = contigs.data(); T.fields = fields.data(); T.info = info.data(); T.fmt = fmt.data();
    T.n_contigs = (int32_t)contigs.size(); T.n_fields = (int32_t)fields.size(); T.n_info = (int32_t)info.size(); T.n_fmt = (int32_t)fmt.size();
    T.has_id = has_id ? 1 : 0; T.treat_deletions_as_intervals = opt.treat_deletions_as_intervals ? 1 : 0;
    T.n_samples = n_samples; T.key_row_bits = key_row_bits; T.column_begin = opt.column_begin; T.column_end = opt.column_end;
    return T;
  }
};

// same walk over the schema as import_callsets_to_cells; what the bodies do not cover is refused by name
// contigs_only: for a caller that reads nothing but CHROM, POS and END of a line (the splitter): no field is looked at, none refused
inline ImportTablesHost build_import_tables(const VidMapper& vid, bool contigs_only = false) {
  if (!vid.is_initialized() || !vid.is_callset_mapping_initialized()) throw VCF2BinaryException("vid and callset mappings are needed");
  ImportTablesHost H;
  H.has_id = vid.get_field_info("ID") != nullptr;
  auto attr_of = [&](const FieldInfo& f, bool sum_like) {
    gdbimp::ImpAttr a;
    memset(&a, 0, sizeof(a));
    a.name_off = H.add_name(f.m_vcf_name); a.name_len = (uint32_t)f.m_vcf_name.size(); a.num_elements = f.m_num_elements;
    a.elem = (uint8_t)f.m_element_type; a.fixed = f.is_fixed_length_field() ? 1 : 0; a.sum_like = sum_like ? 1 : 0;
    a.gt = f.m_vcf_name == "GT" ? 1 : 0; a.pp = f.m_length_descriptor == GDB_VL_PP ? 1 : 0;
    return a;
  };
  auto refuse_2d = [](const FieldInfo& f) {
    if (f.is_flattened_field()) throw VCF2BinaryException("field " + f.m_name + ": flattened tuple elements are not imported by the device importer of this build (the host importer takes this vid)");
    if (f.m_num_dimensions == 2) throw VCF2BinaryException("field " + f.m_name + ": 2-dimensional (allele-specific) fields are not imported by the device importer of this build (the host importer takes this vid)");
  };
  for (unsigned i = 0; i < vid.get_num_fields() && !contigs_only; ++i) {
    const FieldInfo& f = vid.get_field_info(i);
    if (f.m_name == "END") continue;
    const GdbCombineOp op = f.m_VCF_field_combine_operation;
    const bool sum_like = op == GDB_OP_SUM || op == GDB_OP_DP || op == GDB_OP_ELEMENT_WISE_SUM || op == GDB_OP_HISTOGRAM_SUM;
    if (f.m_unsupported_on_device && (f.m_is_vcf_INFO_field || f.m_is_vcf_FORMAT_field))
      throw VCF2BinaryException("field " + f.m_name + ": fields of more than 2 dimensions are not imported by this build");
    if (f.get_num_elements_in_tuple() > 1u) {
      if (f.m_num_dimensions != 2) throw VCF2BinaryException("field " + f.m_name + ": tuple elements are only imported for 2-dimensional fields");
      refuse_2d(f);
    }
    if (f.m_is_vcf_INFO_field) { refuse_2d(f); H.info.push_back(attr_of(f, sum_like)); H.info_names.push_back(f.m_name); }
  }
  for (unsigned i = 0; i < vid.get_num_fields() && !contigs_only; ++i) {
    const FieldInfo& f = vid.get_field_info(i);
    if (f.m_name != "END" && f.m_is_vcf_FORMAT_field) { refuse_2d(f); H.fmt.push_back(attr_of(f, false)); H.fmt_names.push_back(f.m_name); }
  }
  for (unsigned i = 0; i < vid.get_num_contigs(); ++i) {       // first match in index order, like VidMapper::get_contig_info
    const ContigInfo& c = vid.get_contig_info(i);
    gdbimp::ImpName n; n.off = H.add_name(c.m_name); n.len = (uint32_t)c.m_name.size(); n.value = c.m_tiledb_column_offset;
    H.contigs.push_back(n);
  }
  for (unsigned i = 0; i < vid.get_num_fields(); ++i) {        // a FILTER value is looked up among ALL field names, as the host does
    const FieldInfo& f = vid.get_field_info(i);
    if (vid.get_field_info(f.m_name) != &f) continue;
    gdbimp::ImpName n; n.off = H.add_name(f.m_name); n.len = (uint32_t)f.m_name.size(); n.value = f.m_field_idx;
    H.fields.push_back(n);
  }
  for (const CallSetInfo& cs : vid.get_callsets()) {
    if (cs.m_row_idx < 0) throw VCF2BinaryException("callset " + cs.m_name + " has a negative row index");
    if (cs.m_row_idx > H.max_row) H.max_row = cs.m_row_idx;
  }
  while (H.key_row_bits < 62 && (H.max_row >> H.key_row_bits) != 0) ++H.key_row_bits;
  return H;
}

struct ImportFile { std::string name, path; std::vector<const CallSetInfo*> callsets; GdbFileType type = GDB_FILE_VCF; };
// callsets grouped by file, in mapping order; only the callsets inside opt's row bounds, and only the files that have one
inline std::vector<ImportFile> import_files(const VidMapper& vid, const ImportOptions& opt) {
  std::vector<ImportFile> files;
  std::unordered_map<std::string, size_t> at;
  for (const CallSetInfo& cs : vid.get_callsets()) {
    if (cs.m_filename.empty()) throw VCF2BinaryException("callset " + cs.m_name + " has no \"filename\"");
    if (!row_in_bounds(opt, cs.m_row_idx)) continue;
    if (!at.count(cs.m_filename)) {
      at[cs.m_filename] = files.size();
      ImportFile f;
      f.name = cs.m_filename;
      f.path = (cs.m_filename[0] != '/' && !opt.file_root.empty()) ? opt.file_root + "/" + cs.m_filename : cs.m_filename;
      f.type = vid.get_file_type(cs.m_filename);
      files.push_back(f);
    }
    files[at[cs.m_filename]].callsets.push_back(&cs);
  }
  return files;
}

// what the CSV bodies (core/gdb_import_csv.hpp) do not cover, refused by name when the mapping has a CSV file
inline void refuse_for_csv(const VidMapper& vid, const ImportTablesHost& H, const std::vector<ImportFile>& files) {
  const ImportFile* csv = nullptr;
  for (const ImportFile& f : files) if (f.type != GDB_FILE_VCF && !csv) csv = &f;
  if (!csv) return;
  // the reference's fixed field indices (variant_array_schema.h:44-48) do not account for the ID attribute: it misreads such lines
  if (H.has_id) throw VCF2BinaryException("field ID: a vid that declares ID is not imported from CSV cell files (" + csv->path + ")");
  auto check = [&](const gdbimp::ImpAttr& a, const std::string& name) {
    if (a.elem != GDB_ET_INT && a.elem != GDB_ET_FLOAT && a.elem != GDB_ET_CHAR)
      throw VCF2BinaryException("field " + name + ": only int, float and char attributes are imported from CSV cell files (" + csv->path + ")");
    if (a.elem == GDB_ET_CHAR && a.fixed)
      throw VCF2BinaryException("field " + name + ": fixed-length char attributes are not imported from CSV cell files (" + csv->path + ")");
  };
  for (size_t i = 0; i < H.info.size(); ++i) check(H.info[i], H.info_names[i]);
  for (size_t i = 0; i < H.fmt.size(); ++i) check(H.fmt[i], H.fmt_names[i]);
}
// the rows of a CSV file's callsets, ascending and without repeats: the table a line's row is looked up in
inline std::vector<int64_t> csv_rows_of(const ImportFile& file) {
  std::vector<int64_t> rows;
  for (const CallSetInfo* cs : file.callsets) rows.push_back(cs->m_row_idx);
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  return rows;
}
// CSV cell files are opened as they are (the reference uses fopen): compressed content is refused by name
inline void refuse_compressed_csv(const char* data, size_t n, const std::string& path) {
  if (n >= 2 && (uint8_t)data[0] == 0x1f && (uint8_t)data[1] == 0x8b)
    throw VCF2BinaryException(path + " is gzip or BGZF: compressed CSV cell files are not imported");
}
// where a batch of text that begins at pos ends: at most `budget` bytes cut behind a newline; a line longer than the budget grows its batch
inline size_t import_text_cut(const char* text, size_t size, size_t pos, uint64_t budget) {
  size_t stop = size;
  if (stop - pos > budget) {
    const void* nl = memrchr(text + pos, '\n', (size_t)budget);
    if (!nl) nl = memchr(text + pos + budget, '\n', size - pos - (size_t)budget);
    if (nl) stop = (size_t)((const char*)nl - text) + 1;
  }
  return stop;
}

struct ImportHeader {
  size_t record_begin = 0;          // offset of the first line that is neither empty nor a '#' line
  int64_t lines_before = 0;         // physical lines in front of it
  int n_samples = 0;
  std::vector<int64_t> sample_row;  // sample of the file -> array row (-1: not imported)
};
// the leading '#' lines: every #CHROM line maps the samples anew (callset -> row through idx_in_file), as the host importer does
inline ImportHeader parse_import_header(const std::string& text, const ImportFile& file) {
  ImportHeader h;
  size_t pos = 0;
  while (pos < text.size()) {
    size_t eol = text.find('\n', pos);
    if (eol == std::string::npos) eol = text.size();
    const char* lp = text.data() + pos;
    size_t ln = eol - pos;
    if (ln && lp[ln - 1] == '\r') --ln;
    if (ln && lp[0] != '#') break;
    if (ln > 6 && memcmp(lp, "#CHROM", 6) == 0) {
      std::vector<std::string> cols;
      size_t b = 0;
      for (size_t i = 0; i <= ln; ++i) if (i == ln || lp[i] == '\t') { cols.emplace_back(lp + b, i - b); b = i + 1; }
      h.n_samples = cols.size() > 9 ? (int)cols.size() - 9 : 0;
      h.sample_row.assign((size_t)h.n_samples, -1);
      for (const CallSetInfo* cs : file.callsets) {
        if (cs->m_idx_in_file < 0 || cs->m_idx_in_file >= h.n_samples) throw VCF2BinaryException("idx_in_file out of range for callset " + cs->m_name);
        const std::string& want = cols[9 + (size_t)cs->m_idx_in_file];
        for (int s = 0; s < h.n_samples; ++s) if (cols[9 + (size_t)s] == want) h.sample_row[(size_t)s] = cs->m_row_idx;
      }
    }
    pos = eol + 1;
    ++h.lines_before;
  }
  h.record_begin = pos < text.size() ? pos : text.size();
  // a #CHROM line among the records would remap the samples half way: the host importer follows that, the device path does not
  if (h.record_begin < text.size() && memmem(text.data() + h.record_begin, text.size() - h.record_begin, "\n#CHROM", 7))
    throw VCF2BinaryException("a #CHROM line after the first record in " + file.path + " is not imported by the device importer of this build");
  return h;
}

// a record line of host text as the bodies take it
struct ImpHostLine {
  std::vector<uint32_t> tabs;
  gdbimp::ImpLine line;
  ImpHostLine(const char* text, uint32_t begin, uint32_t end) {
    if (end > begin && text[end - 1] == '\r') --end;
    for (uint32_t i = begin; i < end; ++i) if (text[i] == '\t') tabs.push_back(i);
    line.text = text; line.begin = begin; line.end = end; line.tabs = tabs.data(); line.ntabs = (uint32_t)tabs.size();
  }
};

// the 4 bytes of a deferred token, by the host importer's own parsers (which throw what the host importer throws)
inline uint32_t resolve_deferred(const gdbimp::ImpDeferred& d, const char* text, const ImportTablesHost& H) {
  std::string what = d.what == gdbimp::IMP_WHAT_QUAL ? "QUAL" : d.what == gdbimp::IMP_WHAT_GT ? "GT" : d.what == gdbimp::IMP_WHAT_FILTER ? "FILTER"
                     : d.what >= gdbimp::IMP_WHAT_FMT_BASE ? H.fmt_names.at((size_t)(d.what - gdbimp::IMP_WHAT_FMT_BASE)) : H.info_names.at((size_t)d.what);
  union { float f; uint32_t u; int32_t i; } x;
  if (d.kind == gdbimp::IMP_KIND_CSV_INT) x.i = (int32_t)import_csv_parse_int(text + d.tok_off, d.tok_len, what);      // truncated to the attribute's width
  else if (d.kind == gdbimp::IMP_KIND_CSV_FLOAT) x.f = import_csv_parse_float(text + d.tok_off, d.tok_len, what);
  else if (d.kind == gdbimp::IMP_KIND_INT) {
    int64_t v = import_parse_int(text + d.tok_off, d.tok_len, what);
    if (d.divide) v = gdbimp::imp_divide_among_samples(v, (int)d.divide, (int)d.sample_idx);
    x.i = (int32_t)v;
  } else {
    float v = (float)import_parse_double(text + d.tok_off, d.tok_len, what);
    if (d.divide) v = v / (float)d.divide;
    x.f = v;
  }
  return x.u;
}

// the message of an error the bodies flagged on a line (ImpErr bit), in the host importer's words; `where` = "<path> line <n>"
inline std::string describe_line_error(uint32_t bit, const ImportTablesHost& H, const ImportOptions& opt, const ImportHeader& hdr, const char* text,
                                       uint32_t begin, uint32_t end, const std::string& where) {
  using namespace gdbimp;
  ImpHostLine hl(text, begin, end);
  const ImpLine& L = hl.line;
  auto str = [&](ImpTok t) { return std::string(text + t.b, t.n()); };
  switch (bit) {
    case IMP_ERR_SHORT_LINE: return "short record line in " + where;
    case IMP_ERR_CONTIG: return "contig " + str(imp_column(L, 0)) + " is not in the vid mapping (" + where + ")";
    case IMP_ERR_COORD_TEXT: {
      const ImpTok pos = imp_column(L, 1);
      int64_t v;
      ImpTok endv;
      if (!imp_parse_int(text + pos.b, pos.n(), &v)) import_parse_int(text + pos.b, pos.n(), "POS");       // throws when the host would
      else if (imp_info_find(text, imp_column(L, 7), "END", 3u, &endv)) import_parse_int(text + endv.b, endv.n(), "END");
      return "POS / END not in plain decimal form: not imported by the device importer of this build (" + where + ")";
    }
    case IMP_ERR_COORD_RANGE: return "a column outside what the device importer's (column, row) sort key holds (" + where + ")";
    case IMP_ERR_FILTER: {
      const ImpTok filter = imp_column(L, 6);
      uint32_t at = filter.b;
      ImpTok f;
      while (imp_next(text, &at, filter.e, ';', &f)) {
        bool known = false;
        for (const ImpName& n : H.fields) known = known || imp_tok_eq(text, f, H.names.data() + n.off, n.len);
        if (!known) return "FILTER " + str(f) + " is not in the vid mapping (" + where + ")";
      }
      break;
    }
    case IMP_ERR_COUNT: {
      const ImpTok info = imp_column(L, 7);
      for (size_t i = 0; i < H.info.size(); ++i) {
        const ImpAttr& a = H.info[i];
        ImpTok v;
        if (!a.fixed || a.elem > GDB_ET_FLOAT || !imp_info_find(text, info, H.names.data() + a.name_off, a.name_len, &v) || imp_is_dot(text, v)) continue;
        const uint32_t n = imp_count_pieces(text, v, ',');
        if (n != a.num_elements) return "field " + H.info_names[i] + ": " + std::to_string(n) + " values, expected " + std::to_string(a.num_elements) + " (" + where + ")";
      }
      return "a fixed-length FORMAT field with a wrong number of values (" + where + ")";
    }
    default: break;
  }
  return "malformed record (" + where + ")";
}

// the same for a line of a CSV cell file (ImpCsvErr bits, core/gdb_import_csv.hpp)
inline std::string describe_csv_error(uint32_t bit, const std::string& where) {
  using namespace gdbimp;
  switch (bit) {
    case IMP_ERR_CSV_QUOTE: return "a '\"' in a CSV line: quoted tokens are not imported (" + where + ")";
    case IMP_ERR_CSV_COORD: return "row, column or END of a CSV line cannot be parsed as a 64-bit integer (" + where + ")";
    case IMP_ERR_CSV_COUNT: return "a count token of a CSV line is null, negative, not a number or runs past the line (" + where + ")";
    case IMP_ERR_CSV_EXTRA: return "tokens left over after the last attribute of a CSV line (" + where + ")";
    case IMP_ERR_CSV_OPEN: return "a CSV line ends before its last attribute (" + where + ")";
    case IMP_ERR_COORD_RANGE: return "a column outside what the device importer's (column, row) sort key holds (" + where + ")";
    default: break;
  }
  return "malformed CSV line (" + where + ")";
}

inline uint32_t first_import_error_bit(uint32_t bits) { for (uint32_t b = 1; b; b <<= 1) if (bits & b) return b; return 0; }

}  // namespace genomicsdb_amd
