// hostsim_import.cc - the bodies of the device importer (core/gdb_import.hpp) driven on the CPU, line by line: measure, scan,
// write, deferred tokens, the partition-begin rule, stable sort and gather - the steps of kernels/gdb_import.hip as plain loops
// around the same functions and the same host share (host/import_common.hpp).  Test infrastructure only.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/common/gz_text.hpp"
#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"
#include "../../genomicsdb_amd/csrc/host/import_common.hpp"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbimp;

namespace {
thread_local std::string g_error;

struct Slot { uint64_t key, off, size, tag; int64_t row; };

std::vector<uint8_t> run(const VidMapper& vid, const ImportOptions& opt, int64_t* stats) {
  const ImportTablesHost H = build_import_tables(vid);
  const std::vector<ImportFile> files = import_files(vid, opt);
  int col_bits = 0;
  while (col_bits < 63 && opt.column_begin > 0 && (opt.column_begin >> col_bits) != 0) ++col_bits;
  const int seq_bits = 64 - col_bits;
  std::vector<uint64_t> row_best((size_t)H.max_row + 1, 0);
  std::vector<uint8_t> bytes;
  std::vector<Slot> slots;
  int64_t records = 0, deferred = 0, global_line = 0;
  for (const ImportFile& file : files) {
    std::string text;
    try { text = gz_text::read_all(file.path); } catch (const std::exception& e) { throw VCF2BinaryException(e.what()); }
    const ImportHeader hdr = parse_import_header(text, file);
    const ImpTables T = H.view(opt, hdr.n_samples);
    std::vector<int> imported;
    for (int s = 0; s < hdr.n_samples; ++s) if (hdr.sample_row[(size_t)s] >= 0) imported.push_back(s);
    size_t pos = hdr.record_begin;
    int64_t line_no = hdr.lines_before;
    while (pos < text.size()) {
      size_t eol = text.find('\n', pos);
      if (eol == std::string::npos) eol = text.size();
      ImpHostLine hl(text.data(), (uint32_t)pos, (uint32_t)eol);
      const ImpLine& L = hl.line;
      const uint32_t lb = (uint32_t)pos, le = (uint32_t)eol;
      pos = eol + 1;
      ++line_no; ++global_line;
      const std::string where = file.path + " line " + std::to_string(line_no);
      if (L.end > L.begin && text[L.begin] != '#') ++records;
      const size_t n_slots = imported.empty() ? 1 : imported.size();
      for (size_t j = 0; j < n_slots; ++j) {
        const int sample = imported.empty() ? -1 : imported[j];
        const ImpSlot s = imp_measure(T, L, sample);
        if (s.err) throw VCF2BinaryException(describe_line_error(first_import_error_bit(s.err), H, opt, hdr, text.data(), lb, le, where));
        if (sample < 0 || L.end == L.begin || text[L.begin] == '#' || s.col > opt.column_end) continue;
        const int64_t row = hdr.sample_row[(size_t)sample];
        uint64_t tag = 0;
        if (opt.column_begin > 0 && s.col <= opt.column_begin) {
          if (seq_bits < 64 && ((uint64_t)global_line >> seq_bits) != 0) throw VCF2BinaryException("too many lines for the partition-begin rule");
          tag = ((uint64_t)s.col << seq_bits) | (uint64_t)global_line;
          row_best[(size_t)row] = std::max(row_best[(size_t)row], tag);
        }
        if (s.kind == IMP_SLOT_NONE) continue;
        const size_t off = bytes.size();
        bytes.resize(off + s.size);
        std::vector<ImpDeferred> def(1024);
        uint32_t ndef = 0;
        ImpSink<true> o;
        o.out = bytes.data() + off; o.base = off; o.def = def.data(); o.ndef = &ndef; o.def_cap = (uint32_t)def.size(); o.line = (uint32_t)line_no;
        const uint32_t err = imp_write(T, L, sample, row, s, o);
        if (o.n != s.size) throw VCF2BinaryException("measure and write disagree (" + where + ")");
        if (err) throw VCF2BinaryException(describe_line_error(first_import_error_bit(err), H, opt, hdr, text.data(), lb, le, where));
        if (ndef > def.size()) throw VCF2BinaryException("more than 1024 deferred values in one cell (" + where + ")");
        for (uint32_t i = 0; i < ndef; ++i) {
          uint32_t v;
          try { v = resolve_deferred(def[i], text.data(), H); }
          catch (const std::exception& e) { std::string m = e.what(); const std::string pre = "VCF2BinaryException : "; if (m.compare(0, pre.size(), pre) == 0) m = m.substr(pre.size()); throw VCF2BinaryException(m + " (" + where + ")"); }
          memcpy(bytes.data() + def[i].out_off, &v, 4);
        }
        deferred += ndef;
        slots.push_back(Slot{imp_sort_key(T, s.col, row), off, s.size, s.kind == IMP_SLOT_SPANNING_CANDIDATE ? tag : 0, row});
      }
    }
  }
  int64_t spanning = 0;
  std::vector<Slot> kept;
  for (const Slot& s : slots) {
    if (s.tag) { if (s.tag != row_best[(size_t)s.row]) continue; ++spanning; }
    kept.push_back(s);
  }
  std::stable_sort(kept.begin(), kept.end(), [](const Slot& a, const Slot& b) { return a.key < b.key; });
  std::vector<uint8_t> out;
  out.reserve(bytes.size());
  for (const Slot& s : kept) out.insert(out.end(), bytes.begin() + (ptrdiff_t)s.off, bytes.begin() + (ptrdiff_t)(s.off + s.size));
  if (stats) { stats[0] = (int64_t)files.size(); stats[1] = records; stats[2] = (int64_t)kept.size(); stats[3] = spanning; stats[4] = deferred; }
  return out;
}
}  // namespace

extern "C" {

const char* hsi_last_error(void) { return g_error.c_str(); }

// stats: files, records, cells, spanning cells, deferred values
int hsi_import(const char* vid_file, const char* callsets_file, const char* file_root, int treat_deletions_as_intervals, int64_t column_begin, int64_t column_end,
               uint8_t** cells, uint64_t* nbytes, int64_t* stats) {
  try {
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_file));
    vid.parse_callsets_json(mini_json::parse_file(callsets_file));
    ImportOptions opt;
    opt.treat_deletions_as_intervals = treat_deletions_as_intervals != 0;
    opt.column_begin = column_begin; opt.column_end = column_end;
    if (file_root) opt.file_root = file_root;
    const std::vector<uint8_t> out = run(vid, opt, stats);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *nbytes = out.size();
    g_error.clear();
    return 0;
  } catch (const std::exception& e) { g_error = e.what(); return -1; }
}
void hsi_free(void* p) { free(p); }

// n NUL-terminated strings at blob + offs[i]: fast path (accepted, bits) next to (float)strtod over the whole string (ok, bits)
void hsi_check_floats(const char* blob, const uint32_t* offs, uint32_t n, uint8_t* accepted, uint32_t* bits, uint8_t* ref_ok, uint32_t* ref_bits) {
  for (uint32_t i = 0; i < n; ++i) {
    const char* s = blob + offs[i];
    float f = 0;
    accepted[i] = imp_parse_float(s, (uint32_t)strlen(s), &f) ? 1 : 0;
    memcpy(&bits[i], &f, 4);
    char* e = nullptr;
    const float r = (float)strtod(s, &e);
    ref_ok[i] = (*s && !*e) ? 1 : 0;
    memcpy(&ref_bits[i], &r, 4);
  }
}
void hsi_check_ints(const char* blob, const uint32_t* offs, uint32_t n, uint8_t* accepted, int64_t* values, uint8_t* ref_ok, int64_t* ref_values) {
  for (uint32_t i = 0; i < n; ++i) {
    const char* s = blob + offs[i];
    int64_t v = 0;
    accepted[i] = imp_parse_int(s, (uint32_t)strlen(s), &v) ? 1 : 0;
    values[i] = v;
    char* e = nullptr;
    ref_values[i] = strtoll(s, &e, 10);
    ref_ok[i] = (*s && !*e) ? 1 : 0;
  }
}

}  // extern "C"
