// hostsim_import_csv.cc - the CSV path of the device importer driven on the CPU: the files of the callset mapping by their type, batches
// cut behind newlines, the line index, measure, scan, write, deferred tokens, stable sort and gather - the steps of
// kernels/gdb_import.hip as plain loops around the same bodies (core/gdb_import_csv.hpp; core/gdb_import.hpp for the VCF text files
// of a mixed mapping) and the same host share (host/import_common.hpp).  Every batch's text lives in a heap block of its exact
// size, so a sanitizer sees every read outside it.  With -DHOSTSIM_IMPORT_CSV_MAIN the file is a stand-alone program.
// Test infrastructure only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
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
struct Stats { int64_t files = 0, records = 0, cells = 0, spanning = 0, deferred = 0, batches = 0, text_bytes = 0; };
struct Stream { std::string name; const char* data; size_t n; };

std::string strip(const std::exception& e) {
  std::string m = e.what();
  const std::string pre = "VCF2BinaryException : ";
  return m.compare(0, pre.size(), pre) == 0 ? m.substr(pre.size()) : m;
}

std::vector<uint8_t> run(const VidMapper& vid, const ImportOptions& opt, uint64_t budget, const std::vector<Stream>& streams, Stats* stats) {
  const ImportTablesHost H = build_import_tables(vid);
  const std::vector<ImportFile> files = import_files(vid, opt);
  refuse_for_csv(vid, H, files);
  int col_bits = 0;
  while (col_bits < 63 && opt.column_begin > 0 && (opt.column_begin >> col_bits) != 0) ++col_bits;
  const int seq_bits = 64 - col_bits;
  std::vector<uint64_t> row_best((size_t)H.max_row + 1, 0);
  std::vector<uint8_t> bytes;
  std::vector<Slot> slots;
  Stats st;
  int64_t global_line = 0;
  for (const ImportFile& file_ : files) {
    ImportFile file = file_;
    std::string text;
    const Stream* from = nullptr;
    for (const Stream& s : streams) if (s.name == file.name) from = &s;
    const bool csv = file.type != GDB_FILE_VCF;
    if (from) { text.assign(from->data, from->n); file.path = file.name; }
    else if (csv) {
      std::ifstream in(file.path, std::ios::binary);
      if (!in) throw VCF2BinaryException("cannot open " + file.path);
      text.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    } else {
      try { text = gz_text::read_all(file.path); } catch (const std::exception& e) { throw VCF2BinaryException(e.what()); }
    }
    ++st.files;
    ImportHeader hdr;
    std::vector<int64_t> rows;
    if (csv) { refuse_compressed_csv(text.data(), text.size(), file.path); rows = csv_rows_of(file); }
    else hdr = parse_import_header(text, file);
    const std::unique_ptr<int64_t[]> row_table(new int64_t[rows.size()]);     // exact size, like the batch text
    std::copy(rows.begin(), rows.end(), row_table.get());
    const ImpCsvRows R{row_table.get(), (int32_t)rows.size()};
    const ImpTables T = H.view(opt, hdr.n_samples);
    std::vector<int> imported;
    for (int s = 0; s < hdr.n_samples; ++s) if (hdr.sample_row[(size_t)s] >= 0) imported.push_back(s);
    size_t pos = hdr.record_begin;
    int64_t line_no = hdr.lines_before;
    while (pos < text.size()) {
      const size_t stop = import_text_cut(text.data(), text.size(), pos, budget);
      const size_t n = stop - pos;
      ++st.batches;
      st.text_bytes += (int64_t)n;
      const std::unique_ptr<char[]> batch(new char[n]);
      memcpy(batch.get(), text.data() + pos, n);
      pos = stop;
      const char* bt = batch.get();
      for (size_t lb = 0; lb < n;) {
        const void* nl = memchr(bt + lb, '\n', n - lb);
        const size_t le = nl ? (size_t)((const char*)nl - bt) : n;
        ImpHostLine hl(bt, (uint32_t)lb, (uint32_t)le);
        const ImpLine& L = hl.line;
        ++line_no; ++global_line;
        const std::string where = file.path + " line " + std::to_string(line_no);
        auto refuse = [&](uint32_t err) {
          const uint32_t bit = first_import_error_bit(err);
          throw VCF2BinaryException(csv ? describe_csv_error(bit, where) : describe_line_error(bit, H, opt, hdr, bt, (uint32_t)lb, (uint32_t)le, where));
        };
        if (L.end > L.begin && (csv || bt[L.begin] != '#')) ++st.records;
        const size_t n_slots = csv || imported.empty() ? 1 : imported.size();
        for (size_t j = 0; j < n_slots; ++j) {
          const int sample = csv ? 0 : imported.empty() ? -1 : imported[j];
          int64_t row = -1;
          const ImpSlot s = csv ? imp_csv_measure(T, R, L, &row) : imp_measure(T, L, sample);
          if (s.err) refuse(s.err);
          uint64_t tag = 0;
          if (!csv) {
            if (sample < 0 || L.end == L.begin || bt[L.begin] == '#' || s.col > opt.column_end) continue;
            row = hdr.sample_row[(size_t)sample];
            if (opt.column_begin > 0 && s.col <= opt.column_begin) {
              if (seq_bits < 64 && ((uint64_t)global_line >> seq_bits) != 0) throw VCF2BinaryException("too many lines for the partition-begin rule");
              tag = ((uint64_t)s.col << seq_bits) | (uint64_t)global_line;
              row_best[(size_t)row] = std::max(row_best[(size_t)row], tag);
            }
          }
          if (s.kind == IMP_SLOT_NONE) continue;
          std::unique_ptr<uint8_t[]> cell(new uint8_t[s.size]);
          std::vector<ImpDeferred> def(1024);
          uint32_t ndef = 0;
          ImpSink<true> o;
          o.out = cell.get(); o.base = 0; o.def = def.data(); o.ndef = &ndef; o.def_cap = (uint32_t)def.size(); o.line = (uint32_t)line_no;
          const uint32_t err = csv ? imp_csv_write(T, L, s, o, &row) : imp_write(T, L, sample, row, s, o);
          if (err) refuse(err);
          if (o.n != s.size) throw VCF2BinaryException("measure and write disagree (" + where + ")");
          if (ndef > def.size()) throw VCF2BinaryException("more than 1024 deferred values in one cell (" + where + ")");
          for (uint32_t i = 0; i < ndef; ++i) {
            uint32_t v;
            try { v = resolve_deferred(def[i], bt, H); }
            catch (const std::exception& e) { throw VCF2BinaryException(strip(e) + " (" + where + ")"); }
            if (def[i].out_off + 4u > s.size) throw VCF2BinaryException("deferred value outside its cell (" + where + ")");
            memcpy(cell.get() + def[i].out_off, &v, 4);
          }
          st.deferred += ndef;
          const size_t off = bytes.size();
          bytes.insert(bytes.end(), cell.get(), cell.get() + s.size);
          slots.push_back(Slot{imp_sort_key(T, s.col, row), off, s.size, s.kind == IMP_SLOT_SPANNING_CANDIDATE ? tag : 0, row});
        }
        lb = le + 1;
      }
    }
  }
  std::vector<Slot> kept;
  for (const Slot& s : slots) {
    if (s.tag) { if (s.tag != row_best[(size_t)s.row]) continue; ++st.spanning; }
    kept.push_back(s);
  }
  std::stable_sort(kept.begin(), kept.end(), [](const Slot& a, const Slot& b) { return a.key < b.key; });
  std::vector<uint8_t> out;
  out.reserve(bytes.size());
  for (const Slot& s : kept) out.insert(out.end(), bytes.begin() + (ptrdiff_t)s.off, bytes.begin() + (ptrdiff_t)(s.off + s.size));
  st.cells = (int64_t)kept.size();
  if (stats) *stats = st;
  return out;
}

std::vector<uint8_t> run_files(const char* vid_file, const char* callsets_file, const char* file_root, int treat, int64_t column_begin, int64_t column_end, uint64_t budget,
                               const std::vector<Stream>& streams, Stats* st) {
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(vid_file));
  vid.parse_callsets_json(mini_json::parse_file(callsets_file));
  ImportOptions opt;
  opt.treat_deletions_as_intervals = treat != 0;
  opt.column_begin = column_begin; opt.column_end = column_end;
  if (file_root) opt.file_root = file_root;
  return run(vid, opt, budget ? budget : (uint64_t)64 << 20, streams, st);
}
}  // namespace

extern "C" {

const char* hsc_last_error(void) { return g_error.c_str(); }

// stats: files, records, cells, spanning cells, deferred values, batches, text bytes.  A callset file whose "filename" equals
// stream_names[i] is read from stream_data[i] instead
int hsc_import(const char* vid_file, const char* callsets_file, const char* file_root, int treat_deletions_as_intervals, int64_t column_begin, int64_t column_end,
               uint64_t budget, const char* const* stream_names, const char* const* stream_data, const uint64_t* stream_bytes, int n_streams, uint8_t** cells,
               uint64_t* nbytes, int64_t* stats) {
  try {
    std::vector<Stream> streams;
    for (int i = 0; i < n_streams; ++i) streams.push_back(Stream{stream_names[i], stream_data[i], (size_t)stream_bytes[i]});
    Stats st;
    const std::vector<uint8_t> out = run_files(vid_file, callsets_file, file_root, treat_deletions_as_intervals, column_begin, column_end, budget, streams, &st);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *nbytes = out.size();
    if (stats) { stats[0] = st.files; stats[1] = st.records; stats[2] = st.cells; stats[3] = st.spanning; stats[4] = st.deferred; stats[5] = st.batches; stats[6] = st.text_bytes; }
    g_error.clear();
    return 0;
  } catch (const std::exception& e) { g_error = e.what(); return -1; }
}
void hsc_free(void* p) { free(p); }

// the CSV value parsers of the bodies next to strtoll(base 0) / strtof: n NUL-terminated strings at blob + offs[i]
void hsc_check_numbers(const char* blob, const uint32_t* offs, uint32_t n, uint8_t* int_taken, int64_t* int_value, uint8_t* full_ok, int64_t* full_value, uint8_t* ref_int_ok,
                       int64_t* ref_int, uint8_t* float_taken, uint32_t* float_bits, uint8_t* ref_float_ok, uint32_t* ref_float_bits) {
  for (uint32_t i = 0; i < n; ++i) {
    const char* s = blob + offs[i];
    const uint32_t len = (uint32_t)strlen(s);
    int64_t v = 0;
    int_taken[i] = imp_csv_plain_int(s, len, &v) ? 1 : 0; int_value[i] = v;
    v = 0;
    full_ok[i] = (uint8_t)imp_csv_integer(s, len, &v); full_value[i] = v;
    char* e = nullptr;
    ref_int[i] = strtoll(s, &e, 0); ref_int_ok[i] = e != s ? 1 : 0;
    float f = 0;
    float_taken[i] = imp_csv_plain_float(s, len, &f) ? 1 : 0; memcpy(&float_bits[i], &f, 4);
    e = nullptr;
    const float r = strtof(s, &e);
    ref_float_ok[i] = e != s ? 1 : 0; memcpy(&ref_float_bits[i], &r, 4);
  }
}

}  // extern "C"

#ifdef HOSTSIM_IMPORT_CSV_MAIN
// hostsim_import_csv_main <vid> <callsets> <file_root> [budget ...]: imports the mapping once per budget (default: one batch) and
// prints "<budget> <cells> <bytes> <deferred> <batches>" per run; a refusal is printed and counts as a failure
int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <vid.json> <callsets.json> <file_root> [budget ...]\n", argv[0]); return 2; }
  std::vector<uint64_t> budgets;
  for (int i = 4; i < argc; ++i) budgets.push_back(strtoull(argv[i], nullptr, 10));
  if (budgets.empty()) budgets.push_back(0);
  for (uint64_t b : budgets) {
    try {
      Stats st;
      const std::vector<uint8_t> out = run_files(argv[1], argv[2], argv[3], 1, 0, INT64_MAX - 1, b, {}, &st);
      printf("%llu %lld %zu %lld %lld\n", (unsigned long long)b, (long long)st.cells, out.size(), (long long)st.deferred, (long long)st.batches);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
  }
  return 0;
}
#endif
