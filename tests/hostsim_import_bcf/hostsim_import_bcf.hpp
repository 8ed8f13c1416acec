// hostsim_import_bcf.hpp - the BCF2 path of the device importer driven on the CPU: header parse, record walk, batches, index,
// measure, scan, write, the partition-begin rule, stable sort and gather - the steps of kernels/gdb_import.hip as plain loops
// around the same bodies (core/gdb_import_bcf.hpp) and the same host share (host/import_bcf.hpp).  Record bytes and the index
// pass's tables live in heap blocks of their exact sizes, so a sanitizer sees every read or write outside them.
// Test infrastructure only.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/host/import_bcf.hpp"

namespace hostsim_bcf {
using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbimp;

struct Slot { uint64_t key, off, size, tag; int64_t row; };
struct Stats { int64_t files = 0, records = 0, cells = 0, spanning = 0, batches = 0; };

// error_bit (optional): the ImpErr / ImpBcfErr bit of a record the bodies refused (0: an error of the header or the walk)
inline std::vector<uint8_t> run(const VidMapper& vid, const ImportOptions& opt, uint64_t budget, const std::function<std::string(const ImportFile&)>& read, Stats* stats,
                                uint32_t* error_bit = nullptr) {
  if (error_bit) *error_bit = 0;
  const ImportTablesHost H = build_import_tables(vid);
  const std::vector<ImportFile> files = import_files(vid, opt);
  int col_bits = 0;
  while (col_bits < 63 && opt.column_begin > 0 && (opt.column_begin >> col_bits) != 0) ++col_bits;
  const int seq_bits = 64 - col_bits;
  std::vector<uint64_t> row_best((size_t)H.max_row + 1, 0);
  std::vector<uint8_t> bytes;
  std::vector<Slot> slots;
  Stats st;
  int64_t global_rec = 0;
  const size_t n_attr = H.info.size() + H.fmt.size();
  for (const ImportFile& file : files) {
    const std::string data = read(file);
    ++st.files;
    if (!is_bcf2(data.data(), data.size())) throw VCF2BinaryException(file.path + " is not BCF2: this harness drives the BCF2 path only");
    const BcfHeaderHost hdr = parse_bcf_header(data.data(), data.size(), file, H);
    const ImpTables T = H.view(opt, hdr.samples.n_samples);
    // the per-file tables in blocks of their exact sizes
    const std::vector<int32_t> dict_info(hdr.dict_info), dict_fmt(hdr.dict_fmt), dict_filter(hdr.dict_filter);
    const std::vector<int64_t> contig_off(hdr.contig_off);
    ImpBcfTables B = hdr.view();
    B.dict_info = dict_info.data(); B.dict_fmt = dict_fmt.data(); B.dict_filter = dict_filter.data(); B.contig_off = contig_off.data();
    std::vector<int> imported;
    for (int s = 0; s < hdr.samples.n_samples; ++s) if (hdr.samples.sample_row[(size_t)s] >= 0) imported.push_back(s);
    std::vector<uint64_t> offs;
    bcf_walk_records(data.data(), data.size(), hdr.records_begin, file.path, offs);
    for (size_t first = 0; first + 1 < offs.size();) {
      const size_t last = bcf_next_batch(offs, first, budget);
      ++st.batches;
      const uint64_t base = offs[first], n_bytes = offs[last] - base;
      const uint32_t n_rec = (uint32_t)(last - first);
      std::unique_ptr<uint8_t[]> batch(new uint8_t[n_bytes]);
      memcpy(batch.get(), data.data() + base, n_bytes);
      std::unique_ptr<ImpBcfRec[]> rec(new ImpBcfRec[n_rec]);
      std::unique_ptr<ImpBcfField[]> fld(new ImpBcfField[(size_t)n_rec * n_attr]);
      // ---- index
      for (uint32_t r = 0; r < n_rec; ++r)
        imp_bcf_index(T, B, batch.get(), (uint32_t)(offs[first + r] - base), (uint32_t)(offs[first + r + 1] - base), &rec[r], fld.get() + (size_t)r * n_attr);
      // ---- measure and write, one (record, imported sample) at a time
      for (uint32_t r = 0; r < n_rec; ++r) {
        ++global_rec; ++st.records;
        const std::string where = file.path + " record " + std::to_string(first + r + 1);
        auto refuse = [&](uint32_t err) {
          const uint32_t bit = first_import_error_bit(err);
          if (error_bit) *error_bit = bit;
          throw VCF2BinaryException(describe_bcf_error(bit, H, opt, hdr, batch.get(), (uint32_t)(offs[first + r] - base), (uint32_t)(offs[first + r + 1] - base), where));
        };
        const ImpBcfField* F = fld.get() + (size_t)r * n_attr;
        const size_t n_slots = imported.empty() ? 1 : imported.size();
        for (size_t j = 0; j < n_slots; ++j) {
          const int sample = imported.empty() ? -1 : imported[j];
          const ImpSlot s = imp_bcf_measure(T, B, batch.get(), rec[r], F, sample);
          if (s.err) refuse(s.err);
          if (sample < 0 || s.col > opt.column_end) continue;
          const int64_t row = hdr.samples.sample_row[(size_t)sample];
          uint64_t tag = 0;
          if (opt.column_begin > 0 && s.col <= opt.column_begin) {
            if (seq_bits < 64 && ((uint64_t)global_rec >> seq_bits) != 0) throw VCF2BinaryException("too many records for the partition-begin rule");
            tag = ((uint64_t)s.col << seq_bits) | (uint64_t)global_rec;
            row_best[(size_t)row] = std::max(row_best[(size_t)row], tag);
          }
          if (s.kind == IMP_SLOT_NONE) continue;
          std::unique_ptr<uint8_t[]> cell(new uint8_t[s.size]);
          ImpSink<true> o;
          o.out = cell.get();
          const uint32_t err = imp_bcf_write(T, B, batch.get(), rec[r], F, sample, row, s, o);
          if (o.n != s.size) throw VCF2BinaryException("measure and write disagree (" + where + ")");
          if (err) refuse(err);
          const size_t off = bytes.size();
          bytes.insert(bytes.end(), cell.get(), cell.get() + s.size);
          slots.push_back(Slot{imp_sort_key(T, s.col, row), off, s.size, s.kind == IMP_SLOT_SPANNING_CANDIDATE ? tag : 0, row});
        }
      }
      first = last;
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

}  // namespace hostsim_bcf
