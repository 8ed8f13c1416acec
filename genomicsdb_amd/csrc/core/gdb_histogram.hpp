// gdb_histogram.hpp - bodies of the input histogram (vcf_histogram): which bin of a uniform histogram over the columns a record line
// of (g)VCF text, or a BCF2 record, counts for.  Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of
// kernels/gdb_histogram.hip and the CPU harness tests/hostsim_histogram/ run the same code.
//
// The arithmetic is the reference's UniformHistogram (utils/histogram.{h,cc}) with lo = 0 and hi = max_histogram_range:
//   size_of_bin = (hi - lo + 1 + (num_bins - 1)) / num_bins          (the ceiling)
//   bin         = (value - lo) / size_of_bin
//   the text form names bin b as lo + b * size_of_bin , lo + (b + 1) * size_of_bin - 1
// and the value of a record is its column: contig offset + POS - 1 (File2TileDBBinaryBase::create_histogram,
// tiledb_loader_file_base.cc:483-512, adds the record's column once per enabled callset of the file - the weight, which the caller
// multiplies in).  A record counts iff its column lies in [column_begin, column_end] of the loader's partition; the histogram always
// spans [0, max_histogram_range].  A counted column above max_histogram_range is the reference's HistogramException ("outsize the
// range"): here the error bit IMP_ERR_HIST_RANGE.
//
// Two differences from the reference ("Histogram of the input files"):
//   - the reference reaches the partition by a tabix seek, which can also fetch a record that begins in front of the partition and
//     reaches into it; such a record is not counted here: only the column a record begins at decides;
//   - a line the reference's reader would skip or misread (contig not in the vid, POS / END that is no plain integer, a short
//     line) is an error named by file and line, in the splitter's words (the CHROM / POS / END parse is the splitter's call,
//     gdbimp::imp_coords_text).
#pragma once
#include <cstdint>

#include "gdb_import_bcf.hpp"

namespace genomicsdb_amd {
namespace gdbhist {

// a free bit of the ImpErr numbering (1 .. 32 text, 64 .. 2048 BCF2, 4096 .. 65536 CSV): it fits the importer's error words
constexpr uint32_t IMP_ERR_HIST_RANGE = 131072u;

struct HistParams {
  uint64_t hi;                        // max_histogram_range (lo is 0)
  uint64_t num_bins, size_of_bin;
  int64_t column_begin, column_end;   // the loader's partition
};
struct HistSel { uint64_t bin; uint32_t err; uint8_t record, counted; };      // record: a record line / record; counted: it counts, for `bin`

GDB_HD uint64_t hist_size_of_bin(uint64_t lo, uint64_t hi, uint64_t num_bins) { return (hi - lo + 1u + (num_bins - 1u)) / num_bins; }
GDB_HD uint64_t hist_bin_of(const HistParams& P, uint64_t value) { return value / P.size_of_bin; }
GDB_HD uint64_t hist_bin_lo(const HistParams& P, uint64_t b) { return b * P.size_of_bin; }
GDB_HD uint64_t hist_bin_hi(const HistParams& P, uint64_t b) { return (b + 1u) * P.size_of_bin - 1u; }
GDB_HD HistParams hist_params(uint64_t max_histogram_range, uint64_t num_bins, int64_t column_begin, int64_t column_end) {
  HistParams P;
  P.hi = max_histogram_range; P.num_bins = num_bins; P.size_of_bin = hist_size_of_bin(0u, max_histogram_range, num_bins);
  P.column_begin = column_begin; P.column_end = column_end;
  return P;
}

// a record that begins at `col`
GDB_HD HistSel hist_column(const HistParams& P, int64_t col) {
  HistSel s; s.bin = 0; s.err = 0; s.record = 1; s.counted = 0;
  if (col < P.column_begin || col > P.column_end) return s;
  if (col < 0 || (uint64_t)col > P.hi) { s.err = IMP_ERR_HIST_RANGE; return s; }
  s.bin = hist_bin_of(P, (uint64_t)col);
  s.counted = 1;
  return s;
}

// one line of a batch of text: L as the importer's index gives it ('\r' cut off).  Empty lines and '#' lines give nothing
GDB_HD HistSel hist_line(const gdbimp::ImpTables& T, const HistParams& P, const gdbimp::ImpLine& L) {
  HistSel none; none.bin = 0; none.err = 0; none.record = 0; none.counted = 0;
  if (L.end == L.begin || L.text[L.begin] == '#') return none;
  int64_t col = 0, tend = 0;
  bool has_end = false;
  const uint32_t e = gdbimp::imp_coords_text(T, L, &col, &tend, &has_end);
  if (e) { none.record = 1; none.err = e; return none; }
  return hist_column(P, col);
}

// one BCF2 record [begin, end) of the batch's bytes: rid and pos through the header's dictionary, as imp_bcf_index reads them
GDB_HD HistSel hist_bcf_record(const gdbimp::ImpBcfTables& B, const HistParams& P, const uint8_t* p, uint32_t begin, uint32_t end) {
  HistSel bad; bad.bin = 0; bad.err = 0; bad.record = 1; bad.counted = 0;
  if (end < begin || end - begin < 32u) { bad.err = gdbimp::IMP_ERR_BCF_BOUNDS; return bad; }
  const int32_t rid = (int32_t)gdbimp::bcf_u32(p, begin + 8u), pos = (int32_t)gdbimp::bcf_u32(p, begin + 12u);      // POS is 0-based here
  if (rid < 0 || rid >= B.n_contig) { bad.err = gdbimp::IMP_ERR_BCF_DICT; return bad; }
  if (B.contig_off[rid] < 0) { bad.err = gdbimp::IMP_ERR_CONTIG; return bad; }
  return hist_column(P, B.contig_off[rid] + (int64_t)pos);
}

}  // namespace gdbhist
}  // namespace genomicsdb_amd
