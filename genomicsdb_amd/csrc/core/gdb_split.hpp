// gdb_split.hpp - bodies of the device splitter (vcf2tiledb --split-files): which column partitions a line of (g)VCF text goes to.
// Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_split.hip and the CPU harness
// tests/hostsim_split/ run the same code.  CHROM, POS and INFO END are parsed by gdb_import.hpp's imp_coords_text, the importer's own.
//
// The rule ("Splitting input files by column partition"): a record line's interval is [col, tend] with
//   col  = contig offset + POS - 1
//   tend = contig offset + END - 1 when INFO carries END (the last END counts), else col + len(REF) - 1   (tabix's VCF rule)
// and the line goes to every partition p whose [begin_p, end_p] it overlaps.  The partitions are given sorted by begin and do not
// overlap each other, so the partitions of a line are one run p_lo .. p_hi of the sorted list.  A '#' line goes to every
// partition, an empty line to none.
#pragma once
#include <cstdint>

#include "gdb_import.hpp"

namespace genomicsdb_amd {
namespace gdbsplit {

constexpr uint32_t kMaxPartitions = 4096;

struct SplitParts { const int64_t* begins; const int64_t* ends; uint32_t n; };      // sorted by begin; end_p < begin_(p+1)
struct SplitSel { uint32_t p_lo, p_hi, err; };                                      // p_lo > p_hi: no partition; err: ImpErr bits
GDB_HD bool split_selected(const SplitSel& s, uint32_t p) { return s.p_lo <= p && p <= s.p_hi; }

// number of v[i] < x (v ascending)
GDB_HD uint32_t split_count_below(const int64_t* v, uint32_t n, int64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < x) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// the run of partitions that [col, tend] overlaps: the first whose end reaches col .. the last whose begin is at or below tend
GDB_HD SplitSel split_partitions_of(const SplitParts& P, int64_t col, int64_t tend) {
  SplitSel s;
  s.err = 0;
  const uint32_t upto = tend == INT64_MAX ? P.n : split_count_below(P.begins, P.n, tend + 1);      // partitions that begin at or below tend
  if (upto == 0u) { s.p_lo = 1u; s.p_hi = 0u; return s; }               // in front of the first partition
  s.p_lo = split_count_below(P.ends, P.n, col);                         // partitions that end in front of col
  s.p_hi = upto - 1u;
  return s;
}

// one line of the batch: L as the importer's index gives it ('\r' cut off)
GDB_HD SplitSel split_classify(const gdbimp::ImpTables& T, const SplitParts& P, const gdbimp::ImpLine& L) {
  SplitSel none; none.p_lo = 1u; none.p_hi = 0u; none.err = 0;
  if (L.end == L.begin) return none;
  if (L.text[L.begin] == '#') { SplitSel all; all.p_lo = 0u; all.p_hi = P.n - 1u; all.err = 0; return P.n ? all : none; }
  int64_t col = 0, tend = 0;
  bool has_end = false;
  const uint32_t e = gdbimp::imp_coords_text(T, L, &col, &tend, &has_end);
  if (e) { none.err = e; return none; }
  if (!has_end) tend = col + (int64_t)gdbimp::imp_column(L, 3).n() - 1;
  return split_partitions_of(P, col, tend);
}

}  // namespace gdbsplit
}  // namespace genomicsdb_amd
