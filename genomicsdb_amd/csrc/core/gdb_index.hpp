// gdb_index.hpp - bodies of the device tabix builder (.tbi of bgzipped VCF text): the rule of host/vcf_index.cc restated per record.
// Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_index.hip and the CPU harness
// tests/hostsim_index/ run the same code.  Where this text and vcf_index.cc disagree, vcf_index.cc wins: the device builder writes
// the host builder's file, byte for byte.
//
// A line (the bytes up to a newline, a '\r' included; a last line without a newline is a line) is a RECORD iff it is non-empty, does
// not begin with '#' and has at least 4 tabs among its first 8.  Its interval is beg = atoll(POS) - 1, end = beg + len(REF); with a
// 7th tab, the first ';'-separated token of INFO (which runs to the 8th tab or the end of the line) that begins with "END=" and is
// longer than 4 characters overrides end with atoll of what follows; then end <= beg gives end = beg + 1.  atoll as the C library
// reads it: blanks, a sign, digits up to the first non-digit, and like the C library it reads on to the end of the line, not of the
// column.  POS below 1 and POS or END at or above 2^31 are refused (IDX_ERR_*): the host builder's behaviour there is undefined.
//
// Virtual offsets: `ubase` / `coff` are the uncompressed and the file offsets of the BGZF members that hold data (ISIZE > 0), in
// file order.  voff(u) = coff[m] << 16 | (u - ubase[m]) for the member m that contains u; voff(u >= total) = v_total (the file's
// size << 16 when the table is the whole file's).  A record's vbeg = voff(line start), its vend = voff(position behind its newline,
// at most total): a line that ends with its member has its vend at offset 0 of the next member that holds data.
//
// Bin: reg2bin(beg, end) with min_shift 14 and depth 5.  Chunks: a record extends the last chunk of its bin iff the previous record
// OF THE SAME CONTIG had the same bin, so with the records sorted stably by contig id a chunk begins where contig or bin differ
// from the neighbour in front.  Linear index: per 16 kb window of [beg >> 14, (end - 1) >> 14] the smallest vbeg.
#pragma once
#include <cstdint>

#include "gdb_import.hpp"
#include "gdb_index_types.h"

namespace genomicsdb_amd {
namespace gdbidx {

constexpr int kMinShift = 14, kDepth = 5;
constexpr int64_t kCoordLimit = (int64_t)1 << 31;

struct IdxMembers { const uint64_t* ubase; const uint64_t* coff; uint32_t n; uint64_t total, v_total; };
struct IdxRec { uint64_t vbeg, vend; uint32_t bin, w0, w1, err; };

// bin of [beg, end) (SAM specification 5.3 with CSIv1's constants): host/vcf_index.cc's reg2bin
GDB_HD int idx_reg2bin(int64_t beg, int64_t end) {
  int l, s = kMinShift, t = ((1 << (kDepth * 3)) - 1) / 7;
  for (--end, l = kDepth; l > 0; --l, s += 3, t -= 1 << (l * 3))
    if (beg >> s == end >> s) return t + (int)(beg >> s);
  return 0;
}

GDB_HD bool idx_isspace(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
// atoll of text[at, end): the value saturates at +-2^62, far beyond what is accepted
GDB_HD int64_t idx_atoll(const char* text, uint32_t at, uint32_t end) {
  while (at < end && idx_isspace(text[at])) ++at;
  bool neg = false;
  if (at < end && (text[at] == '+' || text[at] == '-')) { neg = text[at] == '-'; ++at; }
  int64_t v = 0;
  const int64_t cap = (int64_t)1 << 62;
  for (; at < end && text[at] >= '0' && text[at] <= '9'; ++at) { v = v * 10 + (text[at] - '0'); if (v > cap) v = cap; }
  return neg ? -v : v;
}

// L: the whole line, a '\r' in front of the newline included; tabs / ntabs: every tab of the line
GDB_HD bool idx_is_record(const gdbimp::ImpLine& L) { return L.end > L.begin && L.text[L.begin] != '#' && L.ntabs >= 4u; }

// the member that contains u < total: the last one with ubase <= u
GDB_HD uint64_t idx_voff(const IdxMembers& M, uint64_t u) {
  if (u >= M.total || M.n == 0u) return M.v_total;
  uint32_t lo = 0, hi = M.n;      // ubase[lo] <= u < ubase[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (M.ubase[mid] <= u) lo = mid; else hi = mid;
  }
  return (M.coff[lo] << 16) | (u - M.ubase[lo]);
}

// a record line; u_text: the uncompressed position of L.text[0]; has_newline: a newline follows L.end
GDB_HD IdxRec idx_record(const IdxMembers& M, const gdbimp::ImpLine& L, uint64_t u_text, bool has_newline) {
  IdxRec r;
  r.err = 0; r.bin = 0; r.w0 = 0; r.w1 = 0;
  r.vbeg = idx_voff(M, u_text + L.begin);
  r.vend = idx_voff(M, u_text + L.end + (has_newline ? 1u : 0u));
  const uint32_t k = L.ntabs < 8u ? L.ntabs : 8u;
  const int64_t pos = idx_atoll(L.text, L.tabs[0] + 1u, L.end);
  int64_t end = pos - 1 + (int64_t)(L.tabs[3] - L.tabs[2] - 1u);
  if (k >= 7u) {
    const uint32_t ie = k >= 8u ? L.tabs[7] : L.end;
    uint32_t p = L.tabs[6] + 1u;
    while (p < ie) {
      uint32_t q = p;
      while (q < ie && L.text[q] != ';') ++q;
      if (q - p > 4u && L.text[p] == 'E' && L.text[p + 1u] == 'N' && L.text[p + 2u] == 'D' && L.text[p + 3u] == '=') {
        end = idx_atoll(L.text, p + 4u, L.end);
        if (end >= kCoordLimit) r.err |= IDX_ERR_RANGE;
        break;
      }
      p = q + 1u;
    }
  }
  if (pos < 1) r.err |= IDX_ERR_POS_LOW;
  if (pos >= kCoordLimit) r.err |= IDX_ERR_RANGE;
  if (r.err) return r;
  const int64_t beg = pos - 1;
  if (end <= beg) end = beg + 1;
  r.bin = (uint32_t)idx_reg2bin(beg, end);
  r.w0 = (uint32_t)(beg >> kMinShift);
  r.w1 = (uint32_t)((end - 1) >> kMinShift);
  return r;
}

// CHROM of a record line: [L.begin, L.tabs[0])
GDB_HD bool idx_same_chrom(const gdbimp::ImpLine& a, const gdbimp::ImpLine& b) {
  const uint32_t n = a.tabs[0] - a.begin;
  if (b.tabs[0] - b.begin != n) return false;
  for (uint32_t i = 0; i < n; ++i) if (a.text[a.begin + i] != b.text[b.begin + i]) return false;
  return true;
}

// records sorted stably by contig id: does record i (contig tid, bin) begin a chunk, given its neighbour in front?
GDB_HD bool idx_chunk_head(bool first, uint32_t tid, uint32_t bin, uint32_t prev_tid, uint32_t prev_bin) { return first || tid != prev_tid || bin != prev_bin; }

// the same order: must the record write window w of its contig, given its neighbour in front?  Not when the neighbour covers w too:
// it comes first in the file, so its vbeg is the smaller one, and it (or one in front of it) writes.  The host builder keeps 0 for
// "no record yet", so a record at virtual offset 0 (the first line of a file without a header) writes no window and hides none
GDB_HD bool idx_window_mine(bool has_prev, uint32_t tid, uint32_t w, uint32_t prev_tid, uint32_t prev_w0, uint32_t prev_w1, uint64_t prev_vbeg) {
  return !(has_prev && prev_vbeg != 0u && prev_tid == tid && prev_w0 <= w && w <= prev_w1);
}

}  // namespace gdbidx
}  // namespace genomicsdb_amd
