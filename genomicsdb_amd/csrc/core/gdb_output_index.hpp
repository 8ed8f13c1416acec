// gdb_output_index.hpp - bodies of the index of the combined output (.tbi of the "z" stream, .csi of the "b" stream), built page by
// page while the page is in device memory.  Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of
// kernels/gdb_output_index.hip and the CPU harness tests/hostsim_output_index/ run the same code.  The file is the one the host
// builders of host/vcf_index.cc write when they re-read the finished file, byte for byte; where the two disagree, vcf_index.cc wins.
//
// A page is cut into records by the pipeline's record offsets, so no newline / tab pass over the page is needed: record k is the
// bytes [rec_off[k] - base, rec_off[k + 1] - base) of the page.
//   text   the rule of gdbidx::idx_record (core/gdb_index.hpp), called on the record's first 8 tabs: POS, len(REF), the first END= token
//          of INFO, end <= beg -> beg + 1, the IDX_ERR_* bits.  CHROM is looked up among the names of the header's ##contig lines
//          (every contig of the output has one): the name of the record in front of the page first, then its successor, then all of
//          them.  The host turns these header positions into the .tbi's ids, which follow first appearance.  A line the host builder
//          would not index (fewer than 4 tabs, '#') gets no contig.
//   BCF2   CHROM, POS, rlen are the three int32 at byte 8 of the record; the interval is [pos, pos + max(1, rlen)); a negative CHROM
//          is not indexed (build_csi_index).
// Virtual offsets are PAGE-RELATIVE: the page is deflated in blocks of B input bytes (the last one shorter), boff[0 .. nblocks] are
// the blocks' compressed offsets inside the page, voff(u) = boff[u / B] << 16 | u % B and voff(page size) = boff[nblocks] << 16.  The
// host adds the page's offset in the file (<< 16) to every chunk bound and window minimum, so nothing here depends on how much the
// pages in front compressed to.  The stream begins with the header's block, so no record of the file is at virtual offset 0 and
// the host builder's "0 = no record yet" never meets a record: the window rule runs without that exception (prev_vbeg = 1).
//
// Chunks and windows: gdbidx::idx_chunk_head and gdbidx::idx_window_mine over the records sorted stably by contig.
#pragma once
#include <cstdint>

#include "gdb_index.hpp"

namespace genomicsdb_amd {
namespace gdboidx {

constexpr uint32_t kNoContig = 0xFFFFFFFFu;        // the record is not indexed
constexpr uint32_t OIDX_ERR_CHROM = 4u;            // a CHROM that the header does not name (text), or an id at or above n_ref (BCF2)
constexpr uint32_t OIDX_ERR_SHAPE = 8u;            // record offsets that leave the page, a record of 4 GiB or more, a BCF2 record below 20 bytes

struct OutRec { uint32_t bin, w0, w1, kid, err; };      // kid: position among the header's contigs

// name k = bytes[off[k], off[k + 1])
struct ContigTable { const char* bytes; const uint32_t* off; uint32_t n; };

GDB_HD bool oidx_name_is(const ContigTable& C, uint32_t k, const char* t, uint32_t n) {
  const uint32_t a = C.off[k];
  if (C.off[k + 1u] - a != n) return false;
  for (uint32_t i = 0; i < n; ++i) if (C.bytes[a + i] != t[i]) return false;
  return true;
}
// hint: the contig of the record in front of the page (any value: kNoContig for none)
GDB_HD uint32_t oidx_contig_of(const ContigTable& C, const char* t, uint32_t n, uint32_t hint) {
  if (hint < C.n && oidx_name_is(C, hint, t, n)) return hint;
  if (hint < C.n && hint + 1u < C.n && oidx_name_is(C, hint + 1u, t, n)) return hint + 1u;
  for (uint32_t k = 0; k < C.n; ++k) if (oidx_name_is(C, k, t, n)) return k;
  return kNoContig;
}

GDB_HD uint32_t oidx_next_tab(const char* t, uint32_t at, uint32_t end) {
  while (at < end && t[at] != '\t') ++at;
  return at;
}

// one record of a text page: t[0, len), its newline included
GDB_HD OutRec oidx_text_record(const char* t, uint32_t len, const ContigTable& C, uint32_t hint) {
  OutRec o;
  o.bin = 0; o.w0 = 0; o.w1 = 0; o.kid = kNoContig; o.err = 0;
  const uint32_t end = (len && t[len - 1u] == '\n') ? len - 1u : len;
  // the first 8 tabs, each in a variable of its own: the positions stay in registers
  const uint32_t t0 = oidx_next_tab(t, 0u, end);
  const uint32_t t1 = oidx_next_tab(t, t0 < end ? t0 + 1u : end, end);
  const uint32_t t2 = oidx_next_tab(t, t1 < end ? t1 + 1u : end, end);
  const uint32_t t3 = oidx_next_tab(t, t2 < end ? t2 + 1u : end, end);
  const uint32_t t4 = oidx_next_tab(t, t3 < end ? t3 + 1u : end, end);
  const uint32_t t5 = oidx_next_tab(t, t4 < end ? t4 + 1u : end, end);
  const uint32_t t6 = oidx_next_tab(t, t5 < end ? t5 + 1u : end, end);
  const uint32_t t7 = oidx_next_tab(t, t6 < end ? t6 + 1u : end, end);
  const uint32_t tabs[8] = {t0, t1, t2, t3, t4, t5, t6, t7};
  const uint32_t ntabs = (t0 < end) + (t1 < end) + (t2 < end) + (t3 < end) + (t4 < end) + (t5 < end) + (t6 < end) + (t7 < end);
  gdbimp::ImpLine L;
  L.text = t; L.begin = 0u; L.end = end; L.tabs = tabs; L.ntabs = ntabs;
  if (!gdbidx::idx_is_record(L)) return o;
  const gdbidx::IdxMembers none{nullptr, nullptr, 0u, 0u, 0u};      // (the offsets are taken behind the deflate: oidx_voff)
  const gdbidx::IdxRec r = gdbidx::idx_record(none, L, 0u, true);
  o.err = r.err; o.bin = r.bin; o.w0 = r.w0; o.w1 = r.w1;
  o.kid = oidx_contig_of(C, t, t0, hint);
  if (o.kid == kNoContig) o.err |= OIDX_ERR_CHROM;
  return o;
}

GDB_HD int32_t oidx_le32(const uint8_t* p) { return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }

// one record of a BCF2 page: l_shared, l_indiv, then CHROM, POS, rlen
GDB_HD OutRec oidx_bcf_record(const uint8_t* rec, uint64_t len, uint32_t n_ref) {
  OutRec o;
  o.bin = 0; o.w0 = 0; o.w1 = 0; o.kid = kNoContig; o.err = 0;
  if (len < 20u) { o.err = OIDX_ERR_SHAPE; return o; }
  const int32_t chrom = oidx_le32(rec + 8), pos = oidx_le32(rec + 12), rlen = oidx_le32(rec + 16);
  if (chrom < 0) return o;
  if ((uint32_t)chrom >= n_ref) { o.err = OIDX_ERR_CHROM; return o; }
  if (pos < 0) { o.err = gdbidx::IDX_ERR_POS_LOW; return o; }
  const int64_t beg = pos, end = (int64_t)pos + (rlen > 1 ? rlen : 1);
  o.kid = (uint32_t)chrom;
  o.bin = (uint32_t)gdbidx::idx_reg2bin(beg, end);
  o.w0 = (uint32_t)(beg >> gdbidx::kMinShift);
  o.w1 = (uint32_t)((end - 1) >> gdbidx::kMinShift);
  return o;
}

// page-relative virtual offset of the uncompressed page offset u; B: input bytes per block
GDB_HD uint64_t oidx_voff(const uint64_t* boff, uint32_t nblocks, uint32_t B, uint64_t page_bytes, uint64_t u) {
  if (u >= page_bytes) return boff[nblocks] << 16;
  return (boff[u / B] << 16) | (u % B);
}

// records sorted stably by contig (kid_s; n_kid and above: not indexed, they come last): is record i the last one of its chunk?
GDB_HD bool oidx_chunk_tail(bool last, uint32_t next_kid, uint32_t n_kid, bool next_is_head) { return last || next_kid >= n_kid || next_is_head; }

}  // namespace gdboidx
}  // namespace genomicsdb_amd
