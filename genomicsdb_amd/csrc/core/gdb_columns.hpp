// gdb_columns.hpp - bodies of the column decoder: a page of BCF2 records (what k_bcf_write leaves in the arena, or any other
// stream of BCF2 records) -> typed columns: the site columns per record, requested INFO fields [R, W], requested FORMAT fields
// [R, N, W].  Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_columns.hip and the CPU harness
// tests/hostsim_columns/ run the same code.  No allocation in the bodies.
//
// A record is [l_shared u32][l_indiv u32][shared block][individual block] (VCFv4.2/BCFv2.2 specification, section 6), decoded as the
// specification lays it out - typed descriptors with the count-15 overflow, int8 / int16 / int32 / float / char vectors, FORMAT
// blocks of n_sample x L elements of one type - and not only as this build's encoder writes it.
//
//   col_measure  one record: walks both blocks, checks every length against the end of its block, leaves one ColEntry per
//                requested field (present, byte offset of its block in the page, BCF type, vector length L), the byte length of the
//                record's alleles joined by ',', and folds L into the page's per-field maximum
//   col_site     one record: contig, pos, end, column, qual, n_allele, the joined alleles
//   col_scatter  one (record, sample, requested field): the sample's L elements converted to the requested dtype, W elements written
//
// Sentinels of the output are BCF's own for the output dtype: missing -128 / -32768 / INT32_MIN / 0x7F800001, end-of-vector the
// next value up.  Elements behind L up to W are end-of-vector; a field the record does not have is [missing, end-of-vector, ...].
// So is a sample whose vector is end-of-vector from its first element on (how htslib pads a sample without a GT).
// Nothing is truncated or wrapped: a vector longer than a given width and an integer outside [BCF_MIN_BT, BCF_MAX_BT] of the output
// dtype (htslib's bounds: the eight values below each type's minimum are reserved) are faults that name field and record.
#pragma once
#include "gdb_import_bcf.hpp"

#include <string>

namespace genomicsdb_amd {
namespace gdbcol {
using namespace gdbimp;      // the typed-descriptor readers of the BCF2 importer: bcf_desc, bcf_typed_int, bcf_int, bcf_width

constexpr int kColMaxFields = GDB_MAX_COLUMN_REQUESTS;                 // requested fields of one selection
enum ColDtype { COL_INT8 = 1, COL_INT16 = 2, COL_INT32 = 3, COL_INT64 = 4, COL_FLOAT32 = 5, COL_UINT8 = 6 };   // 1, 2, 3, 5: the BCF type codes
// faults, per kind a mask of the fields that raised it
enum ColErrKind { COL_ERR_RECORD = 0,   // a record that is no BCF2 record: a length past its block, an unknown type code, n_sample or rid outside the header's
                  COL_ERR_TYPE = 1,     // float values for an integer field, integers for a float field, char data for either
                  COL_ERR_WIDTH = 2,    // a vector longer than the width the caller gave
                  COL_ERR_RANGE = 3,    // an integer outside the output dtype
                  kColErrKinds = 4 };
constexpr int kColErrWords = 1 + kColErrKinds * kColMaxFields;      // [0]: kinds raised (bit k), [1 + k * kColMaxFields + f]: smallest record that raised kind k for field f
struct ColFault { uint32_t mask[kColErrKinds]; };

struct ColField { int32_t key; int32_t dtype; int32_t width; uint8_t is_info, is_float, is_gt, pad; };      // key: id in the header's dictionary; width 0: the page's longest vector
struct ColFields { int32_t n; ColField f[kColMaxFields]; };
struct ColEntry { uint64_t off; uint32_t len; uint8_t type, present, pad[2]; };      // off: of the block (FORMAT: sample 0's values) from the page's first byte; len: L
struct ColRecord { uint32_t alleles_at, n_allele; };                                  // alleles_at: REF's typed descriptor, from the record's first byte

GDB_HD uint32_t col_dtype_size(int32_t d) { return d == COL_INT8 || d == COL_UINT8 ? 1u : d == COL_INT16 ? 2u : d == COL_INT64 ? 8u : 4u; }
GDB_HD int32_t col_missing(int32_t d) { return d == COL_INT8 ? -128 : d == COL_INT16 ? -32768 : d == COL_FLOAT32 ? (int32_t)kBcfFloatMissingBits : INT32_MIN; }
GDB_HD int32_t col_vector_end(int32_t d) { return col_missing(d) + 1; }
// htslib's BCF_MIN_BT_* / BCF_MAX_BT_*
GDB_HD bool col_fits(int32_t v, int32_t d) {
  return d == COL_INT8 ? (v >= -120 && v <= 127) : d == COL_INT16 ? (v >= -32760 && v <= 32767) : v >= INT32_MIN + 8;
}
GDB_HD void col_store(void* out, int32_t d, uint32_t i, int32_t v) {
  if (d == COL_INT8) ((int8_t*)out)[i] = (int8_t)v;
  else if (d == COL_INT16) ((int16_t*)out)[i] = (int16_t)v;
  else ((int32_t*)out)[i] = v;      // int32, and the bits of a float32
}

// ---- what differs between a kernel and the CPU harness: the two read-modify-write operations ------------------------------------
GDB_HD void col_min_u32(uint32_t* at, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(at, v);
#else
  if (v < *at) *at = v;
#endif
}
GDB_HD void col_max_u32(uint32_t* at, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (v > *(volatile uint32_t*)at) atomicMax(at, v);      // (the word only grows: a stale read costs one atomic more, never a lost maximum; nearly every record skips it)
#else
  if (v > *at) *at = v;
#endif
}
GDB_HD void col_or_u32(uint32_t* at, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(at, v);
#else
  *at |= v;
#endif
}
// err: kColErrWords words, [0] zeroed and the others 0xFFFFFFFF in front of the pass
GDB_HD void col_raise(uint32_t* err, const ColFault& f, uint32_t record) {
  for (uint32_t k = 0; k < (uint32_t)kColErrKinds; ++k) {
    if (!f.mask[k]) continue;
    col_or_u32(&err[0], 1u << k);
    for (uint32_t i = 0; i < (uint32_t)kColMaxFields; ++i) if (f.mask[k] & (1u << i)) col_min_u32(&err[1u + k * kColMaxFields + i], record);
  }
}
GDB_HD bool col_faulted(const ColFault& f) { return (f.mask[0] | f.mask[1] | f.mask[2] | f.mask[3]) != 0u; }

// ---- measure: one record -------------------------------------------------------------------------------------------------------
// The record is page[rb, re).  E: Q.n entries.  max_len: Q.n words, the page's longest vector of every field (a field the record
// does not have counts 1: its column holds one missing value).  *requested_bytes: bytes of the record the later passes read (the
// shared block and the blocks of the requested FORMAT fields).
GDB_HD ColFault col_measure(const ColFields& Q, const uint8_t* page, uint64_t rb, uint64_t re, int32_t n_sample_header, int32_t n_contig, ColEntry* E, ColRecord* R,
                            int64_t* alleles_len, uint32_t* max_len, uint64_t* requested_bytes) {
  ColFault fault; fault.mask[0] = fault.mask[1] = fault.mask[2] = fault.mask[3] = 0u;
  for (int32_t i = 0; i < Q.n; ++i) { E[i].off = 0; E[i].len = 0; E[i].type = 0; E[i].present = 0; E[i].pad[0] = E[i].pad[1] = 0; }
  R->alleles_at = 0; R->n_allele = 0; *alleles_len = 0; *requested_bytes = 0;
#define COL_BAD_RECORD do { fault.mask[COL_ERR_RECORD] = 1u; return fault; } while (0)
  if (re < rb || re - rb < 32u || re - rb > 0xFFFFFFFFull) COL_BAD_RECORD;
  const uint8_t* p = page + rb;
  const uint32_t end = (uint32_t)(re - rb);
  const uint32_t l_shared = bcf_u32(p, 0), l_indiv = bcf_u32(p, 4);
  if (l_shared < 24u || (uint64_t)l_shared + (uint64_t)l_indiv + 8u != (uint64_t)end) COL_BAD_RECORD;
  const uint32_t sh_end = 8u + l_shared;
  const int32_t rid = (int32_t)bcf_u32(p, 8);
  const uint32_t n_allele_info = bcf_u32(p, 24), n_fmt_sample = bcf_u32(p, 28);
  const uint32_t n_info = n_allele_info & 0xFFFFu, n_allele = n_allele_info >> 16, n_sample = n_fmt_sample & 0xFFFFFFu, n_fmt = n_fmt_sample >> 24;
  if (n_sample != (uint32_t)n_sample_header) COL_BAD_RECORD;
  if (rid < 0 || rid >= n_contig) COL_BAD_RECORD;
  uint32_t at = 32u, n, t;
  // ID: a typed string
  if (bcf_desc(p, &at, sh_end, &n, &t)) COL_BAD_RECORD;
  if (t != BCF_T_CHAR && n != 0u) COL_BAD_RECORD;
  at += n;
  // REF and the ALTs: typed strings
  R->alleles_at = at; R->n_allele = n_allele;
  uint64_t joined = n_allele ? n_allele - 1u : 0u;
  for (uint32_t k = 0; k < n_allele; ++k) {
    if (bcf_desc(p, &at, sh_end, &n, &t)) COL_BAD_RECORD;
    if (t != BCF_T_CHAR && n != 0u) COL_BAD_RECORD;
    at += n; joined += n;
  }
  // FILTER: a vector of dictionary ids
  if (bcf_desc(p, &at, sh_end, &n, &t)) COL_BAD_RECORD;
  if (!bcf_is_int(t) && n != 0u) COL_BAD_RECORD;
  at += n * bcf_width(t);
  // INFO: (key, typed vector) pairs, any type; the last pair of a key counts
  for (uint32_t k = 0; k < n_info; ++k) {
    int32_t key;
    if (bcf_typed_int(p, &at, sh_end, &key)) COL_BAD_RECORD;
    if (bcf_desc(p, &at, sh_end, &n, &t)) COL_BAD_RECORD;
    for (int32_t i = 0; i < Q.n; ++i)
      if (Q.f[i].is_info && Q.f[i].key == key) { E[i].off = rb + at; E[i].len = n; E[i].type = (uint8_t)t; E[i].present = 1; }
    at += n * bcf_width(t);
  }
  if (at != sh_end) COL_BAD_RECORD;
  uint64_t bytes = sh_end;
  // FORMAT: (key, type, n_sample x L values) blocks
  for (uint32_t k = 0; k < n_fmt; ++k) {
    int32_t key;
    if (bcf_typed_int(p, &at, end, &key)) COL_BAD_RECORD;
    if (bcf_desc(p, &at, end, &n, &t)) COL_BAD_RECORD;
    const uint64_t block = (uint64_t)n * bcf_width(t) * n_sample;
    if (block > (uint64_t)(end - at)) COL_BAD_RECORD;
    for (int32_t i = 0; i < Q.n; ++i)
      if (!Q.f[i].is_info && Q.f[i].key == key) { E[i].off = rb + at; E[i].len = n; E[i].type = (uint8_t)t; E[i].present = 1; bytes += block; }
    at += (uint32_t)block;
  }
  if (at != end) COL_BAD_RECORD;
#undef COL_BAD_RECORD
  *alleles_len = (int64_t)joined;
  *requested_bytes = bytes;
  for (int32_t i = 0; i < Q.n; ++i) {
    ColEntry& e = E[i];
    if (e.present && (e.len == 0u || e.type == BCF_T_NULL)) e.present = 0;      // a key without values: the field is not there
    if (e.present && (Q.f[i].is_float ? e.type != BCF_T_FLOAT : !bcf_is_int(e.type))) { fault.mask[COL_ERR_TYPE] |= 1u << i; e.present = 0; }
    const uint32_t len = e.present ? e.len : 1u;
    if (Q.f[i].width > 0 && len > (uint32_t)Q.f[i].width) fault.mask[COL_ERR_WIDTH] |= 1u << i;
    col_max_u32(&max_len[i], len);
  }
  return fault;
}

// ---- site: one record (that col_measure found whole) -----------------------------------------------------------------------------
struct ColSiteOut {
  int32_t* contig; int64_t* pos; int64_t* end; int64_t* column; uint32_t* qual; int32_t* n_allele;
  uint8_t* alleles; const int64_t* alleles_off;      // alleles_off[r] .. alleles_off[r + 1]: REF and the ALTs of record r joined by ','
};
GDB_HD void col_site(const uint8_t* page, uint64_t rb, const ColRecord& R, const int64_t* contig_off, int64_t r, const ColSiteOut& O) {
  const uint8_t* p = page + rb;
  const int32_t rid = (int32_t)bcf_u32(p, 8), pos0 = (int32_t)bcf_u32(p, 12), rlen = (int32_t)bcf_u32(p, 16);
  O.contig[r] = rid;
  O.pos[r] = (int64_t)pos0 + 1;
  O.end[r] = (int64_t)pos0 + (int64_t)rlen;      // pos + rlen - 1, pos 1-based
  O.column[r] = contig_off[rid] + (int64_t)pos0;
  O.qual[r] = bcf_u32(p, 20);
  O.n_allele[r] = (int32_t)R.n_allele;
  uint8_t* out = O.alleles + O.alleles_off[r];
  const uint32_t sh_end = 8u + bcf_u32(p, 0);
  uint32_t at = R.alleles_at, n, t;
  for (uint32_t k = 0; k < R.n_allele; ++k) {
    if (bcf_desc(p, &at, sh_end, &n, &t)) return;      // (cannot happen: walked by col_measure)
    if (k) *out++ = (uint8_t)',';
    for (uint32_t i = 0; i < n; ++i) *out++ = p[at + i];
    at += n;
  }
}

// ---- scatter: one (record, sample, field) ------------------------------------------------------------------------------------------
// out: the W elements of out[r, s, :] (INFO: s = 0, out[r, :]); phase: the same of GT_phase (GT only)
GDB_HD ColFault col_scatter(const ColField& q, int field, const ColEntry& e, const uint8_t* page, uint64_t s, uint32_t W, void* out, uint8_t* phase) {
  ColFault fault; fault.mask[0] = fault.mask[1] = fault.mask[2] = fault.mask[3] = 0u;
  const int32_t d = q.dtype, missing = col_missing(d), vend = col_vector_end(d);
  if (!e.present) {
    for (uint32_t i = 0; i < W; ++i) { col_store(out, d, i, i == 0u ? (q.is_gt ? -1 : missing) : vend); if (q.is_gt) phase[i] = 0; }
    return fault;
  }
  const uint32_t t = e.type, w = bcf_width(t), L = e.len;
  const uint8_t* src = page + e.off + s * (uint64_t)L * w;
  for (uint32_t i = 0; i < W; ++i) {
    // what the element is is decided by the SOURCE type's sentinels; a real value that happens to equal a sentinel of the output dtype is out of range
    int32_t v = 0;
    uint8_t ph = 0;
    bool is_end = true, is_missing = false;
    if (i < L) {
      if (q.is_float) {
        v = (int32_t)bcf_u32(src, 4u * i);      // the bit pattern is kept, sentinels included
        is_end = (uint32_t)v == kBcfFloatVectorEndBits; is_missing = (uint32_t)v == kBcfFloatMissingBits;
      } else {
        const int32_t x = bcf_int(src, i * w, t);
        is_end = bcf_int_vector_end(x, t);
        is_missing = !is_end && (bcf_int_missing(x, t) || (q.is_gt && (x == 0 || x == 1)));
        if (!is_end && !is_missing && !col_fits(x, (int32_t)t)) { fault.mask[COL_ERR_RANGE] |= 1u << field; is_missing = true; }      // one of the source type's other reserved codes
        if (!is_end && !is_missing) {
          if (q.is_gt) {
            if (x < 0) { fault.mask[COL_ERR_RANGE] |= 1u << field; is_missing = true; }
            else { v = (x >> 1) - 1; ph = (uint8_t)(x & 1); }
          } else v = x;
          if (!is_missing && !col_fits(v, d)) { fault.mask[COL_ERR_RANGE] |= 1u << field; is_missing = true; }
        }
      }
    }
    if (i == 0u && is_end) { is_end = false; is_missing = true; }      // a vector that ends before its first element prints as '.': the sample has no value
    if (is_end) v = vend;
    else if (is_missing) v = q.is_gt ? -1 : missing;
    col_store(out, d, i, v);
    if (q.is_gt) phase[i] = ph;
  }
  return fault;
}

// ---- host side: the error words as the exception text -------------------------------------------------------------------------------
// The smallest offending record speaks (of several kinds at that record: the first in ColErrKind order).  -> false: no fault
inline bool col_first_fault(const uint32_t* err, uint32_t* record, int* kind, int* field) {
  if (!err[0]) return false;
  uint32_t at = 0xFFFFFFFFu; int bk = -1, bf = -1;
  for (int k = 0; k < kColErrKinds; ++k)
    for (int f = 0; f < kColMaxFields; ++f) {
      const uint32_t r = err[1 + k * kColMaxFields + f];
      if (r < at) { at = r; bk = k; bf = f; }
    }
  *record = at; *kind = bk; *field = bf;
  return bk >= 0;
}
inline std::string col_fault_text(int kind, const std::string& field, int32_t dtype, int32_t width, int64_t pos, uint32_t record) {
  const std::string where = " (record " + std::to_string(record) + " of the page, pos " + std::to_string(pos) + ")";
  const char* dn = dtype == COL_INT8 ? "int8" : dtype == COL_INT16 ? "int16" : dtype == COL_FLOAT32 ? "float32" : "int32";
  switch (kind) {
    case COL_ERR_RECORD: return "record columns: a record of the page is no whole BCF2 record" + where;
    case COL_ERR_TYPE: return "record columns: field " + field + " holds values of another type than its header line declares" + where;
    case COL_ERR_WIDTH: return "record columns: field " + field + " has a vector longer than the width " + std::to_string(width) + " asked for; nothing is truncated" + where;
    default: return "record columns: field " + field + " has an integer that does not fit " + dn + where;
  }
}

}  // namespace gdbcol
}  // namespace genomicsdb_amd
