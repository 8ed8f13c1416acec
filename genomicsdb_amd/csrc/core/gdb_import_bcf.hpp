// gdb_import_bcf.hpp - bodies of the device importer for BCF2 input: one BCF2 record + one sample -> one begin-cell, the bytes
// core/gdb_import.hpp (and so host/vcf_importer.cc) makes of the same record written as VCF text.  Plain functions that compile
// under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_import.hip and the CPU harness tests/hostsim_import_bcf/ run the same
// code.  No allocation, no std::string.
//
// A record is [l_shared u32][l_indiv u32][shared block][individual block] (VCFv4.2/BCFv2.2 specification, section 6).  An index
// pass (imp_bcf_index, once per record) walks both blocks, checks every length against the end of its block and leaves an
// ImpBcfRec (coordinates, offsets of ID / REF / ALT / FILTER) and one ImpBcfField per vid attribute (offset, type, count), so the
// measure and write passes (imp_bcf_body<W> over the ImpSink<W> of the text path) find the FORMAT slice of a sample in O(1) and
// never walk a multi-sample record per sample.  There is no decimal text, so nothing is deferred to the host.
//
// Every read is inside [record begin, record end): offsets come from imp_bcf_index, which refuses (error bit) a descriptor with
// an unknown type code, a vector that runs past its block, a dictionary or contig id outside the header's tables and an n_sample
// other than the header's; a record with an error bit is never measured or written.
#pragma once
#include "gdb_import.hpp"

namespace genomicsdb_amd {
namespace gdbimp {

enum ImpBcfErr : uint32_t {        // continue ImpErr
  IMP_ERR_BCF_TYPE_CODE = 64u,     // a typed descriptor with an unknown type code, or a type its place does not allow
  IMP_ERR_BCF_BOUNDS = 128u,       // a vector or a block that runs past the end of its block / record
  IMP_ERR_BCF_DICT = 256u,         // a dictionary or contig id outside the header's range
  IMP_ERR_BCF_NSAMPLE = 512u,      // n_sample differs from the header's
  IMP_ERR_BCF_FIELD_TYPE = 1024u,  // float or char values for an integer attribute, char for a numeric one, numbers for a char one
  IMP_ERR_BCF_END = 2048u          // INFO END without one integer value
};

enum { BCF_T_NULL = 0, BCF_T_INT8 = 1, BCF_T_INT16 = 2, BCF_T_INT32 = 3, BCF_T_FLOAT = 5, BCF_T_CHAR = 7 };
constexpr uint32_t kBcfFloatVectorEndBits = 0x7F800002u;
constexpr uint8_t kBcfStrMissing = 7;      // htslib's bcf_str_missing, printed as '.'

// per file: the header's dictionaries resolved against the vid (-1: not in the vid; an error only when a record uses it)
struct ImpBcfTables {
  const int32_t* dict_info;      // dictionary id -> index of the INFO attribute
  const int32_t* dict_fmt;       // dictionary id -> index of the FORMAT attribute
  const int32_t* dict_filter;    // dictionary id -> vid field index
  const int64_t* contig_off;     // contig id -> column offset
  int32_t n_dict, n_contig;
  int32_t end_key;               // dictionary id of END (-1: none)
  int32_t n_samples;             // samples of the header
};

struct ImpBcfField { uint32_t off, count; uint8_t type, present, pad[2]; };   // off: of the values in the batch (FORMAT: sample 0's); count: elements (per sample)
struct ImpBcfRec {
  int64_t col, end;
  uint32_t err;
  uint32_t qual;
  uint32_t id_off, id_len, ref_off, ref_len;
  uint32_t alt_off, alt_end, n_alt;      // the typed strings of the ALT alleles lie in [alt_off, alt_end)
  uint32_t filter_off, filter_n, filter_type;
};

GDB_HD uint32_t bcf_width(uint32_t t) { return (t == BCF_T_INT8 || t == BCF_T_CHAR) ? 1u : t == BCF_T_INT16 ? 2u : (t == BCF_T_INT32 || t == BCF_T_FLOAT) ? 4u : 0u; }
GDB_HD bool bcf_is_int(uint32_t t) { return t >= BCF_T_INT8 && t <= BCF_T_INT32; }
GDB_HD uint32_t bcf_u32(const uint8_t* p, uint32_t at) { return (uint32_t)p[at] | ((uint32_t)p[at + 1u] << 8) | ((uint32_t)p[at + 2u] << 16) | ((uint32_t)p[at + 3u] << 24); }
// an integer of type t (int8 / int16 / int32) widened
GDB_HD int32_t bcf_int(const uint8_t* p, uint32_t at, uint32_t t) {
  if (t == BCF_T_INT8) return (int32_t)(int8_t)p[at];
  if (t == BCF_T_INT16) return (int32_t)(int16_t)((uint32_t)p[at] | ((uint32_t)p[at + 1u] << 8));
  return (int32_t)bcf_u32(p, at);
}
GDB_HD bool bcf_int_missing(int32_t v, uint32_t t) { return t == BCF_T_INT8 ? v == -128 : t == BCF_T_INT16 ? v == -32768 : v == INT32_MIN; }
GDB_HD bool bcf_int_vector_end(int32_t v, uint32_t t) { return t == BCF_T_INT8 ? v == -127 : t == BCF_T_INT16 ? v == -32767 : v == INT32_MIN + 1; }
// element i of a numeric vector: is it the vector_end / the missing value of its type
GDB_HD bool bcf_elem_vector_end(const uint8_t* p, uint32_t off, uint32_t i, uint32_t t) {
  return t == BCF_T_FLOAT ? bcf_u32(p, off + 4u * i) == kBcfFloatVectorEndBits : bcf_int_vector_end(bcf_int(p, off + bcf_width(t) * i, t), t);
}
GDB_HD bool bcf_elem_missing(const uint8_t* p, uint32_t off, uint32_t i, uint32_t t) {
  return t == BCF_T_FLOAT ? bcf_u32(p, off + 4u * i) == kBcfFloatMissingBits : bcf_int_missing(bcf_int(p, off + bcf_width(t) * i, t), t);
}

// typed descriptor at *at, inside [.., end): element count and type; *at moves to the first value.  The n values of width
// bcf_width(t) are checked to lie below `end`.  Returns ImpBcfErr bits.
GDB_HD uint32_t bcf_desc(const uint8_t* p, uint32_t* at, uint32_t end, uint32_t* n, uint32_t* t) {
  if (*at >= end) return IMP_ERR_BCF_BOUNDS;
  const uint32_t b = p[(*at)++];
  *t = b & 15u; *n = b >> 4;
  if (*t != BCF_T_NULL && !bcf_is_int(*t) && *t != BCF_T_FLOAT && *t != BCF_T_CHAR) return IMP_ERR_BCF_TYPE_CODE;
  if (*n == 15u) {       // the count follows as a typed integer
    if (*at >= end) return IMP_ERR_BCF_BOUNDS;
    const uint32_t b2 = p[(*at)++], t2 = b2 & 15u;
    if ((b2 >> 4) != 1u || !bcf_is_int(t2)) return IMP_ERR_BCF_TYPE_CODE;
    const uint32_t w2 = bcf_width(t2);
    if (end - *at < w2) return IMP_ERR_BCF_BOUNDS;
    const int32_t v = bcf_int(p, *at, t2);
    *at += w2;
    if (v < 0) return IMP_ERR_BCF_BOUNDS;
    *n = (uint32_t)v;
  }
  if ((uint64_t)*n * bcf_width(*t) > (uint64_t)(end - *at)) return IMP_ERR_BCF_BOUNDS;
  return 0;
}
// one typed integer (a dictionary key)
GDB_HD uint32_t bcf_typed_int(const uint8_t* p, uint32_t* at, uint32_t end, int32_t* v) {
  uint32_t n, t;
  const uint32_t e = bcf_desc(p, at, end, &n, &t);
  if (e) return e;
  if (n != 1u || !bcf_is_int(t)) return IMP_ERR_BCF_TYPE_CODE;
  *v = bcf_int(p, *at, t);
  *at += bcf_width(t);
  return 0;
}
// length of char data up to its first NUL
GDB_HD uint32_t bcf_strlen(const uint8_t* p, uint32_t off, uint32_t n) { uint32_t m = 0; while (m < n && p[off + m] != 0) ++m; return m; }

// ---- index pass: once per record ---------------------------------------------------------------------------------------------
// p: the batch's bytes; the record is [begin, end) (the host's walk of the l_shared / l_indiv chain).  F: n_info + n_fmt entries.
GDB_HD uint32_t imp_bcf_index(const ImpTables& T, const ImpBcfTables& B, const uint8_t* p, uint32_t begin, uint32_t end, ImpBcfRec* R, ImpBcfField* F) {
  const int n_attr = T.n_info + T.n_fmt;
  for (int i = 0; i < n_attr; ++i) { F[i].off = 0; F[i].count = 0; F[i].type = 0; F[i].present = 0; F[i].pad[0] = F[i].pad[1] = 0; }
  R->col = 0; R->end = 0; R->err = 0; R->qual = 0; R->id_off = R->id_len = R->ref_off = R->ref_len = 0;
  R->alt_off = R->alt_end = R->n_alt = 0; R->filter_off = R->filter_n = R->filter_type = 0;
  if (end < begin || end - begin < 32u) return R->err = IMP_ERR_BCF_BOUNDS;
  const uint32_t l_shared = bcf_u32(p, begin), l_indiv = bcf_u32(p, begin + 4u);
  if (l_shared < 24u || (uint64_t)l_shared + (uint64_t)l_indiv + 8u != (uint64_t)(end - begin)) return R->err = IMP_ERR_BCF_BOUNDS;
  const uint32_t sh_end = begin + 8u + l_shared;
  const int32_t rid = (int32_t)bcf_u32(p, begin + 8u), pos = (int32_t)bcf_u32(p, begin + 12u);      // (rlen at + 16 is ignored)
  R->qual = bcf_u32(p, begin + 20u);
  const uint32_t n_allele_info = bcf_u32(p, begin + 24u), n_fmt_sample = bcf_u32(p, begin + 28u);
  const uint32_t n_info = n_allele_info & 0xFFFFu, n_allele = n_allele_info >> 16, n_sample = n_fmt_sample & 0xFFFFFFu, n_fmt = n_fmt_sample >> 24;
  if (n_sample != (uint32_t)B.n_samples) return R->err = IMP_ERR_BCF_NSAMPLE;
  if (rid < 0 || rid >= B.n_contig) return R->err = IMP_ERR_BCF_DICT;
  if (B.contig_off[rid] < 0) return R->err = IMP_ERR_CONTIG;
  uint32_t at = begin + 32u, n, t, e;
  // ID, REF and the ALTs: typed strings
  if ((e = bcf_desc(p, &at, sh_end, &n, &t))) return R->err = e;
  if (t != BCF_T_CHAR && n != 0u) return R->err = IMP_ERR_BCF_TYPE_CODE;
  R->id_off = at; R->id_len = n; at += n;
  if (n_allele == 0u) return R->err = IMP_ERR_BCF_BOUNDS;
  if ((e = bcf_desc(p, &at, sh_end, &n, &t))) return R->err = e;
  if (t != BCF_T_CHAR && n != 0u) return R->err = IMP_ERR_BCF_TYPE_CODE;
  R->ref_off = at; R->ref_len = n; at += n;
  R->alt_off = at; R->n_alt = n_allele - 1u;
  for (uint32_t k = 1; k < n_allele; ++k) {
    if ((e = bcf_desc(p, &at, sh_end, &n, &t))) return R->err = e;
    if (t != BCF_T_CHAR && n != 0u) return R->err = IMP_ERR_BCF_TYPE_CODE;
    at += n;
  }
  R->alt_end = at;
  // FILTER: a vector of dictionary ids
  if ((e = bcf_desc(p, &at, sh_end, &n, &t))) return R->err = e;
  if (!bcf_is_int(t) && n != 0u) return R->err = IMP_ERR_BCF_TYPE_CODE;
  R->filter_off = at; R->filter_n = n; R->filter_type = t;
  for (uint32_t k = 0; k < n; ++k) {
    const int32_t id = bcf_int(p, at + k * bcf_width(t), t);
    if (id < 0 || id >= B.n_dict) return R->err = IMP_ERR_BCF_DICT;
    if (B.dict_filter[id] < 0) return R->err = IMP_ERR_FILTER;
  }
  at += n * bcf_width(t);
  // INFO: (key, typed vector) pairs; the last pair of a key counts
  bool has_end = false;
  int32_t end_value = 0;
  for (uint32_t k = 0; k < n_info; ++k) {
    int32_t key;
    if ((e = bcf_typed_int(p, &at, sh_end, &key))) return R->err = e;
    if ((e = bcf_desc(p, &at, sh_end, &n, &t))) return R->err = e;
    if (key < 0 || key >= B.n_dict) return R->err = IMP_ERR_BCF_DICT;
    if (key == B.end_key) {
      if (!bcf_is_int(t) || n < 1u || bcf_elem_missing(p, at, 0, t) || bcf_elem_vector_end(p, at, 0, t)) return R->err = IMP_ERR_BCF_END;
      has_end = true; end_value = bcf_int(p, at, t);
    }
    const int32_t a = B.dict_info[key];
    if (a >= 0 && a < T.n_info) { F[a].off = at; F[a].count = n; F[a].type = (uint8_t)t; F[a].present = 1; }
    at += n * bcf_width(t);
  }
  if (at != sh_end) return R->err = IMP_ERR_BCF_BOUNDS;
  // FORMAT: (key, type, n_sample x count values) blocks
  for (uint32_t k = 0; k < n_fmt; ++k) {
    int32_t key;
    if ((e = bcf_typed_int(p, &at, end, &key))) return R->err = e;
    if ((e = bcf_desc(p, &at, end, &n, &t))) return R->err = e;
    if (key < 0 || key >= B.n_dict) return R->err = IMP_ERR_BCF_DICT;
    const uint64_t bytes = (uint64_t)n * bcf_width(t) * n_sample;
    if (bytes > (uint64_t)(end - at)) return R->err = IMP_ERR_BCF_BOUNDS;
    const int32_t a = B.dict_fmt[key];
    if (a >= 0 && a < T.n_fmt) { ImpBcfField& f = F[T.n_info + a]; f.off = at; f.count = n; f.type = (uint8_t)t; f.present = 1; }
    at += (uint32_t)bytes;
  }
  if (at != end) return R->err = IMP_ERR_BCF_BOUNDS;
  // coordinates: imp_coords over the binary fields (POS is 0-based here; END in INFO is 1-based as in text)
  const int64_t offset = B.contig_off[rid];
  const int64_t col = offset + (int64_t)pos;
  int64_t cend = col;
  if (has_end) cend = offset + (int64_t)end_value - 1;
  else if (T.treat_deletions_as_intervals) {
    ImpTok ref; ref.b = R->ref_off; ref.e = R->ref_off + R->ref_len;
    uint32_t a_at = R->alt_off;
    for (uint32_t k = 0; k < R->n_alt; ++k) {
      if (bcf_desc(p, &a_at, R->alt_end, &n, &t)) break;       // (cannot happen: walked above)
      ImpTok alt; alt.b = a_at; alt.e = a_at + n;
      a_at += n;
      if (imp_deletion_indel((const char*)p, ref, alt)) { cend = col + (int64_t)ref.n() - 1; break; }
    }
  }
  R->col = col; R->end = cend;
  if (col < 0 || (col >> (63 - T.key_row_bits)) != 0) return R->err = IMP_ERR_COORD_RANGE;
  return 0;
}

// ---- attributes ------------------------------------------------------------------------------------------------------------
template <bool W> GDB_HD void imp_bcf_null(ImpSink<W>& o, const ImpAttr& a) {      // what imp_values writes for a missing numeric attribute
  if (a.fixed) for (uint32_t i = 0; i < a.num_elements; ++i) { if (a.elem == GDB_ET_INT) o.i32(kNullInt); else o.u32(kNullFloatBits); }
  else o.i32(0);
}

// imp_values for one typed vector: count elements of `type` at off.  "Missing" is the text rule `!present || value == "."`: an
// absent key, no values, or one element that is the type's missing value (char data: empty or "." once cut at its first NUL)
template <bool W>
GDB_HD void imp_bcf_values(ImpSink<W>& o, const ImpAttr& a, const uint8_t* p, uint32_t off, uint32_t count, uint32_t type, bool present, bool info, int n_samples,
                           int sample_idx) {
  if (a.elem == GDB_ET_FLAG) { o.u8(present ? (uint8_t)1 : kNullChar); return; }
  const bool rec_char = type == BCF_T_CHAR;
  uint32_t m = 0;       // elements up to the first vector_end / chars up to the first NUL
  bool missing = true;
  if (present && type != BCF_T_NULL) {
    if (rec_char) { m = bcf_strlen(p, off, count); missing = m == 0u || (m == 1u && (p[off] == (uint8_t)'.' || p[off] == kBcfStrMissing)); }
    else { while (m < count && !bcf_elem_vector_end(p, off, m, type)) ++m; missing = m == 0u || (m == 1u && bcf_elem_missing(p, off, 0, type)); }
  }
  if (a.elem == GDB_ET_CHAR) {
    if (missing) { o.i32(0); return; }
    if (!rec_char) { o.err |= IMP_ERR_BCF_FIELD_TYPE; o.i32(0); return; }
    o.i32((int32_t)m);
    for (uint32_t i = 0; i < m; ++i) o.u8(p[off + i] == kBcfStrMissing ? (uint8_t)'.' : p[off + i]);
    return;
  }
  const bool is_int = a.elem == GDB_ET_INT;
  if (missing) { imp_bcf_null<W>(o, a); return; }
  if (rec_char || (is_int && type == BCF_T_FLOAT)) { o.err |= IMP_ERR_BCF_FIELD_TYPE; imp_bcf_null<W>(o, a); return; }
  if (a.fixed && m != a.num_elements) {       // an error; both passes still agree on the size
    o.err |= IMP_ERR_COUNT;
    for (uint32_t i = 0; i < a.num_elements; ++i) o.i32(kNullInt);
    return;
  }
  if (!a.fixed) o.i32((int32_t)m);
  if (!W) { o.n += 4ull * m; return; }
  const bool divide = a.sum_like && info && n_samples > 1;
  for (uint32_t i = 0; i < m; ++i) {
    if (type == BCF_T_FLOAT) {
      const uint32_t bits = bcf_u32(p, off + 4u * i);
      if (bits == kBcfFloatMissingBits || !divide) { o.u32(bits); continue; }      // every float keeps its bits
      union { float f; uint32_t u; } x; x.u = bits;
      o.f32(x.f / (float)n_samples);
      continue;
    }
    const int32_t v = bcf_int(p, off + bcf_width(type) * i, type);
    if (bcf_int_missing(v, type)) { if (is_int) o.i32(kBcfIntMissing); else o.u32(kBcfFloatMissingBits); continue; }
    if (is_int) o.i32(divide ? (int32_t)imp_divide_among_samples((int64_t)v, n_samples, sample_idx) : v);
    else { float f = (float)v; if (divide) f = f / (float)n_samples; o.f32(f); }      // what (float)strtod makes of the same digits
  }
}

// imp_gt: allele = (v >> 1) - 1, phase flag in front of allele i = v_i & 1; vector_end padding of a lower ploidy is cut
template <bool W>
GDB_HD void imp_bcf_gt(ImpSink<W>& o, const ImpAttr& a, const uint8_t* p, uint32_t off, uint32_t count, uint32_t type, bool present) {
  uint32_t m = 0;
  if (present && type != BCF_T_NULL) {
    if (!bcf_is_int(type)) { o.err |= IMP_ERR_BCF_FIELD_TYPE; present = false; }
    else while (m < count && !bcf_elem_vector_end(p, off, m, type)) ++m;
  }
  if (!present || m == 0u) { o.i32(1); o.i32(-1); return; }
  o.i32((int32_t)(a.pp ? 2u * m - 1u : m));
  for (uint32_t i = 0; i < m; ++i) {
    const int32_t v = bcf_int(p, off + bcf_width(type) * i, type);
    if (a.pp && i) o.i32(v & 1);
    o.i32((v >> 1) - 1);
  }
}

// everything of a cell after [row][col][cell_size], as imp_body.  sample = index in the file
template <bool W>
GDB_HD void imp_bcf_body(const ImpTables& T, const ImpBcfTables& B, const uint8_t* p, const ImpBcfRec& R, const ImpBcfField* F, int sample, ImpSink<W>& o) {
  o.i64(R.end);
  o.i32((int32_t)R.ref_len);
  for (uint32_t i = 0; i < R.ref_len; ++i) o.u8(p[R.ref_off + i]);
  // ALT: alleles joined by '|', <NON_REF> as '&'
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t at = R.alt_off, len = 0, n, t;
    for (uint32_t k = 0; k < R.n_alt; ++k) {
      if (bcf_desc(p, &at, R.alt_end, &n, &t)) break;       // (cannot happen: walked by imp_bcf_index)
      ImpTok a; a.b = at; a.e = at + n;
      at += n;
      const bool non_ref = imp_tok_eq((const char*)p, a, "<NON_REF>", 9u);
      if (pass == 0) { len += (k ? 1u : 0u) + (non_ref ? 1u : n); continue; }
      if (k) o.u8((uint8_t)'|');
      if (non_ref) o.u8((uint8_t)'&');
      else for (uint32_t i = a.b; i < a.e; ++i) o.u8(p[i]);
    }
    if (pass == 0) o.i32((int32_t)len);
  }
  if (T.has_id) {
    const uint32_t n = bcf_strlen(p, R.id_off, R.id_len);
    if (n == 0u || (n == 1u && p[R.id_off] == (uint8_t)'.')) o.i32(0);
    else { o.i32((int32_t)n); for (uint32_t i = 0; i < n; ++i) o.u8(p[R.id_off + i]); }
  }
  o.u32(R.qual == kBcfFloatMissingBits ? kNullFloatBits : R.qual);
  o.i32((int32_t)R.filter_n);
  for (uint32_t k = 0; k < R.filter_n; ++k) {
    const int32_t id = bcf_int(p, R.filter_off + k * bcf_width(R.filter_type), R.filter_type);
    o.i32(id >= 0 && id < B.n_dict ? B.dict_filter[id] : -1);
  }
  for (int i = 0; i < T.n_info; ++i) {
    const ImpBcfField& f = F[i];
    imp_bcf_values<W>(o, T.info[i], p, f.off, f.count, f.type, f.present != 0, true, T.n_samples, sample);
  }
  for (int i = 0; i < T.n_fmt; ++i) {
    const ImpBcfField& f = F[T.n_info + i];
    const uint32_t off = f.off + (uint32_t)sample * f.count * bcf_width(f.type);      // the sample's slice (sample < n_sample, checked by the index pass)
    if (T.fmt[i].gt) imp_bcf_gt<W>(o, T.fmt[i], p, off, f.count, f.type, f.present != 0);
    else imp_bcf_values<W>(o, T.fmt[i], p, off, f.count, f.type, f.present != 0, false, 1, 0);
  }
}

// measure pass of one (record, imported sample), as imp_measure
GDB_HD ImpSlot imp_bcf_measure(const ImpTables& T, const ImpBcfTables& B, const uint8_t* p, const ImpBcfRec& R, const ImpBcfField* F, int sample) {
  ImpSlot s; s.col = R.col; s.end = R.end; s.size = 0; s.kind = IMP_SLOT_NONE; s.err = R.err;
  if (s.err || sample < 0 || sample >= B.n_samples || s.col > T.column_end) return s;
  if (s.col < T.column_begin) {
    if (s.end < T.column_begin) return s;
    s.kind = IMP_SLOT_SPANNING_CANDIDATE;
  } else s.kind = IMP_SLOT_CELL;
  ImpSink<false> o;
  imp_bcf_body<false>(T, B, p, R, F, sample, o);
  s.err |= o.err;
  s.size = 24u + o.n;
  return s;
}

// write pass, as imp_write
GDB_HD uint32_t imp_bcf_write(const ImpTables& T, const ImpBcfTables& B, const uint8_t* p, const ImpBcfRec& R, const ImpBcfField* F, int sample, int64_t row,
                              const ImpSlot& s, ImpSink<true>& o) {
  o.limit = s.size;
  o.i64(row); o.i64(s.col); o.i64((int64_t)s.size);
  imp_bcf_body<true>(T, B, p, R, F, sample, o);
  return o.err;
}

}  // namespace gdbimp
}  // namespace genomicsdb_amd
