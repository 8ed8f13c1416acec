// gdb_import.hpp - bodies of the device importer: one (g)VCF record line + one sample -> one begin-cell, byte for byte what
// host/vcf_importer.cc (import_callsets_to_cells) makes of it.  Plain functions that compile under g++ and hipcc (GDB_HD): the
// kernels of kernels/gdb_import.hip and the CPU harness tests/hostsim_import/ run the same code.  No allocation, no std::string.
//
// A record line is given as its text range plus the offsets of its tabs (ImpLine), so column k is found in O(1) and a
// multi-sample line is not rescanned per sample.  A cell is produced by one template (imp_body<W>) in two passes: W = false
// measures (the size of a cell never depends on a value), W = true writes the bytes.
//
// Numbers keep the bits of the host's parse_int / (float)parse_double:
//   integers  [+-]?[0-9]+ that fit in 64 bits are parsed here;
//   floats    [+-]?(digits[.digits]|.digits)([eE][+-]?digits)? whose digit string - leading and trailing zeros stripped - has at
//             most 15 digits and whose decimal exponent over that digit string read as an integer is within +-22: the digits are
//             an exact double, one multiplication or division by an exact power of ten is correctly rounded, and the cast to
//             float is the same second rounding as (float)strtod;
//   every other numeric token is DEFERRED: 4 placeholder bytes are written and an ImpDeferred entry names the token and the
//   bytes; the host parses exactly those tokens with the host importer's own functions.
#pragma once
#include <cstdint>

#include "gdb_types.h"

namespace genomicsdb_amd {
namespace gdbimp {

constexpr int32_t kNullInt = INT32_MAX;             // TileDB null (fixed-length field without a value)
constexpr uint32_t kNullFloatBits = 0x7F7FFFFFu;    // FLT_MAX
constexpr uint8_t kNullChar = 127;
constexpr int32_t kBcfIntMissing = INT32_MIN;       // a '.' element of a vector
constexpr uint32_t kBcfFloatMissingBits = 0x7F800001u;

enum ImpErr : uint32_t {
  IMP_ERR_SHORT_LINE = 1u, IMP_ERR_CONTIG = 2u, IMP_ERR_FILTER = 4u, IMP_ERR_COUNT = 8u,
  IMP_ERR_COORD_TEXT = 16u,     // POS / END outside the integer fast path: coordinates decide sizes and order, they are not deferred
  IMP_ERR_COORD_RANGE = 32u     // a column that the 64-bit (column, row) sort key cannot hold
  // 64 .. 2048: ImpBcfErr (gdb_import_bcf.hpp); 4096 .. 65536: ImpCsvErr (gdb_import_csv.hpp)
};

struct ImpName { uint32_t off, len; int64_t value; };      // contig: value = column offset; field: value = field index
struct ImpAttr {
  uint32_t name_off, name_len, num_elements;
  uint8_t elem, fixed, sum_like, gt, pp, pad[3];
};
struct ImpTables {
  const char* names;                 // blob all name offsets point into
  const ImpName* contigs; const ImpName* fields; const ImpAttr* info; const ImpAttr* fmt;
  int32_t n_contigs, n_fields, n_info, n_fmt;
  int32_t has_id, treat_deletions_as_intervals;
  int32_t n_samples;                 // samples of the file (INFO sums are divided among all of them)
  int32_t key_row_bits;              // sort key = column << key_row_bits | row
  int64_t column_begin, column_end;
};
struct ImpLine { const char* text; uint32_t begin, end; const uint32_t* tabs; uint32_t ntabs; };   // end: '\r' already cut
struct ImpTok { uint32_t b, e; GDB_HD uint32_t n() const { return e - b; } };

enum { IMP_KIND_INT = 0, IMP_KIND_FLOAT = 1, IMP_KIND_CSV_INT = 2, IMP_KIND_CSV_FLOAT = 3 };   // CSV: strtoll(base 0) / strtof over a prefix
enum { IMP_WHAT_QUAL = -1, IMP_WHAT_GT = -2, IMP_WHAT_FILTER = -3, IMP_WHAT_FMT_BASE = 1 << 16 };   // else: index of the INFO attribute
struct ImpDeferred {
  uint32_t tok_off, tok_len;         // the token's text (offset in the batch)
  uint64_t out_off;                  // its 4 output bytes (offset in the batch's cell buffer)
  uint32_t line;                     // record line in the batch
  int32_t what;                      // IMP_WHAT_*
  uint16_t kind, sample_idx;         // sample_idx: the sample's index in the file, for the division among samples
  uint32_t divide;                   // number of samples to divide among, 0: none
};

GDB_HD uint32_t imp_atomic_inc(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicAdd(p, 1u);
#else
  return (*p)++;
#endif
}

// ---- tokens ----------------------------------------------------------------------------------------------------------------
GDB_HD uint32_t imp_num_columns(const ImpLine& L) { return L.ntabs + 1u; }
GDB_HD ImpTok imp_column(const ImpLine& L, uint32_t k) {
  ImpTok t;
  t.b = k == 0 ? L.begin : L.tabs[k - 1] + 1u;
  t.e = k < L.ntabs ? L.tabs[k] : L.end;
  return t;
}
GDB_HD bool imp_tok_eq(const char* text, ImpTok t, const char* s, uint32_t n) {
  if (t.n() != n) return false;
  for (uint32_t i = 0; i < n; ++i) if (text[t.b + i] != s[i]) return false;
  return true;
}
GDB_HD bool imp_is_dot(const char* text, ImpTok t) { return t.n() == 1u && text[t.b] == '.'; }
// next piece of [*at, e) up to sep; false when nothing is left.  An empty range yields one empty piece, like the host's split()
GDB_HD bool imp_next(const char* text, uint32_t* at, uint32_t e, char sep, ImpTok* out) {
  if (*at > e) return false;
  uint32_t i = *at;
  while (i < e && text[i] != sep) ++i;
  out->b = *at; out->e = i;
  *at = i + 1u;
  return true;
}
GDB_HD uint32_t imp_count_pieces(const char* text, ImpTok t, char sep) {
  uint32_t n = 1;
  for (uint32_t i = t.b; i < t.e; ++i) n += text[i] == sep;
  return n;
}

// ---- numbers ---------------------------------------------------------------------------------------------------------------
GDB_HD bool imp_parse_int(const char* p, uint32_t n, int64_t* out) {
  uint32_t i = 0;
  bool neg = false;
  if (n && (p[0] == '+' || p[0] == '-')) { neg = p[0] == '-'; i = 1; }
  if (i >= n) return false;
  const uint64_t limit = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1u;
  uint64_t w = 0;
  for (; i < n; ++i) {
    const uint32_t d = (uint32_t)(uint8_t)p[i] - (uint32_t)'0';
    if (d > 9u) return false;
    if (w > (limit - d) / 10u) return false;       // does not fit: strtoll would saturate, leave that to the host
    w = w * 10u + d;
  }
  *out = neg ? (int64_t)(0u - w) : (int64_t)w;
  return true;
}

GDB_HD double imp_pow10(int e) {   // 10^e, 0 <= e <= 22: exactly representable
  switch (e) {
    case 0: return 1e0; case 1: return 1e1; case 2: return 1e2; case 3: return 1e3; case 4: return 1e4; case 5: return 1e5;
    case 6: return 1e6; case 7: return 1e7; case 8: return 1e8; case 9: return 1e9; case 10: return 1e10; case 11: return 1e11;
    case 12: return 1e12; case 13: return 1e13; case 14: return 1e14; case 15: return 1e15; case 16: return 1e16; case 17: return 1e17;
    case 18: return 1e18; case 19: return 1e19; case 20: return 1e20; case 21: return 1e21; default: return 1e22;
  }
}

// the value as a double: the digits times an exact power of ten, one correctly rounded operation
GDB_HD bool imp_parse_decimal(const char* p, uint32_t n, double* out) {
  uint32_t i = 0;
  bool neg = false;
  if (n && (p[0] == '+' || p[0] == '-')) { neg = p[0] == '-'; i = 1; }
  uint64_t w = 0;              // the significant digits up to the last non-zero one
  int nd = 0;                  // how many
  int fd = 0, w_fd = 0;        // fraction digits seen / of them inside w
  int pend_int = 0, pend = 0;  // zeros after w's last digit: of the integer part / all
  bool any = false, frac = false;
  for (; i < n; ++i) {
    const char c = p[i];
    if (c == '.') { if (frac) return false; frac = true; continue; }
    const uint32_t d = (uint32_t)(uint8_t)c - (uint32_t)'0';
    if (d > 9u) break;
    any = true;
    if (frac) ++fd;
    if (d == 0u) { if (w) { ++pend; if (!frac) ++pend_int; } continue; }
    nd += pend + 1;
    if (nd > 15) return false;
    for (int k = 0; k < pend; ++k) w *= 10u;
    w = w * 10u + d;
    pend = 0; pend_int = 0; w_fd = fd;
  }
  if (!any) return false;
  int ex = 0;
  if (i < n) {
    if (p[i] != 'e' && p[i] != 'E') return false;
    ++i;
    bool eneg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; ++i; }
    if (i >= n) return false;
    for (; i < n; ++i) {
      const uint32_t d = (uint32_t)(uint8_t)p[i] - (uint32_t)'0';
      if (d > 9u) return false;
      if (ex < 100000) ex = ex * 10 + (int)d;
    }
    if (eneg) ex = -ex;
  }
  double v;
  if (w == 0u) v = 0.0;
  else {
    const int e10 = ex - w_fd + pend_int;
    if (e10 < -22 || e10 > 22) return false;
    v = (double)w;
    v = e10 < 0 ? v / imp_pow10(-e10) : v * imp_pow10(e10);
  }
  *out = neg ? -v : v;
  return true;
}
GDB_HD bool imp_parse_float(const char* p, uint32_t n, float* out) {
  double v;
  if (!imp_parse_decimal(p, n, &v)) return false;
  *out = (float)v;
  return true;
}

GDB_HD int64_t imp_divide_among_samples(int64_t v, int n_samples, int sample_idx) {   // floor division, remainder to the first samples
  int64_t q = v / n_samples, r = v % n_samples;
  if (r < 0) { r += n_samples; --q; }
  return q + (sample_idx < r ? 1 : 0);
}

// ---- sink ------------------------------------------------------------------------------------------------------------------
template <bool W> struct ImpSink {
  uint8_t* out = nullptr;       // the cell's first byte
  uint64_t n = 0, limit = 0;    // bytes so far / the measured size (W only: nothing is stored at or beyond it)
  uint64_t base = 0;            // offset of `out` in the batch's cell buffer, for the deferred list
  ImpDeferred* def = nullptr; uint32_t* ndef = nullptr; uint32_t def_cap = 0;
  uint32_t line = 0, err = 0;
  GDB_HD void u8(uint8_t b) { if (W) { if (n < limit) out[n] = b; } ++n; }
  GDB_HD void u32(uint32_t v) { if (W) { for (int i = 0; i < 4; ++i) { if (n + i < limit) out[n + i] = (uint8_t)(v >> (8 * i)); } } n += 4; }
  GDB_HD void i32(int32_t v) { u32((uint32_t)v); }
  GDB_HD void i64(int64_t v) { u32((uint32_t)(uint64_t)v); u32((uint32_t)((uint64_t)v >> 32)); }
  GDB_HD void f32(float f) { union { float f; uint32_t u; } x; x.f = f; u32(x.u); }
  GDB_HD void chars(const char* text, ImpTok t) { i32((int32_t)t.n()); if (W) { for (uint32_t i = t.b; i < t.e; ++i) { if (n + (i - t.b) < limit) out[n + (i - t.b)] = (uint8_t)text[i]; } } n += t.n(); }
  GDB_HD void defer(ImpTok t, int what, int kind, uint32_t divide, int sample_idx) {   // the next 4 bytes belong to token t
    if (W) {
      const uint32_t at = imp_atomic_inc(ndef);
      if (at < def_cap) {
        ImpDeferred d;
        d.tok_off = t.b; d.tok_len = t.n(); d.out_off = base + n; d.line = line; d.what = what; d.kind = (uint16_t)kind;
        d.sample_idx = (uint16_t)sample_idx; d.divide = divide;
        def[at] = d;
      }
    }
    u32(0u);
  }
};

// ---- coordinates -----------------------------------------------------------------------------------------------------------
// the last `key[=value]` of INFO counts; value empty for a key without '='
GDB_HD bool imp_info_find(const char* text, ImpTok info, const char* key, uint32_t kn, ImpTok* val) {
  if (imp_is_dot(text, info)) return false;
  bool found = false;
  uint32_t at = info.b;
  ImpTok kv;
  while (imp_next(text, &at, info.e, ';', &kv)) {
    uint32_t eq = kv.b;
    while (eq < kv.e && text[eq] != '=') ++eq;
    ImpTok k; k.b = kv.b; k.e = eq;
    if (!imp_tok_eq(text, k, key, kn)) continue;
    found = true;
    if (eq < kv.e) { val->b = eq + 1u; val->e = kv.e; } else { val->b = kv.e; val->e = kv.e; }
  }
  return found;
}

GDB_HD char imp_upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - 'a' + 'A') : c; }
// the host importer's deletion_indel (htslib's variant type INDEL with REF longer than ALT), case-insensitive
GDB_HD bool imp_deletion_indel(const char* text, ImpTok ref, ImpTok alt) {
  const uint32_t rn = ref.n(), an = alt.n();
  const char* rp = text + ref.b;
  const char* ap = text + alt.b;
  if (an == 0u || ap[0] == '<' || (an == 1u && (ap[0] == '*' || ap[0] == '.'))) return false;
  if (rn == 1u && an == 1u) return false;
  uint32_t r = 0, a = 0;
  while (r < rn && a < an && imp_upper(rp[r]) == imp_upper(ap[a])) { ++r; ++a; }
  if (a < an && r == rn) return false;
  if (r < rn && a == an) return true;
  if (r == rn && a == an) return false;
  uint32_t re = rn - 1u, ae = an - 1u;
  while (re > r && ae > a && imp_upper(rp[re]) == imp_upper(ap[ae])) { --re; --ae; }
  if (ae == a) { if (re == r) return false; return imp_upper(rp[re]) == imp_upper(ap[ae]) && rn > an; }
  if (re == r) return imp_upper(rp[re]) == imp_upper(ap[ae]) && rn > an;
  return false;
}

// CHROM, POS and INFO END of a record line - the parse that the importer (imp_coords) and the splitter (core/gdb_split.hpp) share.
// col = contig offset + POS - 1; *has_end: INFO carries END (the last one counts), then *end = contig offset + END - 1, else *end = col.
// Returns IMP_ERR_SHORT_LINE, IMP_ERR_CONTIG or IMP_ERR_COORD_TEXT (0: fine)
GDB_HD uint32_t imp_coords_text(const ImpTables& T, const ImpLine& L, int64_t* col_out, int64_t* end_out, bool* has_end) {
  if (imp_num_columns(L) < 8u) return IMP_ERR_SHORT_LINE;
  const char* text = L.text;
  const ImpTok chrom = imp_column(L, 0);
  int ci = -1;
  for (int i = 0; i < T.n_contigs && ci < 0; ++i)
    if (imp_tok_eq(text, chrom, T.names + T.contigs[i].off, T.contigs[i].len)) ci = i;
  if (ci < 0) return IMP_ERR_CONTIG;
  const int64_t offset = T.contigs[ci].value;
  const ImpTok pos = imp_column(L, 1);
  int64_t v;
  if (!imp_parse_int(text + pos.b, pos.n(), &v)) return IMP_ERR_COORD_TEXT;
  const int64_t col = offset + v - 1;
  int64_t end = col;
  ImpTok endv;
  *has_end = imp_info_find(text, imp_column(L, 7), "END", 3u, &endv);
  if (*has_end) {
    if (!imp_parse_int(text + endv.b, endv.n(), &v)) return IMP_ERR_COORD_TEXT;
    end = offset + v - 1;
  }
  *col_out = col;
  *end_out = end;
  return 0;
}

// column and END of a record line; returns ImpErr bits (0: fine)
GDB_HD uint32_t imp_coords(const ImpTables& T, const ImpLine& L, int64_t* col_out, int64_t* end_out) {
  int64_t col = 0, end = 0;
  bool has_end = false;
  const uint32_t e = imp_coords_text(T, L, &col, &end, &has_end);
  if (e) return e;
  const char* text = L.text;
  if (!has_end && T.treat_deletions_as_intervals) {
    const ImpTok ref = imp_column(L, 3), alt = imp_column(L, 4);
    if (!imp_is_dot(text, alt)) {
      uint32_t at = alt.b;
      ImpTok a;
      while (imp_next(text, &at, alt.e, ',', &a))
        if (imp_deletion_indel(text, ref, a)) { end = col + (int64_t)ref.n() - 1; break; }
    }
  }
  *col_out = col;
  *end_out = end;
  if (col < 0 || (col >> (63 - T.key_row_bits)) != 0) return IMP_ERR_COORD_RANGE;
  return 0;
}

// ---- attributes ------------------------------------------------------------------------------------------------------------
template <bool W>
GDB_HD void imp_number(ImpSink<W>& o, const char* text, ImpTok t, bool is_int, int what, int n_samples, int sample_idx, bool divide) {
  if (!W) { o.n += 4; return; }
  if (imp_is_dot(text, t)) { if (is_int) o.i32(kBcfIntMissing); else o.u32(kBcfFloatMissingBits); return; }
  if (is_int) {
    int64_t v;
    if (!imp_parse_int(text + t.b, t.n(), &v)) { o.defer(t, what, IMP_KIND_INT, divide ? (uint32_t)n_samples : 0u, sample_idx); return; }
    if (divide) v = imp_divide_among_samples(v, n_samples, sample_idx);
    o.i32((int32_t)v);
  } else {
    float f;
    if (!imp_parse_float(text + t.b, t.n(), &f)) { o.defer(t, what, IMP_KIND_FLOAT, divide ? (uint32_t)n_samples : 0u, sample_idx); return; }
    if (divide) f = f / (float)n_samples;
    o.f32(f);
  }
}

// the host importer's encode_values for 1-dimensional attributes
template <bool W>
GDB_HD void imp_values(ImpSink<W>& o, const ImpAttr& a, int what, const char* text, bool present, ImpTok v, bool info, int n_samples, int sample_idx) {
  const bool missing = !present || imp_is_dot(text, v);
  if (a.elem == GDB_ET_FLAG) { o.u8(present ? (uint8_t)1 : kNullChar); return; }
  if (a.elem == GDB_ET_CHAR) { if (missing) o.i32(0); else o.chars(text, v); return; }
  const bool is_int = a.elem == GDB_ET_INT;
  if (missing) {
    if (a.fixed) for (uint32_t i = 0; i < a.num_elements; ++i) { if (is_int) o.i32(kNullInt); else o.u32(kNullFloatBits); }
    else o.i32(0);
    return;
  }
  const uint32_t count = imp_count_pieces(text, v, ',');
  if (a.fixed && count != a.num_elements) {       // an error; both passes still agree on the size
    o.err |= IMP_ERR_COUNT;
    for (uint32_t i = 0; i < a.num_elements; ++i) o.i32(kNullInt);
    return;
  }
  if (!a.fixed) o.i32((int32_t)count);
  const bool divide = a.sum_like && info && n_samples > 1;
  uint32_t at = v.b;
  ImpTok t;
  while (imp_next(text, &at, v.e, ',', &t)) imp_number<W>(o, text, t, is_int, what, n_samples, sample_idx, divide);
}

// the host importer's encode_gt: allele indices, phase flags interleaved for the PP layout
template <bool W>
GDB_HD void imp_gt(ImpSink<W>& o, const ImpAttr& a, const char* text, bool present, ImpTok v) {
  if (!present || imp_is_dot(text, v)) { o.i32(1); o.i32(-1); return; }
  uint32_t n_alleles = 1;
  for (uint32_t i = v.b; i < v.e; ++i) n_alleles += text[i] == '/' || text[i] == '|';
  o.i32((int32_t)(a.pp ? 2u * n_alleles - 1u : n_alleles));
  uint32_t b = v.b;
  for (uint32_t i = v.b; i <= v.e; ++i) {
    if (i != v.e && text[i] != '/' && text[i] != '|') continue;
    if (a.pp && b != v.b) o.i32(text[b - 1u] == '|' ? 1 : 0);
    ImpTok t; t.b = b; t.e = i;
    if (imp_is_dot(text, t)) o.i32(-1);
    else imp_number<W>(o, text, t, true, IMP_WHAT_GT, 1, 0, false);
    b = i + 1u;
  }
}

// everything of a cell after [row][col][cell_size]: END, REF, ALT, [ID], QUAL, FILTER, INFO.., FORMAT..  sample = index in the file
template <bool W>
GDB_HD void imp_body(const ImpTables& T, const ImpLine& L, int sample, int64_t end, ImpSink<W>& o) {
  const char* text = L.text;
  o.i64(end);
  o.chars(text, imp_column(L, 3));
  const ImpTok alt = imp_column(L, 4);
  if (imp_is_dot(text, alt)) o.i32(0);
  else {
    uint32_t len = 0, at = alt.b, k = 0;
    ImpTok a;
    while (imp_next(text, &at, alt.e, ',', &a)) { len += (k ? 1u : 0u) + (imp_tok_eq(text, a, "<NON_REF>", 9u) ? 1u : a.n()); ++k; }
    o.i32((int32_t)len);
    at = alt.b; k = 0;
    while (imp_next(text, &at, alt.e, ',', &a)) {
      if (k++) o.u8((uint8_t)'|');
      if (imp_tok_eq(text, a, "<NON_REF>", 9u)) o.u8((uint8_t)'&');
      else for (uint32_t i = a.b; i < a.e; ++i) o.u8((uint8_t)text[i]);
    }
  }
  if (T.has_id) { const ImpTok id = imp_column(L, 2); if (id.n() && !imp_is_dot(text, id)) o.chars(text, id); else o.i32(0); }
  const ImpTok qual = imp_column(L, 5);
  if (imp_is_dot(text, qual)) o.u32(kNullFloatBits);
  else if (!W) o.n += 4;
  else { float q; if (imp_parse_float(text + qual.b, qual.n(), &q)) o.f32(q); else o.defer(qual, IMP_WHAT_QUAL, IMP_KIND_FLOAT, 0u, 0); }
  const ImpTok filter = imp_column(L, 6);
  if (imp_is_dot(text, filter)) o.i32(0);
  else {
    o.i32((int32_t)imp_count_pieces(text, filter, ';'));
    uint32_t at = filter.b;
    ImpTok f;
    while (imp_next(text, &at, filter.e, ';', &f)) {
      int32_t idx = -1;
      if (W) {
        for (int i = 0; i < T.n_fields && idx < 0; ++i)
          if (imp_tok_eq(text, f, T.names + T.fields[i].off, T.fields[i].len)) idx = (int32_t)T.fields[i].value;
        if (idx < 0) o.err |= IMP_ERR_FILTER;
      }
      o.i32(idx);
    }
  }
  const ImpTok info = imp_column(L, 7);
  for (int i = 0; i < T.n_info; ++i) {
    const ImpAttr& a = T.info[i];
    ImpTok v; v.b = v.e = info.e;
    const bool present = imp_info_find(text, info, T.names + a.name_off, a.name_len, &v);
    imp_values<W>(o, a, i, text, present, v, true, T.n_samples, sample);
  }
  const uint32_t ncols = imp_num_columns(L);
  ImpTok keys; keys.b = keys.e = L.end;
  ImpTok vals = keys;
  const bool has_keys = ncols > 8u, has_vals = ncols > 9u + (uint32_t)sample;
  if (has_keys) keys = imp_column(L, 8);
  if (has_vals) vals = imp_column(L, 9u + (uint32_t)sample);
  for (int i = 0; i < T.n_fmt; ++i) {
    const ImpAttr& a = T.fmt[i];
    ImpTok v; v.b = v.e = L.end;
    bool present = false;
    if (has_keys && has_vals) {      // key i pairs with value i; the last matching pair counts
      uint32_t ka = keys.b, va = vals.b;
      ImpTok k, x;
      while (imp_next(text, &ka, keys.e, ':', &k) && imp_next(text, &va, vals.e, ':', &x))
        if (imp_tok_eq(text, k, T.names + a.name_off, a.name_len)) { v = x; present = true; }
    }
    if (a.gt) imp_gt<W>(o, a, text, present, v);
    else imp_values<W>(o, a, IMP_WHAT_FMT_BASE + i, text, present, v, false, 1, 0);
  }
}

// what one (record line, imported sample) becomes
enum { IMP_SLOT_NONE = 0, IMP_SLOT_CELL = 1, IMP_SLOT_SPANNING_CANDIDATE = 2 };
struct ImpSlot { int64_t col, end; uint64_t size; uint32_t kind, err; };

// measure pass of one (line, sample): coordinates, partition filter, cell size.  Lines that are empty or begin with '#' give nothing.
GDB_HD ImpSlot imp_measure(const ImpTables& T, const ImpLine& L, int sample) {
  ImpSlot s; s.col = 0; s.end = 0; s.size = 0; s.kind = IMP_SLOT_NONE; s.err = 0;
  if (L.end == L.begin || L.text[L.begin] == '#') return s;
  s.err = imp_coords(T, L, &s.col, &s.end);
  if (s.err || sample < 0 || s.col > T.column_end) return s;
  if (s.col < T.column_begin) {
    if (s.end < T.column_begin) return s;      // (still takes part in the per-row choice: the caller sees col <= column_begin)
    s.kind = IMP_SLOT_SPANNING_CANDIDATE;
  } else s.kind = IMP_SLOT_CELL;
  ImpSink<false> o;
  imp_body<false>(T, L, sample, s.end, o);
  s.err |= o.err;
  s.size = 24u + o.n;
  return s;
}

// write pass: the cell's bytes at out (size bytes, as measured); returns ImpErr bits
GDB_HD uint32_t imp_write(const ImpTables& T, const ImpLine& L, int sample, int64_t row, const ImpSlot& s, ImpSink<true>& o) {
  o.limit = s.size;
  o.i64(row); o.i64(s.col); o.i64((int64_t)s.size);
  imp_body<true>(T, L, sample, s.end, o);
  return o.err;
}

GDB_HD uint64_t imp_sort_key(const ImpTables& T, int64_t col, int64_t row) { return ((uint64_t)col << T.key_row_bits) | (uint64_t)row; }

}  // namespace gdbimp
}  // namespace genomicsdb_amd
