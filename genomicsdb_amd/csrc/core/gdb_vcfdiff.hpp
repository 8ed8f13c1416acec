// gdb_vcfdiff.hpp - bodies of the device vcfdiff: the keys of a record line (contig, pos, end, flags, error bits) and the semantic
// compare of a pair of record lines, allele order aside (reference tools/src/vcfdiff.cc compare_line :659-758, compare_unequal_fields
// :472-594, compare_unequal_vector :378-470, the float rule :366-376, the genotype index maps of tools/include/vcfdiff.h:57-100).
// Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_vcfdiff.hip and the CPU harness
// tests/hostsim_vcfdiff/ run the same code.  No allocation, no std::string.  The rule itself is written out in DESIGN.md
// ("Comparing two VCFs").
//
// A pair is compared in two parts.  vd_site does what the line has once: ID, the allele map (gold index -> test index), QUAL, FILTER,
// INFO and the match of the FORMAT keys.  vd_sample does one gold sample against the test sample of the same name and is a template
// over how the lanes of a wavefront share a vector:
//   VdLane   one lane walks both samples token by token (the light path: identity map or at most 3 alleles)
//   a Coop   the lanes of one wavefront index the commas of both vectors into `offs` arrays and compare element k against element
//            m(k) in parallel (the cooperative path; VdSerialCoop below is its one-lane form for the CPU harness)
// Float tokens that are neither byte-identical nor both inside imp_parse_float's exact range are not decided here: they are appended
// to a deferred list and the host decides them with strtod and the same rule.
#pragma once
#include <cmath>
#include <cstdint>

#include "gdb_import.hpp"

namespace genomicsdb_amd {
namespace gdbvdiff {
using gdbimp::ImpLine;
using gdbimp::ImpTok;
using gdbimp::imp_column;
using gdbimp::imp_num_columns;

enum VdErr : uint32_t {      // the lowest bit of a line speaks
  VD_ERR_SHORT = 1u, VD_ERR_CONTIG = 2u, VD_ERR_COORD = 4u, VD_ERR_INFO_KEY = 8u, VD_ERR_NKEYS = 16u, VD_ERR_FMT_KEY = 32u, VD_ERR_ALLELES = 64u,
  VD_ERR_MASK = 255u,
  VD_KEY_RECORD = 256u, VD_KEY_REFBLOCK = 512u, VD_KEY_LONG_REF = 1024u
};
enum { VD_FLAG_ID = 1u, VD_FLAG_ALLELES = 2u, VD_FLAG_QUAL = 4u, VD_FLAG_FILTER = 8u };
enum { VD_MISSING_IN_TEST = 0, VD_ADDED_IN_TEST = 1, VD_TYPE_DIFFERS = 2, VD_DIFFERS = 3 };
enum { VD_T_INT = 0, VD_T_FLOAT = 1, VD_T_FLAG = 2, VD_T_STR = 3 };
enum { VD_C_IDENTITY = 0, VD_C_A = 1, VD_C_R = 2, VD_C_G = 3, VD_C_GT = 4 };
enum { VD_F_TYPE_DIFFERS = 1u, VD_F_NUMBER_DIFFERS = 2u, VD_F_IN_GOLD = 4u, VD_F_IN_TEST = 8u };
enum { VD_WHAT_QUAL = -1, VD_WHAT_FMT_BASE = 64 };      // else: index of the INFO field
constexpr uint32_t kVdMaxFields = 64u, kVdMaxKeys = 64u, kVdMaxAlleles = 255u;

struct VdName { uint32_t off, len; int32_t value; };
struct VdField { uint32_t off, len; uint8_t type, cls, flags, pad; };
struct VdTables {
  const char* names;                       // blob all name offsets point into
  const VdName* contigs[2];                // per file (0 gold, 1 test): the names of its own header -> index in the order of work
  int32_t n_contigs[2];
  const VdField* info; const VdField* fmt; // the union of the names of both headers
  int32_t n_info, n_fmt;
  const int32_t* sample_map;               // gold sample -> test sample of the same name
  int32_t n_samples;
  double threshold;
};
struct VdKey {
  int64_t pos, end;
  int32_t contig; uint32_t bits;           // VdErr | VD_KEY_*
  uint32_t begin, stop, tab_first, ntabs;  // the line in its batch: text range and tabs
};
struct VdDeferred { const char* a; const char* b; uint32_t an, bn; uint32_t pair; int32_t what; };      // a decides the relative difference
struct VdDefer {
  VdDeferred* list; uint32_t* n; uint32_t cap, pair; bool active;
  GDB_HD void push(const char* a, uint32_t an, const char* b, uint32_t bn, int what) const {
    if (!active) return;
    const uint32_t at = gdbimp::imp_atomic_inc(n);
    if (at < cap) { VdDeferred d; d.a = a; d.b = b; d.an = an; d.bn = bn; d.pair = pair; d.what = what; list[at] = d; }
  }
};
struct VdSite {
  uint32_t flags, n_alleles, identity, nkeys_g, nkeys_t, has_fmt, gt_first, pad;
  uint64_t info[4];
  uint8_t amap[256];
  int8_t key_field[kVdMaxKeys];      // gold key i -> FORMAT field (-1: a repeat of an earlier key)
  int8_t key_test[kVdMaxKeys];       // gold key i -> the first test key of the same name (-1: none)
  int8_t tkey_field[kVdMaxKeys];     // test key i -> FORMAT field when no gold key has the name and i is its first (-1 else)
};
struct VdMasks { uint64_t m[4]; };

// ---- tokens ----------------------------------------------------------------------------------------------------------------
GDB_HD bool vd_missing(const char* p, uint32_t n) { return n == 0u || (n == 1u && p[0] == '.'); }
GDB_HD bool vd_bytes_eq(const char* a, uint32_t an, const char* b, uint32_t bn) {
  if (an != bn) return false;
  for (uint32_t i = 0; i < an; ++i) if (a[i] != b[i]) return false;
  return true;
}
GDB_HD bool vd_name_eq(const VdTables& T, uint32_t off, uint32_t len, const char* p, uint32_t n) { return vd_bytes_eq(T.names + off, len, p, n); }
GDB_HD uint32_t vd_count(const char* text, ImpTok t, char sep) { return gdbimp::imp_count_pieces(text, t, sep); }
// piece n of t (an empty range has one empty piece); false when t has fewer
GDB_HD bool vd_nth(const char* text, ImpTok t, char sep, uint32_t n, ImpTok* out) {
  uint32_t at = t.b;
  for (uint32_t k = 0;; ++k) {
    if (!gdbimp::imp_next(text, &at, t.e, sep, out)) return false;
    if (k == n) return true;
  }
}
GDB_HD bool vd_all_missing(const char* text, ImpTok t) {
  uint32_t at = t.b; ImpTok p;
  while (gdbimp::imp_next(text, &at, t.e, ',', &p)) if (!vd_missing(text + p.b, p.n())) return false;
  return true;
}
GDB_HD int vd_find_field(const VdTables& T, const VdField* f, int n, const char* p, uint32_t len) {
  for (int i = 0; i < n; ++i) if (vd_name_eq(T, f[i].off, f[i].len, p, len)) return i;
  return -1;
}
GDB_HD ImpTok vd_info_key(const char* text, ImpTok kv, ImpTok* val) {
  uint32_t eq = kv.b;
  while (eq < kv.e && text[eq] != '=') ++eq;
  ImpTok k; k.b = kv.b; k.e = eq;
  val->b = eq < kv.e ? eq + 1u : kv.e; val->e = kv.e;
  return k;
}

// ---- values ----------------------------------------------------------------------------------------------------------------
// compare_unequal<float> (:366-376): a decides the relative difference; NaN (a missing value against a number) compares false
GDB_HD bool vd_float_rule(float a, float b, double threshold) {
  const float diff = fabsf(a - b);
  const float rel = (a != 0) ? fabsf(diff / a) : 0.0f;
  return ((double)diff > threshold && (double)rel > threshold);
}
GDB_HD bool vd_float_differs(const char* a, uint32_t an, const char* b, uint32_t bn, double threshold, const VdDefer& D, int what) {
  const bool am = vd_missing(a, an), bm = vd_missing(b, bn);
  if (am || bm) return false;                  // both missing: equal; one missing: NaN, never different
  if (vd_bytes_eq(a, an, b, bn)) return false;
  float x, y;
  if (gdbimp::imp_parse_float(a, an, &x) && gdbimp::imp_parse_float(b, bn, &y)) return vd_float_rule(x, y, threshold);
  D.push(a, an, b, bn, what);
  return false;
}
GDB_HD bool vd_int_differs(const char* a, uint32_t an, const char* b, uint32_t bn) {
  const bool am = vd_missing(a, an), bm = vd_missing(b, bn);
  if (am && bm) return false;
  if (am || bm) return true;
  if (vd_bytes_eq(a, an, b, bn)) return false;
  int64_t x, y;
  if (!gdbimp::imp_parse_int(a, an, &x) || !gdbimp::imp_parse_int(b, bn, &y)) return true;
  return x != y;
}
// gold element g against test element t of a field of `type`
GDB_HD bool vd_elem_differs(int type, const char* g, uint32_t gn, const char* t, uint32_t tn, double threshold, const VdDefer& D, int what) {
  if (type == VD_T_FLOAT) return vd_float_differs(g, gn, t, tn, threshold, D, what);
  if (type == VD_T_INT) return vd_int_differs(g, gn, t, tn);
  return !((vd_missing(g, gn) && vd_missing(t, tn)) || vd_bytes_eq(g, gn, t, tn));
}

// ---- genotype index maps ---------------------------------------------------------------------------------------------------
GDB_HD uint64_t vd_binom(uint32_t n, uint32_t k) {
  if (k > n) return 0u;
  uint64_t r = 1u;
  for (uint32_t i = 1; i <= k; ++i) r = r * (uint64_t)(n - k + i) / i;
  return r;
}
// element k of gold's vector -> the element of test's vector it is compared with
GDB_HD uint32_t vd_map_index(int cls, uint32_t k, const uint8_t* amap, uint32_t n_alleles, uint32_t ploidy) {
  if (cls == VD_C_A) return k + 1u < n_alleles ? (uint32_t)amap[k + 1u] - 1u : k;
  if (cls == VD_C_R) return k < n_alleles ? (uint32_t)amap[k] : k;
  if (cls != VD_C_G || ploidy < 1u || ploidy > 8u) return k;
  if ((uint64_t)k >= vd_binom(n_alleles + ploidy - 1u, ploidy)) return k;
  if (ploidy == 1u) return amap[k];
  uint32_t al[8];
  uint64_t rest = k;
  for (uint32_t m = ploidy; m >= 1u; --m) {       // the combinatorial number system, largest allele first
    uint32_t a = 0;
    while (vd_binom(a + m, m) <= rest) ++a;
    rest -= vd_binom(a + m - 1u, m);
    al[m - 1u] = amap[a];
  }
  for (uint32_t i = 1; i < ploidy; ++i) {         // ascending again after the map
    const uint32_t v = al[i];
    uint32_t j = i;
    while (j > 0u && al[j - 1u] > v) { al[j] = al[j - 1u]; --j; }
    al[j] = v;
  }
  uint64_t idx = 0;
  for (uint32_t m = 0; m < ploidy; ++m) idx += vd_binom(al[m] + m, m + 1u);
  return (uint32_t)idx;
}

// ---- GT: allele tokens and the separators in front of the 2nd and later alleles, position by position ------------------------
GDB_HD bool vd_gt_next(const char* text, uint32_t* at, uint32_t e, ImpTok* out, char* sep_after) {
  if (*at > e) return false;
  uint32_t i = *at;
  while (i < e && text[i] != '/' && text[i] != '|') ++i;
  out->b = *at; out->e = i;
  *sep_after = i < e ? text[i] : 0;
  *at = i + 1u;
  return true;
}
GDB_HD uint32_t vd_gt_ploidy(const char* text, ImpTok t) {
  uint32_t n = 1;
  for (uint32_t i = t.b; i < t.e; ++i) n += (text[i] == '/' || text[i] == '|');
  return n;
}
GDB_HD bool vd_gt_differs(const char* gtext, ImpTok g, const char* ttext, ImpTok t) {
  uint32_t ga = g.b, ta = t.b;
  char gsep = 0, tsep = 0;
  for (;;) {
    ImpTok x, y;
    char gs2 = 0, ts2 = 0;
    const bool hg = vd_gt_next(gtext, &ga, g.e, &x, &gs2), ht = vd_gt_next(ttext, &ta, t.e, &y, &ts2);
    if (!hg && !ht) return false;
    if (hg && ht && gsep && tsep && gsep != tsep) return true;
    if (vd_int_differs(hg ? gtext + x.b : ".", hg ? x.n() : 1u, ht ? ttext + y.b : ".", ht ? y.n() : 1u)) return true;
    gsep = hg ? gs2 : 0; tsep = ht ? ts2 : 0;
  }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------
// one line of a batch of text of file `file` (0 gold, 1 test): L as the importer's index gives it ('\r' cut off)
GDB_HD VdKey vd_keys(const VdTables& T, int file, const ImpLine& L) {
  VdKey K; K.pos = 0; K.end = 0; K.contig = -1; K.bits = 0; K.begin = L.begin; K.stop = L.end; K.tab_first = 0; K.ntabs = L.ntabs;
  if (L.end == L.begin || L.text[L.begin] == '#') return K;
  K.bits = VD_KEY_RECORD;
  if (imp_num_columns(L) < 8u) { K.bits |= VD_ERR_SHORT; return K; }
  const char* text = L.text;
  const ImpTok chrom = imp_column(L, 0);
  for (int i = 0; i < T.n_contigs[file] && K.contig < 0; ++i)
    if (vd_name_eq(T, T.contigs[file][i].off, T.contigs[file][i].len, text + chrom.b, chrom.n())) K.contig = T.contigs[file][i].value;
  if (K.contig < 0) K.bits |= VD_ERR_CONTIG;
  const ImpTok pos = imp_column(L, 1), ref = imp_column(L, 3), alt = imp_column(L, 4), info = imp_column(L, 7);
  int64_t v = 0;
  if (!gdbimp::imp_parse_int(text + pos.b, pos.n(), &v)) K.bits |= VD_ERR_COORD;
  K.pos = v - 1;
  K.end = K.pos + (int64_t)ref.n() - 1;
  if (!gdbimp::imp_is_dot(text, info)) {
    ImpTok endv;
    if (gdbimp::imp_info_find(text, info, "END", 3u, &endv)) {      // the last one counts
      if (!gdbimp::imp_parse_int(text + endv.b, endv.n(), &v)) K.bits |= VD_ERR_COORD; else K.end = v - 1;
    }
    uint32_t at = info.b; ImpTok kv;
    while (gdbimp::imp_next(text, &at, info.e, ';', &kv)) {
      ImpTok val;
      const ImpTok k = vd_info_key(text, kv, &val);
      if (gdbimp::imp_tok_eq(text, k, "END", 3u)) continue;
      const int f = vd_find_field(T, T.info, T.n_info, text + k.b, k.n());
      if (f < 0 || !(T.info[f].flags & (file ? VD_F_IN_TEST : VD_F_IN_GOLD))) K.bits |= VD_ERR_INFO_KEY;
    }
  }
  if (imp_num_columns(L) > 8u) {
    const ImpTok keys = imp_column(L, 8);
    if (vd_count(text, keys, ':') > kVdMaxKeys) K.bits |= VD_ERR_NKEYS;
    uint32_t at = keys.b; ImpTok k;
    while (gdbimp::imp_next(text, &at, keys.e, ':', &k)) {
      const int f = vd_find_field(T, T.fmt, T.n_fmt, text + k.b, k.n());
      if (f < 0 || !(T.fmt[f].flags & (file ? VD_F_IN_TEST : VD_F_IN_GOLD))) K.bits |= VD_ERR_FMT_KEY;
    }
  }
  if (!gdbimp::imp_is_dot(text, alt) && 1u + vd_count(text, alt, ',') > kVdMaxAlleles) K.bits |= VD_ERR_ALLELES;
  if (gdbimp::imp_tok_eq(text, alt, "<NON_REF>", 9u)) K.bits |= VD_KEY_REFBLOCK;
  if (ref.n() > 1u) K.bits |= VD_KEY_LONG_REF;
  return K;
}

// ---- vectors ---------------------------------------------------------------------------------------------------------------
// one lane, token by token: the test cursor runs along while m(k) == k, else token m(k) is looked up
GDB_HD bool vd_vector_serial(const VdField& fd, const char* gtext, ImpTok g, const char* ttext, ImpTok t, const VdSite& S, uint32_t ploidy, double threshold,
                             const VdDefer& D, int what) {
  if (fd.cls == VD_C_GT) return vd_gt_differs(gtext, g, ttext, t);
  const bool mapped = fd.cls == VD_C_A || fd.cls == VD_C_R || fd.cls == VD_C_G;
  if (mapped) {
    if (S.flags & VD_FLAG_ALLELES) return true;
    if (vd_count(gtext, g, ',') != vd_count(ttext, t, ',')) return !(vd_all_missing(gtext, g) && vd_all_missing(ttext, t));
  }
  uint32_t ga = g.b, ta = t.b, k = 0;
  ImpTok x, y, z;
  bool hg = gdbimp::imp_next(gtext, &ga, g.e, ',', &x), ht = gdbimp::imp_next(ttext, &ta, t.e, ',', &y);
  for (; hg && ht; ++k) {
    const uint32_t m = mapped ? vd_map_index(fd.cls, k, S.amap, S.n_alleles, ploidy) : k;
    z = y;
    if (m != k && !vd_nth(ttext, t, ',', m, &z)) return true;      // beyond test's vector
    if (vd_elem_differs(fd.type, gtext + x.b, x.n(), ttext + z.b, z.n(), threshold, D, what)) return true;
    hg = gdbimp::imp_next(gtext, &ga, g.e, ',', &x); ht = gdbimp::imp_next(ttext, &ta, t.e, ',', &y);
  }
  for (; hg; hg = gdbimp::imp_next(gtext, &ga, g.e, ',', &x)) if (!vd_missing(gtext + x.b, x.n())) return true;      // the surplus of the longer list
  for (; ht; ht = gdbimp::imp_next(ttext, &ta, t.e, ',', &y)) if (!vd_missing(ttext + y.b, y.n())) return true;
  return false;
}

// the light path: no index, one lane
struct VdLane {
  static constexpr bool kIndexed = false;
  GDB_HD uint32_t lane() const { return 0u; }
  GDB_HD uint32_t lanes() const { return 1u; }
  GDB_HD bool any(bool x) const { return x; }
  GDB_HD uint32_t index(const char*, ImpTok, uint32_t*, uint32_t) const { return 0u; }
};
// the cooperative path with a wavefront of one lane (the CPU harness)
struct VdSerialCoop {
  static constexpr bool kIndexed = true;
  GDB_HD uint32_t lane() const { return 0u; }
  GDB_HD uint32_t lanes() const { return 1u; }
  GDB_HD bool any(bool x) const { return x; }
  // offs[k] = begin of token k, offs[n] = t.e + 1; -> n (nothing is stored at or beyond cap: n >= cap means "not indexed")
  GDB_HD uint32_t index(const char* text, ImpTok t, uint32_t* offs, uint32_t cap) const {
    uint32_t n = 0;
    offs[0] = t.b;
    for (uint32_t i = t.b; i < t.e; ++i) if (text[i] == ',') { ++n; if (n < cap) offs[n] = i + 1u; }
    ++n;
    if (n < cap) offs[n] = t.e + 1u;
    return n;
  }
};

template <class Coop>
GDB_HD bool vd_vector(const Coop& C, const VdField& fd, const char* gtext, ImpTok g, const char* ttext, ImpTok t, const VdSite& S, uint32_t ploidy, double threshold,
                      const VdDefer& D, int what, uint32_t* goffs, uint32_t* toffs, uint32_t cap) {
  VdDefer lane0 = D; lane0.active = D.active && C.lane() == 0u;      // what every lane computes alike is deferred once
  if (!Coop::kIndexed || fd.cls == VD_C_GT) return vd_vector_serial(fd, gtext, g, ttext, t, S, ploidy, threshold, lane0, what);
  const bool mapped = fd.cls == VD_C_A || fd.cls == VD_C_R || fd.cls == VD_C_G;
  if (mapped && (S.flags & VD_FLAG_ALLELES)) return true;
  const uint32_t ng = C.index(gtext, g, goffs, cap), nt = C.index(ttext, t, toffs, cap);
  if (ng >= cap || nt >= cap) return vd_vector_serial(fd, gtext, g, ttext, t, S, ploidy, threshold, lane0, what);
  bool differs = false, valued = false;
  const uint32_t lo = ng < nt ? ng : nt, hi = ng < nt ? nt : ng;
  if (mapped && ng != nt) {
    for (uint32_t k = C.lane(); k < hi; k += C.lanes()) {
      if (k < ng && !vd_missing(gtext + goffs[k], goffs[k + 1u] - 1u - goffs[k])) valued = true;
      if (k < nt && !vd_missing(ttext + toffs[k], toffs[k + 1u] - 1u - toffs[k])) valued = true;
    }
    return C.any(valued);
  }
  for (uint32_t k = C.lane(); k < hi; k += C.lanes()) {
    if (k < lo) {
      const uint32_t m = mapped ? vd_map_index(fd.cls, k, S.amap, S.n_alleles, ploidy) : k;
      if (m >= nt) { differs = true; continue; }
      if (vd_elem_differs(fd.type, gtext + goffs[k], goffs[k + 1u] - 1u - goffs[k], ttext + toffs[m], toffs[m + 1u] - 1u - toffs[m], threshold, D, what)) differs = true;
    } else if (k < ng) { if (!vd_missing(gtext + goffs[k], goffs[k + 1u] - 1u - goffs[k])) differs = true; }
    else if (!vd_missing(ttext + toffs[k], toffs[k + 1u] - 1u - toffs[k])) differs = true;
  }
  return C.any(differs);
}

// what compare_unequal_fields does with one field: both lines have it (tv != nullptr) or only one (which = VD_MISSING_IN_TEST / VD_ADDED_IN_TEST)
template <class Coop>
GDB_HD void vd_field_both(const Coop& C, const VdField& fd, int f, VdMasks& M, const char* gtext, ImpTok g, const char* ttext, ImpTok t, const VdSite& S, uint32_t ploidy,
                          double threshold, const VdDefer& D, int what, uint32_t* goffs, uint32_t* toffs, uint32_t cap) {
  if (fd.flags & VD_F_TYPE_DIFFERS) { M.m[VD_TYPE_DIFFERS] |= 1ull << f; return; }
  if (fd.type == VD_T_FLAG) return;
  if ((fd.flags & VD_F_NUMBER_DIFFERS) || vd_vector(C, fd, gtext, g, ttext, t, S, ploidy, threshold, D, what, goffs, toffs, cap)) M.m[VD_DIFFERS] |= 1ull << f;
}
GDB_HD void vd_field_one(const VdField& fd, int f, VdMasks& M, int which, const char* text, ImpTok v) {
  if (fd.type != VD_T_FLAG && !vd_all_missing(text, v)) M.m[which] |= 1ull << f;
}

// ---- the site part ---------------------------------------------------------------------------------------------------------
GDB_HD bool vd_token_in(const char* text, ImpTok list, char s1, char s2, const char* p, uint32_t n) {
  uint32_t b = list.b;
  for (uint32_t i = list.b; i <= list.e; ++i)
    if (i == list.e || text[i] == s1 || text[i] == s2) { if (vd_bytes_eq(text + b, i - b, p, n)) return true; b = i + 1u; }
  return false;
}
GDB_HD bool vd_tokens_subset(const char* atext, ImpTok a, const char* btext, ImpTok b, char s1, char s2) {      // every token of a is one of b's
  uint32_t s = a.b;
  for (uint32_t i = a.b; i <= a.e; ++i)
    if (i == a.e || atext[i] == s1 || atext[i] == s2) { if (!vd_token_in(btext, b, s1, s2, atext + s, i - s)) return false; s = i + 1u; }
  return true;
}

GDB_HD void vd_site(const VdTables& T, const ImpLine& G, const ImpLine& Tt, bool pos_equal, const VdDefer& D, VdSite& S) {
  const char* gt = G.text; const char* tt = Tt.text;
  S.flags = 0; S.identity = 1; S.nkeys_g = 0; S.nkeys_t = 0; S.has_fmt = 0; S.gt_first = 0; S.pad = 0;
  for (int i = 0; i < 4; ++i) S.info[i] = 0;
  // ID: the two sets of tokens split at ';' and ',' (:596-610)
  const ImpTok gid = imp_column(G, 2), tid = imp_column(Tt, 2);
  if (!vd_tokens_subset(gt, gid, tt, tid, ';', ',') || !vd_tokens_subset(tt, tid, gt, gid, ';', ',')) S.flags |= VD_FLAG_ID;
  // alleles and the map gold index -> test index (:688-711)
  const ImpTok gref = imp_column(G, 3), tref = imp_column(Tt, 3), galt = imp_column(G, 4), talt = imp_column(Tt, 4);
  const uint32_t gn = gdbimp::imp_is_dot(gt, galt) ? 0u : vd_count(gt, galt, ','), tn = gdbimp::imp_is_dot(tt, talt) ? 0u : vd_count(tt, talt, ',');
  S.n_alleles = 1u + gn;
  S.amap[0] = 0;
  if (gn != tn || gn + 1u > kVdMaxAlleles || (pos_equal && !vd_bytes_eq(gt + gref.b, gref.n(), tt + tref.b, tref.n()))) S.flags |= VD_FLAG_ALLELES;
  else if (gn) {
    if (!vd_tokens_subset(tt, talt, gt, galt, ',', ',')) S.flags |= VD_FLAG_ALLELES;
    uint32_t at = galt.b, i = 1; ImpTok a;
    for (; !(S.flags & VD_FLAG_ALLELES) && gdbimp::imp_next(gt, &at, galt.e, ',', &a); ++i) {
      uint32_t bt = talt.b, j = 1; ImpTok b; bool found = false;
      for (; !found && gdbimp::imp_next(tt, &bt, talt.e, ',', &b); ++j) found = vd_bytes_eq(gt + a.b, a.n(), tt + b.b, b.n());
      if (!found) { S.flags |= VD_FLAG_ALLELES; break; }
      S.amap[i] = (uint8_t)(j - 1u);
      if (j - 1u != i) S.identity = 0;
    }
  }
  if (S.flags & VD_FLAG_ALLELES) S.identity = 1;      // no vector goes through the map
  // QUAL: a is test (:714)
  const ImpTok gq = imp_column(G, 5), tq = imp_column(Tt, 5);
  if (vd_float_differs(tt + tq.b, tq.n(), gt + gq.b, gq.n(), T.threshold, D, VD_WHAT_QUAL)) S.flags |= VD_FLAG_QUAL;
  // FILTER (:718-735)
  const ImpTok gf = imp_column(G, 6), tf = imp_column(Tt, 6);
  const uint32_t gfn = gdbimp::imp_is_dot(gt, gf) ? 0u : vd_count(gt, gf, ';'), tfn = gdbimp::imp_is_dot(tt, tf) ? 0u : vd_count(tt, tf, ';');
  if (gfn != tfn || (tfn && !vd_tokens_subset(tt, tf, gt, gf, ';', ';'))) S.flags |= VD_FLAG_FILTER;
  // INFO, END skipped; a key that repeats counts once, with its last value
  const ImpTok gi = imp_column(G, 7), ti = imp_column(Tt, 7);
  VdMasks M; for (int i = 0; i < 4; ++i) M.m[i] = 0;
  const VdLane lane;
  for (int side = 0; side < 2; ++side) {
    const char* at_text = side ? tt : gt; const char* ot_text = side ? gt : tt;
    const ImpTok mine = side ? ti : gi, other = side ? gi : ti;
    if (gdbimp::imp_is_dot(at_text, mine)) continue;
    uint32_t at = mine.b; ImpTok kv;
    while (gdbimp::imp_next(at_text, &at, mine.e, ';', &kv)) {
      ImpTok val, oval;
      const ImpTok k = vd_info_key(at_text, kv, &val);
      if (gdbimp::imp_tok_eq(at_text, k, "END", 3u)) continue;
      bool earlier = false;
      { uint32_t bt = mine.b; ImpTok kv2, v2; while (!earlier && gdbimp::imp_next(at_text, &bt, mine.e, ';', &kv2) && kv2.b < kv.b) { const ImpTok k2 = vd_info_key(at_text, kv2, &v2); earlier = vd_bytes_eq(at_text + k2.b, k2.n(), at_text + k.b, k.n()); } }
      if (earlier) continue;
      const int f = vd_find_field(T, T.info, T.n_info, at_text + k.b, k.n());
      if (f < 0) continue;      // (refused by the keys pass)
      ImpTok last = val;
      gdbimp::imp_info_find(at_text, mine, at_text + k.b, k.n(), &last);      // the last value of a key that repeats
      const bool has = gdbimp::imp_info_find(ot_text, other, at_text + k.b, k.n(), &oval);
      if (!has) vd_field_one(T.info[f], f, M, side ? VD_ADDED_IN_TEST : VD_MISSING_IN_TEST, at_text, last);
      else if (!side) vd_field_both(lane, T.info[f], f, M, gt, last, tt, oval, S, 0u, T.threshold, D, f, nullptr, nullptr, 0u);
    }
  }
  for (int i = 0; i < 4; ++i) S.info[i] = M.m[i];
  // the match of the FORMAT keys
  if (imp_num_columns(G) > 8u && imp_num_columns(Tt) > 8u) {
    S.has_fmt = 1;
    const ImpTok gk = imp_column(G, 8), tk = imp_column(Tt, 8);
    uint32_t at = gk.b; ImpTok k;
    while (S.nkeys_g < kVdMaxKeys && gdbimp::imp_next(gt, &at, gk.e, ':', &k)) {
      const uint32_t i = S.nkeys_g++;
      if (i == 0u && gdbimp::imp_tok_eq(gt, k, "GT", 2u)) S.gt_first = 1;
      S.key_field[i] = -1; S.key_test[i] = -1;
      uint32_t bt = gk.b; ImpTok k2; bool earlier = false;
      while (!earlier && gdbimp::imp_next(gt, &bt, gk.e, ':', &k2) && k2.b < k.b) earlier = vd_bytes_eq(gt + k2.b, k2.n(), gt + k.b, k.n());
      if (earlier) continue;
      S.key_field[i] = (int8_t)vd_find_field(T, T.fmt, T.n_fmt, gt + k.b, k.n());
      uint32_t ct = tk.b, j = 0;
      for (; gdbimp::imp_next(tt, &ct, tk.e, ':', &k2); ++j) if (j < kVdMaxKeys && vd_bytes_eq(tt + k2.b, k2.n(), gt + k.b, k.n())) { S.key_test[i] = (int8_t)j; break; }
    }
    at = tk.b;
    while (S.nkeys_t < kVdMaxKeys && gdbimp::imp_next(tt, &at, tk.e, ':', &k)) {
      const uint32_t i = S.nkeys_t++;
      S.tkey_field[i] = -1;
      uint32_t bt = tk.b; ImpTok k2; bool earlier = false;
      while (!earlier && gdbimp::imp_next(tt, &bt, tk.e, ':', &k2) && k2.b < k.b) earlier = vd_bytes_eq(tt + k2.b, k2.n(), tt + k.b, k.n());
      if (earlier || vd_token_in(gt, gk, ':', ':', tt + k.b, k.n())) continue;
      S.tkey_field[i] = (int8_t)vd_find_field(T, T.fmt, T.n_fmt, tt + k.b, k.n());
    }
  }
}
// which per-sample path a pair takes
GDB_HD bool vd_is_heavy(const VdSite& S) { return S.has_fmt && !S.identity && S.n_alleles > 3u; }

// ---- one gold sample j against the test sample of the same name --------------------------------------------------------------
GDB_HD ImpTok vd_sample_column(const ImpLine& L, uint32_t s) {
  if (9u + s < imp_num_columns(L)) return imp_column(L, 9u + s);
  ImpTok none; none.b = L.end; none.e = L.end;
  return none;
}
// subfield i of a sample; an absent trailing subfield is the one-element list [missing] (an empty range)
GDB_HD ImpTok vd_subfield(const char* text, ImpTok col, uint32_t i) {
  ImpTok out;
  if (!vd_nth(text, col, ':', i, &out)) { out.b = col.e; out.e = col.e; }
  return out;
}
template <class Coop>
GDB_HD VdMasks vd_sample(const Coop& C, const VdTables& T, const ImpLine& G, const ImpLine& Tt, const VdSite& S, uint32_t j, const VdDefer& D, uint32_t* goffs,
                         uint32_t* toffs, uint32_t cap) {
  VdMasks M; for (int i = 0; i < 4; ++i) M.m[i] = 0;
  if (!S.has_fmt) return M;
  const char* gt = G.text; const char* tt = Tt.text;
  const ImpTok gs = vd_sample_column(G, j), ts = vd_sample_column(Tt, (uint32_t)T.sample_map[j]);
  const uint32_t ploidy = S.gt_first ? vd_gt_ploidy(gt, vd_subfield(gt, gs, 0u)) : 0u;
  for (uint32_t i = 0; i < S.nkeys_g; ++i) {
    const int f = S.key_field[i];
    if (f < 0) continue;
    const ImpTok gv = vd_subfield(gt, gs, i);
    if (S.key_test[i] < 0) vd_field_one(T.fmt[f], f, M, VD_MISSING_IN_TEST, gt, gv);
    else vd_field_both(C, T.fmt[f], f, M, gt, gv, tt, vd_subfield(tt, ts, (uint32_t)S.key_test[i]), S, ploidy, T.threshold, D, VD_WHAT_FMT_BASE + f, goffs, toffs, cap);
  }
  for (uint32_t i = 0; i < S.nkeys_t; ++i) {
    const int f = S.tkey_field[i];
    if (f >= 0) vd_field_one(T.fmt[f], f, M, VD_ADDED_IN_TEST, tt, vd_subfield(tt, ts, i));
  }
  return M;
}

}  // namespace gdbvdiff
}  // namespace genomicsdb_amd
