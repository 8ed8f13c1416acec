// gdb_variants.hpp - the variants query: what `gt_mpi_gather` prints when it is given no mode flag.
//
// The reference calls VariantQueryProcessor::gt_get_column_interval for every query interval (src/main/cpp/src/genomicsdb/query_variants.cc:687-843):
// the calls whose interval covers the interval's begin, sorted by (begin, row), then every cell that begins behind it, each moved into the
// Variant that holds the same (begin, end, REF, set of ALT strings) or into a new one behind all others (GA4GHCallInfoToVariantIdx::find_or_insert,
// variant.cc:26-71).  Variants with more than one call go through GA4GHOperator::operate + copy_back_remapped_fields
// (src/query_operations/variant_operations.cc:572-728): merged REF / ALT become the variant's common fields, GT and every field whose length
// depends on the alleles are rewritten in merged allele order.  print_variants (variant.cc:942-1000) prints the lot with Variant::print /
// VariantCall::print and the VariantField*::print family of variant_field_data.h under std::fixed, precision 6.
//
// Here the staged cells are sorted by (begin, row) already, so the reference's call order is the cell order of the selected cells
// (calls_select, gdb_calls.hpp) and a group never crosses a begin column.  A call is a thread: all calls of a group carry the same ALT set,
// so the merged allele list is the group's first call's ALT (<NON_REF> last) and every call can remap its own fields knowing only that
// first call - no per-group pass, no skew.  The bodies below compile under hipcc and g++ (tests/hostsim_variants).
#pragma once
#include "gdb_calls.hpp"

namespace genomicsdb_amd {

#define GDB_GA4GH_MAX_ALT_FOR_GENOTYPE_FIELDS 50   // MAX_DIPLOID_ALT_ALLELES_THAT_CAN_BE_GENOTYPED: GA4GHOperator is built with its default (query_variants.cc:825)

// ---- std::ostream << std::fixed << std::setprecision(6) << float  ( = printf("%.6f", (double)f) ) ------------------------------------
// A float is M * 2^e2 with M < 2^24: M * 10^6 fits 44 bits, so the value times 10^6 is an exact integer shift away.  e2 < 0: one 64-bit
// shift with round-half-even on the exact remainder (what glibc does in the default rounding mode); e2 >= 0: the exact integer, up to
// 148 bits, taken apart in 10^9 limbs.
template <class Sink> GDB_HD void put_float_fixed6(Sink& s, float f) {
  const uint32_t bits = gdb_f2u(f);
  if (bits >> 31) s.put('-');
  const uint32_t ex = (bits >> 23) & 0xFFu, man = bits & 0x7FFFFFu;
  if (ex == 0xFFu) { put_lit(s, man ? "nan" : "inf"); return; }
  const uint64_t M = ex ? (uint64_t)(man | 0x800000u) : (uint64_t)man;
  const int e2 = (ex ? (int)ex : 1) - 150;
  const uint64_t P = M * 1000000ull;
  if (e2 < 0) {
    const int sh = -e2;
    uint64_t q = 0;
    if (sh < 64) {
      q = P >> sh;
      const uint64_t rem = P & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
      if (rem > half || (rem == half && (q & 1ull))) ++q;
    }
    put_u64(s, q / 1000000ull);
    s.put('.');
    uint32_t fr = (uint32_t)(q % 1000000ull);
    for (uint32_t d = 100000u; d; d /= 10u) { s.put((char)('0' + fr / d)); fr %= d; }
    return;
  }
  uint32_t w[6] = {0, 0, 0, 0, 0, 0};
  {
    const int word = e2 >> 5, bit = e2 & 31;
    const uint64_t a = (P & 0xFFFFFFFFull) << bit, b = ((P >> 32) << bit) + (a >> 32);
    w[word] = (uint32_t)a; w[word + 1] = (uint32_t)b; w[word + 2] = (uint32_t)(b >> 32);
  }
  uint32_t limb[5];
  int nl = 0;
  for (;;) {
    uint64_t r = 0;
    uint32_t any = 0;
    for (int i = 5; i >= 0; --i) { const uint64_t cur = (r << 32) | w[i]; w[i] = (uint32_t)(cur / 1000000000ull); r = cur % 1000000000ull; any |= w[i]; }
    limb[nl++] = (uint32_t)r;
    if (!any || nl == 5) break;
  }
  char d[48];
  int nd = 0;
  for (int i = nl - 1; i >= 0; --i) {
    uint32_t v = limb[i];
    for (uint32_t p = 100000000u; p; p /= 10u) { const uint32_t dg = v / p; v %= p; if (nd || dg) d[nd++] = (char)('0' + dg); }
  }
  s.write(d, nd - 6); s.put('.'); s.write(d + nd - 6, 6);      // (e2 >= 0: the value is at least 2^23, so nd > 6)
}

// ---- ALT tokens ('|' separated as stored; "&" is <NON_REF>) ---------------------------------------------------------------------------
struct VarAlt { const char* p; int n; int16_t b[GDB_MAX_INPUT_ALLELES], l[GDB_MAX_INPUT_ALLELES]; };
GDB_HD void var_alt_split(const FragmentView& fr, const CombinePlan& pl, int64_t c, VarAlt& a, uint32_t* err) {
  int len;
  a.p = cell_field<char>(fr, pl, pl.f_ALT, c, len);
  a.n = 0;
  if (len <= 0) return;
  if (len > 32000) { *err |= GDB_ERR_TOO_MANY_INPUT_ALLELES; len = 32000; }
  int b = 0;
  for (;;) {
    int e = b;
    while (e < len && a.p[e] != '|') ++e;
    if (a.n + 1 >= GDB_MAX_INPUT_ALLELES) { *err |= GDB_ERR_TOO_MANY_INPUT_ALLELES; return; }     // (REF counts as an allele)
    a.b[a.n] = (int16_t)b; a.l[a.n] = (int16_t)(e - b); ++a.n;
    if (e >= len) break;
    b = e + 1;
  }
}
GDB_HD bool var_tok_is_non_ref(const VarAlt& a, int i) { return a.l[i] == 1 && a.p[a.b[i]] == '&'; }
GDB_HD int var_tok_cmp(const VarAlt& x, int i, const VarAlt& y, int j) {
  const int n = x.l[i] < y.l[j] ? x.l[i] : y.l[j];
  for (int k = 0; k < n; ++k) { const unsigned char p = (unsigned char)x.p[x.b[i] + k], q = (unsigned char)y.p[y.b[j] + k]; if (p != q) return p < q ? -1 : 1; }
  return x.l[i] == y.l[j] ? 0 : (x.l[i] < y.l[j] ? -1 : 1);
}
// the tokens as a std::set<std::string> would hold them: sorted, each once.  ord[] = token indices; returns how many
GDB_HD int var_alt_sorted_set(const VarAlt& a, uint8_t* ord) {
  int n = 0;
  for (int i = 0; i < a.n; ++i) {
    int j = n;
    bool dup = false;
    while (j > 0) { const int r = var_tok_cmp(a, ord[j - 1], a, i); if (r == 0) { dup = true; break; } if (r < 0) break; --j; }
    if (dup) continue;
    for (int k = n; k > j; --k) ord[k] = ord[k - 1];
    ord[j] = (uint8_t)i; ++n;
  }
  return n;
}

// ---- the grouping key: (begin, end, REF, ALT set) --------------------------------------------------------------------------------------
GDB_HD uint64_t var_fnv(uint64_t h, const char* p, int n) { for (int i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; } return h; }
GDB_HD uint64_t var_call_hash(const FragmentView& fr, const CombinePlan& pl, int64_t c, int64_t end, uint32_t* err) {
  uint64_t h = 14695981039346656037ull;
  const int64_t be[2] = {fr.begin[c], end};
  h = var_fnv(h, (const char*)be, 16);
  int nref;
  const char* ref = cell_field<char>(fr, pl, pl.f_REF, c, nref);
  h = var_fnv(h, ref, nref);
  VarAlt a;
  var_alt_split(fr, pl, c, a, err);
  uint8_t ord[GDB_MAX_INPUT_ALLELES];
  const int n = var_alt_sorted_set(a, ord);
  for (int i = 0; i < n; ++i) { const char sep = (char)0xFF; h = var_fnv(h, &sep, 1); h = var_fnv(h, a.p + a.b[ord[i]], a.l[ord[i]]); }
  return h;
}
// equal keys, by content
GDB_HD bool var_same_key(const FragmentView& fr, const CombinePlan& pl, int64_t c1, int64_t end1, int64_t c2, int64_t end2) {
  if (c1 == c2) return true;
  if (fr.begin[c1] != fr.begin[c2] || end1 != end2) return false;
  int n1, n2;
  const char* r1 = cell_field<char>(fr, pl, pl.f_REF, c1, n1);
  const char* r2 = cell_field<char>(fr, pl, pl.f_REF, c2, n2);
  if (n1 != n2) return false;
  for (int i = 0; i < n1; ++i) if (r1[i] != r2[i]) return false;
  const char* a1 = cell_field<char>(fr, pl, pl.f_ALT, c1, n1);
  const char* a2 = cell_field<char>(fr, pl, pl.f_ALT, c2, n2);
  if (n1 == n2) { bool same = true; for (int i = 0; i < n1; ++i) if (a1[i] != a2[i]) { same = false; break; } if (same) return true; }
  uint32_t e = 0;
  VarAlt x, y;
  var_alt_split(fr, pl, c1, x, &e); var_alt_split(fr, pl, c2, y, &e);
  uint8_t ox[GDB_MAX_INPUT_ALLELES], oy[GDB_MAX_INPUT_ALLELES];
  const int nx = var_alt_sorted_set(x, ox), ny = var_alt_sorted_set(y, oy);
  if (nx != ny) return false;
  for (int i = 0; i < nx; ++i) if (var_tok_cmp(x, ox[i], y, oy[i]) != 0) return false;
  return true;
}
// The first call of sorted position p's group.  sorted[]: call indices stably sorted by hash (so ascending inside a run of equal hashes),
// run_start[p]: first position of p's run.  Calls with the run head's content - all of them unless two keys collide - need one comparison.
GDB_HD int64_t var_find_leader(const FragmentView& fr, const CombinePlan& pl, const int64_t* call_cell, const int64_t* call_end, const int64_t* sorted, const int64_t* run_start, int64_t p) {
  const int64_t i = sorted[p];
  for (int64_t q = run_start[p]; q < p; ++q) {
    const int64_t j = sorted[q];
    if (var_same_key(fr, pl, call_cell[i], call_end[i], call_cell[j], call_end[j])) return j;
  }
  return i;
}

// ---- GA4GHOperator for one call of a group whose first call is `lead` --------------------------------------------------------------------
struct VarRemap {
  bool on;            // m_remapping_needed: the merged alleles are not those of a plain reference block
  bool non_ref;
  int num_merged;     // REF included
  int ploidy;         // of this call's GT (0: GT not queried or not valid)
  int8_t m2i[GDB_MAX_INPUT_ALLELES], i2m[GDB_MAX_INPUT_ALLELES];   // merged allele -> this call's allele (-1: none) and back
  int8_t merged_tok[GDB_MAX_INPUT_ALLELES];                          // merged ALT j (0-based) -> token of the first call
};
GDB_HD void var_build_remap(const FragmentView& fr, const CombinePlan& pl, int64_t c, int64_t lead, VarRemap& rm, VarAlt& la, uint32_t* err) {
  VarAlt own;
  var_alt_split(fr, pl, lead, la, err);
  var_alt_split(fr, pl, c, own, err);
  int nm = 0;
  rm.non_ref = false;
  for (int i = 0; i < la.n; ++i) {                                   // merge_alt_alleles: first sight decides the place, <NON_REF> goes last
    if (var_tok_is_non_ref(la, i)) { rm.non_ref = true; continue; }
    bool seen = false;
    for (int j = 0; j < nm && !seen; ++j) seen = var_tok_cmp(la, rm.merged_tok[j], la, i) == 0;
    if (!seen) rm.merged_tok[nm++] = (int8_t)i;
  }
  if (rm.non_ref) for (int i = 0; i < la.n; ++i) if (var_tok_is_non_ref(la, i)) { rm.merged_tok[nm++] = (int8_t)i; break; }
  rm.num_merged = nm + 1;
  int nref;
  (void)cell_field<char>(fr, pl, pl.f_REF, lead, nref);
  rm.on = !(nref == 1 && nm == 1 && rm.non_ref);
  for (int j = 0; j < GDB_MAX_INPUT_ALLELES; ++j) { rm.m2i[j] = -1; rm.i2m[j] = -1; }
  rm.m2i[0] = 0; rm.i2m[0] = 0;
  for (int a = 0; a < own.n; ++a)                                    // (the LUT keeps the last pair added for a merged allele)
    for (int j = 0; j < nm; ++j)
      if (var_tok_cmp(la, rm.merged_tok[j], own, a) == 0) { rm.m2i[j + 1] = (int8_t)(a + 1); rm.i2m[a + 1] = (int8_t)(j + 1); break; }
  rm.ploidy = 0;
  if (pl.f_GT >= 0) {
    int n;
    const int32_t* gt = cell_field<int32_t>(fr, pl, pl.f_GT, c, n);
    bool valid = false;
    for (int i = 0; i < n; ++i) if (gt[i] != GDB_TILEDB_NULL_INT32) valid = true;
    if (valid) rm.ploidy = pl.field[pl.f_GT].length == GDB_VL_PP ? (n + 1) / 2 : n;
    if (rm.ploidy > GDB_MAX_PLOIDY) { *err |= GDB_ERR_UNSUPPORTED_PLOIDY; rm.ploidy = 0; }
  }
}

GDB_HD int32_t var_missing(int32_t) { return GDB_BCF_INT32_MISSING; }
GDB_HD float var_missing(float) { union { uint32_t u; float f; } x; x.u = GDB_BCF_FLOAT_MISSING_BITS; return x.f; }
template <class Sink> GDB_HD void var_put_elem(Sink& s, int32_t v) { put_i32(s, v); }
template <class Sink> GDB_HD void var_put_elem(Sink& s, float v) { put_float_fixed6(s, v); }
template <class Sink> struct VarList {     // VariantFieldPrimitiveVectorData::print: "[ a,b ]"
  Sink& s; bool first;
  GDB_HD explicit VarList(Sink& q) : s(q), first(true) { put_lit(s, "[ "); }
  template <class T> GDB_HD void add(T v) { if (!first) s.put(','); first = false; var_put_elem(s, v); }
  GDB_HD void close() { put_lit(s, " ]"); }
};
// remap_data_based_on_alleles / remap_data_based_on_genotype (variant_field_handler.cc:41-398) of one call, printed as they come
template <class T, class Sink> GDB_HD void var_put_remapped(Sink& s, const T* p, int n, int length, const VarRemap& rm) {
  VarList<Sink> out(s);
  const T miss = var_missing(T());
  const int nm = rm.num_merged;
  if (length == GDB_VL_R || length == GDB_VL_A) {
    const int d = length == GDB_VL_A ? 1 : 0;
    for (int j = d; j < nm; ++j) { const int in = rm.m2i[j] - d; out.add(rm.m2i[j] >= 0 && in < n ? p[in] : miss); }
  } else if (rm.ploidy == 1) {
    for (int j = 0; j < nm; ++j) out.add(rm.m2i[j] >= 0 && rm.m2i[j] < n ? p[rm.m2i[j]] : miss);
  } else if (rm.ploidy == 2) {
    for (int k = 0; k < nm; ++k)
      for (int j = 0; j <= k; ++j) {
        if (rm.m2i[j] < 0 || rm.m2i[k] < 0) { out.add(miss); continue; }
        const int in = gdb_alleles2gt(rm.m2i[j], rm.m2i[k]);
        out.add(in < n ? p[in] : miss);
      }
  } else if (rm.ploidy == 0) {                           // the field is resized to the one genotype of ploidy 0 and nothing is remapped
    out.add(n > 0 ? p[0] : T(0));
  } else {
    int a[GDB_MAX_PLOIDY], b[GDB_MAX_PLOIDY];
    for (int i = 0; i < rm.ploidy; ++i) a[i] = 0;
    do {
      bool ok = true;
      for (int i = 0; i < rm.ploidy; ++i) { b[i] = rm.m2i[a[i]]; ok = ok && b[i] >= 0; }
      const int64_t in = ok ? gdb_genotype_index(b, rm.ploidy) : -1;
      out.add(ok && in < n ? p[in] : miss);
    } while (gdb_next_genotype(a, rm.ploidy, nm));
  }
  out.close();
}

// validity of a Variant field (VariantFieldPrimitiveVectorData / VariantFieldData<std::string>::binary_deserialize): some element is not the TileDB null
GDB_HD bool variants_field_valid(const FragmentView& fr, const CombinePlan& pl, int f, int64_t c) {
  const GdbFieldDesc& fd = pl.field[f];
  int n;
  if (fd.elem == GDB_ET_INT) { const int32_t* p = cell_field<int32_t>(fr, pl, f, c, n); for (int i = 0; i < n; ++i) if (p[i] != GDB_TILEDB_NULL_INT32) return true; }
  else if (fd.elem == GDB_ET_FLOAT) { const float* p = cell_field<float>(fr, pl, f, c, n); for (int i = 0; i < n; ++i) if (gdb_f2u(p[i]) != GDB_TILEDB_NULL_FLOAT_BITS) return true; }
  else { const char* p = cell_field<char>(fr, pl, f, c, n); for (int i = 0; i < n; ++i) if (p[i] != GDB_TILEDB_NULL_CHAR) return true; }
  return false;
}
template <class Sink> GDB_HD void var_put_alt_token(Sink& s, const VarAlt& a, int i) {
  s.put('"');
  if (var_tok_is_non_ref(a, i)) put_lit(s, "<NON_REF>"); else s.write(a.p + a.b[i], a.l[i]);
  s.put('"');
}
// VariantField*::print of field f of call c; rm: the remap of its variant (null: a variant of one call)
template <class Sink> GDB_HD void variants_put_field(Sink& s, const FragmentView& fr, const CombinePlan& pl, int f, int64_t c, const VarRemap* rm, uint32_t* err) {
  const GdbFieldDesc& fd = pl.field[f];
  int n;
  if (f == pl.f_ALT) {
    VarAlt a;
    var_alt_split(fr, pl, c, a, err);
    put_lit(s, "[ ");
    for (int i = 0; i < a.n; ++i) { if (i) s.put(','); var_put_alt_token(s, a, i); }
    put_lit(s, " ]");
    return;
  }
  if (fd.elem == GDB_ET_CHAR) { const char* p = cell_field<char>(fr, pl, f, c, n); s.put('"'); s.write(p, n); s.put('"'); return; }
  if (fd.elem == GDB_ET_FLAG) {
    const unsigned char* p = (const unsigned char*)cell_field<char>(fr, pl, f, c, n);
    VarList<Sink> out(s);
    for (int i = 0; i < n; ++i) out.add((int32_t)p[i]);
    out.close();
    return;
  }
  const bool remap = rm && rm->on;
  if (remap && f == pl.f_GT && fd.elem == GDB_ET_INT) {                 // VariantOperations::remap_GT_field
    const int32_t* p = cell_field<int32_t>(fr, pl, f, c, n);
    const int step = fd.length == GDB_VL_PP ? 2 : 1;
    VarList<Sink> out(s);
    for (int i = 0; i < n; ++i) {
      int32_t v = p[i];
      if (i % step == 0 && v != GDB_TILEDB_NULL_INT32 && v != -1 && v != GDB_BCF_INT32_MISSING) {
        const int m = v >= 0 && v < GDB_MAX_INPUT_ALLELES ? rm->i2m[v] : -1;
        v = m >= 0 ? m : (rm->non_ref ? rm->num_merged - 1 : -1);
      }
      out.add(v);
    }
    out.close();
    return;
  }
  const bool by_allele = fd.length == GDB_VL_A || fd.length == GDB_VL_R || fd.length == GDB_VL_G;
  const bool dropped = fd.length == GDB_VL_G && rm && rm->num_merged - 1 > GDB_GA4GH_MAX_ALT_FOR_GENOTYPE_FIELDS;   // too_many_alt_alleles_for_genotype_length_fields: left as stored
  if (fd.elem == GDB_ET_INT) {
    const int32_t* p = cell_field<int32_t>(fr, pl, f, c, n);
    if (remap && by_allele && !dropped) { var_put_remapped(s, p, n, fd.length, *rm); return; }
    VarList<Sink> out(s);
    for (int i = 0; i < n; ++i) out.add(p[i]);
    out.close();
  } else {
    const float* p = cell_field<float>(fr, pl, f, c, n);
    if (remap && by_allele && !dropped) { var_put_remapped(s, p, n, fd.length, *rm); return; }
    VarList<Sink> out(s);
    for (int i = 0; i < n; ++i) out.add(p[i]);
    out.close();
  }
}

template <class Sink> GDB_HD void var_put_intervals(Sink& s, const QueryWindow& qw, int64_t begin, int64_t end, int indent, const char* sep) {
  put_spaces(s, indent); put_lit(s, "\"interval\": [ "); put_i64(s, begin); put_lit(s, sep); put_i64(s, end); put_lit(s, " ],\n");
  const int ci = find_contig(qw, begin);
  if (ci >= 0) {
    const GdbContig& g = qw.contigs[ci];
    const int64_t pos = begin - g.offset;
    put_spaces(s, indent); put_lit(s, "\"genomic_interval\": { \""); s.write(qw.contig_names + g.name_off, g.name_len);
    put_lit(s, "\" : [ "); put_i64(s, pos + 1); put_lit(s, ", "); put_i64(s, pos + 1 + (end - begin)); put_lit(s, " ] },\n");
  }
}

// One call's share of the document: Variant::print's frame in front of the first call of a variant (",\n" in front of every variant: the
// caller drops the first) and behind its last one, VariantCall::print in between.  lead: the cell of the variant's first call.
template <class Sink> GDB_HD void variants_emit_call(Sink& s, const FragmentView& fr, const CombinePlan& pl, const QueryWindow& qw, const CallsNames& names, int64_t c, int64_t end,
                                                     int64_t lead, bool first, bool last, uint32_t* err) {
  const int64_t begin = fr.begin[c];
  const bool multi = !(first && last);
  VarRemap rm;
  VarAlt la;
  rm.on = false;
  if (multi) var_build_remap(fr, pl, c, lead, rm, la, err);
  if (first) {
    put_lit(s, ",\n"); put_spaces(s, 8); put_lit(s, "{\n");
    var_put_intervals(s, qw, begin, end, 12, ", ");
    put_spaces(s, 12); put_lit(s, " \"common_fields\" : {\n");
    if (multi) {
      int nref;
      const char* ref = cell_field<char>(fr, pl, pl.f_REF, lead, nref);
      put_spaces(s, 16); s.put('"'); s.write(names.text + names.off[pl.f_REF], names.off[pl.f_REF + 1] - names.off[pl.f_REF]); put_lit(s, "\": \""); s.write(ref, nref); put_lit(s, "\",\n");
      put_spaces(s, 16); s.put('"'); s.write(names.text + names.off[pl.f_ALT], names.off[pl.f_ALT + 1] - names.off[pl.f_ALT]); put_lit(s, "\": [ ");
      for (int j = 0; j + 1 < rm.num_merged; ++j) { if (j) s.put(','); var_put_alt_token(s, la, rm.merged_tok[j]); }
      put_lit(s, " ]");
    }
    s.put('\n'); put_spaces(s, 12); put_lit(s, "},\n");
    put_spaces(s, 12); put_lit(s, "\"variant_calls\": [\n");
  } else put_lit(s, ",\n");
  put_spaces(s, 16); put_lit(s, "{\n");
  put_spaces(s, 20); put_lit(s, "\"row\": "); put_i64(s, calls_array_row(fr, names, c)); put_lit(s, ",\n");
  var_put_intervals(s, qw, begin, end, 20, ", ");
  put_spaces(s, 20); put_lit(s, "\"fields\": {\n");
  bool none = true;
  for (int f = 0; f < pl.nfields; ++f) {
    if (!variants_field_valid(fr, pl, f, c)) continue;
    if (!none) put_lit(s, ",\n");
    put_spaces(s, 24); s.put('"'); s.write(names.text + names.off[f], names.off[f + 1] - names.off[f]); put_lit(s, "\": ");
    variants_put_field(s, fr, pl, f, c, multi ? &rm : nullptr, err);
    none = false;
  }
  s.put('\n'); put_spaces(s, 20); put_lit(s, "}\n"); put_spaces(s, 16); s.put('}');
  if (last) { s.put('\n'); put_spaces(s, 12); put_lit(s, "]\n"); put_spaces(s, 8); s.put('}'); }
}

}  // namespace genomicsdb_amd
