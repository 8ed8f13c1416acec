// tests/hostsim_numtext/hostsim_numtext.cc - CPU harness around the number-text bodies of csrc/core/gdb_core.hpp (put_i64, put_u32,
// put_float), the single-pass ALT token iterator (AltTokens, against alt_token(idx)) and the first-cell table of the site pass
// (stage_first_cell in csrc/core/gdb_stages.hpp, against the binary search of site_first_ref).  Built twice: as a shared library for
// the Python tests, and with -DHOSTSIM_NUMTEXT_MAIN as a stand-alone program under the address and undefined-behaviour sanitizers
// that runs the same comparisons against the C library.  Test infrastructure only.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_stages.hpp"

namespace {

// the first-cell answer of site_first_ref for every record, with the table (use_table) or with the search: the REF's offset in the
// REF column (-1: null) and its length
void first_ref_all(const int64_t* begin, int64_t ncells, const uint8_t* ref_valid, const uint32_t* ref_off, const char* ref_data, const int64_t* rstart,
                   int64_t P, int64_t qb, int64_t qe, int use_table, int use_first_record_at, int64_t* table_out, int64_t* ref_at, int32_t* ref_len) {
  SiteCtx* cx = new SiteCtx();
  memset((void*)cx, 0, sizeof(SiteCtx));
  std::vector<uint64_t> vmask((size_t)ncells + 1, 0);
  for (int64_t c = 0; c < ncells; ++c) vmask[(size_t)c] = ref_valid[c] ? 1ull : 0ull;
  cx->fr.ncells = ncells;
  cx->fr.begin = begin;
  cx->fr.col[0].data = ref_data;
  cx->fr.col[0].off = ref_off;
  cx->pl.nfields = 1;
  cx->pl.f_REF = 0;
  cx->cm.vmask = vmask.data();
  RecordTable rec{P, rstart, rstart};
  cx->rec = rec;
  std::vector<int64_t> table((size_t)P + 1, -1);
  std::vector<int32_t> fra;
  if (use_table) {
    if (use_first_record_at) {             // entry p = first record whose start is >= qb + p (P if none), as the pipeline builds it
      const int64_t W = qe - qb + 2;
      fra.assign((size_t)W, (int32_t)P);
      for (int64_t k = 0; k < P; ++k) fra[(size_t)(rstart[k] - qb)] = (int32_t)k;
      for (int64_t p = W - 2; p >= 0; --p) if (fra[(size_t)p + 1] < fra[(size_t)p]) fra[(size_t)p] = fra[(size_t)p + 1];
    }
    for (int64_t c = 0; c < ncells; ++c) stage_first_cell(cx->fr, rec, c, qb, qe, use_first_record_at ? fra.data() : nullptr, table.data());
    cx->first_cell_at = table.data();
  }
  for (int64_t k = 0; k < P; ++k) {
    int len = -7;
    const char* r = site_first_ref(*cx, k, rstart[k], len);
    ref_at[k] = r ? (int64_t)(r - ref_data) : -1;
    ref_len[k] = len;
    if (table_out) table_out[k] = table[(size_t)k];
  }
  delete cx;
}

int alt_by_iterator(const char* s, int len, int32_t* off, int32_t* tlen, int cap) {
  const char* tok; int tl, n = 0;
  for (AltTokens at(s, len); at.next(tok, tl);) {
    if (at.idx != n) return -1;
    if (n < cap) { off[n] = (int32_t)(tok - s); tlen[n] = tl; }
    ++n;
  }
  return n;
}
int alt_by_index(const char* s, int len, int32_t* off, int32_t* tlen, int cap) {
  const char* tok; int tl, n = 0;
  for (int i = 0; alt_token(s, len, i, tok, tl); ++i) {
    if (n < cap) { off[n] = (int32_t)(tok - s); tlen[n] = tl; }
    ++n;
  }
  return n;
}

}  // namespace

extern "C" {

int hostsim_numtext_put_i64(int64_t v, char* out) { ByteSink s(out); put_i64(s, v); return (int)s.pos(); }
int hostsim_numtext_put_u32(uint32_t v, char* out) { ByteSink s(out); put_u32(s, v); return (int)s.pos(); }
int hostsim_numtext_put_float(uint32_t bits, char* out) { ByteSink s(out); union { uint32_t u; float f; } x; x.u = bits; put_float(s, x.f); return (int)s.pos(); }
// n values, each followed by '\n' (out: 22 bytes per value are enough); returns the bytes written.  CountSink has to agree.
int64_t hostsim_numtext_put_i64_many(const int64_t* v, int64_t n, char* out) {
  ByteSink s(out);
  for (int64_t i = 0; i < n; ++i) {
    char* before = s.p;
    put_i64(s, v[i]);
    CountSink cs; put_i64(cs, v[i]);
    if ((int64_t)cs.n != (int64_t)(s.p - before)) return -1;
    s.put('\n');
  }
  return (int64_t)(s.p - out);
}
int hostsim_numtext_alt_iterator(const char* s, int len, int32_t* off, int32_t* tlen, int cap) { return alt_by_iterator(s, len, off, tlen, cap); }
int hostsim_numtext_alt_indexed(const char* s, int len, int32_t* off, int32_t* tlen, int cap) { return alt_by_index(s, len, off, tlen, cap); }
void hostsim_numtext_first_ref(const int64_t* begin, int64_t ncells, const uint8_t* ref_valid, const uint32_t* ref_off, const char* ref_data, const int64_t* rstart,
                               int64_t P, int64_t qb, int64_t qe, int use_table, int use_first_record_at, int64_t* table_out, int64_t* ref_at, int32_t* ref_len) {
  first_ref_all(begin, ncells, ref_valid, ref_off, ref_data, rstart, P, qb, qe, use_table, use_first_record_at, table_out, ref_at, ref_len);
}

}  // extern "C"

#ifdef HOSTSIM_NUMTEXT_MAIN
namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
int g_bad = 0;
void fail(const char* what, const std::string& a, const std::string& b) { if (++g_bad <= 20) printf("MISMATCH %s: got '%s' want '%s'\n", what, a.c_str(), b.c_str()); }

void check_i64(int64_t v) {
  char got[32], want[32];
  const int n = hostsim_numtext_put_i64(v, got);
  got[n] = 0;
  snprintf(want, sizeof want, "%" PRId64, v);
  if (strcmp(got, want)) fail("put_i64", got, want);
}
void check_u32(uint32_t v) {
  char got[32], want[32];
  const int n = hostsim_numtext_put_u32(v, got);
  got[n] = 0;
  snprintf(want, sizeof want, "%" PRIu32, v);
  if (strcmp(got, want)) fail("put_u32", got, want);
}
void check_alt(const std::string& s) {
  int32_t o1[64], l1[64], o2[64], l2[64];
  // an exact-size heap copy, so that a read past the end is seen
  char* p = (char*)malloc(s.size() ? s.size() : 1);
  memcpy(p, s.data(), s.size());
  const int n1 = alt_by_iterator(p, (int)s.size(), o1, l1, 64), n2 = alt_by_index(p, (int)s.size(), o2, l2, 64);
  bool same = n1 == n2;
  for (int i = 0; same && i < n1 && i < 64; ++i) same = o1[i] == o2[i] && l1[i] == l2[i];
  if (!same) fail("alt tokens", s, std::to_string(n1) + " vs " + std::to_string(n2));
  free(p);
}
void check_first_cell(int round) {
  const int64_t qb = 1000 + (int64_t)(rnd() % 50), W = 40 + (int64_t)(rnd() % 60), qe = qb + W - 1;
  const int ncells = (int)(rnd() % 80);
  std::vector<int64_t> begin;
  int64_t pos = qb - 20;
  for (int c = 0; c < ncells; ++c) { if (rnd() % 3) pos += (int64_t)(rnd() % 5); begin.push_back(pos); }   // runs of equal begin; some before qb, some behind qe
  std::vector<uint8_t> valid; std::vector<uint32_t> off(1, 0); std::string data;
  for (int c = 0; c < ncells; ++c) { valid.push_back(rnd() % 4 != 0); const int n = 1 + (int)(rnd() % 3); data.append((size_t)n, "ACGT"[rnd() % 4]); off.push_back((uint32_t)data.size()); }
  std::vector<int64_t> rstart;
  for (int64_t p = qb; p <= qe; ++p) if (rnd() % 2 || p == qb || p == qe) rstart.push_back(p);
  if (round % 7 == 0 && rstart.size() > 2) { rstart.erase(rstart.begin()); rstart.pop_back(); }
  const int64_t P = (int64_t)rstart.size();
  std::vector<int64_t> a0((size_t)P + 1), a1((size_t)P + 1), a2((size_t)P + 1);
  std::vector<int32_t> l0((size_t)P + 1), l1((size_t)P + 1), l2((size_t)P + 1);
  const int64_t* bp = begin.empty() ? nullptr : begin.data();
  first_ref_all(bp, ncells, valid.data(), off.data(), data.data(), rstart.data(), P, qb, qe, 0, 0, nullptr, a0.data(), l0.data());
  first_ref_all(bp, ncells, valid.data(), off.data(), data.data(), rstart.data(), P, qb, qe, 1, 1, nullptr, a1.data(), l1.data());
  first_ref_all(bp, ncells, valid.data(), off.data(), data.data(), rstart.data(), P, qb, qe, 1, 0, nullptr, a2.data(), l2.data());
  for (int64_t k = 0; k < P; ++k)
    if (a0[k] != a1[k] || l0[k] != l1[k] || a0[k] != a2[k] || l0[k] != l2[k]) fail("first cell", std::to_string(a1[k]) + "/" + std::to_string(a2[k]), std::to_string(a0[k]));
}
}  // namespace

int main() {
  const int64_t edge[] = {0, 1, -1, 9, 10, 99, 100, 99999999, 100000000, 100000001, 2147483647ll, 4294967295ll, 4294967296ll, 9999999999999999ll, 10000000000000000ll,
                          INT64_MAX, INT64_MIN, INT64_MIN + 1, -4294967296ll, -100000000};
  for (int64_t v : edge) check_i64(v);
  uint64_t lo = 1;
  for (int d = 1; d <= 19; ++d) {                      // 10^5 values of every digit count, both signs
    const uint64_t hi = d == 19 ? (uint64_t)INT64_MAX : lo * 10 - 1;
    for (int i = 0; i < 100000; ++i) { const int64_t v = (int64_t)(lo + rnd() % (hi - lo + 1)); check_i64(i & 1 ? -v : v); }
    lo *= 10;
  }
  const uint32_t uedge[] = {0u, 9u, 10u, 99u, 100u, 99999999u, 100000000u, 999999999u, 1000000000u, 4294967295u};
  for (uint32_t v : uedge) check_u32(v);
  for (int i = 0; i < 1000000; ++i) check_u32((uint32_t)rnd() >> (rnd() % 32));
  const char* alts[] = {"", "|", "A", "A|", "|A", "A||C", "&", "A|&", "||"};
  for (const char* a : alts) check_alt(a);
  for (int i = 0; i < 10000; ++i) {
    std::string s;
    const int n = (int)(rnd() % 24);
    for (int j = 0; j < n; ++j) s.push_back("AC|&*<>"[rnd() % 7]);
    check_alt(s);
  }
  for (int r = 0; r < 2000; ++r) check_first_cell(r);
  // the float text over every sink: the counted length is the written one (the bytes themselves are held to the C library by the Python test)
  for (int i = 0; i < 1000000; ++i) {
    char buf[64];
    const uint32_t bits = (uint32_t)rnd();
    const int n = hostsim_numtext_put_float(bits, buf);
    union { uint32_t u; float f; } x; x.u = bits;
    CountSink cs; put_float(cs, x.f);
    if ((int)cs.n != n || n <= 0 || n > 40) fail("put_float length", std::to_string(n), std::to_string(cs.n));
  }
  printf("%s: %d mismatches\n", g_bad ? "FAILED" : "ok", g_bad);
  return g_bad ? 1 : 0;
}
#endif
