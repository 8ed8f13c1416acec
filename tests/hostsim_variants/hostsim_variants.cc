// hostsim_variants.cc - the variants query with the kernel bodies of core/gdb_variants.hpp on the host: the same selection, hashing,
// leader search and emitters the device runs, around std::stable_sort instead of rocPRIM.  Tests only.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_stages.hpp"
#include "../../genomicsdb_amd/csrc/core/gdb_variants.hpp"
#include "../../genomicsdb_amd/csrc/host/combine_plan.h"
#include "../../genomicsdb_amd/csrc/host/fragment.h"

using namespace genomicsdb_amd;

namespace {
FragmentView make_view(const HostFragment& fr) {
  FragmentView v;
  memset(&v, 0, sizeof(v));
  v.ncells = fr.ncells();
  v.row = fr.row.data(); v.begin = fr.begin.data(); v.end = fr.end.data();
  v.nmarkers = (int64_t)fr.marker_begin.size(); v.marker_begin = fr.marker_begin.data();
  for (size_t f = 0; f < fr.cols.size(); ++f) {
    v.col[f].data = fr.cols[f].data.data();
    v.col[f].off = fr.cols[f].var ? fr.cols[f].off.data() : nullptr;
  }
  return v;
}
}  // namespace

extern "C" {

int hostsim_query_variants(const char* query_json_text, const uint8_t* cells, uint64_t nbytes, char** out, uint64_t* out_len, char* errmsg, uint64_t errlen) {
  try {
    VariantQueryConfig qc;
    qc.read_from_json(mini_json::parse(query_json_text), 0, "");
    qc.do_query_bookkeeping(qc.get_vid_mapper().get_num_callsets(), 0);
    HostPlan hp = build_combine_plan(qc, "");
    HostFragment hf = fragment_from_cells(cells, nbytes, qc, hp);
    const CombinePlan& pl = hp.plan;
    for (int f = 0; f < pl.nfields; ++f) if (pl.field[f].ndim == 2) throw std::runtime_error("query_variants: 2-dimensional fields are not printed");
    const FragmentView fr = make_view(hf);
    const int64_t C = fr.ncells;
    uint32_t err = 0;
    std::vector<uint64_t> vmask(C); std::vector<uint32_t> cflags(C); std::vector<int32_t> dpval(C), k_lo(C), k_hi(C); std::vector<int64_t> eff_end(C);
    CellMeta cm{vmask.data(), cflags.data(), dpval.data(), eff_end.data(), k_lo.data(), k_hi.data()};
    for (int64_t c = 0; c < C; ++c) classify_cell(fr, pl, cm, c, &err);
    std::vector<int64_t> perm(C), rm_begin(C), span(C);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return fr.row[a] < fr.row[b]; });
    for (int64_t j = 0; j < C; ++j) stage_eff_end(fr, cm, perm.data(), j, rm_begin.data(), span.data(), &err);
    std::string names_text; std::vector<int32_t> names_off;
    for (const auto& nm : hp.field_names) { names_off.push_back((int32_t)names_text.size()); names_text += nm; }
    names_off.push_back((int32_t)names_text.size());
    std::vector<int64_t> q2a;
    { CellStreamLayout L(qc, hp); for (size_t r = 0; r < L.row_map.size(); ++r) if (L.row_map[r] >= 0) { if ((size_t)L.row_map[r] >= q2a.size()) q2a.resize((size_t)L.row_map[r] + 1, 0); q2a[(size_t)L.row_map[r]] = (int64_t)r; } }
    CallsNames names{names_text.data(), names_off.data(), q2a.empty() ? nullptr : q2a.data()};
    QueryWindow qw;
    memset(&qw, 0, sizeof(qw));
    qw.contigs = hp.contigs.data(); qw.ncontigs = (int32_t)hp.contigs.size(); qw.contig_names = hp.contig_names.data();
    std::vector<std::pair<int64_t, int64_t>> ivs;
    for (unsigned i = 0; i < qc.get_num_column_intervals(); ++i) ivs.emplace_back(qc.get_column_begin(i), qc.get_column_end(i));
    const bool whole = ivs.empty();
    if (whole) ivs.emplace_back(0, INT64_MAX - 1);
    const bool grouped = pl.f_REF >= 0 && pl.f_ALT >= 0;
    std::string body;
    for (const auto& iv : ivs) {
      std::vector<int64_t> call_cell, call_end;
      for (int64_t c = 0; c < C; ++c) { int64_t end; if (calls_select(fr, eff_end.data(), c, iv.first, iv.second, !whole, end)) { call_cell.push_back(c); call_end.push_back(end); } }
      const int64_t n = (int64_t)call_cell.size();
      std::vector<int64_t> leader(n), sorted(n), run_start(n), order(n);
      std::iota(leader.begin(), leader.end(), 0);
      if (grouped) {
        std::vector<uint64_t> h(n);
        for (int64_t i = 0; i < n; ++i) h[i] = var_call_hash(fr, pl, call_cell[i], call_end[i], &err);
        std::iota(sorted.begin(), sorted.end(), 0);
        std::stable_sort(sorted.begin(), sorted.end(), [&](int64_t a, int64_t b) { return h[a] < h[b]; });
        for (int64_t p = 0; p < n; ++p) run_start[p] = p > 0 && h[sorted[p]] == h[sorted[p - 1]] ? run_start[p - 1] : p;
        for (int64_t p = 0; p < n; ++p) leader[sorted[p]] = var_find_leader(fr, pl, call_cell.data(), call_end.data(), sorted.data(), run_start.data(), p);
      }
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return leader[a] < leader[b]; });
      for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order[k];
        const bool first = k == 0 || leader[order[k - 1]] != leader[i], last = k + 1 == n || leader[order[k + 1]] != leader[i];
        CountSink cs; variants_emit_call(cs, fr, pl, qw, names, call_cell[i], call_end[i], call_cell[leader[i]], first, last, &err);
        std::string t((size_t)cs.n, '\0');
        ByteSink bs(&t[0]); variants_emit_call(bs, fr, pl, qw, names, call_cell[i], call_end[i], call_cell[leader[i]], first, last, &err);
        body += t;
      }
    }
    if (err) throw std::runtime_error("device error bits " + std::to_string(err));
    std::string o = "{\n    \"variants\": [\n";
    if (!body.empty()) o.append(body, 2, std::string::npos);
    o += "\n    ]\n}\n";
    *out = (char*)malloc(o.size() + 1); memcpy(*out, o.data(), o.size()); *out_len = o.size();
    return 0;
  } catch (const std::exception& e) { snprintf(errmsg, errlen, "%s", e.what()); return 1; }
}
void hostsim_variants_free(char* p) { free(p); }

// the float emitter of the variants document: text of `v` as std::fixed << std::setprecision(6) prints it
int hostsim_put_float_fixed6(float v, char* buf, uint64_t cap) {
  CountSink cs; put_float_fixed6(cs, v);
  if (cs.n + 1 > cap) return -1;
  ByteSink bs(buf); put_float_fixed6(bs, v);
  buf[cs.n] = 0;
  return (int)cs.n;
}
// many at once: texts joined by '\n' (each at most 63 bytes); returns the length
int64_t hostsim_put_float_fixed6_many(const float* v, int64_t n, char* buf, uint64_t cap) {
  uint64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (at + 64 > cap) return -1;
    ByteSink bs(buf + at); put_float_fixed6(bs, v[i]);
    at = (uint64_t)(bs.p - buf);
    buf[at++] = '\n';
  }
  return (int64_t)at;
}
}
