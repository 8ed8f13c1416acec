// hostsim_vcfdiff - the bodies of the device vcfdiff (csrc/core/gdb_vcfdiff.hpp) on the CPU, with the host's share of the tool
// (csrc/host/vcfdiff_common.hpp): what kernels/gdb_vcfdiff.hip does with two files, without a device.  Built with the address and
// undefined-behaviour sanitizers; tests/test_vcfdiff_bodies_cpu.py compares its report with the plain-Python model.
//   hostsim_vcfdiff [-t threshold] [-r regions] <gold> <test>
// stdout: {"report": <the report>, "pairs_light": n, "pairs_heavy": n, "deferred": n}; an error: its words on stderr, exit 1.
// A pair takes the path the device gives it: vd_sample<VdLane> (light) or vd_sample<VdSerialCoop>, the cooperative path with a
// wavefront of one lane.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/host/vcfdiff_common.hpp"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbvdiff;
using namespace genomicsdb_amd::vdhost;

static std::string read_all(const std::string& path) {
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) throw VCFDiffException("cannot open " + path);
  std::string out;
  std::vector<char> buf(1 << 16);
  int n;
  while ((n = gzread(f, buf.data(), (unsigned)buf.size())) > 0) out.append(buf.data(), (size_t)n);
  gzclose(f);
  return out;
}

struct HostFile {
  std::string text;
  size_t record_begin = 0;
  int64_t lines_before = 0;
  std::vector<uint32_t> tabs;
  std::vector<VdRecord> lines;
  gdbimp::ImpLine line(const VdRecord& r) const {
    gdbimp::ImpLine L; L.text = text.data(); L.begin = r.key.begin; L.end = r.key.stop; L.tabs = tabs.data() + r.key.tab_first; L.ntabs = r.key.ntabs;
    return L;
  }
};

static void load(HostFile& F, const std::string& path) {
  F.text = read_all(path);
  if (F.text.size() >= 5 && F.text.compare(0, 4, "BCF\2") == 0) throw VCFDiffException(path + " is BCF2: vcfdiff reads VCF text only (plain, gzip or BGZF) in this build");
  if (!F.text.empty() && F.text.back() != '\n') F.text += '\n';
  size_t pos = 0;
  while (pos < F.text.size()) {
    const size_t eol = F.text.find('\n', pos);
    size_t ln = eol - pos;
    if (ln && F.text[eol - 1] == '\r') --ln;
    if (ln && F.text[pos] != '#') break;
    pos = eol + 1;
    ++F.lines_before;
  }
  F.record_begin = pos;
}

int main(int argc, char** argv) {
  double threshold = 1e-5;
  std::string regions;
  int at = 1;
  while (at + 1 < argc && argv[at][0] == '-') {
    if (std::string(argv[at]) == "-t") threshold = strtod(argv[at + 1], nullptr);
    else if (std::string(argv[at]) == "-r") regions = argv[at + 1];
    else break;
    at += 2;
  }
  if (at + 2 > argc) { std::cerr << "hostsim_vcfdiff [-t threshold] [-r regions] <gold> <test>\n"; return 2; }
  const std::string path[2] = {argv[at], argv[at + 1]};
  try {
    HostFile F[2];
    for (int f = 0; f < 2; ++f) load(F[f], path[f]);
    const VdHeader gh = vd_parse_header(F[0].text.substr(0, F[0].record_begin)), th = vd_parse_header(F[1].text.substr(0, F[1].record_begin));
    const VdTablesHost H = vd_build_tables(gh, th);
    const VdTables T = H.view(threshold);
    std::vector<VdRecord> recs[2];
    for (int f = 0; f < 2; ++f) {
      HostFile& X = F[f];
      int64_t line_no = X.lines_before;
      for (size_t pos = X.record_begin; pos < X.text.size();) {
        const size_t eol = X.text.find('\n', pos);
        size_t end = eol;
        if (end > pos && X.text[end - 1] == '\r') --end;
        const uint32_t first = (uint32_t)X.tabs.size();
        for (size_t i = pos; i < end; ++i) if (X.text[i] == '\t') X.tabs.push_back((uint32_t)i);
        gdbimp::ImpLine L; L.text = X.text.data(); L.begin = (uint32_t)pos; L.end = (uint32_t)end; L.tabs = X.tabs.data() + first; L.ntabs = (uint32_t)X.tabs.size() - first;
        VdRecord r; r.key = vd_keys(T, f, L); r.key.tab_first = first; r.line_no = ++line_no; r.batch = 0;
        X.lines.push_back(r);
        pos = eol + 1;
      }
      recs[f] = vd_records(path[f], X.lines, H, f, regions, [&](size_t i) { return X.text.substr(X.lines[i].key.begin, X.lines[i].key.stop - X.lines[i].key.begin); });
    }
    std::vector<VdEvent> events = vd_walk(recs[0], recs[1], H);
    std::vector<VdDeferred> def(1 << 20);
    uint32_t ndef = 0;
    int64_t light = 0, heavy = 0;
    std::vector<uint32_t> goffs(4096), toffs(4096);
    std::vector<size_t> of_pair;
    for (size_t k = 0; k < events.size(); ++k) {
      VdEvent& e = events[k];
      if (e.pair < 0) continue;
      of_pair.push_back(k);
      const VdRecord& g = recs[0][(size_t)e.g]; const VdRecord& t = recs[1][(size_t)e.t];
      const gdbimp::ImpLine G = F[0].line(g), Tt = F[1].line(t);
      const VdDefer D{def.data(), &ndef, (uint32_t)def.size(), (uint32_t)e.pair, true};
      VdSite S;
      vd_site(T, G, Tt, g.key.pos == t.key.pos, D, S);
      e.flags = S.flags;
      for (int m = 0; m < 4; ++m) e.info[m] = S.info[m];
      const bool is_heavy = vd_is_heavy(S);
      if (is_heavy) ++heavy; else ++light;
      for (int32_t j = 0; j < T.n_samples; ++j) {
        const VdMasks M = is_heavy ? vd_sample(VdSerialCoop(), T, G, Tt, S, (uint32_t)j, D, goffs.data(), toffs.data(), (uint32_t)goffs.size())
                                   : vd_sample(VdLane(), T, G, Tt, S, (uint32_t)j, D, nullptr, nullptr, 0u);
        for (int m = 0; m < 4; ++m) e.fmt[m] |= M.m[m];
      }
    }
    if (ndef > def.size()) throw VCFDiffException("hostsim: more deferred tokens than the list holds");
    for (uint32_t i = 0; i < ndef; ++i)
      if (vd_deferred_differs(std::string(def[i].a, def[i].an), std::string(def[i].b, def[i].bn), threshold)) vd_apply_deferred(events[of_pair[def[i].pair]], def[i].what);
    std::vector<VdEventText> text(events.size());
    for (size_t k = 0; k < events.size(); ++k) {
      const VdEvent& e = events[k];
      if (!vd_event_listed(e)) continue;
      if (e.g >= 0) { const VdKey& K = recs[0][(size_t)e.g].key; text[k].gold = F[0].text.substr(K.begin, K.stop - K.begin); }
      if (e.t >= 0) { const VdKey& K = recs[1][(size_t)e.t].key; text[k].test = F[1].text.substr(K.begin, K.stop - K.begin); }
    }
    std::cout << "{\"report\": " << vd_report_json(events, text, recs[0], recs[1], H) << ", \"pairs_light\": " << light << ", \"pairs_heavy\": " << heavy
              << ", \"deferred\": " << ndef << "}\n";
  } catch (const std::exception& e) {
    std::cerr << e.what() << "\n";
    return 1;
  }
  return 0;
}
