// vcfdiff_common.hpp - the host's share of the device vcfdiff (kernels/gdb_vcfdiff.hip), without HIP types so that the CPU harness of the
// bodies (tests/hostsim_vcfdiff) runs the very same code: the three things read from a header, the field tables the bodies of
// core/gdb_vcfdiff.hpp read, the refusals, the regions, the errors of a file's lines, the walk over the keys, the deferred floats and
// the report.  The rule is written out in DESIGN.md ("Comparing two VCFs").
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../core/gdb_vcfdiff.hpp"

namespace genomicsdb_amd {

class VCFDiffException : public std::runtime_error {
 public:
  explicit VCFDiffException(const std::string& m) : std::runtime_error("VCFDiffException : " + m) {}
};

namespace vdhost {
using namespace gdbvdiff;

struct VdFieldDef { std::string id, number, type; };
struct VdHeader {
  std::vector<std::string> contigs, filters, samples;
  std::vector<VdFieldDef> info, fmt;      // in the order of first declaration; a later line of the same ID replaces Number and Type
};

// ID=..,Number=..,Type=..,Description=".." at the top level of <...>
inline std::map<std::string, std::string> vd_attrs(const std::string& body) {
  std::map<std::string, std::string> out;
  std::string key, val;
  bool in_q = false, on_val = false;
  for (size_t i = 0; i <= body.size(); ++i) {
    const char c = i < body.size() ? body[i] : ',';
    if (c == '"') { in_q = !in_q; val += c; }
    else if (c == ',' && !in_q) { if (!key.empty()) out[key] = val; key.clear(); val.clear(); on_val = false; }
    else if (c == '=' && !on_val && !in_q) on_val = true;
    else if (on_val) val += c;
    else key += c;
  }
  return out;
}

inline VdHeader vd_parse_header(const std::string& head) {
  VdHeader h;
  size_t pos = 0;
  while (pos < head.size()) {
    size_t eol = head.find('\n', pos);
    if (eol == std::string::npos) eol = head.size();
    std::string line = head.substr(pos, eol - pos);
    pos = eol + 1;
    while (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.compare(0, 6, "#CHROM") == 0) {
      h.samples.clear();
      size_t b = 0; int col = 0;
      for (size_t i = 0; i <= line.size(); ++i) if (i == line.size() || line[i] == '\t') { if (col >= 9) h.samples.push_back(line.substr(b, i - b)); b = i + 1; ++col; }
      continue;
    }
    int what = -1;
    size_t open = 0;
    const char* tags[4] = {"##contig=<", "##INFO=<", "##FORMAT=<", "##FILTER=<"};
    for (int k = 0; k < 4; ++k) if (line.compare(0, strlen(tags[k]), tags[k]) == 0) { what = k; open = strlen(tags[k]); }
    while (!line.empty() && (line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (what < 0 || line.empty() || line.back() != '>') continue;
    const std::map<std::string, std::string> a = vd_attrs(line.substr(open, line.size() - 1 - open));
    if (!a.count("ID")) continue;
    const std::string& id = a.at("ID");
    if (what == 0) { if (std::find(h.contigs.begin(), h.contigs.end(), id) == h.contigs.end()) h.contigs.push_back(id); }
    else if (what == 3) h.filters.push_back(id);
    else {
      std::vector<VdFieldDef>& defs = what == 1 ? h.info : h.fmt;
      VdFieldDef d; d.id = id; d.number = a.count("Number") ? a.at("Number") : "."; d.type = a.count("Type") ? a.at("Type") : "String";
      bool seen = false;
      for (VdFieldDef& e : defs) if (e.id == id) { e = d; seen = true; }
      if (!seen) defs.push_back(d);
    }
  }
  return h;
}

struct VdTablesHost {
  std::string names;
  std::vector<VdName> contigs[2];
  std::vector<VdField> info, fmt;
  std::vector<std::string> info_names, fmt_names, order;      // order: the contigs in the order of work
  int n_common = 0;                                           // the first n_common of `order` are in both headers
  std::vector<int> only;                                      // per contig of `order`: -1 both, 0 only gold, 1 only test
  std::vector<int32_t> sample_map;
  uint32_t add_name(const std::string& s) { const uint32_t off = (uint32_t)names.size(); names += s; return off; }
  VdTables view(double threshold) const {
    VdTables T;
    T.names = names.data();
    for (int f = 0; f < 2; ++f) { T.contigs[f] = contigs[f].data(); T.n_contigs[f] = (int32_t)contigs[f].size(); }
    T.info = info.data(); T.fmt = fmt.data(); T.n_info = (int32_t)info.size(); T.n_fmt = (int32_t)fmt.size();
    T.sample_map = sample_map.data(); T.n_samples = (int32_t)sample_map.size(); T.threshold = threshold;
    return T;
  }
};

inline bool vd_known_name(const std::string& n, int* cls) {      // known_field_info.cc:42-71 and :239-283
  static const char* known[] = {"END", "REF", "ALT", "QUAL", "FILTER", "BaseQRankSum", "ClippingRankSum", "MQRankSum", "ReadPosRankSum", "DP", "MQ", "RAW_MQ", "MQ0", "DP_FORMAT",
                                "MIN_DP", "GQ", "SB", "AD", "PL", "AF", "AN", "AC", "GT", "PS", "PGT", "PID", "ExcessHet", "ID"};
  for (const char* k : known)
    if (n == k) {
      *cls = (n == "AF" || n == "AC") ? VD_C_A : n == "AD" ? VD_C_R : n == "PL" ? VD_C_G : n == "GT" ? VD_C_GT : VD_C_IDENTITY;
      return true;
    }
  return false;
}

inline void vd_field_table(VdTablesHost& H, const std::vector<VdFieldDef>& gold, const std::vector<VdFieldDef>& test, const char* what, std::vector<VdField>& out,
                           std::vector<std::string>& out_names) {
  auto find = [](const std::vector<VdFieldDef>& defs, const std::string& id) -> const VdFieldDef* { for (const VdFieldDef& d : defs) if (d.id == id) return &d; return nullptr; };
  std::vector<std::string> names;
  for (const VdFieldDef& d : gold) names.push_back(d.id);
  for (const VdFieldDef& d : test) if (!find(gold, d.id)) names.push_back(d.id);
  if (names.size() > kVdMaxFields)
    throw VCFDiffException("more than 64 distinct " + std::string(what) + " names in the two headers (" + std::to_string(names.size()) + "): the result masks are 64 bits wide");
  for (const std::string& n : names) {
    const VdFieldDef* g = find(gold, n); const VdFieldDef* t = find(test, n);
    const VdFieldDef* d = g ? g : t;
    VdField f; memset(&f, 0, sizeof(f));
    f.off = H.add_name(n); f.len = (uint32_t)n.size();
    f.type = d->type == "Integer" ? VD_T_INT : d->type == "Float" ? VD_T_FLOAT : d->type == "Flag" ? VD_T_FLAG : VD_T_STR;
    int cls = VD_C_IDENTITY;
    if (!vd_known_name(n, &cls)) {
      cls = d->number == "A" ? VD_C_A : d->number == "R" ? VD_C_R : d->number == "G" ? VD_C_G : VD_C_IDENTITY;
      if (g && t && g->number != t->number) f.flags |= VD_F_NUMBER_DIFFERS;
    }
    f.cls = (uint8_t)cls;
    if (g) f.flags |= VD_F_IN_GOLD;
    if (t) f.flags |= VD_F_IN_TEST;
    if (g && t && g->type != t->type) f.flags |= VD_F_TYPE_DIFFERS;
    out.push_back(f); out_names.push_back(n);
  }
}

// the refusals that need both headers, then the tables
inline VdTablesHost vd_build_tables(const VdHeader& gh, const VdHeader& th) {
  for (const VdHeader* h : {&gh, &th}) {
    std::vector<std::string> s = h->samples;
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) throw VCFDiffException("duplicate sample name in a file header");
  }
  {
    std::vector<std::string> a = gh.samples, b = th.samples;
    std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
    if (a != b) throw VCFDiffException("Sample names in the 2 file headers are different - cannot perform any further comparisons");
  }
  VdTablesHost H;
  vd_field_table(H, gh.info, th.info, "INFO", H.info, H.info_names);
  vd_field_table(H, gh.fmt, th.fmt, "FORMAT", H.fmt, H.fmt_names);
  for (const std::string& s : gh.samples) H.sample_map.push_back((int32_t)(std::find(th.samples.begin(), th.samples.end(), s) - th.samples.begin()));
  auto has = [](const std::vector<std::string>& v, const std::string& s) { return std::find(v.begin(), v.end(), s) != v.end(); };
  for (const std::string& c : gh.contigs) if (has(th.contigs, c)) H.order.push_back(c);
  std::sort(H.order.begin(), H.order.end());      // byte order (:801)
  H.n_common = (int)H.order.size();
  H.only.assign(H.order.size(), -1);
  for (const std::string& c : gh.contigs) if (!has(th.contigs, c)) { H.order.push_back(c); H.only.push_back(0); }
  for (const std::string& c : th.contigs) if (!has(gh.contigs, c)) { H.order.push_back(c); H.only.push_back(1); }
  for (int f = 0; f < 2; ++f)
    for (const std::string& c : (f ? th : gh).contigs) {
      VdName n; n.off = H.add_name(c); n.len = (uint32_t)c.size();
      n.value = (int32_t)(std::find(H.order.begin(), H.order.end(), c) - H.order.begin());
      H.contigs[f].push_back(n);
    }
  return H;
}

// chr | chr:pos | chr:from-to | chr:from- , comma separated; the first entry per contig counts (:807-848) -> 0-based, inclusive
inline std::map<std::string, std::pair<int64_t, int64_t>> vd_parse_regions(const std::string& regions) {
  std::map<std::string, std::pair<int64_t, int64_t>> out;
  size_t b = 0;
  for (size_t i = 0; i <= regions.size(); ++i) {
    if (i < regions.size() && regions[i] != ',') continue;
    const std::string entry = regions.substr(b, i - b);
    b = i + 1;
    if (entry.empty()) continue;
    std::string name = entry;
    int64_t lo = 0, hi = (int64_t)1 << 62;
    const size_t c = entry.rfind(':');
    if (c != std::string::npos && c > 0) {
      const std::string r = entry.substr(c + 1);
      size_t d = 0;
      while (d < r.size() && r[d] >= '0' && r[d] <= '9') ++d;
      bool ok = d > 0 && d <= 18;
      size_t d2 = d;
      if (ok && d < r.size()) { ok = r[d] == '-'; d2 = d + 1; while (d2 < r.size() && r[d2] >= '0' && r[d2] <= '9') ++d2; ok = ok && d2 == r.size() && d2 - d - 1 <= 18; }
      if (ok) {
        name = entry.substr(0, c);
        lo = strtoll(r.substr(0, d).c_str(), nullptr, 10) - 1;
        hi = d == r.size() ? lo : (d + 1 < r.size() ? strtoll(r.substr(d + 1).c_str(), nullptr, 10) - 1 : (int64_t)1 << 62);
      }
    }
    if (!out.count(name)) out[name] = std::make_pair(lo, hi);
  }
  return out;
}

struct VdRecord { VdKey key; int64_t line_no; uint32_t batch; };      // a record line of a file; batch: which resident batch holds it

// the errors of a file's lines, the first offending line speaks (a line's own error before the order of the contigs); keeps the record
// lines, and of them those inside the regions.  line_text(i) fetches line i of `lines` for a message that names a key
inline std::vector<VdRecord> vd_records(const std::string& path, const std::vector<VdRecord>& lines, const VdTablesHost& H, int file, const std::string& regions,
                                        const std::function<std::string(size_t)>& line_text) {
  const auto R = vd_parse_regions(regions);
  std::vector<VdRecord> out;
  std::vector<char> seen(H.order.size(), 0);
  const VdRecord* cur = nullptr;
  for (size_t i = 0; i < lines.size(); ++i) {
    const VdRecord& r = lines[i];
    if (!(r.key.bits & VD_KEY_RECORD)) continue;
    const std::string where = path + " line " + std::to_string(r.line_no);
    const uint32_t err = r.key.bits & VD_ERR_MASK;
    if (err) {
      if (err & VD_ERR_SHORT) throw VCFDiffException("short record line in " + where);
      const std::string text = line_text(i);
      std::vector<std::string> cols;
      { size_t s = 0; for (size_t k = 0; k <= text.size(); ++k) if (k == text.size() || text[k] == '\t') { cols.push_back(text.substr(s, k - s)); s = k + 1; } }
      auto undeclared = [&](const std::string& col, char sep, const std::vector<VdField>& fields, const std::vector<std::string>& names, bool info) {
        size_t s = 0;
        for (size_t k = 0; k <= col.size(); ++k) {
          if (k < col.size() && col[k] != sep) continue;
          std::string key = col.substr(s, k - s);
          s = k + 1;
          if (info) key = key.substr(0, key.find('='));
          if (info && key == "END") continue;
          bool ok = false;
          for (size_t f = 0; f < names.size(); ++f) ok = ok || (names[f] == key && (fields[f].flags & (file ? VD_F_IN_TEST : VD_F_IN_GOLD)));
          if (!ok) return key;
        }
        return std::string();
      };
      if (err & VD_ERR_CONTIG) throw VCFDiffException("contig " + cols.at(0) + " is not in the header of its file (" + where + ")");
      if (err & VD_ERR_COORD) throw VCFDiffException("POS / END not in plain decimal form (" + where + ")");
      if (err & VD_ERR_INFO_KEY) throw VCFDiffException("INFO key " + undeclared(cols.at(7), ';', H.info, H.info_names, true) + " is not declared in the header (" + where + ")");
      if (err & VD_ERR_NKEYS) throw VCFDiffException("more than 64 FORMAT keys on a line (" + where + ")");
      if (err & VD_ERR_FMT_KEY) throw VCFDiffException("FORMAT key " + undeclared(cols.at(8), ':', H.fmt, H.fmt_names, false) + " is not declared in the header (" + where + ")");
      throw VCFDiffException("more than 255 alleles on a line (" + where + ")");
    }
    const std::string& contig = H.order.at((size_t)r.key.contig);
    if (!cur || cur->key.contig != r.key.contig) {
      if (seen[(size_t)r.key.contig]) throw VCFDiffException("the records of contig " + contig + " are not contiguous (" + where + ")");
      seen[(size_t)r.key.contig] = 1;
    } else if (r.key.pos < cur->key.pos) throw VCFDiffException("POS goes back within contig " + contig + " (" + where + ")");
    cur = &r;
    if (!regions.empty()) {
      const auto it = R.find(contig);
      if (it == R.end() || r.key.pos > it->second.second || r.key.end < it->second.first) continue;
    }
    out.push_back(r);
  }
  return out;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
enum { VD_EV_COMPARED = 0, VD_EV_REF_BLOCKS_OVERLAP = 1, VD_EV_DIFFERENT_POSITIONS = 2, VD_EV_EXTRA_LINES = 3 };
struct VdEvent {
  int kind; int64_t g, t;       // indices into the kept records of gold / test, -1: none
  int64_t pair;                 // index among the compared pairs, -1: not compared
  uint32_t flags; uint64_t info[4], fmt[4];
};

inline std::vector<VdEvent> vd_walk(const std::vector<VdRecord>& gold, const std::vector<VdRecord>& test, const VdTablesHost& H) {
  std::vector<VdEvent> ev;
  int64_t n_pairs = 0;
  auto add = [&](int kind, int64_t g, int64_t t) {
    VdEvent e; memset(&e, 0, sizeof(e));
    e.kind = kind; e.g = g; e.t = t; e.pair = (kind == VD_EV_COMPARED || kind == VD_EV_REF_BLOCKS_OVERLAP) ? n_pairs++ : -1;
    ev.push_back(e);
  };
  // the records of one contig are contiguous in a file: [first, last) per contig
  auto ranges = [&](const std::vector<VdRecord>& r) {
    std::vector<std::pair<int64_t, int64_t>> out(H.order.size(), std::make_pair((int64_t)0, (int64_t)0));
    for (size_t i = 0; i < r.size(); ++i) {
      auto& p = out[(size_t)r[i].key.contig];
      if (p.second == p.first) p.first = (int64_t)i;
      p.second = (int64_t)i + 1;
    }
    return out;
  };
  const auto gr = ranges(gold), tr = ranges(test);
  for (size_t c = 0; c < H.order.size(); ++c) {
    int64_t i = gr[c].first, j = tr[c].first;
    const int64_t ie = gr[c].second, je = tr[c].second;
    while (i < ie && j < je) {
      const VdKey& g = gold[(size_t)i].key; const VdKey& t = test[(size_t)j].key;
      const bool overlap = g.pos <= t.end && t.pos <= g.end;
      if (g.pos == t.pos && g.end == t.end) { add(VD_EV_COMPARED, i, j); ++i; ++j; }
      else if ((g.bits & VD_KEY_REFBLOCK) && (t.bits & VD_KEY_REFBLOCK) && overlap) {
        add(VD_EV_REF_BLOCKS_OVERLAP, i, j);
        const bool ag = g.end <= t.end, at = t.end <= g.end;      // the smaller end, both when equal (:1222-1236)
        if (ag) ++i;
        if (at) ++j;
      } else {
        add(VD_EV_DIFFERENT_POSITIONS, i, j);
        if (!overlap) {      // the file with the smaller pos seeks to the other's pos
          if (g.pos < t.pos) { while (i < ie && gold[(size_t)i].key.end < t.pos) ++i; }
          else { while (j < je && test[(size_t)j].key.end < g.pos) ++j; }
        } else if (t.end > g.end) { if ((t.bits & VD_KEY_LONG_REF) && t.pos <= g.pos) ++j; else ++i; }
        else if (g.end > t.end) { if ((g.bits & VD_KEY_LONG_REF) && g.pos <= t.pos) ++i; else ++j; }
        else { ++i; ++j; }
      }
    }
    if (i < ie) add(VD_EV_EXTRA_LINES, i, -1);
    else if (j < je) add(VD_EV_EXTRA_LINES, -1, j);
  }
  return ev;
}

// ---- deferred floats: the host's strtod, then the same rule -----------------------------------------------------------------------
inline bool vd_deferred_differs(const std::string& a, const std::string& b, double threshold) {
  const float x = (float)strtod(a.c_str(), nullptr), y = (float)strtod(b.c_str(), nullptr);
  return vd_float_rule(x, y, threshold);
}
inline void vd_apply_deferred(VdEvent& e, int what) {
  if (what == VD_WHAT_QUAL) e.flags |= VD_FLAG_QUAL;
  else if (what >= VD_WHAT_FMT_BASE) e.fmt[VD_DIFFERS] |= 1ull << (what - VD_WHAT_FMT_BASE);
  else e.info[VD_DIFFERS] |= 1ull << what;
}

// ---- the report ------------------------------------------------------------------------------------------------------------------
inline bool vd_event_listed(const VdEvent& e) {
  if (e.kind != VD_EV_COMPARED) return true;
  uint64_t any = e.flags;
  for (int m = 0; m < 4; ++m) any |= e.info[m] | e.fmt[m];
  return any != 0;
}
inline std::string vd_json_string(const std::string& s) {
  std::string out = "\"";
  char buf[8];
  for (const char ch : s) {
    const unsigned char c = (unsigned char)ch;
    if (c == '"' || c == '\\') { out += '\\'; out += (char)c; }
    else if (c < 0x20 || c >= 0x7f) { snprintf(buf, sizeof(buf), "\\u%04x", (unsigned)c); out += buf; }
    else out += (char)c;
  }
  return out + "\"";
}
struct VdEventText { std::string gold, test; };
inline const char* vd_kind_name(int kind) {
  static const char* names[] = {"COMPARED", "REF_BLOCKS_OVERLAP", "DIFFERENT_POSITIONS", "EXTRA_LINES"};
  return names[kind];
}
inline const char* const* vd_flag_names() { static const char* n[] = {"ID", "ALLELES", "QUAL", "FILTER"}; return n; }
inline const char* const* vd_mask_names() { static const char* n[] = {"MISSING_IN_TEST", "ADDED_IN_TEST", "TYPE_DIFFERS", "DIFFERS"}; return n; }

// one JSON document: {"compared": n, "events": [...]}; an event is listed when it is not COMPARED or a bit is set
inline std::string vd_report_json(const std::vector<VdEvent>& ev, const std::vector<VdEventText>& text, const std::vector<VdRecord>& gold, const std::vector<VdRecord>& test,
                                  const VdTablesHost& H) {
  int64_t compared = 0;
  for (const VdEvent& e : ev) compared += e.pair >= 0;
  std::string out = "{\"compared\": " + std::to_string(compared) + ", \"events\": [";
  bool first = true;
  for (size_t k = 0; k < ev.size(); ++k) {
    const VdEvent& e = ev[k];
    if (!vd_event_listed(e)) continue;
    if (!first) out += ", ";
    first = false;
    out += std::string("{\"kind\": \"") + vd_kind_name(e.kind) + "\", \"gold_line\": " + std::to_string(e.g >= 0 ? gold[(size_t)e.g].line_no : 0) +
           ", \"test_line\": " + std::to_string(e.t >= 0 ? test[(size_t)e.t].line_no : 0) + ", \"gold_text\": " + vd_json_string(text[k].gold) +
           ", \"test_text\": " + vd_json_string(text[k].test);
    if (e.pair >= 0) {
      out += ", \"flags\": [";
      bool f1 = true;
      for (int b = 0; b < 4; ++b) if (e.flags & (1u << b)) { out += std::string(f1 ? "" : ", ") + "\"" + vd_flag_names()[b] + "\""; f1 = false; }
      out += "]";
      for (int side = 0; side < 2; ++side) {
        out += side ? ", \"format\": {" : ", \"info\": {";
        const std::vector<std::string>& names = side ? H.fmt_names : H.info_names;
        for (int m = 0; m < 4; ++m) {
          out += std::string(m ? ", " : "") + "\"" + vd_mask_names()[m] + "\": [";
          bool n1 = true;
          const uint64_t mask = side ? e.fmt[m] : e.info[m];
          for (size_t f = 0; f < names.size(); ++f) if (mask & (1ull << f)) { out += std::string(n1 ? "" : ", ") + vd_json_string(names[f]); n1 = false; }
          out += "]";
        }
        out += "}";
      }
    }
    out += "}";
  }
  return out + "]}";
}

}  // namespace vdhost
}  // namespace genomicsdb_amd
