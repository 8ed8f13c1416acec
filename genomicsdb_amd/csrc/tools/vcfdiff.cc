// vcfdiff - command line of the reference's semantic VCF differ (reference: tools/src/vcfdiff.cc, tools/include/vcfdiff.h):
//   vcfdiff [-t <threshold>] [-r <regions>] <gold> <test>
// Two VCF text files (plain, gzip or BGZF; no index is needed) are compared on the GPU (GDBAMD_DEVICE / LOCAL_RANK, as the other tools
// choose it; kernels/gdb_vcfdiff.hip), allele order, the order of INFO keys, FORMAT keys and sample columns and float noise below the
// threshold aside.  The reference's message strings are printed (:682-755, :1074-1168), the lines as they stand in the files:
// differences and misplaced or extra lines on stderr, the warning for overlapping reference blocks on stdout.  The messages of the
// INFO and FORMAT fields of a pair come in the gold line's key order, then the added ones in the test line's key order.  One
// GENOMICSDB_TIMER,vcfdiff,... line on stderr carries the statistics.  Exit 0 as the reference's; -1 for bad arguments, for what this
// build refuses by name (BCF2 input, -l / --loader-config, -p, --test_to_gold_callset_map_file) and for an error.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <algorithm>
#include <string>
#include <vector>

#include "../kernels/gdb_vcfdiff.h"

using namespace genomicsdb_amd;

static std::string column(const std::string& line, int k) {
  size_t b = 0;
  for (int c = 0;; ++c) {
    const size_t e = line.find('\t', b);
    if (c == k) return line.substr(b, e == std::string::npos ? std::string::npos : e - b);
    if (e == std::string::npos) return std::string();
    b = e + 1;
  }
}

// the keys of an INFO (';', up to '=') or FORMAT (':') column, in the line's order
static std::vector<std::string> keys_of(const std::string& line, int col, char sep) {
  std::vector<std::string> out;
  const std::string c = column(line, col);
  size_t b = 0;
  for (size_t i = 0; i <= c.size(); ++i)
    if (i == c.size() || c[i] == sep) { const std::string kv = c.substr(b, i - b); out.push_back(kv.substr(0, kv.find('='))); b = i + 1; }
  return out;
}

int main(int argc, char** argv) {
  enum { ARG_CALLSET_MAP = 1000 };
  static struct option long_options[] = {{"threshold", 1, 0, 't'}, {"regions", 1, 0, 'r'}, {"loader-config", 1, 0, 'l'}, {"process-idx", 1, 0, 'p'},
                                         {"test_to_gold_callset_map_file", 1, 0, ARG_CALLSET_MAP}, {0, 0, 0, 0}};
  VcfDiffRequest req;
  int c;
  while ((c = getopt_long(argc, argv, "t:r:l:p:", long_options, NULL)) >= 0) {
    switch (c) {
      case 't': req.threshold = strtod(optarg, 0); break;
      case 'r': req.regions = optarg; break;
      case 'l': std::cerr << "vcfdiff: -l / --loader-config (the loader-partition mode) is not in this build\n"; return -1;
      case 'p': std::cerr << "vcfdiff: -p (the loader-partition mode) is not in this build\n"; return -1;
      case ARG_CALLSET_MAP: std::cerr << "vcfdiff: --test_to_gold_callset_map_file is not in this build: samples are matched by name\n"; return -1;
      default: std::cerr << "Unknown command line argument\n"; return -1;
    }
  }
  if (optind + 2 > argc) { std::cerr << "Needs 2 VCF files as input <gold> <test>\n"; return -1; }
  req.gold = argv[optind]; req.test = argv[optind + 1];
  if (const char* e = getenv("GDBAMD_DEVICE")) req.device = atoi(e); else if (const char* e2 = getenv("LOCAL_RANK")) req.device = atoi(e2);
  if (const char* e = getenv("GDBAMD_VCFDIFF_TEXT_BUDGET")) req.text_budget_bytes = strtoull(e, nullptr, 10);
  try {
    VcfDiffStats st;
    const VcfDiffReport rep = vcfdiff_device(req, &st);
    const char* bar = "=====================================================================\n";
    for (const VcfDiffEvent& e : rep.events) {
      if (e.kind == 3) {
        std::cerr << "ERROR: " << (e.gold_line ? "Gold" : "Test") << " vcf has extra line(s) - printing the first extra line\n" << (e.gold_line ? e.gold_text : e.test_text) << "\n";
        continue;
      }
      if (e.kind == 2) {
        std::cerr << "ERROR: Lines with different positions found - resetting file ptr to next match position\n" << e.gold_text << "\n" << e.test_text << "\n";
        continue;
      }
      if (e.kind == 1) {
        const long long gp = atoll(column(e.gold_text, 1).c_str()), tp = atoll(column(e.test_text, 1).c_str());
        std::cout << "WARNING: Gold and test REF blocks overlap, but do not match exactly at position " << column(e.test_text, 0) << "," << (gp < tp ? gp : tp) << "\n"
                  << e.gold_text << "\n" << e.test_text << "\n";
      }
      uint64_t any = e.flags;
      for (int m = 0; m < 4; ++m) any |= e.info[m] | e.fmt[m];
      if (!any) continue;
      std::cerr << bar << e.gold_text << "\n" << e.test_text << "\n";
      if (e.flags & 1u) std::cerr << "ID field different\n";
      if (e.flags & 2u) std::cerr << "Allele list different\n";
      if (e.flags & 4u) std::cerr << "QUAL field different\n";
      if (e.flags & 8u) std::cerr << "FILTER list different\n";
      for (int side = 0; side < 2; ++side) {
        const char* what = side ? "FORMAT" : "INFO";
        const std::vector<std::string>& names = side ? rep.fmt_names : rep.info_names;
        const uint64_t* m = side ? e.fmt : e.info;
        // gold's messages in the gold line's key order, then the added ones in the test line's key order
        uint64_t said = 0;
        for (const std::string& key : keys_of(e.gold_text, side ? 8 : 7, side ? ':' : ';')) {
          const size_t f = (size_t)(std::find(names.begin(), names.end(), key) - names.begin());
          if (f >= names.size() || (said & (1ull << f))) continue;
          said |= 1ull << f;
          const uint64_t bit = 1ull << f;
          if (m[0] & bit) std::cerr << "ERROR: " << what << " field " << names[f] << " missing in test line\n";
          if (m[2] & bit) std::cerr << "ERROR: " << what << " field " << names[f] << " type is different in gold and test\n";
          if (m[3] & bit) std::cerr << "ERROR: Gold and test differ in the " << what << " field " << names[f] << "\n";
        }
        said = 0;
        for (const std::string& key : keys_of(e.test_text, side ? 8 : 7, side ? ':' : ';')) {
          const size_t f = (size_t)(std::find(names.begin(), names.end(), key) - names.begin());
          if (f >= names.size() || (said & (1ull << f))) continue;
          said |= 1ull << f;
          if (m[1] & (1ull << f)) std::cerr << "ERROR: " << what << " field " << names[f] << " added in test line\n";
        }
      }
      std::cerr << bar;
    }
    std::cerr << "GENOMICSDB_TIMER,vcfdiff,Wall-clock time(s)," << st.s_total << ",gold_records," << st.gold_records << ",test_records," << st.test_records << ",compared,"
              << st.pairs_compared << ",light," << st.pairs_light << ",heavy," << st.pairs_heavy << ",deferred," << st.deferred << ",events," << st.events << ",batches,"
              << st.num_batches << ",resident_bytes," << st.resident_bytes << ",index_ms," << st.ms_index << ",inflate_ms," << st.ms_inflate << ",keys_ms," << st.ms_keys
              << ",compare_ms," << st.ms_compare << ",read_s," << st.s_read << ",walk_s," << st.s_walk << "\n";
  } catch (const std::exception& e) {
    std::cerr << "vcfdiff: " << e.what() << "\n";
    return -1;
  }
  return 0;
}
