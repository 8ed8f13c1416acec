// malformed_bcf.cc - the BCF2 path of the device importer on hostile input, on the CPU: a valid stream and seeded mutations of
// it go through the harness of hostsim_import_bcf.hpp.  Built with -fsanitize=address,undefined -fno-sanitize-recover=all and
// run as a program of its own: each case either is refused with an error or yields cells, and any read or write outside the
// exact-size blocks of the harness ends the program with the sanitizer's report.
//
//   malformed_bcf VID.json CALLSETS.json STREAM.bcf [N=2000] [SEED=1] [HOSTILE.bcf ...]
//
// Every HOSTILE.bcf is one more case that must be refused (a non-zero exit otherwise): the few malformed inputs that the GPU tests
// use are shown here first to be refused without a read outside a block.
// The callset mapping must name one file; its content is STREAM.bcf, mutated.  Half of the mutations fall in the first 200 bytes
// of a record, every 7th case is truncated as well.  Prints one line of counts by error kind.
#include <cstdio>
#include <fstream>
#include <map>
#include <random>
#include <sstream>

#include "hostsim_import_bcf.hpp"
#include "../../genomicsdb_amd/csrc/common/mini_json.hpp"

using namespace genomicsdb_amd;

static const char* kind_name(uint32_t bit) {
  switch (bit) {
    case gdbimp::IMP_ERR_CONTIG: return "contig_not_in_vid";
    case gdbimp::IMP_ERR_FILTER: return "filter_not_in_vid";
    case gdbimp::IMP_ERR_COUNT: return "fixed_length_count";
    case gdbimp::IMP_ERR_COORD_RANGE: return "column_range";
    case gdbimp::IMP_ERR_BCF_TYPE_CODE: return "type_code";
    case gdbimp::IMP_ERR_BCF_BOUNDS: return "bounds";
    case gdbimp::IMP_ERR_BCF_DICT: return "dictionary_id";
    case gdbimp::IMP_ERR_BCF_NSAMPLE: return "n_sample";
    case gdbimp::IMP_ERR_BCF_FIELD_TYPE: return "field_type";
    case gdbimp::IMP_ERR_BCF_END: return "info_end";
    default: return "other";
  }
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: malformed_bcf VID.json CALLSETS.json STREAM.bcf [N] [SEED]\n"); return 2; }
  const int n_cases = argc > 4 ? atoi(argv[4]) : 2000;
  const unsigned seed = argc > 5 ? (unsigned)atoi(argv[5]) : 1u;
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(argv[1]));
  vid.parse_callsets_json(mini_json::parse_file(argv[2]));
  std::ifstream in(argv[3], std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string valid = ss.str();
  ImportOptions opt;
  opt.treat_deletions_as_intervals = true;
  // the records of the valid stream (it must import)
  std::vector<uint64_t> offs;
  {
    hostsim_bcf::Stats st;
    const std::vector<uint8_t> cells = hostsim_bcf::run(vid, opt, 4096, [&](const ImportFile&) { return valid; }, &st);
    if (cells.empty()) { fprintf(stderr, "the valid stream gave no cells\n"); return 1; }
    const ImportTablesHost H = build_import_tables(vid);
    const std::vector<ImportFile> files = import_files(vid, opt);
    const BcfHeaderHost hdr = parse_bcf_header(valid.data(), valid.size(), files.at(0), H);
    bcf_walk_records(valid.data(), valid.size(), hdr.records_begin, "valid", offs);
  }
  const size_t n_rec = offs.size() - 1;
  std::mt19937 rng(seed);
  std::map<std::string, int> counts;
  for (int k = 0; k < n_cases; ++k) {
    std::string s = valid;
    const int n_mut = 1 + (int)(rng() % 3u);
    for (int m = 0; m < n_mut; ++m) {
      const size_t r = rng() % n_rec;
      const size_t len = (size_t)(offs[r + 1] - offs[r]);
      const size_t span = (k % 2 == 0) ? std::min<size_t>(len, 200) : len;       // half of the cases: the first 200 bytes of a record
      const size_t at = (size_t)offs[r] + rng() % span;
      switch (rng() % 4u) {
        case 0: s[at] = (char)(rng() & 0xFF); break;
        case 1: s[at] = (char)(s[at] ^ (1u << (rng() % 8u))); break;
        case 2: s[at] = (char)0xFF; break;
        default: s[at] = (char)((s[at] & 0xF0) | (rng() % 16u)); break;      // another type code in a descriptor
      }
    }
    if (k % 7 == 6) s.resize((size_t)offs[0] + rng() % (s.size() - (size_t)offs[0]));      // truncated
    uint32_t bit = 0;
    try {
      hostsim_bcf::Stats st;
      hostsim_bcf::run(vid, opt, (k % 3 == 0) ? 256 : 4096, [&](const ImportFile&) { return s; }, &st, &bit);
      ++counts["imported"];
    } catch (const VCF2BinaryException& e) {
      if (bit) ++counts[kind_name(bit)];
      else if (strstr(e.what(), "truncated BCF2 record") || strstr(e.what(), "l_shared")) ++counts["broken_chain"];
      else ++counts["other"];
    }
  }
  for (int a = 6; a < argc; ++a) {
    std::ifstream hin(argv[a], std::ios::binary);
    std::stringstream hs;
    hs << hin.rdbuf();
    const std::string s = hs.str();
    for (uint64_t budget : {(uint64_t)256, (uint64_t)1 << 20}) {
      try {
        hostsim_bcf::Stats st;
        hostsim_bcf::run(vid, opt, budget, [&](const ImportFile&) { return s; }, &st);
        fprintf(stderr, "%s was imported, not refused\n", argv[a]);
        return 1;
      } catch (const VCF2BinaryException&) { ++counts["hostile_refused"]; }
    }
  }
  printf("cases %d", n_cases);
  for (const auto& kv : counts) printf(" %s %d", kv.first.c_str(), kv.second);
  printf("\n");
  return 0;
}
