// vcf_histogram - command line of the reference's histogram tool (reference: tools/src/vcf_histogram.cc;
// VCF2TileDBConverter::create_and_print_histogram, src/main/cpp/src/loader/tiledb_loader.cc:428-456):
//   vcf_histogram [-r <rank>] [--inflate-on-host] [--equi-partitions <N>]... <json>
// <json> is a loader JSON that also carries "max_histogram_range" and "num_bins" (both required, as the reference requires them).
// One pass over every input file of the callset mapping on the rank's GPU (LOCAL_RANK / GDBAMD_DEVICE, as the other tools choose it;
// kernels/gdb_histogram.hip) counts the records per column bin, weighted by the file's callsets inside "lb_callset_row_idx" /
// "ub_callset_row_idx"; only records that begin inside column partition `rank` count.  stdout carries the reference's print:
//   Histogram: [
//   lo,hi,count        per non-zero bin
//   ]
// and, for every --equi-partitions N, the text of gdbamd_equi_partition_text over the same counts (hist_begin 0, bin_size
// size_of_bin, num_parts N): the partitioning that gt_mpi_gather --produce-histogram prints for an array that exists already.
// One GENOMICSDB_TIMER,Rank,<r>,input_histogram,... line on stderr carries the statistics.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../api/genomicsdb_bcf_generator.h"
#include "../common/mini_json.hpp"
#include "../kernels/gdb_histogram.h"

using namespace genomicsdb_amd;

extern "C" int64_t gdbamd_equi_partition_text(const uint64_t* counts, uint64_t nbins, uint64_t hist_begin, uint64_t bin_size, uint64_t num_parts, char* dst, uint64_t cap);

static int launcher_rank() {
  for (const char* name : {"OMPI_COMM_WORLD_RANK", "PMI_RANK", "PMIX_RANK", "SLURM_PROCID", "RANK"})
    if (const char* e = getenv(name)) return atoi(e);
  return 0;
}

static int64_t required_int(const mini_json::Value& doc, const char* key) {
  if (!doc.HasMember(key) || !doc[key].IsInt64()) throw GenomicsDBConfigException(std::string("the JSON needs the integer \"") + key + "\"");
  return doc[key].GetInt64();
}

int main(int argc, char** argv) {
  enum { ARG_INFLATE_ON_HOST = 1000, ARG_EQUI_PARTITIONS };
  static struct option long_options[] = {{"rank", 1, 0, 'r'}, {"inflate-on-host", 0, 0, ARG_INFLATE_ON_HOST}, {"equi-partitions", 1, 0, ARG_EQUI_PARTITIONS}, {0, 0, 0, 0}};
  int rank = launcher_rank();
  bool inflate_on_host = false;
  std::vector<uint64_t> equi;
  int c;
  while ((c = getopt_long(argc, argv, "r:", long_options, NULL)) >= 0) {
    switch (c) {
      case 'r': rank = atoi(optarg); break;
      case ARG_INFLATE_ON_HOST: inflate_on_host = true; break;
      case ARG_EQUI_PARTITIONS: equi.push_back(strtoull(optarg, nullptr, 10)); break;
      default: std::cerr << "Unknown command line argument\n"; return -1;
    }
  }
  if (optind + 1 > argc) { std::cerr << "Needs 1 arg <json_config_file>\n"; return -1; }
  try {
    const mini_json::Value doc = mini_json::parse_file(argv[optind]);
    InputHistogramRequest req;
    req.max_histogram_range = required_int(doc, "max_histogram_range");
    const int64_t num_bins = required_int(doc, "num_bins");
    if (num_bins < 0) throw GenomicsDBConfigException("\"num_bins\" is negative");
    req.num_bins = (uint64_t)num_bins;
    GenomicsDBImportConfig loader;
    loader.read_from_json(doc, rank);
    if (loader.m_vid_mapping_file.empty() || loader.m_callset_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file and callset_mapping_file");
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(loader.m_vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(loader.m_callset_mapping_file));
    const ColumnRange part = loader.get_column_partition(rank);
    req.column_begin = part.first; req.column_end = part.second;
    req.row_begin = loader.m_lb_callset_row_idx; req.row_end = loader.m_ub_callset_row_idx;
    req.inflate_mode = inflate_on_host ? 1 : 0;
    if (const char* e = getenv("GDBAMD_DEVICE")) req.device = atoi(e); else if (const char* e2 = getenv("LOCAL_RANK")) req.device = atoi(e2);
    if (const char* e = getenv("GDBAMD_HISTOGRAM_TEXT_BUDGET")) req.text_budget_bytes = strtoull(e, nullptr, 10);
    InputHistogramStats st;
    const std::vector<uint64_t> counts = input_histogram_device(vid, req, &st);
    std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",input_histogram,Wall-clock time(s)," << st.s_total << ",files," << st.num_files << ",records," << st.num_records
              << ",counted," << st.num_counted << ",total_weight," << st.total_weight << ",batches," << st.num_batches << ",atomics," << st.num_atomics << ",index_ms,"
              << st.ms_index << ",inflate_ms," << st.ms_inflate << ",histogram_ms," << st.ms_histogram << ",read_s," << st.s_read << ",h2d_s," << st.s_h2d << "\n";
    std::cout << histogram_text(counts.data(), counts.size(), (uint64_t)req.max_histogram_range);
    const uint64_t bin_size = ((uint64_t)req.max_histogram_range + 1u + (req.num_bins - 1u)) / req.num_bins;
    for (const uint64_t parts : equi) {
      const int64_t n = gdbamd_equi_partition_text(counts.data(), counts.size(), 0u, bin_size, parts, nullptr, 0);
      if (n < 0) throw GenomicsDBConfigException("--equi-partitions " + std::to_string(parts) + ": the number of partitions must be positive and below num_bins");
      std::string text((size_t)n, '\0');
      gdbamd_equi_partition_text(counts.data(), counts.size(), 0u, bin_size, parts, &text[0], (uint64_t)n);
      std::cout << text;
    }
  } catch (const std::exception& e) {
    std::cerr << "vcf_histogram: " << e.what() << "\n";
    return -1;
  }
  return 0;
}
