// vcf2tiledb - command line of the reference's import tool for what this build implements:
//   vcf2tiledb [-r <rank>] [--import-on-device [--inflate-on-host]] [--merge-window-bytes <N>] <loader.json>
// (reference: tools/src/vcf2tiledb.cc:54-140; VCF2TileDBLoader::read_all, src/main/cpp/src/loader/tiledb_loader.cc:845-965).
// The (g)VCFs of the callset mapping are converted to begin-cells of column partition `rank` (host, vcf_importer.cc) and
//   "produce_tiledb_array": true  -> written to <workspace>/<array>/cells.bin, the array file gt_mpi_gather and the JNI stream open
//   "produce_combined_vcf": true  -> combined in-line on the GPU (same path as gt_mpi_gather --produce-Broad-GVCF) and written
//                                    to stdout, like the reference loader's in-line BroadCombinedGVCFOperator
// --import-on-device: the conversion runs on the rank's GPU (LOCAL_RANK / GDBAMD_DEVICE, as the other tools choose it) and gives the
// same cells; the default is the host importer.  On the device, bgzip'ed input (BGZF) is inflated there too and crosses the link
// compressed; --inflate-on-host keeps zlib on the host for every file.  BCF2 files (.bcf, sniffed by content) are read with
// --import-on-device only; without it the tool names the file and exits with an error.
// Incremental import: "lb_callset_row_idx" / "ub_callset_row_idx" of the loader JSON choose the callsets of this batch, and with
//   "delete_and_create_tiledb_array": false  (written out; the reference's default)
// a batch is MERGED into an existing <workspace>/<array>/cells.bin on the rank's GPU (kernels/gdb_merge.hip), the result written to a
// temporary name in the same directory and renamed over cells.bin.  With the key absent or true the array file is overwritten.
// --merge-window-bytes <N>: the merge goes window by window from the cells.bin file and the batch to the new file, with at most N input
// bytes on the device (0: derived from its free memory) - for arrays larger than device memory; cells.bin is never read whole.  Without
// the option the merge runs in-core, and turns to the windowed path, saying so, only when the sizes do not fit the device together.
// "produce_combined_vcf" in the same run combines the cells of the batch only, like the reference's in-line operator.
// Splitting (reference tools/src/vcf2tiledb.cc:118-151; nothing is imported):
//   vcf2tiledb [-r <rank>] --split-files [--split-all-partitions] [--split-files-results-directory <dir>] [--split-output-filename <file>]
//              [--split-callset-mapping-file] [--split-index-on-device] <loader.json> [more VCF files ..]
// cuts every (g)VCF text file of the callset mapping, and the files named behind the loader JSON, into one bgzipped and tabix-indexed
// file per column partition on the rank's GPU (kernels/gdb_split.hip): partition `rank`, or all of them in one pass per file with
// --split-all-partitions.  Outputs are <dir, or the input's directory>/partition_<p>_<basename> unless the callset mapping's
// "split_files_paths" or --split-output-filename (one input, one partition) names them.  --split-callset-mapping-file also writes,
// per produced partition, the callset mapping that names the split files and a loader JSON that names those mappings, by the same
// path rule.  --split-index-on-device builds each output's .tbi on the GPU while the output is written (kernels/gdb_index.hip) instead
// of re-reading the finished file on the host; the files are the same.  With "row_based_partitioning": true the reference's message is printed and nothing is done.
#include <getopt.h>
#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../api/genomicsdb_bcf_generator.h"
#include "../api/loader_outputs.h"
#include "../common/mini_json.hpp"
#include "../host/vcf_importer.h"
#include "../kernels/gdb_split.h"

using namespace genomicsdb_amd;

static int launcher_rank() {
  for (const char* name : {"OMPI_COMM_WORLD_RANK", "PMI_RANK", "PMIX_RANK", "SLURM_PROCID", "RANK"})
    if (const char* e = getenv(name)) return atoi(e);
  return 0;
}
static void write_text_file(const std::string& path, const std::string& text, const char* what) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) throw GenomicsDBConfigException(std::string("Could not write to partitioned ") + what + " JSON file " + path);
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0 || !ok) throw GenomicsDBConfigException(std::string("Could not write to partitioned ") + what + " JSON file " + path);
}

// --split-files: see the head of this file
static int split_files_main(const std::string& loader_json, int rank, bool all_partitions, const std::string& results_directory, const std::string& output_filename,
                            bool write_mappings, bool inflate_on_host, bool index_on_device, const std::vector<std::string>& extra_paths) {
  const mini_json::Value doc = mini_json::parse_file(loader_json);
  if (doc.HasMember("row_based_partitioning") && doc["row_based_partitioning"].GetBool()) {
    std::cerr << "Splitting is available for column partitioning, row partitioning should be trivial if samples are scattered across files. See wiki page "
                 "https://github.com/Intel-HLS/GenomicsDB/wiki/Dealing-with-multiple-GenomicsDB-partitions for more information\n";
    return 0;
  }
  GenomicsDBImportConfig loader;
  loader.read_from_json(doc, rank);
  if (loader.m_vid_mapping_file.empty() || loader.m_callset_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file and callset_mapping_file");
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse_file(loader.m_vid_mapping_file));
  vid.parse_callsets_json(mini_json::parse_file(loader.m_callset_mapping_file));
  SplitRequest req;
  const size_t np = std::max<size_t>(loader.m_column_partitions.size(), 1);
  for (size_t p = 0; p < np; ++p) { const ColumnRange r = loader.get_column_partition((int)p); req.partitions.emplace_back(r.first, r.second); }
  if (!all_partitions) req.produce.push_back(rank);
  req.results_directory = results_directory;
  req.extra_paths = extra_paths;
  req.inflate_mode = inflate_on_host ? 1 : 0;
  req.index_on_device = index_on_device;
  if (const char* e = getenv("GDBAMD_DEVICE")) req.device = atoi(e); else if (const char* e2 = getenv("LOCAL_RANK")) req.device = atoi(e2);
  if (const char* e = getenv("GDBAMD_SPLIT_TEXT_BUDGET")) req.text_budget_bytes = strtoull(e, nullptr, 10);
  const std::vector<std::pair<std::string, std::string>> inputs = split_input_files(vid, req);
  // (the reference: only with one file and one partition, else the option is ignored)
  if (!all_partitions && inputs.size() == 1u && !output_filename.empty()) vid.set_single_split_file_path(inputs[0].first, output_filename);
  SplitStats st;
  const std::vector<SplitOutput> done = split_files_device(vid, req, &st);
  std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",split_files,Wall-clock time(s)," << st.s_total << ",files," << st.num_files << ",record_lines," << st.num_record_lines
            << ",lines_written," << st.num_lines_written << ",text_bytes_in," << st.text_bytes_in << ",text_bytes_out," << st.text_bytes_out << ",compressed_bytes_out,"
            << st.compressed_bytes_out << ",batches," << st.num_batches << ",index_ms," << st.ms_index << ",classify_ms," << st.ms_classify << ",scan_gather_ms,"
            << st.ms_scan_gather << ",deflate_ms," << st.ms_deflate << ",inflate_ms," << st.ms_inflate << ",read_s," << st.s_read << ",h2d_s," << st.s_h2d
            << ",d2h_write_s," << st.s_d2h_write << ",index_build_s," << st.s_index_build << ",index_kernels_ms," << st.ms_index_kernels << "\n";
  if (!write_mappings) return 0;
  // the callset mapping of a partition (reference vid_mapper.cc:1083-1151): every callset with its row, its index in the file and the split file
  auto split_path_of = [&](const std::string& original, int p) {
    for (const SplitOutput& o : done) if (o.original == original && o.partition == p) return o.path;
    throw GenomicsDBConfigException("no split file of " + original + " for partition " + std::to_string(p));
  };
  std::vector<int> produced;
  if (all_partitions) for (size_t p = 0; p < np; ++p) produced.push_back((int)p); else produced.push_back(rank);
  for (const int p : produced) {
    mini_json::Value callsets = mini_json::make_object();
    for (const CallSetInfo& cs : vid.get_callsets()) {
      mini_json::Value one = mini_json::make_object();
      one.obj.emplace_back("row_idx", mini_json::make_int(cs.m_row_idx));
      one.obj.emplace_back("idx_in_file", mini_json::make_int(cs.m_idx_in_file));
      one.obj.emplace_back("filename", mini_json::make_string(split_path_of(cs.m_filename, p)));
      callsets.obj.emplace_back(cs.m_name, one);
    }
    // (the file-type lists of the reference's writer name CSV files and buffer streams: the splitter refuses the first and has none of the second)
    mini_json::Value out = mini_json::make_object();
    out.obj.emplace_back("callsets", callsets);
    write_text_file(vid.get_split_file_path(loader.m_callset_mapping_file, results_directory, p), mini_json::serialize(out), "callsets");
  }
  // the loader JSON (reference vid_mapper.cc:1153-1185): "callset_mapping_file" names the partition's mapping, or lists all of them
  mini_json::Value ldoc = doc;
  for (size_t i = 0; i < ldoc.obj.size();) { if (ldoc.obj[i].first == "callset_mapping_file") ldoc.obj.erase(ldoc.obj.begin() + (long)i); else ++i; }
  if (produced.size() > 1) {
    mini_json::Value list = mini_json::make_array();
    for (const int p : produced) list.arr.push_back(mini_json::make_string(vid.get_split_file_path(loader.m_callset_mapping_file, results_directory, p)));
    ldoc.obj.emplace_back("callset_mapping_file", list);
  } else ldoc.obj.emplace_back("callset_mapping_file", mini_json::make_string(vid.get_split_file_path(loader.m_callset_mapping_file, results_directory, rank)));
  write_text_file(vid.get_split_file_path(loader_json, results_directory, rank), mini_json::serialize(ldoc), "loader");
  return 0;
}

int main(int argc, char** argv) {
  enum { ARG_VERSION = 1000, ARG_IMPORT_ON_DEVICE, ARG_INFLATE_ON_HOST, ARG_SPLIT_FILES, ARG_SPLIT_ALL, ARG_SPLIT_DIRECTORY, ARG_SPLIT_OUTPUT, ARG_SPLIT_MAPPING, ARG_SPLIT_INDEX_ON_DEVICE, ARG_MERGE_WINDOW_BYTES };
  static struct option long_options[] = {{"tmp-directory", 1, 0, 'T'}, {"rank", 1, 0, 'r'}, {"version", 0, 0, ARG_VERSION}, {"import-on-device", 0, 0, ARG_IMPORT_ON_DEVICE},
                                         {"inflate-on-host", 0, 0, ARG_INFLATE_ON_HOST}, {"merge-window-bytes", 1, 0, ARG_MERGE_WINDOW_BYTES},
                                         {"split-files", 0, 0, ARG_SPLIT_FILES}, {"split-all-partitions", 0, 0, ARG_SPLIT_ALL},
                                         {"split-files-results-directory", 1, 0, ARG_SPLIT_DIRECTORY}, {"split-output-filename", 1, 0, ARG_SPLIT_OUTPUT},
                                         {"split-callset-mapping-file", 0, 0, ARG_SPLIT_MAPPING}, {"split-index-on-device", 0, 0, ARG_SPLIT_INDEX_ON_DEVICE},
                                         {0, 0, 0, 0}};
  int rank = launcher_rank();
  bool import_on_device = false, inflate_on_host = false;
  bool split_index_on_device = false;
  bool merge_windowed = false;
  uint64_t merge_window_bytes = 0;
  bool split_files = false, split_all = false, split_mapping = false;      // (any of the five split options turns splitting on; the reference needs --split-files next to the others)
  std::string split_directory, split_output;
  int c;
  while ((c = getopt_long(argc, argv, "T:r:", long_options, NULL)) >= 0) {
    switch (c) {
      case 'T': break;   // no temporary files are written
      case 'r': rank = atoi(optarg); break;
      case ARG_VERSION: std::cout << "genomicsdb_amd (MI355X variant-combine path) for GenomicsDB 0.10.2 loader JSON\n"; return 0;
      case ARG_IMPORT_ON_DEVICE: import_on_device = true; break;
      case ARG_INFLATE_ON_HOST: inflate_on_host = true; break;
      case ARG_MERGE_WINDOW_BYTES: merge_windowed = true; merge_window_bytes = strtoull(optarg, nullptr, 10); break;
      case ARG_SPLIT_FILES: split_files = true; break;
      case ARG_SPLIT_ALL: split_files = true; split_all = true; break;
      case ARG_SPLIT_DIRECTORY: split_files = true; split_directory = optarg; break;
      case ARG_SPLIT_OUTPUT: split_files = true; split_output = optarg; break;
      case ARG_SPLIT_MAPPING: split_files = true; split_mapping = true; break;
      case ARG_SPLIT_INDEX_ON_DEVICE: split_files = true; split_index_on_device = true; break;
      default: std::cerr << "Unknown command line argument\n"; return -1;
    }
  }
  if (optind + 1 > argc) { std::cerr << "Needs 1 argument <loader_json_config_file>\n"; return -1; }
  const std::string loader_json = argv[optind];
  if (split_files) {
    try {
      return split_files_main(loader_json, rank, split_all, split_directory, split_output, split_mapping, inflate_on_host, split_index_on_device,
                              std::vector<std::string>(argv + optind + 1, argv + argc));
    } catch (const std::exception& e) {
      std::cerr << "vcf2tiledb: " << e.what() << "\n";
      return -1;
    }
  }
  try {
    const auto t0 = std::chrono::steady_clock::now();
    const std::string loader_text = mini_json::read_text_file(loader_json);
    const mini_json::Value doc = mini_json::parse(loader_text);
    GenomicsDBImportConfig loader;
    loader.read_from_json(doc, rank);
    if (loader.m_vid_mapping_file.empty() || loader.m_callset_mapping_file.empty()) throw GenomicsDBConfigException("loader JSON needs vid_mapping_file and callset_mapping_file");
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(loader.m_vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(loader.m_callset_mapping_file));
    const ColumnRange part = loader.get_column_partition(rank);
    ImportOptions opt;
    opt.treat_deletions_as_intervals = loader.m_treat_deletions_as_intervals;
    opt.column_begin = part.first;
    opt.column_end = part.second;
    opt.row_begin = loader.m_lb_callset_row_idx;
    opt.row_end = loader.m_ub_callset_row_idx;
    ImportStats st;
    int device = 0;
    if (const char* e = getenv("GDBAMD_DEVICE")) device = atoi(e); else if (const char* e2 = getenv("LOCAL_RANK")) device = atoi(e2);
    const std::vector<uint8_t> cells = import_on_device ? import_callsets_to_cells_device(vid, opt, device, 0, &st, inflate_on_host ? 1 : 0) : import_callsets_to_cells(vid, opt, &st);
    const double t_import = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",vcf2binary,Wall-clock time(s)," << t_import << ",files," << st.num_files << ",records," << st.num_records
              << ",cells," << st.num_cells << ",bytes," << st.num_bytes << ",device," << (import_on_device ? 1 : 0) << ",deferred," << st.num_deferred_values << "\n";
    if (import_on_device)
      std::cerr << "GENOMICSDB_TIMER,Rank," << rank << ",vcf2binary_inflate,compressed_bytes," << st.compressed_bytes << ",device_members," << st.num_device_members
                << ",host_inflated_files," << st.num_host_inflated_files << ",inflate_kernel_ms," << st.ms_inflate << "\n";
    LoaderOutputs out;
    out.loader_text = loader_text; out.rank = rank; out.device = device; out.tool = "vcf2tiledb";
    out.merge_windowed = merge_windowed; out.merge_window_bytes = merge_window_bytes;
    produce_loader_outputs(out, doc, loader, &cells);
  } catch (const std::exception& e) {
    std::cerr << "vcf2tiledb: " << e.what() << "\n";
    return -1;
  }
  return 0;
}
