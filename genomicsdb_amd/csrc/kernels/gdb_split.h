// gdb_split.h - the device splitter: every (g)VCF text file of a callset mapping cut into one bgzipped, tabix-indexed file per column
// partition, in ONE pass over the file (host-visible interface, no HIP types).  The step the reference puts in front of a
// multi-partition import: vcf2tiledb --split-files (reference tools/src/vcf2tiledb.cc:118-151, src/main/cpp/src/vcf/vcf2binary.cc:1198-1261,
// which runs one tabix region query per partition, that is P passes).
//
// The files, windows, batch cuts, BGZF inflate and newline / tab index are the device importer's own (a text tap on DeviceImporter,
// kernels/gdb_import.h), run once per batch whatever the number of partitions.  Then, per batch:
//   classify  k_split_classify: one thread per line -> the run of partitions the line overlaps (core/gdb_split.hpp), its byte length
//             with the newline, error bits with the smallest offending line
//   compact   per produced partition that the batch touches: k_split_select (length or 0 per line), rocPRIM exclusive scan,
//             k_split_gather: one wavefront per selected line copies it behind the partition's packed text with aligned 16-byte stores
//   compress  a partition's packed text accumulates on the device and leaves it as BGZF blocks (BgzfDeviceCompressor, text mode)
// The '#' lines go through bgzf_compress_host once per output, kBgzfEofBlock ends it, host/vcf_index.h writes <output>.tbi - or, with
// index_on_device, kernels/gdb_index.h builds it while the output is written: every deflated piece of packed text is a batch of the
// index, taken while the text is still in device memory, with the blocks it just became as the member table.  An output
// is written under a temporary name and renamed when its whole input went through: on an error no output of that input is left.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../host/vid_mapper.h"

namespace genomicsdb_amd {

struct SplitStats {
  int64_t num_files = 0, num_record_lines = 0;
  int64_t num_lines_written = 0;               // record lines, summed over the produced partitions
  uint64_t text_bytes_in = 0;                  // inflated bytes of the inputs
  uint64_t text_bytes_out = 0;                 // inflated bytes of the outputs
  uint64_t compressed_bytes_out = 0;           // bytes of the outputs as written (without the .tbi files)
  int64_t num_batches = 0;
  float ms_index = 0, ms_classify = 0, ms_scan_gather = 0, ms_deflate = 0;      // HIP-event time per phase, summed
  double s_read = 0, s_h2d = 0, s_d2h_write = 0, s_index_build = 0, s_total = 0;      // wall clock: file read (+ host inflate), uploads, compressed download + write, .tbi, all
  float ms_inflate = 0;                        // HIP-event time of the BGZF inflate kernel (BGZF input)
  double ms_index_kernels = 0;                 // HIP-event time of the index kernels (index_on_device; s_index_build is the wall clock on either path)
};

struct SplitRequest {
  std::vector<std::pair<int64_t, int64_t>> partitions;      // [begin, end] per partition index (the loader's column_partitions, ends derived)
  std::vector<int> produce;                                 // partition indices to write; empty: all
  std::string file_root, results_directory;
  std::string single_output;                                // output path of the only input (one input, one produced partition), else empty
  std::vector<std::string> extra_paths;                     // inputs that the callset mapping does not list
  int device = 0; uint64_t text_budget_bytes = 0; int inflate_mode = 0;      // as for DeviceImporter
  // the outputs' .tbi by kernels/gdb_index.h while they are written: from the packed text still in device memory, the blocks the deflate
  // just made and the header member; false: host/vcf_index.h re-reads each finished output.  The files are the same, byte for byte
  bool index_on_device = false;
};

struct SplitOutput { std::string original; int partition = 0; std::string path; };

// inputs of a split run in order: the "filename"s of the callset mapping (each once), then extra_paths; -> (original name, path to read)
std::vector<std::pair<std::string, std::string>> split_input_files(const VidMapper& vid, const SplitRequest& req);

// Refuses, before any launch and by name: BCF2 and CSV inputs, more than gdbsplit::kMaxPartitions partitions, partitions that
// overlap, a partition index outside the list.  A line error (contig not in the vid, POS / END not a plain integer, fewer than
// 8 columns) names file and 1-based line like the device importer.
std::vector<SplitOutput> split_files_device(const VidMapper& vid, const SplitRequest& req, SplitStats* stats = nullptr);

}  // namespace genomicsdb_amd
