// gdb_histogram.h - the input histogram on the device: one pass over every input file of a callset mapping counts its records per
// column bin, weighted by the file's callsets inside the row bounds (host-visible interface, no HIP types).  The step the reference
// puts in front of choosing column partitions: vcf_histogram <json> (reference tools/src/vcf_histogram.cc,
// VCF2TileDBConverter::create_and_print_histogram, tiledb_loader.cc:428-456, UniformHistogram, utils/histogram.{h,cc}).
//
// The files, windows, batch cuts, BGZF inflate and newline / tab index are the device importer's own (the taps of DeviceImporter,
// kernels/gdb_import.h).  Then, per batch, one kernel:
//   text   k_hist_lines: one thread per line -> (bin, error bits) by core/gdb_histogram.hpp
//   BCF2   k_hist_records: one thread per record of the uploaded batch, the same (rid / pos through the header's dictionary; the
//          importer's per-record index pass is not needed and not run)
// and both end alike: runs of equal bins inside a wavefront are found with __shfl_up + __ballot and one 64-bit atomicAdd of
// run_length * weight per run goes to the num_bins counters in device memory, which stay there across all batches and files and are
// copied out once.  Error words: the error bits and per bit the smallest offending line / record of the batch.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../host/vcf_importer.h"
#include "../host/vid_mapper.h"

namespace genomicsdb_amd {

struct InputHistogramStats {
  int64_t num_files = 0;
  int64_t num_records = 0;                     // record lines / records seen
  int64_t num_counted = 0;                     // those inside the column bounds
  uint64_t total_weight = 0;                   // the sum of all bins
  int64_t num_batches = 0;
  int64_t num_atomics = 0;                     // atomicAdds on the counters: the sum of runs
  float ms_index = 0, ms_inflate = 0, ms_histogram = 0;      // HIP-event time per phase, summed over the batches
  double s_read = 0, s_h2d = 0, s_total = 0;   // wall clock: file read (+ host inflate), uploads, all
};

struct InputHistogramRequest {
  int64_t max_histogram_range = 0; uint64_t num_bins = 0;
  int64_t column_begin = 0, column_end = INT64_MAX - 1;      // the loader's partition: records that begin inside are counted
  int64_t row_begin = 0, row_end = INT64_MAX - 1;            // lb / ub_callset_row_idx: the callsets that weigh; a file without one is not opened
  std::string file_root;
  int device = 0; uint64_t text_budget_bytes = 0; int inflate_mode = 0;      // as for DeviceImporter
  std::vector<ImportStream> streams;                         // files held in memory, by their "filename" (as for import_cells)
};

// -> num_bins counters.  Refused before any launch: num_bins == 0, a negative max_histogram_range, counters that do not fit in the
// device's free memory (with the sizes), CSV cell files (by name), a stream that no callset names.  A line or record error (contig not
// in the vid, POS / END not a plain integer, fewer than 8 columns, a counted column above max_histogram_range) names
// "<path> line <n>" / "<path> record <n>", 1-based, and nothing is returned.  No device: GenomicsDBDeviceException, there is no CPU path.
std::vector<uint64_t> input_histogram_device(const VidMapper& vid, const InputHistogramRequest& req, InputHistogramStats* stats = nullptr);

// Histogram::print of the reference: "Histogram: [\n", "lo,hi,count\n" per non-zero bin, "]\n"
inline std::string histogram_text(const uint64_t* counts, uint64_t num_bins, uint64_t max_histogram_range) {
  std::string out = "Histogram: [\n";
  const uint64_t size = num_bins ? (max_histogram_range + 1u + (num_bins - 1u)) / num_bins : 0u;
  char line[96];
  for (uint64_t b = 0; b < num_bins; ++b) {
    if (!counts[b]) continue;
    snprintf(line, sizeof(line), "%llu,%llu,%llu\n", (unsigned long long)(b * size), (unsigned long long)((b + 1u) * size - 1u), (unsigned long long)counts[b]);
    out += line;
  }
  out += "]\n";
  return out;
}

}  // namespace genomicsdb_amd
