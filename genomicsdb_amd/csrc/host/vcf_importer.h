// vcf_importer.h - product host layer: (g)VCF text -> begin-cells in the reference's binary cell layout, the step that
// CREATES what the scan-and-combine path consumes.
//
// What it restates: VCF2Binary::convert_VCF_to_binary_for_callset (reference src/main/cpp/src/vcf/vcf2binary.cc:991-1196; field
// conversion :715-989; deletions as intervals :1043-1059; INFO values of multi-sample files divided among the samples :34-53)
// for the array schema of VidMapper::build_tiledb_array_schema (src/main/cpp/src/utils/vid_mapper.cc:354-442), and the
// column-major hand-over of VCF2TileDBLoader (src/main/cpp/src/loader/tiledb_loader.cc:845-965).
//
//   cell = [row i64][col i64][cell_size u64][END i64][REF: i32 n + chars][ALT: i32 n + 'A|C|&' ('&' = <NON_REF>)]
//          [ID: i32 n + chars (only when the vid declares ID)][QUAL f32][FILTER: i32 n + n x i32 field idx]
//          [INFO attributes in vid order][FORMAT attributes in vid order]
//          fixed-length attribute = num x element (missing: TileDB null), var-length = i32 num + num x element (missing: num 0)
//
// Not done (documented in DESIGN.md): htslib's record-level checks, fields of more than 2 dimensions.  BCF2 files, buffer streams
// and CSV cell files (the "sorted_csv_files" / "unsorted_csv_files" of the callset mapping; core/gdb_import_csv.hpp) are read by the
// device path only (host/import_bcf.hpp); import_callsets_to_cells refuses a BCF2 file and a CSV file by name.  2-dimensional (allele-specific) fields and intervals that reach across a partition begin ARE imported by
// import_callsets_to_cells; the device path (import_callsets_to_cells_device, kernels/gdb_import.hip) refuses 2-dimensional
// fields and flattened tuple elements by name and leaves those vids to the host importer.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "vid_mapper.h"

namespace genomicsdb_amd {

class VCF2BinaryException : public std::runtime_error {
 public:
  explicit VCF2BinaryException(const std::string& m) : std::runtime_error("VCF2BinaryException : " + m) {}
};

struct ImportOptions {
  bool treat_deletions_as_intervals = false;       // loader JSON key of the same name
  int64_t column_begin = 0, column_end = INT64_MAX - 1;   // column partition: cells that begin inside are kept
  std::string file_root;                           // prefix of relative "filename" entries of the callset mapping
  // loader JSON "lb_callset_row_idx" / "ub_callset_row_idx": only callsets whose row lies inside are converted (an incremental
  // import); a file without such a callset is not opened.  Clamped by clamp_row_bounds before use
  int64_t row_begin = 0, row_end = INT64_MAX - 1;
};
// GenomicsDBImportConfig::fix_callset_row_idx_bounds of the reference (genomicsdb_config_base.cc:167-180): negative -> 0, swapped when
// reversed, the upper bound capped at the mapping's largest row (max_row < 0: not known, no cap)
inline void clamp_row_bounds(int64_t* lb, int64_t* ub, int64_t max_row) {
  if (*lb < 0) *lb = 0;
  if (*ub < 0) *ub = 0;
  if (*ub < *lb) { const int64_t t = *lb; *lb = *ub; *ub = t; }
  if (max_row >= 0 && *ub > max_row) *ub = max_row;
}
inline ImportOptions with_clamped_row_bounds(const ImportOptions& opt, const VidMapper& vid) {
  ImportOptions o = opt;
  int64_t max_row = -1;
  for (const CallSetInfo& cs : vid.get_callsets()) if (cs.m_row_idx > max_row) max_row = cs.m_row_idx;
  clamp_row_bounds(&o.row_begin, &o.row_end, max_row);
  return o;
}
inline bool row_in_bounds(const ImportOptions& opt, int64_t row) { return row >= opt.row_begin && row <= opt.row_end; }
struct ImportStats {
  int64_t num_files = 0, num_records = 0, num_cells = 0, num_spanning_cells = 0; uint64_t num_bytes = 0;   // num_spanning_cells: intervals replayed at the partition begin
  // device path only
  int64_t num_deferred_values = 0;     // numeric tokens outside the device's exact fast path, parsed by the host functions
  int64_t num_batches = 0; uint64_t text_bytes = 0;
  float ms_index = 0, ms_measure = 0, ms_write = 0, ms_sort_gather = 0;      // HIP-event time per phase, summed over the batches
  double s_read = 0, s_h2d = 0, s_deferred = 0, s_d2h = 0, s_total = 0;     // wall clock: file read + inflate, text upload, host parsing of deferred tokens, result download
  // BGZF input of the device path (kernels/gdb_inflate.hip)
  uint64_t compressed_bytes = 0;       // bytes of the input files as they are on disk
  int64_t num_device_members = 0;      // BGZF members inflated on the device
  int64_t num_host_inflated_files = 0; // files inflated whole on the host (not BGZF, or inflate_mode = host)
  float ms_inflate = 0;                // HIP-event time of the inflate kernel
  uint64_t bytes_h2d = 0;              // input bytes uploaded: text (host inflate) or compressed members, their descriptors and the header member's tail
};

// every callset of vid's callset mapping (file, idx_in_file, row_idx); cells in column-major (column, row) order
std::vector<uint8_t> import_callsets_to_cells(const VidMapper& vid, const ImportOptions& opt, ImportStats* stats = nullptr);

// The same bytes, made on GPU `device` (kernels/gdb_import.hip): the host reads the files and maps the samples, the device
// inflates BGZF input, indexes, measures, writes, sorts and gathers the cells.  text_budget_bytes: record text per batch (0: default).
// inflate_mode: 0 BGZF files are inflated on the device and every other file on the host, 1 always on the host, 2 a file that is
// not BGZF is an error.  Refuses, before any launch, 2-dimensional fields, flattened tuple elements and what
// import_callsets_to_cells refuses; a BGZF member whose stream, ISIZE or CRC32 is wrong refuses the file.
// BCF2 files (sniffed by content, plain or compressed) are imported too; compressed BCF2 is inflated on the host and is an error in
// inflate_mode 2.  streams: a callset file whose "filename" equals a stream's name is read from that memory instead (VCF text or
// BCF2, plain or gzip); a stream that no callset names is an error.  A file or stream that the callset mapping lists as a CSV cell
// file is read as one (one line = one cell; not replayed at a partition begin; compressed content is refused).
struct ImportStream { std::string name; const void* data = nullptr; uint64_t nbytes = 0; };
std::vector<uint8_t> import_callsets_to_cells_device(const VidMapper& vid, const ImportOptions& opt, int device, uint64_t text_budget_bytes,
                                                     ImportStats* stats = nullptr, int inflate_mode = 0,
                                                     const std::vector<ImportStream>& streams = std::vector<ImportStream>());

// Incremental import: k >= 1 streams of begin-cells in host memory, each sorted by (column, row) as an importer or a cells.bin gives
// them, become one stream in that order on GPU `device` (kernels/gdb_merge.hip; the reference's "new fragment, then
// consolidate_tiledb_array").  Schema-agnostic: only the 24-byte header of a cell is read, payloads move as opaque bytes.  Refused
// (VCF2BinaryException, nothing returned): a size chain that runs past its stream's end (stream, byte offset), a stream that is not
// sorted (stream, cell index), a negative row, and a row that two streams share (the smallest one) - the batches of an incremental
// import have disjoint rows, so there are no key ties across streams; equal keys inside one stream keep their order.  Inputs, keys and
// the result must fit in the device's free memory together (refused with the sizes otherwise).  No device: GenomicsDBDeviceException.
struct CellStream { const void* data = nullptr; uint64_t nbytes = 0; };
struct MergeStats {
  int64_t num_streams = 0, cells_in = 0, cells_out = 0; uint64_t bytes_out = 0;
  int64_t tile = 0;                                        // output cells per workgroup of the rank kernel
  float ms_keys = 0, ms_rank = 0, ms_scan = 0, ms_gather = 0;   // HIP-event time: keys + checks, merge-path rank rounds, size scatter + scan, gather
  double s_h2d = 0, s_d2h = 0, s_total = 0;                // wall clock
};
std::vector<uint8_t> merge_cell_streams_device(const std::vector<CellStream>& streams, int device, MergeStats* stats = nullptr);

// The same merge from files to a file, for arrays larger than device memory (kernels/gdb_merge.hip, host/merge_files_common.hpp): the
// sources - files of begin-cells, read with pread, or memory - are merged round by round through pinned staging and device pools
// bounded by `window_bytes`, and the output, byte for byte what merge_cell_streams_device gives, is written to <output_path>.merge.tmp
// and renamed to output_path on success.  A round loads whole cells of every source up to its share of the window, emits the cells
// strictly below the smallest last-loaded key of the sources not yet exhausted (the watermark) and carries the rest; a round that can
// emit nothing doubles the share of the sources that hold the watermark (`grown`).  window_bytes caps the input cell bytes resident on
// the device (carried + fresh, over all sources; growth aside; every source gets the same share of it, but no more than it is long);
// 0: a sixteenth of the free device memory, at most 64 MiB, the fastest window measured (profiles/device_merge_files.md).  Peak device
// memory is about 8.7 x window_bytes (two pools, the output buffer, 136 bytes of tables per 24 bytes of pool - the smallest cell) plus
// the row bitmaps (sources x largest row / 8 bytes); pinned host memory is 4.7 x window_bytes; neither depends on the sources' lengths.
// Refusals keep the words of the in-core merge; cell indices and byte offsets count from the start of the source.  The shared row
// named is the smallest one known in the round that first finds one (the in-core merge sees all rows at once and names the smallest
// of all).  After a refusal neither output_path (when it did not exist) nor the temporary file is left.  Returns the number of cells.
struct CellSource { std::string path; const void* data = nullptr; uint64_t nbytes = 0; };      // a file when path is not empty, else memory
struct MergeFilesOptions { int device = 0; uint64_t window_bytes = 0; };
struct MergeFilesStats : MergeStats {        // (s_h2d, s_d2h stay 0: the transfers overlap the kernels; ms_gather includes the wait for the previous round's download)
  int64_t rounds = 0, carried_cells = 0, grown = 0;       // carried_cells: summed over the rounds
  uint64_t window_bytes = 0, device_bytes_peak = 0, pinned_bytes = 0;      // the window as used (after growth: the sum of the shares)
  double s_read = 0, s_write = 0, s_wait_device = 0;      // wall clock of the host thread: refills, writes, waiting for the device
};
uint64_t merge_cell_files_device(const std::vector<CellSource>& sources, const std::string& output_path, const MergeFilesOptions& options, MergeFilesStats* stats = nullptr);

// the importer's number parsers (strtoll / strtod over the whole token, VCF2BinaryException otherwise): the device path runs
// them on the tokens it deferred
int64_t import_parse_int(const char* p, size_t n, const std::string& what);
double import_parse_double(const char* p, size_t n, const std::string& what);
// the CSV reader's (reference include/vcf/vcf.h:238-313): strtoll(token, &end, 0) / strtof(token, &end) over a PREFIX of the token -
// leading whitespace, a sign, 0x and 0 prefixes, trailing text ignored - and VCF2BinaryException when nothing can be parsed
int64_t import_csv_parse_int(const char* p, size_t n, const std::string& what);
float import_csv_parse_float(const char* p, size_t n, const std::string& what);

}  // namespace genomicsdb_amd
