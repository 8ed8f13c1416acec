// gdb_import_stream.h - the streaming device importer: buffer streams of VCF text or BCF2 records, imported batch by batch with
// bounded device memory (host-visible interface, no HIP types).
//
// The caller writes whole records into the buffers of its streams and calls import_batch().  A batch converts every byte of every
// buffer with the kernels of the device importer (kernels/gdb_import.hip), checks that each stream's columns do not go back, and
// hands over, in column-major order, every pending cell whose column lies strictly below W = the smallest last delivered column over
// the streams that have not ended.  The other cells stay in device memory; the streams whose last column is not above W are reported
// exhausted and must be refilled (or ended by an empty write, or by no write).  Concatenated over the batches, the cells are those of
// DeviceImporter::finish() - and of the host importer - on the same records.  core/gdb_import_stream.hpp has the per-slot rules.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../host/vcf_importer.h"
#include "../host/vid_mapper.h"

namespace genomicsdb_amd {

struct BufferStreamDecl {
  std::string name; bool is_bcf = false; size_t capacity = 0;
  std::vector<uint8_t> init;      // the header (VCF text through the #CHROM line, or BCF\2\2 + l_text + text); records behind it are the first write
};
struct StreamImportStats {
  int64_t num_batches = 0, num_records = 0, num_cells = 0; uint64_t num_bytes = 0;      // import_batch calls; records read; cells and bytes handed over
  int64_t max_pending_cells = 0; uint64_t max_pending_bytes = 0;      // the most a batch held before it emitted: cells carried over (16-byte aligned in their pool) + cells of the new writes
  int64_t num_deferred_values = 0, num_spanning_cells = 0;
  float ms_order = 0, ms_classify = 0, ms_sort_gather = 0, ms_compact = 0;      // HIP-event time, summed over the batches
  double s_h2d = 0, s_d2h = 0;                                                      // wall clock
};

class DeviceStreamImporter {
 public:
  // vid: the vid mapping with ALL callsets (those of the streams included); a callset names its stream where a file's callset names
  // its "filename".  Parses the headers; refuses what DeviceImporter refuses
  DeviceStreamImporter(int device, const VidMapper& vid, const ImportOptions& opt, const std::vector<BufferStreamDecl>& streams);
  ~DeviceStreamImporter();
  DeviceStreamImporter(const DeviceStreamImporter&) = delete;
  DeviceStreamImporter& operator=(const DeviceStreamImporter&) = delete;
  // stream -> index of its name among the sources of the callset mapping, in order of first appearance; -1: no callset inside the row bounds uses it
  const std::vector<int64_t>& stream_file_idx() const;
  size_t num_used_streams() const;
  void write(int64_t stream_idx, unsigned partition_idx, const uint8_t* data, size_t nbytes);
  void import_batch(std::vector<uint8_t>& cells);      // cells: what this batch hands over
  const std::vector<std::pair<int64_t, int>>& exhausted() const;      // (stream, partition 0), ascending, after import_batch
  bool is_done() const;
  void finish();      // only when done: frees the pools
  const StreamImportStats& stats() const;
 private:
  struct Impl;
  Impl* m_;
};

}  // namespace genomicsdb_amd
