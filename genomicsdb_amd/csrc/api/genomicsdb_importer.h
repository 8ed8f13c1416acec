// genomicsdb_importer.h - GenomicsDBImporter: the reference's batch-wise import of buffer streams
// (src/main/cpp/include/loader/genomicsdb_importer.h:46-144), on one GPU with bounded device memory.
//
//   GenomicsDBImporter imp(loader_json_file, rank);
//   imp.add_buffer_stream(name, VCF_BUFFER_STREAM | BCF_BUFFER_STREAM, capacity, header_bytes, n);   // once per stream
//   imp.setup_loader(callsets_json_string);          // callsets of the string join those of the loader's callset_mapping_file
//   while (!imp.is_done()) {
//     imp.import_batch();
//     for (id : imp.get_exhausted_buffer_stream_identifiers()) imp.write_data_to_buffer_stream(id.first, id.second, data, n);
//   }                                                // a stream ends by a write of 0 bytes, or by no write at all
//   imp.finish();
//
// The loader JSON is read as vcf2tiledb reads it (vid and callset files, column_partitions[rank], treat_deletions_as_intervals,
// lb_/ub_callset_row_idx); the device is GDBAMD_DEVICE, else LOCAL_RANK, else 0.  kernels/gdb_import_stream.h has the batch rules:
// what a batch hands over, and which streams it reports exhausted.  finish() makes the loader's outputs (api/loader_outputs.h); with
// "produce_tiledb_array" alone the cells go to <array>/cells.bin.import.tmp batch by batch and are renamed over cells.bin in
// finish(), so device AND host memory stay bounded; a combined VCF, a merge into an existing array and a compressed fragment take
// the cells whole, and then every batch is also kept in host memory until finish().
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace genomicsdb_amd {

class GenomicsDBImporterException : public std::runtime_error {
 public:
  explicit GenomicsDBImporterException(const std::string& m) : std::runtime_error("GenomicsDBImporterException : " + m) {}
};

enum VidFileTypeEnum { VCF_BUFFER_STREAM_TYPE = 0, BCF_BUFFER_STREAM_TYPE = 1 };
typedef std::pair<int64_t, unsigned> BufferStreamIdentifier;      // (buffer stream index, partition index)
struct StreamImportStats;

class GenomicsDBImporter {
 public:
  // device < 0: from the environment
  GenomicsDBImporter(const std::string& loader_config_file, int rank, int device = -1);
  GenomicsDBImporter(const GenomicsDBImporter&) = delete;
  GenomicsDBImporter& operator=(const GenomicsDBImporter&) = delete;
  GenomicsDBImporter(GenomicsDBImporter&& other);
  ~GenomicsDBImporter();
  void add_buffer_stream(const std::string& name, VidFileTypeEnum buffer_stream_type, size_t capacity) { add_buffer_stream(name, buffer_stream_type, capacity, nullptr, 0); }
  void add_buffer_stream(const std::string& name, VidFileTypeEnum buffer_stream_type, size_t capacity, const uint8_t* initialization_buffer,
                         size_t num_bytes_in_initialization_buffer);
  void setup_loader(const std::string& buffer_stream_callset_mapping_json_string = "");
  const std::vector<int64_t>& get_buffer_stream_idx_to_global_file_idx_vec() const;
  size_t get_max_num_buffer_stream_identifiers() const;
  void write_data_to_buffer_stream(int64_t buffer_stream_idx, unsigned partition_idx, const uint8_t* data, size_t num_bytes);
  void import_batch();
  const std::vector<BufferStreamIdentifier>& get_exhausted_buffer_stream_identifiers() const;
  bool is_done() const;
  void finish();
  // this build's additions
  const std::vector<uint8_t>& last_batch_cells() const;      // what the last import_batch handed over
  const StreamImportStats& stats() const;
 private:
  struct Impl;
  Impl* m_;
};

// The file import of a loader JSON on the device, then the loader's outputs: what `vcf2tiledb --import-on-device <loader.json>` does
// (the reference's VCF2TileDBLoader::read_all behind jniGenomicsDBImporter).  device < 0: from the environment
void import_files_of_loader(const std::string& loader_config_file, int rank, int device = -1);

// {"contigs":[{"<name>":[begin,end]},...]}: the 1-based intervals of the contigs that column partition `rank` of the loader JSON (a path, or
// the JSON itself) covers, in column order (reference VidMapper::get_contig_intervals_for_column_partition, vid_mapper.cc:576-609)
std::string chromosome_intervals_for_column_partition(const std::string& loader_config_file, int rank);

}  // namespace genomicsdb_amd
