// gdb_import.h - the device importer: (g)VCF record text -> begin-cells on one GPU (host-visible interface, no HIP types).
//
// The host reads a file, maps its samples to rows from the #CHROM line and hands the record text over in batches of at most
// `text_budget_bytes`, cut at a newline.  A BGZF file crosses the link compressed: only the members that hold the header are
// inflated on the host, the rest on the device (kernels/gdb_inflate.hip), in windows of about one text budget; every other file is
// inflated on the host and its text uploaded.  Per batch the device indexes newlines and tabs, measures one cell per
// (record line, imported sample), lays the cells out by a scan and writes them - the bodies of core/gdb_import.hpp, the same
// bytes as host/vcf_importer.cc.  BCF2 input (a file or a stream in memory, sniffed by content; compressed BCF2 is inflated on the
// host) takes the same path with another index pass: the host walks the l_shared / l_indiv chain and cuts batches at record
// boundaries, the device indexes each record once (core/gdb_import_bcf.hpp) and measures and writes per (record, sample).
// finish() resolves the intervals that span the partition begin, sorts all cells by
// (column, row) with ties in append order, gathers them into column-major order and copies the result out once.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../host/vcf_importer.h"
#include "../host/vid_mapper.h"

namespace genomicsdb_amd {

namespace gdbimp { struct ImpTables; struct ImpBcfTables; }      // core/gdb_import.hpp, core/gdb_import_bcf.hpp

// A text tap takes the importer's batches in place of the cells (kernels/gdb_split.hip, kernels/gdb_histogram.hip): the same files, windows, batch cuts and
// newline / tab index, then on_batch instead of measure and write.  Every pointer of a batch is device memory that is valid until
// on_batch returns; the index is queued on `stream` (a hipStream_t), on which on_batch queues its own work.
struct ImportTextBatch {
  const std::string* path;                      // the file, for messages
  const char* d_text;                           // n_bytes of whole lines (the last one ends with a newline), padded for 16-byte loads
  const uint32_t* d_nl; const uint32_t* d_first_tab; const uint32_t* d_tab;      // the index: newline positions, tabs in front of a line, tab positions
  uint32_t n_bytes, n_lines;
  int64_t lines_before;                         // physical lines of the file in front of the batch
  const gdbimp::ImpTables* tables;              // the contigs of the vid, in device memory (the struct itself is the host's)
  void* stream;
  std::function<std::string(uint32_t bit, uint32_t line)> describe;      // the words of an ImpErr bit raised on a line of the batch
};
// The same for a batch of BCF2 records (kernels/gdb_histogram.hip): the bytes as the host's walk of the l_shared / l_indiv chain cut
// them, record r in [d_rec_off[r], d_rec_off[r + 1]); then on_records instead of the index pass, measure and write.
struct ImportRecordBatch {
  const std::string* path;                      // the file or stream, for messages
  const uint8_t* d_bytes; const uint32_t* d_rec_off;      // n_bytes of whole records; n_rec + 1 offsets
  uint32_t n_bytes, n_rec;
  int64_t records_before;                       // records of the file in front of the batch
  const gdbimp::ImpBcfTables* bcf_tables;       // the header's dictionaries against the vid, in device memory (the struct itself is the host's)
  void* stream;
  std::function<std::string(uint32_t bit, uint32_t rec)> describe;       // the words of an error bit raised on a record of the batch
};
struct ImportTextTap {
  std::function<void(const std::string& path, const std::string& head)> on_header;      // a file's lines in front of its first record line
  std::function<void(const ImportTextBatch&)> on_batch;
  std::function<void(const ImportRecordBatch&)> on_records;      // unset: BCF2 input is refused by name
};

class DeviceImporter {
 public:
  static constexpr uint64_t kDefaultTextBudget = (uint64_t)64 << 20;
  // refuses (VCF2BinaryException) what the bodies do not cover before anything is launched
  enum { kInflateAuto = 0, kInflateHost = 1, kInflateDevice = 2 };      // BGZF on the device else the host; always the host; a file that is not BGZF is an error
  // tap: see ImportTextTap; with one, only the contigs of the vid are needed (no field is refused), finish() has nothing to give
  DeviceImporter(int device, const VidMapper& vid, const ImportOptions& opt, uint64_t text_budget_bytes = 0, int inflate_mode = kInflateAuto,
                 const ImportTextTap* tap = nullptr);
  ~DeviceImporter();
  DeviceImporter(const DeviceImporter&) = delete;
  DeviceImporter& operator=(const DeviceImporter&) = delete;
  // every file of the callset mapping, in mapping order: append_buffer where a stream has the file's name, else append_file
  void import_all(const std::vector<ImportStream>& streams = std::vector<ImportStream>());
  // a "filename" of the callset mapping.  The content decides: VCF text or BCF2 ('BCF\2\1' / 'BCF\2\2'), plain, gzip or BGZF
  void append_file(const std::string& filename);
  // with a tap: a file of VCF text (plain, gzip or BGZF) by its path, in the callset mapping or not
  void append_text_path(const std::string& path);
  // the same from memory (the buffer-stream input of the reference's importer): `name` is a "filename" of the callset mapping whose
  // content is the nbytes at ptr, sniffed like a file's
  void append_buffer(const std::string& name, const void* ptr, uint64_t nbytes);
  void finish(std::vector<uint8_t>& cells);
  const ImportStats& stats() const;
 private:
  friend class DeviceStreamImporter;      // kernels/gdb_import_stream.h: the same batches, emitted batch by batch
  struct Impl;
  Impl* m_;
};

}  // namespace genomicsdb_amd
