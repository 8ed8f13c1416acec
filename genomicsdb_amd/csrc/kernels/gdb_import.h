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
#include <string>
#include <vector>

#include "../host/vcf_importer.h"
#include "../host/vid_mapper.h"

namespace genomicsdb_amd {

class DeviceImporter {
 public:
  static constexpr uint64_t kDefaultTextBudget = (uint64_t)64 << 20;
  // refuses (VCF2BinaryException) what the bodies do not cover before anything is launched
  enum { kInflateAuto = 0, kInflateHost = 1, kInflateDevice = 2 };      // BGZF on the device else the host; always the host; a file that is not BGZF is an error
  DeviceImporter(int device, const VidMapper& vid, const ImportOptions& opt, uint64_t text_budget_bytes = 0, int inflate_mode = kInflateAuto);
  ~DeviceImporter();
  DeviceImporter(const DeviceImporter&) = delete;
  DeviceImporter& operator=(const DeviceImporter&) = delete;
  // every file of the callset mapping, in mapping order: append_buffer where a stream has the file's name, else append_file
  void import_all(const std::vector<ImportStream>& streams = std::vector<ImportStream>());
  // a "filename" of the callset mapping.  The content decides: VCF text or BCF2 ('BCF\2\1' / 'BCF\2\2'), plain, gzip or BGZF
  void append_file(const std::string& filename);
  // the same from memory (the buffer-stream input of the reference's importer): `name` is a "filename" of the callset mapping whose
  // content is the nbytes at ptr, sniffed like a file's
  void append_buffer(const std::string& name, const void* ptr, uint64_t nbytes);
  void finish(std::vector<uint8_t>& cells);
  const ImportStats& stats() const;
 private:
  struct Impl;
  Impl* m_;
};

}  // namespace genomicsdb_amd
