// gdb_output_index.h - the index of the combined output, built on the device page by page: .tbi next to a "z" stream, .csi next to a
// "b" stream (host-visible interface, no HIP types).  The file is the one build_tbi_index / build_csi_index (host/vcf_index.cc) write
// when they re-read the finished file, byte for byte; the bodies are core/gdb_output_index.hpp.
//
// Per page, everything is queued on the pipeline's stream (DevicePipeline::PageIndexSink, called from begin_page):
//   records   BEFORE the deflate overwrites the page: k_oidx_text_records / k_oidx_bcf_records, one thread per record of the page's
//             record offsets: interval, bin, windows, contig (position among the header's contigs), the record's uncompressed begin
//             and end offset in the page, error bits with the smallest offending record
//   voff      BEHIND the deflate: k_oidx_voff turns the two offsets into page-relative virtual offsets with the compressor's block
//             offsets (BgzfDeviceCompressor::block_offsets)
// and once the page's compressed size is known (merge_page, after finish_page):
//   chunks    stable rocPRIM radix sort by contig; k_oidx_chunk_heads: contig or bin differ from the neighbour in front -> scan ->
//             k_oidx_chunk_firsts, k_oidx_chunks: {vbeg of the head, vend of the last record, records}
//   linear    k_oidx_window_extent: largest window per contig; k_oidx_windows: one thread per record in contig order loops over its
//             windows and issues a 64-bit atomicMin only where the lane in front does not cover the window too
// The host adds the page's file offset, joins the pages (TbiBatchMerger) and writes (write_tbi_index / write_csi_index).  The vend of
// a page's last record is the first block of the next page - or, for the stream's last page, the file's size with its EOF block -
// so it stays pending (TbiBatchMerger::resolve_pending) until the next page or write() names it.
//
// Device memory: two sets of record tables (one per page arena), each reused page after page and grown to the largest page:
// 52 bytes per record of the page (two 64-bit offsets; bin, first and last window, contig = the sort's key, the record's number = its
// value; key and value sorted; chunk head flag, its scan) plus 36 bytes per chunk and 8 per 16 kb window of the page, and rocPRIM's
// scratch for the sort.  OutputIndexStats::table_bytes reports what is held.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "gdb_pipeline.h"

namespace genomicsdb_amd {

struct OutputIndexStats {
  int64_t pages = 0, records = 0;
  int64_t contigs = 0, bins = 0, chunks = 0, linear_windows = 0;      // of the index as written (bins without the meta bin)
  int64_t atomics = 0;                                                // atomicMin issued on the window minima
  double ms_records = 0, ms_voff = 0, ms_chunks = 0, ms_linear = 0;   // HIP-event time per phase, summed over the pages
  double s_write = 0;                                                 // wall clock: merge of the pages, layout, compression, file write
  uint64_t table_bytes = 0;                                           // device memory held by the record tables
};

class DeviceOutputIndexer : public DevicePipeline::PageIndexSink {
 public:
  // bcf: pages of BCF2 records (.csi), else VCF text (.tbi).  header_contigs: the IDs of the header's ##contig lines, in order (their
  // count is the .csi's n_ref).  header_compressed_bytes: what the stream holds in front of the first page (> 0).  header_lines: lines
  // of the header (text; for the line a refused record is reported at)
  DeviceOutputIndexer(bool bcf, const std::vector<std::string>& header_contigs, uint64_t header_compressed_bytes, int64_t header_lines);
  ~DeviceOutputIndexer() override;
  DeviceOutputIndexer(const DeviceOutputIndexer&) = delete;
  DeviceOutputIndexer& operator=(const DeviceOutputIndexer&) = delete;
  void page_records(int arena, const DevicePipeline::PageView& page, void* stream) override;
  void page_blocks(int arena, const uint64_t* d_boff, uint64_t nblocks, uint32_t block_input, void* stream) override;
  // the page of `arena` is complete and compressed_bytes long in the file: its chunks and windows join the pages before it.  Returns
  // with the stream idle.  A refused record throws
  void merge_page(int arena, uint64_t compressed_bytes);
  // the stream has ended (its EOF block follows the last page): writes the .tbi / .csi
  void write(const std::string& path);
  OutputIndexStats st;
  struct Impl;
 private:
  Impl* m_;
};

}  // namespace genomicsdb_amd
