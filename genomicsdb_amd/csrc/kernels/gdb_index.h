// gdb_index.h - the tabix index (.tbi) of bgzipped VCF text, built on the device (host-visible interface, no HIP types).  The rule is
// the host builder's (host/vcf_index.cc), restated per record in core/gdb_index.hpp; the file is the host builder's, byte for byte.
//
// Per batch of whole lines in device memory (all launches on one stream):
//   lines     the importer's newline / tab index pass (impdev::index_lines: k_imp_count, scan, k_imp_scatter)
//   select    k_idx_select: one thread per line, is it a record -> rocPRIM exclusive scan -> k_idx_compact: record -> line
//   records   k_idx_records: one thread per record: interval, bin, windows, the two virtual offsets (a binary search in the table of
//             the file's BGZF members), error bits with the smallest offending line, and is its CHROM another one than the
//             record's in front (a run head).  A scan numbers the runs, k_idx_head_names packs the heads' names, the host gives
//             every run its contig id (first appearance; a name that comes back gets its old id)
//   chunks    stable rocPRIM radix sort by contig id; k_idx_chunk_heads: contig or bin differ from the neighbour in front -> scan ->
//             k_idx_chunks: {vbeg of the head, vend of the last record, records}; stable radix sort of the chunks by (contig id, bin)
//   linear    k_idx_window_extent: largest window per contig; k_idx_windows: one thread per record in contig order loops over its
//             windows and issues a 64-bit atomicMin only where the lane in front does not cover the window too
// The host joins the batches (TbiBatchMerger), fills the empty windows, lays the bytes out and compresses them (write_tbi_index).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace genomicsdb_amd {

struct IndexStats {
  int64_t members = 0;                         // BGZF members of the file, the empty ones included
  int64_t batches = 0, lines = 0, records = 0;
  int64_t contigs = 0, bins = 0, chunks = 0, linear_windows = 0;      // of the index as written (bins without the meta bin)
  uint64_t text_bytes = 0;                     // inflated bytes
  int64_t atomics = 0;                         // atomicMin issued on the window minima
  double ms_inflate = 0, ms_index = 0, ms_records = 0, ms_chunks = 0, ms_linear = 0;      // HIP-event time per phase, summed over the batches
  double s_read = 0, s_serialize_write = 0, s_total = 0;      // wall clock: file read, merge + layout + compress + write, all
};

// the members that hold data, in file order; v_total: the virtual offset of a position at or behind `total`
struct IndexMemberTable { std::vector<uint64_t> ubase, coff; uint64_t total = 0, v_total = 0; };

// The batches of one file.  `stream`: a hipStream_t on which every launch is queued; every call returns with the stream idle.
class DeviceTbiBuilder {
 public:
  DeviceTbiBuilder(const std::string& path_for_messages, void* stream);
  ~DeviceTbiBuilder();
  DeviceTbiBuilder(const DeviceTbiBuilder&) = delete;
  DeviceTbiBuilder& operator=(const DeviceTbiBuilder&) = delete;
  // the table the next batches look their virtual offsets up in.  v_total == kPending: the offset behind the text is not known yet,
  // resolve_pending names it before the next batch or finish
  static constexpr uint64_t kPending = ~(uint64_t)0;
  void set_members(const IndexMemberTable& table);
  void resolve_pending(uint64_t voff);
  // n bytes at d_text (device memory, 16-byte aligned, 64 bytes allocated behind them) that begin at a line start, the first one at
  // uncompressed position u_text of the file.  The whole lines among them are the batch: -> the bytes used, up to and with the last
  // newline (0: no newline, nothing was done).  A refused record throws with the file and the 1-based line
  uint32_t add_batch(const char* d_text, uint32_t n, uint64_t u_text);
  void finish(const std::string& tbi_path);      // writes the index
  // another file: nothing of the last one is kept but the device buffers.  lines_before: lines of the file that no batch will hold
  void reset(const std::string& path_for_messages, int64_t lines_before = 0);
  IndexStats st;
 private:
  struct Impl;
  Impl* m_;
};

// <path>.tbi of a bgzipped VCF, through a temporary name: an error leaves no .tbi behind.  -> the index path.  Refused: a file that is
// not a BGZF chain from its first byte to its last (with the byte offset where the chain breaks), a member with a bad stream, ISIZE or
// CRC32 (as the device inflater words it), a record with POS < 1 or POS / END >= 2^31 (file and 1-based line).  No device: no CPU path.
std::string index_vcf_device(const std::string& path, int device, uint64_t text_budget_bytes, IndexStats* stats = nullptr);

}  // namespace genomicsdb_amd
