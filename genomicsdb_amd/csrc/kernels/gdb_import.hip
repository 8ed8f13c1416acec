// gdb_import.hip - see gdb_import.h.  Kernels for gfx950 around the bodies of core/gdb_import.hpp, and their orchestration.
//
// Per batch of record text (all launches on one stream):
//   index    k_imp_count: newlines and tabs per 4 KiB tile -> rocPRIM exclusive scan of the tile counts -> k_imp_scatter: positions
//            of the newlines and the tabs plus, per line, the number of tabs in front of it, so (line, column k) -> byte offset is O(1)
//   measure  k_imp_measure: one thread per (line, imported sample): coordinates, partition filter, cell size, errors, the packed
//            atomicMax (column, line sequence number) per row for the partition-begin rule
//   layout   rocPRIM exclusive scan of the sizes
//   write    k_imp_write: the same grid emits the cells, the deferred-token list and the 64-bit sort key (column, row) per slot
// finish():  k_imp_resolve drops the spanning candidates that are not their row's choice, a stable rocPRIM radix sort of the keys
//            over the slots of all batches (slots are in the host importer's append order, so ties resolve as std::stable_sort
//            does), k_imp_gather copies the variable-size cells into column-major order, one copy to the host.
//
// Where the text comes from: a BGZF file (a valid chain of members from its first byte to its last, bgzf_walk) is read as it is; the
// host inflates only the leading members that hold the '#' lines, the rest goes to the device in WINDOWS of whole members
// (kernels/gdb_inflate.hip: one wavefront per member; stream, ISIZE and CRC32 of every member verified).  A window is [the
// partial line carried from the window before | the inflated members], about one text budget, floor one member; batches are cut
// inside it exactly as on the host - the last newline below the budget is found by k_imp_find_newlines - and copied, device to
// device, to the aligned and padded d_text the kernels above read.  The bytes behind a window's last newline are carried to the
// front of the next one, so a batch never crosses a window: with the same budget, num_batches can be larger than for the same text
// inflated on the host (the cells do not depend on where batches are cut), and each cut costs one small launch and round trip.  Every other file (plain text, plain gzip, a chain that breaks) is inflated by gz_text::read_all and
// its text uploaded, as before.
//
// BCF2 input (a file or a buffer whose inflated bytes begin with 'BCF\2\1' / 'BCF\2\2'; compressed BCF2 is inflated on the host, because
// records cross BGZF members): the host parses the header and walks the l_shared / l_indiv chain (host/import_bcf.hpp), cuts batches at
// record boundaries and uploads the bytes and the record offsets; k_imp_bcf_index - one thread per record - takes the place of the
// newline / tab index and leaves a table per record (core/gdb_import_bcf.hpp); measure, write and finish() are the kernels above,
// instantiated over ImpBcfSrc instead of ImpTextSrc, one thread per (record, imported sample).
//
// CSV cell files (the callset mapping's "sorted_csv_files" / "unsorted_csv_files"; core/gdb_import_csv.hpp): the text path's newline
// index, batch cuts, LDS staging, key sort and gather, instantiated over ImpCsvSrc.  A line is one slot and names its own row, which
// is looked up in the ascending table of the file's rows; its slots carry no partition-begin tag, so k_imp_resolve leaves them alone
// (and is not launched when no other source queued a batch).  Both passes walk the line's tokens: there is no per-line token index,
// see profiles/device_import_csv.md.
#include "gdb_import.h"

#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <zlib.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <type_traits>

#include "../common/gz_text.hpp"
#include "../host/import_bcf.hpp"
#include "../host/import_common.hpp"
#include "gdb_import_device.hpp"
#include "gdb_import_impl.hpp"
#include "gdb_inflate.h"
#include "gdb_pipeline.h"

namespace genomicsdb_amd {

namespace {
using namespace gdbimp;
using namespace impdev;

constexpr uint64_t kDroppedKey = ~(uint64_t)0;

// counts of one thread's 16 bytes: newlines in the high word, tabs in the low word
__device__ __forceinline__ uint64_t imp_count16(const char* text, uint32_t n, uint64_t at, uint4* bytes) {
  *bytes = *reinterpret_cast<const uint4*>(text + at);     // (the buffer is padded: at + 16 <= n + kTextPad)
  const uint8_t* b = reinterpret_cast<const uint8_t*>(bytes);
  uint32_t nl = 0, tab = 0;
#pragma unroll
  for (int i = 0; i < kBytesPerThread; ++i) {
    const bool in = at + (uint64_t)i < (uint64_t)n;
    nl += in && b[i] == '\n';
    tab += in && b[i] == '\t';
  }
  return ((uint64_t)nl << 32) | tab;
}

__global__ void __launch_bounds__(kBlock) k_imp_count(const char* text, uint32_t n, uint64_t* tile_counts) {
  __shared__ unsigned long long s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const uint64_t at = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kBytesPerThread;
  uint64_t c = 0;
  uint4 bytes;
  if (at < n) c = imp_count16(text, n, at, &bytes);
  if (c) atomicAdd(&s_count, (unsigned long long)c);
  __syncthreads();
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = s_count;
}

__global__ void __launch_bounds__(kBlock) k_imp_scatter(const char* text, uint32_t n, const uint64_t* tile_base, uint32_t* nl_pos, uint32_t* line_first_tab,
                                                       uint32_t* tab_pos, uint32_t n_lines, uint32_t n_tabs) {
  __shared__ uint64_t s_scan[kBlock];
  const uint64_t at = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kBytesPerThread;
  uint4 bytes = make_uint4(0, 0, 0, 0);
  const uint64_t mine = at < n ? imp_count16(text, n, at, &bytes) : 0;
  s_scan[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {       // inclusive scan over the block
    const uint64_t add = (int)threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += add;
    __syncthreads();
  }
  if (!mine) return;
  const uint64_t before = tile_base[blockIdx.x] + s_scan[threadIdx.x] - mine;
  uint32_t nl = (uint32_t)(before >> 32), tab = (uint32_t)before;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(&bytes);
  for (int i = 0; i < kBytesPerThread; ++i) {
    if (at + (uint64_t)i >= (uint64_t)n) break;
    if (b[i] == '\n') { if (nl < n_lines) { nl_pos[nl] = (uint32_t)at + i; line_first_tab[nl + 1u] = tab; } ++nl; }
    else if (b[i] == '\t') { if (tab < n_tabs) tab_pos[tab] = (uint32_t)at + i; ++tab; }
  }
}

// where a batch is cut: out[0] = 1 + position of the last newline in [lo, mid) (0: none), out[1] = position of the first newline in
// [mid, hi) (all ones: none); one thread per byte of [lo, hi), one atomic per wavefront and side
__global__ void __launch_bounds__(kBlock) k_imp_find_newlines(const char* text, uint64_t lo, uint64_t mid, uint64_t hi, unsigned long long* out) {
  const uint64_t i = lo + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool nl = i < hi && text[i] == '\n';
  const bool below = nl && i < mid, above = nl && i >= mid;
  const unsigned long long b = __ballot(below), a = __ballot(above);
  const uint32_t lane = threadIdx.x & 63u;
  if (below && lane == 63u - (uint32_t)__clzll((long long)b)) atomicMax(&out[0], (unsigned long long)i + 1ull);
  if (above && lane == (uint32_t)__ffsll((unsigned long long)a) - 1u) atomicMin(&out[1], (unsigned long long)i);
}
// a line that begins with "#CHROM" (the caller's text begins at a line start)
__global__ void __launch_bounds__(kBlock) k_imp_find_chrom(const char* text, uint64_t n, uint32_t* found) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i + 6u > n || text[i] != '#' || (i > 0 && text[i - 1u] != '\n')) return;
  if (text[i + 1u] == 'C' && text[i + 2u] == 'H' && text[i + 3u] == 'R' && text[i + 4u] == 'O' && text[i + 5u] == 'M') *found = 1u;
}

struct ImpSamples { const int32_t* file_idx; const int64_t* row; int32_t n; };    // imported samples of the file
struct ImpSpan { unsigned long long* row_best; int32_t seq_bits; uint64_t line_seq_base; int64_t max_row; };   // row_best null: no partition begin

// Where the slots of a batch come from: record lines of text (index: newlines and tabs) or BCF2 records (index: k_imp_bcf_index).
// measure / write are the two passes of one slot; is_record: the line counts as a record.  A slot of text or BCF2 is one (line or
// record, imported sample of the file) and its row is the sample's; a slot of a CSV cell file is one line, which names its own row.
struct ImpPerSample {
  __device__ __forceinline__ uint32_t per_line(const ImpSamples& S) const { return S.n > 0 ? (uint32_t)S.n : 1u; }
  __device__ __forceinline__ int sample_of(const ImpSamples& S, uint32_t j) const { return S.n > 0 ? S.file_idx[j] : -1; }
  __device__ __forceinline__ int64_t row_of(const ImpSamples& S, uint32_t j) const { return S.n > 0 ? S.row[j] : -1; }
};
struct ImpTextSrc : ImpPerSample {
  ImpBatch B;
  __device__ __forceinline__ ImpSlot measure(const ImpTables& T, uint32_t line, int sample, bool* is_record) const {
    const ImpLine L = imp_line_of(B, line);
    *is_record = L.end > L.begin && B.text[L.begin] != '#';
    return imp_measure(T, L, sample);
  }
  __device__ __forceinline__ uint32_t write(const ImpTables& T, uint32_t line, int sample, int64_t* row, const ImpSlot& s, ImpSink<true>& o) const {
    return imp_write(T, imp_line_of(B, line), sample, *row, s, o);
  }
};
struct ImpBcfSrc : ImpPerSample {
  ImpBcfTables BT; const uint8_t* bytes; const ImpBcfRec* rec; const ImpBcfField* fld; uint32_t n_attr;
  __device__ __forceinline__ ImpSlot measure(const ImpTables& T, uint32_t r, int sample, bool* is_record) const {
    *is_record = true;
    return imp_bcf_measure(T, BT, bytes, rec[r], fld + (uint64_t)r * n_attr, sample);
  }
  __device__ __forceinline__ uint32_t write(const ImpTables& T, uint32_t r, int sample, int64_t* row, const ImpSlot& s, ImpSink<true>& o) const {
    return imp_bcf_write(T, BT, bytes, rec[r], fld + (uint64_t)r * n_attr, sample, *row, s, o);
  }
};
// a line of a CSV cell file (core/gdb_import_csv.hpp): the newline index of the text path finds it, both passes walk its tokens once
// (no per-line token index: profiles/device_import_csv.md), rows: the rows of the file's callsets, ascending
struct ImpCsvSrc {
  ImpBatch B; ImpCsvRows rows;
  __device__ __forceinline__ uint32_t per_line(const ImpSamples&) const { return 1u; }
  __device__ __forceinline__ int sample_of(const ImpSamples&, uint32_t) const { return 0; }
  __device__ __forceinline__ int64_t row_of(const ImpSamples&, uint32_t) const { return -1; }       // (the write pass reads it from the line)
  __device__ __forceinline__ ImpSlot measure(const ImpTables& T, uint32_t line, int, bool* is_record) const {
    const ImpLine L = imp_line_of(B, line);
    *is_record = L.end > L.begin;
    int64_t row;
    return imp_csv_measure(T, rows, L, &row);
  }
  __device__ __forceinline__ uint32_t write(const ImpTables& T, uint32_t line, int, int64_t* row, const ImpSlot& s, ImpSink<true>& o) const {
    return imp_csv_write(T, imp_line_of(B, line), s, o, row);
  }
};

// the index pass of a BCF2 batch: one thread per record walks the shared block and the FORMAT blocks once (core/gdb_import_bcf.hpp)
__global__ void __launch_bounds__(kBlock) k_imp_bcf_index(ImpTables T, ImpBcfTables BT, const uint8_t* bytes, uint32_t n_bytes, const uint32_t* rec_off, uint32_t n_rec,
                                                         ImpBcfRec* rec, ImpBcfField* fld, uint32_t n_attr) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  uint32_t b = rec_off[r], e = rec_off[r + 1u];
  if (e > n_bytes) e = n_bytes;       // (never, by the host's walk: no read leaves the batch)
  if (b > e) b = e;
  imp_bcf_index(T, BT, bytes, b, e, &rec[r], fld + (uint64_t)r * n_attr);
}

// one thread per (record line, imported sample); with no imported sample one thread per line, for the checks and the count
template <class Src>
__global__ void __launch_bounds__(kBlock) k_imp_measure(ImpTables T, Src src, ImpSamples S, ImpSpan P, uint64_t n_slots, int64_t* col, int64_t* end,
                                                       uint64_t* size, uint8_t* kind, uint32_t* err, unsigned long long* counters) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t per_line = src.per_line(S);
  bool is_record = false, is_cell = false;
  if (slot < n_slots) {
    const uint32_t line = (uint32_t)(slot / per_line), j = (uint32_t)(slot % per_line);
    const int sample = src.sample_of(S, j);
    bool record_line = false;
    const ImpSlot s = src.measure(T, line, sample, &record_line);
    is_record = j == 0u && record_line;
    if (s.err) imp_raise(err, s.err, line);
    else if (P.row_best && sample >= 0 && record_line && s.col <= T.column_end && s.col <= T.column_begin) {
      const int64_t row = src.row_of(S, j);
      if (row >= 0 && row <= P.max_row)
        atomicMax(&P.row_best[row], ((unsigned long long)s.col << P.seq_bits) | (unsigned long long)(P.line_seq_base + line + 1u));
    }
    col[slot] = s.col; end[slot] = s.end; size[slot] = s.err ? 0u : s.size; kind[slot] = s.err ? (uint8_t)IMP_SLOT_NONE : (uint8_t)s.kind;
    is_cell = !s.err && s.kind != IMP_SLOT_NONE;
  }
  const unsigned long long rec = __ballot(is_record), cel = __ballot(is_cell);
  if ((threadIdx.x & 63u) == 0u) {
    if (rec) atomicAdd(&counters[0], (unsigned long long)__popcll(rec));
    if (cel) atomicAdd(&counters[1], (unsigned long long)__popcll(cel));
  }
}

constexpr uint32_t kStageBytes = 64u << 10;   // LDS a block may stage its cells in (gfx950: 160 KiB per CU, so two blocks fit)

// The slots of a block are consecutive, so its cells are one contiguous byte range of the batch's cell buffer.  STAGE: the threads
// write their cells - byte by byte, as the bodies do - into LDS at the range's own alignment, and the block then stores the range
// with aligned dwords, consecutive lanes on consecutive words; a block whose cells do not fit writes them directly like STAGE = false
// (profiles/device_import.md has the A/B).
template <bool STAGE, class Src>
__global__ void __launch_bounds__(kBlock) k_imp_write(ImpTables T, Src from, ImpSamples S, ImpSpan P, uint64_t n_slots, const int64_t* col, const int64_t* end,
                                                     const uint64_t* size, const uint8_t* kind, const uint64_t* off, uint8_t* cells, uint64_t cells_bytes,
                                                     ImpDeferred* def, uint32_t* ndef, uint32_t def_cap, uint64_t* key_out, uint64_t* src_out, uint32_t* size_out,
                                                     uint64_t* tag_out, uint32_t* err) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[STAGE ? kStageBytes : 16];
  const uint64_t first = (uint64_t)blockIdx.x * kBlock;
  const uint64_t last = first + kBlock < n_slots ? first + kBlock : n_slots;        // (first < n_slots by the grid)
  const uint64_t block_base = off[first], block_end = off[last];
  const uint32_t pad = (uint32_t)(block_base & 3u);
  const bool staged = STAGE && block_end <= cells_bytes && block_end - block_base + pad <= (uint64_t)kStageBytes;
  const uint64_t slot = first + threadIdx.x;
  if (slot < n_slots) {
    const uint32_t per_line = from.per_line(S);
    const uint32_t line = (uint32_t)(slot / per_line), j = (uint32_t)(slot % per_line);
    const int sample = from.sample_of(S, j);
    uint64_t key = kDroppedKey, tag = 0, src = 0;
    uint32_t sz = 0;
    const uint8_t k = kind[slot];
    if (k != IMP_SLOT_NONE && sample >= 0) {
      ImpSlot s; s.col = col[slot]; s.end = end[slot]; s.size = size[slot]; s.kind = k; s.err = 0;
      const uint64_t at = off[slot];
      // (always true, by the scan: nothing is stored outside the batch's cells, nor outside the block's range of them)
      if (at >= block_base && at + s.size <= block_end && at + s.size <= cells_bytes && s.size < ((uint64_t)1 << 32)) {
        int64_t row = from.row_of(S, j);
        ImpSink<true> o;
        o.out = staged ? s_stage + (at - block_base) + pad : cells + at;
        o.base = at; o.def = def; o.ndef = ndef; o.def_cap = def_cap; o.line = line;
        const uint32_t e = from.write(T, line, sample, &row, s, o);
        if (e) imp_raise(err, e, line);
        if (row < 0 || row > P.max_row) row = 0;      // (never: a kept slot's row is a row of the mapping)
        key = imp_sort_key(T, s.col, row);
        src = (uint64_t)(uintptr_t)(cells + at);
        sz = (uint32_t)s.size;
        if (k == IMP_SLOT_SPANNING_CANDIDATE) tag = ((uint64_t)s.col << P.seq_bits) | (P.line_seq_base + line + 1u);
      }
    }
    key_out[slot] = key; src_out[slot] = src; size_out[slot] = sz;
    if (tag_out) tag_out[slot] = tag;
  }
  if (!STAGE || !staged) return;      // (uniform over the block)
  __syncthreads();
  const uint64_t g0 = block_base - pad;                                   // 4-byte aligned: the cell buffer is
  const uint32_t n_words = (uint32_t)((block_end - g0 + 3u) >> 2);
  for (uint32_t w = threadIdx.x; w < n_words; w += kBlock) {
    const uint64_t g = g0 + 4ull * w;
    if (g >= block_base && g + 4u <= block_end) *reinterpret_cast<uint32_t*>(cells + g) = *reinterpret_cast<const uint32_t*>(s_stage + 4u * w);
    else for (uint32_t i = 0; i < 4u; ++i) if (g + i >= block_base && g + i < block_end) cells[g + i] = s_stage[4u * w + i];
  }
}

__global__ void k_imp_patch(uint8_t* cells, uint64_t cells_bytes, const uint64_t* at, const uint32_t* value, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || at[i] + 4u > cells_bytes) return;
  for (int b = 0; b < 4; ++b) cells[at[i] + b] = (uint8_t)(value[i] >> (8 * b));
}

// a spanning candidate stays only if it is its row's latest cell at or before the partition begin
__global__ void k_imp_resolve(uint64_t* key, const uint64_t* tag, uint64_t n, const unsigned long long* row_best, int32_t key_row_bits, int64_t max_row,
                              unsigned long long* counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !tag[i] || key[i] == kDroppedKey) return;
  const int64_t row = (int64_t)(key[i] & (((uint64_t)1 << key_row_bits) - 1u));
  if (row <= max_row && row_best[row] == tag[i]) atomicAdd(&counters[2], 1ull);
  else { key[i] = kDroppedKey; atomicAdd(&counters[3], 1ull); }
}

__global__ void k_imp_iota(uint32_t* v, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}
__global__ void k_imp_sorted_sizes(const uint32_t* idx, const uint32_t* size, uint64_t kept, uint64_t* out /* kept + 1 */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kept) out[i] = size[idx[i]];
  else if (i == kept) out[i] = 0;
}
// one wavefront per cell: consecutive lanes copy consecutive bytes
__global__ void __launch_bounds__(kBlock) k_imp_gather(const uint32_t* idx, const uint64_t* src, const uint32_t* size, const uint64_t* off, uint64_t kept,
                                                      uint8_t* out, uint64_t out_bytes) {
  const uint64_t cell = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (cell >= kept) return;
  const uint32_t lane = threadIdx.x & 63u, slot = idx[cell], n = size[slot];
  const uint8_t* from = reinterpret_cast<const uint8_t*>((uintptr_t)src[slot]);
  const uint64_t at = off[cell];
  if (!from || at + n > out_bytes) return;
  for (uint32_t i = lane; i < n; i += 64u) out[at + i] = from[i];
}

}  // namespace

namespace impdev {
void launch_iota(uint32_t* v, uint64_t n, hipStream_t s) { if (n) hipLaunchKernelGGL(k_imp_iota, dim3(grid_for(n)), dim3(kBlock), 0, s, v, n); }
void launch_sorted_sizes(const uint32_t* idx, const uint32_t* size, uint64_t kept, uint64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_imp_sorted_sizes, dim3(grid_for(kept + 1)), dim3(kBlock), 0, s, idx, size, kept, out);
}
void launch_gather(const uint32_t* idx, const uint64_t* src, const uint32_t* size, const uint64_t* off, uint64_t kept, uint8_t* out, uint64_t out_bytes, hipStream_t s) {
  if (kept) hipLaunchKernelGGL(k_imp_gather, dim3(grid_for(kept * 64)), dim3(kBlock), 0, s, idx, src, size, off, kept, out, out_bytes);
}
// the index pass of a batch, also for the translation units that index text of their own (kernels/gdb_index.hip)
void index_lines(const char* text, uint32_t n, DBuf<uint64_t>& tile, DBuf<uint64_t>& tile_scan, DBuf<char>& scan_tmp, DBuf<uint32_t>& nl, DBuf<uint32_t>& first_tab,
                 DBuf<uint32_t>& tab, hipStream_t stream, uint32_t* n_lines_out, uint32_t* n_tabs_out) {
  const uint32_t n_tiles = (n + kTile - 1u) / kTile;
  tile.ensure((size_t)n_tiles + 1);
  tile_scan.ensure((size_t)n_tiles + 1);
  IMP_HIP_CHECK(hipMemsetAsync(tile.p + n_tiles, 0, sizeof(uint64_t), stream));
  hipLaunchKernelGGL(k_imp_count, dim3(n_tiles), dim3(kBlock), 0, stream, text, n, tile.p);
  size_t bytes = 0;
  IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (const uint64_t*)tile.p, tile_scan.p, (uint64_t)0, (size_t)n_tiles + 1, rocprim::plus<uint64_t>(), stream));
  scan_tmp.ensure(std::max<size_t>(bytes, 16));
  IMP_HIP_CHECK(rocprim::exclusive_scan((void*)scan_tmp.p, bytes, (const uint64_t*)tile.p, tile_scan.p, (uint64_t)0, (size_t)n_tiles + 1, rocprim::plus<uint64_t>(), stream));
  uint64_t totals = 0;
  IMP_HIP_CHECK(hipMemcpyAsync(&totals, tile_scan.p + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  const uint32_t n_lines = (uint32_t)(totals >> 32), n_tabs = (uint32_t)totals;
  *n_lines_out = n_lines; *n_tabs_out = n_tabs;
  if (n_lines == 0) return;
  nl.ensure(n_lines);
  first_tab.ensure((size_t)n_lines + 1);
  tab.ensure(std::max<uint32_t>(n_tabs, 1));
  IMP_HIP_CHECK(hipMemsetAsync(first_tab.p, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_imp_scatter, dim3(n_tiles), dim3(kBlock), 0, stream, text, n, (const uint64_t*)tile_scan.p, nl.p, first_tab.p, tab.p, n_lines, n_tabs);
}
}  // namespace impdev

DeviceImporter::DeviceImporter(int device, const VidMapper& vid, const ImportOptions& opt, uint64_t text_budget_bytes, int inflate_mode, const ImportTextTap* tap)
    : m_(new Impl) {
  try {
    if (tap) m_->tap = *tap;
    m_->tapped = tap != nullptr;
    if (inflate_mode < kInflateAuto || inflate_mode > kInflateDevice) throw VCF2BinaryException("inflate mode " + std::to_string(inflate_mode) + ": 0 (auto), 1 (host) or 2 (device)");
    m_->inflate_mode = inflate_mode;
    m_->device = device;
    m_->opt = with_clamped_row_bounds(opt, vid);
    m_->budget = text_budget_bytes ? text_budget_bytes : kDefaultTextBudget;
    m_->budget = std::min<uint64_t>(m_->budget, (uint64_t)1 << 30);
    if (const char* e = getenv("GDBAMD_IMPORT_STAGE_LDS")) m_->stage_in_lds = atoi(e) != 0;
    // the A/B of profiles/device_inflate.md: one thread per BGZF member instead of one wavefront (9.6 x slower; kept for that comparison)
    if (const char* e = getenv("GDBAMD_INFLATE_KERNEL")) m_->inflater.set_kernel(std::string(e) == "thread" ? BgzfDeviceInflater::kThreadPerMember : BgzfDeviceInflater::kWavePerMember);
    m_->H = build_import_tables(vid, m_->tapped);     // the refusals: before the device is touched (a tap copies lines: contigs only)
    m_->files = import_files(vid, m_->opt);
    for (const CallSetInfo& cs : vid.get_callsets()) {
      bool used = false;
      for (const ImportFile& f : m_->files) used = used || f.name == cs.m_filename;
      if (!used) m_->skipped_files.push_back(cs.m_filename);
    }
    if (!m_->tapped) refuse_for_csv(vid, m_->H, m_->files);
    Impl& M = *m_;
    if (opt.column_begin > 0) {
      int col_bits = 0;
      while (col_bits < 63 && (opt.column_begin >> col_bits) != 0) ++col_bits;
      M.spanning = true;
      M.seq_bits = 64 - col_bits;
    }
    if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the device importer has no CPU fallback (import_callsets_to_cells is the host importer)");
    IMP_HIP_CHECK(hipSetDevice(device));
    IMP_HIP_CHECK(hipStreamCreate(&M.stream));
    for (auto& e : M.ev) IMP_HIP_CHECK(hipEventCreate(&e));
    auto up = [&](auto& buf, const auto* src, size_t n) {
      buf.ensure(std::max<size_t>(n, 1));
      if (n) IMP_HIP_CHECK(hipMemcpy(buf.p, src, n * sizeof(*src), hipMemcpyHostToDevice));
    };
    up(M.d_names, M.H.names.data(), M.H.names.size());
    up(M.d_contigs, M.H.contigs.data(), M.H.contigs.size());
    up(M.d_fields, M.H.fields.data(), M.H.fields.size());
    up(M.d_info, M.H.info.data(), M.H.info.size());
    up(M.d_fmt, M.H.fmt.data(), M.H.fmt.size());
    M.d_row_best.ensure((size_t)M.H.max_row + 1);
    IMP_HIP_CHECK(hipMemset(M.d_row_best.p, 0, ((size_t)M.H.max_row + 1) * sizeof(unsigned long long)));
    M.d_counters.ensure(4);
    IMP_HIP_CHECK(hipMemset(M.d_counters.p, 0, 4 * sizeof(unsigned long long)));
    M.d_err.ensure(kErrWords);
    M.d_ndef.ensure(1);
    M.d_find.ensure(2);
  } catch (...) { this->~DeviceImporter(); throw; }
}

DeviceImporter::~DeviceImporter() {
  if (!m_) return;
  if (m_->stream) { (void)hipSetDevice(m_->device); (void)hipStreamSynchronize(m_->stream); }
  m_->free_batches();
  for (auto& e : m_->ev) if (e) (void)hipEventDestroy(e);
  if (m_->stream) (void)hipStreamDestroy(m_->stream);
  delete m_;
  m_ = nullptr;
}

const ImportStats& DeviceImporter::stats() const { return m_->st; }

void DeviceImporter::import_all(const std::vector<ImportStream>& streams) {
  for (const ImportStream& s : streams) {
    bool used = false;
    for (const ImportFile& f : m_->files) used = used || f.name == s.name;
    for (const std::string& name : m_->skipped_files) used = used || name == s.name;      // (of another batch: left alone)
    if (!used) throw VCF2BinaryException("stream " + s.name + " is not a \"filename\" of the callset mapping");
  }
  for (const ImportFile& f : m_->files) {
    const ImportStream* from = nullptr;
    for (const ImportStream& s : streams) if (s.name == f.name) from = &s;
    if (from) append_buffer(f.name, from->data, from->nbytes);
    else append_file(f.name);
  }
}

namespace {
uint64_t file_bytes(const std::string& path) { struct stat sb; return stat(path.c_str(), &sb) == 0 ? (uint64_t)sb.st_size : 0u; }
std::string bad_member(const std::string& path, uint64_t offset, const std::string& why) {
  return "corrupt BGZF member at byte offset " + std::to_string(offset) + " of " + path + ": " + why;
}
// one member by zlib, appended to `out`; the same three checks as on the device
void inflate_member_host(const std::string& raw, const BgzfMember& m, std::string& out, const std::string& path) {
  const size_t old = out.size();
  out.resize(old + (size_t)m.isize + 1u);
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, -15) != Z_OK) throw VCF2BinaryException("zlib inflateInit2 failed");
  zs.next_in = (Bytef*)(raw.data() + m.offset + m.data_off); zs.avail_in = m.data_len;
  zs.next_out = (Bytef*)(&out[old]); zs.avail_out = m.isize + 1u;
  const int rc = inflate(&zs, Z_FINISH);
  const uint64_t got = zs.total_out;
  inflateEnd(&zs);
  out.resize(old + (size_t)std::min<uint64_t>(got, m.isize));
  if (rc != Z_STREAM_END) throw VCF2BinaryException(bad_member(path, m.offset, "invalid DEFLATE stream"));
  if (got != m.isize) throw VCF2BinaryException(bad_member(path, m.offset, "the data is not ISIZE bytes long"));
  if ((uint32_t)crc32(0L, (const Bytef*)(out.data() + old), m.isize) != m.crc) throw VCF2BinaryException(bad_member(path, m.offset, "CRC32 mismatch"));
}
}  // namespace

void DeviceImporter::append_file(const std::string& filename) {
  Impl& M = *m_;
  IMP_HIP_CHECK(hipSetDevice(M.device));
  const ImportFile* file = &M.file_named(filename);
  const double t0 = now_s();
  if (file->type != GDB_FILE_VCF) {       // the callset mapping decides; read as it is
    std::ifstream in(file->path, std::ios::binary);
    if (!in) throw VCF2BinaryException("cannot open " + file->path);
    in.seekg(0, std::ios::end);
    const std::streamoff size = in.tellg();
    in.seekg(0, std::ios::beg);
    std::string data(size > 0 ? (size_t)size : 0, '\0');
    if (!data.empty() && !in.read(&data[0], (std::streamsize)data.size())) throw VCF2BinaryException("cannot read " + file->path);
    M.st.s_read += now_s() - t0;
    M.st.compressed_bytes += data.size();
    ++M.st.num_files;
    M.append_csv(*file, data.data(), data.size());
    return;
  }
  if (file_is_bcf2(file->path)) {       // the content decides, plain or compressed; BCF2 records cross BGZF members, so the host inflates
    if (M.inflate_mode == kInflateDevice)
      throw VCF2BinaryException(file->path + " is BCF2: BCF2 input is inflated on the host in this build, and inflating on the device was required");
    std::string data;
    try { data = gz_text::read_all(file->path); }
    catch (const std::exception&) { throw VCF2BinaryException("cannot read " + file->path); }
    M.st.s_read += now_s() - t0;
    M.st.compressed_bytes += file_bytes(file->path);
    ++M.st.num_files;
    ++M.st.num_host_inflated_files;
    M.append_bcf(*file, data.data(), data.size());
    return;
  }
  M.append_vcf_path(*file, t0);
}

void DeviceImporter::append_text_path(const std::string& path) {
  Impl& M = *m_;
  if (!M.tapped) throw VCF2BinaryException("append_text_path needs a text tap: " + path + " has no callset to make cells for");
  IMP_HIP_CHECK(hipSetDevice(M.device));
  ImportFile file;
  file.name = path; file.path = path;
  for (const ImportFile& f : M.files) if (f.path == path) file = f;
  M.append_vcf_path(file, now_s());
}

void DeviceImporter::Impl::append_vcf_path(const ImportFile& file_, double t0) {
  Impl& M = *this;
  const ImportFile* file = &file_;
  std::string raw;
  std::vector<BgzfMember> mem;
  bool is_bgzf = false;
  if (M.inflate_mode != kInflateHost) {
    std::ifstream in(file->path, std::ios::binary);
    if (!in) throw VCF2BinaryException("cannot open " + file->path);
    // the first member's header decides: a file that does not begin like BGZF is not read here at all
    char first[18];
    in.read(first, sizeof(first));
    if (in.gcount() == (std::streamsize)sizeof(first) && bgzf_begins((const uint8_t*)first)) {
      in.clear();
      in.seekg(0, std::ios::end);
      const std::streamoff size = in.tellg();
      in.seekg(0, std::ios::beg);
      raw.resize(size > 0 ? (size_t)size : 0);
      if (!raw.empty() && !in.read(&raw[0], (std::streamsize)raw.size())) throw VCF2BinaryException("cannot read " + file->path);
      is_bgzf = bgzf_walk((const uint8_t*)raw.data(), raw.size(), mem, nullptr);
    }
  }
  if (is_bgzf) {
    M.st.s_read += now_s() - t0;
    M.st.compressed_bytes += raw.size();
    ++M.st.num_files;
    M.append_bgzf(*file, raw, mem);
    return;
  }
  if (M.inflate_mode == kInflateDevice)
    throw VCF2BinaryException(file->path + " is not a BGZF file from its first byte to its last, and inflating on the device was required");
  raw = std::string();
  std::string text;
  try { text = gz_text::read_all(file->path); }
  catch (const std::exception&) { throw VCF2BinaryException("cannot open " + file->path); }
  M.st.s_read += now_s() - t0;
  M.st.compressed_bytes += file_bytes(file->path);
  ++M.st.num_files;
  ++M.st.num_host_inflated_files;
  M.append_text(*file, text);
}

int DeviceImporter::Impl::upload_samples(const ImportHeader& hdr) {
  std::vector<int32_t> samp_idx;
  std::vector<int64_t> samp_row;
  for (int s = 0; s < hdr.n_samples; ++s) if (hdr.sample_row[(size_t)s] >= 0) { samp_idx.push_back(s); samp_row.push_back(hdr.sample_row[(size_t)s]); }
  const int n_imp = (int)samp_idx.size();
  d_samp_idx.ensure(std::max(n_imp, 1));
  d_samp_row.ensure(std::max(n_imp, 1));
  if (n_imp) {
    IMP_HIP_CHECK(hipMemcpyAsync(d_samp_idx.p, samp_idx.data(), (size_t)n_imp * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipMemcpyAsync(d_samp_row.p, samp_row.data(), (size_t)n_imp * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
  }
  return n_imp;
}

void DeviceImporter::Impl::append_text(const ImportFile& file_, const std::string& text) {
  const ImportFile* file = &file_;
  Impl& M = *this;
  const ImportHeader hdr = parse_import_header(text, *file);
  const int n_imp = upload_samples(hdr);
  if (tapped && tap.on_header) tap.on_header(file->path, text.substr(0, hdr.record_begin));
  // batches of at most the budget, cut behind a newline; a line longer than the budget grows its batch
  size_t pos = hdr.record_begin;
  int64_t lines_before = hdr.lines_before;
  while (pos < text.size()) {
    const size_t stop = import_text_cut(text.data(), text.size(), pos, M.budget);
    const size_t n = stop - pos;
    if (n >= ((size_t)1 << 31)) throw VCF2BinaryException("a record line of 2 GiB or more in " + file->path);
    const bool add_newline = text[stop - 1] != '\n';
    lines_before += M.batch(*file, hdr, text.data() + pos, n, add_newline, lines_before, n_imp);
    pos = stop;
  }
}

void DeviceImporter::Impl::append_csv(const ImportFile& file, const char* data, size_t size) {
  refuse_compressed_csv(data, size, file.path);
  const std::vector<int64_t> rows = csv_rows_of(file);
  d_samp_row.ensure(std::max<size_t>(rows.size(), 1));
  IMP_HIP_CHECK(hipMemcpyAsync(d_samp_row.p, rows.data(), rows.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  const ImportHeader none;
  size_t pos = 0;
  int64_t lines_before = 0;
  while (pos < size) {
    const size_t stop = import_text_cut(data, size, pos, budget);
    const size_t n = stop - pos;
    if (n >= ((size_t)1 << 31)) throw VCF2BinaryException("a line of 2 GiB or more in " + file.path);
    lines_before += batch(file, none, data + pos, n, data[stop - 1] != '\n', lines_before, 1, (int)rows.size());
    pos = stop;
  }
}

void DeviceImporter::Impl::find_newlines(const char* text, uint64_t lo, uint64_t mid, uint64_t hi, uint64_t* last_below, uint64_t* first_above) {
  unsigned long long r[2] = {0ull, ~0ull};
  if (hi > lo) {
    IMP_HIP_CHECK(hipMemcpyAsync(d_find.p, r, sizeof(r), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_imp_find_newlines, dim3(grid_for(hi - lo)), dim3(kBlock), 0, stream, text, lo, mid, hi, d_find.p);
    IMP_HIP_CHECK(hipMemcpyAsync(r, d_find.p, sizeof(r), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
  }
  *last_below = r[0];
  *first_above = r[1];
}

void DeviceImporter::Impl::append_bgzf(const ImportFile& file, const std::string& raw, const std::vector<BgzfMember>& mem) {
  // ---- the '#' lines: leading members on the host, until a record line has begun
  double t0 = now_s();
  std::string head;
  size_t k = 0, line_start = 0;
  bool complete = false;
  while (!complete && k < mem.size()) {
    inflate_member_host(raw, mem[k], head, file.path);
    ++k;
    for (;;) {
      const size_t nl = head.find('\n', line_start);
      const size_t e = nl == std::string::npos ? head.size() : nl;
      size_t ln = e - line_start;
      if (ln && head[e - 1] == '\r') --ln;
      if (ln && head[line_start] != '#') { complete = true; break; }
      if (nl == std::string::npos) break;      // a '#' line (or nothing yet) that the next member continues
      line_start = nl + 1;
    }
  }
  st.s_read += now_s() - t0;
  const ImportHeader hdr = parse_import_header(head, file);
  const int n_imp = upload_samples(hdr);
  if (tapped && tap.on_header) tap.on_header(file.path, head.substr(0, hdr.record_begin));
  const std::string chrom_error = "a #CHROM line after the first record in " + file.path + " is not imported by the device importer of this build";

  // ---- windows: [carried partial line | members k .. k2)
  int cur = 0;
  uint64_t carry = head.size() - hdr.record_begin;
  if (carry >= ((uint64_t)1 << 31)) throw VCF2BinaryException("a record line of 2 GiB or more in " + file.path);
  d_win[cur].ensure((size_t)carry + 16);
  if (carry) {
    t0 = now_s();
    IMP_HIP_CHECK(hipMemcpyAsync(d_win[cur].p, head.data() + hdr.record_begin, (size_t)carry, hipMemcpyHostToDevice, stream));
    st.bytes_h2d += carry;
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    st.s_h2d += now_s() - t0;
  }
  int64_t lines_before = hdr.lines_before;
  for (;;) {
    size_t k2 = k;
    uint64_t w_bytes = 0;
    const uint64_t room = budget > carry ? budget - carry : 0;
    while (k2 < mem.size() && (k2 == k || w_bytes + mem[k2].isize <= room)) w_bytes += mem[k2++].isize;
    const bool last = k2 == mem.size();
    const uint64_t wend = carry + w_bytes;
    if (d_win[cur].cap < wend + 16) {          // grows, and keeps the carried bytes
      d_win[1 - cur].ensure((size_t)wend + 16);
      if (carry) IMP_HIP_CHECK(hipMemcpyAsync(d_win[1 - cur].p, d_win[cur].p, (size_t)carry, hipMemcpyDeviceToDevice, stream));
      cur = 1 - cur;
    }
    char* win = d_win[cur].p;
    if (k2 > k) {
      const float ms_before = inflater.ms_kernel, up_before = inflater.ms_upload;
      const uint64_t h2d_before = inflater.bytes_h2d;
      uint32_t err = 0;
      const int64_t bad = inflater.inflate((const uint8_t*)raw.data(), mem.data(), k, k2, (uint8_t*)win + carry, (void*)stream, &err);
      st.ms_inflate += inflater.ms_kernel - ms_before;
      st.bytes_h2d += inflater.bytes_h2d - h2d_before;
      st.s_h2d += (double)(inflater.ms_upload - up_before) * 1e-3;
      if (bad >= 0) throw VCF2BinaryException(bad_member(file.path, mem[(size_t)bad].offset, bgzf_inflate_error_text(err)));
      st.num_device_members += (int64_t)(k2 - k);
    }
    char last_byte = '\n';
    if (wend) {
      uint32_t found = 0;
      IMP_HIP_CHECK(hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), stream));
      hipLaunchKernelGGL(k_imp_find_chrom, dim3(grid_for(wend)), dim3(kBlock), 0, stream, (const char*)win, wend, d_err.p);
      IMP_HIP_CHECK(hipMemcpyAsync(&found, d_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      if (last) IMP_HIP_CHECK(hipMemcpyAsync(&last_byte, win + wend - 1, 1, hipMemcpyDeviceToHost, stream));
      IMP_HIP_CHECK(hipStreamSynchronize(stream));
      if (found) throw VCF2BinaryException(chrom_error);
    }
    // batches of at most the budget, cut behind a newline; a line longer than the budget grows its batch
    uint64_t pos = 0;
    while (pos < wend) {
      uint64_t stop = wend, below = 0, above = 0;
      if (wend - pos > budget) {
        find_newlines(win, pos, pos + budget, wend, &below, &above);
        if (below) stop = below;
        else if (above != ~(uint64_t)0) stop = above + 1;
        else if (!last) break;                 // the line goes on in the next window
      } else if (!last) {
        find_newlines(win, pos, wend, wend, &below, &above);
        if (!below) break;
        stop = below;
      }
      const uint64_t n = stop - pos;
      if (n >= ((uint64_t)1 << 31)) throw VCF2BinaryException("a record line of 2 GiB or more in " + file.path);
      const bool add_newline = stop == wend && last && last_byte != '\n';
      d_text.ensure((size_t)n + 1 + kTextPad);
      IMP_HIP_CHECK(hipMemcpyAsync(d_text.p, win + pos, (size_t)n, hipMemcpyDeviceToDevice, stream));
      lines_before += batch(file, hdr, nullptr, (size_t)n, add_newline, lines_before, n_imp);
      pos = stop;
    }
    carry = wend - pos;
    if (last) break;
    if (carry >= ((uint64_t)1 << 31)) throw VCF2BinaryException("a record line of 2 GiB or more in " + file.path);
    if (pos) {                                 // the partial line moves to the front of the next window
      d_win[1 - cur].ensure(std::max((size_t)carry + 16, d_win[cur].cap));      // (as large as this one: the next window fits without a second move)
      if (carry) IMP_HIP_CHECK(hipMemcpyAsync(d_win[1 - cur].p, win + pos, (size_t)carry, hipMemcpyDeviceToDevice, stream));
      cur = 1 - cur;
    }
    k = k2;
  }
}

uint32_t DeviceImporter::Impl::batch(const ImportFile& file, const ImportHeader& hdr, const char* text, size_t n_text, bool add_newline, int64_t lines_before, int n_imp,
                                     int n_csv_rows) {
  const uint32_t n = (uint32_t)(n_text + (add_newline ? 1 : 0));
  ++st.num_batches;
  st.text_bytes += n_text;
  double t0 = now_s();
  if (text) {
    d_text.ensure((size_t)n + kTextPad);
    IMP_HIP_CHECK(hipMemcpyAsync(d_text.p, text, n_text, hipMemcpyHostToDevice, stream));
    st.bytes_h2d += n_text;
  } else if (d_text.cap < (size_t)n + kTextPad) throw GenomicsDBDeviceException("batch text is not in d_text");
  if (add_newline) IMP_HIP_CHECK(hipMemsetAsync(d_text.p + n_text, '\n', 1, stream));
  IMP_HIP_CHECK(hipMemsetAsync(d_text.p + n, 0, kTextPad, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  if (text) st.s_h2d += now_s() - t0;
  // text that was inflated on the device comes to the host only when a deferred token or an error message needs it
  std::string text_copy;
  auto host_text = [&]() -> const char* {
    if (text) return text;
    if (text_copy.empty() && n_text) {
      text_copy.resize(n_text);
      IMP_HIP_CHECK(hipMemcpy(&text_copy[0], d_text.p, n_text, hipMemcpyDeviceToHost));
    }
    return text_copy.data();
  };

  // ---- index
  IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
  uint32_t n_lines = 0, n_tabs = 0;
  index_lines(d_text.p, n, d_tile, d_tile_scan, d_tmp, d_nl, d_first_tab, d_tab, stream, &n_lines, &n_tabs);     // (the text ends with a newline)
  if (n_lines == 0) return 0;
  IMP_HIP_CHECK(hipEventRecord(ev[1], stream));

  const ImpTables T = tables(hdr.n_samples);
  BatchWords words;
  words.host_text = host_text; words.n_text = n_text;
  words.where = [&](uint32_t line) { return file.path + " line " + std::to_string(lines_before + (int64_t)line + 1); };
  if (n_csv_rows >= 0) {
    words.describe = [&](uint32_t bit, uint32_t line) { return describe_csv_error(bit, words.where(line)); };
    cells_of_batch(ImpCsvSrc{ImpBatch{d_text.p, d_nl.p, d_first_tab.p, d_tab.p, n_lines}, ImpCsvRows{d_samp_row.p, n_csv_rows}}, T, n_lines, n_imp, words, true);
    return n_lines;
  }
  words.describe = [&](uint32_t bit, uint32_t line) {
    uint32_t lb = 0, le = 0;
    if (line) { IMP_HIP_CHECK(hipMemcpy(&lb, d_nl.p + (line - 1), sizeof(uint32_t), hipMemcpyDeviceToHost)); ++lb; }
    IMP_HIP_CHECK(hipMemcpy(&le, d_nl.p + line, sizeof(uint32_t), hipMemcpyDeviceToHost));
    le = std::min<uint32_t>(le, (uint32_t)n_text);
    return describe_line_error(bit, H, opt, hdr, host_text(), lb, le, words.where(line));
  };
  if (tapped) {       // the indexed batch is the product
    ImportTextBatch b;
    b.path = &file.path; b.d_text = d_text.p; b.d_nl = d_nl.p; b.d_first_tab = d_first_tab.p; b.d_tab = d_tab.p;
    b.n_bytes = n; b.n_lines = n_lines; b.lines_before = lines_before; b.tables = &T; b.stream = (void*)stream; b.describe = words.describe;
    if (tap.on_batch) tap.on_batch(b);
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0;
    IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_index += ms;
    return n_lines;
  }
  cells_of_batch(ImpTextSrc{{}, ImpBatch{d_text.p, d_nl.p, d_first_tab.p, d_tab.p, n_lines}}, T, n_lines, n_imp, words, true);
  return n_lines;
}

template <class Src> void DeviceImporter::Impl::cells_of_batch(const Src& src, const ImpTables& T, uint32_t n_lines, int n_imp, const BatchWords& words, bool text) {
  // ---- measure
  if (spanning && seq_bits < 64 && ((line_seq + n_lines + 1) >> seq_bits) != 0)
    throw VCF2BinaryException("too many record lines for the partition-begin rule of the device importer at column_begin " + std::to_string(opt.column_begin));
  const uint64_t n_slots = (uint64_t)n_lines * (uint64_t)std::max(n_imp, 1);
  if (total_slots + n_slots >= ((uint64_t)1 << 32)) throw VCF2BinaryException("more than 2^32 (record line, sample) pairs in one device import: split the callset mapping");
  d_col.ensure(n_slots); d_end.ensure(n_slots); d_size.ensure(n_slots + 1); d_off.ensure(n_slots + 1); d_kind.ensure(n_slots);
  const ImpSamples S{d_samp_idx.p, d_samp_row.p, n_imp};
  const bool by_sample = !std::is_same<Src, ImpCsvSrc>::value;     // a CSV line is never replayed at the partition begin: no row_best, no tags
  const ImpSpan P{spanning && by_sample ? d_row_best.p : nullptr, seq_bits, line_seq, H.max_row};
  spanning_slots = spanning_slots || (spanning && by_sample);
  IMP_HIP_CHECK(hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), stream));
  IMP_HIP_CHECK(hipMemsetAsync(d_err.p + 1, 0xFF, (kErrWords - 1) * sizeof(uint32_t), stream));
  IMP_HIP_CHECK(hipMemsetAsync(d_counters.p, 0, 2 * sizeof(unsigned long long), stream));
  IMP_HIP_CHECK(hipMemsetAsync(d_size.p + n_slots, 0, sizeof(uint64_t), stream));
  hipLaunchKernelGGL(k_imp_measure<Src>, dim3(grid_for(n_slots)), dim3(kBlock), 0, stream, T, src, S, P, n_slots, d_col.p, d_end.p, d_size.p, d_kind.p, d_err.p, d_counters.p);
  IMP_HIP_CHECK(hipEventRecord(ev[2], stream));
  scan<uint64_t>(d_size.p, d_off.p, (size_t)n_slots + 1);
  uint64_t cells_bytes = 0;
  unsigned long long counters[2] = {0, 0};
  IMP_HIP_CHECK(hipMemcpyAsync(&cells_bytes, d_off.p + n_slots, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));

  // ---- write
  batches.emplace_back();
  Batch& b = batches.back();
  b.n_slots = n_slots; b.cells_bytes = cells_bytes;
  b.key = dalloc<uint64_t>(n_slots); b.src = dalloc<uint64_t>(n_slots); b.size = dalloc<uint32_t>(n_slots);
  if (spanning) b.tag = dalloc<uint64_t>(n_slots);
  b.cells = dalloc<uint8_t>(cells_bytes + 16);
  d_def.ensure(std::max<size_t>(d_def.cap, 1 << 16));
  uint32_t ndef = 0;
  uint32_t err[kErrWords];
  for (int attempt = 0;; ++attempt) {
    IMP_HIP_CHECK(hipMemsetAsync(d_ndef.p, 0, sizeof(uint32_t), stream));
    IMP_HIP_CHECK(hipEventRecord(ev[3], stream));
    if (stage_in_lds)
      hipLaunchKernelGGL((k_imp_write<true, Src>), dim3(grid_for(n_slots)), dim3(kBlock), 0, stream, T, src, S, P, n_slots, (const int64_t*)d_col.p, (const int64_t*)d_end.p,
                         (const uint64_t*)d_size.p, (const uint8_t*)d_kind.p, (const uint64_t*)d_off.p, b.cells, cells_bytes, d_def.p, d_ndef.p, (uint32_t)d_def.cap,
                         b.key, b.src, b.size, b.tag, d_err.p);
    else
      hipLaunchKernelGGL((k_imp_write<false, Src>), dim3(grid_for(n_slots)), dim3(kBlock), 0, stream, T, src, S, P, n_slots, (const int64_t*)d_col.p, (const int64_t*)d_end.p,
                         (const uint64_t*)d_size.p, (const uint8_t*)d_kind.p, (const uint64_t*)d_off.p, b.cells, cells_bytes, d_def.p, d_ndef.p, (uint32_t)d_def.cap,
                         b.key, b.src, b.size, b.tag, d_err.p);
    IMP_HIP_CHECK(hipEventRecord(ev[4], stream));
    IMP_HIP_CHECK(hipMemcpyAsync(&ndef, d_ndef.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    if (ndef <= d_def.cap || attempt > 0) break;
    d_def.ensure(ndef);            // the list was too short: the write pass is repeated into the same places
  }
  if (ndef > d_def.cap) throw GenomicsDBDeviceException("deferred-token list overflow");
  float ms = 0;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_index += ms;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[1], ev[2])); st.ms_measure += ms;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[3], ev[4])); st.ms_write += ms;

  // ---- deferred tokens: the host importer's parsers, on exactly those tokens
  const double t0 = now_s();
  std::vector<ImpDeferred> def(ndef);
  if (ndef) IMP_HIP_CHECK(hipMemcpy(def.data(), d_def.p, (size_t)ndef * sizeof(ImpDeferred), hipMemcpyDeviceToHost));
  std::vector<uint64_t> patch_at(ndef);
  std::vector<uint32_t> patch_val(ndef);
  uint32_t bad_line = UINT32_MAX;
  std::string bad_text;
  for (uint32_t i = 0; i < ndef; ++i) {
    const ImpDeferred& d = def[i];
    if ((uint64_t)d.tok_off + d.tok_len > words.n_text) throw GenomicsDBDeviceException("deferred token outside the batch");
    patch_at[i] = d.out_off;
    try { patch_val[i] = resolve_deferred(d, words.host_text(), H); }
    catch (const VCF2BinaryException& e) {
      if (d.line < bad_line) { bad_line = d.line; bad_text = e.what(); bad_text = bad_text.substr(strlen("VCF2BinaryException : ")); }
    }
  }
  // ---- errors: the smallest offending line speaks
  uint32_t err_line = UINT32_MAX, err_bit = 0;
  for (int k = 0; k < kErrWords - 1; ++k) if ((err[0] & (1u << k)) && err[1 + k] < err_line) { err_line = err[1 + k]; err_bit = 1u << k; }
  if (err_bit || bad_line != UINT32_MAX) {
    if (err_line <= bad_line) throw VCF2BinaryException(words.describe(err_bit, err_line));
    throw VCF2BinaryException(bad_text + " (" + words.where(bad_line) + ")");
  }
  if (ndef) {
    d_patch_at.ensure(ndef); d_patch_val.ensure(ndef);
    IMP_HIP_CHECK(hipMemcpyAsync(d_patch_at.p, patch_at.data(), (size_t)ndef * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipMemcpyAsync(d_patch_val.p, patch_val.data(), (size_t)ndef * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_imp_patch, dim3(grid_for(ndef)), dim3(kBlock), 0, stream, b.cells, cells_bytes, (const uint64_t*)d_patch_at.p, (const uint32_t*)d_patch_val.p, ndef);
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
  }
  st.s_deferred += now_s() - t0;
  st.num_deferred_values += ndef;
  st.num_records += (int64_t)counters[0];
  total_cells += counters[1];
  total_slots += n_slots;
  line_seq += n_lines;
  if (after_batch) after_batch(n_lines, (uint32_t)std::max(n_imp, 1), text);
}

ImpBcfTables DeviceImporter::Impl::upload_bcf_tables(const BcfHeaderHost& hdr) {
  auto up = [&](auto& buf, const auto& v) {
    buf.ensure(std::max<size_t>(v.size(), 1));
    if (!v.empty()) IMP_HIP_CHECK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, stream));
  };
  up(d_dict_info, hdr.dict_info); up(d_dict_fmt, hdr.dict_fmt); up(d_dict_filter, hdr.dict_filter); up(d_contig_off, hdr.contig_off);
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  ImpBcfTables BT = hdr.view();
  BT.dict_info = d_dict_info.p; BT.dict_fmt = d_dict_fmt.p; BT.dict_filter = d_dict_filter.p; BT.contig_off = d_contig_off.p;
  return BT;
}

void DeviceImporter::Impl::append_bcf(const ImportFile& file, const char* data, size_t n) {
  const BcfHeaderHost hdr = parse_bcf_header(data, n, file, H);
  const int n_imp = upload_samples(hdr.samples);
  const ImpBcfTables BT = upload_bcf_tables(hdr);
  // the host walks the chain (8 bytes per record) and cuts batches at record boundaries
  std::vector<uint64_t> offs;
  bcf_walk_records(data, n, hdr.records_begin, file.path, offs);
  bcf_batches(file, hdr, BT, n_imp, data, offs, 0);
}

void DeviceImporter::Impl::bcf_batches(const ImportFile& file, const BcfHeaderHost& hdr, const ImpBcfTables& BT, int n_imp, const char* data,
                                       const std::vector<uint64_t>& offs, uint64_t records_before) {
  const ImpTables T = tables(hdr.samples.n_samples);
  const uint32_t n_attr = (uint32_t)(H.info.size() + H.fmt.size());
  std::vector<uint32_t> rel;
  for (size_t first = 0; first + 1 < offs.size();) {
    const size_t last = bcf_next_batch(offs, first, budget);
    const uint64_t base = offs[first], n_bytes = offs[last] - base;
    if (n_bytes >= ((uint64_t)1 << 31)) throw VCF2BinaryException("a BCF2 record of 2 GiB or more in " + file.path);
    const uint32_t n_rec = (uint32_t)(last - first);
    rel.resize((size_t)n_rec + 1);
    for (size_t k = 0; k <= n_rec; ++k) rel[k] = (uint32_t)(offs[first + k] - base);
    ++st.num_batches;
    st.text_bytes += n_bytes;
    const double t0 = now_s();
    d_text.ensure((size_t)n_bytes + kTextPad);
    d_rec_off.ensure((size_t)n_rec + 1);
    d_rec.ensure(n_rec);
    d_fld.ensure(std::max<size_t>((size_t)n_rec * n_attr, 1));
    IMP_HIP_CHECK(hipMemcpyAsync(d_text.p, data + base, (size_t)n_bytes, hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipMemcpyAsync(d_rec_off.p, rel.data(), rel.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    st.bytes_h2d += n_bytes + rel.size() * sizeof(uint32_t);
    st.s_h2d += now_s() - t0;
    if (tapped) {       // the uploaded batch is the product
      if (!tap.on_records) throw VCF2BinaryException(file.path + " is BCF2: this tap takes (g)VCF text only");
      ImportRecordBatch b;
      b.path = &file.path; b.d_bytes = (const uint8_t*)d_text.p; b.d_rec_off = d_rec_off.p; b.n_bytes = (uint32_t)n_bytes; b.n_rec = n_rec;
      b.records_before = (int64_t)(records_before + first); b.bcf_tables = &BT; b.stream = (void*)stream;
      b.describe = [&](uint32_t bit, uint32_t r) {
        return describe_bcf_error(bit, H, opt, hdr, (const uint8_t*)data + base, rel[r], rel[r + 1u],
                                  file.path + " record " + std::to_string(records_before + first + r + 1));
      };
      tap.on_records(b);
      IMP_HIP_CHECK(hipStreamSynchronize(stream));
      first = last;
      continue;
    }
    // ---- index: one thread per record
    IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(k_imp_bcf_index, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, T, BT, (const uint8_t*)d_text.p, (uint32_t)n_bytes, (const uint32_t*)d_rec_off.p, n_rec,
                       d_rec.p, d_fld.p, n_attr);
    IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
    BatchWords words;
    words.host_text = []() -> const char* { return nullptr; };      // (nothing is deferred)
    words.where = [&](uint32_t r) { return file.path + " record " + std::to_string(records_before + first + r + 1); };
    words.describe = [&](uint32_t bit, uint32_t r) {
      return describe_bcf_error(bit, H, opt, hdr, (const uint8_t*)data + base, rel[r], rel[r + 1u], words.where(r));
    };
    cells_of_batch(ImpBcfSrc{{}, BT, (const uint8_t*)d_text.p, d_rec.p, d_fld.p, n_attr}, T, n_rec, n_imp, words, false);
    first = last;
  }
}

const ImportFile& DeviceImporter::Impl::file_named(const std::string& filename) const {
  for (const ImportFile& f : files) if (f.name == filename) return f;
  throw VCF2BinaryException("file " + filename + " is not in the callset mapping");
}

void DeviceImporter::append_buffer(const std::string& name, const void* ptr, uint64_t nbytes) {
  Impl& M = *m_;
  IMP_HIP_CHECK(hipSetDevice(M.device));
  ImportFile file = M.file_named(name);
  file.path = name;       // messages name the stream
  if (!ptr && nbytes) throw VCF2BinaryException("stream " + name + ": null data");
  const char* data = (const char*)ptr;
  const double t0 = now_s();
  if (file.type != GDB_FILE_VCF) {
    M.st.s_read += now_s() - t0;
    M.st.compressed_bytes += nbytes;
    ++M.st.num_files;
    M.append_csv(file, data, (size_t)nbytes);
    return;
  }
  std::string inflated;
  const bool gz = is_gzip(data, (size_t)nbytes);
  if (gz) {
    // a BGZF stream of VCF text may still be inflated on the device; BCF2 records cross members, so BCF2 is inflated here
    std::vector<BgzfMember> mem;
    if (M.inflate_mode != kInflateHost && nbytes >= 18 && bgzf_begins((const uint8_t*)data) && bgzf_walk((const uint8_t*)data, (size_t)nbytes, mem, nullptr)) {
      const std::string first = inflate_gzip_buffer(data, mem.size() > 1 ? (size_t)mem[1].offset : (size_t)nbytes, name);
      if (!is_bcf2(first.data(), first.size())) {
        M.st.s_read += now_s() - t0;
        M.st.compressed_bytes += nbytes;
        ++M.st.num_files;
        M.append_bgzf(file, std::string(data, (size_t)nbytes), mem);
        return;
      }
    }
    inflated = inflate_gzip_buffer(data, (size_t)nbytes, name);
    data = inflated.data();
  }
  const size_t n = gz ? inflated.size() : (size_t)nbytes;
  const bool bcf = is_bcf2(data, n);
  if (M.inflate_mode == kInflateDevice)
    throw VCF2BinaryException(bcf ? name + " is BCF2: BCF2 input is inflated on the host in this build, and inflating on the device was required"
                                  : name + " is not a BGZF file from its first byte to its last, and inflating on the device was required");
  M.st.s_read += now_s() - t0;
  M.st.compressed_bytes += nbytes;
  ++M.st.num_files;
  ++M.st.num_host_inflated_files;
  if (bcf) M.append_bcf(file, data, n);
  else M.append_text(file, gz ? inflated : std::string(data, n));
}

void DeviceImporter::finish(std::vector<uint8_t>& cells) {
  Impl& M = *m_;
  IMP_HIP_CHECK(hipSetDevice(M.device));
  if (M.finished) throw VCF2BinaryException("DeviceImporter::finish called twice");
  M.finished = true;
  cells.clear();
  const uint64_t N = M.total_slots;
  if (N == 0 || M.total_cells == 0) { M.st.num_cells = 0; M.st.num_bytes = 0; M.free_batches(); return; }
  hipStream_t st = M.stream;
  DBuf<uint64_t> key, key_sorted, src, tag, sorted_size, sorted_off;
  DBuf<uint32_t> size, idx, idx_sorted;
  key.ensure(N); key_sorted.ensure(N); src.ensure(N); size.ensure(N); idx.ensure(N); idx_sorted.ensure(N);
  if (M.spanning) tag.ensure(N);
  IMP_HIP_CHECK(hipEventRecord(M.ev[0], st));
  uint64_t at = 0;
  for (const Impl::Batch& b : M.batches) {
    IMP_HIP_CHECK(hipMemcpyAsync(key.p + at, b.key, b.n_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    IMP_HIP_CHECK(hipMemcpyAsync(src.p + at, b.src, b.n_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    IMP_HIP_CHECK(hipMemcpyAsync(size.p + at, b.size, b.n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (M.spanning) IMP_HIP_CHECK(hipMemcpyAsync(tag.p + at, b.tag, b.n_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    at += b.n_slots;
  }
  IMP_HIP_CHECK(hipMemsetAsync(M.d_counters.p, 0, 4 * sizeof(unsigned long long), st));
  if (M.spanning_slots)
    hipLaunchKernelGGL(k_imp_resolve, dim3(grid_for(N)), dim3(kBlock), 0, st, key.p, (const uint64_t*)tag.p, N, (const unsigned long long*)M.d_row_best.p, M.H.key_row_bits,
                       M.H.max_row, M.d_counters.p);
  hipLaunchKernelGGL(k_imp_iota, dim3(grid_for(N)), dim3(kBlock), 0, st, idx.p, N);
  {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, key.p, key_sorted.p, idx.p, idx_sorted.p, (size_t)N, 0, 64, st));
    M.d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::radix_sort_pairs((void*)M.d_tmp.p, bytes, key.p, key_sorted.p, idx.p, idx_sorted.p, (size_t)N, 0, 64, st));
  }
  unsigned long long counters[4] = {0, 0, 0, 0};
  IMP_HIP_CHECK(hipMemcpyAsync(counters, M.d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipStreamSynchronize(st));
  const uint64_t kept = M.total_cells - counters[3];       // the dropped keys sort behind every cell
  M.st.num_spanning_cells = (int64_t)counters[2];
  M.st.num_cells = (int64_t)kept;
  uint64_t out_bytes = 0;
  DBuf<uint8_t> out;
  if (kept) {
    sorted_size.ensure(kept + 1); sorted_off.ensure(kept + 1);
    hipLaunchKernelGGL(k_imp_sorted_sizes, dim3(grid_for(kept + 1)), dim3(kBlock), 0, st, (const uint32_t*)idx_sorted.p, (const uint32_t*)size.p, kept, sorted_size.p);
    M.scan<uint64_t>(sorted_size.p, sorted_off.p, (size_t)kept + 1);
    IMP_HIP_CHECK(hipMemcpyAsync(&out_bytes, sorted_off.p + kept, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    IMP_HIP_CHECK(hipStreamSynchronize(st));
    out.ensure(out_bytes + 16);
    hipLaunchKernelGGL(k_imp_gather, dim3(grid_for(kept * 64)), dim3(kBlock), 0, st, (const uint32_t*)idx_sorted.p, (const uint64_t*)src.p, (const uint32_t*)size.p,
                       (const uint64_t*)sorted_off.p, kept, out.p, out_bytes);
  }
  IMP_HIP_CHECK(hipEventRecord(M.ev[1], st));
  IMP_HIP_CHECK(hipStreamSynchronize(st));
  float ms = 0;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, M.ev[0], M.ev[1]));
  M.st.ms_sort_gather += ms;
  const double t0 = now_s();
  cells.resize(out_bytes);
  if (out_bytes) IMP_HIP_CHECK(hipMemcpy(cells.data(), out.p, out_bytes, hipMemcpyDeviceToHost));
  M.st.s_d2h += now_s() - t0;
  M.st.num_bytes = out_bytes;
  M.free_batches();
}

std::vector<uint8_t> import_callsets_to_cells_device(const VidMapper& vid, const ImportOptions& opt, int device, uint64_t text_budget_bytes, ImportStats* stats,
                                                     int inflate_mode, const std::vector<ImportStream>& streams) {
  const double t0 = now_s();
  DeviceImporter imp(device, vid, opt, text_budget_bytes, inflate_mode);
  imp.import_all(streams);
  std::vector<uint8_t> out;
  imp.finish(out);
  if (stats) { *stats = imp.stats(); stats->s_total = now_s() - t0; }
  return out;
}

}  // namespace genomicsdb_amd
