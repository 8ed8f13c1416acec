// gdb_merge.hip - merge_cell_streams_device (host/vcf_importer.h): k sorted streams of begin-cells -> one, on one GPU.
// Kernels for gfx950 around the bodies of core/gdb_merge.hpp, and their orchestration (all launches on one stream):
//   offsets  the host walks each stream's size chain (host/merge_common.hpp) and uploads the streams and the cell offsets
//   keys     k_merge_keys: one thread per cell reads the unaligned 24-byte header -> (column, row) key, size, the cell's own index
//   checks   k_merge_check: every stream non-decreasing in key (first offender per stream), its rows into the stream's bitmap;
//            k_merge_disjoint: one thread per 32 rows looks for a row that two bitmaps share (the smallest wins)
//   rank     k_merge_rank, pairwise in rounds over (key, index) pairs: a workgroup owns kMergeTile output cells, finds the tile's two
//            merge-path splits by binary search over the key arrays, loads both key runs into LDS and ranks them there
//   scan     k_merge_sizes scatters the sizes and source offsets into merged order, a rocPRIM exclusive scan gives 64-bit output offsets
//   gather   k_merge_gather: 16 lanes per cell, consecutive lanes copy consecutive bytes - bytewise up to the destination's next
//            16-byte boundary and behind the last whole 16, 16 bytes per lane in between (aligned stores, loads at the source's alignment)
// Payload bytes move once.  Everything must fit in HBM together: checked against hipMemGetInfo before the allocations.
// merge_cell_files_device merges files to a file round by round through a bounded window of device memory (the rounds and their
// planner: host/merge_files_common.hpp).  Its rounds run the same launches on the cells below the round's watermark, and add
//   cut      k_merge_cut: per source the resident cells strictly below the watermark, by binary search over the source's keys
//   prefix   k_merge_prefix: the emitted prefixes side by side, as the lists of the rank rounds
//   carry    k_merge_carry: the tables of the kept cells -> the front of the other pool's tables (the kept bytes move as one block)
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "../core/gdb_merge.hpp"
#include "../host/merge_common.hpp"
#include "../host/merge_files_common.hpp"
#include "gdb_pipeline.h"

namespace genomicsdb_amd {

#define MERGE_HIP_CHECK(expr)                                                                                      \
  do {                                                                                                             \
    hipError_t _e = (expr);                                                                                        \
    if (_e != hipSuccess)                                                                                          \
      throw GenomicsDBDeviceException(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

namespace {
using namespace gdbmerge;

constexpr int kBlock = 256;
// error words: [0] bits, [1] largest row, [2] first cell (global index) with a negative row, [3] smallest shared row, [4 + s] first unsorted cell of stream s
enum { kErrBits = 0, kErrMaxRow = 1, kErrNegCell = 2, kErrSharedRow = 3, kErrPerStream = 4 };
enum : unsigned long long { kBitNegativeRow = 1, kBitBadCell = 2 };
constexpr unsigned long long kNone = ~0ull;

// The largest row and the row bitmaps are a few words that millions of cells agree on: a relaxed device-scope load (past the CU's own
// cache) says whether the atomic would change anything, and nearly every thread then skips it (44 ms -> see profiles/device_merge.md)
template <class T> __device__ __forceinline__ T merge_peek(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kBlock) k_merge_keys(const uint8_t* in, uint64_t in_bytes, const uint64_t* off, uint64_t first, uint64_t n, MergeKey* key,
                                                      uint64_t* size, uint64_t* ref, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = first + i, at = off[g];
  MergeKey k; k.col = 0; k.row = 0;
  uint64_t sz = 0;
  if (at + kMergeHeaderBytes <= in_bytes) merge_load_header(in + at, &k, &sz);
  if (sz < kMergeHeaderBytes || sz > in_bytes - at) { sz = 0; atomicOr(&err[kErrBits], kBitBadCell); }      // (the host walked this chain: cannot be)
  key[g] = k; size[g] = sz; ref[g] = g;
  if (k.row < 0) { atomicOr(&err[kErrBits], kBitNegativeRow); atomicMin(&err[kErrNegCell], (unsigned long long)g); }
  else if ((unsigned long long)k.row > merge_peek(&err[kErrMaxRow])) atomicMax(&err[kErrMaxRow], (unsigned long long)k.row);
}

__global__ void __launch_bounds__(kBlock) k_merge_check(const MergeKey* key, uint64_t first, uint64_t n, int stream, uint32_t* bitmap, uint64_t words,
                                                       unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const MergeKey k = key[first + i];
  if (i > 0 && merge_key_less(k, key[first + i - 1])) atomicMin(&err[kErrPerStream + stream], (unsigned long long)i);
  if (k.row >= 0 && ((uint64_t)k.row >> 5) < words) {
    const uint32_t bit = 1u << ((uint32_t)k.row & 31u);
    if (!(merge_peek(&bitmap[(uint64_t)k.row >> 5]) & bit)) atomicOr(&bitmap[(uint64_t)k.row >> 5], bit);
  }
}

__global__ void __launch_bounds__(kBlock) k_merge_disjoint(const uint32_t* bitmaps, int k, uint64_t words, unsigned long long* err) {
  const uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= words) return;
  uint32_t seen = 0, shared = 0;
  for (int s = 0; s < k; ++s) { const uint32_t b = bitmaps[(uint64_t)s * words + w]; shared |= seen & b; seen |= b; }
  if (shared) atomicMin(&err[kErrSharedRow], (unsigned long long)(w * 32u + (uint64_t)(__ffs((int)shared) - 1)));
}

// merge of A[0, na) and B[0, nb) into out[0, na + nb): one workgroup per kMergeTile output cells
__global__ void __launch_bounds__(kMergeBlock) k_merge_rank(const MergeKey* A, const uint64_t* a_ref, uint64_t na, const MergeKey* B, const uint64_t* b_ref, uint64_t nb,
                                                           MergeKey* out, uint64_t* out_ref) {
  __shared__ MergeKey s_keys[kMergeTile];
  __shared__ MergeTile s_tile;
  if (threadIdx.x == 0) s_tile = merge_tile_of(blockIdx.x, A, na, B, nb);
  __syncthreads();
  const MergeTile t = s_tile;
  const uint32_t n = t.na + t.nb;       // <= kMergeTile
  const uint64_t base = (uint64_t)blockIdx.x * kMergeTile;
  for (uint32_t i = threadIdx.x; i < n; i += kMergeBlock) s_keys[i] = i < t.na ? A[t.a0 + i] : B[t.b0 + (i - t.na)];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += kMergeBlock) {
    const uint32_t pos = merge_tile_position(s_keys, t, i);
    if (pos >= n) continue;
    out[base + pos] = s_keys[i];
    out_ref[base + pos] = i < t.na ? a_ref[t.a0 + i] : b_ref[t.b0 + (i - t.na)];
  }
}

// sizes and source offsets in merged order, so that the gather has one load between a cell's number and its bytes
// (limit: the rows of size[] and off[] - n for the in-core merge, whose tables hold the merged cells and no others)
__global__ void __launch_bounds__(kBlock) k_merge_sizes(const uint64_t* ref, const uint64_t* size, const uint64_t* off, uint64_t n, uint64_t limit, uint64_t* out /* n + 1 */,
                                                       uint64_t* from /* n */) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) { const uint64_t g = ref[i]; out[i] = g < limit ? size[g] : 0; from[i] = g < limit ? off[g] : 0; }
  else if (i == n) out[i] = 0;
}

// ---- the windowed merge (merge_cell_files_device)
// the cut: per source the number of resident cells strictly below the watermark, by binary search over the source's keys, and their
// bytes.  mode 0: cut at w, 1: every cell (all sources are exhausted), 2: none (a source has loaded no cell yet)
struct MergeCutSource { uint64_t first, cells, end; };      // the source's first row of the tables, its resident cells, the byte of the pool where they end
__global__ void __launch_bounds__(kBlock) k_merge_cut(const MergeKey* key, const uint64_t* off, const MergeCutSource* src, int k, MergeKey w, int mode,
                                                     unsigned long long* out /* 2 k: cells, bytes */) {
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= k) return;
  const MergeCutSource c = src[s];
  const uint64_t n = mode == 1 ? c.cells : mode == 2 ? 0 : merge_cut_below(key + c.first, c.cells, w);
  const uint64_t begin = c.cells ? off[c.first] : c.end, cut_at = n < c.cells ? off[c.first + n] : c.end;
  out[2 * s] = n;
  out[2 * s + 1] = cut_at - begin;
}
// the emitted prefix of a source, compact, as a list of the rank rounds: its keys and the rows they came from
__global__ void __launch_bounds__(kBlock) k_merge_prefix(const MergeKey* key, uint64_t first, uint64_t n, MergeKey* list_key, uint64_t* list_ref) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  list_key[i] = key[first + i];
  list_ref[i] = first + i;
}
// the carry of a source's tables: rows [from_row, from_row + n) of this round's tables -> rows [to_row, ..) of the other set, the
// offsets moved with the kept bytes (which the host copies as one block: they are contiguous)
__global__ void __launch_bounds__(kBlock) k_merge_carry(const MergeKey* key, const uint64_t* size, const uint64_t* off, uint64_t from_row, uint64_t n, uint64_t kept_from,
                                                       uint64_t kept_to, MergeKey* to_key, uint64_t* to_size, uint64_t* to_off, uint64_t to_row) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  to_key[to_row + i] = key[from_row + i];
  to_size[to_row + i] = size[from_row + i];
  to_off[to_row + i] = merge_carry_offset(off[from_row + i], kept_from, kept_to);
}

typedef uint32_t MergeVec16 __attribute__((ext_vector_type(4)));
typedef MergeVec16 MergeVec16Unaligned __attribute__((aligned(1)));      // a 16-byte global load at any address

// kGatherLanes consecutive lanes per cell.  k_imp_gather's scheme is a whole wavefront per cell; a begin-cell is some 160 bytes, 10 lanes'
// worth of 16-byte loads, and a wave that serves one cell spends its time waiting for that cell's offsets (profiles/device_merge.md)
constexpr uint32_t kGatherLanes = 16;
__global__ void __launch_bounds__(kBlock) k_merge_gather(const uint64_t* src_off, const uint64_t* out_off /* n + 1 */, uint64_t n, const uint8_t* in, uint64_t in_bytes,
                                                        uint8_t* out, uint64_t out_bytes) {
  const uint64_t cell = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kGatherLanes;
  if (cell >= n) return;
  const uint32_t lane = threadIdx.x % kGatherLanes;
  const uint64_t from = src_off[cell], at = out_off[cell], len = out_off[cell + 1] - at;
  if (from > in_bytes || len > in_bytes - from || at > out_bytes || len > out_bytes - at) return;
  const uint8_t* src = in + from;
  uint8_t* dst = out + at;
  const uint64_t to_boundary = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u, head = len < to_boundary ? len : to_boundary;
  const uint64_t nvec = (len - head) >> 4, tail = head + (nvec << 4);
  for (uint64_t i = lane; i < head; i += kGatherLanes) dst[i] = src[i];
  for (uint64_t v = lane; v < nvec; v += kGatherLanes)
    *reinterpret_cast<MergeVec16*>(dst + head + (v << 4)) = *reinterpret_cast<const MergeVec16Unaligned*>(src + head + (v << 4));
  for (uint64_t i = tail + lane; i < len; i += kGatherLanes) dst[i] = src[i];
}

template <class T> struct DMem {
  T* p = nullptr;
  void alloc(size_t n) { MERGE_HIP_CHECK(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T))); }
  ~DMem() { if (p) (void)hipFree(p); }
};
struct Handles {
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Handles() {
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

void refuse_if_too_large(uint64_t in_bytes, uint64_t key_bytes, uint64_t out_bytes) {
  size_t free_b = 0, total_b = 0;
  MERGE_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t slack = (uint64_t)256 << 20;       // scan scratch, runtime
  if (in_bytes + key_bytes + out_bytes + slack > (uint64_t)free_b)
    throw VCF2BinaryException("merge: the streams (" + std::to_string(in_bytes) + " bytes), their keys and tables (" + std::to_string(key_bytes) + " bytes) and the result (" +
                              std::to_string(out_bytes) + " bytes) must fit in device memory together, and " + std::to_string(free_b) + " of " + std::to_string(total_b) +
                              " bytes are free: arrays larger than device memory are not merged by this build");
}

// ---- the launches, shared by merge_cell_streams_device and merge_cell_files_device
// keys (and, for the caller that wants them, the cells' own rows as `ref`) of cells [first, first + n) of the offset table
void launch_keys(hipStream_t q, const uint8_t* in, uint64_t in_bytes, const uint64_t* off, uint64_t first, uint64_t n, MergeKey* key, uint64_t* size, uint64_t* ref,
                 unsigned long long* err) {
  if (n) hipLaunchKernelGGL(k_merge_keys, dim3(grid_for(n)), dim3(kBlock), 0, q, in, in_bytes, off, first, n, key, size, ref, err);
}
// order inside cells [first, first + n) of one stream (the offender counted from `first`) and their rows into the stream's bitmap
void launch_check(hipStream_t q, const MergeKey* key, uint64_t first, uint64_t n, int stream, uint32_t* bitmap, uint64_t words, unsigned long long* err) {
  if (n) hipLaunchKernelGGL(k_merge_check, dim3(grid_for(n)), dim3(kBlock), 0, q, key, first, n, stream, bitmap, words, err);
}
void launch_disjoint(hipStream_t q, const uint32_t* bitmaps, size_t k, uint64_t words, unsigned long long* err) {
  if (k > 1 && words) hipLaunchKernelGGL(k_merge_disjoint, dim3(grid_for(words)), dim3(kBlock), 0, q, bitmaps, (int)k, words, err);
}
// rank: adjacent lists (begin, count) of key[0] / ref[0] pairwise, in rounds between the two sets; a merged pair takes the place of its
// two lists, which must be contiguous.  Returns the set that holds the one merged list
int launch_rank_rounds(hipStream_t q, std::vector<std::pair<uint64_t, uint64_t>> lists, MergeKey* const key[2], uint64_t* const ref[2]) {
  int cur = 0;
  while (lists.size() > 1) {
    std::vector<std::pair<uint64_t, uint64_t>> next;
    for (size_t i = 0; i < lists.size(); i += 2) {
      const uint64_t b = lists[i].first, na = lists[i].second;
      if (i + 1 == lists.size()) {      // the odd one moves over as it is
        if (na) {
          MERGE_HIP_CHECK(hipMemcpyAsync(key[cur ^ 1] + b, key[cur] + b, na * sizeof(MergeKey), hipMemcpyDeviceToDevice, q));
          MERGE_HIP_CHECK(hipMemcpyAsync(ref[cur ^ 1] + b, ref[cur] + b, na * sizeof(uint64_t), hipMemcpyDeviceToDevice, q));
        }
        next.emplace_back(b, na);
        continue;
      }
      const uint64_t nb = lists[i + 1].second, b2 = lists[i + 1].first;
      const uint64_t tiles = (na + nb + kMergeTile - 1) / kMergeTile;
      if (tiles) hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)tiles), dim3(kMergeBlock), 0, q, (const MergeKey*)key[cur] + b, (const uint64_t*)ref[cur] + b, na,
                                    (const MergeKey*)key[cur] + b2, (const uint64_t*)ref[cur] + b2, nb, key[cur ^ 1] + b, ref[cur ^ 1] + b);
      next.emplace_back(b, na + nb);
    }
    lists.swap(next);
    cur ^= 1;
  }
  return cur;
}
// sizes and source offsets of the n merged cells (ref: their rows of size[] / off[], which have `limit` rows) and the scan -> moff[0, n]
size_t scan_scratch_bytes(uint64_t n, hipStream_t q) {
  size_t bytes = 0;
  MERGE_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), q));
  return std::max<size_t>(bytes, 16);
}
void launch_sizes_scan(hipStream_t q, const uint64_t* ref, const uint64_t* size, const uint64_t* off, uint64_t n, uint64_t limit, uint64_t* msize, uint64_t* moff,
                       uint64_t* mfrom, void* scratch, size_t scratch_bytes) {
  hipLaunchKernelGGL(k_merge_sizes, dim3(grid_for(n + 1)), dim3(kBlock), 0, q, ref, size, off, n, limit, msize, mfrom);
  MERGE_HIP_CHECK(rocprim::exclusive_scan(scratch, scratch_bytes, msize, moff, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), q));
}
void launch_gather(hipStream_t q, const uint64_t* mfrom, const uint64_t* moff, uint64_t n, const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_bytes) {
  if (n) hipLaunchKernelGGL(k_merge_gather, dim3(grid_for(n * kGatherLanes)), dim3(kBlock), 0, q, mfrom, moff, n, in, in_bytes, out, out_bytes);
}

}  // namespace

std::vector<uint8_t> merge_cell_streams_device(const std::vector<CellStream>& streams, int device, MergeStats* stats) {
  const double t_begin = now_s();
  MergeStats st;
  const size_t k = streams.size();
  if (k == 0) throw VCF2BinaryException("merge: at least one stream is needed");
  if (k > 4096) throw VCF2BinaryException("merge: " + std::to_string(k) + " streams, at most 4096 are merged at once");
  st.num_streams = (int64_t)k;
  st.tile = kMergeTile;
  // ---- offsets: the host walks the size chains; stream s lies at base[s] of the device copy, 16-byte aligned
  std::vector<uint64_t> base(k), first(k + 1, 0), offs;
  uint64_t in_bytes = 0, out_bytes = 0;
  for (size_t s = 0; s < k; ++s) {
    base[s] = in_bytes;
    merge_walk_cells((const uint8_t*)streams[s].data, streams[s].nbytes, s, base[s], offs);
    first[s + 1] = offs.size();
    in_bytes = align16(in_bytes + streams[s].nbytes);
    out_bytes += streams[s].nbytes;
  }
  const uint64_t N = offs.size();
  st.cells_in = (int64_t)N;
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the cell merge runs on the GPU and has no CPU fallback");
  MERGE_HIP_CHECK(hipSetDevice(device));
  std::vector<uint8_t> result;
  if (N == 0) { st.s_total = now_s() - t_begin; if (stats) *stats = st; return result; }
  // keys and (index) twice for the rounds, offsets, sizes, sizes in merged order and their scan, error words
  const uint64_t key_bytes = N * (2 * sizeof(MergeKey) + 2 * sizeof(uint64_t) + 3 * sizeof(uint64_t)) + 2 * (N + 1) * sizeof(uint64_t) + (kErrPerStream + k) * sizeof(uint64_t);
  refuse_if_too_large(in_bytes, key_bytes, out_bytes);
  Handles h;
  MERGE_HIP_CHECK(hipStreamCreate(&h.stream));
  for (auto& e : h.ev) MERGE_HIP_CHECK(hipEventCreate(&e));
  hipStream_t q = h.stream;
  DMem<uint8_t> d_in, d_out, d_tmp;
  DMem<uint64_t> d_off, d_size, d_ref[2], d_msize, d_moff, d_mfrom;
  DMem<MergeKey> d_key[2];
  DMem<unsigned long long> d_err;
  DMem<uint32_t> d_bitmap;
  d_in.alloc(in_bytes + 16); d_off.alloc(N); d_size.alloc(N); d_msize.alloc(N + 1); d_moff.alloc(N + 1); d_mfrom.alloc(N);
  for (int i = 0; i < 2; ++i) { d_key[i].alloc(N); d_ref[i].alloc(N); }
  const size_t n_err = kErrPerStream + k;
  d_err.alloc(n_err);
  // ---- upload
  double t0 = now_s();
  for (size_t s = 0; s < k; ++s)
    if (streams[s].nbytes) MERGE_HIP_CHECK(hipMemcpyAsync(d_in.p + base[s], streams[s].data, streams[s].nbytes, hipMemcpyHostToDevice, q));
  MERGE_HIP_CHECK(hipMemcpyAsync(d_off.p, offs.data(), N * sizeof(uint64_t), hipMemcpyHostToDevice, q));
  std::vector<unsigned long long> err(n_err, kNone);
  err[kErrBits] = 0; err[kErrMaxRow] = 0;
  MERGE_HIP_CHECK(hipMemcpyAsync(d_err.p, err.data(), n_err * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  st.s_h2d = now_s() - t0;
  // ---- keys
  MERGE_HIP_CHECK(hipEventRecord(h.ev[0], q));
  for (size_t s = 0; s < k; ++s) launch_keys(q, d_in.p, in_bytes, d_off.p, first[s], first[s + 1] - first[s], d_key[0].p, d_size.p, d_ref[0].p, d_err.p);
  MERGE_HIP_CHECK(hipMemcpyAsync(err.data(), d_err.p, n_err * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  auto stream_of = [&](uint64_t g) { size_t s = 0; while (s + 1 < k && g >= first[s + 1]) ++s; return s; };
  if (err[kErrBits] & kBitBadCell) throw VCF2BinaryException("merge: a cell header on the device does not match the size chain the host walked");
  if (err[kErrBits] & kBitNegativeRow) {
    const size_t s = stream_of(err[kErrNegCell]);
    throw VCF2BinaryException("merge: stream " + std::to_string(s) + ": cell " + std::to_string(err[kErrNegCell] - first[s]) + " has a negative row");
  }
  // ---- checks: one bitmap of rows per stream
  const uint64_t words = (uint64_t)(err[kErrMaxRow] >> 5) + 1u;
  if (words > ((uint64_t)1 << 40) / k) throw VCF2BinaryException("merge: row " + std::to_string(err[kErrMaxRow]) + " is too large for the row bitmaps of the disjointness check");
  refuse_if_too_large(in_bytes, key_bytes + words * k * sizeof(uint32_t), out_bytes);
  d_bitmap.alloc(words * k);
  MERGE_HIP_CHECK(hipMemsetAsync(d_bitmap.p, 0, words * k * sizeof(uint32_t), q));
  for (size_t s = 0; s < k; ++s) launch_check(q, d_key[0].p, first[s], first[s + 1] - first[s], (int)s, d_bitmap.p + s * words, words, d_err.p);
  launch_disjoint(q, d_bitmap.p, k, words, d_err.p);
  MERGE_HIP_CHECK(hipEventRecord(h.ev[1], q));
  MERGE_HIP_CHECK(hipMemcpyAsync(err.data(), d_err.p, n_err * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  for (size_t s = 0; s < k; ++s)
    if (err[kErrPerStream + s] != kNone) throw VCF2BinaryException(merge_unsorted_message(s, err[kErrPerStream + s]));
  if (err[kErrSharedRow] != kNone) throw VCF2BinaryException(merge_shared_row_message(err[kErrSharedRow]));
  // ---- rank
  std::vector<std::pair<uint64_t, uint64_t>> lists;       // (begin, count)
  for (size_t s = 0; s < k; ++s) lists.emplace_back(first[s], first[s + 1] - first[s]);
  MergeKey* const keys[2] = {d_key[0].p, d_key[1].p};
  uint64_t* const refs[2] = {d_ref[0].p, d_ref[1].p};
  const int cur = launch_rank_rounds(q, lists, keys, refs);
  MERGE_HIP_CHECK(hipEventRecord(h.ev[2], q));
  // ---- scan
  const size_t scratch_bytes = scan_scratch_bytes(N, q);
  d_tmp.alloc(scratch_bytes);
  launch_sizes_scan(q, d_ref[cur].p, d_size.p, d_off.p, N, N, d_msize.p, d_moff.p, d_mfrom.p, d_tmp.p, scratch_bytes);
  uint64_t scanned = 0;
  MERGE_HIP_CHECK(hipMemcpyAsync(&scanned, d_moff.p + N, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
  MERGE_HIP_CHECK(hipEventRecord(h.ev[3], q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  if (scanned != out_bytes) throw VCF2BinaryException("merge: the merged sizes add up to " + std::to_string(scanned) + " bytes, the streams to " + std::to_string(out_bytes));
  // ---- gather
  d_out.alloc(out_bytes + 16);
  launch_gather(q, d_mfrom.p, d_moff.p, N, d_in.p, in_bytes, d_out.p, out_bytes);
  MERGE_HIP_CHECK(hipEventRecord(h.ev[4], q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  MERGE_HIP_CHECK(hipGetLastError());
  MERGE_HIP_CHECK(hipEventElapsedTime(&st.ms_keys, h.ev[0], h.ev[1]));
  MERGE_HIP_CHECK(hipEventElapsedTime(&st.ms_rank, h.ev[1], h.ev[2]));
  MERGE_HIP_CHECK(hipEventElapsedTime(&st.ms_scan, h.ev[2], h.ev[3]));
  MERGE_HIP_CHECK(hipEventElapsedTime(&st.ms_gather, h.ev[3], h.ev[4]));
  t0 = now_s();
  result.resize(out_bytes);
  MERGE_HIP_CHECK(hipMemcpy(result.data(), d_out.p, out_bytes, hipMemcpyDeviceToHost));
  st.s_d2h = now_s() - t0;
  st.cells_out = (int64_t)N;
  st.bytes_out = out_bytes;
  st.s_total = now_s() - t_begin;
  if (stats) *stats = st;
  return result;
}

// ---- merge_cell_files_device: the backend of host/merge_files_common.hpp on the device.  Three streams, ordered by events: `in`
// uploads round r + 1 while `run` works on round r and `out` downloads what round r merged; the host meanwhile writes round r - 1
// and reads round r + 1.  Pool, table and staging `set` belong to the rounds with (round & 1) == set.
namespace {

struct MergeFilesDevice {
  struct Dev { void* p = nullptr; size_t cap = 0; };
  hipStream_t q_in = nullptr, q = nullptr, q_out = nullptr;
  hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_d2h[2] = {nullptr, nullptr}, ev_done = nullptr, ev_t[2][6] = {};
  Dev pool[2], t_key[2], t_size[2], t_off[2], w_key[2], w_ref[2], msize, moff, mfrom, d_out, scratch, ctl, bitmap;
  Dev h_bytes[2], h_offs[2], h_out[2], h_ctl;          // pinned
  size_t k = 0, want_pool = 0, want_cells = 0, scratch_want = 0;
  uint64_t words = 0;
  uint64_t dev_now = 0, dev_peak = 0, pinned_now = 0;
  int last_d2h = -1;
  bool timed[2] = {false, false};
  MergeFilesStats* st = nullptr;

  explicit MergeFilesDevice(MergeFilesStats* stats) : st(stats) {
    MERGE_HIP_CHECK(hipStreamCreate(&q_in));
    MERGE_HIP_CHECK(hipStreamCreate(&q));
    MERGE_HIP_CHECK(hipStreamCreate(&q_out));
    for (auto& e : ev_h2d) MERGE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : ev_d2h) MERGE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    MERGE_HIP_CHECK(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
    for (auto& set : ev_t) for (auto& e : set) MERGE_HIP_CHECK(hipEventCreate(&e));
  }
  MergeFilesDevice(const MergeFilesDevice&) = delete;
  MergeFilesDevice& operator=(const MergeFilesDevice&) = delete;
  ~MergeFilesDevice() {
    (void)hipDeviceSynchronize();        // (after a refusal transfers may still be under way)
    for (Dev* d : {&pool[0], &pool[1], &t_key[0], &t_key[1], &t_size[0], &t_size[1], &t_off[0], &t_off[1], &w_key[0], &w_key[1], &w_ref[0], &w_ref[1], &msize, &moff, &mfrom,
                   &d_out, &scratch, &ctl, &bitmap})
      if (d->p) (void)hipFree(d->p);
    for (Dev* d : {&h_bytes[0], &h_bytes[1], &h_offs[0], &h_offs[1], &h_out[0], &h_out[1], &h_ctl})
      if (d->p) (void)hipHostFree(d->p);
    for (auto& e : ev_h2d) if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_d2h) if (e) (void)hipEventDestroy(e);
    if (ev_done) (void)hipEventDestroy(ev_done);
    for (auto& set : ev_t) for (auto& e : set) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {q_in, q, q_out}) if (s) (void)hipStreamDestroy(s);
  }
  // a buffer of at least `bytes`; what it held is gone when it grows.  Nothing may be under way on it
  void device(Dev& d, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (bytes <= d.cap) return;
    if (d.p) { MERGE_HIP_CHECK(hipFree(d.p)); d.p = nullptr; dev_now -= d.cap; d.cap = 0; }
    MERGE_HIP_CHECK(hipMalloc(&d.p, bytes));
    d.cap = bytes; dev_now += bytes;
    dev_peak = std::max(dev_peak, dev_now);
  }
  void pinned(Dev& d, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (bytes <= d.cap) return;
    if (d.p) { MERGE_HIP_CHECK(hipHostFree(d.p)); d.p = nullptr; pinned_now -= d.cap; d.cap = 0; }
    MERGE_HIP_CHECK(hipHostMalloc(&d.p, bytes, hipHostMallocDefault));
    d.cap = bytes; pinned_now += bytes;
  }
  void pool_and_tables(int set) {
    device(pool[set], want_pool + 16);
    device(t_key[set], want_cells * sizeof(MergeKey)); device(t_size[set], want_cells * sizeof(uint64_t)); device(t_off[set], want_cells * sizeof(uint64_t));
  }
  // the words of the control block: [3 k cut sources][4 + k error words][2 k cut results]; the first two go up, the last two come down
  size_t ctl_up() const { return 3 * k + kErrPerStream + k; }
  size_t ctl_down() const { return kErrPerStream + k + 2 * k; }
  unsigned long long* d_err() const { return (unsigned long long*)ctl.p + 3 * k; }

  void reserve(uint64_t pool_bytes, uint64_t table_cells, size_t sources, int keep) {
    if (keep >= 0) MERGE_HIP_CHECK(hipDeviceSynchronize());      // growth: every buffer but the running round's is replaced
    k = sources; want_pool = pool_bytes; want_cells = table_cells;
    for (int set = 0; set < 2; ++set) {
      if (set != keep) pool_and_tables(set);
      device(w_key[set], want_cells * sizeof(MergeKey)); device(w_ref[set], want_cells * sizeof(uint64_t));
      pinned(h_bytes[set], want_pool + 16); pinned(h_offs[set], want_cells * sizeof(uint64_t)); pinned(h_out[set], want_pool + 16);
    }
    device(msize, (want_cells + 1) * sizeof(uint64_t)); device(moff, (want_cells + 1) * sizeof(uint64_t)); device(mfrom, want_cells * sizeof(uint64_t));
    device(d_out, want_pool + 16);
    scratch_want = scan_scratch_bytes(want_cells, q);
    device(scratch, scratch_want);
    device(ctl, (3 * k + kErrPerStream + k + 2 * k) * sizeof(uint64_t));
    pinned(h_ctl, (ctl_up() + ctl_down() + 2) * sizeof(uint64_t));
  }
  uint8_t* stage_bytes(int set) { return (uint8_t*)h_bytes[set].p; }
  uint64_t* stage_offs(int set) { return (uint64_t*)h_offs[set].p; }

  // a layout that does not fit the buffers never reaches a kernel
  void check_layout(const MergeRoundLayout& L, int set) const {
    for (size_t s = 0; s < k; ++s) {
      const uint64_t rows = L.kept_cells[s] + std::max(L.fresh_cells[s], L.read_len[s] / kMergeHeaderBytes), bytes = L.kept_bytes[s] + std::max(L.fresh_bytes[s], L.read_len[s]);
      if (L.first[s] + rows > t_off[set].cap / sizeof(uint64_t) || L.first[s] + rows > t_key[set].cap / sizeof(MergeKey) || L.rbase[s] + bytes > pool[set].cap ||
          L.rbase[s] + bytes > h_bytes[set].cap || L.first[s] + rows > h_offs[set].cap / sizeof(uint64_t) || L.first[s] + rows > w_ref[0].cap / sizeof(uint64_t))
        throw VCF2BinaryException("merge: the layout of stream " + std::to_string(s) + " does not fit the window's buffers");
    }
  }

  void upload(int set, const MergeRoundLayout& L) {
    check_layout(L, set);
    for (size_t s = 0; s < k; ++s) {
      if (!L.fresh_cells[s]) continue;
      const uint64_t at = L.rbase[s] + L.kept_bytes[s], row = L.first[s] + L.kept_cells[s];
      MERGE_HIP_CHECK(hipMemcpyAsync((uint8_t*)pool[set].p + at, stage_bytes(set) + at, L.fresh_bytes[s], hipMemcpyHostToDevice, q_in));
      MERGE_HIP_CHECK(hipMemcpyAsync((uint64_t*)t_off[set].p + row, stage_offs(set) + row, L.fresh_cells[s] * sizeof(uint64_t), hipMemcpyHostToDevice, q_in));
    }
    MERGE_HIP_CHECK(hipEventRecord(ev_h2d[set], q_in));
  }

  // the row bitmaps live for the whole merge and grow when a larger row appears
  void grow_bitmaps(uint64_t max_row) {
    const uint64_t need = (((max_row >> 5) + 1u) + 255u) & ~(uint64_t)255u;
    if (need <= words) return;
    if (need > ((uint64_t)1 << 40) / k) throw VCF2BinaryException("merge: row " + std::to_string(max_row) + " is too large for the row bitmaps of the disjointness check");
    Dev bigger;
    MERGE_HIP_CHECK(hipMalloc(&bigger.p, need * k * sizeof(uint32_t)));
    bigger.cap = need * k * sizeof(uint32_t);
    dev_now += bigger.cap; dev_peak = std::max(dev_peak, dev_now);
    hipError_t e = hipMemsetAsync(bigger.p, 0, bigger.cap, q);
    for (size_t s = 0; s < k && words && e == hipSuccess; ++s)
      e = hipMemcpyAsync((uint32_t*)bigger.p + s * need, (const uint32_t*)bitmap.p + s * words, words * sizeof(uint32_t), hipMemcpyDeviceToDevice, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) { (void)hipFree(bigger.p); dev_now -= bigger.cap; MERGE_HIP_CHECK(e); }
    if (bitmap.p) { (void)hipFree(bitmap.p); dev_now -= bitmap.cap; }
    bitmap = bigger; words = need;
  }

  MergeCutResult cut(int set, const MergeRoundLayout& L, const MergeWatermark& w, uint64_t max_row) {
    check_layout(L, set);
    MERGE_HIP_CHECK(hipStreamWaitEvent(q, ev_h2d[set], 0));
    grow_bitmaps(max_row);
    uint64_t* up = (uint64_t*)h_ctl.p;
    uint64_t* down = up + ctl_up();
    for (size_t s = 0; s < k; ++s) { up[3 * s] = L.first[s]; up[3 * s + 1] = L.cells(s); up[3 * s + 2] = L.rbase[s] + L.bytes(s); }
    uint64_t* err_up = up + 3 * k;
    for (size_t i = 0; i < kErrPerStream + k; ++i) err_up[i] = kNone;
    err_up[kErrBits] = 0; err_up[kErrMaxRow] = 0;
    MERGE_HIP_CHECK(hipMemcpyAsync(ctl.p, up, ctl_up() * sizeof(uint64_t), hipMemcpyHostToDevice, q));
    MERGE_HIP_CHECK(hipEventRecord(ev_t[set][0], q));
    const MergeKey* key = (const MergeKey*)t_key[set].p;
    for (size_t s = 0; s < k; ++s) {
      const uint64_t row = L.first[s] + L.kept_cells[s], n = L.fresh_cells[s];
      launch_keys(q, (const uint8_t*)pool[set].p, pool[set].cap, (const uint64_t*)t_off[set].p, row, n, (MergeKey*)t_key[set].p, (uint64_t*)t_size[set].p, (uint64_t*)w_ref[0].p, d_err());
      launch_check(q, key, row, n, (int)s, (uint32_t*)bitmap.p + s * words, words, d_err());
    }
    launch_disjoint(q, (const uint32_t*)bitmap.p, k, words, d_err());
    hipLaunchKernelGGL(k_merge_cut, dim3(grid_for(k)), dim3(kBlock), 0, q, key, (const uint64_t*)t_off[set].p, (const MergeCutSource*)ctl.p, (int)k, w.key, w.all ? 1 : w.nothing ? 2 : 0,
                       d_err() + kErrPerStream + k);
    MERGE_HIP_CHECK(hipEventRecord(ev_t[set][1], q));
    MERGE_HIP_CHECK(hipMemcpyAsync(down, d_err(), ctl_down() * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
    MERGE_HIP_CHECK(hipStreamSynchronize(q));
    MERGE_HIP_CHECK(hipGetLastError());
    float ms = 0;
    MERGE_HIP_CHECK(hipEventElapsedTime(&ms, ev_t[set][0], ev_t[set][1]));
    st->ms_keys += ms;
    MergeCutResult c(k);
    c.bad_cell = (down[kErrBits] & kBitBadCell) != 0;
    if (down[kErrBits] & kBitNegativeRow) {
      const uint64_t g = down[kErrNegCell];
      for (size_t s = 0; s < k; ++s) {
        const uint64_t row = L.first[s] + L.kept_cells[s];
        if (g >= row && g < row + L.fresh_cells[s]) { c.negative_source = (int64_t)s; c.negative_cell = g - row; }
      }
      if (c.negative_source < 0) c.bad_cell = true;
    }
    for (size_t s = 0; s < k; ++s) {
      c.unsorted[s] = down[kErrPerStream + s];
      c.emit_cells[s] = down[kErrPerStream + k + 2 * s]; c.emit_bytes[s] = down[kErrPerStream + k + 2 * s + 1];
    }
    c.shared_row = down[kErrSharedRow];
    return c;
  }

  void merge_and_carry(int set, const MergeRoundLayout& L, const MergeCutResult& c, const MergeRoundLayout& next) {
    const int other = set ^ 1;
    pool_and_tables(other);           // (after a growth: nothing is under way on the other set, whose last round is over)
    check_layout(next, other);
    uint64_t total = 0, out_bytes = 0;
    for (size_t s = 0; s < k; ++s) { total += c.emit_cells[s]; out_bytes += c.emit_bytes[s]; }
    if (total > want_cells || out_bytes > d_out.cap || out_bytes > h_out[set].cap) throw VCF2BinaryException("merge: a round's output does not fit the window's buffers");
    MergeKey* const keys[2] = {(MergeKey*)w_key[0].p, (MergeKey*)w_key[1].p};
    uint64_t* const refs[2] = {(uint64_t*)w_ref[0].p, (uint64_t*)w_ref[1].p};
    uint64_t* scanned = (uint64_t*)h_ctl.p + ctl_up() + ctl_down();
    if (total) {
      MERGE_HIP_CHECK(hipEventRecord(ev_t[set][2], q));
      std::vector<std::pair<uint64_t, uint64_t>> lists;
      uint64_t at = 0;
      for (size_t s = 0; s < k; ++s) {
        const uint64_t n = c.emit_cells[s];
        if (!n) continue;
        hipLaunchKernelGGL(k_merge_prefix, dim3(grid_for(n)), dim3(kBlock), 0, q, (const MergeKey*)t_key[set].p, L.first[s], n, keys[0] + at, refs[0] + at);
        lists.emplace_back(at, n);
        at += n;
      }
      const int cur = launch_rank_rounds(q, lists, keys, refs);
      MERGE_HIP_CHECK(hipEventRecord(ev_t[set][3], q));
      launch_sizes_scan(q, refs[cur], (const uint64_t*)t_size[set].p, (const uint64_t*)t_off[set].p, total, t_off[set].cap / sizeof(uint64_t), (uint64_t*)msize.p,
                        (uint64_t*)moff.p, (uint64_t*)mfrom.p, scratch.p, scratch_want);
      MERGE_HIP_CHECK(hipMemcpyAsync(&scanned[set], (uint64_t*)moff.p + total, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
      MERGE_HIP_CHECK(hipEventRecord(ev_t[set][4], q));
      if (last_d2h >= 0) MERGE_HIP_CHECK(hipStreamWaitEvent(q, ev_d2h[last_d2h], 0));      // the one output buffer: its last download must be over
      launch_gather(q, (const uint64_t*)mfrom.p, (const uint64_t*)moff.p, total, (const uint8_t*)pool[set].p, pool[set].cap, (uint8_t*)d_out.p, out_bytes);
      MERGE_HIP_CHECK(hipEventRecord(ev_t[set][5], q));
      MERGE_HIP_CHECK(hipEventRecord(ev_done, q));
    }
    // the carry: the kept cells of a source are one block of bytes; tables by kernel
    for (size_t s = 0; s < k; ++s) {
      const uint64_t n = next.kept_cells[s];
      if (!n) continue;
      const uint64_t from = L.rbase[s] + c.emit_bytes[s], to = next.rbase[s];
      MERGE_HIP_CHECK(hipMemcpyAsync((uint8_t*)pool[other].p + to, (const uint8_t*)pool[set].p + from, next.kept_bytes[s], hipMemcpyDeviceToDevice, q));
      hipLaunchKernelGGL(k_merge_carry, dim3(grid_for(n)), dim3(kBlock), 0, q, (const MergeKey*)t_key[set].p, (const uint64_t*)t_size[set].p, (const uint64_t*)t_off[set].p,
                         L.first[s] + c.emit_cells[s], n, from, to, (MergeKey*)t_key[other].p, (uint64_t*)t_size[other].p, (uint64_t*)t_off[other].p, next.first[s]);
    }
    if (total) {
      MERGE_HIP_CHECK(hipStreamWaitEvent(q_out, ev_done, 0));
      MERGE_HIP_CHECK(hipMemcpyAsync(h_out[set].p, d_out.p, out_bytes, hipMemcpyDeviceToHost, q_out));
      MERGE_HIP_CHECK(hipEventRecord(ev_d2h[set], q_out));
      last_d2h = set;
      timed[set] = true;
    }
  }

  const uint8_t* collect(int set, uint64_t nbytes) {
    MERGE_HIP_CHECK(hipEventSynchronize(ev_d2h[set]));
    const uint64_t scanned = ((const uint64_t*)h_ctl.p)[ctl_up() + ctl_down() + (size_t)set];
    if (scanned != nbytes) throw VCF2BinaryException("merge: the merged sizes add up to " + std::to_string(scanned) + " bytes, the round's cells to " + std::to_string(nbytes));
    if (timed[set]) {
      float ms = 0;
      MERGE_HIP_CHECK(hipEventElapsedTime(&ms, ev_t[set][2], ev_t[set][3])); st->ms_rank += ms;
      MERGE_HIP_CHECK(hipEventElapsedTime(&ms, ev_t[set][3], ev_t[set][4])); st->ms_scan += ms;
      MERGE_HIP_CHECK(hipEventElapsedTime(&ms, ev_t[set][4], ev_t[set][5])); st->ms_gather += ms;
      timed[set] = false;
    }
    return (const uint8_t*)h_out[set].p;
  }
};

}  // namespace

uint64_t merge_cell_files_device(const std::vector<CellSource>& sources, const std::string& output_path, const MergeFilesOptions& options, MergeFilesStats* stats) {
  const double t_begin = now_s();
  MergeFilesStats st;
  if (sources.empty()) throw VCF2BinaryException("merge: at least one stream is needed");
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the cell merge runs on the GPU and has no CPU fallback");
  MERGE_HIP_CHECK(hipSetDevice(options.device));
  uint64_t window = options.window_bytes;
  if (!window) {      // a sixteenth of what is free (the buffers take 8.7 windows), at most 64 MiB: the fastest window measured, since a
                      // larger one only adds to the time spent allocating pinned staging (profiles/device_merge_files.md)
    size_t free_b = 0, total_b = 0;
    MERGE_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    window = std::max<uint64_t>(std::min<uint64_t>((uint64_t)free_b / 16, (uint64_t)64 << 20), (uint64_t)1 << 20);
  }
  MergeFilesPlanner plan(sources, window);
  uint64_t cells = 0;
  {
    MergeFilesDevice dev(&st);
    try {
      cells = merge_files_run(plan, output_path, dev, st);
    } catch (...) {
      st.device_bytes_peak = dev.dev_peak; st.pinned_bytes = dev.pinned_now;
      throw;
    }
    st.device_bytes_peak = dev.dev_peak; st.pinned_bytes = dev.pinned_now;
  }
  st.s_total = now_s() - t_begin;
  if (stats) *stats = st;
  return cells;
}


}  // namespace genomicsdb_amd
