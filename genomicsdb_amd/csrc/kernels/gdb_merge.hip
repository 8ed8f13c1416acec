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
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "../core/gdb_merge.hpp"
#include "../host/merge_common.hpp"
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
__global__ void __launch_bounds__(kBlock) k_merge_sizes(const uint64_t* ref, const uint64_t* size, const uint64_t* off, uint64_t n, uint64_t* out /* n + 1 */,
                                                       uint64_t* from /* n */) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) { const uint64_t g = ref[i]; out[i] = g < n ? size[g] : 0; from[i] = g < n ? off[g] : 0; }
  else if (i == n) out[i] = 0;
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
  for (size_t s = 0; s < k; ++s) {
    const uint64_t n = first[s + 1] - first[s];
    if (n) hipLaunchKernelGGL(k_merge_keys, dim3(grid_for(n)), dim3(kBlock), 0, q, (const uint8_t*)d_in.p, in_bytes, (const uint64_t*)d_off.p, first[s], n, d_key[0].p, d_size.p,
                              d_ref[0].p, d_err.p);
  }
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
  for (size_t s = 0; s < k; ++s) {
    const uint64_t n = first[s + 1] - first[s];
    if (n) hipLaunchKernelGGL(k_merge_check, dim3(grid_for(n)), dim3(kBlock), 0, q, (const MergeKey*)d_key[0].p, first[s], n, (int)s, d_bitmap.p + s * words, words, d_err.p);
  }
  if (k > 1) hipLaunchKernelGGL(k_merge_disjoint, dim3(grid_for(words)), dim3(kBlock), 0, q, (const uint32_t*)d_bitmap.p, (int)k, words, d_err.p);
  MERGE_HIP_CHECK(hipEventRecord(h.ev[1], q));
  MERGE_HIP_CHECK(hipMemcpyAsync(err.data(), d_err.p, n_err * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  for (size_t s = 0; s < k; ++s)
    if (err[kErrPerStream + s] != kNone) throw VCF2BinaryException(merge_unsorted_message(s, err[kErrPerStream + s]));
  if (err[kErrSharedRow] != kNone) throw VCF2BinaryException(merge_shared_row_message(err[kErrSharedRow]));
  // ---- rank: adjacent lists pairwise, in rounds; a merged pair takes the place of its two lists, so the lists stay contiguous
  std::vector<std::pair<uint64_t, uint64_t>> lists;       // (begin, count)
  for (size_t s = 0; s < k; ++s) lists.emplace_back(first[s], first[s + 1] - first[s]);
  int cur = 0;
  while (lists.size() > 1) {
    std::vector<std::pair<uint64_t, uint64_t>> next;
    for (size_t i = 0; i < lists.size(); i += 2) {
      const uint64_t b = lists[i].first, na = lists[i].second;
      if (i + 1 == lists.size()) {      // the odd one moves over as it is
        if (na) {
          MERGE_HIP_CHECK(hipMemcpyAsync(d_key[cur ^ 1].p + b, d_key[cur].p + b, na * sizeof(MergeKey), hipMemcpyDeviceToDevice, q));
          MERGE_HIP_CHECK(hipMemcpyAsync(d_ref[cur ^ 1].p + b, d_ref[cur].p + b, na * sizeof(uint64_t), hipMemcpyDeviceToDevice, q));
        }
        next.emplace_back(b, na);
        continue;
      }
      const uint64_t nb = lists[i + 1].second, b2 = lists[i + 1].first;
      const uint64_t tiles = (na + nb + kMergeTile - 1) / kMergeTile;
      if (tiles) hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)tiles), dim3(kMergeBlock), 0, q, (const MergeKey*)d_key[cur].p + b, (const uint64_t*)d_ref[cur].p + b, na,
                                    (const MergeKey*)d_key[cur].p + b2, (const uint64_t*)d_ref[cur].p + b2, nb, d_key[cur ^ 1].p + b, d_ref[cur ^ 1].p + b);
      next.emplace_back(b, na + nb);
    }
    lists.swap(next);
    cur ^= 1;
  }
  MERGE_HIP_CHECK(hipEventRecord(h.ev[2], q));
  // ---- scan
  hipLaunchKernelGGL(k_merge_sizes, dim3(grid_for(N + 1)), dim3(kBlock), 0, q, (const uint64_t*)d_ref[cur].p, (const uint64_t*)d_size.p, (const uint64_t*)d_off.p, N, d_msize.p,
                     d_mfrom.p);
  {
    size_t bytes = 0;
    MERGE_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, d_msize.p, d_moff.p, (uint64_t)0, (size_t)N + 1, rocprim::plus<uint64_t>(), q));
    d_tmp.alloc(std::max<size_t>(bytes, 16));
    MERGE_HIP_CHECK(rocprim::exclusive_scan((void*)d_tmp.p, bytes, d_msize.p, d_moff.p, (uint64_t)0, (size_t)N + 1, rocprim::plus<uint64_t>(), q));
  }
  uint64_t scanned = 0;
  MERGE_HIP_CHECK(hipMemcpyAsync(&scanned, d_moff.p + N, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
  MERGE_HIP_CHECK(hipEventRecord(h.ev[3], q));
  MERGE_HIP_CHECK(hipStreamSynchronize(q));
  if (scanned != out_bytes) throw VCF2BinaryException("merge: the merged sizes add up to " + std::to_string(scanned) + " bytes, the streams to " + std::to_string(out_bytes));
  // ---- gather
  d_out.alloc(out_bytes + 16);
  hipLaunchKernelGGL(k_merge_gather, dim3(grid_for(N * kGatherLanes)), dim3(kBlock), 0, q, (const uint64_t*)d_mfrom.p, (const uint64_t*)d_moff.p, N, (const uint8_t*)d_in.p,
                     in_bytes, d_out.p, out_bytes);
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

}  // namespace genomicsdb_amd
