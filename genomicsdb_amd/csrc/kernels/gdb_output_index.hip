// gdb_output_index.hip - see gdb_output_index.h.  Kernels for gfx950 around the bodies of core/gdb_output_index.hpp and core/gdb_index.hpp,
// and their orchestration per page.
#include "gdb_output_index.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstring>

#include "../core/gdb_output_index.hpp"
#include "../host/vcf_importer.h"
#include "../host/vcf_index.h"
#include "gdb_import_device.hpp"

namespace genomicsdb_amd {

namespace {
using namespace gdbidx;
using namespace gdboidx;
using namespace impdev;

constexpr int kOErrWords = 5;      // [0]: error bits, [1 + b]: smallest record of the page that raised bit b
constexpr size_t kRecordBytes = 2 * 8 + 9 * 4;      // per record of a page: two 64-bit offsets and nine 32-bit tables

struct ORecOut { uint64_t* a; uint64_t* b; uint32_t* bin; uint32_t* w0; uint32_t* w1; uint32_t* kid; uint32_t* rec; };

__device__ __forceinline__ void oidx_raise(uint32_t* err, uint32_t bits, uint32_t rec) {
  atomicOr(&err[0], bits);
  for (uint32_t b = 0; b < (uint32_t)kOErrWords - 1u; ++b) if (bits & (1u << b)) atomicMin(&err[1u + b], rec);
}
__device__ __forceinline__ void oidx_store(const ORecOut& O, uint32_t r, uint64_t ub, uint64_t ue, const OutRec& o, uint32_t n_kid, uint32_t* err) {
  if (o.err) oidx_raise(err, o.err, r);
  O.a[r] = ub; O.b[r] = ue; O.bin[r] = o.bin; O.w0[r] = o.w0; O.w1[r] = o.w1;
  O.kid[r] = (o.err == 0u && o.kid < n_kid) ? o.kid : n_kid;      // the sort's key: records that are not indexed come last
  O.rec[r] = r;
}

// one thread per record of the page: rec_off points at the page's first record, n_rec + 1 offsets are read
__global__ void __launch_bounds__(kBlock) k_oidx_text_records(const char* page, uint64_t page_bytes, const uint64_t* rec_off, uint64_t base, uint32_t n_rec, ContigTable C, uint32_t hint,
                                                             ORecOut O, uint32_t* err) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t ub = rec_off[r] - base, ue = rec_off[r + 1u] - base;
  OutRec o;
  o.bin = 0; o.w0 = 0; o.w1 = 0; o.kid = kNoContig; o.err = OIDX_ERR_SHAPE;
  if (rec_off[r] >= base && ub <= ue && ue <= page_bytes && ue - ub < ((uint64_t)1 << 32)) o = oidx_text_record(page + ub, (uint32_t)(ue - ub), C, hint);
  oidx_store(O, r, ub, ue, o, C.n, err);
}
__global__ void __launch_bounds__(kBlock) k_oidx_bcf_records(const char* page, uint64_t page_bytes, const uint64_t* rec_off, uint64_t base, uint32_t n_rec, uint32_t n_ref, ORecOut O,
                                                            uint32_t* err) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t ub = rec_off[r] - base, ue = rec_off[r + 1u] - base;
  OutRec o;
  o.bin = 0; o.w0 = 0; o.w1 = 0; o.kid = kNoContig; o.err = OIDX_ERR_SHAPE;
  if (rec_off[r] >= base && ub <= ue && ue <= page_bytes) o = oidx_bcf_record((const uint8_t*)page + ub, ue - ub, n_ref);
  oidx_store(O, r, ub, ue, o, n_ref, err);
}

// behind the deflate: the uncompressed offsets become page-relative virtual offsets, in place.  vend[n_rec] = the offset behind the page
__global__ void __launch_bounds__(kBlock) k_oidx_voff(uint64_t* a, uint64_t* b, uint32_t n_rec, const uint64_t* boff, uint32_t nblocks, uint32_t B, uint64_t page_bytes) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r == n_rec) b[r] = oidx_voff(boff, nblocks, B, page_bytes, page_bytes);
  if (r >= n_rec) return;
  const uint64_t ub = a[r], ue = b[r];
  a[r] = oidx_voff(boff, nblocks, B, page_bytes, ub < page_bytes ? ub : page_bytes);
  b[r] = oidx_voff(boff, nblocks, B, page_bytes, ue < page_bytes ? ue : page_bytes);
}

// records in contig order (kid_s ascending, file order inside a contig; ord: the record): chead has n_rec + 1 entries, the last one 0
__global__ void __launch_bounds__(kBlock) k_oidx_chunk_heads(const uint32_t* kid_s, const uint32_t* ord, const uint32_t* bin, uint32_t n_rec, uint32_t n_kid, uint32_t* chead) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == n_rec) chead[i] = 0u;
  if (i >= n_rec) return;
  const uint32_t p = i ? i - 1u : 0u;
  chead[i] = (kid_s[i] < n_kid && idx_chunk_head(i == 0u, kid_s[i], bin[ord[i]], kid_s[p], bin[ord[p]])) ? 1u : 0u;
}
__global__ void __launch_bounds__(kBlock) k_oidx_chunk_firsts(const uint32_t* chead, const uint32_t* coff, uint32_t n_rec, uint32_t n_chunks, uint32_t* cfirst) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n_rec && chead[i] && coff[i] < n_chunks) cfirst[coff[i]] = i;
}
// one thread per record; the last record of a chunk writes it: vbeg of the chunk's first record, vend of this one
__global__ void __launch_bounds__(kBlock) k_oidx_chunks(const uint32_t* cfirst, const uint32_t* chead, const uint32_t* coff, const uint32_t* kid_s, const uint32_t* ord, const uint32_t* bin,
                                                       const uint64_t* vbeg, const uint64_t* vend, uint32_t n_rec, uint32_t n_kid, uint32_t n_chunks, IdxChunk* chunks) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_rec || kid_s[i] >= n_kid) return;
  const bool last = i + 1u == n_rec;
  if (!oidx_chunk_tail(last, last ? 0u : kid_s[i + 1u], n_kid, !last && chead[i + 1u] != 0u)) return;
  const uint32_t c = coff[i] + chead[i] - 1u;      // (an indexed record has a head at or in front of it: never below 0)
  if (c >= n_chunks) return;                       // (never, by the scan)
  const uint32_t i0 = cfirst[c];
  if (i0 > i) return;                              // (never)
  IdxChunk k;
  k.tid = kid_s[i0]; k.bin = bin[ord[i0]];
  k.beg = vbeg[ord[i0]]; k.end = vend[ord[i]];
  k.count = i - i0 + 1u;
  k.flags = ((i0 == 0u || kid_s[i0 - 1u] != k.tid) ? IDX_CHUNK_FIRST : 0u) | ((last || kid_s[i + 1u] != k.tid) ? IDX_CHUNK_LAST : 0u);
  chunks[c] = k;
}

// 1 + the largest window per contig of the page: a lane whose neighbour in front is of the same contig and reaches at least as far issues nothing
__global__ void __launch_bounds__(kBlock) k_oidx_window_extent(const uint32_t* kid_s, const uint32_t* ord, const uint32_t* w1, uint32_t n_rec, uint32_t n_kid, uint32_t* extent) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < n_rec;
  const uint32_t kid = valid ? kid_s[i] : UINT32_MAX, mine = valid ? w1[ord[i]] : 0u;
  const uint32_t pkid = (uint32_t)__shfl_up((int)kid, 1, 64), pw = (uint32_t)__shfl_up((int)mine, 1, 64);
  const bool covered = (threadIdx.x & 63u) != 0u && pkid == kid && pw >= mine;
  if (valid && !covered && kid < n_kid) atomicMax(&extent[kid], mine + 1u);
}

// One thread per record, in contig order: the lane loops over its windows and issues the 64-bit atomicMin only where the lane in front
// does not cover the window too (idx_window_mine; no record of the file is at virtual offset 0, so the neighbour's offset is passed as 1).
// tally[0]: atomics issued
__global__ void __launch_bounds__(kBlock) k_oidx_windows(const uint32_t* kid_s, const uint32_t* ord, const uint64_t* vbeg, const uint32_t* w0, const uint32_t* w1, uint32_t n_rec,
                                                        const uint32_t* win_off, uint32_t n_kid, unsigned long long* win, uint32_t n_win, unsigned long long* tally) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool valid = i < n_rec;
  uint32_t kid = UINT32_MAX, a = 1u, b = 0u;
  uint64_t vb = 0;
  if (valid) { const uint32_t r = ord[i]; kid = kid_s[i]; a = w0[r]; b = w1[r]; vb = vbeg[r]; }
  const uint32_t pkid = (uint32_t)__shfl_up((int)kid, 1, 64), pa = (uint32_t)__shfl_up((int)a, 1, 64), pb = (uint32_t)__shfl_up((int)b, 1, 64);
  uint32_t issued = 0;
  if (valid && kid < n_kid) {
    const uint32_t base = win_off[kid];
    for (uint32_t w = a; w <= b; ++w) {
      if (!idx_window_mine(lane != 0u, kid, w, pkid, pa, pb, 1u)) continue;
      const uint64_t at = (uint64_t)base + w;
      if (at < n_win) { atomicMin(&win[at], (unsigned long long)vb); ++issued; }      // (always inside: the extent pass sized it)
    }
  }
  for (int d = 32; d; d >>= 1) issued += (uint32_t)__shfl_xor((int)issued, d, 64);
  if (lane == 0u && issued) atomicAdd(&tally[0], (unsigned long long)issued);
}

std::string record_error(uint32_t bits, int64_t line, int64_t record, bool bcf) {
  if (!bcf && (bits & (IDX_ERR_POS_LOW | IDX_ERR_RANGE))) return tbi_record_error(bits, "the output stream", line);
  const std::string where = " (record " + std::to_string(record) + " of the output stream)";
  if (bits & IDX_ERR_POS_LOW) return "index: a record with a negative POS is not indexed" + where;
  if (bits & OIDX_ERR_CHROM) return "index: a record whose CHROM the header has no ##contig line for" + where;
  return "index: a record that does not lie inside its page, or is too short or too long" + where;
}

}  // namespace

struct DeviceOutputIndexer::Impl {
  bool bcf = false;
  uint32_t n_kid = 0;
  int64_t header_lines = 0, records_before = 0;
  OutputIndexMerger merger;
  int device = 0;
  DBuf<char> d_names; DBuf<uint32_t> d_name_off;
  // per page arena
  template <class T> struct View { T* p = nullptr; };      // a table inside the set's slab
  struct Set {
    // the per-record tables and the error words are one allocation: a device allocation costs far more than the kernels of a small page
    DBuf<char> slab;
    size_t cap = 0;                                         // records the slab holds (+ 1 for the offset behind the page)
    View<uint64_t> a, b;
    View<uint32_t> bin, w0, w1, kid, rec, kid_s, ord, chead, coff, err;
    DBuf<uint32_t> cfirst;
    DBuf<IdxChunk> chunks;
    void carve(size_t n) {
      slab.ensure(n * kRecordBytes + kOErrWords * sizeof(uint32_t));
      cap = n;
      char* p = slab.p;
      a.p = (uint64_t*)p; p += n * 8; b.p = (uint64_t*)p; p += n * 8;
      for (View<uint32_t>* v : {&bin, &w0, &w1, &kid, &rec, &kid_s, &ord, &chead, &coff}) { v->p = (uint32_t*)p; p += n * 4; }
      err.p = (uint32_t*)p;
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // records: 0-1, voff: 2-3
    hipStream_t stream = nullptr;
    uint32_t n_rec = 0;
    uint64_t page_bytes = 0;
    bool records_queued = false, blocks_queued = false;
    uint64_t bytes() const { return slab.cap + cfirst.cap * 4 + chunks.cap * sizeof(IdxChunk); }
  } set[2];
  // shared by the two sets: used by merge_page only, which leaves the stream idle
  DBuf<char> d_tmp;
  DBuf<uint32_t> d_extent, d_win_off;
  DBuf<unsigned long long> d_win, d_tally;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};        // chunks: 0-1, linear: 2-3
  bool tally_ready = false;

  Impl(bool bcf_, const std::vector<std::string>& contigs, uint64_t header_bytes) : bcf(bcf_), merger(bcf_, contigs, header_bytes) {}
  void scan(hipStream_t stream, const uint32_t* in, uint32_t* out, size_t n) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::exclusive_scan((void*)d_tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), stream));
  }
  void sort_pairs(hipStream_t stream, const uint32_t* k_in, uint32_t* k_out, const uint32_t* v_in, uint32_t* v_out, size_t n, unsigned bits) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::radix_sort_pairs((void*)d_tmp.p, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
  }
  uint64_t table_bytes() const { return set[0].bytes() + set[1].bytes() + d_tmp.cap + (d_extent.cap + d_win_off.cap) * 4 + (d_win.cap + d_tally.cap) * 8; }
};

DeviceOutputIndexer::DeviceOutputIndexer(bool bcf, const std::vector<std::string>& header_contigs, uint64_t header_compressed_bytes, int64_t header_lines)
    : m_(new Impl(bcf, header_contigs, header_compressed_bytes)) {
  m_->header_lines = header_lines;
  if (header_contigs.size() >= ((size_t)1 << 31)) { delete m_; throw GenomicsDBDeviceException("index: too many contigs"); }
  m_->n_kid = (uint32_t)header_contigs.size();
}
DeviceOutputIndexer::~DeviceOutputIndexer() {
  for (Impl::Set& s : m_->set) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    for (hipEvent_t e : s.ev) if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : m_->ev) if (e) (void)hipEventDestroy(e);
  delete m_;
}

void DeviceOutputIndexer::page_records(int arena, const DevicePipeline::PageView& page, void* stream_) {
  Impl& S = *m_;
  Impl::Set& T = S.set[arena & 1];
  const hipStream_t stream = (hipStream_t)stream_;
  T.records_queued = false; T.blocks_queued = false;
  if (!page.valid || page.last <= page.first) { T.n_rec = 0; return; }
  if (page.last - page.first >= ((int64_t)1 << 31)) throw GenomicsDBDeviceException("index: 2^31 records or more in one page");
  const uint32_t n_rec = (uint32_t)(page.last - page.first);
  IMP_HIP_CHECK(hipGetDevice(&S.device));
  if (!T.ev[0]) for (hipEvent_t& e : T.ev) IMP_HIP_CHECK(hipEventCreate(&e));
  if (!S.ev[0]) for (hipEvent_t& e : S.ev) IMP_HIP_CHECK(hipEventCreate(&e));
  if (!S.bcf && !S.d_name_off.p) {      // the header's contig names, once
    std::vector<uint32_t> off(1, 0u);
    std::string bytes;
    for (const std::string& n : S.merger.contigs) { bytes += n; off.push_back((uint32_t)bytes.size()); }
    S.d_names.ensure(std::max<size_t>(bytes.size(), 1)); S.d_name_off.ensure(off.size());
    if (!bytes.empty()) IMP_HIP_CHECK(hipMemcpy(S.d_names.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    IMP_HIP_CHECK(hipMemcpy(S.d_name_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (T.cap < (size_t)n_rec + 1) {      // growing frees tables that work queued for the set's page in front may still use
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    T.carve((size_t)n_rec + (n_rec >> 3) + 64);
  }
  T.stream = stream; T.n_rec = n_rec; T.page_bytes = page.nbytes;
  IMP_HIP_CHECK(hipMemsetAsync(T.err.p, 0, sizeof(uint32_t), stream));
  IMP_HIP_CHECK(hipMemsetAsync(T.err.p + 1, 0xFF, (kOErrWords - 1) * sizeof(uint32_t), stream));
  const ORecOut O{T.a.p, T.b.p, T.bin.p, T.w0.p, T.w1.p, T.kid.p, T.rec.p};
  IMP_HIP_CHECK(hipEventRecord(T.ev[0], stream));
  if (S.bcf)
    hipLaunchKernelGGL(k_oidx_bcf_records, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, page.page, page.nbytes, page.rec_off + page.first, page.base, n_rec, S.n_kid, O, T.err.p);
  else
    hipLaunchKernelGGL(k_oidx_text_records, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, page.page, page.nbytes, page.rec_off + page.first, page.base, n_rec,
                       ContigTable{S.d_names.p, S.d_name_off.p, S.n_kid}, S.merger.last_contig(), O, T.err.p);
  IMP_HIP_CHECK(hipEventRecord(T.ev[1], stream));
  T.records_queued = true;
}

void DeviceOutputIndexer::page_blocks(int arena, const uint64_t* d_boff, uint64_t nblocks, uint32_t block_input, void* stream_) {
  Impl& S = *m_;
  Impl::Set& T = S.set[arena & 1];
  if (!T.records_queued) return;
  const hipStream_t stream = (hipStream_t)stream_;
  if (!d_boff || block_input == 0u || nblocks != (T.page_bytes + block_input - 1) / block_input || nblocks >= ((uint64_t)1 << 31))
    throw GenomicsDBDeviceException("index: the compressor's block table does not belong to the page");
  IMP_HIP_CHECK(hipEventRecord(T.ev[2], stream));
  hipLaunchKernelGGL(k_oidx_voff, dim3(grid_for((uint64_t)T.n_rec + 1)), dim3(kBlock), 0, stream, T.a.p, T.b.p, T.n_rec, d_boff, (uint32_t)nblocks, block_input, T.page_bytes);
  IMP_HIP_CHECK(hipEventRecord(T.ev[3], stream));
  T.blocks_queued = true;
}

void DeviceOutputIndexer::merge_page(int arena, uint64_t compressed_bytes) {
  Impl& S = *m_;
  Impl::Set& T = S.set[arena & 1];
  if (!T.records_queued || !T.blocks_queued || T.n_rec == 0) {      // a page without records
    T.records_queued = false;
    const double t0 = now_s();
    S.merger.add_page(nullptr, 0, 0, nullptr, std::vector<uint32_t>(S.n_kid, 0u).data(), nullptr, compressed_bytes);
    st.s_write += now_s() - t0;
    return;
  }
  T.records_queued = false; T.blocks_queued = false;
  IMP_HIP_CHECK(hipSetDevice(S.device));
  const hipStream_t stream = T.stream;
  const uint32_t n_rec = T.n_rec, n_kid = S.n_kid;
  unsigned kid_bits = 1;
  while (kid_bits < 32u && (n_kid >> kid_bits) != 0u) ++kid_bits;      // (n_kid itself is a key: the records that are not indexed)
  if (!S.tally_ready) { S.d_tally.ensure(1); IMP_HIP_CHECK(hipMemsetAsync(S.d_tally.p, 0, sizeof(unsigned long long), stream)); S.tally_ready = true; }
  // ---- contig order, chunk heads, the extent of the windows
  S.d_extent.ensure(std::max<uint32_t>(n_kid, 1)); S.d_win_off.ensure(std::max<uint32_t>(n_kid, 1));
  IMP_HIP_CHECK(hipEventRecord(S.ev[0], stream));
  S.sort_pairs(stream, T.kid.p, T.kid_s.p, T.rec.p, T.ord.p, n_rec, kid_bits);
  hipLaunchKernelGGL(k_oidx_chunk_heads, dim3(grid_for((uint64_t)n_rec + 1)), dim3(kBlock), 0, stream, (const uint32_t*)T.kid_s.p, (const uint32_t*)T.ord.p, (const uint32_t*)T.bin.p, n_rec,
                     n_kid, T.chead.p);
  S.scan(stream, T.chead.p, T.coff.p, (size_t)n_rec + 1);
  IMP_HIP_CHECK(hipMemsetAsync(S.d_extent.p, 0, (size_t)std::max<uint32_t>(n_kid, 1) * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_oidx_window_extent, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)T.kid_s.p, (const uint32_t*)T.ord.p, (const uint32_t*)T.w1.p, n_rec, n_kid,
                     S.d_extent.p);
  uint32_t err[kOErrWords], n_chunks = 0;
  uint64_t page_vend = 0;
  std::vector<uint32_t> extent(n_kid, 0u), win_off(n_kid, 0u);
  IMP_HIP_CHECK(hipMemcpyAsync(err, T.err.p, sizeof(err), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipMemcpyAsync(&n_chunks, T.coff.p + n_rec, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipMemcpyAsync(&page_vend, T.b.p + n_rec, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  if (n_kid) IMP_HIP_CHECK(hipMemcpyAsync(extent.data(), S.d_extent.p, (size_t)n_kid * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  uint32_t err_rec = UINT32_MAX, err_bit = 0;
  for (int k = 0; k < kOErrWords - 1; ++k) if ((err[0] & (1u << k)) && err[1 + k] < err_rec) { err_rec = err[1 + k]; err_bit = 1u << k; }
  if (err_bit) throw VCF2BinaryException(record_error(err_bit, S.header_lines + S.records_before + (int64_t)err_rec + 1, S.records_before + (int64_t)err_rec + 1, S.bcf));
  // ---- chunks
  T.cfirst.ensure(std::max<uint32_t>(n_chunks, 1)); T.chunks.ensure(std::max<uint32_t>(n_chunks, 1));
  std::vector<IdxChunk> chunks(n_chunks);
  if (n_chunks) {
    hipLaunchKernelGGL(k_oidx_chunk_firsts, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)T.chead.p, (const uint32_t*)T.coff.p, n_rec, n_chunks, T.cfirst.p);
    hipLaunchKernelGGL(k_oidx_chunks, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)T.cfirst.p, (const uint32_t*)T.chead.p, (const uint32_t*)T.coff.p,
                       (const uint32_t*)T.kid_s.p, (const uint32_t*)T.ord.p, (const uint32_t*)T.bin.p, (const uint64_t*)T.a.p, (const uint64_t*)T.b.p, n_rec, n_kid, n_chunks, T.chunks.p);
  }
  IMP_HIP_CHECK(hipEventRecord(S.ev[1], stream));
  if (n_chunks) IMP_HIP_CHECK(hipMemcpyAsync(chunks.data(), T.chunks.p, (size_t)n_chunks * sizeof(IdxChunk), hipMemcpyDeviceToHost, stream));
  // ---- linear: the minima of the page's windows
  uint64_t n_win = 0;
  for (uint32_t c = 0; c < n_kid; ++c) { win_off[c] = (uint32_t)n_win; n_win += extent[c]; }
  if (n_win >= ((uint64_t)1 << 31)) throw VCF2BinaryException("index: more than 2^31 windows of 16 kb in one page of the output stream");
  S.d_win.ensure(std::max<uint64_t>(n_win, 1));
  IMP_HIP_CHECK(hipEventRecord(S.ev[2], stream));
  if (n_kid) IMP_HIP_CHECK(hipMemcpyAsync(S.d_win_off.p, win_off.data(), (size_t)n_kid * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_win.p, 0xFF, (size_t)std::max<uint64_t>(n_win, 1) * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_oidx_windows, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)T.kid_s.p, (const uint32_t*)T.ord.p, (const uint64_t*)T.a.p, (const uint32_t*)T.w0.p,
                     (const uint32_t*)T.w1.p, n_rec, (const uint32_t*)S.d_win_off.p, n_kid, S.d_win.p, (uint32_t)n_win, S.d_tally.p);
  IMP_HIP_CHECK(hipEventRecord(S.ev[3], stream));
  std::vector<uint64_t> win((size_t)n_win);
  if (n_win) IMP_HIP_CHECK(hipMemcpyAsync(win.data(), S.d_win.p, (size_t)n_win * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  IMP_HIP_CHECK(hipGetLastError());
  float ms = 0;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, T.ev[0], T.ev[1])); st.ms_records += ms;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, T.ev[2], T.ev[3])); st.ms_voff += ms;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, S.ev[0], S.ev[1])); st.ms_chunks += ms;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, S.ev[2], S.ev[3])); st.ms_linear += ms;
  // ---- the page joins the ones before it
  const double t0 = now_s();
  S.merger.add_page(chunks.data(), chunks.size(), page_vend, win_off.data(), extent.data(), win.data(), compressed_bytes);
  st.s_write += now_s() - t0;
  ++st.pages;
  st.records += n_rec;
  S.records_before += n_rec;
  st.table_bytes = S.table_bytes();
}

void DeviceOutputIndexer::write(const std::string& path) {
  Impl& S = *m_;
  unsigned long long atomics = 0;
  if (S.tally_ready) {
    IMP_HIP_CHECK(hipSetDevice(S.device));
    IMP_HIP_CHECK(hipMemcpy(&atomics, S.d_tally.p, sizeof(atomics), hipMemcpyDeviceToHost));
  }
  st.atomics = (int64_t)atomics;
  const double t0 = now_s();
  const TbiBatchMerger& M = S.merger.merger;
  st.contigs = S.bcf ? (int64_t)S.n_kid : (int64_t)M.names.size();
  st.bins = (int64_t)M.num_bins(); st.chunks = (int64_t)M.num_chunks();
  S.merger.write(path);
  st.linear_windows = (int64_t)S.merger.merger.num_windows();
  st.s_write += now_s() - t0;
  st.table_bytes = S.table_bytes();
}

}  // namespace genomicsdb_amd
