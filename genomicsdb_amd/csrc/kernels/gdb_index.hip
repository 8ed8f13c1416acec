// gdb_index.hip - see gdb_index.h.  Kernels for gfx950 around the bodies of core/gdb_index.hpp, and their orchestration.
#include "gdb_index.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../core/gdb_index.hpp"
#include "../host/vcf_importer.h"
#include "../host/vcf_index.h"
#include "gdb_import_device.hpp"
#include "gdb_inflate.h"

namespace genomicsdb_amd {

namespace {
using namespace gdbimp;
using namespace gdbidx;
using namespace impdev;

struct IdxBatch { const char* text; const uint32_t* nl; const uint32_t* first_tab; const uint32_t* tab; uint32_t n_lines; };

// the whole line: a '\r' in front of the newline belongs to it, as for the host builder
__device__ __forceinline__ ImpLine idx_line_of(const IdxBatch& B, uint32_t line) {
  ImpLine L;
  L.text = B.text;
  L.begin = line ? B.nl[line - 1u] + 1u : 0u;
  L.end = B.nl[line];
  const uint32_t first = B.first_tab[line];
  L.tabs = B.tab + first;
  L.ntabs = B.first_tab[line + 1u] - first;
  return L;
}

// flag has n_lines + 1 entries, the last one 0 (the scan's total)
__global__ void __launch_bounds__(kBlock) k_idx_select(IdxBatch B, uint32_t* flag) {
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  if (line < B.n_lines) flag[line] = idx_is_record(idx_line_of(B, line)) ? 1u : 0u;
  else if (line == B.n_lines) flag[line] = 0u;
}

__global__ void __launch_bounds__(kBlock) k_idx_compact(const uint32_t* flag, const uint32_t* off, uint32_t n_lines, uint32_t* rec_line, uint32_t n_rec) {
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  if (line < n_lines && flag[line] && off[line] < n_rec) rec_line[off[line]] = line;
}

struct IdxRecOut { uint64_t* vbeg; uint64_t* vend; uint32_t* bin; uint32_t* w0; uint32_t* w1; uint32_t* head; };

// one thread per record; head has n_rec + 1 entries, the last one 0
__global__ void __launch_bounds__(kBlock) k_idx_records(IdxBatch B, IdxMembers M, uint64_t u_text, const uint32_t* rec_line, uint32_t n_rec, IdxRecOut O, uint32_t* err) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r == n_rec) O.head[r] = 0u;
  if (r >= n_rec) return;
  const uint32_t line = rec_line[r];
  const ImpLine L = idx_line_of(B, line);
  const IdxRec rec = idx_record(M, L, u_text, true);
  if (rec.err) imp_raise(err, rec.err, line);
  O.vbeg[r] = rec.vbeg; O.vend[r] = rec.vend; O.bin[r] = rec.bin; O.w0[r] = rec.w0; O.w1[r] = rec.w1;
  O.head[r] = (r == 0u || !idx_same_chrom(L, idx_line_of(B, rec_line[r - 1u]))) ? 1u : 0u;
}

// the run heads' names: where they are, how long (name_len has n_runs + 1 entries, the last one 0)
__global__ void __launch_bounds__(kBlock) k_idx_head_lens(IdxBatch B, const uint32_t* rec_line, const uint32_t* head, const uint32_t* hoff, uint32_t n_rec, uint32_t n_runs,
                                                         uint32_t* name_at, uint32_t* name_len) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r == 0u) name_len[n_runs] = 0u;
  if (r >= n_rec || !head[r] || hoff[r] >= n_runs) return;
  const ImpLine L = idx_line_of(B, rec_line[r]);
  name_at[hoff[r]] = L.begin;
  name_len[hoff[r]] = L.tabs[0] - L.begin;
}
__global__ void __launch_bounds__(kBlock) k_idx_head_names(const char* text, const uint32_t* name_at, const uint32_t* name_len, const uint32_t* name_off, uint32_t n_runs,
                                                          char* names, uint32_t names_bytes) {
  const uint32_t run = blockIdx.x * kBlock + threadIdx.x;
  if (run >= n_runs) return;
  const uint32_t at = name_at[run], n = name_len[run], to = name_off[run];
  if ((uint64_t)to + n > names_bytes) return;      // (never, by the scan)
  for (uint32_t i = 0; i < n; ++i) names[to + i] = text[at + i];
}

// contig id of every record (its run's), and the record's own number as the value the sort carries
__global__ void __launch_bounds__(kBlock) k_idx_keys(const uint32_t* head, const uint32_t* hoff, const uint32_t* run_tid, uint32_t n_rec, uint32_t n_runs, uint32_t* tid,
                                                    uint32_t* rec) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const uint32_t run = hoff[r] + head[r] - 1u;      // (head[0] = 1: never below 0)
  tid[r] = run < n_runs ? run_tid[run] : 0u;
  rec[r] = r;
}

// records in contig order (tid_s ascending, file order inside a contig; ord: the record): chead has n_rec + 1 entries, the last one 0
__global__ void __launch_bounds__(kBlock) k_idx_chunk_heads(const uint32_t* tid_s, const uint32_t* ord, const uint32_t* bin, uint32_t n_rec, uint32_t* chead) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == n_rec) chead[i] = 0u;
  if (i >= n_rec) return;
  const uint32_t p = i ? i - 1u : 0u;
  chead[i] = idx_chunk_head(i == 0u, tid_s[i], bin[ord[i]], tid_s[p], bin[ord[p]]) ? 1u : 0u;
}
// where every chunk begins in the contig order; cfirst has n_chunks + 1 entries, the last one n_rec
__global__ void __launch_bounds__(kBlock) k_idx_chunk_firsts(const uint32_t* chead, const uint32_t* coff, uint32_t n_rec, uint32_t n_chunks, uint32_t* cfirst) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0u) cfirst[n_chunks] = n_rec;
  if (i < n_rec && chead[i] && coff[i] < n_chunks) cfirst[coff[i]] = i;
}
// one thread per chunk: vbeg of its first record, vend of its last, and the key (contig id, bin) of the chunks' sort
__global__ void __launch_bounds__(kBlock) k_idx_chunks(const uint32_t* cfirst, const uint32_t* tid_s, const uint32_t* ord, const uint32_t* bin, const uint64_t* vbeg,
                                                      const uint64_t* vend, uint32_t n_rec, uint32_t n_chunks, IdxChunk* chunks, uint64_t* key) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_chunks) return;
  const uint32_t i0 = cfirst[c], i1 = cfirst[c + 1u];
  if (i0 >= i1 || i1 > n_rec) return;      // (never, by the scan)
  IdxChunk k;
  k.tid = tid_s[i0]; k.bin = bin[ord[i0]];
  k.beg = vbeg[ord[i0]]; k.end = vend[ord[i1 - 1u]];
  k.count = i1 - i0;
  k.flags = ((i0 == 0u || tid_s[i0 - 1u] != k.tid) ? IDX_CHUNK_FIRST : 0u) | ((i1 == n_rec || tid_s[i1] != k.tid) ? IDX_CHUNK_LAST : 0u);
  chunks[c] = k;
  key[c] = ((uint64_t)k.tid << 32) | k.bin;
}

// 1 + the largest window per contig of the batch.  w1 mostly grows inside a contig: a lane whose neighbour in front is of the same
// contig and reaches at least as far issues nothing
__global__ void __launch_bounds__(kBlock) k_idx_window_extent(const uint32_t* tid_s, const uint32_t* ord, const uint32_t* w1, uint32_t n_rec, uint32_t n_contigs, uint32_t* extent) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < n_rec;
  const uint32_t tid = valid ? tid_s[i] : UINT32_MAX, mine = valid ? w1[ord[i]] : 0u;
  const uint32_t ptid = (uint32_t)__shfl_up((int)tid, 1, 64), pw = (uint32_t)__shfl_up((int)mine, 1, 64);
  const bool covered = (threadIdx.x & 63u) != 0u && ptid == tid && pw >= mine;
  if (valid && !covered && tid < n_contigs) atomicMax(&extent[tid], mine + 1u);
}

// One thread per record, in contig order: hundreds of neighbours share a 16 kb window, and a reference block covers hundreds of
// windows.  The lane loops over its windows and issues the 64-bit atomicMin only where the lane in front does not cover the window
// too (idx_window_mine): per (contig, window) one atomic per wavefront instead of one per record.  tally[0]: atomics issued
__global__ void __launch_bounds__(kBlock) k_idx_windows(const uint32_t* tid_s, const uint32_t* ord, const uint64_t* vbeg, const uint32_t* w0, const uint32_t* w1, uint32_t n_rec,
                                                       const uint32_t* win_off, uint32_t n_contigs, unsigned long long* win, uint32_t n_win, unsigned long long* tally) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool valid = i < n_rec;
  uint32_t tid = UINT32_MAX, a = 1u, b = 0u;
  uint64_t vb = 0;
  if (valid) { const uint32_t r = ord[i]; tid = tid_s[i]; a = w0[r]; b = w1[r]; vb = vbeg[r]; }
  const uint32_t ptid = (uint32_t)__shfl_up((int)tid, 1, 64), pa = (uint32_t)__shfl_up((int)a, 1, 64), pb = (uint32_t)__shfl_up((int)b, 1, 64);
  const uint64_t pvb = __shfl_up(vb, 1, 64);
  uint32_t issued = 0;
  if (valid && vb != 0u && tid < n_contigs) {
    const uint32_t base = win_off[tid];
    for (uint32_t w = a; w <= b; ++w) {
      if (!idx_window_mine(lane != 0u, tid, w, ptid, pa, pb, pvb)) continue;
      const uint64_t at = (uint64_t)base + w;
      if (at < n_win) { atomicMin(&win[at], (unsigned long long)vb); ++issued; }      // (always inside: the extent pass sized it)
    }
  }
  for (int d = 32; d; d >>= 1) issued += (uint32_t)__shfl_xor((int)issued, d, 64);
  if (lane == 0u && issued) atomicAdd(&tally[0], (unsigned long long)issued);
}

std::string bad_member(const std::string& path, uint64_t offset, const std::string& why) {
  return "corrupt BGZF member at byte offset " + std::to_string(offset) + " of " + path + ": " + why;
}

}  // namespace

struct DeviceTbiBuilder::Impl {
  std::string path;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  TbiBatchMerger merger;
  int64_t lines_before = 0;
  IdxMembers M{nullptr, nullptr, 0, 0, 0};
  DBuf<uint64_t> d_members;                                  // ubase, then coff
  DBuf<uint64_t> d_tile, d_tile_scan, d_vbeg, d_vend, d_key, d_key_s;
  DBuf<char> d_tmp, d_names;
  DBuf<uint32_t> d_nl, d_first_tab, d_tab, d_flag, d_off, d_rec_line, d_bin, d_w0, d_w1, d_head, d_hoff, d_name_at, d_name_len, d_name_off, d_run_tid, d_tid, d_rec,
      d_tid_s, d_ord, d_chead, d_coff, d_cfirst, d_extent, d_win_off, d_err;
  DBuf<IdxChunk> d_chunks, d_chunks_s;
  DBuf<unsigned long long> d_win, d_tally;

  template <class T> void scan(const T* in, T* out, size_t n) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::exclusive_scan((void*)d_tmp.p, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
  }
  template <class K, class V> void sort_pairs(const K* k_in, K* k_out, const V* v_in, V* v_out, size_t n, unsigned bits) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::radix_sort_pairs((void*)d_tmp.p, bytes, k_in, k_out, v_in, v_out, n, 0u, bits, stream));
  }
  uint32_t fetch(const uint32_t* d) {
    uint32_t v = 0;
    IMP_HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    return v;
  }
  double span(int a, int b) { float ms = 0; IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[a], ev[b])); return ms; }
};

DeviceTbiBuilder::DeviceTbiBuilder(const std::string& path_for_messages, void* stream) : m_(new Impl) {
  m_->path = path_for_messages;
  m_->stream = (hipStream_t)stream;
  try {
    for (auto& e : m_->ev) IMP_HIP_CHECK(hipEventCreate(&e));
    m_->d_err.ensure(kErrWords);
    m_->d_tally.ensure(1);
    IMP_HIP_CHECK(hipMemsetAsync(m_->d_tally.p, 0, sizeof(unsigned long long), m_->stream));
    IMP_HIP_CHECK(hipStreamSynchronize(m_->stream));
  } catch (...) { for (auto& e : m_->ev) if (e) (void)hipEventDestroy(e); delete m_; throw; }
}
DeviceTbiBuilder::~DeviceTbiBuilder() {
  (void)hipStreamSynchronize(m_->stream);
  for (auto& e : m_->ev) if (e) (void)hipEventDestroy(e);
  delete m_;
}

void DeviceTbiBuilder::reset(const std::string& path_for_messages, int64_t lines_before) {
  Impl& S = *m_;
  S.path = path_for_messages;
  S.merger = TbiBatchMerger();
  S.lines_before = lines_before;
  st = IndexStats();
  IMP_HIP_CHECK(hipMemsetAsync(S.d_tally.p, 0, sizeof(unsigned long long), S.stream));
  IMP_HIP_CHECK(hipStreamSynchronize(S.stream));
}

void DeviceTbiBuilder::set_members(const IndexMemberTable& t) {
  Impl& S = *m_;
  const size_t n = t.ubase.size();
  if (t.coff.size() != n || n >= ((size_t)1 << 31)) throw GenomicsDBDeviceException("index: bad member table");
  S.d_members.ensure(std::max<size_t>(2 * n, 1));
  if (n) {
    IMP_HIP_CHECK(hipMemcpyAsync(S.d_members.p, t.ubase.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, S.stream));
    IMP_HIP_CHECK(hipMemcpyAsync(S.d_members.p + n, t.coff.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, S.stream));
    IMP_HIP_CHECK(hipStreamSynchronize(S.stream));
  }
  S.M = IdxMembers{S.d_members.p, S.d_members.p + n, (uint32_t)n, t.total, t.v_total};
}
void DeviceTbiBuilder::resolve_pending(uint64_t voff) { m_->merger.resolve_pending(voff); }

uint32_t DeviceTbiBuilder::add_batch(const char* d_text, uint32_t n, uint64_t u_text) {
  Impl& S = *m_;
  const hipStream_t stream = S.stream;
  if (!n) return 0;
  if (S.merger.pending_tid >= 0) throw GenomicsDBDeviceException("index: a batch while the offset behind the last one is not known");
  // ---- lines
  IMP_HIP_CHECK(hipEventRecord(S.ev[0], stream));
  uint32_t n_lines = 0, n_tabs = 0;
  index_lines(d_text, n, S.d_tile, S.d_tile_scan, S.d_tmp, S.d_nl, S.d_first_tab, S.d_tab, stream, &n_lines, &n_tabs);
  IMP_HIP_CHECK(hipEventRecord(S.ev[1], stream));
  if (n_lines == 0) { IMP_HIP_CHECK(hipStreamSynchronize(stream)); return 0; }      // a piece of one line: the caller brings more
  const uint32_t used = S.fetch(S.d_nl.p + (n_lines - 1u)) + 1u;      // behind the last newline
  ++st.batches;
  st.text_bytes += used;
  const IdxBatch B{d_text, S.d_nl.p, S.d_first_tab.p, S.d_tab.p, n_lines};
  const int64_t lines_before = S.lines_before;
  S.lines_before += n_lines;
  st.lines += n_lines;
  // ---- select and compact
  S.d_flag.ensure((size_t)n_lines + 1); S.d_off.ensure((size_t)n_lines + 1);
  IMP_HIP_CHECK(hipEventRecord(S.ev[2], stream));
  hipLaunchKernelGGL(k_idx_select, dim3(grid_for((uint64_t)n_lines + 1)), dim3(kBlock), 0, stream, B, S.d_flag.p);
  S.scan<uint32_t>(S.d_flag.p, S.d_off.p, (size_t)n_lines + 1);
  const uint32_t n_rec = S.fetch(S.d_off.p + n_lines);
  if (n_rec == 0) {
    IMP_HIP_CHECK(hipEventRecord(S.ev[3], stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    st.ms_index += S.span(0, 1); st.ms_records += S.span(2, 3);
    return used;
  }
  st.records += n_rec;
  S.d_rec_line.ensure(n_rec); S.d_vbeg.ensure(n_rec); S.d_vend.ensure(n_rec); S.d_bin.ensure(n_rec); S.d_w0.ensure(n_rec); S.d_w1.ensure(n_rec);
  S.d_head.ensure((size_t)n_rec + 1); S.d_hoff.ensure((size_t)n_rec + 1);
  hipLaunchKernelGGL(k_idx_compact, dim3(grid_for(n_lines)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_flag.p, (const uint32_t*)S.d_off.p, n_lines, S.d_rec_line.p, n_rec);
  // ---- records: interval, bin, windows, virtual offsets, run heads
  IMP_HIP_CHECK(hipMemsetAsync(S.d_err.p, 0, sizeof(uint32_t), stream));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_err.p + 1, 0xFF, (kErrWords - 1) * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_idx_records, dim3(grid_for((uint64_t)n_rec + 1)), dim3(kBlock), 0, stream, B, S.M, u_text, (const uint32_t*)S.d_rec_line.p, n_rec,
                     IdxRecOut{S.d_vbeg.p, S.d_vend.p, S.d_bin.p, S.d_w0.p, S.d_w1.p, S.d_head.p}, S.d_err.p);
  S.scan<uint32_t>(S.d_head.p, S.d_hoff.p, (size_t)n_rec + 1);
  uint32_t err[kErrWords];
  IMP_HIP_CHECK(hipMemcpyAsync(err, S.d_err.p, sizeof(err), hipMemcpyDeviceToHost, stream));
  const uint32_t n_runs = S.fetch(S.d_hoff.p + n_rec);
  uint32_t err_line = UINT32_MAX, err_bit = 0;
  for (int k = 0; k < kErrWords - 1; ++k) if ((err[0] & (1u << k)) && err[1 + k] < err_line) { err_line = err[1 + k]; err_bit = 1u << k; }
  if (err_bit) throw VCF2BinaryException(tbi_record_error(err_bit, S.path, lines_before + (int64_t)err_line + 1));
  // ---- the run heads' names -> contig ids
  S.d_name_at.ensure(n_runs); S.d_name_len.ensure((size_t)n_runs + 1); S.d_name_off.ensure((size_t)n_runs + 1); S.d_run_tid.ensure(n_runs);
  hipLaunchKernelGGL(k_idx_head_lens, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, B, (const uint32_t*)S.d_rec_line.p, (const uint32_t*)S.d_head.p, (const uint32_t*)S.d_hoff.p,
                     n_rec, n_runs, S.d_name_at.p, S.d_name_len.p);
  S.scan<uint32_t>(S.d_name_len.p, S.d_name_off.p, (size_t)n_runs + 1);
  std::vector<uint32_t> name_off((size_t)n_runs + 1);
  IMP_HIP_CHECK(hipMemcpyAsync(name_off.data(), S.d_name_off.p, name_off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  const uint32_t names_bytes = name_off[n_runs];
  S.d_names.ensure(std::max<uint32_t>(names_bytes, 1));
  hipLaunchKernelGGL(k_idx_head_names, dim3(grid_for(n_runs)), dim3(kBlock), 0, stream, d_text, (const uint32_t*)S.d_name_at.p, (const uint32_t*)S.d_name_len.p,
                     (const uint32_t*)S.d_name_off.p, n_runs, S.d_names.p, names_bytes);
  IMP_HIP_CHECK(hipEventRecord(S.ev[3], stream));
  std::string names(names_bytes, '\0');
  if (names_bytes) IMP_HIP_CHECK(hipMemcpyAsync(&names[0], S.d_names.p, names_bytes, hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  std::vector<uint32_t> run_tid(n_runs);
  for (uint32_t r = 0; r < n_runs; ++r) run_tid[r] = S.merger.id_of(names.substr(name_off[r], name_off[r + 1] - name_off[r]));
  const uint32_t n_contigs = (uint32_t)S.merger.names.size();
  unsigned tid_bits = 1;
  while (tid_bits < 32u && (n_contigs >> tid_bits) != 0u) ++tid_bits;
  // ---- chunks: contig order, heads, the chunks sorted by (contig id, bin)
  S.d_tid.ensure(n_rec); S.d_rec.ensure(n_rec); S.d_tid_s.ensure(n_rec); S.d_ord.ensure(n_rec); S.d_chead.ensure((size_t)n_rec + 1); S.d_coff.ensure((size_t)n_rec + 1);
  IMP_HIP_CHECK(hipMemcpyAsync(S.d_run_tid.p, run_tid.data(), (size_t)n_runs * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  IMP_HIP_CHECK(hipEventRecord(S.ev[4], stream));
  hipLaunchKernelGGL(k_idx_keys, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_head.p, (const uint32_t*)S.d_hoff.p, (const uint32_t*)S.d_run_tid.p, n_rec,
                     n_runs, S.d_tid.p, S.d_rec.p);
  S.sort_pairs<uint32_t, uint32_t>(S.d_tid.p, S.d_tid_s.p, S.d_rec.p, S.d_ord.p, n_rec, tid_bits);
  hipLaunchKernelGGL(k_idx_chunk_heads, dim3(grid_for((uint64_t)n_rec + 1)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_tid_s.p, (const uint32_t*)S.d_ord.p,
                     (const uint32_t*)S.d_bin.p, n_rec, S.d_chead.p);
  S.scan<uint32_t>(S.d_chead.p, S.d_coff.p, (size_t)n_rec + 1);
  const uint32_t n_chunks = S.fetch(S.d_coff.p + n_rec);
  S.d_cfirst.ensure((size_t)n_chunks + 1); S.d_chunks.ensure(n_chunks); S.d_chunks_s.ensure(n_chunks); S.d_key.ensure(n_chunks); S.d_key_s.ensure(n_chunks);
  hipLaunchKernelGGL(k_idx_chunk_firsts, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_chead.p, (const uint32_t*)S.d_coff.p, n_rec, n_chunks, S.d_cfirst.p);
  hipLaunchKernelGGL(k_idx_chunks, dim3(grid_for(n_chunks)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_cfirst.p, (const uint32_t*)S.d_tid_s.p, (const uint32_t*)S.d_ord.p,
                     (const uint32_t*)S.d_bin.p, (const uint64_t*)S.d_vbeg.p, (const uint64_t*)S.d_vend.p, n_rec, n_chunks, S.d_chunks.p, S.d_key.p);
  S.sort_pairs<uint64_t, IdxChunk>(S.d_key.p, S.d_key_s.p, S.d_chunks.p, S.d_chunks_s.p, n_chunks, 32u + tid_bits);
  IMP_HIP_CHECK(hipEventRecord(S.ev[5], stream));
  std::vector<IdxChunk> chunks(n_chunks);
  IMP_HIP_CHECK(hipMemcpyAsync(chunks.data(), S.d_chunks_s.p, (size_t)n_chunks * sizeof(IdxChunk), hipMemcpyDeviceToHost, stream));
  // ---- linear: the extent per contig, then the minima
  S.d_extent.ensure(n_contigs); S.d_win_off.ensure(n_contigs);
  IMP_HIP_CHECK(hipEventRecord(S.ev[6], stream));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_extent.p, 0, (size_t)n_contigs * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_idx_window_extent, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_tid_s.p, (const uint32_t*)S.d_ord.p, (const uint32_t*)S.d_w1.p, n_rec,
                     n_contigs, S.d_extent.p);
  std::vector<uint32_t> extent(n_contigs), win_off(n_contigs);
  IMP_HIP_CHECK(hipMemcpyAsync(extent.data(), S.d_extent.p, (size_t)n_contigs * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  uint64_t n_win = 0;
  for (uint32_t c = 0; c < n_contigs; ++c) { win_off[c] = (uint32_t)n_win; n_win += extent[c]; }
  if (n_win >= ((uint64_t)1 << 31)) throw VCF2BinaryException("index: more than 2^31 windows of 16 kb in one batch of " + S.path);
  S.d_win.ensure(std::max<uint64_t>(n_win, 1));
  IMP_HIP_CHECK(hipMemcpyAsync(S.d_win_off.p, win_off.data(), (size_t)n_contigs * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_win.p, 0xFF, (size_t)n_win * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_idx_windows, dim3(grid_for(n_rec)), dim3(kBlock), 0, stream, (const uint32_t*)S.d_tid_s.p, (const uint32_t*)S.d_ord.p, (const uint64_t*)S.d_vbeg.p,
                     (const uint32_t*)S.d_w0.p, (const uint32_t*)S.d_w1.p, n_rec, (const uint32_t*)S.d_win_off.p, n_contigs, S.d_win.p, (uint32_t)n_win, S.d_tally.p);
  IMP_HIP_CHECK(hipEventRecord(S.ev[7], stream));
  std::vector<uint64_t> win((size_t)n_win);
  if (n_win) IMP_HIP_CHECK(hipMemcpyAsync(win.data(), S.d_win.p, (size_t)n_win * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  IMP_HIP_CHECK(hipStreamSynchronize(stream));
  IMP_HIP_CHECK(hipGetLastError());
  st.ms_index += S.span(0, 1); st.ms_records += S.span(2, 3); st.ms_chunks += S.span(4, 5); st.ms_linear += S.span(6, 7);
  // ---- the batch joins the ones before it
  const double t0 = now_s();
  S.merger.add_chunks(chunks.data(), chunks.size());
  for (uint32_t c = 0; c < n_contigs; ++c) if (extent[c]) S.merger.add_windows(c, win.data() + win_off[c], extent[c]);
  st.s_serialize_write += now_s() - t0;
  return used;
}

void DeviceTbiBuilder::finish(const std::string& tbi_path) {
  Impl& S = *m_;
  if (S.merger.pending_tid >= 0) throw GenomicsDBDeviceException("index: the offset behind the last batch is not known");
  unsigned long long atomics = 0;
  IMP_HIP_CHECK(hipMemcpyAsync(&atomics, S.d_tally.p, sizeof(atomics), hipMemcpyDeviceToHost, S.stream));
  IMP_HIP_CHECK(hipStreamSynchronize(S.stream));
  st.atomics = (int64_t)atomics;
  const double t0 = now_s();
  st.contigs = (int64_t)S.merger.names.size(); st.bins = (int64_t)S.merger.num_bins(); st.chunks = (int64_t)S.merger.num_chunks();
  S.merger.write(tbi_path);
  st.linear_windows = (int64_t)S.merger.num_windows();
  st.s_serialize_write += now_s() - t0;
}

std::string index_vcf_device(const std::string& path, int device, uint64_t text_budget_bytes, IndexStats* stats) {
  const double t0 = now_s();
  // ---- the file, as it is; the refusals that need no device
  std::string raw;
  {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw VCF2BinaryException("index: cannot open " + path);
    in.seekg(0, std::ios::end);
    const std::streamoff size = in.tellg();
    in.seekg(0, std::ios::beg);
    raw.resize(size > 0 ? (size_t)size : 0);
    if (!raw.empty() && !in.read(&raw[0], (std::streamsize)raw.size())) throw VCF2BinaryException("index: cannot read " + path);
  }
  std::vector<BgzfMember> mem;
  uint64_t total = 0, break_at = 0;
  if (!bgzf_walk((const uint8_t*)raw.data(), raw.size(), mem, &total, &break_at))
    throw VCF2BinaryException("index: " + path + " is not a BGZF file from its first byte to its last: the chain breaks at byte offset " + std::to_string(break_at));
  const double s_read = now_s() - t0;
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the device index builder has no CPU fallback (gdbamd_build_output_index is the host builder)");
  IMP_HIP_CHECK(hipSetDevice(device));
  uint64_t budget = text_budget_bytes ? text_budget_bytes : ((uint64_t)64 << 20);
  budget = std::min<uint64_t>(budget, (uint64_t)1 << 30);
  IndexMemberTable table;
  for (const BgzfMember& m : mem) if (m.isize) { table.ubase.push_back(m.out_off); table.coff.push_back(m.offset); }
  table.total = total; table.v_total = (uint64_t)raw.size() << 16;

  const std::string tbi = path + ".tbi", tmp = tbi + ".tmp";
  hipStream_t stream = nullptr;
  IMP_HIP_CHECK(hipStreamCreate(&stream));
  IndexStats st;
  try {
    DeviceTbiBuilder builder(path, (void*)stream);
    builder.set_members(table);
    BgzfDeviceInflater inflater;
    DBuf<char> d_win[2];
    int cur = 0;
    uint64_t carry = 0, u_done = 0;      // bytes of a partial line at the front of the window; uncompressed position of the window's first byte
    size_t k = 0;
    while (k < mem.size()) {
      // ---- a window: [the partial line carried over | whole members of about one budget, one at least]
      size_t k2 = k;
      uint64_t w_bytes = 0;
      const uint64_t room = budget > carry ? budget - carry : 0;
      while (k2 < mem.size() && (k2 == k || w_bytes + mem[k2].isize <= room)) w_bytes += mem[k2++].isize;
      const bool last = k2 == mem.size();
      uint64_t wend = carry + w_bytes;
      if (wend + 1 >= ((uint64_t)1 << 31)) throw VCF2BinaryException("a line of 2 GiB or more in " + path);
      if (d_win[cur].cap < wend + 1 + kTextPad) {      // grows, and keeps the carried bytes
        d_win[1 - cur].ensure((size_t)wend + 1 + kTextPad);
        if (carry) IMP_HIP_CHECK(hipMemcpyAsync(d_win[1 - cur].p, d_win[cur].p, (size_t)carry, hipMemcpyDeviceToDevice, stream));
        cur = 1 - cur;
      }
      char* win = d_win[cur].p;
      uint32_t err = 0;
      const int64_t bad = inflater.inflate((const uint8_t*)raw.data(), mem.data(), k, k2, (uint8_t*)win + carry, (void*)stream, &err);
      if (bad >= 0) throw VCF2BinaryException(bad_member(path, mem[(size_t)bad].offset, bgzf_inflate_error_text(err)));
      k = k2;
      if (!wend) continue;
      // ---- the whole lines of the window are the batch; a last line without a newline is a line
      if (last) {
        char last_byte = '\n';
        IMP_HIP_CHECK(hipMemcpyAsync(&last_byte, win + wend - 1, 1, hipMemcpyDeviceToHost, stream));
        IMP_HIP_CHECK(hipStreamSynchronize(stream));
        if (last_byte != '\n') { IMP_HIP_CHECK(hipMemsetAsync(win + wend, '\n', 1, stream)); ++wend; }
      }
      const uint64_t used = builder.add_batch(win, (uint32_t)wend, u_done);
      u_done += used;
      carry = wend - used;
      if (carry && used && !last) {      // the partial line moves to the front of the next window
        d_win[1 - cur].ensure(std::max((size_t)carry + 1 + kTextPad, d_win[cur].cap));
        IMP_HIP_CHECK(hipMemcpyAsync(d_win[1 - cur].p, win + used, (size_t)carry, hipMemcpyDeviceToDevice, stream));
        IMP_HIP_CHECK(hipStreamSynchronize(stream));
        cur = 1 - cur;
      }
    }
    builder.st.members = (int64_t)mem.size();
    builder.st.ms_inflate = inflater.ms_kernel;
    builder.finish(tmp);
    if (rename(tmp.c_str(), tbi.c_str()) != 0) throw VCF2BinaryException("index: cannot rename " + tmp + " to " + tbi);
    st = builder.st;
  } catch (...) {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
    (void)remove(tmp.c_str());
    throw;
  }
  (void)hipStreamDestroy(stream);
  st.s_read = s_read;
  st.s_total = now_s() - t0;
  if (stats) *stats = st;
  return tbi;
}

}  // namespace genomicsdb_amd
