// gdb_import_stream.hip - see gdb_import_stream.h.  Kernels for gfx950 around the bodies of core/gdb_import_stream.hpp, and the
// batch-by-batch orchestration on top of the device importer's batches (kernels/gdb_import_impl.hpp).
//
// Per write of a stream: the device importer's own batch (index, k_imp_measure, scan, k_imp_write, deferred tokens), then
//   order    k_str_order: one thread per record compares its column with the record before it (for the first record: the stream's
//            last column of the write before) -> the smallest offending record, and the stream's new last column
// and the batch's slots (key, size, tag, source pointer) are appended to the pending slots; its cell bytes stay where they are.
// Per import_batch, once every buffer is converted and W is known (all launches on one stream):
//   classify k_str_classify: one thread per pending slot: emit, keep or drop; emit keys, keep flags and pool bytes for the scans
//   emit     stable rocPRIM radix sort of the emit keys (pending slots are in append order per stream, and equal (column, row) keys
//            only come from one stream, so ties resolve as the single sort of DeviceImporter::finish() does), then finish()'s
//            k_imp_sorted_sizes, scan and k_imp_gather, one copy to the host
//   compact  scans of the keep flags and of the kept cells' 16-byte aligned sizes, k_str_compact: one wavefront per kept cell moves
//            its bytes to the front of the OTHER pool and its slot to the other slot arrays; pools and arrays ping-pong, nothing
//            moves in place.  The write batches' cell buffers are freed; pools grow geometrically and stay until finish().
#include "gdb_import_stream.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>

#include "../core/gdb_import_stream.hpp"
#include "gdb_import_impl.hpp"

namespace genomicsdb_amd {

namespace {
using namespace gdbstr;
using namespace impdev;

// out[0]: smallest error word (kNoError: none), out[1]: column of the write's last record
__global__ void __launch_bounds__(kBlock) k_str_order(const int64_t* col, uint32_t per_line, uint32_t n_rec, int64_t last_before, const char* text, const uint32_t* nl_pos,
                                                     unsigned long long* out) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rec) return;
  const bool is_record = nl_pos ? str_text_line_is_record(text, nl_pos, r) : true;
  const uint64_t w = str_order_check(col, per_line, r, last_before, is_record);
  if (w != kNoError) atomicMin(&out[0], (unsigned long long)w);
  if (r == n_rec - 1u) out[1] = (unsigned long long)col[(uint64_t)r * per_line];
}

// counters: [0] emitted, [1] kept, [2] emitted partition-begin cells, [3] pool bytes of the kept
__global__ void __launch_bounds__(kBlock) k_str_classify(const uint64_t* key, const uint64_t* tag, const uint32_t* size, uint64_t n, int32_t key_row_bits, int64_t max_row,
                                                        const unsigned long long* row_best, int64_t W, int64_t column_begin, uint8_t* cls, uint64_t* emit_key,
                                                        uint64_t* keep_flag, uint64_t* keep_bytes, unsigned long long* counters) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t c = STR_DROP;
  bool spanning = false;
  uint64_t bytes = 0;
  if (i < n) {
    const uint64_t t = tag ? tag[i] : 0u;
    c = str_classify(key[i], t, key_row_bits, max_row, row_best, W, column_begin);
    spanning = c == STR_EMIT && t != 0u;
    bytes = c == STR_KEEP ? str_pool_bytes(size[i]) : 0u;
    cls[i] = (uint8_t)c;
    emit_key[i] = c == STR_EMIT ? key[i] : kNoCell;
    keep_flag[i] = c == STR_KEEP ? 1u : 0u;
    keep_bytes[i] = bytes;
  }
  const unsigned long long e = __ballot(c == STR_EMIT), k = __ballot(c == STR_KEEP), s = __ballot(spanning);
  unsigned long long wave_bytes = bytes;      // one atomic per wavefront and counter
  for (int d = 32; d > 0; d >>= 1) wave_bytes += __shfl_down(wave_bytes, d);
  if ((threadIdx.x & 63u) == 0u) {
    if (e) atomicAdd(&counters[0], (unsigned long long)__popcll(e));
    if (k) atomicAdd(&counters[1], (unsigned long long)__popcll(k));
    if (s) atomicAdd(&counters[2], (unsigned long long)__popcll(s));
    if (wave_bytes) atomicAdd(&counters[3], wave_bytes);
  }
}

// one wavefront per pending slot; a kept one moves to slot dst[] of the other arrays and to byte doff[] of the other pool.
// The pool is 16-byte aligned and so is every doff: a source that is aligned too (a cell that already sat in a pool) moves in 16-byte
// words, a cell of a write batch (packed, any alignment) byte by byte.
__global__ void __launch_bounds__(kBlock) k_str_compact(const uint8_t* cls, const uint64_t* dst, const uint64_t* doff, uint64_t n, const uint64_t* key, const uint32_t* size,
                                                       const uint64_t* tag, const uint64_t* src, uint64_t* key2, uint32_t* size2, uint64_t* tag2, uint64_t* src2,
                                                       uint8_t* pool, uint64_t pool_bytes, uint64_t n_keep) {
  const uint64_t slot = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (slot >= n || cls[slot] != STR_KEEP) return;
  const uint32_t lane = threadIdx.x & 63u, bytes = size[slot];
  const uint64_t j = dst[slot], at = doff[slot];
  const uint8_t* from = reinterpret_cast<const uint8_t*>((uintptr_t)src[slot]);
  if (j >= n_keep || !from || at + str_pool_bytes(bytes) > pool_bytes) return;      // (never, by the scans: nothing is stored outside the arrays and the pool)
  uint8_t* to = pool + at;
  if (lane == 0u) { key2[j] = key[slot]; size2[j] = bytes; if (tag2) tag2[j] = tag[slot]; src2[j] = (uint64_t)(uintptr_t)to; }
  uint32_t done = 0;
  if (((uintptr_t)from & 15u) == 0u) {
    const uint32_t words = bytes >> 4;
    for (uint32_t w = lane; w < words; w += 64u) reinterpret_cast<uint4*>(to)[w] = reinterpret_cast<const uint4*>(from)[w];
    done = words << 4;
  }
  for (uint32_t i = done + lane; i < bytes; i += 64u) to[i] = from[i];
}

template <class T> void grow_keep(DBuf<T>& b, size_t need, size_t have, hipStream_t s) {      // grows geometrically and keeps the first `have` elements
  if (need <= b.cap) return;
  const size_t cap = std::max(need, 2 * b.cap);
  T* p = nullptr;
  IMP_HIP_CHECK(hipMalloc((void**)&p, cap * sizeof(T)));
  if (have && b.p) {
    hipError_t e = hipMemcpyAsync(p, b.p, have * sizeof(T), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(p); IMP_HIP_CHECK(e); }
  }
  if (b.p) (void)hipFree(b.p);
  b.p = p; b.cap = cap;
}
template <class T> void grow_drop(DBuf<T>& b, size_t need) { if (need > b.cap) b.ensure(std::max(need, 2 * b.cap)); }      // the content is not needed
}  // namespace

struct DeviceStreamImporter::Impl {
  struct Stream {
    BufferStreamDecl decl;
    int64_t file_idx = -1;
    bool used = false, ended = false, reported = true;      // reported: exhausted by the last batch (every used stream before the first one)
    ImportFile file;
    ImportHeader text_hdr; BcfHeaderHost bcf_hdr;
    std::vector<uint8_t> buf;
    int64_t last = kColNegInf;
    uint64_t records = 0, bytes_before = 0;      // records and bytes of the stream in front of buf
    int64_t lines_before = 0;
  };
  struct Slots { DBuf<uint64_t> key, src, tag; DBuf<uint32_t> size; };
  DeviceImporter imp;
  std::vector<Stream> streams;
  std::vector<int64_t> file_idx;
  std::vector<std::pair<int64_t, int>> exhausted;
  size_t n_used = 0;
  StreamImportStats st;
  bool failed = false, finished = false;
  Stream* cur = nullptr;                  // the stream whose write is being converted
  Slots slots[2]; int cur_slots = 0;
  DBuf<uint8_t> pool[2];                  // kept cells; pool[cur_slots] holds those of the pending slots that are not in a write batch
  uint64_t n_pending = 0, pending_bytes = 0;      // slots / bytes held (pool bytes of the carried + cell bytes of the new batches)
  int64_t pending_cells = 0;
  std::vector<uint8_t*> batch_cells;      // cell buffers of the write batches since the last compaction
  DBuf<unsigned long long> d_order, d_counters;
  DBuf<uint8_t> d_cls, d_out;
  DBuf<uint64_t> d_emit_key, d_key_sorted, d_keep_flag, d_keep_bytes, d_dst, d_doff, d_sorted_size, d_sorted_off;
  DBuf<uint32_t> d_idx, d_idx_sorted;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

  Impl(int device, const VidMapper& vid, const ImportOptions& opt) : imp(device, vid, opt, (uint64_t)1 << 30) {}
  DeviceImporter::Impl& M() { return *imp.m_; }
  void adopt_batch(uint32_t n_rec, uint32_t per_line, bool text);
  void convert(Stream& s);
  void free_batch_cells() { for (uint8_t* p : batch_cells) (void)hipFree(p); batch_cells.clear(); }
  void need_usable(const char* what) const {
    if (failed) throw VCF2BinaryException(std::string(what) + ": an earlier call of this importer failed; it can only be closed");
    if (finished) throw VCF2BinaryException(std::string(what) + " after finish()");
  }
};

DeviceStreamImporter::DeviceStreamImporter(int device, const VidMapper& vid, const ImportOptions& opt, const std::vector<BufferStreamDecl>& decls) : m_(nullptr) {
  m_ = new Impl(device, vid, opt);
  try {
    Impl& S = *m_;
    DeviceImporter::Impl& M = S.M();
    // the sources of the callset mapping in order of first appearance (the reference's global file index)
    std::vector<std::string> sources;
    for (const CallSetInfo& cs : vid.get_callsets()) if (std::find(sources.begin(), sources.end(), cs.m_filename) == sources.end()) sources.push_back(cs.m_filename);
    for (const BufferStreamDecl& d : decls) {
      S.streams.emplace_back();
      Impl::Stream& s = S.streams.back();
      s.decl = d;
      for (const ImportFile& f : M.files) if (f.name == d.name) { s.used = true; s.file = f; }
      if (s.used) {
        s.file.path = "stream " + d.name;      // messages name the stream
        if (s.file.type != GDB_FILE_VCF) throw VCF2BinaryException("stream " + d.name + " is listed as a CSV file: CSV buffer streams are not imported");
        s.file_idx = (int64_t)(std::find(sources.begin(), sources.end(), d.name) - sources.begin());
        ++S.n_used;
        const char* p = (const char*)d.init.data();
        const size_t n = d.init.size();
        if (is_gzip(p, n)) throw VCF2BinaryException("stream " + d.name + ": the initialisation bytes are gzip or BGZF; buffer streams carry plain VCF text or plain BCF2");
        if (is_bcf2(p, n) != d.is_bcf)
          throw VCF2BinaryException("stream " + d.name + " was added as " + (d.is_bcf ? "BCF2" : "VCF text") + ", but its initialisation bytes " +
                                    (d.is_bcf ? "do not begin with a BCF2 header" : "begin with a BCF2 header"));
        size_t records_begin = 0;
        if (d.is_bcf) { s.bcf_hdr = parse_bcf_header(p, n, s.file, M.H); records_begin = s.bcf_hdr.records_begin; }
        else { s.text_hdr = parse_import_header(std::string(p, n), s.file); records_begin = s.text_hdr.record_begin; s.lines_before = s.text_hdr.lines_before; }
        s.bytes_before = records_begin;
        s.buf.assign(d.init.begin() + (long)records_begin, d.init.end());
      } else s.reported = false;
      S.file_idx.push_back(s.file_idx);
    }
    for (const ImportFile& f : M.files) {
      bool have = false;
      for (const Impl::Stream& s : S.streams) have = have || s.decl.name == f.name;
      if (!have) throw VCF2BinaryException("callset source " + f.name + " has no buffer stream: the streaming importer reads buffer streams only");
    }
    IMP_HIP_CHECK(hipSetDevice(M.device));
    for (auto& e : S.ev) IMP_HIP_CHECK(hipEventCreate(&e));
    S.d_order.ensure(2);
    S.d_counters.ensure(4);
    M.after_batch = [this](uint32_t n, uint32_t per_line, bool text) { m_->adopt_batch(n, per_line, text); };
  } catch (...) { this->~DeviceStreamImporter(); throw; }
}

DeviceStreamImporter::~DeviceStreamImporter() {
  if (!m_) return;
  DeviceImporter::Impl& M = m_->M();
  if (M.stream) { (void)hipSetDevice(M.device); (void)hipStreamSynchronize(M.stream); }
  m_->free_batch_cells();
  for (auto& e : m_->ev) if (e) (void)hipEventDestroy(e);
  delete m_;
  m_ = nullptr;
}

const std::vector<int64_t>& DeviceStreamImporter::stream_file_idx() const { return m_->file_idx; }
size_t DeviceStreamImporter::num_used_streams() const { return m_->n_used; }
const std::vector<std::pair<int64_t, int>>& DeviceStreamImporter::exhausted() const { return m_->exhausted; }
const StreamImportStats& DeviceStreamImporter::stats() const { return m_->st; }

bool DeviceStreamImporter::is_done() const {
  if (m_->failed || m_->st.num_batches == 0) return false;
  for (const Impl::Stream& s : m_->streams) if (s.used && !s.ended) return false;
  return m_->n_pending == 0;
}

void DeviceStreamImporter::write(int64_t idx, unsigned partition_idx, const uint8_t* data, size_t n) {
  Impl& S = *m_;
  S.need_usable("write_data_to_buffer_stream");
  if (idx < 0 || (size_t)idx >= S.streams.size()) throw VCF2BinaryException("buffer stream index " + std::to_string(idx) + " is not one of the " + std::to_string(S.streams.size()) + " streams");
  Impl::Stream& s = S.streams[(size_t)idx];
  if (partition_idx != 0) throw VCF2BinaryException("stream " + s.decl.name + ": partition index " + std::to_string(partition_idx) + "; an importer has one partition, index 0");
  if (!s.used) throw VCF2BinaryException("stream " + s.decl.name + " is not used by a callset inside the row bounds: nothing can be written to it");
  if (s.ended) throw VCF2BinaryException("stream " + s.decl.name + " has ended: nothing can be written to it");
  if (!data && n) throw VCF2BinaryException("stream " + s.decl.name + ": null data");
  if (n >= ((size_t)1 << 31)) throw VCF2BinaryException("stream " + s.decl.name + ": a write of 2 GiB or more");
  // whole records only
  if (n && !s.decl.is_bcf && data[n - 1] != '\n') {
    const void* nl = memrchr(data, '\n', n);
    const size_t tail = nl ? (size_t)((const uint8_t*)nl - data) + 1 : 0;
    throw VCF2BinaryException("stream " + s.decl.name + ": the write ends inside a record line that begins at byte offset " + std::to_string(s.bytes_before + tail) +
                              " of the stream; a write holds whole lines");
  }
  if (n && s.decl.is_bcf) {
    size_t at = 0;
    while (at < n) {
      uint32_t l_shared = 0, l_indiv = 0;
      if (n - at >= 8) { memcpy(&l_shared, data + at, 4); memcpy(&l_indiv, data + at + 4, 4); }
      if (n - at < 8 || 8ull + l_shared + l_indiv > n - at)
        throw VCF2BinaryException("stream " + s.decl.name + ": the write ends inside the BCF2 record that begins at byte offset " + std::to_string(s.bytes_before + at) +
                                  " of the stream; a write holds whole l_shared / l_indiv records");
      at += 8ull + l_shared + l_indiv;
    }
  }
  s.buf.assign(data, data + n);      // replaces the buffer, as the reference's write does
  s.decl.capacity = std::max(s.decl.capacity, n);
}

// the hook of DeviceImporter::Impl::cells_of_batch: order check of the write, then its slots join the pending ones
void DeviceStreamImporter::Impl::adopt_batch(uint32_t n_rec, uint32_t per_line, bool text) {
  DeviceImporter::Impl& D = M();
  Stream& s = *cur;
  hipStream_t q = D.stream;
  const unsigned long long init[2] = {kNoError, 0ull};
  unsigned long long got[2] = {kNoError, 0ull};
  IMP_HIP_CHECK(hipMemcpyAsync(d_order.p, init, sizeof(init), hipMemcpyHostToDevice, q));
  IMP_HIP_CHECK(hipEventRecord(ev[0], q));
  hipLaunchKernelGGL(k_str_order, dim3(grid_for(n_rec)), dim3(kBlock), 0, q, (const int64_t*)D.d_col.p, per_line, n_rec, s.last, text ? (const char*)D.d_text.p : nullptr,
                     text ? (const uint32_t*)D.d_nl.p : nullptr, d_order.p);
  IMP_HIP_CHECK(hipEventRecord(ev[1], q));
  IMP_HIP_CHECK(hipMemcpyAsync(got, d_order.p, sizeof(got), hipMemcpyDeviceToHost, q));
  IMP_HIP_CHECK(hipStreamSynchronize(q));
  float ms = 0;
  IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_order += ms;
  if (got[0] != kNoError) {
    const uint64_t record = s.records + (got[0] & (((uint64_t)1 << 62) - 1u)) + 1u;
    if ((got[0] >> 62) == STR_ERR_NOT_A_RECORD)
      throw VCF2BinaryException("stream " + s.decl.name + ": line " + std::to_string(record) + " of its records is empty or a '#' line; a write holds record lines only");
    throw VCF2BinaryException("stream " + s.decl.name + ": record " + std::to_string(record) + " lies at a column in front of the record before it; a stream cannot go back");
  }
  s.last = (int64_t)got[1];
  s.records += n_rec;
  // the batch's slots join the pending ones; its cells stay in its buffer until the next compaction
  DeviceImporter::Impl::Batch b = D.batches.back();
  const uint64_t n = b.n_slots;
  Slots& P = slots[cur_slots];
  grow_keep(P.key, n_pending + n, n_pending, q); grow_keep(P.src, n_pending + n, n_pending, q); grow_keep(P.size, n_pending + n, n_pending, q);
  if (D.spanning) grow_keep(P.tag, n_pending + n, n_pending, q);
  IMP_HIP_CHECK(hipMemcpyAsync(P.key.p + n_pending, b.key, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, q));
  IMP_HIP_CHECK(hipMemcpyAsync(P.src.p + n_pending, b.src, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, q));
  IMP_HIP_CHECK(hipMemcpyAsync(P.size.p + n_pending, b.size, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, q));
  if (D.spanning) IMP_HIP_CHECK(hipMemcpyAsync(P.tag.p + n_pending, b.tag, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, q));
  IMP_HIP_CHECK(hipStreamSynchronize(q));
  D.batches.pop_back();
  (void)hipFree(b.key); (void)hipFree(b.src); (void)hipFree(b.size); if (b.tag) (void)hipFree(b.tag);
  batch_cells.push_back(b.cells);
  n_pending += n;
  pending_cells += (int64_t)D.total_cells;
  pending_bytes += b.cells_bytes;
  D.total_slots = 0; D.total_cells = 0;      // (they bound one finish(); here a batch is handed over long before)
}

void DeviceStreamImporter::Impl::convert(Stream& s) {
  DeviceImporter::Impl& D = M();
  cur = &s;
  const char* data = (const char*)s.buf.data();
  const size_t n = s.buf.size();
  if (!s.decl.is_bcf) {
    const int n_imp = D.upload_samples(s.text_hdr);
    s.lines_before += D.batch(s.file, s.text_hdr, data, n, false, s.lines_before, n_imp);
  } else {
    const int n_imp = D.upload_samples(s.bcf_hdr.samples);
    const gdbimp::ImpBcfTables BT = D.upload_bcf_tables(s.bcf_hdr);
    std::vector<uint64_t> offs;
    bcf_walk_records(data, n, 0, s.file.path, offs);
    D.bcf_batches(s.file, s.bcf_hdr, BT, n_imp, data, offs, s.records);
  }
  s.bytes_before += n;
  s.buf.clear();
  cur = nullptr;
}

void DeviceStreamImporter::import_batch(std::vector<uint8_t>& cells) {
  Impl& S = *m_;
  S.need_usable("import_batch");
  cells.clear();
  DeviceImporter::Impl& D = S.M();
  hipStream_t q = D.stream;
  try {
    IMP_HIP_CHECK(hipSetDevice(D.device));
    // ---- every buffer is consumed; an exhausted stream without bytes has ended
    for (Impl::Stream& s : S.streams) {
      if (!s.used || s.ended) continue;
      if (!s.buf.empty()) S.convert(s);
      else if (s.reported) { s.ended = true; s.last = kColPosInf; }
    }
    ++S.st.num_batches;
    int64_t W = kColPosInf;
    for (const Impl::Stream& s : S.streams) if (s.used && !s.ended) W = std::min(W, s.last);
    S.st.max_pending_cells = std::max(S.st.max_pending_cells, S.pending_cells);
    S.st.max_pending_bytes = std::max(S.st.max_pending_bytes, S.pending_bytes);
    const uint64_t N = S.n_pending;
    if (N) {
      Impl::Slots& P = S.slots[S.cur_slots];
      Impl::Slots& O = S.slots[1 - S.cur_slots];
      // ---- classify
      grow_drop(S.d_cls, N); grow_drop(S.d_emit_key, N); grow_drop(S.d_keep_flag, N); grow_drop(S.d_keep_bytes, N); grow_drop(S.d_dst, N); grow_drop(S.d_doff, N);
      unsigned long long c[4] = {0, 0, 0, 0};
      IMP_HIP_CHECK(hipMemsetAsync(S.d_counters.p, 0, sizeof(c), q));
      IMP_HIP_CHECK(hipEventRecord(S.ev[2], q));
      hipLaunchKernelGGL(k_str_classify, dim3(grid_for(N)), dim3(kBlock), 0, q, (const uint64_t*)P.key.p, D.spanning ? (const uint64_t*)P.tag.p : nullptr, (const uint32_t*)P.size.p,
                         N, D.H.key_row_bits, D.H.max_row, D.spanning ? (const unsigned long long*)D.d_row_best.p : nullptr, W, D.opt.column_begin, S.d_cls.p, S.d_emit_key.p,
                         S.d_keep_flag.p, S.d_keep_bytes.p, S.d_counters.p);
      IMP_HIP_CHECK(hipEventRecord(S.ev[3], q));
      IMP_HIP_CHECK(hipMemcpyAsync(c, S.d_counters.p, sizeof(c), hipMemcpyDeviceToHost, q));
      IMP_HIP_CHECK(hipStreamSynchronize(q));
      const uint64_t n_emit = c[0], n_keep = c[1], keep_pool_bytes = c[3];
      float ms = 0;
      IMP_HIP_CHECK(hipEventElapsedTime(&ms, S.ev[2], S.ev[3])); S.st.ms_classify += ms;
      // ---- emit: finish()'s sort and gather over the emit keys (every other slot sorts behind the emitted)
      if (n_emit) {
        grow_drop(S.d_key_sorted, N); grow_drop(S.d_idx, N); grow_drop(S.d_idx_sorted, N); grow_drop(S.d_sorted_size, n_emit + 1); grow_drop(S.d_sorted_off, n_emit + 1);
        IMP_HIP_CHECK(hipEventRecord(S.ev[4], q));
        launch_iota(S.d_idx.p, N, q);
        size_t bytes = 0;
        IMP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, S.d_emit_key.p, S.d_key_sorted.p, S.d_idx.p, S.d_idx_sorted.p, (size_t)N, 0, 64, q));
        D.d_tmp.ensure(std::max<size_t>(bytes, 16));
        IMP_HIP_CHECK(rocprim::radix_sort_pairs((void*)D.d_tmp.p, bytes, S.d_emit_key.p, S.d_key_sorted.p, S.d_idx.p, S.d_idx_sorted.p, (size_t)N, 0, 64, q));
        launch_sorted_sizes(S.d_idx_sorted.p, P.size.p, n_emit, S.d_sorted_size.p, q);
        D.scan<uint64_t>(S.d_sorted_size.p, S.d_sorted_off.p, (size_t)n_emit + 1);
        uint64_t out_bytes = 0;
        IMP_HIP_CHECK(hipMemcpyAsync(&out_bytes, S.d_sorted_off.p + n_emit, sizeof(uint64_t), hipMemcpyDeviceToHost, q));
        IMP_HIP_CHECK(hipStreamSynchronize(q));
        grow_drop(S.d_out, out_bytes + 16);
        launch_gather(S.d_idx_sorted.p, P.src.p, P.size.p, S.d_sorted_off.p, n_emit, S.d_out.p, out_bytes, q);
        IMP_HIP_CHECK(hipEventRecord(S.ev[5], q));
        IMP_HIP_CHECK(hipStreamSynchronize(q));
        IMP_HIP_CHECK(hipEventElapsedTime(&ms, S.ev[4], S.ev[5])); S.st.ms_sort_gather += ms;
        const double t0 = now_s();
        cells.resize(out_bytes);
        if (out_bytes) IMP_HIP_CHECK(hipMemcpy(cells.data(), S.d_out.p, out_bytes, hipMemcpyDeviceToHost));
        S.st.s_d2h += now_s() - t0;
        S.st.num_cells += (int64_t)n_emit;
        S.st.num_bytes += out_bytes;
        S.st.num_spanning_cells += (int64_t)c[2];
      }
      // ---- compact: the kept slots and their bytes move to the other arrays and the other pool
      if (n_keep) {
        grow_drop(O.key, n_keep); grow_drop(O.src, n_keep); grow_drop(O.size, n_keep);
        if (D.spanning) grow_drop(O.tag, n_keep);
        grow_drop(S.pool[1 - S.cur_slots], keep_pool_bytes + 16);
        IMP_HIP_CHECK(hipEventRecord(S.ev[6], q));
        D.scan<uint64_t>(S.d_keep_flag.p, S.d_dst.p, (size_t)N);
        D.scan<uint64_t>(S.d_keep_bytes.p, S.d_doff.p, (size_t)N);
        hipLaunchKernelGGL(k_str_compact, dim3(grid_for(N * 64)), dim3(kBlock), 0, q, (const uint8_t*)S.d_cls.p, (const uint64_t*)S.d_dst.p, (const uint64_t*)S.d_doff.p, N,
                           (const uint64_t*)P.key.p, (const uint32_t*)P.size.p, D.spanning ? (const uint64_t*)P.tag.p : nullptr, (const uint64_t*)P.src.p, O.key.p, O.size.p,
                           D.spanning ? O.tag.p : nullptr, O.src.p, S.pool[1 - S.cur_slots].p, keep_pool_bytes, n_keep);
        IMP_HIP_CHECK(hipEventRecord(S.ev[7], q));
        IMP_HIP_CHECK(hipStreamSynchronize(q));
        IMP_HIP_CHECK(hipEventElapsedTime(&ms, S.ev[6], S.ev[7])); S.st.ms_compact += ms;
        S.cur_slots = 1 - S.cur_slots;
      }
      S.free_batch_cells();
      S.n_pending = n_keep; S.pending_cells = (int64_t)n_keep; S.pending_bytes = n_keep ? keep_pool_bytes : 0;
    }
    // ---- who must be refilled
    S.exhausted.clear();
    for (size_t i = 0; i < S.streams.size(); ++i) {
      Impl::Stream& s = S.streams[i];
      s.reported = s.used && !s.ended && s.last <= W;
      if (s.reported) S.exhausted.emplace_back((int64_t)i, 0);
    }
    S.st.num_records = D.st.num_records;
    S.st.num_deferred_values = D.st.num_deferred_values;
    S.st.s_h2d = D.st.s_h2d;
  } catch (...) { S.failed = true; S.cur = nullptr; cells.clear(); throw; }
}

void DeviceStreamImporter::finish() {
  Impl& S = *m_;
  S.need_usable("finish");
  if (!is_done()) throw VCF2BinaryException("finish() before the import is done: a stream has not ended, or import_batch was never called");
  S.finished = true;
  for (DBuf<uint8_t>& p : S.pool) if (p.p) { (void)hipFree(p.p); p.p = nullptr; p.cap = 0; }
}

}  // namespace genomicsdb_amd
