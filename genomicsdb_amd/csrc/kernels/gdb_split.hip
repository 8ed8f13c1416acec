// gdb_split.hip - see gdb_split.h.  Kernels for gfx950 around the bodies of core/gdb_split.hpp, and their orchestration.
#include "gdb_split.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../core/gdb_split.hpp"
#include "../host/import_bcf.hpp"
#include "../host/import_common.hpp"
#include "../host/vcf_index.h"
#include "gdb_bgzf.h"
#include "gdb_import.h"
#include "gdb_import_device.hpp"
#include "gdb_index.h"
#include "gdb_inflate.h"

namespace genomicsdb_amd {

namespace {
using namespace gdbimp;
using namespace gdbsplit;
using namespace impdev;

// counters: [0] record lines, [1] smallest p_lo, [2] largest p_hi + 1 of the lines that go anywhere
// One thread per line.  The sorted begins and ends are staged in LDS (16 bytes per partition, at most 64 KiB): every thread
// searches them twice.
__global__ void __launch_bounds__(kBlock) k_split_classify(ImpTables T, ImpBatch B, const int64_t* begins, const int64_t* ends, uint32_t n_parts, uint32_t* p_lo,
                                                          uint32_t* p_hi, uint32_t* len, uint32_t* err, unsigned int* counters) {
  extern __shared__ int64_t s_parts[];
  for (uint32_t i = threadIdx.x; i < n_parts; i += kBlock) { s_parts[i] = begins[i]; s_parts[n_parts + i] = ends[i]; }
  __syncthreads();
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  bool is_record = false;
  uint32_t lo = 1u, hi = 0u;
  if (line < B.n_lines) {
    const ImpLine L = imp_line_of(B, line);
    const SplitParts P{s_parts, s_parts + n_parts, n_parts};
    const SplitSel s = split_classify(T, P, L);
    if (s.err) imp_raise(err, s.err, line);
    is_record = L.end > L.begin && B.text[L.begin] != '#';
    lo = s.p_lo; hi = s.p_hi;
    p_lo[line] = lo; p_hi[line] = hi;
    len[line] = B.nl_pos[line] + 1u - L.begin;       // with the newline (and a '\r' in front of it)
  }
  const unsigned long long rec = __ballot(is_record);
  uint32_t first = lo <= hi ? lo : UINT32_MAX, behind = lo <= hi ? hi + 1u : 0u;      // reduced over the wavefront: one atomic each
  for (int d = 32; d; d >>= 1) {
    const uint32_t f = (uint32_t)__shfl_xor((int)first, d), h = (uint32_t)__shfl_xor((int)behind, d);
    first = f < first ? f : first;
    behind = h > behind ? h : behind;
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (rec) atomicAdd(&counters[0], (unsigned int)__popcll(rec));
    if (behind) { atomicMin(&counters[1], first); atomicMax(&counters[2], behind); }
  }
}

// the lines of partition p: their length, 0 for every other line; sel has n_lines + 1 entries, the last one 0 (the scan's total)
__global__ void __launch_bounds__(kBlock) k_split_select(uint32_t p, const uint32_t* p_lo, const uint32_t* p_hi, const uint32_t* len, const char* text,
                                                        const uint32_t* nl_pos, uint32_t n_lines, uint32_t* sel, unsigned int* n_selected) {
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  bool in = false, record = false;
  if (line < n_lines) {
    in = p_lo[line] <= p && p <= p_hi[line];
    sel[line] = in ? len[line] : 0u;
    record = in && text[line ? nl_pos[line - 1u] + 1u : 0u] != '#';
  } else if (line == n_lines) sel[line] = 0u;
  const unsigned long long m = __ballot(record);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(n_selected, (unsigned int)__popcll(m));
}

// 16 bytes that begin `sh` (1 .. 15) bytes into lo, continued in hi
__device__ __forceinline__ uint4 split_align16(const uint4 lo, const uint4 hi, uint32_t sh) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8u;
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (ws == (uint32_t)j) { a = w[i + j]; b = w[i + j + 1]; }
    o[i] = (uint32_t)((((uint64_t)b << 32) | (uint64_t)a) >> bs);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// One wavefront per selected line (100 B to many KB): bytes up to the destination's next 16-byte boundary, then one aligned
// 16-byte store per lane and step - the source is read with aligned 16-byte loads too and shifted into place (its alignment
// relative to the destination is the same for the whole line) - then the bytes left over.  The loads may touch up to 15 bytes
// in front of the line (inside the text: it begins 16-byte aligned) and 31 behind it (inside the text's padding, kTextPad).
__global__ void __launch_bounds__(kBlock) k_split_gather(const char* text, uint32_t n_text, const uint32_t* nl_pos, const uint32_t* sel, const uint32_t* off,
                                                        uint32_t n_lines, char* dst, uint64_t dst_room) {
  const uint32_t line = (blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (line >= n_lines) return;
  const uint32_t n = sel[line];
  if (!n) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t from = line ? nl_pos[line - 1u] + 1u : 0u;
  const uint64_t at = off[line];
  if ((uint64_t)from + n > (uint64_t)n_text || at + n > dst_room) return;      // (never, by the index and the scan: nothing leaves the buffers)
  const char* s = text + from;
  char* d = dst + at;
  uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > n) head = n;
  if (lane < head) d[lane] = s[lane];
  const uint32_t n16 = (n - head) >> 4;
  const uint32_t sh = (uint32_t)((uintptr_t)(s + head) & 15u);
  const uint4* sa = reinterpret_cast<const uint4*>(s + head - sh);
  uint4* da = reinterpret_cast<uint4*>(d + head);
  for (uint32_t k = lane; k < n16; k += 64u) da[k] = sh ? split_align16(sa[k], sa[k + 1u], sh) : sa[k];
  const uint32_t done = head + (n16 << 4);
  if (lane < n - done) d[done + lane] = s[done + lane];
}

constexpr uint64_t kChunkBytes = (uint64_t)16 << 20;      // packed text a partition collects on the device before it is deflated

struct PartOut {
  int partition = 0; uint32_t sorted_at = 0;
  std::string final_path, tmp_path;
  FILE* f = nullptr;
  DBuf<char>* acc = nullptr; uint64_t fill = 0;      // the packed text it has collected (Splitter::accs: kept from file to file)
  // index_on_device: the output so far, in uncompressed and in file bytes, the lines of its header, and its index builder
  uint64_t u_done = 0, file_pos = 0; int64_t header_lines = 0;
  size_t slot = 0; bool tbi_begun = false;      // Splitter::tbis[slot]
};

void remove_quietly(const std::string& path) { if (!path.empty()) (void)remove(path.c_str()); }

struct Splitter {
  const VidMapper& vid;
  const SplitRequest& req;
  SplitStats st;
  hipStream_t stream = nullptr;                // the importer's, taken from the first batch
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<int64_t> begins, ends;           // sorted by begin
  std::vector<int> sorted_to_index;
  std::vector<int> produce;                    // partition indices
  uint64_t chunk = kChunkBytes;
  BgzfDeviceCompressor comp;
  DBuf<int64_t> d_parts;
  DBuf<uint32_t> d_lo, d_hi, d_len, d_sel, d_off, d_err;
  DBuf<unsigned int> d_counters;
  DBuf<char> d_tmp, d_z;
  std::vector<std::unique_ptr<DBuf<char>>> accs;      // one per produced partition
  std::vector<std::unique_ptr<DeviceTbiBuilder>> tbis;      // index_on_device: the same (the device buffers are kept from file to file)
  std::vector<BgzfMember> blocks;
  std::vector<char> h_z;
  std::vector<PartOut> outs;                   // of the input that is being read
  std::string original;                        // its name
  bool header_seen = false;
  std::vector<SplitOutput> done;

  Splitter(const VidMapper& v, const SplitRequest& r) : vid(v), req(r) { comp.set_text(true); }
  ~Splitter() {
    abort_file();
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  }

  void abort_file() {
    for (PartOut& o : outs) {
      if (o.f) { fclose(o.f); o.f = nullptr; }
      if (!o.tmp_path.empty()) { remove_quietly(o.tmp_path); remove_quietly(o.tmp_path + ".tbi"); }
    }
    outs.clear();
  }

  void write(PartOut& o, const char* p, size_t n) {
    if (n && fwrite(p, 1, n, o.f) != n) throw VCF2BinaryException("short write to " + o.tmp_path);
    st.compressed_bytes_out += n;
  }

  // the outputs of one input: opened under their temporary names, the '#' lines written
  void begin_file(const std::string& name, const std::string& path) {
    original = name;
    header_seen = false;
    outs.clear();
    outs.resize(produce.size());
    for (size_t i = 0; i < produce.size(); ++i) {
      PartOut& o = outs[i];
      o.partition = produce[i];
      if (accs.size() <= i) accs.emplace_back(new DBuf<char>());
      o.acc = accs[i].get();
      if (tbis.size() <= i) tbis.resize(i + 1);
      o.slot = i;
      o.sorted_at = (uint32_t)(std::find(sorted_to_index.begin(), sorted_to_index.end(), produce[i]) - sorted_to_index.begin());
      o.final_path = !req.single_output.empty() ? req.single_output : vid.get_split_file_path(name, req.results_directory, o.partition, path);
      o.tmp_path = o.final_path + ".split.tmp";
    }
    for (PartOut& o : outs) {
      o.f = fopen(o.tmp_path.c_str(), "wb");
      if (!o.f) { const std::string p = o.tmp_path; o.tmp_path.clear(); throw VCF2BinaryException("cannot write " + p); }
    }
  }

  void on_header(const std::string&, const std::string& head) {
    header_seen = true;
    std::string lines;                         // the '#' lines; an empty line is no line of the output
    size_t pos = 0;
    while (pos < head.size()) {
      size_t eol = head.find('\n', pos);
      if (eol == std::string::npos) eol = head.size();
      size_t ln = eol - pos;
      if (ln && head[pos + ln - 1] == '\r') --ln;
      if (ln) { lines.append(head, pos, eol - pos); lines.push_back('\n'); }
      pos = eol + 1;
    }
    st.text_bytes_in += head.size();
    if (lines.empty()) return;
    const std::string z = bgzf_compress_host(lines);
    const int64_t n_lines = (int64_t)std::count(lines.begin(), lines.end(), '\n');
    for (PartOut& o : outs) {
      write(o, z.data(), z.size()); st.text_bytes_out += lines.size();
      o.u_done += lines.size(); o.file_pos += z.size(); o.header_lines += n_lines;
    }
  }

  // index_on_device: the output's builder, made when the first block of the first output is there and then kept
  DeviceTbiBuilder& builder_of(PartOut& o) {
    std::unique_ptr<DeviceTbiBuilder>& b = tbis.at(o.slot);
    if (!b) b.reset(new DeviceTbiBuilder(o.tmp_path, (void*)stream));
    if (!o.tbi_begun) { b->reset(o.tmp_path, o.header_lines); o.tbi_begun = true; }
    return *b;
  }
  // the packed text that flush() just deflated is still in o.acc, the blocks it became are in h_z: a batch of the output's index.
  // What lies behind the batch's last line is the next block, which is not written yet: its offset is named with the next
  // batch, or in end_file
  void index_flushed(PartOut& o, uint64_t n_compressed) {
    const double t0 = now_s();
    DeviceTbiBuilder& B = builder_of(o);
    B.resolve_pending(o.file_pos << 16);
    uint64_t total = 0, break_at = 0;
    if (!bgzf_walk((const uint8_t*)h_z.data(), n_compressed, blocks, &total, &break_at) || total != o.fill)
      throw GenomicsDBDeviceException("split: the deflated blocks of " + o.tmp_path + " are not the text they were made of");
    IndexMemberTable table;
    for (const BgzfMember& m : blocks) if (m.isize) { table.ubase.push_back(o.u_done + m.out_off); table.coff.push_back(o.file_pos + m.offset); }
    table.total = o.u_done + o.fill; table.v_total = DeviceTbiBuilder::kPending;
    B.set_members(table);
    if (B.add_batch(o.acc->p, (uint32_t)o.fill, o.u_done) != o.fill) throw GenomicsDBDeviceException("split: the packed text of " + o.tmp_path + " does not end with a line");
    st.s_index_build += now_s() - t0;
  }

  template <class T> void scan(const T* in, T* out, size_t n) {
    size_t bytes = 0;
    IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
    d_tmp.ensure(std::max<size_t>(bytes, 16));
    IMP_HIP_CHECK(rocprim::exclusive_scan((void*)d_tmp.p, bytes, in, out, T(0), n, rocprim::plus<T>(), stream));
  }

  // the partition's packed text -> BGZF blocks -> its file
  void flush(PartOut& o) {
    if (!o.fill) return;
    d_z.ensure((size_t)bgzf_bound(o.fill));
    float ms = 0;
    const uint64_t n = comp.compress(o.acc->p, o.fill, d_z.p, (void*)stream, &ms);
    st.ms_deflate += ms;
    const double t0 = now_s();
    h_z.resize((size_t)n);
    IMP_HIP_CHECK(hipMemcpy(h_z.data(), d_z.p, (size_t)n, hipMemcpyDeviceToHost));
    write(o, h_z.data(), (size_t)n);
    st.s_d2h_write += now_s() - t0;
    st.text_bytes_out += o.fill;
    if (req.index_on_device) index_flushed(o, n);
    o.u_done += o.fill; o.file_pos += n;
    o.fill = 0;
  }

  void on_batch(const ImportTextBatch& b) {
    if (!stream) {
      stream = (hipStream_t)b.stream;
      for (auto& e : ev) IMP_HIP_CHECK(hipEventCreate(&e));
      const uint32_t np = (uint32_t)begins.size();
      d_parts.ensure(2 * (size_t)np);
      IMP_HIP_CHECK(hipMemcpyAsync(d_parts.p, begins.data(), np * sizeof(int64_t), hipMemcpyHostToDevice, stream));
      IMP_HIP_CHECK(hipMemcpyAsync(d_parts.p + np, ends.data(), np * sizeof(int64_t), hipMemcpyHostToDevice, stream));
      d_err.ensure(kErrWords);
      d_counters.ensure(4);
    }
    const uint32_t np = (uint32_t)begins.size(), n_lines = b.n_lines;
    ++st.num_batches;
    st.text_bytes_in += b.n_bytes;
    d_lo.ensure(n_lines); d_hi.ensure(n_lines); d_len.ensure(n_lines); d_sel.ensure((size_t)n_lines + 1); d_off.ensure((size_t)n_lines + 1);
    // ---- classify: once per batch
    const unsigned int init[4] = {0u, UINT32_MAX, 0u, 0u};
    IMP_HIP_CHECK(hipMemcpyAsync(d_counters.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
    IMP_HIP_CHECK(hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), stream));
    IMP_HIP_CHECK(hipMemsetAsync(d_err.p + 1, 0xFF, (kErrWords - 1) * sizeof(uint32_t), stream));
    IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(k_split_classify, dim3(grid_for(n_lines)), dim3(kBlock), 2 * (size_t)np * sizeof(int64_t), stream, *b.tables,
                       ImpBatch{b.d_text, b.d_nl, b.d_first_tab, b.d_tab, n_lines}, (const int64_t*)d_parts.p, (const int64_t*)(d_parts.p + np), np, d_lo.p, d_hi.p, d_len.p,
                       d_err.p, d_counters.p);
    IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
    unsigned int counters[4];
    uint32_t err[kErrWords];
    IMP_HIP_CHECK(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0;
    IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_classify += ms;
    // ---- errors: the smallest offending line speaks
    uint32_t err_line = UINT32_MAX, err_bit = 0;
    for (int k = 0; k < kErrWords - 1; ++k) if ((err[0] & (1u << k)) && err[1 + k] < err_line) { err_line = err[1 + k]; err_bit = 1u << k; }
    if (err_bit) {
      std::string words;
      try { words = b.describe(err_bit, err_line); }
      catch (const VCF2BinaryException& e) {      // the host parser's own words for a POS / END it refuses too: they name no line, so it is added
        words = e.what();
        if (words.compare(0, strlen("VCF2BinaryException : "), "VCF2BinaryException : ") == 0) words = words.substr(strlen("VCF2BinaryException : "));
        words += " (" + *b.path + " line " + std::to_string(b.lines_before + (int64_t)err_line + 1) + ")";
      }
      throw VCF2BinaryException(words);
    }
    st.num_record_lines += counters[0];
    // ---- compact: the produced partitions that the batch touches
    for (PartOut& o : outs) {
      if (counters[1] > o.sorted_at || o.sorted_at >= counters[2]) continue;
      IMP_HIP_CHECK(hipMemsetAsync(d_counters.p + 3, 0, sizeof(unsigned int), stream));
      IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
      hipLaunchKernelGGL(k_split_select, dim3(grid_for((uint64_t)n_lines + 1)), dim3(kBlock), 0, stream, o.sorted_at, (const uint32_t*)d_lo.p, (const uint32_t*)d_hi.p,
                         (const uint32_t*)d_len.p, b.d_text, b.d_nl, n_lines, d_sel.p, d_counters.p + 3);
      scan<uint32_t>(d_sel.p, d_off.p, (size_t)n_lines + 1);
      IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
      uint32_t total = 0;
      unsigned int n_selected = 0;
      IMP_HIP_CHECK(hipMemcpyAsync(&total, d_off.p + n_lines, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      IMP_HIP_CHECK(hipMemcpyAsync(&n_selected, d_counters.p + 3, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
      IMP_HIP_CHECK(hipStreamSynchronize(stream));
      IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_scan_gather += ms;
      if (!total) continue;
      const uint64_t pad = req.index_on_device ? kTextPad : 0u;      // (the index pass reads whole 16-byte groups)
      if (o.fill + total + pad > o.acc->cap) flush(o);
      o.acc->ensure((size_t)(std::max<uint64_t>(chunk, (uint64_t)total) + pad));      // (grows only when empty: flush() came first)
      IMP_HIP_CHECK(hipEventRecord(ev[2], stream));
      hipLaunchKernelGGL(k_split_gather, dim3(grid_for((uint64_t)n_lines * 64u)), dim3(kBlock), 0, stream, b.d_text, b.n_bytes, b.d_nl, (const uint32_t*)d_sel.p,
                         (const uint32_t*)d_off.p, n_lines, o.acc->p + o.fill, (uint64_t)o.acc->cap - o.fill);
      IMP_HIP_CHECK(hipEventRecord(ev[3], stream));
      IMP_HIP_CHECK(hipStreamSynchronize(stream));
      IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[2], ev[3])); st.ms_scan_gather += ms;
      o.fill += total;
      st.num_lines_written += n_selected;
    }
  }

  // the input went through: last blocks, EOF block, index, and only then the outputs' own names
  void end_file() {
    if (!header_seen) on_header(original, std::string());      // (an empty input)
    for (PartOut& o : outs) {
      flush(o);
      write(o, (const char*)kBgzfEofBlock, sizeof(kBgzfEofBlock));
      const int rc = fclose(o.f);
      o.f = nullptr;
      if (rc != 0) throw VCF2BinaryException("cannot write " + o.tmp_path);
      const double t0 = now_s();
      if (req.index_on_device) {
        DeviceTbiBuilder& B = builder_of(o);
        B.resolve_pending((o.file_pos + sizeof(kBgzfEofBlock)) << 16);      // behind the last line: the end of the file
        B.finish(o.tmp_path + ".tbi");
        st.ms_index_kernels += B.st.ms_index + B.st.ms_records + B.st.ms_chunks + B.st.ms_linear;
      } else build_tbi_index(o.tmp_path);
      st.s_index_build += now_s() - t0;
    }
    for (PartOut& o : outs) {
      if (rename(o.tmp_path.c_str(), o.final_path.c_str()) != 0 || rename((o.tmp_path + ".tbi").c_str(), (o.final_path + ".tbi").c_str()) != 0) {
        for (PartOut& x : outs) { remove_quietly(x.final_path); remove_quietly(x.final_path + ".tbi"); }
        throw VCF2BinaryException("cannot rename " + o.tmp_path + " to " + o.final_path);
      }
      o.tmp_path.clear();
      SplitOutput so; so.original = original; so.partition = o.partition; so.path = o.final_path;
      done.push_back(so);
    }
    outs.clear();
    ++st.num_files;
  }
};

}  // namespace

std::vector<std::pair<std::string, std::string>> split_input_files(const VidMapper& vid, const SplitRequest& req) {
  std::vector<std::pair<std::string, std::string>> files;
  auto add = [&](const std::string& name, const std::string& path) {
    for (const auto& f : files) if (f.first == name) return;
    files.emplace_back(name, path);
  };
  for (const CallSetInfo& cs : vid.get_callsets()) {
    if (cs.m_filename.empty()) throw VCF2BinaryException("callset " + cs.m_name + " has no \"filename\"");
    add(cs.m_filename, (cs.m_filename[0] != '/' && !req.file_root.empty()) ? req.file_root + "/" + cs.m_filename : cs.m_filename);
  }
  for (const std::string& p : req.extra_paths) add(p, p);
  return files;
}

std::vector<SplitOutput> split_files_device(const VidMapper& vid, const SplitRequest& req, SplitStats* stats) {
  const double t0 = now_s();
  Splitter S(vid, req);
  // ---- the refusals: before the device is touched
  const size_t np = req.partitions.size();
  if (np == 0) throw VCF2BinaryException("split: no column partition");
  if (np > gdbsplit::kMaxPartitions) throw VCF2BinaryException("split: " + std::to_string(np) + " column partitions, at most " + std::to_string(gdbsplit::kMaxPartitions) + " are split in one run");
  S.sorted_to_index.resize(np);
  for (size_t i = 0; i < np; ++i) S.sorted_to_index[i] = (int)i;
  std::sort(S.sorted_to_index.begin(), S.sorted_to_index.end(), [&](int a, int b) { return req.partitions[(size_t)a].first < req.partitions[(size_t)b].first; });
  for (size_t i = 0; i < np; ++i) {
    const auto& r = req.partitions[(size_t)S.sorted_to_index[i]];
    if (r.first > r.second) throw VCF2BinaryException("split: column partition " + std::to_string(S.sorted_to_index[i]) + " ends in front of its begin");
    if (i && r.first <= S.ends.back()) throw VCF2BinaryException("split: column partitions " + std::to_string(S.sorted_to_index[i - 1]) + " and " + std::to_string(S.sorted_to_index[i]) + " overlap");
    S.begins.push_back(r.first);
    S.ends.push_back(r.second);
  }
  S.produce = req.produce;
  if (S.produce.empty()) for (size_t i = 0; i < np; ++i) S.produce.push_back((int)i);
  for (size_t i = 0; i < S.produce.size(); ++i) {
    if (S.produce[i] < 0 || (size_t)S.produce[i] >= np) throw VCF2BinaryException("split: partition index " + std::to_string(S.produce[i]) + " is not one of the " + std::to_string(np) + " column partitions");
    for (size_t k = 0; k < i; ++k) if (S.produce[k] == S.produce[i]) throw VCF2BinaryException("split: partition index " + std::to_string(S.produce[i]) + " is asked for twice");
  }
  const std::vector<std::pair<std::string, std::string>> files = split_input_files(vid, req);
  if (!req.single_output.empty() && (files.size() != 1 || S.produce.size() != 1))
    throw VCF2BinaryException("split: one output name needs exactly one input file and one partition");
  for (const auto& f : files) {
    if (vid.get_file_type(f.first) != GDB_FILE_VCF) throw VCF2BinaryException(f.second + " is a CSV cell file: only (g)VCF text files are split by this build");
    if (file_is_bcf2(f.second)) throw VCF2BinaryException(f.second + " is BCF2: only (g)VCF text files are split by this build");
  }
  if (req.text_budget_bytes) S.chunk = std::max<uint64_t>(std::min<uint64_t>(req.text_budget_bytes, kChunkBytes), 4096);

  ImportTextTap tap;
  tap.on_header = [&](const std::string& path, const std::string& head) { S.on_header(path, head); };
  tap.on_batch = [&](const ImportTextBatch& b) { S.on_batch(b); };
  ImportOptions opt;
  opt.file_root = req.file_root;
  {
    DeviceImporter imp(req.device, vid, opt, req.text_budget_bytes, req.inflate_mode, &tap);
    struct DropBuilders { Splitter& s; ~DropBuilders() { s.tbis.clear(); } } drop{S};      // (they wait on the importer's stream: gone before it is)
    for (const auto& f : files) {
      try {
        S.begin_file(f.first, f.second);
        imp.append_text_path(f.second);
        S.end_file();
      } catch (...) {
        S.abort_file();
        throw;
      }
    }
    const ImportStats& is = imp.stats();
    S.st.ms_index = is.ms_index; S.st.ms_inflate = is.ms_inflate; S.st.s_read = is.s_read; S.st.s_h2d = is.s_h2d;
  }
  S.st.s_total = now_s() - t0;
  if (stats) *stats = S.st;
  return S.done;
}

}  // namespace genomicsdb_amd
