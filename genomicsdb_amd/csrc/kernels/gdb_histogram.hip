// gdb_histogram.hip - see gdb_histogram.h.  Kernels for gfx950 around the bodies of core/gdb_histogram.hpp, and their orchestration.
#include "gdb_histogram.h"

#include <hip/hip_runtime.h>

#include <cstring>

#include "../core/gdb_histogram.hpp"
#include "../host/import_common.hpp"
#include "gdb_import.h"
#include "gdb_import_device.hpp"

namespace genomicsdb_amd {

namespace {
using namespace gdbimp;
using namespace gdbhist;
using namespace impdev;

// tally: [0] record lines / records seen, [1] counted, [2] atomicAdds on the counters
struct HistOut { unsigned long long* counts; unsigned long long* tally; uint32_t* err; };

// The end of both kernels, reached by every lane of the wavefront.  A file is sorted by column within a contig, so neighbouring
// lanes mostly agree on the bin: the first lane of a run of equal bins adds run_length * weight (as k_column_histogram does for
// the cells of an array).
__device__ __forceinline__ void hist_commit(const HistSel s, bool valid, uint32_t idx, const HistParams& P, unsigned long long weight, const HistOut& O) {
  const uint32_t lane = threadIdx.x & 63u;
  if (valid && s.err) imp_raise(O.err, s.err, idx);
  const bool counted = valid && !s.err && s.counted && s.bin < P.num_bins;      // (bin < num_bins always, by the range check: nothing is added outside the counters)
  const uint64_t key = counted ? s.bin : ~0ull;
  const uint64_t prev = __shfl_up(key, 1, 64);
  const bool head = lane == 0u || prev != key;
  const unsigned long long heads = __ballot(head);
  const bool issue = head && counted;
  if (issue) {
    const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const unsigned long long run = above ? (unsigned long long)__builtin_ctzll(above) + 1ull : 64ull - lane;
    atomicAdd(&O.counts[key], run * weight);
  }
  const unsigned long long rec = __ballot(valid && s.record), cnt = __ballot(counted), iss = __ballot(issue);
  if (lane == 0u) {
    if (rec) atomicAdd(&O.tally[0], (unsigned long long)__popcll(rec));
    if (cnt) atomicAdd(&O.tally[1], (unsigned long long)__popcll(cnt));
    if (iss) atomicAdd(&O.tally[2], (unsigned long long)__popcll(iss));
  }
}

// one thread per line of a text batch
__global__ void __launch_bounds__(kBlock) k_hist_lines(ImpTables T, ImpBatch B, HistParams P, unsigned long long weight, HistOut O) {
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = line < B.n_lines;
  HistSel s; s.bin = 0; s.err = 0; s.record = 0; s.counted = 0;
  if (valid) s = hist_line(T, P, imp_line_of(B, line));
  hist_commit(s, valid, line, P, weight, O);
}

// one thread per record of a BCF2 batch
__global__ void __launch_bounds__(kBlock) k_hist_records(ImpBcfTables BT, const uint8_t* bytes, uint32_t n_bytes, const uint32_t* rec_off, uint32_t n_rec, HistParams P,
                                                        unsigned long long weight, HistOut O) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = r < n_rec;
  HistSel s; s.bin = 0; s.err = 0; s.record = 0; s.counted = 0;
  if (valid) {
    uint32_t b = rec_off[r], e = rec_off[r + 1u];
    if (e > n_bytes) e = n_bytes;       // (never, by the host's walk: no read leaves the batch)
    if (b > e) b = e;
    s = hist_bcf_record(BT, P, bytes, b, e);
  }
  hist_commit(s, valid, r, P, weight, O);
}

struct Histogrammer {
  const InputHistogramRequest& req;
  HistParams P;
  InputHistogramStats st;
  hipEvent_t ev[2] = {nullptr, nullptr};
  DBuf<unsigned long long> d_counts, d_tally;
  DBuf<uint32_t> d_err;
  unsigned long long weight = 0;      // of the file that is being read

  explicit Histogrammer(const InputHistogramRequest& r) : req(r) {
    P = hist_params((uint64_t)r.max_histogram_range, r.num_bins, r.column_begin, r.column_end);
  }
  ~Histogrammer() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }

  void allocate() {
    size_t free_b = 0, total_b = 0;
    IMP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (P.num_bins > (uint64_t)free_b / sizeof(unsigned long long))
      throw VCF2BinaryException("histogram: " + std::to_string(P.num_bins) + " bins of 8 bytes do not fit in the " + std::to_string(free_b) + " bytes that device " +
                                std::to_string(req.device) + " has free");
    d_counts.ensure((size_t)P.num_bins);
    d_tally.ensure(4);
    d_err.ensure(kErrWords);
    IMP_HIP_CHECK(hipMemset(d_counts.p, 0, (size_t)P.num_bins * sizeof(unsigned long long)));
    IMP_HIP_CHECK(hipMemset(d_tally.p, 0, 4 * sizeof(unsigned long long)));
    IMP_HIP_CHECK(hipDeviceSynchronize());      // (the kernels run on the importer's stream)
    for (auto& e : ev) IMP_HIP_CHECK(hipEventCreate(&e));
  }

  // what both kinds of batch share: the error words in front of the kernel, the time and the errors behind it
  template <class Launch, class Describe>
  void run_batch(hipStream_t stream, const std::string& path, const char* unit, int64_t before, const Describe& describe, const Launch& launch) {
    ++st.num_batches;
    IMP_HIP_CHECK(hipMemsetAsync(d_err.p, 0, sizeof(uint32_t), stream));
    IMP_HIP_CHECK(hipMemsetAsync(d_err.p + 1, 0xFF, (kErrWords - 1) * sizeof(uint32_t), stream));
    IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
    launch(HistOut{d_counts.p, d_tally.p, d_err.p});
    IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
    uint32_t err[kErrWords];
    IMP_HIP_CHECK(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0;
    IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_histogram += ms;
    // ---- errors: the smallest offending line / record speaks
    uint32_t at = UINT32_MAX, bit = 0;
    for (int k = 0; k < kErrWords - 1; ++k) if ((err[0] & (1u << k)) && err[1 + k] < at) { at = err[1 + k]; bit = 1u << k; }
    if (!bit) return;
    const std::string where = path + " " + unit + " " + std::to_string(before + (int64_t)at + 1);
    if (bit == IMP_ERR_HIST_RANGE)
      throw VCF2BinaryException("a column outside the range of the histogram [0," + std::to_string(P.hi) + "] (" + where + ")");
    std::string words;
    try { words = describe(bit, at); }
    catch (const VCF2BinaryException& e) {      // the host parser's own words for a POS / END it refuses too: they name no line, so it is added
      words = e.what();
      if (words.compare(0, strlen("VCF2BinaryException : "), "VCF2BinaryException : ") == 0) words = words.substr(strlen("VCF2BinaryException : "));
      words += " (" + where + ")";
    }
    throw VCF2BinaryException(words);
  }

  void on_batch(const ImportTextBatch& b) {
    const hipStream_t stream = (hipStream_t)b.stream;
    run_batch(stream, *b.path, "line", b.lines_before, b.describe, [&](const HistOut& O) {
      hipLaunchKernelGGL(k_hist_lines, dim3(grid_for(b.n_lines)), dim3(kBlock), 0, stream, *b.tables, ImpBatch{b.d_text, b.d_nl, b.d_first_tab, b.d_tab, b.n_lines}, P, weight, O);
    });
  }
  void on_records(const ImportRecordBatch& b) {
    const hipStream_t stream = (hipStream_t)b.stream;
    run_batch(stream, *b.path, "record", b.records_before, b.describe, [&](const HistOut& O) {
      hipLaunchKernelGGL(k_hist_records, dim3(grid_for(b.n_rec)), dim3(kBlock), 0, stream, *b.bcf_tables, b.d_bytes, b.n_bytes, b.d_rec_off, b.n_rec, P, weight, O);
    });
  }
};

}  // namespace

std::vector<uint64_t> input_histogram_device(const VidMapper& vid, const InputHistogramRequest& req, InputHistogramStats* stats) {
  const double t0 = now_s();
  // ---- the refusals: before the device is touched
  if (req.num_bins == 0) throw VCF2BinaryException("histogram: num_bins is 0");
  if (req.max_histogram_range < 0) throw VCF2BinaryException("histogram: max_histogram_range " + std::to_string(req.max_histogram_range) + " is negative");
  if (req.num_bins > ((uint64_t)1 << 60)) throw VCF2BinaryException("histogram: " + std::to_string(req.num_bins) + " bins are more than a device holds");
  if (!vid.is_initialized() || !vid.is_callset_mapping_initialized()) throw VCF2BinaryException("vid and callset mappings are needed");
  ImportOptions opt;
  opt.file_root = req.file_root;
  opt.row_begin = req.row_begin; opt.row_end = req.row_end;
  const std::vector<ImportFile> files = import_files(vid, with_clamped_row_bounds(opt, vid));
  for (const ImportFile& f : files)
    if (f.type != GDB_FILE_VCF) throw VCF2BinaryException(f.path + " is a CSV cell file: only (g)VCF text and BCF2 files are counted by this build");
  for (const ImportStream& s : req.streams) {
    bool used = false;
    for (const CallSetInfo& cs : vid.get_callsets()) used = used || cs.m_filename == s.name;
    if (!used) throw VCF2BinaryException("stream " + s.name + " is not a \"filename\" of the callset mapping");
  }
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the input histogram has no CPU fallback");
  IMP_HIP_CHECK(hipSetDevice(req.device));
  Histogrammer S(req);
  S.allocate();

  ImportTextTap tap;
  tap.on_batch = [&](const ImportTextBatch& b) { S.on_batch(b); };
  tap.on_records = [&](const ImportRecordBatch& b) { S.on_records(b); };
  {
    DeviceImporter imp(req.device, vid, opt, req.text_budget_bytes, req.inflate_mode, &tap);
    for (const ImportFile& f : files) {
      S.weight = (unsigned long long)f.callsets.size();
      const ImportStream* from = nullptr;
      for (const ImportStream& s : req.streams) if (s.name == f.name) from = &s;
      if (from) imp.append_buffer(f.name, from->data, from->nbytes);
      else imp.append_file(f.name);
    }
    const ImportStats& is = imp.stats();
    S.st.num_files = is.num_files;
    S.st.ms_index = is.ms_index; S.st.ms_inflate = is.ms_inflate; S.st.s_read = is.s_read; S.st.s_h2d = is.s_h2d;
  }
  // ---- the counters leave the device once
  std::vector<uint64_t> counts((size_t)req.num_bins);
  unsigned long long tally[4];
  IMP_HIP_CHECK(hipMemcpy(counts.data(), S.d_counts.p, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  IMP_HIP_CHECK(hipMemcpy(tally, S.d_tally.p, sizeof(tally), hipMemcpyDeviceToHost));
  S.st.num_records = (int64_t)tally[0]; S.st.num_counted = (int64_t)tally[1]; S.st.num_atomics = (int64_t)tally[2];
  for (const uint64_t c : counts) S.st.total_weight += c;
  S.st.s_total = now_s() - t0;
  if (stats) *stats = S.st;
  return counts;
}

}  // namespace genomicsdb_amd
