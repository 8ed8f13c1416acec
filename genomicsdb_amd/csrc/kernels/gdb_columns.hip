// gdb_columns.hip - see gdb_columns.h.  Kernels for gfx950 around the bodies of core/gdb_columns.hpp, and their orchestration:
//   k_col_measure   one thread per record: the per-record table of the requested fields, the allele lengths, the per-field maxima
//   rocPRIM scan    allele lengths -> alleles_off
//   k_col_site      one thread per record: the site columns and the joined alleles
//   k_col_scatter   one thread per (record, sample) of one field, consecutive lanes on consecutive samples: the lanes of a wavefront
//                   read one contiguous piece of the record's FORMAT block and write one contiguous piece of out[r, :, :]
#include "gdb_columns.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <map>
#include <memory>

#include "../core/gdb_columns.hpp"
#include "gdb_import_device.hpp"

namespace genomicsdb_amd {

namespace {
using namespace gdbcol;
using impdev::DBuf;
using impdev::grid_for;
using impdev::kBlock;

// records [0, R) of the page: record r is page[rec_off[r] - base, rec_off[r + 1] - base)
struct ColPage { const uint8_t* bytes; uint64_t nbytes; const uint64_t* rec_off; uint64_t base; int64_t R; };

__global__ void __launch_bounds__(kBlock) k_col_measure(ColFields Q, ColPage P, int32_t n_sample, int32_t n_contig, ColEntry* E, ColRecord* rec, int64_t* alleles_len,
                                                        uint32_t* max_len, uint32_t* err, unsigned long long* bytes_read) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long bytes = 0;
  if (r < P.R) {
    const uint64_t rb = P.rec_off[r] - P.base, re = P.rec_off[r + 1] - P.base;
    ColFault f;
    uint64_t b = 0;
    if (rb > re || re > P.nbytes) {      // (never, by the pipeline's offsets: no read leaves the page)
      f.mask[0] = 1u; f.mask[1] = f.mask[2] = f.mask[3] = 0u;
      for (int32_t i = 0; i < Q.n; ++i) { ColEntry& e = E[r * Q.n + i]; e.off = 0; e.len = 0; e.type = 0; e.present = 0; e.pad[0] = e.pad[1] = 0; }
      rec[r].alleles_at = 0; rec[r].n_allele = 0; alleles_len[r] = 0;
    } else f = col_measure(Q, P.bytes, rb, re, n_sample, n_contig, E + r * Q.n, &rec[r], &alleles_len[r], max_len, &b);
    if (col_faulted(f)) col_raise(err, f, (uint32_t)r);
    bytes = b;
  }
  for (int o = 32; o; o >>= 1) bytes += __shfl_down(bytes, o, 64);
  if ((threadIdx.x & 63u) == 0u && bytes) atomicAdd(bytes_read, bytes);
}

__global__ void __launch_bounds__(kBlock) k_col_site(ColPage P, const ColRecord* rec, const int64_t* contig_off, ColSiteOut O) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r < P.R) col_site(P.bytes, P.rec_off[r] - P.base, rec[r], contig_off, r, O);
}

// N: samples of the field's rows (INFO: 1)
__global__ void __launch_bounds__(kBlock) k_col_scatter(ColField q, int field, int n_fields, const ColEntry* E, const uint8_t* page, int64_t R, int64_t N, uint32_t W, uint8_t* out,
                                                        uint8_t* phase, uint32_t* err) {
  const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (uint64_t)R * (uint64_t)N) return;
  const uint64_t r = idx / (uint64_t)N, s = idx - r * (uint64_t)N;
  const ColFault f = col_scatter(q, field, E[r * (uint64_t)n_fields + field], page, s, W, out + idx * W * col_dtype_size(q.dtype), q.is_gt ? phase + idx * W : nullptr);
  if (col_faulted(f)) col_raise(err, f, (uint32_t)r);
}

struct Resolved { ColumnRequest req; ColField f; };

std::string format_name(const HostPlan& hp) { return hp.plan.bcf_mode ? (hp.bgzf ? "b" : "bu") : (hp.bgzf ? "z" : ""); }

// "##FORMAT=<ID=x,Number=n,Type=t,..." -> kind, id, type
bool header_line(const std::string& l, std::string* kind, std::string* id, std::string* type) {
  if (l.compare(0, 2, "##") != 0) return false;
  const size_t eq = l.find("=<");
  if (eq == std::string::npos) return false;
  *kind = l.substr(2, eq - 2);
  auto value_of = [&](const char* key) {
    const std::string k = std::string(key) + "=";
    size_t at = eq + 2;
    while (true) {
      const size_t hit = l.find(k, at);
      if (hit == std::string::npos) return std::string();
      if (hit == eq + 2 || l[hit - 1] == ',') { const size_t e = l.find_first_of(",>", hit + k.size()); return l.substr(hit + k.size(), e == std::string::npos ? e : e - hit - k.size()); }
      at = hit + 1;
    }
  };
  *id = value_of("ID"); *type = value_of("Type");
  return !id->empty();
}
}  // namespace

struct RecordColumns::Impl {
  int device = 0;
  int32_t n_sample = 0, n_contig = 0;
  std::vector<Resolved> fields;
  ColFields Q;
  std::vector<int64_t> contig_off;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  DBuf<ColEntry> d_entry; DBuf<ColRecord> d_rec; DBuf<int64_t> d_alleles_len, d_alleles_off, d_contig_off;
  DBuf<uint32_t> d_err, d_max_len; DBuf<unsigned long long> d_bytes; DBuf<uint8_t> d_temp;
  std::vector<std::unique_ptr<DBuf<uint8_t>>> d_out;      // one block per column
  std::vector<RecordColumn> cols;
  bool device_ready = false;

  ~Impl() {
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
  void prepare_device() {
    if (device_ready) return;
    IMP_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) IMP_HIP_CHECK(hipEventCreate(&e));
    d_contig_off.ensure(std::max<size_t>(1, contig_off.size()));
    if (!contig_off.empty()) IMP_HIP_CHECK(hipMemcpy(d_contig_off.p, contig_off.data(), contig_off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    d_err.ensure(kColErrWords); d_max_len.ensure(kColMaxFields); d_bytes.ensure(1);
    device_ready = true;
  }
  // grows the blocks that are too small, after asking the device whether they fit (what they hold now comes back first)
  size_t growth_ = 0, released_ = 0;
  template <class T> void want(DBuf<T>& b, size_t n) { if (n > b.cap) { growth_ += n * sizeof(T); released_ += b.cap * sizeof(T); } }
  void check_fits(const char* what, int64_t R) {
    if (!growth_) return;
    size_t free_b = 0, total_b = 0;
    IMP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t need = growth_, back = released_;
    growth_ = released_ = 0;
    if (need > free_b + back)
      throw GenomicsDBDeviceException(std::string("record columns: the ") + what + " of a page of " + std::to_string(R) + " records x " + std::to_string(n_sample) + " samples take " +
                                      std::to_string(need) + " bytes, device " + std::to_string(device) + " has " + std::to_string(free_b) + " bytes free: use a smaller arena_bytes or fewer fields");
  }
  [[noreturn]] void raise(const uint32_t* err, const ColPage& P) {
    uint32_t r = 0; int kind = 0, field = 0;
    col_first_fault(err, &r, &kind, &field);
    uint64_t off[2] = {0, 0};
    uint32_t pos0 = 0;
    IMP_HIP_CHECK(hipMemcpy(off, P.rec_off + r, sizeof(off), hipMemcpyDeviceToHost));
    if (off[0] >= P.base && off[1] >= off[0] + 16 && off[1] - P.base <= P.nbytes) IMP_HIP_CHECK(hipMemcpy(&pos0, P.bytes + (off[0] - P.base) + 12, 4, hipMemcpyDeviceToHost));
    const bool whole = kind == COL_ERR_RECORD;
    throw GenomicsDBDeviceException(col_fault_text(kind, whole ? "" : fields[(size_t)field].req.name, whole ? 0 : Q.f[field].dtype, whole ? 0 : Q.f[field].width, (int64_t)(int32_t)pos0 + 1, r));
  }
};

RecordColumns::RecordColumns(const HostPlan& hp, int device, const std::vector<ColumnRequest>& requests) : m_(nullptr) {
  // ---- the refusals: before the device is touched
  if (!hp.plan.bcf_mode || hp.bgzf)
    throw UnsupportedOnDeviceException("record columns are decoded from BCF2 pages: the engine's output format is \"" + format_name(hp) + "\", create it with output format \"bu\"");
  if (hp.plan.use_missing_values_not_vector_end)
    throw UnsupportedOnDeviceException("record columns: the engine was created with use_missing_values_only_not_vector_end, whose pages hold missing values where a vector ends: "
                                       "the length of a vector could not be told from its padding");
  if (requests.size() > (size_t)kColMaxFields) throw UnsupportedOnDeviceException("record columns: " + std::to_string(requests.size()) + " fields asked for, at most " + std::to_string(kColMaxFields) + " at a time");
  // FORMAT / INFO ids of the header: dictionary index and Type
  struct Line { int idx; std::string type; };
  std::map<std::string, Line> format, info;
  for (size_t i = 0; i < hp.header_lines.size(); ++i) {
    std::string kind, id, type;
    if (hp.header_line_idx[i] < 0 || !header_line(hp.header_lines[i], &kind, &id, &type)) continue;
    if (kind == "FORMAT") format.emplace(id, Line{hp.header_line_idx[i], type});
    else if (kind == "INFO") info.emplace(id, Line{hp.header_line_idx[i], type});
  }
  std::unique_ptr<Impl> S(new Impl);
  S->device = device;
  memset(&S->Q, 0, sizeof(S->Q));
  for (const ColumnRequest& rq : requests) {
    const std::string& name = rq.name;
    for (const Resolved& o : S->fields) if (o.req.name == name) throw UnsupportedOnDeviceException("record columns: field " + name + " is asked for twice");
    if (name == "ID" || name == "FILTER") throw UnsupportedOnDeviceException("record columns: " + name + " is a column of strings, which this build does not decode into a tensor");
    std::string id = name;
    bool want_info = false, want_format = false;
    if (name.compare(0, 5, "INFO/") == 0) { id = name.substr(5); want_info = true; }
    else if (name.compare(0, 7, "FORMAT/") == 0) { id = name.substr(7); want_format = true; }
    const auto fi = format.find(id), ii = info.find(id);
    const bool is_format = !want_info && fi != format.end(), is_info = !is_format && !want_format && ii != info.end();
    if (!is_format && !is_info) throw UnsupportedOnDeviceException("record columns: " + name + " is neither a FORMAT nor an INFO id of the engine's header");
    const Line& line = is_format ? fi->second : ii->second;
    Resolved R;
    R.req = rq;
    memset(&R.f, 0, sizeof(R.f));
    R.f.key = line.idx; R.f.is_info = is_info ? 1 : 0; R.f.width = rq.width;
    R.f.is_gt = is_format && id == "GT";
    if (rq.width < 0) throw UnsupportedOnDeviceException("record columns: field " + name + ": width " + std::to_string(rq.width) + " is negative");
    if (R.f.is_gt || line.type == "Integer") {
      if (rq.dtype != RC_DEFAULT && rq.dtype != RC_INT8 && rq.dtype != RC_INT16 && rq.dtype != RC_INT32)
        throw UnsupportedOnDeviceException("record columns: field " + name + " holds integers: its dtype is int8, int16 or int32");
      R.f.dtype = rq.dtype == RC_DEFAULT ? RC_INT32 : rq.dtype;
    } else if (line.type == "Float") {
      if (rq.dtype != RC_DEFAULT && rq.dtype != RC_FLOAT32) throw UnsupportedOnDeviceException("record columns: field " + name + " holds floats: its dtype is float32");
      R.f.dtype = RC_FLOAT32; R.f.is_float = 1;
    } else if (line.type == "Flag") throw UnsupportedOnDeviceException("record columns: " + name + " is a Flag, which has no values to decode");
    else throw UnsupportedOnDeviceException("record columns: " + name + " is a string field (Type=" + line.type + "), which this build does not decode into a tensor");
    S->Q.f[S->Q.n++] = R.f;
    S->fields.push_back(R);
  }
  S->n_sample = hp.plan.bcf_n_sample;
  for (const GdbContig& c : hp.contigs) S->n_contig = std::max(S->n_contig, c.rid + 1);
  S->contig_off.assign((size_t)S->n_contig, 0);
  for (const GdbContig& c : hp.contigs) if (c.rid >= 0) S->contig_off[(size_t)c.rid] = c.offset;
  m_ = S.release();
}

RecordColumns::~RecordColumns() { delete m_; }

const std::vector<RecordColumn>& RecordColumns::decode(const DevicePipeline::PageView& page, ColumnsStats* stats) {
  Impl& S = *m_;
  if (!page.valid || !page.page || !page.rec_off) throw GenomicsDBDeviceException("record columns: there is no page: ask for one with next_page first");
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: the column decoder has no CPU fallback");
  IMP_HIP_CHECK(hipSetDevice(S.device));
  S.prepare_device();
  const hipStream_t st = S.stream;
  const int64_t R = page.last - page.first, N = S.n_sample;
  const int F = S.Q.n;
  if (R < 0 || R >= (int64_t)0xFFFFFFFFll) throw GenomicsDBDeviceException("record columns: a page of " + std::to_string(R) + " records: use a smaller arena_bytes");
  const ColPage P{(const uint8_t*)page.page, page.nbytes, page.rec_off + page.first, page.base, R};
  ColumnsStats cs;
  cs.records = R; cs.n_fields = F;
  // ---- measure + scan
  S.want(S.d_entry, (size_t)R * std::max(F, 1) + 1); S.want(S.d_rec, (size_t)R + 1); S.want(S.d_alleles_len, (size_t)R + 1); S.want(S.d_alleles_off, (size_t)R + 1);
  size_t temp_bytes = 0;
  IMP_HIP_CHECK(rocprim::exclusive_scan(nullptr, temp_bytes, S.d_alleles_len.p, S.d_alleles_off.p, (int64_t)0, (size_t)R + 1, rocprim::plus<int64_t>(), st));
  S.want(S.d_temp, temp_bytes + 1);
  S.check_fits("per-record tables", R);
  S.d_entry.ensure((size_t)R * std::max(F, 1) + 1); S.d_rec.ensure((size_t)R + 1); S.d_alleles_len.ensure((size_t)R + 1); S.d_alleles_off.ensure((size_t)R + 1); S.d_temp.ensure(temp_bytes + 1);
  uint32_t h_err[kColErrWords], h_max[kColMaxFields];
  for (int i = 0; i < kColErrWords; ++i) h_err[i] = i ? 0xFFFFFFFFu : 0u;
  for (int i = 0; i < kColMaxFields; ++i) h_max[i] = 1u;      // (a column has one element at least)
  IMP_HIP_CHECK(hipMemcpyAsync(S.d_err.p, h_err, sizeof(h_err), hipMemcpyHostToDevice, st));
  IMP_HIP_CHECK(hipMemcpyAsync(S.d_max_len.p, h_max, sizeof(h_max), hipMemcpyHostToDevice, st));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_bytes.p, 0, sizeof(unsigned long long), st));
  IMP_HIP_CHECK(hipMemsetAsync(S.d_alleles_len.p + R, 0, sizeof(int64_t), st));
  IMP_HIP_CHECK(hipEventRecord(S.ev[0], st));
  if (R) hipLaunchKernelGGL(k_col_measure, dim3(grid_for((uint64_t)R)), dim3(kBlock), 0, st, S.Q, P, (int32_t)N, S.n_contig, S.d_entry.p, S.d_rec.p, S.d_alleles_len.p, S.d_max_len.p, S.d_err.p, S.d_bytes.p);
  IMP_HIP_CHECK(rocprim::exclusive_scan((void*)S.d_temp.p, temp_bytes, S.d_alleles_len.p, S.d_alleles_off.p, (int64_t)0, (size_t)R + 1, rocprim::plus<int64_t>(), st));
  IMP_HIP_CHECK(hipEventRecord(S.ev[1], st));
  int64_t alleles_total = 0;
  unsigned long long bytes_read = 0;
  IMP_HIP_CHECK(hipMemcpyAsync(h_err, S.d_err.p, sizeof(h_err), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipMemcpyAsync(h_max, S.d_max_len.p, sizeof(h_max), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipMemcpyAsync(&alleles_total, S.d_alleles_off.p + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipMemcpyAsync(&bytes_read, S.d_bytes.p, sizeof(bytes_read), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipStreamSynchronize(st));
  if (h_err[0]) S.raise(h_err, P);
  cs.bytes_read = bytes_read;
  // ---- the columns: name, dtype, shape; blocks grown on demand
  S.cols.clear();
  auto add = [&](const std::string& name, int dtype, int ndim, int64_t a, int64_t b, int64_t c) {
    RecordColumn col; col.name = name; col.dtype = dtype; col.ndim = ndim; col.shape[0] = a; col.shape[1] = ndim > 1 ? b : 0; col.shape[2] = ndim > 2 ? c : 0;
    S.cols.push_back(col);
  };
  add("contig", RC_INT32, 1, R, 1, 1); add("pos", RC_INT64, 1, R, 1, 1); add("end", RC_INT64, 1, R, 1, 1); add("column", RC_INT64, 1, R, 1, 1);
  add("qual", RC_FLOAT32, 1, R, 1, 1); add("n_allele", RC_INT32, 1, R, 1, 1); add("alleles", RC_UINT8, 1, alleles_total, 1, 1); add("alleles_off", RC_INT64, 1, R + 1, 1, 1);
  std::vector<int> field_col((size_t)F, 0);
  for (int i = 0; i < F; ++i) {
    const ColField& q = S.Q.f[i];
    const int64_t W = q.width > 0 ? q.width : (int64_t)h_max[i];
    cs.width[i] = (int32_t)W;
    field_col[(size_t)i] = (int)S.cols.size();
    if (q.is_info) add(S.fields[(size_t)i].req.name, q.dtype, 2, R, W, 1); else add(S.fields[(size_t)i].req.name, q.dtype, 3, R, N, W);
    if (q.is_gt) add(S.fields[(size_t)i].req.name + "_phase", RC_UINT8, 3, R, N, W);
  }
  while (S.d_out.size() < S.cols.size()) S.d_out.emplace_back(new DBuf<uint8_t>);
  std::vector<size_t> nbytes(S.cols.size());
  for (size_t c = 0; c < S.cols.size(); ++c) {
    const RecordColumn& col = S.cols[c];
    if (c == 7) { nbytes[c] = 0; continue; }      // alleles_off is the scan's output
    const uint64_t n = (uint64_t)col.shape[0] * (uint64_t)(col.ndim > 1 ? col.shape[1] : 1) * (uint64_t)(col.ndim > 2 ? col.shape[2] : 1);
    nbytes[c] = (size_t)n * col_dtype_size(col.dtype);
    cs.bytes_written += nbytes[c];
    S.want(*S.d_out[c], nbytes[c] + 16);
  }
  cs.bytes_written += (uint64_t)(R + 1) * sizeof(int64_t);
  S.check_fits("columns", R);
  for (size_t c = 0; c < S.cols.size(); ++c) {
    if (c == 7) { S.cols[c].dev_ptr = S.d_alleles_off.p; continue; }
    S.d_out[c]->ensure(nbytes[c] + 16);
    S.cols[c].dev_ptr = S.d_out[c]->p;
  }
  // ---- site
  IMP_HIP_CHECK(hipEventRecord(S.ev[2], st));
  const ColSiteOut so{(int32_t*)S.cols[0].dev_ptr, (int64_t*)S.cols[1].dev_ptr, (int64_t*)S.cols[2].dev_ptr, (int64_t*)S.cols[3].dev_ptr, (uint32_t*)S.cols[4].dev_ptr,
                      (int32_t*)S.cols[5].dev_ptr, (uint8_t*)S.cols[6].dev_ptr, (const int64_t*)S.d_alleles_off.p};
  if (R) hipLaunchKernelGGL(k_col_site, dim3(grid_for((uint64_t)R)), dim3(kBlock), 0, st, P, (const ColRecord*)S.d_rec.p, (const int64_t*)S.d_contig_off.p, so);
  IMP_HIP_CHECK(hipEventRecord(S.ev[3], st));
  // ---- scatter: one launch per field
  for (int i = 0; i < F; ++i) {
    const ColField& q = S.Q.f[i];
    const int64_t rows = q.is_info ? 1 : N;
    const uint64_t threads = (uint64_t)R * (uint64_t)rows;
    if (!threads) continue;
    if ((threads + kBlock - 1) / kBlock > 0x7FFFFFFFull) throw GenomicsDBDeviceException("record columns: a page of " + std::to_string(R) + " records: use a smaller arena_bytes");
    const int c = field_col[(size_t)i];
    hipLaunchKernelGGL(k_col_scatter, dim3(grid_for(threads)), dim3(kBlock), 0, st, q, i, F, (const ColEntry*)S.d_entry.p, P.bytes, R, rows, (uint32_t)cs.width[i], (uint8_t*)S.cols[(size_t)c].dev_ptr,
                       q.is_gt ? (uint8_t*)S.cols[(size_t)c + 1].dev_ptr : (uint8_t*)nullptr, S.d_err.p);
  }
  IMP_HIP_CHECK(hipEventRecord(S.ev[4], st));
  IMP_HIP_CHECK(hipMemcpyAsync(h_err, S.d_err.p, sizeof(h_err), hipMemcpyDeviceToHost, st));
  IMP_HIP_CHECK(hipStreamSynchronize(st));
  IMP_HIP_CHECK(hipGetLastError());
  if (h_err[0]) S.raise(h_err, P);
  IMP_HIP_CHECK(hipEventElapsedTime(&cs.ms_measure, S.ev[0], S.ev[1]));
  IMP_HIP_CHECK(hipEventElapsedTime(&cs.ms_site, S.ev[2], S.ev[3]));
  IMP_HIP_CHECK(hipEventElapsedTime(&cs.ms_scatter, S.ev[3], S.ev[4]));
  if (stats) *stats = cs;
  return S.cols;
}

}  // namespace genomicsdb_amd
