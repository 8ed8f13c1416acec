// gdb_vcfdiff.hip - see gdb_vcfdiff.h.  Kernels for gfx950 around the bodies of core/gdb_vcfdiff.hpp, and their orchestration.
#include "gdb_vcfdiff.h"

#include <hip/hip_runtime.h>
#include <zlib.h>

#include <cstring>

#include "../common/mini_json.hpp"
#include "../core/gdb_vcfdiff.hpp"
#include "../host/import_bcf.hpp"
#include "../host/import_common.hpp"
#include "../host/vcfdiff_common.hpp"
#include "gdb_import.h"
#include "gdb_import_device.hpp"

namespace genomicsdb_amd {

namespace {
using namespace gdbimp;
using namespace gdbvdiff;
using namespace vdhost;
using namespace impdev;

constexpr uint32_t kHeavyCap = 4096;          // tokens of one sample's vector that the cooperative path indexes in LDS; longer ones are walked by one lane
constexpr uint32_t kHeavySlices = 64;         // blocks per heavy pair: the samples are dealt out among them
constexpr uint32_t kPairsPerLaunch = 1u << 20;

struct VdLineRef { const char* text; const uint32_t* tabs; uint32_t begin, end, ntabs, pos_equal; };      // pos_equal: of the pair (in the gold ref)
struct VdPair { VdLineRef g, t; };
struct VdOut { uint32_t flags, heavy; unsigned long long info[4], fmt[4]; };

__device__ __forceinline__ ImpLine line_of(const VdLineRef& r) {
  ImpLine L; L.text = r.text; L.begin = r.begin; L.end = r.end; L.tabs = r.tabs; L.ntabs = r.ntabs;
  return L;
}

// one thread per line of a text batch
__global__ void __launch_bounds__(kBlock) k_vdiff_keys(VdTables T, int file, ImpBatch B, VdKey* keys) {
  const uint32_t line = blockIdx.x * kBlock + threadIdx.x;
  if (line >= B.n_lines) return;
  VdKey K = vd_keys(T, file, imp_line_of(B, line));
  K.tab_first = B.line_first_tab[line];
  keys[line] = K;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

// one workgroup per pair: the site part by one lane into LDS, then one lane per gold sample (the light path).  A pair for the
// cooperative path is only listed here: its FORMAT words are written as 0 and k_vdiff_heavy ORs into them
__global__ void __launch_bounds__(kBlock) k_vdiff_compare(VdTables T, const VdPair* pairs, uint32_t n_pairs, uint32_t pair_base, VdOut* out, uint32_t* heavy_list,
                                                         uint32_t* counters, VdDeferred* def, uint32_t def_cap) {
  __shared__ VdSite S;
  __shared__ unsigned long long acc[4];
  const uint32_t p = blockIdx.x;
  if (p >= n_pairs) return;
  const ImpLine G = line_of(pairs[p].g), Tt = line_of(pairs[p].t);
  const VdDefer D{def, &counters[1], def_cap, pair_base + p, true};
  if (threadIdx.x == 0) {
    vd_site(T, G, Tt, pairs[p].g.pos_equal != 0u, D, S);
    for (int m = 0; m < 4; ++m) acc[m] = 0ull;
  }
  __syncthreads();
  const bool heavy = vd_is_heavy(S);
  if (!heavy && S.has_fmt) {
    VdMasks M; for (int m = 0; m < 4; ++m) M.m[m] = 0ull;
    const VdLane lane;
    for (uint32_t j = threadIdx.x; j < (uint32_t)T.n_samples; j += blockDim.x) {
      const VdMasks one = vd_sample(lane, T, G, Tt, S, j, D, nullptr, nullptr, 0u);
      for (int m = 0; m < 4; ++m) M.m[m] |= one.m[m];
    }
    for (int m = 0; m < 4; ++m) {
      const unsigned long long w = wave_or(M.m[m]);
      if ((threadIdx.x & 63u) == 0u && w) atomicOr(&acc[m], w);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    VdOut o;
    o.flags = S.flags; o.heavy = heavy ? 1u : 0u;
    for (int m = 0; m < 4; ++m) { o.info[m] = S.info[m]; o.fmt[m] = acc[m]; }
    out[p] = o;
    if (heavy) heavy_list[atomicAdd(&counters[0], 1u)] = p;
  }
}

// the lanes of one wavefront (a workgroup of 64) share a vector
struct VdWave {
  static constexpr bool kIndexed = true;
  __device__ uint32_t lane() const { return threadIdx.x & 63u; }
  __device__ uint32_t lanes() const { return 64u; }
  __device__ bool any(bool x) const { return __ballot(x) != 0ull; }
  // offs[k] = begin of token k, offs[n] = t.e + 1: the commas of 64 bytes by __ballot, their places by a prefix popcount
  __device__ uint32_t index(const char* text, ImpTok t, uint32_t* offs, uint32_t cap) const {
    __syncthreads();      // (the readers of the last index are done)
    const uint32_t l = lane();
    uint32_t n = 0;
    if (l == 0u) offs[0] = t.b;
    for (uint32_t base = t.b; base < t.e; base += 64u) {
      const uint32_t i = base + l;
      const bool comma = i < t.e && text[i] == ',';
      const unsigned long long mask = __ballot(comma);
      if (comma) {
        const uint32_t at = n + (uint32_t)__popcll(mask & ((1ull << l) - 1ull)) + 1u;
        if (at < cap) offs[at] = i + 1u;
      }
      n += (uint32_t)__popcll(mask);
    }
    ++n;
    if (l == 0u && n < cap) offs[n] = t.e + 1u;
    __syncthreads();
    return n;
  }
};

// the cooperative path: block (h, s) takes the samples s, s + gridDim.y, ... of heavy pair h, one wavefront per sample
__global__ void __launch_bounds__(64) k_vdiff_heavy(VdTables T, const VdPair* pairs, const uint32_t* heavy_list, uint32_t n_heavy, uint32_t pair_base, VdOut* out,
                                                   uint32_t* counters, VdDeferred* def, uint32_t def_cap) {
  __shared__ VdSite S;
  __shared__ uint32_t goffs[kHeavyCap], toffs[kHeavyCap];
  if (blockIdx.x >= n_heavy) return;
  const uint32_t p = heavy_list[blockIdx.x];
  const ImpLine G = line_of(pairs[p].g), Tt = line_of(pairs[p].t);
  VdDefer D{def, &counters[1], def_cap, pair_base + p, false};      // the site's own deferred tokens were listed by k_vdiff_compare
  if (threadIdx.x == 0) vd_site(T, G, Tt, pairs[p].g.pos_equal != 0u, D, S);
  __syncthreads();
  D.active = true;
  VdMasks M; for (int m = 0; m < 4; ++m) M.m[m] = 0ull;
  const VdWave wave;
  for (uint32_t j = blockIdx.y; j < (uint32_t)T.n_samples; j += gridDim.y) {
    const VdMasks one = vd_sample(wave, T, G, Tt, S, j, D, goffs, toffs, kHeavyCap);
    for (int m = 0; m < 4; ++m) M.m[m] |= one.m[m];
  }
  if (threadIdx.x == 0)
    for (int m = 0; m < 4; ++m) if (M.m[m]) atomicOr(&out[p].fmt[m], M.m[m]);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the lines in front of the first record line, through zlib (plain, gzip and BGZF alike)
std::string read_head(const std::string& path) {
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) throw VCFDiffException("cannot open " + path);
  std::string head;
  std::vector<char> buf(1 << 16);
  size_t line_start = 0;
  bool complete = false;
  while (!complete) {
    const int n = gzread(f, buf.data(), (unsigned)buf.size());
    if (n <= 0) break;
    head.append(buf.data(), (size_t)n);
    for (;;) {
      const size_t nl = head.find('\n', line_start);
      const size_t e = nl == std::string::npos ? head.size() : nl;
      size_t ln = e - line_start;
      if (ln && head[e - 1] == '\r') --ln;
      if (ln && head[line_start] != '#') { complete = true; break; }
      if (nl == std::string::npos) break;
      line_start = nl + 1;
    }
  }
  gzclose(f);
  return head.substr(0, line_start);
}

struct ResidentBatch { char* text = nullptr; uint32_t* tabs = nullptr; };

struct Differ {
  const VcfDiffRequest& req;
  VcfDiffStats st;
  VdTablesHost H;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t stream = nullptr;
  DBuf<char> d_names;
  DBuf<VdName> d_contigs[2];
  DBuf<VdField> d_info, d_fmt;
  DBuf<int32_t> d_sample_map;
  DBuf<VdKey> d_keys;
  std::vector<ResidentBatch> batches;
  std::vector<VdRecord> lines[2];      // every line of a file, in order
  int file = 0;

  explicit Differ(const VcfDiffRequest& r) : req(r) {}
  ~Differ() {
    for (ResidentBatch& b : batches) { if (b.text) (void)hipFree(b.text); if (b.tabs) (void)hipFree(b.tabs); }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  }

  VdTables tables() const {
    VdTables T = H.view(req.threshold);
    T.names = d_names.p;
    for (int f = 0; f < 2; ++f) T.contigs[f] = d_contigs[f].p;
    T.info = d_info.p; T.fmt = d_fmt.p; T.sample_map = d_sample_map.p;
    return T;
  }
  void upload_tables() {
    auto up = [&](auto& buf, const auto* src, size_t n) {
      buf.ensure(std::max<size_t>(n, 1));
      if (n) IMP_HIP_CHECK(hipMemcpy(buf.p, src, n * sizeof(*src), hipMemcpyHostToDevice));
    };
    up(d_names, H.names.data(), H.names.size());
    for (int f = 0; f < 2; ++f) up(d_contigs[f], H.contigs[f].data(), H.contigs[f].size());
    up(d_info, H.info.data(), H.info.size());
    up(d_fmt, H.fmt.data(), H.fmt.size());
    up(d_sample_map, H.sample_map.data(), H.sample_map.size());
    for (auto& e : ev) IMP_HIP_CHECK(hipEventCreate(&e));
  }

  // pass 1: the keys of a batch's lines; its text and tab index stay resident
  void on_batch(const ImportTextBatch& b) {
    stream = (hipStream_t)b.stream;
    ++st.num_batches;
    uint32_t n_tabs = 0;
    IMP_HIP_CHECK(hipMemcpyAsync(&n_tabs, b.d_first_tab + b.n_lines, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t need = (uint64_t)b.n_bytes + kTextPad + (uint64_t)std::max<uint32_t>(n_tabs, 1u) * sizeof(uint32_t) + (uint64_t)b.n_lines * sizeof(VdKey);
    size_t free_b = 0, total_b = 0;
    IMP_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need > (uint64_t)free_b)
      throw VCFDiffException("the text of both files does not fit on device " + std::to_string(req.device) + ": " + std::to_string(st.resident_bytes) + " bytes are resident, the next batch of " +
                             *b.path + " needs " + std::to_string(need) + " and " + std::to_string(free_b) + " are free (a streamed test file is not in this build)");
    ResidentBatch rb;
    batches.push_back(rb);
    ResidentBatch& R = batches.back();
    IMP_HIP_CHECK(hipMalloc((void**)&R.text, (size_t)b.n_bytes + kTextPad));
    IMP_HIP_CHECK(hipMalloc((void**)&R.tabs, (size_t)std::max<uint32_t>(n_tabs, 1u) * sizeof(uint32_t)));
    st.resident_bytes += (uint64_t)b.n_bytes + kTextPad + (uint64_t)std::max<uint32_t>(n_tabs, 1u) * sizeof(uint32_t);
    IMP_HIP_CHECK(hipMemcpyAsync(R.text, b.d_text, (size_t)b.n_bytes + kTextPad, hipMemcpyDeviceToDevice, stream));
    if (n_tabs) IMP_HIP_CHECK(hipMemcpyAsync(R.tabs, b.d_tab, (size_t)n_tabs * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    d_keys.ensure(b.n_lines);
    IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(k_vdiff_keys, dim3(grid_for(b.n_lines)), dim3(kBlock), 0, stream, tables(), file, ImpBatch{b.d_text, b.d_nl, b.d_first_tab, b.d_tab, b.n_lines}, d_keys.p);
    IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
    std::vector<VdKey> keys(b.n_lines);
    IMP_HIP_CHECK(hipMemcpyAsync(keys.data(), d_keys.p, keys.size() * sizeof(VdKey), hipMemcpyDeviceToHost, stream));
    IMP_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0;
    IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_keys += ms;
    for (uint32_t i = 0; i < b.n_lines; ++i) {
      VdRecord r; r.key = keys[i]; r.line_no = b.lines_before + (int64_t)i + 1; r.batch = (uint32_t)batches.size() - 1u;
      lines[file].push_back(r);
    }
  }

  std::string line_text(const VdRecord& r) const {
    std::string s((size_t)(r.key.stop - r.key.begin), '\0');
    if (!s.empty()) IMP_HIP_CHECK(hipMemcpy(&s[0], batches[r.batch].text + r.key.begin, s.size(), hipMemcpyDeviceToHost));
    return s;
  }
  VdLineRef ref_of(const VdRecord& r) const {
    VdLineRef l;
    l.text = batches[r.batch].text; l.tabs = batches[r.batch].tabs + r.key.tab_first; l.begin = r.key.begin; l.end = r.key.stop; l.ntabs = r.key.ntabs; l.pos_equal = 0;
    return l;
  }

  // pass 2 over the pairs of `ev`
  void compare(std::vector<VdEvent>& events, const std::vector<VdRecord>& gold, const std::vector<VdRecord>& test) {
    std::vector<size_t> of_pair;
    for (size_t k = 0; k < events.size(); ++k) if (events[k].pair >= 0) of_pair.push_back(k);
    st.pairs_compared = (int64_t)of_pair.size();
    if (of_pair.empty()) return;
    if (!stream) IMP_HIP_CHECK(hipStreamCreate(&stream));
    const VdTables T = tables();
    DBuf<VdPair> d_pairs; DBuf<VdOut> d_out; DBuf<uint32_t> d_heavy, d_counters; DBuf<VdDeferred> d_def;
    uint32_t def_cap = 1u << 16;
    d_counters.ensure(2);
    d_def.ensure(def_cap);
    for (size_t base = 0; base < of_pair.size(); base += kPairsPerLaunch) {
      const uint32_t n = (uint32_t)std::min<size_t>(kPairsPerLaunch, of_pair.size() - base);
      std::vector<VdPair> pairs(n);
      for (uint32_t i = 0; i < n; ++i) {
        const VdEvent& e = events[of_pair[base + i]];
        pairs[i].g = ref_of(gold[(size_t)e.g]); pairs[i].t = ref_of(test[(size_t)e.t]);
        pairs[i].g.pos_equal = gold[(size_t)e.g].key.pos == test[(size_t)e.t].key.pos ? 1u : 0u;
      }
      d_pairs.ensure(n); d_out.ensure(n); d_heavy.ensure(n);
      IMP_HIP_CHECK(hipMemcpyAsync(d_pairs.p, pairs.data(), (size_t)n * sizeof(VdPair), hipMemcpyHostToDevice, stream));
      std::vector<VdOut> out(n);
      uint32_t counters[2] = {0, 0};
      for (;;) {      // again with a longer deferred list when it was full
        IMP_HIP_CHECK(hipMemsetAsync(d_counters.p, 0, 2 * sizeof(uint32_t), stream));
        IMP_HIP_CHECK(hipEventRecord(ev[0], stream));
        const unsigned block = T.n_samples <= 64 ? 64u : (unsigned)kBlock;
        hipLaunchKernelGGL(k_vdiff_compare, dim3(n), dim3(block), 0, stream, T, (const VdPair*)d_pairs.p, n, (uint32_t)base, d_out.p, d_heavy.p, d_counters.p, d_def.p, def_cap);
        IMP_HIP_CHECK(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
        IMP_HIP_CHECK(hipStreamSynchronize(stream));
        if (counters[0]) {
          const unsigned slices = (unsigned)std::max<int32_t>(1, std::min<int32_t>((int32_t)kHeavySlices, T.n_samples));
          hipLaunchKernelGGL(k_vdiff_heavy, dim3(counters[0], slices), dim3(64), 0, stream, T, (const VdPair*)d_pairs.p, (const uint32_t*)d_heavy.p, counters[0], (uint32_t)base, d_out.p,
                             d_counters.p, d_def.p, def_cap);
        }
        IMP_HIP_CHECK(hipEventRecord(ev[1], stream));
        IMP_HIP_CHECK(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
        IMP_HIP_CHECK(hipMemcpyAsync(out.data(), d_out.p, (size_t)n * sizeof(VdOut), hipMemcpyDeviceToHost, stream));
        IMP_HIP_CHECK(hipStreamSynchronize(stream));
        float ms = 0;
        IMP_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); st.ms_compare += ms;
        if (counters[1] <= def_cap) break;
        def_cap = counters[1];
        d_def.ensure(def_cap);
      }
      for (uint32_t i = 0; i < n; ++i) {
        VdEvent& e = events[of_pair[base + i]];
        e.flags = out[i].flags;
        for (int m = 0; m < 4; ++m) { e.info[m] = out[i].info[m]; e.fmt[m] = out[i].fmt[m]; }
        if (out[i].heavy) ++st.pairs_heavy; else ++st.pairs_light;
      }
      // the deferred float tokens: the host's strtod, the same rule
      std::vector<VdDeferred> def(counters[1]);
      if (!def.empty()) IMP_HIP_CHECK(hipMemcpy(def.data(), d_def.p, def.size() * sizeof(VdDeferred), hipMemcpyDeviceToHost));
      st.deferred += (int64_t)def.size();
      for (const VdDeferred& d : def) {
        std::string a(std::min<uint32_t>(d.an, 1024u), '\0'), b(std::min<uint32_t>(d.bn, 1024u), '\0');
        IMP_HIP_CHECK(hipMemcpy(&a[0], d.a, a.size(), hipMemcpyDeviceToHost));
        IMP_HIP_CHECK(hipMemcpy(&b[0], d.b, b.size(), hipMemcpyDeviceToHost));
        if (vd_deferred_differs(a, b, req.threshold)) vd_apply_deferred(events[of_pair[d.pair]], d.what);
      }
    }
  }
};

}  // namespace

VcfDiffReport vcfdiff_device(const VcfDiffRequest& req, VcfDiffStats* stats) {
  const double t0 = now_s();
  // ---- the refusals: before the device is touched
  for (const std::string* p : {&req.gold, &req.test}) {
    if (p->empty()) throw VCFDiffException("vcfdiff needs two paths, gold and test");
    if (file_is_bcf2(*p)) throw VCFDiffException(*p + " is BCF2: vcfdiff reads VCF text only (plain, gzip or BGZF) in this build");
  }
  if (!(req.threshold >= 0)) throw VCFDiffException("the threshold is negative or not a number");
  Differ S(req);
  const VdHeader gh = vd_parse_header(read_head(req.gold)), th = vd_parse_header(read_head(req.test));
  S.H = vd_build_tables(gh, th);
  if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible: vcfdiff has no CPU fallback");
  IMP_HIP_CHECK(hipSetDevice(req.device));
  S.upload_tables();

  // ---- pass 1: both files through the importer's text tap (the tool has no vid file: an empty one serves the constructor)
  VidMapper vid;
  vid.parse_vid_json(mini_json::parse("{\"contigs\": {}, \"fields\": {}}"));
  vid.parse_callsets_json(mini_json::parse("{\"callsets\": {}}"));
  ImportTextTap tap;
  tap.on_batch = [&](const ImportTextBatch& b) { S.on_batch(b); };
  ImportOptions opt;
  DeviceImporter imp(req.device, vid, opt, req.text_budget_bytes, DeviceImporter::kInflateAuto, &tap);
  S.file = 0; imp.append_text_path(req.gold);
  S.file = 1; imp.append_text_path(req.test);
  {
    const ImportStats& is = imp.stats();
    S.st.ms_index = is.ms_index; S.st.ms_inflate = is.ms_inflate; S.st.s_read = is.s_read;
  }

  // ---- the keys on the host: a file's errors, then the walk
  const double t1 = now_s();
  std::vector<VdRecord> recs[2];
  for (int f = 0; f < 2; ++f)
    recs[f] = vd_records(f ? req.test : req.gold, S.lines[f], S.H, f, req.regions, [&](size_t i) { return S.line_text(S.lines[f][i]); });
  S.st.gold_records = (int64_t)recs[0].size(); S.st.test_records = (int64_t)recs[1].size();
  std::vector<VdEvent> events = vd_walk(recs[0], recs[1], S.H);
  S.st.s_walk = now_s() - t1;

  // ---- pass 2
  S.compare(events, recs[0], recs[1]);

  // ---- only the lines of listed events come back
  VcfDiffReport rep;
  rep.info_names = S.H.info_names; rep.fmt_names = S.H.fmt_names;
  std::vector<VdEventText> text(events.size());
  for (size_t k = 0; k < events.size(); ++k) {
    const VdEvent& e = events[k];
    rep.compared += e.pair >= 0;
    if (!vd_event_listed(e)) continue;
    if (e.g >= 0) text[k].gold = S.line_text(recs[0][(size_t)e.g]);
    if (e.t >= 0) text[k].test = S.line_text(recs[1][(size_t)e.t]);
    VcfDiffEvent o;
    o.kind = e.kind; o.gold_line = e.g >= 0 ? recs[0][(size_t)e.g].line_no : 0; o.test_line = e.t >= 0 ? recs[1][(size_t)e.t].line_no : 0;
    o.gold_text = text[k].gold; o.test_text = text[k].test; o.compared = e.pair >= 0; o.flags = e.flags;
    for (int m = 0; m < 4; ++m) { o.info[m] = e.info[m]; o.fmt[m] = e.fmt[m]; }
    rep.events.push_back(o);
  }
  rep.json = vd_report_json(events, text, recs[0], recs[1], S.H);
  S.st.events = (int64_t)rep.events.size();
  S.st.s_total = now_s() - t0;
  if (stats) *stats = S.st;
  return rep;
}

}  // namespace genomicsdb_amd
