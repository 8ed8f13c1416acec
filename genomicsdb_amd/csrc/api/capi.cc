// capi.cc - extern "C" surface declared in include/genomicsdb_amd.h
#include "../../../include/genomicsdb_amd.h"

#include <functional>
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>

#include "genomicsdb_bcf_generator.h"
#include "genomicsdb_importer.h"
#include "../kernels/gdb_import_stream.h"
#include "../kernels/gdb_bgzf.h"
#include "../kernels/gdb_inflate.h"
#include "../kernels/gdb_histogram.h"
#include "../kernels/gdb_index.h"
#include "../kernels/gdb_columns.h"

static_assert(GDBAMD_MAX_COLUMN_REQUESTS == GDB_MAX_COLUMN_REQUESTS, "the public limit is the decoder's");
#include "../kernels/gdb_vcfdiff.h"
#include "../kernels/gdb_split.h"
#include "../host/vcf_importer.h"
#include "../host/vcf_index.h"

using namespace genomicsdb_amd;

namespace {
thread_local std::string g_last_error;
template <class F, class R> R guarded(F f, R on_error) {
  try { g_last_error.clear(); return f(); }
  catch (const std::exception& e) { g_last_error = e.what(); return on_error; }
  catch (...) { g_last_error = "unknown exception"; return on_error; }
}
struct EngineHandle {
  std::unique_ptr<CombineEngine> eng; std::string calls_text; int calls_text_mode = -1;
  std::unique_ptr<RecordColumns> columns; bool has_page = false;      // the column decoder of gdbamd_engine_columns_select; has_page: next_page returned a page and no other call on the engine (staging, run_interval, the lanes, the printers) has come since
};   // calls_text: the document of gdbamd_engine_print_cells(mode) between its sizing and its copying call
// every entry point that stages, runs an interval or the lanes, prints or loads begins with this: the page next_page returned is no longer the caller's
void page_gone(void* e) { if (e) ((EngineHandle*)e)->has_page = false; }
}  // namespace

extern "C" {

const char* gdb_mi355_last_error(void) { return g_last_error.c_str(); }
int gdb_mi355_device_count(void) { return DevicePipeline::device_count(); }

void* gdb_mi355_init(const char* loader_json_file, const char* query_json_file, const char* chr, int start, int end, int rank, uint64_t buffer_capacity,
                     uint64_t segment_size, int is_bcf, int produce_header_only, int use_missing, int keep_idx) {
  return guarded([&]() -> void* {
    return new GenomicsDBBCFGenerator(loader_json_file ? loader_json_file : "", query_json_file ? query_json_file : "", chr, start, end, rank, buffer_capacity,
                                      segment_size, is_bcf ? "bu" : "", produce_header_only != 0, is_bcf && use_missing, is_bcf && keep_idx);
  }, (void*)nullptr);
}
void* gdb_mi355_init_from_memory(const char* query_json_text, const uint8_t* cells, uint64_t nbytes, uint64_t buffer_capacity, int produce_header_only) {
  return guarded([&]() -> void* { return new GenomicsDBBCFGenerator(std::string(query_json_text), cells, nbytes, buffer_capacity, produce_header_only != 0); }, (void*)nullptr);
}
void* gdb_mi355_init_from_memory_format(const char* query_json_text, const uint8_t* cells, uint64_t nbytes, uint64_t buffer_capacity, int produce_header_only, int is_bcf,
                                        int use_missing, int keep_idx) {
  return guarded([&]() -> void* {
    return new GenomicsDBBCFGenerator(std::string(query_json_text), cells, nbytes, buffer_capacity, produce_header_only != 0, is_bcf ? "bu" : "", is_bcf && use_missing, keep_idx != 0);
  }, (void*)nullptr);
}
void* gdb_mi355_init_output_format(const char* loader_json_file, const char* query_json_file, const char* chr, int start, int end, int rank, uint64_t buffer_capacity,
                                   uint64_t segment_size, const char* output_format, int produce_header_only, int use_missing, int keep_idx) {
  return guarded([&]() -> void* {
    const std::string fmt = output_format ? output_format : "";
    const bool bcf = fmt == "bu" || fmt == "b";
    return new GenomicsDBBCFGenerator(loader_json_file ? loader_json_file : "", query_json_file ? query_json_file : "", chr, start, end, rank, buffer_capacity,
                                      segment_size, fmt.c_str(), produce_header_only != 0, bcf && use_missing, bcf && keep_idx, true);
  }, (void*)nullptr);
}
void* gdb_mi355_init_from_memory_output_format(const char* query_json_text, const uint8_t* cells, uint64_t nbytes, uint64_t buffer_capacity, int produce_header_only,
                                               const char* output_format, int use_missing, int keep_idx) {
  return guarded([&]() -> void* {
    const std::string fmt = output_format ? output_format : "";
    const bool bcf = fmt == "bu" || fmt == "b";
    return new GenomicsDBBCFGenerator(std::string(query_json_text), cells, nbytes, buffer_capacity, produce_header_only != 0, fmt.c_str(), bcf && use_missing, keep_idx != 0);
  }, (void*)nullptr);
}
uint64_t gdb_mi355_close(void* h) { delete (GenomicsDBBCFGenerator*)h; return 0; }
uint64_t gdb_mi355_get_num_bytes_available(void* h) { return h ? ((GenomicsDBBCFGenerator*)h)->get_buffer_capacity() : 0; }
int gdb_mi355_read_next_byte(void* h) {
  if (!h) return -1;
  return guarded([&]() -> int { auto* g = (GenomicsDBBCFGenerator*)h; if (g->end()) return -1; return (int)g->read_next_byte(); }, -1);
}
int64_t gdb_mi355_read(void* h, uint8_t* dst, uint64_t offset, uint64_t n) {
  if (!h) return 0;
  return guarded([&]() -> int64_t { return (int64_t)((GenomicsDBBCFGenerator*)h)->read_and_advance(dst, offset, n); }, (int64_t)-1);
}
int64_t gdb_mi355_skip(void* h, uint64_t n) {
  if (!h) return 0;
  return guarded([&]() -> int64_t { return (int64_t)((GenomicsDBBCFGenerator*)h)->read_and_advance(nullptr, 0, n); }, (int64_t)-1);
}

int gdb_mi355_peek(void* h, const uint8_t** ptr, uint64_t* n) {
  if (!h || !ptr || !n) return -1;
  return guarded([&]() -> int {
    auto* g = (GenomicsDBBCFGenerator*)h;
    for (;;) {
      const GenomicsDBBCFGenerator::RWBuffer b = g->get_read_batch();
      if (b.m_num_valid_bytes > b.m_next_read_idx) { *ptr = b.m_buffer + b.m_next_read_idx; *n = b.m_num_valid_bytes - b.m_next_read_idx; return 1; }
      if (g->end() || b.m_buffer == nullptr) { *ptr = nullptr; *n = 0; return 0; }
      g->read_and_advance(nullptr, 0, SIZE_MAX);     // an exhausted batch: produce the next one
    }
  }, -1);
}
int gdb_mi355_get_stream_stats(void* h, gdb_mi355_stream_stats* out) {
  if (!h || !out) return -1;
  const GenomicsDBBCFGenerator::DrainStats& d = ((GenomicsDBBCFGenerator*)h)->drain_stats();
  out->pages = d.pages; out->chunks = d.chunks; out->bytes = d.bytes;
  out->seconds_waiting_for_copies = d.seconds_waiting_for_copies; out->seconds_producing = d.seconds_producing;
  return 0;
}

int gdb_mi355_enable_index(void* h) {
  if (!h) return -1;
  return guarded([&]() -> int { ((GenomicsDBBCFGenerator*)h)->enable_output_index(); return 0; }, -1);
}
int gdb_mi355_write_index(void* h, const char* path, gdb_mi355_index_stats* stats) {
  if (!h || !path) return -1;
  return guarded([&]() -> int {
    const OutputIndexStats& s = ((GenomicsDBBCFGenerator*)h)->write_output_index(path);
    if (stats) {
      stats->pages = s.pages; stats->records = s.records; stats->contigs = s.contigs; stats->bins = s.bins; stats->chunks = s.chunks; stats->linear_windows = s.linear_windows;
      stats->atomics = s.atomics; stats->ms_records = s.ms_records; stats->ms_voff = s.ms_voff; stats->ms_chunks = s.ms_chunks; stats->ms_linear = s.ms_linear;
      stats->s_write = s.s_write; stats->table_bytes = s.table_bytes;
    }
    return 0;
  }, -1);
}

void* gdbamd_engine_create(const char* query_json_text, int device) {
  return guarded([&]() -> void* { auto* e = new EngineHandle; e->eng.reset(new CombineEngine(mini_json::parse(query_json_text), device)); return e; }, (void*)nullptr);
}
void* gdbamd_engine_create_format(const char* query_json_text, int device, int is_bcf, int use_missing) {
  return guarded([&]() -> void* {
    auto* e = new EngineHandle;
    e->eng.reset(new CombineEngine(mini_json::parse(query_json_text), device, nullptr, 0, is_bcf ? "bu" : "", is_bcf && use_missing));
    return e;
  }, (void*)nullptr);
}
void* gdbamd_engine_create_output_format(const char* query_json_text, int device, const char* output_format, int use_missing) {
  return guarded([&]() -> void* {
    const std::string fmt = output_format ? output_format : "";
    auto* e = new EngineHandle;
    e->eng.reset(new CombineEngine(mini_json::parse(query_json_text), device, nullptr, 0, fmt, (fmt == "bu" || fmt == "b") && use_missing));
    return e;
  }, (void*)nullptr);
}
// BGZF blocks of n host bytes, compressed by the device kernels (a utility and the test hook of kernels/gdb_bgzf.hip)
int gdbamd_bgzf_compress(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels) {
  return gdbamd_bgzf_compress_mode(src, n, dst, dst_cap, dst_len, ms_kernels, 0);
}
int gdbamd_bgzf_compress_mode(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels, int vcf_text) {
  return guarded([&]() -> int {
    if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible");
    const uint64_t bound = bgzf_bound(n);
    char* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)bound + 64) != hipSuccess) throw GenomicsDBDeviceException("hipMalloc failed");
    uint64_t got = 0;
    try {
      if (n && hipMemcpy(d, src, (size_t)n, hipMemcpyHostToDevice) != hipSuccess) throw GenomicsDBDeviceException("copy to the device failed");
      BgzfDeviceCompressor c;
      c.set_text(vcf_text != 0);
      got = c.compress(d, n, d, nullptr, ms_kernels);
      if (got > dst_cap) throw GenomicsDBDeviceException("destination too small: " + std::to_string(got) + " bytes needed");
      if (got && hipMemcpy(dst, d, (size_t)got, hipMemcpyDeviceToHost) != hipSuccess) throw GenomicsDBDeviceException("copy from the device failed");
    } catch (...) { (void)hipFree(d); throw; }
    (void)hipFree(d);
    *dst_len = got;
    return 0;
  }, -1);
}
uint64_t gdbamd_bgzf_bound(uint64_t n) { return bgzf_bound(n); }
// the counterpart: a whole BGZF buffer inflated by the kernel of kernels/gdb_inflate.hip (a utility and its test hook)
int gdbamd_bgzf_decompress(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, float* ms_kernels, int device) {
  return guarded([&]() -> int {
    if (!src || !dst_len) throw GenomicsDBConfigException("gdbamd_bgzf_decompress: null argument");
    std::vector<BgzfMember> mem;
    uint64_t total = 0;
    uint64_t break_at = 0;
    if (!bgzf_walk(src, n, mem, &total, &break_at))
      throw GenomicsDBConfigException("gdbamd_bgzf_decompress: the buffer is not BGZF from its first byte to its last: no whole member at byte offset " + std::to_string(break_at));
    *dst_len = total;
    if (!dst) return 0;
    if (total > dst_cap) throw GenomicsDBDeviceException("destination too small: " + std::to_string(total) + " bytes needed");
    if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible");
    if (hipSetDevice(device) != hipSuccess) throw GenomicsDBDeviceException("no HIP device " + std::to_string(device));
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)total + 64) != hipSuccess) throw GenomicsDBDeviceException("hipMalloc failed");
    try {
      BgzfDeviceInflater inf;
      const size_t step = 8192;           // members per launch: at most 512 MiB of them
      for (size_t m0 = 0; m0 < mem.size(); m0 += step) {
        const size_t m1 = std::min(mem.size(), m0 + step);
        uint32_t err = 0;
        const int64_t bad = inf.inflate(src, mem.data(), m0, m1, d + mem[m0].out_off, nullptr, &err);
        if (bad >= 0) throw GenomicsDBDeviceException("corrupt BGZF member at byte offset " + std::to_string(mem[(size_t)bad].offset) + ": " + bgzf_inflate_error_text(err));
      }
      if (ms_kernels) *ms_kernels = inf.ms_kernel;
      if (total && hipMemcpy(dst, d, (size_t)total, hipMemcpyDeviceToHost) != hipSuccess) throw GenomicsDBDeviceException("copy from the device failed");
    } catch (...) { (void)hipFree(d); throw; }
    (void)hipFree(d);
    return 0;
  }, -1);
}
// independent DEFLATE tiles through the tile inflater of the fragment reader (k_inflate_tiles; a diagnostic and its test hook)
int gdbamd_inflate_tiles(const uint8_t* src, const uint64_t* in_off, const uint32_t* want, uint64_t ntiles, uint8_t fill, uint8_t* out, uint8_t* status, int device) {
  return guarded([&]() -> int {
    if (!in_off || (ntiles && (!want || !out || !status)) || (ntiles && in_off[ntiles] && !src)) throw GenomicsDBConfigException("gdbamd_inflate_tiles: null argument");
    if (DevicePipeline::device_count() <= 0) throw GenomicsDBDeviceException("no HIP device visible");
    inflate_tiles_on_device(src, in_off, want, ntiles, fill, out, status, device);
    return 0;
  }, -1);
}
void gdbamd_engine_destroy(void* e) { delete (EngineHandle*)e; }
int gdbamd_engine_num_fields(void* e) { return e ? ((EngineHandle*)e)->eng->plan().plan.nfields : -1; }
const char* gdbamd_engine_field_name(void* e, int f) {
  if (!e) return nullptr;
  const HostPlan& hp = ((EngineHandle*)e)->eng->plan();
  return (f >= 0 && f < hp.plan.nfields) ? hp.field_names[(size_t)f].c_str() : nullptr;
}
int gdbamd_engine_field_info(void* e, int f, int* elem_type, int* is_var, int* fixed_num) {
  if (!e) return -1;
  const CombinePlan& pl = ((EngineHandle*)e)->eng->plan().plan;
  if (f < 0 || f >= pl.nfields) return -1;
  *elem_type = pl.field[f].elem;
  *is_var = pl.field[f].length != GDB_VL_FIXED;
  *fixed_num = pl.field[f].fixed_num;
  return 0;
}
uint64_t gdbamd_engine_header(void* e, char* dst, uint64_t cap) {
  if (!e) return 0;
  const std::string& h = ((EngineHandle*)e)->eng->plan().header_text;
  if (dst && cap) memcpy(dst, h.data(), std::min<uint64_t>(cap, h.size()));
  return h.size();
}
int gdbamd_engine_stage_cells(void* e, const uint8_t* cells, uint64_t nbytes) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->stage_cells(cells, nbytes); return 0; }, 1);
}
int gdbamd_engine_stage_cells_begin(void* e) {
  page_gone(e); return guarded([&]() -> int { ((EngineHandle*)e)->eng->stage_cells_begin(); return 0; }, 1); }
int gdbamd_engine_stage_cells_append(void* e, const uint8_t* cells, uint64_t nbytes) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->stage_cells_append(cells, nbytes); return 0; }, 1);
}
int gdbamd_engine_stage_cells_end(void* e) {
  page_gone(e); return guarded([&]() -> int { ((EngineHandle*)e)->eng->stage_cells_end(); return 0; }, 1); }
int gdbamd_engine_adopt_device_fragment(void* e, int64_t ncells, const int32_t* row, const int64_t* begin, const int64_t* end, const gdbamd_device_column* cols,
                                        int ncols, uint64_t reference_cell_bytes) {
  page_gone(e);
  return guarded([&]() -> int {
    CombineEngine& eng = *((EngineHandle*)e)->eng;
    if (ncols != eng.plan().plan.nfields) throw GenomicsDBDeviceException("adopt_device_fragment: ncols != number of plan fields");
    FragmentView v;
    memset(&v, 0, sizeof(v));
    v.ncells = ncells; v.row = row; v.begin = begin; v.end = end;
    for (int f = 0; f < ncols; ++f) { v.col[f].data = cols[f].data; v.col[f].off = cols[f].off; }
    eng.pipeline().adopt_fragment(v);
    eng.reference_cell_bytes = reference_cell_bytes;
    eng.has_cells = ncells > 0;
    eng.num_cells = ncells;
    return 0;
  }, 1);
}
int gdbamd_engine_open_array(void* e, const char* dir) {
  page_gone(e); return guarded([&]() -> int { ((EngineHandle*)e)->eng->open_array(dir ? dir : ""); return 0; }, 1); }
int gdbamd_engine_open_memory_cells(void* e, const uint8_t* cells, uint64_t nbytes) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->open_memory_cells(cells, nbytes); return 0; }, 1);
}
int gdbamd_pin_host_memory(const void* p, uint64_t nbytes) {
  return guarded([&]() -> int {
    if (!p || !nbytes) return 0;
    if (hipHostRegister(const_cast<void*>(p), (size_t)nbytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); throw GenomicsDBDeviceException("hipHostRegister failed (locked-memory limit?)"); }
    return 0;
  }, 1);
}
int gdbamd_unpin_host_memory(const void* p) {
  return guarded([&]() -> int {
    if (p && hipHostUnregister(const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); throw GenomicsDBDeviceException("hipHostUnregister failed"); }
    return 0;
  }, 1);
}
int gdbamd_engine_open_cell_callback(void* e, gdbamd_cell_chunk_fn fn, void* user) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->open_cell_callback(fn, user); return 0; }, 1);
}
int gdbamd_engine_cover(void* e, int64_t column, int64_t* lo, int64_t* hi) {
  page_gone(e);
  return guarded([&]() -> int {
    const CombineEngine::Coverage c = ((EngineHandle*)e)->eng->cover(column);
    if (lo) *lo = c.lo;
    if (hi) *hi = c.hi;
    return 0;
  }, 1);
}
int gdbamd_engine_staged_info(void* e, int64_t* ncells, uint64_t* reference_cell_bytes) {
  if (!e) return 1;
  CombineEngine& eng = *((EngineHandle*)e)->eng;
  if (ncells) *ncells = eng.num_cells;
  if (reference_cell_bytes) *reference_cell_bytes = eng.reference_cell_bytes;
  return 0;
}
int gdbamd_engine_set_reference(void* e, int64_t begin, const char* bases, uint64_t len) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->set_reference_window(begin, std::string(bases, len)); return 0; }, 1);
}

namespace {
struct HostCopy { char* dst; uint64_t cap, len; };
void copy_page(void* user, const char* dev, uint64_t n) {
  HostCopy* hc = (HostCopy*)user;
  if (hc->dst && hc->len < hc->cap) {
    uint64_t k = std::min(n, hc->cap - hc->len);
    if (hipMemcpy(hc->dst + hc->len, dev, k, hipMemcpyDeviceToHost) != hipSuccess) throw GenomicsDBDeviceException("page copy to host failed");
  }
  hc->len += n;
}
}  // namespace

static void fill_interval_stats(gdbamd_interval_stats* out, const IntervalStats& s, CombineEngine& eng) {
  out->num_cells = s.num_cells; out->num_cells_in_window = s.num_cells_in_window; out->num_records = s.num_records;
  out->num_heavy_incidences = s.num_heavy_incidences; out->bytes_out = s.bytes_out; out->bytes_in_reference_cells = eng.reference_cell_bytes;
  out->pages = s.pages; out->write_launches = s.write_launches; out->err_bits = s.err_bits;
  out->ms_sweep = s.ms_sweep; out->ms_site = s.ms_site; out->ms_size = s.ms_size; out->ms_write = s.ms_write; out->ms_total = s.ms_total;
  out->ms_write_kernel_avg = s.ms_write_kernel_avg;
  out->num_record_types = s.num_record_types; out->resolved_entry_bytes = s.resolved_entry_bytes;
  out->num_text_slots = s.num_text_slots; out->text_pool_bytes = s.text_pool_bytes;
  out->num_remap_elements = s.num_remap_elements;
  out->bytes_compressed = s.bytes_compressed; out->ms_compress = s.ms_compress; out->page_kernel = s.page_kernel;
  for (int i = 0; i < GDBAMD_GT_NUM_STATS; ++i) out->gt_profile_stats[i] = s.gt_profile[i];
  out->huge_records = s.huge_records; out->huge_fallbacks = s.huge_fallbacks;
  out->sorted_median_fields = s.sorted_median_fields; out->big_median_records = s.big_median_records; out->big_median_unlisted = s.big_median_unlisted;
}
int gdbamd_engine_run_interval(void* e, int64_t qb, int64_t qe, uint64_t arena_bytes, char* host_out, uint64_t host_cap, uint64_t* host_len,
                               gdbamd_interval_stats* out) {
  page_gone(e);
  return guarded([&]() -> int {
    CombineEngine& eng = *((EngineHandle*)e)->eng;
    HostCopy hc{host_out, host_cap, 0};
    eng.stage_reference_for(qb, qe);  // no-op unless the query names a reference_genome and cells were staged from host
    IntervalStats s = eng.pipeline().run_interval(qb, qe, arena_bytes, host_out ? copy_page : nullptr, &hc);
    if (host_len) *host_len = host_out ? hc.len : s.bytes_out;
    if (out) fill_interval_stats(out, s, eng);
    return 0;
  }, 1);
}
int gdbamd_engine_run_intervals(void* e, int n, const int64_t* begins, const int64_t* ends, uint64_t arena_bytes, int lanes, gdbamd_interval_stats* stats,
                                char* const* host_out, const uint64_t* host_cap, uint64_t* host_len) {
  page_gone(e);
  return guarded([&]() -> int {
    CombineEngine& eng = *((EngineHandle*)e)->eng;
    std::vector<std::pair<int64_t, int64_t>> ivs;
    for (int i = 0; i < n; ++i) ivs.emplace_back(begins[i], ends[i]);
    std::vector<HostCopy> hc;
    std::function<void(size_t, const char*, uint64_t)> on_page;
    if (host_out) {      // (interval i's pages go to host_out[i], each interval from one thread only)
      for (int i = 0; i < n; ++i) hc.push_back(HostCopy{host_out[i], host_cap ? host_cap[i] : 0, 0});
      on_page = [&hc](size_t i, const char* dev, uint64_t nbytes) { copy_page(&hc[i], dev, nbytes); };
    }
    const std::vector<IntervalStats> res = eng.run_intervals(ivs, arena_bytes, lanes, on_page);
    if (host_len) for (int i = 0; i < n; ++i) host_len[i] = host_out ? hc[(size_t)i].len : res[(size_t)i].bytes_out;
    if (stats) for (int i = 0; i < n; ++i) fill_interval_stats(&stats[i], res[(size_t)i], eng);
    return 0;
  }, 1);
}

int gdbamd_engine_lane_footprint(void* e, int64_t interval_columns, uint64_t arena_bytes, uint64_t* bytes) {
  return guarded([&]() -> int { *bytes = ((EngineHandle*)e)->eng->lane_footprint_bytes(interval_columns, arena_bytes); return 0; }, -1);
}
int gdbamd_engine_release_lanes(void* e) {
  page_gone(e);
  return guarded([&]() -> int { ((EngineHandle*)e)->eng->release_lanes(); return 0; }, -1);
}

int gdbamd_engine_prepare_interval(void* e, int64_t qb, int64_t qe) {
  return guarded([&]() -> int {
    CombineEngine& eng = *((EngineHandle*)e)->eng;
    ((EngineHandle*)e)->has_page = false;
    eng.stage_reference_for(qb, qe);
    eng.pipeline().prepare_interval(qb, qe);
    return 0;
  }, -1);
}
int gdbamd_engine_next_page(void* e, uint64_t arena_bytes, const void** dev_ptr, uint64_t* nbytes) {
  return guarded([&]() -> int {
    const char* p = nullptr;
    uint64_t n = 0;
    ((EngineHandle*)e)->has_page = false;
    const bool more = ((EngineHandle*)e)->eng->pipeline().next_page(arena_bytes, &p, &n);
    ((EngineHandle*)e)->has_page = more;
    if (dev_ptr) *dev_ptr = more ? p : nullptr;
    if (nbytes) *nbytes = more ? n : 0;
    return more ? 1 : 0;
  }, -1);
}

int gdbamd_engine_columns_select(void* e, const gdbamd_column_request* requests, int n) {
  return guarded([&]() -> int {
    EngineHandle* h = (EngineHandle*)e;
    if (n < 0 || (n > 0 && !requests)) throw GenomicsDBDeviceException("columns_select: no requests given");
    std::vector<ColumnRequest> rq;
    for (int i = 0; i < n; ++i) { ColumnRequest r; r.name = requests[i].name ? requests[i].name : ""; r.dtype = requests[i].dtype; r.width = requests[i].width; rq.push_back(r); }
    h->columns.reset();
    h->columns.reset(new RecordColumns(h->eng->plan(), h->eng->device(), rq));
    return 0;
  }, -1);
}
int gdbamd_engine_page_columns(void* e, gdbamd_column* out_columns, int cap, int* n, gdbamd_columns_stats* stats) {
  return guarded([&]() -> int {
    EngineHandle* h = (EngineHandle*)e;
    if (!h->columns) throw GenomicsDBDeviceException("page_columns: no fields chosen: call gdbamd_engine_columns_select first");
    if (!h->has_page) throw GenomicsDBDeviceException("page_columns: there is no page: gdbamd_engine_next_page has not returned one, or the interval is exhausted");
    ColumnsStats cs;
    const std::vector<RecordColumn>& cols = h->columns->decode(h->eng->pipeline().last_page(), &cs);
    if (n) *n = (int)cols.size();
    for (int i = 0; out_columns && i < cap && i < (int)cols.size(); ++i) {
      const RecordColumn& c = cols[(size_t)i];
      out_columns[i].name = c.name.c_str(); out_columns[i].dtype = c.dtype; out_columns[i].ndim = c.ndim;
      for (int k = 0; k < 3; ++k) out_columns[i].shape[k] = c.shape[k];
      out_columns[i].dev_ptr = c.dev_ptr;
    }
    if (stats) {
      memset(stats, 0, sizeof(*stats));
      stats->records = cs.records; stats->bytes_read = cs.bytes_read; stats->bytes_written = cs.bytes_written;
      stats->ms_measure = cs.ms_measure; stats->ms_site = cs.ms_site; stats->ms_scatter = cs.ms_scatter; stats->n_fields = cs.n_fields;
      for (int i = 0; i < GDBAMD_MAX_COLUMN_REQUESTS; ++i) stats->width[i] = cs.width[i];
    }
    return 0;
  }, -1);
}

int gdbamd_engine_split_point(void* engine, int64_t qb, int64_t qe, int64_t max_columns, int64_t* piece_end) {
  try { *piece_end = ((EngineHandle*)engine)->eng->pipeline().split_point(qb, qe, max_columns); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_engine_column_histogram(void* engine, uint64_t hist_begin, uint64_t hist_end, uint64_t bin_size, uint64_t* counts, uint64_t nbins, int accumulate) {
  page_gone(engine);
  try { ((EngineHandle*)engine)->eng->pipeline().column_histogram(hist_begin, hist_end, bin_size, counts, nbins, accumulate != 0); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
// gt_mpi_gather --print-calls: the document is produced by the call with dst == NULL (which returns its length) and kept in the handle
// for the call that copies it
int64_t gdbamd_engine_print_calls(void* engine, char* dst, uint64_t cap) { return gdbamd_engine_print_cells(engine, 0, dst, cap); }
// mode 0: --print-calls, 1: --print-csv, 2: --print-AC
int64_t gdbamd_engine_print_cells(void* engine, int mode, char* dst, uint64_t cap) {
  page_gone(engine);
  try {
    EngineHandle* h = (EngineHandle*)engine;
    auto make = [&]() { h->calls_text_mode = mode; return mode == 0 ? h->eng->print_calls() : mode == 1 ? h->eng->print_csv() : h->eng->print_allele_counts(); };
    if (!dst) { h->calls_text = make(); return (int64_t)h->calls_text.size(); }
    if (h->calls_text_mode != mode) h->calls_text = make();     // (nothing kept, or the document of another mode)
    const size_t n = h->calls_text.size();
    if (cap < n) { g_last_error = "print_calls: destination too small"; return -1; }
    memcpy(dst, h->calls_text.data(), n);
    std::string().swap(h->calls_text);                          // handed over: a multi-GB document does not stay in the handle
    h->calls_text_mode = -1;
    return (int64_t)n;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
// gt_mpi_gather without a mode flag: the variants document, same two-call convention (kept in the handle as "mode 3")
int64_t gdbamd_engine_query_variants(void* engine, char* dst, uint64_t cap) {
  page_gone(engine);
  try {
    EngineHandle* h = (EngineHandle*)engine;
    auto make = [&]() { h->calls_text_mode = 3; return h->eng->query_variants(); };
    if (!dst) { h->calls_text = make(); return (int64_t)h->calls_text.size(); }
    if (h->calls_text_mode != 3) h->calls_text = make();
    const size_t n = h->calls_text.size();
    if (cap < n) { g_last_error = "query_variants: destination too small"; return -1; }
    memcpy(dst, h->calls_text.data(), n);
    std::string().swap(h->calls_text);
    h->calls_text_mode = -1;
    return (int64_t)n;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
// ColumnHistogramOperator::equi_partition_and_print_bins (variant_operations.cc:769-796), the text it prints; returns its length (dst may be NULL), -1 when
// num_parts >= nbins (the reference prints a complaint and returns false)
int64_t gdbamd_equi_partition_text(const uint64_t* counts, uint64_t nbins, uint64_t hist_begin, uint64_t bin_size, uint64_t num_parts, char* dst, uint64_t cap) {
  if (num_parts >= nbins || num_parts == 0) return -1;
  unsigned long long total = 0;
  for (uint64_t i = 0; i < nbins; ++i) total += counts[i];
  const double per = (double)total / (double)num_parts;
  std::string out;
  char line[160];
  snprintf(line, sizeof(line), "Total %llu #bins %llu count/bins %.1f\n", total, (unsigned long long)num_parts, per);
  out += line;
  // (no cell at all - an empty array, or query rows without cells: the reference's loop would not advance (its assert(j > i)); the header
  // line alone is the answer here)
  for (uint64_t i = 0; i < nbins && total > 0;) {
    uint64_t j = i;
    unsigned long long cur = 0;
    for (; (double)cur < per && j < nbins; cur += counts[j], ++j) {}
    snprintf(line, sizeof(line), "%llu,%llu,%llu\n", (unsigned long long)(hist_begin + i * bin_size), (unsigned long long)(hist_begin + j * bin_size - 1), cur);
    out += line;
    i = j;
  }
  out += "\n";
  if (dst && cap) { const size_t n = std::min<size_t>(out.size(), (size_t)cap); memcpy(dst, out.data(), n); }
  return (int64_t)out.size();
}
int gdbamd_build_output_index(const char* path, int is_bcf) {
  try { if (is_bcf) build_csi_index(path); else build_tbi_index(path); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_engine_save_fragment(void* engine, const char* path) {
  try { ((EngineHandle*)engine)->eng->save_fragment(path); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_engine_save_fragment_compressed(void* engine, const char* path) {
  try { ((EngineHandle*)engine)->eng->save_fragment(path, true); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_engine_load_fragment(void* engine, const char* path) {
  page_gone(engine);
  try { ((EngineHandle*)engine)->eng->load_fragment(path); return 0; } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}

int gdbamd_column_partition(const char* loader_json_text, int rank, int64_t* begin, int64_t* end) {
  try {
    GenomicsDBImportConfig cfg;
    cfg.read_from_json(mini_json::parse(std::string(loader_json_text ? loader_json_text : "")), rank);
    const ColumnRange r = cfg.get_column_partition(rank);
    if (begin) *begin = r.first;
    if (end) *end = r.second;
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}

int gdbamd_import_cells(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                        int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells) {
  return gdbamd_import_cells_rows(vid_mapping_file, callset_mapping_file, file_root, treat_deletions_as_intervals, column_begin, column_end, cells, nbytes, ncells, 0,
                                  INT64_MAX - 1, nullptr);
}
int gdbamd_import_cells_rows(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                             int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int64_t lb_callset_row_idx,
                             int64_t ub_callset_row_idx, int64_t* nfiles) {
  try {
    if (!vid_mapping_file || !callset_mapping_file || !cells || !nbytes) throw GenomicsDBConfigException("gdbamd_import_cells: null argument");
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(callset_mapping_file));
    ImportOptions opt;
    opt.treat_deletions_as_intervals = treat_deletions_as_intervals != 0;
    opt.column_begin = column_begin;
    opt.column_end = column_end;
    if (file_root) opt.file_root = file_root;
    opt.row_begin = lb_callset_row_idx;
    opt.row_end = ub_callset_row_idx;
    ImportStats st;
    const std::vector<uint8_t> out = import_callsets_to_cells(vid, opt, &st);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!*cells) throw GenomicsDBConfigException("out of memory");
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *nbytes = out.size();
    if (ncells) *ncells = st.num_cells;
    if (nfiles) *nfiles = st.num_files;
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_import_cells_device(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                               int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device, uint64_t text_budget_bytes,
                               double* stats) {
  return gdbamd_import_cells_device_ex(vid_mapping_file, callset_mapping_file, file_root, treat_deletions_as_intervals, column_begin, column_end, cells, nbytes, ncells,
                                       device, text_budget_bytes, 0, stats, stats ? GDBAMD_IMPORT_NUM_STATS : 0);
}
int gdbamd_import_cells_device_ex(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                  int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device, uint64_t text_budget_bytes,
                                  int inflate_mode, double* stats, int nstats) {
  return gdbamd_import_cells_device_streams(vid_mapping_file, callset_mapping_file, file_root, treat_deletions_as_intervals, column_begin, column_end, cells, nbytes, ncells,
                                            device, text_budget_bytes, inflate_mode, stats, nstats, 0, nullptr, nullptr, nullptr);
}
int gdbamd_import_cells_device_streams(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                       int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device,
                                       uint64_t text_budget_bytes, int inflate_mode, double* stats, int nstats, int nstreams, const char* const* names,
                                       const void* const* data, const uint64_t* stream_nbytes) {
  return gdbamd_import_cells_device_rows(vid_mapping_file, callset_mapping_file, file_root, treat_deletions_as_intervals, column_begin, column_end, cells, nbytes, ncells,
                                         device, text_budget_bytes, inflate_mode, stats, nstats, nstreams, names, data, stream_nbytes, 0, INT64_MAX - 1);
}
int gdbamd_import_cells_device_rows(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int treat_deletions_as_intervals,
                                    int64_t column_begin, int64_t column_end, uint8_t** cells, uint64_t* nbytes, int64_t* ncells, int device,
                                    uint64_t text_budget_bytes, int inflate_mode, double* stats, int nstats, int nstreams, const char* const* names,
                                    const void* const* data, const uint64_t* stream_nbytes, int64_t lb_callset_row_idx, int64_t ub_callset_row_idx) {
  try {
    if (!vid_mapping_file || !callset_mapping_file || !cells || !nbytes) throw GenomicsDBConfigException("gdbamd_import_cells_device: null argument");
    if (nstreams < 0 || (nstreams > 0 && (!names || !data || !stream_nbytes))) throw GenomicsDBConfigException("gdbamd_import_cells_device_streams: null stream arrays");
    std::vector<ImportStream> streams;
    for (int i = 0; i < nstreams; ++i) {
      if (!names[i]) throw GenomicsDBConfigException("gdbamd_import_cells_device_streams: null stream name");
      ImportStream s;
      s.name = names[i]; s.data = data[i]; s.nbytes = stream_nbytes[i];
      streams.push_back(s);
    }
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(callset_mapping_file));
    ImportOptions opt;
    opt.treat_deletions_as_intervals = treat_deletions_as_intervals != 0;
    opt.column_begin = column_begin;
    opt.column_end = column_end;
    if (file_root) opt.file_root = file_root;
    opt.row_begin = lb_callset_row_idx;
    opt.row_end = ub_callset_row_idx;
    ImportStats st;
    const std::vector<uint8_t> out = import_callsets_to_cells_device(vid, opt, device, text_budget_bytes, &st, inflate_mode, streams);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!*cells) throw GenomicsDBConfigException("out of memory");
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *nbytes = out.size();
    if (ncells) *ncells = st.num_cells;
    if (stats && nstats > 0) {
      const double v[GDBAMD_IMPORT_NUM_STATS_EX] = {(double)st.num_files, (double)st.num_records, (double)st.num_cells, (double)st.num_spanning_cells, (double)st.num_bytes,
                                                    (double)st.num_deferred_values, (double)st.num_batches, (double)st.text_bytes, st.ms_index, st.ms_measure, st.ms_write,
                                                    st.ms_sort_gather, st.s_read, st.s_h2d, st.s_deferred, st.s_d2h, st.s_total,
                                                    (double)st.compressed_bytes, (double)st.num_device_members, (double)st.num_host_inflated_files, st.ms_inflate, (double)st.bytes_h2d};
      memcpy(stats, v, sizeof(double) * (size_t)std::min<int>(nstats, GDBAMD_IMPORT_NUM_STATS_EX));
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_merge_cells(int nstreams, const void* const* data, const uint64_t* nbytes, uint8_t** cells, uint64_t* out_nbytes, int64_t* ncells, int device, double* stats,
                       int nstats) {
  try {
    if (nstreams <= 0 || !data || !nbytes || !cells || !out_nbytes) throw GenomicsDBConfigException("gdbamd_merge_cells: null argument or no stream");
    std::vector<CellStream> streams((size_t)nstreams);
    for (int i = 0; i < nstreams; ++i) { streams[(size_t)i].data = data[i]; streams[(size_t)i].nbytes = nbytes[i]; }
    MergeStats st;
    const std::vector<uint8_t> out = merge_cell_streams_device(streams, device, &st);
    *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
    if (!*cells) throw GenomicsDBConfigException("out of memory");
    if (!out.empty()) memcpy(*cells, out.data(), out.size());
    *out_nbytes = out.size();
    if (ncells) *ncells = st.cells_out;
    if (stats && nstats > 0) {
      const double v[GDBAMD_MERGE_NUM_STATS] = {(double)st.num_streams, (double)st.cells_in, (double)st.cells_out, (double)st.bytes_out, (double)st.tile,
                                                st.ms_keys, st.ms_rank, st.ms_scan, st.ms_gather, st.s_h2d, st.s_d2h, st.s_total};
      memcpy(stats, v, sizeof(double) * (size_t)std::min<int>(nstats, GDBAMD_MERGE_NUM_STATS));
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int64_t gdbamd_merge_cell_files(int nsources, const char* const* paths, const void* const* data, const uint64_t* nbytes, const char* output_path, int device,
                                uint64_t window_bytes, double* stats, int nstats) {
  try {
    if (nsources <= 0 || !output_path || !*output_path) throw GenomicsDBConfigException("gdbamd_merge_cell_files: no source or no output path");
    std::vector<CellSource> sources((size_t)nsources);
    for (int i = 0; i < nsources; ++i) {
      CellSource& s = sources[(size_t)i];
      if (paths && paths[i]) { s.path = paths[i]; if (s.path.empty()) throw GenomicsDBConfigException("gdbamd_merge_cell_files: empty path"); continue; }
      if (!nbytes || (nbytes[i] && (!data || !data[i]))) throw GenomicsDBConfigException("gdbamd_merge_cell_files: source " + std::to_string(i) + " has neither a path nor data");
      s.data = data ? data[i] : nullptr; s.nbytes = nbytes[i];
    }
    MergeFilesOptions opt;
    opt.device = device; opt.window_bytes = window_bytes;
    MergeFilesStats st;
    const uint64_t cells = merge_cell_files_device(sources, output_path, opt, &st);
    if (stats && nstats > 0) {
      const double v[GDBAMD_MERGE_FILES_NUM_STATS] = {(double)st.num_streams, (double)st.cells_in, (double)st.cells_out, (double)st.bytes_out, (double)st.tile,
                                                      st.ms_keys, st.ms_rank, st.ms_scan, st.ms_gather, st.s_h2d, st.s_d2h, st.s_total,
                                                      (double)st.rounds, (double)st.carried_cells, (double)st.grown, (double)st.window_bytes, (double)st.device_bytes_peak,
                                                      (double)st.pinned_bytes, st.s_read, st.s_write, st.s_wait_device};
      memcpy(stats, v, sizeof(double) * (size_t)std::min<int>(nstats, GDBAMD_MERGE_FILES_NUM_STATS));
    }
    g_last_error.clear();
    return (int64_t)cells;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_split_files_device(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int npartitions, const int64_t* begins,
                              const int64_t* ends, int produce, const char* results_directory, const char* single_output_name, int device,
                              uint64_t text_budget_bytes, int inflate_mode, int nextra, const char* const* extra_paths, double* stats, int nstats, char** outputs) {
  return gdbamd_split_files_device_index(vid_mapping_file, callset_mapping_file, file_root, npartitions, begins, ends, produce, results_directory, single_output_name, device,
                                         text_budget_bytes, inflate_mode, nextra, extra_paths, stats, std::min<int>(nstats, GDBAMD_SPLIT_NUM_STATS), outputs, 0);
}
int gdbamd_split_files_device_index(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int npartitions, const int64_t* begins,
                                    const int64_t* ends, int produce, const char* results_directory, const char* single_output_name, int device,
                                    uint64_t text_budget_bytes, int inflate_mode, int nextra, const char* const* extra_paths, double* stats, int nstats, char** outputs,
                                    int index_on_device) {
  try {
    if (!vid_mapping_file || !callset_mapping_file || npartitions <= 0 || !begins || !ends) throw GenomicsDBConfigException("gdbamd_split_files_device: null argument or no partition");
    if (nextra < 0 || (nextra > 0 && !extra_paths)) throw GenomicsDBConfigException("gdbamd_split_files_device: null extra_paths");
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(callset_mapping_file));
    SplitRequest req;
    for (int i = 0; i < npartitions; ++i) req.partitions.emplace_back(begins[i], ends[i]);
    if (produce >= 0) req.produce.push_back(produce);
    if (file_root) req.file_root = file_root;
    if (results_directory) req.results_directory = results_directory;
    if (single_output_name) req.single_output = single_output_name;
    for (int i = 0; i < nextra; ++i) { if (!extra_paths[i]) throw GenomicsDBConfigException("gdbamd_split_files_device: null extra path"); req.extra_paths.push_back(extra_paths[i]); }
    req.device = device; req.text_budget_bytes = text_budget_bytes; req.inflate_mode = inflate_mode;
    req.index_on_device = index_on_device != 0;
    SplitStats st;
    const std::vector<SplitOutput> done = split_files_device(vid, req, &st);
    if (outputs) {
      std::string text;
      for (const SplitOutput& o : done) text += o.original + "\t" + std::to_string(o.partition) + "\t" + o.path + "\n";
      *outputs = (char*)malloc(text.size() + 1);
      if (!*outputs) throw GenomicsDBConfigException("out of memory");
      memcpy(*outputs, text.c_str(), text.size() + 1);
    }
    if (stats && nstats > 0) {
      const double v[GDBAMD_SPLIT_INDEX_NUM_STATS] = {(double)st.num_files, (double)st.num_record_lines, (double)st.num_lines_written, (double)st.text_bytes_in, (double)st.text_bytes_out,
                                                (double)st.compressed_bytes_out, (double)st.num_batches, st.ms_index, st.ms_classify, st.ms_scan_gather, st.ms_deflate,
                                                st.s_read, st.s_h2d, st.s_d2h_write, st.s_index_build, st.s_total, st.ms_inflate, st.ms_index_kernels};
      memcpy(stats, v, sizeof(double) * (size_t)std::min<int>(nstats, GDBAMD_SPLIT_INDEX_NUM_STATS));
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_index_vcf_device(const char* path, int device, uint64_t text_budget_bytes, gdbamd_index_stats* stats) {
  try {
    if (!path) throw GenomicsDBConfigException("gdbamd_index_vcf_device: null path");
    IndexStats st;
    index_vcf_device(path, device, text_budget_bytes, &st);
    if (stats) {
      stats->members = st.members; stats->batches = st.batches; stats->lines = st.lines; stats->records = st.records;
      stats->contigs = st.contigs; stats->bins = st.bins; stats->chunks = st.chunks; stats->linear_windows = st.linear_windows;
      stats->text_bytes = st.text_bytes; stats->atomics = st.atomics;
      stats->ms_inflate = st.ms_inflate; stats->ms_index = st.ms_index; stats->ms_records = st.ms_records; stats->ms_chunks = st.ms_chunks; stats->ms_linear = st.ms_linear;
      stats->s_read = st.s_read; stats->s_serialize_write = st.s_serialize_write; stats->s_total = st.s_total;
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int gdbamd_input_histogram(const char* vid_mapping_file, const char* callset_mapping_file, const char* file_root, int64_t max_histogram_range, uint64_t num_bins,
                           int64_t column_begin, int64_t column_end, int64_t lb_callset_row_idx, int64_t ub_callset_row_idx, int device,
                           uint64_t text_budget_bytes, int inflate_mode, int nstreams, const char* const* names, const void* const* data,
                           const uint64_t* stream_nbytes, uint64_t* counts, gdbamd_histogram_stats* stats) {
  try {
    if (!vid_mapping_file || !callset_mapping_file || !counts) throw GenomicsDBConfigException("gdbamd_input_histogram: null argument");
    if (nstreams < 0 || (nstreams > 0 && (!names || !data || !stream_nbytes))) throw GenomicsDBConfigException("gdbamd_input_histogram: null stream arrays");
    InputHistogramRequest req;
    for (int i = 0; i < nstreams; ++i) {
      if (!names[i]) throw GenomicsDBConfigException("gdbamd_input_histogram: null stream name");
      ImportStream s;
      s.name = names[i]; s.data = data[i]; s.nbytes = stream_nbytes[i];
      req.streams.push_back(s);
    }
    VidMapper vid;
    vid.parse_vid_json(mini_json::parse_file(vid_mapping_file));
    vid.parse_callsets_json(mini_json::parse_file(callset_mapping_file));
    req.max_histogram_range = max_histogram_range; req.num_bins = num_bins;
    req.column_begin = column_begin; req.column_end = column_end;
    req.row_begin = lb_callset_row_idx; req.row_end = ub_callset_row_idx;
    if (file_root) req.file_root = file_root;
    req.device = device; req.text_budget_bytes = text_budget_bytes; req.inflate_mode = inflate_mode;
    InputHistogramStats st;
    const std::vector<uint64_t> out = input_histogram_device(vid, req, &st);
    memcpy(counts, out.data(), out.size() * sizeof(uint64_t));
    if (stats) {
      stats->num_files = st.num_files; stats->num_records = st.num_records; stats->num_counted = st.num_counted; stats->total_weight = st.total_weight;
      stats->num_batches = st.num_batches; stats->num_atomics = st.num_atomics;
      stats->ms_index = st.ms_index; stats->ms_inflate = st.ms_inflate; stats->ms_histogram = st.ms_histogram;
      stats->s_read = st.s_read; stats->s_h2d = st.s_h2d; stats->s_total = st.s_total;
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
int64_t gdbamd_histogram_text(const uint64_t* counts, uint64_t num_bins, int64_t max_histogram_range, char* dst, uint64_t cap) {
  if (!counts || num_bins == 0 || max_histogram_range < 0) return -1;
  const std::string out = histogram_text(counts, num_bins, (uint64_t)max_histogram_range);
  if (dst && cap) { const size_t n = std::min<size_t>(out.size(), (size_t)cap); memcpy(dst, out.data(), n); }
  return (int64_t)out.size();
}
int gdbamd_vcfdiff(const char* gold, const char* test, double threshold, const char* regions, int device, uint64_t text_budget_bytes, char** report_json,
                   gdbamd_vcfdiff_stats* stats) {
  try {
    if (!gold || !test || !report_json) throw GenomicsDBConfigException("gdbamd_vcfdiff: null argument");
    VcfDiffRequest req;
    req.gold = gold; req.test = test; req.threshold = threshold;
    if (regions) req.regions = regions;
    req.device = device; req.text_budget_bytes = text_budget_bytes;
    VcfDiffStats st;
    const VcfDiffReport rep = vcfdiff_device(req, &st);
    char* out = (char*)malloc(rep.json.size() + 1);
    if (!out) throw GenomicsDBConfigException("gdbamd_vcfdiff: out of memory");
    memcpy(out, rep.json.c_str(), rep.json.size() + 1);
    *report_json = out;
    if (stats) {
      stats->gold_records = st.gold_records; stats->test_records = st.test_records;
      stats->pairs_compared = st.pairs_compared; stats->pairs_light = st.pairs_light; stats->pairs_heavy = st.pairs_heavy;
      stats->deferred = st.deferred; stats->events = st.events; stats->num_batches = st.num_batches; stats->resident_bytes = st.resident_bytes;
      stats->ms_index = st.ms_index; stats->ms_inflate = st.ms_inflate; stats->ms_keys = st.ms_keys; stats->ms_compare = st.ms_compare;
      stats->s_read = st.s_read; stats->s_walk = st.s_walk; stats->s_total = st.s_total;
    }
    g_last_error.clear();
    return 0;
  } catch (const std::exception& e) { g_last_error = e.what(); return -1; }
}
// ---- the streaming importer (api/genomicsdb_importer.h)
void* gdbamd_importer_create(const char* loader_json, int rank, int device) {
  return guarded([&]() -> void* {
    if (!loader_json) throw GenomicsDBConfigException("gdbamd_importer_create: null loader JSON");
    return new GenomicsDBImporter(loader_json, rank, device);
  }, (void*)nullptr);
}
static GenomicsDBImporter& importer_of(void* h) {
  if (!h) throw GenomicsDBConfigException("null importer handle");
  return *static_cast<GenomicsDBImporter*>(h);
}
int gdbamd_importer_add_buffer_stream(void* h, const char* name, int is_bcf, uint64_t capacity, const uint8_t* init, uint64_t init_nbytes) {
  return guarded([&] {
    if (!name) throw GenomicsDBConfigException("gdbamd_importer_add_buffer_stream: null name");
    importer_of(h).add_buffer_stream(name, is_bcf ? BCF_BUFFER_STREAM_TYPE : VCF_BUFFER_STREAM_TYPE, (size_t)capacity, init, (size_t)init_nbytes);
    return 0;
  }, -1);
}
int gdbamd_importer_setup_loader(void* h, const char* callsets_json, int64_t* max_identifiers) {
  return guarded([&] {
    GenomicsDBImporter& imp = importer_of(h);
    imp.setup_loader(callsets_json ? callsets_json : "");
    if (max_identifiers) *max_identifiers = (int64_t)imp.get_max_num_buffer_stream_identifiers();
    return 0;
  }, -1);
}
int gdbamd_importer_stream_file_idx(void* h, int64_t stream_idx, int64_t* file_idx) {
  return guarded([&] {
    const std::vector<int64_t>& v = importer_of(h).get_buffer_stream_idx_to_global_file_idx_vec();
    if (stream_idx < 0 || (size_t)stream_idx >= v.size() || !file_idx) throw GenomicsDBConfigException("gdbamd_importer_stream_file_idx: no such stream");
    *file_idx = v[(size_t)stream_idx];
    return 0;
  }, -1);
}
int gdbamd_importer_write(void* h, int64_t stream_idx, unsigned partition_idx, const uint8_t* data, uint64_t nbytes) {
  return guarded([&] { importer_of(h).write_data_to_buffer_stream(stream_idx, partition_idx, data, (size_t)nbytes); return 0; }, -1);
}
int gdbamd_importer_import_batch(void* h, uint8_t** cells, uint64_t* nbytes, int64_t* exhausted_pairs, int64_t* n_exhausted) {
  return guarded([&] {
    GenomicsDBImporter& imp = importer_of(h);
    if (cells && !nbytes) throw GenomicsDBConfigException("gdbamd_importer_import_batch: cells without nbytes");
    if (!exhausted_pairs || !n_exhausted) throw GenomicsDBConfigException("gdbamd_importer_import_batch: null exhausted arrays");
    imp.import_batch();
    const std::vector<uint8_t>& out = imp.last_batch_cells();
    if (cells) {
      *cells = (uint8_t*)malloc(out.size() ? out.size() : 1);
      if (!*cells) throw GenomicsDBConfigException("out of memory");
      if (!out.empty()) memcpy(*cells, out.data(), out.size());
    }
    if (nbytes) *nbytes = out.size();
    const std::vector<BufferStreamIdentifier>& ex = imp.get_exhausted_buffer_stream_identifiers();
    for (size_t i = 0; i < ex.size(); ++i) { exhausted_pairs[2 * i] = ex[i].first; exhausted_pairs[2 * i + 1] = (int64_t)ex[i].second; }
    *n_exhausted = (int64_t)ex.size();
    return 0;
  }, -1);
}
int gdbamd_importer_is_done(void* h) { return guarded([&] { return importer_of(h).is_done() ? 1 : 0; }, -1); }
int gdbamd_importer_finish(void* h) { return guarded([&] { importer_of(h).finish(); return 0; }, -1); }
int gdbamd_importer_stats(void* h, double* stats) {
  return guarded([&] {
    if (!stats) throw GenomicsDBConfigException("gdbamd_importer_stats: null stats");
    const StreamImportStats& st = importer_of(h).stats();
    const double v[GDBAMD_IMPORTER_NUM_STATS] = {(double)st.num_batches, (double)st.num_records, (double)st.num_cells, (double)st.num_bytes, (double)st.max_pending_cells,
                                                 (double)st.max_pending_bytes, (double)st.num_deferred_values, (double)st.num_spanning_cells, st.ms_order, st.ms_classify,
                                                 st.ms_sort_gather, st.ms_compact, st.s_h2d, st.s_d2h};
    memcpy(stats, v, sizeof(v));
    return 0;
  }, -1);
}
void gdbamd_importer_destroy(void* h) { delete static_cast<GenomicsDBImporter*>(h); }
int gdbamd_chromosome_intervals_for_column_partition(const char* loader_json, int rank, char** json) {
  return guarded([&] {
    if (!loader_json || !json) throw GenomicsDBConfigException("gdbamd_chromosome_intervals_for_column_partition: null argument");
    const std::string text = chromosome_intervals_for_column_partition(loader_json, rank);
    *json = (char*)malloc(text.size() + 1);
    if (!*json) throw GenomicsDBConfigException("out of memory");
    memcpy(*json, text.c_str(), text.size() + 1);
    return 0;
  }, -1);
}
void gdbamd_free(void* p) { free(p); }

}  // extern "C"
