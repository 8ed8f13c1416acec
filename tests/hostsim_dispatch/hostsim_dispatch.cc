// hostsim_dispatch.cc - the decision of kernels/gdb_assembly_choice.hpp driven the way prepare_interval and begin_page drive it, on the
// CPU: knob strings and an interval's record sizes in, the paging and the IntervalStats figures out (tests/test_assembly_choice_cpu.py).
#include <cstring>
#include <vector>

#include "../../genomicsdb_amd/csrc/kernels/gdb_assembly_choice.hpp"

using namespace genomicsdb_amd;

namespace {
const char* const* g_names; const char* const* g_values; int g_nknobs;   // what the reader's look-up answers from (one caller at a time)
const char* lookup(const char* name) {
  for (int i = 0; i < g_nknobs; ++i) if (!strcmp(name, g_names[i])) return g_values[i];
  return nullptr;
}
}

// names / values: nknobs knobs by their full GDBAMD_* name (a null value: unset).  rec_bytes: the bytes of the interval's P records.
// out: {pages, page_kernel of the last page, resolved_entry_bytes; of the last page: run, forks, resolve_kernel, res_rows; frun, chunk_major,
//       xcd_aware, page_priority (-1: unset)}
extern "C" void hostsim_dispatch(const char* const* names, const char* const* values, int nknobs, const uint64_t* rec_bytes, int64_t P, int32_t N,
                                 int bcf, int untabled, int any_over255, uint64_t arena_bytes, int64_t* out) {
  g_names = names; g_values = values; g_nknobs = nknobs;
  const AssemblyKnobs knobs = read_assembly_knobs(lookup);
  const AssemblySizing sz = choose_sizing(knobs, IntervalFacts{bcf != 0, P, N, untabled != 0, any_over255 != 0});
  const int nchunks = (N + kAsmRows - 1) / kAsmRows;
  std::vector<uint64_t> rec_off((size_t)P + 1, 0);
  uint64_t max_record = 0;
  for (int64_t k = 0; k < P; ++k) { rec_off[(size_t)k + 1] = rec_off[(size_t)k] + rec_bytes[k]; max_record = std::max(max_record, rec_bytes[k]); }
  const uint64_t total = rec_off[(size_t)P], arena_cap = std::max(arena_bytes, max_record);
  int64_t pages = 0;
  PageChoice pc{};
  for (int64_t kp = 0; kp < P; ++pages) {   // begin_page, page after page (total: IntervalStats::bytes_out)
    const int64_t ke = kp > 0 || total > arena_cap ? page_end(knobs, sz, rec_off.data(), kp, P, arena_cap) : P;
    pc = choose_page(knobs, sz, kp, ke, P, nchunks, total, max_record, sz.use_events);   // (order_iv is valid whenever the change lists exist)
    kp = ke;
  }
  out[0] = pages; out[1] = pc.code; out[2] = sz.resolved_entry_bytes;
  out[3] = pc.run; out[4] = pc.forks; out[5] = pc.resolve_kernel; out[6] = pc.res_rows;
  out[7] = sz.frun; out[8] = sz.chunk_major; out[9] = knobs.xcd_aware; out[10] = knobs.page_priority;
}
