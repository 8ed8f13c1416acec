// gdb_import_device.hpp - what the translation units that launch kernels over the importer's batches share (kernels/gdb_import.hip, kernels/gdb_split.hip):
// the launch constants, a batch's newline / tab index as the kernels read it, the error words, and small device-memory helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "../core/gdb_import.hpp"
#include "gdb_pipeline.h"

namespace genomicsdb_amd {

#define IMP_HIP_CHECK(expr)                                                                                        \
  do {                                                                                                             \
    hipError_t _e = (expr);                                                                                        \
    if (_e != hipSuccess)                                                                                          \
      throw GenomicsDBDeviceException(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

namespace impdev {
using namespace gdbimp;

constexpr int kBlock = 256;              // 4 wavefronts
constexpr int kBytesPerThread = 16;      // one 16-byte load
constexpr uint32_t kTile = kBlock * kBytesPerThread;
constexpr uint32_t kTextPad = 64;        // bytes behind the text that the 16-byte loads may touch
constexpr int kErrWords = 20;            // [0]: ImpErr bits, [1 + b]: smallest line that raised bit b

struct ImpBatch { const char* text; const uint32_t* nl_pos; const uint32_t* line_first_tab; const uint32_t* tab_pos; uint32_t n_lines; };

__device__ __forceinline__ ImpLine imp_line_of(const ImpBatch& B, uint32_t line) {
  ImpLine L;
  L.text = B.text;
  L.begin = line ? B.nl_pos[line - 1u] + 1u : 0u;
  L.end = B.nl_pos[line];
  if (L.end > L.begin && B.text[L.end - 1u] == '\r') --L.end;
  const uint32_t first = B.line_first_tab[line];
  L.tabs = B.tab_pos + first;
  L.ntabs = B.line_first_tab[line + 1u] - first;
  return L;
}

__device__ __forceinline__ void imp_raise(uint32_t* err, uint32_t bits, uint32_t line) {
  atomicOr(&err[0], bits);
  for (uint32_t b = 0; b < (uint32_t)kErrWords - 1u; ++b) if (bits & (1u << b)) atomicMin(&err[1u + b], line);
}

template <class T> struct DBuf {       // grow-only device block
  T* p = nullptr; size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    IMP_HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
  }
  ~DBuf() { if (p) (void)hipFree(p); }
};
template <class T> T* dalloc(size_t n) { T* p = nullptr; IMP_HIP_CHECK(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T))); return p; }

// The importer's newline / tab index pass (defined in gdb_import.hip: k_imp_count, an exclusive scan of the tile counts, k_imp_scatter)
// over n bytes of text that begin 16-byte aligned and have kTextPad bytes allocated behind them: nl[l] = position of the l-th
// newline, tab[] = positions of the tabs, first_tab[l] = tabs in front of line l (n_lines + 1 entries).  Waits for the stream once,
// between the scan and the scatter, for the two totals; the scatter is queued when it returns.  No newline: nothing is scattered.
void index_lines(const char* text, uint32_t n, DBuf<uint64_t>& tile, DBuf<uint64_t>& tile_scan, DBuf<char>& scan_tmp, DBuf<uint32_t>& nl, DBuf<uint32_t>& first_tab,
                 DBuf<uint32_t>& tab, hipStream_t stream, uint32_t* n_lines, uint32_t* n_tabs);

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace impdev
}  // namespace genomicsdb_amd
