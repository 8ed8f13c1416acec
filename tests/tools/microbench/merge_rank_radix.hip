// merge_rank_radix.hip - scratch measurement for profiles/device_merge.md, not part of the product: what ranking the cells of
// two sorted streams costs by the importer's route (keys packed as finish() of kernels/gdb_import.hip packs them, concatenated,
// a stable 64-bit rocPRIM radix sort of (key, index) pairs), for the keys of two cell files.  The product ranks by merge path
// (kernels/gdb_merge.hip); its time is the "ms_rank" of merge_cells' statistics.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 merge_rank_radix.hip -o merge_rank_radix
//   merge_rank_radix <array cells.bin> <batch cells.bin> [repetitions]
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 1; } } while (0)

static bool read_keys(const char* path, std::vector<int64_t>& rows, std::vector<int64_t>& cols) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> data((size_t)n);
  const bool ok = n == 0 || fread(data.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  if (!ok) return false;
  for (size_t at = 0; at + 24 <= data.size();) {
    int64_t row, col; uint64_t size;
    memcpy(&row, &data[at], 8); memcpy(&col, &data[at + 8], 8); memcpy(&size, &data[at + 16], 8);
    if (size < 24 || size > data.size() - at) return false;
    rows.push_back(row); cols.push_back(col);
    at += size;
  }
  return true;
}

__global__ void k_iota(uint32_t* v, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: merge_rank_radix <array cells> <batch cells> [repetitions]\n"); return 2; }
  const int reps = argc > 3 ? atoi(argv[3]) : 5;
  std::vector<int64_t> rows, cols;
  if (!read_keys(argv[1], rows, cols) || !read_keys(argv[2], rows, cols)) { fprintf(stderr, "cannot read the cell files\n"); return 1; }
  const size_t n = rows.size();
  int64_t max_row = 0;
  for (int64_t r : rows) max_row = std::max(max_row, r);
  int row_bits = 1;
  while ((max_row >> row_bits) != 0) ++row_bits;
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < n; ++i) keys[i] = ((uint64_t)cols[i] << row_bits) | (uint64_t)rows[i];
  uint64_t *d_key = nullptr, *d_key_sorted = nullptr;
  uint32_t *d_idx = nullptr, *d_idx_sorted = nullptr;
  void* d_tmp = nullptr;
  CHECK(hipMalloc((void**)&d_key, n * 8 + 8)); CHECK(hipMalloc((void**)&d_key_sorted, n * 8 + 8));
  CHECK(hipMalloc((void**)&d_idx, n * 4 + 4)); CHECK(hipMalloc((void**)&d_idx_sorted, n * 4 + 4));
  size_t tmp_bytes = 0;
  CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_key, d_key_sorted, d_idx, d_idx_sorted, n, 0, 64, (hipStream_t)0));
  CHECK(hipMalloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  printf("{\"cells\": %zu, \"row_bits\": %d, \"radix_rank_ms\": [", n, row_bits);
  for (int r = 0; r <= reps; ++r) {      // (run 0 is the warm-up and is not printed)
    CHECK(hipMemcpy(d_key, keys.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_idx, (uint64_t)n);
    CHECK(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_key, d_key_sorted, d_idx, d_idx_sorted, n, 0, 64, (hipStream_t)0));
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) printf("%s%.3f", r > 1 ? ", " : "", ms);
  }
  std::vector<uint64_t> sorted(n);
  CHECK(hipMemcpy(sorted.data(), d_key_sorted, n * 8, hipMemcpyDeviceToHost));
  printf("], \"sorted\": %s}\n", std::is_sorted(sorted.begin(), sorted.end()) ? "true" : "false");
  return 0;
}
