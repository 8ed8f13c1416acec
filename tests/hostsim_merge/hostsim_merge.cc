// hostsim_merge.cc - CPU harness around the GDB_HD bodies of the cell-stream merge (core/gdb_merge.hpp) and the host's walk over the
// size chain (host/merge_common.hpp): the very functions kernels/gdb_merge.hip runs, driven tile by tile as the rank kernel drives
// them.  Test infrastructure only.  With -DHOSTSIM_MERGE_MAIN the same file is a stand-alone program (built with the address and
// undefined-behaviour sanitizers) that checks the bodies against std::stable_sort on seeded inputs and exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_merge.hpp"
#include "../../genomicsdb_amd/csrc/host/merge_common.hpp"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbmerge;

namespace {
// what k_merge_rank does, one "workgroup" after the other: src[pos] = index of the cell at output position pos (B's cells counted from na)
void merge_by_tiles(const MergeKey* A, uint64_t na, const MergeKey* B, uint64_t nb, uint64_t* src) {
  const uint64_t total = na + nb, tiles = (total + kMergeTile - 1) / kMergeTile;
  std::vector<MergeKey> keys(kMergeTile);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    const MergeTile t = merge_tile_of(tile, A, na, B, nb);
    const uint32_t n = t.na + t.nb;
    for (uint32_t i = 0; i < n; ++i) keys[i] = i < t.na ? A[t.a0 + i] : B[t.b0 + (i - t.na)];
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t pos = merge_tile_position(keys.data(), t, i);
      src[tile * kMergeTile + pos] = i < t.na ? t.a0 + i : na + t.b0 + (i - t.na);
    }
  }
}
}  // namespace

extern "C" {

int hm_tile() { return (int)kMergeTile; }

// keys and sizes of the n cells at off[] of `bytes` (headers at any alignment); keys as (col, row) pairs
void hm_keys(const uint8_t* bytes, const uint64_t* off, uint64_t n, int64_t* keys, uint64_t* size) {
  for (uint64_t i = 0; i < n; ++i) {
    MergeKey k;
    merge_load_header(bytes + off[i], &k, &size[i]);
    keys[2 * i] = k.col; keys[2 * i + 1] = k.row;
  }
}

uint64_t hm_split(uint64_t diag, const int64_t* a, uint64_t na, const int64_t* b, uint64_t nb) {
  return merge_path_split(diag, (const MergeKey*)a, na, (const MergeKey*)b, nb);
}

void hm_merge(const int64_t* a, uint64_t na, const int64_t* b, uint64_t nb, uint64_t* src) {
  merge_by_tiles((const MergeKey*)a, na, (const MergeKey*)b, nb, src);
}

// the cell offsets of a stream -> off (at most cap), returns their number, or -1 with the refusal's text in msg
int64_t hm_walk(const uint8_t* data, uint64_t nbytes, int stream_idx, uint64_t* off, uint64_t cap, char* msg, uint64_t msg_cap) {
  try {
    std::vector<uint64_t> offs;
    merge_walk_cells(data, nbytes, (size_t)stream_idx, 0, offs);
    for (size_t i = 0; i < offs.size() && i < cap; ++i) off[i] = offs[i];
    return (int64_t)offs.size();
  } catch (const std::exception& e) {
    if (msg && msg_cap) { snprintf(msg, (size_t)msg_cap, "%s", e.what()); }
    return -1;
  }
}

}  // extern "C"

#ifdef HOSTSIM_MERGE_MAIN
namespace {
int failures = 0;
void check_merge(const char* what, const std::vector<MergeKey>& A, const std::vector<MergeKey>& B) {
  const uint64_t na = A.size(), nb = B.size();
  std::vector<uint64_t> src(na + nb, ~(uint64_t)0), want(na + nb);
  merge_by_tiles(A.data(), na, B.data(), nb, src.data());
  for (uint64_t i = 0; i < na + nb; ++i) want[i] = i;
  auto key_of = [&](uint64_t i) { return i < na ? A[i] : B[i - na]; };
  std::stable_sort(want.begin(), want.end(), [&](uint64_t x, uint64_t y) { return merge_key_less(key_of(x), key_of(y)); });
  if (src != want) { fprintf(stderr, "MISMATCH %s (na %llu, nb %llu)\n", what, (unsigned long long)na, (unsigned long long)nb); ++failures; }
  for (uint64_t d = 0; d <= na + nb; ++d) {      // every diagonal's split is what the sorted order says
    uint64_t from_a = 0;
    for (uint64_t i = 0; i < d; ++i) from_a += want[i] < na;
    if (merge_path_split(d, A.data(), na, B.data(), nb) != from_a) { fprintf(stderr, "SPLIT %s diag %llu\n", what, (unsigned long long)d); ++failures; break; }
    if (na + nb > 3 * (uint64_t)kMergeTile) d += 37;
  }
}
std::vector<MergeKey> sorted_keys(std::mt19937_64& rng, size_t n, int64_t col_range, int64_t row_lo, int64_t row_hi) {
  std::vector<MergeKey> v(n);
  for (MergeKey& k : v) { k.col = (int64_t)(rng() % (uint64_t)col_range); k.row = row_lo + (int64_t)(rng() % (uint64_t)(row_hi - row_lo + 1)); }
  std::stable_sort(v.begin(), v.end(), merge_key_less);
  return v;
}
}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  const size_t T = kMergeTile, lens[] = {0, 1, T - 1, T, T + 1};
  for (size_t na : lens) for (size_t nb : lens) {
    check_merge("disjoint rows", sorted_keys(rng, na, 50, 0, 9), sorted_keys(rng, nb, 50, 10, 19));
    check_merge("tied keys", sorted_keys(rng, na, 5, 0, 2), sorted_keys(rng, nb, 5, 0, 2));
  }
  {
    std::vector<MergeKey> lo = sorted_keys(rng, 2 * T + 3, 100, 0, 5), hi = sorted_keys(rng, T + 7, 100, 0, 5);
    for (MergeKey& k : hi) k.col += 1000;
    check_merge("all A then B", lo, hi);
    check_merge("all B then A", hi, lo);
    std::vector<MergeKey> even, odd;
    for (int64_t i = 0; i < (int64_t)(2 * T + 1); ++i) { MergeKey k; k.col = i; k.row = i & 1; ((i & 1) ? odd : even).push_back(k); }
    check_merge("alternation", even, odd);
    std::vector<MergeKey> runs(3 * T, MergeKey{7, 3}), other = sorted_keys(rng, T + 1, 14, 4, 6);
    check_merge("long runs of equal keys", runs, other);
    check_merge("long runs of equal keys, B", other, runs);
  }
  {
    // headers at every alignment, and the chain walk over them; a truncated chain is refused
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<MergeKey> keys;
    for (int i = 0; i < 40; ++i) {
      const uint64_t size = 24 + (uint64_t)(i % 19);
      MergeKey k; k.col = (int64_t)(rng() >> 1) * ((i & 1) ? -1 : 1); k.row = (int64_t)(rng() >> 1);
      off.push_back(bytes.size()); keys.push_back(k);
      bytes.resize(bytes.size() + size, (uint8_t)i);
      memcpy(&bytes[off.back()], &k.row, 8); memcpy(&bytes[off.back() + 8], &k.col, 8); memcpy(&bytes[off.back() + 16], &size, 8);
    }
    std::vector<uint8_t> exact(bytes);      // (an exact-size heap block: the sanitizer sees a read past the last header)
    std::vector<uint64_t> walked;
    merge_walk_cells(exact.data(), exact.size(), 0, 0, walked);
    if (walked != off) { fprintf(stderr, "WALK\n"); ++failures; }
    for (size_t i = 0; i < off.size(); ++i) {
      MergeKey k; uint64_t size = 0;
      merge_load_header(exact.data() + off[i], &k, &size);
      if (k.col != keys[i].col || k.row != keys[i].row || size != 24 + (uint64_t)(i % 19)) { fprintf(stderr, "HEADER %zu\n", i); ++failures; }
    }
    for (size_t cut : {(size_t)1, (size_t)23, (size_t)25, exact.size() - 1}) {
      std::vector<uint8_t> part(exact.begin(), exact.begin() + (ptrdiff_t)cut);
      bool refused = false;
      try { std::vector<uint64_t> o; merge_walk_cells(part.data(), part.size(), 3, 0, o); } catch (const VCF2BinaryException& e) { refused = strstr(e.what(), "stream 3") != nullptr; }
      if (!refused) { fprintf(stderr, "TRUNCATED %zu\n", cut); ++failures; }
    }
  }
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("hostsim_merge: ok\n");
  return 0;
}
#endif
