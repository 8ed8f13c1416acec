// gdb_merge.hpp - bodies of the cell-stream merge (kernels/gdb_merge.hip): two streams of begin-cells, each sorted by
// (column, row), become one.  Plain functions that compile under g++ and hipcc (GDB_HD); tests/hostsim_merge runs them on the CPU.
//
// The merge is schema-agnostic: of a cell it reads the 24-byte header [row i64][col i64][cell_size u64] and nothing else.
//   key     (column, row) as two signed 64-bit words: the full range of both, no packing assumption
//   order   column first, then row; equal keys of one stream keep their order, and on a tie between the two sides the cell of
//           side A (the earlier stream) comes first - that rule makes the merge a total function
//   rank    merge path: output positions [d0, d1) of a tile are made of A[a0, a1) and B[d0 - a0, d1 - a1), where a = the split of
//           diagonal d (merge_path_split, a binary search over the two key arrays).  Inside a tile an element's position is its own
//           index plus the number of elements of the OTHER side that come before it (merge_rank_of_a / merge_rank_of_b), searched
//           in the tile's keys only - on the device those are in LDS.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gdb_types.h"

namespace genomicsdb_amd {
namespace gdbmerge {

constexpr uint32_t kMergeBlock = 256;                 // threads of a rank workgroup: 4 wavefronts
constexpr uint32_t kMergeTile = 1024;                 // output cells per workgroup; its keys (16 B each) take 16 KiB of LDS
constexpr uint32_t kMergeHeaderBytes = 24;

struct MergeKey { int64_t col, row; };

GDB_HD bool merge_key_less(const MergeKey& a, const MergeKey& b) { return a.col != b.col ? a.col < b.col : a.row < b.row; }

// the header of the cell at p, which has no alignment: on the host byte loads assembled little-endian, on the device unaligned 8-byte loads
GDB_HD uint64_t merge_load_u64(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint64_t unaligned_u64 __attribute__((aligned(1)));      // gfx950 loads 8 bytes of global memory at any address
  return *reinterpret_cast<const unaligned_u64*>(p);
#else
  uint64_t v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | (uint64_t)p[i];
  return v;
#endif
}
GDB_HD void merge_load_header(const uint8_t* p, MergeKey* key, uint64_t* cell_size) {
  key->row = (int64_t)merge_load_u64(p);
  key->col = (int64_t)merge_load_u64(p + 8);
  *cell_size = merge_load_u64(p + 16);
}

// how many of the first `diag` cells of the merge of A[0, na) and B[0, nb) come from A (0 <= diag <= na + nb)
GDB_HD uint64_t merge_path_split(uint64_t diag, const MergeKey* A, uint64_t na, const MergeKey* B, uint64_t nb) {
  uint64_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (!merge_key_less(B[diag - 1 - mid], A[mid])) lo = mid + 1;      // A[mid] <= B[..]: A's cell is taken first
    else hi = mid;
  }
  return lo;
}

// elements of B[0, nb) that come before `a` of side A: those strictly smaller
GDB_HD uint32_t merge_rank_of_a(const MergeKey& a, const MergeKey* B, uint32_t nb) {
  uint32_t lo = 0, hi = nb;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (merge_key_less(B[mid], a)) lo = mid + 1; else hi = mid; }
  return lo;
}
// elements of A[0, na) that come before `b` of side B: those smaller or equal
GDB_HD uint32_t merge_rank_of_b(const MergeKey& b, const MergeKey* A, uint32_t na) {
  uint32_t lo = 0, hi = na;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (!merge_key_less(b, A[mid])) lo = mid + 1; else hi = mid; }
  return lo;
}

// A tile of the output, as one workgroup sees it: the keys of A[a0, a0 + na) followed by those of B[b0, b0 + nb), na + nb <= kMergeTile
struct MergeTile { uint64_t a0, b0; uint32_t na, nb; };
GDB_HD MergeTile merge_tile_of(uint64_t tile, const MergeKey* A, uint64_t na, const MergeKey* B, uint64_t nb) {
  const uint64_t total = na + nb;
  uint64_t d0 = tile * (uint64_t)kMergeTile, d1 = d0 + kMergeTile;
  if (d0 > total) d0 = total;
  if (d1 > total) d1 = total;
  const uint64_t a0 = merge_path_split(d0, A, na, B, nb), a1 = merge_path_split(d1, A, na, B, nb);
  MergeTile t;
  t.a0 = a0; t.b0 = d0 - a0; t.na = (uint32_t)(a1 - a0); t.nb = (uint32_t)((d1 - a1) - (d0 - a0));
  return t;
}
// position inside the tile of local element i (i < na: of A, else of B); keys = the tile's keys as laid out above
GDB_HD uint32_t merge_tile_position(const MergeKey* keys, const MergeTile& t, uint32_t i) {
  if (i < t.na) return i + merge_rank_of_a(keys[i], keys + t.na, t.nb);
  return (i - t.na) + merge_rank_of_b(keys[i], keys, t.na);
}

// ---- the windowed merge (merge_cell_files_device): a source's resident cells are cut at the round's watermark, the cells below it
// are merged and the rest carried to the other pool
// the cut: how many of the sorted keys K[0, n) lie strictly below `w` - those a round may emit.  Strict, so that a run of keys equal
// to the watermark is never split between two rounds
GDB_HD uint64_t merge_cut_below(const MergeKey* K, uint64_t n, const MergeKey& w) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (merge_key_less(K[mid], w)) lo = mid + 1; else hi = mid; }
  return lo;
}
// the order check across a chunk boundary: the first cell of a refill must not come before the source's previous cell
GDB_HD bool merge_boundary_in_order(const MergeKey& previous, const MergeKey& first_new) { return !merge_key_less(first_new, previous); }
// the carry: a kept cell at byte `off` of its pool, where the source's kept bytes begin at `kept_from`, lies at this byte of the other
// pool, where they begin at `kept_to` (the kept cells of a source are contiguous, so they move as one block)
GDB_HD uint64_t merge_carry_offset(uint64_t off, uint64_t kept_from, uint64_t kept_to) { return off - kept_from + kept_to; }

}  // namespace gdbmerge
}  // namespace genomicsdb_amd
