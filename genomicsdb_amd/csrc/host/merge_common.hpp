// merge_common.hpp - the host's share of the cell-stream merge (kernels/gdb_merge.hip), without HIP types so that the CPU harness of
// the bodies (tests/hostsim_merge) runs the same code: the walk over a stream's size chain and the words of the refusals.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../core/gdb_merge.hpp"
#include "vcf_importer.h"

namespace genomicsdb_amd {

// the byte offsets of the cells of stream `stream_idx`, each plus `base`, appended to offs.  A chain that does not end exactly at the
// stream's last byte refuses the stream
inline void merge_walk_cells(const uint8_t* data, uint64_t nbytes, size_t stream_idx, uint64_t base, std::vector<uint64_t>& offs) {
  const std::string who = "merge: stream " + std::to_string(stream_idx);
  if (!data && nbytes) throw VCF2BinaryException(who + ": null data");
  uint64_t at = 0;
  while (at < nbytes) {
    if (nbytes - at < gdbmerge::kMergeHeaderBytes)
      throw VCF2BinaryException(who + ": the size chain runs past the end of the stream: a cell header at byte offset " + std::to_string(at) + " of " +
                                std::to_string(nbytes) + " bytes");
    const uint64_t size = gdbmerge::merge_load_u64(data + at + 16);
    if (size < gdbmerge::kMergeHeaderBytes)
      throw VCF2BinaryException(who + ": cell_size " + std::to_string(size) + " at byte offset " + std::to_string(at) + " is smaller than a cell header");
    if (size > nbytes - at)
      throw VCF2BinaryException(who + ": the size chain runs past the end of the stream: the cell at byte offset " + std::to_string(at) + " has cell_size " +
                                std::to_string(size) + ", the stream " + std::to_string(nbytes) + " bytes");
    offs.push_back(base + at);
    at += size;
  }
}

inline std::string merge_unsorted_message(size_t stream_idx, uint64_t cell) {
  return "merge: stream " + std::to_string(stream_idx) + " is not sorted by (column, row): cell " + std::to_string(cell) + " comes before cell " +
         std::to_string(cell - 1);
}
inline std::string merge_shared_row_message(uint64_t row) {
  return "merge: row " + std::to_string(row) + " is in more than one stream: the streams of a merge hold disjoint sets of rows (it is the smallest shared row)";
}

}  // namespace genomicsdb_amd
