// gdb_index_types.h - what a batch of the device tabix builder hands to the host (core/gdb_index.hpp makes it, host/vcf_index.h joins
// the batches): plain data, no device code.
#pragma once
#include <cstdint>

namespace genomicsdb_amd {
namespace gdbidx {

constexpr uint32_t IDX_ERR_POS_LOW = 1u;      // POS below 1
constexpr uint32_t IDX_ERR_RANGE = 2u;        // POS or END at or above 2^31
constexpr uint32_t IDX_CHUNK_FIRST = 1u, IDX_CHUNK_LAST = 2u;      // the chunk holds its contig's first / last record of the batch

struct IdxChunk { uint64_t beg, end; uint32_t tid, bin, flags, count; };      // count: records of the chunk

}  // namespace gdbidx
}  // namespace genomicsdb_amd
