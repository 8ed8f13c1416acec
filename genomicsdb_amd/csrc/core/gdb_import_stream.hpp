// gdb_import_stream.hpp - bodies of the streaming importer (kernels/gdb_import_stream.hip): what one thread decides about one record
// of a write (order check, last column) and about one pending slot (emit, keep or drop; where a kept slot moves to).  Plain functions
// that compile under g++ and hipcc (GDB_HD): the kernels and the CPU harness tests/hostsim_import_stream/ run the same code.
//
// A pending slot is a cell that a stream delivered and that is not yet handed over: its 64-bit sort key (column << key_row_bits | row,
// all ones: no cell), its size in bytes and its partition-begin tag (0: a cell inside the partition; else (column << seq_bits) |
// sequence number of its record, the value the per-row atomicMax of the measure kernel compares).
//
// With W = the smallest "last delivered column" over all streams that are still open (kColNegInf before a stream's first record,
// kColPosInf when every stream has ended), a cell may leave when its column is strictly below W: the stream that defines W may still
// deliver records at column W itself, and equal (column, row) keys must keep their append order.
#pragma once
#include <cstdint>

#include "gdb_types.h"

namespace genomicsdb_amd {
namespace gdbstr {

constexpr int64_t kColNegInf = INT64_MIN, kColPosInf = INT64_MAX;
constexpr uint64_t kNoCell = ~(uint64_t)0;
constexpr uint64_t kNoError = ~(uint64_t)0;
enum : uint32_t { STR_DROP = 0, STR_KEEP = 1, STR_EMIT = 2 };
enum : uint32_t { STR_ERR_ORDER = 0, STR_ERR_NOT_A_RECORD = 1 };      // the error word: kind << 62 | record of the write (0-based)

GDB_HD uint64_t str_error_word(uint32_t kind, uint32_t record) { return ((uint64_t)kind << 62) | (uint64_t)record; }

// a line of a text write is a record: not empty and not a '#' line (a write holds nothing else)
GDB_HD bool str_text_line_is_record(const char* text, const uint32_t* nl_pos, uint32_t line) {
  const uint32_t begin = line ? nl_pos[line - 1u] + 1u : 0u;
  uint32_t end = nl_pos[line];
  if (end > begin && text[end - 1u] == '\r') --end;
  return end > begin && text[begin] != '#';
}

// record r of a write against the record before it; for the first record that is the stream's last column of the write before.
// col: the measure pass's column per slot, per_line slots per record (every slot of a record holds the record's column, also the
// records the partition filters out).  Returns kNoError or the error word of record r.
GDB_HD uint64_t str_order_check(const int64_t* col, uint32_t per_line, uint32_t r, int64_t last_before, bool is_record) {
  if (!is_record) return str_error_word(STR_ERR_NOT_A_RECORD, r);
  const int64_t mine = col[(uint64_t)r * per_line];
  const int64_t before = r ? col[(uint64_t)(r - 1u) * per_line] : last_before;
  return mine < before ? str_error_word(STR_ERR_ORDER, r) : kNoError;
}

// what becomes of a pending slot at watermark W.  row_best: the per-row choice of the partition-begin rule (may be null without a
// partition begin).  A candidate that is not its row's choice can never become it again (the choice only moves forward), so it is
// dropped at once; the chosen one leaves, at its own coordinates, in the first batch whose W lies behind the partition begin -
// from then on no stream can deliver a record at or before column_begin, so the choice is final.
GDB_HD uint32_t str_classify(uint64_t key, uint64_t tag, int32_t key_row_bits, int64_t max_row, const unsigned long long* row_best, int64_t W, int64_t column_begin) {
  if (key == kNoCell) return STR_DROP;
  const int64_t col = (int64_t)(key >> key_row_bits);
  if (tag) {
    const int64_t row = (int64_t)(key & (((uint64_t)1 << key_row_bits) - 1u));
    if (!row_best || row > max_row || row_best[row] != tag) return STR_DROP;
    return W > column_begin ? STR_EMIT : STR_KEEP;
  }
  return col < W ? STR_EMIT : STR_KEEP;
}

// a kept cell's bytes begin at a multiple of 16 in the pool they move to
GDB_HD uint64_t str_pool_bytes(uint32_t size) { return ((uint64_t)size + 15u) & ~(uint64_t)15u; }

}  // namespace gdbstr
}  // namespace genomicsdb_amd
