// hostsim_import_stream.cc - CPU harness around the bodies of the streaming importer (core/gdb_import_stream.hpp): the per-record
// order check, the per-slot classification and the compaction order run in plain loops where the kernels of
// kernels/gdb_import_stream.hip run them per thread, inside the caller's loop that tests/tools/stream_import_model.py assumes.
// Test infrastructure only: the product links none of this.
//
// A case (text, numbers separated by white space):
//   key_row_bits max_row column_begin column_end n_streams
//   per stream: used n_writes;  per write: n_records;  per record: column n_cells;  per cell: row end size
// The report, one line per batch:
//   W <W> | <column> <row> <size> ... | <exhausted stream> ... | <pending cells> <pending bytes>
// and "ERROR order <stream> <record>" when a stream goes back.  W is printed as -inf / inf at the ends.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_import_stream.hpp"

using namespace genomicsdb_amd::gdbstr;

namespace {
struct Cell { int64_t row, end; uint32_t size; };
struct Record { int64_t col; std::vector<Cell> cells; };
struct Stream { bool used = false; std::vector<std::vector<Record>> writes; size_t next = 0; bool ended = false, reported = false; int64_t last = kColNegInf; uint64_t records = 0; };

std::string run_case(const std::string& text) {
  std::istringstream in(text);
  int key_row_bits = 0, n_streams = 0;
  int64_t max_row = 0, column_begin = 0, column_end = 0;
  in >> key_row_bits >> max_row >> column_begin >> column_end >> n_streams;
  std::vector<Stream> streams((size_t)n_streams);
  for (Stream& s : streams) {
    int used = 0; size_t n_writes = 0;
    in >> used >> n_writes;
    s.used = used != 0; s.reported = s.used; s.ended = !s.used;
    s.writes.resize(n_writes);
    for (auto& w : s.writes) {
      size_t n_rec = 0;
      in >> n_rec;
      w.resize(n_rec);
      for (Record& r : w) {
        size_t n_cells = 0;
        in >> r.col >> n_cells;
        r.cells.resize(n_cells);
        for (Cell& c : r.cells) in >> c.row >> c.end >> c.size;
      }
    }
  }
  if (!in) return "ERROR case\n";
  int col_bits = 0;
  while (col_bits < 63 && (column_begin >> col_bits) != 0) ++col_bits;
  const int seq_bits = 64 - col_bits;
  std::vector<unsigned long long> row_best((size_t)max_row + 1, 0ull);
  // the pending slots, as the device keeps them: two sets of arrays and two pools, used in turn
  struct Slots { std::vector<uint64_t> key, tag, src; std::vector<uint32_t> size; } slots[2];
  std::vector<uint8_t> pool[2];
  int cur = 0;
  uint64_t seq = 0, held_bytes = 0;
  std::ostringstream out;
  for (;;) {
    Slots& P = slots[cur];
    uint64_t held_cells = P.key.size();
    // ---- the writes: measure's share (row_best, kinds) in plain code, the order check by the body
    for (size_t si = 0; si < streams.size(); ++si) {
      Stream& s = streams[si];
      if (s.ended || !s.reported) continue;
      static const std::vector<Record> none;
      const std::vector<Record>& w = s.next < s.writes.size() ? s.writes[s.next] : none;
      ++s.next;
      if (w.empty()) { s.ended = true; s.last = kColPosInf; continue; }
      std::vector<int64_t> col(w.size());
      for (size_t r = 0; r < w.size(); ++r) col[r] = w[r].col;
      uint64_t err = kNoError;
      for (uint32_t r = 0; r < (uint32_t)w.size(); ++r) err = std::min(err, str_order_check(col.data(), 1u, r, s.last, true));
      if (err != kNoError) { out << "ERROR order " << si << " " << s.records + (err & (((uint64_t)1 << 62) - 1u)) + 1u << "\n"; return out.str(); }
      s.last = col.back();
      s.records += w.size();
      for (const Record& r : w) {
        ++seq;
        if (r.col <= column_end && r.col <= column_begin)
          for (const Cell& c : r.cells) row_best[(size_t)c.row] = std::max(row_best[(size_t)c.row], ((unsigned long long)r.col << seq_bits) | seq);
        if (r.col > column_end) continue;
        for (const Cell& c : r.cells) {
          uint64_t tag = 0;
          if (r.col < column_begin) { if (c.end < column_begin) continue; tag = ((uint64_t)r.col << seq_bits) | seq; }
          P.key.push_back(((uint64_t)r.col << key_row_bits) | (uint64_t)c.row);
          P.tag.push_back(tag); P.size.push_back(c.size); P.src.push_back(0);
          ++held_cells; held_bytes += c.size;
        }
      }
    }
    int64_t W = kColPosInf;
    for (const Stream& s : streams) if (!s.ended) W = std::min(W, s.last);
    // ---- classify: the body per slot
    const size_t N = P.key.size();
    std::vector<uint32_t> cls(N);
    for (size_t i = 0; i < N; ++i) cls[i] = str_classify(P.key[i], P.tag[i], key_row_bits, max_row, column_begin > 0 ? row_best.data() : nullptr, W, column_begin);
    // ---- emit: a stable sort of the emit keys
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < N; ++i) if (cls[i] == STR_EMIT) idx.push_back((uint32_t)i);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return P.key[a] < P.key[b]; });
    if (W == kColPosInf) out << "W inf |"; else if (W == kColNegInf) out << "W -inf |"; else out << "W " << W << " |";
    for (uint32_t i : idx) out << " " << (int64_t)(P.key[i] >> key_row_bits) << " " << (P.key[i] & (((uint64_t)1 << key_row_bits) - 1u)) << " " << P.size[i];
    // ---- compact: exclusive scans of the keep flags and of the pool bytes; the kept slots move, in order, to the other set
    Slots& O = slots[1 - cur];
    O.key.clear(); O.tag.clear(); O.size.clear(); O.src.clear();
    uint64_t dst = 0, doff = 0;
    std::vector<uint64_t> at(N), to(N);
    for (size_t i = 0; i < N; ++i) { at[i] = dst; to[i] = doff; if (cls[i] == STR_KEEP) { ++dst; doff += str_pool_bytes(P.size[i]); } }
    pool[1 - cur].assign((size_t)doff, 0);
    O.key.resize((size_t)dst); O.tag.resize((size_t)dst); O.size.resize((size_t)dst); O.src.resize((size_t)dst);
    for (size_t i = 0; i < N; ++i) {
      if (cls[i] != STR_KEEP) continue;
      O.key[(size_t)at[i]] = P.key[i]; O.tag[(size_t)at[i]] = P.tag[i]; O.size[(size_t)at[i]] = P.size[i]; O.src[(size_t)at[i]] = to[i];
      memset(pool[1 - cur].data() + to[i], 0xAB, P.size[i]);      // (the cell's bytes: inside the pool, by the scan)
    }
    P.key.clear(); P.tag.clear(); P.size.clear(); P.src.clear();
    cur = 1 - cur;
    out << " |";
    bool all_ended = true;
    for (size_t si = 0; si < streams.size(); ++si) {
      Stream& s = streams[si];
      s.reported = !s.ended && s.last <= W;
      if (s.reported) out << " " << si;
      all_ended = all_ended && s.ended;
    }
    out << " | " << held_cells << " " << held_bytes << "\n";
    held_bytes = doff;
    if (all_ended && dst == 0) break;
  }
  return out.str();
}
}  // namespace

extern "C" {
// -> bytes of the report (the first `cap` are written to out)
uint64_t hostsim_import_stream_run(const char* case_text, char* out, uint64_t cap) {
  const std::string r = run_case(case_text);
  if (out && cap) memcpy(out, r.data(), (size_t)std::min<uint64_t>(cap, r.size()));
  return r.size();
}
}

#ifdef HOSTSIM_IMPORT_STREAM_MAIN
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: hostsim_import_stream_main <case file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
  fclose(f);
  const std::string r = run_case(text);
  fwrite(r.data(), 1, r.size(), stdout);
  return r.compare(0, 10, "ERROR case") == 0 ? 1 : 0;
}
#endif
