// hostsim_merge_files.cc - CPU harness of the windowed merge (merge_cell_files_device): the sources, the round planner and the round
// loop of host/merge_files_common.hpp - the very code the device path runs - over a backend that keeps the two pools in host memory,
// runs the GDB_HD bodies of core/gdb_merge.hpp (the cut, the boundary order check, the carry's address arithmetic) where the device
// runs them in kernels, and ranks and gathers with a plain loop.  Test infrastructure only.  With -DHOSTSIM_MERGE_FILES_MAIN the same
// file is a stand-alone program (built with the address and undefined-behaviour sanitizers) that merges seeded sources at several
// windows and compares with std::stable_sort; it exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_merge.hpp"
#include "../../genomicsdb_amd/csrc/host/merge_files_common.hpp"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbmerge;

namespace {

struct HostBackend {
  std::vector<uint8_t> pool[2], stage[2], out[2];
  std::vector<uint64_t> t_off[2], t_size[2], stage_off[2];
  std::vector<MergeKey> t_key[2];
  std::vector<std::vector<bool>> rows;       // per source: the rows seen so far
  size_t k = 0;

  void reserve(uint64_t pool_bytes, uint64_t table_cells, size_t sources, int keep) {
    k = sources;
    rows.resize(k);
    for (int set = 0; set < 2; ++set) {
      if (set != keep) { pool[set].resize(pool_bytes); t_off[set].resize(table_cells); t_size[set].resize(table_cells); t_key[set].resize(table_cells); }
      stage[set].resize(pool_bytes); stage_off[set].resize(table_cells);
    }
    want_pool = pool_bytes; want_cells = table_cells;
  }
  uint64_t want_pool = 0, want_cells = 0;
  uint8_t* stage_bytes(int set) { return stage[set].data(); }
  uint64_t* stage_offs(int set) { return stage_off[set].data(); }

  void upload(int set, const MergeRoundLayout& L) {
    for (size_t s = 0; s < k; ++s) {
      if (!L.fresh_cells[s]) continue;
      const uint64_t at = L.rbase[s] + L.kept_bytes[s], row = L.first[s] + L.kept_cells[s];
      memcpy(pool[set].data() + at, stage[set].data() + at, L.fresh_bytes[s]);
      memcpy(t_off[set].data() + row, stage_off[set].data() + row, L.fresh_cells[s] * sizeof(uint64_t));
    }
  }

  MergeCutResult cut(int set, const MergeRoundLayout& L, const MergeWatermark& w, uint64_t max_row) {
    MergeCutResult c(k);
    uint64_t negative_at = kMergeNone;
    for (size_t s = 0; s < k; ++s) {
      if (rows[s].size() < max_row + 1) rows[s].resize(max_row + 1, false);
      const uint64_t row = L.first[s] + L.kept_cells[s];
      for (uint64_t i = 0; i < L.fresh_cells[s]; ++i) {
        const uint64_t g = row + i;
        merge_load_header(pool[set].data() + t_off[set][g], &t_key[set][g], &t_size[set][g]);
        const MergeKey key = t_key[set][g];
        if (key.row < 0) { if (g < negative_at) { negative_at = g; c.negative_source = (int64_t)s; c.negative_cell = i; } }
        else rows[s][(size_t)key.row] = true;
        if (i > 0 && merge_key_less(key, t_key[set][g - 1]) && c.unsorted[s] == kMergeNone) c.unsorted[s] = i;
      }
    }
    for (uint64_t r = 0; r <= max_row && c.shared_row == kMergeNone; ++r) {
      int holders = 0;
      for (size_t s = 0; s < k; ++s) holders += r < rows[s].size() && rows[s][(size_t)r];
      if (holders > 1) c.shared_row = r;
    }
    for (size_t s = 0; s < k; ++s) {
      const uint64_t n = L.cells(s), end = L.rbase[s] + L.bytes(s);
      const uint64_t below = w.all ? n : w.nothing ? 0 : merge_cut_below(t_key[set].data() + L.first[s], n, w.key);
      const uint64_t begin = n ? t_off[set][L.first[s]] : end, cut_at = below < n ? t_off[set][L.first[s] + below] : end;
      c.emit_cells[s] = below; c.emit_bytes[s] = cut_at - begin;
    }
    return c;
  }

  void merge_and_carry(int set, const MergeRoundLayout& L, const MergeCutResult& c, const MergeRoundLayout& next) {
    const int other = set ^ 1;
    pool[other].resize(want_pool); t_off[other].resize(want_cells); t_size[other].resize(want_cells); t_key[other].resize(want_cells);
    // rank and gather, as a plain loop: the smallest head goes first, the earlier source on a tie
    std::vector<uint64_t> head(k, 0);
    std::vector<uint8_t>& o = out[set];
    o.clear();
    for (;;) {
      size_t best = k;
      for (size_t s = 0; s < k; ++s) {
        if (head[s] >= c.emit_cells[s]) continue;
        if (best == k || merge_key_less(t_key[set][L.first[s] + head[s]], t_key[set][L.first[best] + head[best]])) best = s;
      }
      if (best == k) break;
      const uint64_t g = L.first[best] + head[best]++;
      o.insert(o.end(), pool[set].begin() + (ptrdiff_t)t_off[set][g], pool[set].begin() + (ptrdiff_t)(t_off[set][g] + t_size[set][g]));
    }
    for (size_t s = 0; s < k; ++s) {
      const uint64_t n = next.kept_cells[s];
      if (!n) continue;
      const uint64_t from = L.rbase[s] + c.emit_bytes[s], to = next.rbase[s], from_row = L.first[s] + c.emit_cells[s];
      memcpy(pool[other].data() + to, pool[set].data() + from, next.kept_bytes[s]);
      for (uint64_t i = 0; i < n; ++i) {
        t_key[other][next.first[s] + i] = t_key[set][from_row + i];
        t_size[other][next.first[s] + i] = t_size[set][from_row + i];
        t_off[other][next.first[s] + i] = merge_carry_offset(t_off[set][from_row + i], from, to);
      }
    }
  }

  const uint8_t* collect(int set, uint64_t nbytes) {
    if (out[set].size() != nbytes) throw VCF2BinaryException("merge: the merged sizes add up to " + std::to_string(out[set].size()) + " bytes, the round's cells to " + std::to_string(nbytes));
    return out[set].data();
  }
};

uint64_t merge_on_the_host(const std::vector<CellSource>& sources, const std::string& output, uint64_t window, MergeFilesStats& st) {
  MergeFilesPlanner plan(sources, window);
  HostBackend be;
  return merge_files_run(plan, output, be, st);
}

}  // namespace

extern "C" {

// the windowed merge on the CPU.  Source i is the file paths[i], or the memory data[i] when paths[i] is NULL.  Returns the number of
// cells, or -1 with the refusal's text in msg.  stats (5 doubles): rounds, carried cells, growths, window as used, cells in
int64_t hmf_merge(int nsources, const char* const* paths, const void* const* data, const uint64_t* nbytes, const char* output, uint64_t window, double* stats, char* msg,
                  uint64_t msg_cap) {
  try {
    std::vector<CellSource> sources((size_t)nsources);
    for (int i = 0; i < nsources; ++i) {
      if (paths && paths[i]) sources[(size_t)i].path = paths[i];
      else { sources[(size_t)i].data = data[i]; sources[(size_t)i].nbytes = nbytes[i]; }
    }
    MergeFilesStats st;
    const uint64_t cells = merge_on_the_host(sources, output, window, st);
    if (stats) { stats[0] = (double)st.rounds; stats[1] = (double)st.carried_cells; stats[2] = (double)st.grown; stats[3] = (double)st.window_bytes; stats[4] = (double)st.cells_in; }
    return (int64_t)cells;
  } catch (const std::exception& e) {
    if (msg && msg_cap) snprintf(msg, (size_t)msg_cap, "%s", e.what());
    return -1;
  }
}

// the bodies by themselves; keys as (col, row) pairs
uint64_t hmf_cut_below(const int64_t* keys, uint64_t n, int64_t col, int64_t row) { return merge_cut_below((const MergeKey*)keys, n, MergeKey{col, row}); }
int hmf_boundary_in_order(int64_t prev_col, int64_t prev_row, int64_t col, int64_t row) { return merge_boundary_in_order(MergeKey{prev_col, prev_row}, MergeKey{col, row}) ? 1 : 0; }
uint64_t hmf_carry_offset(uint64_t off, uint64_t kept_from, uint64_t kept_to) { return merge_carry_offset(off, kept_from, kept_to); }

}  // extern "C"

#ifdef HOSTSIM_MERGE_FILES_MAIN
namespace {
struct Cell { MergeKey key; std::vector<uint8_t> bytes; };
std::vector<uint8_t> stream_of(std::mt19937_64& rng, size_t n, int64_t cols, int64_t row_lo, int64_t row_hi, size_t max_payload) {
  std::vector<Cell> cells(n);
  for (Cell& c : cells) {
    c.key.col = (int64_t)(rng() % (uint64_t)cols); c.key.row = row_lo + (int64_t)(rng() % (uint64_t)(row_hi - row_lo + 1));
    const uint64_t size = 24 + rng() % (max_payload + 1);
    c.bytes.resize(size);
    for (uint8_t& b : c.bytes) b = (uint8_t)rng();
    memcpy(&c.bytes[0], &c.key.row, 8); memcpy(&c.bytes[8], &c.key.col, 8); memcpy(&c.bytes[16], &size, 8);
  }
  std::stable_sort(cells.begin(), cells.end(), [](const Cell& a, const Cell& b) { return merge_key_less(a.key, b.key); });
  std::vector<uint8_t> out;
  for (const Cell& c : cells) out.insert(out.end(), c.bytes.begin(), c.bytes.end());
  return out;
}
std::vector<uint8_t> expected(const std::vector<std::vector<uint8_t>>& streams) {
  std::vector<Cell> cells;
  for (const auto& s : streams)
    for (uint64_t at = 0; at < s.size();) {
      Cell c; uint64_t size = 0;
      merge_load_header(s.data() + at, &c.key, &size);
      c.bytes.assign(s.begin() + (ptrdiff_t)at, s.begin() + (ptrdiff_t)(at + size));
      cells.push_back(c);
      at += size;
    }
  std::stable_sort(cells.begin(), cells.end(), [](const Cell& a, const Cell& b) { return merge_key_less(a.key, b.key); });
  std::vector<uint8_t> out;
  for (const Cell& c : cells) out.insert(out.end(), c.bytes.begin(), c.bytes.end());
  return out;
}
std::vector<uint8_t> read_all(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string output = dir + "/hostsim_merge_files.out", as_file = dir + "/hostsim_merge_files.in";
  std::mt19937_64 rng(20240917);
  int failures = 0;
  for (int shape = 0; shape < 4; ++shape) {
    std::vector<std::vector<uint8_t>> streams;
    if (shape == 0) { streams.push_back(stream_of(rng, 700, 60, 0, 2, 70)); streams.push_back(stream_of(rng, 500, 60, 3, 4, 70)); }
    if (shape == 1) { streams.push_back(stream_of(rng, 900, 3, 0, 0, 10)); streams.push_back(stream_of(rng, 40, 9, 1, 2, 3000)); streams.push_back(std::vector<uint8_t>()); }
    if (shape == 2) streams.push_back(stream_of(rng, 300, 50, 0, 5, 40));
    if (shape == 3) for (int s = 0; s < 5; ++s) streams.push_back(stream_of(rng, 100 + 37 * (size_t)s, 20, s, s, 33));
    const std::vector<uint8_t> want = expected(streams);
    { FILE* f = fopen(as_file.c_str(), "wb"); if (!f || (streams[0].size() && fwrite(streams[0].data(), 1, streams[0].size(), f) != streams[0].size())) { fprintf(stderr, "cannot write %s\n", as_file.c_str()); return 2; } fclose(f); }
    for (uint64_t window : {(uint64_t)1, (uint64_t)100, (uint64_t)641, (uint64_t)4096, (uint64_t)1 << 20}) {
      for (int first_as_file = 0; first_as_file < 2; ++first_as_file) {
        std::vector<CellSource> sources(streams.size());
        for (size_t s = 0; s < streams.size(); ++s) {
          // (an exact-size heap block per source: the sanitizer sees a read past its end)
          if (s == 0 && first_as_file) sources[s].path = as_file; else { sources[s].data = streams[s].data(); sources[s].nbytes = streams[s].size(); }
        }
        MergeFilesStats st;
        try {
          merge_on_the_host(sources, output, window, st);
          if (read_all(output) != want) { fprintf(stderr, "MISMATCH shape %d window %llu file %d\n", shape, (unsigned long long)window, first_as_file); ++failures; }
        } catch (const std::exception& e) { fprintf(stderr, "REFUSED shape %d window %llu: %s\n", shape, (unsigned long long)window, e.what()); ++failures; }
      }
    }
  }
  remove(output.c_str()); remove(as_file.c_str());
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("hostsim_merge_files: ok\n");
  return 0;
}
#endif
