// merge_files_common.hpp - the host's share of the windowed merge (merge_cell_files_device, kernels/gdb_merge.hip), without HIP types
// so that the CPU harness (tests/hostsim_merge_files) runs the same code: the sources (a file read with pread, or memory), the round
// planner (shares, refill, chain walk with source-global offsets, watermark, growth, end condition, the words of every refusal) and
// the round loop itself, merge_files_run, over a backend that holds the pools:
//   Backend::reserve(pool_bytes, table_cells, k, keep)     every buffer can hold a round of that size (grows, never shrinks); pool and
//                                                          table `keep` hold the running round and follow when they are next carried into
//   Backend::stage_bytes(set) / stage_offs(set)            host staging of a round, laid out like the pool and the offset table
//   Backend::upload(set, layout)                           fresh bytes and offsets of `layout` -> pool `set`, table `set`
//   Backend::cut(set, layout, watermark, max_row) -> MergeCutResult      keys and checks of the fresh cells, the cut per source
//   Backend::merge_and_carry(set, layout, cut, next)       the emitted prefixes merged into output `set`, the rest carried to pool set ^ 1
//   Backend::collect(set, nbytes) -> const uint8_t*        the merged bytes of that round, when they have arrived
// A round's pool is pool (round & 1).  A source's region of a pool begins at rbase (16-byte aligned) and holds its kept cells, then
// its fresh cells, without a gap; its rows of the tables begin at `first` in the same order.  Both are laid out before the refill
// from the length of the planned read, so the carry of round r and the read of round r + 1 do not wait for each other.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../core/gdb_merge.hpp"
#include "merge_common.hpp"
#include "vcf_importer.h"

namespace genomicsdb_amd {

constexpr uint64_t kMergeNone = ~(uint64_t)0;

inline double merge_files_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint64_t merge_align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

// one source of a windowed merge
struct MergeFileSource {
  int fd = -1;
  const uint8_t* mem = nullptr;
  uint64_t nbytes = 0;
  std::string name;
  MergeFileSource() = default;
  MergeFileSource(const MergeFileSource&) = delete;
  MergeFileSource& operator=(const MergeFileSource&) = delete;
  ~MergeFileSource() { if (fd >= 0) ::close(fd); }
  void open(const CellSource& src, size_t idx) {
    name = "merge: stream " + std::to_string(idx);
    if (src.path.empty()) {
      if (!src.data && src.nbytes) throw VCF2BinaryException(name + ": null data");
      mem = (const uint8_t*)src.data; nbytes = src.nbytes;
      return;
    }
    fd = ::open(src.path.c_str(), O_RDONLY);
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0) throw VCF2BinaryException(name + ": cannot read " + src.path + ": " + strerror(errno));
    nbytes = (uint64_t)st.st_size;
  }
  void read_at(uint64_t pos, uint8_t* dst, uint64_t n) const {
    if (fd < 0) { if (n) memcpy(dst, mem + pos, n); return; }
    while (n) {
      const ssize_t got = ::pread(fd, dst, n, (off_t)pos);
      if (got < 0 && errno == EINTR) continue;
      if (got <= 0) throw VCF2BinaryException(name + ": short read at byte offset " + std::to_string(pos));
      dst += got; pos += (uint64_t)got; n -= (uint64_t)got;
    }
  }
};

// where the sources lie in a round's pool and tables (indexed by source)
struct MergeRoundLayout {
  std::vector<uint64_t> rbase, first, kept_cells, kept_bytes, read_len, fresh_cells, fresh_bytes;
  explicit MergeRoundLayout(size_t k = 0) : rbase(k, 0), first(k, 0), kept_cells(k, 0), kept_bytes(k, 0), read_len(k, 0), fresh_cells(k, 0), fresh_bytes(k, 0) {}
  uint64_t cells(size_t s) const { return kept_cells[s] + fresh_cells[s]; }
  uint64_t bytes(size_t s) const { return kept_bytes[s] + fresh_bytes[s]; }
};

struct MergeWatermark { bool all = false, nothing = false; gdbmerge::MergeKey key{0, 0}; };      // all: every source is exhausted; nothing: a source has loaded no cell yet

// what the backend found in a round; indices of cells count from the first FRESH cell of their source
struct MergeCutResult {
  bool bad_cell = false;
  int64_t negative_source = -1; uint64_t negative_cell = 0;
  std::vector<uint64_t> unsorted;            // per source: the first fresh cell that comes before its predecessor, or kMergeNone
  uint64_t shared_row = kMergeNone;
  std::vector<uint64_t> emit_cells, emit_bytes;
  explicit MergeCutResult(size_t k = 0) : unsorted(k, kMergeNone), emit_cells(k, 0), emit_bytes(k, 0) {}
};

struct MergeFilesPlanner {
  std::vector<MergeFileSource> src;
  std::vector<uint64_t> share, pos, cells_loaded;
  std::vector<uint8_t> has_last;
  std::vector<gdbmerge::MergeKey> last_key;
  uint64_t max_row = 0;          // the largest row among the cells loaded: sizes the row bitmaps
  int64_t grown = 0;

  MergeFilesPlanner(const std::vector<CellSource>& sources, uint64_t window_bytes) : src(sources.size()) {
    const size_t k = sources.size();
    if (k == 0) throw VCF2BinaryException("merge: at least one stream is needed");
    if (k > 4096) throw VCF2BinaryException("merge: " + std::to_string(k) + " streams, at most 4096 are merged at once");
    for (size_t s = 0; s < k; ++s) src[s].open(sources[s], s);
    // every source the same share of the window, but no more than it is long
    const uint64_t one = window_bytes / k;
    share.assign(k, one ? one : 1);
    for (size_t s = 0; s < k; ++s) if (src[s].nbytes < share[s]) share[s] = src[s].nbytes ? src[s].nbytes : 1;
    pos.assign(k, 0); cells_loaded.assign(k, 0); has_last.assign(k, 0); last_key.assign(k, gdbmerge::MergeKey{0, 0});
  }
  size_t k() const { return src.size(); }
  bool exhausted(size_t s) const { return pos[s] == src[s].nbytes; }
  uint64_t window() const { uint64_t w = 0; for (uint64_t v : share) w += v; return w; }
  // what every buffer must hold while the shares are what they are (a source never holds more than its share)
  uint64_t pool_bytes() const { uint64_t b = 0; for (uint64_t v : share) b += merge_align16(v) + 16; return b; }
  uint64_t table_cells() const { return pool_bytes() / gdbmerge::kMergeHeaderBytes + k(); }

  // the layout of the round after one that kept (kept_cells, kept_bytes) of every source
  MergeRoundLayout layout(const std::vector<uint64_t>& kept_cells, const std::vector<uint64_t>& kept_bytes) const {
    MergeRoundLayout L(k());
    uint64_t at = 0, row = 0;
    for (size_t s = 0; s < k(); ++s) {
      L.rbase[s] = at; L.first[s] = row;
      L.kept_cells[s] = kept_cells[s]; L.kept_bytes[s] = kept_bytes[s];
      const uint64_t room = share[s] > kept_bytes[s] ? share[s] - kept_bytes[s] : 0, left = src[s].nbytes - pos[s];
      L.read_len[s] = room < left ? room : left;
      at = merge_align16(at + kept_bytes[s] + L.read_len[s]);
      row += kept_cells[s] + L.read_len[s] / gdbmerge::kMergeHeaderBytes;
    }
    return L;
  }

  // Refill: every source reads read_len bytes behind its kept bytes and the host walks their size chain, as merge_walk_cells does; a
  // cell cut by the end of the read is read again next round.  Notes the key of the last whole cell and checks the order across the
  // chunk boundary.  bytes / offs: the round's staging (offsets are pool offsets)
  void refill(MergeRoundLayout& L, uint8_t* bytes, uint64_t* offs) {
    for (size_t s = 0; s < k(); ++s) {
      L.fresh_cells[s] = L.fresh_bytes[s] = 0;
      const uint64_t len = L.read_len[s];
      if (!len) continue;
      const uint64_t base = L.rbase[s] + L.kept_bytes[s], total = src[s].nbytes;
      uint8_t* p = bytes + base;
      src[s].read_at(pos[s], p, len);
      uint64_t at = 0, n = 0;
      uint64_t* o = offs + L.first[s] + L.kept_cells[s];
      const std::string& who = src[s].name;
      gdbmerge::MergeKey key{0, 0}, first_key{0, 0}, whole_key{0, 0};
      while (at < len) {
        const uint64_t g = pos[s] + at;        // the byte offset counted from the start of the source
        if (len - at < gdbmerge::kMergeHeaderBytes) {
          if (g + (len - at) < total) break;      // the read cut the header
          throw VCF2BinaryException(who + ": the size chain runs past the end of the stream: a cell header at byte offset " + std::to_string(g) + " of " +
                                    std::to_string(total) + " bytes");
        }
        uint64_t size = 0;
        gdbmerge::merge_load_header(p + at, &key, &size);
        if (size < gdbmerge::kMergeHeaderBytes)
          throw VCF2BinaryException(who + ": cell_size " + std::to_string(size) + " at byte offset " + std::to_string(g) + " is smaller than a cell header");
        if (size > total - g)
          throw VCF2BinaryException(who + ": the size chain runs past the end of the stream: the cell at byte offset " + std::to_string(g) + " has cell_size " +
                                    std::to_string(size) + ", the stream " + std::to_string(total) + " bytes");
        if (size > len - at) break;               // the read cut the payload
        if (n == 0) first_key = key;
        if (key.row >= 0 && (uint64_t)key.row > max_row) max_row = (uint64_t)key.row;
        whole_key = key;
        o[n++] = base + at;
        at += size;
      }
      if (n) {
        if (has_last[s] && !gdbmerge::merge_boundary_in_order(last_key[s], first_key)) throw VCF2BinaryException(merge_unsorted_message(s, cells_loaded[s]));
        last_key[s] = whole_key; has_last[s] = 1;
      }
      L.fresh_cells[s] = n; L.fresh_bytes[s] = at;
      pos[s] += at; cells_loaded[s] += n;
    }
  }

  // the smallest last-loaded key over the sources that are not exhausted
  MergeWatermark watermark() const {
    MergeWatermark w;
    w.all = true;
    for (size_t s = 0; s < k(); ++s) {
      if (exhausted(s)) continue;
      if (!has_last[s]) w.nothing = true;
      else if (w.all || gdbmerge::merge_key_less(last_key[s], w.key)) w.key = last_key[s];
      w.all = false;
    }
    return w;
  }

  // the refusals of a round, in the in-core merge's words and order
  void refuse(const MergeRoundLayout& L, const MergeCutResult& c) const {
    if (c.bad_cell) throw VCF2BinaryException("merge: a cell header on the device does not match the size chain the host walked");
    if (c.negative_source >= 0) {
      const size_t s = (size_t)c.negative_source;
      throw VCF2BinaryException("merge: stream " + std::to_string(s) + ": cell " + std::to_string(cells_loaded[s] - L.fresh_cells[s] + c.negative_cell) + " has a negative row");
    }
    for (size_t s = 0; s < k(); ++s)
      if (c.unsorted[s] != kMergeNone) throw VCF2BinaryException(merge_unsorted_message(s, cells_loaded[s] - L.fresh_cells[s] + c.unsorted[s]));
    if (c.shared_row != kMergeNone) throw VCF2BinaryException(merge_shared_row_message(c.shared_row));
  }

  // Growth: the round emitted nothing although a source is not exhausted - one cell, or a run of one key, is larger than a share.
  // The sources that hold the watermark (or have loaded no cell yet) get twice their share
  void grow(const MergeWatermark& w) {
    for (size_t s = 0; s < k(); ++s) {
      if (exhausted(s)) continue;
      if (!has_last[s] || (!w.nothing && !gdbmerge::merge_key_less(w.key, last_key[s]))) {
        if (share[s] > (kMergeNone >> 2)) throw VCF2BinaryException(src[s].name + ": the window cannot grow any further");
        share[s] *= 2;
      }
    }
    ++grown;
  }
};

// the output of a windowed merge: <path>.merge.tmp, renamed to <path> by commit(); gone after anything else
struct MergeFilesOutput {
  std::string path, tmp;
  int fd = -1;
  explicit MergeFilesOutput(const std::string& p) : path(p), tmp(p + ".merge.tmp") {
    fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw VCF2BinaryException("merge: cannot write " + tmp + ": " + strerror(errno));
  }
  MergeFilesOutput(const MergeFilesOutput&) = delete;
  MergeFilesOutput& operator=(const MergeFilesOutput&) = delete;
  ~MergeFilesOutput() { if (fd >= 0) { ::close(fd); ::remove(tmp.c_str()); } }
  void write(const uint8_t* p, uint64_t n) {
    while (n) {
      const ssize_t put = ::write(fd, p, n);
      if (put < 0 && errno == EINTR) continue;
      if (put <= 0) throw VCF2BinaryException("merge: short write to " + tmp);
      p += put; n -= (uint64_t)put;
    }
  }
  void commit() {
    const int rc = ::close(fd);
    fd = -1;
    if (rc != 0 || ::rename(tmp.c_str(), path.c_str()) != 0) { ::remove(tmp.c_str()); throw VCF2BinaryException("merge: cannot rename " + tmp + " to " + path); }
  }
};

// The rounds.  While the backend works on round r, the host writes the output of round r - 1 and reads round r + 1.
template <class Backend>
uint64_t merge_files_run(MergeFilesPlanner& plan, const std::string& output_path, Backend& be, MergeFilesStats& st) {
  const size_t k = plan.k();
  MergeFilesOutput out(output_path);
  st.num_streams = (int64_t)k;
  st.tile = gdbmerge::kMergeTile;
  const std::vector<uint64_t> zero(k, 0);
  MergeRoundLayout L = plan.layout(zero, zero);
  be.reserve(plan.pool_bytes(), plan.table_cells(), k, -1);
  double t0 = merge_files_now();
  plan.refill(L, be.stage_bytes(0), be.stage_offs(0));
  st.s_read += merge_files_now() - t0;
  be.upload(0, L);
  int pending_set = -1;
  uint64_t pending_bytes = 0;
  auto flush = [&]() {
    if (pending_set < 0) return;
    double t = merge_files_now();
    const uint8_t* p = be.collect(pending_set, pending_bytes);
    const double t1 = merge_files_now();
    st.s_wait_device += t1 - t;
    out.write(p, pending_bytes);
    st.s_write += merge_files_now() - t1;
    pending_set = -1;
  };
  for (uint64_t round = 0;; ++round) {
    const int set = (int)(round & 1);
    const MergeWatermark w = plan.watermark();
    t0 = merge_files_now();
    const MergeCutResult cut = be.cut(set, L, w, plan.max_row);
    st.s_wait_device += merge_files_now() - t0;
    plan.refuse(L, cut);
    ++st.rounds;
    std::vector<uint64_t> kept_cells(k), kept_bytes(k);
    uint64_t emit_cells = 0, emit_bytes = 0, kept = 0;
    for (size_t s = 0; s < k; ++s) {
      if (cut.emit_cells[s] > L.cells(s) || cut.emit_bytes[s] > L.bytes(s)) throw VCF2BinaryException("merge: the cut of stream " + std::to_string(s) + " lies outside its cells");
      kept_cells[s] = L.cells(s) - cut.emit_cells[s]; kept_bytes[s] = L.bytes(s) - cut.emit_bytes[s];
      emit_cells += cut.emit_cells[s]; emit_bytes += cut.emit_bytes[s]; kept += kept_cells[s];
      st.cells_in += (int64_t)L.fresh_cells[s];
    }
    const bool done = w.all;
    if (done && kept) throw VCF2BinaryException("merge: cells were kept after the last round");
    if (!done && emit_cells == 0) {
      plan.grow(w);
      flush();                 // (the staging that holds the previous round's output is about to be replaced)
      be.reserve(plan.pool_bytes(), plan.table_cells(), k, set);
    }
    st.carried_cells += (int64_t)kept;
    MergeRoundLayout next = plan.layout(kept_cells, kept_bytes);
    be.merge_and_carry(set, L, cut, next);
    flush();
    if (emit_cells) { pending_set = set; pending_bytes = emit_bytes; }
    st.cells_out += (int64_t)emit_cells; st.bytes_out += emit_bytes;
    if (done) break;
    t0 = merge_files_now();
    plan.refill(next, be.stage_bytes(set ^ 1), be.stage_offs(set ^ 1));
    st.s_read += merge_files_now() - t0;
    be.upload(set ^ 1, next);
    L = next;
  }
  flush();
  t0 = merge_files_now();
  out.commit();
  st.s_write += merge_files_now() - t0;
  st.grown = plan.grown;
  st.window_bytes = plan.window();
  return (uint64_t)st.cells_out;
}

}  // namespace genomicsdb_amd
