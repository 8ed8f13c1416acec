// hostsim_index - the bodies of the device tabix builder (csrc/core/gdb_index.hpp) on the CPU (test infrastructure only): a library
// for pytest and, with -DHOSTSIM_INDEX_MAIN, a stand-alone program built with the address and undefined-behaviour sanitizers.
//
//   hostsim_index <file.vcf.gz> <out.tbi> <batch bytes>
//       The file's BGZF members are inflated by zlib, its lines are taken in batches of whole lines of at most <batch bytes> (one
//       line at least), and every batch goes serially through the stages of kernels/gdb_index.hip: select the record lines, one
//       idx_record per record, run heads by idx_same_chrom, a stable sort by contig id, chunk heads, a stable sort of the chunks by
//       (contig id, bin), and the window minima in "wavefronts" of 64 neighbours (idx_window_mine).  The batches are joined by
//       TbiBatchMerger and written by write_tbi_index (host/vcf_index.h), the serialiser the host builder uses.
//       Prints "stats members <m> batches <b> lines <l> records <r> contigs <c> bins <x> chunks <y> windows <w> atomics <a>".
// A named error prints "error: <what>" and ends with status 0: only a crash or a sanitizer report ends otherwise.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_index.hpp"
#include "../../genomicsdb_amd/csrc/host/vcf_index.h"
#include "../../genomicsdb_amd/csrc/kernels/gdb_inflate.h"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbidx;

namespace {

enum { kMembers, kBatches, kLines, kRecords, kContigs, kBins, kChunks, kWindows, kAtomics, kNumStats };

std::string inflate_all(const std::string& raw, const std::vector<BgzfMember>& mem, const std::string& path) {
  std::string text;
  for (const BgzfMember& m : mem) {
    const size_t old = text.size();
    text.resize(old + m.isize);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("zlib inflateInit2 failed");
    uint8_t spare = 0;
    zs.next_in = (Bytef*)(raw.data() + m.offset + m.data_off); zs.avail_in = m.data_len;
    zs.next_out = m.isize ? (Bytef*)&text[old] : &spare; zs.avail_out = m.isize;
    const int rc = inflate(&zs, Z_FINISH);
    const uint64_t got = zs.total_out;
    inflateEnd(&zs);
    const std::string where = "corrupt BGZF member at byte offset " + std::to_string(m.offset) + " of " + path + ": ";
    if (rc != Z_STREAM_END) throw std::runtime_error(where + "invalid DEFLATE stream");
    if (got != m.isize) throw std::runtime_error(where + "the data is not ISIZE bytes long");
    if ((uint32_t)crc32(0L, (const Bytef*)(text.data() + old), m.isize) != m.crc) throw std::runtime_error(where + "CRC32 mismatch");
  }
  return text;
}

// one batch: text[b0, b1) of whole lines, the first one line number lines_before + 1
void index_batch(const std::string& path, const std::string& text, size_t b0, size_t b1, int64_t lines_before, const IdxMembers& M, TbiBatchMerger& merger, uint64_t* st) {
  const char* t = text.data() + b0;
  const uint32_t n = (uint32_t)(b1 - b0);
  // ---- the index: lines, and every tab of a line
  struct Line { uint32_t begin, end, first_tab, ntabs; bool newline; };
  std::vector<Line> lines;
  std::vector<uint32_t> tabs;
  for (uint32_t at = 0; at < n;) {
    Line l;
    l.begin = at; l.first_tab = (uint32_t)tabs.size();
    while (at < n && t[at] != '\n') { if (t[at] == '\t') tabs.push_back(at); ++at; }
    l.end = at; l.ntabs = (uint32_t)tabs.size() - l.first_tab; l.newline = at < n;
    lines.push_back(l);
    at += 1;
  }
  tabs.push_back(0);      // (so that tabs.data() + first_tab is a pointer into the vector for a last line without tabs)
  st[kLines] += lines.size();
  auto line_of = [&](uint32_t i) { gdbimp::ImpLine L; L.text = t; L.begin = lines[i].begin; L.end = lines[i].end; L.tabs = tabs.data() + lines[i].first_tab; L.ntabs = lines[i].ntabs; return L; };
  // ---- select and compact, one idx_record per record
  std::vector<uint32_t> rec_line;
  for (uint32_t i = 0; i < lines.size(); ++i) if (idx_is_record(line_of(i))) rec_line.push_back(i);
  const uint32_t nr = (uint32_t)rec_line.size();
  st[kRecords] += nr;
  if (!nr) return;
  std::vector<IdxRec> rec(nr);
  for (uint32_t r = 0; r < nr; ++r) {
    rec[r] = idx_record(M, line_of(rec_line[r]), (uint64_t)b0, lines[rec_line[r]].newline);
    if (rec[r].err) throw std::runtime_error(tbi_record_error(rec[r].err, path, lines_before + (int64_t)rec_line[r] + 1));
  }
  // ---- run heads -> names -> ids
  std::vector<uint32_t> tid(nr);
  for (uint32_t r = 0; r < nr; ++r) {
    const gdbimp::ImpLine L = line_of(rec_line[r]);
    if (r == 0 || !idx_same_chrom(L, line_of(rec_line[r - 1]))) tid[r] = merger.id_of(std::string(t + L.begin, L.tabs[0] - L.begin));
    else tid[r] = tid[r - 1];
  }
  // ---- stable sort by contig id, chunk heads, chunks sorted stably by (contig id, bin)
  std::vector<uint32_t> order(nr);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tid[a] < tid[b]; });
  std::vector<IdxChunk> chunks;
  for (uint32_t i = 0; i < nr; ++i) {
    const uint32_t r = order[i], p = i ? order[i - 1] : 0u;
    if (idx_chunk_head(i == 0, tid[r], rec[r].bin, tid[p], rec[p].bin)) {
      IdxChunk c;
      c.beg = rec[r].vbeg; c.end = rec[r].vend; c.tid = tid[r]; c.bin = rec[r].bin; c.count = 0;
      c.flags = (i == 0 || tid[p] != tid[r]) ? IDX_CHUNK_FIRST : 0u;
      chunks.push_back(c);
    }
    chunks.back().end = rec[r].vend;
    ++chunks.back().count;
    if (i + 1 == nr || tid[order[i + 1]] != tid[r]) chunks.back().flags |= IDX_CHUNK_LAST;
  }
  std::stable_sort(chunks.begin(), chunks.end(), [](const IdxChunk& a, const IdxChunk& b) { return a.tid != b.tid ? a.tid < b.tid : a.bin < b.bin; });
  merger.add_chunks(chunks.data(), chunks.size());
  // ---- window minima: per contig [0, largest window], lanes of 64 neighbours in the sorted order
  std::vector<std::vector<uint64_t>> win(merger.names.size());
  for (uint32_t r = 0; r < nr; ++r) if (win[tid[r]].size() <= rec[r].w1) win[tid[r]].resize((size_t)rec[r].w1 + 1, ~0ull);
  for (uint32_t i = 0; i < nr; ++i) {
    const uint32_t r = order[i], p = i ? order[i - 1] : 0u;
    if (rec[r].vbeg == 0) continue;
    for (uint32_t w = rec[r].w0; w <= rec[r].w1; ++w) {
      if (!idx_window_mine((i & 63u) != 0u, tid[r], w, tid[p], rec[p].w0, rec[p].w1, rec[p].vbeg)) continue;
      ++st[kAtomics];
      win[tid[r]].at(w) = std::min(win[tid[r]].at(w), rec[r].vbeg);
    }
  }
  for (uint32_t c = 0; c < win.size(); ++c) if (!win[c].empty()) merger.add_windows(c, win[c].data(), win[c].size());
}

void build(const std::string& path, const std::string& tbi_path, uint64_t batch_bytes, uint64_t* st) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error("index: cannot open " + path);
  const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<BgzfMember> mem;
  uint64_t total = 0, break_at = 0;
  if (!bgzf_walk((const uint8_t*)raw.data(), raw.size(), mem, &total, &break_at))
    throw std::runtime_error("index: " + path + " is not a BGZF file from its first byte to its last: the chain breaks at byte offset " + std::to_string(break_at));
  const std::string text = inflate_all(raw, mem, path);
  if (text.size() >= ((size_t)1 << 31)) throw std::runtime_error("2 GiB or more in " + path);
  std::vector<uint64_t> ubase, coff;
  for (const BgzfMember& m : mem) if (m.isize) { ubase.push_back(m.out_off); coff.push_back(m.offset); }
  const IdxMembers M{ubase.data(), coff.data(), (uint32_t)ubase.size(), total, (uint64_t)raw.size() << 16};
  for (int i = 0; i < kNumStats; ++i) st[i] = 0;
  st[kMembers] = mem.size();
  TbiBatchMerger merger;
  if (batch_bytes == 0) batch_bytes = ~0ull;
  size_t pos = 0;
  int64_t lines_before = 0;
  while (pos < text.size()) {
    size_t stop = pos;
    for (;;) {      // whole lines while they fit, one at least
      const size_t nl = text.find('\n', stop);
      const size_t e = nl == std::string::npos ? text.size() : nl + 1;
      if (stop > pos && e - pos > batch_bytes) break;
      stop = e;
      if (stop >= text.size()) break;
    }
    const uint64_t lines_then = st[kLines];
    index_batch(path, text, pos, stop, lines_before, M, merger, st);
    lines_before += (int64_t)(st[kLines] - lines_then);
    ++st[kBatches];
    pos = stop;
  }
  st[kContigs] = merger.names.size(); st[kBins] = merger.num_bins(); st[kChunks] = merger.num_chunks();
  merger.write(tbi_path);
  st[kWindows] = merger.num_windows();
}

}  // namespace

extern "C" int hostsim_index_build(const char* path, const char* tbi_path, uint64_t batch_bytes, uint64_t* stats /* 9 */, char* err, uint64_t err_cap) {
  uint64_t st[kNumStats];
  try {
    build(path, tbi_path, batch_bytes, st);
    if (stats) memcpy(stats, st, sizeof(st));
    return 0;
  } catch (const std::exception& e) {
    if (err && err_cap) { strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = '\0'; }
    return -1;
  }
}

#ifdef HOSTSIM_INDEX_MAIN
int main(int argc, char** argv) {
  if (argc < 4) { std::cerr << "usage: hostsim_index <file.vcf.gz> <out.tbi> <batch bytes>\n"; return 2; }
  uint64_t st[kNumStats];
  try {
    build(argv[1], argv[2], strtoull(argv[3], nullptr, 10), st);
  } catch (const std::exception& e) {
    std::cout << "error: " << e.what() << "\n";
    return 0;
  }
  std::cout << "stats members " << st[kMembers] << " batches " << st[kBatches] << " lines " << st[kLines] << " records " << st[kRecords] << " contigs " << st[kContigs]
            << " bins " << st[kBins] << " chunks " << st[kChunks] << " windows " << st[kWindows] << " atomics " << st[kAtomics] << "\n";
  return 0;
}
#endif
