// hostsim_output_index - the bodies of the device builder of the output's index (csrc/core/gdb_output_index.hpp, with the chunk and
// window rules of csrc/core/gdb_index.hpp) on the CPU (test infrastructure only): a library for pytest and, with
// -DHOSTSIM_OUTPUT_INDEX_MAIN, a stand-alone program built with the address and undefined-behaviour sanitizers.
//
//   hostsim_output_index <case file> <out.tbi | out.csi>
//       The case file holds the pages of one output stream as the device sees them (little endian):
//         "OIDX1\0\0\0"; u32 bcf, u32 B (input bytes per block); u64 compressed bytes of the header; u64 lines of the header;
//         u32 contigs, u32 bytes of their names, the names of the header's ##contig lines, each followed by '\n';
//         u32 pages; per page: u64 bytes, u32 records, u32 blocks, the page's uncompressed bytes, u64 rec_off[records + 1]
//         (page-relative), u32 compressed size of every block.
//       Every page goes serially through the stages of kernels/gdb_output_index.hip: one oidx_text_record / oidx_bcf_record per record,
//       oidx_voff over the exclusive scan of the block sizes, a stable sort by contig, chunk heads and tails, the window minima in
//       "wavefronts" of 64 neighbours (idx_window_mine).  The pages are joined by OutputIndexMerger and written by write_tbi_index /
//       write_csi_index (host/vcf_index.h), the serialisers the host builders use.
//       Prints "stats pages <p> records <r> contigs <c> bins <x> chunks <y> windows <w> atomics <a>".
// A named error prints "error: <what>" and ends with status 0: only a crash or a sanitizer report ends otherwise.
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

#include "../../genomicsdb_amd/csrc/core/gdb_output_index.hpp"
#include "../../genomicsdb_amd/csrc/host/vcf_index.h"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbidx;
using namespace genomicsdb_amd::gdboidx;

namespace {

enum { kPages, kRecords, kContigs, kBins, kChunks, kWindows, kAtomics, kNumStats };

struct Reader {
  const std::string& s; size_t at = 0;
  explicit Reader(const std::string& s_) : s(s_) {}
  const char* take(size_t n) { if (n > s.size() - at) throw std::runtime_error("case file: truncated"); const char* p = s.data() + at; at += n; return p; }
  template <class T> T get() { T v; memcpy(&v, take(sizeof(T)), sizeof(T)); return v; }
};

struct Page { std::string bytes; std::vector<uint64_t> rec_off; std::vector<uint32_t> csize; };

// one page: what page_records, page_blocks and merge_page of the device builder do
void index_page(bool bcf, const Page& P, uint32_t B, const ContigTable& C, uint32_t n_kid, int64_t records_before, OutputIndexMerger& merger, uint64_t* st) {
  const uint32_t n_rec = (uint32_t)(P.rec_off.size() - 1);
  const uint64_t page_bytes = P.bytes.size();
  uint64_t compressed = 0;
  std::vector<uint64_t> boff(P.csize.size() + 1, 0);
  for (size_t k = 0; k < P.csize.size(); ++k) { boff[k + 1] = boff[k] + P.csize[k]; compressed += P.csize[k]; }
  const uint32_t nblocks = (uint32_t)P.csize.size();
  if (nblocks != (page_bytes + B - 1) / B) throw std::runtime_error("case file: the blocks do not cover the page");
  const std::vector<uint32_t> none(n_kid, 0u);
  if (n_rec == 0) { merger.add_page(nullptr, 0, 0, nullptr, none.data(), nullptr, compressed); return; }
  // ---- records (before the deflate), then their virtual offsets (behind it)
  std::vector<uint64_t> a(n_rec), b((size_t)n_rec + 1);
  std::vector<uint32_t> bin(n_rec), w0(n_rec), w1(n_rec), kid(n_rec);
  const uint32_t hint = merger.last_contig();
  for (uint32_t r = 0; r < n_rec; ++r) {
    const uint64_t ub = P.rec_off[r], ue = P.rec_off[r + 1];
    OutRec o;
    o.bin = 0; o.w0 = 0; o.w1 = 0; o.kid = kNoContig; o.err = OIDX_ERR_SHAPE;
    if (ub <= ue && ue <= page_bytes && ue - ub < ((uint64_t)1 << 32))
      o = bcf ? oidx_bcf_record((const uint8_t*)P.bytes.data() + ub, ue - ub, n_kid) : oidx_text_record(P.bytes.data() + ub, (uint32_t)(ue - ub), C, hint);
    if (o.err) throw std::runtime_error("index: record " + std::to_string(records_before + r + 1) + " of the output stream is refused (bits " + std::to_string(o.err) + ")");
    a[r] = ub; b[r] = ue; bin[r] = o.bin; w0[r] = o.w0; w1[r] = o.w1; kid[r] = o.kid < n_kid ? o.kid : n_kid;
  }
  for (uint32_t r = 0; r < n_rec; ++r) {
    a[r] = oidx_voff(boff.data(), nblocks, B, page_bytes, std::min(a[r], page_bytes));
    b[r] = oidx_voff(boff.data(), nblocks, B, page_bytes, std::min(b[r], page_bytes));
  }
  b[n_rec] = oidx_voff(boff.data(), nblocks, B, page_bytes, page_bytes);
  // ---- stable sort by contig, chunk heads, the chunk written by its last record
  std::vector<uint32_t> ord(n_rec);
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return kid[x] < kid[y]; });
  std::vector<uint32_t> kid_s(n_rec), chead((size_t)n_rec + 1, 0u), coff((size_t)n_rec + 1, 0u);
  for (uint32_t i = 0; i < n_rec; ++i) kid_s[i] = kid[ord[i]];
  for (uint32_t i = 0; i < n_rec; ++i) {
    const uint32_t p = i ? i - 1u : 0u;
    chead[i] = (kid_s[i] < n_kid && idx_chunk_head(i == 0u, kid_s[i], bin[ord[i]], kid_s[p], bin[ord[p]])) ? 1u : 0u;
  }
  for (uint32_t i = 0; i < n_rec; ++i) coff[i + 1] = coff[i] + chead[i];
  const uint32_t n_chunks = coff[n_rec];
  std::vector<uint32_t> cfirst(n_chunks);
  for (uint32_t i = 0; i < n_rec; ++i) if (chead[i]) cfirst.at(coff[i]) = i;
  std::vector<IdxChunk> chunks(n_chunks);
  for (uint32_t i = 0; i < n_rec; ++i) {
    if (kid_s[i] >= n_kid) continue;
    const bool last = i + 1u == n_rec;
    if (!oidx_chunk_tail(last, last ? 0u : kid_s[i + 1u], n_kid, !last && chead[i + 1u] != 0u)) continue;
    const uint32_t c = coff[i] + chead[i] - 1u, i0 = cfirst.at(c);
    IdxChunk k;
    k.tid = kid_s[i0]; k.bin = bin[ord[i0]]; k.beg = a[ord[i0]]; k.end = b[ord[i]]; k.count = i - i0 + 1u;
    k.flags = ((i0 == 0u || kid_s[i0 - 1u] != k.tid) ? IDX_CHUNK_FIRST : 0u) | ((last || kid_s[i + 1u] != k.tid) ? IDX_CHUNK_LAST : 0u);
    chunks.at(c) = k;
  }
  // ---- window minima: per contig [0, largest window], lanes of 64 neighbours in the sorted order
  std::vector<uint32_t> extent(n_kid, 0u), win_off(n_kid, 0u);
  for (uint32_t i = 0; i < n_rec; ++i) if (kid_s[i] < n_kid) extent[kid_s[i]] = std::max(extent[kid_s[i]], w1[ord[i]] + 1u);
  uint64_t n_win = 0;
  for (uint32_t c = 0; c < n_kid; ++c) { win_off[c] = (uint32_t)n_win; n_win += extent[c]; }
  std::vector<uint64_t> win((size_t)n_win, ~0ull);
  for (uint32_t i = 0; i < n_rec; ++i) {
    if (kid_s[i] >= n_kid) continue;
    const uint32_t r = ord[i], p = i ? ord[i - 1] : 0u, pk = i ? kid_s[i - 1] : 0u;
    for (uint32_t w = w0[r]; w <= w1[r]; ++w) {
      if (!idx_window_mine((i & 63u) != 0u, kid_s[i], w, pk, w0[p], w1[p], 1u)) continue;
      ++st[kAtomics];
      uint64_t& m = win.at((size_t)win_off[kid_s[i]] + w);
      m = std::min(m, a[r]);
    }
  }
  merger.add_page(chunks.data(), chunks.size(), b[n_rec], win_off.data(), extent.data(), win.data(), compressed);
  ++st[kPages];
  st[kRecords] += n_rec;
}

void build(const std::string& case_path, const std::string& out_path, uint64_t* st) {
  std::ifstream in(case_path, std::ios::binary);
  if (!in) throw std::runtime_error("cannot open " + case_path);
  const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  Reader R(raw);
  if (memcmp(R.take(8), "OIDX1\0\0\0", 8) != 0) throw std::runtime_error("case file: bad magic");
  const bool bcf = R.get<uint32_t>() != 0;
  const uint32_t B = R.get<uint32_t>();
  if (B == 0 || B > 65536u) throw std::runtime_error("case file: bad block size");
  const uint64_t header_bytes = R.get<uint64_t>();
  (void)R.get<uint64_t>();      // (lines of the header: only the device builder's messages name lines)
  const uint32_t n_kid = R.get<uint32_t>(), names_len = R.get<uint32_t>();
  const std::string names(R.take(names_len), names_len);
  std::vector<std::string> contigs;
  std::vector<uint32_t> name_off(1, 0u);
  std::string name_bytes;
  for (size_t p = 0; p < names.size();) {
    size_t e = names.find('\n', p);
    if (e == std::string::npos) e = names.size();
    contigs.push_back(names.substr(p, e - p));
    name_bytes += contigs.back();
    name_off.push_back((uint32_t)name_bytes.size());
    p = e + 1;
  }
  if (contigs.size() != n_kid) throw std::runtime_error("case file: the names do not match their count");
  name_bytes.push_back('\0');
  const ContigTable C{name_bytes.data(), name_off.data(), n_kid};
  for (int i = 0; i < kNumStats; ++i) st[i] = 0;
  OutputIndexMerger merger(bcf, contigs, header_bytes);
  const uint32_t n_pages = R.get<uint32_t>();
  int64_t records_before = 0;
  for (uint32_t p = 0; p < n_pages; ++p) {
    Page P;
    const uint64_t nbytes = R.get<uint64_t>();
    const uint32_t n_rec = R.get<uint32_t>(), nblocks = R.get<uint32_t>();
    P.bytes.assign(R.take(nbytes), nbytes);
    P.rec_off.resize((size_t)n_rec + 1);
    memcpy(P.rec_off.data(), R.take(P.rec_off.size() * 8), P.rec_off.size() * 8);
    P.csize.resize(nblocks);
    if (nblocks) memcpy(P.csize.data(), R.take((size_t)nblocks * 4), (size_t)nblocks * 4);
    index_page(bcf, P, B, C, n_kid, records_before, merger, st);
    records_before += n_rec;
  }
  st[kContigs] = bcf ? n_kid : merger.merger.names.size();
  merger.write(out_path);
  st[kBins] = merger.merger.num_bins(); st[kChunks] = merger.merger.num_chunks(); st[kWindows] = merger.merger.num_windows();
}

}  // namespace

extern "C" int hostsim_output_index_build(const char* case_path, const char* out_path, uint64_t* stats /* 7 */, char* err, uint64_t err_cap) {
  uint64_t st[kNumStats];
  try {
    build(case_path, out_path, st);
    if (stats) memcpy(stats, st, sizeof(st));
    return 0;
  } catch (const std::exception& e) {
    if (err && err_cap) { strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = '\0'; }
    return -1;
  }
}

#ifdef HOSTSIM_OUTPUT_INDEX_MAIN
int main(int argc, char** argv) {
  if (argc < 3) { std::cerr << "usage: hostsim_output_index <case file> <out.tbi | out.csi>\n"; return 2; }
  uint64_t st[kNumStats];
  try {
    build(argv[1], argv[2], st);
  } catch (const std::exception& e) {
    std::cout << "error: " << e.what() << "\n";
    return 0;
  }
  std::cout << "stats pages " << st[kPages] << " records " << st[kRecords] << " contigs " << st[kContigs] << " bins " << st[kBins] << " chunks " << st[kChunks] << " windows "
            << st[kWindows] << " atomics " << st[kAtomics] << "\n";
  return 0;
}
#endif
