// gdb_assembly_choice.hpp - which sizing and page kernels an interval's sample columns take: the GDBAMD_* knobs that select them, read
// in one place, and the whole decision as host arithmetic (no HIP types: tests/hostsim_dispatch compiles it with g++ and
// tests/test_assembly_choice_cpu.py holds it against tests/variant_shapes.py).  gdb_pipeline.hip launches what these functions name.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace genomicsdb_amd {

constexpr int kAsmRows = 64;             // samples per (record, chunk): one wavefront
constexpr int kWaveLds = 8 * 1024;       // LDS image of one (record, chunk)
constexpr int kCooperativeEntry = 512;   // entry texts longer than this are copied pool -> page by the whole wavefront, not through the LDS image

// IntervalStats::page_kernel: the decimal digits S K W C II of the sizing kernel, the page kernel, its wavefronts per workgroup, its
// COOP_U (0: none) and its LDS image in KiB
enum { kSizeKernelPlain = 0, kSizeKernel3x8 = 1, kSizeKernel3x16 = 2, kSizeKernelPieces = 3, kSizeKernelEvents = 4 };
enum { kPageKernelWrite = 1, kPageKernelWrite2 = 2, kPageKernelWrite3 = 3, kPageKernelEvents = 4, kPageKernelBcf = 5 };
constexpr int page_kernel_code(int size_kernel, int page_kernel, int waves, int coop_u, int lds_bytes) {
  return size_kernel * 100000 + page_kernel * 10000 + waves * 1000 + coop_u * 100 + lds_bytes / 1024;
}

// The knobs that select sizing and page kernels.  prepare_interval reads them once into the interval's state and begin_page uses that
// snapshot: a knob flipped between prepare_interval and a later begin_page of the same interval takes effect with the next interval.
// (GDBAMD_RES_LAYOUT alone is read once per process: the pipeline overwrites res_chunk_major with what the process started with.)
struct AssemblyKnobs {
  // Records one wavefront takes in a row.  Measured on c2 (200 kb windows): the sizing pass, which starts every run with a
  // binary search per sample, is fastest at 64; the page pass (no per-run set-up beyond one 64-lane scalar fetch) at 32 -
  // more, shorter runs balance better across the 256 CUs than longer ones amortise.  GDBAMD_RUN / GDBAMD_RUN_W override.
  int run, run_w, run_w2, run_f;   // GDBAMD_RUN (default 128 with the piece-wise kernel: measured 0.3 ms faster than 64, 256 slower; else 64), _RUN_W, _RUN_W2, _RUN_F
  // HBM the resolved (record, sample) matrix of a whole interval may take (8 bytes x records x samples rounded up to 64);
  // wider intervals resolve page by page.  GDBAMD_RESOLVED_MB overrides (tests use 0 to force the per-page path).
  uint64_t resolved_budget_bytes;
  // GDBAMD_EVENTS=1 selects the change-list page assembly instead of the dense matrix; GDBAMD_EV_RUN: its records per (run, chunk) (<= 64)
  // (off by default: measured slower than the dense matrix, with scalar loads of the changes and with vector loads + v_readlane)
  bool events; int ev_run;
  int asm_path;                    // GDBAMD_ASM_PATH 0..3: see choose_sizing
  int size3_rounds;                // GDBAMD_SIZE3, sizing pass: 8 = k_assemble_size3 in rounds of 8 records (default), 16 = rounds of 16, 0 = k_assemble_size
  bool size3_check;                // GDBAMD_SIZE3_CHECK: the piece-wise sizing kernels are compared with k_assemble_size word for word
  // compact resolved matrix (ResMatrix): 1 (default) whenever the interval allows it, 0 never (A/B runs); the check mode of the sizing
  // kernels compares the wide layout word for word, so it keeps that one
  bool res_compact;
  bool res_chunk_major;            // GDBAMD_RES_LAYOUT=1 (measured: no difference; record-major stays)
  int write_waves;                 // GDBAMD_WRITE_WAVES: wavefronts (= neighbouring 64-sample chunks) per workgroup of the page assembly: 4 measured best on the store-only model
  // LDS image of one (record, 64-sample chunk) of the page kernel.  GDBAMD_WRITE_IMAGE_KB = 4 / 6 / 8 forces one; otherwise by the
  // interval's average chunk: 4 KiB while a chunk (c2: 2.8 KB) and its alignment slack fit - more resident wavefronts per CU, 0.4-0.6 ms
  // of a 12 ms launch, three A/B rounds inside one call (profiles/r5_ab_image.txt) - and 8 KiB for wider entries (c3's width: ~6 KB
  // per chunk would take two passes through a 4 KiB image)
  bool write_image_set; int write_image_kb;
  int order_block_log2;            // GDBAMD_ORDER_BLOCK_LOG2: records are grouped by type inside blocks of 2^this consecutive records
  bool coop_unroll, xcd_aware;     // GDBAMD_COOP_UNROLL (A/B: 0 keeps the word-by-word copy of long entries), GDBAMD_XCD_AWARE
  int page_priority;               // GDBAMD_PAGE_PRIORITY=0 / 1 overrides what the engine asked for (set_page_priority); -1: unset

  int image_kb(uint64_t avg_chunk_bytes) const { return write_image_set ? write_image_kb : avg_chunk_bytes && avg_chunk_bytes <= 3400 ? 4 : 8; }
  bool page_priority_on(bool engine_asks) const { return page_priority >= 0 ? page_priority == 1 : engine_asks; }
};

typedef const char* (*KnobLookup)(const char* name);   // getenv in the product; a harness feeds strings (unset: nullptr)

inline bool res_layout_chunk_major(KnobLookup get) { const char* e = get("GDBAMD_RES_LAYOUT"); return e && *e == '1'; }

inline AssemblyKnobs read_assembly_knobs(KnobLookup get) {
  const auto num = [get](const char* name, int unset, int lo, int hi) { const char* e = get(name); return e && *e ? std::max(lo, std::min(hi, atoi(e))) : unset; };
  const auto on = [get](const char* name) { const char* e = get(name); return e && *e && *e != '0'; };
  const auto not_off = [get](const char* name) { const char* e = get(name); return !(e && *e == '0'); };
  const int any = 0x7fffffff;
  AssemblyKnobs k{};
  const int size3 = num("GDBAMD_SIZE3", 8, -any, any);
  k.size3_rounds = size3 == 0 ? 0 : size3 >= 16 ? 16 : 8;
  k.run = num("GDBAMD_RUN", k.size3_rounds ? 128 : 64, 1, any);
  k.run_w = num("GDBAMD_RUN_W", 32, 1, any);
  k.run_w2 = num("GDBAMD_RUN_W2", 64, 1, any);
  k.run_f = num("GDBAMD_RUN_F", 128, 1, any);
  const char* mb = get("GDBAMD_RESOLVED_MB");
  k.resolved_budget_bytes = mb && *mb ? (uint64_t)atoll(mb) << 20 : (uint64_t)32 << 30;
  k.events = on("GDBAMD_EVENTS");
  k.ev_run = num("GDBAMD_EV_RUN", 32, 1, 64);
  k.asm_path = num("GDBAMD_ASM_PATH", 0, 0, 3);
  k.size3_check = on("GDBAMD_SIZE3_CHECK");
  k.res_compact = !k.size3_check && not_off("GDBAMD_RES_COMPACT");
  k.res_chunk_major = res_layout_chunk_major(get);
  k.write_waves = num("GDBAMD_WRITE_WAVES", 1, -any, any);
  const char* image = get("GDBAMD_WRITE_IMAGE_KB");
  k.write_image_set = image && *image;
  k.write_image_kb = k.write_image_set ? atoi(image) : 0;
  k.order_block_log2 = num("GDBAMD_ORDER_BLOCK_LOG2", 12, 0, 30);
  k.coop_unroll = not_off("GDBAMD_COOP_UNROLL");
  k.xcd_aware = not_off("GDBAMD_XCD_AWARE");
  const char* prio = get("GDBAMD_PAGE_PRIORITY");
  k.page_priority = prio && (*prio == '0' || *prio == '1') ? *prio - '0' : -1;
  return k;
}

// the sizing kernel of `run` records per wavefront where nothing else decides (path 0, and the per-page resolution of a matrix over the budget)
inline int size_kernel_for(const AssemblyKnobs& k, int run) {
  return k.size3_rounds == 0 || run > 64 * 1024 ? kSizeKernelPlain : k.size3_rounds >= 16 ? kSizeKernel3x16 : kSizeKernel3x8;
}

struct IntervalFacts { bool bcf_mode; int64_t P; int32_t N; bool untabled_records, any_over255; };   // records, samples, UR > 0, an entry text over 255 bytes

struct AssemblySizing {
  bool bcf_mode;              // the interval is written as BCF2 records, not text
  int asm_path;               // GDBAMD_ASM_PATH after its adjustments
  bool piece_path;            // matrix-free page assembly (paths 1 and 3)
  int size_kernel;            // kSizeKernel*: what sizes the interval
  int run, frun, evrun;       // records per wavefront of the sizing kernel, of k_fill2, of the change-list kernels
  bool use_events;            // k_assemble_size_ev leaves change lists, pages on order-block boundaries replay them
  bool resolved_whole;        // the (record, sample) matrix of the whole interval is resolved while sizing; else page by page
  bool res_compact;           // ResMatrix in its compact layout: the default kernels (text and BCF2), no entry longer than a byte can say
  bool chunk_major;           // GDBAMD_RES_LAYOUT=1 on a text interval whose matrix a sizing kernel writes (not k_fill2): the kernels are told its row count
  int resolved_entry_bytes;   // IntervalStats: 0 no matrix, 5 compact, 8 wide
  int64_t res_rows(int64_t rows) const { return chunk_major ? rows : 0; }
};

// How an interval's sample columns are sized and assembled (GDBAMD_ASM_PATH, read per interval; measured in DESIGN.md section 5):
//   0 (default)  the sizing pass of rounds 1-3 (k_assemble_size: every (record, sample) pair walked, sizes and matrix in one pass), pages by k_assemble_write
//   1            text only: sizes from pieces (k_size2), no matrix at all, the page pass walks the pieces itself (k_write2)
//   2            sizes from pieces (k_size2), the matrix from a piece walker per lane (k_fill2), pages by k_assemble_write / the BCF kernels
//   3            text only: sizes from pieces (k_size2), piece lists (k_plist), pages by k_write3 (no matrix, no walking in the page pass)
// GDBAMD_EVENTS forces path 0; BCF2 has no matrix-free kernels, so its odd paths become 2; records of untabled types have a slot per
// (record, sample), which the piece lists of path 3 do not carry: path 0 takes over.
inline AssemblySizing choose_sizing(const AssemblyKnobs& k, const IntervalFacts& f) {
  AssemblySizing s{};
  s.bcf_mode = f.bcf_mode;
  const uint64_t nchunks = (uint64_t)((f.N + kAsmRows - 1) / kAsmRows), entry = 8;   // (bytes of a wide matrix entry and of a change)
  s.asm_path = k.events ? 0 : (f.bcf_mode && (k.asm_path & 1)) ? 2 : k.asm_path;
  if (s.asm_path == 3 && f.untabled_records) s.asm_path = 0;
  s.piece_path = s.asm_path == 1 || s.asm_path == 3;
  s.run = k.run; s.frun = k.run_f; s.evrun = k.ev_run;
  const bool events_fit_blocks = k.events && ((1 << k.order_block_log2) % k.ev_run) == 0;   // a run of the change list must divide the order block
  s.resolved_whole = !s.piece_path && (f.bcf_mode || ((uint64_t)f.P * nchunks * kAsmRows * entry <= k.resolved_budget_bytes && !events_fit_blocks));
  s.res_compact = s.asm_path == 0 && !k.events && !f.any_over255 && k.res_compact && (!f.bcf_mode || s.resolved_whole);
  const uint64_t ev_blocks = (uint64_t)((f.P + s.evrun - 1) / s.evrun) * nchunks;
  s.use_events = !f.bcf_mode && events_fit_blocks && ev_blocks * (uint64_t)s.evrun * kAsmRows * entry <= k.resolved_budget_bytes;
  s.size_kernel = s.use_events ? kSizeKernelEvents : s.asm_path != 0 ? kSizeKernelPieces : size_kernel_for(k, s.run);
  s.chunk_major = k.res_chunk_major && !f.bcf_mode && s.asm_path != 2;
  s.resolved_entry_bytes = s.piece_path || k.events ? 0 : s.res_compact ? 5 : 8;
  return s;
}

// end of the page that starts at record kp: the largest ke with rec_off[ke] - rec_off[kp] <= arena_cap.  The change list is laid out
// over the interval's order blocks: a page that ends on a block boundary can use it as it is, so such a page is cut back to one.
inline int64_t page_end(const AssemblyKnobs& k, const AssemblySizing& s, const uint64_t* rec_off, int64_t kp, int64_t P, uint64_t arena_cap) {
  int64_t lo = kp + 1, hi = P;
  while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (rec_off[mid] - rec_off[kp] <= arena_cap) lo = mid; else hi = mid - 1; }
  const int64_t blk = (int64_t)1 << k.order_block_log2;
  if (s.use_events && lo < P && (kp % blk) == 0 && (lo / blk) * blk > kp) lo = (lo / blk) * blk;
  return lo;
}

struct PageChoice {
  int kernel;              // kPageKernel*
  int waves, coop_u;       // template arguments of the page kernel: wavefronts per workgroup, words per lane of the cooperative copy (0: none)
  int lds_bytes, run;      // its LDS image, records per wavefront
  int resolve_kernel;      // the page's records are resolved first (!resolved_whole): kSizeKernelPieces = k_fill2, another kSizeKernel* = that sizing kernel; -1: nothing to resolve
  int64_t res_rows;        // row count of a chunk-major matrix (0: record-major)
  bool forks;              // the kernel runs on the forked high-priority stream when page priority is on (k_bcf_write and k_assemble_write only)
  int code;                // IntervalStats::page_kernel
};

// the kernel of the page of records [kp, ke) of an interval of P records: total_bytes of text, the largest record max_record_bytes
inline PageChoice choose_page(const AssemblyKnobs& k, const AssemblySizing& s, int64_t kp, int64_t ke, int64_t P, int nchunks, uint64_t total_bytes, uint64_t max_record_bytes, bool order_iv_valid) {
  PageChoice c{};
  const int64_t blk = (int64_t)1 << k.order_block_log2;
  const int ww = k.write_waves, wl = k.image_kb(P > 0 && nchunks > 0 ? total_bytes / ((uint64_t)P * (uint64_t)nchunks) : 0);
  c.waves = 1; c.resolve_kernel = -1;
  c.run = s.piece_path ? k.run_w2 : k.run_w;
  if (s.bcf_mode) {   // k_bcf_shared, k_bcf_same_layout, k_bcf_write: one wavefront, no LDS image
    c.kernel = kPageKernelBcf; c.forks = true;
  } else if (s.use_events && order_iv_valid && (kp % blk) == 0 && (ke == P || (ke % blk) == 0)) {
    c.kernel = kPageKernelEvents; c.waves = ww >= 4 ? 4 : 1; c.lds_bytes = kWaveLds; c.run = s.evrun;
  } else if (s.asm_path == 3) {
    c.kernel = kPageKernelWrite3; c.lds_bytes = wl <= 4 ? 4096 : 8192;
  } else if (s.asm_path == 1) {
    c.kernel = kPageKernelWrite2; c.waves = ww >= 4 ? 4 : 1; c.lds_bytes = wl <= 4 ? 4096 : (wl <= 6 && ww < 4) ? 6144 : 8192;
  } else {
    c.kernel = kPageKernelWrite; c.coop_u = 2; c.forks = true;
    // the largest record's average entry is a long one (copied by the whole wavefront): the variant that keeps 4 words per lane in flight
    const bool long_entries = k.coop_unroll && nchunks > 0 && max_record_bytes / ((uint64_t)nchunks * kAsmRows) > (uint64_t)kCooperativeEntry;
    if (long_entries && ww == 1) { c.coop_u = 4; c.lds_bytes = 8192; }
    else { c.waves = ww >= 4 ? 4 : ww == 2 ? 2 : 1; c.lds_bytes = wl <= 4 ? 4096 : (wl <= 6 && ww >= 4) ? 6144 : 8192; }
    if (!s.resolved_whole) c.resolve_kernel = s.asm_path == 2 ? kSizeKernelPieces : size_kernel_for(k, c.run);
    c.res_rows = s.res_rows(s.resolved_whole ? P : ke - kp);
  }
  c.code = page_kernel_code(s.size_kernel, c.kernel, c.waves, c.coop_u, c.lds_bytes);
  return c;
}

}  // namespace genomicsdb_amd
