// gdb_inflate.hpp - bodies of the BGZF inflater: one raw DEFLATE stream (RFC 1951) of a BGZF member -> at most 65 536 bytes, plus
// the CRC32 of those bytes.  Plain functions that compile under g++ and hipcc (GDB_HD): the kernels of kernels/gdb_inflate.hip and
// the CPU harness tests/hostsim_inflate/ run the same code, the driver inf_member included.  No allocation.
//
// The work of a member is cut into PHASES; a cooperative phase takes (lane, nlanes) and touches only what no other lane of the
// same phase touches, so "all lanes, then a barrier" (a wavefront) and "a loop over the lanes" (the harness, or one thread alone)
// give the same bytes.  `Exec` runs a phase: see InfLoopExec below and InfWaveExec in the kernel file.
//   stage    cooperative: the next kInBuf compressed bytes -> S.in (the decoder never reads the stream itself, and never past it)
//   serial   lane 0: a block header (stored: LEN / NLEN; fixed / dynamic: the code lengths, their counts, the canonical codes,
//            the symbols in code order) or a decode round: literals go straight to `out`, matches are queued
//   tables   cooperative: clear and fill the primary lookup tables (kLitBits / kDistBits bits; entry = symbol << 4 | length); a
//            code longer than the table leaves its entries 0 and is decoded canonically, bit by bit, from counts and symbols
//   copy     cooperative, one queued match after the other: consecutive lanes copy consecutive bytes (distance < length: the
//            pattern repeats, byte i comes from i mod distance); a stored block is one such copy from the stream
//   crc      cooperative: CRC32 of one chunk per lane, then lane 0 joins them: crc(A|B) = crc(A) * x^(8 len B) mod P  xor  crc(B)
// Every read of the stream is bounded by the member's end, every write by `isize`; a malformed stream ends in an InfErr.
#pragma once
#include <cstdint>

#include "gdb_types.h"

namespace genomicsdb_amd {
namespace gdbinf {

constexpr uint32_t kMaxOut = 65536u;      // ISIZE of a BGZF member is at most this
constexpr uint32_t kLitBits = 10u, kDistBits = 8u;
constexpr uint32_t kInBuf = 2048u;        // staged compressed bytes per round
constexpr uint32_t kInMargin = 16u;       // a round ends when fewer staged bytes than this are left (a token takes at most 48 bits)
constexpr uint32_t kQueue = 512u;         // matches per round
constexpr uint32_t kMaxLanes = 64u;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

enum InfErr : uint32_t {
  INF_OK = 0,
  INF_ERR_BLOCK_TYPE = 1,   // reserved block type 3
  INF_ERR_CODE = 2,         // over-subscribed or incomplete code, bad code-length repeat, too many symbols
  INF_ERR_NO_EOB = 3,       // no end-of-block code
  INF_ERR_SYMBOL = 4,       // length / distance symbol out of range, or bits that are no code
  INF_ERR_DISTANCE = 5,     // distance reaches before the start of the member
  INF_ERR_OUTPUT = 6,       // more output than ISIZE
  INF_ERR_INPUT = 7,        // input exhausted
  INF_ERR_STORED_LEN = 8,   // LEN / NLEN mismatch
  INF_ERR_ISIZE = 9,        // the stream ended with fewer bytes than ISIZE
  INF_ERR_CRC = 10
};
enum { INF_ACT_NONE = 0, INF_ACT_TABLES = 1, INF_ACT_STORED = 2, INF_ACT_MATCHES = 3 };

struct InfCode { uint16_t count[16]; uint16_t sym[288]; };      // canonical form: codes per length, symbols in code order

struct InfState {
  // control, written by lane 0 in the serial phase only
  uint32_t err, done, action, in_block, last_block;
  uint32_t out_pos;                 // bytes decoded so far
  uint32_t in_pos;                  // stream bytes taken into the bit buffer
  uint32_t bit_cnt; uint64_t bit_buf;
  uint32_t nq;                      // queued matches
  uint32_t stored_src, stored_len;
  uint32_t nlit, ndist;
  uint32_t crc;
  // tables
  uint16_t lit_tab[1u << kLitBits], dist_tab[1u << kDistBits];
  InfCode lit, dist;
  uint8_t lens[320];
  uint16_t code[320];               // canonical code of each symbol (literal/length symbols, then distance symbols)
  uint32_t q_pos_len[kQueue]; uint16_t q_dist[kQueue];      // pos | len << 16
  uint32_t lane_crc[kMaxLanes];
  uint8_t in[kInBuf];
};

struct InfBits { const uint8_t* in; uint32_t base, lim, pos, cnt; uint64_t buf; };

GDB_HD void inf_refill(InfBits& b) {
  while (b.cnt <= 56u && b.pos < b.lim) { b.buf |= (uint64_t)b.in[b.pos - b.base] << b.cnt; ++b.pos; b.cnt += 8u; }
}
// k <= 16 bits; false: the input is exhausted
GDB_HD bool inf_take(InfBits& b, uint32_t k, uint32_t* v) {
  if (b.cnt < k) { inf_refill(b); if (b.cnt < k) return false; }
  *v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
  b.buf >>= k; b.cnt -= k;
  return true;
}
GDB_HD uint32_t inf_reverse(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
  return r;
}

// lengths -> counts, symbols in code order, the code of every symbol.  Returns what is left of the code space: 0 complete,
// > 0 incomplete, < 0 over-subscribed.
GDB_HD int inf_construct(InfCode& h, const uint8_t* lens, uint32_t n, uint16_t* code) {
  uint16_t offs[16], next[16];
  for (uint32_t l = 0; l < 16u; ++l) h.count[l] = 0;
  for (uint32_t s = 0; s < n; ++s) ++h.count[lens[s] & 15u];
  int left = 1;
  for (uint32_t l = 1; l < 16u; ++l) { left <<= 1; left -= (int)h.count[l]; if (left < 0) return left; }
  offs[1] = 0; next[1] = 0;
  for (uint32_t l = 1; l < 15u; ++l) { offs[l + 1u] = (uint16_t)(offs[l] + h.count[l]); next[l + 1u] = (uint16_t)((next[l] + h.count[l]) << 1); }
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15u;
    if (l) { h.sym[offs[l]++] = (uint16_t)s; code[s] = next[l]++; }
  }
  return left;
}

// one symbol: >= 0 the symbol, -1 bits that are no code, -2 input exhausted
GDB_HD int inf_decode(const uint16_t* tab, uint32_t tab_bits, const InfCode& h, InfBits& b) {
  inf_refill(b);
  const uint32_t e = tab[b.buf & ((1u << tab_bits) - 1u)], len = e & 15u;
  if (len) {
    if (len > b.cnt) return -2;
    b.buf >>= len; b.cnt -= len;
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;       // the overflow of long codes (and bits that are no code at all)
  for (uint32_t l = 1; l <= 15u; ++l) {
    if (l > b.cnt) return -2;
    code |= (int)((b.buf >> (l - 1u)) & 1u);
    const int count = (int)h.count[l];
    if (code - count < first) { b.buf >>= l; b.cnt -= l; return (int)h.sym[index + (code - first)]; }
    index += count; first += count; first <<= 1; code <<= 1;
  }
  return -1;
}

// ---- phases

GDB_HD void inf_phase_stage(InfState& S, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t nlanes) {
  const uint32_t base = S.in_pos;
  for (uint32_t i = lane; i < kInBuf; i += nlanes) S.in[i] = base + i < n && base + i >= base ? src[base + i] : (uint8_t)0;
}

GDB_HD void inf_load_bits(const InfState& S, uint32_t n, InfBits& b) {
  b.in = S.in; b.base = S.in_pos; b.pos = S.in_pos; b.cnt = S.bit_cnt; b.buf = S.bit_buf;
  b.lim = n - b.base < kInBuf ? n : b.base + kInBuf;        // (in_pos <= n always)
}
GDB_HD void inf_save_bits(InfState& S, const InfBits& b) { S.in_pos = b.pos; S.bit_cnt = b.cnt; S.bit_buf = b.buf; }

// a block header: S.action = INF_ACT_STORED (S.stored_src / S.stored_len) or INF_ACT_TABLES (S.lens, S.lit, S.dist, S.code)
GDB_HD uint32_t inf_header(InfState& S, uint32_t n, uint32_t isize) {
  InfBits b;
  inf_load_bits(S, n, b);
  uint32_t v;
  if (!inf_take(b, 3u, &v)) return INF_ERR_INPUT;
  S.last_block = v & 1u;
  const uint32_t type = v >> 1;
  if (type == 3u) return INF_ERR_BLOCK_TYPE;
  if (type == 0u) {
    // the rest of the current byte is dropped; whole bytes still in the bit buffer are given back to the stream
    b.buf >>= (b.cnt & 7u); b.cnt &= ~7u;
    uint32_t len, nlen;
    if (!inf_take(b, 16u, &len) || !inf_take(b, 16u, &nlen)) return INF_ERR_INPUT;
    if ((len ^ 0xFFFFu) != nlen) return INF_ERR_STORED_LEN;
    const uint32_t at = b.pos - b.cnt / 8u;
    if (len > n - at) return INF_ERR_INPUT;
    if (len > isize - S.out_pos) return INF_ERR_OUTPUT;
    S.stored_src = at; S.stored_len = len;
    S.in_pos = at + len; S.bit_cnt = 0; S.bit_buf = 0;
    S.action = INF_ACT_STORED;
    return INF_OK;
  }
  uint32_t nlit, ndist;
  if (type == 1u) {
    nlit = 288u; ndist = 30u;
    for (uint32_t s = 0; s < 288u; ++s) S.lens[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8);
    for (uint32_t s = 0; s < 30u; ++s) S.lens[288u + s] = 5;
  } else {
    uint32_t ncode;
    if (!inf_take(b, 5u, &nlit) || !inf_take(b, 5u, &ndist) || !inf_take(b, 4u, &ncode)) return INF_ERR_INPUT;
    nlit += 257u; ndist += 1u; ncode += 4u;
    if (nlit > 286u || ndist > 30u) return INF_ERR_CODE;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (uint32_t i = 0; i < 19u; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) { if (!inf_take(b, 3u, &v)) return INF_ERR_INPUT; cl[order[i]] = (uint8_t)v; }
    // the code-length code: a 7-bit table of its own, in the literal table's place (which is filled only afterwards)
    if (inf_construct(S.lit, cl, 19u, S.code) != 0) return INF_ERR_CODE;
    uint16_t* tab = S.lit_tab;
    for (uint32_t i = 0; i < 128u; ++i) tab[i] = 0;
    for (uint32_t s = 0; s < 19u; ++s) {
      const uint32_t l = cl[s];
      if (l) for (uint32_t i = inf_reverse(S.code[s], l); i < 128u; i += 1u << l) tab[i] = (uint16_t)(s << 4 | l);
    }
    uint32_t at = 0;
    while (at < nlit + ndist) {
      inf_refill(b);
      const uint32_t e = tab[b.buf & 127u], l = e & 15u;
      if (!l) return INF_ERR_CODE;
      if (l > b.cnt) return INF_ERR_INPUT;
      b.buf >>= l; b.cnt -= l;
      const uint32_t s = e >> 4;
      if (s < 16u) { S.lens[at++] = (uint8_t)s; continue; }
      uint32_t rep, val = 0;
      if (s == 16u) { if (!at) return INF_ERR_CODE; val = S.lens[at - 1u]; if (!inf_take(b, 2u, &rep)) return INF_ERR_INPUT; rep += 3u; }
      else if (s == 17u) { if (!inf_take(b, 3u, &rep)) return INF_ERR_INPUT; rep += 3u; }
      else { if (!inf_take(b, 7u, &rep)) return INF_ERR_INPUT; rep += 11u; }
      if (at + rep > nlit + ndist) return INF_ERR_CODE;
      while (rep--) S.lens[at++] = (uint8_t)val;
    }
    if (S.lens[256] == 0) return INF_ERR_NO_EOB;
    // the distance lengths move behind the 288 literal/length slots
    for (uint32_t s = ndist; s-- > 0u;) S.lens[288u + s] = S.lens[nlit + s];
    for (uint32_t s = nlit; s < 288u; ++s) S.lens[s] = 0;
  }
  // RFC 1951: an incomplete code is allowed only as ONE code of one bit (or, for distances, no code at all)
  const int left_l = inf_construct(S.lit, S.lens, nlit, S.code);
  if (left_l < 0 || (type == 2u && left_l > 0 && !(S.lit.count[1] == 1u && nlit - S.lit.count[0] == 1u))) return INF_ERR_CODE;
  const int left_d = inf_construct(S.dist, S.lens + 288, ndist, S.code + 288);
  if (left_d < 0 || (type == 2u && left_d > 0 && ndist - S.dist.count[0] != 0u && !(S.dist.count[1] == 1u && ndist - S.dist.count[0] == 1u))) return INF_ERR_CODE;
  S.nlit = nlit; S.ndist = ndist;
  inf_save_bits(S, b);
  S.action = INF_ACT_TABLES;
  return INF_OK;
}

GDB_HD void inf_phase_clear(InfState& S, uint32_t lane, uint32_t nlanes) {
  for (uint32_t i = lane; i < (1u << kLitBits); i += nlanes) S.lit_tab[i] = 0;
  for (uint32_t i = lane; i < (1u << kDistBits); i += nlanes) S.dist_tab[i] = 0;
}
// one symbol per lane and step; the entries of two symbols never coincide (the code is prefix-free: checked by inf_construct)
GDB_HD void inf_phase_fill(InfState& S, uint32_t lane, uint32_t nlanes) {
  for (uint32_t s = lane; s < 320u; s += nlanes) {
    const bool is_dist = s >= 288u;
    if (is_dist ? s - 288u >= S.ndist : s >= S.nlit) continue;
    const uint32_t l = S.lens[s], bits = is_dist ? kDistBits : kLitBits;
    if (!l || l > bits) continue;
    uint16_t* tab = is_dist ? S.dist_tab : S.lit_tab;
    const uint16_t e = (uint16_t)((is_dist ? s - 288u : s) << 4 | l);
    for (uint32_t i = inf_reverse(S.code[s], l); i < (1u << bits); i += 1u << l) tab[i] = e;
  }
}

// a decode round: until the end of the block, a full queue or the end of the staged input
GDB_HD uint32_t inf_round(InfState& S, uint32_t n, uint8_t* out, uint32_t isize) {
  InfBits b;
  inf_load_bits(S, n, b);
  uint32_t pos = S.out_pos, nq = 0, err = INF_OK;
  for (;;) {
    if (nq == kQueue || (b.lim != n && b.pos + kInMargin > b.lim)) break;
    const int sym = inf_decode(S.lit_tab, kLitBits, S.lit, b);
    if (sym < 0) { err = sym == -2 ? INF_ERR_INPUT : INF_ERR_SYMBOL; break; }
    if (sym < 256) {
      if (pos >= isize) { err = INF_ERR_OUTPUT; break; }
      out[pos++] = (uint8_t)sym;
      continue;
    }
    if (sym == 256) { S.in_block = 0; if (S.last_block) S.done = 1; break; }
    if (sym > 285) { err = INF_ERR_SYMBOL; break; }
    const uint32_t li = (uint32_t)sym - 257u;
    uint32_t len, extra = 0, v = 0;
    if (li < 8u) len = 3u + li;
    else if (li == 28u) len = 258u;
    else { extra = (li >> 2) - 1u; len = 3u + ((4u + (li & 3u)) << extra); }
    if (extra) { if (!inf_take(b, extra, &v)) { err = INF_ERR_INPUT; break; } len += v; }
    const int ds = inf_decode(S.dist_tab, kDistBits, S.dist, b);
    if (ds < 0) { err = ds == -2 ? INF_ERR_INPUT : INF_ERR_SYMBOL; break; }
    if (ds > 29) { err = INF_ERR_SYMBOL; break; }
    uint32_t dist;
    extra = 0;
    if (ds < 4) dist = 1u + (uint32_t)ds;
    else { extra = ((uint32_t)ds >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)ds & 1u)) << extra); }
    if (extra) { if (!inf_take(b, extra, &v)) { err = INF_ERR_INPUT; break; } dist += v; }
    if (dist > pos) { err = INF_ERR_DISTANCE; break; }
    if (len > isize - pos) { err = INF_ERR_OUTPUT; break; }
    S.q_pos_len[nq] = pos | len << 16; S.q_dist[nq] = (uint16_t)(dist - 1u);
    ++nq;
    pos += len;
  }
  inf_save_bits(S, b);
  S.out_pos = pos; S.nq = nq;
  S.action = INF_ACT_MATCHES;
  return err;
}

GDB_HD void inf_phase_serial(InfState& S, uint32_t n, uint8_t* out, uint32_t isize, uint32_t lane) {
  if (lane != 0u) return;
  S.action = INF_ACT_NONE; S.nq = 0;
  const uint32_t err = S.in_block ? inf_round(S, n, out, isize) : inf_header(S, n, isize);
  if (err) S.err = err;
}

// queued match m: pos + len <= isize and dist <= pos were checked when it was queued
GDB_HD void inf_phase_match(const InfState& S, uint8_t* out, uint32_t m, uint32_t lane, uint32_t nlanes) {
  const uint32_t pl = S.q_pos_len[m], pos = pl & 0xFFFFu, len = pl >> 16, dist = (uint32_t)S.q_dist[m] + 1u;
  const uint8_t* from = out + (pos - dist);
  if (dist >= len) for (uint32_t i = lane; i < len; i += nlanes) out[pos + i] = from[i];
  else for (uint32_t i = lane; i < len; i += nlanes) out[pos + i] = from[i % dist];
}
GDB_HD void inf_phase_stored(InfState& S, const uint8_t* src, uint8_t* out, uint32_t lane, uint32_t nlanes) {
  const uint32_t at = S.out_pos;
  for (uint32_t i = lane; i < S.stored_len; i += nlanes) out[at + i] = src[S.stored_src + i];
}
GDB_HD void inf_after_stored(InfState& S, uint32_t lane) {
  if (lane != 0u) return;
  S.out_pos += S.stored_len;
  if (S.last_block) S.done = 1;
}

// ---- CRC32 (reflected, polynomial 0xEDB88320); a polynomial is held with x^0 in bit 31
GDB_HD uint32_t inf_crc_bytes(const uint8_t* p, uint32_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  }
  return ~c;
}
GDB_HD uint32_t inf_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
GDB_HD uint32_t inf_xpow8(uint32_t len) {       // x^(8 len) mod P
  uint32_t r = 1u << 31, sq = 1u << 23;          // x^0, x^8
  for (; len; len >>= 1) { if (len & 1u) r = inf_mulmod(sq, r); sq = inf_mulmod(sq, sq); }
  return r;
}
GDB_HD uint32_t inf_crc_chunk(uint32_t total, uint32_t nlanes) { return (total + nlanes - 1u) / nlanes; }
GDB_HD void inf_phase_crc(InfState& S, const uint8_t* out, uint32_t total, uint32_t lane, uint32_t nlanes) {
  const uint32_t chunk = inf_crc_chunk(total, nlanes), b = lane * chunk;
  if (lane < kMaxLanes) S.lane_crc[lane] = b < total ? inf_crc_bytes(out + b, total - b < chunk ? total - b : chunk) : 0u;
}
GDB_HD void inf_phase_verify(InfState& S, uint32_t total, uint32_t isize, uint32_t want_crc, uint32_t lane, uint32_t nlanes) {
  if (lane != 0u) return;
  const uint32_t chunk = inf_crc_chunk(total, nlanes), xp = inf_xpow8(chunk);
  uint32_t crc = 0;
  for (uint32_t l = 0; l < nlanes && l * chunk < total; ++l) {
    const uint32_t len = total - l * chunk < chunk ? total - l * chunk : chunk;
    crc = inf_mulmod(len == chunk ? xp : inf_xpow8(len), crc) ^ S.lane_crc[l];
  }
  S.crc = crc;
  if (!S.err && total != isize) S.err = INF_ERR_ISIZE;
  if (!S.err && crc != want_crc) S.err = INF_ERR_CRC;
}

GDB_HD void inf_init(InfState& S, uint32_t lane) {
  if (lane != 0u) return;
  S.err = 0; S.done = 0; S.action = 0; S.in_block = 0; S.last_block = 0; S.out_pos = 0; S.in_pos = 0; S.bit_cnt = 0; S.bit_buf = 0; S.nq = 0;
  S.stored_src = 0; S.stored_len = 0; S.nlit = 0; S.ndist = 0; S.crc = 0;
}

// runs every lane of a phase one after the other: the CPU harness (nlanes = 64) and one thread alone (nlanes = 1)
struct InfLoopExec {
  uint32_t nlanes;
  template <class F> GDB_HD void operator()(F f) const { for (uint32_t l = 0; l < nlanes; ++l) f(l, nlanes); }
};

// One member: src[0, n) is its raw DEFLATE stream, out has room for isize <= kMaxOut bytes.  Every lane of a wavefront calls this
// with the same arguments (control flow depends only on S, read behind a barrier); returns the InfErr, the same on every lane.
template <class Exec>
GDB_HD uint32_t inf_member(const Exec& ex, InfState& S, const uint8_t* src, uint32_t n, uint8_t* out, uint32_t isize, uint32_t want_crc) {
  ex([&](uint32_t lane, uint32_t) { inf_init(S, lane); });
  if (isize > kMaxOut) isize = kMaxOut;       // (the host never sends more)
  for (;;) {
    ex([&](uint32_t lane, uint32_t nl) { inf_phase_stage(S, src, n, lane, nl); });
    ex([&](uint32_t lane, uint32_t) { inf_phase_serial(S, n, out, isize, lane); });
    const uint32_t action = S.action, nq = S.nq, err = S.err, done = S.done;
    if (action == INF_ACT_TABLES && !err) {
      ex([&](uint32_t lane, uint32_t nl) { inf_phase_clear(S, lane, nl); });
      ex([&](uint32_t lane, uint32_t nl) { inf_phase_fill(S, lane, nl); if (lane == 0u) S.in_block = 1; });
    } else if (action == INF_ACT_STORED && !err) {
      ex([&](uint32_t lane, uint32_t nl) { inf_phase_stored(S, src, out, lane, nl); });
      ex([&](uint32_t lane, uint32_t) { inf_after_stored(S, lane); });
    } else if (action == INF_ACT_MATCHES) {
      // (also after an error: the queued matches are all valid, and the round's bytes stay defined)
      for (uint32_t m = 0; m < nq; ++m) ex([&](uint32_t lane, uint32_t nl) { inf_phase_match(S, out, m, lane, nl); });
    }
    if (err || done || S.done) break;
  }
  const uint32_t total = S.out_pos;
  ex([&](uint32_t lane, uint32_t nl) { inf_phase_crc(S, out, total, lane, nl); });
  ex([&](uint32_t lane, uint32_t nl) { inf_phase_verify(S, total, isize, want_crc, lane, nl); });
  return S.err;
}

}  // namespace gdbinf
}  // namespace genomicsdb_amd
