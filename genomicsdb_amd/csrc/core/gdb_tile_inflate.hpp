// gdb_tile_inflate.hpp - body of the tile inflater of compressed fragment files (version 3): one raw DEFLATE stream (RFC 1951) of
// a tile -> at most kTileBytes bytes, decoded front to back by ONE thread.  Plain functions that compile under g++ and hipcc
// (GDB_HD): the kernel k_inflate_tiles of kernels/gdb_pipeline.hip and the CPU harness tests/hostsim_tile_inflate/ run the same
// code.  No allocation.
//
// The writer (save_fragment, zlib with strategy Z_FIXED) emits stored and FIXED-Huffman blocks only: the decoder then needs no
// per-stream code tables - a literal / length code is 7 to 9 bits and is classified arithmetically (RFC 1951, 3.2.6).  Blocks with
// dynamic codes (a file compressed by something else) are decoded too, with tables in the caller's scratch memory.
// Every read of the stream stays inside [in, in_end), every write inside out[0, want); the scratch is kTileScratch bytes, 2-byte
// aligned.  A malformed, short or overlong stream ends in a TileErr; bytes behind the final block are not looked at.
#pragma once
#include <cstdint>

#include "gdb_types.h"

namespace genomicsdb_amd {
namespace gdbtile {

constexpr uint32_t kTileBytes = 8192;

// why a tile was refused (the counterpart of gdbinf::InfErr)
enum TileErr : uint32_t {
  TILE_OK = 0,
  TILE_ERR_BLOCK_TYPE = 1,   // reserved block type 3
  TILE_ERR_CODE = 2,         // over-subscribed or incomplete code, bad code-length repeat, too many symbols
  TILE_ERR_NO_EOB = 3,       // no end-of-block code
  TILE_ERR_SYMBOL = 4,       // length / distance symbol out of range, or bits that are no code
  TILE_ERR_DISTANCE = 5,     // distance reaches before the start of the tile
  TILE_ERR_OUTPUT = 6,       // more output than the tile's size
  TILE_ERR_INPUT = 7,        // input exhausted
  TILE_ERR_STORED_LEN = 8,   // LEN / NLEN mismatch
  TILE_ERR_SIZE = 9          // the stream ended with fewer bytes than the tile's size
};
inline const char* tile_err_text(uint32_t e) {       // (host only)
  switch (e) {
    case TILE_OK: return "no error";
    case TILE_ERR_BLOCK_TYPE: return "reserved block type";
    case TILE_ERR_CODE: return "invalid Huffman code lengths";
    case TILE_ERR_NO_EOB: return "no end-of-block code";
    case TILE_ERR_SYMBOL: return "invalid length or distance symbol";
    case TILE_ERR_DISTANCE: return "distance reaches before the start of the tile";
    case TILE_ERR_OUTPUT: return "more bytes than the tile's size";
    case TILE_ERR_INPUT: return "stream ends early";
    case TILE_ERR_STORED_LEN: return "LEN / NLEN mismatch of a stored block";
    case TILE_ERR_SIZE: return "fewer bytes than the tile's size";
  }
  return "unknown error";
}

// the base / extra-bits tables of RFC 1951, 3.2.5: in device memory for the kernel, plain arrays for the host
#if defined(__HIP_DEVICE_COMPILE__)
#define GDB_TILE_TABLE static __device__ const
#else
#define GDB_TILE_TABLE static const
#endif
GDB_TILE_TABLE uint16_t kInfLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
GDB_TILE_TABLE uint8_t kInfLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
GDB_TILE_TABLE uint16_t kInfDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
GDB_TILE_TABLE uint8_t kInfDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
#undef GDB_TILE_TABLE

// the 32 bits of v in reverse order (Huffman codes are packed most-significant bit first)
GDB_HD uint32_t tile_brev(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(v);
#else
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  return (v >> 16) | (v << 16);
#endif
}

struct InflateBits {
  const uint8_t* p; const uint8_t* end;
  uint64_t buf; int n;
  // After refill() at least 33 bits are buffered while input remains (no consumer takes more than 19 between two refills).  Eight
  // bytes at a time while they last: the stream is read front to back by one lane, one unaligned 8-byte load per 3 to 7 bytes used.
  GDB_HD void refill() {
    if (n > 32) return;
    if (p + 8 <= end) {
      uint64_t w;
      __builtin_memcpy(&w, p, 8);
      buf |= w << n;
      const int take = (63 - n) >> 3;
      p += take; n += take * 8;
      buf &= (1ull << n) - 1ull;                 // (n <= 63: the bits of the byte that was not taken are read again next time)
    } else while (n <= 56 && p < end) { buf |= (uint64_t)(*p++) << n; n += 8; }
  }
  GDB_HD uint32_t peek(int k) const { return (uint32_t)(buf & ((1ull << k) - 1ull)); }
  GDB_HD void drop(int k) { buf >>= k; n -= k; }
  GDB_HD uint32_t get(int k) { const uint32_t v = peek(k); drop(k); return v; }   // (k <= 16; refill() first)
};
// Blocks with DYNAMIC codes (what a default zlib / gzip writer produces): canonical Huffman decoding bit by bit over a count-per-length
// and a symbols-in-code-order table (RFC 1951, 3.2.2 and 3.2.7), the tables of a lane in its own slice of a global scratch buffer.
// Slower than the fixed codes (up to 15 steps per symbol, tables in memory) - the files this build writes do not need it.
struct InflateCode { uint16_t* count; uint16_t* symbol; };            // count[16], symbol[n]
constexpr int kTileScratch = 320 + 2 * (16 + 288) + 2 * (16 + 32);    // bytes per lane: code lengths, literal / length code, distance code
// one symbol: >= 0 the symbol, -1 bits that are no code, -2 input exhausted
GDB_HD int inflate_decode(InflateBits& b, const InflateCode& h) {
  int code = 0, first = 0, index = 0;
  b.refill();
  for (int len = 1; len <= 15; ++len) {
    if (b.n < 1) return -2;
    code |= (int)b.get(1);
    const int count = h.count[len];
    if (code - count < first) return h.symbol[index + (code - first)];
    index += count; first += count;
    first <<= 1; code <<= 1;
    if (len == 8) b.refill();
  }
  return -1;
}
// code lengths -> tables; returns the number of unused codes (0: complete; < 0: over-subscribed)
GDB_HD int inflate_construct(const InflateCode& h, const uint8_t* length, int n) {
  for (int len = 0; len <= 15; ++len) h.count[len] = 0;
  for (int sym = 0; sym < n; ++sym) h.count[length[sym]]++;
  if (h.count[0] == n) return 0;
  int left = 1;
  for (int len = 1; len <= 15; ++len) { left <<= 1; left -= h.count[len]; if (left < 0) return left; }
  uint16_t offs[16];
  offs[1] = 0;
  for (int len = 1; len < 15; ++len) offs[len + 1] = (uint16_t)(offs[len] + h.count[len]);
  for (int sym = 0; sym < n; ++sym) if (length[sym] != 0) h.symbol[offs[length[sym]]++] = (uint16_t)sym;
  return left;
}
// RFC 1951: a code that leaves `left` > 0 of its space unused is allowed only as ONE code of one bit (what zlib and
// core/gdb_inflate.hpp accept); n symbols were given to inflate_construct
GDB_HD bool inflate_incomplete_ok(const InflateCode& h, int n) { return h.count[1] == 1 && n - h.count[0] == 1; }
// The copy of a match: 8 bytes per load / store while the distance allows it (a copy with dist >= 8 never reads a byte its own
// current 8-byte store writes; bytes written by EARLIER stores of the same lane are seen - the vector memory pipeline keeps one
// lane's accesses to an address in order, which the byte-by-byte loop of round 2 relied on as well).  The byte loop made every
// copied byte a global load behind a global store - one memory round trip per byte, the largest item of the kernel's time.
GDB_HD void inflate_copy_match(uint8_t* o, uint32_t at, uint32_t len, uint32_t dist) {
  uint32_t i = 0;
  if (dist >= 8u)
    for (; i + 8u <= len; i += 8u) { uint64_t w; __builtin_memcpy(&w, o + at - dist + i, 8); __builtin_memcpy(o + at + i, &w, 8); }
  for (; i < len; ++i) o[at + i] = o[at + i - dist];
}

// one tile: the raw DEFLATE stream [in, in_end) -> exactly `want` <= kTileBytes bytes at `out`; scratch: kTileScratch bytes of the caller
GDB_HD TileErr tile_inflate(const uint8_t* in, const uint8_t* in_end, uint32_t want, uint8_t* out, uint8_t* scratch) {
  uint8_t* const lengths = scratch;                                                                        // [320]
  const InflateCode lencode{reinterpret_cast<uint16_t*>(lengths + 320), reinterpret_cast<uint16_t*>(lengths + 320) + 16};
  const InflateCode distcode{lencode.symbol + 288, lencode.symbol + 288 + 16};
  uint8_t* const o = out;
  InflateBits b{in, in_end, 0ull, 0};
  uint32_t at = 0;
  bool last = false;
  while (!last) {
    b.refill();
    if (b.n < 3) return TILE_ERR_INPUT;
    last = b.get(1) != 0;
    const uint32_t type = b.get(2);
    if (type == 0) {                                   // stored: LEN, NLEN, bytes
      b.drop(b.n & 7);
      b.refill();
      if (b.n < 32) return TILE_ERR_INPUT;
      const uint32_t len = b.get(16), nlen = b.get(16);
      if ((len ^ nlen) != 0xFFFFu) return TILE_ERR_STORED_LEN;
      if (at + len > want) return TILE_ERR_OUTPUT;
      for (uint32_t i = 0; i < len; ++i) { b.refill(); if (b.n < 8) return TILE_ERR_INPUT; o[at++] = (uint8_t)b.get(8); }
    } else if (type == 1) {                            // fixed Huffman codes
      for (;;) {
        b.refill();
        if (b.n < 7) return TILE_ERR_INPUT;
        uint32_t sym;
        const uint32_t c7 = tile_brev(b.peek(7)) >> 25;   // Huffman codes are packed most-significant bit first
        if (c7 <= 0x17u) { sym = 256u + c7; b.drop(7); }
        else {
          const uint32_t c8 = tile_brev(b.peek(8)) >> 24;
          if (c8 >= 0x30u && c8 <= 0xBFu) { sym = c8 - 0x30u; b.drop(8); }
          else if (c8 >= 0xC0u && c8 <= 0xC7u) { sym = 280u + (c8 - 0xC0u); b.drop(8); }
          else {
            const uint32_t c9 = tile_brev(b.peek(9)) >> 23;
            if (c9 < 0x190u) return TILE_ERR_SYMBOL;
            sym = 144u + (c9 - 0x190u); b.drop(9);
          }
        }
        if (b.n < 0) return TILE_ERR_INPUT;
        if (sym < 256u) { if (at >= want) return TILE_ERR_OUTPUT; o[at++] = (uint8_t)sym; continue; }
        if (sym == 256u) break;
        if (sym > 285u) return TILE_ERR_SYMBOL;
        b.refill();
        const uint32_t li = sym - 257u;
        const uint32_t len = kInfLenBase[li] + b.get(kInfLenExtra[li]);
        const uint32_t dc = tile_brev(b.get(5)) >> 27;
        if (dc >= 30u) return b.n < 0 ? TILE_ERR_INPUT : TILE_ERR_SYMBOL;
        b.refill();
        const uint32_t dist = kInfDistBase[dc] + b.get(kInfDistExtra[dc]);
        if (b.n < 0) return TILE_ERR_INPUT;
        if (dist > at) return TILE_ERR_DISTANCE;
        if (at + len > want) return TILE_ERR_OUTPUT;
        inflate_copy_match(o, at, len, dist);
        at += len;
      }
    } else if (type == 2) {                            // dynamic codes: read the code lengths, build both tables, decode
      b.refill();
      if (b.n < 14) return TILE_ERR_INPUT;
      const int nlen = (int)b.get(5) + 257, ndist = (int)b.get(5) + 1, ncode = (int)b.get(4) + 4;
      if (nlen > 286 || ndist > 30) return TILE_ERR_CODE;
      const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      for (int i = 0; i < 19; ++i) lengths[i] = 0;
      for (int i = 0; i < ncode; ++i) { b.refill(); if (b.n < 3) return TILE_ERR_INPUT; lengths[order[i]] = (uint8_t)b.get(3); }
      if (inflate_construct(lencode, lengths, 19) != 0) return TILE_ERR_CODE;       // the code-length code must be complete
      int index = 0;
      while (index < nlen + ndist) {
        int sym = inflate_decode(b, lencode);
        if (sym < 0) return sym == -2 ? TILE_ERR_INPUT : TILE_ERR_CODE;
        if (sym < 16) lengths[index++] = (uint8_t)sym;
        else {
          int rep_len = 0;
          b.refill();
          if (sym == 16) { if (index == 0) return TILE_ERR_CODE; rep_len = lengths[index - 1]; sym = 3 + (int)b.get(2); }
          else if (sym == 17) sym = 3 + (int)b.get(3);
          else sym = 11 + (int)b.get(7);
          if (b.n < 0) return TILE_ERR_INPUT;
          if (index + sym > nlen + ndist) return TILE_ERR_CODE;
          while (sym--) lengths[index++] = (uint8_t)rep_len;
        }
      }
      if (lengths[256] == 0) return TILE_ERR_NO_EOB;                                // no end-of-block code
      // (the distance lengths are moved aside first: building the literal / length tables must not clobber them)
      uint8_t dlen[30];
      for (int i = 0; i < ndist; ++i) dlen[i] = lengths[nlen + i];
      int rc = inflate_construct(lencode, lengths, nlen);
      if (rc < 0 || (rc > 0 && !inflate_incomplete_ok(lencode, nlen))) return TILE_ERR_CODE;
      rc = inflate_construct(distcode, dlen, ndist);
      if (rc < 0 || (rc > 0 && !inflate_incomplete_ok(distcode, ndist))) return TILE_ERR_CODE;
      for (;;) {
        const int sym = inflate_decode(b, lencode);
        if (sym < 0) return sym == -2 ? TILE_ERR_INPUT : TILE_ERR_SYMBOL;
        if (sym < 256) { if (at >= want) return TILE_ERR_OUTPUT; o[at++] = (uint8_t)sym; continue; }
        if (sym == 256) break;
        if (sym > 285) return TILE_ERR_SYMBOL;
        b.refill();
        const uint32_t li = (uint32_t)sym - 257u;
        const uint32_t len = kInfLenBase[li] + b.get(kInfLenExtra[li]);
        const int dc = inflate_decode(b, distcode);
        if (dc < 0) return dc == -2 || b.n < 0 ? TILE_ERR_INPUT : TILE_ERR_SYMBOL;
        if (dc >= 30) return TILE_ERR_SYMBOL;
        b.refill();
        const uint32_t dist = kInfDistBase[dc] + b.get(kInfDistExtra[dc]);
        if (b.n < 0) return TILE_ERR_INPUT;
        if (dist > at) return TILE_ERR_DISTANCE;
        if (at + len > want) return TILE_ERR_OUTPUT;
        inflate_copy_match(o, at, len, dist);
        at += len;
      }
    } else return TILE_ERR_BLOCK_TYPE;                 // the reserved block type
  }
  return at == want ? TILE_OK : TILE_ERR_SIZE;
}

}  // namespace gdbtile
}  // namespace genomicsdb_amd
