// hostsim_tile_inflate.cc - the body of the tile inflater of compressed fragment files (core/gdb_tile_inflate.hpp) driven on the
// CPU: gdbtile::tile_inflate, the function every thread of k_inflate_tiles calls, over one tile at a time.  Every tile gets a heap
// copy of its stream of the exact size and an output slot of exactly kTileBytes bytes prefilled with a pattern: a read or write
// out of bounds is a heap overflow a sanitizer sees (tile_inflate_fuzz), a write behind `want` a changed pattern byte the caller
// sees.  Test infrastructure only.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../genomicsdb_amd/csrc/core/gdb_tile_inflate.hpp"

using namespace genomicsdb_amd::gdbtile;

extern "C" {

// one raw DEFLATE stream -> slot (kTileBytes bytes: the decoded bytes, then `fill`); returns the TileErr, -1: want too large
int hostsim_tile_inflate(const uint8_t* src, uint32_t n, uint32_t want, uint8_t fill, uint8_t* slot) {
  if (want > kTileBytes) return -1;
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(in, src, n);
  uint8_t* out = (uint8_t*)malloc(kTileBytes);
  memset(out, fill, kTileBytes);
  uint16_t* scratch = (uint16_t*)malloc(kTileScratch);      // (2-byte aligned, as a lane's slice of the kernel's scratch buffer is)
  memset(scratch, 0xA5, kTileScratch);                       // the kernel's scratch is not cleared between launches either
  const TileErr e = tile_inflate(in, in + n, want, out, (uint8_t*)scratch);
  memcpy(slot, out, kTileBytes);
  free(scratch); free(out); free(in);
  return (int)e;
}

// the kernel's job list: stream t = src[in_off[t], in_off[t + 1]) -> slot t of out, status[t] = its TileErr
int hostsim_tile_inflate_many(const uint8_t* src, const uint64_t* in_off, const uint32_t* want, uint64_t ntiles, uint8_t fill, uint8_t* out, uint8_t* status) {
  for (uint64_t t = 0; t < ntiles; ++t) {
    const int e = hostsim_tile_inflate(src + in_off[t], (uint32_t)(in_off[t + 1] - in_off[t]), want[t], fill, out + t * kTileBytes);
    if (e < 0) return -1;
    status[t] = (uint8_t)e;
  }
  return 0;
}

uint32_t hostsim_tile_bytes() { return kTileBytes; }
uint32_t hostsim_tile_scratch_bytes() { return (uint32_t)kTileScratch; }
const char* hostsim_tile_err_text(uint32_t e) { return tile_err_text(e); }

}  // extern "C"
