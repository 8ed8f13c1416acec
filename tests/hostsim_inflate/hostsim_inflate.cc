// hostsim_inflate.cc - the bodies of the BGZF inflater (core/gdb_inflate.hpp) driven on the CPU: inf_member with a loop over
// emulated lanes in place of a wavefront, and the host's walk over the member headers (kernels/gdb_inflate.h).  Test
// infrastructure only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../genomicsdb_amd/csrc/core/gdb_inflate.hpp"
#include "../../genomicsdb_amd/csrc/kernels/gdb_inflate.h"

using namespace genomicsdb_amd;
using namespace genomicsdb_amd::gdbinf;

extern "C" {

// one raw DEFLATE stream -> out (room for `isize` bytes); returns the InfErr, *out_len / *crc: what was decoded
int hostsim_inflate_member(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t isize, uint32_t want_crc, uint32_t nlanes, uint32_t* out_len, uint32_t* crc) {
  if (nlanes == 0 || nlanes > kMaxLanes || isize > kMaxOut) return -1;
  std::vector<uint8_t> in(src, src + n);          // exact size: a read past the member's end is a heap overflow a sanitizer sees
  std::vector<uint8_t> buf(isize);
  InfState* S = new InfState;
  memset(S, 0xA5, sizeof(*S));
  const uint32_t err = inf_member(InfLoopExec{nlanes}, *S, in.data(), n, buf.data(), isize, want_crc);
  if (out_len) *out_len = S->out_pos;
  if (crc) *crc = S->crc;
  if (isize) memcpy(out, buf.data(), isize);
  delete S;
  return (int)err;
}

// a whole BGZF buffer: 0 and *dst_len, -1 not BGZF, -2 dst too small, else 1 + the index of the first bad member (*err: its InfErr, *bad_offset: its offset)
int hostsim_inflate_bgzf(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, uint32_t nlanes, uint32_t* err, uint64_t* bad_offset) {
  std::vector<BgzfMember> mem;
  uint64_t total = 0;
  if (!bgzf_walk(src, n, mem, &total)) return -1;
  if (total > dst_cap) return -2;
  for (size_t i = 0; i < mem.size(); ++i) {
    const BgzfMember& m = mem[i];
    uint32_t got = 0, crc = 0;
    std::vector<uint8_t> out(m.isize ? m.isize : 1);
    const int e = hostsim_inflate_member(src + m.offset + m.data_off, m.data_len, out.data(), m.isize, m.crc, nlanes, &got, &crc);
    if (e) { if (err) *err = (uint32_t)e; if (bad_offset) *bad_offset = m.offset; return 1 + (int)i; }
    if (m.isize) memcpy(dst + m.out_off, out.data(), m.isize);
  }
  if (dst_len) *dst_len = total;
  return 0;
}

uint32_t hostsim_inflate_state_bytes() { return (uint32_t)sizeof(InfState); }

}  // extern "C"
