// gdb_inflate.h - BGZF (blocked gzip) input inflated ON THE DEVICE: the counterpart of gdb_bgzf.h, and the front of the device
// importer (gdb_import.hip).  Host-visible interface, no HIP types.
//
// A BGZF file is a chain of gzip members of at most 64 KiB of data each; a member's header gives its compressed size (the "BC"
// extra subfield), its trailer the CRC32 and the size of the data.  The host walks that chain (bgzf_walk), so the members are
// independent work with known output offsets (a host prefix sum of ISIZE); the device inflates one member per wavefront with the
// bodies of core/gdb_inflate.hpp and verifies stream, length and CRC32 of every member.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace genomicsdb_amd {

struct BgzfMember {
  uint64_t offset;        // of the member in the file
  uint32_t data_off;      // of its raw DEFLATE stream, from `offset`
  uint32_t data_len;
  uint32_t isize, crc;    // the trailer
  uint64_t out_off;       // of its data in the inflated file
};

// true: p[0, n) is BGZF from byte 0 to byte n - magic 1f 8b 08 04, a "BC" subfield of 2 bytes, BSIZE, trailer, ISIZE <= 65 536 in
// every member - and n > 0.  Anything else (plain gzip, plain text, a chain that breaks) is not BGZF; *break_at: where the chain breaks.
inline bool bgzf_walk(const uint8_t* p, uint64_t n, std::vector<BgzfMember>& members, uint64_t* total_out, uint64_t* break_at = nullptr) {
  members.clear();
  uint64_t at = 0, out = 0;
  struct Note { uint64_t* to; const uint64_t& at; ~Note() { if (to) *to = at; } } note{break_at, at};
  auto u16 = [&](uint64_t i) { return (uint32_t)p[i] | (uint32_t)p[i + 1] << 8; };
  auto u32 = [&](uint64_t i) { return u16(i) | u16(i + 2) << 16; };
  while (at < n) {
    if (n - at < 12u + 6u + 8u || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || p[at + 3] != 4) return false;
    const uint32_t xlen = u16(at + 10);
    if (n - at < 12u + (uint64_t)xlen + 8u) return false;
    uint32_t bsize = 0, x = 0;
    bool found = false;
    while (x + 4u <= xlen) {
      const uint64_t f = at + 12u + x;
      const uint32_t slen = u16(f + 2);
      if (x + 4u + slen > xlen) return false;
      if (p[f] == 'B' && p[f + 1] == 'C' && slen == 2u) { bsize = u16(f + 4) + 1u; found = true; }
      x += 4u + slen;
    }
    if (!found || x != xlen || bsize < 12u + xlen + 8u || bsize > n - at) return false;
    BgzfMember m;
    m.offset = at; m.data_off = 12u + xlen; m.data_len = bsize - m.data_off - 8u;
    m.crc = u32(at + bsize - 8u); m.isize = u32(at + bsize - 4u);
    m.out_off = out;
    if (m.isize > 65536u) return false;
    members.push_back(m);
    out += m.isize;
    at += bsize;
  }
  if (total_out) *total_out = out;
  return !members.empty();
}

// the 18 bytes a BGZF file begins with when "BC" is its first subfield, as bgzip and htslib write it (a cheap test before a file is read whole)
inline bool bgzf_begins(const uint8_t* p) {
  return p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && p[3] == 4 && p[12] == 'B' && p[13] == 'C' && p[14] == 2 && p[15] == 0;
}

// text of an InfErr (core/gdb_inflate.hpp)
const char* bgzf_inflate_error_text(uint32_t err);

class BgzfDeviceInflater {
 public:
  enum Kernel { kWavePerMember = 0, kThreadPerMember = 1 };     // the A/B of profiles/device_inflate.md (the device importer maps GDBAMD_INFLATE_KERNEL=wave|thread to it)
  BgzfDeviceInflater();
  ~BgzfDeviceInflater();
  BgzfDeviceInflater(const BgzfDeviceInflater&) = delete;
  BgzfDeviceInflater& operator=(const BgzfDeviceInflater&) = delete;
  void set_kernel(Kernel k);
  // Members [m0, m1) of the file at host_src: their bytes are uploaded and inflated to dev_dst + (out_off - members[m0].out_off);
  // dev_dst holds at least the sum of their ISIZE.  `stream`: a hipStream_t (null: the default stream); the call returns after
  // the kernel has finished.  Returns -1 when every member is a valid stream of ISIZE bytes with the trailer's CRC32, else the
  // index of the first member that is not, its InfErr in *err; nothing of dev_dst is then to be used.
  int64_t inflate(const uint8_t* host_src, const BgzfMember* members, size_t m0, size_t m1, uint8_t* dev_dst, void* stream, uint32_t* err);
  float ms_kernel = 0;            // HIP-event time of the inflate kernel, summed
  float ms_upload = 0;            // HIP-event time of the uploads in front of it, summed
  uint64_t bytes_h2d = 0;         // compressed bytes and member descriptors uploaded, summed
 private:
  struct Impl;
  Impl* m_;
};

}  // namespace genomicsdb_amd
