// inflate_fuzz.cc - stand-alone driver of the bodies of the BGZF inflater (core/gdb_inflate.hpp, through hostsim_inflate.cc) over
// seeded mutations of valid members, meant for a sanitizer build on the CPU (see the Makefile).  Every stream is copied into a
// heap block of its exact size and the output block has exactly ISIZE bytes, so a read or write out of bounds is an error the
// sanitizer reports.  A result is either zlib's bytes with the trailer's CRC32, or an error code.  Test infrastructure only.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int hostsim_inflate_member(const uint8_t* src, uint32_t n, uint8_t* out, uint32_t isize, uint32_t want_crc, uint32_t nlanes, uint32_t* out_len, uint32_t* crc);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t)((g_rng >> 11) % n);
}

static std::string vcf_like(size_t n) {
  std::string s;
  uint32_t pos = 1000;
  char line[256];
  while (s.size() < n) {
    pos += 1 + rnd(300);
    snprintf(line, sizeof(line), "1\t%u\t.\t%c\t<NON_REF>\t.\t.\tEND=%u\tGT:DP:GQ:MIN_DP:PL\t0/0:%u:%u:%u:0,%u,%u\n", pos, "ACGT"[rnd(4)], pos + rnd(200), rnd(60), rnd(99), rnd(60),
             rnd(120), rnd(1800));
    s += line;
  }
  s.resize(n);
  return s;
}

static std::vector<uint8_t> deflate_raw(const std::string& data, int level, int strategy, size_t flush_at) {
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, 9, strategy) != Z_OK) abort();
  std::vector<uint8_t> out(deflateBound(&zs, (uLong)data.size()) + 64);
  zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
  zs.next_in = (Bytef*)data.data();
  if (flush_at && flush_at < data.size()) {
    zs.avail_in = (uInt)flush_at;
    if (deflate(&zs, Z_FULL_FLUSH) != Z_OK) abort();
    zs.avail_in = (uInt)(data.size() - flush_at);
  } else zs.avail_in = (uInt)data.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

int main() {
  struct Base { std::string data; std::vector<uint8_t> z; };
  std::vector<Base> bases;
  const struct { int level, strategy; size_t n, flush_at; } kinds[] = {{6, Z_DEFAULT_STRATEGY, 6000, 0}, {1, Z_DEFAULT_STRATEGY, 3000, 0}, {9, Z_FIXED, 800, 0},
                                                                       {0, Z_DEFAULT_STRATEGY, 500, 0}, {9, Z_DEFAULT_STRATEGY, 2500, 700}, {6, Z_DEFAULT_STRATEGY, 65536, 0}};
  for (const auto& k : kinds) { Base b; b.data = vcf_like(k.n); b.z = deflate_raw(b.data, k.level, k.strategy, k.flush_at); bases.push_back(b); }
  int ok = 0, errors = 0, by_code[16] = {0};
  const uint32_t lanes[3] = {64, 1, 7};
  for (int k = 0; k < 2000 + (int)bases.size(); ++k) {
    const Base& b = bases[(size_t)k % bases.size()];
    std::vector<uint8_t> s = b.z;
    uint32_t isize = (uint32_t)b.data.size();
    if (k >= (int)bases.size()) {          // (the first ones unchanged: they must inflate)
      const uint32_t at = (k % 3) ? rnd((uint32_t)s.size()) : rnd((uint32_t)std::min<size_t>(s.size(), 120));
      if (k % 2) s[at] ^= (uint8_t)(1u << rnd(8)); else s[at] = (uint8_t)(s[at] + 1 + rnd(255));
      if (k % 7 == 0) s.resize(rnd((uint32_t)s.size()));          // and truncated
      if (k % 11 == 0) isize = rnd(isize + 1);                    // and an ISIZE that is too small
    }
    const uint32_t want_crc = (uint32_t)crc32(0L, (const Bytef*)b.data.data(), (uInt)b.data.size());
    std::vector<uint8_t> out(isize ? isize : 1);
    uint32_t got = 0, crc = 0;
    const int err = hostsim_inflate_member(s.data(), (uint32_t)s.size(), out.data(), isize, want_crc, lanes[k % 3], &got, &crc);
    if (err < 0 || err > 10) { fprintf(stderr, "mutation %d: error code %d\n", k, err); return 1; }
    ++by_code[err];
    if (err == 0) {
      if (got != b.data.size() || isize != b.data.size() || memcmp(out.data(), b.data.data(), isize) != 0 || crc != want_crc) { fprintf(stderr, "mutation %d: accepted with other bytes\n", k); return 1; }
      ++ok;
    } else {
      if (k < (int)bases.size()) { fprintf(stderr, "valid member %d refused with %d\n", k, err); return 1; }
      ++errors;
    }
  }
  printf("inflate_fuzz: %d members: %d inflated to zlib's bytes, %d refused; by error code:", ok + errors, ok, errors);
  for (int i = 0; i <= 10; ++i) printf(" %d:%d", i, by_code[i]);
  printf("\n");
  return 0;
}
