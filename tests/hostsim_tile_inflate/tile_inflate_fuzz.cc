// tile_inflate_fuzz.cc - stand-alone driver of the tile inflater's body (core/gdb_tile_inflate.hpp, through hostsim_tile_inflate.cc),
// meant for a sanitizer build on the CPU (see the Makefile).  Every stream lies in a heap block of its exact size and the output
// slot has exactly 8192 bytes, so a read or write out of bounds is an error the sanitizer reports.  Two sources of streams:
//   - seeded mutations (bit flips, byte replacements, truncations) of tiles zlib wrote, always;
//   - a case file (argv[1]) written by tests/test_tile_inflate_bodies_cpu.py: the hand-made streams with the TileErr expected of each.
// Every result is compared with zlib's own inflate of the same bytes (Z_FINISH into exactly `want` bytes, as the host side of the
// fragment reader does): same verdict, same bytes when accepted, and the slot untouched behind `want`.  Test infrastructure only.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int hostsim_tile_inflate(const uint8_t* src, uint32_t n, uint32_t want, uint8_t fill, uint8_t* slot);

static const uint32_t kTile = 8192;
static const uint8_t kFill = 0xA5;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t)((g_rng >> 11) % n);
}

static std::string payload(int kind, size_t n) {
  std::string s;
  if (kind == 0) {                       // VCF-like text
    uint32_t pos = 1000;
    char line[256];
    while (s.size() < n) {
      pos += 1 + rnd(300);
      snprintf(line, sizeof(line), "1\t%u\t.\t%c\t<NON_REF>\t.\t.\tEND=%u\tGT:DP:GQ:MIN_DP:PL\t0/0:%u:%u:%u:0,%u,%u\n", pos, "ACGT"[rnd(4)], pos + rnd(200), rnd(60), rnd(99), rnd(60),
               rnd(120), rnd(1800));
      s += line;
    }
  } else if (kind == 1) { while (s.size() < n) s += (char)rnd(256); }                                   // random bytes
  else if (kind == 2) { while (s.size() < n) s += "ACGT"[rnd(4)]; }
  else if (kind == 3) { while (s.size() < n) s += std::string(1 + rnd(40), (char)('a' + rnd(3))); }     // runs
  else { while (s.size() < n) { uint32_t v = 0; while (v < 200 && rnd(2)) ++v; s += (char)v; } }        // a geometric alphabet
  s.resize(n);
  return s;
}

static std::vector<uint8_t> deflate_raw(const std::string& data, int level, int strategy, int mem_level, size_t flush_every, int flush) {
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) abort();
  std::vector<uint8_t> out(deflateBound(&zs, (uLong)data.size()) + 64 + (flush_every ? 16 * (data.size() / flush_every + 1) : 0));
  zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
  size_t at = 0;
  if (flush_every) for (; at + flush_every < data.size(); at += flush_every) {
    zs.next_in = (Bytef*)data.data() + at; zs.avail_in = (uInt)flush_every;
    if (deflate(&zs, flush) != Z_OK) abort();
  }
  zs.next_in = (Bytef*)data.data() + at; zs.avail_in = (uInt)(data.size() - at);
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

// zlib's answer: true and `out` (want bytes) when the stream ends as a stream of exactly `want` bytes
static bool zlib_inflate(const std::vector<uint8_t>& s, uint32_t want, std::vector<uint8_t>& out) {
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, -15) != Z_OK) abort();
  out.assign((size_t)want + 1, 0);
  static uint8_t none = 0;
  zs.next_in = s.empty() ? &none : const_cast<Bytef*>(s.data()); zs.avail_in = (uInt)s.size();
  zs.next_out = out.data(); zs.avail_out = want;
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
  inflateEnd(&zs);
  out.resize(want);
  return ok;
}

static int g_by_code[16];
// -> 0, or 1 after a message
static int check(const char* what, long k, const std::vector<uint8_t>& s, uint32_t want, int expect) {
  std::vector<uint8_t> slot(kTile), ref;
  const int err = hostsim_tile_inflate(s.data(), (uint32_t)s.size(), want, kFill, slot.data());
  if (err < 0 || err > 9) { fprintf(stderr, "%s %ld: error code %d\n", what, k, err); return 1; }
  ++g_by_code[err];
  const bool z_ok = zlib_inflate(s, want, ref);
  if (z_ok != (err == 0)) { fprintf(stderr, "%s %ld: zlib %s, the body says %d\n", what, k, z_ok ? "accepts" : "refuses", err); return 1; }
  if (expect >= 0 && err != expect) { fprintf(stderr, "%s %ld: TileErr %d, expected %d\n", what, k, err, expect); return 1; }
  if (err == 0 && want && memcmp(slot.data(), ref.data(), want) != 0) { fprintf(stderr, "%s %ld: accepted with other bytes than zlib's\n", what, k); return 1; }
  for (uint32_t i = want; i < kTile; ++i) if (slot[i] != kFill) { fprintf(stderr, "%s %ld: byte %u behind want = %u was written\n", what, k, i, want); return 1; }
  return 0;
}

static int run_case_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
  char magic[8];
  uint32_t count = 0;
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "TILECASE", 8) != 0 || fread(&count, 4, 1, f) != 1) { fprintf(stderr, "%s: not a case file\n", path); fclose(f); return 1; }
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t h[3];
    if (fread(h, 4, 3, f) != 3 || h[0] > (1u << 20) || h[1] > kTile) { fprintf(stderr, "%s: case %u is cut\n", path, k); fclose(f); return 1; }
    std::vector<uint8_t> s(h[0]);
    if (h[0] && fread(s.data(), 1, h[0], f) != h[0]) { fprintf(stderr, "%s: case %u is cut\n", path, k); fclose(f); return 1; }
    if (check("case", (long)k, s, h[1], (int)h[2])) { fclose(f); return 1; }
  }
  fclose(f);
  printf("tile_inflate_fuzz: %u cases of %s agree with zlib and with their expected TileErr\n", count, path);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && run_case_file(argv[1])) return 1;
  struct Base { std::string data; std::vector<uint8_t> z; };
  std::vector<Base> bases;
  const int flushes[4] = {Z_SYNC_FLUSH, Z_FULL_FLUSH, Z_PARTIAL_FLUSH, Z_BLOCK};
  const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
  const int levels[4] = {0, 1, 6, 9};
  for (int i = 0; i < 60; ++i) {
    Base b;
    const size_t n = i < 6 ? (size_t)i : i == 6 ? 8191 : i == 7 ? 8192 : 1 + rnd(8192);
    b.data = payload(i % 5, n);
    b.z = deflate_raw(b.data, levels[rnd(4)], strategies[rnd(5)], 1 + (int)rnd(9), rnd(3) ? 0 : 1 + rnd(3000), flushes[rnd(4)]);
    if (check("base", i, b.z, (uint32_t)n, 0)) return 1;
    if (check("base (want - 1)", i, b.z, (uint32_t)n - (n ? 1 : 0), n ? -1 : 0)) return 1;
    if (n < kTile && check("base (want + 1)", i, b.z, (uint32_t)n + 1, -1)) return 1;
    bases.push_back(b);
  }
  int accepted = 0, refused = 0;
  memset(g_by_code, 0, sizeof(g_by_code));
  for (int k = 0; k < 4000; ++k) {
    const Base& b = bases[(size_t)k % bases.size()];
    std::vector<uint8_t> s = b.z;
    const int kind = k % 5;
    if (kind == 4) s.resize(rnd((uint32_t)s.size() + 1));                                           // truncated
    else {
      const uint32_t at = (k % 3) ? rnd((uint32_t)s.size()) : rnd((uint32_t)(s.size() < 40 ? s.size() : 40));   // (a third of them in the block header)
      if (kind < 3) s[at] ^= (uint8_t)(1u << rnd(8)); else s[at] = (uint8_t)(s[at] + 1 + rnd(255));
    }
    const int before = g_by_code[0];
    if (check("mutation", k, s, (uint32_t)b.data.size(), -1)) return 1;
    if (g_by_code[0] != before) ++accepted; else ++refused;
  }
  printf("tile_inflate_fuzz: %d mutations of %d tiles: %d accepted as zlib accepts them, %d refused as zlib refuses them; by TileErr:", accepted + refused, (int)bases.size(), accepted, refused);
  for (int i = 0; i <= 9; ++i) printf(" %d:%d", i, g_by_code[i]);
  printf("\n");
  return 0;
}
