// bgzf_host.cc - the host half of kernels/gdb_bgzf.h: BGZF blocks of a host buffer by zlib, and the EOF block.  Plain C++, so that the
// index writer (host/vcf_index.cc) and the CPU harnesses link it without the device code.
#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../kernels/gdb_bgzf.h"

namespace genomicsdb_amd {

const unsigned char kBgzfEofBlock[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

std::string bgzf_compress_host(const std::string& bytes) {
  std::string out;
  const size_t kHostBlock = 0xff00;                            // htslib's BGZF_BLOCK_SIZE
  for (size_t at = 0; at < bytes.size(); at += kHostBlock) {
    const size_t n = std::min<size_t>(kHostBlock, bytes.size() - at);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("BGZF: deflateInit2 failed");
    std::vector<unsigned char> buf(deflateBound(&zs, (uLong)n) + 16);
    zs.next_in = (Bytef*)bytes.data() + at; zs.avail_in = (uInt)n;
    zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
    const int rc = deflate(&zs, Z_FINISH);
    const size_t c = buf.size() - zs.avail_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) throw std::runtime_error("BGZF: deflate failed");
    const uint32_t bs = (uint32_t)(c + kBgzfHeaderBytes + kBgzfTrailerBytes - 1);
    if (bs > 0xFFFFu) throw std::runtime_error("BGZF: block too large");
    const unsigned char hdr[18] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, (unsigned char)(bs & 0xFFu), (unsigned char)(bs >> 8)};
    out.append((const char*)hdr, 18);
    out.append((const char*)buf.data(), c);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)bytes.data() + at, (uInt)n), isize = (uint32_t)n;
    out.append((const char*)&crc, 4);
    out.append((const char*)&isize, 4);
  }
  return out;
}

}  // namespace genomicsdb_amd
