// gdb_inflate.hip - see gdb_inflate.h.  Kernels for gfx950 around the bodies of core/gdb_inflate.hpp.
//
// k_inflate_members         one wavefront (a workgroup of 64) per BGZF member.  Decode state and tables (InfState, ~10 KiB) and
//                           the member's whole output (<= 64 KiB) live in LDS: literals and match copies never leave the CU, a
//                           distance of 32 768 is an LDS read like any other, and the CRC32 is taken from LDS.  The output is
//                           placed in LDS at the destination's own alignment mod 16 and flushed once, with 16-byte stores on
//                           consecutive lanes.  ~76 KiB per workgroup is more than the 64 KiB a kernel gets by default, so the
//                           launch asks for it as dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize); two workgroups fit
//                           in the 160 KiB of a CU.  That is 2 wavefronts per CU, chosen knowingly: the serial decode on lane 0
//                           is a chain of dependent LDS look-ups that more resident waves would hide better, but a window that
//                           keeps only the last 32 KiB in LDS would gain one more wave at best (3 x 44 KiB) for a second copy
//                           path, and a decoder that writes to HBM pays an HBM round trip per match.  A file has thousands of
//                           members, so the grid itself is never short of work.
// k_inflate_members_thread  the A/B partner: one THREAD per member runs the same bodies (InfLoopExec with one lane), state in a
//                           per-thread block of global memory, output written straight to HBM - the shape of k_inflate_tiles.
//                           Measured 9.6 x slower on bgzip-sized members (profiles/device_inflate.md); it stays for that
//                           comparison only, behind set_kernel.
#include "gdb_inflate.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../core/gdb_inflate.hpp"
#include "gdb_pipeline.h"

namespace genomicsdb_amd {

#define INF_HIP_CHECK(expr)                                                                                        \
  do {                                                                                                             \
    hipError_t _e = (expr);                                                                                        \
    if (_e != hipSuccess)                                                                                          \
      throw GenomicsDBDeviceException(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

namespace {
using namespace gdbinf;

constexpr uint32_t kWave = 64;
constexpr uint32_t kStateBytes = (uint32_t)((sizeof(InfState) + 15u) & ~(size_t)15u);
constexpr uint32_t kLdsBytes = kStateBytes + kMaxOut + 16u;          // state, output, up to 15 bytes of alignment in front of the output
static_assert(2u * kLdsBytes <= 160u * 1024u, "two members per CU");
constexpr uint32_t kBadDescriptor = 0xFFu;

struct InfDesc { uint32_t src_off, src_len, isize, crc; uint64_t out_off; };     // src_off: in the uploaded range; out_off: in dst

// a phase on every lane of the wavefront, then the barrier that makes its LDS writes visible to the next phase
struct InfWaveExec {
  uint32_t lane;
  template <class F> __device__ __forceinline__ void operator()(F f) const { f(lane, kWave); __syncthreads(); }
};

__device__ __forceinline__ bool inf_desc_ok(const InfDesc& d, uint64_t src_bytes, uint64_t dst_bytes) {
  return (uint64_t)d.src_off + d.src_len <= src_bytes && d.isize <= kMaxOut && d.out_off <= dst_bytes && (uint64_t)d.isize <= dst_bytes - d.out_off;
}

__global__ void __launch_bounds__(kWave) k_inflate_members(const uint8_t* src, uint64_t src_bytes, const InfDesc* desc, uint32_t n, uint8_t* dst, uint64_t dst_bytes,
                                                          uint32_t* status) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_inf[];
  const uint32_t m = blockIdx.x, lane = threadIdx.x;
  if (m >= n) return;
  const InfDesc d = desc[m];
  if (!inf_desc_ok(d, src_bytes, dst_bytes)) {      // (never, by the host's walk: nothing is read or written outside the buffers)
    if (lane == 0) status[m] = kBadDescriptor;
    return;
  }
  InfState& S = *reinterpret_cast<InfState*>(s_inf);
  uint8_t* g = dst + d.out_off;
  const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u);
  uint8_t* out = s_inf + kStateBytes + pad;
  const uint32_t err = inf_member(InfWaveExec{lane}, S, src + d.src_off, d.src_len, out, d.isize, d.crc);
  if (lane == 0) status[m] = err;
  if (err) return;                                  // (uniform) a refused member writes nothing
  // flush: bytes up to the first 16-byte boundary of the destination, aligned 16-byte stores, bytes behind the last boundary
  const uint32_t head = std::min<uint32_t>(d.isize, (16u - pad) & 15u);
  const uint32_t nvec = (d.isize - head) >> 4, tail = head + (nvec << 4);
  for (uint32_t i = lane; i < head; i += kWave) g[i] = out[i];
  for (uint32_t v = lane; v < nvec; v += kWave) *reinterpret_cast<uint4*>(g + head + (v << 4)) = *reinterpret_cast<const uint4*>(out + head + (v << 4));
  for (uint32_t i = tail + lane; i < d.isize; i += kWave) g[i] = out[i];
}

__global__ void __launch_bounds__(kWave) k_inflate_members_thread(const uint8_t* src, uint64_t src_bytes, const InfDesc* desc, uint32_t n, uint8_t* dst, uint64_t dst_bytes,
                                                                 uint32_t* status, InfState* scratch) {
  const uint32_t m = blockIdx.x * kWave + threadIdx.x;
  if (m >= n) return;
  const InfDesc d = desc[m];
  if (!inf_desc_ok(d, src_bytes, dst_bytes)) { status[m] = kBadDescriptor; return; }
  status[m] = inf_member(InfLoopExec{1u}, scratch[m], src + d.src_off, d.src_len, dst + d.out_off, d.isize, d.crc);
}

template <class T> struct DBuf {       // grow-only device block
  T* p = nullptr; size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    INF_HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
    cap = n;
  }
  ~DBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

const char* bgzf_inflate_error_text(uint32_t err) {
  switch (err) {
    case INF_OK: return "no error";
    case INF_ERR_BLOCK_TYPE: return "reserved DEFLATE block type";
    case INF_ERR_CODE: return "invalid Huffman code lengths";
    case INF_ERR_NO_EOB: return "no end-of-block code";
    case INF_ERR_SYMBOL: return "invalid length or distance symbol";
    case INF_ERR_DISTANCE: return "distance reaches before the start of the member";
    case INF_ERR_OUTPUT: return "more data than ISIZE";
    case INF_ERR_INPUT: return "compressed data ends early";
    case INF_ERR_STORED_LEN: return "stored block with LEN / NLEN mismatch";
    case INF_ERR_ISIZE: return "less data than ISIZE";
    case INF_ERR_CRC: return "CRC32 mismatch";
    default: return "bad member descriptor";
  }
}

struct BgzfDeviceInflater::Impl {
  Kernel kernel = kWavePerMember;
  bool lds_asked = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  DBuf<uint8_t> d_src;
  DBuf<InfDesc> d_desc;
  DBuf<uint32_t> d_status;
  DBuf<InfState> d_scratch;
  std::vector<InfDesc> desc;
  std::vector<uint32_t> status;
};

BgzfDeviceInflater::BgzfDeviceInflater() : m_(new Impl) {}
BgzfDeviceInflater::~BgzfDeviceInflater() {
  for (auto& e : m_->ev) if (e) (void)hipEventDestroy(e);
  delete m_;
}
void BgzfDeviceInflater::set_kernel(Kernel k) { m_->kernel = k; }

int64_t BgzfDeviceInflater::inflate(const uint8_t* host_src, const BgzfMember* members, size_t m0, size_t m1, uint8_t* dev_dst, void* stream_, uint32_t* err) {
  Impl& M = *m_;
  if (m1 <= m0) return -1;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = m1 - m0;
  if (n >= ((size_t)1 << 31)) throw GenomicsDBDeviceException("too many BGZF members in one call");
  const BgzfMember& first = members[m0];
  const BgzfMember& last = members[m1 - 1];
  const uint64_t lo = first.offset, hi = last.offset + last.data_off + last.data_len + 8u, src_bytes = hi - lo;
  const uint64_t dst_bytes = last.out_off + last.isize - first.out_off;
  if (src_bytes >= ((uint64_t)1 << 32)) throw GenomicsDBDeviceException("more than 4 GiB of BGZF members in one call");
  M.desc.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const BgzfMember& b = members[m0 + i];
    M.desc[i] = InfDesc{(uint32_t)(b.offset - lo) + b.data_off, b.data_len, b.isize, b.crc, b.out_off - first.out_off};
  }
  for (auto& e : M.ev) if (!e) INF_HIP_CHECK(hipEventCreate(&e));
  M.d_src.ensure(src_bytes + 16);
  M.d_desc.ensure(n);
  M.d_status.ensure(n);
  INF_HIP_CHECK(hipEventRecord(M.ev[2], stream));
  INF_HIP_CHECK(hipMemcpyAsync(M.d_src.p, host_src + lo, src_bytes, hipMemcpyHostToDevice, stream));
  INF_HIP_CHECK(hipMemcpyAsync(M.d_desc.p, M.desc.data(), n * sizeof(InfDesc), hipMemcpyHostToDevice, stream));
  INF_HIP_CHECK(hipMemsetAsync(M.d_status.p, 0xFF, n * sizeof(uint32_t), stream));
  bytes_h2d += src_bytes + n * sizeof(InfDesc);
  INF_HIP_CHECK(hipEventRecord(M.ev[0], stream));
  if (M.kernel == kWavePerMember) {
    if (!M.lds_asked) {
      INF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_inflate_members), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
      M.lds_asked = true;
    }
    hipLaunchKernelGGL(k_inflate_members, dim3((unsigned)n), dim3(kWave), kLdsBytes, stream, (const uint8_t*)M.d_src.p, src_bytes, (const InfDesc*)M.d_desc.p, (uint32_t)n,
                       dev_dst, dst_bytes, M.d_status.p);
  } else {
    M.d_scratch.ensure(n);
    hipLaunchKernelGGL(k_inflate_members_thread, dim3((unsigned)((n + kWave - 1) / kWave)), dim3(kWave), 0, stream, (const uint8_t*)M.d_src.p, src_bytes,
                       (const InfDesc*)M.d_desc.p, (uint32_t)n, dev_dst, dst_bytes, M.d_status.p, M.d_scratch.p);
  }
  INF_HIP_CHECK(hipGetLastError());
  INF_HIP_CHECK(hipEventRecord(M.ev[1], stream));
  M.status.resize(n);
  INF_HIP_CHECK(hipMemcpyAsync(M.status.data(), M.d_status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  INF_HIP_CHECK(hipStreamSynchronize(stream));
  float ms = 0;
  INF_HIP_CHECK(hipEventElapsedTime(&ms, M.ev[0], M.ev[1]));
  ms_kernel += ms;
  INF_HIP_CHECK(hipEventElapsedTime(&ms, M.ev[2], M.ev[0]));
  ms_upload += ms;
  for (size_t i = 0; i < n; ++i) if (M.status[i] != INF_OK) { if (err) *err = M.status[i]; return (int64_t)(m0 + i); }
  return -1;
}

}  // namespace genomicsdb_amd
