// rayfed_amd HIP extension — MI355X (gfx950) data-plane kernels.
//
// Replaces the reference's CPU cloudpickle payload path
// (/root/reference/fed/proxy/grpc/grpc_proxy.py:202) with device-side
// pack/CRC and aggregation:
//
//   * crc32       — zlib-compatible CRC32 of a device byte buffer, fully
//                   parallel: per-thread slice CRCs (slice-by-8, tables in
//                   LDS) + GF(2) shift-matrix combine in-kernel, finalized
//                   by a 1-thread kernel.  Exact for any length.
//   * pack_crc    — fused flatten-copy + CRC32 (one HBM read pass) into the
//                   device staging buffer that hipMemcpyAsync then DMAs to
//                   pinned host memory.
//   * pack_fp8 /  — wire compression: bf16/f32 -> OCP fp8 e4m3 cast fused
//     unpack_fp8    with CRC (half the bytes on the wire), and the inverse.
//   * fedavg_reduce_ / masked_add_ — weighted gradient aggregation for
//     intra-party FedAvg (bf16/f16/f32, fp32 accumulation, vectorized
//     16-byte loads per lane — CDNA4 guide Appendix B: element-wise ops are
//     HBM-bound, always vectorize).
//   * secagg_mask / secagg_aggregate — secure aggregation in Z/2^32 with
//     in-register ChaCha20 pairwise masks (secagg_kernels.h).
//   * secagg_mask_noise / sumsq — differential privacy on top of it: L2
//     norm for clipping and binomial noise generated inside the mask pass.
//
// Wavefront size is 64 on CDNA4 (not 32); reductions below use width-64
// shuffles.  Compiled for gfx950 only — no CUDA shims, no multi-arch.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_fp8.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "crc32_math.h"

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));    \
  } while (0)

namespace {

constexpr int kWave = 64;              // CDNA4 wavefront
constexpr int kBlock = 256;            // threads per workgroup
constexpr uint32_t kSubLen = 4096;     // bytes CRC'd per thread (uniform)
constexpr int kMaxPow = 24;            // M_sub^(2^j), j < kMaxPow

// ---------------------------------------------------------------------------
// device-side GF(2) apply
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t* m, uint32_t v) {
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    s ^= (m[i] & (0u - ((v >> i) & 1u)));
  }
  return s;
}

// slice-by-8 step over 8 bytes (init-0 linear CRC), tables in LDS.
__device__ __forceinline__ uint32_t crc_step8(const uint32_t* t, uint32_t crc,
                                              uint32_t lo, uint32_t hi) {
  lo ^= crc;
  return t[7 * 256 + (lo & 0xFFu)] ^ t[6 * 256 + ((lo >> 8) & 0xFFu)] ^
         t[5 * 256 + ((lo >> 16) & 0xFFu)] ^ t[4 * 256 + (lo >> 24)] ^
         t[3 * 256 + (hi & 0xFFu)] ^ t[2 * 256 + ((hi >> 8) & 0xFFu)] ^
         t[1 * 256 + ((hi >> 16) & 0xFFu)] ^ t[0 * 256 + (hi >> 24)];
}

struct CrcShared {
  uint32_t tables[8 * 256];
  uint32_t pows[kMaxPow * 32];
  uint32_t halfmat[32];  // shift matrix for kSubLen/2 zero bytes
};

__device__ __forceinline__ void load_crc_shared(CrcShared& sh,
                                                const uint32_t* g_tables,
                                                const uint32_t* g_pows,
                                                const uint32_t* g_halfmat) {
  for (int i = threadIdx.x; i < 8 * 256; i += blockDim.x)
    sh.tables[i] = g_tables[i];
  for (int i = threadIdx.x; i < kMaxPow * 32; i += blockDim.x)
    sh.pows[i] = g_pows[i];
  if (threadIdx.x < 32) sh.halfmat[threadIdx.x] = g_halfmat[threadIdx.x];
  __syncthreads();
}

// xor-reduce `v` (a 32- or 64-bit word) across the block, atomically xor
// into *out from one lane.
template <typename W>
__device__ __forceinline__ void block_xor_out(W v, W* out, W* lds_scratch) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v ^= __shfl_down(v, off, kWave);
  const int wid = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) lds_scratch[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    W acc = 0;
    for (int w = 0; w < (int)(blockDim.x / kWave); ++w) acc ^= lds_scratch[w];
    if (acc) atomicXor(out, acc);
  }
}

// `crc` shifted past k whole slices (binary powers of the slice matrix).
__device__ __forceinline__ uint32_t crc_shift_slices(const CrcShared& sh,
                                                     uint32_t crc,
                                                     uint32_t k) {
  int j = 0;
  while (k) {
    if (k & 1u) crc = gf2_apply(&sh.pows[j * 32], crc);
    k >>= 1;
    ++j;
  }
  return crc;
}

// The two block reductions that end a CRC kernel: out[0] ^= the full-slice
// terms, out[1] ^= the tail term.
__device__ __forceinline__ void crc_block_out(uint32_t contrib_full,
                                              uint32_t contrib_tail,
                                              uint32_t* out,
                                              uint32_t* lds_scratch) {
  block_xor_out(contrib_full, &out[0], lds_scratch);
  __syncthreads();
  block_xor_out(contrib_tail, &out[1], lds_scratch);
}

// ---------------------------------------------------------------------------
// CRC32 kernel (optionally fused with a flatten copy src->dst)
//
// Thread t < T-1 CRCs bytes [t*kSubLen, (t+1)*kSubLen); the last thread takes
// the tail.  Full threads apply M_sub^(T-2-t) on-device (binary powers in
// LDS); the shared tail shift + init/final constant are applied by
// crc_finalize_kernel.  out[0] = xor of full-thread terms, out[1] = L(tail).
// ---------------------------------------------------------------------------
template <bool kPack>
__global__ void crc32_kernel(const uint8_t* __restrict__ data,
                             uint8_t* __restrict__ dst,
                             unsigned long long n, uint32_t T,
                             const uint32_t* __restrict__ g_tables,
                             const uint32_t* __restrict__ g_pows,
                             const uint32_t* __restrict__ g_halfmat,
                             uint32_t* __restrict__ out) {
  __shared__ CrcShared sh;
  __shared__ uint32_t lds_scratch[kBlock / kWave];
  load_crc_shared(sh, g_tables, g_pows, g_halfmat);

  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t contrib_full = 0, contrib_tail = 0;
  if (t < T) {
    const unsigned long long off = (unsigned long long)t * kSubLen;
    const uint32_t len = (t == T - 1) ? (uint32_t)(n - off) : kSubLen;
    uint32_t crc = 0;
    const uint8_t* p = data + off;
    uint8_t* q = kPack ? dst + off : nullptr;
    uint32_t i = 0;
    if ((((uintptr_t)p) & 15u) == 0 && len == kSubLen) {
      // Full slice: TWO independent CRC streams (halves of the slice) to
      // break the serial table-lookup dependency chain — the kernel is
      // latency-bound otherwise (PMC: 85 % SQ_WAIT).  Streams combine with
      // the half-length shift matrix at the end.
      constexpr uint32_t H = kSubLen / 2;
      uint32_t crc_b = 0;
      for (; i + 16 <= H; i += 16) {
        const uint4 va = *reinterpret_cast<const uint4*>(p + i);
        const uint4 vb = *reinterpret_cast<const uint4*>(p + H + i);
        if (kPack) {
          *reinterpret_cast<uint4*>(q + i) = va;
          *reinterpret_cast<uint4*>(q + H + i) = vb;
        }
        crc = crc_step8(sh.tables, crc, va.x, va.y);
        crc_b = crc_step8(sh.tables, crc_b, vb.x, vb.y);
        crc = crc_step8(sh.tables, crc, va.z, va.w);
        crc_b = crc_step8(sh.tables, crc_b, vb.z, vb.w);
      }
      crc = gf2_apply(sh.halfmat, crc) ^ crc_b;
      i = kSubLen;
    } else if ((((uintptr_t)p) & 15u) == 0) {
      for (; i + 16 <= len; i += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + i);
        if (kPack) *reinterpret_cast<uint4*>(q + i) = v;
        crc = crc_step8(sh.tables, crc, v.x, v.y);
        crc = crc_step8(sh.tables, crc, v.z, v.w);
      }
    }
    for (; i < len; ++i) {
      const uint8_t b = p[i];
      if (kPack) q[i] = b;
      crc = (crc >> 8) ^ sh.tables[(crc ^ b) & 0xFFu];
    }
    if (t == T - 1) {
      contrib_tail = crc;
    } else {
      contrib_full = crc_shift_slices(sh, crc, T - 2 - t);
    }
  }
  crc_block_out(contrib_full, contrib_tail, out, lds_scratch);
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) {
  union {
    uint32_t u;
    float f;
  } c;
  c.u = (uint32_t)h << 16;
  return c.f;
}

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  // Round to nearest even with the hardware convert (v_cvt_pk_bf16_f32):
  // one instruction, and NaN stays NaN.  The integer form
  // (u + 0x7FFF + lsb) >> 16 carries a high-mantissa NaN such as 0x7FFFFFFF
  // over into the sign bit (-> -0).
  const __bf16 h = (__bf16)f;
  uint16_t r;
  __builtin_memcpy(&r, &h, sizeof(r));
  return r;
}

// ---------------------------------------------------------------------------
// hash64 — memory-rate 64-bit integrity hash for the device-IPC lane.
//
// The CRC32 kernel above is LDS-lookup bound (~1.2 TB/s measured); on the
// same-node IPC lane the checksum pass is the round bottleneck (kernel
// trace r01: CRC 289.7 ms vs reduce 33.5 ms per fedavg soak).  This hash
// is FNV-1a over fixed SLOTS (=4*kHashLanes) interleaved word streams with
// a murmur-style finalizer per lane — pure streaming reads + 2 VALU ops
// per word, so it runs at HBM rate.  The slot mapping is a function of
// nbytes ONLY (fixed lane count, grid-strided), so sender and receiver
// agree for any launch, and tests pin it against a numpy reference
// (rayfed_amd/ops/hash_ref.py).  Error-detection only — NOT crypto.
// ---------------------------------------------------------------------------
constexpr uint32_t kHashLanes = 524288;  // fixed: 2048 blocks x 256 threads
// (8 waves/CU — 4 was latency-limited; the mapping constant is mirrored in
// rayfed_amd/ops/hash_ref.py and must change in lockstep)
constexpr unsigned long long kFnvOff = 0xcbf29ce484222325ull;
constexpr unsigned long long kFnvP = 0x100000001b3ull;

__device__ __forceinline__ unsigned long long fmix64(unsigned long long h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// The pieces every hash64-mapped kernel shares: the four lane accumulators'
// start values, their fold into the lane's term, and lane 0's terms for the
// tail word and the length.
__device__ __forceinline__ void hash64_init(unsigned long long h[4],
                                            uint32_t lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    h[k] = (kFnvOff ^ (unsigned long long)(lane * 4u + k)) * kFnvP;
}

__device__ __forceinline__ unsigned long long hash64_fold(
    const unsigned long long h[4]) {
  return fmix64(
      ((((h[0] * kFnvP ^ h[1]) * kFnvP ^ h[2]) * kFnvP ^ h[3]) * kFnvP));
}

__device__ __forceinline__ unsigned long long hash64_tail_term(
    unsigned long long tw) {
  return fmix64((kFnvOff ^ tw) * kFnvP);
}

__device__ __forceinline__ unsigned long long hash64_len_term(
    unsigned long long nbytes) {
  return fmix64((nbytes * kFnvP) ^ kFnvOff);
}

template <bool kPack>
__global__ void hash64_kernel(const unsigned long long* __restrict__ words,
                              unsigned long long* __restrict__ dst,
                              unsigned long long n_words,
                              const uint8_t* __restrict__ tail,
                              uint8_t* __restrict__ dst_tail,
                              uint32_t tail_len,
                              unsigned long long nbytes,
                              unsigned long long* __restrict__ out) {
  __shared__ unsigned long long lds[kBlock / kWave];
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;  // < kHashLanes
  const unsigned long long slots = 4ull * kHashLanes;
  unsigned long long h[4];
  hash64_init(h, lane);
  // Iteration j: lane reads words j*slots + lane*4 + k — consecutive lanes
  // read consecutive 32-byte chunks (fully coalesced); 4 independent
  // accumulators hide the multiply latency.  kPack fuses the staging copy
  // into the same read pass (one HBM read instead of copy ∥ hash reading
  // the source twice).
  for (unsigned long long base = (unsigned long long)lane * 4ull;
       base < n_words; base += slots) {
    if (base + 4 <= n_words) {
      unsigned long long w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = words[base + k];
        h[k] = (h[k] ^ w[k]) * kFnvP;
      }
      if (kPack) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[base + k] = w[k];
      }
    } else {
      for (unsigned long long i = base; i < n_words; ++i) {
        const unsigned long long w = words[i];
        h[i - base] = (h[i - base] ^ w) * kFnvP;
        if (kPack) dst[i] = w;
      }
    }
  }
  unsigned long long v = hash64_fold(h);
  if (lane == 0) {
    if (tail_len) {
      unsigned long long tw = 0;
      for (uint32_t i = 0; i < tail_len; ++i) {
        tw |= (unsigned long long)tail[i] << (8 * i);
        if (kPack) dst_tail[i] = tail[i];
      }
      v ^= hash64_tail_term(tw);
    }
    v ^= hash64_len_term(nbytes);
  }
  block_xor_out(v, out, lds);
}

// ---------------------------------------------------------------------------
// Fused FedAvg combine + integrity hash (zero-copy receive path).
//
// out[i] = fma(wa, local[i], wb*peer[i]) (bf16, fp32 math; written as an
// explicit fmaf so the rounding does not hang on the compiler's contraction
// choice) while computing the
// hash64 of the PEER bytes in the same pass — the receiver combines
// directly from the sender's IPC slab, never materializing a copy and
// never re-reading it for the verify.  The thread/word mapping is
// IDENTICAL to hash64_kernel (fixed kHashLanes slots), so the sender's
// per-slab hash values verify unchanged.
// ---------------------------------------------------------------------------
__global__ void fedavg_combine_hash_kernel(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ local,
    const unsigned long long* __restrict__ peer_words,
    unsigned long long n_words, const uint8_t* __restrict__ peer_tail,
    uint32_t tail_len, unsigned long long nbytes, float wa, float wb,
    unsigned long long* __restrict__ hash_out) {
  __shared__ unsigned long long lds[kBlock / kWave];
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long slots = 4ull * kHashLanes;
  const unsigned long long* lw =
      reinterpret_cast<const unsigned long long*>(local);
  unsigned long long h[4];
  hash64_init(h, lane);
  for (unsigned long long base = (unsigned long long)lane * 4ull;
       base < n_words; base += slots) {
    if (base + 4 <= n_words) {
      unsigned long long pw[4], ow[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pw[k] = peer_words[base + k];
        h[k] = (h[k] ^ pw[k]) * kFnvP;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long lv = lw[base + k];
        unsigned long long o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = bf16_to_f32((uint16_t)(pw[k] >> (16 * e)));
          const float l = bf16_to_f32((uint16_t)(lv >> (16 * e)));
          o |= (unsigned long long)f32_to_bf16(fmaf(wa, l, wb * p)) << (16 * e);
        }
        ow[k] = o;
      }
      unsigned long long* outw = reinterpret_cast<unsigned long long*>(out);
#pragma unroll
      for (int k = 0; k < 4; ++k) outw[base + k] = ow[k];
    } else {
      for (unsigned long long i = base; i < n_words; ++i) {
        const unsigned long long pw = peer_words[i];
        const unsigned long long lv = lw[i];
        h[i - base] = (h[i - base] ^ pw) * kFnvP;
        unsigned long long o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = bf16_to_f32((uint16_t)(pw >> (16 * e)));
          const float l = bf16_to_f32((uint16_t)(lv >> (16 * e)));
          o |= (unsigned long long)f32_to_bf16(fmaf(wa, l, wb * p)) << (16 * e);
        }
        reinterpret_cast<unsigned long long*>(out)[i] = o;
      }
    }
  }
  unsigned long long v = hash64_fold(h);
  if (lane == 0) {
    if (tail_len) {
      unsigned long long tw = 0;
      for (uint32_t i = 0; i < tail_len; ++i)
        tw |= (unsigned long long)peer_tail[i] << (8 * i);
      v ^= hash64_tail_term(tw);
      // Combine the tail elements too (bf16 => tail_len is even).
      const unsigned long long e0 = n_words * 4;
      for (uint32_t e = 0; e < tail_len / 2; ++e) {
        const float p = bf16_to_f32(
            (uint16_t)(peer_tail[2 * e] | (peer_tail[2 * e + 1] << 8)));
        const float l = bf16_to_f32(local[e0 + e]);
        out[e0 + e] = f32_to_bf16(fmaf(wa, l, wb * p));
      }
    }
    v ^= hash64_len_term(nbytes);
  }
  block_xor_out(v, hash_out, lds);
}

struct TailParam {
  uint32_t m[32];       // shift matrix for the tail length
  uint32_t final_xor;   // shift_len(0xFFFFFFFF) ^ 0xFFFFFFFF
};

__global__ void crc_finalize_kernel(uint32_t* out, TailParam p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) s ^= (p.m[i] & (0u - ((out[0] >> i) & 1u)));
    out[2] = s ^ out[1] ^ p.final_xor;
  }
}

// ---------------------------------------------------------------------------
// fp8 wire cast (OCP e4m3), fused with CRC over the produced bytes
// ---------------------------------------------------------------------------
// Wire contract (CPU reference: rayfed_amd/ops/fp8_ref.py): round to nearest
// even, finite |x| > 448 saturates to 0x7E/0xFE, +-Inf and NaN become the NaN
// byte sign|0x7F.  The non-finite case is decided here, not by the hardware
// convert: on gfx950 that maps +-Inf to 0x7F/0xFF but every NaN to 0xFF.
__device__ __forceinline__ uint8_t f32_to_fp8(float f) {
  const uint32_t u = __float_as_uint(f);
  __hip_fp8_e4m3 v(f);
  // (u >> 24) | 0x7F == sign | 0x7F; a select, not a branch.
  return ((u & 0x7F800000u) == 0x7F800000u) ? (uint8_t)((u >> 24) | 0x7Fu)
                                             : (uint8_t)v.__x;
}

__device__ __forceinline__ float fp8_to_f32(uint8_t b) {
  __hip_fp8_e4m3 v;
  v.__x = b;
  return (float)v;
}

// 8 fp8 bytes (one u64 word) -> 8 bf16 in element order (one 16-byte store).
__device__ __forceinline__ uint4 bf16x8_from_fp8x8(unsigned long long w) {
  uint32_t parts[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    parts[e] =
        (uint32_t)f32_to_bf16(fp8_to_f32((uint8_t)(w >> (16 * e)))) |
        ((uint32_t)f32_to_bf16(fp8_to_f32((uint8_t)(w >> (16 * e + 8))))
         << 16);
  }
  return make_uint4(parts[0], parts[1], parts[2], parts[3]);
}

// src: bf16 elements; dst: fp8 bytes.  Thread t produces kSubLen output
// bytes (= kSubLen input bf16 elements); same combine scheme as crc32_kernel.
// kVec: src is 16-byte and dst 8-byte aligned (decided on the host; slice
// offsets are multiples of kSubLen so one answer holds for every thread).
// Otherwise every element takes the scalar loop.
template <bool kVec>
__global__ void pack_fp8_kernel(const uint16_t* __restrict__ src,
                                uint8_t* __restrict__ dst,
                                unsigned long long n_elems, uint32_t T,
                                const uint32_t* __restrict__ g_tables,
                                const uint32_t* __restrict__ g_pows,
                                const uint32_t* __restrict__ g_halfmat,
                                uint32_t* __restrict__ out) {
  __shared__ CrcShared sh;
  __shared__ uint32_t lds_scratch[kBlock / kWave];
  load_crc_shared(sh, g_tables, g_pows, g_halfmat);

  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t contrib_full = 0, contrib_tail = 0;
  if (t < T) {
    const unsigned long long off = (unsigned long long)t * kSubLen;
    const uint32_t len =
        (t == T - 1) ? (uint32_t)(n_elems - off) : kSubLen;  // elements
    uint32_t crc = 0;
    const uint16_t* p = src + off;
    uint8_t* q = dst + off;
    uint32_t i = 0;
    for (; kVec && i + 8 <= len; i += 8) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + i);  // 8 bf16
      uint32_t lo = 0, hi = 0;
      lo |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.x & 0xFFFFu)));
      lo |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.x >> 16))) << 8;
      lo |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.y & 0xFFFFu))) << 16;
      lo |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.y >> 16))) << 24;
      hi |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.z & 0xFFFFu)));
      hi |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.z >> 16))) << 8;
      hi |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.w & 0xFFFFu))) << 16;
      hi |= (uint32_t)f32_to_fp8(bf16_to_f32((uint16_t)(v.w >> 16))) << 24;
      *reinterpret_cast<uint2*>(q + i) = make_uint2(lo, hi);
      crc = crc_step8(sh.tables, crc, lo, hi);
    }
    for (; i < len; ++i) {
      const uint8_t b = f32_to_fp8(bf16_to_f32(p[i]));
      q[i] = b;
      crc = (crc >> 8) ^ sh.tables[(crc ^ b) & 0xFFu];
    }
    if (t == T - 1) {
      contrib_tail = crc;
    } else {
      contrib_full = crc_shift_slices(sh, crc, T - 2 - t);
    }
  }
  crc_block_out(contrib_full, contrib_tail, out, lds_scratch);
}

// fp8 wire cast fused with the hash64 slot mapping over the PRODUCED fp8
// bytes (the LDS-table CRC in pack_fp8_kernel is the bottleneck otherwise).
// Output word k packs 8 fp8 from 8 bf16 (two input u64 words).
__global__ void pack_fp8_hash64_kernel(const uint16_t* __restrict__ src,
                                       unsigned long long* __restrict__ dst,
                                       unsigned long long n_words,  // output
                                       uint32_t tail_elems,
                                       unsigned long long nbytes,   // output
                                       unsigned long long* __restrict__ out) {
  __shared__ unsigned long long lds[kBlock / kWave];
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long slots = 4ull * kHashLanes;
  unsigned long long h[4];
  hash64_init(h, lane);
  for (unsigned long long base = (unsigned long long)lane * 4ull;
       base < n_words; base += slots) {
    const int cnt = (int)((base + 4 <= n_words) ? 4 : (n_words - base));
    for (int k = 0; k < cnt; ++k) {
      const unsigned long long i = base + k;
      const uint4 v = *reinterpret_cast<const uint4*>(src + i * 8);  // 8 bf16
      unsigned long long w = 0;
      const uint32_t parts[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w |= (unsigned long long)f32_to_fp8(
                 bf16_to_f32((uint16_t)(parts[e] & 0xFFFFu)))
             << (16 * e);
        w |= (unsigned long long)f32_to_fp8(
                 bf16_to_f32((uint16_t)(parts[e] >> 16)))
             << (16 * e + 8);
      }
      h[k] = (h[k] ^ w) * kFnvP;
      dst[i] = w;
    }
  }
  unsigned long long v = hash64_fold(h);
  if (lane == 0) {
    if (tail_elems) {
      unsigned long long tw = 0;
      uint8_t* dtail = reinterpret_cast<uint8_t*>(dst + n_words);
      for (uint32_t e = 0; e < tail_elems; ++e) {
        const uint8_t b = f32_to_fp8(bf16_to_f32(src[n_words * 8 + e]));
        dtail[e] = b;
        tw |= (unsigned long long)b << (8 * e);
      }
      v ^= hash64_tail_term(tw);
    }
    v ^= hash64_len_term(nbytes);
  }
  block_xor_out(v, out, lds);
}

// Inverse: fp8 -> bf16 expand fused with the hash64 of the INPUT fp8 bytes
// (receiver-side verify without a second read).
__global__ void unpack_fp8_hash64_kernel(
    const unsigned long long* __restrict__ src, uint16_t* __restrict__ dst,
    unsigned long long n_words,  // input u64 words
    uint32_t tail_elems, unsigned long long nbytes,
    unsigned long long* __restrict__ out) {
  __shared__ unsigned long long lds[kBlock / kWave];
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long slots = 4ull * kHashLanes;
  unsigned long long h[4];
  hash64_init(h, lane);
  for (unsigned long long base = (unsigned long long)lane * 4ull;
       base < n_words; base += slots) {
    const int cnt = (int)((base + 4 <= n_words) ? 4 : (n_words - base));
    for (int k = 0; k < cnt; ++k) {
      const unsigned long long i = base + k;
      const unsigned long long w = src[i];
      h[k] = (h[k] ^ w) * kFnvP;
      *reinterpret_cast<uint4*>(dst + i * 8) = bf16x8_from_fp8x8(w);
    }
  }
  unsigned long long v = hash64_fold(h);
  if (lane == 0) {
    if (tail_elems) {
      unsigned long long tw = 0;
      const uint8_t* stail = reinterpret_cast<const uint8_t*>(src + n_words);
      for (uint32_t e = 0; e < tail_elems; ++e) {
        tw |= (unsigned long long)stail[e] << (8 * e);
        dst[n_words * 8 + e] = f32_to_bf16(fp8_to_f32(stail[e]));
      }
      v ^= hash64_tail_term(tw);
    }
    v ^= hash64_len_term(nbytes);
  }
  block_xor_out(v, out, lds);
}

// kVec: src is 8-byte and dst 16-byte aligned (decided on the host).
template <bool kVec>
__global__ void unpack_fp8_kernel(const uint8_t* __restrict__ src,
                                  uint16_t* __restrict__ dst,
                                  unsigned long long n_elems) {
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x * 8ull;
  for (unsigned long long base =
           ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * 8ull;
       base < n_elems; base += stride) {
    if (kVec && base + 8 <= n_elems) {
      const uint2 v = *reinterpret_cast<const uint2*>(src + base);
      *reinterpret_cast<uint4*>(dst + base) =
          bf16x8_from_fp8x8(v.x | ((unsigned long long)v.y << 32));
    } else {
      const unsigned long long end =
          base + 8 <= n_elems ? base + 8 : n_elems;
      for (unsigned long long i = base; i < end; ++i)
        dst[i] = f32_to_bf16(fp8_to_f32(src[i]));
    }
  }
}

// ---------------------------------------------------------------------------
// FedAvg weighted reduce: out = sum_k w_k * in_k   (fp32 accumulation)
// ---------------------------------------------------------------------------
constexpr int kMaxInputs = 16;

struct ReduceArgs {
  const void* in[kMaxInputs];
  float w[kMaxInputs];
  int k;
};

template <typename T>
__device__ __forceinline__ float to_f32(T v);
template <>
__device__ __forceinline__ float to_f32<uint16_t>(uint16_t v) {
  return bf16_to_f32(v);
}
template <>
__device__ __forceinline__ float to_f32<__half>(__half v) {
  return __half2float(v);
}
template <>
__device__ __forceinline__ float to_f32<float>(float v) {
  return v;
}

template <typename T>
__device__ __forceinline__ T from_f32(float v);
template <>
__device__ __forceinline__ uint16_t from_f32<uint16_t>(float v) {
  return f32_to_bf16(v);
}
template <>
__device__ __forceinline__ __half from_f32<__half>(float v) {
  return __float2half(v);
}
template <>
__device__ __forceinline__ float from_f32<float>(float v) {
  return v;
}

// VEC elements per lane per iteration, sized to 16-byte loads.  kVec: out and
// every input are 16-byte aligned (decided on the host); otherwise each lane
// walks its VEC elements with scalar accesses — same values, same order.
template <typename T, int VEC, bool kVec>
__global__ void fedavg_reduce_kernel(T* __restrict__ out, ReduceArgs args,
                                     unsigned long long n) {
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x * VEC;
  for (unsigned long long base =
           ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
       base < n; base += stride) {
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    const bool full = kVec && base + VEC <= n;
    const unsigned long long end = base + VEC <= n ? base + VEC : n;
    for (int j = 0; j < args.k; ++j) {
      const T* in = reinterpret_cast<const T*>(args.in[j]);
      const float w = args.w[j];
      if (full) {
        // One 16-byte load per input per iteration.
        using VecT = uint4;
        const VecT raw = *reinterpret_cast<const VecT*>(in + base);
        const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += w * to_f32<T>(e[v]);
      } else {
        for (unsigned long long i = base; i < end; ++i)
          acc[i - base] += w * to_f32<T>(in[i]);
      }
    }
    if (full) {
      T tmp[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) tmp[v] = from_f32<T>(acc[v]);
      *reinterpret_cast<uint4*>(out + base) = *reinterpret_cast<uint4*>(tmp);
    } else {
      for (unsigned long long i = base; i < end; ++i)
        out[i] = from_f32<T>(acc[i - base]);
    }
  }
}

// ---------------------------------------------------------------------------
// MFMA variant of the weighted combine (bf16, k <= 32).
//
// Maps out[j] = Σ_k w_k·in_k[j] onto v_mfma_f32_16x16x32_bf16 as
// C = A·B with A[i][kk] = in_kk[base+i] (16 output positions per MFMA) and
// B[kk][j] = w_kk (constant across j).  C's column 0 lanes write the tile.
//
// This op is HBM-bound, so the VALU kernel above (16-byte lanes) is the
// default and is faster — the guide's rule is that GEMM-shaped work belongs
// on MFMA, and a weighted elementwise combine is not GEMM-shaped.  This
// kernel exists as the measured MFMA alternative (numbers in
// profiles/microbench): per MFMA only 16 of 256 output slots are useful and
// the A-operand reads amplify 32/k×.
// ---------------------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__global__ void fedavg_reduce_mfma_kernel(uint16_t* __restrict__ out,
                                          ReduceArgs args,
                                          unsigned long long n) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const unsigned long long waves_total =
      (unsigned long long)gridDim.x * blockDim.x / kWave;

  // B fragment: lane l supplies B[kk][j] for kk = (l>>4)*8 + e, j = l&15.
  bf16x8 b_frag;
  {
    const int kk_base = (lane >> 4) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kk = kk_base + e;
      const float w = (kk < args.k) ? args.w[kk] : 0.0f;
      b_frag[e] = (short)f32_to_bf16(w);
    }
  }

  // Each wave iteration computes 16 consecutive outputs.
  const int i = lane & 15;           // output position within the tile
  const int kk_base = (lane >> 4) * 8;
  for (unsigned long long base = (unsigned long long)wave * 16; base < n;
       base += waves_total * 16) {
    bf16x8 a_frag;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kk = kk_base + e;
      uint16_t v = 0;
      if (kk < args.k && base + i < n) {
        v = reinterpret_cast<const uint16_t*>(args.in[kk])[base + i];
      }
      a_frag[e] = (short)v;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, b_frag, acc, 0, 0, 0);
    // C layout: col = lane&15, row = (lane>>4)*4 + reg.  A's rows are the
    // output positions, so lanes in column 0 write rows (= positions).
    if ((lane & 15) == 0) {
      const int row0 = (lane >> 4) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned long long j = base + row0 + r;
        if (j < n) out[j] = f32_to_bf16(acc[r]);
      }
    }
  }
}

// dst += mask ? src : 0   (secure-aggregation style mask-add)
template <typename T>
__global__ void masked_add_kernel(T* __restrict__ dst,
                                  const T* __restrict__ src,
                                  const uint8_t* __restrict__ mask,
                                  unsigned long long n) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += stride) {
    if (mask[i])
      dst[i] = from_f32<T>(to_f32<T>(dst[i]) + to_f32<T>(src[i]));
  }
}

// ---------------------------------------------------------------------------
// host-side state: tables + power matrices on device (uploaded once)
// ---------------------------------------------------------------------------
struct DeviceConsts {
  uint32_t* tables = nullptr;   // 8*256
  uint32_t* pows = nullptr;     // kMaxPow*32
  uint32_t* halfmat = nullptr;  // 32 (shift by kSubLen/2)
};

DeviceConsts& get_device_consts() {
  static DeviceConsts consts;
  static std::once_flag flag;
  std::call_once(flag, [] {
    std::vector<uint32_t> tables(8 * 256);
    rayfed_crc::make_slice8_tables(tables.data());
    std::vector<uint32_t> pows(kMaxPow * 32);
    // pows[j] = shift matrix for kSubLen * 2^j zero bytes
    uint32_t m[32];
    rayfed_crc::shift_matrix(m, kSubLen);
    std::memcpy(&pows[0], m, sizeof(m));
    for (int j = 1; j < kMaxPow; ++j) {
      rayfed_crc::gf2_square(&pows[j * 32], &pows[(j - 1) * 32]);
    }
    uint32_t halfmat[32];
    rayfed_crc::shift_matrix(halfmat, kSubLen / 2);
    HIP_CHECK(hipMalloc(&consts.tables, tables.size() * 4));
    HIP_CHECK(hipMalloc(&consts.pows, pows.size() * 4));
    HIP_CHECK(hipMalloc(&consts.halfmat, sizeof(halfmat)));
    HIP_CHECK(hipMemcpy(consts.tables, tables.data(), tables.size() * 4,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(consts.pows, pows.data(), pows.size() * 4,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(consts.halfmat, halfmat, sizeof(halfmat),
                        hipMemcpyHostToDevice));
  });
  return consts;
}

TailParam make_tail_param(unsigned long long n, uint32_t T) {
  TailParam p;
  const unsigned long long tail =
      (T == 0) ? 0 : n - (unsigned long long)(T - 1) * kSubLen;
  rayfed_crc::shift_matrix(p.m, tail);
  p.final_xor = rayfed_crc::shift_apply(n, 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
  return p;
}

inline bool aligned_to(const void* p, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// The recurring argument check; each caller raises its own message.
inline bool cuda_contiguous(const torch::Tensor& t, at::ScalarType dtype) {
  return t.is_cuda() && t.dtype() == dtype && t.is_contiguous();
}

// Kernel element types as bits, so that a call site names the ones it has
// kernels for.
constexpr unsigned kBf16 = 1u, kF16 = 2u, kF32 = 4u;
constexpr unsigned kAnyFloat = kBf16 | kF16 | kF32;

inline unsigned elem_bit(const torch::Tensor& t) {
  return t.dtype() == torch::kBFloat16 ? kBf16
         : t.dtype() == torch::kHalf   ? kF16
         : t.dtype() == torch::kFloat  ? kF32
                                       : 0u;
}

// Calls f(T{}) with the kernel element type of t's dtype: uint16_t for bf16,
// __half, float.  A dtype outside kAllowed raises `msg` followed by the dtype,
// and f is instantiated for the allowed types only.
template <unsigned kAllowed, typename F>
void dispatch_elem(const torch::Tensor& t, const char* msg, F&& f) {
  const unsigned bit = elem_bit(t) & kAllowed;
  TORCH_CHECK(bit, msg, t.dtype());
  if constexpr ((kAllowed & kBf16) != 0) {
    if (bit == kBf16) return f(uint16_t{});
  }
  if constexpr ((kAllowed & kF16) != 0) {
    if (bit == kF16) return f(__half{});
  }
  if constexpr ((kAllowed & kF32) != 0) {
    if (bit == kF32) return f(float{});
  }
}

template <typename T>
T* elem_ptr(const torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

// Launch shared by the CRC kernels (one thread per kSubLen output bytes) and
// the finalize kernel behind them: int32[3] on src's device, out[2] = CRC32
// of the src.numel() bytes the kernel reads or produces.
template <typename SrcT>
torch::Tensor crc_launch(void (*kernel)(const SrcT*, uint8_t*,
                                        unsigned long long, uint32_t,
                                        const uint32_t*, const uint32_t*,
                                        const uint32_t*, uint32_t*),
                         const torch::Tensor& src, uint8_t* dst) {
  const unsigned long long n = src.numel();
  auto out = torch::zeros(
      {3}, torch::dtype(torch::kInt32).device(src.device()));
  if (n == 0) return out;  // crc32("") == 0 — out[2] already 0
  auto& consts = get_device_consts();
  const uint32_t T = (uint32_t)((n + kSubLen - 1) / kSubLen);  // threads
  const uint32_t blocks = (T + kBlock - 1) / kBlock;
  auto stream = at::hip::getCurrentHIPStream();
  uint32_t* o = reinterpret_cast<uint32_t*>(out.data_ptr<int32_t>());
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream,
                     elem_ptr<const SrcT>(src), dst, n, T, consts.tables,
                     consts.pows, consts.halfmat, o);
  hipLaunchKernelGGL(crc_finalize_kernel, dim3(1), dim3(kWave), 0, stream, o,
                     make_tail_param(n, T));
  return out;
}

// Launch shared by the hash64-mapped kernels: the zeroed int64[1] result on
// `dev`, the split of nbytes into u64 words and a tail, and the fixed grid
// the slot mapping rests on.  launch(grid, stream, n_words, tail, out) starts
// the kernel.
template <typename F>
torch::Tensor hash64_launch(const torch::Device& dev,
                            unsigned long long nbytes, F&& launch) {
  auto out = torch::zeros({1}, torch::dtype(torch::kInt64).device(dev));
  launch(dim3(kHashLanes / kBlock), at::hip::getCurrentHIPStream(),
         nbytes / 8, (uint32_t)(nbytes % 8),
         reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()));
  return out;
}

// ---------------------------------------------------------------------------
// torch bindings
// ---------------------------------------------------------------------------
torch::Tensor crc32_async(torch::Tensor bytes) {
  TORCH_CHECK(cuda_contiguous(bytes, torch::kUInt8),
              "crc32 expects a contiguous CUDA uint8 tensor");
  return crc_launch(crc32_kernel<false>, bytes, nullptr);
}

torch::Tensor hash64_async(torch::Tensor bytes) {
  TORCH_CHECK(cuda_contiguous(bytes, torch::kUInt8),
              "hash64 expects a contiguous CUDA uint8 tensor");
  const unsigned long long n = bytes.numel();
  const uint8_t* p = bytes.data_ptr<uint8_t>();
  TORCH_CHECK(aligned_to(p, 8), "hash64 requires 8-byte-aligned data");
  return hash64_launch(
      bytes.device(), n,
      [&](dim3 grid, hipStream_t stream, unsigned long long n_words,
          uint32_t tail_len, unsigned long long* out) {
        hipLaunchKernelGGL(hash64_kernel<false>, grid, dim3(kBlock), 0, stream,
                           reinterpret_cast<const unsigned long long*>(p),
                           nullptr, n_words, p + n_words * 8, nullptr,
                           tail_len, n, out);
      });
}

torch::Tensor pack_hash64_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kUInt8),
              "pack_hash64 expects contiguous CUDA uint8 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kUInt8) &&
                  dst.numel() >= src.numel(),
              "pack_hash64 dst too small");
  const unsigned long long n = src.numel();
  const uint8_t* p = src.data_ptr<uint8_t>();
  uint8_t* q = dst.data_ptr<uint8_t>();
  TORCH_CHECK(aligned_to(p, 8) && aligned_to(q, 8),
              "pack_hash64 requires 8-byte alignment");
  return hash64_launch(
      src.device(), n,
      [&](dim3 grid, hipStream_t stream, unsigned long long n_words,
          uint32_t tail_len, unsigned long long* out) {
        hipLaunchKernelGGL(hash64_kernel<true>, grid, dim3(kBlock), 0, stream,
                           reinterpret_cast<const unsigned long long*>(p),
                           reinterpret_cast<unsigned long long*>(q), n_words,
                           p + n_words * 8, q + n_words * 8, tail_len, n, out);
      });
}

int64_t crc32_sync(torch::Tensor bytes) {
  auto out = crc32_async(bytes);
  return (int64_t)(uint32_t)out[2].item<int32_t>();
}

torch::Tensor pack_crc_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kUInt8),
              "pack_crc expects contiguous CUDA uint8 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kUInt8) &&
                  dst.numel() >= src.numel(),
              "pack_crc dst too small");
  // The kernel picks 16-byte loads AND stores from src's alignment alone.
  TORCH_CHECK(!aligned_to(src.data_ptr(), 16) || aligned_to(dst.data_ptr(), 16),
              "pack_crc: dst must be 16-byte aligned when src is");
  return crc_launch(crc32_kernel<true>, src, dst.data_ptr<uint8_t>());
}

torch::Tensor pack_fp8_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kBFloat16),
              "pack_fp8 expects contiguous CUDA bf16 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kUInt8) &&
                  dst.numel() >= src.numel(),
              "pack_fp8 dst too small");
  // uint4 loads of src / uint2 stores of dst need 16 / 8-byte alignment;
  // views at odd element offsets take the scalar instantiation.
  const bool vec =
      aligned_to(src.data_ptr(), 16) && aligned_to(dst.data_ptr(), 8);
  return crc_launch(vec ? pack_fp8_kernel<true> : pack_fp8_kernel<false>, src,
                    dst.data_ptr<uint8_t>());
}

torch::Tensor pack_fp8_hash64_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kBFloat16),
              "pack_fp8_hash64 expects contiguous CUDA bf16 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kUInt8) &&
                  dst.numel() >= src.numel(),
              "pack_fp8_hash64 dst too small");
  const unsigned long long n = src.numel();  // fp8 output bytes
  TORCH_CHECK(aligned_to(src.data_ptr(), 16) && aligned_to(dst.data_ptr(), 8),
              "pack_fp8_hash64 alignment");
  return hash64_launch(
      src.device(), n,
      [&](dim3 grid, hipStream_t stream, unsigned long long n_words,
          uint32_t tail, unsigned long long* out) {
        hipLaunchKernelGGL(pack_fp8_hash64_kernel, grid, dim3(kBlock), 0,
                           stream, elem_ptr<const uint16_t>(src),
                           elem_ptr<unsigned long long>(dst), n_words, tail, n,
                           out);
      });
}

torch::Tensor unpack_fp8_hash64_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kUInt8),
              "unpack_fp8_hash64 expects contiguous CUDA uint8 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kBFloat16) &&
                  dst.numel() == src.numel(),
              "unpack_fp8_hash64 dst mismatch");
  const unsigned long long n = src.numel();
  TORCH_CHECK(aligned_to(src.data_ptr(), 8) && aligned_to(dst.data_ptr(), 16),
              "unpack_fp8_hash64 alignment");
  return hash64_launch(
      src.device(), n,
      [&](dim3 grid, hipStream_t stream, unsigned long long n_words,
          uint32_t tail, unsigned long long* out) {
        hipLaunchKernelGGL(unpack_fp8_hash64_kernel, grid, dim3(kBlock), 0,
                           stream, elem_ptr<const unsigned long long>(src),
                           elem_ptr<uint16_t>(dst), n_words, tail, n, out);
      });
}

void unpack_fp8_async(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(cuda_contiguous(src, torch::kUInt8),
              "unpack_fp8 expects contiguous CUDA uint8 src");
  TORCH_CHECK(cuda_contiguous(dst, torch::kBFloat16) &&
                  dst.numel() == src.numel(),
              "unpack_fp8 dst mismatch");
  const unsigned long long n = src.numel();
  if (n == 0) return;
  const uint32_t blocks =
      std::min<unsigned long long>(4096ull, (n / 8 + kBlock - 1) / kBlock + 1);
  auto stream = at::hip::getCurrentHIPStream();
  const bool vec =
      aligned_to(src.data_ptr(), 8) && aligned_to(dst.data_ptr(), 16);
  hipLaunchKernelGGL(vec ? unpack_fp8_kernel<true> : unpack_fp8_kernel<false>,
                     dim3(blocks), dim3(kBlock), 0, stream,
                     src.data_ptr<uint8_t>(), elem_ptr<uint16_t>(dst), n);
}

torch::Tensor fedavg_combine_hash_async(torch::Tensor out,
                                        torch::Tensor local,
                                        torch::Tensor peer_bytes, double wa,
                                        double wb) {
  TORCH_CHECK(cuda_contiguous(out, torch::kBFloat16),
              "combine_hash: out must be contiguous CUDA bf16");
  TORCH_CHECK(cuda_contiguous(local, torch::kBFloat16) &&
                  local.numel() == out.numel(),
              "combine_hash: local mismatch");
  TORCH_CHECK(cuda_contiguous(peer_bytes, torch::kUInt8) &&
                  peer_bytes.numel() == out.numel() * 2,
              "combine_hash: peer byte count mismatch");
  const unsigned long long nbytes = peer_bytes.numel();
  const uint8_t* p = peer_bytes.data_ptr<uint8_t>();
  TORCH_CHECK(aligned_to(p, 8) && aligned_to(local.data_ptr(), 8) &&
                  aligned_to(out.data_ptr(), 8),
              "combine_hash requires 8-byte alignment");
  return hash64_launch(
      out.device(), nbytes,
      [&](dim3 grid, hipStream_t stream, unsigned long long n_words,
          uint32_t tail_len, unsigned long long* hash_out) {
        hipLaunchKernelGGL(fedavg_combine_hash_kernel, grid, dim3(kBlock), 0,
                           stream, elem_ptr<uint16_t>(out),
                           elem_ptr<const uint16_t>(local),
                           reinterpret_cast<const unsigned long long*>(p),
                           n_words, p + n_words * 8, tail_len, nbytes,
                           (float)wa, (float)wb, hash_out);
      });
}

// Checks `inputs` against `out` and fills the kernel's table with the first
// kMaxInputs of them (the callers bound the count, each in its own words).
// Returns whether `out` and every input are 16-byte aligned.
bool fill_reduce_args(ReduceArgs& args, const torch::Tensor& out,
                      const std::vector<torch::Tensor>& inputs,
                      const std::vector<double>& weights) {
  const long long n = out.numel();
  args.k = (int)inputs.size();
  bool vec = aligned_to(out.data_ptr(), 16);
  for (int j = 0; j < args.k && j < kMaxInputs; ++j) {
    TORCH_CHECK(inputs[j].is_cuda() && inputs[j].is_contiguous() &&
                    inputs[j].numel() == n && inputs[j].dtype() == out.dtype(),
                "input ", j, " mismatch");
    args.in[j] = inputs[j].data_ptr();
    args.w[j] = (float)weights[j];
    vec = vec && aligned_to(args.in[j], 16);
  }
  return vec;
}

void fedavg_reduce_(torch::Tensor out, std::vector<torch::Tensor> inputs,
                    std::vector<double> weights) {
  TORCH_CHECK(!inputs.empty() && inputs.size() <= kMaxInputs,
              "fedavg_reduce_: 1..16 inputs");
  TORCH_CHECK(weights.size() == inputs.size(), "weights/inputs mismatch");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(), "out must be CUDA contiguous");
  const unsigned long long n = out.numel();
  ReduceArgs args;
  // The kernel's uint4 accesses need every pointer 16-byte aligned; slices
  // of a flat buffer at odd element offsets take the scalar instantiation.
  const bool vec = fill_reduce_args(args, out, inputs, weights);
  auto stream = at::hip::getCurrentHIPStream();
  // >= 2048 workgroups to fill 256 CUs across 8 XCDs (guide §1).
  const int blocks = 4096;
  dispatch_elem<kAnyFloat>(
      out, "fedavg_reduce_: unsupported dtype ", [&](auto tag) {
        using T = decltype(tag);
        constexpr int VEC = 16 / (int)sizeof(T);  // one 16-byte load per lane
        hipLaunchKernelGGL((vec ? fedavg_reduce_kernel<T, VEC, true>
                                : fedavg_reduce_kernel<T, VEC, false>),
                           dim3(blocks), dim3(kBlock), 0, stream,
                           elem_ptr<T>(out), args, n);
      });
}

void fedavg_reduce_mfma_(torch::Tensor out, std::vector<torch::Tensor> inputs,
                         std::vector<double> weights) {
  TORCH_CHECK(!inputs.empty() && inputs.size() <= 32,
              "fedavg_reduce_mfma_: 1..32 inputs");
  TORCH_CHECK(weights.size() == inputs.size(), "weights/inputs mismatch");
  TORCH_CHECK(cuda_contiguous(out, torch::kBFloat16),
              "out must be contiguous CUDA bf16");
  const unsigned long long n = out.numel();
  ReduceArgs args;
  fill_reduce_args(args, out, inputs, weights);
  TORCH_CHECK(args.k <= kMaxInputs,
              "fedavg_reduce_mfma_: pointer table limited to ", kMaxInputs);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(fedavg_reduce_mfma_kernel, dim3(4096), dim3(kBlock), 0,
                     stream, elem_ptr<uint16_t>(out), args, n);
}

void masked_add_(torch::Tensor dst, torch::Tensor src, torch::Tensor mask) {
  TORCH_CHECK(dst.is_cuda() && src.is_cuda() && mask.is_cuda() &&
                  dst.is_contiguous() && src.is_contiguous() &&
                  mask.is_contiguous(),
              "masked_add_: contiguous CUDA tensors required");
  TORCH_CHECK(src.dtype() == dst.dtype(),
              "masked_add_: src dtype ", src.dtype(), " != dst dtype ",
              dst.dtype());
  TORCH_CHECK(src.numel() == dst.numel() && mask.numel() == dst.numel(),
              "masked_add_: size mismatch");
  TORCH_CHECK(mask.dtype() == torch::kUInt8 || mask.dtype() == torch::kBool,
              "mask must be uint8/bool");
  const unsigned long long n = dst.numel();
  auto stream = at::hip::getCurrentHIPStream();
  const int blocks = 4096;
  dispatch_elem<kBf16 | kF32>(
      dst, "masked_add_: unsupported dtype ", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((masked_add_kernel<T>), dim3(blocks), dim3(kBlock),
                           0, stream, elem_ptr<T>(dst), elem_ptr<const T>(src),
                           static_cast<const uint8_t*>(mask.data_ptr()), n);
      });
}

int64_t crc32_combine_py(int64_t crc1, int64_t crc2, int64_t len2) {
  return (int64_t)rayfed_crc::crc32_combine((uint32_t)crc1, (uint32_t)crc2,
                                            (uint64_t)len2);
}

// ---------------------------------------------------------------------------
// Device IPC lane: same-node parties exchange GPU buffers directly
// (hipIpc*/dmabuf) — no host bounce at all.  The sender packs+CRCs into a
// dedicated hipMalloc'd staging buffer, ships the 64-byte handle; the
// receiver opens it (cached) and D2D-copies at HBM/xGMI rate.
// ---------------------------------------------------------------------------
std::tuple<int64_t, py::bytes> ipc_alloc(int64_t nbytes) {
  void* ptr = nullptr;
  HIP_CHECK(hipMalloc(&ptr, (size_t)nbytes));
  hipIpcMemHandle_t handle;
  HIP_CHECK(hipIpcGetMemHandle(&handle, ptr));
  return {reinterpret_cast<int64_t>(ptr),
          py::bytes(reinterpret_cast<const char*>(&handle), sizeof(handle))};
}

void ipc_free(int64_t ptr) {
  HIP_CHECK(hipFree(reinterpret_cast<void*>(ptr)));
}

int64_t ipc_open(py::bytes handle_bytes) {
  std::string h = handle_bytes;
  TORCH_CHECK(h.size() == sizeof(hipIpcMemHandle_t), "bad ipc handle size");
  hipIpcMemHandle_t handle;
  std::memcpy(&handle, h.data(), sizeof(handle));
  void* ptr = nullptr;
  HIP_CHECK(hipIpcOpenMemHandle(&ptr, handle, hipIpcMemLazyEnablePeerAccess));
  return reinterpret_cast<int64_t>(ptr);
}

void ipc_close(int64_t ptr) {
  HIP_CHECK(hipIpcCloseMemHandle(reinterpret_cast<void*>(ptr)));
}

torch::Tensor tensor_from_ptr(int64_t ptr, int64_t nbytes, int64_t device) {
  // Non-owning uint8 view of a raw device pointer (e.g. an opened IPC
  // mapping); the caller guarantees lifetime until the ack.
  auto options =
      torch::dtype(torch::kUInt8).device(torch::kCUDA, (int)device);
  return torch::from_blob(reinterpret_cast<void*>(ptr), {nbytes}, options);
}

// Pin an existing host mapping (e.g. a /dev/shm segment) for true-DMA
// D2H/H2D — the same-host shm lane registers pooled segments once.
void host_register(int64_t ptr, int64_t size) {
  HIP_CHECK(hipHostRegister(reinterpret_cast<void*>(ptr), (size_t)size,
                            hipHostRegisterDefault));
}

void host_unregister(int64_t ptr) {
  HIP_CHECK(hipHostUnregister(reinterpret_cast<void*>(ptr)));
}

#include "secagg_kernels.h"

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "rayfed_amd MI355X data-plane kernels (gfx950)";
  m.def("crc32_async", &crc32_async,
        "CRC32 of a device uint8 tensor -> int32[3] device tensor "
        "(out[2] = finalized CRC)");
  m.def("crc32", &crc32_sync, "CRC32 of a device uint8 tensor (synchronizes)");
  m.def("pack_hash64_async", &pack_hash64_async,
        "fused copy src->dst + hash64 of the bytes (one HBM read pass) -> "
        "int64[1] device tensor");
  m.def("hash64_async", &hash64_async,
        "memory-rate 64-bit FNV/murmur integrity hash -> int64[1] device "
        "tensor (device-IPC lane checksum; numpy reference in "
        "rayfed_amd/ops/hash_ref.py)");
  m.def("pack_crc_async", &pack_crc_async,
        "fused copy src->dst + CRC32; returns int32[3] device tensor");
  m.def("pack_fp8_async", &pack_fp8_async,
        "fused bf16 -> OCP fp8 e4m3 cast + CRC32 of the fp8 bytes");
  m.def("unpack_fp8_async", &unpack_fp8_async, "fp8 e4m3 bytes -> bf16");
  m.def("pack_fp8_hash64_async", &pack_fp8_hash64_async,
        "bf16 -> fp8 e4m3 cast fused with hash64 of the fp8 bytes");
  m.def("unpack_fp8_hash64_async", &unpack_fp8_hash64_async,
        "fp8 e4m3 bytes -> bf16 fused with hash64 of the fp8 bytes");
  m.def("fedavg_reduce_", &fedavg_reduce_,
        "out = sum_k w_k * in_k (bf16/f16/f32, fp32 accumulation)");
  m.def("fedavg_combine_hash_async", &fedavg_combine_hash_async,
        "out = wa*local + wb*peer_bytes(bf16) fused with the hash64 of the "
        "peer bytes -> int64[1] device tensor (zero-copy IPC combine)");
  m.def("fedavg_reduce_mfma_", &fedavg_reduce_mfma_,
        "MFMA (v_mfma_f32_16x16x32_bf16) variant of the weighted combine");
  m.def("masked_add_", &masked_add_, "dst += mask ? src : 0");
  m.def("secagg_mask_async", &secagg_mask_async,
        "out_i32 = quantise(x*weight) + sum_k signs[k]*ChaCha20(keys[k]) in "
        "Z/2^32 (spec + numpy reference: rayfed_amd/ops/secagg_ref.py)");
  m.def("secagg_aggregate_async", &secagg_aggregate_async,
        "out = dequantise(ring-sum of int32 inputs - signed ChaCha20 "
        "corrections of dropped parties)");
  m.def("secagg_mask_noise_async", &secagg_mask_noise_async,
        "secagg_mask_async plus on-device binomial noise: step * (popcount "
        "of `words` words of the noise key's ChaCha20 stream - 16*words) per "
        "element (differential privacy; same spec module)",
        pybind11::arg("x"), pybind11::arg("out"), pybind11::arg("keys"),
        pybind11::arg("signs"), pybind11::arg("noise_key"),
        pybind11::arg("words"), pybind11::arg("step"), pybind11::arg("round"),
        pybind11::arg("offset"), pybind11::arg("weight"),
        pybind11::arg("frac_bits"), pybind11::arg("max_blocks") = 0);
  m.def("sumsq_async", &sumsq_async,
        "float64 sum of squares of an fp32/bf16/fp16 tensor -> double[1] "
        "device tensor (per-block partials, no atomics: reproducible)");
  m.def("crc32_combine", &crc32_combine_py, "zlib-style CRC combine");
  m.def("host_register", &host_register, "hipHostRegister an existing mapping");
  m.def("host_unregister", &host_unregister, "hipHostUnregister");
  m.def("ipc_alloc", &ipc_alloc,
        "hipMalloc + hipIpcGetMemHandle -> (ptr, handle bytes)");
  m.def("ipc_free", &ipc_free);
  m.def("ipc_open", &ipc_open, "hipIpcOpenMemHandle -> ptr");
  m.def("ipc_close", &ipc_close);
  m.def("tensor_from_ptr", &tensor_from_ptr,
        "non-owning uint8 CUDA tensor over a raw device pointer");
}
