// Secure aggregation kernels — pairwise ChaCha20 masks in the ring Z/2^32.
//
// Included from rayfed_hip.hip inside its anonymous namespace (uses kBlock,
// kMaxInputs, to_f32/from_f32 and the host helpers aligned_to,
// cuda_contiguous, dispatch_elem).  The bit-exact specification and the numpy
// oracle are in rayfed_amd/ops/secagg_ref.py; tests/test_secagg_gpu.py pins
// every path here against it.
//
//   * secagg_mask_kernel<T>       sender: quantise fp32/bf16/fp16 to
//     fixed point and add the signed ChaCha20 keystream of up to 15 peers.
//   * secagg_mask_noise_kernel<T, W>  the same pass with on-device binomial
//     noise (popcounts of a private ChaCha20 stream, W words per element)
//     added before the masks — differential privacy.
//   * sumsq_kernel<T>             float64 sum of squares (the L2 norm that
//     clipping needs), per-block partials, no atomics.
//   * secagg_aggregate_kernel<OutT, EPL>  aggregator: ring-sum of K int32
//     inputs, subtract the residual keystreams of dropped parties,
//     dequantise.  EPL = 4 is the pure streaming reduce (no corrections,
//     one 16-byte load per input per lane, as fedavg_reduce_kernel);
//     EPL = 16 gives each lane whole ChaCha20 blocks.
//
// The keystream lives entirely in registers: one lane runs one 16-word
// block per peer, keys and signs are kernel arguments (wave-uniform), the
// rotates compile to single v_alignbit_b32 ops, and there is no LDS.
#pragma once

#include <type_traits>

constexpr int kSecaggMaxKeys = 16;  // per launch; the wrapper chunks more
constexpr int kSecaggMaxFracBits = 30;
constexpr unsigned long long kSecaggMaxElements = 1ull << 36;

struct SecaggKeys {
  uint32_t key[kSecaggMaxKeys][8];  // little-endian key words
  int32_t sign[kSecaggMaxKeys];     // +1 / -1
  int k;
};

// Binomial-noise stream (differential privacy): the party's private key and
// the third nonce word that separates it from every pair-mask keystream.
constexpr uint32_t kSecaggNoiseNonce = 1u;
constexpr int64_t kSecaggMaxNoiseStep = 1ll << 20;

struct SecaggNoiseKey {
  uint32_t key[8];  // little-endian key words
};

struct SecaggInputs {
  const int32_t* in[kMaxInputs];
  int k;
};

#define SECAGG_QR(a, b, c, d)                           \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 16);    \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 12);    \
  a += b; d ^= a; d = __builtin_rotateleft32(d, 8);     \
  c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// One ChaCha20 block (RFC 8439 §2.3 layout): counter `ctr`, nonce words
// (n0, n1, n2).  `key` is wave-uniform.  n2 is 0 for the pair-mask
// keystream and kSecaggNoiseNonce for the noise stream; both are literals at
// the call sites, so the pair-mask code is what it was with a fixed 0.
__device__ __forceinline__ void chacha20_block(const uint32_t* key,
                                               uint32_t ctr, uint32_t n0,
                                               uint32_t n1, uint32_t n2,
                                               uint32_t out[16]) {
  const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u,
                 c3 = 0x6b206574u;
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3;
  uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
  uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
  uint32_t x12 = ctr, x13 = n0, x14 = n1, x15 = n2;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    SECAGG_QR(x0, x4, x8, x12)
    SECAGG_QR(x1, x5, x9, x13)
    SECAGG_QR(x2, x6, x10, x14)
    SECAGG_QR(x3, x7, x11, x15)
    SECAGG_QR(x0, x5, x10, x15)
    SECAGG_QR(x1, x6, x11, x12)
    SECAGG_QR(x2, x7, x8, x13)
    SECAGG_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + c0;       out[1] = x1 + c1;
  out[2] = x2 + c2;       out[3] = x3 + c3;
  out[4] = x4 + key[0];   out[5] = x5 + key[1];
  out[6] = x6 + key[2];   out[7] = x7 + key[3];
  out[8] = x8 + key[4];   out[9] = x9 + key[5];
  out[10] = x10 + key[6]; out[11] = x11 + key[7];
  out[12] = x12 + ctr;    out[13] = x13 + n0;
  out[14] = x14 + n1;     out[15] = x15 + n2;
}

#undef SECAGG_QR

// acc[e] += sign * KS(key, round, block ctr)[e] for every key in `keys`.
// kNegate flips every sign (the aggregator SUBTRACTS its corrections).
template <bool kNegate>
__device__ __forceinline__ void secagg_apply_keys(const SecaggKeys& keys,
                                                  uint32_t ctr, uint32_t n0,
                                                  uint32_t n1,
                                                  uint32_t acc[16]) {
  for (int j = 0; j < keys.k; ++j) {
    uint32_t ks[16];
    chacha20_block(keys.key[j], ctr, n0, n1, 0u, ks);
    if ((keys.sign[j] > 0) != kNegate) {  // wave-uniform branch
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] += ks[e];
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] -= ks[e];
    }
  }
}

// sat_i32(rint(fl32(x*w) * scale)); NaN -> 0.  Two separate fp32 multiplies
// (nothing to contract into an FMA), v_rndne for the half-to-even rint, and
// an explicit clamp instead of relying on the conversion's saturation.
__device__ __forceinline__ uint32_t secagg_quantize(float x, float w,
                                                    float scale) {
  const float t = x * w;
  const float r = rintf(t * scale);
  int q;
  if (r >= 2147483648.0f) {
    q = 2147483647;
  } else if (r <= -2147483648.0f) {
    q = -2147483647 - 1;
  } else if (r != r) {
    q = 0;
  } else {
    q = (int)r;
  }
  return (uint32_t)q;
}

// Each lane owns whole 16-element blocks: block b covers elements
// [16b, 16b+16) of x and uses ChaCha20 counter blk0 + b.  `vec_ok` (both
// base pointers 16-byte aligned) selects 16-byte loads/stores for full
// blocks; the ragged final block and misaligned views go element-wise.
template <typename T>
__global__ void secagg_mask_kernel(const T* __restrict__ x,
                                   int32_t* __restrict__ out,
                                   unsigned long long n,
                                   unsigned long long blk0, uint32_t n0,
                                   uint32_t n1, float weight, float scale,
                                   SecaggKeys keys, bool vec_ok) {
  const unsigned long long nblk = (n + 15ull) / 16ull;
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long b =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       b < nblk; b += stride) {
    const unsigned long long base = b * 16ull;
    const bool vec = vec_ok && (base + 16ull <= n);
    const int cnt = (base + 16ull <= n) ? 16 : (int)(n - base);
    uint32_t acc[16];
    if (vec) {
      constexpr int kLoads = (int)sizeof(T);  // 16 elements = sizeof(T) uint4
      uint4 raw[kLoads];
#pragma unroll
      for (int v = 0; v < kLoads; ++v)
        raw[v] = reinterpret_cast<const uint4*>(x + base)[v];
      const T* e = reinterpret_cast<const T*>(raw);
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[i] = secagg_quantize(to_f32<T>(e[i]), weight, scale);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[i] = (i < cnt)
                     ? secagg_quantize(to_f32<T>(x[base + i]), weight, scale)
                     : 0u;
    }
    secagg_apply_keys<false>(keys, (uint32_t)(blk0 + b), n0, n1, acc);
    if (vec) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        reinterpret_cast<uint4*>(out + base)[v] = make_uint4(
            acc[4 * v], acc[4 * v + 1], acc[4 * v + 2], acc[4 * v + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < cnt) out[base + i] = (int32_t)acc[i];
    }
  }
}

// acc[i] += step * (sum_{t<W} popcount(NS(W*(16*blk + i) + t)) - 16*W) for the
// 16 elements of block `blk`: the binomial noise of secagg_ref.py.  The
// element's W words never straddle a ChaCha20 block, so noise block t (counter
// W*blk + t) carries the words of elements [t*E, t*E + E), E = 16/W.  The
// t loop stays rolled (one block function in the code); the uniform compare
// `t == i / E` routes each sum to its accumulator with static register
// indices only.
template <int W>
__device__ __forceinline__ void secagg_add_noise(const SecaggNoiseKey& nk,
                                                 uint32_t blk, uint32_t n0,
                                                 uint32_t n1, uint32_t step,
                                                 uint32_t acc[16]) {
  constexpr int E = 16 / W;  // elements per noise block
  const uint32_t centre = 0u - 16u * (uint32_t)W * step;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] += centre;
#pragma unroll 1
  for (int t = 0; t < W; ++t) {
    uint32_t ns[16];
    chacha20_block(nk.key, (uint32_t)W * blk + (uint32_t)t, n0, n1,
                   kSecaggNoiseNonce, ns);
    uint32_t s[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < W; ++j)
        c += (uint32_t)__builtin_popcount(ns[W * k + j]);
      s[k] = c * step;
    }
    if constexpr (W == 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += s[i];
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += (t == i / E) ? s[i % E] : 0u;
    }
  }
}

// secagg_mask_kernel plus on-device binomial noise (W keystream words per
// element): same lane ownership, loads and stores; the un-noised quantised
// update never reaches memory.  Noise counters W*(blk0 + b) + t, t < W.
template <typename T, int W>
__global__ void secagg_mask_noise_kernel(const T* __restrict__ x,
                                         int32_t* __restrict__ out,
                                         unsigned long long n,
                                         unsigned long long blk0, uint32_t n0,
                                         uint32_t n1, float weight,
                                         float scale, SecaggKeys keys,
                                         SecaggNoiseKey nkey, uint32_t step,
                                         bool vec_ok) {
  const unsigned long long nblk = (n + 15ull) / 16ull;
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long b =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       b < nblk; b += stride) {
    const unsigned long long base = b * 16ull;
    const bool vec = vec_ok && (base + 16ull <= n);
    const int cnt = (base + 16ull <= n) ? 16 : (int)(n - base);
    uint32_t acc[16];
    if (vec) {
      constexpr int kLoads = (int)sizeof(T);  // 16 elements = sizeof(T) uint4
      uint4 raw[kLoads];
#pragma unroll
      for (int v = 0; v < kLoads; ++v)
        raw[v] = reinterpret_cast<const uint4*>(x + base)[v];
      const T* e = reinterpret_cast<const T*>(raw);
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[i] = secagg_quantize(to_f32<T>(e[i]), weight, scale);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[i] = (i < cnt)
                     ? secagg_quantize(to_f32<T>(x[base + i]), weight, scale)
                     : 0u;
    }
    // (offset + n) * W <= 2^36 is validated: W*(blk0 + b) + t fits 32 bits.
    secagg_add_noise<W>(nkey, (uint32_t)(blk0 + b), n0, n1, step, acc);
    secagg_apply_keys<false>(keys, (uint32_t)(blk0 + b), n0, n1, acc);
    if (vec) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        reinterpret_cast<uint4*>(out + base)[v] = make_uint4(
            acc[4 * v], acc[4 * v + 1], acc[4 * v + 2], acc[4 * v + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < cnt) out[base + i] = (int32_t)acc[i];
    }
  }
}

// Sum of squares for L2 clipping.  Each lane accumulates double(x)^2 in a
// double (every square of an fp32/bf16/fp16 value is exact in double), the
// wave reduces by shuffles, the block's four waves through LDS, and each
// block writes one partial; sumsq_final_kernel adds the partials in a fixed
// order.  No atomics: the result is reproducible run to run.
__device__ __forceinline__ double sumsq_block_reduce(double v, double* wsum) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) r += wsum[w];
  }
  return r;  // valid in thread 0
}

template <typename T>
__device__ __forceinline__ double sumsq_vec(const uint4& raw, double acc) {
  constexpr int kPer = 16 / (int)sizeof(T);
  const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const double d = (double)to_f32<T>(e[i]);
    acc = fma(d, d, acc);  // d*d is exact, so this is acc + d^2 rounded once
  }
  return acc;
}

// kVec: x is 16-byte aligned; lanes stream uint4s (four in flight per
// iteration) and the first lanes of the grid take the < 16-byte tail.
template <typename T, bool kVec>
__global__ void sumsq_kernel(const T* __restrict__ x, unsigned long long n,
                             double* __restrict__ partials) {
  __shared__ double wsum[kBlock / kWave];
  const unsigned long long tid =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  double acc = 0.0;
  if constexpr (kVec) {
    constexpr int kPer = 16 / (int)sizeof(T);
    const unsigned long long nvec = n / kPer;
    const uint4* xv = reinterpret_cast<const uint4*>(x);
    unsigned long long v = tid;
    for (; v + 3ull * stride < nvec; v += 4ull * stride) {
      const uint4 r0 = xv[v];
      const uint4 r1 = xv[v + stride];
      const uint4 r2 = xv[v + 2ull * stride];
      const uint4 r3 = xv[v + 3ull * stride];
      acc = sumsq_vec<T>(r0, acc);
      acc = sumsq_vec<T>(r1, acc);
      acc = sumsq_vec<T>(r2, acc);
      acc = sumsq_vec<T>(r3, acc);
    }
    for (; v < nvec; v += stride) acc = sumsq_vec<T>(xv[v], acc);
    const unsigned long long i = nvec * kPer + tid;  // tail: < kPer elements
    if (i < n) {
      const double d = (double)to_f32<T>(x[i]);
      acc = fma(d, d, acc);
    }
  } else {
    for (unsigned long long i = tid; i < n; i += stride) {
      const double d = (double)to_f32<T>(x[i]);
      acc = fma(d, d, acc);
    }
  }
  const double r = sumsq_block_reduce(acc, wsum);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

__global__ void sumsq_final_kernel(const double* __restrict__ partials,
                                   int count, double* __restrict__ out) {
  __shared__ double wsum[kBlock / kWave];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += kBlock) acc += partials[i];
  const double r = sumsq_block_reduce(acc, wsum);
  if (threadIdx.x == 0) out[0] = r;
}

// OutT = int32_t stores the raw ring sum (the accumulator between chunked
// correction launches); float / uint16_t (bf16) / __half dequantise.
template <typename OutT>
__device__ __forceinline__ OutT secagg_finish(uint32_t s, float inv_scale) {
  if constexpr (std::is_same_v<OutT, int32_t>) {
    return (int32_t)s;
  } else {
    return from_f32<OutT>((float)(int32_t)s * inv_scale);  // v_cvt: RNE
  }
}

// `out` may alias an input (the in-place int32 accumulator): every lane
// reads exactly the elements it writes, so neither side is __restrict__.
template <typename OutT, int EPL>
__global__ void secagg_aggregate_kernel(OutT* out, SecaggInputs ins,
                                        unsigned long long n,
                                        unsigned long long blk0, uint32_t n0,
                                        uint32_t n1, float inv_scale,
                                        SecaggKeys corr, bool vec_ok) {
  static_assert(EPL == 4 || EPL == 16, "4 (streaming) or 16 (ChaCha block)");
  const unsigned long long nchunk = (n + EPL - 1ull) / EPL;
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long b =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       b < nchunk; b += stride) {
    const unsigned long long base = b * EPL;
    const bool full = base + EPL <= n;
    const bool vec = vec_ok && full;
    const int cnt = full ? EPL : (int)(n - base);
    uint32_t acc[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) acc[i] = 0u;
    for (int j = 0; j < ins.k; ++j) {
      const int32_t* in = ins.in[j];
      if (vec) {
#pragma unroll
        for (int v = 0; v < EPL / 4; ++v) {
          const uint4 raw = reinterpret_cast<const uint4*>(in + base)[v];
          acc[4 * v] += raw.x;
          acc[4 * v + 1] += raw.y;
          acc[4 * v + 2] += raw.z;
          acc[4 * v + 3] += raw.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < EPL; ++i)
          if (i < cnt) acc[i] += (uint32_t)in[base + i];
      }
    }
    if constexpr (EPL == 16) {
      secagg_apply_keys<true>(corr, (uint32_t)(blk0 + b), n0, n1, acc);
    }
    if (vec) {
      // EPL*sizeof(OutT) is 8 (one 8-byte store) or a multiple of 16.
      alignas(16) OutT tmp[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i)
        tmp[i] = secagg_finish<OutT>(acc[i], inv_scale);
      constexpr int kBytes = EPL * (int)sizeof(OutT);
      if constexpr (kBytes % 16 == 0) {
#pragma unroll
        for (int v = 0; v < kBytes / 16; ++v)
          reinterpret_cast<uint4*>(out + base)[v] =
              reinterpret_cast<const uint4*>(tmp)[v];
      } else {
        static_assert(kBytes == 8, "unexpected store width");
        *reinterpret_cast<uint2*>(out + base) =
            *reinterpret_cast<const uint2*>(tmp);
      }
    } else {
#pragma unroll
      for (int i = 0; i < EPL; ++i)
        if (i < cnt) out[base + i] = secagg_finish<OutT>(acc[i], inv_scale);
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
inline void secagg_check_range(const char* who, unsigned long long n,
                               int64_t offset, int64_t frac_bits) {
  TORCH_CHECK(frac_bits >= 0 && frac_bits <= kSecaggMaxFracBits, who,
              ": frac_bits must be in [0, 30]");
  TORCH_CHECK(offset >= 0 && offset % 16 == 0, who,
              ": offset must be a non-negative multiple of 16");
  TORCH_CHECK((unsigned long long)offset <= kSecaggMaxElements &&
                  n <= kSecaggMaxElements - (unsigned long long)offset,
              who, ": offset + n exceeds 2^36 (ChaCha20 counter would wrap)");
}

// Eight little-endian key words from 32 key bytes.
inline void secagg_unpack_key(uint32_t dst[8], const uint8_t* p) {
  for (int w = 0; w < 8; ++w, p += 4)
    dst[w] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) |
             ((uint32_t)p[3] << 24);
}

// Fill `dst` from rows [lo, lo+cnt) of a CPU uint8[K,32] / int32[K] pair.
inline void secagg_fill_keys(SecaggKeys& dst, const torch::Tensor& keys,
                             const torch::Tensor& signs, int64_t lo,
                             int64_t cnt) {
  dst.k = (int)cnt;
  const uint8_t* kp = keys.data_ptr<uint8_t>() + lo * 32;
  const int32_t* sp = signs.data_ptr<int32_t>() + lo;
  for (int64_t j = 0; j < cnt; ++j) {
    secagg_unpack_key(dst.key[j], kp + j * 32);
    dst.sign[j] = sp[j];
  }
}

inline void secagg_check_keys(const char* who, const torch::Tensor& keys,
                              const torch::Tensor& signs) {
  TORCH_CHECK(!keys.is_cuda() && keys.dtype() == torch::kUInt8 &&
                  keys.is_contiguous() && keys.dim() == 2 &&
                  keys.size(1) == 32,
              who, ": keys must be a contiguous CPU uint8[K,32] tensor");
  TORCH_CHECK(!signs.is_cuda() && signs.dtype() == torch::kInt32 &&
                  signs.is_contiguous() && signs.dim() == 1 &&
                  signs.size(0) == keys.size(0),
              who, ": signs must be a contiguous CPU int32[K] tensor");
  const int32_t* sp = signs.data_ptr<int32_t>();
  for (int64_t j = 0; j < signs.size(0); ++j)
    TORCH_CHECK(sp[j] == 1 || sp[j] == -1, who, ": signs must be +1 or -1");
}

// Where a launch sits in the keystream: the round is the ChaCha20 nonce's
// first two words, the element offset the first block counter.
struct SecaggPos {
  unsigned long long blk0;
  uint32_t n0, n1;
};

inline SecaggPos secagg_pos(uint64_t round, int64_t offset) {
  return {(unsigned long long)offset / 16ull,
          (uint32_t)(round & 0xffffffffull), (uint32_t)(round >> 32)};
}

// Enough workgroups to fill 256 CUs; the kernels grid-stride beyond that.
inline int secagg_grid(unsigned long long items) {
  const unsigned long long want = (items + kBlock - 1) / kBlock;
  return (int)std::min<unsigned long long>(
      4096ull, std::max<unsigned long long>(1ull, want));
}

// What secagg_mask and secagg_mask_noise share before their own launch: the
// checks of x, out, the peers' keys and the range, and every kernel argument
// that follows from them.  n may be 0; the caller then launches nothing.
struct SecaggMaskPlan {
  SecaggKeys keys{};
  unsigned long long n;
  SecaggPos pos;
  float weight, scale;
  bool vec_ok;
  int blocks;
  int32_t* out;
};

inline SecaggMaskPlan secagg_mask_plan(const char* who, const torch::Tensor& x,
                                       const torch::Tensor& out,
                                       const torch::Tensor& keys,
                                       const torch::Tensor& signs,
                                       uint64_t round, int64_t offset,
                                       double weight, int64_t frac_bits) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), who,
              ": x must be CUDA contiguous");
  TORCH_CHECK(cuda_contiguous(out, torch::kInt32) &&
                  out.numel() == x.numel() && out.device() == x.device(),
              who,
              ": out must be a contiguous int32 tensor of x's length on x's "
              "device");
  secagg_check_keys(who, keys, signs);
  TORCH_CHECK(keys.size(0) <= kSecaggMaxKeys - 1, who, ": at most 15 peers");
  SecaggMaskPlan p;
  p.n = x.numel();
  secagg_check_range(who, p.n, offset, frac_bits);
  secagg_fill_keys(p.keys, keys, signs, 0, keys.size(0));
  p.pos = secagg_pos(round, offset);
  p.weight = (float)weight;
  p.scale = (float)(1ull << frac_bits);
  p.vec_ok = aligned_to(x.data_ptr(), 16) && aligned_to(out.data_ptr(), 16);
  p.blocks = secagg_grid((p.n + 15ull) / 16ull);
  p.out = out.data_ptr<int32_t>();
  return p;
}

void secagg_mask_async(torch::Tensor x, torch::Tensor out, torch::Tensor keys,
                       torch::Tensor signs, uint64_t round, int64_t offset,
                       double weight, int64_t frac_bits) {
  const SecaggMaskPlan p = secagg_mask_plan("secagg_mask", x, out, keys, signs,
                                            round, offset, weight, frac_bits);
  if (p.n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_elem<kAnyFloat>(
      x, "secagg_mask: unsupported dtype ", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((secagg_mask_kernel<T>), dim3(p.blocks),
                           dim3(kBlock), 0, stream, elem_ptr<const T>(x),
                           p.out, p.n, p.pos.blk0, p.pos.n0, p.pos.n1,
                           p.weight, p.scale, p.keys, p.vec_ok);
      });
}

// max_blocks = 0: the normal grid; > 0 caps it (drives the grid-stride loop
// at a small n).
void secagg_mask_noise_async(torch::Tensor x, torch::Tensor out,
                             torch::Tensor keys, torch::Tensor signs,
                             torch::Tensor noise_key, int64_t words,
                             int64_t step, uint64_t round, int64_t offset,
                             double weight, int64_t frac_bits,
                             int64_t max_blocks) {
  const char* bad_dtype = "secagg_mask_noise: unsupported dtype ";
  const SecaggMaskPlan p =
      secagg_mask_plan("secagg_mask_noise", x, out, keys, signs, round, offset,
                       weight, frac_bits);
  TORCH_CHECK(elem_bit(x) & kAnyFloat, bad_dtype, x.dtype());
  TORCH_CHECK(!noise_key.is_cuda() && noise_key.dtype() == torch::kUInt8 &&
                  noise_key.is_contiguous() && noise_key.dim() == 1 &&
                  noise_key.size(0) == 32,
              "secagg_mask_noise: noise_key must be a contiguous CPU "
              "uint8[32] tensor");
  TORCH_CHECK(words == 1 || words == 2 || words == 4 || words == 8 ||
                  words == 16,
              "secagg_mask_noise: words must be 1, 2, 4, 8 or 16");
  TORCH_CHECK(step >= 1 && step <= kSecaggMaxNoiseStep,
              "secagg_mask_noise: step must be in [1, 2^20]");
  TORCH_CHECK(max_blocks >= 0, "secagg_mask_noise: max_blocks must be >= 0");
  // offset + n <= 2^36 holds, so the product below cannot overflow 64 bits.
  TORCH_CHECK(((unsigned long long)offset + p.n) * (unsigned long long)words <=
                  kSecaggMaxElements,
              "secagg_mask_noise: (offset + n) * words exceeds 2^36 (the "
              "noise stream's ChaCha20 counter would wrap)");
  if (p.n == 0) return;
  SecaggNoiseKey nk{};
  secagg_unpack_key(nk.key, noise_key.data_ptr<uint8_t>());
  const int blocks = (max_blocks > 0 && max_blocks < p.blocks)
                         ? (int)max_blocks
                         : p.blocks;
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_elem<kAnyFloat>(x, bad_dtype, [&](auto tag) {
    using T = decltype(tag);
#define SECAGG_NOISE_CASE(W)                                                  \
  case W:                                                                     \
    hipLaunchKernelGGL((secagg_mask_noise_kernel<T, W>), dim3(blocks),        \
                       dim3(kBlock), 0, stream, elem_ptr<const T>(x), p.out,  \
                       p.n, p.pos.blk0, p.pos.n0, p.pos.n1, p.weight,         \
                       p.scale, p.keys, nk, (uint32_t)step, p.vec_ok);        \
    break;
    switch (words) {
      SECAGG_NOISE_CASE(1)
      SECAGG_NOISE_CASE(2)
      SECAGG_NOISE_CASE(4)
      SECAGG_NOISE_CASE(8)
      SECAGG_NOISE_CASE(16)
    }
#undef SECAGG_NOISE_CASE
  });
}

// Enough blocks for 8 waves per SIMD on 256 CUs; one double per block.
constexpr int kSumsqMaxBlocks = 2048;

torch::Tensor sumsq_async(torch::Tensor x) {
  const char* bad_dtype = "sumsq: unsupported dtype ";
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
              "sumsq: x must be CUDA contiguous");
  TORCH_CHECK(elem_bit(x) & kAnyFloat, bad_dtype, x.dtype());
  auto opts = torch::dtype(torch::kFloat64).device(x.device());
  const unsigned long long n = x.numel();
  if (n == 0) return torch::zeros({1}, opts);
  auto out = torch::empty({1}, opts);
  // one 16-byte load per lane per item; the scalar path just strides more
  const unsigned long long per = 16ull / (unsigned long long)x.element_size();
  const unsigned long long want = ((n + per - 1) / per + kBlock - 1) / kBlock;
  const int blocks = (int)std::min<unsigned long long>(
      (unsigned long long)kSumsqMaxBlocks, want);
  auto partials = torch::empty({(long long)blocks}, opts);
  auto stream = at::hip::getCurrentHIPStream();
  double* pp = partials.data_ptr<double>();
  const bool vec = aligned_to(x.data_ptr(), 16);
  dispatch_elem<kAnyFloat>(x, bad_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(
        (vec ? sumsq_kernel<T, true> : sumsq_kernel<T, false>), dim3(blocks),
        dim3(kBlock), 0, stream, elem_ptr<const T>(x), n, pp);
  });
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(kBlock), 0, stream,
                     static_cast<const double*>(pp), blocks,
                     out.data_ptr<double>());
  return out;
}

template <typename OutT, int EPL>
void secagg_launch_aggregate(OutT* out, const SecaggInputs& ins,
                             unsigned long long n, const SecaggPos& pos,
                             float inv_scale, const SecaggKeys& corr,
                             bool vec_ok, hipStream_t stream) {
  const int blocks = secagg_grid((n + EPL - 1ull) / EPL);
  hipLaunchKernelGGL((secagg_aggregate_kernel<OutT, EPL>), dim3(blocks),
                     dim3(kBlock), 0, stream, out, ins, n, pos.blk0, pos.n0,
                     pos.n1, inv_scale, corr, vec_ok);
}

void secagg_aggregate_async(torch::Tensor out,
                            std::vector<torch::Tensor> inputs,
                            torch::Tensor corr_keys, torch::Tensor corr_signs,
                            uint64_t round, int64_t offset,
                            int64_t frac_bits) {
  const char* bad_dtype = "secagg_aggregate: unsupported out dtype ";
  TORCH_CHECK(!inputs.empty() && inputs.size() <= kMaxInputs,
              "secagg_aggregate: 1..16 inputs");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(),
              "secagg_aggregate: out must be CUDA contiguous");
  secagg_check_keys("secagg_aggregate", corr_keys, corr_signs);
  const unsigned long long n = out.numel();
  secagg_check_range("secagg_aggregate", n, offset, frac_bits);
  TORCH_CHECK(elem_bit(out) & kAnyFloat, bad_dtype, out.dtype());
  SecaggInputs ins;
  ins.k = (int)inputs.size();
  bool vec_ok = aligned_to(out.data_ptr(), 16);
  for (int j = 0; j < ins.k; ++j) {
    TORCH_CHECK(cuda_contiguous(inputs[j], torch::kInt32) &&
                    inputs[j].numel() == (long long)n &&
                    inputs[j].device() == out.device(),
                "secagg_aggregate: input ", j, " mismatch");
    ins.in[j] = inputs[j].data_ptr<int32_t>();
    vec_ok = vec_ok && aligned_to(ins.in[j], 16);
  }
  if (n == 0) return;
  const SecaggPos pos = secagg_pos(round, offset);
  const float inv_scale = 1.0f / (float)(1ull << frac_bits);
  auto stream = at::hip::getCurrentHIPStream();

  // More corrections than one argument block holds: fold all but the last
  // chunk into an int32 ring accumulator, in place after the first launch.
  const int64_t C = corr_keys.size(0);
  int64_t done = 0;
  SecaggKeys corr{};
  torch::Tensor acc;
  while (C - done > kSecaggMaxKeys) {
    secagg_fill_keys(corr, corr_keys, corr_signs, done, kSecaggMaxKeys);
    if (!acc.defined()) {
      acc = torch::empty({(long long)n},
                         torch::dtype(torch::kInt32).device(out.device()));
    }
    secagg_launch_aggregate<int32_t, 16>(
        acc.data_ptr<int32_t>(), ins, n, pos, 0.0f, corr,
        vec_ok && aligned_to(acc.data_ptr(), 16), stream);
    ins.k = 1;
    ins.in[0] = acc.data_ptr<int32_t>();
    vec_ok = aligned_to(out.data_ptr(), 16) && aligned_to(acc.data_ptr(), 16);
    done += kSecaggMaxKeys;
  }
  secagg_fill_keys(corr, corr_keys, corr_signs, done, C - done);
  // Without corrections in the last launch it is the streaming reduce.
  dispatch_elem<kAnyFloat>(out, bad_dtype, [&](auto tag) {
    using T = decltype(tag);
    if (corr.k == 0) {
      secagg_launch_aggregate<T, 4>(elem_ptr<T>(out), ins, n, pos, inv_scale,
                                    corr, vec_ok, stream);
    } else {
      secagg_launch_aggregate<T, 16>(elem_ptr<T>(out), ins, n, pos, inv_scale,
                                     corr, vec_ok, stream);
    }
  });
}
