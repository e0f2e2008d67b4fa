// Channels-last 2-D convolution for the UnivNet spectral discriminator
// (models/vocoder/modules/discriminator.py:450-580 of the reference): six
// valid-padding Conv2d over (frames, frequency) with kernels up to (3, 9), row
// stride 1 and column stride 1 or 2.  Activations are (B, H, W, C) rows.
//
// One geometry (Geo) serves the forward and the data gradient: a stride-sw
// gather with zero padding before the first row / column, writing the output
// columns oc0 + ostep * m.  The forward is (pad 0, ostep 1); the data gradient
// of a stride-sw layer is sw stride-1 launches, one per input-column phase p,
// each over the taps kw = p (mod sw) of the flipped kernel with pad (kh - 1,
// Kp - 1), writing columns p, p + sw, ...: a gather, no atomics.
//
// Kernels:
//   k_sconv_cc<T, RB>   C -> C implicit GEMM on the matrix core (bf16:
//                       v_mfma_f32_32x32x16_bf16, fp32: v_mfma_f32_32x32x2_f32);
//                       the input patch (kh + RB - 1 rows x sw * 63 + kw columns x
//                       32 channels) is staged once per channel chunk in LDS and
//                       re-read by every tap; epilogue from the accumulators.
//   k_sconv_1c<T>       1 -> C streaming VALU kernel on fp32 input, weights in LDS.
//   k_sconv_c1<T>       C -> 1 per-position reduction (4 lanes per position).
//   k_sconv_wg_cc<T>    C -> C weight gradient: per block a contiguous range of
//                       output rows, taps dealt over the 4 waves, positions as
//                       the MFMA reduction axis; fixed-order partials.
//   k_sconv_wg_small    1 -> C and C -> 1 weight gradients (VALU).
//   k_sconv_wg_finish   fixed-order sum of the partials into the torch layout.
#include "conv_common.h"

namespace sel {
namespace sconv {

using conv::bf16x8;
using conv::floatx16;
using conv::from_f;
using conv::to_f;

struct Geo {
  int B, Hi, Wi, Ci;       // input (B, Hi, Wi, Ci)
  int Ho, Wo, Co;          // output tensor (B, Ho, Wo, Co)
  int kh, kw, sw, ph, pw;  // taps, column stride, zero rows / columns before the input
  int oc0, ostep, Wm;      // this launch writes output columns oc0 + ostep * m, m < Wm
  int epi;                 // 0: + bias (when given); 1: + bias, LeakyReLU; 2: * LeakyReLU'(aux)
  float slope;
  // C -> C, bf16 forward: element offset of the weights' second bf16 term (the
  // rounding remainder w - bf16(w)), 0 = none.  With it the forward's
  // pre-activations carry only the rounding of the stored activations, not of
  // the weights too: fewer LeakyReLU masks land on the other side of zero than
  // in the unrounded network, and a flipped mask costs the gradient far more
  // (a factor 1 against 0.2 on that unit) than the rounding that caused it.
  int wlo;
};

constexpr int BM = 64;  // output columns per block of the matrix-core kernels

// LDS row pitch (elements) of a 32-channel chunk and elements per 16 bytes.
// bf16: 72-byte rows (18 banks): the 8-byte operand reads of the 32 positions of
// a half-wave and the 2-byte transposed reads of the weight gradient fall in
// distinct banks at both column strides.  fp32: 33 dwords.
template <typename T> struct Elt;
template <> struct Elt<__bf16> { static constexpr int P = 36, VEC = 8; };
template <> struct Elt<float> { static constexpr int P = 33, VEC = 4; };

__device__ __forceinline__ float leaky(float v, float s) { return v > 0.f ? v : v * s; }
__device__ __forceinline__ float leaky_grad(float y, float s) { return y > 0.f ? 1.f : s; }

template <typename T>
__device__ __forceinline__ void lds_put16(T* dst, uint4 val) {
  if constexpr (sizeof(T) == 2) {
    reinterpret_cast<uint2*>(dst)[0] = make_uint2(val.x, val.y);
    reinterpret_cast<uint2*>(dst)[1] = make_uint2(val.z, val.w);
  } else {
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    d[0] = val.x, d[1] = val.y, d[2] = val.z, d[3] = val.w;
  }
}

// rows x NC columns x 32 channels [cc, cc + 32) of sample b from input row hin0 /
// column win0 on; positions outside the input are zeros
template <typename T, int NT>
__device__ __forceinline__ void stage_patch(T* xs, const T* __restrict__ x, const Geo& g, int b, int hin0, int win0,
                                            int rows, int NC, int cc) {
  constexpr int P = Elt<T>::P, VEC = Elt<T>::VEC, VPR = 32 / VEC;
  for (int idx = threadIdx.x; idx < rows * NC * VPR; idx += NT) {
    const int v = idx % VPR, ci = (idx / VPR) % NC, rr = idx / (VPR * NC);
    const int hi = hin0 + rr, wi = win0 + ci;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (hi >= 0 && hi < g.Hi && wi >= 0 && wi < g.Wi)
      val = *reinterpret_cast<const uint4*>(x + ((int64_t(b) * g.Hi + hi) * g.Wi + wi) * g.Ci + cc + v * VEC);
    lds_put16<T>(xs + (rr * NC + ci) * P + v * VEC, val);
  }
}

__device__ __forceinline__ bf16x8 lds_get8(const __bf16* p) {
  const uint2 a = reinterpret_cast<const uint2*>(p)[0], b = reinterpret_cast<const uint2*>(p)[1];
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

// ---------------------------------------------------------------------------
// C -> C.  Block = RB output rows x 64 output columns x 32 output channels
// (blockIdx.y); wave (rw, cw) owns row rw, columns 32 cw ... 32 cw + 31.
// Operands swapped (weights as A, positions as B): a lane holds position
// lane & 31 and channels (e & 3) + 8 (e >> 2) + 4 (lane >> 5).
// ---------------------------------------------------------------------------
template <typename T, int RB>
__global__ __launch_bounds__(RB * 128) void k_sconv_cc(Geo g, const T* __restrict__ x, const T* __restrict__ wp,
                                                       const float* __restrict__ bias, const T* __restrict__ aux,
                                                       T* __restrict__ out) {
  constexpr int P = Elt<T>::P, NT = RB * 128;
  extern __shared__ __align__(16) unsigned char smem[];
  T* const xs = reinterpret_cast<T*>(smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rw = wave >> 1, cw = wave & 1, half = lane >> 5, r = lane & 31;
  const int mt = (g.Wm + BM - 1) / BM, ht = (g.Ho + RB - 1) / RB;
  int bid = blockIdx.x;
  const int m0 = (bid % mt) * BM;
  bid /= mt;
  const int h0 = (bid % ht) * RB;
  const int b = bid / ht;
  const int n0 = blockIdx.y * 32;
  const int NC = g.sw * (BM - 1) + g.kw, rows = g.kh + RB - 1;
  const int mloc = cw * 32 + r;

  floatx16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  for (int cc = 0; cc < g.Ci; cc += 32) {
    __syncthreads();
    stage_patch<T, NT>(xs, x, g, b, h0 - g.ph, g.sw * m0 - g.pw, rows, NC, cc);
    __syncthreads();
    for (int i = 0; i < g.kh; ++i) {
      for (int j = 0; j < g.kw; ++j) {
        const T* wrow = wp + (int64_t(i * g.kw + j) * g.Co + n0 + r) * g.Ci + cc;
        const T* xrow = xs + ((rw + i) * NC + g.sw * mloc + j) * P;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int co = 16 * ks + 8 * half;
            const bf16x8 bw = *reinterpret_cast<const bf16x8*>(wrow + co);
            const bf16x8 af = lds_get8(xrow + co);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, af, acc, 0, 0, 0);
            if (g.wlo) {
              const bf16x8 bl = *reinterpret_cast<const bf16x8*>(wrow + g.wlo + co);
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, af, acc, 0, 0, 0);
            }
          }
        } else {
#pragma unroll 4
          for (int c2 = 0; c2 < 32; c2 += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[c2 + half], xrow[c2 + half], acc, 0, 0, 0);
        }
      }
    }
  }

  const int m = m0 + mloc, h = h0 + rw;
  if (m >= g.Wm || h >= g.Ho) return;
  const int64_t o = ((int64_t(b) * g.Ho + h) * g.Wo + g.oc0 + g.ostep * m) * g.Co;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + 8 * q + 4 * half;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = acc[4 * q + e];
      if (g.epi != 2 && bias) v[e] += bias[n + e];
      if (g.epi == 1) v[e] = leaky(v[e], g.slope);
      if (g.epi == 2) v[e] *= leaky_grad(to_f(aux[o + n + e]), g.slope);
    }
    if constexpr (sizeof(T) == 2) {
      typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
      const bf16x4 ov = {__bf16(v[0]), __bf16(v[1]), __bf16(v[2]), __bf16(v[3])};
      *reinterpret_cast<bf16x4*>(out + o + n) = ov;
    } else {
      *reinterpret_cast<float4*>(out + o + n) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ---------------------------------------------------------------------------
// 1 -> C: one thread per (position, 8 channels), fp32 input read directly,
// weights wk[tap][C] (fp32) in LDS.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_sconv_1c(Geo g, const float* __restrict__ x, const float* __restrict__ wk,
                                                  const float* __restrict__ bias, const T* __restrict__ aux,
                                                  T* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* const ws = reinterpret_cast<float*>(smem);
  const int ntap = g.kh * g.kw, C = g.Co;
  for (int i = threadIdx.x; i < ntap * C; i += 256) ws[i] = wk[i];
  __syncthreads();
  const int cgs = C / 8;
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int cg = int(idx % cgs);
  int64_t pos = idx / cgs;
  if (pos >= int64_t(g.B) * g.Ho * g.Wm) return;
  const int m = int(pos % g.Wm);
  pos /= g.Wm;
  const int h = int(pos % g.Ho), b = int(pos / g.Ho);
  float a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = 0.f;
  for (int i = 0; i < g.kh; ++i) {
    const int hi = h + i - g.ph;
    if (hi < 0 || hi >= g.Hi) continue;
    const float* xr = x + (int64_t(b) * g.Hi + hi) * g.Wi;
    for (int j = 0; j < g.kw; ++j) {
      const int wi = g.sw * m + j - g.pw;
      if (wi < 0 || wi >= g.Wi) continue;
      const float xv = xr[wi];
      const float4 w0 = *reinterpret_cast<const float4*>(ws + (i * g.kw + j) * C + cg * 8);
      const float4 w1 = *reinterpret_cast<const float4*>(ws + (i * g.kw + j) * C + cg * 8 + 4);
      a[0] += xv * w0.x, a[1] += xv * w0.y, a[2] += xv * w0.z, a[3] += xv * w0.w;
      a[4] += xv * w1.x, a[5] += xv * w1.y, a[6] += xv * w1.z, a[7] += xv * w1.w;
    }
  }
  const int64_t o = ((int64_t(b) * g.Ho + h) * g.Wo + g.oc0 + g.ostep * m) * C + cg * 8;
  alignas(16) T av[8];
  if (g.epi == 2) {
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<uint4*>(av) = *reinterpret_cast<const uint4*>(aux + o);
    } else {
      *reinterpret_cast<float4*>(av) = *reinterpret_cast<const float4*>(aux + o);
      *reinterpret_cast<float4*>(av + 4) = *reinterpret_cast<const float4*>(aux + o + 4);
    }
  }
  alignas(16) T ov[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v = a[e];
    if (g.epi != 2 && bias) v += bias[cg * 8 + e];
    if (g.epi == 1) v = leaky(v, g.slope);
    if (g.epi == 2) v *= leaky_grad(to_f(av[e]), g.slope);
    ov[e] = from_f<T>(v);
  }
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<const uint4*>(ov);
  } else {
    *reinterpret_cast<float4*>(out + o) = *reinterpret_cast<const float4*>(ov);
    *reinterpret_cast<float4*>(out + o + 4) = *reinterpret_cast<const float4*>(ov + 4);
  }
}

// ---------------------------------------------------------------------------
// C -> 1: 4 lanes per output position, each over the 8-channel vectors
// l, l + 4, ... of every tap; fp32 output (+ bias[0] when given).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_sconv_c1(Geo g, const T* __restrict__ x, const float* __restrict__ wk,
                                                  const float* __restrict__ bias, float* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* const ws = reinterpret_cast<float*>(smem);
  const int ntap = g.kh * g.kw, C = g.Ci;
  for (int i = threadIdx.x; i < ntap * C; i += 256) ws[i] = wk[i];
  __syncthreads();
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int l = int(idx & 3);
  int64_t pos = idx >> 2;
  const bool live = pos < int64_t(g.B) * g.Ho * g.Wm;  // (the 4 lanes of a position agree)
  if (!live) pos = 0;
  const int m = int(pos % g.Wm);
  pos /= g.Wm;
  const int h = int(pos % g.Ho), b = int(pos / g.Ho);
  float a = 0.f;
  for (int i = 0; i < g.kh; ++i) {
    const int hi = h + i - g.ph;
    if (hi < 0 || hi >= g.Hi) continue;
    for (int j = 0; j < g.kw; ++j) {
      const int wi = g.sw * m + j - g.pw;
      if (wi < 0 || wi >= g.Wi) continue;
      const T* xp = x + ((int64_t(b) * g.Hi + hi) * g.Wi + wi) * C;
      const float* wt = ws + (i * g.kw + j) * C;
      for (int c = l * 8; c < C; c += 32) {
        alignas(16) T xv[8];
        if constexpr (sizeof(T) == 2) {
          *reinterpret_cast<uint4*>(xv) = *reinterpret_cast<const uint4*>(xp + c);
        } else {
          *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(xp + c);
          *reinterpret_cast<float4*>(xv + 4) = *reinterpret_cast<const float4*>(xp + c + 4);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) a += to_f(xv[e]) * wt[c + e];
      }
    }
  }
  a += __shfl_xor(a, 1, 64);
  a += __shfl_xor(a, 2, 64);
  if (live && l == 0) {
    if (bias) a += bias[0];
    out[(int64_t(b) * g.Ho + h) * g.Wo + g.oc0 + g.ostep * m] = a;
  }
}

// ---------------------------------------------------------------------------
// C -> C weight gradient.  Block (s, cy): output rows [R s / nsplit, R (s + 1) /
// nsplit) of the R = B * Ho rows, one 32 x 32 (input, output) channel block.
// Wave w holds the taps w, w + 4, ... (<= 7 accumulators); the positions of a
// 64-column tile are the MFMA reduction axis: A[c][pos] = x, B[pos][n] = gy,
// both read transposed from the [position][channel] LDS images.
//   part[((s * ntap + tap) * Ci + c) * Co + n],  bpart[s * Co + n]
// ---------------------------------------------------------------------------
constexpr int WG_TAPS = 7;

template <typename T>
__global__ __launch_bounds__(256) void k_sconv_wg_cc(Geo g, const T* __restrict__ x, const T* __restrict__ gy,
                                                     float* __restrict__ part, float* __restrict__ bpart,
                                                     int nsplit) {
  constexpr int P = Elt<T>::P, VEC = Elt<T>::VEC, VPR = 32 / VEC;
  extern __shared__ __align__(16) unsigned char smem[];
  T* const xs = reinterpret_cast<T*>(smem);
  const int NC = g.sw * (BM - 1) + g.kw;
  T* const gs = xs + g.kh * NC * P;  // [64][P]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int s = blockIdx.x, ncb = g.Ci / 32;
  const int c0 = (blockIdx.y % ncb) * 32, n0 = (blockIdx.y / ncb) * 32;
  const int64_t R = int64_t(g.B) * g.Ho;
  const int64_t r_lo = R * s / nsplit, r_hi = R * (s + 1) / nsplit;
  const int ntap = g.kh * g.kw;

  floatx16 acc[WG_TAPS];
  int toff[WG_TAPS];
#pragma unroll
  for (int q = 0; q < WG_TAPS; ++q) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
    const int t = wave + 4 * q;
    toff[q] = t < ntap ? ((t / g.kw) * NC + t % g.kw) * P : 0;
  }
  float bsum = 0.f;

  for (int64_t rr = r_lo; rr < r_hi; ++rr) {
    const int b = int(rr / g.Ho), h = int(rr % g.Ho);
    for (int m0 = 0; m0 < g.Wo; m0 += BM) {
      __syncthreads();
      stage_patch<T, 256>(xs, x, g, b, h, g.sw * m0, g.kh, NC, c0);
      for (int idx = tid; idx < BM * VPR; idx += 256) {
        const int v = idx % VPR, p = idx / VPR;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (m0 + p < g.Wo)
          val = *reinterpret_cast<const uint4*>(gy + ((int64_t(b) * g.Ho + h) * g.Wo + m0 + p) * g.Co + n0 + v * VEC);
        lds_put16<T>(gs + p * P + v * VEC, val);
      }
      __syncthreads();
      if (c0 == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) bsum += to_f(gs[((tid >> 5) * 8 + q) * P + r]);
      }
      if constexpr (sizeof(T) == 2) {
        for (int ks = 0; ks < BM / 16; ++ks) {
          const int p0 = 16 * ks + 8 * half;
          bf16x8 bg;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) bg[jj] = gs[(p0 + jj) * P + r];
#pragma unroll
          for (int q = 0; q < WG_TAPS; ++q) {
            if (wave + 4 * q < ntap) {
              bf16x8 ax;
#pragma unroll
              for (int jj = 0; jj < 8; ++jj) ax[jj] = xs[toff[q] + g.sw * (p0 + jj) * P + r];
              acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ax, bg, acc[q], 0, 0, 0);
            }
          }
        }
      } else {
        for (int kk = 0; kk < BM; kk += 2) {
          const int p = kk + half;
          const float bg = gs[p * P + r];
#pragma unroll
          for (int q = 0; q < WG_TAPS; ++q) {
            if (wave + 4 * q < ntap)
              acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[toff[q] + g.sw * p * P + r], bg, acc[q], 0, 0, 0);
          }
        }
      }
    }
  }

  // D[row = c][col = n]: lane -> n = lane & 31, element e -> c = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int q = 0; q < WG_TAPS; ++q) {
    const int t = wave + 4 * q;
    if (t >= ntap) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = c0 + (e & 3) + 8 * (e >> 2) + 4 * half;
      part[((int64_t(s) * ntap + t) * g.Ci + c) * g.Co + n0 + r] = acc[q][e];
    }
  }
  if (c0 == 0) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [8][32]
    red[tid] = bsum;
    __syncthreads();
    if (tid < 32) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) v += red[q * 32 + tid];
      bpart[int64_t(s) * g.Co + n0 + tid] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// 1 -> C (FIRST: sc = the fp32 input, vec = gy) and C -> 1 (sc = the fp32 gy,
// vec = x) weight gradients: thread (c = tid & 31, taps tid >> 5, + 8, ...).
// Partials in the [tap][Ci][Co] order of k_sconv_wg_finish.
// ---------------------------------------------------------------------------
template <typename T, bool FIRST>
__global__ __launch_bounds__(256) void k_sconv_wg_small(Geo g, const float* __restrict__ sc,
                                                        const T* __restrict__ vec, float* __restrict__ part,
                                                        float* __restrict__ bpart, int nsplit) {
  const int tid = threadIdx.x, tg = tid >> 5;
  const int C = FIRST ? g.Co : g.Ci;
  const int c = blockIdx.y * 32 + (tid & 31);
  const int s = blockIdx.x, ntap = g.kh * g.kw;
  const int64_t R = int64_t(g.B) * g.Ho;
  const int64_t r_lo = R * s / nsplit, r_hi = R * (s + 1) / nsplit;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int ti[4], tj[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tg + 8 * q;
    ti[q] = t < ntap ? t / g.kw : 0;
    tj[q] = t < ntap ? t % g.kw : 0;
  }
  float bs = 0.f;
  for (int64_t rr = r_lo; rr < r_hi; ++rr) {
    const int b = int(rr / g.Ho), h = int(rr % g.Ho);
    for (int m = 0; m < g.Wo; ++m) {
      const int64_t po = (int64_t(b) * g.Ho + h) * g.Wo + m;
      if constexpr (FIRST) {
        const float v = to_f(vec[po * C + c]);
        bs += v;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[q] += sc[(int64_t(b) * g.Hi + h + ti[q]) * g.Wi + g.sw * m + tj[q]] * v;
      } else {
        const float sv = sc[po];
        bs += sv;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          acc[q] += sv * to_f(vec[((int64_t(b) * g.Hi + h + ti[q]) * g.Wi + g.sw * m + tj[q]) * C + c]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tg + 8 * q;
    if (t < ntap) part[(int64_t(s) * ntap + t) * C + c] = acc[q];
  }
  if (FIRST) {
    if (tg == 0) bpart[int64_t(s) * C + c] = bs;
  } else if (tid == 0 && blockIdx.y == 0) {
    bpart[s] = bs;
  }
}

// gw[n][c][tap] (the torch layout (Cout, Cin, kh, kw)) and gb[n]: sums over the
// splits in index order
__global__ __launch_bounds__(256) void k_sconv_wg_finish(const float* __restrict__ part,
                                                         const float* __restrict__ bpart, int nsplit, int ntap,
                                                         int Ci, int Co, float* __restrict__ gw,
                                                         float* __restrict__ gb) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int tot = ntap * Ci * Co;
  if (idx < tot) {
    float v = 0.f;
    for (int s = 0; s < nsplit; ++s) v += part[int64_t(s) * tot + idx];
    const int t = idx / (Ci * Co), c = (idx / Co) % Ci, n = idx % Co;
    gw[(int64_t(n) * Ci + c) * ntap + t] = v;
  } else if (idx < tot + Co && gb) {
    const int n = idx - tot;
    float v = 0.f;
    for (int s = 0; s < nsplit; ++s) v += bpart[int64_t(s) * Co + n];
    gb[n] = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int check(const sel_sconv_desc* d) {
  SEL_REQUIRE(d, SEL_ERR_ARG, "sconv: null descriptor");
  SEL_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, SEL_ERR_ARG, "sconv: empty shape");
  SEL_REQUIRE(d->kh >= 1 && d->kh <= 3, SEL_ERR_ARG, "sconv: kernel height %d outside the limit kh <= 3", d->kh);
  SEL_REQUIRE(d->kw >= 1 && d->kw <= 9, SEL_ERR_ARG, "sconv: kernel width %d outside the limit kw <= 9", d->kw);
  SEL_REQUIRE(d->sh == 1, SEL_ERR_ARG, "sconv: frame-axis stride %d outside the limit sh = 1", d->sh);
  SEL_REQUIRE(d->sw == 1 || d->sw == 2, SEL_ERR_ARG, "sconv: frequency-axis stride %d outside the limit sw in {1, 2}",
              d->sw);
  SEL_REQUIRE(d->kw >= d->sw, SEL_ERR_ARG, "sconv: kernel width %d below the stride %d", d->kw, d->sw);
  const bool first = d->Cin == 1 && d->Cout % 32 == 0;
  const bool mid = d->Cin % 32 == 0 && d->Cout % 32 == 0;
  const bool last = d->Cin % 32 == 0 && d->Cout == 1;
  SEL_REQUIRE(first || mid || last, SEL_ERR_ARG,
              "sconv: channels %d -> %d outside the limit 1 -> C, C -> C, C -> 1 with C %% 32 == 0", d->Cin, d->Cout);
  SEL_REQUIRE(d->Cin <= 256 && d->Cout <= 256, SEL_ERR_ARG, "sconv: channels %d -> %d outside the limit C <= 256",
              d->Cin, d->Cout);
  SEL_REQUIRE(d->H >= d->kh && d->W >= d->kw, SEL_ERR_ARG, "sconv: input %d x %d smaller than the kernel %d x %d",
              d->H, d->W, d->kh, d->kw);
  const int cm = d->Cin > d->Cout ? d->Cin : d->Cout;
  SEL_REQUIRE(int64_t(d->B) * d->H * d->W * cm < (int64_t(1) << 40) && int64_t(d->B) * d->H * d->W < (int64_t(1) << 31),
              SEL_ERR_ARG, "sconv: tensor too large");
  return SEL_OK;
}

static inline int ho_of(const sel_sconv_desc* d) { return d->H - d->kh + 1; }
static inline int wo_of(const sel_sconv_desc* d) { return (d->W - d->kw) / d->sw + 1; }

template <typename T>
static size_t cc_lds(const Geo& g, int RB) {
  return size_t(g.kh + RB - 1) * (g.sw * (BM - 1) + g.kw) * Elt<T>::P * sizeof(T);
}

// one launch of the generic gather; x / out element types follow the channel form
template <typename T>
static int launch(const Geo& g, const void* x, const void* w, const float* bias, const void* aux, void* out,
                  hipStream_t s) {
  const int64_t npos = int64_t(g.B) * g.Ho * g.Wm;
  if (npos <= 0) return SEL_OK;
  if (g.Ci == 1) {
    const int64_t nthr = npos * (g.Co / 8);
    hipLaunchKernelGGL(k_sconv_1c<T>, dim3(unsigned((nthr + 255) / 256)), dim3(256),
                       size_t(g.kh) * g.kw * g.Co * sizeof(float), s, g, static_cast<const float*>(x),
                       static_cast<const float*>(w), bias, static_cast<const T*>(aux), static_cast<T*>(out));
  } else if (g.Co == 1) {
    hipLaunchKernelGGL(k_sconv_c1<T>, dim3(unsigned((npos * 4 + 255) / 256)), dim3(256),
                       size_t(g.kh) * g.kw * g.Ci * sizeof(float), s, g, static_cast<const T*>(x),
                       static_cast<const float*>(w), bias, static_cast<float*>(out));
  } else {
    constexpr int RB = sizeof(T) == 2 ? 2 : 1;
    const int64_t nblk = int64_t(g.B) * ((g.Ho + RB - 1) / RB) * ((g.Wm + BM - 1) / BM);
    hipLaunchKernelGGL((k_sconv_cc<T, RB>), dim3(unsigned(nblk), g.Co / 32), dim3(RB * 128), cc_lds<T>(g, RB), s, g,
                       static_cast<const T*>(x), static_cast<const T*>(w), bias, static_cast<const T*>(aux),
                       static_cast<T*>(out));
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

static int launch_dt(int dtype, const Geo& g, const void* x, const void* w, const float* bias, const void* aux,
                     void* out, hipStream_t s) {
  return dtype == SEL_BF16 ? launch<__bf16>(g, x, w, bias, aux, out, s) : launch<float>(g, x, w, bias, aux, out, s);
}

static int wg_splits(const sel_sconv_desc* d) {
  const int64_t R = int64_t(d->B) * ho_of(d);
  const int cap = (d->Cin == 1 || d->Cout == 1) ? 1024 : 128;
  return int(R < cap ? R : cap);
}

}  // namespace sconv
}  // namespace sel

using namespace sel::sconv;

extern "C" {

int sel_sconv_check(const sel_sconv_desc* d) { return check(d); }

int sel_sconv_fwd(const sel_sconv_desc* d, int dtype, const void* x, const void* wpack, const float* bias, void* y,
                  sel_stream_t stream) {
  if (int rc = check(d)) return rc;
  SEL_REQUIRE(x && wpack && y && (dtype == SEL_F32 || dtype == SEL_BF16), SEL_ERR_ARG, "sconv_fwd: bad arguments");
  Geo g{d->B, d->H, d->W, d->Cin, ho_of(d), wo_of(d), d->Cout, d->kh, d->kw, d->sw, 0, 0, 0, 1, wo_of(d),
        d->act ? 1 : 0, d->slope,
        (dtype == SEL_BF16 && d->Cin > 1 && d->Cout > 1) ? d->kh * d->kw * d->Cin * d->Cout : 0};
  return launch_dt(dtype, g, x, wpack, bias, nullptr, y, reinterpret_cast<hipStream_t>(stream));
}

int sel_sconv_bwd_data(const sel_sconv_desc* d, int dtype, const void* gy, const void* wadj, const void* aux,
                       void* gx, sel_stream_t stream) {
  if (int rc = check(d)) return rc;
  SEL_REQUIRE(gy && wadj && gx && (dtype == SEL_F32 || dtype == SEL_BF16), SEL_ERR_ARG, "sconv_bwd_data: bad arguments");
  SEL_REQUIRE(!(aux && d->Cin == 1), SEL_ERR_ARG, "sconv_bwd_data: the 1-channel input has no activation");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t esz = (d->Cin == 1 || d->Cout == 1 || dtype == SEL_F32) ? 4 : 2;  // packed adjoint element
  size_t woff = 0;
  for (int p = 0; p < d->sw; ++p) {
    const int Kp = (d->kw - p + d->sw - 1) / d->sw;
    const int Wm = (d->W - p + d->sw - 1) / d->sw;
    Geo g{d->B, ho_of(d), wo_of(d), d->Cout, d->H, d->W, d->Cin, d->kh, Kp, 1, d->kh - 1, Kp - 1, p, d->sw, Wm,
          aux ? 2 : 0, d->slope, 0};
    if (int rc = launch_dt(dtype, g, gy, static_cast<const char*>(wadj) + woff, nullptr, aux, gx, s)) return rc;
    woff += size_t(d->kh) * Kp * d->Cin * d->Cout * esz;
  }
  return SEL_OK;
}

size_t sel_sconv_wgrad_workspace(const sel_sconv_desc* d, int dtype) {
  (void)dtype;
  if (check(d)) return 0;
  return size_t(wg_splits(d)) * (size_t(d->kh) * d->kw * d->Cin * d->Cout + d->Cout) * sizeof(float);
}

int sel_sconv_wgrad(const sel_sconv_desc* d, int dtype, const void* gy, const void* x, float* gw, float* gb, void* ws,
                    size_t ws_bytes, sel_stream_t stream) {
  if (int rc = check(d)) return rc;
  SEL_REQUIRE(gy && x && gw && ws && (dtype == SEL_F32 || dtype == SEL_BF16), SEL_ERR_ARG, "sconv_wgrad: bad arguments");
  SEL_REQUIRE(ws_bytes >= sel_sconv_wgrad_workspace(d, dtype), SEL_ERR_WORKSPACE, "sconv_wgrad: workspace too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nsplit = wg_splits(d), ntap = d->kh * d->kw;
  float* part = static_cast<float*>(ws);
  float* bpart = part + size_t(nsplit) * ntap * d->Cin * d->Cout;
  Geo g{d->B, d->H, d->W, d->Cin, ho_of(d), wo_of(d), d->Cout, d->kh, d->kw, d->sw, 0, 0, 0, 1, wo_of(d), 0, d->slope, 0};
  const bool bf = dtype == SEL_BF16;
  if (d->Cin == 1) {
    if (bf)
      hipLaunchKernelGGL((k_sconv_wg_small<__bf16, true>), dim3(nsplit, d->Cout / 32), dim3(256), 0, s, g,
                         static_cast<const float*>(x), static_cast<const __bf16*>(gy), part, bpart, nsplit);
    else
      hipLaunchKernelGGL((k_sconv_wg_small<float, true>), dim3(nsplit, d->Cout / 32), dim3(256), 0, s, g,
                         static_cast<const float*>(x), static_cast<const float*>(gy), part, bpart, nsplit);
  } else if (d->Cout == 1) {
    if (bf)
      hipLaunchKernelGGL((k_sconv_wg_small<__bf16, false>), dim3(nsplit, d->Cin / 32), dim3(256), 0, s, g,
                         static_cast<const float*>(gy), static_cast<const __bf16*>(x), part, bpart, nsplit);
    else
      hipLaunchKernelGGL((k_sconv_wg_small<float, false>), dim3(nsplit, d->Cin / 32), dim3(256), 0, s, g,
                         static_cast<const float*>(gy), static_cast<const float*>(x), part, bpart, nsplit);
  } else {
    const dim3 grid(nsplit, (d->Cin / 32) * (d->Cout / 32));
    const int NC = d->sw * (BM - 1) + d->kw;
    if (bf)
      hipLaunchKernelGGL(k_sconv_wg_cc<__bf16>, grid, dim3(256), size_t(d->kh * NC + BM) * Elt<__bf16>::P * 2, s, g,
                         static_cast<const __bf16*>(x), static_cast<const __bf16*>(gy), part, bpart, nsplit);
    else
      hipLaunchKernelGGL(k_sconv_wg_cc<float>, grid, dim3(256), size_t(d->kh * NC + BM) * Elt<float>::P * 4, s, g,
                         static_cast<const float*>(x), static_cast<const float*>(gy), part, bpart, nsplit);
  }
  SEL_LAUNCH_CHECK();
  const int tot = ntap * d->Cin * d->Cout + d->Cout;
  hipLaunchKernelGGL(k_sconv_wg_finish, dim3((tot + 255) / 256), dim3(256), 0, s, part, bpart, nsplit, ntap, d->Cin,
                     d->Cout, gw, gb);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
