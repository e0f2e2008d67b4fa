// Device code that more than one of the conv kernel files (conv.hip,
// conv_ru.hip, conv_wgrad.hip) uses; only those three include it, and
// dconv_wgrad.hip for tr_read / tr_frag.  What a single file uses stays in
// that file.
#pragma once
#include "conv_common.h"

namespace sel {
namespace conv {

// Staged tiles of the generic kernels (k_conv_fwd, k_conv_wgrad).
constexpr int CK = 32;  // channels per reduction chunk

template <typename T> struct Pitch;
template <> struct Pitch<float> { static constexpr int v = 36; };   // 144 B rows: conflict-free b128
template <> struct Pitch<__bf16> { static constexpr int v = 40; };  // 80 B rows: conflict-free b128

// Flat input row for (output row m, tap k) or -1 (zero).
__device__ __forceinline__ int64_t in_row(const Args& a, int64_t m, int k) {
  const int64_t b = m / a.T;
  const int t = int(m - b * a.T);
  int ti = t + k * a.dil - a.pad;
  if (ti < 0 || ti >= a.T) {
    if (a.pad_mode == SEL_PAD_ZERO) return -1;
    ti = ti < 0 ? 0 : a.T - 1;
  }
  return b * a.T + ti;
}

// Stage `nrows` input rows starting at flat row g0 (channels [c0, c0+CK)) into LDS.
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ in, const Args& a, int64_t g0, int nrows,
                                           int c0, T* __restrict__ xs, bool elu_on) {
  constexpr int P = Pitch<T>::v;
  constexpr int VEC = 16 / sizeof(T);  // elements per 16-B load
  constexpr int PER_ROW = CK / VEC;
  const bool vec_ok = (a.C % VEC == 0) && (c0 + CK <= a.C);
  for (int idx = threadIdx.x; idx < nrows * PER_ROW; idx += blockDim.x) {
    const int r = idx / PER_ROW, v = idx % PER_ROW;
    const int64_t g = g0 + r;
    const int c = c0 + v * VEC;
    T vals[VEC];
    if (g >= 0 && g < a.rows && vec_ok) {
      const uint4 raw = *reinterpret_cast<const uint4*>(in + g * a.C + c);
      *reinterpret_cast<uint4*>(vals) = raw;
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        vals[e] = (g >= 0 && g < a.rows && c + e < a.C) ? in[g * a.C + c + e] : from_f<T>(0.f);
    }
    if (elu_on) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) vals[e] = from_f<T>(elu(to_f(vals[e])));
    }
    *reinterpret_cast<uint4*>(xs + r * P + v * VEC) = *reinterpret_cast<uint4*>(vals);
  }
}

// Stage packed weights Wp[n][k][c] for n in [n0, n0+BN), one tap, channels chunk.
template <typename T, int BN>
__device__ __forceinline__ void stage_w(const T* __restrict__ wp, const Args& a, int n0, int k, int c0,
                                        T* __restrict__ ws) {
  constexpr int P = Pitch<T>::v;
  constexpr int VEC = 16 / sizeof(T);
  constexpr int PER_ROW = CK / VEC;
  const bool vec_ok = (a.C % VEC == 0) && (c0 + CK <= a.C);
  for (int idx = threadIdx.x; idx < BN * PER_ROW; idx += blockDim.x) {
    const int r = idx / PER_ROW, v = idx % PER_ROW;
    const int n = n0 + r;
    const int c = c0 + v * VEC;
    T vals[VEC];
    const int64_t base = (int64_t(n) * a.K + k) * a.C + c;
    if (n < a.N && vec_ok) {
      *reinterpret_cast<uint4*>(vals) = *reinterpret_cast<const uint4*>(wp + base);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) vals[e] = (n < a.N && c + e < a.C) ? wp[base + e] : from_f<T>(0.f);
    }
    *reinterpret_cast<uint4*>(ws + r * P + v * VEC) = *reinterpret_cast<uint4*>(vals);
  }
}

// acc += A(16 rows from xs) * B(16 cols from ws) over one 32-channel chunk.
__device__ __forceinline__ void mma_chunk(floatx4& acc, const float* xs_row, const float* ws_row, int lane,
                                          bool valid) {
  // lane: row/col = lane & 15, channel group 4*(lane >> 4) (+16)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 16 * h + 4 * (lane >> 4);
    float4 av = *reinterpret_cast<const float4*>(xs_row + c);
    const float4 bv = *reinterpret_cast<const float4*>(ws_row + c);
    if (!valid) av = make_float4(0.f, 0.f, 0.f, 0.f);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
  }
}
__device__ __forceinline__ void mma_chunk(floatx4& acc, const __bf16* xs_row, const __bf16* ws_row,
                                          int lane, bool valid) {
  const int c = 8 * (lane >> 4);
  bf16x8 av = *reinterpret_cast<const bf16x8*>(xs_row + c);
  const bf16x8 bv = *reinterpret_cast<const bf16x8*>(ws_row + c);
  if (!valid) av = bf16x8{};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
}

// v or zeros, component-wise (a ternary on the float4 struct makes hipcc select
// between two ADDRESSES: both operands go to scratch memory)
__device__ __forceinline__ float4 keep4(bool ok, const float4& v) {
  return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}

constexpr int F4_P = 40;  // staged row pitch (bf16 elements) = 80 B

// Tile geometry of the weight-stationary thin kernel (k_conv_thin_bf16 in
// conv.hip, described there); k_ru_thin_bf16 runs its conv1 on the same tiles.
template <int C, int N, int K, int R, bool E = false>
struct Thin {
  static constexpr int PLANES = C / 32;
  // NS output slices of 32 channels, RG row groups; at N = 96 the fourth
  // wave has no slice (it stages and runs the epilogue only)
  static constexpr int NS = N / 32, RG = 4 / NS;
  static constexpr int WR = R / RG, TM = WR / 32;
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int CV = C / 8;  // 16-B vectors per staged row
  static constexpr int XV = (SPAN * CV + 255) / 256;
  static constexpr int OP = N + 4;  // fp32 out-tile pitch (conflict-free b128)
  static constexpr size_t LDS_STAGE = size_t(PLANES) * SPAN * F4_P * 2;
  static constexpr size_t LDS_OUT = size_t(R) * OP * 4;
  static constexpr size_t LDS = LDS_STAGE > LDS_OUT ? LDS_STAGE : LDS_OUT;
  // E: epilogue-operand prefetch, EJ 16-B vectors per lane and operand held
  // in VGPRs across the MFMA phase (costs up to 8*EJ VGPRs, i.e. occupancy on
  // some instances: chosen per instance, kThinEpfDefault), plus the split
  // tile loop (separate staging and out tiles in LDS) where both fit in 64 KB
  static constexpr int EJ = (R * (N / 8) + 255) / 256;
  static constexpr bool EPF = E && EJ <= 8;
  static constexpr bool SPLIT = EPF && LDS_STAGE + LDS_OUT <= 64 * 1024;
  static constexpr size_t LDS_TOTAL = SPLIT ? LDS_STAGE + LDS_OUT : LDS;
  static_assert(N == 32 || N == 64 || N == 96 || N == 128, "thin kernel: N in {32, 64, 96, 128}");
  static_assert(C % 32 == 0 && WR % 32 == 0, "thin kernel tiling");
  static_assert(LDS <= 64 * 1024, "thin kernel LDS");
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// branch-free output store into a buffer resource (ru_rsrc): a row outside the
// tile's valid rows takes RU_OOB and is dropped by the hardware.  Every wave
// then issues the same number of stores per tile, so the compiler counts the
// next tile's prefetch exactly (a conditional store made the staging wait at
// the top of the next tile fall back to vmcnt(0), i.e. wait for these stores'
// completion too).
// AUX: the store's cache policy (2 = nt, streaming).
template <int AUX = 0>
__device__ __forceinline__ void ru_bstore(__amdgpu_buffer_rsrc_t rs, int byte_off, bf16x8 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, byte_off, 0, AUX);
}

// Single-input-channel kernels (k_conv_c1, k_wgrad_c1): shape limits, and the
// input activation.
constexpr int C1_NMAX = 64;
constexpr int C1_KMAX = 8;
constexpr int C1_HALO = 64;   // max (K-1)*dil
// TI = float (the reference-precision path): exact expm1 / exp in the ELU and
// ELU' (the bf16 build rounds its result to bf16 and uses the hardware exp)
template <typename TI>
__device__ __forceinline__ float c1_act(float v) {
  if constexpr (sizeof(TI) == 4) return elu(v);
  else return elu_fast(v);
}

// Transposing LDS reads (ds_read_b64_tr_b16, 4 rows x 16 columns per 16-lane
// group): the MFMA operands of the bf16 weight gradients (the discriminator's
// in dconv_wgrad.hip too), which reduce over the ROW index of row-major LDS
// tiles (k_wgrad_bf16's comment has the layout).
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ v4i16 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)(p));
}
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p, int pitch) {
  const v4i16 lo = tr_read(p);
  const v4i16 hi = tr_read(p + 16 * pitch);
  const v8i16 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace conv
}  // namespace sel
