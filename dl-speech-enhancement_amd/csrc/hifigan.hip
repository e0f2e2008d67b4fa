// HiFi-GAN vocoder generator (models/vocoder/HiFiGAN.py:28-305 of the reference):
// one grouped conv primitive over channels-last rows with a LeakyReLU prologue
// and a bias / residual / tanh / scale-accumulate epilogue (include/sel.h,
// sel_hfg_conv_desc).  Inference only.
//
//   k_hfg_mfma  bf16 operands, v_mfma_f32_16x16x32_bf16, fp32 accumulation.
//               One block = 64 output rows of one sample x 16*WN output channels
//               of one group.  The activated input rows of the tile (64 rows +
//               the (K-1)*dil halo, CK channels at a time) are staged once in
//               LDS, rounded to bf16 after the prologue; the K taps then read
//               shifted row windows of that tile.  Weights come straight from
//               global memory, one 16-B fragment per lane and MFMA column tile,
//               shared by the 4 / WN row strips of the wave.
//   k_hfg_valu  one thread per output element: the fp32 instance, and in bf16
//               the thin outputs (N / G <= 4, the 32 -> 1 output conv) and
//               whatever does not fit the MFMA tile's LDS.
//   k_hfg_reslayer  both convs of a residual layer at 32 / 64 channels per group
//               in one launch, the conv1 tile kept in LDS (further down).
#include "sel_common.h"

namespace sel {
namespace hfg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

struct HArgs {
  int64_t rows;
  int T, To, Cg, Ng, N, K, dil, pad, pad_mode, G;
  int igs, rgs, ldin, ldres, bias_period, act_skip, tanh_out, accumulate;
  float slope, scale;
  int tps;    // row tiles per sample (MFMA kernel)
  int CK;     // channels staged per pass (multiple of 32)
  int vec_in; // input rows and weights are 16-B loadable in 8-channel pieces
};

constexpr int BM = 64;
constexpr int kLdsBytes = 64 * 1024;

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return float(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __bf16 from_f<__bf16>(float v) { return __bf16(v); }

__device__ __forceinline__ float lrelu(float v, float slope) { return v >= 0.f ? v : slope * v; }

// input row of tap position ti of a sample: -1 = reads as zero
__device__ __forceinline__ int in_row(const HArgs& a, int ti) {
  if (a.pad_mode == SEL_PAD_REPLICATE) return min(max(ti, 0), a.T - 1);
  return (ti >= 0 && ti < a.T) ? ti : -1;
}

template <typename TO>
__device__ __forceinline__ void epilogue(const HArgs& a, float v, int64_t orow, int g, int n, const float* bias,
                                         const TO* res, TO* out) {
  const int col = g * a.Ng + n;
  if (a.bias_period) v += bias[col % a.bias_period];
  if (res) v += to_f(res[orow * a.ldres + g * a.rgs + n]);
  if (a.tanh_out) v = tanhf(v);
  v *= a.scale;
  TO* o = out + orow * a.N + col;
  if (a.accumulate) v += to_f(*o);
  *o = from_f<TO>(v);
}

template <int WN, typename TO>
__global__ __launch_bounds__(256) void k_hfg_mfma(HArgs a, const __bf16* __restrict__ in,
                                                  const __bf16* __restrict__ wp, const float* __restrict__ bias,
                                                  const TO* res, TO* out) {
  constexpr int WM = 4 / WN;  // waves along the rows
  constexpr int MS = WN;      // 16-row strips per wave
  extern __shared__ __attribute__((aligned(16))) __bf16 xs[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w % WN, wm = w / WN;
  const int b = blockIdx.x / a.tps, t0 = (blockIdx.x % a.tps) * BM;
  const int g = blockIdx.z;
  const int n = blockIdx.y * (16 * WN) + wn * 16 + (lane & 15);  // this lane's output channel in the group
  const int q = lane >> 4;
  const int span = BM + (a.K - 1) * a.dil;
  const int P = a.CK + 8;  // LDS row pitch: 16 B past a power of two, rows 4 banks apart
  const __bf16* inb = in + int64_t(b) * a.T * a.ldin + g * a.igs;
  const __bf16* wg = wp + int64_t(g) * a.Ng * a.K * a.Cg;

  floatx4 acc[MS];
#pragma unroll
  for (int i = 0; i < MS; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.Cg; c0 += a.CK) {
    const int cw = min(a.CK, a.Cg - c0);
    const int cwp = (cw + 31) & ~31;  // zero-padded to the MFMA K step
    const int nvec = cwp >> 3;
    if (c0) __syncthreads();
    for (int i = tid; i < span * nvec; i += 256) {
      const int r = i / nvec, v = i - r * nvec;
      const int ti = t0 - a.pad + r;
      const int tr = in_row(a, ti);
      const int c = c0 + v * 8;
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = __bf16(0.f);
      if (tr >= 0 && c < a.Cg) {
        const float sl = tr < a.act_skip ? 1.f : a.slope;
        const __bf16* src = inb + int64_t(tr) * a.ldin + c;
        if (a.vec_in) {
          const bf16x8 x = *reinterpret_cast<const bf16x8*>(src);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = __bf16(lrelu(float(x[j]), sl));
        } else {
          for (int j = 0; j < 8; ++j)
            if (c + j < a.Cg) o[j] = __bf16(lrelu(float(src[j]), sl));
        }
      }
      *reinterpret_cast<bf16x8*>(xs + r * P + v * 8) = o;
    }
    __syncthreads();
    for (int k = 0; k < a.K; ++k) {
      const __bf16* wr = wg + (int64_t(n) * a.K + k) * a.Cg;
      for (int cc = 0; cc < cwp; cc += 32) {
        const int c = c0 + cc + q * 8;
        bf16x8 bw;
#pragma unroll
        for (int j = 0; j < 8; ++j) bw[j] = __bf16(0.f);
        if (n < a.Ng && c < a.Cg) {
          if (a.vec_in) {
            bw = *reinterpret_cast<const bf16x8*>(wr + c);
          } else {
            for (int j = 0; j < 8; ++j)
              if (c + j < a.Cg) bw[j] = wr[c + j];
          }
        }
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          const int row = (wm + i * WM) * 16 + (lane & 15) + k * a.dil;
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + row * P + cc + q * 8);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw, acc[i], 0, 0, 0);
        }
      }
    }
  }
  if (n >= a.Ng) return;
#pragma unroll
  for (int i = 0; i < MS; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + (wm + i * WM) * 16 + q * 4 + r;
      if (t < a.To) epilogue<TO>(a, acc[i][r], int64_t(b) * a.To + t, g, n, bias, res, out);
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void k_hfg_valu(HArgs a, const TI* __restrict__ in, const TI* __restrict__ wp,
                                                  const float* __restrict__ bias, const TO* res, TO* out) {
  constexpr bool kBf16 = sizeof(TI) == 2;
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= a.rows * a.N) return;
  const int col = int(idx % a.N);
  const int64_t m = idx / a.N;
  const int b = int(m / a.To), t = int(m % a.To);
  const int g = col / a.Ng, n = col - g * a.Ng;
  const TI* inb = in + int64_t(b) * a.T * a.ldin + g * a.igs;
  float acc = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const int tr = in_row(a, t + k * a.dil - a.pad);
    if (tr < 0) continue;
    const float sl = tr < a.act_skip ? 1.f : a.slope;
    const TI* xr = inb + int64_t(tr) * a.ldin;
    const TI* wr = wp + (int64_t(col) * a.K + k) * a.Cg;
    int c = 0;
    if constexpr (kBf16) {
      if (a.vec_in)
        for (; c + 8 <= a.Cg; c += 8) {
          const bf16x8 x = *reinterpret_cast<const bf16x8*>(xr + c);
          const bf16x8 wv = *reinterpret_cast<const bf16x8*>(wr + c);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc = fmaf(float(__bf16(lrelu(float(x[j]), sl))), float(wv[j]), acc);
        }
    }
    for (; c < a.Cg; ++c) {
      float v = lrelu(to_f(xr[c]), sl);
      if constexpr (kBf16) v = float(__bf16(v));  // the prologue result is rounded to bf16 once
      acc = fmaf(v, to_f(wr[c]), acc);
    }
  }
  epilogue<TO>(a, acc, m, g, n, bias, res, out);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// channels staged per pass of the MFMA kernel (0: the tile does not fit)
static int mfma_chunk(const HArgs& a) {
  const int64_t span = BM + int64_t(a.K - 1) * a.dil;
  const int cgp = (a.Cg + 31) & ~31;
  if (span * (32 + 8) * 2 > kLdsBytes) return 0;
  int ck = 32;
  while (ck < 256 && ck < cgp && span * (2 * ck + 8) * 2 <= kLdsBytes) ck *= 2;
  return ck;
}

static int check(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* in, const void* wpack,
                 const float* bias, const void* out, HArgs& a) {
  SEL_REQUIRE(d && in && wpack && out, SEL_ERR_ARG, "sel_hfg_conv_fwd: null pointer");
  SEL_REQUIRE((in_dtype == SEL_F32 && out_dtype == SEL_F32) ||
                  (in_dtype == SEL_BF16 && (out_dtype == SEL_BF16 || out_dtype == SEL_F32)),
              SEL_ERR_ARG, "sel_hfg_conv_fwd: bad dtypes (%d, %d)", in_dtype, out_dtype);
  SEL_REQUIRE(d->K > 0 && d->dil > 0 && d->T > 0 && d->T_out >= 0 && d->pad >= 0, SEL_ERR_ARG,
              "sel_hfg_conv_fwd: K, dil and T must be positive (K %d, dil %d, T %d, T_out %d, pad %d)", d->K, d->dil,
              d->T, d->T_out, d->pad);
  const int To = d->T_out ? d->T_out : d->T;
  SEL_REQUIRE(d->rows > 0 && d->rows % To == 0, SEL_ERR_ARG, "sel_hfg_conv_fwd: rows %lld is no multiple of %d",
              (long long)d->rows, To);
  SEL_REQUIRE(d->groups > 0 && d->C > 0 && d->N > 0 && d->C % d->groups == 0 && d->N % d->groups == 0, SEL_ERR_ARG,
              "sel_hfg_conv_fwd: groups %d must divide C %d and N %d", d->groups, d->C, d->N);
  const int Cg = d->C / d->groups, Ng = d->N / d->groups;
  SEL_REQUIRE(d->in_group_stride == 0 || d->in_group_stride == Cg, SEL_ERR_ARG,
              "sel_hfg_conv_fwd: in_group_stride %d is neither 0 nor C/G = %d", d->in_group_stride, Cg);
  SEL_REQUIRE(d->res_group_stride == 0 || d->res_group_stride == Ng, SEL_ERR_ARG,
              "sel_hfg_conv_fwd: res_group_stride %d is neither 0 nor N/G = %d", d->res_group_stride, Ng);
  SEL_REQUIRE(d->pad_mode == SEL_PAD_ZERO || d->pad_mode == SEL_PAD_REPLICATE, SEL_ERR_ARG,
              "sel_hfg_conv_fwd: bad pad_mode %d", d->pad_mode);
  SEL_REQUIRE(d->bias_period >= 0 && (d->bias_period == 0 || (bias && d->N % d->bias_period == 0)), SEL_ERR_ARG,
              "sel_hfg_conv_fwd: bias_period %d needs a bias and must divide N %d", d->bias_period, d->N);
  SEL_REQUIRE(d->act_skip >= 0, SEL_ERR_ARG, "sel_hfg_conv_fwd: act_skip %d < 0", d->act_skip);
  const int64_t B = d->rows / To;
  const int ldin = d->in_group_stride ? d->C : Cg;
  SEL_REQUIRE(B * d->T * ldin < (int64_t(1) << 40) && d->rows * d->N < (int64_t(1) << 40) &&
                  int64_t(d->K - 1) * d->dil < (1 << 24) && int64_t(d->N) * d->K * Cg < (int64_t(1) << 31),
              SEL_ERR_UNSUPPORTED, "sel_hfg_conv_fwd: shape too large");
  a.rows = d->rows;
  a.T = d->T, a.To = To, a.Cg = Cg, a.Ng = Ng, a.N = d->N, a.K = d->K, a.dil = d->dil, a.pad = d->pad;
  a.pad_mode = d->pad_mode, a.G = d->groups, a.igs = d->in_group_stride, a.rgs = d->res_group_stride;
  a.ldin = ldin, a.ldres = d->res_group_stride ? d->N : Ng;
  a.bias_period = d->bias_period, a.act_skip = d->act_skip, a.tanh_out = d->tanh_out != 0;
  a.accumulate = d->accumulate != 0, a.slope = d->act_slope, a.scale = d->out_scale;
  a.tps = (To + BM - 1) / BM;
  a.vec_in = in_dtype == SEL_BF16 && Cg % 8 == 0 && aligned16(in) && aligned16(wpack);
  a.CK = 0;
  return SEL_OK;
}

template <int WN, typename TO>
static void launch_mfma(const HArgs& a, const void* in, const void* wp, const float* bias, const void* res, void* out,
                        hipStream_t s) {
  const int64_t span = BM + int64_t(a.K - 1) * a.dil;
  const size_t lds = size_t(span) * (a.CK + 8) * 2;
  dim3 grid(unsigned((a.rows / a.To) * a.tps), unsigned((a.Ng + 16 * WN - 1) / (16 * WN)), unsigned(a.G));
  hipLaunchKernelGGL((k_hfg_mfma<WN, TO>), grid, dim3(256), lds, s, a, static_cast<const __bf16*>(in),
                     static_cast<const __bf16*>(wp), bias, static_cast<const TO*>(res), static_cast<TO*>(out));
}

template <typename TI, typename TO>
static void launch_valu(const HArgs& a, const void* in, const void* wp, const float* bias, const void* res, void* out,
                        hipStream_t s) {
  const int64_t total = a.rows * a.N;
  hipLaunchKernelGGL((k_hfg_valu<TI, TO>), dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, a,
                     static_cast<const TI*>(in), static_cast<const TI*>(wp), bias, static_cast<const TO*>(res),
                     static_cast<TO*>(out));
}

// 0 = VALU kernel, else the MFMA kernel's WN
static int pick(HArgs& a, int in_dtype) {
  if (in_dtype != SEL_BF16 || a.Ng <= 4) return 0;
  a.CK = mfma_chunk(a);
  if (!a.CK) return 0;
  const int64_t blocks = (a.rows / a.To) * a.tps;
  if (blocks >= (int64_t(1) << 31) || a.G > 65535 || (a.Ng + 15) / 16 > 65535) return 0;
  return a.Ng > 32 ? 4 : a.Ng > 16 ? 2 : 1;
}


// ---- fused residual layer (sel_hfg_reslayer_fwd) ------------------------------------------
// out = x + conv2_{K,1}(lrelu(conv1_{K,d}(lrelu(x)) + b1)) + b2 for one 64-row
// tile of one sample and one group (C/G = 16 * WN in {32, 64}).  The activated x
// tile (HR + (K-1)*d rows) and the activated conv1 tile (the 64 output rows
// plus the K-1 halo rows conv2 needs, HR = 80 rows = 5 MFMA strips) stay in
// LDS; h never goes to HBM.  Same arithmetic as two k_hfg_mfma launches: the
// same MFMA sequence per output (taps outer, 32-channel steps inner), h rounded
// to bf16 as the first launch would store it, its LeakyReLU rounded to bf16
// as the second launch's prologue does -- so the results are bit-identical.
constexpr int RL_HR = 80;   // conv1 rows per tile: 64 + (K - 1) <= 80 for K <= 17
constexpr int RL_S1 = RL_HR / 16;

template <int WN, typename TO>
__global__ __launch_bounds__(256) void k_hfg_reslayer(HArgs a, const __bf16* __restrict__ x,
                                                      const __bf16* __restrict__ w1, const float* __restrict__ b1,
                                                      const __bf16* __restrict__ w2, const float* __restrict__ b2,
                                                      TO* out) {
  constexpr int WM = 4 / WN;
  constexpr int CG = 16 * WN;
  constexpr int P = CG + 8;
  constexpr int MS1 = (RL_S1 + WM - 1) / WM, MS2 = 4 / WM;
  extern __shared__ __attribute__((aligned(16))) __bf16 xs[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w % WN, wm = w / WN;
  const int b = blockIdx.x / a.tps, t0 = (blockIdx.x % a.tps) * BM;
  const int g = blockIdx.z;
  const int n = wn * 16 + (lane & 15);
  const int q = lane >> 4;
  const int K = a.K, dil = a.dil;
  const int span = RL_HR + (K - 1) * dil;
  __bf16* hs = xs + span * P;
  const __bf16* xb = x + int64_t(b) * a.T * a.ldin + g * a.igs;

  // activated x rows t0 - (K-1) - (K-1)*dil ... (zero outside the sample)
  constexpr int NV = CG / 8;
  for (int i = tid; i < span * NV; i += 256) {
    const int r = i / NV, v = i - r * NV;
    const int tr = t0 - (K - 1) - (K - 1) * dil + r;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = __bf16(0.f);
    if (tr >= 0 && tr < a.T) {
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xb + int64_t(tr) * a.ldin + v * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = __bf16(lrelu(float(xv[j]), a.slope));
    }
    *reinterpret_cast<bf16x8*>(xs + r * P + v * 8) = o;
  }
  __syncthreads();

  // conv1 on rows t0 - (K-1) + [0, 80)
  {
    floatx4 acc[MS1];
#pragma unroll
    for (int i = 0; i < MS1; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    const __bf16* wg = w1 + (int64_t(g) * CG + n) * K * CG;
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int cc = 0; cc < CG; cc += 32) {
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(wg + k * CG + cc + q * 8);
#pragma unroll
        for (int i = 0; i < MS1; ++i) {
          const int strip = wm + i * WM;
          if (strip < RL_S1) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + (strip * 16 + (lane & 15) + k * dil) * P + cc + q * 8);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw, acc[i], 0, 0, 0);
          }
        }
      }
    const float bias1 = b1 ? b1[g * CG + n] : 0.f;
#pragma unroll
    for (int i = 0; i < MS1; ++i) {
      const int strip = wm + i * WM;
      if (strip < RL_S1)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = strip * 16 + q * 4 + r;
          const int th = t0 - (K - 1) + j;
          // conv2's causal pad is zero rows of lrelu(h), not conv1 of the padding
          const float h = float(__bf16(acc[i][r] + bias1));
          hs[j * P + n] = th >= 0 ? __bf16(lrelu(h, a.slope)) : __bf16(0.f);
        }
    }
  }
  __syncthreads();

  // conv2 (dilation 1) on rows t0 + [0, 64), epilogue with x as the residual
  floatx4 acc[MS2];
#pragma unroll
  for (int i = 0; i < MS2; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  const __bf16* wg = w2 + (int64_t(g) * CG + n) * K * CG;
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int cc = 0; cc < CG; cc += 32) {
      const bf16x8 bw = *reinterpret_cast<const bf16x8*>(wg + k * CG + cc + q * 8);
#pragma unroll
      for (int i = 0; i < MS2; ++i) {
        const int row = (wm + i * WM) * 16 + (lane & 15) + k;
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(hs + row * P + cc + q * 8);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw, acc[i], 0, 0, 0);
      }
    }
#pragma unroll
  for (int i = 0; i < MS2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + (wm + i * WM) * 16 + q * 4 + r;
      if (t < a.T) epilogue<TO>(a, acc[i][r], int64_t(b) * a.T + t, g, n, b2, reinterpret_cast<const TO*>(x), out);
    }
}

// (C/G, K) pairs on which the fused layer measured faster than two launches in
// the same-call A/B of tools/vocoder_bench.py; the others
// keep two launches
static bool reslayer_default(int Cg, int K) {
  // all six measured faster (B = 16 x 1 s at 48 kHz: 0.062 vs 0.102 ms at (32, 3) ... 0.107-0.120 vs
  // 0.130-0.132 ms at (64, 11))
  return (Cg == 32 || Cg == 64) && (K == 3 || K == 7 || K == 11);
}

}  // namespace hfg
}  // namespace sel

extern "C" {

int sel_hfg_conv_kernel(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype) {
  sel::hfg::HArgs a;
  static const int dummy = 0;
  const float fb = 0.f;
  if (int rc = sel::hfg::check(d, in_dtype, out_dtype, &dummy, &dummy, &fb, &dummy, a)) return rc;
  a.vec_in = in_dtype == SEL_BF16 && a.Cg % 8 == 0;
  return sel::hfg::pick(a, in_dtype);
}

int sel_hfg_conv_fwd(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* in, const void* wpack,
                     const float* bias, const void* res, void* out, sel_stream_t stream) {
  using namespace sel::hfg;
  HArgs a;
  if (int rc = check(d, in_dtype, out_dtype, in, wpack, bias, out, a)) return rc;
  SEL_REQUIRE(sel::initialized(), SEL_ERR_STATE, "sel_init() has not succeeded");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int wn = pick(a, in_dtype);
  const bool of = out_dtype == SEL_F32;
  if (wn == 0) {
    SEL_REQUIRE(a.rows * a.N < (int64_t(1) << 39), SEL_ERR_UNSUPPORTED, "sel_hfg_conv_fwd: too many outputs");
    if (in_dtype == SEL_F32)
      launch_valu<float, float>(a, in, wpack, bias, res, out, s);
    else if (of)
      launch_valu<__bf16, float>(a, in, wpack, bias, res, out, s);
    else
      launch_valu<__bf16, __bf16>(a, in, wpack, bias, res, out, s);
  } else if (of) {
    if (wn == 4) launch_mfma<4, float>(a, in, wpack, bias, res, out, s);
    else if (wn == 2) launch_mfma<2, float>(a, in, wpack, bias, res, out, s);
    else launch_mfma<1, float>(a, in, wpack, bias, res, out, s);
  } else {
    if (wn == 4) launch_mfma<4, __bf16>(a, in, wpack, bias, res, out, s);
    else if (wn == 2) launch_mfma<2, __bf16>(a, in, wpack, bias, res, out, s);
    else launch_mfma<1, __bf16>(a, in, wpack, bias, res, out, s);
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_hfg_reslayer_fwd(const sel_hfg_conv_desc* d1, int dtype, const void* x, const void* w1pack, const float* b1,
                         const void* w2pack, const float* b2, void* out, sel_stream_t stream) {
  using namespace sel::hfg;
  HArgs a;
  SEL_REQUIRE(w2pack, SEL_ERR_ARG, "sel_hfg_reslayer_fwd: null pointer");
  if (int rc = check(d1, dtype, dtype, x, w1pack, b1, out, a)) return rc;
  SEL_REQUIRE(!a.bias_period || b2, SEL_ERR_ARG, "sel_hfg_reslayer_fwd: bias_period %d needs both biases",
              a.bias_period);
  const int force = sel::tune(71);  // 1: always two launches, 2: the fused kernel wherever it applies
  const int64_t lds = (int64_t(RL_HR) * 2 + int64_t(a.K - 1) * a.dil) * (a.Cg + 8) * 2;
  const bool shape_ok = dtype == SEL_BF16 && d1->C == d1->N && (a.Cg == 32 || a.Cg == 64) &&
                        (a.K == 3 || a.K == 7 || a.K == 11) && a.pad_mode == SEL_PAD_ZERO &&
                        a.pad == (a.K - 1) * a.dil && a.To == a.T && a.act_skip == 0 && !a.tanh_out &&
                        (a.bias_period == 0 || a.bias_period == a.N) && (a.igs == 0) == (a.rgs == 0) && a.vec_in &&
                        aligned16(w2pack) && lds <= kLdsBytes && (a.rows / a.T) * a.tps < (int64_t(1) << 31) &&
                        a.G <= 65535;
  SEL_REQUIRE(shape_ok && force != 1 && (force == 2 || reslayer_default(a.Cg, a.K)), SEL_ERR_UNSUPPORTED,
              "sel_hfg_reslayer_fwd: two launches of sel_hfg_conv_fwd serve this layer (C/G %d, K %d, tune key 71 = %d)",
              a.Cg, a.K, force);
  SEL_REQUIRE(sel::initialized(), SEL_ERR_STATE, "sel_init() has not succeeded");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(unsigned((a.rows / a.T) * a.tps), 1, unsigned(a.G));
  const __bf16* xp = static_cast<const __bf16*>(x);
  const __bf16* w1 = static_cast<const __bf16*>(w1pack);
  const __bf16* w2 = static_cast<const __bf16*>(w2pack);
  const float* bb1 = a.bias_period ? b1 : nullptr;
  if (a.Cg == 64)
    hipLaunchKernelGGL((k_hfg_reslayer<4, __bf16>), grid, dim3(256), size_t(lds), s, a, xp, w1, bb1, w2, b2,
                       static_cast<__bf16*>(out));
  else
    hipLaunchKernelGGL((k_hfg_reslayer<2, __bf16>), grid, dim3(256), size_t(lds), s, a, xp, w1, bb1, w2, b2,
                       static_cast<__bf16*>(out));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
