// Backward of the HiFi-GAN generator's grouped conv primitive (include/sel.h,
// sel_hfg_conv_bwd_data / sel_hfg_conv_wgrad).  With the forward written as
//   out = prev*[accumulate] + out_scale * tanh?( conv(act(x)) + bias + res ),
// gpre = out_scale * gout * (1 - out^2 when tanh_out) is the gradient at the conv's
// own output.  out_scale is a scalar, so every kernel here sums products of the
// UNSCALED operands (gout is used as stored: no second rounding of a bf16
// gradient) and multiplies the fp32 sum by out_scale once.
//
//   k_bwd_data_mfma  bf16: one block = 64 gin rows of one sample x 16*WN input
//                    channels of one group (all groups summed when the input is
//                    shared).  The gout rows of the tile (64 + the (K-1)*dil
//                    halo, CK channels at a time) are staged once in LDS, the K
//                    taps read shifted row windows; weights come from global
//                    memory in the transposed pack Wd[G][C/G][K][N/G], one 16-B
//                    fragment per lane.  Epilogue: replicate-pad edge terms,
//                    LeakyReLU', skip, accumulate, one rounding.
//   k_bwd_data_valu  one thread per gin element: fp32, the tanh output conv,
//                    thin shapes and what does not fit the MFMA tile's LDS.
//   k_wgrad_mfma     bf16: one block = one tap x one group x 64 out x 64 in
//                    channels over the 64-row tiles of one row split; gout and
//                    the activated, tap-shifted input tile are staged TRANSPOSED
//                    in LDS (rows are the MFMA reduction axis); fp32 partials.
//   k_wgrad_valu     one thread per weight (and bias) element and row split.
//   k_wgrad_finish   fixed-order sum of the split partials, times out_scale; the
//                    bias folds its phases (n mod bias_period).  No atomics: two
//                    runs give the same bits.
#include "sel_common.h"

namespace sel {
namespace hfgb {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

struct BArgs {
  int64_t rows;
  int T, C, N, Cg, Ng, K, dil, pad, pad_mode, G;
  int igs, ldin, bias_period, tanh_out, accumulate;
  float slope, scale, skip_scale;
  int tps;     // 64-row tiles per sample
  int CK;      // gout channels staged per pass of the data kernel (multiple of 32)
  int vec;     // 16-B loads of gout / x / weights in 8-channel pieces
  // weight gradient
  int ntiles, nsplit, tiles_per_split, ntn, ntc;
  int64_t per;  // N * K * Cg
};

constexpr int BM = 64;
constexpr int kLdsBytes = 64 * 1024;
constexpr int PT = 68;  // pitch of the transposed wgrad tiles (8-B aligned rows)
constexpr int kTuneSplit = 72;

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return float(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __bf16 from_f<__bf16>(float v) { return __bf16(v); }

__device__ __forceinline__ float lrelu(float v, float slope) { return v >= 0.f ? v : slope * v; }

// input row of tap position ti of a sample: -1 = reads as zero
__device__ __forceinline__ int in_row(const BArgs& a, int ti) {
  if (a.pad_mode == SEL_PAD_REPLICATE) return min(max(ti, 0), a.T - 1);
  return (ti >= 0 && ti < a.T) ? ti : -1;
}

// gout * (1 - out^2 when tanh_out), without out_scale
template <typename TG>
__device__ __forceinline__ float gpre_at(const BArgs& a, const TG* gout, const TG* out, int64_t i) {
  float v = to_f(gout[i]);
  if (a.tanh_out) {
    const float o = to_f(out[i]);
    v *= 1.f - o * o;
  }
  return v;
}

// sum over taps k, output rows t with in_row(t + k*dil - pad) == s and the N/G
// outputs of group g of Wd[g][c][k][n] * gpre[b, t, n].  edge_only: only the
// clamped taps of the replicate pad (t != s - k*dil + pad), which the matrix
// tile does not cover.
template <typename TW, typename TG>
__device__ float tap_sum(const BArgs& a, const TW* wd, const TG* gout, const TG* out, int b, int s, int g, int c,
                         bool edge_only) {
  float acc = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const int base = s - k * a.dil + a.pad;
    int lo = base, hi = base;
    if (a.pad_mode == SEL_PAD_REPLICATE) {
      if (s == 0) lo = 0;
      if (s == a.T - 1) hi = a.T - 1;
    }
    lo = max(lo, 0), hi = min(hi, a.T - 1);
    const TW* wr = wd + ((int64_t(g) * a.Cg + c) * a.K + k) * a.Ng;
    for (int t = lo; t <= hi; ++t) {
      if (edge_only && t == base) continue;
      const int64_t o = (int64_t(b) * a.T + t) * a.N + g * a.Ng;
      for (int n = 0; n < a.Ng; ++n) acc = fmaf(to_f(wr[n]), gpre_at(a, gout, out, o + n), acc);
    }
  }
  return acc;
}

// v = the fp32 tap sum (unscaled) of gin element (row m, column col of pitch ldin)
template <typename TI>
__device__ __forceinline__ void finish_gin(const BArgs& a, float v, int64_t m, int col, int c, const TI* x,
                                           const TI* gskip, TI* gin) {
  v *= a.scale;
  const int64_t i = m * a.ldin + col;
  if (a.slope != 1.f && !(to_f(x[i]) > 0.f)) v *= a.slope;
  if (gskip) {
    float sk;
    if (a.igs) {
      sk = to_f(gskip[m * a.C + col]);
    } else {
      sk = 0.f;
      for (int g = 0; g < a.G; ++g) sk += to_f(gskip[m * a.C + g * a.Cg + c]);
    }
    v = fmaf(a.skip_scale, sk, v);
  }
  if (a.accumulate) v += to_f(gin[i]);
  gin[i] = from_f<TI>(v);
}

template <typename TI, typename TG>
__global__ __launch_bounds__(256) void k_bwd_data_valu(BArgs a, const TG* __restrict__ gout,
                                                       const TG* __restrict__ out, const TI* __restrict__ x,
                                                       const TI* __restrict__ wd, const TI* gskip, TI* gin) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= a.rows * a.ldin) return;
  const int col = int(idx % a.ldin);
  const int64_t m = idx / a.ldin;
  const int b = int(m / a.T), s = int(m % a.T);
  const int g0 = a.igs ? col / a.Cg : 0, g1 = a.igs ? g0 + 1 : a.G;
  const int c = col - (a.igs ? g0 * a.Cg : 0);
  float acc = 0.f;
  for (int g = g0; g < g1; ++g) acc += tap_sum(a, wd, gout, out, b, s, g, c, false);
  finish_gin<TI>(a, acc, m, col, c, x, gskip, gin);
}

template <int WN>
__global__ __launch_bounds__(256) void k_bwd_data_mfma(BArgs a, const __bf16* __restrict__ gout,
                                                       const __bf16* __restrict__ x, const __bf16* __restrict__ wd,
                                                       const __bf16* gskip, __bf16* gin) {
  constexpr int WM = 4 / WN;
  constexpr int MS = WN;
  extern __shared__ __attribute__((aligned(16))) __bf16 gs[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w % WN, wm = w / WN;
  const int b = blockIdx.x / a.tps, s0 = (blockIdx.x % a.tps) * BM;
  const int c = blockIdx.y * (16 * WN) + wn * 16 + (lane & 15);  // this lane's input channel in the group
  const int q = lane >> 4;
  const int span = BM + (a.K - 1) * a.dil;
  const int P = a.CK + 8;
  const int g0 = a.igs ? int(blockIdx.z) : 0, g1 = a.igs ? g0 + 1 : a.G;
  const int tlo = s0 + a.pad - (a.K - 1) * a.dil;  // gout row of LDS row 0

  floatx4 acc[MS];
#pragma unroll
  for (int i = 0; i < MS; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};

  bool first = true;
  for (int g = g0; g < g1; ++g) {
    const __bf16* gb = gout + int64_t(b) * a.T * a.N + g * a.Ng;
    for (int n0 = 0; n0 < a.Ng; n0 += a.CK) {
      const int cw = min(a.CK, a.Ng - n0);
      const int cwp = (cw + 31) & ~31;
      const int nvec = cwp >> 3;
      if (!first) __syncthreads();
      first = false;
      for (int i = tid; i < span * nvec; i += 256) {
        const int r = i / nvec, v = i - r * nvec;
        const int t = tlo + r;
        const int n = n0 + v * 8;
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = __bf16(0.f);
        if (t >= 0 && t < a.T && n < a.Ng) {
          const __bf16* src = gb + int64_t(t) * a.N + n;
          if (a.vec) {
            o = *reinterpret_cast<const bf16x8*>(src);
          } else {
            for (int j = 0; j < 8; ++j)
              if (n + j < a.Ng) o[j] = src[j];
          }
        }
        *reinterpret_cast<bf16x8*>(gs + r * P + v * 8) = o;
      }
      __syncthreads();
      for (int k = 0; k < a.K; ++k) {
        const int shift = (a.K - 1 - k) * a.dil;
        const __bf16* wr = wd + ((int64_t(g) * a.Cg + c) * a.K + k) * a.Ng;
        for (int nn = 0; nn < cwp; nn += 32) {
          const int n = n0 + nn + q * 8;
          bf16x8 bw;
#pragma unroll
          for (int j = 0; j < 8; ++j) bw[j] = __bf16(0.f);
          if (c < a.Cg && n < a.Ng) {
            if (a.vec) {
              bw = *reinterpret_cast<const bf16x8*>(wr + n);
            } else {
              for (int j = 0; j < 8; ++j)
                if (n + j < a.Ng) bw[j] = wr[n + j];
            }
          }
#pragma unroll
          for (int i = 0; i < MS; ++i) {
            const int row = (wm + i * WM) * 16 + (lane & 15) + shift;
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(gs + row * P + nn + q * 8);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw, acc[i], 0, 0, 0);
          }
        }
      }
    }
  }
  if (c >= a.Cg) return;
  const int col = a.igs ? g0 * a.Cg + c : c;
#pragma unroll
  for (int i = 0; i < MS; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = s0 + (wm + i * WM) * 16 + q * 4 + r;
      if (s >= a.T) continue;
      float v = acc[i][r];
      if (a.pad_mode == SEL_PAD_REPLICATE && (s == 0 || s == a.T - 1))
        for (int g = g0; g < g1; ++g) v += tap_sum(a, wd, gout, gout, b, s, g, c, true);
      finish_gin<__bf16>(a, v, int64_t(b) * a.T + s, col, c, x, gskip, gin);
    }
}

// ---- weight gradient ------------------------------------------------------------------------
template <typename TI, typename TG>
__global__ __launch_bounds__(256) void k_wgrad_valu(BArgs a, const TG* __restrict__ gout, const TG* __restrict__ out,
                                                    const TI* __restrict__ x, float* __restrict__ part) {
  constexpr bool kBf16 = sizeof(TI) == 2;
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.per + a.N) return;
  const int split = blockIdx.y;
  const int tile0 = split * a.tiles_per_split, tile1 = min(a.ntiles, tile0 + a.tiles_per_split);
  float acc = 0.f;
  if (i < a.per) {
    const int c = int(i % a.Cg);
    const int k = int((i / a.Cg) % a.K);
    const int n = int(i / (int64_t(a.Cg) * a.K));
    const int g = n / a.Ng;
    for (int tile = tile0; tile < tile1; ++tile) {
      const int b = tile / a.tps, t0 = (tile % a.tps) * BM;
      const int t1 = min(a.T, t0 + BM);
      for (int t = t0; t < t1; ++t) {
        const int tr = in_row(a, t + k * a.dil - a.pad);
        if (tr < 0) continue;
        float v = lrelu(to_f(x[(int64_t(b) * a.T + tr) * a.ldin + g * a.igs + c]), a.slope);
        if constexpr (kBf16) v = float(__bf16(v));  // the prologue result the forward multiplied
        acc = fmaf(gpre_at(a, gout, out, (int64_t(b) * a.T + t) * a.N + n), v, acc);
      }
    }
  } else {
    const int n = int(i - a.per);
    for (int tile = tile0; tile < tile1; ++tile) {
      const int b = tile / a.tps, t0 = (tile % a.tps) * BM;
      const int t1 = min(a.T, t0 + BM);
      for (int t = t0; t < t1; ++t) acc += gpre_at(a, gout, out, (int64_t(b) * a.T + t) * a.N + n);
    }
  }
  part[int64_t(split) * (a.per + a.N) + i] = acc;
}

__global__ __launch_bounds__(256) void k_wgrad_mfma(BArgs a, const __bf16* __restrict__ gout,
                                                    const __bf16* __restrict__ x, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) __bf16 gT[64 * PT];  // [n][t]
  __shared__ __attribute__((aligned(16))) __bf16 aT[64 * PT];  // [c][t], rows shifted by the block's tap
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q = lane >> 4;
  const int split = blockIdx.x;
  const int tiles_nc = a.ntn * a.ntc;
  const int k = blockIdx.y / tiles_nc, rem = blockIdx.y % tiles_nc;
  const int n0 = (rem / a.ntc) * 64, c0 = (rem % a.ntc) * 64;
  const int g = blockIdx.z;
  const int tile0 = split * a.tiles_per_split, tile1 = min(a.ntiles, tile0 + a.tiles_per_split);
  const bool bias_block = k == 0 && c0 == 0;

  floatx4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  for (int tile = tile0; tile < tile1; ++tile) {
    const int b = tile / a.tps, t0 = (tile % a.tps) * BM;
    if (tile != tile0) __syncthreads();
    for (int i = tid; i < 64 * 8; i += 256) {
      const int tl = i >> 3, v = i & 7;
      const int t = t0 + tl;
      bf16x8 go, xo;
#pragma unroll
      for (int j = 0; j < 8; ++j) go[j] = __bf16(0.f), xo[j] = __bf16(0.f);
      if (t < a.T) {
        const int n = n0 + v * 8;
        if (n < a.Ng) {
          const __bf16* src = gout + (int64_t(b) * a.T + t) * a.N + g * a.Ng + n;
          if (a.vec) {
            go = *reinterpret_cast<const bf16x8*>(src);
          } else {
            for (int j = 0; j < 8; ++j)
              if (n + j < a.Ng) go[j] = src[j];
          }
        }
        const int c = c0 + v * 8;
        const int tr = in_row(a, t + k * a.dil - a.pad);
        if (tr >= 0 && c < a.Cg) {
          const __bf16* src = x + (int64_t(b) * a.T + tr) * a.ldin + g * a.igs + c;
          if (a.vec) {
            const bf16x8 xv = *reinterpret_cast<const bf16x8*>(src);
#pragma unroll
            for (int j = 0; j < 8; ++j) xo[j] = __bf16(lrelu(float(xv[j]), a.slope));
          } else {
            for (int j = 0; j < 8; ++j)
              if (c + j < a.Cg) xo[j] = __bf16(lrelu(float(src[j]), a.slope));
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        gT[(v * 8 + j) * PT + tl] = go[j];
        aT[(v * 8 + j) * PT + tl] = xo[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 64; tt += 32) {
      const __bf16* ap = gT + (w * 16 + (lane & 15)) * PT + tt + q * 8;
      const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(ap), a1 = *reinterpret_cast<const bf16x4*>(ap + 4);
      const bf16x8 af = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const __bf16* bp = aT + (ct * 16 + (lane & 15)) * PT + tt + q * 8;
        const bf16x4 b0 = *reinterpret_cast<const bf16x4*>(bp), b1 = *reinterpret_cast<const bf16x4*>(bp + 4);
        const bf16x8 bf = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[ct], 0, 0, 0);
      }
    }
    if (bias_block && tid < 64)
      for (int t = 0; t < 64; ++t) bsum += float(gT[tid * PT + t]);
  }
  float* ps = part + int64_t(split) * (a.per + a.N);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + w * 16 + q * 4 + r, c = c0 + ct * 16 + (lane & 15);
      if (n < a.Ng && c < a.Cg) ps[((int64_t(g) * a.Ng + n) * a.K + k) * a.Cg + c] = acc[ct][r];
    }
  if (bias_block && tid < 64 && n0 + tid < a.Ng) ps[a.per + g * a.Ng + n0 + tid] = bsum;
}

__global__ __launch_bounds__(256) void k_wgrad_finish(BArgs a, const float* __restrict__ part,
                                                      float* __restrict__ gwp, float* __restrict__ gbias) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t stride = a.per + a.N;
  if (i < a.per) {
    float acc = 0.f;
    for (int s = 0; s < a.nsplit; ++s) acc += part[s * stride + i];
    gwp[i] = acc * a.scale;
  } else if (gbias && i < a.per + a.bias_period) {
    const int j = int(i - a.per);
    float acc = 0.f;
    for (int s = 0; s < a.nsplit; ++s)
      for (int n = j; n < a.N; n += a.bias_period) acc += part[s * stride + a.per + n];
    gbias[j] = acc * a.scale;
  }
}

// ---- host -----------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int check(const char* fn, const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, BArgs& a) {
  SEL_REQUIRE(d, SEL_ERR_ARG, "%s: null descriptor", fn);
  SEL_REQUIRE((in_dtype == SEL_F32 && out_dtype == SEL_F32) ||
                  (in_dtype == SEL_BF16 && (out_dtype == SEL_BF16 || out_dtype == SEL_F32)),
              SEL_ERR_ARG, "%s: bad dtypes (%d, %d)", fn, in_dtype, out_dtype);
  SEL_REQUIRE(d->K > 0 && d->dil > 0 && d->T > 0 && d->T_out >= 0 && d->pad >= 0, SEL_ERR_ARG,
              "%s: K, dil and T must be positive (K %d, dil %d, T %d, T_out %d, pad %d)", fn, d->K, d->dil, d->T,
              d->T_out, d->pad);
  const int To = d->T_out ? d->T_out : d->T;
  SEL_REQUIRE(d->rows > 0 && d->rows % To == 0, SEL_ERR_ARG, "%s: rows %lld is no multiple of %d", fn,
              (long long)d->rows, To);
  SEL_REQUIRE(d->groups > 0 && d->C > 0 && d->N > 0 && d->C % d->groups == 0 && d->N % d->groups == 0, SEL_ERR_ARG,
              "%s: groups %d must divide C %d and N %d", fn, d->groups, d->C, d->N);
  const int Cg = d->C / d->groups, Ng = d->N / d->groups;
  SEL_REQUIRE(d->in_group_stride == 0 || d->in_group_stride == Cg, SEL_ERR_ARG,
              "%s: in_group_stride %d is neither 0 nor C/G = %d", fn, d->in_group_stride, Cg);
  SEL_REQUIRE(d->res_group_stride == 0 || d->res_group_stride == Ng, SEL_ERR_ARG,
              "%s: res_group_stride %d is neither 0 nor N/G = %d", fn, d->res_group_stride, Ng);
  SEL_REQUIRE(d->pad_mode == SEL_PAD_ZERO || d->pad_mode == SEL_PAD_REPLICATE, SEL_ERR_ARG, "%s: bad pad_mode %d", fn,
              d->pad_mode);
  SEL_REQUIRE(d->bias_period >= 0 && (d->bias_period == 0 || d->N % d->bias_period == 0), SEL_ERR_ARG,
              "%s: bias_period %d must divide N %d", fn, d->bias_period, d->N);
  SEL_REQUIRE(d->act_skip >= 0, SEL_ERR_ARG, "%s: act_skip %d < 0", fn, d->act_skip);
  SEL_REQUIRE(To == d->T && d->act_skip == 0, SEL_ERR_UNSUPPORTED,
              "%s: the streaming forms (T_out %d != T %d, act_skip %d) have no backward", fn, d->T_out, d->T,
              d->act_skip);
  SEL_REQUIRE(d->rows * std::max(d->C, d->N) < (int64_t(1) << 40) && int64_t(d->K - 1) * d->dil < (1 << 24) &&
                  int64_t(d->N) * d->K * Cg < (int64_t(1) << 31),
              SEL_ERR_UNSUPPORTED, "%s: shape too large", fn);
  a.rows = d->rows;
  a.T = d->T, a.C = d->C, a.N = d->N, a.Cg = Cg, a.Ng = Ng, a.K = d->K, a.dil = d->dil, a.pad = d->pad;
  a.pad_mode = d->pad_mode, a.G = d->groups, a.igs = d->in_group_stride;
  a.ldin = d->in_group_stride ? d->C : Cg;
  a.bias_period = d->bias_period, a.tanh_out = d->tanh_out != 0, a.accumulate = d->accumulate != 0;
  a.slope = d->act_slope, a.scale = d->out_scale, a.skip_scale = 0.f;
  a.tps = (d->T + BM - 1) / BM;
  a.CK = 0, a.vec = 0;
  a.ntiles = 0, a.nsplit = 0, a.tiles_per_split = 0, a.ntn = 0, a.ntc = 0;
  a.per = int64_t(d->N) * d->K * Cg;
  return SEL_OK;
}

// data gradient: 0 = VALU kernel, else the MFMA kernel's WN
static int pick_data(BArgs& a, int in_dtype, int out_dtype) {
  if (in_dtype != SEL_BF16 || out_dtype != SEL_BF16 || a.tanh_out || a.Cg <= 4 || a.Ng <= 4) return 0;
  const int64_t span = BM + int64_t(a.K - 1) * a.dil;
  const int ngp = (a.Ng + 31) & ~31;
  if (span * (32 + 8) * 2 > kLdsBytes) return 0;
  int ck = 32;
  while (ck < 256 && ck < ngp && span * (2 * ck + 8) * 2 <= kLdsBytes) ck *= 2;
  a.CK = ck;
  const int64_t blocks = (a.rows / a.T) * a.tps;
  if (blocks >= (int64_t(1) << 31) || a.G > 65535 || (a.Cg + 15) / 16 > 65535) return 0;
  return a.Cg > 32 ? 4 : a.Cg > 16 ? 2 : 1;
}

// weight gradient: 1 = the MFMA kernel, 0 = VALU; fills the split plan
static int plan_wgrad(BArgs& a, int in_dtype, int out_dtype) {
  a.ntn = (a.Ng + 63) / 64, a.ntc = (a.Cg + 63) / 64;
  int mfma = in_dtype == SEL_BF16 && out_dtype == SEL_BF16 && !a.tanh_out && a.Cg > 4 && a.Ng > 4 && a.G <= 65535 &&
             int64_t(a.K) * a.ntn * a.ntc <= 65535;
  const int64_t ntiles = (a.rows / a.T) * a.tps;
  if (ntiles >= (int64_t(1) << 30)) return -1;
  a.ntiles = int(ntiles);
  const int64_t per_split = mfma ? int64_t(a.K) * a.ntn * a.ntc * a.G : (a.per + a.N + 255) / 256;
  int64_t want = sel::tune(kTuneSplit) > 0 ? sel::tune(kTuneSplit) : std::max<int64_t>(1, 2048 / per_split);
  want = std::min<int64_t>(std::min<int64_t>(want, 1024), ntiles);
  a.tiles_per_split = int((ntiles + want - 1) / want);
  a.nsplit = (a.ntiles + a.tiles_per_split - 1) / a.tiles_per_split;
  return mfma;
}

}  // namespace hfgb
}  // namespace sel

extern "C" {

int sel_hfg_conv_bwd_kernel(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, int wgrad) {
  using namespace sel::hfgb;
  BArgs a;
  if (int rc = check("sel_hfg_conv_bwd_kernel", d, in_dtype, out_dtype, a)) return rc;
  if (!wgrad) return pick_data(a, in_dtype, out_dtype);
  const int m = plan_wgrad(a, in_dtype, out_dtype);
  SEL_REQUIRE(m >= 0, SEL_ERR_UNSUPPORTED, "sel_hfg_conv_bwd_kernel: shape too large");
  return m;
}

int sel_hfg_conv_bwd_data(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* gout, const void* out,
                          const void* x, const void* wdpack, const void* gskip, float skip_scale, void* gin,
                          sel_stream_t stream) {
  using namespace sel::hfgb;
  BArgs a;
  if (int rc = check("sel_hfg_conv_bwd_data", d, in_dtype, out_dtype, a)) return rc;
  SEL_REQUIRE(gout && wdpack && gin, SEL_ERR_ARG, "sel_hfg_conv_bwd_data: null pointer");
  SEL_REQUIRE(x || d->act_slope == 1.f, SEL_ERR_ARG, "sel_hfg_conv_bwd_data: act_slope %g needs the saved input x",
              double(d->act_slope));
  SEL_REQUIRE(out || !d->tanh_out, SEL_ERR_ARG, "sel_hfg_conv_bwd_data: tanh_out needs the saved output");
  a.skip_scale = skip_scale;
  SEL_REQUIRE(sel::initialized(), SEL_ERR_STATE, "sel_init() has not succeeded");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  a.vec = in_dtype == SEL_BF16 && a.Ng % 8 == 0 && aligned16(gout) && aligned16(wdpack);
  const int wn = pick_data(a, in_dtype, out_dtype);
  if (wn) {
    const int64_t span = BM + int64_t(a.K - 1) * a.dil;
    const size_t lds = size_t(span) * (a.CK + 8) * 2;
    const auto* g = static_cast<const __bf16*>(gout);
    const auto* xp = static_cast<const __bf16*>(x);
    const auto* w = static_cast<const __bf16*>(wdpack);
    const auto* sk = static_cast<const __bf16*>(gskip);
    auto* gi = static_cast<__bf16*>(gin);
    dim3 grid(unsigned((a.rows / a.T) * a.tps), unsigned((a.Cg + 16 * wn - 1) / (16 * wn)),
              unsigned(a.igs ? a.G : 1));
    if (wn == 4) hipLaunchKernelGGL(k_bwd_data_mfma<4>, grid, dim3(256), lds, s, a, g, xp, w, sk, gi);
    else if (wn == 2) hipLaunchKernelGGL(k_bwd_data_mfma<2>, grid, dim3(256), lds, s, a, g, xp, w, sk, gi);
    else hipLaunchKernelGGL(k_bwd_data_mfma<1>, grid, dim3(256), lds, s, a, g, xp, w, sk, gi);
  } else {
    const int64_t total = a.rows * a.ldin;
    SEL_REQUIRE(total < (int64_t(1) << 39), SEL_ERR_UNSUPPORTED, "sel_hfg_conv_bwd_data: too many outputs");
    dim3 grid(unsigned((total + 255) / 256));
    if (in_dtype == SEL_F32)
      hipLaunchKernelGGL((k_bwd_data_valu<float, float>), grid, dim3(256), 0, s, a, static_cast<const float*>(gout),
                         static_cast<const float*>(out), static_cast<const float*>(x),
                         static_cast<const float*>(wdpack), static_cast<const float*>(gskip),
                         static_cast<float*>(gin));
    else if (out_dtype == SEL_F32)
      hipLaunchKernelGGL((k_bwd_data_valu<__bf16, float>), grid, dim3(256), 0, s, a, static_cast<const float*>(gout),
                         static_cast<const float*>(out), static_cast<const __bf16*>(x),
                         static_cast<const __bf16*>(wdpack), static_cast<const __bf16*>(gskip),
                         static_cast<__bf16*>(gin));
    else
      hipLaunchKernelGGL((k_bwd_data_valu<__bf16, __bf16>), grid, dim3(256), 0, s, a,
                         static_cast<const __bf16*>(gout), static_cast<const __bf16*>(out),
                         static_cast<const __bf16*>(x), static_cast<const __bf16*>(wdpack),
                         static_cast<const __bf16*>(gskip), static_cast<__bf16*>(gin));
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

size_t sel_hfg_conv_wgrad_workspace(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype) {
  using namespace sel::hfgb;
  BArgs a;
  if (check("sel_hfg_conv_wgrad_workspace", d, in_dtype, out_dtype, a)) return 0;
  if (plan_wgrad(a, in_dtype, out_dtype) < 0) return 0;
  return size_t(a.nsplit) * size_t(a.per + a.N) * sizeof(float);
}

int sel_hfg_conv_wgrad(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* gout, const void* out,
                       const void* x, float* gwpack, float* gbias, void* ws, size_t ws_bytes, sel_stream_t stream) {
  using namespace sel::hfgb;
  BArgs a;
  if (int rc = check("sel_hfg_conv_wgrad", d, in_dtype, out_dtype, a)) return rc;
  SEL_REQUIRE(gout && x && gwpack && ws, SEL_ERR_ARG, "sel_hfg_conv_wgrad: null pointer");
  SEL_REQUIRE(out || !d->tanh_out, SEL_ERR_ARG, "sel_hfg_conv_wgrad: tanh_out needs the saved output");
  SEL_REQUIRE((gbias != nullptr) == (d->bias_period > 0), SEL_ERR_ARG,
              "sel_hfg_conv_wgrad: bias_period %d goes with a bias gradient, 0 with none", d->bias_period);
  const int mfma = plan_wgrad(a, in_dtype, out_dtype);
  SEL_REQUIRE(mfma >= 0, SEL_ERR_UNSUPPORTED, "sel_hfg_conv_wgrad: shape too large");
  const size_t need = size_t(a.nsplit) * size_t(a.per + a.N) * sizeof(float);
  SEL_REQUIRE(ws_bytes >= need, SEL_ERR_ARG, "sel_hfg_conv_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
  SEL_REQUIRE(sel::initialized(), SEL_ERR_STATE, "sel_init() has not succeeded");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(ws);
  a.vec = in_dtype == SEL_BF16 && a.Ng % 8 == 0 && a.Cg % 8 == 0 && aligned16(gout) && aligned16(x);
  if (mfma) {
    dim3 grid(unsigned(a.nsplit), unsigned(a.K * a.ntn * a.ntc), unsigned(a.G));
    hipLaunchKernelGGL(k_wgrad_mfma, grid, dim3(256), 0, s, a, static_cast<const __bf16*>(gout),
                       static_cast<const __bf16*>(x), part);
  } else {
    dim3 grid(unsigned((a.per + a.N + 255) / 256), unsigned(a.nsplit));
    if (in_dtype == SEL_F32)
      hipLaunchKernelGGL((k_wgrad_valu<float, float>), grid, dim3(256), 0, s, a, static_cast<const float*>(gout),
                         static_cast<const float*>(out), static_cast<const float*>(x), part);
    else if (out_dtype == SEL_F32)
      hipLaunchKernelGGL((k_wgrad_valu<__bf16, float>), grid, dim3(256), 0, s, a, static_cast<const float*>(gout),
                         static_cast<const float*>(out), static_cast<const __bf16*>(x), part);
    else
      hipLaunchKernelGGL((k_wgrad_valu<__bf16, __bf16>), grid, dim3(256), 0, s, a, static_cast<const __bf16*>(gout),
                         static_cast<const __bf16*>(out), static_cast<const __bf16*>(x), part);
  }
  SEL_LAUNCH_CHECK();
  const int64_t nfin = a.per + (gbias ? a.bias_period : 0);
  hipLaunchKernelGGL(k_wgrad_finish, dim3(unsigned((nfin + 255) / 256)), dim3(256), 0, s, a, part, gwpack, gbias);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
