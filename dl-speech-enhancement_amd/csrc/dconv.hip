// HiFi-GAN multi-scale + multi-period discriminator on gfx950
// (models/vocoder/HiFiGAN.py:308-395, models/vocoder/modules/discriminator.py:26-447):
// the forward / adjoint primitive.  Its weight gradients are in
// dconv_wgrad.hip, the weight packing in dconv_pack.hip, the front-end data
// movement and the GAN losses in gan.hip.
//
// Every discriminator layer — the grouped, strided k41 Conv1d of the MSD, the
// (k,1) Conv2d of the MPD (a 1-D conv along T/p with the p columns as extra
// sequences), the dense k5/k3/k2 output convs — and every adjoint is ONE
// primitive (include/sel.h sel_dconv_desc):
//
//   out[b, j, col(g, o)] = sum_{i<K, r<S, c<Cg} Wp[g][o][i][r][c] * x[b, j+q0+i, r*Cs + g*Cg + c]
//
// over channels-last rows.  A stride-s conv is run on the PHASE VIEW of its
// input (rows of s consecutive samples: x[b, s*t + r, c] = view[b, t, r*C + c],
// a free reinterpretation when the row count is padded to a multiple of s), so
// it becomes a stride-1 conv with ceil(K/s)+1 taps over s*C channels and no
// wasted output rows; its adjoint is the same primitive on gout with So = s
// output phases.  Groups index disjoint channel slices, so no MFMA lane ever
// multiplies a structural zero of a grouped weight (a group narrower than the
// 32-wide MFMA tile is padded to 32 output channels; only the MSD's 8-input /
// 16-output-channel layer pays that, 2x on 4% of the flops).
//
//   MFMA kernel (Cg % 8 == 0): v_mfma_f32_32x32x16_bf16 (bf16 path) or
//     v_mfma_f32_32x32x2_f32 (exact-fp32 parity path).  Reduction vectors are
//     8 consecutive channels of one (tap, phase): each 32-lane half of a wave
//     feeds one vector per MFMA.  The input span of a BM-row tile is staged once
//     per 32-channel chunk and re-read by every tap; weights are staged per tap
//     group.  Epilogue: + bias, LeakyReLU, or (+ res) * LeakyReLU'(aux) for the
//     adjoint, rows past Tvalid written as exact zeros (the next layer's padding).
//   VALU kernel: the 1-channel input / 1-channel output layers (first and last
//     conv of every sub-discriminator and their adjoints), where a 32-wide MFMA
//     tile would be 1/32 useful.
//   Weight gradient: dconv_wgrad.hip.
#include <algorithm>

#include "conv_common.h"  // dconv_ws_*: the layers that run on conv.hip's warp-specialised kernels
#include "dconv_common.h"

namespace sel {
namespace dconv {

// XCD-aware tile order of the row-tile x (group, column tile) grids: the
// launcher rounds grid.x (row tiles) up to a multiple of 8; linear block ids
// are dealt round-robin to the 8 XCDs, so decoding id -> (xcd = id % 8, slot =
// id / 8) -> (row tile 8 (slot / ny) + xcd, y = slot % ny) puts every (group,
// column) block of one row tile on ONE XCD, one after the other: the input rows
// they all read (a grouped layer's blocks each read a 64-B slice of every row)
// are fetched into that XCD's L2 once.  false: a padding block (row tile >= nx).
// (C5, alternating in one call: 45.14 / 45.05 ms per step against 45.21 / 45.24
// with the plain 2-D order)
__device__ __forceinline__ bool xcd_rowtile(int nx, int& rt, int& y) {
  const int ny = gridDim.y;
  const int64_t id = int64_t(blockIdx.y) * gridDim.x + blockIdx.x;
  const int64_t slot = id >> 3;
  rt = int((slot / ny) * 8 + (id & 7));
  y = int(slot % ny);
  return rt < nx;
}

__device__ __forceinline__ float leaky(float v, float s) { return v > 0.f ? v : v * s; }
__device__ __forceinline__ float leaky_grad(float y, float s) { return y > 0.f ? 1.f : s; }

template <typename T> struct Elt;
template <> struct Elt<__bf16> { static constexpr int VEC = 8; static constexpr int P = 40; };  // 80-B LDS rows
template <> struct Elt<float> { static constexpr int VEC = 4; static constexpr int P = 36; };   // 144-B LDS rows

constexpr int CH = 32;  // reduction channels per staged chunk
constexpr int KC = 8;   // taps per staged weight group

// ---------------------------------------------------------------------------
// MFMA primitive.  Block = BM output rows of one sequence x BN local output
// channels of one group; 4 waves as 2 x 2 (wave tile BM/2 x BN/2, 32x32 MFMA
// sub-tiles).  LDS: x span [BM + K - 1][P] of the current 32-channel chunk,
// weights [BN][KC][P] of the current tap group.
// ---------------------------------------------------------------------------
// Epilogue of one 32x32 accumulator (operands swapped: lane -> output row
// lane & 31, element e -> output channel ob + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)):
// + bias, + res, * LeakyReLU'(aux), LeakyReLU; rows past Tvalid written as exact
// zeros.  bf16 with contiguous output columns (col = col0 + o - o0): each run
// of 4 channels is one 8-byte load / store; otherwise per element.
template <typename T>
__device__ __forceinline__ void dconv_epilogue(const D& d, int g, int ob, int no_per_g, int64_t orow, bool valid,
                                               const floatx16& a, const float* __restrict__ bias,
                                               const T* __restrict__ aux, const T* __restrict__ res,
                                               T* __restrict__ out, bool contig) {
  const int hl = (threadIdx.x & 63) >> 5;
  if constexpr (sizeof(T) == 2) {
    if (contig) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = ob + 8 * q + 4 * hl;
        if (o >= no_per_g) continue;  // no_per_g % 4 == 0 (contig)
        const int64_t col = out_col(d, g, o);
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 rv = {}, av = {}, ov;
        if (valid && res) rv = *reinterpret_cast<const bf16x4*>(res + orow + col);
        if (valid && aux) av = *reinterpret_cast<const bf16x4*>(aux + orow + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = 0.f;
          if (valid) {
            v = a[4 * q + e];
            if (bias) v += bias[col + e];
            if (res) v += float(rv[e]);
            if (aux) v *= leaky_grad(float(av[e]), d.slope);
            if (d.act) v = leaky(v, d.slope);
          }
          ov[e] = __bf16(v);
        }
        *reinterpret_cast<bf16x4*>(out + orow + col) = ov;
      }
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int o = ob + (e & 3) + 8 * (e >> 2) + 4 * hl;
    if (o >= no_per_g) continue;
    const int64_t col = out_col(d, g, o);
    float v = 0.f;
    if (valid) {
      v = a[e];
      if (bias) v += bias[col];
      if (res) v += to_f(res[orow + col]);
      if (aux) v *= leaky_grad(to_f(aux[orow + col]), d.slope);
      if (d.act) v = leaky(v, d.slope);
    }
    out[orow + col] = from_f<T>(v);
  }
}

// output columns of a group contiguous in runs of 4 (8-byte aligned)
__device__ __forceinline__ bool dconv_contig4(const D& d) {
  return (d.So == 1 || d.Ns == d.Ng) && (d.Ng & 3) == 0 && (d.ldo & 3) == 0 && (d.G == 1 || d.So == 1);
}

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256) void k_dconv_mfma(D d, const T* __restrict__ x, const T* __restrict__ wp,
                                                    const float* __restrict__ bias, const T* __restrict__ aux,
                                                    const T* __restrict__ res, T* __restrict__ out) {
  constexpr int P = Elt<T>::P;
  constexpr int VEC = Elt<T>::VEC;
  constexpr int WAVES_N = BN / 32, WAVES_M = 4 / WAVES_N;
  constexpr int TM = BM / (32 * WAVES_M);
  static_assert(TM >= 1 && WAVES_N * WAVES_M == 4, "tile");
  extern __shared__ __align__(16) unsigned char smem[];
  T* const xs = reinterpret_cast<T*>(smem);
  const int span = BM + d.K - 1;
  T* const ws = xs + span * P;  // [BN][KC][P]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int tps = (d.Tvo + BM - 1) / BM;
  int rt_, by_;
  if (!xcd_rowtile(d.B * tps, rt_, by_)) return;
  const int b = rt_ / tps;
  const int j0 = (rt_ % tps) * BM;
  const int no_per_g = d.So * d.Ng;
  const int ntile_g = (no_per_g + BN - 1) / BN;
  const int g = by_ / ntile_g;
  const int o0 = (by_ % ntile_g) * BN;
  const int64_t xrow0 = int64_t(b) * d.Tvs;
  const int nred = d.S * d.Cg;  // reduction channels per tap

  floatx16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  // this lane's output rows (B operand column) and channel (A operand row)
  int lrow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) lrow[i] = wm * (BM / WAVES_M) + i * 32 + (lane & 31);
  const int half = lane >> 5;
  const int nw_ = wn * 32 + (lane & 31);
  const int vpr = CH / VEC;

  for (int cc = 0; cc < nred; cc += CH) {
    const int chn = nred - cc < CH ? nred - cc : CH;  // multiple of 8 (host-checked)
    __syncthreads();
    // stage x span rows [j0 + q0, j0 + q0 + span) x chunk channels (vectors of VEC)
    for (int idx = tid; idx < span * vpr; idx += 256) {
      const int rr = idx / vpr, v = idx % vpr;
      const int t = j0 + d.q0 + rr;
      const int ch = cc + v * VEC;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (t >= 0 && t < d.Tv && v * VEC < chn) {
        const int rph = ch / d.Cg, c = ch - rph * d.Cg;
        val = *reinterpret_cast<const uint4*>(x + (xrow0 + t) * d.ldx + in_col(d, g, rph, c));
      }
      *reinterpret_cast<uint4*>(xs + rr * P + v * VEC) = val;
    }
    for (int k0 = 0; k0 < d.K; k0 += KC) {
      const int kn = d.K - k0 < KC ? d.K - k0 : KC;
      if (k0) __syncthreads();
      for (int idx = tid; idx < BN * KC * vpr; idx += 256) {
        const int v = idx % vpr, kk = (idx / vpr) % KC, n = idx / (vpr * KC);
        uint4 val = make_uint4(0, 0, 0, 0);
        if (kk < kn && o0 + n < no_per_g && v * VEC < chn)
          val = *reinterpret_cast<const uint4*>(
              wp + ((int64_t(g) * no_per_g + o0 + n) * d.K + k0 + kk) * nred + cc + v * VEC);
        *reinterpret_cast<uint4*>(ws + (n * KC + kk) * P + v * VEC) = val;
      }
      __syncthreads();
      for (int kk = 0; kk < kn; ++kk) {
        const int k = k0 + kk;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int h = 0; h < CH / 16; ++h) {
            if (h * 16 >= chn) break;
            const int co = 16 * h + 8 * half;
            const bf16x8 bw = *reinterpret_cast<const bf16x8*>(ws + (nw_ * KC + kk) * P + co);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
              const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + (lrow[i] + k) * P + co);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, af, acc[i], 0, 0, 0);
            }
          }
        } else {
          for (int c2 = 0; c2 < chn; c2 += 2) {
            const int co = c2 + half;
            const float bw = ws[(nw_ * KC + kk) * P + co];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
              const float af = xs[(lrow[i] + k) * P + co];
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(bw, af, acc[i], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // epilogue (operands swapped: lane -> output row lane & 31 of its sub-tile,
  // element e -> channel (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the wave's 32)
  const bool contig = dconv_contig4(d);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int j = j0 + lrow[i];
    if (j >= d.Tvo) continue;
    const int64_t orow = (int64_t(b) * d.Tvo + j) * d.ldo;
    dconv_epilogue<T>(d, g, o0 + wn * 32, no_per_g, orow, j < d.Tvalid, acc[i], bias, aux, res, out, contig);
  }
}

// ---------------------------------------------------------------------------
// k_dconv_mfma with a register-prefetched pipeline (bf16): the (32-channel
// chunk, 8-tap group) stages run in the same order with the same MFMAs (same
// bits), but the next stage's weight slice (and, at a chunk boundary, the next
// input span) is fetched into registers while the current stage's MFMAs run;
// k_dconv_mfma staged both synchronously, exposing a load latency per stage
// (the MSD's 41-tap grouped convs: 2 chunks x 6 tap groups per tile).
// ---------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(256) void k_dconv_gpf(D d, const __bf16* __restrict__ x, const __bf16* __restrict__ wp,
                                                   const float* __restrict__ bias, const __bf16* __restrict__ aux,
                                                   const __bf16* __restrict__ res, __bf16* __restrict__ out) {
  constexpr int P = Elt<__bf16>::P;
  constexpr int WAVES_N = BN / 32, WAVES_M = 4 / WAVES_N;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int XV = ((BM + KC * 8) * 4 + 255) / 256;  // span rows (<= BM + K - 1 <= BM + 63) x 4 vectors
  constexpr int WV = (BN * KC * 4 + 255) / 256;
  static_assert(TM >= 1 && WAVES_N * WAVES_M == 4, "tile");
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);
  const int span = BM + d.K - 1;
  __bf16* const ws = xs + span * P;  // [BN][KC][P]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int tps = (d.Tvo + BM - 1) / BM;
  int rt_, by_;
  if (!xcd_rowtile(d.B * tps, rt_, by_)) return;
  const int b = rt_ / tps;
  const int j0 = (rt_ % tps) * BM;
  const int no_per_g = d.So * d.Ng;
  const int ntile_g = (no_per_g + BN - 1) / BN;
  const int g = by_ / ntile_g;
  const int o0 = (by_ % ntile_g) * BN;
  const int64_t xrow0 = int64_t(b) * d.Tvs;
  const int nred = d.S * d.Cg;
  const int nchunk = (nred + CH - 1) / CH;
  const int ntg = (d.K + KC - 1) / KC;
  const int nstage = nchunk * ntg;

  floatx16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  int lrow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) lrow[i] = wm * (BM / WAVES_M) + i * 32 + (lane & 31);
  const int half = lane >> 5;
  const int nw_ = wn * 32 + (lane & 31);

  uint4 xr[XV], wr[WV];
  bool xok[XV], wok[WV];
  auto load_x = [&](int cc) {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int idx = tid + u * 256;
      const int rr = idx >> 2, v = idx & 3;
      const int t = j0 + d.q0 + rr;
      const int ch = cc + v * 8;
      xok[u] = rr < span && t >= 0 && t < d.Tv && ch < nred;
      const int rph = (xok[u] ? ch : 0) / d.Cg, c = (xok[u] ? ch : 0) - rph * d.Cg;
      if ((u * 256) / 4 < span)
        xr[u] = *reinterpret_cast<const uint4*>(x + (xrow0 + (xok[u] ? t : 0)) * d.ldx + in_col(d, g, rph, c));
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int idx = tid + u * 256;
      const int rr = idx >> 2, v = idx & 3;
      if (rr >= span) continue;
      *reinterpret_cast<uint4*>(xs + rr * P + v * 8) = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
    }
  };
  auto load_w = [&](int cc, int k0) {
    const int kn = d.K - k0 < KC ? d.K - k0 : KC;
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int idx = tid + u * 256;
      const int v = idx & 3, kk = (idx >> 2) % KC, n = idx / (4 * KC);
      wok[u] = n < BN && kk < kn && o0 + n < no_per_g && cc + v * 8 < nred;
      wr[u] = *reinterpret_cast<const uint4*>(
          wp + ((int64_t(g) * no_per_g + (wok[u] ? o0 + n : 0)) * d.K + (wok[u] ? k0 + kk : 0)) * nred +
          (wok[u] ? cc + v * 8 : 0));
    }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int idx = tid + u * 256;
      const int v = idx & 3, kk = (idx >> 2) % KC, n = idx / (4 * KC);
      if (n >= BN) continue;
      *reinterpret_cast<uint4*>(ws + (n * KC + kk) * P + v * 8) = wok[u] ? wr[u] : make_uint4(0, 0, 0, 0);
    }
  };

  load_x(0);
  load_w(0, 0);
  for (int st = 0; st < nstage; ++st) {
    const int ci = st / ntg, tg = st - ci * ntg;
    const int cc = ci * CH, k0 = tg * KC;
    __syncthreads();  // every wave is done with the previous stage's LDS
    if (tg == 0) store_x();
    store_w();
    __syncthreads();
    if (st + 1 < nstage) {  // next stage's operands in flight during this stage's MFMAs
      const int ci1 = (st + 1) / ntg, tg1 = (st + 1) - ci1 * ntg;
      if (tg1 == 0) load_x(ci1 * CH);
      load_w(ci1 * CH, tg1 * KC);
    }
    const int kn = d.K - k0 < KC ? d.K - k0 : KC;
    const int chn = nred - cc < CH ? nred - cc : CH;
    for (int kk = 0; kk < kn; ++kk) {
      const int k = k0 + kk;
#pragma unroll
      for (int h = 0; h < CH / 16; ++h) {
        if (h * 16 >= chn) break;
        const int co = 16 * h + 8 * half;
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(ws + (nw_ * KC + kk) * P + co);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + (lrow[i] + k) * P + co);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, af, acc[i], 0, 0, 0);
        }
      }
    }
  }

  const bool contig = dconv_contig4(d);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int j = j0 + lrow[i];
    if (j >= d.Tvo) continue;
    const int64_t orow = (int64_t(b) * d.Tvo + j) * d.ldo;
    dconv_epilogue<__bf16>(d, g, o0 + wn * 32, no_per_g, orow, j < d.Tvalid, acc[i], bias, aux, res, out, contig);
  }
}

// ---------------------------------------------------------------------------
// Register-prefetched MFMA primitive for one group with a contiguous reduction
// row (G == 1, S == 1 or Cs == Cg: every MPD layer and the MSD's dense ones)
// and K <= 8 taps: the next 32-channel chunk's input span and ALL K weight
// slices are fetched into registers while the current chunk's MFMAs run (the
// tap-grouped kernel above stages each chunk synchronously: ~5% of the bf16
// peak on the MPD's 512/1024-wide layers, profiles/r2_c5_kernel_stats.md).
// ---------------------------------------------------------------------------
constexpr int PF_KMAX = 8;

template <int BM, int BN>
__global__ __launch_bounds__(256) void k_dconv_pf(D d, const __bf16* __restrict__ x, const __bf16* __restrict__ wp,
                                                  const float* __restrict__ bias, const __bf16* __restrict__ aux,
                                                  const __bf16* __restrict__ res, __bf16* __restrict__ out) {
  constexpr int P = Elt<__bf16>::P;
  constexpr int WAVES_N = BN / 32, WAVES_M = 4 / WAVES_N;
  constexpr int TM = BM / (32 * WAVES_M);
  constexpr int XV = ((BM + PF_KMAX - 1) * 4 + 255) / 256;
  constexpr int WV = (PF_KMAX * BN * 4 + 255) / 256;
  static_assert(TM >= 1 && WAVES_N * WAVES_M == 4, "tile");
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);
  const int span = BM + d.K - 1;
  __bf16* const ws = xs + span * P;  // [K][BN][P]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int hl = lane >> 5;
  const int tps = (d.Tvo + BM - 1) / BM;
  int rt_, by_;
  if (!xcd_rowtile(d.B * tps, rt_, by_)) return;
  const int b = rt_ / tps;
  const int j0 = (rt_ % tps) * BM;
  const int no_per_g = d.So * d.Ng;
  const int o0 = by_ * BN;
  const int nred = d.S * d.Cg;
  const int nchunk = (nred + CH - 1) / CH;

  const __bf16* xsrc[XV];
  bool xok[XV];
  int xsub[XV];
#pragma unroll
  for (int u = 0; u < XV; ++u) {
    const int v = tid + u * 256, rr = v >> 2;
    const int t = j0 + d.q0 + rr;
    xok[u] = rr < span && t >= 0 && t < d.Tv;
    xsub[u] = (v & 3) * 8;
    xsrc[u] = x + (int64_t(b) * d.Tvs + (xok[u] ? t : 0)) * d.ldx + xsub[u];
  }
  const __bf16* wsrc[WV];
  bool wok[WV];
#pragma unroll
  for (int u = 0; u < WV; ++u) {
    const int v = tid + u * 256;
    const int k = v / (BN * 4), n = (v >> 2) % BN;
    wok[u] = k < d.K && o0 + n < no_per_g;
    wsrc[u] = wp + (int64_t(wok[u] ? o0 + n : 0) * d.K + (wok[u] ? k : 0)) * nred + (v & 3) * 8;
  }
  uint4 xr[XV], wr[WV];
  auto load = [&](int cc) {
#pragma unroll
    for (int u = 0; u < XV; ++u)
      if ((u * 256) / 4 < span) xr[u] = *reinterpret_cast<const uint4*>(xsrc[u] + (cc + xsub[u] < nred ? cc : 0));
#pragma unroll
    for (int u = 0; u < WV; ++u)
      if ((u * 256) / (BN * 4) < d.K) wr[u] = *reinterpret_cast<const uint4*>(wsrc[u] + (cc + (((tid + u * 256) & 3) * 8) < nred ? cc : 0));
  };
  auto store = [&](int cc) {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      if ((v >> 2) >= span) continue;
      const uint4 val = (xok[u] && cc + xsub[u] < nred) ? xr[u] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(xs + (v >> 2) * P + xsub[u]) = val;
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int v = tid + u * 256;
      const int k = v / (BN * 4), n = (v >> 2) % BN;
      if (k >= d.K) continue;
      const uint4 val = (wok[u] && cc + (v & 3) * 8 < nred) ? wr[u] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(ws + (k * BN + n) * P + (v & 3) * 8) = val;
    }
  };

  floatx16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  int lrow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) lrow[i] = wm * (BM / WAVES_M) + i * 32 + (lane & 31);
  const int nw_ = wn * 32 + (lane & 31);

  load(0);
  for (int ch = 0; ch < nchunk; ++ch) {
    const int cc = ch * CH;
    if (ch) __syncthreads();
    store(cc);
    __syncthreads();
    if (ch + 1 < nchunk) load(cc + CH);
    const int chn = nred - cc < CH ? nred - cc : CH;
    for (int k = 0; k < d.K; ++k) {
#pragma unroll
      for (int h = 0; h < CH / 16; ++h) {
        if (h * 16 >= chn) break;
        const int co = 16 * h + 8 * hl;
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(ws + (k * BN + nw_) * P + co);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + (lrow[i] + k) * P + co);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, af, acc[i], 0, 0, 0);
        }
      }
    }
  }

  // epilogue as k_dconv_mfma
  const bool contig = dconv_contig4(d);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int j = j0 + lrow[i];
    if (j >= d.Tvo) continue;
    const int64_t orow = (int64_t(b) * d.Tvo + j) * d.ldo;
    dconv_epilogue<__bf16>(d, 0, o0 + wn * 32, no_per_g, orow, j < d.Tvalid, acc[i], bias, aux, res, out, contig);
  }
}

// ---------------------------------------------------------------------------
// VALU primitive (any Cg; used when S*Cg*K or the group output width is tiny).
// One thread per (row, output channel); the reduction walks (i, r, c).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_dconv_valu(D d, const T* __restrict__ x, const T* __restrict__ wp,
                                                    const float* __restrict__ bias, const T* __restrict__ aux,
                                                    const T* __restrict__ res, T* __restrict__ out) {
  const int no_per_g = d.So * d.Ng;
  const int64_t nout = int64_t(d.G) * no_per_g;
  const int64_t total = int64_t(d.B) * d.Tvo * nout;
  const int nred = d.S * d.Cg;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * 256) {
    const int64_t row = idx / nout;
    const int oc = int(idx - row * nout);
    const int g = oc / no_per_g, o = oc - g * no_per_g;
    const int b = int(row / d.Tvo), j = int(row - int64_t(b) * d.Tvo);
    const int64_t orow = row * d.ldo;
    const int64_t col = out_col(d, g, o);
    float v = 0.f;
    if (j < d.Tvalid) {
      const T* w = wp + (int64_t(g) * no_per_g + o) * d.K * nred;
      for (int i = 0; i < d.K; ++i) {
        const int t = j + d.q0 + i;
        if (t < 0 || t >= d.Tv) continue;
        const T* xr = x + (int64_t(b) * d.Tvs + t) * d.ldx;
        for (int r = 0; r < d.S; ++r)
          for (int c = 0; c < d.Cg; ++c) v += to_f(w[i * nred + r * d.Cg + c]) * to_f(xr[in_col(d, g, r, c)]);
      }
      if (bias) v += bias[col];
      if (res) v += to_f(res[orow + col]);
      if (aux) v *= leaky_grad(to_f(aux[orow + col]), d.slope);
      if (d.act) v = leaky(v, d.slope);
    }
    out[orow + col] = from_f<T>(v);
  }
}

// Short-reduction primitive (K * S * Cg <= 64, one group, single output phase,
// Ng % 8 == 0): the 1-channel-input convs (MSD k15, MPD k5/s3 -> 2 taps x 3
// phases) and the adjoints of the 1-channel-output convs.  One thread = one
// output row x 8 consecutive channels: the row's input window in registers, the
// weights in LDS (fp32), one 16-B (bf16) / 32-B (fp32) store.

template <typename T, int KR>
__global__ __launch_bounds__(256) void k_dconv_short(D d, const T* __restrict__ x, const T* __restrict__ wp,
                                                     const float* __restrict__ bias, const T* __restrict__ aux,
                                                     const T* __restrict__ res, T* __restrict__ out) {
  constexpr int RW = 4;   // rows per thread: each weight read from LDS serves RW rows
  extern __shared__ float wsh[];  // [K * nred][Ng] (transposed: a thread's 8 channels are 2 float4)
  const int nred = d.S * d.Cg;
  for (int e = threadIdx.x; e < d.Ng * KR; e += 256) {
    const int n = e / KR, k = e - n * KR;
    wsh[k * d.Ng + n] = to_f(wp[e]);
  }
  __syncthreads();
  // tap offset and input column of reduction element e (kernel-uniform: hoisted
  // out of the row loop, where the runtime divisions cost ~60 VALU per element)
  int tap[KR], col[KR];
#pragma unroll
  for (int e = 0; e < KR; ++e) {
    const int i = e / nred, rc = e - i * nred;
    const int r = rc / d.Cg, c = rc - r * d.Cg;
    tap[e] = d.q0 + i;
    col[e] = int(in_col(d, 0, r, c));
  }
  const int n8 = d.Ng / 8;
  const int rows = d.B * d.Tvo;  // < 2^31 (host check)
  const int total = (rows + RW - 1) / RW * n8;
  for (int idx = int(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += int(gridDim.x) * 256) {
    const int rg = idx / n8;
    const int n0 = (idx - rg * n8) * 8;
    float xw[RW][KR];
    int64_t orow[RW];
    bool valid[RW];
    int row = rg * RW, b = row / d.Tvo, j = row - b * d.Tvo;
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      orow[q] = row < rows ? int64_t(row) * d.ldo : -1;
      valid[q] = row < rows && j < d.Tvalid;
      const T* xb = x + int64_t(b) * d.Tvs * d.ldx;
#pragma unroll
      for (int e = 0; e < KR; ++e) {
        const int t = j + tap[e];
        xw[q][e] = (valid[q] && t >= 0 && t < d.Tv) ? to_f(xb[int64_t(t) * d.ldx + col[e]]) : 0.f;
      }
      ++row;
      if (++j == d.Tvo) j = 0, ++b;
    }
    float acc[RW][8];
#pragma unroll
    for (int q = 0; q < RW; ++q)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[q][c] = 0.f;
#pragma unroll
    for (int e = 0; e < KR; ++e) {
      const float4 w0 = *reinterpret_cast<const float4*>(wsh + e * d.Ng + n0);
      const float4 w1 = *reinterpret_cast<const float4*>(wsh + e * d.Ng + n0 + 4);
      const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int q = 0; q < RW; ++q)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[q][c] = fmaf(w[c], xw[q][e], acc[q][c]);
    }
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      if (orow[q] < 0) continue;
      T ov[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float a = 0.f;
        if (valid[q]) {
          const int64_t col = n0 + c;
          a = acc[q][c];
          if (bias) a += bias[col];
          if (res) a += to_f(res[orow[q] + col]);
          if (aux) a *= leaky_grad(to_f(aux[orow[q] + col]), d.slope);
          if (d.act) a = leaky(a, d.slope);
        }
        ov[c] = from_f<T>(a);
      }
      if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(out + orow[q] + n0) = *reinterpret_cast<uint4*>(ov);
      } else {
        *reinterpret_cast<uint4*>(out + orow[q] + n0) = *reinterpret_cast<uint4*>(ov);
        *reinterpret_cast<uint4*>(out + orow[q] + n0 + 4) = *reinterpret_cast<uint4*>(ov + 4);
      }
    }
  }
}

// Staged form of the short-reduction forward for a contiguous phase view (G = 1,
// Cs = Cg, ldx = S*Cg = NR: the 1-channel-input convs): reduction element
// e = i*NR + rc of output row j reads x[j + q0 + i][rc], i.e. the flat window
// xs[(j - j0)*NR + e] of a tile staged once in LDS.  k_dconv_short issues KR
// per-lane global loads per row (the MSD's k15 1 -> 128 conv: 60 loads per
// thread, bound by the texture unit's address rate at 645 us for 393 MB of
// output); here a thread's RW rows read one (RW + K - 1)*NR-float window from LDS.
template <typename T, int K, int NR>
__global__ __launch_bounds__(256) void k_dconv_shortx(D d, const T* __restrict__ x, const T* __restrict__ wp,
                                                      const float* __restrict__ bias, const T* __restrict__ aux,
                                                      const T* __restrict__ res, T* __restrict__ out) {
  constexpr int KR = K * NR, RW = 8, XW = (RW + K - 1) * NR;
  extern __shared__ float sh[];
  float* const wsh = sh;            // [KR][Ng]
  float* const xs = sh + KR * d.Ng;  // [(RB + K - 1) * NR]
  for (int e = threadIdx.x; e < d.Ng * KR; e += 256) {
    const int n = e / KR, k = e - n * KR;
    wsh[k * d.Ng + n] = to_f(wp[e]);
  }
  const int n8 = d.Ng / 8, RL = 256 / n8, RB = RL * RW;
  const int rl = threadIdx.x / n8, n0 = (threadIdx.x - rl * n8) * 8;
  const int tps = (d.Tvo + RB - 1) / RB, ntiles = d.B * tps;
  // (a one-tile-ahead register fetch of the window was measured neutral on C5
  // in round 2 and dropped)
  const int np = (RB + K - 1) * NR;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, j0 = (tile - b * tps) * RB;
    __syncthreads();  // the previous tile's window reads are done (and the weights are in)
    for (int p = threadIdx.x; p < np; p += 256) {
      const int t = j0 + d.q0 + p / NR;
      xs[p] = (t >= 0 && t < d.Tv) ? to_f(x[(int64_t(b) * d.Tvs + t) * NR + p % NR]) : 0.f;
    }
    __syncthreads();
    const int jr = rl * RW;
    if (j0 + jr >= d.Tvo) continue;
    float xw[XW];
#pragma unroll
    for (int u = 0; u < XW; ++u) xw[u] = xs[jr * NR + u];
    // channel pairs as 2-vectors: one packed fp32 FMA (v_pk_fma_f32) per pair,
    // per element the same fused multiply-add as fmaf, so bit-identical
    typedef float shx_f2 __attribute__((ext_vector_type(2)));
    shx_f2 acc2[RW][4];
#pragma unroll
    for (int q = 0; q < RW; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc2[q][c] = shx_f2{0.f, 0.f};
#pragma unroll
    for (int e = 0; e < KR; ++e) {
      const float4 w0 = *reinterpret_cast<const float4*>(wsh + e * d.Ng + n0);
      const float4 w1 = *reinterpret_cast<const float4*>(wsh + e * d.Ng + n0 + 4);
      const shx_f2 w[4] = {shx_f2{w0.x, w0.y}, shx_f2{w0.z, w0.w}, shx_f2{w1.x, w1.y}, shx_f2{w1.z, w1.w}};
#pragma unroll
      for (int q = 0; q < RW; ++q) {
        const float xv = xw[q * NR + e];
        const shx_f2 x2 = shx_f2{xv, xv};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc2[q][c] = __builtin_elementwise_fma(w[c], x2, acc2[q][c]);
      }
    }
    float acc[RW][8];
#pragma unroll
    for (int q = 0; q < RW; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[q][2 * c] = acc2[q][c].x, acc[q][2 * c + 1] = acc2[q][c].y;
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      const int j = j0 + jr + q;
      if (j >= d.Tvo) break;
      const int64_t orow = (int64_t(b) * d.Tvo + j) * d.ldo;
      const bool valid = j < d.Tvalid;
      T ov[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float a = 0.f;
        if (valid) {
          const int64_t col = n0 + c;
          a = acc[q][c];
          if (bias) a += bias[col];
          if (res) a += to_f(res[orow + col]);
          if (aux) a *= leaky_grad(to_f(aux[orow + col]), d.slope);
          if (d.act) a = leaky(a, d.slope);
        }
        ov[c] = from_f<T>(a);
      }
      if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(out + orow + n0) = *reinterpret_cast<uint4*>(ov);
      } else {
        *reinterpret_cast<uint4*>(out + orow + n0) = *reinterpret_cast<uint4*>(ov);
        *reinterpret_cast<uint4*>(out + orow + n0 + 4) = *reinterpret_cast<uint4*>(ov + 4);
      }
    }
  }
}

}  // namespace dconv
}  // namespace sel

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace sel;
using namespace sel::dconv;

namespace {

// The launch of every forward / adjoint kernel (they share one signature):
// typed pointers, the dynamic-LDS limit raised where a tile needs more than
// 64 KiB, the launch and its check.  Grid and LDS size are the caller's.
template <typename T>
using FwdKernel = void (*)(D, const T*, const T*, const float*, const T*, const T*, T*);

template <typename T>
int launch_fwd(FwdKernel<T> kern, dim3 grid, size_t lds, const sel_dconv_desc* d, const void* x, const void* wp,
               const float* bias, const void* aux, const void* res, void* out, hipStream_t s) {
  if (lds > 64 * 1024)
    SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, *d, static_cast<const T*>(x), static_cast<const T*>(wp), bias,
                     static_cast<const T*>(aux), static_cast<const T*>(res), static_cast<T*>(out));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

bool mfma_ok(const sel_dconv_desc* d, int dtype) {
  const int vec = dtype == SEL_BF16 ? 8 : 4;
  // 8-channel (bf16) / 4-channel (fp32) vectors may not straddle a phase or a
  // group.  A group narrower than the 32-wide MFMA tile still runs on the
  // matrix cores when its reduction is long (the 1-channel-output convs and the
  // adjoints of the 1-channel-input convs: K * S * Cg >= 256 products per output,
  // where the VALU kernel's per-thread strided row walk is far slower than a
  // 1/32-filled MFMA tile fed from LDS)
  const int width = d->So * d->Ng;
  return d->Cg % vec == 0 && d->Cs % vec == 0 && d->ldx % vec == 0 && (d->S * d->Cg) % 8 == 0 && d->K <= 64 &&
         (width >= 16 || d->K * d->S * d->Cg >= 256);
}

// Very narrow outputs with a short reduction (the MPD first layer's adjoint:
// 3 output phases x 1 channel from 2 taps x 32 channels of gout): one thread
// per output row computes all `width` outputs from 16-B input vectors, weights
// in LDS as fp32 (the generic VALU kernel walked the reduction with one 2-byte
// load per product and thread).  bf16, one group, contiguous reduction row.
template <int MAXW>
__global__ __launch_bounds__(256) void k_dconv_tiny(D d, const __bf16* __restrict__ x, const __bf16* __restrict__ wp,
                                                    const float* __restrict__ bias, const __bf16* __restrict__ aux,
                                                    const __bf16* __restrict__ res, __bf16* __restrict__ out) {
  extern __shared__ float wsm[];  // [width][K][nred]
  const int width = d.So * d.Ng, nred = d.S * d.Cg;
  for (int e = threadIdx.x; e < width * d.K * nred; e += 256) wsm[e] = float(wp[e]);
  __syncthreads();
  const int64_t rows = int64_t(d.B) * d.Tvo;
  for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row < rows; row += int64_t(gridDim.x) * 256) {
    const int b = int(row / d.Tvo), j = int(row - int64_t(b) * d.Tvo);
    const bool valid = j < d.Tvalid;
    float acc[MAXW];
#pragma unroll
    for (int o = 0; o < MAXW; ++o) acc[o] = 0.f;
    if (valid) {
      for (int i = 0; i < d.K; ++i) {
        const int t = j + d.q0 + i;
        if (t < 0 || t >= d.Tv) continue;
        const __bf16* xr = x + (int64_t(b) * d.Tvs + t) * d.ldx;
        for (int v = 0; v < nred; v += 8) {
          const uint4 raw = *reinterpret_cast<const uint4*>(xr + v);
          const __bf16* xv = reinterpret_cast<const __bf16*>(&raw);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xf = float(xv[e]);
#pragma unroll
            for (int o = 0; o < MAXW; ++o)
              if (o < width) acc[o] = fmaf(wsm[(o * d.K + i) * nred + v + e], xf, acc[o]);
          }
        }
      }
    }
    const int64_t orow = (int64_t(b) * d.Tvo + j) * d.ldo;
#pragma unroll
    for (int o = 0; o < MAXW; ++o) {
      if (o >= width) break;
      const int64_t col = out_col(d, 0, o);
      float v = 0.f;
      if (valid) {
        v = acc[o];
        if (bias) v += bias[col];
        if (res) v += float(res[orow + col]);
        if (aux) v *= leaky_grad(float(aux[orow + col]), d.slope);
        if (d.act) v = leaky(v, d.slope);
      }
      out[orow + col] = __bf16(v);
    }
  }
}

bool tiny_ok(const sel_dconv_desc* d, int dtype) {
  const int width = d->So * d->Ng, nred = d->S * d->Cg;
  return dtype == SEL_BF16 && d->G == 1 && (d->S == 1 || d->Cs == d->Cg) && width <= 4 && nred % 8 == 0 &&
         d->ldx % 8 == 0 && size_t(width) * d->K * nred * sizeof(float) <= 48 * 1024 && tune(31) != 1;
}

int launch_tiny(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                const void* res, void* out, hipStream_t s) {
  const int width = d->So * d->Ng, nred = d->S * d->Cg;
  const size_t lds = size_t(width) * d->K * nred * sizeof(float);
  const int64_t rows = int64_t(d->B) * d->Tvo;
  const unsigned blocks = unsigned(std::min<int64_t>((rows + 255) / 256, 4096));
  return launch_fwd<__bf16>(k_dconv_tiny<4>, dim3(blocks), lds, d, x, wp, bias, aux, res, out, s);
}

// gpf: the register-prefetched pipeline (plan_fwd's SEL_DPATH_GPF; bf16 only)
template <typename T, int BM, int BN>
int launch_mfma(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                const void* res, void* out, hipStream_t s, bool gpf) {
  constexpr int P = Elt<T>::P;
  const size_t lds = (size_t(BM + d->K - 1) * P + size_t(BN) * KC * P) * sizeof(T);
  SEL_REQUIRE(lds <= 160 * 1024, SEL_ERR_UNSUPPORTED, "dconv tile needs %zu B of LDS", lds);
  const int tps = (d->Tvo + BM - 1) / BM;
  const int ntg = (d->So * d->Ng + BN - 1) / BN;
  dim3 grid(unsigned((int64_t(d->B) * tps + 7) / 8 * 8), unsigned(ntg * d->G));  // xcd_rowtile
  if constexpr (sizeof(T) == 2) {
    if (gpf) return launch_fwd<__bf16>(k_dconv_gpf<BM, BN>, grid, lds, d, x, wp, bias, aux, res, out, s);
  }
  return launch_fwd<T>(k_dconv_mfma<T, BM, BN>, grid, lds, d, x, wp, bias, aux, res, out, s);
}

template <typename T>
int launch_valu(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                const void* res, void* out, hipStream_t s) {
  const int64_t total = int64_t(d->B) * d->Tvo * d->G * d->So * d->Ng;
  const unsigned blocks = unsigned(std::min<int64_t>((total + 255) / 256, 65536));
  return launch_fwd<T>(k_dconv_valu<T>, dim3(blocks), 0, d, x, wp, bias, aux, res, out, s);
}

bool short_ok(const sel_dconv_desc* d) {
  return d->G == 1 && d->So == 1 && d->Ng % 8 == 0 && d->ldo % 8 == 0 && short_kr_ok(d->K * d->S * d->Cg) &&
         int64_t(d->B) * d->Tvo + 4 < (int64_t(1) << 31) &&
         size_t(d->Ng) * d->K * d->S * d->Cg * sizeof(float) <= 64 * 1024;
}

// the staged kernel's (K, NR) instance for this layer; nullptr: use k_dconv_short
template <typename T>
FwdKernel<T> shortx_kernel(const sel_dconv_desc* d) {
  const int nr = d->S * d->Cg, n8 = d->Ng / 8;
  if (tune(18) == 1 || d->G != 1 || d->So != 1 || d->Cs != d->Cg || d->ldx != nr || d->Ng % 8 != 0 || n8 > 256 ||
      256 % n8 != 0)
    return nullptr;
#define SEL_DSX_PICK(K_, NR_) \
  if (d->K == K_ && nr == NR_) return k_dconv_shortx<T, K_, NR_>;
  SEL_DSHORTX_TABLE(SEL_DSX_PICK)
#undef SEL_DSX_PICK
  return nullptr;
}

template <typename T>
int launch_short(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                 const void* res, void* out, hipStream_t s) {
  if (auto kx = shortx_kernel<T>(d)) {
    // tune key 18: 1 = the unstaged kernel
    const int kr = d->K * d->S * d->Cg, rb = 256 / (d->Ng / 8) * 8;
    const size_t lds = (size_t(d->Ng) * kr + size_t(rb + d->K - 1) * d->S * d->Cg) * sizeof(float);
    const int64_t ntiles = int64_t(d->B) * ((d->Tvo + rb - 1) / rb);
    const unsigned blocks = unsigned(std::min<int64_t>(ntiles, 2048));
    return launch_fwd<T>(kx, dim3(blocks), lds, d, x, wp, bias, aux, res, out, s);
  }
  const int64_t total = (int64_t(d->B) * d->Tvo + 3) / 4 * (d->Ng / 8);
  const unsigned blocks = unsigned(std::min<int64_t>((total + 255) / 256, 16384));
  const int kr = d->K * d->S * d->Cg;
  const size_t lds = size_t(d->Ng) * kr * sizeof(float);
  FwdKernel<T> kern = kr == 2 ? k_dconv_short<T, 2> : kr == 3 ? k_dconv_short<T, 3> : kr == 6 ? k_dconv_short<T, 6>
                                                                                            : k_dconv_short<T, 15>;
  return launch_fwd<T>(kern, dim3(blocks), lds, d, x, wp, bias, aux, res, out, s);
}

template <int BM, int BN>
int launch_pf(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
              const void* res, void* out, hipStream_t s) {
  constexpr int P = Elt<__bf16>::P;
  const size_t lds = (size_t(BM + d->K - 1) + size_t(d->K) * BN) * P * sizeof(__bf16);
  const int tps = (d->Tvo + BM - 1) / BM;
  const int ntg = (d->So * d->Ng + BN - 1) / BN;
  dim3 grid(unsigned((int64_t(d->B) * tps + 7) / 8 * 8), unsigned(ntg));  // xcd_rowtile
  return launch_fwd<__bf16>(k_dconv_pf<BM, BN>, grid, lds, d, x, wp, bias, aux, res, out, s);
}

// the prefetching kernel's shapes: bf16, one group, contiguous reduction rows, K <= 8
bool pf_ok(const sel_dconv_desc* d, int dtype) {
  return dtype == SEL_BF16 && d->G == 1 && (d->S == 1 || d->Cs == d->Cg) && d->K <= PF_KMAX && tune(16) != 1;
}

// Kernel family a forward / adjoint launch of this shape takes (include/sel.h
// SEL_DPATH_*): the single decision both the launcher and sel_dconv_kernel use.
struct FwdPlan {
  int path, bm, bn;
};

FwdPlan plan_fwd(const sel_dconv_desc* d, int dtype) {
  if (tune(9) == 1) return {SEL_DPATH_VALU, 0, 0};
  if (!mfma_ok(d, dtype)) {
    if (short_ok(d)) return {shortx_kernel<float>(d) ? SEL_DPATH_SHORTX : SEL_DPATH_SHORT, 0, 0};
    // tune key 31 = 1: the generic VALU kernel instead of the narrow-output one
    if (tiny_ok(d, dtype)) return {SEL_DPATH_TINY, 0, 0};
    return {SEL_DPATH_VALU, 0, 0};
  }
  const int width = d->So * d->Ng;
  const int64_t rows = int64_t(d->B) * d->Tvo;
  const bool bf = dtype == SEL_BF16;
  if (bf) {
    // the MPD's >= 128-wide one-group layers and adjoints: warp-specialised
    // 256 x 128 tiles (conv.hip k_conv_ws_bf16; tune key 21: 1 = off)
    if (tune(21) != 1 && width % 128 == 0 && d->S * d->Cg >= 64 && rows * (width / 128) >= 65536) {
      const int m = sel::conv::dconv_ws_mode(d);
      if (m >= 0) return {m == 1 ? SEL_DPATH_WS_FLAT : SEL_DPATH_WS, 256, sel::conv::dconv_ws8_ok(d) ? 256 : 128};
    }
    if (width > 32 && pf_ok(d, dtype)) {
      // tune key 19: tile A/B (1: 256x64, 2: 128x128, 3: 256x128)
      if (tune(19) == 1) return {SEL_DPATH_PF, 256, 64};
      if (tune(19) == 3 && width % 128 == 0) return {SEL_DPATH_PF, 256, 128};
      // 128-column tiles halve the input re-staging per output (MPD 512 -> 1024 k5 s3: 8.4 -> 5.5 ms,
      // 1024 -> 1024 k5: 1.22 -> 0.80 ms at the probe's sizes, tools/dconv_probe.py, bit-identical)
      if (width % 128 == 0 && (tune(19) == 2 || (tune(19) == 0 && rows * (width / 128) >= 65536)))
        return {SEL_DPATH_PF, 128, 128};
      if (rows * (width / 64) < 65536) return {SEL_DPATH_PF, 64, 64};
      return {SEL_DPATH_PF, 128, 64};
    }
  }
  int bm, bn;
  // narrow groups: 32-wide tiles; short sequences / few rows: 64-row tiles
  if (width <= 32) {
    bn = 32;
    bm = rows * d->G < 131072 ? 128 : 256;
  } else if (rows * d->G * (width / 64) < 65536) {
    bm = 64, bn = 64;
  } else {
    // 256-row tiles: each staged tap group of weights serves twice the rows (the
    // MSD's 41-tap grouped layers: C5 50.5 -> 49.7 ms/step; tune key 28 bit 0 = 128 rows)
    bm = bf && !(tune(28) & 1) ? 256 : 128, bn = 64;
  }
  // register-prefetched pipeline (same stages, same bits; tune key 30 = 1: off);
  // its prefetch registers cover a span of BM + 63 rows.  Decided here alone:
  // launch_mfma is told.
  const bool gpf = bf && tune(30) != 1 && d->K - 1 <= KC * 8;
  return {gpf ? SEL_DPATH_GPF : SEL_DPATH_MFMA, bm, bn};
}

template <typename T>
int dispatch_fwd(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                 const void* res, void* out, hipStream_t s, int dtype) {
  const FwdPlan p = plan_fwd(d, dtype);
  switch (p.path) {
    case SEL_DPATH_VALU: return launch_valu<T>(d, x, wp, bias, aux, res, out, s);
    case SEL_DPATH_SHORT:
    case SEL_DPATH_SHORTX: return launch_short<T>(d, x, wp, bias, aux, res, out, s);
    case SEL_DPATH_TINY: return launch_tiny(d, x, wp, bias, aux, res, out, s);
    default: break;
  }
  if constexpr (sizeof(T) == 2) {
    if (p.path == SEL_DPATH_WS || p.path == SEL_DPATH_WS_FLAT)
      return sel::conv::dconv_ws_fwd(d, x, wp, bias, aux, res, out, s);
    if (p.path == SEL_DPATH_PF) {
      if (p.bm == 256 && p.bn == 64) return launch_pf<256, 64>(d, x, wp, bias, aux, res, out, s);
      if (p.bm == 256) return launch_pf<256, 128>(d, x, wp, bias, aux, res, out, s);
      if (p.bn == 128) return launch_pf<128, 128>(d, x, wp, bias, aux, res, out, s);
      if (p.bm == 64) return launch_pf<64, 64>(d, x, wp, bias, aux, res, out, s);
      return launch_pf<128, 64>(d, x, wp, bias, aux, res, out, s);
    }
  }
  const bool gpf = p.path == SEL_DPATH_GPF;  // k_dconv_gpf, else k_dconv_mfma
  if (p.bn == 32) {
    if (p.bm == 128) return launch_mfma<T, 128, 32>(d, x, wp, bias, aux, res, out, s, gpf);
    return launch_mfma<T, 256, 32>(d, x, wp, bias, aux, res, out, s, gpf);
  }
  if (p.bm == 64) return launch_mfma<T, 64, 64>(d, x, wp, bias, aux, res, out, s, gpf);
  if (p.bm == 256) return launch_mfma<T, 256, 64>(d, x, wp, bias, aux, res, out, s, gpf);
  return launch_mfma<T, 128, 64>(d, x, wp, bias, aux, res, out, s, gpf);
}

}  // namespace

extern "C" {

int sel_dconv_fwd(const sel_dconv_desc* d, int dtype, const void* x, const void* wpack, const float* bias,
                  const void* aux, const void* res, void* out, sel_stream_t stream) {
  if (int rc = check(d)) return rc;
  SEL_REQUIRE(x && wpack && out, SEL_ERR_ARG, "null pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SEL_BF16) return dispatch_fwd<__bf16>(d, x, wpack, bias, aux, res, out, s, dtype);
  if (dtype == SEL_F32) return dispatch_fwd<float>(d, x, wpack, bias, aux, res, out, s, dtype);
  set_error("sel_dconv_fwd: unsupported dtype %d", dtype);
  return SEL_ERR_UNSUPPORTED;
}

int sel_dconv_kernel(const sel_dconv_desc* d, int dtype, char* name, size_t cap) {
  if (!d || check(d) != SEL_OK || (dtype != SEL_BF16 && dtype != SEL_F32)) return -1;
  const FwdPlan p = plan_fwd(d, dtype);
  if (name && cap) {
    const char* t = dtype == SEL_BF16 ? "bf16" : "float";
    switch (p.path) {
      case SEL_DPATH_WS:
      case SEL_DPATH_WS_FLAT:
        if (p.bn == 256) snprintf(name, cap, "k_conv_ws8<%d, bf16, 256, 256>", d->K);
        else snprintf(name, cap, "k_conv_ws_bf16<%d>", d->K);
        break;
      case SEL_DPATH_PF: snprintf(name, cap, "k_dconv_pf<%d, %d>", p.bm, p.bn); break;
      case SEL_DPATH_GPF: snprintf(name, cap, "k_dconv_gpf<%d, %d>", p.bm, p.bn); break;
      case SEL_DPATH_MFMA: snprintf(name, cap, "k_dconv_mfma<%s, %d, %d>", t, p.bm, p.bn); break;
      case SEL_DPATH_SHORTX: snprintf(name, cap, "k_dconv_shortx<%s, %d, %d>", t, d->K, d->S * d->Cg); break;
      case SEL_DPATH_SHORT: snprintf(name, cap, "k_dconv_short<%s, %d>", t, d->K * d->S * d->Cg); break;
      case SEL_DPATH_TINY: snprintf(name, cap, "k_dconv_tiny<4>"); break;
      default: snprintf(name, cap, "k_dconv_valu<%s>", t); break;
    }
  }
  return p.path;
}

}  // extern "C"
