// Weight gradients of the conv primitive (conv.hip): gWp[n][k][c] = sum_m
// gout[m][n] * act(in[row(m, k)][c]) and the bias sums, as a split-M reduction
// (one partial per split in a workspace) followed by a deterministic split
// reduce.
//   fp32:  k_wgrad_f32 on sample-aligned tiles, k_conv_wgrad for other shapes
//          (v_mfma_f32_16x16x4_f32), k_wgrad_c1 for a single input channel
//   bf16:  k_wgrad3_bf16 (k_wgrad2_bf16 / k_wgrad_bf16 by tune key 1 or shape),
//          k_wgrad_c1
//   reduce: k_split_* per layer, k_wgrad_finish_many batched over layers.
// The plan (wgrad_mode, wgrad_plan) picks kernel and split count; wgrad_impl
// launches it.  The fused residual-unit backward kernels that write the same
// partials are in conv_ru.hip.
#include <algorithm>

#include "conv_tile.h"

namespace sel {
namespace conv {

constexpr int C1_TR = 256;    // rows per sample-aligned tile (weight gradient)

// Weight gradient of a single-input-channel layer: gWp[n][k] = sum_m g[m][n] *
// act(x[row(m, k)]) and the bias sums.  Thread = (8-wide n group, row lane);
// each block walks its contiguous range of sample-aligned 256-row tiles with the
// samples staged in LDS, then reduces its lanes (shuffles, LDS over waves) into
// one partial per block.
// 8 consecutive gout values of one row: one 16-B load (bf16) or two (fp32)
struct F8 {
  float4 lo, hi;
};
template <typename TI> struct G8;
template <> struct G8<__bf16> {
  using type = uint4;
  static __device__ __forceinline__ type load(const __bf16* p) { return *reinterpret_cast<const uint4*>(p); }
  static __device__ __forceinline__ void get(const type& v, float (&f)[8]) {
    const __bf16* h = reinterpret_cast<const __bf16*>(&v);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = float(h[e]);
  }
};
template <> struct G8<float> {
  using type = F8;
  static __device__ __forceinline__ type load(const float* p) {
    return F8{*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4)};
  }
  static __device__ __forceinline__ void get(const type& v, float (&f)[8]) {
    f[0] = v.lo.x, f[1] = v.lo.y, f[2] = v.lo.z, f[3] = v.lo.w;
    f[4] = v.hi.x, f[5] = v.hi.y, f[6] = v.hi.z, f[7] = v.hi.w;
  }
};

template <typename TI, int NG>  // 1, 2, 4 or 8 n-groups (N / 8)
__global__ __launch_bounds__(256) void k_wgrad_c1(Args a, const TI* __restrict__ gout,
                                                  const TI* __restrict__ in, int64_t tiles_per_split,
                                                  float* __restrict__ part, float* __restrict__ bpart) {
  __shared__ float xs[C1_TR + C1_HALO];
  __shared__ float red[4][C1_NMAX * (C1_KMAX + 1)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid % NG, rl = tid / NG, nrl = 256 / NG;
  const int tps = (a.T + C1_TR - 1) / C1_TR;
  const int64_t ntiles = (a.rows / a.T) * tps;
  const int64_t tb = int64_t(blockIdx.x) * tiles_per_split;
  const int64_t te = tb + tiles_per_split < ntiles ? tb + tiles_per_split : ntiles;
  float acc[8][C1_KMAX], bsum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bsum[e] = 0.f;
#pragma unroll
    for (int k = 0; k < C1_KMAX; ++k) acc[e][k] = 0.f;
  }
  // the next tile's samples are fetched into registers while this tile is
  // reduced; this tile's gout rows are requested together before the FMAs
  const int span = C1_TR + (a.K - 1) * a.dil;
  float pre[2];
  auto fetch = [&](int64_t tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * C1_TR;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = threadIdx.x + 256 * u;
      int ti = t0 - a.pad + r;
      const bool ok = r < span && ((ti >= 0 && ti < a.T) || a.pad_mode == SEL_PAD_REPLICATE);
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      const float v = ok ? to_f(in[b * a.T + ti]) : 0.f;
      pre[u] = ok && a.in_elu ? c1_act<TI>(v) : v;
    }
  };
  constexpr int MAXR = C1_TR * NG / 256;  // rows per thread and tile
  // this tile's gout rows (next tile's: requested before this tile's FMAs)
  using GV = typename G8<TI>::type;
  GV gq[MAXR];
  auto fetch_g = [&](int64_t tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * C1_TR;
    const int rows = a.T - t0 < C1_TR ? a.T - t0 : C1_TR;
#pragma unroll
    for (int j = 0; j < MAXR; ++j) {
      const int r = rl + j * nrl;
      if (j * nrl < C1_TR && r < rows)
        gq[j] = G8<TI>::load(gout + (b * a.T + t0 + r) * a.N + grp * 8);
    }
  };
  if (tb < te) {
    fetch(tb);
    fetch_g(tb);
  }
  for (int64_t tile = tb; tile < te; ++tile) {
    const int t0 = int(tile % tps) * C1_TR;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (threadIdx.x + 256 * u < span) xs[threadIdx.x + 256 * u] = pre[u];
    __syncthreads();
    if (tile + 1 < te) fetch(tile + 1);
    const int rows = a.T - t0 < C1_TR ? a.T - t0 : C1_TR;
    GV gc[MAXR];
#pragma unroll
    for (int j = 0; j < MAXR; ++j) gc[j] = gq[j];
    if (tile + 1 < te) fetch_g(tile + 1);
#pragma unroll
    for (int j = 0; j < MAXR; ++j) {
      const int r = rl + j * nrl;
      if (j * nrl >= C1_TR || r >= rows) break;
      float gv[8];
      G8<TI>::get(gc[j], gv);
      float xv[C1_KMAX];
#pragma unroll
      for (int k = 0; k < C1_KMAX; ++k) xv[k] = k < a.K ? xs[r + k * a.dil] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = gv[e];
        bsum[e] += g;
#pragma unroll
        for (int k = 0; k < C1_KMAX; ++k) acc[e][k] = fmaf(g, xv[k], acc[e][k]);
      }
    }
  }
  // lanes of one wave with the same n group differ in the bits >= log2(NG)
#pragma unroll
  for (int e = 0; e < 8; ++e) {
#pragma unroll
    for (int k = 0; k <= C1_KMAX; ++k) {
      float v = k < C1_KMAX ? acc[e][k] : bsum[e];
      for (int o = 32; o >= NG; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane < NG) red[wave][(grp * 8 + e) * (C1_KMAX + 1) + k] = v;
    }
  }
  __syncthreads();
  for (int i = tid; i < a.N * (C1_KMAX + 1); i += 256) {
    const int n = i / (C1_KMAX + 1), k = i % (C1_KMAX + 1);
    const float v = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    if (k < a.K) part[int64_t(blockIdx.x) * a.N * a.K + n * a.K + k] = v;
    else if (k == C1_KMAX && bpart) bpart[int64_t(blockIdx.x) * a.N + n] = v;
  }
}

// ---------------------------------------------------------------------------
// weight gradient: gWp[n][k][c] = sum_m gout[m][n] * act(in[row(m,k)][c])
// block = (n-tile BN, c-chunk CK, m-split); all K taps per block.
// ---------------------------------------------------------------------------
constexpr int WG_BM = 64;        // m rows per staged chunk
constexpr int WG_GP = 16;        // pitch padding for fp32 LDS reads
constexpr int WG_MAXT = 16;      // max 16x16 output tiles per wave

template <typename TI, int BN>
__global__ __launch_bounds__(256) void k_conv_wgrad(Args a, const TI* __restrict__ gout,
                                                    const TI* __restrict__ in, int64_t rows_per_split,
                                                    float* __restrict__ part, float* __restrict__ bpart) {
  constexpr int GPITCH = BN + WG_GP;  // fp32
  constexpr int XPITCH = CK + WG_GP;  // fp32
  extern __shared__ __align__(16) unsigned char smem[];
  const int halo = (a.K - 1) * a.dil;
  const int span = WG_BM + halo;
  float* gs = reinterpret_cast<float*>(smem);
  float* xs = gs + WG_BM * GPITCH;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * BN;
  const int c0 = blockIdx.y * CK;
  const int split = blockIdx.z;
  const int64_t mbeg = int64_t(split) * rows_per_split;
  const int64_t mend = std::min<int64_t>(a.rows, mbeg + rows_per_split);

  // output tiles: (k, nt, ct) with nt < BN/16, ct < 2; distributed round-robin over waves
  const int ntile = a.K * (BN / 16) * 2;
  floatx4 acc[WG_MAXT];
#pragma unroll
  for (int j = 0; j < WG_MAXT; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;  // bias partial for column (threadIdx.x) when c0 == 0

  for (int64_t mc = mbeg; mc < mend; mc += WG_BM) {
    __syncthreads();
    // stage gout[mc .. mc+64) x [n0, n0+BN) as fp32
    for (int idx = threadIdx.x; idx < WG_BM * BN; idx += blockDim.x) {
      const int r = idx / BN, cc = idx % BN;
      const int64_t m = mc + r;
      const int n = n0 + cc;
      float v = 0.f;
      if (m < mend && n < a.N) v = to_f(gout[m * a.N + n]);
      gs[r * GPITCH + cc] = v;
    }
    // stage input rows [mc - pad, mc + 64 + halo - pad) channels [c0, c0+32) fp32 (+ELU)
    const int64_t g0 = mc - a.pad;
    for (int idx = threadIdx.x; idx < span * CK; idx += blockDim.x) {
      const int r = idx / CK, cc = idx % CK;
      const int64_t g = g0 + r;
      const int c = c0 + cc;
      float v = 0.f;
      if (g >= 0 && g < a.rows && c < a.C) {
        v = to_f(in[g * a.C + c]);
        if (a.in_elu) v = elu(v);
      }
      xs[r * XPITCH + cc] = v;
    }
    __syncthreads();
    if (bpart && c0 == 0 && threadIdx.x < BN) {
      for (int r = 0; r < WG_BM; ++r) bsum += gs[r * GPITCH + threadIdx.x];
    }
    // per-lane row validity / xs row for each (k): rows handled by this lane: mm = 4*q + (lane>>4)
#pragma unroll
    for (int j = 0; j < WG_MAXT; ++j) {
      const int tid = wave + 4 * j;
      if (tid >= ntile) break;
      const int k = tid / ((BN / 16) * 2);
      const int rem = tid % ((BN / 16) * 2);
      const int nt = rem >> 1, ct = rem & 1;
      const float* gcol = gs + nt * 16 + (lane & 15);
      const float* xcol = xs + ct * 16 + (lane & 15);
#pragma unroll 4
      for (int q = 0; q < WG_BM / 4; ++q) {
        const int r = 4 * q + (lane >> 4);
        const int64_t m = mc + r;
        float av = gcol[r * GPITCH];
        float bv = 0.f;
        if (m < mend) {
          const int64_t g = in_row(a, m, k);
          if (g >= 0) bv = xcol[int(g - g0) * XPITCH];
        }
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
  }
  // write partial tiles: part[split][n][k][c]  (C/D: col=c (lane&15), row=n (4*(lane>>4)+e))
  float* pdst = part + int64_t(split) * a.N * a.K * a.C;
#pragma unroll
  for (int j = 0; j < WG_MAXT; ++j) {
    const int tid = wave + 4 * j;
    if (tid >= ntile) break;
    const int k = tid / ((BN / 16) * 2);
    const int rem = tid % ((BN / 16) * 2);
    const int nt = rem >> 1, ct = rem & 1;
    const int c = c0 + ct * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + nt * 16 + 4 * (lane >> 4) + e;
      if (n < a.N && c < a.C) pdst[(int64_t(n) * a.K + k) * a.C + c] = acc[j][e];
    }
  }
  if (bpart && c0 == 0 && threadIdx.x < BN && n0 + int(threadIdx.x) < a.N)
    bpart[int64_t(split) * a.N + n0 + threadIdx.x] = bsum;
}

// fp32 weight gradient on sample-aligned 64-row tiles (the reference-precision
// path; the generic k_conv_wgrad above remains for other shapes).  One
// workgroup owns 64 output channels (16 per wave) x 32 input channels x all K
// taps and a contiguous range of 64-row tiles that never cross a sample, so
// the causal halo is zero- or replicate-filled while staging and the MFMA loop
// has no per-row address arithmetic or masks.  The next tile's g and x rows
// are fetched (16-B loads) into registers while the current tile's MFMAs run.
// MFMA v_mfma_f32_16x16x4_f32: A = g^T (lane: n = l & 15, row 4q + l >> 4),
// B = ELU(x) rows shifted by the tap (col c = l & 15); the 4 rows of one
// k-step are 80 / 48 floats apart in LDS (distinct 16-bank groups).
constexpr int WF_BM = 64, WF_XR = 128;
// NB output x CB input channels per workgroup: (64, 32), or (32, 64) / (32, 32)
// for the 32-wide layers (a 64-wide block would leave two of its waves on
// absent output channels); waves = (NB / 16) along n x the rest along c, each
// 16 n x CT 16-wide c tiles x all taps.  Row pitches NB + 16 / CB + 16 floats
// put the 4 rows of one k-step in distinct 16-bank groups.
template <int KM, int NB, int CB>
__global__ __launch_bounds__(256) void k_wgrad_f32(Args a, const float* __restrict__ gout,
                                                   const float* __restrict__ in, int tps, int64_t n_tiles,
                                                   int tiles_per_split, float* __restrict__ part,
                                                   float* __restrict__ bpart) {
  constexpr int GP = NB + 16, XP = CB + 16;
  constexpr int WN = NB / 16, WC = 4 / WN, CT = CB / (16 * WC);
  constexpr int G4 = NB / 4, GRP = 256 / G4, GI = WF_BM / GRP;   // gout float4 per row, rows per pass, passes
  constexpr int X4 = CB / 4, XRP = 256 / X4, XI = WF_XR / XRP;   // input float4 per row, rows per pass, passes
  static_assert(WN * WC == 4 && CT >= 1, "wave layout");
  __shared__ __align__(16) float gs[WF_BM * GP];
  __shared__ __align__(16) float xs[WF_XR * XP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wc = wave / WN;
  const int n0 = blockIdx.x * NB, c0 = blockIdx.y * CB;
  const int split = blockIdx.z;
  const int64_t tb = int64_t(split) * tiles_per_split;
  const int64_t te = tb + tiles_per_split < n_tiles ? tb + tiles_per_split : n_tiles;
  const int span = WF_BM + (a.K - 1) * a.dil;
  const bool want_bias = bpart != nullptr && c0 == 0;

  floatx4 acc[KM][CT];
#pragma unroll
  for (int k = 0; k < KM; ++k)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[k][ct] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  // raw loads of clamped (valid) addresses and their predicates; the zero
  // select happens in put() (a load under a per-element condition is a branch
  // with a vmcnt(0) wait, and a select right behind a load waits for it)
  float4 gr[GI], xr[XI];
  bool gok[GI], xok[XI];
  auto fetch = [&](int64_t tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile - b * tps) * WF_BM;
#pragma unroll
    for (int i = 0; i < GI; ++i) {
      const int r = i * GRP + tid / G4, n = n0 + (tid % G4) * 4;
      const int t = t0 + r;
      const int tc = t < a.T ? t : a.T - 1, nc = n < a.N ? n : a.N - 4;
      gr[i] = *reinterpret_cast<const float4*>(gout + (b * a.T + tc) * a.N + nc);
      gok[i] = t < a.T && n < a.N;
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int r = i * XRP + tid / X4, c = c0 + (tid % X4) * 4;
      int ti = t0 - a.pad + r;
      bool ok = r < span && c < a.C;
      if (ti < 0 || ti >= a.T) {
        if (a.pad_mode == SEL_PAD_ZERO) ok = false;
        ti = ti < 0 ? 0 : a.T - 1;
      }
      xr[i] = *reinterpret_cast<const float4*>(in + (b * a.T + ti) * a.C + (c < a.C ? c : a.C - 4));
      xok[i] = ok;
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int i = 0; i < GI; ++i)
      *reinterpret_cast<float4*>(gs + (i * GRP + tid / G4) * GP + (tid % G4) * 4) = keep4(gok[i], gr[i]);
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      float4 v = keep4(xok[i], xr[i]);
      if (a.in_elu) v = make_float4(elu(v.x), elu(v.y), elu(v.z), elu(v.w));
      *reinterpret_cast<float4*>(xs + (i * XRP + tid / X4) * XP + (tid % X4) * 4) = v;
    }
  };

  if (tb < te) fetch(tb);
  const float* gcol = gs + wn * 16 + (lane & 15);
  const float* xcol = xs + wc * CT * 16 + (lane & 15);
  for (int64_t tile = tb; tile < te; ++tile) {
    __syncthreads();  // the previous tile's MFMAs are done with gs / xs
    put();
    __syncthreads();
    if (tile + 1 < te) fetch(tile + 1);
    if (want_bias && tid < NB)
      for (int r = 0; r < WF_BM; ++r) bsum += gs[r * GP + tid];
#pragma unroll 2
    for (int q = 0; q < WF_BM / 4; ++q) {
      const int r = 4 * q + (lane >> 4);
      const float av = gcol[r * GP];
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k >= a.K) break;
        const float* xrow = xcol + (r + k * a.dil) * XP;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[k][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xrow[16 * ct], acc[k][ct], 0, 0, 0);
      }
    }
  }
  // partials: part[split][n][k][c] (C/D: col = c (lane & 15), row = n (4 (lane >> 4) + e))
  float* pdst = part + int64_t(split) * a.N * a.K * a.C;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k >= a.K) break;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c = c0 + (wc * CT + ct) * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + wn * 16 + 4 * (lane >> 4) + e;
        if (n < a.N && c < a.C) pdst[(int64_t(n) * a.K + k) * a.C + c] = acc[k][ct][e];
      }
    }
  }
  if (want_bias && tid < NB && n0 + tid < a.N) bpart[int64_t(split) * a.N + n0 + tid] = bsum;
}

// bf16 weight gradient.  One workgroup owns (n-tile BN, c-tile 32, all K taps) and
// a contiguous range of 64-row m-tiles that never cross a sample boundary (so
// the causal halo can be zero/replicate-filled while staging and no per-element
// masks are needed).  Both MFMA operands reduce over m, i.e. over the ROW index
// of the row-major LDS tiles: they are read with ds_read_b64_tr_b16 (gfx950
// transposing LDS read, 4 rows x 16 columns per 16-lane group).  The MFMA k-index
// kk = 8g + e maps to tile row 4g + e (e < 4) / 16 + 4g + e - 4 (e >= 4) so that
// each 32-lane half reads 8 consecutive rows: with a row pitch of 8u dwords
// (u odd) those reads are bank-conflict free.
constexpr int WB_BM = 64;
constexpr int WB_BC = 32;
constexpr int WB_MAXJ = 16;

template <int BN>
__global__ __launch_bounds__(256) void k_wgrad_bf16(Args a, const __bf16* __restrict__ gout,
                                                    const __bf16* __restrict__ in, int tiles_per_sample,
                                                    int64_t n_tiles, int tiles_per_split,
                                                    float* __restrict__ part, float* __restrict__ bpart) {
  constexpr int NT = BN / 16;
  constexpr int WPN = 4 / NT;        // waves sharing one n-subtile
  constexpr int PG = BN + 16;        // elements; (PG/2) dwords = 8 x odd
  constexpr int PX = WB_BC + 16;     // 48 elements = 24 dwords
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* gs = reinterpret_cast<__bf16*>(smem);
  __bf16* xs = gs + WB_BM * PG;
  const int halo = (a.K - 1) * a.dil;
  const int span = WB_BM + halo;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = wave % NT, wsub = wave / NT;
  const int n0 = blockIdx.x * BN, c0 = blockIdx.y * WB_BC;
  const int64_t tb = int64_t(blockIdx.z) * tiles_per_split;
  const int64_t te = tb + tiles_per_split < n_tiles ? tb + tiles_per_split : n_tiles;
  const int npairs = a.K * (WB_BC / 16);
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const bool vecG = (a.N % 8) == 0, vecX = (a.C % 8) == 0;

  floatx4 acc[WB_MAXJ];
#pragma unroll
  for (int j = 0; j < WB_MAXJ; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  for (int64_t tile = tb; tile < te; ++tile) {
    const int64_t b = tile / tiles_per_sample;
    const int t0 = int(tile % tiles_per_sample) * WB_BM;
    const int64_t rb = b * a.T;
    __syncthreads();
    for (int idx = tid; idx < WB_BM * (BN / 8); idx += 256) {
      const int r = idx / (BN / 8), v = (idx % (BN / 8)) * 8;
      const int t = t0 + r, n = n0 + v;
      __bf16 vals[8];
      if (t < a.T && vecG && n + 8 <= a.N) {
        *reinterpret_cast<uint4*>(vals) = *reinterpret_cast<const uint4*>(gout + (rb + t) * a.N + n);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          vals[e] = (t < a.T && n + e < a.N) ? gout[(rb + t) * a.N + n + e] : __bf16(0.f);
      }
      *reinterpret_cast<uint4*>(gs + r * PG + v) = *reinterpret_cast<uint4*>(vals);
    }
    for (int idx = tid; idx < span * (WB_BC / 8); idx += 256) {
      const int r = idx / (WB_BC / 8), v = (idx % (WB_BC / 8)) * 8;
      int ti = t0 - a.pad + r;
      const int c = c0 + v;
      bool ok = ti >= 0 && ti < a.T;
      if (!ok && a.pad_mode == SEL_PAD_REPLICATE) {
        ti = ti < 0 ? 0 : a.T - 1;
        ok = true;
      }
      __bf16 vals[8];
      if (ok && vecX && c + 8 <= a.C) {
        *reinterpret_cast<uint4*>(vals) = *reinterpret_cast<const uint4*>(in + (rb + ti) * a.C + c);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) vals[e] = (ok && c + e < a.C) ? in[(rb + ti) * a.C + c + e] : __bf16(0.f);
      }
      if (a.in_elu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) vals[e] = __bf16(elu_fast(float(vals[e])));
      }
      *reinterpret_cast<uint4*>(xs + r * PX + v) = *reinterpret_cast<uint4*>(vals);
    }
    __syncthreads();
    if (bpart && c0 == 0 && tid < BN) {
      for (int r = 0; r < WB_BM; ++r) bsum += float(gs[r * PG + tid]);
    }
#pragma unroll
    for (int grp = 0; grp < WB_BM / 32; ++grp) {
      const bf16x8 A = tr_frag(gs + (grp * 32 + 4 * g + q) * PG + nt * 16 + 4 * p, PG);
#pragma unroll
      for (int j = 0; j < WB_MAXJ; ++j) {
        const int pr = wsub + WPN * j;
        if (pr >= npairs) break;
        const int k = pr >> 1, ct = pr & 1;
        const bf16x8 Bf = tr_frag(xs + (grp * 32 + 4 * g + q + k * a.dil) * PX + ct * 16 + 4 * p, PX);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, Bf, acc[j], 0, 0, 0);
      }
    }
  }
  float* pdst = part + int64_t(blockIdx.z) * a.N * a.K * a.C;
#pragma unroll
  for (int j = 0; j < WB_MAXJ; ++j) {
    const int pr = wsub + WPN * j;
    if (pr >= npairs) break;
    const int k = pr >> 1, ct = pr & 1;
    const int c = c0 + ct * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + nt * 16 + 4 * (lane >> 4) + e;
      if (n < a.N && c < a.C) pdst[(int64_t(n) * a.K + k) * a.C + c] = acc[j][e];
    }
  }
  if (bpart && c0 == 0 && tid < BN && n0 + tid < a.N) bpart[int64_t(blockIdx.z) * a.N + n0 + tid] = bsum;
}

// bf16 weight gradient, fast path (C % 32 == 0, N % 32 == 0, halo <= 64, K <= 8):
// block = (32 output channels n, 32 input channels c, m-split).  m-tiles are 128
// rows of one sample; each of the 4 waves owns 32 rows of the tile and
// accumulates ALL K taps as 32x32 tiles (v_mfma_f32_32x32x16_bf16), reading
// both operands with ds_read_b64_tr_b16 from 64-B LDS rows (rows 4h..4h+3 per
// 32-lane half: conflict free).  The next tile's rows are prefetched into
// registers during the MFMAs (branch-free clamped loads); the 4 waves' partial
// tiles are summed through LDS once per split.
constexpr int W2_BM = 128;
constexpr int W2_HALO = 64;

template <int TW>  // waves split taps into TW groups and rows into 4/TW groups
__global__ __launch_bounds__(256) void k_wgrad2_bf16(Args a, const __bf16* __restrict__ gout,
                                                     const __bf16* __restrict__ in, int tiles_per_sample,
                                                     int64_t n_tiles, int tiles_per_split,
                                                     float* __restrict__ part, float* __restrict__ bpart) {
  constexpr int GV = W2_BM * 32 / 8 / 256;                  // 2
  constexpr int XV = ((W2_BM + W2_HALO) * 4 + 255) / 256;   // 3
  constexpr int GS = W2_BM * 32, XS = (W2_BM + W2_HALO) * 32;  // elements per buffer
  constexpr int RG = 4 / TW;                                // row groups
  constexpr int RROWS = W2_BM / RG;                         // rows per wave per tile
  constexpr int KPW = TW == 1 ? 1 : 2;                      // taps per wave: K=1 | K<=4 (TW=2) | K<=8 (TW=4)
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const base = reinterpret_cast<__bf16*>(smem);  // [buf]{G[128][32], X[192][32]}

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tg = wave % TW, rg = wave / TW;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int64_t tb = int64_t(blockIdx.z) * tiles_per_split;
  const int64_t te = tb + tiles_per_split < n_tiles ? tb + tiles_per_split : n_tiles;
  const int halo = (a.K - 1) * a.dil;
  const int span = W2_BM + halo;

  uint4 gr[GV], xr[XV];
  auto load = [&](int64_t tile) {
    const int64_t b = tile / tiles_per_sample;
    const int t0 = int(tile % tiles_per_sample) * W2_BM;
    const int64_t rb = b * a.T;
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      const int t = t0 + (v >> 2);
      const bool ok = t < a.T;
      uint4 val = *reinterpret_cast<const uint4*>(gout + (rb + (ok ? t : 0)) * a.N + n0 + (v & 3) * 8);
      if (!ok) val = make_uint4(0, 0, 0, 0);
      gr[u] = val;
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      if (u * 64 >= span) {  // block-uniform: no halo rows to fetch (K = 1 / short halo)
        xr[u] = make_uint4(0, 0, 0, 0);
        continue;
      }
      const int v = tid + u * 256;
      const int r = v >> 2;
      int ti = t0 - a.pad + r;
      const bool inside = ti >= 0 && ti < a.T;
      const bool ok = r < span && (inside || a.pad_mode == SEL_PAD_REPLICATE);
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      uint4 val = *reinterpret_cast<const uint4*>(in + (rb + ti) * a.C + c0 + (v & 3) * 8);
      if (!ok) val = make_uint4(0, 0, 0, 0);
      xr[u] = val;
    }
  };
  auto store = [&](int buf) {
    __bf16* g = base + buf * (GS + XS);
    __bf16* x = g + GS;
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      *reinterpret_cast<uint4*>(g + (v >> 2) * 32 + (v & 3) * 8) = gr[u];
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      if ((v >> 2) >= W2_BM + W2_HALO) continue;
      uint4 val = xr[u];
      if (a.in_elu) {
        val = elu8(val);
      }
      *reinterpret_cast<uint4*>(x + (v >> 2) * 32 + (v & 3) * 8) = val;
    }
  };

  floatx16 acc[KPW];
#pragma unroll
  for (int j = 0; j < KPW; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  float bsum = 0.f;

  const int h = lane >> 5;
  const int col = ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
  const int q = (lane & 15) >> 2;

  if (tb < te) load(tb);
  int buf = 0;
  for (int64_t tile = tb; tile < te; ++tile, buf ^= 1) {
    store(buf);
    __syncthreads();
    if (tile + 1 < te) load(tile + 1);
    const __bf16* g = base + buf * (GS + XS);
    const __bf16* x = g + GS;
#pragma unroll
    for (int kh = 0; kh < RROWS / 16; ++kh) {
      const int R = rg * RROWS + kh * 16;
      const v4i16 a0 = tr_read(g + (R + 4 * h + q) * 32 + col);
      const v4i16 a1 = tr_read(g + (R + 8 + 4 * h + q) * 32 + col);
      const bf16x8 A = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
      if (bpart && tg == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum += float(A[e]);
      }
#pragma unroll
      for (int j = 0; j < KPW; ++j) {
        const int k = tg + j * TW;
        if (k >= a.K) break;
        const int Rx = R + k * a.dil;
        const v4i16 b0 = tr_read(x + (Rx + 4 * h + q) * 32 + col);
        const v4i16 b1 = tr_read(x + (Rx + 8 + 4 * h + q) * 32 + col);
        const bf16x8 Bf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, Bf, acc[j], 0, 0, 0);
      }
    }
  }

  // sum the RG row-group partials of every tap, write the split partial
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [wave][KPW][32*32]
#pragma unroll
  for (int j = 0; j < KPW; ++j) {
    if (tg + j * TW >= a.K) break;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      red[(wave * KPW + j) * 1024 + row * 32 + (lane & 31)] = acc[j][r];
    }
  }
  if (bpart) {
    bsum += __shfl_xor(bsum, 32, 64);
  }
  __syncthreads();
  float* pdst = part + int64_t(blockIdx.z) * a.N * a.K * a.C;
  for (int i = tid; i < a.K * 1024; i += 256) {
    const int k = i >> 10, e = i & 1023;
    const int t = k % TW, j = k / TW;
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < RG; ++r) v += red[((r * TW + t) * KPW + j) * 1024 + e];
    const int n = n0 + (e >> 5), c = c0 + (e & 31);
    pdst[(int64_t(n) * a.K + k) * a.C + c] = v;
  }
  if (bpart && c0 == 0) {
    __syncthreads();
    if (tg == 0 && lane < 32) red[rg * 32 + lane] = bsum;
    __syncthreads();
    if (tid < 32) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < RG; ++r) v += red[r * 32 + tid];
      bpart[int64_t(blockIdx.z) * a.N + n0 + tid] = v;
    }
  }
}

// rows of one k_wgrad3_bf16 X plane: the 128-row tile + this layer's halo,
// rounded up to 16 rows (at most W2_BM + W2_HALO)
__host__ __device__ constexpr int wgrad3_xrows(int K, int dil) { return W2_BM + (((K - 1) * dil + 15) & ~15); }

// bf16 weight gradient, general tr-read path (C % 32 == 0, N % 32 == 0,
// halo <= 64, K <= 8).  A block owns NB = 32*NT output channels x CB = 32*CT
// input channels x ALL K taps over a contiguous range of 128-row tiles, so a
// 64x64 layer streams gout and act(in) exactly once (the 32x32 kernel above
// re-read both per (n, c) block).  The TT = NT*CT*K 32x32 accumulator tiles are
// spread over the 4 waves (TPW each, contiguous so consecutive tiles share the
// gout fragment); with TT < 4 the waves split the tile rows instead (RG row
// groups) and meet in LDS.  Operands come from 64-B LDS rows through
// ds_read_b64_tr_b16 (conflict free); the next tile is prefetched into
// registers during the MFMAs.  Grid x = row split (fastest), so the blocks
// sharing a row range are 8-aligned apart... i.e. on the same XCD when the
// split count is a multiple of 8.
template <int NT, int CT, int MAXT, bool PIPE>
__global__ __launch_bounds__(256) void k_wgrad3_bf16(Args a, const __bf16* __restrict__ gout,
                                                     const __bf16* __restrict__ in, int tiles_per_sample,
                                                     int64_t n_tiles, int tiles_per_split,
                                                     float* __restrict__ part, float* __restrict__ bpart) {
  constexpr int NB = 32 * NT, CB = 32 * CT;
  constexpr int XROWS = W2_BM + W2_HALO;
  constexpr int GV = W2_BM * NB / 8 / 256;   // 2*NT
  constexpr int XV = XROWS * CB / 8 / 256;   // 3*CT
  constexpr int GS = NT * W2_BM * 32;
  constexpr int WPN = 4 / NT;                // waves per 32-wide n subtile
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const base = reinterpret_cast<__bf16*>(smem);  // [buf]{G[NT][128][32], X[CT][192][32]}

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t split = blockIdx.x;
  const int n0 = blockIdx.y * NB, c0 = blockIdx.z * CB;
  const int64_t tb = split * tiles_per_split;
  const int64_t te = tb + tiles_per_split < n_tiles ? tb + tiles_per_split : n_tiles;
  const int halo = (a.K - 1) * a.dil;
  const int span = W2_BM + halo;
  // X planes sized for this layer's halo (wgrad3_xrows; the launch sizes the LDS
  // the same way): a k1 / k3 layer's blocks need less LDS, more fit on a CU
  const int xrows = wgrad3_xrows(a.K, a.dil);
  const int XS = CT * xrows * 32;
  // wave -> (n subtile, (ct, k) pairs); too few pairs -> the waves split the rows
  const int P = CT * a.K;
  const int RG = P >= WPN ? 1 : WPN / P;     // P in {1, 2} when RG > 1
  const int WPP = WPN / RG;                  // waves sharing the pair list
  const int nt = wave / WPN, wsub = wave % WPN;
  const int rg = wsub / WPP, pw = wsub % WPP;
  const int RROWS = W2_BM / RG;
  const bool do_bias = bpart && blockIdx.z == 0;

  uint4 gr[GV], xr[XV];
  bool gok[GV], xok[XV];
  // branch-free buffer loads over one sample (ru_bload: rows past T / the span,
  // padded rows and a dead request read nothing): the compiler then counts the
  // request exactly, and the MFMA phase no longer waits on it with vmcnt(0)
  auto load = [&](int64_t tile, bool live) {
    const int64_t b = tile / tiles_per_sample;
    const int t0 = int(tile % tiles_per_sample) * W2_BM;
    const int64_t rb = b * a.T;
    const __amdgpu_buffer_rsrc_t rg = ru_rsrc(gout + rb * a.N, int64_t(a.T) * a.N);
    const __amdgpu_buffer_rsrc_t rx = ru_rsrc(in + rb * a.C, int64_t(a.T) * a.C);
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      const int t = t0 + v / (NB / 8);
      gok[u] = t < a.T;
      gr[u] = ru_bload(rg, live && gok[u] ? (t * a.N + n0 + (v % (NB / 8)) * 8) * 2 : RU_OOB);
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / (CB / 8);
      int ti = t0 - a.pad + r;
      const bool inside = ti >= 0 && ti < a.T;
      xok[u] = r < span && (inside || a.pad_mode == SEL_PAD_REPLICATE);
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      xr[u] = ru_bload(rx, live && xok[u] ? (ti * a.C + c0 + (v % (CB / 8)) * 8) * 2 : RU_OOB);
    }
  };
  // zero-fill happens here, after the wait (see the v4 forward kernel's store())
  auto store = [&](int buf) {
    __bf16* g = base + buf * (GS + XS);
    __bf16* x = g + GS;
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      const int r = v / (NB / 8), c8 = v % (NB / 8);
      *reinterpret_cast<uint4*>(g + (c8 >> 2) * (W2_BM * 32) + r * 32 + (c8 & 3) * 8) =
          gok[u] ? gr[u] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      if (u * 256 / (CB / 8) >= span) continue;
      const int v = tid + u * 256;
      const int r = v / (CB / 8), c8 = v % (CB / 8);
      if (r >= span) continue;  // the X planes end at xrows (no tap reads past span - 1)
      uint4 val = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
      if (a.in_elu) {
        val = elu8(val);
      }
      *reinterpret_cast<uint4*>(x + (c8 >> 2) * (xrows * 32) + r * 32 + (c8 & 3) * 8) = val;
    }
  };

  // pair j of this wave: p = pw + WPP*j -> (ct, k); slots past P compute into
  // accumulators that are never stored (branch-free MFMA stream)
  int xoff[MAXT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    int p = pw + WPP * j;
    p = p < P ? p : P - 1;
    xoff[j] = (p / a.K) * (xrows * 32) + (p % a.K) * a.dil * 32;
  }

  floatx16 acc[MAXT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  float bsum = 0.f;
  const int bcol = tid % NB, brow = tid / NB;

  const int h = lane >> 5;
  const int col = ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
  const int q = (lane & 15) >> 2;
  const int lrow = (4 * h + q) * 32 + col;

  if (tb < te) load(tb, true);
  int buf = 0;
  for (int64_t tile = tb; tile < te; ++tile, buf ^= 1) {
    store(buf);
    __syncthreads();
    load(tile + 1 < te ? tile + 1 : tile, tile + 1 < te);  // unconditional: exact counts
    const __bf16* g = base + buf * (GS + XS) + nt * (W2_BM * 32);
    const __bf16* x = base + buf * (GS + XS) + GS;
    if (do_bias) {
      // the column's rows in four independent chains (a single running sum
      // made every 2-byte LDS read wait for the previous one: the bias blocks
      // then trailed the others by ~3 k cycles per tile)
      constexpr int BSTEP = 256 / NB, BN_ = W2_BM / BSTEP;
      const __bf16* gb = base + buf * (GS + XS) + (bcol >> 5) * (W2_BM * 32) + (bcol & 31) + brow * 32;
      float b4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < BN_; ++i) b4[i & 3] += float(gb[i * BSTEP * 32]);
      bsum += (b4[0] + b4[1]) + (b4[2] + b4[3]);
    }
    // fragments of row step kh + 1 are read while step kh's MFMAs run (two
    // register sets, two steps per trip: RROWS / 16 is even)
    struct Frags {
      bf16x8 A, B[MAXT];
    };
    auto fetch = [&](int kh, Frags& f) {
      const int R = (rg * RROWS + kh * 16) * 32 + lrow;
      const v4i16 a0 = tr_read(g + R);
      const v4i16 a1 = tr_read(g + R + 8 * 32);
      f.A = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const v4i16 b0 = tr_read(x + xoff[j] + R);
        const v4i16 b1 = tr_read(x + xoff[j] + R + 8 * 32);
        f.B[j] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
      }
    };
    auto mma = [&](const Frags& f) {
#pragma unroll
      for (int j = 0; j < MAXT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.A, f.B[j], acc[j], 0, 0, 0);
    };
    const int nk = RROWS / 16;
    if constexpr (PIPE) {
      Frags f0, f1;
      fetch(0, f0);
      for (int kh = 0; kh < nk; kh += 2) {
        fetch(kh + 1, f1);
        mma(f0);
        if (kh + 2 < nk) fetch(kh + 2, f0);
        mma(f1);
      }
    } else {
      // four pairs per wave (the k7 layers) and the short layers (T <= 400):
      // measured 2-6% slower pipelined (the second register set costs
      // occupancy), so one set, one step at a time
      for (int kh = 0; kh < nk; ++kh) {
        Frags f;
        fetch(kh, f);
        mma(f);
      }
    }
  }

  float* pdst = part + split * int64_t(a.N) * a.K * a.C;
  if (RG == 1) {
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      const int p = pw + WPP * j;
      if (p >= P) break;
      const int ct = p / a.K, k = p % a.K;
      const int c = c0 + ct * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        pdst[(int64_t(n) * a.K + k) * a.C + c] = acc[j][r];
      }
    }
  } else {
    // RG > 1 only for P < WPN, i.e. MAXT slots hold at most one pair per wave
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [wave][32*32]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      red[wave * 1024 + row * 32 + (lane & 31)] = acc[0][r];
    }
    __syncthreads();
    for (int i = tid; i < NT * P * 1024; i += 256) {
      const int e = i & 1023, pi = (i >> 10) % P, ni = (i >> 10) / P;
      float v = 0.f;
      for (int r = 0; r < RG; ++r) v += red[(ni * WPN + r * WPP + pi) * 1024 + e];
      const int ct = pi / a.K, k = pi % a.K;
      const int n = n0 + ni * 32 + (e >> 5), c = c0 + ct * 32 + (e & 31);
      pdst[(int64_t(n) * a.K + k) * a.C + c] = v;
    }
  }
  if (do_bias) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    red[tid] = bsum;
    __syncthreads();
    if (tid < NB) {
      float v = 0.f;
      for (int r = 0; r < 256 / NB; ++r) v += red[r * NB + tid];
      bpart[split * a.N + n0 + tid] = v;
    }
  }
}

// Deterministic split reduction in two parallel passes:
//   pass 1: part2[g][i] = sum_{s in group g (32 splits)} part[s][i]   (grid: i-blocks x groups)
//   pass 2: out[j] = sum_g sum_{i % period == j} part2[g][i]
constexpr int SPLIT_GROUP = 32;

// sum of the partials p[0], p[n], ... p[(cnt - 1) n] of one split group (cnt <= 32)
template <int W>
__device__ __forceinline__ float split_tree(const float* __restrict__ p, int cnt, int64_t n) {
  // W loads in flight at once (slots past cnt hold exact zeros), then a fixed
  // pairwise tree: deterministic for a given cnt
  float v[W];
#pragma unroll
  for (int u = 0; u < W; ++u) v[u] = u < cnt ? p[int64_t(u) * n] : 0.f;
#pragma unroll
  for (int w = 1; w < W; w *= 2)
#pragma unroll
    for (int u = 0; u < W; u += 2 * w) v[u] += v[u + w];
  return v[0];
}
__device__ __forceinline__ float split_group_sum(const float* __restrict__ p, int cnt, int64_t n,
                                                 bool four_at_a_time = false) {
  // a full group: all 32 loads in flight at once (a serial chain of dependent
  // adds made the compiler issue them a few at a time: latency-bound)
  if (cnt == SPLIT_GROUP) return split_tree<SPLIT_GROUP>(p, cnt, n);
  // partial groups (round 6: the RU256 k7 layers' 16 splits, 29 MB each, went
  // four loads per round trip): the smallest power-of-two tree holding cnt;
  // tune key 68 = 1: the four-at-a-time loop
  if (!four_at_a_time) {
    if (cnt > 16) return split_tree<32>(p, cnt, n);
    if (cnt > 8) return split_tree<16>(p, cnt, n);
    if (cnt > 4) return split_tree<8>(p, cnt, n);
    return split_tree<4>(p, cnt, n);
  }
  float acc = 0.f;
  int u = 0;
  for (; u + 4 <= cnt; u += 4) {
    const float a0 = p[int64_t(u) * n], a1 = p[int64_t(u + 1) * n], a2 = p[int64_t(u + 2) * n],
                a3 = p[int64_t(u + 3) * n];
    acc += (a0 + a1) + (a2 + a3);
  }
  for (; u < cnt; ++u) acc += p[int64_t(u) * n];
  return acc;
}

__global__ __launch_bounds__(256) void k_split_sum1(const float* __restrict__ part, int nsplit, int64_t n,
                                                    float* __restrict__ part2) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int s0 = blockIdx.y * SPLIT_GROUP;
  const int s1 = s0 + SPLIT_GROUP < nsplit ? s0 + SPLIT_GROUP : nsplit;
  part2[int64_t(blockIdx.y) * n + i] = split_group_sum(part + int64_t(s0) * n + i, s1 - s0, n);
}

__global__ __launch_bounds__(256) void k_split_sum2(const float* __restrict__ part2, int ngroups, int64_t n,
                                                    int period, float* __restrict__ out) {
  const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (j >= period) return;
  float acc = 0.f;
  for (int g = 0; g < ngroups; ++g)
    for (int64_t i = j; i < n; i += period) acc += part2[int64_t(g) * n + i];
  out[j] = acc;
}

// Packed index of torch-layout weight element i (the gather map of k_unpack, conv_pack.hip).
__device__ __forceinline__ int64_t unpack_src(int kind, int64_t i, int cout, int cin, int K, int s) {
  if (kind == SEL_PACK_FWD) {
    const int k = int(i % K);
    const int ci = int((i / K) % cin);
    const int co = int(i / (int64_t(K) * cin));
    return (int64_t(co) * K + k) * cin + ci;
  }
  const int KK = 2 * s;
  const int k = int(i % KK);
  if (kind == SEL_PACK_FWD_STRIDED) {
    const int ci = int((i / KK) % cin);
    const int co = int(i / (int64_t(KK) * cin));
    int tap, ph;
    if (k <= s - 2) { tap = 0; ph = k + 1; }
    else if (k <= 2 * s - 2) { tap = 1; ph = k - s + 1; }
    else { tap = 2; ph = 0; }
    return (int64_t(co) * 3 + tap) * (int64_t(s) * cin) + ph * cin + ci;
  }
  const int co = int((i / KK) % cout);
  const int ci = int(i / (int64_t(KK) * cout));
  const int ph = k < s ? k : k - s;
  const int tap = k < s ? 1 : 0;
  return (int64_t(ph * cout + co) * 2 + tap) * cin + ci;
}

// Second reduction pass fused with the unpack: gw (torch layout) = sum over the
// split groups of the packed partials (one launch instead of two per layer).
__global__ __launch_bounds__(256) void k_split_sum2_unpack(const float* __restrict__ part2, int ngroups, int64_t n,
                                                           int64_t n_torch, int kind, int cout, int cin, int K,
                                                           int s, float* __restrict__ gw) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n_torch) return;
  const int64_t j = unpack_src(kind, i, cout, cin, K, s);
  const float* p = part2 + j;
  float acc = 0.f;
  int g = 0;
  for (; g + 4 <= ngroups; g += 4) {  // 4 loads in flight, fixed order
    const float a0 = p[int64_t(g) * n], a1 = p[int64_t(g + 1) * n], a2 = p[int64_t(g + 2) * n],
                a3 = p[int64_t(g + 3) * n];
    acc += (a0 + a1) + (a2 + a3);
  }
  for (; g < ngroups; ++g) acc += p[int64_t(g) * n];
  gw[i] = acc;
}

// One split group (nsplit <= 32): both reduction passes, the unpack and the bias
// fold in one launch, with the arithmetic of k_split_sum1 + k_split_sum2(_unpack)
// (the second pass adds one group sum to 0, exactly): threads [0, nt) write the
// weight gradient (torch layout when kind >= 0, else the packed one), threads
// [nt, nt + period) the bias.
__global__ __launch_bounds__(256) void k_split_finish1(const float* __restrict__ part, int nsplit, int64_t nw,
                                                       int64_t nt, int kind, int cout, int cin, int K, int s,
                                                       float* __restrict__ gw, const float* __restrict__ bpart,
                                                       int64_t nb, int period, float* __restrict__ gb) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < nt) {
    const int64_t j = kind >= 0 ? unpack_src(kind, i, cout, cin, K, s) : i;
    gw[i] = 0.f + split_group_sum(part + j, nsplit, nw);
  } else if (gb && i < nt + period) {
    const int64_t jb = i - nt;
    float acc = 0.f;
    for (int64_t q = jb; q < nb; q += period) acc += split_group_sum(bpart + q, nsplit, nb);
    gb[jb] = acc;
  }
}

// Batched split reduction (sel_wgrad_finish_many), with exactly the arithmetic
// of k_split_sum1 + k_split_sum2_unpack / k_split_sum2 (and of k_split_finish1,
// the one-group case of the same formula): group sums of 32 splits
// (split_group_sum), then the groups in order, four at a time.  A weight block
// owns 256 consecutive PACKED elements of one job (coalesced partial reads),
// one per thread: the thread adds its element's group sums in order and
// scatters to the torch layout.  A bias block owns one bias
// element: its threads compute the (group, column) sums, thread 0 adds them in
// order.  Block ranges per job come in the kernel argument.
constexpr int FM_MAXJ = 24;
constexpr int FM_MAXG = 32;  // split groups per job (nsplit <= 1024)
struct FinishJobs {
  sel_wgrad_job j[FM_MAXJ];
  int wblocks[FM_MAXJ];  // weight blocks of job j; its bias blocks follow
  int bstart[FM_MAXJ + 1];
  int njobs;
  int four;  // tune key 68 = 1: partial split groups four loads at a time (A/B)
};

// packed weight index -> torch-layout index (-1: a structural zero of the strided form)
__device__ __forceinline__ int64_t pack_dst(int kind, int64_t j, int cout, int cin, int K, int s) {
  if (kind < 0) return j;
  const int ci = int(j % cin);
  if (kind == SEL_PACK_FWD) {
    const int k = int((j / cin) % K);
    const int64_t co = j / (int64_t(cin) * K);
    return (co * cin + ci) * K + k;
  }
  if (kind == SEL_PACK_FWD_STRIDED) {
    const int ph = int((j / cin) % s);
    const int tap = int((j / (int64_t(s) * cin)) % 3);
    const int64_t co = j / (int64_t(3) * s * cin);
    const int k = tap == 0 ? (ph >= 1 ? ph - 1 : -1) : (tap == 1 ? ph + s - 1 : (ph == 0 ? 2 * s - 1 : -1));
    return k < 0 ? -1 : (co * cin + ci) * (2 * s) + k;
  }
  const int tap = int((j / cin) % 2);
  const int64_t r = j / (int64_t(2) * cin);
  const int ph = int(r / cout), co = int(r % cout);
  const int k = tap ? ph : ph + s;
  return (int64_t(ci) * cout + co) * (2 * s) + k;
}

__global__ __launch_bounds__(256) void k_wgrad_finish_many(FinishJobs fj) {
  __shared__ float gs[FM_MAXG][65];
  int jb = 0;
  while (jb + 1 < fj.njobs && int(blockIdx.x) >= fj.bstart[jb + 1]) ++jb;  // block-uniform
  const sel_wgrad_job& J = fj.j[jb];
  const int lb = int(blockIdx.x) - fj.bstart[jb];
  const int ng = (J.nsplit + SPLIT_GROUP - 1) / SPLIT_GROUP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto group = [&](const float* p, int g, int64_t n) {
    const int s0 = g * SPLIT_GROUP, cnt = J.nsplit - s0 < SPLIT_GROUP ? J.nsplit - s0 : SPLIT_GROUP;
    return split_group_sum(p + int64_t(s0) * n, cnt, n, fj.four != 0);
  };
  if (lb < fj.wblocks[jb]) {
    // one packed element per thread, its group sums in order (the reduction
    // needs no LDS: all 256 threads stream partials, where the 64-element
    // blocks left three of four waves idle for the common one-group jobs)
    (void)lane;
    (void)wave;
    const int64_t j = int64_t(lb) * 256 + tid;
    if (j < J.nw) {
      float acc = 0.f;
      int g = 0;
      for (; g + 4 <= ng; g += 4) {
        const float g0 = group(J.part + j, g, J.nw), g1 = group(J.part + j, g + 1, J.nw);
        const float g2 = group(J.part + j, g + 2, J.nw), g3 = group(J.part + j, g + 3, J.nw);
        acc += (g0 + g1) + (g2 + g3);
      }
      for (; g < ng; ++g) acc += group(J.part + j, g, J.nw);
      const int64_t i = pack_dst(J.kind, j, J.cout, J.cin, J.k, J.stride);
      if (i >= 0) J.gw[i] = acc;
    }
  } else {
    const int jb2 = lb - fj.wblocks[jb];  // bias element
    const int M = J.N / J.bias_period;     // columns folded into it
    const float* bp = J.part + int64_t(J.nsplit) * J.nw;
    float* const ts = &gs[0][0];           // [g][m]
    for (int t = tid; t < ng * M; t += 256) ts[t] = group(bp + jb2 + int64_t(t % M) * J.bias_period, t / M, J.N);
    __syncthreads();
    if (tid == 0) {
      float acc = 0.f;
      for (int t = 0; t < ng * M; ++t) acc += ts[t];
      J.gb[jb2] = acc;
    }
  }
}
}  // namespace conv
}  // namespace sel

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace sel;
using namespace sel::conv;

namespace {

constexpr int kWgBN = 64;

int wgrad_bn(int N) { return N <= 16 ? 16 : (N <= 32 ? 32 : 64); }

// Split plan shared by both dtypes: 64-row m-tiles that never cross a sample,
// enough splits for ~2 workgroups per CU, partial buffer capped at 64 MB.
struct WgPlan {
  int64_t tiles_per_sample, n_tiles;
  int nsplit, tiles_per_split, bn;
  int mode;  // 0 generic (k_wgrad_bf16 / fp32), 2 k_wgrad2_bf16 (32x32), 3 k_wgrad3_bf16
  int nt, ct, maxt;
};

bool wgrad_tr_ok(const sel_conv_desc* d) {
  // (one sample's gout / input rows must fit a 2^31-byte buffer resource: ru_rsrc)
  return d->C % 32 == 0 && d->N % 32 == 0 && (d->K - 1) * d->dil <= W2_HALO && d->K <= 8 &&
         ru_region_ok(int64_t(d->T) * std::max(d->C, d->N) * 2);
}

// tune key 1: 0 = k_wgrad3 where legal, 1 = generic, 2 = k_wgrad2 (32x32 blocks)
bool wgrad_c1_ok(const sel_conv_desc* d) {
  return d->C == 1 && d->N % 8 == 0 && d->N <= C1_NMAX && d->K <= C1_KMAX && (d->K - 1) * d->dil <= C1_HALO;
}

int wgrad_mode(const sel_conv_desc* d, int dtype) {
  // fp32: the single-channel kernel where it applies (tune key 54 = 1: generic)
  if (dtype != SEL_BF16) return wgrad_c1_ok(d) && tune(54) != 1 ? 4 : 0;
  const int t = tune(1);
  if (wgrad_c1_ok(d) && t != 1) return 4;
  if (t == 1 || !wgrad_tr_ok(d)) return 0;
  return t == 2 ? 2 : 3;
}

WgPlan wgrad_plan(const sel_conv_desc* d, int mode) {
  WgPlan p;
  p.mode = mode;
  p.nt = p.ct = p.maxt = 1;
  if (mode == 4) {  // k_wgrad_c1_bf16: contiguous ranges of sample-aligned 256-row tiles
    p.bn = d->N;
    p.tiles_per_sample = (d->T + C1_TR - 1) / C1_TR;
    p.n_tiles = (d->rows / d->T) * p.tiles_per_sample;
    p.tiles_per_split = int(std::max<int64_t>(1, (p.n_tiles + 511) / 512));
    p.nsplit = int((p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
    return p;
  }
  const bool tr = mode >= 2;
  const int bm = tr ? W2_BM : WB_BM;
  int bn, bc;
  if (mode == 3) {
    // widest block whose per-wave tile count stays <= 4 (8 accumulators = 1 wave/SIMD,
    // measured slower than re-reading a 32-wide operand from L2)
    auto tiles_per_wave = [&](int nt, int ct) {
      const int wpn = 4 / nt, pairs = ct * d->K;
      const int wpp = pairs >= wpn ? wpn : pairs;  // waves sharing one pair list (kernel: WPN / RG)
      return (pairs + wpp - 1) / wpp;
    };
    p.nt = d->N % 64 == 0 ? 2 : 1;
    p.ct = d->C % 64 == 0 ? 2 : 1;
    if (tiles_per_wave(p.nt, p.ct) > 4 && p.ct == 2) p.ct = 1;
    if (tiles_per_wave(p.nt, p.ct) > 4 && p.nt == 2) p.nt = 1;
    const int tpw = tiles_per_wave(p.nt, p.ct);
    // exact per-wave tile count (the strided k3 layers at 64 input channels per
    // block: 3 pairs per wave, which the 4-slot form ran with a never-stored slot)
    p.maxt = tpw <= 4 ? tpw : 8;
    bn = 32 * p.nt;
    bc = 32 * p.ct;
  } else {
    bn = tr ? 32 : wgrad_bn(d->N);
    bc = tr ? 32 : WB_BC;
  }
  p.bn = bn;
  p.tiles_per_sample = (d->T + bm - 1) / bm;
  p.n_tiles = (d->rows / d->T) * p.tiles_per_sample;
  const int64_t blocks = int64_t((d->N + bn - 1) / bn) * ((d->C + bc - 1) / bc);
  // tune key 10 > 0: workgroup-count target override (A/B sweeps)
  const int64_t target = tune(10) > 0 ? tune(10) : (mode == 3 ? 512 : 768);
  int64_t want = std::max<int64_t>(1, (target + blocks - 1) / blocks);
  if (mode == 3) want = (want + 7) / 8 * 8;  // splits on x: blocks of one row range share an XCD
  const int64_t per_split = (int64_t(d->N) * d->K * d->C + d->N) * 4;
  // split partials per layer capped at 32 MB (mode 3; tune key 62 > 0: another cap in MB)
  const int64_t cap_mb = mode == 3 ? (tune(62) > 0 ? tune(62) : 32) : 64;
  want = std::min<int64_t>(want, std::max<int64_t>(1, (cap_mb << 20) / per_split));
  want = std::min<int64_t>(want, std::max<int64_t>(1, p.n_tiles));
  p.tiles_per_split = int((p.n_tiles + want - 1) / want);
  if (p.tiles_per_split < 1) p.tiles_per_split = 1;
  p.nsplit = int((p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  if (p.nsplit < 1) p.nsplit = 1;
  return p;
}

template <int NT, int CT>
hipError_t launch_wgrad3(const WgPlan& p, const Args& a, const __bf16* gout, const __bf16* in, float* part,
                         float* bpart, hipStream_t s) {
  constexpr size_t lds_max = size_t(2) * (NT * W2_BM * 32 + CT * (W2_BM + W2_HALO) * 32) * sizeof(__bf16);
  const size_t lds = size_t(2) * (NT * W2_BM * 32 + CT * wgrad3_xrows(a.K, a.dil) * 32) * sizeof(__bf16);
  dim3 grid(unsigned(p.nsplit), unsigned(a.N / (32 * NT)), unsigned(a.C / (32 * CT)));
  // the two-set fragment pipeline (tune key 57 = 1) for the k2 / k3 layers
  // with >= 64 k rows: faster in tools/ab_wgrad.sh (256 -> 128 down conv
  // 69 -> 58 us, inputs re-read from the cache), not inside the profiled C3
  // step (<2, 1, 2> 55.8 -> 59 us, <2, 2, 3> 53.5 -> 52.3 us), so off
  const bool pipe = p.maxt <= 3 && a.rows >= 65536 && tune(57) == 1;
#define SEL_WG3(MT)                                                                                            \
  {                                                                                                            \
    auto kern = pipe ? k_wgrad3_bf16<NT, CT, MT, (MT <= 3)> : k_wgrad3_bf16<NT, CT, MT, false>;                \
    if (lds_max > 64 * 1024) {                                                                                 \
      hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_max)); \
      if (e != hipSuccess) return e;                                                                           \
    }                                                                                                          \
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, gout, in, int(p.tiles_per_sample), p.n_tiles,          \
                       p.tiles_per_split, part, bpart);                                                        \
  }
  if (p.maxt == 1) SEL_WG3(1)
  else if (p.maxt == 2) SEL_WG3(2)
  else if (p.maxt == 3) SEL_WG3(3)
  else if (p.maxt == 4) SEL_WG3(4)
  else SEL_WG3(8)
#undef SEL_WG3
  return hipGetLastError();
}

}  // namespace

namespace sel {
namespace conv {
struct UnpackSpec {
  int kind, cout, cin, k, stride;
};

int wgrad_impl(const sel_conv_desc* d, int dtype, const void* gout, const void* in, float* gwpack,
               const UnpackSpec* up, float* gbias, void* ws, size_t ws_bytes, sel_stream_t stream,
               int* partials_only = nullptr) {
  if (int rc = check_desc(d)) return rc;
  SEL_REQUIRE(d->K * 2 <= WB_MAXJ * 1 || dtype == SEL_F32, SEL_ERR_UNSUPPORTED, "wgrad: K=%d too large", d->K);
  SEL_REQUIRE(dtype == SEL_BF16 || d->K * (kWgBN / 16) * 2 <= 4 * WG_MAXT, SEL_ERR_UNSUPPORTED,
              "wgrad: K=%d too large", d->K);
  SEL_REQUIRE(ws_bytes >= sel_conv_wgrad_workspace(d), SEL_ERR_WORKSPACE, "workspace too small");
  const Args a = to_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const WgPlan p = wgrad_plan(d, wgrad_mode(d, dtype));
  float* part = static_cast<float*>(ws);
  float* bpart = gbias ? part + size_t(p.nsplit) * d->N * d->K * d->C : nullptr;
  if (d->rows > 0 && p.mode == 4) {
    if (dtype == SEL_F32) {
      auto kc1 = d->N == 8 ? k_wgrad_c1<float, 1> : d->N == 16 ? k_wgrad_c1<float, 2>
                 : d->N == 32 ? k_wgrad_c1<float, 4> : k_wgrad_c1<float, 8>;
      hipLaunchKernelGGL(kc1, dim3(unsigned(p.nsplit)), dim3(256), 0, s, a, static_cast<const float*>(gout),
                         static_cast<const float*>(in), int64_t(p.tiles_per_split), part, bpart);
    } else {
      auto kc1 = d->N == 8 ? k_wgrad_c1<__bf16, 1> : d->N == 16 ? k_wgrad_c1<__bf16, 2>
                 : d->N == 32 ? k_wgrad_c1<__bf16, 4> : k_wgrad_c1<__bf16, 8>;
      hipLaunchKernelGGL(kc1, dim3(unsigned(p.nsplit)), dim3(256), 0, s, a, static_cast<const __bf16*>(gout),
                         static_cast<const __bf16*>(in), int64_t(p.tiles_per_split), part, bpart);
    }
    SEL_LAUNCH_CHECK();
  } else if (d->rows > 0 && p.mode == 3) {
    const __bf16* g16 = static_cast<const __bf16*>(gout);
    const __bf16* x16 = static_cast<const __bf16*>(in);
    if (p.nt == 1 && p.ct == 1) SEL_HIP((launch_wgrad3<1, 1>(p, a, g16, x16, part, bpart, s)));
    else if (p.nt == 2 && p.ct == 1) SEL_HIP((launch_wgrad3<2, 1>(p, a, g16, x16, part, bpart, s)));
    else if (p.nt == 1 && p.ct == 2) SEL_HIP((launch_wgrad3<1, 2>(p, a, g16, x16, part, bpart, s)));
    else SEL_HIP((launch_wgrad3<2, 2>(p, a, g16, x16, part, bpart, s)));
  } else if (d->rows > 0 && p.mode == 2) {
    // staging double buffer (40 KB) also hosts the [wave][taps][32x32] fp32 reduction
    const size_t lds = std::max<size_t>(size_t(2) * (W2_BM * 32 + (W2_BM + W2_HALO) * 32) * sizeof(__bf16),
                                        size_t(4) * 8 * 1024 * sizeof(float) / 4 * 1);
    dim3 grid(unsigned(d->N / 32), unsigned(d->C / 32), unsigned(p.nsplit));
#define SEL_WG2_LAUNCH(KM)                                                                                    \
  hipLaunchKernelGGL(k_wgrad2_bf16<KM>, grid, dim3(256), lds, s, a, static_cast<const __bf16*>(gout),          \
                     static_cast<const __bf16*>(in), int(p.tiles_per_sample), p.n_tiles, p.tiles_per_split, part, \
                     bpart)
    if (d->K == 1) SEL_WG2_LAUNCH(1);
    else if (d->K <= 4) SEL_WG2_LAUNCH(2);
    else SEL_WG2_LAUNCH(4);
#undef SEL_WG2_LAUNCH
    SEL_LAUNCH_CHECK();
  } else if (d->rows > 0 && dtype == SEL_BF16) {
    const int span = WB_BM + (d->K - 1) * d->dil;
    const size_t lds = (size_t(WB_BM) * (p.bn + 16) + size_t(span) * (WB_BC + 16)) * sizeof(__bf16);
    SEL_REQUIRE(lds <= 160 * 1024, SEL_ERR_UNSUPPORTED, "wgrad tile needs %zu B of LDS", lds);
    dim3 grid(unsigned((d->N + p.bn - 1) / p.bn), unsigned((d->C + WB_BC - 1) / WB_BC), unsigned(p.nsplit));
#define SEL_WG_LAUNCH(BNV)                                                                                     \
  {                                                                                                            \
    auto kern = k_wgrad_bf16<BNV>;                                                                             \
    if (lds > 64 * 1024)                                                                                       \
      SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));   \
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, static_cast<const __bf16*>(gout),                     \
                       static_cast<const __bf16*>(in), int(p.tiles_per_sample), p.n_tiles, p.tiles_per_split,  \
                       part, bpart);                                                                           \
  }
    if (p.bn == 16) SEL_WG_LAUNCH(16)
    else if (p.bn == 32) SEL_WG_LAUNCH(32)
    else SEL_WG_LAUNCH(64)
#undef SEL_WG_LAUNCH
    SEL_LAUNCH_CHECK();
  } else if (d->rows > 0 && dtype == SEL_F32 && d->C % 4 == 0 && d->N % 4 == 0 && d->K <= 8 &&
             (d->K - 1) * d->dil <= WF_XR - WF_BM && d->pad <= (d->K - 1) * d->dil && tune(54) != 1) {
    // fp32 on sample-aligned tiles (tune key 54 = 1: the generic kernel below);
    // every split of the plan owns at least one tile
    // block shape: 64 x 32 channels, or 32 x 64 / 32 x 32 for the 32-wide layers
    const int nb = d->N <= 32 ? 32 : 64, cb = nb == 64 ? 32 : (d->C % 64 == 0 ? 64 : 32);
    dim3 grid(unsigned((d->N + nb - 1) / nb), unsigned((d->C + cb - 1) / cb), unsigned(p.nsplit));
#define SEL_WGF(NB, CB)                                                                                       \
  {                                                                                                           \
    auto kern = d->K == 1 ? k_wgrad_f32<1, NB, CB> : d->K <= 3 ? k_wgrad_f32<3, NB, CB> : k_wgrad_f32<8, NB, CB>; \
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, a, static_cast<const float*>(gout),                       \
                       static_cast<const float*>(in), int(p.tiles_per_sample), p.n_tiles, p.tiles_per_split, \
                       part, bpart);                                                                          \
  }
    if (nb == 64) SEL_WGF(64, 32)
    else if (cb == 64) SEL_WGF(32, 64)
    else SEL_WGF(32, 32)
#undef SEL_WGF
    SEL_LAUNCH_CHECK();
  } else if (d->rows > 0 && dtype == SEL_F32) {
    // fp32 parity path: flat row ranges, same number of splits as the plan
    const int64_t rps = ((d->rows + p.nsplit - 1) / p.nsplit + WG_BM - 1) / WG_BM * WG_BM;
    const int nsplit = int((d->rows + rps - 1) / rps);
    SEL_REQUIRE(nsplit <= p.nsplit, SEL_ERR_STATE, "internal split plan mismatch");
    const int span = WG_BM + (d->K - 1) * d->dil;
    const size_t lds = (size_t(WG_BM) * (kWgBN + WG_GP) + size_t(span) * (CK + WG_GP)) * sizeof(float);
    SEL_REQUIRE(lds <= 160 * 1024, SEL_ERR_UNSUPPORTED, "wgrad tile needs %zu B of LDS", lds);
    // unused tail splits must contribute zeros
    if (nsplit < p.nsplit)
      SEL_HIP(hipMemsetAsync(part + size_t(nsplit) * d->N * d->K * d->C, 0,
                             size_t(p.nsplit - nsplit) * d->N * d->K * d->C * sizeof(float), s));
    if (bpart && nsplit < p.nsplit)
      SEL_HIP(hipMemsetAsync(bpart + size_t(nsplit) * d->N, 0, size_t(p.nsplit - nsplit) * d->N * sizeof(float), s));
    dim3 grid(unsigned((d->N + kWgBN - 1) / kWgBN), unsigned((d->C + CK - 1) / CK), unsigned(nsplit));
    auto kern = k_conv_wgrad<float, kWgBN>;
    if (lds > 64 * 1024)
      SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, static_cast<const float*>(gout),
                       static_cast<const float*>(in), rps, part, bpart);
    SEL_LAUNCH_CHECK();
  } else if (d->rows > 0) {
    set_error("bad dtype %d", dtype);
    return SEL_ERR_ARG;
  }
  if (partials_only) {  // sel_conv_wgrad_partials: the reduction is batched later
    *partials_only = p.nsplit;
    return SEL_OK;
  }
  // two-pass split reduction; the second-level partials live after the first-level ones
  const int64_t nw = int64_t(d->N) * d->K * d->C;
  const int ng = (p.nsplit + SPLIT_GROUP - 1) / SPLIT_GROUP;
  if (ng == 1 && tune(20) != 1) {  // one launch for both passes, the unpack and the bias (tune key 20: 1 = off)
    const int64_t nt = up ? (up->kind == SEL_PACK_CONVT ? int64_t(up->cin) * up->cout * 2 * up->stride
                             : int64_t(up->cout) * up->cin * (up->kind == SEL_PACK_FWD ? up->k : 2 * up->stride))
                          : nw;
    const int64_t nthreads = nt + (gbias ? d->bias_period : 0);
    hipLaunchKernelGGL(k_split_finish1, dim3(unsigned((nthreads + 255) / 256)), dim3(256), 0, s, part, p.nsplit, nw, nt,
                       up ? up->kind : -1, up ? up->cout : 0, up ? up->cin : 0, up ? up->k : 0, up ? up->stride : 0,
                       gwpack, bpart, int64_t(d->N), gbias ? d->bias_period : 0, gbias);
    SEL_LAUNCH_CHECK();
    return SEL_OK;
  }
  float* part2 = part + size_t(p.nsplit) * (size_t(d->N) * d->K * d->C + d->N);
  hipLaunchKernelGGL(k_split_sum1, dim3(unsigned((nw + 255) / 256), unsigned(ng)), dim3(256), 0, s, part, p.nsplit,
                     nw, part2);
  SEL_LAUNCH_CHECK();
  if (up) {
    const int64_t nt = up->kind == SEL_PACK_CONVT ? int64_t(up->cin) * up->cout * 2 * up->stride
                       : int64_t(up->cout) * up->cin * (up->kind == SEL_PACK_FWD ? up->k : 2 * up->stride);
    hipLaunchKernelGGL(k_split_sum2_unpack, dim3(unsigned((nt + 255) / 256)), dim3(256), 0, s, part2, ng, nw, nt,
                       up->kind, up->cout, up->cin, up->k, up->stride, gwpack);
  } else {
    hipLaunchKernelGGL(k_split_sum2, dim3(unsigned((nw + 255) / 256)), dim3(256), 0, s, part2, ng, nw, int(nw),
                       gwpack);
  }
  SEL_LAUNCH_CHECK();
  if (gbias) {
    float* bpart2 = part2 + size_t(ng) * nw;
    hipLaunchKernelGGL(k_split_sum1, dim3(unsigned((d->N + 255) / 256), unsigned(ng)), dim3(256), 0, s, bpart,
                       p.nsplit, int64_t(d->N), bpart2);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_split_sum2, dim3(unsigned((d->bias_period + 255) / 256)), dim3(256), 0, s, bpart2, ng,
                       int64_t(d->N), d->bias_period, gbias);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}
}  // namespace conv
}  // namespace sel

extern "C" {

size_t sel_conv_wgrad_workspace(const sel_conv_desc* d) {
  // (an invalid descriptor sizes nothing: sel_conv_wgrad* rejects it itself)
  if (!d || d->rows <= 0 || check_desc(d) != SEL_OK) return 16;
  int ns = wgrad_plan(d, 0).nsplit;
  if (wgrad_tr_ok(d)) ns = std::max(ns, std::max(wgrad_plan(d, 2).nsplit, wgrad_plan(d, 3).nsplit));
  if (wgrad_c1_ok(d)) ns = std::max(ns, wgrad_plan(d, 4).nsplit);
  const int ng = (ns + SPLIT_GROUP - 1) / SPLIT_GROUP;
  return size_t(ns + ng) * (size_t(d->N) * d->K * d->C + d->N) * sizeof(float);
}

int sel_conv_wgrad(const sel_conv_desc* d, int dtype, const void* gout, const void* in, float* gwpack,
                   float* gbias, void* ws, size_t ws_bytes, sel_stream_t stream) {
  return sel::conv::wgrad_impl(d, dtype, gout, in, gwpack, nullptr, gbias, ws, ws_bytes, stream);
}

int sel_conv_wgrad_unpacked(const sel_conv_desc* d, int dtype, const void* gout, const void* in, int kind, int cout,
                            int cin, int k, int stride, float* gw, float* gbias, void* ws, size_t ws_bytes,
                            sel_stream_t stream) {
  SEL_REQUIRE(kind >= SEL_PACK_FWD && kind <= SEL_PACK_CONVT, SEL_ERR_ARG, "bad pack kind");
  const int64_t packed = kind == SEL_PACK_FWD ? int64_t(cout) * k * cin
                         : kind == SEL_PACK_FWD_STRIDED ? int64_t(cout) * 3 * stride * cin
                                                        : int64_t(stride) * cout * 2 * cin;
  SEL_REQUIRE(d && packed == int64_t(d->N) * d->K * d->C, SEL_ERR_ARG, "weight shape does not match the descriptor");
  const sel::conv::UnpackSpec up{kind, cout, cin, k, stride};
  return sel::conv::wgrad_impl(d, dtype, gout, in, gw, &up, gbias, ws, ws_bytes, stream);
}

int sel_conv_wgrad_partials(const sel_conv_desc* d, int dtype, const void* gout, const void* in, int want_bias,
                            void* ws, size_t ws_bytes, int* nsplit, sel_stream_t stream) {
  SEL_REQUIRE(nsplit, SEL_ERR_ARG, "null nsplit");
  int ns = 0;
  // a non-null bias pointer only selects the bias partials (it is never written here)
  float dummy = 0.f;
  const int rc = sel::conv::wgrad_impl(d, dtype, gout, in, nullptr, nullptr, want_bias ? &dummy : nullptr, ws,
                                       ws_bytes, stream, &ns);
  *nsplit = ns;
  return rc;
}

int sel_wgrad_finish_many(const sel_wgrad_job* jobs, int njobs, sel_stream_t stream) {
  using namespace sel::conv;
  SEL_REQUIRE(njobs >= 0 && (njobs == 0 || jobs), SEL_ERR_ARG, "bad job list");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += FM_MAXJ) {
    FinishJobs fj{};
    fj.njobs = std::min(FM_MAXJ, njobs - j0);
    fj.four = tune(68) == 1;
    int64_t blocks = 0;
    for (int j = 0; j < fj.njobs; ++j) {
      const sel_wgrad_job& J = jobs[j0 + j];
      SEL_REQUIRE(J.part && J.gw && J.nsplit > 0 && J.nsplit <= FM_MAXG * SPLIT_GROUP && J.nw > 0 && J.N > 0 &&
                      (J.gb == nullptr || (J.bias_period > 0 && J.N % J.bias_period == 0 &&
                                           (J.N / J.bias_period) * ((J.nsplit + SPLIT_GROUP - 1) / SPLIT_GROUP) <=
                                               FM_MAXG * 65)),
                  SEL_ERR_ARG, "bad wgrad job %d", j0 + j);
      fj.j[j] = J;
      fj.wblocks[j] = int((J.nw + 255) / 256);
      fj.bstart[j] = int(blocks);
      blocks += fj.wblocks[j] + (J.gb ? J.bias_period : 0);
    }
    fj.bstart[fj.njobs] = int(blocks);
    SEL_REQUIRE(blocks < (int64_t(1) << 31), SEL_ERR_ARG, "wgrad jobs too large");
    if (blocks > 0) {
      hipLaunchKernelGGL(k_wgrad_finish_many, dim3(unsigned(blocks)), dim3(256), 0, s, fj);
      SEL_LAUNCH_CHECK();
    }
  }
  return SEL_OK;
}

}  // extern "C"
