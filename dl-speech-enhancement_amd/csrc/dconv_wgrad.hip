// Weight gradients of the discriminator conv primitive (dconv.hip: the
// descriptor, the phase view and the forward / adjoint kernels).
//
//   Weight gradient: gW = sum_rows gout^T x as split-row partials (MFMA with
//     transposing LDS reads for bf16, VALU for fp32 / thin layers), then one
//     deterministic reduction fused with the unpack to the torch layout and the
//     weight-norm backward (torch.nn.utils.weight_norm, used by the MPD).
#include <algorithm>

#include "conv_tile.h"  // tr_read / tr_frag: the library's transposing LDS reads
#include "dconv_common.h"

namespace sel {
namespace dconv {

typedef float floatx4 __attribute__((ext_vector_type(4)));
using conv::tr_frag;
using conv::tr_read;
using conv::v4i16;

// ---------------------------------------------------------------------------
// Weight gradient partials.  gW[g][o][i][r][c] = sum over rows (b, j < Tvalid)
// of gout[b, j, col(g, o)] * x[b, j + q0 + i, r*Cs + g*Cg + c]; bias partials
// gb[col] = sum gout.  part[split][...] (fp32), reduced by k_dwgrad_finish.
// ---------------------------------------------------------------------------
// VALU: thread per weight element, rows of its split.  A split can be every
// row of the layer (wg_plan: one split when the layer has >= 2^20 weights), so
// the fp32 kernel sums its rows with compensation (Kahan): a plain running fp32
// sum of 16400 full-mantissa terms was 2e-6 off norm-wise, 20 x a pairwise
// sum's error (tests/test_gpu_dconv_edges.py).  bf16 products carry 16
// mantissa bits and lose an order of magnitude less: plain sum there.
template <typename T>
__device__ __forceinline__ void dwgrad_add(float& acc, float& comp, float g, float xv) {
  if constexpr (sizeof(T) == 4) {
    const float y = fmaf(g, xv, -comp);
    const float t = acc + y;
    comp = (t - acc) - y;
    acc = t;
  } else {
    acc += g * xv;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_dwgrad_valu(D d, const T* __restrict__ gout, const T* __restrict__ x,
                                                     int rows_per_split, float* __restrict__ part,
                                                     float* __restrict__ bpart) {
  const int no_per_g = d.So * d.Ng;
  const int nred = d.S * d.Cg;
  const int64_t nw = int64_t(d.G) * no_per_g * d.K * nred;
  const int64_t nb = bpart ? int64_t(d.G) * no_per_g : 0;
  const int64_t total_rows = int64_t(d.B) * d.Tvalid;
  const int64_t r0 = int64_t(blockIdx.y) * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < total_rows ? r0 + rows_per_split : total_rows;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < nw + nb; idx += int64_t(gridDim.x) * 256) {
    float acc = 0.f, comp = 0.f;
    if (idx < nw) {
      const int rc = int(idx % nred);
      const int i = int((idx / nred) % d.K);
      const int64_t go = idx / (int64_t(nred) * d.K);
      const int g = int(go / no_per_g), o = int(go - int64_t(g) * no_per_g);
      const int rph = rc / d.Cg, c = rc - rph * d.Cg;
      const int64_t oc = out_col(d, g, o), ic = in_col(d, g, rph, c);
      int b = int(r0 / d.Tvalid), j = int(r0 - int64_t(b) * d.Tvalid);  // one division, then a row walk
      for (int64_t rr = r0; rr < r1; ++rr) {
        const int t = j + d.q0 + i;
        if (t >= 0 && t < d.Tv)
          dwgrad_add<T>(acc, comp, to_f(gout[(int64_t(b) * d.Tvo + j) * d.ldo + oc]),
                        to_f(x[(int64_t(b) * d.Tvs + t) * d.ldx + ic]));
        if (++j == d.Tvalid) j = 0, ++b;
      }
      part[int64_t(blockIdx.y) * nw + idx] = acc;
    } else {
      const int64_t go = idx - nw;
      const int g = int(go / no_per_g), o = int(go - int64_t(g) * no_per_g);
      const int64_t oc = out_col(d, g, o);
      int b = int(r0 / d.Tvalid), j = int(r0 - int64_t(b) * d.Tvalid);
      for (int64_t rr = r0; rr < r1; ++rr) {
        dwgrad_add<T>(acc, comp, to_f(gout[(int64_t(b) * d.Tvo + j) * d.ldo + oc]), 1.f);
        if (++j == d.Tvalid) j = 0, ++b;
      }
      bpart[int64_t(blockIdx.y) * nb + go] = acc;
    }
  }
}

// bf16 MFMA weight gradient (Cg % 8 == 0, group output width a multiple of 16).
// Block = (16*NT local outputs o, 32 reduction channels (r, c), tap group of
// <= WG_TAPS taps, split of 64-row tiles).  Both operands reduce over ROWS of the
// row-major LDS tiles and are read with ds_read_b64_tr_b16 (gfx950 transposing
// LDS read), v_mfma_f32_16x16x32_bf16.
constexpr int WG_BM = 64;
constexpr int WG_TAPS = 8;

template <int NT>
__global__ __launch_bounds__(256) void k_dwgrad_mfma(D d, const __bf16* __restrict__ gout,
                                                     const __bf16* __restrict__ x, int tiles_per_seq,
                                                     int tiles_per_split, int ntg, float* __restrict__ part) {
  constexpr int BN = 16 * NT;
  constexpr int PG = BN + 16;  // (PG/2) dwords = 8 x odd: conflict-free transposing reads
  constexpr int PX = 32 + 16;
  constexpr int WPN = 4 / NT;  // waves per 16-wide output sub-tile
  constexpr int MAXJ = (WG_TAPS * 2 + WPN - 1) / WPN;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const gs = reinterpret_cast<__bf16*>(smem);
  __bf16* const xs = gs + WG_BM * PG;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = wave % NT, wsub = wave / NT;
  const int no_per_g = d.So * d.Ng;
  const int ntile_g = (no_per_g + BN - 1) / BN;
  const int g = blockIdx.x / ntile_g;
  const int o0 = (blockIdx.x % ntile_g) * BN;
  const int nred = d.S * d.Cg;
  const int cc = blockIdx.y * 32;
  const int tgi = blockIdx.z % ntg, split = blockIdx.z / ntg;
  const int k0 = tgi * WG_TAPS;
  const int kn = d.K - k0 < WG_TAPS ? d.K - k0 : WG_TAPS;
  const int span = WG_BM + kn - 1;
  const int64_t ntiles = int64_t(d.B) * tiles_per_seq;
  const int64_t tb = int64_t(split) * tiles_per_split;
  const int64_t te = tb + tiles_per_split < ntiles ? tb + tiles_per_split : ntiles;
  const int npairs = kn * 2;
  const int gq_ = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;

  floatx4 acc[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // forward layers (So == 1): the 8 outputs of a vector are contiguous columns,
  // and the next tile's gout / x vectors are fetched into registers while this
  // tile's MFMAs run (same MFMAs in the same order as the synchronous loop below)
  const bool vec = d.So == 1 && (d.ldo & 7) == 0 && (d.Ng & 7) == 0;
  if (vec) {
    constexpr int GQ = (WG_BM * (BN / 8) + 255) / 256;
    constexpr int XQ = ((WG_BM + WG_TAPS - 1) * 4 + 255) / 256;
    uint4 gq[GQ], xq[XQ];
    bool gok[GQ], xok[XQ];
    auto load = [&](int64_t tile) {
      const int b = int(tile / tiles_per_seq);
      const int j0 = int(tile % tiles_per_seq) * WG_BM;
#pragma unroll
      for (int u = 0; u < GQ; ++u) {
        const int idx = tid + u * 256;
        const int rr = idx / (BN / 8), v = (idx % (BN / 8)) * 8;
        const int j = j0 + rr;
        gok[u] = idx < WG_BM * (BN / 8) && j < d.Tvalid && o0 + v < no_per_g;
        gq[u] = *reinterpret_cast<const uint4*>(gout + (int64_t(b) * d.Tvo + (gok[u] ? j : 0)) * d.ldo +
                                                out_col(d, g, gok[u] ? o0 + v : 0));
      }
#pragma unroll
      for (int u = 0; u < XQ; ++u) {
        const int idx = tid + u * 256;
        const int rr = idx >> 2, v = (idx & 3) * 8;
        const int t = j0 + d.q0 + k0 + rr;
        const int ch = cc + v;
        xok[u] = rr < span && t >= 0 && t < d.Tv && ch < nred;
        const int rph = (xok[u] ? ch : 0) / d.Cg, c = (xok[u] ? ch : 0) - rph * d.Cg;
        if ((u * 256) / 4 < span)
          xq[u] = *reinterpret_cast<const uint4*>(x + (int64_t(b) * d.Tvs + (xok[u] ? t : 0)) * d.ldx +
                                                  in_col(d, g, rph, c));
      }
    };
    if (tb < te) load(tb);
    for (int64_t tile = tb; tile < te; ++tile) {
      __syncthreads();
#pragma unroll
      for (int u = 0; u < GQ; ++u) {
        const int idx = tid + u * 256;
        if (idx >= WG_BM * (BN / 8)) continue;
        const int rr = idx / (BN / 8), v = (idx % (BN / 8)) * 8;
        *reinterpret_cast<uint4*>(gs + rr * PG + v) = gok[u] ? gq[u] : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < XQ; ++u) {
        const int idx = tid + u * 256;
        const int rr = idx >> 2, v = (idx & 3) * 8;
        if (rr >= span) continue;
        *reinterpret_cast<uint4*>(xs + rr * PX + v) = xok[u] ? xq[u] : make_uint4(0, 0, 0, 0);
      }
      __syncthreads();
      if (tile + 1 < te) load(tile + 1);
#pragma unroll
      for (int grp = 0; grp < WG_BM / 32; ++grp) {
        const bf16x8 A = tr_frag(gs + (grp * 32 + 4 * gq_ + q) * PG + nt * 16 + 4 * p, PG);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
          const int pr = wsub + WPN * j;
          if (pr >= npairs) break;
          const int k = pr >> 1, ct = pr & 1;
          const bf16x8 Bf = tr_frag(xs + (grp * 32 + 4 * gq_ + q + k) * PX + ct * 16 + 4 * p, PX);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, Bf, acc[j], 0, 0, 0);
        }
      }
    }
  }
  for (int64_t tile = vec ? te : tb; tile < te; ++tile) {
    const int b = int(tile / tiles_per_seq);
    const int j0 = int(tile % tiles_per_seq) * WG_BM;
    __syncthreads();
    for (int idx = tid; idx < WG_BM * (BN / 8); idx += 256) {
      const int rr = idx / (BN / 8), v = (idx % (BN / 8)) * 8;
      const int j = j0 + rr;
      __bf16 vals[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int o = o0 + v + e;
        vals[e] = (j < d.Tvalid && o < no_per_g) ? gout[(int64_t(b) * d.Tvo + j) * d.ldo + out_col(d, g, o)]
                                                 : __bf16(0.f);
      }
      *reinterpret_cast<uint4*>(gs + rr * PG + v) = *reinterpret_cast<uint4*>(vals);
    }
    for (int idx = tid; idx < span * 4; idx += 256) {
      const int rr = idx >> 2, v = (idx & 3) * 8;
      const int t = j0 + d.q0 + k0 + rr;
      const int ch = cc + v;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (t >= 0 && t < d.Tv && ch < nred) {
        const int rph = ch / d.Cg, c = ch - rph * d.Cg;
        val = *reinterpret_cast<const uint4*>(x + (int64_t(b) * d.Tvs + t) * d.ldx + in_col(d, g, rph, c));
      }
      *reinterpret_cast<uint4*>(xs + rr * PX + v) = val;
    }
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < WG_BM / 32; ++grp) {
      const bf16x8 A = tr_frag(gs + (grp * 32 + 4 * gq_ + q) * PG + nt * 16 + 4 * p, PG);
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int pr = wsub + WPN * j;
        if (pr >= npairs) break;
        const int k = pr >> 1, ct = pr & 1;
        const bf16x8 Bf = tr_frag(xs + (grp * 32 + 4 * gq_ + q + k) * PX + ct * 16 + 4 * p, PX);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, Bf, acc[j], 0, 0, 0);
      }
    }
  }
  const int64_t nw = int64_t(d.G) * no_per_g * d.K * nred;
  float* pdst = part + int64_t(split) * nw;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int pr = wsub + WPN * j;
    if (pr >= npairs) break;
    const int k = k0 + (pr >> 1), ct = pr & 1;
    const int ch = cc + ct * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = o0 + nt * 16 + 4 * (lane >> 4) + e;
      if (o < no_per_g && ch < nred) pdst[((int64_t(g) * no_per_g + o) * d.K + k) * nred + ch] = acc[j][e];
    }
  }
}

// Weight gradient for one group with a contiguous reduction row and K <= 8
// taps (every MPD layer, the MSD's dense ones): the generator's k_wgrad3_bf16
// scheme on the dconv descriptor.  A block owns 32*NT output x 32*CT reduction
// channels x ALL taps over a contiguous range of 128-row tiles of one
// sequence: gout and x are read once per block (the 16-wide per-tap-group
// kernel above re-read them (N/32)*(nred/32) times, ~5% of the bf16 peak),
// double-buffered in LDS with a register prefetch of the next tile, operands
// through transposing reads, 32x32x16 MFMA.
constexpr int W3_BM = 128, W3_HALO = 64;

// bpart != nullptr: the bias partials of the same split too (per output column,
// summed from the staged gout tiles by the first reduction-channel block of
// each column block: gap rows are staged as zeros), replacing a separate pass
// over gout (k_dbias_part_v) per layer.
template <int NT, int CT, int MAXT>
__global__ __launch_bounds__(256) void k_dwgrad_w3(D d, const __bf16* __restrict__ gout, const __bf16* __restrict__ x,
                                                   int tiles_per_seq, int64_t n_tiles, int tiles_per_split,
                                                   float* __restrict__ part, int flat_p, float* __restrict__ bpart) {
  constexpr int NB = 32 * NT, CB = 32 * CT;
  constexpr int XROWS = W3_BM + W3_HALO;
  constexpr int GV = W3_BM * NB / 8 / 256;
  constexpr int XV = XROWS * CB / 8 / 256;
  constexpr int GS = NT * W3_BM * 32, XS = CT * XROWS * 32;
  constexpr int WPN = 4 / NT;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const base = reinterpret_cast<__bf16*>(smem);  // [buf]{G[NT][128][32], X[CT][192][32]}

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t split = blockIdx.x;
  const int n0 = blockIdx.y * NB, c0 = blockIdx.z * CB;
  const int nred = d.S * d.Cg;
  const int64_t tb = split * tiles_per_split;
  const int64_t te = tb + tiles_per_split < n_tiles ? tb + tiles_per_split : n_tiles;
  const int span = W3_BM + d.K - 1;
  const int P = CT * d.K;
  const int RG = P >= WPN ? 1 : WPN / P;
  const int WPP = WPN / RG;
  const int nt = wave / WPN, wsub = wave % WPN;
  const int rg = wsub / WPP, pw = wsub % WPP;
  const int RROWS = W3_BM / RG;

  uint4 gr[GV], xr[XV];
  bool gok[GV], xok[XV];
  // branch-free buffer loads (sel_common.h ru_bload): invalid rows and a dead
  // request (live = false) read nothing, so the request is counted exactly and
  // the MFMA phase does not wait on it
  auto load = [&](int64_t tile, bool live) {
    // flat_p > 0: one row space over all sequences (pitch flat_p, zero gaps; see
    // conv.hip dconv_ws_fwd), rows valid by their position in their sequence
    const int b = int(tile / tiles_per_seq);
    const int j0 = int(tile % tiles_per_seq) * W3_BM;
    const int nflat = flat_p * d.B;
    const __amdgpu_buffer_rsrc_t rg = ru_rsrc(gout + int64_t(b) * d.Tvo * d.ldo, int64_t(d.B - b) * d.Tvo * d.ldo);
    const __amdgpu_buffer_rsrc_t rx = ru_rsrc(x + int64_t(b) * d.Tvs * d.ldx, int64_t(d.B - b) * d.Tvs * d.ldx);
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      const int j = j0 + v / (NB / 8);
      gok[u] = flat_p ? j < nflat && j % flat_p < d.Tvalid : j < d.Tvalid;
      gr[u] = ru_bload(rg, live && gok[u] ? (j * d.ldo + n0 + (v % (NB / 8)) * 8) * 2 : RU_OOB);
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / (CB / 8);
      const int t = j0 + d.q0 + r;
      xok[u] = r < span && t >= 0 && (flat_p ? t < nflat && t % flat_p < d.Tv : t < d.Tv);
      xr[u] = ru_bload(rx, live && xok[u] ? (t * d.ldx + c0 + (v % (CB / 8)) * 8) * 2 : RU_OOB);
    }
  };
  auto store = [&](int buf) {
    __bf16* g = base + buf * (GS + XS);
    __bf16* xx = g + GS;
#pragma unroll
    for (int u = 0; u < GV; ++u) {
      const int v = tid + u * 256;
      const int r = v / (NB / 8), c8 = v % (NB / 8);
      *reinterpret_cast<uint4*>(g + (c8 >> 2) * (W3_BM * 32) + r * 32 + (c8 & 3) * 8) =
          gok[u] ? gr[u] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      if (u * 256 / (CB / 8) >= span) continue;
      const int v = tid + u * 256;
      const int r = v / (CB / 8), c8 = v % (CB / 8);
      *reinterpret_cast<uint4*>(xx + (c8 >> 2) * (XROWS * 32) + r * 32 + (c8 & 3) * 8) =
          xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
    }
  };

  int xoff[MAXT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    int p = pw + WPP * j;
    p = p < P ? p : P - 1;
    xoff[j] = (p / d.K) * (XROWS * 32) + (p % d.K) * 32;
  }
  floatx16 acc[MAXT];
#pragma unroll
  for (int j = 0; j < MAXT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  const int h = lane >> 5;
  const int col = ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
  const int q = (lane & 15) >> 2;
  const int lrow = (4 * h + q) * 32 + col;

  const bool bias_on = bpart != nullptr && blockIdx.z == 0;  // block-uniform
  const int bn = tid % NB;
  float bsum = 0.f;
  if (tb < te) load(tb, true);
  int buf = 0;
  for (int64_t tile = tb; tile < te; ++tile, buf ^= 1) {
    store(buf);
    __syncthreads();
    load(tile + 1 < te ? tile + 1 : tile, tile + 1 < te);  // unconditional: exact counts
    if (bias_on) {
      const __bf16* gb = base + buf * (GS + XS) + (bn >> 5) * (W3_BM * 32) + (bn & 31);
      for (int r = tid / NB; r < W3_BM; r += 256 / NB) bsum += float(gb[r * 32]);
    }
    const __bf16* g = base + buf * (GS + XS) + nt * (W3_BM * 32);
    const __bf16* xx = base + buf * (GS + XS) + GS;
    for (int kh = 0; kh < RROWS / 16; ++kh) {
      const int R = (rg * RROWS + kh * 16) * 32 + lrow;
      const v4i16 a0 = tr_read(g + R);
      const v4i16 a1 = tr_read(g + R + 8 * 32);
      const bf16x8 A = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const v4i16 b0 = tr_read(xx + xoff[j] + R);
        const v4i16 b1 = tr_read(xx + xoff[j] + R + 8 * 32);
        const bf16x8 Bf = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, Bf, acc[j], 0, 0, 0);
      }
    }
  }

  const int64_t nw = int64_t(d.Ng) * d.K * nred;
  float* pdst = part + split * nw;
  if (RG == 1) {
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      const int p = pw + WPP * j;
      if (p >= P) break;
      const int ct = p / d.K, k = p % d.K;
      const int c = c0 + ct * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        pdst[(int64_t(n) * d.K + k) * nred + c] = acc[j][r];
      }
    }
  } else {
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
      const int ct = pi / d.K, k = pi % d.K;
      const int n = n0 + ni * 32 + (e >> 5), c = c0 + ct * 32 + (e & 31);
      pdst[(int64_t(n) * d.K + k) * nred + c] = v;
    }
  }
  if (bias_on) {  // the 256 / NB row lanes of each column, added in lane order
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    red[tid] = bsum;
    __syncthreads();
    if (tid < NB) {
      float v = 0.f;
      for (int q = 0; q < 256 / NB; ++q) v += red[q * NB + tid];
      bpart[split * d.Ng + n0 + tid] = v;
    }
  }
}

// bias partials for the MFMA wgrad path: gb[col] over a split of rows.  Block =
// 64 output columns x 4 row lanes (a row's 64 columns are one coalesced read),
// row walk without divisions, the 4 lanes summed in LDS.
template <typename T>
__global__ __launch_bounds__(256) void k_dbias_part(D d, const T* __restrict__ gout, int rows_per_split,
                                                    float* __restrict__ bpart) {
  __shared__ float red[4][64];
  const int no_per_g = d.So * d.Ng;
  const int64_t nb = int64_t(d.G) * no_per_g;
  const int64_t total_rows = int64_t(d.B) * d.Tvalid;
  const int64_t r0 = int64_t(blockIdx.y) * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < total_rows ? r0 + rows_per_split : total_rows;
  const int cl = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int64_t go = int64_t(blockIdx.x) * 64 + cl;
  float acc = 0.f;
  if (go < nb) {
    const int g = int(go / no_per_g), o = int(go - int64_t(g) * no_per_g);
    const int64_t oc = out_col(d, g, o);
    int64_t rr = r0 + ly;
    int b = int(rr / d.Tvalid), j = int(rr - int64_t(b) * d.Tvalid);
    for (; rr < r1; rr += 4) {
      acc += to_f(gout[(int64_t(b) * d.Tvo + j) * d.ldo + oc]);
      j += 4;
      while (j >= d.Tvalid) j -= d.Tvalid, ++b;
    }
  }
  red[ly][cl] = acc;
  __syncthreads();
  if (ly == 0 && go < nb) bpart[int64_t(blockIdx.y) * nb + go] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// Vector form (bf16, So == 1, 8-aligned contiguous columns): a thread sums 8
// consecutive columns with 16-B loads over every 32nd row of the split, the 32
// row lanes are added in order through LDS (the scalar kernel above issued one
// 2-byte load per lane and row: ~1 TB/s).
__global__ __launch_bounds__(256) void k_dbias_part_v(D d, const __bf16* __restrict__ gout, int rows_per_split,
                                                      float* __restrict__ bpart) {
  __shared__ float red[32][65];
  const int64_t nb = int64_t(d.G) * d.Ng;
  const int64_t total_rows = int64_t(d.B) * d.Tvalid;
  const int64_t r0 = int64_t(blockIdx.y) * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < total_rows ? r0 + rows_per_split : total_rows;
  const int cg = threadIdx.x & 7, ly = threadIdx.x >> 3;
  const int64_t c0 = int64_t(blockIdx.x) * 64 + cg * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < nb) {
    int64_t rr = r0 + ly;
    int b = int(rr / d.Tvalid), j = int(rr - int64_t(b) * d.Tvalid);
    for (; rr < r1; rr += 32) {
      const uint4 raw = *reinterpret_cast<const uint4*>(gout + (int64_t(b) * d.Tvo + j) * d.ldo + c0);
      const __bf16* v = reinterpret_cast<const __bf16*>(&raw);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += float(v[e]);
      j += 32;
      while (j >= d.Tvalid) j -= d.Tvalid, ++b;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ly][cg * 8 + e] = acc[e];
  __syncthreads();
  const int64_t go = int64_t(blockIdx.x) * 64 + threadIdx.x;
  if (threadIdx.x < 64 && go < nb) {
    float t = 0.f;
    for (int l = 0; l < 32; ++l) t += red[l][threadIdx.x];
    bpart[int64_t(blockIdx.y) * nb + go] = t;
  }
}

// bias partials of a forward layer's gout: the vector kernel where it applies
// (tune key 25 = 1: the scalar one)
void launch_dbias_part(const sel_dconv_desc* d, const __bf16* gout, int rows_per_split, int bsplit, float* bpart,
                       hipStream_t s) {
  const int64_t nb = int64_t(d->G) * d->So * d->Ng;
  dim3 bg(unsigned((nb + 63) / 64), unsigned(bsplit));
  if (d->So == 1 && nb % 8 == 0 && d->ldo % 8 == 0 && tune(25) != 1)
    hipLaunchKernelGGL(k_dbias_part_v, bg, dim3(256), 0, s, *d, gout, rows_per_split, bpart);
  else
    hipLaunchKernelGGL(k_dbias_part<__bf16>, bg, dim3(256), 0, s, *d, gout, rows_per_split, bpart);
}

// Partial sums over groups of PRESUM splits (coalesced over the weights), so the
// final per-output reduction reads at most PRESUM partials.
constexpr int PRESUM = 16;
__global__ __launch_bounds__(256) void k_presum(const float* __restrict__ part, int nsplit, int64_t n,
                                                float* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int s0 = blockIdx.y * PRESUM, s1 = s0 + PRESUM < nsplit ? s0 + PRESUM : nsplit;
  float acc = 0.f;
  int sp = s0;
  for (; sp + 4 <= s1; sp += 4) {
    const float a0 = part[int64_t(sp) * n + i], a1 = part[int64_t(sp + 1) * n + i], a2 = part[int64_t(sp + 2) * n + i],
                a3 = part[int64_t(sp + 3) * n + i];
    acc += (a0 + a1) + (a2 + a3);
  }
  for (; sp < s1; ++sp) acc += part[int64_t(sp) * n + i];
  out[int64_t(blockIdx.y) * n + i] = acc;
}

// Weight gradient of the short-reduction layers (K * S * Cg = KR in {2, 3, 6, 15},
// one group, one output phase): block = a row range; thread = one output channel
// n x one row lane, KR + 1 accumulators (weights and bias) over its rows; the row
// lanes summed in LDS; one partial per block.
template <typename T, int KR>
__global__ __launch_bounds__(256) void k_dwgrad_short(D d, const T* __restrict__ gout, const T* __restrict__ x,
                                                      int rows_per_split, float* __restrict__ part,
                                                      float* __restrict__ bpart) {
  __shared__ float red[256 * (KR + 1) <= 4096 ? 256 * (KR + 1) : 4096];
  const int N = d.Ng;
  const int nl = N < 256 ? N : 256;  // lanes over n (N <= 256 here)
  const int RL = 256 / nl;
  const int n = threadIdx.x % nl, rl = threadIdx.x / nl;
  const int nred = d.S * d.Cg;
  const int64_t total_rows = int64_t(d.B) * d.Tvalid;
  const int64_t r0 = int64_t(blockIdx.x) * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < total_rows ? r0 + rows_per_split : total_rows;
  float acc[KR + 1];
#pragma unroll
  for (int e = 0; e <= KR; ++e) acc[e] = 0.f;
  int tap[KR], col[KR];  // hoisted as in k_dconv_short
#pragma unroll
  for (int e = 0; e < KR; ++e) {
    const int i = e / nred, rc = e - i * nred;
    const int r = rc / d.Cg, c = rc - r * d.Cg;
    tap[e] = d.q0 + i;
    col[e] = int(in_col(d, 0, r, c));
  }
  int64_t rr = r0 + rl;
  if (rr < r1 && threadIdx.x < nl * RL) {
    int b = int(rr / d.Tvalid), j = int(rr - int64_t(b) * d.Tvalid);
    for (; rr < r1; rr += RL) {
      const float gv = to_f(gout[(int64_t(b) * d.Tvo + j) * d.ldo + n]);
      const T* xb = x + int64_t(b) * d.Tvs * d.ldx;
#pragma unroll
      for (int e = 0; e < KR; ++e) {
        const int t = j + tap[e];
        if (t >= 0 && t < d.Tv) acc[e] = fmaf(gv, to_f(xb[int64_t(t) * d.ldx + col[e]]), acc[e]);
      }
      acc[KR] += gv;
      j += RL;
      while (j >= d.Tvalid) j -= d.Tvalid, ++b;
    }
  }
  // reduce the RL row lanes: red[rl][n][e]
#pragma unroll
  for (int e = 0; e <= KR; ++e) {
    if (threadIdx.x < nl * RL) red[(rl * nl + n) * (KR + 1) + e] = acc[e];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < nl * (KR + 1); o += 256) {
    float sum = 0.f;
    for (int l = 0; l < RL; ++l) sum += red[l * nl * (KR + 1) + o];
    const int nn = o / (KR + 1), e = o - nn * (KR + 1);
    if (e < KR) part[int64_t(blockIdx.x) * N * KR + int64_t(nn) * KR + e] = sum;
    else if (bpart) bpart[int64_t(blockIdx.x) * N + nn] = sum;
  }
}

// Staged weight gradient of the same layers (contiguous phase view, see
// k_dconv_shortx): a thread owns 2 output channels (one 4-B gout load per row)
// and 16 consecutive rows of each tile, whose x windows come from the tile staged
// in LDS, 4 rows per register window; blocks accumulate over their tiles and
// reduce their row lanes into one partial.  k_dwgrad_short's per-row global x
// loads ran the MSD's k15 1 -> 128 layer at 2.6 ms for 393 MB of gout.
template <typename T, int K, int NR>
__global__ __launch_bounds__(256) void k_dwgrad_shortx(D d, const T* __restrict__ gout, const T* __restrict__ x,
                                                       float* __restrict__ part, float* __restrict__ bpart) {
  constexpr int KR = K * NR, RR = 16, XW = (4 + K - 1) * NR;
  extern __shared__ float sh[];  // x window [(RB + K - 1) * NR], then the row-lane reduction [RL][Ng][KR + 1]
  const int N = d.Ng, NL = N / 2, RL = 256 / NL, RB = RL * RR;
  const int rl = threadIdx.x / NL, n = (threadIdx.x - rl * NL) * 2;
  float a0[KR + 1], a1[KR + 1];
#pragma unroll
  for (int e = 0; e <= KR; ++e) a0[e] = a1[e] = 0.f;
  const int tps = (d.Tvalid + RB - 1) / RB, ntiles = d.B * tps;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tps, j0 = (tile - b * tps) * RB;
    __syncthreads();
    for (int p = threadIdx.x; p < (RB + K - 1) * NR; p += 256) {
      const int t = j0 + d.q0 + p / NR;
      sh[p] = (t >= 0 && t < d.Tv) ? to_f(x[(int64_t(b) * d.Tvs + t) * NR + p % NR]) : 0.f;
    }
    __syncthreads();
    const T* grow = gout + int64_t(b) * d.Tvo * d.ldo + n;
#pragma unroll 1
    for (int q4 = 0; q4 < RR; q4 += 4) {
      const int jl = rl * RR + q4;
      if (j0 + jl >= d.Tvalid) break;
      float gx[4], gy[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + jl + r;
        gx[r] = gy[r] = 0.f;
        if (j < d.Tvalid) {
          const T* gp = grow + int64_t(j) * d.ldo;
          gx[r] = to_f(gp[0]);
          gy[r] = to_f(gp[1]);
        }
      }
      float xw[XW];
#pragma unroll
      for (int u = 0; u < XW; ++u) xw[u] = sh[jl * NR + u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e = 0; e < KR; ++e) {
          a0[e] = fmaf(gx[r], xw[r * NR + e], a0[e]);
          a1[e] = fmaf(gy[r], xw[r * NR + e], a1[e]);
        }
        a0[KR] += gx[r];
        a1[KR] += gy[r];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e <= KR; ++e) {
    sh[(rl * N + n) * (KR + 1) + e] = a0[e];
    sh[(rl * N + n + 1) * (KR + 1) + e] = a1[e];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < N * (KR + 1); o += 256) {
    float sum = 0.f;
    for (int l = 0; l < RL; ++l) sum += sh[l * N * (KR + 1) + o];
    const int nn = o / (KR + 1), e = o - nn * (KR + 1);
    if (e < KR) part[int64_t(blockIdx.x) * N * KR + int64_t(nn) * KR + e] = sum;
    else if (bpart) bpart[int64_t(blockIdx.x) * N + nn] = sum;
  }
}

// Final wgrad reduction: sum the split partials, unpack to the torch layout,
// and (weight norm) gv = (g/||v||) (gw - w_hat (w_hat . gw)), gg = w_hat . gw.
// One block per output channel n; the partials are walked in their packed
// (tap, phase, channel) order, so each split's slice is one coalesced read, and
// scattered once into the torch (channel, tap) positions.
__device__ __forceinline__ void dwgrad_finish_channel(const PackGeo& pg, const float* __restrict__ part, int nsplit,
                                                      const float* __restrict__ bpart, int bsplit,
                                                      const float* __restrict__ v, const float* __restrict__ wg,
                                                      float* __restrict__ gw, float* __restrict__ gg,
                                                      float* __restrict__ gb, int n);

__global__ __launch_bounds__(256) void k_dwgrad_finish(PackGeo pg, const float* __restrict__ part, int nsplit,
                                                       const float* __restrict__ bpart, int bsplit,
                                                       const float* __restrict__ v, const float* __restrict__ wg,
                                                       float* __restrict__ gw, float* __restrict__ gg,
                                                       float* __restrict__ gb) {
  dwgrad_finish_channel(pg, part, nsplit, bpart, bsplit, v, wg, gw, gg, gb, blockIdx.x);
}

// batched form (sel_dconv_wgrad_finish_many): the final reductions of several
// layers in one launch, block ranges per job in the kernel argument (a
// sub-discriminator's layers finish together after its chain backward instead
// of one launch per layer)
constexpr int DWF_MAXJ = 24;
struct DwgradJobs {
  PackGeo pg[DWF_MAXJ];
  const float* part[DWF_MAXJ];
  const float* bpart[DWF_MAXJ];
  const float* v[DWF_MAXJ];
  const float* wg[DWF_MAXJ];
  float* gw[DWF_MAXJ];
  float* gg[DWF_MAXJ];
  float* gb[DWF_MAXJ];
  int nsplit[DWF_MAXJ], bsplit[DWF_MAXJ];
  int bstart[DWF_MAXJ + 1];
  int njobs;
};

__global__ __launch_bounds__(256) void k_dwgrad_finish_many(DwgradJobs dj) {
  int j = 0;
  while (j + 1 < dj.njobs && int(blockIdx.x) >= dj.bstart[j + 1]) ++j;  // block-uniform
  dwgrad_finish_channel(dj.pg[j], dj.part[j], dj.nsplit[j], dj.bpart[j], dj.bsplit[j], dj.v[j], dj.wg[j], dj.gw[j],
                        dj.gg[j], dj.gb[j], int(blockIdx.x) - dj.bstart[j]);
}

__device__ __forceinline__ void dwgrad_finish_channel(const PackGeo& pg, const float* __restrict__ part, int nsplit,
                                                      const float* __restrict__ bpart, int bsplit,
                                                      const float* __restrict__ v, const float* __restrict__ wg,
                                                      float* __restrict__ gw, float* __restrict__ gg,
                                                      float* __restrict__ gb, int n) {
  __shared__ float red[16];
  __shared__ float bc[2];
  const int per = pg.Cg * pg.Kt;
  const int Ng = pg.N / pg.G, g = n / Ng, nl = n - g * Ng;
  const int nred = pg.s * pg.Cg;
  const int64_t nw = int64_t(pg.N) * pg.K * nred;
  const int64_t base = (int64_t(g) * Ng + nl) * pg.K * nred;
  float dot = 0.f, vv = 0.f;
  for (int e = threadIdx.x; e < pg.K * nred; e += 256) {
    const int i = e / nred, rc = e - i * nred;
    const int r = rc / pg.Cg, c = rc - r * pg.Cg;
    const int k = pg.s * (pg.q0 + i) + r + pg.pad;
    if (k < 0 || k >= pg.Kt) continue;  // structural zero of the phase view
    float acc = 0.f;
    int sp = 0;
    for (; sp + 4 <= nsplit; sp += 4) {  // 4 loads in flight, fixed order
      const float a0 = part[int64_t(sp) * nw + base + e], a1 = part[int64_t(sp + 1) * nw + base + e],
                  a2 = part[int64_t(sp + 2) * nw + base + e], a3 = part[int64_t(sp + 3) * nw + base + e];
      acc += (a0 + a1) + (a2 + a3);
    }
    for (; sp < nsplit; ++sp) acc += part[int64_t(sp) * nw + base + e];
    const int64_t o = int64_t(n) * per + c * pg.Kt + k;
    gw[o] = acc;
    if (v) {
      const float vv_ = v[o];
      dot += vv_ * acc;
      vv += vv_ * vv_;
    }
  }
  if (gb) {  // the bias partials of this n, spread over the block (fixed order per thread)
    float acc = 0.f;
    for (int sp = threadIdx.x; sp < bsplit; sp += 256) acc += bpart[int64_t(sp) * pg.N + n];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) gb[n] = acc;
  }
  if (!v) return;
  dot = block_sum(dot, red);
  if (threadIdx.x == 0) bc[0] = dot;
  vv = block_sum(vv, red);
  if (threadIdx.x == 0) bc[1] = vv;
  __syncthreads();
  const float nv = sqrtf(bc[1]);
  const float gn = wg[n];
  // w = gn * v / nv ; dL/dgn = (v . gw) / nv ; dL/dv = gn/nv * (gw - v (v . gw) / nv^2)
  if (threadIdx.x == 0) gg[n] = bc[0] / nv;
  const float a = gn / nv, bcoef = gn * bc[0] / (nv * nv * nv);
  __syncthreads();  // every gw[o] of this n written before the in-place update
  for (int e = threadIdx.x; e < per; e += 256) {
    const int64_t o = int64_t(n) * per + e;
    gw[o] = a * gw[o] - bcoef * v[o];
  }
}

}  // namespace dconv
}  // namespace sel

using namespace sel;
using namespace sel::dconv;

namespace {

struct WgPlanD {
  int flat_p;  // k_dwgrad_w3 flat tiling pitch (0: per-sequence tiles)
  bool mfma, shortk, shortx, w3;  // shortx: the short reduction on the staged kernel (k_dwgrad_shortx)
  int w3_nt, w3_ct, w3_maxt;
  int nsplit, bsplit;
  int rows_per_split, brows_per_split;
  int tiles_per_seq, tiles_per_split, ntg, nt;
};

// split-partial budget per layer (bytes; tune key 45 > 0: MB, A/B sweeps)
inline int64_t wg_cap() { return int64_t(tune(45) > 0 ? tune(45) : 64) << 20; }

// the staged short weight-gradient kernel has an instance for (K, nred)
bool dwshortx_inst(int K, int nred) {
#define SEL_DWSX_HAS(K_, NR_) \
  if (K == K_ && nred == NR_) return true;
  SEL_DSHORTX_TABLE(SEL_DWSX_HAS)
#undef SEL_DWSX_HAS
  return false;
}

// the k_dwgrad_w3<NT, CT, MAXT> instances wg_plan can ask for: (nt, ct) in
// {1, 2}^2 and K = 1..8 give exactly these 16 (MAXT = per-wave pair count
// ceil(CT K / (waves per pair set)), 6..8 rounded up to the 8-slot form);
// tests/test_dconv_cases_host.py holds this list to that enumeration
#define SEL_W3_TABLE(X)                                   \
  X(1, 1, 1) X(1, 1, 2)                                   \
  X(1, 2, 1) X(1, 2, 2) X(1, 2, 3) X(1, 2, 4)             \
  X(2, 1, 1) X(2, 1, 2) X(2, 1, 3) X(2, 1, 4)             \
  X(2, 2, 1) X(2, 2, 2) X(2, 2, 3) X(2, 2, 4) X(2, 2, 5) X(2, 2, 8)

// the launch of the instance the plan names (p.w3_nt, p.w3_ct, p.w3_maxt)
template <int NT, int CT, int MAXT>
hipError_t launch_w3(const sel_dconv_desc* d, const WgPlanD& p, const void* gout, const void* x, float* part,
                     float* bpart, hipStream_t s) {
  const int width = d->So * d->Ng;
  const int nred = d->S * d->Cg;
  const int NB = 32 * p.w3_nt, CB = 32 * p.w3_ct;
  const size_t lds = 2 * (size_t(p.w3_nt) * W3_BM * 32 + size_t(p.w3_ct) * (W3_BM + W3_HALO) * 32) * sizeof(__bf16);
  const int64_t ntiles = p.flat_p ? p.tiles_per_seq : int64_t(d->B) * p.tiles_per_seq;
  dim3 grid(unsigned(p.nsplit), unsigned(width / NB), unsigned(nred / CB));
  auto kern = k_dwgrad_w3<NT, CT, MAXT>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, *d, static_cast<const __bf16*>(gout),
                     static_cast<const __bf16*>(x), p.tiles_per_seq, ntiles, p.tiles_per_split, part, p.flat_p, bpart);
  return hipGetLastError();  // (bias partials: in the kernel, p.bsplit == p.nsplit)
}

// Which weight-gradient kernel a layer takes and how its rows are split: the
// single decision the launcher (wgrad_fill) and sel_dconv_wgrad_kernel use.
WgPlanD wg_plan(const sel_dconv_desc* d, int dtype) {
  WgPlanD p{};
  const int width = d->So * d->Ng;
  const int nred = d->S * d->Cg;
  p.mfma = dtype == SEL_BF16 && d->Cg % 8 == 0 && d->Cs % 8 == 0 && d->ldx % 8 == 0 && nred % 8 == 0 &&
           width % 16 == 0 && tune(9) != 1;
  const int64_t rows = int64_t(d->B) * d->Tvalid;
  const int64_t nw = int64_t(d->G) * width * d->K * nred;
  p.shortk = !p.mfma && tune(9) != 1 && d->G == 1 && d->So == 1 && d->Ng <= 256 && (256 % d->Ng) == 0 &&
             short_kr_ok(d->K * nred);
  if (p.shortk) {
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(2048, rows / 64));
    p.rows_per_split = int((rows + want - 1) / want);
    p.nsplit = int((rows + p.rows_per_split - 1) / p.rows_per_split);
    p.bsplit = p.nsplit;
    // staged kernel (tune key 18: 1 = off) where the phase view is contiguous
    p.shortx = tune(18) != 1 && d->Cs == d->Cg && d->ldx == nred && d->Ng % 2 == 0 && d->ldo % 2 == 0 &&
               int64_t(d->B) * d->Tvo < (int64_t(1) << 31) && dwshortx_inst(d->K, nred);
    return p;
  }
  p.w3 = p.mfma && d->G == 1 && d->So == 1 && (d->S == 1 || d->Cs == d->Cg) && d->K <= 8 && width % 32 == 0 &&
         nred % 32 == 0 && d->ldo % 8 == 0 && tune(16) != 1 &&
         // gout and x as buffer resources (ru_rsrc): ru_region_ok
         ru_region_ok(int64_t(d->B) * d->Tvo * d->ldo * 2) && ru_region_ok(int64_t(d->B) * d->Tvs * d->ldx * 2);
  if (p.w3) {
    p.w3_nt = width % 64 == 0 ? 2 : 1;
    p.w3_ct = nred % 64 == 0 ? 2 : 1;
    const int P = p.w3_ct * d->K, WPN = 4 / p.w3_nt;
    const int RG = P >= WPN ? 1 : WPN / P, WPP = WPN / RG;
    const int need = (P + WPP - 1) / WPP;
    // exact per-wave tile count where an instance exists (the MPD's K = 5 layers at
    // 64 input channels per block: 5 pairs per wave, which the 8-slot form ran
    // with 3 of 8 MFMA slots computing never-stored accumulators)
    p.w3_maxt = need <= 5 ? need : 8;
    // flat tiling across zero-gapped sequences (the conditions of conv.hip
    // dconv_ws_fwd; tune key 26 = 1: off): short MPD columns fill whole tiles
    const int P_ = d->Tvo;
    p.flat_p = tune(26) != 1 && d->Tvs == P_ && P_ - d->Tv >= -d->q0 && P_ - d->Tvalid >= d->q0 + d->K - 1 &&
                       int64_t(d->B) * P_ < (int64_t(1) << 31)
                   ? P_ : 0;
    p.tiles_per_seq = p.flat_p ? int((int64_t(d->B) * P_ + W3_BM - 1) / W3_BM) : (d->Tvalid + W3_BM - 1) / W3_BM;
    const int64_t ntiles = p.flat_p ? p.tiles_per_seq : int64_t(d->B) * p.tiles_per_seq;
    const int64_t blocks = int64_t(width / (32 * p.w3_nt)) * (nred / (32 * p.w3_ct));
    int64_t want = std::max<int64_t>(1, (512 + blocks - 1) / blocks);
    want = std::min<int64_t>(want, std::max<int64_t>(1, wg_cap() / (nw * 4)));
    want = std::min<int64_t>(want, std::max<int64_t>(1, ntiles));
    p.tiles_per_split = int((ntiles + want - 1) / want);
    p.nsplit = int((ntiles + p.tiles_per_split - 1) / p.tiles_per_split);
  } else if (p.mfma) {
    p.nt = width % 32 == 0 ? 2 : 1;
    p.ntg = (d->K + WG_TAPS - 1) / WG_TAPS;
    p.tiles_per_seq = (d->Tvalid + WG_BM - 1) / WG_BM;
    const int64_t ntiles = int64_t(d->B) * p.tiles_per_seq;
    const int64_t blocks = int64_t(d->G) * ((width + 16 * p.nt - 1) / (16 * p.nt)) * ((nred + 31) / 32) * p.ntg;
    int64_t want = std::max<int64_t>(1, (1024 + blocks - 1) / blocks);
    want = std::min<int64_t>(want, std::max<int64_t>(1, wg_cap() / (nw * 4)));
    want = std::min<int64_t>(want, std::max<int64_t>(1, ntiles));
    p.tiles_per_split = int((ntiles + want - 1) / want);
    p.nsplit = int((ntiles + p.tiles_per_split - 1) / p.tiles_per_split);
  } else {
    const int64_t want_threads = int64_t(1) << 20;
    int64_t want = std::max<int64_t>(1, want_threads / std::max<int64_t>(1, nw + int64_t(d->G) * width));
    want = std::min<int64_t>(want, std::max<int64_t>(1, wg_cap() / ((nw + width * d->G) * 4)));
    want = std::min<int64_t>(want, std::max<int64_t>(1, rows));
    p.rows_per_split = int((rows + want - 1) / want);
    p.nsplit = int((rows + p.rows_per_split - 1) / p.rows_per_split);
  }
  int64_t bwant = std::max<int64_t>(1, std::min<int64_t>(256, rows / 256));
  p.brows_per_split = int((rows + bwant - 1) / bwant);
  p.bsplit = int((rows + p.brows_per_split - 1) / std::max(1, p.brows_per_split));
  if (p.bsplit < 1) p.bsplit = 1;
  if (p.w3) p.bsplit = p.nsplit;  // k_dwgrad_w3 writes the bias partials of its own splits
  return p;
}

// bias partials the final reduction reads (the VALU kernel writes one per row split)
inline int wg_bsplit(const WgPlanD& p) { return (p.mfma || p.shortk) ? p.bsplit : p.nsplit; }

size_t wg_bytes(const sel_dconv_desc* d, const WgPlanD& p) {
  const int64_t width = int64_t(d->So) * d->Ng;
  const int64_t nw = int64_t(d->G) * width * d->K * d->S * d->Cg;
  const int64_t nb = int64_t(d->G) * width;
  const int64_t ng = (p.nsplit + PRESUM - 1) / PRESUM;
  return size_t(int64_t(p.nsplit) * nw + int64_t(std::max(p.bsplit, p.nsplit)) * nb + (ng + 1) * nw) * sizeof(float) +
         256;
}

hipError_t wgrad_fill(const sel_dconv_desc* d, int dtype, const WgPlanD& p, const void* gout, const void* x,
                      float* part, float* bpart, hipStream_t s) {
  const int width = d->So * d->Ng;
  const int nred = d->S * d->Cg;
  if (p.shortk) {
    const int kr = d->K * nred;
    if (p.shortx) {
      const int rl = 256 / (d->Ng / 2), rb = rl * 16;
      const size_t lds = std::max<size_t>(size_t(rb + d->K - 1) * nred, size_t(rl) * d->Ng * (kr + 1)) * sizeof(float);
      void (*kx)(D, const __bf16*, const __bf16*, float*, float*) = nullptr;
      void (*kf)(D, const float*, const float*, float*, float*) = nullptr;
#define SEL_DWSX(K_, NR_)                                                       \
  if (d->K == K_ && nred == NR_) {                                              \
    kx = k_dwgrad_shortx<__bf16, K_, NR_>;                                      \
    kf = k_dwgrad_shortx<float, K_, NR_>;                                       \
  }
      SEL_DSHORTX_TABLE(SEL_DWSX)
#undef SEL_DWSX
      if (!kx) return hipErrorInvalidValue;
      const void* kern = dtype == SEL_BF16 ? (const void*)kx : (const void*)kf;
      if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
      }
      if (dtype == SEL_BF16)
        hipLaunchKernelGGL(kx, dim3(p.nsplit), dim3(256), lds, s, *d, static_cast<const __bf16*>(gout),
                           static_cast<const __bf16*>(x), part, bpart);
      else
        hipLaunchKernelGGL(kf, dim3(p.nsplit), dim3(256), lds, s, *d, static_cast<const float*>(gout),
                           static_cast<const float*>(x), part, bpart);
      return hipGetLastError();
    }
#define SEL_DWS(TT, KR)                                                                                     \
  hipLaunchKernelGGL((k_dwgrad_short<TT, KR>), dim3(p.nsplit), dim3(256), 0, s, *d, static_cast<const TT*>(gout), \
                     static_cast<const TT*>(x), p.rows_per_split, part, bpart)
#define SEL_DWS_T(TT) \
  if (kr == 2) SEL_DWS(TT, 2); else if (kr == 3) SEL_DWS(TT, 3); else if (kr == 6) SEL_DWS(TT, 6); else SEL_DWS(TT, 15);
    if (dtype == SEL_BF16) { SEL_DWS_T(__bf16) } else { SEL_DWS_T(float) }
#undef SEL_DWS_T
#undef SEL_DWS
    return hipGetLastError();
  }
  if (p.w3) {
#define SEL_W3(NT_, CT_, MT_)                                 \
  if (p.w3_nt == NT_ && p.w3_ct == CT_ && p.w3_maxt == MT_) \
    return launch_w3<NT_, CT_, MT_>(d, p, gout, x, part, bpart, s);
    SEL_W3_TABLE(SEL_W3)
#undef SEL_W3
    return hipErrorInvalidValue;
  }
  if (p.mfma) {
    const int bn = 16 * p.nt;
    dim3 grid(unsigned(d->G * ((width + bn - 1) / bn)), unsigned((nred + 31) / 32), unsigned(p.nsplit * p.ntg));
    const size_t lds = (size_t(WG_BM) * (bn + 16) + size_t(WG_BM + WG_TAPS - 1) * 48) * sizeof(__bf16);
    if (p.nt == 2)
      hipLaunchKernelGGL(k_dwgrad_mfma<2>, grid, dim3(256), lds, s, *d, static_cast<const __bf16*>(gout),
                         static_cast<const __bf16*>(x), p.tiles_per_seq, p.tiles_per_split, p.ntg, part);
    else
      hipLaunchKernelGGL(k_dwgrad_mfma<1>, grid, dim3(256), lds, s, *d, static_cast<const __bf16*>(gout),
                         static_cast<const __bf16*>(x), p.tiles_per_seq, p.tiles_per_split, p.ntg, part);
    if (bpart) launch_dbias_part(d, static_cast<const __bf16*>(gout), p.brows_per_split, p.bsplit, bpart, s);
    return hipGetLastError();
  }
  const int64_t nw = int64_t(d->G) * width * d->K * nred;
  const int64_t nb = bpart ? int64_t(d->G) * width : 0;
  dim3 grid(unsigned(std::min<int64_t>((nw + nb + 255) / 256, 65535)), unsigned(p.nsplit));
  if (dtype == SEL_BF16)
    hipLaunchKernelGGL(k_dwgrad_valu<__bf16>, grid, dim3(256), 0, s, *d, static_cast<const __bf16*>(gout),
                       static_cast<const __bf16*>(x), p.rows_per_split, part, bpart);
  else
    hipLaunchKernelGGL(k_dwgrad_valu<float>, grid, dim3(256), 0, s, *d, static_cast<const float*>(gout),
                       static_cast<const float*>(x), p.rows_per_split, part, bpart);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int sel_dconv_wgrad_kernel(const sel_dconv_desc* d, int dtype, char* name, size_t cap, int32_t plan[4]) {
  if (!d || check(d) != SEL_OK || (dtype != SEL_BF16 && dtype != SEL_F32) || d->So != 1) return -1;
  const WgPlanD p = wg_plan(d, dtype);
  const int nred = d->S * d->Cg;
  if (name && cap) {
    const char* t = dtype == SEL_BF16 ? "bf16" : "float";
    if (p.shortk && p.shortx) snprintf(name, cap, "k_dwgrad_shortx<%s, %d, %d>", t, d->K, nred);
    else if (p.shortk) snprintf(name, cap, "k_dwgrad_short<%s, %d>", t, d->K * nred);
    else if (p.w3) snprintf(name, cap, "k_dwgrad_w3<%d, %d, %d>", p.w3_nt, p.w3_ct, p.w3_maxt);
    else if (p.mfma) snprintf(name, cap, "k_dwgrad_mfma<%d>", p.nt);
    else snprintf(name, cap, "k_dwgrad_valu<%s>", t);
  }
  if (plan) {
    plan[0] = p.nsplit;
    plan[1] = (p.w3 || p.mfma) ? p.tiles_per_split : p.rows_per_split;
    plan[2] = wg_bsplit(p);
    plan[3] = p.flat_p;
  }
  return SEL_OK;
}

int sel_dconv_w3_instances(int32_t* triples, int cap) {
  static const int32_t tab[][3] = {
#define SEL_W3_ROW(NT_, CT_, MT_) {NT_, CT_, MT_},
      SEL_W3_TABLE(SEL_W3_ROW)
#undef SEL_W3_ROW
  };
  const int n = int(sizeof(tab) / sizeof(tab[0]));
  for (int i = 0; triples && i < n && i < cap; ++i)
    for (int e = 0; e < 3; ++e) triples[3 * i + e] = tab[i][e];
  return n;
}

size_t sel_dconv_wgrad_workspace(const sel_dconv_desc* d, int dtype) {
  if (!d || check(d) != SEL_OK) return 16;
  return wg_bytes(d, wg_plan(d, dtype));
}

int sel_dconv_wgrad(const sel_dconv_desc* d, int dtype, const void* gout, const void* x, int N, int Cg, int Kt,
                    int stride, int pad, const float* v, const float* wg, float* gw, float* gg, float* gb, void* ws,
                    size_t ws_bytes, sel_stream_t stream) {
  sel_dwgrad_job job;
  if (int rc = sel_dconv_wgrad_partials(d, dtype, gout, x, N, Cg, Kt, stride, pad, v, wg, gw, gg, gb, ws, ws_bytes,
                                        &job, stream))
    return rc;
  const PackGeo pg = pack_geo(job.N, job.Cg, job.Kt, job.stride, job.pad, job.G);
  hipLaunchKernelGGL(k_dwgrad_finish, dim3(job.N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pg,
                     job.part, job.nsplit, job.bpart, job.bsplit, job.v, job.wg, job.gw, job.gg, job.gb);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_dconv_wgrad_finish_many(const sel_dwgrad_job* jobs, int njobs, sel_stream_t stream) {
  SEL_REQUIRE(njobs >= 0 && (njobs == 0 || jobs), SEL_ERR_ARG, "bad wgrad finish job list");
  for (int j = 0; j < njobs; ++j) {
    const sel_dwgrad_job& J = jobs[j];
    SEL_REQUIRE(J.part && J.gw && J.N > 0 && J.Cg > 0 && J.Kt > 0 && J.stride > 0 && J.pad >= 0 && J.G > 0 &&
                    J.N % J.G == 0 && J.nsplit > 0 && J.nsplit <= PRESUM && (!J.gb || (J.bpart && J.bsplit > 0)) &&
                    (!J.v || (J.wg && J.gg)),
                SEL_ERR_ARG, "bad wgrad finish job %d", j);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int j = 0;
  while (j < njobs) {
    DwgradJobs dj{};
    int n = 0, blocks = 0;
    for (; j < njobs && n < DWF_MAXJ; ++j, ++n) {
      const sel_dwgrad_job& J = jobs[j];
      dj.pg[n] = pack_geo(J.N, J.Cg, J.Kt, J.stride, J.pad, J.G);
      dj.part[n] = J.part;
      dj.bpart[n] = J.bpart;
      dj.nsplit[n] = J.nsplit;
      dj.bsplit[n] = J.bsplit;
      dj.v[n] = J.v;
      dj.wg[n] = J.wg;
      dj.gw[n] = J.gw;
      dj.gg[n] = J.gg;
      dj.gb[n] = J.gb;
      dj.bstart[n] = blocks;
      blocks += J.N;
    }
    dj.bstart[n] = blocks;
    dj.njobs = n;
    hipLaunchKernelGGL(k_dwgrad_finish_many, dim3(unsigned(blocks)), dim3(256), 0, s, dj);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

int sel_dconv_wgrad_partials(const sel_dconv_desc* d, int dtype, const void* gout, const void* x, int N, int Cg,
                             int Kt, int stride, int pad, const float* v, const float* wg, float* gw, float* gg,
                             float* gb, void* ws, size_t ws_bytes, sel_dwgrad_job* job, sel_stream_t stream) {
  SEL_REQUIRE(job != nullptr, SEL_ERR_ARG, "sel_dconv_wgrad_partials: job is NULL");
  if (int rc = check(d)) return rc;
  SEL_REQUIRE(dtype == SEL_BF16 || dtype == SEL_F32, SEL_ERR_UNSUPPORTED, "dtype %d", dtype);
  SEL_REQUIRE(d->So == 1 && d->S == stride && d->G * d->Ng == N && d->Cg == Cg, SEL_ERR_ARG,
              "sel_dconv_wgrad: descriptor must be the forward layer's");
  const PackGeo pg = pack_geo(N, Cg, Kt, stride, pad, d->G);
  SEL_REQUIRE(pg.K == d->K && pg.q0 == d->q0, SEL_ERR_ARG, "tap geometry mismatch (K %d vs %d, q0 %d vs %d)",
              pg.K, d->K, pg.q0, d->q0);
  SEL_REQUIRE(!v || (wg && gg), SEL_ERR_ARG, "weight norm needs v, g and gg");
  const WgPlanD p = wg_plan(d, dtype);
  SEL_REQUIRE(ws_bytes >= wg_bytes(d, p), SEL_ERR_WORKSPACE, "wgrad workspace too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(ws);
  const int64_t nw = int64_t(N) * d->K * d->S * d->Cg;
  float* bpart = gb ? part + int64_t(p.nsplit) * nw : nullptr;
  SEL_HIP(wgrad_fill(d, dtype, p, gout, x, part, bpart, s));
  const int bsplit = wg_bsplit(p);
  int nsplit = p.nsplit;
  if (nsplit > PRESUM) {  // fold the partials to <= PRESUM per weight before the per-output pass
    float* tmp = part + int64_t(p.nsplit) * nw + int64_t(std::max(p.bsplit, p.nsplit)) * N;
    float* src = part;
    while (nsplit > PRESUM) {
      const int ng = (nsplit + PRESUM - 1) / PRESUM;
      float* dst = src == part ? tmp : part;
      hipLaunchKernelGGL(k_presum, dim3(unsigned((nw + 255) / 256), unsigned(ng)), dim3(256), 0, s, src, nsplit, nw,
                         dst);
      src = dst;
      nsplit = ng;
    }
    part = src;
  }
  *job = sel_dwgrad_job{part, bpart, v, wg, gw, gg, gb, N, Cg, Kt, stride, pad, d->G, nsplit, bsplit};
  return SEL_OK;
}

}  // extern "C"
