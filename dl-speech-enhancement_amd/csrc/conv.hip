// AudioDec conv stack on gfx950 (layers/conv_layer.py, models/autoencoder*/modules/*):
// the forward primitive.
//
// One primitive (see include/sel.h): a stride-1, K-tap, dilated conv over
// channels-last rows, as an implicit GEMM on MFMA.
//   rows  m = (b, t)  -> GEMM M,   output channels n -> GEMM N,
//   reduction r = (tap k, in-channel c).
// A workgroup (4 waves, 2x2) owns a BM x BN output tile.  For each 32-channel
// chunk it stages the input rows [m0 - pad, m0 + BM + (K-1)*dil - pad) ONCE in
// LDS (the causal halo) and re-reads them for every tap (K-fold reuse, the
// point of the implicit GEMM), while the packed weight slice of each tap is
// staged next to it.  ELU of the input is applied while staging (fusing
// residual_unit.py:32 into the conv prologue); bias, ELU-backward multiplier
// and residual add are fused into the epilogue.
//   fp32:  v_mfma_f32_16x16x4_f32 (exact fp32, parity path)
//   bf16:  v_mfma_f32_16x16x32_bf16 with fp32 accumulation (C3 path)
// This file holds every form of it (generic, fp32 tiles, pipelined bf16 tiles,
// the two warp-specialised kernels, thin, pointwise, single-channel) with their
// launchers and the one dispatch decision (fwd_pick), and the discriminator's
// shim onto the warp-specialised kernels (dconv_ws_*).  The fused residual-unit
// kernels live in conv_ru.hip, the weight gradients in conv_wgrad.hip, the
// sample-tile kernel in conv_wss.hip; weight packing, the replicate-pad fix-up
// and the cast in conv_pack.hip.  Device helpers shared with conv_ru.hip or
// conv_wgrad.hip are in conv_tile.h.
#include <algorithm>

#include "conv_tile.h"

namespace sel {
namespace conv {

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int n = 4; };
template <> struct Vec16<__bf16> { static constexpr int n = 8; };

// Forward primitive.  Per 32-channel chunk: stage the input rows (with halo) and
// the packed weights of ALL K taps once, one barrier pair, then K x TM x TN MFMAs
// per wave.  Epilogue goes through LDS so every lane stores/loads 16 B vectors.
template <typename TI, typename TO, int BM, int BN>
__global__ __launch_bounds__(256) void k_conv_fwd(Args a, const TI* __restrict__ in,
                                                  const TI* __restrict__ wp,
                                                  const float* __restrict__ bias,
                                                  const TO* __restrict__ aux,
                                                  const TO* __restrict__ res, TO* __restrict__ out) {
  constexpr int P = Pitch<TI>::v;
  constexpr int TM = BM / 32, TN = BN / 32;  // 16x16 tiles per wave (2x2 waves)
  constexpr int OP = BN + 4;                 // fp32 epilogue tile pitch
  extern __shared__ __align__(16) unsigned char smem[];
  const int halo = (a.K - 1) * a.dil;
  const int span = BM + halo;
  TI* xs = reinterpret_cast<TI*>(smem);
  TI* ws = xs + span * P;  // [K][BN][P]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = int64_t(blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  const int64_t g0 = m0 - a.pad;

  // per-lane output rows: local row and time index inside its sample
  int lr[TM], tt[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    lr[i] = wm * (BM / 2) + i * 16 + (lane & 15);
    const int64_t m = m0 + lr[i];
    tt[i] = m < a.rows ? int(m % a.T) : -(1 << 30);
  }

  floatx4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.C; c0 += CK) {
    __syncthreads();
    stage_rows<TI>(in, a, g0, span, c0, xs, a.in_elu != 0);
    for (int k = 0; k < a.K; ++k) stage_w<TI, BN>(wp, a, n0, k, c0, ws + k * BN * P);
    __syncthreads();
    for (int k = 0; k < a.K; ++k) {
      const TI* wk = ws + k * BN * P;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        int ti = tt[i] + k * a.dil - a.pad;
        bool valid = ti >= 0 && ti < a.T;
        int xr = lr[i] + k * a.dil;
        if (!valid && a.pad_mode == SEL_PAD_REPLICATE && tt[i] >= 0) {
          const int tc = ti < 0 ? 0 : a.T - 1;
          xr = lr[i] + a.pad + tc - tt[i];
          valid = true;
        }
        const TI* xrow = xs + (valid ? xr : 0) * P;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int nc = wn * (BN / 2) + j * 16 + (lane & 15);
          mma_chunk(acc[i][j], xrow, wk + nc * P, lane, valid);
        }
      }
    }
  }

  // epilogue: accumulators -> LDS (fp32) -> 16-B vectors with bias / ELU' / residual
  __syncthreads();
  float* ot = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * (BN / 2) + j * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) ot[(wm * (BM / 2) + i * 16 + 4 * (lane >> 4) + e) * OP + col] = acc[i][j][e];
    }
  __syncthreads();
  constexpr int V = Vec16<TO>::n;
  const bool vec_ok = (a.N % V) == 0;
  for (int idx = threadIdx.x; idx < BM * (BN / V); idx += blockDim.x) {
    const int r = idx / (BN / V), cv = (idx % (BN / V)) * V;
    const int64_t m = m0 + r;
    const int n = n0 + cv;
    if (m >= a.rows || n >= a.N) continue;
    const int64_t o = m * a.N + n;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int ne = n + e;
      const float bv = (bias && a.bias_period && ne < a.N) ? bias[ne % a.bias_period] : 0.f;
      v[e] = ot[r * OP + cv + e] + bv;
    }
    if (vec_ok) {
      if (aux) {
        TO av[V];
        *reinterpret_cast<uint4*>(av) = *reinterpret_cast<const uint4*>(aux + o);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] *= elu_grad(to_f(av[e]));
      }
      if (res) {
        TO rv[V];
        *reinterpret_cast<uint4*>(rv) = *reinterpret_cast<const uint4*>(res + o);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] += to_f(rv[e]);
      }
      TO ov[V];
#pragma unroll
      for (int e = 0; e < V; ++e) ov[e] = from_f<TO>(v[e]);
      *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<uint4*>(ov);
    } else {
      for (int e = 0; e < V && n + e < a.N; ++e) {
        float x = v[e];
        if (aux) x *= elu_grad(to_f(aux[o + e]));
        if (res) x += to_f(res[o + e]);
        out[o + e] = from_f<TO>(x);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fp32 forward primitive on sample-aligned tiles (the reference-precision path;
// also every fp32 dgrad, as the forward of the adjoint descriptor).  BM x BN
// output tile, 4 waves of (BM / WM) x 32, v_mfma_f32_16x16x4_f32.  Per
// 16-channel chunk the input span (tile + halo, ELU applied once, zero- or
// replicate-filled per sample: no masks in the MFMA loop) and the weights of
// all K taps are staged in LDS (80-B rows: conflict-free 16-B fragment reads;
// 16 instead of 32 channels keeps the K = 7 stage at 46 KB, 3 workgroups per
// CU, where the generic kernel's 82 KB allowed one), and the next chunk's
// rows and weights are fetched into registers (16-B loads) during this
// chunk's MFMAs.  Epilogue as k_conv_fwd (bias, ELU'(aux), residual, in that
// order) through an fp32 LDS tile.
constexpr int FF_CK = 16, FF_P = 20, FF_HALO = 64;
template <int BM, int BN>
constexpr int ff_xv() { return ((BM + FF_HALO) * (FF_CK / 4) + 255) / 256; }
template <int KM, int BM, int BN>
__global__ __launch_bounds__(256) void k_conv_fwd_f32(Args a, const float* __restrict__ in,
                                                      const float* __restrict__ wp, const float* __restrict__ bias,
                                                      const float* __restrict__ aux, const float* __restrict__ res,
                                                      float* __restrict__ out) {
  constexpr int WN = BN / 32, WM = 4 / WN, TM = BM / WM / 16, TN = 2;
  constexpr int XV = ff_xv<BM, BN>();
  constexpr int WV = (KM * BN * (FF_CK / 4) + 255) / 256;
  extern __shared__ __align__(16) unsigned char smem[];
  float* const xs = reinterpret_cast<float*>(smem);      // [BM + halo][FF_P]
  float* const ws = xs + (BM + FF_HALO) * FF_P;          // [K][BN][FF_P]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tps = (a.T + BM - 1) / BM;
  const int64_t b = blockIdx.x / tps;
  const int t0 = int(blockIdx.x - b * tps) * BM;
  const int n0 = blockIdx.y * BN;
  const int span = BM + (a.K - 1) * a.dil;
  const float* __restrict__ xb = in + b * a.T * int64_t(a.C);

  // raw loads and their predicates: the zero select happens in put(), after
  // the next chunk's MFMAs (a select right behind a load waits for it)
  floatx4 xr[XV], wr[WV];
  bool xok[XV];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      const int r = v >> 2, c = c0 + (v & 3) * 4;
      int ti = t0 - a.pad + r;
      bool ok = r < span;
      if (ti < 0 || ti >= a.T) {
        if (a.pad_mode == SEL_PAD_ZERO) ok = false;
        ti = ti < 0 ? 0 : a.T - 1;
      }
      // unconditional load of a clamped (valid) row: a load under a
      // per-element condition becomes a branch with its own vmcnt(0) wait
      xr[u] = *reinterpret_cast<const floatx4*>(xb + int64_t(ti) * a.C + c);
      xok[u] = ok;
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int v = tid + u * 256;
      const int q = v & 3, row = v >> 2;  // row = k * BN + n
      const int k = row / BN, n = row % BN;
      const int kc = k < a.K ? k : a.K - 1;  // taps past K: never stored
      wr[u] = *reinterpret_cast<const floatx4*>(wp + (int64_t(n0 + n) * a.K + kc) * a.C + c0 + 4 * q);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      const int r = v >> 2;
      const bool ok = xok[u];
      floatx4 x = floatx4{ok ? xr[u][0] : 0.f, ok ? xr[u][1] : 0.f, ok ? xr[u][2] : 0.f, ok ? xr[u][3] : 0.f};
      if (a.in_elu) x = floatx4{elu(x[0]), elu(x[1]), elu(x[2]), elu(x[3])};
      if (r < BM + FF_HALO) *reinterpret_cast<floatx4*>(xs + r * FF_P + (v & 3) * 4) = x;
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int v = tid + u * 256;
      // (the stage holds K, not KM, taps)
      if ((v >> 2) < a.K * BN) *reinterpret_cast<floatx4*>(ws + (v >> 2) * FF_P + (v & 3) * 4) = wr[u];
    }
  };

  floatx4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int arow = wm * (BM / WM) + (lane & 15);
  const int g4 = 4 * (lane >> 4);
  fetch(0);
  for (int c0 = 0; c0 < a.C; c0 += FF_CK) {
    __syncthreads();  // every wave is done with the previous chunk
    put();
    __syncthreads();
    if (c0 + FF_CK < a.C) fetch(c0 + FF_CK);
    for (int k = 0; k < a.K; ++k) {
      float4 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const float4*>(xs + (arow + 16 * i + k * a.dil) * FF_P + g4);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bv[j] = *reinterpret_cast<const float4*>(ws + (k * BN + wn * 32 + 16 * j + (lane & 15)) * FF_P + g4);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
        }
    }
  }
  // epilogue: accumulators -> LDS (fp32) -> 16-B vectors with bias / ELU' / residual
  constexpr int OP = BN + 4;
  __syncthreads();
  float* ot = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * 32 + j * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) ot[(wm * (BM / WM) + i * 16 + g4 + e) * OP + col] = acc[i][j][e];
    }
  __syncthreads();
  const int mrows = a.T - t0 < BM ? a.T - t0 : BM;
  for (int idx = tid; idx < BM * (BN / 4); idx += 256) {
    const int r = idx / (BN / 4), cv = (idx % (BN / 4)) * 4;
    if (r >= mrows) continue;
    const int64_t o = (b * a.T + t0 + r) * a.N + n0 + cv;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ne = n0 + cv + e;
      const float bv = (bias && a.bias_period) ? bias[ne % a.bias_period] : 0.f;
      v[e] = ot[r * OP + cv + e] + bv;
    }
    if (aux) {
      const float4 av = *reinterpret_cast<const float4*>(aux + o);
      v[0] *= elu_grad(av.x), v[1] *= elu_grad(av.y), v[2] *= elu_grad(av.z), v[3] *= elu_grad(av.w);
    }
    if (res) {
      const float4 rv = *reinterpret_cast<const float4*>(res + o);
      v[0] += rv.x, v[1] += rv.y, v[2] += rv.z, v[3] += rv.w;
    }
    *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---------------------------------------------------------------------------
// bf16 forward primitive (the hot one).  Per 32-channel chunk the input rows
// [m0 - pad, m0 + BM + (K-1)*dil - pad) are staged ONCE (ELU applied once per
// element) together with the packed weights of all K taps; the K taps then
// re-read the staged rows at shifted offsets (implicit GEMM).  The next
// chunk's rows/weights are fetched into registers while the current chunk's
// MFMAs run (T14 issue-early / write-late), and all global loads are branch-free
// (clamped address + select; requires C % 32 == 0) so hipcc emits no per-element
// fallback waits.  MFMA: v_mfma_f32_32x32x16_bf16; staged rows are 80 B apart,
// which makes its 16-B fragment reads bank-conflict free.
// ---------------------------------------------------------------------------

template <int BM, int BN, int WAVES_M, int KMAX, typename TO>
__global__ __launch_bounds__(256) void k_conv_fwd_bf16(Args a, const __bf16* __restrict__ in,
                                                       const __bf16* __restrict__ wp,
                                                       const float* __restrict__ bias,
                                                       const TO* __restrict__ aux, const TO* __restrict__ res,
                                                       TO* __restrict__ out, int ncol) {
  constexpr int P = F4_P;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int XV = ((BM + F4_HALOMAX) * 4 + 255) / 256;
  constexpr int WV = (KMAX * BN * 4 + 255) / 256;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);
  const int halo = (a.K - 1) * a.dil;
  const int span = BM + halo;
  __bf16* const ws = xs + span * P;  // [k][BN][P]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  // sample-aligned tiles: every output row of the block belongs to sample b, so
  // the causal zero / replicate padding is resolved once while staging and the
  // MFMA loop needs no per-tap row validity (blocks past T are clipped at store)
  const int tps = (a.T + BM - 1) / BM;
  int64_t mt;
  int nt;
  xcd_tile(ncol, mt, nt);
  const int64_t b = mt / tps;
  const int t0 = int(mt % tps) * BM;
  const int64_t m0 = b * a.T + t0;
  const int mrows = a.T - t0 < BM ? a.T - t0 : BM;
  const int n0 = nt * BN;
  const int nchunk = a.C / CK;

  // staging row r <-> input time t0 - pad + r of sample b; per-thread source
  // pointers computed once (chunks only add the channel offset)
  const __bf16* xsrc[XV];
  bool xok[XV];
#pragma unroll
  for (int u = 0; u < XV; ++u) {
    const int r = (tid + u * 256) >> 2;
    int ti = t0 - a.pad + r;
    const bool inside = ti >= 0 && ti < a.T;
    xok[u] = r < span && (inside || a.pad_mode == SEL_PAD_REPLICATE);
    ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
    xsrc[u] = in + (b * a.T + ti) * a.C + ((tid + u * 256) & 3) * 8;
  }
  const __bf16* wsrc[WV];
  bool wok[WV];
#pragma unroll
  for (int u = 0; u < WV; ++u) {
    const int v = tid + u * 256;
    const int k = v / (BN * 4), n = (v >> 2) % BN;
    const bool ok = k < a.K && n0 + n < a.N;
    wok[u] = ok;
    wsrc[u] = wp + (int64_t(ok ? n0 + n : 0) * a.K + (ok ? k : 0)) * a.C + (v & 3) * 8;
  }
  uint4 xr[XV], wr[WV];
  auto load = [&](int c0) {
#pragma unroll
    for (int u = 0; u < XV; ++u) xr[u] = *reinterpret_cast<const uint4*>(xsrc[u] + c0);  // masked in store()
#pragma unroll
    for (int u = 0; u < WV; ++u) wr[u] = *reinterpret_cast<const uint4*>(wsrc[u] + c0);
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = tid + u * 256;
      if ((v >> 2) >= span) continue;
      // zero-fill AFTER the wait: masking right at the load would make hipcc wait
      // on the load there (vmcnt(0)) and serialise the register prefetch
      uint4 val = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
      if (a.in_elu) {
        val = elu8(val);
      }
      *reinterpret_cast<uint4*>(xs + (v >> 2) * P + (v & 3) * 8) = val;
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int v = tid + u * 256;
      const int k = v / (BN * 4), n = (v >> 2) % BN;
      const uint4 val = wok[u] ? wr[u] : make_uint4(0, 0, 0, 0);
      if (k < a.K) *reinterpret_cast<uint4*>(ws + (k * BN + n) * P + (v & 3) * 8) = val;
    }
  };

  // per-lane output row of each 32-row tile -> its staged-row offset
  int lr[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) lr[i] = (wm * WTM + i * 32 + (lane & 31)) * P;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load(0);
  for (int ch = 0; ch < nchunk; ++ch) {
    if (ch) __syncthreads();
    store();
    __syncthreads();
    if (ch + 1 < nchunk) load((ch + 1) * CK);
    for (int k = 0; k < a.K; ++k) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // two K=16 halves of the 32-channel chunk
        const int co = 16 * h + 8 * (lane >> 5);
        bf16x8 bf[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bf[j] = *reinterpret_cast<const bf16x8*>(ws + (k * BN + wn * WTN + j * 32 + (lane & 31)) * P + co);
        const int kofs = k * a.dil * P + co;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + lr[i] + kofs);
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[j], af, acc[i][j], 0, 0, 0);
        }
      }
    }
  }

  // epilogue straight from the accumulators (operands were swapped, so C/D is
  // out^T): lane -> output row m = lane & 31 of its 32-row tile, element r ->
  // n = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5): four runs of 4 consecutive
  // channels, each stored as one 8-B (bf16) / 16-B (fp32) vector.
  const bool bias_vec = bias && a.bias_period && (a.bias_period % 4) == 0;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int r = wm * WTM + i * 32 + (lane & 31);
    if (r >= mrows) continue;
    const int64_t m = m0 + r;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * WTN + j * 32 + 8 * g + 4 * (lane >> 5);
        if (n >= a.N) continue;
        const int64_t o = m * a.N + n;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e];
        if (bias_vec) {
          const float4 bv = *reinterpret_cast<const float4*>(bias + (n % a.bias_period));
          v[0] += bv.x, v[1] += bv.y, v[2] += bv.z, v[3] += bv.w;
        } else if (bias && a.bias_period) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (n + e < a.N) v[e] += bias[(n + e) % a.bias_period];
        }
        if (a.N % 4 == 0) {
          if (aux) {
            TO av[4];
            if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(av) = *reinterpret_cast<const uint2*>(aux + o);
            else *reinterpret_cast<uint4*>(av) = *reinterpret_cast<const uint4*>(aux + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= elu_grad_fast(to_f(av[e]));
          }
          if (res) {
            TO rv[4];
            if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(rv) = *reinterpret_cast<const uint2*>(res + o);
            else *reinterpret_cast<uint4*>(rv) = *reinterpret_cast<const uint4*>(res + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += to_f(rv[e]);
          }
          TO ov[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) ov[e] = from_f<TO>(v[e]);
          if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(out + o) = *reinterpret_cast<uint2*>(ov);
          else *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<uint4*>(ov);
        } else {
          for (int e = 0; e < 4 && n + e < a.N; ++e) {
            float x = v[e];
            if (aux) x *= elu_grad_fast(to_f(aux[o + e]));
            if (res) x += to_f(res[o + e]);
            out[o + e] = from_f<TO>(x);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Warp-specialised bf16 forward for the wide layers at few rows (256 output
// channels at T = 400 x 64 clips: the RU256 k7 forwards and dgrads, the
// 640 -> 256 phase-view strided conv).  The tiled kernel above runs those at
// 2 waves per SIMD with staging (ELU + LDS stores) and MFMAs in separate
// barrier phases: SQ counters show the matrix pipe busy 28% of the kernel and
// ~3,700 VALU instructions per wave, as many issue cycles as its MFMAs
// (profiles/r2_ws_conv.md).  Here one 256 x 128 tile per CU, 12 waves:
//   waves 0-7  consumers: 4 x 2 grid of 64 x 64 wave tiles; per 16-channel
//              chunk K taps x 4 MFMAs, the next tap's fragments read while the
//              current tap's MFMAs run;
//   waves NC..NC+3 producers: global -> LDS DMA (global_load_lds_dwordx4) of the
//              input span and the K weight slices three chunks ahead into a
//              4-slot LDS ring, then the input ELU in place one chunk ahead;
//   all 12:    the epilogue, through an fp32 LDS tile with row-contiguous 16-B
//              global accesses.
// One barrier per chunk.  LDS rows are 32 B (16 channels) with the 16-B slot
// XOR-swizzled by row bit 3 (conflict-free ds_read_b128 for both MFMA operands);
// the DMA destination is lane-linear, so the swizzle is applied to the SOURCE
// address.  Padding rows are DMA'd from a zero buffer.
// Measured limits (block stamps, tools/ws_probe.py): consumers alone run the
// main loop at ~75% of the MFMA pipe (2.1 GHz); the producers' DMA into LDS
// costs the consumers ~900 cycles per chunk and lowers the clock to ~1.87 GHz,
// the in-place ELU ~3 us per launch; one wave of 256 tiles leaves the prologue
// and the epilogue (~2 us fwd, ~4 us with aux + res) exposed.
// ---------------------------------------------------------------------------
constexpr int WS_BM = 256, WS_BN = 128, WS_CK = 16, WS_NBUF = 4;
constexpr int WS_RPI = 1024 / (WS_CK * 2);    // LDS rows per 1-KB DMA piece
constexpr int WS_SPR = WS_CK / 8;             // 16-B slots per LDS row
constexpr int WS_XROWS = WS_BM + F4_HALOMAX;  // staged input rows per chunk (multiple of WS_RPI)
constexpr int WS_CMAX = 4096;                 // input channels the zero source covers
constexpr int WS_EP = WS_BN + 4;              // fp32 epilogue tile pitch (conflict-free 16-B writes)

__device__ __attribute__((aligned(64))) __bf16 g_ws_zero[WS_CMAX];

// XOR pattern of LDS row `row`'s 16-B slots: conflict-free ds_read_b128 of 16
// consecutive rows per lane group for both row widths (brute-force checked)
__device__ __forceinline__ int ws_swzbits(int row) { return WS_CK == 16 ? (row >> 3) & 1 : (row >> 2) & 3; }
// element offset of 16-B slot `slot` of LDS row `row` (WS_CK channels)
__device__ __forceinline__ int ws_swz(int row, int slot) { return row * WS_CK + ((slot ^ ws_swzbits(row)) << 3); }

inline size_t ws_buf_bytes(int K) { return (size_t(WS_XROWS) + size_t(K) * WS_BN) * WS_CK * 2; }
// CPB chunks per barrier: the ring has 4 * CPB slots and slots free CPB at a time
inline size_t ws_lds_bytes(int K, int cpb = 1) {
  return std::max(size_t(WS_NBUF) * cpb * ws_buf_bytes(K), size_t(WS_BM) * WS_EP * sizeof(float));
}

// DMA piece of producer wave pw's u-th slot: q = 4u + pw, clamped to the last piece
template <int TI>
__device__ __forceinline__ int ws_piece(int u, int pw) {
  return u * 4 + pw < TI ? u * 4 + pw : TI - 1;
}

// In-place input ELU of producer wave pw's input pieces (q = 4u + pw < XI) of
// one ring slot: each lane rewrites exactly the 16 B its own DMA wrote, so this
// wave's vmcnt wait alone orders it (elementwise, so the swizzle does not
// matter).  Inline-asm LDS access: hipcc would put vmcnt(0) before a plain LDS
// read while DMAs are in flight, draining the next chunk's prefetch too.
template <int PW>
__device__ __forceinline__ void ws_elu_pieces(unsigned char* lane_base, int pw, int xi) {
#pragma unroll
  for (int u = 0; u < PW; ++u) {
    const int q = u * 4 + pw;
    if (q >= xi) break;
    const unsigned addr = unsigned(reinterpret_cast<uintptr_t>(lane_base + q * 1024));
    bf16x8 val;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(val) : "v"(addr) : "memory");
    val = __builtin_bit_cast(bf16x8, elu8(__builtin_bit_cast(uint4, val)));
    asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(val) : "memory");
  }
}

template <int KT, typename TO, int NC, int CPB>
__global__ __launch_bounds__((NC + 4) * 64) void k_conv_ws_bf16(Args a, const __bf16* __restrict__ in,
                                                      const __bf16* __restrict__ wp,
                                                      const float* __restrict__ bias, const TO* __restrict__ aux,
                                                      const TO* __restrict__ res, TO* __restrict__ out, int ncol,
                                                      int dbg) {
  constexpr int BM = WS_BM, BN = WS_BN;
  // NC consumer waves as 4 x 2 (64 x 64 each) or 2 x 2 (128 x 64: six fragment
  // reads per eight MFMAs instead of four per four)
  static_assert(NC == 8 || NC == 4, "consumer waves");
  constexpr int NT = (NC + 4) * 64;
  constexpr int TM = 16 / NC, TN = 2, WTM = 32 * TM, WTN = 64;
  constexpr int XI = WS_XROWS / WS_RPI;  // DMA pieces (1 KB) per chunk: input span
  constexpr int WI = KT * BN / WS_RPI;   // weight slices
  constexpr int TI = XI + WI;
  constexpr int PW = (TI + 3) / 4;   // per producer wave (the last one repeats its final piece)
  constexpr int BUF = (WS_XROWS + KT * BN) * WS_CK;  // bf16 elements per ring slot
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const lds = reinterpret_cast<__bf16*>(smem);
  const int halo = (KT - 1) * a.dil;
  const int span = BM + halo;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // diagnostic (tune key 13 bit 3): per-block start / end stamps (100 MHz
  // realtime) and hardware ids into the output buffer instead of results
  const uint64_t t_start = (dbg & 8) ? __builtin_amdgcn_s_memrealtime() : 0;
  const uint64_t c_start = (dbg & 8) ? __builtin_amdgcn_s_memtime() : 0;
  uint64_t t_loop = 0;
  const int tps = (a.T + BM - 1) / BM;
  int64_t mt;
  int nt;
  xcd_tile(ncol, mt, nt);
  const int64_t b = mt / tps;
  const int t0 = int(mt % tps) * BM;
  const int64_t m0 = b * a.T + t0;
  const int mrows = a.T - t0 < BM ? a.T - t0 : BM;
  const int n0 = nt * BN;
  const int nchunk = a.C / WS_CK;

  if (wave >= NC) {
    // ---------------- producers ----------------
    const int pw = wave - NC;
    // DMA piece q (1 KB) goes to producer wave q % 4 (the input pieces, which
    // get the ELU pass, spread over all four); a wave short of PW repeats its last
    const __bf16* src[PW];
#pragma unroll
    for (int u = 0; u < PW; ++u) {
      const int q = ws_piece<TI>(u, pw);
      if (q < XI) {
        const int R = q * WS_RPI + lane / WS_SPR, ls = (lane % WS_SPR) ^ ws_swzbits(R);
        int ti = t0 - a.pad + R;
        const bool valid =
            R < span && (a.seq_pitch > 0 ? ti >= 0 && ti < a.T && ti % a.seq_pitch < a.tin_valid
                                         : (ti >= 0 && ti < a.tin_valid) || a.pad_mode == SEL_PAD_REPLICATE);
        // flat tiling: ti is a row of the whole row space (b == 0) and `valid`
        // already keeps it in range; only the per-sequence form clamps into
        // the sequence (replicate pad)
        if (a.seq_pitch == 0) ti = ti < 0 ? 0 : (ti >= a.tin_valid ? a.tin_valid - 1 : ti);
        src[u] = valid ? in + (b * a.tin_pitch + ti) * a.ldx + 8 * ls : g_ws_zero + 8 * ls;
      } else {
        const int R = (q - XI) * WS_RPI + lane / WS_SPR, ls = (lane % WS_SPR) ^ ws_swzbits(R);
        const int k = R / BN, n = R % BN;
        src[u] = wp + (int64_t(n0 + n) * KT + k) * a.C + 8 * ls;
      }
    }
    auto issue = [&](int ch) {
      unsigned char* const base = smem + (ch % (WS_NBUF * CPB)) * (BUF * 2);
#pragma unroll
      for (int u = 0; u < PW; ++u) {
        const int q = ws_piece<TI>(u, pw);
        if ((dbg & 32) && q < XI) continue;   // diagnostic: no input DMA (tune key 13 bit 5)
        if ((dbg & 64) && q >= XI) continue;  // diagnostic: no weight DMA (tune key 13 bit 6)
        const int off = q < XI ? q * 1024 : WS_XROWS * WS_CK * 2 + (q - XI) * 1024;
        __builtin_amdgcn_global_load_lds((const void*)(src[u] + ch * WS_CK), (lds_ptr_t)(base + off), 16, 0, 0);
      }
    };
      const int xi_used = (span + WS_RPI - 1) / WS_RPI;  // input pieces holding rows < span (the rest stay zero)
    auto elu_pass = [&](int ch) __attribute__((always_inline)) {
      ws_elu_pieces<PW>(smem + (ch % (WS_NBUF * CPB)) * (BUF * 2) + lane * 16, pw, xi_used);
    };
    // stages of CPB chunks, one barrier per stage
    const int nst = (nchunk + CPB - 1) / CPB;
    if (dbg & 1) {  // diagnostic: consumers alone (tune key 13 bit 0)
      for (int st = 0; st <= nst; ++st) __syncthreads();
    } else {
    // ring of NB = 4 CPB slots, prefetch distance D = NB - CPB chunks (slots are
    // released a stage at a time); wait_chunk(n): chunk landed with n younger
    // chunks still allowed in flight
    constexpr int NB = WS_NBUF * CPB, D = NB - CPB;
    static_assert(D >= 1 && 2 * CPB * PW < 64, "ring depth / vmcnt range");
    auto wait_chunk = [&](int younger) __attribute__((always_inline)) {
      if (younger >= 4 && 2 * CPB >= 4) ws_wait_vm<(2 * CPB >= 4 ? 4 * PW : 0)>();
      else if (younger == 3 && 2 * CPB >= 3) ws_wait_vm<(2 * CPB >= 3 ? 3 * PW : 0)>();
      else if (younger >= 2) ws_wait_vm<2 * PW>();
      else if (younger == 1) ws_wait_vm<PW>();
      else ws_wait_vm<0>();
    };
    for (int c = 0; c < D && c < nchunk; ++c) issue(c);
    // stage 0 landed (its last chunk with the younger ones in flight), then its ELU
    wait_chunk(std::min(D, nchunk) - std::min(CPB, nchunk));
    if (a.in_elu && !(dbg & 16))  // bit 4: diagnostic without the ELU pass
      for (int c = 0; c < CPB && c < nchunk; ++c) elu_pass(c);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int st = 0; st < nst; ++st) {
      // issue first: the slots of stage st-1 were released by the last barrier,
      // and the count below assumes chunks up to min(st CPB + D + CPB - 1,
      // nchunk - 1) are out
      const int c0 = st * CPB;
      for (int c = c0 + D; c < c0 + D + CPB && c < nchunk; ++c) issue(c);
      if (c0 + CPB < nchunk) {
        // stage st+1 landed (later chunks may still be in flight), then its ELU
        const int issued = std::min(c0 + D + CPB, nchunk) - 1;
        const int need = std::min(c0 + 2 * CPB, nchunk) - 1;
        wait_chunk(issued - need);
        if (a.in_elu && !(dbg & 16))
          for (int c = c0 + CPB; c < c0 + 2 * CPB && c < nchunk; ++c) elu_pass(c);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    }
  } else {
  // ---------------- consumers ----------------
  const int wm = wave >> 1, wn = wave & 1;
  const int hl = lane >> 5;
  int arow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) arow[i] = wm * WTM + i * 32 + (lane & 31);
  int boff[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) boff[j] = WS_XROWS * WS_CK + ws_swz(wn * WTN + j * 32 + (lane & 31), hl);

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  __syncthreads();
  // consumers outrank the producers in the SIMD's issue arbitration (tune key
  // 13 bit 7 = diagnostic without)
  if (!(dbg & 128)) __builtin_amdgcn_s_setprio(2);
  for (int ch = 0; ch < nchunk; ++ch) {
    // one barrier per stage of CPB chunks (after its last chunk)
    const bool stage_end = (ch + 1) % CPB == 0 || ch + 1 == nchunk;
    if (dbg & 2) {  // diagnostic: producers alone (tune key 13 bit 1)
      if (stage_end) __syncthreads();
      continue;
    }
    const __bf16* const xb = lds + (ch % (WS_NBUF * CPB)) * BUF;
    bf16x8 fa[2][TM], fb[2][TN];
    constexpr int NS = KT * (WS_CK / 16);  // (tap, 16-channel half) steps
    // slot bit 1 <-> element offset bit 4 (row * 32 keeps bits 0-4 clear)
    auto fetch = [&](int st, int q) {
      const int k = st / (WS_CK / 16), h = st % (WS_CK / 16);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[q][j] = *reinterpret_cast<const bf16x8*>(xb + ((boff[j] + k * BN * WS_CK) ^ (16 * h)));
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[q][i] = *reinterpret_cast<const bf16x8*>(xb + ws_swz(arow[i] + k * a.dil, 2 * h + hl));
    };
    for (int rep = 0; rep < ((dbg & 256) ? 2 : 1); ++rep) {  // bit 8: diagnostic double MFMA work
    fetch(0, 0);
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      // pin the order: the next step's fragment reads go out before this step's MFMAs
      if (st + 1 < NS) fetch(st + 1, (st + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[st & 1][j], fa[st & 1][i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    }
    if (stage_end) __syncthreads();
  }

  __builtin_amdgcn_s_setprio(0);
  if (dbg & 8) {
    if (tid == 0) t_loop = __builtin_amdgcn_s_memrealtime();
  }
  if (!(dbg & 4)) {
    // accumulators -> fp32 tile [BM][BN + 4] over the (drained) ring: lane ->
    // row lane & 31 of its 32-row tile, element r -> column (r & 3) + 8 (r >> 2)
    // + 4 (lane >> 5), i.e. four 16-B runs per accumulator
    float* const tile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r = wm * WTM + i * 32 + (lane & 31);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          floatx4 v4;
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = acc[i][j][4 * g + e];
          *reinterpret_cast<floatx4*>(tile + r * WS_EP + wn * WTN + j * 32 + 8 * g + 4 * hl) = v4;
        }
    }
  }
  }
  if (dbg & 4) return;  // diagnostic: no epilogue (tune key 13 bit 2)
  __syncthreads();

  // epilogue by all NC + 4 waves: 8 consecutive channels per thread, row-contiguous
  // 16-B global accesses (aux / res fetched for every vector first)
  struct alignas(16) V8 { TO v[8]; };
  constexpr int EV = (BM * BN / 8 + NT - 1) / NT;
  const float* const tile = reinterpret_cast<const float*>(smem);
  const int nvec = mrows * (BN / 8);
  V8 av[EV], rv[EV];
#pragma unroll
  for (int u = 0; u < EV; ++u) {
    const int v = tid + u * NT;
    if (v >= nvec) break;
    const int64_t o = (m0 + (v >> 4)) * a.ldo + n0 + (v & 15) * 8;
    if (aux) av[u] = *reinterpret_cast<const V8*>(aux + o);
    if (res) rv[u] = *reinterpret_cast<const V8*>(res + o);
  }
#pragma unroll
  for (int u = 0; u < EV; ++u) {
    const int v = tid + u * NT;
    if (v >= nvec) break;
    const int row = v >> 4, c8 = (v & 15) * 8;
    const int64_t o = (m0 + row) * a.ldo + n0 + c8;
    const floatx4 lo = *reinterpret_cast<const floatx4*>(tile + row * WS_EP + c8);
    const floatx4 hi = *reinterpret_cast<const floatx4*>(tile + row * WS_EP + c8 + 4);
    float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    if (a.epi) {
      // discriminator epilogue (k_dconv_mfma order): + bias, + res, * LeakyReLU'(aux),
      // LeakyReLU; rows past the computed ones are the next layer's zero padding
      const bool valid = (a.seq_pitch > 0 ? (t0 + row) % a.seq_pitch : t0 + row) < a.tout_valid;
      float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (bias) {
        const floatx4 b0 = *reinterpret_cast<const floatx4*>(bias + n0 + c8);
        const floatx4 b1 = *reinterpret_cast<const floatx4*>(bias + n0 + c8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = b0[e], bv[e + 4] = b1[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float y = 0.f;
        if (valid) {
          y = x[e];
          if (bias) y += bv[e];
          if (res) y += to_f(rv[u].v[e]);
          if (aux) y *= to_f(av[u].v[e]) > 0.f ? 1.f : a.slope;
          if (a.act) y = y > 0.f ? y : y * a.slope;
        }
        x[e] = y;
      }
    } else {
    if (bias && a.bias_period) {
      if (a.bias_period % 8 == 0) {
        const float* const bp = bias + (n0 + c8) % a.bias_period;
        const floatx4 b0 = *reinterpret_cast<const floatx4*>(bp), b1 = *reinterpret_cast<const floatx4*>(bp + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] += b0[e], x[e + 4] += b1[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] += bias[(n0 + c8 + e) % a.bias_period];
      }
    }
    if (aux) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] *= elu_grad_fast(to_f(av[u].v[e]));
    }
    if (res) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] += to_f(rv[u].v[e]);
    }
    }
    V8 ov;
#pragma unroll
    for (int e = 0; e < 8; ++e) ov.v[e] = from_f<TO>(x[e]);
    *reinterpret_cast<V8*>(out + o) = ov;
  }
  if ((dbg & 8) && bias && !a.bias_period) {
    // diagnostic (tune key 13 bit 3): per-block stamps into a scratch "bias"
    // buffer: realtime (100 MHz) start / main-loop end / block end, shader
    // clock start / end, HW_ID, XCC_ID
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      uint64_t* st = reinterpret_cast<uint64_t*>(const_cast<float*>(bias)) +
                     8 * (int64_t(blockIdx.y) * gridDim.x + blockIdx.x);
      st[0] = t_start;
      st[1] = t_loop;
      st[2] = __builtin_amdgcn_s_memrealtime();
      st[3] = c_start;
      st[4] = __builtin_amdgcn_s_memtime();
      st[5] = uint64_t(__builtin_amdgcn_s_getreg(4 | (31 << 11)));   // HW_ID
      st[6] = uint64_t(__builtin_amdgcn_s_getreg(20 | (31 << 11)));  // XCC_ID
    }
  }
}

// ---------------------------------------------------------------------------
// Eight-wave form of the warp-specialised kernel (k_conv_ws8).  Same LDS ring
// layout, swizzle, DMA sources and (chunk, tap) MFMA order as k_conv_ws_bf16,
// hence bit-identical outputs, but:
//   - no producer waves: each of the 8 waves issues its share of the chunk's
//     1-KB DMA pieces (q = 8u + wave) and ELUs the input pieces it DMA'd;
//   - 128 x 64 per wave (4 x 2 MFMA tiles of 32 x 32): six fragment reads per
//     eight MFMAs instead of four per four, at 2 waves per SIMD with the
//     256-VGPR budget the 128 accumulators need;
//   - block tiles of 256 x 256 (the MPD's 512 / 1024-wide layers: half the
//     weight-slice DMA per flop of a 256 x 128 tile) or 512 x 128 (the 128-wide
//     k7 dgrads at T = 2000: 4 tiles per sample, 256 per launch);
//   - a 3-slot ring: chunk c + 2 is issued while chunk c is computed, chunk
//     c + 1 is waited for (counted vmcnt, never 0 while a later chunk is in
//     flight) after the first tap of chunk c, one raw barrier per chunk.
// The LDS image per chunk is what the 12-wave kernel's producers build, so
// the DMA and the ELU are unchanged; the LDS reads per flop fall by a quarter
// and the DMA'd weight bytes per flop by up to a half.
// ---------------------------------------------------------------------------
template <int KT, int BM, int BN, int HALO, int TM = 4>
struct Ws8 {
  static constexpr int WTM = 32 * TM;               // wave tile rows (x 64 columns)
  static constexpr int WM = BM / WTM, WN = BN / 64;  // wave grid
  static_assert(WM * WN == 8 && BM % 128 == 0, "eight wave tiles");
  static constexpr int XROWS = BM + HALO;           // staged input rows per chunk
  static constexpr int XI = XROWS / WS_RPI;         // input pieces (1 KB = 32 rows x 16 channels)
  static constexpr int WI = KT * BN / WS_RPI;       // weight pieces
  static constexpr int TI = XI + WI;
  static constexpr int PW = (TI + 7) / 8;           // pieces per wave per chunk
  static constexpr int NB = 3;                      // ring slots
  static constexpr int BUF = (XROWS + KT * BN) * WS_CK;  // bf16 elements per slot
  static constexpr int EP = BN + 4;                 // fp32 epilogue pitch (conflict-free 16-B writes)
  static constexpr size_t RING = size_t(NB) * BUF * 2;
  // epilogue pass rows: 256 where that fp32 tile fits over the ring (the 512 x
  // 128 tiles: 2 passes instead of 4, half the exposed aux / res load latency)
  static constexpr int PR = (BM >= 256 && size_t(256) * EP * 4 <= RING) ? 256 : 128;
  static constexpr size_t EPI = size_t(PR) * EP * 4;
  static constexpr size_t LDS = RING > EPI ? RING : EPI;
  static_assert(XROWS % WS_RPI == 0 && WI * WS_RPI == KT * BN && LDS <= 160 * 1024, "LDS");
  static_assert(2 * PW < 64, "vmcnt range");
};

template <int PW>
__device__ __forceinline__ void ws8_elu_pieces(unsigned char* slot, int lane, int wave, int xi) {
#pragma unroll
  for (int u = 0; u < PW; ++u) {
    const int q = u * 8 + wave;
    if (q >= xi) break;
    const unsigned addr = unsigned(reinterpret_cast<uintptr_t>(slot + q * 1024 + lane * 16));
    bf16x8 val;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(val) : "v"(addr) : "memory");
    val = __builtin_bit_cast(bf16x8, elu8(__builtin_bit_cast(uint4, val)));
    asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(val) : "memory");
  }
}

template <int KT, typename TO, int BM, int BN, int HALO, int TM>
__global__ __launch_bounds__(512) void k_conv_ws8(Args a, const __bf16* __restrict__ in,
                                                  const __bf16* __restrict__ wp, const float* __restrict__ bias,
                                                  const TO* __restrict__ aux, const TO* __restrict__ res,
                                                  TO* __restrict__ out, int ncol, int dbg) {
  // dbg (tune key 13, diagnostics only): bit 0 = no DMA in the loop, bit 1 =
  // no MFMAs, bit 2 = no barriers in the loop, bit 3 = no epilogue
  using G = Ws8<KT, BM, BN, HALO, TM>;
  constexpr int PW = G::PW, XI = G::XI, TI = G::TI, NB = G::NB, BUF = G::BUF, XROWS = G::XROWS;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const lds = reinterpret_cast<__bf16*>(smem);
  const int span = BM + (KT - 1) * a.dil;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tps = (a.T + BM - 1) / BM;
  int64_t mt;
  int nt;
  xcd_tile(ncol, mt, nt);
  const int64_t b = mt / tps;
  const int t0 = int(mt % tps) * BM;
  const int64_t m0 = b * a.T + t0;
  const int mrows = a.T - t0 < BM ? a.T - t0 : BM;
  const int n0 = nt * BN;
  const int nchunk = a.C / WS_CK;

  // this wave's DMA pieces q = 8u + wave (past the last piece: the last one again)
  const __bf16* src[PW];
#pragma unroll
  for (int u = 0; u < PW; ++u) {
    const int q = u * 8 + wave < TI ? u * 8 + wave : TI - 1;
    if (q < XI) {
      const int R = q * WS_RPI + lane / WS_SPR, ls = (lane % WS_SPR) ^ ws_swzbits(R);
      int ti = t0 - a.pad + R;
      const bool valid =
          R < span && (a.seq_pitch > 0 ? ti >= 0 && ti < a.T && ti % a.seq_pitch < a.tin_valid
                                       : (ti >= 0 && ti < a.tin_valid) || a.pad_mode == SEL_PAD_REPLICATE);
      if (a.seq_pitch == 0) ti = ti < 0 ? 0 : (ti >= a.tin_valid ? a.tin_valid - 1 : ti);
      src[u] = valid ? in + (b * a.tin_pitch + ti) * a.ldx + 8 * ls : g_ws_zero + 8 * ls;
    } else {
      const int R = (q - XI) * WS_RPI + lane / WS_SPR, ls = (lane % WS_SPR) ^ ws_swzbits(R);
      const int k = R / BN, n = R % BN;
      src[u] = wp + (int64_t(n0 + n) * KT + k) * a.C + 8 * ls;
    }
  }
  auto issue = [&](int ch) __attribute__((always_inline)) {
    unsigned char* const base = smem + (ch % NB) * (BUF * 2);
#pragma unroll
    for (int u = 0; u < PW; ++u) {
      const int q = u * 8 + wave < TI ? u * 8 + wave : TI - 1;
      const int off = q < XI ? q * 1024 : XROWS * WS_CK * 2 + (q - XI) * 1024;
      __builtin_amdgcn_global_load_lds((const void*)(src[u] + ch * WS_CK), (lds_ptr_t)(base + off), 16, 0, 0);
    }
  };
  const int xi_used = (span + WS_RPI - 1) / WS_RPI;  // input pieces holding rows < span
  auto elu_pass = [&](int ch) __attribute__((always_inline)) {
    ws8_elu_pieces<PW>(smem + (ch % NB) * (BUF * 2), lane, wave, xi_used);
  };

  const int wm = wave / G::WN, wn = wave % G::WN;
  const int hl = lane >> 5;
  int arow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) arow[i] = wm * G::WTM + i * 32 + (lane & 31);
  int boff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) boff[j] = XROWS * WS_CK + ws_swz(wn * 64 + j * 32 + (lane & 31), hl);
  floatx16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // prologue: chunks 0 and 1 in flight, chunk 0 landed (and ELU'd) before the first barrier
  constexpr int D = NB - 1;
  for (int c = 0; c < D && c < nchunk; ++c) issue(c);
  if (nchunk > 1) ws_wait_vm<PW>();
  else ws_wait_vm<0>();
  if (a.in_elu) elu_pass(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int ch = 0; ch < nchunk; ++ch) {
    // chunk ch - 1's slot is free (every wave passed the barrier after reading it)
    if (ch + D < nchunk && !(dbg & 1)) issue(ch + D);
    const __bf16* const xb = lds + (ch % NB) * BUF;
    bf16x8 fa[2][TM], fb[2][2];
    auto fetch = [&](int k, int q) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[q][j] = *reinterpret_cast<const bf16x8*>(xb + boff[j] + k * BN * WS_CK);
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[q][i] = *reinterpret_cast<const bf16x8*>(xb + ws_swz(arow[i] + k * a.dil, hl));
    };
    fetch(0, 0);
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k + 1 < KT) fetch(k + 1, (k + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
      if (!(dbg & 2)) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[k & 1][j], fa[k & 1][i], acc[i][j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (k == 0 && ch + 1 < nchunk) {
        // chunk ch + 1 landed (chunk ch + 2, when issued above, still in flight), then its ELU
        if (ch + D < nchunk && !(dbg & 1)) ws_wait_vm<PW>();
        else ws_wait_vm<0>();
        if (a.in_elu) elu_pass(ch + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!(dbg & 4)) __builtin_amdgcn_s_barrier();
  }
  if (dbg & 8) return;

  // epilogue in BM / PR passes of PR rows: the waves whose rows fall in pass p
  // write their accumulators into an fp32 [PR][BN + 4] tile over the (drained)
  // ring, then all 8 waves run row-contiguous 16-B accesses (the 12-wave
  // kernel's epilogue)
  struct alignas(16) V8 { TO v[8]; };
  constexpr int PR = G::PR, BNV = BN / 8, EV = PR * BNV / 512, NP = BM / PR;
  float* const tile = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (wm * G::WTM / PR == p) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * G::WTM % PR + i * 32 + (lane & 31);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            floatx4 v4;
#pragma unroll
            for (int e = 0; e < 4; ++e) v4[e] = acc[i][j][4 * g + e];
            *reinterpret_cast<floatx4*>(tile + r * G::EP + wn * 64 + j * 32 + 8 * g + 4 * hl) = v4;
          }
      }
    }
    __syncthreads();
    const int prow = p * PR;
#pragma unroll
    for (int u = 0; u < EV; ++u) {
      const int v = tid + u * 512;
      const int row = v / BNV, c8 = (v % BNV) * 8;
      if (prow + row >= mrows) continue;
      const int64_t o = (m0 + prow + row) * a.ldo + n0 + c8;
      V8 av, rv;
      if (aux) av = *reinterpret_cast<const V8*>(aux + o);
      if (res) rv = *reinterpret_cast<const V8*>(res + o);
      const floatx4 lo = *reinterpret_cast<const floatx4*>(tile + row * G::EP + c8);
      const floatx4 hi = *reinterpret_cast<const floatx4*>(tile + row * G::EP + c8 + 4);
      float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (a.epi) {
        const bool valid = (a.seq_pitch > 0 ? (t0 + prow + row) % a.seq_pitch : t0 + prow + row) < a.tout_valid;
        float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (bias) {
          const floatx4 b0 = *reinterpret_cast<const floatx4*>(bias + n0 + c8);
          const floatx4 b1 = *reinterpret_cast<const floatx4*>(bias + n0 + c8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[e] = b0[e], bv[e + 4] = b1[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float y = 0.f;
          if (valid) {
            y = x[e];
            if (bias) y += bv[e];
            if (res) y += to_f(rv.v[e]);
            if (aux) y *= to_f(av.v[e]) > 0.f ? 1.f : a.slope;
            if (a.act) y = y > 0.f ? y : y * a.slope;
          }
          x[e] = y;
        }
      } else {
        if (bias && a.bias_period) {
          if (a.bias_period % 8 == 0) {
            const float* const bp = bias + (n0 + c8) % a.bias_period;
            const floatx4 b0 = *reinterpret_cast<const floatx4*>(bp), b1 = *reinterpret_cast<const floatx4*>(bp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] += b0[e], x[e + 4] += b1[e];
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] += bias[(n0 + c8 + e) % a.bias_period];
          }
        }
        if (aux) {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] *= elu_grad_fast(to_f(av.v[e]));
        }
        if (res) {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] += to_f(rv.v[e]);
        }
      }
      V8 ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) ov.v[e] = from_f<TO>(x[e]);
      *reinterpret_cast<V8*>(out + o) = ov;
    }
    if (p + 1 < NP) __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Weight-stationary streaming conv for the thin layers (32/64/96 input and
// 32/64 output channels: the residual-unit convs at T = 24000 / 8000, their
// dgrads, the first strided layer and the last transposed layer's dgrad).
// These are HBM-bound, yet the tiled kernel above re-stages every tap of the
// weight slice for each 128-row tile (for a 64x64 k7 layer, 3x the tile's
// activation bytes through L2 and LDS), and its neighbouring tiles land on
// different XCDs, so the causal halo is re-fetched from HBM (rocprofv3 PMC:
// 1.85x the algorithmic read bytes at 32 channels, profiles/r1_c3_pmc_traffic.md).
// Here each wave keeps the MFMA A-fragments of its 32-channel output slice
// for ALL taps and input channels in VGPRs (K*C/16 fragments, loaded once
// per block), and the block streams a CONTIGUOUS range of sample-aligned
// R-row tiles (the halo re-read hits the block's own XCD L2):
//   stage rows + causal halo (ELU applied, padding resolved) in LDS
//   -> K*C/16*TM MFMAs per wave while the next tile's rows are in flight
//   -> accumulators -> LDS (fp32) -> one fully coalesced 16-B epilogue pass
//      (bias, ELU'(aux), residual) over the tile's contiguous output rows.
// ---------------------------------------------------------------------------
template <int C, int N, int K, int R, bool E>
__global__ __launch_bounds__(256) void k_conv_thin_bf16(Args a, const __bf16* __restrict__ in,
                                                        const __bf16* __restrict__ wp,
                                                        const float* __restrict__ bias,
                                                        const __bf16* __restrict__ aux,
                                                        const __bf16* __restrict__ res, __bf16* __restrict__ out,
                                                        int tiles_per_block, int epi_pf) {
  using G = Thin<C, N, K, R, E>;
  constexpr int P = F4_P;
  constexpr int CV = G::CV;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);  // [PLANES][SPAN][P]
  // [R][OP] fp32 out tile: aliases xs, or follows it when the tile loop is split
  float* const ot = reinterpret_cast<float*>(smem + (G::SPLIT ? G::LDS_STAGE : 0));
  const bool split = G::SPLIT && (epi_pf & 2);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ns = wave % G::NS, rg = wave / G::NS;
  const int span = R + (K - 1) * a.dil;
  const int tps = (a.T + R - 1) / R;
  const int64_t ntiles = (a.rows / a.T) * tps;
  // XCD-contiguous tile ranges: the grid is a multiple of 8 and block b runs on
  // XCD b % 8, so virtual block (b % 8) * (grid / 8) + b / 8 gives each XCD one
  // contiguous run of tiles, walked in dispatch order -> a tile's causal halo
  // was just fetched into the same L2 by its predecessor
  const int64_t vb = int64_t(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
  const int64_t tile0 = vb * tiles_per_block;
  const int64_t tile_end = tile0 + tiles_per_block < ntiles ? tile0 + tiles_per_block : ntiles;
  if (tile0 >= tile_end) return;  // block-uniform

  // A fragments of output slice ns: wf[k][g] = Wp[n][k][16g + 8*(lane>>5) .. +8]
  bf16x8 wf[K][C / 16];
  {
    const __bf16* wrow = wp + int64_t(ns * 32 + (lane & 31)) * K * C + 8 * (lane >> 5);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int g = 0; g < C / 16; ++g) wf[k][g] = *reinterpret_cast<const bf16x8*>(wrow + k * C + 16 * g);
  }
  ws_wait_vm<0>();  // weights landed: the tile loop's MFMAs then wait on no request of the loop

  uint4 xr[G::XV];
  bool xok[G::XV];
  // branch-free buffer loads (Ru32Stage::load): rows past the span, zero-padded
  // rows and a dead request (live = false) read nothing and return zeros
  auto load = [&](int64_t tile, bool live) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const __amdgpu_buffer_rsrc_t rs = ru_rsrc(in + b * a.T * C, int64_t(a.T) * C);
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      int ti = t0 - a.pad + r;
      const bool inside = ti >= 0 && ti < a.T;
      xok[u] = r < span && (inside || a.pad_mode == SEL_PAD_REPLICATE);
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      xr[u] = ru_bload(rs, live && xok[u] ? (ti * C + c) * 2 : RU_OOB);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      if (r >= span) continue;
      uint4 val = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
      if (a.in_elu) {
        val = elu8(val);
      }
      *reinterpret_cast<uint4*>(xs + ((c >> 5) * G::SPAN + r) * P + (c & 31)) = val;
    }
  };

  // the bias over this kernel's N output channels in LDS (bs[n] = bias[n % period]):
  // a global bias load in the epilogue would wait behind the next tile's request
  __shared__ __align__(16) float bs[N];
  const bool has_bias = bias && a.bias_period;
  if (has_bias && tid < N) bs[tid] = bias[tid % a.bias_period];
  load(tile0, true);
  if (split) {
    store();
    __syncthreads();
    if (tile0 + 1 < tile_end) load(tile0 + 1, true);
  }
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    if (!split) {
      __syncthreads();  // the previous tile's epilogue is done with ot (= xs)
      store();
      __syncthreads();
      load(tile + 1 < tile_end ? tile + 1 : tile, tile + 1 < tile_end);  // unconditional: exact counts
    }

    // this tile's epilogue operands (ELU'(aux), residual), fetched before the
    // MFMA phase so their HBM latency hides behind it instead of stalling the
    // epilogue (N <= 64: <= 8 16-B vectors per lane per operand)
    const int64_t eb = tile / tps;
    const int et0 = int(tile % tps) * R;
    const int emrows = a.T - et0 < R ? a.T - et0 : R;
    const int64_t eobase = (eb * a.T + et0) * N;
    uint4 apf[G::EPF ? G::EJ : 1], rpf[G::EPF ? G::EJ : 1];
    if constexpr (G::EPF) {
      if (epi_pf & 1) {
#pragma unroll
        for (int j = 0; j < G::EJ; ++j) {
          const int idx = tid + j * 256, r = idx / (N / 8), n = (idx % (N / 8)) * 8;
          const int64_t o = eobase + int64_t(r) * N + n;
          if (aux && r < emrows) apf[j] = *reinterpret_cast<const uint4*>(aux + o);
          if (res && r < emrows) rpf[j] = *reinterpret_cast<const uint4*>(res + o);
        }
      }
    }

    const bool mma_wave = G::NS * G::RG == 4 || rg < G::RG;  // wave-uniform
    floatx16 acc[G::TM];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const __bf16* xw = xs + ((mma_wave ? rg : 0) * G::WR + (lane & 31)) * P + 8 * (lane >> 5);
    if (mma_wave) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int g = 0; g < C / 16; ++g) {
          const __bf16* xb = xw + ((g >> 1) * G::SPAN + k * a.dil) * P + 16 * (g & 1);
#pragma unroll
          for (int i = 0; i < G::TM; ++i) {
            const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xb + i * 32 * P);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][g], xf, acc[i], 0, 0, 0);
          }
        }
      }
    }

    // accumulators (out^T: lane -> row, element r -> channel) -> fp32 tile in LDS
    __syncthreads();  // every wave is done reading xs (split: and the last epilogue with ot)
    if (mma_wave) {
#pragma unroll
      for (int i = 0; i < G::TM; ++i) {
        const int row = rg * G::WR + i * 32 + (lane & 31);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = ns * 32 + 8 * g + 4 * (lane >> 5);
          *reinterpret_cast<floatx4*>(ot + row * G::OP + n) =
              floatx4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
        }
      }
    }
    // split loop: the next tile is staged beside this tile's out tile, so a
    // tile costs two barriers and its epilogue overlaps the next MFMA phase
    if (split && tile + 1 < tile_end) store();
    __syncthreads();
    if (split && tile + 2 < tile_end) load(tile + 2, true);

    // coalesced epilogue: a sample-aligned tile's output rows are contiguous in HBM
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    const int64_t obase = (b * a.T + t0) * N;
    constexpr int GN = N / 8;
    auto epilogue = [&](int idx, const uint4* apv, const uint4* rpv) {
      const int r = idx / GN, n = (idx % GN) * 8;
      const floatx4 lo = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n);
      const floatx4 hi = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (has_bias) {
        const floatx4 b0 = *reinterpret_cast<const floatx4*>(bs + n);
        const floatx4 b1 = *reinterpret_cast<const floatx4*>(bs + n + 4);
        v[0] += b0[0], v[1] += b0[1], v[2] += b0[2], v[3] += b0[3];
        v[4] += b1[0], v[5] += b1[1], v[6] += b1[2], v[7] += b1[3];
      }
      const int64_t o = obase + int64_t(r) * N + n;
      // explicit roundings (no FMA contraction): every instance, and the fused
      // residual-unit kernels, produce the same bits
      if (aux) {
        uint4 raw = apv ? *apv : *reinterpret_cast<const uint4*>(aux + o);
        const __bf16* av = reinterpret_cast<const __bf16*>(&raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __fmul_rn(v[e], elu_grad_fast(float(av[e])));
      }
      if (res) {
        uint4 raw = rpv ? *rpv : *reinterpret_cast<const uint4*>(res + o);
        const __bf16* rv = reinterpret_cast<const __bf16*>(&raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __fadd_rn(v[e], float(rv[e]));
      }
      uint4 ov;
      __bf16* op = reinterpret_cast<__bf16*>(&ov);
#pragma unroll
      for (int e = 0; e < 8; ++e) op[e] = __bf16(v[e]);
      *reinterpret_cast<uint4*>(out + o) = ov;
    };
    if (G::EPF && (epi_pf & 1)) {
#pragma unroll
      for (int j = 0; j < (G::EPF ? G::EJ : 1); ++j)
        if (tid + j * 256 < mrows * GN) epilogue(tid + j * 256, &apf[j], &rpf[j]);
    } else {
      for (int idx = tid; idx < mrows * GN; idx += 256) epilogue(idx, nullptr, nullptr);
    }
  }
}

// ---------------------------------------------------------------------------
// Pointwise (1x1) conv for the 256-wide residual units at T = 400
// (residual_unit.py:43-46's conv2 forward, out = x + W ELU(h), and its dgrad,
// gh = ELU'(h) * W^T g).  The tiled kernel ran them as 8 dependent
// 32-channel chunk steps per 64 x 128 tile (one global-load latency per
// step): 19 us per launch for 39 MB, 2 TB/s.  Here one workgroup per CU owns
// a contiguous range of rows:
//   - N/32 waves; wave w holds the MFMA fragments of output columns
//     [32w, 32w + 32) for all C input channels in VGPRs;
//   - a pass over up to SUB 32-row sub-tiles requests everything up front,
//     in use order: sub-tile 0's rows and epilogue operands, the weights,
//     then the later sub-tiles (all row-contiguous 16-B pieces);
//   - per sub-tile: wait for its own rows only, ELU them into its LDS slice,
//     barrier, C/16 MFMAs per wave with every fragment read ahead,
//     accumulators -> fp32 LDS tile, barrier, and a row-contiguous epilogue
//     (bias, ELU'(aux), residual; 16-B stores), overlapping the arrival of
//     the later sub-tiles;
//   - every access is a buffer access over the block's own row range, so rows
//     past it read zeros and their stores are dropped (no tail masking).
// Same MFMA (32x32x16, weights as the first operand), same channel order and
// the same epilogue roundings as k_conv_fwd_bf16: bit-identical outputs for
// one epilogue operand (the residual-unit forms).
// ---------------------------------------------------------------------------
template <int C, int N>
struct Pw {
  static constexpr int WAVES = N / 32;
  static constexpr int THREADS = WAVES * 64;
  static constexpr int R = 32;                       // rows per sub-tile (one 32x32 MFMA tile)
  static constexpr int SUB = 4;                      // sub-tiles per pass
  static constexpr int RB = R * SUB;                 // rows per pass
  static constexpr int PITCH = C + 8;                // LDS row pitch (bf16): conflict-free b128 reads
  static constexpr int OP = N + 4;                   // fp32 out-tile pitch
  static constexpr int XV = R * (C / 8) / THREADS;   // 16-B input pieces per thread per sub-tile
  static constexpr int EV = R * (N / 8) / THREADS;   // 16-B output pieces per thread per sub-tile
  static constexpr size_t LDS_X = size_t(RB) * PITCH * 2;
  static constexpr size_t LDS = LDS_X + size_t(R) * OP * 4;
  static_assert(XV >= 1 && R * (C / 8) % THREADS == 0 && EV >= 1 && R * (N / 8) % THREADS == 0, "pw pieces");
};

#ifndef SEL_W_PW
#define SEL_W_PW 2
#endif
// timing ablations (diagnostic builds only, tools/pw_abl.sh): 1 no weight
// loads, 2 no MFMAs, 4 no epilogue operand loads, 8 no output stores
#ifndef SEL_PW_ABL
#define SEL_PW_ABL 0
#endif

template <int C, int N, bool ELU, bool AUX, bool RES>
__global__ __launch_bounds__((N / 32) * 64) __attribute__((amdgpu_waves_per_eu(SEL_W_PW))) void k_pw_bf16(
    Args a, const __bf16* __restrict__ in, const __bf16* __restrict__ wp, const float* __restrict__ bias,
    const __bf16* __restrict__ aux, const __bf16* __restrict__ res, __bf16* __restrict__ out, int rows_per_block) {
  using G = Pw<C, N>;
  constexpr int R = G::R, SUB = G::SUB, PITCH = G::PITCH, OP = G::OP, T = G::THREADS;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);             // [RB][PITCH]
  float* const ot = reinterpret_cast<float*>(smem + G::LDS_X);    // [R][OP]
  __shared__ __align__(16) float bs[N];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = int64_t(blockIdx.x) * rows_per_block;
  if (r0 >= a.rows) return;  // block-uniform
  const int nrows = int(a.rows - r0 < rows_per_block ? a.rows - r0 : rows_per_block);

  const __amdgpu_buffer_rsrc_t rin = ru_rsrc(in + r0 * C, int64_t(nrows) * C);
  const __amdgpu_buffer_rsrc_t rout = ru_rsrc(out + r0 * N, int64_t(nrows) * N);
  const __amdgpu_buffer_rsrc_t raux = ru_rsrc(AUX ? aux + r0 * N : out, AUX ? int64_t(nrows) * N : 0);
  const __amdgpu_buffer_rsrc_t rres = ru_rsrc(RES ? res + r0 * N : out, RES ? int64_t(nrows) * N : 0);

  // the bias over the N columns (bs[n] = bias[n % period]) goes to LDS after
  // the first sub-tile's requests; its value is requested here
  const bool has_bias = bias && a.bias_period;
  const float bval = has_bias && tid < N ? bias[tid % a.bias_period] : 0.f;

  // input piece u of a sub-tile: row v / (C/8), channels (v % (C/8)) * 8;
  // output piece j: row v / (N/8), channels (v % (N/8)) * 8 (v = tid + u*T)
  uint4 xr[SUB][G::XV], ar[SUB][G::EV], rr[SUB][G::EV];
  auto request = [&](int p0, int s) {
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * T;
      xr[s][u] = ru_bload(rin, ((p0 + s * R + v / (C / 8)) * C + (v % (C / 8)) * 8) * 2);
    }
#pragma unroll
    for (int j = 0; j < G::EV; ++j) {
      const int v = tid + j * T;
      const int off = ((p0 + s * R + v / (N / 8)) * N + (v % (N / 8)) * 8) * 2;
      if constexpr (SEL_PW_ABL & 4) {
        ar[s][j] = make_uint4(off, 7u, 9u, 11u);
        rr[s][j] = make_uint4(off ^ 5, 3u, 1u, 13u);
      } else {
        if constexpr (AUX) ar[s][j] = ru_bload(raux, off);
        if constexpr (RES) rr[s][j] = ru_bload(rres, off);
      }
    }
  };
  // weight fragments of this wave's 32 output columns: wf[g] = Wp[n][16g + 8*(lane>>5) .. +8]
  bf16x8 wf[C / 16];
  const __bf16* const wrow = wp + int64_t(wave * 32 + (lane & 31)) * C + 8 * (lane >> 5);

  for (int p0 = 0; p0 < nrows; p0 += G::RB) {
    if (p0) __syncthreads();  // the previous pass is done with xs / ot
    request(p0, 0);
#pragma unroll
    for (int g = 0; g < C / 16; ++g) {
      if constexpr (SEL_PW_ABL & 1) wf[g] = __builtin_bit_cast(bf16x8, make_uint4(lane * 7u + g, g, lane, 3u));
      else wf[g] = *reinterpret_cast<const bf16x8*>(wrow + 16 * g);
    }
#pragma unroll
    for (int s = 1; s < SUB; ++s) request(p0, s);
    if (tid < N) bs[tid] = bval;  // visible after the first sub-tile's barrier

#pragma unroll
    for (int s = 0; s < SUB; ++s) {
      if (p0 + s * R >= nrows) break;  // block-uniform
      // sub-tile s's rows -> its own LDS slice
#pragma unroll
      for (int u = 0; u < G::XV; ++u) {
        const int v = tid + u * T;
        const uint4 val = ELU ? elu8(xr[s][u]) : xr[s][u];
        *reinterpret_cast<uint4*>(xs + (s * R + v / (C / 8)) * PITCH + (v % (C / 8)) * 8) = val;
      }
      __syncthreads();
      // every fragment of the sub-tile requested before the first MFMA
      const __bf16* xb = xs + (s * R + (lane & 31)) * PITCH + 8 * (lane >> 5);
      bf16x8 xf[C / 16];
#pragma unroll
      for (int g = 0; g < C / 16; ++g) xf[g] = *reinterpret_cast<const bf16x8*>(xb + 16 * g);
      __builtin_amdgcn_sched_barrier(0);
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      if constexpr (SEL_PW_ABL & 2) {
#pragma unroll
        for (int g = 0; g < C / 16; ++g) acc[g] = float(xf[g][0]) + float(wf[g][1]);
      } else {
#pragma unroll
        for (int g = 0; g < C / 16; ++g) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[g], xf[g], acc, 0, 0, 0);
      }
      // accumulators (out^T: lane -> row, element 4q + e -> channel 32w + 8q + 4*(lane>>5) + e)
      // -> fp32 tile; the previous sub-tile's epilogue reads ended before this
      // sub-tile's barrier
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<floatx4*>(ot + (lane & 31) * OP + wave * 32 + 8 * q + 4 * (lane >> 5)) =
            floatx4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
      __syncthreads();
#pragma unroll
      for (int j = 0; j < G::EV; ++j) {
        const int v = tid + j * T, r = v / (N / 8), n = (v % (N / 8)) * 8;
        const floatx4 lo = *reinterpret_cast<const floatx4*>(ot + r * OP + n);
        const floatx4 hi = *reinterpret_cast<const floatx4*>(ot + r * OP + n + 4);
        float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if (has_bias) {
          const floatx4 b0 = *reinterpret_cast<const floatx4*>(bs + n);
          const floatx4 b1 = *reinterpret_cast<const floatx4*>(bs + n + 4);
          x[0] += b0[0], x[1] += b0[1], x[2] += b0[2], x[3] += b0[3];
          x[4] += b1[0], x[5] += b1[1], x[6] += b1[2], x[7] += b1[3];
        }
        if constexpr (AUX) {
          const __bf16* av = reinterpret_cast<const __bf16*>(&ar[s][j]);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = __fmul_rn(x[e], elu_grad_fast(float(av[e])));
        }
        if constexpr (RES) {
          const __bf16* rv = reinterpret_cast<const __bf16*>(&rr[s][j]);
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = __fadd_rn(x[e], float(rv[e]));
        }
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = __bf16(x[e]);
        if (!(SEL_PW_ABL & 8) || x[0] == 1234.5f)
          ru_bstore(rout, ((p0 + s * R + r) * N + n) * 2, o);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Single-input-channel layers (the encoder's first conv 1->32 k7, and the dgrad
// of the decoder's last conv 32->1 k7): an implicit GEMM with a reduction of
// only K taps would leave MFMA idle and stage a 1-wide tile, so this is a
// streaming kernel instead: one output row per thread, K input samples, N x K
// FMAs against LDS-broadcast weights, 16-B vector stores of the N outputs.
// ---------------------------------------------------------------------------
// rows per tile of the forward kernel: 768 (round 6; was 1024).  One resident
// round is 1024 workgroups at C3: 64 x 24000 rows in 1024-row tiles are 1536
// tiles, so half the workgroups ran two and the launch took two tile times;
// 768-row tiles are 2048 tiles, two per workgroup, 1.5 (1024-row) tile times
constexpr int C1F_TR = 768;

// (c1_act_grad as c1_act: exact for TI = float, the hardware exp for bf16)
template <typename TI>
__device__ __forceinline__ float c1_act_grad(float v) {
  if constexpr (sizeof(TI) == 4) return elu_grad(v);
  else return elu_grad_fast(v);
}
// Thread = (8-wide output group g, row lane rl): its 8 x K weights live in
// registers; per row it reads K staged samples and writes one 16-B vector, the
// NG lanes of a row together writing the row's contiguous N outputs.
template <typename TI, typename TO, int TR>
__global__ __launch_bounds__(256) void k_conv_c1(Args a, const TI* __restrict__ in,
                                                 const TI* __restrict__ wp, const float* __restrict__ bias,
                                                 const TO* __restrict__ aux, const TO* __restrict__ res,
                                                 TO* __restrict__ out) {
  __shared__ float xs[TR + C1_HALO];
  constexpr int PV = (TR + C1_HALO + 255) / 256;  // staged samples per thread
  constexpr int V = Vec16<TO>::n;  // outputs per vector store (8 bf16 / 4 fp32)
  const int NG = a.N / V;
  const int tid = threadIdx.x, grp = tid % NG, rl = tid / NG, nrl = 256 / NG;
  float w[V][C1_KMAX], bs[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int n = grp * V + e;
    bs[e] = (bias && a.bias_period) ? bias[n % a.bias_period] : 0.f;
#pragma unroll
    for (int k = 0; k < C1_KMAX; ++k) w[e][k] = k < a.K ? to_f(wp[n * a.K + k]) : 0.f;
  }
  const int tps = (a.T + TR - 1) / TR;
  const int64_t ntiles = (a.rows / a.T) * tps;
  // the next tile's samples are fetched into registers while this tile is
  // computed and stored (one resident round of workgroups walks the tiles)
  const int span = TR + (a.K - 1) * a.dil;
  float pre[PV];
  auto fetch = [&](int64_t tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * TR;
#pragma unroll
    for (int u = 0; u < PV; ++u) {
      const int r = threadIdx.x + 256 * u;
      int ti = t0 - a.pad + r;
      const bool ok = r < span && ((ti >= 0 && ti < a.T) || a.pad_mode == SEL_PAD_REPLICATE);
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      const float v = ok ? to_f(in[b * a.T + ti]) : 0.f;
      pre[u] = ok && a.in_elu ? c1_act<TI>(v) : v;
    }
  };
  if (int64_t(blockIdx.x) < ntiles) fetch(blockIdx.x);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * TR;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PV; ++u)
      if (threadIdx.x + 256 * u < span) xs[threadIdx.x + 256 * u] = pre[u];
    __syncthreads();
    if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x);
    const int rows = a.T - t0 < TR ? a.T - t0 : TR;
    for (int r = rl; r < rows; r += nrl) {
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = bs[e];
#pragma unroll
      for (int k = 0; k < C1_KMAX; ++k) {
        if (k >= a.K) break;
        const float x = xs[r + k * a.dil];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = fmaf(w[e][k], x, v[e]);
      }
      const int64_t o = (b * a.T + t0 + r) * a.N + grp * V;
      if (aux) {
        TO av[V];
        *reinterpret_cast<uint4*>(av) = *reinterpret_cast<const uint4*>(aux + o);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] *= c1_act_grad<TI>(to_f(av[e]));
      }
      if (res) {
        TO rv[V];
        *reinterpret_cast<uint4*>(rv) = *reinterpret_cast<const uint4*>(res + o);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] += to_f(rv[e]);
      }
      TO ov[V];
#pragma unroll
      for (int e = 0; e < V; ++e) ov[e] = from_f<TO>(v[e]);
      *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<uint4*>(ov);
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

namespace sel {
namespace conv {

int check_desc(const sel_conv_desc* d) {
  SEL_REQUIRE(d != nullptr, SEL_ERR_ARG, "null conv descriptor");
  SEL_REQUIRE(d->rows >= 0 && d->T > 0 && d->rows % d->T == 0, SEL_ERR_ARG,
              "rows (%lld) must be a multiple of T (%d)", (long long)d->rows, d->T);
  SEL_REQUIRE(d->C > 0 && d->N > 0 && d->K > 0 && d->dil > 0 && d->pad >= 0, SEL_ERR_ARG,
              "bad conv shape C=%d N=%d K=%d dil=%d pad=%d", d->C, d->N, d->K, d->dil, d->pad);
  SEL_REQUIRE(d->pad_mode == SEL_PAD_ZERO || (d->pad_mode == SEL_PAD_REPLICATE && d->pad <= (d->K - 1) * d->dil),
              SEL_ERR_ARG, "bad pad mode");
  SEL_REQUIRE(d->bias_period >= 0 && (d->bias_period == 0 || d->N % d->bias_period == 0), SEL_ERR_ARG,
              "bias_period must divide N");
  SEL_REQUIRE((d->K - 1) * d->dil <= 512, SEL_ERR_UNSUPPORTED, "receptive halo > 512 rows");
  return SEL_OK;
}

Args to_args(const sel_conv_desc* d) {
  Args a;
  a.rows = d->rows;
  a.T = d->T;
  a.C = d->C;
  a.N = d->N;
  a.K = d->K;
  a.dil = d->dil;
  a.pad = d->pad;
  a.pad_mode = d->pad_mode;
  a.in_elu = d->in_elu;
  a.bias_period = d->bias_period;
  a.tin_valid = a.tin_pitch = a.tout_valid = d->T;
  a.ldx = d->C;
  a.ldo = d->N;
  a.epi = a.act = 0;
  a.slope = 0.f;
  a.seq_pitch = 0;
  return a;
}

}  // namespace conv
}  // namespace sel

namespace {

template <typename TI, typename TO, int BM, int BN>
size_t fwd_lds(const Args& a) {
  const size_t stage = (size_t(BM + (a.K - 1) * a.dil) + size_t(a.K) * BN) * Pitch<TI>::v * sizeof(TI);
  const size_t epi = size_t(BM) * (BN + 4) * sizeof(float);
  return stage > epi ? stage : epi;
}

template <typename TI, typename TO, int BM, int BN>
int launch_fwd(const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
               const void* res, void* out, hipStream_t s) {
  const size_t lds = fwd_lds<TI, TO, BM, BN>(a);
  SEL_REQUIRE(lds <= 160 * 1024, SEL_ERR_UNSUPPORTED, "conv tile needs %zu B of LDS", lds);
  dim3 grid(unsigned((a.rows + BM - 1) / BM), unsigned((a.N + BN - 1) / BN));
  if (grid.x == 0) return SEL_OK;
  auto kern = k_conv_fwd<TI, TO, BM, BN>;
  if (lds > 64 * 1024)
    SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, static_cast<const TI*>(in),
                     static_cast<const TI*>(wp), bias, static_cast<const TO*>(aux),
                     static_cast<const TO*>(res), static_cast<TO*>(out));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int BM, int BN>
int launch_fwd_f32(const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
                   const void* res, void* out, hipStream_t s) {
  const size_t stage = (size_t(BM + FF_HALO) + size_t(a.K) * BN) * FF_P * sizeof(float);
  const size_t epi = size_t(BM) * (BN + 4) * sizeof(float);
  const size_t lds = stage > epi ? stage : epi;
  const int64_t tiles = (a.rows / a.T) * ((a.T + BM - 1) / BM);  // sample-aligned tiles
  if (tiles == 0) return SEL_OK;
  dim3 grid(unsigned(tiles), unsigned(a.N / BN));
  auto kern = a.K == 1 ? k_conv_fwd_f32<1, BM, BN> : a.K <= 3 ? k_conv_fwd_f32<3, BM, BN> : k_conv_fwd_f32<8, BM, BN>;
  if (lds > 64 * 1024)
    SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, static_cast<const float*>(in), static_cast<const float*>(wp),
                     bias, static_cast<const float*>(aux), static_cast<const float*>(res), static_cast<float*>(out));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int BM, int BN, int WAVES_M, int KMAX, typename TO>
int launch_fwd4(const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
                const void* res, void* out, hipStream_t s) {
  const int span = BM + (a.K - 1) * a.dil;
  const size_t lds = (size_t(span) + size_t(a.K) * BN) * F4_P * 2;
  const int64_t tiles = (a.rows / a.T) * ((a.T + BM - 1) / BM);  // sample-aligned tiles
  const int ncol = (a.N + BN - 1) / BN;
  if (tiles == 0) return SEL_OK;
  // tune key 8 = 1: plain 2-D grid instead of the XCD-aware 1-D order
  const bool xcd = ncol > 1 && tune(8) == 0 && tiles * ncol < (int64_t(1) << 31);
  const dim3 grid = xcd ? dim3(unsigned(tiles * ncol)) : dim3(unsigned(tiles), unsigned(ncol));
  auto kern = k_conv_fwd_bf16<BM, BN, WAVES_M, KMAX, TO>;
  if (lds > 64 * 1024)
    SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a, static_cast<const __bf16*>(in),
                     static_cast<const __bf16*>(wp), bias, static_cast<const TO*>(aux), static_cast<const TO*>(res),
                     static_cast<TO*>(out), xcd ? ncol : 0);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// (measured and dropped in round 2: four consumer waves of 128 x 64, two
// chunks per barrier for the two-tap layers)
template <int KT, typename TO>
int launch_ws(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
              void* out, hipStream_t s) {
  const size_t lds = ws_lds_bytes(KT, 1);
  const int64_t tiles = (a.rows / a.T) * ((a.T + WS_BM - 1) / WS_BM);
  const int ncol = a.N / WS_BN;
  if (tiles == 0) return SEL_OK;
  const bool xcd = ncol > 1 && tune(8) == 0 && tiles * ncol < (int64_t(1) << 31);
  const dim3 grid = xcd ? dim3(unsigned(tiles * ncol)) : dim3(unsigned(tiles), unsigned(ncol));
  auto kern = k_conv_ws_bf16<KT, TO, 8, 1>;
  SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL(kern, grid, dim3(768), lds, s, a, static_cast<const __bf16*>(in),
                     static_cast<const __bf16*>(wp), bias, static_cast<const TO*>(aux), static_cast<const TO*>(res),
                     static_cast<TO*>(out), xcd ? ncol : 0, tune(13));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int KT, typename TO, int BM, int BN, int HALO, int TM = 4>
int launch_ws8(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
               void* out, hipStream_t s) {
  using G = Ws8<KT, BM, BN, HALO, TM>;
  SEL_REQUIRE(a.K == KT && a.N % BN == 0 && a.C % WS_CK == 0 && a.C <= WS_CMAX && (KT - 1) * a.dil <= HALO &&
                  a.T > 0 && a.rows % a.T == 0,
              SEL_ERR_ARG, "k_conv_ws8<%d, %d, %d>: bad shape C=%d N=%d K=%d dil=%d", KT, BM, BN, a.C, a.N, a.K,
              a.dil);
  const int64_t tiles = (a.rows / a.T) * ((a.T + BM - 1) / BM);
  const int ncol = a.N / BN;
  if (tiles == 0) return SEL_OK;
  const bool xcd = ncol > 1 && tune(8) == 0 && tiles * ncol < (int64_t(1) << 31);
  const dim3 grid = xcd ? dim3(unsigned(tiles * ncol)) : dim3(unsigned(tiles), unsigned(ncol));
  auto kern = k_conv_ws8<KT, TO, BM, BN, HALO, TM>;
  SEL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(G::LDS)));
  hipLaunchKernelGGL(kern, grid, dim3(512), G::LDS, s, a, static_cast<const __bf16*>(in),
                     static_cast<const __bf16*>(wp), bias, static_cast<const TO*>(aux), static_cast<const TO*>(res),
                     static_cast<TO*>(out), xcd ? ncol : 0, tune(13));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// the eight-wave kernel's 512 x 128 tiles for the 128-wide k7 layers (legal
// shapes; forced with tune key 0 = 28)
bool ws8_gen_ok(const Args& a) {
  return a.K == 7 && a.N == 128 && a.C % WS_CK == 0 && a.C <= WS_CMAX && (a.K - 1) * a.dil <= 64 && a.T >= 1024;
}
// ... and where the heuristic takes them: the k7 dgrads at >= 64 k rows (the C3
// RU128 dgrads at T = 2000: 4 tiles per sample, 256 per launch); tune key 37:
// 1 = off (the 12-wave kernel), 2 = the ELU-prologue forwards too
bool ws8_gen_pick(const Args& a) {
  return tune(37) != 1 && ws8_gen_ok(a) && a.rows >= 65536 && ((a.pad == 0 && !a.in_elu) || tune(37) == 2);
}
// eight waves of 64 x 64 on the 12-wave kernel's 256 x 128 tile (variant 29):
// the 256-wide K = 3 / 7 layers at T = 400; tune key 38 = 1: on
bool ws8w_ok(const Args& a) {
  return (a.K == 7 || a.K == 3) && a.N % 128 == 0 && a.C % WS_CK == 0 && a.C <= WS_CMAX &&
         (a.K - 1) * a.dil <= 64;
}

// the warp-specialised kernel's legal shapes: K in {3, 7}, 128-multiple N,
// 16-multiple C within the zero source, halo within the staged span, the
// 4-slot ring within 160 KB
bool ws_ok(const Args& a) {
  // (K = 2: the phase-view transposed convs and their adjoints, round 4;
  // tune key 46 = 1: those on the tiled kernel again)
  return ((a.K == 2 && tune(46) != 1) || a.K == 3 || a.K == 7) && a.N % WS_BN == 0 && a.C % WS_CK == 0 && a.C <= WS_CMAX &&
         (a.K - 1) * a.dil <= F4_HALOMAX && ws_lds_bytes(a.K) <= 160 * 1024;
}

template <typename TO>
int launch_ws_k(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
                void* out, hipStream_t s) {
  return a.K == 7 ? launch_ws<7, TO>(a, in, wp, bias, aux, res, out, s)
         : a.K == 3 ? launch_ws<3, TO>(a, in, wp, bias, aux, res, out, s)
                    : launch_ws<2, TO>(a, in, wp, bias, aux, res, out, s);
}

// the sample-tile kernel (conv_wss.hip, variant 30) for the 256-wide layers at
// T = 400: tune key 47 = 1 on, 2 off, 0 = kWssDefault
constexpr bool kWssDefault = true;
bool wss_pick(const Args& a) {
  const int k = tune(47);
  int S = 0, tm = 0;
  // (at T = 2000 not the replicate-pad transposed conv 128 -> 256 phases:
  // tools/conv_bench.py 49.6 us on k_conv_ws_bf16 against 53.0)
  return (k == 1 || (k == 0 && kWssDefault)) && a.N >= 256 && a.rows >= 16384 && wss_ok(a) &&
         wss_geometry(a, S, tm) && (S == 25 || a.pad_mode == SEL_PAD_ZERO);
}
// ... and its 512-row tiles (S = 32) for the 128-wide layers at T = 2000 without an
// input ELU or replicate pad (the k7 / k3 / k2 adjoints and the s4 down conv:
// tools/conv_bench.py RU128 k7d9 dgrad 47.3 -> 40.9 us, down1 45.3 -> 43.2; the
// ELU'd forwards gain nothing, the replicate-pad up conv loses); tune key 50:
// 1 = on, 2 = off, 0 = kWssTallDefault
constexpr bool kWssTallDefault = true;
bool wss_pick_tall(const Args& a) {
  const int k = tune(50);
  int S = 0, tm = 0;
  return (k == 1 || (k == 0 && kWssTallDefault)) && a.N == 128 && a.rows >= 65536 && !a.in_elu &&
         a.pad_mode == SEL_PAD_ZERO && wss_ok(a) && wss_geometry(a, S, tm) && S == 32;
}
// the (16, 128) tiles for the ELU'd 128-wide forwards at T = 2000 (tune key 52:
// 1 = on, 2 = off, 0 = kWssEluDefault): tools/conv_bench.py RU128 k7d9 fwd
// 49.4 (k_conv_fwd_bf16<256, 64>) -> 43.9 us; neutral in the step (the
// launches overlap the side-stream weight gradients)
constexpr bool kWssEluDefault = true;
bool wss_pick_elu(const Args& a) {
  const int k = tune(52);
  int S = 0, tm = 0;
  return (k == 1 || (k == 0 && kWssEluDefault)) && a.N == 128 && a.rows >= 65536 && a.in_elu &&
         a.pad_mode == SEL_PAD_ZERO && wss_ok(a) && wss_geometry(a, S, tm) && S == 16;
}

// the sample-tile kernel on five-sample tiles for the T = 80 layers (the C3
// down / up convs at the 512-wide stage and their adjoints run on 128 x 32 tiles
// at 80 of 128 rows per tile).  Measured in round 6: 55.7 -> 52.7, 50.6 -> 45.4,
// 46.2 -> 44.8 us for the wide layers, but 14.9 -> 23.3 and 22.2 -> 39.2 us at
// N = 64 (13 tiles per 64-wide column are too few workgroups), and the step
// unchanged or slower in same-call A/Bs either way (5.42-5.46 off, 5.47-5.48
// for N >= 512, 5.50-5.51 everywhere).  So off by default; tune key 67: 1 = on
// wherever it applies, 3 = for N >= 512 only
bool wss_pick_short(const Args& a) {
  const int k = tune(67);
  return (k == 1 || (k == 3 && a.N >= 512)) && wss_spt(a) > 1 && a.N % 64 == 0 && wss_ok(a);
}

}  // namespace

namespace sel {
namespace conv {
// Variant of a bf16 forward launch on the pipelined kernels (fwd4_variant
// launches it), -1 when the generic (non-pipelined) kernel is used.  Tune key
// 0 = 21-30 forces a variant where its shape is legal.  out_f32: an fp32-output
// launch (the sample-tile kernel takes those at T <= 400 only, wss_ok_out).
int fwd4_choice(const Args& a, bool out_f32) {
  const int v = tune(0);
  if (!((a.C % CK) == 0 && (a.K - 1) * a.dil <= F4_HALOMAX && a.K <= 8 && (v == 0 || v > 20))) return -1;
  if (v > 20 && v <= 30 && (v != 27 || ws_ok(a)) && (v != 28 || ws8_gen_ok(a)) && (v != 29 || ws8w_ok(a)) &&
      (v != 30 || wss_ok_out(a, out_f32)))
    return v;
  // heuristic from tools/conv_bench.py on the C3 layer shapes (profiles/r1_conv_bench.md):
  // narrow / non-64-multiple outputs and short row counts favour 128x32 tiles
  // (more workgroups in flight); wide layers 128x64 or 256x64.
  // (the T = 80 layers: 128 x 64 / 128 x 128 / 64 x 128 tiles measured 13-50 us
  // slower per graph-replayed C3 step, round 6)
  if (wss_pick_short(a) && wss_ok_out(a, out_f32)) return 30;
  if (a.N <= 32 || (a.N % 64) != 0 || a.rows < 8192) return 22;
  // 256-wide 1x1 (RU256 1x1 fwd 27.5 -> 20.9 us, dgrad 22.5 -> 19.2): 64x128 tiles
  if (a.N >= 256 && a.K == 1) return 26;
  // 256-wide layers at 400 samples x 64 clips (25.6k rows): the warp-specialised
  // 256x128 kernel where legal (rocprofv3 kernel trace, profiles/r2_ws_conv.md:
  // RU256 k7 fwd+dgrad 43.5 -> 38.4 us, down2 46.6 -> 41.8), else 256x64 tiles
  // (RU256 k7 fwd 50.7 -> 36.2 us, dgrad 54.2 -> 43.0, down2 51.2 -> 43.1)
  if (a.N >= 256 && a.rows >= 16384)
    return wss_pick(a) && wss_ok_out(a, out_f32) ? 30 : tune(38) == 1 && ws8w_ok(a) ? 29 : ws_ok(a) ? 27 : 24;
  if (a.N <= 64 || a.rows < 65536) return 23;
  // 128-wide layers at >= 64 k rows on the warp-specialised kernel (one
  // 128-column tile: no input re-read across column tiles) for the k7 dgrads
  // (RU128 d9: 63.6 -> 53.2 us) and the k3 convs (down1: 49.3 -> 44.1 us), not
  // the k7 forwards with their ELU'd 54-row halo (48.6 -> 52.9 us);
  // tools/conv_bench.py.
  if ((wss_pick_tall(a) || wss_pick_elu(a)) && wss_ok_out(a, out_f32)) return 30;
  if (ws8_gen_pick(a)) return 28;
  if (a.N == 128 && ws_ok(a) && (a.K <= 3 || (a.K == 7 && a.pad == 0 && !a.in_elu))) return 27;
  // 128-wide k7 dgrad at 2000 samples (pad 0, no input ELU): 128x32 tiles (76.5 -> 62.6 us)
  if (a.N == 128 && a.K > 1 && a.pad == 0 && !a.in_elu) return 22;
  return 24;
}
}  // namespace conv
}  // namespace sel

namespace {

// launches variant v = fwd4_choice(a, TO is fp32)
template <int KMAX, typename TO>
int fwd4_variant(int v, const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
                 const void* res, void* out, hipStream_t s) {
  switch (v) {
    case 21: return launch_fwd4<256, 32, 4, KMAX, TO>(a, in, wp, bias, aux, res, out, s);
    case 22: return launch_fwd4<128, 32, 4, KMAX, TO>(a, in, wp, bias, aux, res, out, s);
    case 23: return launch_fwd4<128, 64, 2, KMAX, TO>(a, in, wp, bias, aux, res, out, s);
    case 24: return launch_fwd4<256, 64, 4, KMAX, TO>(a, in, wp, bias, aux, res, out, s);
    case 25: return launch_fwd4<128, 128, 2, KMAX, TO>(a, in, wp, bias, aux, res, out, s);
    case 27: return launch_ws_k<TO>(a, in, wp, bias, aux, res, out, s);
    case 28: return launch_ws8<7, TO, 512, 128, 64>(a, in, wp, bias, aux, res, out, s);
    case 29:
      if (a.K == 7) return launch_ws8<7, TO, 256, 128, 64, 2>(a, in, wp, bias, aux, res, out, s);
      return launch_ws8<3, TO, 256, 128, 64, 2>(a, in, wp, bias, aux, res, out, s);
    case 30: return launch_wss<TO>(a, in, wp, bias, aux, res, out, s);
    default: return launch_fwd4<64, 128, 1, KMAX, TO>(a, in, wp, bias, aux, res, out, s);  // 26
  }
}

// Weight-stationary thin kernel (tune key 4: 0 = use where legal, 1 = off;
// key 5: target workgroup count, 0 = 1024).

template <int C, int N, int K, int R, bool E>
int launch_thin(const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
                const void* res, void* out, hipStream_t s) {
  using G = Thin<C, N, K, R, E>;
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  // one round of resident workgroups (each pays the weight-fragment prologue
  // once; a grid just past the resident capacity would add a whole round for
  // its tail); tune key 5 > 0 overrides the workgroup target
  static const int64_t slots =
      resident_blocks((const void*)k_conv_thin_bf16<C, N, K, R, E>, 256, G::LDS_TOTAL) / 8 * 8;
  const int64_t target = tune(5) > 0 ? tune(5) : (slots > 0 ? slots : 1024);
  const int64_t tpb = tiles_per_block(ntiles, target);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));  // multiple of 8 (XCD map)
  hipLaunchKernelGGL((k_conv_thin_bf16<C, N, K, R, E>), dim3(nb), dim3(256), G::LDS_TOTAL, s, a,
                     static_cast<const __bf16*>(in), static_cast<const __bf16*>(wp), bias,
                     static_cast<const __bf16*>(aux), static_cast<const __bf16*>(res), static_cast<__bf16*>(out),
                     int(tpb), 3 & ~tune(11));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// the (i, C, N, K) instances with their default / alternative tile rows:
// residual-unit k7 / 1x1 at 32 and 64 channels, the first strided conv
// (96 -> 64, 3 taps), the last transposed conv's dgrad (96 -> 64, 2 taps),
// the 128-channel residual-unit 1x1 (one 32-channel output slice per wave;
// k_pw_bf16 by default), and the last transposed conv's forward (64 -> 96,
// 2 taps, replicate pad) and the first strided conv's dgrad (64 -> 96, 3
// taps): three output slices, the fourth wave stages and stores only.
// A/B knobs: tune key 7 bit i = instance i off (tiled kernel instead),
// key 6 bit i = instance i on its alternative tile rows
#define SEL_THIN_SHAPES(X) X(0, 32, 32, 7, 256, 128) X(1, 32, 32, 1, 256, 128) X(2, 64, 64, 7, 128, 64) \
  X(3, 64, 64, 1, 128, 64) X(4, 96, 64, 3, 128, 64) X(5, 96, 64, 2, 128, 64) X(6, 128, 128, 1, 64, 32) \
  X(7, 64, 96, 2, 128, 64) X(8, 64, 96, 3, 128, 64)

int thin_index(const Args& a) {
  // (one sample's rows must fit a 2^31-byte buffer resource: ru_rsrc)
  if (tune(4) == 1 || (a.K - 1) * a.dil > F4_HALOMAX || !ru_region_ok(int64_t(a.T) * a.C * 2)) return -1;
#define SEL_THIN_IDX(I_, C_, N_, K_, R_, R2_) \
  if (a.C == C_ && a.N == N_ && a.K == K_) return (tune(7) >> I_) & 1 ? -1 : I_;
  SEL_THIN_SHAPES(SEL_THIN_IDX)
#undef SEL_THIN_IDX
  return -1;
}

// measured per layer (tools/conv_bench.py 30 34 35 36 37, profiles/r1_conv_bench_epf.md):
// the prefetch pays on the k7 dgrads (ELU'(aux) operand) at 32 channels /
// 256 rows (113 -> 88 us) and 64 channels / 64 rows (77 -> 72 us); on the
// 1x1 and strided instances the VGPRs it takes cost more occupancy than it hides
constexpr int kThinEpfDefault = 0b101;  // instances 0 and 2
constexpr int kThinEpfAlt = 0b100;      // instance 2 on its 64-row tiles

// epilogue prefetch + split loop: only for launches with epilogue operands
// (aux and/or res), per instance by kThinEpfDefault (key 12 bit i flips
// instance i, key 11 bit 0 forces it off); kThinEpfAlt instances run it on
// their alternative tile rows.  Returns the E flag, sets the tile rows.
bool thin_variant(const Args& a, bool has_epilogue, int& rows) {
  const int i = thin_index(a);
  const bool epf = has_epilogue && ((kThinEpfDefault ^ tune(12)) >> i & 1) && !(tune(11) & 1);
  const bool alt = (((tune(6) >> i) & 1) != 0) != (epf && ((kThinEpfAlt >> i) & 1));
  rows = 0;
#define SEL_THIN_RV(I_, C_, N_, K_, R_, R2_) if (i == I_) rows = alt ? R2_ : R_;
  SEL_THIN_SHAPES(SEL_THIN_RV)
#undef SEL_THIN_RV
  return epf;
}

// instance i (thin_index) with the E flag and tile rows of thin_variant
int launch_thin_variant(int i, bool e, int rows, const Args& a, const void* in, const void* wp, const float* bias,
                        const void* aux, const void* res, void* out, hipStream_t s) {
#define SEL_THIN_LAUNCH(I_, C_, N_, K_, R_, R2_)                                                   \
  if (i == I_)                                                                                     \
    return e ? (rows == R2_ ? launch_thin<C_, N_, K_, R2_, true>(a, in, wp, bias, aux, res, out, s)   \
                            : launch_thin<C_, N_, K_, R_, true>(a, in, wp, bias, aux, res, out, s))   \
             : (rows == R2_ ? launch_thin<C_, N_, K_, R2_, false>(a, in, wp, bias, aux, res, out, s)  \
                            : launch_thin<C_, N_, K_, R_, false>(a, in, wp, bias, aux, res, out, s));
  SEL_THIN_SHAPES(SEL_THIN_LAUNCH)
#undef SEL_THIN_LAUNCH
  set_error("no thin kernel instance %d", i);
  return SEL_ERR_STATE;
}

// Pointwise kernel (k_pw_bf16) where it applies: 1x1, C = N in {128, 256}
// (the RU128 / RU256 1x1 forwards and dgrads; rocprof on the C3 shapes:
// 21.0 -> 19.6 us at 128 (thin kernel before), 19.1 -> 14.3 us at 256);
// tune key 42: 1 = off; key 43 > 0: workgroup count
bool pw_ok(const Args& a) {
  // (a forced tiled variant, tune key 0, takes precedence)
  if (a.K != 1 || a.C != a.N || a.pad != 0 || tune(42) == 1 || tune(0) != 0) return false;
  if (!(a.N == 256 || a.N == 128)) return false;
  // every block's row range is one buffer resource
  return ru_region_ok(a.rows * int64_t(a.N) * 2);
}

template <int C, int N, bool ELU, bool AUX, bool RES>
int launch_pw_t(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
                void* out, hipStream_t s) {
  using G = Pw<C, N>;
  if (a.rows == 0) return SEL_OK;
  // one round of resident workgroups, each over an equal contiguous row range
  static const int64_t round = resident_blocks((const void*)k_pw_bf16<C, N, ELU, AUX, RES>, G::THREADS, G::LDS);
  const int64_t target = tune(43) > 0 ? tune(43) : (round > 0 ? round : 256);
  int64_t nb = std::min<int64_t>(target, (a.rows + G::R - 1) / G::R);
  // (a pass covers RB rows: a range of more rows takes several passes)
  const int64_t rpb = (a.rows + nb - 1) / nb;
  nb = (a.rows + rpb - 1) / rpb;
  hipLaunchKernelGGL((k_pw_bf16<C, N, ELU, AUX, RES>), dim3(unsigned(nb)), dim3(G::THREADS), G::LDS, s, a,
                     static_cast<const __bf16*>(in), static_cast<const __bf16*>(wp), bias,
                     static_cast<const __bf16*>(aux), static_cast<const __bf16*>(res), static_cast<__bf16*>(out),
                     int(rpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int C, int N, bool ELU>
int launch_pw_e(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
                void* out, hipStream_t s) {
  if (aux && res) return launch_pw_t<C, N, ELU, true, true>(a, in, wp, bias, aux, res, out, s);
  if (aux) return launch_pw_t<C, N, ELU, true, false>(a, in, wp, bias, aux, res, out, s);
  if (res) return launch_pw_t<C, N, ELU, false, true>(a, in, wp, bias, aux, res, out, s);
  return launch_pw_t<C, N, ELU, false, false>(a, in, wp, bias, aux, res, out, s);
}

template <int C, int N>
int launch_pw(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
              void* out, hipStream_t s) {
  return a.in_elu ? launch_pw_e<C, N, true>(a, in, wp, bias, aux, res, out, s)
                  : launch_pw_e<C, N, false>(a, in, wp, bias, aux, res, out, s);
}

// single-input-channel forward (k_conv_c1_bf16): one resident round of
// workgroups walking TR-row tiles (they prefetch their next tile); tune key
// 44 = 1: the round-3 256-row tiles
template <typename TI, typename TO, int TR>
int launch_c1(const Args& a, const void* in, const void* wp, const float* bias, const void* aux, const void* res,
              void* out, hipStream_t s) {
  static const int64_t round = resident_blocks((const void*)k_conv_c1<TI, TO, TR>, 256, 0);
  const int64_t slots = round > 0 ? std::max<int64_t>(256, round) : 4096;
  const int64_t blocks = std::min<int64_t>((a.rows / a.T) * ((a.T + TR - 1) / TR), tune(23) > 0 ? tune(23) : slots);
  if (blocks <= 0) return SEL_OK;
  hipLaunchKernelGGL((k_conv_c1<TI, TO, TR>), dim3(unsigned(blocks)), dim3(256), 0, s, a,
                     static_cast<const TI*>(in), static_cast<const TI*>(wp), bias,
                     static_cast<const TO*>(aux), static_cast<const TO*>(res), static_cast<TO*>(out));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// Kernel family of a forward launch and the variant within it.  The order
// pw -> thin -> c1 -> pipelined tiles -> generic is stated here alone:
// sel_conv_fwd launches the pick, sel_conv_fwd_kernel_id reports it.
enum Family {
  kPw,        // k_pw_bf16; v = N
  kThin,      // k_conv_thin_bf16; v = instance (thin_variant gives the E flag and tile rows)
  kC1,        // k_conv_c1; v = tile rows
  kFast,      // the pipelined bf16 kernels; v = fwd4_choice
  kF32Tiles,  // k_conv_fwd_f32; v = BM (64: 64 x 64 tiles, 128: 128 x 32)
  kGeneric    // k_conv_fwd; v = tile 1-6 (tune key 0 forces one)
};
struct FwdPick {
  Family family;
  int v;
};

bool c1_shape(const Args& a, int nmult) {
  return a.C == 1 && a.N % nmult == 0 && a.N <= C1_NMAX && a.K <= C1_KMAX && (a.K - 1) * a.dil <= C1_HALO;
}

FwdPick fwd_pick(const Args& a, int in_dtype, int out_dtype) {
  if (in_dtype == SEL_BF16) {
    if (out_dtype == SEL_BF16) {
      if (pw_ok(a)) return {kPw, a.N};
      if (const int i = thin_index(a); i >= 0) return {kThin, i};
    }
    // tune key 44: 1 = the round-3 256-row tiles, 2 = 1024-row tiles
    if (c1_shape(a, 8) && tune(3) == 0) return {kC1, tune(44) == 1 ? 256 : tune(44) == 2 ? 1024 : C1F_TR};
    if (const int v = fwd4_choice(a, out_dtype == SEL_F32); v >= 0) return {kFast, v};
    if (const int v = tune(0); v >= 1 && v <= 6) return {kGeneric, v};
    return {kGeneric, a.N <= 32 ? 1 : (a.N <= 64 || a.K >= 5) ? 2 : a.rows >= 4096 ? 3 : 4};
  }
  if (out_dtype == SEL_F32 && tune(55) != 1) {  // tune key 55 = 1: the generic kernel
    // single input channel: the streaming kernel with exact fp32 ELU
    if (c1_shape(a, 4)) return {kC1, C1F_TR};
    // sample-aligned fp32 tiles
    if (a.C % FF_CK == 0 && a.N % 32 == 0 && a.K <= 8 && (a.K - 1) * a.dil <= FF_HALO)
      return {kF32Tiles, a.N % 64 == 0 ? 64 : 128};
  }
  return {kGeneric, a.N <= 32 ? 1 : 4};
}

template <typename TI, typename TO>
int dispatch_fwd(const Args& a, const void* in, const void* wp, const float* bias, const void* aux,
                 const void* res, void* out, hipStream_t s) {
  const FwdPick p = fwd_pick(a, sizeof(TI) == 4 ? SEL_F32 : SEL_BF16, sizeof(TO) == 4 ? SEL_F32 : SEL_BF16);
  if constexpr (sizeof(TI) == 2) {
    switch (p.family) {
      case kPw:
        return a.N == 256 ? launch_pw<256, 256>(a, in, wp, bias, aux, res, out, s)
                          : launch_pw<128, 128>(a, in, wp, bias, aux, res, out, s);
      case kThin: {
        int rows = 0;
        const bool e = thin_variant(a, aux || res, rows);
        return launch_thin_variant(p.v, e, rows, a, in, wp, bias, aux, res, out, s);
      }
      case kC1:
        return p.v == 256    ? launch_c1<TI, TO, 256>(a, in, wp, bias, aux, res, out, s)
               : p.v == 1024 ? launch_c1<TI, TO, 1024>(a, in, wp, bias, aux, res, out, s)
                             : launch_c1<TI, TO, C1F_TR>(a, in, wp, bias, aux, res, out, s);
      case kFast:
        if (a.K == 1) return fwd4_variant<1, TO>(p.v, a, in, wp, bias, aux, res, out, s);
        if (a.K <= 3) return fwd4_variant<3, TO>(p.v, a, in, wp, bias, aux, res, out, s);
        return fwd4_variant<8, TO>(p.v, a, in, wp, bias, aux, res, out, s);
      default: break;
    }
    switch (p.v) {  // kGeneric
      case 2: return launch_fwd<TI, TO, 128, 64>(a, in, wp, bias, aux, res, out, s);
      case 3: return launch_fwd<TI, TO, 128, 128>(a, in, wp, bias, aux, res, out, s);
      case 5: return launch_fwd<TI, TO, 256, 32>(a, in, wp, bias, aux, res, out, s);
      case 6: return launch_fwd<TI, TO, 256, 64>(a, in, wp, bias, aux, res, out, s);
      default: break;
    }
  } else {
    if (p.family == kC1) return launch_c1<TI, TO, C1F_TR>(a, in, wp, bias, aux, res, out, s);
    if (p.family == kF32Tiles)
      return p.v == 64 ? launch_fwd_f32<64, 64>(a, in, wp, bias, aux, res, out, s)
                       : launch_fwd_f32<128, 32>(a, in, wp, bias, aux, res, out, s);
  }
  if (p.v == 1) return launch_fwd<TI, TO, 128, 32>(a, in, wp, bias, aux, res, out, s);
  return launch_fwd<TI, TO, 64, 64>(a, in, wp, bias, aux, res, out, s);
}

}  // namespace

// Discriminator layers (dconv.hip's plan_fwd, sel_dconv_desc) on the warp-specialised
// 256 x 128 kernel: one group, a contiguous reduction row (S == 1 or Cs == Cg:
// the phase view of a strided layer is S * Cg contiguous channels), contiguous
// output columns, K in {2, 3, 5, 7}.  The MPD's (5,1) convs are K = 5 (stride 1)
// or K = 2 taps over 3 * Cin channels (stride 3, phase view); their adjoints the
// same K over gout with So = 3 output phases.  Returns SEL_ERR_UNSUPPORTED for
// any other shape (the caller keeps its own kernels).
namespace sel {
namespace conv {
int dconv_ws_mode(const sel_dconv_desc* d) {
  const int width = d->So * d->Ng, nred = d->S * d->Cg;
  const bool ok = d->G == 1 && (d->S == 1 || d->Cs == d->Cg) && (d->So == 1 || d->Ns == d->Ng) &&
                  (d->K == 2 || d->K == 3 || d->K == 5 || d->K == 7) && width % WS_BN == 0 &&
                  nred % WS_CK == 0 && nred <= WS_CMAX && d->ldx % 8 == 0 && d->ldo % 8 == 0 &&
                  d->ldx >= nred && d->ldo >= width && d->Tvo > 0 && d->B > 0 && d->Tv <= d->Tvs &&
                  d->K - 1 <= F4_HALOMAX && -d->q0 <= F4_HALOMAX && ws_lds_bytes(d->K) <= 160 * 1024;
  if (!ok) return -1;
  // flat tiling (tune key 22: 1 = off) where the layout leaves zero gaps
  // between sequences (sel.dconvops allocates the MPD chain so; its deep layers
  // have 54-300 rows per period column, a 256-row sample-aligned tile wastes up
  // to 80% there): every row a tap may read across a sequence boundary lies in a gap
  // (input row >= Tv) or feeds an output row that is written as zero (>= Tvalid)
  const int P = d->Tvo;
  const bool flat = tune(22) != 1 && d->Tvs == P && P - d->Tv >= -d->q0 && P - d->Tvalid >= d->q0 + d->K - 1 &&
                    int64_t(d->B) * P < (int64_t(1) << 31);
  return flat ? 1 : 0;
}

// the eight-wave kernel's 256 x 256 tiles for the MPD's 128 -> 512 stride-3
// layer (K = 2 taps over 384 phase channels: 141 -> 126 us at period 2, D
// step, tools/ws8_probe.py); the deeper K = 2 / 5 layers stay on the 12-wave
// kernel (512 -> 1024 s3: 218 vs 248 us, 1024 -> 1024 k5: 279 vs 339 us: with
// 64-96 chunks per tile the DMA issue the eight waves take on costs more than
// the fragment reads they save); tune key 37 = 1: off
bool dconv_ws8_ok(const sel_dconv_desc* d) {
  return tune(37) != 1 && d->K == 2 && d->S * d->Cg <= 512 && (d->So * d->Ng) % 256 == 0 && dconv_ws_mode(d) >= 0;
}

int dconv_ws_fwd(const sel_dconv_desc* d, const void* x, const void* wp, const float* bias, const void* aux,
                 const void* res, void* out, hipStream_t s) {
  const int mode = dconv_ws_mode(d);
  if (mode < 0) return SEL_ERR_UNSUPPORTED;
  const bool flat = mode == 1;
  const int width = d->So * d->Ng, nred = d->S * d->Cg;
  const int P = d->Tvo;
  Args a;
  a.rows = int64_t(d->B) * d->Tvo;
  a.T = flat ? int(a.rows) : d->Tvo;
  a.seq_pitch = flat ? P : 0;
  a.C = nred;
  a.N = width;
  a.K = d->K;
  a.dil = 1;
  a.pad = -d->q0;
  a.pad_mode = SEL_PAD_ZERO;
  a.in_elu = 0;
  a.bias_period = 0;
  a.tin_valid = d->Tv;
  a.tin_pitch = d->Tvs;
  a.ldx = d->ldx;
  a.ldo = d->ldo;
  a.tout_valid = d->Tvalid;
  a.epi = 1;
  a.act = d->act;
  a.slope = d->slope;
  if (dconv_ws8_ok(d)) return launch_ws8<2, __bf16, 256, 256, 32>(a, x, wp, bias, aux, res, out, s);  // K == 2
  switch (d->K) {
    case 2: return launch_ws<2, __bf16>(a, x, wp, bias, aux, res, out, s);
    case 3: return launch_ws<3, __bf16>(a, x, wp, bias, aux, res, out, s);
    case 5: return launch_ws<5, __bf16>(a, x, wp, bias, aux, res, out, s);
    default: return launch_ws<7, __bf16>(a, x, wp, bias, aux, res, out, s);
  }
}
}  // namespace conv
}  // namespace sel

extern "C" {

int sel_conv_fwd_kernel_id(const sel_conv_desc* d, int in_dtype, int out_dtype, int has_epilogue) {
  if (!d || in_dtype != SEL_BF16 || check_desc(d) != SEL_OK) return -1;
  const Args a = to_args(d);
  const FwdPick p = fwd_pick(a, in_dtype, out_dtype);
  if (p.family == kPw) return 930000000 + a.N;  // pointwise: 9.3e8 + N
  if (p.family == kThin) {  // thin: 1e9 + E*5e8 + ((R/32*1000 + C)*1000 + N)*10 + K
    int r = 0;
    const bool e = thin_variant(a, has_epilogue != 0, r);
    return 1000000000 + (e ? 500000000 : 0) + ((r / 32 * 1000 + a.C) * 1000 + a.N) * 10 + a.K;
  }
  if (p.family != kFast) return -1;
  const int v = p.v;
  // warp-specialised kernels: 9e8 + K (12 waves), 9.1e8 + K (eight waves, 512 x 128)
  if (v == 27) return 900000000 + a.K;
  if (v == 28) return 910000000 + a.K;
  if (v == 29) return 920000000 + a.K;
  if (v == 30) {  // sample-tile kernel: 9.4e8 + 1e6 (SPT - 1) + 1e4 BN + 10 S + K
    int S = 0, tm = 0, BN = 0;
    wss_geometry(a, S, tm, BN);
    return 940000000 + 1000000 * (wss_spt(a) - 1) + 10000 * BN + 10 * S + a.K;
  }
  const int kmax = a.K == 1 ? 1 : (a.K <= 3 ? 3 : 8);
  static const int bm[] = {256, 128, 128, 256, 128, 64}, bn[] = {32, 32, 64, 64, 128, 128}, wm[] = {4, 4, 2, 4, 2, 1};
  const int i = v - 21;
  return ((bm[i] * 1000 + bn[i]) * 10 + wm[i]) * 10 + kmax;  // BM,BN,WAVES_M,KMAX packed
}

int sel_conv_fwd(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* in, const void* wpack,
                 const float* bias, const void* aux, const void* res, void* out, sel_stream_t stream) {
  if (int rc = check_desc(d)) return rc;
  const Args a = to_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (in_dtype == SEL_F32 && out_dtype == SEL_F32)
    return dispatch_fwd<float, float>(a, in, wpack, bias, aux, res, out, s);
  if (in_dtype == SEL_BF16 && out_dtype == SEL_BF16)
    return dispatch_fwd<__bf16, __bf16>(a, in, wpack, bias, aux, res, out, s);
  if (in_dtype == SEL_BF16 && out_dtype == SEL_F32)
    return dispatch_fwd<__bf16, float>(a, in, wpack, bias, aux, res, out, s);
  set_error("unsupported dtype combination in=%d out=%d", in_dtype, out_dtype);
  return SEL_ERR_UNSUPPORTED;
}

}  // extern "C"
