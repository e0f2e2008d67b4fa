// Grouped streaming step primitive (sel_hfg_conv_step, and its slot-indexed pool
// form sel_hfg_conv_step_pool): one causal layer of one
// HiFi-GAN vocoder hop, the grouped LeakyReLU primitive of hifigan.hip with the
// reference's pad_buffer as an explicit carry.
//
// The design is that of stream.hip (weight-streaming: each weight element is
// used once per launch, so 16-byte weight vectors go straight into MFMA B
// operands and the A operand is gathered from [carry | act(in)]):
//
//   block      = 16 output channels of ONE group x RT row tiles of 16 rows, NW
//                waves; ceil((N/G)/16) masked column tiles per group, because the
//                A operand (the group's input channels) is shared by the tile's
//                16 columns
//   wave w     = reduction chunks w, w + NW, ... of the flat K*(C/G) axis
//   reduction  = every wave's 16 x 16 fp32 accumulator goes to LDS and is summed
//                in wave order: no atomics, and NW depends on K*(C/G) alone, so
//                an output's bits do not depend on B, T, the row-tile count or
//                the group count
//   carry_out  = written by extra blocks of the same launch, pitch C (once per
//                group when the new rows are shared), the same act() on the new rows
#include "step_common.h"

#include <algorithm>

namespace sel {
namespace hfgstep {
using namespace sel::step;

struct GArgs {
  int64_t rows;
  int T, C, Cg, N, Ng, K, dil, P;
  int ldin, igs, ldres, rgs;      // pitch of the new rows / res, group offsets in them
  int bias_period, act, tanh_out, accumulate;
  float slope, scale;
  int KC, nchunk, tpg, ncol, ngrp;  // K*(C/G), its chunks, column tiles per group, G * tpg, row groups
  int64_t carry_elems;              // B * P * C
};

// the activation of the new rows: one function for the conv operand and for
// carry_out, so the carried rows are the bits the conv consumed (bf16: rounded once)
__device__ __forceinline__ float act1(float v, float slope) { return v >= 0.f ? v : slope * v; }
__device__ __forceinline__ __bf16 act1(__bf16 v, float slope) { return __bf16(act1(float(v), slope)); }

// channel c of group g, row vrow of sample b's virtual input [carry (P rows, pitch C) | act(in) (T rows)];
// bc is the sample's row of the carry: b itself, or its slot in a pool
template <typename TI>
__device__ __forceinline__ TI virt(const GArgs& a, const TI* __restrict__ carry, const TI* __restrict__ in, int bc,
                                   int b, int vrow, int g, int c) {
  if (vrow < a.P) return carry[(int64_t(bc) * a.P + vrow) * a.C + g * a.Cg + c];
  const TI v = in[(int64_t(b) * a.T + (vrow - a.P)) * a.ldin + g * a.igs + c];
  return a.act ? act1(v, a.slope) : v;
}

template <typename TI, bool VEC>
__device__ __forceinline__ typename Frag<TI>::type load_a(const GArgs& a, const TI* __restrict__ carry,
                                                          const TI* __restrict__ in, bool ok, int bc, int b, int t,
                                                          int g, int r0) {
  typedef typename Frag<TI>::type F;
  constexpr int E = Frag<TI>::E;
  F f;
#pragma unroll
  for (int i = 0; i < E; ++i) f[i] = TI(0.f);
  if (!ok) return f;
  if constexpr (VEC) {
    if (r0 < a.KC) {   // (C/G) % 8 == 0: the E elements share one tap
      const int k = r0 / a.Cg, c = r0 - k * a.Cg;
      const int vrow = t + k * a.dil;
      if (vrow < a.P) {
        f = *reinterpret_cast<const F*>(carry + (int64_t(bc) * a.P + vrow) * a.C + g * a.Cg + c);
      } else {
        f = *reinterpret_cast<const F*>(in + (int64_t(b) * a.T + (vrow - a.P)) * a.ldin + g * a.igs + c);
        if (a.act) {
#pragma unroll
          for (int i = 0; i < E; ++i) f[i] = act1(f[i], a.slope);
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int r = r0 + i;
      if (r < a.KC) {
        const int k = r / a.Cg, c = r - k * a.Cg;
        f[i] = virt(a, carry, in, bc, b, t + k * a.dil, g, c);
      }
    }
  }
  return f;
}

// n: the output channel over all groups, or -1 for a masked column
template <typename TI, bool VEC>
__device__ __forceinline__ typename Frag<TI>::type load_b(const GArgs& a, const TI* __restrict__ wp, int n, int r0) {
  typedef typename Frag<TI>::type F;
  constexpr int E = Frag<TI>::E;
  F f;
#pragma unroll
  for (int i = 0; i < E; ++i) f[i] = TI(0.f);
  if (n < 0) return f;
  const TI* row = wp + int64_t(n) * a.KC;
  if constexpr (VEC) {
    if (r0 < a.KC) f = *reinterpret_cast<const F*>(row + r0);
  } else {
#pragma unroll
    for (int i = 0; i < E; ++i)
      if (r0 + i < a.KC) f[i] = row[r0 + i];
  }
  return f;
}

// POOL = false is sel_hfg_conv_step (p unused); POOL = true adds the slot table and
// the per-tick row count, everything else is shared so the two give the same bits
template <typename TI, typename TO, bool VEC, int RT, bool POOL>
__device__ __forceinline__ void hfg_step_body(const Launch& lc, const GArgs& a, const PoolArgs& p,
                                              const TI* __restrict__ carry, const TI* __restrict__ in,
                                              const TI* __restrict__ wp, const float* __restrict__ bias,
                                              const TO* __restrict__ res, TO* out,
                                              TI* __restrict__ carry_out) {
  extern __shared__ float red[];  // [NW][RT][4][64]
  constexpr int E = Frag<TI>::E;
  constexpr int CH = 4 * E;
  const int nconv = a.ncol * a.ngrp;
  const int tid = lc.tid;
  int64_t rows = a.rows;   // the rows that exist: all of them, or this tick's n * T
  int nact = 0;
  if constexpr (POOL) {
    nact = pool_count(p);
    rows = int64_t(nact) * a.T;
  }
  if (int(lc.bid) >= nconv) {
    // carry_out[b][j] = v[b][T + j] over all C channels: old carry rows while T + j < P, then the new rows
    const int64_t stride = int64_t(lc.nblk - nconv) * lc.bdim;
    const int64_t pc = int64_t(a.P) * a.C;
    if constexpr (POOL) {
      const int64_t live = int64_t(nact) * pc;   // the active samples' elements; blocks past them do nothing
      for (int64_t e = int64_t(lc.bid - nconv) * lc.bdim + tid; e < live; e += stride) {
        const int b = int(e / pc);
        const int rem = int(e - int64_t(b) * pc);
        const int j = rem / a.C, cf = rem - j * a.C;
        const int g = cf / a.Cg;
        const int slot = p.slots[b];
        if (pool_slot_ok(p, slot))
          carry_out[int64_t(slot) * pc + rem] = virt(a, carry, in, slot, b, a.T + j, g, cf - g * a.Cg);
      }
    } else {
      for (int64_t e = int64_t(lc.bid - nconv) * lc.bdim + tid; e < a.carry_elems; e += stride) {
        const int b = int(e / pc);
        const int rem = int(e - int64_t(b) * pc);
        const int j = rem / a.C, cf = rem - j * a.C;
        const int g = cf / a.Cg;
        carry_out[e] = virt(a, carry, in, b, b, a.T + j, g, cf - g * a.Cg);
      }
    }
    return;
  }
  const int NW = lc.bdim >> 6;
  const int lane = tid & 63, w = tid >> 6;
  const int col = int(lc.bid) % a.ncol, grp = int(lc.bid) / a.ncol;
  const int g = col / a.tpg, nt = col - g * a.tpg;
  const int ng = nt * 16 + (lane & 15);               // this lane's B column inside the group
  const int n = ng < a.Ng ? g * a.Ng + ng : -1;
  const int roff = E * (lane >> 4);

  if constexpr (POOL) {
    if (int64_t(grp) * RT * 16 >= rows) return;   // a row group past this tick's rows: before any load
  }
  bool ok[RT];
  int sb[RT], sc[RT], st[RT];
  floatx4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t m = (int64_t(grp) * RT + rt) * 16 + (lane & 15);
    ok[rt] = m < rows;
    sb[rt] = ok[rt] ? int(m / a.T) : 0;
    st[rt] = ok[rt] ? int(m - int64_t(sb[rt]) * a.T) : 0;
    sc[rt] = sb[rt];
    if constexpr (POOL) {
      if (ok[rt]) {
        sc[rt] = p.slots[sb[rt]];
        ok[rt] = pool_slot_ok(p, sc[rt]);
      }
    }
    acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // U chunks in flight per wave (one row tile: the loads are the whole latency);
  // a chunk past the end loads zeros on both operands
  constexpr int U = RT == 1 ? 4 : 1;
  for (int ch = w; ch < a.nchunk; ch += NW * U) {
    typename Frag<TI>::type fb[U], fa[U][RT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r0 = (ch + u * NW) * CH + roff;
      fb[u] = load_b<TI, VEC>(a, wp, n, r0);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) fa[u][rt] = load_a<TI, VEC>(a, carry, in, ok[rt], sc[rt], sb[rt], st[rt], g, r0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = mma(fa[u][rt], fb[u], acc[rt]);
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[((w * RT + rt) * 4 + i) * 64 + lane] = acc[rt][i];
  __syncthreads();
  for (int o = tid; o < RT * 256; o += lc.bdim) {
    const int rt = o >> 8, i = (o >> 6) & 3, l = o & 63;
    float s = red[(rt * 4 + i) * 64 + l];
    for (int ww = 1; ww < NW; ++ww) s += red[((ww * RT + rt) * 4 + i) * 64 + l];  // fixed order
    const int64_t m = (int64_t(grp) * RT + rt) * 16 + (l >> 4) * 4 + i;
    const int nn = nt * 16 + (l & 15);
    bool live = m < rows && nn < a.Ng;
    if constexpr (POOL) {
      if (live) live = pool_slot_ok(p, p.slots[int(m / a.T)]);
    }
    if (live) {
      // the epilogue of sel_hfg_conv_fwd, in its order
      const int c = g * a.Ng + nn;
      if (a.bias_period > 0) s += bias[c % a.bias_period];
      if (res) s += to_f(res[m * a.ldres + g * a.rgs + nn]);
      if (a.tanh_out) s = tanhf(s);
      s *= a.scale;
      TO* op = out + m * a.N + c;
      if (a.accumulate) s += to_f(*op);
      *op = from_f<TO>(s);
    }
  }
}

template <typename TI, typename TO, bool VEC, int RT>
__global__ void __launch_bounds__(MAX_NW * 64)
k_hfg_step(GArgs a, const TI* __restrict__ carry, const TI* __restrict__ in, const TI* __restrict__ wp,
           const float* __restrict__ bias, const TO* __restrict__ res, TO* out, TI* __restrict__ carry_out) {
  const Launch lc{blockIdx.x, gridDim.x, threadIdx.x, blockDim.x};
  hfg_step_body<TI, TO, VEC, RT, false>(lc, a, PoolArgs{}, carry, in, wp, bias, res, out, carry_out);
}

template <typename TI, typename TO, bool VEC, int RT>
__global__ void __launch_bounds__(MAX_NW * 64)
k_hfg_step_pool(GArgs a, PoolArgs p, const TI* __restrict__ carry, const TI* __restrict__ in,
                const TI* __restrict__ wp, const float* __restrict__ bias, const TO* __restrict__ res, TO* out,
                TI* __restrict__ carry_out) {
  const Launch lc{blockIdx.x, gridDim.x, threadIdx.x, blockDim.x};
  hfg_step_body<TI, TO, VEC, RT, true>(lc, a, p, carry, in, wp, bias, res, out, carry_out);
}

template <typename TI, typename TO>
int launch_step(const GArgs& a, const PoolArgs* p, bool vec, int rt, int nw, int ncarry, const void* carry,
                const void* in, const void* wp, const float* bias, const void* res, void* out, void* carry_out,
                hipStream_t s) {
  const dim3 grid(unsigned(a.ncol * a.ngrp + ncarry)), block(unsigned(nw * 64));
  const size_t lds = size_t(nw) * rt * 256 * sizeof(float);
#define SEL_HSTEP_LAUNCH(V, R)                                                                                    \
  do {                                                                                                            \
    if (p)                                                                                                        \
      hipLaunchKernelGGL((k_hfg_step_pool<TI, TO, V, R>), grid, block, lds, s, a, *p,                             \
                         static_cast<const TI*>(carry), static_cast<const TI*>(in), static_cast<const TI*>(wp),   \
                         bias, static_cast<const TO*>(res), static_cast<TO*>(out), static_cast<TI*>(carry_out)); \
    else                                                                                                          \
      hipLaunchKernelGGL((k_hfg_step<TI, TO, V, R>), grid, block, lds, s, a, static_cast<const TI*>(carry),       \
                         static_cast<const TI*>(in), static_cast<const TI*>(wp), bias,                            \
                         static_cast<const TO*>(res), static_cast<TO*>(out), static_cast<TI*>(carry_out));       \
  } while (0)
  if (vec && rt == 1) SEL_HSTEP_LAUNCH(true, 1);
  else if (vec) SEL_HSTEP_LAUNCH(true, BIG_RT);
  else if (rt == 1) SEL_HSTEP_LAUNCH(false, 1);
  else SEL_HSTEP_LAUNCH(false, BIG_RT);
#undef SEL_HSTEP_LAUNCH
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// sel_hfg_conv_step (pool == nullptr) and sel_hfg_conv_step_pool share the validation and the geometry
int hfg_conv_step(const char* fn, const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const PoolArgs* pool,
                  const void* carry, const void* in, const void* wpack, const float* bias, const void* res,
                  void* out, void* carry_out, sel_stream_t stream) {
  SEL_REQUIRE(d, SEL_ERR_ARG, "%s: null descriptor", fn);
  SEL_REQUIRE(d->rows > 0 && d->T > 0 && d->C > 0 && d->N > 0 && d->K > 0 && d->dil > 0 && d->groups > 0, SEL_ERR_ARG,
              "%s: rows, T, C, N, K, dil and groups must be positive", fn);
  SEL_REQUIRE(d->T_out == 0 || d->T_out == d->T, SEL_ERR_ARG,
              "%s: T_out (%d) must be 0 or T (%d): T counts the new rows", fn, d->T_out, d->T);
  SEL_REQUIRE(d->rows % d->T == 0, SEL_ERR_ARG, "%s: rows (%lld) is not a multiple of T (%d)", fn,
              (long long)d->rows, d->T);
  const int64_t P64 = int64_t(d->K - 1) * d->dil;
  SEL_REQUIRE(d->pad == P64, SEL_ERR_ARG,
              "%s: pad (%d) must be (K-1)*dil = %lld: the carry is the pad", fn, d->pad, (long long)P64);
  SEL_REQUIRE(d->pad_mode == SEL_PAD_ZERO, SEL_ERR_ARG, "%s: pad_mode must be SEL_PAD_ZERO", fn);
  SEL_REQUIRE(d->act_skip == 0, SEL_ERR_ARG,
              "%s: act_skip (%d) must be 0: the carry is the skipped part", fn, d->act_skip);
  SEL_REQUIRE(d->C % d->groups == 0 && d->N % d->groups == 0, SEL_ERR_ARG,
              "%s: groups %d must divide C %d and N %d", fn, d->groups, d->C, d->N);
  const int G = d->groups, Cg = d->C / G, Ng = d->N / G;
  SEL_REQUIRE(d->in_group_stride == 0 || d->in_group_stride == Cg, SEL_ERR_ARG,
              "%s: in_group_stride %d is neither 0 nor C/G = %d", fn, d->in_group_stride, Cg);
  SEL_REQUIRE(d->res_group_stride == 0 || d->res_group_stride == Ng, SEL_ERR_ARG,
              "%s: res_group_stride %d is neither 0 nor N/G = %d", fn, d->res_group_stride, Ng);
  SEL_REQUIRE(d->bias_period >= 0 && (d->bias_period == 0 || d->N % d->bias_period == 0), SEL_ERR_ARG,
              "%s: bias_period %d must be 0 or divide N %d", fn, d->bias_period, d->N);
  SEL_REQUIRE((in_dtype == SEL_F32 && out_dtype == SEL_F32) ||
                  (in_dtype == SEL_BF16 && (out_dtype == SEL_BF16 || out_dtype == SEL_F32)),
              SEL_ERR_ARG, "%s: dtypes must be fp32 -> fp32 or bf16 -> bf16 / fp32", fn);
  const int64_t B = d->rows / d->T;
  const int64_t KC = int64_t(d->K) * Cg;
  SEL_REQUIRE(B < (1 << 24) && KC < (int64_t(1) << 30) && int64_t(d->N) * KC < (int64_t(1) << 40) &&
                  d->rows < (int64_t(1) << 31) && P64 * d->C < (int64_t(1) << 30),
              SEL_ERR_ARG, "%s: shape out of range", fn);
  SEL_REQUIRE(in && wpack && out, SEL_ERR_ARG, "%s: null in / wpack / out", fn);
  SEL_REQUIRE(d->bias_period == 0 || bias, SEL_ERR_ARG, "%s: bias_period > 0 without a bias", fn);
  if (pool) {
    SEL_REQUIRE(pool->slots && pool->n_active, SEL_ERR_ARG, "%s: null slots / n_active", fn);
    SEL_REQUIRE(pool->nslots > 0 && pool->nslots < (1 << 24), SEL_ERR_ARG, "%s: nslots (%d) out of range", fn,
                pool->nslots);
  }
  const int P = int(P64);
  if (P > 0) {
    SEL_REQUIRE(carry && carry_out, SEL_ERR_ARG,
                "%s: K > 1 needs carry and carry_out (%d rows per sample)", fn, P);
    SEL_REQUIRE(carry != carry_out, SEL_ERR_ARG, "%s: carry_out must not alias carry", fn);
    SEL_REQUIRE(carry_out != in && static_cast<const void*>(out) != carry && out != carry_out &&
                    carry_out != res,
                SEL_ERR_ARG, "%s: carry_out / out alias an input", fn);
  }
  SEL_REQUIRE(static_cast<const void*>(out) != in && out != res, SEL_ERR_ARG,
              "%s: out aliases in / res", fn);

  const int es = in_dtype == SEL_BF16 ? 2 : 4;
  const int E = 16 / es;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // fast path: 16-byte operand loads (every row, group and tap start 16-byte aligned)
  const bool vec = Cg % 8 == 0 && al16(in) && al16(wpack) && (P == 0 || al16(carry));
  GArgs a{};
  a.rows = d->rows; a.T = d->T; a.C = d->C; a.Cg = Cg; a.N = d->N; a.Ng = Ng; a.K = d->K; a.dil = d->dil; a.P = P;
  a.igs = d->in_group_stride; a.ldin = a.igs ? d->C : Cg;
  a.rgs = d->res_group_stride; a.ldres = a.rgs ? d->N : Ng;
  a.bias_period = d->bias_period; a.act = d->act_slope != 1.f; a.tanh_out = d->tanh_out != 0;
  a.accumulate = d->accumulate != 0; a.slope = d->act_slope; a.scale = d->out_scale;
  a.KC = int(KC);
  a.nchunk = int((KC + 4 * E - 1) / (4 * E));
  a.tpg = (Ng + 15) / 16;
  a.carry_elems = B * P * d->C;
  // the reduction split depends on K*(C/G) alone (bit-identical outputs for any B, T and group count)
  const int nw = std::min(MAX_NW, std::max(1, a.nchunk / 4));
  const int64_t ntile = (d->rows + 15) / 16;
  const int rt = ntile >= RT_SWITCH ? BIG_RT : 1;
  const int64_t ngrp = (ntile + rt - 1) / rt;
  const int64_t ncol = int64_t(a.tpg) * G;
  const int64_t per_blk = int64_t(nw) * 64;
  const int64_t ncarry = P > 0 ? std::min<int64_t>(64, (a.carry_elems + per_blk - 1) / per_blk) : 0;
  SEL_REQUIRE(ncol < (int64_t(1) << 24) && ngrp * ncol + ncarry < (int64_t(1) << 31), SEL_ERR_ARG,
              "%s: too many tiles", fn);
  a.ncol = int(ncol);
  a.ngrp = int(ngrp);
  PoolArgs pa{};
  if (pool) {
    pa = *pool;
    pa.cap = int(B);
  }
  const PoolArgs* p = pool ? &pa : nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (in_dtype == SEL_F32)
    return launch_step<float, float>(a, p, vec, rt, nw, int(ncarry), carry, in, wpack, bias, res, out, carry_out, s);
  if (out_dtype == SEL_BF16)
    return launch_step<__bf16, __bf16>(a, p, vec, rt, nw, int(ncarry), carry, in, wpack, bias, res, out, carry_out, s);
  return launch_step<__bf16, float>(a, p, vec, rt, nw, int(ncarry), carry, in, wpack, bias, res, out, carry_out, s);
}

}  // namespace hfgstep
}  // namespace sel

extern "C" {

int sel_hfg_conv_step(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* carry, const void* in,
                      const void* wpack, const float* bias, const void* res, void* out, void* carry_out,
                      sel_stream_t stream) {
  return sel::hfgstep::hfg_conv_step("sel_hfg_conv_step", d, in_dtype, out_dtype, nullptr, carry, in, wpack, bias,
                                     res, out, carry_out, stream);
}

int sel_hfg_conv_step_pool(const sel_hfg_conv_desc* d, int in_dtype, int out_dtype, const void* carry,
                           void* carry_out, int nslots, const int32_t* slots, const int32_t* n_active,
                           const void* in, const void* wpack, const float* bias, const void* res, void* out,
                           sel_stream_t stream) {
  sel::hfgstep::PoolArgs p{slots, n_active, nslots, 0};
  return sel::hfgstep::hfg_conv_step("sel_hfg_conv_step_pool", d, in_dtype, out_dtype, &p, carry, in, wpack, bias,
                                     res, out, carry_out, stream);
}

}  // extern "C"
