// Streaming step primitive (sel_conv_step), the carry commit (sel_stream_commit)
// and their slot-indexed forms for stream pools (sel_conv_step_pool,
// sel_stream_copy_slots).
//
// A streaming hop runs every causal layer on a few rows (300, 100, 25, 5, 1 at
// B = 1 with a 300-sample hop): each weight element is used once per launch, so
// the kernel streams the packed weights Wp[N][K*C] as 16-byte vectors straight
// into MFMA B operands (no LDS staging: there is no second row tile to reuse
// them) and gathers the A operand from the virtual input [carry | act(in)].
//
//   block      = 16 output channels x RT row tiles of 16 rows, NW waves
//   wave w     = reduction chunks w, w + NW, ... of the flat K*C axis
//                (32 elements per bf16 MFMA, 16 per four fp32 MFMAs)
//   reduction  = every wave's 16 x 16 fp32 accumulator goes to LDS and is
//                summed in wave order 0, 1, ..., NW - 1: no atomics, and NW
//                depends on K*C alone, so an output's bits do not depend on B,
//                T or the row-tile count
//   carry_out  = written by extra blocks of the same launch (the last P rows of
//                the virtual input, the same act() on the new rows)
#include "step_common.h"

#include <algorithm>

namespace sel {
namespace stream {
using namespace sel::step;

constexpr int COMMIT_MAXJ = 48;

struct StepArgs {
  int64_t rows;
  int T, C, N, K, dil, P, in_elu, bias_period;
  int KC, nchunk, ncol, ngrp;
  int64_t carry_elems;  // B * P * C
};

// the activation of the new rows: one function for the conv operand and for
// carry_out, so the carried rows are the bits the conv consumed
__device__ __forceinline__ float act1(float v) { return elu(v); }
__device__ __forceinline__ __bf16 act1(__bf16 v) { return __bf16(elu_fast(float(v))); }

// element (vrow, c) of sample b's virtual input [carry (P rows) | act(in) (T rows)];
// bc is the sample's row of the carry: b itself, or its slot in a pool
template <typename TI>
__device__ __forceinline__ TI virt(const StepArgs& a, const TI* __restrict__ carry, const TI* __restrict__ in, int bc,
                                   int b, int vrow, int c) {
  if (vrow < a.P) return carry[(int64_t(bc) * a.P + vrow) * a.C + c];
  const TI v = in[(int64_t(b) * a.T + (vrow - a.P)) * a.C + c];
  return a.in_elu ? act1(v) : v;
}

template <typename TI, bool VEC>
__device__ __forceinline__ typename Frag<TI>::type load_a(const StepArgs& a, const TI* __restrict__ carry,
                                                          const TI* __restrict__ in, bool ok, int bc, int b, int t,
                                                          int r0) {
  typedef typename Frag<TI>::type F;
  constexpr int E = Frag<TI>::E;
  F f;
#pragma unroll
  for (int i = 0; i < E; ++i) f[i] = TI(0.f);
  if (!ok) return f;
  if constexpr (VEC) {
    if (r0 < a.KC) {   // C % 8 == 0: the E elements share one tap
      const int k = r0 / a.C, c = r0 - k * a.C;
      const int vrow = t + k * a.dil;
      if (vrow < a.P) {
        f = *reinterpret_cast<const F*>(carry + (int64_t(bc) * a.P + vrow) * a.C + c);
      } else {
        f = *reinterpret_cast<const F*>(in + (int64_t(b) * a.T + (vrow - a.P)) * a.C + c);
        if (a.in_elu) {
#pragma unroll
          for (int i = 0; i < E; ++i) f[i] = act1(f[i]);
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int r = r0 + i;
      if (r < a.KC) {
        const int k = r / a.C, c = r - k * a.C;
        f[i] = virt(a, carry, in, bc, b, t + k * a.dil, c);
      }
    }
  }
  return f;
}

template <typename TI, bool VEC>
__device__ __forceinline__ typename Frag<TI>::type load_b(const StepArgs& a, const TI* __restrict__ wp, int n, int r0) {
  typedef typename Frag<TI>::type F;
  constexpr int E = Frag<TI>::E;
  F f;
#pragma unroll
  for (int i = 0; i < E; ++i) f[i] = TI(0.f);
  if (n >= a.N) return f;
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

// POOL = false is sel_conv_step (p unused); POOL = true adds the slot table and
// the per-tick row count, everything else is shared so the two give the same bits
template <typename TI, typename TO, bool VEC, int RT, bool POOL>
__device__ __forceinline__ void conv_step_body(const Launch& lc, const StepArgs& a, const PoolArgs& p,
                                               const TI* __restrict__ carry, const TI* __restrict__ in,
                                               const TI* __restrict__ wp, const float* __restrict__ bias,
                                               const TO* __restrict__ res, TO* __restrict__ out,
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
    // carry_out[b][j] = v[b][T + j]: old carry rows while T + j < P, then the new rows
    const int64_t stride = int64_t(lc.nblk - nconv) * lc.bdim;
    const int64_t pc = int64_t(a.P) * a.C;
    if constexpr (POOL) {
      const int64_t live = int64_t(nact) * pc;   // the active samples' elements; blocks past them do nothing
      for (int64_t e = int64_t(lc.bid - nconv) * lc.bdim + tid; e < live; e += stride) {
        const int b = int(e / pc);
        const int rem = int(e - int64_t(b) * pc);
        const int j = rem / a.C, c = rem - j * a.C;
        const int slot = p.slots[b];
        if (pool_slot_ok(p, slot)) carry_out[int64_t(slot) * pc + rem] = virt(a, carry, in, slot, b, a.T + j, c);
      }
    } else {
      for (int64_t e = int64_t(lc.bid - nconv) * lc.bdim + tid; e < a.carry_elems; e += stride) {
        const int b = int(e / pc);
        const int rem = int(e - int64_t(b) * pc);
        const int j = rem / a.C, c = rem - j * a.C;
        carry_out[e] = virt(a, carry, in, b, b, a.T + j, c);
      }
    }
    return;
  }
  const int NW = lc.bdim >> 6;
  const int lane = tid & 63, w = tid >> 6;
  const int col = int(lc.bid) % a.ncol, grp = int(lc.bid) / a.ncol;
  const int n = col * 16 + (lane & 15);
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
      for (int rt = 0; rt < RT; ++rt) fa[u][rt] = load_a<TI, VEC>(a, carry, in, ok[rt], sc[rt], sb[rt], st[rt], r0);
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
    const int nn = col * 16 + (l & 15);
    bool live = m < rows && nn < a.N;
    if constexpr (POOL) {
      if (live) live = pool_slot_ok(p, p.slots[int(m / a.T)]);
    }
    if (live) {
      if (a.bias_period > 0) s += bias[nn % a.bias_period];
      if (res) s += to_f(res[m * a.N + nn]);
      out[m * a.N + nn] = from_f<TO>(s);
    }
  }
}

template <typename TI, typename TO, bool VEC, int RT>
__global__ void __launch_bounds__(MAX_NW * 64)
k_conv_step(StepArgs a, const TI* __restrict__ carry, const TI* __restrict__ in, const TI* __restrict__ wp,
            const float* __restrict__ bias, const TO* __restrict__ res, TO* __restrict__ out,
            TI* __restrict__ carry_out) {
  const Launch lc{blockIdx.x, gridDim.x, threadIdx.x, blockDim.x};
  conv_step_body<TI, TO, VEC, RT, false>(lc, a, PoolArgs{}, carry, in, wp, bias, res, out, carry_out);
}

template <typename TI, typename TO, bool VEC, int RT>
__global__ void __launch_bounds__(MAX_NW * 64)
k_conv_step_pool(StepArgs a, PoolArgs p, const TI* __restrict__ carry, const TI* __restrict__ in,
                 const TI* __restrict__ wp, const float* __restrict__ bias, const TO* __restrict__ res,
                 TO* __restrict__ out, TI* __restrict__ carry_out) {
  const Launch lc{blockIdx.x, gridDim.x, threadIdx.x, blockDim.x};
  conv_step_body<TI, TO, VEC, RT, true>(lc, a, p, carry, in, wp, bias, res, out, carry_out);
}

struct CopyJobs {
  int n;
  sel_copy_job j[COMMIT_MAXJ];
};

__global__ void __launch_bounds__(256) k_stream_commit(CopyJobs js) {
  const sel_copy_job J = js.j[blockIdx.y];
  const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const char* src = static_cast<const char*>(J.src);
  char* dst = static_cast<char*>(J.dst);
  int64_t done = 0;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const int64_t n16 = J.bytes >> 4;
    for (int64_t i = g; i < n16; i += stride)
      reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    done = n16 << 4;
  }
  for (int64_t i = done + g; i < J.bytes; i += stride) dst[i] = src[i];
}

// slot row src_slots[i] of every job's src -> slot row dst_slots[i] of its dst,
// i < min(*n, cap); grid = (blocks over a row, jobs, list entries)
struct SlotJobs {
  int n, cap, nslots;
  const int* src_slots;
  const int* dst_slots;
  const int* count;
  sel_copy_job j[COMMIT_MAXJ];
};

__global__ void __launch_bounds__(256) k_stream_copy_slots(SlotJobs js) {
  const int live = min(max(*js.count, 0), js.cap);
  const sel_copy_job J = js.j[blockIdx.y];
  const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int i = int(blockIdx.z); i < live; i += int(gridDim.z)) {
    const int ss = js.src_slots[i], ds = js.dst_slots[i];
    if (unsigned(ss) >= unsigned(js.nslots) || unsigned(ds) >= unsigned(js.nslots)) continue;
    const char* src = static_cast<const char*>(J.src) + int64_t(ss) * J.bytes;
    char* dst = static_cast<char*>(J.dst) + int64_t(ds) * J.bytes;
    int64_t done = 0;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
      const int64_t n16 = J.bytes >> 4;
      for (int64_t e = g; e < n16; e += stride)
        reinterpret_cast<uint4*>(dst)[e] = reinterpret_cast<const uint4*>(src)[e];
      done = n16 << 4;
    }
    for (int64_t e = done + g; e < J.bytes; e += stride) dst[e] = src[e];
  }
}

template <typename TI, typename TO>
int launch_step(const StepArgs& a, const PoolArgs* p, bool vec, int rt, int nw, int ncarry, const void* carry,
                const void* in, const void* wp, const float* bias, const void* res, void* out, void* carry_out,
                hipStream_t s) {
  const dim3 grid(unsigned(a.ncol * a.ngrp + ncarry)), block(unsigned(nw * 64));
  const size_t lds = size_t(nw) * rt * 256 * sizeof(float);
#define SEL_STEP_LAUNCH(V, R)                                                                                     \
  do {                                                                                                            \
    if (p)                                                                                                        \
      hipLaunchKernelGGL((k_conv_step_pool<TI, TO, V, R>), grid, block, lds, s, a, *p,                            \
                         static_cast<const TI*>(carry), static_cast<const TI*>(in), static_cast<const TI*>(wp),   \
                         bias, static_cast<const TO*>(res), static_cast<TO*>(out), static_cast<TI*>(carry_out)); \
    else                                                                                                          \
      hipLaunchKernelGGL((k_conv_step<TI, TO, V, R>), grid, block, lds, s, a, static_cast<const TI*>(carry),      \
                         static_cast<const TI*>(in), static_cast<const TI*>(wp), bias,                            \
                         static_cast<const TO*>(res), static_cast<TO*>(out), static_cast<TI*>(carry_out));       \
  } while (0)
  if (vec && rt == 1) SEL_STEP_LAUNCH(true, 1);
  else if (vec) SEL_STEP_LAUNCH(true, BIG_RT);
  else if (rt == 1) SEL_STEP_LAUNCH(false, 1);
  else SEL_STEP_LAUNCH(false, BIG_RT);
#undef SEL_STEP_LAUNCH
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// sel_conv_step (p == nullptr) and sel_conv_step_pool share the validation and the geometry
int conv_step(const char* fn, const sel_conv_desc* d, int in_dtype, int out_dtype, const PoolArgs* pool,
              const void* carry, const void* in, const void* wpack, const float* bias, const void* res, void* out,
              void* carry_out, sel_stream_t stream) {
  SEL_REQUIRE(d, SEL_ERR_ARG, "%s: null descriptor", fn);
  SEL_REQUIRE(d->rows > 0 && d->T > 0 && d->C > 0 && d->N > 0 && d->K > 0 && d->dil > 0, SEL_ERR_ARG,
              "%s: rows, T, C, N, K and dil must be positive", fn);
  SEL_REQUIRE(d->rows % d->T == 0, SEL_ERR_ARG, "%s: rows (%lld) is not a multiple of T (%d)", fn,
              (long long)d->rows, d->T);
  const int64_t P64 = int64_t(d->K - 1) * d->dil;
  SEL_REQUIRE(d->pad == P64, SEL_ERR_ARG, "%s: pad (%d) must be (K-1)*dil = %lld: the carry is the pad", fn, d->pad,
              (long long)P64);
  SEL_REQUIRE(d->pad_mode == SEL_PAD_ZERO, SEL_ERR_ARG, "%s: pad_mode must be SEL_PAD_ZERO", fn);
  SEL_REQUIRE(d->bias_period >= 0, SEL_ERR_ARG, "%s: negative bias_period", fn);
  SEL_REQUIRE((in_dtype == SEL_F32 && out_dtype == SEL_F32) || (in_dtype == SEL_BF16 && (out_dtype == SEL_BF16 || out_dtype == SEL_F32)),
              SEL_ERR_ARG, "%s: dtypes must be fp32 -> fp32 or bf16 -> bf16 / fp32", fn);
  const int64_t B = d->rows / d->T;
  const int64_t KC = int64_t(d->K) * d->C;
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
    SEL_REQUIRE(carry && carry_out, SEL_ERR_ARG, "%s: K > 1 needs carry and carry_out (%d rows per sample)", fn, P);
    SEL_REQUIRE(carry != carry_out, SEL_ERR_ARG, "%s: carry_out must not alias carry", fn);
    SEL_REQUIRE(carry_out != in && static_cast<const void*>(out) != carry && out != carry_out, SEL_ERR_ARG,
                "%s: carry_out / out alias an input", fn);
  }
  SEL_REQUIRE(static_cast<const void*>(out) != in && out != res, SEL_ERR_ARG, "%s: out aliases in / res", fn);

  const int es = in_dtype == SEL_BF16 ? 2 : 4;
  const int E = 16 / es;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // fast path: 16-byte operand loads (every row start and tap start 16-byte aligned)
  const bool vec = d->C % 8 == 0 && al16(in) && al16(wpack) && (P == 0 || al16(carry));
  StepArgs a{};
  a.rows = d->rows; a.T = d->T; a.C = d->C; a.N = d->N; a.K = d->K; a.dil = d->dil; a.P = P;
  a.in_elu = d->in_elu ? 1 : 0; a.bias_period = d->bias_period;
  a.KC = int(KC);
  a.nchunk = int((KC + 4 * E - 1) / (4 * E));
  a.ncol = (d->N + 15) / 16;
  a.carry_elems = B * P * d->C;
  // the reduction split depends on the layer shape alone (bit-identical outputs for any B, T)
  const int nw = std::min(MAX_NW, std::max(1, a.nchunk / 4));
  const int64_t ntile = (d->rows + 15) / 16;
  const int rt = ntile >= RT_SWITCH ? BIG_RT : 1;
  const int64_t ngrp = (ntile + rt - 1) / rt;
  const int64_t per_blk = int64_t(nw) * 64;
  const int64_t ncarry = P > 0 ? std::min<int64_t>(64, (a.carry_elems + per_blk - 1) / per_blk) : 0;
  SEL_REQUIRE(ngrp * a.ncol + ncarry < (int64_t(1) << 31), SEL_ERR_ARG, "%s: too many tiles", fn);
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
    return launch_step<__bf16, __bf16>(a, p, vec, rt, nw, int(ncarry), carry, in, wpack, bias, res, out, carry_out,
                                       s);
  return launch_step<__bf16, float>(a, p, vec, rt, nw, int(ncarry), carry, in, wpack, bias, res, out, carry_out, s);
}

}  // namespace stream
}  // namespace sel

extern "C" {

int sel_conv_step(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* carry, const void* in,
                  const void* wpack, const float* bias, const void* res, void* out, void* carry_out,
                  sel_stream_t stream) {
  return sel::stream::conv_step("sel_conv_step", d, in_dtype, out_dtype, nullptr, carry, in, wpack, bias, res, out,
                                carry_out, stream);
}

int sel_conv_step_pool(const sel_conv_desc* d, int in_dtype, int out_dtype, const void* carry, void* carry_out,
                       int nslots, const int32_t* slots, const int32_t* n_active, const void* in, const void* wpack,
                       const float* bias, const void* res, void* out, sel_stream_t stream) {
  sel::stream::PoolArgs p{slots, n_active, nslots, 0};
  return sel::stream::conv_step("sel_conv_step_pool", d, in_dtype, out_dtype, &p, carry, in, wpack, bias, res, out,
                                carry_out, stream);
}

int sel_stream_commit(const sel_copy_job* jobs, int njobs, sel_stream_t stream) {
  using namespace sel::stream;
  SEL_REQUIRE(jobs && njobs > 0, SEL_ERR_ARG, "sel_stream_commit: empty job table");
  for (int j = 0; j < njobs; ++j)
    SEL_REQUIRE(jobs[j].src && jobs[j].dst && jobs[j].bytes > 0 && jobs[j].src != jobs[j].dst, SEL_ERR_ARG,
                "sel_stream_commit: job %d needs distinct non-null src / dst and bytes > 0", j);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += COMMIT_MAXJ) {
    CopyJobs cj{};
    cj.n = std::min(COMMIT_MAXJ, njobs - j0);
    int64_t most = 0;
    for (int j = 0; j < cj.n; ++j) {
      cj.j[j] = jobs[j0 + j];
      most = std::max(most, cj.j[j].bytes);
    }
    const unsigned bx = unsigned(std::min<int64_t>(32, std::max<int64_t>(1, (most / 16 + 255) / 256)));
    hipLaunchKernelGGL(k_stream_commit, dim3(bx, unsigned(cj.n)), dim3(256), 0, s, cj);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

int sel_stream_copy_slots(const sel_copy_job* jobs, int njobs, int nslots, const int32_t* src_slots,
                          const int32_t* dst_slots, int cap, const int32_t* n, sel_stream_t stream) {
  using namespace sel::stream;
  SEL_REQUIRE(jobs && njobs > 0, SEL_ERR_ARG, "sel_stream_copy_slots: empty job table");
  SEL_REQUIRE(src_slots && dst_slots && n, SEL_ERR_ARG, "sel_stream_copy_slots: null src_slots / dst_slots / n");
  SEL_REQUIRE(nslots > 0 && nslots < (1 << 24) && cap > 0 && cap < (1 << 24), SEL_ERR_ARG,
              "sel_stream_copy_slots: nslots (%d) and cap (%d) must be positive", nslots, cap);
  for (int j = 0; j < njobs; ++j)
    SEL_REQUIRE(jobs[j].src && jobs[j].dst && jobs[j].bytes > 0 && jobs[j].bytes < (int64_t(1) << 32), SEL_ERR_ARG,
                "sel_stream_copy_slots: job %d needs non-null src / dst and 0 < bytes per slot < 2^32", j);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += COMMIT_MAXJ) {
    SlotJobs sj{};
    sj.n = std::min(COMMIT_MAXJ, njobs - j0);
    sj.cap = cap; sj.nslots = nslots;
    sj.src_slots = src_slots; sj.dst_slots = dst_slots; sj.count = n;
    int64_t most = 0;
    for (int j = 0; j < sj.n; ++j) {
      sj.j[j] = jobs[j0 + j];
      most = std::max(most, sj.j[j].bytes);
    }
    const unsigned bx = unsigned(std::min<int64_t>(8, std::max<int64_t>(1, (most / 16 + 255) / 256)));
    hipLaunchKernelGGL(k_stream_copy_slots, dim3(bx, unsigned(sj.n), unsigned(std::min(cap, 256))), dim3(256), 0, s,
                       sj);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

}  // extern "C"
