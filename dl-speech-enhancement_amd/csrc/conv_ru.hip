// Fused residual-unit kernels of the conv stack (residual_unit.py:43-46:
// conv1 = causal k7 dilated C -> C behind an ELU, conv2 = 1x1 C -> C behind an
// ELU, out = x + conv2(ELU(conv1(ELU(x))))), one launch per unit and direction
// instead of two launches of the primitive (conv.hip):
//   forward            k_ru32_fwd, k_ru32_fwd4, k_ru64_fwd, k_ru_thin_bf16
//   backward           k_ru32_bwd, k_ru64_bwd
//   backward + wgrads  k_ru32_bwdw, k_ru64_bwdw (the encoder's units)
// with their launchers and the sel_resunit_* entry points.  Same MFMA order,
// bf16 rounding points and epilogue arithmetic as the two-launch path, so the
// results are bit-identical to it.  The 128-channel forward runs on the
// sample-tile kernel (conv_wss.hip: launch_wss_pw).
#include <algorithm>

#include "conv_tile.h"

namespace sel {
namespace conv {

// residual-unit kernels' occupancy targets (waves per SIMD the register
// allocation must allow)
#ifndef SEL_W_RU32F
#define SEL_W_RU32F 3
#endif
#ifndef SEL_W_RU32F128
#define SEL_W_RU32F128 4
#endif
#ifndef SEL_W_RU32B
#define SEL_W_RU32B 3
#endif
#ifndef SEL_W_RU32W
#define SEL_W_RU32W 2
#endif
#ifndef SEL_W_RU64F
#define SEL_W_RU64F 2
#endif
#ifndef SEL_W_RU64B
#define SEL_W_RU64B 2
#endif

// ---------------------------------------------------------------------------
// Fused residual-unit forward for the thin layers (residual_unit.py:43-46 with
// conv1 = causal K-tap dilated C->C, conv2 = 1x1 C->C, no bias in AudioDec):
//   h   = conv1(ELU(x))                       -> HBM (saved for the backward)
//   out = x + conv2(ELU(h))                   -> HBM
// One pass over the tile: conv1 as in k_conv_thin_bf16 (weights in VGPRs,
// ELU at staging), its accumulators -> fp32 tile in LDS -> coalesced h store
// AND ELU(bf16(h)) staged straight into a second LDS tile that feeds conv2's
// MFMAs (its weights also in VGPRs); the residual is re-read from L2 in the
// final coalesced epilogue.  vs. two primitive calls this drops the h re-read
// and one x re-read from HBM (5 -> 3 activation-sized tensors per unit).
// ---------------------------------------------------------------------------
template <int C, int K, int R>
struct RuThin {
  using G = Thin<C, C, K, R>;
  static constexpr size_t LDS_HS = size_t(G::PLANES) * R * F4_P * 2;
  static constexpr size_t LDS = G::LDS + LDS_HS;
  static_assert(LDS <= 64 * 1024, "fused residual unit LDS");
};

template <int C, int K, int R>
__global__ __launch_bounds__(256) void k_ru_thin_bf16(Args a, const __bf16* __restrict__ in,
                                                      const __bf16* __restrict__ w1p, const float* __restrict__ b1,
                                                      const __bf16* __restrict__ w2p, const float* __restrict__ b2,
                                                      __bf16* __restrict__ hout, __bf16* __restrict__ out,
                                                      int tiles_per_block) {
  using G = Thin<C, C, K, R>;
  constexpr int P = F4_P;
  constexpr int CV = G::CV;
  constexpr int N = C;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);                   // [PLANES][SPAN][P]
  float* const ot = reinterpret_cast<float*>(smem);                     // [R][OP], aliases xs
  __bf16* const hs = reinterpret_cast<__bf16*>(smem + G::LDS);          // [PLANES][R][P]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ns = wave % G::NS, rg = wave / G::NS;
  const int span = R + (K - 1) * a.dil;
  const int tps = (a.T + R - 1) / R;
  const int64_t ntiles = (a.rows / a.T) * tps;
  const int64_t vb = int64_t(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
  const int64_t tile0 = vb * tiles_per_block;
  const int64_t tile_end = tile0 + tiles_per_block < ntiles ? tile0 + tiles_per_block : ntiles;
  if (tile0 >= tile_end) return;  // block-uniform

  bf16x8 wf[K][C / 16], wf2[C / 16];
  {
    const __bf16* wrow = w1p + int64_t(ns * 32 + (lane & 31)) * K * C + 8 * (lane >> 5);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int g = 0; g < C / 16; ++g) wf[k][g] = *reinterpret_cast<const bf16x8*>(wrow + k * C + 16 * g);
    const __bf16* wrow2 = w2p + int64_t(ns * 32 + (lane & 31)) * C + 8 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < C / 16; ++g) wf2[g] = *reinterpret_cast<const bf16x8*>(wrow2 + 16 * g);
  }

  uint4 xr[G::XV];
  bool xok[G::XV];
  auto load = [&](int64_t tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      int ti = t0 - a.pad + r;
      xok[u] = r < span && ti >= 0 && ti < a.T;
      ti = ti < 0 ? 0 : (ti >= a.T ? a.T - 1 : ti);
      if ((u * 256) / CV < span) xr[u] = *reinterpret_cast<const uint4*>(in + (b * a.T + ti) * C + c);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      if (r >= span) continue;
      uint4 val = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
      val = elu8(val);
      *reinterpret_cast<uint4*>(xs + ((c >> 5) * G::SPAN + r) * P + (c & 31)) = val;
    }
  };
  // accumulators (out^T: lane -> row, element -> channel) -> fp32 tile in LDS
  auto acc_to_ot = [&](const floatx16 (&acc)[G::TM]) {
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
  };
  constexpr int GN = N / 8;

  load(tile0);
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    __syncthreads();  // the previous tile's epilogue is done with ot (= xs)
    store();
    __syncthreads();
    if (tile + 1 < tile_end) load(tile + 1);
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    const int64_t obase = (b * a.T + t0) * N;

    // conv1
    floatx16 acc[G::TM];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    {
      const __bf16* xw = xs + (rg * G::WR + (lane & 31)) * P + 8 * (lane >> 5);
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int g = 0; g < C / 16; ++g) {
          const __bf16* xb = xw + ((g >> 1) * G::SPAN + k * a.dil) * P + 16 * (g & 1);
#pragma unroll
          for (int i = 0; i < G::TM; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][g], *reinterpret_cast<const bf16x8*>(xb + i * 32 * P),
                                                             acc[i], 0, 0, 0);
        }
    }
    __syncthreads();  // every wave is done reading xs
    acc_to_ot(acc);
    __syncthreads();
    // h epilogue: + b1, store h (bf16), stage ELU(h) for conv2
    for (int idx = tid; idx < R * GN; idx += 256) {
      const int r = idx / GN, n = (idx % GN) * 8;
      const floatx4 lo = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n);
      const floatx4 hi = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (b1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b1[n + e];
      }
      uint4 hv, ev;
      __bf16* hp = reinterpret_cast<__bf16*>(&hv);
      __bf16* ep = reinterpret_cast<__bf16*>(&ev);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        hp[e] = __bf16(v[e]);
        ep[e] = __bf16(elu_fast(float(hp[e])));
      }
      if (r < mrows) *reinterpret_cast<uint4*>(hout + obase + int64_t(r) * N + n) = hv;
      *reinterpret_cast<uint4*>(hs + ((n >> 5) * R + r) * P + (n & 31)) = ev;
    }
    __syncthreads();
    // conv2 (1x1)
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    {
      const __bf16* hw = hs + (rg * G::WR + (lane & 31)) * P + 8 * (lane >> 5);
#pragma unroll
      for (int g = 0; g < C / 16; ++g) {
        const __bf16* hb = hw + (g >> 1) * R * P + 16 * (g & 1);
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf2[g], *reinterpret_cast<const bf16x8*>(hb + i * 32 * P),
                                                           acc[i], 0, 0, 0);
      }
    }
    acc_to_ot(acc);  // ot is free: the h epilogue read it before the last barrier
    __syncthreads();
    for (int idx = tid; idx < mrows * GN; idx += 256) {
      const int r = idx / GN, n = (idx % GN) * 8;
      const floatx4 lo = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n);
      const floatx4 hi = *reinterpret_cast<const floatx4*>(ot + r * G::OP + n + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (b2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b2[n + e];
      }
      const int64_t o = obase + int64_t(r) * N + n;
      uint4 raw = *reinterpret_cast<const uint4*>(in + o);
      const __bf16* rv = reinterpret_cast<const __bf16*>(&raw);
      uint4 ov;
      __bf16* op = reinterpret_cast<__bf16*>(&ov);
#pragma unroll
      for (int e = 0; e < 8; ++e) op[e] = __bf16(v[e] + float(rv[e]));
      *reinterpret_cast<uint4*>(out + o) = ov;
    }
  }
}

// ---------------------------------------------------------------------------
// Residual unit at 32 channels, forward and backward in ONE launch each, with
// the 1x1 conv done in registers (residual_unit.py:43-46; conv1 = causal k7
// dilated 32 -> 32, conv2 = 1x1 32 -> 32, both with bias in AudioDec).
//
// A wave owns 32-row sub-tiles of a sample-aligned R-row tile and all 32
// channels of them.  conv1's accumulators (lane -> row, element e -> channel
// (e & 3) + 8 (e >> 2) + 4 (lane >> 5)) are packed to bf16 and re-laid out with
// two v_permlane32_swap per channel-group pair into 8-consecutive-channel
// vectors: exactly the B operand of the next 32x32x16 MFMA AND one 16-B
// store.  So h goes to HBM (saved for the backward) and ELU(h) straight into
// conv2's MFMAs without an LDS round trip or a block barrier; the only shared
// stage is the input tile with its causal halo.  HBM per row: forward reads x
// and writes h, out (3 tensors instead of 5 over two launches); backward
// reads g (grad of out), h, x and writes gx (+ gh for the weight gradient):
// 4-5 tensors instead of 7 over two launches.
//
// Same MFMA order, same bf16 rounding points and the same epilogue arithmetic
// as the two-launch primitive path, so the results are bit-identical to it
// (test_gpu_conv.py::test_resunit32_*).
// ---------------------------------------------------------------------------
constexpr int RU_C = 32, RU_K = 7;

// Global stores of the fused residual-unit kernels' outputs (h, out, gh, gx:
// written once, read by a later launch).  SEL_RU_NT=1 builds them as streaming
// (non-temporal) stores, the |X| kernel's lever (A/B library: make nt).
#ifndef SEL_RU_NT
#define SEL_RU_NT 0
#endif
__device__ __forceinline__ void ru_store(__bf16* p, bf16x8 v) {
  if constexpr (SEL_RU_NT) __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v), reinterpret_cast<u32x4*>(p));
  else *reinterpret_cast<bf16x8*>(p) = v;
}

// Cache policy of the buffer stores (ru_bstore's AUX; 2 = nt).  Judged inside the
// profiled step (tools/ru_bench.py re-reads its own inputs, which favours
// anything that keeps them cached): nt pays on k_ru32_fwd's h rows (read
// again only by the backward), and loses on outputs the next kernel reads
// (k_ru32_bwd's gx) or on rows two waves write in halves (k_ru64_fwd's h)
// k_ru32_fwd's h rows (read again only by the backward, much later) leave as
// nt stores: 71.7-72.5 -> 69.1-69.5 us per unit inside the profiled C3 step;
// nt on both h and out measured 1.5-2x slower, nt on out alone neutral
// (A/B builds: SEL_RU_FWD_*NT)
#ifndef SEL_RU_FWD_HNT
#define SEL_RU_FWD_HNT 2
#endif
#ifndef SEL_RU_FWD_ONT
#define SEL_RU_FWD_ONT 0
#endif
// k_ru32_bwd's gx rows: plain stores.  nt measured 86 -> 79 us per unit in
// tools/ru_bench.py but 87.4-88.0 -> 90.8-91.0 us inside the profiled C3 step
// (the next layer's backward reads gx right away); A/B builds: SEL_RU32B_GXNT=2
#ifndef SEL_RU32B_GXNT
#define SEL_RU32B_GXNT 0
#endif

// N dropped stores (a zero-byte region; distinct offsets so that the compiler
// keeps them apart) after a tile loop's first prefetch: the loop issues N
// output stores after each later prefetch, so both paths into the staging
// waits carry the same count and the compiler leaves those stores pending
template <int N>
__device__ __forceinline__ void ru_dummy_stores(const __bf16* base) {
  const __amdgpu_buffer_rsrc_t rz = ru_rsrc(base, 0);
  const bf16x8 z = {};
#pragma unroll
  for (int i = 0; i < N; ++i) ru_bstore(rz, 16 * i, z);
}

// acc (one 32x32 MFMA result) -> bf16, re-laid out: frag[kc] = channels
// 16 kc + 8 (lane >> 5) .. +8 of this lane's row (T21 of the HIP guide)
__device__ __forceinline__ void ru_acc_to_frags(const float (&v)[16], bf16x8 (&frag)[2]) {
  unsigned pk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
    pk[q] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{v[2 * q], v[2 * q + 1]}), bf16x2));
  // group g = elements 4g..4g+3 = pk[2g], pk[2g+1]; swap pairs (0,1) and (2,3)
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    unsigned a0 = pk[4 * pr], a1 = pk[4 * pr + 1], b0 = pk[4 * pr + 2], b1 = pk[4 * pr + 3];
    const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 w = {r0[0], r1[0], r0[1], r1[1]};
    frag[pr] = __builtin_bit_cast(bf16x8, w);
  }
}

template <int R>
struct Ru32 {
  static constexpr int P = F4_P;
  static constexpr int SPAN = R + F4_HALOMAX;   // staged rows (tile + max halo)
  static constexpr int XV = (SPAN * 4 + 255) / 256;
  static constexpr int TM = R / 128;            // 32-row sub-tiles per wave
  static constexpr size_t LDS_FWD = size_t(SPAN + R) * P * 2;  // ELU(x) span + raw tile rows
  static constexpr size_t LDS_BWD = 3 * size_t(SPAN) * P * 2;  // g, gh and h tiles
  static_assert(R % 128 == 0, "ru32 tile rows");
};

// stage `span` rows of a 32-channel tensor starting at sample row t0 + off
// (rows outside [0, T) -> zero) into registers / LDS (optionally ELU'd)
template <int R>
struct Ru32Stage {
  uint4 r[Ru32<R>::XV];
  bool ok[Ru32<R>::XV];
  // Buffer loads over sample b: rows outside [0, T), past the span or of a
  // dead request (live = false: no next tile) take an out-of-range offset and
  // return zeros without touching memory.  No branch around any load, so the
  // compiler counts this request exactly and later waits in the tile loop do
  // not fall back to vmcnt(0) behind it.
  __device__ __forceinline__ void load(const Args& a, const __bf16* __restrict__ src, int64_t b, int t0, int off,
                                       int span, bool live = true) {
    const __amdgpu_buffer_rsrc_t rs = ru_rsrc(src + b * a.T * RU_C, a.T * RU_C);
#pragma unroll
    for (int u = 0; u < Ru32<R>::XV; ++u) {
      const int v = threadIdx.x + u * 256;
      const int row = v >> 2, c = (v & 3) * 8;
      const int ti = t0 + off + row;
      ok[u] = row < span && ti >= 0 && ti < a.T;
      r[u] = ru_bload(rs, live && ok[u] ? (ti * RU_C + c) * 2 : RU_OOB);
      // program order pinned: the same order from the prologue and the tile
      // loop, so the staging waits count both paths into them exactly
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // raw != nullptr: rows [raw_off, raw_off + R) are also stored un-ELU'd into raw
  __device__ __forceinline__ void store(__bf16* xs, int span, bool elu, __bf16* raw = nullptr, int raw_off = 0,
                                        int pitch = F4_P) {
#pragma unroll
    for (int u = 0; u < Ru32<R>::XV; ++u) {
      const int v = threadIdx.x + u * 256;
      const int row = v >> 2, c = (v & 3) * 8;
      if (row >= span) continue;
      uint4 val = ok[u] ? r[u] : make_uint4(0, 0, 0, 0);
      if (raw && row >= raw_off && row < raw_off + R) *reinterpret_cast<uint4*>(raw + (row - raw_off) * F4_P + c) = val;
      if (elu) {
        val = elu8(val);
      }
      *reinterpret_cast<uint4*>(xs + row * pitch + c) = val;
    }
  }
};

// XCD-contiguous tile range of this block (as k_conv_thin_bf16)
__device__ __forceinline__ bool ru_tiles(int64_t ntiles, int tiles_per_block, int64_t& t_begin, int64_t& t_end) {
  const int64_t vb = int64_t(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
  t_begin = vb * tiles_per_block;
  t_end = t_begin + tiles_per_block < ntiles ? t_begin + tiles_per_block : ntiles;
  return t_begin < t_end;
}

// A fragments of a packed [32][K][32] weight (row n = lane & 31, channels 16 g + 8 (lane >> 5))
template <int K>
__device__ __forceinline__ void ru_wfrags(const __bf16* __restrict__ wp, bf16x8 (&wf)[K][2]) {
  const int lane = threadIdx.x & 63;
  const __bf16* wrow = wp + int64_t(lane & 31) * K * RU_C + 8 * (lane >> 5);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int g = 0; g < 2; ++g) wf[k][g] = *reinterpret_cast<const bf16x8*>(wrow + k * RU_C + 16 * g);
}

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R == 128 ? SEL_W_RU32F128 : SEL_W_RU32F))) void k_ru32_fwd(Args a, const __bf16* __restrict__ x,
                                                  const __bf16* __restrict__ w1p, const float* __restrict__ b1,
                                                  const __bf16* __restrict__ w2p, const float* __restrict__ b2,
                                                  __bf16* __restrict__ hout, __bf16* __restrict__ out,
                                                  int tiles_per_block, int dbg) {
  using G = Ru32<R>;
  constexpr int P = G::P;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);  // [SPAN][P]: ELU(x) rows t0 - pad ..
  __bf16* const xr = xs + G::SPAN * P;                 // [R][P]: raw x rows t0 .. (the residual)
  const int lane = threadIdx.x & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int span = R + a.pad;
  const int tps = (a.T + R - 1) / R;
  int64_t tile0, tile_end;
  if (!ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) return;

  bf16x8 wf[RU_K][2], w2f[1][2];
  ru_wfrags<RU_K>(w1p, wf);
  ru_wfrags<1>(w2p, w2f);
  ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads

  // both biases staged in LDS once (k_ru64_fwd)
  __shared__ __align__(16) float bsm[2][RU_C];
  if (threadIdx.x < 2 * RU_C) {
    const int i = threadIdx.x;
    const float* bp = i < RU_C ? b1 : b2;
    bsm[i / RU_C][i % RU_C] = bp ? bp[i % RU_C] : 0.f;
  }
  Ru32Stage<R> st;
  st.load(a, x, tile0 / tps, int(tile0 % tps) * R, -a.pad, span);
  ru_dummy_stores<4 * G::TM>(out);  // the loop's h / out stores after each prefetch
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    __syncthreads();  // every wave is done with the previous tile's rows
    st.store(xs, span, true, xr, a.pad);
    __syncthreads();
    {  // unconditional (a dead request loads nothing): exact counts
      const bool live = tile + 1 < tile_end;
      const int64_t nt = live ? tile + 1 : tile;
      st.load(a, x, nt / tps, int(nt % tps) * R, -a.pad, span, live);
    }
    // every sub-tile computes and stores (rows past T to RU_OOB): a fixed count
    // of stores per tile keeps the next tile's staging wait exact (ru_bstore)
    const __amdgpu_buffer_rsrc_t rh = ru_rsrc(hout + b * a.T * RU_C, int64_t(a.T) * RU_C);
    const __amdgpu_buffer_rsrc_t ro = ru_rsrc(out + b * a.T * RU_C, int64_t(a.T) * RU_C);
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = wave * (R / 4) + i * 32 + (lane & 31);  // this lane's row in the tile
      const bool valid = lr < mrows;
      const int off = ((t0 + lr) * RU_C + 8 * hl) * 2;
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const __bf16* xw = xs + lr * P + 8 * hl;
#pragma unroll
      for (int k = 0; k < RU_K; ++k)
#pragma unroll
        for (int g = 0; g < 2; ++g)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][g], *reinterpret_cast<const bf16x8*>(xw + k * a.dil * P + 16 * g),
                                                        acc, 0, 0, 0);
      // h = conv1 + b1 -> bf16 -> HBM, ELU(h) -> conv2
      // bias in accumulator order: element group q = channels 8 q + 4 hl .. +4
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 bq = *reinterpret_cast<const floatx4*>(&bsm[0][8 * q + 4 * hl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc[4 * q + e] + bq[e];
      }
      bf16x8 hf[2];
      ru_acc_to_frags(v, hf);
      const bool hst = valid && !(dbg & 1);  // tune key 15 bit 0: diagnostic without the h store
      ru_bstore<SEL_RU_FWD_HNT>(rh, hst ? off : RU_OOB, hf[0]);
      ru_bstore<SEL_RU_FWD_HNT>(rh, hst ? off + 32 : RU_OOB, hf[1]);
      floatx16 acc2;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const bf16x8 ef = __builtin_bit_cast(bf16x8, elu8(__builtin_bit_cast(uint4, hf[g])));
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[0][g], ef, acc2, 0, 0, 0);
      }
      // out = conv2 + b2 + x (the residual in accumulator order: 4 runs of 4 channels)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 xres = *reinterpret_cast<const uint2*>(xr + lr * P + 8 * q + 4 * hl);
        const __bf16* rv = reinterpret_cast<const __bf16*>(&xres);
        const floatx4 bq = *reinterpret_cast<const floatx4*>(&bsm[1][8 * q + 4 * hl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc2[4 * q + e] + bq[e] + float(rv[e]);
      }
      bf16x8 of[2];
      ru_acc_to_frags(v, of);
      const bool ost = valid && !(dbg & 2);  // bit 1: diagnostic without the out store
      ru_bstore<SEL_RU_FWD_ONT>(ro, ost ? off : RU_OOB, of[0]);
      ru_bstore<SEL_RU_FWD_ONT>(ro, ost ? off + 32 : RU_OOB, of[1]);
    }
  }
}

// k_ru32_fwd at four blocks per CU (tune key 70 = 1; round 6): the conv1
// weights live in LDS (one A-fragment ds_read_b128 per MFMA instead of 56
// VGPRs), ELU(x) rows are 64 B with their 16-B slots XOR-swizzled by
// (row >> 2) & 3 (the 16 rows of every ds_read_b128 lane group hit 16 distinct
// bank groups), and the residual rows are re-read from global memory (staged
// one tile earlier: L2-hot) instead of a raw LDS plane.  35 KB of LDS and at
// most 128 VGPRs: four blocks per CU instead of three keep a third more tiles'
// loads in flight.  Same operands, MFMA order and epilogue as k_ru32_fwd:
// bit-identical.
constexpr int RU4_WP = RU_K * RU_C + 8;  // bf16 pitch of a W1 row in LDS (464 B: conflict-free A reads)
__device__ __forceinline__ int ru4_swz(int row) { return (row >> 2) & 3; }

template <int R>
struct Ru32F4 {
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int TM = R / 128;
  static constexpr size_t LDS = size_t(SPAN) * RU_C * 2 + size_t(RU_C) * RU4_WP * 2;
};

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_ru32_fwd4(
    Args a, const __bf16* __restrict__ x, const __bf16* __restrict__ w1p, const float* __restrict__ b1,
    const __bf16* __restrict__ w2p, const float* __restrict__ b2, __bf16* __restrict__ hout,
    __bf16* __restrict__ out, int tiles_per_block) {
  using G = Ru32F4<R>;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);  // [SPAN][32]: ELU(x) rows t0 - pad .., swizzled slots
  __bf16* const wsm = xs + G::SPAN * RU_C;             // [32][RU4_WP]: W1 rows (packed [n][k][c])
  const int lane = threadIdx.x & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int span = R + a.pad;
  const int tps = (a.T + R - 1) / R;
  int64_t tile0, tile_end;
  if (!ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) return;

  for (int i = threadIdx.x; i < RU_C * RU_K * RU_C / 8; i += 256) {
    const int n = i / (RU_K * RU_C / 8), r = i % (RU_K * RU_C / 8);
    *reinterpret_cast<uint4*>(wsm + n * RU4_WP + 8 * r) =
        *reinterpret_cast<const uint4*>(w1p + int64_t(n) * RU_K * RU_C + 8 * r);
  }
  bf16x8 w2f[1][2];
  ru_wfrags<1>(w2p, w2f);
  ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads

  __shared__ __align__(16) float bsm[2][RU_C];
  if (threadIdx.x < 2 * RU_C) {
    const int i = threadIdx.x;
    const float* bp = i < RU_C ? b1 : b2;
    bsm[i / RU_C][i % RU_C] = bp ? bp[i % RU_C] : 0.f;
  }
  const __bf16* const wrow = wsm + (lane & 31) * RU4_WP + 8 * hl;
  Ru32Stage<R> st;
  st.load(a, x, tile0 / tps, int(tile0 % tps) * R, -a.pad, span);
  ru_dummy_stores<4 * G::TM>(out);  // the loop's h / out stores after each prefetch
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    __syncthreads();  // every wave is done with the previous tile's rows (and W1 / biases staged)
#pragma unroll
    for (int u = 0; u < Ru32<R>::XV; ++u) {
      const int v = threadIdx.x + u * 256;
      const int row = v >> 2, slot = v & 3;
      if (row >= span) continue;
      const uint4 val = elu8(st.ok[u] ? st.r[u] : make_uint4(0, 0, 0, 0));
      *reinterpret_cast<uint4*>(xs + row * RU_C + 8 * (slot ^ ru4_swz(row))) = val;
    }
    __syncthreads();
    {  // unconditional (a dead request loads nothing): exact counts
      const bool live = tile + 1 < tile_end;
      const int64_t nt = live ? tile + 1 : tile;
      st.load(a, x, nt / tps, int(nt % tps) * R, -a.pad, span, live);
    }
    const __amdgpu_buffer_rsrc_t rh = ru_rsrc(hout + b * a.T * RU_C, int64_t(a.T) * RU_C);
    const __amdgpu_buffer_rsrc_t ro = ru_rsrc(out + b * a.T * RU_C, int64_t(a.T) * RU_C);
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = wave * (R / 4) + i * 32 + (lane & 31);  // this lane's row in the tile
      const bool valid = lr < mrows;
      const int off = ((t0 + lr) * RU_C + 8 * hl) * 2;
      // the residual rows (raw x), requested before conv1: branch-free, clamped row
      const int64_t orow = (b * a.T + t0 + (valid ? lr : 0)) * RU_C;
      uint2 xres[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xres[q] = *reinterpret_cast<const uint2*>(x + orow + 8 * q + 4 * hl);
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int k = 0; k < RU_K; ++k) {
        const int row = lr + k * a.dil;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(wrow + k * RU_C + 16 * g);
          const bf16x8 bf = *reinterpret_cast<const bf16x8*>(xs + row * RU_C + 8 * ((2 * g + hl) ^ ru4_swz(row)));
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
        }
      }
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 bq = *reinterpret_cast<const floatx4*>(&bsm[0][8 * q + 4 * hl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc[4 * q + e] + bq[e];
      }
      bf16x8 hf[2];
      ru_acc_to_frags(v, hf);
      ru_bstore<SEL_RU_FWD_HNT>(rh, valid ? off : RU_OOB, hf[0]);
      ru_bstore<SEL_RU_FWD_HNT>(rh, valid ? off + 32 : RU_OOB, hf[1]);
      floatx16 acc2;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const bf16x8 ef = __builtin_bit_cast(bf16x8, elu8(__builtin_bit_cast(uint4, hf[g])));
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[0][g], ef, acc2, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const __bf16* rv = reinterpret_cast<const __bf16*>(&xres[q]);
        const floatx4 bq = *reinterpret_cast<const floatx4*>(&bsm[1][8 * q + 4 * hl]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc2[4 * q + e] + bq[e] + float(rv[e]);
      }
      bf16x8 of[2];
      ru_acc_to_frags(v, of);
      ru_bstore<SEL_RU_FWD_ONT>(ro, valid ? off : RU_OOB, of[0]);
      ru_bstore<SEL_RU_FWD_ONT>(ro, valid ? off + 32 : RU_OOB, of[1]);
    }
  }
}

// Residual unit at 64 channels, forward in ONE launch (round 3): the 32-channel
// scheme with the 1x1 still fed from registers, but a wave computes conv1 for
// one 32-channel output slice only (all 64 x 7 input fragments of its slice in
// VGPRs, as k_conv_thin_bf16), so the 1x1 (all 64 h channels of a row) needs
// the partner wave's slice: each wave writes ELU(bf16(h)) of its rows and slice
// to a [2][R][P] LDS tile in the 1x1's B-fragment order, one block barrier, and
// every wave reads its four fragments back.  Waves = 2 row groups x 2 slices.
// h and out leave from the re-laid-out fragments as 16-B stores; the residual
// rows (raw x) are requested before conv1 (L2-hot: the tile was just staged).
// Same MFMA order, rounding points and epilogue arithmetic as the two thin
// launches (k7 then 1x1), so the results are bit-identical to them.
template <int R>
struct Ru64 {
  static constexpr int C = 64, K = 7, P = F4_P;
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int CV = C / 8;
  static constexpr int XV = (SPAN * CV + 255) / 256;
  static constexpr int WR = R / 2;  // rows per row group
  static constexpr int TM = WR / 32;
  // ELU(x) span planes + ELU(h) planes + raw x tile planes (the residual)
  static constexpr size_t LDS = size_t(2) * (SPAN + 2 * R) * P * 2;
  static_assert(R % 64 == 0, "ru64 tile rows");
};

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SEL_W_RU64F))) void k_ru64_fwd(Args a, const __bf16* __restrict__ x,
                                                  const __bf16* __restrict__ w1p, const float* __restrict__ b1,
                                                  const __bf16* __restrict__ w2p, const float* __restrict__ b2,
                                                  __bf16* __restrict__ hout, __bf16* __restrict__ out,
                                                  int tiles_per_block) {
  using G = Ru64<R>;
  constexpr int P = G::P, C = G::C, K = G::K, CV = G::CV;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const xs = reinterpret_cast<__bf16*>(smem);  // [2][SPAN][P]: ELU(x) rows t0 - pad ..
  __bf16* const hs = xs + 2 * G::SPAN * P;             // [2][R][P]: ELU(h) rows t0 ..
  __bf16* const xraw = hs + 2 * R * P;                 // [2][R][P]: raw x rows t0 .. (the residual)
  const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ns = wave & 1, rg = wave >> 1;
  const int span = R + a.pad;
  const int tps = (a.T + R - 1) / R;
  int64_t tile0, tile_end;
  if (!ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) return;

  bf16x8 wf[K][C / 16], wf2[C / 16];
  {
    const __bf16* wrow = w1p + int64_t(ns * 32 + (lane & 31)) * K * C + 8 * hl;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int g = 0; g < C / 16; ++g) wf[k][g] = *reinterpret_cast<const bf16x8*>(wrow + k * C + 16 * g);
    const __bf16* wrow2 = w2p + int64_t(ns * 32 + (lane & 31)) * C + 8 * hl;
#pragma unroll
    for (int g = 0; g < C / 16; ++g) wf2[g] = *reinterpret_cast<const bf16x8*>(wrow2 + 16 * g);
  }
  ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads
  // biases in accumulator order (element group q = channels ns*32 + 8q + 4hl .. +4),
  // read where used (L1-hot; registers are what bounds this kernel's occupancy)
  // both biases staged in LDS once (zeros when absent): a global bias load in
  // the tile loop would wait behind the next tile's prefetch (memory counters
  // retire in order)
  __shared__ __align__(16) float bsm[2][C];
  for (int i = tid; i < 2 * C; i += 256) {
    const float* bp = i < C ? b1 : b2;
    bsm[i / C][i % C] = bp ? bp[i % C] : 0.f;
  }
  auto bias_q = [&](int which, int q) { return *reinterpret_cast<const floatx4*>(&bsm[which][ns * 32 + 8 * q + 4 * hl]); };

  uint4 xr[G::XV];
  bool xok[G::XV];
  auto load = [&](int64_t tile, bool live) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const __amdgpu_buffer_rsrc_t rs = ru_rsrc(x + b * a.T * C, int64_t(a.T) * C);
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      const int ti = t0 - a.pad + r;
      xok[u] = r < span && ti >= 0 && ti < a.T;
      xr[u] = ru_bload(rs, live && xok[u] ? (ti * C + c) * 2 : RU_OOB);  // Ru32Stage::load
      __builtin_amdgcn_sched_barrier(0);  // program order pinned (Ru32Stage::load)
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      if (r >= span) continue;
      const uint4 raw = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
      if (r >= a.pad && r < a.pad + R) *reinterpret_cast<uint4*>(xraw + ((c >> 5) * R + r - a.pad) * P + (c & 31)) = raw;
      *reinterpret_cast<uint4*>(xs + ((c >> 5) * G::SPAN + r) * P + (c & 31)) = elu8(raw);
    }
  };

  load(tile0, true);
  ru_dummy_stores<4 * G::TM>(out);  // the loop's h / out stores after each prefetch
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    __syncthreads();  // every wave is done with the previous tile's xs / hs
    store();
    __syncthreads();
    // the next tile's rows (no other global load in the tile loop: the
    // residual rows come from the staged raw planes)
    load(tile + 1 < tile_end ? tile + 1 : tile, tile + 1 < tile_end);  // unconditional: exact counts

    // conv1 (k_conv_thin_bf16 order: taps, 16-channel chunks, sub-tiles)
    floatx16 acc[G::TM];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const __bf16* xw = xs + (rg * G::WR + (lane & 31)) * P + 8 * hl;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int g = 0; g < C / 16; ++g) {
        const __bf16* xb = xw + ((g >> 1) * G::SPAN + k * a.dil) * P + 16 * (g & 1);
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][g], *reinterpret_cast<const bf16x8*>(xb + i * 32 * P),
                                                           acc[i], 0, 0, 0);
      }
    // every sub-tile stores (rows past T to RU_OOB): a fixed count of stores per
    // tile keeps the next tile's staging wait exact (ru_bstore)
    const __amdgpu_buffer_rsrc_t rh = ru_rsrc(hout + b * a.T * C, int64_t(a.T) * C);
    const __amdgpu_buffer_rsrc_t ro = ru_rsrc(out + b * a.T * C, int64_t(a.T) * C);
    // h = conv1 + b1 -> bf16 -> HBM; ELU(h) -> the 1x1's LDS tile (plane ns)
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = rg * G::WR + i * 32 + (lane & 31);
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 bq = bias_q(0, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc[i][4 * q + e] + bq[e];
      }
      bf16x8 hf[2];
      ru_acc_to_frags(v, hf);
      const int off = ((t0 + lr) * C + ns * 32 + 8 * hl) * 2;
      // (plain stores: nt on these h rows, whose 128-B lines the two
      // channel-slice waves write in halves, measured 60 -> 79 us)
      ru_bstore(rh, lr < mrows ? off : RU_OOB, hf[0]);
      ru_bstore(rh, lr < mrows ? off + 32 : RU_OOB, hf[1]);
#pragma unroll
      for (int g = 0; g < 2; ++g)
        *reinterpret_cast<uint4*>(hs + (ns * R + lr) * P + 16 * g + 8 * hl) = elu8(__builtin_bit_cast(uint4, hf[g]));
    }
    __syncthreads();
    // out = x + conv2(ELU(h)) + b2 (k_conv_thin_bf16 epilogue order: + bias, then the residual)
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = rg * G::WR + i * 32 + (lane & 31);
      floatx16 acc2;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
      const __bf16* hw = hs + lr * P + 8 * hl;
#pragma unroll
      for (int g = 0; g < C / 16; ++g)
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf2[g], *reinterpret_cast<const bf16x8*>(hw + (g >> 1) * R * P + 16 * (g & 1)),
                                                       acc2, 0, 0, 0);
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 xres = *reinterpret_cast<const uint2*>(xraw + (ns * R + lr) * P + 8 * q + 4 * hl);
        const __bf16* rv = reinterpret_cast<const __bf16*>(&xres);
        const floatx4 bq = bias_q(1, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = __fadd_rn(acc2[4 * q + e] + bq[e], float(rv[e]));
      }
      bf16x8 of[2];
      ru_acc_to_frags(v, of);
      const int off = ((t0 + lr) * C + ns * 32 + 8 * hl) * 2;
      ru_bstore(ro, lr < mrows ? off : RU_OOB, of[0]);
      ru_bstore(ro, lr < mrows ? off + 32 : RU_OOB, of[1]);
    }
  }
}

// Residual unit at 64 channels, backward in ONE launch (the k_ru32_bwd scheme
// with 32-channel output slices per wave, as k_ru64_fwd): g (grad of out) is
// staged over the tile + anti-causal halo; gh = (W2^T g) * ELU'(h) per (32-row
// sub-tile, slice) into a [2][SPAN][P] LDS tile (and HBM for the weight
// gradient); after one barrier gx = conv1^T(gh) * ELU'(x) + g per (row group,
// slice) from the dgrad-packed weights in VGPRs.  Same MFMA order, rounding
// points and epilogue arithmetic as the two thin adjoint launches (1x1 with
// ELU'(h), then k7 with ELU'(x) + g): bit-identical to them.
template <int R>
struct Ru64B {
  static constexpr int C = 64, K = 7, P = F4_P;
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int CV = C / 8;
  static constexpr int XV = (SPAN * CV + 255) / 256;
  static constexpr int WR = R / 2;
  static constexpr int TM = WR / 32;
  static constexpr int NSUBMAX = (SPAN + 31) / 32;
  static constexpr int UPW = (NSUBMAX * 2 + 3) / 4;  // gh (sub-tile, slice) units per wave
  static constexpr size_t LDS = size_t(4) * SPAN * P * 2;  // g planes + gh planes
};

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SEL_W_RU64B))) void k_ru64_bwd(
    Args a, const __bf16* __restrict__ g, const __bf16* __restrict__ h, const __bf16* __restrict__ x,
    const __bf16* __restrict__ wd1, const __bf16* __restrict__ wd2, __bf16* __restrict__ ghout,
    __bf16* __restrict__ gx, int tiles_per_block) {
  using G = Ru64B<R>;
  constexpr int P = G::P, C = G::C, K = G::K, CV = G::CV;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const gs = reinterpret_cast<__bf16*>(smem);  // [2][SPAN][P]: g rows t0 ..
  __bf16* const ghs = gs + 2 * G::SPAN * P;            // [2][SPAN][P]: gh rows t0 ..
  const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ns = wave & 1, rg = wave >> 1;
  const int halo = (K - 1) * a.dil;
  const int span = R + halo;
  const int nsub = (span + 31) / 32;
  const int tps = (a.T + R - 1) / R;
  int64_t tile0, tile_end;
  if (!ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) return;

  bf16x8 wf[K][C / 16];  // the 1x1 adjoint's fragments are read per gh unit (L1-hot)
  {
    const __bf16* wrow = wd1 + int64_t(ns * 32 + (lane & 31)) * K * C + 8 * hl;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int q = 0; q < C / 16; ++q) wf[k][q] = *reinterpret_cast<const bf16x8*>(wrow + k * C + 16 * q);
  }
  // the 1x1 adjoint's weights [C][C] in LDS (rows padded to W2P: 16-B reads of
  // 32 rows x 2 lane halves spread over the banks); a per-unit global load in
  // the gh phase waited behind every request before it (memory counters
  // retire in order)
  constexpr int W2P = C + 8;
  __shared__ __align__(16) __bf16 w2s[C * W2P];
  for (int i = tid; i < C * C / 8; i += 256) {
    const int n = i / (C / 8), c8 = (i % (C / 8)) * 8;
    *reinterpret_cast<bf16x8*>(w2s + n * W2P + c8) = *reinterpret_cast<const bf16x8*>(wd2 + int64_t(n) * C + c8);
  }
  ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads

  uint4 xr[G::XV];
  bool xok[G::XV];
  auto load = [&](int64_t tile, bool live) {  // g rows t0 .. t0 + span (rows >= T: zero; Ru32Stage::load)
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const __amdgpu_buffer_rsrc_t rs = ru_rsrc(g + b * a.T * C, int64_t(a.T) * C);
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      const int ti = t0 + r;
      xok[u] = r < span && ti < a.T;
      xr[u] = ru_bload(rs, live && xok[u] ? (ti * C + c) * 2 : RU_OOB);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < G::XV; ++u) {
      const int v = tid + u * 256;
      const int r = v / CV, c = (v % CV) * 8;
      if (r >= span) continue;
      *reinterpret_cast<uint4*>(gs + ((c >> 5) * G::SPAN + r) * P + (c & 31)) = xok[u] ? xr[u] : make_uint4(0, 0, 0, 0);
    }
  };

  load(tile0, true);
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    __syncthreads();  // every wave is done with the previous tile's gs / ghs
    store();
    __syncthreads();
    // h rows of a gh unit (the ELU'(h) factor), one unit ahead of its MFMAs
    auto load_h = [&](int unit, uint2 (&hq)[4]) {
      const int sb = unit >> 1, sl = unit & 1;
      const int ti = t0 + sb * 32 + (lane & 31);
      const bool inside = unit < 2 * nsub && ti < a.T;
      const int64_t orow = (b * a.T + (inside ? ti : 0)) * C + sl * 32;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        hq[q] = inside ? *reinterpret_cast<const uint2*>(h + orow + 8 * q + 4 * hl) : make_uint2(0, 0);
    };
    // every gh unit's h rows requested up front (one latency per tile, not one per unit)
    uint2 hall[G::UPW][4];
#pragma unroll
    for (int uu = 0; uu < G::UPW; ++uu) load_h(wave + 4 * uu, hall[uu]);
    // x rows of this wave's gx sub-tiles (the ELU'(x) factor), requested before
    // the gh phase so their HBM latency hides behind it
    uint2 xpre[G::TM][4];
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = rg * G::WR + i * 32 + (lane & 31);
      const bool in = lr < mrows;
      const int64_t orow = (b * a.T + t0 + (in ? lr : 0)) * C + ns * 32 + 4 * hl;
#pragma unroll
      for (int q = 0; q < 4; ++q) xpre[i][q] = in ? *reinterpret_cast<const uint2*>(x + orow + 8 * q) : make_uint2(0, 0);
    }

    // gh = (W2^T g) * ELU'(h), units u = (sub-tile, slice) round-robin over the waves
#pragma unroll
    for (int uu = 0; uu < G::UPW; ++uu) {
      const int unit = wave + 4 * uu;
      if (unit >= 2 * nsub) break;  // wave-uniform
      const int sb = unit >> 1, sl = unit & 1;
      const int lr = sb * 32 + (lane & 31);
      const int ti = t0 + lr;
      const bool inside = ti < a.T;
      const int64_t orow = (b * a.T + (inside ? ti : 0)) * C + sl * 32;
      uint2 hq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) hq[q] = hall[uu][q];
      // the slice-sl weights of the 1x1 adjoint: rows n = sl*32 + (lane & 31), from LDS
      bf16x8 w2q[C / 16];
      {
        const __bf16* wr2 = w2s + (sl * 32 + (lane & 31)) * W2P + 8 * hl;
#pragma unroll
        for (int q = 0; q < C / 16; ++q) w2q[q] = *reinterpret_cast<const bf16x8*>(wr2 + 16 * q);
      }
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const __bf16* gw = gs + lr * P + 8 * hl;
#pragma unroll
      for (int q = 0; q < C / 16; ++q)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2q[q], *reinterpret_cast<const bf16x8*>(gw + (q >> 1) * G::SPAN * P + 16 * (q & 1)),
                                                      acc, 0, 0, 0);
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const __bf16* hv = reinterpret_cast<const __bf16*>(&hq[q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = __fmul_rn(acc[4 * q + e], elu_grad_fast(float(hv[e])));
      }
      bf16x8 ghf[2];
      ru_acc_to_frags(v, ghf);
      if (lr < span) {
        *reinterpret_cast<bf16x8*>(ghs + (sl * G::SPAN + lr) * P + 8 * hl) = ghf[0];
        *reinterpret_cast<bf16x8*>(ghs + (sl * G::SPAN + lr) * P + 16 + 8 * hl) = ghf[1];
      }
      if (ghout && lr < mrows) {
        ru_store(ghout + orow + 8 * hl, ghf[0]);
        ru_store(ghout + orow + 16 + 8 * hl, ghf[1]);
      }
    }
    __syncthreads();
    // the next tile's g rows, requested after the gh phase: its h / x / weight
    // loads then wait only for each other (memory counters retire in order),
    // and this request has the gx phase to land
    load(tile + 1 < tile_end ? tile + 1 : tile, tile + 1 < tile_end);  // unconditional: exact counts
    // gx = conv1^T(gh) * ELU'(x) + g (k_conv_thin_bf16 order: taps, chunks, sub-tiles)
    floatx16 acc[G::TM];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const __bf16* hw = ghs + (rg * G::WR + (lane & 31)) * P + 8 * hl;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int q = 0; q < C / 16; ++q) {
        const __bf16* hb = hw + ((q >> 1) * G::SPAN + k * a.dil) * P + 16 * (q & 1);
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][q], *reinterpret_cast<const bf16x8*>(hb + i * 32 * P),
                                                           acc[i], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = rg * G::WR + i * 32 + (lane & 31);
      if (__builtin_amdgcn_readfirstlane(rg * G::WR + i * 32) >= mrows) break;
      const bool valid = lr < mrows;
      const int64_t orow = (b * a.T + t0 + (valid ? lr : 0)) * C + ns * 32;
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 graw = *reinterpret_cast<const uint2*>(gs + (ns * G::SPAN + lr) * P + 8 * q + 4 * hl);
        const __bf16* xv = reinterpret_cast<const __bf16*>(&xpre[i][q]);
        const __bf16* gv = reinterpret_cast<const __bf16*>(&graw);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[4 * q + e] = __fadd_rn(__fmul_rn(acc[i][4 * q + e], elu_grad_fast(float(xv[e]))), float(gv[e]));
      }
      bf16x8 of[2];
      ru_acc_to_frags(v, of);
      if (valid) {
        ru_store(gx + orow + 8 * hl, of[0]);
        ru_store(gx + orow + 16 + 8 * hl, of[1]);
      }
    }
  }
}

// Backward: gh = (W2^T g) * ELU'(h) over the tile + its anti-causal halo (the
// adjoint of the causal conv reads rows t .. t + 6 dil), in registers -> LDS
// (and HBM when the weight gradient needs it); gx = conv1^T(gh) * ELU'(x) + g.
// wd1 / wd2 are the dgrad-packed weights of the primitive path.
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R == 128 ? SEL_W_RU32B : 1))) void k_ru32_bwd(Args a, const __bf16* __restrict__ g,
                                                  const __bf16* __restrict__ h, const __bf16* __restrict__ x,
                                                  const __bf16* __restrict__ wd1, const __bf16* __restrict__ wd2,
                                                  __bf16* __restrict__ ghout, __bf16* __restrict__ gx,
                                                  int tiles_per_block) {
  using G = Ru32<R>;
  constexpr int P = G::P;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const gs = reinterpret_cast<__bf16*>(smem);  // [SPAN][P]: g rows t0 ..
  __bf16* const ghs = gs + G::SPAN * P;                // [SPAN][P]: gh rows t0 ..
  __bf16* const hs = ghs + G::SPAN * P;                // [SPAN][P]: h rows t0 .. (the ELU'(h) factor)
  const int lane = threadIdx.x & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int halo = (RU_K - 1) * a.dil;
  const int span = R + halo;
  const int nsub = (span + 31) / 32;  // gh sub-tiles (tile + halo)
  const int tps = (a.T + R - 1) / R;
  int64_t tile0, tile_end;
  if (!ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) return;

  bf16x8 wf[RU_K][2], w2f[1][2];
  ru_wfrags<RU_K>(wd1, wf);
  ru_wfrags<1>(wd2, w2f);
  ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads

  // g and h rows staged one tile ahead (k_ru32_bwdw): the gh phase reads h from
  // LDS instead of waiting on a request made at the top of the tile
  Ru32Stage<R> st, sh;
  st.load(a, g, tile0 / tps, int(tile0 % tps) * R, 0, span);
  sh.load(a, h, tile0 / tps, int(tile0 % tps) * R, 0, span);
  ru_dummy_stores<2 * G::TM>(gx);  // the loop's gx stores after each prefetch
  for (int64_t tile = tile0; tile < tile_end; ++tile) {
    const int64_t b = tile / tps;
    const int t0 = int(tile % tps) * R;
    const int mrows = a.T - t0 < R ? a.T - t0 : R;
    __syncthreads();  // every wave is done with the previous tile's g / gh rows
    st.store(gs, span, false);
    sh.store(hs, span, false);
    __syncthreads();
    // the x rows of this wave's gx sub-tiles (ELU'(x)), requested up front (their
    // latency hides behind the gh phase)
    constexpr int NSUB_W = (G::SPAN / 32 + 3) / 4;  // gh sub-tiles per wave (max)
    uint2 xpre[G::TM][4];
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = wave * (R / 4) + i * 32 + (lane & 31);
      const bool in = lr < mrows;
      const int64_t orow = (b * a.T + t0 + (in ? lr : 0)) * RU_C;
#pragma unroll
      for (int q = 0; q < 4; ++q) xpre[i][q] = in ? *reinterpret_cast<const uint2*>(x + orow + 8 * q + 4 * hl) : make_uint2(0, 0);
    }
    // gh for rows t0 .. t0 + span (rows >= T: g staged as zero -> gh = 0)
#pragma unroll
    for (int j = 0; j < NSUB_W; ++j) {
      const int sb = wave + 4 * j;
      if (sb >= nsub) break;
      const int lr = sb * 32 + (lane & 31);
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const __bf16* gw = gs + lr * P + 8 * hl;
#pragma unroll
      for (int c = 0; c < 2; ++c)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[0][c], *reinterpret_cast<const bf16x8*>(gw + 16 * c), acc, 0, 0, 0);
      const int ti = t0 + lr;
      const bool inside = ti < a.T;
      const int64_t orow = (b * a.T + (inside ? ti : 0)) * RU_C;
      uint2 hq[4];  // h rows (zero past T), as staged
#pragma unroll
      for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const uint2*>(hs + lr * P + 8 * q + 4 * hl);
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const __bf16* hv = reinterpret_cast<const __bf16*>(&hq[q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = acc[4 * q + e] * elu_grad_fast(float(hv[e]));
      }
      bf16x8 ghf[2];
      ru_acc_to_frags(v, ghf);
      if (lr < span) {
        *reinterpret_cast<bf16x8*>(ghs + lr * P + 8 * hl) = ghf[0];
        *reinterpret_cast<bf16x8*>(ghs + lr * P + 16 + 8 * hl) = ghf[1];
      }
      if (ghout && lr < mrows) {
        ru_store(ghout + orow + 8 * hl, ghf[0]);
        ru_store(ghout + orow + 16 + 8 * hl, ghf[1]);
      }
    }
    __syncthreads();
    // the next tile's g rows, requested after the gh phase (k_ru64_bwd)
    {  // unconditional (a dead request loads nothing): exact counts
      const bool live = tile + 1 < tile_end;
      const int64_t nt = live ? tile + 1 : tile;
      st.load(a, g, nt / tps, int(nt % tps) * R, 0, span, live);
      sh.load(a, h, nt / tps, int(nt % tps) * R, 0, span, live);
    }
    // every sub-tile stores (rows past T to RU_OOB): a fixed count of stores per
    // tile keeps the next tile's staging waits exact (ru_bstore)
    const __amdgpu_buffer_rsrc_t rgx = ru_rsrc(gx + b * a.T * RU_C, int64_t(a.T) * RU_C);
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
      const int lr = wave * (R / 4) + i * 32 + (lane & 31);
      floatx16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const __bf16* hw = ghs + lr * P + 8 * hl;
#pragma unroll
      for (int k = 0; k < RU_K; ++k)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][c], *reinterpret_cast<const bf16x8*>(hw + k * a.dil * P + 16 * c),
                                                        acc, 0, 0, 0);
      const bool valid = lr < mrows;
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 graw = *reinterpret_cast<const uint2*>(gs + lr * P + 8 * q + 4 * hl);
        const __bf16* xv = reinterpret_cast<const __bf16*>(&xpre[i][q]);
        const __bf16* gv = reinterpret_cast<const __bf16*>(&graw);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[4 * q + e] = __fadd_rn(__fmul_rn(acc[4 * q + e], elu_grad_fast(float(xv[e]))), float(gv[e]));
      }
      bf16x8 of[2];
      ru_acc_to_frags(v, of);
      const int off = ((t0 + lr) * RU_C + 8 * hl) * 2;
      ru_bstore<SEL_RU32B_GXNT>(rgx, valid ? off : RU_OOB, of[0]);
      ru_bstore<SEL_RU32B_GXNT>(rgx, valid ? off + 32 : RU_OOB, of[1]);
    }
  }
}

// ---------------------------------------------------------------------------
// Residual unit at 32 channels: backward AND both weight gradients in one
// launch (the encoder's units, whose weights train; residual_unit.py:43-46,
// conv_layer.py:139-142).  k_ru32_bwd's two phases (gh, then gx), plus:
//  * ELU(bf16 h) of the tile rows -> LDS, from the h rows the gh phase already
//    holds for ELU'(h); ELU(x) of the tile + its causal halo -> LDS, staged with
//    g (the operands conv1 and the 1x1 consumed in the forward, same elu8);
//  * after gx, the 7 conv1 taps and the 1x1 as eight 32x32 MFMA accumulators,
//    two per wave (waves 0-2: taps 2w, 2w+1 sharing the gh operand; wave 3:
//    tap 6 and the 1x1), reduced over the tile rows with transposing LDS reads
//    (ds_read_b64_tr_b16: the k_wgrad3_bf16 operand scheme) and carried across
//    all of the block's tiles;
//  * one fp32 partial per block of each weight (+ the bias column sums of gh
//    and g, waves 0 and 3), in the packed [N][K][C] layout that
//    sel_wgrad_finish_many reduces in block order (deterministic).
// HBM per row: reads g, h, x and writes gx; the unfused path also wrote gh and
// re-read g, h, gh, x for the two weight-gradient launches (9 tensors).
// The gh and gx phases are k_ru32_bwd's arithmetic exactly (same bits).
// ---------------------------------------------------------------------------
template <int R>
struct Ru32W {
  static constexpr int P = F4_P;   // g / gh rows (80 B: conflict-free ds_read_b128 of the gx phase)
  static constexpr int PW = 32;    // ELU(x) / ELU(h) rows (64 B: conflict-free transposing reads)
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int NW1 = RU_C * RU_K * RU_C, NW2 = RU_C * RU_C;  // packed weight elements
  // g, gh and h planes (pitch P) + ELU(x) span and ELU(h) tile planes (pitch PW)
  static constexpr size_t LDS = size_t(3) * SPAN * P * 2 + size_t(SPAN + R) * PW * 2;
  static_assert(R % 128 == 0, "ru32 tile rows");
};

template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SEL_W_RU32W))) void k_ru32_bwdw(Args a, const __bf16* __restrict__ g,
                                                   const __bf16* __restrict__ h, const __bf16* __restrict__ x,
                                                   const __bf16* __restrict__ wd1, const __bf16* __restrict__ wd2,
                                                   __bf16* __restrict__ gx, float* __restrict__ part1,
                                                   float* __restrict__ part2, int tiles_per_block) {
  using G = Ru32W<R>;
  constexpr int P = G::P, PW = G::PW;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const gs = reinterpret_cast<__bf16*>(smem);  // [SPAN][P]: g rows t0 ..
  __bf16* const ghs = gs + G::SPAN * P;                // [SPAN][P]: gh rows t0 ..
  __bf16* const xs = ghs + G::SPAN * P;                // [SPAN][PW]: ELU(x) rows t0 - halo ..
  __bf16* const es = xs + G::SPAN * PW;                // [R][PW]: ELU(h) rows t0 ..
  __bf16* const hs = es + R * PW;                      // [SPAN][P]: h rows t0 .. (the ELU'(h) factor)
  const int lane = threadIdx.x & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int halo = (RU_K - 1) * a.dil;
  const int span = R + halo;
  const int nsub = (span + 31) / 32;
  const int tps = (a.T + R - 1) / R;

  // weight-gradient jobs of this wave: job 0 = conv1 tap k0 (A = gh), job 1 =
  // conv1 tap k0 + 1 (waves 0-2, same A) or the 1x1 (wave 3: A = g, B = ELU(h))
  const int k0 = wave < 3 ? 2 * wave : 6;
  floatx16 wacc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) wacc[j][e] = 0.f;
  float bsum = 0.f;  // wave 0: column sums of gh (conv1 bias), wave 3: of g (1x1 bias)
  // transposing-read lane geometry (k_wgrad3_bf16): rows 4 hl + q and 8 + 4 hl + q, 4 columns at col
  const int tq = (lane & 15) >> 2;
  const int tcol = ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
  auto trfrag = [&](const __bf16* base, int pitch, int r0) {
    const v4i16 lo = tr_read(base + (r0 + 4 * hl + tq) * pitch + tcol);
    const v4i16 hi = tr_read(base + (r0 + 8 + 4 * hl + tq) * pitch + tcol);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  int64_t tile0, tile_end;
  if (ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end)) {
    bf16x8 wf[RU_K][2], w2f[1][2];
    ru_wfrags<RU_K>(wd1, wf);
    ru_wfrags<1>(wd2, w2f);
    ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads

    // g, x and h rows staged one tile ahead (branch-free buffer loads): the gh
    // phase then reads h from LDS instead of waiting on a request made at the
    // top of the tile
    Ru32Stage<R> st, sx, sh;
    st.load(a, g, tile0 / tps, int(tile0 % tps) * R, 0, span);
    sx.load(a, x, tile0 / tps, int(tile0 % tps) * R, -halo, span);
    sh.load(a, h, tile0 / tps, int(tile0 % tps) * R, 0, span);
    ru_dummy_stores<2 * Ru32<R>::TM>(gx);  // the loop's gx stores after each prefetch
    for (int64_t tile = tile0; tile < tile_end; ++tile) {
      const int64_t b = tile / tps;
      const int t0 = int(tile % tps) * R;
      const int mrows = a.T - t0 < R ? a.T - t0 : R;
      __syncthreads();  // every wave is done with the previous tile's rows
      st.store(gs, span, false);
      sx.store(xs, span, true, nullptr, 0, PW);
      sh.store(hs, span, false);
      __syncthreads();
      constexpr int NSUB_W = (G::SPAN / 32 + 3) / 4;
      uint2 xpre[Ru32<R>::TM][4];
#pragma unroll
      for (int i = 0; i < Ru32<R>::TM; ++i) {
        const int lr = wave * (R / 4) + i * 32 + (lane & 31);
        const bool in = lr < mrows;
        const int64_t orow = (b * a.T + t0 + (in ? lr : 0)) * RU_C;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          xpre[i][q] = in ? *reinterpret_cast<const uint2*>(x + orow + 8 * q + 4 * hl) : make_uint2(0, 0);
      }
      // gh for rows t0 .. t0 + span (k_ru32_bwd); ELU(h) of the tile rows -> es
#pragma unroll
      for (int j = 0; j < NSUB_W; ++j) {
        const int sb = wave + 4 * j;
        if (sb >= nsub) break;
        const int lr = sb * 32 + (lane & 31);
        floatx16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const __bf16* gw = gs + lr * P + 8 * hl;
#pragma unroll
        for (int c = 0; c < 2; ++c)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[0][c], *reinterpret_cast<const bf16x8*>(gw + 16 * c), acc, 0,
                                                        0, 0);
        uint2 hq[4];  // h rows (zero past T), as staged
#pragma unroll
        for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const uint2*>(hs + lr * P + 8 * q + 4 * hl);
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const __bf16* hv = reinterpret_cast<const __bf16*>(&hq[q]);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * q + e] = acc[4 * q + e] * elu_grad_fast(float(hv[e]));
        }
        bf16x8 ghf[2];
        ru_acc_to_frags(v, ghf);
        if (lr < span) {
          *reinterpret_cast<bf16x8*>(ghs + lr * P + 8 * hl) = ghf[0];
          *reinterpret_cast<bf16x8*>(ghs + lr * P + 16 + 8 * hl) = ghf[1];
        }
        if (sb < R / 32) {  // wave-uniform: a tile sub-tile (rows past T hold h = 0 -> ELU = 0)
#pragma unroll
          for (int qq = 0; qq < 2; ++qq) {
            const uint4 e8 = elu8(make_uint4(hq[2 * qq].x, hq[2 * qq].y, hq[2 * qq + 1].x, hq[2 * qq + 1].y));
            *reinterpret_cast<uint2*>(es + lr * PW + 16 * qq + 4 * hl) = make_uint2(e8.x, e8.y);
            *reinterpret_cast<uint2*>(es + lr * PW + 16 * qq + 8 + 4 * hl) = make_uint2(e8.z, e8.w);
          }
        }
      }
      __syncthreads();
      // the next tile's g and x rows, requested after the gh phase (k_ru64_bwd)
      {  // unconditional (a dead request loads nothing): exact counts
        const bool live = tile + 1 < tile_end;
        const int64_t nt = live ? tile + 1 : tile;
        st.load(a, g, nt / tps, int(nt % tps) * R, 0, span, live);
        sx.load(a, x, nt / tps, int(nt % tps) * R, -halo, span, live);
        sh.load(a, h, nt / tps, int(nt % tps) * R, 0, span, live);
      }
      // gx = conv1^T(gh) * ELU'(x) + g (k_ru32_bwd); every sub-tile stores
      // (rows past T to RU_OOB): a fixed count of stores per tile keeps the
      // next tile's staging waits exact (ru_bstore)
      const __amdgpu_buffer_rsrc_t rgx = ru_rsrc(gx + b * a.T * RU_C, int64_t(a.T) * RU_C);
#pragma unroll
      for (int i = 0; i < Ru32<R>::TM; ++i) {
        const int lr = wave * (R / 4) + i * 32 + (lane & 31);
        floatx16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        const __bf16* hw = ghs + lr * P + 8 * hl;
#pragma unroll
        for (int k = 0; k < RU_K; ++k)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][c],
                                                          *reinterpret_cast<const bf16x8*>(hw + k * a.dil * P + 16 * c),
                                                          acc, 0, 0, 0);
        const bool valid = lr < mrows;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint2 graw = *reinterpret_cast<const uint2*>(gs + lr * P + 8 * q + 4 * hl);
          const __bf16* xv = reinterpret_cast<const __bf16*>(&xpre[i][q]);
          const __bf16* gv = reinterpret_cast<const __bf16*>(&graw);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[4 * q + e] = __fadd_rn(__fmul_rn(acc[4 * q + e], elu_grad_fast(float(xv[e]))), float(gv[e]));
        }
        bf16x8 of[2];
        ru_acc_to_frags(v, of);
        const int off = ((t0 + lr) * RU_C + 8 * hl) * 2;
        ru_bstore(rgx, valid ? off : RU_OOB, of[0]);
        ru_bstore(rgx, valid ? off + 32 : RU_OOB, of[1]);
      }
      // weight gradients over the tile rows (rows past T: g = 0 -> gh = 0)
      const __bf16* b0p = xs + k0 * a.dil * PW;
      const __bf16* b1p = wave < 3 ? b0p + a.dil * PW : es;
#pragma unroll
      for (int kh = 0; kh < R / 16; ++kh) {
        const bf16x8 A0 = trfrag(ghs, P, kh * 16);
        const bf16x8 B0 = trfrag(b0p, PW, kh * 16);
        const bf16x8 B1 = trfrag(b1p, PW, kh * 16);
        wacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B0, wacc[0], 0, 0, 0);
        if (wave < 3) {
          wacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B1, wacc[1], 0, 0, 0);
          if (wave == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bsum += float(A0[e]);
          }
        } else {
          const bf16x8 A1 = trfrag(gs, P, kh * 16);
          wacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B1, wacc[1], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 8; ++e) bsum += float(A1[e]);
        }
      }
    }
  }
  // this block's partials (zeros from a block without tiles): accumulator
  // element r of lane l -> n = (r & 3) + 8 (r >> 2) + 4 hl, c = l & 31
  const int nb = gridDim.x;
  float* const p1 = part1 + int64_t(blockIdx.x) * G::NW1;
  float* const p2 = part2 + int64_t(blockIdx.x) * G::NW2;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = (r & 3) + 8 * (r >> 2) + 4 * hl, c = lane & 31;
    p1[(n * RU_K + k0) * RU_C + c] = wacc[0][r];
    if (wave < 3) p1[(n * RU_K + k0 + 1) * RU_C + c] = wacc[1][r];
    else p2[n * RU_C + c] = wacc[1][r];
  }
  bsum += __shfl_xor(bsum, 32, 64);
  if (wave == 0 && lane < 32) part1[int64_t(nb) * G::NW1 + int64_t(blockIdx.x) * RU_C + lane] = bsum;
  if (wave == 3 && lane < 32) part2[int64_t(nb) * G::NW2 + int64_t(blockIdx.x) * RU_C + lane] = bsum;
}

// ---------------------------------------------------------------------------
// Residual unit at 64 channels: backward AND both weight gradients in one
// launch (round 4; the encoder's units, residual_unit.py:43-46 and the wgrad of
// conv_layer.py:139-142).  The weight-gradient accumulators (28 conv1 tiles +
// 4 1x1 tiles of 32x32 fp32 = 128 registers per lane over four waves) do not
// fit beside k_ru64_bwd's register-resident k7 adjoint (112 VGPRs), so the
// workgroup has eight waves in two roles that share every LDS plane:
//  * all eight stage the next tile's g, h and x span rows (registers, one
//    tile ahead, branch-free buffer loads) and compute gh = (W2^T g) * ELU'(h)
//    over the tile + its anti-causal halo (k_ru64_bwd's gh units) into LDS,
//    plus ELU(bf16 h) of the tile rows;
//  * waves 0-3 compute gx = conv1^T(gh) * ELU'(x) + g exactly as k_ru64_bwd
//    (same MFMA order, rounding points and epilogue: same bits);
//  * waves 4-7 accumulate the weight gradients over the tile rows with
//    transposing LDS reads (the k_ru32_bwdw / k_wgrad3_bf16 operand scheme):
//    wave 4 + v owns h-channel slice v & 1 and, for v < 2, conv1 taps 0-3, for
//    v >= 2 taps 4-6 and the 1x1 (A = g, B = ELU(h)), both input-channel
//    slices, plus the bias column sums of gh (v < 2) or g (v >= 2).
// A workgroup's waves are dealt to the SIMDs cyclically, so each SIMD runs one
// gx wave beside one weight-gradient wave.  The roles' tile loops are separate
// code (so neither role's registers are live in the other) with the same
// barrier sequence.  One workgroup per CU (the planes take 159 KB of LDS);
// one fp32 partial per workgroup of every weight, in the packed layouts that
// sel_wgrad_finish_many reduces in block order (deterministic).
// HBM per row: reads g, h, x and writes gx; k_ru64_bwd with gh plus the two
// k_wgrad3 launches moved 9 tensors.
// ---------------------------------------------------------------------------
template <int R>
struct Ru64W {
  static constexpr int C = 64, K = 7, P = F4_P, PW = 32;
  static constexpr int SPAN = R + F4_HALOMAX;
  static constexpr int CV = C / 8;
  static constexpr int XV = (SPAN * CV + 511) / 512;  // staged 16-B pieces per thread and tensor
  static constexpr int UPW = (2 * (SPAN / 32) + 7) / 8;  // gh (sub-tile, slice) units per wave
  static constexpr int NW1 = C * K * C, NW2 = C * C;
  static constexpr int W2P = C + 8;
  // planes (bf16 elements): g, gh, h [2][SPAN][P]; ELU(x) span [2][SPAN][PW];
  // raw x tile [2][R][P] (ELU'(x)); ELU(h) tile [2][R][PW]; the 1x1 adjoint [C][W2P]
  static constexpr size_t OFF_GH = size_t(2) * SPAN * P;
  static constexpr size_t OFF_H = 2 * OFF_GH;
  static constexpr size_t OFF_XS = 3 * OFF_GH;
  static constexpr size_t OFF_XR = OFF_XS + size_t(2) * SPAN * PW;
  static constexpr size_t OFF_ES = OFF_XR + size_t(2) * R * P;
  static constexpr size_t OFF_W2 = OFF_ES + size_t(2) * R * PW;
  static constexpr size_t LDS = (OFF_W2 + size_t(C) * W2P) * 2;
  static_assert(R % 64 == 0 && LDS <= 160 * 1024, "ru64w tile rows / LDS");
  static_assert(SPAN * CV % 512 == 0, "ru64w staging pieces");
};

template <int R>
struct Ru64WStage {
  uint4 g[Ru64W<R>::XV], h[Ru64W<R>::XV], x[Ru64W<R>::XV];
};

// one tile's g, h (rows t0 .. t0 + span) and x (rows t0 - halo .. t0 + R) into
// registers: branch-free buffer loads (rows outside [0, T), past the span or of
// a dead request read nothing and return zeros; Ru32Stage::load)
template <int R>
__device__ __forceinline__ void ru64w_load(Ru64WStage<R>& st, const Args& a, const __bf16* __restrict__ g,
                                           const __bf16* __restrict__ h, const __bf16* __restrict__ x, int64_t tile,
                                           int tps, int halo, bool live) {
  using G = Ru64W<R>;
  const int64_t b = tile / tps;
  const int t0 = int(tile % tps) * R;
  const int64_t base = b * a.T * G::C;
  const __amdgpu_buffer_rsrc_t rg = ru_rsrc(g + base, int64_t(a.T) * G::C);
  const __amdgpu_buffer_rsrc_t rh = ru_rsrc(h + base, int64_t(a.T) * G::C);
  const __amdgpu_buffer_rsrc_t rx = ru_rsrc(x + base, int64_t(a.T) * G::C);
  const int span = R + halo;
#pragma unroll
  for (int u = 0; u < G::XV; ++u) {
    const int v = threadIdx.x + u * 512;
    const int r = v / G::CV, c = (v % G::CV) * 8;
    const int tg = t0 + r, tx = t0 - halo + r;
    const bool gok = live && r < span && tg < a.T;
    const bool xok = live && r < span && tx >= 0 && tx < a.T;
    // program order pinned (sched_barrier): the loads leave in the same order
    // from the prologue and from the tile loop, so the waits of the staging
    // store count them exactly on both paths into it
    st.g[u] = ru_bload(rg, gok ? (tg * G::C + c) * 2 : RU_OOB);
    __builtin_amdgcn_sched_barrier(0);
    st.h[u] = ru_bload(rh, gok ? (tg * G::C + c) * 2 : RU_OOB);
    __builtin_amdgcn_sched_barrier(0);
    st.x[u] = ru_bload(rx, xok ? (tx * G::C + c) * 2 : RU_OOB);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the staged tile -> LDS planes (out-of-range rows were loaded as zeros)
template <int R>
__device__ __forceinline__ void ru64w_store(const Ru64WStage<R>& st, __bf16* smem_bf, int span, int halo) {
  using G = Ru64W<R>;
  constexpr int P = G::P, PW = G::PW, SPAN = G::SPAN;
  __bf16* const gs = smem_bf;
  __bf16* const hs = smem_bf + G::OFF_H;
  __bf16* const xs = smem_bf + G::OFF_XS;
  __bf16* const xr = smem_bf + G::OFF_XR;
#pragma unroll
  for (int u = 0; u < G::XV; ++u) {
    const int v = threadIdx.x + u * 512;
    const int r = v / G::CV, c = (v % G::CV) * 8;
    if (r >= span) continue;
    const int pl = c >> 5, cc = c & 31;
    *reinterpret_cast<uint4*>(gs + (pl * SPAN + r) * P + cc) = st.g[u];
    *reinterpret_cast<uint4*>(hs + (pl * SPAN + r) * P + cc) = st.h[u];
    *reinterpret_cast<uint4*>(xs + (pl * SPAN + r) * PW + cc) = elu8(st.x[u]);
    if (r >= halo && r < halo + R) *reinterpret_cast<uint4*>(xr + (pl * R + r - halo) * P + cc) = st.x[u];
  }
}

// gh = (W2^T g) * ELU'(h) over rows t0 .. t0 + span (k_ru64_bwd's units, round
// robin over the eight waves) -> ghs; ELU(bf16 h) of the tile rows -> es
template <int R>
__device__ __forceinline__ void ru64w_gh(__bf16* smem_bf, int wave, int lane, int nsub, int span) {
  using G = Ru64W<R>;
  constexpr int P = G::P, PW = G::PW, SPAN = G::SPAN, C = G::C;
  const __bf16* const gs = smem_bf;
  __bf16* const ghs = smem_bf + G::OFF_GH;
  const __bf16* const hs = smem_bf + G::OFF_H;
  __bf16* const es = smem_bf + G::OFF_ES;
  const __bf16* const w2s = smem_bf + G::OFF_W2;
  const int hl = lane >> 5;
#pragma unroll
  for (int uu = 0; uu < G::UPW; ++uu) {
    const int unit = wave + 8 * uu;
    if (unit >= 2 * nsub) break;  // wave-uniform
    const int sb = unit >> 1, sl = unit & 1;
    const int lr = sb * 32 + (lane & 31);
    bf16x8 w2q[C / 16];
    {
      const __bf16* wr2 = w2s + (sl * 32 + (lane & 31)) * G::W2P + 8 * hl;
#pragma unroll
      for (int q = 0; q < C / 16; ++q) w2q[q] = *reinterpret_cast<const bf16x8*>(wr2 + 16 * q);
    }
    floatx16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const __bf16* gw = gs + lr * P + 8 * hl;
#pragma unroll
    for (int q = 0; q < C / 16; ++q)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2q[q], *reinterpret_cast<const bf16x8*>(gw + (q >> 1) * SPAN * P + 16 * (q & 1)),
                                                    acc, 0, 0, 0);
    uint2 hq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) hq[q] = *reinterpret_cast<const uint2*>(hs + (sl * SPAN + lr) * P + 8 * q + 4 * hl);
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const __bf16* hv = reinterpret_cast<const __bf16*>(&hq[q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * q + e] = __fmul_rn(acc[4 * q + e], elu_grad_fast(float(hv[e])));
    }
    bf16x8 ghf[2];
    ru_acc_to_frags(v, ghf);
    if (lr < span) {
      *reinterpret_cast<bf16x8*>(ghs + (sl * SPAN + lr) * P + 8 * hl) = ghf[0];
      *reinterpret_cast<bf16x8*>(ghs + (sl * SPAN + lr) * P + 16 + 8 * hl) = ghf[1];
    }
    if (sb < R / 32) {  // wave-uniform: a tile sub-tile (rows past T hold h = 0 -> ELU = 0)
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const uint4 e8 = elu8(make_uint4(hq[2 * qq].x, hq[2 * qq].y, hq[2 * qq + 1].x, hq[2 * qq + 1].y));
        *reinterpret_cast<uint2*>(es + (sl * R + lr) * PW + 16 * qq + 4 * hl) = make_uint2(e8.x, e8.y);
        *reinterpret_cast<uint2*>(es + (sl * R + lr) * PW + 16 * qq + 8 + 4 * hl) = make_uint2(e8.z, e8.w);
      }
    }
  }
}

// WG = false: the same kernel without the weight-gradient role (the decoder's
// units, whose weights are frozen): all eight waves compute gx, one 32-row
// sub-tile and 32-channel slice each (part1 / part2 unused).
template <int R, bool WG = true>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void k_ru64_bwdw(
    Args a, const __bf16* __restrict__ g, const __bf16* __restrict__ h, const __bf16* __restrict__ x,
    const __bf16* __restrict__ wd1, const __bf16* __restrict__ wd2, __bf16* __restrict__ gx,
    float* __restrict__ part1, float* __restrict__ part2, int tiles_per_block) {
  using G = Ru64W<R>;
  constexpr int P = G::P, PW = G::PW, C = G::C, K = G::K, SPAN = G::SPAN;
  extern __shared__ __align__(16) unsigned char smem[];
  __bf16* const sb = reinterpret_cast<__bf16*>(smem);
  const __bf16* const gs = sb;
  const __bf16* const ghs = sb + G::OFF_GH;
  const __bf16* const xs = sb + G::OFF_XS;
  const __bf16* const xr = sb + G::OFF_XR;
  const __bf16* const es = sb + G::OFF_ES;
  const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int halo = (K - 1) * a.dil;
  const int span = R + halo;
  const int nsub = (span + 31) / 32;
  const int tps = (a.T + R - 1) / R;
  int64_t tile0 = 0, tile_end = 0;
  const bool any = ru_tiles((a.rows / a.T) * tps, tiles_per_block, tile0, tile_end);

  // the 1x1 adjoint's weights [C][C] -> LDS (rows padded to W2P; k_ru64_bwd)
  if (any) {
    __bf16* const w2s = sb + G::OFF_W2;
    for (int i = tid; i < C * C / 8; i += 512) {
      const int n = i / (C / 8), c8 = (i % (C / 8)) * 8;
      *reinterpret_cast<bf16x8*>(w2s + n * G::W2P + c8) = *reinterpret_cast<const bf16x8*>(wd2 + int64_t(n) * C + c8);
    }
  }

  if (!WG || wave < 4) {
    // ---- gx role: k_ru64_bwd's gx phase (row group rg, output slice ns) ----
    if (!any) return;  // workgroup-uniform: a block without tiles has no barriers
    const int ns = wave & 1, rg = wave >> 1;
    constexpr int WR = WG ? R / 2 : R / 4, TM = WR / 32;
    bf16x8 wf[K][C / 16];
    {
      const __bf16* wrow = wd1 + int64_t(ns * 32 + (lane & 31)) * K * C + 8 * hl;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int q = 0; q < C / 16; ++q) wf[k][q] = *reinterpret_cast<const bf16x8*>(wrow + k * C + 16 * q);
    }
    ws_wait_vm<0>();  // weights landed: the tile loop's waits then count only its own loads
    Ru64WStage<R> st;
    ru64w_load<R>(st, a, g, h, x, tile0, tps, halo, true);
    ru_dummy_stores<2 * TM>(gx);  // the loop's gx stores after each prefetch
    for (int64_t tile = tile0; tile < tile_end; ++tile) {
      const int64_t b = tile / tps;
      const int t0 = int(tile % tps) * R;
      const int mrows = a.T - t0 < R ? a.T - t0 : R;
      __syncthreads();  // B1: every wave is done with the previous tile's planes
      ru64w_store<R>(st, sb, span, halo);
      __syncthreads();  // B2
      ru64w_load<R>(st, a, g, h, x, tile + 1 < tile_end ? tile + 1 : tile, tps, halo, tile + 1 < tile_end);
      ru64w_gh<R>(sb, wave, lane, nsub, span);
      __syncthreads();  // B3: gh planes complete
      floatx16 acc[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
      const __bf16* hw = ghs + (rg * WR + (lane & 31)) * P + 8 * hl;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int q = 0; q < C / 16; ++q) {
          const __bf16* hb = hw + ((q >> 1) * SPAN + k * a.dil) * P + 16 * (q & 1);
#pragma unroll
          for (int i = 0; i < TM; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[k][q], *reinterpret_cast<const bf16x8*>(hb + i * 32 * P),
                                                             acc[i], 0, 0, 0);
        }
      // every sub-tile is stored (rows past T to RU_OOB): a fixed count of
      // stores per tile keeps the next tile's staging wait exact (ru_bstore)
      const __amdgpu_buffer_rsrc_t rgx = ru_rsrc(gx + b * a.T * C, int64_t(a.T) * C);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int lr = rg * WR + i * 32 + (lane & 31);
        const bool valid = lr < mrows;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint2 graw = *reinterpret_cast<const uint2*>(gs + (ns * SPAN + lr) * P + 8 * q + 4 * hl);
          const uint2 xraw = *reinterpret_cast<const uint2*>(xr + (ns * R + lr) * P + 8 * q + 4 * hl);
          const __bf16* xv = reinterpret_cast<const __bf16*>(&xraw);
          const __bf16* gv = reinterpret_cast<const __bf16*>(&graw);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[4 * q + e] = __fadd_rn(__fmul_rn(acc[i][4 * q + e], elu_grad_fast(float(xv[e]))), float(gv[e]));
        }
        bf16x8 of[2];
        ru_acc_to_frags(v, of);
        const int off = ((t0 + lr) * C + ns * 32 + 8 * hl) * 2;
        ru_bstore(rgx, valid ? off : RU_OOB, of[0]);
        ru_bstore(rgx, valid ? off + 32 : RU_OOB, of[1]);
      }
    }
    return;
  }
  if constexpr (WG) {
  // ---- weight-gradient role ----
  const int v = wave - 4;
  const int wn = v & 1;     // h-channel (output) slice of the weight gradients
  const int upper = v >> 1;  // 0: conv1 taps 0-3; 1: taps 4-6 + the 1x1
  floatx16 wacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) wacc[j][e] = 0.f;
  float bsum = 0.f;  // column sums of gh (upper = 0: conv1 bias) or g (upper = 1: the 1x1's)
  if (any) {
    const int tq = (lane & 15) >> 2;
    const int tcol = ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
    auto trfrag = [&](const __bf16* base, int pitch, int r0) {
      const v4i16 lo = tr_read(base + (r0 + 4 * hl + tq) * pitch + tcol);
      const v4i16 hi = tr_read(base + (r0 + 8 + 4 * hl + tq) * pitch + tcol);
      return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    // wave-uniform operand bases: A0 = gh slice wn; jobs 0-5 = taps kb + j/2 over
    // ELU(x) input slice j & 1; jobs 6-7: A1 (gh again / g) against tap 3 of
    // ELU(x) (upper = 0) or ELU(h) (upper = 1), input slice j & 1
    const int kb = upper ? 4 : 0;
    const __bf16* const a0p = ghs + wn * SPAN * P;
    const __bf16* const a1p = upper ? gs + wn * SPAN * P : a0p;
    const __bf16* const b67 = upper ? es : xs + 3 * a.dil * PW;
    const int b67s = upper ? R * PW : SPAN * PW;
    Ru64WStage<R> st;
    ru64w_load<R>(st, a, g, h, x, tile0, tps, halo, true);
    for (int64_t tile = tile0; tile < tile_end; ++tile) {
      __syncthreads();  // B1
      ru64w_store<R>(st, sb, span, halo);
      __syncthreads();  // B2
      ru64w_load<R>(st, a, g, h, x, tile + 1 < tile_end ? tile + 1 : tile, tps, halo, tile + 1 < tile_end);
      ru64w_gh<R>(sb, wave, lane, nsub, span);
      __syncthreads();  // B3
      // rows past T hold g = 0 -> gh = 0: no masks
#pragma unroll 1
      for (int kh = 0; kh < R / 16; ++kh) {
        const bf16x8 A0 = trfrag(a0p, P, kh * 16);
        const bf16x8 A1 = trfrag(a1p, P, kh * 16);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const bf16x8 B = trfrag(xs + ((j & 1) * SPAN + (kb + (j >> 1)) * a.dil) * PW, PW, kh * 16);
          wacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, B, wacc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16x8 B = trfrag(b67 + j * b67s, PW, kh * 16);
          wacc[6 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, B, wacc[6 + j], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum += float(A1[e]);
      }
    }
  }
  // this block's partials (zeros from a block without tiles): accumulator
  // element r of lane l -> n = wn*32 + (r & 3) + 8 (r >> 2) + 4 hl, c = slice*32 + (l & 31)
  const int nb = gridDim.x;
  float* const p1 = part1 + int64_t(blockIdx.x) * G::NW1;
  float* const p2 = part2 + int64_t(blockIdx.x) * G::NW2;
  const int kb = upper ? 4 : 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl, c = lane & 31;
#pragma unroll
    for (int j = 0; j < 6; ++j) p1[(n * K + kb + (j >> 1)) * C + (j & 1) * 32 + c] = wacc[j][r];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (upper) p2[n * C + j * 32 + c] = wacc[6 + j][r];
      else p1[(n * K + 3) * C + j * 32 + c] = wacc[6 + j][r];
    }
  }
  bsum += __shfl_xor(bsum, 32, 64);
  if (lane < 32) {
    if (upper) part2[int64_t(nb) * G::NW2 + int64_t(blockIdx.x) * C + wn * 32 + lane] = bsum;
    else part1[int64_t(nb) * G::NW1 + int64_t(blockIdx.x) * C + wn * 32 + lane] = bsum;
  }
  }  // WG
}

}  // namespace conv
}  // namespace sel

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using namespace sel;
using namespace sel::conv;

namespace {

// Fused residual-unit forward instances: (C, K, R) = (32, 7, 128), (64, 7, 64).
template <int C, int K, int R>
int launch_ru_thin(const Args& a, const void* in, const void* w1p, const float* b1, const void* w2p,
                   const float* b2, void* h, void* out, hipStream_t s) {
  using RU = RuThin<C, K, R>;
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  const int64_t target = 1024;
  const int64_t tpb = tiles_per_block(ntiles, target);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));  // multiple of 8 (XCD map)
  hipLaunchKernelGGL((k_ru_thin_bf16<C, K, R>), dim3(nb), dim3(256), RU::LDS, s, a,
                     static_cast<const __bf16*>(in), static_cast<const __bf16*>(w1p), b1,
                     static_cast<const __bf16*>(w2p), b2, static_cast<__bf16*>(h), static_cast<__bf16*>(out),
                     int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// fused 32-channel residual unit: one round of resident workgroups, each
// walking an XCD-contiguous range of sample-aligned tiles
template <int R, bool BWD>
int64_t ru32_tiles_per_block(int64_t ntiles) {
  static const int64_t slots = resident_blocks(BWD ? (const void*)k_ru32_bwd<R> : (const void*)k_ru32_fwd<R>, 256,
                                               BWD ? Ru32<R>::LDS_BWD : Ru32<R>::LDS_FWD) / 8 * 8;
  const int64_t target = slots > 0 ? slots : 1024;
  return tiles_per_block(ntiles, target);
}

template <int R>
int launch_ru32_fwd(const Args& a, const void* x, const void* w1p, const float* b1, const void* w2p,
                    const float* b2, void* h, void* out, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  const int64_t tpb = ru32_tiles_per_block<R, false>(ntiles);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));
  hipLaunchKernelGGL(k_ru32_fwd<R>, dim3(nb), dim3(256), Ru32<R>::LDS_FWD, s, a, static_cast<const __bf16*>(x),
                     static_cast<const __bf16*>(w1p), b1, static_cast<const __bf16*>(w2p), b2,
                     static_cast<__bf16*>(h), static_cast<__bf16*>(out), int(tpb), tune(15));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int launch_ru32_fwd4(const Args& a, const void* x, const void* w1p, const float* b1, const void* w2p,
                     const float* b2, void* h, void* out, hipStream_t s) {
  constexpr int R = 256;
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  static const int64_t slots = resident_blocks((const void*)k_ru32_fwd4<R>, 256, Ru32F4<R>::LDS) / 8 * 8;
  const int64_t target = slots > 0 ? slots : 1024;
  const int64_t tpb = tiles_per_block(ntiles, target);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));
  hipLaunchKernelGGL(k_ru32_fwd4<R>, dim3(nb), dim3(256), Ru32F4<R>::LDS, s, a, static_cast<const __bf16*>(x),
                     static_cast<const __bf16*>(w1p), b1, static_cast<const __bf16*>(w2p), b2,
                     static_cast<__bf16*>(h), static_cast<__bf16*>(out), int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int R>
int launch_ru64_fwd(const Args& a, const void* x, const void* w1p, const float* b1, const void* w2p,
                    const float* b2, void* h, void* out, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  static const int64_t slots = resident_blocks((const void*)k_ru64_fwd<R>, 256, Ru64<R>::LDS) / 8 * 8;
  const int64_t target = tune(24) > 0 ? tune(24) : (slots > 0 ? slots : 1024);
  const int64_t tpb = tiles_per_block(ntiles, target);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));
  hipLaunchKernelGGL(k_ru64_fwd<R>, dim3(nb), dim3(256), Ru64<R>::LDS, s, a, static_cast<const __bf16*>(x),
                     static_cast<const __bf16*>(w1p), b1, static_cast<const __bf16*>(w2p), b2,
                     static_cast<__bf16*>(h), static_cast<__bf16*>(out), int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int R>
int launch_ru64_bwd(const Args& a, const void* g, const void* h, const void* x, const void* wd1, const void* wd2,
                    void* gh, void* gx, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  static const int64_t slots = resident_blocks((const void*)k_ru64_bwd<R>, 256, Ru64B<R>::LDS) / 8 * 8;
  const int64_t target = slots > 0 ? slots : 1024;
  const int64_t tpb = tiles_per_block(ntiles, target);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));
  hipLaunchKernelGGL(k_ru64_bwd<R>, dim3(nb), dim3(256), Ru64B<R>::LDS, s, a, static_cast<const __bf16*>(g),
                     static_cast<const __bf16*>(h), static_cast<const __bf16*>(x), static_cast<const __bf16*>(wd1),
                     static_cast<const __bf16*>(wd2), static_cast<__bf16*>(gh), static_cast<__bf16*>(gx), int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

template <int R>
int launch_ru32_bwd(const Args& a, const void* g, const void* h, const void* x, const void* wd1, const void* wd2,
                    void* gh, void* gx, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0) return SEL_OK;
  const int64_t tpb = ru32_tiles_per_block<R, true>(ntiles);
  const unsigned nb = unsigned(blocks_for8(ntiles, tpb));
  hipLaunchKernelGGL(k_ru32_bwd<R>, dim3(nb), dim3(256), Ru32<R>::LDS_BWD, s, a, static_cast<const __bf16*>(g),
                     static_cast<const __bf16*>(h), static_cast<const __bf16*>(x), static_cast<const __bf16*>(wd1),
                     static_cast<const __bf16*>(wd2), static_cast<__bf16*>(gh), static_cast<__bf16*>(gx), int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// fused 32-channel backward with the weight gradients: one block per partial
template <int R>
int ru32w_blocks(int64_t ntiles, int64_t& tpb) {
  static const int64_t slots = resident_blocks((const void*)k_ru32_bwdw<R>, 256, Ru32W<R>::LDS) / 8 * 8;
  const int64_t target = tune(35) > 0 ? tune(35) : (slots > 0 ? slots : 512);
  tpb = tiles_per_block(ntiles, target);
  return int(blocks_for8(ntiles, tpb));
}

template <int R>
int launch_ru32_bwdw(const Args& a, const void* g, const void* h, const void* x, const void* wd1, const void* wd2,
                     void* gx, float* part1, float* part2, int nsplit, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  int64_t tpb = 1;
  const int nb = ru32w_blocks<R>(ntiles, tpb);
  SEL_REQUIRE(nb == nsplit, SEL_ERR_ARG, "sel_resunit_bwd_wgrad: nsplit %d, this shape needs %d", nsplit, nb);
  hipLaunchKernelGGL(k_ru32_bwdw<R>, dim3(unsigned(nb)), dim3(256), Ru32W<R>::LDS, s, a, static_cast<const __bf16*>(g),
                     static_cast<const __bf16*>(h), static_cast<const __bf16*>(x), static_cast<const __bf16*>(wd1),
                     static_cast<const __bf16*>(wd2), static_cast<__bf16*>(gx), part1, part2, int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// fused 64-channel backward with the weight gradients: one 512-thread block per
// CU (its LDS planes), one partial per block
template <int R, bool WG = true>
int ru64w_blocks(int64_t ntiles, int64_t& tpb) {
  // (the occupancy query needs the kernel's 159 KB of dynamic LDS allowed first)
  static const int64_t slots =
      hipFuncSetAttribute((const void*)k_ru64_bwdw<R, WG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(Ru64W<R>::LDS)) == hipSuccess
          ? resident_blocks((const void*)k_ru64_bwdw<R, WG>, 512, Ru64W<R>::LDS) / 8 * 8
          : 0;
  const int64_t target = tune(40) > 0 ? tune(40) : (slots > 0 ? slots : 256);
  tpb = tiles_per_block(ntiles, target);
  return int(blocks_for8(ntiles, tpb));
}

template <int R, bool WG = true>
int launch_ru64_bwdw(const Args& a, const void* g, const void* h, const void* x, const void* wd1, const void* wd2,
                     void* gx, float* part1, float* part2, int nsplit, hipStream_t s) {
  const int64_t ntiles = (a.rows / a.T) * ((a.T + R - 1) / R);
  if (ntiles == 0 && !WG) return SEL_OK;
  int64_t tpb = 1;
  const int nb = ru64w_blocks<R, WG>(ntiles, tpb);
  SEL_REQUIRE(!WG || nb == nsplit, SEL_ERR_ARG, "sel_resunit_bwd_wgrad: nsplit %d, this shape needs %d", nsplit, nb);
  SEL_HIP(hipFuncSetAttribute((const void*)k_ru64_bwdw<R, WG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              int(Ru64W<R>::LDS)));
  hipLaunchKernelGGL((k_ru64_bwdw<R, WG>), dim3(unsigned(nb)), dim3(512), Ru64W<R>::LDS, s, a,
                     static_cast<const __bf16*>(g), static_cast<const __bf16*>(h), static_cast<const __bf16*>(x),
                     static_cast<const __bf16*>(wd1), static_cast<const __bf16*>(wd2), static_cast<__bf16*>(gx), part1,
                     part2, int(tpb));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

bool ru_fused_ok(const Args& a) {
  return (a.C == 32 || a.C == 64) && a.N == a.C && a.K == 7 && a.pad == (a.K - 1) * a.dil &&
         a.pad_mode == SEL_PAD_ZERO && a.in_elu == 1 && (a.K - 1) * a.dil <= F4_HALOMAX &&
         (a.bias_period == 0 || a.bias_period == a.N) && ru_region_ok(int64_t(a.T) * a.C * 2);
}

}  // namespace

extern "C" {

/* Fused residual unit forward (residual_unit.py:43-46): h = conv1(ELU(x)) and
 * out = x + conv1x1(ELU(h)) in one pass (bf16, C = N in {32, 64}, or 128 where
 * the (16, 128) k_conv_wss tile applies, K = 7, causal
 * zero pad, ELU prologue; d1 describes conv1, its bias_period 0 or N).  Returns
 * SEL_ERR_UNSUPPORTED for other shapes (callers then use two sel_conv_fwd calls). */
int sel_resunit_fwd(const sel_conv_desc* d1, int dtype, const void* x, const void* w1pack, const float* b1,
                    const void* w2pack, const float* b2, void* h, void* out, sel_stream_t stream) {
  if (int rc = check_desc(d1)) return rc;
  const Args a = to_args(d1);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // 128 channels (round 6): the (16, 128) k_conv_wss tile with the 1x1 in its
  // epilogue, where conv1 alone runs on that tile (T = 2000, >= 65536 rows:
  // the C3 RU128 units); tune key 69 = 1: off
  if (dtype == SEL_BF16 && a.C == 128 && fwd4_choice(a, false) == 30 && wss_pw_ok(a))
    return launch_wss_pw(a, x, w1pack, b1, w2pack, b2, h, out, s);
  SEL_REQUIRE(dtype == SEL_BF16 && ru_fused_ok(a), SEL_ERR_UNSUPPORTED,
              "sel_resunit_fwd: fused path needs bf16, C = N in {32, 64} (128 on the (16, 128) k_conv_wss tile), "
              "K = 7, causal zero pad, ELU prologue");
  // tune key 56 = 1: 128-row tiles (4 resident workgroups per CU instead of 3):
  // 66-67 -> 58.6-59 us per unit in tools/ru_bench.py, which re-reads the same
  // input, but 69.5 -> 72.6 us inside the profiled C3 step, so off
  // tune key 70 = 1: k_ru32_fwd4 (W1 in LDS, four blocks per CU; bit-identical)
  if (a.C == 32 && tune(70) == 1 && tune(56) != 1) return launch_ru32_fwd4(a, x, w1pack, b1, w2pack, b2, h, out, s);
  if (a.C == 32)
    return tune(56) == 1 ? launch_ru32_fwd<128>(a, x, w1pack, b1, w2pack, b2, h, out, s)
                         : launch_ru32_fwd<256>(a, x, w1pack, b1, w2pack, b2, h, out, s);
  // tune key 24 < 0: the LDS-staged k_ru_thin_bf16 (round 2) instead of k_ru64_fwd
  if (tune(24) < 0) return launch_ru_thin<64, 7, 64>(a, x, w1pack, b1, w2pack, b2, h, out, s);
  return launch_ru64_fwd<128>(a, x, w1pack, b1, w2pack, b2, h, out, s);
}

/* Fused residual unit backward at 32 channels (residual_unit.py:43-46 adjoint):
 * gh = (W2^T g) * ELU'(h), gx = conv1^T(gh) * ELU'(x) + g in one launch.  d1 is
 * the forward conv1 descriptor; wd1 / wd2 the dgrad-packed weights; gh may be
 * null (only the weight gradient of conv1 needs it). */
int sel_resunit_bwd(const sel_conv_desc* d1, int dtype, const void* g, const void* h, const void* x,
                    const void* wd1pack, const void* wd2pack, void* gh, void* gx, sel_stream_t stream) {
  if (int rc = check_desc(d1)) return rc;
  const Args a = to_args(d1);
  SEL_REQUIRE(dtype == SEL_BF16 && ru_fused_ok(a), SEL_ERR_UNSUPPORTED,
              "sel_resunit_bwd: fused path needs bf16, C = N in {32, 64}, K = 7, causal zero pad, ELU prologue");
  SEL_REQUIRE(g && h && x && wd1pack && wd2pack && gx, SEL_ERR_ARG, "null pointer");
  // tune key 41 = 1 (without gh): the eight-wave LDS-staged form, k_ru64_bwdw's
  // gx role on all waves (one workgroup per CU: measured slower than two
  // four-wave k_ru64_bwd workgroups, 82-83 vs 72 us per unit at C3)
  if (a.C == 64 && gh == nullptr && tune(41) == 1)
    return launch_ru64_bwdw<128, false>(a, g, h, x, wd1pack, wd2pack, gx, nullptr, nullptr, 0,
                                        reinterpret_cast<hipStream_t>(stream));
  if (a.C == 64)
    return launch_ru64_bwd<128>(a, g, h, x, wd1pack, wd2pack, gh, gx, reinterpret_cast<hipStream_t>(stream));
  return launch_ru32_bwd<128>(a, g, h, x, wd1pack, wd2pack, gh, gx, reinterpret_cast<hipStream_t>(stream));
}

int sel_resunit_wgrad_splits(const sel_conv_desc* d1, int dtype) {
  if (int rc = check_desc(d1)) return rc;
  const Args a = to_args(d1);
  SEL_REQUIRE(dtype == SEL_BF16 && ru_fused_ok(a) && a.rows > 0, SEL_ERR_UNSUPPORTED,
              "sel_resunit_bwd_wgrad: needs bf16, C = N in {32, 64}, K = 7, causal zero pad, ELU prologue");
  int64_t tpb = 1;
  const int64_t ntiles = (a.rows / a.T) * ((a.T + 127) / 128);
  return a.C == 64 ? ru64w_blocks<128>(ntiles, tpb) : ru32w_blocks<128>(ntiles, tpb);
}

int sel_resunit_bwd_wgrad(const sel_conv_desc* d1, int dtype, const void* g, const void* h, const void* x,
                          const void* wd1pack, const void* wd2pack, void* gx, float* part1, float* part2, int nsplit,
                          sel_stream_t stream) {
  if (int rc = check_desc(d1)) return rc;
  const Args a = to_args(d1);
  SEL_REQUIRE(dtype == SEL_BF16 && ru_fused_ok(a) && a.rows > 0, SEL_ERR_UNSUPPORTED,
              "sel_resunit_bwd_wgrad: needs bf16, C = N in {32, 64}, K = 7, causal zero pad, ELU prologue");
  SEL_REQUIRE(g && h && x && wd1pack && wd2pack && gx && part1 && part2, SEL_ERR_ARG, "null pointer");
  if (a.C == 64)
    return launch_ru64_bwdw<128>(a, g, h, x, wd1pack, wd2pack, gx, part1, part2, nsplit,
                                 reinterpret_cast<hipStream_t>(stream));
  return launch_ru32_bwdw<128>(a, g, h, x, wd1pack, wd2pack, gx, part1, part2, nsplit,
                               reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
