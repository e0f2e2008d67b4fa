// Residual VQ for a streaming hop (include/sel.h: sel_rvq_step,
// sel_rvq_lookup_step): the quantizer and the codebook lookup as stateless,
// capturable step launches on few rows -- a B = 1 hop has one row, a 16-stream
// tick sixteen.  sel_rvq_fwd (vq.hip) is built for thousands of rows in 16-row
// blocks and also produces the histogram, SSE, loss and perplexity of training.
//
// Quantize: one workgroup per row, threads over codes, the residual in LDS.
// Per (row, stage, code) the arithmetic is k_rvq_fwd's: |r|^2 with lanes over d
// and wave_sum, dot and |e_k|^2 as fmaf chains over d ascending from the same
// loaded column, dist = (|r|^2 - 2 dot) + |e_k|^2, lowest index on ties, then
// q = e_idx, qst = r + (q - r), r <- r - qst, zq += qst.  A row's bits depend on
// the row alone, so any grouping of rows into blocks gives the same result.
//   k_rvq_step_col: D = 64, K = 1024 (the product codebooks).  512 threads, two
//     adjacent codes each (one 8-byte load per row d), the codes' 64-value
//     columns in registers (128 VGPRs of the 256 a thread has at 2 waves per
//     SIMD).  A column does not depend on the
//     residual: the next stage's columns are requested as soon as this stage's
//     dot products have consumed the registers, and are in flight while the
//     argmin -> gather -> update chain of this stage resolves.
//   k_rvq_step_any: every accepted shape.  256 threads, 4 codes per thread per
//     pass of 1024 codes, columns read inside the d loop.
// No atomics, no workspace; idx is written per stage, so S is unbounded.
//
// Wire format (include/sel.h, wire version 1): both quantize kernels have a
// WIRE instance (sel_rvq_step_wire) in which wave 0, where the pick already
// lives, also shifts it into the row's bit-packed record and stores the bytes
// that fill; the lookup has one (sel_rvq_lookup_wire_step) that takes its ids
// out of such records instead of an int64 buffer.  A row owns its bytes.
//
// Datagrams (wire version 2): a third instance of each kernel (DGRAM:
// sel_rvq_step_dgram, sel_rvq_lookup_dgram_step).  The quantizer stops its chain
// after the sample's stage budget, read from device memory, and writes a header
// and truncated records into the sample's region; the lookup reads the stage
// count from the header and, for a sample that is lost, sums the record its
// slot holds from the last valid hop.  The arithmetic is the one body above.
#include <algorithm>

#include "sel_common.h"

namespace sel {
namespace vqstep {

constexpr int MAXD = 256;
constexpr int COL_D = 64, COL_K = 1024;  // k_rvq_step_col's shape
constexpr int COL_T = 512;                // its threads: COL_K / COL_T codes each
constexpr int ANY_T = 256, ANY_CPT = 4;  // k_rvq_step_any: threads, codes per thread per pass

__device__ __forceinline__ bool better(float d, int k, float bd, int bk) {
  return d < bd || (d == bd && k < bk);
}

__device__ __forceinline__ void wave_argmin(float& d0, int& k0) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float d1 = __shfl_xor(d0, o, 64);
    const int k1 = __shfl_xor(k0, o, 64);
    if (better(d1, k1, d0, k0)) {
      d0 = d1;
      k0 = k1;
    }
  }
}

// rows of this launch: all of them, or the first min(max(*n_active, 0), cap) samples
__device__ __forceinline__ int64_t active_rows(const int32_t* n_active, int cap, int T, int64_t rows) {
  return n_active ? int64_t(min(max(*n_active, 0), cap)) * T : rows;
}

// ---- the packed record of a row: field s in bits [s * bits, (s + 1) * bits), bit i of the
// record = bit i % 8 of byte i / 8; ceil(S * bits / 8) bytes, the pad bits zero ----
__host__ __device__ __forceinline__ int wire_bits(int K) {
  int b = 1;
  while (b < 31 && (int64_t(1) << b) < K) ++b;
  return b;
}

template <bool WIRE> struct WireDst {};  // a kernel argument: empty unless the instance packs
template <> struct WireDst<true> {
  uint8_t* wire;  // (rows, frame_bytes)
  int64_t frame_bytes;
  int bits;
};

// The writer's state, the same in every lane of wave 0: at most 7 + 31 bits are
// ever held, whole bytes leave as they fill, so S is unbounded here too.
template <bool WIRE> struct WirePack {
  __device__ __forceinline__ WirePack(const WireDst<WIRE>&, int64_t) {}
};
template <> struct WirePack<true> {
  uint8_t* p;    // the record's next byte
  uint64_t acc;  // fields not yet stored, lowest bit first
  int fill;      // bits in acc: < 8 between stages
  int bits;
  __device__ __forceinline__ WirePack(const WireDst<true>& w, int64_t row)
      : p(w.wire + row * w.frame_bytes), acc(0), fill(0), bits(w.bits) {}
  __device__ __forceinline__ WirePack(uint8_t* record, int bits_) : p(record), acc(0), fill(0), bits(bits_) {}
  __device__ __forceinline__ void put(int k, bool writer) {
    acc |= uint64_t(uint32_t(k)) << fill;
    fill += bits;
    while (fill >= 8) {
      if (writer) *p = uint8_t(acc);
      ++p;
      acc >>= 8;
      fill -= 8;
    }
  }
  __device__ __forceinline__ void finish(bool writer) {  // the last partial byte, zero-padded
    if (fill > 0 && writer) *p = uint8_t(acc);
  }
};

// ---- the datagram of a sample (include/sel.h, wire version 2): the header {2, s, seq low, seq
// high} and the sample's rows_per_sample records of s <= S fields each, inside the sample's own
// dgram_stride bytes.  The DGRAM instances take this in WireDst's place. ----
__host__ __device__ __forceinline__ int64_t record_bytes(int stages, int bits) {
  return (int64_t(stages) * bits + 7) / 8;
}

struct DgramDst {
  uint8_t* dgram;         // sample i owns [i * stride, (i + 1) * stride)
  int64_t stride;
  const int32_t* stages;  // device, one per sample; null: S
  const int32_t* seq;     // device, one per sample; null: 0
  int bits;
};
template <bool WIRE, bool DGRAM> struct StepDst { using type = WireDst<WIRE>; };
template <> struct StepDst<true, true> { using type = DgramDst; };

// The row's packer and the stages it runs.  The budget comes from memory but is the same in the
// whole block: through readfirstlane it is a scalar, so the stage loop and the prefetch branch
// that test it stay scalar branches.  The block of a sample's first row writes the header.
template <bool WIRE, bool DGRAM>
__device__ __forceinline__ WirePack<WIRE> open_pack(const typename StepDst<WIRE, DGRAM>::type& w, int64_t row, int T,
                                                    int S, int& ns) {
  if constexpr (DGRAM) {
    const int64_t i = row / T;
    const int r = int(row - i * T);
    const int budget = w.stages ? w.stages[i] : S;
    ns = __builtin_amdgcn_readfirstlane(min(max(budget, 1), S));
    uint8_t* base = w.dgram + i * w.stride;
    if (r == 0 && threadIdx.x == 0) {
      const uint32_t q = w.seq ? uint32_t(w.seq[i]) : 0u;
      base[0] = uint8_t(SEL_DGRAM_VERSION);
      base[1] = uint8_t(ns);
      base[2] = uint8_t(q);
      base[3] = uint8_t(q >> 8);
    }
    return WirePack<true>(base + SEL_DGRAM_HEADER_BYTES + r * record_bytes(ns, w.bits), w.bits);
  } else {
    return WirePack<WIRE>(w, row);
  }
}

// What both quantize kernels do once every thread holds its best (distance, code):
// the block argmin (NW waves), then the first wave applies the pick to the row.
// A row whose distances are all NaN keeps the initial 0x7fffffff: the pick is
// forced to code 0 before anything is read through it.
template <int NW, bool WIRE>
__device__ __forceinline__ void pick_and_update(float bd, int bk, int D, int K, const float* __restrict__ E,
                                                float* res, float* acc, float* red_d, int* red_k,
                                                int64_t* __restrict__ idx_out, int64_t idx_off,
                                                WirePack<WIRE>& pack) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  wave_argmin(bd, bk);
  if (lane == 0) {
    red_d[wave] = bd;
    red_k[wave] = bk;
  }
  __syncthreads();
  if (wave == 0) {
    float d0 = lane < NW ? red_d[lane] : __builtin_inff();
    int k0 = lane < NW ? red_k[lane] : 0x7fffffff;
    wave_argmin(d0, k0);
    if (unsigned(k0) >= unsigned(K)) k0 = 0;
    if constexpr (WIRE) {  // idx is optional next to the record
      if (lane == 0 && idx_out) *idx_out = int64_t(k0) + idx_off;
      pack.put(k0, lane == 0);
    } else {
      if (lane == 0) *idx_out = int64_t(k0) + idx_off;
    }
    for (int d = lane; d < D; d += 64) {
      const float q = E[int64_t(d) * K + k0];
      const float rv = res[d];
      const float diff = q - rv;
      const float qst = rv + diff;
      res[d] = rv - qst;
      acc[d] += qst;
    }
  }
  __syncthreads();
}

template <bool WIRE, bool DGRAM = false>
__global__ __launch_bounds__(COL_T) void k_rvq_step_col(const float* __restrict__ z, int64_t rows, int T,
                                                        const float* __restrict__ embeds, int S,
                                                        const int32_t* __restrict__ n_active, int cap, int flatten,
                                                        int64_t* __restrict__ idx, float* __restrict__ zq,
                                                        typename StepDst<WIRE, DGRAM>::type wire) {
  constexpr int D = COL_D, K = COL_K, NW = COL_T / 64, C = COL_K / COL_T;
  __shared__ __align__(16) float res[D];
  __shared__ float acc[D];
  __shared__ float red_d[NW];
  __shared__ int red_k[NW];
  __shared__ float xn;
  const int64_t row = blockIdx.x;
  if (row >= active_rows(n_active, cap, T, rows)) return;  // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ns = S;  // the stages this row runs: all of them, or (DGRAM) its sample's budget
  WirePack<WIRE> pack = open_pack<WIRE, DGRAM>(wire, row, T, S, ns);

  // One stage's codebook as a buffer resource: a load is then one VGPR byte
  // offset (the thread's code pair) plus a scalar offset (the row d) -- 64
  // separate 64-bit addresses would cost as many registers as the columns.
  auto load_cols = [&](int s, float (&e)[C][D]) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(embeds + int64_t(s) * D * K), 0, D * K * int(sizeof(float)), 0x00020000);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float2 v = __builtin_bit_cast(
          float2, __builtin_amdgcn_raw_buffer_load_b64(rs, tid * C * int(sizeof(float)), d * K * int(sizeof(float)), 0));
      e[0][d] = v.x;
      e[1][d] = v.y;
    }
  };
  static_assert(C == 2, "one 8-byte load per row d covers the thread's two adjacent codes");
  float e[C][D];  // the columns of codes C * tid + j
  load_cols(0, e);
  if (tid < D) {
    res[tid] = z[row * D + tid];
    acc[tid] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < ns; ++s) {
    const float* __restrict__ E = embeds + int64_t(s) * D * K;
    if (wave == 0) {
      float v = 0.f;
      v = fmaf(res[lane], res[lane], v);
      v = wave_sum(v);
      if (lane == 0) xn = v;
    }
    float dot[C], en[C];
#pragma unroll
    for (int j = 0; j < C; ++j) dot[j] = en[j] = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < D; d4 += 4) {
      const float4 r4 = *reinterpret_cast<const float4*>(res + d4);
      const float rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < C; ++j) {
          en[j] = fmaf(e[j][d4 + i], e[j][d4 + i], en[j]);
          dot[j] = fmaf(rr[i], e[j][d4 + i], dot[j]);
        }
    }
    // the registers are free: the next stage's columns, in flight during the pick
    // (the empty asm pins the finished sums here: the compiler otherwise sinks
    // the fmaf chains below the loads, towards their use after the barrier, and
    // both stages' columns are live at once)
#pragma unroll
    for (int j = 0; j < C; ++j) asm volatile("" : "+v"(dot[j]), "+v"(en[j]) : : "memory");
    if (s + 1 < ns) load_cols(s + 1, e);
    __syncthreads();
    float bd = __builtin_inff();
    int bk = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < C; ++j) {  // ascending codes
      const float dist = (xn - 2.f * dot[j]) + en[j];
      if (better(dist, C * tid + j, bd, bk)) {
        bd = dist;
        bk = C * tid + j;
      }
    }
    pick_and_update<NW, WIRE>(bd, bk, D, K, E, res, acc, red_d, red_k,
                              WIRE && !idx ? nullptr : idx + int64_t(s) * rows + row, flatten ? int64_t(s) * K : 0,
                              pack);
  }
  if constexpr (WIRE) pack.finish(tid == 0);
  if constexpr (DGRAM) {  // the stages not run: ids the lookup skips
    if (idx)
      for (int s = ns + tid; s < S; s += COL_T) idx[int64_t(s) * rows + row] = -1;
  }
  if (zq && tid < D) zq[row * D + tid] = acc[tid];
}

template <bool WIRE, bool DGRAM = false>
__global__ __launch_bounds__(ANY_T) void k_rvq_step_any(const float* __restrict__ z, int64_t rows, int T, int D,
                                                        const float* __restrict__ embeds, int S, int K,
                                                        const int32_t* __restrict__ n_active, int cap, int flatten,
                                                        int64_t* __restrict__ idx, float* __restrict__ zq,
                                                        typename StepDst<WIRE, DGRAM>::type wire) {
  constexpr int NW = ANY_T / 64;
  __shared__ float res[MAXD];
  __shared__ float acc[MAXD];
  __shared__ float red_d[NW];
  __shared__ int red_k[NW];
  __shared__ float xn;
  const int64_t row = blockIdx.x;
  if (row >= active_rows(n_active, cap, T, rows)) return;  // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ns = S;  // the stages this row runs: all of them, or (DGRAM) its sample's budget
  WirePack<WIRE> pack = open_pack<WIRE, DGRAM>(wire, row, T, S, ns);
  for (int d = tid; d < D; d += ANY_T) {
    res[d] = z[row * D + d];
    acc[d] = 0.f;
  }
  __syncthreads();

  for (int s = 0; s < ns; ++s) {
    const float* __restrict__ E = embeds + int64_t(s) * D * K;
    if (wave == 0) {
      float v = 0.f;
      for (int d = lane; d < D; d += 64) v = fmaf(res[d], res[d], v);
      v = wave_sum(v);
      if (lane == 0) xn = v;
    }
    __syncthreads();
    const float x2 = xn;
    float bd = __builtin_inff();
    int bk = 0x7fffffff;
    for (int64_t kb = 0; kb < K; kb += ANY_T * ANY_CPT) {
      float dot[ANY_CPT], en[ANY_CPT];
      int64_t col[ANY_CPT];  // a dead code reads column 0 and is not scored
#pragma unroll
      for (int j = 0; j < ANY_CPT; ++j) {
        dot[j] = en[j] = 0.f;
        const int64_t k = kb + tid + j * ANY_T;
        col[j] = k < K ? k : 0;
      }
      for (int d = 0; d < D; ++d) {
        const float rv = res[d];
        const float* __restrict__ Ed = E + int64_t(d) * K;
#pragma unroll
        for (int j = 0; j < ANY_CPT; ++j) {
          const float ev = Ed[col[j]];
          en[j] = fmaf(ev, ev, en[j]);
          dot[j] = fmaf(rv, ev, dot[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < ANY_CPT; ++j) {
        const int64_t k = kb + tid + j * ANY_T;
        if (k >= K) continue;
        const float dist = (x2 - 2.f * dot[j]) + en[j];
        if (better(dist, int(k), bd, bk)) {
          bd = dist;
          bk = int(k);
        }
      }
    }
    pick_and_update<NW, WIRE>(bd, bk, D, K, E, res, acc, red_d, red_k,
                              WIRE && !idx ? nullptr : idx + int64_t(s) * rows + row, flatten ? int64_t(s) * K : 0,
                              pack);
  }
  if constexpr (WIRE) pack.finish(tid == 0);
  if constexpr (DGRAM) {
    if (idx)
      for (int s = ns + tid; s < S; s += ANY_T) idx[int64_t(s) * rows + row] = -1;
  }
  if (zq)
    for (int d = tid; d < D; d += ANY_T) zq[row * D + d] = acc[d];
}

// ---- lookup: out[row] = sum over stages of codebook[idx[s, row]], stages ascending ----
template <typename TO> __device__ __forceinline__ TO to_out(float v);
template <> __device__ __forceinline__ float to_out<float>(float v) { return v; }
template <> __device__ __forceinline__ __bf16 to_out<__bf16>(float v) { return static_cast<__bf16>(v); }  // RNE

struct LookupArgs {
  const int64_t* idx;
  const float* codebook;
  const float* mean;
  const float* scale;
  const int32_t* n_active;
  int64_t rows, ncodes;
  int T, S, D, cap;
};

constexpr int LK_T = 256;

// WIRE: the ids come out of the rows' packed records (LookupArgs::idx is unused,
// ncodes = S * K): a thread streams its row's bytes through the accumulator the
// packer uses, byte loads only, so the buffer may have any alignment.
template <bool WIRE> struct WireSrc {};
template <> struct WireSrc<true> {
  const uint8_t* wire;  // (rows, frame_bytes)
  int64_t* idx_out;     // (S, rows) flattened ids, -1 for a refused field; may be null
  int64_t frame_bytes;
  int K, bits;
};

// DGRAM: the records come out of the samples' datagrams, or, for a sample that is
// lost (flagged, or with a header this receiver refuses), out of the record its slot
// holds from the last valid hop: hold row = {stages held (0: none), that record}.
struct DgramSrc {
  const uint8_t* dgram;  // sample i owns [i * stride, (i + 1) * stride)
  int64_t stride;
  const int32_t* slots;  // device, one per sample; null: slot i
  const int32_t* lost;   // device, one per sample; null: none
  uint8_t* hold;         // (nslots, hold_stride); may be null
  int64_t hold_stride;
  int nslots;
  int64_t* idx_out;
  int K, bits;
};
template <bool WIRE, bool DGRAM> struct LookupSrc { using type = WireSrc<WIRE>; };
template <> struct LookupSrc<true, true> { using type = DgramSrc; };

// V = 4: one thread per 4 channels (D % 4 == 0, 16-byte aligned operands); V = 1: per channel
template <typename TO, int V, bool WIRE, bool DGRAM = false>
__global__ __launch_bounds__(LK_T) void k_rvq_lookup_step(LookupArgs a, TO* __restrict__ out,
                                                          typename LookupSrc<WIRE, DGRAM>::type w) {
  const int per_row = a.D / V;
  const int64_t live = active_rows(a.n_active, a.cap, a.T, a.rows);
  const int64_t i0 = int64_t(blockIdx.x) * LK_T;
  if (i0 / per_row >= live) return;  // block-uniform: the whole block lies beyond the active rows
  const int64_t i = i0 + threadIdx.x;
  const int64_t row = i / per_row;
  if (row >= live) return;
  const int d0 = int(i % per_row) * V;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  bool first = true;
  const uint8_t* p = nullptr;  // WIRE: the record's next byte, the bytes left in it, the bits held
  int64_t left = 0;
  uint64_t held = 0;
  int fill = 0;
  int ns = a.S;  // the stages of this row's record
  if constexpr (DGRAM) {
    const int64_t smp = row / a.T;
    const int r = int(row - smp * a.T);
    const uint8_t* base = w.dgram + smp * w.stride;
    const int slot = w.slots ? w.slots[smp] : int(smp);
    const bool held = w.hold && unsigned(slot) < unsigned(w.nslots);  // else: lost with nothing held
    int got = 0;  // the header's stage count; a flagged sample's bytes are not looked at
    if (!w.lost || w.lost[smp] == 0) {
      if (base[0] == SEL_DGRAM_VERSION) got = base[1];
    }
    if (got >= 1 && got <= a.S) {  // valid: the row's own record; the last row's is kept
      ns = got;
      left = record_bytes(ns, w.bits);
      p = base + SEL_DGRAM_HEADER_BYTES + r * left;
      if (held && d0 == 0 && r == a.T - 1) {
        uint8_t* h = w.hold + slot * w.hold_stride;
        h[0] = uint8_t(ns);
        for (int64_t b = 0; b < left; ++b) h[1 + b] = p[b];
      }
    } else if (held) {  // lost: every row decodes the held record; hold is only read
      const uint8_t* h = w.hold + slot * w.hold_stride;
      ns = min(int(h[0]), a.S);
      left = record_bytes(ns, w.bits);
      p = h + 1;
    } else {
      ns = 0;  // the empty sum
    }
  } else if constexpr (WIRE) {
    p = w.wire + row * w.frame_bytes;
    left = w.frame_bytes;
  }
  for (int s = 0; s < ns; ++s) {
    int64_t id;
    if constexpr (WIRE) {
      while (fill < w.bits && left > 0) {  // never beyond the row's own bytes
        held |= uint64_t(*p++) << fill;
        fill += 8;
        --left;
      }
      const uint32_t k = uint32_t(held) & ((1u << w.bits) - 1u);
      held >>= w.bits;
      fill -= w.bits;
      id = k < uint32_t(w.K) ? int64_t(s) * w.K + k : -1;  // a field >= K is refused
      if (w.idx_out && d0 == 0) w.idx_out[int64_t(s) * a.rows + row] = id;
    } else {
      id = a.idx[int64_t(s) * a.rows + row];
    }
    if (id < 0 || id >= a.ncodes) continue;  // contributes zero; nothing is read through it
    const float* __restrict__ c = a.codebook + id * a.D + d0;
    float v[V];
    if constexpr (V == 4) {
      const float4 c4 = *reinterpret_cast<const float4*>(c);
      v[0] = c4.x; v[1] = c4.y; v[2] = c4.z; v[3] = c4.w;
    } else {
      v[0] = c[0];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = first ? v[j] : __fadd_rn(acc[j], v[j]);
    first = false;
  }
  if constexpr (DGRAM) {  // the fields that are not there
    if (w.idx_out && d0 == 0)
      for (int s = ns; s < a.S; ++s) w.idx_out[int64_t(s) * a.rows + row] = -1;
  }
  if (a.mean) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = __fdiv_rn(__fsub_rn(acc[j], a.mean[d0 + j]), a.scale[d0 + j]);
  }
  TO* __restrict__ o = out + row * a.D + d0;
  if constexpr (V == 4 && sizeof(TO) == 4) {
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else if constexpr (V == 4) {
    union {
      __bf16 h[4];
      uint2 u;
    } p;
#pragma unroll
    for (int j = 0; j < 4; ++j) p.h[j] = to_out<__bf16>(acc[j]);
    *reinterpret_cast<uint2*>(o) = p.u;
  } else {
    o[0] = to_out<TO>(acc[0]);
  }
}

}  // namespace vqstep
}  // namespace sel

using namespace sel;
using namespace sel::vqstep;

namespace {

struct DgramCtl {  // what sel_rvq_step_dgram passes beside sel_rvq_step_wire's arguments
  const int32_t* stages;
  const int32_t* seq;
  int64_t stride;
};

// sel_rvq_step, sel_rvq_step_wire and sel_rvq_step_dgram: one set of checks, one dispatch
template <bool WIRE, bool DGRAM = false>
int rvq_step_launch(const char* who, const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S,
                    int K, const int32_t* n_active, int flatten, int64_t* idx, float* zq, uint8_t* wire,
                    sel_stream_t stream, DgramCtl g = {}) {
  SEL_REQUIRE(rows >= 1 && rows_per_sample >= 1 && rows % rows_per_sample == 0, SEL_ERR_ARG,
              "%s: rows (%d) must be a positive multiple of rows_per_sample (%d)", who, rows, rows_per_sample);
  SEL_REQUIRE(D > 0 && D <= MAXD && K > 0 && S > 0, SEL_ERR_ARG, "%s: bad shape D=%d (1..%d) K=%d S=%d", who, D, MAXD,
              K, S);
  if constexpr (WIRE)
    SEL_REQUIRE(z && embeds && wire, SEL_ERR_ARG, "%s: null z / embeds / wire", who);
  else
    SEL_REQUIRE(z && embeds && idx, SEL_ERR_ARG, "%s: null z / embeds / idx", who);
  SEL_REQUIRE(zq != z, SEL_ERR_ARG, "%s: zq aliases z", who);
  typename StepDst<WIRE, DGRAM>::type w;
  if constexpr (WIRE) {
    const int bits = wire_bits(K);
    SEL_REQUIRE(bits <= 31 && (int64_t(1) << bits) >= K, SEL_ERR_ARG, "%s: K=%d needs more than 31 bits per field", who,
                K);
    SEL_REQUIRE(int64_t(S) * K <= (int64_t(1) << 40), SEL_ERR_ARG, "%s: S*K = %lld ids out of range", who,
                (long long)(int64_t(S) * K));
    if constexpr (DGRAM) {
      SEL_REQUIRE(S <= 255, SEL_ERR_ARG, "%s: S=%d does not fit the header's stage byte (<= 255)", who, S);
      const int64_t need = SEL_DGRAM_HEADER_BYTES + rows_per_sample * record_bytes(S, bits);
      SEL_REQUIRE(g.stride >= need, SEL_ERR_ARG, "%s: dgram_stride %lld is below the full datagram's %lld bytes", who,
                  (long long)g.stride, (long long)need);
      w = DgramDst{wire, g.stride, g.stages, g.seq, bits};
    } else {
      w.wire = wire;
      w.frame_bytes = (int64_t(S) * bits + 7) / 8;
      w.bits = bits;
    }
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int cap = rows / rows_per_sample;
  if (D == COL_D && K == COL_K)
    hipLaunchKernelGGL((k_rvq_step_col<WIRE, DGRAM>), dim3(unsigned(rows)), dim3(COL_T), 0, s, z, int64_t(rows),
                       rows_per_sample, embeds, S, n_active, cap, flatten, idx, zq, w);
  else
    hipLaunchKernelGGL((k_rvq_step_any<WIRE, DGRAM>), dim3(unsigned(rows)), dim3(ANY_T), 0, s, z, int64_t(rows),
                       rows_per_sample, D, embeds, S, K, n_active, cap, flatten, idx, zq, w);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

// sel_rvq_lookup_step and sel_rvq_lookup_wire_step: idx, or the packed records of K-code stages
template <bool WIRE, bool DGRAM = false>
int rvq_lookup_launch(const char* who, const int64_t* idx, typename LookupSrc<WIRE, DGRAM>::type w, int rows,
                      int rows_per_sample, int S,
                      int64_t ncodes, int D, const float* codebook, const float* mean, const float* scale,
                      const int32_t* n_active, int out_dtype, void* out, sel_stream_t stream) {
  SEL_REQUIRE(rows >= 1 && rows_per_sample >= 1 && rows % rows_per_sample == 0, SEL_ERR_ARG,
              "%s: rows (%d) must be a positive multiple of rows_per_sample (%d)", who, rows, rows_per_sample);
  SEL_REQUIRE(S > 0 && D > 0 && ncodes > 0, SEL_ERR_ARG, "%s: bad shape S=%d D=%d ncodes=%lld", who, S, D,
              (long long)ncodes);
  SEL_REQUIRE(ncodes <= (int64_t(1) << 40) / D, SEL_ERR_ARG, "%s: codebook of %lld x %d out of range", who,
              (long long)ncodes, D);
  if constexpr (DGRAM) {
    SEL_REQUIRE(w.dgram && codebook && out, SEL_ERR_ARG, "%s: null dgram / codebook / out", who);
    const int64_t need = SEL_DGRAM_HEADER_BYTES + rows_per_sample * record_bytes(S, w.bits);
    SEL_REQUIRE(w.stride >= need, SEL_ERR_ARG, "%s: dgram_stride %lld is below the full datagram's %lld bytes", who,
                (long long)w.stride, (long long)need);
    SEL_REQUIRE(!w.hold || (w.hold_stride >= 1 + record_bytes(S, w.bits) && w.nslots >= 1), SEL_ERR_ARG,
                "%s: hold rows of %lld bytes x %d slots, a row needs %lld and one slot at least", who,
                (long long)w.hold_stride, w.nslots, (long long)(1 + record_bytes(S, w.bits)));
  } else if constexpr (WIRE)
    SEL_REQUIRE(w.wire && codebook && out, SEL_ERR_ARG, "%s: null wire / codebook / out", who);
  else
    SEL_REQUIRE(idx && codebook && out, SEL_ERR_ARG, "%s: null idx / codebook / out", who);
  SEL_REQUIRE((mean == nullptr) == (scale == nullptr), SEL_ERR_ARG, "%s: mean and scale come together or not at all",
              who);
  SEL_REQUIRE(out_dtype == SEL_F32 || out_dtype == SEL_BF16, SEL_ERR_ARG, "%s: out_dtype must be fp32 or bf16", who);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = D % 4 == 0 && al16(codebook) && al16(out) && al16(mean) && al16(scale);
  LookupArgs a{idx, codebook, mean, scale, n_active, int64_t(rows), ncodes, rows_per_sample, S, D,
               rows / rows_per_sample};
  const int64_t threads = int64_t(rows) * (vec ? D / 4 : D);
  SEL_REQUIRE(threads / LK_T < (int64_t(1) << 31) - 1, SEL_ERR_ARG, "%s: rows * D out of range", who);
  const dim3 grid(unsigned((threads + LK_T - 1) / LK_T));
  if (out_dtype == SEL_F32) {
    if (vec) hipLaunchKernelGGL((k_rvq_lookup_step<float, 4, WIRE, DGRAM>), grid, dim3(LK_T), 0, s, a, static_cast<float*>(out), w);
    else hipLaunchKernelGGL((k_rvq_lookup_step<float, 1, WIRE, DGRAM>), grid, dim3(LK_T), 0, s, a, static_cast<float*>(out), w);
  } else {
    if (vec) hipLaunchKernelGGL((k_rvq_lookup_step<__bf16, 4, WIRE, DGRAM>), grid, dim3(LK_T), 0, s, a, static_cast<__bf16*>(out), w);
    else hipLaunchKernelGGL((k_rvq_lookup_step<__bf16, 1, WIRE, DGRAM>), grid, dim3(LK_T), 0, s, a, static_cast<__bf16*>(out), w);
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // namespace

extern "C" {

int sel_rvq_step(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                 const int32_t* n_active, int flatten, int64_t* idx, float* zq, sel_stream_t stream) {
  return rvq_step_launch<false>("sel_rvq_step", z, rows, rows_per_sample, D, embeds, S, K, n_active, flatten, idx, zq,
                                nullptr, stream);
}

int sel_rvq_step_wire(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                      const int32_t* n_active, int flatten, int64_t* idx, float* zq, uint8_t* wire,
                      sel_stream_t stream) {
  return rvq_step_launch<true>("sel_rvq_step_wire", z, rows, rows_per_sample, D, embeds, S, K, n_active, flatten, idx,
                               zq, wire, stream);
}

int sel_rvq_lookup_step(const int64_t* idx, int rows, int rows_per_sample, int S, int64_t ncodes, int D,
                        const float* codebook, const float* mean, const float* scale, const int32_t* n_active,
                        int out_dtype, void* out, sel_stream_t stream) {
  return rvq_lookup_launch<false>("sel_rvq_lookup_step", idx, WireSrc<false>{}, rows, rows_per_sample, S, ncodes, D,
                                  codebook, mean, scale, n_active, out_dtype, out, stream);
}

int sel_rvq_lookup_wire_step(const uint8_t* wire, int rows, int rows_per_sample, int S, int K, int D,
                             const float* codebook, const float* mean, const float* scale, const int32_t* n_active,
                             int out_dtype, void* out, int64_t* idx_out, sel_stream_t stream) {
  const char* who = "sel_rvq_lookup_wire_step";
  SEL_REQUIRE(S > 0 && K > 0, SEL_ERR_ARG, "%s: bad shape S=%d K=%d", who, S, K);
  const int bits = wire_bits(K);
  SEL_REQUIRE(bits <= 31 && (int64_t(1) << bits) >= K, SEL_ERR_ARG, "%s: K=%d needs more than 31 bits per field", who, K);
  SEL_REQUIRE(int64_t(S) * K <= (int64_t(1) << 40), SEL_ERR_ARG, "%s: S*K = %lld ids out of range", who,
              (long long)(int64_t(S) * K));
  WireSrc<true> w{wire, idx_out, (int64_t(S) * bits + 7) / 8, K, bits};
  return rvq_lookup_launch<true>(who, nullptr, w, rows, rows_per_sample, S, int64_t(S) * K, D, codebook, mean, scale,
                                 n_active, out_dtype, out, stream);
}

int sel_rvq_step_dgram(const float* z, int rows, int rows_per_sample, int D, const float* embeds, int S, int K,
                       const int32_t* n_active, const int32_t* stages, const int32_t* seq, int flatten, int64_t* idx,
                       float* zq, uint8_t* dgram, int64_t dgram_stride, sel_stream_t stream) {
  return rvq_step_launch<true, true>("sel_rvq_step_dgram", z, rows, rows_per_sample, D, embeds, S, K, n_active,
                                     flatten, idx, zq, dgram, stream, DgramCtl{stages, seq, dgram_stride});
}

int sel_rvq_lookup_dgram_step(const uint8_t* dgram, int64_t dgram_stride, int rows, int rows_per_sample, int S, int K,
                              int D, const float* codebook, const float* mean, const float* scale,
                              const int32_t* n_active, const int32_t* slots, const int32_t* lost, uint8_t* hold,
                              int64_t hold_stride, int nslots, int out_dtype, void* out, int64_t* idx_out,
                              sel_stream_t stream) {
  const char* who = "sel_rvq_lookup_dgram_step";
  SEL_REQUIRE(S > 0 && S <= 255 && K > 0, SEL_ERR_ARG, "%s: bad shape S=%d (1..255) K=%d", who, S, K);
  const int bits = wire_bits(K);
  SEL_REQUIRE(bits <= 31 && (int64_t(1) << bits) >= K, SEL_ERR_ARG, "%s: K=%d needs more than 31 bits per field", who, K);
  DgramSrc w{dgram, dgram_stride, slots, lost, hold, hold_stride, nslots, idx_out, K, bits};
  return rvq_lookup_launch<true, true>(who, nullptr, w, rows, rows_per_sample, S, int64_t(S) * K, D, codebook, mean,
                                       scale, n_active, out_dtype, out, stream);
}

}  // extern "C"
