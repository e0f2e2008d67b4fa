// What the two streaming step kernels share (stream.hip: sel_conv_step,
// hfg_step.hip: sel_hfg_conv_step): the block geometry constants, the 16-byte
// operand fragments, the MFMA issue and the slot table of their pool forms.
// Their operand gathers differ (groups, pitches, activation) and stay with each
// kernel.
#pragma once
#include "conv_common.h"

namespace sel {
namespace step {
using namespace sel::conv;

constexpr int MAX_NW = 8;     // waves per block (reduction split)
constexpr int BIG_RT = 4;     // row tiles per block on large row counts
constexpr int RT_SWITCH = 64; // row tiles (of 16 rows) from which a block takes BIG_RT of them

template <typename T> struct Frag;
template <> struct Frag<__bf16> { typedef bf16x8 type; static constexpr int E = 8; };
template <> struct Frag<float> { typedef floatx4 type; static constexpr int E = 4; };

__device__ __forceinline__ floatx4 mma(bf16x8 a, bf16x8 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// four 16x16x4 products: product j takes element j of every lane's vector, i.e.
// the reduction index 16*chunk + 4*(lane >> 4) + j on both operands
__device__ __forceinline__ floatx4 mma(floatx4 a, floatx4 b, floatx4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
  return c;
}

// The launch coordinates, read in the __global__ function itself (where the
// compiler folds them against the kernel's launch bounds) and handed to the
// shared body of a step kernel and its pool form.
struct Launch {
  unsigned bid, nblk, tid, bdim;
};

// The slot table of a pool launch (sel_conv_step_pool, sel_hfg_conv_step_pool):
// sample i of the dense in / res / out buffers carries its state in row
// slots[i] of carry / carry_out.
struct PoolArgs {
  const int* slots;
  const int* n_active;
  int nslots, cap;
};

// samples of this tick: min(*n_active, capacity), never negative
__device__ __forceinline__ int pool_count(const PoolArgs& p) { return min(max(*p.n_active, 0), p.cap); }
// a list entry outside the pool makes its sample absent
__device__ __forceinline__ bool pool_slot_ok(const PoolArgs& p, int slot) {
  return unsigned(slot) < unsigned(p.nslots);
}

}  // namespace step
}  // namespace sel
