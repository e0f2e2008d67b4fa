// Training-mode residual VQ: the EMA codebook update (layers/vq_module.py:74-80)
// for all stages of one forward on gfx950.
//
// The assignment is sel_rvq_fwd's (vq.hip): every stage picks its code with its
// own pre-update codebook, so this file only adds the update.  Three launches:
//
//   k_ema_residuals  one thread per (row, dim) carries its element through the
//                    stages with the forward's three fp32 operations and writes
//                    r_s (S, N, D) to the workspace: the strided 4-byte code
//                    gather from the (D, K) layout happens once per (row, stage).
//   k_ema_sums       one wave per (stage, code): scans idx[s, :] 64 entries at
//                    a time, ballots the matches and adds the matching residual
//                    rows in ascending row order (lanes over d, coalesced row
//                    reads), then folds the sum into embed_avg and the count
//                    into cluster_size.  No atomics: one wave owns a code, and
//                    the order of its additions depends on idx alone.
//   k_ema_finish     n = sum_k cluster_size (fp64, fixed tree), the Laplace
//                    smoothing and embed = embed_avg / cs.
//
// The stacked codebooks the forward read are never written: the backward reads them.
#include <algorithm>

#include "sel_common.h"

namespace sel {
namespace vqema {

constexpr int MAXD = 256;  // sel_rvq_fwd's
constexpr int MAXS = 16;   // the fused forward's SM
constexpr int CW = 4;      // waves (codes) per k_ema_sums block
constexpr int UN = 4;      // member rows in flight per wave in k_ema_sums
constexpr int FT = 256;    // k_ema_finish threads

struct Stages {
  sel_rvq_ema_stage s[MAXS];
};

__global__ __launch_bounds__(256) void k_ema_residuals(const float* __restrict__ x, int64_t N, int D,
                                                       const float* __restrict__ embeds, int S, int K,
                                                       const int64_t* __restrict__ idx,
                                                       float* __restrict__ res) {
  const int64_t total = N * D;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t row = i / D;
    const int d = int(i - row * D);
    float rv = x[i];
    for (int s = 0; s < S; ++s) {
      res[int64_t(s) * total + i] = rv;
      // (an index outside the codebook cannot come from sel_rvq_fwd; clamped so
      // that a caller's mistake reads inside the stack)
      const int k = int(std::min<int64_t>(std::max<int64_t>(idx[int64_t(s) * N + row], 0), K - 1));
      const float q = embeds[(int64_t(s) * D + d) * K + k];
      // the forward's row update: diff = q - r; qst = r + diff; r <- r - qst
      const float diff = q - rv;
      const float qst = rv + diff;
      rv = rv - qst;
    }
  }
}

// Q dims per lane: 1 for D <= 64 (the recipe's), else MAXD / 64
template <int Q>
__global__ __launch_bounds__(64 * CW) void k_ema_sums(const float* __restrict__ res, int64_t N, int D, int K,
                                                     const int64_t* __restrict__ idx,
                                                     const int32_t* __restrict__ counts, Stages tab, float decay,
                                                     float omd) {
  const int s = blockIdx.y;
  const sel_rvq_ema_stage st = tab.s[s];
  if (!st.update) return;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * CW + (threadIdx.x >> 6);
  if (k >= K) return;  // wave-uniform; the kernel has no barrier
  const int cnt = counts[int64_t(s) * K + k];
  const int64_t* __restrict__ ix = idx + int64_t(s) * N;
  const float* __restrict__ R = res + int64_t(s) * N * D;
  float acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.f;
  // counts is the histogram of idx: the scan ends at the code's last member row
  // (a code with no rows reads nothing and decays with a zero sum); the next
  // chunk's indices are requested before this chunk's rows
  int left = cnt;
  int64_t cur = (left > 0 && lane < N) ? ix[lane] : -1;
  for (int64_t b = 0; b < N && left > 0; b += 64) {
    const int64_t nn = b + 64 + lane;
    const int64_t nxt = nn < N ? ix[nn] : -1;
    unsigned long long mask = __ballot(cur == int64_t(k));
    cur = nxt;
    left -= __popcll(mask);
    // the member rows of this chunk, UN at a time: their loads are independent
    // and go out together, the additions stay in ascending row order (a code
    // that holds most rows is one long chain of dependent adds, not of loads)
    while (mask) {
      int j[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        j[u] = __ffsll(mask) - 1;  // -1 once the chunk's matches are used up
        mask &= mask - 1;
      }
      float v[UN][Q];
#pragma unroll
      for (int u = 0; u < UN; ++u)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int d = lane + 64 * q;
          v[u][q] = (j[u] >= 0 && d < D) ? R[(b + j[u]) * D + d] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < UN; ++u)
        if (j[u] >= 0) {
#pragma unroll
          for (int q = 0; q < Q; ++q) acc[q] += v[u][q];
        }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = lane + 64 * q;
    if (d < D) {
      const int64_t o = int64_t(d) * K + k;
      st.embed_avg[o] = __fmaf_rn(acc[q], omd, st.embed_avg[o] * decay);
    }
  }
  if (lane == 0) st.cluster_size[k] = __fmaf_rn(float(cnt), omd, st.cluster_size[k] * decay);
}

// blocks (x) of one stage (y) each sum the stage's cluster sizes in the same
// order and normalise their slice of the (D, K) codebook
__global__ __launch_bounds__(FT) void k_ema_finish(int D, int K, Stages tab, float eps) {
  __shared__ double red[16];
  __shared__ double n_sh;
  const sel_rvq_ema_stage st = tab.s[blockIdx.y];
  if (!st.update) return;  // block-uniform
  double v = 0.0;
  for (int k = threadIdx.x; k < K; k += FT) v += double(st.cluster_size[k]);
  v = block_sum<double>(v, red);
  if (threadIdx.x == 0) n_sh = v;
  __syncthreads();
  const float n = float(n_sh);
  const float den = n + float(K) * eps;
  const int64_t total = int64_t(D) * K;
  for (int64_t i = int64_t(blockIdx.x) * FT + threadIdx.x; i < total; i += int64_t(gridDim.x) * FT) {
    const int k = int(i % K);
    const float cs = (st.cluster_size[k] + eps) / den * n;
    st.embed[i] = st.embed_avg[i] / cs;
  }
}

inline size_t res_bytes(int64_t N, int D, int S) {
  return (size_t(S) * size_t(N) * size_t(D) * sizeof(float) + 255) & ~size_t(255);
}

}  // namespace vqema
}  // namespace sel

using namespace sel;
using namespace sel::vqema;

extern "C" {

size_t sel_rvq_ema_workspace(int64_t N, int D, int S, int K) {
  (void)K;
  if (N < 0 || D < 0 || S < 0) return 0;  // (sel_rvq_ema_update rejects the shape itself)
  return res_bytes(N, D, S);
}

int sel_rvq_ema_update(const float* x, int64_t N, int D, const float* embeds, int S, int K, const int64_t* idx,
                       const int32_t* counts, const sel_rvq_ema_stage* stages, float decay, float eps, void* ws,
                       size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(N >= 1 && D > 0 && D <= MAXD && S > 0 && S <= MAXS && K > 0, SEL_ERR_ARG,
              "bad rvq ema shape N=%lld D=%d S=%d K=%d", (long long)N, D, S, K);
  SEL_REQUIRE(ws_bytes >= sel_rvq_ema_workspace(N, D, S, K), SEL_ERR_WORKSPACE, "rvq ema workspace too small");
  SEL_REQUIRE(stages, SEL_ERR_ARG, "rvq ema: null stage table");
  SEL_REQUIRE(x && embeds && idx && counts && ws, SEL_ERR_ARG, "rvq ema: null pointer");
  Stages tab{};
  bool any = false;
  for (int s = 0; s < S; ++s) {
    tab.s[s] = stages[s];
    if (!tab.s[s].update) continue;
    any = true;
    SEL_REQUIRE(tab.s[s].embed && tab.s[s].cluster_size && tab.s[s].embed_avg, SEL_ERR_ARG,
                "rvq ema: null buffer in stage %d", s);
  }
  if (!any) return SEL_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* res = static_cast<float*>(ws);
  const int64_t total = N * D;
  hipLaunchKernelGGL(k_ema_residuals, dim3(unsigned(std::min<int64_t>(1 << 20, (total + 255) / 256))), dim3(256), 0,
                     st, x, N, D, embeds, S, K, idx, res);
  SEL_LAUNCH_CHECK();
  const float omd = 1.f - decay;
  const dim3 sgrid(unsigned((K + CW - 1) / CW), unsigned(S));
  if (D <= 64)
    hipLaunchKernelGGL(k_ema_sums<1>, sgrid, dim3(64 * CW), 0, st, res, N, D, K, idx, counts, tab, decay, omd);
  else
    hipLaunchKernelGGL(k_ema_sums<MAXD / 64>, sgrid, dim3(64 * CW), 0, st, res, N, D, K, idx, counts, tab, decay,
                       omd);
  SEL_LAUNCH_CHECK();
  const int64_t dk = int64_t(D) * K;
  hipLaunchKernelGGL(k_ema_finish, dim3(unsigned(std::min<int64_t>(64, (dk + 4 * FT - 1) / (4 * FT))), unsigned(S)),
                     dim3(FT), 0, st, D, K, tab, eps);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
