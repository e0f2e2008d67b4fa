// Training-mode residual VQ under data parallelism: the EMA codebook update
// (layers/vq_module.py:74-80) split at the point where its statistics exist on
// their own, so that ranks can exchange them (sel.dist.gather_blocks) before any
// codebook is written.  vq_ema.hip's fused update folds each code's sum straight
// into embed_avg; here
//
//   sel_rvq_ema_stats   k_sync_residuals  the residuals r_s (S, N, D), exactly as
//                                         vq_ema.hip's k_ema_residuals forms them;
//                       k_sync_sums       one wave per (stage, code, segment): scans
//                                         the segment's idx 64 entries at a time,
//                                         ballots the matches, adds the matching
//                                         residual rows in ascending row order and
//                                         counts them (popcount of the ballots: an
//                                         integer, no histogram pass).  Writes the
//                                         sums and the count of EVERY code, member
//                                         rows or not, into block g of `stats`.
//   sel_rvq_ema_apply   k_sync_fold       blocks summed left to right in block
//                                         order (fp32 sums, counts in double), then
//                                         the decay fmaf of the fused update;
//                       k_sync_finish     k_ema_finish's arithmetic and tree.
//
// With one segment and one block the pair writes the bits of sel_rvq_ema_update.
// No float atomics anywhere: every output element has one owner and the order of
// its additions depends on idx and the block order alone.
#include <algorithm>

#include "sel_common.h"

namespace sel {
namespace vqsync {

constexpr int MAXD = 256;  // sel_rvq_fwd's
constexpr int MAXS = 16;   // the fused forward's SM
constexpr int CW = 4;      // waves (codes) per k_sync_sums block
constexpr int UN = 4;      // member rows in flight per wave in k_sync_sums
constexpr int FT = 256;    // k_sync_fold / k_sync_finish threads
constexpr int64_t MAXSEG = int64_t(1) << 24;  // rows per segment: the fp32 count stays exact
constexpr int MAXNSEG = 65535;                // gridDim.z

struct Stages {
  sel_rvq_ema_stage s[MAXS];
};

__global__ __launch_bounds__(256) void k_sync_residuals(const float* __restrict__ x, int64_t N, int D,
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
      // (clamped as in k_ema_residuals: a caller's mistake reads inside the stack)
      const int k = int(std::min<int64_t>(std::max<int64_t>(idx[int64_t(s) * N + row], 0), K - 1));
      const float q = embeds[(int64_t(s) * D + d) * K + k];
      // the forward's row update: diff = q - r; qst = r + diff; r <- r - qst
      const float diff = q - rv;
      const float qst = rv + diff;
      rv = rv - qst;
    }
  }
}

// Q dims per lane: 1 for D <= 64 (the recipe's), else MAXD / 64.  Grid: x codes
// / CW, y stages, z segments; segment g is the rows [g * n, (g + 1) * n).
template <int Q>
__global__ __launch_bounds__(64 * CW) void k_sync_sums(const float* __restrict__ res, int64_t N, int64_t n, int D,
                                                      int S, int K, const int64_t* __restrict__ idx,
                                                      float* __restrict__ stats) {
  const int s = blockIdx.y;
  const int g = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * CW + (threadIdx.x >> 6);
  if (k >= K) return;  // wave-uniform; the kernel has no barrier
  const int64_t base = int64_t(g) * n;
  const int64_t* __restrict__ ix = idx + int64_t(s) * N + base;
  const float* __restrict__ R = res + (int64_t(s) * N + base) * D;
  float acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.f;
  int cnt = 0;
  // the whole segment is scanned (the count is the scan's own); the next chunk's
  // indices are requested before this chunk's rows
  int64_t cur = lane < n ? ix[lane] : -1;
  for (int64_t b = 0; b < n; b += 64) {
    const int64_t nn = b + 64 + lane;
    const int64_t nxt = nn < n ? ix[nn] : -1;
    unsigned long long mask = __ballot(cur == int64_t(k));
    cur = nxt;
    cnt += __popcll(mask);
    // the member rows of this chunk, UN at a time: their loads are independent
    // and go out together, the additions stay in ascending row order
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
  float* __restrict__ out = stats + (int64_t(g) * S + s) * int64_t(D + 1) * K;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = lane + 64 * q;
    if (d < D) out[int64_t(d) * K + k] = acc[q];
  }
  if (lane == 0) out[int64_t(D) * K + k] = float(cnt);
}

// one thread per element of a stage's (D + 1, K) block: rows 0..D-1 into
// embed_avg, row D into cluster_size
__global__ __launch_bounds__(FT) void k_sync_fold(const float* __restrict__ stats, int nblk, int D, int S, int K,
                                                  Stages tab, float decay, float omd) {
  const int s = blockIdx.y;
  const sel_rvq_ema_stage st = tab.s[s];
  if (!st.update) return;
  const int64_t dk = int64_t(D) * K;
  const int64_t per = dk + K;          // one stage of one block
  const int64_t stride = per * S;      // one block
  const float* __restrict__ p = stats + int64_t(s) * per;
  for (int64_t i = int64_t(blockIdx.x) * FT + threadIdx.x; i < per; i += int64_t(gridDim.x) * FT) {
    if (i < dk) {
      float sum = p[i];
      for (int b = 1; b < nblk; ++b) sum = sum + p[int64_t(b) * stride + i];
      st.embed_avg[i] = __fmaf_rn(sum, omd, st.embed_avg[i] * decay);
    } else {
      const int64_t k = i - dk;
      double c = double(p[i]);
      for (int b = 1; b < nblk; ++b) c += double(p[int64_t(b) * stride + i]);
      st.cluster_size[k] = __fmaf_rn(float(c), omd, st.cluster_size[k] * decay);
    }
  }
}

// k_ema_finish's arithmetic: blocks (x) of one stage (y) each sum the stage's
// cluster sizes in the same order and normalise their slice of the (D, K) codebook
__global__ __launch_bounds__(FT) void k_sync_finish(int D, int K, Stages tab, float eps) {
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

}  // namespace vqsync
}  // namespace sel

using namespace sel;
using namespace sel::vqsync;

extern "C" {

size_t sel_rvq_ema_stats_floats(int D, int S, int K) {
  if (D < 0 || S < 0 || K < 0) return 0;  // (the calls reject the shape themselves)
  return size_t(S) * (size_t(D) + 1) * size_t(K);
}

size_t sel_rvq_ema_stats_workspace(int64_t N, int D, int S, int K) {
  (void)K;
  if (N < 0 || D < 0 || S < 0) return 0;
  return res_bytes(N, D, S);
}

int sel_rvq_ema_stats(const float* x, int64_t N, int D, const float* embeds, int S, int K, const int64_t* idx,
                      int nseg, float* stats, void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(N >= 1 && D > 0 && D <= MAXD && S > 0 && S <= MAXS && K > 0, SEL_ERR_ARG,
              "bad rvq ema stats shape N=%lld D=%d S=%d K=%d", (long long)N, D, S, K);
  SEL_REQUIRE(nseg >= 1 && nseg <= MAXNSEG && N % nseg == 0 && N / nseg <= MAXSEG, SEL_ERR_ARG,
              "rvq ema stats: %d segments do not divide N=%lld into equal parts of at most 2^24 rows", nseg,
              (long long)N);
  SEL_REQUIRE(ws_bytes >= sel_rvq_ema_stats_workspace(N, D, S, K), SEL_ERR_WORKSPACE,
              "rvq ema stats workspace too small");
  SEL_REQUIRE(x && embeds && idx && stats && ws, SEL_ERR_ARG, "rvq ema stats: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* res = static_cast<float*>(ws);
  const int64_t total = N * D;
  hipLaunchKernelGGL(k_sync_residuals, dim3(unsigned(std::min<int64_t>(1 << 20, (total + 255) / 256))), dim3(256), 0,
                     st, x, N, D, embeds, S, K, idx, res);
  SEL_LAUNCH_CHECK();
  const int64_t n = N / nseg;
  const dim3 sgrid(unsigned((K + CW - 1) / CW), unsigned(S), unsigned(nseg));
  if (D <= 64)
    hipLaunchKernelGGL(k_sync_sums<1>, sgrid, dim3(64 * CW), 0, st, res, N, n, D, S, K, idx, stats);
  else
    hipLaunchKernelGGL(k_sync_sums<MAXD / 64>, sgrid, dim3(64 * CW), 0, st, res, N, n, D, S, K, idx, stats);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_rvq_ema_apply(const float* stats, int nblk, int D, int S, int K, const sel_rvq_ema_stage* stages,
                      float decay, float eps, sel_stream_t stream) {
  SEL_REQUIRE(D > 0 && D <= MAXD && S > 0 && S <= MAXS && K > 0, SEL_ERR_ARG, "bad rvq ema apply shape D=%d S=%d K=%d",
              D, S, K);
  SEL_REQUIRE(nblk >= 1, SEL_ERR_ARG, "rvq ema apply: %d blocks", nblk);
  SEL_REQUIRE(stages, SEL_ERR_ARG, "rvq ema apply: null stage table");
  SEL_REQUIRE(stats, SEL_ERR_ARG, "rvq ema apply: null pointer");
  Stages tab{};
  bool any = false;
  for (int s = 0; s < S; ++s) {
    tab.s[s] = stages[s];
    if (!tab.s[s].update) continue;
    any = true;
    SEL_REQUIRE(tab.s[s].embed && tab.s[s].cluster_size && tab.s[s].embed_avg, SEL_ERR_ARG,
                "rvq ema apply: null buffer in stage %d", s);
  }
  if (!any) return SEL_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float omd = 1.f - decay;
  const int64_t dk = int64_t(D) * K;
  hipLaunchKernelGGL(k_sync_fold, dim3(unsigned(std::min<int64_t>(1024, (dk + K + FT - 1) / FT)), unsigned(S)),
                     dim3(FT), 0, st, stats, nblk, D, S, K, tab, decay, omd);
  SEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sync_finish, dim3(unsigned(std::min<int64_t>(64, (dk + 4 * FT - 1) / (4 * FT))), unsigned(S)),
                     dim3(FT), 0, st, D, K, tab, eps);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
