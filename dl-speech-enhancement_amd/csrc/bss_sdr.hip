// BSS-eval SDR: torchmetrics 1.2.0 signal_distortion_ratio with
// the direct solve, over the last dim of (B, T) fp32.  Both signals go to fp64
// (minus the row mean with zero_mean) and are scaled to unit norm (the norm
// floored at 1e-6); r[k] = sum_n t[n] t[n + k] and b[k] = sum_n t[n] p[n + k],
// k < L, are the LINEAR correlations (terms with n + k >= T are absent, so lags
// k >= T are 0; torchmetrics' wrapped lags at T < L are not reproduced);
// r[0] += load_diag; sol = toeplitz(r)^-1 b by a Levinson recursion in fp64;
// coh = b . sol and the value is 10 log10(coh / (1 - coh)).
//
// Degenerate rows: 1 - coh <= 0 (preds equal to target up to scale, or T so
// small that L taps fit anything) gives +inf; a silent target (r[0] <= 0, where
// torchmetrics raises on the singular solve) gives NaN in that row and in the
// batch mean, and leaves the other rows alone.
//
// Every entry point validates first, allocates nothing, never synchronises
// with the host and can be captured into a graph.  No atomics: the results are
// the same bits run to run.
#include <cmath>

#include "sel_common.h"

namespace sel {
namespace bss {

constexpr int kMaxTaps = 512;
constexpr int kChunk = 2048;  // samples of n per correlation block

// Ragged batches: row b is its first lengths[b] samples, T stays the
// row stride.  A length above T counts as T, a negative one as 0.
__device__ __forceinline__ int64_t row_len(const int64_t* __restrict__ lens, int64_t b, int64_t T) {
  const int64_t n = lens[b];
  return n > T ? T : (n < 0 ? 0 : n);
}

// One block per row: the two means in fp64 (launched only with zero_mean).
template <bool VAR>
__global__ __launch_bounds__(256) void k_bss_means(const float* __restrict__ p, const float* __restrict__ t,
                                                   int64_t stride, const int64_t* __restrict__ lens,
                                                   double* __restrict__ means) {
  __shared__ double red[16];
  const int64_t b = blockIdx.x;
  const float* __restrict__ pr = p + b * stride;
  const float* __restrict__ tr = t + b * stride;
  int64_t T = stride;  // the row's own length
  if constexpr (VAR) T = row_len(lens, b, stride);
  double sp = 0.0, st = 0.0;
  for (int64_t i = threadIdx.x; i < T; i += blockDim.x) {
    sp += double(pr[i]);
    st += double(tr[i]);
  }
  sp = block_sum<double>(sp, red);
  st = block_sum<double>(st, red);
  if (threadIdx.x == 0) {
    means[2 * b] = sp / double(T);
    means[2 * b + 1] = st / double(T);
  }
}

// Block (c, b) owns n in [c kChunk, min((c + 1) kChunk, T)) of row b.  It
// stages (t, p)[n0 .. n0 + kChunk + kMaxTaps) in LDS as fp64 pairs, already
// centred; a sample at or past T is zero AFTER centring (not -mean: the
// correlations are linear).  Thread k < L sums t[n] t[n + k] and t[n] p[n + k]
// over the chunk.  The pair at n + k is one 16-byte read, consecutive across
// lanes.  t[n] is wave-uniform: each lane reads one of 64 consecutive t[n] and
// the wave passes them round with v_readlane (as an LDS broadcast read per n
// they would cost half as many LDS cycles again as the pairs do).  The loop
// runs to the next multiple of 64 past the chunk's end: t[n] is 0 there.
// part: (B, chunks, 2L + 1) = r, b, sum p^2.  With lengths a chunk that starts at
// or past the row's end writes zero partials (the solve sums every chunk).
template <bool VAR>
__global__ __launch_bounds__(kMaxTaps) void k_bss_corr(const float* __restrict__ p, const float* __restrict__ t,
                                                       int64_t stride, const int64_t* __restrict__ lens, int L,
                                                       const double* __restrict__ means, double* __restrict__ part) {
  __shared__ double2 s[kChunk + kMaxTaps];  // .x = t, .y = p
  __shared__ double red[16];
  const int64_t b = blockIdx.y;
  const int64_t n0 = int64_t(blockIdx.x) * kChunk;
  const int tid = threadIdx.x, lane = tid & 63;
  int64_t T = stride;  // the row's own length
  if constexpr (VAR) {
    T = row_len(lens, b, stride);
    if (n0 >= T) {  // block-uniform
      double* __restrict__ z = part + (b * gridDim.x + blockIdx.x) * int64_t(2 * L + 1);
      if (tid < L) {
        z[tid] = 0.0;
        z[L + tid] = 0.0;
      }
      if (tid == 0) z[2 * L] = 0.0;
      return;
    }
  }
  const double mp = means ? means[2 * b] : 0.0, mt = means ? means[2 * b + 1] : 0.0;
  const float* __restrict__ pr = p + b * stride;
  const float* __restrict__ tr = t + b * stride;
  for (int i = tid; i < kChunk + kMaxTaps; i += blockDim.x) {
    const int64_t g = n0 + i;
    double2 v = {0.0, 0.0};
    if (g < T) v = {double(tr[g]) - mt, double(pr[g]) - mp};
    s[i] = v;
  }
  __syncthreads();
  const int cn = int(T - n0 < kChunk ? T - n0 : kChunk);
  double pp = 0.0;
  for (int i = tid; i < cn; i += blockDim.x) pp += s[i].y * s[i].y;
  pp = block_sum<double>(pp, red);
  double* __restrict__ out = part + (b * gridDim.x + blockIdx.x) * int64_t(2 * L + 1);
  if (tid == 0) out[2 * L] = pp;
  double r0 = 0.0, b0 = 0.0, r1 = 0.0, b1 = 0.0;  // two chains each: one does not hide the fp64 FMA latency
  const double2* __restrict__ sk = s + tid;       // tid < 512: n + tid stays inside s
  for (int nb = 0; nb < cn; nb += 64) {
    const double av = s[nb + lane].x;
    const int alo = __double2loint(av), ahi = __double2hiint(av);
#pragma unroll
    for (int j = 0; j < 64; j += 2) {
      const double a0 = __hiloint2double(__builtin_amdgcn_readlane(ahi, j), __builtin_amdgcn_readlane(alo, j));
      const double a1 =
          __hiloint2double(__builtin_amdgcn_readlane(ahi, j + 1), __builtin_amdgcn_readlane(alo, j + 1));
      const double2 v0 = sk[nb + j], v1 = sk[nb + j + 1];
      r0 = fma(a0, v0.x, r0);
      b0 = fma(a0, v0.y, b0);
      r1 = fma(a1, v1.x, r1);
      b1 = fma(a1, v1.y, b1);
    }
  }
  if (tid < L) {
    out[tid] = r0 + r1;
    out[L + tid] = b0 + b1;
  }
}

// One block of L threads (rounded up to a wave) per row: the partials summed
// in chunk order, the scaling, then the Levinson recursion for R sol = b with
// one vector element per thread.  Step m extends the order-(m - 1) predictor a
// (a[0] = 1, R a = (E, 0, ..)) and the solution x of the leading m x m system
// to order m:
//   k = -(r[m] + sum_{1 <= i < m} a[i] r[m - i]) / E,  a[i] += k a[m - i],  a[m] = k,  E *= 1 - k^2
//   q = (b[m] - sum_{i < m} x[i] r[m - i]) / E,         x[i] += q a[m - i],  x[m] = q
// Both sums use only the state of the step before, so they share one reduction.
template <bool VAR>
__global__ __launch_bounds__(kMaxTaps) void k_bss_solve(const double* __restrict__ part, int chunks, int L,
                                                        double load_diag, int64_t T,
                                                        const int64_t* __restrict__ lens, double* __restrict__ corr,
                                                        double* __restrict__ dvals, float* __restrict__ vals) {
  __shared__ double r[kMaxTaps], bv[kMaxTaps];
  __shared__ double abuf[2][kMaxTaps];
  __shared__ double red[2][kMaxTaps / 64];
  const int64_t row = blockIdx.x;
  const int i = threadIdx.x;
  const int lane = i & 63, w = i >> 6, nw = blockDim.x >> 6;
  const bool live = i < L;
  const int stride = 2 * L + 1;
  const double* __restrict__ pr = part + row * chunks * int64_t(stride);
  double ri = 0.0, bi = 0.0, pp = 0.0, tt = 0.0;
  for (int c = 0; c < chunks; ++c) {
    const double* __restrict__ q = pr + int64_t(c) * stride;
    if (live) {
      ri += q[i];
      bi += q[L + i];
    }
    tt += q[0];  // ||t||^2 = r_raw[0]
    pp += q[2 * L];
  }
  const double nt = fmax(sqrt(tt), 1e-6), np = fmax(sqrt(pp), 1e-6);
  ri /= nt * nt;
  bi /= nt * np;
  if (i == 0) ri += load_diag;
  if (live && corr) {
    corr[(row * 2) * L + i] = ri;
    corr[(row * 2 + 1) * L + i] = bi;
  }
  r[i] = live ? ri : 0.0;
  bv[i] = live ? bi : 0.0;
  abuf[0][i] = i == 0 ? 1.0 : 0.0;
  __syncthreads();
  const double r0 = r[0];
  double E = r0;
  double ai = i == 0 ? 1.0 : 0.0;
  double xi = i == 0 ? bi / r0 : 0.0;
  int cur = 0;
  for (int m = 1; m < L; ++m) {
    const int nwa = (m >> 6) + 1 < nw ? (m >> 6) + 1 : nw;  // waves that hold an element below m
    const double rm = i < m ? r[m - i] : 0.0;
    double d1 = i >= 1 ? ai * rm : 0.0;
    double d2 = xi * rm;
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    if (lane == 0) {
      red[0][w] = d1;
      red[1][w] = d2;
    }
    __syncthreads();
    d1 = 0.0;
    d2 = 0.0;
    for (int j = 0; j < nwa; ++j) {
      d1 += red[0][j];
      d2 += red[1][j];
    }
    const double k = -(r[m] + d1) / E;
    E *= 1.0 - k * k;
    if (i >= 1 && i < m) ai = fma(k, abuf[cur][m - i], ai);
    if (i == m) ai = k;
    abuf[cur ^ 1][i] = ai;
    __syncthreads();  // also fences red against the next step's writes
    cur ^= 1;
    const double q = (bv[m] - d2) / E;
    if (i <= m) xi = fma(q, abuf[cur][m - i], xi);  // x[m] = 0 + q a[0]
  }
  double coh = block_sum<double>(live ? bi * xi : 0.0, red[0]);
  if (i == 0) {
    double v = 10.0 * log10(coh / (1.0 - coh));
    if (1.0 - coh <= 0.0) v = INFINITY;
    if (!(r0 > 0.0)) v = NAN;  // silent target
    if constexpr (VAR) {
      if (row_len(lens, row, T) < 1) v = NAN;  // an empty row (r0 may be load_diag alone)
    }
    dvals[row] = v;
    vals[row] = float(v);
  }
}

// the batch mean of the fp64 row values by one block, in a fixed order (a strided sum per thread, then a tree)
__global__ __launch_bounds__(256) void k_bss_mean(const double* __restrict__ dvals, int64_t B,
                                                  float* __restrict__ mean) {
  __shared__ double red[16];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) acc += dvals[b];
  acc = block_sum<double>(acc, red);
  if (threadIdx.x == 0) mean[0] = float(acc / double(B));
}

inline int64_t chunks_of(int64_t T) { return (T + kChunk - 1) / kChunk; }

}  // namespace bss
}  // namespace sel

using namespace sel;
using namespace sel::bss;

extern "C" {

int64_t sel_bss_sdr_chunk(void) { return kChunk; }

// fp64: (mean p, mean t) per row, the row values, then the partials (B, chunks, 2L + 1)
size_t sel_bss_sdr_workspace(int64_t B, int64_t T, int filter_length) {
  if (B <= 0 || B > 65535 || T <= 0 || T > (int64_t(1) << 32) || filter_length < 1 || filter_length > kMaxTaps)
    return 0;
  return size_t(B) * (3 + size_t(chunks_of(T)) * size_t(2 * filter_length + 1)) * sizeof(double);
}

namespace {

// sel_bss_sdr and sel_bss_sdr_var: lens == nullptr is the fixed-length call
int bss_sdr(const char* fn, const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lens,
            int filter_length, int zero_mean, double load_diag, float* vals, float* mean, double* corr, void* ws,
            size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(pred && target && vals && ws, SEL_ERR_ARG, "%s: null pointer", fn);
  SEL_REQUIRE(B > 0 && B <= 65535, SEL_ERR_ARG, "%s: B must be in [1, 65535]", fn);
  SEL_REQUIRE(T > 0 && T <= (int64_t(1) << 32), SEL_ERR_ARG, "%s: T must be in [1, 2^32]", fn);
  SEL_REQUIRE(filter_length >= 1 && filter_length <= kMaxTaps, SEL_ERR_ARG, "%s: filter_length must be in [1, %d]",
              fn, kMaxTaps);
  SEL_REQUIRE((zero_mean | 1) == 1, SEL_ERR_ARG, "%s: zero_mean must be 0 or 1", fn);
  SEL_REQUIRE(std::isfinite(load_diag) && load_diag >= 0.0, SEL_ERR_ARG,
              "%s: load_diag must be finite and not negative", fn);
  SEL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, SEL_ERR_ARG, "%s: workspace not 8-byte aligned", fn);
  SEL_REQUIRE(ws_bytes >= sel_bss_sdr_workspace(B, T, filter_length), SEL_ERR_WORKSPACE, "%s: workspace too small",
              fn);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int L = filter_length;
  const int threads = (L + 63) / 64 * 64;
  const int chunks = int(chunks_of(T));
  double* means = static_cast<double*>(ws);
  double* dvals = means + 2 * B;
  double* part = dvals + B;
  const double* cm = zero_mean ? means : static_cast<const double*>(nullptr);
  if (lens) {
    if (zero_mean) {
      hipLaunchKernelGGL(k_bss_means<true>, dim3(unsigned(B)), dim3(256), 0, s, pred, target, T, lens, means);
      SEL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_bss_corr<true>, dim3(unsigned(chunks), unsigned(B)), dim3(threads), 0, s, pred, target, T,
                       lens, L, cm, part);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bss_solve<true>, dim3(unsigned(B)), dim3(threads), 0, s, part, chunks, L, load_diag, T, lens,
                       corr, dvals, vals);
  } else {
    if (zero_mean) {
      hipLaunchKernelGGL(k_bss_means<false>, dim3(unsigned(B)), dim3(256), 0, s, pred, target, T, lens, means);
      SEL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_bss_corr<false>, dim3(unsigned(chunks), unsigned(B)), dim3(threads), 0, s, pred, target, T,
                       lens, L, cm, part);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bss_solve<false>, dim3(unsigned(B)), dim3(threads), 0, s, part, chunks, L, load_diag, T,
                       lens, corr, dvals, vals);
  }
  SEL_LAUNCH_CHECK();
  if (mean) {
    hipLaunchKernelGGL(k_bss_mean, dim3(1), dim3(256), 0, s, dvals, B, mean);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

}  // namespace

int sel_bss_sdr(const float* pred, const float* target, int64_t B, int64_t T, int filter_length, int zero_mean,
                double load_diag, float* vals, float* mean, double* corr, void* ws, size_t ws_bytes,
                sel_stream_t stream) {
  return bss_sdr("sel_bss_sdr", pred, target, B, T, nullptr, filter_length, zero_mean, load_diag, vals, mean, corr, ws,
                 ws_bytes, stream);
}

int sel_bss_sdr_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int filter_length, int zero_mean, double load_diag, float* vals, float* mean, double* corr,
                    void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(lengths, SEL_ERR_ARG, "sel_bss_sdr_var: null lengths");
  return bss_sdr("sel_bss_sdr_var", pred, target, B, T, lengths, filter_length, zero_mean, load_diag, vals, mean, corr,
                 ws, ws_bytes, stream);
}

}  // extern "C"
