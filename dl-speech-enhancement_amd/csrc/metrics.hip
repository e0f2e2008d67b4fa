// Evaluation measures: the SDR family (SNR / SI-SDR, optionally
// zero-mean; torchmetrics 1.2.0 formulas) with the gradient with respect to the
// prediction, and STOI / ESTOI at 10 kHz.  Every entry point validates first,
// allocates nothing, never synchronises with the host and can be captured into
// a graph: frame counts (kept, M, J) are device data the host never reads.
#include <cmath>

#include "sel_common.h"

namespace sel {
namespace metrics {

constexpr double kEps32 = 1.1920928955078125e-07;  // torch.finfo(float32).eps
constexpr double kEps = 2.220446049250313e-16;     // numpy.finfo(float64).eps (pystoi's EPS)

// ---------------------------------------------------------------------------
// SDR family.  Workspace: (num, den) pairs (2B doubles, the layout of
// sel_snr_fwd's sums), then (mean p, mean t, S_pt, S_pp) per row (4B doubles).
// ---------------------------------------------------------------------------

// Ragged batches: row b is its first lengths[b] samples, T stays the
// row stride.  A length above T counts as T, a negative one as 0.
__device__ __forceinline__ int64_t row_len(const int64_t* __restrict__ lens, int64_t b, int64_t T) {
  const int64_t n = lens[b];
  return n > T ? T : (n < 0 ? 0 : n);
}

// One block per row, fp64 sums; with zero_mean a first pass takes the means and
// the second sums the centred values (moments of the raw values would lose the
// residual under a DC offset).
template <bool VAR>
__global__ __launch_bounds__(256) void k_sdr_sums(const float* __restrict__ p, const float* __restrict__ t,
                                                  int64_t stride, const int64_t* __restrict__ lens, int zero_mean,
                                                  double* __restrict__ pairs, double* __restrict__ ext) {
  __shared__ double red[16];
  __shared__ double bc[2];
  const int64_t b = blockIdx.x;
  const float* __restrict__ pr = p + b * stride;
  const float* __restrict__ tr = t + b * stride;
  int64_t T = stride;  // the row's own length
  if constexpr (VAR) T = row_len(lens, b, stride);
  double mp = 0.0, mt = 0.0;
  if (zero_mean) {
    double sp = 0.0, st = 0.0;
    for (int64_t i = threadIdx.x; i < T; i += blockDim.x) {
      sp += double(pr[i]);
      st += double(tr[i]);
    }
    sp = block_sum<double>(sp, red);
    st = block_sum<double>(st, red);
    if (threadIdx.x == 0) {
      bc[0] = sp / double(T);
      bc[1] = st / double(T);
    }
    __syncthreads();
    mp = bc[0];
    mt = bc[1];
  }
  double stt = 0.0, sdd = 0.0, spt = 0.0, spp = 0.0;
  for (int64_t i = threadIdx.x; i < T; i += blockDim.x) {
    const double pc = double(pr[i]) - mp, tc = double(tr[i]) - mt, d = tc - pc;
    stt += tc * tc;
    sdd += d * d;
    spt += pc * tc;
    spp += pc * pc;
  }
  stt = block_sum<double>(stt, red);
  sdd = block_sum<double>(sdd, red);
  spt = block_sum<double>(spt, red);
  spp = block_sum<double>(spp, red);
  if (threadIdx.x == 0) {
    pairs[2 * b] = stt;
    pairs[2 * b + 1] = sdd;
    ext[4 * b] = mp;
    ext[4 * b + 1] = mt;
    ext[4 * b + 2] = spt;
    ext[4 * b + 3] = spp;
  }
}

// numerator and denominator of the ratio under the logarithm (eps included)
__device__ __forceinline__ void sdr_ratio(double stt, double sdd, double spt, double spp, int si, double& alpha,
                                          double& num, double& den) {
  if (!si) {
    alpha = 1.0;
    num = stt + kEps32;
    den = sdd + kEps32;
    return;
  }
  alpha = (spt + kEps32) / (stt + kEps32);
  const double e = alpha * alpha * stt;
  const double r = e - 2.0 * alpha * spt + spp;  // sum (alpha t - p)^2
  num = e + kEps32;
  den = (r > 0.0 ? r : 0.0) + kEps32;
}

template <bool VAR>
__global__ __launch_bounds__(256) void k_sdr_finish(const double* __restrict__ pairs, const double* __restrict__ ext,
                                                    int64_t B, int64_t T, const int64_t* __restrict__ lens, int si,
                                                    float* __restrict__ vals, float* __restrict__ mean) {
  __shared__ double red[16];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    double alpha, num, den;
    sdr_ratio(pairs[2 * b], pairs[2 * b + 1], ext[4 * b + 2], ext[4 * b + 3], si, alpha, num, den);
    double v = 10.0 * log10(num / den);
    if constexpr (VAR) {
      if (row_len(lens, b, T) < 1) v = NAN;  // an empty row has no value
    }
    vals[b] = float(v);
    acc += v;
  }
  acc = block_sum<double>(acc, red);
  if (threadIdx.x == 0) mean[0] = float(acc / double(B));
}

// per-row values of the plain SNR from sel_snr_fwd's sums, in its arithmetic
__global__ __launch_bounds__(256) void k_snr_rows(const double* __restrict__ sums, int64_t B,
                                                  float* __restrict__ vals) {
  const float eps = 1.1920928955078125e-07f;
  const int64_t b = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b < B) vals[b] = 10.f * log10f((float(sums[2 * b]) + eps) / (float(sums[2 * b + 1]) + eps));
}

// The plain SNR (scale_invariant = zero_mean = 0) of a ragged batch, in the
// arithmetic of sel_snr_fwd (k_snr_sums / k_snr_finish) and k_snr_rows.
__global__ __launch_bounds__(256) void k_snr_sums_var(const float* __restrict__ p, const float* __restrict__ t,
                                                      int64_t T, const int64_t* __restrict__ lens,
                                                      double* __restrict__ sums) {
  __shared__ double red[16];
  const int64_t b = blockIdx.x;
  const int64_t n = row_len(lens, b, T);
  double st = 0.0, sd = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const float tv = t[b * T + i], d = tv - p[b * T + i];
    st += double(tv) * tv;
    sd += double(d) * d;
  }
  st = block_sum<double>(st, red);
  sd = block_sum<double>(sd, red);
  if (threadIdx.x == 0) {
    sums[2 * b] = st;
    sums[2 * b + 1] = sd;
  }
}

__global__ __launch_bounds__(256) void k_snr_finish_var(const double* __restrict__ sums, int64_t B, int64_t T,
                                                        const int64_t* __restrict__ lens, float* __restrict__ vals,
                                                        float* __restrict__ mean) {
  __shared__ float red[16];
  const float eps = 1.1920928955078125e-07f;
  float v = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    float r = 10.f * log10f((float(sums[2 * b]) + eps) / (float(sums[2 * b + 1]) + eps));
    if (row_len(lens, b, T) < 1) r = NAN;
    vals[b] = r;
    v += r;
  }
  v = block_sum<float>(v, red);
  if (threadIdx.x == 0) mean[0] = v / float(B);
}

constexpr int kBwdChunk = 4096;  // elements of a row per block of the gradient kernel

// g_pred = g_row * (ct * (t - mean t) + cp * (p - mean p)); the two coefficients
// follow from d/dp of 10 log10(num / den)
template <bool VAR>
__global__ __launch_bounds__(256) void k_sdr_bwd(const float* __restrict__ p, const float* __restrict__ t, int64_t B,
                                                 int64_t T, const int64_t* __restrict__ lens, int cpr, int si,
                                                 int zero_mean, const double* __restrict__ pairs,
                                                 const double* __restrict__ ext, const float* __restrict__ g_vals,
                                                 const float* __restrict__ g_mean, float* __restrict__ gp) {
  const int64_t b = blockIdx.x / cpr;
  const int c = int(blockIdx.x % cpr);
  const double stt = pairs[2 * b], sdd = pairs[2 * b + 1];
  const double mp = zero_mean ? ext[4 * b] : 0.0, mt = zero_mean ? ext[4 * b + 1] : 0.0;
  const double spt = ext[4 * b + 2], spp = ext[4 * b + 3];
  double g = 0.0;
  if (g_vals) g += double(g_vals[b]);
  if (g_mean) g += double(g_mean[0]) / double(B);
  const double K = 10.0 / 2.302585092994046;
  double ct, cp;
  if (!si) {
    ct = 2.0 * K / (sdd + kEps32);
    cp = -ct;
  } else {
    double alpha, num, den;
    sdr_ratio(stt, sdd, spt, spp, 1, alpha, num, den);
    const double q = stt + kEps32;
    ct = K * (2.0 * alpha * stt / (q * num) - 2.0 * (alpha * stt - spt) / (q * den) + 2.0 * alpha / den);
    cp = -2.0 * K / den;
  }
  ct *= g;
  cp *= g;
  const int64_t i1 = int64_t(c + 1) * kBwdChunk < T ? int64_t(c + 1) * kBwdChunk : T;
  if constexpr (VAR) {  // exact zeros at and past the row's length; nothing there is read
    const int64_t n = row_len(lens, b, T);
    for (int64_t i = int64_t(c) * kBwdChunk + threadIdx.x; i < i1; i += blockDim.x)
      gp[b * T + i] = i < n ? float(ct * (double(t[b * T + i]) - mt) + cp * (double(p[b * T + i]) - mp)) : 0.f;
    return;
  }
  for (int64_t i = int64_t(c) * kBwdChunk + threadIdx.x; i < i1; i += blockDim.x)
    gp[b * T + i] = float(ct * (double(t[b * T + i]) - mt) + cp * (double(p[b * T + i]) - mp));
}

// the plain SNR's gradient from the batch mean alone, in the arithmetic of sel_snr_bwd (k_snr_bwd)
__global__ __launch_bounds__(256) void k_snr_bwd_var(const float* __restrict__ p, const float* __restrict__ t,
                                                     int64_t B, int64_t T, const int64_t* __restrict__ lens, int cpr,
                                                     const double* __restrict__ sums, const float* __restrict__ g,
                                                     float* __restrict__ gp) {
  const float eps = 1.1920928955078125e-07f;
  const float gv = g[0] * (20.f / 2.302585092994046f) / float(B);
  const int64_t b = blockIdx.x / cpr;
  const int c = int(blockIdx.x % cpr);
  const int64_t n = row_len(lens, b, T);
  const float den = float(sums[2 * b + 1]) + eps;
  const int64_t i1 = int64_t(c + 1) * kBwdChunk < T ? int64_t(c + 1) * kBwdChunk : T;
  for (int64_t i = int64_t(c) * kBwdChunk + threadIdx.x; i < i1; i += blockDim.x)
    gp[b * T + i] = i < n ? gv * (t[b * T + i] - p[b * T + i]) / den : 0.f;
}

// ---------------------------------------------------------------------------
// STOI / ESTOI (10 kHz; frame 256, hop 128, FFT 512, 15 third-octave bands,
// segments of 30 frames).
// ---------------------------------------------------------------------------
constexpr int kFrame = 256, kHop = 128, kNfft = 512, kBands = 15, kSeg = 30;
constexpr float kDynRange = 40.f;

// band b sums bins [edge(b), edge(b + 1)): the bins nearest 150 * 2^((2b -+ 1) / 6) Hz on the 10000 / 512 grid
__host__ __device__ inline int band_edge(int i) {
  constexpr int e[kBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
  return e[i];
}

// hanning(258)[1:-1]
__device__ __forceinline__ double stoi_window(int n) {
  return 0.5 - 0.5 * cospi(2.0 * double(n + 1) / double(kFrame + 1));
}

inline int64_t stoi_frames(int64_t T) { return (T - kFrame) / kHop + 1; }

// e_i = 20 log10(||w x[128 i : 128 i + 256]|| + EPS) of the clean signal: one wave per frame
// frames of a ragged row: 0 below one frame
__device__ __forceinline__ int stoi_row_frames(const int64_t* __restrict__ lens, int64_t b, int64_t T) {
  const int64_t n = row_len(lens, b, T);
  return n >= kFrame ? int((n - kFrame) / kHop + 1) : 0;
}

template <bool VAR>
__global__ __launch_bounds__(256) void k_stoi_energy(const float* __restrict__ clean, int64_t T, int F,
                                                     const int64_t* __restrict__ lens, float* __restrict__ e) {
  __shared__ float w[kFrame];
  w[threadIdx.x] = float(stoi_window(threadIdx.x));
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t b = blockIdx.y;
  if (i >= F) return;
  if constexpr (VAR) {
    if (i >= stoi_row_frames(lens, b, T)) return;
  }
  const float* __restrict__ x = clean + b * T + int64_t(i) * kHop;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = w[lane + 64 * r] * x[lane + 64 * r];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) e[b * F + i] = float(20.0 * log10(sqrt(double(s)) + kEps));
}

// One wave per row: the maximum, then the kept frames' indices compacted in
// order, 64 frames per round.  cnt = (frames, kept, M = kept - 1).
template <bool VAR>
__global__ __launch_bounds__(64) void k_stoi_mask(const float* __restrict__ e, int Fs, int64_t T,
                                                  const int64_t* __restrict__ lens, int* __restrict__ kidx,
                                                  int* __restrict__ cnt, int* __restrict__ info) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* __restrict__ er = e + b * Fs;
  int* __restrict__ kr = kidx + b * Fs;
  int F = Fs;  // the row's own frame count; Fs stays the stride
  if constexpr (VAR) F = stoi_row_frames(lens, b, T);
  float mx = -INFINITY;
  for (int i = lane; i < F; i += 64) mx = fmaxf(mx, er[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float thr = mx - kDynRange;
  int base = 0;
  for (int i0 = 0; i0 < F; i0 += 64) {
    const int i = i0 + lane;
    const bool keep = i < F && er[i] > thr;
    const unsigned long long m = __ballot(keep);
    if (keep) kr[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
    base += __popcll(m);
  }
  if (lane == 0) {
    const int M = base > 0 ? base - 1 : 0;
    cnt[3 * b] = F;
    cnt[3 * b + 1] = base;
    cnt[3 * b + 2] = M;
    if (info) {
      info[3 * b] = F;
      info[3 * b + 1] = base;
      info[3 * b + 2] = M;
    }
  }
}

// The transform runs in fp64: in fp32 its rounding error scales with the frame's
// strongest bin, which the per-band normalisations of weak bands then amplify
// (ESTOI deviated by up to 2e-4 from the fp64 definition).
struct cf {
  double x, y;
};
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf mul_mi(cf a) { return {a.y, -a.x}; }  // a * (-i)

// 4-point forward DFT, natural order
__device__ __forceinline__ void dft4(cf b0, cf b1, cf b2, cf b3, cf& y0, cf& y1, cf& y2, cf& y3) {
  const cf c0 = cadd(b0, b2), c2 = csub(b0, b2), c1 = cadd(b1, b3), c3 = mul_mi(csub(b1, b3));
  y0 = cadd(c0, c1);
  y1 = cadd(c2, c3);
  y2 = csub(c0, c1);
  y3 = csub(c2, c3);
}

// 8-point forward DFT in place, natural order (one decimation-in-frequency split, then two 4-point DFTs)
__device__ __forceinline__ void dft8(cf (&v)[8]) {
  const double s = 0.70710678118654752440;
  const cf a0 = cadd(v[0], v[4]), a1 = cadd(v[1], v[5]), a2 = cadd(v[2], v[6]), a3 = cadd(v[3], v[7]);
  const cf a4 = csub(v[0], v[4]);
  const cf a5 = cmul(csub(v[1], v[5]), cf{s, -s});
  const cf a6 = mul_mi(csub(v[2], v[6]));
  const cf a7 = cmul(csub(v[3], v[7]), cf{-s, -s});
  dft4(a0, a1, a2, a3, v[0], v[2], v[4], v[6]);
  dft4(a4, a5, a6, a7, v[1], v[3], v[5], v[7]);
}

// One wave per re-framed column j < M, both signals in one complex 512-point
// FFT (clean in the real part, processed in the imaginary part; the two spectra
// are separated by symmetry).  The column's 256 samples are gathered from the
// three kept frames that overlap it, so the overlap-added signal is never
// stored.  Stockham radix-8, three passes, eight points per lane, fp64.
// bands: (B, 2, F - 1, 15) fp64.
__global__ __launch_bounds__(64) void k_stoi_bands(const float* __restrict__ clean, const float* __restrict__ proc,
                                                   int64_t T, int F, const int* __restrict__ kidx,
                                                   const int* __restrict__ cnt, double* __restrict__ bands) {
  __shared__ double w[kFrame];
  __shared__ cf tw[kNfft];
  __shared__ cf buf[kNfft];
  __shared__ double pw[2][kFrame];
  const int lane = threadIdx.x;
  const int j = blockIdx.x;
  const int64_t b = blockIdx.y;
  if (j >= cnt[3 * b + 2]) return;  // block-uniform
#pragma unroll
  for (int r = 0; r < 4; ++r) w[lane + 64 * r] = stoi_window(lane + 64 * r);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    double sn, cs;
    sincospi(-2.0 * double(lane + 64 * r) / double(kNfft), &sn, &cs);
    tw[lane + 64 * r] = cf{cs, sn};
  }
  __syncthreads();
  const int* __restrict__ kr = kidx + b * F;
  const int k0 = kr[j], kp = kr[j + 1], km = j > 0 ? kr[j - 1] : -1;
  const float* __restrict__ xc = clean + b * T;
  const float* __restrict__ xp = proc + b * T;
  cf v[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = lane + 64 * r;
    const int64_t i0 = int64_t(k0) * kHop + n;
    double ac = w[n] * double(xc[i0]), ap = w[n] * double(xp[i0]);
    if (r < 2) {  // first half: the second half of the kept frame before
      if (km >= 0) {
        const int64_t i1 = int64_t(km) * kHop + kHop + n;
        ac += w[n + kHop] * double(xc[i1]);
        ap += w[n + kHop] * double(xp[i1]);
      }
    } else {  // second half: the first half of the kept frame after
      const int64_t i1 = int64_t(kp) * kHop + n - kHop;
      ac += w[n - kHop] * double(xc[i1]);
      ap += w[n - kHop] * double(xp[i1]);
    }
    v[r] = cf{w[n] * ac, w[n] * ap};
  }
#pragma unroll
  for (int r = 4; r < 8; ++r) v[r] = cf{0.0, 0.0};
  // pass Ns = 1
  dft8(v);
#pragma unroll
  for (int q = 0; q < 8; ++q) buf[lane * 8 + q] = v[q];
  __syncthreads();
  // pass Ns = 8
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
  __syncthreads();
  {
    const int k = lane & 7;
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[k * r * 8]);
    dft8(v);
    const int base = (lane >> 3) * 64 + k;
#pragma unroll
    for (int q = 0; q < 8; ++q) buf[base + q * 8] = v[q];
  }
  __syncthreads();
  // pass Ns = 64
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
  __syncthreads();
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[lane * r]);
  dft8(v);
#pragma unroll
  for (int q = 0; q < 8; ++q) buf[lane + q * 64] = v[q];
  __syncthreads();
  // |X|^2, |Y|^2 of the bins the bands use, from Z = X + iY
  for (int k = band_edge(0) + lane; k < band_edge(kBands); k += 64) {
    const cf a = buf[k], c = buf[kNfft - k];
    const double xr = a.x + c.x, xi = a.y - c.y, yr = a.y + c.y, yi = a.x - c.x;
    pw[0][k] = 0.25 * (xr * xr + xi * xi);
    pw[1][k] = 0.25 * (yr * yr + yi * yi);
  }
  __syncthreads();
  const int sg = lane >> 5, bd = lane & 31;
  if (bd < kBands) {
    double s = 0.0;
    for (int k = band_edge(bd); k < band_edge(bd + 1); ++k) s += pw[sg][k];
    bands[((b * 2 + sg) * int64_t(F - 1) + j) * kBands + bd] = sqrt(s);
  }
}

// One block per segment s < J = M - 29 (columns [s, s + 30)): its intermediate
// correlation summed over bands (STOI) or columns (ESTOI), in fp64, to seg (B, F - 30).
__global__ __launch_bounds__(64) void k_stoi_seg(const double* __restrict__ bands, const int* __restrict__ cnt, int F,
                                                 int extended, double* __restrict__ seg) {
  __shared__ double X[kSeg * kBands], Y[kSeg * kBands];
  __shared__ double part[kSeg];
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int M = cnt[3 * b + 2];
  if (M < kSeg || s > M - kSeg) return;  // block-uniform
  const double* __restrict__ bx = bands + ((b * 2) * int64_t(F - 1) + s) * kBands;
  const double* __restrict__ by = bands + ((b * 2 + 1) * int64_t(F - 1) + s) * kBands;
  for (int i = lane; i < kSeg * kBands; i += 64) {  // [column][band], as stored
    X[i] = bx[i];
    Y[i] = by[i];
  }
  __syncthreads();
  if (!extended) {
    if (lane < kBands) {
      double nx = 0.0, ny = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane], y = Y[c * kBands + lane];
        nx += x * x;
        ny += y * y;
      }
      const double scale = sqrt(nx) / (sqrt(ny) + kEps);
      const double beta = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20)
      double sx = 0.0, sy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane];
        const double y = fmin(scale * Y[c * kBands + lane], x * beta);
        Y[c * kBands + lane] = y;
        sx += x;
        sy += y;
      }
      const double mx = sx / kSeg, my = sy / kSeg;
      double sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double dx = X[c * kBands + lane] - mx, dy = Y[c * kBands + lane] - my;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
      }
      part[lane] = sxy / ((sqrt(sxx) + kEps) * (sqrt(syy) + kEps));
    }
  } else {
    if (lane < kBands) {  // rows: each band over the 30 columns
      for (int sgn = 0; sgn < 2; ++sgn) {
        double* A = sgn ? Y : X;
        double m = 0.0;
        for (int c = 0; c < kSeg; ++c) m += A[c * kBands + lane];
        m /= kSeg;
        double n2 = 0.0;
        for (int c = 0; c < kSeg; ++c) {
          const double dv = A[c * kBands + lane] - m;
          n2 += dv * dv;
        }
        const double inv = 1.0 / (sqrt(n2) + kEps);
        for (int c = 0; c < kSeg; ++c) A[c * kBands + lane] = (A[c * kBands + lane] - m) * inv;
      }
    }
    __syncthreads();
    if (lane < kSeg) {  // columns: each column over the 15 bands
      double mx = 0.0, my = 0.0;
      for (int k = 0; k < kBands; ++k) {
        mx += X[lane * kBands + k];
        my += Y[lane * kBands + k];
      }
      mx /= kBands;
      my /= kBands;
      double sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int k = 0; k < kBands; ++k) {
        const double dx = X[lane * kBands + k] - mx, dy = Y[lane * kBands + k] - my;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
      }
      part[lane] = sxy / ((sqrt(sxx) + kEps) * (sqrt(syy) + kEps));
    }
  }
  __syncthreads();
  if (lane == 0) {
    const int n = extended ? kSeg : kBands;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += part[i];
    seg[b * int64_t(F - kSeg) + s] = acc;
  }
}

// d_b = sum_s seg / (15 J) (STOI) or / (30 J) (ESTOI), summed in segment order; 1e-5 when M < 30
template <bool VAR>
__global__ __launch_bounds__(256) void k_stoi_finish(const double* __restrict__ seg, const int* __restrict__ cnt,
                                                     int64_t B, int F, int extended, float* __restrict__ d,
                                                     float* __restrict__ mean) {
  __shared__ double red[16];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    const int M = cnt[3 * b + 2];
    double v = 1e-5;
    if (M >= kSeg) {
      const int J = M - kSeg + 1;
      double s = 0.0;
      for (int i = 0; i < J; ++i) s += seg[b * int64_t(F - kSeg) + i];
      v = s / (double(extended ? kSeg : kBands) * double(J));
    }
    if constexpr (VAR) {
      if (cnt[3 * b] == 0) v = NAN;  // a row below one frame
    }
    d[b] = float(v);
    acc += v;
  }
  acc = block_sum<double>(acc, red);
  if (threadIdx.x == 0 && mean) mean[0] = float(acc / double(B));
}

// ---------------------------------------------------------------------------
// Ragged MAE / MSE / Mel-L1: one block per row, fp64 sums in a
// fixed order (a strided sum per thread over the counted elements in
// (sub-row, element) order, then the block tree).  An empty row is NaN.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_l1_l2(const float* __restrict__ a, const float* __restrict__ b,
                                                    int64_t inner, int64_t stride, const int64_t* __restrict__ lens,
                                                    float* __restrict__ l1, float* __restrict__ l2) {
  __shared__ double red[16];
  const int64_t row = blockIdx.x;
  const int64_t n = row_len(lens, row, stride);
  const float* __restrict__ ar = a + row * inner * stride;
  const float* __restrict__ br = b + row * inner * stride;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t r = 0; r < inner; ++r)
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const double d = double(ar[r * stride + i]) - double(br[r * stride + i]);
      s1 += fabs(d);
      s2 += d * d;
    }
  s1 = block_sum<double>(s1, red);
  s2 = block_sum<double>(s2, red);
  if (threadIdx.x == 0) {
    const double cntd = double(inner) * double(n);
    l1[row] = n > 0 ? float(s1 / cntd) : NAN;
    l2[row] = n > 0 ? float(s2 / cntd) : NAN;
  }
}

// means[0], means[1] = the batch means of the per-row values, fp64 in a fixed order
__global__ __launch_bounds__(256) void k_rows_means2(const float* __restrict__ l1, const float* __restrict__ l2,
                                                     int64_t B, float* __restrict__ means) {
  __shared__ double red[16];
  double a1 = 0.0, a2 = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    a1 += double(l1[b]);
    a2 += double(l2[b]);
  }
  a1 = block_sum<double>(a1, red);
  a2 = block_sum<double>(a2, red);
  if (threadIdx.x == 0) {
    means[0] = float(a1 / double(B));
    means[1] = float(a2 / double(B));
  }
}

// ---------------------------------------------------------------------------
// Gradient of STOI / ESTOI with respect to the processed signal.
// Three gathers, each summed in a fixed order (no atomics): the segments'
// adjoints, the columns' (two transforms each), the samples'.
// ---------------------------------------------------------------------------

// g_row / (n J): the factor of one segment's sum in the incoming gradient
__device__ __forceinline__ double stoi_seg_weight(const float* __restrict__ g_d, const float* __restrict__ g_mean,
                                                  int64_t b, int64_t B, int M, int extended) {
  double g = 0.0;
  if (g_d) g += double(g_d[b]);
  if (g_mean) g += double(g_mean[0]) / double(B);
  return g / (double(extended ? kSeg : kBands) * double(M - kSeg + 1));
}

// One block per segment s < J: the gradient of the segment's sum with respect
// to its 30 x 15 processed band magnitudes, times g_row / (n J), to
// gseg (B, F - 30, 30, 15) fp64.  The forward of k_stoi_seg is recomputed.
__global__ __launch_bounds__(64) void k_stoi_seg_bwd(const double* __restrict__ bands, const int* __restrict__ cnt,
                                                     int64_t B, int F, int extended, const float* __restrict__ g_d,
                                                     const float* __restrict__ g_mean, double* __restrict__ gseg) {
  __shared__ double X[kSeg * kBands], Y[kSeg * kBands];
  __shared__ double nrm[kBands];
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int M = cnt[3 * b + 2];
  if (M < kSeg || s > M - kSeg) return;  // block-uniform
  const double* __restrict__ bx = bands + ((b * 2) * int64_t(F - 1) + s) * kBands;
  const double* __restrict__ by = bands + ((b * 2 + 1) * int64_t(F - 1) + s) * kBands;
  double* __restrict__ go = gseg + (b * int64_t(F - kSeg) + s) * (kSeg * kBands);
  for (int i = lane; i < kSeg * kBands; i += 64) {  // [column][band], as stored
    X[i] = bx[i];
    Y[i] = by[i];
  }
  __syncthreads();
  const double wgt = stoi_seg_weight(g_d, g_mean, b, B, M, extended);
  if (!extended) {
    if (lane < kBands) {
      double nx = 0.0, ny = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane], y = Y[c * kBands + lane];
        nx += x * x;
        ny += y * y;
      }
      const double rx = sqrt(nx), ry = sqrt(ny);
      const double scale = rx / (ry + kEps);
      const double beta = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20)
      double sx = 0.0, sy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane];
        sx += x;
        sy += fmin(scale * Y[c * kBands + lane], x * beta);
      }
      const double mx = sx / kSeg, my = sy / kSeg;
      double sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane];
        const double dx = x - mx, dy = fmin(scale * Y[c * kBands + lane], x * beta) - my;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
      }
      // rho = sxy / (a q): d rho / d dy = ca dx - cb dy, then the mean removal's adjoint
      const double rs = sqrt(syy), a = sqrt(sxx) + kEps, q = rs + kEps;
      const double ca = 1.0 / (a * q), cb = rs > 0.0 ? sxy / (a * q * q * rs) : 0.0;
      double hm = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane];
        hm += ca * (x - mx) - cb * (fmin(scale * Y[c * kBands + lane], x * beta) - my);
      }
      hm /= kSeg;
      // y' = scale y where scale y < beta x (scale depends on every y of the band), a constant elsewhere
      double dot = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane], y = Y[c * kBands + lane];
        if (scale * y < x * beta) dot += (ca * (x - mx) - cb * (scale * y - my) - hm) * y;
      }
      const double dscale = ry > 0.0 ? -rx / ((ry + kEps) * (ry + kEps) * ry) : 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double x = X[c * kBands + lane], y = Y[c * kBands + lane];
        double g = dot * dscale * y;
        if (scale * y < x * beta) g += scale * (ca * (x - mx) - cb * (scale * y - my) - hm);
        go[c * kBands + lane] = wgt * g;
      }
    }
    return;
  }
  if (lane < kBands) {  // rows: each band over the 30 columns; Y keeps the row-normalised values
    for (int sgn = 0; sgn < 2; ++sgn) {
      double* A = sgn ? Y : X;
      double m = 0.0;
      for (int c = 0; c < kSeg; ++c) m += A[c * kBands + lane];
      m /= kSeg;
      double n2 = 0.0;
      for (int c = 0; c < kSeg; ++c) {
        const double dv = A[c * kBands + lane] - m;
        n2 += dv * dv;
      }
      const double r = sqrt(n2);
      if (sgn) nrm[lane] = r;
      const double inv = 1.0 / (r + kEps);
      for (int c = 0; c < kSeg; ++c) A[c * kBands + lane] = (A[c * kBands + lane] - m) * inv;
    }
  }
  __syncthreads();
  if (lane < kSeg) {  // columns: d rho_c / d (row-normalised y), over X's column (no longer needed)
    double mx = 0.0, my = 0.0;
    for (int k = 0; k < kBands; ++k) {
      mx += X[lane * kBands + k];
      my += Y[lane * kBands + k];
    }
    mx /= kBands;
    my /= kBands;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = 0; k < kBands; ++k) {
      const double dx = X[lane * kBands + k] - mx, dy = Y[lane * kBands + k] - my;
      sxx += dx * dx;
      syy += dy * dy;
      sxy += dx * dy;
    }
    const double rs = sqrt(syy), a = sqrt(sxx) + kEps, q = rs + kEps;
    const double ca = 1.0 / (a * q), cb = rs > 0.0 ? sxy / (a * q * q * rs) : 0.0;
    double hm = 0.0;
    for (int k = 0; k < kBands; ++k) {
      const double h = ca * (X[lane * kBands + k] - mx) - cb * (Y[lane * kBands + k] - my);
      X[lane * kBands + k] = h;
      hm += h;
    }
    hm /= kBands;
    for (int k = 0; k < kBands; ++k) X[lane * kBands + k] -= hm;
  }
  __syncthreads();
  if (lane < kBands) {  // rows: through r = v / (||v|| + EPS), v = y - mean y
    const double r = nrm[lane], q = r + kEps;
    double dot = 0.0;
    for (int c = 0; c < kSeg; ++c) dot += X[c * kBands + lane] * Y[c * kBands + lane];
    const double cr = r > 0.0 ? dot / r : 0.0;
    double gm = 0.0;
    for (int c = 0; c < kSeg; ++c) gm += X[c * kBands + lane] / q - cr * Y[c * kBands + lane];
    gm /= kSeg;
    for (int c = 0; c < kSeg; ++c)
      go[c * kBands + lane] = wgt * (X[c * kBands + lane] / q - cr * Y[c * kBands + lane] - gm);
  }
}

// 512-point forward transform of v (lane holds points lane + 64 r) into buf in
// natural order: the three Stockham radix-8 passes of k_stoi_bands, which keeps
// its own copy so that its code, and with it the forward's bits, stay as they were.
__device__ __forceinline__ void fft512(cf (&v)[8], cf* __restrict__ buf, const cf* __restrict__ tw, int lane) {
  dft8(v);
#pragma unroll
  for (int q = 0; q < 8; ++q) buf[lane * 8 + q] = v[q];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
  __syncthreads();
  {
    const int k = lane & 7;
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[k * r * 8]);
    dft8(v);
    const int base = (lane >> 3) * 64 + k;
#pragma unroll
    for (int q = 0; q < 8; ++q) buf[base + q * 8] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
  __syncthreads();
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[lane * r]);
  dft8(v);
#pragma unroll
  for (int q = 0; q < 8; ++q) buf[lane + q * 64] = v[q];
  __syncthreads();
}

// One wave per re-framed column j < M of a row with M >= 30.  g_band[j] is the
// sum over the at most 30 segments holding column j, in ascending s.  The
// column's spectrum Y is recomputed as k_stoi_bands does (processed signal
// only); with G_k = (g_band / band) Y_k on bins 7..218 (0 where band is 0) the
// gradient with respect to the column of the overlap-added signal is
// gz[n] = w[n] Re sum_k G_k e^{+2 pi i k n / 512}, n < 256: w[n] times the real
// part of the forward transform of conj(G).  gz: (B, F - 1, 256) fp64.
__global__ __launch_bounds__(64) void k_stoi_col_bwd(const float* __restrict__ proc, int64_t T, int F,
                                                     const int* __restrict__ kidx, const int* __restrict__ cnt,
                                                     const double* __restrict__ bands,
                                                     const double* __restrict__ gseg, double* __restrict__ gz) {
  __shared__ double w[kFrame];
  __shared__ cf tw[kNfft];
  __shared__ cf buf[kNfft];
  __shared__ double coef[kBands];
  const int lane = threadIdx.x;
  const int j = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int M = cnt[3 * b + 2];
  if (M < kSeg || j >= M) return;  // block-uniform
#pragma unroll
  for (int r = 0; r < 4; ++r) w[lane + 64 * r] = stoi_window(lane + 64 * r);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    double sn, cs;
    sincospi(-2.0 * double(lane + 64 * r) / double(kNfft), &sn, &cs);
    tw[lane + 64 * r] = cf{cs, sn};
  }
  if (lane < kBands) {
    const int J = M - kSeg + 1;
    const int s0 = j - (kSeg - 1) > 0 ? j - (kSeg - 1) : 0, s1 = j < J - 1 ? j : J - 1;
    const double* __restrict__ gs = gseg + b * int64_t(F - kSeg) * (kSeg * kBands);
    double g = 0.0;
    for (int s = s0; s <= s1; ++s) g += gs[(int64_t(s) * kSeg + (j - s)) * kBands + lane];
    const double bd = bands[((b * 2 + 1) * int64_t(F - 1) + j) * kBands + lane];
    coef[lane] = bd != 0.0 ? g / bd : 0.0;
  }
  __syncthreads();
  const int* __restrict__ kr = kidx + b * F;
  const int k0 = kr[j], kp = kr[j + 1], km = j > 0 ? kr[j - 1] : -1;
  const float* __restrict__ xp = proc + b * T;
  cf v[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = lane + 64 * r;
    double ap = w[n] * double(xp[int64_t(k0) * kHop + n]);
    if (r < 2) {
      if (km >= 0) ap += w[n + kHop] * double(xp[int64_t(km) * kHop + kHop + n]);
    } else {
      ap += w[n - kHop] * double(xp[int64_t(kp) * kHop + n - kHop]);
    }
    v[r] = cf{w[n] * ap, 0.0};
  }
#pragma unroll
  for (int r = 4; r < 8; ++r) v[r] = cf{0.0, 0.0};
  fft512(v, buf, tw, lane);
  // conj(G_k) on the bins of the bands, zero elsewhere (bins >= 256 hold none)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = lane + 64 * r;
    v[r] = cf{0.0, 0.0};
    if (k >= band_edge(0) && k < band_edge(kBands)) {
      int bd = 0;
      while (k >= band_edge(bd + 1)) ++bd;
      const double c = coef[bd];
      v[r] = cf{c * buf[k].x, -c * buf[k].y};
    }
  }
#pragma unroll
  for (int r = 4; r < 8; ++r) v[r] = cf{0.0, 0.0};
  __syncthreads();
  fft512(v, buf, tw, lane);
  double* __restrict__ out = gz + (b * int64_t(F - 1) + j) * kFrame;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[lane + 64 * r] = w[lane + 64 * r] * buf[lane + 64 * r].x;
}

// inv[i] = position of frame i in the row's kept list, or -1: a binary search per frame
__global__ __launch_bounds__(256) void k_stoi_inv(const int* __restrict__ kidx, const int* __restrict__ cnt, int F,
                                                  int* __restrict__ inv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (i >= F) return;
  const int* __restrict__ kr = kidx + b * F;
  int lo = 0, hi = cnt[3 * b + 1];  // first position with kr[pos] >= i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (kr[mid] < i) lo = mid + 1; else hi = mid;
  }
  inv[b * F + i] = lo < cnt[3 * b + 1] && kr[lo] == i ? lo : -1;
}

// One thread per sample t.  Frames t / 128 - 1 and t / 128 cover it; a kept
// frame at position q adds w[n] times its sample of column q and of column
// q + 1 (n >= 128) or q - 1 (n < 128): at most four terms, frames then columns
// ascending.  0 for a row with M < 30, for samples no kept frame covers and for
// the tail past the last frame.
__global__ __launch_bounds__(256) void k_stoi_gather(const double* __restrict__ gz, const int* __restrict__ inv,
                                                     const int* __restrict__ cnt, int64_t T, int F,
                                                     float* __restrict__ g_proc) {
  __shared__ double w[kFrame];
  w[threadIdx.x] = stoi_window(threadIdx.x);
  __syncthreads();
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t b = blockIdx.y;
  if (t >= T) return;
  const int M = cnt[3 * b + 2];
  double acc = 0.0;
  if (M >= kSeg) {
    const double* __restrict__ gr = gz + b * int64_t(F - 1) * kFrame;
    const int i1 = int(t / kHop);
    for (int i = i1 - 1; i <= i1; ++i) {
      if (i < 0 || i >= F) continue;
      const int q = inv[b * F + i];
      if (q < 0) continue;
      const int n = int(t - int64_t(i) * kHop);  // i1 - 1: [128, 256); i1: [0, 128)
      const int ja = n < kHop ? q - 1 : q, jb = ja + 1;
      const int na = n < kHop ? n + kHop : n, nb = n < kHop ? n : n - kHop;
      double c = 0.0;
      if (ja >= 0 && ja < M) c += gr[int64_t(ja) * kFrame + na];
      if (jb < M) c += gr[int64_t(jb) * kFrame + nb];
      acc += w[n] * c;
    }
  }
  g_proc[b * T + t] = float(acc);
}

}  // namespace metrics
}  // namespace sel

using namespace sel;
using namespace sel::metrics;

extern "C" {

size_t sel_sdr_workspace(int64_t B) { return B > 0 ? size_t(B) * 6 * sizeof(double) : 0; }

namespace {

// sel_sdr_fwd and sel_sdr_fwd_var: lens == nullptr is the fixed-length call
int sdr_fwd(const char* fn, const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lens,
            int scale_invariant, int zero_mean, float* vals, float* mean, void* ws, size_t ws_bytes,
            sel_stream_t stream) {
  SEL_REQUIRE(pred && target && vals && mean && ws, SEL_ERR_ARG, "%s: null pointer", fn);
  SEL_REQUIRE(B > 0 && T > 0 && B <= (int64_t(1) << 30), SEL_ERR_ARG, "%s: bad shape", fn);
  SEL_REQUIRE((scale_invariant | zero_mean | 1) == 1, SEL_ERR_ARG, "%s: flags must be 0 or 1", fn);
  SEL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, SEL_ERR_ARG, "%s: workspace not 8-byte aligned", fn);
  SEL_REQUIRE(ws_bytes >= sel_sdr_workspace(B), SEL_ERR_WORKSPACE, "%s: workspace too small", fn);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* pairs = static_cast<double*>(ws);
  double* ext = pairs + 2 * B;
  if (!scale_invariant && !zero_mean) {
    if (lens) {
      hipLaunchKernelGGL(k_snr_sums_var, dim3(unsigned(B)), dim3(256), 0, s, pred, target, T, lens, pairs);
      SEL_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_snr_finish_var, dim3(1), dim3(256), 0, s, pairs, B, T, lens, vals, mean);
      SEL_LAUNCH_CHECK();
      return SEL_OK;
    }
    // the plain SNR is sel_snr_fwd itself (same sums, same mean), plus its per-row values
    const int rc = sel_snr_fwd(pred, target, B, T, pairs, mean, stream);
    if (rc != SEL_OK) return rc;
    hipLaunchKernelGGL(k_snr_rows, dim3(unsigned((B + 255) / 256)), dim3(256), 0, s, pairs, B, vals);
    SEL_LAUNCH_CHECK();
    return SEL_OK;
  }
  if (lens) {
    hipLaunchKernelGGL(k_sdr_sums<true>, dim3(unsigned(B)), dim3(256), 0, s, pred, target, T, lens, zero_mean, pairs,
                       ext);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sdr_finish<true>, dim3(1), dim3(256), 0, s, pairs, ext, B, T, lens, scale_invariant, vals,
                       mean);
  } else {
    hipLaunchKernelGGL(k_sdr_sums<false>, dim3(unsigned(B)), dim3(256), 0, s, pred, target, T, lens, zero_mean, pairs,
                       ext);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sdr_finish<false>, dim3(1), dim3(256), 0, s, pairs, ext, B, T, lens, scale_invariant, vals,
                       mean);
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sdr_bwd(const char* fn, const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lens,
            int scale_invariant, int zero_mean, const float* g_vals, const float* g_mean, float* g_pred,
            const void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(pred && target && g_pred && ws, SEL_ERR_ARG, "%s: null pointer", fn);
  SEL_REQUIRE(g_vals || g_mean, SEL_ERR_ARG, "%s: no incoming gradient", fn);
  SEL_REQUIRE(B > 0 && T > 0 && B <= (int64_t(1) << 30), SEL_ERR_ARG, "%s: bad shape", fn);
  const int64_t cpr = (T + kBwdChunk - 1) / kBwdChunk;
  SEL_REQUIRE(cpr <= (int64_t(1) << 30) / B, SEL_ERR_ARG, "%s: batch too large", fn);
  SEL_REQUIRE((scale_invariant | zero_mean | 1) == 1, SEL_ERR_ARG, "%s: flags must be 0 or 1", fn);
  SEL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, SEL_ERR_ARG, "%s: workspace not 8-byte aligned", fn);
  SEL_REQUIRE(ws_bytes >= sel_sdr_workspace(B), SEL_ERR_WORKSPACE, "%s: workspace too small", fn);
  const double* pairs = static_cast<const double*>(ws);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!scale_invariant && !zero_mean && !g_vals) {
    if (!lens) return sel_snr_bwd(pred, target, B, T, pairs, g_mean, g_pred, stream);
    hipLaunchKernelGGL(k_snr_bwd_var, dim3(unsigned(B * cpr)), dim3(256), 0, s, pred, target, B, T, lens, int(cpr),
                       pairs, g_mean, g_pred);
    SEL_LAUNCH_CHECK();
    return SEL_OK;
  }
  if (lens)
    hipLaunchKernelGGL(k_sdr_bwd<true>, dim3(unsigned(B * cpr)), dim3(256), 0, s, pred, target, B, T, lens, int(cpr),
                       scale_invariant, zero_mean, pairs, pairs + 2 * B, g_vals, g_mean, g_pred);
  else
    hipLaunchKernelGGL(k_sdr_bwd<false>, dim3(unsigned(B * cpr)), dim3(256), 0, s, pred, target, B, T, lens, int(cpr),
                       scale_invariant, zero_mean, pairs, pairs + 2 * B, g_vals, g_mean, g_pred);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // namespace

int sel_sdr_fwd(const float* pred, const float* target, int64_t B, int64_t T, int scale_invariant, int zero_mean,
                float* vals, float* mean, void* ws, size_t ws_bytes, sel_stream_t stream) {
  return sdr_fwd("sel_sdr_fwd", pred, target, B, T, nullptr, scale_invariant, zero_mean, vals, mean, ws, ws_bytes,
                 stream);
}

int sel_sdr_fwd_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int scale_invariant, int zero_mean, float* vals, float* mean, void* ws, size_t ws_bytes,
                    sel_stream_t stream) {
  SEL_REQUIRE(lengths, SEL_ERR_ARG, "sel_sdr_fwd_var: null lengths");
  return sdr_fwd("sel_sdr_fwd_var", pred, target, B, T, lengths, scale_invariant, zero_mean, vals, mean, ws, ws_bytes,
                 stream);
}

int sel_sdr_bwd(const float* pred, const float* target, int64_t B, int64_t T, int scale_invariant, int zero_mean,
                const float* g_vals, const float* g_mean, float* g_pred, const void* ws, size_t ws_bytes,
                sel_stream_t stream) {
  return sdr_bwd("sel_sdr_bwd", pred, target, B, T, nullptr, scale_invariant, zero_mean, g_vals, g_mean, g_pred, ws,
                 ws_bytes, stream);
}

int sel_sdr_bwd_var(const float* pred, const float* target, int64_t B, int64_t T, const int64_t* lengths,
                    int scale_invariant, int zero_mean, const float* g_vals, const float* g_mean, float* g_pred,
                    const void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(lengths, SEL_ERR_ARG, "sel_sdr_bwd_var: null lengths");
  return sdr_bwd("sel_sdr_bwd_var", pred, target, B, T, lengths, scale_invariant, zero_mean, g_vals, g_mean, g_pred,
                 ws, ws_bytes, stream);
}

int sel_stoi_band_edges(int* edges) {
  SEL_REQUIRE(edges, SEL_ERR_ARG, "sel_stoi_band_edges: null pointer");
  for (int i = 0; i <= kBands; ++i) edges[i] = band_edge(i);
  return SEL_OK;
}

// fp64 first: segment sums (F - 30 per row) and band magnitudes (2 x (F - 1) x 15);
// then frame energies, kept-frame lists (F each) and counts (3), 4 bytes each
size_t sel_stoi_workspace(int64_t B, int64_t T) {
  if (B <= 0 || T < kFrame) return 0;
  const size_t F = size_t(stoi_frames(T));
  const size_t J = F > size_t(kSeg) ? F - kSeg : 0;
  return size_t(B) * ((J + 2 * (F - 1) * kBands) * sizeof(double) + (2 * F + 3) * sizeof(float));
}

namespace {

// sel_stoi and sel_stoi_var: lens == nullptr is the fixed-length call.  With
// lengths the strides (frames F, bands F - 1, segments F - 30) and the J > 0
// launch skip still come from T; each row's own frame count is device data.
int stoi_fwd(const char* fn, const float* clean, const float* proc, int64_t B, int64_t T, const int64_t* lens,
             int extended, float* d, float* mean, int* info, void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(clean && proc && d && ws, SEL_ERR_ARG, "%s: null pointer", fn);
  SEL_REQUIRE(B > 0 && B <= 65535, SEL_ERR_ARG, "%s: B must be in [1, 65535]", fn);
  SEL_REQUIRE(T >= kFrame && T <= (int64_t(1) << 30), SEL_ERR_ARG, "%s: T must be in [256, 2^30]", fn);
  SEL_REQUIRE((extended | 1) == 1, SEL_ERR_ARG, "%s: extended must be 0 or 1", fn);
  SEL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, SEL_ERR_ARG, "%s: workspace not 8-byte aligned", fn);
  SEL_REQUIRE(ws_bytes >= sel_stoi_workspace(B, T), SEL_ERR_WORKSPACE, "%s: workspace too small", fn);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int F = int(stoi_frames(T));
  const int J = F > kSeg ? F - kSeg : 0;
  double* seg = static_cast<double*>(ws);
  double* bands = seg + size_t(B) * J;
  float* e = reinterpret_cast<float*>(bands + size_t(B) * 2 * (F - 1) * kBands);
  int* kidx = reinterpret_cast<int*>(e + size_t(B) * F);
  int* cnt = kidx + size_t(B) * F;
  const dim3 eg(unsigned((F + 3) / 4), unsigned(B));
  if (lens) {
    hipLaunchKernelGGL(k_stoi_energy<true>, eg, dim3(256), 0, s, clean, T, F, lens, e);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stoi_mask<true>, dim3(unsigned(B)), dim3(64), 0, s, e, F, T, lens, kidx, cnt, info);
  } else {
    hipLaunchKernelGGL(k_stoi_energy<false>, eg, dim3(256), 0, s, clean, T, F, lens, e);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stoi_mask<false>, dim3(unsigned(B)), dim3(64), 0, s, e, F, T, lens, kidx, cnt, info);
  }
  SEL_LAUNCH_CHECK();
  if (J > 0) {  // fewer than 31 frames cannot give M >= 30: every row is 1e-5
    hipLaunchKernelGGL(k_stoi_bands, dim3(unsigned(F - 1), unsigned(B)), dim3(64), 0, s, clean, proc, T, F, kidx, cnt,
                       bands);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stoi_seg, dim3(unsigned(J), unsigned(B)), dim3(64), 0, s, bands, cnt, F, extended, seg);
    SEL_LAUNCH_CHECK();
  }
  if (lens)
    hipLaunchKernelGGL(k_stoi_finish<true>, dim3(1), dim3(256), 0, s, seg, cnt, B, F, extended, d, mean);
  else
    hipLaunchKernelGGL(k_stoi_finish<false>, dim3(1), dim3(256), 0, s, seg, cnt, B, F, extended, d, mean);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // namespace

int sel_stoi(const float* clean, const float* proc, int64_t B, int64_t T, int extended, float* d, float* mean,
             int* info, void* ws, size_t ws_bytes, sel_stream_t stream) {
  return stoi_fwd("sel_stoi", clean, proc, B, T, nullptr, extended, d, mean, info, ws, ws_bytes, stream);
}

int sel_stoi_var(const float* clean, const float* proc, int64_t B, int64_t T, const int64_t* lengths, int extended,
                 float* d, float* mean, int* info, void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(lengths, SEL_ERR_ARG, "sel_stoi_var: null lengths");
  return stoi_fwd("sel_stoi_var", clean, proc, B, T, lengths, extended, d, mean, info, ws, ws_bytes, stream);
}

// Per-row mean |a - b| and mean (a - b)^2 of a ragged batch: row b is `inner`
// sub-rows of `stride` elements, of which the first n[b] count.
int sel_rows_l1_l2_var(const float* a, const float* b, int64_t B, int64_t inner, int64_t stride, const int64_t* n,
                       float* l1, float* l2, float* means, sel_stream_t stream) {
  SEL_REQUIRE(a && b && n && l1 && l2, SEL_ERR_ARG, "sel_rows_l1_l2_var: null pointer");
  SEL_REQUIRE(B > 0 && B <= (int64_t(1) << 30) && inner > 0 && stride > 0, SEL_ERR_ARG,
              "sel_rows_l1_l2_var: bad shape");
  SEL_REQUIRE(inner <= (int64_t(1) << 40) / stride && B <= (int64_t(1) << 60) / (inner * stride), SEL_ERR_ARG,
              "sel_rows_l1_l2_var: batch too large");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_rows_l1_l2, dim3(unsigned(B)), dim3(256), 0, s, a, b, inner, stride, n, l1, l2);
  SEL_LAUNCH_CHECK();
  if (means) {
    hipLaunchKernelGGL(k_rows_means2, dim3(1), dim3(256), 0, s, l1, l2, B, means);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

// fp64 first: the segments' adjoints ((F - 30) x 30 x 15 per row) and the columns'
// ((F - 1) x 256); then the inverse kept-frame index (F ints), rounded up to 8 bytes
size_t sel_stoi_bwd_workspace(int64_t B, int64_t T) {
  if (B <= 0 || T < kFrame) return 0;
  const size_t F = size_t(stoi_frames(T));
  const size_t J = F > size_t(kSeg) ? F - kSeg : 0;
  const size_t bytes = size_t(B) * ((J * kSeg * kBands + (F - 1) * kFrame) * sizeof(double) + F * sizeof(int));
  return (bytes + 7) / 8 * 8;
}

int sel_stoi_bwd(const float* clean, const float* proc, int64_t B, int64_t T, int extended, const float* g_d,
                 const float* g_mean, float* g_proc, const void* ws_fwd, size_t ws_fwd_bytes, void* ws_bwd,
                 size_t ws_bwd_bytes, sel_stream_t stream) {
  SEL_REQUIRE(clean && proc && g_proc && ws_fwd && ws_bwd, SEL_ERR_ARG, "sel_stoi_bwd: null pointer");
  SEL_REQUIRE(g_d || g_mean, SEL_ERR_ARG, "sel_stoi_bwd: no incoming gradient");
  SEL_REQUIRE(B > 0 && B <= 65535, SEL_ERR_ARG, "sel_stoi_bwd: B must be in [1, 65535]");
  SEL_REQUIRE(T >= kFrame && T <= (int64_t(1) << 30), SEL_ERR_ARG, "sel_stoi_bwd: T must be in [256, 2^30]");
  SEL_REQUIRE((extended | 1) == 1, SEL_ERR_ARG, "sel_stoi_bwd: extended must be 0 or 1");
  SEL_REQUIRE(reinterpret_cast<uintptr_t>(ws_fwd) % 8 == 0 && reinterpret_cast<uintptr_t>(ws_bwd) % 8 == 0,
              SEL_ERR_ARG, "sel_stoi_bwd: workspace not 8-byte aligned");
  SEL_REQUIRE(ws_fwd_bytes >= sel_stoi_workspace(B, T), SEL_ERR_WORKSPACE,
              "sel_stoi_bwd: forward workspace too small");
  SEL_REQUIRE(ws_bwd_bytes >= sel_stoi_bwd_workspace(B, T), SEL_ERR_WORKSPACE,
              "sel_stoi_bwd: backward workspace too small");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int F = int(stoi_frames(T));
  const int J = F > kSeg ? F - kSeg : 0;
  // the forward's layout (sel_stoi)
  const double* bands = static_cast<const double*>(ws_fwd) + size_t(B) * J;
  const int* kidx = reinterpret_cast<const int*>(bands + size_t(B) * 2 * (F - 1) * kBands) + size_t(B) * F;
  const int* cnt = kidx + size_t(B) * F;
  double* gseg = static_cast<double*>(ws_bwd);
  double* gz = gseg + size_t(B) * J * kSeg * kBands;
  int* inv = reinterpret_cast<int*>(gz + size_t(B) * (F - 1) * kFrame);
  if (J > 0) {  // fewer than 31 frames: every row is the constant 1e-5 and the gather writes zeros
    hipLaunchKernelGGL(k_stoi_seg_bwd, dim3(unsigned(J), unsigned(B)), dim3(64), 0, s, bands, cnt, B, F, extended,
                       g_d, g_mean, gseg);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stoi_col_bwd, dim3(unsigned(F - 1), unsigned(B)), dim3(64), 0, s, proc, T, F, kidx, cnt,
                       bands, gseg, gz);
    SEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stoi_inv, dim3(unsigned((F + 255) / 256), unsigned(B)), dim3(256), 0, s, kidx, cnt, F, inv);
    SEL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_stoi_gather, dim3(unsigned((T + 255) / 256), unsigned(B)), dim3(256), 0, s, gz, inv, cnt, T, F,
                     g_proc);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
