// Weight packing of the discriminator conv primitive (dconv.hip): torch
// Conv1d / (k,1) Conv2d weight [N][Cg][Kt], optional weight norm
// w = g * v / ||v||, into the phase-view forms
//   fwd  Wp[g][n][i][r][c] = w[g*Ng + n][c][s*(q0 + i) + r + pad]   (0 if out of [0, Kt))
//   dgrad Wd[g][(r,c)][i'][n] = Wp[g][n][K-1-i'][r][c]
#include "dconv_common.h"

namespace sel {
namespace dconv {

// one block per output channel n: ||v_n|| then the packed weights
template <typename T>
__device__ __forceinline__ void dpack_channel(const PackGeo& pg, int mode, const float* __restrict__ w,
                                              const float* __restrict__ wg, T* __restrict__ out, int n);

template <typename T>
__global__ __launch_bounds__(256) void k_dpack(PackGeo pg, int mode, const float* __restrict__ w,
                                               const float* __restrict__ wg, T* __restrict__ out) {
  dpack_channel<T>(pg, mode, w, wg, out, blockIdx.x);
}

// batched form: block ranges per job in the kernel argument
constexpr int DPM_MAXJ = 24;
struct DPackJobs {
  PackGeo pg[DPM_MAXJ];
  const float* w[DPM_MAXJ];
  const float* wg[DPM_MAXJ];
  void* out[DPM_MAXJ];
  int mode[DPM_MAXJ];
  int bstart[DPM_MAXJ + 1];
  int njobs;
};

template <typename T>
__global__ __launch_bounds__(256) void k_dpack_many(DPackJobs dj) {
  int j = 0;
  while (j + 1 < dj.njobs && int(blockIdx.x) >= dj.bstart[j + 1]) ++j;  // block-uniform
  dpack_channel<T>(dj.pg[j], dj.mode[j], dj.w[j], dj.wg[j], static_cast<T*>(dj.out[j]),
                   int(blockIdx.x) - dj.bstart[j]);
}

// mode-2 jobs: the adjoint form as a tiled transpose of the forward form just
// packed (Wp[g][nl][i][rc] -> Wd[g][rc][K-1-i][nl]): pure data movement, so the
// adjoint holds exactly the forward form's values, with coalesced reads and
// writes (the per-channel adjoint pack writes every element Ng apart).
// Block = (job, group, 64 output channels, 64 (tap, reduction) columns).
struct DPackTrJobs {
  PackGeo pg[DPM_MAXJ];
  const void* src[DPM_MAXJ];
  void* out[DPM_MAXJ];
  int ntn[DPM_MAXJ], ntc[DPM_MAXJ];  // channel / column tiles per group
  int bstart[DPM_MAXJ + 1];
  int njobs;
};

template <typename T>
__global__ __launch_bounds__(256) void k_dpack_tr_many(DPackTrJobs dj) {
  __shared__ T tile[64][65];
  int j = 0;
  while (j + 1 < dj.njobs && int(blockIdx.x) >= dj.bstart[j + 1]) ++j;  // block-uniform
  const PackGeo& pg = dj.pg[j];
  const T* __restrict__ src = static_cast<const T*>(dj.src[j]);
  T* __restrict__ out = static_cast<T*>(dj.out[j]);
  const int lb = int(blockIdx.x) - dj.bstart[j];
  const int ct = lb % dj.ntc[j], nt = (lb / dj.ntc[j]) % dj.ntn[j], g = lb / (dj.ntc[j] * dj.ntn[j]);
  const int Ng = pg.N / pg.G, nred = pg.s * pg.Cg, cols = pg.K * nred;
  const int nl0 = nt * 64, c0 = ct * 64;
  const int t = threadIdx.x, lo = t & 63, hi = t >> 6;
#pragma unroll 4
  for (int r = hi; r < 64; r += 4) {  // rows = output channels, columns = (i, rc) contiguous
    const int nl = nl0 + r, c = c0 + lo;
    if (nl < Ng && c < cols) tile[r][lo] = src[(int64_t(g) * Ng + nl) * cols + c];
  }
  __syncthreads();
#pragma unroll 4
  for (int q = hi; q < 64; q += 4) {  // column q of the tile -> one Wd row, channels contiguous
    const int c = c0 + q, nl = nl0 + lo;
    if (nl < Ng && c < cols) {
      const int i = c / nred, rc = c - i * nred;
      out[((int64_t(g) * nred + rc) * pg.K + (pg.K - 1 - i)) * Ng + nl] = tile[lo][q];
    }
  }
}

template <typename T>
__device__ __forceinline__ void dpack_channel(const PackGeo& pg, int mode, const float* __restrict__ w,
                                              const float* __restrict__ wg, T* __restrict__ out, int n) {
  __shared__ float red[16];
  const int per = pg.Cg * pg.Kt;
  float scale = 1.f;
  if (wg) {
    float ss = 0.f;
    for (int e = threadIdx.x; e < per; e += 256) {
      const float v = w[int64_t(n) * per + e];
      ss += v * v;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) red[0] = ss;
    __syncthreads();
    scale = wg[n] / sqrtf(red[0]);
  }
  const int Ng = pg.N / pg.G, g = n / Ng, nl = n - g * Ng;
  const int nred = pg.s * pg.Cg;
  for (int e = threadIdx.x; e < pg.K * nred; e += 256) {
    const int i = e / nred, rc = e - i * nred;
    const int r = rc / pg.Cg, c = rc - r * pg.Cg;
    const int k = pg.s * (pg.q0 + i) + r + pg.pad;
    const float v = (k >= 0 && k < pg.Kt) ? w[(int64_t(n) * pg.Cg + c) * pg.Kt + k] * scale : 0.f;
    if (mode == 0) {
      out[((int64_t(g) * Ng + nl) * pg.K + i) * nred + rc] = from_f<T>(v);
    } else {  // dgrad: [g][(r,c)][K-1-i][n]
      out[((int64_t(g) * nred + rc) * pg.K + (pg.K - 1 - i)) * Ng + nl] = from_f<T>(v);
    }
  }
}

}  // namespace dconv
}  // namespace sel

using namespace sel;
using namespace sel::dconv;

extern "C" {

int sel_dconv_geometry(int Kt, int stride, int pad, int* K, int* q0) {
  SEL_REQUIRE(Kt > 0 && stride > 0 && pad >= 0 && K && q0, SEL_ERR_ARG, "bad conv geometry");
  const PackGeo pg = pack_geo(1, 1, Kt, stride, pad, 1);
  *K = pg.K;
  *q0 = pg.q0;
  return SEL_OK;
}

int sel_dconv_pack(int mode, const float* w, const float* wg, int N, int Cg, int Kt, int stride, int pad, int G,
                   int dtype, void* out, sel_stream_t stream) {
  SEL_REQUIRE(w && out && N > 0 && Cg > 0 && Kt > 0 && stride > 0 && pad >= 0 && G > 0 && N % G == 0 &&
                  (mode == 0 || mode == 1),
              SEL_ERR_ARG, "bad dconv pack arguments");
  const PackGeo pg = pack_geo(N, Cg, Kt, stride, pad, G);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SEL_BF16)
    hipLaunchKernelGGL(k_dpack<__bf16>, dim3(N), dim3(256), 0, s, pg, mode, w, wg, static_cast<__bf16*>(out));
  else if (dtype == SEL_F32)
    hipLaunchKernelGGL(k_dpack<float>, dim3(N), dim3(256), 0, s, pg, mode, w, wg, static_cast<float*>(out));
  else {
    set_error("sel_dconv_pack: dtype %d", dtype);
    return SEL_ERR_UNSUPPORTED;
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_dconv_pack_many(const sel_dpack_job* jobs, int njobs, int dtype, sel_stream_t stream) {
  SEL_REQUIRE(njobs >= 0 && (njobs == 0 || jobs) && (dtype == SEL_BF16 || dtype == SEL_F32), SEL_ERR_ARG,
              "bad dconv pack job list");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int j = 0; j < njobs; ++j) {
    const sel_dpack_job& J = jobs[j];
    SEL_REQUIRE(J.w && J.out && J.N > 0 && J.Cg > 0 && J.Kt > 0 && J.stride > 0 && J.pad >= 0 && J.G > 0 &&
                    J.N % J.G == 0 && (J.mode == 0 || J.mode == 1 || J.mode == 2),
                SEL_ERR_ARG, "bad dconv pack job %d", j);
  }
  // modes 0 / 1 from the torch weights, then the mode-2 transposes of forward
  // forms (possibly packed by the first launch: stream order)
  for (int pass = 0; pass < 2; ++pass) {
    int j = 0;
    while (j < njobs) {
      DPackJobs dj{};
      DPackTrJobs tj{};
      int n = 0, blocks = 0;
      for (; j < njobs && n < DPM_MAXJ; ++j) {
        const sel_dpack_job& J = jobs[j];
        if ((J.mode == 2) != (pass == 1)) continue;
        const PackGeo pg = pack_geo(J.N, J.Cg, J.Kt, J.stride, J.pad, J.G);
        if (pass == 0) {
          dj.pg[n] = pg;
          dj.w[n] = J.w;
          dj.wg[n] = J.wg;
          dj.out[n] = J.out;
          dj.mode[n] = J.mode;
          dj.bstart[n] = blocks;
          blocks += J.N;
        } else {
          tj.pg[n] = pg;
          tj.src[n] = J.w;
          tj.out[n] = J.out;
          tj.ntn[n] = (J.N / J.G + 63) / 64;
          tj.ntc[n] = (pg.K * J.stride * J.Cg + 63) / 64;
          tj.bstart[n] = blocks;
          blocks += J.G * tj.ntn[n] * tj.ntc[n];
        }
        ++n;
      }
      if (n == 0 || blocks == 0) continue;
      if (pass == 0) {
        dj.njobs = n;
        dj.bstart[n] = blocks;
        if (dtype == SEL_BF16)
          hipLaunchKernelGGL(k_dpack_many<__bf16>, dim3(unsigned(blocks)), dim3(256), 0, s, dj);
        else
          hipLaunchKernelGGL(k_dpack_many<float>, dim3(unsigned(blocks)), dim3(256), 0, s, dj);
      } else {
        tj.njobs = n;
        tj.bstart[n] = blocks;
        if (dtype == SEL_BF16)
          hipLaunchKernelGGL(k_dpack_tr_many<__bf16>, dim3(unsigned(blocks)), dim3(256), 0, s, tj);
        else
          hipLaunchKernelGGL(k_dpack_tr_many<float>, dim3(unsigned(blocks)), dim3(256), 0, s, tj);
      }
      SEL_LAUNCH_CHECK();
    }
  }
  return SEL_OK;
}

}  // extern "C"
