// Around the HiFi-GAN discriminators (dconv.hip): the data movement of their
// front-ends (the MSD's AvgPool1d, the MPD's period fold / unfold) and the GAN
// losses (losses/adversarial_loss.py, losses/feat_match_loss.py).
#include <algorithm>

#include "sel_common.h"

namespace sel {
namespace dconv {

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return float(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __bf16 from_f<__bf16>(float v) { return __bf16(v); }

// ---------------------------------------------------------------------------
// Data movement of the discriminator front-ends
// ---------------------------------------------------------------------------
// AvgPool1d(kernel 4, stride 2, padding 2, count_include_pad) between MSD scales
// (discriminator.py:428-447): (B, T) fp32 -> (B, Tout_alloc) with zeros past To.
__global__ void k_avgpool_fwd(const float* __restrict__ x, int B, int T, int ldx, int kw, int st, int pad,
                              int To, int ldo, float* __restrict__ y) {
  const int64_t total = int64_t(B) * ldo;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int b = int(i / ldo), t = int(i - int64_t(b) * ldo);
    float v = 0.f;
    if (t < To) {
      for (int k = 0; k < kw; ++k) {
        const int u = t * st + k - pad;
        if (u >= 0 && u < T) v += x[int64_t(b) * ldx + u];
      }
      v /= float(kw);
    }
    y[i] = v;
  }
}

__global__ void k_avgpool_bwd(const float* __restrict__ gy, int B, int T, int ldx, int kw, int st, int pad, int To,
                              int ldo, float* __restrict__ gx) {
  const int64_t total = int64_t(B) * ldx;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int b = int(i / ldx), u = int(i - int64_t(b) * ldx);
    float v = 0.f;
    if (u < T) {
      // outputs t with t*st + k - pad == u, 0 <= k < kw
      const int lo = (u + pad - kw + 1 + st - 1) / st > 0 ? (u + pad - kw + 1 + st - 1) / st : 0;
      for (int t = lo; t * st - pad <= u && t < To; ++t) v += gy[int64_t(b) * ldo + t];
      v /= float(kw);
    }
    gx[i] = v;
  }
}

// MPD front-end (discriminator.py:120-126): reflect-pad T to a multiple of the
// period p, view (B, 1, T/p, p) -> our (B*p, L_alloc) sequences (column-major
// over the p columns), rows past L zero.  Backward folds the reflect pad.
__global__ void k_mpd_fold(const float* __restrict__ x, int B, int T, int ldx, int p, int L, int Lalloc,
                           float* __restrict__ y) {
  const int64_t total = int64_t(B) * p * Lalloc;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t seq = i / Lalloc;
    const int l = int(i - seq * Lalloc);
    const int b = int(seq / p), col = int(seq - int64_t(b) * p);
    float v = 0.f;
    if (l < L) {
      int u = l * p + col;
      if (u >= T) u = 2 * (T - 1) - u;  // reflect (F.pad mode "reflect")
      v = x[int64_t(b) * ldx + u];
    }
    y[i] = v;
  }
}

__global__ void k_mpd_unfold(const float* __restrict__ gy, int B, int T, int ldx, int p, int L, int Lalloc,
                             float* __restrict__ gx) {
  const int64_t total = int64_t(B) * ldx;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int b = int(i / ldx), u = int(i - int64_t(b) * ldx);
    float v = 0.f;
    if (u < T) {
      v = gy[(int64_t(b) * p + u % p) * Lalloc + u / p];
      const int up = 2 * (T - 1) - u;  // padded position mirrored onto u
      if (up >= T && up < L * p) v += gy[(int64_t(b) * p + up % p) * Lalloc + up / p];
    }
    gx[i] = v;
  }
}

// ---------------------------------------------------------------------------
// GAN losses over strided (up to 4-D) views: sum |a - b| (feature matching) or
// sum (a - target)^2 (LSGAN) / sum min(+-a - 1, 0) (hinge), fp64 block partials,
// and their elementwise gradients written into a buffer of the same view.
// ---------------------------------------------------------------------------
struct View4 {
  int64_t size[4];
  int64_t stride[4];
};

// 4-D index of flat element i (last dim fastest) with 32-bit divisions (the host
// permutes the views to memory order, so the last dim is the contiguous one)
struct Idx4 {
  uint32_t i0, i1, i2, i3;
};
__device__ __forceinline__ Idx4 unflat(const View4& v, uint32_t i) {
  Idx4 r;
  const uint32_t s3 = uint32_t(v.size[3]), s2 = uint32_t(v.size[2]), s1 = uint32_t(v.size[1]);
  uint32_t q = i / s3;
  r.i3 = i - q * s3;
  uint32_t q2 = q / s2;
  r.i2 = q - q2 * s2;
  r.i0 = q2 / s1;
  r.i1 = q2 - r.i0 * s1;
  return r;
}
__device__ __forceinline__ int64_t off4(const View4& v, const Idx4& x) {
  return int64_t(x.i0) * v.stride[0] + int64_t(x.i1) * v.stride[1] + int64_t(x.i2) * v.stride[2] +
         int64_t(x.i3) * v.stride[3];
}

// per-element loss term and its derivative (times coef c)
__device__ __forceinline__ float gan_val(int kind, float x, float y, float target) {
  if (kind == 0) return fabsf(x - y);                  // L1
  if (kind == 1) return (x - target) * (x - target);   // MSE to target
  if (kind == 2) return fminf(x - 1.f, 0.f);           // hinge real: min(x - 1, 0)
  if (kind == 3) return fminf(-x - 1.f, 0.f);          // hinge fake: min(-x - 1, 0)
  return x;                                            // plain sum (generator hinge: -mean)
}
__device__ __forceinline__ float gan_dval(int kind, float x, float y, float target, float c) {
  if (kind == 0) {
    const float dlt = x - y;
    return dlt > 0.f ? c : (dlt < 0.f ? -c : 0.f);
  }
  if (kind == 1) return 2.f * (x - target) * c;
  if (kind == 2) return x - 1.f < 0.f ? c : 0.f;
  if (kind == 3) return -x - 1.f < 0.f ? -c : 0.f;
  return c;
}

template <typename T>
__global__ __launch_bounds__(256) void k_gan_reduce(int kind, const T* __restrict__ a, View4 va,
                                                    const T* __restrict__ b, View4 vb, float target, int64_t n,
                                                    double* __restrict__ partials) {
  __shared__ double red[16];
  float s = 0.f;  // per-thread partial (<= a few hundred terms), fp64 across threads and blocks
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const Idx4 ix = unflat(va, uint32_t(i));
    const float x = to_f(a[off4(va, ix)]);
    s += gan_val(kind, x, kind == 0 ? to_f(b[off4(vb, ix)]) : 0.f, target);
  }
  const double t = block_sum(double(s), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// 16-B vector forms: every view's last dim contiguous with a multiple of V = 16 /
// sizeof(T) elements, the other strides multiples of V and the bases 16-B
// aligned (the channels-last feature maps): one index decomposition and one
// 16-B load per V elements instead of per element
template <typename T>
struct Vec16 {
  static constexpr int V = 16 / sizeof(T);
  T v[V];
};

template <typename T>
__global__ __launch_bounds__(256) void k_gan_reduce_v(int kind, const T* __restrict__ a, View4 va,
                                                      const T* __restrict__ b, View4 vb, float target, uint32_t nv,
                                                      double* __restrict__ partials) {
  constexpr int V = Vec16<T>::V;
  __shared__ double red[16];
  float s = 0.f;
  for (uint32_t iv = blockIdx.x * 256u + threadIdx.x; iv < nv; iv += gridDim.x * 256u) {
    const Idx4 ix = unflat(va, iv * V);
    const Vec16<T> xa = *reinterpret_cast<const Vec16<T>*>(a + off4(va, ix));
    Vec16<T> xb;
    if (kind == 0) xb = *reinterpret_cast<const Vec16<T>*>(b + off4(vb, ix));
#pragma unroll
    for (int e = 0; e < V; ++e) s += gan_val(kind, to_f(xa.v[e]), kind == 0 ? to_f(xb.v[e]) : 0.f, target);
  }
  const double t = block_sum(double(s), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ void k_gan_finish(const double* __restrict__ partials, int nblocks, double scale, float* __restrict__ out,
                             int accumulate) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) s += partials[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = float(s * scale) + (accumulate ? out[0] : 0.f);
}

// grad[i] (+)= coef * dv/da (coef is a device scalar: the upstream grad / n)
template <typename T>
__global__ __launch_bounds__(256) void k_gan_grad(int kind, const T* __restrict__ a, View4 va,
                                                  const T* __restrict__ b, View4 vb, float target, int64_t n,
                                                  const float* __restrict__ gscale, float mult,
                                                  T* __restrict__ grad, View4 vg, int accumulate) {
  const float c = gscale[0] * mult;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const Idx4 ix = unflat(va, uint32_t(i));
    const float x = to_f(a[off4(va, ix)]);
    const float gv = gan_dval(kind, x, kind == 0 ? to_f(b[off4(vb, ix)]) : 0.f, target, c);
    const int64_t o = off4(vg, ix);
    grad[o] = from_f<T>(accumulate ? to_f(grad[o]) + gv : gv);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_gan_grad_v(int kind, const T* __restrict__ a, View4 va,
                                                    const T* __restrict__ b, View4 vb, float target, uint32_t nv,
                                                    const float* __restrict__ gscale, float mult,
                                                    T* __restrict__ grad, View4 vg, int accumulate) {
  constexpr int V = Vec16<T>::V;
  const float c = gscale[0] * mult;
  for (uint32_t iv = blockIdx.x * 256u + threadIdx.x; iv < nv; iv += gridDim.x * 256u) {
    const Idx4 ix = unflat(va, iv * V);
    const Vec16<T> xa = *reinterpret_cast<const Vec16<T>*>(a + off4(va, ix));
    Vec16<T> xb, go;
    if (kind == 0) xb = *reinterpret_cast<const Vec16<T>*>(b + off4(vb, ix));
    Vec16<T>* gp = reinterpret_cast<Vec16<T>*>(grad + off4(vg, ix));
    if (accumulate) go = *gp;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float gv = gan_dval(kind, to_f(xa.v[e]), kind == 0 ? to_f(xb.v[e]) : 0.f, target, c);
      go.v[e] = from_f<T>(accumulate ? to_f(go.v[e]) + gv : gv);
    }
    *gp = go;
  }
}

// the 16-B vector kernels apply to this view (see Vec16)
template <typename T>
bool vec_view(const void* base, const View4& v) {
  constexpr int V = 16 / sizeof(T);
  return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && v.stride[3] == 1 && v.size[3] % V == 0 &&
         v.stride[0] % V == 0 && v.stride[1] % V == 0 && v.stride[2] % V == 0;
}

}  // namespace dconv
}  // namespace sel

using namespace sel;
using namespace sel::dconv;

namespace {

int launch_blocks(int64_t n) { return int(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192))); }

bool view_ok(const int64_t* size, const int64_t* stride) { return size && stride; }

View4 to_view(const int64_t* size, const int64_t* stride, int ndim) {
  View4 v;
  for (int i = 0; i < 4; ++i) {
    const int src = i - (4 - ndim);
    v.size[i] = src >= 0 ? size[src] : 1;
    v.stride[i] = src >= 0 ? stride[src] : 0;
  }
  return v;
}

}  // namespace

extern "C" {

int sel_avgpool1d_fwd(const float* x, int B, int T, int ldx, int kernel, int stride, int pad, int To, int ldo,
                      float* y, sel_stream_t stream) {
  SEL_REQUIRE(x && y && B > 0 && T > 0 && ldx >= T && kernel > 0 && stride > 0 && ldo >= To && To > 0, SEL_ERR_ARG,
              "bad avgpool arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_avgpool_fwd, dim3(launch_blocks(int64_t(B) * ldo)), dim3(256), 0, s, x, B, T, ldx, kernel,
                     stride, pad, To, ldo, y);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_avgpool1d_bwd(const float* gy, int B, int T, int ldx, int kernel, int stride, int pad, int To, int ldo,
                      float* gx, sel_stream_t stream) {
  SEL_REQUIRE(gy && gx && B > 0 && T > 0 && ldx >= T && kernel > 0 && stride > 0 && ldo >= To, SEL_ERR_ARG,
              "bad avgpool arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_avgpool_bwd, dim3(launch_blocks(int64_t(B) * ldx)), dim3(256), 0, s, gy, B, T, ldx, kernel,
                     stride, pad, To, ldo, gx);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_mpd_fold(const float* x, int B, int T, int ldx, int period, int Lalloc, float* y, sel_stream_t stream) {
  SEL_REQUIRE(x && y && B > 0 && period > 0 && T > period && ldx >= T, SEL_ERR_ARG, "bad mpd fold arguments");
  const int L = (T + period - 1) / period;
  SEL_REQUIRE(Lalloc >= L, SEL_ERR_ARG, "Lalloc %d < L %d", Lalloc, L);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mpd_fold, dim3(launch_blocks(int64_t(B) * period * Lalloc)), dim3(256), 0, s, x, B, T, ldx,
                     period, L, Lalloc, y);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_mpd_unfold(const float* gy, int B, int T, int ldx, int period, int Lalloc, float* gx, sel_stream_t stream) {
  SEL_REQUIRE(gy && gx && B > 0 && period > 0 && T > period && ldx >= T, SEL_ERR_ARG, "bad mpd unfold arguments");
  const int L = (T + period - 1) / period;
  SEL_REQUIRE(Lalloc >= L, SEL_ERR_ARG, "Lalloc %d < L %d", Lalloc, L);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mpd_unfold, dim3(launch_blocks(int64_t(B) * ldx)), dim3(256), 0, s, gy, B, T, ldx, period, L,
                     Lalloc, gx);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

size_t sel_gan_workspace(void) { return 1024 * sizeof(double); }

int sel_gan_reduce(int kind, int dtype, const void* a, const int64_t* a_size, const int64_t* a_stride,
                   const void* b, const int64_t* b_size, const int64_t* b_stride, int ndim, float target,
                   double scale, int accumulate, float* out, void* ws, size_t ws_bytes, sel_stream_t stream) {
  SEL_REQUIRE(kind >= 0 && kind <= 4 && a && out && ndim >= 1 && ndim <= 4 && view_ok(a_size, a_stride),
              SEL_ERR_ARG, "bad gan reduce arguments");
  SEL_REQUIRE(kind != 0 || (b && view_ok(b_size, b_stride)), SEL_ERR_ARG, "L1 needs b");
  SEL_REQUIRE(ws_bytes >= sel_gan_workspace(), SEL_ERR_WORKSPACE, "workspace too small");
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    n *= a_size[i];
    if (kind == 0) SEL_REQUIRE(b_size[i] == a_size[i], SEL_ERR_ARG, "shape mismatch");
  }
  SEL_REQUIRE(n < (int64_t(1) << 32), SEL_ERR_ARG, "view too large (%lld elements)", (long long)n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const View4 va = to_view(a_size, a_stride, ndim);
  const View4 vb = kind == 0 ? to_view(b_size, b_stride, ndim) : va;
  double* part = static_cast<double*>(ws);
  const void* bb = b ? b : a;
  const bool vec = dtype == SEL_BF16 ? vec_view<__bf16>(a, va) && (kind != 0 || vec_view<__bf16>(bb, vb))
                                     : vec_view<float>(a, va) && (kind != 0 || vec_view<float>(bb, vb));
  const int vw = dtype == SEL_BF16 ? 8 : 4;
  const int64_t nt = vec ? n / vw : n;  // threads' work items
  const int nb = int(std::min<int64_t>(1024, std::max<int64_t>(1, (nt + 255) / 256)));
  if (dtype == SEL_BF16 && vec)
    hipLaunchKernelGGL(k_gan_reduce_v<__bf16>, dim3(nb), dim3(256), 0, s, kind, static_cast<const __bf16*>(a), va,
                       static_cast<const __bf16*>(bb), vb, target, uint32_t(nt), part);
  else if (dtype == SEL_BF16)
    hipLaunchKernelGGL(k_gan_reduce<__bf16>, dim3(nb), dim3(256), 0, s, kind, static_cast<const __bf16*>(a), va,
                       static_cast<const __bf16*>(bb), vb, target, n, part);
  else if (vec)
    hipLaunchKernelGGL(k_gan_reduce_v<float>, dim3(nb), dim3(256), 0, s, kind, static_cast<const float*>(a), va,
                       static_cast<const float*>(bb), vb, target, uint32_t(nt), part);
  else
    hipLaunchKernelGGL(k_gan_reduce<float>, dim3(nb), dim3(256), 0, s, kind, static_cast<const float*>(a), va,
                       static_cast<const float*>(bb), vb, target, n, part);
  hipLaunchKernelGGL(k_gan_finish, dim3(1), dim3(256), 0, s, part, nb, scale, out, accumulate);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_gan_grad(int kind, int dtype, const void* a, const int64_t* a_size, const int64_t* a_stride, const void* b,
                 const int64_t* b_size, const int64_t* b_stride, int ndim, float target, const float* gscale,
                 float mult, void* grad, const int64_t* g_stride, int accumulate, sel_stream_t stream) {
  SEL_REQUIRE(kind >= 0 && kind <= 4 && a && grad && gscale && ndim >= 1 && ndim <= 4 && view_ok(a_size, a_stride) &&
                  g_stride,
              SEL_ERR_ARG, "bad gan grad arguments");
  SEL_REQUIRE(kind != 0 || (b && view_ok(b_size, b_stride)), SEL_ERR_ARG, "L1 needs b");
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= a_size[i];
  SEL_REQUIRE(n < (int64_t(1) << 32), SEL_ERR_ARG, "view too large (%lld elements)", (long long)n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const View4 va = to_view(a_size, a_stride, ndim);
  const View4 vb = kind == 0 ? to_view(b_size, b_stride, ndim) : va;
  const View4 vg = to_view(a_size, g_stride, ndim);
  const void* bb = b ? b : a;
  const bool vec = dtype == SEL_BF16 ? vec_view<__bf16>(a, va) && vec_view<__bf16>(grad, vg) &&
                                           (kind != 0 || vec_view<__bf16>(bb, vb))
                                     : vec_view<float>(a, va) && vec_view<float>(grad, vg) &&
                                           (kind != 0 || vec_view<float>(bb, vb));
  const int64_t nt = vec ? n / (dtype == SEL_BF16 ? 8 : 4) : n;
  const unsigned nb = unsigned(launch_blocks(nt));
  if (dtype == SEL_BF16 && vec)
    hipLaunchKernelGGL(k_gan_grad_v<__bf16>, dim3(nb), dim3(256), 0, s, kind, static_cast<const __bf16*>(a), va,
                       static_cast<const __bf16*>(bb), vb, target, uint32_t(nt), gscale, mult,
                       static_cast<__bf16*>(grad), vg, accumulate);
  else if (vec)
    hipLaunchKernelGGL(k_gan_grad_v<float>, dim3(nb), dim3(256), 0, s, kind, static_cast<const float*>(a), va,
                       static_cast<const float*>(bb), vb, target, uint32_t(nt), gscale, mult,
                       static_cast<float*>(grad), vg, accumulate);
  else if (dtype == SEL_BF16)
    hipLaunchKernelGGL(k_gan_grad<__bf16>, dim3(nb), dim3(256), 0, s, kind, static_cast<const __bf16*>(a), va,
                       static_cast<const __bf16*>(b ? b : a), vb, target, n, gscale, mult,
                       static_cast<__bf16*>(grad), vg, accumulate);
  else
    hipLaunchKernelGGL(k_gan_grad<float>, dim3(nb), dim3(256), 0, s, kind, static_cast<const float*>(a), va,
                       static_cast<const float*>(b ? b : a), vb, target, n, gscale, mult, static_cast<float*>(grad),
                       vg, accumulate);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
