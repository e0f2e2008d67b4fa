// Weight packing and unpacking, the replicate-pad dgrad fix-up and the dtype
// cast of the conv stack, with their entry points.
#include <algorithm>

#include "conv_common.h"

namespace sel {
namespace conv {

// ---------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------
// strided fwd pack: Wp[co][tap][ph*Cin+ci] = W[co][ci][k(tap,ph)]
__device__ __forceinline__ int strided_k(int tap, int ph, int s) {
  if (tap == 0) return ph >= 1 ? ph - 1 : -1;
  if (tap == 1) return ph + s - 1;
  return ph == 0 ? 2 * s - 1 : -1;
}

template <typename TO>
__global__ void k_pack(int kind, const float* __restrict__ w, int cout, int cin, int K, int s,
                       TO* __restrict__ wp) {
  int64_t total;
  if (kind == SEL_PACK_FWD) total = int64_t(cout) * K * cin;
  else if (kind == SEL_PACK_FWD_STRIDED) total = int64_t(cout) * 3 * s * cin;
  else total = int64_t(s) * cout * 2 * cin;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * blockDim.x) {
    float v = 0.f;
    if (kind == SEL_PACK_FWD) {
      const int c = int(i % cin);
      const int k = int((i / cin) % K);
      const int n = int(i / (int64_t(cin) * K));
      v = w[(int64_t(n) * cin + c) * K + k];
    } else if (kind == SEL_PACK_FWD_STRIDED) {
      const int Cp = s * cin;
      const int cp = int(i % Cp);
      const int tap = int((i / Cp) % 3);
      const int n = int(i / (int64_t(Cp) * 3));
      const int ph = cp / cin, ci = cp % cin;
      const int k = strided_k(tap, ph, s);
      v = k >= 0 ? w[(int64_t(n) * cin + ci) * (2 * s) + k] : 0.f;
    } else {  // CONVT: Wp[(ph*cout+co)][tap][ci] = Wt[ci][co][tap==0 ? ph+s : ph]
      const int ci = int(i % cin);
      const int tap = int((i / cin) % 2);
      const int nn = int(i / (int64_t(cin) * 2));
      const int ph = nn / cout, co = nn % cout;
      const int k = tap == 0 ? ph + s : ph;
      v = w[(int64_t(ci) * cout + co) * (2 * s) + k];
    }
    wp[i] = from_f<TO>(v);
  }
}

template <typename T>
__global__ void k_pack_dgrad(const T* __restrict__ wp, int N, int K, int C, T* __restrict__ wd) {
  const int64_t total = int64_t(N) * K * C;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * blockDim.x) {
    // wd[c][j][n] = wp[n][K-1-j][c]
    const int n = int(i % N);
    const int j = int((i / N) % K);
    const int c = int(i / (int64_t(N) * K));
    wd[i] = wp[(int64_t(n) * K + (K - 1 - j)) * C + c];
  }
}

// Multi-tensor pack: every job's fwd pack Wp and (optionally) its dgrad form Wd
// in ONE launch (the per-layer launches of sel_pack_weight + sel_pack_dgrad were
// ~120 x 4 us per training step).  Grid-stride over TWO ranges of the
// concatenated packed elements: [0, total) writes Wp in its own order, [total,
// 2 total) writes Wd in ITS own order (gathering the source element), so both
// write streams are coalesced (writing Wd as the transpose of the Wp walk made
// every 2-B store its own partial line: 45 us per C3 step).  A thread
// binary-searches its job in the device job table.
template <typename TO>
__global__ void k_pack_many(const sel_pack_job* __restrict__ jobs, int njobs, int64_t total) {
  for (int64_t i2 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i2 < 2 * total;
       i2 += int64_t(gridDim.x) * blockDim.x) {
    const bool dg = i2 >= total;  // dgrad-form range
    const int64_t i = dg ? i2 - total : i2;
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (jobs[mid].offset <= i) lo = mid;
      else hi = mid - 1;
    }
    const sel_pack_job& J = jobs[lo];
    if (dg && !J.wdgrad) continue;
    // a layer's packed index fits 32 bits (host-checked): unsigned 32-bit
    // division instead of the 64-bit sequences (the per-step pack of the C3
    // weights took 105 us with them)
    const unsigned li = unsigned(i - J.offset);
    const unsigned s = unsigned(J.stride), cin = unsigned(J.cin), cout = unsigned(J.cout), K = unsigned(J.k);
    // packed geometry: Wp[n][kp][cp] (N rows, KP taps, CP channels per tap)
    unsigned N, KP, CP;
    if (J.kind == SEL_PACK_FWD) N = cout, KP = K, CP = cin;
    else if (J.kind == SEL_PACK_FWD_STRIDED) N = cout, KP = 3, CP = s * cin;
    else N = s * cout, KP = 2, CP = cin;
    unsigned n, kp, cp;
    if (!dg) {  // li = (n * KP + kp) * CP + cp
      const unsigned q = li / CP;
      cp = li - q * CP;
      n = q / KP;
      kp = q - n * KP;
    } else {  // Wd[c][j][n] = Wp[n][KP-1-j][c]: li = (cp * KP + j) * N + n
      const unsigned r = li / N;
      n = li - r * N;
      cp = r / KP;
      kp = KP - 1 - (r - cp * KP);
    }
    float v = 0.f;
    if (J.kind == SEL_PACK_FWD) {
      v = J.w[(n * cin + cp) * K + kp];
    } else if (J.kind == SEL_PACK_FWD_STRIDED) {
      const unsigned ph = cp / cin, ci = cp - ph * cin;
      const int k = strided_k(int(kp), int(ph), int(s));
      v = k >= 0 ? J.w[(n * cin + ci) * (2 * s) + unsigned(k)] : 0.f;
    } else {
      const unsigned ph = n / cout, co = n - ph * cout;
      const unsigned k = kp == 0 ? ph + s : ph;
      v = J.w[(cp * cout + co) * (2 * s) + k];
    }
    static_cast<TO*>(dg ? J.wdgrad : J.wpack)[li] = from_f<TO>(v);
  }
}

// The same with the job table in the kernel arguments (sel_pack_many_host): no
// device copy of the table, hence no pinned staging and no host-to-device copy
// in the step (the pinned allocation + copy per weight update of the device-table
// form left the GPU idle ~0.3 ms per C3 step while the host waited on them).
// A launch packs the element range [lo, hi) of `total` that its jobs cover.
constexpr int PM_MAXJ = 48;
struct PackJobs {
  sel_pack_job j[PM_MAXJ];
  int n;
};
template <typename TO>
__global__ void k_pack_many_arg(PackJobs pj, int64_t lo, int64_t hi, int64_t total) {
  const int64_t len = hi - lo;
  for (int64_t i2 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i2 < 2 * len;
       i2 += int64_t(gridDim.x) * blockDim.x) {
    const bool dg = i2 >= len;
    const int64_t i = lo + (dg ? i2 - len : i2);
    int a = 0, b = pj.n - 1;
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if (pj.j[mid].offset <= i) a = mid;
      else b = mid - 1;
    }
    const sel_pack_job& J = pj.j[a];
    if (dg && !J.wdgrad) continue;
    const unsigned li = unsigned(i - J.offset);
    const unsigned s = unsigned(J.stride), cin = unsigned(J.cin), cout = unsigned(J.cout), K = unsigned(J.k);
    unsigned N, KP, CP;
    if (J.kind == SEL_PACK_FWD) N = cout, KP = K, CP = cin;
    else if (J.kind == SEL_PACK_FWD_STRIDED) N = cout, KP = 3, CP = s * cin;
    else N = s * cout, KP = 2, CP = cin;
    unsigned n, kp, cp;
    if (!dg) {
      const unsigned q = li / CP;
      cp = li - q * CP;
      n = q / KP;
      kp = q - n * KP;
    } else {
      const unsigned r = li / N;
      n = li - r * N;
      cp = r / KP;
      kp = KP - 1 - (r - cp * KP);
    }
    float v = 0.f;
    if (J.kind == SEL_PACK_FWD) {
      v = J.w[(n * cin + cp) * K + kp];
    } else if (J.kind == SEL_PACK_FWD_STRIDED) {
      const unsigned ph = cp / cin, ci = cp - ph * cin;
      const int k = strided_k(int(kp), int(ph), int(s));
      v = k >= 0 ? J.w[(n * cin + ci) * (2 * s) + unsigned(k)] : 0.f;
    } else {
      const unsigned ph = n / cout, co = n - ph * cout;
      const unsigned k = kp == 0 ? ph + s : ph;
      v = J.w[(cp * cout + co) * (2 * s) + k];
    }
    static_cast<TO*>(dg ? J.wdgrad : J.wpack)[li] = from_f<TO>(v);
  }
  (void)total;
}

// Tiled form of k_pack_many_arg (the product's per-step repack): a workgroup
// owns a 32 (n) x 32 (cp) x KP tile of one job's packed geometry, gathers it
// from the torch-layout weight with (cp, kp)-contiguous reads into an fp32 LDS
// tile, then writes the tile's forward form Wp[n][kp][cp] (32 consecutive cp per
// run) and its dgrad form Wd[cp][KP-1-kp][n] (32 consecutive n per run): both
// forms leave as coalesced runs.  The per-element form gathered the dgrad
// form's source across whole weight rows (one cache line per lane): 72 us per
// C3 step for 31 MB of traffic (rocprof, profiles/r6f_kernel_stats.md).  Same
// values (a copy with the same rounding).
constexpr int PT_T = 32, PT_KMAX = 8, PT_P = PT_T + 1;
struct PackTiles {
  sel_pack_job j[PM_MAXJ];
  int tstart[PM_MAXJ + 1];  // first tile of each job; tstart[n] = tile count
  int n;
};
__device__ __forceinline__ void pack_geom(const sel_pack_job& J, unsigned& N, unsigned& KP, unsigned& CP) {
  const unsigned s = unsigned(J.stride), cin = unsigned(J.cin), cout = unsigned(J.cout), K = unsigned(J.k);
  if (J.kind == SEL_PACK_FWD) N = cout, KP = K, CP = cin;
  else if (J.kind == SEL_PACK_FWD_STRIDED) N = cout, KP = 3, CP = s * cin;
  else N = s * cout, KP = 2, CP = cin;
}
// 1024 threads: one (n, cp) pair of the 32 x 32 tile per thread, with all its
// KP taps, so no index needs a division by the job's tap count, and the KP
// loads of a pair are all issued before its LDS stores.  (At 256 threads, four
// elements a thread one after another, the small launches of a C3 step -- 32-64
// tiles, one workgroup each -- took 17-18 us; now 6-7 us, and the 640-tile
// launch 11.4 -> 9.8 us.)
template <typename TO, unsigned PT_THREADS>
__global__ __launch_bounds__(PT_THREADS) void k_pack_tiles(PackTiles pt) {
  __shared__ float tile[PT_T * PT_KMAX * PT_P];
  int a = 0, b = pt.n - 1;
  const int t = int(blockIdx.x);
  while (a < b) {  // block-uniform
    const int mid = (a + b + 1) >> 1;
    if (pt.tstart[mid] <= t) a = mid;
    else b = mid - 1;
  }
  const sel_pack_job& J = pt.j[a];
  unsigned N, KP, CP;
  pack_geom(J, N, KP, CP);
  const unsigned s = unsigned(J.stride), cin = unsigned(J.cin), cout = unsigned(J.cout), K = unsigned(J.k);
  const unsigned ntc = (CP + PT_T - 1) / PT_T;
  const unsigned lt = unsigned(t - pt.tstart[a]);
  const unsigned n0 = (lt / ntc) * PT_T, c0 = (lt % ntc) * PT_T;
  // gather: pair (nl, cl), cl fastest; its KP taps are contiguous in the FWD
  // source; out-of-range taps load w[0] and are replaced by zeros
  for (unsigned r = threadIdx.x; r < PT_T * PT_T; r += PT_THREADS) {
    const unsigned cl = r % PT_T, nl = r / PT_T;
    const unsigned n = n0 + nl, cp = c0 + cl;
    const bool in = n < N && cp < CP;
    unsigned base = 0, ph = 0;
    if (J.kind == SEL_PACK_FWD) {
      base = (n * cin + cp) * K;
    } else if (J.kind == SEL_PACK_FWD_STRIDED) {
      ph = cp / cin;
      base = (n * cin + (cp - ph * cin)) * (2 * s);
    } else {
      ph = n / cout;
      base = (cp * cout + (n - ph * cout)) * (2 * s);
    }
    float v[PT_KMAX];
    bool ok[PT_KMAX];
#pragma unroll
    for (unsigned kp = 0; kp < PT_KMAX; ++kp) {
      if (kp >= KP) break;  // block-uniform
      int k = int(kp);
      if (J.kind == SEL_PACK_FWD_STRIDED) k = strided_k(int(kp), int(ph), int(s));
      else if (J.kind == SEL_PACK_CONVT) k = int(kp == 0 ? ph + s : ph);
      ok[kp] = in && k >= 0;
      v[kp] = J.w[ok[kp] ? base + unsigned(k) : 0];
    }
#pragma unroll
    for (unsigned kp = 0; kp < PT_KMAX; ++kp) {
      if (kp >= KP) break;
      tile[(nl * KP + kp) * PT_P + cl] = ok[kp] ? v[kp] : 0.f;
    }
  }
  __syncthreads();
  TO* const wp = static_cast<TO*>(J.wpack);
  for (unsigned r = threadIdx.x; r < PT_T * PT_T; r += PT_THREADS) {  // Wp[n][kp][cp]: cp fastest
    const unsigned cl = r % PT_T, nl = r / PT_T;
    const unsigned n = n0 + nl, cp = c0 + cl;
    if (n < N && cp < CP)
      for (unsigned kp = 0; kp < KP; ++kp) wp[(n * KP + kp) * CP + cp] = from_f<TO>(tile[(nl * KP + kp) * PT_P + cl]);
  }
  if (J.wdgrad) {
    TO* const wd = static_cast<TO*>(J.wdgrad);
    for (unsigned r = threadIdx.x; r < PT_T * PT_T; r += PT_THREADS) {  // Wd[cp][j][n]: n fastest
      const unsigned nl = r % PT_T, cl = r / PT_T;
      const unsigned n = n0 + nl, cp = c0 + cl;
      if (n < N && cp < CP)
        for (unsigned j = 0; j < KP; ++j)
          wd[(cp * KP + j) * N + n] = from_f<TO>(tile[(nl * KP + (KP - 1 - j)) * PT_P + cl]);
    }
  }
}


__global__ void k_unpack(int kind, const float* __restrict__ gp, int cout, int cin, int K, int s,
                         float* __restrict__ gw) {
  // iterate over torch-layout elements
  int64_t total = (kind == SEL_PACK_CONVT) ? int64_t(cin) * cout * 2 * s
                                           : int64_t(cout) * cin * (kind == SEL_PACK_FWD ? K : 2 * s);
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += int64_t(gridDim.x) * blockDim.x) {
    float v;
    if (kind == SEL_PACK_FWD) {
      const int k = int(i % K);
      const int ci = int((i / K) % cin);
      const int co = int(i / (int64_t(K) * cin));
      v = gp[(int64_t(co) * K + k) * cin + ci];
    } else if (kind == SEL_PACK_FWD_STRIDED) {
      const int KK = 2 * s;
      const int k = int(i % KK);
      const int ci = int((i / KK) % cin);
      const int co = int(i / (int64_t(KK) * cin));
      int tap, ph;
      if (k <= s - 2) { tap = 0; ph = k + 1; }
      else if (k <= 2 * s - 2) { tap = 1; ph = k - s + 1; }
      else { tap = 2; ph = 0; }
      v = gp[(int64_t(co) * 3 + tap) * (int64_t(s) * cin) + ph * cin + ci];
    } else {
      const int KK = 2 * s;
      const int k = int(i % KK);
      const int co = int((i / KK) % cout);
      const int ci = int(i / (int64_t(KK) * cout));
      const int ph = k < s ? k : k - s;
      const int tap = k < s ? 1 : 0;
      v = gp[(int64_t(ph * cout + co) * 2 + tap) * cin + ci];
    }
    gw[i] = v;
  }
}

// adjoint of the replicate pad: gin[b*T, c] += sum_n gout[b*T, n] * Wp[n][0][c]
// block = (sample b, 64 channels); 16 waves split n, LDS reduce.
template <typename T>
__global__ __launch_bounds__(1024) void k_replicate_fix(Args a, const T* __restrict__ gout, const T* __restrict__ wp,
                                                        T* __restrict__ gin) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = int64_t(blockIdx.x) * a.T;
  const int c = blockIdx.y * 64 + lane;
  float s = 0.f;
  if (c < a.C) {
    // 8 (gout, weight) pairs in flight per step, summed in the same n order
    int n = wave;
    for (; n + 16 * 7 < a.N; n += 16 * 8) {
      float gv[8], wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        gv[u] = to_f(gout[row * a.N + n + 16 * u]);
        wv[u] = to_f(wp[(int64_t(n + 16 * u) * a.K + 0) * a.C + c]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += gv[u] * wv[u];
    }
    for (; n < a.N; n += 16) s += to_f(gout[row * a.N + n]) * to_f(wp[(int64_t(n) * a.K + 0) * a.C + c]);
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < a.C) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w][lane];
    gin[row * a.C + c] = from_f<T>(to_f(gin[row * a.C + c]) + t);
  }
}

template <typename TS, typename TD>
__global__ void k_cast(const TS* __restrict__ s, TD* __restrict__ d, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * blockDim.x)
    d[i] = from_f<TD>(to_f(s[i]));
}


}  // namespace conv
}  // namespace sel

using namespace sel;
using namespace sel::conv;

extern "C" {

int sel_pack_weight(int kind, const float* w, int cout, int cin, int k, int stride, int dtype, void* wpack,

                    sel_stream_t stream) {
  SEL_REQUIRE(kind >= SEL_PACK_FWD && kind <= SEL_PACK_CONVT, SEL_ERR_ARG, "bad pack kind");
  SEL_REQUIRE(kind == SEL_PACK_FWD || k == 2 * stride, SEL_ERR_UNSUPPORTED,
              "strided/transposed conv needs kernel_size == 2*stride (got %d, %d)", k, stride);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = kind == SEL_PACK_FWD ? int64_t(cout) * k * cin
                        : kind == SEL_PACK_FWD_STRIDED ? int64_t(cout) * 3 * stride * cin
                                                       : int64_t(stride) * cout * 2 * cin;
  dim3 grid(unsigned(std::min<int64_t>(4096, (total + 255) / 256)));
  if (dtype == SEL_F32)
    hipLaunchKernelGGL(k_pack<float>, grid, dim3(256), 0, s, kind, w, cout, cin, k, stride,
                       static_cast<float*>(wpack));
  else
    hipLaunchKernelGGL(k_pack<__bf16>, grid, dim3(256), 0, s, kind, w, cout, cin, k, stride,
                       static_cast<__bf16*>(wpack));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_pack_many(const sel_pack_job* jobs, int njobs, int64_t total, int dtype, sel_stream_t stream) {
  SEL_REQUIRE(jobs && njobs > 0 && total > 0, SEL_ERR_ARG, "empty pack job table");
  // (the job table is device memory: each job's element count is checked < 2^31
  // by the host binding, sel/convops.py PackCache._refresh)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(unsigned(std::min<int64_t>(8192, (2 * total + 255) / 256)));
  if (dtype == SEL_F32)
    hipLaunchKernelGGL(k_pack_many<float>, grid, dim3(256), 0, s, jobs, njobs, total);
  else
    hipLaunchKernelGGL(k_pack_many<__bf16>, grid, dim3(256), 0, s, jobs, njobs, total);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_pack_many_host(const sel_pack_job* jobs, int njobs, int64_t total, int dtype, sel_stream_t stream) {
  using namespace sel::conv;
  SEL_REQUIRE(jobs && njobs > 0 && total > 0, SEL_ERR_ARG, "empty pack job table");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += PM_MAXJ) {
    PackJobs pj{};
    pj.n = std::min(PM_MAXJ, njobs - j0);
    for (int j = 0; j < pj.n; ++j) {
      pj.j[j] = jobs[j0 + j];
      SEL_REQUIRE(pj.j[j].offset >= 0 && pj.j[j].offset < total && (j == 0 || pj.j[j].offset > pj.j[j - 1].offset),
                  SEL_ERR_ARG, "pack jobs must have increasing offsets within total");
    }
    // tiled kernel (k_pack_tiles) unless a job's taps exceed its tile (K > 8)
    // or tune key 60 = 1 asks for the per-element form
    PackTiles pt{};
    bool tiled = tune(60) != 1;
    int64_t tiles = 0;
    pt.n = pj.n;
    for (int j = 0; j < pj.n && tiled; ++j) {
      const sel_pack_job& J = pj.j[j];
      const int64_t N = J.kind == SEL_PACK_CONVT ? int64_t(J.stride) * J.cout : J.cout;
      const int64_t KP = J.kind == SEL_PACK_FWD ? J.k : J.kind == SEL_PACK_FWD_STRIDED ? 3 : 2;
      const int64_t CP = J.kind == SEL_PACK_FWD_STRIDED ? int64_t(J.stride) * J.cin : J.cin;
      if (KP > PT_KMAX) tiled = false;
      pt.j[j] = J;
      pt.tstart[j] = int(tiles);
      tiles += ((N + PT_T - 1) / PT_T) * ((CP + PT_T - 1) / PT_T);
    }
    pt.tstart[pt.n] = int(tiles);
    if (tiled && tiles > 0 && tiles < (int64_t(1) << 31)) {
      if (dtype == SEL_F32)
        hipLaunchKernelGGL((k_pack_tiles<float, 1024>), dim3(unsigned(tiles)), dim3(1024), 0, s, pt);
      else
        hipLaunchKernelGGL((k_pack_tiles<__bf16, 1024>), dim3(unsigned(tiles)), dim3(1024), 0, s, pt);
      SEL_LAUNCH_CHECK();
      continue;
    }
    const int64_t lo = pj.j[0].offset;
    const int64_t hi = j0 + pj.n < njobs ? jobs[j0 + pj.n].offset : total;
    dim3 grid(unsigned(std::min<int64_t>(8192, (2 * (hi - lo) + 255) / 256)));
    if (dtype == SEL_F32)
      hipLaunchKernelGGL(k_pack_many_arg<float>, grid, dim3(256), 0, s, pj, lo, hi, total);
    else
      hipLaunchKernelGGL(k_pack_many_arg<__bf16>, grid, dim3(256), 0, s, pj, lo, hi, total);
    SEL_LAUNCH_CHECK();
  }
  return SEL_OK;
}

int sel_pack_dgrad(const void* wpack, int N, int K, int C, int dtype, void* wd, sel_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = int64_t(N) * K * C;
  dim3 grid(unsigned(std::min<int64_t>(4096, (total + 255) / 256)));
  if (dtype == SEL_F32)
    hipLaunchKernelGGL(k_pack_dgrad<float>, grid, dim3(256), 0, s, static_cast<const float*>(wpack), N, K, C,
                       static_cast<float*>(wd));
  else
    hipLaunchKernelGGL(k_pack_dgrad<__bf16>, grid, dim3(256), 0, s, static_cast<const __bf16*>(wpack), N, K,
                       C, static_cast<__bf16*>(wd));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_unpack_wgrad(int kind, const float* gwpack, int cout, int cin, int k, int stride, float* gw,
                     sel_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = int64_t(cout) * cin * (kind == SEL_PACK_FWD ? k : 2 * stride);
  dim3 grid(unsigned(std::min<int64_t>(4096, (total + 255) / 256)));
  hipLaunchKernelGGL(k_unpack, grid, dim3(256), 0, s, kind, gwpack, cout, cin, k, stride, gw);
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_conv_replicate_fix(const sel_conv_desc* d, int dtype, const void* gout, const void* wpack, void* gin,
                           sel_stream_t stream) {
  if (int rc = check_desc(d)) return rc;
  const Args a = to_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = unsigned(d->rows / d->T);
  if (nb == 0) return SEL_OK;
  const dim3 grid(nb, unsigned((d->C + 63) / 64));
  if (dtype == SEL_F32)
    hipLaunchKernelGGL(k_replicate_fix<float>, grid, dim3(1024), 0, s, a, static_cast<const float*>(gout),
                       static_cast<const float*>(wpack), static_cast<float*>(gin));
  else
    hipLaunchKernelGGL(k_replicate_fix<__bf16>, grid, dim3(1024), 0, s, a, static_cast<const __bf16*>(gout),
                       static_cast<const __bf16*>(wpack), static_cast<__bf16*>(gin));
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

int sel_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, sel_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n <= 0) return SEL_OK;
  dim3 grid(unsigned(std::min<int64_t>(8192, (n + 255) / 256)));
  if (src_dtype == SEL_F32 && dst_dtype == SEL_BF16)
    hipLaunchKernelGGL((k_cast<float, __bf16>), grid, dim3(256), 0, s, static_cast<const float*>(src),
                       static_cast<__bf16*>(dst), n);
  else if (src_dtype == SEL_BF16 && dst_dtype == SEL_F32)
    hipLaunchKernelGGL((k_cast<__bf16, float>), grid, dim3(256), 0, s, static_cast<const __bf16*>(src),
                       static_cast<float*>(dst), n);
  else {
    set_error("unsupported cast %d -> %d", src_dtype, dst_dtype);
    return SEL_ERR_UNSUPPORTED;
  }
  SEL_LAUNCH_CHECK();
  return SEL_OK;
}

}  // extern "C"
