// What more than one of the discriminator translation units (dconv.hip,
// dconv_wgrad.hip, dconv_pack.hip) uses; what a single file uses stays there.
#pragma once
#include "sel_common.h"

namespace sel {
namespace dconv {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return float(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __bf16 from_f<__bf16>(float v) { return __bf16(v); }

using D = sel_dconv_desc;

__device__ __forceinline__ int64_t in_col(const D& d, int g, int r, int c) {
  return int64_t(r) * d.Cs + int64_t(g) * d.Cg + c;
}
__device__ __forceinline__ int64_t out_col(const D& d, int g, int o) {
  const int ro = o / d.Ng, no = o - ro * d.Ng;
  return int64_t(ro) * d.Ns + int64_t(g) * d.Ng + no;
}

// Tap geometry of a torch weight [N][Cg][Kt] (stride s, padding pad, G groups)
// in the phase view: the packing (dconv_pack.hip) and the final weight-gradient
// reduction (dconv_wgrad.hip) index the packed forms by it.
struct PackGeo {
  int N, Cg, Kt, s, pad, G, K, q0;
};

__host__ __device__ inline PackGeo pack_geo(int N, int Cg, int Kt, int s, int pad, int G) {
  PackGeo p{N, Cg, Kt, s, pad, G, 0, 0};
  // q0 = floor(-pad / s), K = floor((Kt - 1 - pad) / s) - q0 + 1
  const int a = -pad;
  p.q0 = a >= 0 ? a / s : -((-a + s - 1) / s);
  const int e = Kt - 1 - pad;
  const int qe = e >= 0 ? e / s : -((-e + s - 1) / s);
  p.K = qe - p.q0 + 1;
  return p;
}

// (static: the library exports no symbol for the shared host functions)
static inline int check(const sel_dconv_desc* d) {
  SEL_REQUIRE(d != nullptr, SEL_ERR_ARG, "null dconv descriptor");
  SEL_REQUIRE(d->B > 0 && d->Tv >= 0 && d->Tvs >= d->Tv && d->Tvs > 0 && d->Tvo > 0 && d->Tvalid >= 0 && d->Tvalid <= d->Tvo && d->K > 0 &&
                  d->S > 0 && d->Cg > 0 && d->G > 0 && d->So > 0 && d->Ng > 0,
              SEL_ERR_ARG, "bad dconv shape B=%d Tv=%d Tvo=%d Tvalid=%d K=%d S=%d Cg=%d G=%d So=%d Ng=%d", d->B,
              d->Tv, d->Tvo, d->Tvalid, d->K, d->S, d->Cg, d->G, d->So, d->Ng);
  SEL_REQUIRE(int64_t(d->S - 1) * d->Cs + int64_t(d->G) * d->Cg <= d->ldx, SEL_ERR_ARG,
              "input columns exceed the row pitch ldx=%d", d->ldx);
  SEL_REQUIRE(int64_t(d->So - 1) * d->Ns + int64_t(d->G) * d->Ng <= d->ldo, SEL_ERR_ARG,
              "output columns exceed the row pitch ldo=%d", d->ldo);
  return SEL_OK;
}

// instantiated reductions: MSD first conv (15 taps), MPD first conv (2 taps x 3
// phases), the adjoints of the 1-channel output convs (3 / 2 taps)
static inline bool short_kr_ok(int kr) { return kr == 2 || kr == 3 || kr == 6 || kr == 15; }

// The (K, NR) instances of the staged short kernels, forward (k_dconv_shortx)
// and weight gradient (k_dwgrad_shortx): the one list both dispatches expand.
#define SEL_DSHORTX_TABLE(X) X(15, 1) X(2, 3) X(3, 1) X(2, 1) X(6, 1) X(1, 2) X(1, 3)

}  // namespace dconv
}  // namespace sel
