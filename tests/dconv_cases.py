"""Cases, fp64 references and bounds of the discriminator conv kernels
(csrc/dconv.hip and its hand-off to conv.hip's warp-specialised kernels,
csrc/dconv_wgrad.hip, csrc/dconv_pack.hip),
shared by tests/test_gpu_dconv_edges.py and tests/test_dconv_cases_host.py, and
the bf16 checker tests/test_gpu_gan.py and tests/test_gpu_dconv_variants.py use.
Nothing here needs a GPU: the library's dispatch reporters run on the host.

What lives here:
  * CASES: (cin, cout, Kt, stride, pad, groups, Bs, T) layers, each the smallest
    shape that reaches one kernel or one branch of plan_fwd / wg_plan, with the
    kernel names it must reach (bf16 forward / adjoint, fp32 forward / adjoint,
    weight gradient in both dtypes) written out, so that a dispatch change
    cannot move a case onto another kernel unnoticed;
  * VARIANTS: the same layers with a widened descriptor: input gap rows
    [Tv, Tvs) holding finite garbage ("gap"), output rows [Tvalid, Tvo)
    prefilled ("zrows"), row pitches 8 wider than the used columns ("pitch");
  * operands / reference: the buffers of a case in the descriptor's layout and
    the fp64 torch conv1d of the layer on the same rounded operands, its
    autograd for the adjoint and the weight / bias gradients, and the sums of
    absolute products the fp32 bounds scale with;
  * wg_plan: the weight-gradient plan of dconv_wgrad.hip restated;
  * pack_ref / prim_ref: the pack order and the primitive's formula
    (include/sel.h) restated index by index, for the host test that ties the
    layer view to the descriptor view.

Bounds.  u = 2^-24, eps = 2 u = 2^-23 (fp32), bf16 has 8 significant bits.

bf16 forward / adjoint: operands are the same bf16 values in kernel and
reference, products of two bf16 values are exact in fp32, the sums run in
fp32 (relative error ~1e-6, invisible here), and the output is rounded to bf16
once: relative error <= 2^-9 = 1.95e-3 per element where nothing cancels.  The
project's bound for that situation (tests/test_gpu_c3.py _check) is
    ||a - b|| <= 4e-3 ||b||   and   |a - b| <= 8e-3 |b| + 2e-3 max|b|  per element;
8e-3 is 2 bf16 ulps (2^-7 at the top of a binade), the absolute term covers
the elements that are small by cancellation (and a LeakyReLU side picked the
other way for a pre-activation within rounding of zero: both sides are then
within rounding of zero, far below 2e-3 max|b|).

fp32 forward / adjoint: 1e-5 norm-wise (the project's figure), and per element
    |a - b| <= (n + 4) eps S,   S = sum |w| |x| (+ |bias| + |res|),
n = K S Cg products.  Any order of summing n + 2 terms in fp32 is within
(n + 1) u S(1 + O(u)) of the exact sum (fma products add no rounding); the
LeakyReLU' / LeakyReLU multiplies add one rounding each; eps = 2u leaves a
factor 2.  S is computed by the reference from the same operands in fp64.  The
addends of the epilogue are terms of the same sum, so they are counted in S.

Weight / bias gradients (fp32 sums over n = Bs * T_out rows of exact products,
in nsplit partials that are summed afterwards): per element
    |a - b| <= (n + nsplit + 2) eps sum |g| |x|
for any summation order, and norm-wise 1e-5 for layers of at most 4096 rows
(the project's figure for fp32 sums of exact products: tests/test_gpu_conv.py,
tests/test_gpu_hfg_bwd_kernels.py).  For longer sums the norm-wise limit is
4 x the error of a plain fp32 torch evaluation of the same sum on the same
operands (measured in the same test against the same fp64 reference), capped
at 1e-4 (the older dconv bound).
"""
import math

import torch
import torch.nn.functional as F

from sel import dconvops as DC

EPS32 = 2.0 ** -23
SLOPE = 0.1
BF16, F32 = torch.bfloat16, torch.float32
GAP_FILL = 1.0e3       # finite garbage in input gap rows and pad columns
OUT_FILL = 7.0         # prefill of the output buffers
WG_NORM_ROWS = 4096    # rows up to which the weight gradient is held to 1e-5 norm-wise

# the constants of dconv_wgrad.hip / sel_common.h, restated
W3_BM, WG_BM, WG_TAPS, PRESUM = 128, 64, 8, 16
WG_CAP = 64 << 20
RU_OOB = 0x7FFFFFF0


def _names(fb, ab, ff, af, wb, wf):
    return dict(fwd_bf16=fb, adj_bf16=ab, fwd_f32=ff, adj_f32=af, wg_bf16=wb, wg_f32=wf)


class Case:
    """One layer: torch Conv1d(cin, cout, Kt, stride, padding=pad, groups) on Bs
    sequences of T samples.  layout "plain": input rows rounded up to the
    stride, outputs T_out rows; "period": the MPD chain's zero-gapped layout
    (output pitch P = T_out + 2, input pitch P * stride)."""

    def __init__(self, name, shape, names, layout="plain", variant=None):
        self.name, self.shape, self.names, self.layout, self.variant = name, shape, names, layout, variant
        self.cin, self.cout, self.Kt, self.stride, self.pad, self.groups, self.Bs, self.T = shape

    @property
    def spec(self):
        return DC.LayerSpec(self.cin, self.cout, self.Kt, self.stride, self.pad, self.groups, True)

    def descs(self):
        """(forward descriptor, adjoint descriptor), widened by the variant."""
        sp, s = self.spec, self.stride
        T_out = sp.t_out(self.T)
        if self.layout == "period":
            To_alloc = T_out + 2
            Ta = To_alloc * s
        else:
            To_alloc, Ta = T_out, DC._roundup(self.T, s)
        df = DC._fwd_desc(sp, self.Bs, self.T, Ta, T_out, To_alloc, SLOPE)
        da = DC._dgrad_desc(sp, self.Bs, Ta, T_out, To_alloc, SLOPE, False, T_in=self.T)
        for d in (df, da):
            if self.variant == "gap":
                d.Tvs = d.Tv + 3
            elif self.variant == "zrows":
                d.Tvo = d.Tvalid + 3
            elif self.variant == "pitch":
                d.ldx += 8
                d.ldo += 8
        return df, da


_W3_SHAPES = [(32, 32, 1), (32, 32, 3), (32, 32, 5),
              (64, 32, 2), (64, 32, 3), (64, 32, 5), (64, 32, 7),
              (32, 64, 1), (32, 64, 3), (32, 64, 5), (32, 64, 8),
              (64, 64, 1), (64, 64, 2), (64, 64, 3), (64, 64, 4), (64, 64, 5), (64, 64, 7)]

# name -> (shape, layout, kernel names); names filled in below (_EXPECT)
_SHAPES = {
    "gpf256x32": ((128, 128, 41, 1, 20, 16, 2, 4100), "plain"),
    "gpf256x64": ((256, 256, 41, 2, 20, 4, 2, 16400), "plain"),
    "g_narrow": ((48, 48, 41, 4, 20, 6, 3, 301), "plain"),
    "k9": ((32, 64, 9, 1, 4, 1, 3, 301), "plain"),
    "k64": ((16, 32, 64, 1, 32, 1, 2, 200), "plain"),
    "k65": ((16, 32, 65, 1, 32, 1, 2, 200), "plain"),
    "t_lt_k": ((128, 128, 41, 4, 20, 4, 2, 24), "plain"),
    "pf128x128": ((64, 128, 4, 1, 2, 1, 8, 8192), "plain"),
    "pf128x64": ((64, 64, 5, 1, 2, 1, 8, 8200), "plain"),
    "pf_ragged": ((40, 72, 5, 3, 2, 1, 3, 301), "plain"),
    "ws3": ((64, 128, 3, 1, 1, 1, 16, 4100), "plain"),
    "ws7": ((64, 128, 7, 1, 3, 1, 16, 4100), "plain"),
    "ws_flat5": ((1024, 1024, 5, 1, 2, 1, 150, 54), "period"),
    "ws_flat2": ((512, 1024, 5, 3, 2, 1, 150, 162), "period"),
    "ws8_flat": ((128, 512, 5, 3, 2, 1, 300, 162), "period"),
    "tiny4": ((8, 4, 3, 1, 1, 1, 3, 301), "plain"),
    "tiny_adj2": ((1, 32, 4, 2, 1, 1, 3, 301), "plain"),
    "valu": ((12, 20, 5, 1, 2, 1, 3, 100), "plain"),
    "short15": ((1, 24, 15, 1, 7, 1, 2, 300), "plain"),
    "short6": ((2, 16, 3, 1, 1, 1, 2, 300), "plain"),
    "shortx6": ((1, 16, 6, 1, 3, 1, 2, 300), "plain"),
    "k1nr2": ((1, 16, 2, 2, 0, 1, 2, 300), "plain"),
    "k1nr3": ((1, 16, 3, 3, 0, 1, 2, 300), "plain"),
    "n1": ((1024, 1, 3, 1, 1, 1, 2, 48), "plain"),
    "wg_mfma1": ((16, 48, 9, 1, 4, 1, 3, 301), "plain"),
    "w3_strided": ((32, 64, 4, 2, 1, 1, 3, 301), "plain"),
    "w3_short_seq": ((64, 64, 5, 1, 2, 1, 7, 50), "plain"),
}
for _ci, _co, _k in _W3_SHAPES:
    _SHAPES[f"w3_{_ci}_{_co}_k{_k}"] = ((_ci, _co, _k, 1, _k // 2, 1, 3, 300), "plain")

VARIANT_BASES = ("g_narrow", "pf_ragged", "tiny4", "valu", "short15", "shortx6", "w3_64_64_k5")
VARIANTS = ("gap", "zrows", "pitch")

# the weight-gradient kernel of every w3 case, by the arithmetic of wg_plan
# (NT = 2 at 64 outputs, CT = 2 at 64 reduction channels, MAXT from CT * K)
_W3_OF = {(32, 32, 1): (1, 1, 1), (32, 32, 3): (1, 1, 1), (32, 32, 5): (1, 1, 2),
          (64, 32, 2): (1, 2, 1), (64, 32, 3): (1, 2, 2), (64, 32, 5): (1, 2, 3), (64, 32, 7): (1, 2, 4),
          (32, 64, 1): (2, 1, 1), (32, 64, 3): (2, 1, 2), (32, 64, 5): (2, 1, 3), (32, 64, 8): (2, 1, 4),
          (64, 64, 1): (2, 2, 1), (64, 64, 2): (2, 2, 2), (64, 64, 3): (2, 2, 3), (64, 64, 4): (2, 2, 4),
          (64, 64, 5): (2, 2, 5), (64, 64, 7): (2, 2, 8)}

# name (or name/variant where the variant moves a launch onto another kernel) ->
# (forward bf16, adjoint bf16, forward fp32, adjoint fp32, weight gradient bf16, weight gradient fp32)
_EXPECT = {
    "gpf256x32": ("k_dconv_gpf<256, 32>", "k_dconv_gpf<256, 32>",
                  "k_dconv_mfma<float, 256, 32>", "k_dconv_mfma<float, 256, 32>",
                  "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "gpf256x64": ("k_dconv_gpf<256, 64>", "k_dconv_gpf<256, 64>",
                  "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                  "k_dwgrad_mfma<2>", "k_dwgrad_valu<float>"),
    "g_narrow": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<128, 32>",
                 "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 128, 32>",
                 "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "k9": ("k_dconv_gpf<64, 64>", "k_dconv_gpf<128, 32>",
           "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
           "k_dwgrad_mfma<2>", "k_dwgrad_valu<float>"),
    "k64": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<128, 32>",
            "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 128, 32>",
            "k_dwgrad_mfma<2>", "k_dwgrad_valu<float>"),
    "k65": ("k_dconv_valu<bf16>", "k_dconv_valu<bf16>",
            "k_dconv_valu<float>", "k_dconv_valu<float>",
            "k_dwgrad_mfma<2>", "k_dwgrad_valu<float>"),
    "t_lt_k": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<64, 64>",
               "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 64, 64>",
               "k_dwgrad_mfma<2>", "k_dwgrad_valu<float>"),
    "pf128x128": ("k_dconv_pf<128, 128>", "k_dconv_pf<128, 64>",
                  "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                  "k_dwgrad_w3<2, 2, 4>", "k_dwgrad_valu<float>"),
    "pf128x64": ("k_dconv_pf<128, 64>", "k_dconv_pf<128, 64>",
                 "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                 "k_dwgrad_w3<2, 2, 5>", "k_dwgrad_valu<float>"),
    "pf_ragged": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                  "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                  "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "ws3": ("k_conv_ws_bf16<3>", "k_dconv_pf<128, 64>",
            "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
            "k_dwgrad_w3<2, 2, 3>", "k_dwgrad_valu<float>"),
    "ws7": ("k_conv_ws_bf16<7>", "k_dconv_pf<128, 64>",
            "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
            "k_dwgrad_w3<2, 2, 8>", "k_dwgrad_valu<float>"),
    "ws_flat5": ("k_conv_ws_bf16<5>", "k_conv_ws_bf16<5>",
                 "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                 "k_dwgrad_w3<2, 2, 5>", "k_dwgrad_valu<float>"),
    "ws_flat2": ("k_conv_ws_bf16<2>", "k_conv_ws_bf16<2>",
                 "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                 "k_dwgrad_w3<2, 2, 2>", "k_dwgrad_valu<float>"),
    "ws8_flat": ("k_conv_ws8<2, bf16, 256, 256>", "k_dconv_pf<128, 64>",
                 "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 64>",
                 "k_dwgrad_w3<2, 2, 2>", "k_dwgrad_valu<float>"),
    "tiny4": ("k_dconv_tiny<4>", "k_dconv_valu<bf16>",
              "k_dconv_valu<float>", "k_dconv_valu<float>",
              "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "tiny_adj2": ("k_dconv_short<bf16, 6>", "k_dconv_tiny<4>",
                  "k_dconv_short<float, 6>", "k_dconv_valu<float>",
                  "k_dwgrad_short<bf16, 6>", "k_dwgrad_short<float, 6>"),
    "valu": ("k_dconv_valu<bf16>", "k_dconv_valu<bf16>",
             "k_dconv_valu<float>", "k_dconv_valu<float>",
             "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "short15": ("k_dconv_short<bf16, 15>", "k_dconv_gpf<128, 32>",
                "k_dconv_short<float, 15>", "k_dconv_mfma<float, 128, 32>",
                "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "short6": ("k_dconv_short<bf16, 6>", "k_dconv_tiny<4>",
               "k_dconv_short<float, 6>", "k_dconv_valu<float>",
               "k_dwgrad_short<bf16, 6>", "k_dwgrad_short<float, 6>"),
    "shortx6": ("k_dconv_shortx<bf16, 6, 1>", "k_dconv_tiny<4>",
                "k_dconv_shortx<float, 6, 1>", "k_dconv_valu<float>",
                "k_dwgrad_shortx<bf16, 6, 1>", "k_dwgrad_shortx<float, 6, 1>"),
    "shortx6/pitch": ("k_dconv_short<bf16, 6>", "k_dconv_tiny<4>",
                      "k_dconv_short<float, 6>", "k_dconv_valu<float>",
                      "k_dwgrad_short<bf16, 6>", "k_dwgrad_short<float, 6>"),
    "k1nr2": ("k_dconv_shortx<bf16, 1, 2>", "k_dconv_tiny<4>",
              "k_dconv_shortx<float, 1, 2>", "k_dconv_valu<float>",
              "k_dwgrad_shortx<bf16, 1, 2>", "k_dwgrad_shortx<float, 1, 2>"),
    "k1nr3": ("k_dconv_shortx<bf16, 1, 3>", "k_dconv_tiny<4>",
              "k_dconv_shortx<float, 1, 3>", "k_dconv_valu<float>",
              "k_dwgrad_shortx<bf16, 1, 3>", "k_dwgrad_shortx<float, 1, 3>"),
    "n1": ("k_dconv_gpf<128, 32>", "k_dconv_shortx<bf16, 3, 1>",
           "k_dconv_mfma<float, 128, 32>", "k_dconv_shortx<float, 3, 1>",
           "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>"),
    "wg_mfma1": ("k_dconv_gpf<64, 64>", "k_dconv_gpf<128, 32>",
                 "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
                 "k_dwgrad_mfma<1>", "k_dwgrad_valu<float>"),
    "w3_strided": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                   "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                   "k_dwgrad_w3<2, 2, 3>", "k_dwgrad_valu<float>"),
    "w3_short_seq": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                     "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                     "k_dwgrad_w3<2, 2, 5>", "k_dwgrad_valu<float>"),
    "w3_32_32_k1": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<1, 1, 1>", "k_dwgrad_valu<float>"),
    "w3_32_32_k3": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<1, 1, 1>", "k_dwgrad_valu<float>"),
    "w3_32_32_k5": ("k_dconv_gpf<128, 32>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<1, 1, 2>", "k_dwgrad_valu<float>"),
    "w3_64_32_k2": ("k_dconv_gpf<128, 32>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<1, 2, 1>", "k_dwgrad_valu<float>"),
    "w3_64_32_k3": ("k_dconv_gpf<128, 32>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<1, 2, 2>", "k_dwgrad_valu<float>"),
    "w3_64_32_k5": ("k_dconv_gpf<128, 32>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<1, 2, 3>", "k_dwgrad_valu<float>"),
    "w3_64_32_k7": ("k_dconv_gpf<128, 32>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 128, 32>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<1, 2, 4>", "k_dwgrad_valu<float>"),
    "w3_32_64_k1": ("k_dconv_pf<64, 64>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<2, 1, 1>", "k_dwgrad_valu<float>"),
    "w3_32_64_k3": ("k_dconv_pf<64, 64>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<2, 1, 2>", "k_dwgrad_valu<float>"),
    "w3_32_64_k5": ("k_dconv_pf<64, 64>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<2, 1, 3>", "k_dwgrad_valu<float>"),
    "w3_32_64_k8": ("k_dconv_pf<64, 64>", "k_dconv_gpf<128, 32>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 128, 32>",
                    "k_dwgrad_w3<2, 1, 4>", "k_dwgrad_valu<float>"),
    "w3_64_64_k1": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 1>", "k_dwgrad_valu<float>"),
    "w3_64_64_k2": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 2>", "k_dwgrad_valu<float>"),
    "w3_64_64_k3": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 3>", "k_dwgrad_valu<float>"),
    "w3_64_64_k4": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 4>", "k_dwgrad_valu<float>"),
    "w3_64_64_k5": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 5>", "k_dwgrad_valu<float>"),
    "w3_64_64_k7": ("k_dconv_pf<64, 64>", "k_dconv_pf<64, 64>",
                    "k_dconv_mfma<float, 64, 64>", "k_dconv_mfma<float, 64, 64>",
                    "k_dwgrad_w3<2, 2, 8>", "k_dwgrad_valu<float>"),
}


def names_of(case):
    """The kernel names the library reports for a case (host only)."""
    df, da = case.descs()
    out = {}
    for dt, key in ((BF16, "bf16"), (F32, "f32")):
        out["fwd_" + key] = DC.kernel(df, dt)[1]
        out["adj_" + key] = DC.kernel(da, dt)[1]
        out["wg_" + key] = DC.wgrad_kernel(df, dt)[0]
    return out


def _make_cases():
    out = []
    for name, (shape, layout) in _SHAPES.items():
        for v in (None,) + (VARIANTS if name in VARIANT_BASES else ()):
            key = name if v is None else f"{name}/{v}"
            out.append(Case(key, shape, _names(*_EXPECT.get(key, _EXPECT[name])), layout, v))
    return out


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------
# operands in the descriptors' layouts, fp64 references
# ---------------------------------------------------------------------------
def zeros_in(t, every=7):
    """Exact zeros planted in an aux operand (LeakyReLU'(0) = slope)."""
    t.view(-1)[::every] = 0
    return t


def _filled(shape, dtype, dev, rows_valid, cols_valid, fill):
    """(B, rows, pitch) buffer: `fill` everywhere outside [:, :rows_valid, :cols_valid]."""
    buf = torch.full(shape, fill, dtype=dtype, device=dev)
    buf[:, :rows_valid, :cols_valid] = 0
    return buf


class Operands:
    """Buffers of a case in dtype `dt` on `dev`, laid out as its descriptors say.
    x: forward input (phase view); g_adj: the adjoint's input; g_wg: the same
    gradient in the forward output's layout (rows [T_out, Tvo) and the pad
    columns hold garbage: the weight gradient may not read them); aux / res:
    the adjoint's epilogue operands in its output layout."""

    def __init__(self, case, dt, dev, seed=0):
        sp, s = case.spec, case.stride
        df, da = case.descs()
        self.case, self.dt, self.df, self.da, self.sp = case, dt, df, da, sp
        gen = torch.Generator(device=dev).manual_seed(1000 * seed + 7 * case.Kt + case.cin + 3 * case.cout)
        rn = lambda *sh: torch.randn(*sh, generator=gen, device=dev)  # noqa: E731
        Bs, T, cin, cout = case.Bs, case.T, case.cin, case.cout
        self.T_out = T_out = sp.t_out(T)
        garbage_rows = GAP_FILL if case.variant == "gap" else 0.0
        # forward input: T samples, zero up to Tv * s, then the gap rows
        self.xv = rn(Bs, T, cin).to(dt)
        tmp = torch.zeros(Bs, df.Tv * s, cin, dtype=dt, device=dev)
        tmp[:, :T] = self.xv
        self.x = torch.full((Bs, df.Tvs, df.ldx), GAP_FILL, dtype=dt, device=dev)
        self.x[:, df.Tv:, :s * cin] = garbage_rows
        self.x[:, :df.Tv, :s * cin] = tmp.view(Bs, df.Tv, s * cin)
        fan = (cin // case.groups) * case.Kt
        self.w = rn(cout, cin // case.groups, case.Kt) / fan ** 0.5
        self.wq = self.w.to(dt)
        self.b = rn(cout)
        self.gv = rn(Bs, T_out, cout).to(dt)
        self.g_adj = torch.full((Bs, da.Tvs, da.ldx), GAP_FILL, dtype=dt, device=dev)
        self.g_adj[:, da.Tv:, :cout] = garbage_rows
        self.g_adj[:, :T_out, :cout] = self.gv
        self.g_wg = torch.full((Bs, df.Tvo, df.ldo), GAP_FILL, dtype=dt, device=dev)
        self.g_wg[:, :T_out, :cout] = self.gv
        self.aux = zeros_in(rn(Bs, da.Tvo, da.ldo).to(dt))
        self.res = rn(Bs, da.Tvo, da.ldo).to(dt)

    def out_fwd(self):
        return torch.full((self.case.Bs, self.df.Tvo, self.df.ldo), OUT_FILL, dtype=self.dt, device=self.x.device)

    def out_adj(self):
        return torch.full((self.case.Bs, self.da.Tvo, self.da.ldo), OUT_FILL, dtype=self.dt, device=self.x.device)


def _conv_pass(case, x, w, b, g, rows):
    """conv1d of (Bs, rows, cin) fp64 `x` cut to T_out rows, and its autograd on
    cotangent g: (pre-activation, d/dx over all `rows`, d/dw, d/db)."""
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    pre = F.conv1d(xr.permute(0, 2, 1), wr, br, stride=case.stride, padding=case.pad, groups=case.groups)
    pre = pre[:, :, :g.shape[1]].permute(0, 2, 1)
    pre.backward(g)
    return pre.detach().contiguous(), xr.grad, wr.grad, br.grad


def reference(op, dtype=torch.float64, with_abs=True):
    """fp64 layer reference of an Operands (or, with dtype = float32, the plain
    fp32 torch evaluation of the same sums).  Returns a dict:
      y (Bs, T_out, cout) after bias + LeakyReLU; gin, gin_epi (Bs, Tvalid_adj,
      s * cin) in the adjoint's phase view, plain and with (+ res) * LeakyReLU'(aux);
      gw, gb; and, with_abs, the sums of absolute terms S_y, S_gin, S_gin_epi,
      S_gw, S_gb the fp32 bounds scale with."""
    case, da, s = op.case, op.da, op.case.stride
    Bs, cin = case.Bs, case.cin
    rows = da.Tvalid * s
    x = torch.zeros(Bs, rows, cin, dtype=dtype, device=op.xv.device)
    x[:, :case.T] = op.xv.to(dtype)
    w, b, g = op.wq.to(dtype), op.b.to(dtype), op.gv.to(dtype)
    pre, gin, gw, gb = _conv_pass(case, x, w, b, g, rows)
    gin = gin.reshape(Bs, da.Tvalid, s * cin)
    aux = op.aux[:, :da.Tvalid, :s * cin].to(dtype)
    res = op.res[:, :da.Tvalid, :s * cin].to(dtype)
    lg = torch.where(aux > 0, 1.0, SLOPE).to(dtype)
    r = dict(y=F.leaky_relu(pre, SLOPE), gin=gin, gin_epi=(gin + res) * lg, gw=gw, gb=gb)
    if with_abs:
        pa, ga, wa, ba = _conv_pass(case, x.abs(), w.abs(), b.abs(), g.abs(), rows)
        ga = ga.reshape(Bs, da.Tvalid, s * cin)
        r.update(S_y=pa, S_gin=ga, S_gin_epi=ga + res.abs(), S_gw=wa, S_gb=ba)
    return r


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def check_bf16(got, ref, what):
    """The project's bound for one bf16-rounded output of fp32 sums of exact
    products (module docstring); returns (norm-wise error, worst element / allowed)."""
    g, ref = got.double(), ref.double()
    e = _rel(g, ref)
    allowed = 8e-3 * ref.abs() + 2e-3 * ref.abs().max()
    worst = ((g - ref).abs() / allowed).max().item()
    print(f"{what}: bf16 norm-wise {e:.3e} (<= 4e-3), worst element / allowed {worst:.3f}")
    assert e <= 4e-3, (what, e)
    assert worst <= 1.0, (what, worst, int(((g - ref).abs() > allowed).sum()))
    return e, worst


def check_f32(got, ref, S, n, what, norm=1e-5):
    """fp32 sums of n exact products: norm-wise `norm`, and (n + 4) eps S per element."""
    g = got.double()
    e = _rel(g, ref)
    allowed = (n + 4) * EPS32 * S
    diff = (g - ref).abs()
    worst = (diff / allowed.clamp_min(1e-300)).max().item()
    print(f"{what}: fp32 norm-wise {e:.3e} (<= {norm:.1e}), worst element / allowed {worst:.3f} (n = {n})")
    assert e <= norm, (what, e)
    assert bool((diff <= allowed).all()), (what, worst, int((diff > allowed).sum()))
    return e, worst


def check_wgrad(got, ref, S, n, nsplit, what, norm):
    """A weight / bias gradient: (n + nsplit + 2) eps S per element, `norm` norm-wise."""
    g = got.double()
    e = _rel(g, ref)
    allowed = (n + nsplit + 2) * EPS32 * S
    diff = (g - ref).abs()
    worst = (diff / allowed.clamp_min(1e-300)).max().item()
    print(f"{what}: norm-wise {e:.3e} (<= {norm:.3e}), worst element / allowed {worst:.4f} "
          f"(n = {n}, nsplit = {nsplit})")
    assert e <= norm, (what, e, norm)
    assert bool((diff <= allowed).all()), (what, worst, int((diff > allowed).sum()))
    return e, worst


def wgrad_norm_limit(rows, plain_fp32_err):
    """Norm-wise limit of a weight gradient over `rows` rows (module docstring)."""
    if rows <= WG_NORM_ROWS:
        return 1e-5
    return min(4.0 * plain_fp32_err, 1e-4)


# ---------------------------------------------------------------------------
# wg_plan of dconv_wgrad.hip, restated
# ---------------------------------------------------------------------------
_SHORT_KR = (2, 3, 6, 15)
_DWSX = ((15, 1), (2, 3), (3, 1), (2, 1), (6, 1), (1, 2), (1, 3))


def _cdiv(a, b):
    return -(-a // b)


def w3_instance(nt, ct, K):
    """(NT, CT, MAXT) of k_dwgrad_w3 for K taps, and its row groups RG."""
    P, WPN = ct * K, 4 // nt
    RG = 1 if P >= WPN else WPN // P
    WPP = WPN // RG
    need = _cdiv(P, WPP)
    return (nt, ct, need if need <= 5 else 8), RG


def w3_reachable():
    return {w3_instance(nt, ct, K)[0] for nt in (1, 2) for ct in (1, 2) for K in range(1, 9)}


def wg_plan(d, dt):
    """(kernel name, (nsplit, tiles or rows per split, bias splits, flat pitch))
    of the weight gradient of forward descriptor d at the default tune settings."""
    bf = dt == BF16
    t = "bf16" if bf else "float"
    width, nred = d.So * d.Ng, d.S * d.Cg
    rows = d.B * d.Tvalid
    nw = d.G * width * d.K * nred
    mfma = bf and d.Cg % 8 == 0 and d.Cs % 8 == 0 and d.ldx % 8 == 0 and nred % 8 == 0 and width % 16 == 0
    if not mfma and d.G == 1 and d.So == 1 and d.Ng <= 256 and 256 % d.Ng == 0 and d.K * nred in _SHORT_KR:
        want = max(1, min(2048, rows // 64))
        per = _cdiv(rows, want)
        nsplit = _cdiv(rows, per)
        staged = d.Cs == d.Cg and d.ldx == nred and d.Ng % 2 == 0 and d.ldo % 2 == 0 and d.B * d.Tvo < 2 ** 31 and \
            (d.K, nred) in _DWSX
        name = f"k_dwgrad_shortx<{t}, {d.K}, {nred}>" if staged else f"k_dwgrad_short<{t}, {d.K * nred}>"
        return name, (nsplit, per, nsplit, 0)
    bwant = max(1, min(256, rows // 256))
    bsplit = max(1, _cdiv(rows, max(1, _cdiv(rows, bwant))))
    w3 = mfma and d.G == 1 and d.So == 1 and (d.S == 1 or d.Cs == d.Cg) and d.K <= 8 and width % 32 == 0 and \
        nred % 32 == 0 and d.ldo % 8 == 0 and d.B * d.Tvo * d.ldo * 2 <= RU_OOB and d.B * d.Tvs * d.ldx * 2 <= RU_OOB
    if w3:
        inst, _rg = w3_instance(2 if width % 64 == 0 else 1, 2 if nred % 64 == 0 else 1, d.K)
        P = d.Tvo
        flat = P if (d.Tvs == P and P - d.Tv >= -d.q0 and P - d.Tvalid >= d.q0 + d.K - 1 and d.B * P < 2 ** 31) else 0
        ntiles = _cdiv(d.B * P, W3_BM) if flat else d.B * _cdiv(d.Tvalid, W3_BM)
        blocks = (width // (32 * inst[0])) * (nred // (32 * inst[1]))
        want = max(1, _cdiv(512, blocks))
        want = min(want, max(1, WG_CAP // (nw * 4)), max(1, ntiles))
        per = _cdiv(ntiles, want)
        nsplit = _cdiv(ntiles, per)
        return "k_dwgrad_w3<%d, %d, %d>" % inst, (nsplit, per, nsplit, flat)
    if mfma:
        nt = 2 if width % 32 == 0 else 1
        ntg = _cdiv(d.K, WG_TAPS)
        ntiles = d.B * _cdiv(d.Tvalid, WG_BM)
        blocks = d.G * _cdiv(width, 16 * nt) * _cdiv(nred, 32) * ntg
        want = max(1, _cdiv(1024, blocks))
        want = min(want, max(1, WG_CAP // (nw * 4)), max(1, ntiles))
        per = _cdiv(ntiles, want)
        return f"k_dwgrad_mfma<{nt}>", (_cdiv(ntiles, per), per, bsplit, 0)
    want = max(1, (1 << 20) // max(1, nw + d.G * width))
    want = min(want, max(1, WG_CAP // ((nw + width * d.G) * 4)), max(1, rows))
    per = _cdiv(rows, want)
    nsplit = _cdiv(rows, per)
    return f"k_dwgrad_valu<{t}>", (nsplit, per, nsplit, 0)


# ---------------------------------------------------------------------------
# the pack order and the primitive (include/sel.h), index by index
# ---------------------------------------------------------------------------
def pack_ref(w, sp, mode):
    """torch weight w[N][Cg][Kt] -> Wp[g][n][i][r][c] (mode 0) or Wd[g][(r, c)][K-1-i][n]
    (mode 1) as nested python lists flattened in that order (fp64)."""
    N, Cg, Kt = w.shape
    G, s, K, q0 = sp.groups, sp.stride, sp.K, sp.q0
    Ng = N // G
    Wp = torch.zeros(G, Ng, K, s, Cg, dtype=torch.float64)
    for g in range(G):
        for n in range(Ng):
            for i in range(K):
                for r in range(s):
                    k = s * (q0 + i) + r + sp.pad
                    if 0 <= k < Kt:
                        for c in range(Cg):
                            Wp[g, n, i, r, c] = float(w[g * Ng + n, c, k])
    if mode == 0:
        return Wp
    Wd = torch.zeros(G, s * Cg, K, Ng, dtype=torch.float64)
    for g in range(G):
        for n in range(Ng):
            for i in range(K):
                for r in range(s):
                    for c in range(Cg):
                        Wd[g, r * Cg + c, K - 1 - i, n] = Wp[g, n, i, r, c]
    return Wd


def prim_ref(d, x, Wp):
    """out[b, j, col(g, o)] = sum_{i < K, r < S, c < Cg} Wp[g][o][i][r][c] x[b, j + q0 + i, r Cs + g Cg + c],
    input rows outside [0, Tv) read as 0, col(g, o) = (o / Ng) Ns + g Ng + o % Ng; rows
    [Tvalid, Tvo) zero; columns no (g, o) maps to are left as they are (NaN here).
    x: (B, Tvs, ldx) fp64, Wp: (G, So * Ng, K, S, Cg)."""
    out = torch.full((d.B, d.Tvo, d.ldo), math.nan, dtype=torch.float64)
    for b in range(d.B):
        for j in range(d.Tvo):
            for g in range(d.G):
                for o in range(d.So * d.Ng):
                    col = (o // d.Ng) * d.Ns + g * d.Ng + o % d.Ng
                    acc = 0.0
                    if j < d.Tvalid:
                        for i in range(d.K):
                            t = j + d.q0 + i
                            if t < 0 or t >= d.Tv:
                                continue
                            for r in range(d.S):
                                for c in range(d.Cg):
                                    acc += float(Wp[g, o, i, r, c]) * float(x[b, t, r * d.Cs + g * d.Cg + c])
                    out[b, j, col] = acc
    return out
