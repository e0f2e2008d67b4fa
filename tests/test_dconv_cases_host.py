"""CPU checks of the cases of tests/test_gpu_dconv_edges.py (tests/dconv_cases.py;
the library's dispatch reporters need no device): every case reaches exactly
the kernels its table entry names, the cases together reach every SEL_DPATH_*
family, every forward tile and every k_dwgrad_w3 / k_dwgrad_mfma instance, the
restated weight-gradient plan is the library's, the library's k_dwgrad_w3
table is the reachable set, the fp64 layer references equal an index-level
evaluation of the primitive's formula (include/sel.h) on weights in the
restated pack order, and the bound functions reject what they are there to
reject."""
import pytest
import torch

import dconv_cases as C
from sel import dconvops as DC

NAMES = [c.name for c in C.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_named_kernels(name):
    case = C.BY_NAME[name]
    assert C.names_of(case) == case.names
    df, da = case.descs()
    for dt in (C.BF16, C.F32):
        assert C.wg_plan(df, dt) == DC.wgrad_kernel(df, dt), (name, dt)
        assert DC.wgrad_kernel(df, dt)[0] == case.names["wg_bf16" if dt == C.BF16 else "wg_f32"]
    print(name, case.shape, case.names, DC.wgrad_kernel(df, C.BF16)[1])


def test_cases_reach_every_path_and_instance():
    paths, fwd, wg = set(), set(), set()
    for case in C.CASES:
        df, da = case.descs()
        for dt in (C.BF16, C.F32):
            for d in (df, da):
                p, n = DC.kernel(d, dt)
                paths.add(p)
                fwd.add(n)
            wg.add(DC.wgrad_kernel(df, dt)[0])
    assert paths == set(DC.PATH_NAMES.values()), set(DC.PATH_NAMES.values()) - paths
    want = {"k_dconv_gpf<256, 32>", "k_dconv_gpf<256, 64>", "k_dconv_gpf<128, 32>", "k_dconv_gpf<64, 64>",
            "k_dconv_mfma<float, 256, 32>", "k_dconv_mfma<float, 128, 64>", "k_dconv_mfma<float, 128, 32>",
            "k_dconv_mfma<float, 64, 64>", "k_dconv_pf<128, 128>", "k_dconv_pf<128, 64>", "k_dconv_pf<64, 64>",
            "k_dconv_short<bf16, 15>", "k_dconv_short<float, 15>", "k_dconv_short<bf16, 6>", "k_dconv_short<float, 6>",
            "k_dconv_shortx<bf16, 6, 1>", "k_dconv_shortx<bf16, 1, 2>", "k_dconv_shortx<bf16, 1, 3>",
            "k_dconv_shortx<float, 6, 1>", "k_dconv_shortx<float, 1, 2>", "k_dconv_shortx<float, 1, 3>",
            "k_dconv_shortx<bf16, 3, 1>", "k_dconv_valu<bf16>", "k_dconv_valu<float>", "k_dconv_tiny<4>",
            "k_conv_ws_bf16<2>", "k_conv_ws_bf16<3>", "k_conv_ws_bf16<5>", "k_conv_ws_bf16<7>",
            "k_conv_ws8<2, bf16, 256, 256>"}
    assert want <= fwd, want - fwd
    assert {"k_dwgrad_mfma<1>", "k_dwgrad_mfma<2>", "k_dwgrad_valu<bf16>", "k_dwgrad_valu<float>",
            "k_dwgrad_short<bf16, 6>", "k_dwgrad_short<float, 6>"} <= wg, wg
    for k, nr in ((6, 1), (1, 2), (1, 3)):
        assert {f"k_dwgrad_shortx<bf16, {k}, {nr}>", f"k_dwgrad_shortx<float, {k}, {nr}>"} <= wg
    assert {"k_dwgrad_w3<%d, %d, %d>" % i for i in C.w3_reachable()} <= wg
    # the tiny kernel at both widths, as forward (4 columns) and adjoint (2 output phases of 1 channel)
    d4, d2 = C.BY_NAME["tiny4"].descs()[0], C.BY_NAME["tiny_adj2"].descs()[1]
    assert DC.kernel(d4, C.BF16)[0] == "tiny" and d4.So * d4.Ng == 4
    assert DC.kernel(d2, C.BF16)[0] == "tiny" and (d2.So, d2.Ng) == (2, 1)
    # flat tiles (ws_flat, and k_dwgrad_w3's flat pitch) only where the layout has its gaps, or no tap crosses
    for n in ("ws_flat5", "ws_flat2", "ws8_flat"):
        d = C.BY_NAME[n].descs()[0]
        assert DC.kernel(d, C.BF16)[0] == "ws_flat" and DC.wgrad_kernel(d, C.BF16)[1][3] == d.Tvo == d.Tvalid + 2
    assert DC.kernel(C.BY_NAME["ws3"].descs()[0], C.BF16)[0] == "ws"


def test_w3_table_is_the_reachable_set():
    """(nt, ct) in {1, 2}^2 x K = 1..8 reach 16 instances; the library holds exactly those."""
    reach = C.w3_reachable()
    assert len(reach) == 16
    gone = {(1, 1, 3), (1, 1, 4), (1, 1, 5), (1, 2, 5), (2, 1, 5), (2, 1, 8)}
    assert not (gone & reach)
    tab = DC.w3_instances()
    assert len(tab) == len(set(tab)) and set(tab) == reach, set(tab) ^ reach
    # the row-group forms: fewer (tap, channel tile) pairs than waves of a column tile
    rg = {(nt, ct, K): C.w3_instance(nt, ct, K)[1] for nt in (1, 2) for ct in (1, 2) for K in range(1, 9)}
    assert {k for k, v in rg.items() if v == 4} == {(1, 1, 1)}
    assert {k for k, v in rg.items() if v == 2} == {(1, 1, 2), (1, 2, 1), (2, 1, 1)}
    for (ci, co, K), inst in (((32, 32, 1), (1, 1, 1)), ((64, 32, 2), (1, 2, 1)), ((32, 64, 1), (2, 1, 1))):
        assert C.BY_NAME[f"w3_{ci}_{co}_k{K}"].names["wg_bf16"] == "k_dwgrad_w3<%d, %d, %d>" % inst


def test_case_properties_by_hand():
    """What each case is named for, from the shape arithmetic."""
    def fa(n):
        return C.BY_NAME[n].descs()
    d, a = fa("gpf256x32")
    assert d.B * d.Tvo * d.G == 131200 > 131072 and d.So * d.Ng == 8
    d, a = fa("gpf256x64")
    assert a.So == 2 and DC.wgrad_kernel(d, C.BF16)[0] == "k_dwgrad_mfma<2>" and C._cdiv(d.K, C.WG_TAPS) == 3
    d, a = fa("g_narrow")
    assert d.Ng == 8 and a.So == 4 and a.G == 6 and d.K == 11 and d.K % 8 == 3 and d.S * d.Cg == 32
    assert fa("k9")[0].K == 9 and fa("k64")[0].K == 64 and fa("k65")[0].K == 65
    d, a = fa("t_lt_k")
    assert d.Tvalid == 6 < d.K
    d, a = fa("pf_ragged")
    assert d.S * d.Cg == 120 and 120 % 32 == 24 and d.Ng == 72 and 72 % 64 == 8 and d.S == 3 and C.BY_NAME[
        "pf_ragged"].T % 3 != 0
    d, a = fa("n1")
    assert d.So * d.Ng == 1 and d.K * d.S * d.Cg >= 256
    for ci, co, K in C._W3_SHAPES:
        d = fa(f"w3_{ci}_{co}_k{K}")[0]
        assert d.Tvalid in (300, 301) and d.Tvalid // C.W3_BM == 2 and d.Tvalid % C.W3_BM in (44, 45)
    d = fa("w3_strided")[0]
    assert d.S == 2 and d.Cs == d.Cg
    d = fa("w3_short_seq")[0]
    name, (nsplit, per, _b, flat) = DC.wgrad_kernel(d, C.BF16)
    assert d.Tvalid < C.W3_BM and d.B == 7 and flat == 0 and (nsplit, per) == (7, 1)   # seven one-tile splits
    d = fa("pf128x128")[0]
    name, (nsplit, per, _b, flat) = DC.wgrad_kernel(d, C.BF16)
    ntiles = d.B * C._cdiv(d.Tvalid, C.W3_BM)
    assert (nsplit - 1) * per < ntiles < nsplit * per                                 # the last split is short
    d = fa("k65")[0]
    assert DC.wgrad_kernel(d, C.BF16)[0] == "k_dwgrad_mfma<2>" and C._cdiv(d.K, C.WG_TAPS) == 9 and d.K % 8 == 1
    d = fa("wg_mfma1")[0]
    assert d.Ng % 32 == 16 and d.S * d.Cg == 16 and C._cdiv(d.K, C.WG_TAPS) == 2
    # variants widen what they say
    for base in C.VARIANT_BASES:
        d0, a0 = fa(base)
        for v, field, by in (("gap", "Tvs", 3), ("zrows", "Tvo", 3), ("pitch", "ldx", 8), ("pitch", "ldo", 8)):
            for p, q in zip(fa(f"{base}/{v}"), (d0, a0)):
                assert getattr(p, field) == getattr(q, field) + by or (field in ("Tvs", "Tvo") and getattr(
                    p, field) == (p.Tv if field == "Tvs" else p.Tvalid) + 3)


TOY = (4, 6, 5, 2, 2, 2, 2, 9)   # grouped, strided, odd T: phase view, q0 < 0, col(g, o) with So = 2 in the adjoint


@pytest.mark.parametrize("variant", [None, "gap", "zrows", "pitch"])
def test_layer_reference_is_the_primitive_formula(variant):
    """The layer view (torch conv1d and its autograd) equals the descriptor view
    (the formula of include/sel.h evaluated index by index on buffers in the
    descriptor's layout and weights in the restated pack order)."""
    case = C.Case("toy", TOY, None, "plain", variant)
    op = C.Operands(case, torch.float32, torch.device("cpu"))
    ref = C.reference(op)
    df, da, sp = op.df, op.da, op.sp
    assert (sp.K, sp.q0) == (3, -1) and df.S == 2 and da.So == 2 and da.q0 == -sp.q0 - (sp.K - 1)
    Wp = C.pack_ref(op.wq, sp, 0)
    y = C.prim_ref(df, op.x.double(), Wp)
    cols = case.cout
    pre = y[:, :df.Tvalid, :cols] + op.b.double()
    got = torch.where(pre > 0, pre, C.SLOPE * pre)
    assert torch.allclose(got, ref["y"], rtol=1e-12, atol=1e-12)
    assert torch.count_nonzero(y[:, df.Tvalid:, :cols]).item() == 0
    assert bool(torch.isnan(y[:, :, cols:]).all())
    Wd = C.pack_ref(op.wq, sp, 1).reshape(da.G, da.So * da.Ng, da.K, 1, da.Cg)
    gin = C.prim_ref(da, op.g_adj.double(), Wd)
    cin_cols = case.stride * case.cin
    assert torch.allclose(gin[:, :da.Tvalid, :cin_cols], ref["gin"], rtol=1e-12, atol=1e-12)
    assert torch.count_nonzero(gin[:, da.Tvalid:, :cin_cols]).item() == 0
    # the weight gradient from its definition
    gw = torch.zeros_like(ref["gw"])
    x, g = op.xv.double(), op.gv.double()
    Ng, Cg = case.cout // case.groups, case.cin // case.groups
    for n in range(case.cout):
        for c in range(Cg):
            for k in range(case.Kt):
                for j in range(op.T_out):
                    t = j * case.stride + k - case.pad
                    if 0 <= t < case.T:
                        gw[n, c, k] += (g[:, j, n] * x[:, t, (n // Ng) * Cg + c]).sum()
    assert torch.allclose(gw, ref["gw"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(g.sum((0, 1)), ref["gb"], rtol=1e-12, atol=1e-12)
    # the sums of absolute terms bound the sums
    assert bool((ref["S_y"] >= ref["y"].abs() - 1e-12).all()) and bool((ref["S_gw"] >= ref["gw"].abs() - 1e-12).all())
    assert bool((ref["S_gin_epi"] >= ref["gin_epi"].abs() - 1e-12).all())


def test_device_pack_order_is_the_restated_one():
    """pack_ref against the adjoint form's definition as the forward form's transpose."""
    case = C.Case("toy", TOY, None)
    op = C.Operands(case, torch.float32, torch.device("cpu"))
    Wp, Wd = C.pack_ref(op.wq, op.sp, 0), C.pack_ref(op.wq, op.sp, 1)
    G, Ng, K, s, Cg = Wp.shape
    assert torch.equal(Wd, Wp.flip(2).permute(0, 3, 4, 2, 1).reshape(G, s * Cg, K, Ng))
    assert int((Wp != 0).sum()) == op.wq.numel()      # every torch tap lands exactly once


def _ref_for_bounds():
    case = C.BY_NAME["valu"]
    op = C.Operands(case, torch.bfloat16, torch.device("cpu"))
    return case, op, C.reference(op)


def test_bounds_reject_planted_errors():
    case, op, ref = _ref_for_bounds()
    y = ref["y"]
    y = y * (1.25 / y.abs().max())          # largest element 1.25: 2 bf16 ulps there are 1.25 % of it
    got = y.to(torch.bfloat16)
    C.check_bf16(got, y, "honest bf16 rounding")
    i = int(y.abs().argmax())
    ulp = 2.0 ** -7                          # of bf16 in [1, 2)
    bad = got.double().clone()
    bad.view(-1)[i] += 2 * ulp * (1 if bad.view(-1)[i] > 0 else -1)
    assert (bad - y).norm() / y.norm() < 1e-2     # invisible to the old norm-wise limit
    with pytest.raises(AssertionError):
        C.check_bf16(bad, y, "2 ulps at the largest element")
    # a dropped tap: the reference of the same operands with the last tap's weights zeroed
    op2 = C.Operands(case, torch.bfloat16, torch.device("cpu"))
    op2.wq = op2.wq.clone()
    op2.wq[:, :, -1] = 0
    dropped = C.reference(op2)
    with pytest.raises(AssertionError):
        C.check_bf16(dropped["y"].to(torch.bfloat16), ref["y"], "dropped tap, bf16")
    n = op.df.K * op.df.S * op.df.Cg
    with pytest.raises(AssertionError):
        C.check_f32(dropped["y"].float(), ref["y"], ref["S_y"], n, "dropped tap, fp32")
    with pytest.raises(AssertionError):
        C.check_wgrad(dropped["gin"].float(), ref["gin"], ref["S_gin"], n, 1, "dropped tap, adjoint", 1e-5)
    # a dropped tap in two outputs of ONE row (a wrong tile tail): norm-wise small, element-wise caught
    one = ref["y"].clone()
    one[1, 50, :2] = dropped["y"][1, 50, :2]
    assert (one - ref["y"]).norm() / ref["y"].norm() < 1e-2
    with pytest.raises(AssertionError):
        C.check_bf16(one.to(torch.bfloat16), ref["y"], "dropped tap in one row")
    C.check_bf16(ref["y"].to(torch.bfloat16), ref["y"], "honest")


def test_bounds_are_monotone():
    """Each bound passes an error just inside its allowance and fails one just outside; a
    larger reference or sum of absolute terms allows more."""
    case, op, ref = _ref_for_bounds()
    y, S = ref["y"], ref["S_y"]
    n = op.df.K * op.df.S * op.df.Cg
    allowed = (n + 4) * C.EPS32 * S
    C.check_f32(y + 0.9 * allowed, y, S, n, "inside", norm=1.0)
    with pytest.raises(AssertionError):
        C.check_f32(y + 1.1 * allowed, y, S, n, "outside", norm=1.0)
    C.check_f32(y + 1.1 * allowed, y, 2 * S, n, "inside a doubled sum", norm=1.0)
    with pytest.raises(AssertionError):
        C.check_f32(y + 0.9 * allowed, y, S, n, "norm-wise")
    ab = 8e-3 * y.abs() + 2e-3 * y.abs().max()
    sgn = torch.where(torch.arange(y.numel()).reshape(y.shape) % 2 == 0, 1.0, -1.0)
    C.check_bf16(y + 0.2 * ab * sgn, y, "inside")      # 0.2: the norm-wise limit holds too
    with pytest.raises(AssertionError):
        C.check_bf16(y + 1.1 * ab * sgn, y, "outside")
    gw, Sg = ref["gw"], ref["S_gw"]
    rows = case.Bs * op.T_out
    aw = (rows + 5 + 2) * C.EPS32 * Sg
    C.check_wgrad(gw + 0.9 * aw, gw, Sg, rows, 5, "inside", 1.0)
    with pytest.raises(AssertionError):
        C.check_wgrad(gw + 1.1 * aw, gw, Sg, rows, 5, "outside", 1.0)
    with pytest.raises(AssertionError):
        C.check_wgrad(gw + 0.9 * aw, gw, Sg, rows, 5, "norm-wise", 1e-9)
    assert C.wgrad_norm_limit(4096, 1.0) == 1e-5 and C.wgrad_norm_limit(4097, 2e-6) == 8e-6
    assert C.wgrad_norm_limit(10 ** 6, 1.0) == 1e-4
