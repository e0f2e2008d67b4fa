"""tests/conv_cases.py on the host (no GPU): every case reaches the kernel it
names, k_conv_wss's neighbours stay off it, the restated weight-gradient plan is
the library's, the fp64 primitive is torch's conv1d, and the checkers refuse
the wrong answers they are there to refuse."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_cases as C
import conv_dispatch_cases as DCASES
from sel import convops as CO

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from sel import _lib as L
    return L.load()


# ---------------------------------------------------------------- dispatch
def test_every_case_reaches_the_kernel_it_names(lib):
    before = [lib.sel_tune_get(k) for k in (0, 4, 42, 51)]
    for case in C.CASES:
        for dt in case.dtypes:
            got = C.kernel_name(case, dt)
            if case.family == "gen":
                assert got.startswith(case.kernel), (case.name, dt, got)
            else:
                assert got == case.name_for(dt), (case.name, dt, got)
    assert [lib.sel_tune_get(k) for k in (0, 4, 42, 51)] == before
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    for c in C.CASES:       # the smallest shapes that reach their edges
        assert c.B <= 11 and c.d.T <= 1100 and c.d.C <= 192 and c.d.N <= 256 and c.d.rows <= 4500, c.name


def test_sample_tile_name_of_the_16x128_tile(lib):
    """The id's BN = 128 carries into the SPT digit; the name must not."""
    d = CO.ConvDesc(2 * 241, 241, 64, 256, 7, 9, 54, 0, 1, 0)
    with C.tuned(lib, {0: 30}):
        assert CO.fwd_kernel_name(d, torch.bfloat16, torch.bfloat16) == "k_conv_wss<7, 16, 128, bf16>"
        kid = lib.sel_conv_fwd_kernel_id(ctypes.byref(d), CO.BF16, CO.BF16, 0)
    assert kid == CO.WSS_PW_KID == 941280167
    # the five-sample tiles keep their SPT argument
    d5 = CO.ConvDesc(5 * 80, 80, 64, 128, 7, 9, 54, 0, 0, 128)
    with C.tuned(lib, {67: 1}):
        assert CO.fwd_kernel_name(d5, torch.bfloat16, torch.bfloat16) == "k_conv_wss<7, 25, 64, bf16, 5>"


def test_neighbours_do_not_reach_the_sample_tile_kernel(lib):
    for shape, pad, dt, why in C.NOT_WSS:
        d = C.not_wss_desc(shape, pad)
        with C.tuned(lib, {0: 30}):
            name = CO.fwd_kernel_name(d, torch.bfloat16, C.F32 if dt == "f32" else C.BF16)
        assert not name.startswith("k_conv_wss"), (shape, why, name)
    # ... and fp32 output takes it exactly where S = 25
    for case in C.CASES:
        if case.family == "wss":
            assert ("f32" in case.dtypes) == (", 25, 64, " in case.kernel), case.name
            if "f32" not in case.dtypes:
                with C.tuned(lib, case.tune):
                    assert not CO.fwd_kernel_name(case.d, C.BF16, C.F32).startswith("k_conv_wss"), case.name


def test_case_set_covers_the_listed_edges():
    by_family = {f: [c for c in C.CASES if c.family == f] for f in C.FAMILIES}
    halo = lambda c: (c.d.K - 1) * c.d.dil  # noqa: E731
    f4 = by_family["f4"]
    assert {int(c.kernel.split(",")[3]) for c in f4} == {1, 3, 8}                       # KMAX
    assert {c.tune[0] for c in f4} == set(range(21, 27))
    assert any(c.d.T == 1 for c in f4) and any(halo(c) == 64 for c in f4) and any(halo(c) > c.d.T for c in f4)
    assert any(c.d.N % 4 and c.d.bias_period % 4 for c in f4)
    for fam in ("f4", "ws", "wss"):
        assert any(c.d.pad_mode == 1 for c in by_family[fam]), fam
    centred = {c.tune[0] for c in C.CASES if c.family != "gen" and c.d.pad_mode == 0 and 0 < c.d.pad < halo(c)}
    assert centred >= set(range(23, 31)), centred
    assert {c.tune[0] for c in C.CASES if c.family != "gen" and halo(c) == 64} >= {23, 27, 29, 30}
    assert any(c.d.pad_mode == 1 and c.d.pad == 1 for c in f4) and any(c.d.pad_mode == 1 and c.d.pad == halo(c) for c in f4)
    for fam in ("f4", "ws"):
        assert any(c.adjoint and c.epi == "both" for c in by_family[fam]), fam
    # row tiles x column tiles with full groups of 8 AND a tail (xcd_tile)
    tile = {"f4": lambda c: int(c.kernel.split("<")[1].split(",")[0]), "ws": lambda c: 256, "ws8w": lambda c: 256}
    for fam, bm in tile.items():
        assert any(c.B * -(-c.d.T // bm(c)) > 8 and (c.B * -(-c.d.T // bm(c))) % 8 and c.d.N >= 256
                   for c in by_family[fam]), fam
    assert any(c.B * -(-c.d.T // 400) > 8 and c.d.N // 64 > 1 for c in by_family["wss"])
    # ring prologues: fewer chunks than the prefetch distance, exactly the ring
    assert {c.d.C // 16 for c in by_family["ws"]} >= {2, 4, 6, 10}
    assert {c.d.C // 16 for c in by_family["ws8"]} >= {2, 4, 6}
    assert {c.d.C // 32 for c in by_family["wss"]} >= {2, 4, 6}
    assert any(c.d.bias_period % 8 for c in by_family["ws"])
    assert {c.d.T for c in by_family["ws8"]} >= {1024, 1025, 1031}
    assert {c.d.T for c in by_family["wss"]} >= {385, 399, 400, 497, 511, 512, 1009, 1000, 241, 499}
    assert {c.kernel.split("<")[1].split(", {to}")[0] for c in by_family["wss"]} >= {
        "7, 25, 64", "3, 25, 64", "2, 25, 64", "7, 32, 64", "3, 32, 64", "2, 32, 64", "7, 16, 128"}
    for fam in ("f4", "ws", "ws8", "ws8w", "wss"):
        assert any(c.d.in_elu for c in by_family[fam]), fam
        assert {c.epi for c in by_family[fam]} >= {"aux", "res"} or {c.epi for c in by_family[fam]} >= {"both"}, fam
    assert {c.tune.get(0) for c in by_family["gen"]} >= set(range(1, 7))
    assert sum(c.in32 for c in by_family["gen"]) == 3


# ---------------------------------------------------------------- weight-gradient plan
def _ws(lib, d):
    return int(lib.sel_conv_wgrad_workspace(ctypes.byref(d)))


def test_restated_wgrad_plan_is_the_librarys(lib):
    for case in C.WGRAD_CASES:
        assert C.wgrad_workspace(case.d) == _ws(lib, case.d), case.name
    bad = [c for c in DCASES.conv_cases() if C.wgrad_workspace(CO.ConvDesc(*c)) != _ws(lib, CO.ConvDesc(*c))]
    assert not bad, bad[:5]


def test_wgrad_cases_get_the_plan_they_name():
    for case in C.WGRAD_CASES:
        p = C.wgrad_plan(case.d, C.wgrad_mode(case.d, case.bf16, case.tune), case.tune)
        assert {k: p[k] for k in case.plan} == case.plan, (case.name, p)
        assert C.wgrad_kernel(case.d, case.bf16, case.tune) == case.kernel, case.name
        assert case.d.rows <= 4500 and (case.B == 3 or "wg3_short" in case.name or "ns42" in case.name or
                                        "unpack" in case.name), case.name


def test_wgrad_case_set_covers_the_listed_edges():
    W = C.WGRAD_CASES
    reach = C.wgrad3_reachable()
    assert len(reach) == 14 and all(m <= 4 for _, _, m in reach)        # MAXT = 8 is never asked for
    assert {c.plan["inst"] for c in W if c.plan["mode"] == 3} == reach
    m3 = [c for c in W if c.plan["mode"] == 3 and c.B == 3]
    assert {c.d.T for c in m3} >= {1, 127, 129, 300}
    assert {(c.d.C, c.d.N, c.d.K) for c in m3} >= {(32, 32, 1), (32, 32, 2)}               # P = 1, 2
    short = C.W_BY_NAME["wg3_short_last_split"]
    p = C.wgrad_plan(short.d, 3)
    assert (p["n_tiles"], p["tiles_per_split"], p["nsplit"]) == (17, 2, 9)
    assert any(C.wgrad_plan(c.d, 3)["n_tiles"] < 8 for c in m3)                             # n_tiles < want
    for big in (False, True):
        for bias in (False, True):
            assert any((c.plan["nsplit"] > 32) == big and bool(c.d.bias_period) == bias for c in W), (big, bias)
    assert {c.unpack[0] for c in W if c.unpack and c.plan["nsplit"] > 32} == {CO.PACK_FWD, CO.PACK_FWD_STRIDED,
                                                                              CO.PACK_CONVT}
    names = {c.kernel for c in W}
    assert names >= {"k_wgrad_bf16<16>", "k_wgrad_bf16<32>", "k_wgrad_bf16<64>", "k_wgrad2_bf16<1>", "k_wgrad2_bf16<2>",
                     "k_wgrad2_bf16<4>", "k_wgrad_f32<3, 64, 32>", "k_wgrad_f32<8, 32, 64>", "k_wgrad_f32<1, 32, 32>",
                     "k_conv_wgrad<float>"}
    assert names >= {f"k_wgrad_c1<{t}, {m}>" for t in ("bf16", "float") for m in (1, 2, 4, 8)}
    g = C.W_BY_NAME["wgf_generic"]
    assert g.d.C % 4 and C.generic_f32_splits(g.d, g.plan["nsplit"]) < g.plan["nsplit"]     # the memset tail
    assert any(c.d.pad_mode == 1 for c in W) and any(c.d.in_elu and c.bf16 for c in W)


# ---------------------------------------------------------------- the reference is torch's conv1d
def _layer(case, x, wp, bias):
    """The layer view of a primitive in fp64: conv1d over (B, C, T) with weight
    (N, C, K), dilation, left pad `pad` and right pad halo - pad (zero or
    replicate), cut to T outputs."""
    d = case.d
    halo = (d.K - 1) * d.dil
    xl = x.view(case.B, d.T, d.C).permute(0, 2, 1)
    right = max(0, halo - d.pad)
    xl = F.pad(xl, (d.pad, right), mode="replicate" if d.pad_mode else "constant")
    y = F.conv1d(xl, wp.permute(0, 2, 1), None, dilation=d.dil)[:, :, :d.T]
    y = y.permute(0, 2, 1).reshape(d.rows, d.N)
    return y + bias.double().repeat(d.N // bias.numel()) if bias is not None else y


@pytest.mark.parametrize("name", ["f4_257_v23", "f4_centred", "f4_rep1", "f4_rephalo", "f4_halo_gt_t", "f4_t1_k8", "wss_399"])
def test_reference_is_torch_conv1d(name):
    case = C.BY_NAME[name]
    if case.d.in_elu:
        case = C.Case(case.name, case.family, (case.B, case.d.T, case.d.C, case.d.N, case.d.K, case.d.dil), case.kernel,
                      pad=case.d.pad, mode=case.d.pad_mode, bias=case.d.bias_period)
    x, wp, b, _, _ = C.operands(case, CPU)
    xr, wr = x.double().requires_grad_(True), wp.double().requires_grad_(True)
    y = _layer(case, xr, wr, b)
    ref = C._ref(x, wp, case.d, case.B, b)
    assert torch.allclose(y.detach(), ref, rtol=1e-12, atol=1e-12), name
    # the adjoint primitive and the weight gradient are that layer's autograd
    g = torch.randn(case.d.rows, case.d.N, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    y.backward(g.double())
    if case.d.pad_mode == 0:
        da = case.d.adjoint()
        wd = wp.permute(2, 1, 0).flip(1).contiguous()      # Wd[c][K-1-k][n] = Wp[n][k][c]
        gx = C._ref(g, wd, da, case.B)
        assert torch.allclose(gx, xr.grad, rtol=1e-12, atol=1e-12), name
    wc = C.WCase(name, (case.B, case.d.T, case.d.C, case.d.N, case.d.K, case.d.dil), "", 0, 0, 0, pad=case.d.pad,
                 mode=case.d.pad_mode, bias=case.d.bias_period)
    r = C.wgrad_reference(wc, g, x)
    assert torch.allclose(r["gw"], wr.grad, rtol=1e-12, atol=1e-12), name
    if case.d.bias_period:
        assert torch.allclose(r["gb"], g.double().sum(0).view(-1, case.d.bias_period).sum(0), rtol=1e-12, atol=1e-12)


def test_unpack_ref_is_the_pack_inverse():
    """unpack_ref sends the packed gradient of a layer to d(layer)/d(torch weight)."""
    g = torch.Generator().manual_seed(3)
    # strided conv (cout, cin, 2 s), stride s, causal: phase view C = s cin, K = 3, pad 2
    cout, cin, s, B, To = 4, 3, 2, 2, 9
    w = torch.randn(cout, cin, 2 * s, generator=g, dtype=torch.float64, requires_grad=True)
    x = torch.randn(B, cin, To * s, generator=g, dtype=torch.float64)
    gy = torch.randn(B, cout, To, generator=g, dtype=torch.float64)
    y = F.conv1d(F.pad(x, (2 * s - 1, 0)), w, stride=s)[:, :, :To]
    y.backward(gy)
    wc = C.WCase("s", (B, To, s * cin, cout, 3, 1), "", 0, 0, 0, pad=2, dt="f32")
    xp = x.permute(0, 2, 1).reshape(B * To, s * cin).float()
    r = C.wgrad_reference(wc, gy.permute(0, 2, 1).reshape(B * To, cout).float(), xp)
    got = C.unpack_ref(CO.PACK_FWD_STRIDED, r["gw"], cout, cin, 2 * s, s)
    assert torch.allclose(got, w.grad, rtol=1e-5, atol=1e-5)
    wf = torch.randn(5, 3, 4, dtype=torch.float64, generator=g)
    assert torch.equal(C.unpack_ref(CO.PACK_FWD, wf.permute(0, 2, 1).contiguous(), 5, 3, 4, 1), wf)


# ---------------------------------------------------------------- the checkers have teeth
def _teeth_cases(fam):
    """Per family the three or more smallest cases a mutation can apply to."""
    cs = sorted((c for c in C.CASES if c.family == fam and c.d.rows > 1 and c.d.C >= 32),
                key=lambda c: c.d.rows * c.d.C * c.d.N * c.d.K)
    return cs[:4]


_TEETH = {}


def _teeth_setup(case):
    if _TEETH.get("name") != case.name:
        _TEETH.clear()
        ops = C.operands(case, CPU)
        _TEETH.update(name=case.name, ops=ops, ref=C.reference(case, ops))
    return _TEETH["ops"], _TEETH["ref"]


@pytest.mark.parametrize("fam", C.FAMILIES)
def test_checkers_have_teeth(fam):
    cases = _teeth_cases(fam)
    assert len(cases) >= 3, fam
    caught = {m: 0 for m in C.MUTATIONS}
    for case in cases:
        ops, ref = _teeth_setup(case)
        for dt in case.dtypes:
            tdt = C.BF16 if dt == "bf16" else C.F32
            C.check_output(case, dt, ref["y"].to(tdt), ref, f"{case.name} {dt} rounded reference")
        for how in C.MUTATIONS:
            wrong = C.mutate(case, ops, ref, how)
            hits = 0
            for dt in case.dtypes:
                with pytest.raises(AssertionError):
                    C.check_output(case, dt, wrong.to(C.BF16 if dt == "bf16" else C.F32), ref, f"{case.name} {dt} {how}")
                hits += 1
            caught[how] += hits == len(case.dtypes)
    assert all(n >= 3 for n in caught.values()), caught


def test_wgrad_checker_has_teeth():
    picks = ["wg3_c64_n64_k3_t127", "wg3_c64_n32_k5_t300", "wg_generic_bn32", "wg2_k4", "wgf_64x32"]
    for name in picks:
        case = C.W_BY_NAME[name]
        g, x = C.wgrad_operands(case, CPU)
        ref = C.wgrad_reference(case, g, x)
        n, ns = case.d.rows, case.plan["nsplit"]
        C.check_wgrad(ref["gw"].float(), ref["gw"], ref["S_gw"], n, ns, f"{name} rounded reference", ref["slack"])
        for how in C.WGRAD_MUTATIONS:
            wrong = C.mutate_wgrad(case, g, x, ref, how)
            with pytest.raises(AssertionError):
                C.check_wgrad(wrong.float(), ref["gw"], ref["S_gw"], n, ns, f"{name} {how}", ref["slack"])


# ---------------------------------------------------------------- ELU ambiguity
def test_ambiguous_share_of_elu_cases_is_small():
    seen = 0
    for case in C.CASES:
        if case.d.in_elu and not case.in32:
            x = C.operands(case, CPU)[0]
            _, ulp = C.act_operand(x, case.d)
            share = float((ulp > 0).double().mean())
            print(f"{case.name}: ambiguous share {share:.4%}")
            assert share < 0.01, (case.name, share)
            seen += 1
    for case in C.WGRAD_CASES:
        if case.d.in_elu and case.bf16:
            _, ulp = C.act_operand(C.wgrad_operands(case, CPU)[1], case.d)
            assert float((ulp > 0).double().mean()) < 0.01, case.name
            seen += 1
    assert seen >= 6
