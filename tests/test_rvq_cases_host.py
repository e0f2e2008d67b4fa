"""CPU checks of the cases of tests/test_gpu_rvq_edges.py: that every case has
the dispatch property it is named for (the dispatch arithmetic is restated in
tests/rvq_cases.py, not read from the library), that the share of (row, stage)
pairs in which a wrong pick could hide stays under its cap, that an honest fp32
evaluation (oracle.ref_ops.rvq_forward) passes check_picks, so the derived bound
is not tighter than fp32 arithmetic allows, that check_picks does reject wrong
picks, and that the closed-form gradient is fp64 autograd's."""
import pytest
import torch

import rvq_cases as C
from oracle import ref_ops as R


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_has_its_named_property(name):
    p = C.check_properties(name)
    print(name, C.CASES[name], {k: v for k, v in p.items() if k not in ("rows",)},
          [C.kernel_of(C.CASES[name], *st) for st in C.SETTINGS])


def test_dispatch_by_hand():
    """The restated dispatch at values read off sel_rvq_fwd."""
    assert C.kernel_of((5120, 64, 1024, 8), 0, 0) == "mfma" and C.kernel_of((5120, 64, 1024, 8), 0, 2) == "mfma2"
    assert C.kernel_of((4064, 64, 1024, 8), 0, 2) == "mfma"          # 127 blocks of 32 rows: key 39 stays off
    assert C.kernel_of((77, 12, 40, 3), 2, 0) == "direct"            # D % 8 != 0
    assert C.kernel_of((40, 72, 64, 2), 0, 0) == "staged"            # the default at D = 72
    assert C.kernel_of((40, 64, 62, 2), 0, 0) == "mfma" and C.kernel_of((40, 64, 62, 2), 2, 0) == "direct"
    # what the suite ran before these cases: one pass, at most 8 stages, D <= 64 off the direct kernel
    for shape in ((5120, 64, 1024, 8), (333, 64, 1000, 3), (40, 16, 64, 2), (77, 12, 40, 3)):
        p = C.properties(shape)
        assert p["passes"] == 1 and shape[3] <= 8 and not p["bwd_wraps"]
    assert C.properties((5120, 64, 1024, 8))["last_rows"]["mfma2"] == 32      # the one key-39 shape: no ragged block


_ORACLE = {}


def _oracle_picks(name):
    """fp32 picks of the reference's own expression on the CPU, once per case"""
    if name not in _ORACLE:
        x, embeds = C.inputs(name)
        with torch.no_grad():
            idx = R.rvq_forward(x, list(embeds))[3]
        if name == "dup":
            # the reference promises no tie-break among bit-equal columns; the
            # unique column a pick stands for is what its distance is checked on
            idx = idx % C.NDUP
        _ORACLE[name] = idx
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(C.CASES))
def test_fp32_reference_passes_and_little_can_hide(name):
    x, embeds = C.inputs(name)
    N, D, K, S = C.CASES[name]
    assert x.dtype == embeds.dtype == torch.float32 and tuple(x.shape) == (N, D) and tuple(embeds.shape) == (S, D, K)
    r = C.check_picks(x, embeds, _oracle_picks(name), C.unique_of(name))
    print(f"{name}: pairs {r['pairs']} worst gap/allowed {r['worst']:.3e} hide share {100 * r['hide']:.3f} %")
    assert r["pairs"] == N * S
    assert r["nbad"] == 0 and r["out_of_range"] == 0, r["bad"]
    assert r["worst"] <= 1.0
    assert r["hide"] <= C.hide_cap(r["pairs"]), r["hide"]


def test_dup_columns_are_bit_equal():
    x, embeds = C.inputs("dup")
    K = embeds.shape[2]
    assert torch.equal(embeds, embeds[:, :, torch.arange(K) % C.NDUP])
    assert embeds[0, :, :C.NDUP].unique(dim=1).shape[1] == C.NDUP


@pytest.mark.parametrize("name", ["tiny", "d60", "dup"])
def test_check_picks_rejects_wrong_picks(name):
    """One pick moved to the row's second-best code, where the top-2 margin is
    clear, is a violation; so is an index out of range, and for `dup` a
    duplicate of the right column."""
    x, embeds = C.inputs(name)
    N, D, K, S = C.CASES[name]
    U = C.unique_of(name) or K
    idx = _oracle_picks(name)
    s = S - 1
    # the fp64 residual of the last stage, chained on idx
    r = x.double()
    for t in range(s):
        r = r - embeds[t].double()[:, idx[t]].t()
    e = embeds[s].double()[:, :U]
    dist = (r * r).sum(1, keepdim=True) - 2 * r @ e + (e * e).sum(0, keepdim=True)
    d2, k2 = torch.topk(dist, 2, dim=1, largest=False)
    row = int((d2[:, 1] - d2[:, 0]).argmax())
    wrong = idx.clone()
    wrong[s, row] = k2[row, 1]
    res = C.check_picks(x, embeds, wrong, C.unique_of(name))
    assert res["nbad"] == 1 and res["bad"][0][:2] == (row, s) and res["worst"] > 1.0
    for v in (-1, K):
        wrong = idx.clone()
        wrong[0, 0] = v
        res = C.check_picks(x, embeds, wrong, C.unique_of(name))
        assert res["out_of_range"] == 1 and res["nbad"] >= 1
    if name == "dup":
        wrong = idx.clone()
        wrong[0, 0] += C.NDUP                                        # the same column bit for bit, but not the lowest index
        res = C.check_picks(x, embeds, wrong, C.NDUP)
        assert res["out_of_range"] == 1 and res["nbad"] >= 1


def test_restate_matches_reference_fp64():
    """restate is the reference's out / losses / perplexities on the same picks"""
    g = torch.Generator().manual_seed(3)
    x = 1.5 * torch.randn(37, 6, generator=g, dtype=torch.float64)
    embeds = torch.randn(3, 6, 11, generator=g, dtype=torch.float64)
    out, losses, ppls, idx = R.rvq_forward(x, list(embeds))
    o, l, p, c = C.restate(x, embeds, idx, commitment=1.0)
    assert C.rel(o, out) < 1e-14 and C.rel(l, losses) < 1e-14 and C.rel(p, ppls) < 1e-14
    assert torch.equal(c.sum(1), torch.full((3,), 37)) and c.dtype == torch.int64
    l4 = C.restate(x, embeds, idx)[1]
    assert C.rel(l4, losses * C.COMMITMENT) < 1e-14


@pytest.mark.parametrize("terms", ["out", "losses", "both"])
def test_closed_form_gradient_is_fp64_autograd(terms):
    g = torch.Generator().manual_seed(4)
    N, D, K, S = 37, 6, 11, 3
    x = (1.5 * torch.randn(N, D, generator=g, dtype=torch.float64)).requires_grad_(True)
    embeds = torch.randn(S, D, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, D, generator=g, dtype=torch.float64)
    wl = torch.randn(S, generator=g, dtype=torch.float64)             # a weight on every stage's loss
    out, losses, _, idx = R.rvq_forward(x, list(embeds))
    loss = 0.0
    if terms in ("out", "both"):
        loss = loss + (out * w).sum()
    if terms in ("losses", "both"):
        loss = loss + (losses * wl).sum()
    loss.backward()
    ref = C.grad_closed(x, embeds, idx, w if terms != "losses" else None, wl if terms != "out" else None,
                        commitment=1.0)                               # the reference's commitment
    d = float((x.grad - ref).abs().max())
    print(terms, "max difference", d)
    assert d <= 1e-15 * max(1.0, float(ref.abs().max()))
    b = C.grad_elem_bound(x, embeds, idx, w if terms != "losses" else None, wl if terms != "out" else None, 1.0)
    assert bool((b >= 0).all()) and float(b.max()) > 0
