"""GPU checks of the residual-VQ kernels (vq.hip) at the edges of their
dispatch: every case of tests/rvq_cases.py under the four settings of tune
keys 2 and 39 (default, direct, staged, two row groups per matrix-core block),
against fp64 on the CPU.  That each case has the property it is named for, and
that little can hide from the pick check, is asserted without a GPU by
tests/test_rvq_cases_host.py.

A  picks: in range, within the derived bound of rvq_cases.check_picks of the
   fp64 argmin, chained on the kernel's own picks; `dup`: lowest index wins.
   counts = bincount(picks).  out / losses / perplexities against the fp64
   restatement on the kernel's own picks at the project's RVQ tolerances
   (1e-6 / 1e-5 / 1e-6, norm-wise).  Picks, out and perplexities bit-identical
   across the four settings, losses to 1e-6.
B  backward on `wrap`, `d255`, `d60` against the closed form, with the output
   gradient, the loss gradient or both present.
C  argument checks that must raise before any kernel runs.
"""
import contextlib

import pytest
import torch

import rvq_cases as C

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_LOSS, TOL_PPL = 1e-6, 1e-5, 1e-6


@contextlib.contextmanager
def _poisoned_empty():
    """While active, torch.empty / torch.empty_like (what ResidualVQFn allocates
    its outputs, its gradient and its workspace with) hand out NaN (all-ones
    bytes / -1 for integers) instead of whatever the caching allocator's block
    held: the four settings produce identical results in the block the last one
    freed, so an element a kernel does not write would otherwise pass on a stale
    copy."""
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            return t.fill_(float("nan"))
        return t.fill_(255 if t.dtype == torch.uint8 else -1)

    torch.empty = lambda *a, **k: fill(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(real_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


def _forward(gpu, x, embeds, key2, key39, commitment=C.COMMITMENT):
    from sel import _lib as L
    from sel.vqops import ResidualVQFn
    lib = L.lib()
    prev, prevg = lib.sel_tune(2, key2), lib.sel_tune(39, key39)
    try:
        aux = {}
        with _poisoned_empty():
            out, losses, ppls, idx = ResidualVQFn.apply(x.to(gpu), embeds.to(gpu), commitment, aux)
            torch.cuda.synchronize()
    finally:
        lib.sel_tune(2, prev)
        lib.sel_tune(39, prevg)
    return out.cpu(), losses.cpu(), ppls.cpu(), idx.cpu(), aux["counts"].cpu()


# ---------------------------------------------------------------------------
# A. forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_matches_fp64_under_every_setting(gpu, name):
    case = C.CASES[name]
    N, D, K, S = case
    C.check_properties(name)
    x, embeds = C.inputs(name)
    runs = []
    for key2, key39 in C.SETTINGS:
        out, losses, ppls, idx, counts = _forward(gpu, x, embeds, key2, key39)
        tag = f"{name} keys ({key2}, {key39}) {C.kernel_of(case, key2, key39)}"
        assert tuple(out.shape) == (N, D) and tuple(idx.shape) == (S, N) and tuple(counts.shape) == (S, K)
        assert tuple(losses.shape) == tuple(ppls.shape) == (S,)
        assert idx.dtype == torch.int64 and counts.dtype == torch.int32
        assert int(idx.min()) >= 0 and int(idx.max()) < K, (tag, int(idx.min()), int(idx.max()))
        r = C.check_picks(x, embeds, idx, C.unique_of(name))
        o, l, p, c = C.restate(x, embeds, idx)
        e = dict(out=C.rel(out, o), losses=C.rel(losses, l), ppls=C.rel(ppls, p))
        print(f"{tag}: worst gap/allowed {r['worst']:.3e} hide share {100 * r['hide']:.3f} % of {r['pairs']} pairs; "
              + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert r["nbad"] == 0 and r["out_of_range"] == 0, (tag, r["bad"])
        assert r["hide"] <= C.hide_cap(r["pairs"]), (tag, r["hide"])
        assert torch.equal(counts.long(), c), (tag, (counts.long() != c).nonzero()[:6].tolist())
        assert bool(torch.isfinite(out).all() and torch.isfinite(losses).all() and torch.isfinite(ppls).all()), tag
        assert e["out"] <= TOL_OUT and e["losses"] <= TOL_LOSS and e["ppls"] <= TOL_PPL, (tag, e)
        runs.append((tag, out, losses, ppls, idx))
    tag0, o0, l0, p0, i0 = runs[0]
    for tag, o1, l1, p1, i1 in runs[1:]:
        assert torch.equal(i1, i0), (tag, tag0, (i1 != i0).nonzero()[:6].tolist())
        assert torch.equal(o1, o0) and torch.equal(p1, p0), (tag, tag0)
        torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------
# B. backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["out", "losses", "both"])
@pytest.mark.parametrize("name", C.BWD_CASES)
def test_backward_matches_closed_form(gpu, name, terms):
    from sel.vqops import ResidualVQFn
    N, D, K, S = C.CASES[name]
    x, embeds = C.inputs(name)
    g = torch.Generator().manual_seed(11)
    w = torch.randn(N, D, generator=g)
    wl = torch.randn(S, generator=g)
    xg = x.to(gpu).requires_grad_(True)
    out, losses, _, idx = ResidualVQFn.apply(xg, embeds.to(gpu), C.COMMITMENT)
    loss = 0.0
    if terms in ("out", "both"):
        loss = loss + (out * w.to(gpu)).sum()          # alone: the loss gradient arrives as None
    if terms in ("losses", "both"):
        loss = loss + (losses * wl.to(gpu)).sum()      # alone: the output gradient arrives as None
    with _poisoned_empty():                            # an element the kernel leaves unwritten is NaN
        loss.backward()
        torch.cuda.synchronize()
    go, gl = (w if terms != "losses" else None), (wl if terms != "out" else None)
    ref = C.grad_closed(x, embeds, idx, go, gl)
    got = xg.grad.cpu()
    e = C.rel(got, ref)
    print(f"{name} {terms}: gradient {e:.2e}")
    assert tuple(got.shape) == (N, D) and bool(torch.isfinite(got).all())
    assert e <= 1e-6, e
    if name == "wrap":
        # the second grid-stride sweep writes the last 1024 elements only
        assert N * D - C.BWD_GRID == 1024
        tail, rt = got.flatten()[-2048:].double(), ref.flatten()[-2048:]
        bound = C.grad_elem_bound(x, embeds, idx, go, gl).flatten()[-2048:]
        err = (tail - rt).abs()
        print(f"{name} {terms}: tail worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (err > bound).nonzero()[:6].tolist()
        assert C.rel(tail[-1024:], rt[-1024:]) <= 1e-6 and C.rel(tail[:1024], rt[:1024]) <= 1e-6


# ---------------------------------------------------------------------------
# C. argument checks: no kernel runs
# ---------------------------------------------------------------------------
def test_bad_arguments_raise(gpu):
    from sel import _lib as L
    from sel.vqops import ResidualVQFn
    x = torch.randn(8, 4, device=gpu)
    embeds = torch.randn(2, 4, 16, device=gpu)
    with pytest.raises(L.SelError, match="fp32"):
        ResidualVQFn.apply(x, embeds.bfloat16(), 1.0)
    with pytest.raises(L.SelError, match="D = 4"):
        ResidualVQFn.apply(x, torch.randn(2, 8, 16, device=gpu), 1.0)
    with pytest.raises(L.SelError, match="D = 4"):
        ResidualVQFn.apply(x, embeds[0], 1.0)
    with pytest.raises(L.SelError, match=r"\(N, D\)"):
        ResidualVQFn.apply(x.reshape(2, 4, 4), embeds, 1.0)


def test_empty_input_raises_and_library_stays_usable(gpu):
    from sel import _lib as L
    x, embeds = C.inputs("one")
    with pytest.raises(L.SelError, match="sel_rvq_finish"):
        _forward(gpu, x[:0], embeds, 0, 0)
    out, losses, ppls, idx, counts = _forward(gpu, x, embeds, 0, 0)
    o, l, p, c = C.restate(x, embeds, idx)
    assert torch.equal(idx, torch.zeros(1, 1, dtype=torch.int64)) and torch.equal(counts.long(), c)
    assert C.rel(out, o) <= TOL_OUT and C.rel(losses, l) <= TOL_LOSS and C.rel(ppls, p) <= TOL_PPL
