"""GPU checks of the streaming RVQ step kernels (csrc/vq_step.hip) on the cases
of tests/rvq_step_ref.py (each the smallest shape that reaches one edge; that
it does, and that little can hide from the pick check, is asserted without a
GPU by tests/test_rvq_step_host.py).

A  sel_rvq_step: idx and zq bit-identical to sel_rvq_fwd under the four
   settings of tune keys 2 and 39; the picks within rvq_cases.check_picks of the
   fp64 argmin, flattened and not; zq = NULL; every n_active of {NULL, 0, 1, all,
   all + 1, -1} with sentinel-filled outputs whose rows beyond the active ones
   must stay untouched; one captured launch replayed on three staged counts.
B  sel_rvq_lookup_step: fp32 output bit-identical to the ascending-order loop of
   torch adds, bf16 output to that loop's .to(bfloat16); with mean / scale
   bit-identical to torch's (c - mean) / scale in fp32 and in bf16.  The
   contract allows one ulp there; the MI355X shows equal bits on every
   element of every stats case (both sides subtract and divide with correct
   rounding), so equality is what is asserted, after the one-ulp bound.  The
   same n_active set; the element-wise path through an odd D and through a
   misaligned codebook.
C  operand checks of the bindings that must raise before any launch.
"""
import pytest
import torch

import rvq_cases as C
import rvq_step_ref as SR

pytestmark = pytest.mark.gpu

COUNTS = ("null", 0, 1, "all", "all+1", -1)


def _count(c, B):
    return {"null": None, "all": B, "all+1": B + 1}.get(c, c)


def _active(c, B):
    n = _count(c, B)
    return B if n is None else min(max(n, 0), B)


_FWD = {}


def _module_path(gpu, name):
    """sel_rvq_fwd's (idx, out) under the four settings, once per case"""
    if name not in _FWD:
        from sel import _lib as L
        from sel.vqops import ResidualVQFn
        z, embeds = SR.inputs(name)
        lib = L.lib()
        runs = []
        for key2, key39 in C.SETTINGS:
            prev, prevg = lib.sel_tune(2, key2), lib.sel_tune(39, key39)
            try:
                out, _, _, idx = ResidualVQFn.apply(z.to(gpu), embeds.to(gpu), C.COMMITMENT)
                torch.cuda.synchronize()
            finally:
                lib.sel_tune(2, prev)
                lib.sel_tune(39, prevg)
            runs.append((idx.cpu(), out.cpu()))
        _FWD[name] = runs
    return _FWD[name]


def _step(gpu, name, count="null", flatten=False, with_zq=True):
    """One eager sel_rvq_step on sentinel-filled outputs -> (idx, zq) on the CPU."""
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    z, embeds = SR.inputs(name)
    idx = torch.full((S, rows), -1, dtype=torch.int64, device=gpu)
    zq = torch.full((rows, D), float("nan"), device=gpu) if with_zq else None
    n = _count(count, rows // T)
    n_active = None if n is None else torch.tensor([n], dtype=torch.int32, device=gpu)
    SO.rvq_step(z.to(gpu), embeds.to(gpu), idx, T, n_active, flatten, zq)
    torch.cuda.synchronize()
    return idx.cpu(), (zq.cpu() if with_zq else None)


# ---------------------------------------------------------------------------
# A. sel_rvq_step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_equals_module_path_and_fp64(gpu, name):
    rows, T, D, K, S = SR.CASES[name]
    SR.check_properties(name)
    z, embeds = SR.inputs(name)
    idx, zq = _step(gpu, name)
    assert int(idx.min()) >= 0 and int(idx.max()) < K and bool(torch.isfinite(zq).all())
    for (key2, key39), (i0, o0) in zip(C.SETTINGS, _module_path(gpu, name)):
        tag = f"{name} keys ({key2}, {key39}) {C.kernel_of((rows, D, K, S), key2, key39)}"
        assert torch.equal(idx, i0), (tag, (idx != i0).nonzero()[:6].tolist())
        assert torch.equal(zq, o0), (tag, (zq != o0).nonzero()[:6].tolist())
    flat, zq_f = _step(gpu, name, flatten=True)
    assert torch.equal(flat, idx + K * torch.arange(S).view(-1, 1)) and torch.equal(zq_f, zq)
    for tag, picks in (("plain", idx), ("flatten", flat - K * torch.arange(S).view(-1, 1))):
        r = C.check_picks(z, embeds, picks, SR.unique_of(name))
        print(f"{name} {tag}: worst gap/allowed {r['worst']:.3e} hide share {100 * r['hide']:.3f} % of {r['pairs']}")
        assert r["nbad"] == 0 and r["out_of_range"] == 0, (name, tag, r["bad"])
        assert r["hide"] <= C.hide_cap(r["pairs"]), (name, r["hide"])
    only_idx, none = _step(gpu, name, with_zq=False)
    assert none is None and torch.equal(only_idx, idx)


@pytest.mark.parametrize("count", COUNTS, ids=[str(c) for c in COUNTS])
@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_active_set(gpu, name, count):
    rows, T, D, K, S = SR.CASES[name]
    live = _active(count, rows // T) * T
    full_idx, full_zq = _module_path(gpu, name)[0]
    idx, zq = _step(gpu, name, count)
    assert torch.equal(idx[:, :live], full_idx[:, :live]) and torch.equal(zq[:live], full_zq[:live])
    assert bool((idx[:, live:] == -1).all()) and bool(torch.isnan(zq[live:]).all())


@pytest.mark.parametrize("name", ["hop", "pool", "d255", "s17"])
def test_step_captured_launch_follows_staged_counts(gpu, name):
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    z, embeds = SR.inputs(name)
    zd, ed = z.to(gpu), embeds.to(gpu)
    idx = torch.full((S, rows), -1, dtype=torch.int64, device=gpu)
    zq = torch.full((rows, D), float("nan"), device=gpu)
    n_active = torch.zeros(1, dtype=torch.int32, device=gpu)
    SO.rvq_step(zd, ed, idx, T, n_active, True, zq)          # loads the kernel; no active row
    torch.cuda.synchronize()
    assert bool((idx == -1).all()) and bool(torch.isnan(zq).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        SO.rvq_step(zd, ed, idx, T, n_active, True, zq)
    full_idx, full_zq = _module_path(gpu, name)[0]
    full_idx = full_idx + K * torch.arange(S).view(-1, 1)
    for n in (B, max(B // 2, 1) if B > 1 else 0, B + 3):
        idx.fill_(-1)
        zq.fill_(float("nan"))
        n_active.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        live = min(n, B) * T
        assert torch.equal(idx.cpu()[:, :live], full_idx[:, :live]) and torch.equal(zq.cpu()[:live], full_zq[:live])
        assert bool((idx[:, live:] == -1).all()) and bool(torch.isnan(zq[live:]).all())


# ---------------------------------------------------------------------------
# B. sel_rvq_lookup_step
# ---------------------------------------------------------------------------
LK_ROWS, LK_T, LK_K = 6, 2, 5


def _lookup_inputs(gpu, D, S, misalign=False):
    g = torch.Generator().manual_seed(100 * D + S)
    ncodes = S * LK_K
    cb = torch.randn(ncodes, D, generator=g)
    idx = torch.randint(0, ncodes, (S, LK_ROWS), generator=g)
    idx[0, 0], idx[-1, -1] = 0, ncodes - 1
    idx[0, 1] = ncodes - 1
    idx[-1, 2] = 0
    mean = torch.randn(D, generator=g)
    scale = torch.rand(D, generator=g) + 0.5
    if misalign:
        pad = torch.zeros(ncodes * D + 1, device=gpu)
        cbd = pad[1:].view(ncodes, D)
        cbd.copy_(cb)
        assert cbd.data_ptr() % 16 == 4 and cbd.is_contiguous()
    else:
        cbd = cb.to(gpu)
    return idx.to(gpu), cbd, mean.to(gpu), scale.to(gpu)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("D", [3, 64, 256, "64-misaligned"])
def test_lookup_equals_ordered_torch_loop(gpu, D, S, dtype, stats):
    from sel import streamops as SO
    misalign = D == "64-misaligned"
    D = 64 if misalign else D
    idx, cb, mean, scale = _lookup_inputs(gpu, D, S, misalign)
    assert int(idx.min()) == 0 and int(idx.max()) == cb.shape[0] - 1
    ms = (mean, scale) if stats else (None, None)
    ref = SR.ordered_lookup(idx, cb, *ms).to(dtype)
    B = LK_ROWS // LK_T
    for count in COUNTS:
        out = torch.full((LK_ROWS, D), float("nan"), dtype=dtype, device=gpu)
        n = _count(count, B)
        n_active = None if n is None else torch.tensor([n], dtype=torch.int32, device=gpu)
        SO.rvq_lookup_step(idx, cb, out, LK_T, ms[0], ms[1], n_active)
        torch.cuda.synchronize()
        live = _active(count, B) * LK_T
        assert bool(torch.isnan(out[live:]).all()), count
        got, want = out[:live], ref[:live]
        if stats:
            # the contract: one ulp of torch's (c - mean) / scale in the output dtype
            ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
            err = (got.double() - want.double()).abs()
            differ = int((got != want).sum())
            print(f"D {D} S {S} {dtype} count {count}: {differ} of {got.numel()} elements differ from torch, "
                  f"worst {float((err / want.double().abs().clamp_min(1e-300)).max()) if live else 0.0:.3e} relative")
            assert bool((err <= ulp * want.double().abs()).all()), count
        assert torch.equal(got, want), (count, (got != want).nonzero()[:6].tolist())


# ---------------------------------------------------------------------------
# C. the bindings refuse bad operands before any launch
# ---------------------------------------------------------------------------
def test_bindings_refuse_bad_operands(gpu):
    from sel import _lib as L
    from sel import streamops as SO
    z = torch.zeros(4, 8, device=gpu)
    e = torch.zeros(2, 8, 16, device=gpu)
    idx = torch.zeros(2, 4, dtype=torch.int64, device=gpu)
    for bad in (dict(z=z.cpu()), dict(z=z.bfloat16()), dict(z=z[:, :4]), dict(z=z.t().contiguous().t()),
                dict(embeds=e.bfloat16()), dict(embeds=e[0]), dict(embeds=e.transpose(1, 2)),
                dict(idx=idx.int()), dict(idx=idx[:, :3]), dict(idx=idx.t().contiguous().t()),
                dict(zq=z.bfloat16()), dict(zq=z[:2]), dict(rows_per_sample=3), dict(rows_per_sample=0),
                dict(n_active=torch.zeros(1, device=gpu)), dict(n_active=torch.zeros(1, dtype=torch.int32))):
        a = dict(z=z, embeds=e, idx=idx)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_step(**a)
    cb = torch.zeros(32, 8, device=gpu)
    out = torch.zeros(4, 8, device=gpu)
    m = torch.zeros(8, device=gpu)
    for bad in (dict(idx=idx.cpu()), dict(idx=idx.int()), dict(idx=idx[0]), dict(codebook=cb.bfloat16()),
                dict(codebook=cb[:, :4]), dict(out=out.half()), dict(out=out[:2]), dict(out=out.t().contiguous().t()),
                dict(mean=m), dict(scale=m), dict(mean=m[:4], scale=m), dict(mean=m.double(), scale=m),
                dict(rows_per_sample=3), dict(n_active=torch.zeros(1, device=gpu))):
        a = dict(idx=idx, codebook=cb, out=out)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_lookup_step(**a)
