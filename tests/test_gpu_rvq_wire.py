"""GPU checks of the wire-format kernels (csrc/vq_step.hip: sel_rvq_step_wire,
sel_rvq_lookup_wire_step) on the nine cases of tests/rvq_step_ref.py.  Two
references, neither the code under test: tests/wire_ref.py (the format in plain
Python integers) and the existing sel_rvq_step / sel_rvq_lookup_step.  Every
comparison is exact.

A  sel_rvq_step_wire: idx and zq torch.equal to sel_rvq_step's, flattened and
   not; the records equal wire_ref.pack of those picks byte for byte on a buffer
   pre-filled with 0xFF (so the zero pad bits are checked); idx = NULL and
   zq = NULL; every n_active of {NULL, 0, 1, all, all + 1, -1} with the bytes of
   the rows beyond the active ones still 0xFF; one captured launch replayed on
   three staged counts.
B  sel_rvq_lookup_wire_step: output torch.equal to sel_rvq_lookup_step on the
   unpacked ids, fp32 and bf16, with and without mean / scale; idx_out equal to
   the ids; a wire view starting one byte into its allocation; all-ones pad
   bits; a field >= K in a stage that is not the last (a kernel without the
   guard would read the next stage's rows, inside the codebook) equals the sum
   without that stage; the same n_active set on NaN / sentinel-filled outputs.
C  operand checks of the bindings that must raise before any launch.
"""
import pytest
import torch

import rvq_step_ref as SR
import wire_ref as WR

pytestmark = pytest.mark.gpu

COUNTS = ("null", 0, 1, "all", "all+1", -1)


def _count(c, B):
    return {"null": None, "all": B, "all+1": B + 1}.get(c, c)


def _active(c, B):
    n = _count(c, B)
    return B if n is None else min(max(n, 0), B)


def _n_active(gpu, count, B):
    n = _count(count, B)
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=gpu)


_STEP = {}


def _existing_step(gpu, name):
    """sel_rvq_step's (idx unflattened, zq) on the CPU, once per case"""
    if name not in _STEP:
        from sel import streamops as SO
        rows, T, D, K, S = SR.CASES[name]
        z, embeds = SR.inputs(name)
        idx = torch.full((S, rows), -1, dtype=torch.int64, device=gpu)
        zq = torch.full((rows, D), float("nan"), device=gpu)
        SO.rvq_step(z.to(gpu), embeds.to(gpu), idx, T, None, False, zq)
        torch.cuda.synchronize()
        assert int(idx.min()) >= 0 and int(idx.max()) < K
        _STEP[name] = (idx.cpu(), zq.cpu())
    return _STEP[name]


def _step_wire(gpu, name, count="null", flatten=False, with_idx=True, with_zq=True):
    """One eager sel_rvq_step_wire on sentinel-filled outputs -> (idx, zq, wire) on the CPU."""
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    z, embeds = SR.inputs(name)
    idx = torch.full((S, rows), -1, dtype=torch.int64, device=gpu) if with_idx else None
    zq = torch.full((rows, D), float("nan"), device=gpu) if with_zq else None
    wire = torch.full((rows, WR.frame_bytes(S, K)), 0xFF, dtype=torch.uint8, device=gpu)
    SO.rvq_step_wire(z.to(gpu), embeds.to(gpu), wire, T, _n_active(gpu, count, rows // T), flatten, idx, zq)
    torch.cuda.synchronize()
    return (idx.cpu() if with_idx else None), (zq.cpu() if with_zq else None), wire.cpu()


# ---------------------------------------------------------------------------
# A. sel_rvq_step_wire
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_wire_equals_step_and_the_reference(gpu, name):
    rows, T, D, K, S = SR.CASES[name]
    idx0, zq0 = _existing_step(gpu, name)
    want = WR.pack(idx0, K)
    idx, zq, wire = _step_wire(gpu, name)
    assert torch.equal(idx, idx0) and torch.equal(zq, zq0)
    assert torch.equal(wire, want), (wire != want).nonzero()[:6].tolist()
    flat, zq_f, wire_f = _step_wire(gpu, name, flatten=True)
    assert torch.equal(flat, idx0 + K * torch.arange(S).view(-1, 1)) and torch.equal(zq_f, zq0)
    assert torch.equal(wire_f, want)                      # the record holds un-flattened codes either way
    none, zq_n, wire_n = _step_wire(gpu, name, with_idx=False)
    assert none is None and torch.equal(zq_n, zq0) and torch.equal(wire_n, want)
    idx_n, none, wire_n = _step_wire(gpu, name, with_zq=False)
    assert none is None and torch.equal(idx_n, idx0) and torch.equal(wire_n, want)
    none, none2, wire_n = _step_wire(gpu, name, with_idx=False, with_zq=False)
    assert none is None and none2 is None and torch.equal(wire_n, want)


@pytest.mark.parametrize("count", COUNTS, ids=[str(c) for c in COUNTS])
@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_wire_active_set(gpu, name, count):
    rows, T, D, K, S = SR.CASES[name]
    live = _active(count, rows // T) * T
    idx0, zq0 = _existing_step(gpu, name)
    idx, zq, wire = _step_wire(gpu, name, count)
    assert torch.equal(idx[:, :live], idx0[:, :live]) and torch.equal(zq[:live], zq0[:live])
    assert torch.equal(wire[:live], WR.pack(idx0, K)[:live])
    assert bool((idx[:, live:] == -1).all()) and bool(torch.isnan(zq[live:]).all())
    assert bool((wire[live:] == 0xFF).all())


@pytest.mark.parametrize("name", ["hop", "pool", "d255", "s17"])
def test_step_wire_captured_launch_follows_staged_counts(gpu, name):
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    z, embeds = SR.inputs(name)
    zd, ed = z.to(gpu), embeds.to(gpu)
    idx = torch.full((S, rows), -1, dtype=torch.int64, device=gpu)
    zq = torch.full((rows, D), float("nan"), device=gpu)
    wire = torch.full((rows, WR.frame_bytes(S, K)), 0xFF, dtype=torch.uint8, device=gpu)
    n_active = torch.zeros(1, dtype=torch.int32, device=gpu)
    SO.rvq_step_wire(zd, ed, wire, T, n_active, True, idx, zq)          # loads the kernel; no active row
    torch.cuda.synchronize()
    assert bool((idx == -1).all()) and bool(torch.isnan(zq).all()) and bool((wire == 0xFF).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        SO.rvq_step_wire(zd, ed, wire, T, n_active, True, idx, zq)
    idx0, zq0 = _existing_step(gpu, name)
    want = WR.pack(idx0, K)
    flat0 = idx0 + K * torch.arange(S).view(-1, 1)
    for n in (B, max(B // 2, 1) if B > 1 else 0, B + 3):
        idx.fill_(-1)
        zq.fill_(float("nan"))
        wire.fill_(0xFF)
        n_active.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        live = min(n, B) * T
        assert torch.equal(idx.cpu()[:, :live], flat0[:, :live]) and torch.equal(zq.cpu()[:live], zq0[:live])
        assert torch.equal(wire.cpu()[:live], want[:live])
        assert bool((idx[:, live:] == -1).all()) and bool(torch.isnan(zq[live:]).all())
        assert bool((wire[live:] == 0xFF).all())


# ---------------------------------------------------------------------------
# B. sel_rvq_lookup_wire_step
# ---------------------------------------------------------------------------
LK_ROWS, LK_T = 6, 2
LK_SHAPES = [(64, 1024, 8), (3, 37, 2), (256, 1000, 1), (8, 16, 17)]        # (D, K, S)


def _lookup_inputs(gpu, D, K, S):
    g = torch.Generator().manual_seed(7 * D + 3 * K + S)
    cb = torch.randn(S * K, D, generator=g)
    k = torch.randint(0, K, (S, LK_ROWS), generator=g)
    k[0, 0], k[-1, -1] = 0, K - 1
    k[0, 1], k[-1, 2] = K - 1, 0
    mean = torch.randn(D, generator=g)
    scale = torch.rand(D, generator=g) + 0.5
    return k, cb.to(gpu), mean.to(gpu), scale.to(gpu)


def _existing_lookup(gpu, ids, cb, dtype, ms):
    """sel_rvq_lookup_step on flattened ids (S, rows), every row active"""
    from sel import streamops as SO
    out = torch.full((ids.shape[1], cb.shape[1]), float("nan"), dtype=dtype, device=gpu)
    SO.rvq_lookup_step(ids.to(gpu), cb, out, LK_T, ms[0], ms[1], None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    return out


def _lookup_wire(gpu, wire, cb, S, dtype, ms, count="null", with_idx=True):
    from sel import streamops as SO
    rows = wire.shape[0]
    out = torch.full((rows, cb.shape[1]), float("nan"), dtype=dtype, device=gpu)
    idx_out = torch.full((S, rows), -7, dtype=torch.int64, device=gpu) if with_idx else None
    SO.rvq_lookup_wire_step(wire, cb, S, out, LK_T, ms[0], ms[1], _n_active(gpu, count, rows // LK_T), idx_out)
    torch.cuda.synchronize()
    return out, idx_out


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,K,S", LK_SHAPES)
def test_lookup_wire_equals_lookup_step(gpu, D, K, S, dtype, stats):
    k, cb, mean, scale = _lookup_inputs(gpu, D, K, S)
    ms = (mean, scale) if stats else (None, None)
    ids = k + K * torch.arange(S).view(-1, 1)
    ref = _existing_lookup(gpu, ids, cb, dtype, ms)
    packed = WR.pack(k, K)
    fb = packed.shape[1]
    B = LK_ROWS // LK_T
    for count in COUNTS:
        out, idx_out = _lookup_wire(gpu, packed.to(gpu), cb, S, dtype, ms, count)
        live = _active(count, B) * LK_T
        assert torch.equal(out[:live], ref[:live]), (count, (out[:live] != ref[:live]).nonzero()[:6].tolist())
        assert bool(torch.isnan(out[live:].float()).all()), count
        assert torch.equal(idx_out[:, :live].cpu(), ids[:, :live]) and bool((idx_out[:, live:] == -7).all()), count
    out, none = _lookup_wire(gpu, packed.to(gpu), cb, S, dtype, ms, with_idx=False)
    assert none is None and torch.equal(out, ref)
    # a view that starts one byte into its allocation
    pad = torch.zeros(LK_ROWS * fb + 1, dtype=torch.uint8, device=gpu)
    view = pad[1:].view(LK_ROWS, fb)
    view.copy_(packed)
    assert view.data_ptr() % 2 == 1
    out, idx_out = _lookup_wire(gpu, view, cb, S, dtype, ms)
    assert torch.equal(out, ref) and torch.equal(idx_out.cpu(), ids)
    # all-ones pad bits
    dirty = WR.set_pad_bits(packed, S, K)
    assert (8 * fb == S * WR.bits_of(K)) == torch.equal(dirty, packed)
    out, idx_out = _lookup_wire(gpu, dirty.to(gpu), cb, S, dtype, ms)
    assert torch.equal(out, ref) and torch.equal(idx_out.cpu(), ids)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lookup_wire_refuses_a_field_beyond_K(gpu, dtype):
    """K = 1000, field value 1023 in stage 1 of 3: s * K + 1023 lies inside the
    codebook (stage 2's rows), so only the guard keeps it out of the sum."""
    from sel import streamops as SO
    D, K, S, bad = 64, 1000, 3, 1
    k, cb, _, _ = _lookup_inputs(gpu, D, K, S)
    assert WR.bits_of(K) == 10 and bad != S - 1 and bad * K + 1023 < S * K
    recs = []
    for r in range(LK_ROWS):
        rec = 0
        for s in range(S):
            rec |= (1023 if s == bad else int(k[s, r])) << (10 * s)
        recs.append(list(rec.to_bytes(WR.frame_bytes(S, K), "little")))
    wire = torch.tensor(recs, dtype=torch.uint8)
    assert torch.equal(WR.unpack(wire, S, K)[bad], torch.full((LK_ROWS,), -1))
    out, idx_out = _lookup_wire(gpu, wire.to(gpu), cb, S, dtype, (None, None))
    # the sum without that stage: sel_rvq_lookup_step with an id it refuses itself (-1)
    ids = k + K * torch.arange(S).view(-1, 1)
    ids[bad] = -1
    ref = torch.full((LK_ROWS, D), float("nan"), dtype=dtype, device=gpu)
    SO.rvq_lookup_step(ids.to(gpu), cb, ref, LK_T)
    torch.cuda.synchronize()
    two = (cb[ids[0].to(gpu)] + cb[ids[2].to(gpu)]).to(dtype)         # and the same two rows added by torch
    assert torch.equal(ref, two)
    assert torch.equal(out, ref) and torch.equal(idx_out.cpu(), ids)


# ---------------------------------------------------------------------------
# C. the bindings refuse bad operands before any launch
# ---------------------------------------------------------------------------
def test_wire_bindings_refuse_bad_operands(gpu):
    from sel import _lib as L
    from sel import streamops as SO
    z = torch.zeros(4, 8, device=gpu)
    e = torch.zeros(2, 8, 16, device=gpu)                     # S = 2, K = 16: one byte per record
    idx = torch.zeros(2, 4, dtype=torch.int64, device=gpu)
    wire = torch.zeros(4, 1, dtype=torch.uint8, device=gpu)
    wide = torch.zeros(4, 2, dtype=torch.uint8, device=gpu)
    for bad in (dict(z=z.cpu()), dict(z=z.bfloat16()), dict(z=z[:, :4]), dict(embeds=e.bfloat16()), dict(embeds=e[0]),
                dict(idx=idx.int()), dict(idx=idx[:, :3]), dict(zq=z.bfloat16()), dict(zq=z[:2]),
                dict(rows_per_sample=3), dict(n_active=torch.zeros(1, device=gpu)),
                dict(wire=None), dict(wire=wire.cpu()), dict(wire=wire.int()), dict(wire=wide), dict(wire=wire[:3]),
                dict(wire=wide[:, :1]), dict(wire=wire.view(4))):
        a = dict(z=z, embeds=e, wire=wire, idx=idx)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_step_wire(**a)
    cb = torch.zeros(32, 8, device=gpu)
    out = torch.zeros(4, 8, device=gpu)
    m = torch.zeros(8, device=gpu)
    for bad in (dict(wire=wire.cpu()), dict(wire=wire.int()), dict(wire=wide), dict(wire=wide[:, :1]),
                dict(wire=wire.view(4)), dict(codebook=cb.bfloat16()), dict(codebook=cb[:, :4]), dict(codebooks=3),
                dict(codebooks=0), dict(out=out.half()), dict(out=out[:2]), dict(mean=m), dict(scale=m),
                dict(mean=m[:4], scale=m), dict(rows_per_sample=3), dict(n_active=torch.zeros(1, device=gpu)),
                dict(idx_out=idx.int()), dict(idx_out=idx[:, :3])):
        a = dict(wire=wire, codebook=cb, codebooks=2, out=out)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_lookup_wire_step(**a)
