"""The 1-D conv primitive (csrc/conv.hip, csrc/conv_wss.hip and its weight
gradients, csrc/conv_wgrad.hip) against fp64 at its tile and dispatch edges: every case of tests/conv_cases.py through sel_conv_fwd
in each of its output dtypes with its epilogue operands, and every
weight-gradient case through sel_conv_wgrad (or sel_conv_wgrad_unpacked), each
held element by element to the bounds derived in that module's docstring.  A
test first asserts the kernel its case is there for (the library's own
reporter; the restated plan for the weight gradients), then runs under the
case's tune settings, which it restores.  Forward outputs go into a prefilled
buffer with a guard tail: every element must be written, none beyond rows x N."""
import ctypes

import pytest
import torch

import conv_cases as C

pytestmark = pytest.mark.gpu

_SLOT = {}  # the operands and the reference of ONE case, shared by its tests


def _setup(gpu, name):
    if _SLOT.get("name") != name:
        _SLOT.clear()
        case = C.BY_NAME[name]
        ops = C.operands(case, gpu)
        _SLOT.update(name=name, ops=ops, ref=C.reference(case, ops))
    return _SLOT["ops"], _SLOT["ref"]


def _run(case, ops, tdt, settings):
    """sel_conv_fwd of a case into a prefilled buffer under `settings`; the
    output, after checking that the guard tail kept its fill."""
    from sel import _lib as L
    from sel import convops as CO
    x, wp, b, a_, r_ = ops
    d = case.d
    n = d.rows * d.N
    buf = torch.full((n + C.GUARD,), C.OUT_FILL, dtype=tdt, device=x.device)
    with C.tuned(L.lib(), settings):
        CO.prim(d, x, wp, bias=b, aux=a_.to(tdt) if a_ is not None else None,
                res=r_.to(tdt) if r_ is not None else None, out=buf[:n].view(d.rows, d.N))
    torch.cuda.synchronize()
    assert bool((buf[n:] == C.OUT_FILL).all()), (case.name, "written past rows x N")
    return buf[:n].view(d.rows, d.N)


@pytest.mark.parametrize("name,dt", [(c.name, dt) for c in C.CASES for dt in c.dtypes])
def test_forward_edge_case(gpu, name, dt):
    from sel import _lib as L
    case = C.BY_NAME[name]
    lib = L.lib()
    before = [lib.sel_tune_get(k) for k in (0, 4, 42, 51)]
    got_name = C.kernel_name(case, dt)
    assert got_name.startswith(case.kernel) if case.family == "gen" else got_name == case.name_for(dt), got_name
    ops, ref = _setup(gpu, name)
    tdt = C.F32 if dt == "f32" else C.BF16
    got = _run(case, ops, tdt, case.tune)
    C.check_output(case, dt, got, ref, f"{name} {dt} ({got_name})")
    if case.family in ("ws8", "ws8w"):
        # the eight-wave kernels keep the 12-wave kernel's (chunk, tap) MFMA order per output: same bits
        assert torch.equal(got, _run(case, ops, tdt, {**case.tune, 0: 27})), (name, dt)
    assert [lib.sel_tune_get(k) for k in (0, 4, 42, 51)] == before


def _wgrad_run(case, g, x):
    from sel import _lib as L
    from sel import convops as CO
    lib = L.lib()
    d = case.d
    with C.tuned(lib, case.tune):
        if case.unpack is None:
            gw, gb = CO.wgrad(d, g, x, bool(d.bias_period))
        else:
            kind, cout, cin, k, stride = case.unpack
            shape = (cin, cout, k) if kind == CO.PACK_CONVT else (cout, cin, k)
            ws = L.workspace(lib.sel_conv_wgrad_workspace(ctypes.byref(d)), x.device)
            gw = torch.full(shape, C.OUT_FILL, dtype=torch.float32, device=x.device)
            gb = torch.full((d.bias_period,), C.OUT_FILL, dtype=torch.float32, device=x.device) if d.bias_period else None
            L.call("sel_conv_wgrad_unpacked", ctypes.byref(d), CO._code(x.dtype), L.ptr(g), L.ptr(x), kind, cout, cin,
                   k, stride, L.ptr(gw), L.ptr(gb), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return gw, gb


@pytest.mark.parametrize("name", [c.name for c in C.WGRAD_CASES])
def test_wgrad_edge_case(gpu, name):
    from sel import _lib as L
    case = C.W_BY_NAME[name]
    lib = L.lib()
    d = case.d
    before = [lib.sel_tune_get(k) for k in (1, 10, 54, 62)]
    plan = C.wgrad_plan(d, C.wgrad_mode(d, case.bf16, case.tune), case.tune)
    assert {k: plan[k] for k in case.plan} == case.plan and C.wgrad_kernel(d, case.bf16, case.tune) == case.kernel
    assert C.wgrad_workspace(d) == int(lib.sel_conv_wgrad_workspace(ctypes.byref(d)))
    g, x = C.wgrad_operands(case, gpu)
    ref = C.wgrad_reference(case, g, x)
    gw, gb = _wgrad_run(case, g, x)
    want, S, slack = ref["gw"], ref["S_gw"], ref["slack"]
    if case.unpack is not None:
        un = lambda t: C.unpack_ref(*((case.unpack[0], t) + case.unpack[1:]))  # noqa: E731
        want, S = un(want), un(S)
        assert not torch.isnan(want).any()      # every torch weight element has a packed source
    n, ns = d.rows, plan["nsplit"]
    C.check_wgrad(gw, want, S, n, ns, f"{name} weight gradient ({case.kernel})", slack)
    if d.bias_period:
        C.check_wgrad(gb, ref["gb"], ref["S_gb"], n * (d.N // d.bias_period), ns, f"{name} bias gradient")
    assert [lib.sel_tune_get(k) for k in (1, 10, 54, 62)] == before
