"""CPU checks of the streaming RVQ step kernels' host side and of the cases of
tests/test_gpu_rvq_step.py: every refusal of sel_rvq_step / sel_rvq_lookup_step
through ctypes (SEL_ERR_ARG before any device work: the pointers below are never
dereferenced), that each case reaches the edge it is named for, and that the
fp32 restatement of the contract (tests/rvq_step_ref.py) passes the fp64 pick
check of tests/rvq_cases.py on inputs in which little can hide."""
import ctypes

import pytest
import torch

import rvq_cases as C
import rvq_step_ref as SR

SEL_ERR_ARG = -1
P = ctypes.c_void_p(0x1000)      # a non-null pointer no refused call may touch
NULL = None


def _lib():
    from sel import _lib
    return _lib.load()


def _step(**kw):
    a = dict(z=P, rows=4, T=2, D=64, embeds=P, S=8, K=1024, n_active=NULL, flatten=1, idx=P, zq=NULL)
    a.update(kw)
    return _lib().sel_rvq_step(a["z"], a["rows"], a["T"], a["D"], a["embeds"], a["S"], a["K"], a["n_active"],
                               a["flatten"], a["idx"], a["zq"], None)


def _lookup(**kw):
    a = dict(idx=P, rows=4, T=2, S=8, ncodes=8192, D=64, codebook=P, mean=NULL, scale=NULL, n_active=NULL,
             out_dtype=0, out=P)
    a.update(kw)
    return _lib().sel_rvq_lookup_step(a["idx"], a["rows"], a["T"], a["S"], a["ncodes"], a["D"], a["codebook"],
                                      a["mean"], a["scale"], a["n_active"], a["out_dtype"], a["out"], None)


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(T=-2), dict(rows=5, T=2), dict(D=0), dict(D=-1), dict(D=257),
    dict(K=0), dict(K=-1), dict(S=0), dict(S=-1), dict(z=NULL), dict(embeds=NULL), dict(idx=NULL),
    dict(zq=P),          # zq aliases z
], ids=lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"
                          for k, v in b.items()))
def test_rvq_step_refuses(bad):
    lib = _lib()
    assert _step(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_step" in lib.sel_last_error()


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(rows=5, T=2), dict(S=0), dict(S=-1), dict(D=0), dict(D=-3),
    dict(ncodes=0), dict(ncodes=-1), dict(ncodes=1 << 40, D=256), dict(idx=NULL), dict(codebook=NULL),
    dict(out=NULL), dict(mean=P), dict(scale=P), dict(out_dtype=2), dict(out_dtype=-1),
    dict(rows=(1 << 31) - 1, T=1, D=1 << 20),
], ids=lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"
                          for k, v in b.items()))
def test_rvq_lookup_step_refuses(bad):
    lib = _lib()
    assert _lookup(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_lookup_step" in lib.sel_last_error()


@pytest.mark.parametrize("name", list(SR.CASES))
def test_case_reaches_its_edge(name):
    print(name, SR.CASES[name], SR.check_properties(name))


def test_every_instance_and_every_listed_edge_is_covered():
    assert {SR.instance_of(c) for c in SR.CASES.values()} == {"col", "any"}
    for shape in ((1, 1, 64, 1024, 8), (1, 1, 4, 1, 1), (5, 1, 60, 1000, 3), (3, 3, 255, 37, 2),
                  (2, 1, 256, 2050, 2), (64, 4, 64, 1024, 8), (2, 2, 8, 16, 17)):
        assert shape in SR.CASES.values(), shape
    assert SR.unique_of("dup") == SR.unique_of("dup_col") == C.NDUP and SR.unique_of("hop") is None


_PICKS = {}


def restated(name):
    if name not in _PICKS:
        z, embeds = SR.inputs(name)
        _PICKS[name] = SR.rvq_step(z, embeds)
    return _PICKS[name]


@pytest.mark.parametrize("name", list(SR.CASES))
def test_restatement_passes_fp64_and_little_can_hide(name):
    rows, T, D, K, S = SR.CASES[name]
    z, embeds = SR.inputs(name)
    assert z.dtype == embeds.dtype == torch.float32 and tuple(z.shape) == (rows, D)
    assert tuple(embeds.shape) == (S, D, K)
    idx, zq = restated(name)
    r = C.check_picks(z, embeds, idx, SR.unique_of(name))
    print(f"{name}: pairs {r['pairs']} worst gap/allowed {r['worst']:.3e} hide share {100 * r['hide']:.3f} %")
    assert r["pairs"] == rows * S and r["nbad"] == 0 and r["out_of_range"] == 0, r["bad"]
    assert r["worst"] <= 1.0
    assert r["hide"] <= C.hide_cap(r["pairs"]), r["hide"]
    # zq is the sum of the picked codes up to the update's rounding (four roundings per stage)
    o = C.restate(z, embeds, idx)[0]
    assert C.rel(zq, o) <= 1e-6


def test_restatement_flatten_and_ties():
    z, embeds = SR.inputs("dup")
    K = embeds.shape[2]
    idx, _ = restated("dup")
    flat, _ = SR.rvq_step(z, embeds, flatten=True)
    assert torch.equal(flat, idx + K * torch.arange(idx.shape[0]).view(-1, 1))
    assert int(idx.max()) < C.NDUP                       # the lowest of the bit-equal columns


def test_ordered_lookup_is_the_stage_sum():
    g = torch.Generator().manual_seed(5)
    cb = torch.randn(24, 3, generator=g)
    idx = torch.randint(0, 24, (8, 7), generator=g)
    ref = cb.double()[idx].sum(0)
    got = SR.ordered_lookup(idx, cb)
    assert got.dtype == torch.float32 and C.rel(got, ref) < 1e-6
    mean, scale = torch.randn(3, generator=g), torch.rand(3, generator=g) + 0.5
    assert C.rel(SR.ordered_lookup(idx, cb, mean, scale), (ref - mean.double()) / scale.double()) < 1e-6
