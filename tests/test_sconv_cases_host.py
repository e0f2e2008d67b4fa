"""CPU checks of the cases of tests/test_gpu_sconv_edges.py: that every case has
the shape property it is named for (rows per weight-gradient split, a sample
boundary inside a split, tail parities, tile remainders: the split arithmetic is
restated in tests/sconv_cases.py, not read from the library), that the library
accepts every case, and that the exact-arithmetic cases are exact: their caps,
the two-term bf16 identity of the forward weights, the sensitivity of the bf16
forward to a dropped second term, and fp32 F.conv2d equal to fp64 F.conv2d bit
for bit, also with the channel order (the summation order) permuted."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import sconv_cases as C


@pytest.mark.parametrize("name", list(C.EDGE_CASES) + ["s2_odd_tail", "tile_plus"])
def test_case_has_its_shape_property(name):
    case = C.EDGE_CASES.get(name) or C.LAYER_CASES[name]
    p = C.check_properties(name, case)
    print(name, p)
    assert p["R"] == case[0] * (case[1] - case[5][0] + 1)


def test_split_properties_by_hand():
    """The restated split arithmetic at the values the case comments quote."""
    R, cap, rng = C.wg_ranges(C.EDGE_CASES["wg_rows_2"])
    assert (R, cap, len(rng)) == (200, 128, 128) and rng[51] == (79, 81) and 79 < 2 * 40 < 81
    R, cap, rng = C.wg_ranges(C.EDGE_CASES["wg_rows_3_tiles"])
    assert (R, cap) == (3 * 128 + 6, 128) and rng[42] == (127, 131) and 127 < 130 < 131
    for name in ("wg_first_rows", "wg_last_rows"):
        R, cap, rng = C.wg_ranges(C.EDGE_CASES[name])
        assert (R, cap, len(rng)) == (1536, 1024, 1024) and rng[341] == (511, 513)
    # every case of the existing layer suite has one row per split: the gap these cases close
    for name, case in C.LAYER_CASES.items():
        R, cap, rng = C.wg_ranges(case)
        assert R <= 9 and all(hi - lo == 1 for lo, hi in rng), name
    # the example shape B = 4, Ho = 50 puts every sample boundary on a split edge
    assert not C.boundary_inside_split((4, 52, 20, 32, 32, (3, 9), (1, 1)))


@pytest.mark.parametrize("name", list(C.EDGE_CASES))
def test_library_accepts_every_case(name):
    from sel import _lib
    from sel import sconvops as SC
    B, H, W, ci, co, k, s = C.EDGE_CASES[name]
    sp = SC.LayerSpec(ci, co, k, s, co != 1)
    for slope in (C.SLOPE, C.EXACT_SLOPE):
        d = sp.desc(B, H, W, slope)
        assert _lib.load().sel_sconv_check(ctypes.byref(d)) == 0, _lib.load().sel_last_error()


@pytest.mark.parametrize("name", list(C.EXACT_CASES))
def test_exact_case_conditions(name):
    case = C.EXACT_CASES[name]
    B, H, W, ci, co, k, s = case
    e = C.exact_case(name, case)          # asserts the caps, the two-term identity and the sensitivity
    print(name, {k_: f"{v:.3f}" for k_, v in e["caps"].items()}, "sensitivity", e["sens"])
    assert all(v < 1.0 for v in e["caps"].values())
    if ci != 1 and co != 1:
        assert e["sens"] >= 0.25
    # fp32 arithmetic on these inputs is exact in whatever order it sums
    perm = torch.randperm(ci, generator=torch.Generator().manual_seed(5))
    z64 = F.conv2d(e["x"], e["wf"], e["b"], stride=s)
    for xx, ww in ((e["x"], e["wf"]), (e["x"][:, perm], e["wf"][:, perm])):
        z32 = F.conv2d(xx.float(), ww.float(), e["b"].float(), stride=s)
        assert torch.equal(z32.double(), z64)
    y = F.leaky_relu(z64, C.EXACT_SLOPE) if e["leaky"] else z64
    assert torch.equal(y, e["y32"])
    xf = e["x"].float().requires_grad_(True)
    wf = e["wa"].float().requires_grad_(True)
    bf = e["b"].float().requires_grad_(True)
    (F.conv2d(xf, wf, bf, stride=s) * e["gy"].float()).sum().backward()
    gx = xf.grad.double() * (C._lgrad(e["x"], C.EXACT_SLOPE) if ci != 1 else 1.0)
    assert torch.equal(gx, e["gx32"])
    assert torch.equal(wf.grad.double(), e["gw"]) and torch.equal(bf.grad.double(), e["gb"])
    # the inputs are what they are said to be
    assert set(e["x"].unique().tolist()) <= ({-2.0, -1.0, 1.0, 2.0} if ci != 1 else {0.0, 1.0, 2.0})
    assert set(e["gy"].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert torch.equal(e["x"].float().to(torch.bfloat16).double(), e["x"])
    assert float(e["b"].abs().max()) <= 4 and torch.equal((e["b"] * 16).round(), e["b"] * 16)
