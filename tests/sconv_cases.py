"""Cases and CPU references of the channels-last 2-D conv kernels (sconv2d.hip),
shared by tests/test_gpu_univnet.py, tests/test_gpu_sconv_edges.py and
tests/test_sconv_cases_host.py.  A plain helper: nothing here needs a GPU.

Three things live here:
  * the layer cases, (B, H, W, Cin, Cout, kernel, stride) tuples, and the
    weight-gradient split arithmetic of the library restated (wg_ranges), so
    that the shape property of every case is asserted, not assumed;
  * layer_ref: random-valued inputs and the fp64 F.conv2d reference;
  * exact_case: inputs for which every product and every partial sum, in any
    order, is exactly representable in fp32, so that the kernels' outputs are
    compared bit for bit in fp32 and in bf16.
"""
import numpy as np
import torch
import torch.nn.functional as F

TILE = 64  # output columns per block of the matrix-core kernels (sconv2d.hip BM)
SLOPE = 0.2
EXACT_SLOPE = 0.25  # a power of two: v * slope never changes v's significand

# (B, H, W, Cin, Cout, kernel, stride)
LAYER_CASES = {
    "s2_odd_tail": (3, 4, 40, 32, 32, (3, 9), (1, 2)),    # W - kw odd: the last input column is read by no tap
    "s1": (3, 4, 40, 32, 32, (3, 9), (1, 1)),
    "one_row": (2, 3, 11, 32, 32, (3, 3), (1, 1)),        # one output row, fewer columns than a tile
    "tile_plus": (2, 5, 2 * (TILE + 13 - 1) + 9, 32, 32, (3, 9), (1, 2)),  # output width TILE + 13
    "first": (3, 5, 21, 1, 32, (3, 9), (1, 1)),
    "last": (3, 4, 13, 32, 1, (3, 3), (1, 1)),
    "c64": (2, 4, 24, 64, 64, (3, 9), (1, 2)),
}

# The shapes are the smallest that reach the named path; the properties are
# asserted by check_properties below (host test and GPU test alike).
EDGE_CASES = {
    # R = 200 rows over 128 splits: 1 or 2 rows each; split 51 = rows [79, 81) holds
    # the last row of sample 1 and the first of sample 2
    "wg_rows_2": (5, 42, 20, 32, 32, (3, 9), (1, 1)),
    # R = 3 * 128 + 6 (3 * 128 + 5 = 389 is prime, so it has no B > 1 factorisation):
    # 3 or 4 rows per split, Ho = 130 is no multiple of 3, output width TILE + 13
    "wg_rows_3_tiles": (3, 132, 2 * (TILE + 13 - 1) + 9, 32, 32, (3, 9), (1, 2)),
    "wg_first_rows": (3, 514, 12, 1, 32, (3, 9), (1, 1)),     # R = 1536 over 1024 splits
    "wg_last_rows": (3, 514, 5, 32, 1, (3, 3), (1, 1)),       # R = 1536 over 1024 splits
    "cin_lt_cout": (2, 4, 24, 32, 64, (3, 9), (1, 2)),
    "cin_gt_cout": (2, 4, 24, 64, 32, (3, 9), (1, 2)),
    "c96": (2, 4, 11, 96, 32, (3, 3), (1, 1)),
    "c256": (1, 4, 12, 256, 256, (3, 3), (1, 1)),             # the accepted maximum
    "k1x1": (2, 3, 11, 32, 32, (1, 1), (1, 1)),
    "k2x4_s2": (2, 4, 2 * (TILE + 6 - 1) + 4 + 1, 32, 32, (2, 4), (1, 2)),   # W - 4 odd, output width TILE + 6
    "k1x2_s2": (2, 3, 23, 32, 32, (1, 2), (1, 2)),            # kw == sw; W - 2 odd: an unread column too
    "single_position": (2, 3, 9, 32, 32, (3, 9), (1, 2)),
    "first_k2x4_s2": (2, 4, 21, 1, 32, (2, 4), (1, 2)),       # W - 4 odd: the last input column unread
    "last_k1x1": (2, 3, 11, 32, 1, (1, 1), (1, 1)),
    "s2_even_tail": (3, 4, 41, 32, 32, (3, 9), (1, 2)),       # the complement of s2_odd_tail
}

# the cases of the bit-for-bit comparison
EXACT_CASES = {k: EDGE_CASES[k] for k in ("wg_rows_2", "wg_rows_3_tiles", "cin_lt_cout", "cin_gt_cout", "k2x4_s2",
                                          "wg_first_rows", "wg_last_rows", "c96", "c256", "k1x2_s2",
                                          "single_position", "first_k2x4_s2", "last_k1x1")}
EXACT_CASES["tile_plus"] = LAYER_CASES["tile_plus"]


def rel(a, b):
    a = a.detach().double().cpu()
    b = torch.as_tensor(np.asarray(b)).double() if not torch.is_tensor(b) else b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _cl(t):
    """(B, C, H, W) -> channels-last rows (B, H, W, C)"""
    return t.permute(0, 2, 3, 1).contiguous()


def out_hw(case):
    B, H, W, ci, co, k, s = case
    return H - k[0] + 1, (W - k[1]) // s[1] + 1


# ---------------------------------------------------------------------------
# the weight gradient's row splits, restated from the kernel's comments: nsplit =
# min(B * Ho, cap), cap 128 for C -> C and 1024 for the 1-channel ends; split s
# walks the rows [R s / nsplit, R (s + 1) / nsplit) of the R = B * Ho output rows
# ---------------------------------------------------------------------------
def wg_ranges(case):
    B, H, W, ci, co, k, s = case
    Ho, _ = out_hw(case)
    R = B * Ho
    cap = 1024 if ci == 1 or co == 1 else 128
    n = min(R, cap)
    return R, cap, [(R * i // n, R * (i + 1) // n) for i in range(n)]


def boundary_inside_split(case):
    """a split [lo, hi) with lo < b * Ho < hi: rows of two samples in one block"""
    Ho, _ = out_hw(case)
    _, _, rng = wg_ranges(case)
    return any(lo < m < hi for lo, hi in rng for m in range(Ho, case[0] * Ho, Ho))


def check_properties(name, case):
    """The shape property a case is named for, from the shape arithmetic alone."""
    B, H, W, ci, co, k, s = case
    Ho, Wo = out_hw(case)
    R, cap, rng = wg_ranges(case)
    rows = sorted({hi - lo for lo, hi in rng})
    assert rng[0][0] == 0 and rng[-1][1] == R and all(a[1] == b[0] for a, b in zip(rng, rng[1:]))
    if name == "wg_rows_2":
        assert (ci, co, k, s) == (32, 32, (3, 9), (1, 1)) and R == 200 and rows == [1, 2]
        assert boundary_inside_split(case)
    elif name == "wg_rows_3_tiles":
        assert (ci, co, k, s) == (32, 32, (3, 9), (1, 2)) and B == 3 and Ho % 3 != 0
        assert 3 * cap < R < 4 * cap and R % cap != 0 and rows == [3, 4] and boundary_inside_split(case)
        assert Wo == TILE + 13                                   # two column tiles, the second partial
    elif name in ("wg_first_rows", "wg_last_rows"):
        assert (ci, co, k, s) == ((1, 32, (3, 9), (1, 1)) if name == "wg_first_rows" else (32, 1, (3, 3), (1, 1)))
        assert cap == 1024 and R > cap and R % cap != 0 and rows == [1, 2] and boundary_inside_split(case)
    elif name == "cin_lt_cout":
        assert (ci, co, k, s) == (32, 64, (3, 9), (1, 2))
    elif name == "cin_gt_cout":
        assert (ci, co, k, s) == (64, 32, (3, 9), (1, 2))
    elif name == "c96":
        assert (ci, co, k, s) == (96, 32, (3, 3), (1, 1))
    elif name == "c256":
        assert (ci, co, k, s) == (256, 256, (3, 3), (1, 1)) and B * Ho * Wo <= 64
    elif name == "k1x1":
        assert (ci, co, k, s) == (32, 32, (1, 1), (1, 1))
    elif name == "k2x4_s2":
        assert (ci, co, k, s) == (32, 32, (2, 4), (1, 2)) and (W - 4) % 2 == 1
        assert TILE < Wo < 2 * TILE                              # both phases of the data gradient cross a tile edge
        assert all((k[1] - p + 1) // 2 == 2 for p in (0, 1))     # even kw at stride 2: equal Kp
    elif name == "k1x2_s2":
        assert (ci, co, k, s) == (32, 32, (1, 2), (1, 2)) and k[1] == s[1] and (W - 2) % 2 == 1
        assert all((k[1] - p + 1) // 2 == 1 for p in (0, 1))     # one tap per column phase
    elif name == "single_position":
        assert (ci, co, k, s) == (32, 32, (3, 9), (1, 2)) and (H, W) == k and (Ho, Wo) == (1, 1)
    elif name == "first_k2x4_s2":
        assert (ci, co, k, s) == (1, 32, (2, 4), (1, 2)) and (W - 4) % 2 == 1
    elif name == "last_k1x1":
        assert (ci, co, k, s) == (32, 1, (1, 1), (1, 1))
    elif name == "s2_even_tail":
        assert (ci, co, k, s) == (32, 32, (3, 9), (1, 2)) and (W - 9) % 2 == 0
    elif name == "s2_odd_tail":
        assert (W - k[1]) % 2 == 1
    elif name == "tile_plus":
        assert Wo == TILE + 13
    else:
        raise KeyError(name)
    return dict(R=R, cap=cap, rows=rows, Ho=Ho, Wo=Wo)


# ---------------------------------------------------------------------------
# random-valued reference
# ---------------------------------------------------------------------------
_REF = {}


def layer_ref(name, case):
    """fp64 CPU reference of one case, computed once and shared by both precisions."""
    key = (name, case)
    if key in _REF:
        return _REF[key]
    B, H, W, ci, co, k, s = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    leaky = co != 1
    u = torch.randn(B, ci, H, W, generator=g)
    x = F.leaky_relu(u, SLOPE) if ci != 1 else u.abs()        # a stored LeakyReLU output / magnitudes
    w = torch.randn(co, ci, *k, generator=g) / (ci * k[0] * k[1]) ** 0.5
    b = 0.1 * torch.randn(co, generator=g)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    z = F.conv2d(xd, wd, bd, stride=s)
    gpre = torch.randn(z.shape, generator=g)
    (z * gpre.double()).sum().backward()
    gx = xd.grad * torch.where(x > 0, 1.0, SLOPE).double() if ci != 1 else xd.grad
    y = F.leaky_relu(z, SLOPE) if leaky else z
    _REF[key] = dict(x=x, w=w, b=b, gpre=gpre, y=y.detach(), gx=gx, gw=wd.grad, gb=bd.grad, leaky=leaky)
    return _REF[key]


def abs_conv(r, case):
    """A = conv2d(|x|, |w|, |b|) in fp64: the scale of the forward's per-element
    rounding bound (n + 2) 2^-24 A + 2^-23 |ref|, n = kh kw Cin."""
    if "A" not in r:
        r["A"] = F.conv2d(r["x"].double().abs(), r["w"].double().abs(), r["b"].double().abs(), stride=case[6])
    return r["A"]


# ---------------------------------------------------------------------------
# exact-arithmetic cases
# ---------------------------------------------------------------------------
def _ints(g, shape, lo, hi, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        v = torch.where(v == 0, torch.randint(0, 2, shape, generator=g) * 2 - 1, v)
    return v.double()


def _bf(t):
    """round to nearest even into bf16, returned in fp64"""
    return t.float().to(torch.bfloat16).double()


def _lgrad(x, slope):
    """sconv2d.hip leaky_grad: y > 0 ? 1 : slope (0 is excluded from x anyway)"""
    return torch.where(x > 0, 1.0, slope).double()


_EXACT = {}


def exact_case(name, case):
    """Inputs and bit-exact references of one case; every condition that makes the
    comparison bit for bit legitimate is asserted here, on the CPU, before
    anything is compared.  All tensors are fp64 holding fp32- (and where stated
    bf16-) representable values, in the torch layout (B, C, H, W).

    x, gy     integers in [-2, 2]; x without 0 where it has channels (it is the
              LeakyReLU' argument of the data gradient), magnitudes in [0, 2]
              for the 1-channel input
    wf        forward weights k 2^-12, |k| < 2^12 (2^11 for Cin >= 64): up to 13
              significant bits, two bf16 terms hold them and one cannot
    wa        data-gradient weights k 2^-7, |k| <= 127: one bf16 term
    b         multiples of 2^-4, |b| <= 4
    y32/y16   leaky(exact sum + bias) and its bf16 rounding (fp32 for Cout = 1)
    gx32/gx16 exact * leaky'(x) and its bf16 rounding (fp32 for Cin = 1)
    gw, gb    exact in both precisions"""
    key = (name, case)
    if key in _EXACT:
        return _EXACT[key]
    B, H, W, ci, co, k, s = case
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    sl = EXACT_SLOPE
    leaky = co != 1
    mid = ci != 1 and co != 1
    x = _ints(g, (B, ci, H, W), -2, 2, nonzero=True) if ci != 1 else _ints(g, (B, ci, H, W), 0, 2)
    kmax = 2 ** 11 if ci >= 64 else 2 ** 12
    wf = _ints(g, (co, ci, *k), -(kmax - 1), kmax - 1) * 2.0 ** -12
    wa = _ints(g, (co, ci, *k), -127, 127) * 2.0 ** -7
    b = _ints(g, (co,), -64, 64) * 2.0 ** -4
    Ho, Wo = out_hw(case)
    gy = _ints(g, (B, co, Ho, Wo), -2, 2)

    # forward
    z = F.conv2d(x, wf, b, stride=s)
    y = F.leaky_relu(z, sl) if leaky else z
    cap_f = float(F.conv2d(x.abs(), wf.abs(), b.abs(), stride=s).max())
    assert cap_f * 2 ** 12 < 2 ** 24, (name, cap_f)
    assert torch.equal(y.float().double(), y)
    hi = _bf(wf)
    lo = _bf(wf - hi)
    if mid:
        assert torch.equal(hi + lo, wf), name                     # the two-term identity
        assert not torch.equal(hi, wf)
    y16 = _bf(y) if leaky else y
    sens = None
    if mid:
        z1 = F.conv2d(x, hi, b, stride=s)
        sens = float((_bf(F.leaky_relu(z1, sl)) != y16).double().mean())
        assert sens >= 0.25, (name, sens)                         # a dropped second term cannot hide

    # gradients (the weight gradient does not depend on the weights)
    xd = x.clone().requires_grad_(True)
    wd = wa.clone().requires_grad_(True)
    bd = b.clone().requires_grad_(True)
    (F.conv2d(xd, wd, bd, stride=s) * gy).sum().backward()
    gx = xd.grad * _lgrad(x, sl) if ci != 1 else xd.grad
    xa = x.abs().requires_grad_(True)
    waa = wa.abs().requires_grad_(True)
    (F.conv2d(xa, waa, None, stride=s) * gy.abs()).sum().backward()
    cap_d, cap_w = float(xa.grad.max()), float(waa.grad.max())
    assert cap_d * 2 ** 7 < 2 ** 24 and cap_w < 2 ** 24, (name, cap_d, cap_w)
    assert float(gy.abs().sum(dim=(0, 2, 3)).max()) < 2 ** 24
    assert torch.equal(_bf(wa), wa)
    for t in (gx, wd.grad, bd.grad):
        assert torch.equal(t.float().double(), t)
    gx16 = _bf(gx) if ci != 1 else gx
    _EXACT[key] = dict(x=x, wf=wf, wa=wa, b=b, gy=gy, y32=y.detach(), y16=y16.detach(), gx32=gx.detach(),
                       gx16=gx16.detach(), gw=wd.grad, gb=bd.grad, leaky=leaky, sens=sens,
                       caps=dict(fwd=cap_f * 2 ** 12 / 2 ** 24, gx=cap_d * 2 ** 7 / 2 ** 24, gw=cap_w / 2 ** 24))
    return _EXACT[key]


def describe_mismatch(kind, got, ref, case, limit=6):
    """The first few mismatching elements of a channels-last (B, H, W, C) output
    (or of gw (Cout, Cin, kh, kw)) with the tile and phase they fall in."""
    bad = (got != ref).nonzero()
    lines = [f"{kind}: {bad.shape[0]} of {ref.numel()} elements differ"]
    sw = case[6][1]
    for idx in bad[:limit].tolist():
        t = tuple(idx)
        if kind == "gw":
            where = f"n {t[0]} c {t[1]} tap ({t[2]}, {t[3]}) channel blocks ({t[1] // 32}, {t[0] // 32})"
        elif kind == "gb":
            where = f"n {t[0]}"
        else:
            col = t[2]
            step = sw if kind == "gx" else 1                       # the data gradient runs one launch per column phase
            where = (f"sample {t[0]} row {t[1]} column {col} channel {t[3]}: tile {(col // step) // TILE}"
                     f" lane {(col // step) % TILE} phase {col % step} channel block {t[3] // 32}")
        lines.append(f"  {where}: got {float(got[t])!r} want {float(ref[t])!r}")
    return "\n".join(lines)
