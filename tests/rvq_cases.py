"""Cases and fp64 CPU references of the residual-VQ kernels (vq.hip), shared by
tests/test_gpu_rvq_edges.py and tests/test_rvq_cases_host.py.  A plain helper:
nothing here needs a GPU.

Three things live here:
  * the cases, (N, D, K, S) tuples, each the smallest shape that reaches one
    path of the forward dispatch, and that dispatch's arithmetic restated
    (properties / kernel_of), so that the property of every case is asserted,
    not assumed;
  * check_picks: the fp64 reference of the code picks, chained on the picks it
    is given, with a derived rounding bound (below);
  * restate / grad_closed: out, losses, perplexities, counts and the input
    gradient in fp64 from given picks.

The bound.  For stage s, row residual r (fp64, r_0 = x, r_{s+1} = r_s - e_s[idx_s])
and code k the reference distance is dist(k) = |r|^2 - 2 r.e_k + |e_k|^2
(oracle/ref_ops.py vq_distance).  An fp32 evaluation computes each of the three
terms as a D-term fma chain (error at most D u times the sum of the terms'
magnitudes, u = 2^-24), adds three more roundings in the distance expression,
and starts from an fp32 residual that carries s stages of update rounding (four
roundings per stage: q - r, r + diff, r - qst and the running sum).  With
eps32 = 2u, which leaves a factor 2,

    b(k) = (D + 4 + 4 s) eps32 (|r|^2 + 2 sum_d |r_d| |e_dk| + |e_k|^2)

bounds the error of dist(k), and a pick is accepted when
dist(idx) - min_k dist(k) <= b(idx) + b(argmin).  A wrong pick can hide only in
a (row, stage) pair whose fp64 top-2 margin is itself below b(best) + b(second):
check_picks returns the share of such pairs, a condition on the inputs.
"""
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
COMMITMENT = 0.25            # a power of two: a dropped or doubled factor cannot hide in rounding
NDUP = 17                    # unique columns of the `dup` codebooks (coprime to the 16-code tile)

# the constants of vq.hip, restated
MFMA_MAXD, MFMA_MAXK, MFMA_MAXS = 64, 8192, 16     # DM, kHistMaxK, SM
MAXD = 256
TILE = 16                    # codes per matrix-core tile
WAVES = 8                    # waves per matrix-core block
PASS = 1024                  # codes per pass: THREADS * CPT (direct) = KP (staged)
DCHUNK = 8                   # dims per staged chunk (DC)
ROWS = {"mfma": 16, "mfma2": 32, "staged": 20, "direct": 16}
RG2_MIN_BLOCKS = 128         # key 39 = 2 engages at this many 32-row blocks
BWD_GRID = 4096 * 256        # elements one sweep of k_rvq_bwd covers
HIST_ROWS = 4096             # rows per k_rvq_hist block

# (key 2, key 39): default, direct, staged, matrix-core with two row groups per block
SETTINGS = ((0, 0), (1, 0), (2, 0), (0, 2))

# (N, D, K, S)
CASES = {
    "one": (1, 4, 1, 1),             # one row, one code, one tile, seven idle waves
    "s16": (17, 4, 16, 16),          # S = SM; the second block holds one row
    "s17": (17, 8, 16, 17),          # S > SM: staged by default, direct with key 2 = 1
    "k8192": (33, 64, 8192, 2),      # the matrix-core limit, 512 tiles, full histogram bins
    "k8196": (33, 64, 8196, 2),      # K > 8192: staged / direct, 9 passes, the last of 4 codes
    "d128": (45, 128, 1028, 2),      # staged at D > 64, 2 passes, 3 blocks of 20 rows (the last has 5)
    "d256": (21, 256, 2052, 1),      # D = MAXD, 32 dim-chunks x 3 passes
    "d255": (19, 255, 1030, 2),      # direct only (odd D, K % 4 != 0), 2 passes
    "tiny": (50, 3, 5, 3),           # D < 4, K < 16
    "rg2": (4100, 64, 48, 2),        # key 39 = 2 engages: 129 blocks of 32 rows, the last has 4; 3 tiles < 8 waves
    "d60": (333, 60, 1000, 3),       # zero-padded fragments, 63 tiles: the waves differ in tile count
    "wrap": (16400, 64, 64, 1),      # N D > 4096 x 256: the backward's grid-stride loop wraps; 5 histogram blocks
    "dup": (333, 64, 1020, 2),       # embeds[:, :, k] = base[:, :, k % 17]: exact ties
}
# one seed per case; a case whose hide share broke its cap would get another
SEEDS = {name: 0 for name in CASES}
BWD_CASES = ("wrap", "d255", "d60")


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------
# the dispatch of sel_rvq_fwd, restated from its comments
# ---------------------------------------------------------------------------
def properties(case):
    N, D, K, S = case
    mfma_ok = D % 4 == 0 and D <= MFMA_MAXD and K <= MFMA_MAXK and S <= MFMA_MAXS
    staged_ok = D % DCHUNK == 0 and K % 4 == 0
    tiles = _cdiv(K, TILE)
    blocks = {v: _cdiv(N, r) for v, r in ROWS.items()}
    return dict(mfma_ok=mfma_ok, staged_ok=staged_ok, tiles=tiles, passes=_cdiv(K, PASS),
                last_pass=K - (_cdiv(K, PASS) - 1) * PASS, rows=dict(ROWS), blocks=blocks,
                last_rows={v: N - (blocks[v] - 1) * r for v, r in ROWS.items()},
                key39=mfma_ok and blocks["mfma2"] >= RG2_MIN_BLOCKS,
                tiles_per_wave=[len(range(w, tiles, WAVES)) for w in range(WAVES)],
                bwd_wraps=N * D > BWD_GRID, bwd_excess=N * D - BWD_GRID, hist_blocks=_cdiv(N, HIST_ROWS))


def kernel_of(case, key2, key39):
    """the kernel a (key 2, key 39) setting runs for a shape"""
    p = properties(case)
    if p["mfma_ok"] and key2 == 0:
        return "mfma2" if key39 == 2 and p["key39"] else "mfma"
    if p["staged_ok"] and key2 != 1:
        return "staged"
    return "direct"


def check_properties(name):
    """The property a case is named for, from the shape arithmetic alone."""
    case = CASES[name]
    N, D, K, S = case
    p = properties(case)
    ker = [kernel_of(case, *st) for st in SETTINGS]
    assert 0 < D <= MAXD and N > 0 and K > 0 and S > 0
    if name == "one":
        assert case == (1, 4, 1, 1) and p["mfma_ok"] and p["tiles"] == 1
        assert p["tiles_per_wave"] == [1] + [0] * 7
    elif name == "s16":
        assert S == MFMA_MAXS and p["mfma_ok"] and p["blocks"]["mfma"] == 2 and p["last_rows"]["mfma"] == 1
        assert not p["staged_ok"] and ker == ["mfma", "direct", "direct", "mfma"]
    elif name == "s17":
        assert S == MFMA_MAXS + 1 and not p["mfma_ok"] and p["staged_ok"]
        assert D % 4 == 0 and D <= MFMA_MAXD and K <= MFMA_MAXK          # S alone keeps it off the matrix cores
        assert ker == ["staged", "direct", "staged", "staged"]
    elif name == "k8192":
        assert K == MFMA_MAXK and p["mfma_ok"] and p["tiles"] == 512 and p["blocks"]["mfma"] > 1
        assert ker == ["mfma", "direct", "staged", "mfma"]
    elif name == "k8196":
        assert K > MFMA_MAXK and not p["mfma_ok"] and p["staged_ok"] and D % 4 == 0 and D <= MFMA_MAXD and S <= MFMA_MAXS
        assert p["passes"] == 9 and p["last_pass"] == 4
        assert ker == ["staged", "direct", "staged", "staged"]
    elif name == "d128":
        assert D > MFMA_MAXD and p["staged_ok"] and p["passes"] == 2 and p["last_pass"] == 4
        assert p["blocks"]["staged"] == 3 and p["last_rows"]["staged"] == 5
        assert ker == ["staged", "direct", "staged", "staged"]
    elif name == "d256":
        assert D == MAXD and p["staged_ok"] and D // DCHUNK == 32 and p["passes"] == 3 and p["last_pass"] == 4
        assert p["blocks"]["staged"] == 2 and p["blocks"]["direct"] == 2
        assert ker == ["staged", "direct", "staged", "staged"]
    elif name == "d255":
        assert D % 2 == 1 and D == MAXD - 1 and K % 4 != 0 and not p["mfma_ok"] and not p["staged_ok"]
        assert p["passes"] == 2 and p["blocks"]["direct"] == 2 and ker == ["direct"] * 4
    elif name == "tiny":
        assert D < 4 and K < TILE and not p["mfma_ok"] and not p["staged_ok"] and ker == ["direct"] * 4
        assert p["blocks"]["direct"] == 4 and p["last_rows"]["direct"] == 2
    elif name == "rg2":
        assert p["key39"] and p["blocks"]["mfma2"] == 129 and p["last_rows"]["mfma2"] == 4
        assert p["tiles"] == 3 and p["tiles"] < WAVES and p["hist_blocks"] == 2
        assert ker == ["mfma", "direct", "staged", "mfma2"]
    elif name == "d60":
        assert p["mfma_ok"] and D % 16 != 0 and D < MFMA_MAXD and not p["staged_ok"] and p["tiles"] == 63
        assert sorted(set(p["tiles_per_wave"])) == [7, 8] and S >= 3    # odd and even counts: both buffer parities
        assert K % TILE != 0 and ker == ["mfma", "direct", "direct", "mfma"]
    elif name == "wrap":
        assert p["bwd_wraps"] and p["bwd_excess"] == 1024 and p["hist_blocks"] == 5 and p["mfma_ok"]
        assert p["key39"] and ker == ["mfma", "direct", "staged", "mfma2"]
    elif name == "dup":
        assert p["mfma_ok"] and p["staged_ok"] and math.gcd(NDUP, TILE) == 1 and K // NDUP == 60
        assert ker == ["mfma", "direct", "staged", "mfma"]
    else:
        raise KeyError(name)
    # no other case may engage key 39 by accident, and only `wrap` wraps the backward
    assert p["key39"] == (name in ("rg2", "wrap")) and p["bwd_wraps"] == (name == "wrap")
    return p


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
_IN = {}


def inputs(name):
    """x = 1.5 randn(N, D), embeds = randn(S, D, K), fp32 on the CPU, computed once."""
    if name not in _IN:
        N, D, K, S = CASES[name]
        g = torch.Generator().manual_seed(SEEDS[name])
        x = 1.5 * torch.randn(N, D, generator=g)
        if name == "dup":
            base = torch.randn(S, D, NDUP, generator=g)
            embeds = base[:, :, torch.arange(K) % NDUP].contiguous()
        else:
            embeds = torch.randn(S, D, K, generator=g)
        _IN[name] = (x, embeds)
    return _IN[name]


def unique_of(name):
    return NDUP if name == "dup" else None


# ---------------------------------------------------------------------------
# the reference of the picks
# ---------------------------------------------------------------------------
def check_picks(x, embeds, idx, unique=None):
    """fp64 check of the picks idx (S, N) for x (N, D) and embeds (S, D, K), chained
    on idx itself.  With ``unique`` = U the codebooks repeat their first U columns
    (column k equals column k % U bit for bit): the reference is the argmin over
    those U, and every pick must be < U (lowest index wins, exactly).

    Returns dict(pairs, nbad, bad (the first few (row, stage, gap, allowed)),
    worst (largest gap / allowed), hide (share of pairs whose fp64 top-2 margin
    is below b(best) + b(second)), out_of_range)."""
    x, embeds, idx = x.detach().double().cpu(), embeds.detach().double().cpu(), idx.detach().cpu().long()
    N, D = x.shape
    S, _, K = embeds.shape
    assert tuple(idx.shape) == (S, N) and embeds.shape[1] == D
    U = K if unique is None else unique
    rows = torch.arange(N)
    r = x.clone()
    bad, nbad, worst, hidden, oor = [], 0, 0.0, 0, 0
    for s in range(S):
        e = embeds[s][:, :U]
        if unique is not None:
            assert torch.equal(embeds[s], e[:, torch.arange(K) % U])
        pick = idx[s]
        inr = (pick >= 0) & (pick < U)
        oor += int((~inr).sum())
        pk = pick.clamp(0, U - 1)
        r2, e2 = (r * r).sum(1, keepdim=True), (e * e).sum(0, keepdim=True)
        dist = r2 - 2 * r @ e + e2
        b = (D + 4 + 4 * s) * EPS32 * (r2 + 2 * r.abs() @ e.abs() + e2)
        dmin, amin = dist.min(1)
        gap = dist[rows, pk] - dmin
        allowed = b[rows, pk] + b[rows, amin]
        ratio = gap / allowed
        worst = max(worst, float(ratio.max()))
        viol = (gap > allowed) | ~inr
        nbad += int(viol.sum())
        for row in viol.nonzero().flatten()[:6].tolist():
            bad.append((row, s, int(pick[row]), int(amin[row]), float(gap[row]), float(allowed[row])))
        if U > 1:
            d2, k2 = torch.topk(dist, 2, dim=1, largest=False)
            hidden += int(((d2[:, 1] - d2[:, 0]) < b[rows, k2[:, 0]] + b[rows, k2[:, 1]]).sum())
        r = r - embeds[s][:, pk].t()
    return dict(pairs=N * S, nbad=nbad, bad=bad[:6], worst=worst, hide=hidden / (N * S), out_of_range=oor)


def hide_cap(pairs):
    """at most 1 % of the pairs may be able to hide a wrong pick; none below 200 pairs"""
    return 0.0 if pairs < 200 else 0.01


# ---------------------------------------------------------------------------
# everything else, restated in fp64 from given picks
# ---------------------------------------------------------------------------
def restate(x, embeds, idx, commitment=COMMITMENT):
    """out (N, D), losses (S,), ppls (S,) in fp64 and counts (S, K) int64 from idx (S, N)"""
    x, embeds, idx = x.detach().double().cpu(), embeds.detach().double().cpu(), idx.detach().cpu().long()
    N, D = x.shape
    S, _, K = embeds.shape
    r = x.clone()
    out = torch.zeros_like(x)
    losses, ppls, counts = [], [], []
    for s in range(S):
        q = embeds[s][:, idx[s]].t()
        losses.append(((q - r) ** 2).mean() * commitment)
        c = torch.bincount(idx[s], minlength=K)
        p = c.double() / N
        ppls.append(torch.exp(-(p * torch.log(p + 1e-10)).sum()))
        counts.append(c)
        out = out + q
        r = r - q
    return out, torch.stack(losses), torch.stack(ppls), torch.stack(counts)


def grad_closed(x, embeds, idx, g_out=None, g_loss=None, commitment=COMMITMENT):
    """d/dx of sum(out g_out) + sum(losses g_loss) in fp64: out is the
    straight-through value, so d out / d x = 1, and every later residual has a
    zero derivative, so only the first stage's loss contributes."""
    x, e0 = x.detach().double().cpu(), embeds[0].detach().double().cpu()
    N, D = x.shape
    g = torch.zeros_like(x) if g_out is None else g_out.detach().double().cpu().clone()
    if g_loss is not None:
        q0 = e0[:, idx[0].detach().cpu().long()].t()
        g = g + float(g_loss[0]) * commitment * 2.0 * (x - q0) / (N * D)
    return g


def grad_elem_bound(x, embeds, idx, g_out=None, g_loss=None, commitment=COMMITMENT):
    """Per-element rounding bound of the fp32 gradient g_out + c (x - q): c takes
    four roundings (g_loss commitment, 2 / (N D) and the product), x - q and the
    product one each, the sum one more: 4 eps32 (|g_out| + |c| |x - q|) covers
    7 u of relative error on the second term and u on the sum."""
    zero = torch.zeros(x.shape, dtype=torch.float64)
    go = zero if g_out is None else g_out.detach().double().cpu().abs()
    second = grad_closed(x, embeds, idx, None, g_loss, commitment).abs() if g_loss is not None else zero
    return 4 * EPS32 * (go + second)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
