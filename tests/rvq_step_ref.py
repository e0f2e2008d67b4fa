"""Cases, inputs and a CPU restatement of the streaming RVQ step kernels
(csrc/vq_step.hip: sel_rvq_step, sel_rvq_lookup_step), shared by
tests/test_rvq_step_host.py and tests/test_gpu_rvq_step.py.  A plain helper:
nothing here needs a GPU.  The fp64 reference of the picks and its rounding
bound are rvq_cases.check_picks.
"""
import torch

import rvq_cases as C

# (rows, rows_per_sample, D, K, S): each the smallest shape that reaches one edge
CASES = {
    "hop": (1, 1, 64, 1024, 8),        # the B = 1 hop: one row, the register-resident instance
    "one": (1, 1, 4, 1, 1),            # one code
    "d60": (5, 1, 60, 1000, 3),        # K and D off every vector / wave multiple
    "d255": (3, 3, 255, 37, 2),        # four d passes per lane in |r|^2, K below one wave
    "k2050": (2, 1, 256, 2050, 2),     # D at its limit, three code passes, the last of 2 codes
    "pool": (64, 4, 64, 1024, 8),      # 16 streams x 4 frames: one block per row, 64 blocks
    "s17": (2, 2, 8, 16, 17),          # S above sel_rvq_fwd's matrix-core limit of 16
    "dup": (5, 1, 64, 1020, 2),        # embeds[:, :, k] = base[:, :, k % 17]: exact ties, generic loop
    "dup_col": (5, 1, 64, 1024, 2),    # the same on the register-resident instance
}
# one seed per case, chosen so that no (row, stage) pair of a case under 200
# pairs, and at most 1 % of a larger one, has an fp64 top-2 margin below the
# rounding bound (rvq_cases.hide_cap); tests/test_rvq_step_host.py asserts it
SEEDS = {name: 0 for name in CASES}

THREADS, CPT = 256, 4                  # the generic kernel: codes per pass = THREADS * CPT
COL_SHAPE = (64, 1024)                 # (D, K) of the register-resident instance


def unique_of(name):
    return C.NDUP if name.startswith("dup") else None


def instance_of(case):
    rows, T, D, K, S = case
    return "col" if (D, K) == COL_SHAPE else "any"


def check_properties(name):
    """The edge a case is named for, from the shape arithmetic alone."""
    case = CASES[name]
    rows, T, D, K, S = case
    assert rows >= 1 and rows % T == 0 and 0 < D <= C.MAXD and K > 0 and S > 0
    passes = -(-K // (THREADS * CPT))
    if name == "hop":
        assert rows == 1 and instance_of(case) == "col" and S == 8
    elif name == "one":
        assert K == 1 and rows == 1 and S == 1
    elif name == "d60":
        assert D % 8 and D % 64 and K % 64 and K % 16 and instance_of(case) == "any" and rows > 1
    elif name == "d255":
        assert -(-D // 64) == 4 and D % 2 == 1 and K < 64 and T == rows == 3
    elif name == "k2050":
        assert D == C.MAXD and passes == 3 and K - 2 * THREADS * CPT == 2
    elif name == "pool":
        assert rows == 16 * 4 and T == 4 and instance_of(case) == "col"
    elif name == "s17":
        assert S > C.MFMA_MAXS and T == 2
    elif name == "dup":
        assert instance_of(case) == "any" and K // C.NDUP == 60
    elif name == "dup_col":
        assert instance_of(case) == "col"
    else:
        raise KeyError(name)
    return dict(passes=passes, instance=instance_of(case))


_IN = {}


def inputs(name):
    """z = 1.5 randn(rows, D), embeds = randn(S, D, K), fp32 on the CPU, computed once."""
    if name not in _IN:
        rows, T, D, K, S = CASES[name]
        g = torch.Generator().manual_seed(SEEDS[name])
        z = 1.5 * torch.randn(rows, D, generator=g)
        if unique_of(name):
            base = torch.randn(S, D, C.NDUP, generator=g)
            embeds = base[:, :, torch.arange(K) % C.NDUP].contiguous()
        else:
            embeds = torch.randn(S, D, K, generator=g)
        _IN[name] = (z, embeds)
    return _IN[name]


def _fma(a, b, c):
    """fmaf(a, b, c) on fp32 tensors: the product is exact in fp64, the sum is
    rounded to fp64 and then to fp32 (a double rounding, off from the single one
    in the last place once in about 2^29 sums)."""
    return (a.double() * b.double() + c.double()).float()


def rvq_step(z, embeds, flatten=False):
    """The sel_rvq_step contract in fp32 on the CPU: idx (S, rows) int64 and zq
    (rows, D).  Per (row, stage, code): |r|^2 with 64 lanes over d and the xor
    butterfly, dot and |e_k|^2 as fma chains over d ascending,
    dist = (|r|^2 - 2 dot) + |e_k|^2, lowest index on ties (torch.min's first
    minimum is not promised: the tie is broken explicitly), then q = e_idx,
    qst = r + (q - r), r <- r - qst, zq += qst."""
    assert z.dtype == embeds.dtype == torch.float32
    rows, D = z.shape
    S, _, K = embeds.shape
    r = z.clone()
    zq = torch.zeros_like(z)
    idx = torch.empty((S, rows), dtype=torch.int64)
    ks = torch.arange(K)
    for s in range(S):
        E = embeds[s]
        lanes = torch.zeros(rows, 64)
        for d0 in range(0, D, 64):
            w = min(64, D - d0)
            lanes[:, :w] = _fma(r[:, d0:d0 + w], r[:, d0:d0 + w], lanes[:, :w])
        o = 32
        while o:
            lanes = lanes + lanes[:, torch.arange(64) ^ o]
            o >>= 1
        r2 = lanes[:, :1]
        dot = torch.zeros(rows, K)
        en = torch.zeros(1, K)
        for d in range(D):
            en = _fma(E[d:d + 1], E[d:d + 1], en)
            dot = _fma(r[:, d:d + 1], E[d:d + 1], dot)
        dist = (r2 - 2.0 * dot) + en
        best = dist.min(1, keepdim=True).values
        pick = torch.where(dist == best, ks, K).min(1).values
        pick = torch.where(pick >= K, 0, pick)          # a NaN row picks code 0
        q = E[:, pick].t()
        qst = r + (q - r)
        r = r - qst
        zq = zq + qst
        idx[s] = pick + (s * K if flatten else 0)
    return idx, zq


def ordered_lookup(idx, codebook, mean=None, scale=None):
    """The sel_rvq_lookup_step contract with torch elementwise ops (any device):
    codebook rows added one stage after the other in ascending order, fp32."""
    acc = codebook[idx[0]]
    for s in range(1, idx.shape[0]):
        acc = acc + codebook[idx[s]]
    if mean is not None:
        acc = (acc - mean) / scale
    return acc
