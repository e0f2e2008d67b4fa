"""GPU checks of the datagram kernels (csrc/vq_step.hip: sel_rvq_step_dgram,
sel_rvq_lookup_dgram_step).  Two references, neither the code under test:
tests/dgram_ref.py (wire version 2 in plain Python integers) and the existing
sel_rvq_step / sel_rvq_step_wire / sel_rvq_lookup_step.  Every comparison is
exact.  Every output buffer starts as a sentinel (0xFF, NaN, -1 / -7), so that
"not written" is observable.

A  sel_rvq_step_dgram on the nine cases of tests/rvq_step_ref.py with mixed
   budgets in one launch: idx[:s_i] equal to sel_rvq_step's (flattened and not),
   idx[s_i:] == -1, zq equal to sel_rvq_step with S = s_i on embeds[:s_i], header
   and records equal to dgram_ref, every byte past a datagram's length still
   0xFF; the clamps; stages = NULL; at full budget the records of
   sel_rvq_step_wire; idx = NULL and zq = NULL; a view one byte into its
   allocation with a wider stride; seq 0, 65535, 65536; the six n_active values;
   a captured launch replayed on three staged (count, budgets, seq) sets.
B  sel_rvq_lookup_dgram_step: mixed budgets equal to sel_rvq_lookup_step on the
   -1-padded ids, and idx_out; the three-launch hold sequence; bad headers; a
   field >= K inside a truncated record; all-ones pad bits; hold = NULL; slots
   NULL / a permutation / -1 / nslots; the n_active set; a misaligned buffer; a
   captured launch on three staged sets.
C  operand checks of the bindings that must raise before any launch.
"""
import pytest
import torch

import dgram_ref as DR
import rvq_step_ref as SR
import wire_ref as WR

pytestmark = pytest.mark.gpu

COUNTS = ("null", 0, 1, "all", "all+1", -1)
INT_MAX = (1 << 31) - 1

# the budgets each case runs (one list per launch, one entry per sample)
BUDGETS = {
    "hop": [[s] for s in range(1, 9)],
    "pool": [list(range(1, 9)) + list(range(8, 0, -1))],
    "s17": [[1], [2], [16], [17]],            # 4-bit fields: a padded byte, a full byte, 64 and 68 bits
    "d255": [[1], [2]],                       # three frames per sample
    "k2050": [[1, 1], [2, 1]],                # 12 bits in two bytes
    "d60": [[1, 2, 3, 3, 1], [0, -5, 4, INT_MAX, 3]],      # and the clamps
    "one": [[1]],
    "dup": [[1, 2, 2, 1, 2]],
    "dup_col": [[2, 1, 1, 2, 1]],
}
LAUNCHES = [(name, i) for name in SR.CASES for i in range(len(BUDGETS[name]))]


def _count(c, B):
    return {"null": None, "all": B, "all+1": B + 1}.get(c, c)


def _active(c, B):
    n = _count(c, B)
    return B if n is None else min(max(n, 0), B)


def _n_active(gpu, count, B):
    n = _count(count, B)
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=gpu)


def _i32(gpu, values):
    return None if values is None else torch.tensor(values, dtype=torch.int32, device=gpu)


_STEP = {}


def _existing_step(gpu, name, s=None):
    """sel_rvq_step's (idx unflattened, zq) with S = s on embeds[:s], on the CPU, once per (case, s)"""
    rows, T, D, K, S = SR.CASES[name]
    s = S if s is None else s
    if (name, s) not in _STEP:
        from sel import streamops as SO
        z, embeds = SR.inputs(name)
        idx = torch.full((s, rows), -1, dtype=torch.int64, device=gpu)
        zq = torch.full((rows, D), float("nan"), device=gpu)
        SO.rvq_step(z.to(gpu), embeds[:s].contiguous().to(gpu), idx, T, None, False, zq)
        torch.cuda.synchronize()
        assert int(idx.min()) >= 0 and int(idx.max()) < K
        _STEP[name, s] = (idx.cpu(), zq.cpu())
    return _STEP[name, s]


def _expected(gpu, name, budgets, seq, live=None):
    """(idx unflattened with -1 beyond the budgets, zq, datagrams) from the references, per sample"""
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    full, _ = _existing_step(gpu, name)
    idx = torch.full((S, rows), -1, dtype=torch.int64)
    zq = torch.empty(rows, D)
    st = [DR.clamp(b, S) for b in budgets]
    for i, s in enumerate(st):
        cut, zq_s = _existing_step(gpu, name, s)
        r = slice(i * T, (i + 1) * T)
        assert torch.equal(cut[:, r], full[:s, r])                 # the reference's own scalability
        idx[:s, r] = full[:s, r]
        zq[r] = zq_s[r]
    return idx, zq, DR.pack(full, st, seq, K, T), st


def _step_dgram(gpu, name, budgets, seq=None, count="null", flatten=False, with_idx=True, with_zq=True, extra=0,
                offset=0):
    """One eager sel_rvq_step_dgram on sentinel-filled outputs -> (idx, zq, dgram) on the CPU."""
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    z, embeds = SR.inputs(name)
    idx = torch.full((S, rows), -7, dtype=torch.int64, device=gpu) if with_idx else None
    zq = torch.full((rows, D), float("nan"), device=gpu) if with_zq else None
    stride = DR.dgram_bytes(S, K, T) + extra
    store = torch.full((B * stride + offset,), 0xFF, dtype=torch.uint8, device=gpu)
    dgram = store[offset:].view(B, stride)
    assert dgram.data_ptr() % 2 == offset % 2
    SO.rvq_step_dgram(z.to(gpu), embeds.to(gpu), dgram, T, _n_active(gpu, count, B), _i32(gpu, budgets),
                      _i32(gpu, seq), flatten, idx, zq)
    torch.cuda.synchronize()
    return (idx.cpu() if with_idx else None), (zq.cpu() if with_zq else None), dgram.cpu()


def _check_bytes(dgram, want, live_samples):
    """row i < live starts with want[i] and is 0xFF behind it; the rows beyond are all 0xFF"""
    for i in range(dgram.shape[0]):
        n = len(want[i]) if i < live_samples else 0
        assert bytes(dgram[i, :n].tolist()) == want[i][:n], (i, bytes(dgram[i, :n].tolist()).hex(), want[i].hex())
        assert bool((dgram[i, n:] == 0xFF).all()), i


# ---------------------------------------------------------------------------
# A. sel_rvq_step_dgram
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", LAUNCHES, ids=[f"{n}-{i}" for n, i in LAUNCHES])
def test_step_dgram_equals_step_and_the_reference(gpu, name, which):
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    budgets = BUDGETS[name][which]
    assert len(budgets) == B
    seq = [(65534 + 3 * i) & 0x7FFFFFFF for i in range(B)]
    want_idx, want_zq, want, st = _expected(gpu, name, budgets, seq)
    flat = torch.where(want_idx >= 0, want_idx + K * torch.arange(S).view(-1, 1), want_idx)
    idx, zq, dgram = _step_dgram(gpu, name, budgets, seq)
    assert torch.equal(idx, want_idx) and torch.equal(zq, want_zq)
    _check_bytes(dgram, want, B)
    idx_f, zq_f, dgram_f = _step_dgram(gpu, name, budgets, seq, flatten=True)
    assert torch.equal(idx_f, flat) and torch.equal(zq_f, want_zq) and torch.equal(dgram_f, dgram)
    none, zq_n, dgram_n = _step_dgram(gpu, name, budgets, seq, with_idx=False)
    assert none is None and torch.equal(zq_n, want_zq) and torch.equal(dgram_n, dgram)
    idx_n, none, dgram_n = _step_dgram(gpu, name, budgets, seq, with_zq=False)
    assert none is None and torch.equal(idx_n, want_idx) and torch.equal(dgram_n, dgram)
    none, none2, dgram_n = _step_dgram(gpu, name, budgets, seq, with_idx=False, with_zq=False)
    assert none is None and none2 is None and torch.equal(dgram_n, dgram)
    # a view one byte into its allocation, rows three bytes apart from one another
    idx_o, zq_o, dgram_o = _step_dgram(gpu, name, budgets, seq, extra=3, offset=1)
    assert torch.equal(idx_o, want_idx) and torch.equal(zq_o, want_zq)
    _check_bytes(dgram_o, want, B)


@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_dgram_without_budgets_is_step_wire_with_a_header(gpu, name):
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    full, zq0 = _existing_step(gpu, name)
    z, embeds = SR.inputs(name)
    wire = torch.full((rows, WR.frame_bytes(S, K)), 0xFF, dtype=torch.uint8, device=gpu)
    SO.rvq_step_wire(z.to(gpu), embeds.to(gpu), wire, T)
    torch.cuda.synchronize()
    for budgets, seq in ((None, None), ([S] * B, [0] * B), ([S + 1] * B, None)):
        idx, zq, dgram = _step_dgram(gpu, name, budgets, seq)
        assert torch.equal(idx, full) and torch.equal(zq, zq0)
        assert torch.equal(dgram[:, :4], torch.tensor([[2, S, 0, 0]] * B, dtype=torch.uint8))
        assert torch.equal(dgram[:, 4:].reshape(rows, -1), wire.cpu())
        _check_bytes(dgram, DR.pack(full, [S] * B, [0] * B, K, T), B)


@pytest.mark.parametrize("name", ["hop", "d60", "d255"])
def test_step_dgram_sequence_numbers_wrap(gpu, name):
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    for q in (0, 65535, 65536, 65537, -1, INT_MAX):
        _, _, dgram = _step_dgram(gpu, name, None, [q] * B, with_idx=False, with_zq=False)
        assert torch.equal(dgram[:, 2:4], torch.tensor([[q & 0xFF, (q >> 8) & 0xFF]] * B, dtype=torch.uint8)), q
        assert [DR.parse(bytes(r.tolist()), S, K, T) for r in dgram] == [(S, q & 0xFFFF)] * B


@pytest.mark.parametrize("count", COUNTS, ids=[str(c) for c in COUNTS])
@pytest.mark.parametrize("name", list(SR.CASES))
def test_step_dgram_active_set(gpu, name, count):
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    budgets = BUDGETS[name][0]
    seq = list(range(7, 7 + B))
    live = _active(count, B)
    want_idx, want_zq, want, _ = _expected(gpu, name, budgets, seq)
    idx, zq, dgram = _step_dgram(gpu, name, budgets, seq, count)
    assert torch.equal(idx[:, :live * T], want_idx[:, :live * T]) and torch.equal(zq[:live * T], want_zq[:live * T])
    assert bool((idx[:, live * T:] == -7).all()) and bool(torch.isnan(zq[live * T:]).all())
    _check_bytes(dgram, want, live)


@pytest.mark.parametrize("name", ["hop", "pool", "d255", "s17", "d60"])
def test_step_dgram_captured_launch_follows_staged_words(gpu, name):
    from sel import streamops as SO
    rows, T, D, K, S = SR.CASES[name]
    B = rows // T
    z, embeds = SR.inputs(name)
    zd, ed = z.to(gpu), embeds.to(gpu)
    idx = torch.full((S, rows), -7, dtype=torch.int64, device=gpu)
    zq = torch.full((rows, D), float("nan"), device=gpu)
    dgram = torch.full((B, DR.dgram_bytes(S, K, T)), 0xFF, dtype=torch.uint8, device=gpu)
    ctl = torch.zeros(1 + 2 * B, dtype=torch.int32, device=gpu)          # [n, budgets..., seq...]: one tensor
    n_active, stages, seq = ctl[:1], ctl[1:1 + B], ctl[1 + B:]
    SO.rvq_step_dgram(zd, ed, dgram, T, n_active, stages, seq, False, idx, zq)   # loads the kernel; no active row
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool(torch.isnan(zq).all()) and bool((dgram == 0xFF).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        SO.rvq_step_dgram(zd, ed, dgram, T, n_active, stages, seq, False, idx, zq)
    sets = [(B, [1 + (i + 2) % S for i in range(B)], [100 + i for i in range(B)]),
            (max(B // 2, 1) if B > 1 else 0, [S - i % S for i in range(B)], [65535] * B),
            (B + 3, [1 + (5 * i) % S for i in range(B)], [65536 + i for i in range(B)])]
    for n, budgets, q in sets:
        idx.fill_(-7)
        zq.fill_(float("nan"))
        dgram.fill_(0xFF)
        ctl.copy_(torch.tensor([n] + budgets + q, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        live = min(n, B)
        want_idx, want_zq, want, _ = _expected(gpu, name, budgets, q)
        assert torch.equal(idx.cpu()[:, :live * T], want_idx[:, :live * T])
        assert torch.equal(zq.cpu()[:live * T], want_zq[:live * T])
        assert bool((idx[:, live * T:] == -7).all()) and bool(torch.isnan(zq[live * T:]).all())
        _check_bytes(dgram.cpu(), want, live)


# ---------------------------------------------------------------------------
# B. sel_rvq_lookup_dgram_step
# ---------------------------------------------------------------------------
LK_B, LK_T = 4, 2
LK_ROWS = LK_B * LK_T
LK_SHAPES = [(64, 1024, 8), (3, 37, 2), (256, 1000, 1), (8, 16, 17)]        # (D, K, S)


def _lookup_inputs(gpu, D, K, S, hop=0):
    g = torch.Generator().manual_seed(7 * D + 3 * K + S)
    cb = torch.randn(S * K, D, generator=g)
    mean = torch.randn(D, generator=g)
    scale = torch.rand(D, generator=g) + 0.5
    g.manual_seed(11 * D + 5 * K + S + 1000 * hop)
    k = torch.randint(0, K, (S, LK_ROWS), generator=g)
    k[0, 0], k[-1, -1] = 0, K - 1
    k[0, 1], k[-1, 2] = K - 1, 0
    return k, cb.to(gpu), mean.to(gpu), scale.to(gpu)


def _mixed(S):
    """budgets of the four samples: all, one, and two in between (as far as S allows)"""
    return [S, 1, max(S // 2, 1), min(2, S)]


def _flat(k, K, stages=None):
    """(S, rows) un-flattened codes -> flattened ids, -1 beyond each sample's stage count"""
    S = k.shape[0]
    ids = k + K * torch.arange(S).view(-1, 1)
    if stages is not None:
        for i, s in enumerate(stages):
            ids[s:, i * LK_T:(i + 1) * LK_T] = -1
    return ids


def _existing_lookup(gpu, ids, cb, dtype, ms):
    """sel_rvq_lookup_step on flattened ids (S, rows) with -1 for absent fields, every row active"""
    from sel import streamops as SO
    out = torch.full((ids.shape[1], cb.shape[1]), float("nan"), dtype=dtype, device=gpu)
    SO.rvq_lookup_step(ids.to(gpu), cb, out, LK_T, ms[0], ms[1], None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    return out


def _held_ids(ids):
    """what a lost sample decodes: its last row's ids in every one of its rows"""
    return ids.view(ids.shape[0], LK_B, LK_T)[:, :, -1:].expand(-1, -1, LK_T).reshape(ids.shape[0], -1).contiguous()


def _hold(gpu, S, K, nslots=LK_B, fill=0):
    return torch.full((nslots, 1 + DR.fb(S, K)), fill, dtype=torch.uint8, device=gpu)


def _lookup_dgram(gpu, dgram, cb, S, dtype, ms, count="null", slots=None, lost=None, hold=None, with_idx=True):
    from sel import streamops as SO
    rows = dgram.shape[0] * LK_T
    out = torch.full((rows, cb.shape[1]), float("nan"), dtype=dtype, device=gpu)
    idx_out = torch.full((S, rows), -7, dtype=torch.int64, device=gpu) if with_idx else None
    SO.rvq_lookup_dgram_step(dgram, cb, S, out, LK_T, ms[0], ms[1], _n_active(gpu, count, dgram.shape[0]),
                             _i32(gpu, slots), _i32(gpu, lost), hold, idx_out)
    torch.cuda.synchronize()
    return out, (idx_out.cpu() if with_idx else None)


def _want_hold(datagrams, S, K, prev=None, valid=None):
    """the hold rows after a launch: {stages, last record} of every valid sample, prev elsewhere"""
    out = torch.zeros((len(datagrams), 1 + DR.fb(S, K)), dtype=torch.uint8) if prev is None else prev.clone()
    for i, d in enumerate(datagrams):
        if valid is None or valid[i]:
            s = d[1]
            n = DR.fb(s, K)
            out[i, 0] = s
            out[i, 1:1 + n] = torch.tensor(list(d[len(d) - n:]), dtype=torch.uint8)
    return out


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,K,S", LK_SHAPES)
def test_lookup_dgram_mixed_budgets_equal_lookup_step(gpu, D, K, S, dtype, stats):
    k, cb, mean, scale = _lookup_inputs(gpu, D, K, S)
    ms = (mean, scale) if stats else (None, None)
    stages = _mixed(S)
    ids = _flat(k, K, stages)
    ref = _existing_lookup(gpu, ids, cb, dtype, ms)
    dgs = DR.pack(k, stages, [9, 65535, 0, 1], K, LK_T)
    stride = DR.dgram_bytes(S, K, LK_T)
    buf = DR.buffer(dgs, stride)                              # 0xFF behind every datagram: never read
    for i, d in enumerate(dgs):
        assert torch.equal(DR.unpack(d, S, K, LK_T, flatten=True), ids[:, i * LK_T:(i + 1) * LK_T])
    sentinel = _hold(gpu, S, K, fill=0xEE)
    for count in COUNTS:
        hold = sentinel.clone()
        out, idx_out = _lookup_dgram(gpu, buf.to(gpu), cb, S, dtype, ms, count, hold=hold)
        live = _active(count, LK_B)
        assert torch.equal(out[:live * LK_T], ref[:live * LK_T]), count
        assert bool(torch.isnan(out[live * LK_T:].float()).all()), count
        assert torch.equal(idx_out[:, :live * LK_T], ids[:, :live * LK_T]) and bool((idx_out[:, live * LK_T:] == -7).all())
        # the hold rows of the active samples: their record; of the inactive ones: untouched
        want = _want_hold(dgs, S, K, prev=sentinel.cpu(), valid=[i < live for i in range(LK_B)])
        got = hold.cpu()
        for i in range(LK_B):
            n = 1 + DR.fb(stages[i], K) if i < live else got.shape[1]
            assert torch.equal(got[i, :n], want[i, :n]), (count, i)
            assert bool((got[i, n:] == 0xEE).all()), (count, i)
    out, none = _lookup_dgram(gpu, buf.to(gpu), cb, S, dtype, ms, with_idx=False)           # hold = NULL too
    assert none is None and torch.equal(out, ref)
    # a view one byte into its allocation, with a wider stride
    store = torch.full((LK_B * (stride + 3) + 1,), 0xFF, dtype=torch.uint8, device=gpu)
    view = store[1:].view(LK_B, stride + 3)
    view[:, :stride].copy_(buf)
    assert view.data_ptr() % 2 == 1
    out, idx_out = _lookup_dgram(gpu, view, cb, S, dtype, ms, hold=_hold(gpu, S, K))
    assert torch.equal(out, ref) and torch.equal(idx_out, ids)
    # all-ones pad bits
    dirty = DR.buffer([DR.set_pad_bits(d, S, K, LK_T) for d in dgs], stride)
    out, idx_out = _lookup_dgram(gpu, dirty.to(gpu), cb, S, dtype, ms)
    assert torch.equal(out, ref) and torch.equal(idx_out, ids)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,K,S", LK_SHAPES)
def test_lookup_dgram_hold_sequence(gpu, D, K, S, dtype, stats):
    """1: all valid (slots 0..3 of 5).  2: samples 1 and 3 lost -> their held records, hold
    unchanged for them.  3: lost again, plus slot 4, which never received anything: the empty sum."""
    k1, cb, mean, scale = _lookup_inputs(gpu, D, K, S, hop=1)
    k2 = _lookup_inputs(gpu, D, K, S, hop=2)[0]
    ms = (mean, scale) if stats else (None, None)
    stride = DR.dgram_bytes(S, K, LK_T)
    st1, st2 = _mixed(S), list(reversed(_mixed(S)))
    hold = _hold(gpu, S, K, nslots=5)
    slots = [0, 1, 2, 3]
    d1 = DR.pack(k1, st1, [0] * 4, K, LK_T)
    ids1 = _flat(k1, K, st1)
    out, idx_out = _lookup_dgram(gpu, DR.buffer(d1, stride).to(gpu), cb, S, dtype, ms, slots=slots, hold=hold)
    assert torch.equal(out, _existing_lookup(gpu, ids1, cb, dtype, ms)) and torch.equal(idx_out, ids1)
    h1 = torch.cat([_want_hold(d1, S, K), torch.zeros(1, 1 + DR.fb(S, K), dtype=torch.uint8)])
    assert torch.equal(hold.cpu(), h1)
    # 2: the lost samples' bytes are garbage that would parse (a valid header): the flag decides
    d2 = DR.pack(k2, st2, [1] * 4, K, LK_T)
    lost = [0, 1, 0, 1]
    ids2 = _flat(k2, K, st2)
    held1 = _held_ids(ids1)
    want2 = ids2.clone()
    for i in (1, 3):
        want2[:, i * LK_T:(i + 1) * LK_T] = held1[:, i * LK_T:(i + 1) * LK_T]
    out, idx_out = _lookup_dgram(gpu, DR.buffer(d2, stride).to(gpu), cb, S, dtype, ms, slots=slots, lost=lost,
                                 hold=hold)
    assert torch.equal(idx_out, want2) and torch.equal(out, _existing_lookup(gpu, want2, cb, dtype, ms))
    h2 = torch.cat([_want_hold(d2, S, K, prev=h1[:4], valid=[1, 0, 1, 0]), h1[4:]])
    got = hold.cpu()
    for i in range(5):          # a shorter record leaves the tail of a longer one behind it: compare what is held
        n = 1 + DR.fb(int(h2[i, 0]), K)
        assert torch.equal(got[i, :n], h2[i, :n]), i
    assert torch.equal(got[[1, 3, 4]], h1[[1, 3, 4]])                      # read, not written
    # 3: everything lost; sample 2 now sits on slot 4, which holds nothing
    held2 = _held_ids(ids2)
    want3 = torch.full_like(ids2, -1)
    want3[:, 0:LK_T] = held2[:, 0:LK_T]                                    # slot 0: hop 2's record
    want3[:, LK_T:2 * LK_T] = held1[:, LK_T:2 * LK_T]                      # slot 1: still hop 1's
    want3[:, 3 * LK_T:] = held1[:, 3 * LK_T:]                              # slot 3: still hop 1's
    before = hold.clone()
    out, idx_out = _lookup_dgram(gpu, torch.zeros(4, stride, dtype=torch.uint8, device=gpu), cb, S, dtype, ms,
                                 slots=[0, 1, 4, 3], lost=[1, 1, 1, 1], hold=hold)
    assert torch.equal(idx_out, want3) and torch.equal(out, _existing_lookup(gpu, want3, cb, dtype, ms))
    assert torch.equal(hold, before)
    empty = out[2 * LK_T:3 * LK_T].float().cpu()
    want_empty = ((torch.zeros(D) - mean.cpu()) / scale.cpu()) if stats else torch.zeros(D)
    assert torch.equal(empty, want_empty.to(dtype).float().expand(LK_T, D))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lookup_dgram_bad_headers_are_lost(gpu, dtype):
    D, K, S = 64, 1024, 8
    k0, cb, _, _ = _lookup_inputs(gpu, D, K, S, hop=1)
    k1 = _lookup_inputs(gpu, D, K, S, hop=2)[0]
    stride = DR.dgram_bytes(S, K, LK_T)
    hold = _hold(gpu, S, K)
    st0 = [3, 8, 1, 5]
    _lookup_dgram(gpu, DR.buffer(DR.pack(k0, st0, [0] * 4, K, LK_T), stride).to(gpu), cb, S, dtype, (None, None),
                  hold=hold)
    before = hold.clone()
    buf = DR.buffer(DR.pack(k1, [8, 8, 8, 2], [1] * 4, K, LK_T), stride)
    buf[0, 0], buf[1, 1], buf[2, 1] = 3, 0, S + 1                          # version 3, 0 stages, S + 1 stages
    want = _held_ids(_flat(k0, K, st0))
    want[:, 3 * LK_T:] = _flat(k1, K, [8, 8, 8, 2])[:, 3 * LK_T:]
    out, idx_out = _lookup_dgram(gpu, buf.to(gpu), cb, S, dtype, (None, None), hold=hold)
    assert torch.equal(idx_out, want) and torch.equal(out, _existing_lookup(gpu, want, cb, dtype, (None, None)))
    assert torch.equal(hold[:3], before[:3]) and int(hold[3, 0]) == 2
    # 255 stages in a receiver of 8: nothing beyond the sample's region is read (the next row is 0xFF)
    buf[0, 0], buf[0, 1] = 2, 255
    out, idx_out = _lookup_dgram(gpu, buf.to(gpu), cb, S, dtype, (None, None), hold=hold)
    assert torch.equal(idx_out, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lookup_dgram_refuses_a_field_beyond_K(gpu, dtype):
    """K = 1000, stage 1 of the 3 sent (S = 4) holds 1023: 1 * K + 1023 lies inside the
    codebook (stage 2's rows), so only the guard keeps it out of the sum."""
    D, K, S, sent, bad = 64, 1000, 4, 3, 1
    k, cb, _, _ = _lookup_inputs(gpu, D, K, S)
    assert DR.bits_of(K) == 10 and bad * K + 1023 < S * K
    dgs = []
    for i in range(LK_B):
        body = b""
        for r in range(LK_T):
            rec = 0
            for j in range(sent):
                rec |= (1023 if j == bad else int(k[j, i * LK_T + r])) << (10 * j)
            body += rec.to_bytes(DR.fb(sent, K), "little")
        dgs.append(bytes([2, sent, i, 0]) + body)
    ids = _flat(k, K, [sent] * LK_B)
    ids[bad] = -1
    for i, d in enumerate(dgs):
        assert torch.equal(DR.unpack(d, S, K, LK_T, flatten=True), ids[:, i * LK_T:(i + 1) * LK_T])
    out, idx_out = _lookup_dgram(gpu, DR.buffer(dgs, DR.dgram_bytes(S, K, LK_T)).to(gpu), cb, S, dtype, (None, None))
    ref = _existing_lookup(gpu, ids, cb, dtype, (None, None))
    two = (cb[ids[0].to(gpu)] + cb[ids[2].to(gpu)]).to(dtype)               # and the same two rows added by torch
    assert torch.equal(ref, two) and torch.equal(out, ref) and torch.equal(idx_out, ids)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lookup_dgram_slots(gpu, dtype):
    D, K, S = 8, 16, 17
    k, cb, mean, scale = _lookup_inputs(gpu, D, K, S)
    ms = (mean, scale)
    stages = _mixed(S)
    ids = _flat(k, K, stages)
    dgs = DR.pack(k, stages, [0] * 4, K, LK_T)
    buf = DR.buffer(dgs, DR.dgram_bytes(S, K, LK_T)).to(gpu)
    ref = _existing_lookup(gpu, ids, cb, dtype, ms)
    full = _want_hold(dgs, S, K)
    # NULL: slot i; a permutation: the records land in the permuted rows
    for slots in (None, [2, 0, 3, 1]):
        hold = _hold(gpu, S, K)
        out, idx_out = _lookup_dgram(gpu, buf, cb, S, dtype, ms, slots=slots, hold=hold)
        assert torch.equal(out, ref) and torch.equal(idx_out, ids)
        perm = list(range(4)) if slots is None else slots
        for i, s in enumerate(perm):
            assert torch.equal(hold.cpu()[s], full[i]), (slots, i)
    # -1 and nslots: valid samples still decode, nothing is written through the slot
    hold = _hold(gpu, S, K, fill=0xEE)
    out, idx_out = _lookup_dgram(gpu, buf, cb, S, dtype, ms, slots=[-1, 4, INT_MAX, -INT_MAX], hold=hold)
    assert torch.equal(out, ref) and torch.equal(idx_out, ids) and bool((hold == 0xEE).all())
    # ... and lost ones are the empty sum, whatever the sentinel in hold says
    out, idx_out = _lookup_dgram(gpu, buf, cb, S, dtype, ms, slots=[-1, 4, INT_MAX, -INT_MAX], lost=[1] * 4,
                                 hold=hold)
    none = torch.full_like(ids, -1)
    assert torch.equal(idx_out, none) and torch.equal(out, _existing_lookup(gpu, none, cb, dtype, ms))
    assert bool((hold == 0xEE).all())
    # hold = NULL: lost is the empty sum as well
    out, idx_out = _lookup_dgram(gpu, buf, cb, S, dtype, ms, lost=[0, 1, 0, 1])
    mixed = ids.clone()
    mixed[:, LK_T:2 * LK_T] = -1
    mixed[:, 3 * LK_T:] = -1
    assert torch.equal(idx_out, mixed) and torch.equal(out, _existing_lookup(gpu, mixed, cb, dtype, ms))


@pytest.mark.parametrize("D,K,S", LK_SHAPES)
def test_lookup_dgram_captured_launch_follows_staged_words(gpu, D, K, S):
    from sel import streamops as SO
    k1, cb, mean, scale = _lookup_inputs(gpu, D, K, S, hop=1)
    k2 = _lookup_inputs(gpu, D, K, S, hop=2)[0]
    stride = DR.dgram_bytes(S, K, LK_T)
    dgram = torch.zeros((LK_B, stride), dtype=torch.uint8, device=gpu)
    hold = _hold(gpu, S, K, nslots=6)
    out = torch.full((LK_ROWS, D), float("nan"), dtype=torch.bfloat16, device=gpu)
    idx_out = torch.full((S, LK_ROWS), -7, dtype=torch.int64, device=gpu)
    ctl = torch.zeros(1 + 2 * LK_B, dtype=torch.int32, device=gpu)       # [n, slots..., lost...]
    args = (dgram, cb, S, out, LK_T, mean, scale, ctl[:1], ctl[1:1 + LK_B], ctl[1 + LK_B:], hold, idx_out)
    SO.rvq_lookup_dgram_step(*args)                                       # n = 0: nothing moves
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool((idx_out == -7).all()) and not bool(hold.any())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        SO.rvq_lookup_dgram_step(*args)
    st1, st2 = _mixed(S), list(reversed(_mixed(S)))
    ids1, ids2 = _flat(k1, K, st1), _flat(k2, K, st2)
    held1 = _held_ids(ids1)
    w2 = ids2.clone()
    w2[:, :LK_T] = held1[:, 3 * LK_T:]                     # sample 0 sits on slot 5, where hop 1's sample 3 was held
    w2[:, 2 * LK_T:3 * LK_T] = -1                          # sample 2 sits on slot 0, never written: the empty sum
    w3 = torch.cat([_held_ids(ids2)[:, LK_T:2 * LK_T], held1[:, 3 * LK_T:]], 1)
    sets = [(4, [2, 3, 4, 5], [0, 0, 0, 0], DR.pack(k1, st1, [0] * 4, K, LK_T), ids1),
            (3, [5, 1, 0, 9], [1, 0, 1, 0], DR.pack(k2, st2, [1] * 4, K, LK_T), w2),
            (9, [1, 5, 7, -1], [1, 1, 1, 1], [b"\x02\x01\x00\x00"] * 4, None)]
    for n, slots, lost, dgs, want in sets:
        out.fill_(float("nan"))
        idx_out.fill_(-7)
        dgram.copy_(DR.buffer(dgs, stride, fill=0))
        ctl.copy_(torch.tensor([n] + slots + lost, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        live = min(n, LK_B) * LK_T
        if want is None:                                   # slots 1 and 5 hold hop 2's sample 1 and hop 1's sample 3
            want = torch.full((S, LK_ROWS), -1, dtype=torch.int64)
            want[:, :2 * LK_T] = w3
        ref = _existing_lookup(gpu, want, cb, torch.bfloat16, (mean, scale))
        assert torch.equal(idx_out.cpu()[:, :live], want[:, :live]) and bool((idx_out[:, live:] == -7).all())
        assert torch.equal(out[:live], ref[:live]) and bool(torch.isnan(out[live:].float()).all())


# ---------------------------------------------------------------------------
# C. the bindings refuse bad operands before any launch
# ---------------------------------------------------------------------------
def test_dgram_bindings_refuse_bad_operands(gpu):
    from sel import _lib as L
    from sel import streamops as SO
    z = torch.zeros(4, 8, device=gpu)
    e = torch.zeros(2, 8, 16, device=gpu)                     # S = 2, K = 16: one byte per record, T = 2: 6 bytes
    idx = torch.zeros(2, 4, dtype=torch.int64, device=gpu)
    dg = torch.zeros(2, 6, dtype=torch.uint8, device=gpu)
    wide = torch.zeros(2, 12, dtype=torch.uint8, device=gpu)
    w = torch.zeros(2, dtype=torch.int32, device=gpu)
    SO.rvq_step_dgram(z, e, wide[:, :8], 2, None, w, w, True, idx)            # rows apart from one another: fine
    for bad in (dict(z=z.cpu()), dict(z=z.bfloat16()), dict(z=z[:, :4]), dict(embeds=e.bfloat16()), dict(embeds=e[0]),
                dict(idx=idx.int()), dict(idx=idx[:, :3]), dict(zq=z.bfloat16()), dict(zq=z[:2]),
                dict(rows_per_sample=3), dict(n_active=torch.zeros(1, device=gpu)),
                dict(dgram=None), dict(dgram=dg.cpu()), dict(dgram=dg.int()), dict(dgram=dg[:, :5]), dict(dgram=dg[:1]),
                dict(dgram=wide.view(4, 6)), dict(dgram=dg.view(12)), dict(dgram=wide[:, ::2]),
                dict(stages=w.long()), dict(stages=w[:1]), dict(stages=w.cpu()), dict(stages=w.float()),
                dict(seq=w.long()), dict(seq=w[:1]), dict(seq=w.cpu()),
                dict(embeds=torch.zeros(256, 8, 2, device=gpu), dgram=torch.zeros(2, 80, dtype=torch.uint8, device=gpu),
                     idx=None)):
        a = dict(z=z, embeds=e, dgram=dg, rows_per_sample=2, idx=idx)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_step_dgram(**a)
    cb = torch.zeros(32, 8, device=gpu)
    out = torch.zeros(4, 8, device=gpu)
    m = torch.zeros(8, device=gpu)
    hold = torch.zeros(3, 2, dtype=torch.uint8, device=gpu)
    SO.rvq_lookup_dgram_step(wide[:, :8], cb, 2, out, 2, slots=w, lost=w, hold=hold, idx_out=idx)
    for bad in (dict(dgram=None), dict(dgram=dg.cpu()), dict(dgram=dg.int()), dict(dgram=dg[:, :5]),
                dict(dgram=dg.view(12)), dict(dgram=wide[:, ::2]), dict(codebook=cb.bfloat16()), dict(codebook=cb[:, :4]), dict(codebooks=3),
                dict(codebooks=0), dict(out=out.half()), dict(out=out[:2]), dict(mean=m), dict(scale=m),
                dict(mean=m[:4], scale=m), dict(rows_per_sample=0), dict(rows_per_sample=3),
                dict(n_active=torch.zeros(1, device=gpu)), dict(idx_out=idx.int()), dict(idx_out=idx[:, :3]),
                dict(slots=w.long()), dict(slots=w[:1]), dict(slots=w.cpu()), dict(lost=w.bool()), dict(lost=w[:1]),
                dict(hold=hold.cpu()), dict(hold=hold.int()), dict(hold=hold[:, :1]), dict(hold=hold[:0]),
                dict(hold=hold.view(6))):
        a = dict(dgram=dg, codebook=cb, codebooks=2, out=out, rows_per_sample=2)
        a.update(bad)
        with pytest.raises(L.SelError):
            SO.rvq_lookup_dgram_step(**a)
    torch.cuda.synchronize()
