"""The data-parallel codebook update on the GPU: sel_rvq_ema_stats /
sel_rvq_ema_apply (csrc/vq_ema_sync.hip), ResidualVQ.enable_ema_sync,
sel.dist.gather_blocks / sync_vq and the stage-1 trainer under a process group.

Inputs are the committed fixtures of tests/test_gpu_vq_train.py (the
reference's own runs): cases (N, D, K, S, steps) c0 (150, 64, 256, 3, 3), c1
(150, 64, 8, 2, 2: nearly all rows on one code), c2 (37, 6, 1000, 2, 2), c3
(130, 130, 40, 2, 2: the D > 64 path), and the trainer fixture (2 clips x 3600
samples).

Bounds.  Buffers against fp64 and against the fixture: that module's
max(1e-6, 3 x e32.<name>), unchanged -- a segmented sum (per-segment chains
added in segment order) does not round worse than the single chain the bound
was made for.  The one-segment pair against the fused update, two runs, two
ranks, and two ranks against one process with ``segments=2``: bit equality.
The trainer under two ranks against one process on both clips:
tests/test_gpu_ddp.py's criteria (step-0 gradients 1e-6 norm-wise, rank-mean
losses 1e-5, weight update 1e-3 norm-wise and at most 2 % of the weights off by
more than half a learning rate).

The fp64 restatement of the segmented update is ``ema64_segmented`` below:
test_gpu_vq_train.ema64 with the per-segment sums added in segment order.
"""
import copy
import ctypes
import functools
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import test_gpu_vq_train as T
from test_gpu_vq_train import BUFS, rel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "vq_sync_worker.py")


def ema64_segmented(x, state, idx, decay, eps, nseg, update=None):
    """test_gpu_vq_train.ema64 with the sums and counts formed per segment of
    N / nseg rows and added in segment order (in fp64 the order is immaterial to
    the bound; it is kept for the restatement to say what the kernels do)."""
    r = x.double().cpu()
    N = r.shape[0]
    assert N % nseg == 0
    n = N // nseg
    new = []
    for s, st in enumerate(state):
        K = st["cluster_size"].numel()
        ind = idx[s].cpu().long()
        if update is None or update[s]:
            counts = torch.zeros(K, dtype=torch.float64)
            esum = torch.zeros_like(st["embed_avg"])
            for g in range(nseg):
                sl = slice(g * n, (g + 1) * n)
                counts = counts + torch.bincount(ind[sl], minlength=K).double()
                esum = esum + torch.zeros_like(esum).index_add_(1, ind[sl], r[sl].t())
            csz = st["cluster_size"] * decay + counts * (1 - decay)
            eavg = st["embed_avg"] * decay + esum * (1 - decay)
            new.append({"cluster_size": csz, "embed_avg": eavg, "embed": T._embed64(csz, eavg, eps)})
        else:
            new.append(dict(st))
        q = st["embed"].t()[ind]                 # the pre-update codebook picks the code
        r = r - (r + (q - r))
    return new


def _cfg(c):
    return tuple(int(v) for v in c["cfg"])


def _forward(M, x):
    """What _train_forward does before the update: the assignment on the
    pre-update stack; returns (x the kernel read, stack, idx)."""
    from sel.vqops import ResidualVQFn
    aux = {}
    stack = torch.stack([l.embed for l in M.layers])
    with torch.no_grad():
        _, _, _, idx = ResidualVQFn.apply(x, stack, M.layers[0].commitment, aux)
    return aux["x"], stack, idx


def _nan_stats(nseg, S, D, K, dev):
    return torch.full((nseg, S, D + 1, K), float("nan"), dtype=torch.float32, device=dev)


def _stats_into(stats, x, stack, idx, nseg):
    """sel_rvq_ema_stats into a caller's (pre-filled) buffer"""
    from sel import _lib as L
    S, D, K = stack.shape
    N = x.shape[0]
    ws = L.workspace(L.lib().sel_rvq_ema_stats_workspace(N, D, S, K), x.device)
    L.call("sel_rvq_ema_stats", L.ptr(x), N, D, L.ptr(stack), S, K, L.ptr(idx), nseg, L.ptr(stats), L.ptr(ws),
           ws.numel(), L.stream())
    return stats


@pytest.mark.parametrize("name", T.CASES)
def test_one_segment_pair_gives_the_fused_updates_bits(gpu, name):
    """1. nseg = nblk = 1 on every step of c0-c3: stats (into a NaN-filled
    buffer) + apply on one module, the fused update on its twin; all three
    buffers of every layer equal bit for bit after every step."""
    from sel.vqops import rvq_ema_apply
    c = T._case(name)
    N, D, K, S, steps = _cfg(c)
    A, B = T._module(c, gpu), T._module(c, gpu)
    for t in range(steps):
        x = T._x(c, t, gpu)
        xk, stack, idx = _forward(A, x)
        stats = _stats_into(_nan_stats(1, S, D, K, gpu), xk, stack, idx, 1)
        assert not torch.isnan(stats).any(), (name, t)
        rvq_ema_apply(stats, list(A.layers), [True] * S)
        for l in A.layers:
            l.invalidate_codebook()
        with torch.no_grad():
            B(x)
        for i, (sa, sb) in enumerate(zip(T._state(A), T._state(B))):
            for b in BUFS:
                assert torch.equal(sa[b], sb[b]), (name, t, i, b, rel(sa[b], sb[b]))
    assert not torch.equal(A.layers[0].embed.cpu(), torch.from_numpy(c["init.embed.0"].astype(np.float32)))


def test_one_segment_pair_with_a_mixed_update_mask(gpu):
    """1. (continued) c0 with update = [1, 0, 1]: stage 1 keeps its bits, stages
    0 and 2 get the fused update's."""
    from sel.vqops import rvq_ema_apply
    c = T._case("c0")
    N, D, K, S, steps = _cfg(c)
    A, B = T._module(c, gpu), T._module(c, gpu)
    B.layers[1].eval()
    for t in range(steps):
        x = T._x(c, t, gpu)
        before = T._state(A)
        xk, stack, idx = _forward(A, x)
        stats = _stats_into(_nan_stats(1, S, D, K, gpu), xk, stack, idx, 1)
        rvq_ema_apply(stats, list(A.layers), [1, 0, 1])
        for l in A.layers:
            l.invalidate_codebook()
        with torch.no_grad():
            B(x)
        after = T._state(A)
        for b in BUFS:
            assert torch.equal(after[1][b], before[1][b]), (t, b)
            for i in range(S):
                assert torch.equal(after[i][b], T._state(B)[i][b]), (t, i, b)
        assert not torch.equal(after[0]["embed"], before[0]["embed"])


@functools.lru_cache(maxsize=None)
def _segmented_run(name, nseg, which=0):
    """One training-mode run of the case with ``enable_ema_sync(segments=nseg)``
    and no process group (nblk = nseg), shared by the tests: per step the
    indices, the stats' count planes summed over blocks, and the buffers."""
    from sel.vqops import rvq_ema_stats
    dev = torch.device("cuda:0")
    c = T._case(name)
    N, D, K, S, steps = _cfg(c)
    M = T._module(c, dev)
    M.enable_ema_sync(segments=nseg)
    rec = []
    for t in range(steps):
        x = T._x(c, t, dev)
        xk, stack, idx = _forward(M, x)
        stats = rvq_ema_stats(xk, stack, idx, nseg)
        assert tuple(stats.shape) == (nseg, S, D + 1, K)
        with torch.no_grad():
            M(x)
        rec.append(dict(idx=idx.cpu(), counts=stats[:, :, D, :].double().sum(0).cpu(),
                        state=[{b: v.cpu() for b, v in st.items()} for st in T._state(M)]))
    return rec


SEGMENTED = [("c0", 2), ("c0", 3), ("c0", 5), ("c1", 2), ("c3", 2)]


@pytest.mark.parametrize("name, nseg", SEGMENTED)
def test_segmented_update_matches_fp64_and_the_fixture(gpu, name, nseg):
    """2. nblk = nseg segments in one process: the buffers against the segmented
    fp64 restatement chained on the GPU's own indices and against the
    reference's fixture, both within max(1e-6, 3 x e32); two runs give the same
    bits; the count planes summed over blocks are bincount(idx) exactly."""
    c = T._case(name)
    N, D, K, S, steps = _cfg(c)
    decay, eps = float(c["decay"]), float(c["eps"])
    run = _segmented_run(name, nseg)
    again = _segmented_run(name, nseg, 1)
    e0 = [torch.from_numpy(c[f"init.embed.{i}"].astype(np.float64)) for i in range(S)]
    state = [{"cluster_size": torch.zeros(K, dtype=torch.float64), "embed_avg": e.clone(), "embed": e.clone()}
             for e in e0]
    for t, r in enumerate(run):
        assert torch.equal(r["idx"], torch.from_numpy(c[f"idx.{t}"].astype(np.int64))), (name, t)
        for s in range(S):
            assert torch.equal(r["counts"][s], torch.bincount(r["idx"][s], minlength=K).double()), (name, t, s)
        state = ema64_segmented(T._x(c, t, "cpu"), state, r["idx"], decay, eps, nseg)
        for i in range(S):
            csz = torch.from_numpy(c[f"cluster_size.{t}.{i}"]).double()
            eavg = torch.from_numpy(c[f"embed_avg.{t}.{i}"]).double()
            fixture = {"cluster_size": csz, "embed_avg": eavg, "embed": T._embed64(csz, eavg, eps)}
            for b in BUFS:
                bound = T._bound(c, b, t, i)
                e64, efx = rel(r["state"][i][b], state[i][b]), rel(r["state"][i][b], fixture[b])
                print(f"{name} nseg {nseg} step {t} layer {i} {b}: fp64 {e64:.2e} fixture {efx:.2e} "
                      f"(bound {bound:.1e})")
                assert e64 <= bound, (name, nseg, t, i, b, e64)
                assert efx <= bound, (name, nseg, t, i, b, efx)
                assert torch.equal(r["state"][i][b], again[t]["state"][i][b]), (name, nseg, t, i, b)


def _codes():
    import re
    text = open(os.path.join(os.path.dirname(HERE), "include", "sel.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SEL_ERR_\w+)\s*=\s*(-?\d+)", text)}


def test_refusals_write_nothing(gpu):
    """3. c2 (37 rows) at nseg = 2, nseg = 0, a short workspace; nblk = 0 and a
    null stage buffer: the documented code, stats (NaN-filled) and the codebook
    buffers untouched."""
    from sel import _lib as L
    from sel.vqops import _EmaStage
    code = _codes()
    c = T._case("c2")
    N, D, K, S, steps = _cfg(c)
    M = T._module(c, gpu)
    xk, stack, idx = _forward(M, T._x(c, 0, gpu))
    lib = L.lib()
    need = lib.sel_rvq_ema_stats_workspace(N, D, S, K)
    ws = L.workspace(need, gpu)
    stats = _nan_stats(2, S, D, K, gpu)

    def stats_call(nseg, ws_bytes):
        return lib.sel_rvq_ema_stats(L.ptr(xk), N, D, L.ptr(stack), S, K, L.ptr(idx), nseg, L.ptr(stats), L.ptr(ws),
                                     ws_bytes, L.stream())
    assert N % 2 == 1
    assert stats_call(2, need) == code["SEL_ERR_ARG"]
    assert stats_call(0, need) == code["SEL_ERR_ARG"]
    assert stats_call(1, need - 1) == code["SEL_ERR_WORKSPACE"]
    torch.cuda.synchronize()
    assert torch.isnan(stats).all()

    good = _stats_into(_nan_stats(1, S, D, K, gpu), xk, stack, idx, 1)
    before = T._state(M)

    def table(null_in=None):
        tab = (_EmaStage * S)()
        for s, l in enumerate(M.layers):
            tab[s] = _EmaStage(l.embed.data_ptr(), l.cluster_size.data_ptr(),
                               None if s == null_in else l.embed_avg.data_ptr(), 1, 0)
        return tab

    def apply_call(nblk, tab):
        return lib.sel_rvq_ema_apply(L.ptr(good), nblk, D, S, K, ctypes.cast(tab, ctypes.c_void_p) if tab else None,
                                     float(M.layers[0].decay), float(M.layers[0].eps), L.stream())
    assert apply_call(0, table()) == code["SEL_ERR_ARG"]
    assert apply_call(1, table(null_in=S - 1)) == code["SEL_ERR_ARG"]     # stage 0 is fine: still nothing written
    assert apply_call(1, None) == code["SEL_ERR_ARG"]
    torch.cuda.synchronize()
    assert T._equal_states(T._state(M), before)
    with pytest.raises(L.SelError):
        from sel.vqops import rvq_ema_stats
        rvq_ema_stats(xk, stack, idx, 2)
    assert apply_call(1, table()) == 0                                   # and the valid call does write
    torch.cuda.synchronize()
    assert not T._equal_states(T._state(M), before)


def test_segmented_forward_is_capturable(gpu):
    """4. single-process segments = 2: two replays of a captured training-mode
    forward equal two eager steps from the same state (out and every buffer),
    with the existing capture test's stream setup."""
    c = T._case("c0")
    xs = T._x(c, 0, gpu)
    A = T._module(c, gpu)
    A.enable_ema_sync(segments=2)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            A(xs)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    B = copy.deepcopy(A)                      # the state the capture starts from
    assert B._ema_sync == (None, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out_s, losses_s, ppls_s = A(xs)
    assert T._equal_states(T._state(A), T._state(B))   # capturing ran nothing
    start = T._state(B)
    for step in range(2):
        graph.replay()
        with torch.no_grad():
            out_e, losses_e, ppls_e = B(xs)
        torch.cuda.synchronize(gpu)
        assert torch.equal(out_s, out_e) and torch.equal(losses_s, losses_e) and torch.equal(ppls_s, ppls_e), step
        assert T._equal_states(T._state(A), T._state(B)), step
    assert not T._equal_states(T._state(A), start)
    # the segmented path ran: its bits are the shared segments = 2 run's, three steps in
    C = T._module(c, gpu)
    C.enable_ema_sync(segments=2)
    with torch.no_grad():
        for t in range(3):
            C(T._x(c, t, gpu))
    ref = _segmented_run("c0", 2)[-1]["state"]
    assert all(torch.equal(sa[b].cpu(), sb[b]) for sa, sb in zip(T._state(C), ref) for b in BUFS)


# ---- two real ranks ------------------------------------------------------------
CHILD_TIMEOUT = 240   # seconds, each child's own limit
_FAILED = []          # a launch that failed: nothing is launched after it


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(mode, tmp, world=2):
    """Both ranks as fresh child processes; the launcher polls them, and on the
    first non-zero exit or expired limit kills the other."""
    if _FAILED:
        pytest.fail(f"not launched: an earlier launch failed ({_FAILED[0]})")
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        log = open(tmp / f"{mode}_rank{r}.log", "w")
        procs.append((subprocess.Popen([sys.executable, "-u", WORKER, mode, str(tmp / f"{mode}_rank{r}.pt")],
                                       env=env, stdout=log, stderr=subprocess.STDOUT), log))
    deadline = time.monotonic() + CHILD_TIMEOUT
    why = None
    try:
        while why is None:
            rcs = [p.poll() for p, _ in procs]
            if any(rc not in (None, 0) for rc in rcs):
                why = f"ranks exited {rcs}"
            elif all(rc == 0 for rc in rcs):
                break
            elif time.monotonic() > deadline:
                why = f"time limit of {CHILD_TIMEOUT} s (exit codes so far {rcs})"
            else:
                time.sleep(0.05)
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    if why is not None:
        _FAILED.append(f"{mode}: {why}")
        logs = "\n".join((tmp / f"{mode}_rank{r}.log").read_text()[-3000:] for r in range(world))
        raise AssertionError(f"{mode}: {why}\n{logs}")
    return [torch.load(tmp / f"{mode}_rank{r}.pt", weights_only=True) for r in range(world)]


@pytest.fixture(scope="module")
def ranks(gpu, tmp_path_factory):
    """The one launch of both ranks in mode "all"."""
    res = _launch("all", tmp_path_factory.mktemp("vq_sync"))
    assert [tuple(r["rank_world"]) for r in res] == [(0, 2), (1, 2)]
    return res


@pytest.fixture(scope="module")
def ranks_nosync(gpu, ranks, tmp_path_factory):
    """The negative control's launch (after, and only after, the main one)."""
    return _launch("nosync", tmp_path_factory.mktemp("vq_nosync"))


def _fixture_state(c, t, i):
    csz = torch.from_numpy(c[f"cluster_size.{t}.{i}"]).double()
    eavg = torch.from_numpy(c[f"embed_avg.{t}.{i}"]).double()
    return {"cluster_size": csz, "embed_avg": eavg, "embed": T._embed64(csz, eavg, float(c["eps"]))}


@pytest.mark.parametrize("name", ["c0", "c1", "c3"])
def test_two_ranks_keep_one_codebook(gpu, ranks, name):
    """5a. each rank on its half of every x.t under sync_vq (rank 1's codebooks
    re-randomised before it): both ranks' buffers equal bit for bit, equal to
    this process's segments = 2 run on the whole batch, within the bound of the
    reference's fixture; the indices are the fixture's."""
    c = T._case(name)
    N, D, K, S, steps = _cfg(c)
    r0, r1 = (r["vq"][name] for r in ranks)
    one = _segmented_run(name, 2)
    assert len(r0) == len(r1) == steps
    for t in range(steps):
        want_idx = torch.from_numpy(c[f"idx.{t}"].astype(np.int64))
        assert torch.equal(torch.cat([r0[t]["idx"], r1[t]["idx"]], dim=1), want_idx), (name, t)
        for i in range(S):
            fx = _fixture_state(c, t, i)
            for b in BUFS:
                assert torch.equal(r0[t]["state"][i][b], r1[t]["state"][i][b]), (name, t, i, b)
                assert torch.equal(r0[t]["state"][i][b], one[t]["state"][i][b]), (name, t, i, b)
                e = rel(r0[t]["state"][i][b], fx[b])
                print(f"{name} step {t} layer {i} {b}: {e:.2e} (bound {T._bound(c, b, t, i):.1e})")
                assert e <= T._bound(c, b, t, i), (name, t, i, b, e)


def test_without_the_sync_the_ranks_drift(gpu, ranks_nosync):
    """Negative control: the same two ranks on c0 without sync_vq.  Their
    ``embed`` differ, and rank 0's is off the fixture by more than the bound: the
    data sees the drift the feature removes."""
    c = T._case("c0")
    N, D, K, S, steps = _cfg(c)
    r0, r1 = (r["vq"]["c0"] for r in ranks_nosync)
    want_idx = torch.from_numpy(c["idx.0"].astype(np.int64))
    assert torch.equal(torch.cat([r0[0]["idx"], r1[0]["idx"]], dim=1), want_idx)   # same start, same assignment
    for t in range(steps):
        for i in range(S):
            assert not torch.equal(r0[t]["state"][i]["embed"], r1[t]["state"][i]["embed"]), (t, i)
            e = rel(r0[t]["state"][i]["embed"], _fixture_state(c, t, i)["embed"])
            print(f"no sync, step {t} layer {i} embed: {e:.2e} (bound {T._bound(c, 'embed', t, i):.1e})")
            assert e > T._bound(c, "embed", t, i), (t, i, e)


@functools.lru_cache(maxsize=None)
def _trainer_one_process():
    import vq_sync_worker as W
    res = W.run_trainer(torch.device("cuda:0"), segments=2)
    torch.cuda.synchronize()
    return res


def test_two_ranks_train_stage_one_like_one_process(gpu, ranks):
    """5b. trainer/autoencoder.Trainer._train_step, three steps, generator and
    discriminator under wrap_ddp with one clip per rank, against one process on
    both clips with segments = 2."""
    from conftest import golden
    import vq_sync_worker as W
    g = golden("autoencoder_trainer_step")
    t0, t1 = (r["trainer"] for r in ranks)
    ref = _trainer_one_process()
    # the replicas stay identical: parameters, codebook buffers, all-reduced gradients
    for k, v in t0["params"].items():
        assert torch.equal(v, t1["params"][k]), k
    for k, v in t0["grads"].items():
        assert torch.equal(v, t1["grads"][k]), k
    for s in range(W.TRAINER_STEPS):
        for i in range(2):
            for b in BUFS:
                assert torch.equal(t0["steps"][s]["state"][i][b], t1["steps"][s]["state"][i][b]), (s, i, b)
    # the quantizer's indices: the fixture's, each rank its clip's rows
    for s in range(W.TRAINER_STEPS):
        ncall = 2 if s == 2 else 1
        assert len(t0["steps"][s]["idx"]) == len(t1["steps"][s]["idx"]) == len(ref["steps"][s]["idx"]) == ncall
        for cidx in range(ncall):
            want = torch.from_numpy(g[f"idx.{s}.{cidx}"].astype(np.int64))
            got = torch.cat([t0["steps"][s]["idx"][cidx], t1["steps"][s]["idx"][cidx]], dim=1)
            assert torch.equal(got, want), (s, cidx)
            assert torch.equal(ref["steps"][s]["idx"][cidx], want), (s, cidx)
    # the codebook buffers after steps 0 and 1 against the reference's; step 2 leaves them alone
    for s in range(2):
        assert t0["steps"][s]["training"]
        for i in range(2):
            for b in BUFS:
                bound = max(1e-6, 3.0 * float(g[f"e32.buf.{s}.{i}.{b}"]))
                e = rel(t0["steps"][s]["state"][i][b], g[f"buf.{s}.{i}.{b}"])
                eo = rel(ref["steps"][s]["state"][i][b], g[f"buf.{s}.{i}.{b}"])
                print(f"step {s} codebook {i} {b}: two ranks {e:.2e}, one process {eo:.2e} (bound {bound:.1e})")
                assert e <= bound, (s, i, b, e)
                assert eo <= bound, (s, i, b, eo)
    assert not t0["steps"][2]["training"]
    for i in range(2):
        for b in BUFS:
            assert torch.equal(t0["steps"][2]["state"][i][b], t0["steps"][1]["state"][i][b]), (i, b)
    # step-0 gradients after the all-reduce against the one process's
    assert set(t0["grads"]) == set(ref["grads"]) and t0["grads"]
    num = sum(((t0["grads"][k].double() - v.double()) ** 2).sum().item() for k, v in ref["grads"].items())
    den = sum((v.double() ** 2).sum().item() for v in ref["grads"].values())
    gerr = (num / den) ** 0.5
    print(f"step-0 generator gradients, two ranks vs one process: {gerr:.2e}")
    assert gerr <= 1e-6, gerr
    # every logged loss term is a shard mean: the mean over ranks is the one process's value
    for s in range(W.TRAINER_STEPS):
        assert set(t0["steps"][s]["losses"]) == set(ref["steps"][s]["losses"]) and ref["steps"][s]["losses"]
        for k, v in ref["steps"][s]["losses"].items():
            got = 0.5 * (t0["steps"][s]["losses"][k] + t1["steps"][s]["losses"][k])
            print(f"step {s} {k}: ranks' mean {got:.8g}, one process {v:.8g}")
            assert abs(got - v) <= 1e-5 * abs(v) + 1e-7, (s, k, got, v)
    # the weight updates of the three steps
    for prefix, lr in (("G.", W.LR_G), ("D.", W.LR_D)):
        flips = tot = 0
        num = den = 0.0
        for k, v in ref["params"].items():
            if not k.startswith(prefix):
                continue
            assert torch.equal(t0["p0"][k], ref["p0"][k]), k
            du_ref = v.double() - ref["p0"][k].double()
            du = t0["params"][k].double() - t0["p0"][k].double()
            flips += ((du - du_ref).abs() > 0.5 * lr).sum().item()
            tot += du.numel()
            num += ((du - du_ref) ** 2).sum().item()
            den += (du_ref ** 2).sum().item()
        print(f"{prefix} three-step update: {flips} of {tot} off by > 0.5 lr, norm-wise {(num / den) ** 0.5:.2e}")
        assert tot > 0 and flips <= 0.02 * tot, (prefix, flips, tot)
        assert (num / den) ** 0.5 <= 1e-3, (prefix, (num / den) ** 0.5)
