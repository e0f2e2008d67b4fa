"""CPU checks of the data-parallel codebook update's host side: the rank-ordered
block gather of sel.dist (world-size-2 gloo group on 127.0.0.1, and its identity
form without a group), the new ops' refusal of CPU tensors, the C entry points'
argument validation before any device work, and that switching the sync on or
off adds nothing to a quantizer's state_dict."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD),
                      LOCAL_RANK=str(rank))
    try:
        from sel import dist as D
        D.init_from_env(backend="gloo")
        t = torch.arange(24, dtype=torch.float32).view(2, 3, 4) + 100.0 * rank
        out = D.gather_blocks(t)
        # a non-contiguous input, and an explicit group
        tt = D.gather_blocks(t.transpose(0, 2), process_group=dist.group.WORLD)
        # sync_vq on a CPU quantizer: broadcast from rank 0, sync switched on
        from layers.vq_module import ResidualVQ
        torch.manual_seed(10 + rank)
        M = ResidualVQ(num_quantizers=2, dim=4, codebook_size=8)
        epochs = [l._codebook_epoch for l in M.layers]
        touched = D.sync_vq(M)
        ok = (touched == 2 and M._ema_sync is not None and all(l._ema_sync is not None for l in M.layers)
              and all(l._codebook_epoch == e + 1 for l, e in zip(M.layers, epochs)))
        q.put((rank, out.numpy(), tt.numpy(), torch.stack([l.embed for l in M.layers]).numpy(), ok))
    except Exception as e:  # pragma: no cover - surfaced by the parent
        q.put((rank, e))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gather_blocks_is_rank_ordered_on_both_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for g in got:
        if isinstance(g[1], Exception):
            raise g[1]
    res = {g[0]: g[1:] for g in got}
    base = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    want = torch.stack([base, base + 100.0])
    for r in range(WORLD):
        out, tt, embeds, ok = res[r]
        assert out.shape == (WORLD, 2, 3, 4)
        assert torch.equal(torch.from_numpy(out), want), r
        assert torch.equal(torch.from_numpy(tt), want.transpose(1, 3)), r
        assert ok, r
    # the codebooks came from different random streams and are rank 0's now
    assert torch.equal(torch.from_numpy(res[0][2]), torch.from_numpy(res[1][2]))
    torch.manual_seed(10)
    from layers.vq_module import ResidualVQ
    M0 = ResidualVQ(num_quantizers=2, dim=4, codebook_size=8)
    assert torch.equal(torch.from_numpy(res[1][2]), torch.stack([l.embed for l in M0.layers]))


def test_gather_blocks_is_the_identity_without_a_group():
    from sel import dist as D
    assert not D.is_dist()
    t = torch.arange(6.0).view(2, 3)
    out = D.gather_blocks(t)
    assert out.shape == (1, 2, 3) and torch.equal(out[0], t)
    assert out.data_ptr() == t.data_ptr()    # a view, no copy


def test_sync_vq_does_nothing_without_a_group():
    from layers.vq_module import ResidualVQ
    from sel import dist as D
    M = ResidualVQ(num_quantizers=2, dim=4, codebook_size=8)
    assert D.sync_vq(M) == 0
    assert M._ema_sync is None and all(l._ema_sync is None for l in M.layers)


def test_new_ops_refuse_cpu_tensors():
    from layers.vq_module import ResidualVQ
    from sel import _lib as L
    from sel.vqops import rvq_ema_apply, rvq_ema_stats
    M = ResidualVQ(num_quantizers=2, dim=4, codebook_size=8)
    x = torch.zeros(6, 4)
    stack = torch.stack([l.embed for l in M.layers])
    idx = torch.zeros(2, 6, dtype=torch.int64)
    with pytest.raises(L.SelError, match="CPU tensor"):
        rvq_ema_stats(x, stack, idx, nseg=2)
    with pytest.raises(L.SelError, match="CPU tensor"):
        rvq_ema_apply(torch.zeros(1, 2, 5, 8), list(M.layers), [True, True])


def test_enable_and_disable_leave_the_state_dict_alone():
    from layers.vq_module import ResidualVQ, VectorQuantize
    for M in (ResidualVQ(num_quantizers=2, dim=4, codebook_size=8), VectorQuantize(dim=4, codebook_size=8)):
        keys = list(M.state_dict().keys())
        M.enable_ema_sync(segments=2)
        assert M._ema_sync == (None, 2)
        assert list(M.state_dict().keys()) == keys
        M.load_state_dict(M.state_dict(), strict=True)
        M.disable_ema_sync()
        assert M._ema_sync is None
        assert list(M.state_dict().keys()) == keys


# ---- the C entry points: every refusal happens before any device work --------
N, D_, S, K = 64, 64, 3, 256


class Stage(ctypes.Structure):  # sel_rvq_ema_stage (include/sel.h)
    _fields_ = [("embed", ctypes.c_void_p), ("cluster_size", ctypes.c_void_p), ("embed_avg", ctypes.c_void_p),
                ("update", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@pytest.fixture(scope="module")
def lib():
    from sel import _lib
    return _lib.load()


def test_sync_symbols_exported(lib):
    from sel import _lib
    for name in ("sel_rvq_ema_stats_floats", "sel_rvq_ema_stats_workspace", "sel_rvq_ema_stats",
                 "sel_rvq_ema_apply"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.sel_rvq_ema_stats_floats(64, 8, 1024) == 8 * 65 * 1024
    assert lib.sel_rvq_ema_stats_workspace(5120, 64, 8, 1024) >= 5120 * 64 * 8 * 4


def _stats(lib, n=N, d=D_, s=S, k=K, nseg=1, ws_bytes=None):
    """Every device pointer is null: no call here can reach the device even if a
    check were missing (the pointers are checked last)."""
    need = lib.sel_rvq_ema_stats_workspace(max(n, 1), min(d, 256), min(s, 16), k)
    return lib.sel_rvq_ema_stats(None, n, d, None, s, k, None, nseg, None, None,
                                 need if ws_bytes is None else ws_bytes, None)


def _codes():
    """SEL_ERR_* as include/sel.h defines them"""
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(os.path.dirname(here), "include", "sel.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SEL_ERR_\w+)\s*=\s*(-?\d+)", text)}


@pytest.mark.parametrize("case, kwargs, code, says", [
    ("N = 0", dict(n=0), "SEL_ERR_ARG", "N=0"),
    ("D = 257", dict(d=257), "SEL_ERR_ARG", "D=257"),
    ("S = 17", dict(s=17), "SEL_ERR_ARG", "S=17"),
    ("nseg = 0", dict(nseg=0), "SEL_ERR_ARG", "segments"),
    ("nseg = -1", dict(nseg=-1), "SEL_ERR_ARG", "segments"),
    ("ragged segments", dict(n=37, nseg=2), "SEL_ERR_ARG", "segments"),
    ("segment over 2^24 rows", dict(n=(1 << 24) + 1, d=1, s=1, k=2), "SEL_ERR_ARG", "segments"),
    ("short workspace", dict(ws_bytes=N * D_ * S * 4 - 1), "SEL_ERR_WORKSPACE", "workspace"),
    ("null pointers", dict(), "SEL_ERR_ARG", "null pointer"),
])
def test_stats_refuses_before_device_work(lib, case, kwargs, code, says):
    rc = _stats(lib, **kwargs)
    assert rc == _codes()[code], (case, rc)
    assert says in lib.sel_last_error().decode(), (case, lib.sel_last_error())


def _apply(lib, nblk=1, d=D_, s=S, k=K, table=True, stats=1, update=0):
    tab = (Stage * 16)()
    for i in range(16):
        tab[i].update = update
    return lib.sel_rvq_ema_apply(ctypes.c_void_p(stats) if stats else None, nblk, d, s, k,
                                 ctypes.cast(tab, ctypes.c_void_p) if table else None, 0.8, 1e-5, None)


@pytest.mark.parametrize("case, kwargs, says", [
    ("nblk = 0", dict(nblk=0), "blocks"),
    ("D = 0", dict(d=0), "D=0"),
    ("S = 17", dict(s=17), "S=17"),
    ("null table", dict(table=False), "table"),
    ("null stats", dict(stats=0), "null pointer"),
    ("null stage buffer", dict(update=1), "null buffer in stage 0"),
])
def test_apply_refuses_before_device_work(lib, case, kwargs, says):
    rc = _apply(lib, **kwargs)
    assert rc == _codes()["SEL_ERR_ARG"], (case, rc)
    assert says in lib.sel_last_error().decode(), (case, lib.sel_last_error())


def test_apply_with_no_updating_stage_is_a_no_op(lib):
    # every stage in eval mode: SEL_OK without touching the device (stats is a
    # dangling non-null address here, so a launch would not go unnoticed)
    assert _apply(lib, update=0) == 0
