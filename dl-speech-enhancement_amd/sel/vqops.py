"""Autograd op over the residual-VQ kernel (layers/vq_module.py:61-88, :119-134)."""
import ctypes

import torch

from . import _lib as L


class ResidualVQFn(torch.autograd.Function):
    """(x (N, D), embeds (S, D, K)) -> (out (N, D), losses (S,), ppls (S,), idx (S, N))."""

    @staticmethod
    def forward(ctx, x, embeds, commitment, aux=None):
        """``aux`` (a dict, optional) receives what the training-mode codebook
        update needs beside the four outputs: the contiguous fp32 ``x`` the kernel
        read and the code histogram ``counts`` (S, K)."""
        L.need_device(x, embeds)
        # the kernel reads embeds as fp32 (S, D, K) memory with x's D: anything
        # else would be read past its end
        if x.dim() != 2:
            raise L.SelError(f"ResidualVQFn: x must be (N, D), got {tuple(x.shape)}")
        if embeds.dim() != 3 or embeds.dtype != torch.float32 or embeds.shape[1] != x.shape[1]:
            raise L.SelError(f"ResidualVQFn: embeds must be an fp32 (S, D, K) stack with D = {x.shape[1]}, got "
                             f"{embeds.dtype} {tuple(embeds.shape)}")
        x = x.contiguous().float()
        embeds = embeds.contiguous()
        N, D = x.shape
        S, _, K = embeds.shape
        dev = x.device
        out = torch.empty_like(x)
        idx = torch.empty((S, N), dtype=torch.int64, device=dev)
        counts = torch.empty((S, K), dtype=torch.int32, device=dev)
        sqerr = torch.empty(S, dtype=torch.float64, device=dev)
        ws = L.workspace(L.lib().sel_rvq_workspace(N, S, K), dev)
        L.call("sel_rvq_fwd", L.ptr(x), N, D, L.ptr(embeds), S, K, L.ptr(out), L.ptr(idx), L.ptr(counts),
               L.ptr(sqerr), L.ptr(ws), ws.numel(), L.stream())
        loss = torch.empty(S, dtype=torch.float32, device=dev)
        ppl = torch.empty(S, dtype=torch.float32, device=dev)
        L.call("sel_rvq_finish", L.ptr(counts), L.ptr(sqerr), N, D, S, K, float(commitment), L.ptr(loss),
               L.ptr(ppl), L.stream())
        ctx.save_for_backward(x, embeds, idx)
        ctx.commitment = float(commitment)
        ctx.mark_non_differentiable(ppl, idx)
        # the perplexities / indices (and an unused loss) take no gradient:
        # None in backward instead of materialised zero tensors (two fill
        # launches per step)
        ctx.set_materialize_grads(False)
        ctx.counts = counts
        ctx.has_aux = aux is not None
        if aux is not None:
            aux["x"], aux["counts"] = x, counts
        return out, loss, ppl, idx

    @staticmethod
    def backward(ctx, g_out, g_loss, g_ppl, g_idx):
        x, embeds, idx = ctx.saved_tensors
        N, D = x.shape
        K = embeds.shape[2]
        gx = torch.empty_like(x)
        go = g_out.contiguous() if g_out is not None else None
        gl = g_loss.contiguous() if g_loss is not None else None
        L.call("sel_rvq_bwd", L.ptr(x), N, D, L.ptr(embeds[0]), K, L.ptr(idx[0]), L.ptr(go), L.ptr(gl),
               ctx.commitment, L.ptr(gx), L.stream())
        return (gx, None, None, None) if ctx.has_aux else (gx, None, None)


class _EmaStage(ctypes.Structure):
    """sel_rvq_ema_stage (include/sel.h)"""
    _fields_ = [("embed", ctypes.c_void_p), ("cluster_size", ctypes.c_void_p), ("embed_avg", ctypes.c_void_p),
                ("update", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@torch.no_grad()
def rvq_ema_update(x, stack, idx, counts, layers, update=None):
    """The EMA codebook update of every training-mode layer (vq_module.py:74-80)
    after one ResidualVQFn forward, in one C call: x (N, D) fp32 and the stack
    (S, D, K) are what the forward read, idx / counts what it wrote.  ``layers``
    own the buffers (one per layer: they are state_dict entries); ``update[s]``
    (default: ``layers[s].training``) selects the stages written.  The stack is
    left untouched: the backward reads it."""
    L.need_device(x, stack, idx, counts)
    S, D, K = stack.shape
    N = x.shape[0]
    if len(layers) != S or x.shape[1] != D or tuple(idx.shape) != (S, N) or tuple(counts.shape) != (S, K):
        raise L.SelError(f"rvq_ema_update: shapes disagree (x {tuple(x.shape)}, stack {tuple(stack.shape)}, "
                         f"idx {tuple(idx.shape)}, counts {tuple(counts.shape)}, {len(layers)} layers)")
    if not (x.is_contiguous() and stack.is_contiguous() and idx.is_contiguous() and counts.is_contiguous()
            and x.dtype == torch.float32 and stack.dtype == torch.float32):
        raise L.SelError("rvq_ema_update: needs the forward's own contiguous fp32 tensors")
    update = [l.training for l in layers] if update is None else list(update)
    decay, eps = layers[0].decay, layers[0].eps
    tab = (_EmaStage * S)()
    for s, (l, u) in enumerate(zip(layers, update)):
        if (l.decay, l.eps) != (decay, eps):
            raise L.SelError("rvq_ema_update: the layers' decay / eps differ")
        for b in (l.embed, l.cluster_size, l.embed_avg):
            L.need_device(b)
            if not (b.is_contiguous() and b.dtype == torch.float32):
                raise L.SelError("rvq_ema_update: codebook buffers must be contiguous fp32")
        if (tuple(l.embed.shape) != (D, K) or tuple(l.embed_avg.shape) != (D, K)
                or tuple(l.cluster_size.shape) != (K,) or l.embed.data_ptr() == stack[s].data_ptr()):
            raise L.SelError("rvq_ema_update: a layer's embed / embed_avg must be (D, K), its cluster_size (K), "
                             "and embed must not alias the stack")
        tab[s] = _EmaStage(l.embed.data_ptr(), l.cluster_size.data_ptr(), l.embed_avg.data_ptr(), int(bool(u)), 0)
    ws = L.workspace(L.lib().sel_rvq_ema_workspace(N, D, S, K), x.device)
    L.call("sel_rvq_ema_update", L.ptr(x), N, D, L.ptr(stack), S, K, L.ptr(idx), L.ptr(counts),
           ctypes.cast(tab, ctypes.c_void_p), float(decay), float(eps), L.ptr(ws), ws.numel(), L.stream())


@torch.no_grad()
def rvq_ema_stats(x, stack, idx, nseg=1):
    """The statistics of the EMA codebook update (vq_module.py:74-80) on their
    own, after one ResidualVQFn forward: (nseg, S, D + 1, K) fp32, block g
    holding, per stage, the per-code sums of the residual rows of segment g (rows
    [g N / nseg, (g + 1) N / nseg), planes 0..D-1) and their counts (plane D).
    Every element is written.  ``rvq_ema_apply`` folds such blocks -- this
    process's, or all ranks' gathered in rank order -- into the codebooks."""
    L.need_device(x, stack, idx)
    S, D, K = stack.shape
    N = x.shape[0]
    if x.dim() != 2 or x.shape[1] != D or tuple(idx.shape) != (S, N):
        raise L.SelError(f"rvq_ema_stats: shapes disagree (x {tuple(x.shape)}, stack {tuple(stack.shape)}, "
                         f"idx {tuple(idx.shape)})")
    if not (x.is_contiguous() and stack.is_contiguous() and idx.is_contiguous() and x.dtype == torch.float32
            and stack.dtype == torch.float32 and idx.dtype == torch.int64):
        raise L.SelError("rvq_ema_stats: needs the forward's own contiguous fp32 tensors and int64 indices")
    nseg = int(nseg)
    stats = torch.empty((max(nseg, 0), S, D + 1, K), dtype=torch.float32, device=x.device)
    ws = L.workspace(L.lib().sel_rvq_ema_stats_workspace(N, D, S, K), x.device)
    L.call("sel_rvq_ema_stats", L.ptr(x), N, D, L.ptr(stack), S, K, L.ptr(idx), nseg, L.ptr(stats), L.ptr(ws),
           ws.numel(), L.stream())
    return stats


@torch.no_grad()
def rvq_ema_apply(stats, layers, update=None):
    """Fold ``stats`` (nblk, S, D + 1, K) -- blocks of ``rvq_ema_stats``, summed
    left to right in block order -- into the buffers of ``layers`` (one per
    stage); ``update[s]`` (default: ``layers[s].training``) selects the stages
    written.  One block from one segment gives the bits of ``rvq_ema_update``."""
    L.need_device(stats)
    if stats.dim() != 4 or len(layers) != stats.shape[1]:
        raise L.SelError(f"rvq_ema_apply: stats {tuple(stats.shape)} is not (nblk, S, D + 1, K) for "
                         f"{len(layers)} layers")
    nblk, S, D1, K = stats.shape
    D = D1 - 1
    if not (stats.is_contiguous() and stats.dtype == torch.float32):
        raise L.SelError("rvq_ema_apply: stats must be contiguous fp32")
    update = [l.training for l in layers] if update is None else list(update)
    if len(update) != S:
        raise L.SelError("rvq_ema_apply: one update flag per layer")
    decay, eps = layers[0].decay, layers[0].eps
    tab = (_EmaStage * S)()
    for s, (l, u) in enumerate(zip(layers, update)):
        if (l.decay, l.eps) != (decay, eps):
            raise L.SelError("rvq_ema_apply: the layers' decay / eps differ")
        for b in (l.embed, l.cluster_size, l.embed_avg):
            L.need_device(b)
            if not (b.is_contiguous() and b.dtype == torch.float32):
                raise L.SelError("rvq_ema_apply: codebook buffers must be contiguous fp32")
        if (tuple(l.embed.shape) != (D, K) or tuple(l.embed_avg.shape) != (D, K)
                or tuple(l.cluster_size.shape) != (K,)):
            raise L.SelError("rvq_ema_apply: a layer's embed / embed_avg must be (D, K), its cluster_size (K)")
        tab[s] = _EmaStage(l.embed.data_ptr(), l.cluster_size.data_ptr(), l.embed_avg.data_ptr(), int(bool(u)), 0)
    L.call("sel_rvq_ema_apply", L.ptr(stats), nblk, D, S, K, ctypes.cast(tab, ctypes.c_void_p), float(decay),
           float(eps), L.stream())
