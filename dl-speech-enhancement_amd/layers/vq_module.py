"""Vector quantizer — drop-in for the reference ``layers/vq_module.py``.

VectorQuantize (:19-104) and ResidualVQ (:107-161) keep their constructor
arguments and buffers (``embed`` (dim, n_embed), ``cluster_size``,
``embed_avg``), so reference checkpoints load.  Eval-mode forward (the denoise
trainer's, trainer/denoise.py:60) runs the fused all-stage HIP kernel
(sel/vqops.py); training mode runs the same kernel for the assignment and then
the fused EMA codebook update (:74-80, csrc/vq_ema.hip) for all stages at once.

Data parallel, ``enable_ema_sync`` (switched on by ``sel.dist.sync_vq``) replaces
the fused update by its two halves (csrc/vq_ema_sync.hip): per-code statistics of
this rank's rows, gathered from all ranks in rank order, then applied -- so every
rank's codebooks follow the rows of the whole batch and stay bit-identical.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from sel.dist import gather_blocks
from sel.vqops import ResidualVQFn, rvq_ema_apply, rvq_ema_stats, rvq_ema_update


def _train_forward(flatten, stack, layers, sync=None):
    """Training-mode forward of ``layers`` on ``stack`` (their codebooks before
    the update, S, D, K): the eval-mode assignment -- every stage picks its code
    with its own pre-update codebook, so out / losses / perplexities / gradient
    are the all-stage kernel's -- then the EMA update (reference :74-80) of the
    layers in training mode, which touches only the layers' own buffers.

    ``sync`` = (process group or None, segments or None), set by
    ``enable_ema_sync``: the update in two halves.  The statistics of this
    process's rows, one block per segment, are gathered from every rank of the
    group in rank order and applied block by block, so the codebooks follow the
    global batch and are the same bits on every rank.  out / idx / losses /
    perplexities / gradient are untouched (they come from the pre-update stack);
    the perplexities stay rank-local, computed from this rank's rows."""
    aux = {}
    out, losses, ppls, idx = ResidualVQFn.apply(flatten, stack, layers[0].commitment, aux)
    update = [l.training for l in layers]
    if sync is None:
        rvq_ema_update(aux["x"], stack.detach(), idx, aux["counts"], layers, update)
    else:
        group, segments = sync
        stats = rvq_ema_stats(aux["x"], stack.detach(), idx, segments or 1)
        blocks = gather_blocks(stats, group)            # (W, nseg, S, D + 1, K), rank-major
        rvq_ema_apply(blocks.view(-1, *stats.shape[1:]), layers, update)
    for l, u in zip(layers, update):
        if u:
            l._codebook_epoch += 1
    return out, losses, ppls


class VectorQuantize(nn.Module):
    """Vector quantization w/ exponential moving averages (EMA)."""

    def __init__(self, dim, codebook_size, decay=0.8, commitment=1.0, eps=1e-5, n_embed=None):
        super().__init__()
        n_embed = codebook_size if n_embed is None else n_embed
        self.dim = dim
        self.n_embed = n_embed
        self.decay = decay
        self.eps = eps
        self.commitment = commitment
        embed = torch.randn(dim, n_embed)
        self.register_buffer("embed", embed)
        self.register_buffer("cluster_size", torch.zeros(n_embed))
        self.register_buffer("embed_avg", embed.clone())
        # bumped by every codebook write this module makes or sees (EMA update,
        # load_state_dict, .to()/.cuda()); ResidualVQ's stack cache keys on it.
        # A write that bypasses both (.data / raw device pointers) must call
        # invalidate_codebook().
        self._codebook_epoch = 0
        self._ema_sync = None  # (process group, segments) once enable_ema_sync was called

    def invalidate_codebook(self):
        self._codebook_epoch += 1

    def enable_ema_sync(self, process_group=None, segments=None):
        """Update the codebook from the rows of every rank of ``process_group``
        (None: the default group, if one is initialised) instead of this rank's
        alone; see ``ResidualVQ.enable_ema_sync``.  Opt-in; not part of the
        state_dict."""
        self._ema_sync = (process_group, segments)

    def disable_ema_sync(self):
        self._ema_sync = None

    def _apply(self, fn, *args, **kwargs):
        self._codebook_epoch += 1
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._codebook_epoch += 1
        return super()._load_from_state_dict(*args, **kwargs)

    @property
    def codebook(self):
        return self.embed.transpose(0, 1)

    def forward(self, input):
        flatten = input.reshape(-1, self.dim)
        if self.training:
            # the one-stage case of ResidualVQ's training forward; the stack is
            # a copy, because the update writes self.embed and the backward
            # reads the codebook the assignment used
            out, loss, ppl = _train_forward(flatten, self.embed.unsqueeze(0).clone(), [self], self._ema_sync)
        else:
            out, loss, ppl, _ = ResidualVQFn.apply(flatten, self.embed.unsqueeze(0), self.commitment)
        return out.view_as(input), loss[0], ppl[0]

    def forward_index(self, input):
        flatten = input.reshape(-1, self.dim)
        out, _, _, idx = ResidualVQFn.apply(flatten, self.embed.unsqueeze(0), self.commitment)
        return out.view_as(input), idx[0].view(*input.shape[:-1])


class ResidualVQ(nn.Module):
    """Residual VQ (https://arxiv.org/pdf/2107.03312.pdf algorithm 1)."""

    def __init__(self, *, num_quantizers, **kwargs):
        super().__init__()
        self.layers = nn.ModuleList([VectorQuantize(**kwargs) for _ in range(num_quantizers)])
        self._ema_sync = None

    def enable_ema_sync(self, process_group=None, segments=None):
        """Data-parallel EMA update (opt-in; ``sel.dist.sync_vq`` calls it after
        broadcasting the buffers): each training forward computes the per-code
        statistics of its own rows in ``segments or 1`` equal row segments
        (sel.vqops.rvq_ema_stats), gathers every rank's blocks in rank order
        (sel.dist.gather_blocks) and applies them left to right
        (rvq_ema_apply).  The codebooks then follow the global batch and are
        bit-identical on all ranks, for any world size and collective algorithm.
        ``segments=W`` without a process group is the simulated data-parallel
        mode: one process on the concatenated batch of W equal shards produces
        the bits that W ranks produce.  The perplexities stay rank-local.  Nothing
        is added to the state_dict."""
        self._ema_sync = (process_group, segments)

    def disable_ema_sync(self):
        self._ema_sync = None

    def _stacked(self):
        # the (S, D, K) codebook stack, rebuilt only when a codebook changed
        # (EMA update, load_state_dict, .to(): a bumped epoch, new storage or
        # a bumped version; writes through .data or raw pointers -- the replays
        # of a captured training-mode forward among them -- must call
        # VectorQuantize.invalidate_codebook())
        embeds = [l.embed for l in self.layers]
        if any(e.requires_grad for e in embeds):
            return torch.stack(embeds)
        key = tuple((l._codebook_epoch, e.data_ptr(), e._version, e.dtype, e.device)
                    for l, e in zip(self.layers, embeds))
        if getattr(self, "_stack_key", None) != key:
            self._stack_cache = torch.stack(embeds)
            self._stack_key = key
        return self._stack_cache

    def forward(self, x):
        flatten = x.reshape(-1, x.shape[-1])
        if any(l.training for l in self.layers):
            # every step writes the codebooks, so the stack is rebuilt here
            # rather than cached: inside a graph capture the restack is then part
            # of the graph and a replay reads the codebooks the last replay wrote
            out, losses, ppls = _train_forward(flatten, torch.stack([l.embed for l in self.layers]), self.layers,
                                               self._ema_sync)
        else:
            out, losses, ppls, _ = ResidualVQFn.apply(flatten, self._stacked(), self.layers[0].commitment)
        return out.view(x.shape), losses, ppls

    def forward_index(self, x, flatten_idx=False):
        flatten = x.reshape(-1, x.shape[-1])
        out, _, _, idx = ResidualVQFn.apply(flatten, self._stacked(), self.layers[0].commitment)
        idx = idx.view(len(self.layers), *x.shape[:-1])
        if flatten_idx:
            idx = idx + (self.codebook_size * torch.arange(len(self.layers), device=idx.device)).view(
                -1, *([1] * (idx.dim() - 1)))
        return out.view(x.shape), idx.squeeze(1)

    def initial(self):
        self.codebook = torch.stack([l.codebook for l in self.layers])
        self.codebook_size = self.codebook.size(1)
        self.codebook = self.codebook.reshape(-1, self.codebook.size(-1))

    def lookup(self, indices):
        return torch.sum(F.embedding(indices, self.codebook), dim=0, keepdim=True)
