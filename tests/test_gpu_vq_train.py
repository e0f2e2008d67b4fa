"""Training-mode residual VQ (layers/vq_module.py on csrc/vq_ema.hip) and the
stage-1 trainer (trainer/autoencoder.py) on the GPU, against the reference's own
runs recorded on the CPU (tests/golden/make_goldens_autoencoder_train.py).

Bounds.  Buffers (cluster_size, embed_avg, embed): max(1e-6, 3 x e32.<name>)
norm-wise, e32 being the fixture's own fp32-versus-fp64 difference for that
tensor (DESIGN section 10's bound form).  out 1e-6, losses 1e-5, perplexities
1e-6: the existing VQ tests' tolerances.  ``embed`` after a step is not in the
fixture (the size limit): it is evaluated here in fp64 from the fixture's
cluster_size and embed_avg by the reference's expression (:78-79), which the
fixture script checked to reproduce the reference's fp64 embed to 5e-7.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

CASES = ["c0", "c1", "c2", "c3"]
BUFS = ("cluster_size", "embed_avg", "embed")


def rel(a, b):
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).double()
            for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _fixtures():
    g = dict(golden("vq_train"))
    g.update(golden("vq_train_c0"))
    return g


def _case(name):
    return {k[len(name) + 1:]: v for k, v in _fixtures().items() if k.startswith(name + ".")}


def _module(c, dev):
    from layers.vq_module import ResidualVQ
    N, D, K, S, steps = (int(v) for v in c["cfg"])
    M = ResidualVQ(num_quantizers=S, dim=D, codebook_size=K)
    with torch.no_grad():
        for i, l in enumerate(M.layers):
            assert (l.decay, l.eps, l.commitment) == (float(c["decay"]), float(c["eps"]), float(c["commitment"]))
            e = torch.from_numpy(c[f"init.embed.{i}"].astype(np.float32))
            l.embed.copy_(e)
            l.embed_avg.copy_(e)
            l.cluster_size.zero_()
    return M.to(dev).train()


def _x(c, t, dev):
    return torch.from_numpy(c[f"x.{t}"].astype(np.float32)).to(dev)


def _state(M):
    return [{b: getattr(l, b).detach().clone() for b in BUFS} for l in M.layers]


def _embed64(cluster_size, embed_avg, eps):
    """vq_module.py:78-79 in fp64"""
    n = cluster_size.sum()
    cs = (cluster_size + eps) / (n + cluster_size.numel() * eps) * n
    return embed_avg / cs.unsqueeze(0)


def ema64(x, state, idx, decay, eps, update=None):
    """The EMA update (vq_module.py:74-80) restated in fp64 on the CPU: one
    training step of every layer from ``state`` (list of {buffer: fp64 tensor})
    with the GIVEN indices (S, N); returns the new state."""
    r = x.double().cpu()
    new = []
    for s, st in enumerate(state):
        K = st["cluster_size"].numel()
        ind = idx[s].cpu().long()
        if update is None or update[s]:
            counts = torch.bincount(ind, minlength=K).double()
            csz = st["cluster_size"] * decay + counts * (1 - decay)
            esum = torch.zeros_like(st["embed_avg"]).index_add_(1, ind, r.t())
            eavg = st["embed_avg"] * decay + esum * (1 - decay)
            new.append({"cluster_size": csz, "embed_avg": eavg, "embed": _embed64(csz, eavg, eps)})
        else:
            new.append(dict(st))
        q = st["embed"].t()[ind]                 # the pre-update codebook picks the code
        r = r - (r + (q - r))
    return new


@functools.lru_cache(maxsize=None)
def _run(name):
    """One training-mode run of the case on the GPU, shared by the tests: per
    step the indices (forward_index on the pre-update codebooks), the outputs
    and the buffers after the step, all on the CPU."""
    dev = torch.device("cuda:0")
    c = _case(name)
    N, D, K, S, steps = (int(v) for v in c["cfg"])
    M = _module(c, dev)
    rec = []
    for t in range(steps):
        x = _x(c, t, dev)
        with torch.no_grad():
            _, idx = M.forward_index(x)
            out, losses, ppls = M(x)
        rec.append(dict(idx=idx.reshape(S, N).cpu(), out=out.cpu(), losses=losses.cpu(), ppls=ppls.cpu(),
                        state=[{b: v.cpu() for b, v in st.items()} for st in _state(M)]))
    return rec


def _bound(c, b, t, i):
    return max(1e-6, 3.0 * float(c[f"e32.{b}.{t}.{i}"]))


@pytest.mark.parametrize("name", CASES)
def test_ema_update_matches_fp64_restatement_on_own_indices(gpu, name):
    """(a) the contract: every step's buffers against the fp64 EMA chained from
    the initial state with the GPU's own indices."""
    c = _case(name)
    N, D, K, S, steps = (int(v) for v in c["cfg"])
    e0 = [torch.from_numpy(c[f"init.embed.{i}"].astype(np.float64)) for i in range(S)]
    state = [{"cluster_size": torch.zeros(K, dtype=torch.float64), "embed_avg": e.clone(), "embed": e.clone()}
             for e in e0]
    for t, r in enumerate(_run(name)):
        assert int(r["idx"].min()) >= 0 and int(r["idx"].max()) < K
        state = ema64(_x(c, t, "cpu"), state, r["idx"], float(c["decay"]), float(c["eps"]))
        for i in range(S):
            for b in BUFS:
                e = rel(r["state"][i][b], state[i][b])
                print(f"{name} step {t} layer {i} {b}: {e:.2e} (bound {_bound(c, b, t, i):.1e})")
                assert e <= _bound(c, b, t, i), (name, t, i, b, e)


@pytest.mark.parametrize("name", CASES)
def test_training_forward_matches_reference_fixture(gpu, name):
    """(b) the reference's own training-mode run: identical indices (the
    fixture's margins exceed the tie bound), outputs and buffers per step."""
    c = _case(name)
    N, D, K, S, steps = (int(v) for v in c["cfg"])
    for t, r in enumerate(_run(name)):
        assert torch.equal(r["idx"], torch.from_numpy(c[f"idx.{t}"].astype(np.int64))), (name, t)
        for key, tol in (("out", 1e-6), ("losses", 1e-5), ("ppls", 1e-6)):
            e = rel(r[key], c[f"{key}.{t}"])
            print(f"{name} step {t} {key}: {e:.2e}")
            assert e <= tol, (name, t, key, e)
        for i in range(S):
            csz = torch.from_numpy(c[f"cluster_size.{t}.{i}"]).double()
            eavg = torch.from_numpy(c[f"embed_avg.{t}.{i}"]).double()
            want = {"cluster_size": csz, "embed_avg": eavg, "embed": _embed64(csz, eavg, float(c["eps"]))}
            for b in BUFS:
                e = rel(r["state"][i][b], want[b])
                print(f"{name} step {t} layer {i} {b}: {e:.2e} (bound {_bound(c, b, t, i):.1e})")
                assert e <= _bound(c, b, t, i), (name, t, i, b, e)


def _equal_states(a, b):
    return all(torch.equal(sa[k].cpu(), sb[k].cpu()) for sa, sb in zip(a, b) for k in BUFS)


def test_update_is_deterministic_and_capturable(gpu):
    """(c) two fresh modules give the same bits after 3 steps; a captured
    training-mode forward replays to the bits of eager steps from the same state
    (out and every buffer), which also needs the restack of the updated
    codebooks to be part of the graph."""
    c = _case("c0")
    first = _run("c0")
    M = _module(c, gpu)
    with torch.no_grad():
        for t in range(3):
            M(_x(c, t, gpu))
    assert _equal_states(_state(M), first[-1]["state"])

    xs = _x(c, 0, gpu)
    A = _module(c, gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            A(xs)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    B = copy.deepcopy(A)                      # the state the capture starts from
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out_s, losses_s, ppls_s = A(xs)
    assert _equal_states(_state(A), _state(B))   # capturing ran nothing
    for step in range(2):
        graph.replay()
        with torch.no_grad():
            out_e, losses_e, ppls_e = B(xs)
        torch.cuda.synchronize(gpu)
        assert torch.equal(out_s, out_e) and torch.equal(losses_s, losses_e) and torch.equal(ppls_s, ppls_e), step
        assert _equal_states(_state(A), _state(B)), step
    assert not _equal_states(_state(A), first[0]["state"])


def test_mixed_mode_leaves_eval_layers_untouched(gpu):
    """(d) S = 3 with layer 1 in eval mode: its buffers keep their bits, layers
    0 and 2 update as in the all-training run (same bits; and within the bound
    of the fp64 restatement), and the outputs are the all-training run's."""
    c = _case("c0")
    N, D, K, S, steps = (int(v) for v in c["cfg"])
    ref = _run("c0")[0]
    M = _module(c, gpu)
    M.layers[1].eval()
    before = _state(M)
    epoch = [l._codebook_epoch for l in M.layers]
    with torch.no_grad():
        out, losses, ppls = M(_x(c, 0, gpu))
    after = _state(M)
    for b in BUFS:
        assert torch.equal(after[1][b], before[1][b]), b
        for i in (0, 2):
            assert torch.equal(after[i][b].cpu(), ref["state"][i][b]), (i, b)
    assert [l._codebook_epoch - e for l, e in zip(M.layers, epoch)] == [1, 0, 1]
    assert torch.equal(out.cpu(), ref["out"]) and torch.equal(losses.cpu(), ref["losses"])
    assert torch.equal(ppls.cpu(), ref["ppls"])
    want = ema64(_x(c, 0, "cpu"), [{b: v.double().cpu() for b, v in st.items()} for st in before], ref["idx"],
                 float(c["decay"]), float(c["eps"]), update=[True, False, True])
    for i in range(S):
        for b in BUFS:
            assert rel(after[i][b], want[i][b]) <= _bound(c, b, 0, i), (i, b)


def test_gradient_uses_the_pre_update_codebook(gpu):
    """(e) backward after the training forward (the codebooks have moved by
    then) gives the eval-mode gradient of a copy taken before the update."""
    c = _case("c0")
    M = _module(c, gpu)
    with torch.no_grad():
        M(_x(c, 0, gpu))                      # non-trivial cluster sizes
    E = copy.deepcopy(M).eval()
    for weigh_out in (1.0, 0.0):              # the issue's loss; and the commitment term alone
        grads = []
        for mod in (M, E):
            x = _x(c, 1, gpu).requires_grad_(True)
            e0 = mod.layers[0].embed.clone()
            out, losses, _ = mod(x)
            assert mod is E or not torch.equal(mod.layers[0].embed, e0)   # the training forward moved it
            (weigh_out * out.sum() + losses.sum()).backward()
            grads.append(x.grad)
        e = rel(grads[0], grads[1])
        print(f"training-mode gradient vs eval-mode (out weight {weigh_out}): {e:.2e}")
        assert e <= 1e-6, (weigh_out, e)
        M = copy.deepcopy(E).train()          # the same starting state for the second loss


# the three-step parameter delta against the fixture (see the test's docstring)
MEASURED_FLIPS = 0.0        # MI355X: 0 of 160,108 entries off by more than 0.5 lr
MEASURED_DELTA = 1.59e-5    # MI355X, norm-wise (the reference's own fp32 run against fp64: 1.5e-5)
FLIPS_CAP = 0.0             # 2 x 0
DELTA_CAP = 4e-5            # 2 x 1.59e-5 = 3.18e-5 -> 4e-5 (one digit, rounded up)
assert FLIPS_CAP <= 0.02 and DELTA_CAP <= 0.10   # never looser than the vocoder trainer test's caps


def test_autoencoder_trainer_steps_match_reference_golden(gpu):
    """(f) trainer/autoencoder.Trainer._train_step against the reference CLASS
    ITSELF (tests/golden/autoencoder_trainer_step.npz): reduced PQC generator,
    reduced MSD + MPD discriminator (regenerated by seed 93, checksummed), 48
    kHz mel loss, lambda 1 / 45 / 1 / 2, Adam 1e-4 / 2e-4 (0.5, 0.9) -- fused
    here -- three steps from steps = 0 with start_steps {generator 0,
    discriminator 2}, paradigm 'efficient'.  Steps 0 and 1 train the whole codec
    and update the codebooks; step 2 freezes the encoder side, puts the
    codebooks into eval mode and adds the adversarial half and the
    discriminator update.  Logged keys equal; values 1e-5 (step 0) / 1e-4
    (later); gradient norms after step 0 1e-4; quantizer buffers after steps 0
    and 1 max(1e-6, 3 x e32), bit-unchanged by step 2; encoder / projector
    parameters frozen and bit-unchanged by step 2, with no gradient.  The
    three-step parameter delta: entries off by more than 0.5 lr and the
    norm-wise difference, capped at twice the measured MI355X figures rounded
    up to one digit and never above the vocoder test's 2 % / 0.10.  Measured:
    0 of 160,108 entries and 1.59e-5 norm-wise, so the caps are 0 entries and
    4e-5 (the reference's own fp32 run against fp64: 0 entries and 1.5e-5)."""
    from losses import (DiscriminatorAdversarialLoss, FeatureMatchLoss, GeneratorAdversarialLoss,
                        MultiMelSpectrogramLoss)
    from models.autoencoder.AudioDec import Generator
    from models.vocoder.HiFiGAN import Discriminator
    from sel.convops import precision
    from trainer.autoencoder import Trainer
    from golden.make_goldens import D_PARAMS
    g = golden("autoencoder_trainer_step")
    g3 = golden("autoencoder_trainer_step_sd3")
    gp = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
    torch.manual_seed(93)
    D = Discriminator(**D_PARAMS)
    chk = sum(float(p.double().abs().sum()) for p in D.parameters())
    assert abs(chk - float(g["chk.discriminator"])) <= 1e-9 * float(g["chk.discriminator"])
    G = Generator(**gp)
    sd0 = {k[3:]: torch.from_numpy(v.astype(np.float32) if v.dtype == np.float16 else v)
           for k, v in g.items() if k.startswith("sd.")}
    G.load_state_dict(sd0, strict=True)
    D, G = D.to(gpu), G.to(gpu).train()
    lr = 1e-4
    crit = {"mel": MultiMelSpectrogramLoss(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048],
                                           window="hann_window", num_mels=80, fmin=0, fmax=24000,
                                           log_base=None).to(gpu),
            "gen_adv": GeneratorAdversarialLoss(average_by_discriminators=False),
            "dis_adv": DiscriminatorAdversarialLoss(average_by_discriminators=False),
            "feat_match": FeatureMatchLoss(average_by_discriminators=False, average_by_layers=False,
                                           include_final_outputs=False)}
    cfg = {"outdir": None, "train_max_steps": 10, "use_mel_loss": True, "use_stft_loss": False,
           "use_shape_loss": False, "lambda_vq_loss": 1.0, "lambda_mel_loss": 45.0, "lambda_adv": 1.0,
           "lambda_feat_match": 2.0, "use_feat_match_loss": True, "generator_grad_norm": -1,
           "discriminator_grad_norm": -1, "paradigm": "efficient",
           "start_steps": {"generator": 0, "discriminator": 2}}
    og = torch.optim.Adam(G.parameters(), lr=lr, betas=(0.5, 0.9), weight_decay=0.0, fused=True)
    od = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=0.0, fused=True)
    sg = torch.optim.lr_scheduler.MultiStepLR(og, milestones=[200000], gamma=0.5)
    sdd = torch.optim.lr_scheduler.MultiStepLR(od, milestones=[200000], gamma=0.5)
    tr = Trainer(steps=0, epochs=0, data_loader={}, model={"generator": G, "discriminator": D}, criterion=crit,
                 optimizer={"generator": og, "discriminator": od},
                 scheduler={"generator": sg, "discriminator": sdd}, config=cfg, device=gpu)
    x = torch.from_numpy(g["x"])
    book = G.quantizer.codebook
    frozen = {k: p for part in ("encoder", "projector", "quantizer")
              for k, p in getattr(G, part).named_parameters(prefix=part)}
    assert frozen and len(frozen) < len(list(G.parameters()))
    with precision(torch.float32):
        for s in range(3):
            if s == 2:
                held = {k: p.detach().clone() for k, p in frozen.items()}
                bufs1 = _state(book)
                assert all(p.requires_grad for p in frozen.values()) and book.training
            tr._train_step(x)
            tol = 1e-5 if s == 0 else 1e-4
            rec = {k: float(v) for k, v in tr.total_train_loss.items()}
            ref = {k[len(f"rec.{s}."):]: float(v) for k, v in g.items() if k.startswith(f"rec.{s}.")}
            assert set(rec) == set(ref), set(rec) ^ set(ref)
            for k, v in ref.items():
                print(f"step {s} {k}: {rec[k]:.8g} (reference {v:.8g})")
            for k, v in ref.items():
                assert abs(rec[k] - v) <= tol * abs(v) + 1e-7, (s, k, rec[k], v)
            tr.total_train_loss.clear()
            if s == 0:
                for k, p in G.named_parameters():
                    want = float(g["gnorm." + k])
                    assert abs(float(p.grad.double().norm()) - want) <= 1e-4 * want, (k, float(p.grad.norm()), want)
            if s < 2:
                for i, l in enumerate(book.layers):
                    for b in BUFS:
                        e = rel(getattr(l, b), g[f"buf.{s}.{i}.{b}"])
                        bound = max(1e-6, 3.0 * float(g[f"e32.buf.{s}.{i}.{b}"]))
                        print(f"step {s} codebook {i} {b}: {e:.2e} (bound {bound:.1e})")
                        assert e <= bound, (s, i, b, e)
    # step 2: the encoder side is frozen and the codebooks are in eval mode
    assert tr.fix_encoder and tr.discriminator_train and not book.training
    assert _equal_states(_state(book), bufs1)
    for k, p in frozen.items():
        assert not p.requires_grad and p.grad is None and torch.equal(p.detach(), held[k]), k
    flips, tot, num, den = 0, 0, 0.0, 0.0
    for k, p in G.named_parameters():
        refd = torch.from_numpy(g3["sd3." + k]).double() - sd0[k].double()
        d = p.detach().double().cpu() - sd0[k].double()
        flips += ((d - refd).abs() > 0.5 * lr).sum().item()
        tot += d.numel()
        num += ((d - refd) ** 2).sum().item()
        den += (refd ** 2).sum().item()
    print(f"three-step delta: {flips} of {tot} entries off by > 0.5 lr ({flips / tot:.2e}), "
          f"norm-wise {(num / den) ** 0.5:.2e}")
    assert flips <= FLIPS_CAP * tot, (flips, tot)
    assert (num / den) ** 0.5 <= DELTA_CAP, (num / den) ** 0.5
