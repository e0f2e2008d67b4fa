"""Autoencoder trainer — drop-in for trainer/autoencoder.py (Trainer :19-166): the
first training stage of AudioDec, which produces the checkpoint the denoise and
vocoder stages start from.

Until ``start_steps.discriminator`` the whole codec (encoder -> projector ->
residual VQ -> decoder) trains on the metric loss plus the commitment loss, and
the quantizer's codebooks follow by their EMA update (layers/vq_module.py, one
fused call per forward).  From that step on the discriminator trains and the
generator adds the adversarial and feature-matching losses; under the
``'efficient'`` paradigm (the default) the encoder, projector and quantizer are
frozen at that point and the codebooks are kept in eval mode, so only the
decoder goes on learning.  The discriminator step recomputes the prediction
under no_grad from the updated generator (:117-126).

Under a process group (torch.distributed.run, the models wrapped by
sel.dist.wrap_ddp) the codebooks are buffers that gradient averaging does not
reach: the constructor calls sel.dist.sync_vq, which broadcasts them from rank 0
and makes every EMA update use the statistics of all ranks' rows, so the
replicas stay bit-identical and the checkpoint holds the global batch's codebook.
"""
import logging

import torch

from sel import dist as seldist
from trainer.trainerGAN import TrainerVQGAN


class Trainer(TrainerVQGAN):
    def __init__(self, steps, epochs, data_loader, model, criterion, optimizer, scheduler, config,
                 device=torch.device("cpu")):
        super().__init__(steps=steps, epochs=epochs, data_loader=data_loader, model=model, criterion=criterion,
                         optimizer=optimizer, scheduler=scheduler, config=config, device=device)
        self.fix_encoder = False
        self.paradigm = config.get("paradigm", "efficient")
        start = config.get("start_steps", {})
        self.generator_start = start.get("generator", 0)
        self.discriminator_start = start.get("discriminator", 200000)
        if seldist.is_dist():  # (sync_vq does nothing with one rank)
            seldist.sync_vq(self._gen())

    def _gen(self):
        """The generator's own module (a data-parallel wrapper keeps it as .module)."""
        gen = self.model["generator"]
        return getattr(gen, "module", gen)

    def _freeze_encoder_side(self):
        gen = self._gen()
        for part in (gen.encoder, gen.projector, gen.quantizer):
            for p in part.parameters():
                p.requires_grad = False
        self.fix_encoder = True
        logging.info("Encoder, projector, quantizer, and codebook are fixed")

    def _train_step(self, batch):
        mode = "train"
        x = batch.to(self.device)
        gen = self.model["generator"]

        self.generator_train = self.steps >= self.generator_start
        self.discriminator_train = self.steps >= self.discriminator_start
        if self.discriminator_train and not self.fix_encoder and self.paradigm == "efficient":
            self._freeze_encoder_side()
        if self.fix_encoder:
            self._gen().quantizer.codebook.eval()  # no EMA update once the encoder side is fixed

        # generator: commitment + metric (+ adversarial + feature matching)
        if self.generator_train:
            y_, _, _, vqloss, perplexity = gen(x)
            self._perplexity(perplexity, mode=mode)
            gen_loss = self._vq_loss(vqloss, mode=mode)
            gen_loss = gen_loss + self._metric_loss(y_, x, mode=mode)
            if self.discriminator_train:
                p_ = self.model["discriminator"](y_)
                if self.config["use_feat_match_loss"]:
                    with torch.no_grad():
                        p = self.model["discriminator"](x)
                else:
                    p = None
                gen_loss = gen_loss + self._adv_loss(p_, p, mode=mode)
            self._record_loss("generator_loss", gen_loss, mode=mode)
            self._update_generator(gen_loss)

        # discriminator, on a prediction recomputed from the updated generator
        if self.discriminator_train:
            with torch.no_grad():
                y_ = gen(x)[0]
            p = self.model["discriminator"](x)
            p_ = self.model["discriminator"](y_.detach())
            self._update_discriminator(self._dis_loss(p_, p, mode=mode))

        self.steps += 1
        self.tqdm.update(1)
        self._check_train_finish()

    @torch.no_grad()
    def _eval_step(self, batch):
        mode = "eval"
        x = batch.to(self.device)
        y_, _, _, vqloss, perplexity = self.model["generator"](x)
        self._perplexity(perplexity, mode=mode)
        gen_loss = self._vq_loss(vqloss, mode=mode)
        gen_loss = gen_loss + self._metric_loss(y_, x, mode=mode)
        if self.discriminator_train:
            p_ = self.model["discriminator"](y_)
            p = self.model["discriminator"](x)
            gen_loss = gen_loss + self._adv_loss(p_, p, mode=mode)
            self._dis_loss(p_, p, mode=mode)
        self._record_loss("generator_loss", gen_loss, mode=mode)
        self._eval_measures(y_, x)
