"""Vocoder trainer — drop-in for trainer/vocoder.py (Trainer :19-146): the second
training stage of AudioDec.  A frozen analyzer (encoder -> projector ->
quantizer, eval mode) feeds the HiFi-GAN generator, which is trained with the
metric loss plus the adversarial and feature-matching losses of the MSD + MPD
discriminator; the discriminator step recomputes the prediction under no_grad
(:96-103).  ``generator_train_start_steps`` / ``discriminator_train_start_steps``
gate the two halves (:65, :79, :95).

The generator's training path is opt-in (models/vocoder/HiFiGAN.py
``enable_training``): the trainer switches it on."""
import logging

import torch

from trainer.trainerGAN import TrainerGAN


class Trainer(TrainerGAN):
    def __init__(self, steps, epochs, data_loader, model, criterion, optimizer, scheduler, config,
                 device=torch.device("cpu")):
        super().__init__(steps=steps, epochs=epochs, data_loader=data_loader, model=model, criterion=criterion,
                         optimizer=optimizer, scheduler=scheduler, config=config, device=device)
        self.fix_analyzer = False
        self.generator_start = config.get("generator_train_start_steps", 0)
        self.discriminator_start = config.get("discriminator_train_start_steps", 0)
        gen = self.model["generator"]
        gen = getattr(gen, "module", gen)  # DDP-wrapped
        if hasattr(gen, "enable_training"):
            gen.enable_training()

    def _predict(self, x):
        """analyzer (frozen) -> generator"""
        an = self.model["analyzer"]
        zq, _, _ = an.quantizer(an.projector(an.encoder(x)))
        return self.model["generator"](zq)

    def _train_step(self, batch):
        mode = "train"
        x = batch.to(self.device)

        if not self.fix_analyzer:
            for p in self.model["analyzer"].parameters():
                p.requires_grad = False
            self.fix_analyzer = True
            logging.info("Analyzer is fixed!")
        self.model["analyzer"].eval()

        # generator: metric + adversarial + feature matching
        if self.steps > self.generator_start:
            y_ = self._predict(x)
            gen_loss = self._metric_loss(y_, x, mode=mode)
            if self.steps > self.discriminator_start:
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
        if self.steps > self.discriminator_start:
            with torch.no_grad():
                y_ = self._predict(x)
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
        y_ = self._predict(x)
        gen_loss = self._metric_loss(y_, x, mode=mode)
        if self.steps > self.discriminator_start:
            p_ = self.model["discriminator"](y_)
            p = self.model["discriminator"](x) if self.config["use_feat_match_loss"] else None
            gen_loss = gen_loss + self._adv_loss(p_, p, mode=mode)
            self._dis_loss(p_, p, mode=mode)
        self._record_loss("generator_loss", gen_loss, mode=mode)
        self._eval_measures(y_, x)
