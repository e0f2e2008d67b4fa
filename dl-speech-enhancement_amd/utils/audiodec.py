"""AudioDec codec facade -- drop-in for the reference's utils/audiodec.py
(AudioDec :18-57, assign_model :106-164): same names, arguments and checkpoint
layout (``torch.load(path)['model']['generator']``, ``config.yml`` beside it).

Decoder types ``symAudioDec*`` are this project's AudioDec ``StreamGenerator``;
``HiFiGAN`` / ``UnivNet`` are ``models.vocoder.HiFiGAN.StreamGenerator`` on its
own inference path.  One addition: ``open_session`` returns the transmitter's
``sel.streaming.StreamSession`` and the receiver's session (a ``StreamSession``,
or a ``VocoderSession`` for a vocoder decoder) after the reference's warm-up,
and ``open_pool`` the same pair as stream pools for independent streams.
``AudioDecStreamer`` (the sound-device loop) is not provided.
"""
import os

import torch

from bin.stream import AudioCodec
from models.autoencoder.AudioDec import StreamGenerator as generator_audiodec
from models.vocoder.HiFiGAN import StreamGenerator as generator_hifigan

_AUTOENCODERS = ("symAudioDec", "symAudioDecUniv")
_VOCODERS = ("HiFiGAN", "UnivNet")


def _load_generator(cls, config, checkpoint):
    model = cls(**config["generator_params"])
    model.load_state_dict(torch.load(checkpoint, map_location="cpu")["model"]["generator"])
    return model


class AudioDec(AudioCodec):
    def __init__(self, tx_device="cpu", rx_device="cpu", receptive_length=8192):
        # (the symAD_vctk_48000_hop300 encoder's receptive field is 7209 samples)
        super().__init__(tx_device=tx_device, rx_device=rx_device, receptive_length=receptive_length)

    def _load_encoder(self, checkpoint):
        config = self._load_config(checkpoint)
        if config["model_type"] not in _AUTOENCODERS:
            raise NotImplementedError(f"Encoder type {config['model_type']} is not supported!")
        return _load_generator(generator_audiodec, config, checkpoint)

    def _load_decoder(self, checkpoint):
        config = self._load_config(checkpoint)
        if config["model_type"] in _AUTOENCODERS:
            return _load_generator(generator_audiodec, config, checkpoint)
        if config["model_type"] in _VOCODERS:
            return _load_generator(generator_hifigan, config, checkpoint)
        raise NotImplementedError(f"Decoder {config['model_type']} is not supported!")

    def open_session(self, batch=1, chunk=300, graph=True, codes=False, wire=False, datagrams=False):
        """(tx, rx) streaming sessions, warmed up as load_transmitter / load_receiver
        left the models: ``tx.encode -> tx.quantize`` on the transmitter,
        ``rx.lookup -> rx.decode`` on the receiver.  The receiver's session runs
        the lookup on rx_encoder's codebook and the decode on the decoder: a
        ``StreamSession`` for an AudioDec generator, a ``VocoderSession`` of
        ``chunk / hop`` frames per hop for the HiFi-GAN vocoder decoder (hop =
        the product of its upsample scales).  ``codes=True`` also calls
        ``enable_codes()`` on both (after the warm-up state is loaded and the
        receiver knows rx_encoder): ``tx.transmit`` / ``rx.receive`` then run the
        quantizer and the lookup inside the hop.  ``wire=True`` (with ``codes``)
        makes that ``enable_codes(wire=True)``: ``tx.transmit_packets`` returns and
        ``rx.receive_packets`` takes the bytes of the wire format (sel/wire.py).
        ``datagrams=True`` (with ``codes``) adds ``enable_codes(datagrams=True)``:
        ``tx.transmit_datagrams(x, stages)`` / ``rx.receive_datagrams(p, lost)``,
        datagrams with a header, a stage budget per stream and loss concealment."""
        from sel.streaming import StreamSession, VocoderSession
        if self.tx_encoder is None or self.rx_encoder is None or self.decoder is None:
            raise RuntimeError("open_session: call load_transmitter and load_receiver first")
        tx = StreamSession(self.tx_encoder, batch, chunk, graph)
        tx.load_state()
        if isinstance(self.decoder, generator_audiodec):
            rx = StreamSession(self.decoder, batch, chunk, graph)
        else:
            hop = 1
            for up in self.decoder.upsamples:
                hop *= up.stride
            if chunk % hop:
                raise ValueError(f"open_session: chunk ({chunk}) is not a multiple of the vocoder's hop ({hop})")
            rx = VocoderSession(self.decoder, batch, chunk // hop, graph)
        rx.load_state()
        rx.lookup_generator = self.rx_encoder
        if codes:
            tx.enable_codes(wire=wire, datagrams=datagrams)
            rx.enable_codes(wire=wire, datagrams=datagrams)
        return tx, rx

    def open_pool(self, capacity, chunk=300, graph=True, codes=False, wire=False, datagrams=False):
        """(tx_pool, rx_pool) for `capacity` independent streams, mirroring
        open_session: a ``StreamPool`` on the transmitter, a ``StreamPool`` or a
        ``VocoderPool`` (``chunk / hop`` frames per hop) on the receiver, both
        with the models' warmed-up pad_buffers as the template every newly
        opened stream starts from.  ``codes=True``, ``wire=True`` and
        ``datagrams=True`` as in ``open_session``."""
        from sel.streaming import StreamPool, VocoderPool
        if self.tx_encoder is None or self.rx_encoder is None or self.decoder is None:
            raise RuntimeError("open_pool: call load_transmitter and load_receiver first")
        tx = StreamPool(self.tx_encoder, capacity, chunk, graph)
        tx.load_state()
        if isinstance(self.decoder, generator_audiodec):
            rx = StreamPool(self.decoder, capacity, chunk, graph)
        else:
            hop = 1
            for up in self.decoder.upsamples:
                hop *= up.stride
            if chunk % hop:
                raise ValueError(f"open_pool: chunk ({chunk}) is not a multiple of the vocoder's hop ({hop})")
            rx = VocoderPool(self.decoder, capacity, chunk // hop, graph)
        rx.load_state()
        rx.lookup_generator = self.rx_encoder
        if codes:
            tx.enable_codes(wire=wire, datagrams=datagrams)
            rx.enable_codes(wire=wire, datagrams=datagrams)
        return tx, rx


def assign_model(model):
    """(sample_rate, encoder_checkpoint, decoder_checkpoint) of a released model name."""
    ae, voc, dn = "autoencoder", "vocoder", "denoise"
    table = {
        # name: (sample rate, (tx stage, tx experiment, tx steps), (rx stage, rx experiment, rx steps))
        "libritts_v1": (24000, (ae, "symAD_libritts_24000_hop300", 500000),
                        (voc, "AudioDec_v1_symAD_libritts_24000_hop300_clean", 500000)),
        "libritts_sym": (24000, (ae, "symAD_libritts_24000_hop300", 500000),
                         (ae, "symAD_libritts_24000_hop300", 1000000)),
        "vctk_v1": (48000, (ae, "symAD_vctk_48000_hop300", 200000),
                    (voc, "AudioDec_v1_symAD_vctk_48000_hop300_clean", 500000)),
        "vctk_sym": (48000, (ae, "symAD_vctk_48000_hop300", 200000), (ae, "symAD_vctk_48000_hop300", 700000)),
        "vctk_v0": (48000, (ae, "symAD_vctk_48000_hop300", 200000),
                    (voc, "AudioDec_v0_symAD_vctk_48000_hop300_clean", 500000)),
        "vctk_v2": (48000, (ae, "symAD_vctk_48000_hop300", 200000),
                    (voc, "AudioDec_v2_symAD_vctk_48000_hop300_clean", 500000)),
        "vctk_denoise": (48000, (dn, "symAD_vctk_48000_hop300", 200000),
                         (voc, "AudioDec_v1_symAD_vctk_48000_hop300_clean", 500000)),
        "vctk_univ": (48000, (ae, "symADuniv_vctk_48000_hop300", 500000),
                      (voc, "AudioDec_v3_symADuniv_vctk_48000_hop300_clean", 500000)),
        "vctk_univ_sym": (48000, (ae, "symADuniv_vctk_48000_hop300", 500000),
                          (ae, "symADuniv_vctk_48000_hop300", 1000000)),
    }
    if model not in table:
        raise NotImplementedError(f"Model {model} is not supported!")
    rate, tx, rx = table[model]
    path = lambda e: os.path.join("exp", e[0], e[1], f"checkpoint-{e[2]}steps.pkl")  # noqa: E731
    return rate, path(tx), path(rx)
