"""Codec endpoints -- drop-in for the model-loading half of the reference's
bin/stream.py (AudioCodec :23-77).

A transmitter holds an encoder; a receiver holds its own copy of the encoder
(for the codebook lookup) and a decoder.  Loading a model moves it to its
device, puts it in eval mode and runs the reference's warm-up: ``receptive_length``
zero samples through the encoder, the resulting codes through the decoder.

``AudioCodecStreamer`` (the sound-device loop of the reference, :80-) is not
provided: it needs a sound device and torchaudio.
"""
import abc
import os

import yaml


class AudioCodec(abc.ABC):
    def __init__(self, tx_device="cpu", rx_device="cpu", receptive_length=8192):
        self.tx_device = tx_device
        self.rx_device = rx_device
        self.receptive_length = receptive_length
        self.tx_encoder = None
        self.rx_encoder = None
        self.decoder = None

    @abc.abstractmethod
    def _load_encoder(self, checkpoint):
        """Build the encoder generator and load ``checkpoint`` into it."""

    @abc.abstractmethod
    def _load_decoder(self, checkpoint):
        """Build the decoder generator and load ``checkpoint`` into it."""

    def _load_config(self, checkpoint, config_name="config.yml"):
        """The training config saved beside the checkpoint."""
        with open(os.path.join(os.path.dirname(checkpoint), config_name)) as f:
            return yaml.load(f, Loader=yaml.Loader)

    def load_transmitter(self, encoder_checkpoint):
        assert os.path.exists(encoder_checkpoint), f"{encoder_checkpoint} does not exist!"
        self.tx_encoder = self._load_encoder(encoder_checkpoint)
        self.tx_encoder.eval().to(self.tx_device)
        self.tx_encoder.initial_encoder(self.receptive_length, self.tx_device)
        print("Load tx_encoder: %s" % (encoder_checkpoint))

    def load_receiver(self, encoder_checkpoint, decoder_checkpoint):
        assert os.path.exists(encoder_checkpoint), f"{encoder_checkpoint} does not exist!"
        self.rx_encoder = self._load_encoder(encoder_checkpoint)
        self.rx_encoder.eval().to(self.rx_device)
        zq = self.rx_encoder.initial_encoder(self.receptive_length, self.rx_device)
        print("Load rx_encoder: %s" % (encoder_checkpoint))

        assert os.path.exists(decoder_checkpoint), f"{decoder_checkpoint} does not exist!"
        self.decoder = self._load_decoder(decoder_checkpoint)
        self.decoder.eval().to(self.rx_device)
        self.decoder.initial_decoder(zq)
        print("Load decoder: %s" % (decoder_checkpoint))
