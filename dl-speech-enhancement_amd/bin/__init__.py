"""Entry-point helpers mirroring the reference's bin/ (stream.py: the codec endpoints)."""
