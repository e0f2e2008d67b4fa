"""User-facing helpers mirroring the reference's utils/ (audiodec.py: the codec facade)."""
