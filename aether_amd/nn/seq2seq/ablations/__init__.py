"""Ablations of the seq2seq Aether (the reference's nn/seq2seq/ablations)."""
from .aether_charges import AetherCharges  # noqa: F401
