"""Neighbour sampling on the device (``python/dgl/sampling/neighbor.py``)."""
from .neighbor import sample_neighbors  # noqa: F401

__all__ = ["sample_neighbors"]
