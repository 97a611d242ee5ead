"""Sampling on the device (``python/dgl/sampling/``): neighbour sampling, random walks and
the PinSAGE samplers."""
from .neighbor import sample_neighbors, select_topk  # noqa: F401
from .randomwalks import random_walk, pack_traces  # noqa: F401
from .pinsage import RandomWalkNeighborSampler, PinSAGESampler  # noqa: F401

__all__ = ["sample_neighbors", "select_topk", "random_walk", "pack_traces", "RandomWalkNeighborSampler",
           "PinSAGESampler"]
