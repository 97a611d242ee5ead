"""Names shared across the package (``python/dgl/base.py``)."""
from ._ffi import DGLError  # noqa: F401

# the feature that holds the parent's node / edge ids on an induced graph
NID = "_ID"
EID = "_ID"
