"""Evaluation of a reconstructed mesh on the device (reference: code/evaluation)."""
from .chamfer import mesh_chamfer  # noqa: F401
