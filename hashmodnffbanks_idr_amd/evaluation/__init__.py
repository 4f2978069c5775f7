"""Evaluation of a reconstructed mesh on the device (reference: code/evaluation)."""
from .chamfer import dtu_chamfer, load_dtu_scan, mesh_chamfer  # noqa: F401
