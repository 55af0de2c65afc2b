"""Signed-distance fields of a triangle mesh (sdf/ and main_sdf.py of the reference): network, device dataset, trainer."""
from .network import SDFNetwork  # noqa: F401
