"""The sequence sources under the reference's module name (optic/comm/sources.py): host numpy, bit for bit the reference's."""
from .imddtx import bitSource, prbsGenerator, symbolSource  # noqa: F401
