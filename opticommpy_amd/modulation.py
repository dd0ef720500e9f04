"""Modulation and detection under the reference's module name (optic/comm/modulation.py), gathered from the modules that
implement them."""
from .fec import modulateGray  # noqa: F401
from .metrics import demodulateGray  # noqa: F401
from .seqdet import detector, mlse  # noqa: F401
from .wdm_tx import grayMapping  # noqa: F401

__all__ = ["grayMapping", "modulateGray", "demodulateGray", "detector", "mlse"]
