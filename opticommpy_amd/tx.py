"""The transmitters under the reference's module name (optic/models/tx.py): ``simpleWDMTx`` (opticommpy_amd.wdm_tx) and
``pamTransmitter`` (opticommpy_amd.imddtx)."""
from .imddtx import pamTransmitter  # noqa: F401
from .wdm_tx import simpleWDMTx  # noqa: F401
