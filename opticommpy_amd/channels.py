"""The channel models under the reference's module name (optic/models/channels.py): ``awgn`` (opticommpy_amd.imddtx) and the
fiber channels (opticommpy_amd.models)."""
from .imddtx import awgn  # noqa: F401
from .models import convergenceCondition, linearFiberChannel, manakovSSF, nlinPhaseRot, ssfm  # noqa: F401
