"""The optical devices under the reference's module name (optic/models/devices.py): the modulators and the attenuator
(opticommpy_amd.imddtx), the receiver-side devices (opticommpy_amd.rx), the amplifier (opticommpy_amd.models), the laser
(opticommpy_amd.wdm_tx) and the converters (opticommpy_amd.clock)."""
from .clock import adc, dac  # noqa: F401
from .imddtx import iqm, mzm, pm, voa  # noqa: F401
from .models import edfa  # noqa: F401
from .rx import balancedPD, coherentReceiver, opticalHybrid2x4, pbs, pdmCoherentReceiver, photodiode  # noqa: F401
from .wdm_tx import basicLaserModel  # noqa: F401
