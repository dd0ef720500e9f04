"""The signal-processing helpers under the reference's module name (optic/dsp/core.py), gathered from the modules that implement
them."""
from .device import freqShift  # noqa: F401
from .clock import clockSamplingInterp, quantizer, resample  # noqa: F401
from .imddtx import upsample  # noqa: F401
from .metrics import anorm, pnorm, signalPower  # noqa: F401
from .models import blockwiseFFTConv  # noqa: F401
from .rx import decimate, delaySignal, firFilter, iqMixing, lowPassFIR  # noqa: F401
from .seqdet import autocorr, estimateWhiteningFilter, levinson  # noqa: F401
from .sync import finddelay, symbolSync  # noqa: F401
from .synchronization import movingAverage  # noqa: F401
from .wdm_tx import phaseNoise, pulseShape  # noqa: F401
