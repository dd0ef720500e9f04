"""opticommpy_amd -- MI355X-native split-step Fourier fiber propagation.

Drop-in for the fiber-channel functions of OptiCommPy's ``optic.models.modelsGPU``
(``ssfm``, ``manakovSSF``, ``manakovDBP``, ``edfa``, ``setPowerforParSSFM``) plus
``checkGPU``: numpy in, numpy out, same parameters-object API.  Host code is plain
Python + numpy calling hand-written HIP kernels (gfx950) through the C ABI declared
in ``include/ssf.h`` (``libssf_hip.so``).  There is no CPU fallback: without the
library or without a GPU every propagation call raises.

The receiver side is there as well, on numpy arrays and ``DeviceArray``s alike: the coherent chain (``pdmCoherentReceiver``,
``decimate``, ``edc``, ``symbolSync``, ``mimoAdaptEqualizer``, ``cpr``, ``metrics``, ``calcLLR``, ``decodeLDPC``) and the
equalizers of the direct-detection chain, ``ffe``, ``dfe`` and ``volterra`` with ``pnorm`` and ``anorm``
(``opticommpy_amd.sisoeq``; also importable from ``opticommpy_amd.equalization``, as in the reference).

The front of the direct-detection notebooks is there too (``opticommpy_amd.imddtx``): ``pamTransmitter``, the modulators ``pm``,
``mzm`` and ``iqm``, ``voa``, ``upsample`` and the ``awgn`` channel on numpy arrays and ``DeviceArray``s, and the host-side sources
``bitSource``, ``prbsGenerator`` and ``symbolSource``; also importable from ``opticommpy_amd.tx``, ``.devices``, ``.channels``,
``.core`` and ``.sources``, as in the reference.

``syncDataSequences`` (``opticommpy_amd.synchronization``) aligns the transmitted sequence to a delayed, repeated received copy and
returns the reference symbols of the equalizers; ``movingAverage`` (also in ``.core``) and ``bert``, ``theoryBER``, ``Qfunc`` (also
in ``.metrics``) complete the names the direct-detection notebooks import.
"""
from .utils import parameters  # noqa: F401
from .models import (  # noqa: F401
    blockwiseFFTConv, checkGPU, convergenceCondition, edc, edfa, linearFiberChannel, manakovDBP, manakovSSF, nlinPhaseRot,
    setPowerforParSSFM, ssfm,
    last_run, set_device, set_engine,
)

from .device import DeviceArray, concatenate, freqShift, full, stack, to_device, zeros  # noqa: F401
from .rx import (  # noqa: F401
    balancedPD, coherentReceiver, decimate, delaySignal, firFilter, iqMixing, lowPassFIR, opticalHybrid2x4, pbs,
    pdmCoherentReceiver, pdmCoherentReceiverChain, photodiode,
)

from .wdm_tx import basicLaserModel, grayMapping, phaseNoise, pulseShape, simpleWDMTx  # noqa: F401
from . import metrics  # noqa: F401  (a callable module: oa.metrics(rx, tx, M, constType) returns all seven link metrics)
from .metrics import calcEVM, demodulateGray, fastBERcalc, monteCarloGMI, monteCarloMI, anorm, pnorm, signalPower  # noqa: F401
from . import theory  # noqa: F401
from .theory import (  # noqa: F401
    ASE_NyquistWDM, GN_Model_NyquistWDM, GNmodel_OSNR, calcLinOSNR, calcMI, condEntropy, constellationMI, theoryMI,
)
from . import cpr  # noqa: F401  (a callable module: oa.cpr(sigIn, param) is the reference's cpr)
from .cpr import bps, bpsGPU, fourthPowerFOE  # noqa: F401
from .sync import finddelay, symbolSync  # noqa: F401
from .equalization import mimoAdaptEqualizer  # noqa: F401
from . import sisoeq  # noqa: F401
from .sisoeq import dfe, ffe, volterra  # noqa: F401
from .fec import calcLLR, decodeLDPC, encodeLDPC, modulateGray, par2gen, readAlist, triangP1P2, writeAlist  # noqa: F401
from .ofdm import calcSymbolRate, demodulateOFDM, hermit, modulateOFDM, zeroPad  # noqa: F401
from .perturbation import calcNLINperturbation, calcNLINperturbationSimplified, calcPertCoeffMatrix, perturbationNLIN  # noqa: F401
from . import imddtx  # noqa: F401
from .imddtx import awgn, bitSource, iqm, mzm, pamTransmitter, pm, prbsGenerator, symbolSource, upsample, voa  # noqa: F401
from . import seqdet  # noqa: F401
from .seqdet import autocorr, detector, estimateWhiteningFilter, levinson, mlse  # noqa: F401
from . import synchronization  # noqa: F401
from .synchronization import Qfunc, bert, movingAverage, syncDataSequences, theoryBER  # noqa: F401
from . import clock  # noqa: F401
from .clock import (  # noqa: F401
    adc, calcClockDrift, clockSamplingInterp, dac, gardnerClockRecovery, gardnerTED, gardnerTEDnyquist, interpolator, quantizer, resample,
)

__all__ = ["simpleWDMTx", "basicLaserModel", "pulseShape", "phaseNoise", "grayMapping", "DeviceArray", "to_device", "firFilter", "lowPassFIR", "decimate", "delaySignal", "iqMixing", "pbs", "photodiode", "balancedPD",
           "opticalHybrid2x4", "coherentReceiver", "pdmCoherentReceiver", "pdmCoherentReceiverChain", "parameters", "ssfm", "manakovSSF", "manakovDBP", "nlinPhaseRot", "convergenceCondition", "edfa", "edc", "blockwiseFFTConv", "linearFiberChannel",
           "setPowerforParSSFM", "checkGPU", "last_run", "set_device", "set_engine",
           "metrics", "fastBERcalc", "monteCarloGMI", "monteCarloMI", "calcEVM", "demodulateGray", "pnorm", "signalPower",
           "cpr", "bps", "bpsGPU", "fourthPowerFOE", "symbolSync", "finddelay", "mimoAdaptEqualizer", "ffe", "dfe", "volterra", "anorm", "calcLLR", "decodeLDPC", "readAlist",
           "encodeLDPC", "modulateGray", "par2gen", "triangP1P2", "writeAlist",
           "modulateOFDM", "demodulateOFDM", "hermit", "zeroPad", "calcSymbolRate",
           "calcPertCoeffMatrix", "calcNLINperturbation", "calcNLINperturbationSimplified", "perturbationNLIN",
           "clockSamplingInterp", "quantizer", "resample", "adc", "dac", "gardnerClockRecovery", "calcClockDrift", "gardnerTED",
           "gardnerTEDnyquist", "interpolator",
           "pamTransmitter", "mzm", "pm", "iqm", "voa", "upsample", "awgn", "bitSource", "prbsGenerator", "symbolSource",
           "mlse", "detector", "autocorr", "levinson", "estimateWhiteningFilter",
           "syncDataSequences", "movingAverage", "bert", "theoryBER", "Qfunc",
           "theoryMI", "constellationMI", "calcMI", "condEntropy", "GN_Model_NyquistWDM", "ASE_NyquistWDM", "GNmodel_OSNR", "calcLinOSNR",
           "concatenate", "stack", "zeros", "full", "freqShift"]
