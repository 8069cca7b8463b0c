"""pint_amd — MI355X-native implementation of PINT's fit-and-residual hot path.

Reference API kept (Jackson-D-Taylor/PINT): get_model / get_model_and_toas
(model_builder.py:777/:859), Residuals (residuals.py:40), WLSFitter / GLSFitter /
DownhillWLSFitter / DownhillGLSFitter / Fitter.auto (fitter.py), grid_chisq
(gridutils.py:166).  Compute runs in libpint_hip.so (hand-written HIP for gfx950) via a
ctypes C-ABI (include/pint_amd.h); there is no CPU fallback.
"""
from .timing_model import TimingModel, get_model  # noqa: F401
from .toa import TOAs, get_TOAs, get_TOAs_array, get_model_and_toas  # noqa: F401
from .residuals import Residuals, WidebandDMResiduals, WidebandTOAResiduals  # noqa: F401
from .fitter import (Fitter, WLSFitter, GLSFitter, DownhillWLSFitter, DownhillGLSFitter, WidebandTOAFitter,  # noqa: F401
                     WidebandDownhillFitter,  # noqa: F401
                     MaxiterReached, StepProblem, InvalidModelParameters, CorrelatedErrors)
from .gridutils import grid_chisq, grid_chisq_derived, tuple_chisq, tuple_chisq_derived  # noqa: F401
from .wavex import wavex_setup, dmwavex_setup, cmwavex_setup, get_wavex_freqs, get_wavex_amps  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # BayesianTiming (bayesian.py) and the priors need scipy.stats: imported at first use, so
    # that `import pint_amd` stays as quick as it was
    if name == "BayesianTiming":
        from .bayesian import BayesianTiming
        return BayesianTiming
    # the photon-event modules (event_optimize needs scipy.stats too): the same rule
    if name == "PhotonTiming":
        from .event_optimize import PhotonTiming
        return PhotonTiming
    if name == "get_event_TOAs":
        from .event_toas import get_event_TOAs
        return get_event_TOAs
    if name in ("Polycos", "PolycoEntry"):
        from . import polycos
        return getattr(polycos, name)
    # the ensemble sampler over the batched posteriors, and the fitter on it
    if name in ("EnsembleSampler", "get_initial_pos", "integrated_time"):
        from . import sampler
        return getattr(sampler, name)
    if name == "MCMCFitter":
        from .mcmc_fitter import MCMCFitter
        return MCMCFitter
    if name in ("eventstats", "event_optimize", "event_toas", "polycos", "sampler", "mcmc_fitter"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
