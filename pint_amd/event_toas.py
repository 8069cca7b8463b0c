"""Photon event times as TOAs (reference ``src/pint/event_toas.py``, the part after the FITS file is
read): every photon becomes a TOA at infinite frequency with a 1 us error, prepared by pint_amd.prep
like the TOAs of a tim file, so that the device evaluates its absolute phase.

Event lists come in two forms (event_toas.py load_fits_TOAs): geocentred times in TT (``gtbary
tcorrect=geo``, or a satellite's times moved to the geocenter) and barycentred times in TDB (``gtbary``,
``barycorr``).  Both are taken here as MJD arrays; reading FITS files and spacecraft orbit files is
out of scope.
"""
from __future__ import annotations

import numpy as np

from .toa import TOAs

LD = np.longdouble
EVENT_ERROR_US = 1.0  # (event_toas.py: every event TOA carries a 1 us error)


def get_event_TOAs(mjds, timesys="TT", obs="geocenter", weights=None, energies=None, model=None) -> TOAs:
    """TOAs of photon arrival times.

    mjds : the event MJDs (float64 or longdouble; longdouble keeps sub-ns precision).
    timesys, obs : "TT" with "geocenter", or "TDB" with "barycenter"; other combinations are refused.
    weights, energies : one value per photon, kept as the columns "weights" and "energies" (keV or
        whatever unit the caller uses; they do not enter the timing).
    model : when given, its EPHEM / CLOCK are checked like get_TOAs does, and the TZR TOA comes from it
        (TOAs.tzr_for: TZRMJD at TZRSITE, prepared the same way).
    """
    from . import prep
    from .toa import _bipm_choice, _ephem_choice
    t = np.atleast_1d(np.asarray(mjds))
    t = t.astype(LD) if t.dtype != LD else t
    if t.ndim != 1 or t.size == 0:
        raise ValueError("No events found!")
    ts, site = str(timesys).upper(), str(obs).lower()
    n = t.size
    if (ts, site) == ("TT", "geocenter"):
        day, frac = prep.tt_to_utc_parts(t)  # (prep.prepare takes the geocenter's times in UTC)
    elif (ts, site) == ("TDB", "barycenter"):
        day = np.floor(t.astype(np.float64))
        frac = (t - LD(day)).astype(np.float64)
    else:
        raise NotImplementedError(f"event times in {timesys} at {obs}: only TT at the geocenter and TDB at the "
                                  "barycenter are built (spacecraft-local times need an orbit file)")
    ephem = _ephem_choice(None, model)
    if model is not None:
        _bipm_choice(False, model)
    cols = prep.prepare(day, frac, [site] * n)
    cols["freq_mhz"] = np.full(n, np.inf)
    cols["err_us"] = np.full(n, EVENT_ERROR_US)
    cols["delta_pulse_number"] = np.zeros(n)
    for name, v in (("weights", weights), ("energies", energies)):
        if v is not None:
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (n,):
                raise ValueError(f"{name} must have one value per event ({n}), got {v.shape}")
            cols[name] = v.copy()
    out = TOAs(cols, {}, None, "events", [site] * n)
    out.ephem = ephem
    out.clock = "TT(TAI)"
    out.prepared = {"ephem": ephem, "include_bipm": False, "clock_files": None, "planets": False}
    return out
