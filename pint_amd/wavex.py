"""WaveX / DMWaveX set-up helpers, in the reference's signatures and semantics
(``utils.py:1457-1642`` wavex_setup / dmwavex_setup, ``:1841-1954`` get_wavex_freqs /
get_wavex_amps).

The components themselves live in ``TimingModel`` (``add_wavex_component(s)``,
``remove_wavex_component``, ``get_wavex_indices``); their delays and design-matrix columns are
the device kernel ``k_wavex``.  Frequencies are in 1 / d, WaveX amplitudes in s, DMWaveX
amplitudes in pc / cm3, CMWaveX amplitudes in pc / cm3 / MHz2 (``cmwavex_setup``,
``utils.py:1645-1736``; ``get_wavex_freqs`` / ``get_wavex_amps`` are WaveX's alone, as in the reference), and the Wave
<-> WaveX translations (``utils.py:1794``, ``:1957``; host-only).  Not provided:
``find_optimal_nharms``, ``plrednoise_from_wavex`` and ``pldmnoise_from_dmwavex``.
"""
from __future__ import annotations

import warnings

import numpy as np

from .timing_model import WAVEX_STEMS

__all__ = ["wavex_setup", "dmwavex_setup", "cmwavex_setup", "get_wavex_freqs", "get_wavex_amps",
           "translate_wave_to_wavex", "translate_wavex_to_wave"]


def _setup(model, comp, T_span, freqs, n_freqs, freeze_params):
    stem = WAVEX_STEMS[comp]
    if freqs is None and n_freqs is None:
        raise ValueError(f"{comp} component base frequencies are not specified. "
                         "Please input either freqs or n_freqs")
    if freqs is not None and n_freqs is not None:
        raise ValueError("Both freqs and n_freqs are specified. Only one or the other should be used")
    if n_freqs is not None and n_freqs <= 0:
        raise ValueError("Must use a non-zero number of wave frequencies")
    T_span = float(T_span)
    model._ensure_wavex(comp)  # (add_component(WaveX()): harmonic 0001 at 0.1 / d, free zero amplitudes)
    first = model[f"{stem}FREQ_0001"]
    if freqs is not None:
        freqs = np.sort(np.atleast_1d(np.asarray(freqs, dtype=np.float64)))
        if len(freqs) > 1 and np.min(np.diff(freqs)) < 1.0 / (2.0 * T_span):
            warnings.warn(("Wave" if comp == "WaveX" else comp) +
                          " frequency spacing is finer than frequency resolution of data")
    else:
        freqs = np.arange(1, n_freqs + 1) / T_span
    first.value = float(freqs[0])
    if len(freqs) > 1:
        model.add_wavex_components(freqs[1:], component=comp)
    for n in model.params:
        if n.startswith((f"{stem}SIN", f"{stem}COS")):
            model[n].frozen = bool(freeze_params)
    return model.get_wavex_indices(comp)


def wavex_setup(model, T_span, freqs=None, n_freqs=None, freeze_params=False):
    """Set up a WaveX model from a list of frequencies (1 / d) or from ``n_freqs`` harmonics
    ``n / T_span``; amplitudes start at zero.  Assumes the model has no WaveX component yet.
    Returns the indices of the harmonics."""
    return _setup(model, "WaveX", T_span, freqs, n_freqs, freeze_params)


def dmwavex_setup(model, T_span, freqs=None, n_freqs=None, freeze_params=False):
    """wavex_setup for DMWaveX."""
    return _setup(model, "DMWaveX", T_span, freqs, n_freqs, freeze_params)


def cmwavex_setup(model, T_span, freqs=None, n_freqs=None, freeze_params=False):
    """wavex_setup for CMWaveX (``utils.py:1645-1736``); amplitudes in pc / cm3 / MHz2.  The model
    needs a ChromaticCM component (CM, TNCHROMIDX) before it validates or evaluates."""
    return _setup(model, "CMWaveX", T_span, freqs, n_freqs, freeze_params)


def _drop_component(model, comp):
    for n in [n for n, p in model._params.items() if p.component == comp]:
        model.remove_param(n)
    model.components.pop(comp, None)


def translate_wave_to_wavex(model):
    """utils.py:1794-1838: a copy of the model with its Wave component replaced by a WaveX
    component: WXEPOCH = WAVEEPOCH, WXFREQ_k = k WAVE_OM / (2 pi) for WAVEk, k = 1 ... n, and
    WXSIN_k / WXCOS_k = -a_k / -b_k (a Wave term is a phase, a WaveX term a delay).  As in the
    reference the first harmonic keeps the constructor's free amplitudes and the others are
    frozen."""
    from . import parameter as P
    new = model.copy()
    terms = [model[n] for n in model.wave_terms()]
    om, epoch = model.WAVE_OM.value, model.WAVEEPOCH.value
    _drop_component(new, "Wave")
    new._ensure_wavex("WaveX")
    new.WXEPOCH.value = P.LD(epoch)
    for k, t in enumerate(terms):
        a, b = t.value
        f = (om * (k + 1)) / (2.0 * np.pi)
        if k == 0:
            new.WXFREQ_0001.value, new.WXSIN_0001.value, new.WXCOS_0001.value = float(f), float(-a), float(-b)
        else:
            new.add_wavex_component(f, wxsin=float(-a), wxcos=float(-b))
    return new


def translate_wavex_to_wave(model):
    """utils.py:1957-1999: a copy of the model with its WaveX component replaced by a Wave
    component.  Every harmonic must give the same WAVE_OM = 2 pi WXFREQ_k / k (to 1e-3 / d, the
    reference's allclose); their mean becomes WAVE_OM, WAVEEPOCH = WXEPOCH and WAVEk = (-WXSIN_k,
    -WXCOS_k)."""
    from . import parameter as P
    new = model.copy()
    indices = [int(i) for i in model.get_wavex_indices("WaveX")]
    oms = [(2.0 * np.pi * model[f"WXFREQ_{i:04d}"].value) / (i - 1 + 1.0) for i in indices]
    if len(oms) > 1 and not np.allclose(oms, oms[0], atol=1e-3):
        raise ValueError("This WaveX model cannot be properly translated into a Wave model due to the WaveX "
                         "frequencies not producing a consistent WAVEOM value")
    om = oms[0] if len(oms) == 1 else sum(oms) / len(oms)
    amps = [(model[f"WXSIN_{i:04d}"].value, model[f"WXCOS_{i:04d}"].value) for i in indices]
    epoch = model.WXEPOCH.value
    _drop_component(new, "WaveX")
    for n, v in (("WAVEEPOCH", None if epoch is None else P.LD(epoch)), ("WAVE_OM", float(om))):
        p = P.make_param(n)
        p.value = v
        new.add_param(p)
    for i, (s, c) in zip(indices, amps):
        p = P.make_param(f"WAVE{i}")
        p.value = (P.LD(s) * P.LD(-1.0), P.LD(c) * P.LD(-1.0))
        new.add_param(p)
    new.validate()
    return new


def _select(model, index, pick):
    if index is None:
        idx = list(model.get_wavex_indices("WaveX"))
        return pick(idx[0]) if len(idx) == 1 else [pick(i) for i in idx]
    if isinstance(index, (int, float, np.integer)):
        return pick(int(index))
    if isinstance(index, (list, set, np.ndarray)):
        return [pick(int(i)) for i in index]
    raise TypeError(f"index most be a float, int, set, list, array, or None - not {type(index)}")


def get_wavex_freqs(model, index=None, quantity=False):
    """The WXFREQ_ parameters of the model (all, one index, or a list of indices); with
    ``quantity`` their values."""
    out = _select(model, index, lambda i: model[f"WXFREQ_{i:04d}"])
    if quantity:
        return [p.quantity for p in out] if isinstance(out, list) else [out.quantity]
    return out


def get_wavex_amps(model, index=None, quantity=False):
    """The (WXSIN_, WXCOS_) parameter pairs of the model (all, one index, or a list of
    indices); with ``quantity`` their values."""
    out = _select(model, index, lambda i: (model[f"WXSIN_{i:04d}"], model[f"WXCOS_{i:04d}"]))
    if quantity:
        return [(s.quantity, c.quantity) for s, c in out] if isinstance(out, list) else tuple(p.quantity for p in out)
    return out
