"""Golden fixtures for the ChromaticCM and CMWaveX components (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* cm_wls : WLS.  An isolated pulsar (F0 218 Hz, F1, equatorial astrometry, DM) with CM, CM1, CM2
           free and non-zero, CMEPOCH different from PEPOCH, no TNCHROMIDX line (the default 4),
           CMWaveX harmonics 0001 and 0003 (a gap; 0003 non-harmonic, CMWXCOS_0003 frozen
           non-zero), CMWXEPOCH given, one WaveX harmonic and one glitch inside the span.
           400 TOAs at 430 / 820 / 1400 / 2300 MHz from the geocentre over MJD 54500-55600, 1 us
           errors.  Captured from a perturbed start.  Beside what gen_synth.capture(fit="wls")
           records: the absolute phase of the TOAs and of the TZR TOA, each chromatic component's
           delay for both, the post-fit as_parfile(), a 5x5 grid_chisq over (CM, DM), +-3 sigma of
           the one-step fit, what the reference does with "TNCHROMIDX 4 1", the reference's
           cmwavex_setup ("setup") and change_cmepoch ("cmepoch").
* cm_gls : GLS.  gen_synth.pta_par(22, "ELL1") (the bench's per-pulsar shape: DMX, PLRedNoise,
           EFAC/EQUAD) with CM free, TNCHROMIDX 2.6, 4 CMWaveX harmonics from the reference's
           cmwavex_setup (no CMWXEPOCH line: PEPOCH fills it in), every amplitude free and
           non-zero, and 2 DMWaveX harmonics; 1000 TOAs at 800 / 1200 / 1600 / 2000 MHz.
* cm_fit_spread.json : gen_fit_spread.measure of the two plus the Downhill spread, in
           wx_fit_spread.json's schema.

The builders assert the conditions the tests rely on (see check() and fixed_point()).

The order of the delay components.  dmwavex, chromatic_constant and cmwavex are not categories of
the reference's DEFAULT_ORDER, so DMWaveX, ChromaticCM and CMWaveX follow everything else in the
order its model builder adds them -- the iteration order of a set of names, which changes with the
interpreter's hash seed, as does the order of the component types (phase, delay, noise), which
places a glitch's parameters before or after the delay components'.  The device path sums
... WaveX, DMWaveX, ChromaticCM, CMWaveX and its host model lists the phase components'
parameters first, as the committed wx_wls / gl_wls fixtures have them; the fixtures are captured
in a run that has both (check() asserts it; seed 34 gives it), so that the parameter and column
orders recorded are the ones the host model has.

Usage: PYTHONHASHSEED=34 oracle/refenv/run_ref.sh scripts/refgen/gen_chromatic.py [cm_wls cm_gls spread]
"""
import copy
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle", "refgen"))

import astropy.units as u  # noqa: E402
import refcommon  # noqa: E402
from refcommon import GOLDEN, register_clockless_sites, split_ld  # noqa: E402
import gen_synth  # noqa: E402
from gen_synth import pta_par, capture  # noqa: E402  (the real capture: gen_fit_spread replaces the module's)
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
from pint import DMconst  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402
from pint.utils import cmwavex_setup, dmwavex_setup  # noqa: E402

from gen_solar_wind import with_save, write_par, downhill_spread  # noqa: E402

CANONICAL = ["WaveX", "DMWaveX", "ChromaticCM", "CMWaveX"]
CHROM_FUNCS = {"cm_delay": "constant_chromatic_delay", "cmwavex_delay": "cmwavex_delay"}


def wls_par(cm="52.0", cm1="9.0", cm2="-6.0", s1="31.0", c1="-24.0", s3="-18.0", wxsin="1.5e-6", glf0_1="3e-9",
            idx_line=""):
    return f"""PSR J1012-CM
RAJ 10:12:33.4372 1
DECJ 53:07:02.512 1
F0 218.8118404 1
F1 -4.08e-16 1
PEPOCH 55000
POSEPOCH 55000
DM 9.0233 1
CM2 {cm2} 1
CM {cm} 1
CM1 {cm1} 1
CMEPOCH 55090.25
{idx_line}CMWXEPOCH 55050.5
CMWXFREQ_0003 0.00417
CMWXSIN_0003 {s3} 1
CMWXCOS_0003 21.0
CMWXFREQ_0001 0.00090909090909090909
CMWXSIN_0001 {s1} 1
CMWXCOS_0001 {c1} 1
WXEPOCH 55050.5
WXFREQ_0001 0.0018181818181818182
WXSIN_0001 {wxsin} 1
WXCOS_0001 -0.8e-6 1
GLEP_1 55120.3
GLF0_1 {glf0_1} 1
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55400.1234
TZRFRQ 1400
TZRSITE geocenter
"""


T_GLS = 3652.0
CMWX_TRUE = [(0.030, -0.024), (0.022, 0.027), (-0.019, 0.016), (0.015, -0.018)]
DMWX_TRUE = [(1.0e-4, -1.4e-4), (0.8e-4, 0.6e-4)]


def gls_par(scale=1.0, cm=0.05):
    """pta_par(22, "ELL1") plus the lines of the reference's own cmwavex_setup / dmwavex_setup."""
    m = get_model(io.StringIO(pta_par(22, "ELL1") + "CM 0.0\n"))
    icm = cmwavex_setup(m, T_GLS, n_freqs=len(CMWX_TRUE))
    idm = dmwavex_setup(m, T_GLS, n_freqs=len(DMWX_TRUE))
    lines = f"CM {cm!r} 1\nTNCHROMIDX 2.6\n"
    for i, (s, c) in zip(icm, CMWX_TRUE):
        lines += (f"CMWXFREQ_{i:04d} {getattr(m, f'CMWXFREQ_{i:04d}').value!r}\n"
                  f"CMWXSIN_{i:04d} {s * scale!r} 1\nCMWXCOS_{i:04d} {c * scale!r} 1\n")
    lines += "DMWXEPOCH 54900\n"
    for i, (s, c) in zip(idm, DMWX_TRUE):
        lines += (f"DMWXFREQ_{i:04d} {getattr(m, f'DMWXFREQ_{i:04d}').value!r}\n"
                  f"DMWXSIN_{i:04d} {s * scale!r} 1\nDMWXCOS_{i:04d} {c * scale!r} 1\n")
    return pta_par(22, "ELL1") + lines


def extra_arrays(model, ts):
    """The absolute phase (abs_phase=False: no TZR subtraction) of the TOAs and of the TZR TOA, and
    each chromatic component's delay for both."""
    out = {}
    tz = model.get_TZR_toa(ts)
    for key, t in (("abs", ts), ("tzr_abs", tz)):
        ph = model.phase(t, abs_phase=False)
        out[key + "_phase_int"] = np.asarray(ph.int.value, dtype=np.float64)
        out[key + "_phase_frac_hi"], out[key + "_phase_frac_lo"] = split_ld(ph.frac.value)
    for key, t in (("", ts), ("tzr_", tz)):
        parts = refcommon.component_delays(model, t)
        for n, fn in CHROM_FUNCS.items():
            out[key + n] = parts["delay_" + fn]
    return out


def check(model, ts, more, alpha_test=False):
    """The conditions the tests rely on; returns the recorded figures."""
    order = [type(c).__name__ for c in model.DelayComponent_list if type(c).__name__ in CANONICAL]
    assert order == [c for c in CANONICAL if c in order], (order, "run with another PYTHONHASHSEED (34)")
    assert list(model.components.keys())[0] == "AbsPhase", "run with another PYTHONHASHSEED (34)"
    M, names, _ = model.designmatrix(ts)
    names = list(names)
    chrom = [n for n in names if n == "CM" or (n.startswith("CM") and n[2:].isdigit())
             or n.startswith(("CMWXSIN_", "CMWXCOS_"))]
    assert chrom, names
    for n in chrom:
        assert np.max(np.abs(M[:, names.index(n)])) > 0, n
    for n in CHROM_FUNCS:
        assert np.max(np.abs(more[n])) > 2.5e-6, (n, np.max(np.abs(more[n])))
    meta = {}
    if alpha_test:  # a hard-wired exponent 4 must miss
        bf = model.barycentric_radio_freq(ts).to_value(u.MHz)
        cm = model.components["ChromaticCM"].cm_value(ts).value
        d4 = np.asarray(cm * DMconst.value * bf ** (-4.0), dtype=np.float64)
        rel = float(np.max(np.abs(d4 - more["cm_delay"]) / np.abs(more["cm_delay"])))
        assert rel > 1e-6, rel
        meta["cm_alpha4_rel"] = rel
    tdb = ts.table["tdbld"]
    amax = 0.0
    for n in model.params:
        if n.startswith("CMWXFREQ_"):
            ap = np.asarray(2.0 * np.pi * getattr(model, n).value * (tdb - model.CMWXEPOCH.value), dtype=np.float64)
            amax = max(amax, float(np.max(np.abs(ap))))
    s = M / np.sqrt(np.sum(M * M, axis=0))
    cond = float(np.linalg.cond(s.T @ s))
    print(f"  {len(names)} columns, normalised Gram condition number {cond:.3g}; max|a'| {amax:.4g}; "
          f"cm delay up to {np.max(np.abs(more['cm_delay'])):.3g} s, cmwavex delay up to "
          f"{np.max(np.abs(more['cmwavex_delay'])):.3g} s", file=sys.stderr)
    assert cond < 1e12, cond
    meta.update({"cmwx_max_arg": amax, "cm_gram_cond": cond,
                 "delay_components": [type(c).__name__ for c in model.DelayComponent_list]})
    return meta


def check_errors(f):
    errs = np.array([getattr(f.model, p).uncertainty_value for p in f.model.free_params], dtype=np.float64)
    assert np.all(np.isfinite(errs)) and np.all(errs > 0), errs


def fixed_point(model, ts, down_cls, step_cls):
    """How far one more plain fit step moves the reference's Downhill result, in sigma (the worst
    parameter).  Downhill keeps the iterate with the lowest chi2, and near the minimum the
    reference's own chi2 rounding (1e-7 relative from one iterate to the next) decides which that
    is; two correct implementations may stop one iterate apart.  The start is chosen so that this
    does not matter at the tests' 1e-3 sigma: the figure must be below a quarter of it."""
    f = down_cls(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=10)
    h = step_cls(ts, copy.deepcopy(f.model))
    h.fit_toas(maxiter=1)
    dev = {p: abs(float((getattr(h.model, p).value - getattr(f.model, p).value) / getattr(f.model, p).uncertainty_value))
           for p in f.model.free_params}
    pw = max(dev, key=dev.get)
    print(f"  Downhill result to one more step: {dev[pw]:.2e} sigma ({pw})", file=sys.stderr)
    assert dev[pw] < 2.5e-4, (pw, dev[pw])
    return {"sigma": dev[pw], "param": pw}


def setup_records():
    """Indices and frequencies of the reference's cmwavex_setup."""
    rec = {}
    base = wls_par().split("CMWXEPOCH")[0] + "EPHEM builtin\nUNITS TDB\n"
    for case, kw in (("n3", dict(n_freqs=3)), ("list", dict(freqs=[0.004, 0.001, 0.0025])),
                     ("list1", dict(freqs=[0.0025])), ("frozen", dict(n_freqs=2, freeze_params=True))):
        m = get_model(io.StringIO(base))
        try:
            idx = [int(i) for i in cmwavex_setup(m, 1000.0, **kw)]
        except Exception as e:  # (recorded: the tests reproduce what the reference does)
            rec[f"cmwavex_{case}"] = {"error": type(e).__name__}
            continue
        rec[f"cmwavex_{case}"] = {
            "indices": idx, "freqs": [float(getattr(m, f"CMWXFREQ_{i:04d}").value) for i in idx],
            "frozen": [bool(getattr(m, n).frozen) for n in m.params if n.startswith("CMWXSIN_")],
            "params": [n for n in m.params if n.startswith("CM") or n == "TNCHROMIDX"],
            "free_params": list(m.free_params), "components": list(m.components.keys())}
    m = get_model(io.StringIO(base))
    try:
        cmwavex_setup(m, 1000.0, freqs=[0.001], n_freqs=1)
    except Exception as e:
        rec["cmwavex_both"] = type(e).__name__
    return rec


def cmepoch_record():
    """ChromaticCM.change_cmepoch of the cm_wls model to MJD 55400.75: the terms before and after."""
    m = get_model(io.StringIO(wls_par()))
    comp = m.components["ChromaticCM"]
    rec = {"new_epoch": 55400.75, "before": [repr(np.longdouble(q.value)) for q in comp.get_CM_terms()]}
    comp.change_cmepoch(55400.75)
    rec["after"] = [str(np.longdouble(q.value)) for q in comp.get_CM_terms()]
    rec["after_hi_lo"] = [[float(x) for x in split_ld(np.longdouble(q.value))] for q in comp.get_CM_terms()]
    rec["cmepoch_after"] = float(m.CMEPOCH.value)
    return rec


def idx_fit_behaviour(ts):
    """What the reference does with a TNCHROMIDX line whose fit flag is 1."""
    par = wls_par(idx_line="TNCHROMIDX 4 1\n")
    out = {"par_line": "TNCHROMIDX 4 1"}
    try:
        m = get_model(io.StringIO(par))
        out["frozen"] = bool(m.TNCHROMIDX.frozen)
        out["in_free_params"] = "TNCHROMIDX" in m.free_params
        m.designmatrix(ts)
        out["designmatrix"] = "ok"
    except Exception as e:
        out["designmatrix"] = type(e).__name__
        out["message"] = str(e)
    return out


def build_wls():
    np.random.seed(61)
    true = get_model(io.StringIO(wls_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 400, true, freq=np.tile([430.0, 820.0, 1400.0, 2300.0], 100) * u.MHz,
                                    obs="geocenter", error=1 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = wls_par(cm="51.0", cm1="9.6", cm2="-5.5", s1="29.5", c1="-25.0", s3="-17.0", wxsin="1.3e-6",
                  glf0_1="3.002e-9")
    return par, get_model(io.StringIO(par)), ts


def build_gls():
    np.random.seed(23)
    true = get_model(io.StringIO(gls_par()))
    ts = sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False)
    par = gls_par(scale=0.97, cm=0.0495)
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def gen_wls():
    par, model, ts = build_wls()
    write_par("cm_wls", par)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    check_errors(f)
    print(f"  WLS chi2 {float(chi2):.3f}; CM {f.model.CM.value:.5g} +- {f.model.CM.uncertainty_value:.3g}",
          file=sys.stderr)
    g0 = np.longdouble(f.model.CM.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.CM.uncertainty_value)
    g1 = np.longdouble(f.model.DM.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.DM.uncertainty_value)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    more["grid_CM_hi"], more["grid_CM_lo"] = split_ld(g0)
    more["grid_DM_hi"], more["grid_DM_lo"] = split_ld(g1)
    fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
    c2, _ = grid_chisq(fg, ("CM", "DM"), (g0 * f.model.CM.units, g1 * u.pc / u.cm ** 3), ncpu=1, printprogress=False)
    more["grid_chi2"] = np.asarray(c2, dtype=np.float64)
    print(f"  grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
    # (the parameter lines only: the header names the run that wrote it)
    meta["wls_parfile"] = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    meta["setup"] = setup_records()
    meta["cmepoch"] = cmepoch_record()
    meta["idx_fit"] = idx_fit_behaviour(ts)
    meta["delay_funcs"] = [df.__name__ for df in model.delay_funcs]
    meta["down_fixed_point"] = fixed_point(model, ts, pfit.DownhillWLSFitter, pfit.WLSFitter)
    with_save(gen_synth, "cm_wls", more, meta)
    capture("cm_wls", model, ts, fit="wls")


def gen_gls():
    par, model, ts = build_gls()
    write_par("cm_gls", par)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more, alpha_test=True)
    f = pfit.GLSFitter(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=1)
    check_errors(f)
    meta["gls_parfile"] = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    meta["delay_funcs"] = [df.__name__ for df in model.delay_funcs]
    meta["down_fixed_point"] = fixed_point(model, ts, pfit.DownhillGLSFitter, pfit.GLSFitter)
    with_save(gen_synth, "cm_gls", more, meta)
    capture("cm_gls", model, ts, fit="gls")


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "cm_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    todo = {"cm_wls": (build_wls, "wls", pfit.DownhillWLSFitter), "cm_gls": (build_gls, "gls", pfit.DownhillGLSFitter)}
    for n in names:
        build, fit, cls = todo[n]
        _, model, ts = build()
        gen_fit_spread.check_same(n, ts)
        res[n] = gen_fit_spread.measure(model, ts, fit, True)
        res[n]["downhill"] = downhill_spread(model, ts, cls)
        print(n, json.dumps(res[n]), file=sys.stderr, flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    register_clockless_sites()
    which = sys.argv[1:] or ["cm_wls", "cm_gls", "spread"]
    if "cm_wls" in which:
        gen_wls()
    if "cm_gls" in which:
        gen_gls()
    if "spread" in which:
        gen_spread([n for n in ("cm_wls", "cm_gls") if n in which] or ["cm_wls", "cm_gls"])
