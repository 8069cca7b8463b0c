"""Golden fixtures for the Glitch component (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* gl_wls : WLS.  A Vela-like isolated pulsar (F0 11.19 Hz, F1, F2, equatorial astrometry with
           proper motion, DM) with two glitches: glitch 1 with a frozen epoch and every other
           parameter free (phase step, F0/F1/F2 steps, a decaying step with its time constant),
           glitch 2 -- listed first in the par file -- with a free epoch and free F0/F1 steps and
           no GLPH line.  400 TOAs at 1400 / 2300 MHz from the geocentre over MJD 54500-55600,
           20 us errors; TZRMJD lies between the two epochs.  Captured from a start perturbed in
           (GLF0_1, GLF0D_1, GLTD_1, GLEP_2, GLF0_2).  Beside what gen_synth.capture(fit="wls")
           records: the absolute phase of the TOAs and of the TZR TOA, the component's
           glitch_phase of both, the post-fit model's as_parfile(), and a 5x5 grid_chisq over
           (GLEP_2, GLTD_1), +-3 sigma of the one-step fit.
* gl_gls : GLS.  gen_synth.pta_par(22, "ELL1") (the bench's per-pulsar shape: DMX, PLRedNoise,
           EFAC/EQUAD) with an ECORR line and one glitch inside the span (GLEP_1 frozen; GLPH_1,
           GLF0_1, GLF1_1 free); 1000 TOAs; the same extra phase arrays.  Like the family's
           EFAC/EQUAD lines the ECORR line selects on `-f fake`, which these TOAs do not carry:
           the component is in the model but has no epochs, because a pulsar with ECORR epochs
           leaves the generated-Fourier compact fit path this fixture has to take.
* gl_fit_spread.json : gen_fit_spread.measure(model, toas, fit, down=True) of the two, in
           fit_spread.json's schema, plus under "downhill" the per-parameter Downhill spread by
           gen_downhill_spread.spread's loop (5 ps residual shifts, 8 seeds).

Both builders assert the conditions the tests rely on: no TOA (nor the TZR TOA) within 1 ms of a
glitch epoch -- the grid's GLEP_2 values included -- and at least 20 TOAs on either side of
every glitch.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_glitch.py [gl_wls gl_gls spread]
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
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402

from gen_solar_wind import with_save, write_par, downhill_spread  # noqa: E402


def wls_par(glf0_1="2.3e-5", glf0d_1="1.5e-7", gltd_1="35", glep_2="55300.5", glf0_2="4e-8"):
    return f"""PSR J0835-GL
RAJ 08:35:20.61149 1
DECJ -45:10:34.8751 1
PMRA -49.68 1
PMDEC 29.9 1
POSEPOCH 55000
F0 11.18965 1
F1 -1.5567e-11 1
F2 1e-21 1
PEPOCH 55000
DM 67.99 1
GLEP_2 {glep_2} 1
GLF0_2 {glf0_2} 1
GLF1_2 -3e-15 1
GLEP_1 54800.25
GLPH_1 0.13 1
GLF0_1 {glf0_1} 1
GLF1_1 -1.2e-13 1
GLF2_1 2e-22 1
GLF0D_1 {glf0d_1} 1
GLTD_1 {gltd_1} 1
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55100.1234
TZRFRQ 1400
TZRSITE geocenter
"""


GLS_GLITCH = "GLEP_1 55000.37\nGLPH_1 {glph} 1\nGLF0_1 {glf0} 1\nGLF1_1 -1e-17 1\n"
GLS_ECORR = "ECORR -f fake 0.3\n"


def gls_par(glph="0.05", glf0="2e-8"):
    return pta_par(22, "ELL1") + GLS_ECORR + GLS_GLITCH.format(glph=glph, glf0=glf0)


def check_epochs(model, ts, more_epochs=()):
    """No TOA nor the TZR TOA within 1 ms of a glitch epoch; >= 20 TOAs on either side."""
    delay = model.delay(ts).to_value(u.s)
    tz = model.get_TZR_toa(ts)
    tzd = model.delay(tz).to_value(u.s)
    eps = [np.longdouble(getattr(model, n).value) for n in model.params if n.startswith("GLEP_")]
    for ep in eps + [np.longdouble(e) for e in more_epochs]:
        dt = np.asarray((ts.table["tdbld"] - ep) * 86400 - delay, dtype=np.float64)
        dz = float((tz.table["tdbld"][0] - ep) * 86400 - tzd[0])
        assert np.min(np.abs(dt)) > 1e-3 and abs(dz) > 1e-3, (ep, np.min(np.abs(dt)), dz)
        if ep in eps:
            assert np.sum(dt < 0) >= 20 and np.sum(dt > 0) >= 20, (ep, np.sum(dt < 0), np.sum(dt > 0))
        print(f"  epoch {float(ep):.4f}: {int(np.sum(dt < 0))} TOAs before, {int(np.sum(dt > 0))} after, "
              f"nearest {np.min(np.abs(dt)):.3g} s, TZR {dz:.3g} s", file=sys.stderr)


def phase_arrays(model, ts):
    """The absolute phase (abs_phase=False: no TZR subtraction) of the TOAs and of the TZR TOA,
    and Glitch.glitch_phase of both (timing_model.py:1548 phase, glitch.py:193)."""
    out = {}
    tz = model.get_TZR_toa(ts)
    gl = model.components["Glitch"]
    for key, t in (("abs", ts), ("tzr_abs", tz)):
        ph = model.phase(t, abs_phase=False)
        out[key + "_phase_int"] = np.asarray(ph.int.value, dtype=np.float64)
        out[key + "_phase_frac_hi"], out[key + "_phase_frac_lo"] = split_ld(ph.frac.value)
    for key, t in (("glitch_phase", ts), ("tzr_glitch_phase", tz)):
        g = np.asarray(gl.glitch_phase(t, model.delay(t)).value, dtype=np.longdouble)
        out[key + "_hi"], out[key + "_lo"] = split_ld(g)
    print(f"  glitch phase up to {float(np.max(np.abs(out['glitch_phase_hi']))):.4g} cycles, TZR "
          f"{float(out['tzr_glitch_phase_hi'][0]):.6g}", file=sys.stderr)
    return out


def build_wls():
    np.random.seed(41)
    true = get_model(io.StringIO(wls_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 400, true, freq=np.tile([1400.0, 2300.0], 200) * u.MHz,
                                    obs="geocenter", error=20 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = wls_par(glf0_1="2.30002e-5", glf0d_1="1.53e-7", gltd_1="35.5", glep_2="55300.5002", glf0_2="4.01e-8")
    return par, get_model(io.StringIO(par)), ts


def build_gls():
    np.random.seed(22)
    true = get_model(io.StringIO(gls_par()))
    ts = sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False)
    par = gls_par(glph="0.0502", glf0="2.0001e-8")
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def gen_wls():
    par, model, ts = build_wls()
    write_par("gl_wls", par)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    print(f"  WLS chi2 {float(chi2):.3f}; GLEP_2 {f.model.GLEP_2.value} +- {f.model.GLEP_2.uncertainty_value:.3g} d, "
          f"GLTD_1 {f.model.GLTD_1.value:.4f} +- {f.model.GLTD_1.uncertainty_value:.3g} d", file=sys.stderr)
    g0 = np.longdouble(f.model.GLEP_2.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.GLEP_2.uncertainty_value)
    g1 = np.longdouble(f.model.GLTD_1.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.GLTD_1.uncertainty_value)
    check_epochs(model, ts, more_epochs=list(g0) + [f.model.GLEP_2.value])
    more = phase_arrays(model, ts)
    more["grid_GLEP_2_hi"], more["grid_GLEP_2_lo"] = split_ld(g0)
    more["grid_GLTD_1_hi"], more["grid_GLTD_1_lo"] = split_ld(g1)
    fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
    c2, _ = grid_chisq(fg, ("GLEP_2", "GLTD_1"), (g0, g1 * u.d), ncpu=1, printprogress=False)
    more["grid_chi2"] = np.asarray(c2, dtype=np.float64)
    M, names, _ = model.designmatrix(ts)
    s = M / np.sqrt(np.sum(M * M, axis=0))
    print(f"  {len(names)} columns, scaled condition number {np.linalg.cond(s):.3g}; "
          f"grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
    # (the parameter lines only: the header names the run that wrote it)
    text = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    with_save(gen_synth, "gl_wls", more, {"wls_parfile": text})
    capture("gl_wls", model, ts, fit="wls")


def gen_gls():
    par, model, ts = build_gls()
    write_par("gl_gls", par)
    check_epochs(model, ts)
    with_save(gen_synth, "gl_gls", phase_arrays(model, ts), {})
    capture("gl_gls", model, ts, fit="gls")


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "gl_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    todo = {"gl_wls": (build_wls, "wls", pfit.DownhillWLSFitter), "gl_gls": (build_gls, "gls", pfit.DownhillGLSFitter)}
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
    which = sys.argv[1:] or ["gl_wls", "gl_gls", "spread"]
    if "gl_wls" in which:
        gen_wls()
    if "gl_gls" in which:
        gen_gls()
    if "spread" in which:
        gen_spread([n for n in ("gl_wls", "gl_gls") if n in which] or ["gl_wls", "gl_gls"])
