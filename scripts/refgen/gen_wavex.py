"""Golden fixtures for the WaveX and DMWaveX components (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* wx_wls : WLS.  An isolated pulsar (F0 218 Hz, F1, equatorial astrometry, DM) with WaveX
           harmonics 0001, 0002 and 0004 (a gap; 0004 non-harmonic; 0002 at a negative frequency;
           0002 has WXSIN free and WXCOS frozen non-zero), WXEPOCH given and different from
           PEPOCH, and one glitch inside the span (GLEP_1 frozen, GLF0_1 free).  400 TOAs at
           1400 / 2300 MHz from the geocentre over MJD 54500-55600, 1 us errors.  Captured from a
           perturbed start.  Beside what gen_synth.capture(fit="wls") records: the absolute phase
           of the TOAs and of the TZR TOA, wavex_delay of both, the post-fit as_parfile(), a 5x5
           grid_chisq over (WXSIN_0001, F1), +-3 sigma of the one-step fit, and what the reference
           does with a WXFREQ_ line whose fit flag is 1.
* wx_gls : GLS.  gen_synth.pta_par(22, "ELL1") (the bench's per-pulsar shape: DMX, PLRedNoise,
           EFAC/EQUAD) with 5 WaveX harmonics of 1 / T_span from the reference's wavex_setup and
           4 DMWaveX harmonics from dmwavex_setup (no DMWXEPOCH line: PEPOCH fills it in), every
           amplitude free and non-zero; 1000 TOAs; also dmwavex_dm and the same extra arrays.
* wx_fit_spread.json : gen_fit_spread.measure of the two plus the Downhill spread, in
           gl_fit_spread.json's schema.
* "setup" in wx_wls.json: indices and frequencies of the reference's wavex_setup / dmwavex_setup
           (n_freqs=3; an explicit list; both given).

The builders assert the conditions the tests rely on (see check()).

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_wavex.py [wx_wls wx_gls spread]
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
from pint.utils import wavex_setup, dmwavex_setup  # noqa: E402

from gen_solar_wind import with_save, write_par, downhill_spread  # noqa: E402


def wls_par(wxsin_1="1.5e-6", wxcos_1="-0.8e-6", wxsin_2="2.1e-6", wxsin_4="-1.2e-6", wxcos_4="0.9e-6",
            glf0_1="3e-9", freq_flag=""):
    return f"""PSR J1012-WX
RAJ 10:12:33.4372 1
DECJ 53:07:02.512 1
F0 218.8118404 1
F1 -4.08e-16 1
PEPOCH 55000
POSEPOCH 55000
DM 9.0233 1
WXEPOCH 55050.5
WXFREQ_0002 -0.0018181818181818182
WXSIN_0002 {wxsin_2} 1
WXCOS_0002 1.7e-6
WXFREQ_0001 0.00090909090909090909{freq_flag}
WXSIN_0001 {wxsin_1} 1
WXCOS_0001 {wxcos_1} 1
WXFREQ_0004 0.00417
WXSIN_0004 {wxsin_4} 1
WXCOS_0004 {wxcos_4} 1
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
WX_TRUE = [(1.1e-6, -0.7e-6), (0.6e-6, 0.9e-6), (-0.5e-6, 0.4e-6), (0.3e-6, -0.35e-6), (0.25e-6, 0.2e-6)]
DMWX_TRUE = [(1.0e-4, -1.4e-4), (0.8e-4, 0.6e-4), (-0.7e-4, 0.5e-4), (0.4e-4, -0.6e-4)]


def gls_par(scale=1.0):
    """pta_par(22, "ELL1") plus the lines of the reference's own wavex_setup / dmwavex_setup."""
    m = get_model(io.StringIO(pta_par(22, "ELL1")))
    iw = wavex_setup(m, T_GLS, n_freqs=len(WX_TRUE))
    idm = dmwavex_setup(m, T_GLS, n_freqs=len(DMWX_TRUE))
    lines = "WXEPOCH 54900\n"
    for i, (s, c) in zip(iw, WX_TRUE):
        lines += (f"WXFREQ_{i:04d} {getattr(m, f'WXFREQ_{i:04d}').value!r}\n"
                  f"WXSIN_{i:04d} {s * scale!r} 1\nWXCOS_{i:04d} {c * scale!r} 1\n")
    for i, (s, c) in zip(idm, DMWX_TRUE):
        lines += (f"DMWXFREQ_{i:04d} {getattr(m, f'DMWXFREQ_{i:04d}').value!r}\n"
                  f"DMWXSIN_{i:04d} {s * scale!r} 1\nDMWXCOS_{i:04d} {c * scale!r} 1\n")
    return pta_par(22, "ELL1") + lines


def extra_arrays(model, ts):
    """The absolute phase (abs_phase=False: no TZR subtraction) of the TOAs and of the TZR TOA,
    wavex_delay / dmwavex_delay / dmwavex_dm of both."""
    out = {}
    tz = model.get_TZR_toa(ts)
    for key, t in (("abs", ts), ("tzr_abs", tz)):
        ph = model.phase(t, abs_phase=False)
        out[key + "_phase_int"] = np.asarray(ph.int.value, dtype=np.float64)
        out[key + "_phase_frac_hi"], out[key + "_phase_frac_lo"] = split_ld(ph.frac.value)
    for key, t in (("", ts), ("tzr_", tz)):
        parts = refcommon.component_delays(model, t)
        for n in ("wavex_delay", "dmwavex_delay"):
            if "delay_" + n in parts:
                out[key + n] = parts["delay_" + n]
        if "DMWaveX" in model.components:
            out[key + "dmwavex_dm"] = np.asarray(model.components["DMWaveX"].dmwavex_dm(t).value, dtype=np.float64)
    return out


def check(model, ts, more):
    """The conditions the tests rely on; returns max |a'| over both components."""
    M, names, _ = model.designmatrix(ts)
    names = list(names)
    for n in names:
        if n.startswith(("WXSIN_", "WXCOS_", "DMWXSIN_", "DMWXCOS_")):
            assert np.max(np.abs(M[:, names.index(n)])) > 0, n
    assert np.max(np.abs(more["wavex_delay"])) > 100e-9
    if "dmwavex_delay" in more:
        assert np.max(np.abs(more["dmwavex_delay"])) > 100e-9
    tdb = ts.table["tdbld"]
    amax, dsin = 0.0, 0.0
    # (the delay accumulated before wavex_delay, as TimingModel.delay forms it)
    acc = np.zeros(ts.ntoas) * u.s
    for dc in model.DelayComponent_list:
        if type(dc).__name__ == "WaveX":
            break
        for df in dc.delay_funcs_component:
            acc += df(ts, acc)
    D = acc.to_value(u.d)
    for pre, ep in (("WXFREQ_", "WXEPOCH"), ("DMWXFREQ_", "DMWXEPOCH")):
        for n in model.params:
            if n.startswith(pre):
                f = getattr(model, n).value
                ap = np.asarray(2.0 * np.pi * f * (tdb - getattr(model, ep).value), dtype=np.float64)
                amax = max(amax, float(np.max(np.abs(ap))))
                if pre == "WXFREQ_":
                    a = np.asarray(2.0 * np.pi * f * (tdb - getattr(model, ep).value - D), dtype=np.float64)
                    dsin = max(dsin, float(np.max(np.abs(np.sin(a) - np.sin(ap)))))
    s = M / np.sqrt(np.sum(M * M, axis=0))
    cond = float(np.linalg.cond(s.T @ s))
    print(f"  {len(names)} columns, normalised Gram condition number {cond:.3g}; max|a'| {amax:.4g}; "
          f"max |sin a - sin a'| {dsin:.3g}; wavex delay up to {np.max(np.abs(more['wavex_delay'])):.3g} s",
          file=sys.stderr)
    assert cond < 1e12, cond
    return {"wx_max_arg": amax, "wx_max_dsin": dsin, "wx_gram_cond": cond}


def setup_records():
    """Indices and frequencies of the reference's wavex_setup / dmwavex_setup."""
    rec = {}
    for name, fn, pre in (("wavex", wavex_setup, "WXFREQ_"), ("dmwavex", dmwavex_setup, "DMWXFREQ_")):
        for case, kw in (("n3", dict(n_freqs=3)), ("list", dict(freqs=[0.004, 0.001, 0.0025])),
                         ("list1", dict(freqs=[0.0025])), ("frozen", dict(n_freqs=2, freeze_params=True))):
            m = get_model(io.StringIO(wls_par().split("WXEPOCH")[0] + "EPHEM builtin\nUNITS TDB\n"))
            try:
                idx = [int(i) for i in fn(m, 1000.0, **kw)]
            except Exception as e:  # (recorded: the tests reproduce what the reference does)
                rec[f"{name}_{case}"] = {"error": type(e).__name__}
                continue
            rec[f"{name}_{case}"] = {
                "indices": idx, "freqs": [float(getattr(m, f"{pre}{i:04d}").value) for i in idx],
                "frozen": [bool(getattr(m, n).frozen) for n in m.params if n.startswith(pre.replace("FREQ", "SIN"))],
                "params": [n for n in m.params if "WX" in n], "free_params": list(m.free_params),
                "components": list(m.components.keys())}
        m = get_model(io.StringIO(wls_par().split("WXEPOCH")[0] + "EPHEM builtin\nUNITS TDB\n"))
        try:
            fn(m, 1000.0, freqs=[0.001], n_freqs=1)
        except Exception as e:
            rec[f"{name}_both"] = type(e).__name__
    return rec


def build_wls():
    np.random.seed(51)
    true = get_model(io.StringIO(wls_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 400, true, freq=np.tile([1400.0, 2300.0], 200) * u.MHz,
                                    obs="geocenter", error=1 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = wls_par(wxsin_1="1.3e-6", wxcos_1="-0.9e-6", wxsin_2="2.3e-6", wxsin_4="-1.0e-6", wxcos_4="1.0e-6",
                  glf0_1="3.002e-9")
    return par, get_model(io.StringIO(par)), ts


def build_gls():
    np.random.seed(22)
    true = get_model(io.StringIO(gls_par()))
    ts = sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False)
    par = gls_par(scale=0.9)
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def freq_fit_behaviour(ts):
    """What the reference does with a WXFREQ_ line whose fit flag is 1."""
    par = wls_par(freq_flag=" 1")
    out = {"par_line": "WXFREQ_0001 0.00090909090909090909 1"}
    try:
        m = get_model(io.StringIO(par))
        out["frozen"] = bool(m.WXFREQ_0001.frozen)
        out["in_free_params"] = "WXFREQ_0001" in m.free_params
        m.designmatrix(ts)
        out["designmatrix"] = "ok"
    except Exception as e:
        out["designmatrix"] = type(e).__name__
        out["message"] = str(e)
    return out


def gen_wls():
    par, model, ts = build_wls()
    write_par("wx_wls", par)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    errs = [getattr(f.model, p).uncertainty_value for p in f.model.free_params]
    assert np.all(np.isfinite(errs)), errs
    print(f"  WLS chi2 {float(chi2):.3f}; WXSIN_0001 {f.model.WXSIN_0001.value:.4g} +- "
          f"{f.model.WXSIN_0001.uncertainty_value:.3g} s", file=sys.stderr)
    g0 = np.longdouble(f.model.WXSIN_0001.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.WXSIN_0001.uncertainty_value)
    g1 = np.longdouble(f.model.F1.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.F1.uncertainty_value)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    more["grid_WXSIN_0001_hi"], more["grid_WXSIN_0001_lo"] = split_ld(g0)
    more["grid_F1_hi"], more["grid_F1_lo"] = split_ld(g1)
    fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
    c2, _ = grid_chisq(fg, ("WXSIN_0001", "F1"), (g0 * u.s, g1 * u.Hz / u.s), ncpu=1, printprogress=False)
    more["grid_chi2"] = np.asarray(c2, dtype=np.float64)
    print(f"  grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
    # (the parameter lines only: the header names the run that wrote it)
    meta["wls_parfile"] = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    meta["setup"] = setup_records()
    meta["freq_fit"] = freq_fit_behaviour(ts)
    meta["delay_funcs"] = [df.__name__ for df in model.delay_funcs]
    with_save(gen_synth, "wx_wls", more, meta)
    capture("wx_wls", model, ts, fit="wls")


def gen_gls():
    par, model, ts = build_gls()
    write_par("wx_gls", par)
    more = extra_arrays(model, ts)
    meta = check(model, ts, more)
    assert meta["wx_max_dsin"] > 1e-6, meta
    f = pfit.GLSFitter(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=1)
    errs = [getattr(f.model, p).uncertainty_value for p in f.model.free_params]
    assert np.all(np.isfinite(errs)), errs
    meta["gls_parfile"] = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    meta["delay_funcs"] = [df.__name__ for df in model.delay_funcs]
    with_save(gen_synth, "wx_gls", more, meta)
    capture("wx_gls", model, ts, fit="gls")


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "wx_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    todo = {"wx_wls": (build_wls, "wls", pfit.DownhillWLSFitter), "wx_gls": (build_gls, "gls", pfit.DownhillGLSFitter)}
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
    which = sys.argv[1:] or ["wx_wls", "wx_gls", "spread"]
    if "wx_wls" in which:
        gen_wls()
    if "wx_gls" in which:
        gen_gls()
    if "spread" in which:
        gen_spread([n for n in ("wx_wls", "wx_gls") if n in which] or ["wx_wls", "wx_gls"])
