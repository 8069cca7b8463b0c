"""Golden fixtures for the PiecewiseSpindown, Wave and IFunc components (reference run; container
only; TEST INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* pw_wls  : WLS.  A Vela-like isolated pulsar (F0 11.19 Hz, F1, equatorial astrometry, DM, one
            glitch) with three pieces: piece 1 with PWPH / PWF0 / PWF1 free; piece 2 with PWF0 /
            PWF2 free, whose window overlaps piece 1's by 100 d; piece 3 frozen and non-zero, with
            TZRMJD inside it.  No PWEP at its window's centre.  300 TOAs at 1400 / 2300 MHz from
            the geocentre over MJD 54500-55600, 20 us errors.  Captured from a start perturbed in
            (PWPH_1, PWF0_1, PWF0_2, GLF0_1).  Beside what gen_synth.capture(fit="wls") records:
            the absolute phase of the TOAs and of the TZR TOA, each component's own phase of both,
            the post-fit as_parfile(), a 5x5 grid_chisq over (PWF0_1, F0), and under "forms" what
            the reference does with the malformed models the host has to mirror.
* wave_wls: WLS.  The same kind of pulsar with five WAVE terms (WAVEEPOCH != PEPOCH) and SIFUNC 2
            with six unevenly spaced IFUNC points; F0, F1 and the astrometry free.  Also the same
            model's IFunc phase with SIFUNC 0, and the reference's translate_wave_to_wavex /
            translate_wavex_to_wave results (parameters and values).
* pw_gls  : GLS.  gen_synth.pta_par(22, "ELL1") (the bench's per-pulsar shape) with two pieces,
            PWF0 / PWF1 free; 1000 TOAs.
* pw_fit_spread.json : gen_fit_spread.measure of the three plus the Downhill spread, in
            gl_fit_spread.json's schema.

The two WLS models carry no proper motion.  With Vela's (-49.68, 29.9 mas / yr) the reference's
own chi2 is not one number: the pulsar direction it takes through erfa's pmsafe moves by ~2e-11
rad (9 ns, an annual term growing away from POSEPOCH) between evaluations whose parameters
differ by 1e-8 sigma, so successive WLSFitter iterations at the converged point give chi2
274.70701 and 274.70509 in turn, and the serial and the executor path of grid_chisq differ by
2.7e-5 of chi2 on a 5x5 grid.  Without it successive iterations agree to 1e-8 of chi2.

piecewise and ifunc are not categories of the reference's DEFAULT_ORDER, so the place of those
components among the phase components changes with the interpreter's hash seed, as does the order
of the component types.  The host model always has Spindown, Wave, Glitch, PiecewiseSpindown,
IFunc with the phase components first; check_order() asserts a run that has the same (seed 34).

Usage: PYTHONHASHSEED=34 oracle/refenv/run_ref.sh scripts/refgen/gen_phase_terms.py [pw_wls wave_wls pw_gls spread]
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
from pint.utils import translate_wave_to_wavex, translate_wavex_to_wave  # noqa: E402

from gen_solar_wind import with_save, write_par, downhill_spread  # noqa: E402

CANONICAL = ["AbsPhase", "Spindown", "Wave", "Glitch", "PiecewiseSpindown", "IFunc"]
COMPONENT_PHASE = {"PiecewiseSpindown": "piecewise_phase", "Wave": "wave_phase", "IFunc": "ifunc_phase",
                   "Glitch": "glitch_phase"}

HEAD = """PSR J0835-PW
RAJ 08:35:20.61149 1
DECJ -45:10:34.8751 1
F0 11.18965 1
F1 -1.5567e-11 1
PEPOCH 55000
DM 67.99
GLEP_1 54900.25
GLF0_1 {glf0} 1
GLF1_1 -1.2e-13
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55100.1234
TZRFRQ 1400
TZRSITE geocenter
"""


def pw_par(pwph_1="0.1", pwf0_1="2e-4", pwf0_2="1.5e-4", glf0="2.3e-5"):
    return HEAD.format(glf0=glf0) + f"""PWSTART_1 54550.3
PWSTOP_1 54850.7
PWEP_1 54600.25
PWPH_1 {pwph_1} 1
PWF0_1 {pwf0_1} 1
PWF1_1 -3e-13 1
PWF2_1 0
PWSTART_2 54750.4
PWSTOP_2 55000.6
PWEP_2 54800.5
PWPH_2 0.25
PWF0_2 {pwf0_2} 1
PWF1_2 0
PWF2_2 1e-20 1
PWSTART_3 55050.2
PWSTOP_3 55300.8
PWEP_3 55100.0
PWPH_3 0.3
PWF0_3 1e-5
PWF1_3 -2e-14
PWF2_3 1e-22
"""


WAVE_LINES = """WAVEEPOCH 54900
WAVE_OM 0.0057119866
WAVE1 0.1 -0.05
WAVE2 -0.02 0.03
WAVE3 0.008 0.004 7
WAVE4 -0.003 0.001
WAVE5 0.0007 -0.0012
"""
IFUNC_LINES = """SIFUNC {sifunc} 0
IFUNC1 54600.0 0.0012 0
IFUNC2 54700.5 -0.0021 0
IFUNC3 54850.25 0.0034 0
IFUNC4 55100.0 -0.0008 0
IFUNC5 55350.75 0.0026 0
IFUNC6 55500.0 -0.0015 0
"""


def wave_par(f0="11.18965", glf0="2.3e-5", sifunc=2):
    return HEAD.format(glf0=glf0).replace("F0 11.18965 1", f"F0 {f0} 1") + WAVE_LINES + IFUNC_LINES.format(sifunc=sifunc)


GLS_PW = """PWSTART_1 53500.3
PWSTOP_1 54400.7
PWEP_1 53700.1
PWPH_1 0.2
PWF0_1 {pwf0_1} 1
PWF1_1 1e-15 1
PWF2_1 0
PWSTART_2 55200.4
PWSTOP_2 56000.6
PWEP_2 55600.2
PWPH_2 -0.1
PWF0_2 -2e-7 1
PWF1_2 {pwf1_2} 1
PWF2_2 0
"""


def gls_par(pwf0_1="1e-6", pwf1_2="-3e-15"):
    return pta_par(22, "ELL1") + GLS_PW.format(pwf0_1=pwf0_1, pwf1_2=pwf1_2)


def export_model(model):
    """refcommon.export_model for a model with pair parameters (WAVEn, IFUNCn), whose two values
    the committed exporter cannot record: it sees them unset, and their record is filled in
    here as [[hi, lo], [hi, lo]]."""
    from pint.models.parameter import pairParameter
    pairs = {}
    for n in model.params:
        par = getattr(model, n)
        comp = getattr(par, "param_comp", par)
        if isinstance(comp, pairParameter) and comp._quantity is not None:
            pairs[n] = (comp, comp._quantity)
    for comp, _ in pairs.values():
        comp._quantity = None
    try:
        rec = refcommon.export_model(model)
    finally:
        for comp, q in pairs.values():
            comp._quantity = q
    for n in pairs:
        rec["values"][n]["value"] = [list(map(float, split_ld(np.longdouble(x)))) for x in getattr(model, n).value]
    return rec


gen_synth.export_model = export_model


def check_order(model):
    order = [type(c).__name__ for c in model.PhaseComponent_list if type(c).__name__ in CANONICAL]
    assert order == [c for c in CANONICAL if c in order], (order, "run with another PYTHONHASHSEED (34)")
    assert list(model.components.keys())[0] == "AbsPhase", "run with another PYTHONHASHSEED (34)"


def check_edges(model, ts, more_models=()):
    """No TOA nor the TZR TOA within 1 ms of a PWSTART / PWSTOP (on tdbld) nor of an IFUNC point (on
    ts = tdbld - delay); >= 20 TOAs outside every piece, before the first IFUNC point and after the
    last."""
    delay = model.delay(ts).to_value(u.s)
    tz = model.get_TZR_toa(ts)
    tzd = model.delay(tz).to_value(u.s)
    t, t_tz = ts.table["tdbld"], tz.table["tdbld"][0]
    inside = np.zeros(len(t), dtype=bool)
    for n in model.params:
        if n.startswith(("PWSTART_", "PWSTOP_")):
            e = np.longdouble(getattr(model, n).value)
            near = float(np.min(np.abs((t - e) * 86400)))
            assert near > 1e-3 and abs(float((t_tz - e) * 86400)) > 1e-3, (n, near)
        if n.startswith("PWSTART_"):
            i = n.split("_")[1]
            a, b = getattr(model, n).value, getattr(model, "PWSTOP_" + i).value
            inside |= np.asarray((t >= a) & (t < b))
            print(f"  piece {i}: {int(np.sum((t >= a) & (t < b)))} TOAs", file=sys.stderr)
    if "PiecewiseSpindown" in model.components:
        assert np.sum(~inside) >= 20, np.sum(~inside)
        print(f"  {int(np.sum(~inside))} TOAs outside every piece", file=sys.stderr)
    if "IFunc" in model.components:
        x = np.array([getattr(model, f"IFUNC{i}").value[0] for i in range(1, model.components["IFunc"].num_terms + 1)],
                     dtype=np.longdouble)
        tb = t - delay / 86400
        tbz = t_tz - tzd[0] / 86400
        for e in x:
            assert float(np.min(np.abs((tb - e) * 86400))) > 1e-3 and abs(float((tbz - e) * 86400)) > 1e-3, e
        assert np.sum(tb < x[0]) >= 20 and np.sum(tb > x[-1]) >= 20
        print(f"  IFunc: {int(np.sum(tb < x[0]))} TOAs before the first point, {int(np.sum(tb > x[-1]))} after the last, "
              f"{int(np.sum((tb >= x[0]) & (tb < x[1])))} in [x0, x1)", file=sys.stderr)


def phase_arrays(model, ts):
    """The absolute phase (abs_phase=False: no TZR subtraction) of the TOAs and of the TZR TOA, and
    each phase component's own phase of both, as (hi, lo)."""
    out = {}
    tz = model.get_TZR_toa(ts)
    for key, t in (("abs", ts), ("tzr_abs", tz)):
        ph = model.phase(t, abs_phase=False)
        out[key + "_phase_int"] = np.asarray(ph.int.value, dtype=np.float64)
        out[key + "_phase_frac_hi"], out[key + "_phase_frac_lo"] = split_ld(ph.frac.value)
    for comp, fn in COMPONENT_PHASE.items():
        if comp not in model.components:
            continue
        for key, t in ((fn, ts), ("tzr_" + fn, tz)):
            g = np.asarray(getattr(model.components[comp], fn)(t, model.delay(t)).value, dtype=np.longdouble)
            out[key + "_hi"], out[key + "_lo"] = split_ld(g)
        print(f"  {comp}: phase up to {float(np.max(np.abs(out[fn + '_hi']))):.6g} cycles, TZR "
              f"{float(out['tzr_' + fn + '_hi'][0]):.6g}", file=sys.stderr)
    return out


def forms():
    """What the reference does with the models the host has to refuse the same way: the stage
    (get_model, designmatrix or phase), the exception class and its text."""
    np.random.seed(3)
    base = get_model(io.StringIO(pw_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 30, base, freq=1400 * u.MHz, obs="geocenter", error=20 * u.us,
                                    include_bipm=False)
    pw, wv = pw_par(), wave_par()
    cases = {
        "free_PWEP_1": pw.replace("PWEP_1 54600.25", "PWEP_1 54600.25 1"),
        "free_PWSTART_1": pw.replace("PWSTART_1 54550.3", "PWSTART_1 54550.3 1"),
        "free_WAVE_OM": wv.replace("WAVE_OM 0.0057119866", "WAVE_OM 0.0057119866 1"),
        "piece_without_PWPH": pw.replace("PWPH_2 0.25\n", ""),
        "piece_without_PWEP": pw.replace("PWEP_2 54800.5\n", ""),
        "piece_without_PWSTART": pw.replace("PWSTART_3 55050.2\n", ""),
        "piece_without_PWSTOP": pw.replace("PWSTOP_3 55300.8\n", ""),
        "wave_gap": wv.replace("WAVE3 ", "WAVE7 "),
        "ifunc_gap": wv.replace("IFUNC4 ", "IFUNC9 "),
        "no_SIFUNC": wv.replace("SIFUNC 2 0\n", ""),
        "SIFUNC_1": wv.replace("SIFUNC 2 0", "SIFUNC 1 0"),
    }
    out = {}
    for name, par in cases.items():
        rec = {"par": par, "stage": None, "error": None, "message": None}
        stage = "get_model"
        try:
            m = get_model(io.StringIO(par))
            stage = "phase"
            m.phase(ts, abs_phase=False)
            stage = "designmatrix"
            m.designmatrix(ts)
        except Exception as e:  # noqa: BLE001 (the record is the exception)
            rec.update(stage=stage, error=type(e).__name__, message=str(e),
                       bases=[c.__name__ for c in type(e).__mro__[1:-1]])
        out[name] = rec
        print(f"  forms {name}: {rec['stage']} {rec['error']}: {(rec['message'] or '')[:100]!r}", file=sys.stderr)
    return out


def build_wls():
    np.random.seed(71)
    true = get_model(io.StringIO(pw_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 300, true, freq=np.tile([1400.0, 2300.0], 150) * u.MHz,
                                    obs="geocenter", error=20 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = pw_par(pwph_1="0.102", pwf0_1="2.0000005e-4", pwf0_2="1.500004e-4", glf0="2.30002e-5")
    return par, get_model(io.StringIO(par)), ts


def build_wave():
    np.random.seed(72)
    true = get_model(io.StringIO(wave_par()))
    ts = sim.make_fake_toas_uniform(54500, 55600, 300, true, freq=np.tile([1400.0, 2300.0], 150) * u.MHz,
                                    obs="geocenter", error=20 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = wave_par(f0="11.1896500002", glf0="2.30002e-5")
    return par, get_model(io.StringIO(par)), ts


def build_gls():
    np.random.seed(24)
    true = get_model(io.StringIO(gls_par()))
    ts = sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False)
    par = gls_par(pwf0_1="1.00002e-6", pwf1_2="-3.0001e-15")
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def param_record(model, prefixes):
    out = {}
    for n in model.params:
        if n.startswith(prefixes):
            p = getattr(model, n)
            v = p.value
            if v is None:
                continue
            vals = [list(map(float, split_ld(np.longdouble(x)))) for x in (v if isinstance(v, (list, tuple)) else [v])]
            out[n] = {"value": vals, "frozen": bool(p.frozen)}
    return out


def gen_wls():
    par, model, ts = build_wls()
    check_order(model)
    write_par("pw_wls", par)
    check_edges(model, ts)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    chi2 = f.fit_toas(maxiter=1)
    print(f"  WLS chi2 {float(chi2):.3f}; PWF0_1 {f.model.PWF0_1.value} +- {f.model.PWF0_1.uncertainty_value:.3g}",
          file=sys.stderr)
    g0 = np.longdouble(f.model.PWF0_1.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.PWF0_1.uncertainty_value)
    g1 = np.longdouble(f.model.F0.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.F0.uncertainty_value)
    more = phase_arrays(model, ts)
    for i in (1, 2):  # each free piece's phase exceeds 1e3 cycles somewhere
        one = copy.deepcopy(model)
        for n in one.params:
            if n.startswith(("PWPH_", "PWF0_", "PWF1_", "PWF2_")) and not n.endswith(f"_{i}"):
                getattr(one, n).value = 0.0
        big =float(np.max(np.abs(one.components["PiecewiseSpindown"].piecewise_phase(ts, one.delay(ts)).value)))
        assert big > 1e3, (i, big)
        more[f"piece{i}_max_phase"] = np.array([big])
    more["grid_PWF0_1_hi"], more["grid_PWF0_1_lo"] = split_ld(g0)
    more["grid_F0_hi"], more["grid_F0_lo"] = split_ld(g1)
    # the grid on the reference's executor path (its default): every point fitted on a copy of the
    # base model, as the device's batch of independent points is.  Its single-process path
    # (ncpu=1) fits the points one after another on one fitter, each from the previous point's
    # fitted parameters: an order-dependent number where one step does not converge (recorded
    # beside it: here the two agree to 2e-8 of chi2)
    for key, ncpu in (("grid_chi2", 2), ("grid_chi2_serial", 1)):
        fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
        c2, _ = grid_chisq(fg, ("PWF0_1", "F0"), (g0 * u.Hz, g1 * u.Hz), ncpu=ncpu, printprogress=False)
        more[key] = np.asarray(c2, dtype=np.float64)
    print(f"  serial against executor grid: max rel {np.max(np.abs(more['grid_chi2_serial'] / more['grid_chi2'] - 1)):.3g}",
          file=sys.stderr)
    c2 = more["grid_chi2"]
    M, names, _ = model.designmatrix(ts)
    s = M / np.sqrt(np.sum(M * M, axis=0))
    print(f"  {len(names)} columns {list(names)}, scaled condition number {np.linalg.cond(s):.3g}; "
          f"grid chi2 {np.min(c2):.3f} .. {np.max(c2):.3f}", file=sys.stderr)
    # (the parameter lines only: the header names the run that wrote it)
    text = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    with_save(gen_synth, "pw_wls", more, {"wls_parfile": text, "forms": forms()})
    capture("pw_wls", model, ts, fit="wls")


def gen_wave():
    par, model, ts = build_wave()
    check_order(model)
    write_par("wave_wls", par)
    check_edges(model, ts)
    more = phase_arrays(model, ts)
    assert float(np.max(np.abs(more["wave_phase_hi"]))) > 1.0
    # the same model with SIFUNC 0: all three of the reference's cases (before x0, [x0, x1), from x1 on)
    m0 = get_model(io.StringIO(wave_par(f0="11.1896500002", glf0="2.30002e-5", sifunc=0)))
    tz = m0.get_TZR_toa(ts)
    x = [np.longdouble(getattr(m0, f"IFUNC{i}").value[0]) for i in (1, 2)]
    tb = ts.table["tdbld"] - m0.delay(ts).to_value(u.s) / 86400
    counts = [int(np.sum(tb < x[0])), int(np.sum((tb >= x[0]) & (tb < x[1]))), int(np.sum(tb >= x[1]))]
    assert min(counts) >= 10, counts
    for key, t in (("ifunc0_phase", ts), ("tzr_ifunc0_phase", tz)):
        g = np.asarray(m0.components["IFunc"].ifunc_phase(t, m0.delay(t)).value, dtype=np.longdouble)
        more[key + "_hi"], more[key + "_lo"] = split_ld(g)
    y = [float(getattr(m0, f"IFUNC{i}").value[1]) for i in range(1, 7)]
    t0 = np.asarray(more["ifunc0_phase_hi"], dtype=np.float64) / float(m0.F0.value)
    print(f"  SIFUNC 0: {counts} TOAs in the three cases; distinct offsets {sorted(set(np.round(t0, 9)))} of y {y}",
          file=sys.stderr)
    wx = translate_wave_to_wavex(model)
    back = translate_wavex_to_wave(wx)
    extra = {"wls_parfile": "".join(l + "\n" for l in model.as_parfile().splitlines() if not l.startswith("#")),
             "sifunc0_counts": counts,
             "wave_to_wavex": param_record(wx, ("WX",)), "wave_to_wavex_components": list(wx.components.keys()),
             "wavex_to_wave": param_record(back, ("WAVE",)), "wavex_to_wave_components": list(back.components.keys())}
    with_save(gen_synth, "wave_wls", more, extra)
    capture("wave_wls", model, ts, fit="wls")


def gen_gls():
    par, model, ts = build_gls()
    check_order(model)
    write_par("pw_gls", par)
    check_edges(model, ts)
    with_save(gen_synth, "pw_gls", phase_arrays(model, ts), {})
    capture("pw_gls", model, ts, fit="gls")


TODO = {"pw_wls": (build_wls, "wls", pfit.DownhillWLSFitter), "wave_wls": (build_wave, "wls", pfit.DownhillWLSFitter),
        "pw_gls": (build_gls, "gls", pfit.DownhillGLSFitter)}


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "pw_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for n in names:
        build, fit, cls = TODO[n]
        _, model, ts = build()
        gen_fit_spread.check_same(n, ts)
        res[n] = gen_fit_spread.measure(model, ts, fit, True)
        res[n]["downhill"] = downhill_spread(model, ts, cls)
        print(n, json.dumps(res[n]), file=sys.stderr, flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    register_clockless_sites()
    which = sys.argv[1:] or ["pw_wls", "wave_wls", "pw_gls", "spread"]
    if "pw_wls" in which:
        gen_wls()
    if "wave_wls" in which:
        gen_wave()
    if "pw_gls" in which:
        gen_gls()
    if "spread" in which:
        gen_spread([n for n in TODO if n in which] or list(TODO))
