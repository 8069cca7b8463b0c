"""Golden fixtures for SolarWindDispersion, SWM 0 (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

* sw_ecl : WLS.  A J2145-0750-like pulsar 5.3 deg off the ecliptic (ecliptic astrometry with
           proper motion and parallax, ELL1, DM + DM1, NE_SW free), 400 TOAs at 430 / 820 /
           1400 / 2300 MHz from the geocentre, simulated at NE_SW 7.9, DM 9.0025 and captured
           from NE_SW 6.0, DM 9.0026.  Beside what gen_synth.capture(fit="wls") records: a
           5x5 grid_chisq over (NE_SW, DM), +-3 sigma of the one-step fit (serial and
           parallel, as gen_ngc6440e does for (F0, F1)), and the post-fit model's as_parfile().
* sw_pta : GLS.  gen_synth.pta_par(21, "DD") (the bench's per-pulsar shape) moved to
           J2145-0750's position, NE_SW 6.0 free; 1000 TOAs; captured from NE_SW 4.0.
* sw_wb  : wideband.  gen_wideband.build()'s construction with the same position and NE_SW
           lines; 600 TOAs; captured from NE_SW 4.0 with gen_wideband.main()'s keys.
* sw_fit_spread.json : gen_fit_spread.measure(model, toas, fit, down=True) of the three, in
           fit_spread.json's schema, plus under "downhill" the per-parameter Downhill spread by
           gen_downhill_spread.spread's loop (5 ps residual shifts, 8 seeds).

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_solar_wind.py [sw_ecl sw_pta sw_wb spread]
"""
import copy
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle", "refgen"))

import astropy.units as u  # noqa: E402
import refcommon  # noqa: E402
from refcommon import GOLDEN, register_clockless_sites, designmatrix_outputs, split_ld  # noqa: E402
import gen_synth  # noqa: E402
from gen_synth import pta_par, capture  # noqa: E402  (the real capture: gen_fit_spread replaces the module's)
import gen_wideband  # noqa: E402
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
import pint.residuals as pres  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.gridutils import grid_chisq  # noqa: E402

POSITION = {"RAJ": "RAJ 21:45:50.46 1", "DECJ": "DECJ -07:50:18.5 1"}


def ecl_par(ne_sw, dm):
    return f"""PSR J2145-SW
ELONG 326.0245814536 1
ELAT 5.3130530398 1
PMELONG -12.05 1
PMELAT -4.1 1
PX 1.6 1
ECL IERS2010
POSEPOCH 55000
F0 62.2958887614696 1
F1 -1.1538e-16 1
PEPOCH 55000
DM {dm} 1
DM1 1e-4 1
DMEPOCH 55000
NE_SW {ne_sw} 1
SWM 0
BINARY ELL1
PB 6.8389 1
A1 10.1641 1
TASC 55000.1234567 1
EPS1 -6.8e-6 1
EPS2 -1.6e-5 1
EPHEM builtin
CLK TT(TAI)
UNITS TDB
TZRMJD 55000.1234
TZRFRQ 1400
TZRSITE geocenter
"""


def pta_sw_par(ne_sw, extra=""):
    lines = [POSITION.get(l.split()[0], l) for l in pta_par(21, "DD").splitlines()]
    return "\n".join(lines) + "\n" + extra + f"NE_SW {ne_sw} 1\nSWM 0\n"


def sun_stats(model, toas):
    ang = model.sun_angle(toas).to_value(u.deg)
    d = model.solar_wind_delay(toas).to_value(u.us)
    print(f"  min elongation {ang.min():.2f} deg, {int(np.sum(ang < 15))} TOAs within 15 deg, "
          f"solar-wind delay {np.abs(d).min():.3g} .. {np.abs(d).max():.3g} us", file=sys.stderr)


def with_save(module, name, more_arrays, more_meta):
    """Route module.save(...) to refcommon.save(name, ...) with extra arrays / meta entries."""
    def save(_, arrays, meta):
        arrays = dict(arrays)
        arrays.update(more_arrays)
        meta = dict(meta)
        meta.update(more_meta)
        meta["name"] = name
        refcommon.save(name, arrays, meta)
    module.save = save


def build_ecl():
    np.random.seed(31)
    true = get_model(io.StringIO(ecl_par(7.9, 9.0025)))
    ts = sim.make_fake_toas_uniform(54500, 55600, 400, true, freq=np.tile([430.0, 820.0, 1400.0, 2300.0], 100) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    par = ecl_par(6.0, 9.0026)
    return par, get_model(io.StringIO(par)), ts


def build_pta():
    np.random.seed(21)
    true = get_model(io.StringIO(pta_sw_par(6.0)))
    ts = sim.make_fake_toas_uniform(53000, 56652, 1000, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False)
    par = pta_sw_par(4.0)
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def build_wb():
    np.random.seed(21)
    true = get_model(io.StringIO(pta_sw_par(6.0, gen_wideband.EXTRA)))
    ts = sim.make_fake_toas_uniform(53000, 56652, 600, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, add_correlated_noise=True,
                                    include_bipm=False, multi_freqs_in_epoch=False, wideband=True,
                                    wideband_dm_error=2e-4 * u.pc / u.cm ** 3)
    par = pta_sw_par(4.0, gen_wideband.EXTRA)
    model = get_model(io.StringIO(par))
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def write_par(name, par):
    with open(os.path.join(GOLDEN, name + ".par"), "w") as f:
        f.write(par)


def gen_ecl():
    par, model, ts = build_ecl()
    sun_stats(model, ts)
    write_par("sw_ecl", par)
    f = pfit.WLSFitter(ts, copy.deepcopy(model))
    f.fit_toas(maxiter=1)
    print(f"  WLS NE_SW {f.model.NE_SW.value:.4f} +- {f.model.NE_SW.uncertainty_value:.4f}", file=sys.stderr)
    g0 = np.longdouble(f.model.NE_SW.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.NE_SW.uncertainty_value)
    g1 = np.longdouble(f.model.DM.value) + np.linspace(-3, 3, 5) * np.longdouble(f.model.DM.uncertainty_value)
    more = {}
    more["grid_NE_SW_hi"], more["grid_NE_SW_lo"] = split_ld(g0)
    more["grid_DM_hi"], more["grid_DM_lo"] = split_ld(g1)
    axes = (g0 * u.cm ** -3, g1 * u.pc / u.cm ** 3)
    for key, ncpu in (("grid_chi2_serial", 1), ("grid_chi2_parallel", 2)):
        fg = pfit.WLSFitter(ts, copy.deepcopy(f.model))
        chi2, _ = grid_chisq(fg, ("NE_SW", "DM"), axes, ncpu=ncpu, printprogress=False)
        more[key] = np.asarray(chi2, dtype=np.float64)
    # (the parameter lines only: the header names the run that wrote it)
    text = "".join(l + "\n" for l in f.model.as_parfile().splitlines() if not l.startswith("#"))
    with_save(gen_synth, "sw_ecl", more, {"wls_parfile": text})
    capture("sw_ecl", model, ts, fit="wls")


def gen_pta():
    par, model, ts = build_pta()
    sun_stats(model, ts)
    write_par("sw_pta", par)
    with_save(gen_synth, "sw_pta", {}, {})
    capture("sw_pta", model, ts, fit="gls")


def gen_wb():
    par, model, ts = build_wb()
    sun_stats(model, ts)
    write_par("sw_wb", par)
    _, dmm = designmatrix_outputs(model, ts)
    more = {"psr_dir_icrs": np.asarray(model.ssb_to_psb_xyz_ICRS(epoch=ts.table["tdbld"].astype(np.float64)),
                                       dtype=np.float64)}
    with_save(gen_wideband, "sw_wb", more, dmm)
    gen_wideband.build = lambda: (par, model, ts)
    with tempfile.TemporaryDirectory() as tmp:  # (main() writes its par text as wb_dd.par)
        gen_wideband.GOLDEN = tmp
        gen_wideband.main()


def downhill_spread(model, toas, cls):
    """gen_downhill_spread.spread's loop on (model, toas)."""
    import gen_downhill_spread as gds
    v0, e0, s0, c0 = gds.fit(model, toas, cls)
    worst = {p: 0.0 for p in v0}
    statuses, chi2s = [], []
    orig = pres.Residuals.calc_time_resids
    try:
        for rep in range(1, gds.NREP + 1):
            delta = np.random.default_rng(rep).normal(size=len(toas)) * gds.SIGMA_S

            def calc(self, *a, **k):
                return orig(self, *a, **k) + delta * u.s

            pres.Residuals.calc_time_resids = calc
            v, e, s, c = gds.fit(model, toas, cls)
            statuses.append(s)
            chi2s.append(c / c0 - 1)
            for p in v0:
                worst[p] = max(worst[p], abs(float((v[p] - v0[p]) / np.longdouble(e0[p]))))
    finally:
        pres.Residuals.calc_time_resids = orig
    return {"sigma_s": gds.SIGMA_S, "nrep": gds.NREP, "status": s0, "statuses": statuses,
            "chi2_rel": [float(x) for x in chi2s], "max_dev_sigma": worst}


def gen_spread(names):
    import gen_fit_spread
    path = os.path.join(GOLDEN, "sw_fit_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    todo = {"sw_ecl": (build_ecl, "wls", pfit.DownhillWLSFitter), "sw_pta": (build_pta, "gls", pfit.DownhillGLSFitter),
            "sw_wb": (build_wb, "wb", pfit.WidebandDownhillFitter)}
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
    which = sys.argv[1:] or ["sw_ecl", "sw_pta", "sw_wb", "spread"]
    if "sw_ecl" in which:
        gen_ecl()
    if "sw_pta" in which:
        gen_pta()
    if "sw_wb" in which:
        gen_wb()
    if "spread" in which:
        gen_spread([n for n in ("sw_ecl", "sw_pta", "sw_wb") if n in which] or ["sw_ecl", "sw_pta", "sw_wb"])
