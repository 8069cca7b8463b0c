"""Golden fixtures for BayesianTiming (reference run; container only; TEST INFRASTRUCTURE).
Reuses the committed generators under oracle/refgen as they are.

* bayes_nb    : narrowband, 300 TOAs.  gen_synth.pta_par(41, "ELL1") without its red noise, DMX and
                flag-keyed EFAC / EQUAD, with two EFACs and two EQUADs on MJD ranges instead: the
                ranges overlap (EFAC1 x EFAC2, EFAC x EQUAD1), EQUAD2's range holds exactly one TOA
                (a white-noise class of a single TOA), and the TOAs after the last range are under no
                mask.  Every timing parameter and the four noise parameters free.  No PhaseOffset.
* bayes_phoff : the same with PHOFF free (no implicit mean subtraction).
* bayes_wb    : wideband, 300 TOAs.  pta_par(42, "ELL1") (20 DMX bins, all free: the compact DMX
                layout) without its red noise, with DMJUMP, DMEFAC and DMEQUAD on MJD ranges
                (gen_wideband's lines) beside an EFAC and an EQUAD on overlapping MJD ranges; all of them free.

For each: the packed TOAs (refcommon.pack_toas) and TZR TOA, the mask table, the model, the
prior_info the BayesianTiming object was built with, 16 points drawn within +-3 sigma of the
reference's one-step WLS fit (noise parameters within +-30 %) as (hi, lo) pairs, and per point the
reference's lnlikelihood, lnprior, lnposterior, time residuals, chi2_toa, sum log sigma_toa, chi2_dm,
sum log sigma_dm (exactly the reference's expressions, bayesian.py:202-252: the DM errors through
.si.value), a fixed 16-point unit cube with its prior_transform, lnprior of points outside the
priors, and under "forms" the class and message of each refused construction.  No TOA's phase
residual comes within 0.05 cycle of a wrap at any point (asserted).

bayes_spread.json: per fixture and point, the reference's own |delta lnL| (and |delta chi2_toa|) when
its time residuals are shifted by gen_fit_spread.patterns at 5 ps and 30 ps rms -- the rule of
gen_fit_spread.measure -- and the reference's time per lnlikelihood call.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_bayesian.py [bayes_nb bayes_phoff bayes_wb]
"""
import copy
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle", "refgen"))

import astropy.units as u  # noqa: E402
import refcommon  # noqa: E402
from refcommon import (GOLDEN, register_clockless_sites, pack_toas, export_model, mask_table,  # noqa: E402
                       residual_outputs, split_ld)
from gen_synth import pta_par  # noqa: E402
import gen_fit_spread  # noqa: E402
import pint.simulation as sim  # noqa: E402
import pint.fitter as pfit  # noqa: E402
import pint.residuals as pres  # noqa: E402
from pint.bayesian import BayesianTiming  # noqa: E402
from pint.models import get_model  # noqa: E402

NPTS = 16
NOISE = ("EFAC", "EQUAD", "DMEFAC", "DMEQUAD")
DMU = u.pc / u.cm ** 3


def strip(par, prefixes):
    return "\n".join(l for l in par.splitlines() if not (l.split() and l.split()[0].startswith(prefixes))) + "\n"


def nb_par(mjds, phoff):
    """The narrowband par: mask ranges set from the simulated TOAs' MJDs (sorted)."""
    base = strip(pta_par(41, "ELL1"), ("TNRed", "DMX", "EFAC", "EQUAD"))
    def mid(k):  # a boundary half-way between TOA k-1 and TOA k
        return 0.5 * (mjds[k - 1] + mjds[k])
    e = [mid(1) - 1.0, mid(120), mid(80), mid(200), mid(40), mid(160), mid(230), mid(231)]
    par = base + (f"EFAC mjd {e[0]:.4f} {e[1]:.4f} 1.2 1\nEFAC mjd {e[2]:.4f} {e[3]:.4f} 0.9 1\n"
                  f"EQUAD mjd {e[4]:.4f} {e[5]:.4f} 0.3 1\nEQUAD mjd {e[6]:.4f} {e[7]:.4f} 0.5 1\n")
    if phoff:
        par += "PHOFF 0.0 1\n"
    return par


def build_nb(phoff=False):
    np.random.seed(41)
    true = get_model(io.StringIO(strip(pta_par(41, "ELL1"), ("TNRed", "DMX", "EFAC", "EQUAD"))))
    ts = sim.make_fake_toas_uniform(53000, 56652, 300, true, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False)
    mjds = np.sort(np.asarray(ts.get_mjds().value, dtype=np.float64))
    par = nb_par(mjds, phoff)
    return par, get_model(io.StringIO(par)), ts


WB_EXTRA = """EFAC mjd 53000 55500 1.1 1
EQUAD mjd 54500 56700 0.1 1
DMJUMP mjd 53000 54200 0.0012 1
DMEFAC mjd 54000 56700 1.3 1
DMEQUAD mjd 53000 55000 0.0002 1
"""


def build_wb():
    np.random.seed(42)
    par = strip(pta_par(42, "ELL1"), ("TNRed", "EFAC", "EQUAD")) + WB_EXTRA
    model = get_model(io.StringIO(par))
    ts = sim.make_fake_toas_uniform(53000, 56652, 300, model, freq=np.array([800, 1200, 1600, 2000]) * u.MHz,
                                    obs="geocenter", error=0.5 * u.us, add_noise=True, include_bipm=False,
                                    multi_freqs_in_epoch=False, wideband=True, wideband_dm_error=2e-4 * DMU)
    model.find_empty_masks(ts, freeze=True)
    return par, model, ts


def is_noise(p):
    return p.startswith(NOISE)


def fit_sigmas(model, ts, wb):
    """The one-step WLS fit of the timing parameters (noise parameters held): values (longdouble, par
    units) and uncertainties (par units) per free timing parameter."""
    m = copy.deepcopy(model)
    for p in m.free_params:
        if is_noise(p):
            getattr(m, p).frozen = True
    f = (pfit.WidebandTOAFitter if wb else pfit.WLSFitter)(ts, m)
    f.fit_toas(maxiter=2)
    out = {}
    for p in f.model.free_params:
        par = getattr(f.model, p)
        try:
            s = float(par.uncertainty.to_value(par.units))
        except Exception:  # noqa: BLE001
            s = float(par.uncertainty_value)
        out[p] = (np.longdouble(par.value), s)
    return out


def draw_points(model, fit, seed):
    rng = np.random.default_rng(seed)
    labels = list(model.free_params)
    pts = np.zeros((NPTS, len(labels)), dtype=np.longdouble)
    prior_info = {}
    for j, p in enumerate(labels):
        if is_noise(p):
            v = float(getattr(model, p).value)
            pts[:, j] = v * rng.uniform(0.7, 1.3, NPTS)
            prior_info[p] = {"distr": "uniform", "pmin": 0.1 * v, "pmax": 3.0 * v}
        else:
            v, s = fit[p]
            pts[:, j] = v + np.longdouble(s) * rng.uniform(-3, 3, NPTS).astype(np.longdouble)
            if p in ("F1", "PB"):
                prior_info[p] = {"distr": "normal", "mu": float(v), "sigma": 5.0 * s}
            else:
                prior_info[p] = {"distr": "uniform", "pmin": float(v) - 10.0 * s, "pmax": float(v) + 10.0 * s}
    return labels, pts, prior_info


def point_record(bt, ts, pt, wb):
    """The reference's terms at one point, by its own expressions (bayesian.py:202-252)."""
    lnl = float(bt.lnlikelihood(pt))
    if wb:
        res = pres.WidebandTOAResiduals(ts, bt.model, toa_resid_args={"track_mode": bt.track_mode})
        rt, rd = res.toa, res.dm
        chi2_dm = float(rd.calc_chi2())
        lsd = float(np.sum(np.log(bt.model.scaled_dm_uncertainty(ts).si.value)))
        lsd_pccm3 = float(np.sum(np.log(bt.model.scaled_dm_uncertainty(ts).to_value(DMU))))
        dmres = np.asarray(rd.resids.to_value(DMU), dtype=np.float64)
    else:
        rt = pres.Residuals(ts, bt.model, track_mode=bt.track_mode)
        chi2_dm, lsd, lsd_pccm3, dmres = 0.0, 0.0, 0.0, np.zeros(0)
    full = rt.calc_phase_resids(subtract_mean=False)
    full = np.asarray(getattr(full, "value", full), dtype=np.float64)
    assert np.max(np.abs(full)) < 0.45, ("a residual within 0.05 cycle of a wrap", float(np.max(np.abs(full))))
    return {"lnl": lnl, "chi2_toa": float(rt.calc_chi2()),
            "lsig_toa": float(np.sum(np.log(bt.model.scaled_toa_uncertainty(ts).si.value))),
            "chi2_dm": chi2_dm, "lsig_dm": lsd, "lsig_dm_pccm3": lsd_pccm3,
            "time": np.asarray(rt.time_resids.to_value(u.s), dtype=np.float64), "dm": dmres,
            "sig_toa": np.asarray(bt.model.scaled_toa_uncertainty(ts).to_value(u.s), dtype=np.float64),
            "wrap": float(np.max(np.abs(full)))}


def forms(model, ts, prior_info):
    """Class and message of each construction or call the reference refuses."""
    out = {}

    def rec(name, fn):
        try:
            fn()
            out[name] = {"error": None, "message": None}
        except Exception as e:  # noqa: BLE001 (the record is the exception)
            out[name] = {"error": type(e).__name__, "message": str(e)}
        print(f"  forms {name}: {out[name]['error']}: {(out[name]['message'] or '')[:90]!r}", file=sys.stderr)

    first = model.free_params[0]
    bad = copy.deepcopy(prior_info)
    bad[first] = {"distr": "lognormal", "mu": 0.0, "sigma": 1.0}
    rec("distr_lognormal", lambda: BayesianTiming(model, ts, prior_info=bad))
    less = {k: v for k, v in prior_info.items() if k != first}
    rec("unbounded_" + first, lambda: BayesianTiming(model, ts, prior_info=less))
    bt = BayesianTiming(model, ts, prior_info=prior_info)
    rec("wrong_length_lnprior", lambda: bt.lnprior(np.zeros(bt.nparams + 1)))
    rec("wrong_length_lnposterior", lambda: bt.lnposterior(np.zeros(bt.nparams - 1)))
    par = model.as_parfile()
    for name, extra in (("ecorr", "ECORR mjd 53000 56700 0.5\n"), ("plrednoise", "TNRedAmp -13.8\nTNRedGam 4.1\nTNRedC 10\n"),
                        ("pldmnoise", "TNDMAMP -13.2\nTNDMGAM 2.8\nTNDMC 10\n")):
        m = get_model(io.StringIO(par + extra))
        rec("correlated_" + name, lambda m=m: BayesianTiming(m, ts, prior_info=prior_info))

    def not_prior():
        copy.deepcopy(model).F0.prior = 3.0
    rec("prior_setter_float", not_prior)
    return out


def spread(bt, ts, pts, base):
    """|delta lnL| and |delta chi2_toa| per point under gen_fit_spread.patterns at each level."""
    orig = pres.Residuals.calc_time_resids
    out = {}
    try:
        for key, sig in gen_fit_spread.LEVELS.items():
            dl, dc = np.zeros(NPTS), np.zeros(NPTS)
            for pat in gen_fit_spread.patterns(ts):
                shift = pat * sig * u.s

                def calc(self, *a, **k):
                    return orig(self, *a, **k) + shift
                pres.Residuals.calc_time_resids = calc
                for k in range(NPTS):
                    lnl = float(bt.lnlikelihood(pts[k]))
                    dl[k] = max(dl[k], abs(lnl - base[k]["lnl"]))
                    # (lnL = -chi2_toa / 2 + terms the shift does not touch)
                    dc[k] = max(dc[k], 2.0 * abs(lnl - base[k]["lnl"]))
                pres.Residuals.calc_time_resids = orig
            out[key] = {"lnl": dl.tolist(), "chi2_toa": dc.tolist()}
    finally:
        pres.Residuals.calc_time_resids = orig
    return out


def gen(name):
    wb = name == "bayes_wb"
    par, model, ts = build_wb() if wb else build_nb(phoff=name == "bayes_phoff")
    with open(os.path.join(GOLDEN, name + ".par"), "w") as f:
        f.write(par)
    fit = fit_sigmas(model, ts, wb)
    labels, pts, prior_info = draw_points(model, fit, {"bayes_nb": 1, "bayes_phoff": 2, "bayes_wb": 3}[name])
    bt = BayesianTiming(model, ts, prior_info=prior_info)
    assert list(bt.param_labels) == labels
    print(f"{name}: {len(labels)} free parameters {labels}; likelihood_method {bt.likelihood_method}", file=sys.stderr)

    arr, flags = pack_toas(ts)
    tza, _ = pack_toas(model.get_TZR_toa(ts))
    arrays = dict(arr)
    arrays.update({"tzr_" + k: v for k, v in tza.items()})
    masks = mask_table(model, ts)
    arrays.update(masks)
    _, ra, rm = residual_outputs(model, ts)
    arrays.update(ra)
    if wb:
        arrays["wb_pp_dm"] = np.asarray(ts.get_dms().to_value(DMU), dtype=np.float64)
        arrays["wb_pp_dme"] = np.asarray(ts.get_dm_errors().to_value(DMU), dtype=np.float64)
    meta = {"name": name, "model": export_model(model), "flags": flags, "labels": labels, "prior_info": prior_info}
    obs = [str(o) for o in ts.get_obss()]
    meta["obs_names"] = sorted(set(obs))
    arrays["obs_index"] = np.array([meta["obs_names"].index(o) for o in obs], dtype=np.int16)
    meta.update(rm)
    meta["fit_sigma"] = {p: s for p, (_, s) in fit.items()}
    meta["is_wideband"] = bool(bt.is_wideband)
    meta["track_mode"] = bt.track_mode
    meta["likelihood_method"] = bt.likelihood_method

    arrays["pts_hi"], arrays["pts_lo"] = split_ld(pts)
    recs = []
    t0 = time.perf_counter()
    for k in range(NPTS):
        bt.lnlikelihood(pts[k])
    meta["ref_seconds_per_lnlikelihood"] = (time.perf_counter() - t0) / NPTS
    for k in range(NPTS):
        recs.append(point_record(bt, ts, pts[k], wb))
    for key in ("lnl", "chi2_toa", "lsig_toa", "chi2_dm", "lsig_dm", "lsig_dm_pccm3", "wrap"):
        arrays["pt_" + key] = np.array([r[key] for r in recs], dtype=np.float64)
    arrays["pt_time"] = np.array([r["time"] for r in recs])
    arrays["pt_dm_resid"] = np.array([r["dm"] for r in recs])
    arrays["pt_sig_toa"] = np.array([r["sig_toa"] for r in recs])
    arrays["pt_lnprior"] = np.array([float(bt.lnprior(pts[k])) for k in range(NPTS)])
    arrays["pt_lnposterior"] = np.array([float(bt.lnposterior(pts[k])) for k in range(NPTS)])
    for k in range(NPTS):  # the terms add up to the reference's lnlikelihood
        r = recs[k]
        tot = -r["chi2_toa"] / 2 - r["lsig_toa"] - r["chi2_dm"] / 2 - r["lsig_dm"]
        assert abs(tot - r["lnl"]) <= 1e-9 * abs(r["lnl"]), (k, tot, r["lnl"])
    # points outside the priors: each moves one parameter past its bound (uniform) and leaves the
    # rest at point 0; lnprior and lnposterior are -inf there
    uni = [j for j, p in enumerate(labels) if prior_info[p]["distr"] == "uniform"]
    out_pts = np.tile(pts[0], (len(uni), 1))
    for i, j in enumerate(uni):
        pi = prior_info[labels[j]]
        out_pts[i, j] = np.longdouble(pi["pmax"]) + np.longdouble(pi["pmax"] - pi["pmin"])
    arrays["out_hi"], arrays["out_lo"] = split_ld(out_pts)
    arrays["out_lnprior"] = np.array([float(bt.lnprior(p)) for p in out_pts])
    arrays["out_lnposterior"] = np.array([float(bt.lnposterior(p)) for p in out_pts])
    assert np.all(np.isneginf(arrays["out_lnprior"])) and np.all(np.isneginf(arrays["out_lnposterior"]))
    cube = np.random.default_rng(99).uniform(0.02, 0.98, (NPTS, len(labels)))
    arrays["cube"] = cube
    arrays["cube_transform"] = np.array([np.asarray(bt.prior_transform(c), dtype=np.float64) for c in cube])
    arrays["cube_lnprior"] = np.array([float(bt.lnprior(x)) for x in arrays["cube_transform"]])
    meta["forms"] = forms(model, ts, prior_info)
    print(f"  lnL {arrays['pt_lnl'].min():.3f} .. {arrays['pt_lnl'].max():.3f}; chi2_toa {arrays['pt_chi2_toa'].min():.2f} .. "
          f"{arrays['pt_chi2_toa'].max():.2f}; chi2_dm {arrays['pt_chi2_dm'].min():.2f} .. {arrays['pt_chi2_dm'].max():.2f}; "
          f"largest |phase residual| {arrays['pt_wrap'].max():.3g}; {meta['ref_seconds_per_lnlikelihood'] * 1e3:.1f} ms per call",
          file=sys.stderr)
    # the white-noise classes: TOAs grouped by the set of EFAC / EQUAD masks that select them
    keys = sorted(k for k in masks if k.startswith(("mask_EFAC", "mask_EQUAD")))
    sets = [tuple(k for k in keys if masks[k][i]) for i in range(ts.ntoas)]
    sizes = {}
    for s in sets:
        sizes["+".join(x[5:] for x in s) or "none"] = sizes.get("+".join(x[5:] for x in s) or "none", 0) + 1
    meta["noise_class_sizes"] = sizes
    print(f"  classes {sizes}", file=sys.stderr)
    refcommon.save(name, arrays, meta)

    path = os.path.join(GOLDEN, "bayes_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[name] = spread(bt, ts, pts, recs)
    res[name]["ref_seconds_per_lnlikelihood"] = meta["ref_seconds_per_lnlikelihood"]
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"  spread 5 ps: max |dlnL| {max(res[name]['5ps']['lnl']):.3g}; 30 ps: {max(res[name]['30ps']['lnl']):.3g}",
          file=sys.stderr)


if __name__ == "__main__":
    register_clockless_sites()
    for n in sys.argv[1:] or ["bayes_nb", "bayes_phoff", "bayes_wb"]:
        gen(n)
