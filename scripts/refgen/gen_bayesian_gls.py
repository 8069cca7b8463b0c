"""Golden fixtures for BayesianTiming(correlated_noise=True) (reference run; container only; TEST
INFRASTRUCTURE).  Reuses the committed generators under oracle/refgen as they are.

The reference's BayesianTiming refuses correlated noise; the number recorded per point is its
Residuals(toas, model, track_mode="nearest").lnlikelihood() (residuals.py:567-716) with the model's
free parameters set to the point, which is what a BayesianTiming with the GLS likelihood evaluates.

Every fixture: 300 TOAs, gen_synth.pta_par(43, "ELL1") without its DMX and flag-keyed EFAC / EQUAD and
with PX 5 mas (the +-3 sigma draws stay at positive parallaxes),
simulated with multi_freqs_in_epoch=True (75 epochs of the four frequencies; the TOAs of an epoch
lie within a microsecond of each other), white and correlated noise added.  Mask ranges on the
epochs' MJDs: ECORR1 over epochs 0-29, ECORR2 over epochs 40-74 (the 40 TOAs of epochs 30-39 are in no
ECORR epoch); epoch 29's two upper frequencies are moved 0.4 s later before the simulation and ECORR1's
range ends 0.2 s after the epoch, so that its ECORR epoch holds 2 TOAs; EFAC over epochs 0-49 and EQUAD
over epochs 20-59 (the TOAs of epochs 60-74 are in no EFAC / EQUAD class).

* bayes_gls_red       : PLRedNoise (TNREDC 10) + ECORR + EFAC / EQUAD, no PhaseOffset (the 1e40 column
                        of ones); every timing and noise parameter free.
* bayes_gls_red_phoff : the same with PHOFF free.
* bayes_gls_ecorr     : ECORR + EFAC / EQUAD only, PHOFF free (the reference's Sherman-Morrison branch,
                        _calc_ecorr_chi2).
* bayes_gls_dmn       : PLRedNoise (TNREDC 8) + PLDMNoise (TNDMC 10) + ECORR, no PhaseOffset: 37 columns.

Per fixture 16 points: timing parameters within +-3 sigma of a one-step GLS fit, EFAC / EQUAD / ECORR
within +-30 %, log amplitudes within +-0.5, indices within +-1; per point lnlikelihood, chi2, the log
normalisation, the time residuals, that cho_factor succeeded, lnprior and lnposterior from the
fixture's prior_info (BayesianTiming's expressions), the largest |phase residual| (asserted < 0.45).

bayes_gls_spread.json: gen_fit_spread.measure's rule at 5 and 30 ps on lnL and chi2, and the reference's
seconds per lnlikelihood call.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_bayesian_gls.py [names]
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
from astropy.time import TimeDelta  # noqa: E402
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
from pint.models.priors import Prior  # noqa: E402
from scipy.stats import norm, uniform  # noqa: E402

NPTS = 16
NAMES = ("bayes_gls_red", "bayes_gls_red_phoff", "bayes_gls_ecorr", "bayes_gls_dmn")
SCALE = ("EFAC", "EQUAD", "ECORR")
AMP = ("TNREDAMP", "TNDMAMP")
GAM = ("TNREDGAM", "TNDMGAM")
NOISE_LINES = {
    "bayes_gls_red": "TNREDAMP -13.3 1\nTNREDGAM 3.6 1\nTNREDC 10\n",
    "bayes_gls_red_phoff": "TNREDAMP -13.3 1\nTNREDGAM 3.6 1\nTNREDC 10\nPHOFF 0.0 1\n",
    "bayes_gls_ecorr": "PHOFF 0.0 1\n",
    "bayes_gls_dmn": "TNREDAMP -13.3 1\nTNREDGAM 3.6 1\nTNREDC 8\nTNDMAMP -13.0 1\nTNDMGAM 2.8 1\nTNDMC 10\n",
}


def strip(par, prefixes):
    return "\n".join(l for l in par.splitlines() if not (l.split() and l.split()[0].startswith(prefixes))) + "\n"


def is_noise(p):
    return p.startswith(SCALE) or p in AMP or p in GAM


def build(name):
    np.random.seed(43)
    # (PX 5 mas instead of pta_par's 1 mas: 300 TOAs fix it to 1.2 mas, and a +-3 sigma draw about 1 mas
    # would sample negative parallaxes, which are unphysical)
    base = strip(pta_par(43, "ELL1"), ("TNRed", "DMX", "EFAC", "EQUAD", "PX")) + "PX 5.0 1\n"
    freqs = np.array([800, 1200, 1600, 2000]) * u.MHz
    true = get_model(io.StringIO(base))
    ts0 = sim.make_fake_toas_uniform(53000, 56652, 300, true, freq=freqs, obs="geocenter", error=0.5 * u.us,
                                     add_noise=False, include_bipm=False, multi_freqs_in_epoch=True)
    mj = np.asarray(ts0.get_mjds().value, dtype=np.float64)
    ep = np.unique(np.round(mj, 6))  # the epochs
    assert len(ep) in (75, 76) and ts0.ntoas == 300, (len(ep), ts0.ntoas)
    # epoch 29: its two upper frequencies 0.4 s later
    fr = np.asarray(ts0.get_freqs().to_value(u.MHz))
    move = (np.abs(mj - ep[29]) < 1e-6) & (fr > 1400)
    assert move.sum() == 2
    delta = np.where(move, 0.4, 0.0) * u.s
    ts0.adjust_TOAs(TimeDelta(delta))

    def mid(k):
        return 0.5 * (ep[k - 1] + ep[k])
    cut = ep[29] + 0.2 / 86400.0
    par = base + (f"EFAC mjd {ep[0] - 1.0:.4f} {mid(50):.4f} 1.2 1\nEQUAD mjd {mid(20):.4f} {mid(60):.4f} 0.3 1\n"
                  f"ECORR mjd {ep[0] - 1.0:.4f} {cut:.8f} 0.6 1\nECORR mjd {mid(40):.4f} {ep[-1] + 1.0:.4f} 0.4 1\n")
    par += NOISE_LINES[name]
    model = get_model(io.StringIO(par))
    ts = sim.make_fake_toas(ts0, model, add_noise=True, add_correlated_noise=True)
    return par, model, ts


def fit_sigmas(model, ts):
    """A one-step GLS fit of the timing parameters (noise parameters held)."""
    m = copy.deepcopy(model)
    for p in m.free_params:
        if is_noise(p):
            getattr(m, p).frozen = True
    f = pfit.GLSFitter(ts, m)
    f.fit_toas(maxiter=1)
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
        if p.startswith(SCALE):
            v = float(getattr(model, p).value)
            pts[:, j] = v * rng.uniform(0.7, 1.3, NPTS)
            prior_info[p] = {"distr": "uniform", "pmin": 0.1 * v, "pmax": 3.0 * v}
        elif p in AMP or p in GAM:
            v = float(getattr(model, p).value)
            w = 0.5 if p in AMP else 1.0
            pts[:, j] = v + rng.uniform(-w, w, NPTS)
            prior_info[p] = {"distr": "uniform", "pmin": v - 3 * w, "pmax": v + 3 * w}
        else:
            v, s = fit[p]
            pts[:, j] = v + np.longdouble(s) * rng.uniform(-3, 3, NPTS).astype(np.longdouble)
            if p in ("F1", "PB"):
                prior_info[p] = {"distr": "normal", "mu": float(v), "sigma": 5.0 * s}
            else:
                prior_info[p] = {"distr": "uniform", "pmin": float(v) - 10.0 * s, "pmax": float(v) + 10.0 * s}
    return labels, pts, prior_info


def set_priors(model, prior_info):
    """BayesianTiming.__init__'s prior_info handling (bayesian.py:80-93)."""
    for par, info in prior_info.items():
        if info["distr"] == "uniform":
            getattr(model, par).prior = Prior(uniform(info["pmin"], info["pmax"] - info["pmin"]))
        else:
            getattr(model, par).prior = Prior(norm(info["mu"], info["sigma"]))


def lnprior(model, labels, pt):
    """BayesianTiming.lnprior (bayesian.py:124-148)."""
    tot = 0.0
    for v, p in zip(pt, labels):
        lp = getattr(model, p).prior_pdf(v, logpdf=True)
        if lp in (np.nan, -np.inf):
            return -np.inf
        tot += lp
    return float(tot)


def branch(model):
    """calc_chi2's dispatch (residuals.py:703-711)."""
    if not model.has_time_correlated_errors and "PhaseOffset" in model.components:
        return "ecorr"
    return "gls"


def evaluate(model, ts, labels, pt):
    model.set_param_values(dict(zip(labels, pt)))
    res = pres.Residuals(ts, model, track_mode="nearest")
    try:
        chi2, lognorm = res.calc_chi2(lognorm=True)
        ok = True
    except np.linalg.LinAlgError:
        chi2, lognorm, ok = np.nan, np.nan, False
    return res, float(chi2), float(lognorm), ok


def point_record(model, ts, labels, pt):
    res, chi2, lognorm, ok = evaluate(model, ts, labels, pt)
    lnl = float(res.lnlikelihood())
    full = res.calc_phase_resids(subtract_mean=False)
    full = np.asarray(getattr(full, "value", full), dtype=np.float64)
    assert np.max(np.abs(full)) < 0.45, ("a residual within 0.05 cycle of a wrap", float(np.max(np.abs(full))))
    return {"lnl": lnl, "chi2": chi2, "lognorm": lognorm, "chol_ok": ok,
            "time": np.asarray(res.time_resids.to_value(u.s), dtype=np.float64),
            "sig_toa": np.asarray(model.scaled_toa_uncertainty(ts).to_value(u.s), dtype=np.float64),
            "wrap": float(np.max(np.abs(full)))}


def spread(model, ts, labels, pts, base):
    """|delta lnL| and |delta chi2| per point under gen_fit_spread.patterns at each level."""
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
                    _, chi2, lognorm, _ = evaluate(model, ts, labels, pts[k])
                    dl[k] = max(dl[k], abs(-(chi2 / 2 + lognorm) - base[k]["lnl"]))
                    dc[k] = max(dc[k], abs(chi2 - base[k]["chi2"]))
                pres.Residuals.calc_time_resids = orig
            out[key] = {"lnl": dl.tolist(), "chi2": dc.tolist()}
    finally:
        pres.Residuals.calc_time_resids = orig
    return out


def gen(name):
    par, model, ts = build(name)
    with open(os.path.join(GOLDEN, name + ".par"), "w") as f:
        f.write(par)
    fit = fit_sigmas(model, ts)
    labels, pts, prior_info = draw_points(model, fit, 10 + NAMES.index(name))
    work = copy.deepcopy(model)
    set_priors(work, prior_info)
    print(f"{name}: {len(labels)} free parameters {labels}; branch {branch(model)}", file=sys.stderr)

    arr, flags = pack_toas(ts)
    tza, _ = pack_toas(model.get_TZR_toa(ts))
    arrays = dict(arr)
    arrays.update({"tzr_" + k: v for k, v in tza.items()})
    masks = mask_table(model, ts)
    arrays.update(masks)
    _, ra, rm = residual_outputs(model, ts)
    arrays.update(ra)
    meta = {"name": name, "model": export_model(model), "flags": flags, "labels": labels, "prior_info": prior_info}
    obs = [str(o) for o in ts.get_obss()]
    meta["obs_names"] = sorted(set(obs))
    arrays["obs_index"] = np.array([meta["obs_names"].index(o) for o in obs], dtype=np.int16)
    meta.update(rm)
    meta["fit_sigma"] = {p: s for p, (_, s) in fit.items()}
    meta["track_mode"] = "nearest"
    meta["likelihood_method"] = "gls"
    meta["ref_branch"] = branch(model)
    meta["ones_column"] = "PHOFF" not in model.free_params
    try:
        BayesianTiming(model, ts, prior_info=prior_info)
        meta["ref_bayesian_refusal"] = None
    except Exception as e:  # noqa: BLE001 (the record is the exception)
        meta["ref_bayesian_refusal"] = {"error": type(e).__name__, "message": str(e)}

    # the ECORR epochs: sizes per ECORR parameter, TOAs in none
    U = model.components["EcorrNoise"].get_noise_basis(ts)
    meta["ecorr_epoch_sizes"] = [int(x) for x in U.sum(axis=0)]
    meta["toas_in_no_epoch"] = int(np.sum(U.sum(axis=1) == 0))
    arrays["ecorr_basis_epoch"] = np.where(U.sum(axis=1) > 0, np.argmax(U, axis=1), -1).astype(np.int32)
    keys = sorted(k for k in masks if k.startswith(("mask_EFAC", "mask_EQUAD")))
    sets = [tuple(k for k in keys if masks[k][i]) for i in range(ts.ntoas)]
    sizes = {}
    for s in sets:
        sizes["+".join(x[5:] for x in s) or "none"] = sizes.get("+".join(x[5:] for x in s) or "none", 0) + 1
    meta["noise_class_sizes"] = sizes
    print(f"  epochs {sorted(set(meta['ecorr_epoch_sizes']))} x {len(meta['ecorr_epoch_sizes'])}, "
          f"{meta['toas_in_no_epoch']} TOAs in none; classes {sizes}", file=sys.stderr)

    arrays["pts_hi"], arrays["pts_lo"] = split_ld(pts)
    t0 = time.perf_counter()
    for k in range(NPTS):
        evaluate(work, ts, labels, pts[k])[0].lnlikelihood()
    meta["ref_seconds_per_lnlikelihood"] = (time.perf_counter() - t0) / NPTS
    recs = [point_record(work, ts, labels, pts[k]) for k in range(NPTS)]
    for key in ("lnl", "chi2", "lognorm", "wrap"):
        arrays["pt_" + key] = np.array([r[key] for r in recs], dtype=np.float64)
    arrays["pt_chol_ok"] = np.array([r["chol_ok"] for r in recs], dtype=bool)
    arrays["pt_time"] = np.array([r["time"] for r in recs])
    arrays["pt_sig_toa"] = np.array([r["sig_toa"] for r in recs])
    arrays["pt_lnprior"] = np.array([lnprior(work, labels, pts[k]) for k in range(NPTS)])
    arrays["pt_lnposterior"] = arrays["pt_lnprior"] + arrays["pt_lnl"]
    assert np.all(arrays["pt_chol_ok"]) and np.all(np.isfinite(arrays["pt_lnl"]))
    print(f"  lnL {arrays['pt_lnl'].min():.3f} .. {arrays['pt_lnl'].max():.3f}; chi2 {arrays['pt_chi2'].min():.2f} .. "
          f"{arrays['pt_chi2'].max():.2f}; largest |phase residual| {arrays['pt_wrap'].max():.3g}; "
          f"{meta['ref_seconds_per_lnlikelihood'] * 1e3:.1f} ms per call", file=sys.stderr)
    refcommon.save(name, arrays, meta)

    path = os.path.join(GOLDEN, "bayes_gls_spread.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[name] = spread(work, ts, labels, pts, recs)
    res[name]["ref_seconds_per_lnlikelihood"] = meta["ref_seconds_per_lnlikelihood"]
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"  spread 5 ps: max |dlnL| {max(res[name]['5ps']['lnl']):.3g}; 30 ps: {max(res[name]['30ps']['lnl']):.3g}",
          file=sys.stderr)


if __name__ == "__main__":
    register_clockless_sites()
    for n in sys.argv[1:] or NAMES:
        gen(n)
