"""Golden fixtures for the photon-event path (reference run; container only; TEST INFRASTRUCTURE).
Reuses the committed generators under oracle/refgen as they are.

* photon_geo  : 1500 photons at the geocenter.  gen_synth.pta_par(51, "ELL1") without its noise and DMX,
                with TZRMJD (AbsPhase); F0, F1, A1, PB, TASC, EPS1 and EPS2 free, each with an uncertainty
                in the par file.  Weighted (beta-distributed weights).  256-bin template from a
                two-component Gaussian file, divided by its mean (event_optimize.py:747-748).
* photon_bary : 256 photons at the barycentre, isolated pulsar, no AbsPhase; F0 and F1 free.  Unweighted,
                100-bin template.

The photons: make_fake_toas_uniform's zero-residual TOAs at infinite frequency, each shifted by
dphi / F0 (TOAs.adjust_TOAs) with dphi drawn from the two-Gaussian profile for a fraction of the photons
and uniformly for the rest (fixed seed).

For each: the packed TOAs (refcommon.pack_toas; the TZR TOA with AbsPhase), the photons' times in the
scale get_event_TOAs takes (TT at the geocenter, TDB at the barycentre) as (hi, lo) pairs, the model, 16
points within +-3 sigma of the par file's uncertainties as (hi, lo) pairs with PHASE in [0, 1] last, and
per point model.phase(toas).frac % 1, profile_likelihood, emcee_fitter.lnposterior's triple, hm, hmw,
z2m, z2mw and em_four at m = 20, and the scan of marginalize_over_phase(minimize=False, resolution=1/64)
(its returned pair, and profile_likelihood at each of its offsets).  The template, the Gaussian file's
text, gaussian_profile at a list of arguments, and the survival / significance functions on fixed lists.

Asserted: no (phi + PHASE) mod 1 lies within 1e-6 of (L - 1) / L, and at least 3 photons per point lie
in ((L - 1) / L, 1): the constant last segment of np.interp(..., right=tmpl[0]) is exercised.

photon_spread.json: per fixture and point, the reference's own |delta lnL|, |delta S_j| (the weighted trig
sums), |delta H| and |delta Z^2_j| when its phases are shifted by gen_fit_spread.patterns at 5 ps x F0 and
30 ps x F0 rms -- the rule of gen_fit_spread.measure and bayes_spread.json -- and the reference's time
per lnposterior call.

Usage: oracle/refenv/run_ref.sh scripts/refgen/gen_photon.py [photon_geo photon_bary]
"""
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle", "refgen"))

import astropy.units as u  # noqa: E402
from astropy.time import TimeDelta  # noqa: E402
from scipy.stats import norm, uniform  # noqa: E402
import refcommon  # noqa: E402
from refcommon import GOLDEN, register_clockless_sites, pack_toas, export_model, split_ld  # noqa: E402
from gen_synth import pta_par  # noqa: E402
import gen_fit_spread  # noqa: E402
import pint.simulation as sim  # noqa: E402
import pint.eventstats as es  # noqa: E402
from pint.models import get_model  # noqa: E402
from pint.models.priors import Prior  # noqa: E402
from pint.pulsar_mjd import time_to_longdouble  # noqa: E402
from pint.scripts.event_optimize import (emcee_fitter, gaussian_profile, marginalize_over_phase,  # noqa: E402
                                         profile_likelihood, read_gaussfitfile)

NPTS = 16
M = 20
GAUSS = """# two-component Gaussian template
const = 0.0
phas1 = 0.18000 +/- 0.00000
ampl1 = 0.60000 +/- 0.00000
fwhm1 = 0.05000 +/- 0.00000
phas2 = 0.61000 +/- 0.00000
ampl2 = 0.25000 +/- 0.00000
fwhm2 = 0.12000 +/- 0.00000
"""
PULSED = 0.65  # the fraction of the photons drawn from the profile
CASES = {
    "photon_geo": dict(seed=51, binary="ELL1", n=1500, nbin=256, obs="geocenter", weighted=True, abs_phase=True,
                       sigma={"F0": 4e-11, "F1": 3e-19, "A1": 3e-5, "PB": 2e-8, "TASC": 8e-6, "EPS1": 4e-6,
                              "EPS2": 4e-6}),
    "photon_bary": dict(seed=52, binary="", n=256, nbin=100, obs="@", weighted=False, abs_phase=False,
                        sigma={"F0": 4e-11, "F1": 3e-19}),
}


def par_text(case):
    """pta_par without noise, DMX (and TZR without AbsPhase); only the case's parameters free, each with
    its uncertainty in the fourth column."""
    drop = ("TNRed", "DMX", "EFAC", "EQUAD") + (() if case["abs_phase"] else ("TZR",))
    out = []
    for line in pta_par(case["seed"], case["binary"]).splitlines():
        t = line.split()
        if not t or t[0].startswith(drop):
            continue
        if t[0] in case["sigma"]:
            out.append(f"{t[0]} {t[1]} 1 {case['sigma'][t[0]]:.3e}")
        elif len(t) >= 3 and t[2] == "1" and t[0] not in ("PSR", "EPHEM", "CLK", "UNITS", "BINARY"):
            out.append(f"{t[0]} {t[1]}")
        else:
            out.append(line)
    return "\n".join(out) + "\n"


def template(nbin):
    with tempfile.NamedTemporaryFile("w", suffix=".gauss", delete=False) as f:
        f.write(GAUSS)
    try:
        raw = read_gaussfitfile(f.name, nbin)
    finally:
        os.unlink(f.name)
    t = raw.copy()
    t /= t.mean()  # (event_optimize.py:747-748)
    return raw, t


def draw_dphi(rng, n):
    """Phase offsets: the two Gaussians (wrapped) for a fraction PULSED, uniform for the rest."""
    comp = rng.uniform(size=n)
    amp = np.array([0.6, 0.25])
    which = rng.uniform(size=n) < amp[0] / amp.sum()
    g = np.where(which, rng.normal(0.18, 0.05 / 2.35482, n), rng.normal(0.61, 0.12 / 2.35482, n))
    return np.where(comp < PULSED, g % 1.0, rng.uniform(size=n))


def build(name):
    case = CASES[name]
    np.random.seed(case["seed"])
    par = par_text(case)
    model = get_model(io.StringIO(par))
    n = case["n"]
    ts = sim.make_fake_toas_uniform(53000, 56652, n, model, freq=np.inf * u.MHz, obs=case["obs"], error=1.0 * u.us,
                                    add_noise=False, include_bipm=False)
    rng = np.random.default_rng(case["seed"])
    dphi = draw_dphi(rng, n)
    ts.adjust_TOAs(TimeDelta(dphi / float(model.F0.value) * u.s))
    weights = rng.beta(1.2, 1.6, n) if case["weighted"] else None
    # a fresh model: zeroing the residuals added an AbsPhase component (TZRMJD = the first TOA) to the one
    # the TOAs were made with, and model.phase(toas) would then be relative to it
    model = get_model(io.StringIO(par))
    assert ("AbsPhase" in model.components) == case["abs_phase"]
    return case, par, model, ts, weights


def stat_table():
    """The survival and significance functions on fixed arguments."""
    hs = [1e-3, 0.5, 3.0, 12.0, 40.0, 110.0, 700.0]
    zs = [0.2, 3.0, 15.0, 60.0, 400.0]
    sig = [0.9, 0.32, 0.05, 2.7e-3, 1e-9, 1e-120, 1e-310]
    lsig = [-0.1, -3.0, -50.0, -600.0, -800.0, -5000.0]
    out = {"h": hs, "sf_hm": [float(es.sf_hm(h)) for h in hs], "sf_hm_log": [float(es.sf_hm(h, logprob=True)) for h in hs],
           "h2sig": [float(es.h2sig(h)) for h in hs],
           "z": zs, "sf_z2m": {str(m): [float(es.sf_z2m(z, m=m)) for z in zs] for m in (1, 2, 10, 20)},
           "sig": sig, "sig2sigma": [float(es.sig2sigma(s)) for s in sig],
           "sig2sigma_one": [float(es.sig2sigma(s, two_tailed=False)) for s in sig if s <= 0.5],
           "lsig": lsig, "sig2sigma_log": [float(es.sig2sigma(s, logprob=True)) for s in lsig],
           "sig2sigma_log_one": [float(es.sig2sigma(s, two_tailed=False, logprob=True)) for s in lsig[1:]]}
    return out


GP_ARGS = [(64, 0.1, 0.05), (64, 0.93, 0.2), (100, 0.5, 0.01), (33, 1.25, 0.4), (256, 0.0, 0.003)]


def stats_at(ph, w):
    """The reference's statistics of one set of phases."""
    wt = np.ones_like(ph) if w is None else w
    ak, bk = es.em_four(ph, m=M, weights=w)
    return {"hm": float(es.hm(ph, m=M)), "hmw": float(es.hmw(ph, wt, m=M)), "z2m": np.asarray(es.z2m(ph, m=M)),
            "z2mw": np.asarray(es.z2mw(ph, wt, m=M)), "ak": np.asarray(ak), "bk": np.asarray(bk),
            "S": np.concatenate([np.asarray(ak), np.asarray(bk)]) * (len(ph) if w is None else w.sum())}


def gen(name):
    case, par, model, ts, weights = build(name)
    with open(os.path.join(GOLDEN, name + ".par"), "w") as f:
        f.write(par)
    n, L = case["n"], case["nbin"]
    raw, tmpl = template(L)
    xtemp = np.arange(L) * 1.0 / L
    labels = [p for p in model.params if not getattr(model, p).frozen]
    assert set(labels) == set(case["sigma"]), labels
    rng = np.random.default_rng(1000 + case["seed"])
    prior_info = {}
    base = {p: np.longdouble(getattr(model, p).value) for p in labels}
    for p in labels:
        v, s = float(base[p]), case["sigma"][p]
        if p in ("F1", "PB"):
            prior_info[p] = {"distr": "normal", "mu": v, "sigma": 5.0 * s}
        else:
            prior_info[p] = {"distr": "uniform", "pmin": v - 10.0 * s, "pmax": v + 10.0 * s}
    for p, info in prior_info.items():  # (BayesianTiming.__init__'s prior_info handling, bayesian.py:80-93)
        if info["distr"] == "normal":
            getattr(model, p).prior = Prior(norm(info["mu"], info["sigma"]))
        else:
            getattr(model, p).prior = Prior(uniform(info["pmin"], info["pmax"] - info["pmin"]))
    ftr = emcee_fitter(ts, model, tmpl, weights, phs=0.5, phserr=0.03)
    assert ftr.fitkeys == labels + ["PHASE"], ftr.fitkeys

    pts = np.zeros((NPTS, len(labels) + 1), dtype=np.longdouble)
    phases = np.zeros((NPTS, n))
    edge = (L - 1.0) / L
    for k in range(NPTS):
        for j, p in enumerate(labels):
            pts[k, j] = base[p] + np.longdouble(case["sigma"][p]) * np.longdouble(rng.uniform(-3, 3))
        ftr.set_params(dict(zip(labels, pts[k, :-1])))
        phases[k] = np.asarray(ftr.get_event_phases(), dtype=np.float64)
        assert np.all((phases[k] >= 0) & (phases[k] < 1))
        for _ in range(1000):  # a PHASE that exercises the last segment and keeps clear of its step
            phs = rng.uniform(0.0, 1.0)
            x = (phases[k] + phs) % 1
            if np.min(np.abs(x - edge)) > 1e-6 and np.count_nonzero(x > edge) >= 3:
                break
        else:
            raise AssertionError((name, k, "no PHASE meets the last-segment conditions"))
        pts[k, -1] = phs

    arr, flags = pack_toas(ts)
    arrays = dict(arr)
    if case["abs_phase"]:
        tza, _ = pack_toas(model.get_TZR_toa(ts))
        arrays.update({"tzr_" + k: v for k, v in tza.items()})
    t = ts.table["mjd"]
    scale = [x.tdb if case["obs"] == "@" else x.tt for x in t]
    arrays["ev_hi"], arrays["ev_lo"] = split_ld(np.array([time_to_longdouble(x) for x in scale], dtype=np.longdouble))
    if weights is not None:
        arrays["weights"] = weights
    arrays["tmpl"], arrays["tmpl_raw"] = tmpl, raw
    for i, (N, ph, fw) in enumerate(GP_ARGS):
        arrays[f"gp_{i}"] = gaussian_profile(N, ph, fw)
    meta = {"name": name, "model": export_model(model), "flags": flags, "labels": labels + ["PHASE"],
            "prior_info": prior_info, "gauss": GAUSS, "gp_args": GP_ARGS, "nbin": L, "abs_phase": case["abs_phase"],
            "weighted": case["weighted"], "fit_sigma": case["sigma"], "stats": stat_table(), "m": M}
    obs = [str(o) for o in ts.get_obss()]
    meta["obs_names"] = sorted(set(obs))
    arrays["obs_index"] = np.array([meta["obs_names"].index(o) for o in obs], dtype=np.int16)
    arrays["pts_hi"], arrays["pts_lo"] = split_ld(pts)
    arrays["pt_phase"] = phases

    lnl, post, scan, scan_ret, st = [], [], [], [], []
    t0 = time.perf_counter()
    for k in range(NPTS):
        post.append([float(x) for x in ftr.lnposterior(pts[k])])
    meta["ref_seconds_per_lnposterior"] = (time.perf_counter() - t0) / NPTS
    dphss = np.arange(0.0, 1.0, 1.0 / 64)
    for k in range(NPTS):
        x = (phases[k] + np.float64(pts[k, -1])) % 1
        assert np.min(np.abs(x - edge)) > 1e-6 and np.count_nonzero(x > edge) >= 3, (name, k)
        lnl.append(float(profile_likelihood(np.float64(pts[k, -1]), xtemp, phases[k], tmpl, weights)))
        assert abs(lnl[-1] - post[k][2]) <= 1e-12 * abs(lnl[-1]), (k, lnl[-1], post[k])
        scan.append([float(profile_likelihood(np.float64(d), xtemp, phases[k], tmpl, weights)) for d in dphss])
        r = marginalize_over_phase(phases[k], tmpl, weights=weights, resolution=1.0 / 64, minimize=False)
        scan_ret.append([float(r[0]), float(r[1])])
        assert abs(scan_ret[-1][1] - max(scan[-1])) <= 1e-12 * abs(scan_ret[-1][1]), (k, scan_ret[-1], max(scan[-1]))
        st.append(stats_at(phases[k], weights))
    arrays["pt_lnl"] = np.array(lnl)
    arrays["pt_post"] = np.array(post)
    arrays["pt_scan"] = np.array(scan)
    arrays["pt_scan_ret"] = np.array(scan_ret)
    for key in ("hm", "hmw", "z2m", "z2mw", "ak", "bk"):
        arrays["pt_" + key] = np.array([s[key] for s in st])
    print(f"{name}: {labels}; lnL {min(lnl):.3f} .. {max(lnl):.3f}; H {arrays['pt_hmw'].min():.1f} .. "
          f"{arrays['pt_hmw'].max():.1f}; {meta['ref_seconds_per_lnposterior'] * 1e3:.1f} ms per lnposterior",
          file=sys.stderr)
    refcommon.save(name, arrays, meta)

    # the reference's own spread under phase shifts of 5 ps x F0 and 30 ps x F0 rms
    f0 = float(model.F0.value)
    res = {}
    for key, sig in gen_fit_spread.LEVELS.items():
        d = {"lnl": np.zeros(NPTS), "S": np.zeros((NPTS, 2 * M)), "h": np.zeros(NPTS), "z2": np.zeros((NPTS, M)),
             "scan": np.zeros(NPTS)}
        for pat in gen_fit_spread.patterns(ts):
            for k in range(NPTS):
                ph = (phases[k] + pat * sig * f0) % 1
                l2 = float(profile_likelihood(np.float64(pts[k, -1]), xtemp, ph, tmpl, weights))
                s2 = stats_at(ph, weights)
                sc = max(abs(float(profile_likelihood(np.float64(dd), xtemp, ph, tmpl, weights)) - scan[k][i])
                         for i, dd in enumerate(dphss))
                d["lnl"][k] = max(d["lnl"][k], abs(l2 - lnl[k]))
                d["scan"][k] = max(d["scan"][k], sc)
                d["S"][k] = np.maximum(d["S"][k], np.abs(s2["S"] - st[k]["S"]))
                hk = "hmw" if weights is not None else "hm"
                zk = "z2mw" if weights is not None else "z2m"
                d["h"][k] = max(d["h"][k], abs(s2[hk] - st[k][hk]))
                d["z2"][k] = np.maximum(d["z2"][k], np.abs(s2[zk] - st[k][zk]))
        res[key] = {a: b.tolist() for a, b in d.items()}
    res["ref_seconds_per_lnposterior"] = meta["ref_seconds_per_lnposterior"]
    res["F0"] = f0
    path = os.path.join(GOLDEN, "photon_spread.json")
    allres = json.load(open(path)) if os.path.exists(path) else {}
    allres[name] = res
    with open(path, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
    print(f"  spread 5 ps: max |dlnL| {max(res['5ps']['lnl']):.3g}; 30 ps: {max(res['30ps']['lnl']):.3g}", file=sys.stderr)


if __name__ == "__main__":
    register_clockless_sites()
    for nm in sys.argv[1:] or list(CASES):
        gen(nm)
