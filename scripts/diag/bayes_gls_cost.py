"""What a batch of BayesianTiming(correlated_noise=True).lnlikelihood_batch costs, beside the only route
to the same number without the batched pass and beside the white-noise pass on the same shape.  Three
shapes: N = 4096 points of the 300-TOA fixtures bayes_gls_red (21 columns, 65 ECORR epochs) and bayes_gls_dmn
(37 columns), and N = 256 points of a 10,000-TOA pulsar with 30 + 30 Fourier modes (c5_ell1 with a PLDMNoise
added: 121 columns).

Each figure is the median of REPS host-clock windows around calls that end in a device synchronise (the
Session is not lazy), after WARM warm-up rounds, the variants alternating inside one round:

  white      set_points + eval + point_lnlike       (the white-noise pass on the same batch: a lower bound)
  gls        set_points + eval + point_lnlike_gls   (the difference to white: the new pass against k_point_lnl)
  batch      BayesianTiming.lnlikelihood_batch      (gls plus the host's class, epoch and Fourier values)
  per_point  the route without the pass, one point at a time on fixed residuals: pint_set_sigma +
             pint_set_noise_weights + pint_fit_step(1) + pint_chi2_gls + pint_lognorm
             (NoiseLikelihood kind 3), timed over PER_POINT points, per point

and the pass's own work per point: (n + nep) W (W + 1) + W^3 / 3 flops (W = columns + 1: the lower triangle
of the augmented Gram in 4x4 tiles, then the Cholesky) and the bytes of the rows it reads.  A tree without
the pass (the keyword correlated_noise) runs per_point and white alone.  One JSON line on stdout.

Usage: python scripts/diag/bayes_gls_cost.py [--reps 20] [--warm 3] [--per-point 16]
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LD = np.longdouble
PEAK_FP64_TFLOPS = 78.6  # MI355X vector FP64


def draw(model, labels, offsets, base, N):
    rng = np.random.default_rng(5)
    pts = np.tile(base, (N, 1))
    for j, p in enumerate(labels):
        if p in offsets:
            pts[:, j] += abs(base[j]) * LD(1e-12) * rng.uniform(-1, 1, N).astype(LD)
        elif p.endswith(("AMP", "GAM")):
            pts[:, j] += rng.uniform(-0.3, 0.3, N)
        else:
            pts[:, j] *= rng.uniform(0.8, 1.2, N)
    return pts


def per_point_route(model, toas, noise, pts_noise, reps):
    """NoiseLikelihood's Woodbury route at each row of pts_noise, ms per point."""
    from pint_amd.noisefit import NoiseLikelihood
    nl = NoiseLikelihood(toas, model, noise)
    try:
        for x in pts_noise[:2]:
            nl.evaluate(list(x), grad=False)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for x in pts_noise:
                nl.evaluate(list(x * (1 + 1e-9 * len(t))), grad=False)  # (a new key each time: no cache hit)
            t.append((time.perf_counter() - t0) * 1e3 / len(pts_noise))
        return float(np.median(t)), float(np.subtract(*np.percentile(t, [75, 25]))), nl.kind
    finally:
        nl.close()


def measure(tag, model, toas, prior_info, N, a):
    from pint_amd import BayesianTiming
    have = "correlated_noise" in inspect.signature(BayesianTiming.__init__).parameters
    noise = [p for p in model.free_params if p.startswith(("EFAC", "EQUAD", "ECORR", "TNRED", "TNDM"))]
    out = {"shape": tag, "ntoas": toas.ntoas, "npoints": N, "has_pass": have}
    base_noise = np.array([float(model[p].value) for p in noise])
    rng = np.random.default_rng(6)
    pn = base_noise * rng.uniform(0.9, 1.1, (a.per_point, len(noise)))
    try:
        med, iqr, kind = per_point_route(model, toas, noise, pn, max(3, a.reps // 4))
    except Exception as e:  # noqa: BLE001 (a shape the route refuses: the record is the message)
        med, iqr, kind = float("nan"), float("nan"), str(e)
    out["per_point_route_ms_per_point"], out["per_point_route_iqr_ms"], out["per_point_route_kind"] = med, iqr, kind
    if not have:
        return out
    bt = BayesianTiming(model, toas, prior_info=prior_info, correlated_noise=True)
    s, lay = bt._device(), bt.lay
    pts = draw(bt.model, bt.param_labels, lay.offsets, bt._base_values, N)
    names = [p for _, p in bt._timing]
    cols = [j for j, _ in bt._timing]
    qf = bt._qf(pts, bt._cls)
    ep = bt._ep_phi(pts) if bt._ep else None
    ph = bt._four_phi(pts) if len(bt._ff) else None

    def white():
        s.set_points(lay, bt._table0, names, pts[:, cols])
        s.eval(False)
        s.point_lnlike(qf)

    def gls():
        s.set_points(lay, bt._table0, names, pts[:, cols])
        s.eval(False)
        s.point_lnlike_gls(qf, ep, ph, bt._ones)

    def batch():
        bt.lnlikelihood_batch(pts)

    variants = {"white": white, "gls": gls, "batch": batch}
    t = {k: [] for k in variants}
    for r in range(a.warm + a.reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= a.warm:
                t[k].append(dt * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    nep = getattr(lay, "nep", 0) or 0
    W = 2 * lay.nred + bt._ones + 1
    nd = lay.nred - lay.spec.dmn0 if lay.nred else 0
    flops = (lay.n + nep) * W * (W + 1) + W ** 3 / 3
    # p, ftay, sigma0 (8 B each), class (4 B), e^{i theta} and e^{i 8 theta} (32 B); PLDMNoise: the row's time
    # (16 B), frequency (8 B) and velocity (24 B); the epochs' rows once more
    row = 28 + (32 if lay.nred else 0) + (48 if nd else 0)
    nbytes = row * (lay.n + (int(lay.ep_ptr[-1]) if nep else 0)) + 28 * lay.n
    pass_ms = med["gls"] - med["white"]
    out.update({"nfree": bt.nparams, "columns": W - 1, "nep": nep, "ms": med,
                "ms_iqr": {k: float(np.subtract(*np.percentile(v, [75, 25]))) for k, v in t.items()},
                "new_pass_minus_white_pass_ms": pass_ms, "host_share_of_batch_ms": med["batch"] - med["gls"],
                "us_per_point": med["batch"] * 1e3 / N,
                "per_point_route_over_batch": med_ratio(out["per_point_route_ms_per_point"], med["batch"] / N),
                "pass_flops_per_point": flops, "pass_bytes_per_point": nbytes,
                "pass_gflops": flops * N / max(pass_ms, 1e-9) * 1e-6,
                "pass_fraction_of_fp64_peak": flops * N / max(pass_ms, 1e-9) * 1e-9 / PEAK_FP64_TFLOPS,
                "pass_gbytes_per_s": nbytes * N / max(pass_ms, 1e-9) * 1e-6})
    bt.close()
    return out


def med_ratio(a, b):
    return float(a / b) if b > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--per-point", type=int, default=16)
    a = ap.parse_args()
    import golden_util
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    res = []
    spread = json.load(open(os.path.join(golden_util.GOLDEN, "bayes_gls_spread.json")))
    for name in ("bayes_gls_red", "bayes_gls_dmn"):
        z = dict(np.load(os.path.join(golden_util.GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(golden_util.GOLDEN, name + ".json")))
        toas = from_arrays_with_tzr(z, dict(meta["flag_columns"]), name, meta.get("obs_names"))
        model = get_model(os.path.join(golden_util.GOLDEN, name + ".par"))
        model.free_params = list(meta["model"]["free_params"])
        res.append(measure(name, model, toas, meta["prior_info"], 4096, a))
        res[-1]["reference_ms_per_point"] = spread[name]["ref_seconds_per_lnlikelihood"] * 1e3
    _, toas, _, _ = golden_util.load("c5_ell1")
    par = open(os.path.join(golden_util.GOLDEN, "c5_ell1.par")).read()
    par = "\n".join(l for l in par.splitlines() if not l.upper().startswith(("TNRED", "TNDM"))) + "\n"
    model = get_model(par + "TNREDAMP -13.5 1\nTNREDGAM 3.5 1\nTNREDC 30\nTNDMAMP -13.2 1\nTNDMGAM 2.8 1\nTNDMC 30\n")
    # (DMX frozen: with its bins free the per-point route's normal matrix, timing columns + 120 noise columns,
    # is beyond pint_fit_step's LDS solve)
    model.free_params = [p for p in model.free_params if p not in ("TNREDC", "TNDMC") and not p.startswith("DMX_")]
    pi = {}
    for p in model.free_params:
        v = float(model[p].value)
        w = 3.0 if p.startswith("TN") else max(abs(v) * 1e-6, 1e-12)
        pi[p] = {"distr": "uniform", "pmin": v - w, "pmax": v + w}
    res.append(measure("c5_ell1_10k_30+30", model, toas, pi, 256, a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
