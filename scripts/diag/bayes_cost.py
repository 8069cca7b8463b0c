"""What a batch of BayesianTiming.lnlikelihood_batch costs, beside the floor the grid path could
already run on the same shape: pint_set_grid (16 variables at most) + pint_eval(0) + pint_chi2_wls with
the pulsar's own sigma.  Two shapes: N = 4096 points of the 300-TOA bayes_nb fixture (thousands of
small points) and N = 256 points of a 10,000-TOA pulsar (c5_ell1 without its red noise).

Each figure is the median of REPS host-clock windows around calls that end in a device synchronise
(the Session is not lazy), after WARM warm-up rounds, the variants alternating inside one round:

  floor      set_grid + eval + chi2_wls
  points     set_points + eval + chi2_wls      (the difference to floor: pint_set_points)
  lnlike     set_points + eval + point_lnlike  (the difference to points: the new pass against k_chi2w)
  batch      BayesianTiming.lnlikelihood_batch (lnlike plus the host's class values and copies)

and the bytes the new pass reads per row.  One JSON line on stdout.

Usage: python scripts/diag/bayes_cost.py [--reps 30] [--warm 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LD = np.longdouble


def measure(tag, model, toas, prior_info, N, reps, warm):
    from pint_amd import BayesianTiming
    bt = BayesianTiming(model, toas, prior_info=prior_info)
    s, lay = bt._device(), bt.lay
    rng = np.random.default_rng(5)
    base = bt._base_values
    pts = np.tile(base, (N, 1))
    for j, p in enumerate(bt.param_labels):
        scale = abs(base[j]) * LD(1e-12) if p in lay.offsets else abs(base[j]) * LD(0.05)
        pts[:, j] += scale * rng.uniform(-1, 1, N).astype(LD)
    names = [p for _, p in bt._timing]
    cols = [j for j, _ in bt._timing]
    grid_vars = [(p, pts[:, j], 1, N) for j, p in list(zip(cols, names))[:16]]
    qf = bt._qf(pts, bt._cls)
    dqf = bt._qf(pts, bt._dmcls) if bt.is_wideband else None

    def floor():
        s.set_grid(lay, bt._table0, grid_vars, N)
        s.eval(False)
        s.chi2_wls()

    def points():
        s.set_points(lay, bt._table0, names, pts[:, cols])
        s.eval(False)
        s.chi2_wls()

    def lnlike():
        s.set_points(lay, bt._table0, names, pts[:, cols])
        s.eval(False)
        s.point_lnlike(qf, dqf)

    def batch():
        bt.lnlikelihood_batch(pts)

    variants = {"floor": floor, "points": points, "lnlike": lnlike, "batch": batch}
    t = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= warm:
                t[k].append(dt * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"shape": tag, "ntoas": lay.n, "npoints": N, "nfree": bt.nparams, "ntable_free": len(names),
           "grid_variables_in_floor": len(grid_vars), "ms": med,
           "ms_iqr": {k: float(np.subtract(*np.percentile(v, [75, 25]))) for k, v in t.items()},
           "set_points_minus_set_grid_ms": med["points"] - med["floor"],
           "new_pass_minus_chi2w_ms": med["lnlike"] - med["points"],
           "host_share_of_batch_ms": med["batch"] - med["lnlike"],
           "us_per_point": med["batch"] * 1e3 / N,
           # p, ftay, sigma0 (8 B each) and the class (4 B), read by each of the pass's two sweeps
           "new_pass_bytes_per_row": 28 * 2 + (48 if bt.is_wideband else 0),
           "set_points_bytes_per_point": 8 * (lay.tstride + 2 * len(names))}
    bt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    import golden_util
    from pint_amd import get_model
    from test_bayesian import load
    res = []
    model, toas, z, meta = load("bayes_nb")
    res.append(measure("bayes_nb", model, toas, meta["prior_info"], 4096, a.reps, a.warm))
    res[-1]["reference_ms_per_point"] = meta["ref_seconds_per_lnlikelihood"] * 1e3
    _, toas, _, _ = golden_util.load("c5_ell1")
    par = open(os.path.join(golden_util.GOLDEN, "c5_ell1.par")).read()
    model = get_model("\n".join(l for l in par.splitlines() if not l.upper().startswith("TNRED")) + "\n")
    free = [p for p in model.free_params]
    pi = {}
    for p in free:
        v = float(model[p].value)
        w = max(abs(v) * 1e-6, 1e-12)
        pi[p] = {"distr": "uniform", "pmin": v - w, "pmax": v + w}
    res.append(measure("c5_ell1_10k", model, toas, pi, 256, a.reps, a.warm))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
