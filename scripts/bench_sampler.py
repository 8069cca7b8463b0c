#!/usr/bin/env python
"""Steps per second of the ensemble sampler (pint_amd/sampler.py): (a) the device-resident path
against (b) the host-stepped mode -- the same algorithm and random numbers, each half-step one
``target.lnposterior_batch`` call from numpy, which is what a generic vectorised sampler would do with
this package -- on a narrowband and a wideband BayesianTiming target of 300 TOAs (the bayes_nb and
bayes_wb fixtures) and a PhotonTiming target of 1500 photons (photon_geo), at 64, 512 and 4096 walkers.

Timing: a warm-up run of the same shape, then the wall time of ``run_mcmc`` over --steps steps (it
returns after the chain was read back, so the device work is complete), the median of --reps runs.

    python scripts/bench_sampler.py [--steps 200] [--reps 5] [--walkers 64,512,4096] [--json out.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble


def fixture(name):
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
    fc = dict(meta["flag_columns"])
    if "wb_pp_dm" in z:
        fc["pp_dm"] = [repr(float(x)) for x in z["wb_pp_dm"]]
        fc["pp_dme"] = [repr(float(x)) for x in z["wb_pp_dme"]]
    toas = from_arrays_with_tzr(z, fc, name, meta.get("obs_names"))
    model = get_model(os.path.join(GOLDEN, name + ".par"))
    model.free_params = list(meta["model"]["free_params"])
    return model, toas, z, meta


def make_target(name):
    """(target, the fixture's points in the target's column order)."""
    from pint_amd import BayesianTiming, PhotonTiming
    model, toas, z, meta = fixture(name)
    if name.startswith("photon"):
        t = PhotonTiming(model, toas, z["tmpl"], weights=z.get("weights"), prior_info=meta["prior_info"])
    else:
        t = BayesianTiming(model, toas, prior_info=meta["prior_info"])
    perm = [meta["labels"].index(p) for p in t.param_labels]
    return t, (z["pts_hi"].astype(LD) + z["pts_lo"].astype(LD))[:, perm]


def start(pts, W, seed=0, width=0.2):
    c, s = pts.mean(axis=0), pts.astype(np.float64).std(axis=0)
    return c + (width * s * np.random.default_rng(seed).standard_normal((W, pts.shape[1]))).astype(LD)


def rate(target, pos, W, resident, steps, reps):
    from pint_amd import EnsembleSampler
    s = EnsembleSampler(target, W, seed=1, resident=resident)
    s.run_mcmc(pos, max(steps // 10, 5))  # warm-up: every launch of the timed shape
    times = []
    for _ in range(reps):
        s.reset()
        s.run_mcmc(pos, 0)  # (the start's evaluation is not part of a step)
        t0 = time.perf_counter()
        s.run_mcmc(None, steps)
        times.append(time.perf_counter() - t0)
    acc = float(np.mean(s.acceptance_fraction))
    s.close()
    return steps / float(np.median(times)), acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walkers", default="64,512,4096")
    ap.add_argument("--targets", default="bayes_nb,bayes_wb,photon_geo")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)
    rows = []
    print("| target | walkers | resident steps/s | host-stepped steps/s | ratio | acceptance |")
    print("|---|---|---|---|---|---|")
    for name in a.targets.split(","):
        target, pts = make_target(name)
        for W in (int(w) for w in a.walkers.split(",")):
            pos = start(pts, W)
            r, acc = rate(target, pos, W, True, a.steps, a.reps)
            h, _ = rate(target, pos, W, False, a.steps, a.reps)
            rows.append({"target": name, "walkers": W, "resident_steps_per_s": r, "host_steps_per_s": h,
                         "ratio": r / h, "acceptance": acc, "steps": a.steps, "reps": a.reps})
            print(f"| {name} | {W} | {r:.0f} | {h:.1f} | {r / h:.1f} | {acc:.2f} |", flush=True)
        target.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
