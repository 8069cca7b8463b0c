"""What the polyco calls cost, beside the photon-event path on the same photons and the reference.

Steps (each a fresh child process under its own time limit; the run stops at the first that fails):

  fit     pint_polyco_fit_host, 10^4 segments of 20 nodes and 12 coefficients (synthetic phases)
  eval    pint_polyco_eval (the phase), N = 10^7 barycentric times inside the poly_bary fixture's table
  trig    pint_polyco_trig(m = 20) on the same times, unweighted and weighted
  events  the same N photons through get_event_TOAs + PhotonTiming.htest_batch (one point), the host's
          preparation included; its parts are reported too

Each figure is the median of REPS host-clock windows around calls that end in a device synchronise (the
polyco calls synchronise before they return), after WARM warm-up calls.  The windows of eval and trig
contain the host-to-device copy of the times (and the read-back of eval's phases): the calls take host
arrays.  Beside the times: the bytes per time each call moves, the rate that makes, its fraction of the
6.29 TB/s copy rate, and the reference's seconds from the fixtures (per generate_polycos segment, per
10^5 eval_abs_phase times).  One JSON line on stdout.

Usage: python scripts/diag/polyco_cost.py [--reps 7] [--warm 2] [--n 10000000] [--steps fit,eval,trig,events]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LD = np.longdouble
COPY_RATE = 6.29e12  # B/s, the measured device copy rate
LIMITS = {"fit": 120, "eval": 240, "trig": 300, "events": 600}  # seconds per step


def windows(fn, reps, warm):
    t = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warm:
            t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(t)), "ms_iqr": float(np.subtract(*np.percentile(t, [75, 25])))}


def rate(res, nbytes, n):
    res["bytes_per_time"] = nbytes
    res["GB_per_s"] = nbytes * n / (res["ms"] * 1e-3) / 1e9
    res["fraction_of_copy_rate"] = nbytes * n / (res["ms"] * 1e-3) / COPY_RATE
    res["ns_per_time"] = res["ms"] * 1e6 / n
    return res


def table_and_times(n):
    from test_polycos import load, pair, table_from
    z, meta = load("poly_bary")
    p = table_from(z, meta)
    rng = np.random.default_rng(3)
    a, b = float(p["t_start"][0]) + 1e-6, float(p["t_stop"][-1]) - 1e-6
    t = np.sort(rng.uniform(a, b, n))
    return p, z, meta, t


def step_fit(a):
    from pint_amd.engine import Session
    nseg, nn, nc = 10_000, 20, 12
    rng = np.random.default_rng(1)
    x = np.linspace(-30.0, 30.0, nn)
    u = x / 30.0
    y = 0.3 * np.sin(2.1 * u[None, :] + rng.uniform(0, 6, (nseg, 1))) + 1e-9 * rng.standard_normal((nseg, nn))
    ph = np.zeros(nseg * (nn + 1) + 1)
    ph[:-1].reshape(nseg, nn + 1)[:, :nn] = y
    dt = np.tile(x, (nseg, 1))
    s = Session()
    try:
        res = windows(lambda: s.polyco_fit_host(nseg, nn, nc, ph, np.zeros_like(ph), dt, np.zeros_like(dt), 0.0), a.reps, a.warm)
    finally:
        s.close()
    res.update(nseg=nseg, nnode=nn, ncoeff=nc, us_per_segment=res["ms"] * 1e3 / nseg)
    return res


def step_eval(a):
    p, z, meta, t = table_and_times(a.n)
    s = p._device()
    lo = np.zeros_like(t)
    res = rate(windows(lambda: s.polyco_eval(t, lo, 1), a.reps, a.warm), 32, a.n)  # 16 B in, 16 B out
    res.update(n=a.n, reference_s_per_1e5=meta["ref_seconds_per_1e5_eval"],
               reference_ms_scaled=meta["ref_seconds_per_1e5_eval"] * a.n / 1e5 * 1e3)
    return res


def step_trig(a):
    p, z, meta, t = table_and_times(a.n)
    s = p._device()
    lo = np.zeros_like(t)
    w = np.random.default_rng(4).beta(1.2, 1.6, a.n)
    out = {"unweighted": rate(windows(lambda: s.polyco_trig(t, lo, None, 20), a.reps, a.warm), 16, a.n),
           "weighted": rate(windows(lambda: s.polyco_trig(t, lo, w, 20), a.reps, a.warm), 24, a.n), "n": a.n, "m": 20}
    t0 = time.perf_counter()
    H, _ = p.htest(t, m=20)
    out["htest_ms"] = (time.perf_counter() - t0) * 1e3
    out["H"] = float(H)
    return out


def step_events(a):
    import warnings
    from pint_amd import PhotonTiming, get_event_TOAs, get_model
    from pint_amd.polycos import Polycos
    p, z, meta, t = table_and_times(a.n)
    model = get_model(os.path.join(ROOT, "tests", "golden", "poly_bary.par"))
    Polycos._add_tzr(model, p["tmid"][0])  # (the TZR the polycos were generated with)
    model.free_params = ["F0"]
    out = {"n": a.n}
    t0 = time.perf_counter()
    toas = get_event_TOAs(t.astype(LD), timesys="TDB", obs="barycenter", model=model)
    out["prepare_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pt = PhotonTiming(model, toas, None)
        pts = np.asarray(pt._base_values, dtype=LD)[None, :]
        H, _ = pt.htest_batch(pts, m=20)
    out["upload_and_first_htest_ms"] = (time.perf_counter() - t0) * 1e3
    out["htest_batch"] = windows(lambda: pt.htest_batch(pts, m=20), a.reps, a.warm)
    out["total_first_answer_ms"] = out["prepare_ms"] + out["upload_and_first_htest_ms"]
    out["H"] = float(np.ravel(H)[0])
    pt.close()
    return out


STEPS = {"fit": step_fit, "eval": step_eval, "trig": step_trig, "events": step_events}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--steps", default="fit,eval,trig,events")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(STEPS[a.child](a)))
        return
    res = {}
    for name in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warm", str(a.warm),
               "--n", str(a.n)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            res[name] = {"error": f"time limit of {LIMITS[name]} s"}
            break
        if r.returncode != 0:
            res[name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    from test_polycos import load
    res["reference_s_per_segment"] = {c: load(c)[1]["ref_seconds_per_segment"] for c in ("poly_bary", "poly_gbt", "poly_short", "poly_long")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
