"""What a batch of the photon-event passes costs, beside the floor the parent could already run on the
same shape: pint_set_points + pint_eval(0).  Two shapes: N = 4096 points of the 1500-photon photon_geo
fixture (thousands of small points) and N = 256 points of a 100,000-photon synthetic pulsar (the same
model, photons spread uniformly over its span at the barycentre, 256-bin template, weighted).

Each figure is the median of REPS host-clock windows around calls that end in a device synchronise
(the Session is not lazy), after WARM warm-up rounds, the variants alternating inside one round:

  floor      set_points + eval                          (what the parent runs)
  lnlike     floor + point_photon_lnlike, one offset    (the difference to floor: k_photon_lnl)
  scan64     floor + point_photon_lnlike, 64 offsets
  trig20     floor + point_photon_trig(20)              (the difference to floor: k_photon_trig<24>)
  trig64     floor + point_photon_trig(64)              (k_photon_trig<64>)
  readback   floor + read_eval                          (what a user without the passes does: 16 B per photon
                                                         and point over the host link, before any numpy)
  batch      PhotonTiming.lnlikelihood_batch            (lnlike plus the host's share)
  htest      PhotonTiming.htest_batch(m=20)

and the bytes each pass reads per photon and point.  One JSON line on stdout.

Usage: python scripts/diag/photon_cost.py [--reps 20] [--warm 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LD = np.longdouble


def measure(tag, model, toas, tmpl, weights, N, reps, warm, readback=True):
    from pint_amd import PhotonTiming
    pt = PhotonTiming(model, toas, tmpl, weights=weights)
    s, lay = pt._device(), pt.lay
    rng = np.random.default_rng(5)
    base = pt._base_values
    pts = np.tile(base, (N, 1))
    for j in range(pt.nparams - 1):
        pts[:, j] += abs(base[j]) * LD(1e-12) * rng.uniform(-1, 1, N).astype(LD)
    pts[:, -1] = rng.uniform(0, 1, N)
    phs1 = np.asarray(pts[:, -1], dtype=np.float64)
    phs64 = np.tile(np.arange(64) / 64.0, (N, 1))

    def floor():
        pt._eval_points(s, pts)
        s.L.pint_sync(s.ctx)

    def with_(fn):
        def run():
            pt._eval_points(s, pts)
            fn()
        return run

    variants = {"floor": floor, "lnlike": with_(lambda: s.point_photon_lnlike(phs1)),
                "scan64": with_(lambda: s.point_photon_lnlike(phs64)), "trig20": with_(lambda: s.point_photon_trig(20)),
                "trig64": with_(lambda: s.point_photon_trig(64)), "batch": lambda: pt.lnlikelihood_batch(pts),
                "htest": lambda: pt.htest_batch(pts, m=20)}
    if readback:
        variants["readback"] = with_(lambda: s.L.pint_read_eval(s.ctx, *hold))
        bufs = [np.empty(N * (lay.n + 1)) for _ in range(2)]  # phase hi and lo of every row
        hold = [b.ctypes.data_as(C.POINTER(C.c_double)) for b in bufs] + [None, None]
    t = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= warm:
                t[k].append(dt * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    w = weights is not None
    out = {"shape": tag, "nphotons": lay.n, "npoints": N, "nbin": len(tmpl), "weighted": w, "ms": med,
           "ms_iqr": {k: float(np.subtract(*np.percentile(v, [75, 25]))) for k, v in t.items()},
           "pass_minus_floor_ms": {k: med[k] - med["floor"] for k in med if k != "floor"},
           "us_per_point_batch": med["batch"] * 1e3 / N,
           # phase hi and lo (and the weight) per photon, once per tile of 8 offsets / once per trig call
           "bytes_per_photon_point": {"lnlike": 24 if w else 16, "scan64": 8 * (24 if w else 16), "trig": 24 if w else 16,
                                      "readback": 16}}
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    from photon_util import load, spread
    from pint_amd import get_event_TOAs
    res = []
    model, toas, z, meta = load("photon_geo")
    res.append(measure("photon_geo", model, toas, z["tmpl"], z["weights"], 4096, a.reps, a.warm))
    res[-1]["reference_ms_per_point"] = spread()["photon_geo"]["ref_seconds_per_lnposterior"] * 1e3
    rng = np.random.default_rng(7)
    n = 100_000
    mjds = np.sort(rng.uniform(53000.0, 56652.0, n)).astype(LD)
    big = get_event_TOAs(mjds, timesys="TDB", obs="barycenter", model=model)
    res.append(measure("synthetic_100k", model, big, z["tmpl"], rng.beta(1.2, 1.6, n), 256, a.reps, a.warm))
    # the reference's time scales with the photon count (its phase evaluation and np.interp are per photon)
    res[-1]["reference_ms_per_point_scaled"] = res[0]["reference_ms_per_point"] * n / 1500.0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
