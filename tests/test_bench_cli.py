"""bench.py's command line on the GPU, at a small shape (4 pulsars x 2000 TOAs): a plain run
times exactly --steps steps, runs none of the --full legs, and --dump-outputs writes the last
timed step's fit outputs, which are those of the same step made call by call in this
process (the synchronous Session path the fitters use).

Tolerances.  Both sides run the same kernels on the same inputs; they differ only in the
order of floating-point reductions that use atomics (FP64, ~1e-16 per term).  chi2 is a sum
of ~2000 positive terms: 1e-9 relative is far above that.  The parameter steps pass through
the Cholesky solve of a normal matrix whose condition number multiplies the rounding, so
they are compared in units of the fit's own 1-sigma errors: 1e-6 sigma."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPSR, NTOAS, STEPS, WARMUP = 4, 2000, 3, 1


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--npsr", str(NPSR), "--ntoas", str(NTOAS),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), d, p.stderr


@pytest.mark.gpu
def test_plain_run_result_line(plain_run):
    res, _, err = plain_run
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["full"] is False
    assert res["unit"] == "fits/s" and res["higher_is_better"] is True and res["dtype"] == "f64+dd"
    assert res["ms_per_step"] > 0
    # value = pulsars per second of one step (both rounded in the line)
    assert res["value"] == pytest.approx(NPSR / (res["ms_per_step"] * 1e-3), rel=1e-3)
    for leg in ("roofline", "pta_weak", "predicted_strong", "cold_start", "grid", "j0740", "c2", "cpu_baseline"):
        assert res[leg] is None, leg
    assert "[emulate" not in err and "cold start" not in err


@pytest.mark.gpu
def test_dump_is_the_step_a_caller_receives(plain_run):
    from pint_amd import simulation as sim
    from pint_amd.engine import Session, pack_table
    _, d, _ = plain_run
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert {"steps", "errors", "covariances", "chi2_linearised", "chi2", "pl_red_noise"} <= set(got)
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    items = sim.make_pta(npsr=NPSR, ntoas=NTOAS)
    s = Session()
    try:
        lays = s.add_all(items)
        s.set_instances([(l, pack_table(l, m)) for l, (m, _) in zip(lays, items)])
        s.eval(want_M=Session.FIT)
        s.fit_step_apply(1, 1.0)
        dp, er, covs, cl = s.read_step()
        nz = s.noise_resids()
        s.eval(want_M=False)
        c2 = s.chi2_gls()
        s.check()
        steps, errors = np.concatenate(list(dp)), np.concatenate(list(er))
        cov = np.concatenate([c.ravel() for c in covs])
        red = np.concatenate([d_["pl_red_noise"] for d_ in nz if "pl_red_noise" in d_])
        c2, cl = np.array(c2), np.array(cl)
    finally:
        s.close()
    assert got["steps"].shape == steps.shape and got["covariances"].shape == cov.shape
    np.testing.assert_allclose(got["chi2"], c2, rtol=1e-9)
    assert got["chi2_linearised"].shape == cl.shape and got["errors"].shape == errors.shape
    ok = errors > 0
    assert ok.sum() > NPSR * 10
    assert np.max(np.abs(got["steps"] - steps)[ok] / errors[ok]) < 1e-6
    assert got["pl_red_noise"].shape == red.shape
