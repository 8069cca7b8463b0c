"""pint_set_instances as plan, refuse or commit (plan_batch / commit_batch, pint_hip.hip).

Three properties of the batch set-up that the sweeps do not reach:

* a refused call (a pulsar id outside the context) leaves the resident batch as it was;
* a pulsar's k_gram_v layout follows the batch it is in, not the batches that came before: the
  per-pulsar records (row tiles, slot count, the rows' slot ids on the device) are shared by all
  batches of a context and re-formed whenever the layout changes;
* pint_set_grid's reuse of the resident batch (PINT_QUERY_NREUSE) gives what a fresh batch gives.

The pulsars are shape_cases' synthetic models on its 530-TOA set, fit layout, PINT_NSPLIT = 1.
"""
import numpy as np
import pytest

import shape_cases as SC

pytestmark = pytest.mark.gpu

# P: Offset, F0, F1 beside 8 free DMX bins (the fewest the compact layout takes) and 2 red-noise
# modes: [T | r] is 4 columns wide, so one row tile holds it with 12 DMX slots (8 bins, distinct
# mod 12).  Q: 16 timing columns (the fewest whose [T | r], 17 wide, needs a second row tile),
# the same bins and modes: 15 slots.
P = SC.Case("P", 3, 8, 2, layout="fit")
Q = SC.Case("Q", 16, 8, 2, layout="fit")


@pytest.fixture(scope="module")
def toas():
    from pint_amd.simulation import make_fake_toas_batch
    base = SC.model_of(SC.Case("base", 8, SC.BASE_NDMX, 30))
    return make_fake_toas_batch([dict(model=base, start=SC.MJD0, end=SC.MJD1, ntoas=530, freq=[800, 1200, 1600, 2000],
                                      obs="geocenter", error_us=0.5, add_noise=True, seed=630)])[0]


def run_step(s):
    """eval for a fit, the residuals and their chi2, one GLS step: everything as copies."""
    from pint_amd.engine import Session
    s.eval(want_M=Session.FIT)
    tr, _, c2 = s.read_resids()
    s.fit_step(1)
    dp, er, _, cl = s.read_step()
    return dict(resid=[np.array(x) for x in tr], chi2=np.array(c2), step=[np.array(x) for x in dp],
                errs=[np.array(x) for x in er], chi2lin=np.array(cl), chi2_gls=np.array(s.chi2_gls()),
                plan=s.last_plan(), nsplit=s.nsplit(), nvgram=s.n_vgram())


def assert_same(a, b):
    assert a["plan"] == b["plan"] and a["nsplit"] == b["nsplit"] and a["nvgram"] == b["nvgram"]
    for k in ("resid", "step", "errs"):
        for x, y in zip(a[k], b[k]):
            np.testing.assert_array_equal(x, y, err_msg=k)
    for k in ("chi2", "chi2lin", "chi2_gls"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_refused_set_instances_leaves_the_batch(toas, monkeypatch):
    """pint_set_instances naming a pulsar id one past the last returns PINT_E_INVALID ("bad pulsar
    id") with the context unchanged: without setting a batch again, evaluation, residuals, chi2,
    fit step, split count, k_gram_v instances and plan are those of before, bit for bit.

    Before the batch set-up planned first, the refusal came after the resident batch had been
    freed (ninst 0), and the second pint_eval here failed with PINT_E_INVALID."""
    import ctypes as C
    from pint_amd import _lib
    from pint_amd.engine import Session, build_layout, pack_table
    monkeypatch.setenv("PINT_NSPLIT", "1")
    s = Session()
    try:
        lay = s.add(build_layout(SC.model_of(P), toas, track_mode="nearest"))
        tab = pack_table(lay)
        s.set_instances([(lay, tab)])
        first = run_step(s)
        assert first["nvgram"] == 1 and first["plan"]["gram_v"]
        vg = s.vgram_layout(lay)
        ids = np.array([lay.psr_id, lay.psr_id + 1], dtype=np.int32)
        tabs = np.ascontiguousarray(np.concatenate([tab, tab]))
        rc = s.L.pint_set_instances(s.ctx, 2, _lib.ptr(ids, C.c_int32), _lib.ptr(tabs))
        assert rc == _lib.PINT_E_INVALID
        assert s.L.pint_last_error(s.ctx).decode() == "bad pulsar id"
        assert s.vgram_layout(lay) == vg
        assert_same(run_step(s), first)
    finally:
        s.close()


def test_layout_follows_the_batch_not_the_history(toas, monkeypatch):
    """Batches A = [P], B = [P, Q], A again in one Session.  Both batches are latency-bound, so
    every k_gram_v pulsar takes the largest row-tile count any of the batch needs: P alone takes
    one row tile (12 slots, key 10 (1 - 1) + 2 = 2: [T | r | slots] 16 wide + 4 Fourier columns
    = 32), beside Q two (28 slots, key 10 (2 - 1) + 3 = 13, with Q: 48 wide), and one again in
    the second A -- its rows' slot ids re-formed and uploaded at each change.

    P: ntim 3, ndmx 8, nred 2 (red0c + 1 = 4); Q: ntim 16, ndmx 8, nred 2 (red0c + 1 = 17).
    Observed on an MI355X: keys as last_plan() reports them A ((2, True),), B ((13, True),), A again
    ((2, True),); P's vgram_layout() (1, 12, 32, 3) in A, (3, 28, 48, 3) in B (28 slots leave an
    all-slot row tile: the binned DMX x Fourier body as well); P in B against P in A: step 2.5e-13
    sigma, errors 2.0e-15, chi2 1.8e-15 relative.

    The second A equals the first bit for bit (plan and outputs).  In B a different tile shape
    sums in another order, and the batch carries Q's WaveX pass: P's step, errors and chi2 agree
    with A's to test_shape_sweep's bars for them -- step 1e-9 sigma, errors and chi2 1e-9
    relative."""
    from pint_amd.engine import Session, build_layout, pack_table
    monkeypatch.setenv("PINT_NSPLIT", "1")
    n, mjd = toas.ntoas, toas.arrays["mjd_float"]
    for c, (ntr, ns) in ((P, (1, 12)), (Q, (2, 15))):  # the cases are what the docstring says
        assert SC.vgram_layout(c, n, SC.free_rows(c, mjd), 1)[:3] == (1, ntr, ns)
    s = Session()
    try:
        lp = s.add(build_layout(SC.model_of(P), toas, track_mode="nearest"))
        lq = s.add(build_layout(SC.model_of(Q), toas, track_mode="nearest"))
        tp, tq = pack_table(lp), pack_table(lq)
        s.set_instances([(lp, tp)])
        a1 = run_step(s)
        vg_a = s.vgram_layout(lp)
        s.set_instances([(lp, tp), (lq, tq)])
        b = run_step(s)
        vg_b = s.vgram_layout(lp)
        s.set_instances([(lp, tp)])
        a2 = run_step(s)
        vg_a2 = s.vgram_layout(lp)
    finally:
        s.close()
    print("k_gram_v keys: A", a1["plan"]["gram_v"], "B", b["plan"]["gram_v"], "layouts of P:", vg_a, vg_b, vg_a2)
    assert a1["nvgram"] == 1 and b["nvgram"] == 2
    keys_a = {k for k, _ in a1["plan"]["gram_v"]}
    keys_b = {k for k, _ in b["plan"]["gram_v"]}
    assert keys_a == {2} and keys_b == {13}
    assert not (keys_a & keys_b)
    assert vg_a != vg_b and vg_a2 == vg_a
    assert_same(a2, a1)
    sig = a1["errs"][0]
    e_step = float(np.max(np.abs(b["step"][0] - a1["step"][0])[:lp.K] / sig[:lp.K]))
    e_errs = float(np.max(np.abs(b["errs"][0][:lp.K] / sig[:lp.K] - 1)))
    e_chi2 = max(float(abs(b[k][0] / a1[k][0] - 1)) for k in ("chi2", "chi2lin", "chi2_gls"))
    print(f"P in B against P in A: step {e_step:.1e} sigma, errors {e_errs:.1e}, chi2 {e_chi2:.1e}")
    assert e_step <= 1e-9 and e_errs <= 1e-9 and e_chi2 <= 1e-9


def test_reused_grid_batch_equals_a_fresh_one():
    """Two pint_set_grid calls of equal shape on one session, the second on the reuse branch
    (PINT_QUERY_NREUSE goes up by one) after an evaluation, a chi2 read and a fit step on the
    first: the chi2 of all its 221 points, and a WLS step's linearised chi2, equal bit for bit
    those of a fresh session given the second grid alone (NGC6440E)."""
    from golden_util import load
    from pint_amd.engine import Session, build_layout, pack_table
    from pint_amd.gridutils import meshgrid_axes
    model, toas_n, _, _ = load("ngc6440e")
    LD = np.longdouble
    F0, F1 = LD(model.F0.value), LD(model.F1.value)

    def grid(lo0, lo1):
        g0 = F0 + np.linspace(lo0, lo0 + 6, 17, dtype=LD) * LD(1e-11)
        g1 = F1 + np.linspace(lo1, lo1 + 6, 13, dtype=LD) * LD(1e-19)
        axes, npts = meshgrid_axes((g0, g1))
        return [(p, a, st, sz) for p, (a, st, sz) in zip(("F0", "F1"), axes)], npts

    def run(grids):
        s = Session()
        try:
            lay = s.add(build_layout(model, toas_n))
            base = pack_table(lay, model)
            for var, npts in grids:
                before = s.n_batch_reuse()
                s.set_grid(lay, base, var, npts)
                reused = s.n_batch_reuse() - before
                s.eval(want_M=True)
                c2 = np.array(s.read_resids()[2])
                s.fit_step(0)
                cl = np.array(s.read_step()[3])
            return c2, cl, reused
        finally:
            s.close()

    ga, gb = grid(-3, -3), grid(-2, -4)
    assert ga[1] == gb[1] == 221
    c_res, l_res, reused = run([ga, gb])
    assert reused == 1
    c_new, l_new, reused = run([gb])
    assert reused == 0
    assert np.all(np.isfinite(c_new)) and len(c_new) == 221 and len(set(c_new.tolist())) > 200
    np.testing.assert_array_equal(c_res, c_new)
    np.testing.assert_array_equal(l_res, l_new)
