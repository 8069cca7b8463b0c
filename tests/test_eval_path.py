"""What pint_eval launched, as its plan reports it (plan_eval, pint_hip.hip).

Session.eval_path() and Session.eval_kinds() report the decisions of the last evaluation: where
the per-instance constants came from, k_sw_geom, the spin pass, the merged launch, the block
kinds with a launch of their own, and the builds at a fixed register budget.  Every case states
both words exactly.  Where two runs are compared, the paths are asserted to differ first; then
phases, delays, Taylor factors, design matrix, residuals and chi2 are equal bit for bit.

All on the golden fixtures; the batches are the smallest that reach each branch.
"""
import numpy as np
import pytest

from golden_util import load

pytestmark = pytest.mark.gpu

PREP_LANE_TAB = 64  # k_prep_lanes takes a batch whose longest table has at most this many doubles
EF_ROWS = 254       # rows per evaluation block with the residual pass's first half fused in (256 without)
ISO, ELL1, DD, ELL1H = 1 << 0, 1 << 1, 1 << 2, 1 << 3  # eval_kinds() bits (PINT_BIN_*)


def prep_bit(S, lays):
    """The k_prep form of a batch of these layouts (prep_lanes, pint_hip.hip)."""
    return S.EVAL_PREP_LANES if max(l.tstride for l in lays) <= PREP_LANE_TAB else S.EVAL_PREP


def path(s):
    return s.eval_path(), s.eval_kinds()


def outputs(s):
    """Everything the last eval(want_M) wrote, as copies: phases (hi, lo), Taylor factors, delays,
    the design matrix, time and phase residuals, chi2."""
    out = [np.concatenate(x).copy() for x in s.read_eval()]
    out += [x.copy() for x in s.read_designmatrix()]
    tr, pr, c2 = s.read_resids()
    return out + [np.concatenate(tr).copy(), np.concatenate(pr).copy(), np.array(c2, copy=True)]


def assert_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def batch(s, names):
    """A session's batch of one instance per fixture; the layouts."""
    from pint_amd.engine import build_layout, pack_table
    items = [load(n)[:2] for n in names]
    lays = [s.add(build_layout(m, t)) for m, t in items]
    s.set_instances([(l, pack_table(l, m)) for l, (m, _) in zip(lays, items)])
    return lays


def test_source_of_the_constants(monkeypatch):
    """Three NGC6440E instances (tables of at most 64 doubles): the first evaluation forms the
    constants with k_prep_lanes, or k_prep under PINT_PREP_LANES=0; a second evaluation with
    nothing changed, and one after apply_step_uniform (k_apply refreshed them), launch neither.
    One isolated model: its own launch at the register budget throughout."""
    from pint_amd.engine import Session as S

    def run(lanes):
        monkeypatch.setenv("PINT_PREP_LANES", str(lanes))
        s = S()
        try:
            lays = batch(s, ["ngc6440e"] * 3)
            assert max(l.tstride for l in lays) <= PREP_LANE_TAB
            s.eval(want_M=True)
            paths = [path(s)]
            out = outputs(s)
            s.eval(want_M=True)
            paths.append(path(s))
            s.fit_step(0)
            s.apply_step_uniform(1.0)
            s.eval(want_M=True)
            paths.append(path(s))
            return paths, out + outputs(s)
        finally:
            s.close()

    (pa, a), (pb, b) = run(1), run(0)
    same = (S.EVAL_KIND_BUDGET, ISO)
    assert pa == [(S.EVAL_PREP_LANES | S.EVAL_KIND_BUDGET, ISO), same, same], pa
    assert pb == [(S.EVAL_PREP | S.EVAL_KIND_BUDGET, ISO), same, same], pb
    assert_equal(a, b)


def test_restore_reads_the_snapshot():
    """save_tables, a GLS step, its apply, restore_tables, then the evaluation in the fit layout:
    it reads the snapshot and writes it back itself, without k_prep, and gives the first
    evaluation's outputs bit for bit -- which are those of a fresh session on the same tables,
    whose evaluation ran k_prep.

    The fit layout leaves the design-matrix buffer's DMX and generated-Fourier columns unwritten
    (they live in the bin sums and in k_gram_v), so across sessions those entries hold whatever
    the allocation held: there the design matrix is compared through the GLS step that reads it
    (step, errors, covariance, linearised chi2, bit for bit); within the session the whole buffer
    is compared as well."""
    from pint_amd.engine import Session as S
    names = ["pta_dd", "pta_ell1", "pta_iso"]
    nM = len(names)  # outputs(): four evaluation arrays, then one design matrix per instance

    def step(s):
        s.fit_step(1)
        dp, er, cov, cl = s.read_step()
        return [x.copy() for x in dp] + [x.copy() for x in er] + [x.copy() for x in cov] + [np.array(cl, copy=True)]

    def run(refit):
        s = S()
        try:
            lays = batch(s, names)
            s.eval(want_M=S.FIT)
            first = path(s), outputs(s)
            if not refit:
                return lays, first + (step(s),)
            s.save_tables()
            s.fit_step(1)
            s.apply_step_uniform(1.0)
            s.restore_tables()
            s.eval(want_M=S.FIT)
            return lays, first, (path(s), outputs(s), step(s))
        finally:
            s.close()

    lays, (p1, o1), (p2, o2, s2) = run(True)
    _, (p3, o3, s3) = run(False)
    prep = prep_bit(S, lays)
    assert p1 == p3 == (prep | S.EVAL_MERGED, 0), (p1, p3)
    assert p2 == (S.EVAL_SNAPSHOT | S.EVAL_MERGED, 0), p2
    assert_equal(o2, o1)
    assert_equal(o2[:4] + o2[4 + nM:], o3[:4] + o3[4 + nM:])
    assert_equal(s2, s3)


def ngc_grid(lo0, lo1):
    """test_batch_layout's 17 x 13 F0 x F1 grid of NGC6440E: (model, toas, variables, npts)."""
    from pint_amd.gridutils import meshgrid_axes
    model, toas = load("ngc6440e")[:2]
    LD = np.longdouble
    g0 = LD(model.F0.value) + np.linspace(lo0, lo0 + 6, 17, dtype=LD) * LD(1e-11)
    g1 = LD(model.F1.value) + np.linspace(lo1, lo1 + 6, 13, dtype=LD) * LD(1e-19)
    axes, npts = meshgrid_axes((g0, g1))
    assert npts == 221
    return model, toas, [(p, a, st, sz) for p, (a, st, sz) in zip(("F0", "F1"), axes)], npts


def test_spin_pass(monkeypatch):
    """A spin-only grid's first evaluation with the design matrix takes the shared head and the
    spin part, and no block kind is launched; once a step is applied the isolated kind has its
    launch again.  PINT_SPIN_EVAL=0 takes that form from the first evaluation on and gives equal
    outputs."""
    from pint_amd.engine import Session as S, build_layout, pack_table
    model, toas, var, npts = ngc_grid(-3, -3)

    def run(spin):
        monkeypatch.setenv("PINT_SPIN_EVAL", str(spin))
        s = S()
        try:
            lay = s.add(build_layout(model, toas))
            s.set_grid(lay, pack_table(lay, model), var, npts)
            s.eval(want_M=True)
            p1, out, n1 = path(s), outputs(s), s.n_spin_eval()
            s.fit_step(0)
            s.apply_step_uniform(1.0)
            s.eval(want_M=True)
            return prep_bit(S, [lay]), p1, path(s), out, (n1, s.n_spin_eval())
        finally:
            s.close()

    prep, a1, a2, a, na = run(1)
    _, b1, b2, b, nb = run(0)
    assert a1 == (prep | S.EVAL_SPIN, 0), a1
    assert a2 == b2 == (S.EVAL_KIND_BUDGET, ISO), (a2, b2)
    assert b1 == (prep | S.EVAL_KIND_BUDGET, ISO), b1
    assert na == (1, 1) and nb == (0, 0)
    assert_equal(a, b)


def test_merged_or_per_kind(monkeypatch):
    """A DD, an ELL1 and an isolated pulsar: one merged launch (well under 512 blocks: not the
    budget build) and no kind of its own; PINT_EVAL_MERGE=0 launches the three kinds (the isolated
    one at its budget) and gives equal outputs.  With an ELL1H pulsar beside them the merged launch
    stays and ELL1H alone has its own."""
    from pint_amd.engine import Session as S
    names = ["pta_dd", "pta_ell1", "pta_iso"]

    def run(merge, more=()):
        if merge is not None:
            monkeypatch.setenv("PINT_EVAL_MERGE", str(merge))
        s = S()
        try:
            lays = batch(s, names + list(more))
            s.eval(want_M=True)
            return prep_bit(S, lays), path(s), outputs(s)
        finally:
            s.close()

    prep, pa, a = run(None)
    _, ph, _ = run(None, ["ell1h_h3"])
    _, pb, b = run(0)
    assert pa == (prep | S.EVAL_MERGED, 0), pa
    assert pb == (prep | S.EVAL_KIND_BUDGET, ISO | ELL1 | DD), pb
    assert ph == (prep | S.EVAL_MERGED, ELL1H), ph
    assert_equal(a, b)


def test_merged_register_budget_build(monkeypatch):
    """k_eval_mix_w<1, 3> needs more than 512 evaluation blocks of two kinds with the design
    matrix: the fewest 10k-row J0740 (ELL1) instances that pass 512 blocks beside one isolated
    pulsar, against PINT_EVAL_WPE=0's unconstrained merged build on the same batch."""
    from pint_amd.engine import Session as S, build_layout, pack_table
    (mj, tj), (mi, ti) = load("j0740_10k")[:2], load("pta_iso")[:2]
    # no pass follows these models' evaluation and the batch is off the small-instance path, so the
    # residual pass's first half rides in the evaluation's blocks: EF_ROWS rows each
    bj, bi = -(-tj.ntoas // EF_ROWS), -(-ti.ntoas // EF_ROWS)
    k = (2 * 256 - bi) // bj + 1
    assert (k - 1) * bj + bi <= 2 * 256 < k * bj + bi

    def run(wpe):
        monkeypatch.setenv("PINT_EVAL_WPE", str(wpe))
        s = S()
        try:
            lj, li = s.add(build_layout(mj, tj)), s.add(build_layout(mi, ti))
            s.set_instances([(lj, pack_table(lj, mj))] * k + [(li, pack_table(li, mi))])
            s.eval(want_M=True)
            assert s.resid_path() & S.RESID_EFUSED  # (the block count above)
            return prep_bit(S, [lj, li]), path(s), outputs(s)
        finally:
            s.close()

    prep, pa, a = run(3)
    _, pb, b = run(0)
    assert pa == (prep | S.EVAL_MERGED | S.EVAL_MERGED_BUDGET, 0), pa
    assert pb == (prep | S.EVAL_MERGED, 0), pb
    assert_equal(a, b)


def test_solar_wind_geometry():
    """A solar-wind model (sw_ecl: ELL1, NE_SW free): k_sw_geom runs before the evaluation."""
    from test_solar_wind import load as load_sw
    from pint_amd.engine import Session as S, build_layout, pack_table
    model, toas = load_sw("sw_ecl")[:2]
    s = S()
    try:
        lay = s.add(build_layout(model, toas))
        s.set_instances([(lay, pack_table(lay, model))])
        s.eval(want_M=True)
        assert path(s) == (prep_bit(S, [lay]) | S.EVAL_SW_GEOM, ELL1), path(s)
    finally:
        s.close()
