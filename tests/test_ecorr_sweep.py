"""The ECORR elimination swept over epoch shapes, layouts and launch paths, against longdouble.

Every GLS fit of a pulsar with ECORR indexes TOAs through the epoch lists (ep_ptr, ep_idx,
toa_ep, ep_bin, bep_ptr, bep_idx): k_ecorr forms the epoch sums, k_gram<T, CH, true> folds them
into the Gram, k_ecorr_dmx takes their share from the compact layout's DMX rows, k_onesrow
corrects the virtual ones row, k_wsolve the Woodbury chi2, k_noise_ecorr back-substitutes the
epoch coefficients, k_noise_lnl is the Sherman-Morrison likelihood of the noise fit.  The other
sweeps run ECORR at one epoch shape (four TOAs per epoch, every TOA in one).  The sets here
(ecorr_cases.py; rows built at chosen times, residuals replaced by a seeded N(0, sigma_i) vector)
have epochs of 2 .. 70 rows in an unsorted order, an epoch count that is no multiple of 4, rows
in no epoch, a shuffled row order, 262 small epochs with 70 in one DMX bin, none in another and
some in a frozen one, two ECORR parameters with two epochs at one time, an epoch with rows in a
free bin and in none, an epoch across two free bins, and a TOA in two epochs.  Per case, in one
session:

(a) Session.last_plan() equals shape_cases.predict_plan, fit_layout is as expected, the layout's
    epochs are the designed ones, and the properties the case stands for (test_ecorr_cases.
    set_properties, from the uploaded ep_ptr / ep_idx and shape_cases.free_rows) hold.
(b) debug_gram(pre_ecorr=True) and debug_gram() against [M | F | r]^T N^-1 [M | F | r] in
    longdouble (M from a full-layout read_designmatrix() of a separate session, F from
    ld_util.host_fourier; PLDMNoise's columns, which need the barycentric frequency, stay the
    stored ones) and against it with the epoch block eliminated, G - sum_e s_e s_e^T / D_e.  The
    elimination cancels, so the bar is |dA_ij| <= 1e-12 sqrt(D0_i D0_j) with D0 the reference's
    diagonal before the elimination, the size of the numbers subtracted; D0_i / D_i <= 100 is
    asserted from the reference alone.  Column sums of squares 1e-12 relative.  The WLS case
    compares the Gram with the un-eliminated reference.
(c) step, errors, covariance against a longdouble solve of the device's own normalised system
    (ld_util.step_errors, shared with test_shape_sweep.py): max(1e-9, 3 e_ref), e_ref <= 1e-7.
(d) chi2_gls() against ld_woodbury_chi2 with U = [F | E | ones], 1e-9 relative, r^T N^-1 r / chi2
    <= 10 asserted; the ones column has prior 1e40 also where PHOFF is frozen and the fit has no
    Offset column (k_onesrow).  The post-fit chi2 of the device's own residuals on two cases.
(e) noise_resids(): the ECORR part per TOA against c_e = (s_e[r] - s_e . x_dev) / D_e in
    longdouble, x_dev the device's own step, bar 1e-12 (|s_e[r]| + sum_c |s_e[c] x_c|) / D_e; rows
    in no epoch exactly 0; the red-noise part against F x_dev, bar 1e-12 sum_k |x_k|.
(f) k_noise_lnl through NoiseLikelihood on mix, many and two, kinds 0, 1, 2, at two trial points:
    lnL, chi2 and logdet C / 2 against ld_util.ld_block_likelihood (one dense block and Cholesky
    factor per epoch, no Sherman-Morrison), 1e-10 relative; kinds 0 and 1: the EFAC and ECORR
    derivatives against 1/2 r^T C^-1 dC C^-1 r - 1/2 tr(C^-1 dC) from the same blocks, 1e-9 of the
    sum of the two terms' absolute values.
(g) test_every_target_was_run: the union of the plans and of the asserted properties.

Overlapping epochs (ec_overlap: ECORR -g A 0.5 and a second ECORR on -f fake, which every TOA
carries: 18 + 168 epochs, every row of the first 18 in two).  The epoch block of Sigma is then
not diagonal, and the reference here eliminates it with a dense longdouble inverse
(ld_util.ld_ecorr_eliminate).  Measured on the code before the refusal, full layout, K = 44:
  second ECORR 0.4 us   pint_fit_step: "Woodbury Sigma (noise basis) not positive definite"
  second ECORR 0.1 us   pint_fit_step: "normal matrix not positive definite"
  second ECORR 0.02 us  no error; Gram 1.2e-15 from the per-epoch form G - sum_e s_e s_e^T / D_e
                        and 2.8e-2 sqrt(D0_i D0_j) from the model's; step 0.068 sigma, errors
                        2.5 %, chi2_gls 5.1e-4 relative from the model's
so the step, the errors, the GLS chi2 and the realisations of such a model were wrong, silently
where the coupling is weak.  pint_fit_step, its apply and enqueue forms, chi2_gls and
noise_resids now refuse such a batch (PINT_E_INVALID, "overlapping ECORR epochs") before any
launch; the case asserts the refusals, the all-zero plan, the unchanged tables and residuals,
the fitters' NotImplementedError, and a WLS step of the same session afterwards against
longdouble.

Unreachable by the dispatch rules: k_gram<2, 64, true> and <3, 64, true> are the other sweeps'
(ecorr_Kp112, ecorr_Kp144); T >= 7 with ECORR needs a GLS system of K >= 208, beyond k_solve's
LDS (K <= 196).  The compact layout's Gram is k_gram<1> in every case here: its Kpd <= 80 holds
Kd <= 79 dense columns, and a compact ECORR case of T = 2 (Kd >= 80) adds no epoch indexing that
ec_fit_Kd68 (both column chunks of k_ecorr and k_ecorr_dmx) and the full-layout T = 4, 5, 6 do
not run.  ECORR never rides k_gram_v (vgram_layout).  k_noise_lnl reads no DMX or layout data,
so its cases do not vary them.

Measured on an MI355X (22 cases and 9 likelihood cases, all within their bars; D0_i / D_i <= 2.6):
                                        bar                 measured, worst case
  stored Fourier columns                5e-13               1.4e-15
  Gram before the elimination           1e-12 sqrt(D0 D0)   2.8e-15
  Gram after the elimination            1e-12 sqrt(D0 D0)   2.7e-15 (5.6e-15 by the eliminated diagonal)
  column sums of squares                1e-12               4.5e-15
  step (sigma)                          max(1e-9, 3 e_ref)  4.8e-14   (e_ref up to 4.4e-14)
  errors (relative)                     max(1e-9, 3 s_ref)  3.1e-14   (s_ref up to 2.7e-14)
  covariance (sigma_i sigma_j)          max(1e-9, 3 c_ref)  6.1e-14   (c_ref up to 5.4e-14)
  GLS chi2 (relative)                   1e-9                2.3e-16
  post-fit chi2 (2 cases)               1e-9                1.7e-16
  ECORR realisation (its bar's scale)   1e-12               1.0e-15
  red-noise realisation (sum |x_k|)     1e-12               9.8e-16
  k_noise_lnl lnL / chi2 / logdet       1e-10               1.9e-16 / 1.8e-16 / 1.5e-16
  k_noise_lnl EFAC, ECORR derivatives   1e-9                2.9e-16

Per case (plan: Gram, +e its ECORR variant, s k_gram_s / N-splits / solve / Sigma / rows
k_dmx_rows, gather k_dmx, edmx k_ecorr_dmx, defer k_schur and the deferred covariance;
ec_overlap is refused before any launch):
  case                  K nep plan                                      Gram     step    e_ref   errors      cov     chi2    ECORR      red
  ec_fit_many          17 262 T1+e/1/dmx8/fused/rows/edmx             1.9e-15  7.7e-16  8.4e-16  3.3e-16  7.7e-16  1.8e-16  1.0e-15        -
  ec_small             24   5 s+T1+e/1/blk1/side4                     1.4e-15  5.1e-16  2.0e-15  8.7e-16  1.4e-15  1.3e-16  1.1e-16  9.8e-16
  ec_fit_mix           28  18 T1+e/1/dmx8/fused/rows/edmx             1.5e-15  3.2e-15  7.1e-16  7.3e-16  1.6e-15  1.3e-16  1.1e-16        -
  ec_fit_shuf_d2       28  18 T1+e/1/dmx8/fused/rows/gather/edmx/defer 1.4e-15 2.2e-15  1.2e-15  1.1e-15  2.2e-15  1.2e-16  1.6e-16        -
  ec_fit_two_d2        28  19 T1+e/1/dmx8/fused/rows/edmx/defer       1.4e-15  2.5e-15  1.5e-15  4.2e-16  1.2e-15  1.2e-16  1.6e-16        -
  ec_fit_many_red_d2   41 262 T1+e/1/dmx8/fused/rows/edmx/defer       2.1e-15  4.8e-14  1.5e-14  2.0e-14  4.0e-14  2.0e-16  2.7e-16  8.8e-16
  ec_fit_frozen        43  18 T1+e/1/dmx8/fused/rows/edmx             1.8e-15  3.4e-14  8.5e-15  3.1e-14  6.1e-14  9.9e-17  1.3e-16  5.8e-16
  ec_fit_shuf          44  18 T1+e/1/dmx8/fused/rows/gather/edmx      2.5e-15  9.3e-15  3.3e-15  1.1e-14  2.2e-14  3.8e-17  1.3e-16  7.5e-16
  ec_fit_two           44  19 T1+e/1/dmx8/fused/rows/edmx             1.8e-15  2.7e-14  8.6e-15  1.2e-14  2.5e-14  1.3e-16  1.0e-16  5.8e-16
  ec_straddle          44  18 T1+e/1/blk4/side4                       1.8e-15  1.0e-14  3.2e-15  1.0e-14  2.1e-14  9.9e-17  8.2e-17  5.6e-16
  ec_wls               44  18 T1/1/blk1/-    (WLS)                    1.8e-15  1.8e-15  5.3e-15  4.7e-16  7.5e-16        -        -        -
  ec_ones_full         48  18 T1+e/1/blk4/side4                       1.8e-15  3.3e-15  1.4e-15  1.0e-15  2.1e-15  1.1e-19  1.4e-16  6.2e-16
  ec_ones_fit          48  18 T1+e/1/dmx8/fused/rows/edmx             1.8e-15  1.0e-14  2.7e-15  7.0e-15  1.4e-14  1.1e-19  1.1e-16  6.3e-16
  ec_ones_fit_dmn      56  18 T1+e/1/dmx8/fused/rows/edmx             1.8e-15  1.1e-14  2.8e-14  1.1e-14  2.3e-14  2.3e-16  1.6e-16  7.7e-16
  ec_ones_full_dmn     56  18 T1+e/1/blk4/side4                       1.8e-15  1.6e-14  2.4e-14  1.2e-14  2.4e-14  2.3e-16  1.5e-16  7.7e-16
  ec_fit_mix_red_d2    60  18 T1+e/1/dmx8/fused/rows/edmx/defer       2.7e-15  3.1e-14  6.5e-15  1.4e-14  2.8e-14  1.2e-16  1.4e-16  5.6e-16
  ec_T1                79  18 T1+e/1/blk4/side4                       2.7e-15  1.5e-14  2.0e-14  9.6e-15  1.9e-14  1.4e-16  7.4e-17  5.9e-16
  ec_fit_Kd68          88  18 T1+e/1/dmx8/fused/rows/edmx             2.7e-15  6.4e-15  1.4e-14  2.7e-15  3.9e-15  1.5e-17  1.4e-16  6.2e-16
  ec_T4               159  18 T4+e/1/blk16/side16                     2.7e-15  2.2e-14  2.0e-14  1.0e-14  2.1e-14  1.5e-17  9.1e-17  5.9e-16
  ec_T4_ns3           159  18 T4+e/3/blk16/side16                     1.1e-15  5.2e-15  4.4e-14  5.0e-15  1.0e-14  1.5e-17  9.1e-17  5.8e-16
  ec_T5               191  18 T5+e/1/blk16/side16                     2.7e-15  9.5e-15  4.7e-15  4.5e-15  9.4e-15  8.9e-17  1.0e-16  6.2e-16
  ec_T6               196  18 T6+e/1/column/side16                    2.7e-15  1.2e-14  1.3e-14  1.4e-14  2.8e-14  8.9e-17  1.1e-16  6.4e-16

Mutations (arithmetic-only edits of a scratch copy of pint_hip.hip, never committed; the whole
module run on each) and the cases that failed on them:
  k_ecorr without its tail loop                         every GLS case (21): Gram after the elimination
  k_ecorr's later 64-row chunks with the first's        the 19 GLS cases with an epoch of more than 64 rows
    weights                                             (all but ec_fit_many, ec_fit_many_red_d2): Gram
  k_ecorr_dmx: dd_ from a bin's first 64 epochs only    ec_fit_many, ec_fit_many_red_d2: Gram (5e-2)
  k_ecorr: every row of every epoch counted into eC     ec_fit_frozen: Gram (0.22); an epoch with no bin is
    (ep_bin = -1 and drow < 0 ignored)                  read by nobody, the rows without a bin in an epoch
                                                        that has one are what shows it
  k_onesrow: w -> 1 in the j == R term                  ec_ones_full, ec_ones_fit, ec_ones_fit_dmn,
                                                        ec_ones_full_dmn: chi2_gls (1.4e-4, 1.6e-4)
  k_noise_ecorr: column K - 1 for the residual          every GLS case (21): ECORR realisation
  k_noise_lnl: epochs >= 256 skipped                    test_noise_lnl[many-kind1], [many-kind2]
"""
import numpy as np
import pytest

import ecorr_cases as EC
import shape_cases as SC
from ld_util import (LD, host_fourier, ld_block_likelihood, ld_ecorr_eliminate, ld_gram, ld_woodbury_chi2,
                     step_errors)
from test_ecorr_cases import PROPS, epochs_of, set_properties

pytestmark = pytest.mark.gpu

CASES = sorted(EC.cases(), key=lambda c: c.K)
RAN = {}       # case name -> the plan that ran
SEEN = {}      # case name -> the set properties asserted on its upload
LNL_RAN = set()
_REF = {}
_TOAS = {}


def toas_of(name):
    """(TOAs, seeded unit normal vector) of a set, made once."""
    if name not in _TOAS:
        t = EC.toa_set(name).toas()
        _TOAS[name] = (t, np.random.default_rng(t.ntoas).standard_normal(t.ntoas))
    return _TOAS[name]


def reference(c, toas):
    """(M | F in longdouble, sigma in s, phi, epochs [(TOA indices, ECORR^2)]) of the case's
    model: the stored full-layout design matrix, its PLRedNoise columns replaced by the host's."""
    key = (c.ntim, c.ndmx, c.nred, c.dmx_free, c.dmx_frozen, c.toas, c.ecorr_par, c.phoff, c.ndmn, c.dmx_edge)
    if key in _REF:
        return _REF[key]
    from pint_amd.engine import Session, build_layout, pack_table
    from pint_amd.noise import scaled_sigma_us
    model = SC.model_of(c)
    s = Session()
    try:
        s.set_vgram(False)
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.eval(want_M=True)
        M = np.array(s.read_designmatrix()[0], dtype=LD)
    finally:
        s.close()
    ncol = len(lay.columns)
    assert (ncol, lay.nred, lay.K) == (c.ncol, c.nred, c.K), (lay.columns, lay.nred)
    phi = np.zeros(0, dtype=LD)
    if c.nred:
        nr = 2 * int(lay.spec.dmn0)
        assert nr == 2 * (c.nred - c.ndmn)
        F = host_fourier(lay, toas)[:, :nr]
        dF = float(np.max(np.abs(M[:, ncol:ncol + nr] - F)))
        print(f"{c.name}: stored Fourier columns vs host longdouble {dF:.2e}")
        assert dF <= 5e-13
        M[:, ncol:ncol + nr] = F
        phi = np.asarray(lay.red_phi, dtype=LD)
    sigma = np.asarray(scaled_sigma_us(model, toas), dtype=LD) * LD(1e-6)
    ep = [(idx, LD(lay.ep_phi[e])) for e, idx in enumerate(epochs_of(lay))]
    _REF[key] = (M, sigma, phi, ep)
    return _REF[key]


def check_epochs(c, lay):
    """The uploaded epochs are the designed ones, per parameter."""
    s = EC.toa_set(c.toas)
    got = sorted((q, tuple(e)) for q, e in zip(lay.ep_param, epochs_of(lay)))
    if c.ecorr_par == EC.EC_OVER:  # the second ECORR selects every row: the designed epochs and the -g N pairs
        first = [e for q, e in got if q == "ECORR1"]
        assert first == sorted(tuple(r) for r in s.designed("A"))
        assert sum(1 for q, _ in got if q == "ECORR2") == len(first) + EC.NSLOT // 3
        return
    want = sorted((f"ECORR{k + 1}", tuple(rows)) for k, (_, v, _) in enumerate(c.ecorr_par) for rows in s.designed(v))
    assert got == want


def refused(c, s, lay, toas, r, want):
    """ec_overlap: every GLS entry point refuses, nothing launched or changed; WLS still works."""
    from pint_amd import GLSFitter, _lib
    tabs = s.read_tables_flat().copy()

    def refuses(f):
        with pytest.raises(_lib.PintError) as e:
            f()
        assert e.value.code == _lib.PINT_E_INVALID and "overlapping ECORR epochs" in str(e.value), str(e.value)

    refuses(lambda: s.fit_step(1))
    assert s.last_plan() == want
    refuses(lambda: s.fit_step_apply(1))
    refuses(lambda: s.chi2_gls())
    refuses(lambda: s.noise_resids())
    s.set_lazy(True)
    try:
        refuses(lambda: s.fit_step_enqueue())
    finally:
        s.set_lazy(False)
    assert s.last_plan() == want
    assert np.array_equal(s.read_tables_flat(), tabs)
    assert np.array_equal(s.read_resids()[0][0], r)
    with pytest.raises(NotImplementedError, match="overlapping ECORR epochs"):
        GLSFitter(toas, SC.model_of(c)).fit_toas(maxiter=1)
    # the session afterwards: a WLS step of the same batch (no ECORR work) against longdouble
    s.fit_step(0)
    plan = s.last_plan()
    assert plan["gram_T"] == (1,) and not plan["gram_ecorr"] and not plan["dmx_rows"]
    G, colsq = s.debug_gram()[0]
    dp, er, cov, _ = s.read_step()
    e_dev, e_ref, *_ = step_errors(G, colsq, c.K, c.ncol, 0, lay.red_phi, np.array(dp[0]), np.array(er[0]), np.array(cov[0]))
    print(f"{c.name}: refused by fit_step, fit_step_apply, fit_step_enqueue, chi2_gls, noise_resids and GLSFitter; "
          f"WLS step afterwards {e_dev:.1e} (ref {e_ref:.1e})")
    assert e_ref <= 1e-7 and e_dev <= max(1e-9, 3 * e_ref)
    RAN[c.name] = dict(want, refused=True)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_ecorr(c, monkeypatch):
    from pint_amd.engine import Session, build_layout, pack_table
    monkeypatch.setenv("PINT_NSPLIT", str(c.nsplit))
    toas, z = toas_of(c.toas)
    n = toas.ntoas
    want = SC.predict_plan(c, n, toas.arrays["mjd_float"])
    s = Session()
    try:
        s.set_vgram(c.vgram)
        s.set_vbin(c.vbin)
        lay = s.add(build_layout(SC.model_of(c), toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_cov_defer(c.cov_defer)
        s.set_schur(c.schur)
        s.eval(want_M=Session.FIT if c.layout == "fit" else True)
        # (a) layout and epochs
        assert s.fit_layout(lay)[0] == int(c.ndmx_free >= 8 and not c.ecorr_off)
        check_epochs(c, lay)
        props = set_properties(c, lay, toas)
        assert PROPS.get(c.name, set()) <= props
        SEEN[c.name] = props
        if c.refused:
            from pint_amd.noise import scaled_sigma_us
            r = np.asarray(z * scaled_sigma_us(lay.model, toas) * 1e-6, dtype=np.float64)
            s.debug_set_resids([r])
            refused(c, s, lay, toas, r, want)
            return
        M, sigma, phi, ep = reference(c, toas)
        r = np.asarray(z * sigma, dtype=np.float64)
        s.debug_set_resids([r])
        s.fit_step(c.mode)
        plan = s.last_plan()
        assert plan == want, {k: (plan[k], want[k]) for k in plan if plan[k] != want[k]}
        G, colsq = s.debug_gram()[0]
        G0 = s.debug_gram(pre_ecorr=True)[0][0] if c.mode == 1 else None  # (WLS: no epoch sums were formed)
        dp, er, cov, _ = s.read_step()
        dp, er, cov = np.array(dp[0]), np.array(er[0]), np.array(cov[0])
        nz = s.noise_resids()[0] if c.mode == 1 else None
        c2 = s.chi2_gls()[0] if c.mode == 1 else None
        post = None
        if c.postfit:
            s.eval(False)
            post = (np.array(s.read_resids()[0][0]), s.chi2_gls()[0])
    finally:
        s.close()
    K, ncol = c.K, c.ncol
    # (b) Gram before and after the elimination
    X = np.concatenate([M, np.asarray(r, dtype=LD)[:, None]], axis=1)
    Gref0, csref = ld_gram(M, r, sigma)
    D0 = np.sqrt(np.diag(Gref0))
    if c.mode == 1:
        Gref, S, De = ld_ecorr_eliminate(Gref0, X, sigma, ep)
        keep = float(np.max(np.diag(Gref0) / np.diag(Gref)))
        assert keep <= 100, keep
        eg0 = float(np.max(np.abs(G0 - Gref0) / np.outer(D0, D0)))
    else:
        Gref, keep, eg0 = Gref0, 1.0, 0.0
    D = np.sqrt(np.diag(Gref))
    eg = float(np.max(np.abs(G - Gref) / np.outer(D0, D0)))
    egn = float(np.max(np.abs(G - Gref) / np.outer(D, D)))
    ec = float(np.max(np.abs(colsq / csref - 1)))
    # (c) step, errors, covariance: the device's own normalised system
    e_dev, e_ref, s_dev, s_ref, c_dev, c_ref = step_errors(G, colsq, K, ncol, c.mode, lay.red_phi, dp, er, cov)
    line = (f"{c.name}: K {K} n {n} nep {lay.nep} D0/D {keep:.1f} gram pre {eg0:.1e} post {eg:.1e} (by the eliminated diagonal "
            f"{egn:.1e}) colsq {ec:.1e} step {e_dev:.1e} (ref {e_ref:.1e}) errs {s_dev:.1e} (ref {s_ref:.1e}) "
            f"cov {c_dev:.1e} (ref {c_ref:.1e})")
    e2 = epost = ee = er_ = None
    if c.mode == 1:
        # (d) GLS chi2: U = [F | E | ones]
        E = np.zeros((n, len(ep)), dtype=LD)
        for e, (idx, _) in enumerate(ep):
            E[idx, e] = 1
        U = np.concatenate([M[:, ncol:], E, np.ones((n, 1), dtype=LD)], axis=1)
        ph = np.concatenate([phi, np.array([p for _, p in ep], dtype=LD), [LD(1e40)]])
        ref2, rNr = ld_woodbury_chi2(r, sigma, U, ph)
        assert rNr / ref2 <= 10
        e2 = float(abs(c2 / ref2 - 1))
        line += f" chi2 {e2:.1e}"
        if post is not None:
            refp, rNr = ld_woodbury_chi2(post[0], sigma, U, ph)
            assert rNr / refp <= 10, (rNr, refp)
            epost = float(abs(post[1] / refp - 1))
            line += f" post-fit chi2 {epost:.1e}"
        # (e) realisations from the device's own step
        x = np.asarray(dp[:K], dtype=LD)
        got = np.asarray(nz["ecorr_noise"], dtype=LD)
        inep = np.zeros(n, dtype=bool)
        ee = 0.0
        for e, (idx, _) in enumerate(ep):
            ce = (S[e, K] - S[e, :K] @ x) / De[e]
            bar = (abs(S[e, K]) + np.sum(np.abs(S[e, :K] * x))) / De[e]
            ee = max(ee, float(np.max(np.abs(got[idx] - ce)) / bar))
            inep[idx] = True
        assert np.any(~inep) and np.all(nz["ecorr_noise"][~inep] == 0)
        line += f" ecorr realisation {ee:.1e}"
        nr = 2 * int(lay.spec.dmn0)
        if nr:
            xr = x[ncol:ncol + nr]
            er_ = float(np.max(np.abs(np.asarray(nz["pl_red_noise"], dtype=LD) - M[:, ncol:ncol + nr] @ xr)) / np.sum(np.abs(xr)))
            line += f" red realisation {er_:.1e}"
    sol = plan["solve"] if plan["solve"] != "none" else f"dmx{plan['solve_dmx_waves']}"
    print(line + f" | gram {'s+' if plan['gram_s'] else ''}{plan['gram_T']} ecorr {int(plan['gram_ecorr'])} nsplit {plan['nsplit']} "
          f"dmx_rows {int(plan['dmx_rows'])} k_dmx {int(plan['dmx'])} ecorr_dmx {int(plan['ecorr_dmx'])} solve {sol} "
          f"sigma {'fused' if plan['fuse_sigma'] else ('side%d' % plan['sigma_waves'] if plan['side_sigma'] else '-')}"
          f" schur {int(plan['schur'])} defer {int(plan['cov_deferred'])}")
    RAN[c.name] = plan
    assert eg0 <= 1e-12 and eg <= 1e-12 and ec <= 1e-12
    assert e_ref <= 1e-7
    assert e_dev <= max(1e-9, 3 * e_ref)
    assert s_dev <= max(1e-9, 3 * s_ref)
    assert c_dev <= max(1e-9, 3 * c_ref)
    assert e2 is None or e2 <= 1e-9
    assert epost is None or epost <= 1e-9
    assert ee is None or ee <= 1e-12
    assert er_ is None or er_ <= 1e-12


LNL = [(name, kind) for name in EC.LNL_SETS for kind in (0, 1, 2)]


@pytest.mark.parametrize("name,kind", LNL, ids=[f"{n}-kind{k}" for n, k in LNL])
def test_noise_lnl(name, kind):
    """k_noise_lnl against the block-by-block longdouble likelihood, at the par's values and at
    another point (EFACs 1.25 and 0.9, EQUAD 0.3, ECORRs 1.5 and 0.7 times theirs)."""
    from pint_amd.noisefit import NoiseLikelihood
    from pint_amd.timing_model import get_model
    toas, z = toas_of(name)
    n = toas.ntoas
    model = get_model(EC.lnl_par(kind, EC.LNL_SETS[name]))
    efacs, equads, ecorrs = (model.mask_params(b) for b in ("EFAC", "EQUAD", "ECORR"))
    assert len(efacs) == 2 and len(equads) == 1 and len(ecorrs) == (len(EC.LNL_SETS[name]) if kind else 0)
    params = efacs + equads + ecorrs
    x0 = np.array([float(model[p].value) for p in params])
    x1 = x0 * np.array([1.25 / 1.1, 0.9 / 1.3, 3.0] + [1.5, 0.7][:len(ecorrs)])
    sel = {p: toas.select_mask(model[p].key, model[p].key_value) for p in efacs + equads}
    s0 = np.asarray(toas.get_errors(), dtype=LD)
    r = np.asarray(z * s0 * 1e-6, dtype=np.float64)
    nl = NoiseLikelihood(toas, model, params=params)
    try:
        assert nl.kind == kind
        nl.set_resids(r)
        eps = epochs_of(nl.lay) if kind else []
        epp = list(nl.lay.ep_param) if kind else []
        if kind:
            assert len(eps) == len(EC.toa_set(name).sizes("A")) + len(EC.toa_set(name).sizes("B"))
        out = [nl.evaluate(list(x), grad=kind < 2) for x in (x0, x1)]
    finally:
        nl.close()
    worst = dict(lnl=0.0, chi2=0.0, logdet=0.0, grad=0.0)
    for x, (lnl, chi2, ln, grad) in zip((x0, x1), out):
        v = dict(zip(params, (LD(float(t)) for t in x)))
        q2, f = np.zeros(n, dtype=LD), np.ones(n, dtype=LD)
        for p in equads:
            q2[sel[p]] += v[p] ** 2
        for p in efacs:
            f[sel[p]] *= v[p]
        N = (s0 * s0 + q2) * f * f * LD(1e-12)
        ep = [(idx, (v[q] * LD(1e-6)) ** 2) for idx, q in zip(eps, epp)]
        dN = [np.where(np.isin(np.arange(n), sel[p]), 2 * N / v[p], LD(0)) for p in efacs]
        dphi = [np.array([2 * v[p] * LD(1e-12) if q == p else LD(0) for q in epp], dtype=LD) for p in ecorrs]
        rc, rl, rg, (a, b) = ld_block_likelihood(r, N, ep, dN, dphi)
        if kind == 2:  # the 1e40 offset column
            b = LD(1e-40) + b
            rc = rc - a * a / b
            rl = rl + (np.log(LD(1e40)) + np.log(b)) / 2
        worst["chi2"] = max(worst["chi2"], float(abs(chi2 / rc - 1)))
        worst["logdet"] = max(worst["logdet"], float(abs(ln / rl - 1)))
        worst["lnl"] = max(worst["lnl"], float(abs(lnl / -(rc / 2 + rl) - 1)))
        if kind < 2:
            gi = [params.index(p) for p in efacs + ecorrs]
            for k, (g, scale) in zip(gi, rg):
                worst["grad"] = max(worst["grad"], float(abs(grad[k] - g) / scale))
    print(f"lnl {name} kind {kind}: n {n} nep {len(eps)} lnL {worst['lnl']:.1e} chi2 {worst['chi2']:.1e} "
          f"logdet {worst['logdet']:.1e} grad {worst['grad']:.1e}")
    LNL_RAN.add((name, kind, len(eps)))
    assert worst["lnl"] <= 1e-10 and worst["chi2"] <= 1e-10 and worst["logdet"] <= 1e-10
    assert worst["grad"] <= 1e-9


def test_every_target_was_run():
    """The union of the plans that ran (each asserted equal to its prediction) and of the
    properties asserted on the uploads covers what the sweep was written for; no case skipped."""
    assert sorted(RAN) == sorted(c.name for c in CASES)
    ec = [p for p in RAN.values() if p["gram_ecorr"]]
    assert {1, 4, 5, 6} <= {T for p in ec for T in p["gram_T"]}
    assert any(p["gram_s"] and p["gram_T"] == (1,) for p in ec)
    assert {p["ecorr_dmx"] for p in ec} == {False, True}
    assert any(p["dmx"] and p["ecorr_dmx"] for p in ec)
    assert any(p["fuse_sigma"] for p in ec) and any(p["side_sigma"] for p in ec)
    assert any(p["cov_deferred"] and p["schur"] for p in ec)
    assert any(p["nsplit"] == 3 for p in ec)
    assert any(p.get("refused") for p in RAN.values())
    assert not RAN["ec_wls"]["gram_ecorr"] and not RAN["ec_straddle"]["dmx_rows"]
    by = {c.name: c for c in CASES}
    fit = set().union(*(SEEN[k] for k in SEEN if by[k].layout == "fit" and not by[k].ecorr_off))
    assert {"epoch > 64 rows", "size % 4", "epoch count % 4", "ep_idx not contiguous", "rows in no epoch", "ep_bin = -1",
            "drow < 0 in a binned epoch", "bin > 64 epochs", "epochs per bin % 4", "bin with no epoch", "Kd > 63",
            "two ECORR parameters", "two epochs at one time"} <= fit
    full = set().union(*(SEEN[k] for k in SEEN if by[k].layout == "full"))
    assert {"epoch > 64 rows", "size % 4", "epoch count % 4", "rows in no epoch"} <= full
    assert "epoch in two free bins" in SEEN["ec_straddle"] and "TOA in two epochs" in SEEN["ec_overlap"]
    # k_onesrow with epochs in both layouts, and its PLDMNoise branch
    assert {(c.layout, bool(c.ndmn)) for c in CASES if c.phoff} == {("full", False), ("fit", False), ("full", True), ("fit", True)}
    # k_noise_lnl: every kind on every set, more than 256 epochs among them
    assert {(n, k) for n, k, _ in LNL_RAN} == set(LNL)
    assert max(nep for _, k, nep in LNL_RAN if k) > 256
