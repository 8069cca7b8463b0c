"""The wideband DM rows (k_wb_gram, k_dm_resid) swept over index maps, loop edges and launch
routes, against a longdouble reference.

The two wideband fixtures (wb_dd, sw_wb) are one pulsar, one instance and one route each, checked
end to end.  Every case here (wb_cases.py) is a synthetic model on one of the shape sweep's fake
TOA sets with flag columns (-fe, -be, -gp) and wideband DMs written onto it: pp_dm = DM_model +
z dm_sigma, DM_model in longdouble from the par values, the time residuals replaced by a seeded
N(0, sigma) vector.  One Session per case, as test_shape_sweep: set_vgram / set_vbin /
set_cov_defer / set_schur, add, set_instances, set_wideband, set_wbfit, eval(FIT),
debug_set_resids, fit_step(1).

(a) Session.last_plan() equals the plan shape_cases.predict_plan derives for the case, wb_gram
    included; test_every_wideband_route_was_run asserts the union: k_wb_gram after k_gram_s, after
    k_gram<T> with k_dmx_rows, with k_dmx, with k_ecorr_dmx, after k_gram_v with and without the
    binned body, after k_greduce over 3 and 5 N-splits on either Gram path, and before
    k_solve_dmx<8> (covariance in the solve, deferred, deferred with k_schur), k_solve_dmx<16>, the
    compact layout's general-solve fall-back (k_solve_blk<16>) and k_eig.
(b) Session.dm_resids() plain, with the weighted and with the unweighted mean removed, against
    pp_dm - DM_model in longdouble from the par values (wb_cases.dm_model) and against
    oracle.dm_residuals (pinned to the reference's wb_dd); the two references must agree to the
    bars before the device is judged.  Bars 1e-12 pc/cm^3 and 1e-12 relative on chi2
    (test_wideband.py's).  DMEFAC 1.3 and a DMEQUAD act on -fe B only and the unscaled errors
    spread over a factor 5, so the weighted mean (unscaled weights) and chi2 (scaled) differ.
(c) debug_gram() against [M | F | r]^T N^-1 [M | F | r] + [M_dm | 0 | r_dm]^T W_dm [M_dm | 0 | r_dm]
    in longdouble: M and F as in test_shape_sweep (a full-layout session of its own; host Fourier
    columns; the ECORR block eliminated over the TOA rows only), M_dm from wb_cases.dm_design,
    colsq against the unweighted sums of squares over all 2 n rows.  Bars |dA_ij| <= 1e-12
    sqrt(D_i D_j) and 1e-12 relative.  The DM rows' share must move a normalised entry by more
    than 1e-6, in the reference and in the device's Gram (measured 0.49 .. 1.0), so a k_wb_gram
    that added nothing cannot pass.
(d) step, errors and covariance against the longdouble solve of the device's own normalised
    system, as test_shape_sweep (c): e_dev <= max(1e-9, 3 e_ref) with e_ref <= 1e-7 asserted.
    DM free beside every bin free is singular, so every case with DM free freezes bins; each
    case's e_ref was checked on the CPU (oracle design matrix, float64 Cholesky of the longdouble
    Gram) while the table was written; on the device 7e-16 .. 1.5e-12.
(e) for three cases (wb_cases.E2E) WidebandTOAFitter.fit_toas(maxiter=1) on TOAs zeroed on the
    case's own model against oracle.wideband_gls_step: parameters 1e-3 sigma, errors 1e-5
    (test_gpu_wideband_fit's bars); measured 3.7e-5 sigma and 3e-13.

Index maps, and the assertion that catches each off-by-one (by reasoning: no mutated kernel was
run on a device):
  * DMJUMP mask bit against free-column index: wb_dmjgap_grams, wb_vb and the grid-like batch
    free DMJUMP1 and DMJUMP3 around a frozen DMJUMP2, wb_dmx16 frees DMJUMP2, 3 behind a frozen
    DMJUMP1.  Reading bit 1 for DMJUMP3 selects -be X instead of -fe B: a different third of the
    TOAs, so the DMJUMP3 row and column of the Gram and its colsq move by O(1) of their size -> (c).
  * Taylor order against free-column index: wb_dm12_b21, wb_dm12zero (DM frozen, DM1 and DM2
    free), wb_m1_b9 (DM1 alone, where index 0 would give a column of ones): dt^k / k! with k one
    too small changes colsq by orders of magnitude -> (c).
  * cc[m] = cmap[c] against the full-layout index: the DMJUMP columns follow the DMX block in the
    model's order, so in every case with a free DMJUMP the two differ by ndc -> (c), wrong rows.
  * dmx_a (bin among all bins) against the compact column (free bins only): the cases with
    frozen bins in front of free ones (wb_m3_b10, wb_m8_b11, wb_dm12zero, wb_shuffle, wb_vb, the
    batches).  The modelled DM then takes a neighbouring bin's value, ~1e-3 pc/cm^3 = several
    sigma_dm, for most TOAs -> (b) in k_dm_resid, the residual row of (c) in k_wb_gram; frozen
    bins keep non-zero values so that leaving them out shows in the same way.
  * DD / DCS / Sd rows by compact column a: the one-TOA bin of wb_dm12_b21 and the bins of
    unequal counts make a shifted a visible in DD (sum of weights) and colsq (count) -> (c).
  * colsq[(coff + cc) nsplit]: the N-split cases (k_greduce leaves the sum in slot 0 of nsplit);
    a slot without the stride lands in another column's partial -> (c) colsq.  The triangle
    G[min * Kp + max]: an entry left in the other triangle is missing from what k_debug_gram
    reads -> (c); a solve route that read another triangle or slot than k_debug_gram would give a
    step that is not the solution of the system (d) rebuilds from debug_gram -> (d), per route.
  * instance offsets goff, sdoff, ddoff, ooff, coff, ic[blockIdx.x]: test_mixed_batch (A, B, A' of
    different widths) and test_grid_like_batch (4 tables); B's Gram and step bit for bit those of
    a session without the wideband rows, its DM residuals zeros with chi2 NaN (!Pd.wb).
  * `any`: wb_dm12zero has DM1 = DM2 = 0 free: the modelled DM at x = 0, the derivative columns
    at dt -> (c) (columns of zeros otherwise, and a singular system in (d)).
  * weights: mean by 1 / pp_dme^2, chi2 and Gram by 1 / dm_sigma^2; swapped, the weighted-mean
    residuals move by ~1e-5 pc/cm^3 (the two means differ by a fraction of sigma_dm / sqrt(n)) -> (b).
Loop edges: n = 300, 530, 1100 (no multiples of 256), ndc = 8, 9, 10, 11, 16, 20, 21 (every ndc
% 4), bins of 1, 24 .. 79 and 137 / 138 TOAs (one, two and three passes of 64 lanes), m = 0
(wb_m0_b8) and m = 8 = WB_MAXC (wb_m8_*), TOAs in two and three DMJUMP masks, TOAs outside every
free bin, k_dm_resid on 37 TOAs (test_dm_resid_alone).  NE_SW (wb_nesw, Gram stage only): the
geometry is the device's own, d delay / d NE_SW over d delay / d DM of its TOA design matrix
(pinned to the reference by test_solar_wind.py), so the case checks k_wb_gram's use of the
geometry (column, modelled DM, NE_SW in front of DM in the column order), not the geometry.

Guards: pint_fit_step with the wideband rows asked for now refuses (PINT_E_INVALID, nothing
launched) a design matrix in the full layout and a wideband pulsar off the compact DMX layout;
before, it took a TOA-only step (test_wideband_step_off_the_compact_layout_is_refused).

ECORR: the compact layout with ECORR is reachable (every epoch of the e1100 set lies within
one bin; fit_layout reports compact): wb_ecorr and wb_ecorr_ns3 run k_ecorr_dmx (-=)
and k_wb_gram (+=) on the same Sd and DD and meet the bars; fitter.py's "no ECORR" text was wrong
and is corrected.

Unreachable or left out: k_wb_gram after k_gram_v with ECORR or with gathered (k_dmx) bins (the
generated-Fourier path takes neither); k_gram_v's third row tile with wideband data as a target
(no WaveX beside wideband data: at most 16 dense columns; slot collisions alone could ask for
it); more than WB_MAXC columns (refused: test_wideband.py); a wideband pulsar with fewer than 8
free bins in a fit step (refused, above).  Not covered here: a TOA in a free and an overlapping
frozen bin (dmx_b, dmx_x in the modelled DM); test_dmx_overlap.py covers those maps on the TOA
side.  No bug was found in k_wb_gram or k_dm_resid.

Measured on an MI355X (plan: Gram / N-splits / solve; Gram s = k_gram_s, Tn = k_gram<n>, vK =
k_gram_v key K, vb its binned body, +rows k_dmx_rows, +dmx k_dmx, +ecorr k_ecorr_dmx; errors as
in (b), (c), (d)); k_eig on wb_dmjgap_grams: step 3.0e-15, errors 9.3e-16, covariance 1.6e-15
against the bar 1e-8; k_dm_resid alone on 37 TOAs: 5.9e-16 pc/cm^3, chi2 1.4e-13:
  case                  K     n  m ndc  plan                      dm resid     chi2     Gram    colsq     step    e_ref   errors      cov
  wb_m0_b8             14  1100  0   8  v1vb/1/dmx8                5.1e-16  1.5e-14  7.7e-15  1.0e-16  8.3e-16  7.5e-16  2.3e-16  4.6e-16
  wb_m1_b9             32   530  1   9  v13vb/1/dmx8               5.0e-16  1.6e-14  6.2e-15  1.3e-16  8.0e-15  5.9e-14  2.0e-14  4.0e-14
  wb_m3_b10            35   530  3  10  v13vb/1/dmx8               5.0e-16  2.6e-14  1.1e-14  1.3e-16  1.6e-14  9.3e-14  1.0e-14  1.9e-14
  wb_m8_b11            57  1100  8  11  v14vb/1/dmx8               7.8e-16  3.8e-15  9.7e-14  2.1e-16  3.7e-15  4.1e-13  4.7e-14  9.4e-14
  wb_dm12_b21          45   530  2  21  v13vb/1/dmx8               5.1e-16  1.9e-14  6.6e-15  1.3e-16  2.7e-14  4.1e-13  7.8e-15  2.6e-14
  wb_dmjgap_grams      16   300  2   8  s+rows/1/dmx8              6.4e-16  3.1e-14  9.8e-14  1.4e-16  7.8e-16  9.3e-16  3.1e-16  6.2e-16
  wb_dm12zero          34   530  2  10  v13vb/1/dmx8               2.9e-16  1.3e-14  5.5e-15  1.3e-16  8.0e-15  7.7e-14  1.1e-14  2.1e-14
  wb_shuffle           35   530  5   8  T1+rows+dmx/1/dmx8         7.5e-16  2.8e-14  8.7e-14  3.9e-16  1.3e-14  1.0e-13  5.9e-15  1.2e-14
  wb_reverse           35   530  5   8  v13vb/1/dmx8               7.5e-16  2.8e-14  8.7e-14  2.1e-16  1.2e-14  3.9e-14  1.3e-14  2.5e-14
  wb_shuffle_ns3       35   530  5   8  T1+rows+dmx/3/dmx8         7.5e-16  2.8e-14  8.7e-14  6.1e-16  1.2e-14  6.9e-14  1.6e-14  3.2e-14
  wb_m8_novg           57  1100  8  11  T1+rows/1/dmx8             7.8e-16  3.8e-15  9.7e-14  4.5e-16  1.5e-14  1.0e-13  3.0e-14  5.9e-14
  wb_vb                63  1100  5  20  v14vb/1/dmx8               7.1e-16  1.1e-14  8.8e-14  1.4e-16  1.2e-14  1.6e-13  3.6e-14  7.2e-14
  wb_novb              63  1100  5  20  v14/1/dmx8                 7.1e-16  1.1e-14  8.8e-14  1.4e-16  1.4e-14  1.5e-13  4.2e-14  8.4e-14
  wb_novg              63  1100  5  20  T1+rows/1/dmx8             7.1e-16  1.1e-14  8.8e-14  4.5e-16  3.6e-15  1.3e-13  3.5e-15  1.1e-14
  wb_vb_ns3            63  1100  5  20  v14vb/3/dmx8               7.1e-16  1.1e-14  8.8e-14  1.4e-16  7.2e-15  1.8e-13  4.4e-14  8.8e-14
  wb_vb_ns5            63  1100  5  20  v14vb/5/dmx8               7.1e-16  1.1e-14  8.8e-14  3.0e-16  9.0e-15  1.8e-13  2.7e-14  5.5e-14
  wb_novg_ns3          63  1100  5  20  T1+rows/3/dmx8             7.1e-16  1.1e-14  8.8e-14  2.6e-16  4.4e-15  1.0e-13  4.5e-14  9.0e-14
  wb_dmx8_d0          137  1100  3  16  T3+rows/1/dmx8             7.0e-16  1.4e-14  9.9e-14  1.8e-15  5.9e-15  1.5e-12  5.6e-14  1.1e-13
  wb_dmx8_d2          137  1100  3  16  T3+rows/1/dmx8/schur/defer 7.0e-16  1.4e-14  9.9e-14  1.8e-15  5.9e-15  1.5e-12  5.6e-14  1.1e-13
  wb_dmx8_d2_noschur  137  1100  3  16  T3+rows/1/dmx8/defer       7.0e-16  1.4e-14  9.9e-14  1.8e-15  5.9e-15  1.5e-12  5.6e-14  1.1e-13
  wb_dmx16            147  1100  3  16  T3+rows/1/dmx16            7.0e-16  1.3e-14  1.0e-13  3.1e-15  6.4e-15  1.1e-12  2.5e-14  4.8e-14
  wb_blk77            186  1100  2  16  T5+rows/1/blk16            7.0e-16  1.4e-14  9.9e-14  5.3e-15  2.8e-16  1.3e-13  1.6e-14  3.3e-14
  wb_ecorr             45  1100  3  20  T1+rows+ecorr/1/dmx8       7.6e-16  1.3e-14  1.0e-13  6.3e-16  3.2e-14  5.5e-14  6.3e-15  3.1e-14
  wb_ecorr_ns3         45  1100  3  20  T1+rows+ecorr/3/dmx8       7.6e-16  1.3e-14  1.0e-13  3.2e-16  1.8e-14  4.3e-14  5.3e-15  2.1e-14
  wb_nesw              33   530  3   8  v13vb/1/dmx8               6.9e-16  1.9e-14  5.7e-14  1.3e-16        -        -        -        -
  mixed batch, A[0]                                         7.5e-16  2.4e-14  1.2e-14  1.8e-16  1.5e-14  1.3e-13  1.0e-14  2.0e-14
  mixed batch, A[2]                                         6.9e-16  3.2e-14  6.9e-15  1.8e-16  1.0e-14  1.5e-13  9.4e-15  1.8e-14
  grid-like batch, A[0]                                     7.5e-16  2.4e-14  8.5e-14  1.3e-16  3.6e-15  7.6e-14  4.5e-15  9.0e-15
  grid-like batch, A[1]                                     6.9e-16  3.2e-14  4.8e-14  1.3e-16  1.3e-14  2.2e-13  9.8e-15  1.9e-14
  grid-like batch, A[2]                                     7.1e-16  5.1e-14  6.2e-14  1.3e-16  1.8e-14  1.1e-13  1.0e-14  2.0e-14
  grid-like batch, A[3]                                     8.8e-16  1.8e-13  1.1e-13  2.0e-16  1.7e-14  1.3e-13  1.8e-14  3.6e-14
"""
import copy

import numpy as np
import pytest

import pint_oracle as O
import shape_cases as SC
import wb_cases as WB
from ld_util import LD, ld_gram, ld_inverse, ld_solve
from test_shape_sweep import chol64, host_fourier, toa_sets  # noqa: F401  (toa_sets: the sweep's fixture)

pytestmark = pytest.mark.gpu

NESW = WB.case("wb_nesw", 6, 12, 8, "n530", dm_free=("DM",), ndmjump=1, dmx_frozen=WB.third(12), nesw=True)
CASES = WB.cases() + [NESW]
EIG = "wb_dmjgap_grams"   # the case that also runs k_eig on its wideband system
BATCH_A = WB.case("wb_batchA", 6, 15, 8, "n530", dm_free=WB.ALL_DM, ndmjump=3, dmj_frozen=(1,), dmx_frozen=WB.third(15))
# (in the mixed batch, which also runs without the wideband rows, the DMJUMPs are frozen: a free
# DMJUMP has no TOA-row entries, and the TOA-only normal matrix would be singular)
MIXED_A = BATCH_A.but(name="wb_mixedA", dmj_frozen=(0, 1, 2))
BATCH_B = SC.Case("plain_B", 6, 9, 8, toas="n300", layout="fit")
RAN = {}


def oracle_inputs(model, toas):
    om, ot = O.from_product_model(model), O.toas_from_product(toas)
    ot["pp_dm"], ot["pp_dme"] = toas.get_dms(), toas.get_dm_errors()
    return om, ot


def timing_columns(model, toas, tables=None):
    """Per table (default: the model's own) the full-layout design matrix of a session of its
    own without k_gram_v and without wideband data, in longdouble, the Fourier columns replaced
    by the host's; and (sigma in s, phi, ECORR epochs, layout)."""
    from pint_amd.engine import Session, build_layout, pack_table
    from pint_amd.noise import scaled_sigma_us
    s = Session()
    try:
        s.set_vgram(False)
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, t) for t in (tables if tables is not None else [pack_table(lay)])])
        s.eval(want_M=True)
        Ms = [np.array(m, dtype=LD) for m in s.read_designmatrix()]
    finally:
        s.close()
    ncol, phi = len(lay.columns), None
    if lay.nred:
        F = host_fourier(lay, toas)
        for M in Ms:
            assert float(np.max(np.abs(M[:, ncol:] - F))) <= 5e-13
            M[:, ncol:] = F
        phi = np.asarray(lay.red_phi, dtype=LD)
    sigma = np.asarray(scaled_sigma_us(model, toas), dtype=LD) * LD(1e-6)
    ep = None
    if lay.nep:
        ep = [(lay.ep_idx[lay.ep_ptr[e]:lay.ep_ptr[e + 1]], LD(lay.ep_phi[e])) for e in range(lay.nep)]
    return Ms, sigma, phi, ep, lay


def host_dm(c, model, toas, geometry=None):
    """(DM residuals pp_dm - DM_model, scaled DM errors) in longdouble."""
    dm = WB.dm_model(c, model, toas)
    if geometry is not None:
        dm = dm + LD(model["NE_SW"].value) * geometry
    return np.asarray(toas.get_dms(), dtype=LD) - dm, WB.scaled_dm_errors(c, toas)


def check_dm_resids(c, model, toas, got, geometry=None):
    """got: {(subtract_mean, weighted): (resids, chi2)} of the device.  The host longdouble
    residuals and the oracle's must agree before the device is judged; returns the device's worst
    (residual error in pc/cm^3, relative chi2 error)."""
    rd, sd = host_dm(c, model, toas, geometry)
    om, ot = oracle_inputs(model, toas)
    w = 1 / np.asarray(toas.get_dm_errors(), dtype=LD) ** 2  # the unscaled errors weight the mean
    er = ec = 0.0
    for (sub, wt), (res, chi2) in got.items():
        ref = rd - ((np.sum(rd * w) / np.sum(w) if wt else np.mean(rd)) if sub else 0)
        c2 = np.sum((ref / sd) ** 2)
        if geometry is None:  # (the oracle has no solar wind)
            o = O.dm_residuals(om, ot, subtract_mean=sub, use_weighted_mean=wt)
            assert float(np.max(np.abs(o["resids"] - ref))) < 1e-12 and abs(float(o["chi2"] / c2 - 1)) < 1e-12
        er = max(er, float(np.max(np.abs(res - ref))))
        ec = max(ec, abs(float(chi2 / c2 - 1)))
    return er, ec


def read_dm_resids(s, k=0):
    out = {}
    for sub, wt in ((False, True), (True, True), (True, False)):
        res, chi2 = s.dm_resids(subtract_mean=sub, use_weighted_mean=wt)
        out[(sub, wt)] = (np.array(res[k]), float(chi2[k]))
    return out


def reference_gram(c, model, toas, lay, M, sigma, ep, r, geometry=None):
    """The combined system [M | F | r]^T N^-1 [M | F | r] + [M_dm | 0 | r_dm]^T W_dm [M_dm | 0 | r_dm]
    in longdouble (the ECORR block eliminated over the TOA rows), the column sums of squares over
    all 2 n rows, and the DM rows' share alone."""
    Gt, cst = ld_gram(M, r, sigma)
    if ep is not None:
        Xw = np.concatenate([M, np.asarray(r, dtype=LD)[:, None]], axis=1) / (sigma * sigma)[:, None]
        for idx, ph_e in ep:
            se = Xw[idx].sum(axis=0)
            Gt = Gt - np.outer(se, se) / (1 / ph_e + np.sum(1 / (sigma[idx] * sigma[idx])))
    Md = np.zeros(M.shape, dtype=LD)
    ncol = len(lay.columns)
    Md[:, :ncol] = WB.dm_design(c, model, lay.columns, toas, {"NE_SW": geometry})
    if geometry is None:  # the second reference: the oracle's DM design matrix (float64)
        om, ot = oracle_inputs(model, toas)
        Mo = O.dm_designmatrix(om, list(lay.columns), ot)
        assert float(np.max(np.abs(Mo - Md[:, :ncol]) / np.maximum(1, np.abs(Md[:, :ncol])))) <= 1e-15
    rd, sd = host_dm(c, model, toas, geometry)
    Gd, csd = ld_gram(Md, rd, sd)
    return Gt + Gd, cst + csd, Gd


def check_gram(G, colsq, Gref, csref, Gd):
    D = np.sqrt(np.diag(Gref))
    eg = float(np.max(np.abs(G - Gref) / np.outer(D, D)))
    ec = float(np.max(np.abs(colsq / csref - 1)))
    moved = float(np.max(np.abs(Gd) / np.outer(D, D)))           # the DM rows' share of the reference ...
    moved_dev = float(np.max(np.abs(G - (Gref - Gd)) / np.outer(D, D)))  # ... and of the device's Gram
    return eg, ec, min(moved, moved_dev)


def check_step(c, lay, G, colsq, dp, er, cov):
    """Step, errors and covariance against the longdouble solve of the device's own normalised
    system (test_shape_sweep part (c)); returns (e_dev, e_ref, s_dev, s_ref, c_dev, c_ref)."""
    K, ncol = lay.K, len(lay.columns)
    inv = 1.0 / np.sqrt(colsq)
    Ad = G[:K, :K] * (inv[:, None] * inv[None, :])
    if lay.nred:
        i = np.arange(ncol, K)
        Ad[i, i] += (inv[ncol:] * inv[ncol:]) / np.asarray(lay.red_phi)
    bd = G[:K, K] * inv
    x = ld_solve(Ad, bd) * inv
    X = ld_inverse(Ad) * np.outer(inv, inv)
    sg = np.sqrt(np.diag(X))
    X64 = chol64(Ad, np.eye(K)) * np.outer(inv, inv)
    ss = np.outer(sg[:ncol], sg[:ncol])
    return (float(np.max(np.abs(dp[:K] - x) / sg)), float(np.max(np.abs(chol64(Ad, bd) * inv - x) / sg)),
            float(np.max(np.abs(er[:K] / sg - 1))), float(np.max(np.abs(np.sqrt(np.diag(X64)) / sg - 1))),
            float(np.max(np.abs(cov - X[:ncol, :ncol]) / ss)), float(np.max(np.abs(X64[:ncol, :ncol] - X[:ncol, :ncol]) / ss)))


def case_data(c, sets):
    """(TOAs with flags and wideband DMs, model, time residuals, NE_SW geometry or None)."""
    base, z = sets[c.toas]
    geometry = None
    if c.nesw:
        # the solar-wind DM per unit NE_SW of every TOA: the device's own TOA design-matrix
        # columns, d delay / d NE_SW over d delay / d DM (both carry DMconst / f^2 at the
        # barycentric frequency and the same chain factor)
        plain, model = WB.case_toas(c, base)
        (M,), _, _, _, lay = timing_columns(model, plain)
        geometry = M[:, lay.columns.index("NE_SW")] / M[:, lay.columns.index("DM")]
        assert 1e-7 < float(np.min(geometry)) and float(np.max(geometry)) < 1e-2
    toas, model = WB.case_toas(c, base, None if geometry is None else LD(SC.NE_SW) * geometry)
    return toas, model, z[WB.order_index(c, base.ntoas)], geometry


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_wideband_shape(c, toa_sets, monkeypatch):
    from pint_amd.engine import Session, build_layout, pack_table
    monkeypatch.setenv("PINT_NSPLIT", str(c.nsplit))
    toas, model, z, geometry = case_data(c, toa_sets)
    (M,), sigma, phi, ep, _ = timing_columns(model, toas)
    r = np.asarray(z * sigma, dtype=np.float64)
    want = SC.predict_plan(c, toas.ntoas, toas.arrays["mjd_float"])
    s = Session()
    try:
        s.set_vgram(c.vgram)
        s.set_vbin(c.vbin)
        s.set_cov_defer(c.cov_defer)
        s.set_schur(c.schur)
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_wideband(lay)
        s.set_wbfit(True)
        assert s.fit_layout(lay)[0] == 1  # (ECORR: every epoch within one bin keeps the compact layout)
        assert (len(lay.columns), lay.nred, lay.K, bool(lay.nep)) == (c.ncol, c.nred, c.K, c.ecorr)
        s.eval(want_M=Session.FIT)
        s.debug_set_resids([r])
        dmr = read_dm_resids(s)
        s.fit_step(1)
        plan = s.last_plan()
        G, colsq = s.debug_gram()[0]
        dp, er, cov, _ = s.read_step()
        dp, er, cov = np.array(dp[0]), np.array(er[0]), np.array(cov[0])
        eig = None
        if c.name == EIG:  # k_eig on the same Gram: every direction kept, the step outputs replaced
            assert s.solve_eig(1, np.zeros(1)) == [[]]
            d2, e2, c2, _ = s.read_step()
            eig = (np.array(d2[0]), np.array(e2[0]), np.array(c2[0]))
    finally:
        s.close()
    # (a) plan
    assert plan == want, {k: (plan[k], want[k]) for k in plan if plan[k] != want[k]}
    RAN[c.name] = plan
    # (b) DM residuals and chi2
    e_r, e_c2 = check_dm_resids(c, model, toas, dmr, geometry)
    # (c) Gram
    Gref, csref, Gd = reference_gram(c, model, toas, lay, M, sigma, ep, r, geometry)
    eg, ec, moved = check_gram(G, colsq, Gref, csref, Gd)
    line = f"{c.name}: K {lay.K} n {toas.ntoas} m {c.m_dm} ndc {c.ndmx_free} dm resid {e_r:.1e} chi2 {e_c2:.1e} gram {eg:.1e} colsq {ec:.1e} moved {moved:.1e}"
    # (d) step, errors, covariance (the NE_SW case: Gram stage only)
    st = None
    if not c.nesw:
        st = check_step(c, lay, G, colsq, dp, er, cov)
        line += " step {:.1e} (ref {:.1e}) errs {:.1e} (ref {:.1e}) cov {:.1e} (ref {:.1e})".format(*st)
    if eig is not None:
        se = check_step(c, lay, G, colsq, *eig)
        line += f" | k_eig step {se[0]:.1e} errs {se[2]:.1e} cov {se[4]:.1e}"
    sol = plan["solve"] if plan["solve"] != "none" else f"dmx{plan['solve_dmx_waves']}"
    print(line + f" | gram {plan['gram_T'] or plan['gram_v'] or 'small'} nsplit {plan['nsplit']} dmx_rows {int(plan['dmx_rows'])} "
          f"dmx {int(plan['dmx'])} ecorr_dmx {int(plan['ecorr_dmx'])} solve {sol} schur {int(plan['schur'])} defer {int(plan['cov_deferred'])}")
    assert e_r <= 1e-12 and e_c2 <= 1e-12
    assert eg <= 1e-12 and ec <= 1e-12
    assert moved > 1e-6
    if st is not None:
        e_dev, e_ref, s_dev, s_ref, c_dev, c_ref = st
        assert e_ref <= 1e-7
        assert e_dev <= max(1e-9, 3 * e_ref)
        assert s_dev <= max(1e-9, 3 * s_ref)
        assert c_dev <= max(1e-9, 3 * c_ref)
    if eig is not None:  # test_svd_path_matches_cholesky's bar, here against the longdouble solve
        assert max(se[0], se[2], se[4]) < 1e-8


def test_every_wideband_route_was_run():
    """The union of the plans that ran (each asserted equal to its prediction): k_wb_gram after
    every Gram route and before every solve route; no case may be skipped."""
    assert sorted(RAN) == sorted(c.name for c in CASES)
    plans = list(RAN.values())
    assert all(p["wb_gram"] for p in plans)
    assert any(p["dmx"] for p in plans)
    assert any(p["dmx_rows"] and not p["dmx"] for p in plans)
    assert any(p["gram_s"] for p in plans) and any(p["gram_T"] and not p["greduce"] for p in plans)
    assert {True, False} <= {vb for p in plans for _, vb in p["gram_v"]}
    assert any(p["greduce"] and p["gram_v"] and p["nsplit"] > 1 for p in plans)
    assert any(p["greduce"] and p["gram_T"] and p["nsplit"] > 1 for p in plans)
    assert {1, 3, 5} <= {p["nsplit"] for p in plans}
    assert any(p["ecorr_dmx"] and p["gram_ecorr"] for p in plans)
    assert {8, 16} <= {p["solve_dmx_waves"] for p in plans}
    assert any(p["solve"] == "blk16" and p["dmx_rows"] for p in plans)  # the compact layout's general-solve fall-back
    assert any(p["cov_deferred"] and p["schur"] for p in plans) and any(p["cov_deferred"] and not p["schur"] for p in plans)
    assert any(p["solve_dmx_waves"] and not p["cov_deferred"] for p in plans)


def perturbed(c, model, k):
    """The model with DM, one DMX value (a frozen bin's, when there is one) and one DMJUMP moved."""
    m = copy.deepcopy(model)
    m["DM"].value = LD(m["DM"].value) + LD(3e-4) * k
    a = (c.dmx_frozen or (1,))[0]
    m[f"DMX_{a + 1:04d}"].value = LD(m[f"DMX_{a + 1:04d}"].value) - LD(2e-4) * k
    j = m.mask_params("DMJUMP")[-1]
    m[j].value = LD(m[j].value) + LD(5e-4) * k
    return m


def run_batch(insts_of, wb_lays, wbfit, resids):
    """One session over the instances insts_of(session) builds; returns (layouts, per-instance
    DM residual reads, Grams, steps, plan)."""
    from pint_amd.engine import Session
    s = Session()
    try:
        lays = insts_of(s)
        for lay in wb_lays(lays):
            s.set_wideband(lay)
        s.set_wbfit(wbfit)
        s.eval(want_M=Session.FIT)
        s.debug_set_resids(resids)
        dmr = [read_dm_resids(s, k) for k in range(len(lays))] if wbfit else None
        s.fit_step(1)
        grams = s.debug_gram()
        dp, er, cov, _ = s.read_step()
        steps = [(np.array(dp[k]), np.array(er[k]), np.array(cov[k])) for k in range(len(lays))]
        return lays, dmr, grams, steps, s.last_plan()
    finally:
        s.close()


def check_instance(c, model, toas, lay, M, sigma, ep, r, dmr, gram, step, tag):
    e_r, e_c2 = check_dm_resids(c, model, toas, dmr)
    Gref, csref, Gd = reference_gram(c, model, toas, lay, M, sigma, ep, r)
    eg, ec, moved = check_gram(gram[0], gram[1], Gref, csref, Gd)
    st = check_step(c, lay, gram[0], gram[1], *step)
    print(f"{tag}: dm resid {e_r:.1e} chi2 {e_c2:.1e} gram {eg:.1e} colsq {ec:.1e} moved {moved:.1e} "
          "step {:.1e} (ref {:.1e}) errs {:.1e} (ref {:.1e}) cov {:.1e} (ref {:.1e})".format(*st))
    assert e_r <= 1e-12 and e_c2 <= 1e-12 and eg <= 1e-12 and ec <= 1e-12 and moved > 1e-6
    assert st[1] <= 1e-7 and st[0] <= max(1e-9, 3 * st[1]) and st[2] <= max(1e-9, 3 * st[3]) and st[4] <= max(1e-9, 3 * st[5])


def test_mixed_batch(toa_sets):
    """Three instances: wideband pulsar A at its table, a pulsar B without wideband data, A at a
    perturbed table (the instance offsets goff, sdoff, ddoff, ooff, coff and ic[blockIdx.x]; the
    !Pd.wb early return).  A's instances against the longdouble references; B's Gram bit for bit
    that of a session without the wideband rows, its DM residuals zeros with chi2 NaN."""
    from pint_amd.engine import build_layout, pack_table
    tA, mA, zA, _ = case_data(MIXED_A, toa_sets)
    mA2 = perturbed(MIXED_A, mA, 1)
    tB, zB = toa_sets[BATCH_B.toas]
    mB = SC.model_of(BATCH_B)
    layA0 = build_layout(mA, tA, track_mode="nearest")
    tabs = [pack_table(layA0), pack_table(layA0, mA2)]
    Ms, sigma, phi, ep, _ = timing_columns(mA, tA, tabs)
    from pint_amd.noise import scaled_sigma_us
    rA = np.asarray(zA * sigma, dtype=np.float64)
    rB = zB * scaled_sigma_us(mB, tB) * 1e-6

    def insts(s):
        la = s.add(build_layout(mA, tA, track_mode="nearest"))
        lb = s.add(build_layout(mB, tB, track_mode="nearest"))
        s.set_instances([(la, tabs[0]), (lb, pack_table(lb)), (la, tabs[1])])
        return [la, lb, la]
    lays, dmr, grams, steps, plan = run_batch(insts, lambda l: [l[0]], True, [rA, rB, rA])
    assert plan["wb_gram"]
    _, _, grams0, steps0, plan0 = run_batch(insts, lambda l: [], False, [rA, rB, rA])
    assert not plan0["wb_gram"]
    for k, m in ((0, mA), (2, mA2)):
        check_instance(MIXED_A, m, tA, lays[k], Ms[k // 2], sigma, ep, rA, dmr[k], grams[k], steps[k], f"mixed batch, A[{k}]")
    assert np.array_equal(grams[1][0], grams0[1][0]) and np.array_equal(grams[1][1], grams0[1][1])
    assert all(np.array_equal(a, b) for a, b in zip(steps[1], steps0[1]))
    for res, chi2 in dmr[1].values():
        assert np.all(res == 0) and len(res) == tB.ntoas and np.isnan(chi2)
    # the DM rows did move A's Grams
    assert not np.array_equal(grams[0][0], grams0[0][0]) and not np.array_equal(grams[2][0], grams0[2][0])


def test_grid_like_batch(toa_sets):
    """Four tables of one wideband pulsar through set_instances_of (grid points)."""
    from pint_amd.engine import build_layout, pack_table
    tA, mA, zA, _ = case_data(BATCH_A, toa_sets)
    models = [perturbed(BATCH_A, mA, k) for k in range(4)]
    lay0 = build_layout(mA, tA, track_mode="nearest")
    tabs = [pack_table(lay0, m) for m in models]
    Ms, sigma, phi, ep, _ = timing_columns(mA, tA, tabs)
    rA = np.asarray(zA * sigma, dtype=np.float64)

    def insts(s):
        la = s.add(build_layout(mA, tA, track_mode="nearest"))
        s.set_instances_of(la, np.array(tabs))
        return [la] * 4
    lays, dmr, grams, steps, plan = run_batch(insts, lambda l: [l[0]], True, [rA] * 4)
    assert plan["wb_gram"]
    for k in range(4):
        check_instance(BATCH_A, models[k], tA, lays[k], Ms[k], sigma, ep, rA, dmr[k], grams[k], steps[k], f"grid-like batch, A[{k}]")


def test_dm_resid_alone(toa_sets):
    """k_dm_resid on 37 TOAs (threads without rows), every bin frozen: no compact layout, no fit."""
    from pint_amd.engine import Session, build_layout, pack_table
    c = WB.case("wb_n37", 6, 8, 0, "n300", dmx_free=False, dm_free=("DM1",), ndmjump=5)
    base, _ = toa_sets["n300"]
    toas, model = WB.case_toas(c, base[np.arange(0, 296, 8)])
    assert toas.ntoas == 37
    s = Session()
    try:
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_wideband(lay)
        assert s.fit_layout(lay)[0] == 0
        s.eval(False)
        dmr = read_dm_resids(s)
    finally:
        s.close()
    e_r, e_c2 = check_dm_resids(c, model, toas, dmr)
    print(f"k_dm_resid alone, n 37: dm resid {e_r:.1e} chi2 {e_c2:.1e}")
    assert e_r <= 1e-12 and e_c2 <= 1e-12


@pytest.mark.parametrize("what", ["full_layout", "no_compact_dmx"])
def test_wideband_step_off_the_compact_layout_is_refused(what, toa_sets):
    """pint_fit_step with the wideband rows asked for refuses a design matrix in the full layout,
    and a wideband pulsar that is not on the compact DMX layout (5 free bins), before any
    launch, instead of taking a TOA-only step."""
    from pint_amd import _lib
    from pint_amd.engine import Session, build_layout, pack_table
    c = WB.case("wb_refused", 6, 8 if what == "full_layout" else 5, 0, "n300", dm_free=("DM1",))
    toas, model, z, _ = case_data(c, toa_sets)
    s = Session()
    try:
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_wideband(lay)
        s.set_wbfit(True)
        assert s.fit_layout(lay)[0] == (1 if what == "full_layout" else 0)
        s.eval(want_M=True if what == "full_layout" else Session.FIT)
        with pytest.raises(_lib.PintError) as e:
            s.fit_step(1)
        assert e.value.code == _lib.PINT_E_INVALID
        assert ("compact fit layout" if what == "full_layout" else "compact DMX layout") in str(e.value)
        assert not any(v for k, v in s.last_plan().items() if k != "solve")  # nothing launched
        # the same session still fits without the wideband rows
        s.set_wbfit(False)
        s.fit_step(1)
        assert not s.last_plan()["wb_gram"]
    finally:
        s.close()


def test_a_refused_step_changes_no_state(toa_sets):
    """A refused pint_fit_step between two valid ones (the refusal test's 5-free-bin wideband
    pulsar, the DM rows switched on for the refused call only): the plan it leaves is all-zero,
    not the previous step's, and the next valid step's outputs are bit for bit those of a fresh
    session that never saw the refusal."""
    from pint_amd import _lib
    from pint_amd.engine import Session, build_layout, pack_table
    c = WB.case("wb_refused", 6, 5, 0, "n300", dm_free=("DM1",))
    toas, model, z, _ = case_data(c, toa_sets)

    def valid_step(s):
        s.fit_step(1)
        dp, er, cov, cl = s.read_step()
        return [np.array(dp[0]), np.array(er[0]), np.array(cov[0]), np.array(cl)], s.last_plan()

    def session():
        s = Session()
        lay = s.add(build_layout(model, toas, track_mode="nearest"))
        s.set_instances([(lay, pack_table(lay))])
        s.set_wideband(lay)
        s.eval(want_M=Session.FIT)
        s.debug_set_resids([1e-6 * z])
        return s
    s = session()
    try:
        before, plan = valid_step(s)
        assert any(v for k, v in plan.items() if k != "solve") and np.all(np.isfinite(before[0]))
        s.set_wbfit(True)
        with pytest.raises(_lib.PintError) as e:
            s.fit_step(1)
        assert e.value.code == _lib.PINT_E_INVALID
        refused = s.last_plan()
        assert refused["solve"] == "none" and not any(v for k, v in refused.items() if k != "solve")
        s.set_wbfit(False)
        after, plan_after = valid_step(s)
    finally:
        s.close()
    s = session()
    try:
        fresh, plan_fresh = valid_step(s)
    finally:
        s.close()
    assert plan_after == plan_fresh == plan
    for a, b, f in zip(before, after, fresh):
        assert a.tobytes() == f.tobytes() and b.tobytes() == f.tobytes()


@pytest.fixture(scope="module")
def e2e_toas():
    """Fake TOAs zeroed on each end-to-end case's own model (so that the step is of the order
    of the errors), one batch."""
    from pint_amd.simulation import make_fake_toas_batch
    cs = [c for c in CASES if c.name in WB.E2E]
    toas = make_fake_toas_batch([dict(model=SC.model_of(c), start=SC.MJD0, end=SC.MJD1, ntoas=int(c.toas[1:]),
                                      freq=[800, 1200, 1600, 2000], obs="geocenter", error_us=0.5, add_noise=True,
                                      seed=200 + k) for k, c in enumerate(cs)])
    return {c.name: t for c, t in zip(cs, toas)}


@pytest.mark.parametrize("name", WB.E2E)
def test_end_to_end_against_the_oracle(name, e2e_toas):
    """WidebandTOAFitter.fit_toas(maxiter=1) against the oracle's wideband GLS step (pinned to the
    reference's wb_dd fit) from the same start: parameters 1e-3 sigma, errors 1e-5."""
    from pint_amd import WidebandTOAFitter
    c = {c.name: c for c in CASES}[name]
    toas, model = WB.case_toas(c, e2e_toas[name])
    st = O.wideband_gls_step(*oracle_inputs(model, toas))
    f = WidebandTOAFitter(toas, copy.deepcopy(model))
    f.fit_toas(maxiter=1)
    worst = werr = 0.0
    for j, p in enumerate(st["names"]):
        if p == "Offset":
            continue
        ref = LD(model[p].value) + LD(st["dpars"][j])
        worst = max(worst, abs(float((LD(f.model[p].value) - ref) / LD(st["errs"][j]))))
        werr = max(werr, abs(float(f.model[p].uncertainty / st["errs"][j] - 1)))
    print(f"{name}: end to end worst {worst:.2e} sigma, errors {werr:.2e}")
    assert worst < 1e-3 and werr < 1e-5
