"""Host checks of the shape sweep's builder (shape_cases.py) and longdouble helpers
(ld_util.py): the width arithmetic and the predicted launch plans against a hand-written
table, the built models against their named widths, the helpers against float64 numpy."""
import numpy as np
import pytest

import shape_cases as SC
from ld_util import ld_gram, ld_inverse, ld_solve, ld_woodbury_chi2


def host_toas(n):
    """Unzeroed fake TOAs (host only): evenly spaced, four frequencies."""
    from pint_amd.simulation import _row_arrays, _times_freqs, _tzr
    from pint_amd.toa import TOAs
    base = SC.model_of(SC.Case("base", 8, SC.BASE_NDMX, 30))
    t, f = _times_freqs(SC.MJD0, SC.MJD1, n, [800, 1200, 1600, 2000], False)
    return TOAs(_row_arrays(t, f, 0.5, "geocenter"), {"name": ["fake"] * n}, _tzr(base, "geocenter"), "fake")


def mjd(n):
    return np.linspace(SC.MJD0, SC.MJD1, n)


def test_timing_split():
    assert [SC.timing_split(k) for k in (1, 2, 8, 9, 10, 11, 40)] == [(0, 0), (1, 0), (7, 0), (6, 1), (7, 1),
                                                                      (6, 2), (7, 16)]
    assert np.allclose(SC.wavex_freqs(3) * SC.TSPAN, [2.5, 3.5, 4.5])
    assert np.allclose(SC.wavex_freqs(2, 30) * SC.TSPAN, [30.5, 31.5])


def test_gram_tiles_per_wave():
    # Kp -> T = ceil(nt (nt + 1) / 2 / 16), nt = Kp / 16: the widest nt of every T, the narrowest of 2 and 3
    table = {16: 1, 32: 1, 80: 1, 96: 2, 112: 2, 128: 3, 144: 3, 160: 4, 192: 5, 208: 6, 224: 7, 240: 8, 256: 9}
    assert {kp: SC.gram_T(kp) for kp in table} == table


def test_column_solve_limit():
    assert SC.column_solve_fits(196) and not SC.column_solve_fits(197)


def test_vgram_keys():
    assert SC.vgram_keys_reachable() == [1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 23, 24, 25, 26, 27]


# name -> (K, Gram, nsplit, solve, k_solve_dmx waves, Sigma, k_schur, deferred covariance), by hand
# from the dispatch rules
PLANS = {
    "solve_K4": (4, (1,), 1, "lanes4", 0, "side4", False, False),
    "solve_K5": (5, (1,), 1, "lanes8", 0, "side4", False, False),
    "solve_K8": (8, (1,), 1, "lanes8", 0, "side4", False, False),
    "solve_K9": (9, (1,), 1, "blk1", 0, "side4", False, False),
    "solve_K16": (16, (1,), 1, "blk1", 0, "side4", False, False),
    "solve_K17": (17, (1,), 1, "blk1", 0, "side4", False, False),
    "solve_K32": (32, (1,), 1, "blk1", 0, "side4", False, False),
    "solve_K33": (33, (1,), 1, "blk4", 0, "side4", False, False),
    "solve_K80": (80, (2,), 1, "blk4", 0, "side4", False, False),
    "solve_K81": (81, (2,), 1, "blk16", 0, "side4", False, False),
    "grams_Kp16": (12, "small", 1, "blk1", 0, "side4", False, False),
    "grams_Kp32": (31, "small", 1, "blk1", 0, "side4", False, False),
    "gram_Kp160": (159, (4,), 1, "blk16", 0, "side16", False, False),
    "solve_K192": (192, (6,), 1, "blk16", 0, "side16", False, False),
    "solve_K193": (193, (6,), 1, "column", 0, "side16", False, False),
    "solve_K196": (196, (6,), 1, "column", 0, "side4", False, False),
    "solve_K197_fit": (197, (2,), 1, "none", 8, "fused", False, False),
    "gram_Kp256": (255, (9,), 1, "blk16", 0, "-", False, False),
    "gram_Kp144_ns5": (143, (3,), 5, "blk16", 0, "side4", False, False),
    "vg_R1_nred0": (15, ((1, True),), 1, "none", 8, "-", False, False),
    "vg_R1_nred31": (77, ((5, True),), 1, "none", 8, "fused", False, False),
    "vg_R2_nred16": (58, ((14, True),), 1, "none", 8, "fused", False, False),
    "vg_R3_nred31": (101, ((27, False),), 1, "none", 8, "fused", False, False),
    "vg_R3_nred31_novb": (101, ((27, False),), 1, "none", 8, "fused", False, False),
    "vg_R2_nred16_novb": (58, ((14, False),), 1, "none", 8, "fused", False, False),
    "vg_R3_wt37": (62, ((24, True),), 1, "none", 8, "fused", False, False),
    "vg_off_nred32": (90, (1,), 1, "none", 8, "fused", False, False),
    "dmx_nbd8_d0": (144, (3,), 1, "none", 8, "fused", False, False),
    "dmx_nbd9_d2": (145, (3,), 1, "none", 16, "fused", True, True),
    "dmx_nbd9_d2_noschur": (145, (3,), 1, "none", 16, "fused", False, True),
    "dmx_blk75_nbs9_d2": (166, (4,), 1, "none", 16, "fused", True, True),
    "dmx_nbs10_d0": (174, (4,), 1, "none", 16, "fused", False, False),
    "dmx_blk76_lds": (178, (3,), 1, "blk16", 0, "side16", False, False),
    "dmx_blk77": (186, (5,), 1, "blk16", 0, "side16", False, False),
    "sigma_nred39": (90, (2,), 1, "blk16", 0, "side4", False, False),
    "sigma_nred40": (92, (2,), 1, "blk16", 0, "side16", False, False),
    "sigma_nred95": (192, (6,), 1, "blk16", 0, "side16", False, False),
    "sigma_nred96": (194, (6,), 1, "column", 0, "in-solve", False, False),
    "wfuse_nred64": (156, (3,), 1, "none", 16, "fused", False, False),
}


def test_case_names_are_unique_and_tabled():
    names = [c.name for c in SC.cases()]
    assert len(set(names)) == len(names)
    assert set(PLANS) <= set(names)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_predicted_plan(name):
    c = {c.name: c for c in SC.cases()}[name]
    n = int(c.toas[1:])
    p = SC.predict_plan(c, n, mjd(n))
    K, gram, nsplit, solve, waves, sigma, schur, defer = PLANS[name]
    assert c.K == K
    if gram == "small":
        assert p["gram_s"] and not p["gram_T"] and not p["gram_v"]
    elif isinstance(gram[0], tuple):
        assert p["gram_v"] == gram and not p["gram_T"] and p["greduce"] and not p["dmx_rows"]
    else:
        assert p["gram_T"] == gram and not p["gram_v"] and not p["gram_s"]
    assert (p["nsplit"], p["solve"], p["solve_dmx_waves"]) == (nsplit, solve, waves)
    got = ("fused" if p["fuse_sigma"] else "side%d" % p["sigma_waves"] if p["side_sigma"] else
           "in-solve" if p["do_sigma"] else "-")
    assert got == sigma
    assert (p["schur"], p["cov_deferred"]) == (schur, defer)
    assert p["greduce"] == (nsplit > 1 or bool(p["gram_v"]))


def test_refused_case_predicts_no_launch():
    c = {c.name: c for c in SC.cases()}["solve_K197"]
    p = SC.predict_plan(c, 1100, mjd(1100))
    assert c.K == 197 and p.pop("solve") == "none" and not any(p.values())


def test_predicted_plans_cover_every_target():
    plans = [SC.predict_plan(c, int(c.toas[1:]), mjd(int(c.toas[1:]))) for c in SC.cases()]
    assert set(range(1, 10)) <= {T for p in plans for T in p["gram_T"]}
    keys = {kv for p in plans for kv in p["gram_v"]}
    for k in SC.vgram_keys_reachable():
        assert (k, False) in keys and (k % 10 > 6 or (k, True) in keys), k
    assert {"lanes4", "lanes8", "blk1", "blk4", "blk16", "column"} <= {p["solve"] for p in plans}
    assert {8, 16} <= {p["solve_dmx_waves"] for p in plans} and {4, 16} <= {p["sigma_waves"] for p in plans}
    assert {1, 3, 5} <= {p["nsplit"] for p in plans}


@pytest.mark.parametrize("name", ["solve_K4", "solve_K33", "gram_Kp144", "vg_R3_wt37", "dmx_nbd9_d0",
                                  "vg_R1_nred0", "sigma_nred96", "gram_Kp256"])
def test_built_model_has_the_named_widths(name):
    from pint_amd.engine import build_layout
    c = {c.name: c for c in SC.cases()}[name]
    lay = build_layout(SC.model_of(c), host_toas(64), track_mode="nearest")
    ndmx = sum(1 for n in lay.columns if n.startswith("DMX_"))
    assert (len(lay.columns), ndmx, lay.nred, lay.K) == (c.ncol, c.ndmx_free, c.nred, c.K)
    assert lay.columns[0] == "Offset"
    nwx = SC.timing_split(c.ntim)[1]
    if nwx:
        f = np.array([float(lay.model[f"WXFREQ_{i + 1:04d}"].value) for i in range(nwx)]) * SC.TSPAN
        assert np.allclose(f, max(c.nred, 2) + np.arange(nwx) + 0.5, rtol=0, atol=1e-9)


def test_dmx_rows_follow_the_ranges():
    d = SC.dmx_rows(mjd(530), 20)
    assert d[0] == 0 and d[-1] == 19 and np.all(np.diff(d) >= 0) and len(set(d)) == 20


@pytest.mark.parametrize("n", [1, 5, 40])
def test_ld_solve_and_inverse_against_float64(n):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n + 3, n))
    A = B.T @ B + np.eye(n)
    b = rng.standard_normal(n)
    x = ld_solve(A, b)
    assert x.dtype == np.longdouble
    assert np.max(np.abs(x.astype(float) - np.linalg.solve(A, b))) <= 1e-12 * np.max(np.abs(x))
    X = ld_inverse(A)
    assert np.max(np.abs(X.astype(float) - np.linalg.inv(A))) <= 1e-12 * np.max(np.abs(X))
    assert float(np.max(np.abs(np.asarray(A, dtype=np.longdouble) @ X - np.eye(n)))) <= 1e-16 * n * np.linalg.cond(A)


def test_ld_gram_and_woodbury_against_float64():
    rng = np.random.default_rng(3)
    n, k = 50, 6
    M, r = rng.standard_normal((n, k)), rng.standard_normal(n)
    sigma = rng.uniform(0.5, 2, n)
    G, cs = ld_gram(M, r, sigma)
    X = np.concatenate([M, r[:, None]], axis=1)
    assert np.allclose(G.astype(float), X.T @ (X / sigma[:, None] ** 2), rtol=1e-13, atol=0)
    assert np.allclose(cs.astype(float), (M * M).sum(0), rtol=1e-14)
    phi = rng.uniform(0.1, 3, k)
    c2, rNr = ld_woodbury_chi2(r, sigma, M, phi)
    Cm = np.diag(sigma ** 2) + M @ np.diag(phi) @ M.T
    assert abs(float(c2) / (r @ np.linalg.solve(Cm, r)) - 1) <= 1e-12
    assert abs(float(rNr) / np.sum((r / sigma) ** 2) - 1) <= 1e-14
