"""Host checks of the ECORR sweep's builder (ecorr_cases.py, shape_cases.py's ECORR fields): the
sets' epoch sizes and counts from the row arithmetic and from the layout's own ep_ptr / ep_idx,
the properties the sweep's targets rest on (set_properties, which test_ecorr_sweep.py asserts
again on what it uploads), the built models' widths, and the predicted plans against a table
written by hand from the dispatch rules."""
import numpy as np
import pytest

import ecorr_cases as EC
import shape_cases as SC

CASES = {c.name: c for c in EC.cases()}
_LAY = {}


def layout_of(c):
    from pint_amd.engine import build_layout
    if c.name not in _LAY:
        toas = EC.toa_set(c.toas).toas()
        _LAY[c.name] = (build_layout(SC.model_of(c), toas, track_mode="nearest"), toas)
    return _LAY[c.name]


def epochs_of(lay):
    return [lay.ep_idx[lay.ep_ptr[e]:lay.ep_ptr[e + 1]] for e in range(lay.nep)]


def set_properties(c, lay, toas):
    """The "never run" items the case's upload shows, from the layout's own epoch lists and
    shape_cases.free_rows (nothing assumed from the builder)."""
    ep = epochs_of(lay)
    size = np.array([len(e) for e in ep])
    inep = np.zeros(toas.ntoas, dtype=int)
    for e in ep:
        inep[e] += 1
    p = set()
    if size.max() > 64:
        p.add("epoch > 64 rows")
    if np.any(size % 4):
        p.add("size % 4")
    if lay.nep % 4:
        p.add("epoch count % 4")
    if any(np.any(np.diff(e) != 1) for e in ep):
        p.add("ep_idx not contiguous")
    if np.any(inep == 0):
        p.add("rows in no epoch")
    if lay.nep > 256:
        p.add("> 256 epochs")
    if len(set(size)) > 1:
        p.add("uneven sizes")
    if np.any(inep > 1):
        p.add("TOA in two epochs")
    if len(set(lay.ep_param)) > 1:
        p.add("two ECORR parameters")
        t = np.asarray(toas.tdbld, dtype=np.float64)
        first = {(round(float(t[e].min()) * 86400) // 2, q) for e, q in zip(ep, lay.ep_param)}
        if len({k for k, _ in first}) < len(first):
            p.add("two epochs at one time")
    if c.layout == "fit" and c.ndmx_free >= 8:
        drow = SC.free_rows(c, toas.arrays["mjd_float"])
        bins = [set(drow[e][drow[e] >= 0]) for e in ep]
        if any(len(b) > 1 for b in bins):
            p.add("epoch in two free bins")
        else:
            per = np.bincount([min(b) for b in bins if b], minlength=c.ndmx_free)
            if any(not b for b in bins):
                p.add("ep_bin = -1")
            if any(b and np.any(drow[e] < 0) for b, e in zip(bins, ep)):
                p.add("drow < 0 in a binned epoch")
            if per.max() > 64:
                p.add("bin > 64 epochs")
            if np.any(per % 4):
                p.add("epochs per bin % 4")
            if np.any(per == 0):
                p.add("bin with no epoch")
            if c.ndense + 2 * c.nred > 63:
                p.add("Kd > 63")
    return p


def test_set_sizes_from_the_row_arithmetic():
    mix = EC.toa_set("mix")
    assert mix.sizes() == list(EC.SIZES) * 2 and mix.n == sum(EC.SIZES) * 2 + EC.NSLOT * 4 // 3 == 1166
    assert sorted(set(EC.SIZES)) == [2, 3, 4, 5, 7, 63, 64, 65, 70] and list(EC.SIZES) != sorted(EC.SIZES)
    assert len(mix.sizes()) % 4 == 2
    assert np.all(np.diff(mix.t) > 0) and mix.n <= 1200
    # slots: lone -g A rows, lone -g N rows and -g N pairs, a third each, over the whole span
    lone = mix.ep < 0
    assert np.sum(lone & (mix.g == "A")) == 150 and np.sum(lone & (mix.g == "N")) == 450
    assert float(mix.t[lone].min()) < SC.MJD0 + 5 and float(mix.t[lone].max()) > SC.MJD1 - 5
    sh = EC.toa_set("mix_shuffled")
    assert sorted(sh.t) == sorted(mix.t) and np.any(np.diff(sh.t) < 0) and sh.sizes() == mix.sizes()
    sm = EC.toa_set("mix_small")
    assert sm.sizes() == [5, 64, 2, 70, 3] and sm.n == 144 + 300 <= SC.GS_MAXN
    two = EC.toa_set("two")
    assert sorted(two.sizes("A") + two.sizes("B")) == sorted([5, 64, 2, 70, 3, 65, 7, 63, 4, 5, 64, 2, 35, 35, 3, 65, 7, 63, 4])
    assert len(two.sizes("A")) == 9 and len(two.sizes("B")) == 10
    many = EC.toa_set("many")
    assert len(many.sizes()) == sum(EC.MANY_COUNTS) == 262 >= 261 and set(many.sizes()) == {2, 3}
    assert max(EC.MANY_COUNTS) >= 69 and 0 in EC.MANY_COUNTS and EC.MANY_COUNTS[EC.MANY_FROZEN[0]] > 0
    assert many.n <= 1200 and np.all(np.diff(many.t) > 0)
    # every cluster is more than 10 s from the next: no slot joins an epoch
    for s in (mix, many):
        first = np.concatenate([[True], (s.ep[1:] != s.ep[:-1]) | (s.sl[1:] != s.sl[:-1])])
        assert float(np.min(np.diff(s.t[first]))) * 86400 > 10


@pytest.mark.parametrize("name", ["mix", "mix_shuffled", "mix_small", "two", "many"])
def test_layout_epochs_are_the_designed_ones(name):
    """noise.ecorr_epochs on the built TOAs (through build_layout) finds the designed epochs, per
    parameter, and nothing else: no lone row, no unflagged pair."""
    c = next(c for c in EC.cases() if c.toas == name and not c.refused and not c.dmx_edge)
    lay, toas = layout_of(c)
    s = EC.toa_set(name)
    want = [(f"ECORR{k + 1}", tuple(rows)) for k, (_, v, _) in enumerate(c.ecorr_par) for rows in s.designed(v)]
    got = [(q, tuple(e)) for q, e in zip(lay.ep_param, epochs_of(lay))]
    assert got == want
    assert [float(x) for x in lay.ep_phi] == [(dict((f"ECORR{k + 1}", x) for k, (_, _, x) in enumerate(c.ecorr_par))[q] * 1e-6) ** 2
                                            for q in lay.ep_param]


# name -> the properties its upload must show
PROPS = {
    "ec_T1": {"epoch > 64 rows", "size % 4", "epoch count % 4", "rows in no epoch", "uneven sizes"},
    "ec_fit_shuf": {"ep_idx not contiguous", "epoch > 64 rows", "size % 4"},
    "ec_fit_many": {"> 256 epochs", "uneven sizes", "ep_bin = -1", "bin > 64 epochs", "epochs per bin % 4", "bin with no epoch"},
    "ec_fit_two": {"two ECORR parameters", "two epochs at one time", "rows in no epoch"},
    "ec_fit_Kd68": {"Kd > 63", "epoch > 64 rows"},
    "ec_fit_frozen": {"ep_bin = -1", "drow < 0 in a binned epoch"},
    "ec_straddle": {"epoch in two free bins"},
    "ec_overlap": {"TOA in two epochs", "two ECORR parameters"},
    "ec_small": {"epoch > 64 rows", "size % 4"},
}


@pytest.mark.parametrize("name", sorted(PROPS))
def test_set_properties(name):
    c = CASES[name]
    lay, toas = layout_of(c)
    got = set_properties(c, lay, toas)
    assert PROPS[name] <= got, PROPS[name] - got
    if name not in ("ec_overlap",):
        assert "TOA in two epochs" not in got
    if name not in ("ec_straddle", "ec_overlap"):
        assert "epoch in two free bins" not in got


def test_many_bins():
    c = CASES["ec_fit_many"]
    lay, toas = layout_of(c)
    drow = SC.free_rows(c, toas.arrays["mjd_float"])
    per = np.zeros(c.ndmx_free, dtype=int)
    none = 0
    for e in epochs_of(lay):
        b = set(drow[e])
        assert len(b) == 1
        if min(b) < 0:
            none += 1
        else:
            per[min(b)] += 1
    # the free bins in order (bin 3 frozen: its 24 epochs have no bin); 70 in one bin, none in another
    assert list(per) == [25, 70, 23, 26, 0, 25, 23, 24, 22] and none == 24
    assert np.all(np.bincount(drow[drow >= 0]) >= 36)  # every free bin keeps rows in no epoch


def test_straddled_epoch():
    a, x = EC.straddle_edge()
    c = CASES["ec_straddle"]
    lay, toas = layout_of(c)
    b = SC.bin_rows(c, toas.arrays["mjd_float"])
    split = [e for e in epochs_of(lay) if len(set(b[e])) > 1]
    assert len(split) == 1 and len(split[0]) == 70
    assert list(b[split[0]]) == [a] * 35 + [a + 1] * 35
    # mjd_float resolves the 0.01 s between the rows
    assert np.all(np.diff(toas.arrays["mjd_float"][split[0]]) > 0)
    assert CASES["ec_fit_frozen"].dmx_frozen == (a + 1,)


# name -> (K, Gram, ECORR Gram, N-splits, k_dmx_rows, k_dmx, k_ecorr_dmx, solve, Sigma, k_schur + deferred), by hand
# from the dispatch rules
PLANS = {
    "ec_T1": (79, (1,), True, 1, False, False, False, "blk4", "side4", False),
    "ec_T4": (159, (4,), True, 1, False, False, False, "blk16", "side16", False),
    "ec_T5": (191, (5,), True, 1, False, False, False, "blk16", "side16", False),
    "ec_T6": (196, (6,), True, 1, False, False, False, "column", "side16", False),
    "ec_T4_ns3": (159, (4,), True, 3, False, False, False, "blk16", "side16", False),
    "ec_small": (24, "small+T1", True, 1, False, False, False, "blk1", "side4", False),
    "ec_fit_mix": (28, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_fit_mix_red_d2": (60, (1,), True, 1, True, False, True, 8, "fused", True),
    "ec_fit_shuf": (44, (1,), True, 1, True, True, True, 8, "fused", False),
    "ec_fit_shuf_d2": (28, (1,), True, 1, True, True, True, 8, "fused", True),
    "ec_fit_many": (17, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_fit_many_red_d2": (41, (1,), True, 1, True, False, True, 8, "fused", True),
    "ec_fit_two": (44, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_fit_two_d2": (28, (1,), True, 1, True, False, True, 8, "fused", True),
    "ec_fit_Kd68": (88, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_fit_frozen": (43, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_ones_full": (48, (1,), True, 1, False, False, False, "blk4", "side4", False),
    "ec_ones_fit": (48, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_ones_fit_dmn": (56, (1,), True, 1, True, False, True, 8, "fused", False),
    "ec_ones_full_dmn": (56, (1,), True, 1, False, False, False, "blk4", "side4", False),
    "ec_straddle": (44, (1,), True, 1, False, False, False, "blk4", "side4", False),
    "ec_wls": (44, (1,), False, 1, False, False, False, "blk1", "-", False),
}


def test_case_names_are_unique_and_tabled():
    names = [c.name for c in EC.cases()]
    assert len(set(names)) == len(names)
    assert set(PLANS) | {"ec_overlap"} == set(names)
    import wb_cases as WB
    assert not set(names) & ({c.name for c in SC.cases()} | {c.name for c in WB.cases()})


@pytest.mark.parametrize("name", sorted(PLANS))
def test_predicted_plan(name):
    c = CASES[name]
    lay, toas = layout_of(c)
    p = SC.predict_plan(c, toas.ntoas, toas.arrays["mjd_float"])
    K, gram, ecorr, nsplit, rows, gather, ecorr_dmx, solve, sigma, defer = PLANS[name]
    assert (c.K, lay.K, len(lay.columns), lay.nred) == (K, K, c.ncol, c.nred)
    assert ("Offset" in lay.columns) == (not c.phoff)
    if gram == "small+T1":
        assert p["gram_s"] and p["gram_T"] == (1,) and toas.ntoas <= SC.GS_MAXN
    else:
        assert p["gram_T"] == gram and not p["gram_s"]
    assert not p["gram_v"] and not p["wb_gram"]
    assert (p["gram_ecorr"], p["nsplit"], p["dmx_rows"], p["dmx"], p["ecorr_dmx"]) == (ecorr, nsplit, rows, gather, ecorr_dmx)
    assert p["greduce"] == (nsplit + ecorr > 1)
    if isinstance(solve, int):
        assert (p["solve"], p["solve_dmx_waves"]) == ("none", solve)
    else:
        assert (p["solve"], p["solve_dmx_waves"]) == (solve, 0)
    got = ("fused" if p["fuse_sigma"] else "side%d" % p["sigma_waves"] if p["side_sigma"] else
           "in-solve" if p["do_sigma"] else "-")
    assert got == sigma
    assert (p["schur"], p["cov_deferred"]) == (defer, defer)


def test_gram_widths_follow_gram_maxkp():
    for T, kp in EC.GRAM_MAXKP.items():
        assert SC.gram_T(kp) == T and SC.gram_T(kp + 16) == T + 1
    for T in (1, 4, 5, 6):
        c = CASES[f"ec_T{T}"]
        assert SC._pad16(c.K + 1) == EC.GRAM_MAXKP[T] and c.K <= EC.K_MAX


def test_refused_case_predicts_no_launch():
    c = CASES["ec_overlap"]
    lay, toas = layout_of(c)
    p = SC.predict_plan(c, toas.ntoas, toas.arrays["mjd_float"])
    assert p.pop("solve") == "none" and not any(p.values())
    assert lay.ep_overlap and not layout_of(CASES["ec_fit_two"])[0].ep_overlap


def test_predicted_plans_cover_every_target():
    plans = []
    for c in EC.cases():
        lay, toas = layout_of(c)
        plans.append(SC.predict_plan(c, toas.ntoas, toas.arrays["mjd_float"]))
    ec = [p for p in plans if p["gram_ecorr"]]
    assert {1, 4, 5, 6} <= {T for p in ec for T in p["gram_T"]}
    assert any(p["gram_s"] for p in ec)
    assert {p["ecorr_dmx"] for p in ec} == {False, True}
    assert any(p["dmx"] and p["ecorr_dmx"] for p in ec)
    assert any(p["fuse_sigma"] for p in ec) and any(p["side_sigma"] for p in ec) and any(p["cov_deferred"] for p in ec)
    assert any(p["nsplit"] == 3 for p in ec)


def test_existing_cases_predict_what_they_did():
    """The ECORR fields are defaulted: the shape sweep's ECORR cases keep their par line."""
    c = {c.name: c for c in SC.cases()}["ecorr_Kp112"]
    assert SC.par_of(c).count("ECORR") == 1 and "ECORR -f fake 0.5" in SC.par_of(c)
    assert "PHOFF" not in SC.par_of(c) and "TNDM" not in SC.par_of(c)


def test_lnl_pars():
    from pint_amd.noisefit import likelihood_kind
    from pint_amd.timing_model import get_model
    for kind in (0, 1, 2):
        m = get_model(EC.lnl_par(kind, EC.EC_AB))
        if kind == 1:
            m.free_params = list(m.free_params)
            assert "PHOFF" in m.free_params
        assert likelihood_kind(m) == kind and len(m.mask_params("ECORR")) == (2 if kind else 0)


def test_ld_block_likelihood_against_float64():
    from ld_util import ld_block_likelihood, ld_ecorr_eliminate, ld_gram
    rng = np.random.default_rng(11)
    n = 40
    r, N = rng.standard_normal(n), rng.uniform(0.5, 2, n)
    ep = [(np.array([3, 4, 9]), 0.7), (np.arange(20, 31), 1.9)]
    C = np.diag(N)
    dC = np.zeros((n, n))
    for idx, ph in ep:
        C[np.ix_(idx, idx)] += ph
        dC[np.ix_(idx, idx)] += 1
    d = rng.uniform(0, 1, n)
    chi2, ld, grads, ones = ld_block_likelihood(r, N, ep, dN=[d], dphi=[np.ones(2)])
    Ci = np.linalg.inv(C)
    assert abs(float(chi2) / (r @ Ci @ r) - 1) <= 1e-12
    assert abs(float(ld) / (0.5 * np.linalg.slogdet(C)[1]) - 1) <= 1e-12
    for (g, _), dc in zip(grads, (np.diag(d), dC)):
        assert abs(float(g) - (0.5 * r @ Ci @ dc @ Ci @ r - 0.5 * np.trace(Ci @ dc))) <= 1e-11
    assert abs(float(ones[0]) - np.sum(Ci @ r)) <= 1e-12 and abs(float(ones[1]) - np.sum(Ci)) <= 1e-12
    # the elimination: disjoint epochs by the diagonal form, overlapping ones densely, both against
    # the dense float64 Schur complement
    M = rng.standard_normal((n, 4))
    sig = np.sqrt(N)
    G, _ = ld_gram(M, r, sig)
    X = np.concatenate([M, r[:, None]], axis=1)
    for eps in (ep, ep + [(np.array([4, 25, 33]), 0.4)]):
        E = np.zeros((n, len(eps)))
        for e, (idx, _) in enumerate(eps):
            E[idx, e] = 1
        S = E.T @ (X / N[:, None])
        SigE = E.T @ (E / N[:, None]) + np.diag([1 / ph for _, ph in eps])
        want = X.T @ (X / N[:, None]) - S.T @ np.linalg.solve(SigE, S)
        got = ld_ecorr_eliminate(G, X, sig, eps)[0]
        assert np.max(np.abs(got.astype(float) - want)) <= 1e-11 * np.max(np.abs(want))
