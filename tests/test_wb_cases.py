"""Host checks of the wideband sweep's builder (shape_cases.py's wideband fields, wb_cases.py):
the built models against a hand-written table (dense column order, m, the free and frozen bin
maps), the predicted plans, and the host longdouble DM model, DM design matrix and scaled DM
errors against the oracle (pinned to the reference's wb_dd fixture)."""
import numpy as np
import pytest

import pint_oracle as O
import shape_cases as SC
import wb_cases as WB
from test_shape_cases import host_toas

TIM6 = ["Offset", "RAJ", "DECJ", "PMRA", "F0", "F1"]
TIM8 = ["Offset", "PX", "RAJ", "DECJ", "PMRA", "PMDEC", "F0", "F1"]
# name -> (dense columns in order, m, free bins (1-based DMX numbers), frozen bins), by hand
TABLE = {
    "wb_m0_b8": (TIM6, 0, list(range(1, 9)), []),
    "wb_m1_b9": (TIM6 + ["DM1"], 1, list(range(1, 10)), []),
    "wb_m3_b10": (TIM6 + ["DM", "DM1", "DM2"], 3, [2, 3, 5, 6, 8, 9, 11, 12, 14, 15], [1, 4, 7, 10, 13]),
    "wb_m8_b11": (TIM6 + ["DM", "DM1", "DM2", "DMJUMP1", "DMJUMP2", "DMJUMP3", "DMJUMP4", "DMJUMP5"], 8,
                  [1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13], [2, 8, 14]),
    "wb_dm12_b21": (TIM6 + ["DM1", "DM2"], 2, [b for b in range(1, 23) if b != 6], [6]),
    "wb_dmjgap_grams": (TIM6 + ["DMJUMP1", "DMJUMP3"], 2, list(range(1, 9)), []),
    "wb_dm12zero": (TIM6 + ["DM1", "DM2"], 2, list(range(2, 12)), [1, 12]),
    "wb_shuffle": (TIM6 + ["DM", "DM1", "DM2", "DMJUMP1", "DMJUMP2"], 5, [2, 3, 5, 6, 8, 9, 11, 12], [1, 4, 7, 10]),
    "wb_vb": (TIM6 + ["DM", "DM1", "DM2", "DMJUMP1", "DMJUMP3"], 5, [b for b in range(1, 25) if b not in (3, 10, 17, 24)],
              [3, 10, 17, 24]),
    "wb_dmx16": (TIM8 + ["DM1", "DMJUMP2", "DMJUMP3"], 3, list(range(1, 17)), []),
    "wb_blk77": (TIM8 + ["DMJUMP1", "DMJUMP2"], 2, list(range(1, 17)), []),
    "wb_ecorr": (TIM6 + ["DM1", "DMJUMP1", "DMJUMP2"], 3, list(range(1, 21)), []),
}
CASES = {c.name: c for c in WB.cases()}
_TOAS = {}


def toas_of(c, n=None):
    key = (c.toas, n)
    if key not in _TOAS:
        _TOAS[key] = host_toas(n or int(c.toas[1:]))
    return WB.case_toas(c, _TOAS[key])


def test_case_names_are_unique_and_tabled():
    names = [c.name for c in WB.cases()]
    assert len(set(names)) == len(names) and set(TABLE) <= set(names) and set(WB.E2E) <= set(names)
    assert not set(names) & {c.name for c in SC.cases()}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_built_model_against_the_table(name):
    from pint_amd.engine import build_layout
    c = CASES[name]
    dense, m, free, frozen = TABLE[name]
    toas, model = toas_of(c, 64)
    lay = build_layout(model, toas, track_mode="nearest")
    cols = list(lay.columns)
    # the model's order: the DMJUMPs follow the DMX block, so their compact (dense) column index
    # differs from their index in the full layout
    head = [n for n in dense if not n.startswith("DMJUMP")]
    assert cols == head + [f"DMX_{b:04d}" for b in free] + dense[len(head):]
    assert (c.m_dm, c.ndense, c.ndmx_free, c.ncol, c.K) == (m, len(dense), len(free), len(cols), lay.K)
    # every frozen bin keeps a non-zero value; every DMJUMP, free or frozen, as well
    assert sorted(free + frozen) == list(range(1, c.ndmx + 1))
    assert all(float(model[f"DMX_{b:04d}"].value) != 0 and model[f"DMX_{b:04d}"].frozen for b in frozen)
    jumps = model.mask_params("DMJUMP")
    assert len(jumps) == c.ndmjump and all(float(model[j].value) != 0 for j in jumps)
    assert [j for j in jumps if model[j].frozen] == [jumps[k] for k in c.dmj_frozen]
    # the DM-type columns' kinds and table indices as k_wb_gram reads them: Taylor order, mask bit
    from pint_amd import _lib as L
    for j, n in enumerate(cols):
        kind, idx = lay.spec.col_kind[j], lay.spec.col_index[j]
        if n in WB.ALL_DM:
            assert (kind, idx) == (L.COL_DM, WB.ALL_DM.index(n))
        elif n.startswith("DMJUMP"):
            assert (kind, idx) == (L.COL_ZERO, int(n[6:]) - 1)


def test_free_and_frozen_bin_maps():
    c = CASES["wb_m3_b10"]
    mjd = np.linspace(SC.MJD0, SC.MJD1, 530)
    b, f = SC.bin_rows(c, mjd), SC.free_rows(c, mjd)
    assert b.min() == 0 and b.max() == 14 and np.all(np.diff(b) >= 0)
    # model bins 0, 3, 6, ... are frozen: no compact column; 1, 2, 4, 5, ... are columns 0, 1, 2, 3, ...
    assert np.all(f[b % 3 == 0] == -1)
    assert np.all(f[b % 3 != 0] == (b - b // 3 - 1)[b % 3 != 0])
    assert sorted(set(f)) == list(range(-1, 10))
    # without frozen bins the sweep's own map
    c0 = CASES["wb_m1_b9"]
    assert np.array_equal(SC.free_rows(c0, mjd), SC.dmx_rows(mjd, 9)) and np.array_equal(SC.bin_rows(c0, mjd), SC.dmx_rows(mjd, 9))


def test_one_toa_bin():
    c = CASES["wb_dm12_b21"]
    mjd = np.linspace(SC.MJD0, SC.MJD1, 530)
    b, f = SC.bin_rows(c, mjd), SC.free_rows(c, mjd)
    assert np.sum(b == 2) == 1 and np.sum(f == 2) == 1
    assert np.sum(b == -1) == 23 and np.sum(f == -1) == 23 + np.sum(b == 5)  # bin 2's other TOAs; the frozen bin
    cnt = np.bincount(f[f >= 0])
    assert len(cnt) == 21 and cnt.min() == 1 and sorted(cnt)[1] >= 24


def test_orders():
    c = CASES["wb_shuffle"]
    mjd = np.linspace(SC.MJD0, SC.MJD1, 530)
    for order, contig in (("", True), ("reverse", True), ("shuffle", False)):
        cc = c.but(order=order)
        idx = WB.order_index(cc, 530)
        assert sorted(idx) == list(range(530))
        assert SC.rows_contiguous(SC.free_rows(cc, mjd[idx]), cc.ndmx_free) == contig


# name -> (Gram, N-splits, k_dmx_rows, k_dmx, k_ecorr_dmx, solve), by hand from the dispatch rules
PLANS = {
    "wb_m0_b8": (((1, True),), 1, False, False, False, 8),
    "wb_m8_b11": (((14, True),), 1, False, False, False, 8),
    "wb_dmjgap_grams": ("small", 1, True, False, False, 8),
    "wb_shuffle": ((1,), 1, True, True, False, 8),
    "wb_shuffle_ns3": ((1,), 3, True, True, False, 8),
    "wb_reverse": (((13, True),), 1, False, False, False, 8),
    "wb_novb": (((14, False),), 1, False, False, False, 8),
    "wb_novg_ns3": ((1,), 3, True, False, False, 8),
    "wb_vb_ns5": (((14, True),), 5, False, False, False, 8),
    "wb_dmx8_d2": ((3,), 1, True, False, False, 8),
    "wb_dmx16": ((3,), 1, True, False, False, 16),
    "wb_blk77": ((5,), 1, True, False, False, "blk16"),
    "wb_ecorr": ((1,), 1, True, False, True, 8),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_predicted_plan(name):
    c = CASES[name]
    n = int(c.toas[1:])
    mjd = np.linspace(SC.MJD0, SC.MJD1, n)[WB.order_index(c, n)]
    p = SC.predict_plan(c, n, mjd)
    gram, nsplit, rows, gather, ecorr_dmx, solve = PLANS[name]
    assert p["wb_gram"]
    if gram == "small":
        assert p["gram_s"] and not p["gram_T"] and not p["gram_v"]
    elif isinstance(gram[0], tuple):
        assert p["gram_v"] == gram and not p["gram_T"] and p["greduce"]
    else:
        assert p["gram_T"] == gram and not p["gram_v"] and not p["gram_s"]
    assert (p["nsplit"], p["dmx_rows"], p["dmx"], p["ecorr_dmx"], p["gram_ecorr"]) == (nsplit, rows, gather, ecorr_dmx, ecorr_dmx)
    if solve == "blk16":
        assert (p["solve"], p["solve_dmx_waves"], p["side_sigma"]) == ("blk16", 0, True)
    else:
        assert (p["solve"], p["solve_dmx_waves"], p["fuse_sigma"]) == ("none", solve, c.nred > 0)
    assert (p["cov_deferred"], p["schur"]) == (c.cov_defer == 2, c.cov_defer == 2 and c.schur)


def test_sweep_cases_predict_no_wideband_rows():
    for c in SC.cases():
        n = int(c.toas[1:])
        p = SC.predict_plan(c, n, np.linspace(SC.MJD0, SC.MJD1, n))
        assert not p["wb_gram"] and not p["dmx"] and not p["ecorr_dmx"]


@pytest.mark.parametrize("name", ["wb_m8_b11", "wb_dm12_b21", "wb_dm12zero", "wb_shuffle", "wb_vb", "wb_ecorr"])
def test_host_dm_model_against_the_oracle(name):
    """DM_model, M_dm and the scaled DM errors in longdouble from the par values against the
    oracle's total_dm, dm_designmatrix and scaled_dm_sigma: 1e-15 relative."""
    from pint_amd.engine import build_layout
    c = CASES[name]
    toas, model = toas_of(c)
    cols = list(build_layout(model, toas, track_mode="nearest").columns)
    om, ot = O.from_product_model(model), O.toas_from_product(toas)
    ot["pp_dm"], ot["pp_dme"] = toas.get_dms(), toas.get_dm_errors()
    dm = WB.dm_model(c, model, toas)
    assert float(np.max(np.abs(O.total_dm(om, ot) / dm - 1))) <= 1e-15
    Md, Mo = WB.dm_design(c, model, cols, toas), O.dm_designmatrix(om, cols, ot)
    assert np.array_equal(Md != 0, Mo != 0)
    nz = Md != 0
    assert float(np.max(np.abs(Mo[nz] / Md[nz] - 1))) <= 1e-15
    assert np.all(Md[:, 0] == 0) and all(np.all(Md[:, j] == 0) for j, n in enumerate(cols) if n in TIM8)
    assert float(np.max(np.abs(O.scaled_dm_sigma(om, ot) / WB.scaled_dm_errors(c, toas) - 1))) <= 1e-15
    # the data: pp_dm - DM_model = z dm_sigma to float64 rounding of pp_dm, errors spread by ~5
    z = (np.asarray(toas.get_dms(), dtype=WB.LD) - dm) / WB.scaled_dm_errors(c, toas)
    assert float(np.max(np.abs(z - WB.dm_noise(toas.ntoas)[WB.order_index(c, toas.ntoas)]))) < 1e-11
    e = toas.get_dm_errors()
    assert e.max() / e.min() > 4.5 and toas.is_wideband()
    # a TOA subset lies in two DMJUMP masks
    if c.ndmjump >= 2:
        assert np.any(sum(WB.selected(toas, k, v).astype(int) for k, v in SC.DMJ_KEYS[:c.ndmjump]) >= 2)


def test_attach_wideband_round_trips():
    from pint_amd.simulation import attach_wideband
    t = host_toas(5)
    dm = np.array([3.1, 3.1 + 2 ** -50, 1e-4 / 3, 12.5, np.pi])
    attach_wideband(t, dm, dm * 1e-4, {"fe": list("ABCDA")})
    assert np.array_equal(t.get_dms(), dm) and np.array_equal(t.get_dm_errors(), dm * 1e-4)
    assert t.flag_columns["fe"] == tuple("ABCDA") and t.flag_columns["name"] == ("fake",) * 5
    with pytest.raises(ValueError):
        attach_wideband(t, dm[:4], dm[:4])
