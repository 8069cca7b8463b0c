"""The host side of the photon-event path (pint_amd/eventstats.py, event_optimize.py, event_toas.py)
against values recorded from the reference (scripts/refgen/gen_photon.py: eventstats, scripts.event_optimize),
and the refusals.  No GPU.

Bars.  Statistics, survival functions and templates: 1e-12 relative (the same expressions in float64 on
both sides; sums of <= 1500 terms).  get_event_TOAs against the packed columns: the TDB within 1 ns at
the geocenter, tests/test_prep.py's bar for UTC -> TT -> TDB (a longdouble MJD near 55000 has an ulp of
2^-48 d = 0.31 ns, which the recorded TT and TDB each carry; the times go TT -> UTC parts -> TT through
prep.prepare), and exactly at the barycentre (TDB in, TDB out); positions within 1 m, velocities within
1e-6 km/s.
"""
import io

import numpy as np
import pytest

from photon_util import NAMES, load, spread

LD = np.longdouble
REL = 1e-12


def close(a, b, rel=REL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rel * np.abs(b))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """What the tests rely on, on the committed files."""
    model, toas, z, meta = load(name)
    n, L = (1500, 256) if name == "photon_geo" else (256, 100)
    assert toas.ntoas == n and z["tmpl"].shape == (L,) and meta["nbin"] == L
    assert np.all(np.isinf(toas.get_freqs())) and np.all(toas.get_errors() == 1.0)
    assert ("weights" in z) == (name == "photon_geo") == meta["weighted"]
    assert ("AbsPhase" in model.components) == meta["abs_phase"] == (name == "photon_geo")
    assert meta["labels"][-1] == "PHASE" and z["pts_hi"].shape == (16, len(meta["labels"]))
    assert np.isclose(z["tmpl"].mean(), 1.0, rtol=1e-14)
    ph = z["pts_hi"][:, -1]
    assert np.all((ph >= 0) & (ph <= 1))
    edge = (L - 1.0) / L
    for k in range(16):
        x = (z["pt_phase"][k] + ph[k]) % 1
        assert np.min(np.abs(x - edge)) > 1e-6          # no photon on the step of the last node
        assert np.count_nonzero(x > edge) >= 3          # the constant last segment is exercised
    assert np.all((z["pt_phase"] >= 0) & (z["pt_phase"] < 1))
    assert np.allclose(z["pt_post"][:, 0], z["pt_post"][:, 1] + z["pt_post"][:, 2], rtol=1e-13)
    assert np.array_equal(z["pt_post"][:, 2], z["pt_lnl"]) and np.all(np.isfinite(z["pt_post"]))
    sp = spread()[name]
    for lev in ("5ps", "30ps"):
        assert np.asarray(sp[lev]["lnl"]).shape == (16,) and np.all(np.asarray(sp[lev]["lnl"]) > 0)
        assert np.asarray(sp[lev]["S"]).shape == (16, 40) and np.asarray(sp[lev]["z2"]).shape == (16, 20)
    assert sp["ref_seconds_per_lnposterior"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_statistics_against_reference(name):
    from pint_amd import eventstats as es
    _, _, z, meta = load(name)
    w = z.get("weights")
    wt = np.ones(z["pt_phase"].shape[1]) if w is None else w
    for k in range(16):
        ph = z["pt_phase"][k]
        assert close(es.z2m(ph, 20), z["pt_z2m"][k]) and close(es.z2mw(ph, wt, 20), z["pt_z2mw"][k])
        assert close(es.hm(ph), z["pt_hm"][k]) and close(es.hmw(ph, wt), z["pt_hmw"][k])
        assert close(es.hm(ph, m=20, c=4), z["pt_hm"][k])
        ak, bk = es.em_four(ph, 20, weights=w)
        assert close(ak, z["pt_ak"][k]) and close(bk, z["pt_bk"][k])
    # ... and from ready-made sums, batched
    sums = np.array([es.trig_sums(z["pt_phase"][k], 20, w) for k in range(16)])
    assert sums.shape == (16, 42)
    assert close(es.z2mw(None, None, 20, sums=sums), z["pt_z2mw"]) and close(es.hmw(None, None, sums=sums), z["pt_hmw"])
    if w is None:
        assert close(es.z2m(None, 20, sums=sums), z["pt_z2m"]) and close(es.hm(None, sums=sums), z["pt_hm"])
    assert close(es.z2m(None, 5, sums=sums[3]), z["pt_z2m" if w is None else "pt_z2mw"][3, :5] *
                 (1.0 if w is None else sums[3, -1] / sums[3, -2]))
    with pytest.raises(ValueError, match="sums must hold"):
        es.z2m(None, 21, sums=sums)


def test_survival_functions():
    from pint_amd import eventstats as es
    st = load("photon_geo")[3]["stats"]
    for h, a, b, c in zip(st["h"], st["sf_hm"], st["sf_hm_log"], st["h2sig"]):
        assert close(es.sf_hm(h), a) and close(es.sf_hm(h, m=20, c=4, logprob=True), b) and close(es.h2sig(h), c)
    assert es.sf_hm(0.0) == 1.0
    for m, vals in st["sf_z2m"].items():
        assert close(es.sf_z2m(np.array(st["z"]), m=int(m)), vals)
    assert close(es.sig2sigma(np.array(st["sig"])), st["sig2sigma"])
    assert close([es.sig2sigma(s, two_tailed=False) for s in st["sig"] if s <= 0.5], st["sig2sigma_one"])
    assert close(es.sig2sigma(np.array(st["lsig"]), logprob=True), st["sig2sigma_log"])
    assert close(es.sig2sigma(np.array(st["lsig"][1:]), two_tailed=False, logprob=True), st["sig2sigma_log_one"])
    assert np.ndim(es.sig2sigma(0.05)) == 0
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="Probability must be between 0 and 1"):
            es.sig2sigma(bad)
    with pytest.raises(ValueError, match="Probability must be between 0 and 1"):
        es.sig2sigma(0.5, logprob=True)
    with pytest.raises(NotImplementedError, match="sf_hm: m = 0"):
        es.sf_hm(3.0, m=0)
    with pytest.raises(NotImplementedError, match="c = -1"):
        es.sf_hm(3.0, c=-1)
    with pytest.raises(NotImplementedError, match="one H value at a time"):
        es.sf_hm(np.array([1.0, 2.0]))


@pytest.mark.parametrize("name", NAMES)
def test_templates_and_host_likelihood(name, tmp_path):
    from pint_amd import event_optimize as eo
    _, _, z, meta = load(name)
    for i, (N, ph, fw) in enumerate(meta["gp_args"]):
        assert close(eo.gaussian_profile(N, ph, fw), z[f"gp_{i}"])
    L = meta["nbin"]
    raw = eo.read_gaussfitfile(io.StringIO(meta["gauss"]), L)
    assert close(raw, z["tmpl_raw"]) and close(raw / raw.mean(), z["tmpl"])
    path = tmp_path / "t.gauss"
    path.write_text(meta["gauss"])
    assert np.array_equal(eo.read_gaussfitfile(str(path), L), raw)
    with pytest.raises(ValueError, match="are not the same"):
        eo.read_gaussfitfile(io.StringIO(meta["gauss"] + "phas3 = 0.5 +/- 0\n"), L)
    w = z.get("weights")
    xt = np.arange(L) * 1.0 / L
    for k in (0, 7, 15):
        ph = z["pt_phase"][k]
        assert close(eo.profile_likelihood(z["pts_hi"][k, -1], xt, ph, z["tmpl"], w), z["pt_lnl"][k])
        off, best = eo.marginalize_over_phase(ph, z["tmpl"], weights=w, resolution=1.0 / 64, minimize=False)
        assert off == z["pt_scan_ret"][k, 0] and close(best, z["pt_scan_ret"][k, 1])
    off, best = eo.marginalize_over_phase(z["pt_phase"][0], z["tmpl"], weights=w)
    assert best >= z["pt_scan_ret"][0, 1] - 1e-9 and abs(float(off[0]) - z["pt_scan_ret"][0, 0]) <= 0.03 * L + 1e-9
    with pytest.raises(NotImplementedError, match="fftfit"):
        eo.marginalize_over_phase(z["pt_phase"][0], z["tmpl"], fftfit=True)
    with pytest.raises(NotImplementedError, match="showplot"):
        eo.marginalize_over_phase(z["pt_phase"][0], z["tmpl"], showplot=True)


@pytest.mark.parametrize("name", NAMES)
def test_get_event_toas(name):
    from pint_amd import get_event_TOAs
    model, toas, z, meta = load(name)
    ev = z["ev_hi"].astype(LD) + z["ev_lo"].astype(LD)
    geo = name == "photon_geo"
    w = z.get("weights")
    t = get_event_TOAs(ev, timesys="TT" if geo else "TDB", obs="geocenter" if geo else "barycenter", weights=w,
                       energies=None if w is None else 100.0 * (1 + w), model=model)
    assert t.ntoas == toas.ntoas and np.all(np.isinf(t.get_freqs())) and np.all(t.get_errors() == 1.0)
    dt = ((t.tdbld - toas.tdbld) * LD(86400)).astype(np.float64)
    print(f"{name}: max |dTDB| {np.max(np.abs(dt)):.3g} s")
    assert np.max(np.abs(dt)) <= (1e-9 if geo else 0.0)
    for k, bar in (("ssb_obs_pos_km", 1e-3), ("ssb_obs_vel_kms", 1e-6), ("obs_sun_pos_km", 1e-3)):
        assert np.max(np.abs(t.arrays[k] - toas.arrays[k])) <= bar, k
    # mjd_float (mask selection only): the same float64 but on the days that end in a leap second
    # (MJD 53735, 54831, 56108), where astropy's UTC MJD stretches the day to 86401 s and the pulsar_mjd
    # convention of prep (86400 s days) does not: there within that second
    dm = np.abs(t.arrays["mjd_float"] - toas.arrays["mjd_float"])
    leap = np.isin(np.floor(toas.arrays["mjd_float"]), (53735.0, 54831.0, 56108.0))
    assert np.max(dm[~leap]) <= 1e-9 and np.all(dm[leap] <= 1.0 / 86400)
    assert np.array_equal(t.arrays["is_bary"], toas.arrays["is_bary"])
    if w is not None:
        assert np.array_equal(t.arrays["weights"], w) and np.array_equal(t[10:20].arrays["energies"], 100.0 * (1 + w[10:20]))
    tz = t.tzr_for(model)
    if geo:  # the TZR row from the model, prepared like the events
        ref = toas.tzr
        d = (LD(tz["tdb_hi"][0]) + LD(tz["tdb_lo"][0]) - LD(ref["tdb_hi"][0]) - LD(ref["tdb_lo"][0])) * LD(86400)
        assert abs(float(d)) <= 1e-9 and float(tz["freq_mhz"][0]) == float(ref["freq_mhz"][0])
    else:
        assert tz is None
    for ts_, obs in (("TT", "barycenter"), ("TDB", "geocenter"), ("UTC", "geocenter"), ("TT", "gbt")):
        with pytest.raises(NotImplementedError, match="only TT at the geocenter and TDB at the barycenter"):
            get_event_TOAs(ev, timesys=ts_, obs=obs)
    with pytest.raises(ValueError, match="weights must have one value per event"):
        get_event_TOAs(ev, timesys="TT" if geo else "TDB", obs="geocenter" if geo else "barycenter", weights=np.ones(3))
    with pytest.raises(ValueError, match="No events found"):
        get_event_TOAs(np.zeros(0))


def test_photon_timing_host_refusals():
    """What PhotonTiming refuses before it touches the device."""
    from pint_amd import PhotonTiming
    model, toas, z, meta = load("photon_geo")
    with pytest.raises(ValueError, match="1..4096 bins"):
        PhotonTiming(model, toas, np.ones(4097))
    with pytest.raises(ValueError, match="one value per photon"):
        PhotonTiming(model, toas, z["tmpl"], weights=np.ones(7))
    with pytest.raises(NotImplementedError, match="Only uniform and normal"):
        PhotonTiming(model, toas, z["tmpl"], prior_info={"F0": {"distr": "lognormal"}})
    m2 = load("photon_geo")[0]
    m2.TZRMJD.frozen = False  # (a parameter of the model that is no entry of the device table)
    with pytest.raises(NotImplementedError, match="free parameter TZRMJD has no slot in the device table"):
        PhotonTiming(m2, toas, z["tmpl"])
    pt = PhotonTiming(model, toas, z["tmpl"], weights=z["weights"], prior_info=meta["prior_info"], phs=0.5)
    assert pt.param_labels[-1] == "PHASE" and set(pt.param_labels) == set(meta["labels"])
    assert pt.nparams == len(meta["labels"]) and pt.fitvals[-1] == 0.5 and pt.fiterrs[-1] == 0.03
    perm = [meta["labels"].index(p) for p in pt.param_labels]
    pts = (z["pts_hi"].astype(LD) + z["pts_lo"].astype(LD))[:, perm]
    assert close(pt.lnprior_batch(pts), z["pt_post"][:, 1]) and close(pt.lnprior(pts[3]), z["pt_post"][3, 1])
    out = pts[:3].copy()
    out[0, -1], out[1, -1] = LD(1.0001), LD(-1e-9)
    out[2, 0] += LD(1.0)  # F0 far outside its uniform prior
    assert np.all(np.isneginf(pt.lnprior_batch(out)))
    edge = pts[:2].copy()
    edge[0, -1], edge[1, -1] = LD(0.0), LD(1.0)  # the ends of [0, 1] are inside
    assert np.all(np.isfinite(pt.lnprior_batch(edge)))
    with pytest.raises(IndexError, match="number of input parameters"):
        pt.lnprior(pts[0, :-1])
    with pytest.raises(ValueError, match="offsets per point"):
        pt.phase_scan(pts[:1], resolution=1.0 / 4096)
    none = PhotonTiming(model, toas, None)
    with pytest.raises(ValueError, match="no template"):
        none.lnlikelihood_batch(pts[:1])
