"""Wideband cases for test_wideband_sweep.py, pure host: the case table, the flag columns and
wideband DM data written onto the sweep's fake TOAs, and the longdouble references of the
modelled DM and of the DM rows' design matrix, formed from the par values alone (no engine
code): DM_model = sum_k DMk x^k / k! (x in Julian years from DMEPOCH) + the DMX value of the
TOA's bin (free or frozen) - the DMJUMPs selecting it; M_dm: Offset 0, DMk x^k / k!, DMX bin
1, DMJUMP -1, every other column 0.
"""
import math

import numpy as np

import shape_cases as SC
from ld_util import LD

# pc/cm^3: the smallest DM error; the largest is 5 DME0.  pp_dm - DM_model is formed in float64 at
# |DM| ~ 3.1 (one ulp 4.4e-16), so a residual carries ~1e-15 of rounding, 2e-12 of its error at DME0;
# n such terms of random sign move chi2 and the normalised Gram's residual entries by ~2 * 2e-12 /
# sqrt(n) <= 2.5e-13 (n >= 300), under the 1e-12 bars with room for the sums' own rounding
DME0 = 5e-4
DJY = 365.25   # days per Julian year


def wb_flags(n):
    """The flag columns the cases' mask parameters select on, by the TOA's index in time order."""
    i = np.arange(n)
    return {"fe": ["ABCD"[k % 4] for k in i], "be": ["XYZ"[k % 3] for k in i],
            "gp": ["G" if k % 5 < 2 else "H" for k in i]}


def order_index(c, n):
    if c.order == "reverse":
        return np.arange(n)[::-1]
    if c.order == "shuffle":
        return np.random.default_rng(n).permutation(n)
    if c.order:
        raise ValueError(c.order)
    return np.arange(n)


def dm_errors(n):
    """Unscaled DM errors, DME0 .. 5 DME0 (seeded; by the TOA's index in time order)."""
    return DME0 * (1 + 4 * np.random.default_rng(4000 + n).uniform(size=n))


def dm_noise(n):
    return np.random.default_rng(5000 + n).standard_normal(n)


def years(model, toas):
    return (np.asarray(toas.tdbld, dtype=LD) - LD(model["DMEPOCH"].value)) / LD(DJY)


def selected(toas, key, value):
    return np.array([f == value for f in toas.flag_columns[key.lstrip("-")]], dtype=bool)


def dm_model(c, model, toas):
    """The modelled DM of every TOA in longdouble from the model's values (pc/cm^3)."""
    x = years(model, toas)
    dm = np.zeros(toas.ntoas, dtype=LD)
    for k, name in enumerate(("DM", "DM1", "DM2")):
        dm += LD(model[name].value) * x ** k / math.factorial(k)
    b = SC.bin_rows(c, toas.arrays["mjd_float"])
    val = np.array([LD(model[f"DMX_{a + 1:04d}"].value) for a in range(c.ndmx)] + [LD(0)], dtype=LD)
    dm += val[b]
    for (key, v), name in zip(SC.DMJ_KEYS, model.mask_params("DMJUMP")):
        assert (model[name].key, list(model[name].key_value)) == (key, [v])
        dm -= np.where(selected(toas, key, v), LD(model[name].value), LD(0))
    return dm


def dm_design(c, model, columns, toas, extra=None):
    """The DM rows of the named columns in longdouble; extra: {name: column} for columns the
    host does not form (NE_SW)."""
    x = years(model, toas)
    b = SC.bin_rows(c, toas.arrays["mjd_float"])
    jumps = dict(zip(model.mask_params("DMJUMP"), SC.DMJ_KEYS))
    M = np.zeros((toas.ntoas, len(columns)), dtype=LD)
    for j, name in enumerate(columns):
        if name in ("DM", "DM1", "DM2"):
            k = ("DM", "DM1", "DM2").index(name)
            M[:, j] = x ** k / math.factorial(k)
        elif name.startswith("DMX_"):
            M[:, j] = (b == int(name[4:]) - 1)
        elif name in jumps:
            M[:, j] = -selected(toas, *jumps[name]).astype(LD)
        elif extra and name in extra:
            M[:, j] = extra[name]
    return M


def scaled_dm_errors(c, toas):
    """DMEQUAD in quadrature, then DMEFAC, on -fe B (noise_model.py:291-315)."""
    s = np.asarray(toas.get_dm_errors(), dtype=LD)
    if c.dmefac:
        sel = selected(toas, "-fe", "B")
        s = np.where(sel, LD("1.3") * np.sqrt(s * s + LD("0.0002") ** 2), s)
    return s


def case_toas(c, base, extra_dm=None):
    """The case's TOAs: the set in the case's order, with the flag columns and wideband DMs
    pp_dm = DM_model + z dm_sigma (the scaled error); extra_dm: a share of DM_model the host does
    not form (the solar wind's), per TOA of the ordered set."""
    from pint_amd.simulation import attach_wideband
    n = base.ntoas
    idx = order_index(c, n)
    fl = wb_flags(n)
    t = attach_wideband(base[idx], np.zeros(n), dm_errors(n)[idx], {k: [v[i] for i in idx] for k, v in fl.items()})
    model = SC.model_of(c)
    dm = dm_model(c, model, t) + LD(1) * dm_noise(n)[idx] * scaled_dm_errors(c, t)
    if extra_dm is not None:
        dm = dm + extra_dm
    return attach_wideband(t, np.asarray(dm, dtype=np.float64), dm_errors(n)[idx]), model


# ---- the cases -------------------------------------------------------------------------------
ALL_DM = ("DM", "DM1", "DM2")


def case(name, ntim, ndmx, nred, toas, **kw):
    kw.setdefault("dmefac", True)
    return SC.Case(name, ntim, ndmx, nred, toas=toas, layout="fit", wb=True, **kw)


def third(ndmx):
    return tuple(range(0, ndmx, 3))


def cases():
    out = [
        # m = 0: only DMX free; 8 bins of 137 TOAs (three passes of 64 lanes), k_gram_v without the binned body
        case("wb_m0_b8", 6, 8, 0, "n1100"),
        # m = 1: DM1 alone; ndc = 9 (ndc % 4 = 1)
        case("wb_m1_b9", 6, 9, 8, "n530", dm_free=("DM1",)),
        # m = 3, every third bin frozen at its non-zero value: 10 free of 15 (ndc % 4 = 2)
        case("wb_m3_b10", 6, 15, 8, "n530", dm_free=ALL_DM, dmx_frozen=third(15)),
        # m = 8 = WB_MAXC: DM, DM1, DM2 and 5 DMJUMPs; 11 free of 14 (ndc % 4 = 3)
        case("wb_m8_b11", 6, 14, 16, "n1100", dm_free=ALL_DM, ndmjump=5, dmx_frozen=(1, 7, 13)),
        # DM frozen, DM1 and DM2 free (Taylor order != free-column index); 21 free bins, one of one TOA
        case("wb_dm12_b21", 6, 22, 8, "n530", dm_free=("DM1", "DM2"), dmx_frozen=(5,), one_toa=True),
        # a frozen DMJUMP between two free ones (mask bit != free-column index); k_gram_s + k_dmx_rows
        case("wb_dmjgap_grams", 6, 8, 0, "n300", ndmjump=3, dmj_frozen=(1,), vgram=False),
        # DM1 = DM2 = 0 and free: the modelled DM at x = 0, the derivative columns at dt
        case("wb_dm12zero", 6, 12, 8, "n530", dm_free=("DM1", "DM2"), dm12_zero=True, dmx_frozen=(0, 11)),
        # rows of a bin not contiguous: k_dmx; reversed: contiguous again
        case("wb_shuffle", 6, 12, 8, "n530", dm_free=ALL_DM, ndmjump=2, dmx_frozen=third(12), order="shuffle"),
        case("wb_reverse", 6, 12, 8, "n530", dm_free=ALL_DM, ndmjump=2, dmx_frozen=third(12), order="reverse"),
        case("wb_shuffle_ns3", 6, 12, 8, "n530", dm_free=ALL_DM, ndmjump=2, dmx_frozen=third(12), order="shuffle", nsplit=3),
        # m = 8 through k_gram<T> + k_dmx_rows
        case("wb_m8_novg", 6, 14, 16, "n1100", dm_free=ALL_DM, ndmjump=5, dmx_frozen=(1, 7, 13), vgram=False),
    ]
    # k_gram_v's binned body on and off, k_gram<T> + k_dmx_rows, N-splits through k_greduce
    vb = case("wb_vb", 6, 24, 16, "n1100", dm_free=ALL_DM, ndmjump=3, dmj_frozen=(1,), dmx_frozen=(2, 9, 16, 23))
    out += [vb, vb.but(name="wb_novb", vbin=False), vb.but(name="wb_novg", vgram=False),
            vb.but(name="wb_vb_ns3", nsplit=3), vb.but(name="wb_vb_ns5", nsplit=5),
            vb.but(name="wb_novg_ns3", vgram=False, nsplit=3)]
    # k_solve_dmx<8>: covariance in the solve, deferred with and without k_schur; <16>; the
    # general-solve fall-back of the compact layout (77 blocks)
    d8 = case("wb_dmx8", 6, 16, 56, "n1100", dm_free=("DM1",), ndmjump=2)
    out += [d8.but(name="wb_dmx8_d0", cov_defer=0), d8.but(name="wb_dmx8_d2", cov_defer=2),
            d8.but(name="wb_dmx8_d2_noschur", cov_defer=2, schur=False)]
    out.append(case("wb_dmx16", 8, 16, 60, "n1100", dm_free=("DM1",), ndmjump=3, dmj_frozen=(0,)))
    out.append(case("wb_blk77", 8, 16, 80, "n1100", ndmjump=2))
    # ECORR in the compact layout: every epoch of four TOAs within one bin
    ec = case("wb_ecorr", 6, 20, 8, "e1100", dm_free=("DM1",), ndmjump=2, ecorr=True)
    out += [ec, ec.but(name="wb_ecorr_ns3", nsplit=3)]
    return out


E2E = ("wb_m3_b10", "wb_m8_b11", "wb_dm12_b21")  # end to end against the oracle's wideband GLS step
