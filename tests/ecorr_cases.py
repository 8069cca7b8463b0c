"""ECORR cases for test_ecorr_sweep.py, pure host: TOA sets built row by row at chosen times
(the sweep replaces the residuals by a seeded N(0, sigma_i) vector, so the arrival times need no
zeroing) and the case table.

A set is a list of clusters in time order: an ECORR epoch of m rows 0.01 s apart (m <= 70: within
the 1 s bucket of noise.ecorr_epochs), its row j at 700 + 20 j MHz, or a "slot" between the
epochs, by turns one row with the ECORR's flag -g A (a lone TOA, below nmin = 2: in no epoch),
one row with -g N (no ECORR selects it) and a pair of -g N rows 0.2 s apart (an epoch but for the
flag).  Uncertainties 0.4 .. 1.0 us, seeded (every lane of k_ecorr holds another weight).  Every
row carries -f fake (pta_par's EFAC / EQUAD).

  mix           two rounds of the epoch sizes SIZES (2, 3, 4, 5, 7, 63, 64, 65 and 70, not sorted:
                18 epochs, no multiple of 4) between 450 slots; rows in time order
  mix_shuffled  mix in a seeded random row order (ep_idx not contiguous, bins gathered by k_dmx)
  mix_small     mix's first five epochs (5, 64, 2, 70, 3) and every second slot: n <= 512
  two           mix with every second epoch on -g B (a second ECORR parameter) and the rows of the
                last 70-row epoch by turns A and B: two epochs of 35 at the same time
  many          262 epochs of 2 and 3 rows in ten DMX bins (70 in bin 1, none in bin 5; bin 3 is
                frozen in the cases) between 36 slots per bin

straddle and overlap are mix under another model: a DMX bin edge between the rows of the first
70-row epoch; a second ECORR on -f fake, which selects every row.
"""
import numpy as np

import shape_cases as SC
from ld_util import LD

SIZES = (5, 64, 2, 70, 3, 65, 7, 63, 4)
NSLOT = 450
DT_ROW = LD("0.01")     # s between the rows of an epoch
DT_PAIR = LD("0.2")     # s between the rows of a -g N pair
FREQS = (800.0, 1200.0, 1600.0, 2000.0)
ECORR_A, ECORR_B, ECORR_ALL = 0.5, 0.8, 0.4   # us
MANY_NDMX = 10
MANY_COUNTS = (25, 70, 23, 24, 26, 0, 25, 23, 24, 22)   # epochs per bin: 262
MANY_SLOTS = 36
MANY_FROZEN = (3,)
# widest padded Gram of every tiles-per-wave count T (pint_hip.hip gram_maxkp)
GRAM_MAXKP = {1: 80, 2: 112, 3: 144, 4: 160, 5: 192, 6: 208}
K_MAX = 196  # the last K k_solve takes


def _clusters_mix():
    """[(MJD, kind, size)]: the epochs at (e + 0.37) / 18 of the span, the slots at (k + 0.5) / 450."""
    ne = 2 * len(SIZES)
    cl = [(SC.MJD0 + LD(e + LD("0.37")) * LD(SC.TSPAN) / ne, "epoch", (2 * SIZES)[e]) for e in range(ne)]
    cl += [(SC.MJD0 + (LD(k) + LD("0.5")) * LD(SC.TSPAN) / NSLOT, "slot", k) for k in range(NSLOT)]
    return sorted(cl, key=lambda x: x[0])


def _clusters_many():
    edges = np.linspace(53000, 56652.01, MANY_NDMX + 1)
    cl, e = [], 0
    for b, cnt in enumerate(MANY_COUNTS):
        lo, w = LD(edges[b]), LD(edges[b + 1]) - LD(edges[b])
        for k in range(cnt):
            cl.append((lo + (LD(k) + LD("0.5")) / cnt * w, "epoch", 2 + (e % 2)))
            e += 1
        for k in range(MANY_SLOTS):
            cl.append((lo + (LD(k) + LD("0.31")) / MANY_SLOTS * w, "slot", b * MANY_SLOTS + k))
    return sorted(cl, key=lambda x: x[0])


def _rows(clusters):
    """Rows of the clusters: (MJD longdouble, MHz, -g flag, designed epoch or -1, slot or -1)."""
    t, f, g, ep, sl = [], [], [], [], []
    ne = 0
    day = LD(86400)
    for t0, kind, x in clusters:
        if kind == "epoch":
            for j in range(x):
                t.append(t0 + j * DT_ROW / day)
                f.append(700.0 + 20.0 * j)
                g.append("A")
                ep.append(ne)
                sl.append(-1)
            ne += 1
            continue
        rows = (("A",), ("N",), ("N", "N"))[x % 3]
        for j, flag in enumerate(rows):
            t.append(t0 + j * DT_PAIR / day)
            f.append(FREQS[(x + 2 * j) % 4])
            g.append(flag)
            ep.append(-1)
            sl.append(x)
    return (np.array(t, dtype=LD), np.array(f), np.array(g, dtype=object), np.array(ep), np.array(sl))


class TOASet:
    """The rows of a set (before TOAs are made of them) and the epochs it was designed with."""

    def __init__(self, name, t, f, g, ep, sl):
        self.name, self.t, self.f, self.g, self.ep, self.sl = name, t, f, g, ep, sl
        self.n = len(t)
        self.err = 0.4 + 0.6 * np.random.default_rng(len(t)).uniform(size=len(t))

    def take(self, name, idx):
        s = TOASet(name, self.t[idx], self.f[idx], self.g[idx], self.ep[idx], self.sl[idx])
        s.err = self.err[idx]
        return s

    def designed(self, flag):
        """The designed epochs of the rows with -g flag: row lists, in time order."""
        ids = sorted(set(self.ep[(self.ep >= 0) & (self.g == flag)]), key=lambda e: (self.t[self.ep == e].min(), e))
        return [np.flatnonzero((self.ep == e) & (self.g == flag)) for e in ids]

    def sizes(self, flag="A"):
        return [len(x) for x in self.designed(flag)]

    def toas(self):
        from pint_amd.simulation import _row_arrays, _tzr
        from pint_amd.toa import TOAs
        base = SC.model_of(SC.Case("base", 8, SC.BASE_NDMX, 30))
        fl = {"name": ["fake"] * self.n, "f": ["fake"] * self.n, "g": [str(x) for x in self.g]}
        return TOAs(_row_arrays(self.t, self.f, self.err, "geocenter"), fl, _tzr(base, "geocenter"), "fake")


_SETS = {}


def toa_set(name):
    """The named set's rows (cached)."""
    if name in _SETS:
        return _SETS[name]
    if name == "mix":
        s = TOASet(name, *_rows(_clusters_mix()))
    elif name == "many":
        s = TOASet(name, *_rows(_clusters_many()))
    elif name == "mix_shuffled":
        m = toa_set("mix")
        s = m.take(name, np.random.default_rng(m.n).permutation(m.n))
    elif name == "mix_small":
        m = toa_set("mix")
        s = m.take(name, np.flatnonzero(((m.ep >= 0) & (m.ep < 5)) | ((m.sl >= 0) & (m.sl % 2 == 0))))
    elif name == "two":
        m = toa_set("mix")
        s = m.take(name, np.arange(m.n))
        g = s.g.copy()
        g[(s.ep >= 0) & (s.ep % 2 == 1)] = "B"
        last70 = max(e for e in set(s.ep) if e >= 0 and np.sum(s.ep == e) == 70)
        rows = np.flatnonzero(s.ep == last70)
        g[rows] = np.where(np.arange(len(rows)) % 2 == 0, "A", "B")
        s.g = g
    else:
        raise KeyError(name)
    _SETS[name] = s
    return s


def straddle_edge():
    """(bin a, MJD): an edge of the 20-bin model moved between rows 34 and 35 of mix's first
    70-row epoch, from the nearer side (the bins on both sides keep their other TOAs)."""
    m = toa_set("mix")
    e = min(e for e in set(m.ep) if e >= 0 and np.sum(m.ep == e) == 70)
    rows = np.flatnonzero(m.ep == e)
    x = float((m.t[rows[34]] + m.t[rows[35]]) / 2)
    edges = np.round(np.linspace(53000, 56652.01, 21), 5)
    a = int(np.argmin(np.abs(edges[1:-1] - x)))  # the inner edge nearest the epoch: between bins a and a + 1
    return a, x


# ---- the cases -------------------------------------------------------------------------------
EC_A = (("-g", "A", ECORR_A),)
EC_AB = (("-g", "A", ECORR_A), ("-g", "B", ECORR_B))
EC_OVER = (("-g", "A", ECORR_A), ("-f", "fake", ECORR_ALL))


def _case(name, ntim, ndmx, nred, toas="mix", ecorr_par=EC_A, **kw):
    return SC.Case(name, ntim, ndmx, nred, toas=toas, ecorr=True, ecorr_par=ecorr_par, **kw)


def _full(name, K, nred, **kw):
    """A full-layout case of K columns on 20 free bins."""
    return _case(name, K - 2 * nred - SC.BASE_NDMX, SC.BASE_NDMX, nred, **kw)


def cases():
    out = []
    # full layout, GLS: k_gram<T, CH, true> at the widest Kp of T = 1, 4, 5, 6 (K <= 196)
    for T, nred in ((1, 20), (4, 40), (5, 60), (6, 60)):
        out.append(_full(f"ec_T{T}", min(GRAM_MAXKP[T] - 1, K_MAX), nred))
    out.append(_full("ec_T4_ns3", GRAM_MAXKP[4] - 1, 40, nsplit=3))
    # the small path: k_gram_s and the ECORR rows by k_gram<1, 128, true>
    out.append(_case("ec_small", 8, SC.BASE_NDMX, 8, toas="mix_small", dmx_free=False))
    # compact layout: k_ecorr's eC, k_ecorr_dmx, the fused Sigma, the deferred covariance
    fit = dict(layout="fit")
    out.append(_case("ec_fit_mix", 8, 20, 0, **fit))
    out.append(_case("ec_fit_mix_red_d2", 8, 20, 16, cov_defer=2, **fit))
    out.append(_case("ec_fit_shuf", 8, 20, 8, toas="mix_shuffled", **fit))
    out.append(_case("ec_fit_shuf_d2", 8, 20, 0, toas="mix_shuffled", cov_defer=2, **fit))
    out.append(_case("ec_fit_many", 8, MANY_NDMX, 0, toas="many", dmx_frozen=MANY_FROZEN, **fit))
    out.append(_case("ec_fit_many_red_d2", 8, MANY_NDMX, 12, toas="many", dmx_frozen=MANY_FROZEN, cov_defer=2,
                     postfit=True, **fit))
    out.append(_case("ec_fit_two", 8, 20, 8, toas="two", ecorr_par=EC_AB, **fit))
    out.append(_case("ec_fit_two_d2", 8, 20, 0, toas="two", ecorr_par=EC_AB, cov_defer=2, **fit))
    out.append(_case("ec_fit_Kd68", 8, 20, 30, **fit))  # Kd = 8 + 60 >= 64: k_ecorr_dmx's second column chunk
    # a frozen bin beside the straddled edge: the 70-row epoch has rows in a free bin and rows in
    # none (drow < 0), the epochs inside the frozen bin have no bin (ep_bin = -1)
    a, x = straddle_edge()
    out.append(_case("ec_fit_frozen", 8, 20, 8, dmx_frozen=(a + 1,), dmx_edge=(a, x), **fit))
    # PHOFF frozen: the virtual ones row of k_onesrow, its PLDMNoise branch
    out.append(_case("ec_ones_full", 8, 20, 10, phoff=True, postfit=True))
    out.append(_case("ec_ones_fit", 8, 20, 10, phoff=True, **fit))
    out.append(_case("ec_ones_fit_dmn", 8, 20, 14, phoff=True, ndmn=4, **fit))
    out.append(_case("ec_ones_full_dmn", 8, 20, 14, phoff=True, ndmn=4))
    # the fall-backs of pint_set_ecorr: an epoch in two free bins; a TOA in two epochs (refused)
    out.append(_case("ec_straddle", 8, 20, 8, dmx_edge=(a, x), ecorr_off=True, **fit))
    out.append(_case("ec_overlap", 8, 20, 8, ecorr_par=EC_OVER, ecorr_off=True, refused=True, **fit))
    # WLS: no ECORR work
    out.append(_case("ec_wls", 8, 20, 8, mode=0))
    return out


# the noise likelihood's sets and kinds (k_noise_lnl through NoiseLikelihood): kind 0 without
# ECORR, 1 with ECORR and PHOFF free, 2 with ECORR and no PhaseOffset
LNL_SETS = {"mix": EC_A, "many": EC_A, "two": EC_AB}


def lnl_par(kind, ecorr_par):
    """A par without time-correlated noise for the likelihood kinds: pta_par's EFAC / EQUAD on
    -f fake, a second EFAC on -g N, the set's ECORRs (kinds 1, 2), PHOFF free (kind 1)."""
    from pint_amd.simulation import pta_par
    par = "\n".join(l for l in pta_par(SC.SEED, "", ndmx=SC.BASE_NDMX).split("\n") if not l.startswith("TNRed")) + "\n"
    par += "EFAC -g N 1.3\n"
    if kind:
        par += "".join(f"ECORR {k} {v} {x!r}\n" for k, v, x in ecorr_par)
    if kind == 1:
        par += "PHOFF 0.05 1\n"
    return par
