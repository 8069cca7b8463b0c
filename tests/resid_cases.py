"""Cases of the residual-pass sweep (test_resid_sweep.py), pure host.

An RCase names the row counts of its pulsars (prefixes of one fake TOA set of N_ALL rows), the
instances per pulsar, the session options and the flow; predict_mask repeats the dispatch
arithmetic of plan_batch / plan_eval / plan_resid2 (pint_hip.hip) and returns the bit
mask Session.resid_path() must report, which every case also states by hand (`mask`).

Shared with the GPU test so that the host checks (test_resid_cases.py) see the same inputs:
the two sigma classes, the delta_pulse_number rows, and the F0 / F1 offsets of every instance's
table, which make the phase residual wander by a few turns over the case's own rows.
"""
from dataclasses import dataclass

import numpy as np

import shape_cases as SC

# the dispatcher's constants (pint_hip.hip)
EF_ROWS = 254      # rows per evaluation block with the fused first half
RES_RB = 1024      # rows per residual block
RES_SMALLN = 256   # a wave per residual block up to this many rows
# Session.RESID_* (PINT_RESID_*)
EFUSED, R1_64, R1_256, R12, R2_64, R2_256, TILES, DEFERRED = 1, 2, 4, 8, 16, 32, 64, 128
BIT_NAMES = {EFUSED: "efused", R1_64: "r1<64>", R1_256: "r1<256>", R12: "r12", R2_64: "r2<64>", R2_256: "r2<256>",
             TILES: "tiles", DEFERRED: "deferred"}

N_ALL = 16257
PEPOCH = 54800.0
FREQS = [800, 1200, 1600, 2000]
SEED = 20


@dataclass(frozen=True)
class Opt:
    track: str          # "use_pulse_numbers" or "nearest"
    sub: bool           # subtract_mean
    wm: bool            # use_weighted_mean
    phoff: bool = False  # the model with a free PHOFF (no mean is subtracted then)

    @property
    def name(self):
        return (("pn" if self.track == "use_pulse_numbers" else "near") + ("+mean" if self.sub else "") +
                ("" if not self.sub else ("/w" if self.wm else "/1")) + ("+phoff" if self.phoff else ""))

    @property
    def mean(self):
        return self.sub and not self.phoff


# the option triples that make sense (the mean's weights only matter when it is subtracted), and
# the PhaseOffset model with both track modes
OPTIONS = [Opt(t, s, w) for t in ("use_pulse_numbers", "nearest") for s, w in ((True, True), (True, False), (False, True))]
OPTIONS += [Opt(t, True, True, True) for t in ("use_pulse_numbers", "nearest")]


@dataclass(frozen=True)
class RCase:
    name: str
    ns: tuple            # rows of every pulsar of the batch (a prefix of the TOA set each)
    mask: int            # resid_path() after the (last) evaluation, by hand from the dispatch rules
    ninst: int = 2       # instances per pulsar, each with its own F0 / F1 offsets
    flow: str = "eval"   # "eval": eval(True), the reads.  "tiles": eval(True), fit_step(1), eval(False), the
    #                      reads, chi2_gls.  "fit": eval(FIT), fit_step(1), debug_gram, the reads (flush_r2)
    small: bool = True   # set_small
    efuse: bool = True   # set_efuse
    resid12: bool = True  # PINT_RESID12
    nred: int = 30
    ntim: int = 8
    mask_read: int = 0   # bits a reader of the residuals adds (the flushed second half)

    @property
    def maxn(self):
        return max(self.ns)


def predict_mask(c: RCase, vgram=True):
    """(resid_path() after the case's last pint_eval, bits added by the first reader), as
    pint_eval decides them; vgram: every instance takes k_gram_v (asserted on the device)."""
    smallpath = c.small and c.maxn <= RES_SMALLN
    efz = c.efuse and not smallpath           # (no pass after the evaluation in these models)
    want_M = {"eval": 1, "tiles": 0, "fit": 2}[c.flow]
    wt = 0 < c.nred <= 63 and want_M == 0     # pint_ctx::wfuse and no design matrix
    defer2 = want_M == 2 and vgram and c.maxn <= 64 * (EF_ROWS if efz else RES_RB)
    fused12 = not efz and smallpath and not wt and not defer2 and c.resid12
    r2 = R2_64 if (not efz and smallpath) else R2_256
    m = EFUSED if efz else (R12 if fused12 else (R1_64 if smallpath else R1_256))
    if defer2:
        return m | DEFERRED, r2
    if not fused12:
        m |= r2 | (TILES if wt else 0)
    return m, 0


def mask_names(m):
    return "+".join(n for b, n in BIT_NAMES.items() if m & b)


# ---- the inputs --------------------------------------------------------------------------------
def err_us():
    """Two sigma classes a factor 10 apart, seeded."""
    return np.where(np.random.default_rng(SEED).random(N_ALL) < 0.5, 0.5, 5.0)


def delta_pulse_numbers():
    """+-1, +-2 turns on a seeded tenth of the rows."""
    rng = np.random.default_rng(SEED + 1)
    d = np.zeros(N_ALL)
    idx = rng.choice(N_ALL, N_ALL // 10, replace=False)
    d[idx] = rng.choice([-2.0, -1.0, 1.0, 2.0], len(idx))
    return d


def toa_spec(model):
    """make_fake_toas_batch's spec of the one TOA set."""
    return dict(model=model, start=SC.MJD0, end=SC.MJD1, ntoas=N_ALL, freq=FREQS, obs="geocenter", error_us=err_us(),
                add_noise=True, seed=SEED + 2, flags={"f": "fake"})


def approx_dt(n):
    """Seconds since PEPOCH of the first n rows, to the delays (~500 s)."""
    return (SC.MJD0 + np.arange(n) * (SC.TSPAN / (N_ALL - 1)) - PEPOCH) * 86400.0


def f_offsets(n, k, scale=1.0):
    """(dF0, dF1) of instance k of an n-row pulsar: the phase dF0 dt + dF1 dt^2 / 2 wanders by a
    seeded 2..4 turns (times scale) to either side over the n rows.  Rows far from PEPOCH (a short
    prefix): zero at the rows' centre tc with slope a / h there (h the half span), so the phase
    stays O(a) turns although dt is 1.6e8 s; else a / h and a seeded curvature."""
    rng = np.random.default_rng([SEED, n, k])
    a = rng.uniform(2, 4) * rng.choice([-1.0, 1.0]) * scale
    c = rng.uniform(0.5, 1) * rng.choice([-1.0, 1.0]) * scale
    dt = approx_dt(n)
    tc, h = 0.5 * (dt[0] + dt[-1]), max(0.5 * (dt[-1] - dt[0]), 43200.0)
    if abs(tc) > h:
        s = a / h
        return -s, 2 * s / tc
    return a / h, 2 * c / (h * h)


def tile_scale(o: Opt):
    """F0 / F1 offset scale of the cases that check the GLS chi2, so that r^T N^-1 r / chi2 <= 10
    holds: the Fourier basis absorbs a smooth wander of the residuals nearly whole.  With pulse
    numbers a small wander (+-0.15 turns) under the +-1, +-2 turns of the delta_pulse_number
    rows, which it cannot absorb; in `nearest` mode, which wraps those away, a wander of +-40 to
    80 turns, whose saw-tooth of > 80 teeth lies above the 63 harmonics."""
    return 0.05 if o.track == "use_pulse_numbers" else 20.0


def approx_full(n, k, o: Opt, scale=1.0):
    """The phase residual before the mean to ~1e-2 turns, and the pre-rounding phase of the
    `nearest` branch (relative to the TZR row up to an integer), from the offsets alone: the TOAs
    have zero residuals (to their noise) and the pulse numbers of the true model."""
    d0, d1 = f_offsets(n, k, scale)
    dt = approx_dt(n)
    rel = d0 * dt + 0.5 * d1 * dt * dt + delta_pulse_numbers()[:n]
    if o.track == "use_pulse_numbers":
        return rel, None
    x = rel - rel[0] if o.mean else rel
    return x - np.floor(x + 0.5), x


# ---- the models --------------------------------------------------------------------------------
_MODELS = {}


def last_mjd(n):
    return SC.MJD0 + (n - 1) * (SC.TSPAN / (N_ALL - 1))


def model_of(c: RCase, phoff: bool, n=None):
    """Spin + astrometry + DM + DMX + PLRedNoise (shape_cases.par_of), c.ntim timing columns;
    phoff: a free PHOFF in place of the Offset.  The fit flow frees the 20 DMX bins (k_gram_v
    needs >= 8) and, for a prefix of n rows, lays their ranges over the prefix's own span."""
    fit = c.flow == "fit"
    key = (c.ntim, c.nred, fit, phoff, n if (fit and n < N_ALL - 1) else None)
    if key in _MODELS:
        return _MODELS[key]
    from pint_amd.timing_model import get_model
    sc = SC.Case("resid", c.ntim, SC.BASE_NDMX, c.nred, dmx_free=fit)
    par = SC.par_of(sc)
    if key[4] is not None:
        edges = np.round(np.linspace(SC.MJD0, last_mjd(n) + 0.01, sc.ndmx + 1), 5)
        out = []
        for l in par.split("\n"):
            w = l.split()
            if w and w[0].startswith(("DMXR1_", "DMXR2_")):
                l = f"{w[0]} {edges[int(w[0][6:]) - 1 + int(w[0][4]) - 1]:.5f}"
            out.append(l)
        par = "\n".join(out)
    if phoff:
        par += "PHOFF 0.123 1\n"
    m = get_model(par)
    nb, nwx = SC.timing_split(c.ntim)
    assert nwx == 0
    free = list(SC.TIMING[:nb]) + (["PHOFF"] if phoff else [])
    if fit:
        free += list(m.dmx_params())
    m.free_params = free
    _MODELS[key] = m
    return m


def table_of(lay, n, k, scale=1.0):
    """The layout's parameter table with instance k's F0 / F1 offsets."""
    from pint_amd.engine import pack_table, split_ld
    tab = pack_table(lay).copy()
    for name, d in zip(("F0", "F1"), f_offsets(n, k, scale)):
        o = lay.offsets[name]
        tab[o], tab[o + 1] = split_ld(np.longdouble(tab[o]) + np.longdouble(tab[o + 1]) + np.longdouble(d))
    return tab


# ---- the cases ---------------------------------------------------------------------------------
def cases():
    out = []
    # small path: a wave per instance; ninst 1, 3, 4, 5 leave 3, 1, 0, 3 idle waves in the last
    # workgroup (rb >= nrblk).  k_resid12, and k_resid1<64> + k_resid2<64> with PINT_RESID12=0
    for n in (1, 2, 63, 64, 65, 128, 129, 255, 256):
        for ni in (1, 3, 4, 5):
            # (one row has no time span for the red-noise frequencies: no PLRedNoise there)
            nred = 30 if n > 1 else 0
            out.append(RCase(f"small_n{n}_x{ni}_r12", (n,), R12, ninst=ni, nred=nred))
            out.append(RCase(f"small_n{n}_x{ni}_r1r2", (n,), R1_64 | R2_64, ninst=ni, resid12=False, nred=nred))
    # ... with the one-wave tile store (NW == 1): the post-fit pass of a red-noise batch; 64-row
    # chunks of the wave's 256 rows: one full, two and a row, four less a row, four full
    for n, ni in ((64, 3), (129, 5), (255, 1), (256, 4)):
        out.append(RCase(f"small_tiles_n{n}_x{ni}", (n,), R1_64 | R2_64 | TILES, ninst=ni, flow="tiles", nred=7, ntim=1))
    # the 256-thread kernels: one block and a row, a block less a row, a block, two blocks and a row
    for n in (257, 1023, 1024, 1025, 2049):
        out.append(RCase(f"r256_n{n}", (n,), R1_256 | R2_256, efuse=False))
    # the first half in the evaluation's blocks of 254 rows (+ row 0 and the TZR row on lanes 254, 255)
    for n in (257, 253, 254, 255, 508, 509):
        out.append(RCase(f"efused_n{n}", (n,), EFUSED | R2_256, small=n > 256))
    # instances of different block counts in one batch: rblk_inst, rb0, eb0, the roff - ii offsets
    out.append(RCase("efused_mixed", (254, 1025, 64, 509), EFUSED | R2_256, ninst=1))
    out.append(RCase("r256_mixed", (254, 1025, 64, 509), R1_256 | R2_256, ninst=1, efuse=False))
    # the Woodbury trig tiles: nred at the edges of the a + 8b split, the fused and the unfused
    # first half (n = 65 unfused: the small path's one-wave tiles; fused: set_small(False))
    for n in (65, 257, 1025):
        for nred in (1, 7, 8, 9, 31, 63):
            out.append(RCase(f"tiles_n{n}_nred{nred}_efused", (n,), EFUSED | R2_256 | TILES, ninst=1, flow="tiles",
                             nred=nred, ntim=1, small=n > 256))
            unf = (R1_64 | R2_64) if n <= RES_SMALLN else (R1_256 | R2_256)
            out.append(RCase(f"tiles_n{n}_nred{nred}_unfused", (n,), unf | TILES, ninst=1, flow="tiles", nred=nred,
                             ntim=1, efuse=False))
    # 64 modes: no tiles, the dots from k_wdot
    out.append(RCase("tiles_n1025_nred64_kwdot", (1025,), EFUSED | R2_256, ninst=1, flow="tiles", nred=64, ntim=1))
    # the second half left to k_gram_v and flushed by the read; 64 evaluation blocks of 254 rows is
    # the most the Gram sums on one wave: 16 256 rows defer, 16 257 do not
    out.append(RCase("defer_n1025", (1025,), EFUSED | DEFERRED, flow="fit", nred=8, ntim=3, mask_read=R2_256))
    out.append(RCase("defer_n1025_unfused", (1025,), R1_256 | DEFERRED, flow="fit", nred=8, ntim=3, efuse=False,
                     mask_read=R2_256))
    out.append(RCase("defer_n16256", (16256,), EFUSED | DEFERRED, ninst=1, flow="fit", nred=8, ntim=3, mask_read=R2_256))
    out.append(RCase("defer_n16257_not", (16257,), EFUSED | R2_256, ninst=1, flow="fit", nred=8, ntim=3))
    return out
