"""Synthetic cases of chosen width for the shape sweep (test_shape_sweep.py), pure host.

A Case names an exact number of timing columns (Offset included), of free DMX bins and of
red-noise modes; model_of builds the model from simulation.pta_par by restricting free_params
and adding fitted WaveX amplitudes at half-integer multiples of 1 / Tspan above the red-noise
band (not degenerate with the red-noise basis at the integer multiples); predict_plan repeats
the dispatch arithmetic of pint_set_instances / pint_fit_step (pint_hip.hip) for a batch of
that one pulsar and returns the plan Session.last_plan() must report: of the batch's planner
plan_batch, the PINT_NSPLIT cap of choose_nsplit, vg_ok, slots_ok / first_ntr, vb_rows_ok and
plan_vgram (vgram_layout here) and gram_order's launch keys (gram_T, the k_gram_v key); of
the step's, fit_shape and plan_fit_step.

The wideband sweep (wb_cases.py, test_wideband_sweep.py) uses the same Case with its wideband
fields set: free DM Taylor terms, DMJUMPs and NE_SW beside the ntim timing columns (ndense),
frozen DMX bins and DMJUMPs, a bin of one TOA, the TOA order; bin_rows / free_rows map TOAs to
the model's bins and to the compact DMX columns, and predict_plan adds k_dmx, k_ecorr_dmx and
k_wb_gram to the plan.  Cases without those fields predict what they did before.

The ECORR sweep (ecorr_cases.py, test_ecorr_sweep.py) adds its own: the ECORR lines of the par
(ecorr_par), a pulsar the ECORR rule of pint_set_ecorr takes off the compact layout (ecorr_off),
a PhaseOffset with PHOFF frozen (phoff: no Offset column), PLDMNoise modes among the nred
Fourier modes (ndmn) and one DMX bin edge moved to a chosen MJD (dmx_edge); predict_plan takes
ECORR onto the small path (k_gram_s and the ECORR rows by k_gram<1, 128, true>).
"""
from dataclasses import dataclass, replace

import numpy as np

# the dispatcher's constants (pint_hip.hip)
GS_MAXN = 512      # k_gram_s: at most this many rows
BS_MAXNB = 12      # k_solve_blk / k_sigma: at most this many 16-column blocks
SD_MAXBLK = 76     # k_solve_dmx: S + U blocks
VTRIG = 64         # k_gram_v: nred <= VTRIG / 2 - 1
VMAXR0 = 48        # k_gram_v: timing columns + residual
VMAXKP = 112       # k_gram_v: widest LDS tile
VCH = 64           # k_gram_v rows per chunk
GWAVES = 16        # k_gram waves per workgroup
LDS = 160 * 1024
MJD0, MJD1 = 53000.0, 56652.0
TSPAN = MJD1 - MJD0
SEED = 7
BASE_NDMX = 20
# free timing parameters in the order they are added (DM1 / DM2 last: every TOA lies in a DMX
# bin, so they are nearly degenerate with the bins when those are free)
TIMING = ["F0", "F1", "RAJ", "DECJ", "PMRA", "PMDEC", "PX", "DM1", "DM2"]


@dataclass(frozen=True)
class Case:
    name: str
    ntim: int             # timing columns, Offset included (WaveX amplitudes beyond TIMING)
    ndmx: int             # DMX bins of the model
    nred: int             # PLRedNoise modes (0: no PLRedNoise component)
    dmx_free: bool = True  # the bins are fitted (columns) or frozen
    toas: str = "n530"    # TOA set
    layout: str = "full"  # eval(want_M=True) or "fit" (Session.FIT, the compact layout)
    mode: int = 1         # fit_step mode: 1 GLS, 0 WLS
    nsplit: int = 1       # PINT_NSPLIT
    vgram: bool = True
    vbin: bool = True
    cov_defer: int = 1
    schur: bool = True
    postfit: bool = False  # also the post-fit chi2 of the device's own residuals (the fused Woodbury dots)
    refused: bool = False  # pint_fit_step must refuse the batch before launching
    ecorr: bool = False   # an ECORR on every TOA (the "e" TOA sets: several frequencies per epoch)
    # wideband cases (wb_cases.py; test_wideband_sweep.py): DM-type columns beside the ntim others
    wb: bool = False         # wideband DM data on the TOAs, the DM rows in the fit step
    dm_free: tuple = ()      # free DM Taylor terms, of "DM", "DM1", "DM2"
    ndmjump: int = 0         # DMJUMPs of the model
    dmj_frozen: tuple = ()   # ... of which frozen (0-based, with non-zero values)
    dmx_frozen: tuple = ()   # frozen DMX bins (0-based, with non-zero values)
    dm12_zero: bool = False  # DM1 = DM2 = 0
    dmefac: bool = False     # DMEFAC 1.3 and a DMEQUAD on one flag value
    order: str = ""          # TOA order: "" (by time), "reverse", "shuffle"
    one_toa: bool = False    # bin 2 shrunk onto one TOA (its other TOAs lie in no bin)
    nesw: bool = False       # NE_SW free
    # ECORR cases (ecorr_cases.py; test_ecorr_sweep.py)
    ecorr_par: tuple = ()    # ((flag, value, ECORR in us), ...) instead of the one "ECORR -f fake 0.5"
    ecorr_off: bool = False  # pint_set_ecorr takes the pulsar off the compact layout (an epoch in two free bins, a TOA in two epochs)
    phoff: bool = False      # PhaseOffset with PHOFF frozen: no Offset column (ntim free parameters), the virtual ones row
    ndmn: int = 0            # ... of the nred Fourier modes, the last ndmn are PLDMNoise's
    dmx_edge: tuple = ()     # (a, mjd): the edge between bins a and a + 1 (0-based) moved to mjd

    @property
    def ndmx_free(self):
        return self.ndmx - len(self.dmx_frozen) if self.dmx_free else 0

    @property
    def m_dm(self):
        """Free dense DM-type columns: DM Taylor terms, DMJUMPs, NE_SW (k_wb_gram's m)."""
        return len(self.dm_free) + self.ndmjump - len(self.dmj_frozen) + int(self.nesw)

    @property
    def ndense(self):
        """Columns outside the DMX bins: the ntim timing columns and the DM-type ones."""
        return self.ntim + self.m_dm

    @property
    def ncol(self):
        return self.ndense + self.ndmx_free

    @property
    def K(self):
        return self.ncol + 2 * self.nred

    def but(self, **kw):
        return replace(self, **kw)


def timing_split(ntim):
    """(free TIMING parameters, WaveX harmonics) giving ntim timing columns with the Offset."""
    m = ntim - 1
    if m < 0:
        raise ValueError("a case has at least the Offset column")
    if m <= 7:
        return m, 0
    nb = 7 if (m - 7) % 2 == 0 else 6
    return nb, (m - nb) // 2


def wavex_freqs(nwx, nred=0):
    """Half-integer multiples of 1 / Tspan (1 / d) above the red-noise band (and above 2 / Tspan,
    clear of the spin-down parabola): below it a half-integer harmonic is nearly in the span of
    the weakly constrained low Fourier modes, and the normal equations lose ten digits."""
    return (max(nred, 2) + np.arange(nwx) + 0.5) / TSPAN


def par_of(c: Case) -> str:
    from pint_amd.simulation import pta_par
    par = pta_par(SEED, "", ndmx=c.ndmx, nmodes=max(c.nred - c.ndmn, 1))
    if c.nred - c.ndmn == 0:
        par = "\n".join(l for l in par.split("\n") if not l.startswith("TNRed")) + "\n"
    if c.ecorr_par:
        par += "".join(f"ECORR {k} {v} {x!r}\n" for k, v, x in c.ecorr_par)
    elif c.ecorr:
        par += "ECORR -f fake 0.5\n"
    if c.phoff:
        par += "PHOFF 0.05\n"
    if c.ndmn:
        par += f"TNDMAMP -13.2\nTNDMGAM 2.8\nTNDMC {c.ndmn}\n"
    if c.dmx_edge:
        a, x = c.dmx_edge
        sub = {f"DMXR2_{a + 1:04d}": x, f"DMXR1_{a + 2:04d}": x}
        par = "\n".join(f"{l.split()[0]} {sub[l.split()[0]]!r}" if l.split() and l.split()[0] in sub else l
                        for l in par.split("\n"))
    if c.wb:
        par = wideband_par(c, par)
    return par


# DMJUMP selectors of the wideband cases, in the model's order (wb_cases.wb_flags writes the
# columns): -fe has four values, -be three, -gp two, so no set of them sums to the DM column,
# and TOAs with -fe A -be X, -fe A -gp G, ... lie in two or three masks
DMJ_KEYS = (("-fe", "A"), ("-be", "X"), ("-fe", "B"), ("-be", "Y"), ("-gp", "G"))
DMJ_VALUES = (1.2e-3, -7e-4, 4e-4, -3e-4, 9e-4)
NE_SW = 7.9
WB_DM = (3.1, 1e-4, 1e-5)  # DM (one ulp 4.4e-16: the DM residuals' rounding stays below the Gram's bar), DM1, DM2


def wideband_par(c: Case, par: str) -> str:
    """pta_par's text with the wideband cases' changes: DM, DM1, DM2 values, the one-TOA bin's
    range, DMJUMPs, DMEFAC / DMEQUAD on -fe B, and NE_SW (SWM 0)."""
    dm = WB_DM if not c.dm12_zero else (WB_DM[0], 0.0, 0.0)
    rng = dmx_ranges(c)
    out = []
    for l in par.split("\n"):
        w = l.split()
        if w and w[0] in ("DM", "DM1", "DM2"):
            l = f"{w[0]} {dm[('DM', 'DM1', 'DM2').index(w[0])]!r}"
        elif w and w[0].startswith(("DMXR1_", "DMXR2_")):
            l = f"{w[0]} {rng[int(w[0][6:]) - 1][int(w[0][4]) - 1]:.5f}"
        out.append(l)
    par = "\n".join(out)
    for (k, v), x in list(zip(DMJ_KEYS, DMJ_VALUES))[:c.ndmjump]:
        par += f"DMJUMP {k} {v} {x!r}\n"
    if c.dmefac:
        par += "DMEFAC -fe B 1.3\nDMEQUAD -fe B 0.0002\n"
    if c.nesw:
        par += f"NE_SW {NE_SW!r}\nSWM 0\n"
    return par


def model_of(c: Case):
    from pint_amd.timing_model import get_model
    from pint_amd.wavex import wavex_setup
    m = get_model(par_of(c))
    nb, nwx = timing_split(c.ntim + int(c.phoff))
    free = list(TIMING[:nb])
    if nwx:
        wavex_setup(m, TSPAN, freqs=wavex_freqs(nwx, c.nred))
        free += [n for n in m.params if n.startswith(("WXSIN_", "WXCOS_"))]
    if c.wb:
        if nwx or any(p in free for p in ("DM1", "DM2")):
            raise ValueError("wideband cases: ntim <= 8 (no WaveX beside wideband data); DM terms by dm_free")
        free += list(c.dm_free)
        free += [n for k, n in enumerate(m.mask_params("DMJUMP")) if k not in c.dmj_frozen]
        if c.nesw:
            free.append("NE_SW")
    if c.dmx_free:
        free += [n for a, n in enumerate(m.dmx_params()) if a not in c.dmx_frozen]
    m.free_params = free
    return m


def dmx_rows(mjd, ndmx):
    """The DMX bin of every TOA (pta_par's ranges)."""
    edges = np.round(np.linspace(53000, 56652.01, ndmx + 1), 5)
    return np.clip(np.searchsorted(edges, np.asarray(mjd, dtype=np.float64), side="right") - 1, 0, ndmx - 1)


def dmx_ranges(c):
    """(DMXR1, DMXR2) of every bin of the case's model: pta_par's, bin 2 shrunk onto the first
    TOA at or after its lower edge with one_toa (TOAs evenly spaced over MJD0..MJD1)."""
    edges = np.round(np.linspace(53000, 56652.01, c.ndmx + 1), 5)
    rng = [(float(edges[i]), float(edges[i + 1])) for i in range(c.ndmx)]
    if c.one_toa:
        n = int(c.toas[1:])
        dt = TSPAN / (n - 1)
        k = int(np.ceil((rng[2][0] - MJD0) / dt))
        rng[2] = (round(MJD0 + (k - 0.4) * dt, 5), round(MJD0 + (k + 0.4) * dt, 5))
    if c.dmx_edge:
        a, x = c.dmx_edge
        rng[a], rng[a + 1] = (rng[a][0], float(x)), (float(x), rng[a + 1][1])
    return rng


def bin_rows(c, mjd):
    """The model's DMX bin of every TOA (index among all bins), -1 outside every bin."""
    mjd = np.asarray(mjd, dtype=np.float64)
    out = np.full(len(mjd), -1)
    for a, (r1, r2) in enumerate(dmx_ranges(c)):
        sel = (mjd >= r1) & (mjd <= r2)
        assert np.all(out[sel] < 0), "a TOA in two bins"
        out[sel] = a
    return out


def free_rows(c, mjd):
    """The compact DMX column (index among the free bins) of every TOA, -1 without one."""
    if not (c.dmx_frozen or c.one_toa or c.dmx_edge):
        return dmx_rows(mjd, c.ndmx)
    free = [a for a in range(c.ndmx) if a not in c.dmx_frozen]
    col = np.full(c.ndmx + 1, -1)
    col[free] = np.arange(len(free))
    return col[bin_rows(c, mjd)]


def rows_contiguous(drow, ndc):
    """Every column's TOAs are one contiguous row range (dcontig)."""
    return all(np.all(np.diff(np.flatnonzero(drow == a)) == 1) for a in range(ndc))


def _pad16(k):
    return (k + 15) // 16 * 16


def gram_T(kp):
    nt = kp // 16
    return (nt * (nt + 1) // 2 + GWAVES - 1) // GWAVES


def vgram_layout(c: Case, n, drow, nsplit):
    """(on the k_gram_v path, row tiles, DMX slots, LDS width) as pint_set_instances decides."""
    if not (c.vgram and c.ndmx_free >= 8 and c.nred <= VTRIG // 2 - 1 and c.ndense + 1 <= VMAXR0):
        return 0, 0, 0, 0
    if c.ecorr or not rows_contiguous(drow, c.ndmx_free):  # k_gram_v: no ECORR, contiguous bins
        return 0, 0, 0, 0
    wt, R, ndc = c.ndense + 1, 2 * c.nred, c.ndmx_free
    per = ((n + nsplit - 1) // nsplit + 3) // 4 * 4
    lo = [int(np.flatnonzero(drow == a)[0]) if np.any(drow == a) else 0 for a in range(ndc)]
    hi = [int(np.flatnonzero(drow == a)[-1]) + 1 if np.any(drow == a) else 0 for a in range(ndc)]

    def slots_ok(ntr):
        ns, kpv = 16 * ntr - wt, _pad16(16 * ntr + R)
        if ns < 1 or kpv > VMAXKP:
            return False
        for sp in range(nsplit):
            i0, i1 = sp * per, min(sp * per + per, n)
            seen = set()
            for a in range(ndc):
                if hi[a] <= lo[a] or lo[a] >= i1 or hi[a] <= i0:
                    continue
                if a % ns in seen:
                    return False
                seen.add(a % ns)
        return True

    ntr0 = (wt + 15) // 16
    for ntr in range(ntr0, min(3, ntr0 + 2) + 1):
        if not slots_ok(ntr):
            continue
        ns, kpv = 16 * ntr - wt, _pad16(16 * ntr + R)
        if c.vbin and kpv <= 96 and ns >= 16:
            # the binned DMX x Fourier tile: every 16 rows a wave takes hold at most two bins, of
            # distinct parity; a pulsar that fails it leaves the path
            for sp in range(nsplit):
                i0, i1 = min(sp * per, n), min(sp * per + per, n)
                QV = (i1 - i0 + VCH - 1) // VCH * 16
                for g in range(0, i1 - i0, 16):
                    b0 = b1 = -1
                    for r in range(g, min(g + 16, (g // QV + 1) * QV, i1 - i0)):
                        b = int(drow[i0 + r])
                        if b < 0 or b == b0 or b == b1:
                            continue
                        if b0 < 0:
                            b0 = b
                        elif b1 < 0 and ((b ^ b0) & 1):
                            b1 = b
                        else:
                            return 0, 0, 0, 0
        return 1, ntr, ns, kpv
    return 0, 0, 0, 0


def predict_plan(c: Case, n, mjd):
    """The plan of pint_fit_step(c.mode) for a batch of this one pulsar (wideband DM rows with
    c.wb; default options but those the case names), in
    Session.last_plan()'s form.  mjd: the TOAs' MJDs in the order they are uploaded."""
    plan = dict(gram_T=(), gram_v=(), solve="none", gram_ecorr=False, gram_s=False, greduce=False, dmx_rows=False,
                dmx=False, ecorr_dmx=False, wb_gram=False, fuse_sigma=False, side_sigma=False, do_sigma=False,
                schur=False, cov_deferred=False, nsplit=0, solve_dmx_waves=0, sigma_waves=0)
    if c.refused:
        return plan
    K, Kp = c.K, _pad16(c.K + 1)
    cmp = c.layout == "fit"
    dsplit = c.ndmx_free >= 8 and not c.ecorr_off  # (pint_set_ecorr: the Schur rows would couple DMX columns)
    Kd = c.ndense + 2 * c.nred
    Kpd = _pad16(Kd + 1)
    nsplit = min(c.nsplit, max(1, (n + 63) // 64))
    plan["nsplit"] = nsplit
    vg = 0
    if dsplit:
        drow = free_rows(c, mjd)
        vg, ntr, ns, kpv = vgram_layout(c, n, drow, nsplit)
    vgp = bool(cmp and vg)
    if vgp:
        C = kpv // 16
        plan["gram_v"] = ((10 * (ntr - 1) + C, bool(c.vbin and C <= 6)),)
    else:
        kp = Kpd if (cmp and dsplit) else Kp
        if kp <= 32 and n <= GS_MAXN:
            plan["gram_s"] = True
        else:
            plan["gram_T"] = (gram_T(kp),)
        plan["dmx_rows"] = bool(cmp and dsplit)
        # rows of a bin that are not contiguous: k_dmx gathers them (k_dmx_rows returns at once)
        plan["dmx"] = bool(cmp and dsplit and not rows_contiguous(drow, c.ndmx_free))
    nep = bool(c.ecorr and c.mode == 1)  # the ECORR Schur partial: k_gram<T, ch, true> and one more part
    if nep and plan["gram_s"]:
        plan["gram_T"] = (1,)  # small instances: k_gram_s, their ECORR rows by k_gram<1, 128, true>
    plan["gram_ecorr"] = nep
    # compact layout with ECORR (every epoch within one DMX column): its share of the DMX rows
    plan["ecorr_dmx"] = bool(nep and plan["dmx_rows"])
    plan["wb_gram"] = bool(c.wb and cmp)
    plan["greduce"] = nsplit + nep > 1 or vgp
    # the solve
    mode = c.mode
    kn = 2 * c.nred + 1 if mode == 1 else 0
    Ks, skip, dmx_ok = 0, 0, cmp
    if cmp and dsplit:
        kd = c.ndense if mode == 0 else Kd
        nbd, nbk, nbs = (kd + 15) // 16, (c.ndmx_free + 15) // 16, (kn + 15) // 16
        blk = nbd * (nbd + 1) // 2 + nbd * nbk
        lds_x = 8 * (max(blk, nbs * (nbs + 1) // 2) * 256 + (5 * nbd + 6 * nbk) * 16)
        if blk > SD_MAXBLK or nbd > 17 or nbs > BS_MAXNB or lds_x > LDS - 512:
            dmx_ok = False
        skip = 1 if dmx_ok else 0
    if not skip:
        Ks = c.ncol if mode == 0 else K
    any_noise = mode == 1 and (c.nred > 0 or c.ecorr)
    nbs_sig = (2 * c.nred + 1 + 15) // 16 if any_noise else 0
    if any_noise and nbs_sig <= BS_MAXNB and skip and Ks == 0:
        plan["fuse_sigma"] = True
    elif any_noise and nbs_sig <= BS_MAXNB:
        plan["side_sigma"] = True
        plan["sigma_waves"] = 4 if nbs_sig <= 5 else 16
    elif any_noise:
        plan["do_sigma"] = True
    if skip:
        xw = c.cov_defer == 2
        plan["cov_deferred"] = xw
        plan["schur"] = bool(xw and c.schur)
        plan["solve_dmx_waves"] = 8 if (nbd <= 8 and (not plan["fuse_sigma"] or nbs_sig <= 9)) else 16
    else:
        nbx = max((Ks + 15) // 16, (kn + 15) // 16)
        if nbx > BS_MAXNB:
            plan["solve"] = "column"
        elif nbx <= 1 and Ks <= 8:
            plan["solve"] = "lanes4" if Ks <= 4 else "lanes8"
        elif nbx <= 2:
            plan["solve"] = "blk1"
        else:
            plan["solve"] = "blk4" if nbx <= 5 else "blk16"
    return plan


def column_solve_fits(K):
    """k_solve's LDS: the packed triangle, five vectors and eight scalars in doubles."""
    return 8 * (K * (K + 1) // 2 + 5 * K + 8) <= LDS


def vgram_keys_reachable():
    """Every k_gram_v key 10 (R - 1) + C the layout rules can give: R row tiles (1..3) hold the
    timing columns, the residual and the DMX slots; the 2 nred <= 62 Fourier columns add
    ceil(nred / 8) <= 4 column tiles (none without red noise), up to VMAXKP / 16 = 7."""
    keys = set()
    for R in (1, 2, 3):
        for nred in range(0, VTRIG // 2):
            C = _pad16(16 * R + 2 * nred) // 16
            if 16 * C <= VMAXKP:
                keys.add(10 * (R - 1) + C)
    return sorted(keys)


# ---- the cases -------------------------------------------------------------------------------
def _full(name, K, nred, toas="n1100", ndmx=BASE_NDMX, dmx_free=False, **kw):
    """A full-layout case of K columns: K = timing + free DMX + 2 nred."""
    ntim = K - 2 * nred - (ndmx if dmx_free else 0)
    return Case(name, ntim, ndmx, nred, dmx_free=dmx_free, toas=toas, layout="full", **kw)


def cases():
    out = []
    # general solve, K on each side of every switch (full layout; n = 530 > GS_MAXN keeps the
    # narrow ones on k_gram<1>); K + 1 = 16, 17, 32, 33 are the Gram's tile edges as well
    for K in (4, 5, 8, 9):
        out.append(_full(f"solve_K{K}", K, 1, toas="n530"))
    for K in (15, 16, 17, 31, 32, 33):
        out.append(_full(f"solve_K{K}", K, 4, toas="n530"))
    for K in (80, 81, 95, 96):
        out.append(_full(f"solve_K{K}", K, 20, toas="n530", dmx_free=True))
    # k_gram_s
    out.append(_full("grams_Kp16", 12, 2, toas="n300"))
    out.append(_full("grams_Kp32", 31, 8, toas="n300"))
    # full-layout Gram: the widest nt of T = 1..6 and the narrowest of T = 2, 3 (GLS; Kp = 208
    # holds K = 192 and 193, the blocked / column solve switch, and 196, the last K k_solve takes)
    out.append(_full("gram_Kp80", 79, 30))
    out.append(_full("gram_Kp96", 90, 30, dmx_free=True))
    out.append(_full("gram_Kp112", 111, 30, dmx_free=True))
    out.append(_full("gram_Kp128", 120, 30, dmx_free=True))
    out.append(_full("gram_Kp144", 143, 30, dmx_free=True))
    out.append(_full("gram_Kp160", 159, 40, dmx_free=True))
    out.append(_full("gram_Kp192", 191, 60, dmx_free=True))
    out.append(_full("solve_K192", 192, 60, dmx_free=True))
    out.append(_full("solve_K193", 193, 60, dmx_free=True))
    # (112 free bins: on the compact layout the same model fits k_solve_dmx, 6 dense blocks x 7)
    out.append(_full("solve_K196", 196, 30, ndmx=112, dmx_free=True))
    out.append(_full("solve_K197", 197, 30, ndmx=112, dmx_free=True, refused=True))
    out.append(_full("solve_K197_fit", 197, 30, ndmx=112, dmx_free=True).but(layout="fit"))
    # T = 7, 8, 9: beyond k_solve's LDS as a GLS system, so a WLS step (mode 0 solves the ncol
    # timing columns; the Gram still spans all K)
    out.append(_full("gram_Kp224", 223, 60, dmx_free=True, mode=0))
    out.append(_full("gram_Kp240", 239, 60, dmx_free=True, mode=0))
    out.append(_full("gram_Kp256", 255, 60, dmx_free=True, mode=0))
    # the ECORR variants k_gram<T, ch, true> of T = 2 and 3
    out.append(_full("ecorr_Kp112", 111, 30, toas="e1100", dmx_free=True, ecorr=True))
    out.append(_full("ecorr_Kp144", 143, 30, toas="e1100", dmx_free=True, ecorr=True))
    # N-splits on a full-layout case
    for ns in (3, 5):
        out.append(_full(f"gram_Kp144_ns{ns}", 143, 30, dmx_free=True, nsplit=ns))
    # generated-Fourier Gram: every reachable key, the binned body on and off
    vg = []
    for R, ntim, ndmx in ((1, 6, 9), (2, 6, 20), (3, 6, 33)):
        for nred in (0, 8, 16, 24, 31):
            vg.append(Case(f"vg_R{R}_nred{nred}", ntim, ndmx, nred, layout="fit"))
    vg.append(Case("vg_R1_nred1", 6, 9, 1, layout="fit"))
    vg.append(Case("vg_R2_nred30", 6, 20, 30, layout="fit"))
    # the timing columns alone fill the first row tiles (slots share the last one)
    vg.append(Case("vg_R2_wt21", 20, 10, 8, layout="fit"))
    vg.append(Case("vg_R3_wt37", 36, 10, 8, layout="fit"))
    vg.append(Case("vg_R3_wt40", 39, 8, 8, layout="fit"))
    out += vg
    out += [c.but(name=c.name + "_novb", vbin=False) for c in vg]
    for ns in (3, 5):
        out.append(Case(f"vg_R2_nred16_ns{ns}", 6, 20, 16, layout="fit", nsplit=ns))
    # nred = 32 leaves the generated-Fourier path
    out.append(Case("vg_off_nred32", 6, 20, 32, layout="fit"))
    # DMX-eliminated solve: dense block of 8 and 9 column blocks, the largest block count that
    # fits and the two fall-backs, the fused Sigma of 9 and 10 blocks
    dm = [Case("dmx_nbd8", 8, 16, 60, toas="n1100", layout="fit"),
          Case("dmx_nbd9", 9, 16, 60, toas="n1100", layout="fit"),
          Case("dmx_blk75_nbs9", 10, 20, 68, toas="n1100", layout="fit"),
          Case("dmx_nbs10", 10, 20, 72, toas="n1100", layout="fit")]
    for c in dm:
        out.append(c.but(name=c.name + "_d0", cov_defer=0))
        out.append(c.but(name=c.name + "_d2", cov_defer=2))
        out.append(c.but(name=c.name + "_d2_noschur", cov_defer=2, schur=False))
    out.append(Case("dmx_blk76_lds", 9, 65, 52, toas="n1100", layout="fit"))
    out.append(Case("dmx_blk77", 10, 16, 80, toas="n1100", layout="fit"))
    # Sigma: k_sigma<4> / <16>, the blocked / in-solve switch, the fused post-fit dots' limit
    out.append(_full("sigma_nred39", 90, 39))
    out.append(_full("sigma_nred40", 92, 40))
    out.append(_full("sigma_nred95", 192, 95))
    out.append(_full("sigma_nred96", 194, 96))
    out.append(Case("wfuse_nred63", 8, BASE_NDMX, 63, toas="n1100", layout="fit", postfit=True))
    out.append(Case("wfuse_nred64", 8, BASE_NDMX, 64, toas="n1100", layout="fit", postfit=True))
    return out
