"""Polycos: tempo's piecewise polynomial phase predictor (reference ``src/pint/polycos.py``).

An entry covers ``mjd_span`` minutes around ``tmid`` and predicts, with dt = (t - tmid) 1440 minutes,

    phase(t) = rphase + 60 f0 dt + coeffs[0] + coeffs[1] dt + coeffs[2] dt^2 + ...
    freq(t)  = f0 + (coeffs[1] + 2 coeffs[2] dt + ...) / 60

``Polycos.read`` / ``write_polyco_file`` handle tempo's ``polyco.dat``; ``find_entry`` and the
``eval_*`` methods have the reference's semantics.  The ``eval_*`` methods and ``htest`` take
``device=True`` (the default): the table is put on the device once (pint_set_polycos) and the times go
there as exact (hi, lo) pairs of doubles -- a float64 MJD has an ulp of 0.6 us, so a longdouble time
cannot travel as one double -- to k_polyco_eval / k_polyco_trig.  ``device=False`` evaluates entry by
entry in numpy longdouble as the reference does, and needs no GPU.

Deliberate deviations from the reference:

* ``eval_abs_phase`` returns the phases in input order.  The reference returns them grouped by
  entry, which is the same thing for the sorted input its docstring asks for.
* ``write_polyco_file`` leaves the caller's coefficients alone (the reference adds the rounding
  excess of the printed reference phase into ``coeffs[0]`` on every call, so its second write differs
  from its first).  The file equals the reference's first write.
* when ``ncoeff`` is not a multiple of 3 the coefficient block ends with a newline, as tempo's does;
  the reference glues the next entry's first line onto it and then cannot read its own file.
* only the tempo format is built.
"""
from __future__ import annotations

import io
import os
from collections import namedtuple

import numpy as np

from . import eventstats

__all__ = ["Phase", "PolycoEntry", "PolycoTable", "Polycos", "tempo_polyco_table_reader", "tempo_polyco_table_writer"]

LD = np.longdouble
MIN_PER_DAY = 1440.0
COLUMNS = ("psr", "date", "utc", "tmid", "dm", "doppler", "logrms", "mjd_span", "t_start", "t_stop", "obs", "obsfreq",
           "binary_phase", "f_orbit", "entry")
FORMATS = ("tempo",)


class Phase(namedtuple("Phase", "int frac")):
    """A pulse phase as longdouble arrays (int, frac) with frac in [-1/2, 1/2) (reference phase.py)."""
    __slots__ = ()

    def __new__(cls, a, b=None):
        a = np.atleast_1d(np.asarray(a, dtype=LD))
        fa, ia = np.modf(a)
        if b is not None:
            fb, ib = np.modf(np.atleast_1d(np.asarray(b, dtype=LD)))
            fa, ia = fa + fb, ia + ib
        fa, ia = np.array(fa, dtype=LD), np.array(ia, dtype=LD)
        low = fa < -0.5
        fa[low] += 1.0
        ia[low] -= 1.0
        high = fa >= 0.5
        fa[high] -= 1.0
        ia[high] += 1.0
        return super().__new__(cls, ia, fa)

    def __add__(self, other):
        f = self.frac + other.frac
        carry = np.modf(f)[1]
        return Phase(self.int + other.int + carry, f - carry)

    def __neg__(self):
        return Phase(-self.int, -self.frac)

    def __sub__(self, other):
        return self + (-other)

    @property
    def value(self):
        return self.int + self.frac


def split_pairs(v):
    """A float64 or longdouble array as exact (hi, lo) float64 pairs: hi = float64(v), lo = float64(v - hi)
    (engine.split_ld's rule, elementwise)."""
    v = np.atleast_1d(np.asarray(v))
    if v.dtype != LD:
        hi = np.ascontiguousarray(v, dtype=np.float64)
        return hi, np.zeros_like(hi)
    hi = np.ascontiguousarray(v.astype(np.float64))
    with np.errstate(invalid="ignore"):
        lo = np.ascontiguousarray((v - hi.astype(LD)).astype(np.float64))
    lo[~np.isfinite(hi)] = 0.0
    return hi, lo


class PolycoEntry:
    """One polyco entry: tmid (MJD), mjdspan (minutes), the reference phase as (rph_int, rph_frac), f0 (Hz),
    ncoeff and the coefficients.  Everything is kept in numpy longdouble; ``mjdspan``, ``tstart`` and
    ``tstop`` are in days."""

    def __init__(self, tmid, mjdspan, rph_int, rph_frac, f0, ncoeff, coeffs):
        self.tmid = LD(tmid)
        self.mjdspan = LD(mjdspan / MIN_PER_DAY)
        self.tstart = self.tmid - self.mjdspan / 2
        self.tstop = self.tmid + self.mjdspan / 2
        self.f0 = LD(f0)
        self.ncoeff = int(ncoeff)
        self.rphase = Phase(rph_int, rph_frac)
        self.coeffs = np.array(coeffs, dtype=LD)

    def __repr__(self):
        return (f"PolycoEntry(tmid={self.tmid!r}, span={float(self.mjdspan * MIN_PER_DAY):g} min, "
                f"rphase={self.rphase.int[0]!r}+{self.rphase.frac[0]!r}, f0={self.f0!r}, ncoeff={self.ncoeff})")

    def _dt(self, t):
        return (np.asarray(t, dtype=LD) - self.tmid) * LD(MIN_PER_DAY)

    def evalabsphase(self, t):
        """The absolute phase at the times t (MJD) as a Phase: Horner's rule with the running value kept
        as (int, frac), as the reference does, so that the large 60 f0 dt term costs no fraction bits."""
        dt = np.atleast_1d(self._dt(t))
        p = Phase(np.full(dt.shape, self.coeffs[self.ncoeff - 1], dtype=LD))
        for i in range(self.ncoeff - 2, -1, -1):
            p = Phase(dt * p.int) + Phase(dt * p.frac) + Phase(np.full(dt.shape, self.coeffs[i], dtype=LD))
        return p + Phase(np.broadcast_to(self.rphase.int, dt.shape), np.broadcast_to(self.rphase.frac, dt.shape)) \
            + Phase(dt * LD(60.0) * self.f0)

    def evalphase(self, t):
        """The fractional phase at t, in [-1/2, 1/2)."""
        return self.evalabsphase(t).frac

    def evalfreq(self, t):
        """The spin frequency (Hz) at t."""
        dt = self._dt(t)
        s = LD(0.0)
        for i in range(1, self.ncoeff):
            s = s + LD(i) * self.coeffs[i] * dt ** (i - 1)
        return self.f0 + s / LD(60.0)

    def evalfreqderiv(self, t):
        """The spin frequency derivative (Hz/s) at t."""
        dt = self._dt(t)
        s = LD(0.0)
        for i in range(2, self.ncoeff):
            s = s + LD(i) * LD(i - 1) * self.coeffs[i] * dt ** (i - 2)
        return s / LD(3600.0)


class PolycoTable:
    """The polyco table: one dict per entry with the columns COLUMNS (``binary_phase`` and ``f_orbit``
    for binaries only).  ``tab["t_start"]`` is a column (numeric ones as arrays, longdouble where
    the reference's are), ``tab[i]`` a row (a dict), ``len(tab)`` the entry count."""

    LONG = ("tmid", "t_start", "t_stop")

    def __init__(self, rows=(), meta=None):
        self.rows = [dict(r) for r in rows]
        self.meta = dict(meta or {"name": "Polyco Data Table"})

    def __len__(self):
        return len(self.rows)

    def __iter__(self):
        return iter(self.rows)

    @property
    def colnames(self):
        return [c for c in COLUMNS if self.rows and c in self.rows[0]]

    def __getitem__(self, key):
        if isinstance(key, str):
            if not self.rows or key not in self.rows[0]:
                raise KeyError(key)
            col = [r[key] for r in self.rows]
            if key in self.LONG:
                return np.array(col, dtype=LD)
            if key == "entry":
                out = np.empty(len(col), dtype=object)
                out[:] = col
                return out
            return np.array(col)
        if isinstance(key, slice):
            return PolycoTable(self.rows[key], self.meta)
        return self.rows[key]


def _open(f, mode):
    return (f, False) if hasattr(f, "read" if "r" in mode else "write") else (open(os.fspath(f), mode), True)


def _ld(s):
    return LD(s.replace("D", "e").replace("d", "e"))


def tempo_polyco_table_reader(filename):
    """Read a tempo polyco.dat (tz-polyco.txt: two header lines, then three coefficients per line)
    into a PolycoTable.  tmid, the reference phase, f0 and the coefficients are parsed as longdouble."""
    f, close = _open(filename, "r")
    try:
        lines = [ln for ln in f.read().splitlines()]
    finally:
        if close:
            f.close()
    rows, k = [], 0
    while k < len(lines):
        if not lines[k].strip():
            k += 1
            continue
        a = lines[k].split()
        b = lines[k + 1].split()
        k += 2
        ri, rf = b[0].split(".")
        rph_int, rph_frac = LD(ri), LD("." + rf)
        if rph_int < 0:
            rph_frac = -rph_frac
        span, nc = int(b[3]), int(b[4])
        co = []
        for _ in range((nc + 2) // 3):
            co += [_ld(c) for c in lines[k].split()]
            k += 1
        entry = PolycoEntry(LD(a[3]), span, rph_int, rph_frac, LD(b[1]), nc, np.array(co, dtype=LD))
        row = {"psr": a[0], "date": a[1], "utc": float(a[2]), "tmid": LD(a[3]), "dm": float(a[4]), "doppler": float(a[5]),
               "logrms": float(a[6]), "mjd_span": span, "t_start": entry.tstart, "t_stop": entry.tstop, "obs": b[2],
               "obsfreq": float(b[5])}
        if len(b) >= 8:
            row["binary_phase"], row["f_orbit"] = float(b[6]), float(b[7])
        row["entry"] = entry
        rows.append(row)
    return PolycoTable(rows)


def tempo_polyco_table_writer(table, filename="polyco.dat"):
    """Write a PolycoTable as a tempo polyco.dat.  The reference phase is printed to 6 decimals and the
    rounding excess goes into the first printed coefficient (the caller's entry is not changed)."""
    if len(table) == 0:
        raise ValueError("Empty polyco table! Please make sure polycoTable has data.")
    out = io.StringIO()
    for row in table:
        e = row["entry"]
        name = row["psr"][1:] if row["psr"][0] == "J" else row["psr"]
        out.write("{:10.10s} {:>9.9s}{:11.2f}{:20.11f}{:21.6f} {:6.3f}{:7.3f}\n".format(
            name, row["date"], row["utc"], row["tmid"], row["dm"], row["doppler"], row["logrms"]))
        fr, neg = e.rphase.frac[0], bool(e.rphase.frac[0] < 0)
        pos = fr + neg                     # the fraction in [0, 1)
        printed = np.round(pos, 6)
        excess = pos - printed
        rph = "{:13d}".format(int(e.rphase.int[0]) - neg) + "{:.6f}".format(printed)[1:]
        orbit = "{:7.4f}{:9.4f}".format(row["binary_phase"], row["f_orbit"]) if "binary_phase" in row else ""
        out.write("{:20s} {:17.12f}{:>5s}{:5d}{:5d}{:10.3f}{:16s}\n".format(
            rph, e.f0, row["obs"], row["mjd_span"], e.ncoeff, row["obsfreq"], orbit))
        co = np.array(e.coeffs, dtype=LD)
        co[0] += excess
        for i, c in enumerate(co):
            out.write("{:25.17e}".format(c))
            if (i + 1) % 3 == 0:
                out.write("\n")
        if len(co) % 3:
            out.write("\n")
    f, close = _open(filename, "w")
    try:
        f.write(out.getvalue())
    finally:
        if close:
            f.close()


MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")


def _date_utc(minutes):
    """("dd-Mon-yy", hhmmss.ss as a float) of a UTC time given in whole minutes of MJD."""
    import datetime
    d = datetime.date(1858, 11, 17) + datetime.timedelta(days=minutes // 1440)
    hh, mm = divmod(minutes % 1440, 60)
    return f"{d.day:02d}-{MONTHS[d.month - 1]}-{d.year % 100:02d}", float(hh * 10000 + mm * 100)


def _check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError(f"Unknown polyco file format '{fmt}'\nPlease use function 'Polyco.add_polyco_file_format()'"
                         " to register the format\n")


class Polycos:
    """A table of polyco entries with the reference's interface, evaluated on the device."""

    def __init__(self, filename=None, format="tempo"):
        self.fileName = filename
        self.polycoTable = None
        self._session = None
        self._uploaded = None
        if filename is not None:
            _check_format(format)
            self.fileFormat = format
            self.polycoTable = tempo_polyco_table_reader(filename)
            if len(self.polycoTable) == 0:
                raise ValueError("Zero polycos found for table")

    @classmethod
    def read(cls, filename, format="tempo"):
        """Read a polyco file (only the tempo format is built)."""
        return cls(filename, format=format)

    def read_polyco_file(self, filename, format="tempo"):
        """Deprecated in the reference, where it only raises: use ``Polycos.read``."""
        raise DeprecationWarning("Use `p=pint.polycos.Polycos.read()` rather than `p.read_polyco_file()`")

    def write_polyco_file(self, filename="polyco.dat", format="tempo"):
        """Write the table (tempo format).  See the module docstring for the two deviations."""
        _check_format(format)
        tempo_polyco_table_writer(self.polycoTable, filename)

    def __len__(self):
        return len(self.polycoTable)

    def __getitem__(self, item):
        return self.polycoTable[item]

    @classmethod
    def from_table(cls, table):
        out = cls()
        out.polycoTable = table if isinstance(table, PolycoTable) else PolycoTable(table)
        if len(out.polycoTable) == 0:
            raise ValueError("Zero polycos found for table")
        return out

    # ---- generation ----------------------------------------------------------------------------
    @classmethod
    def generate_polycos(cls, model, mjdStart, mjdEnd, obs, segLength, ncoeff, obsFreq, maxha=12.0, method="TEMPO",
                         numNodes=20, progress=False):
        """Polycos of ``model`` between mjdStart and mjdEnd at observatory ``obs`` (tempo's method, as
        the reference's generate_polycos): segments of segLength minutes around the mid-points
        arange(int(mjdStart 24) 60, int(mjdEnd 24) 60 + segLength, segLength) / 1440, each a polynomial
        of ncoeff coefficients fitted to the model's phase on numNodes nodes (ncoeff + 1 when numNodes <
        ncoeff) spread evenly over the segment.  obsFreq in MHz; 0 means infinite frequency.

        All segments go through one evaluation: the nodes and mid-points of every segment are prepared
        on the host as one TOA list (get_TOAs_array), their absolute phases are formed on the device,
        and pint_polyco_fit solves every segment's least-squares problem there (Householder QR; the
        reference calls np.polyfit per segment).  The table stays on the device for the eval_* methods.

        The TOAs are prepared with include_bipm=False: the reference's get_TOAs_array default would
        apply TT(BIPM), whose table is not bundled.  A model without TZRMJD gets one, as the reference's
        phase(abs_phase=True) does on the first TOAs it sees: the first segment's mid-point (its float64
        MJD, at the barycenter and infinite frequency), left on the caller's model.  ``progress`` is accepted and
        ignored (there is no per-segment loop to report on)."""
        from . import _lib as L
        from .engine import Session, build_layout, pack_table, split_ld
        from .toa import get_TOAs_array
        mjdStart, mjdEnd, segLength = LD(mjdStart), LD(mjdEnd), int(segLength)
        if maxha != 12.0:
            raise ValueError("Maximum hour angle != 12.0 is not supported.")
        if method != "TEMPO":
            raise NotImplementedError("Only TEMPO method has been implemented.")
        ncoeff, numNodes = int(ncoeff), int(numNodes)
        if numNodes < ncoeff:
            numNodes = ncoeff + 1
        if not 1 <= ncoeff <= L.MAX_POLYCO_COEFF or numNodes > L.MAX_POLYCO_NODES:
            raise ValueError(f"{ncoeff} coefficients on {numNodes} nodes: at most {L.MAX_POLYCO_COEFF} coefficients "
                             f"and {L.MAX_POLYCO_NODES} nodes are built")
        obsFreq = float(obsFreq)
        minutes = np.arange(int(mjdStart * 24) * 60, int(mjdEnd * 24) * 60 + segLength, segLength)
        tmids = minutes.astype(LD) / LD(MIN_PER_DAY)
        nseg = len(tmids)
        if nseg == 0:
            raise ValueError("Zero polycos found for table")
        span = LD(segLength / MIN_PER_DAY)
        nodes = np.array([np.linspace(tm - span / 2, tm + span / 2, numNodes) for tm in tmids], dtype=LD)
        if "TZRMJD" not in model or model.TZRMJD.value is None:
            cls._add_tzr(model, tmids[0])
        # per segment its nodes then its mid-point; the parts as the reference hands them over (the
        # integer part and the fraction, the fraction rounded to a double)
        rows = np.concatenate([nodes, tmids[:, None]], axis=1).reshape(-1)
        fr, ip = np.modf(rows)
        toas = get_TOAs_array((ip, fr.astype(np.float64)), obs, freqs=obsFreq, model=model, include_bipm=False)
        dt = (nodes - tmids[:, None]) * LD(MIN_PER_DAY)
        dth, dtl = split_pairs(dt.reshape(-1))
        f0h, f0l = split_ld(model.F0.value)
        s = Session()
        try:
            lay = s.add(build_layout(model, toas))
            s.set_instances([(lay, pack_table(lay))])
            s.eval(False)
            fit = s.polyco_fit(nseg, numNodes, ncoeff, dth, dtl, model.F0.value)
        except Exception:
            s.close()
            raise
        co, ri, rfh, rfl, rms = (fit[k] for k in ("coeffs", "rph_int", "rph_frac_hi", "rph_frac_lo", "rms"))
        binary = cls._binary_columns(model, toas, nseg, numNodes) if model.binary else None
        rows = []
        for k in range(nseg):
            e = PolycoEntry(tmids[k], segLength, LD(ri[k]), LD(rfh[k]) + LD(rfl[k]), model.F0.value, ncoeff, co[k])
            date, utc = _date_utc(int(minutes[k]))
            row = {"psr": model.PSR.value, "date": date, "utc": utc, "tmid": tmids[k],
                   "dm": float(model.DM.value) if "DM" in model else 0.0,
                   "doppler": 0.0, "logrms": 0.0, "mjd_span": segLength, "t_start": e.tstart, "t_stop": e.tstop, "obs": obs,
                   "obsfreq": obsFreq}
            if binary is not None:
                row["binary_phase"], row["f_orbit"] = float(binary[0][k]), binary[1]
            row["entry"] = e
            rows.append(row)
        out = cls.from_table(PolycoTable(rows))
        out.fit_rms = rms
        # the fit's coefficients and rphase are adopted where they are: no upload of the table
        hdr = np.zeros((L.PC_NF, nseg))
        for k, r in enumerate(rows):
            e = r["entry"]
            hdr[0, k], hdr[1, k] = split_ld(e.tmid)
            hdr[2, k], hdr[3, k] = split_ld(e.tstart)
            hdr[4, k], hdr[5, k] = split_ld(e.tstop)
            hdr[9, k], hdr[10, k] = f0h, f0l
        try:
            s.set_polycos(hdr, ncoeff=ncoeff)
        except Exception:
            s.close()
            raise
        out._session, out._uploaded = s, out.polycoTable
        return out

    @staticmethod
    def _add_tzr(model, tmid):
        """AbsPhase for a model without it, as the reference's add_tzr_toa leaves it: TZRMJD = the float64
        MJD of tmid, TZRSITE ssb, TZRFRQ infinite."""
        from . import parameter as P
        v = float(tmid)
        for name in ("TZRMJD", "TZRSITE", "TZRFRQ"):
            if name in model:
                continue
            p = P.make_param(name)
            p.value = None
            model.add_param(p)
        model.TZRMJD.value = LD(v)
        model.TZRSITE.value = "ssb"
        model.TZRFRQ.value = np.inf
        model.TZRMJD.mjd_pair = (float(np.floor(v)), float(v - np.floor(v)))

    @staticmethod
    def _binary_columns(model, toas, nseg, nnode):
        """(binary_phase per segment, f_orbit): the mean orbital phase in cycles at each mid-point
        (timing_model.py:839 orbital_phase: the orbit count at the barycentric time, mod 1) and 1 / PB
        [1/d].  The barycentric time is the TDB minus the delays in front of the binary's; they are
        evaluated on the device with a copy of the model that has no binary (the frequency-dependent
        delays, microseconds, stay in: 1e-11 of an orbit)."""
        mids = toas[np.arange(nseg) * (nnode + 1) + nnode]
        mids.prepared = toas.prepared
        from .timing_model import BIN_IDS
        m = model.copy()
        for name in [n for n in m.params if n in BIN_IDS or n in model.fb_terms()]:
            del m._params[name]
        m.components = type(m.components)((k, v) for k, v in m.components.items() if not k.startswith("Binary"))
        object.__setattr__(m, "_order", None)  # (the caches add_param / remove_param reset)
        object.__setattr__(m, "_names", {})
        m.binary = None
        m.free_params = []
        bary = mids.tdbld - np.asarray(m.delay(mids), dtype=LD) / LD(86400.0)
        ep = model.TASC if "TASC" in model and model.TASC.value is not None else model.T0
        tt0 = (bary - LD(ep.value)) * LD(86400.0)
        fbs = model.fb_terms()
        if fbs and model[fbs[0]].value is not None:
            orbits, fact = LD(0), LD(1)
            for i, n in enumerate(fbs):
                fact = fact * (i + 1)
                orbits = orbits + LD(model[n].value or 0) * tt0 ** (i + 1) / fact
        else:
            pb = LD(model.PB.value) * LD(86400.0)
            pbdot = LD(model.PBDOT.value or 0) if "PBDOT" in model else LD(0)
            if "XPBDOT" in model and model.XPBDOT.value:
                pbdot = pbdot + LD(model.XPBDOT.value)
            orbits = tt0 / pb - LD(0.5) * pbdot * (tt0 / pb) ** 2
        anom = np.remainder((orbits * LD(2) * LD(np.pi)).astype(np.float64), 2 * np.pi)
        return anom / (2 * np.pi), float(1 / model.pb()[0])

    # ---- the entry of a time -------------------------------------------------------------------
    def find_entry(self, t):
        """The index of the entry covering each time (MJD): count(t_start < t) - 1, which must equal
        count(t_stop < t) -- so a time exactly on a boundary belongs to the earlier entry.  ValueError
        when a time is not covered."""
        if self.polycoTable is None:
            raise ValueError("polycoTable not set!")
        t = np.atleast_1d(np.asarray(t))
        a = np.searchsorted(self.polycoTable["t_start"], t) - 1
        b = np.searchsorted(self.polycoTable["t_stop"], t)
        if not np.array_equal(a, b):
            raise ValueError("Some input times not covered by Polyco entries.")
        return a

    # ---- the device ----------------------------------------------------------------------------
    def _device(self):
        """The session holding the table (created and uploaded at first use; uploaded again when the
        table object was replaced -- after editing an entry in place, assign ``polycoTable`` anew)."""
        from . import _lib as L
        from .engine import Session
        if self._session is None:
            self._session = Session()
        tab = self.polycoTable
        if self._uploaded is not tab:
            n = len(tab)
            order = np.argsort(tab["t_start"], kind="stable")
            ents = [tab[int(i)]["entry"] for i in order]
            nc = max(e.ncoeff for e in ents)
            if nc > L.MAX_POLYCO_COEFF:
                raise ValueError(f"{nc} coefficients: the device path takes at most {L.MAX_POLYCO_COEFF}")
            hdr = np.zeros((L.PC_NF, n))
            co = np.zeros((n, nc), dtype=LD)
            for k, e in enumerate(ents):
                hdr[0, k], hdr[1, k] = (float(x[0]) for x in split_pairs(e.tmid))
                hdr[2, k], hdr[3, k] = (float(x[0]) for x in split_pairs(e.tstart))
                hdr[4, k], hdr[5, k] = (float(x[0]) for x in split_pairs(e.tstop))
                ph = Phase(e.rphase.int, e.rphase.frac)  # (normalised, whatever the caller put there)
                hdr[6, k] = float(ph.int[0])
                hdr[7, k], hdr[8, k] = (float(x[0]) for x in split_pairs(ph.frac[0]))
                hdr[9, k], hdr[10, k] = (float(x[0]) for x in split_pairs(e.f0))
                co[k, :e.ncoeff] = e.coeffs[:e.ncoeff]
            chi, clo = split_pairs(co.reshape(-1))
            self._session.set_polycos(hdr, chi.reshape(n, nc), clo.reshape(n, nc))
            self._uploaded = tab
        return self._session

    def _device_eval(self, t, want):
        hi, lo = split_pairs(t)
        *outs, nunc = self._device().polyco_eval(hi, lo, want)
        if nunc:
            raise ValueError(f"Some input times not covered by Polyco entries. ({nunc} of {hi.size})")
        return outs

    def device_trig(self, t, weights=None, m=20):
        """(2 m + 2,): C_1, S_1, ..., C_m, S_m, sum w, sum w^2 of the polyco phases of the times t, summed on
        the device (pint_polyco_trig): the phases are never read back."""
        hi, lo = split_pairs(t)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != hi.shape:
            raise ValueError(f"weights must have {hi.size} entries, got {w.shape}")
        out, nunc = self._device().polyco_trig(hi, lo, w, m)
        if nunc:
            raise ValueError(f"Some input times not covered by Polyco entries. ({nunc} of {hi.size})")
        return out

    # ---- evaluation ----------------------------------------------------------------------------
    def eval_abs_phase(self, t, device=True):
        """The absolute phase at the times t (float64 or longdouble MJDs) as a Phase, in input order."""
        t = np.atleast_1d(np.asarray(t))
        if device:
            pi, pf, _, _ = self._device_eval(t, 1)
            return Phase(pi.astype(LD), pf.astype(LD))
        idx = self.find_entry(t)
        pi, pf = np.empty(t.shape, dtype=LD), np.empty(t.shape, dtype=LD)
        for i in np.unique(idx):
            sel = idx == i
            p = self.polycoTable[int(i)]["entry"].evalabsphase(t[sel])
            pi[sel], pf[sel] = p.int, p.frac
        return Phase(pi, pf)

    def eval_phase(self, t, device=True):
        """The fractional phase, in [-1/2, 1/2), at the times t."""
        return self.eval_abs_phase(t, device=device).frac

    def eval_spin_freq(self, t, device=True):
        """The spin frequency (Hz) at the times t (longdouble; the device's values are float64)."""
        t = np.atleast_1d(np.asarray(t))
        if device:
            return self._device_eval(t, 2)[2].astype(LD)
        idx = self.find_entry(t)
        return np.array([self.polycoTable[int(i)]["entry"].evalfreq(x) for i, x in zip(idx, t)], dtype=LD)

    def eval_spin_freq_derivative(self, t, device=True):
        """The spin frequency derivative (Hz/s) at the times t."""
        t = np.atleast_1d(np.asarray(t))
        if device:
            return self._device_eval(t, 4)[3].astype(LD)
        idx = self.find_entry(t)
        return np.array([self.polycoTable[int(i)]["entry"].evalfreqderiv(x) for i, x in zip(idx, t)], dtype=LD)

    def htest(self, t, weights=None, m=20, c=4, device=True):
        """(H, Z^2_1..m) of the polyco phases of the times t (weighted with ``weights``): eventstats.hm /
        hmw and z2m / z2mw on the device's trigonometric sums, so the phases are never read back.
        ``device=False`` forms the same sums on the host from eval_phase(device=False)."""
        if device:
            sums = self.device_trig(t, weights, m)
        else:
            ph = np.asarray(self.eval_phase(t, device=False), dtype=np.float64)
            sums = eventstats.trig_sums(ph % 1.0, m, weights)
        if weights is None:
            return eventstats.hm(None, m, c, sums=sums), eventstats.z2m(None, m, sums=sums)
        return eventstats.hmw(None, None, m, c, sums=sums), eventstats.z2mw(None, None, m, sums=sums)
