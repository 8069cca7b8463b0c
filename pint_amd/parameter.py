"""Timing-model parameters and par-file parsing (host side).

Mirrors the behaviour of the reference's parameter classes for the parameters on the hot
path (reference ``src/pint/models/parameter.py``): values keep the precision the reference
keeps -- numpy longdouble for ``long_double=True`` parameters and all MJD parameters
(``parameter.py:1064`` MJDParameter, ``:1143`` time_to_longdouble), float64 otherwise
(``fortran_float``) -- and unit-scaled binary rates follow ``parameter.py:765-800``
(``PBDOT 7.2`` means 7.2e-12 when ``|value| > 1e-7``).

Values are held in the reference's par-file units (``.value``); the device code converts
to SI where it evaluates (``pint_amd/csrc/physics.hpp``).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

LD = np.longdouble


def fortran_float(s: str) -> float:
    """Parse a par-file float allowing Fortran ``D`` exponents (parameter.py fortran_float)."""
    return float(s.replace("D", "E").replace("d", "e"))


def data2longdouble(s: str) -> np.longdouble:
    return np.longdouble(s.replace("D", "E").replace("d", "e"))


def mjd_string_to_longdouble(s: str) -> np.longdouble:
    """MJD string -> longdouble as the reference does it: integer day plus the fractional
    part parsed as float64 (pulsar_mjd.py _str_to_mjds + time_to_longdouble)."""
    s = s.strip().replace("D", "E").replace("d", "e")
    if "e" in s.lower():
        return np.longdouble(s)
    neg = s.startswith("-")
    s = s.lstrip("+-")
    if "." in s:
        ip, fp = s.split(".", 1)
    else:
        ip, fp = s, "0"
    v = np.longdouble(int(ip or "0")) + np.longdouble(float("0." + (fp or "0")))
    return -v if neg else v


def parse_sexagesimal(s: str) -> float:
    """``hh:mm:ss.s`` / ``dd:mm:ss.s`` -> float hours/degrees (astropy hms_to_hours /
    dms_to_degrees: sign * (|h| + m/60 + s/3600))."""
    s = s.strip()
    sign = -1.0 if s.startswith("-") else 1.0
    parts = s.lstrip("+-").split(":")
    h = float(parts[0])
    m = float(parts[1]) if len(parts) > 1 else 0.0
    sec = float(parts[2]) if len(parts) > 2 else 0.0
    return sign * (abs(h) + abs(m) / 60.0 + abs(sec) / 3600.0)


@dataclass
class Param:
    """One timing-model parameter (subset of the reference Parameter API)."""

    name: str
    kind: str = "float"  # float | mjd | hourangle | degangle | str | bool | int | mask | pair
    units: str = ""
    long_double: bool = False
    value: object = None
    frozen: bool = True
    uncertainty_value: Optional[float] = None
    key: Optional[str] = None
    key_value: List[str] = field(default_factory=list)
    index: Optional[int] = None
    scale: Optional[tuple] = None  # (scale_factor, threshold) unit_scale params
    component: str = ""
    description: str = ""
    alias: Optional[str] = None       # the par-file spelling when it was an alias (use_alias)
    mjd_pair: Optional[tuple] = None  # MJDs: the parsed (day, fraction) float64 pair
    implicit: bool = False            # a 0 default standing in for the reference's unset value

    # -- value handling ---------------------------------------------------------------
    def set_from_string(self, s: str):
        k = self.kind
        if k in ("str",):
            self.value = s
        elif k == "bool":
            self.value = s.upper() in ("Y", "YES", "T", "TRUE", "1")
        elif k == "int":
            self.value = int(float(s))
        elif k == "hourangle" or k == "degangle":
            self.value = parse_sexagesimal(s) if ":" in s else fortran_float(s)
        elif k == "mjd":
            from .parfile import str_to_mjds
            self.value = mjd_string_to_longdouble(s)
            self.mjd_pair = str_to_mjds(s)
        else:
            v = data2longdouble(s) if self.long_double else fortran_float(s)
            if self.scale is not None and abs(float(v)) > abs(self.scale[1]):
                v = v * (LD(self.scale[0]) if self.long_double else self.scale[0])
            self.value = v

    def set_pair_from_strings(self, a: str, b: str):
        """A pair parameter's two values (parameter.py:2264-2289 pairParameter: ``NAME v1 v2``, a
        third number on the line is ignored; never free, and no uncertainty)."""
        conv = data2longdouble if self.long_double else fortran_float
        self.value = (conv(a), conv(b))

    def set_uncertainty_from_string(self, s: str):
        try:
            # long-double parameters keep a longdouble uncertainty (parameter.py
            # _set_uncertainty parses it like the value)
            u = data2longdouble(s) if (self.long_double and self.kind in ("float", "mjd")) else fortran_float(s)
        except ValueError:
            return
        if self.kind == "hourangle":  # uncertainty in seconds of time (parameter.py AngleParameter)
            u = u / 3600.0
        elif self.kind == "degangle" and self.name in ("DECJ",):
            u = u / 3600.0
        if self.scale is not None and abs(u) > abs(self.scale[1]):
            u *= self.scale[0]
        self.uncertainty_value = u

    @property
    def quantity(self):
        return self.value

    @property
    def uncertainty(self):
        return self.uncertainty_value

    @uncertainty.setter
    def uncertainty(self, v):
        self.uncertainty_value = None if v is None else float(v)

    # -- prior (parameter.py:376-406) --------------------------------------------------
    @property
    def prior(self):
        """The parameter's prior, a :class:`pint_amd.priors.Prior`; an unbounded uniform one
        (no prior) until one is set."""
        p = self.__dict__.get("_prior")
        if p is None:
            from .priors import Prior, UniformUnboundedRV
            p = self.__dict__["_prior"] = Prior(UniformUnboundedRV())
        return p

    @prior.setter
    def prior(self, p):
        from .priors import Prior
        if not isinstance(p, Prior):
            raise ValueError("prior must be an instance of Prior()")
        self.__dict__["_prior"] = p

    def prior_pdf(self, value=None, logpdf=False):
        """The prior density (or its log) at `value`, a plain number or array in the parameter's
        unit; at the parameter's own value when none is given."""
        value = self.value if value is None else value
        return self.prior.logpdf(value) if logpdf else self.prior.pdf(value)

    def __repr__(self):
        return f"{self.name} ({self.units}) {self.value} frozen={self.frozen}"


class FuncParam(Param):
    """The reference's funcParameter (parameter.py:2390): a value computed from other parameters
    (DDS's SINI, DDH's SINI and M2).  Read-only and always frozen: setting it does nothing, as in the
    reference, and it is never written to a par file; None while an input is unset."""

    def __init__(self, name, units, func, inputs, component="Binary"):
        Param.__init__(self, name=name, kind="func", units=units, component=component)
        object.__setattr__(self, "_func", func)
        object.__setattr__(self, "_inputs", tuple(inputs))

    def __setattr__(self, key, v):
        if key not in ("value", "frozen", "uncertainty_value"):
            object.__setattr__(self, key, v)

    @property
    def value(self):
        args = [p.value for p in self._inputs]
        if any(a is None for a in args):
            return None
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._func(*[np.float64(a) for a in args])

    @property
    def frozen(self):
        return True

    @property
    def uncertainty_value(self):
        return None

    def set_from_string(self, s):
        pass

    def set_uncertainty_from_string(self, s):
        pass


# ---- parameter definitions -----------------------------------------------------------
# name -> (component, kind, units, long_double, scale)
_DEFS = {
    # top level
    "PSR": ("", "str", "", False, None), "EPHEM": ("", "str", "", False, None),
    "CLOCK": ("", "str", "", False, None), "CLK": ("", "str", "", False, None),
    "UNITS": ("", "str", "", False, None), "START": ("", "mjd", "d", True, None),
    "FINISH": ("", "mjd", "d", True, None), "TRACK": ("", "str", "", False, None),
    "BINARY": ("", "str", "", False, None), "NTOA": ("", "int", "", False, None),
    "CHI2": ("", "float", "", False, None), "CHI2R": ("", "float", "", False, None),
    "TRES": ("", "float", "us", False, None), "DMDATA": ("", "bool", "", False, None),
    "DMRES": ("", "float", "pc / cm3", False, None),
    "INFO": ("", "str", "", False, None), "TIMEEPH": ("", "str", "", False, None),
    "T2CMETHOD": ("", "str", "", False, None), "DILATEFREQ": ("", "bool", "", False, None),
    "TZRMJD": ("AbsPhase", "mjd", "d", True, None), "TZRSITE": ("AbsPhase", "str", "", False, None),
    "TZRFRQ": ("AbsPhase", "float", "MHz", False, None),
    # astrometry (astrometry.py)
    "POSEPOCH": ("Astrometry", "mjd", "d", True, None), "PX": ("Astrometry", "float", "mas", False, None),
    "PHOFF": ("PhaseOffset", "float", "", False, None),
    "RAJ": ("AstrometryEquatorial", "hourangle", "hourangle", False, None),
    "DECJ": ("AstrometryEquatorial", "degangle", "deg", False, None),
    "PMRA": ("AstrometryEquatorial", "float", "mas / yr", False, None),
    "PMDEC": ("AstrometryEquatorial", "float", "mas / yr", False, None),
    "ELONG": ("AstrometryEcliptic", "degangle", "deg", False, None),
    "ELAT": ("AstrometryEcliptic", "degangle", "deg", False, None),
    "PMELONG": ("AstrometryEcliptic", "float", "mas / yr", False, None),
    "PMELAT": ("AstrometryEcliptic", "float", "mas / yr", False, None),
    "ECL": ("AstrometryEcliptic", "str", "", False, None),
    # spindown (spindown.py)
    "PEPOCH": ("Spindown", "mjd", "d", True, None),
    # dispersion (dispersion_model.py)
    "DM": ("DispersionDM", "float", "pc / cm3", True, None),
    "DMEPOCH": ("DispersionDM", "mjd", "d", True, None),
    "DMX": ("DispersionDMX", "float", "pc / cm3", False, None),
    # solar system / misc zero components
    "PLANET_SHAPIRO": ("SolarSystemShapiro", "bool", "", False, None),
    "CORRECT_TROPOSPHERE": ("TroposphereDelay", "bool", "", False, None),
    "NE_SW": ("SolarWindDispersion", "float", "1 / cm3", False, None),
    "SWM": ("SolarWindDispersion", "int", "", False, None),
    # WaveX / DMWaveX epochs (wavex.py:51-58, dmwavex.py)
    "WXEPOCH": ("WaveX", "mjd", "d", True, None),
    "DMWXEPOCH": ("DMWaveX", "mjd", "d", True, None),
    # ChromaticCM (chromatic_model.py:128-169) and the CMWaveX epoch (cmwavex.py:34-41)
    "CM": ("ChromaticCM", "float", "pc / (cm3 MHz2)", True, None),
    "CMEPOCH": ("ChromaticCM", "mjd", "d", True, None),
    "TNCHROMIDX": ("ChromaticCM", "float", "", True, None),
    "CMWXEPOCH": ("CMWaveX", "mjd", "d", True, None),
    # FDJump's switch (fdjump.py:69-75): log(f / GHz) (Y) or f / GHz (N) as the polynomial's argument
    "FDJUMPLOG": ("FDJump", "bool", "", False, None),
    # Wave (wave.py:30-58): the epoch and the base angular frequency; IFunc's interpolation type
    # (ifunc.py:59-66, a floatParameter)
    "WAVEEPOCH": ("Wave", "mjd", "d", True, None),
    "WAVE_OM": ("Wave", "float", "1 / d", False, None),
    "SIFUNC": ("IFunc", "float", "", False, None),
    # binaries (pulsar_binary.py, binary_ell1.py, binary_dd.py)
    "PB": ("Binary", "float", "d", True, None),
    "PBDOT": ("Binary", "float", "", False, (1e-12, 1e-7)),
    "XPBDOT": ("Binary", "float", "", False, (1e-12, 1e-7)),
    "A1": ("Binary", "float", "ls", False, None),
    "A1DOT": ("Binary", "float", "ls / s", False, (1e-12, 1e-7)),
    "ECC": ("Binary", "float", "", False, None),
    "EDOT": ("Binary", "float", "1 / s", False, (1e-12, 1e-7)),
    "T0": ("Binary", "mjd", "d", True, None),
    "OM": ("Binary", "float", "deg", True, None),
    "OMDOT": ("Binary", "float", "deg / yr", True, None),
    "M2": ("Binary", "float", "solMass", False, None),
    # ELL1H (binary_ell1.py:345-378): H3/H4 (s) and STIGMA longdouble, NHARMS an int
    "H3": ("Binary", "float", "s", True, None), "H4": ("Binary", "float", "s", True, None),
    "STIGMA": ("Binary", "float", "", True, None), "NHARMS": ("Binary", "int", "", False, None),
    "SINI": ("Binary", "float", "", False, None),
    "GAMMA": ("Binary", "float", "s", False, None),
    "DR": ("Binary", "float", "", False, None), "DTH": ("Binary", "float", "", False, None),
    # DDK (binary_ddk.py:120-145): inclination and node longitude (deg), the K96 flag
    "KIN": ("Binary", "float", "deg", False, None), "KOM": ("Binary", "float", "deg", False, None),
    "K96": ("Binary", "bool", "", False, None),
    "A0": ("Binary", "float", "s", False, None), "B0": ("Binary", "float", "s", False, None),
    # DDS (binary_dd.py:180-188): SINI = 1 - exp(-SHAPMAX); ELL1k (binary_ell1.py:475-483): EDOT / ECC
    "SHAPMAX": ("Binary", "float", "", False, None),
    "LNEDOT": ("Binary", "float", "1 / yr", True, None),
    "TASC": ("Binary", "mjd", "d", True, None),
    "EPS1": ("Binary", "float", "", True, None), "EPS2": ("Binary", "float", "", True, None),
    "EPS1DOT": ("Binary", "float", "1e-12 / s", True, None),
    "EPS2DOT": ("Binary", "float", "1e-12 / s", True, None),
    # red noise (noise_model.py:679-805)
    "TNREDAMP": ("PLRedNoise", "float", "", False, None), "TNREDGAM": ("PLRedNoise", "float", "", False, None),
    "TNREDC": ("PLRedNoise", "float", "", False, None), "RNAMP": ("PLRedNoise", "float", "", False, None),
    "RNIDX": ("PLRedNoise", "float", "", False, None),
    "TNDMAMP": ("PLDMNoise", "float", "", False, None), "TNDMGAM": ("PLDMNoise", "float", "", False, None),
    "TNDMC": ("PLDMNoise", "float", "", False, None),
}

_ALIASES = {
    "RA": "RAJ", "DEC": "DECJ", "LAMBDA": "ELONG", "BETA": "ELAT", "PMLAMBDA": "PMELONG",
    "PMBETA": "PMELAT", "E": "ECC", "ECCDOT": "EDOT", "XDOT": "A1DOT", "T2EFAC": "EFAC",
    "T2EQUAD": "EQUAD", "TNECORR": "ECORR", "SOLARN0": "NE_SW", "NE1AU": "NE_SW", "CLK": "CLOCK", "PSRJ": "PSR", "PSRB": "PSR", "VARSIGMA": "STIGMA", "STIG": "STIGMA",
    "FB": "FB0",
}

_PREFIX = {  # prefix params: regex -> (component, units template, long_double)
    r"^F(\d+)$": ("Spindown", "Hz / s^{n}", True),
    r"^DM(\d+)$": ("DispersionDM", "pc / (cm3 yr^{n})", True),
    r"^DMX_(\d+)$": ("DispersionDMX", "pc / cm3", False),
    r"^DMXR1_(\d+)$": ("DispersionDMX", "d", True),
    r"^DMXR2_(\d+)$": ("DispersionDMX", "d", True),
    r"^FD(\d+)$": ("FD", "s", False),
    # the orbital frequency and its derivatives (pulsar_binary.py:192-205): longdouble, 1 / s^(n+1)
    r"^FB(\d+)$": ("Binary", "1 / s^{n+1}", True),
    # Glitch (glitch.py:56-124): the epoch an MJD, the rest float64 in the reference's units
    r"^GLEP_(\d+)$": ("Glitch", "d", True),
    r"^GLPH_(\d+)$": ("Glitch", "pulse phase", False),
    r"^GLF0_(\d+)$": ("Glitch", "Hz", False),
    r"^GLF1_(\d+)$": ("Glitch", "Hz / s", False),
    r"^GLF2_(\d+)$": ("Glitch", "Hz / s2", False),
    r"^GLF0D_(\d+)$": ("Glitch", "Hz", False),
    r"^GLTD_(\d+)$": ("Glitch", "d", False),
    # WaveX (wavex.py:105-136) and DMWaveX (dmwavex.py): float64; only the four-digit index is a
    # par-file name (the reference does not recognise WXSIN_1)
    r"^WXFREQ_(\d{4})$": ("WaveX", "1 / d", False),
    r"^WXSIN_(\d{4})$": ("WaveX", "s", False),
    r"^WXCOS_(\d{4})$": ("WaveX", "s", False),
    r"^DMWXFREQ_(\d{4})$": ("DMWaveX", "1 / d", False),
    r"^DMWXSIN_(\d{4})$": ("DMWaveX", "pc / cm3", False),
    r"^DMWXCOS_(\d{4})$": ("DMWaveX", "pc / cm3", False),
    # ChromaticCM's Taylor terms (longdouble, per yr^n) and CMWaveX (cmwavex.py:91-136)
    r"^CM(\d+)$": ("ChromaticCM", "pc / (cm3 MHz2 yr^{n})", True),
    r"^CMWXFREQ_(\d{4})$": ("CMWaveX", "1 / d", False),
    r"^CMWXSIN_(\d{4})$": ("CMWaveX", "pc / (cm3 MHz2)", False),
    r"^CMWXCOS_(\d{4})$": ("CMWaveX", "pc / (cm3 MHz2)", False),
    # Wave's terms (sine and cosine amplitude, s) and IFunc's control points (MJD, s): pair
    # parameters, longdouble (wave.py:48-58, ifunc.py:67-77)
    r"^WAVE(\d+)$": ("Wave", "s", True),
    r"^IFUNC(\d+)$": ("IFunc", "s", True),
    # PiecewiseSpindown (piecewise.py:54-123): three epochs (MJD) and four float64 spin terms per piece
    r"^PWSTART_(\d+)$": ("PiecewiseSpindown", "d", True),
    r"^PWSTOP_(\d+)$": ("PiecewiseSpindown", "d", True),
    r"^PWEP_(\d+)$": ("PiecewiseSpindown", "d", True),
    r"^PWPH_(\d+)$": ("PiecewiseSpindown", "", False),
    r"^PWF0_(\d+)$": ("PiecewiseSpindown", "Hz", False),
    r"^PWF1_(\d+)$": ("PiecewiseSpindown", "Hz / s", False),
    r"^PWF2_(\d+)$": ("PiecewiseSpindown", "Hz / s2", False),
}
PAIR_NAME = re.compile(r"^(WAVE|IFUNC)\d+$")
MJD_PREFIXES = ("DMXR", "GLEP_", "PWSTART_", "PWSTOP_", "PWEP_")

MASK_PARAMS = {"JUMP": ("PhaseJump", "s"), "EFAC": ("ScaleToaError", ""),
               "EQUAD": ("ScaleToaError", "us"), "TNEQ": ("ScaleToaError", "log10(s)"),
               "ECORR": ("EcorrNoise", "us"),
               # wideband DM data (dispersion_model.py:724 DispersionJump; noise_model.py:228
               # ScaleDmError): DM offsets and DM-error scaling, pc/cm^3
               "DMJUMP": ("DispersionJump", "pc / cm3"), "DMEFAC": ("ScaleDmError", ""),
               "DMEQUAD": ("ScaleDmError", "pc / cm3")}

# FDJump (fdjump.py:76-84): mask parameters FD{p}JUMP{q}, p = the FD index 1..fdjump_max_index, q
# the mask index; the base name of a par line is FD{p}JUMP (tempo2's FDJUMP{p} is the same
# parameter, model_builder._replace_fdjump_in_parfile_dict).  FDJumpDM (dispersion_model.py:805-
# 884): FDJUMPDM{q}, a DM offset of -value on the selected TOAs
FDJUMP_MAX_INDEX = 20
MASK_PARAMS.update({f"FD{_j}JUMP": ("FDJump", "s") for _j in range(1, FDJUMP_MAX_INDEX + 1)})
MASK_PARAMS["FDJUMPDM"] = ("FDJumpDM", "pc / cm3")
FDJUMP_NAME = re.compile(r"^FD(\d+)JUMP(\d+)$")


def fdjump_base(name: str) -> Optional[str]:
    """The base name FD{p}JUMP of a par-file line spelt FD{p}JUMP or FDJUMP{p} (None: neither)."""
    if re.match(r"^FD\d+JUMP$", name):
        return name
    m = re.match(r"^FDJUMP(\d+)$", name)
    return f"FD{int(m.group(1))}JUMP" if m else None


IGNORED = {"MODE", "NITS", "IBOOT", "RM", "SWP", "DMXEP", "DMXF1", "DMXF2"}


def make_param(name: str) -> Optional[Param]:
    if name in _DEFS:
        comp, kind, units, ld, scale = _DEFS[name]
        return Param(name=name, kind=kind, units=units, long_double=ld, scale=scale, component=comp)
    for rx, (comp, units, ld) in _PREFIX.items():
        m = re.match(rx, name)
        if m:
            idx = int(m.group(1))
            kind = "mjd" if name.startswith(MJD_PREFIXES) else ("pair" if PAIR_NAME.match(name) else "float")
            u = units.replace("{n+1}", str(idx + 1)).replace("{n}", str(idx))
            if name == "F0":
                u = "Hz"
            if name.startswith(("DM", "CM")) and not name.startswith(("DMX", "DMWX", "CMWX")) and idx == 0:
                return None
            return Param(name=name, kind=kind, units=u, long_double=ld, component=comp, index=idx)
    return None


@dataclass
class ParLine:
    name: str
    fields: List[str]


def read_parfile(path_or_text) -> List[ParLine]:
    """Tokenise a par file (model_builder.py:102-250 parse semantics: '#' / 'C ' comments)."""
    if hasattr(path_or_text, "read"):
        text = path_or_text.read()
    elif "\n" in str(path_or_text):
        text = str(path_or_text)
    else:
        with open(path_or_text) as f:
            text = f.read()
    out = []
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line.startswith("#") or line.startswith("C ") or line == "C":
            continue
        toks = line.split()
        out.append(ParLine(toks[0].upper() if not toks[0].startswith("TN") else toks[0].upper(), toks[1:]))
    return out
