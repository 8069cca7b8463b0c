"""TimingModel host mirror: par file -> components/parameters -> device spec + table.

Reference API kept: ``get_model`` (model_builder.py:777), ``TimingModel`` attribute access
to parameters (``model.F0.value``), ``params``/``free_params`` (timing_model.py:614/655),
``components``, ``has_correlated_errors``, ``designmatrix`` (:2073), ``delay`` (:1515),
``phase`` (:1548), ``scaled_toa_uncertainty`` (:1644), ``noise_model_designmatrix`` /
``noise_model_basis_weight`` (:1704-1716).  Evaluation runs on the GPU through
``pint_amd.engine``; this module only builds the structure and parameter tables.
"""
from __future__ import annotations

import copy
import re
from collections import OrderedDict
from typing import Dict, List, Optional

import numpy as np

from . import parameter as P
from .parameter import LD, Param

# components supported on the hot path
DELAY_ORDER = ["AstrometryEquatorial", "AstrometryEcliptic", "TroposphereDelay", "SolarSystemShapiro",
               "SolarWindDispersion", "DispersionDM", "DispersionDMX", "BinaryELL1", "BinaryDD", "FD", "WaveX",
               "DMWaveX", "ChromaticCM", "CMWaveX", "FDJump", "FDJumpDM"]
PHASE_ORDER = ["AbsPhase", "Spindown", "Wave", "Glitch", "PiecewiseSpindown", "IFunc", "PhaseOffset", "PhaseJump"]
NOISE = ["ScaleToaError", "EcorrNoise", "PLRedNoise", "PLDMNoise"]

# Glitch (glitch.py): the parameters of one glitch in the order setup / print_par walk them
# (glitch_prop, :130-138), which is also the order of a glitch's 7 table slots and of
# PINT_GL_*; and the order the component declares its index-1 parameters in (:56-124)
GLITCH_PROPS = ("GLEP_", "GLPH_", "GLF0_", "GLF1_", "GLF2_", "GLF0D_", "GLTD_")
GLITCH_DECLARED = ("GLPH_", "GLEP_", "GLF0_", "GLF1_", "GLF2_", "GLF0D_", "GLTD_")

# PiecewiseSpindown (piecewise.py): the parameters of one piece in the order setup / print_par walk
# them (pwsol_prop, :130-138), which is also the order of a piece's 7 table slots and of PINT_PW_*;
# and the order the component declares its index-1 parameters in (:54-123).  Wave (category wave)
# is in the reference's DEFAULT_ORDER, after phase_jump; piecewise and ifunc are not, like glitch,
# so their place among the phase components changes with the interpreter's hash seed.  Here the
# order is always Spindown, Wave, Glitch, PiecewiseSpindown, IFunc (the order of the run the
# pw_wls / wave_wls fixtures were captured in).
PW_PROPS = ("PWEP_", "PWSTART_", "PWSTOP_", "PWPH_", "PWF0_", "PWF1_", "PWF2_")
PW_DECLARED = ("PWSTART_", "PWSTOP_", "PWEP_", "PWPH_", "PWF0_", "PWF1_", "PWF2_")
PW_FITTABLE = ("PWPH_", "PWF0_", "PWF1_", "PWF2_")

# WaveX / DMWaveX (wavex.py, dmwavex.py): component -> parameter-name stem.  wavex is the last
# category of the reference's DEFAULT_ORDER and dmwavex is not in it (it sorts after everything,
# timing_model.py:1296): both delays follow the binary's, and their parameters follow its.
# ChromaticCM (category chromatic_constant) and CMWaveX (cmwavex) are not in DEFAULT_ORDER either: in
# the reference DMWaveX, ChromaticCM and CMWaveX follow everything else in the order its model
# builder adds them (a set's iteration order: it changes with the hash seed).  Here the order is
# always ... binary, WaveX, DMWaveX, ChromaticCM, CMWaveX, for the delays and for the parameters.
# FDJump (category fdjump) and FDJumpDM (fdjumpdm) are not in DEFAULT_ORDER either and follow in the
# same seed-dependent way; here always ... CMWaveX, FDJump, FDJumpDM.
WAVEX_STEMS = {"WaveX": "WX", "DMWaveX": "DMWX", "CMWaveX": "CMWX"}

ELL1_PARAMS = ["PB", "PBDOT", "A1", "A1DOT", "EDOT", "OMDOT", "M2", "SINI", "TASC", "EPS1", "EPS2",
               "EPS1DOT", "EPS2DOT"]
DD_PARAMS = ["PB", "PBDOT", "A1", "A1DOT", "ECC", "EDOT", "T0", "OM", "OMDOT", "M2", "SINI", "A0", "B0",
             "GAMMA", "DR", "DTH"]
DDK_PARAMS = [n for n in DD_PARAMS if n != "SINI"] + ["KIN", "KOM"]  # binary_ddk.py:120-145
# DDS (binary_dd.py:173-198): DD with SHAPMAX in place of SINI, which stays readable as a derived
# parameter; DDH (:409-452): H3 and STIGMA in place of M2 and SINI, both derived; ELL1k
# (binary_ell1.py:455-483): ELL1 less EDOT / EPS1DOT / EPS2DOT, OMDOT re-declared after EPS2, LNEDOT.
# Each in the order the reference's component holds its parameters.
DDS_PARAMS = [n for n in DD_PARAMS if n != "SINI"] + ["SHAPMAX", "SINI"]
DDH_PARAMS = [n for n in DD_PARAMS if n not in ("M2", "SINI")] + ["H3", "STIGMA", "SINI", "M2"]
ELL1K_PARAMS = ["PB", "PBDOT", "A1", "A1DOT", "M2", "SINI", "TASC", "EPS1", "EPS2", "OMDOT", "LNEDOT"]
ELL1K_REMOVED = ("EPS1DOT", "EPS2DOT", "EDOT")
BINARIES = ("ELL1", "DD", "ELL1H", "BT", "DDK", "DDS", "DDH", "ELL1k")
# the models whose orbit may be given by FB0 ... FBn (OrbitFBX, binary_orbits.py:158-239); the other
# four are variants of the same two device bodies and would each add two evaluation builds
FBX_BINARIES = ("ELL1", "ELL1H", "DD", "BT")
FB_NAME = re.compile(r"^FB(\d+)$")
BT_PARAMS = ["PB", "PBDOT", "A1", "A1DOT", "ECC", "EDOT", "T0", "OM", "OMDOT", "GAMMA"]
BIN_IDS = {"PB": 0, "PBDOT": 1, "XPBDOT": 2, "A1": 3, "A1DOT": 4, "ECC": 5, "EDOT": 6, "T0": 7, "OM": 8,
           "OMDOT": 9, "M2": 10, "SINI": 11, "GAMMA": 12, "DR": 13, "DTH": 14, "A0": 15, "B0": 16,
           "TASC": 17, "EPS1": 18, "EPS2": 19, "EPS1DOT": 20, "EPS2DOT": 21, "H3": 22, "H4": 23, "STIGMA": 24,
           "KIN": 25, "KOM": 26, "SHAPMAX": 27, "LNEDOT": 28}
# obliquity values (rad) from the reference's runtime ecliptic.dat (pulsar_ecliptic.py:29)
OBLIQUITY = {"IERS2010": 0.4090926006005829, "IERS2003": 0.40909260011576914,
             "DEFAULT": 84381.406 / 206264.80624709636}


class MissingParameter(ValueError):
    pass


class TimingModelError(ValueError):
    """timing_model.py TimingModelError (an invalid model structure)."""


class UnknownParameter(TimingModelError):
    """timing_model.py UnknownParameter (a name no component of the model declares)."""


class UnknownBinaryModel(TimingModelError):
    """timing_model.py UnknownBinaryModel (a BINARY line that names no model)."""


def _sini_from_shapmax(shapmax):
    """binary_dd.py:18 (DDS)."""
    return 1.0 - np.exp(-shapmax)


def _sini_from_stigma(stigma):
    """binary_dd.py:30 (DDH, Freire & Wex 2010 Eq. 12)."""
    return 2.0 * stigma / (1.0 + stigma ** 2)


def _m2_from_h3_stigma(h3, stigma):
    """binary_dd.py:26 (DDH): H3 / STIGMA^3 / T_sun, in solar masses."""
    return h3 / stigma ** 3 / TSUN_S


TSUN_S = 4.92549094830932e-06  # G M_sun / c^3 (s), the reference's Tsun (pint/__init__.py:80)


class TimingModel:
    """Host-side model: ordered parameters grouped by component."""

    def __init__(self, name: str = ""):
        object.__setattr__(self, "_params", OrderedDict())
        self.name = name
        self.components: "OrderedDict[str, list]" = OrderedDict()
        self.binary: Optional[str] = None

    # -- parameter access -------------------------------------------------------------
    def __getattr__(self, name):
        params = object.__getattribute__(self, "_params")
        if name in params:
            return params[name]
        raise AttributeError(name)

    def __getitem__(self, name):
        return self._params[name]

    def __contains__(self, name):
        return name in self._params

    def add_param(self, p: Param):
        self._params[p.name] = p
        self.components.setdefault(p.component or "TimingModel", []).append(p.name)
        object.__setattr__(self, "_order", None)
        object.__setattr__(self, "_names", {})

    def remove_param(self, name: str):
        """Component.remove_param (timing_model.py): the caches keyed on the parameter count go too."""
        p = self._params.pop(name)
        self.components[p.component or "TimingModel"].remove(name)
        object.__setattr__(self, "_order", None)
        object.__setattr__(self, "_names", {})

    @property
    def params(self) -> List[str]:
        """Parameter order: top level, astrometry, spindown, remaining components
        (timing_model.py:614-652).  Cached until the next add_param (the fitters ask for
        it, and for free_params, several times per fit)."""
        cached = self.__dict__.get("_order")
        if cached is not None and cached[0] == len(self._params):
            return list(cached[1])
        order = self._params_order()
        object.__setattr__(self, "_order", (len(self._params), tuple(order)))
        return order

    def _params_order(self) -> List[str]:
        # one stable sort by group rank (dict order within a group): top level, astrometry,
        # spindown, the delay/phase/noise components in order, the rest
        order = [("Binary" if c.startswith("Binary") else c) for c in DELAY_ORDER]
        # DispersionJump (dispersion_jump) precedes the binary (pulsar_system) in the reference's
        # DEFAULT_ORDER (timing_model.py:107-123), which orders its delay components' parameters
        order.insert(order.index("Binary"), "DispersionJump")
        rest = {}
        for comp in dict.fromkeys(order + ["AbsPhase", "PhaseJump"] + NOISE):
            if not comp.startswith("Astrometry"):
                rest.setdefault(comp, 4 + len(rest))
        big = 4 + len(rest)

        def rank(c):
            if c in ("", "TimingModel"):
                return 0
            if c.startswith("Astrometry"):
                return 1
            if c == "Spindown":
                return 2
            if c == "Wave":  # the phase components: after Spindown, before the delay components
                return 2.5
            if c == "Glitch":
                return 3
            if c in ("PiecewiseSpindown", "IFunc"):
                return 3.2 if c == "PiecewiseSpindown" else 3.3
            return rest.get(c, big)
        ranks = {c: rank(c) for c in {p.component for p in self._params.values()}}
        if "Glitch" not in ranks:
            return sorted(self._params, key=lambda n: ranks[self._params[n].component])

        # Glitch's own order (glitch.py:56-153): the index-1 parameters in the order the component
        # declares them, the other indices in par-file order, then the ones setup filled in
        # (get_model adds those last)
        def key(n):
            p = self._params[n]
            sub = len(GLITCH_DECLARED)
            if p.component == "Glitch" and p.index == 1:
                sub = GLITCH_DECLARED.index(n[:n.index("_") + 1])
            return ranks[p.component], sub
        return sorted(self._params, key=key)

    def as_parfile(self, include_info: bool = True, comment: str = None) -> str:
        """The model as par-file text (timing_model.py:2747 as_parfile, format "pint")."""
        from .parfile import as_parfile
        return as_parfile(self, include_info=include_info, comment=comment)

    def write_parfile(self, filename, include_info: bool = True, comment: str = None):
        """timing_model.py:2823 write_parfile."""
        from .parfile import write_parfile
        write_parfile(self, filename, include_info=include_info, comment=comment)

    @property
    def free_params(self) -> List[str]:
        return [p for p in self.params if not self._params[p].frozen]

    @free_params.setter
    def free_params(self, names):
        want = set(names)
        for n, p in self._params.items():
            p.frozen = n not in want
            want.discard(n)
        if want:
            raise ValueError(f"Parameter(s) not in the model: {sorted(want)}")

    def set_param_values(self, fitp):
        """Set the values of the named parameters (timing_model.py set_param_values): {name: value}.
        Long-double and MJD parameters keep a longdouble (a float lands in it exactly), the others a
        float, as the par-file parser leaves them."""
        for name, v in fitp.items():
            p = self._params[name]
            if p.kind in ("float", "mjd", "hourangle", "degangle", "mask"):
                p.value = LD(v) if (p.long_double or p.kind == "mjd") else float(v)
            else:
                p.value = v

    def get_params_dict(self, which="free", kind="value"):
        names = self.free_params if which == "free" else self.params
        return OrderedDict((n, self._params[n].value) for n in names)

    # -- component queries ------------------------------------------------------------
    @property
    def component_names(self) -> List[str]:
        return [c for c in DELAY_ORDER + PHASE_ORDER + NOISE if c in self.components]

    @property
    def has_correlated_errors(self) -> bool:
        return any(c in self.components for c in ("PLRedNoise", "PLDMNoise", "EcorrNoise"))

    @property
    def has_time_correlated_errors(self) -> bool:
        return "PLRedNoise" in self.components or "PLDMNoise" in self.components

    @property
    def astrometry_kind(self) -> int:
        if "AstrometryEquatorial" in self.components:
            return 1
        if "AstrometryEcliptic" in self.components:
            return 2
        return 0

    @property
    def has_solar_wind(self) -> bool:
        """SolarWindDispersion with something to evaluate: NE_SW free or non-zero (the
        reference's delay and DM are zeros when NE_SW == 0, solar_wind_dispersion.py:378-392)."""
        return "NE_SW" in self._params and (not self.NE_SW.frozen or bool(self.NE_SW.value))

    def _names_of(self, key, build):
        """Name lists derived from the parameter set alone, cached until the next add_param
        (parameters are never removed): build_layout / validate ask for them many times per
        upload, and a regex pass over ~250 parameters each time dominated the host layout."""
        cache = self.__dict__.get("_names")
        if cache is None or cache.get("_n") != len(self._params):  # (a shallow copy shares _params)
            cache = {"_n": len(self._params)}
            object.__setattr__(self, "_names", cache)
        hit = cache.get(key)
        if hit is None:
            hit = cache[key] = tuple(build())
        return list(hit)

    def prefix_list(self, prefix_rx: str) -> List[str]:
        def build():
            rx = re.compile(prefix_rx)
            out = []
            for n in self._params:
                m = rx.match(n)
                if m:
                    out.append((int(m.group(1)), n))
            return [n for _, n in sorted(out)]
        return self._names_of(("prefix", prefix_rx), build)

    def spin_terms(self) -> List[str]:
        return self.prefix_list(r"^F(\d+)$")

    def dm_terms(self) -> List[str]:
        return ["DM"] + self.prefix_list(r"^DM(\d+)$") if "DM" in self._params else []

    def dmx_params(self) -> List[str]:
        return self.prefix_list(r"^DMX_(\d+)$")

    def fb_terms(self) -> List[str]:
        """FB0, FB1, ... in ascending index: the FBn parameters the model carries ([] for the
        period form; they exist only when the par file names one)."""
        return self.prefix_list(r"^FB(\d+)$")

    def pb(self):
        """PulsarBinary.pb at the reference epoch (pulsar_binary.py:566-625): the binary period and
        its uncertainty in days, from PB, or from 1 / FB0 (the uncertainty to first order,
        sigma_FB0 / FB0^2) when the orbit is given by FBn; the uncertainty is None when it is unset
        or zero."""
        if not self.binary:
            raise AttributeError("the model has no binary component")
        if "PB" in self._params and self.PB.value is not None:
            s = self.PB.uncertainty_value
            return LD(self.PB.value), (float(s) if s else None)
        if "FB0" in self._params and self.FB0.value is not None:
            f = LD(self.FB0.value)
            s = self.FB0.uncertainty_value
            return 1 / f / LD(86400), (float(LD(s) / f / f / LD(86400)) if s else None)
        raise AttributeError("Neither PB nor FB0 is present in the timing model.")

    def fd_terms(self) -> List[str]:
        return self.prefix_list(r"^FD(\d+)$")

    def cm_terms(self) -> List[str]:
        """ChromaticCM's Taylor terms CM, CM1, ... in ascending order ([] without the component)."""
        return ["CM"] + self.prefix_list(r"^CM(\d+)$") if "CM" in self._params else []

    def get_CM_terms(self):
        """ChromaticCM.get_CM_terms (chromatic_model.py:207-209): the values [CM, CM1, ..., CMn]."""
        return [self._params[n].value for n in self.cm_terms()]

    def change_cmepoch(self, new_epoch):
        """ChromaticCM.change_cmepoch (chromatic_model.py:272-302): move CMEPOCH to `new_epoch`
        (MJD, TDB) and the Taylor terms with it, CM_n <- sum_{k>=n} CM_k dt^(k-n) / (k-n)!, dt in
        years (taylor_horner_deriv, in longdouble)."""
        new_epoch = LD(new_epoch)
        names = self.cm_terms()
        terms = [LD(0) if self._params[n].value is None else LD(self._params[n].value) for n in names]
        if self.CMEPOCH.value is None:
            if any(t != 0 for t in terms[1:]):
                raise ValueError(f"CMEPOCH not set but some CM derivatives are not zero: {terms}")
            self.CMEPOCH.value = new_epoch
        dt = (new_epoch - LD(self.CMEPOCH.value)) / LD(365.25)
        for n, name in enumerate(names):
            # taylor_horner_deriv(dt, [0, CM, CM1, ...], n + 1): Horner from the highest term down
            der = terms[n:]
            r, fact = LD(0), LD(len(der))
            for c in der[::-1]:
                r = r * dt / fact + c
                fact -= 1
            self._params[name].value = r
        self.CMEPOCH.value = new_epoch

    def add_cmwavex_component(self, cmwxfreq, index=None, cmwxsin=0, cmwxcos=0, frozen=True):
        """CMWaveX.add_cmwavex_component (cmwavex.py:47-138)."""
        return self.add_wavex_component(cmwxfreq, index, cmwxsin, cmwxcos, frozen, component="CMWaveX")

    def add_cmwavex_components(self, cmwxfreqs, indices=None, cmwxsins=0, cmwxcoses=0, frozens=True):
        """CMWaveX.add_cmwavex_components (cmwavex.py:140-252)."""
        return self.add_wavex_components(cmwxfreqs, indices, cmwxsins, cmwxcoses, frozens, component="CMWaveX")

    def remove_cmwavex_component(self, index):
        """CMWaveX.remove_cmwavex_component (cmwavex.py:254-276)."""
        self.remove_wavex_component(index, component="CMWaveX")

    def fdjump_params(self) -> List[str]:
        """FDJump's mask parameters FD{p}JUMP{q} in parameter order (fdjump.py:91-95 fdjumps, the
        unset ones the reference's constructor declares left out)."""
        return self._names_of("fdjump", lambda: [n for n, p in self._params.items()
                                                 if p.kind == "mask" and p.component == "FDJump"])

    def fdjumpdm_params(self) -> List[str]:
        """FDJumpDM's mask parameters FDJUMPDM{q} in parameter order (dispersion_model.py:848-851)."""
        return self.mask_params("FDJUMPDM")

    @staticmethod
    def get_fd_index(par: str) -> int:
        """FDJump.get_fd_index (fdjump.py:103-120): p of FD{p}JUMP{q}."""
        m = P.FDJUMP_NAME.match(par)
        if not m:
            raise ValueError(f"The given parameter {par} does not correspond to an FDJUMP.")
        return int(m.group(1))

    def glitch_indices(self) -> List[int]:
        """The glitch indices that appear in any GL*_n parameter, ascending (glitch.py:139-145)."""
        return self._names_of("glitch", lambda: sorted({p.index for p in self._params.values()
                                                        if p.component == "Glitch"}))

    def setup_glitches(self):
        """Glitch.setup (glitch.py:127-153): every glitch index that appears gets all seven
        parameters, the missing ones 0 and frozen.  A missing epoch stays missing (validate)."""
        for idx in self.glitch_indices():
            for pre in GLITCH_PROPS:
                if pre != "GLEP_" and f"{pre}{idx}" not in self._params:
                    p = P.make_param(f"{pre}{idx}")
                    p.value = 0.0
                    self.add_param(p)

    # -- PiecewiseSpindown, Wave, IFunc (piecewise.py, wave.py, ifunc.py) -------------------------
    def pw_indices(self) -> List[int]:
        """The piece indices that appear in any PW*_n parameter, ascending (piecewise.py:139-144)."""
        return self._names_of("pw", lambda: sorted({p.index for p in self._params.values()
                                                    if p.component == "PiecewiseSpindown"}))

    def wave_terms(self) -> List[str]:
        """WAVE1, WAVE2, ... in ascending index (the terms that have a value)."""
        return [n for n in self.prefix_list(r"^WAVE(\d+)$") if self._params[n].value is not None]

    def ifunc_terms(self) -> List[str]:
        """IFUNC1, IFUNC2, ... in ascending index (the control points that have a value)."""
        return [n for n in self.prefix_list(r"^IFUNC(\d+)$") if self._params[n].value is not None]

    def validate_phase_terms(self):
        """PiecewiseSpindown.setup / validate (piecewise.py:128-171), Wave.validate (wave.py:66-87)
        and IFunc.validate (ifunc.py:85-102)."""
        pieces = self.pw_indices()
        for idx in pieces:  # (setup: register_deriv_funcs on a parameter the piece does not have)
            for pre in PW_FITTABLE:
                if f"{pre}{idx}" not in self._params:
                    raise UnknownParameter(f"Unknown parameter name or alias {pre}{idx}")
        for idx in pieces:
            # (the reference's index-1 epochs always exist, unset, and fail at the first evaluation;
            # here an unset epoch is as missing as an absent one)
            for pre, what in (("PWEP_", "Epoch"), ("PWSTART_", "starting epoch"), ("PWSTOP_", "end epoch")):
                p = self._params.get(f"{pre}{idx}")
                if p is None or p.value is None:
                    raise MissingParameter(f"PiecewiseSpindown.{pre}{idx} Piecewise solution {what} is needed "
                                           f"for Piece {idx}.")
        if "Wave" in self.components:
            if self.WAVEEPOCH.value is None:
                if "PEPOCH" not in self._params or self.PEPOCH.value is None:
                    raise MissingParameter("Wave.WAVEEPOCH WAVEEPOCH or PEPOCH are required if WAVE_OM is set.")
                self.WAVEEPOCH.value = LD(self.PEPOCH.value)
            terms = [self._params[n].index for n in self.wave_terms()]
            for k in range(1, max(terms, default=0) + 1):
                if k not in terms:
                    raise MissingParameter(f"Wave.WAVE{k}")
            if terms and self.WAVE_OM.value is None:
                # (the reference loads such a model and fails when the phase is first evaluated)
                raise MissingParameter("Wave.WAVE_OM WAVE_OM is required if WAVE entries are present.")
        if "IFunc" in self.components:
            if self.SIFUNC.value is None:
                raise MissingParameter("IFunc.SIFUNC SIFUNC is required if IFUNC entries are present.")
            for i, n in enumerate(self.ifunc_terms()):
                if self._params[n].index != i + 1:
                    raise MissingParameter(f"IFunc.IFUNC{i + 1}")
        if sum(c in self.components for c in ("Wave", "WaveX", "PLRedNoise", "IFunc")) > 1:
            # (TimingModel.validate, timing_model.py: logged, not raised)
            import logging
            logging.getLogger("pint_amd").warning("Wave, WaveX, and PLRedNoise cannot be used together. They are "
                                                  "ways of modelling the same effect.")

    # -- WaveX / DMWaveX (wavex.py:63-289, dmwavex.py) ------------------------------------------
    def _wavex_map(self, comp: str, part: str) -> Dict[int, str]:
        """get_prefix_mapping_component(f"{stem}{part}_"): {index: name} in parameter order."""
        pre = f"{WAVEX_STEMS[comp]}{part}_"
        return {p.index: n for n, p in self._params.items() if p.component == comp and n.startswith(pre)}

    def wavex_indices(self, comp: str = "WaveX") -> List[int]:
        """The component's harmonic indices, ascending: the order of its table block and of
        col_index."""
        return sorted(self._wavex_map(comp, "FREQ")) if comp in self.components else []

    def get_wavex_indices(self, component: str = "WaveX"):
        """WaveX.get_indices (wavex.py:279-289): the indices of the FREQ parameters, in
        parameter order."""
        return np.array(list(self._wavex_map(component, "FREQ")), dtype=int)

    def _ensure_wavex(self, comp: str):
        """The component as its constructor leaves it (wavex.py:49-60): the epoch unset, and
        harmonic 0001 at 0.1 / d with zero, *free* amplitudes."""
        stem = WAVEX_STEMS[comp]
        for name, value, frozen in ((f"{stem}EPOCH", None, True), (f"{stem}FREQ_0001", 0.1, True),
                                    (f"{stem}SIN_0001", 0.0, False), (f"{stem}COS_0001", 0.0, False)):
            if name not in self._params:
                p = P.make_param(name)
                p.value, p.frozen = value, frozen
                self.add_param(p)

    def add_wavex_component(self, wxfreq, index=None, wxsin=0, wxcos=0, frozen=True, component="WaveX"):
        """WaveX.add_wavex_component (wavex.py:63-139); returns the index given to the harmonic."""
        return self.add_wavex_components([wxfreq], None if index is None else [index], wxsin, wxcos, frozen,
                                         component=component)[0]

    def add_wavex_components(self, wxfreqs, indices=None, wxsins=0, wxcoses=0, frozens=True, component="WaveX"):
        """WaveX.add_wavex_components (wavex.py:141-253): harmonics at the given frequencies
        (1 / d), amplitudes in s (pc / cm3 for DMWaveX); an index of None takes the largest
        index in use plus one.  Returns the indices."""
        stem = WAVEX_STEMS[component]
        wxfreqs = [float(f) for f in np.atleast_1d(np.asarray(wxfreqs, dtype=np.float64))]
        n = len(wxfreqs)
        indices = [None] * n if indices is None else list(indices)
        cols = []
        for vals, what in ((wxsins, "sine ampltudes"), (wxcoses, "cosine ampltudes")):
            vals = np.atleast_1d(vals)
            if len(vals) == 1:
                vals = np.repeat(vals, n)
            if len(vals) != n:
                raise ValueError(f"Number of base frequencies {n} doesn't match number of {what} {len(vals)}")
            cols.append(vals)
        frozens = np.atleast_1d(frozens)
        if len(frozens) == 1:
            frozens = np.repeat(frozens, n)
        if len(frozens) != n:
            raise ValueError("Number of base frequencies must match number of frozen values")
        self._ensure_wavex(component)
        used = self._wavex_map(component, "FREQ")
        last = max(used)
        added = []
        for f, index, s_, c_, fr in zip(wxfreqs, indices, cols[0], cols[1], frozens):
            if index is None:
                index = last = last + 1
            elif int(index) in used or int(index) in added:
                raise ValueError(f"Index '{index}' is already in use in this model. Please choose another")
            added.append(int(index))
            for part, v, frz in (("FREQ", f, True), ("SIN", float(s_), bool(fr)), ("COS", float(c_), bool(fr))):
                p = P.make_param(f"{stem}{part}_{int(index):04d}")
                p.value, p.frozen = v, frz
                self.add_param(p)
        self.validate_wavex(component)
        return added

    def remove_wavex_component(self, index, component="WaveX"):
        """WaveX.remove_wavex_component (wavex.py:255-277): an index or a list of indices."""
        if isinstance(index, (int, float, np.integer)):
            index = [index]
        elif not isinstance(index, (list, set, np.ndarray)):
            raise TypeError(f"index most be a float, int, set, list, or array - not {type(index)}")
        stem = WAVEX_STEMS[component]
        for i in index:
            for part in ("FREQ", "SIN", "COS"):
                self.remove_param(f"{stem}{part}_{int(i):04d}")
        self.validate_wavex(component)

    def validate_wavex(self, comp: str):
        """WaveX.validate / DMWaveX.validate (wavex.py:303-360, dmwavex.py:293-350)."""
        import warnings
        if comp not in self.components:
            return
        stem = WAVEX_STEMS[comp]
        fm, sm, cm = (self._wavex_map(comp, part) for part in ("FREQ", "SIN", "COS"))
        for a, b, an, bn in ((fm, sm, "FREQ", "SIN"), (fm, cm, "FREQ", "COS"), (sm, cm, "SIN", "COS")):
            if a.keys() != b.keys():
                raise ValueError(f"{stem}{an}_ parameters do not match {stem}{bn}_ parameters."
                                 "Please check your prefixed parameters")
        for name in fm.values():
            v = self._params[name].value
            if v is None or v == 0:
                raise ValueError(f"{name} is zero or None. Please check your prefixed parameters")
            if v < 0.0:
                warnings.warn(f"Frequency {name} is negative")
        ep = self._params[f"{stem}EPOCH"]
        if ep.value is None:
            if "PEPOCH" not in self._params or self.PEPOCH.value is None:
                raise MissingParameter(f"{stem}EPOCH or PEPOCH are required if {comp} is being used")
            ep.value = LD(self.PEPOCH.value)

    def mask_params(self, base: str) -> List[str]:
        def build():
            rx = re.compile(rf"^{base}\d+$")
            return [n for n, p in self._params.items() if p.kind == "mask" and rx.match(n)]
        return self._names_of(("mask", base), build)

    # -- validation (the parts of Component.validate that matter on the hot path) -----
    def validate(self):
        for n in self.spin_terms():
            if self._params[n].value is None:
                raise MissingParameter(n)
        if "F0" not in self._params:
            raise MissingParameter("Spindown requires F0")
        if self.PEPOCH.value is None:
            raise MissingParameter("PEPOCH is required (spindown.py:104)")
        if self.astrometry_kind:
            pml = "PMRA" if self.astrometry_kind == 1 else "PMELONG"
            pmb = "PMDEC" if self.astrometry_kind == 1 else "PMELAT"
            if (self[pml].value or self[pmb].value) and self.POSEPOCH.value is None:
                self.POSEPOCH.value = LD(self.PEPOCH.value)  # astrometry.py:339-349
        if "DispersionDM" in self.components:
            if len(self.dm_terms()) > 1 and any(self[n].value for n in self.dm_terms()[1:]):
                if self.DMEPOCH.value is None:
                    self.DMEPOCH.value = LD(self.PEPOCH.value)  # dispersion_model.py:197
        if self.has_solar_wind and int(self.SWM.value or 0) != 0:
            # SWM 1 (the power-law index SWP; solar_wind_dispersion.py:361-364) is not modelled
            raise NotImplementedError(f"solar-wind dispersion with SWM {self.SWM.value} is outside the supported "
                                      "hot path (SWM 0 only)")
        if "CORRECT_TROPOSPHERE" in self and self.CORRECT_TROPOSPHERE.value:
            raise NotImplementedError("troposphere delay (CORRECT_TROPOSPHERE Y) is outside the supported hot path")
        for idx in self.glitch_indices():  # Glitch.validate (glitch.py:155-183)
            ep = self._params.get(f"GLEP_{idx}")
            if ep is None or ep.value is None:
                raise MissingParameter(f"Glitch GLEP_{idx}: Glitch Epoch is needed for Glitch {idx}.")
            ph = self._params.get(f"GLPH_{idx}")
            if ph is not None and not ep.frozen and not ph.frozen:
                raise ValueError(f"Both the glitch epoch and phase cannot be fit for Glitch {idx}.")
            f0d, td = self._params.get(f"GLF0D_{idx}"), self._params.get(f"GLTD_{idx}")
            if f0d is not None and f0d.value and not (td is not None and td.value):
                raise MissingParameter(f"Glitch GLTD_{idx}: None zero GLF0D_{idx} parameter needs a none zero "
                                       f"GLTD_{idx} parameter")
        self.validate_phase_terms()
        for comp in WAVEX_STEMS:
            self.validate_wavex(comp)
        if "ChromaticCM" in self.components:  # ChromaticCM.validate (chromatic_model.py:183-199)
            cm1 = self._params.get("CM1")
            if cm1 is not None and cm1.value is not None and cm1.value != 0.0 and self.CMEPOCH.value is None:
                if self.PEPOCH.value is None:
                    raise MissingParameter("CMEPOCH or PEPOCH is required if CM1 or higher are set")
                self.CMEPOCH.value = LD(self.PEPOCH.value)
        if "CMWaveX" in self.components and "ChromaticCM" not in self.components:
            # (the reference fails only when the delay is first evaluated, with a KeyError on TNCHROMIDX)
            raise TimingModelError("CMWaveX needs a ChromaticCM component (its TNCHROMIDX is the chromatic index)")
        if self.binary in ("DD", "BT", "DDK", "DDS", "DDH"):
            e = float(self.ECC.value or 0.0)
            if not (0 <= e < 1):
                raise ValueError("Eccentricity should be in the range of [0,1).")
        if self.binary and "PB" in self._params and self.PB.value is not None:
            # PulsarBinary.validate (pulsar_binary.py:311-324), for a model with FBn lines (the period
            # form keeps what it did: its PB is checked when the layout is built)
            fb0 = self._params.get("FB0")
            if fb0 is not None and self.PB.value <= 0:
                raise ValueError(f"Binary period PB must be non-negative ({self.PB.value} d)")
            if fb0 is not None and fb0.value is not None:
                raise ValueError("Model cannot have values for both FB0 and PB")
        if self.binary and "FB0" in self._params and self.FB0.value is not None and self.FB0.value <= 0:
            raise ValueError(f"Binary frequency FB0 must be non-negative ({float(self.FB0.value)} 1 / s)")
        if self.binary == "DDS" and self.SHAPMAX.value is not None and not self.SHAPMAX.value > -np.log(2):
            # BinaryDDS.validate (binary_dd.py:200-208)
            raise ValueError(f"SHAPMAX must be > -log(2) ({self.SHAPMAX.value})")
        if self.binary == "DDK":  # BinaryDDK.validate (binary_ddk.py:200-231)
            if not self.astrometry_kind:
                raise TimingModelError("No valid AstrometryEcliptic or AstrometryEquatorial component found")
            if "PX" not in self or self.PX.value is None or self.PX.value <= 0.0:
                raise TimingModelError("DDK model needs a valid `PX` value.")

    # -- noise ------------------------------------------------------------------------
    def red_noise_params(self):
        """(amp, gamma, nmodes) — noise_model.py:761-768 get_pl_vals."""
        nf = int(self.TNREDC.value) if "TNREDC" in self and self.TNREDC.value is not None else 30
        if "TNREDAMP" in self and self.TNREDAMP.value is not None and self.TNREDGAM.value is not None:
            return 10.0 ** float(self.TNREDAMP.value), float(self.TNREDGAM.value), nf
        fac = (86400.0 * 365.24 * 1e6) / (2.0 * np.pi * np.sqrt(3.0))
        return float(self.RNAMP.value) / fac, -1.0 * float(self.RNIDX.value), nf

    def dm_noise_params(self):
        """(amp, gamma, nmodes) of PLDMNoise (noise_model.py:508-511 get_pl_vals)."""
        nf = int(self.TNDMC.value) if "TNDMC" in self and self.TNDMC.value is not None else 30
        return 10.0 ** float(self.TNDMAMP.value), float(self.TNDMGAM.value), nf

    def find_empty_masks(self, toas, freeze=False):
        """Free mask/DMX parameters that select no TOAs (timing_model.py:2895)."""
        bad = []
        for n in self.free_params:
            p = self[n]
            if p.kind == "mask" and len(toas.select_mask(p.key, p.key_value)) == 0:
                bad.append(n)
        mj = toas.get_mjds()
        for n in self.dmx_params():
            tag = n.split("_")[1]
            r1, r2 = float(self["DMXR1_" + tag].value), float(self["DMXR2_" + tag].value)
            if not np.any((mj >= r1) & (mj <= r2)):
                bad.append(n)
        if freeze:
            for n in bad:
                self[n].frozen = True
        return bad

    def copy(self):
        return copy.deepcopy(self)

    # -- device-side evaluation (delegated to the GPU engine) ---------------------------
    def designmatrix(self, toas, incfrozen=False, incoffset=True):
        from .engine import evaluate_designmatrix
        return evaluate_designmatrix(self, toas)

    def delay(self, toas):
        from .engine import evaluate_delay_phase
        return evaluate_delay_phase(self, toas)["delay"]

    def phase(self, toas, abs_phase=True):
        from .engine import evaluate_delay_phase
        return evaluate_delay_phase(self, toas)["phase"]

    def scaled_toa_uncertainty(self, toas):
        from .noise import scaled_sigma_us
        return scaled_sigma_us(self, toas)

    def noise_model_designmatrix(self, toas):
        from .noise import noise_basis
        return noise_basis(self, toas)[0]

    def noise_model_basis_weight(self, toas):
        """timing_model.py:1716: the prior variances, PLRedNoise, PLDMNoise, then ECORR."""
        from .noise import fourier_modes, noise_basis
        if "PLDMNoise" not in self.components:
            return noise_basis(self, toas)[1]
        _, phi, _ = fourier_modes(self, toas)
        ec = noise_basis(_without(self, "PLRedNoise", "PLDMNoise"), toas)[1] if self.mask_params("ECORR") else None
        return phi if ec is None else np.concatenate([phi, ec])

    def __repr__(self):
        return f"<TimingModel {self.name}: {', '.join(self.component_names)}>"


def _without(model, *comps):
    """A shallow view of model without the named components (for the ECORR weights)."""
    import copy as _copy
    m = _copy.copy(model)
    m.components = {k: v for k, v in model.components.items() if k not in comps}
    return m


def _parse_mask_line(model: TimingModel, base: str, fields: List[str], counters: Dict[str, int]):
    comp, units = P.MASK_PARAMS[base]
    key = fields[0]
    klow = key.lower().lstrip("-") if key.startswith("-") else key.lower()
    nkv = 2 if klow in ("mjd", "freq") and not key.startswith("-") else 1
    key_value = fields[1:1 + nkv]
    rest = fields[1 + nkv:]
    counters[base] = counters.get(base, 0) + 1
    idx = counters[base]
    name = "EQUAD" if base == "TNEQ" else base
    p = Param(name=f"{name}{idx}", kind="mask", units=units if base != "TNEQ" else "us",
              component=comp, key=key, key_value=key_value, index=idx,
              long_double=False)
    v = P.fortran_float(rest[0])
    if base == "TNEQ":  # TNEQ is log10(seconds) (noise_model.py:95-128)
        v = 10.0 ** v * 1e6
    p.value = v
    if len(rest) > 1:
        p.frozen = rest[1] != "1"
        p.uncertainty_value = 0.0
    if len(rest) > 2:
        p.set_uncertainty_from_string(rest[2])
    model.add_param(p)
    return p


def _parse_fdjump_lines(model: TimingModel, lines, counters: Dict[str, int]):
    """FDJump's par lines (fdjump.py, model_builder._replace_fdjump_in_parfile_dict:80-99).  A line
    is spelt FD{p}JUMP or, as tempo2 does, FDJUMP{p}; the reference renames the second spelling's
    key in its dictionary of par lines, so when both spellings of one p occur the lines of the
    spelling that appears later in the file replace the other's (recorded in fdj_wls.json
    "forms").  p outside 1..20 is no parameter: the rewritten line is reported as unrecognised.
    The component has FDJUMPLOG (Y) first, then FD{p}JUMP1 of every p in ascending p, then the
    further masks of each p in the order of the lines."""
    import warnings
    groups: Dict[str, Dict[str, list]] = {}  # base -> spelling -> its lines (both in order of first appearance)
    for l in lines:
        base = P.fdjump_base(l.name)
        if base is not None:
            groups.setdefault(base, {}).setdefault(l.name, []).append(l)
    if not groups and not any(l.name == "FDJUMPLOG" for l in lines):
        return
    p = P.make_param("FDJUMPLOG")  # (fdjump.py:69-75: the constructor's value)
    p.value = True
    model.add_param(p)
    kept = []
    for base, spell in groups.items():
        ls = list(spell.values())[-1]
        if base not in P.MASK_PARAMS:
            for l in ls:
                warnings.warn(f"Unrecognized parfile line '{' '.join([base] + l.fields)}'")
            continue
        kept.append((base, ls))
    first = sorted(kept, key=lambda g: int(P.fdjump_base(g[0])[2:-4]))
    for base, ls in first:
        _parse_mask_line(model, base, ls[0].fields, counters)
    for base, ls in kept:
        for l in ls[1:]:
            _parse_mask_line(model, base, l.fields, counters)


def get_model(parfile) -> TimingModel:
    """Build a TimingModel from a par file (model_builder.py:777 get_model)."""
    lines = P.read_parfile(parfile)
    names = [l.name for l in lines]
    model = TimingModel()
    counters: Dict[str, int] = {}
    binary = None
    for l in lines:
        if l.name == "BINARY" and l.fields:
            # (the reference's component names are case-sensitive: ELL1k, not ELL1K; the other
            # names are all upper case and were always matched after upper())
            binary = l.fields[0] if l.fields[0] == "ELL1k" else l.fields[0].upper()
    if binary == "ELL1K":
        raise UnknownBinaryModel("Pulsar system/Binary model component ELL1K is not provided. Perhaps use ELL1k?")
    if binary not in (None,) + BINARIES:
        raise NotImplementedError(f"BINARY {binary} is outside the supported hot path ({', '.join(BINARIES)})")
    model.binary = binary
    # FB0 (alias FB), FB1, ...: the binary's orbit by orbital frequency.  The parameters exist only
    # when the par file names one (the reference carries an unset FB0 on every binary model)
    fb_lines = [n for n in names if n == "FB" or FB_NAME.match(n)]
    if fb_lines and binary not in FBX_BINARIES and binary is not None:
        raise NotImplementedError(f"BINARY {binary} with an FB0 ... FBn orbit ({fb_lines[0]}) is outside the "
                                  f"supported hot path (FB0 with {', '.join(FBX_BINARIES)})")
    if fb_lines and binary is None:
        raise TimingModelError(f"Parameter {fb_lines[0]} is recognized, but not used in the current timing model "
                               "(it has no binary component).")
    has_eq = any(n in ("RAJ", "RA") for n in names)
    has_ecl = any(n in ("ELONG", "LAMBDA") for n in names)
    # defaults the reference components create (values 0 / None)
    defaults = []
    if has_eq:
        defaults += [("POSEPOCH", None), ("PX", 0.0), ("RAJ", None), ("DECJ", None), ("PMRA", 0.0), ("PMDEC", 0.0)]
    if has_ecl:
        defaults += [("POSEPOCH", None), ("PX", 0.0), ("ELONG", None), ("ELAT", None), ("PMELONG", 0.0),
                     ("PMELAT", 0.0), ("ECL", "IERS2010")]
    defaults += [("F0", None), ("PEPOCH", None)]
    # top-level parameters every reference model carries (timing_model.py:330-350)
    defaults += [("DILATEFREQ", False), ("DMDATA", False), ("NTOA", 0), ("UNITS", "TDB")]
    if has_eq or has_ecl:
        defaults += [("PLANET_SHAPIRO", False)]
    if any(n in ("NE_SW", "SOLARN0", "NE1AU") for n in names):
        defaults += [("SWM", 0)]
    if any(n == "DM" or re.match(r"^DM\d+$", n) for n in names):
        defaults += [("DM", LD(0)), ("DMEPOCH", None)]
    wavex_rx = re.compile(r"^(DM|CM)?WX(EPOCH|(FREQ|SIN|COS)_\d+)$")
    # PiecewiseSpindown, Wave and IFunc as constructed (piecewise.py:54-123: the index-1 piece with
    # its epochs unset and its spin terms 0; wave.py:30-58; ifunc.py:59-77), where the phase
    # components go: after Spindown
    if any(re.match(r"^WAVE(EPOCH|_OM|\d+)$", n) for n in names):
        defaults += [("WAVEEPOCH", None), ("WAVE_OM", None)]
    if any(re.match(r"^PW(START|STOP|EP|PH|F0|F1|F2)_\d+$", n) for n in names):
        defaults += [(f"{pre}1", None if pre in PW_DECLARED[:3] else 0.0) for pre in PW_DECLARED]
    if any(re.match(r"^(SIFUNC|IFUNC\d+)$", n) for n in names):
        defaults += [("SIFUNC", None)]
    if binary in ("ELL1", "ELL1H"):
        defaults += [(n, 0.0) for n in ELL1_PARAMS if not (binary == "ELL1H" and n in ("M2", "SINI"))]
        defaults += [("TASC", None)]
        if binary == "ELL1H":  # binary_ell1.py:345-378 (no values by default)
            defaults += [("H3", None), ("H4", None), ("STIGMA", None), ("NHARMS", None)]
    elif binary == "DD":
        defaults += [(n, 0.0) for n in DD_PARAMS]
        defaults += [("T0", None)]
    elif binary == "DDK":  # DD's parameters less SINI, KIN/KOM 0, K96 unset (default True)
        defaults += [(n, 0.0) for n in DDK_PARAMS]
        defaults += [("T0", None), ("K96", None)]
    elif binary == "DDS":  # SHAPMAX 0 as constructed (binary_dd.py:180-188)
        defaults += [(n, 0.0) for n in DDS_PARAMS if n != "SINI"]
        defaults += [("T0", None)]
    elif binary == "DDH":  # H3 and STIGMA unset (binary_dd.py:414-432)
        defaults += [(n, 0.0 if n not in ("H3", "STIGMA") else None) for n in DDH_PARAMS if n not in ("SINI", "M2")]
        defaults += [("T0", None)]
    elif binary == "ELL1k":  # OMDOT and LNEDOT unset (binary_ell1.py:465-483)
        defaults += [(n, 0.0) for n in ELL1K_PARAMS]
        defaults += [("TASC", None)]
    elif binary == "BT":  # binary_bt.py:38-69: no M2/SINI, GAMMA 0, rates 0
        defaults += [(n, 0.0) for n in BT_PARAMS if n != "T0"]
        defaults += [("T0", None)]
    if fb_lines:  # FB0 where the reference's PulsarBinary declares it, after SINI (pulsar_binary.py:192)
        at = max(i for i, (n, _) in enumerate(defaults) if n in ("SINI", "OMDOT")) + 1
        defaults.insert(at, ("FB0", None))
    for n, v in defaults:
        if n in model:
            continue
        p = P.make_param(n)
        if p is None:
            continue
        if n in ("PB", "OM", "OMDOT", "EPS1", "EPS2", "EPS1DOT", "EPS2DOT", "DM") and v is not None:
            v = LD(v)
        p.value = v
        # ELL1's rates are unset (None) in the reference (binary_ell1.py), 0 here
        p.implicit = binary in ("ELL1", "ELL1H", "ELL1k") and n in ("PBDOT", "A1DOT", "EDOT", "OMDOT", "EPS1DOT",
                                                                    "EPS2DOT", "LNEDOT")
        if p.component == "Binary":
            p.component = "Binary"
        model.add_param(p)
    # the derived parameters, where the reference's constructor adds them (after SHAPMAX / STIGMA)
    if binary == "DDS":
        model.add_param(P.FuncParam("SINI", "", _sini_from_shapmax, [model["SHAPMAX"]]))
    elif binary == "DDH":
        model.add_param(P.FuncParam("SINI", "", _sini_from_stigma, [model["STIGMA"]]))
        model.add_param(P.FuncParam("M2", "solMass", _m2_from_h3_stigma, [model["H3"], model["STIGMA"]]))
    # WaveX, DMWaveX, ChromaticCM, then CMWaveX, after the binary's parameters (the components as
    # constructed; ChromaticCM, chromatic_model.py:128-169: CM 0, CM1 unset, CMEPOCH unset, TNCHROMIDX 4)
    for comp, stem in WAVEX_STEMS.items():
        if comp == "CMWaveX" and any(n in ("CM", "CMEPOCH", "TNCHROMIDX") or re.match(r"^CM\d+$", n) for n in names):
            for n, v in (("CM", LD(0)), ("CM1", None), ("CMEPOCH", None), ("TNCHROMIDX", LD(4))):
                p = P.make_param(n)
                p.value = v
                model.add_param(p)
        if any(re.match(rf"^{stem}(EPOCH|(FREQ|SIN|COS)_\d{{4}})$", n) for n in names):
            model._ensure_wavex(comp)
    _parse_fdjump_lines(model, lines, counters)
    for l in lines:
        raw = l.name
        name = P._ALIASES.get(raw, raw)
        if P.fdjump_base(raw) is not None:  # (_parse_fdjump_lines)
            continue
        if name in P.IGNORED or re.match(r"^DMX(EP|F1|F2)_\d+$", name):
            continue
        if name in P.MASK_PARAMS or raw in ("T2EFAC", "T2EQUAD", "TNECORR"):
            base = P._ALIASES.get(raw, raw)
            mp = _parse_mask_line(model, base, l.fields, counters)
            if raw != base and mp is not None:
                mp.alias = raw
            continue
        if name == "BINARY":
            p = model._params.get("BINARY") or P.make_param("BINARY")
            p.value = l.fields[0] if l.fields else None
            if "BINARY" not in model:
                model.add_param(p)
            continue
        if binary == "ELL1k" and name in ELL1K_REMOVED:
            # (BinaryELL1k removes them, binary_ell1.py:460-463; the reference's model builder then
            # refuses the line, ell1k_wls.json "forms")
            raise TimingModelError(f"Parameter {name} is recognized, but not used in the current timing model "
                                   "(BinaryELL1k has OMDOT and LNEDOT in place of EPS1DOT, EPS2DOT and EDOT).")
        if name not in model:
            p = P.make_param(name)
            if p is None:
                if name in ("SWP", "H3", "STIGMA"):
                    continue
                if wavex_rx.match(name):  # (only the four-digit index is a name: model_builder warns and goes on)
                    import warnings
                    warnings.warn(f"Unrecognized parfile line '{' '.join([raw] + l.fields)}'")
                    continue
                raise NotImplementedError(f"parameter {raw} is outside the supported hot path")
            model.add_param(p)
        p = model[name]
        if raw != name:
            p.alias = raw
        if not l.fields:
            continue
        if p.kind == "pair":  # (pairParameter.from_parfile_line: two values, whatever follows is ignored)
            if len(l.fields) > 1:
                p.set_pair_from_strings(l.fields[0], l.fields[1])
            continue
        p.set_from_string(l.fields[0])
        # TimingModel.validate (timing_model.py:405-413): the only values PINT supports
        if name == "TIMEEPH" and p.value not in (None, "FB90"):
            p.value = "FB90"
        elif name == "T2CMETHOD" and p.value not in (None, "IAU2000B"):
            p.value = "IAU2000B"
        elif name == "DILATEFREQ" and p.value:
            p.value = False
        if len(l.fields) > 1 and p.kind not in ("str", "bool"):
            # parameter.py:551-576: a third field is a fit flag (uncertainty 0 unless a
            # fourth field gives it) or an uncertainty
            fl = l.fields[1]
            if fl in ("0", "1"):
                p.frozen = fl != "1"
                p.uncertainty_value = 0.0
                if len(l.fields) > 2:
                    p.set_uncertainty_from_string(l.fields[2])
            else:
                p.set_uncertainty_from_string(fl)
    if fb_lines:
        # PulsarBinary.setup (pulsar_binary.py:217-228) and OrbitFBX (binary_orbits.py:164-173).  With
        # FBn the model has PB unset unless the par file gives it (validate then refuses both).
        if "PB" not in names:
            model["PB"].value = None
        fbs = {int(FB_NAME.match(n).group(1)): model[n] for n in model.fb_terms()}
        if any(p.value is not None for p in fbs.values()):
            if fbs[0].value is None:
                raise ValueError("Some FBn parameters are set but FB0 is not.")
            indices = {k for k, p in fbs.items() if p.value is not None}
            if indices != set(range(len(indices))):
                # (the reference means to raise this but never does: every FBn is in the list its
                # OrbitFBX is given, so the check sees no index, and the sums then stop at the first
                # missing one, silently dropping the terms above a gap)
                raise ValueError(f"Indices must be 0 up to some number k without gaps but are {indices}.")
    model.setup_glitches()
    # components present
    comps = set()
    for n, p in model._params.items():
        comps.add(p.component)
    if has_eq:
        model.components.setdefault("AstrometryEquatorial", [])
    if has_ecl:
        model.components.setdefault("AstrometryEcliptic", [])
    if has_eq or has_ecl:
        model.components.setdefault("SolarSystemShapiro", [])
    if binary:
        model.components["Binary" + binary] = model.components.pop("Binary", [])
    if model.mask_params("JUMP"):
        model.components.setdefault("PhaseJump", [])
    if "DMX" in model and not model.dmx_params():
        pass
    for noise in ("TNREDAMP", "RNAMP"):
        if noise in model and model[noise].value is not None:
            model.components.setdefault("PLRedNoise", [])
    if "TNDMAMP" in model and model.TNDMAMP.value is not None:
        model.components.setdefault("PLDMNoise", [])
    # normalise the components dict keys used above for the binary
    for n, p in model._params.items():
        if p.component == "Binary":
            p.component = "Binary"
    if "PSR" in model:
        model.name = str(model.PSR.value)
    model.validate()
    return model
