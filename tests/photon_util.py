"""Loader of the photon fixtures (scripts/refgen/gen_photon.py) for tests/test_eventstats.py and
tests/test_photon.py (test infrastructure)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("photon_geo", "photon_bary")
LD = np.longdouble
_CACHE = {}


def load(name):
    """(model, toas, arrays, meta) of a fixture: the arrays, the meta and the TOAs are loaded once,
    shared and never changed; the model is a fresh one per caller."""
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    if name not in _CACHE:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        for v in z.values():
            v.setflags(write=False)
        _CACHE[name] = (from_arrays_with_tzr(z, dict(meta["flag_columns"]), name, meta.get("obs_names")), z, meta)
    toas, z, meta = _CACHE[name]
    model = get_model(os.path.join(GOLDEN, name + ".par"))
    model.free_params = list(meta["model"]["free_params"])
    return model, toas, z, meta


def spread():
    if "spread" not in _CACHE:
        _CACHE["spread"] = json.load(open(os.path.join(GOLDEN, "photon_spread.json")))
    return _CACHE["spread"]


def points(pt, z, meta):
    """The fixture's 16 points (longdouble) in the column order of the PhotonTiming object pt."""
    perm = [meta["labels"].index(p) for p in pt.param_labels]
    return (z["pts_hi"].astype(LD) + z["pts_lo"].astype(LD))[:, perm]
