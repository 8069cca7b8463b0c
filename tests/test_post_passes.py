"""Every pass around the evaluation in one batch (k_sw_geom before it; k_wavex in its chromatic
build, k_fdjump, k_glitch and k_phase_terms after it, in that order): one fixture of each
component family and a plain pulsar side by side, so that every pass is launched and each takes
its block-uniform early return on the instances without its component.  The passes work per row
and know nothing of the batch, so each instance's outputs are the bits of the same model alone.
"""
import copy

import numpy as np
import pytest


def _items():
    """(model, toas) of sw_ecl, wx_wls, cm_wls, fdj_wls, gl_wls, pw_wls, wave_wls and pta_iso, each
    through its own module's load."""
    import golden_util
    import test_chromatic
    import test_fdjump
    import test_glitch
    import test_phase_terms
    import test_solar_wind
    import test_wavex
    return [mod.load(name)[:2] for mod, name in (
        (test_solar_wind, "sw_ecl"), (test_wavex, "wx_wls"), (test_chromatic, "cm_wls"), (test_fdjump, "fdj_wls"),
        (test_glitch, "gl_wls"), (test_phase_terms, "pw_wls"), (test_phase_terms, "wave_wls"), (golden_util, "pta_iso"))]


def _eval_all(items):
    """Of every (model, toas) in one session: delay, phase, spin frequency, the full-layout
    design matrix and the residuals, then the evaluation outputs and the residuals again from an
    evaluation with the fit layout's design matrix (no Gram: a batch chooses its own row split)."""
    from pint_amd.engine import Session, build_layout, pack_table
    s = Session()
    lays = [s.add(build_layout(copy.deepcopy(m), t)) for m, t in items]
    s.set_instances([(lay, pack_table(lay)) for lay in lays])
    out = [[] for _ in items]
    for want in (True, Session.FIT):
        s.eval(want_M=want)
        ev = s.read_eval()
        M = s.read_designmatrix() if want is True else None
        tr, pr, c2 = s.read_resids()
        for k in range(len(items)):
            out[k] += [np.array(x[k], copy=True) for x in ev]
            if M is not None:
                out[k].append(np.array(M[k], copy=True))
            out[k] += [np.array(tr[k], copy=True), np.array(pr[k], copy=True), np.float64(c2[k])]
    s.close()
    return out


@pytest.mark.gpu
def test_gpu_every_pass_in_one_batch():
    items = _items()
    mixed = _eval_all(items)
    for k, it in enumerate(items):
        (alone,) = _eval_all([it])
        assert len(mixed[k]) == len(alone) == 15
        for x, y in zip(mixed[k], alone):
            np.testing.assert_array_equal(x, y)
