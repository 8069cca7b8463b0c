"""What the FBn orbit costs in the evaluation: the device time of the
evaluation with the fit layout's design matrix (pint_last_timing slot 4, fused residual pass off,
as wavex_cost.eval_ms takes it) of the fbx_* fixtures against the same model in the period form:
PB = 1 / FB0 and PBDOT = -FB1 / FB0^2 free in place of FB0 and FB1, the higher terms dropped (two
or three binary columns fewer).  Each fixture is evaluated as one instance (latency) and as --copies
instances of the same pulsar (throughput: 300 rows are two blocks, far below one round of the chip).

    python3 scripts/diag/fbx_cost.py [--copies 256] [--evals 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAMES = ("fbx_ell1_wls", "fbx_ell1h_wls", "fbx_dd_wls", "fbx_bt_wls", "fbx_ell1_gls", "fbx_dd_gls")


def period_form(par):
    """The fixture's par text with PB and PBDOT (free) for FB0 and FB1, FB2 ... dropped."""
    LD = np.longdouble
    vals = {l.split()[0]: LD(l.split()[1]) for l in par.splitlines() if l.split() and l.split()[0].startswith("FB")}
    out = []
    for l in par.splitlines():
        k = l.split()[0] if l.split() else ""
        if k == "FB0":
            l = f"PB {1 / vals['FB0'] / 86400} 1"
        elif k == "FB1":
            l = f"PBDOT {-vals['FB1'] / vals['FB0'] ** 2} 1"
        elif k.startswith("FB"):
            continue
        out.append(l)
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--evals", type=int, default=20)
    args = ap.parse_args()
    from golden_util import GOLDEN
    from wavex_cost import eval_ms
    from pint_amd import get_model
    from pint_amd.toa import from_arrays_with_tzr
    res = {}
    for name in NAMES:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        toas = from_arrays_with_tzr(z, dict(meta["flag_columns"]), name, meta.get("obs_names"))
        par = open(os.path.join(GOLDEN, name + ".par")).read()
        models = {"fbn": get_model(par), "period": get_model(period_form(par))}
        if name.endswith("gls"):
            for m in models.values():
                m.find_empty_masks(toas, freeze=True)
        r = {"rows": toas.ntoas + 1}
        for form, m in models.items():
            r[form + "_ncol"] = len(m.free_params) + 1
            r[form + "_one_ms"] = eval_ms([(m, toas)], args.evals)[0]
            r[form + f"_x{args.copies}_ms"] = eval_ms([(m, toas)] * args.copies, args.evals)[0]
        r["ratio_one"] = r["fbn_one_ms"] / r["period_one_ms"]
        r["ratio_batch"] = r[f"fbn_x{args.copies}_ms"] / r[f"period_x{args.copies}_ms"]
        res[name] = r
        print(name, json.dumps(r), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
