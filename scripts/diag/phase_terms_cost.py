"""What the PiecewiseSpindown / Wave / IFunc pass costs, after fdjump_cost.py's
measurement: the bench's 68-pulsar x 10k-TOA PTA with two pieces (PWF0 / PWF1 free), five WAVE terms
and 64 IFUNC points (SIFUNC 2) on every pulsar, against the same PTA without them, and beside it the
same PTA with one glitch per pulsar (glitch_cost.py's lines), whose pass k_glitch has the same form.

Each pass's own time: the device time of the evaluation with the fit layout's design matrix
(pint_last_timing slot 4, which ends after k_wavex / k_fdjump / k_glitch / k_phase_terms and before
the residual pass) of the batch with the components less that of the plain batch, both with the
fused residual pass off and the red-noise columns stored in M (PINT_OPT_VGRAM 0), so that the two
run the same evaluation kernels and differ by the pass and by the evaluation's zero fill of the
new columns (which the pass then overwrites); median of --evals evaluations.

Per row and evaluation with the design matrix k_phase_terms reads 5 doubles (tdb, delay, phase),
the pieces and the Wave terms from the table (block-uniform, cached) and about log2(64) + 2 IFUNC
points, and writes 2 doubles and 4 doubles of columns; it evaluates one sincos.

    python3 scripts/diag/phase_terms_cost.py [--npsr 68] [--evals 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PW_LINES = ("PWSTART_1 53500.3\nPWSTOP_1 54400.7\nPWEP_1 53700.1\nPWPH_1 0.2\nPWF0_1 1e-6 1\nPWF1_1 1e-15 1\nPWF2_1 0\n"
            "PWSTART_2 55200.4\nPWSTOP_2 56000.6\nPWEP_2 55600.2\nPWPH_2 -0.1\nPWF0_2 -2e-7 1\nPWF1_2 -3e-15 1\nPWF2_2 0\n")
WAVE_LINES = ("WAVEEPOCH 54900\nWAVE_OM 0.0017\nWAVE1 1e-6 -5e-7\nWAVE2 -2e-7 3e-7\nWAVE3 8e-8 4e-8\nWAVE4 -3e-8 1e-8\n"
              "WAVE5 7e-9 -1.2e-8\n")
IFUNC_LINES = "SIFUNC 2 0\n" + "".join(f"IFUNC{i + 1} {53010.25 + 57.5 * i} {((-1) ** i) * 1e-7 * (1 + i % 5)}\n"
                                       for i in range(64))
GLITCH = "GLEP_1 55000.37\nGLPH_1 0.05 1\nGLF0_1 2e-8 1\nGLF1_1 -1e-17 1\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npsr", type=int, default=68)
    ap.add_argument("--ntoas", type=int, default=10000)
    ap.add_argument("--evals", type=int, default=20)
    args = ap.parse_args()
    from wavex_cost import eval_ms
    from pint_amd import get_model
    from pint_amd import simulation as sim
    idx = list(range(args.npsr))
    models = {"plain": [sim.pta_model(i) for i in idx],
              "phase_terms": [get_model(sim.pta_par(i, sim.pta_kind(i)) + PW_LINES + WAVE_LINES + IFUNC_LINES) for i in idx],
              "glitch": [get_model(sim.pta_par(i, sim.pta_kind(i)) + GLITCH) for i in idx]}
    ev = {name: eval_ms(sim.make_pta(ntoas=args.ntoas, indices=idx, models=ms), args.evals) for name, ms in models.items()}
    rows = ev["plain"][1]
    k_pt, k_gl = ev["phase_terms"][0] - ev["plain"][0], ev["glitch"][0] - ev["plain"][0]
    print(json.dumps({"npsr": args.npsr, "ntoas": args.ntoas, "npw": 2, "nwave": 5, "nifunc": 64,
                      "eval_with_M_device_ms": {k: v[0] for k, v in ev.items()}, "rows": rows,
                      "k_phase_terms_ms": k_pt, "k_phase_terms_ns_per_row": k_pt * 1e6 / rows,
                      "k_glitch_ms": k_gl, "k_glitch_ns_per_row": k_gl * 1e6 / rows}))


if __name__ == "__main__":
    main()
