"""What a glitch costs the headline workload: the bench's 68-pulsar x
10k-TOA PTA with one glitch inside the span added to every pulsar (GLEP_1 frozen; GLPH_1, GLF0_1,
GLF1_1 free) against the same PTA without it, timed by the bench's own step loop
(bench.timed_steps: one GLSFitter.fit_toas(maxiter=1) of every pulsar per step), the two batches
alternating.  The glitch batch has three more compact timing columns per pulsar in the Gram and
forms the glitch phase and columns in every evaluation.

    python3 scripts/diag/glitch_cost.py [--steps 100] [--reps 3] [--npsr 68]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

GLITCH = "GLEP_1 55000.37\nGLPH_1 0.05 1\nGLF0_1 2e-8 1\nGLF1_1 -1e-17 1\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--npsr", type=int, default=68)
    ap.add_argument("--ntoas", type=int, default=10000)
    args = ap.parse_args()
    from bench import pipelines, timed_steps
    from pint_amd import get_model
    from pint_amd import simulation as sim
    idx = list(range(args.npsr))
    plain = [sim.pta_model(i) for i in idx]
    glitch = [get_model(sim.pta_par(i, sim.pta_kind(i)) + GLITCH) for i in idx]
    batches = {"plain": sim.make_pta(ntoas=args.ntoas, indices=idx, models=plain),
               "glitch": sim.make_pta(ntoas=args.ntoas, indices=idx, models=glitch)}
    ms = {k: [] for k in batches}
    for rep in range(args.reps):
        for name, items in batches.items():
            ss, lays = pipelines(items, 2)
            dt = timed_steps(ss, args.steps, args.warmup, lambda: None, lambda v: v, graph="0", gram_pass=False,
                             pipes="auto")[0]
            for s in ss:
                s.close()
            ms[name].append(round(dt / args.steps * 1e3, 4))
            print(f"rep {rep} {name}: {ms[name][-1]} ms/step (K max {max(l.K for l in lays)})", file=sys.stderr, flush=True)
    print(json.dumps({"npsr": args.npsr, "ntoas": args.ntoas, "steps": args.steps, "ms_per_step": ms,
                      "median": {k: float(np.median(v)) for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
