"""Search (on the CPU oracle) for motion-only-BA inputs that take the branches of g2o's Levenberg-Marquardt a good prior never reaches: rejected
trials, Terminate, NaN steps.  Its hits are the PNP_HARD tables of tests/case_tables.py.

    python tests/tools/pnp_hard_cases.py                  the (n, prior, outliers) settings PNP_HARD came from
    python tests/tools/pnp_hard_cases.py 1600 2500 4096   the hard settings at these edge counts (PNP_HARD_UNSTAGED: above k_pnp's staging limit)

A hit is printed as (seed, trials, rejections, terminates, NaN step, solve calls, inliers, first noise-level trial): a row whose first noise-level
trial equals its number of trials is comparable to its last trial."""
import os, sys, numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import lvt_amd
from oracle import pyoracle as O
from case_tables import pnp_hard_case, trace_noise
prm = lvt_amd.kitti_params()

SETTINGS = [(300, 1.5, 10, 0.3, 25), (300, 2.0, 10, 0.3, 60), (200, 2.0, 15, 0.3, 200), (100, 3, 30, 0.4, 300), (60, 5, 60, 0.5, 400), (40, 8, 120, 0.5, 400),
            (30, 10, 170, 0.3, 100)]
if len(sys.argv) > 1:
    SETTINGS = [(int(n), off_t, off_deg, outl, big) for n in sys.argv[1:] for (off_t, off_deg, outl, big) in ((5, 60, 0.5, 400), (8, 120, 0.5, 400), (10, 170, 0.3, 100))]

for (n, off_t, off_deg, outl, big) in SETTINGS:
    found = []
    for seed in range(40):
        X, uv, q0, p0 = pnp_hard_case(prm, seed, n, off_t, off_deg, outl, big)
        q, p, marks, tr = O.pnp(prm, q0, p0, X, uv)
        nan = bool(np.isnan(tr).any())
        found.append((seed, O.pnp.last_trials, O.pnp.last_rejections, O.pnp.last_terminates, nan, O.pnp.last_solve_calls, int(marks.sum()), trace_noise(tr)))
    print((n, off_t, off_deg, outl, big))
    print("  rej>0:", [f for f in found if f[2] > 0][:6])
    print("  term>0:", [f for f in found if f[3] > 0][:6])
    print("  nan:", [f for f in found if f[4]][:6])
