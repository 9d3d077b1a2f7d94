#!/usr/bin/env python3
"""Report the observed device-vs-oracle differences of the dense-mass replay (tests/test_gpu_dense.py), per golden
case: used to choose the tolerances stated in tests/_replay.py. Run on a GPU box from the repo root."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_gpu_dense as T  # noqa: E402
from tests._replay import dense_rules, iteration_errors, record_chain, run_snapshots  # noqa: E402

golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
for name in T.DENSE_E2E:
    g = T._load(golden, name)
    tune, draws = int(g["tune"]), int(g["draws"])
    ostep, dstep, start = T._oracle_and_device_steps(g)
    snaps, outs = record_chain(ostep, start, np.random.RandomState(int(g["seeds"][0])), tune, draws)
    rules = dense_rules(str(g["potential"]) not in ("inv", "full64"))
    ran = run_snapshots(dstep, snaps)
    print("%-32s %d iterations at tol %g, skip floor %g" % (name, tune + draws, rules.q[0], rules.floor))
    worst_q = worst_stat = 0.0
    for i, want in enumerate(outs):
        errors, q_err, stat_err = iteration_errors(ran[i], want, snaps[i + 1] if i + 1 < len(snaps) else None, rules)
        worst_q, worst_stat = max(worst_q, q_err), max(worst_stat, stat_err)
        if errors:
            print("    iter %4d margin %.2e%s: %s" % (i, rules.margin(want), " (skipped)" if rules.skips(want) else "", errors))
    print("    worst position error %.3g, worst float statistic error %.3g of the tolerance" % (worst_q, worst_stat))
