"""No GPU: what tests/test_gpu_glm_replay.py relies on and cannot check against the device.

Every iteration of every oracle chain of tests/_glm_oracle.CASES is replayed, from a deep copy of the step and the generator,
with a second and independent statement of the posterior (np.longdouble, BLAS order: _glm_oracle.oracle_glm_longdouble), and
compared by the comparison the device replay runs (tests/_replay.iteration_errors under Rules.diag()): integer statistics
equal, positions at rtol 1e-11 / atol 1e-12, float statistics at 1e-10. These are the tightest comparisons any case is held
to on the device (the dense float64 cases allow atol 1e-11 (1 + max |q|), the float32-born ones 1e-5), so one table serves all.

* reference against reference stays 50 times below the tolerance: the tolerance is not at the noise;
* three small errors in the posterior fail at least half of the iterations: the tolerance is not above what matters;
* at most two iterations per chain have an oracle margin below the floor the device replay skips by, so its
  "checked >= total - 2" hides nothing."""
import copy

import numpy as np
import pytest

from tests import _glm_oracle as GO
from tests._replay import Rules, chain_iterations, iteration_errors

CPU_ITERATIONS_WIDE = 12      # the oracle costs ~50 ms per iteration for d >= 257: a prefix of those chains is replayed here
_table = []


@pytest.fixture(scope="module", autouse=True)
def _separation_table():
    """Prints the table of the cases that ran (pytest -s), after the last of them."""
    yield
    print("\n%-28s %5s %11s %8s %8s %5s" % ("case", "iters", "separation", "margins", "tree", "div"))
    for row in _table:
        print("%-28s %5d %11.4f %8d %8d %5d" % row)


def _replay_with(c, f_other, n_iter):
    """The oracle chain of case ``c`` (record_chain's driver: tests/_replay.chain_iterations); before every iteration the step
    and the generator are deep-copied, the copy is given ``f_other`` and takes the iteration too: the twin's iteration is
    "got", the oracle's "want", under Rules.diag() with no next snapshot (iteration_errors).
    Returns [(all comparisons hold, separation)] per iteration and the chain's positions."""
    ostep, start, seed = GO.oracle_step(c)
    rng = np.random.RandomState(int(seed))
    q = np.array(start, dtype="d")
    out, qs = [], []
    for _i in chain_iterations(ostep, c.tune, n_iter):
        twin, twin_rng = copy.deepcopy(ostep), copy.deepcopy(rng)
        twin.f = f_other
        tq, tst = twin.astep(q.copy(), twin_rng)
        q, st = ostep.astep(q, rng)
        errors, separation, _stat = iteration_errors(dict(q=tq, stats={k: np.ravel(v)[0] for k, v in tst.items()}),
                                                     dict(q=q, stats={k: np.ravel(v)[0] for k, v in st.items()}), None, Rules.diag())
        out.append((not errors, separation))
        qs.append(q.copy())
    return out, np.array(qs)


def _n_iter(c):
    return CPU_ITERATIONS_WIDE if c.d >= 257 else c.tune + c.draws


@pytest.mark.parametrize("c", GO.CASES, ids=GO.case_id)
def test_two_statements_of_the_posterior_replay_each_other(c):
    n = _n_iter(c)
    res, qs = _replay_with(c, GO.oracle_glm_longdouble(c.N, c.d, c.lik), n)
    snaps, outs = GO.oracle_chain(c)
    assert len(outs) == c.tune + c.draws
    # the chain replayed here IS the chain the device test replays
    np.testing.assert_array_equal(qs, np.array([o["q"] for o in outs[:n]]))
    worst = max(sep for _ok, sep in res)
    low = sum(GO.rules(c).skips(o) for o in outs)
    sizes = [o["stats"].get("tree_size", o["stats"].get("n_steps")) for o in outs]
    div = sum(bool(o["stats"]["diverging"]) for o in outs)
    _table.append((GO.case_id(c), n, worst, low, int(max(sizes)), div))
    print("%s: %d iterations, separation %.4f of the tolerance, %d margins below %g, largest tree %d, %d divergences" % (
        GO.case_id(c), n, worst, low, GO.rules(c).floor, max(sizes), div))
    assert all(ok for ok, _sep in res), [i for i, (ok, _s) in enumerate(res) if not ok]
    assert worst < 1.0 / 50.0, worst
    assert low <= 2, low


def test_the_poisson_cell_diverges():
    """(65, 65, poisson) is where the device replay holds the divergence path to the oracle: it needs divergences to hold."""
    c = next(k for k in GO.FUSED if (k.N, k.d, k.lik) == (65, 65, "poisson"))
    assert sum(bool(o["stats"]["diverging"]) for o in GO.oracle_chain(c)[1]) >= 3


@pytest.mark.parametrize("mutant", GO.MUTANTS)
@pytest.mark.parametrize("cell", [(63, 3, "bernoulli"), (65, 65, "poisson")], ids=lambda v: "%d-%d-%s" % v)
def test_a_small_error_in_the_posterior_fails_the_replay(cell, mutant):
    c = next(k for k in GO.FUSED if (k.N, k.d, k.lik) == cell)
    n = c.tune + c.draws
    res, _qs = _replay_with(c, GO.oracle_glm_longdouble(*cell, mutant=mutant), n)
    failing = sum(not ok for ok, _sep in res)
    print("%s %s: %d of %d iterations fail" % (GO.case_id(c), mutant, failing, n))
    assert 2 * failing >= n, (failing, n)
