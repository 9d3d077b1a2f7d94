"""No GPU: what each rule of tests/_replay.py asserts, on synthetic records. For every comparison of the rules table a
perturbation of half the stated tolerance yields no error and one of twice the tolerance yields exactly that error; an exact
comparison (integer statistic, generator position, counts, windows) yields exactly its error for a difference of one."""
import copy

import numpy as np
import pytest

from tests._replay import DeviceIterations, Rules, assert_replay, iteration_errors

TOL, FLOOR = 1e-5, 1e-4
RULES = {"diag": Rules.diag(), "dense": Rules.dense(TOL, FLOOR), "dense-tol": Rules.dense(TOL, FLOOR, da_atol="tol"),
         "dense-all": Rules.dense(TOL, FLOOR, dense_state="all")}
D = 4
ENERGY, DA_COUNT = 12.5, 9


def _records():
    """(got, want, nxt) that agree exactly: one tuning iteration followed by another."""
    rs = np.random.RandomState(7)
    q = 3.0 * rs.randn(D)
    stats = dict(energy=ENERGY, mean_tree_accept=0.83, step_size=0.4, tree_size=7.0, depth=3, diverging=False, tune=True)
    a = rs.randn(D, D)
    cov = a @ a.T + np.eye(D)
    vec = lambda: 1.0 + rs.rand(D)   # noqa: E731
    chain = dict(var=vec(), log_step=-0.7, log_bar=-0.9, hbar=0.3, da_count=DA_COUNT, n_samples=DA_COUNT, fore_mean=vec(),
                 fore_raw_var=vec(), back_mean=vec(), back_raw_var=vec(), fore_w_sum=19.0, back_w_sum=9.0, window=101)
    dense = dict(cov=cov, chol=np.linalg.cholesky(cov), window=101, previous_update=0, fore_n=19.0, back_n=9.0)
    nxt = dict(chain, tune=True, **{k: v for k, v in dense.items() if k != "window"})
    got = dict(q=q.copy(), stats=dict(stats), after=dict(copy.deepcopy(chain), var64=chain["var"].copy()),
               dense=copy.deepcopy(dense), rng_pos=311, tune=True)
    want = dict(q=q, stats=stats, rng_pos=311, lb=1.0, turn=1.0, div=1.0)
    return got, want, nxt


def _bumped(got, path, delta):
    got = copy.deepcopy(got)
    node = got
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = node[path[-1]] + delta
    return got


DA = ("log_step", "log_bar", "hbar")
_DIAG_DA = lambda v, w, n: 1e-13 + 1e-11 * abs(v)   # noqa: E731
_DENSE_DA = lambda v, w, n: TOL * abs(v) + TOL * (1 + ENERGY) * (1 + np.sqrt(DA_COUNT) / 0.05)   # noqa: E731

# (rules, the error's name, where it lives in ``got``, the stated tolerance as a function of (wanted value, want, nxt); None: exact)
COMPARISONS = [
    ("diag", "q", ("q", 1), lambda v, w, n: 1e-12 + 1e-11 * abs(v)),
    ("diag", "energy", ("stats", "energy"), lambda v, w, n: 1e-10 + 1e-10 * abs(v)),
    ("diag", "depth", ("stats", "depth"), None),
    ("diag", "rng_pos", ("rng_pos",), None),
    *[("diag", k, ("after", k), _DIAG_DA) for k in DA],
    ("diag", "var", ("after", "var", 2), lambda v, w, n: 2e-7 * abs(v)),
    ("diag", "var64", ("after", "var64", 2), lambda v, w, n: 1e-12 * abs(v)),
    ("diag", "fore_mean", ("after", "fore_mean", 0), _DIAG_DA),
    ("diag", "window", ("after", "window"), None),
    ("dense", "q", ("q", 1), lambda v, w, n: TOL * abs(v) + TOL * (1 + np.abs(w["q"]).max())),
    ("dense", "energy", ("stats", "energy"), lambda v, w, n: TOL * abs(v) + TOL * (1 + ENERGY)),
    ("dense", "depth", ("stats", "depth"), None),
    ("dense", "rng_pos", ("rng_pos",), None),
    *[("dense", k, ("after", k), _DENSE_DA) for k in DA],
    ("dense-tol", "log_step", ("after", "log_step"), lambda v, w, n: TOL * abs(v) + TOL),
    ("dense", "cov", ("dense", "cov", (1, 2)), lambda v, w, n: 2 * TOL * np.abs(n["cov"]).max()),
    ("dense-all", "chol", ("dense", "chol", (2, 1)), lambda v, w, n: 10 * TOL * np.sqrt(np.abs(n["cov"]).max())),
    ("dense-all", "window", ("dense", "window"), None),
]


@pytest.mark.parametrize("rule, name, path, tolerance", COMPARISONS, ids=["%s-%s" % c[:2] for c in COMPARISONS])
def test_a_comparison_holds_at_half_its_tolerance_and_fails_alone_at_twice(rule, name, path, tolerance):
    got, want, nxt = _records()
    rules = RULES[rule]
    assert iteration_errors(got, want, nxt, rules)[0] == []
    if tolerance is None:
        errors = iteration_errors(_bumped(got, path, 1), want, nxt, rules)[0]
        assert [e[0] for e in errors] == [name], errors
        return
    wanted = got
    for k in path:
        wanted = wanted[k]
    tol = tolerance(wanted, want, nxt)
    for sign in (1.0, -1.0):
        assert iteration_errors(_bumped(got, path, sign * 0.5 * tol), want, nxt, rules)[0] == []
        errors, q_err, stat_err = iteration_errors(_bumped(got, path, sign * 2.0 * tol), want, nxt, rules)
        assert [e[0] for e in errors] == [name], errors
        if path[0] == "q":
            assert q_err == pytest.approx(2.0, rel=1e-3) and stat_err == 0.0
        if path[0] == "stats":
            assert stat_err == pytest.approx(2.0, rel=1e-3) and q_err == 0.0


def test_the_divergence_margin_skips_under_the_dense_rule_only():
    got, want, nxt = _records()
    want = dict(want, div=0.5 * FLOOR)           # lb and turn far above every floor
    ran = DeviceIterations(1)
    ran.iterations[0] = _bumped(got, ("q", 0), 1.0)      # far off: whoever compares it, fails
    assert RULES["dense"].skips(want) and not RULES["diag"].skips(want)
    assert assert_replay(ran, [nxt], [want], RULES["dense"], "div margin")[:2] == (0, 1)
    with pytest.raises(AssertionError, match="div margin iter 0"):
        assert_replay(ran, [nxt], [want], RULES["diag"], "div margin")
    ran.iterations[0] = got
    assert assert_replay(ran, [nxt], [want], RULES["diag"], "div margin")[:2] == (1, 0)
    assert assert_replay(ran, [nxt], [want], RULES["diag"], "div margin", skip=lambda i: True)[:2] == (0, 1)


def test_the_after_reset_hook_runs_once_between_the_reset_and_the_first_iteration():
    """record_chain / chain_iterations(after_reset=...): what the hook sets survives reset_tuning() and is what the first
    snapshot carries -- a chain that starts where no short chain gets to (a dual-averaging count of 16 380)."""
    from oracle import lmc_oracle as orc
    from oracle import targets as OT
    from tests._replay import chain_iterations, record_chain

    d, seed = 3, 77
    calls = []

    def late(step):
        assert step.tune and step.adapt.count == 1 and step.adapt.hbar == 0.0    # reset_tuning() has already run
        calls.append(step)
        step.adapt.count = 16380

    def chain(hook):
        start, ostep = orc.init_nuts(OT.make("std_normal", d), d, seeds=[seed], k=0.6)
        ostep.adapt.count = 5                                                      # (a left-over the reset clears)
        return ostep, record_chain(ostep, start, np.random.RandomState(seed), 4, 2, after_reset=hook)

    ostep, (snaps, outs) = chain(late)
    assert calls == [ostep]
    assert [s["da_count"] for s in snaps] == [16380, 16381, 16382, 16383, 16384, 16384]   # draws do not count
    assert [s["tune"] for s in snaps] == [True] * 4 + [False] * 2 and [s["iter_count"] for s in snaps] == list(range(6))
    _, (plain, plain_outs) = chain(None)
    assert [s["da_count"] for s in plain] == [1, 2, 3, 4, 5, 5]
    np.testing.assert_array_equal(plain[0]["q"], snaps[0]["q"])
    np.testing.assert_array_equal(plain_outs[0]["q"], outs[0]["q"])            # the first transition does not read the count
    assert plain[1]["log_bar"] != snaps[1]["log_bar"]                            # ... its update does: count ** -k
    w = 1.0 / (16380 + 10)
    assert snaps[1]["hbar"] == pytest.approx(w * (0.8 - outs[0]["stats"]["mean_tree_accept"]), rel=1e-14)
    # chain_iterations on its own: once, before the first yield
    calls.clear()
    seen = [(i, len(calls)) for i in chain_iterations(ostep, 2, 3, after_reset=late)]
    assert seen == [(0, 1), (1, 1), (2, 1)]
