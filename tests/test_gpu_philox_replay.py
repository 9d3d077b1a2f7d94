"""momentum_rng="philox" on the device (include/lmc_hip.h: LMC_RNG_PHILOX, run_kernel<NS, W, Target, 1>): the momentum normals
are a pure function of (chain seed, iteration, element), every uniform is the chain's MT19937 stream. The device hands out
its own normals (Engine.counter_draws) and takes any generator state (Engine.set_rng_state), so the UNCHANGED oracle on
tests/_counter_model.MomentumOnlyRng -- the device's normals, numpy's uniforms -- is an exact model of the mode: the stream
is held to the counter mode's and to the host model, every iteration of every kernel shape is replayed against the oracle
under the project's one table of tolerances (tests/_replay.Rules.diag(), generator position exact), and the driver is held to
free-running oracle chains across launch boundaries."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import targets as T
from oracle import lmc_oracle as orc
from oracle import targets as OT
from tests import _counter_model as cm
from tests._gpu_util import FRAGILE, assert_chain_matches
from tests._replay import Rules, assert_replay, record_chain, run_keyed_iterations
from tests.test_gpu_counter_rng import CASES as COUNTER_CASES
from tests.test_gpu_counter_rng import NORMALS_MEASURED_MAX_ABS, SEED, _steps

pytestmark = pytest.mark.gpu

PHILOX = (("momentum_rng", "philox"),)


# ---- a. the stream -------------------------------------------------------------------------------------------------------
def test_the_momentum_stream_is_the_counter_modes_and_the_models():
    """Engine.counter_draws of a momentum_rng="philox" engine at every kernel shape (d = 1: one live lane; 64 / 65: one and two
    elements per lane; 200: four; 600: a team of four wavefronts) and at iterations on both sides of 2^32: bit for bit the
    normals of an rng="counter" engine on the same seeds (both kernels call philox_normals), within 4 x
    NORMALS_MEASURED_MAX_ABS (the bound of tests/test_gpu_counter_rng.py, not re-measured) of the float64 Box-Muller of the
    same Philox words, float32-valued, exactly d columns, and no uniforms to show."""
    chains = 8
    seeds = lmc.distributed.global_seeds(SEED, chains)
    worst = 0.0
    for d in (1, 64, 65, 200, 600):
        eng = lmc.NUTS(T.StdNormal(d), d, momentum_rng="philox")._make_engine(chains)
        twin = lmc.NUTS(T.StdNormal(d), d, rng="counter")._make_engine(chains)
        try:
            assert eng.rng == "philox" and twin.rng == "counter"
            eng.seed(seeds)
            twin.seed(seeds)
            for git in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5):
                normals, none = eng.counter_draws(git)
                assert normals.shape == (chains, d) and none.shape == (chains, 0)
                np.testing.assert_array_equal(normals, twin.counter_draws(git)[0], err_msg="d=%d git=%d" % (d, git))
                assert np.all(normals == normals.astype(np.float32)) and np.all(np.isfinite(normals))
                for c in range(chains):
                    worst = max(worst, float(np.abs(normals[c] - cm.normals(seeds[c], git, d)).max()))
        finally:
            eng.close()
            twin.close()
    print("philox counter_draws normals: max |device - float64 model| = %.3e" % worst)
    assert worst <= 4.0 * NORMALS_MEASURED_MAX_ABS, worst


# ---- b. every iteration against the oracle -----------------------------------------------------------------------------------
# the counter replay's cases with its K, T and tuning split; LMC_RNG_PHILOX refuses a run-time compiled density
CASES = {name: case for name, case in COUNTER_CASES.items() if name != "user_std_normal_16"}
CASE_SEED = {name: SEED for name in CASES}       # a case whose replay skips more than the cap gets another seed here
WANT_SHAPE = {"ar1_200": (4, 1), "ar1_300": (4, 2), "diag_gaussian_600": (4, 4), "ar1_65": (2, 1), "std_normal_1": (1, 1),
              "glm_63_3_bernoulli": (1, 1), "glm_130_130_poisson": (4, 1)}    # (what the counter test lists for its cases)
TEAM_CASES = ("ar1_300", "diag_gaussian_600")
_REPLAYED = {}


def record_chains(make_ostep, start, seeds, normals, n_tune, n_it):
    """The oracle half: one chain per seed, unchanged, on MomentumOnlyRng(seed_c, normals[:, c]). Returns ([(snaps, outs)],
    uniforms consumed [K, T], twist crossed [K, T])."""
    chains, used, crossed = [], [], []
    for c, seed in enumerate(seeds):
        rng = cm.MomentumOnlyRng(seed, normals[:, c])
        chains.append(record_chain(make_ostep(), start, rng, n_tune, n_it - n_tune))
        u, x = rng.finish()
        used.append(u)
        crossed.append(x)
    return chains, np.array(used), np.array(crossed)


def _next_uniforms(state, n=4):
    """The next ``n`` doubles of the stream that continues from ``state``. (Two states are compared by these, not by their 624
    words: numpy twists lazily and the device may twist at another moment, so two word arrays can be the same stream.)"""
    rs = np.random.RandomState(0)
    rs.set_state(tuple(state))
    return rs.random_sample(n)


def _replay(name):
    """Replay every iteration of K oracle chains of case ``name`` on the device; memoised. Returns a dict of counts."""
    if name in _REPLAYED:
        return _REPLAYED[name]
    family, d, K, n_it, n_tune, kind, extra = CASES[name]
    seeds = lmc.distributed.global_seeds(CASE_SEED[name], K)
    step, make_ostep, start = _steps(family, d, kind, extra, seeds, mode=PHILOX)
    eng = step._make_engine(K)
    try:
        assert eng.rng == "philox"
        eng.seed(seeds)                      # once: the momentum stream is keyed by these seeds and nothing else
        normals = np.stack([eng.counter_draws(t)[0] for t in range(n_it)])      # [T, K, d]: the device's own normals
        chains, used, crossed = record_chains(make_ostep, start, seeds, normals, n_tune, n_it)
        for snaps, _outs in chains:          # states a team kernel accepts, and no gaussian the momentum draw would have left
            assert all(s["rng"][2] % 2 == 0 and s["rng"][3] == 0 for s in snaps)
        ran = run_keyed_iterations(step, eng, [snaps for snaps, _outs in chains], n_tune, set_rng=True)
        shape = eng.kernel_shape()
    finally:
        eng.close()
    rules = Rules.diag()
    done = [assert_replay(ran[c], snaps, outs, rules, "%s chain %d" % (name, c)) for c, (snaps, outs) in enumerate(chains)]
    # the generator after an iteration: the stream that continues from the device's state is the oracle's
    states = 0
    for c, (snaps, outs) in enumerate(chains):
        for t in range(n_it - 1):
            if rules.skips(outs[t]):
                continue
            got = ran[c][t]["rng"]
            assert got[2] == ran[c][t]["rng_pos"] and got[3] == 0, (name, c, t, got[2:])
            np.testing.assert_array_equal(_next_uniforms(got), _next_uniforms(snaps[t + 1]["rng"]),
                                          err_msg="%s chain %d: generator state after iteration %d" % (name, c, t))
            states += 1
    kept = np.array([[not rules.skips(o) for o in outs] for _snaps, outs in chains])       # [K, T] iterations compared
    res = dict(checked=sum(r.checked for r in done), skipped=sum(r.skipped for r in done), total=K * n_it,
               twists=int((crossed & kept)[:, 1:].sum()), first_twists=int((crossed & kept)[:, 0].sum()), states=states,
               max_used=int(used.max()), shape=shape, worst_q=max(r.worst_q for r in done), worst_stat=max(r.worst_stat for r in done))
    print("%s: %s" % (name, res))
    _REPLAYED[name] = dict(res, ran=ran, chains=chains)
    return _REPLAYED[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_iteration_replays_against_the_oracle(name):
    """For every iteration t of K chains: the oracle's pre-iteration state -- position, adaptation state AND MT19937 state --
    goes into ONE engine of K chains, seeded once, eng.run(n_tune, t, 1) runs iteration t, and positions, statistics, the
    adaptation state (against the oracle's next snapshot) and the generator's position equal the oracle's under
    Rules.diag(); the oracle runs UNCHANGED on MomentumOnlyRng(seed, the device's normals). The position being exact also
    says the momentum draw consumed no generator word. The stream that continues from the device's generator state after the
    iteration is the oracle's (next four doubles). An iteration whose oracle margin is below the rules' floor is skipped: at
    most max(1, 1 %) of a case. A team case replays at least one twist later than the freshly seeded generator's first."""
    res = _replay(name)
    assert res["checked"] + res["skipped"] == res["total"]
    assert res["skipped"] <= max(1, res["total"] // 100), res
    if name in WANT_SHAPE:
        assert res["shape"][1:] == WANT_SHAPE[name], res["shape"]
    assert res["first_twists"] >= 1            # iteration 0 starts from position 624
    if name in TEAM_CASES:
        assert res["shape"][2] > 1 and res["twists"] >= 1, res["twists"]


def test_replay_skips_next_to_nothing_over_all_cases():
    res = [_replay(name) for name in CASES]
    total, skipped = sum(r["total"] for r in res), sum(r["skipped"] for r in res)
    print("replayed %d iterations, %d skipped, %d twists crossed after iteration 0, %d generator states continued" % (
        total, skipped, sum(r["twists"] for r in res), sum(r["states"] for r in res)))
    assert skipped * 100 <= total, (skipped, total)


def test_another_chains_oracle_does_not_replay():
    """Negative control, on what ar1_16 already ran: the device's iterations of chain c against the oracle's outputs of chain
    (c + 1) % K -- other normals, another generator -- make assert_replay raise for every c."""
    res = _replay("ar1_16")
    ran, chains = res["ran"], res["chains"]
    K = len(chains)
    for c in range(K):
        snaps, outs = chains[(c + 1) % K]
        with pytest.raises(AssertionError, match="shifted chain %d iter" % c):
            assert_replay(ran[c], snaps, outs, Rules.diag(), "shifted chain %d" % c)


# ---- c. the driver, free-running ---------------------------------------------------------------------------------------------
DRIVER_CHAINS, DRIVER_DRAWS, DRIVER_LAUNCH, DRIVER_SOLID = 4, 40, 7, 14
# Chosen without a GPU, on the model's normals rounded to float32 (driver_margins over seeds 1 .. 199): the smallest margin of
# the first 14 iterations is 2.4e-3 (d = 70) and 1.2e-3 (d = 600). The device's normals are within 2e-6 of the model's, which
# moves an energy by ~ sqrt(d) x 2e-6 x |p| ~ 1e-5: the margins stay above 10 x FRAGILE = 1e-3 (asserted below all the same).
DRIVER_SEED = {70: 39, 600: 66}


def _driver_steps(d):
    var = np.full(d, 1.3)
    step = lmc.NUTS(T.StdNormal(d), d, scaling=var, is_cov=True, adapt_step_size=False, momentum_rng="philox")
    ostep = lambda: orc.Step(OT.make("std_normal", d), d, kind="nuts", scaling=var, is_cov=True, adapt_step_size=False)   # noqa: E731
    return step, ostep


def driver_oracle(d, seeds, normals):
    """Free-running oracle chains of the driver test on MomentumOnlyRng: [(snaps, outs)] per chain."""
    start = orc.jitter_start(seeds[0], d)
    ostep = _driver_steps(d)[1]
    return start, [record_chain(ostep(), start, cm.MomentumOnlyRng(seeds[c], normals[:, c]), 0, DRIVER_DRAWS)
                   for c in range(len(seeds))]


def driver_margins(chains, n=DRIVER_SOLID):
    """The smallest oracle margin (multinomial / Metropolis, U-turn) over the first ``n`` iterations of every chain."""
    return min(min(o["lb"], o["turn"]) for _snaps, outs in chains for o in outs[:n])


@pytest.mark.parametrize("d", [70, 600])
def test_the_driver_free_runs_with_the_oracle_across_launches(d):
    """lmc.sample(..., tune=0, draws=40, launch_iters=7) under momentum_rng="philox" with a fixed diagonal and a fixed step
    size (nothing adapts: the chains are not chaotic) against oracle chains that free-run on MomentumOnlyRng with the
    device's normals (a second engine on the same seeds): tests/_gpu_util.assert_chain_matches with the oracle's margins,
    which demands a reason for the first difference. The seeds are such that no margin of the first 14 iterations is below
    10 x FRAGILE, and every chain must verify at least those 14: two launch boundaries, i.e. two round trips of the
    generator state through HBM with no momentum draw in between. d = 70: one wavefront, NS = 2; d = 600: a team of four."""
    chains = DRIVER_CHAINS
    seeds = lmc.distributed.global_seeds(DRIVER_SEED[d], chains)
    step, _ostep = _driver_steps(d)
    eng = _driver_steps(d)[0]._make_engine(chains)
    try:
        assert eng.rng == "philox"
        eng.seed(seeds)
        normals = np.stack([eng.counter_draws(t)[0] for t in range(DRIVER_DRAWS)])
    finally:
        eng.close()
    start, ochains = driver_oracle(d, seeds, normals)
    assert driver_margins(ochains) >= 10 * FRAGILE, driver_margins(ochains)
    trace, stats = lmc.sample(T.StdNormal(d), d, chains=chains, tune=0, draws=DRIVER_DRAWS, launch_iters=DRIVER_LAUNCH,
                              random_seed=seeds, start=start, step=step)
    assert trace.shape == (chains, DRIVER_DRAWS, d)
    verified = []
    for c, (_snaps, outs) in enumerate(ochains):
        want_q = np.array([o["q"] for o in outs])
        names = [k for k in outs[0]["stats"] if k in stats]
        assert "tree_size" in names and "depth" in names and "energy" in names
        want = {k: np.array([o["stats"][k] for o in outs]) for k in names}
        got = {k: np.asarray(stats[k])[c].reshape(DRIVER_DRAWS) for k in names}
        margins = np.array([[o["lb"], o["turn"], o["div"]] for o in outs])
        verified.append(assert_chain_matches(trace[c], got, want_q, want, margins, label="philox driver d=%d chain %d" % (d, c)))
    print("philox driver d=%d: iterations verified per chain %s of %d" % (d, verified, DRIVER_DRAWS))
    assert min(verified) >= DRIVER_SOLID, verified
