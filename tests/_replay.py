"""The teacher-forced replay, once: every iteration of an oracle chain is run on the device from the oracle's exact
pre-iteration state and compared with what the oracle computed from it.

    record_chain      the oracle half: one chain, per iteration the state before it (snapshot) and what came out (output)
    Rules             what a comparison asserts -- THE table of tolerances, skip floors and margins; nothing else states them
    run_snapshots     the device half: one chain per snapshot, one iteration everywhere, everything read back
    run_keyed_iterations   the device half for a stream keyed by (seed, iteration): K seeded chains, iteration t in one launch
    iteration_errors  one iteration against the rules, pure numpy
    assert_replay     the loop: skip by the rules' margin, raise on the first iteration with an error, count the rest

Running and comparing are separate, so a comparison that fails leaves the device's results with the caller."""
import collections
import dataclasses

import numpy as np

from tests._gpu_util import INT_STATS

REPLAY_F32 = 1e-5   # one whole transition started from a float32-born momentum (observed: 6e-7 positions, 3e-6 stats)
REPLAY_F64 = 1e-11
DECISION = 1e-4     # smallest oracle decision margin that must reproduce when the momentum is float32-born

_CHAIN_KEYS = ("log_step", "log_bar", "hbar", "da_count", "iter_count", "n_samples")
_WELFORD_VECTORS = ("fore_mean", "fore_raw_var", "back_mean", "back_raw_var")
_WELFORD_KEYS = _WELFORD_VECTORS + ("fore_w_sum", "back_w_sum", "window")
_DENSE_KEYS = ("cov", "chol", "fore_mean", "fore_raw_cov", "fore_n", "back_mean", "back_raw_cov", "back_n", "window",
               "previous_update")


# ---- 1. the oracle half -------------------------------------------------------------------------------------------------
def chain_iterations(ostep, tune, n, after_reset=None):
    """The chain driver's switching around ``n`` iterations of ``ostep`` (sampling.py:481-521 of the reference): yields i
    with the step ready to take iteration i. The caller takes it. ``after_reset(ostep)`` is called once, right after
    reset_tuning() and before the first iteration: a chain that starts from a state no short chain reaches."""
    ostep.tune = bool(tune)
    ostep.reset_tuning()
    if after_reset is not None:
        after_reset(ostep)
    for i in range(n):
        if i == 0:
            ostep.iter_count = 0
        if i == tune:
            ostep.tune = False
        yield i


def record_chain(ostep, start, rng, tune, draws, after_reset=None):
    """Run one oracle chain on ``rng`` (np.random.RandomState(seed), or _counter_model.CounterRng); return (snaps, outs) per
    iteration. An output carries all three oracle margins; which of them count for skipping is the rules' business.
    ``after_reset``: chain_iterations' hook."""
    from oracle import lmc_oracle as orc

    has_state = hasattr(rng, "get_state")
    q = np.array(start, dtype="d")
    snaps, outs = [], []
    for _i in chain_iterations(ostep, tune, tune + draws, after_reset):
        pot, ad = ostep.pot, ostep.adapt
        snap = dict(q=q.copy(), tune=ostep.tune, iter_count=ostep.iter_count, log_step=float(np.ravel(ad.log_step)[0]),
                    log_bar=float(np.ravel(ad.log_bar)[0]), hbar=float(np.ravel(ad.hbar)[0]), da_count=ad.count,
                    n_samples=getattr(pot, "n_samples", 0))
        if has_state:
            snap["rng"] = rng.get_state()
        if hasattr(pot, "var"):
            snap["var"] = pot.var.copy()
        if isinstance(pot, orc.DiagAdaptPotential):
            snap.update(fore_mean=pot.fore.mean.copy(), fore_raw_var=pot.fore.raw_var.copy(), fore_w_sum=pot.fore.w_sum,
                        back_mean=pot.back.mean.copy(), back_raw_var=pot.back.raw_var.copy(), back_w_sum=pot.back.w_sum,
                        window=pot.window)
        if isinstance(pot, orc.FullAdaptPotential):
            snap.update(cov=pot.cov.copy(), chol=pot.chol.copy(), fore_mean=pot.fore.mean.copy(),
                        fore_raw_cov=pot.fore.raw.copy(), fore_n=pot.fore.n_samples, back_mean=pot.back.mean.copy(),
                        back_raw_cov=pot.back.raw.copy(), back_n=pot.back.n_samples, window=pot.window,
                        previous_update=pot.previous_update)
        q, st = ostep.astep(q, rng)
        m = ostep.last_margins
        out = dict(q=q.copy(), stats={k: np.ravel(v)[0] for k, v in st.items()}, lb=m.lb, turn=m.turn, div=m.div)
        if has_state:
            out["rng_pos"] = rng.get_state()[2]
        snaps.append(snap)
        outs.append(out)
    return snaps, outs


# ---- 2. what a comparison asserts ---------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Rules:
    """A comparison of one device iteration with the oracle's. (rtol, atol) pairs are np.isclose's; integer statistics and
    the generator's position (where recorded) are exact under every rule.

                        Rules.diag()                Rules.dense(tol, floor, da_atol, dense_state)
    skip: min of        lb, turn  < 1e-9            lb, turn, div  < floor
    float statistics    1e-10, 1e-10                tol, tol * (1 + |energy|)
    positions           1e-11, 1e-12                tol, tol * (1 + max |q|)
    after the iteration, against the oracle's next snapshot:
    dual averaging      1e-11, 1e-13                tol, and "tol": tol
                                                         "gain": tol * (1 + |energy|) * (1 + sqrt(max(da_count, 1)) / 0.05)
    da_count, n_samples equal                       equal
    var                 2e-7, 0 (var64: 1e-12, 0)   --
    and, where the next snapshot is in the same phase (tuning / sampling):
    Welford vectors     1e-11, 1e-13                --
    w_sum, window       equal                       --
    cov                 --                          0, 2 * tol * max |cov|
    under "all": chol   --                          0, 10 * tol * sqrt(max |cov|)
      window, previous_update, fore_n, back_n       equal

    "gain": the accept statistic is compared at tol * (1 + |energy|) (a float32-born start energy moves it by a few float32
    ulps of the kinetic energy); hbar averages it and log_step = mu - sqrt(t) / gamma * hbar (step_sizes.py, gamma = 0.05)
    carries it with that gain. "all" is what the golden dense chains were measured at (tests/test_gpu_dense.py) and is
    confined to them."""
    margins: tuple
    floor: float
    stat: tuple
    q: tuple
    da: tuple
    scaled: bool = False        # atol of statistics times 1 + |energy|, of positions times 1 + max |q|
    da_gain: bool = False
    var: tuple = None           # rtol of the float32 diagonal, of the float64 one; None: no diagonal state
    welford: tuple = None
    cov_tol: float = None       # None: no dense state
    dense_state: str = "cov"

    @classmethod
    def diag(cls):
        return cls(margins=("lb", "turn"), floor=1e-9, stat=(1e-10, 1e-10), q=(1e-11, 1e-12), da=(1e-11, 1e-13),
                   var=(2e-7, 1e-12), welford=(1e-11, 1e-13))

    @classmethod
    def dense(cls, tol, floor, da_atol="gain", dense_state="cov"):
        assert da_atol in ("gain", "tol") and dense_state in ("cov", "all")
        return cls(margins=("lb", "turn", "div"), floor=floor, stat=(tol, tol), q=(tol, tol), da=(tol, tol), scaled=True,
                   da_gain=da_atol == "gain", cov_tol=tol, dense_state=dense_state)

    def margin(self, out):
        """The oracle margin an iteration is skipped by."""
        return min(out[m] for m in self.margins)

    def skips(self, out):
        return self.margin(out) < self.floor

    @property
    def dense_fields(self):
        """The dense state the comparison reads back (the matrices are chains x d x d)."""
        return ("cov",) if self.dense_state == "cov" else ("cov", "chol", "window", "previous_update", "fore_n", "back_n")


def dense_rules(f32_born, **kw):
    """The dense rules every family is replayed at: REPLAY_F32 / DECISION where the momentum is float32-born
    (QuadPotentialFull, adapt_full), REPLAY_F64 / 1e-9 otherwise (QuadPotentialFullInv, dtype="float64")."""
    return Rules.dense(REPLAY_F32, DECISION, **kw) if f32_born else Rules.dense(REPLAY_F64, 1e-9, **kw)


# ---- 3. the device half -------------------------------------------------------------------------------------------------
class DeviceIterations:
    """What the device computed, per oracle iteration index i: self[i] = dict(q, stats, after, dense, rng_pos, rng, tune) --
    ``after`` the chain state and ``dense`` the dense state after the iteration (None where not read), ``rng`` the whole
    generator state after it (get_rng_state's tuple; None where not read) and ``rng_pos`` its position, ``tune`` the phase the
    iteration ran in. ``engines``: per engine, the kernel that ran (plan, leaf, wide, kind, dense, shape, mass_f64)."""

    def __init__(self, n):
        self.iterations = [None] * n
        self.engines = []

    def __getitem__(self, i):
        return self.iterations[i]

    def put(self, i, c, tune, q, stats, after, dense=None, rng_pos=None, rng=None):
        """Iteration i is chain c of what one engine returned."""
        pick = lambda arrays: None if arrays is None else {k: v[c] for k, v in arrays.items()}   # noqa: E731
        self.iterations[i] = dict(q=q[c].copy(), stats=pick(stats), after=pick(after), dense=pick(dense), rng_pos=rng_pos,
                                  rng=rng, tune=tune)

    @property
    def q(self):
        return np.stack([it["q"] for it in self.iterations if it is not None])

    def kernels(self, key):
        return {e[key] for e in self.engines}


def engine_report(eng):
    return dict(plan=eng.last_run_plan(), leaf=eng.last_run_leaf_group(), wide=eng.wide, kind=eng.kind,
                dense=eng.last_run_dense_kernel(), shape=eng.kernel_shape(), mass_f64=eng.mass_f64)


def chain_state_of(snaps, mass_f64):
    """The chain state of one engine whose chain c starts from snaps[c] (Engine.set_chain_state)."""
    keys = _CHAIN_KEYS + (("var",) if "var" in snaps[0] else ()) + (_WELFORD_KEYS if "fore_raw_var" in snaps[0] else ())
    state = {k: np.stack([np.asarray(s[k]) for s in snaps]) for k in keys}
    if mass_f64 and "var" in state:   # QuadPotentialDiagAdapt(dtype="float64"): the diagonal travels in its own dtype
        state["var64"] = state.pop("var")
    return state


def run_snapshots(step, snaps, dense_fields=("cov",)):
    """One chain per snapshot, the tuning and the sampling snapshots in two engines; ONE iteration everywhere. Compares nothing."""
    ran = DeviceIterations(len(snaps))
    for tune_flag in (True, False):
        idx = [i for i, s in enumerate(snaps) if s["tune"] == tune_flag]
        if not idx:
            continue
        mine = [snaps[i] for i in idx]
        eng = step._make_engine(len(idx))
        try:
            eng.set_position(np.stack([s["q"] for s in mine]))
            for c, s in enumerate(mine):
                eng.set_rng_state(c, s["rng"])
            eng.set_chain_state(chain_state_of(mine, eng.mass_f64))
            if "cov" in mine[0]:
                eng.set_dense_state({k: np.stack([np.asarray(s[k]) for s in mine]) for k in _DENSE_KEYS})
            eng.reserve(1, keep_trace=True)
            eng.run(1 if tune_flag else 0, 0, 1)
            assert not eng.status().any()
            ran.engines.append(engine_report(eng))
            q = eng.trace()[:, 0]
            stats = {k: v[:, 0] for k, v in step._stats_from_engine(eng, 0, 1).items()}
            after = eng.get_chain_state()
            dense = eng.get_dense_state(fields=dense_fields) if "cov" in mine[0] else None
            for c, i in enumerate(idx):
                ran.put(i, c, tune_flag, q, stats, after, dense, eng.get_rng_state(c)[2])
        finally:
            eng.close()
    return ran


def run_keyed_iterations(step, eng, chain_snaps, n_tune, set_rng=False):
    """The device half for a stream keyed by (seed, iteration) (rng="counter", momentum_rng="philox"; run_snapshots is the
    MT19937 one): the K seeded chains of ``eng`` take iteration t of every chain in ONE launch, eng.run(n_tune, t, 1), each
    from its own snapshot chain_snaps[c][t]. ``set_rng``: the chain's MT19937 state is set from the snapshot before the
    launch (the momentum-only mode: the uniforms are the generator's). The generator state after the launch is kept next
    to ``after``, whole and as a position. Returns one DeviceIterations per chain; compares nothing."""
    n_it = len(chain_snaps[0])
    ran = [DeviceIterations(n_it) for _ in chain_snaps]
    eng.reserve(n_it, keep_trace=True)
    for t in range(n_it):
        now = [snaps[t] for snaps in chain_snaps]
        eng.set_position(np.stack([s["q"] for s in now]))
        if set_rng:
            for c, s in enumerate(now):
                eng.set_rng_state(c, s["rng"])
        eng.set_chain_state(chain_state_of(now, eng.mass_f64))
        eng.run(n_tune, t, 1)
        assert not eng.status().any()
        q = eng.trace(t, 1)[:, 0]
        stats = {k: v[:, 0] for k, v in step._stats_from_engine(eng, t, 1).items()}
        after = eng.get_chain_state()
        for c, s in enumerate(now):
            rng = eng.get_rng_state(c)
            ran[c].put(t, c, s["tune"], q, stats, after, rng_pos=rng[2], rng=rng)
    for r in ran:
        r.engines.append(engine_report(eng))
    return ran


# ---- 4. comparing -------------------------------------------------------------------------------------------------------
def _off(errors, name, got, want, rtol, atol):
    """Where an element is outside |got - want| <= atol + rtol * |want|, append (name, got, want) of the one furthest off;
    return the largest error in units of that tolerance over the finite elements of ``want``."""
    got, want = np.asarray(got, dtype="d"), np.asarray(want, dtype="d")
    bad = ~np.isclose(got, want, rtol=rtol, atol=atol, equal_nan=got.ndim > 0)   # (np.testing.assert_allclose's nan rule)
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(np.isfinite(want), np.abs(got - want) / (atol + rtol * np.abs(want)), 0.0)
    if bad.any():
        j = np.unravel_index(np.argmax(np.where(bad, np.abs(got - want), -1.0)), bad.shape)
        errors.append((name, got[j], want[j]))
    return float(np.max(np.nan_to_num(units, nan=0.0))) if units.size else 0.0


def _differs(errors, name, got, want):
    if got != want:
        errors.append((name, got, want))


def iteration_errors(got, want, nxt, rules):
    """One iteration: ``got`` a DeviceIterations entry, ``want`` the oracle's output, ``nxt`` the oracle's next snapshot
    (None: the state after the iteration is not compared). Returns (errors, q_err, stat_err): the violated comparisons as
    (name, got, want), and the largest position / float statistic error in units of its tolerance."""
    errors, stat_err = [], 0.0
    escale = 1 + abs(want["stats"].get("energy", 0.0)) if rules.scaled else 1.0
    for name, val in want["stats"].items():
        if name in INT_STATS:
            _differs(errors, name, got["stats"][name], val)
        else:
            stat_err = max(stat_err, _off(errors, name, got["stats"][name], val, rules.stat[0], rules.stat[1] * escale))
    qscale = 1 + np.abs(want["q"]).max() if rules.scaled else 1.0
    q_err = _off(errors, "q", got["q"], want["q"], rules.q[0], rules.q[1] * qscale)
    if "rng_pos" in want:
        _differs(errors, "rng_pos", got["rng_pos"], want["rng_pos"])
    if nxt is None:
        return errors, q_err, stat_err
    after, dense = got["after"], got.get("dense")
    if rules.var is not None:
        _off(errors, "var", after["var"], nxt["var"], rules.var[0], 0.0)
        if "var64" in after:      # the engine's diagonal is float64
            _off(errors, "var64", after["var64"], nxt["var"], rules.var[1], 0.0)
    da_atol = rules.da[1]
    if rules.da_gain:
        da_atol *= escale * (1.0 + np.sqrt(max(float(nxt["da_count"]), 1.0)) / 0.05)
    for k in ("log_step", "log_bar", "hbar"):
        _off(errors, k, after[k], nxt[k], rules.da[0], da_atol)
    for k in ("da_count", "n_samples"):
        _differs(errors, k, after[k], nxt[k])
    if nxt["tune"] != got["tune"]:
        return errors, q_err, stat_err
    if rules.welford is not None and "fore_raw_var" in nxt:
        for k in _WELFORD_VECTORS:
            _off(errors, k, after[k], nxt[k], *rules.welford)
        for k in ("fore_w_sum", "back_w_sum", "window"):
            _differs(errors, k, after[k], nxt[k])
    if rules.cov_tol is not None and dense is not None:
        cs = np.abs(nxt["cov"]).max()
        _off(errors, "cov", dense["cov"], nxt["cov"], 0.0, 2 * rules.cov_tol * cs)
        if rules.dense_state == "all":
            _off(errors, "chol", dense["chol"], nxt["chol"], 0.0, 10 * rules.cov_tol * np.sqrt(cs))
            for k in ("window", "previous_update", "fore_n", "back_n"):
                _differs(errors, k, dense[k], nxt[k])
    return errors, q_err, stat_err


Replayed = collections.namedtuple("Replayed", "checked skipped worst_q worst_stat")


def assert_replay(ran, snaps, outs, rules, label="", skip=None):
    """Every iteration of ``ran`` against the oracle's under ``rules``. An iteration whose oracle margin is below the rules'
    floor, or for which ``skip(i)`` names a reason, is not compared. Raises AssertionError on the first iteration that
    violates a comparison; returns Replayed(checked, skipped, worst_q, worst_stat), the worst errors in units of the tolerance."""
    checked = skipped = 0
    worst_q = worst_stat = 0.0
    for i, want in enumerate(outs):
        if rules.skips(want) or (skip is not None and skip(i)):
            skipped += 1
            continue
        errors, q_err, stat_err = iteration_errors(ran[i], want, snaps[i + 1] if i + 1 < len(snaps) else None, rules)
        assert not errors, ("%s iter %d" % (label, i), errors, "margin %g" % rules.margin(want))
        worst_q, worst_stat = max(worst_q, q_err), max(worst_stat, stat_err)
        checked += 1
    return Replayed(checked, skipped, worst_q, worst_stat)


def replay_chain(ostep, step, start, seed, tune, draws, rules, label, skip=None):
    """The three pieces in a row for a caller that needs nothing in between: the oracle chain on MT19937(seed), the device's
    iterations, the comparison. Returns assert_replay's counts."""
    snaps, outs = record_chain(ostep, start, np.random.RandomState(int(seed)), tune, draws)
    return assert_replay(run_snapshots(step, snaps, rules.dense_fields), snaps, outs, rules, label, skip)
