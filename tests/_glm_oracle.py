"""targets.GLM for the oracle (oracle/lmc_oracle.py takes any callable f(q) -> (logp, g)): the float64 statement of the
posterior in the device's operation order (tests/_glm_model.logp_grad -- the order is stated there and nowhere else), an
independent statement of the same posterior in extended precision and BLAS order, the table of cells that
tests/test_gpu_glm_replay.py replays on the device and tests/test_glm_replay_cpu.py holds to the second statement, and the
oracle chains of those cells, computed once per process.

No device is touched at import: the device target of a cell is built when ``target()`` is called."""
import collections
import functools

import numpy as np

from tests import _glm_model as M

TAU, ISIG2 = M.PRIOR_SCALE ** -2, M.SIGMA ** -2
SEEDS_FROM, CHAIN = 4321, 1          # the diagonal chains: seeds derive_seeds(4321, 2), chain 1 (start: jitter of seeds[0])


# ---- the two statements of the posterior -----------------------------------------------------------------------------------
def oracle_glm(N, d, lik):
    """(f, target, start_info): ``f(q) -> (np.float64 logp, g[d])`` in the device's order on M.case(N, d, lik); ``target()``
    builds the matching targets.GLM when called; ``start_info`` = dict(N, d, lik, X, y, tau, isig2)."""
    X, y, _ = M.case(N, d, lik)

    def f(q):
        logp, g = M.logp_grad(X, y, q, lik, TAU, ISIG2)
        return np.float64(logp), g

    def target():
        from littlemcmc_amd import targets as T

        return T.GLM(X, y, lik, prior_scale=M.PRIOR_SCALE, sigma=M.SIGMA)

    return f, target, dict(N=N, d=d, lik=lik, X=X, y=y, tau=TAU, isig2=ISIG2)


def _link_longdouble(eta, y, lik):
    """(l, r) per observation in np.longdouble, written from the definitions (targets.GLM's docstring), not from
    tests/_glm_model.link: softplus by logaddexp, sigmoid by a division."""
    one = np.longdouble(1.0)
    if lik == "bernoulli":
        return y * eta - np.logaddexp(np.longdouble(0.0), eta), y - one / (one + np.exp(-eta))
    if lik == "poisson":
        with np.errstate(over="ignore", invalid="ignore"):
            mu = np.exp(eta)
            return y * eta - mu, y - mu
    res = y - eta
    return -(res * res) * np.longdouble(ISIG2) / 2, res * np.longdouble(ISIG2)


def oracle_glm_longdouble(N, d, lik, mutant=None):
    """The independent statement: np.longdouble, ``X @ q`` and ``X.T @ r`` in numpy's own order, rounded to float64 at the
    end. ``mutant``: one of MUTANTS, a deliberately wrong posterior (what the replay tolerance must tell from the right one)."""
    X, y, _ = M.case(N, d, lik)
    Xl, yl, tau = X.astype(np.longdouble), y.astype(np.longdouble), np.longdouble(TAU)

    def f(q):
        ql = np.asarray(q, dtype=np.longdouble)
        with np.errstate(over="ignore", invalid="ignore"):
            eta = Xl @ ql
            lo, r = _link_longdouble(eta, yl, lik)
            if mutant == "g_last_observation":
                r = r.copy()
                r[-1] *= np.longdouble(1.0) + np.longdouble(1e-8)
            prior_q = ql
            if mutant == "prior_last_coefficient":
                prior_q = ql.copy()
                prior_q[-1] *= np.longdouble(1.0) + np.longdouble(1e-6)
            g = Xl.T @ r - tau * prior_q
            logp = lo.sum() - tau / 2 * (ql @ prior_q)
            if mutant == "logp_scaled":
                logp = logp * (np.longdouble(1.0) + np.longdouble(1e-9))
        return np.float64(logp), g.astype(np.float64)

    return f


# the issue's three small errors: the last observation's term of g scaled by 1 + 1e-8, logp scaled by 1 + 1e-9, the prior
# term of the last coefficient off by 1e-6 relative
MUTANTS = ("g_last_observation", "logp_scaled", "prior_last_coefficient")


def hessian_at_zero(N, d, lik):
    """Hessian of -logp at q = 0: X' W X + tau I with W = -dr/deta at eta = 0 (1/4, 1, 1/sigma^2)."""
    X, _, _ = M.case(N, d, lik)
    w = {"bernoulli": 0.25, "poisson": 1.0, "gaussian": ISIG2}[lik]
    h = w * (X.T @ X) + TAU * np.eye(d)
    return 0.5 * (h + h.T)


def mass_matrix(N, d, lik):
    """The dense cases' mass matrix: the inverse of hessian_at_zero, symmetrised."""
    c = np.linalg.inv(hessian_at_zero(N, d, lik))
    return 0.5 * (c + c.T)


# ---- the table ----------------------------------------------------------------------------------------------------------
# kind: "diag"     init_nuts' float32 adapted diagonal (fused one-wave kernels to d = 256, the general ones beyond)
#       "diag64"   QuadPotentialDiagAdapt(dtype="float64"): the general one-wave kernels at every NS
#       "hmc"      HamiltonianMC(path_length=1.0), float32 adapted diagonal
#       "full"     QuadPotentialFull(mass_matrix)                    float32-born momentum: REPLAY_F32 / DECISION
#       "full64"   QuadPotentialFull(mass_matrix, dtype="float64")
#       "inv"      QuadPotentialFullInv(hessian_at_zero)             the same metric, given as the precision
#       "adapt"    init="adapt_full"                                 float32-born
# seed: the chain's seed for the dense kinds (the diagonal kinds use SEEDS_FROM / CHAIN); chosen, as the issue asks, so that
# at most two iterations of the oracle chain have a margin below the skip floor (test_glm_replay_cpu.py asserts it)
Case = collections.namedtuple("Case", "kind N d lik tune draws seed")
F32_BORN = ("full", "adapt")
DENSE = ("full", "full64", "inv", "adapt")

_FUSED_SHAPES = ((1, 1), (63, 3), (64, 64), (65, 65), (130, 130), (70, 256))
_ALL_LIKS = ((63, 3), (65, 65), (130, 130))


def _diag(N, d, lik, tune=40, draws=8, kind="diag"):
    return Case(kind, N, d, lik, tune, draws, None)


def _dense(kind, N, d, lik, seed):
    return Case(kind, N, d, lik, 13, 6, seed)


FUSED = tuple(_diag(N, d, lik) for N, d in _FUSED_SHAPES
              for lik in (M.LIKELIHOODS if (N, d) in _ALL_LIKS else ("bernoulli",)))
WIDE = (_diag(70, 300, "bernoulli", 24, 6), _diag(70, 300, "poisson", 24, 6), _diag(65, 512, "bernoulli", 24, 6),
        _diag(70, 257, "bernoulli", 24, 6))
DIAG64 = tuple(_diag(N, d, "bernoulli", kind="diag64") for N, d in _ALL_LIKS)
HMC = (_diag(63, 3, "bernoulli", kind="hmc"), _diag(65, 65, "poisson", kind="hmc"))
SHARED = (_dense("full", 63, 3, "bernoulli", 7003), _dense("full", 65, 65, "bernoulli", 7065),
          _dense("full", 130, 128, "bernoulli", 7128))
PER_CHAIN = tuple(_dense(kind, N, d, lik, 8000 + d) for kind in ("full", "full64", "inv")
                  for N, d, lik in ((65, 65, "poisson"), (130, 130, "gaussian")))
ADAPT = (_dense("adapt", 63, 3, "bernoulli", 9003),)
CASES = FUSED + WIDE + DIAG64 + HMC + SHARED + PER_CHAIN + ADAPT


def case_id(c):
    return "%s-%d-%d-%s" % (c.kind, c.N, c.d, c.lik)


def diag_seeds():
    from oracle import lmc_oracle as orc

    return orc.derive_seeds(SEEDS_FROM, 2)


def oracle_step(c, f=None):
    """(oracle step, start, chain seed) of case ``c`` on ``f`` (default: the device-order statement)."""
    from oracle import lmc_oracle as orc

    if f is None:
        f = oracle_glm(c.N, c.d, c.lik)[0]
    d = c.d
    if c.kind in ("diag", "diag64", "hmc"):
        seeds = diag_seeds()
        start = orc.jitter_start(seeds[0], d)
        if c.kind == "diag":
            s0, ostep = orc.init_nuts(f, d, seeds=seeds)
            np.testing.assert_array_equal(s0, start)
        elif c.kind == "diag64":
            ostep = orc.Step(f, d, kind="nuts", potential=orc.DiagAdaptPotential(d, start, np.ones(d), 10, dtype="float64"))
        else:
            ostep = orc.Step(f, d, kind="hmc", path_length=1.0, potential=orc.DiagAdaptPotential(d, np.zeros(d), np.ones(d), 10))
        return ostep, start, seeds[CHAIN]
    if c.kind == "adapt":
        start, ostep = orc.init_nuts(f, d, init="adapt_full", seeds=[c.seed])
        return ostep, start, c.seed
    if c.kind == "full":
        pot = orc.quad_potential(mass_matrix(c.N, d, c.lik), True)
    elif c.kind == "full64":
        pot = orc.FullPotential(mass_matrix(c.N, d, c.lik), dtype="float64")
    else:
        pot = orc.quad_potential(hessian_at_zero(c.N, d, c.lik), False)
    return orc.Step(f, d, kind="nuts", potential=pot), 0.5 * np.random.RandomState(c.seed).randn(d), c.seed


def device_step(c, target=None, **kw):
    """The device step of case ``c`` (``kw``: lds_plan for the fused kernels) and its start. ``target``: another device
    target than the cell's own (a deliberately wrong one)."""
    import littlemcmc_amd as lmc
    from oracle import lmc_oracle as orc

    tgt, d = oracle_glm(c.N, c.d, c.lik)[1]() if target is None else target, c.d
    if c.kind in ("diag", "diag64", "hmc"):
        seeds = diag_seeds()
        start = orc.jitter_start(seeds[0], d)
        if c.kind == "diag":
            s0, step = lmc.init_nuts(tgt, d, random_seed=seeds, **kw)
            np.testing.assert_array_equal(s0, start)
        elif c.kind == "diag64":
            step = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialDiagAdapt(d, start, np.ones(d), 10, dtype="float64"), **kw)
        else:
            step = lmc.HamiltonianMC(tgt, d, path_length=1.0, **kw)
        return step, start
    if c.kind == "adapt":
        np.random.seed(c.seed)
        start, step = lmc.init_nuts(tgt, d, init="adapt_full", random_seed=[c.seed], **kw)
        return step, start
    if c.kind == "full":
        pot = lmc.QuadPotentialFull(mass_matrix(c.N, d, c.lik))
    elif c.kind == "full64":
        pot = lmc.QuadPotentialFull(mass_matrix(c.N, d, c.lik), dtype="float64")
    else:
        pot = lmc.QuadPotentialFullInv(hessian_at_zero(c.N, d, c.lik))
    return lmc.NUTS(tgt, d, potential=pot, **kw), 0.5 * np.random.RandomState(c.seed).randn(d)


@functools.lru_cache(maxsize=None)
def oracle_chain(c):
    """(snaps, outs) of case ``c``'s oracle chain (tests/_replay.record_chain), computed once per process and shared by every
    variant that replays it; nothing in it is modified afterwards."""
    from tests._replay import record_chain

    ostep, start, seed = oracle_step(c)
    snaps, outs = record_chain(ostep, start, np.random.RandomState(int(seed)), c.tune, c.draws)
    for o in outs:
        o["q"].setflags(write=False)
    return snaps, outs


def rules(c):
    """What the replay of case ``c`` asserts, the margin and the floor it skips an iteration by included (tests/_replay.Rules)."""
    from tests._replay import Rules, dense_rules

    return dense_rules(c.kind in F32_BORN) if c.kind in DENSE else Rules.diag()
