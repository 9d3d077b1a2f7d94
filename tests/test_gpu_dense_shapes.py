"""-m gpu: the two dense kernels across their shapes, against the oracle (tests/test_gpu_dense.py holds the captured cases).

run_dense_coop_kernel (QuadPotentialFull up to model_ndim 128: eight chains per workgroup, the float32 matrix in LDS, every
velocity from v_mfma_f64_16x16x4_f64, lmc_dense.hpp: coop_product) and run_dense_kernel (one chain per wavefront) are
replayed iteration by iteration from the oracle's exact pre-iteration state at every shape where their loops change: one or
two elements per lane, one to eight 16-row k-blocks, full and partial last blocks and tiles, workgroups with idle waves.

* The sweep compares with the oracle at the reference's own tolerances (tests/test_gpu_dense.py: REPLAY_F32 for a float32
  momentum, REPLAY_F64 otherwise).
* The contract replay compares the shared-matrix kernel with a host model of the operation it documents, in float64 /
  extended precision, to 1e-10: a float32 operand panel or accumulator, or a momentum solved in float32, fails it where the
  reference tolerance (1e-5) cannot see it.
* The placement knobs (LMC_DENSE_COOP, LMC_DENSE_LDS_SLOTS, LMC_DENSE_CACHE_ROWS, LMC_SUB_BLOCKS) leave results bit for bit.
"""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd._blas_probe import emulate_sdot
from oracle import lmc_oracle as orc
from oracle import targets as otargets
from tests._gpu_util import INT_STATS
from tests._replay import DECISION, REPLAY_F32, Rules, assert_replay, dense_rules, record_chain, run_snapshots

pytestmark = pytest.mark.gpu

CONTRACT = 1e-10           # host model of the shared-matrix kernel: float64 products on both sides, reduction order only
SHARED_D = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 97, 127, 128]   # NS 1 / 2; 1..8 k-blocks of 16 rows, full and partial
TUNE, DRAWS = 13, 6        # two engines of 13 and 6 chains: the last workgroup of eight has idle waves
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spd(d, seed, lo=-1.0, hi=1.0):
    """Random SPD matrix with eigenvalues 10^lo .. 10^hi (condition 1e2 by default) and real off-diagonal mass."""
    rs = np.random.RandomState(seed)
    qm, _ = np.linalg.qr(rs.randn(d, d))
    m = (qm * np.logspace(lo, hi, d)) @ qm.T
    return 0.5 * (m + m.T)


def _ar1_cov(d, rho=0.9):
    idx = np.arange(d)
    return rho ** np.abs(idx[:, None] - idx[None, :])


def _steps(d, kind, pot_kind, mat):
    """(oracle step, device step) on the AR(1) target with the mass matrix ``mat``."""
    of = otargets.make("ar1", d)
    tgt = lmc.targets.AR1(d)
    if pot_kind == "full64":
        opot, dpot = orc.FullPotential(mat, dtype="float64"), lmc.QuadPotentialFull(mat, dtype="float64")
    elif pot_kind == "inv":
        opot, dpot = orc.quad_potential(mat, False), lmc.QuadPotentialFullInv(mat)
    else:
        opot, dpot = orc.quad_potential(mat, True), lmc.QuadPotentialFull(mat)
    cls = lmc.HamiltonianMC if kind == "hmc" else lmc.NUTS
    return orc.Step(of, d, kind=kind, potential=opot), cls(tgt, d, potential=dpot)


def _sweep(d, kind, pot_kind, mat, expect, seed, label):
    ostep, dstep = _steps(d, kind, pot_kind, mat)
    start = 0.5 * np.random.RandomState(seed).randn(d)
    snaps, outs = record_chain(ostep, start, np.random.RandomState(seed), TUNE, DRAWS)
    ran = run_snapshots(dstep, snaps)
    assert ran.kernels("dense") == {expect}, (label, ran.engines)
    res = assert_replay(ran, snaps, outs, dense_rules(pot_kind == "full"), label)
    print("%s: checked %d skipped %d of %d; worst position %.3g / stat %.3g of the tolerance" % (
        label, res.checked, res.skipped, TUNE + DRAWS, res.worst_q, res.worst_stat))
    assert res.checked >= TUNE + DRAWS - 2, res


# ---------------------------------------------------------------------------------------------------
# a. shape sweep at the reference's tolerances
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", SHARED_D)
def test_shared_matrix_kernel_nuts_replays_the_oracle(d):
    _sweep(d, "nuts", "full", _spd(d, 100 + d), "shared", 5000 + d, "shared nuts d=%d" % d)


def test_shared_matrix_kernel_on_the_benchmark_matrix():
    """The benchmark's case (bench.py --mass full): AR(1) target, its own covariance as the mass matrix, d = 128."""
    _sweep(128, "nuts", "full", _ar1_cov(128), "shared", 6128, "shared nuts ar1-cov d=128")


@pytest.mark.parametrize("d", [17, 64, 128])
def test_shared_matrix_kernel_hmc_replays_the_oracle(d):
    _sweep(d, "hmc", "full", _spd(d, 200 + d), "shared", 7000 + d, "shared hmc d=%d" % d)


@pytest.mark.parametrize("pot_kind", ["full", "inv", "full64"])
@pytest.mark.parametrize("d", [65, 100, 128])
def test_per_chain_kernel_at_two_elements_per_lane(d, pot_kind, monkeypatch):
    if pot_kind == "full":
        monkeypatch.setenv("LMC_DENSE_COOP", "0")   # QuadPotentialFull on the per-chain kernel
    _sweep(d, "nuts", pot_kind, _spd(d, 300 + d), "per_chain", 8000 + d, "per-chain %s d=%d" % (pot_kind, d))


@pytest.mark.parametrize("coop", ["1", "0"])
def test_non_symmetric_matrix_uses_its_lower_factor_and_the_matrix_as_given(coop, monkeypatch):
    """The reference factors the lower triangle only (scipy.linalg.cholesky(lower=True)) and forms velocities with cov as
    given (quadpotential.py:446-450): an SPD lower triangle under an upper triangle of its own. A transposed covT / ct, or a
    factor read from the upper triangle, differs here and nowhere else."""
    monkeypatch.setenv("LMC_DENSE_COOP", coop)
    d = 65
    rs = np.random.RandomState(11)
    mat = _spd(d, 400) + np.triu(0.05 * rs.randn(d, d), 1)
    assert np.abs(mat - mat.T).max() > 0.05
    _sweep(d, "nuts", "full", mat, "shared" if coop == "1" else "per_chain", 9065, "non-symmetric coop=%s" % coop)


# ---------------------------------------------------------------------------------------------------
# b. contract replay: the shared-matrix kernel against a host model of what it documents
# ---------------------------------------------------------------------------------------------------
def _near_f32_boundary(exact, bound):
    """True where the float32 rounding of ``exact`` (extended precision) could go either way for a value within ``bound``."""
    f = exact.astype(np.float32)
    lo = (f.astype(np.longdouble) + np.nextafter(f, np.float32(-np.inf)).astype(np.longdouble)) / 2
    hi = (f.astype(np.longdouble) + np.nextafter(f, np.float32(np.inf)).astype(np.longdouble)) / 2
    return bool((np.minimum(np.abs(exact - lo), np.abs(exact - hi)) <= bound).any())


class SharedKernelContract(orc.FullPotential):
    """What run_dense_coop_kernel documents, on the host in float64 / extended precision:
    * the float32 matrix and float32 lower factor as the device holds them (Engine.dense_chain);
    * momentum float32((L^-1)^T z_f32) with L^-1 in extended precision (lmc_dense.hpp: dense_momentum_solved);
    * every velocity the float64 product of the promoted float32 matrix (coop_product);
    * the start state (lmc_dense.hpp:312-347, dense_start_state): v0s = float32(C p0), kinetic = 0.5f * sdot(p0, v0s) in the
      engine's summation order (kSdotNative: exact float32 products summed in float64, rounded once; the OpenBLAS orders
      as _blas_probe.emulate_sdot restates them), energy = double(kinetic) - logp.
    ``fragile[i]``: iteration i drew a momentum element, or formed a start velocity element, that lies within float64
    reduction error of a float32 rounding boundary -- the device may round it the other way."""

    def __init__(self, cov32, chol32):
        self.cov = np.array(cov32, dtype=np.float32)
        self.chol = np.array(chol32, dtype=np.float32)
        self.n = len(self.cov)
        self.n_samples = 0
        self.momentum_f32 = True
        self.cov64 = self.cov.astype(np.float64)
        L = self.chol.astype(np.longdouble)
        n = self.n
        inv = np.zeros((n, n), dtype=np.longdouble)
        eye = np.eye(n, dtype=np.longdouble)
        for i in range(n):   # forward substitution, extended precision
            inv[i] = (eye[i] - L[i, :i].dot(inv[:i])) / L[i, i]
        self.linvT = inv.T.copy()
        self.fragile = []

    def random(self, rng):
        z = rng.normal(size=self.n).astype(np.float32).astype(np.longdouble)
        exact = self.linvT.dot(z)
        # the device sums float64-rounded entries of L^-1 times z in float64: (n + 2) ulps of the absolute sum
        bound = (self.n + 2) * np.finfo(np.float64).eps * np.abs(self.linvT).dot(np.abs(z))
        self.fragile.append(_near_f32_boundary(exact, bound))
        return exact.astype(np.float32)

    def velocity(self, x):
        if x.dtype == np.float32:   # the start state's stored velocity: the float64 product rounded once
            xl = x.astype(np.longdouble)
            exact = self.cov.astype(np.longdouble).dot(xl)
            bound = (self.n + 2) * np.finfo(np.float64).eps * np.abs(self.cov.astype(np.longdouble)).dot(np.abs(xl))
            self.fragile[-1] = self.fragile[-1] or _near_f32_boundary(exact, bound)
            return exact.astype(np.float32)
        return self.cov64.dot(x)

    def velocity_into(self, x, out):
        out[:] = self.cov64.dot(x)


def _sdot_of(mode):
    if mode == _abi.SDOT_NATIVE:
        return lambda x, y: np.float32(np.sum(x.astype(np.longdouble) * y.astype(np.longdouble)))
    return lambda x, y: emulate_sdot(x, y, mode)


@pytest.mark.parametrize("d", SHARED_D)
def test_shared_matrix_kernel_meets_its_float64_contract(d, monkeypatch):
    mat = _spd(d, 100 + d)
    seed = 5000 + d
    tgt = lmc.targets.AR1(d)
    dstep = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(mat))
    with dstep._make_engine(1) as eng:
        cov32, chol32 = eng.dense_chain(0)
        mode = int(eng.cfg.start_energy_sdot)
    np.testing.assert_array_equal(cov32, mat.astype(np.float32))
    pot = SharedKernelContract(cov32, chol32)
    monkeypatch.setattr(orc, "START_SDOT", _sdot_of(mode))
    ostep = orc.Step(otargets.make("ar1", d), d, kind="nuts", potential=pot)
    start = 0.5 * np.random.RandomState(seed).randn(d)
    snaps, outs = record_chain(ostep, start, np.random.RandomState(seed), TUNE, DRAWS)
    assert len(pot.fragile) == TUNE + DRAWS
    ran = run_snapshots(dstep, snaps)
    assert ran.kernels("dense") == {"shared"}, ran.engines
    res = assert_replay(ran, snaps, outs, Rules.dense(CONTRACT, 1e-9), "contract d=%d" % d, skip=lambda i: pot.fragile[i])
    print("contract d=%d: checked %d skipped %d (float32 boundary %d) of %d; worst position %.3g / stat %.3g of %g" % (
        d, res.checked, res.skipped, sum(pot.fragile), TUNE + DRAWS, res.worst_q, res.worst_stat, CONTRACT))
    # skips: oracle margins below 1e-9, and momentum / start-velocity elements within the (rigorous, so generous) float64
    # error bound of a float32 rounding boundary -- 0 to 3 of 19 per shape
    assert res.checked >= TUNE + DRAWS - 4, res


# ---------------------------------------------------------------------------------------------------
# c. bit identity across the placement knobs
# ---------------------------------------------------------------------------------------------------
def _run_direct(step, chains, tune, draws, seed=100):
    eng = step._make_engine(chains)
    try:
        d = eng.dim
        eng.seed(np.arange(chains, dtype=np.uint32) + seed)
        eng.set_position(0.3 * np.random.RandomState(seed).randn(chains, d))
        eng.reset_tuning()
        eng.reserve(tune + draws, keep_trace=True)
        eng.run(tune, 0, tune + draws)
        assert not eng.status().any()
        out = dict(trace=eng.trace(), kernel=eng.last_run_dense_kernel(),
                   rng=np.array([eng.get_rng_state(c)[2] for c in range(chains)]))
        out.update({k: np.asarray(v) for k, v in step._stats_from_engine(eng, 0, tune + draws).items()})
        return out
    finally:
        eng.close()


def _assert_same(a, b, tag):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (tag, k))


_KNOBS = ("LMC_DENSE_COOP", "LMC_DENSE_LDS_SLOTS", "LMC_DENSE_CACHE_ROWS", "LMC_SUB_BLOCKS")


def _with_env(monkeypatch, env, fn):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return fn()


@pytest.mark.parametrize("d", [33, 128])
def test_shared_matrix_results_do_not_depend_on_where_the_tree_stack_lives(d, monkeypatch):
    """Identity mass on AR(1) rho = 0.95: trees reach depth 7 and more, so the subtree stack runs past the LDS slots."""
    tgt = lmc.targets.AR1(d, 0.95)
    step = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(np.eye(d)))
    runs = {s: _with_env(monkeypatch, {} if s is None else {"LMC_DENSE_LDS_SLOTS": s}, lambda: _run_direct(step, 21, 30, 10))
            for s in (None, "0", "1", "3")}
    base = runs[None]
    assert base["kernel"] == "shared" and base["tree_size"].max() > 63, base["tree_size"].max()
    for s, r in runs.items():
        _assert_same(r, base, "LMC_DENSE_LDS_SLOTS=%s" % s)


def test_per_chain_results_do_not_depend_on_where_matrix_rows_and_tree_stack_live(monkeypatch):
    d = 100
    tgt = lmc.targets.AR1(d, 0.95)
    step = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(_spd(d, 500)))
    base = None
    for rows in (None, "0", "16"):
        for slots in (None, "0"):
            env = {"LMC_DENSE_COOP": "0"}
            if rows is not None:
                env["LMC_DENSE_CACHE_ROWS"] = rows
            if slots is not None:
                env["LMC_DENSE_LDS_SLOTS"] = slots
            r = _with_env(monkeypatch, env, lambda: _run_direct(step, 11, 20, 6))
            assert r["kernel"] == "per_chain"
            if base is None:
                base = r
            _assert_same(r, base, str(env))


@pytest.mark.parametrize("chains", [13, 300])
def test_shared_matrix_sub_blocks_start_mid_workgroup(chains, monkeypatch):
    """Two sub-blocks: the second starts at chain_begin = chains // 2, not a multiple of eight."""
    d = 40
    tgt = lmc.targets.AR1(d)
    step = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(_spd(d, 600)))
    one = _with_env(monkeypatch, {"LMC_SUB_BLOCKS": "1"}, lambda: _run_direct(step, chains, 12, 4))
    two = _with_env(monkeypatch, {"LMC_SUB_BLOCKS": "2"}, lambda: _run_direct(step, chains, 12, 4))
    assert one["kernel"] == two["kernel"] == "shared"
    _assert_same(two, one, "LMC_SUB_BLOCKS=2")


# ---------------------------------------------------------------------------------------------------
# d. the benchmark's shape through sample(): selected chains of a 4099-chain job against oracle chains on the same seeds
# ---------------------------------------------------------------------------------------------------
def test_benchmark_shape_chains_follow_the_oracle():
    d, chains, tune, draws, n_it = 128, 4099, 30, 10, 10
    cov = _ar1_cov(d)
    tgt = lmc.targets.AR1(d, 0.9)
    seeds = orc.derive_seeds(2024, chains)   # sample(random_seed=2024) derives the same prefix-stable seeds
    start = orc.jitter_start(seeds[0], d)
    trace, stats, eng = lmc.sample(tgt, d, draws=draws, tune=tune, chains=chains, start=start, random_seed=2024,
                                   step=lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(cov)),
                                   discard_tuned_samples=False, progressbar=False, return_engine=True)
    try:
        assert eng.last_run_dense_kernel() == "shared"
    finally:
        eng.close()
    sel = [0, 7, 8, chains // 2, 4096, 4097, 4098]   # 4096..4098: the last workgroup, five idle waves
    ostep = orc.Step(otargets.make("ar1", d), d, kind="nuts", potential=orc.FullPotential(cov))
    ot, ost, margins = orc.sample(otargets.make("ar1", d), d, draws=0, tune=n_it, step=ostep, chains=len(sel), start=start,
                                  random_seed=[seeds[c] for c in sel], discard_tuned_samples=False, record_margins=True)
    compared = []
    for k, c in enumerate(sel):
        m = np.asarray(margins[k])
        m = m if m.ndim == 1 else m.min(axis=1)
        fragile = np.nonzero(m[:n_it] < DECISION)[0]
        n_q = int(fragile[0]) if len(fragile) else n_it   # a decision within DECISION of its threshold may flip there
        for name in INT_STATS:
            if name in ost:
                np.testing.assert_array_equal(stats[name][c, :n_q, 0], ost[name][k, :n_q, 0], err_msg="chain %d %s" % (c, name))
        # iteration 0 starts from the same state on both sides: one transition, REPLAY_F32 (float32-born momentum). Later
        # iterations carry their own state, and dual averaging feeds the float32 separation back into the step size
        # (geometric growth): there the integer statistics above are the check.
        np.testing.assert_allclose(trace[c, 0], ot[k, 0], rtol=REPLAY_F32, atol=REPLAY_F32 * (1 + np.abs(ot[k, 0]).max()),
                                   err_msg="chain %d" % c)
        compared.append(n_q)
    print("benchmark shape: iterations compared per chain", dict(zip(sel, compared)))
    assert sum(compared) >= 0.8 * n_it * len(sel), compared


# ---------------------------------------------------------------------------------------------------
# rare paths (far starts, divergences, max depth, weight-offset moves) through both dense kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass,coop", [("full", "1"), ("full", "0"), ("full_inv", "1")])
def test_rare_paths_through_the_dense_kernels(mass, coop):
    env = dict(os.environ, LMC_DENSE_COOP=coop)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz_rare.py"), "24", "7", "auto", mass],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    print(tail)
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if "failures:" in ln][-1]
    assert "failures: 0" in summary, summary
    seen = ast.literal_eval(summary[summary.index("{"):summary.index("}") + 1])   # the tool's own dict literal
    assert seen["diverging"] > 0 and seen["maxdepth"] > 0 and seen["rescale"] > 0, seen
    assert ("kernel %s" % ("shared" if (mass == "full" and coop == "1") else "per_chain")) in r.stdout, summary
