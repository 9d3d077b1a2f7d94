"""Sampler settings off their defaults: THE case table (tests/golden/capture.py: capture_settings captures the first seven
from the reference as tests/golden/e2e_set_<case>.npz) and what each case is for, asserted on the oracle's own chain wherever a case is
replayed -- a change of seeds cannot then hollow a case out without a test saying so."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "family d kind kw tune draws")

SEED = 20261116   # random_seed of the captured runs; the chains run on oracle.derive_seeds(SEED, 2)

CASES = {
    "da_params": Case("std_normal", 10, "nuts", dict(target_accept=0.95, gamma=0.1, k=0.6, t0=25.0), 40, 10),
    "low_accept": Case("ar1", 16, "nuts", dict(target_accept=0.6, step_scale=0.5), 40, 10),
    "emax_funnel": Case("funnel", 8, "nuts", dict(Emax=5.0, max_treedepth=6, early_max_treedepth=4), 40, 40),
    "depth_caps": Case("std_normal", 10, "nuts", dict(early_max_treedepth=2, max_treedepth=3, step_scale=0.05), 30, 30),
    "fixed_step": Case("std_normal", 70, "nuts", dict(adapt_step_size=False, step_scale=0.6), 20, 20),
    "hmc_caps": Case("std_normal", 10, "hmc", dict(path_length=0.7, max_steps=3, step_scale=0.1, target_accept=0.9), 30, 20),
    "hmc_emax": Case("funnel", 8, "hmc", dict(Emax=2.0, path_length=3.0), 40, 30),
    # no golden, oracle only: the depth caps on a team of four wavefronts per chain
    "depth_caps_team": Case("std_normal", 600, "nuts", dict(early_max_treedepth=2, max_treedepth=3, step_scale=0.05), 12, 8),
}
GOLDEN = [n for n in CASES if n != "depth_caps_team"]
NUTS_CASES = [n for n in GOLDEN if CASES[n].kind == "nuts"]

# The keywords a case is about: a device step built WITHOUT one of these groups (so on the default) must fail the replay.
ABOUT = {
    "da_params": [("gamma",), ("k",), ("t0",), ("target_accept",)],
    "low_accept": [("step_scale",)],
    "emax_funnel": [("Emax",)],
    "depth_caps": [("early_max_treedepth", "max_treedepth")],
    "fixed_step": [("adapt_step_size",)],
    "hmc_caps": [("max_steps",)],
    "hmc_emax": [("Emax",)],
}


def assert_the_case_does_what_it_is_for(name, stats, tune):
    """``stats``: per-iteration arrays of ONE oracle chain of case ``name`` (tuning iterations first)."""
    case = CASES[name]
    kw = case.kw
    stats = {k: np.ravel(v) for k, v in stats.items()}
    div = stats["diverging"].astype(bool)
    if name == "emax_funnel":
        # divergences that only the lowered Emax reports: the default (1000) would have integrated on through each of them
        # (max_energy_error is the diverging leaf's own energy change, energy_error the proposal's)
        assert div.sum() >= 5 and (np.abs(stats["max_energy_error"][div]) < 1000.0).all(), (div.sum(), stats["max_energy_error"][div])
        assert (np.abs(stats["energy_error"][div]) < 1000.0).all(), stats["energy_error"][div]
    if name in ("depth_caps", "depth_caps_team"):
        at_cap = 10 if name == "depth_caps" else 6   # (the team case has 12 tuning iterations and 8 draws)
        assert (stats["depth"][:tune] == kw["early_max_treedepth"]).sum() >= at_cap, stats["depth"][:tune]
        assert (stats["depth"][tune:] == kw["max_treedepth"]).sum() >= at_cap, stats["depth"][tune:]
        assert stats["depth"][:tune].max() <= kw["early_max_treedepth"] and stats["depth"].max() <= kw["max_treedepth"]
    if name == "hmc_caps":
        assert (stats["n_steps"] == kw["max_steps"]).sum() >= 2 and stats["n_steps"].max() == kw["max_steps"], stats["n_steps"]
        assert (stats["n_steps"] < kw["max_steps"]).any()   # ... and path_length / step_size decides the others
    if name == "fixed_step":
        step = kw["step_scale"] / case.d ** 0.25
        assert (stats["step_size"] == stats["step_size"][0]).all() and (stats["step_size_bar"] == stats["step_size_bar"][0]).all()
        np.testing.assert_allclose([stats["step_size"][0], stats["step_size_bar"][0]], step, rtol=1e-15)
        assert stats["tune"][:tune].all() and tune > 0   # the tuning iterations are there: the fixed step with ``tune`` set
    if name == "hmc_emax":
        # (a first trajectory from the jittered start can leave the funnel altogether, at any Emax: counted out, not required away)
        only_lowered = div & (np.abs(stats["energy_error"]) < 1000.0)
        assert only_lowered.sum() >= 3, stats["energy_error"][div]


def stats_of(outs):
    """Per-iteration arrays from record_chain's outputs."""
    return {k: np.array([o["stats"][k] for o in outs]) for k in outs[0]["stats"]}


def dense_matrix(d, seed):
    """a a^T / d + I / 2 (as tests/test_gpu_dense.py: test_dense_fixed_wide_vectors builds its fixed matrices)."""
    a = np.random.RandomState(seed).randn(d, d) / np.sqrt(d)
    return a @ a.T + 0.5 * np.eye(d)
