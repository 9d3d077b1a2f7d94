"""No GPU: the host plumbing of the eleven sampler settings -- init_nuts / NUTS / HamiltonianMC -> step._make_engine -> Engine ->
engine.engine_config -> struct lmc_config. The Engine is replaced by a recorder that fills the struct exactly as Engine does
(engine_config is the function Engine.__init__ calls) and creates nothing on a device."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, engine
from littlemcmc_amd import targets as T
from tests._settings_cases import CASES

FIELD = {"Emax": "emax"}   # keyword -> lmc_config field, where the names differ
DEFAULTS = dict(target_accept=0.8, Emax=1000.0, gamma=0.05, k=0.75, t0=10.0, adapt_step_size=True, step_scale=0.25,
                max_treedepth=10, early_max_treedepth=8, path_length=2.0, max_steps=1024)
OF_KIND = {"nuts": set(DEFAULTS) - {"path_length", "max_steps"},         # (NUTS takes path_length and never reads it: nuts.py:110)
           "hmc": set(DEFAULTS) - {"max_treedepth", "early_max_treedepth"}}
ALL_OFF = dict(target_accept=0.91, Emax=7.5, gamma=0.02, k=0.55, t0=31.0, adapt_step_size=False, step_scale=0.11,
               max_treedepth=7, early_max_treedepth=3, path_length=1.3, max_steps=17)


class _Recorded(Exception):
    """Carries the struct out of step._make_engine: there is no engine for the potential to push its state to."""


class _Recorder:
    """What step._make_engine constructs instead of an Engine: the same lmc_config, no device."""

    def __init__(self, target, chains, device=0, lib_path=None, first_chain=0, chains_per_group=None, **kw):
        raise _Recorded(engine.engine_config(_abi.load(), target, chains, device=device, **kw)[0])


@pytest.fixture
def config_of(monkeypatch):
    monkeypatch.setattr(engine, "Engine", _Recorder)

    def build(step, chains=3):
        with pytest.raises(_Recorded) as got:
            step._make_engine(chains)
        cfg = got.value.args[0]
        assert cfg.chains == chains and cfg.dim == step.model_ndim
        return cfg

    return build


def _assert_config(cfg, kind, kw):
    assert cfg.kind == {"nuts": _abi.KIND_NUTS, "hmc": _abi.KIND_HMC}[kind]
    for name, default in DEFAULTS.items():
        want = kw[name] if (name in kw and name in OF_KIND[kind]) else default
        got = getattr(cfg, FIELD.get(name, name))
        assert got == want, (name, got, want)
        if name == "adapt_step_size":
            assert got in (0, 1) and got == int(bool(want))


def _steps(case_kind, tgt, d, kw):
    """Every public way to a step of this kind with these keywords."""
    if case_kind == "nuts":
        return [lmc.NUTS(tgt, d, **kw), lmc.init_nuts(tgt, d, random_seed=[5, 6], **kw)[1],
                lmc.init_nuts(tgt, d, init="adapt_full", **kw)[1],
                lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(np.eye(d)), **kw)]
    return [lmc.HamiltonianMC(tgt, d, **kw), lmc.HamiltonianMC(tgt, d, potential=lmc.QuadPotentialFullInv(np.eye(d)), **kw)]


@pytest.mark.parametrize("name", list(CASES))
def test_the_keywords_of_a_settings_case_reach_lmc_config(config_of, name):
    case = CASES[name]
    d = min(case.d, 12)     # (the struct does not depend on the size; dense potentials of d = 600 are not needed here)
    tgt = T.StdNormal(d)
    for step in _steps(case.kind, tgt, d, case.kw):
        _assert_config(config_of(step), case.kind, case.kw)
    # golden keyword values arrive as floats (tests/_gpu_util.py: kwargs_from), booleans as 0.0 / 1.0
    as_floats = {k: (v if k in ("max_treedepth", "early_max_treedepth", "max_steps") else float(v)) for k, v in case.kw.items()}
    for step in _steps(case.kind, tgt, d, as_floats):
        _assert_config(config_of(step), case.kind, case.kw)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_every_setting_off_its_default_at_once_and_one_at_a_time(config_of, kind):
    d = 5
    tgt = T.StdNormal(d)
    mine = {k: v for k, v in ALL_OFF.items() if k in OF_KIND[kind]}
    assert all(mine[k] != DEFAULTS[k] for k in mine)
    for step in _steps(kind, tgt, d, mine):
        _assert_config(config_of(step), kind, mine)
    for k, v in mine.items():       # one at a time: no setting is read from another's argument
        for step in _steps(kind, tgt, d, {k: v}):
            _assert_config(config_of(step), kind, {k: v})
    for step in _steps(kind, tgt, d, {}):
        _assert_config(config_of(step), kind, {})


def test_engine_config_is_what_engine_hands_to_the_library(monkeypatch):
    """Engine.__init__ passes engine_config's struct to lmc_engine_create unchanged (seen by a library stand-in)."""
    import ctypes

    seen = {}
    real = _abi.load()

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        def lmc_engine_create(self, cfg_ref, h_ref):
            seen["cfg"] = bytes(ctypes.string_at(ctypes.addressof(cfg_ref._obj), ctypes.sizeof(_abi.Config)))
            return 1

        def lmc_last_error(self, h):
            return b"stand-in"

    monkeypatch.setattr(_abi, "load", lambda path=None: Lib())
    kw = dict(kind="hmc", potential="diag", **{k: v for k, v in ALL_OFF.items() if k in OF_KIND["hmc"]})
    with pytest.raises(_abi.HipLibraryError, match="stand-in"):
        lmc.Engine(T.StdNormal(4), chains=2, sdot="haswell", tuning={}, **kw)
    cfg, _ = engine.engine_config(real, T.StdNormal(4), 2, sdot="haswell", tuning={}, **kw)
    assert seen["cfg"] == bytes(ctypes.string_at(ctypes.addressof(cfg), ctypes.sizeof(_abi.Config)))
    assert cfg.emax == 7.5 and cfg.max_steps == 17 and cfg.adapt_step_size == 0
