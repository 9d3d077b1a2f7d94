"""No GPU: the host side of the pooled dense mass matrix (QuadPotentialFullPooled) -- Stan's window layout, the job loop
against a stand-in engine, validation, and the five new symbols of the C ABI."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, sampling
from littlemcmc_amd.quadpotential import SNAPSHOTS_PER_WINDOW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_SYMBOLS = ("lmc_engine_pool_reset", "lmc_engine_pool_accumulate", "lmc_engine_pool_get", "lmc_engine_pool_apply",
                "lmc_engine_restart_dual_average")


def test_pooled_windows_quoted_layouts():
    assert sampling.pooled_windows(1000) == [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]
    assert sampling.pooled_windows(400) == [(75, 100), (100, 150), (150, 350)]
    assert sampling.pooled_windows(100) == [(15, 90)]


def test_pooled_windows_are_contiguous_growing_and_inside_tuning():
    for tune in range(0, 3001):
        w = sampling.pooled_windows(tune)
        if tune < 20:
            assert w == [], tune
            continue
        assert w, tune
        for k, (b, e) in enumerate(w):
            assert 0 <= b < e <= tune, (tune, w)
            if k:
                assert b == w[k - 1][1], (tune, w)
                assert e - b >= w[k - 1][1] - w[k - 1][0], (tune, w)


class FakePooledEngine:
    """Records what the pooled job loop asks of an engine (the stand-in of tests/test_host_logic_cpu.py plus the pool calls).
    No GPU here: torch.cuda.ExternalStream fails on the stream handle and _run_job takes the blocking wait."""

    def __init__(self, chains=64, done_when_stopped=0):
        self.chains = chains
        self.target = types.SimpleNamespace(family=_abi.TARGET_STD_NORMAL)
        self.cfg = types.SimpleNamespace(device=0)
        self.calls = []
        self._done = done_when_stopped

    def run_streams(self):
        return [0]

    def run(self, tune, it, n):
        self.calls.append(("run", tune, it, n))

    def progress(self):
        return 0

    def synchronize(self):
        self.calls.append(("sync",))

    def request_stop(self, stop=True):
        self.calls.append(("stop", bool(stop)))

    def completed_iterations(self):
        return self._done

    def pool_reset(self):
        self.calls.append(("pool_reset",))

    def pool_accumulate(self):
        self.calls.append(("pool_accumulate",))

    def pool_apply(self):
        self.calls.append(("pool_apply",))

    def restart_dual_average(self):
        self.calls.append(("restart_dual_average",))


def test_pooled_job_loop_call_sequence():
    eng = FakePooledEngine()
    seen = []
    n_done, interrupted = sampling._run_job_pooled(
        eng, tune=400, n_total=500, per_launch=100, progressbar=False,
        on_enqueued=lambda first, n: seen.append(("window", first, n)),
        before_enqueue=lambda first, n: seen.append(("before", first, n)))
    assert (n_done, interrupted) == (500, False)
    runs = [c for c in eng.calls if c[0] == "run"]
    assert all(c[1] == 400 for c in runs)
    # launches tile [0, 500) without gap or overlap
    at = 0
    for _r, _t, first, n in runs:
        assert first == at and n >= 1
        at += n
    assert at == 500
    # the streamer hooks see every launch, before and after it is enqueued
    assert [s[1:] for s in seen if s[0] == "before"] == [c[2:] for c in runs]
    assert [s[1:] for s in seen if s[0] == "window"] == [c[2:] for c in runs]
    # inside a window: SNAPSHOTS_PER_WINDOW launches, each followed by a snapshot; outside: none
    windows = sampling.pooled_windows(400)
    assert windows == [(75, 100), (100, 150), (150, 350)]
    for b, e in windows:
        inside = [c for c in runs if b <= c[2] < e]
        assert len(inside) == SNAPSHOTS_PER_WINDOW == 8
        assert len({c[3] for c in inside[:-1]}) == 1 and inside[-1][3] >= inside[0][3]
        assert sum(c[3] for c in inside) == e - b and inside[-1][2] + inside[-1][3] == e
    for i, c in enumerate(eng.calls):
        if c[0] == "run":
            in_window = any(b <= c[2] < e for b, e in windows)
            assert (eng.calls[i + 1] == ("pool_accumulate",)) == in_window, (i, c)
    assert sum(c[0] == "pool_accumulate" for c in eng.calls) == 8 * len(windows)
    # the matrix changes exactly at the window ends: apply, restart, reset -- after the device has drained
    ends = []
    reached = 0
    for i, c in enumerate(eng.calls):
        if c[0] == "run":
            reached = c[2] + c[3]
        if c[0] == "pool_apply":
            assert eng.calls[i - 1] == ("sync",)
            assert [x[0] for x in eng.calls[i:i + 3]] == ["pool_apply", "restart_dual_average", "pool_reset"]
            ends.append(reached)
    assert ends == [100, 150, 350]
    assert sum(c[0] == "restart_dual_average" for c in eng.calls) == 3
    assert sum(c[0] == "pool_reset" for c in eng.calls) == 4 and eng.calls[0] == ("pool_reset",)   # (+ the one before the job)


def test_pooled_job_loop_without_windows_is_the_plain_job():
    eng = FakePooledEngine()
    assert sampling._run_job_pooled(eng, tune=10, n_total=40, per_launch=25, progressbar=False) == (40, False)
    assert [c for c in eng.calls if c[0] == "run"] == [("run", 10, 0, 25), ("run", 10, 25, 15)]
    assert not any(c[0] in ("pool_accumulate", "pool_apply", "restart_dual_average") for c in eng.calls)


def test_keyboard_interrupt_inside_a_window_stops_the_device(monkeypatch):
    """Ctrl-C from the wait loop while a window's launches are in flight: stop request, drain, the iterations every chain
    completed come back and no matrix is installed afterwards."""
    eng = FakePooledEngine(done_when_stopped=83)
    real_sync = eng.synchronize
    state = {"armed": True}

    def sync():
        real_sync()
        launched = [c for c in eng.calls if c[0] == "run"]
        if state["armed"] and launched and launched[-1][2] >= 75:     # the first wait inside the window [75, 100)
            state["armed"] = False
            raise KeyboardInterrupt

    monkeypatch.setattr(eng, "synchronize", sync)
    n_done, interrupted = sampling._run_job_pooled(eng, tune=400, n_total=500, per_launch=100, progressbar=False)
    assert (n_done, interrupted) == (83, True)
    kinds = [c[0] for c in eng.calls]
    i = kinds.index("stop")
    assert eng.calls[i] == ("stop", True) and "sync" in kinds[i:] and eng.calls[-1] == ("stop", False)
    assert "pool_apply" not in kinds and "run" not in kinds[i:]


def test_keyboard_interrupt_from_the_callback_inside_a_window(monkeypatch):
    """The same with the interrupt raised by ``callback`` (the reference's way, sampling.py:272-277): the wait loop that
    calls it needs completion events, which a stand-in for torch provides."""
    import sys

    class Event:
        def record(self, stream):
            pass

        def query(self):
            return True

    class Ctx:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    fake_cuda = types.SimpleNamespace(ExternalStream=lambda h, device=None: types.SimpleNamespace(device=device),
                                      device=lambda d: Ctx(), Event=Event)
    monkeypatch.setitem(sys.modules, "torch", types.SimpleNamespace(cuda=fake_cuda, device=lambda *a: a))
    eng = FakePooledEngine(done_when_stopped=80)
    eng.progress = lambda: max([c[2] for c in eng.calls if c[0] == "run"] or [0])

    def cb(trace, draw):
        assert draw.total == 500
        if draw.iteration >= 78:
            raise KeyboardInterrupt

    n_done, interrupted = sampling._run_job_pooled(eng, tune=400, n_total=500, per_launch=100, progressbar=False, callback=cb)
    assert (n_done, interrupted) == (80, True)
    kinds = [c[0] for c in eng.calls]
    assert ("stop", True) in eng.calls and eng.calls[-1] == ("stop", False) and "pool_apply" not in kinds
    assert max(c[2] for c in eng.calls if c[0] == "run") < 100      # nothing beyond the window it was interrupted in


def test_validation():
    tgt = lmc.targets.AR1(16, 0.9)
    with pytest.raises(NotImplementedError, match="256"):
        lmc.QuadPotentialFullPooled(257)
    with pytest.raises(NotImplementedError, match="256"):
        lmc.init_nuts(lmc.targets.StdNormal(300), 300, init="adapt_full_pooled")
    with pytest.raises(ValueError, match="initial_cov"):
        lmc.QuadPotentialFullPooled(4, np.eye(5))
    for init in ("adapt_full_pooled", "jitter+adapt_full_pooled"):
        start, step = lmc.init_nuts(tgt, 16, init=init, random_seed=5)
        assert isinstance(step.potential, lmc.QuadPotentialFullPooled) and isinstance(step.potential, lmc.QuadPotentialFull)
        assert step.potential._engine_kind == "full" and start.shape == (16,)
        assert (start == 0).all() == (init == "adapt_full_pooled")
    np.testing.assert_array_equal(lmc.QuadPotentialFullPooled(3)._cov, np.eye(3, dtype=np.float32))
    # chains * 8 <= model_ndim: refused before anything is launched (no engine is made: this test has no GPU)
    with pytest.raises(ValueError, match="chains"):
        lmc.sample(tgt, 16, draws=10, tune=30, chains=2, init="adapt_full_pooled", random_seed=1, progressbar=False)
    with pytest.raises(NotImplementedError, match="one GPU"):
        lmc.sample(tgt, 16, draws=10, tune=30, chains=64, init="adapt_full_pooled", random_seed=1, devices=[0, 1],
                   progressbar=False)
    with pytest.raises(NotImplementedError, match="one GPU"):
        lmc.sample(tgt, 16, draws=10, tune=30, chains=64, step=lmc.HamiltonianMC(tgt, 16, potential=lmc.QuadPotentialFullPooled(16)),
                   random_seed=1, devices=2, progressbar=False)


def test_pool_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert int(re.search(r"#define LMC_ABI_VERSION (\d+)", header).group(1)) == 9 == _abi.ABI_VERSION
    lib = _abi.load()
    assert lib.lmc_abi_version() == 9
    raw = ctypes.CDLL(_abi.LIB_PATH)      # the binary itself, not the typed binding
    for name in POOL_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert hasattr(raw, name), "liblmc_hip.so does not export %s" % name
    unit = open(os.path.join(ROOT, "littlemcmc_amd", "csrc", "lmc_pool.hip")).read()
    assert "getenv" not in unit and "atomic" not in unit.replace("floating-point atomics", "")
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in unit
