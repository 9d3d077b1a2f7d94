"""Per-group target parameters without a GPU: the row arithmetic (targets.Batched.row_of_chain on the host,
lmc_target_param_row in the library) against its literal statement, the grouped setter's refusals before any HIP call,
targets.Batched's construction rules, and sample()'s dealing of chains and engines with a fake engine."""
import ctypes
import os
import pickle
import types

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, sampling
from littlemcmc_amd import targets as T

NEW_SYMBOLS = ("lmc_engine_set_target_params_grouped", "lmc_engine_target_groups", "lmc_target_param_row")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # LMC_ERR_INVALID


def _lib_row(lib, chain, first, per):
    row = ctypes.c_int64(-1)
    assert lib.lmc_target_param_row(chain, first, per, ctypes.byref(row)) == _abi.OK
    return row.value


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    lib = _abi.load()
    for name in NEW_SYMBOLS + ("lmc_target_groups_check",):
        assert name + "(" in header, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.lmc_abi_version() == 9 == _abi.ABI_VERSION     # additive: the ABI number stays


def test_row_arithmetic_host_and_library_against_the_literal_statement():
    """"Chain j of the job is in group j // chains_per_group", for engines of 1-20 chains whose chain 0 is chain 0-40 of the
    job, in groups of 1-9 chains: the job's chains are listed with their groups first, then every engine chain is looked up."""
    lib = _abi.load()
    for per in range(1, 10):
        group_of_job_chain = [j // per for j in range(40 + 20)]
        for first in range(41):
            for n in range(1, 21):
                want = group_of_job_chain[first:first + n]
                assert [T.Batched.row_of_chain(c, first, per) for c in range(n)] == want
                assert [_lib_row(lib, c, first, per) for c in range(n)] == want


def test_row_arithmetic_rejects_nonsense():
    lib = _abi.load()
    for bad in ((-1, 0, 1), (0, -1, 1), (0, 0, 0), (0, 0, -2), (2 ** 31, 0, 1)):
        assert lib.lmc_target_param_row(*bad, None) == INVALID
    for bad in ((-1, 0, 1), (0, -1, 1), (0, 0, 0)):
        with pytest.raises(ValueError):
            T.Batched.row_of_chain(*bad)
    assert lib.lmc_target_param_row(5, 3, 4, None) == _abi.OK     # (a NULL result pointer is skipped)


def test_grouped_setter_validates_before_any_hip_call():
    """No device is needed to see a refusal. The setter looks at what needs no engine first -- zero groups,
    chains_per_group 0, a negative first_chain are refused even with a NULL engine -- and then runs lmc_target_groups_check,
    the whole validation as a pure function of (family, dim, chains), which is exercised here for every refusal."""
    lib = _abi.load()
    table = np.zeros((4, 3))
    setter = lambda *a: lib.lmc_engine_set_target_params_grouped(None, _abi.ptr(table), *a)   # noqa: E731
    err = lambda: lib.lmc_last_error(None)   # noqa: E731
    assert setter(0, 3, 0, 2) == INVALID and b"n_groups must be >= 1" in err()
    assert setter(4, 3, 0, 0) == INVALID and b"chains_per_group must be >= 1" in err()
    assert setter(4, 3, -1, 2) == INVALID and b"first_chain must be >= 0" in err()
    assert setter(4, 3, 0, 2) == INVALID and b"null engine" in err()          # nothing wrong with the shape: no engine
    assert lib.lmc_engine_target_groups(None, None, None, None, None) == INVALID

    check = lib.lmc_target_groups_check
    ar1, diag = _abi.TARGET_AR1, _abi.TARGET_DIAG_GAUSSIAN
    # (family, dim, chains, n_groups, n_per_group, first_chain, chains_per_group)
    assert check(ar1, 16, 8, 4, 3, 0, 2) == _abi.OK                           # chains 0..7 in pairs: rows 0..3
    assert check(ar1, 16, 8, 4, 3, 0, 3) == _abi.OK                           # table longer than needed
    assert check(ar1, 16, 3, 3, 3, 3, 3) == _abi.OK                           # a device block: chains 3..5 of the job, row 1
    assert check(ar1, 16, 9, 4, 3, 0, 2) == INVALID and b"reads row 4 of a table of 4 rows" in err()
    assert check(ar1, 16, 8, 4, 3, 1, 2) == INVALID and b"reads row 4" in err()   # the block offset counts
    assert check(ar1, 16, 8, 0, 3, 0, 2) == INVALID and b"n_groups" in err()
    assert check(ar1, 16, 8, 4, 3, 0, 0) == INVALID and b"chains_per_group" in err()
    assert check(ar1, 16, 8, 4, 3, -1, 2) == INVALID and b"first_chain" in err()
    for n in (0, 2, 4):
        assert check(ar1, 16, 8, 4, n, 0, 2) == INVALID and b"ar1 needs params" in err()
    assert check(diag, 5, 6, 3, 5, 0, 2) == _abi.OK
    assert check(diag, 5, 6, 3, 4, 0, 2) == INVALID and b"diag_gaussian needs 5" in err()
    assert check(_abi.TARGET_NORMAL1D, 1, 6, 3, 3, 0, 2) == INVALID and b"normal1d" in err()
    assert check(_abi.TARGET_USER, 7, 6, 3, 1, 0, 2) == _abi.OK               # a user density takes any row length
    assert check(ar1, 16, 8, 4, 3, 2 ** 31, 2) == INVALID                     # job chain indices are 32-bit on the device


def _student(d, nu, source=None):
    t = T.UserTarget.separable(d, logp="-0.5*(P[0]+1.0)*log1p(q*q/P[0])", grad="-(P[0]+1.0)*q/(P[0]+q*q)", params=[nu])
    if source is not None:
        t.source = source
    return t


def test_batched_holds_its_members_and_their_table():
    rhos = [0.0, 0.3, 0.9]
    b = T.Batched([T.AR1(16, rho=r) for r in rhos])
    assert isinstance(b, T.DeviceTarget) and b.family == _abi.TARGET_AR1 and b.d == 16 and b.lib_path is None
    assert b.groups == len(b) == 3 and b.params.shape == (3, 3) and b.params.flags["C_CONTIGUOUS"]
    for g, r in enumerate(rhos):
        assert b[g] is b.members[g] and b[g].rho == r
        np.testing.assert_array_equal(b.params[g], T.AR1(16, rho=r).params)
    assert T.Batched([T.StdNormal(4), T.StdNormal(4)]).params.shape == (2, 0)
    assert lmc.targets.require_device_target(b, 16) is b
    with pytest.raises(TypeError, match=r"batched\[g\]\(q\)"):
        b(np.zeros(16))


@pytest.mark.parametrize("members, exc, names", [
    (lambda: [T.AR1(4), T.StdNormal(4)], TypeError, "member 1"),                                    # mixed classes
    (lambda: [T.AR1(4), T.AR1(4), T.AR1(5)], ValueError, "member 2"),                               # mixed d
    (lambda: [T.UserTarget(4, "x", params=[1.0], jit="hiprtc"),
              T.UserTarget(4, "x", params=[1.0, 2.0], jit="hiprtc")], ValueError, "member 1"),      # mixed parameter lengths
    (lambda: [_student(4, 3.0), _student(4, 5.0, source="// another\n")], ValueError, "member 1"),  # different sources
    (lambda: [T.TorchTarget(4, lambda q: (q, q))] * 2, TypeError, "member 0"),                      # a callable sees all chains
    (lambda: [T.CallableTarget(4, lambda q: (0.0, q))], TypeError, "member 0"),
    (lambda: [T.Batched([T.AR1(4)])], TypeError, "member 0"),                                       # nested
    (lambda: [T.AR1(4), "ar1"], TypeError, "member 1"),
    (lambda: [], ValueError, "at least one"),                                                       # empty
])
def test_batched_construction_errors_name_the_member(members, exc, names):
    with pytest.raises(exc, match=names):
        T.Batched(members())


def test_chain_slices_tile_the_chains():
    b = T.Batched([T.Normal1D(loc, 1.0) for loc in range(5)])
    for per in (1, 2, 7):
        chains = 5 * per
        sl = b.chain_slices(chains)
        assert len(sl) == 5
        assert [c for s in sl for c in range(chains)[s]] == list(range(chains))
        for g, s in enumerate(sl):
            assert {b.row_of_chain(c, 0, per) for c in range(chains)[s]} == {g}
    for bad in (0, 4, 6, 11):
        with pytest.raises(ValueError, match="multiple of 5"):
            b.chain_slices(bad)


def test_batched_pickles_like_the_other_targets():
    b = T.Batched([T.DiagGaussian(np.linspace(1.0, 2.0, 5) * (g + 1)) for g in range(3)])
    c = pickle.loads(pickle.dumps(b))
    assert type(c) is T.Batched and c.groups == 3 and c.d == 5 and c.family == b.family
    np.testing.assert_array_equal(c.params, b.params)
    np.testing.assert_array_equal(c[2].params, b[2].params)
    u = pickle.loads(pickle.dumps(T.Batched([_student(7, 3.0), _student(7, 9.0)])))
    assert u[1].params[0] == 9.0 and u[0].source == u[1].source and u[0]._code == {}


def test_engine_grouping_is_resolved_before_anything_is_created():
    from littlemcmc_amd.engine import _target_grouping

    b = T.Batched([T.AR1(8, rho=r) for r in (0.1, 0.2, 0.3)])
    assert _target_grouping(T.AR1(8), 7, 0, None) == (0, None)                # any other target: nothing changes
    assert _target_grouping(b, 6, 0, None) == (0, 2)
    assert _target_grouping(b, 3, 3, 3) == (3, 3)                              # a device block inside the job
    assert _target_grouping(b, 1, 0, 2) == (0, 2)                              # the one-chain residency probe
    with pytest.raises(ValueError, match="chains % groups"):
        _target_grouping(b, 7, 0, None)
    with pytest.raises(ValueError, match="reach past"):
        _target_grouping(b, 4, 3, 2)
    with pytest.raises(ValueError, match="Batched"):
        _target_grouping(T.AR1(8), 6, 2, None)
    with pytest.raises(ValueError):                                            # Engine() itself, before the library is entered
        lmc.Engine(b, chains=7)


# ---- sample() with a fake engine (the style of tests/test_host_logic_cpu.py) ---------------------------------------
class _FakeEngine:
    def __init__(self, chains, dim, target, log):
        self.chains, self.dim, self.target, self.log = chains, dim, target, log
        self.cfg = types.SimpleNamespace(device=0)
        self.wide, self.kind, self.potential = False, "nuts", "diag_adapt"
        self.capacity, self.keep_trace, self.trace_begin, self.thin = 0, False, 0, 1

    def seed(self, seeds):
        self.log.append(("seed", len(seeds)))

    def set_position(self, q):
        pass

    def reset_tuning(self):
        pass

    def reserve(self, capacity, keep_trace=True, trace_begin=0, thin=1):
        pass

    def resident_chains(self):
        return 1024

    def run_streams(self):
        return []

    def run(self, tune, first, n):
        self.log.append(("run", first, n))

    def synchronize(self):
        pass

    def progress(self):
        return 0

    def status(self):
        return np.zeros(self.chains, dtype=np.int32)

    def trace(self, lo, n):
        return np.zeros((self.chains, n, self.dim))

    def counters(self):
        return np.zeros((self.chains, _abi.NUM_COUNTERS), dtype=np.int64)

    def stat_f64(self, stat, lo, n):
        return np.zeros((self.chains, n))

    def close(self):
        pass


class _FakeStep:
    stats_dtypes = [{"tree_size": np.float64}]

    def __init__(self, target, potential=None):
        self.target, self.made = target, []
        self.step_adapt = types.SimpleNamespace(_pull=lambda eng, chain: None)
        self.potential = potential or types.SimpleNamespace(_pull=lambda eng, chain: None)
        self.tune, self._samples_after_tune, self._num_divs_sample = True, 0, 0

    def _make_engine(self, chains, device=0, **group_kw):
        self.made.append((chains, device, group_kw))
        return _FakeEngine(chains, self.target.d, self.target, [])

    def _stats_from_engine(self, eng, lo, n):
        return {"tree_size": np.zeros((eng.chains, n))}


def _sample(target, step, **kw):
    args = dict(draws=3, tune=2, step=step, start=np.zeros(target.d), progressbar=False, stream_results=False, random_seed=1)
    args.update(kw)
    return sampling.sample(target, target.d, **args)


def test_sample_requires_a_multiple_of_the_groups_up_front():
    b = T.Batched([T.AR1(4, rho=r) for r in (0.1, 0.2, 0.3)])
    step = _FakeStep(b)
    for chains in (2, 4, 7):
        with pytest.raises(ValueError, match="multiple of 3"):
            _sample(b, step, chains=chains, devices=[0])
    assert step.made == []                                                     # refused before any engine


def test_sample_refuses_the_pooled_potential():
    b = T.Batched([T.AR1(4, rho=r) for r in (0.1, 0.2)])
    step = _FakeStep(b, potential=lmc.QuadPotentialFullPooled(4))
    with pytest.raises(NotImplementedError, match="Pooled"):
        _sample(b, step, chains=64, devices=[0])
    assert step.made == []


def test_sample_distributed_refuses_a_batched_target():
    from littlemcmc_amd.distributed import sample_distributed

    with pytest.raises(NotImplementedError, match="Batched"):
        sample_distributed(T.Batched([T.AR1(4), T.AR1(4, 0.5)]), 4, chains=4)


def test_make_engines_hands_every_block_its_first_chain():
    from littlemcmc_amd.distributed import chain_block

    b = T.Batched([T.AR1(4, rho=r) for r in (0.1, 0.2, 0.3)])
    step = _FakeStep(b)
    eng = sampling._make_engines(step, 6, [0, 0], 2)                           # blocks 3 + 3: group 1 spans both engines
    assert step.made == [(3, 0, {"first_chain": 0, "chains_per_group": 2}), (3, 0, {"first_chain": 3, "chains_per_group": 2})]
    assert eng.chains == 6
    step = _FakeStep(b)
    sampling._make_engines(step, 21, [0, 1, 2, 3], 7)
    assert [(m[0], m[2]["first_chain"]) for m in step.made] == [(hi - lo, lo) for lo, hi in (chain_block(21, k, 4) for k in range(4))]
    assert all(m[2]["chains_per_group"] == 7 for m in step.made) and [m[1] for m in step.made] == [0, 1, 2, 3]
    # one device: the whole job from chain 0; any other target: the arguments engines were always made with
    step = _FakeStep(b)
    sampling._make_engines(step, 6, [2], 2)
    assert step.made == [(6, 2, {"first_chain": 0, "chains_per_group": 2})]
    step = _FakeStep(T.AR1(4))
    sampling._make_engines(step, 6, [0, 1])
    assert step.made == [(3, 0, {}), (3, 1, {})]


def test_sample_deals_blocks_through_the_whole_path(monkeypatch):
    """sample(devices=[0, 0, 0]) with 7 chains per group and G = 3: the engines get blocks 7 + 7 + 7 here, 3 + 3 with two
    devices and 6 chains; the residency probe (no devices given) is a one-chain engine that still knows its group size."""
    b = T.Batched([T.AR1(4, rho=r) for r in (0.1, 0.2, 0.3)])
    step = _FakeStep(b)
    trace, stats = _sample(b, step, chains=6, devices=[0, 0])
    assert trace.shape == (6, 3, 4)
    assert [(m[0], m[2]) for m in step.made] == [(3, {"first_chain": 0, "chains_per_group": 2}),
                                                 (3, {"first_chain": 3, "chains_per_group": 2})]
    monkeypatch.setattr(sampling, "visible_devices", lambda: 2)
    step = _FakeStep(b)
    _sample(b, step, chains=6)
    assert step.made[0] == (1, 0, {"first_chain": 0, "chains_per_group": 2})   # the probe
    assert step.made[1:] == [(6, 0, {"first_chain": 0, "chains_per_group": 2})]


def test_step_objects_refuse_one_chain_calls_on_a_batched_target():
    b = T.Batched([T.AR1(4, rho=r) for r in (0.1, 0.2)])
    step = lmc.NUTS(b, 4)
    with pytest.raises(ValueError, match=r"batched\[g\]"):
        step._engine()
    with pytest.raises(ValueError, match=r"batched\[g\]"):
        step._astep(np.zeros(4))


def test_batched_user_targets_compile_one_code_object():
    """hiprtc needs no device: two UserTarget.separable members yield ONE code object -- the cache file of member 0."""
    members = [_student(7, 3.0), _student(7, 8.0)]
    b = T.Batched(members)
    got = b.kernels_for(1, 1, 1)
    assert got is members[0].kernels_for(1, 1, 1) and members[1]._code == {}
    cache = os.path.join(os.path.dirname(os.path.abspath(T.__file__)), "_user_targets")
    name = "user_%s_1_1_1.hsaco" % members[0]._digest("hiprtc")
    assert os.path.exists(os.path.join(cache, name))
    assert members[1]._digest("hiprtc") == members[0]._digest("hiprtc")       # member 1 alone would fetch the same file
    assert got[0][:4] == b"\x7fELF" and "run_kernel" in got[1]
