"""rng="counter" without a GPU: the host model of the counter-based streams (tests/_counter_model.py) against Philox's
published known-answer vectors, the properties of the decision uniforms, the ABI additions, the refusals that
lmc_engine_create makes before any HIP call, the host keyword, and the oracle running on the model's stream."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T
from oracle import lmc_oracle as orc
from oracle import targets as OT
from tests import _counter_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()


def _hex(words):
    return " ".join("%08x" % w for w in words)


def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32-10."""
    assert _hex(cm.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(cm.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(cm.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_decision_uniforms_are_the_stated_function_of_seed_iteration_and_index():
    seed, git = 123456789, 17
    u = cm.uniforms(seed, git, 300)
    assert np.all((u >= 0.0) & (u < 1.0)) and len(set(u.tolist())) == 300
    # u_0 and u_1 are the two halves of ONE block: counter (git, git >> 32, k >> 1, "lmcu"), key (seed, 0x4d4f4d31)
    w = cm.philox4x32_10((git, 0, 0, 0x6C6D6375), (seed, 0x4D4F4D31))
    assert u[0] == ((w[0] >> 5) * 2.0 ** 26 + (w[1] >> 6)) / 2.0 ** 53
    assert u[1] == ((w[2] >> 5) * 2.0 ** 26 + (w[3] >> 6)) / 2.0 ** 53
    w1 = cm.philox4x32_10((git, 0, 1, 0x6C6D6375), (seed, 0x4D4F4D31))
    assert u[2] == cm.words_to_unit(w1[0], w1[1]) and u[3] == cm.words_to_unit(w1[2], w1[3])
    # the largest words stay below 1
    assert cm.words_to_unit(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and cm.words_to_unit(0, 0) == 0.0
    # iterations 2^32 - 1 and 2^32 differ in c1 (and in c0): the 64-bit iteration index is the counter's low half
    lo, hi = 2 ** 32 - 1, 2 ** 32
    assert cm.uniform_block(seed, lo, 5) == cm.philox4x32_10((0xFFFFFFFF, 0, 5, cm.C3_UNIFORMS), (seed, cm.KEY1))
    assert cm.uniform_block(seed, hi, 5) == cm.philox4x32_10((0, 1, 5, cm.C3_UNIFORMS), (seed, cm.KEY1))
    assert cm.uniform_block(seed, hi, 5) != cm.uniform_block(seed, 0, 5)
    # the momentum stream lives in another counter space (c3)
    assert cm.C3_MOMENTUM != cm.C3_UNIFORMS
    z = cm.normals(seed, git, 65)
    assert z.shape == (65,) and np.all(np.isfinite(z)) and cm.run_shape(65) == (2, 1)
    assert [cm.run_shape(d) for d in (1, 64, 128, 200, 256, 300, 600, 1024)] == \
        [(1, 1), (1, 1), (2, 1), (4, 1), (4, 1), (4, 2), (4, 4), (4, 4)]


def test_abi_has_the_mode_and_the_inspection_entry_point():
    consts = dict(re.findall(r"#define\s+(LMC_\w+)\s+(\d+)", HEADER))
    assert int(consts["LMC_RNG_COUNTER"]) == 2 == _abi.RNG_COUNTER
    assert int(consts["LMC_RNG_NUMPY"]) == _abi.RNG_NUMPY and int(consts["LMC_RNG_PHILOX"]) == _abi.RNG_PHILOX
    assert re.search(r"^int\s+lmc_engine_counter_draws\s*\(lmc_engine\*\s*e,\s*int64_t\s+iteration,\s*double\*\s*normals,"
                     r"\s*double\*\s*uniforms,\s*int32_t\s+n_uniforms\);", HEADER, re.M)
    assert "lmc_engine_counter_draws" in _abi.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "lmc_engine_counter_draws")
    lib = _abi.load()
    assert lib.lmc_engine_counter_draws.argtypes[1] is ctypes.c_int64
    assert lib.lmc_engine_counter_draws(None, 0, None, None, 0) == 1 and b"null engine" in lib.lmc_last_error(None)


def _create(**fields):
    lib = _abi.load()
    cfg = _abi.Config()
    lib.lmc_config_defaults(ctypes.byref(cfg), 4, fields.pop("dim", 16))
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = lib.lmc_engine_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = (lib.lmc_last_error(None) or b"").decode()
    if rc == _abi.OK:
        lib.lmc_engine_destroy(h)
    return rc, msg


def test_refusals_come_before_any_hip_call():
    """(No GPU is needed to see them: like the lds_plan validation of tests/test_abi_cpu.py.)"""
    rc, msg = _create(rng_mode=3)
    assert rc == 1 and "unknown rng_mode 3" in msg
    rc, msg = _create(rng_mode=_abi.RNG_COUNTER, potential=_abi.POT_FULL)
    assert rc == 1 and "LMC_RNG_COUNTER" in msg
    rc, msg = _create(rng_mode=_abi.RNG_COUNTER, target_family=_abi.TARGET_EXTERNAL)
    assert rc == 1 and "LMC_RNG_COUNTER" in msg
    rc, msg = _create(rng_mode=_abi.RNG_COUNTER, dim=2000)            # the general kernels
    assert rc == 1 and "LMC_RNG_COUNTER" in msg
    rc, msg = _create(rng_mode=_abi.RNG_COUNTER, mass_f64=1)          # the general kernels
    assert rc == 1 and "LMC_RNG_COUNTER" in msg
    rc, msg = _create(rng_mode=_abi.RNG_PHILOX, dim=2000)             # the momentum-only mode keeps its own name
    assert rc == 1 and "LMC_RNG_PHILOX" in msg


def test_steps_take_the_keyword():
    tgt = T.StdNormal(8)
    step = lmc.NUTS(tgt, 8, rng="counter")
    assert step._engine_kwargs()["rng"] == "counter"
    assert lmc.HamiltonianMC(tgt, 8, rng="counter")._engine_kwargs()["rng"] == "counter"
    assert lmc.NUTS(tgt, 8)._engine_kwargs()["rng"] == "numpy"                            # the default is unchanged
    assert lmc.NUTS(tgt, 8, momentum_rng="philox")._engine_kwargs()["rng"] == "philox"    # ... and so is momentum_rng
    assert lmc.NUTS(tgt, 8, momentum_rng="philox", rng="counter")._engine_kwargs()["rng"] == "counter"
    assert lmc.HamiltonianMC(tgt, 8)._engine_kwargs()["rng"] == "numpy"
    for cls in (lmc.NUTS, lmc.HamiltonianMC):
        with pytest.raises(ValueError, match="rng"):
            cls(tgt, 8, rng="mt")
    _start, s2 = lmc.init_nuts(tgt, 8, random_seed=[1, 2], rng="counter")
    assert s2._engine_kwargs()["rng"] == "counter"
    back = pickle.loads(pickle.dumps(step))
    assert back._engine_kwargs()["rng"] == "counter"


def test_user_target_compiles_the_counter_kernel_without_a_gpu():
    from littlemcmc_amd.targets import UserTarget

    t = UserTarget.separable(16, logp="-0.5*q*q", grad="-q")
    code, run, traj, logp, run1 = t.kernels_for(1, 1, 1, counter=True)
    assert code[:4] == b"\x7fELF" and "run_kernel" in run and run1 is None          # one layout: no plan-1 kernel
    assert run != t.kernels_for(1, 1, 1)[1]                                           # not the parity kernel's name
    with pytest.raises(ValueError, match="counter"):
        t.kernels_for(1, 1, 16, general=True, counter=True)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_the_oracle_runs_on_the_counter_stream(kind):
    """oracle/lmc_oracle.py only ever calls rng.normal(size=), rng.uniform(), rng.uniform(lo, hi) and rng.rand(): a
    CounterRng drives Step.astep unchanged, deterministically, and counts what every iteration consumes."""
    d, n_it, seed = 10, 25, 424242

    def run(step_rand=None):
        f = OT.make("std_normal", d)
        step = orc.Step(f, d, kind=kind, potential=orc.DiagAdaptPotential(d, np.zeros(d), np.ones(d), 10), step_rand=step_rand)
        step.reset_tuning()
        rng = cm.CounterRng(seed, [cm.normals(seed, t, d) for t in range(n_it)])
        q = np.full(d, 0.1)
        qs, sizes = [], []
        for _ in range(n_it):
            q, st = step.astep(q, rng)
            qs.append(q.copy())
            sizes.append(int(np.ravel(st["tree_size"] if kind == "nuts" else st["n_steps"])[0]))
        return np.array(qs), np.array(sizes), rng.finish()

    qs, sizes, used = run()
    qs2, _sizes2, used2 = run()
    np.testing.assert_array_equal(qs, qs2)
    assert used == used2 and len(used) == n_it and np.all(np.isfinite(qs))
    if kind == "hmc":
        assert set(used) <= {1, 2}          # path length, then the acceptance uniform unless the trajectory diverged
    else:
        # one direction per doubling and one uniform per merge: a tree of n leapfrogs consumes at least log2 and fewer than 2 n + depth
        assert all(1 <= u <= 2 * s + 20 for u, s in zip(used, sizes))
    _q, _s, used_j = run(step_rand=(0.8, 1.2))   # the jitter's uniform is k = 0: one more per iteration on its own stream position
    assert len(used_j) == n_it and min(used_j) >= 2


# ---- momentum_rng="philox": MomentumOnlyRng, the oracle's rng of the momentum-only mode ----------------------------------
def test_momentum_only_rng_uniforms_are_numpys_whatever_normals_lie_between():
    """rand() / uniform(lo, hi) are np.random.RandomState(seed)'s values bit for bit, in order, however many normal() calls
    are interleaved; normal() hands out its row and leaves get_state() -- words, position, cached gaussian -- as it was."""
    seed, d, n_it = 987654321, 7, 30
    rows = [np.arange(d) + 100.0 * t for t in range(n_it)]
    rng = cm.MomentumOnlyRng(seed, rows)
    twin = np.random.RandomState(seed)
    plan = np.random.RandomState(1)          # how many uniforms every iteration takes, and of which kind
    want_used = []
    for t in range(n_it):
        before = rng.get_state()
        z = rng.normal(size=d)
        after = rng.get_state()
        np.testing.assert_array_equal(z, rows[t])
        assert z.dtype == np.float64
        np.testing.assert_array_equal(after[1], before[1])
        assert after[2:] == before[2:] and after[3] == 0
        n = int(plan.randint(0, 90))
        for j in range(n):
            if j % 3 == 0:
                assert rng.uniform(0.8, 1.2) == twin.uniform(0.8, 1.2)
            elif j % 3 == 1:
                assert rng.rand() == twin.rand()
            else:
                assert rng.uniform() == twin.random_sample()
        want_used.append(n)
    state, twin_state = rng.get_state(), twin.get_state()
    np.testing.assert_array_equal(state[1], twin_state[1])
    assert state[2:] == twin_state[2:]
    used, crossed = rng.finish()
    assert used == want_used and len(crossed) == n_it
    assert crossed[0] == (want_used[0] > 0)          # a freshly seeded generator sits at 624: its first word twists
    assert sum(crossed) == -(-2 * sum(want_used) // 624)   # every generation begun (no iteration here holds two)
    with pytest.raises(AssertionError):
        cm.MomentumOnlyRng(seed, rows).normal(size=d + 1)
    # the seed is taken as the engine takes it: its low 32 bits
    assert cm.MomentumOnlyRng(seed + 2 ** 32, rows).rand() == np.random.RandomState(seed).rand()


def _pos_after(pos, words):
    """numpy's legacy MT19937 position after ``words`` 32-bit words from ``pos``: the twist is lazy, 624 stays 624."""
    end = pos + words
    return end if end <= 624 else (end - 1) % 624 + 1


@pytest.mark.parametrize("d,n_it,n_tune", [(16, 40, 40), (300, 16, 8)])
def test_the_oracle_runs_on_the_momentum_only_rng(d, n_it, n_tune):
    """A recorded oracle chain (tests/_replay.record_chain, ar1, the model's normals rounded to float32 as the device's are)
    on MomentumOnlyRng: every snapshot's generator state is one a team kernel accepts (even position) with no cached
    gaussian, the state is numpy's own stream at that point, and the twist bookkeeping is the positions' -- iteration t
    crossed a twist exactly if its words do not fit behind its snapshot's position."""
    from tests._replay import record_chain

    seed = 20260928 + d
    f = OT.make("ar1", d)
    start = orc.jitter_start(seed, d)
    rows = [cm.normals(seed, t, d).astype(np.float32).astype(np.float64) for t in range(n_it)]
    rng = cm.MomentumOnlyRng(seed, rows)
    snaps, outs = record_chain(orc.init_nuts(f, d, seeds=[seed])[1], start, rng, n_tune, n_it - n_tune)
    used, crossed = rng.finish()
    assert len(snaps) == len(outs) == len(used) == len(crossed) == n_it
    twin = np.random.RandomState(seed)
    for t in range(n_it):
        name, key, pos, has_gauss, gauss = snaps[t]["rng"]
        assert name == "MT19937" and pos % 2 == 0 and has_gauss == 0 and gauss == 0.0, (t, pos, has_gauss)
        tname, tkey, tpos, _hg, _g = twin.get_state()
        np.testing.assert_array_equal(key, tkey)
        assert pos == tpos
        assert used[t] >= 1
        assert outs[t]["rng_pos"] == _pos_after(pos, 2 * used[t]), t
        assert crossed[t] == (pos + 2 * used[t] > 624), t
        assert crossed[t] == (outs[t]["rng_pos"] != pos + 2 * used[t]), t
        if t + 1 < n_it:
            assert snaps[t + 1]["rng"][2] == outs[t]["rng_pos"]      # nothing between two iterations touches the generator
        twin.random_sample(used[t])
    assert crossed[0] and snaps[0]["rng"][2] == 624
