"""-m gpu: sample(thin=k) keeps every k-th draw, from the kernel's store to the returned arrays. Every case runs the same
seeded job twice -- thin=1 and thin=k -- and the thinned result must be bit for bit ``full[:, ::k]``: trace and every
statistic, in every kernel family, result mode and launch layout. 16 chains, tune=7, draws=23 (no multiple of any k used)."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T

pytestmark = pytest.mark.gpu
CHAINS, TUNE, DRAWS = 16, 7, 23
_full_cache = {}


def _job(make, thin, chains=CHAINS, **kw):
    """One seeded job; ``make()`` -> (target, model_ndim, step or None, extra sample() keywords): fresh objects per run."""
    tgt, d, step, extra = make()
    args = dict(draws=DRAWS, tune=TUNE, chains=chains, random_seed=11, progressbar=False, step=step)
    args.update(extra)
    args.update(kw)
    return lmc.sample(tgt, d, thin=thin, **args)


def _full(key, make, **kw):
    """The unthinned job of a case, computed once and shared (never modified)."""
    key = (key,) + tuple(sorted(kw.items()))
    if key not in _full_cache:
        trace, stats = _job(make, 1, **kw)
        trace.setflags(write=False)
        _full_cache[key] = (trace, stats)
    return _full_cache[key]


def _assert_thinned(got, full, k, lo_rows):
    (trace, stats), (ftrace, fstats) = got, full
    rows = -(-lo_rows // k)
    assert trace.shape == (ftrace.shape[0], rows, ftrace.shape[2])
    assert np.array_equal(trace, ftrace[:, ::k])
    assert set(stats) == set(fstats)
    for name in fstats:
        assert stats[name].shape == (ftrace.shape[0], rows, 1), name
        assert stats[name].dtype == fstats[name].dtype, name
        assert np.array_equal(stats[name], fstats[name][:, ::k], equal_nan=True), name


def _std3():
    return T.StdNormal(3), 3, None, {}


@pytest.mark.parametrize("launch_iters", [4, 9, None])
@pytest.mark.parametrize("discard", [True, False])
@pytest.mark.parametrize("stream", ["direct", "windows", False])
@pytest.mark.parametrize("k", [2, 5, 7, 40])
def test_fused_nuts_thinned_equals_the_slice(k, stream, discard, launch_iters):
    kw = dict(stream_results=stream, discard_tuned_samples=discard, launch_iters=launch_iters)
    full = _full("std3", _std3, discard_tuned_samples=discard)     # (modes and launch layouts are bit-identical: test_gpu_round6)
    got = _job(_std3, k, **kw)
    _assert_thinned(got, full, k, DRAWS if discard else TUNE + DRAWS)
    if k == 40:
        assert got[0].shape[1] == 1


def _prec(d):
    return np.linspace(0.5, 2.0, d)


def _ar_cov(d):
    idx = np.arange(d)
    return 0.5 ** np.abs(idx[:, None] - idx[None, :])


def _torch_std(d):
    return T.TorchTarget(d, lambda q: (-0.5 * (q * q).sum(dim=1), -q))


FAMILIES = {
    "one_wave_ns2_ar1_128": lambda: (T.AR1(128, 0.9), 128, None, {}),
    "one_wave_ns4_funnel_200": lambda: (T.Funnel(200), 200, None, {}),
    "four_wave_team_diag_600": lambda: (T.DiagGaussian(_prec(600)), 600, None, {}),
    "general_kernels_1100": lambda: (T.StdNormal(1100), 1100, None, {}),
    "shared_dense_16": lambda: (T.AR1(16, 0.5), 16, lmc.NUTS(T.AR1(16, 0.5), 16, potential=lmc.QuadPotentialFull(_ar_cov(16))), {}),
    "adaptive_dense_10": lambda: (T.AR1(10, 0.5), 10, lmc.NUTS(T.AR1(10, 0.5), 10, potential=lmc.QuadPotentialFullAdapt(
        10, np.zeros(10), np.eye(10), 10, adaptation_window=3)), {}),
    "fused_hmc_10": lambda: (T.StdNormal(10), 10, lmc.HamiltonianMC(T.StdNormal(10), 10, path_length=1.0), {}),
    "counter_stream_16": lambda: (T.StdNormal(16), 16, lmc.NUTS(T.StdNormal(16), 16, rng="counter"), {}),
    "run_time_compiled_16": lambda: (T.UserTarget.separable(16, logp="-0.5*q*q", grad="-q"), 16, None, {}),
    "tick_kernel_torch_16": lambda: (_torch_std(16), 16, None, {}),
    "host_step_rand_8": lambda: (T.StdNormal(8), 8, lmc.NUTS(T.StdNormal(8), 8, step_rand=lambda s: 0.9 * s), {}),
    "pooled_dense_4": lambda: (T.AR1(4, 0.5), 4, None, dict(init="adapt_full_pooled", chains=64)),   # 64 * 8 > 4
    # tune = 7 has no adaptation window (pooled_windows: none below 20); with 40 the job is cut into snapshot launches
    "pooled_dense_4_with_windows": lambda: (T.AR1(4, 0.5), 4, None, dict(init="adapt_full_pooled", chains=64, tune=40)),
}


def _shape(ns, w):
    return lambda eng, step: not eng.wide and eng.kernel_shape()[1:] == (ns, w) and eng.last_run_dense_kernel() is None


# what makes a case the family its name says: asked of the engine (and step) the thinned job ran on
RAN_ON = {
    "one_wave_ns2_ar1_128": _shape(2, 1),
    "one_wave_ns4_funnel_200": _shape(4, 1),
    "four_wave_team_diag_600": _shape(4, 4),
    "general_kernels_1100": lambda eng, step: eng.wide,
    "shared_dense_16": lambda eng, step: not eng.wide and eng.last_run_dense_kernel() == "shared",
    "adaptive_dense_10": lambda eng, step: not eng.wide and eng.last_run_dense_kernel() == "per_chain",
    "fused_hmc_10": lambda eng, step: eng.kind == "hmc" and _shape(1, 1)(eng, step),
    "counter_stream_16": lambda eng, step: eng.rng == "counter" and _shape(1, 1)(eng, step),
    "run_time_compiled_16": lambda eng, step: eng.target.family == _abi.TARGET_USER and _shape(1, 1)(eng, step),
    "tick_kernel_torch_16": lambda eng, step: eng.target.family == _abi.TARGET_EXTERNAL and eng.ticks > 0,
    "host_step_rand_8": lambda eng, step: step._host_step_rand() is not None and _shape(1, 1)(eng, step),
    "pooled_dense_4": lambda eng, step: eng.last_run_dense_kernel() is not None,
    "pooled_dense_4_with_windows": lambda eng, step: eng.last_run_dense_kernel() is not None,
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_kernel_family_thinned_equals_the_slice(family):
    k, make = 3, FAMILIES[family]
    full = _full(family, make)
    tgt, d, step, extra = make()
    made = {"step": step}
    trace, stats, eng = _job(lambda: (tgt, d, made["step"], extra), k, return_engine=True)
    try:
        assert RAN_ON[family](eng, made["step"]), family
    finally:
        eng.close()
    _assert_thinned((trace, stats), full, k, DRAWS)
    assert trace.shape[0] == extra.get("chains", CHAINS) and np.isfinite(trace).all()


def test_the_second_pooled_case_runs_snapshot_launches():
    """The pooled cases above: tune = 7 has no adaptation window, tune = 40 has (its launches are cut by snapshots)."""
    assert not lmc.sampling.pooled_windows(TUNE) and lmc.sampling.pooled_windows(40)


def test_keep_moments_see_every_draw():
    res = {}
    for k in (1, 3):
        _tr, _st, eng = _job(_std3, k, keep_moments=True, return_engine=True)
        try:
            res[k] = eng.moments()
        finally:
            eng.close()
    for a, b in zip(res[1], res[3]):
        assert np.array_equal(a, b)
    assert (res[3][2] == DRAWS).all()


def test_counters_and_tuned_stats_see_every_iteration():
    CT = [_abi.CT_SAMPLES_AFTER_TUNE, _abi.CT_DIVS_AFTER_TUNE, _abi.CT_REACHED_MAX_TREEDEPTH, _abi.CT_LEAPFROGS]
    res = {}
    for k in (1, 3):
        step = lmc.NUTS(T.StdNormal(3), 3)
        _tr, _st, eng = _job(lambda: (T.StdNormal(3), 3, step, {}), k, return_engine=True)
        try:
            res[k] = (eng.stat_f64(_abi.STAT_ACCEPT, 0, TUNE + DRAWS), list(step.step_adapt._tuned_stats), eng.counters()[:, CT].copy(),
                      step._samples_after_tune, step.iter_count)
        finally:
            eng.close()
    assert res[3][0].shape == (CHAINS, TUNE + DRAWS) and np.array_equal(res[1][0], res[3][0])
    assert len(res[3][1]) == DRAWS and res[1][1] == res[3][1]
    assert np.array_equal(res[1][2], res[3][2]) and res[1][3:] == res[3][3:]


@pytest.mark.parametrize("stream", ["direct", "windows", False])
def test_two_engine_group_equals_one_engine(stream):
    k = 3
    one = _job(_std3, k, device=0, stream_results=stream)
    two = _job(_std3, k, devices=[0, 0], stream_results=stream)
    assert np.array_equal(one[0], two[0])
    for name in one[1]:
        assert np.array_equal(one[1][name], two[1][name], equal_nan=True), name
    _assert_thinned(two, _full("std3", _std3, discard_tuned_samples=True), k, DRAWS)
    _tr, _st, grp = _job(_std3, k, devices=[0, 0], stream_results="windows", return_engine=True)
    try:
        assert type(grp).__name__ == "EngineGroup"
        assert (grp.keep_trace, grp.trace_begin, grp.thin, grp.trace_rows()) == (True, TUNE, k, -(-DRAWS // k))
        assert all((e.keep_trace, e.trace_begin, e.thin) == (True, TUNE, k) for e in grp.engines)
        assert np.array_equal(grp.trace(), one[0])
    finally:
        grp.close()


@pytest.mark.parametrize("discard", [True, False])
def test_interrupted_job_returns_the_prefix_of_kept_rows(discard):
    """A callback that raises KeyboardInterrupt once (a host step_rand job calls it once per iteration, as in
    tests/test_gpu_round5.py): the returned arrays are the first m rows of the uninterrupted thinned run, with
    m = ceil(max(iter_count - lo, 0) / k) -- whatever iter_count turns out to be."""
    k, d = 3, 8
    make = FAMILIES["host_step_rand_8"]
    whole = _job(make, k, discard_tuned_samples=discard)
    fired = []

    def cb(trace, draw):
        if not fired and draw.iteration >= 17:
            fired.append(draw.iteration)
            raise KeyboardInterrupt

    tgt, _d, step, _extra = make()
    trace, stats = lmc.sample(tgt, d, draws=DRAWS, tune=TUNE, chains=CHAINS, random_seed=11, progressbar=False, step=step,
                              thin=k, discard_tuned_samples=discard, callback=cb)
    lo = TUNE if discard else 0
    m = -(-max(step.iter_count - lo, 0) // k)
    print("interrupted at %s: iter_count %d, %d rows" % (fired, step.iter_count, m))
    assert fired and 0 < step.iter_count < TUNE + DRAWS
    assert trace.shape == (CHAINS, m, d)
    assert np.array_equal(trace, whole[0][:, :m])
    for name in whole[1]:
        assert stats[name].shape == (CHAINS, m, 1), name
        assert np.array_equal(stats[name], whole[1][name][:, :m], equal_nan=True), name


@pytest.mark.parametrize("stream", ["direct", "windows"])
def test_interrupted_streamed_job_returns_the_prefix_of_kept_rows(stream):
    """The same through the device job loop with streamed results (the interrupt of tests/test_gpu_round6.py: raised from the
    callback once the device reports iteration 50 of a 20 060-iteration job in launches of 25): the returned arrays are views
    of the first m = ceil(iter_count / k) rows of the streamed arrays, and equal the uninterrupted thinned job's rows."""
    k, d, chains, tune = 7, 24, 300, 60
    tgt = T.StdNormal(d)
    kw = dict(tune=tune, chains=chains, random_seed=8, progressbar=False, discard_tuned_samples=False, launch_iters=25, thin=k)

    def fresh_step():
        return lmc.init_nuts(tgt, d, random_seed=lmc.sampling._derive_seeds(8, chains))[1]

    whole = lmc.sample(tgt, d, draws=60, step=fresh_step(), stream_results=False, **kw)

    def stop_at_50(trace, draw):
        if draw.iteration >= 50:
            raise KeyboardInterrupt

    step = fresh_step()
    trace, stats = lmc.sample(tgt, d, draws=20000, step=step, stream_results=stream, callback=stop_at_50, **kw)
    m = -(-step.iter_count // k)
    print("interrupted: iter_count %d, %d rows" % (step.iter_count, m))
    assert 25 <= step.iter_count < 20060
    assert trace.shape == (chains, m, d)
    n = min(m, whole[0].shape[1])
    assert n >= 4 and np.array_equal(trace[:, :n], whole[0][:, :n])
    for name in whole[1]:
        assert stats[name].shape == (chains, m, 1), name
        assert np.array_equal(stats[name][:, :n], whole[1][name][:, :n], equal_nan=True), name


@pytest.mark.parametrize("k", [2, 5, 40])
def test_memory_only_the_kept_rows_exist(k):
    lib = _abi.load()
    rows = -(-DRAWS // k)
    trace, _st, eng = _job(_std3, k, stream_results="windows", return_engine=True)
    try:
        assert lib.lmc_engine_trace_rows(eng._h) == rows == eng.trace_rows() and lib.lmc_engine_thin(eng._h) == k
        assert np.array_equal(eng.trace(), trace)
        from littlemcmc_amd import diagnostics as dg

        assert np.array_equal(dg.trace_tensor(eng).cpu().numpy(), trace)
    finally:
        eng.close()
    trace, _st, eng = _job(_std3, k, stream_results="direct", return_engine=True)
    try:
        assert trace.shape == (CHAINS, rows, 3) and eng._trace_out is not None
        assert np.shares_memory(trace, eng._trace_out) and trace.ctypes.data == eng._trace_out.ctypes.data
        assert int(lib.lmc_engine_trace_device_ptr(eng._h) or 0) != 0 and lib.lmc_engine_trace_rows(eng._h) == rows
    finally:
        eng.close()


def test_engine_level_thinned_reserve_and_strided_window():
    """Below sample(): reserve(thin=k) + run in uneven launches; trace() windows and a strided window copy into device-accessible
    arrays deliver the kept iterations; the stat getters still return every iteration."""
    from littlemcmc_amd.engine import StreamedResults, thin_window

    d, chains, n, lo, k = 5, 9, 30, 4, 4
    out = {}
    for thin in (1, k):
        step = lmc.NUTS(T.StdNormal(d), d)
        eng = step._make_engine(chains)
        try:
            eng.seed(np.arange(chains) + 3)
            eng.set_position(np.zeros((chains, d)))
            eng.reset_tuning()
            eng.reserve(n, keep_trace=True, trace_begin=lo, thin=thin)
            res = StreamedResults(chains, thin_window(lo, n - lo, lo, thin)[1], lo, d, step._result_planes(), thin=thin)
            at = 0
            for size in (1, 6, 2, 9, 5, 7):
                eng.run(10, at, size)
                a, b = max(at, lo), at + size
                if b > a:
                    eng.copy_window_async(res, a, b - a)
                at += size
            assert at == n
            eng.synchronize()
            eng.copy_wait()
            out[thin] = (eng.trace().copy(), eng.trace(9, 13).copy(), res.trace.copy(), {m: v.copy() for m, v in res.stats.items()},
                         eng.stat_i32(_abi.STAT_TREE_SIZE, 0, n).copy())
        finally:
            eng.close()
    full, thinned = out[1], out[k]
    assert thinned[0].shape == (chains, -(-(n - lo) // k), d)
    assert np.array_equal(thinned[0], full[0][:, ::k])
    kept = [it for it in range(lo, n, k) if 9 <= it < 22]
    assert np.array_equal(thinned[1], full[0][:, [it - lo for it in kept]])
    assert np.array_equal(thinned[2], thinned[0]) and np.array_equal(full[2], full[0])
    for name in full[3]:
        assert np.array_equal(thinned[3][name], full[3][name][:, ::k], equal_nan=True), name
    assert np.array_equal(thinned[4], full[4])
