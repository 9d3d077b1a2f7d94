"""thin=k without a GPU: the row arithmetic every launch's kernel arguments, every window copy and the collector come from
(engine.thin_window on the host, lmc_thin_window in the library) against numpy slicing; sample()'s argument check; the new
entry points and their validation before any HIP call."""
import ctypes
import itertools

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T
from littlemcmc_amd.engine import thin_window

NEW_SYMBOLS = ("lmc_engine_reserve_thinned", "lmc_engine_thin", "lmc_engine_trace_rows", "lmc_thin_window",
               "lmc_engine_copy_window_strided_async")


def _lib_window(lib, first, n, lo, k):
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.lmc_thin_window(first, n, lo, k, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == _abi.OK
    return a.value, b.value, c.value


def _splits(n_total, sizes=range(1, 8)):
    """Every way to cut [0, n_total) into consecutive launches of 1..7 iterations: [(first, n), ...] per split."""
    def rec(at):
        if at == n_total:
            yield []
            return
        for n in sizes:
            if at + n <= n_total:
                for rest in rec(at + n):
                    yield [(at, n)] + rest
    return rec(0)


def test_row_arithmetic_equals_numpy_slicing_for_every_launch():
    """In the place of enumerating every split of [0, n_total) for every n_total <= 20 (half a million splits at 20, times 56
    (lo, k) pairs): whole splits are enumerated literally up to n_total = 12 in the next test, and here, for
    all lo <= 6, n_total <= 20, k <= 8: what a launch [first, first + n) addresses depends on (first, n) alone, so
    every launch of 1..7 iterations is checked against the slice -- the kept iterations are those of range(lo, n_total)[::k]
    inside the launch and their rows are their indices in that list -- and a split of the job is a sequence of such
    launches: their rows concatenate to 0, 1, 2, ... (each kept iteration once, in order). Host function and library agree."""
    lib = _abi.load()
    for lo, n_total, k in itertools.product(range(7), range(21), range(1, 9)):
        kept = list(range(lo, n_total)[::k])
        assert kept == list(np.arange(n_total)[lo::k])
        for first in range(n_total):
            for n in range(1, min(7, n_total - first) + 1):
                fk, nk, fr = thin_window(first, n, lo, k)
                assert (fk, nk, fr) == _lib_window(lib, first, n, lo, k)
                inside = [it for it in kept if first <= it < first + n]
                assert [fk + j * k for j in range(nk)] == inside, (lo, n_total, k, first, n)
                if inside:
                    assert fr == kept.index(inside[0])
                else:   # nothing kept: the row the NEXT kept iteration will take
                    assert fr == len([it for it in kept if it < first])
        # the whole job as one window: the shape sample() returns
        assert thin_window(lo, max(n_total - lo, 0), lo, k)[1] == len(kept) == -(-max(n_total - lo, 0) // k)


@pytest.mark.parametrize("n_total", [0, 1, 7, 12])
def test_every_split_addresses_each_kept_row_once_and_in_order(n_total):
    """Literally every split of [0, n_total) into launches of sizes 1-7 (2^11 of them at n_total = 12), all lo <= 6, k <= 8."""
    splits = list(_splits(n_total))
    assert len(splits) == (1 if n_total == 0 else {1: 1, 7: 64, 12: 2000}[n_total])
    for lo, k in itertools.product(range(7), range(1, 9)):
        want_iters = list(range(lo, n_total)[::k])
        for split in splits:
            iters, rows = [], []
            for first, n in split:
                fk, nk, fr = thin_window(first, n, lo, k)
                iters += [fk + j * k for j in range(nk)]
                rows += [fr + j for j in range(nk)]
            assert iters == want_iters and rows == list(range(len(want_iters))), (lo, k, split)


def test_the_kernels_rule_stores_the_slice():
    """What the fused, dense and general kernels do with a launch's window (lmc_sampler.hpp: launch_trace_row), replayed on
    the host: one counter `kept` per launch, iteration `it` of the launch is stored iff it == keep_first + kept * thin, into
    row trace_row0 + kept. Over every launch layout of fixed size 1..7 the stored (iteration, row) pairs are the slice's."""
    for lo, n_total, k, size in itertools.product(range(7), (0, 1, 13, 20), range(1, 9), range(1, 8)):
        stored = []
        for first in range(0, n_total, size):
            n = min(size, n_total - first)
            fk, nk, row0 = thin_window(first, n, lo, k)
            keep_first = fk - first if nk > 0 else 2 ** 31 - 1     # lmc_engine.hip: set_launch_window
            kept = 0
            for it in range(n):
                if it == keep_first + kept * k:
                    stored.append((first + it, row0 + kept))
                    kept += 1
            assert kept == nk
        assert stored == [(it, r) for r, it in enumerate(range(lo, n_total)[::k])], (lo, n_total, k, size)


@pytest.mark.parametrize("n_total", [20])
def test_random_splits_of_the_largest_job(n_total):
    rs = np.random.RandomState(5)
    for _ in range(300):
        lo, k = int(rs.randint(0, 7)), int(rs.randint(1, 9))
        at, rows, iters = 0, [], []
        while at < n_total:
            n = min(int(rs.randint(1, 8)), n_total - at)
            fk, nk, fr = thin_window(at, n, lo, k)
            iters += [fk + j * k for j in range(nk)]
            rows += [fr + j for j in range(nk)]
            at += n
        assert iters == list(range(lo, n_total)[::k]) and rows == list(range(len(iters)))


def test_interrupted_prefix_is_the_kept_rows_below_n_done():
    """An interrupted job returns ceil(max(n_done - lo, 0) / k) rows: the kept iterations every chain completed."""
    for lo, k, n_done in itertools.product(range(7), range(1, 9), range(21)):
        m = thin_window(lo, max(n_done - lo, 0), lo, k)[1]
        assert m == -(-max(n_done - lo, 0) // k) == len(range(lo, n_done)[::k])


def test_thin_window_rejects_nonsense():
    lib = _abi.load()
    for bad in ((0, 3, 0, 0), (-1, 3, 0, 1), (0, -1, 0, 1), (0, 3, -1, 1)):
        with pytest.raises(ValueError):
            thin_window(*bad)
        assert lib.lmc_thin_window(*bad, None, None, None) == 1   # LMC_ERR_INVALID


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3", None])
def test_sample_rejects_a_bad_thin_before_any_library_call(monkeypatch, bad):
    """0, negatives, non-integral floats and bool raise ValueError naming ``thin`` -- before the library is even loaded."""
    def no_library(*a, **kw):
        raise AssertionError("the library was entered before thin was checked")

    monkeypatch.setattr(_abi, "load", no_library)
    with pytest.raises(ValueError, match="thin"):
        lmc.sample(T.StdNormal(3), 3, draws=5, tune=5, chains=2, random_seed=1, progressbar=False, thin=bad)


def test_thin_is_an_explicit_keyword_of_sample():
    import inspect

    p = inspect.signature(lmc.sample).parameters["thin"]
    assert p.default == 1 and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    from littlemcmc_amd.sampling import _check_thin

    assert _check_thin(1) == 1 and _check_thin(np.int64(7)) == 7 and type(_check_thin(np.int32(2))) is int


def test_new_entry_points_are_exported_and_validate_without_a_gpu():
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.lmc_abi_version() == 9        # additive: the ABI number stays
    # thin < 1 is refused before any HIP call (no engine is needed to see it, like the lds_plan validation)
    for thin in (0, -3):
        assert lib.lmc_engine_reserve_thinned(None, 10, 0, thin) == 1 and b"thin must be >= 1" in lib.lmc_last_error(None)
    assert lib.lmc_engine_thin(None) == 1 and lib.lmc_engine_trace_rows(None) == 0
    assert lib.lmc_engine_copy_window_strided_async(None, None, 0, 1, 0) == 1 and b"stride must be >= 1" in lib.lmc_last_error(None)


def test_result_mode_threshold_sees_the_thinned_size():
    """stream_results=True streams only results of at least 8 MiB: the thinned row count is what counts."""
    from littlemcmc_amd.sampling import _result_mode

    kw = dict(return_engine=False, host_rand=False, external=False, has_planes=True, chains=1024, model_ndim=16)
    full_rows = 1000
    assert _result_mode(True, n_out=full_rows, **kw) == "direct"
    assert _result_mode(True, n_out=thin_window(0, full_rows, 0, 50)[1], **kw) is None


def test_streamed_results_hold_the_kept_rows():
    from littlemcmc_amd.engine import StreamedResults

    planes = lmc.NUTS(T.StdNormal(3), 3)._result_planes()
    out = StreamedResults(4, thin_window(7, 23, 7, 5)[1], 7, 3, planes, pinned=False, thin=5)
    assert out.trace.shape == (4, 5, 3) and out.stats["depth"].shape == (4, 5) and out.thin == 5
    w = out.window_dst(None)
    assert (w.n_out, w.first) == (5, 7)
