"""Loader of the test-only probe library (tests/probe/lmc_probe.hip -> tests/probe/liblmc_probe.so): the device primitives
of littlemcmc_amd/csrc behind plain launchers, compiled with the library's own flags so that the code generation is the
product's. Nothing under littlemcmc_amd/ knows about it, and the product library is not touched.

The probe is built by ``__graft_entry__.build()`` (or ``python -m tests._probe``); it is current when the hash stamped into
the binary equals the hash of its sources as they are now (probe source, csrc/, include/lmc_hip.h, flags). Loading is lazy:
importing this module needs neither hipcc nor a GPU. ``LMC_PROBE_LIB`` names another build to load (a variant compiled
around mutated headers, say); it is loaded as it is, without the hash check."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from littlemcmc_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "probe", "lmc_probe.hip")
LIB_NAME = "liblmc_probe.so"
_STAMP = b"LMC_PROBE_HASH="

FAMILIES = {"std_normal": 0, "diag_gaussian": 1, "ar1": 2, "funnel": 3, "normal1d": 4}
# every (NS, W) the product instantiates a density functor for (lmc_engine.hip: unit kernels and LMC_PAIR_SHAPES;
# lmc_wide.hip: the 16-wave team)
LOGP_SHAPES = ([(ns, 1) for ns in (1, 2, 4, 8, 16)] + [(4, 2), (4, 4)] + [(ns, 16) for ns in (1, 2, 4, 8, 16)])
TEAM_WIDTHS = (1, 2, 4, 16)


class ProbeError(RuntimeError):
    pass


def lib_path():
    return os.path.join(HERE, "probe", LIB_NAME)


def source_hash(csrc=None):
    h = hashlib.sha256()
    csrc = csrc or _build.CSRC
    paths = [SOURCE] + [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith(".hpp")]
    paths.append(os.path.join(os.path.dirname(_build.HERE), "include", "lmc_hip.h"))
    for path in paths:
        with open(path, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(_build.HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def binary_hash(path=None):
    try:
        with open(path or lib_path(), "rb") as fh:
            blob = fh.read()
    except OSError:
        return None
    i = blob.find(_STAMP)
    if i < 0:
        return None
    return blob[i + len(_STAMP):blob.find(b"\0", i)].decode("ascii", "replace")


def needs_build(out=None, csrc=None):
    return binary_hash(out or lib_path()) != source_hash(csrc)


def build(out=None, csrc=None, force=False, verbose=False):
    """hipcc tests/probe/lmc_probe.hip with _build.HIPCC_FLAGS and -I csrc (``csrc``: another copy of the headers, for a
    variant build) -> ``out``. Raises on failure."""
    out = out or lib_path()
    if not force and not needs_build(out, csrc):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    cmd = [hipcc] + list(_build.HIPCC_FLAGS) + ['-DLMC_PROBE_HASH="%s"' % source_hash(csrc), "-I", csrc or _build.CSRC,
                                                 SOURCE, "-o", out]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise ProbeError("hipcc failed (%d): %s\n%s\n%s" % (res.returncode, " ".join(cmd), res.stdout, res.stderr))
    return out


_I, _P = C.c_int, C.c_void_p
_SIGNATURES = {
    "lmc_probe_hash": (C.c_char_p, []),
    "lmc_probe_exp": (_I, [_I, _P, _P, _I]),
    "lmc_probe_log_unit": (_I, [_P, _P, _I]),
    "lmc_probe_sum6": (_I, [_P, _P, _I]),
    "lmc_probe_team_rows": (_I, [_P, _P, _P]),
    "lmc_probe_team": (_I, [_I, _I, _I, _P, _P, _P]),
    "lmc_probe_logp": (_I, [_I, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
}
_lib = None


def load():
    """The probe library, loaded once. A missing or stale probe is an error (it is built where the tree is built, not
    on the GPU box), never a skip."""
    global _lib
    if _lib is not None:
        return _lib
    override = os.environ.get("LMC_PROBE_LIB")
    path = os.path.abspath(override or lib_path())
    if not os.path.exists(path):
        raise ProbeError("%s not found: the probe library is not built. Run `python -c \"import __graft_entry__ as g; "
                         "g.build()\"` (needs hipcc) before the GPU tests." % path)
    if not override and needs_build(path):
        raise ProbeError("%s is stale: it carries source hash %s, the tree's is %s. Rebuild it with "
                         "`python -c \"import __graft_entry__ as g; g.build()\"`." % (path, binary_hash(path), source_hash()))
    try:
        lib = C.CDLL(path)
    except OSError as err:
        raise ProbeError("cannot load %s: %s" % (path, err))
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ProbeError("%s does not export %s (stale build?)" % (path, name))
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _check(rc, what):
    if rc != 0:
        raise ProbeError("%s failed with code %d (-1: no such kernel in the probe, -2: bad argument, else hipError_t)" % (what, rc))


def exp_uniform(x, fast=False):
    """exp_uniform / exp_uniform_fast of every x (one wave each). The value is wave-uniform: lane 0's and lane 63's copies
    are asserted to be the same bits before lane 0's is returned."""
    x = _f64(np.ravel(x))
    out = np.empty(2 * x.size)
    _check(load().lmc_probe_exp(1 if fast else 0, _ptr(x), _ptr(out), x.size), "lmc_probe_exp")
    first, last = out[:x.size], out[x.size:]
    assert np.array_equal(first.view(np.uint64), last.view(np.uint64)), "lanes 0 and 63 disagree on a wave-uniform value"
    return first


def log_unit(x):
    x = _f64(np.ravel(x))
    out = np.empty(x.size)
    _check(load().lmc_probe_log_unit(_ptr(x), _ptr(out), x.size), "lmc_probe_log_unit")
    return out


def sum6(x):
    """wave_sum6_totals: x[blocks, 6, 64] -> [blocks, 6]."""
    x = _f64(x)
    assert x.ndim == 3 and x.shape[1:] == (6, 64), x.shape
    out = np.empty((x.shape[0], 6))
    _check(load().lmc_probe_sum6(_ptr(x), _ptr(out), x.shape[0]), "lmc_probe_sum6")
    return out


TEAM_ROWS = dict(sum=0, sum2=(1, 2), np2=(3, 4), np6=(5, 6, 7, 8, 9, 10), bcast0=11, lo_src=12, hi_src=13)
TEAM_N_IN = 14


def team(w, x):
    """Every Team<w> operation, ``rounds`` back to back in one kernel. x[blocks, rounds, 14, 64 w] (rows: TEAM_ROWS).
    Returns dict of per-wave copies sum / sum2a / sum2b / np2 / np6 [blocks, rounds, w] and per-thread bcast0 / below /
    above [blocks, rounds, 64 w]."""
    lib = load()
    rows = np.zeros(3, dtype=np.int32)
    lib.lmc_probe_team_rows(rows[0:].ctypes.data_as(_P), rows[1:].ctypes.data_as(_P), rows[2:].ctypes.data_as(_P))
    assert tuple(rows) == (TEAM_N_IN, 5, 3), tuple(rows)
    x = _f64(x)
    assert x.ndim == 4 and x.shape[2:] == (TEAM_N_IN, 64 * w), x.shape
    blocks, rounds = x.shape[:2]
    outu = np.empty((blocks, rounds, w, 5))
    outt = np.empty((blocks, rounds, 3, 64 * w))
    _check(lib.lmc_probe_team(w, blocks, rounds, _ptr(x), _ptr(outu), _ptr(outt)), "lmc_probe_team<%d>" % w)
    res = {name: outu[..., k] for k, name in enumerate(("sum", "sum2a", "sum2b", "np2", "np6"))}
    res.update({name: outt[:, :, k] for k, name in enumerate(("bcast0", "below", "above"))})
    return res


def logp_grad(family, ns, w, q, params=()):
    """logp_grad of the built-in functor ``family`` as <NS = ns> on Team<w>: q[chains, d] -> (logp[chains, w]: one copy per
    wave, g[chains, 64 ns w]: padding slots included)."""
    lib = load()
    q = _f64(q)
    assert q.ndim == 2
    chains, d = q.shape
    params = _f64(np.ravel(params))
    logp = np.empty((chains, w))
    g = np.empty((chains, 64 * ns * w))
    _check(lib.lmc_probe_logp(FAMILIES[family], ns, w, d, chains, _ptr(params) if params.size else None, params.size,
                              _ptr(q), _ptr(logp), _ptr(g)), "lmc_probe_logp %s <%d,%d> d=%d" % (family, ns, w, d))
    return logp, g


if __name__ == "__main__":
    print(build(force=True, verbose=True))
