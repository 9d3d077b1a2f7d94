"""Posterior predictions at new X (littlemcmc_amd/csrc/lmc_linpred.hip, littlemcmc_amd/predictive.py: linear_predictor,
predict) restated twice for the tests: one ``lmc_glm_linpred`` call in numpy float64, and the linear predictor and its moments
in mpmath at 50 digits on top of ``_predictive_model.reference_loglik`` (which yields ``mu`` and its per-draw bound); plus the
forward error bounds that the numpy model (test_linpred_cpu.py) and the device (test_gpu_linpred.py) are held to.

One call writes ``eta[chains][n][W]`` (W = 64 observations a block; a padding observation has X = 0, so eta = 0) and, per
group and observation over the n draws of the group present, the planes
  0  n_g      1  mean_s eta      2  M2 = sum_s (eta - mean)^2      3  mean_s mu      4  sum_s (mu - mean mu)^2
with mu = sigmoid(eta) | exp(eta) | eta in the expressions of _predictive_model.loglik_mu.

The bounds (u = 2^-53, first order in u; n = the number of draws a plane is taken over). Every implementation forms eta as a
recursive dot product with e ascending -- the device with one fma a term, numpy with a rounded product and a rounded sum --
and both are covered by the bound of _glm_model.reference:
  eta      |d eta_s| <= (d + 2) u S,  S = sum_e |X_e q_se|
  mu       |d mu_s| <= |mu'| |d eta_s| + 8 u |mu_s|,  mu' = sg (1 - sg) | mu | 1        (_predictive_model, unchanged)
The two means and the two M2 are those of _predictive_model's planes 3 and 4 with l replaced by v = eta or mu -- the same
operations on other numbers: per tile a sum and a division, deviations, squares and their sum, then Chan updates
mean_a + delta nb / n, M2_a + M2_b + delta^2 na nb / n, at most n of them in any order:
  mean v   |d mean| <= mean_s |d v_s| + eps,   eps = (5 n + 8) u max_s |v_s|: a sum of n terms in any order is (n - 1) u of
           the sum of magnitudes, and each of at most n Chan updates rounds four times at magnitude <= max |v|
  M2 v     exact perturbation d M2 = 2 sum (v_s - mean) d v_s + sum d v_s^2 (sum (v_s - mean) = 0 removes d mean); evaluation:
           deviations, squares, sums and Chan's cross terms (5 n + 16) u M2, and the means inside the cross terms are off by
           eps:  |d M2| <= 2 sum |v_s - mean| |d v_s| + sum d v_s^2 + (5 n + 16) u M2 + 2 sqrt(n M2) eps + n eps^2
No tolerance is fixed by hand: every number above comes from the inputs. A non-finite eta or mu leaves its planes non-finite
by definition (lmc_hip.h) and has no bound."""
import functools

import numpy as np

from . import _glm_model as G
from . import _predictive_model as P

U = G.U
PLANES = 5


def mu_of(eta, lik):
    """The mean response in the device's expressions (those of _predictive_model.loglik_mu)."""
    with np.errstate(over="ignore", invalid="ignore"):
        if lik == "bernoulli":
            ex = np.exp(-np.abs(eta))
            return np.where(eta >= 0.0, 1.0, ex) / (1.0 + ex)
        if lik == "poisson":
            return np.exp(eta)
        return eta.copy()


def planes_of(eta, mu):
    """The five planes [5, W] of eta[S, W], mu[S, W] (S >= 0 draws), straightforwardly (two passes over all the draws)."""
    S, W = eta.shape
    out = np.zeros((PLANES, W))
    if S == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        out[0] = S
        out[1] = eta.sum(axis=0) / S
        out[2] = ((eta - out[1]) ** 2).sum(axis=0)
        out[3] = mu.sum(axis=0) / S
        out[4] = ((mu - out[3]) ** 2).sum(axis=0)
    return out


def linpred(x, table, first_chain, per, ob0, ob1):
    """One call: x[chains, n, d] float64 whose chain 0 is chain ``first_chain`` of the job, ``table[n_rows, row_len]`` the GLM
    parameter rows, observation blocks [ob0, ob1) -> (eta[chains, n, W], stats[groups touched, 5, W]). eta with e ascending
    (multiply, then add); the y section of a row is not looked at."""
    c, n, d = x.shape
    g0, g1 = first_chain // per, (first_chain + c - 1) // per
    W = 64 * (ob1 - ob0)
    eta = np.zeros((c, n, W))
    stats = np.zeros((g1 - g0 + 1, PLANES, W))
    for g in range(g0, g1 + 1):
        row = np.asarray(table[g])
        lik, npad = P.CODES[int(row[0])], int(row[2])
        assert int(row[5]) == d and 0 <= ob0 < ob1 <= npad // 64
        d8 = (d + 7) // 8 * 8
        Xt = row[8 + npad:8 + npad + d8 * npad].reshape(d8, npad)[:, 64 * ob0:64 * ob1]
        lo, hi = max(g * per - first_chain, 0), min((g + 1) * per - first_chain, c)
        with np.errstate(over="ignore", invalid="ignore"):
            for e in range(d):
                eta[lo:hi] = eta[lo:hi] + x[lo:hi, :, e, None] * Xt[e][None, None, :]
        flat = eta[lo:hi].reshape(-1, W)
        stats[g - g0] = planes_of(flat, mu_of(flat, lik))
    return eta, stats


def linpred_fn(x, table, first_chain, per, ob0, ob1, want_eta=True, want_stats=True):
    """What littlemcmc_amd.predictive takes as ``linpred_fn``: the model in place of the HIP call (torch in, torch out)."""
    import torch

    xs = x.detach().cpu().numpy().astype(np.float64, copy=False)
    eta, stats = linpred(xs, np.asarray(table), int(first_chain), int(per), int(ob0), int(ob1))
    return (torch.from_numpy(eta).to(x.device) if want_eta else None,
            torch.from_numpy(stats).to(x.device) if want_stats else None)


# ---- the 50-digit reference ----------------------------------------------------------------------------------------------------
def reference(X, draws, lik, pl):
    """eta of every draw at 50 digits with its bound, next to the mu and dmu of ``pl`` = a _predictive_model.reference_loglik
    of the same X, draws and likelihood (whatever its y: mu and dmu do not depend on it where the draw is not DEAD; a DEAD
    draw carries dmu = inf and bounds nothing): dict(eta[S][N] (mpf), deta[S, N], mu (mpf), dmu[S, N])."""
    mp = G._mp().mp
    rows, _cols = G.mp_matrix(X)
    S, d = draws.shape
    eta = []
    for s in range(S):
        qm = [mp.mpf(float(v)) for v in draws[s]]
        eta.append([mp.fdot(r, qm) for r in rows])
    deta = (d + 2) * U * (np.abs(draws) @ np.abs(X).T)
    return dict(eta=eta, deta=deta, mu=pl["mu"], dmu=pl["dmu"])


def _moments(col, dv, n, mp):
    """(mean, M2, bound of the mean, bound of M2) of the n exact values ``col`` known to the implementation within ``dv``."""
    mean = mp.fsum(col) / n
    dev = [v - mean for v in col]
    M2 = mp.fsum(v * v for v in dev)
    eps = (5 * n + 8) * U * max(abs(float(v)) for v in col)
    adev = np.array([abs(float(v)) for v in dev])
    b_mean = dv.mean() + eps
    b_M2 = (2 * (adev * dv).sum() + (dv * dv).sum() + (5 * n + 16) * U * float(M2) + 2 * np.sqrt(n * float(M2)) * eps
            + n * eps * eps)
    return float(mean), float(M2), b_mean, b_M2


def reference_planes(ref, idx=None):
    """The planes [5, N] of the draws ``idx`` of a reference() (default: all), rounded to float64 at the end, and their
    bounds [5, N] (plane 0: 0)."""
    mp = G._mp().mp
    idx = list(range(len(ref["eta"]))) if idx is None else list(idx)
    n, N = len(idx), len(ref["eta"][0])
    val, bnd = np.zeros((PLANES, N)), np.zeros((PLANES, N))
    val[0] = n
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(N):
            val[1, j], val[2, j], bnd[1, j], bnd[2, j] = _moments([ref["eta"][s][j] for s in idx], ref["deta"][idx, j], n, mp)
            val[3, j], val[4, j], bnd[3, j], bnd[4, j] = _moments([ref["mu"][s][j] for s in idx], ref["dmu"][idx, j], n, mp)
    return val, bnd


def check_eta(got, ref, idx=None, what=""):
    """Assert got[len(idx), N] against the reference's eta of the draws idx, element by element."""
    idx = list(range(len(ref["eta"]))) if idx is None else list(idx)
    val = np.array([[float(v) for v in ref["eta"][s]] for s in idx])
    ok = P.within(got, val, ref["deta"][idx] + U * np.abs(val))   # (the reference's own rounding to float64)
    assert ok.all(), "%s eta: got %r, reference %r, bound %r" % (what, np.asarray(got)[~ok][:4], val[~ok][:4],
                                                                  ref["deta"][idx][~ok][:4])


def check_planes(got, ref, idx=None, what=""):
    """Assert a block got[5, N] against the reference of the draws idx: the count exactly, every other plane within its bound
    (plus the rounding of the reference value itself to float64)."""
    val, bnd = reference_planes(ref, idx)
    got = np.asarray(got, dtype=np.float64)
    assert np.array_equal(got[0], val[0]), "%s count: got %r, want %r" % (what, got[0][:4], val[0][:4])
    for p in range(1, PLANES):
        ok = P.within(got[p], val[p], bnd[p] + U * np.abs(val[p]))
        assert ok.all(), "%s plane %d: got %r, reference %r, bound %r" % (
            what, p, got[p][~ok][:4], val[p][~ok][:4], bnd[p][~ok][:4])


@functools.lru_cache(maxsize=None)
def case_reference(N, d, lik, count):
    """reference() of _predictive_model's shared inputs: X of _glm_model.case(N, d, lik), the draws of P.draws_of."""
    X, _y, _Q = G.case(N, d, lik)
    return reference(X, P.draws_of(N, d, lik, count), lik, P.case_reference(N, d, lik, count))


def inverse_link(eta, lik):
    """The host's inverse link of predict(): what torch.sigmoid / torch.exp / the identity compute, through torch itself (the
    definition of mu_quantiles is the host's function of the sorted eta, so the test uses that function)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(eta, dtype=np.float64))
    return {"bernoulli": torch.sigmoid, "poisson": torch.exp, "gaussian": lambda v: v}[lik](t).numpy()
