"""targets.GLM restated twice for the tests: in numpy float64, in the operation ORDER of the device functor
(littlemcmc_amd/csrc/lmc_targets.hpp: GLMTarget), and in mpmath at 50 digits; plus the forward error bound both are held to
and the inputs the CPU and the GPU test share.

The order, per chain (one wavefront, lane t owns coefficients t*NS .. t*NS+NS-1, NS = ceil(d/64) rounded up to a power of two):
  eta_n   = sum over e ASCENDING of X[n, e] * q[e]                     (device: one fma per term; numpy: multiply, then add)
  l_n, r_n  from eta_n in the stable forms of `link` below
  lane l    adds the l_n of its observations n = l, 64 + l, 128 + l, ... ascending
  g_e     = sum over n ASCENDING of X[n, e] * r_n, then g_e - tau * q_e
  prior   lane t: pp = sum over its slots ascending of q^2; lane partial = lane's l sum + (-tau/2) * pp
  logp    = the 64 lane partials summed in a balanced binary tree (both of the device's wave reductions are such trees)
numpy has no fused multiply-add: each product here is rounded before it is added, where the device rounds once. Both are
covered by the same bound (a recursive dot product of d terms has |error| <= (d + 2) u sum |x_i y_i| either way, to first
order), which is what test_glm_cpu.py checks for this file and test_gpu_glm.py for the device."""
import functools

import numpy as np

U = 2.0 ** -53
LIKELIHOODS = ("bernoulli", "poisson", "gaussian")


def ns_for(d):
    need, ns = (d + 63) // 64, 1
    while ns < need:
        ns *= 2
    return ns


def link(eta, y, lik, isig2):
    """(l, r) per observation, float64, the device's expressions."""
    if lik == "bernoulli":
        ex = np.exp(-np.abs(eta))
        den = 1.0 + ex
        lo = y * eta - (np.maximum(eta, 0.0) + np.log1p(ex))
        r = y - np.where(eta >= 0.0, 1.0 / den, ex / den)
    elif lik == "poisson":
        with np.errstate(over="ignore", invalid="ignore"):
            mu = np.exp(eta)
            lo = y * eta - mu
            r = y - mu
    else:
        res = y - eta
        lo = -0.5 * ((res * res) * isig2)
        r = res * isig2
    return lo, r


def logp_grad(X, y, q, lik, tau=1.0, isig2=1.0):
    """(logp, g[d]) of one point in float64, device order."""
    N, d = X.shape
    ns = ns_for(d)
    eta = np.zeros(N)
    for e in range(d):
        eta = eta + X[:, e] * q[e]
    lo, r = link(eta, y, lik, isig2)
    lanes = np.zeros(64)
    for n0 in range(0, N, 64):
        blk = lo[n0:n0 + 64]
        lanes[:blk.size] = lanes[:blk.size] + blk
    g = np.zeros(d)
    with np.errstate(invalid="ignore"):
        for n in range(N):
            g = g + X[n] * r[n]
    g = g + (-tau) * q
    qp = np.zeros(64 * ns)
    qp[:d] = q
    qp = qp.reshape(64, ns)
    pp = np.zeros(64)
    for s in range(ns):
        pp = pp + qp[:, s] * qp[:, s]
    part = lanes + (-0.5 * tau) * pp
    while part.size > 1:
        part = part[0::2] + part[1::2]
    return float(part[0]), g


@functools.lru_cache(maxsize=None)
def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def mp_matrix(X):
    """X as rows and columns of 50-digit numbers (exact: a double converts without rounding); made once per design matrix."""
    mp = _mp().mp
    rows = [[mp.mpf(float(v)) for v in row] for row in X]
    return rows, [list(col) for col in zip(*rows)]


def reference(X, y, q, lik, tau=1.0, isig2=1.0, Xm=None):
    """The same posterior at 50 digits, rounded to float64 at the end, and the error bound of the stated order:
    dict(logp, g[d], logp_bound, g_bound[d]). With u = 2^-53, S_n = sum_e |X_ne q_e|, l' = dl/deta = r, r' = dr/deta and
    w_n the magnitude of the operands r_n is formed from (|y_n| + the mean; times 1/sigma^2 for the gaussian):
      |d eta_n| <= (d + 2) u S_n
      |d l_n|   <= |r_n| |d eta_n| + 8 u |l_n|
      |d logp|  <= sum_n |d l_n| + (ceil(N/64) + 8) u sum_n |l_n| + (NS + 8) u tau/2 sum_e q_e^2
      |d r_n|   <= |r'_n| |d eta_n| + 8 u w_n
      |d g_e|   <= sum_n |X_ne| |d r_n| + (N + 2) u sum_n |X_ne r_n| + 3 u tau |q_e|"""
    mp = _mp().mp
    N, d = X.shape
    ns = ns_for(d)
    rows, cols = mp_matrix(X) if Xm is None else Xm
    qm = [mp.mpf(float(v)) for v in q]
    eta = [mp.fdot(rows[n], qm) for n in range(N)]
    lo, r, rp, w = [], [], [], []
    for n in range(N):
        e, yn = eta[n], mp.mpf(float(y[n]))
        if lik == "bernoulli":
            sp = (e if e > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(e)))
            sg = 1 / (1 + mp.exp(-e))
            lo.append(yn * e - sp)
            r.append(yn - sg)
            rp.append(sg * (1 - sg))
            w.append(abs(yn) + sg)
        elif lik == "poisson":
            mu = mp.exp(e)
            lo.append(yn * e - mu)
            r.append(yn - mu)
            rp.append(mu)
            w.append(abs(yn) + mu)
        else:
            lo.append(-(yn - e) ** 2 * isig2 / 2)
            r.append((yn - e) * isig2)
            rp.append(mp.mpf(isig2))
            w.append((abs(yn) + abs(e)) * isig2)
    qq = mp.fdot(qm, qm)
    logp = mp.fsum(lo) - mp.mpf(tau) / 2 * qq
    g = [mp.fdot(cols[e], r) - mp.mpf(tau) * qm[e] for e in range(d)]
    # the bound's ingredients are magnitudes: float64 is enough for them
    f = lambda v: np.array([float(x) for x in v])   # noqa: E731
    lo_f, r_f, rp_f, w_f = f(lo), f(r), f(rp), f(w)
    S = np.abs(X) @ np.abs(q)
    deta = (d + 2) * U * S
    dl = np.abs(r_f) * deta + 8 * U * np.abs(lo_f)
    logp_bound = dl.sum() + ((N + 63) // 64 + 8) * U * np.abs(lo_f).sum() + (ns + 8) * U * 0.5 * tau * float(q @ q)
    dr = rp_f * deta + 8 * U * w_f
    g_bound = np.abs(X).T @ dr + (N + 2) * U * (np.abs(X).T @ np.abs(r_f)) + 3 * U * tau * np.abs(q)
    return dict(logp=float(logp), g=f(g), logp_bound=float(logp_bound), g_bound=g_bound)


# ---- the inputs test_glm_cpu.py and test_gpu_glm.py share ---------------------------------------------------------------------
# (1, 1) a single lane of data; (63, 3), (65, 65), (130, 130) partial last observation blocks; NS = 1, 2, 4 in the fused
# kernels, (70, 300) NS = 8 in the general one-wave kernel
SHAPES = ((1, 1), (63, 3), (64, 64), (65, 65), (130, 130), (70, 256), (70, 300))
N_POINTS = 4


@functools.lru_cache(maxsize=None)
def case(N, d, lik):
    """(X[N, d], y[N], Q[4, d]) of one cell of the grid, deterministic. Q[0] is all zeros, Q[1] a moderate point; for the
    bernoulli likelihood Q[2] and Q[3] are scaled so that the largest |eta| is 40 and 800 (opposite signs, so that both ends
    are reached between them); for the others they are two more moderate points (an exp(eta) that stays finite)."""
    rng = np.random.default_rng(1000 * N + d + 7 * LIKELIHOODS.index(lik))
    X = rng.standard_normal((N, d)) / np.sqrt(d)
    if d > 1:
        X[:, 0] = 1.0   # an intercept
    Q = rng.standard_normal((N_POINTS, d))
    Q[0] = 0.0
    if lik == "bernoulli":
        y = (rng.random(N) < 0.5).astype(np.float64)
        for c, (top, sign) in ((2, (40.0, 1.0)), (3, (800.0, -1.0))):
            eta = X @ Q[c]
            Q[c] *= sign * top / eta[np.argmax(np.abs(eta))]
    elif lik == "poisson":
        y = rng.poisson(2.0, N).astype(np.float64)
    else:
        y = rng.standard_normal(N)
    for a in (X, y, Q):
        a.setflags(write=False)
    return X, y, Q


# scales of the grid's posteriors: not 1, so that tau and 1/sigma^2 are seen to be applied
PRIOR_SCALE, SIGMA = 2.0, 0.5


@functools.lru_cache(maxsize=None)
def case_reference(N, d, lik):
    """reference() at the N_POINTS points of case(N, d, lik), computed once per process."""
    X, y, Q = case(N, d, lik)
    tau, isig2 = PRIOR_SCALE ** -2, SIGMA ** -2
    Xm = mp_matrix(X)
    return tuple(reference(X, y, Q[c], lik, tau, isig2, Xm) for c in range(N_POINTS))
