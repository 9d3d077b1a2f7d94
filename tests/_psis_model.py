"""The PSIS row algorithm of include/lmc_hip.h (lmc_psis_rows; littlemcmc_amd/csrc/lmc_psis.hip) restated for the tests: in
plain numpy float64 (``psis_row``), the same at 50 digits with mpmath (``psis_row_mp``), the exact leave-one-out predictive
density of the gaussian GLM (``exact_loo``), the rows the CPU and GPU tests share, and the functions predictive.loo() takes
as ``psis_fn`` / ``loglik_fn``.

One row l[S], M = tail_len(S, reff):
  1. lw = min l - l (= -l - max(-l), the same bits); any non-finite l: NaN outputs, n_tail 0.
  2. cutoff = max((M + 1)-th largest lw, log(DBL_MIN)); tail = {lw > cutoff}.
  3. n_tail <= 4: k = inf, sigma = NaN. Else the tail sorted by ascending lw (equal lw: descending l),
     x = exp(lw) - exp(cutoff), and the Zhang-Stephens fit with prior_bs = 3, prior_k = 10.
  4. k finite: lw_(i) <- log(exp(cutoff) + sigma expm1(-k log1p(-p_i)) / k), p_i = (i - 0.5) / n_tail; then min(lw, 0).
  5. elpd = min l + log A - log B, A = (S - n_tail) + sum_tail exp(lw' - lw), B = sum w, ess_w = B^2 / sum w^2.

SD_TOTAL, SD_POINT, Z_WORST are MEASURED by tests/test_psis_cpu.py::test_model_against_the_exact_closed_form (20 seeds of
S = 3200 iid posterior draws on the four rungs of _predictive_model.ladder()): the largest seed-to-seed standard deviation
of sum_n (elpd_loo_n - exact_n) over the rungs, of one elpd_loo_n, and the largest |mean deviation| / sd. The test asserts
that what it measures does not exceed them; the GPU end-to-end test reads SD_TOTAL from here."""
import functools
import math

import numpy as np

from . import _glm_model as G
from . import _predictive_model as P

LOG_TINY = -708.3964185322641    # log(DBL_MIN) rounded to nearest: the constant of the kernel
MAX_TAIL = 4096
SD_TOTAL = 0.089                 # sd over seeds of the summed deviation at S = 3200 iid draws, the largest of the four rungs
SD_POINT = 0.040
SD_DRAWS = 3200


def tail_len(S, reff=1.0):
    return min(int(S) // 5, int(math.ceil(3.0 * math.sqrt(int(S) / float(reff)))))


def psis_row(l, reff=1.0, M=None, full=False):
    """(elpd, k, n_tail, ess_w, sigma) of one row in float64; ``full=True`` adds (cutoff, min l)."""
    l = np.asarray(l, dtype=np.float64)
    S = l.shape[0]
    M = tail_len(S, reff) if M is None else int(M)
    M = min(M, S - 1)
    nan = float("nan")
    if not np.isfinite(l).all():
        lmin = nan if np.isnan(l).any() else float(l.min())
        return (nan, nan, 0, nan, nan) + ((nan, lmin) if full else ())
    lmin = l.min()
    lw = lmin - l
    with np.errstate(all="ignore"):
        cutoff = max(float(np.partition(lw, S - 1 - M)[S - 1 - M]), LOG_TINY)   # the (M + 1)-th largest
        expc = np.exp(cutoff)
        in_tail = lw > cutoff
        lt = np.sort(l[in_tail])[::-1]            # descending l: ascending lw, equal lw by descending l
        n = int(lt.shape[0])
        lw_t = lmin - lt
        k, sigma = float("inf"), nan
        new = lw_t.copy()
        if n > 4:
            x = np.exp(lw_t) - expc
            m = 30 + int(math.floor(math.sqrt(n)))
            j = np.arange(1, m + 1, dtype=np.float64)
            b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x[int(math.floor(n / 4.0 + 0.5)) - 1]) + 1.0 / x[n - 1]
            kj = np.log1p(-b[:, None] * x[None, :]).sum(axis=1) / n
            L = n * (np.log(-b / kj) - kj - 1.0)
            w = 1.0 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
            bb = (b * w).sum()
            k = np.log1p(-bb * x).sum() / n
            sigma = float(-k / bb)
            k = float((n * k + 5.0) / (n + 10.0))
            if np.isfinite(k):
                p = (np.arange(1, n + 1, dtype=np.float64) - 0.5) / n
                new = np.log(expc + sigma * np.expm1(-k * np.log1p(-p)) / k)
        new = np.where(new > 0.0, 0.0, new)
        w_rest = np.exp(lw[~in_tail])
        w_tail = np.exp(new)
        A = float(S - n) + np.exp(new - lw_t).sum()
        B = w_rest.sum() + w_tail.sum()
        B2 = (w_rest * w_rest).sum() + (w_tail * w_tail).sum()
        elpd = float(lmin + (np.log(A) - np.log(B)))
        out = (elpd, k, n, float(B * B / B2), sigma)
    return out + ((cutoff, float(lmin)) if full else ())


def psis_row_mp(l, reff=1.0, M=None, bulk_longdouble=50000):
    """The same at 50 digits (every discrete step on the exact values): (elpd, k, n_tail, ess_w, sigma) as floats. A row
    longer than ``bulk_longdouble`` sums its weights OUTSIDE the tail in numpy's extended precision (64-bit mantissa, pairwise:
    three orders of magnitude below a float64 rounding) instead of 50-digit exponentials one by one."""
    mp = G._mp().mp
    l = np.asarray(l, dtype=np.float64)
    S = l.shape[0]
    M = tail_len(S, reff) if M is None else int(M)
    M = min(M, S - 1)
    lmin = l.min()
    order = np.argsort(-l, kind="stable")        # ascending lw (exact: lw is monotone in l)
    lw_cut = mp.mpf(float(lmin)) - mp.mpf(float(l[order[S - 1 - M]]))
    cutoff = max(lw_cut, mp.log(mp.mpf(np.finfo(np.float64).tiny)))
    expc = mp.exp(cutoff)
    lw_sorted = [mp.mpf(float(lmin)) - mp.mpf(float(v)) for v in l[order[S - 1 - M:]]]
    tail = [v for v in lw_sorted if v > cutoff]
    n = len(tail)
    n_rest = S - n
    k, sigma = mp.inf, mp.nan
    new = list(tail)
    if n > 4:
        x = [mp.exp(v) - expc for v in tail]
        m = 30 + int(math.floor(math.sqrt(n)))
        b = [(1 - mp.sqrt(mp.mpf(m) / (j - mp.mpf(1) / 2))) / (3 * x[int(math.floor(n / 4.0 + 0.5)) - 1]) + 1 / x[n - 1]
             for j in range(1, m + 1)]
        kj = [mp.fsum(mp.log1p(-bj * xi) for xi in x) / n for bj in b]
        L = [n * (mp.log(-bj / kv) - kv - 1) for bj, kv in zip(b, kj)]
        w = [1 / mp.fsum(mp.exp(Ll - Lj) for Ll in L) for Lj in L]
        bb = mp.fsum(bj * wj for bj, wj in zip(b, w))
        k = mp.fsum(mp.log1p(-bb * xi) for xi in x) / n
        sigma = -k / bb
        k = (n * k + 5) / (n + 10)
        new = [mp.log(expc + sigma * mp.expm1(-k * mp.log1p(-(mp.mpf(i) - mp.mpf(1) / 2) / n)) / k) for i in range(1, n + 1)]
    new = [min(v, mp.mpf(0)) for v in new]
    rest = l[order[:S - n]]
    if S > bulk_longdouble and np.finfo(np.longdouble).eps < 2e-19:
        e = np.exp(np.longdouble(lmin) - rest.astype(np.longdouble))
        s1, s2 = e.sum(), (e * e).sum()
        hi1, hi2 = np.float64(s1), np.float64(s2)
        b_rest = mp.mpf(float(hi1)) + mp.mpf(float(s1 - hi1))
        b2_rest = mp.mpf(float(hi2)) + mp.mpf(float(s2 - hi2))
    else:
        e = [mp.exp(mp.mpf(float(lmin)) - mp.mpf(float(v))) for v in rest]
        b_rest, b2_rest = mp.fsum(e), mp.fsum(v * v for v in e)
    w_tail = [mp.exp(v) for v in new]
    A = n_rest + mp.fsum(mp.exp(a - b0) for a, b0 in zip(new, tail))
    B = b_rest + mp.fsum(w_tail)
    B2 = b2_rest + mp.fsum(v * v for v in w_tail)
    elpd = mp.mpf(float(lmin)) + mp.log(A) - mp.log(B)
    return float(elpd), float(k), n, float(B * B / B2), float(sigma)


def psis_fn(l2, M):
    """What predictive.psis / loo take as ``psis_fn``: [rows, 8] of the float64 model (the columns of lmc_psis_rows)."""
    import torch

    a = l2.detach().cpu().numpy()
    out = np.zeros((a.shape[0], 8))
    for r in range(a.shape[0]):
        elpd, k, n, ess, sigma, cutoff, lmin = psis_row(a[r], M=M, full=True)
        out[r] = [elpd, k, n, sigma, ess, cutoff, lmin, 0.0]
    return torch.as_tensor(out).to(l2.device)


def loglik_fn(x, table, first_chain, per, ob0, ob1):
    """What predictive.loo takes as ``loglik_fn``: [groups, 64 (ob1 - ob0), per * draws] from _predictive_model.loglik_mu, rows
    decoded from the host table; padding observations hold 0."""
    import torch

    xs = x.detach().cpu().numpy()
    c, n, d = xs.shape
    assert first_chain % per == 0 and c % per == 0
    out = np.zeros((c // per, 64 * (ob1 - ob0), per * n))
    for gi in range(c // per):
        X, y, lik, isig2 = P.decode_row(np.asarray(table[first_chain // per + gi]))
        lo, _mu = P.loglik_mu(X, y, xs[gi * per:(gi + 1) * per].reshape(-1, d), lik, isig2)   # [S, N]
        a, b = 64 * ob0, min(64 * ob1, X.shape[0])
        out[gi, :b - a] = lo[:, a:b].T
    return torch.as_tensor(out).to(x.device)


def exact_loo(tgt):
    """log p(y_n | y_-n)[N] of a gaussian targets.GLM in closed form: with the posterior precision P = X'X / sigma^2 + tau I
    and right-hand side r = X'y / sigma^2, leaving n out removes x_n x_n' / sigma^2 from P and x_n y_n / sigma^2 from r;
    then m_-n = P_-n^-1 r_-n, C_-n = P_-n^-1 and the density of y_n is N(x_n' m_-n, sigma^2 + x_n' C_-n x_n)."""
    X, y, s2 = tgt.X, tgt.y, tgt.sigma ** 2
    prec = X.T @ X / s2 + tgt.tau * np.eye(tgt.d)
    rhs = X.T @ y / s2
    out = np.empty(X.shape[0])
    for n in range(X.shape[0]):
        Pn = prec - np.outer(X[n], X[n]) / s2
        C = np.linalg.inv(Pn)
        mean = X[n] @ np.linalg.solve(Pn, rhs - X[n] * y[n] / s2)
        var = s2 + X[n] @ C @ X[n]
        out[n] = -0.5 * np.log(2 * np.pi * var) - 0.5 * (y[n] - mean) ** 2 / var
    return out


# ---- the rows test_psis_cpu.py and test_gpu_psis.py share -----------------------------------------------------------------
ROW_SIZES = (1, 5, 10, 25, 63, 64, 65, 200, 250, 257, 1000, 3200, 20000)
BIG_S = 1860000   # M = 4092, just under MAX_TAIL
KINDS = ("gaussian", "heavy", "lattice")


@functools.lru_cache(maxsize=None)
def row(kind, S):
    """One row of S log-likelihood values: gaussian (-z^2 / 2 - 1), heavy-tailed (-exp(z)) or lattice-valued (-|round(2 z)| / 2:
    many ties, also at the cutoff)."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + S % 9973 + 17)
    z = rng.standard_normal(S)
    out = {"gaussian": -0.5 * z * z - 1.0, "heavy": -np.exp(z), "lattice": -np.abs(np.round(2.0 * z)) / 2.0}[kind]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_rows():
    """The edge rows (name, l[100 or more]) of one common length 4000: tied (duplicated draws: ties at the cutoff), constant,
    clamped cutoff (-exp(3 z): the cutoff is log(DBL_MIN) and n_tail collapses), one -inf, one NaN, and plain neighbours."""
    rng = np.random.default_rng(99)
    S = 4000
    z = rng.standard_normal(S)
    plain = -0.5 * z * z
    tied = np.repeat(-0.5 * rng.standard_normal(S // 50) ** 2, 50)
    minus_inf, a_nan = plain.copy(), plain.copy()
    minus_inf[1234], a_nan[77] = -np.inf, np.nan
    rows = [("plain0", plain), ("tied", tied), ("constant", np.full(S, -1.3)), ("clamped", -np.exp(3.0 * z)),
            ("plain1", plain[::-1].copy()), ("minus_inf", minus_inf), ("plain2", -np.exp(z)), ("nan", a_nan),
            ("plain3", plain * 2.0)]
    for _name, r in rows:
        r.setflags(write=False)
    return tuple(rows)


def model_rows(mat, M):
    """[rows, 7]: (elpd, k, n_tail, ess_w, sigma, cutoff, min l) of every row of mat at tail length M."""
    return np.array([psis_row(r, M=M, full=True) for r in mat])


# The rounding sensitivity of the row algorithm: the largest relative deviation of elpd, k, sigma, ess_w between psis_row and
# psis_row_mp over the rows above. MEASURED by test_psis_cpu.py::
# test_float64_model_against_the_50_digit_model, which prints it and asserts that it does not exceed this value; the GPU test
# holds the device to 16 x EPS_ROW.
EPS_ROW = 4.2e-13


def rel_dev(got, want):
    """max relative deviation of the floats of two (elpd, k, n_tail, ess_w, sigma) tuples; non-finite entries must agree."""
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        if i == 2:
            continue
        if not (np.isfinite(g) and np.isfinite(w)):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (i, g, w)
            continue
        scale = abs(w)
        worst = max(worst, abs(g - w) / scale if scale > 0 else abs(g - w))
    return worst
