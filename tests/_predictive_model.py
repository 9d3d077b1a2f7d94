"""The pointwise predictive planes (littlemcmc_amd/csrc/lmc_predict.hip, littlemcmc_amd/predictive.py) restated twice for the
tests: in numpy float64 on tests/_glm_model.py's ``link``, and in mpmath at 50 digits; plus the forward error bound that the
numpy model (test_predictive_cpu.py), any merge of split blocks, and the device (test_gpu_predictive.py) are held to.

Per group and observation n, over the draws s of the group (l = the functor's l_n, constants dropped):
  plane 0  n_g                  1  m = max_s l            2  S = sum_s exp(l - m)
        3  mean_s l             4  M2 = sum_s (l - mean)^2    5  sum_s mu      (mu = sigmoid(eta) | exp(eta) | eta)
A draw with l = -inf contributes exp(l - m) := 0; a NaN l makes planes 1..5 NaN.

The bound (u = 2^-53, n = number of draws, first order in u; every implementation forms eta_n as a recursive dot product
with e ascending, then the link of _glm_model). From _glm_model.reference, per draw s and observation:
  |d eta| <= (d + 2) u S_n,  S_n = sum_e |X_ne q_e|         |d l_s| <= |r| |d eta| + 8 u |l_s| + 4 u (|a| + |b|)
  |d mu_s| <= |mu'| |d eta| + 8 u |mu_s|                     (mu' = sg (1 - sg) | mu | 1)
The last term is needed for ONE l where _glm_model's sum over N observations could do without it: the stable forms end in a
difference l = a - b, a = y eta, b = softplus(eta) (bernoulli) or exp(eta) (poisson), and a and b are each rounded at their
own magnitude (b a few ulps: its exp / log1p), which |l| does not measure when they cancel -- y = 1, eta = 29 gives
l = -2.5e-13 from two operands of 29. (Gaussian: a product, no difference; a = b = 0.)
A draw whose exact l is below -1e290 is DEAD: its weight exp(l - m) is zero in any arithmetic whatever its error (this is the
overflowed poisson exp(eta), l = -inf in float64); the maxima and sums below run over the other draws. For m, lse and S a
draw more than 2000 below the maximum, with |d l_s| below half that distance, is LIGHT: its exp(l - m) is an exact zero in
float64 here and there (exp underflows below -745), so its error -- which may be huge in absolute terms: l = -1e217 is
known to 1e203 -- does not enter; max_s |d l_s| runs over the other (heavy) draws.
  m        max is 1-Lipschitz in the sup norm:                |d m| <= max_s |d l_s|
  lse = m + log S, as a function of the computed l, is 1-Lipschitz in the sup norm too, which gives max_s |d l_s|. Its own
           evaluation: l - m is rounded (u |l - m|, and t |log t| <= 1/e for a term t = exp(l - m), with S >= 1), exp to 4 u,
           the sum of n terms and at most n merges -- each a rescaling by a rounded exponential and an addition, 6 u -- so S
           carries (n/e + 4 + n + 6 n) u <= (8 n + 8) u relative, log S that much absolutely plus its rounding, and the two
           final additions round once each:
           |d lse| <= max_s |d l_s| + (8 n + 8) u + 2 u (|m| + |log S| + |lse|)
           (lppd = lse - log n + const: the host's last two roundings are of the same form and are added by the tests)
  S = exp(lse - m):                                          |d S| <= S expm1(|d lse| + |d m|)
  mean     |d mean| <= mean_s |d l_s| + eps,   eps = (5 n + 8) u max_s |l_s|: a sum of n terms in any order is (n - 1) u of
           the sum of magnitudes; each of at most n Chan updates mean_a + delta nb / n rounds four times at magnitude
           <= max |l|
  M2       exact perturbation: d M2 = 2 sum (l_s - mean) d l_s + O(d l^2)  (sum (l_s - mean) = 0 removes d mean); evaluation:
           deviations, squares, sums and Chan's cross terms (5 n + 16) u M2, and the means inside the cross terms are off by
           eps:  |d M2| <= 2 sum |l_s - mean| |d l_s| + sum d l_s^2 + (5 n + 16) u M2 + 2 sqrt(n M2) eps + n eps^2
  sum mu   |d| <= sum_s |d mu_s| + (n + 2) u sum_s |mu_s|
With a dead draw planes 3 .. 5 are non-finite by definition (lmc_hip.h) and have no bound."""
import functools

import numpy as np

from . import _glm_model as G

U = G.U
PLANES = 6
DEAD = -1e290
CODES = {0: "bernoulli", 1: "poisson", 2: "gaussian"}


def loglik_mu(X, y, draws, lik, isig2):
    """(l[S, N], mu[S, N]) in float64: eta with e ascending (multiply, then add), the link of _glm_model."""
    S, d = draws.shape
    N = X.shape[0]
    lo, mu = np.empty((S, N)), np.empty((S, N))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            eta = np.zeros(N)
            for e in range(d):
                eta = eta + X[:, e] * draws[s, e]
            lo[s] = G.link(eta, y, lik, isig2)[0]
            if lik == "bernoulli":
                ex = np.exp(-np.abs(eta))
                mu[s] = np.where(eta >= 0.0, 1.0, ex) / (1.0 + ex)
            elif lik == "poisson":
                mu[s] = np.exp(eta)
            else:
                mu[s] = eta
    return lo, mu


def planes_of(lo, mu):
    """The six planes [6, N] of l[S, N], mu[S, N] (S >= 0 draws), straightforwardly."""
    S, N = lo.shape
    out = np.zeros((PLANES, N))
    out[1] = -np.inf
    if S == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        out[0] = S
        m = np.fmax.reduce(lo, axis=0)            # fmax: a NaN does not hide the others (it is flagged below)
        m = np.where(np.isnan(m), -np.inf, m)
        term = np.where(np.isneginf(lo), 0.0, np.exp(lo - np.where(np.isneginf(m), 0.0, m)))
        out[1], out[2] = m, term.sum(axis=0)
        out[3] = lo.sum(axis=0) / S
        out[4] = ((lo - out[3]) ** 2).sum(axis=0)
        out[5] = mu.sum(axis=0)
        out[1:, np.isnan(lo).any(axis=0)] = np.nan
    return out


def planes(X, y, draws, lik, isig2=1.0):
    return planes_of(*loglik_mu(X, y, draws, lik, isig2))


def merge(a, b):
    """The merge rule on numpy blocks [6, N] through littlemcmc_amd.predictive.merge (the one statement of it on the host)."""
    import torch

    from littlemcmc_amd import predictive

    return predictive.merge(torch.as_tensor(a), torch.as_tensor(b)).numpy()


def decode_row(row):
    """(X[N, d], y[N], likelihood name, isig2) from a GLM parameter row (include/lmc_hip.h: LMC_TARGET_GLM)."""
    lik, N, npad, isig2, d = CODES[int(row[0])], int(row[1]), int(row[2]), float(row[4]), int(row[5])
    d8 = (d + 7) // 8 * 8
    y = row[8:8 + N]
    Xt = row[8 + npad:8 + npad + d8 * npad].reshape(d8, npad)
    return np.ascontiguousarray(Xt[:d, :N].T), np.array(y), lik, isig2


def stats_fn(x, table, first_chain, per):
    """What littlemcmc_amd.predictive takes as ``stats_fn``: the kernel's block [groups touched, 6, N] of the chains x (a
    torch tensor [chains, draws, d]) from the numpy model, rows decoded from the host ``table``."""
    import torch

    xs = x.detach().cpu().numpy()
    c, n, d = xs.shape
    g0, g1 = first_chain // per, (first_chain + c - 1) // per
    out = []
    for g in range(g0, g1 + 1):
        lo_c, hi_c = max(g * per - first_chain, 0), min((g + 1) * per - first_chain, c)
        X, y, lik, isig2 = decode_row(np.asarray(table[g]))
        out.append(planes(X, y, xs[lo_c:hi_c].reshape(-1, d), lik, isig2))
    return torch.as_tensor(np.stack(out)).to(x.device)


def reference_loglik(X, y, draws, lik, isig2=1.0):
    """l and mu of every draw at 50 digits and the per-draw error bounds of the docstring:
    dict(l[S][N] (mpf), mu (mpf), dl[S, N], dmu[S, N]) -- made once per set of draws, shared by every subset of them."""
    mp = G._mp().mp
    S, d = draws.shape
    N = X.shape[0]
    rows, _cols = G.mp_matrix(X)
    ym = [mp.mpf(float(v)) for v in y]
    absX = np.abs(X)
    L, M, dl, dmu = [], [], np.zeros((S, N)), np.zeros((S, N))
    for s in range(S):
        qm = [mp.mpf(float(v)) for v in draws[s]]
        deta = (d + 2) * U * (absX @ np.abs(draws[s]))
        ls, ms = [], []
        for n in range(N):
            e = mp.fdot(rows[n], qm)
            if lik == "bernoulli":
                sg = 1 / (1 + mp.exp(-e))
                lv = ym[n] * e - ((e if e > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(e))))
                r, mv, mup = ym[n] - sg, sg, sg * (1 - sg)
                ops = abs(ym[n] * e) + abs(ym[n] * e - lv)
            elif lik == "poisson":
                mv = mp.exp(e)
                lv, r, mup = ym[n] * e - mv, ym[n] - mv, mv
                ops = abs(ym[n] * e) + mv
            else:
                lv, r, mv, mup = -(ym[n] - e) ** 2 * isig2 / 2, (ym[n] - e) * isig2, e, mp.mpf(1)
                ops = mp.mpf(0)
            ls.append(lv)
            ms.append(mv)
            if lv > DEAD:
                dl[s, n] = abs(float(r)) * deta[n] + 8 * U * abs(float(lv)) + 4 * U * float(ops)
                dmu[s, n] = abs(float(mup)) * deta[n] + 8 * U * abs(float(mv))
            else:
                dl[s, n] = dmu[s, n] = np.inf
        L.append(ls)
        M.append(ms)
    return dict(l=L, mu=M, dl=dl, dmu=dmu)


def reference_planes(ref, idx=None):
    """The planes [6, N] of the draws ``idx`` of a reference_loglik() (default: all), rounded to float64 at the end, their
    bounds [6, N] (plane 0: 0), and lse[N] = m + log S with lse_bound[N]."""
    mp = G._mp().mp
    idx = list(range(len(ref["l"]))) if idx is None else list(idx)
    n = len(idx)
    N = len(ref["l"][0])
    val, bnd, lse, lse_b = np.zeros((PLANES, N)), np.zeros((PLANES, N)), np.zeros(N), np.zeros(N)
    val[0] = n
    eps_c, inf = (5 * n + 8) * U, float("inf")
    with np.errstate(over="ignore", invalid="ignore"):
        return _reference_planes(ref, idx, n, N, val, bnd, lse, lse_b, eps_c, inf, mp)


def _reference_planes(ref, idx, n, N, val, bnd, lse, lse_b, eps_c, inf, mp):
    for j in range(N):
        col = [ref["l"][s][j] for s in idx]
        alive = [i for i, v in enumerate(col) if v > DEAD]
        dl = np.array([ref["dl"][idx[i], j] for i in alive])
        if not alive:
            val[1:, j], bnd[1:, j], lse[j], lse_b[j] = [-inf, 0.0, -inf, np.nan, inf], [0, 0, inf, inf, inf], -inf, 0.0
            continue
        m = max(col[i] for i in alive)
        # LIGHT draws: 2000 below the maximum with an error of less than half that distance -- exp(l - m) underflows to an
        # exact zero in float64 (below exp(-745)) in the reference and in any implementation alike
        heavy = [k for k, i in enumerate(alive) if not (m - col[i] > 2000 and dl[k] < float(m - col[i]) / 2)]
        S = mp.fsum(mp.exp(col[i] - m) for i in alive)
        lse_m = m + mp.log(S)
        val[1, j], val[2, j], lse[j] = float(m), float(S), float(lse_m)
        bnd[1, j] = dl[heavy].max()
        lse_b[j] = dl[heavy].max() + (8 * n + 8) * U + 2 * U * (abs(float(m)) + abs(float(mp.log(S))) + abs(float(lse_m)))
        bnd[2, j] = float(S) * np.expm1(lse_b[j] + bnd[1, j])
        if len(alive) < n:
            val[3:, j], bnd[3:, j] = [-inf, np.nan, inf], inf
            continue
        mean = mp.fsum(col) / n
        dev = [v - mean for v in col]
        M2 = mp.fsum(v * v for v in dev)
        mus = [ref["mu"][s][j] for s in idx]
        val[3, j], val[4, j], val[5, j] = float(mean), float(M2), float(mp.fsum(mus))
        eps = eps_c * max(abs(float(v)) for v in col)
        adev = np.array([abs(float(v)) for v in dev])
        bnd[3, j] = dl.mean() + eps
        bnd[4, j] = (2 * (adev * dl).sum() + (dl * dl).sum() + (5 * n + 16) * U * float(M2)
                     + 2 * np.sqrt(n * float(M2)) * eps + n * eps * eps)
        dmu = np.array([ref["dmu"][s, j] for s in idx])
        bnd[5, j] = dmu.sum() + (n + 2) * U * sum(abs(float(v)) for v in mus)
    return val, bnd, lse, lse_b


def within(got, val, bnd):
    """got within bnd of val, element by element; where val is not finite (a plane the header leaves non-finite, or one
    that is -inf / +inf by definition) got must be non-finite too, and equal where val is an infinity with bound 0."""
    got, val, bnd = np.broadcast_arrays(np.asarray(got, dtype=np.float64), val, bnd)
    fin = np.isfinite(val)
    ok = np.zeros(val.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        ok[fin] = np.abs(got[fin] - val[fin]) <= bnd[fin]
    ok[~fin] = ~np.isfinite(got[~fin])
    exact = ~fin & (bnd == 0) & ~np.isnan(val)
    ok[exact] = got[exact] == val[exact]
    return ok


def check_planes(got, ref, idx=None, what=""):
    """Assert a block got[6, N] against the reference of the draws idx: every plane within its bound, and lse = m + log S
    within its own (tighter than the product of the two planes' bounds)."""
    val, bnd, lse, lse_b = reference_planes(ref, idx)
    got = np.asarray(got, dtype=np.float64)
    for p in range(PLANES):
        ok = within(got[p], val[p], bnd[p])
        assert ok.all(), "%s plane %d: got %r, reference %r, bound %r" % (
            what, p, got[p][~ok][:4], val[p][~ok][:4], bnd[p][~ok][:4])
    with np.errstate(divide="ignore", invalid="ignore"):
        got_lse = got[1] + np.log(got[2])
    got_lse = np.where(np.isneginf(got[1]), -np.inf, got_lse)
    ok = within(got_lse, lse, lse_b + 2 * U * np.abs(np.where(np.isfinite(lse), lse, 0.0)))
    assert ok.all(), "%s lse: got %r, reference %r, bound %r" % (what, got_lse[~ok][:4], lse[~ok][:4], lse_b[~ok][:4])


# ---- the inputs test_predictive_cpu.py and test_gpu_predictive.py share -------------------------------------------------------
T = 8   # draws per loaded X element in pointwise_kernel (csrc/lmc_predict.hip: kPredT)
CHAINS, MAX_DRAWS = 3, 17


@functools.lru_cache(maxsize=None)
def draws_of(N, d, lik, count):
    """count draws around the four points of _glm_model.case(N, d, lik): Q[s % 4] plus a perturbation of 1e-3."""
    _X, _y, Q = G.case(N, d, lik)
    rng = np.random.default_rng(77 + 1000 * N + d + 7 * G.LIKELIHOODS.index(lik))
    out = Q[np.arange(count) % G.N_POINTS] + 1e-3 * rng.standard_normal((count, d))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(N, d, lik, count):
    X, y, _Q = G.case(N, d, lik)
    return reference_loglik(X, y, draws_of(N, d, lik, count), lik, G.SIGMA ** -2)


# ---- the gaussian closed form and the prior-scale ladder of the end-to-end test ---------------------------------------------
def gaussian_closed_form(tgt, X=None, y=None):
    """(lppd[N], p_waic[N]) of a gaussian targets.GLM under its EXACT posterior N(m, Sigma), at its own data or at (X, y):
    with v_n = x_n' Sigma x_n and delta_n = y_n - x_n' m, the predictive density of y_n is N(x_n' m, sigma^2 + v_n), and the
    posterior variance of l_n = -(y_n - x_n' q)^2 / (2 sigma^2) is (2 v_n^2 + 4 v_n delta_n^2) / (4 sigma^4)."""
    X = tgt.X if X is None else np.asarray(X, dtype=np.float64)
    y = tgt.y if y is None else np.asarray(y, dtype=np.float64)
    mean, cov = tgt.posterior_gaussian()
    v = np.einsum("ne,ef,nf->n", X, cov, X)
    delta = y - X @ mean
    s2 = tgt.sigma ** 2
    return -0.5 * np.log(2 * np.pi * (s2 + v)) - 0.5 * delta ** 2 / (s2 + v), (2 * v ** 2 + 4 * v * delta ** 2) / (4 * s2 ** 2)


def monte_carlo_errors(ll):
    """Standard errors (se_lppd[N], se_p_waic[N]) of lppd = log mean_s exp(ll) and of the variance of ll over INDEPENDENT
    draws, from the draws ll[S, N] themselves: the delta method for the log of a mean, and sqrt((m4 - m2^2) / S)."""
    S = ll.shape[0]
    dens = np.exp(ll - ll.max(axis=0))
    c = ll - ll.mean(axis=0)
    m2, m4 = (c ** 2).mean(axis=0), (c ** 4).mean(axis=0)
    return dens.std(axis=0, ddof=1) / np.sqrt(S) / dens.mean(axis=0), np.sqrt((m4 - m2 ** 2) / S)


LADDER_SCALES = (0.1, 1.0, 10.0, 100.0)


@functools.lru_cache(maxsize=None)
def ladder():
    """The end-to-end fixture: one gaussian regression (N = 32, d = 4, sigma = 1, true coefficients of order 1) under the
    prior scales LADDER_SCALES, and 16 fresh points from the same model: (X, y, X_new, y_new, sigma)."""
    rng = np.random.default_rng(4242)
    N, d, sigma = 32, 4, 1.0
    beta = np.array([1.0, -1.5, 0.8, 1.2])
    X = rng.standard_normal((N, d))
    X[:, 0] = 1.0
    y = X @ beta + sigma * rng.standard_normal(N)
    Xn = rng.standard_normal((16, d))
    Xn[:, 0] = 1.0
    yn = Xn @ beta + sigma * rng.standard_normal(16)
    for a in (X, y, Xn, yn):
        a.setflags(write=False)
    return X, y, Xn, yn, sigma
