"""Device log-densities: what ``logp_dlogp_func`` is in this framework.

The reference takes any Python callable ``q -> (logp, dlogp)`` and calls it once per leapfrog
step (/root/reference/littlemcmc/integration.py:40,62,115). On the GPU the callable is a
``__device__`` functor compiled into the transition kernel (littlemcmc_amd/csrc/lmc_targets.hpp).
The objects here name such a functor plus its parameters; they are ALSO callable with the
reference's signature -- the call evaluates the device functor on the GPU for one point -- so
they can be passed wherever the reference expects ``logp_dlogp_func``.

:class:`GLM` is the built-in family that carries data: a bernoulli / poisson / gaussian regression on ``X`` and ``y``.

Arbitrary densities are supported three ways: :class:`UserTarget` compiles a user-supplied HIP snippet into the
kernels (the fast path), :class:`TorchTarget` takes a batched torch callable on the GPU, and a plain per-point
Python callable -- the reference's own plug-in signature -- is wrapped in :class:`CallableTarget`: the sampler still
runs in the HIP tick kernel, the user's function is evaluated on the host between ticks (compatibility path).
"""
import hashlib
import os

import numpy as np

from . import _abi, _build


class DeviceTarget:
    """Base: a device functor family + its parameter vector."""

    family = None
    lib_path = None  # default library

    def __init__(self, d, params=()):
        self.d = int(d)
        self.params = np.ascontiguousarray(params, dtype=np.float64)
        self._eval_engine = None

    # reference plug-in signature, evaluated on the GPU
    def __call__(self, q):
        from .engine import Engine

        if self._eval_engine is None:
            self._eval_engine = Engine(self, chains=1)
        logp, grad = self._eval_engine.logp_dlogp(np.asarray(q, dtype=np.float64).reshape(1, self.d))
        return self._wrap_logp(logp[0]), grad[0]

    def _wrap_logp(self, logp):
        return np.float64(logp)

    def __getstate__(self):  # picklable like the reference requires (docs/tutorials/quickstart.rst:42-46)
        st = dict(self.__dict__)
        st["_eval_engine"] = None
        return st


class StdNormal(DeviceTarget):
    """logp = -1/2 sum q^2."""

    family = _abi.TARGET_STD_NORMAL

    def __init__(self, d):
        super().__init__(d)


class DiagGaussian(DeviceTarget):
    """Independent Gaussian with precisions ``prec`` (1/sigma^2)."""

    family = _abi.TARGET_DIAG_GAUSSIAN

    def __init__(self, prec):
        prec = np.ascontiguousarray(prec, dtype=np.float64)
        super().__init__(prec.shape[0], prec)

    @classmethod
    def ill_conditioned(cls, d, kappa=1e4):
        i = np.arange(d, dtype=np.float64)
        return cls(1.0 / (kappa ** (i / max(d - 1, 1))))


class AR1(DeviceTarget):
    """Stationary AR(1) Gaussian with unit marginal variances (tridiagonal precision)."""

    family = _abi.TARGET_AR1

    def __init__(self, d, rho=0.9):
        c = 1.0 / (1.0 - rho * rho)
        super().__init__(d, [c, (1.0 + rho * rho) * c, -rho * c])
        self.rho = float(rho)


class Funnel(DeviceTarget):
    """Neal's funnel: q_0 ~ N(0, 9), q_i | q_0 ~ N(0, exp(q_0))."""

    family = _abi.TARGET_FUNNEL

    def __init__(self, d):
        super().__init__(d)


class Normal1D(DeviceTarget):
    """The reference's 1-D test target (tests/test_utils.py:19-28): logp has shape (1,)."""

    family = _abi.TARGET_NORMAL1D

    def __init__(self, loc=0.0, scale=1.0):
        super().__init__(1, [loc, scale])

    def _wrap_logp(self, logp):
        return np.array([logp])


def glm_ns(d):
    """Elements per lane of a one-wavefront chain of dimension ``d``: ceil(d / 64) rounded up to a power of two."""
    need, ns = (int(d) + 63) // 64, 1
    while ns < need:
        ns *= 2
    return ns


def glm_row_layout(n_obs, d):
    """Offsets (in doubles) of the sections of a GLM parameter row (include/lmc_hip.h: LMC_TARGET_GLM):
    ``dict(npad, d8, dpad, y, xt, xr, size)``. They depend on (N, d) only, and all of them are even."""
    n_obs, d = int(n_obs), int(d)
    npad = (n_obs + 63) // 64 * 64
    d8 = (d + 7) // 8 * 8
    dpad = 64 * glm_ns(d)
    y0 = _abi.GLM_HEADER
    xt0 = y0 + npad
    xr0 = xt0 + d8 * npad
    return dict(npad=npad, d8=d8, dpad=dpad, y=y0, xt=xt0, xr=xr0, size=xr0 + npad * dpad)


def glm_row(X, y, code, tau, isig2):
    """The parameter row of a GLM: header {likelihood code, N, npad, tau, isig2, d, dpad, 0}, y[npad], Xt[d8][npad] (the eta
    pass reads an observation per lane, eight rows at a time), Xr[npad][dpad] (the gradient pass reads a lane's coefficients
    of one observation); everything beyond n = N or e = d is zero."""
    n_obs, d = X.shape
    lay = glm_row_layout(n_obs, d)
    if lay["size"] >= _abi.GLM_MAX_ROW:
        raise ValueError("GLM: N = %d observations at d = %d make a parameter row of %d doubles; the device addresses a row "
                         "with 32-bit byte offsets (below %d doubles)" % (n_obs, d, lay["size"], _abi.GLM_MAX_ROW))
    row = np.zeros(lay["size"], dtype=np.float64)
    row[:7] = [code, n_obs, lay["npad"], tau, isig2, d, lay["dpad"]]
    row[lay["y"]:lay["y"] + n_obs] = y
    row[lay["xt"]:lay["xr"]].reshape(lay["d8"], lay["npad"])[:d, :n_obs] = X.T
    row[lay["xr"]:].reshape(lay["npad"], lay["dpad"])[:n_obs, :d] = X
    return row


class GLM(DeviceTarget):
    """A regression posterior that carries its data: ``GLM(X, y, likelihood="bernoulli" | "poisson" | "gaussian",
    prior_scale=1.0, sigma=1.0)`` with ``X`` float64 ``[N, d]``, ``y`` float64 ``[N]`` and coefficients ``q`` of length
    ``d = X.shape[1]``. The linear predictor is ``eta = X q`` (an intercept is a column of ones in ``X``; there is no offset),
    the prior ``q_e ~ N(0, prior_scale**2)``:

        logp = sum_n l_n - tau/2 sum_e q_e^2,    g_e = sum_n X[n, e] r_n - tau q_e,    tau = prior_scale**-2

        bernoulli (logit link, y in {0, 1}):  l = y eta - softplus(eta),           r = y - sigmoid(eta)
        poisson   (log link, y >= 0):         l = y eta - exp(eta),                r = y - exp(eta)
        gaussian  (identity, known sigma):    l = -(y - eta)^2 / (2 sigma^2),      r = (y - eta) / sigma^2

    Additive constants that do not depend on ``q`` are DROPPED (log y!, log(sigma sqrt(2 pi)), the prior's normaliser): the
    value is the log posterior up to a constant, which is all a sampler needs; it is not a normalised log-likelihood.
    softplus and sigmoid are evaluated in their stable forms (finite for |eta| up to 800 and beyond); an overflowing exp(eta)
    of the poisson likelihood gives a non-finite logp, which the sampler reports as a divergence.

    One chain is one wavefront, so ``d <= 512``. The target is a plain device target -- NUTS / HMC, ``thin=``,
    ``rng="counter"``, dense mass matrices, ``devices=`` -- and a member of :class:`Batched`: the same model on many data
    sets is ``Batched([GLM(X_g, y_g, ...) for g in ...])`` with equal ``N``, ``d`` and likelihood."""

    family = _abi.TARGET_GLM
    LIKELIHOODS = {"bernoulli": _abi.GLM_BERNOULLI, "poisson": _abi.GLM_POISSON, "gaussian": _abi.GLM_GAUSSIAN}

    def __init__(self, X, y, likelihood="bernoulli", prior_scale=1.0, sigma=1.0):
        X = np.array(X, dtype=np.float64, order="C")
        y = np.array(y, dtype=np.float64, order="C")
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("GLM: X must be [N, d] with N, d >= 1 (got shape %s)" % (X.shape,))
        if y.shape != (X.shape[0],):
            raise ValueError("GLM: y must be [N] = [%d] (got shape %s)" % (X.shape[0], y.shape))
        if X.shape[1] > _abi.GLM_MAX_DIM:
            raise ValueError("GLM: d = %d is beyond %d (one wavefront per chain); use a TorchTarget for wider models"
                             % (X.shape[1], _abi.GLM_MAX_DIM))
        if likelihood not in self.LIKELIHOODS:
            raise ValueError("GLM: likelihood must be one of %s (got %r)" % (sorted(self.LIKELIHOODS), likelihood))
        if not (np.isfinite(X).all() and np.isfinite(y).all()):
            raise ValueError("GLM: X and y must be finite")
        if likelihood == "bernoulli" and not np.isin(y, (0.0, 1.0)).all():
            raise ValueError("GLM: bernoulli y must be 0 or 1")
        if likelihood == "poisson" and (y < 0).any():
            raise ValueError("GLM: poisson y must be >= 0")
        prior_scale, sigma = float(prior_scale), float(sigma)
        if not (np.isfinite(prior_scale) and prior_scale > 0.0 and np.isfinite(sigma) and sigma > 0.0):
            raise ValueError("GLM: prior_scale and sigma must be positive and finite (got %r, %r)" % (prior_scale, sigma))
        self.X, self.y = X, y
        self.likelihood = likelihood
        self.n_obs = X.shape[0]
        self.prior_scale, self.sigma = prior_scale, sigma
        self.tau, self.isig2 = prior_scale ** -2, sigma ** -2
        if not (np.isfinite(self.tau) and self.tau > 0.0 and np.isfinite(self.isig2) and self.isig2 > 0.0):
            raise ValueError("GLM: prior_scale**-2 and sigma**-2 must be positive and finite")
        super().__init__(X.shape[1], glm_row(X, y, self.LIKELIHOODS[likelihood], self.tau, self.isig2))

    def posterior_gaussian(self):
        """``(mean[d], cov[d, d])`` of the exact posterior of the gaussian likelihood (host numpy):
        ``cov = (X'X / sigma^2 + tau I)^-1``, ``mean = cov X'y / sigma^2``."""
        if self.likelihood != "gaussian":
            raise ValueError("posterior_gaussian() is the closed form of likelihood='gaussian' (this is %r)" % self.likelihood)
        prec = self.X.T @ self.X * self.isig2 + self.tau * np.eye(self.d)
        cov = np.linalg.inv(prec)
        cov = 0.5 * (cov + cov.T)
        return np.linalg.solve(prec, self.X.T @ self.y * self.isig2), cov

    def loglik_constant(self, y=None):
        """``const[N]``: what the pointwise log-likelihood ``l_n`` above drops, so that ``l_n + const_n`` is the normalised
        log density of ``y_n`` (default: the target's own ``y``): 0 (bernoulli), ``-lgamma(y + 1)`` (poisson),
        ``-log(sigma) - log(2 pi) / 2`` (gaussian)."""
        import math

        y = self.y if y is None else np.asarray(y, dtype=np.float64)
        if self.likelihood == "poisson":
            return np.array([-math.lgamma(float(v) + 1.0) for v in y], dtype=np.float64).reshape(y.shape)
        if self.likelihood == "gaussian":
            return np.full(y.shape, -math.log(self.sigma) - 0.5 * math.log(2.0 * math.pi))
        return np.zeros(y.shape)

    def pointwise_stats(self, x, **kw):
        """``predictive.pointwise_stats(x, self, ...)``: the per-observation statistics of the draws ``x`` in HBM, ``[1, N]``."""
        from . import predictive

        return predictive.pointwise_stats(x, self, **kw)

    def waic(self, x, **kw):
        """``predictive.waic(x, self, ...)``: lppd / WAIC of the draws ``x`` in HBM (leading axis 1); ``data=(X_new, y_new)``
        scores held-out points."""
        from . import predictive

        return predictive.waic(x, self, **kw)

    def loo(self, x, **kw):
        """``predictive.loo(x, self, ...)``: PSIS-LOO of the draws ``x`` in HBM (leading axis 1) -- ``elpd_loo``, and per
        observation ``elpd_loo_i`` and the Pareto shape ``pareto_k`` that says where the estimate can be trusted."""
        from . import predictive

        return predictive.loo(x, self, **kw)

    def predict(self, x, X_new=None, **kw):
        """``predictive.predict(x, self, X_new, ...)``: posterior predictions at the points ``X_new[N_new, d]`` (default: the
        training design) from the draws ``x`` in HBM (leading axis 1) -- mean and sd of the linear predictor and of the mean
        response, their exact credible bands, and the mean and variance of a new response."""
        from . import predictive

        return predictive.predict(x, self, X_new, **kw)

    def replicate(self, x, X_new=None, **kw):
        """``predictive.replicate(x, self, X_new, ...)``: the replicated responses ``y_rep[chains, draws, W]`` of every draw in
        HBM at ``X_new`` (default: the training design), a pure function of ``random_seed``."""
        from . import predictive

        return predictive.replicate(x, self, X_new, **kw)

    def predict_response(self, x, X_new=None, **kw):
        """``predictive.predict_response(x, self, X_new, ...)``: the prediction band of a NEW response at ``X_new`` -- exact
        quantiles ``y_quantiles[1, P, N_new]``, ``y_min``, ``y_max`` of the replicated responses of the draws in HBM."""
        from . import predictive

        return predictive.predict_response(x, self, X_new, **kw)

    def ppc(self, x, **kw):
        """``predictive.ppc(x, self, ...)``: posterior predictive checks of the draws ``x`` in HBM (leading axis 1) -- mean, sd,
        min, max, zeros and Pearson chi-square of replicated data sets against the observed ``y``, with their p-values."""
        from . import predictive

        return predictive.ppc(x, self, **kw)

    def covariance(self, x, **kw):
        """``diagnostics.covariance(x, ...)``: posterior covariance, correlation and sd of the coefficients from the draws ``x`` in
        HBM -- ``cov[d, d]``, ``corr[d, d]``, ``sd[d]``, ``mean[d]``."""
        from . import diagnostics

        return diagnostics.covariance(x, target=self, **kw)

    def contrasts(self, x, L, **kw):
        """``diagnostics.contrasts`` of ``covariance(x, ...)``: mean[k], sd[k] and cov[k, k] of the combinations ``L q``, L [k, d]."""
        from . import diagnostics

        return diagnostics.contrasts(self.covariance(x, **kw), L, ddof=kw.get("ddof", 1))

    def prob(self, x, thresholds, **kw):
        """``diagnostics.prob(x, thresholds, ...)``: ``p_less``, ``p_equal``, ``p_greater`` ``[K, d]`` of the coefficients against
        the thresholds, counted over the draws ``x`` in HBM; ``prob(x, 0.0)["p_greater"]`` is P(q_e > 0)."""
        from . import diagnostics

        diagnostics._trace_job(x, None, 0, self, whole_job=True)
        return diagnostics.prob(x, thresholds, **kw)

    def direction(self, x, **kw):
        """``diagnostics.direction(x, ...)``: the probability of direction ``pd[d]`` and its ``sign[d]``."""
        from . import diagnostics

        diagnostics._trace_job(x, None, 0, self, whole_job=True)
        return diagnostics.direction(x, **kw)

    def rope(self, x, low, high, **kw):
        """``diagnostics.rope(x, low, high, ...)``: ``inside = P(low <= q <= high)``, ``below``, ``above`` ``[d]``."""
        from . import diagnostics

        diagnostics._trace_job(x, None, 0, self, whole_job=True)
        return diagnostics.rope(x, low, high, **kw)

    def exceedance(self, x, X_new=None, **kw):
        """``predictive.exceedance(x, self, X_new, ...)``: P(prediction < t) at the points ``X_new`` (default: the training
        design) -- ``p_less``, ``p_equal``, ``p_greater`` ``[1, K, N_new]`` on the scale ``"eta"`` or ``"mu"``."""
        from . import predictive

        return predictive.exceedance(x, self, X_new, **kw)

    def __repr__(self):
        return "GLM(%s, N=%d, d=%d)" % (self.likelihood, self.n_obs, self.d)


class UserTarget(DeviceTarget):
    """A user-written device log-density, compiled at run time and linked into the kernels.

    ``source`` must define, in namespace ``lmc``::

        template <int NS> struct UserTarget {
            static constexpr bool kLanePartial = false;
            template <class Team> __device__ void init(Team& tm, const double* params, int d);
            template <class Team> __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const;
        };

    following the thread-distributed contract documented in csrc/lmc_targets.hpp.

    ``jit="hiprtc"`` (default): when an engine is created, the three kernels that depend on the functor -- the
    transition kernel of the engine's shape, the trajectory and the log-density unit kernels -- are compiled in
    process with hiprtc (2-4 s -- one-wavefront shapes compile the sampling kernel twice, once per LDS plan, so that the
    engine can choose the plan per launch as for the built-in densities; cached by content under ``_user_targets/``, which
    is never shipped to another machine) and handed to the stock library
    (``lmc_engine_load_user_kernels``); no compiler is needed on the machine. Diagonal mass matrices.
    ``jit="hipcc"``: a private build of the whole library around the functor (about 10 s, needs hipcc); this is the
    path for dense mass matrices with a user density."""

    family = _abi.TARGET_USER

    def __init__(self, d, source, params=(), jit="hiprtc"):
        super().__init__(d, params)
        self.source = source
        if jit not in ("hiprtc", "hipcc"):
            raise ValueError("jit must be 'hiprtc' or 'hipcc'")
        self.jit = jit
        self._code = {}   # (unit_ns, run_ns, run_w) -> (code object bytes, lowered names)
        if jit == "hipcc":
            self.lib_path = self._build_private_library()

    # ---- hiprtc: the target-dependent kernels only ---------------------------------------------------------
    def _digest(self, extra=""):
        # the cache key covers everything the binary depends on: the snippet, the kernel sources and the compiler flags
        h = hashlib.sha256(self.source.encode())
        for path in _build.sources():
            with open(path, "rb") as fh:
                h.update(fh.read())
        h.update(" ".join(_build.HIPCC_FLAGS).encode())
        h.update(extra.encode())
        return h.hexdigest()[:16]

    def kernels_for(self, unit_ns, run_ns, run_w, general=False, counter=False):
        """(code object, run name, trajectory name, logp name, run name under LDS plan 1 or None) for one engine shape,
        compiled once and cached. ``counter``: the sampling kernel of an rng="counter" engine, run_kernel<NS, W, UserTarget, 2>
        (one LDS layout: no plan-1 kernel)."""
        key = (int(unit_ns), int(run_ns), int(run_w), int(bool(general)), int(bool(counter)))
        if key[3] and key[4]:
            raise ValueError("rng='counter' runs in the fused kernels only")
        if key in self._code:
            return self._code[key]
        if key[3]:   # the general kernels (csrc/lmc_wide.hpp): model_ndim > 1024, dense mass matrices, float64 masses
            names = ["lmc::run_wide_kernel<%d, %d, lmc::UserTarget>" % (key[1], key[2]),
                     "lmc::wide_trajectory_kernel<%d, %d, lmc::UserTarget>" % (key[0], key[2]),
                     "lmc::wide_logp_kernel<%d, %d, lmc::UserTarget>" % (key[0], key[2])]
            tu = ('#include "lmc_wide.hpp"\n' + self.source +
                  "\nnamespace lmc {\n"
                  "template __global__ void run_wide_kernel<%d, %d, UserTarget>(ChainArrays, DenseArrays, SamplerParams, const double*);\n"
                  "template __global__ void wide_trajectory_kernel<%d, %d, UserTarget>(ChainArrays, DenseArrays, const double*, const double*, "
                  "const double*, int, int, double, int, int, double*, double*, double*, double*, double*, double*);\n"
                  "template __global__ void wide_logp_kernel<%d, %d, UserTarget>(ChainArrays, const double*, const double*, double*, double*);\n"
                  "}\n" % (key[1], key[2], key[0], key[2], key[0], key[2]))
        else:
            run_args = "%d, %d, %sUserTarget%s" % (key[1], key[2], "%s", ", 2" if key[4] else "")
            names = ["lmc::run_kernel<%s>" % (run_args % "lmc::"),
                     "lmc::trajectory_kernel<%d, lmc::UserTarget>" % key[0],
                     "lmc::logp_kernel<%d, lmc::UserTarget>" % key[0]]
            tu = ('#include "lmc_sampler.hpp"\n#include "lmc_unit_kernels.hpp"\n' + self.source +
                  "\nnamespace lmc {\n"
                  "template __global__ void run_kernel<%s>(ChainArrays, SamplerParams, const double*);\n"
                  "template __global__ void trajectory_kernel<%d, UserTarget>(ChainArrays, const double*, const double*, const double*, "
                  "int, int, double, int, int, double*, double*, double*, double*, double*, double*);\n"
                  "template __global__ void logp_kernel<%d, UserTarget>(ChainArrays, const double*, const double*, double*, double*);\n"
                  "}\n" % (run_args % "", key[0], key[0]))
            if key[2] == 1 and not key[4]:   # one-wave kernels: also the deep-tree LDS plan (csrc/lmc_sampler.hpp: run_kernel<.., PL = 1>)
                names.append("lmc::run_kernel<%d, 1, lmc::UserTarget, 0, 1>" % key[1])
                tu += ("namespace lmc {\ntemplate __global__ void run_kernel<%d, 1, UserTarget, 0, 1>(ChainArrays, SamplerParams, "
                       "const double*);\n}\n" % key[1])
        cache = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_user_targets")
        os.makedirs(cache, exist_ok=True)
        path = os.path.join(cache, "user_%s_%d_%d_%d%s.hsaco" % (self._digest("hiprtc"), key[0], key[1], key[2],
                                                                 "g" if key[3] else "c" if key[4] else ""))
        lowered = None
        if os.path.exists(path) and os.path.exists(path + ".names"):
            with open(path, "rb") as fh:
                code = fh.read()
            with open(path + ".names") as fh:
                lowered = [ln for ln in fh.read().split("\n") if ln]
        else:
            code, lowered = _hiprtc_compile(tu, names)
            tmp = "%s.%d.tmp" % (path, os.getpid())     # several ranks may compile the same target at once
            with open(tmp, "wb") as fh:
                fh.write(code)
            os.replace(tmp, path)
            with open(tmp, "w") as fh:
                fh.write("\n".join(lowered))
            os.replace(tmp, path + ".names")
        self._code[key] = (code, lowered[0], lowered[1], lowered[2], lowered[3] if len(lowered) > 3 else None)
        return self._code[key]

    def _attach(self, engine):
        """Called by Engine after lmc_engine_create: compile (or fetch) the kernels of the engine's shape and load them."""
        if self.jit != "hiprtc":
            return
        import ctypes as C

        ns, rns, rw = C.c_int32(), C.c_int32(), C.c_int32()
        engine._check(engine._lib.lmc_engine_kernel_shape(engine._h, C.byref(ns), C.byref(rns), C.byref(rw)))
        general = bool(engine._lib.lmc_engine_uses_general_kernels(engine._h))
        counter = int(engine.cfg.rng_mode) == _abi.RNG_COUNTER
        code, run, traj, logp, run1 = self.kernels_for(ns.value, rns.value, rw.value, general, counter)
        buf = C.create_string_buffer(code, len(code))
        engine._check(engine._lib.lmc_engine_load_user_kernels(engine._h, buf, run.encode(), traj.encode(), logp.encode()))
        if run1 is not None:   # the sampling kernel under the deep-tree LDS plan: the engine may now choose per launch
            engine._check(engine._lib.lmc_engine_load_user_run_plan1(engine._h, run1.encode()))

    def __getstate__(self):
        st = super().__getstate__()
        st["_code"] = {}
        return st

    # ---- hipcc: private build of the library ------------------------------------------------------------------
    def _build_private_library(self):
        digest = self._digest("hipcc")
        cache = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_user_targets")
        os.makedirs(cache, exist_ok=True)
        header = os.path.join(cache, "user_%s.hpp" % digest)
        lib = os.path.join(cache, "liblmc_hip_user_%s.so" % digest)
        if not os.path.exists(lib):
            # several ranks may build the same target at once: private temporaries, atomic rename into place
            tmp_tag = "%d_%s" % (os.getpid(), digest)
            tmp_header = os.path.join(cache, "user_%s.tmp.hpp" % tmp_tag)
            tmp_lib = os.path.join(cache, "liblmc_hip_user_%s.tmp.so" % tmp_tag)
            with open(tmp_header, "w") as fh:
                fh.write(self.source)
            try:
                _build.build(out=tmp_lib, extra_flags=["-DLMC_USER_TARGET_HEADER=\"%s\"" % tmp_header, "-DLMC_ONLY_USER"],
                             force=True)
                os.replace(tmp_lib, lib)
                os.replace(tmp_header, header)
            finally:
                for f in (tmp_lib, tmp_header):
                    if os.path.exists(f):
                        os.remove(f)
        return lib


def _hiprtc_compile(source, name_expressions):
    """Compile a translation unit for gfx950 with hiprtc -> (code object bytes, lowered kernel names)."""
    import ctypes as C

    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    try:
        rtc = C.CDLL(os.path.join(rocm, "lib", "libhiprtc.so"))
    except OSError as err:
        raise _abi.HipLibraryError("cannot load libhiprtc.so (%s): UserTarget(jit='hiprtc') needs the ROCm runtime compiler; "
                                   "use jit='hipcc' where hipcc is installed" % err)
    rtc.hiprtcGetErrorString.restype = C.c_char_p
    prog = C.c_void_p()

    def check(rc, what):
        if rc != 0:
            n = C.c_size_t()
            rtc.hiprtcGetProgramLogSize(prog, C.byref(n))
            log = C.create_string_buffer(n.value + 1)
            rtc.hiprtcGetProgramLog(prog, log)
            raise RuntimeError("hiprtc %s failed (%s):\n%s" % (what, rtc.hiprtcGetErrorString(rc).decode(), log.value.decode()[-4000:]))

    check(rtc.hiprtcCreateProgram(C.byref(prog), source.encode(), b"lmc_user_target.hip", 0, None, None), "create")
    try:
        for n in name_expressions:
            check(rtc.hiprtcAddNameExpression(prog, n.encode()), "name expression")
        flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
        opts = [f.encode() for f in flags] + [("-I" + _build.CSRC).encode(), ("-I" + os.path.join(rocm, "include")).encode()]
        arr = (C.c_char_p * len(opts))(*opts)
        check(rtc.hiprtcCompileProgram(prog, len(opts), arr), "compile")
        size = C.c_size_t()
        check(rtc.hiprtcGetCodeSize(prog, C.byref(size)), "code size")
        code = C.create_string_buffer(size.value)
        check(rtc.hiprtcGetCode(prog, code), "code")
        lowered = []
        for n in name_expressions:
            p = C.c_char_p()
            check(rtc.hiprtcGetLoweredName(prog, n.encode(), C.byref(p)), "lowered name")
            lowered.append(p.value.decode())
        return code.raw, lowered
    finally:
        rtc.hiprtcDestroyProgram(C.byref(prog))


class TorchTarget(DeviceTarget):
    """A log-density given as a BATCHED torch callable on the GPU, for densities that are easier to write (or
    differentiate) in torch than as a HIP functor (reference cookbook: docs/_static/scripts/
    sample_pytorch_logp_dlogp_func.py).

        fn(q: float64 cuda tensor [chains, d]) -> (logp [chains], dlogp [chains, d])

    The sampler then runs as a resumable kernel (csrc/lmc_tick.hpp): every "tick" each chain hands over the one
    point it needs the density at, ``fn`` evaluates all chains at once, and the kernel carries every chain on to
    its next evaluation -- finishing leapfrogs, building trees, adapting, starting new iterations -- without
    the chains ever waiting for each other. Nothing is computed on the CPU.

    ``TorchTarget.from_logp(d, logp_fn)`` builds the gradient with autograd from ``logp_fn(q) -> [chains]``.
    Limits: d <= 16 384 with diagonal mass matrices (beyond 1 024 the chain is a workgroup of 16 wavefronts:
    csrc/lmc_tick.hpp: tick_step with TickWideShape, lmc_wide.hip); dense mass matrices (QuadPotentialFull*, init="adapt_full") as for
    the fused kernels up to d = 256. A fused ``UserTarget`` is several times faster (no HBM round trip of
    the chain state per leapfrog); this is the path for "cannot write device code".
    """

    family = _abi.TARGET_EXTERNAL

    def __init__(self, d, fn, graph=False):
        super().__init__(d)
        if not callable(fn):
            raise TypeError("fn must be callable: q[chains, d] -> (logp[chains], dlogp[chains, d])")
        self.fn = fn
        # graph=True: capture fn once into a HIP graph (torch.cuda.CUDAGraph) and replay it every tick. The points
        # always live in the same engine-owned buffer, so the capture is valid for the whole run; it removes the
        # host-side launch cost of fn's kernels (what bounds small batches). fn must be capturable: no host
        # synchronisation, no data-dependent shapes.
        self.graph = bool(graph)

    @classmethod
    def from_logp(cls, d, logp_fn, graph=False):
        import torch

        def fn(q):
            with torch.enable_grad():
                x = q.detach().requires_grad_(True)
                lp = logp_fn(x)
                (g,) = torch.autograd.grad(lp.sum(), x)
            return lp.detach(), g

        return cls(d, fn, graph=graph)

    @classmethod
    def from_pointwise(cls, d, fn, graph=False):
        """``fn(q: tensor[d]) -> (logp: scalar tensor, dlogp: tensor[d])`` written in torch ops for ONE point -- the
        reference's plug-in signature (integration.py:40,62,115) -- batched over the chains with ``torch.vmap``."""
        import torch

        batched = torch.vmap(fn)
        return cls(d, lambda q: batched(q), graph=graph)

    def evaluate(self, q):
        """fn on a [chains, d] tensor, results checked and made contiguous float64."""
        import torch

        logp, grad = self.fn(q)
        if logp.shape != (q.shape[0],) and logp.numel() == q.shape[0]:
            logp = logp.reshape(q.shape[0])
        if logp.shape != (q.shape[0],) or grad.shape != q.shape:
            raise ValueError("TorchTarget fn must return (logp[chains], dlogp[chains, d]); got %s and %s for q %s"
                             % (tuple(logp.shape), tuple(grad.shape), tuple(q.shape)))
        if not (logp.is_cuda and grad.is_cuda):
            raise TypeError("TorchTarget fn must return CUDA (ROCm) tensors: there is no CPU path")
        return logp.to(torch.float64).contiguous(), grad.to(torch.float64).contiguous()

    def __call__(self, q):   # reference plug-in signature, one point
        import torch

        x = torch.as_tensor(np.asarray(q, dtype=np.float64).reshape(1, self.d), device="cuda")
        logp, grad = self.evaluate(x)
        return np.float64(logp[0].item()), grad[0].cpu().numpy()

    def __getstate__(self):
        return dict(self.__dict__)


class CallableTarget(TorchTarget):
    """The reference's own plug-in, unchanged: a per-point Python callable ``fn(q: ndarray[d]) -> (logp, dlogp[d])``
    (integration.py:40,62,115; e.g. tests/test_utils.py:19-28 or docs/_static/scripts/
    sample_pytorch_logp_dlogp_func.py:35-45 with CPU tensors).

    The sampler itself -- leapfrog, trees, adaptation, RNG -- still runs in the HIP tick kernel (csrc/lmc_tick.hpp);
    only the user's density is evaluated where the user's code lives: every tick the points of all chains are copied
    to the host, ``fn`` is called once per chain, and the values go back for the next tick. This is the compatibility
    path (C1-sized jobs: a handful of chains); a :class:`UserTarget` or a batched :class:`TorchTarget` is what the
    many-chain configurations need. ``sample()`` / ``NUTS`` / ``HamiltonianMC`` wrap a plain callable in it."""

    tick_poll = 1   # look at the number of unfinished chains after every tick: no wasted host evaluations

    def __init__(self, d, fn):
        if not callable(fn):
            raise TypeError("fn must be callable: q[d] -> (logp, dlogp[d])")
        self.pointwise = fn
        super().__init__(d, self._batched, graph=False)

    @staticmethod
    def _host(x):
        if hasattr(x, "detach"):   # a torch tensor (CPU or device)
            x = x.detach().cpu().numpy()
        return np.asarray(x, dtype=np.float64)

    def _batched(self, q):
        import torch

        host = q.detach().cpu().numpy()
        logp = np.empty(host.shape[0])
        grad = np.empty_like(host)
        for c in range(host.shape[0]):
            lp, dlp = self.pointwise(host[c].copy())
            logp[c] = self._host(lp).reshape(-1)[0]          # scalar or shape-(1,) array (tests/test_utils.py:27-28)
            grad[c] = self._host(dlp).reshape(self.d)
        return torch.from_numpy(logp).to(q.device), torch.from_numpy(grad).to(q.device)

    def __call__(self, q):   # the callable itself, as the reference would call it
        return self.pointwise(np.asarray(q, dtype=np.float64))


_SEPARABLE_TEMPLATE = r"""
#include "lmc_team.hpp"
namespace lmc {
// generated by littlemcmc_amd.targets.UserTarget.separable: logp(q) = sum_e term(q_e, e; P)
template <int NS>
struct UserTarget {
    static constexpr bool kLanePartial = true;
    const double* P;
    int d;
    template <class Team>
    __device__ void init(Team&, const double* params, int d_) { P = params; d = d_; }
    template <class Team>
    __device__ double logp_grad_partial(Team& tm, const double (&qv)[NS], double (&g)[NS]) const {
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = tm.tid() * NS + s;
            if (e < d) {
                const double q = qv[s];
                %(prelude)s
                g[s] = (%(grad)s);
                part += (%(logp)s);
            } else {
                g[s] = 0.0;
            }
        }
        return part;
    }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&qv)[NS], double (&g)[NS]) const {
        return tm.sum(logp_grad_partial(tm, qv, g));
    }
};
}  // namespace lmc
"""


def _separable(cls, d, logp, grad, params=(), prelude=""):
    """A product density prod_e f(q_e): give the per-coordinate log term and its derivative as C expressions in
    ``q`` (the coordinate), ``e`` (its index) and ``P`` (the parameter vector), e.g. a Student-t with P[0] = nu:

        UserTarget.separable(d, logp="-0.5*(P[0]+1.0)*log1p(q*q/P[0])", grad="-(P[0]+1.0)*q/(P[0]+q*q)", params=[4.0])
    """
    src = _SEPARABLE_TEMPLATE % {"logp": logp, "grad": grad, "prelude": prelude}
    return cls(d, src, params=params)


UserTarget.separable = classmethod(_separable)


class Batched(DeviceTarget):
    """Many posteriors in one job: ``Batched([member_0, ..., member_{G-1}])`` is the same device density with one parameter
    vector per GROUP of chains -- the same model on G data sets, a temperature or prior-scale ladder, a sensitivity sweep.
    ``sample(batched, chains=C)`` deals the chains to the groups in contiguous blocks of ``C // G`` (``C % G`` must be 0):
    chain j samples ``members[j // (C // G)]``, so ``trace.reshape(G, C // G, draws, d)`` is the per-posterior view and every
    chain is, bit for bit, the chain of the same index of ``sample(batched[g], chains=C)`` on the same seeds.

    The members are device targets of ONE class with the same ``d`` and the same number of parameters (``UserTarget``
    members: the same ``source`` and ``jit`` too -- the kernels are those of member 0, compiled once); ``TorchTarget``,
    ``CallableTarget`` and nested ``Batched`` members are refused (a callable already sees all chains and can tell them
    apart itself). ``params`` is the ``[G, n]`` table the engine uploads (lmc_engine_set_target_params_grouped: the kernels
    pick a chain's row where they call the functor's ``init``), ``groups`` is G, ``members`` the list; ``batched[g]`` is member g
    and ``len(batched)`` is G. A ``Batched`` cannot be called with one point -- a point has no group: call ``batched[g](q)``.

    Diagnostics are per posterior: ``batched.summarize(x)`` gives R-hat / ESS ``[G, d]`` of all groups in one pass over the
    draws in HBM (``trace[sl]`` for ``sl`` in ``chain_slices(chains)`` are the chains of one group). R-hat ACROSS groups is
    meaningless -- the groups' chains target different distributions and are supposed to disagree."""

    def __init__(self, members):
        members = list(members)
        if not members:
            raise ValueError("Batched needs at least one member target")
        first = members[0]
        for g, m in enumerate(members):
            if not isinstance(m, DeviceTarget):
                raise TypeError("Batched member %d is not a device target: %r" % (g, m))
            if isinstance(m, (TorchTarget, Batched)):
                raise TypeError("Batched member %d is a %s: a callable density already sees all chains (tell them apart in "
                                "the callable), and a Batched cannot be nested" % (g, type(m).__name__))
            if type(m) is not type(first):
                raise TypeError("Batched member %d is a %s, member 0 a %s: the members share one class (one device functor)"
                                % (g, type(m).__name__, type(first).__name__))
            if m.d != first.d:
                raise ValueError("Batched member %d has d = %d, member 0 has d = %d" % (g, m.d, first.d))
            if m.params.shape != first.params.shape or m.params.ndim != 1:
                raise ValueError("Batched member %d has %s parameters, member 0 has %s"
                                 % (g, m.params.shape, first.params.shape))
            if isinstance(m, GLM) and (m.likelihood != first.likelihood or m.n_obs != first.n_obs):
                raise ValueError("Batched member %d is a %s GLM of N = %d, member 0 a %s GLM of N = %d: the members share one "
                                 "likelihood and one number of observations (rows of equal length can still differ in both)"
                                 % (g, m.likelihood, m.n_obs, first.likelihood, first.n_obs))
            if isinstance(m, UserTarget) and (m.source != first.source or m.jit != first.jit):
                raise ValueError("Batched member %d has another source or jit than member 0: the members share one "
                                 "compiled density and differ in their parameters only" % g)
        super().__init__(first.d, np.stack([m.params for m in members]).reshape(len(members), first.params.size))
        self.members = members
        self.groups = len(members)
        self.family = first.family
        self.lib_path = first.lib_path

    def __len__(self):
        return self.groups

    def __getitem__(self, g):
        return self.members[g]

    def __call__(self, q):
        raise TypeError("a Batched target holds %d posteriors and one point has no group: call batched[g](q) for the "
                        "density of group g" % self.groups)

    def _wrap_logp(self, logp):
        return self.members[0]._wrap_logp(logp)

    # the kernels are member 0's: compiled (or fetched) once for all groups
    def kernels_for(self, *args, **kwargs):
        return self.members[0].kernels_for(*args, **kwargs)

    def _attach(self, engine):
        attach = getattr(self.members[0], "_attach", None)
        if attach is not None:
            attach(engine)

    @staticmethod
    def row_of_chain(chain, first_chain=0, chains_per_group=1):
        """The group (row of ``params``) of chain ``chain`` of an engine whose chain 0 is chain ``first_chain`` of the job,
        with ``chains_per_group`` chains per group: the host mirror of lmc_target_param_row."""
        chain, first_chain, chains_per_group = int(chain), int(first_chain), int(chains_per_group)
        if chain < 0 or first_chain < 0 or chains_per_group < 1:
            raise ValueError("row_of_chain needs chain, first_chain >= 0 and chains_per_group >= 1 (got %r)"
                             % ((chain, first_chain, chains_per_group),))
        return (first_chain + chain) // chains_per_group

    def group_size(self, chains):
        """``chains // groups`` of a job of ``chains`` chains; ValueError unless the chains can be dealt evenly."""
        chains = int(chains)
        if chains < self.groups or chains % self.groups != 0:
            raise ValueError("a Batched target of %d groups needs a multiple of %d chains (got chains=%d)"
                             % (self.groups, self.groups, chains))
        return chains // self.groups

    def chain_slices(self, chains):
        """One ``slice`` of the chain axis per group for a job of ``chains`` chains: ``trace[sl]`` are the chains of one
        posterior -- what R-hat / ESS are taken over (across groups they are meaningless)."""
        per = self.group_size(chains)
        return [slice(g * per, (g + 1) * per) for g in range(self.groups)]

    def summarize(self, x, **kw):
        """``diagnostics.summarize`` per posterior: x is the job's draws in HBM, one tensor [chains, draws, d] or the list of
        per-GPU blocks from ``diagnostics.trace_tensor(engine_group)`` -> rhat[G, d], ess[G, d], rhat_max[G], ess_min[G], ..."""
        from . import diagnostics

        chains = sum(int(b.shape[0]) for b in x) if isinstance(x, (list, tuple)) else int(x.shape[0])
        return diagnostics.summarize(x, chains_per_group=self.group_size(chains), **kw)

    def _per(self, x):
        return self.group_size(sum(int(b.shape[0]) for b in x) if isinstance(x, (list, tuple)) else int(x.shape[0]))

    def quantiles(self, x, probs, **kw):
        """``diagnostics.quantiles`` per posterior: exact quantiles[G, Q, d], min[G, d], max[G, d] from the draws in HBM (one
        tensor or the list of per-GPU blocks)."""
        from . import diagnostics

        return diagnostics.quantiles(x, probs, chains_per_group=self._per(x), **kw)

    def intervals(self, x, level=0.9, **kw):
        """``diagnostics.intervals`` per posterior: equal-tailed lower[G, d], median[G, d], upper[G, d]."""
        from . import diagnostics

        return diagnostics.intervals(x, level, chains_per_group=self._per(x), **kw)

    def tail_ess(self, x, **kw):
        """``diagnostics.tail_ess`` per posterior: ess_tail[G, d], ess_tail_min[G]."""
        from . import diagnostics

        return diagnostics.tail_ess(x, chains_per_group=self._per(x), **kw)

    def covariance(self, x, **kw):
        """``diagnostics.covariance`` per posterior: cov[G, d, d], corr[G, d, d], sd[G, d], mean[G, d], n[G] from the draws in
        HBM (one tensor or the list of per-GPU blocks); ``cov[g]`` is a dense mass matrix for a rerun of posterior g."""
        from . import diagnostics

        return diagnostics.covariance(x, chains_per_group=self._per(x), **kw)

    def contrasts(self, x, L, **kw):
        """``diagnostics.contrasts`` of ``covariance(x, ...)`` per posterior: mean[G, k], sd[G, k], cov[G, k, k] of the
        combinations ``L q``, L [k, d] (the same for every posterior) or [G, k, d]."""
        from . import diagnostics

        return diagnostics.contrasts(self.covariance(x, **kw), L, ddof=kw.get("ddof", 1))

    def prob(self, x, thresholds, **kw):
        """``diagnostics.prob`` per posterior: ``p_less``, ``p_equal``, ``p_greater`` ``[G, K, d]`` against the thresholds ([K, d]
        shared, or [G, K, d]), counted over the draws in HBM (one tensor or the list of per-GPU blocks)."""
        from . import diagnostics

        return diagnostics.prob(x, thresholds, chains_per_group=self._per(x), **kw)

    def direction(self, x, **kw):
        """``diagnostics.direction`` per posterior: the probability of direction ``pd[G, d]`` and its ``sign[G, d]``."""
        from . import diagnostics

        return diagnostics.direction(x, chains_per_group=self._per(x), **kw)

    def rope(self, x, low, high, **kw):
        """``diagnostics.rope`` per posterior: ``inside = P(low <= q <= high)``, ``below``, ``above`` ``[G, d]``."""
        from . import diagnostics

        return diagnostics.rope(x, low, high, chains_per_group=self._per(x), **kw)

    def exceedance(self, x, X_new=None, **kw):
        """``predictive.exceedance(x, self, X_new, ...)`` per posterior (GLM members): P(prediction < t) at ``X_new`` --
        ``p_less``, ``p_equal``, ``p_greater`` ``[G, K, N_new]`` on the scale ``"eta"`` or ``"mu"``."""
        from . import predictive

        return predictive.exceedance(x, self, X_new, **kw)

    def pointwise_stats(self, x, **kw):
        """``predictive.pointwise_stats(x, self, ...)`` per posterior (GLM members): the per-observation statistics ``[G, N]``."""
        from . import predictive

        return predictive.pointwise_stats(x, self, **kw)

    def waic(self, x, **kw):
        """``predictive.waic(x, self, ...)`` per posterior (GLM members): lppd[G, N], elpd_waic[G], se[G], ... of all groups in
        one pass over the draws in HBM; ``data=[(X_new, y_new), ...]`` scores a held-out fold per group."""
        from . import predictive

        return predictive.waic(x, self, **kw)

    def loo(self, x, **kw):
        """``predictive.loo(x, self, ...)`` per posterior (GLM members): PSIS-LOO ``elpd_loo[G]``, ``elpd_loo_i[G, N]``,
        ``pareto_k[G, N]``, ``n_bad_k[G]``, ... of all groups from the draws in HBM, without a refit."""
        from . import predictive

        return predictive.loo(x, self, **kw)

    def predict(self, x, X_new=None, **kw):
        """``predictive.predict(x, self, X_new, ...)`` per posterior (GLM members): predictions at ``X_new``, a list of G arrays
        ``[N_new, d]`` with one common N_new (default: each member's training design) -- ``eta_mean[G, N_new]``,
        ``mu_quantiles[G, Q, N_new]``, ``y_mean``, ``y_var``, ... of all groups from the draws in HBM."""
        from . import predictive

        return predictive.predict(x, self, X_new, **kw)

    def replicate(self, x, X_new=None, **kw):
        """``predictive.replicate(x, self, X_new, ...)`` (GLM members): the replicated responses ``y_rep[chains, draws, W]`` of
        every draw at ``X_new`` (a list of G designs; default: each member's training design)."""
        from . import predictive

        return predictive.replicate(x, self, X_new, **kw)

    def predict_response(self, x, X_new=None, **kw):
        """``predictive.predict_response(x, self, X_new, ...)`` per posterior (GLM members): the prediction band of a new
        response, ``y_quantiles[G, P, N_new]``, ``y_min``, ``y_max``, from the draws in HBM."""
        from . import predictive

        return predictive.predict_response(x, self, X_new, **kw)

    def ppc(self, x, **kw):
        """``predictive.ppc(x, self, ...)`` per posterior (GLM members): posterior predictive checks ``T_obs[G, 5]``,
        ``T_rep_mean``, ``T_rep_quantiles``, ``p_value[G, 6]`` of all groups in one pass over the draws in HBM."""
        from . import predictive

        return predictive.ppc(x, self, **kw)

    def __repr__(self):
        return "Batched(%d x %s, d=%d)" % (self.groups, type(self.members[0]).__name__, self.d)


def require_device_target(logp_dlogp_func, model_ndim=None):
    """What the step methods and ``sample()`` accept as ``logp_dlogp_func``: a device functor (inlined into the
    leapfrog kernel), a batched torch callable (TorchTarget) or -- the reference's own signature -- a plain per-point
    Python callable, which is wrapped in a :class:`CallableTarget` (sampler on the GPU, density evaluated by the
    caller's code between ticks). Anything else is rejected, loudly."""
    if not isinstance(logp_dlogp_func, DeviceTarget):
        if callable(logp_dlogp_func) and model_ndim is not None:
            return CallableTarget(int(model_ndim), logp_dlogp_func)
        raise TypeError(
            "logp_dlogp_func must be a littlemcmc_amd.targets.DeviceTarget (StdNormal, DiagGaussian, AR1, Funnel, "
            "Normal1D, GLM, UserTarget, TorchTarget, Batched) or a callable q[d] -> (logp, dlogp[d]) together with model_ndim; got %r"
            % (logp_dlogp_func,))
    if model_ndim is not None and int(model_ndim) != logp_dlogp_func.d:
        raise ValueError("model_ndim=%s does not match the target's dimension %d" % (model_ndim, logp_dlogp_func.d))
    return logp_dlogp_func
