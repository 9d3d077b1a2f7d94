"""numpy longdouble model of lmc_diag_cross_moments (include/lmc_hip.h) and the tolerance its results are held to.

One call over a block x[chains, draws, d] whose chain 0 is chain ``first_chain`` of the job, ``per`` chains a group, the
sub-series [t0, t0 + n): per touched group the count, the mean row and m2 = sum (x - mean)(x - mean)^T of the group's rows
that lie in the block.

The tolerance is the one tests/test_gpu_pooled.py::test_pooled_statistic_against_numpy derives, with no free factor. With N
rows of a part, shift the part's column mean and a = |x - shift|: the sum S_ij of N products of rounded differences is off
by at most N 2^-52 sum_r a_ri a_rj (2^-53 per factor for x - shift, (N - 1) 2^-53 for the sum in ANY order), the column sums
s_i of the differences by e_i = N 2^-52 sum_r a_ri, hence the correction s_i s_j / N by (|s_i| e_j + |s_j| e_i) / N:

    tol_m2 = N 2^-52 (a^T a) + (|s_i| e_j + |s_j| e_i) / N          tol_mean = e / N + 2^-52 |mean|

Merged parts (``merge_tolerance``). a and b hold (n, mean, m2) with errors within (tm_a, tM_a), (tm_b, tM_b); the rule is
n = na + nb, delta = mb - ma, mean = ma + delta nb / n, m2 = (m2a + m2b) + delta delta^T w, w = na nb / n. With u = 2^-52 (twice
the unit roundoff, which covers the second-order terms), every quantity below taken at its exact value:
  delta_i   is off by at most  ed_i = tm_a,i + tm_b,i + u |delta_i|                              (inputs, one subtraction)
  p_ij = delta_i delta_j w   by  ep_ij = w (|delta_i| ed_j + |delta_j| ed_i + ed_i ed_j) + 3 u |p_ij|   (inputs; w is one
                                                                         division of an exact product, then two products)
  m2_ij     by  tM_a + tM_b + ep_ij + u (|m2a_ij| + |m2b_ij|) + u |m2_ij|                        (inputs, two additions)
  mean_i    by  tm_a,i + (nb / n) ed_i + 2 u |delta_i| nb / n + u |mean_i|        (inputs, a division, a product, an addition)
A side of count 0 is skipped and hands the other side's tolerance on unchanged."""
import numpy as np
import torch

EPS = np.longdouble(2.0) ** -52
LD = np.longdouble


def touched(first_chain, chains, per):
    g0 = first_chain // per
    return g0, (first_chain + chains - 1) // per - g0 + 1


def group_rows(x, first_chain, per, t0=0, n=None):
    """The rows [N_g, d] (longdouble) of every touched group, in group order."""
    x = np.asarray(x)
    c, rows, d = x.shape
    n = rows - t0 if n is None else n
    g0, k = touched(first_chain, c, per)
    out = []
    for g in range(g0, g0 + k):
        lo, hi = max(g * per - first_chain, 0), min((g + 1) * per - first_chain, c)
        out.append(x[lo:hi, t0:t0 + n].reshape(-1, d).astype(LD))
    return out


def part(rows):
    """Exact (longdouble) n, mean, m2 of one part's rows and the tolerance of a device result for it."""
    N = rows.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = rows.mean(axis=0)
        dev = rows - mean
        m2 = dev.T @ dev
        shift = mean.astype(np.float64).astype(LD)        # (to rounding; only the bound uses it)
        a = np.abs(rows - shift)
        s = (rows - shift).sum(axis=0)
        e = N * EPS * a.sum(axis=0)
        tol_m2 = N * EPS * (a.T @ a) + (np.abs(s)[:, None] * e[None, :] + np.abs(s)[None, :] * e[:, None]) / N
        tol_mean = e / N + EPS * np.abs(mean)
    return {"n": LD(N), "mean": mean, "m2": m2, "tol_mean": tol_mean, "tol_m2": tol_m2}


def merge_tolerance(A, B):
    """The exact moments of the union of two parts (``part`` results, or earlier merges) and the tolerance of the merged
    device result, by the derivation in the module docstring."""
    if B["n"] == 0:
        return A
    if A["n"] == 0:
        return B
    na, nb = A["n"], B["n"]
    n = na + nb
    w, f = na * nb / n, nb / n
    delta = B["mean"] - A["mean"]
    ed = A["tol_mean"] + B["tol_mean"] + EPS * np.abs(delta)
    p = np.outer(delta, delta) * w
    ad = np.abs(delta)
    ep = w * (ad[:, None] * ed[None, :] + ad[None, :] * ed[:, None] + ed[:, None] * ed[None, :]) + 3 * EPS * np.abs(p)
    m2 = A["m2"] + B["m2"] + p
    mean = A["mean"] + delta * f
    tol_m2 = A["tol_m2"] + B["tol_m2"] + ep + EPS * (np.abs(A["m2"]) + np.abs(B["m2"])) + EPS * np.abs(m2)
    tol_mean = A["tol_mean"] + f * ed + 2 * EPS * ad * f + EPS * np.abs(mean)
    return {"n": n, "mean": mean, "m2": m2, "tol_mean": tol_mean, "tol_m2": tol_m2}


def zero_part(d):
    z = np.zeros(d, dtype=LD)
    return {"n": LD(0), "mean": z, "m2": np.zeros((d, d), dtype=LD), "tol_mean": z, "tol_m2": np.zeros((d, d), dtype=LD)}


def moments(x, first_chain, per, t0=0, n=None):
    """[touched] list of ``part`` results of one call."""
    return [part(r) for r in group_rows(x, first_chain, per, t0, n)]


def moments_fn(x, first_chain, per):
    """The model as ``diagnostics.cross_moments(..., moments_fn=)``: the exact moments rounded to float64."""
    ps = moments(x.detach().cpu().numpy(), int(first_chain), int(per))
    f = lambda k: torch.from_numpy(np.stack([np.asarray(p[k]).astype(np.float64) for p in ps])).to(x.device)
    return {"n": f("n"), "mean": f("mean"), "m2": f("m2")}


def check(got_n, got_mean, got_m2, parts, label=""):
    """Assert a result [G], [G, d], [G, d, d] (numpy float64) against per-group exact moments and tolerances; returns (and
    prints) the largest error in units of the bound."""
    worst_m2 = worst_mean = 0.0
    ok = True
    assert len(parts) == got_n.shape[0] == got_mean.shape[0] == got_m2.shape[0], label
    for g, p in enumerate(parts):
        assert got_n[g] == float(p["n"]), (label, g)
        err_m2 = np.abs(got_m2[g].astype(LD) - p["m2"])
        err_mean = np.abs(got_mean[g].astype(LD) - p["mean"])
        with np.errstate(invalid="ignore", divide="ignore"):
            r2 = np.where(err_m2 == 0, 0, err_m2 / p["tol_m2"])
            r1 = np.where(err_mean == 0, 0, err_mean / p["tol_mean"])
        worst_m2, worst_mean = max(worst_m2, float(r2.max())), max(worst_mean, float(r1.max()))
        ok = ok and bool((err_m2 <= p["tol_m2"]).all()) and bool((err_mean <= p["tol_mean"]).all())
    print("%s: max |m2 - ref| / bound = %.3g, max |mean - ref| / bound = %.3g" % (label, worst_m2, worst_mean))
    assert ok, (label, worst_m2, worst_mean)
    return worst_m2, worst_mean
