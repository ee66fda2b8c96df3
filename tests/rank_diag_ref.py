"""An independent transcription of the rank-normalised convergence diagnostics of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) as the R
package `posterior` 1.x computes them: z_scale, fold_draws, .rhat, ess_bulk, ess_tail, ess_mean and mcse_mean.  Ranks come from
scipy.stats.rankdata(method="average"), Phi^-1 from scipy.special.ndtri; means and variances are R's (long-double sums, the mean refined by
a second pass: r_mean, r_var) and stay in long double, as do the direct sums of the autocovariances, and the lag window of Geyer's sequence is cut at L lags (the library's max_lag), which changes nothing whenever the sequence ends before L.

Input everywhere: x of shape (m, h), the m = 2 C split chains of h draws of ONE parameter (split_draws makes them from the windows: rows [0, h)
and [nsamp - h, nsamp) of every chain, an odd window dropping its middle row).  Conventions (`posterior`'s should_return_NA): a non-finite draw
or all draws equal gives NaN.  Nothing here is shared with the package under test.
"""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata


def split_draws(windows):
    """(m, h, P) from the C windows (nsamp, P) of the chains, in their order"""
    out = []
    for w in windows:
        nsamp = w.shape[0]
        h = nsamp // 2
        out += [w[:h], w[nsamp - h:]]
    return np.stack(out)


LD = np.longdouble


def r_mean(x, axis=None):
    """R's mean(): a long-double sum, refined by the mean of the residuals.  Kept in long double: rounded to float64, the split-chain means of a
    column like 1e8 + N(0, 1) would lose the eight digits their between-chain variance needs"""
    xl = np.asarray(x, dtype=LD)
    s = xl.mean(axis=axis, keepdims=True)
    s = s + (xl - s).mean(axis=axis, keepdims=True)
    return np.squeeze(s, axis=axis) if axis is not None else s.reshape(())[()]


def r_var(x, axis=None):
    """R's var(): two passes in long double, ddof 1 (kept in long double)"""
    xl = np.asarray(x, dtype=LD)
    mu = r_mean(xl, axis=axis)
    c = xl - (np.expand_dims(mu, axis) if axis is not None else mu)
    n = xl.shape[axis] if axis is not None else xl.size
    return (c * c).sum(axis=axis) / (n - 1)


def should_return_na(x):
    return (not np.all(np.isfinite(x))) or np.all(x == x.flat[0])


def z_scale(x):
    S = x.size
    r = rankdata(x.reshape(-1), method="average").reshape(x.shape)
    return ndtri((r - 3.0 / 8.0) / (S - 2.0 * 3.0 / 8.0 + 1.0))


def fold_draws(x):
    return np.abs(x - np.median(x))


def rhat_basic(x):
    """posterior:::.rhat on the (split) chains x (m, h)"""
    n = x.shape[1]
    chain_mean = r_mean(x, axis=1)
    chain_var = r_var(x, axis=1)
    var_between = n * r_var(chain_mean)
    var_within = r_mean(chain_var)
    with np.errstate(all="ignore"):
        return np.float64(np.sqrt((var_between / var_within + n - 1) / n))


def autocovariance(y, L):
    """lags 0 .. L-1 of one chain, 1 / n normalisation"""
    n = y.size
    c = np.asarray(y, dtype=LD) - r_mean(y)
    return np.array([np.dot(c[:n - t], c[t:]) / n for t in range(L)], dtype=LD)


def ess_basic(x, L):
    """posterior:::.ess on the (split) chains x (m, h), Geyer's initial positive and monotone sequence over the lags below L"""
    if should_return_na(x):
        return np.nan
    m, n = x.shape
    acov = np.stack([autocovariance(x[j], L) for j in range(m)], axis=1)          # (L, m)
    chain_mean = r_mean(x, axis=1)
    mean_var = acov[0].mean() * n / (n - 1)
    var_plus = mean_var * (n - 1) / n
    if m > 1:
        var_plus = var_plus + r_var(chain_mean)
    with np.errstate(all="ignore"):
        rho = 1.0 - (mean_var - acov.mean(axis=1)) / var_plus
    rho[0] = 1.0
    if np.isnan(rho).any():
        return np.nan
    pairs = []
    t = 0
    while t + 1 < L and rho[t] + rho[t + 1] > 0:
        pairs.append([rho[t], rho[t + 1]])
        t += 2
    max_t = t
    last = rho[max_t] if max_t < L and rho[max_t] > 0 else 0.0
    for k in range(1, len(pairs)):                                                # the monotone sequence
        if pairs[k][0] + pairs[k][1] > pairs[k - 1][0] + pairs[k - 1][1]:
            pairs[k][0] = pairs[k][1] = (pairs[k - 1][0] + pairs[k - 1][1]) / 2
    ess = m * n
    tau = -1.0 + 2.0 * sum(a + b for a, b in pairs) + last
    tau = max(tau, 1.0 / np.log10(ess))
    return np.float64(ess / tau)


def diagnostics(x, L):
    """dict of the seven figures for one parameter, x (m, h)"""
    nan = float("nan")
    out = dict(rhat_bulk=nan, rhat_tail=nan, rhat=nan, ess_bulk=nan, ess_tail=nan, ess_mean=nan, mcse_mean=nan)
    if should_return_na(x):
        return out
    out["rhat_bulk"] = rhat_basic(z_scale(x))
    f = fold_draws(x)
    if not should_return_na(f):
        out["rhat_tail"] = rhat_basic(z_scale(f))
    out["rhat"] = np.fmax(out["rhat_bulk"], out["rhat_tail"])      # (the package's one deviation from `posterior`, which takes max)
    out["ess_bulk"] = ess_basic(z_scale(x), L)
    e = [ess_basic((x <= np.quantile(x, p)).astype(np.float64), L) for p in (0.05, 0.95)]
    out["ess_tail"] = nan if np.isnan(e).any() else min(e)
    out["ess_mean"] = ess_basic(x, L)
    with np.errstate(all="ignore"):
        out["mcse_mean"] = np.float64(np.sqrt(r_var(x)) / np.sqrt(out["ess_mean"]))
    return out


FIELDS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")


def diagnostics_all(windows, L):
    """dict of arrays (P,) over every parameter column of the windows"""
    X = split_draws(windows)
    cols = [diagnostics(X[:, :, p], L) for p in range(X.shape[2])]
    return {k: np.array([c[k] for c in cols]) for k in FIELDS}
