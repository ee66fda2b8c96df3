"""SHA-256 of what the six marginal libraries return on fixed inputs: marginal_loglik_raw, marginal_gamma_raw, marginal_predict_raw,
mixture_summary_raw and mixture_score_raw on seeded arrays at the tile edges (n, q, m around 32, 64 and 128; 1, 9 and 13 draws; with and without
W; the batch option 0 and 5, mpred_block_rows 0 and 32); weighted_mixture_raw and stacked_mixture_raw (1 and 33 rows, 1 and 257 components per
row, with and without y and the bounds; K = 3 with one weight 0, the compaction of the stacked mixture); marginal_gamma_cov_raw (all columns and
three of them, with and without weights); and the six chain calls on a 2-chain fit.
One line per output of a call and setting, over all its shapes in a fixed order (--verbose: one line per shape as well).  Run it in two checkouts
and diff the output to see whether a change to that layer is bitwise neutral.  The companion of post_digest.py."""
import sys, os, hashlib, argparse, itertools
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, bnr_amd
from bnr_amd import _capi

NS, QS, MS, DS = (1, 31, 32, 33, 65), (1, 31, 33, 70), (1, 33, 129), (1, 9, 13)
VERBOSE = False


class Digests:
    """one running sha256 per named output of a call"""

    def __init__(self, label, names):
        self.label, self.names, self.h = label, names, [hashlib.sha256() for _ in names]

    def add(self, shape, outs):
        for name, h, a in zip(self.names, self.h, outs):
            b = b"-" if a is None else np.ascontiguousarray(a).tobytes()
            h.update(b)
            if VERBOSE:
                print("  %s %s %s: %s" % (self.label, shape, name, hashlib.sha256(b).hexdigest()[:16]), flush=True)

    def show(self):
        for name, h in zip(self.names, self.h):
            print("%s %s: %s" % (self.label, name, h.hexdigest()), flush=True)


def phi(n, q, D, rng):
    X = rng.standard_normal((n, q))
    y = rng.standard_normal(n)
    return X, y, 0.5 + rng.random(D), rng.standard_normal(D), rng.random((D, q)) * 2.0, rng.standard_normal((D, q)) * 0.3


def raw_cases():
    for use_w, batch in itertools.product((True, False), (0, 5)):
        tag = "W=%d batch=%d" % (use_w, batch)
        for name in ("mloo", "medge", "mpred"):
            getattr(_capi, name + "_set_option")(name + "_batch_draws", batch)
        ll, ga = Digests("marginal_loglik_raw " + tag, ("loglik", "resid", "var", "logml", "n_bad")), Digests("marginal_gamma_raw " + tag, ("m", "v", "n_bad"))
        pr = {blk: Digests("marginal_predict_raw %s block=%d" % (tag, blk), ("mean", "var", "n_bad")) for blk in (0, 32)}
        for n, q, D in itertools.product(NS, QS, DS):
            rng = np.random.default_rng(1000003 * n + 1009 * q + D)
            X, y, t2, mu, S, W = phi(n, q, D, rng)
            W = W if use_w else None
            shape = "n=%d q=%d D=%d" % (n, q, D)
            ll.add(shape, _capi.marginal_loglik_raw(X, y, t2, mu, S, W))
            ga.add(shape, _capi.marginal_gamma_raw(X, y, t2, mu, S, W))
            for m in MS:
                Xn = rng.standard_normal((m, q))
                for blk in (0, 32):
                    _capi.mpred_set_option("mpred_block_rows", blk)
                    pr[blk].add(shape + " m=%d" % m, _capi.marginal_predict_raw(X, y, Xn, t2, mu, S, W))
        for d in (ll, ga, pr[0], pr[32]):
            d.show()
    for name in ("mloo", "medge", "mpred"):
        getattr(_capi, name + "_set_option")(name + "_batch_draws", 0)
    _capi.mpred_set_option("mpred_block_rows", 0)


def mixture_cases():
    for weighted in (False, True):
        su = Digests("mixture_summary_raw weights=%d" % weighted, _capi.MEDGE_SUMMARY_FIELDS)
        sc = Digests("mixture_score_raw weights=%d" % weighted, ("lpd", "pit"))
        for K, nd, q in itertools.product((1, 2, 3), DS, QS):
            rng = np.random.default_rng(7919 * K + 101 * nd + q)
            m, v, y = rng.standard_normal((K * nd, q)), rng.random((K * nd, q)) + 0.1, rng.standard_normal(q)
            w = None
            if weighted:
                w = rng.random(K) + 0.1
                w /= w.sum()
            shape = "K=%d nd=%d q=%d" % (K, nd, q)
            su.add(shape, _capi.mixture_summary_raw(m, v, K, w))
            sc.add(shape, _capi.mixture_score_raw(m, v + 0.5, y, K, w))
        su.show()
        sc.show()


def log_weights(rng, rows, K, nd):
    """rows x (K nd) log weights that sum to 1 within every chain's nd columns"""
    w = rng.random((rows, K, nd)) + 0.05
    return np.log(w / w.sum(axis=2, keepdims=True)).reshape(rows, K * nd)


def weighted_cases():
    """libbnr_mcheck.so and libbnr_mstack.so: the raw mixtures, with and without y (pit) and the bounds (the bracket and the quantile launches)"""
    for has_y, bounds in itertools.product((True, False), (True, False)):
        fields = ("mean", "sd") + (("pit",) if has_y else ()) + (("lower", "upper") if bounds else ())
        tag = "y=%d bounds=%d" % (has_y, bounds)
        wm, sm = Digests("weighted_mixture_raw " + tag, _capi.MCHECK_FIELDS), Digests("stacked_mixture_raw " + tag, _capi.MCHECK_FIELDS)
        for rows, D in itertools.product((1, 33), (1, 257)):
            rng = np.random.default_rng(4099 * rows + D)
            mean, var, y = rng.standard_normal((rows, D)), rng.random((rows, D)) + 0.1, rng.standard_normal(rows) if has_y else None
            shape = "rows=%d D=%d" % (rows, D)
            wm.add(shape, _capi.weighted_mixture_raw(mean, var, log_weights(rng, rows, 1, D), y, 0.05, 0.9, fields=fields))
            sm.add(shape + " K=1", _capi.stacked_mixture_raw(mean, var, log_weights(rng, rows, 1, D), [1.0], 1, y, 0.05, 0.9, fields=fields))
        for rows, nd, w in itertools.product((1, 33), (1, 86), ((0.5, 0.25, 0.25), (0.625, 0.0, 0.375))):       # one weight 0: Kp < K
            rng = np.random.default_rng(4099 * rows + 3 * nd + 7)
            mean, var, y = rng.standard_normal((rows, 3 * nd)), rng.random((rows, 3 * nd)) + 0.1, rng.standard_normal(rows) if has_y else None
            sm.add("rows=%d nd=%d K=3 w=%r" % (rows, nd, w), _capi.stacked_mixture_raw(mean, var, log_weights(rng, rows, 3, nd), w, 3, y, 0.05, 0.9,
                                                                                           fields=fields))
        wm.show()
        sm.show()


def cov_cases():
    """libbnr_mcov.so: the raw covariance of two chains' draws, all columns and a subset, pooled and weighted, the batch option 0 and 5"""
    for batch, subset, weighted in itertools.product((0, 5), (False, True), (False, True)):
        _capi.mcov_set_option("mcov_batch_draws", batch)
        cv = Digests("marginal_gamma_cov_raw batch=%d cols=%d weights=%d" % (batch, subset, weighted), ("mean", "cov", "within", "m", "v", "n_bad"))
        for n, q, nd in itertools.product((31, 33), (3, 33, 70), (1, 9)):
            rng = np.random.default_rng(1000003 * n + 1009 * q + nd)
            X, y, t2, mu, S, W = phi(n, q, 2 * nd, rng)
            cv.add("n=%d q=%d nd=%d" % (n, q, nd), _capi.marginal_gamma_cov_raw(X, y, t2, mu, S, W, cols=(q - 1, 0, q // 2) if subset else None, nchains=2,
                                                                                   weights=(0.25, 0.75) if weighted else None))
        cv.show()
    _capi.mcov_set_option("mcov_batch_draws", 0)


LIBS = ("mloo", "medge", "mpred", "mcheck", "mstack", "mcov")


def chain_cases():
    X, y, _ = bnr_amd.make_synthetic(20, 6, 2, seed=7)
    tot = 60
    chains = [bnr_amd.Chain(X, y, 2, tot, 11, 1)]
    chains.append(bnr_amd.Chain.like(chains[0], 11, 2, tot))
    for ch in chains:
        ch.init_prior()
        ch.run(2, tot, tot)
    rng = np.random.default_rng(8)
    Xn, yn = rng.standard_normal((7, chains[0].q)), rng.standard_normal(7)
    for thin, batch in itertools.product((1, 3), (0, 5)):
        tag = "thin=%d batch=%d" % (thin, batch)
        for name in LIBS:
            getattr(_capi, name + "_set_option")(name + "_batch_draws", batch)
        lo = Digests("chains_marginal_loo " + tag, ("elpd_loo", "pareto_k", "loo_mean", "loo_sd", "logml", "loglik", "n_bad"))
        lo.add("", _capi.chains_marginal_loo(chains, 11, 40, thin, loglik=True))
        lo.show()
        out, m, v, nb = _capi.chains_marginal_edges(chains, 11, 40, thin, per_draw=True)
        ed = Digests("chains_marginal_edges " + tag, _capi.MEDGE_SUMMARY_FIELDS + ("m", "v", "n_bad"))
        ed.add("", out + (m, v, nb))
        ed.show()
        out, m, v, nb = _capi.chains_marginal_predict(chains, 11, 40, Xn, yn, thin, per_draw=True)
        pr = Digests("chains_marginal_predict " + tag, _capi.MPRED_SUMMARY_FIELDS + ("dmean", "dvar", "n_bad"))
        pr.add("", out + (m, v, nb))
        pr.show()
        el, kh, out, ml, ll, nb = _capi.chains_marginal_loo_predict(chains, 11, 40, thin, loglik=True)
        lp = Digests("chains_marginal_loo_predict " + tag, ("elpd_loo", "pareto_k") + _capi.MCHECK_FIELDS + ("logml", "loglik", "n_bad"))
        lp.add("", (el, kh) + out + (ml, ll, nb))
        lp.show()
        for fixed in (None, (1.0, 0.0)):
            w, el, kh, es, gap, it, out, ml, nb = _capi.chains_marginal_stack(chains, 11, 40, thin, weights=fixed)
            st = Digests("chains_marginal_stack %s fixed=%d" % (tag, fixed is not None),
                         ("weights", "elpd_chain", "pareto_k_chain", "elpd_stack", "gap", "iterations") + _capi.MCHECK_FIELDS + ("logml", "n_bad"))
            st.add("", (w, el, kh, es, gap, it) + out + (ml, nb))
            st.show()
        for cols, weights in itertools.product((None, (5, 0, 2)), (None, (0.25, 0.75))):
            ec = Digests("chains_marginal_edge_cov %s cols=%d weights=%d" % (tag, cols is not None, weights is not None),
                         ("mean", "cov", "within", "m", "v", "n_bad"))
            ec.add("", _capi.chains_marginal_edge_cov(chains, 11, 40, thin, cols=cols, weights=weights, per_draw=True))
            ec.show()
    for name in LIBS:
        getattr(_capi, name + "_set_option")(name + "_batch_draws", 0)
    for ch in chains:
        ch.close()


def main():
    global VERBOSE
    ap = argparse.ArgumentParser()
    ap.add_argument("--verbose", action="store_true", help="one line per shape as well")
    VERBOSE = ap.parse_args().verbose
    raw_cases()
    mixture_cases()
    weighted_cases()
    cov_cases()
    chain_cases()


if __name__ == "__main__":
    main()
