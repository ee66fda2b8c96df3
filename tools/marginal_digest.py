"""SHA-256 of what the marginal libraries (libbnr_mloo.so, libbnr_medge.so, libbnr_mpred.so) return on fixed inputs: marginal_loglik_raw,
marginal_gamma_raw, marginal_predict_raw, mixture_summary_raw and mixture_score_raw on seeded arrays at the tile edges (n, q, m around 32, 64 and
128; 1, 9 and 13 draws; with and without W; the batch option 0 and 5, mpred_block_rows 0 and 32), and the three chain calls on a 2-chain fit.
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
        for name in ("mloo", "medge", "mpred"):
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
    for name in ("mloo", "medge", "mpred"):
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
    chain_cases()


if __name__ == "__main__":
    main()
