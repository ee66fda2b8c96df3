"""SHA-256 of what the posterior-analysis entry points return on a few fixed inputs (the PSIS, rank, HDI, inclusion and weighted-quantile matrix
calls on crafted and seeded rows; summary, predict in every input format, loglik_stats, loo, loo_predict, rank_diag, hdi, inclusion, ess_stats,
rhat_stats and the split-Rhat over the chains on a 3-chain group and on a lone chain, the chain stacking and the summaries under its weights on the group, with the default block sizes and
with small ones):
run it with two builds of the library (BNR_HIP_LIB) and diff the output to see whether a change to that layer is bitwise neutral.  The companion of
table_digest.py, which does the same for the sampled tables."""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, bnr_amd
from bnr_amd import _capi

DEV = 0
SEED, PS = 4717, 0xC0FFEE12345
NB, NS = 100, 300


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())          # (float64 throughout, but for the counts and sets of inclusion)
    return h.hexdigest()[:16]


def show(label, arrays):
    print("%s: %s" % (label, digest(arrays)), flush=True)


def crafted_rows(S, rng):
    """the rows of the LOO tests: a chi-square-like row, a constant one, one with many ties (at the cutoff too), three with a GPD tail"""
    rows = [-0.5 * rng.standard_normal(S) ** 2 - 0.9189385332046727, np.full(S, -2.0), np.round(rng.standard_normal(S), 1)]
    for k in (0.3, 0.7, 1.2):
        u = rng.random(S)
        rows.append(-np.log(((1 - u) ** (-k) - 1) / k + 1e-300))
    return np.array(rows)


def psis_case(label, ll, r_eff=None):
    show("psis_loo %s" % label, _capi.psis_loo_raw(ll, r_eff, DEV))
    show("psis_weights %s" % label, _capi.psis_weights_raw(ll, r_eff, DEV))


def matrix_cases():
    for S in (1, 7, 20, 21, 24, 25, 400):                      # M < 5 on both sides of its boundary, the constant row, a smoothed fit
        psis_case("crafted S=%d" % S, crafted_rows(S, np.random.default_rng(S)))
    # 17 large ratios, 30 tied at the cutoff, M = 20: three tied draws join the tail (k_psis_w's draw-index select); a NaN row; a rounded row
    rng = np.random.default_rng(6)
    S = 100
    ll = rng.standard_normal(S) + 3.0
    big = rng.choice(S, 17, replace=False)
    ll[big] = -5.0 - np.arange(17) * 0.1
    tied = np.sort(rng.choice(np.setdiff1d(np.arange(S), big), 30, replace=False))
    ll[tied] = -1.0
    bad = rng.standard_normal(S)
    bad[12] = np.nan
    psis_case("ties, NaN row, rounded row", np.array([ll, bad, np.round(rng.standard_normal(S), 1)]))
    S = 50000                                                   # the longest tail: M = P = 8192
    ll = np.array([-0.5 * rng.standard_normal(S) ** 2, -np.log(((1 - rng.random(S)) ** -0.6 - 1) / 0.6)])
    psis_case("S=50000 M=8192", ll, S * 9.0 / 8192.0 ** 2 * 1.0001)


def seeded_matrix_cases():
    """the rank, HDI, inclusion and weighted-quantile calls on a caller's matrix: a few seeded rows each, ties and a NaN row among them"""
    rng = np.random.default_rng(SEED + 5)
    for S in (2, 7, 256, 1000):
        x = np.array([rng.standard_normal(S), np.round(rng.standard_normal(S), 1), np.full(S, 1.5), np.abs(rng.standard_normal(S)) - 0.2,
                      np.where(np.arange(S) == S // 2, np.nan, rng.standard_normal(S))])
        show("rank_normalize S=%d" % S, _capi.rank_normalize_raw(x, DEV))
        show("hdi S=%d" % S, _capi.hdi_raw(x, (0.5, 0.95), DEV))
        show("hdi S=%d, no level" % S, _capi.hdi_raw(x, (), DEV, fields=("median", "p_pos", "p_neg")))
    for S, B in ((3, 2), (77, 5), (1000, 70)):
        z = rng.random((S, B)) < np.linspace(0.1, 0.9, B)[None, :]
        show("inclusion S=%d B=%d" % (S, B), _capi.inclusion_raw(z, 4, DEV))
        show("inclusion S=%d B=%d, marginals" % (S, B), _capi.inclusion_raw(z, 0, DEV, fields=("prob", "size_pmf")))
    for K, ns in ((1, 9), (3, 50), (4, 333)):
        x = np.array([rng.standard_normal(K * ns), np.round(rng.standard_normal(K * ns), 1), np.full(K * ns, -2.0)])
        w = rng.random(K)
        w[K // 2] = 0.0 if K > 1 else 1.0
        w /= w.sum()
        show("wquantile K=%d nsamp=%d" % (K, ns), _capi.wquantile_raw(x, w, K, 3, K * ns - 2, DEV))
        show("wquantile K=%d nsamp=%d, mean" % (K, ns), _capi.wquantile_raw(x, w, K, 1, 1, DEV, fields=("mean",)))


def chain_cases(label, chains, Xn, yn):
    """every analysis call on `chains`: the pooled entry points for a list of chains, the single-chain ones for a lone chain"""
    lone = chains[0] if len(chains) == 1 else None
    S = len(chains) * NS
    k_lo, k_hi = 23, S - 22
    Xb = np.random.default_rng(SEED + 2).random(Xn.shape) < 0.5
    V = chains[0].V
    formats = [("f64", Xn, False), ("binary f64", Xb.astype(np.float64), False), ("u8", Xb.astype(np.uint8), False), ("i32", Xb.astype(np.int32), False),
               ("matrices", [bnr_amd.create_lower_tri(Xn[i], V) for i in range(Xn.shape[0])], True)]
    if lone:
        show("%s summary" % label, lone.summary(NB + 1, NS, k_lo, k_hi))
        for name, X, xt in formats:
            show("%s predict %s" % (label, name), lone.predict(X, NB + 1, NS, k_lo, k_hi, y=yn, x_transform=xt))
        show("%s loglik_stats" % label, lone.loglik_stats(NB + 1, NS))
        show("%s loo" % label, lone.loo(NB + 1, NS, 0.7))
        show("%s loo_predict" % label, lone.loo_predict(NB + 1, NS, 0.7))
        show("%s rank_diag" % label, lone.rank_diag(NB + 1, NS, 40))
        show("%s hdi" % label, lone.hdi(NB + 1, NS, (0.5, 0.95)))
        for which in (0, 1):
            show("%s inclusion %d" % (label, which), lone.inclusion(NB + 1, NS, which, 5))
    else:
        show("%s summary" % label, _capi.pooled_summary(chains, NB + 1, NS, k_lo, k_hi))
    # (the pooled entry points also for the lone chain: its predictive bounds and PITs)
    for name, X, xt in formats:
        show("%s pooled predict %s" % (label, name), _capi.pooled_predict(chains, X, NB + 1, NS, k_lo, k_hi, y=yn, x_transform=xt, pred_seed=PS, pit=True))
    show("%s pooled loglik_stats" % label, _capi.pooled_loglik_stats(chains, NB + 1, NS, pit=True))
    show("%s pooled loo" % label, _capi.pooled_loo(chains, NB + 1, NS, 0.7))
    show("%s pooled loo_predict" % label, _capi.pooled_loo_predict(chains, NB + 1, NS, 0.7))
    show("%s pooled rank_diag" % label, _capi.pooled_rank_diag(chains, NB + 1, NS, 40))
    show("%s pooled rank_diag, two fields" % label, _capi.pooled_rank_diag(chains, NB + 1, NS, 40, ("rhat_tail", "mcse_mean")))
    show("%s pooled hdi" % label, _capi.pooled_hdi(chains, NB + 1, NS, (0.5, 0.95)))
    for which in (0, 1):
        show("%s pooled inclusion %d" % (label, which), _capi.pooled_inclusion(chains, NB + 1, NS, which, 5))
    if not lone:                                                # the chain stacking, and the summaries under its weights and under given ones
        st = _capi.chains_stack(chains, NB + 1, NS, 0.7)
        show("%s chains_stack" % label, st)
        for wl, w in (("stack", st[0]), ("given", np.array([0.5, 0.0, 0.5]))):
            show("%s stacked_summary %s" % (label, wl), _capi.stacked_summary(chains, w, NB + 1, NS, k_lo, k_hi))
            for name, X, xt in formats[:4]:
                show("%s stacked_predict %s %s" % (label, wl, name), _capi.stacked_predict(chains, w, X, NB + 1, NS, k_lo, k_hi, y=yn, pred_seed=PS))
    for k, ch in enumerate(chains):
        show("%s ess_stats chain %d" % (label, k + 1), [ch.ess_stats(NB + 1, NS, 20)])
        show("%s rhat_stats chain %d" % (label, k + 1), [ch.rhat_stats(NB + 1, NS)])
    show("%s rhat" % label, _capi.rhat(chains, len(chains), None, NB, NS))


def main():
    matrix_cases()
    seeded_matrix_cases()
    X, y, _ = bnr_amd.make_synthetic(60, 12, 3, seed=SEED)                         # the trio of the pooled tests and a lone chain
    trio = [bnr_amd.Chain(X, y, 3, 400, SEED, 1, device=DEV)]
    trio += [bnr_amd.Chain.like(trio[0], SEED, c) for c in (2, 3)]
    grp = bnr_amd.Group(trio)
    lone = bnr_amd.Chain(X, y, 3, 400, SEED + 9, 1, device=DEV)
    for ch in trio + [lone]:
        ch.init_prior()
    grp.run(2, 400, 400)
    lone.run(2, 400, 400)
    Xn, yn, _ = bnr_amd.make_synthetic(37, 12, 3, seed=SEED + 1)
    for rows, cols, rcols in ((0, 0, 0), (32, 7, 5)):
        for ch in (trio[0], lone):
            ch.set_option("predict_block_rows", rows)
            ch.set_option("summary_block_cols", cols)
            ch.set_option("rank_block_cols", rcols)
        tag = "blocks %d/%d/%d" % (rows, cols, rcols)
        chain_cases("trio %s" % tag, trio, Xn, yn)
        chain_cases("lone %s" % tag, [lone], Xn, yn)
    grp.close()
    for ch in trio + [lone]:
        ch.close()


if __name__ == "__main__":
    main()
