// bnr_analysis.hip -- the posterior analysis behind the C ABI (include/bnr_hip.h) over the kernels in bnr_analysis_kernels.h: Summary, rank-normalised
// diagnostics, highest-density intervals, posterior prediction, log-likelihood statistics, PSIS-LOO and its predictive checks.  A translation unit and
// so a gfx950 code object of its own: nothing added here can move a kernel of the sweep (bnr_hip.hip), whose speed depends on where its kernels lie.
// k_fetch_cols, k_summary, k_acov and k_wsummary (k_summary's companion of ABI 16) stay with the sweep kernels and are launched through bnr_internal.h.
#include "bnr_internal.h"
#include "bnr_analysis_kernels.h"

#include <cmath>

// a stream of a call's own (the calls on a caller's matrix), destroyed on every path.  open: the device checked against the device count and made
// current, then the stream on it
namespace {
struct stream_guard {
    hipStream_t s = nullptr;
    ~stream_guard() { if (s) (void)hipStreamDestroy(s); }
    int open(int device)
    {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return fail(BNR_ERR_BAD_ARG, "no such device");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return BNR_OK;
    }
};
}
// Rows of a caller's matrix per block: about `budget` bytes of rows of `len` doubles, between 1 and m
static int block_rows(size_t budget, long long len, int m)
{
    return (int)std::min<size_t>((size_t)m, std::max<size_t>(1, budget / ((size_t)len * sizeof(double))));
}
// Parameter columns per staging block: about 1 GiB of columns of S draws, or the chain's override (`set` > 0), between 1 and np
static int block_cols(long long S, int set, int np)
{
    const long long blk = set > 0 ? set : (long long)(((size_t)1 << 30) / ((size_t)S * sizeof(double)));
    return (int)std::min<long long>(std::max<long long>(blk, 1), np);
}

// The chains of an analysis call (the single-chain entry points pass theirs as a list of one): one device, equal n, V, R, none listed twice,
// none with a pending asynchronous run, the row window inside every table, the pooled draw count within int32
static int pooled_check(bnr_chain *const *cs, int nc, int first_row, int nsamp)
{
    if (!cs) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (nc < 1) return fail(BNR_ERR_BAD_ARG, "need nchains >= 1");
    for (int i = 0; i < nc; ++i) {
        if (!cs[i]) return fail(BNR_ERR_BAD_ARG, "NULL chain");
        for (int k = 0; k < i; ++k) if (cs[k] == cs[i]) return fail(BNR_ERR_BAD_ARG, "chain listed twice");
        const bnr_dev &a = cs[0]->d, &b = cs[i]->d;
        if (cs[i]->device != cs[0]->device || a.n != b.n || a.V != b.V || a.R != b.R)
            return fail(BNR_ERR_BAD_ARG, "pooled chains must live on one device and have equal n, V, R");
    }
    for (int i = 0; i < nc; ++i) if (cs[i]->pending) return fail(BNR_ERR_BAD_ARG, "an asynchronous run is pending");
    for (int i = 0; i < nc; ++i)
        if (first_row < 1 || nsamp < 1 || first_row + nsamp - 1 > cs[i]->d.tot) return fail(BNR_ERR_BAD_ARG, "row window outside the table");
    if ((long long)nc * nsamp > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    return BNR_OK;
}
// The pooled work runs on the first chain's stream and reads the other chains' tables: whatever their own streams (and their group's) still
// hold -- a table load, the tail of a synchronous run -- is waited for here.  (One chain: nothing to order, as before.)
static int pooled_quiesce(bnr_chain *const *cs, int nc)
{
    for (int i = 1; i < nc; ++i) {
        HIPCHK(hipStreamSynchronize(cs[i]->x.stream));
        if (cs[i]->group) HIPCHK(hipStreamSynchronize(cs[i]->group->x.stream));
    }
    return BNR_OK;
}

// Parameter columns p0 .. p0 + pc - 1 of [gamma(q) | xi(V)] over the pooled window, staged by k_fetch_cols: column p of `buf` holds S = nc nsamp
// draws, chain k's window in rows k nsamp .. (k + 1) nsamp - 1 (one launch per chain and per kind of column)
static void stage_cols(hipStream_t st, bnr_chain *const *cs, int nc, int first_row, int nsamp, int p0, int pc, double *buf)
{
    const bnr_dev &d = cs[0]->d;
    const long long S = (long long)nc * nsamp;
    const int g0 = std::min(p0, d.q), g1 = std::min(p0 + pc, d.q);          // gamma columns g0 .. g1 - 1 first, then xi columns x0 .. x1 - 1
    const int x0 = std::max(p0, d.q) - d.q, x1 = std::max(p0 + pc, d.q) - d.q;
    for (int k = 0; k < nc; ++k) {
        const bnr_dev &dk = cs[k]->d;
        double *dst = buf + (size_t)k * nsamp;
        if (g1 > g0)
            launch_fetch_cols(st, dk.trace, dk.rowlen, dk.o_gamma + g0, g1 - g0, first_row - 1, nsamp, dst, S);
        if (x1 > x0)
            launch_fetch_cols(st, dk.trace, dk.rowlen, dk.o_xi + x0, x1 - x0, first_row - 1, nsamp, dst + (size_t)(g1 - g0) * (size_t)S, S);
    }
}

// Summary(results) on the device (gibbs.jl:1214-1250): posterior mean and two order statistics of every gamma_e over rows
// first_row .. first_row+nsamp-1 of every chain listed (pooled: S = nc nsamp draws, draw c nsamp + s = chain c's s-th window row), and the mean
// of every xi_v.  3q + V doubles cross PCIe instead of the gamma traces.  The q + V parameter columns are staged (k_fetch_cols, one launch per
// chain into its nsamp rows of the S-row column) in blocks of columns that keep the staging buffer near 1 GiB ("summary_block_cols" overrides);
// k_summary works on one column per workgroup, so the block size cannot change a result.  With wt (chain stacking, ABI 16: bnr_chains_wsummary)
// the same staging blocks, k_wsummary under these chain weights instead of k_summary.
static int summary_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi, const bnr_wsum_weights *wt,
                        double *mean_gamma, double *lower, double *upper, double *prob_xi)
{
    bnr_chain *c = cs[0];
    const bnr_dev &d = c->d;
    const long long S = (long long)nc * nsamp;
    if (k_lo < 1 || k_lo > S || k_hi < 1 || k_hi > S)
        return fail(BNR_ERR_BAD_ARG, nc == 1 && !wt ? "order statistics must be between 1 and nsamp" : "order statistics must be between 1 and nchains * nsamp");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->x.stream;
    int rc;
    if ((rc = pooled_quiesce(cs, nc))) return rc;
    const int np = d.q + d.V, blk = block_cols(S, c->summary_block_cols, np);
    dev_tmp tmp;
    double *buf = nullptr;
    result_slab out;                                    // the mean, the lower and the upper statistic of the np = q + V parameters, gamma first
    if ((rc = tmp.alloc(&buf, (size_t)blk * (size_t)S, st, false))) return rc;
    if ((rc = out.alloc(tmp, 3, (size_t)np, st))) return rc;
    for (int p0 = 0; p0 < np; p0 += blk) {
        const int pc = std::min(blk, np - p0), gc = std::min(p0 + pc, d.q) - std::min(p0, d.q);
        stage_cols(st, cs, nc, first_row, nsamp, p0, pc, buf);
        if (wt) launch_wsummary(st, pc, buf, S, nsamp, nc, *wt, gc, k_lo, k_hi, out.col(0) + p0, out.col(1) + p0, out.col(2) + p0);
        else launch_summary(st, pc, buf, (int)S, gc, k_lo, k_hi, out.col(0) + p0, out.col(1) + p0, out.col(2) + p0);
    }
    std::vector<double> host(3 * (size_t)np);           // (the callers' arrays hold q and V entries, not q + V)
    if ((rc = out.fetch(st, wt ? "wsummary" : "summary", wt ? "k_wsummary" : "k_summary", {host.data(), host.data() + np, host.data() + 2 * (size_t)np})))
        return rc;
    memcpy(mean_gamma, host.data(), sizeof(double) * d.q);
    memcpy(prob_xi, host.data() + d.q, sizeof(double) * d.V);
    memcpy(lower, host.data() + np, sizeof(double) * d.q);
    memcpy(upper, host.data() + 2 * (size_t)np, sizeof(double) * d.q);
    return BNR_OK;
}
// (here and below a single-chain entry point is its pooled twin on a list of one: of pooled_check's conditions only the pending run and the row
// window can fail there, and the order-statistic message names nsamp)
int bnr_chain_summary(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                      double *mean_gamma, double *lower, double *upper, double *prob_xi)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_summary(&c, 1, first_row, nsamp, k_lo, k_hi, mean_gamma, lower, upper, prob_xi);
}
int bnr_chains_summary(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                       double *mean_gamma, double *lower, double *upper, double *prob_xi)
{
    if (!chains || !mean_gamma || !lower || !upper || !prob_xi) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return summary_call(chains, nchains, first_row, nsamp, k_lo, k_hi, nullptr, mean_gamma, lower, upper, prob_xi);
}

// the rank-normalised diagnostics (ABI 12): k_rank's two (key, index) buffers, one slice of ld entries per column
struct rank_bufs { unsigned long long *keyA = nullptr, *keyB = nullptr; unsigned int *idxA = nullptr, *idxB = nullptr; };
static void launch_rank(hipStream_t st, int cols, const double *buf, long long ld, int nsamp, int nch, int all, const rank_bufs &rb, int k05, int k95,
                        double *ranks, double *z, double *ind05, double *ind95, double *med, int *flag)
{
    hipLaunchKernelGGL(k_rank, dim3(cols), dim3(256), 0, st, buf, ld, nsamp, nch, all, rb.keyA, rb.keyB, rb.idxA, rb.idxB, k05, k95, ranks, z,
                       ind05, ind95, med, flag);
}
static void launch_fold(hipStream_t st, int cols, const double *buf, long long ld, const double *med, int absolute, double *out)
{
    const int chunks = (int)((ld + 255) / 256);
    hipLaunchKernelGGL(k_fold, dim3((unsigned)chunks * (unsigned)cols), dim3(256), 0, st, buf, ld, chunks, med, absolute, out);
}
// Rank-normalised convergence diagnostics (ABI 12; Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021, as `posterior` 1.x computes them) of every
// parameter p in [gamma(q) | xi(V)] over the pooled window of the chains listed.  The columns are staged as in summary_call ("rank_block_cols"
// overrides the block of about 1 GiB of draws); per block: k_rank on the split-chain draws (z, the two tail indicators, the median, the flag),
// k_acov -- unchanged: a pooled column is nc windows of nsamp side by side, i.e. pc nc columns of nsamp -- on z, the indicators and x - med
// (k_fold: the moments of x are taken about the median), k_fold and a second k_rank and k_acov for the folded z.  Each series' message of the block (2 (2 + L) pc nc doubles; L = 1 where only R-hat is
// wanted) is fetched and finished here: bnr_ess_from_stats as it stands, and split-R-hat = sqrt(((h-1)/h W + B) / W).  Work nobody asked for
// is not run.  Conventions: a parameter with a non-finite draw, or with all draws equal, is NaN in every output; rhat_tail is NaN where the
// folded draws are all equal; ess_tail is NaN where either indicator's ESS is.
namespace {
struct split_msg {                                       // k_acov's message of one series of a block, per chain in bnr_ess_from_stats' layout
    std::vector<double> raw, st, ess;
    int nc = 0, pc = 0, L = 0, h = 0;
    double mean(int c, int half, int p) const { return st[((size_t)c * 2 + half) * (size_t)(2 + L) * pc + p]; }
    double var(int c, int half, int p) const { return st[((size_t)c * 2 + half) * (size_t)(2 + L) * pc + pc + p]; }
    void moments(int p, double &W, double &dev2) const  // the mean of the 2 nc variances; the sum of the squared deviations of the 2 nc means
    {
        const int m = 2 * nc;
        double mm = 0.0;
        W = 0.0;
        for (int c = 0; c < nc; ++c) for (int k = 0; k < 2; ++k) { mm += mean(c, k, p); W += var(c, k, p); }
        mm /= m; W /= m;
        dev2 = 0.0;
        for (int c = 0; c < nc; ++c) for (int k = 0; k < 2; ++k) dev2 += (mean(c, k, p) - mm) * (mean(c, k, p) - mm);
    }
    double rhat(int p) const
    {
        double W, dev2;
        moments(p, W, dev2);
        return sqrt(((double)(h - 1) / h * W + dev2 / (2 * nc - 1)) / W);
    }
};
}
static int rank_diag_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, int32_t max_lag, double *rhat_bulk, double *rhat_tail,
                          double *ess_bulk, double *ess_tail, double *ess_mean, double *mcse_mean)
{
    if (!rhat_bulk && !rhat_tail && !ess_bulk && !ess_tail && !ess_mean && !mcse_mean) return fail(BNR_ERR_BAD_ARG, "no output requested");
    if (nsamp < 8) return fail(BNR_ERR_BAD_ARG, "need nsamp >= 8");
    if (max_lag < 2 || max_lag > nsamp / 2) return fail(BNR_ERR_BAD_ARG, "need 2 <= max_lag <= nsamp/2");
    bnr_chain *c = cs[0];
    const bnr_dev &d = c->d;
    const long long S = (long long)nc * nsamp;
    const int h = nsamp / 2, np = d.q + d.V;
    const long long n = (long long)nc * 2 * h;          // the split-chain draws that are ranked
    const int k05 = (int)floor((double)(n - 1) * 0.05) + 1, k95 = (int)floor((double)(n - 1) * 0.95) + 1;
    const bool want_bulk = rhat_bulk || ess_bulk, want_mean = ess_mean || mcse_mean, want_et = ess_tail != nullptr, want_rt = rhat_tail != nullptr;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->x.stream;
    int rc;
    if ((rc = pooled_quiesce(cs, nc))) return rc;
    const int blk = block_cols(S, c->rank_block_cols, np);
    const int Lmax = (ess_bulk || want_et || want_mean) ? max_lag : 1;
    dev_tmp tmp;
    double *X = nullptr, *Z = nullptr, *A = nullptr, *B = nullptr, *med = nullptr, *statd = nullptr;
    int *flagd = nullptr;
    rank_bufs rb;
    const size_t cells = (size_t)blk * (size_t)S;
    if ((rc = tmp.alloc(&X, cells, st, false))) return rc;
    if ((want_bulk || want_rt) && (rc = tmp.alloc(&Z, cells, st, false))) return rc;
    if ((want_et || want_rt || want_mean) && (rc = tmp.alloc(&A, cells, st, false))) return rc;
    if (want_et && (rc = tmp.alloc(&B, cells, st, false))) return rc;
    if ((rc = tmp.alloc(&rb.keyA, cells, st, false)) || (rc = tmp.alloc(&rb.keyB, cells, st, false)) || (rc = tmp.alloc(&rb.idxA, cells, st, false)) ||
        (rc = tmp.alloc(&rb.idxB, cells, st, false)))
        return rc;
    if ((rc = tmp.alloc(&med, (size_t)blk, st)) || (rc = tmp.alloc(&flagd, 2 * (size_t)blk, st))) return rc;
    if ((rc = tmp.alloc(&statd, (size_t)2 * (2 + Lmax) * (size_t)blk * nc, st, false))) return rc;
    const double nanv = NAN;
    std::vector<double> o_rb(np, nanv), o_rt(np, nanv), o_eb(np, nanv), o_et(np, nanv), o_em(np, nanv), o_mc(np, nanv);
    std::vector<int> flags(2 * (size_t)blk);
    split_msg sz, s05, s95, sx, sf;
    for (int p0 = 0; p0 < np; p0 += blk) {
        const int pc = std::min(blk, np - p0);
        stage_cols(st, cs, nc, first_row, nsamp, p0, pc, X);
        // one series: k_acov on the block's pc nc windows, its message fetched and laid out per chain; the ESS where lags were asked for
        auto series = [&](const double *data, int L, split_msg &m) -> int {
            const size_t cnt = (size_t)2 * (2 + L) * (size_t)pc * nc;
            launch_acov(st, data, nsamp, pc * nc, L, statd);
            m.raw.resize(cnt);
            hipError_t e = hipMemcpyAsync(m.raw.data(), statd, sizeof(double) * cnt, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string("rank_diag: ") + hipGetErrorString(e));
            if (int r = check_launch("k_acov")) return r;
            m.nc = nc; m.pc = pc; m.L = L; m.h = h;
            m.st.resize(cnt);
            for (int k = 0; k < 2; ++k) for (int j = 0; j < 2 + L; ++j) {
                const double *src = m.raw.data() + ((size_t)k * (2 + L) + j) * (size_t)pc * nc;
                for (int ch = 0; ch < nc; ++ch) {
                    double *dst = m.st.data() + (((size_t)ch * 2 + k) * (2 + L) + j) * (size_t)pc;
                    for (int p = 0; p < pc; ++p) dst[p] = src[(size_t)p * nc + ch];
                }
            }
            m.ess.assign(pc, NAN);
            if (L >= 2) return bnr_ess_from_stats(m.st.data(), nc, pc, nsamp, L, m.ess.data());
            return BNR_OK;
        };
        launch_rank(st, pc, X, S, nsamp, nc, 0, rb, k05, k95, nullptr, want_bulk ? Z : nullptr, want_et ? A : nullptr, want_et ? B : nullptr, med, flagd);
        if (want_bulk && (rc = series(Z, ess_bulk ? max_lag : 1, sz))) return rc;
        if (want_et && ((rc = series(A, max_lag, s05)) || (rc = series(B, max_lag, s95)))) return rc;
        if (want_mean) {                                     // on x - med: see k_fold
            launch_fold(st, pc, X, S, med, 0, A);
            if ((rc = series(A, max_lag, sx))) return rc;
        }
        if (want_rt) {
            launch_fold(st, pc, X, S, med, 1, A);
            launch_rank(st, pc, A, S, nsamp, nc, 0, rb, k05, k95, nullptr, Z, nullptr, nullptr, nullptr, flagd + blk);
            if ((rc = series(Z, 1, sf))) return rc;
        }
        HIPCHK(hipMemcpyAsync(flags.data(), flagd, sizeof(int) * 2 * (size_t)blk, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if ((rc = check_launch("k_rank"))) return rc;
        for (int p = 0; p < pc; ++p) {
            if (flags[p]) continue;                          // a NaN, an Inf or all draws equal: NaN throughout
            const int P = p0 + p;
            if (want_bulk) { o_rb[P] = sz.rhat(p); o_eb[P] = sz.ess[p]; }
            if (want_rt && !flags[(size_t)blk + p]) o_rt[P] = sf.rhat(p);
            if (want_et) o_et[P] = (s05.ess[p] != s05.ess[p] || s95.ess[p] != s95.ess[p]) ? nanv : std::min(s05.ess[p], s95.ess[p]);
            if (want_mean) {
                double W, dev2;
                sx.moments(p, W, dev2);
                const double sd2 = ((double)(h - 1) * (W * 2 * nc) + (double)h * dev2) / (double)(n - 1);
                o_em[P] = sx.ess[p];
                o_mc[P] = sqrt(sd2) / sqrt(sx.ess[p]);
            }
        }
    }
    const struct { double *dst; const std::vector<double> *src; } outs[] = {{rhat_bulk, &o_rb}, {rhat_tail, &o_rt}, {ess_bulk, &o_eb},
                                                                           {ess_tail, &o_et}, {ess_mean, &o_em}, {mcse_mean, &o_mc}};
    for (const auto &o : outs) if (o.dst) memcpy(o.dst, o.src->data(), sizeof(double) * np);
    return BNR_OK;
}
int bnr_chain_rank_diag(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t max_lag, double *rhat_bulk, double *rhat_tail, double *ess_bulk,
                        double *ess_tail, double *ess_mean, double *mcse_mean)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_rank_diag(&c, 1, first_row, nsamp, max_lag, rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_mean, mcse_mean);
}
int bnr_chains_rank_diag(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t max_lag, double *rhat_bulk,
                         double *rhat_tail, double *ess_bulk, double *ess_tail, double *ess_mean, double *mcse_mean)
{
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return rank_diag_call(chains, nchains, first_row, nsamp, max_lag, rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_mean, mcse_mean);
}
double bnr_host_ndtri(double p) { return bnr_ndtri(p); }

// Average ranks and normal scores of every row of a caller's m x S matrix (host, row-major), each row on its own: the companion of
// bnr_psis_loo / bnr_psis_weights, and k_rank's direct test.  On a stream of its own, the rows in blocks of about 256 MiB.
int bnr_rank_normalize(int32_t device, int32_t m, int32_t S, const double *x, double *ranks, double *z)
{
    if (!x || (!ranks && !z)) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (m < 1 || S < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows and S >= 1 draws");
    int rc;
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    hipStream_t st = guard.s;
    const int blk = block_rows((size_t)1 << 28, S, m);
    const size_t cells = (size_t)blk * (size_t)S;
    dev_tmp tmp;                                        // (freed before the stream goes)
    double *Xd = nullptr, *Rd = nullptr, *Zd = nullptr;
    int *flagd = nullptr;
    rank_bufs rb;
    if ((rc = tmp.alloc(&Xd, cells, st, false))) return rc;
    if (ranks && (rc = tmp.alloc(&Rd, cells, st, false))) return rc;
    if (z && (rc = tmp.alloc(&Zd, cells, st, false))) return rc;
    if ((rc = tmp.alloc(&rb.keyA, cells, st, false)) || (rc = tmp.alloc(&rb.keyB, cells, st, false)) || (rc = tmp.alloc(&rb.idxA, cells, st, false)) ||
        (rc = tmp.alloc(&rb.idxB, cells, st, false)) || (rc = tmp.alloc(&flagd, (size_t)blk, st)))
        return rc;
    for (int i0 = 0; i0 < m; i0 += blk) {
        const int mr = std::min(blk, m - i0);
        const size_t cnt = (size_t)mr * (size_t)S;
        HIPCHK(hipMemcpyAsync(Xd, x + (size_t)i0 * S, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
        launch_rank(st, mr, Xd, S, S, 1, 1, rb, 1, 1, Rd, Zd, nullptr, nullptr, nullptr, flagd);
        if (ranks) HIPCHK(hipMemcpyAsync(ranks + (size_t)i0 * S, Rd, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
        if (z) HIPCHK(hipMemcpyAsync(z + (size_t)i0 * S, Zd, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string("rank_normalize: ") + hipGetErrorString(e));
    return check_launch("k_rank");
}

// highest-density intervals and sign probabilities (ABI 13): k_hdi on `cols` staged columns of n draws with k_rank's key buffers (the index
// buffers stay unused)
static void launch_hdi(hipStream_t st, int cols, const double *buf, long long ld, int n, const rank_bufs &rb, int nprob, const bnr_hdi_levels &lv, double *lower,
                       double *upper, long long lstride, double *med, double *p_pos, double *p_neg)
{
    hipLaunchKernelGGL(k_hdi, dim3(cols), dim3(256), 0, st, buf, ld, n, rb.keyA, rb.keyB, nprob, lv, lower, upper, lstride, med, p_pos, p_neg);
}
// Highest-density intervals, the median and the sign probabilities (ABI 13) of every parameter in [gamma(q) | xi(V)] over the pooled window of
// the chains listed, or of every row of a caller's matrix: include/bnr_hip.h.  hdi_args: the checks that need no device, and the window length
// w = floor(prob n) of every level (in double, as numpy does; at most n - 1).
static int hdi_args(long long n, int32_t nprob, const double *probs, const double *lower, const double *upper, const double *median, const double *p_pos,
                    const double *p_neg, bnr_hdi_levels &lv)
{
    if (!lower && !upper && !median && !p_pos && !p_neg) return fail(BNR_ERR_BAD_ARG, "no output requested");
    if (!lower != !upper) return fail(BNR_ERR_BAD_ARG, "lower and upper come together");
    if (nprob < 0 || nprob > 8) return fail(BNR_ERR_BAD_ARG, "need 0 <= nprob <= 8 levels");
    if (nprob > 0 && !probs) return fail(BNR_ERR_BAD_ARG, "probs is NULL");
    if (lower && nprob < 1) return fail(BNR_ERR_BAD_ARG, "lower and upper need nprob >= 1 levels");
    for (int k = 0; k < 8; ++k) lv.w[k] = 0;
    for (int k = 0; k < nprob; ++k) {
        if (!(probs[k] > 0.0 && probs[k] < 1.0)) return fail(BNR_ERR_BAD_ARG, "every level must lie in (0, 1)");
        lv.w[k] = (int)std::min<double>(floor(probs[k] * (double)n), (double)(n - 1));
    }
    return BNR_OK;
}
// the results of an hdi call on the device: nprob lower and nprob upper bounds, the median, p_pos and p_neg of np columns each
struct hdi_slab {
    double *d = nullptr;
    size_t np = 0;
    int nprob = 0;
    int alloc(dev_tmp &tmp, int levels, size_t cols, hipStream_t st) { nprob = levels; np = cols; return tmp.alloc(&d, (size_t)(2 * nprob + 3) * np, st); }
    double *lower() const { return d; }
    double *upper() const { return d + (size_t)nprob * np; }
    double *med() const { return d + (size_t)2 * nprob * np; }
    double *p_pos() const { return med() + np; }
    double *p_neg() const { return med() + 2 * np; }
    int fetch(hipStream_t st, double *lo, double *up, double *median, double *pp, double *pn) const
    {
        std::vector<double> host((size_t)(2 * nprob + 3) * np);
        hipError_t e = hipMemcpyAsync(host.data(), d, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string("hdi: ") + hipGetErrorString(e));
        if (int rc = check_launch("k_hdi")) return rc;
        const double *h = host.data();
        if (lo) memcpy(lo, h, sizeof(double) * nprob * np);
        if (up) memcpy(up, h + (size_t)nprob * np, sizeof(double) * nprob * np);
        h += (size_t)2 * nprob * np;
        if (median) memcpy(median, h, sizeof(double) * np);
        if (pp) memcpy(pp, h + np, sizeof(double) * np);
        if (pn) memcpy(pn, h + 2 * np, sizeof(double) * np);
        return BNR_OK;
    }
};
static int hdi_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, int32_t nprob, const double *probs, double *lower, double *upper,
                    double *median, double *p_pos, double *p_neg)
{
    bnr_chain *c = cs[0];
    const bnr_dev &d = c->d;
    const long long S = (long long)nc * nsamp;
    bnr_hdi_levels lv;
    int rc;
    if ((rc = hdi_args(S, nprob, probs, lower, upper, median, p_pos, p_neg, lv))) return rc;
    const int np = d.q + d.V, levels = lower ? nprob : 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->x.stream;
    if ((rc = pooled_quiesce(cs, nc))) return rc;
    const int blk = block_cols(S, c->rank_block_cols, np);
    dev_tmp tmp;
    double *X = nullptr;
    rank_bufs rb;
    hdi_slab out;
    const size_t cells = (size_t)blk * (size_t)S;
    if ((rc = tmp.alloc(&X, cells, st, false)) || (rc = tmp.alloc(&rb.keyA, cells, st, false)) || (rc = tmp.alloc(&rb.keyB, cells, st, false))) return rc;
    if ((rc = out.alloc(tmp, levels, (size_t)np, st))) return rc;
    for (int p0 = 0; p0 < np; p0 += blk) {
        const int pc = std::min(blk, np - p0);
        stage_cols(st, cs, nc, first_row, nsamp, p0, pc, X);
        launch_hdi(st, pc, X, S, (int)S, rb, levels, lv, levels ? out.lower() + p0 : nullptr, levels ? out.upper() + p0 : nullptr, np, out.med() + p0,
                   out.p_pos() + p0, out.p_neg() + p0);
    }
    return out.fetch(st, lower, upper, median, p_pos, p_neg);
}
int bnr_chain_hdi(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t nprob, const double *probs, double *lower, double *upper, double *median,
                  double *p_pos, double *p_neg)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_hdi(&c, 1, first_row, nsamp, nprob, probs, lower, upper, median, p_pos, p_neg);
}
int bnr_chains_hdi(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t nprob, const double *probs, double *lower,
                   double *upper, double *median, double *p_pos, double *p_neg)
{
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return hdi_call(chains, nchains, first_row, nsamp, nprob, probs, lower, upper, median, p_pos, p_neg);
}
// k_hdi on every row of a caller's m x S matrix (host, row-major), each row on its own: k_hdi's direct test, as bnr_rank_normalize is k_rank's.
// On a stream of its own, the rows in blocks of about 256 MiB.
int bnr_hdi(int32_t device, int32_t m, int32_t S, const double *x, int32_t nprob, const double *probs, double *lower, double *upper, double *median,
            double *p_pos, double *p_neg)
{
    if (!x) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (m < 1 || S < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows and S >= 1 draws");
    bnr_hdi_levels lv;
    int rc;
    if ((rc = hdi_args(S, nprob, probs, lower, upper, median, p_pos, p_neg, lv))) return rc;
    const int levels = lower ? nprob : 0;
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    hipStream_t st = guard.s;
    const int blk = block_rows((size_t)1 << 28, S, m);
    const size_t cells = (size_t)blk * (size_t)S;
    dev_tmp tmp;                                        // (freed before the stream goes)
    double *Xd = nullptr;
    rank_bufs rb;
    hdi_slab out;
    if ((rc = tmp.alloc(&Xd, cells, st, false)) || (rc = tmp.alloc(&rb.keyA, cells, st, false)) || (rc = tmp.alloc(&rb.keyB, cells, st, false))) return rc;
    if ((rc = out.alloc(tmp, levels, (size_t)m, st))) return rc;
    for (int i0 = 0; i0 < m; i0 += blk) {
        const int mr = std::min(blk, m - i0);
        HIPCHK(hipMemcpyAsync(Xd, x + (size_t)i0 * S, sizeof(double) * (size_t)mr * (size_t)S, hipMemcpyHostToDevice, st));
        launch_hdi(st, mr, Xd, S, S, rb, levels, lv, levels ? out.lower() + i0 : nullptr, levels ? out.upper() + i0 : nullptr, m, out.med() + i0,
                   out.p_pos() + i0, out.p_neg() + i0);
    }
    return out.fetch(st, lower, upper, median, p_pos, p_neg);
}

// The joint posterior of the indicators (ABI 15): include/bnr_hip.h.  The six outputs of a call, and the checks that need no device
#define BNR_INCL_MAX_B 4096                              // k_incl_pack's counters: 4 (2 B + 1) bytes of LDS
namespace {
struct incl_out {
    double *prob, *joint, *size_pmf;
    int64_t *n_distinct;
    uint64_t *top_sets;
    int64_t *top_count;
};
}
static int incl_args(int32_t B, int32_t ntop, const incl_out &o)
{
    if (!o.prob && !o.joint && !o.size_pmf && !o.n_distinct && !o.top_sets && !o.top_count) return fail(BNR_ERR_BAD_ARG, "no output requested");
    if (!o.top_sets != !o.top_count) return fail(BNR_ERR_BAD_ARG, "top_sets and top_count come together");
    if (ntop < 0 || ntop > 256) return fail(BNR_ERR_BAD_ARG, "need 0 <= ntop <= 256");
    if (o.top_sets && ntop < 1) return fail(BNR_ERR_BAD_ARG, "top_sets and top_count need ntop >= 1");
    if (B > BNR_INCL_MAX_B) return fail(BNR_ERR_BAD_ARG, "more than 4096 indicators");
    return BNR_OK;
}
// The device work on S draws of B indicators, on st: k_incl_pack (from the chains' windows `srcd`, or from the bytes `zb`), k_incl_joint where
// the joint counts are wanted, k_incl_group where the distinct patterns are; then the counts come to the host and are divided by S once.
static int incl_run(hipStream_t st, dev_tmp &tmp, const bnr_incl_src *srcd, int nsamp, const unsigned char *zb, long long S_, int B, int32_t ntop,
                    const incl_out &o)
{
    const int S = (int)S_, W = (B + 63) / 64, CW = (int)((S_ + 63) / 64);
    const bool group = o.n_distinct || o.top_sets;
    const int nt = o.top_sets ? ntop : 0;
    unsigned long long *pat = nullptr, *col = nullptr, *keyA = nullptr, *keyB = nullptr, *topd = nullptr;
    unsigned int *marg = nullptr, *size = nullptr, *cnt = nullptr, *idxA = nullptr, *idxB = nullptr;
    long long *ndd = nullptr;                            // n_distinct, then the nt counts
    int rc;
    if ((rc = tmp.alloc(&marg, (size_t)B, st)) || (rc = tmp.alloc(&size, (size_t)B + 1, st))) return rc;
    if (o.joint && ((rc = tmp.alloc(&col, (size_t)B * CW, st, false)) || (rc = tmp.alloc(&cnt, (size_t)B * B, st)))) return rc;
    if (group) {
        if ((rc = tmp.alloc(&pat, (size_t)S * W, st, false)) || (rc = tmp.alloc(&keyA, (size_t)S, st, false)) || (rc = tmp.alloc(&keyB, (size_t)S, st, false)) ||
            (rc = tmp.alloc(&idxA, (size_t)S, st, false)) || (rc = tmp.alloc(&idxB, (size_t)S, st, false)) || (rc = tmp.alloc(&ndd, (size_t)1 + nt, st)) ||
            (rc = tmp.alloc(&topd, (size_t)nt * W, st)))
            return rc;
    }
    hipLaunchKernelGGL(k_incl_pack, dim3(std::min((CW + 3) / 4, 1024)), dim3(256), sizeof(unsigned int) * (2 * (size_t)B + 1), st, srcd, nsamp, zb, S, B, W, CW,
                       pat, col, marg, size);
    if (o.joint) {
        const int np = (B + 31) / 32;
        hipLaunchKernelGGL(k_incl_joint, dim3(np * (np + 1) / 2, std::min((CW + 63) / 64, 16)), dim3(256), 0, st, (const unsigned long long *)col, B, CW, cnt);
    }
    if (group)
        hipLaunchKernelGGL(k_incl_group, dim3(1), dim3(256), 0, st, (const unsigned long long *)pat, S, W, keyA, keyB, idxA, idxB, nt, ndd, topd, ndd + 1);
    std::vector<unsigned int> hm(B), hs((size_t)B + 1), hc(o.joint ? (size_t)B * B : 0);
    std::vector<long long> hn((size_t)1 + nt);
    HIPCHK(hipMemcpyAsync(hm.data(), marg, sizeof(unsigned int) * hm.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs.data(), size, sizeof(unsigned int) * hs.size(), hipMemcpyDeviceToHost, st));
    if (o.joint) HIPCHK(hipMemcpyAsync(hc.data(), cnt, sizeof(unsigned int) * hc.size(), hipMemcpyDeviceToHost, st));
    if (group) HIPCHK(hipMemcpyAsync(hn.data(), ndd, sizeof(long long) * hn.size(), hipMemcpyDeviceToHost, st));
    if (nt) HIPCHK(hipMemcpyAsync(o.top_sets, topd, sizeof(uint64_t) * (size_t)nt * W, hipMemcpyDeviceToHost, st));
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string("inclusion: ") + hipGetErrorString(e));
    if ((rc = check_launch("k_incl_pack"))) return rc;
    const double den = (double)S;
    if (o.prob) for (int k = 0; k < B; ++k) o.prob[k] = (double)hm[k] / den;
    if (o.size_pmf) for (int m = 0; m <= B; ++m) o.size_pmf[m] = (double)hs[m] / den;
    if (o.joint) for (size_t i = 0; i < hc.size(); ++i) o.joint[i] = (double)hc[i] / den;
    if (o.n_distinct) *o.n_distinct = hn[0];
    if (nt) for (int j = 0; j < nt; ++j) o.top_count[j] = hn[1 + j];
    return BNR_OK;
}
static int incl_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, int32_t which, int32_t ntop, const incl_out &o)
{
    if (which != 0 && which != 1) return fail(BNR_ERR_BAD_ARG, "which must be 0 (the node indicators xi) or 1 (the dimensions lambda)");
    int rc;
    bnr_chain *c = cs[0];
    if ((rc = incl_args(which ? c->d.R : c->d.V, ntop, o))) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->x.stream;
    if ((rc = pooled_quiesce(cs, nc))) return rc;
    std::vector<bnr_incl_src> src(nc);
    for (int k = 0; k < nc; ++k) {
        const bnr_dev &dk = cs[k]->d;
        src[k].base = dk.trace + (size_t)(first_row - 1) * dk.rowlen + (which ? dk.o_lam : dk.o_xi);
        src[k].stride = dk.rowlen;
    }
    dev_tmp tmp;
    bnr_incl_src *srcd = nullptr;
    if ((rc = tmp.alloc(&srcd, (size_t)nc, st, false))) return rc;
    HIPCHK(hipMemcpyAsync(srcd, src.data(), sizeof(bnr_incl_src) * nc, hipMemcpyHostToDevice, st));
    return incl_run(st, tmp, srcd, nsamp, nullptr, (long long)nc * nsamp, which ? c->d.R : c->d.V, ntop, o);
}
int bnr_chain_inclusion(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t which, int32_t ntop, double *prob, double *joint, double *size_pmf,
                        int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_inclusion(&c, 1, first_row, nsamp, which, ntop, prob, joint, size_pmf, n_distinct, top_sets, top_count);
}
int bnr_chains_inclusion(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t which, int32_t ntop, double *prob,
                         double *joint, double *size_pmf, int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count)
{
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return incl_call(chains, nchains, first_row, nsamp, which, ntop, incl_out{prob, joint, size_pmf, n_distinct, top_sets, top_count});
}
// the same on a caller's S x B matrix of bytes (host, row-major; != 0 is 1): the kernels' direct test, and the summary of any 0/1 trace.  On a
// stream of its own.
int bnr_inclusion(int32_t device, int32_t S, int32_t B, const uint8_t *z, int32_t ntop, double *prob, double *joint, double *size_pmf,
                  int64_t *n_distinct, uint64_t *top_sets, int64_t *top_count)
{
    if (!z) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (S < 1 || B < 1) return fail(BNR_ERR_BAD_ARG, "need S >= 1 draws and B >= 1 indicators");
    const incl_out o{prob, joint, size_pmf, n_distinct, top_sets, top_count};
    int rc;
    if ((rc = incl_args(B, ntop, o))) return rc;
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    hipStream_t st = guard.s;
    dev_tmp tmp;                                        // (freed before the stream goes)
    unsigned char *zd = nullptr;
    if ((rc = tmp.alloc(&zd, (size_t)S * (size_t)B, st, false))) return rc;
    HIPCHK(hipMemcpyAsync(zd, z, (size_t)S * (size_t)B, hipMemcpyHostToDevice, st));
    return incl_run(st, tmp, nullptr, S, zd, S, B, ntop, o);
}

// What a predict_rows call computes from a block's E behind k_predict, in the order of its launches; every pointer is a device pointer, and a
// NULL one skips its stage
struct pred_stages {
    int k_lo = 0, k_hi = 0;                                        // k_summary: mean and the k_lo-th / k_hi-th smallest of every E column
    double *mean = nullptr, *lower = nullptr, *upper = nullptr;
    double *lpd = nullptr, *pwaic = nullptr;                       // k_pred_loglik (needs yd)
    // PSIS (needs yd): the per-row tail lengths, the kernel's dynamic LDS, its outputs (never NULL).  keep_weights = false: k_psis, which
    // overwrites E; true: k_psis_w and on its weights the LOO predictive checks (ABI 11): k_loo_moments (all three or none) and k_loo_quantile
    // (each bound nullable) with its probabilities and the bracket's c (Phi(-c) < min(p_lo, 1 - p_hi) / 2)
    const int *tail_len = nullptr;
    int lds = 0;
    bool keep_weights = false;
    double *psis_lpd = nullptr, *elpd = nullptr, *khat = nullptr;
    double *loo_mean = nullptr, *loo_sd = nullptr, *loo_pit = nullptr, *loo_lower = nullptr, *loo_upper = nullptr;
    double p_lo = 0.0, p_hi = 0.0, c = 0.0;
    double *pit = nullptr;                                         // k_pred_pit: the PIT of the observed responses (needs yd)
    unsigned long long seed = 0;                                   // k_pred_noise with `seed`, then a second k_summary: the k_lo-th / k_hi-th
    double *pred_lower = nullptr, *pred_upper = nullptr;           // smallest draw of a new observation (both or none; overwrites E)
    // chain stacking (ABI 16): with wt both summaries are k_wsummary under these chain weights (the ranks k_lo / k_hi over K)
    const bnr_wsum_weights *wt = nullptr;
};
// k_psis: the sorted tail, 16 bytes per entry for up to BNR_PSIS_MAX_TAIL entries; k_psis_w: 12 bytes per entry.  On the current device, in front of the
// first launch of either (cheap enough for once per call)
static int psis_lds_attributes()
{
    const void *psis[] = {(const void *)&k_psis<0>, (const void *)&k_psis<1>};
    for (const void *f : psis) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * BNR_PSIS_MAX_TAIL));
    const void *psis_w[] = {(const void *)&k_psis_w<0>, (const void *)&k_psis_w<1>};
    for (const void *f : psis_w) HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, BNR_PSISW_ENTRY_BYTES * BNR_PSIS_MAX_TAIL));
    return BNR_OK;
}
static void launch_loow_inv_sd(hipStream_t st, const double *tau2, int S, double *isd)
{ hipLaunchKernelGGL(k_inv_sd, dim3((S + 255) / 256), dim3(256), 0, st, tau2, S, isd); }
// a block of mr rows starting at row i0 of the call: the weights of the block into LW, then what reads them
static void launch_loow_block(hipStream_t st, const pred_stages &sg, const double *E, double *LW, int S, int mr, int i0, const double *yd, const double *tau2,
                              const double *isd)
{
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psis_w<1>), dim3(mr), dim3(256), sg.lds, st, E, S, yd + i0, tau2, sg.tail_len + i0, LW, sg.psis_lpd + i0, sg.elpd + i0,
                       sg.khat + i0);
    if (sg.loo_mean)
        hipLaunchKernelGGL(k_loo_moments, dim3(mr), dim3(256), 0, st, E, (const double *)LW, S, yd + i0, tau2, sg.loo_mean + i0, sg.loo_sd + i0,
                           sg.loo_pit + i0);
    if (sg.loo_lower || sg.loo_upper)
        hipLaunchKernelGGL(k_loo_quantile, dim3(mr, 2), dim3(256), 0, st, E, (const double *)LW, S, tau2, isd, sg.c, sg.p_lo, sg.p_hi,
                           sg.loo_lower ? sg.loo_lower + i0 : nullptr, sg.loo_upper ? sg.loo_upper + i0 : nullptr);
}
// The device work of the prediction, log-likelihood and LOO calls, eagerly on the first chain's stream: the m rows of X (device, column-major,
// leading dimension ldx, zero in columns q .. q16 - 1 and readable for whole 32-row tiles) in blocks of rows whose E buffer (rows x S doubles,
// S = nc nsamp pooled draws: chain c's window in the columns c nsamp ..) stays near 1 GiB; per block one k_predict per chain, then the stages
// of sg that are wanted, in this order: k_summary (mean, k_lo-th / k_hi-th smallest of every E column), k_pred_loglik, the LOO predictive
// checks (k_psis_w and what reads its weights), k_psis, k_pred_pit, and last what overwrites E: k_pred_noise + a second k_summary (no call asks
// for that and k_psis, which overwrites E as well).  Blocks start at multiples of 32 rows, so an output's MFMA tile position and K order -- and
// with them every result, bit for bit -- do not depend on the block size; the noise is keyed by the row's index in the call.  With one chain
// and no extras: the launches of the single-chain entry points, unchanged.
static int predict_rows(bnr_chain *const *cs, int nc, int first_row, int nsamp, int m, const double *Xd, int ldx, const double *yd, const pred_stages &sg,
                        dev_tmp &tmp)
{
    bnr_chain *c = cs[0];
    const bnr_dev &d = c->d;
    hipStream_t st = c->x.stream;
    const long long S = (long long)nc * nsamp;
    const bool loow = sg.tail_len && sg.keep_weights, psis = sg.tail_len && !sg.keep_weights;
    const size_t budget = loow ? (size_t)1 << 29 : (size_t)1 << 30;        // (half the rows with the log weights beside E: E + LW stay near 1 GiB)
    long long blk = c->predict_block_rows > 0 ? c->predict_block_rows : (long long)(budget / ((size_t)S * sizeof(double))) / 32 * 32;
    blk = std::min<long long>(round_up((int)std::max<long long>(blk, 1), 32), round_up(m, 32));
    double *E = nullptr, *tau2 = nullptr, *pmean = nullptr, *LW = nullptr, *isd = nullptr;
    int rc;
    if ((rc = tmp.alloc(&E, (size_t)blk * (size_t)S, st))) return rc;
    if (loow && (rc = tmp.alloc(&LW, (size_t)blk * (size_t)S, st))) return rc;
    if (yd || sg.pit || sg.pred_lower) {
        if ((rc = tmp.alloc(&tau2, (size_t)S, st))) return rc;
        for (int k = 0; k < nc; ++k)
            launch_fetch_cols(st, cs[k]->d.trace, cs[k]->d.rowlen, ROW_TAU2, 1, first_row - 1, nsamp, tau2 + (size_t)k * nsamp, S);
    }
    if (sg.pred_lower && (rc = tmp.alloc(&pmean, (size_t)m, st))) return rc;      // (k_summary also writes the mean of y~: not returned)
    if (loow && (sg.loo_lower || sg.loo_upper)) {
        if ((rc = tmp.alloc(&isd, (size_t)S, st))) return rc;
        launch_loow_inv_sd(st, tau2, (int)S, isd);
    }
    const int q16 = round_up(d.q, 16);
    for (int i0 = 0; i0 < m; i0 += (int)blk) {
        const int mr = std::min<int>((int)blk, m - i0);
        for (int k = 0; k < nc; ++k) {
            const bnr_dev &dk = cs[k]->d;
            if (mr > 16)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_predict<2>), dim3((nsamp + 127) / 128, (mr + 31) / 32), dim3(256), 0, st, Xd + i0, ldx, q16,
                                   (const double *)dk.trace, dk.rowlen, dk.o_gamma, first_row - 1, nsamp, mr, E + (size_t)k * nsamp, S);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_predict<1>), dim3((nsamp + 127) / 128, 1), dim3(256), 0, st, Xd + i0, ldx, q16,
                                   (const double *)dk.trace, dk.rowlen, dk.o_gamma, first_row - 1, nsamp, mr, E + (size_t)k * nsamp, S);
        }
        if (sg.mean && sg.wt)
            launch_wsummary(st, mr, E, S, nsamp, nc, *sg.wt, mr, sg.k_lo, sg.k_hi, sg.mean + i0, sg.lower + i0, sg.upper + i0);
        else if (sg.mean)
            launch_summary(st, mr, E, (int)S, mr, sg.k_lo, sg.k_hi, sg.mean + i0, sg.lower + i0, sg.upper + i0);
        if (yd && sg.lpd)
            hipLaunchKernelGGL(k_pred_loglik, dim3(mr), dim3(256), 0, st, (const double *)E, (int)S, yd + i0, (const double *)tau2,
                               sg.lpd + i0, sg.pwaic + i0);
        if (loow)                                      // the LOO predictive checks read E: before anything that overwrites it
            launch_loow_block(st, sg, E, LW, (int)S, mr, i0, yd, tau2, isd);
        if (psis)                                      // last: k_psis turns the block's E into l in place
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psis<1>), dim3(mr), dim3(256), sg.lds, st, E, (int)S, yd + i0, (const double *)tau2, sg.tail_len + i0,
                               sg.psis_lpd + i0, sg.elpd + i0, sg.khat + i0);
        if (sg.pit)
            hipLaunchKernelGGL(k_pred_pit, dim3(mr), dim3(256), 0, st, (const double *)E, (int)S, yd + i0, (const double *)tau2, sg.pit + i0);
        if (sg.pred_lower) {                           // last: the block's E becomes draws of new observations in place
            const int gx = (int)((S + 255) / 256), gy = std::max(1, std::min(mr, 8192 / gx));
            hipLaunchKernelGGL(k_pred_noise, dim3(gx, gy), dim3(256), 0, st, E, S, (int)S, mr, i0, (const double *)tau2, sg.seed);
            if (sg.wt) launch_wsummary(st, mr, E, S, nsamp, nc, *sg.wt, mr, sg.k_lo, sg.k_hi, pmean + i0, sg.pred_lower + i0, sg.pred_upper + i0);
            else launch_summary(st, mr, E, (int)S, mr, sg.k_lo, sg.k_hi, pmean + i0, sg.pred_lower + i0, sg.pred_upper + i0);
        }
    }
    return check_launch("k_predict");
}

// The m new rows of a prediction call onto the first chain's device and stream, behind the checks of m, the element type and the matrices and
// behind the quiesce: X_pred goes to the device in its own element type and is converted there (k_x_convert with m rows; a float64 model matrix
// is copied straight in) into Xd, m_pad = round_up(m, 32) rows by round_up(q, 16) columns, and y (nullable) into yd
static int stage_new_rows(bnr_chain *const *cs, int nc, int m, const x_source &xs, const double *y, dev_tmp &tmp, double **Xd_out, double **yd_out)
{
    bnr_chain *c = cs[0];
    const bnr_dev &d = c->d;
    if (m < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows");
    if (xs.dtype < BNR_F64 || xs.dtype > BNR_F32) return fail(BNR_ERR_BAD_ARG, "unknown element type of X");
    if (xs.mats) for (int i = 0; i < m; ++i) if (!xs.mats[i]) return fail(BNR_ERR_BAD_ARG, "NULL adjacency matrix");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->x.stream;
    const int m_pad = round_up(m, 32), q16 = round_up(d.q, 16);
    double *Xd = nullptr;
    int rc;
    if ((rc = pooled_quiesce(cs, nc))) return rc;
    if ((rc = tmp.alloc(&Xd, (size_t)m_pad * q16, st))) return rc;             // zero rows m .. m_pad - 1 and columns q .. q16 - 1 (k_predict)
    *Xd_out = Xd;
    const size_t es = dtype_size(xs.dtype);
    if (!xs.mats && xs.dtype == BNR_F64) {
        HIPCHK(hipMemcpy2DAsync(Xd, (size_t)m_pad * sizeof(double), xs.X, (size_t)m * sizeof(double), (size_t)m * sizeof(double), d.q, hipMemcpyHostToDevice, st));
    } else {
        char *raw = nullptr;
        const size_t count = xs.mats ? (size_t)m * d.V * d.V : (size_t)m * d.q;
        if ((rc = tmp.alloc(&raw, count * es, st))) return rc;
        if (xs.mats) {
            for (int i = 0; i < m; ++i) HIPCHK(hipMemcpyAsync(raw + (size_t)i * d.V * d.V * es, xs.mats[i], (size_t)d.V * d.V * es, hipMemcpyHostToDevice, st));
        } else HIPCHK(hipMemcpyAsync(raw, xs.X, count * es, hipMemcpyHostToDevice, st));
        launch_x_convert(xs.dtype, raw, xs.mats != nullptr, m, d, m_pad, Xd, nullptr, nullptr, st);
    }
    if (y) {
        if ((rc = tmp.alloc(yd_out, (size_t)m, st))) return rc;
        HIPCHK(hipMemcpyAsync(*yd_out, y, sizeof(double) * m, hipMemcpyHostToDevice, st));
    }
    return BNR_OK;
}
// Posterior of the mean response mu + x . gamma of m new rows over rows first_row .. first_row+nsamp-1 of the chains listed (an addition to the
// reference): stage_new_rows, then predict_rows.  pred_lower / pred_upper / pit (host, nullable): the extras of the pooled entry points.
static int predict_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, int32_t m, const x_source &xs, const double *y, int32_t k_lo,
                        int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic, uint64_t pred_seed, double *pred_lower,
                        double *pred_upper, double *pit)
{
    const long long S = (long long)nc * nsamp;
    if (k_lo < 1 || k_lo > S || k_hi < 1 || k_hi > S)
        return fail(BNR_ERR_BAD_ARG, nc == 1 ? "order statistics must be between 1 and nsamp" : "order statistics must be between 1 and nchains * nsamp");
    dev_tmp tmp;
    double *Xd = nullptr, *yd = nullptr;
    result_slab out;
    int rc;
    if ((rc = stage_new_rows(cs, nc, m, xs, y, tmp, &Xd, &yd))) return rc;
    hipStream_t st = cs[0]->x.stream;
    if ((rc = out.alloc(tmp, pred_lower || pit ? 8 : 5, (size_t)m, st))) return rc;
    pred_stages sg;
    sg.k_lo = k_lo; sg.k_hi = k_hi;
    sg.mean = out.col(0); sg.lower = out.col(1); sg.upper = out.col(2);
    if (y) { sg.lpd = out.col(3); sg.pwaic = out.col(4); }
    if (pred_lower) { sg.seed = pred_seed; sg.pred_lower = out.col(5); sg.pred_upper = out.col(6); }
    if (pit) sg.pit = out.col(7);
    if ((rc = predict_rows(cs, nc, first_row, nsamp, m, Xd, round_up(m, 32), yd, sg, tmp))) return rc;
    return out.fetch(st, "predict", "k_predict", {mean, lower, upper, y ? lpd : nullptr, y ? pwaic : nullptr, pred_lower, pred_lower ? pred_upper : nullptr, pit});
}
// the checks of the entry points, in their order: pred_lower and pred_upper come together; lpd / pwaic and pit need y
static int predict_pooled(bnr_chain *const *cs, int32_t nc, int32_t first_row, int32_t nsamp, int32_t m, const x_source &xs, const double *y, int32_t k_lo,
                          int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic, uint64_t pred_seed, double *pred_lower,
                          double *pred_upper, double *pit)
{
    if (!cs || !mean || !lower || !upper || (!xs.X && !xs.mats) || (y && (!lpd || !pwaic)) || (!pred_lower != !pred_upper))
        return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (pit && !y) return fail(BNR_ERR_BAD_ARG, "pit needs the observed responses y");
    if (int rc = pooled_check(cs, nc, first_row, nsamp)) return rc;
    return predict_call(cs, nc, first_row, nsamp, m, xs, y, k_lo, k_hi, mean, lower, upper, lpd, pwaic, pred_seed, pred_lower, pred_upper, pit);
}
int bnr_chain_predict(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t m, const void *X, int32_t x_dtype, const double *y,
                      int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_predict(&c, 1, first_row, nsamp, m, X, x_dtype, y, k_lo, k_hi, mean, lower, upper, lpd, pwaic, 0, nullptr, nullptr, nullptr);
}
int bnr_chain_predict_from_matrices(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t m, const void *const *A, int32_t x_dtype,
                                    const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_predict_from_matrices(&c, 1, first_row, nsamp, m, A, x_dtype, y, k_lo, k_hi, mean, lower, upper, lpd, pwaic, 0, nullptr, nullptr,
                                            nullptr);
}
int bnr_chains_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t m, const void *X, int32_t x_dtype,
                       const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd, double *pwaic,
                       uint64_t pred_seed, double *pred_lower, double *pred_upper, double *pit)
{
    x_source xs;
    xs.X = X; xs.dtype = x_dtype;
    return predict_pooled(chains, nchains, first_row, nsamp, m, xs, y, k_lo, k_hi, mean, lower, upper, lpd, pwaic, pred_seed, pred_lower, pred_upper, pit);
}
int bnr_chains_predict_from_matrices(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t m, const void *const *A,
                                     int32_t x_dtype, const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper,
                                     double *lpd, double *pwaic, uint64_t pred_seed, double *pred_lower, double *pred_upper, double *pit)
{
    x_source xs;
    xs.mats = A; xs.dtype = x_dtype;
    return predict_pooled(chains, nchains, first_row, nsamp, m, xs, y, k_lo, k_hi, mean, lower, upper, lpd, pwaic, pred_seed, pred_lower, pred_upper, pit);
}
// the element-by-element host mirror of k_pred_noise's draws: out[(i - i0) ns + (s - s0)] = bnr_normal(seed, s, SITE_PRED, i, 0)
void bnr_host_pred_noise(uint64_t seed, uint32_t s0, uint32_t ns, uint32_t i0, uint32_t ni, double *out)
{
    if (!out) return;
    for (uint32_t i = 0; i < ni; ++i)
        for (uint32_t s = 0; s < ns; ++s) out[(size_t)i * ns + s] = bnr_normal(seed, s0 + s, SITE_PRED, i0 + i, 0u);
}
// The calls on the chains' own training rows: X (n_pad x q_pad, zero padded) and y are on the device already.  analysis_call holds what they
// share: the device, the quiesce, the result slab of k columns of n doubles and -- with_tails: for PSIS -- the tail lengths on the device
struct analysis_call {
    dev_tmp tmp;
    result_slab out;
    pred_stages sg;
    hipStream_t st = nullptr;
    int begin(bnr_chain *const *cs, int nc, int k, const std::vector<int> *tails, int lds)
    {
        bnr_chain *c = cs[0];
        HIPCHK(hipSetDevice(c->device));
        st = c->x.stream;
        int rc;
        if ((rc = pooled_quiesce(cs, nc))) return rc;
        if ((rc = out.alloc(tmp, k, (size_t)c->d.n, st))) return rc;
        if (tails) {
            int *tl = nullptr;
            if ((rc = tmp.alloc(&tl, (size_t)c->d.n, st))) return rc;
            HIPCHK(hipMemcpyAsync(tl, tails->data(), sizeof(int) * c->d.n, hipMemcpyHostToDevice, st));
            sg.tail_len = tl; sg.lds = lds;
            sg.psis_lpd = out.col(0); sg.elpd = out.col(1); sg.khat = out.col(2);
        }
        return BNR_OK;
    }
    int run(bnr_chain *const *cs, int nc, int first_row, int nsamp)
    {
        const bnr_dev &d = cs[0]->d;
        return predict_rows(cs, nc, first_row, nsamp, d.n, d.X, d.n_pad, d.y, sg, tmp);
    }
};
// pointwise lpd and WAIC penalty (and, pooled entry point only, the PIT)
static int loglik_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, double *lpd, double *pwaic, double *pit)
{
    analysis_call a;
    int rc;
    if ((rc = a.begin(cs, nc, pit ? 3 : 2, nullptr, 0))) return rc;
    a.sg.lpd = a.out.col(0); a.sg.pwaic = a.out.col(1);
    if (pit) a.sg.pit = a.out.col(2);
    if ((rc = a.run(cs, nc, first_row, nsamp))) return rc;
    return a.out.fetch(a.st, "loglik_stats", "k_pred_loglik", {lpd, pwaic, pit});
}
int bnr_chain_loglik_stats(bnr_chain *c, int32_t first_row, int32_t nsamp, double *lpd, double *pwaic)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_loglik_stats(&c, 1, first_row, nsamp, lpd, pwaic, nullptr);
}
int bnr_chains_loglik_stats(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, double *lpd, double *pwaic, double *pit)
{
    if (!chains || !lpd || !pwaic) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return loglik_call(chains, nchains, first_row, nsamp, lpd, pwaic, pit);
}

// loo 2.x's tail length M = ceil(min(0.2 S, 3 sqrt(S / r_eff))) of every row (r_eff NULL: 1), checked against BNR_PSIS_MAX_TAIL, and the
// dynamic LDS of the longest tail that is smoothed (M >= 5), P = its length rounded up to a power of two: 16 bytes per entry for k_psis
// (entry_bytes' default), 12 for k_psis_w; 8 KiB at least (the histogram of the radix select)
static int psis_tail_lengths(int m, int nsamp, const double *r_eff, std::vector<int> &M, int &lds, int entry_bytes = 16)
{
    M.assign(m, 0);
    int pmax = 0;
    for (int i = 0; i < m; ++i) {
        const double r = r_eff ? r_eff[i] : 1.0;
        if (!(r > 0.0) || !std::isfinite(r)) return fail(BNR_ERR_BAD_ARG, "r_eff must be positive and finite");
        const double t = std::ceil(std::min(0.2 * nsamp, 3.0 * std::sqrt(nsamp / r)));
        if (t > BNR_PSIS_MAX_TAIL)
            return fail(BNR_ERR_BAD_ARG, "PSIS tail length " + std::to_string((long long)t) + " of row " + std::to_string(i + 1) + " exceeds the supported " +
                                             std::to_string(BNR_PSIS_MAX_TAIL) + " (raise r_eff or shorten the window)");
        M[i] = (int)t;
        if (M[i] >= 5) {
            int p = 8;
            while (p < M[i]) p <<= 1;
            pmax = std::max(pmax, p);
        }
    }
    lds = std::max(8192, entry_bytes * pmax);
    return BNR_OK;
}
// PSIS-LOO of the chains' own training rows over rows first_row .. first_row+nsamp-1 of every chain listed (k_predict, then k_psis on every block
// of rows); the tail length comes from the pooled draw count
static int loo_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, const double *r_eff, double *lpd, double *elpd_loo, double *pareto_k)
{
    std::vector<int> M;
    int lds = 0, rc;
    if ((rc = psis_tail_lengths(cs[0]->d.n, nc * nsamp, r_eff, M, lds))) return rc;
    HIPCHK(hipSetDevice(cs[0]->device));
    if ((rc = psis_lds_attributes())) return rc;
    analysis_call a;
    if ((rc = a.begin(cs, nc, 3, &M, lds))) return rc;
    if ((rc = a.run(cs, nc, first_row, nsamp))) return rc;
    return a.out.fetch(a.st, "loo", "k_psis", {lpd, elpd_loo, pareto_k});
}
int bnr_chain_loo(bnr_chain *c, int32_t first_row, int32_t nsamp, const double *r_eff, double *lpd, double *elpd_loo, double *pareto_k)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_loo(&c, 1, first_row, nsamp, r_eff, lpd, elpd_loo, pareto_k);
}
int bnr_chains_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, double *lpd, double *elpd_loo,
                   double *pareto_k)
{
    if (!chains || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return loo_call(chains, nchains, first_row, nsamp, r_eff, lpd, elpd_loo, pareto_k);
}

// LOO predictive checks (ABI 11) of the chains' own training rows over the pooled window: k_predict, then k_psis_w (the PSIS weights of the block),
// k_loo_moments and k_loo_quantile on every block of rows.  Every output is nullable; lpd, elpd_loo and pareto_k always come from k_psis_w.
static int loo_predict_call(bnr_chain *const *cs, int nc, int32_t first_row, int32_t nsamp, const double *r_eff, double p_lo, double p_hi, double *lpd,
                            double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit, double *loo_lower, double *loo_upper)
{
    const bool bounds = loo_lower || loo_upper, moments = loo_mean || loo_sd || loo_pit;
    double cc = 0.0;
    if (bounds) {
        if (!(p_lo > 0.0) || !(p_hi < 1.0) || !(p_lo < p_hi)) return fail(BNR_ERR_BAD_ARG, "need 0 < p_lo < p_hi < 1");
        const double pm = 0.5 * std::min(p_lo, 1.0 - p_hi);
        for (cc = 1.0; !(0.5 * std::erfc(cc * 0.70710678118654752440) < pm) && cc < 40.0; cc += 0.5) { }
    }
    std::vector<int> M;
    int lds = 0, rc;
    if ((rc = psis_tail_lengths(cs[0]->d.n, nc * nsamp, r_eff, M, lds, BNR_PSISW_ENTRY_BYTES))) return rc;
    HIPCHK(hipSetDevice(cs[0]->device));
    if ((rc = psis_lds_attributes())) return rc;
    analysis_call a;
    if ((rc = a.begin(cs, nc, 8, &M, lds))) return rc;
    pred_stages &sg = a.sg;
    sg.keep_weights = true;
    if (moments) { sg.loo_mean = a.out.col(3); sg.loo_sd = a.out.col(4); sg.loo_pit = a.out.col(5); }
    if (loo_lower) sg.loo_lower = a.out.col(6);
    if (loo_upper) sg.loo_upper = a.out.col(7);
    sg.p_lo = p_lo; sg.p_hi = p_hi; sg.c = cc;
    if ((rc = a.run(cs, nc, first_row, nsamp))) return rc;
    return a.out.fetch(a.st, "loo_predict", "k_psis_w", {lpd, elpd_loo, pareto_k, loo_mean, loo_sd, loo_pit, loo_lower, loo_upper});
}
int bnr_chain_loo_predict(bnr_chain *c, int32_t first_row, int32_t nsamp, const double *r_eff, double p_lo, double p_hi, double *lpd, double *elpd_loo,
                          double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit, double *loo_lower, double *loo_upper)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_loo_predict(&c, 1, first_row, nsamp, r_eff, p_lo, p_hi, lpd, elpd_loo, pareto_k, loo_mean, loo_sd, loo_pit, loo_lower, loo_upper);
}
int bnr_chains_loo_predict(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, double p_lo, double p_hi,
                           double *lpd, double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *loo_pit, double *loo_lower,
                           double *loo_upper)
{
    if (int rc = pooled_check(chains, nchains, first_row, nsamp)) return rc;
    return loo_predict_call(chains, nchains, first_row, nsamp, r_eff, p_lo, p_hi, lpd, elpd_loo, pareto_k, loo_mean, loo_sd, loo_pit, loo_lower, loo_upper);
}

// The device work of bnr_psis_loo and bnr_psis_weights on the call's stream st: the rows of the caller's matrix in blocks, k_psis<0> on every block
// of about 1 GiB; with log_weights k_psis_w<0> on every block of about 512 MiB (l and the weights side by side), the block's weights copied back
// behind it (and no lpd)
static int psis_matrix(hipStream_t st, int m, int nsamp, const double *loglik, const std::vector<int> &tail_len, int lds, double *log_weights, double *lpd,
                       double *elpd, double *khat)
{
    const int blk = block_rows(log_weights ? (size_t)1 << 29 : (size_t)1 << 30, nsamp, m);
    int rc;
    dev_tmp tmp;                                        // (freed before the stream goes)
    double *Ld = nullptr, *Wd = nullptr;
    int *tl = nullptr;
    result_slab out;
    if ((rc = tmp.alloc(&Ld, (size_t)blk * nsamp, st))) return rc;
    if (log_weights && (rc = tmp.alloc(&Wd, (size_t)blk * nsamp, st))) return rc;
    if ((rc = out.alloc(tmp, 3, (size_t)m, st))) return rc;
    if ((rc = tmp.alloc(&tl, (size_t)m, st))) return rc;
    HIPCHK(hipMemcpyAsync(tl, tail_len.data(), sizeof(int) * m, hipMemcpyHostToDevice, st));
    for (int i0 = 0; i0 < m; i0 += blk) {
        const int mr = std::min(blk, m - i0);
        HIPCHK(hipMemcpyAsync(Ld, loglik + (size_t)i0 * nsamp, sizeof(double) * (size_t)mr * nsamp, hipMemcpyHostToDevice, st));
        if (log_weights) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psis_w<0>), dim3(mr), dim3(256), lds, st, (const double *)Ld, nsamp, (const double *)nullptr,
                               (const double *)nullptr, (const int *)tl + i0, Wd, (double *)nullptr, out.col(1) + i0, out.col(2) + i0);
            HIPCHK(hipMemcpyAsync(log_weights + (size_t)i0 * nsamp, Wd, sizeof(double) * (size_t)mr * nsamp, hipMemcpyDeviceToHost, st));
        } else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psis<0>), dim3(mr), dim3(256), lds, st, Ld, nsamp, (const double *)nullptr, (const double *)nullptr,
                               (const int *)tl + i0, out.col(0) + i0, out.col(1) + i0, out.col(2) + i0);
    }
    return out.fetch(st, log_weights ? "psis_weights" : "psis_loo", log_weights ? "k_psis_w" : "k_psis", {lpd, elpd, khat});
}
// PSIS on a caller's m x nsamp log-likelihood matrix (host, row-major): bnr_psis_loo (k_psis) and its companion bnr_psis_weights, which also
// returns the weights (k_psis_w: log_weights != NULL).  The shared front: the checks in their order, the tail lengths, the device
static int psis_call(int32_t device, int32_t m, int32_t nsamp, const double *loglik, const double *r_eff, double *log_weights, double *lpd, double *elpd_loo,
                     double *pareto_k)
{
    if (m < 1 || nsamp < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows and nsamp >= 1 draws");
    std::vector<int> M;
    int lds = 0, rc;
    if ((rc = psis_tail_lengths(m, nsamp, r_eff, M, lds, log_weights ? BNR_PSISW_ENTRY_BYTES : 16))) return rc;
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    if ((rc = psis_lds_attributes())) return rc;
    return psis_matrix(guard.s, m, nsamp, loglik, M, lds, log_weights, lpd, elpd_loo, pareto_k);
}
int bnr_psis_loo(int32_t device, int32_t m, int32_t nsamp, const double *loglik, const double *r_eff, double *elpd_loo, double *pareto_k, double *lpd)
{
    if (!loglik || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return psis_call(device, m, nsamp, loglik, r_eff, nullptr, lpd, elpd_loo, pareto_k);
}
int bnr_psis_weights(int32_t device, int32_t m, int32_t nsamp, const double *loglik, const double *r_eff, double *log_weights, double *elpd_loo,
                     double *pareto_k)
{
    if (!loglik || !log_weights) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return psis_call(device, m, nsamp, loglik, r_eff, log_weights, nullptr, elpd_loo, pareto_k);
}

// ------------------------------------------------------------------------------------------ chain stacking (ABI 16): include/bnr_hip.h
// The stacking weights of K chains from their pointwise predictive log densities (Yao, Vehtari & Gelman 2022): the maximiser over the simplex of
// f(w) = (1 / n) sum_i log sum_k w_k exp(lpd_ik), by the multiplicative (EM) fixed point w <- w o g, g_k = (1 / n) sum_i p_ik / sum_j w_j p_ij,
// p_ik = exp(lpd_ik - max_k lpd_ik), from w = 1 / K; after every update w is divided by its sum (1 up to rounding: sum_k w_k g_k = 1), so
// that round-off does not accumulate over thousands of updates.  f is concave, so max_k g_k - 1 bounds f(w*) - f(w) whatever produced w: the
// iteration stops when it is <= gap_tol or after max_iter updates.  Pure host code; every sum in index order.
int bnr_stacking_weights(int32_t n, int32_t K, const double *lpd, int32_t max_iter, double gap_tol, double *weights, double *objective, double *gap,
                         int32_t *iters)
{
    if (!lpd || !weights) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (n < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows");
    if (K < 1 || K > BNR_STACK_MAX_CHAINS) return fail(BNR_ERR_BAD_ARG, "need 1 <= K <= 32 chains");
    if (max_iter < 1) return fail(BNR_ERR_BAD_ARG, "need max_iter >= 1");
    if (!std::isfinite(gap_tol) || !(gap_tol > 0.0)) return fail(BNR_ERR_BAD_ARG, "gap_tol must be positive and finite");
    std::vector<double> p((size_t)n * K), rmax(n), g(K), w(K, 1.0 / K);
    for (int i = 0; i < n; ++i) {
        double mx = -INFINITY;
        for (int k = 0; k < K; ++k) {
            const double v = lpd[(size_t)i * K + k];
            if (v != v || v == INFINITY) return fail(BNR_ERR_BAD_ARG, "lpd holds a NaN or +Inf");
            mx = std::max(mx, v);
        }
        if (mx == -INFINITY) return fail(BNR_ERR_BAD_ARG, "row " + std::to_string(i + 1) + " of lpd is -Inf for every chain");
        rmax[i] = mx;
        for (int k = 0; k < K; ++k) p[(size_t)i * K + k] = exp(lpd[(size_t)i * K + k] - mx);
    }
    int it = 0;
    double gp = 0.0, f = 0.0;
    for (;;) {
        for (int k = 0; k < K; ++k) g[k] = 0.0;
        f = 0.0;
        for (int i = 0; i < n; ++i) {
            const double *pi = p.data() + (size_t)i * K;
            double d = 0.0;
            for (int k = 0; k < K; ++k) d += w[k] * pi[k];
            for (int k = 0; k < K; ++k) g[k] += pi[k] / d;
            f += rmax[i] + log(d);
        }
        gp = -INFINITY;
        for (int k = 0; k < K; ++k) { g[k] /= n; gp = std::max(gp, g[k]); }
        gp -= 1.0;
        if (gp <= gap_tol || it == max_iter) break;
        double s = 0.0;
        for (int k = 0; k < K; ++k) { w[k] *= g[k]; s += w[k]; }
        for (int k = 0; k < K; ++k) w[k] /= s;
        ++it;
    }
    memcpy(weights, w.data(), sizeof(double) * K);
    if (objective) *objective = f / n;
    if (gap) *gap = gp;
    if (iters) *iters = it;
    return BNR_OK;
}

// the weights of a weighted call, checked and packed for k_wsummary: finite, >= 0, one > 0, |sum - 1| <= 1e-9; used as given
static int wsum_pack(const double *weights, int K, bnr_wsum_weights &wt)
{
    if (K < 1 || K > BNR_STACK_MAX_CHAINS) return fail(BNR_ERR_BAD_ARG, "need 1 <= nchains <= 32 for a weighted call");
    double s = 0.0;
    bool any = false;
    for (int k = 0; k < BNR_STACK_MAX_CHAINS; ++k) wt.w[k] = 0.0;
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(weights[k]) || weights[k] < 0.0) return fail(BNR_ERR_BAD_ARG, "weights must be finite and >= 0");
        any = any || weights[k] > 0.0;
        s += weights[k];
        wt.w[k] = weights[k];
    }
    if (!any) return fail(BNR_ERR_BAD_ARG, "at least one weight must be > 0");
    if (!(fabs(s - 1.0) <= 1e-9)) return fail(BNR_ERR_BAD_ARG, "weights must sum to 1 (within 1e-9)");
    return BNR_OK;
}
// log sum_{k: w_k > 0} w_k exp(v_k) with the largest such v_k taken out, k ascending (v: stride ldv)
static double wlse(const double *v, size_t ldv, const double *w, int K)
{
    double M = -INFINITY;
    for (int k = 0; k < K; ++k) if (w[k] > 0.0) M = std::max(M, v[k * ldv]);
    double s = 0.0;
    for (int k = 0; k < K; ++k) if (w[k] > 0.0) s += w[k] * exp(v[k * ldv] - M);
    return M + log(s);
}

// bnr_chains_summary under chain weights: summary_call with the packed weights
int bnr_chains_wsummary(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t k_lo, int32_t k_hi,
                        double *mean_gamma, double *lower, double *upper, double *prob_xi)
{
    if (!chains || !weights || !mean_gamma || !lower || !upper || !prob_xi) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc;
    bnr_wsum_weights wt;
    if ((rc = wsum_pack(weights, nchains, wt))) return rc;
    if ((rc = pooled_check(chains, nchains, first_row, nsamp))) return rc;
    return summary_call(chains, nchains, first_row, nsamp, k_lo, k_hi, &wt, mean_gamma, lower, upper, prob_xi);
}

// k_wsummary on every row of a caller's m x (K nsamp) matrix (host, row-major), each row on its own: the kernel's direct test, as bnr_hdi is
// k_hdi's.  On a stream of its own, the rows in blocks of about 256 MiB.
int bnr_wquantile(int32_t device, int32_t m, int32_t K, int32_t nsamp, const double *x, const double *weights, int32_t k_lo, int32_t k_hi, double *mean,
                  double *lower, double *upper)
{
    if (!x || !weights) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!mean && !lower && !upper) return fail(BNR_ERR_BAD_ARG, "no output requested");
    if (!lower != !upper) return fail(BNR_ERR_BAD_ARG, "lower and upper come together");
    if (m < 1 || nsamp < 1) return fail(BNR_ERR_BAD_ARG, "need m >= 1 rows and nsamp >= 1 draws per chain");
    bnr_wsum_weights wt;
    int rc;
    if ((rc = wsum_pack(weights, K, wt))) return rc;
    const long long S = (long long)K * nsamp;
    if (S > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    if (lower && (k_lo < 1 || k_lo > S || k_hi < 1 || k_hi > S)) return fail(BNR_ERR_BAD_ARG, "order statistics must be between 1 and K * nsamp");
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    hipStream_t st = guard.s;
    const int blk = block_rows((size_t)1 << 28, S, m);
    dev_tmp tmp;                                        // (freed before the stream goes)
    double *Xd = nullptr;
    result_slab out;
    if ((rc = tmp.alloc(&Xd, (size_t)blk * (size_t)S, st, false))) return rc;
    if ((rc = out.alloc(tmp, 3, (size_t)m, st))) return rc;
    for (int i0 = 0; i0 < m; i0 += blk) {
        const int mr = std::min(blk, m - i0);
        HIPCHK(hipMemcpyAsync(Xd, x + (size_t)i0 * S, sizeof(double) * (size_t)mr * (size_t)S, hipMemcpyHostToDevice, st));
        launch_wsummary(st, mr, Xd, S, nsamp, K, wt, mr, lower ? k_lo : 1, lower ? k_hi : 1, mean ? out.col(0) + i0 : nullptr,
                        lower ? out.col(1) + i0 : nullptr, lower ? out.col(2) + i0 : nullptr);
    }
    return out.fetch(st, "wquantile", "k_wsummary", {mean, lower, upper});
}

// Per-chain PSIS-LOO and the stacking weights in one call: row k of elpd_chain / pareto_k_chain is bnr_chain_loo of chains[k] (the existing path,
// chain by chain: the tail length comes from nsamp), the weights are bnr_stacking_weights of the rows that are finite in every chain
int bnr_chains_stack(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, const double *r_eff, int32_t max_iter, double gap_tol,
                     double *weights, double *elpd_chain, double *pareto_k_chain, double *elpd_stack, double *gap, int32_t *iters)
{
    if (!chains || !weights) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc;
    if (nchains > BNR_STACK_MAX_CHAINS) return fail(BNR_ERR_BAD_ARG, "need nchains <= 32");
    if ((rc = pooled_check(chains, nchains, first_row, nsamp))) return rc;
    if (max_iter < 1) return fail(BNR_ERR_BAD_ARG, "need max_iter >= 1");
    if (!std::isfinite(gap_tol) || !(gap_tol > 0.0)) return fail(BNR_ERR_BAD_ARG, "gap_tol must be positive and finite");
    const int K = nchains, n = chains[0]->d.n;
    HIPCHK(hipSetDevice(chains[0]->device));
    if ((rc = pooled_quiesce(chains, nchains))) return rc;            // (as every pooled call: what the other chains' streams still hold)
    std::vector<double> el((size_t)K * n), kh((size_t)K * n);
    for (int k = 0; k < K; ++k) {
        bnr_chain *ck = chains[k];
        if ((rc = loo_call(&ck, 1, first_row, nsamp, r_eff, nullptr, el.data() + (size_t)k * n, kh.data() + (size_t)k * n))) return rc;
    }
    std::vector<double> lp;
    std::vector<char> used(n, 1);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < K; ++k) if (!std::isfinite(el[(size_t)k * n + i])) used[i] = 0;
        if (used[i]) for (int k = 0; k < K; ++k) lp.push_back(el[(size_t)k * n + i]);
    }
    const int nu = (int)(lp.size() / K);
    double gp = NAN;
    int32_t it = 0;
    if (nu < 1) for (int k = 0; k < K; ++k) weights[k] = 1.0 / K;
    else if ((rc = bnr_stacking_weights(nu, K, lp.data(), max_iter, gap_tol, weights, nullptr, &gp, &it))) return rc;
    if (elpd_chain) memcpy(elpd_chain, el.data(), sizeof(double) * el.size());
    if (pareto_k_chain) memcpy(pareto_k_chain, kh.data(), sizeof(double) * kh.size());
    if (elpd_stack) for (int i = 0; i < n; ++i) elpd_stack[i] = used[i] ? wlse(el.data() + i, (size_t)n, weights, K) : NAN;
    if (gap) *gap = gp;
    if (iters) *iters = it;
    return BNR_OK;
}

// bnr_chains_predict for a model matrix under chain weights: k_wsummary over the eta columns of the pooled k_predict (and over the columns
// after k_pred_noise); every chain's own lpd from the single-chain launches, combined here
int bnr_chains_wpredict(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t m, const void *X,
                        int32_t x_dtype, const double *y, int32_t k_lo, int32_t k_hi, double *mean, double *lower, double *upper, double *lpd,
                        uint64_t pred_seed, double *pred_lower, double *pred_upper)
{
    if (!chains || !weights || !X || !mean || !lower || !upper || (y && !lpd) || (!pred_lower != !pred_upper)) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc;
    bnr_wsum_weights wt;
    if ((rc = wsum_pack(weights, nchains, wt))) return rc;
    if ((rc = pooled_check(chains, nchains, first_row, nsamp))) return rc;
    const long long S = (long long)nchains * nsamp;
    if (k_lo < 1 || k_lo > S || k_hi < 1 || k_hi > S) return fail(BNR_ERR_BAD_ARG, "order statistics must be between 1 and nchains * nsamp");
    x_source xs;
    xs.X = X; xs.dtype = x_dtype;
    dev_tmp tmp;
    double *Xd = nullptr, *yd = nullptr;
    result_slab out, lc;
    if ((rc = stage_new_rows(chains, nchains, m, xs, y, tmp, &Xd, &yd))) return rc;
    hipStream_t st = chains[0]->x.stream;
    const int m_pad = round_up(m, 32);
    if ((rc = out.alloc(tmp, 5, (size_t)m, st))) return rc;
    pred_stages sg;
    sg.k_lo = k_lo; sg.k_hi = k_hi;
    sg.wt = &wt;
    sg.mean = out.col(0); sg.lower = out.col(1); sg.upper = out.col(2);
    if (y) {
        if ((rc = lc.alloc(tmp, nchains + 1, (size_t)m, st))) return rc;        // every chain's lpd; the last column takes the pwaic nobody reads
        // every chain's own lpd: bnr_chain_predict's launches over that chain alone, on its stream (the inputs are complete first), so column k
        // is its lpd bit for bit; the work buffers of a chain go before the next one's come
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < nchains; ++k) {
            bnr_chain *ck = chains[k];
            dev_tmp tk;
            pred_stages sk;
            sk.lpd = lc.col(k); sk.pwaic = lc.col(nchains);
            if ((rc = predict_rows(&ck, 1, first_row, nsamp, m, Xd, m_pad, yd, sk, tk))) return rc;
            HIPCHK(hipStreamSynchronize(ck->x.stream));
        }
    }
    if (pred_lower) { sg.seed = pred_seed; sg.pred_lower = out.col(3); sg.pred_upper = out.col(4); }
    if ((rc = predict_rows(chains, nchains, first_row, nsamp, m, Xd, m_pad, nullptr, sg, tmp))) return rc;
    std::vector<double> hl;
    if (y) {
        hl.resize((size_t)nchains * m);
        HIPCHK(hipMemcpyAsync(hl.data(), lc.d, sizeof(double) * hl.size(), hipMemcpyDeviceToHost, st));
    }
    if ((rc = out.fetch(st, "wpredict", "k_wsummary", {mean, lower, upper, pred_lower, pred_lower ? pred_upper : nullptr}))) return rc;
    if (y) for (int i = 0; i < m; ++i) lpd[i] = wlse(hl.data() + i, (size_t)m, weights, nchains);
    return BNR_OK;
}

// ------------------------------------------------------------------------------------------ posterior covariance of the edge coefficients (ABI 17): include/bnr_hip.h
// The draws of a covariance call: chain k's window is nsamp rows of rowlen doubles from rows[k] (a trace's first window row at o_gamma, or row
// k nsamp of a caller's matrix); `cols` (host, ncols entries, checked) picks the columns.
// 1. the centres: the chosen columns staged as stage_cols stages them (k_fetch_cols, one launch per chain and run of consecutive columns; blocks
//    of about 1 GiB of draws, or `blk_set` columns) and k_summary's mean of each -- with wt k_wsummary's -- so that the centre IS the mean the
//    Summary calls report, bit for bit.  The staging buffer goes before the Grams come.
// 2. per pair of column blocks I <= J (Bc columns each: `blk_set`, or the largest multiple of 128 whose nc Bc^2 doubles stay within 1 GiB) one
//    k_cov for all chains (blockIdx.z = chain), each into its Bc x Bc slice of G, then k_cov_finish: the chains' Grams added in order, divided, mirrored into covd.
// An entry's sums are fixed by (nc, nsamp): the blocks and the tile shape (TW = 4 where the call has 128 x 128 tiles enough to fill the chip, 2
// below) only move it to another workgroup.
static int cov_run(hipStream_t st, const std::vector<const double *> &rows, long long rowlen, int nsamp, int ncols, const int32_t *cols,
                   const bnr_wsum_weights *wt, int blk_set, double *mean, double *cov)
{
    const int nc = (int)rows.size();
    const long long S = (long long)nc * nsamp;
    if (nc > 65535) return fail(BNR_ERR_BAD_ARG, "more than 65535 chains");        // (the chains are k_cov's grid.z)
    int rc;
    dev_tmp tmp;
    int *colsd = nullptr;
    double *cen = nullptr, *covd = nullptr, *G = nullptr, *wd = nullptr;
    const double **rowsd = nullptr;
    if ((rc = tmp.alloc(&colsd, (size_t)ncols, st, false)) || (rc = tmp.alloc(&cen, (size_t)ncols, st))) return rc;
    HIPCHK(hipMemcpyAsync(colsd, cols, sizeof(int) * (size_t)ncols, hipMemcpyHostToDevice, st));
    if ((rc = tmp.alloc(&rowsd, (size_t)nc, st, false))) return rc;
    HIPCHK(hipMemcpyAsync(rowsd, rows.data(), sizeof(double *) * (size_t)nc, hipMemcpyHostToDevice, st));
    if (wt) {
        if ((rc = tmp.alloc(&wd, (size_t)BNR_STACK_MAX_CHAINS, st, false))) return rc;
        HIPCHK(hipMemcpyAsync(wd, wt->w, sizeof(double) * BNR_STACK_MAX_CHAINS, hipMemcpyHostToDevice, st));
    }
    {
        dev_tmp stage;                                  // (freed at the end of this block: hipFree waits for the device)
        double *buf = nullptr;
        const int sblk = block_cols(S, blk_set, ncols);
        if ((rc = stage.alloc(&buf, (size_t)sblk * (size_t)S, st, false))) return rc;
        for (int p0 = 0; p0 < ncols; p0 += sblk) {
            const int pc = std::min(sblk, ncols - p0);
            for (int p = 0; p < pc;) {
                int run = 1;
                while (p + run < pc && cols[p0 + p + run] == cols[p0 + p] + run) ++run;
                for (int k = 0; k < nc; ++k)
                    launch_fetch_cols(st, rows[k], (int)rowlen, cols[p0 + p], run, 0, nsamp, buf + (size_t)p * (size_t)S + (size_t)k * nsamp, S);
                p += run;
            }
            if (wt) launch_wsummary(st, pc, buf, S, nsamp, nc, *wt, 0, 1, 1, cen + p0, nullptr, nullptr);
            else launch_summary(st, pc, buf, (int)S, 0, 1, 1, cen + p0, nullptr, nullptr);
        }
        HIPCHK(hipStreamSynchronize(st));
        if ((rc = check_launch("k_summary"))) return rc;
    }
    int Bc = blk_set > 0 ? blk_set : std::max(128, (int)sqrt((double)((size_t)1 << 27) / nc) / 128 * 128);
    Bc = std::min(Bc, ncols);
    const long long t128 = ((long long)ncols + 127) / 128;
    const bool big = t128 * (t128 + 1) / 2 * nc >= 512;
    const int wg = big ? 128 : 64;                      // the columns of a workgroup's tile: 2 x 2 waves of 16 TW each
    const size_t gstride = (size_t)Bc * (size_t)Bc;
    if ((rc = tmp.alloc(&G, gstride * (size_t)nc, st, false)) || (rc = tmp.alloc(&covd, (size_t)ncols * (size_t)ncols, st, false))) return rc;
    const double denom = wt ? (double)nsamp : (double)(S - 1);
    for (int a0 = 0; a0 < ncols; a0 += Bc)
        for (int b0 = a0; b0 < ncols; b0 += Bc) {
            const int na = std::min(Bc, ncols - a0), nb = std::min(Bc, ncols - b0);
            const dim3 grid((nb + wg - 1) / wg, (na + wg - 1) / wg, nc);
            if (big)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov<4>), grid, dim3(256), 0, st, (const double *const *)rowsd, rowlen, nsamp, (const int *)colsd,
                                   (const double *)cen, a0, na, b0, nb, G, (long long)gstride, Bc);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov<2>), grid, dim3(256), 0, st, (const double *const *)rowsd, rowlen, nsamp, (const int *)colsd,
                                   (const double *)cen, a0, na, b0, nb, G, (long long)gstride, Bc);
            hipLaunchKernelGGL(k_cov_finish, dim3((nb + 63) / 64, (na + 3) / 4), dim3(256), 0, st, (const double *)G, (long long)gstride, Bc, nc,
                               (const double *)wd, denom, (const double *)cen, a0, na, b0, nb, covd, ncols);
        }
    HIPCHK(hipMemcpyAsync(mean, cen, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost, st));
    hipError_t e = hipMemcpyAsync(cov, covd, sizeof(double) * (size_t)ncols * (size_t)ncols, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string("cov: ") + hipGetErrorString(e));
    return check_launch("k_cov");
}
// the column list of a covariance call over q columns as cov_run takes it: cols as given (every index in 0 .. q - 1), or 0 .. q - 1 for NULL
static int cov_cols(int32_t ncols, const int32_t *cols, int q, std::vector<int32_t> &out)
{
    if (ncols < 1) return fail(BNR_ERR_BAD_ARG, "need ncols >= 1 columns");
    if (!cols && ncols != q) return fail(BNR_ERR_BAD_ARG, "cols == NULL means every column: ncols must be " + std::to_string(q));
    out.resize(ncols);
    for (int p = 0; p < ncols; ++p) {
        out[p] = cols ? cols[p] : p;
        if (out[p] < 0 || out[p] >= q) return fail(BNR_ERR_BAD_ARG, "column index outside 0 .. " + std::to_string(q - 1));
    }
    return BNR_OK;
}
int bnr_chain_cov(bnr_chain *c, int32_t first_row, int32_t nsamp, int32_t ncols, const int32_t *cols, double *mean, double *cov)
{
    if (!c) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    return bnr_chains_cov(&c, 1, nullptr, first_row, nsamp, ncols, cols, mean, cov);
}
int bnr_chains_cov(bnr_chain *const *chains, int32_t nchains, const double *weights, int32_t first_row, int32_t nsamp, int32_t ncols,
                   const int32_t *cols, double *mean, double *cov)
{
    if (!chains || !mean || !cov) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    int rc;
    bnr_wsum_weights wt;
    if (weights && (rc = wsum_pack(weights, nchains, wt))) return rc;
    if ((rc = pooled_check(chains, nchains, first_row, nsamp))) return rc;
    if ((long long)nchains * nsamp < 2) return fail(BNR_ERR_BAD_ARG, "a covariance needs nchains * nsamp >= 2 draws");
    bnr_chain *c = chains[0];
    std::vector<int32_t> hc;
    if ((rc = cov_cols(ncols, cols, c->d.q, hc))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = pooled_quiesce(chains, nchains))) return rc;
    std::vector<const double *> rows(nchains);
    for (int k = 0; k < nchains; ++k) {
        const bnr_dev &dk = chains[k]->d;
        if (dk.rowlen != c->d.rowlen) return fail(BNR_ERR_BAD_ARG, "pooled chains must have equal trace rows");
        rows[k] = dk.trace + (size_t)(first_row - 1) * dk.rowlen + dk.o_gamma;
    }
    return cov_run(c->x.stream, rows, c->d.rowlen, nsamp, ncols, hc.data(), weights ? &wt : nullptr, c->cov_block_cols, mean, cov);
}
// the same on a caller's (K nsamp) x m matrix (host, row-major: draws x columns, chain k's draws in rows k nsamp ..): k_cov's direct test, and
// the covariance of any set of draws.  The matrix is uploaded whole, on a stream of the call's own.
int bnr_cov(int32_t device, int32_t K, int32_t nsamp, int32_t m, const double *x, const double *weights, double *mean, double *cov)
{
    if (!x || !mean || !cov) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (K < 1 || nsamp < 1 || m < 1) return fail(BNR_ERR_BAD_ARG, "need K >= 1 chains, nsamp >= 1 draws per chain and m >= 1 columns");
    int rc;
    bnr_wsum_weights wt;
    if (weights && (rc = wsum_pack(weights, K, wt))) return rc;
    const long long S = (long long)K * nsamp;
    if (S > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    if (S < 2) return fail(BNR_ERR_BAD_ARG, "a covariance needs K * nsamp >= 2 draws");
    std::vector<int32_t> hc;
    if ((rc = cov_cols(m, nullptr, m, hc))) return rc;
    stream_guard guard;
    if ((rc = guard.open(device))) return rc;
    hipStream_t st = guard.s;
    dev_tmp tmp;                                        // (freed before the stream goes)
    double *Xd = nullptr;
    if ((rc = tmp.alloc(&Xd, (size_t)S * (size_t)m, st, false))) return rc;
    HIPCHK(hipMemcpyAsync(Xd, x, sizeof(double) * (size_t)S * (size_t)m, hipMemcpyHostToDevice, st));
    std::vector<const double *> rows(K);
    for (int k = 0; k < K; ++k) rows[k] = Xd + (size_t)k * nsamp * (size_t)m;
    return cov_run(st, rows, m, nsamp, m, hc.data(), weights ? &wt : nullptr, 0, mean, cov);
}

// ------------------------------------------------------------------------------------------ the device side of a chain (ABI 18): include/bnr_hip.h
// What a companion library (libbnr_mloo.so) needs to read a chain's table in place: sizes, row offsets and device pointers, after everything the
// chain's stream and its group's still hold has finished.  A pending asynchronous run stays pending for bnr_chain_sync.  Host code only.
int bnr_chain_device_view(bnr_chain *c, bnr_chain_view *out)
{
    if (!c || !out) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->x.stream));
    if (c->group) HIPCHK(hipStreamSynchronize(c->group->x.stream));
    const bnr_dev &d = c->d;
    out->device = c->device;
    out->n = d.n; out->n_pad = d.n_pad; out->V = d.V; out->R = d.R; out->q = d.q; out->q_pad = d.q_pad; out->tot = d.tot; out->rowlen = d.rowlen;
    out->o_tau2 = ROW_TAU2; out->o_mu = ROW_MU; out->o_lam = d.o_lam; out->o_u = d.o_u; out->o_gamma = d.o_gamma; out->o_S = d.o_S;
    out->ldx = d.n_pad;
    out->X = d.X; out->y = d.y; out->ek = d.ek; out->el = d.el; out->trace = d.trace;
    return BNR_OK;
}
int bnr_set_last_error(int code, const char *msg) { return fail(code, msg ? msg : ""); }
