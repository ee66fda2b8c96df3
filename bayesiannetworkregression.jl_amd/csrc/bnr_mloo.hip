// bnr_mloo.hip -- libbnr_mloo.so behind include/bnr_mloo.h: marginal PSIS-LOO, the edge coefficients integrated out on the device, over the
// kernels of bnr_mloo_kernels.h.  A library and a gfx950 code object of its own: libbnr_hip.so's two stay what they are.  It reaches a chain
// through bnr_chain_device_view, runs PSIS through bnr_psis_weights and leaves its messages with bnr_set_last_error -- the exported calls of
// libbnr_hip.so, nothing of bnr_internal.h.
#include "../../include/bnr_mloo.h"
#include "bnr_mloo_kernels.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

namespace {
int fail(int code, const std::string &msg) { return bnr_set_last_error(code, msg.c_str()); }
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(BNR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

std::atomic<long long> opt_batch_draws{0};

// the device memory and the stream of one call, released on every path
struct call_guard {
    hipStream_t st = nullptr;
    std::vector<void *> p;
    ~call_guard()
    {
        for (void *q : p) (void)hipFree(q);
        if (st) (void)hipStreamDestroy(st);
    }
    int open(int device)
    {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return fail(BNR_ERR_BAD_ARG, "no such device");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return BNR_OK;
    }
    template <typename T>
    int alloc(T **out, size_t count)
    {
        void *q = nullptr;
        HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
        p.push_back(q);
        *out = (T *)q;
        return BNR_OK;
    }
    template <typename T>
    int upload(T **out, const T *src, size_t count)
    {
        int rc = alloc(out, count);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(*out, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        return BNR_OK;
    }
};

// What the batches of a call work on.  X, y on the device; per draw s of the call tau2[s], mu[s] and the pointer Sp[s] to its q values of S.
// Chain form: rowp[s] = the table row of draw s (W, tau2, mu come from it by k_mloo_w).  Raw form: the caller's S and W, uploaded batch by batch
// into Sbuf / Wbuf (Sp[s] points into Sbuf at s % B).
struct mloo_job {
    int n = 0, q = 0, ndraws = 0, ldx = 0;
    const double *X = nullptr, *y = nullptr;
    bnr_chain_view v{};                                 // chain form
    const double *const *rowp = nullptr;                // chain form: device array of ndraws row pointers
    const double *const *hrow = nullptr;                // ... and the same on the host
    const double *hS = nullptr, *hW = nullptr;          // raw form: host S, W
    bool chain_form = false, has_w = false;
    double *tau2 = nullptr, *mu = nullptr;              // ndraws each (raw form: uploaded; chain form: written by k_mloo_w)
    bool want_ll = false, want_resid = false, want_var = false;
};

int round_up(int a, int b) { return (a + b - 1) / b * b; }

// the batches of a call; on return (status OK, stream synchronised) the host vectors hold n x ndraws loglik / resid / var (those wanted), logml and
// the bad flags
int run_job(call_guard &g, mloo_job &job, std::vector<double> &ll, std::vector<double> &resid, std::vector<double> &var, std::vector<double> &logml,
            std::vector<int> &bad)
{
    const int n = job.n, q = job.q, D = job.ndraws, np = round_up(n, MLOO_TILE);
    const size_t mat = (size_t)np * (size_t)(np + 1);   // a draw's L and, above it, L^-1 (k_mloo_factor)
    long long B = opt_batch_draws.load();
    if (B <= 0) B = (long long)(((size_t)1 << 30) / (mat * sizeof(double)));
    B = std::max<long long>(1, std::min<long long>(std::min<long long>(B, D), 32768));
    int rc;
    double *G = nullptr, *r = nullptr, *Wbuf = nullptr, *Sbuf = nullptr, *d_ll = nullptr, *d_resid = nullptr, *d_var = nullptr, *d_logml = nullptr;
    int *d_bad = nullptr;
    const double **Sp = nullptr;
    if ((rc = g.alloc(&G, (size_t)B * mat))) return rc;
    if ((rc = g.alloc(&r, (size_t)B * np))) return rc;
    if (job.has_w && (rc = g.alloc(&Wbuf, (size_t)B * q))) return rc;
    const size_t nout = (size_t)n * (size_t)D;
    if (job.want_ll && (rc = g.alloc(&d_ll, nout))) return rc;
    if (job.want_resid && (rc = g.alloc(&d_resid, nout))) return rc;
    if (job.want_var && (rc = g.alloc(&d_var, nout))) return rc;
    if ((rc = g.alloc(&d_logml, (size_t)D))) return rc;
    if ((rc = g.alloc(&d_bad, (size_t)D))) return rc;
    std::vector<const double *> hSp(D);                 // (lives until the stream is synchronised below)
    if (job.chain_form) {
        for (int s = 0; s < D; ++s) hSp[s] = job.hrow[s] + job.v.o_S;
    } else {
        if ((rc = g.alloc(&Sbuf, (size_t)B * q))) return rc;
        for (int s = 0; s < D; ++s) hSp[s] = Sbuf + (size_t)(s % B) * (size_t)q;
    }
    if ((rc = g.upload(&Sp, hSp.data(), (size_t)D))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    const int nt = np / MLOO_TILE;
    for (int s0 = 0; s0 < D; s0 += (int)B) {
        const int nb = std::min<int>((int)B, D - s0);
        if (job.chain_form) {
            hipLaunchKernelGGL(k_mloo_w, dim3((q + 255) / 256, nb), dim3(256), 0, g.st, job.rowp + s0, job.v.o_tau2, job.v.o_mu, job.v.o_lam, job.v.o_u,
                               job.v.R, q, job.v.ek, job.v.el, Wbuf, job.tau2 + s0, job.mu + s0);
        } else {
            HIPCHK(hipMemcpyAsync(Sbuf, job.hS + (size_t)s0 * q, sizeof(double) * (size_t)nb * q, hipMemcpyHostToDevice, g.st));
            if (job.has_w) HIPCHK(hipMemcpyAsync(Wbuf, job.hW + (size_t)s0 * q, sizeof(double) * (size_t)nb * q, hipMemcpyHostToDevice, g.st));
        }
        hipLaunchKernelGGL(k_mloo_rhs, dim3((np + 255) / 256, (nb + MLOO_RB - 1) / MLOO_RB), dim3(256), 0, g.st, job.X, job.ldx, job.y, n, np, q,
                           (const double *)Wbuf, (const double *)(job.mu + s0), nb, r);
        hipLaunchKernelGGL(k_mloo_gram, dim3(nt * (nt + 1) / 2, (nb + MLOO_DB - 1) / MLOO_DB), dim3(256), 0, g.st, job.X, job.ldx, n, q,
                           (const double *const *)(Sp + s0), nb, G, np, (long long)mat);
        hipLaunchKernelGGL(k_mloo_factor, dim3(nb), dim3(256), 0, g.st, G, (long long)mat, (const double *)r, n, np, q, (const double *const *)(Sp + s0),
                           (const double *)(job.tau2 + s0), (const double *)(job.mu + s0), s0, (long long)D, d_ll, d_resid, d_var, d_logml, d_bad);
        HIPCHK(hipGetLastError());
        if (!job.chain_form) HIPCHK(hipStreamSynchronize(g.st));   // (the next batch's uploads overwrite Sbuf / Wbuf: a pageable source may be staged at once)
    }
    logml.resize(D); bad.resize(D);
    if (job.want_ll) { ll.resize(nout); HIPCHK(hipMemcpyAsync(ll.data(), d_ll, sizeof(double) * nout, hipMemcpyDeviceToHost, g.st)); }
    if (job.want_resid) { resid.resize(nout); HIPCHK(hipMemcpyAsync(resid.data(), d_resid, sizeof(double) * nout, hipMemcpyDeviceToHost, g.st)); }
    if (job.want_var) { var.resize(nout); HIPCHK(hipMemcpyAsync(var.data(), d_var, sizeof(double) * nout, hipMemcpyDeviceToHost, g.st)); }
    HIPCHK(hipMemcpyAsync(logml.data(), d_logml, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipMemcpyAsync(bad.data(), d_bad, sizeof(int) * (size_t)D, hipMemcpyDeviceToHost, g.st));
    HIPCHK(hipStreamSynchronize(g.st));
    HIPCHK(hipGetLastError());
    return BNR_OK;
}
}   // namespace

int bnr_mloo_abi_version(void) { return BNR_MLOO_ABI_VERSION; }

int bnr_mloo_set_option(const char *name, int64_t value)
{
    if (!name) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (std::string(name) == "mloo_batch_draws") {
        if (value < 0) return fail(BNR_ERR_BAD_ARG, "mloo_batch_draws must be >= 0");
        opt_batch_draws.store(value);
        return BNR_OK;
    }
    return fail(BNR_ERR_BAD_ARG, std::string("unknown option ") + name);
}

int bnr_marginal_loglik(int32_t device, int32_t n, int32_t q, int32_t ndraws, const double *X, const double *y, const double *tau2, const double *mu,
                        const double *S, const double *W, double *loglik, double *resid, double *var, double *logml, int32_t *n_bad)
{
    if (!X || !y || !tau2 || !mu || !S) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (!loglik && !resid && !var) return fail(BNR_ERR_BAD_ARG, "ask for loglik, resid or var");
    if (n < 1 || q < 1 || ndraws < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows, q >= 1 edges and ndraws >= 1 draws");
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    int rc;
    if ((rc = g.open(device))) return rc;
    mloo_job job;
    job.n = n; job.q = q; job.ndraws = ndraws; job.ldx = n;
    double *Xd = nullptr, *yd = nullptr;
    if ((rc = g.upload(&Xd, X, (size_t)n * (size_t)q))) return rc;
    if ((rc = g.upload(&yd, y, (size_t)n))) return rc;
    if ((rc = g.upload(&job.tau2, tau2, (size_t)ndraws))) return rc;
    if ((rc = g.upload(&job.mu, mu, (size_t)ndraws))) return rc;
    job.X = Xd; job.y = yd; job.hS = S; job.hW = W; job.has_w = W != nullptr;
    job.want_ll = loglik != nullptr; job.want_resid = resid != nullptr; job.want_var = var != nullptr;
    std::vector<double> ll, rs, vr, lm;
    std::vector<int> bad;
    if ((rc = run_job(g, job, ll, rs, vr, lm, bad))) return rc;
    const size_t nout = (size_t)n * (size_t)ndraws;
    if (loglik) std::copy(ll.begin(), ll.begin() + nout, loglik);
    if (resid) std::copy(rs.begin(), rs.begin() + nout, resid);
    if (var) std::copy(vr.begin(), vr.begin() + nout, var);
    if (logml) std::copy(lm.begin(), lm.end(), logml);
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
    return BNR_OK;
}

int bnr_chains_marginal_loo(bnr_chain *const *chains, int32_t nchains, int32_t first_row, int32_t nsamp, int32_t thin, const double *r_eff,
                            double *elpd_loo, double *pareto_k, double *loo_mean, double *loo_sd, double *logml, double *loglik, int32_t *n_bad)
{
    if (!chains || !elpd_loo || !pareto_k) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    if (nchains < 1) return fail(BNR_ERR_BAD_ARG, "need nchains >= 1");
    if (thin < 1) return fail(BNR_ERR_BAD_ARG, "need thin >= 1");
    for (int i = 0; i < nchains; ++i) {
        if (!chains[i]) return fail(BNR_ERR_BAD_ARG, "NULL chain");
        for (int k = 0; k < i; ++k) if (chains[k] == chains[i]) return fail(BNR_ERR_BAD_ARG, "chain listed twice");
    }
    std::vector<bnr_chain_view> v(nchains);
    int rc;
    for (int i = 0; i < nchains; ++i) {
        if ((rc = bnr_chain_device_view(chains[i], &v[i]))) return rc;
        if (v[i].device != v[0].device || v[i].n != v[0].n || v[i].V != v[0].V || v[i].R != v[0].R || v[i].rowlen != v[0].rowlen)
            return fail(BNR_ERR_BAD_ARG, "pooled chains must live on one device and have equal n, V, R");
    }
    for (int i = 0; i < nchains; ++i)
        if (first_row < 1 || nsamp < 1 || (long long)first_row + nsamp - 1 > v[i].tot) return fail(BNR_ERR_BAD_ARG, "row window outside the table");
    const int nd = (nsamp + thin - 1) / thin;
    if ((long long)nchains * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    const int n = v[0].n, D = nchains * nd;
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    call_guard g;
    if ((rc = g.open(v[0].device))) return rc;
    mloo_job job;
    job.n = n; job.q = v[0].q; job.ndraws = D; job.ldx = v[0].ldx; job.X = v[0].X; job.y = v[0].y; job.v = v[0];
    job.chain_form = true; job.has_w = true;
    job.want_ll = true; job.want_resid = loo_mean || loo_sd; job.want_var = loo_sd != nullptr;
    std::vector<const double *> hrow(D);
    for (int k = 0; k < nchains; ++k)
        for (int j = 0; j < nd; ++j) hrow[(size_t)k * nd + j] = v[k].trace + ((size_t)(first_row - 1) + (size_t)j * thin) * (size_t)v[k].rowlen;
    const double **rowp = nullptr;
    if ((rc = g.upload(&rowp, hrow.data(), (size_t)D))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    job.rowp = rowp; job.hrow = hrow.data();
    if ((rc = g.alloc(&job.tau2, (size_t)D))) return rc;
    if ((rc = g.alloc(&job.mu, (size_t)D))) return rc;
    std::vector<double> ll, rs, vr, lm, yh(n);
    std::vector<int> bad;
    if ((rc = run_job(g, job, ll, rs, vr, lm, bad))) return rc;
    HIPCHK(hipMemcpy(yh.data(), v[0].y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<double> lw((size_t)n * (size_t)D);
    if ((rc = bnr_psis_weights(v[0].device, n, D, ll.data(), r_eff, lw.data(), elpd_loo, pareto_k))) return rc;
    if (loo_mean || loo_sd) {
        for (int i = 0; i < n; ++i) {
            const double *w = lw.data() + (size_t)i * D, *ri = rs.data() + (size_t)i * D, *vi = loo_sd ? vr.data() + (size_t)i * D : nullptr;
            double a = 0.0, b = 0.0;
            for (int s = 0; s < D; ++s) {
                const double ws = std::exp(w[s]);
                a = a + ws * ri[s];
                if (vi) { const double ms = yh[i] - ri[s]; b = b + ws * (vi[s] + ms * ms); }
            }
            const double mean = yh[i] - a;
            if (loo_mean) loo_mean[i] = mean;
            if (loo_sd) loo_sd[i] = std::sqrt(b - mean * mean);
        }
    }
    if (logml) std::copy(lm.begin(), lm.end(), logml);
    if (loglik) std::copy(ll.begin(), ll.end(), loglik);
    if (n_bad) { int nb = 0; for (int f : bad) nb += f != 0; *n_bad = nb; }
    return BNR_OK;
}
