// bnr_mloo_job.h -- the host driver that the six marginal libraries (bnr_mloo.hip, bnr_medge.hip, bnr_mpred.hip, bnr_mcheck.hip, bnr_mstack.hip,
// bnr_mcov.hip) share: the device memory and the stream of one call (call_guard), what the batches of a call work on (mloo_job), how an entry
// point fills it in from its arguments (check_chain_list and open_chain_job for the chain form, open_raw_job for the raw form), the batches
// themselves (run_job) over the kernels of bnr_mloo_kernels.h, and the checks that several of them make: the library's batch option
// (set_batch_draws), the chain weights (weight_check) and the half-width of a quantile's bracket (bracket_halfwidth).  Internal: included by
// those translation units after the kernels, each into its own library and code object; every name here has internal linkage, so each library
// launches its own copy of the kernels and keeps its own batch option.
#pragma once
#include "../../include/bnr_mloo.h"
#include "bnr_mloo_kernels.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>
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

std::atomic<long long> opt_batch_draws{0};              // the library's "*_batch_draws" option (0: automatic)

// bnr_<prefix>_set_option for the option every marginal library has, "<prefix>_batch_draws" (>= 0); any other name is unknown
int set_batch_draws(const char *prefix, const char *name, int64_t value)
{
    if (!name) return fail(BNR_ERR_BAD_ARG, "NULL argument");
    const std::string option = std::string(prefix) + "_batch_draws";
    if (option != name) return fail(BNR_ERR_BAD_ARG, std::string("unknown option ") + name);
    if (value < 0) return fail(BNR_ERR_BAD_ARG, option + " must be >= 0");
    opt_batch_draws.store(value);
    return BNR_OK;
}

// the refusal of the chain weights w[K] of a call, bnr_chains_wsummary's checks (finite, >= 0, one > 0, |sum - 1| <= 1e-9), or NULL
const char *weight_check(const double *w, int K)
{
    double s = 0.0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(w[k]) || w[k] < 0.0) return "weights must be finite and >= 0";
        any = any || w[k] > 0.0;
        s += w[k];
    }
    if (!any) return "at least one weight must be > 0";
    if (!(std::fabs(s - 1.0) <= 1e-9)) return "weights must sum to 1 (within 1e-9)";
    return nullptr;
}

// the half-width c, in sds of a component, of the bracket a mixture's p_lo and p_hi quantiles are searched in (0 < p_lo < p_hi < 1): the first of
// 1, 1.5, .. 40 with Phi(-c) < min(p_lo, 1 - p_hi) / 2
double bracket_halfwidth(double p_lo, double p_hi)
{
    const double pm = 0.5 * std::min(p_lo, 1.0 - p_hi);
    double c = 1.0;
    while (!(0.5 * std::erfc(c * 0.70710678118654752440) < pm) && c < 40.0) c += 0.5;
    return c;
}

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
    // count values to the host, finished when this returns; a NULL out asks for nothing
    template <typename T>
    int fetch(T *out, const T *dev, size_t count)
    {
        if (!out) return BNR_OK;
        HIPCHK(hipMemcpyAsync(out, dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return BNR_OK;
    }
};

// What the batches of a call work on.  X, y on the device; per draw s of the call tau2[s], mu[s] and the pointer Sp[s] to its q values of S.
// Chain form: rowp[s] = the table row of draw s (W, tau2, mu come from it by k_mloo_w).  Raw form: the caller's S and W, uploaded batch by batch
// into Sbuf / Wbuf (Sp[s] points into Sbuf at s % B).
struct mloo_job {
    int n = 0, q = 0, ndraws = 0, ldx = 0;
    const double *X = nullptr, *y = nullptr;
    bnr_chain_view v{};                                 // chain form: the first chain's view (its device, y, offsets and edge lists serve all)
    const double *const *rowp = nullptr;                // chain form: device array of ndraws row pointers
    std::vector<const double *> hrow;                   // ... and the same on the host
    const double *hS = nullptr, *hW = nullptr;          // raw form: host S, W
    bool chain_form = false, has_w = false;
    double *tau2 = nullptr, *mu = nullptr;              // ndraws each (raw form: uploaded; chain form: written by k_mloo_w)
    bool want_ll = false, want_resid = false, want_var = false;
};

// The checks of a chain-form call that need no chain: the counts and the list.  also: a refusal of the caller's own that ranks between the two
// (NULL: none).
int check_chain_list(bnr_chain *const *chains, int nchains, int thin, const char *also = nullptr)
{
    if (nchains < 1) return fail(BNR_ERR_BAD_ARG, "need nchains >= 1");
    if (thin < 1) return fail(BNR_ERR_BAD_ARG, "need thin >= 1");
    if (also) return fail(BNR_ERR_BAD_ARG, also);
    for (int i = 0; i < nchains; ++i) {
        if (!chains[i]) return fail(BNR_ERR_BAD_ARG, "NULL chain");
        for (int k = 0; k < i; ++k) if (chains[k] == chains[i]) return fail(BNR_ERR_BAD_ARG, "chain listed twice");
    }
    return BNR_OK;
}

// The job of a chain-form call over rows first_row + j thin, j = 0 .. nd - 1, of every chain of a checked list (draw k nd + j: chain k's j-th), and
// the call's device and stream: the chains' views and what they must share, the window, the row pointers on both sides, tau2 and mu allocated.
int open_chain_job(call_guard &g, mloo_job &job, bnr_chain *const *chains, int nchains, int first_row, int nsamp, int thin, int &nd)
{
    std::vector<bnr_chain_view> v(nchains);
    int rc;
    for (int i = 0; i < nchains; ++i) {
        if ((rc = bnr_chain_device_view(chains[i], &v[i]))) return rc;
        if (v[i].device != v[0].device || v[i].n != v[0].n || v[i].V != v[0].V || v[i].R != v[0].R || v[i].rowlen != v[0].rowlen)
            return fail(BNR_ERR_BAD_ARG, "pooled chains must live on one device and have equal n, V, R");
    }
    for (int i = 0; i < nchains; ++i)
        if (first_row < 1 || nsamp < 1 || (long long)first_row + nsamp - 1 > v[i].tot) return fail(BNR_ERR_BAD_ARG, "row window outside the table");
    nd = (nsamp + thin - 1) / thin;
    if ((long long)nchains * nd > 0x7FFFFFFFll) return fail(BNR_ERR_BAD_ARG, "more than 2^31 - 1 pooled draws");
    const int D = nchains * nd;
    if (v[0].n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    if ((rc = g.open(v[0].device))) return rc;
    job.n = v[0].n; job.q = v[0].q; job.ndraws = D; job.ldx = v[0].ldx; job.X = v[0].X; job.y = v[0].y; job.v = v[0];
    job.chain_form = true; job.has_w = true;
    job.hrow.resize(D);
    for (int k = 0; k < nchains; ++k)
        for (int j = 0; j < nd; ++j) job.hrow[(size_t)k * nd + j] = v[k].trace + ((size_t)(first_row - 1) + (size_t)j * thin) * (size_t)v[k].rowlen;
    const double **rowp = nullptr;
    if ((rc = g.upload(&rowp, job.hrow.data(), (size_t)D))) return rc;
    HIPCHK(hipStreamSynchronize(g.st));
    job.rowp = rowp;
    if ((rc = g.alloc(&job.tau2, (size_t)D))) return rc;
    return g.alloc(&job.mu, (size_t)D);
}

// The job of a raw-form call and the call's device and stream: the checks of the shapes (also: a refusal of the caller's own that ranks between
// them, NULL: none), X, y, tau2 and mu uploaded, S and W left to the batches.
int open_raw_job(call_guard &g, mloo_job &job, int device, int n, int q, int ndraws, const double *X, const double *y, const double *tau2,
                 const double *mu, const double *S, const double *W, const char *also = nullptr)
{
    if (n < 1 || q < 1 || ndraws < 1) return fail(BNR_ERR_BAD_ARG, "need n >= 1 rows, q >= 1 edges and ndraws >= 1 draws");
    if (also) return fail(BNR_ERR_BAD_ARG, also);
    if (n > BNR_MLOO_MAX_N) return fail(BNR_ERR_BAD_ARG, "n > 2048 is not supported by this version");
    int rc;
    if ((rc = g.open(device))) return rc;
    job.n = n; job.q = q; job.ndraws = ndraws; job.ldx = n;
    double *Xd = nullptr, *yd = nullptr;
    if ((rc = g.upload(&Xd, X, (size_t)n * (size_t)q))) return rc;
    if ((rc = g.upload(&yd, y, (size_t)n))) return rc;
    if ((rc = g.upload(&job.tau2, tau2, (size_t)ndraws))) return rc;
    if ((rc = g.upload(&job.mu, mu, (size_t)ndraws))) return rc;
    job.X = Xd; job.y = yd; job.hS = S; job.hW = W; job.has_w = W != nullptr;
    return BNR_OK;
}

// What a per-batch hook of run_job sees, everything on the device and in order on the call's stream behind the batch's k_mloo_factor: the draws
// s0 .. s0 + nb - 1 of the call; G, draw b's L and L^-1 at G + b mat (np (np + 1) doubles, k_mloo_factor's layout); tau2, mu and Sp of draw
// b at index b; Wbuf (nb x q, NULL without W); resid / var (n x ndraws, draw s in column s; NULL unless wanted) and the bad flags (index s).
struct mloo_batch {
    int s0 = 0, nb = 0, np = 0;
    const double *G = nullptr;
    size_t mat = 0;
    const double *tau2 = nullptr, *mu = nullptr;
    const double *const *Sp = nullptr;
    const double *Wbuf = nullptr, *resid = nullptr, *var = nullptr;
    const int *bad = nullptr;
};
using mloo_hook = std::function<int(const mloo_batch &)>;

// What run_job leaves: on the device (the call_guard's) n x ndraws loglik / resid / var (those wanted, else NULL) and logml (ndraws); on the host
// the bad flags.
struct mloo_out {
    const double *loglik = nullptr, *resid = nullptr, *var = nullptr, *logml = nullptr;
    std::vector<int> bad;
};
int count_bad(const std::vector<int> &bad)
{
    int nb = 0;
    for (int f : bad) nb += f != 0;
    return nb;
}

int round_up(int a, int b) { return (a + b - 1) / b * b; }

// the batches of a call; on return (status OK, stream synchronised) out is filled in.  hook (optional): called once per batch, after the batch's
// k_mloo_factor was enqueued and before the next batch touches G.
int run_job(call_guard &g, mloo_job &job, mloo_out &out, const mloo_hook &hook = nullptr)
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
        if (hook) {
            mloo_batch bt;
            bt.s0 = s0; bt.nb = nb; bt.np = np; bt.G = G; bt.mat = mat; bt.tau2 = job.tau2 + s0; bt.mu = job.mu + s0; bt.Sp = Sp + s0;
            bt.Wbuf = Wbuf; bt.resid = d_resid; bt.var = d_var; bt.bad = d_bad;
            if ((rc = hook(bt))) return rc;
        }
        if (!job.chain_form) HIPCHK(hipStreamSynchronize(g.st));   // (the next batch's uploads overwrite Sbuf / Wbuf: a pageable source may be staged at once)
    }
    out.loglik = d_ll; out.resid = d_resid; out.var = d_var; out.logml = d_logml;
    out.bad.resize(D);
    if ((rc = g.fetch(out.bad.data(), (const int *)d_bad, (size_t)D))) return rc;
    HIPCHK(hipGetLastError());
    return BNR_OK;
}
}   // namespace
