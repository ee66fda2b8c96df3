// bnr_mloo_job.h -- the host driver that libbnr_mloo.so (bnr_mloo.hip) and libbnr_medge.so (bnr_medge.hip) share: the device memory and the
// stream of one call (call_guard), what the batches of a call work on (mloo_job) and the batches themselves (run_job) over the kernels of
// bnr_mloo_kernels.h.  Internal: included by those two translation units after the kernels, each into its own library and code object; every
// name here has internal linkage, so each library launches its own copy of the kernels and keeps its own batch option.
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

int round_up(int a, int b) { return (a + b - 1) / b * b; }

// the batches of a call; on return (status OK, stream synchronised) the host vectors hold n x ndraws loglik / resid / var (those wanted), logml and
// the bad flags.  hook (optional): called once per batch, after the batch's k_mloo_factor was enqueued and before the next batch touches G.
int run_job(call_guard &g, mloo_job &job, std::vector<double> &ll, std::vector<double> &resid, std::vector<double> &var, std::vector<double> &logml,
            std::vector<int> &bad, const mloo_hook &hook = nullptr)
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
