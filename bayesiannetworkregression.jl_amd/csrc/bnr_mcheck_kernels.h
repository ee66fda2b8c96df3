// bnr_mcheck_kernels.h -- the gfx950 kernels of libbnr_mcheck.so (include/bnr_mcheck.h) beside the four of bnr_mloo_kernels.h: the summary of
// one weighted mixture of normals per row,  sum_s w_is N(m_is, var_is),  w_is = exp(lw_is),  over row-major rows x D matrices (a row's D draws
// contiguous).  Three kernels:
//     k_mcheck_stage     w = exp(lw), isd = 1 / sqrt(var) and (chain form) m = y - resid, once per element and call
//     k_mcheck_moments   mean, sd, pit, the bracket of the quantile search and the row's NaN flag, one pass, one workgroup per row
//     k_mcheck_quantile  the p_lo / p_hi quantile of the mixture CDF by bisection, one workgroup per (row, bound)
// A row sum: thread t of the 256 adds the terms of draws t, t + 256, t + 512, ... in that order from 0.0; the 256 partial sums are then added
// in LDS as a tree, partial t taking partial t + 128, then t + 64, 32, 16, 8, 4, 2, 1.  The order is fixed by D alone: no output of a row depends
// on the other rows, the grid, the chunk of rows of a launch, the outputs asked for or the call, bit for bit.  Minima and maxima are exact in any
// order.  Plain C++; no atomics, no dynamic LDS, no scratch.  Compiled with -ffp-contract=off: every product and every sum is rounded on its own.
// Every index into a matrix is formed in 64 bits (rows D may reach 2^31 - 1 elements, 16 GiB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MCHECK_SQRT1_2 0.70710678118654752440
#define MCHECK_MAX_IT 64        // the cap of the bisection; 40 halvings reach 2^-40 of the bracket
#define MCHECK_ROWS_PER_LAUNCH (1 << 20)   // rows per launch of the two row kernels (the host walks the rows in chunks: a grid stays far below 2^32 threads)

// ===================================================================================== k_mcheck_stage
// Per element o of the rows x D matrices (total = rows D, a grid-stride loop in 64 bits; grid = any):
//     Wt[o]  = exp(LW[o]), NaN where LW[o] is not finite (a refused row of bnr_psis_weights, or a caller's -inf / +inf: the row is NaN)
//     Isd[o] = 1 / sqrt(V[o]): +inf for V = 0 (a point mass, and only then), NaN for a NaN or negative V
//     Mo[o]  = y[o / D] - A[o]   (Mo != NULL: the chain form, A = resid; the raw form passes its means as they are and no Mo)
// so that no pass of the bisection evaluates an exp, a sqrt or a division.
__global__ __launch_bounds__(256) void k_mcheck_stage(const double *LW, const double *V, const double *A, const double *y, long long total, int D,
                                                      double *Wt, double *Isd, double *Mo)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long o = (long long)blockIdx.x * 256 + (long long)threadIdx.x; o < total; o += step) {
        const double lw = LW[o];
        Wt[o] = (lw - lw == 0.0) ? exp(lw) : __builtin_nan("");          // (lw - lw is 0 for a finite lw alone)
        Isd[o] = 1.0 / sqrt(V[o]);
        if (Mo) Mo[o] = y[o / D] - A[o];
    }
}

// Phi((t - m) isd) of one component; isd = +inf is the point mass at m: [t >= m]
__device__ __forceinline__ double mcheck_phi(double t, double m, double isd)
{
    const double z = (t - m) * isd;
    return (isd == INFINITY) ? (t >= m ? 1.0 : 0.0) : 0.5 * erfc(z * -MCHECK_SQRT1_2);
}

// ===================================================================================== k_mcheck_moments
// Row i = i0 + blockIdx.x (grid = the rows of the chunk, 256 threads) over M, V, Wt, Isd (rows x D) and y (NULL: none):
//     with y:     r_s = y_i - m_s,   mean = y_i - sum_s w_s r_s,   pit = sum_s w_s Phi(r_s isd_s)  (= F_i(y_i) of k_mcheck_quantile, bit for bit)
//     without y:  mean = sum_s w_s m_s, no pit
//     sd = sqrt(fmax(sum_s w_s (var_s + m_s m_s) - mean mean, 0))
//     brk[2 i], brk[2 i + 1] = min_s (m_s - c sd_s), max_s (m_s + c sd_s),  sd_s = sqrt(var_s)   (brk != NULL: a bound was asked for)
//     flag[i] = 1 where a w_s, isd_s or m_s of the row is NaN (k_mcheck_stage: a log weight that is not finite, a NaN or negative var; a NaN mean)
// A flagged row is NaN in mean, sd and pit; a NaN y makes the three NaN too (they are formed through y) and leaves flag and brk alone.
// mean, sd, pit, brk are nullable; flag is not.  Three row sums, each in the order of the header.  116 VGPRs, 11 KiB of LDS, no scratch.
__global__ __launch_bounds__(256) void k_mcheck_moments(const double *M, const double *V, const double *Wt, const double *Isd, const double *y, int D,
                                                        int i0, double c, double *mean, double *sd, double *pit, double *brk, int *flag)
{
    __shared__ double ra[256], rb[256], rc[256], rlo[256], rhi[256];
    __shared__ int rf[256];
    const int i = i0 + (int)blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)i * (size_t)D;
    const double *m = M + base, *v = V + base, *wt = Wt + base, *isd = Isd + base;
    const bool has_y = y != nullptr;
    const double yi = has_y ? y[i] : 0.0;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (int s = tid; s < D; s += 256) {
        const double w = wt[s], ms = m[s], vs = v[s], is = isd[s];
        if (w != w || is != is || ms != ms) bad = 1;
        if (has_y) {
            const double r = yi - ms;
            a1 = a1 + w * r;
            a3 = a3 + w * mcheck_phi(yi, ms, is);
        } else {
            a1 = a1 + w * ms;
        }
        a2 = a2 + w * (vs + ms * ms);
        const double h = c * sqrt(vs);
        mn = fmin(mn, ms - h);
        mx = fmax(mx, ms + h);
    }
    ra[tid] = a1; rb[tid] = a2; rc[tid] = a3; rlo[tid] = mn; rhi[tid] = mx; rf[tid] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            ra[tid] = ra[tid] + ra[tid + w]; rb[tid] = rb[tid] + rb[tid + w]; rc[tid] = rc[tid] + rc[tid + w];
            rlo[tid] = fmin(rlo[tid], rlo[tid + w]); rhi[tid] = fmax(rhi[tid], rhi[tid + w]); rf[tid] |= rf[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double nanv = __builtin_nan("");
        const bool nan = rf[0] != 0 || yi != yi;
        const double mu = has_y ? yi - ra[0] : ra[0];
        if (mean) mean[i] = nan ? nanv : mu;
        if (sd) sd[i] = nan ? nanv : sqrt(fmax(rb[0] - mu * mu, 0.0));
        if (pit) pit[i] = (nan || !has_y) ? nanv : rc[0];
        if (brk) { brk[2 * (size_t)i] = rlo[0]; brk[2 * (size_t)i + 1] = rhi[0]; }
        flag[i] = rf[0];
    }
}

// ===================================================================================== k_mcheck_quantile
// Row i = i0 + blockIdx.x, blockIdx.y = 0: p_lo -> lower, 1: p_hi -> upper (a NULL output: nothing to do); grid = (the rows of the chunk, 2).
// The p-quantile of F_i(t) = sum_s w_s Phi((t - m_s) isd_s), Phi(z) = erfc(z (-1 / sqrt 2)) / 2, a point mass [t >= m_s], by k_loo_quantile's
// bisection from k_mcheck_moments' bracket [lo, hi] = brk[2 i .. 2 i + 1]: F(mid) < p moves the lower end, anything else the upper one, until the
// bracket is no wider than 2^-40 of the first one (at most MCHECK_MAX_IT halvings); the midpoint.  A bracket without width (one point mass) is its
// own midpoint.  Every F is a row sum in the order of the header, broadcast through LDS: the workgroup branches as one.  A flagged row, or a NaN
// F, gives NaN.  Per evaluation and draw three loads, two products and one erfc.  108 VGPRs, 2 KiB of LDS, no scratch.
__global__ __launch_bounds__(256) void k_mcheck_quantile(const double *M, const double *Wt, const double *Isd, int D, int i0, const double *brk,
                                                         const int *flag, double p_lo, double p_hi, double *lower, double *upper)
{
    __shared__ double ra[256];
    const int i = i0 + (int)blockIdx.x, tid = threadIdx.x;
    double *out = blockIdx.y ? upper : lower;
    if (!out) return;
    if (flag[i]) {
        if (tid == 0) out[i] = __builtin_nan("");
        return;
    }
    const double p = blockIdx.y ? p_hi : p_lo;
    const size_t base = (size_t)i * (size_t)D;
    const double *m = M + base, *wt = Wt + base, *isd = Isd + base;
    double lo = brk[2 * (size_t)i], hi = brk[2 * (size_t)i + 1];
    const double tol = (hi - lo) * 9.094947017729282e-13;                // 2^-40
    bool nan = false;
    for (int it = 0; it < MCHECK_MAX_IT && hi - lo > tol; ++it) {
        const double mid = 0.5 * (lo + hi);
        double acc = 0.0;
        for (int s = tid; s < D; s += 256) acc = acc + wt[s] * mcheck_phi(mid, m[s], isd[s]);
        ra[tid] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w) ra[tid] = ra[tid] + ra[tid + w]; __syncthreads(); }
        const double F = ra[0];
        __syncthreads();
        if (F != F) { nan = true; break; }
        if (F < p) lo = mid; else hi = mid;
    }
    if (tid == 0) out[i] = nan ? __builtin_nan("") : 0.5 * (lo + hi);
}
