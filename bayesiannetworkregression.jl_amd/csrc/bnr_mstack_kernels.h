// bnr_mstack_kernels.h -- the gfx950 kernel of libbnr_mstack.so (include/bnr_mstack.h) beside the four of bnr_mloo_kernels.h and the row kernels
// of bnr_mcheck_kernels.h: the staging of the stacked mixture of K chains,
//     sum_{k: w_k > 0} sum_s (w_k exp(lw_kis)) N(m_kis, var_kis),
// from the pooled rows x D matrices (D = K nd, a row's draws contiguous, chain k's in columns k nd .. (k + 1) nd - 1) into the compacted rows x D+
// matrices k_mcheck_moments and k_mcheck_quantile read (D+ = K+ nd, the K+ chains with w_k > 0 in chain order, then draw order).  It is
// k_mcheck_stage's arithmetic fused with the gather: the columns of a chain with w_k = 0 are never read.  Plain C++; no atomics, no LDS, no
// scratch.  Compiled with -ffp-contract=off.  Every index into a matrix is formed in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MSTACK_STRIP 256        // components of a row per workgroup

// ===================================================================================== k_mstack_stage
// Workgroup (blockIdx.x, blockIdx.y) owns the strip of components j = 256 blockIdx.x + t (t = the thread) of rows blockIdx.y, blockIdx.y +
// gridDim.y, ...; grid = (ceil(D+ / 256), any).  A thread finds its component's place once, before the rows: the retained chain kk = j / nd (one
// 32-bit division per thread and launch, none per element), its draw s = j - kk nd, the source column col = csel[kk] nd + s and the chain weight
// wk = wsel[kk] (csel, wsel: the K+ retained chains' indices, ascending, and their weights).  Per element, with o = i D + col and p = i D+ + j:
//     Wt[p]  = wk * exp(LW[o]), the product rounded once; NaN where LW[o] is not finite (a refused row of bnr_psis_weights, a caller's +-inf)
//     Isd[p] = 1 / sqrt(V[o]): +inf for V = 0 (a point mass, and only then), NaN for a NaN or negative V
//     Mo[p]  = y[i] - A[o]  (y != NULL: the chain form, A = resid)  or  A[o]  (the raw form: A = the means)
//     Vo[p]  = V[o]         (Vo != NULL: a chain was dropped, so the row kernels cannot read V in place)
// With wk = 1 the three are k_mcheck_stage's, bit for bit.
__global__ __launch_bounds__(256) void k_mstack_stage(const double *LW, const double *V, const double *A, const double *y, int rows, int D, int Dp, int nd,
                                                      const int *csel, const double *wsel, double *Wt, double *Isd, double *Mo, double *Vo)
{
    const unsigned j = blockIdx.x * (unsigned)MSTACK_STRIP + threadIdx.x;
    if (j >= (unsigned)Dp) return;
    const unsigned kk = j / (unsigned)nd, s = j - kk * (unsigned)nd;
    const size_t col = (size_t)csel[kk] * (size_t)nd + (size_t)s;
    const double wk = wsel[kk];
    for (long long i = blockIdx.y; i < (long long)rows; i += (long long)gridDim.y) {
        const size_t o = (size_t)i * (size_t)D + col, p = (size_t)i * (size_t)Dp + (size_t)j;
        const double lw = LW[o], v = V[o], a = A[o];
        const double e = (lw - lw == 0.0) ? exp(lw) : __builtin_nan("");          // (lw - lw is 0 for a finite lw alone)
        Wt[p] = wk * e;
        Isd[p] = 1.0 / sqrt(v);
        Mo[p] = y ? y[i] - a : a;
        if (Vo) Vo[p] = v;
    }
}
