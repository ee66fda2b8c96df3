// bnr_mpred_kernels.h -- the gfx950 kernels that libbnr_mpred.so (include/bnr_mpred.h) adds to those of bnr_mloo_kernels.h and
// bnr_medge_kernels.h: the conditional posterior of the mean response of new rows X* (m x q) given phi = (tau2, mu, W, S) of a draw, gamma
// integrated out, and the score of an observed response under the mixture of those normals over the draws.  With D = diag S, A = I + X D X^T =
// L L^T, M = L^-1 and g = A^-1 r as k_mloo_factor leaves them:
//     C = X D X*^T (n x m),   a_j = sum_e x*_je W_e,   d_j = sum_e (x*_je S_e) x*_je,   h_j = sum_i C_ij g_i,   t_j = ||M C_j||^2
//     mean_j = (mu + a_j) + h_j,   var_j = tau2 fmax(d_j - t_j, 0),   vobs_j = var_j + tau2
// Four kernels: k_mpred_rhs (a, d), k_mpred_cross (C on the f64 matrix pipe, by mloo_gram_tile), k_mpred_proj (T = M C on the f64 matrix pipe;
// mean, var, vobs) and k_mpred_score (one wave per new row).  Every sum of the first three runs in an order fixed by (n, q) alone, every sum of
// k_mpred_score in one fixed by (K, nd) alone: no result depends on the batch, on the other draws or new rows, on how the new rows are blocked, on
// the grid or on the call, bit for bit.  Plain C++, MFMA builtins and vector stores; no atomics.  Compiled with -ffp-contract=off: every product
// and every sum is rounded on its own.  Every out-of-range element is the constant 0.0 selected at staging; no address is formed outside its
// operand.
#pragma once
#include "bnr_medge_kernels.h"

#define MPRED_RB 4              // draws per thread of k_mpred_rhs: an element of X* is read once for MPRED_RB draws
#define MPRED_JB 128            // new rows per workgroup of k_mpred_proj: wave w owns rows 32 w .. 32 w + 31 of the block, two 16-column MFMA tiles
#define MPRED_KC 32             // rows of C staged in LDS per step of k_mpred_proj's K loop (8 MFMA steps of 4)
#define MPRED_LD 144            // leading dimension of that panel in doubles (MEDGE_LD's: lane groups g = 0, 1 fall into disjoint LDS banks)

// ===================================================================================== k_mpred_rhs
// a[b][j] = sum_e X*[j][e] W[b][e] (W NULL: 0.0) and d[b][j] = sum_e (X*[j][e] S_b[e]) X*[j][e], e ascending from 0.0.
// grid = (ceil(m / 256), ceil(B / MPRED_RB)), 256 threads: thread = new row j, MPRED_RB draws in registers, X* (column-major, ldn) read once for them
// (coalesced over j; W[b][e] and S_b[e] are one address per wave).  A draw past the batch's end repeats the last one and is not stored.
__global__ __launch_bounds__(256) void k_mpred_rhs(const double *Xn, int ldn, int m, int q, const double *const *Sp, const double *W, int B, double *a,
                                                   double *dq)
{
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x, b0 = (int)blockIdx.y * MPRED_RB;
    if (j >= m) return;
    double aa[MPRED_RB], dd[MPRED_RB];
    const double *w[MPRED_RB], *s[MPRED_RB];
#pragma unroll
    for (int d = 0; d < MPRED_RB; ++d) {
        const int b = min(b0 + d, B - 1);
        aa[d] = 0.0; dd[d] = 0.0;
        w[d] = W ? W + (size_t)b * (size_t)q : nullptr;
        s[d] = Sp[b];
    }
    const double *x = Xn + j;
    if (W) {
        for (int e = 0; e < q; ++e) {
            const double xv = x[(size_t)e * (size_t)ldn];
#pragma unroll
            for (int d = 0; d < MPRED_RB; ++d) { aa[d] = aa[d] + xv * w[d][e]; dd[d] = dd[d] + (xv * s[d][e]) * xv; }
        }
    } else {
        for (int e = 0; e < q; ++e) {
            const double xv = x[(size_t)e * (size_t)ldn];
#pragma unroll
            for (int d = 0; d < MPRED_RB; ++d) dd[d] = dd[d] + (xv * s[d][e]) * xv;
        }
    }
#pragma unroll
    for (int d = 0; d < MPRED_RB; ++d)
        if (b0 + d < B) { a[(size_t)(b0 + d) * (size_t)m + j] = aa[d]; dq[(size_t)(b0 + d) * (size_t)m + j] = dd[d]; }
}

// ===================================================================================== k_mpred_cross
// C_b = X diag(S_b) X*^T for the draws of a batch and the block j0 .. j0 + mblk - 1 of new rows, over mloo_gram_tile (bnr_mloo_kernels.h): no
// triangle, no identity, the second panel rows of X*.  grid = (nt ntj, ceil(B / MLOO_DB)) with nt = np / MLOO_TILE row tiles of X and ntj =
// ceil(mblk / MLOO_TILE) tiles of new rows, 256 threads: workgroup (p, y) is the tiles ti = p / ntj of X and tj = p % ntj of the block.  Every
// address stays inside X (n x q), X* (m x q) and S_b (q).  C_b[(i, jl)], jl = j - j0, is stored at C + b cstride + i + jl np: a column C_j is
// contiguous along i (the layout k_mpred_proj reads it in); all np rows and all 32 ntj columns of the block are written (the padding -- rows of X
// past n, new rows past the block -- as 0.0), cstride >= np 32 ntj.
__global__ __launch_bounds__(256) void k_mpred_cross(const double *X, int ldx, int n, int q, const double *Xn, int ldn, int j0, int mblk,
                                                     const double *const *Sp, int B, double *C, int np, long long cstride)
{
    const int ntj = (mblk + MLOO_TILE - 1) / MLOO_TILE;
    const int ti = (int)blockIdx.x / ntj, tj = (int)blockIdx.x % ntj;
    const int sr = (int)threadIdx.x & 31, rowi = ti * MLOO_TILE + sr, rowj = tj * MLOO_TILE + sr;    // (rowj: within the block)
    mloo_gram_tile<false>(X + min(rowi, n - 1), ldx, rowi < n, Xn + (j0 + min(rowj, mblk - 1)), ldn, rowj < mblk, ti, tj, q, Sp, B, C, np, cstride);
}

// ===================================================================================== k_mpred_proj
// mean, var and vobs of the new rows j0 .. j0 + mblk - 1 for the draws of a batch.  grid = (ceil(mblk / MPRED_JB), B), 256 threads.  Workgroup
// (x, b): the new rows jb0 = x MPRED_JB .. of the block and draw b -- the right operand C_b is the draw's own, so a workgroup owns one draw.
// The panel C_b[k0 .. k0 + 31][jb0 .. jb0 + 127] is staged in LDS (sC[k][j]); the other operand, M = L^-1 of the draw, is read where
// k_mloo_factor left it: M[r][i] at (G_b + np)[r np + i].
//   1. h_j = sum_i C_ij g_i, i ascending from 0.0, by thread j of the workgroup's rows, with g_i = resid_i (tau2 / var_i) from the factor kernel's
//      outputs (out[i ldo + s0 + b]) staged beside the panel.
//   2. T = M C_b by v_mfma_f64_16x16x4_f64, 16 rows r of M at a time (row tile rt), K = the rows i of C in steps of 4 from 0 up to the first
//      multiple of 32 past the tile's diagonal (M is lower triangular); one accumulator per column tile.  The squares of a finished tile are added
//      to a lane's t: lane group g = lane >> 4 holds rows 16 rt + g + 4 j, j = 0 .. 3, and sums them j ascending, rt ascending, from 0.0; at the end
//      t_j = ((t_g0 + t_g1) + t_g2) + t_g3.
//   Masks, all by selecting the constant 0.0 at staging: M[r][i] with i > r (those slots hold entries of L), r >= n or i >= n (never written by the
//   factor kernel), rows of C past n, new rows past the block.  Every address formed stays inside the np mblk doubles of the draw's block of C,
//   inside the np (np + 1) doubles of the draw's factor and inside resid / var.
//   3. mean_j = (mu + a_j) + h_j,  var_j = tau2 fmax(d_j - t_j, 0),  vobs_j = var_j + tau2; a, dq: k_mpred_rhs's, [b m + j].
// A draw flagged in bad[] is NaN in all three.  Out: Mo / Vo / Po[j ldo + s0 + b], row-major per new row (ldo = the draws of the call): the layout
// k_medge_summary reads.
__global__ __launch_bounds__(256) void k_mpred_proj(const double *C, long long cstride, int n, int np, int j0, int mblk, int m, const double *G,
                                                    long long gstride, const double *a, const double *dq, const double *tau2, const double *mu,
                                                    const double *resid, const double *var, const int *bad, int s0, long long ldo, double *Mo,
                                                    double *Vo, double *Po)
{
    __shared__ double sC[MPRED_KC * MPRED_LD];
    __shared__ double sG[MPRED_KC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int jb0 = (int)blockIdx.x * MPRED_JB, b = (int)blockIdx.y;
    const int se = tid & (MPRED_JB - 1), sh = tid >> 7;                 // staging: new row se of the workgroup, rows 16 sh .. 16 sh + 15 of the step
    const bool jv = jb0 + se < mblk;
    const double *ccol = C + (size_t)b * (size_t)cstride + (size_t)min(jb0 + se, mblk - 1) * (size_t)np;
    const double t2 = tau2[b];
    // ---- 1. h
    double h = 0.0;
    for (int k0 = 0; k0 < n; k0 += MPRED_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = sh * 16 + j, i = k0 + k;
            const double cv = ccol[min(i, n - 1)];
            sC[k * MPRED_LD + se] = (jv && i < n) ? cv : 0.0;
        }
        if (tid < MPRED_KC) {
            const int i = k0 + tid;
            const size_t o = (size_t)min(i, n - 1) * (size_t)ldo + (size_t)(s0 + b);
            const double rs = resid[o], vr = var[o], gi = rs * (t2 / vr);
            sG[tid] = (i < n) ? gi : 0.0;
        }
        __syncthreads();
        if (tid < MPRED_JB) {
#pragma unroll 8
            for (int k = 0; k < MPRED_KC; ++k) h = h + sC[k * MPRED_LD + tid] * sG[k];
        }
    }
    // ---- 2. t
    const double *Mp = G + (size_t)b * (size_t)gstride + np;
    double ts[2] = {0.0, 0.0};
    const int nrt = (n + 15) / 16;
    for (int rt = 0; rt < nrt; ++rt) {
        mloo_d4 acc[2];
        acc[0] = acc[1] = mloo_d4{0.0, 0.0, 0.0, 0.0};
        const int r = rt * 16 + c, kend = (rt + 1) * 16;
        const size_t roff = (size_t)r * (size_t)np;
        for (int k0 = 0; k0 < kend; k0 += MPRED_KC) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = sh * 16 + j, i = k0 + k;
                const double cv = ccol[min(i, n - 1)];
                sC[k * MPRED_LD + se] = (jv && i < n) ? cv : 0.0;
            }
            double av[MPRED_KC / 4];
#pragma unroll
            for (int s8 = 0; s8 < MPRED_KC / 4; ++s8) {
                const int i = k0 + 4 * s8 + g;                           // (i <= k0 + 31 <= np - 1, r <= np - 1: inside the draw's M)
                const double mv = Mp[roff + (size_t)i];
                av[s8] = (r < n && i <= r) ? mv : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int s8 = 0; s8 < MPRED_KC / 4; ++s8) {
                const int k = 4 * s8 + g;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const double xb = sC[k * MPRED_LD + w * 32 + ct * 16 + c];
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s8], xb, acc[ct], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int j = 0; j < 4; ++j) ts[ct] = ts[ct] + acc[ct][j] * acc[ct][j];
    }
    // ---- the four lane groups' parts of t meet in LDS (the panel is done with); thread j of the workgroup's rows finishes its row
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) sC[(w * 32 + ct * 16 + c) * 4 + g] = ts[ct];
    __syncthreads();
    if (tid < MPRED_JB && jb0 + tid < mblk) {
        const int j = j0 + jb0 + tid;
        const double nanv = __builtin_nan("");
        const double *tp = sC + tid * 4;
        const double t = ((tp[0] + tp[1]) + tp[2]) + tp[3];
        const double aj = a[(size_t)b * (size_t)m + j], dj = dq[(size_t)b * (size_t)m + j];
        double me = (mu[b] + aj) + h;
        double ve = t2 * fmax(dj - t, 0.0);
        double po = ve + t2;
        if (bad[s0 + b]) { me = nanv; ve = nanv; po = nanv; }
        const size_t o = (size_t)j * (size_t)ldo + (size_t)(s0 + b);
        Mo[o] = me;
        Vo[o] = ve;
        Po[o] = po;
    }
}

// ===================================================================================== k_mpred_score
// The score of an observed response y_j under the mixture sum_s omega_s N(mean_sj, vo_sj) of one new row per wave (grid = ceil(m / 4), 256
// threads; wave w of workgroup x: row 4 x + w).  In: me, vo row-major per new row, row j's D = K nd draws at me + j ld, chain k's in places
// k nd ..; wk[K] the chain weights, omega_s = wk / nd.  Chain sums and statistics in k_medge_summary's order (medge_wave_sum).
//     l_s  = -(log 2 pi + log vo) / 2 - (((y - mean) (y - mean)) / vo) / 2;   vo = 0, the point mass at mean: +inf where y == mean, else -inf
//     mx   = the maximum of l_s over the draws of the chains with wk > 0
//     lpd  = mx + log sum_k (chain sum of exp(l_s - mx) / nd) wk, over the chains with wk > 0, k ascending from 0.0; mx = +inf (y sits on a
//            point mass): +inf; mx = -inf (every component of a weighted chain is a point mass elsewhere): -inf
//     pit  = sum_k (chain sum of Phi((y - mean) / sqrt vo) / nd) wk over all chains, Phi(z) = erfc(z (-1 / sqrt 2)) / 2; vo = 0: [y >= mean]
// A row whose y is NaN, or with a NaN in mean or vo of any draw (a chain of weight 0 included), or with a vo < 0 (l_s is NaN), is NaN in lpd and
// pit.  Every output pointer is nullable.  No LDS, no barrier.
__global__ __launch_bounds__(256) void k_mpred_score(const double *me, const double *vo, long long ld, int m, int K, int nd, const double *wk,
                                                     const double *y, double *lpd, double *pit)
{
    const int lane = threadIdx.x & 63, j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (j >= m) return;                                                  // (a whole wave leaves: no barrier in this kernel)
    const double *mj = me + (size_t)j * (size_t)ld, *vj = vo + (size_t)j * (size_t)ld;
    const double yj = y[j];
    int isnan_ = (yj != yj) ? 1 : 0;
    double mx = -INFINITY, F = 0.0;
    for (int k = 0; k < K; ++k) {
        const bool on = wk[k] > 0.0;
        double ph = 0.0;
        for (int s = lane; s < nd; s += 64) {
            const double mm = mj[(size_t)k * nd + s], vv = vj[(size_t)k * nd + s];
            const double dlt = yj - mm;
            const double l = (vv == 0.0) ? (dlt == 0.0 ? INFINITY : -INFINITY) : -0.5 * (MLOO_LOG_2PI + log(vv)) - 0.5 * ((dlt * dlt) / vv);
            if (mm != mm || vv != vv || l != l) isnan_ = 1;
            if (on) mx = fmax(mx, l);
            const double z = dlt / sqrt(vv);
            ph = ph + ((vv == 0.0) ? (yj >= mm ? 1.0 : 0.0) : 0.5 * erfc(z * -MEDGE_SQRT1_2));
        }
        F = F + (medge_wave_sum(ph) / (double)nd) * wk[k];
    }
    const bool nan = __any(isnan_) != 0;
    const double nanv = __builtin_nan("");
    if (pit && lane == 0) pit[j] = nan ? nanv : F;
    if (!lpd) return;
    if (nan) { if (lane == 0) lpd[j] = nanv; return; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
    if (mx == INFINITY || mx == -INFINITY) { if (lane == 0) lpd[j] = mx; return; }
    double tot = 0.0;
    for (int k = 0; k < K; ++k) {
        if (!(wk[k] > 0.0)) continue;                                    // (the same for every lane)
        double ac = 0.0;
        for (int s = lane; s < nd; s += 64) {
            const double mm = mj[(size_t)k * nd + s], vv = vj[(size_t)k * nd + s];
            const double dlt = yj - mm;
            const double l = (vv == 0.0) ? -INFINITY : -0.5 * (MLOO_LOG_2PI + log(vv)) - 0.5 * ((dlt * dlt) / vv);
            ac = ac + exp(l - mx);
        }
        tot = tot + (medge_wave_sum(ac) / (double)nd) * wk[k];
    }
    if (lane == 0) lpd[j] = mx + log(tot);
}
