// bnr_medge_kernels.h -- the gfx950 kernels that libbnr_medge.so (include/bnr_medge.h) adds to those of bnr_mloo_kernels.h: the conditional
// posterior of every edge coefficient given phi = (tau2, mu, W, S) of a draw, gamma_e | phi, y ~ N(m_e, v_e), and the summary of the mixture of
// those normals over the draws.  With A = I + X diag(S) X^T = L L^T, M = L^-1 and g = A^-1 r as k_mloo_factor leaves them:
//     T = M X,   t_e = sum_r T_re^2 = x_e^T A^-1 x_e,   p_e = sum_i x_ie g_i
//     m_e = W_e + S_e p_e,   v_e = (tau2 S_e) fmax(1 - S_e t_e, 0)
// Two kernels: k_medge_proj (T on the f64 matrix pipe, m and v of a batch of draws) and k_medge_summary (one wave per edge).  Every sum of
// k_medge_proj runs in an order fixed by (n, q) alone, every sum of k_medge_summary in one fixed by (K, nd) alone: no result depends on the batch,
// on the other draws or edges, on the grid or on the call, bit for bit.  Plain C++, MFMA builtins and vector stores; no atomics.  Compiled with
// -ffp-contract=off: every product and every sum is rounded on its own.
#pragma once
#include "bnr_mloo_kernels.h"

#define MEDGE_EB 128            // edges per workgroup of k_medge_proj: wave w owns edges 32 w .. 32 w + 31 of the block, two 16-column MFMA tiles
#define MEDGE_DB 4              // draws per workgroup: a staged panel of X is used MEDGE_DB times
#define MEDGE_KC 32             // rows of X staged in LDS per step of the K loop (8 MFMA steps of 4)
#define MEDGE_LD 144            // leading dimension of the staged panel in doubles: lane groups g = 0, 1 (rows k, k + 1) fall into disjoint LDS banks
#define MEDGE_SQRT1_2 0.70710678118654752440

// ===================================================================================== k_medge_proj
// m and v of every edge for the draws of a batch.  grid = (ceil(q / MEDGE_EB), ceil(B / MEDGE_DB)), 256 threads.  Workgroup (x, y): the edges
// e0 = x MEDGE_EB .. and the draws b0 = y MEDGE_DB .. of the batch.  The panel X[k0 .. k0 + 31][e0 .. e0 + 127] is staged in LDS (sX[k][e]) and
// shared by the draws; the other operand, M = L^-1 of a draw, is read where k_mloo_factor left it: M[r][i] at (G_b + np)[r np + i], contiguous
// along i like a column of X.
//   1. p_e = sum_i x_ie g_i, i ascending from 0.0, by thread e of the block, with g_i = resid_i (tau2 / var_i) from the factor kernel's outputs
//      (out[i ldo + s0 + b]) staged beside the panel.
//   2. T = M X by v_mfma_f64_16x16x4_f64, 16 rows r of M at a time (row tile rt), K = the rows i of X in steps of 4 from 0 up to the first multiple of
//      32 past the tile's diagonal (M is lower triangular); one accumulator per (draw, column tile).  The squares of a finished tile are added to a
//      lane's t: lane group g = lane >> 4 holds rows 16 rt + g + 4 j, j = 0 .. 3, and sums them j ascending, rt ascending, from 0.0; at the end
//      t_e = ((t_g0 + t_g1) + t_g2) + t_g3.
//   Masks, all by selecting the constant 0.0 at staging, never by reading memory that was not asked for: M[r][i] with i > r (those slots hold
//   entries of L), r >= n or i >= n (never written by the factor kernel), rows of X past n, edges past q, draws past B.  Every address formed
//   stays inside X (n x q), inside the np (np + 1) doubles of a draw and inside resid / var.
// A draw flagged in bad[] is NaN in m and v.  Out: Mo / Vo[e ldo + s0 + b], edge-major (ldo = the draws of the call), W NULL: 0.0.
// MFMA layouts as in k_mloo_gram: A lane l = row l & 15, k = l >> 4; B lane l = k = l >> 4, column l & 15; D lane l, reg j = row (l >> 4) + 4 j,
// column l & 15.
__global__ __launch_bounds__(256) void k_medge_proj(const double *X, int ldx, int n, int np, int q, const double *G, long long gstride,
                                                    const double *const *Sp, const double *W, const double *tau2, const double *resid,
                                                    const double *var, const int *bad, int s0, long long ldo, int B, double *Mo, double *Vo)
{
    __shared__ double sX[MEDGE_KC * MEDGE_LD];
    __shared__ double sG[MEDGE_DB * MEDGE_KC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int e0 = (int)blockIdx.x * MEDGE_EB, b0 = (int)blockIdx.y * MEDGE_DB;
    const int se = tid & (MEDGE_EB - 1), sh = tid >> 7;                 // staging: edge se of the block, rows 16 sh .. 16 sh + 15 of the step
    const bool ev = e0 + se < q;
    const double *xcol = X + (size_t)min(e0 + se, q - 1) * (size_t)ldx;
    // ---- 1. p
    double p[MEDGE_DB];
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d) p[d] = 0.0;
    for (int k0 = 0; k0 < n; k0 += MEDGE_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = sh * 16 + j, i = k0 + k;
            const double xv = xcol[min(i, n - 1)];
            sX[k * MEDGE_LD + se] = (ev && i < n) ? xv : 0.0;
        }
        if (tid < MEDGE_DB * MEDGE_KC) {
            const int d = tid >> 5, i = k0 + (tid & 31), b = min(b0 + d, B - 1);
            const size_t o = (size_t)min(i, n - 1) * (size_t)ldo + (size_t)(s0 + b);
            const double rs = resid[o], vr = var[o], gi = rs * (tau2[b] / vr);
            sG[tid] = (i < n && b0 + d < B) ? gi : 0.0;
        }
        __syncthreads();
        if (tid < MEDGE_EB) {
#pragma unroll 8
            for (int k = 0; k < MEDGE_KC; ++k) {
                const double xv = sX[k * MEDGE_LD + tid];
#pragma unroll
                for (int d = 0; d < MEDGE_DB; ++d) p[d] = p[d] + xv * sG[d * MEDGE_KC + k];
            }
        }
    }
    // ---- 2. t
    const double *Mp[MEDGE_DB];
    bool dv[MEDGE_DB];
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d) {
        Mp[d] = G + (size_t)min(b0 + d, B - 1) * (size_t)gstride + np;
        dv[d] = b0 + d < B;
    }
    double ts[MEDGE_DB][2];
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d) ts[d][0] = ts[d][1] = 0.0;
    const int nrt = (n + 15) / 16;
    for (int rt = 0; rt < nrt; ++rt) {
        mloo_d4 acc[MEDGE_DB][2];
#pragma unroll
        for (int d = 0; d < MEDGE_DB; ++d) acc[d][0] = acc[d][1] = mloo_d4{0.0, 0.0, 0.0, 0.0};
        const int r = rt * 16 + c, kend = (rt + 1) * 16;
        const size_t roff = (size_t)r * (size_t)np;
        for (int k0 = 0; k0 < kend; k0 += MEDGE_KC) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = sh * 16 + j, i = k0 + k;
                const double xv = xcol[min(i, n - 1)];
                sX[k * MEDGE_LD + se] = (ev && i < n) ? xv : 0.0;
            }
            double a[MEDGE_DB][MEDGE_KC / 4];
#pragma unroll
            for (int d = 0; d < MEDGE_DB; ++d)
#pragma unroll
                for (int s8 = 0; s8 < MEDGE_KC / 4; ++s8) {
                    const int i = k0 + 4 * s8 + g;                       // (i <= k0 + 31 <= np - 1, r <= np - 1: inside the draw's M)
                    const double mv = Mp[d][roff + (size_t)i];
                    a[d][s8] = (dv[d] && r < n && i <= r) ? mv : 0.0;
                }
            __syncthreads();
#pragma unroll
            for (int s8 = 0; s8 < MEDGE_KC / 4; ++s8) {
                const int k = 4 * s8 + g;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const double xb = sX[k * MEDGE_LD + w * 32 + ct * 16 + c];
#pragma unroll
                    for (int d = 0; d < MEDGE_DB; ++d) acc[d][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[d][s8], xb, acc[d][ct], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < MEDGE_DB; ++d)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int j = 0; j < 4; ++j) ts[d][ct] = ts[d][ct] + acc[d][ct][j] * acc[d][ct][j];
    }
    // ---- the four lane groups' parts of t meet in LDS (the panel is done with); thread e of the block finishes its edge
    __syncthreads();
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) sX[(d * MEDGE_EB + w * 32 + ct * 16 + c) * 4 + g] = ts[d][ct];
    __syncthreads();
    if (tid < MEDGE_EB && ev) {
        const int e = e0 + tid;
        const double nanv = __builtin_nan("");
#pragma unroll
        for (int d = 0; d < MEDGE_DB; ++d) {
            if (b0 + d >= B) break;
            const int b = b0 + d;
            const double *tp = sX + (d * MEDGE_EB + tid) * 4;
            const double t = ((tp[0] + tp[1]) + tp[2]) + tp[3];
            const double Se = Sp[b][e], We = W ? W[(size_t)b * (size_t)q + e] : 0.0, t2 = tau2[b];
            double me = We + Se * p[d];
            double ve = (t2 * Se) * fmax(1.0 - Se * t, 0.0);
            if (bad[s0 + b]) { me = nanv; ve = nanv; }
            const size_t o = (size_t)e * (size_t)ldo + (size_t)(s0 + b);
            Mo[o] = me;
            Vo[o] = ve;
        }
    }
}

// ===================================================================================== k_medge_summary
// The summary of the mixture sum_s omega_s N(m_se, v_se) of one edge per wave (grid = ceil(q / 4), 256 threads; wave w of workgroup x: edge 4 x + w).
// In: m, v edge-major, edge e's D = K nd draws at m + e ld, chain k's in places k nd .. ; wk[K] the chain weights, omega_s = wk / nd.
// A chain sum: lane l adds the terms of draws l, l + 64, l + 128, ... of the chain in that order from 0.0; the 64 lane sums are then added pairwise,
// lane l with lane l ^ 32, then ^ 16, 8, 4, 2, 1 (every lane ends with the same bits).  A statistic: sum_k (chain sum / nd) wk, k ascending from 0.0.
//     mean = sum omega m;  sd = sqrt(fmax(sum omega (v + m m) - mean mean, 0));  var_within = sum omega v
//     p_pos = sum omega erfc((m / sqrt v) (-1 / sqrt 2)) / 2,   p_neg = sum omega erfc((m / sqrt v) (1 / sqrt 2)) / 2;   v = 0: [m > 0], [m < 0]
//     lower / upper: the p_lo / p_hi quantile of F(t) = sum omega Phi((t - m) / sqrt v), Phi(z) = erfc(z (-1 / sqrt 2)) / 2, v = 0: [t >= m]; bisection
//     from [min (m - c sqrt v), max (m + c sqrt v)] as k_loo_quantile does it: F(mid) < p moves the lower end, anything else the upper one, until the
//     bracket is no wider than 2^-40 of the first one (at most MEDGE_MAX_IT halvings); the midpoint.
// An edge with a NaN in m or v is NaN in every output.  Every output pointer is nullable.  No LDS, no barrier.
#define MEDGE_MAX_IT 64
__device__ __forceinline__ double medge_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ double medge_cdf(const double *me, const double *ve, int K, int nd, const double *wk, int lane, double t)
{
    double F = 0.0;
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (int j = lane; j < nd; j += 64) {
            const double mm = me[(size_t)k * nd + j], vv = ve[(size_t)k * nd + j];
            const double z = (t - mm) / sqrt(vv);
            const double ph = (vv == 0.0) ? (t >= mm ? 1.0 : 0.0) : 0.5 * erfc(z * -MEDGE_SQRT1_2);
            a = a + ph;
        }
        F = F + (medge_wave_sum(a) / (double)nd) * wk[k];
    }
    return F;
}
__global__ __launch_bounds__(256) void k_medge_summary(const double *m, const double *v, long long ld, int q, int K, int nd, const double *wk, double c,
                                                       double p_lo, double p_hi, double *mean, double *sd, double *var_within, double *p_pos,
                                                       double *p_neg, double *lower, double *upper)
{
    const int lane = threadIdx.x & 63, e = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (e >= q) return;                                                  // (a whole wave leaves: no barrier in this kernel)
    const double *me = m + (size_t)e * (size_t)ld, *ve = v + (size_t)e * (size_t)ld;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, mn = INFINITY, mx = -INFINITY;
    int isnan_ = 0;
    for (int k = 0; k < K; ++k) {
        double a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
        for (int j = lane; j < nd; j += 64) {
            const double mm = me[(size_t)k * nd + j], vv = ve[(size_t)k * nd + j];
            if (mm != mm || vv != vv) isnan_ = 1;
            const double s = sqrt(vv), r = mm / s;
            a1 = a1 + mm;
            a2 = a2 + (vv + mm * mm);
            a3 = a3 + vv;
            a4 = a4 + ((vv == 0.0) ? (mm > 0.0 ? 1.0 : 0.0) : 0.5 * erfc(r * -MEDGE_SQRT1_2));
            a5 = a5 + ((vv == 0.0) ? (mm < 0.0 ? 1.0 : 0.0) : 0.5 * erfc(r * MEDGE_SQRT1_2));
            mn = fmin(mn, mm - c * s);
            mx = fmax(mx, mm + c * s);
        }
        const double w = wk[k], dn = (double)nd;
        s1 = s1 + (medge_wave_sum(a1) / dn) * w;
        s2 = s2 + (medge_wave_sum(a2) / dn) * w;
        s3 = s3 + (medge_wave_sum(a3) / dn) * w;
        s4 = s4 + (medge_wave_sum(a4) / dn) * w;
        s5 = s5 + (medge_wave_sum(a5) / dn) * w;
    }
    const bool nan = __any(isnan_) != 0;
    const double nanv = __builtin_nan("");
    if (lane == 0) {
        if (mean) mean[e] = nan ? nanv : s1;
        if (sd) sd[e] = nan ? nanv : sqrt(fmax(s2 - s1 * s1, 0.0));
        if (var_within) var_within[e] = nan ? nanv : s3;
        if (p_pos) p_pos[e] = nan ? nanv : s4;
        if (p_neg) p_neg[e] = nan ? nanv : s5;
    }
    if (!lower && !upper) return;
    if (nan) {
        if (lane == 0) { if (lower) lower[e] = nanv; if (upper) upper[e] = nanv; }
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mn = fmin(mn, __shfl_xor(mn, off)); mx = fmax(mx, __shfl_xor(mx, off)); }
    for (int side = 0; side < 2; ++side) {
        double *out = side ? upper : lower;
        if (!out) continue;
        const double p = side ? p_hi : p_lo;
        double lo = mn, hi = mx;
        const double tol = (hi - lo) * 9.094947017729282e-13;             // 2^-40
        bool fnan = false;
        for (int it = 0; it < MEDGE_MAX_IT && hi - lo > tol; ++it) {
            const double mid = 0.5 * (lo + hi);
            const double F = medge_cdf(me, ve, K, nd, wk, lane, mid);
            if (F != F) { fnan = true; break; }
            if (F < p) lo = mid; else hi = mid;
        }
        if (lane == 0) out[e] = fnan ? nanv : 0.5 * (lo + hi);
    }
}
