// bnr_mcov_kernels.h -- the gfx950 kernels that libbnr_mcov.so (include/bnr_mcov.h) adds to those of bnr_mloo_kernels.h and to k_medge_summary: the
// covariance of the edge coefficients with gamma integrated out.  Given phi of a draw s the whole vector gamma is Gaussian, N(m_s, tau2_s (D_s -
// D_s X^T A_s^-1 X D_s)); with T_s = L_s^-1 X as k_mloo_factor leaves L^-1 and the scaled panel T'_sia = (sqrt(tau2_s) S_sa) T_sia
//     within = sum_s omega_s (diag(tau2_s S_s) - T'_s^T T'_s),   between = sum_s omega_s (m_s - mean)(m_s - mean)^T,   cov = within + between
// Four kernels: k_mcov_proj (k_medge_proj's body over the gathered columns; besides m and v it stores tau2 S and the panel T'), k_mcov_gram (the
// symmetric product of a row panel on the f64 matrix pipe, continued from launch to launch in one accumulator per entry), k_mcov_center (m - mean,
// draw-major) and k_mcov_finish (the chains' Grams weighted, subtracted from the diagonal, mirrored).  Every sum of an entry runs in an order fixed
// by (n, K, nd) alone: no result depends on the batch, on the sub-batches, on the grid, on the other columns of the call, on a column's place in
// cols or on the call, bit for bit.  Plain C++, MFMA builtins and vector stores; no atomics.  Compiled with -ffp-contract=off.
#pragma once
#include "bnr_medge_kernels.h"

#define MCOV_T 128              // columns per side of a Gram workgroup's tile pair: 2 x 2 waves of 64 x 64, sixteen 16 x 16 MFMA tiles each
#define MCOV_KC 16              // panel rows staged in LDS per step of the Gram's K loop (4 MFMA steps of 4)
#define MCOV_LD 144             // leading dimension of a staged panel in doubles (MEDGE_LD's reason)

// ===================================================================================== k_mcov_proj
// k_medge_proj over the columns cols[0 .. nc - 1] of X (a copy of its body: a shared one cost that kernel registers): the same
// staging, the same masks, the same order of every sum, so m and v of a column are k_medge_proj's of that edge, bit for bit.  grid =
// (ceil(nc / MEDGE_EB), ceil(B / MEDGE_DB)), 256 threads; B: the draws of the sub-batch, draw b of it at G + b gstride, tau2[b], Sp[b], W + b q and
// place s0 + b of the call.  Besides Mo / Vo[a ldo + s0 + b] (column-major over the chosen columns a) it stores
//     Do[a ldo + s0 + b] = tau2_b S_ba                                      (the diagonal's term; NaN for a flagged draw, like m and v)
//     Tp[(b rs + i) cp + a] = (sqrt(tau2_b) S_ba) T_ia,  i = 0 .. rs - 1     (rs = the rows rounded up to 16, cp = nc rounded up to 16; rows >= n
//                                                                            and columns >= nc are +-0.0: their T is a sum of 0.0 products)
// where T_ia is the finished MFMA accumulator of k_medge_proj's step 2 (K = the rows of X in steps of 4 from 0 up to the first multiple of 32 past
// the row tile's diagonal, one accumulator per entry).  The scale is rounded once (sqrt, then the product with S), then the product with T.
// Masks by selecting the constant 0.0, never by reading memory that was not asked for; every address formed stays inside X (n x q), cols (nc), the
// np (np + 1) doubles of a draw, resid / var, a draw's q values of S and W, and the sub-batch's B rs cp doubles of Tp.
__global__ __launch_bounds__(256) void k_mcov_proj(const double *X, int ldx, int n, int np, int q, const int *cols, int nc, int cp, int rs,
                                                   const double *G, long long gstride, const double *const *Sp, const double *W, const double *tau2,
                                                   const double *resid, const double *var, const int *bad, int s0, long long ldo, int B, double *Mo,
                                                   double *Vo, double *Do, double *Tp)
{
    __shared__ double sX[MEDGE_KC * MEDGE_LD];
    __shared__ double sG[MEDGE_DB * MEDGE_KC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int a0 = (int)blockIdx.x * MEDGE_EB, b0 = (int)blockIdx.y * MEDGE_DB;
    const int se = tid & (MEDGE_EB - 1), sh = tid >> 7;                 // staging: column se of the block, rows 16 sh .. 16 sh + 15 of the step
    const bool ev = a0 + se < nc;
    const double *xcol = X + (size_t)cols[min(a0 + se, nc - 1)] * (size_t)ldx;
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
            const double rsd = resid[o], vr = var[o], gi = rsd * (tau2[b] / vr);
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
    // ---- 2. t and T'
    const double *Mp[MEDGE_DB];
    bool dv[MEDGE_DB];
    double sc[MEDGE_DB][2];                                              // the scale of this lane's two columns: (sqrt tau2) S, 0.0 past nc
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d) {
        const int b = min(b0 + d, B - 1);
        Mp[d] = G + (size_t)b * (size_t)gstride + np;
        dv[d] = b0 + d < B;
        const double st = sqrt(tau2[b]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int a = a0 + w * 32 + ct * 16 + c;
            const double sv = Sp[b][cols[min(a, nc - 1)]];
            sc[d][ct] = (a < nc) ? st * sv : 0.0;
        }
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
            for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ts[d][ct] = ts[d][ct] + acc[d][ct][j] * acc[d][ct][j];
                const int a = a0 + w * 32 + ct * 16 + c;
                if (dv[d] && a < cp) {                                   // (rows 16 rt + g + 4 j < rs, columns < cp, draws < B: inside Tp)
                    double *tp = Tp + ((size_t)(b0 + d) * (size_t)rs + (size_t)(rt * 16 + g)) * (size_t)cp + (size_t)a;
#pragma unroll
                    for (int j = 0; j < 4; ++j) tp[(size_t)(4 * j) * (size_t)cp] = sc[d][ct] * acc[d][ct][j];
                }
            }
    }
    // ---- the four lane groups' parts of t meet in LDS (the panel is done with); thread a of the block finishes its column
    __syncthreads();
#pragma unroll
    for (int d = 0; d < MEDGE_DB; ++d)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) sX[(d * MEDGE_EB + w * 32 + ct * 16 + c) * 4 + g] = ts[d][ct];
    __syncthreads();
    if (tid < MEDGE_EB && ev) {
        const int a = a0 + tid, e = cols[a];
        const double nanv = __builtin_nan("");
#pragma unroll
        for (int d = 0; d < MEDGE_DB; ++d) {
            if (b0 + d >= B) break;
            const int b = b0 + d;
            const double *tp = sX + (d * MEDGE_EB + tid) * 4;
            const double t = ((tp[0] + tp[1]) + tp[2]) + tp[3];
            const double Se = Sp[b][e], We = W ? W[(size_t)b * (size_t)q + e] : 0.0, t2 = tau2[b];
            double me = We + Se * p[d];
            double de = t2 * Se;
            double ve = de * fmax(1.0 - Se * t, 0.0);
            if (bad[s0 + b]) { me = nanv; ve = nanv; de = nanv; }
            const size_t o = (size_t)a * (size_t)ldo + (size_t)(s0 + b);
            Mo[o] = me;
            Vo[o] = ve;
            Do[o] = de;
        }
    }
}

// ===================================================================================== k_mcov_gram
// Gt[a, b] += sum_r P[r][a] P[r][b] over the rows r = 0 .. nrows - 1 of a row panel P (row r at P + r ld, pc columns), lower tile pairs only, by
// v_mfma_f64_16x16x4_f64 with the rows as the K dimension.  grid = nt (nt + 1) / 2 with nt = ceil(pc / MCOV_T), 256 threads: workgroup x owns the
// pair (ta >= tb) number x = ta (ta + 1) / 2 + tb of MCOV_T x MCOV_T entries, kept at Gt + x MCOV_T^2, entry (i, j) of the pair at [i MCOV_T + j]
// (a diagonal pair whole; only its i >= j is read later).  The workgroup LOADS its accumulators from Gt, continues each entry's single MFMA chain
// over the rows in steps of 4 from row 0 up (inside a step the MFMA's own order, lane group g holds row k + g), and stores them: a sequence of
// launches over consecutive panels is the one chain over all their rows -- whatever the panels' sizes, as long as each holds a multiple of 4 rows
// but the last -- so no sum depends on how the rows were cut into launches.  No atomics, no reduction across workgroups.
// Per step of MCOV_KC rows the two column panels are staged in LDS once (thread = column tid & 127, rows 8 (tid >> 7) .. + 7), the next step's
// values already in flight in registers (loaded unconditionally from clamped addresses, masked at the LDS store); wave w owns the 64 x 64 entries (w >> 1, w & 1) of the pair, sixteen accumulators, four values of each
// panel read from LDS per MFMA step of 4 rows.  Rows >= nrows and columns >= pc are the constant 0.0 selected at staging; every address formed
// stays inside the panel's nrows x pc entries and the pair's MCOV_T^2 doubles.  MFMA layouts as in k_mloo_gram.
__global__ __launch_bounds__(256) void k_mcov_gram(const double *P, long long ld, long long nrows, int pc, double *Gt)
{
    __shared__ double sA[MCOV_KC * MCOV_LD], sB[MCOV_KC * MCOV_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    long long ta = (long long)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((ta + 1) * (ta + 2) / 2 <= (long long)blockIdx.x) ++ta;
    while (ta * (ta + 1) / 2 > (long long)blockIdx.x) --ta;
    const long long tb = (long long)blockIdx.x - ta * (ta + 1) / 2;
    const int wa = (w >> 1) * 64, wb = (w & 1) * 64;
    const int scol = tid & (MCOV_T - 1), srow = (tid >> 7) * 8;
    const long long ca = ta * MCOV_T + scol, cb = tb * MCOV_T + scol;
    const bool va = ca < pc, vb = cb < pc;
    const double *pa = P + min(ca, (long long)pc - 1), *pb = P + min(cb, (long long)pc - 1);
    double *gt = Gt + (size_t)blockIdx.x * (size_t)(MCOV_T * MCOV_T);
    mloo_d4 acc[4][4];
#pragma unroll
    for (int at = 0; at < 4; ++at)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[at][bt][j] = gt[(wa + at * 16 + g + 4 * j) * MCOV_T + wb + bt * 16 + c];
    double ra[8], rb[8];                                                 // the next step's values as loaded: masked where they are stored
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long long rc = min((long long)(srow + j), nrows - 1);
        ra[j] = pa[(size_t)rc * (size_t)ld];
        rb[j] = pb[(size_t)rc * (size_t)ld];
    }
    for (long long k0 = 0; k0 < nrows; k0 += MCOV_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool rv = k0 + srow + j < nrows;
            sA[(srow + j) * MCOV_LD + scol] = (va && rv) ? ra[j] : 0.0;
            sB[(srow + j) * MCOV_LD + scol] = (vb && rv) ? rb[j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {                                    // (unconditional, rows clamped into the panel: in flight behind the MFMAs below)
            const long long rc = min(k0 + MCOV_KC + srow + j, nrows - 1);
            ra[j] = pa[(size_t)rc * (size_t)ld];
            rb[j] = pb[(size_t)rc * (size_t)ld];
        }
#pragma unroll
        for (int ks = 0; ks < MCOV_KC; ks += 4) {
            const int k = ks + g;
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = sA[k * MCOV_LD + wa + t * 16 + c];
                b[t] = sB[k * MCOV_LD + wb + t * 16 + c];
            }
#pragma unroll
            for (int at = 0; at < 4; ++at)
#pragma unroll
                for (int bt = 0; bt < 4; ++bt) acc[at][bt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[at], b[bt], acc[at][bt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int at = 0; at < 4; ++at)
#pragma unroll
        for (int bt = 0; bt < 4; ++bt)
#pragma unroll
            for (int j = 0; j < 4; ++j) gt[(wa + at * 16 + g + 4 * j) * MCOV_T + wb + bt * 16 + c] = acc[at][bt][j];
}

// ===================================================================================== k_mcov_center
// C[s cp + a] = m[a ldm + s] - mean[a] for the D draws s and the columns a < nc, 0.0 for nc <= a < cp: the row panel of the between Gram, a draw's
// columns contiguous.  grid = (ceil(D / 32), ceil(cp / 32)), 256 threads; a 32 x 32 block goes through LDS so that both sides are read and written
// along their contiguous index.
__global__ __launch_bounds__(256) void k_mcov_center(const double *m, long long ldm, long long D, const double *mean, int nc, int cp, double *C)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long s0 = (long long)blockIdx.x * 32;
    const int a0 = (int)blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int a = a0 + ty + 8 * j;
        const long long s = s0 + tx;
        const double mv = m[(size_t)min(a, nc - 1) * (size_t)ldm + (size_t)min(s, D - 1)], cv = mean[min(a, nc - 1)];
        tile[ty + 8 * j][tx] = (a < nc) ? mv - cv : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long s = s0 + ty + 8 * j;
        const int a = a0 + tx;
        if (s < D && a < cp) C[(size_t)s * (size_t)cp + (size_t)a] = tile[tx][ty + 8 * j];
    }
}

// ===================================================================================== k_mcov_finish
// within and cov of the nc x nc entries, row-major, both triangles from the lower tile pairs (entry (a, b) and entry (b, a) read the same
// accumulators, hi = max(a, b), lo = min(a, b)): with Gw_k / Gb_k the chains' Grams of T' and of m - mean (chain k's at + k gstride)
//     gw = sum_k (Gw_k[hi, lo] / nd) w_k,   gb = sum_k (Gb_k[hi, lo] / nd) w_k            k ascending from 0.0
//     within[a, b] = (cols[a] == cols[b] ? dg[a] : 0.0) - gw,   cov[a, b] = within[a, b] + gb      (a repeated edge is its own diagonal)
// dg[a]: the chain sums of tau2 S of column a, weighted, as k_medge_summary leaves them (its var_within of the matrix Do).  anybad: NaN everywhere.
// grid = (ceil(nc / 256), min(nc, 65535)), 256 threads: thread = b, rows a = blockIdx.y, + gridDim.y, ...
__global__ __launch_bounds__(256) void k_mcov_finish(const double *Gw, const double *Gb, long long gstride, int K, int nd, const double *wk,
                                                     const double *dg, const int *cols, int nc, int anybad, double *within, double *cov)
{
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nc) return;
    const double dn = (double)nd, nanv = __builtin_nan("");
    const int eb = cols[b];
    for (long long a = blockIdx.y; a < nc; a += gridDim.y) {
        const long long hi = a > b ? a : b, lo = a > b ? b : a, ta = hi / MCOV_T, tb = lo / MCOV_T;
        const size_t off = (size_t)(ta * (ta + 1) / 2 + tb) * (size_t)(MCOV_T * MCOV_T) + (size_t)((hi % MCOV_T) * MCOV_T + lo % MCOV_T);
        double gw = 0.0, gb = 0.0;
        for (int k = 0; k < K; ++k) {
            gw = gw + (Gw[(size_t)k * (size_t)gstride + off] / dn) * wk[k];
            gb = gb + (Gb[(size_t)k * (size_t)gstride + off] / dn) * wk[k];
        }
        const double dd = dg[a];
        double wi = (cols[a] == eb ? dd : 0.0) - gw;
        double cv = wi + gb;
        if (anybad) { wi = nanv; cv = nanv; }
        const size_t o = (size_t)a * (size_t)nc + (size_t)b;
        if (within) within[o] = wi;
        if (cov) cov[o] = cv;
    }
}
