// bnr_mloo_kernels.h -- the gfx950 kernels of libbnr_mloo.so (include/bnr_mloo.h): the marginal leave-one-out terms of a batch of draws that
// share one model matrix X.  For a draw b with phi_b = (tau2_b, mu_b, S_b, W_b):
//     A_b = I + X diag(S_b) X^T = L L^T,   r = y - mu_b - X W_b,   z = L^-1 r,   g = L^-T z = A^-1 r,   c_i = (A^-1)_ii = sum_j (L^-1)_ji^2
//     resid_i = g_i / c_i,   var_i = tau2_b / c_i,   loglik_i = -(log 2 pi + log var_i) / 2 - (resid_i^2 / var_i) / 2
//     logml = -(n / 2) log(2 pi tau2_b) - sum_j log L_jj - (||z||^2 / tau2_b) / 2
// Four kernels: k_mloo_w (W and the scalars of a batch out of the chains' table rows), k_mloo_rhs (r), k_mloo_gram (A on the f64 matrix pipe,
// over mloo_gram_tile) and k_mloo_factor (everything behind A, one workgroup per draw).  Every sum of every output runs in an order fixed by
// (n, q) alone: no result depends on the batch, on the other draws of a call, on the grid or on the call, bit for bit.  Plain C++, MFMA
// builtins and vector stores; no atomics.  Compiled with -ffp-contract=off: every product and every sum is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef double mloo_d4 __attribute__((ext_vector_type(4)));

#define MLOO_TILE 32            // rows / columns of A per Gram workgroup: 2 x 2 waves of one 16 x 16 MFMA tile each
#define MLOO_KC 32              // edges staged in LDS per step of the Gram's K loop (8 MFMA steps of 4)
#define MLOO_LDT 48             // leading dimension of a staged panel in doubles: lane groups g = 0, 1 (k, k + 1) fall into disjoint LDS banks
#define MLOO_DB 8               // draws per Gram workgroup: the staged panels of X are used MLOO_DB times
#define MLOO_RB 4               // draws per thread of k_mloo_rhs: an element of X is read once for MLOO_RB draws
#define MLOO_MAX_N 2048         // the factor kernel keeps z, c and g in LDS: 3 x 16 KiB
#define MLOO_LOG_2PI 1.8378770664093454835606594728112

// ===================================================================================== k_mloo_w
// The prior mean W of the edge coefficients and the scalars of the draws of a batch, out of the table rows rowp[b] (the chain form):
//     W[b][e] = sum_t u[t + R el[e]] lam[t] u[t + R ek[e]],  t ascending from 0.0, as the sweep forms it (edge_W of bnr_kernels.h)
// grid = (ceil(q / 256), B), 256 threads; tau2[b] and mu[b] by the first thread of the row's first workgroup.
__global__ __launch_bounds__(256) void k_mloo_w(const double *const *rowp, int o_tau2, int o_mu, int o_lam, int o_u, int R, int q, const int *ek,
                                                const int *el, double *W, double *tau2, double *mu)
{
    const int b = blockIdx.y, e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const double *row = rowp[b];
    if (e < q) {
        const double *u = row + o_u, *lam = row + o_lam;
        const int l = el[e], k = ek[e];
        double s = 0.0;
        for (int t = 0; t < R; ++t) s += u[t + R * l] * lam[t] * u[t + R * k];
        W[(size_t)b * (size_t)q + e] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { tau2[b] = row[o_tau2]; mu[b] = row[o_mu]; }
}

// ===================================================================================== k_mloo_rhs
// r[b][i] = (y_i - mu_b) - sum_e X[i][e] W[b][e], e ascending from 0.0 (W NULL: the sum is 0.0); rows n .. np - 1 of r are 0.0.
// grid = (ceil(np / 256), ceil(B / MLOO_RB)), 256 threads: thread = row i, MLOO_RB draws in registers, X read once for them (coalesced over i;
// W[b][e] is one address per wave).  A draw past the batch's end repeats the last one and is not stored.
__global__ __launch_bounds__(256) void k_mloo_rhs(const double *X, int ldx, const double *y, int n, int np, int q, const double *W, const double *mu, int B,
                                                  double *r)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x, b0 = (int)blockIdx.y * MLOO_RB;
    if (i >= np) return;
    const bool in = i < n;
    double acc[MLOO_RB];
    const double *w[MLOO_RB];
#pragma unroll
    for (int d = 0; d < MLOO_RB; ++d) { acc[d] = 0.0; w[d] = W ? W + (size_t)min(b0 + d, B - 1) * (size_t)q : nullptr; }
    if (W && in) {
        const double *x = X + i;
        for (int e = 0; e < q; ++e) {
            const double xv = x[(size_t)e * (size_t)ldx];
#pragma unroll
            for (int d = 0; d < MLOO_RB; ++d) acc[d] = acc[d] + xv * w[d][e];
        }
    }
#pragma unroll
    for (int d = 0; d < MLOO_RB; ++d)
        if (b0 + d < B) r[(size_t)(b0 + d) * (size_t)np + i] = in ? (y[i] - mu[b0 + d]) - acc[d] : 0.0;
}

// ===================================================================================== mloo_gram_tile, k_mloo_gram
// One 32 x 32 tile of P_b = Xi diag(S_b) Xj^T (IDENT: of I + that) for MLOO_DB draws of a batch, by v_mfma_f64_16x16x4_f64 with the edges as the K
// dimension: the body of k_mloo_gram and of k_mpred_cross (bnr_mpred_kernels.h).  Called by all 256 threads of workgroup (., y), draws b0 =
// y MLOO_DB .. b0 + MLOO_DB - 1.  xi / xj: this thread's row of the two row panels (row sr = tid & 31 of tile ti of Xi, of tile tj of Xj), already
// clamped into its matrix, leading dimensions ldi / ldj; vi / vj: whether that row exists.  Per K step of MLOO_KC edges the two panels and the
// draws' S are staged in LDS once; wave w owns the 16 x 16 tile (w >> 1, w & 1) of the pair and keeps one accumulator per draw: the A operand is
// xi[i][e] S_b[e] (one multiply per element and draw), the B operand xj[j][e] as staged -- the panels are read from LDS once per MFMA step for all
// MLOO_DB draws.  Padding -- rows that do not exist, edges past q, draws past B -- is the constant 0.0 chosen at staging, never memory that was not
// asked for.  K order of an entry: one accumulator, edges 0, 4, 8, ... in steps of 4, inside a step the MFMA's own order (lane group g = lane >> 4
// holds edge k + g): fixed by q alone.  The identity is added once, to the finished sum.  Entry (i, j) of the tile pair is stored at
// out + b stride + i + j np, all 32 x 32 of them.  MFMA layouts as in k_cov: A lane l = row l & 15, k = l >> 4; B lane l = k = l >> 4, column
// l & 15; D lane l, reg t = row (l >> 4) + 4 t, column l & 15.
template <bool IDENT>
__device__ __forceinline__ void mloo_gram_tile(const double *xi, int ldi, bool vi, const double *xj, int ldj, bool vj, int ti, int tj, int q,
                                               const double *const *Sp, int B, double *out, int np, long long stride)
{
    __shared__ double sXi[MLOO_KC * MLOO_LDT], sXj[MLOO_KC * MLOO_LDT], sS[MLOO_DB * MLOO_KC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
    const int b0 = (int)blockIdx.y * MLOO_DB;
    const int sr = tid & 31, sk = tid >> 5;                              // staging: row sr of a panel, edges sk, sk + 8, sk + 16, sk + 24 of the step
    const double *sp = Sp[min(b0 + sk, B - 1)];                          // staging of S: draw b0 + sk, edge sr of the step
    const bool sv = b0 + sk < B;
    const int ra = (w >> 1) * 16 + c, rb = (w & 1) * 16 + c;
    mloo_d4 acc[MLOO_DB];
#pragma unroll
    for (int d = 0; d < MLOO_DB; ++d) acc[d] = mloo_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < q; k0 += MLOO_KC) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < MLOO_KC / 8; ++p) {
            const int k = sk + 8 * p, e = k0 + k, ec = min(e, q - 1);
            const double a = xi[(size_t)ec * (size_t)ldi], b = xj[(size_t)ec * (size_t)ldj];
            sXi[k * MLOO_LDT + sr] = (e < q && vi) ? a : 0.0;
            sXj[k * MLOO_LDT + sr] = (e < q && vj) ? b : 0.0;
        }
        {
            const int e = k0 + sr;
            const double v = sp[min(e, q - 1)];
            sS[sk * MLOO_KC + sr] = (sv && e < q) ? v : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < MLOO_KC; ks += 4) {
            const int k = ks + g;
            const double xa = sXi[k * MLOO_LDT + ra], xb = sXj[k * MLOO_LDT + rb];
#pragma unroll
            for (int d = 0; d < MLOO_DB; ++d) acc[d] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa * sS[d * MLOO_KC + k], xb, acc[d], 0, 0, 0);
        }
    }
    const int col = tj * MLOO_TILE + (w & 1) * 16 + c;
#pragma unroll
    for (int d = 0; d < MLOO_DB; ++d) {
        if (b0 + d >= B) break;
        double *ob = out + (size_t)(b0 + d) * (size_t)stride;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = ti * MLOO_TILE + (w >> 1) * 16 + g + 4 * t;
            ob[(size_t)row + (size_t)col * (size_t)np] = IDENT ? acc[d][t] + (row == col ? 1.0 : 0.0) : acc[d][t];
        }
    }
}

// A_b = I + X diag(S_b) X^T for the draws of a batch, lower tiles only.  grid = (nt (nt + 1) / 2, ceil(B / MLOO_DB)) with nt = np / MLOO_TILE, 256
// threads: workgroup (p, y) is the tile pair (ti >= tj) number p, both panels rows of X.  A[(i, j)] is stored at G_b[i + j np], G_b = G + b gstride
// (i >= j within the lower tiles; the diagonal tiles whole).
__global__ __launch_bounds__(256) void k_mloo_gram(const double *X, int ldx, int n, int q, const double *const *Sp, int B, double *G, int np,
                                                   long long gstride)
{
    int ti = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const int sr = (int)threadIdx.x & 31, rowi = ti * MLOO_TILE + sr, rowj = tj * MLOO_TILE + sr;
    mloo_gram_tile<true>(X + min(rowi, n - 1), ldx, rowi < n, X + min(rowj, n - 1), ldx, rowj < n, ti, tj, q, Sp, B, G, np, gstride);
}

// ===================================================================================== k_mloo_factor
#define MLOO_UNROLL 8           // loads of each operand issued together in the substitution loops (their sums stay term by term, in order)
// s - sum_{k0 <= k < k1} a[k ld] b[k ld], k ascending, every product and difference rounded on its own; MLOO_UNROLL loads of a and of b in flight
__device__ __forceinline__ double mloo_dot_sub(double s, const double *a, const double *b, size_t ld, int k0, int k1)
{
    int k = k0;
    for (; k + MLOO_UNROLL <= k1; k += MLOO_UNROLL) {
        double av[MLOO_UNROLL], bv[MLOO_UNROLL];
#pragma unroll
        for (int t = 0; t < MLOO_UNROLL; ++t) { av[t] = a[(size_t)(k + t) * ld]; bv[t] = b[(size_t)(k + t) * ld]; }
#pragma unroll
        for (int t = 0; t < MLOO_UNROLL; ++t) s = s - av[t] * bv[t];
    }
    for (; k < k1; ++k) s = s - a[(size_t)k * ld] * b[(size_t)k * ld];
    return s;
}
// Everything behind A for one draw per workgroup (grid = B, 256 threads), in global memory: a draw owns gstride >= np (np + 1) doubles, L in the lower
// triangle of its first np columns and L^-1 above it, shifted by one column (M[r][i], r >= i, at row i of column r + 1):
//   1. left-looking Cholesky of A in place, column j = 0 .. n - 1:  s_r = A[r][j] - sum_{k < j} L[r][k] L[j][k] (k ascending), L[j][j] = sqrt(s_j),
//      L[r][j] = s_r / L[j][j]; thread t owns rows j + t, j + t + 256, ...  The right-hand side rides along as row n of the matrix, so that
//      z_j = (r_j - sum_{k < j} z_k L[j][k]) / L[j][j] is the forward substitution (thread 255; z in LDS).  A pivot that is not > 0 ends the draw.
//   2. M = L^-1 by forward substitution, column i by thread i (then i + 256, ...), rows r ascending: M[r][i] = ([r == i] - sum_{i <= k < r}
//      L[r][k] M[k][i]) / L[r][r] (k ascending; the lanes of a pass start at the pass's first column and select 0.0 for M above their own), stored at M[r np + i] -- a thread reads back only what it wrote, the lanes of a wave read one row of
//      L and consecutive entries of a row of M.  In the same pass c_i = sum_r M[r][i]^2 and g_i = sum_r M[r][i] z_r, r ascending from 0.0.
//   3. resid, var, loglik of the n rows and logml, as defined in the header of this file; out[i ldo + s] with s = s0 + b the draw's place in the call.
// A draw whose tau2, mu or S is not finite, or whose factorization meets a pivot that is not > 0, is NaN in every output and raises bad[s];
// nothing else of the call sees it.
__global__ __launch_bounds__(256) void k_mloo_factor(double *G, long long gstride, const double *r, int n, int np, int q, const double *const *Sp,
                                                     const double *tau2, const double *mu, int s0, long long ldo, double *loglik, double *resid,
                                                     double *var, double *logml, int *bad)
{
    __shared__ double zs[MLOO_MAX_N], cs[MLOO_MAX_N], gs[MLOO_MAX_N];
    __shared__ double piv;
    const int tid = threadIdx.x, b = blockIdx.x, s = s0 + b;
    double *A = G + (size_t)b * (size_t)gstride, *M = A + np;        // M[r][i] = M[r np + i] = A's (i, r + 1): above L, inside the draw's np x (np + 1) doubles
    const double *rb = r + (size_t)b * (size_t)np;
    const double t2 = tau2[b], m = mu[b];
    int nf = (isfinite(t2) && isfinite(m)) ? 0 : 1;
    {
        const double *sp = Sp[b];
        for (int e = tid; e < q; e += 256) if (!isfinite(sp[e])) nf = 1;
    }
    bool isbad = __syncthreads_or(nf) != 0;
    double sumlog = 0.0, zz = 0.0;
    if (!isbad) {
        for (int j = 0; j < n; ++j) {
            const double *Aj = A + j;                                    // L[j][k] = Aj[k np]: one address for the whole workgroup
            for (int rr = j + tid; rr < n; rr += 256) {
                double *Ar = A + rr;
                double sv = Ar[(size_t)j * np];
                sv = mloo_dot_sub(sv, Ar, Aj, (size_t)np, 0, j);
                Ar[(size_t)j * np] = sv;
                if (rr == j) piv = sv;
            }
            double zrow = 0.0;
            if (tid == 255) {
                zrow = rb[j];
                int k = 0;
                for (; k + MLOO_UNROLL <= j; k += MLOO_UNROLL) {
                    double lv[MLOO_UNROLL];
#pragma unroll
                    for (int t = 0; t < MLOO_UNROLL; ++t) lv[t] = Aj[(size_t)(k + t) * np];
#pragma unroll
                    for (int t = 0; t < MLOO_UNROLL; ++t) zrow = zrow - zs[k + t] * lv[t];
                }
                for (; k < j; ++k) zrow = zrow - zs[k] * Aj[(size_t)k * np];
            }
            __syncthreads();
            const double d = piv;
            if (!(d > 0.0)) { isbad = true; break; }                     // (the same value in every thread: the whole workgroup leaves)
            const double sd = sqrt(d);
            sumlog = sumlog + log(sd);
            for (int rr = j + tid; rr < n; rr += 256) A[(size_t)rr + (size_t)j * np] = (rr == j) ? sd : A[(size_t)rr + (size_t)j * np] / sd;
            if (tid == 255) { const double zj = zrow / sd; zs[j] = zj; zz = zz + zj * zj; }
            __syncthreads();
        }
    }
    if (!isbad) {
        for (int i0 = 0; i0 < n; i0 += 256) {
            const int i = i0 + tid;
            const bool act = i < n;
            const double *Mi = M + min(i, n - 1);                        // (a lane past n reads column n - 1 and selects 0.0: every load stays inside M)
            double cacc = 0.0, gacc = 0.0;
            for (int rr = i0; rr < n; ++rr) {
                const double *Ar = A + rr;
                double sv = (rr == i) ? 1.0 : 0.0;
                int k = i0;
                for (; k + MLOO_UNROLL <= rr; k += MLOO_UNROLL) {              // (MLOO_UNROLL loads of each operand in flight; the terms in order, one by one)
                    double lv[MLOO_UNROLL], mv[MLOO_UNROLL];
#pragma unroll
                    for (int t = 0; t < MLOO_UNROLL; ++t) { lv[t] = Ar[(size_t)(k + t) * np]; mv[t] = Mi[(size_t)(k + t) * np]; }
#pragma unroll
                    for (int t = 0; t < MLOO_UNROLL; ++t) sv = sv - lv[t] * ((act && k + t >= i) ? mv[t] : 0.0);
                }
                for (; k < rr; ++k) sv = sv - Ar[(size_t)k * np] * ((act && k >= i) ? Mi[(size_t)k * np] : 0.0);
                const double x = sv / Ar[(size_t)rr * np];
                if (act && rr >= i) { M[(size_t)rr * np + i] = x; cacc = cacc + x * x; gacc = gacc + x * zs[rr]; }
            }
            if (act) { cs[i] = cacc; gs[i] = gacc; }
        }
    }
    __syncthreads();
    if (tid == 0) bad[s] = isbad ? 1 : 0;
    const double nanv = __builtin_nan("");
    for (int i = tid; i < n; i += 256) {
        double rs = nanv, vr = nanv, ll = nanv;
        if (!isbad) {
            const double ci = cs[i];
            rs = gs[i] / ci;
            vr = t2 / ci;
            ll = -0.5 * (MLOO_LOG_2PI + log(vr)) - 0.5 * ((rs * rs) / vr);
        }
        const size_t o = (size_t)i * (size_t)ldo + (size_t)s;
        if (resid) resid[o] = rs;
        if (var) var[o] = vr;
        if (loglik) loglik[o] = ll;
    }
    if (logml && tid == 255) logml[s] = isbad ? nanv : -(0.5 * (double)n) * (MLOO_LOG_2PI + log(t2)) - sumlog - 0.5 * (zz / t2);
}
