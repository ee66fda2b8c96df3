// bnr_analysis_kernels.h -- gfx950 kernels of the posterior analysis (additions to the reference): prediction, log-likelihood, PSIS-LOO and its
// predictive checks, rank-normalised diagnostics, highest-density intervals.  Compiled into bnr_analysis.hip alone: a code object of their own,
// so that nothing here can move a kernel of the sweep (bnr_kernels.h).
#pragma once
#include "bnr_device.h"

// ===================================================================================== posterior prediction (an addition to the reference)
// The mean response of a row x under draw s of the window is eta_s = mu_s + x . gamma_s (y = mu + X gamma + eps, gibbs.jl:270, 432, 566).
//
// k_predict: E[i lde + s] = mu_s + sum_e X[i, e] gamma_s[e] for the rows i < mrows of a block and the samples s < nsamp (lde = nsamp for one
// chain; the pooled draw count where the launches of several chains fill the columns c nsamp .. of one E), by
// v_mfma_f64_16x16x4_f64 with A = a 16-row tile of X, B = gamma^T of 16 samples.  X: column-major, leading dimension ldx, zero in
// the columns q .. q16 - 1 (q16 = q rounded up to 16) and readable (zero) for 16 TI rows of every tile; gamma_s: trace row
// first0 + s at o_gamma, K-contiguous (the columns q .. q16 - 1 of a trace row are the zero padding in front of S).
// K order: one accumulator per output, k0 = 0, 16, ... < q16; inside a step the MFMA t (0..3) takes k = k0 + 4 g + t from lane group
// g = lane >> 4 -- so a lane reads 32 contiguous bytes of its gamma row per step, and X one coalesced 128-byte column piece per
// (tile, t).  The order of an output's sum is fixed by q alone (not by the grid, the block of rows, m or nsamp); its place in an MFMA
// tile is (i mod 16, s mod 16) whatever the launch.  D layout of the f64 MFMA: lane l, reg r = row (l >> 4) + 4 r, column l & 15.
// grid = (ceil(nsamp / 128), ceil(mrows / (16 TI))), 256 threads: wave w owns samples blockIdx.x 128 + 32 w .. + 31 and the TI row
// tiles of blockIdx.y.  Samples past nsamp read the last sample's row and are not stored.
template <int TI>
__global__ __launch_bounds__(256) void k_predict(const double *X, int ldx, int q16, const double *trace, int rowlen, int o_gamma, int first0,
                                                 int nsamp, int mrows, double *E, long long lde)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int i0 = blockIdx.y * 16 * TI, s0 = blockIdx.x * 128 + w * 32;
    if (s0 >= nsamp) return;
    const double *xa[TI];
#pragma unroll
    for (int a = 0; a < TI; ++a) xa[a] = X + (size_t)(i0 + 16 * a + c) + (size_t)ldx * (4 * g);
    const double *gb[2];
    double mu[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const double *row = trace + (size_t)(first0 + min(s0 + 16 * b + c, nsamp - 1)) * rowlen;
        gb[b] = row + o_gamma + 4 * g;
        mu[b] = row[ROW_MU];
    }
    const size_t xstep = (size_t)ldx * 16;
    bnr_d4 acc[TI][2];
#pragma unroll
    for (int a = 0; a < TI; ++a) { acc[a][0] = bnr_d4{0.0, 0.0, 0.0, 0.0}; acc[a][1] = bnr_d4{0.0, 0.0, 0.0, 0.0}; }
    for (int k0 = 0; k0 < q16; k0 += 16) {
        double av[TI][4];
#pragma unroll
        for (int a = 0; a < TI; ++a) {
#pragma unroll
            for (int t = 0; t < 4; ++t) av[a][t] = xa[a][(size_t)ldx * t];
            xa[a] += xstep;
        }
        const bnr_d4 b0 = *(const bnr_d4 *)(gb[0] + k0), b1 = *(const bnr_d4 *)(gb[1] + k0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int a = 0; a < TI; ++a) {
                acc[a][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][t], b0[t], acc[a][0], 0, 0, 0);
                acc[a][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][t], b1[t], acc[a][1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int s = s0 + 16 * b + c;
        if (s >= nsamp) continue;
#pragma unroll
        for (int a = 0; a < TI; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * a + g + 4 * r;
                if (i < mrows) E[(size_t)i * (size_t)lde + s] = mu[b] + acc[a][b][r];
            }
    }
}

// k_pred_loglik: pointwise log predictive density and WAIC penalty of the observed responses y[i] of the rows of a block, from the
// column E[i nsamp ..] of k_predict and tau2_s (fetched by k_fetch_cols):  l_s = -(log 2 pi + log tau2_s) / 2 - (y_i - E_is)^2 / (2 tau2_s),
// lpd_i = max_s l_s + log(sum_s exp(l_s - max) / nsamp) (log-mean-exp), pwaic_i = Var_s(l_s) (ddof 1, two passes).  One workgroup of
// 256 threads per row; every sum in the fixed order of k_summary (thread-strided partial sums, then a tree).
#define BNR_LOG_2PI 1.8378770664093454836
// l_s = log N(y_i | E_is, tau2_s), one expression for k_pred_loglik and k_psis (the library is built with -ffp-contract=off, so both get it bit for bit)
__device__ __forceinline__ double bnr_pred_ell(double yi, double e, double t)
{
    const double r = yi - e;
    return -0.5 * (BNR_LOG_2PI + log(t)) - r * r / (2.0 * t);
}
__global__ __launch_bounds__(256) void k_pred_loglik(const double *E, int nsamp, const double *y, const double *tau2, double *lpd, double *pwaic)
{
    __shared__ double ra[256], rb[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *e = E + (size_t)i * nsamp;
    const double yi = y[i];
    auto ell = [&](int s) { return bnr_pred_ell(yi, e[s], tau2[s]); };
    double mx = -INFINITY, sum = 0.0;
    for (int s = tid; s < nsamp; s += 256) { const double l = ell(s); mx = fmax(mx, l); sum += l; }
    ra[tid] = mx; rb[tid] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { ra[tid] = fmax(ra[tid], ra[tid + w]); rb[tid] += rb[tid + w]; } __syncthreads(); }
    const double M = ra[0], mean = rb[0] / nsamp;
    __syncthreads();
    double se = 0.0, sv = 0.0;
    for (int s = tid; s < nsamp; s += 256) { const double l = ell(s), dl = l - mean; se += exp(l - M); sv += dl * dl; }
    ra[tid] = se; rb[tid] = sv;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { ra[tid] += ra[tid + w]; rb[tid] += rb[tid + w]; } __syncthreads(); }
    if (tid == 0) { lpd[i] = M + log(ra[0] / nsamp); pwaic[i] = rb[0] / (nsamp - 1); }
}

// ===================================================================================== PSIS-LOO (an addition to the reference)
// Pareto-smoothed importance sampling leave-one-out over the draws s < nsamp of a row, as loo 2.x (Vehtari, Gelman & Gabry 2017; psis.R,
// gpdfit.R): log ratios r_s = -l_s, lw_s = r_s - max r; with the tail length M = tail_len[i] >= 5 and a tail of spread >= DBL_EPSILON / 100
// the M largest lw are replaced by the quantiles of a generalized Pareto fit (Zhang & Stephens 2009 with the weakly informative prior) above
// the cutoff, the (M+1)-th largest lw; then lw <- min(lw, 0) and
//   lpd_i = log mean_s exp(l_s)                       (k_pred_loglik's expression and reduction order: bit for bit its lpd)
//   elpd_i = log sum_s exp(lw_s + l_s) - log sum_s exp(lw_s)
//   khat_i = the fitted shape after the prior adjustment; +inf when there is no fit (M < 5, a constant tail, a NaN shape).
// A row with a non-finite l gets elpd NaN, khat +inf.
// Two kernels do this, k_psis (lpd, elpd, khat) and k_psis_w (the per-draw weights as well); what they share is the bnr_psis_* pieces below,
// one source for both, and this contract.  One workgroup of 256 threads per row (blockIdx.x); FROM_E = 1: the row comes as its E column of
// k_predict, l_s = bnr_pred_ell(y_i, E_is, tau2_s); FROM_E = 0: as its l row.  The row is streamed from L2 / HBM on every pass:
//   1  l, its max and min, finiteness (bnr_psis_pass1);  2  sum exp(l - max) (lpd) and the first digit histogram;  3-7  the other digit
//   histograms: exact radix select of K_c, the (M+1)-th largest order-preserving 64-bit key of lw (11-bit digits, 6 passes, integer LDS
//   atomics: exact; bnr_psis_cutoff);  8  gather: the tail into LDS, the per-thread log-sum-exps of the rest.
// The tail is sorted with a bitonic sort in LDS (P entries, P = the smallest power of two >= M, the padding behind the tail), fitted
// (bnr_psis_gpd_fit) and its M terms, smoothed or as they were (bnr_psis_tail_lw), join the log-sum-exps (bnr_psis_lse_tree).  Which draws
// with a key equal to K_c belong to the tail, what a tail entry carries beside its key, and what is written back are each kernel's own.
// Every sum is in a fixed order (thread-strided partial sums, then a tree; the GPD grid: lane-strided partial sums, then a fixed butterfly of
// the wave), so results are bitwise independent of the grid, of the block of rows and of the call.  Dynamic LDS: max(8 KiB, entry bytes x P)
// for the largest M of the launch; M <= BNR_PSIS_MAX_TAIL (the host refuses longer tails).
#define BNR_PSIS_MAX_TAIL 8192
#define BNR_PSIS_MAX_GRID 128          // 30 + floor(sqrt(BNR_PSIS_MAX_TAIL)) = 120 grid points
__device__ __forceinline__ unsigned long long bnr_okey(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double bnr_okey_inv(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
// running log-sum-exp: sum = s exp(m); a NaN term makes the sum NaN
__device__ __forceinline__ void bnr_lse_merge(double &m, double &s, double m2, double s2)
{
    if (isnan(m2) || isnan(s2)) s = NAN;
    else if (m2 > m) { s = s * exp(m - m2) + s2; m = m2; }
    else if (m2 > -INFINITY) s += s2 * exp(m2 - m);
}
// the static LDS of a PSIS workgroup: four reduction arrays, the GPD grid's log-likelihoods and the broadcast scalars
struct bnr_psis_lds {
    double ra[256], rb[256], rc[256], rd[256], lth[BNR_PSIS_MAX_GRID];
    double theta;
    unsigned bin, above, cnt, pos;
};
// the sum / the max of v over the 256 threads in k_pred_loglik's tree, through ra; every thread gets it.  No barrier behind the last read of ra[0]
__device__ __forceinline__ double bnr_block_sum(double *ra, int tid, double v)
{
    ra[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) ra[tid] += ra[tid + w]; __syncthreads(); }
    return ra[0];
}
__device__ __forceinline__ double bnr_block_max(double *ra, int tid, double v)
{
    ra[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) ra[tid] = fmax(ra[tid], ra[tid + w]); __syncthreads(); }
    return ra[0];
}
// (wave 0) the bin of a histogram that holds its want-th largest entry: lane owns the bins [lane per, lane per + per), suffix sums over the
// lanes find the owner; *above = the entries in higher bins, *cnt = the bin's own
__device__ __forceinline__ void bnr_hist_pick(const unsigned *hist, int nbins, unsigned want, int lane, unsigned *bin, unsigned *above, unsigned *cnt)
{
    const int per = nbins / 64;
    unsigned c = 0;
    for (int b = 0; b < per; ++b) c += hist[lane * per + b];
    unsigned suf = c;
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_down(suf, o); if (lane + o < 64) suf += t; }
    const unsigned long long ge = __ballot(suf >= want);
    const int owner = 63 - __clzll((long long)ge);
    if (lane == owner) {
        unsigned acc = suf - c;
        for (int b = per - 1; b >= 0; --b) {
            const unsigned h = hist[lane * per + b];
            if (acc + h >= want) { *bin = (unsigned)(lane * per + b); *above = acc; *cnt = h; break; }
            acc += h;
        }
    }
}
// pass 1: the row's l (from src; stored to dst when `store`), lmax = max l, rmax = max r = -min l; returns nonzero when an l is not finite
template <int FROM_E>
__device__ __forceinline__ int bnr_psis_pass1(const double *src, double *dst, bool store, int nsamp, const double *y, int i, const double *tau2,
                                              bnr_psis_lds &sh, int tid, double &lmax, double &rmax)
{
    double mx = -INFINITY, mn = INFINITY;
    int bad = 0;
    for (int s = tid; s < nsamp; s += 256) {
        const double v = FROM_E ? bnr_pred_ell(y[i], src[s], tau2[s]) : src[s];
        if (store) dst[s] = v;
        mx = fmax(mx, v); mn = fmin(mn, v);
        bad |= !isfinite(v);
    }
    sh.ra[tid] = mx; sh.rb[tid] = mn;
    bad = __syncthreads_or(bad);
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { sh.ra[tid] = fmax(sh.ra[tid], sh.ra[tid + w]); sh.rb[tid] = fmin(sh.rb[tid], sh.rb[tid + w]); } __syncthreads(); }
    lmax = sh.ra[0]; rmax = -sh.rb[0];
    __syncthreads();
    return bad;
}
// passes 2-7: radix select of K_c, the (M+1)-th largest key of lw = -l - rmax (select: the row is finite and M >= 5; otherwise pass 2 alone and
// K_c = all ones: no tail).  want - 1 of the cnt_eq keys == K_c rank above the cutoff, `above` keys are > K_c; se = this thread's part of
// sum_s exp(l_s - lmax) (pass 2).  hist: 2048 unsigned of dynamic LDS
__device__ __forceinline__ unsigned long long bnr_psis_cutoff(const double *l, int nsamp, bool select, int M, double lmax, double rmax, unsigned *hist,
                                                              bnr_psis_lds &sh, int tid, unsigned &want, unsigned &above, unsigned &cnt_eq, double &se)
{
    unsigned long long prefix = 0, mask = 0;
    want = (unsigned)M + 1; above = 0; cnt_eq = 0;
    se = 0.0;
    for (int p = 0; p < 6; ++p) {
        const int shift = p < 5 ? 53 - 11 * p : 0, nbins = p < 5 ? 2048 : 512;
        if (select) {
            for (int b = tid; b < nbins; b += 256) hist[b] = 0u;
            __syncthreads();
        }
        for (int s = tid; s < nsamp; s += 256) {
            const double v = l[s];
            if (p == 0) se += exp(v - lmax);
            if (select) {
                const unsigned long long k = bnr_okey(-v - rmax);
                if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & (unsigned)(nbins - 1)], 1u);
            }
        }
        if (!select) break;
        __syncthreads();
        if ((tid >> 6) == 0) bnr_hist_pick(hist, nbins, want, tid & 63, &sh.bin, &sh.above, &sh.cnt);
        __syncthreads();
        prefix |= (unsigned long long)sh.bin << shift;
        mask |= (unsigned long long)(nbins - 1) << shift;
        above += sh.above; want -= sh.above; cnt_eq = sh.cnt;
        __syncthreads();
    }
    return select ? prefix : ~0ull;
}
// the generalized Pareto fit of a tail; kh = +inf, smooth = false: no fit
struct bnr_psis_fit {
    double kh, sigma, ec;
    bool smooth;
};
// gpdfit (Zhang & Stephens with loo's prior on k) on x_j = exp(lw_(j)) - exp(cutoff), lw_(j) = the sorted keys tk[0 .. M - 1], ascending;
// a tail narrower than .Machine$double.eps / 100 is not fitted.  Reads other threads' keys up to its last barrier-free statement: the caller
// puts a barrier before it overwrites one
__device__ __forceinline__ bnr_psis_fit bnr_psis_gpd_fit(const unsigned long long *tk, int M, unsigned long long Kc, bnr_psis_lds &sh, int tid)
{
    const int lane = tid & 63, wv = tid >> 6;
    bnr_psis_fit f{INFINITY, 0.0, 0.0, false};
    const double cutoff = bnr_okey_inv(Kc);
    const double lo = bnr_okey_inv(tk[0]), hi = bnr_okey_inv(tk[M - 1]);
    if (fabs(hi - lo) < 2.220446049250313e-16 / 100) return f;
    const double ec = exp(cutoff);
    auto xv = [&](int j) { return exp(bnr_okey_inv(tk[j])) - ec; };
    const double xN = xv(M - 1), xstar = xv((int)floor(M / 4.0 + 0.5) - 1);
    const int mg = 30 + (int)floor(sqrt((double)M));
    auto theta = [&](int j) { return 1.0 / xN + (1.0 - sqrt((double)mg / ((double)j + 0.5))) / 3.0 / xstar; };
    for (int j = wv; j < mg; j += 4) {
        const double a = -theta(j);
        double acc = 0.0;
        for (int t = lane; t < M; t += 64) acc += log1p(a * xv(t));
        acc += __shfl_xor(acc, 32); acc += __shfl_xor(acc, 16); acc += __shfl_xor(acc, 8);
        acc += __shfl_xor(acc, 4); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 1);
        const double kj = acc / M;
        if (lane == 0) sh.lth[j] = M * (log(a / kj) - kj - 1.0);
    }
    __syncthreads();
    if (tid == 0) {
        // weights exp(l_j - logSumExp(l)) with matrixStats' logSumExp (max + log1p of the sum over the other points)
        int jm = 0;
        for (int j = 1; j < mg; ++j) if (sh.lth[j] > sh.lth[jm]) jm = j;
        const double lm = sh.lth[jm];
        double sum = 0.0;
        for (int j = 0; j < mg; ++j) if (j != jm) sum += exp(sh.lth[j] - lm);
        const double lse = lm + log1p(sum);
        double th = 0.0;
        for (int j = 0; j < mg; ++j) th += theta(j) * exp(sh.lth[j] - lse);
        sh.theta = th;
    }
    __syncthreads();
    const double th = sh.theta;
    double acc = 0.0;
    for (int t = tid; t < M; t += 256) acc += log1p(-th * xv(t));
    const double k0 = bnr_block_sum(sh.ra, tid, acc) / M;
    f.ec = ec;
    f.sigma = -k0 / th;
    f.kh = k0 * M / (M + 10) + 10 * 0.5 / (M + 10);
    if (isnan(f.kh)) f.kh = INFINITY;
    f.smooth = isfinite(f.kh);
    return f;
}
// the log weight of position j of the sorted tail: the j-th qgpd quantile above the cutoff, or the key as it was; truncated at 0
__device__ __forceinline__ double bnr_psis_tail_lw(const bnr_psis_fit &f, const unsigned long long *tk, int j, int M)
{
    double lw;
    if (f.smooth) {
        const double pj = ((double)j + 0.5) / M;
        const double qq = (isnan(f.sigma) || f.sigma <= 0.0) ? NAN : f.sigma * expm1(-f.kh * log1p(-pj)) / f.kh;
        lw = log(qq + f.ec);
    } else lw = bnr_okey_inv(tk[j]);
    return lw > 0.0 ? 0.0 : lw;
}
// the threads' running log-sum-exps (mA, sA) and (mB, sB) merged in a tree: (ra[0], rb[0]) and (rc[0], rd[0]) hold the two totals
__device__ __forceinline__ void bnr_psis_lse_tree(bnr_psis_lds &sh, int tid, double mA, double sA, double mB, double sB)
{
    __syncthreads();                                   // (every thread has read ra[0] of the sums before)
    sh.ra[tid] = mA; sh.rb[tid] = sA; sh.rc[tid] = mB; sh.rd[tid] = sB;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            double m1 = sh.ra[tid], s1 = sh.rb[tid], m2 = sh.rc[tid], s2 = sh.rd[tid];
            bnr_lse_merge(m1, s1, sh.ra[tid + w], sh.rb[tid + w]);
            bnr_lse_merge(m2, s2, sh.rc[tid + w], sh.rd[tid + w]);
            sh.ra[tid] = m1; sh.rb[tid] = s1; sh.rc[tid] = m2; sh.rd[tid] = s2;
        }
        __syncthreads();
    }
}

// k_psis: lpd, elpd and khat of a row.  L + i nsamp holds the row; FROM_E = 1 writes l back over E in pass 1.  A tail entry is its key and its l
// (16 bytes).  Ties: the tail is every key > K_c plus (M - #{key > K_c}) copies of (K_c, l_c), l_c = max l over key == K_c (found in pass 8); the
// other keys == K_c enter the sums as a counted multiple of (K_c, l_c).  Tied ratios have tied l, so this is the tail any sort would pick; a tie
// created only by the rounding of r - max r moves a result by an ulp of that l.  The tail is sorted by (key, key of l).
template <int FROM_E>
__global__ __launch_bounds__(256) void k_psis(double *L, int nsamp, const double *y, const double *tau2, const int *tail_len, double *lpd,
                                              double *elpd, double *khat)
{
    extern __shared__ unsigned long long psis_dyn[];
    __shared__ bnr_psis_lds sh;
    const int i = blockIdx.x, tid = threadIdx.x;
    double *l = L + (size_t)i * nsamp;
    const int M = tail_len[i];

    double lmax, rmax, se;
    const int bad = bnr_psis_pass1<FROM_E>(l, l, FROM_E != 0, nsamp, y, i, tau2, sh, tid, lmax, rmax);
    const bool select = !bad && M >= 5;
    unsigned want, above_all, cnt_eq;
    const unsigned long long Kc = bnr_psis_cutoff(l, nsamp, select, M, lmax, rmax, (unsigned *)psis_dyn, sh, tid, want, above_all, cnt_eq, se);
    se = bnr_block_sum(sh.ra, tid, se);
    if (tid == 0 && lpd) lpd[i] = lmax + log(se / nsamp);
    __syncthreads();
    if (bad) {
        if (tid == 0) { elpd[i] = NAN; khat[i] = INFINITY; }
        return;
    }

    // pass 8: the tail (keys > K_c) into LDS, l_c, and the log-sum-exps of every other draw
    const int P = select ? (int)(1u << (32 - __clz(M - 1))) : 0;        // the smallest power of two >= M
    unsigned long long *tk = psis_dyn;
    double *tl = (double *)(psis_dyn + P);
    if (tid == 0) sh.pos = 0u;
    __syncthreads();
    double mA = -INFINITY, sA = 0.0, mB = -INFINITY, sB = 0.0, lc = -INFINITY;
    for (int s = tid; s < nsamp; s += 256) {
        const double v = l[s], lw = -v - rmax;
        const unsigned long long k = bnr_okey(lw);
        if (k > Kc) {
            const unsigned pos = atomicAdd(&sh.pos, 1u);
            if (pos < (unsigned)M) { tk[pos] = k; tl[pos] = v; }
        } else if (k == Kc) lc = fmax(lc, v);
        else { bnr_lse_merge(mA, sA, lw + v, 1.0); bnr_lse_merge(mB, sB, lw, 1.0); }
    }
    bnr_psis_fit f{INFINITY, 0.0, 0.0, false};
    if (select) {
        lc = bnr_block_max(sh.ra, tid, lc);
        const int g = (int)above_all;                  // #{key > K_c}; M - g copies of (K_c, l_c) complete the tail
        for (int j = g + tid; j < P; j += 256) {
            if (j < M) { tk[j] = Kc; tl[j] = lc; }
            else { tk[j] = ~0ull; tl[j] = 0.0; }
        }
        __syncthreads();
        // bitonic sort of (key, key of l) ascending; the padding (all-ones keys) ends behind the tail
        for (int kk = 2; kk <= P; kk <<= 1)
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                for (int t = tid; t < P / 2; t += 256) {
                    const int a = (t / jj) * 2 * jj + (t % jj), b = a + jj;
                    const unsigned long long ka = tk[a], kb = tk[b];
                    const bool gt = ka > kb || (ka == kb && bnr_okey(tl[a]) > bnr_okey(tl[b]));
                    if (gt == ((a & kk) == 0)) {
                        tk[a] = kb; tk[b] = ka;
                        const double x = tl[a]; tl[a] = tl[b]; tl[b] = x;
                    }
                }
                __syncthreads();
            }
        f = bnr_psis_gpd_fit(tk, M, Kc, sh, tid);
        for (int j = tid; j < M; j += 256) {
            const double lw = bnr_psis_tail_lw(f, tk, j, M);
            bnr_lse_merge(mA, sA, lw + tl[j], 1.0);
            bnr_lse_merge(mB, sB, lw, 1.0);
        }
    }
    bnr_psis_lse_tree(sh, tid, mA, sA, mB, sB);
    if (tid == 0) {
        double m1 = sh.ra[0], s1 = sh.rb[0], m2 = sh.rc[0], s2 = sh.rd[0];
        if (select) {
            const double ne = (double)(cnt_eq - (want - 1)), lwc = bnr_okey_inv(Kc);   // the keys == K_c outside the tail
            if (ne > 0) { bnr_lse_merge(m1, s1, lwc + lc, ne); bnr_lse_merge(m2, s2, lwc, ne); }
        }
        elpd[i] = (m1 + log(s1)) - (m2 + log(s2));
        khat[i] = f.kh;
    }
}

// ===================================================================================== predictive interval and PIT (additions to the reference)
// Both kernels work on a block of E as k_predict left it (row i's S pooled draws contiguous, leading dimension lde = S) and on the S-vector of
// tau2 fetched chain by chain.
//
// k_pred_noise: E_is <- E_is + sqrt(tau2_s) z_is in place: a draw of a NEW observation y~ = eta + eps, eps ~ N(0, tau2_s), of row i under pooled draw s.
// z_is = bnr_normal(seed, it = s, SITE_PRED, elem = row0 + i, att = 0): keyed by the pooled draw index and the row's index in the caller's m rows
// (row0 = first row of the block), so a draw does not depend on the block size, the grid, the input format or earlier calls, and the host gets the
// same number from bnr_host_pred_noise (same source; the library is built with -ffp-contract=off, so product and sum round separately on both sides).
// grid = (ceil(S / 256), rows in parallel <= mrows), 256 threads: a thread owns ONE draw s (sqrt(tau2_s) once) and walks the rows blockIdx.y,
// blockIdx.y + gridDim.y, ...; a wave reads and writes 512 contiguous bytes per row.  One pass over 8 mrows S bytes each way; per element one
// Philox-4x32-10, a log, a sqrt and bnr_cos2pi -- some 10^2 f64 and quarter-rate 32-bit multiply instructions per 16 bytes of traffic, so the
// kernel is bound by the vector ALUs, not by HBM.  64-bit addressing; no LDS, no scratch.
__global__ __launch_bounds__(256) void k_pred_noise(double *E, long long lde, int S, int mrows, int row0, const double *tau2, unsigned long long seed)
{
    const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (s >= S) return;
    const double sd = sqrt(tau2[s]);
    for (int i = (int)blockIdx.y; i < mrows; i += (int)gridDim.y) {
        double *e = E + (size_t)i * (size_t)lde + (size_t)s;
        const double z = bnr_normal((uint64_t)seed, (uint32_t)s, SITE_PRED, (uint32_t)(row0 + i), 0u);
        *e = *e + sd * z;
    }
}

// k_pred_pit: the probability integral transform of the observed response y_i under the posterior predictive, Rao-Blackwellised over the draws:
// pit_i = (1 / S) sum_s Phi((y_i - E_is) / sqrt(tau2_s)), Phi(z) = erfc(-z / sqrt 2) / 2.  No random numbers.  One workgroup of 256 threads per
// row; the sum in the fixed order of k_pred_loglik (thread-strided partial sums, then a tree): bitwise independent of the grid and the block of rows.
#define BNR_SQRT2 1.41421356237309504880
__global__ __launch_bounds__(256) void k_pred_pit(const double *E, int nsamp, const double *y, const double *tau2, double *pit)
{
    __shared__ double ra[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *e = E + (size_t)i * nsamp;
    const double yi = y[i];
    double acc = 0.0;
    for (int s = tid; s < nsamp; s += 256) {
        const double z = (yi - e[s]) / sqrt(tau2[s]);
        acc += 0.5 * erfc(-z / BNR_SQRT2);
    }
    ra[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) ra[tid] += ra[tid + w]; __syncthreads(); }
    if (tid == 0) pit[i] = ra[0] / nsamp;
}

// ===================================================================================== LOO predictive checks (ABI 11; additions to the reference)
// The PSIS weights themselves and, on top of them, the leave-one-out posterior predictive of every row: mean, standard deviation, PIT and the
// quantiles of the mixture CDF.
//
// k_psis_w: the PSIS of k_psis's header with the per-draw weights kept.  In: the row's eta (FROM_E = 1) or its l row (FROM_E = 0), read once and
// never written.  Out: LW + i nsamp, the NORMALISED log weights lw_s - logsumexp_s lw_s (loo's weights(normalize = TRUE, log = TRUE)) after
// smoothing and truncation at 0; lpd (the shared passes 1-2: k_psis's, bit for bit), elpd = log sum_s w_s exp(l_s) from the same weights, khat.
// A row with a non-finite l: LW all NaN, elpd NaN, khat +inf.
// l is written to LW in pass 1 and overwritten by the weights at the end (not recomputed from eta on every pass: a log and a division per
// draw and pass against one 8-byte read that the pass needs in either form; it also makes the two instantiations one code path behind pass 1).
// Its own passes: [7a-7c only when keys equal to K_c belong to the tail: radix select over the DRAW INDEX among the keys == K_c, 11 + 11 + 10
// bits, of s_c, the t-th largest such index]; 8 gathers (key, draw); 9 the weights.
// Tail and ties: the tail is the M draws largest in the lexicographic order (lw, s) -- what a stable ascending argsort of lw picks -- i.e.
// key > K_c, or key == K_c and s >= s_c; the composite key has no ties, so after the bitonic sort of (key, s) in LDS position j is one
// definite draw and gets the j-th GPD quantile.  A tail entry is the key (8 bytes) and the draw index (4 bytes); its l is read back from
// LW[s].  Dynamic LDS: 96 KiB at M = BNR_PSIS_MAX_TAIL, which with the static LDS fits the CU's 160 KiB -- the longest tail is k_psis's,
// nothing more is refused.  The smoothed tail is scattered back to LW[s] behind a barrier.  Against k_psis, elpd and khat differ only in the
// order of tied terms and of the tail's sums.
// 120 VGPRs, 96 SGPRs, 9 504 bytes of static LDS, no scratch (kernel-resource-usage, gfx950: 4 waves per SIMD); with the dynamic LDS -- 24 KiB
// at the headline's pooled tail of 1 200 draws -- 4 workgroups per CU, one at the longest tail.
#define BNR_PSISW_ENTRY_BYTES 12       // a tail entry of k_psis_w in LDS: the key (8) and the draw index (4); the host sizes the dynamic LDS with it
template <int FROM_E>
__global__ __launch_bounds__(256) void k_psis_w(const double *Lin, int nsamp, const double *y, const double *tau2, const int *tail_len, double *LW,
                                                double *lpd, double *elpd, double *khat)
{
    extern __shared__ unsigned long long psisw_dyn[];
    __shared__ bnr_psis_lds sh;
    __shared__ double s_logz;
    const int i = blockIdx.x, tid = threadIdx.x;
    double *l = LW + (size_t)i * nsamp;
    const int M = tail_len[i];

    double lmax, rmax, se;
    const int bad = bnr_psis_pass1<FROM_E>(Lin + (size_t)i * nsamp, l, true, nsamp, y, i, tau2, sh, tid, lmax, rmax);
    const bool select = !bad && M >= 5;
    unsigned *hist = (unsigned *)psisw_dyn;
    unsigned want, above_all, cnt_eq;
    const unsigned long long Kc = bnr_psis_cutoff(l, nsamp, select, M, lmax, rmax, hist, sh, tid, want, above_all, cnt_eq, se);
    se = bnr_block_sum(sh.ra, tid, se);
    if (tid == 0 && lpd) lpd[i] = lmax + log(se / nsamp);
    __syncthreads();
    if (bad) {
        for (int s = tid; s < nsamp; s += 256) l[s] = NAN;
        if (tid == 0) { if (elpd) elpd[i] = NAN; if (khat) khat[i] = INFINITY; }
        return;
    }

    // passes 7a-7c: want - 1 of the keys == K_c belong to the tail: those of the largest draw index.  s_c = the (want - 1)-th largest
    // draw index among them (no such pass without a tie at the cutoff: want == 1)
    unsigned sc = 0xFFFFFFFFu;
    if (select && want > 1u) {
        unsigned ipre = 0, imask = 0, iwant = want - 1u;
        for (int p = 0; p < 3; ++p) {
            const int shift = p == 0 ? 21 : p == 1 ? 10 : 0, nbins = p < 2 ? 2048 : 1024;
            for (int b = tid; b < nbins; b += 256) hist[b] = 0u;
            __syncthreads();
            for (int s = tid; s < nsamp; s += 256) {
                if (bnr_okey(-l[s] - rmax) == Kc && ((unsigned)s & imask) == ipre) atomicAdd(&hist[((unsigned)s >> shift) & (unsigned)(nbins - 1)], 1u);
            }
            __syncthreads();
            if ((tid >> 6) == 0) bnr_hist_pick(hist, nbins, iwant, tid & 63, &sh.bin, &sh.above, &sh.cnt);
            __syncthreads();
            ipre |= sh.bin << shift;
            imask |= (unsigned)(nbins - 1) << shift;
            iwant -= sh.above;
            __syncthreads();
        }
        sc = ipre;
    }

    // pass 8: the tail (key, draw) into LDS and the log-sum-exps of every other draw
    const int P = select ? (int)(1u << (32 - __clz(M - 1))) : 0;        // the smallest power of two >= M
    unsigned long long *tk = psisw_dyn;
    unsigned *ts = (unsigned *)(psisw_dyn + P);
    if (tid == 0) sh.pos = 0u;
    __syncthreads();
    double mA = -INFINITY, sA = 0.0, mB = -INFINITY, sB = 0.0;
    for (int s = tid; s < nsamp; s += 256) {
        const double v = l[s], lw = -v - rmax;
        const unsigned long long k = bnr_okey(lw);
        if (k > Kc || (k == Kc && (unsigned)s >= sc)) {
            const unsigned pos = atomicAdd(&sh.pos, 1u);
            if (pos < (unsigned)M) { tk[pos] = k; ts[pos] = (unsigned)s; }
        } else { bnr_lse_merge(mA, sA, lw + v, 1.0); bnr_lse_merge(mB, sB, lw, 1.0); }
    }
    double kh = INFINITY;
    if (select) {
        __syncthreads();
        for (int j = (int)min(sh.pos, (unsigned)M) + tid; j < P; j += 256) { tk[j] = ~0ull; ts[j] = 0xFFFFFFFFu; }     // (exactly M draws were gathered: j = M ..)
        __syncthreads();
        // bitonic sort of (key, draw) ascending; the padding ends behind the tail
        for (int kk = 2; kk <= P; kk <<= 1)
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                for (int t = tid; t < P / 2; t += 256) {
                    const int a = (t / jj) * 2 * jj + (t % jj), b = a + jj;
                    const unsigned long long ka = tk[a], kb = tk[b];
                    const unsigned sa = ts[a], sb = ts[b];
                    const bool gt = ka > kb || (ka == kb && sa > sb);
                    if (gt == ((a & kk) == 0)) { tk[a] = kb; tk[b] = ka; ts[a] = sb; ts[b] = sa; }
                }
                __syncthreads();
            }
        const bnr_psis_fit f = bnr_psis_gpd_fit(tk, M, Kc, sh, tid);
        kh = f.kh;
        // the tail's log weights, kept in place of the key.  The barrier ends every read of another thread's key (lo / hi and the x_j of the
        // fit): on the path without a fit there is none since the sort's, and the loop below overwrites tk[0] and tk[M - 1].  Behind it a
        // thread touches only the entries j it owns.
        __syncthreads();
        for (int j = tid; j < M; j += 256) {
            const double lw = bnr_psis_tail_lw(f, tk, j, M);
            if (ts[j] >= (unsigned)nsamp) continue;    // (never: the padding's index; keeps every access inside the row)
            bnr_lse_merge(mA, sA, lw + l[ts[j]], 1.0);
            bnr_lse_merge(mB, sB, lw, 1.0);
            tk[j] = (unsigned long long)__double_as_longlong(lw);
        }
    }
    bnr_psis_lse_tree(sh, tid, mA, sA, mB, sB);
    if (tid == 0) {
        const double lz = sh.rc[0] + log(sh.rd[0]);    // logsumexp_s lw_s
        s_logz = lz;
        if (elpd) elpd[i] = (sh.ra[0] + log(sh.rb[0])) - lz;
        if (khat) khat[i] = kh;
    }
    __syncthreads();
    // pass 9: the normalised log weights of the draws outside the tail over their l, then (behind a barrier: the pass reads the tail's l to
    // tell its draws) the tail's, scattered from LDS
    const double lz = s_logz;
    for (int s = tid; s < nsamp; s += 256) {
        const double lw = -l[s] - rmax;
        const unsigned long long k = bnr_okey(lw);
        if (!(k > Kc || (k == Kc && (unsigned)s >= sc))) l[s] = lw - lz;
    }
    __syncthreads();
    if (select)
        for (int j = tid; j < M; j += 256) if (ts[j] < (unsigned)nsamp) l[ts[j]] = __longlong_as_double((long long)tk[j]) - lz;
}

// k_inv_sd: isd_s = 1 / sqrt(tau2_s), once per pooled draw and call, for every evaluation of the mixture CDF in k_loo_quantile
__global__ __launch_bounds__(256) void k_inv_sd(const double *tau2, int S, double *isd)
{
    const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (s < S) isd[s] = 1.0 / sqrt(tau2[s]);
}

// k_loo_moments: the moments of the LOO posterior predictive of row i, a mixture of N(eta_is, tau2_s) with the PSIS weights w_is = exp(LW_is):
//   mean_i = sum_s w eta,  sd_i = sqrt(sum_s w (tau2 + eta^2) - mean_i^2),  pit_i = sum_s w Phi((y_i - eta) / sqrt(tau2))  (Phi as in k_pred_pit)
// in one pass over (E, LW, tau2).  Layout of k_pred_pit: one workgroup of 256 threads per row, thread-strided partial sums, then a tree: bitwise
// independent of the grid and the block of rows.  A refused row (LW NaN) gets NaN.  No random numbers, no dynamic LDS, no scratch; bound by
// the exp and the erfc (some 10^2 f64 instructions per 16 bytes read), like k_pred_pit.  94 VGPRs, 6 KiB of LDS, no scratch.
__global__ __launch_bounds__(256) void k_loo_moments(const double *E, const double *LW, int nsamp, const double *y, const double *tau2, double *mean,
                                                     double *sd, double *pit)
{
    __shared__ double ra[256], rb[256], rc[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *e = E + (size_t)i * nsamp, *lw = LW + (size_t)i * nsamp;
    const double yi = y[i];
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int s = tid; s < nsamp; s += 256) {
        const double w = exp(lw[s]), eta = e[s], t = tau2[s];
        const double z = (yi - eta) / sqrt(t);
        a1 += w * eta;
        a2 += w * (t + eta * eta);
        a3 += w * (0.5 * erfc(-z / BNR_SQRT2));
    }
    ra[tid] = a1; rb[tid] = a2; rc[tid] = a3;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { ra[tid] += ra[tid + w]; rb[tid] += rb[tid + w]; rc[tid] += rc[tid + w]; } __syncthreads(); }
    if (tid == 0) {
        const double m = ra[0];
        mean[i] = m; sd[i] = sqrt(rb[0] - m * m); pit[i] = rc[0];
    }
}

// k_loo_quantile: the p-quantile of the mixture CDF F_i(t) = sum_s w_is Phi((t - eta_is) isd_s), Phi(z) = erfc(-z / sqrt 2) / 2, of row
// blockIdx.x; blockIdx.y = 0: p_lo -> lower, 1: p_hi -> upper (a NULL output: nothing to do).  Bisection from the bracket
// [min_s(eta_is - c sd_s), max_s(eta_is + c sd_s)], sd_s = sqrt(tau2_s), with the caller's c such that Phi(-c) < min(p_lo, 1 - p_hi) / 2, so that
// F(lower end) < p < F(upper end) whatever the weights; F(mid) < p moves the lower end, anything else the upper one; stops when the bracket is no
// wider than 2^-40 of the first one -- 40 halvings; BNR_LOOQ_MAX_IT caps the loop -- and returns the midpoint.  No sort, no random numbers.
// Every F is summed in k_loo_moments's order (thread-strided, then a tree) and broadcast from LDS, so the whole workgroup takes the same branch
// and the result is bitwise independent of the grid, the block of rows and the call.  A NaN F (a refused row) gives NaN.
// Per evaluation and draw one exp (the weight) and one erfc; the reciprocal of sd is staged by k_inv_sd, -1 / sqrt 2 is a constant factor.
// One workgroup per (row, bound): 2 x 40 evaluation passes per row over (E, LW), which stay in the L2 between passes.  90 VGPRs, 4 KiB of LDS,
// no scratch.
#define BNR_LOOQ_MAX_IT 64
__global__ __launch_bounds__(256) void k_loo_quantile(const double *E, const double *LW, int nsamp, const double *tau2, const double *isd, double c,
                                                      double p_lo, double p_hi, double *lower, double *upper)
{
    __shared__ double ra[256], rb[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double *out = blockIdx.y ? upper : lower;
    if (!out) return;
    const double p = blockIdx.y ? p_hi : p_lo;
    const double *e = E + (size_t)i * nsamp, *lw = LW + (size_t)i * nsamp;
    double mn = INFINITY, mx = -INFINITY;
    for (int s = tid; s < nsamp; s += 256) {
        const double eta = e[s], h = c * sqrt(tau2[s]);
        mn = fmin(mn, eta - h); mx = fmax(mx, eta + h);
    }
    ra[tid] = mn; rb[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { ra[tid] = fmin(ra[tid], ra[tid + w]); rb[tid] = fmax(rb[tid], rb[tid + w]); } __syncthreads(); }
    double lo = ra[0], hi = rb[0];
    __syncthreads();
    const double tol = (hi - lo) * 9.094947017729282e-13;             // 2^-40
    bool nan = false;
    for (int it = 0; it < BNR_LOOQ_MAX_IT && hi - lo > tol; ++it) {
        const double mid = 0.5 * (lo + hi);
        double acc = 0.0;
        for (int s = tid; s < nsamp; s += 256) {
            const double z = (mid - e[s]) * isd[s];
            acc += exp(lw[s]) * (0.5 * erfc(z * -0.70710678118654752440));
        }
        ra[tid] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w) ra[tid] += ra[tid + w]; __syncthreads(); }
        const double F = ra[0];
        __syncthreads();
        if (F != F) { nan = true; break; }
        if (F < p) lo = mid; else hi = mid;
    }
    if (tid == 0) out[i] = nan ? NAN : 0.5 * (lo + hi);
}

// ===================================================================================== k_rank / k_fold (ABI 12: rank-normalised diagnostics)
// k_rank: the average ranks of the draws of one staged column (see k_summary: column p of `buf`, leading dimension ld), their normal scores
// z = Phi^-1((r - 3/8) / (n + 1/4)) (bnr_ndtri), the two tail indicators, the median and a flag, one workgroup of 256 threads per column.
// The column holds nch windows of nsamp draws side by side; all = 0 ranks only the split-chain draws (rows [0, h) and [nsamp - h, nsamp) of
// every window, h = nsamp / 2: an odd window drops its middle row, as k_rhat_stats and k_acov do), all = 1 every draw.  n = nch x (nsamp or 2h).
//   1. keys: the order-preserving 64-bit image of every draw (bnr_key_of, -0 folded onto +0 so that the two tie) and its position in the
//      column (32 bits) go to keyA / idxA; the histograms of all eight 8-bit digits are counted in LDS on the way (integer LDS atomics: the
//      counts do not depend on their order).
//   2. LSD radix sort, 8 bits per pass, between the two (key, index) buffers in global memory; a pass whose digit is the same in every key
//      (the exponent bytes of most columns, seven of eight bytes of a 0/1 column) is skipped.  A pass walks the source in tiles of 256 in
//      order: a thread finds the lanes of its wave that hold its digit with eight ballots (its rank among them is a popcount), the waves'
//      counts meet in LDS (wcnt), and the digit's running base makes the destination: stable, no global atomics.
//   3. tie runs: one forward sweep over the sorted keys, a ballot per wave and a carry per tile, gives every position the start of its run
//      (sa) and every run start the end of its run (ea: written by the head of the next run); both live in the key buffer the sort left free.
//   4. results, scattered to the draws' own positions: rank = (start + end + 1) / 2 (1-based average of start + 1 .. end: an exact multiple
//      of 1/2), z, the indicators I(x <= x_(k05)) and I(x <= x_(k95)) as 0.0 / 1.0 (a comparison of keys), med = (x_(n/2) + x_(n/2+1)) / 2,
//      flag = 1 (a NaN) | 2 (an Inf) | 4 (all draws equal).  A column that holds a NaN gets NaN ranks and z.
// Ranks are a pure function of the data: equal keys end up in one run whatever order the sort left their indices in, so every output is bitwise
// independent of the grid, the block of columns and the call.  Every index stays below n <= ld: nothing is written outside the column's slices.
// 128 VGPRs, 14.1 KiB of LDS, no scratch.
// Phases 1 and 2 are shared with k_hdi (behind k_fold): IDX = true, the draw's position travels with its key (k_rank); false, keys only -- 8 + 8
// bytes per draw and pass instead of 12 + 12, and the index buffers are never touched (k_hdi).  The LDS arrays are the caller's.
template <bool IDX>
__device__ __forceinline__ void bnr_sort_build_keys(const double *x, int n, int nsamp, int per, int hh, int gap, unsigned long long *src, unsigned int *si,
                                                    unsigned int (&hist)[8][256], int (&s_skip)[8], int &s_flag)
{
    const int tid = threadIdx.x;
    int myflag = 0;
    for (int t = tid; t < n; t += 256) {
        const int c = t / per, u = t - c * per;
        const unsigned int pos = (unsigned int)(c * nsamp + (u < hh ? u : u + gap));
        double v = x[pos];
        if (v != v) myflag |= 1;
        else if (fabs(v) == INFINITY) myflag |= 2;
        if (v == 0.0) v = 0.0;                                 // -0 ties with +0
        const unsigned long long key = bnr_key_of(v);
        src[t] = key;
        if constexpr (IDX) si[t] = pos;
#pragma unroll
        for (int b = 0; b < 8; ++b) atomicAdd(&hist[b][(unsigned int)(key >> (8 * b)) & 255u], 1u);
    }
    if (myflag) atomicOr(&s_flag, myflag);
    __syncthreads();
    for (int b = 0; b < 8; ++b) if (hist[b][tid] == (unsigned int)n) s_skip[b] = 1;
    __syncthreads();
}
// (on return src holds the sorted keys -- and si their positions -- and dst / di are free)
template <bool IDX>
__device__ __forceinline__ void bnr_sort_passes(int n, unsigned long long *&src, unsigned long long *&dst, unsigned int *&si, unsigned int *&di,
                                                unsigned int (&hist)[8][256], unsigned int (&base)[256], unsigned int (&tmp)[256],
                                                unsigned int (&wcnt)[4][256], int (&s_skip)[8])
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int pass = 0; pass < 8; ++pass) {
        if (s_skip[pass]) continue;                            // (uniform: read behind the barrier above, never written again)
        const int shift = 8 * pass;
        const unsigned int mine = hist[pass][tid];
        tmp[tid] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned int a = tid >= off ? tmp[tid - off] : 0u;
            __syncthreads();
            tmp[tid] += a;
            __syncthreads();
        }
        base[tid] = tmp[tid] - mine;
        __syncthreads();
        for (int t0 = 0; t0 < n; t0 += 256) {
            const int t = t0 + tid;
            const bool valid = t < n;
            const unsigned long long key = valid ? src[t] : 0ull;
            unsigned int id = 0u;
            if constexpr (IDX) id = valid ? si[t] : 0u;
            const unsigned int d = (unsigned int)(key >> shift) & 255u;
            unsigned long long mask = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const unsigned long long m = __ballot((d >> b) & 1u);
                mask &= ((d >> b) & 1u) ? m : ~m;
            }
            const unsigned int lrank = (unsigned int)__popcll(mask & below), cnt = (unsigned int)__popcll(mask);
            if (valid && lrank == 0u) wcnt[w][d] = cnt;
            __syncthreads();
            unsigned int pos = 0u;
            if (valid) {
                pos = base[d] + lrank;
                for (int ww = 0; ww < w; ++ww) pos += wcnt[ww][d];
            }
            __syncthreads();
            if (valid && lrank == 0u) { atomicAdd(&base[d], cnt); wcnt[w][d] = 0u; }
            if (valid && pos < (unsigned int)n) {
                dst[pos] = key;
                if constexpr (IDX) di[pos] = id;
            }
        }
        __syncthreads();
        unsigned long long *tk = src; src = dst; dst = tk;
        if constexpr (IDX) { unsigned int *ti = si; si = di; di = ti; }
    }
}
__global__ __launch_bounds__(256) void k_rank(const double *buf, long long ld, int nsamp, int nch, int all, unsigned long long *keyA,
                                              unsigned long long *keyB, unsigned int *idxA, unsigned int *idxB, int k05, int k95, double *ranks,
                                              double *z, double *ind05, double *ind95, double *med, int *flag)
{
    __shared__ unsigned int hist[8][256];
    __shared__ unsigned int base[256], tmp[256];
    __shared__ unsigned int wcnt[4][256];
    __shared__ int s_skip[8], wlast[2][4], carry[2], s_flag;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t c0 = (size_t)blockIdx.x * (size_t)ld;
    const double *x = buf + c0;
    const int hh = nsamp / 2, per = all ? nsamp : 2 * hh, gap = nsamp - per;
    const int n = nch * per;
    unsigned long long *src = keyA + c0, *dst = keyB + c0;
    unsigned int *si = idxA + c0, *di = idxB + c0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int b = 0; b < 8; ++b) hist[b][tid] = 0u;
    for (int b = 0; b < 4; ++b) wcnt[b][tid] = 0u;
    if (tid < 8) s_skip[tid] = 0;
    if (tid == 0) { s_flag = 0; carry[0] = 0; carry[1] = 0; }
    __syncthreads();
    // 1. keys and digit histograms
    bnr_sort_build_keys<true>(x, n, nsamp, per, hh, gap, src, si, hist, s_skip, s_flag);
    // 2. the passes
    bnr_sort_passes<true>(n, src, dst, si, di, hist, base, tmp, wcnt, s_skip);
    // 3. tie runs
    unsigned int *sa = (unsigned int *)dst, *ea = sa + ld;
    for (int t0 = 0, it = 0; t0 < n; t0 += 256, ++it) {
        const int par = it & 1, t = t0 + tid;
        const bool valid = t < n;
        const bool head = valid && (t == 0 || src[t] != src[t - 1]);
        const unsigned long long hm = __ballot(head);
        if (lane == 0) wlast[par][w] = hm ? t0 + w * 64 + (63 - __clzll((long long)hm)) : -1;
        __syncthreads();
        int c = carry[par];
        for (int ww = 0; ww < w; ++ww) if (wlast[par][ww] >= 0) c = wlast[par][ww];
        const unsigned long long lo = hm & below, in = hm & (below | (1ull << lane));
        const int sx = lo ? t0 + w * 64 + (63 - __clzll((long long)lo)) : c;        // the start of the run of position t - 1
        const int s_in = in ? t0 + w * 64 + (63 - __clzll((long long)in)) : c;      // the start of the run of position t
        if (valid) {
            sa[t] = (unsigned int)s_in;
            if (head && t > 0) ea[sx] = (unsigned int)t;
            if (t == n - 1) ea[s_in] = (unsigned int)n;
        }
        if (tid == 255) carry[par ^ 1] = s_in;
    }
    __syncthreads();
    // 4. results
    const int fl = s_flag | (ea[0] == (unsigned int)n ? 4 : 0);
    const bool nan = (fl & 1) != 0;
    if (tid == 0) {
        flag[blockIdx.x] = fl;
        if (med) med[blockIdx.x] = n >= 2 ? (bnr_double_of(src[n / 2 - 1]) + bnr_double_of(src[n / 2])) / 2.0 : bnr_double_of(src[0]);
    }
    const unsigned long long q05 = ind05 ? src[k05 - 1] : 0ull, q95 = ind95 ? src[k95 - 1] : 0ull;
    const double den = (double)n + 0.25;
    for (int t = tid; t < n; t += 256) {
        const unsigned int s = sa[t], e = ea[s];
        const double r = (double)((unsigned long long)s + e + 1ull) * 0.5;
        const size_t i = c0 + si[t];
        if (ranks) ranks[i] = nan ? NAN : r;
        if (z) z[i] = nan ? NAN : bnr_ndtri((r - 0.375) / den);
        if (ind05) ind05[i] = src[t] <= q05 ? 1.0 : 0.0;
        if (ind95) ind95[i] = src[t] <= q95 ? 1.0 : 0.0;
    }
}

// k_fold: the draws of every staged column about the column's median, for k_rank's second run and for the moments of x; `chunks` workgroups
// of 256 draws per column.  absolute = 1: the folded draws |x - med| of the tail R-hat; 0: x - med, on which ess_mean and mcse_mean are
// computed -- both are invariant under the shift, and a column like 1e8 + N(0, 1) would otherwise lose eight digits of its split-chain means
// (the between-chain variance B) to the rounding of k_acov's sums.
__global__ __launch_bounds__(256) void k_fold(const double *buf, long long ld, int chunks, const double *med, int absolute, double *out)
{
    const int col = (int)(blockIdx.x / (unsigned)chunks);
    const long long i = (long long)(blockIdx.x % (unsigned)chunks) * 256 + threadIdx.x;
    if (i >= ld) return;
    const size_t o = (size_t)col * (size_t)ld + (size_t)i;
    const double v = buf[o] - med[col];
    out[o] = absolute ? fabs(v) : v;
}

// ===================================================================================== k_hdi (ABI 13: highest-density intervals, sign probabilities)
// k_hdi: of one staged column of n draws (column blockIdx.x of `buf`, leading dimension ld >= n; every draw takes part), one workgroup of 256
// threads per column: the shortest interval that holds w_k + 1 consecutive order statistics for each of nprob <= 8 window lengths w_k (the
// highest-density interval of a sample: ArviZ's _hdi, R's HDInterval::hdi), the median as k_rank takes it, and the shares of draws above and
// below zero.
//   1., 2. k_rank's key image and sort, keys only (bnr_sort_build_keys<false>, bnr_sort_passes<false>).
//   3. sign counts: two binary searches over the sorted keys for the key of +0.0 (-0 was folded onto it) give the number of keys below it and
//      the number not above it: p_neg = below / n, p_pos = (n - not above) / n, integers over n.
//   4. per level, over j = 0 .. n - w - 1 the width d_j = x_(j+w) - x_(j), one f64 subtraction of the decoded keys; every thread walks
//      j = tid, tid + 256, ... and keeps the smallest (d_j, j) in lexicographic order, a fixed tree over the 256 threads merges them: the first
//      minimum, whatever the grid or the order of arrival.  lower = x_(j*), upper = x_(j* + w), level k at offset k lstride of both.
// A column that holds a NaN is NaN in every output and is not sorted; one that holds an Inf (and no NaN) is NaN in lower, upper and med, its
// shares are counted.  A constant column skips every pass and gets lower = upper = the constant.  Every index stays below n <= ld: nothing is
// written outside the column's slices of keyA / keyB, and every output is a pure function of the column's draws.  lower / upper NULL (both):
// phase 4 is not run.
struct bnr_hdi_levels { int w[8]; };
__global__ __launch_bounds__(256) void k_hdi(const double *buf, long long ld, int n, unsigned long long *keyA, unsigned long long *keyB, int nprob,
                                             bnr_hdi_levels lv, double *lower, double *upper, long long lstride, double *med, double *p_pos, double *p_neg)
{
    __shared__ unsigned int hist[8][256];
    __shared__ unsigned int base[256], tmp[256];
    __shared__ unsigned int wcnt[4][256];
    __shared__ double rd[256];
    __shared__ int rj[256];
    __shared__ int s_skip[8], s_flag;
    const int tid = threadIdx.x;
    const size_t c0 = (size_t)blockIdx.x * (size_t)ld;
    unsigned long long *src = keyA + c0, *dst = keyB + c0;
    unsigned int *si = nullptr, *di = nullptr;
    for (int b = 0; b < 8; ++b) hist[b][tid] = 0u;
    for (int b = 0; b < 4; ++b) wcnt[b][tid] = 0u;
    if (tid < 8) s_skip[tid] = 0;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    bnr_sort_build_keys<false>(buf + c0, n, n, n, n / 2, 0, src, si, hist, s_skip, s_flag);
    const int fl = s_flag;                                     // (uniform: behind the function's barriers)
    if (fl & 1) {
        if (tid == 0) { med[blockIdx.x] = NAN; p_pos[blockIdx.x] = NAN; p_neg[blockIdx.x] = NAN; }
        if (lower && tid < nprob) { lower[(size_t)tid * lstride + blockIdx.x] = NAN; upper[(size_t)tid * lstride + blockIdx.x] = NAN; }
        return;
    }
    bnr_sort_passes<false>(n, src, dst, si, di, hist, base, tmp, wcnt, s_skip);
    // 3. sign counts and the median
    if (tid == 0 || tid == 64) {
        const unsigned long long zero = 0x8000000000000000ull;
        int lo = 0, hi = n;                                    // tid 0: the first key >= zero; tid 64: the first key > zero
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const unsigned long long k = src[mid];
            if (tid == 0 ? k < zero : k <= zero) lo = mid + 1; else hi = mid;
        }
        if (tid == 0) p_neg[blockIdx.x] = (double)lo / (double)n;
        else p_pos[blockIdx.x] = (double)(n - lo) / (double)n;
    }
    if (tid == 128)
        med[blockIdx.x] = (fl & 2) ? NAN : n >= 2 ? (bnr_double_of(src[n / 2 - 1]) + bnr_double_of(src[n / 2])) / 2.0 : bnr_double_of(src[0]);
    if (!lower) return;
    if (fl & 2) {
        if (tid < nprob) { lower[(size_t)tid * lstride + blockIdx.x] = NAN; upper[(size_t)tid * lstride + blockIdx.x] = NAN; }
        return;
    }
    // 4. the shortest window of every level
    for (int k = 0; k < nprob; ++k) {
        const int w = lv.w[k], m = n - w;
        double bd = INFINITY;
        int bj = 0x7FFFFFFF;
        for (int j = tid; j < m; j += 256) {
            const double d = bnr_double_of(src[j + w]) - bnr_double_of(src[j]);
            if (d < bd || bj == 0x7FFFFFFF) { bd = d; bj = j; }
        }
        rd[tid] = bd; rj[tid] = bj;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const double od = rd[tid + s];
                const int oj = rj[tid + s];
                if (od < rd[tid] || (od == rd[tid] && oj < rj[tid])) { rd[tid] = od; rj[tid] = oj; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int j = rj[0];
            lower[(size_t)k * lstride + blockIdx.x] = bnr_double_of(src[j]);
            upper[(size_t)k * lstride + blockIdx.x] = bnr_double_of(src[j + w]);
        }
        __syncthreads();
    }
}

// ===================================================================================== k_incl_* (ABI 15: the joint posterior of the indicators)
// Of an S x B matrix of 0/1 indicators z (B = V: xi_v != 0; B = R: lambda_r != 0; or a caller's bytes): the marginal and pairwise inclusion
// counts, the histogram of the number of included indicators, and the distinct rows ("patterns") with their counts.  Every result is an
// integer count; the integer atomics that collect them commute, so every output is bitwise independent of the grid and the call.  The
// indicator is the IEEE comparison x != 0: -0 is zero, a NaN counts as included.
//
// k_incl_pack: the bit images of z.  A wave owns 64 draws (draw tile dt) and walks the W = ceil(B / 64) words of their patterns: for each of
// the 64 draws one coalesced read of 64 indicators (lane = indicator; 512 bytes of a trace row read in place, or 64 bytes of the caller's
// matrix; eight rows in flight), whose ballot is the draw's pattern word -- kept by lane i for draw i and stored to pat[S][W] --, while every lane ORs its own bit
// into the bit-column word of its indicator over these 64 draws, stored to col[B][CW], CW = ceil(S / 64).  Rows past S and indicators past B
// are 0 bits.  The popcounts of the column words are the marginal counts, the popcount of a draw's W words its size: both meet in LDS
// (2 B + 1 counters, dynamic) and leave the workgroup as one global atomic per non-zero counter.  The grid strides over the draw tiles.
// A chain's window: base = the first row's first indicator, stride = doubles between rows; pooled draw s lies in src[s / nsamp].
// 32 VGPRs, 4 (2 B + 1) bytes of LDS, no scratch.
struct bnr_incl_src { const double *base; long long stride; };
__global__ __launch_bounds__(256) void k_incl_pack(const bnr_incl_src *src, int nsamp, const unsigned char *zb, int S, int B, int W, int CW,
                                                   unsigned long long *pat, unsigned long long *col, unsigned int *marg, unsigned int *size)
{
    extern __shared__ unsigned int incl_cnt[];                 // [0, B]: the sizes; [B + 1, 2 B]: the marginal counts
    unsigned int *lsize = incl_cnt, *lmarg = incl_cnt + B + 1;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int t = tid; t < 2 * B + 1; t += 256) incl_cnt[t] = 0u;
    __syncthreads();
    for (int dt = blockIdx.x * 4 + w; dt < CW; dt += gridDim.x * 4) {
        const int s0 = dt * 64, ns = min(64, S - s0);
        const int c0 = zb ? 0 : s0 / nsamp, r0 = zb ? 0 : s0 - c0 * nsamp;
        int npop = 0;
        for (int wj = 0; wj < W; ++wj) {
            const int k = wj * 64 + lane;
            const bool in = k < B;
            unsigned long long mine = 0ull, cw = 0ull;
            for (int i0 = 0; i0 < ns; i0 += 8) {               // eight rows in flight, then their ballots
                bool bit[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = i0 + j;
                    bit[j] = false;
                    if (in && i < ns) {
                        if (zb) bit[j] = zb[(size_t)(s0 + i) * (size_t)B + k] != 0;
                        else {
                            int c = c0, r = r0 + i;
                            while (r >= nsamp) { r -= nsamp; ++c; }            // (the next chain's window)
                            bit[j] = src[c].base[(long long)r * src[c].stride + k] != 0.0;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long m = __ballot(bit[j]);
                    if (lane == i0 + j) mine = m;
                    cw |= (unsigned long long)bit[j] << (i0 + j);
                }
            }
            if (pat && lane < ns) pat[(size_t)(s0 + lane) * W + wj] = mine;
            if (in) {
                if (col) col[(size_t)k * CW + dt] = cw;
                if (cw) atomicAdd(&lmarg[k], (unsigned int)__popcll(cw));
            }
            npop += __popcll(mine);
        }
        if (lane < ns) atomicAdd(&lsize[npop], 1u);
    }
    __syncthreads();
    for (int t = tid; t < 2 * B + 1; t += 256) {
        const unsigned int v = incl_cnt[t];
        if (v) atomicAdd(t <= B ? &size[t] : &marg[t - B - 1], v);
    }
}

// k_incl_joint: count[k][l] = sum over w of popcount(col_k[w] & col_l[w]), one 64-bit AND + popcount for 64 draws.  A workgroup takes a pair
// (I, J <= I) of panels of 32 columns (blockIdx.x) and strides over chunks of 64 column words (blockIdx.y): both panels of a chunk go to LDS,
// word-major and padded, so every col word is read from memory ceil(B / 32) + 1 times; a thread holds column kk = tid % 32 of panel I against
// four columns of panel J in registers over all its chunks and adds them to the full symmetric matrix at the end, with integer atomics: the
// pair (k, l) and, for I != J, its mirror (l, k); a diagonal pair of panels computes both halves itself.  Far below the cost of k_incl_pack
// (V = 300, S = 400 000: 2.8e8 word operations), hence no MFMA path.  58 VGPRs, 33 KiB of LDS, no scratch.
__global__ __launch_bounds__(256) void k_incl_joint(const unsigned long long *col, int B, int CW, unsigned int *count)
{
    __shared__ unsigned long long pa[64][33], pb[64][33];
    const int tid = threadIdx.x, kk = tid & 31, l0 = (tid >> 5) * 4;
    int I = 0, rest = blockIdx.x;
    while (rest > I) { rest -= I + 1; ++I; }                   // blockIdx.x = I (I + 1) / 2 + J
    const int J = rest, nchunks = (CW + 63) / 64;
    unsigned int acc[4] = {0u, 0u, 0u, 0u};
    for (int ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
        const int w0 = ch * 64;
        for (int e = tid; e < 32 * 64; e += 256) {
            const int cidx = e >> 6, x = e & 63, ka = I * 32 + cidx, kb = J * 32 + cidx;
            const bool wi = w0 + x < CW;
            pa[x][cidx] = wi && ka < B ? col[(size_t)ka * CW + w0 + x] : 0ull;
            pb[x][cidx] = wi && kb < B ? col[(size_t)kb * CW + w0 + x] : 0ull;
        }
        __syncthreads();
        for (int x = 0; x < 64; ++x) {
            const unsigned long long a = pa[x][kk];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (unsigned int)__popcll(a & pb[x][l0 + j]);
        }
        __syncthreads();
    }
    const int k = I * 32 + kk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = J * 32 + l0 + j;
        if (k < B && l < B && acc[j]) {
            atomicAdd(&count[(size_t)k * B + l], acc[j]);
            if (I != J) atomicAdd(&count[(size_t)l * B + k], acc[j]);
        }
    }
}

// k_incl_group: the distinct patterns among the S draws and their counts, exactly (no hashing), in one workgroup of 256 threads with k_rank's
// sort (bnr_sort_passes and its LDS arrays, unchanged).
//   1. LSD radix sort of the draw indices over the W pattern words, word 0 (the least significant) first: per word the keys pat[si[t]][w] are
//      gathered in the current order with their eight digit histograms (a word that is the same in every draw skips all its passes), then
//      bnr_sort_passes<true>.  Stable, so the draws end up ascending in the pattern as an integer.
//   2. run heads: position t starts a run where any of the W words differs from position t - 1; the heads are compacted in order (a ballot per
//      wave, a carry per tile of 256) into the free index buffer.  n_distinct = the number of heads, a run's length = the next head - its own.
//   3. the ntop most frequent (ntop > 0): a keys-only sort (bnr_sort_passes<false>) of ((2^32 - 1 - count) << 32) | head position: count
//      descending, ties by position, i.e. by pattern ascending.  The first min(ntop, n_distinct) give top_count and -- through si -- the W
//      words of top_sets; the entries behind them stay the zeros they were allocated as.
// Every index stays below S: si is a permutation of 0 .. S - 1 and head positions are positions of it.  keyA / keyB / idxA / idxB hold S
// entries each.  37 VGPRs, 14.1 KiB of LDS, no scratch.
__global__ __launch_bounds__(256) void k_incl_group(const unsigned long long *pat, int S, int W, unsigned long long *keyA, unsigned long long *keyB,
                                                    unsigned int *idxA, unsigned int *idxB, int ntop, long long *n_distinct,
                                                    unsigned long long *top_sets, long long *top_count)
{
    __shared__ unsigned int hist[8][256];
    __shared__ unsigned int base[256], tmp[256];
    __shared__ unsigned int wcnt[4][256];
    __shared__ int s_skip[8], wheads[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long *src = keyA, *dst = keyB;
    unsigned int *si = idxA, *di = idxB;
    for (int b = 0; b < 4; ++b) wcnt[b][tid] = 0u;
    for (int t = tid; t < S; t += 256) si[t] = (unsigned int)t;
    // 1. the draws in the order of their patterns
    for (int wd = 0; wd < W; ++wd) {
        for (int b = 0; b < 8; ++b) hist[b][tid] = 0u;
        if (tid < 8) s_skip[tid] = 0;
        __syncthreads();
        for (int t = tid; t < S; t += 256) {
            const unsigned long long key = pat[(size_t)si[t] * W + wd];
            src[t] = key;
#pragma unroll
            for (int b = 0; b < 8; ++b) atomicAdd(&hist[b][(unsigned int)(key >> (8 * b)) & 255u], 1u);
        }
        __syncthreads();
        for (int b = 0; b < 8; ++b) if (hist[b][tid] == (unsigned int)S) s_skip[b] = 1;
        __syncthreads();
        bnr_sort_passes<true>(S, src, dst, si, di, hist, base, tmp, wcnt, s_skip);
        __syncthreads();
    }
    // 2. run heads, compacted into di
    int nd = 0;                                                // (the heads so far: the same in every thread)
    for (int t0 = 0; t0 < S; t0 += 256) {
        const int t = t0 + tid;
        bool head = false;
        if (t < S) {
            head = t == 0;
            if (t > 0) {
                const unsigned long long *a = pat + (size_t)si[t] * W, *b = pat + (size_t)si[t - 1] * W;
                for (int wd = 0; wd < W; ++wd) head = head || a[wd] != b[wd];
            }
        }
        const unsigned long long hm = __ballot(head);
        if (lane == 0) wheads[w] = __popcll(hm);
        __syncthreads();
        int at = nd;
        for (int ww = 0; ww < w; ++ww) at += wheads[ww];
        if (head) di[at + __popcll(hm & below)] = (unsigned int)t;
        nd += wheads[0] + wheads[1] + wheads[2] + wheads[3];
        __syncthreads();
    }
    if (tid == 0) *n_distinct = nd;
    if (ntop < 1) return;
    // 3. the most frequent patterns
    for (int b = 0; b < 8; ++b) hist[b][tid] = 0u;
    if (tid < 8) s_skip[tid] = 0;
    __syncthreads();
    for (int j = tid; j < nd; j += 256) {
        const unsigned int at = di[j], cnt = (j + 1 < nd ? di[j + 1] : (unsigned int)S) - at;
        const unsigned long long key = ((unsigned long long)(0xFFFFFFFFu - cnt) << 32) | at;
        src[j] = key;
#pragma unroll
        for (int b = 0; b < 8; ++b) atomicAdd(&hist[b][(unsigned int)(key >> (8 * b)) & 255u], 1u);
    }
    __syncthreads();
    for (int b = 0; b < 8; ++b) if (hist[b][tid] == (unsigned int)nd) s_skip[b] = 1;
    __syncthreads();
    unsigned int *none_a = nullptr, *none_b = nullptr;
    bnr_sort_passes<false>(nd, src, dst, none_a, none_b, hist, base, tmp, wcnt, s_skip);
    __syncthreads();
    for (int j = tid; j < min(ntop, nd); j += 256) {
        const unsigned long long key = src[j];
        top_count[j] = (long long)(0xFFFFFFFFu - (unsigned int)(key >> 32));
        const unsigned long long *a = pat + (size_t)si[(unsigned int)key] * W;
        for (int wd = 0; wd < W; ++wd) top_sets[(size_t)j * W + wd] = a[wd];
    }
}

// ===================================================================================== k_cov (ABI 17: the posterior covariance of the edge coefficients)
// The centred Gram of `ncols` chosen gamma columns over every chain's window, chain blockIdx.z on its own: for the positions pa in [a0, a0 + na)
// and pb in [b0, b0 + nb) of the caller's column list (a pair of column blocks, I <= J), with x = rowsv[blockIdx.z] and G the chain's slice
// G + blockIdx.z gstride,
//   G[(pa - a0) ldg + (pb - b0)] = sum_s (x[s][cols[pa]] - centre[pa]) (x[s][cols[pb]] - centre[pb]),  s = 0 .. nsamp - 1,
// by v_mfma_f64_16x16x4_f64 with the K dimension running over the draws: A[i][k] = the centred draw s0 + k of column pa0 + i, B[k][j] = that of
// column pb0 + j.  x[s] = rows + s rowlen is read in place (a trace row at o_gamma, or a row of a caller's matrix): the 16 lanes of a lane group
// read 16 columns of one draw, 128 contiguous bytes where the columns are consecutive.  The centre (the mean the Summary calls report, computed
// before this kernel) is subtracted in registers BEFORE the product -- never an uncentred Gram corrected by S c c^T, which loses every digit of a
// column like 1e8 + N(0, 1) (see k_fold).  Padding -- the draws past nsamp of the last K step, the columns past the block's end -- is the
// constant 0.0 chosen by a select behind the subtraction, and its loads are clamped to a draw and a column that exist: padding never meets
// garbage, and a NaN lives only in the rows and columns of G that belong to its column.
// K order: one accumulator per entry, k0 = 0, 16, ... < nsamp; inside a step MFMA t (0..3) takes the draws k0 + 4 t + g from lane group
// g = lane >> 4.  So the order of an entry's sum is fixed by nsamp alone: not by the grid, the tile shape TW, the column block or the other
// columns of the call; (pa, pb) and (pb, pa) are the same products in the same order.  D layout: lane l, reg r = row (l >> 4) + 4 r, column l & 15.
// grid = (ceil(nb / (32 TW)), ceil(na / (32 TW)), chains), 256 threads: wave w owns the TW x TW tiles of 16 x 16 at rows (2 blockIdx.y + (w >> 1)) 16 TW,
// columns (2 blockIdx.x + (w & 1)) 16 TW of the block pair; a wave whose entries all lie below the diagonal (pa > pb) or outside the pair
// returns at once (no barrier in the kernel), entries below the diagonal inside a computed tile are written and never read.  The loads of
// K step k0 + 16 are issued in front of the MFMAs of step k0.  No LDS, no scratch; 64-bit addressing.
template <int TW>
__global__ __launch_bounds__(256) void k_cov(const double *const *rowsv, long long rowlen, int nsamp, const int *cols, const double *centre, int a0,
                                             int na, int b0, int nb, double *G, long long gstride, int ldg)
{
    const double *rows = rowsv[blockIdx.z];
    G += (size_t)blockIdx.z * (size_t)gstride;
    constexpr int WT = 16 * TW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int pa0 = a0 + ((int)blockIdx.y * 2 + (w >> 1)) * WT, pb0 = b0 + ((int)blockIdx.x * 2 + (w & 1)) * WT;
    const int aend = a0 + na, bend = b0 + nb;
    if (pa0 >= aend || pb0 >= bend || pa0 > pb0 + WT - 1) return;
    int ca[TW], cb[TW];
    double ma[TW], mb[TW];
    bool va[TW], vb[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i) {
        const int pa = pa0 + 16 * i + c, pb = pb0 + 16 * i + c;
        va[i] = pa < aend; vb[i] = pb < bend;
        ca[i] = cols[va[i] ? pa : a0]; cb[i] = cols[vb[i] ? pb : b0];
        ma[i] = va[i] ? centre[pa] : 0.0; mb[i] = vb[i] ? centre[pb] : 0.0;
    }
    bnr_d4 acc[TW][TW];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[i][j] = bnr_d4{0.0, 0.0, 0.0, 0.0};
    double ra[4][TW], rb[4][TW];                       // the raw draws of the next K step
    auto fetch = [&](int k0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double *row = rows + (size_t)min(k0 + 4 * t + g, nsamp - 1) * (size_t)rowlen;
#pragma unroll
            for (int i = 0; i < TW; ++i) { ra[t][i] = row[ca[i]]; rb[t][i] = row[cb[i]]; }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < nsamp; k0 += 16) {
        double av[4][TW], bv[4][TW];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool ok = k0 + 4 * t + g < nsamp;
#pragma unroll
            for (int i = 0; i < TW; ++i) {
                const double da = ra[t][i] - ma[i], db = rb[t][i] - mb[i];
                av[t][i] = ok && va[i] ? da : 0.0;
                bv[t][i] = ok && vb[i] ? db : 0.0;
            }
        }
        fetch(k0 + 16);                                // (clamped to the last draw behind the window's end)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int j = 0; j < TW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][i], bv[t][j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            const int pb = pb0 + 16 * j + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pa = pa0 + 16 * i + g + 4 * r;
                if (pa < aend && pb < bend) G[(size_t)(pa - a0) * (size_t)ldg + (size_t)(pb - b0)] = acc[i][j][r];
            }
        }
}

// k_cov_finish: the entries pa <= pb of a block pair from the chains' Grams (chain k's at G + k gstride), mirrored into both triangles of the
// ncols x ncols matrix cov:  sum_k G_k / denom (wt NULL: denom = S - 1) or sum_k wt[k] G_k / denom (denom = nsamp), k ascending from 0.0,
// every product and addition rounded on its own.  A column whose centre is not finite (it holds a NaN or an Inf draw) is NaN in its whole row
// and column.  One thread per entry of the pair.
__global__ __launch_bounds__(256) void k_cov_finish(const double *G, long long gstride, int ldg, int nc, const double *wt, double denom,
                                                    const double *centre, int a0, int na, int b0, int nb, double *cov, int ncols)
{
    const int ib = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), ia = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (ia >= na || ib >= nb) return;
    const int pa = a0 + ia, pb = b0 + ib;
    if (pa > pb) return;
    const double *e = G + (size_t)ia * (size_t)ldg + (size_t)ib;
    double tot = 0.0;
    for (int k = 0; k < nc; ++k) {
        const double gk = e[(size_t)k * (size_t)gstride];
        tot = tot + (wt ? wt[k] * gk : gk);
    }
    double v = tot / denom;
    if (!isfinite(centre[pa]) || !isfinite(centre[pb])) v = NAN;
    cov[(size_t)pa * (size_t)ncols + (size_t)pb] = v;
    cov[(size_t)pb * (size_t)ncols + (size_t)pa] = v;
}
