// bnr_kernels.h -- CDNA4 (gfx950) kernels of the Gibbs sweep (reference: src/gibbs.jl:267-677).
//
// Data layout in HBM (one chain):
//   X      n_pad x q_pad doubles, column-major, zero padded (n_pad % 64 == 0): the reference's n x q model matrix
//   trace  tot x rowlen doubles, ROW-major: row = one Gibbs state
//          [tau2, theta, Delta, mu | xi(V) | lam(R) | pi(R x 3) | M(R x R) | u(R x V) | gamma(q) | S(q)]  (col-major pieces)
//          -> every kernel writes its part of the new state straight into the trace row (coalesced); the
//          reference's iteration-fastest Table layout is produced by a transpose on fetch.
//   plan   one entry per iteration of a run call: {rng iteration id, row to write, row to read, ring wrap flag}
//
// Sweep order and what each kernel covers (gibbs.jl:663-677):
//   k_node      update_tau2! (scalar draw from carried sums) + update_u_xi! (one wave per node, log-space weights)
//   k_xpass     W = lowtri(u' L u), sz = sqrt(S) z1, partial GEMVs X W and X sz          (reads X once)
//   k_gram / k_gram8   X diag(S) X' by v_mfma_f64_16x16x4_f64, split-K partial tiles; lower triangle only, and of a diagonal tile only
//               what lies on or below the diagonal at block / MFMA-tile granularity    (reads X once)
//   k_chol_step x n_pad/32   E = [G + I ; I] -> [L ; L^-T]  (right-looking blocked Cholesky, one launch per panel; launch 0 also sums the
//               split-K partials; k_gram_reduce / k_chol_step2 for the two-panel variant of large n)
//   k_rhs, k_solve_w, k_solve_a4   a4 = (G+I)^-1 (a1 - a3) = Y (Y' b); X gamma_new from n-vectors (no third pass over X)
//   k_backproj  gamma (back-projection X' a4), update_D! (GIG draws), partial sums for theta and Lambda (reads X once)
//   k_tail      update_theta!, update_Delta!, update_M!, update_mu!, update_Lambda!, update_pi!, carried sums
// Every sweep kernel exists for ONE chain (descriptor by value: bnr_one) and for a lockstep group of chains (device array
// of descriptors indexed by the grid's chain coordinate: bnr_many); the arithmetic of a chain is the same in both.
// Outside the sweep: k_init_prior (initialize_variables!), k_fetch_cols / k_load_cols (Table layout), k_rhat_stats
// (split-Rhat message), k_summary (Summary statistics), k_acov (ESS message), k_wsummary (k_summary under chain weights, ABI 16; last in this file).  The kernels of the posterior analysis (prediction, PSIS-LOO,
// rank-normalised diagnostics, HDI) are a code object of their own: bnr_analysis_kernels.h.
//   k_x_mask, k_sdigits, k_gram_i8   the Gram of a binary (0/1) model matrix on the i8 matrix pipe (round 5)
// The measured experiments of rounds 3-4 (persistent / resident Gram kernels, left-looking and data-flow factorizations, gates, ...) are not
// part of this tree any more: tools/experiments/ keeps their kernels and drivers for the record (they built against the round-4 tree).
#pragma once
#include "bnr_device.h"

#define BNR_RMAX 32          // latent dimension limit of the small-matrix routines
#define BNR_NB 32            // Cholesky block size
#define BNR_GT 64            // Gram workgroup tile

// What a kernel of the sweep hands to a LATER launch can go to memory through the L2 (write-through) instead of staying dirty in the XCD's write-back L2 until
// the flush at the kernel boundary: same values, same addresses, only the moment the bytes leave the L2 moves.  BNR_STORE_THROUGH: one bit per site; a set bit
// compiles the through form, a cleared one the plain store.  What the same launch reads back (progress, stamp and counter words) is never stored this way.
// The default holds the sites that paid at the headline shape (profiles/store_through.txt): the update roles (8 chains: 2.3 -> 1.75 us between two panel steps for
// 0.1-0.3 us more in the step), the Gram's tiles and launch 0's E and Y (0.8 and 0.9 us off the gap behind them).  The swept block of a panel workgroup stays plain: that
// workgroup ends its launch, and waiting for its own write-through costs the step more than the flush; the small vectors and the scalar queue's PW / PA move nothing.
enum { BNR_ST_GRAM = 1,       // partial tiles of k_gram / k_gram8 / k_gram_i8
       BNR_ST_LAUNCH0 = 2,    // E and Y = I from the reduction (launch 0 of the factorization, k_gram_reduce)
       BNR_ST_UPDATE = 4,     // both update roles of k_chol_step
       BNR_ST_PANEL = 8,      // the swept own block of a panel workgroup
       BNR_ST_RHS = 16,       // xw, a3, b of k_rhs, w of k_solve_w, a4 and xg of k_solve_a4
       BNR_ST_XPASS = 32,     // PW / PA of k_xpass and k_xpass_group
       BNR_ST_BACKPROJ = 64 };  // gamma, S and Psum of k_backproj / k_backproj64
#ifndef BNR_STORE_THROUGH
#define BNR_STORE_THROUGH (BNR_ST_GRAM | BNR_ST_LAUNCH0 | BNR_ST_UPDATE)
#endif
// 8 bytes: a relaxed agent-scope atomic store is a global_store_dwordx2 with sc1
template <int SITE>
__device__ __forceinline__ void bnr_st8(double *p, double v)
{
    if constexpr ((BNR_STORE_THROUGH & SITE) != 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
// 16 bytes (16-byte aligned): there is no 16-byte atomic, so the instruction is written out.  s_nop 1: a store of more than 8 bytes reads its data registers over
// two more cycles, and the compiler, which does not look into the string, may overwrite them with its very next instruction
template <int SITE>
__device__ __forceinline__ void bnr_st16(double *p, const double __attribute__((ext_vector_type(2))) v)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    if constexpr ((BNR_STORE_THROUGH & SITE) != 0) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
    else *(d2 *)p = v;
}


// How a sweep kernel finds its chain.  One chain: the struct travels by value in the kernel arguments (no dependent
// load in front of the first useful one -- the sweep of a single chain is a latency chain of ~30 launches).  Lockstep
// group: a device array indexed by blockIdx.z (one more scalar load, paid once per launch for all members).
// get_x(): kernels whose grid is (chain, workgroup) -- chain fastest, so that the workgroups with the same role of all
// members are dispatched together (k_chol_step: every member's panel workgroups before anybody's update workgroups).
// A descriptor read from memory carries GENERIC pointers: the compiler would emit flat_load/flat_store for everything
// reached through them, and flat operations also count on lgkmcnt -- every wait for an LDS read would then wait for
// the global loads in flight as well (measured in k_gram: the staging loads' latency exposed once per batch).  The
// descriptor's pointers are therefore passed through an address-space cast, after which they are known to be global
// (what the compiler infers by itself for a by-value kernel argument).
// (through an integer: a plain generic -> global -> generic cast pair is folded away before the inference pass runs)
#define BNR_GLOBAL_PTR(member) d.member = (decltype(d.member))(__attribute__((address_space(1))) void *)(unsigned long long)(d.member)
__device__ __forceinline__ bnr_dev bnr_globalized(const bnr_dev *src)
{
    bnr_dev d = *src;
    BNR_GLOBAL_PTR(X); BNR_GLOBAL_PTR(X8); BNR_GLOBAL_PTR(XM); BNR_GLOBAL_PTR(Sdig); BNR_GLOBAL_PTR(y); BNR_GLOBAL_PTR(ek); BNR_GLOBAL_PTR(el); BNR_GLOBAL_PTR(trace); BNR_GLOBAL_PTR(plan);
    BNR_GLOBAL_PTR(pbase); BNR_GLOBAL_PTR(Wbuf); BNR_GLOBAL_PTR(sz); BNR_GLOBAL_PTR(PW); BNR_GLOBAL_PTR(PA); BNR_GLOBAL_PTR(PG);
    BNR_GLOBAL_PTR(Gpart); BNR_GLOBAL_PTR(E); BNR_GLOBAL_PTR(gmap); BNR_GLOBAL_PTR(a3); BNR_GLOBAL_PTR(xw); BNR_GLOBAL_PTR(a4);
    BNR_GLOBAL_PTR(res); BNR_GLOBAL_PTR(xg); BNR_GLOBAL_PTR(bw); BNR_GLOBAL_PTR(wv); BNR_GLOBAL_PTR(scal); BNR_GLOBAL_PTR(Minv);
    BNR_GLOBAL_PTR(Psum); BNR_GLOBAL_PTR(counters); BNR_GLOBAL_PTR(dbg); BNR_GLOBAL_PTR(stamp); BNR_GLOBAL_PTR(gprog); BNR_GLOBAL_PTR(gmapc); BNR_GLOBAL_PTR(dfctl);
    return d;
}
struct bnr_one {
    bnr_dev d;
    static constexpr bool whole = true, lone = true;     // whole: the chain's whole descriptor is at hand; lone: a launch of one chain
    __device__ __forceinline__ const bnr_dev &get() const { return d; }
    __device__ __forceinline__ const bnr_dev &get_x() const { return d; }
    __device__ __forceinline__ const bnr_dev &at(int) const { return d; }
};
struct bnr_many {
    const bnr_dev *p;
    static constexpr bool whole = true, lone = false;
    __device__ __forceinline__ bnr_dev get() const { return bnr_globalized(p + blockIdx.z); }
    __device__ __forceinline__ bnr_dev get_x() const { return bnr_globalized(p + blockIdx.x); }
    __device__ __forceinline__ bnr_dev at(int c) const { return bnr_globalized(p + c); }
};
// A lockstep group of at most 8 chains, for the kernels that need next to nothing of a chain's descriptor (the panel steps p >= 2 of the factorization: E,
// n_pad, the failure counters): those few words travel BY VALUE in the kernel arguments, indexed by the grid's chain coordinate -- one scalar load from
// the kernarg segment instead of "load the descriptor's address, then load the descriptor" in front of the first useful load (a panel step is a chain of
// a few dependent round trips: one fewer is ~0.4 us per step, 16 steps per sweep).
struct bnr_few {
    double *E[8];
    long long *counters[8];
    unsigned long long *dbg[8];
    int n_pad;
    static constexpr bool whole = false, lone = false;
    __device__ __forceinline__ bnr_dev get_x() const
    {
        bnr_dev d{};
        d.E = E[blockIdx.x]; d.counters = counters[blockIdx.x]; d.dbg = dbg[blockIdx.x]; d.n_pad = n_pad;
        BNR_GLOBAL_PTR(E); BNR_GLOBAL_PTR(counters); BNR_GLOBAL_PTR(dbg);
        return d;
    }
    __device__ __forceinline__ bnr_dev get() const { return get_x(); }
    __device__ __forceinline__ bnr_dev at(int) const { return get_x(); }
};
// A failed factorization of G + I (a non-positive or non-finite pivot in any panel, a column of the panel pipeline that never arrived, a non-finite S in front of
// the i8 Gram) is the reference's ONE PosDefException of gibbs.jl:434: every wave and launch that meets it only raises the chain's flag word, and k_solve_w --
// the first launch behind the whole factorization -- turns the flag into one count (counters[3] and the "G+I" place counters[7]) and clears it.  So the count
// is one per failed gamma update whatever the family, the number of panels that see the bad pivot or the group the chain runs in.
__device__ __forceinline__ void bnr_flag_gfail(const bnr_dev &cd) { atomicOr((unsigned long long *)&cd.counters[9], 1ull); }


// wave-uniform values pinned to scalar registers (v_readfirstlane): inside a task loop the compiler cannot use scalar loads for what it
// reads after the first store of the kernel, and a uniform value left in a vector register drags the address arithmetic built on it there too
__device__ __forceinline__ int bnr_sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double bnr_sgpr_f64(double x) { return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x))); }
template <class T>
__device__ __forceinline__ T *bnr_sgpr_global(T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (T *)(__attribute__((address_space(1))) void *)(((unsigned long long)hi << 32) | lo);
}
// ---- single-wave small dense routines on LDS matrices (column-major R x R), blockDim.x == 64 or wave 0 of a block.
// `sync` must be a barrier valid for the participating threads: we always call these from code paths where the
// WHOLE block executes them (other waves just take part in the barriers).
// in-place lower Cholesky, right-looking; returns 0 ok / 1 not positive definite (uniform across the block)
__device__ inline int lds_chol(double *A, int R, int lane_in_block)
{
    for (int j = 0; j < R; ++j) {
        double d = A[j + R * j];
        if (!(d > 0.0) || !isfinite(d)) return 1;
        d = sqrt(d);
        __syncthreads();
        if (lane_in_block == j) A[j + R * j] = d;
        else if (lane_in_block > j && lane_in_block < R) A[lane_in_block + R * j] = A[lane_in_block + R * j] / d;
        __syncthreads();
        int m = R - j - 1;
        for (int idx = lane_in_block; idx < m * m; idx += blockDim.x) {
            int c = j + 1 + idx / m, i = j + 1 + idx % m;
            if (i >= c) A[i + R * c] = A[i + R * c] - A[i + R * j] * A[c + R * j];
        }
        __syncthreads();
    }
    return 0;
}
__device__ __forceinline__ double bnr_readlane_u(double v, int srclane /* wave-uniform */)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane), hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
// x (one value per lane, lane i < R holds b_i) <- L^-1 b ; column oriented, same operation order as a row sweep
__device__ __forceinline__ double wave_fwd_solve(const double *L, int R, int lane, double b)
{
    for (int k = 0; k < R; ++k) {
        double xk = bnr_readlane_u(b, k) / L[k + R * k];
        if (lane == k) b = xk;
        else if (lane > k && lane < R) b = b - L[lane + R * k] * xk;
    }
    return b;
}
// x <- L^-T b
__device__ __forceinline__ double wave_bwd_solve_T(const double *L, int R, int lane, double b)
{
    for (int k = R - 1; k >= 0; --k) {
        double xk = bnr_readlane_u(b, k) / L[k + R * k];
        if (lane == k) b = xk;
        else if (lane < k) b = b - L[k + R * lane] * xk;
    }
    return b;
}

// W_e = sum_r lam_r u[r,l] u[r,k]   (utils.jl:50-55 order; gibbs.jl:271,421,455)
__device__ __forceinline__ double edge_W(const double *u, const double *lam, int R, int l, int k)
{
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += u[r + R * l] * lam[r] * u[r + R * k];
    return s;
}

// ===================================================================================== k_node
// grid = V blocks, 64 threads (one wavefront per node).  mode bit0: tau2 for this row is drawn (else read from the row);
// bit1: node update; bit2: inv(M)/logdet M are recomputed here from row prev (test hooks) instead of read from cd.Minv.
// update_tau2! (gibbs.jl:267-277): tau2 ~ InverseGamma(n/2 + V(V+1)/4, rr/2 + sig_q) from the carried sums; k_tail of the
//   previous sweep has normally pre-drawn it (same draw site, same iteration id), otherwise it is drawn here.
// update_u_xi! (gibbs.jl:293-371) for node k = blockIdx.x, all inputs from row prev (no Gauss-Seidel).  Weights in
// log space (determinant lemma + Woodbury): log w_bot - log w_top = log(D/(1-D)) - 1/2[logdet M + logdet Sigma^-1]
// + 1/2 b' Sigma b,  b = U'H^-1 gamma_k / tau2 -- equal to the reference's ratio of dense (V-1)-dim pdfs whenever
// those do not under/overflow (gibbs.jl:349-351).  Option "xi_weights" = reference (cd.xi_ref): the two log densities themselves,
// l_top = log N(gamma_k; 0, tau2 H) (one more sum over the staged nodes) and l_bot = l_top - 1/2[logdet M + logdet Sigma^-1]
// + 1/2 b' Sigma b (the same lemma), and the reference's w = w_top / (w_bot + w_top) with its under/overflow (bnr_xi_weight_ref).
// The V-1 other nodes are staged through LDS in chunks of 64 (one per lane: U_a = u_a .* lambda, V_a = U_a / h_a,
// g_a / h_a), then lane p accumulates the p-th of the R(R+1)/2 + R sums sequentially over a (the reference's order).
#define BNR_NODE_MAXSUM 9      // ceil((32*33/2 + 32) / 64)
// (-DBNR_STAMPS, tools/stamps_timeline.py) a sweep's kernels on one clock: per kind 4 slots from dbg[4000]: s_memrealtime (100 MHz, the same on every XCD) at the entry of
// workgroup 0, the latest entry of any workgroup, the latest exit of any workgroup's thread 0.  atomicMax: what is read back belongs to the last sweep that ran.
#ifdef BNR_STAMPS
#define BNR_TL_IN(cd, kind, first) do { if (threadIdx.x == 0) { const unsigned long long rt_ = __builtin_amdgcn_s_memrealtime(); if (first) (cd).dbg[4000 + 4 * (kind)] = rt_; \
                                         atomicMax((unsigned long long *)&(cd).dbg[4000 + 4 * (kind) + 1], rt_); } } while (0)
#define BNR_TL_OUT(cd, kind) do { if (threadIdx.x == 0) atomicMax((unsigned long long *)&(cd).dbg[4000 + 4 * (kind) + 2], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
#else
#define BNR_TL_IN(cd, kind, first) do { } while (0)
#define BNR_TL_OUT(cd, kind) do { } while (0)
#endif
enum { TL_GRAM = 0, TL_SOLVE_W, TL_SOLVE_A4, TL_BACKPROJ, TL_PSUM, TL_TAIL, TL_TAIL_A, TL_NODE, TL_XPASS, TL_RHS, TL_SDIGITS, TL_KINDS };
template <class SRC>
__global__ __launch_bounds__(64) void k_node(const SRC chain_src, int s, int mode)
{
    const bnr_dev &cd = chain_src.get();
    extern __shared__ double shn[];                           // 64 x (2R + 1): per staged node [U(R) | V(R) | g/h], then the R x R work matrices
    const int lane = threadIdx.x, k = blockIdx.x, V = cd.V, R = cd.R;
    // (sized by the fit's R, not by BNR_RMAX: 800 of these one-wave workgroups run beside the panel steps of the factorization, and with 33 KB of static LDS
    // each they took the room that the next step's workgroups needed on the CU)
    double *sM = shn + 64 * (2 * R + 1), *sMinv = sM + R * R, *sS = sMinv + R * R, *sL = sS + R * R, *slam = sL + R * R, *sc = slam + R;
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    double *row = cd.trace + (size_t)P.row * cd.rowlen;
    const double *prev = cd.trace + (size_t)P.prev * cd.rowlen;
#ifdef BNR_STAMPS
    if (lane == 0 && k < 256) {                           // diagnostics: when did this node's wave start / finish its sums / end, and on which XCD
        unsigned v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
        unsigned h; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(h));
        cd.dbg[2000 + 4 * k] = __builtin_amdgcn_s_memrealtime(); cd.dbg[2000 + 4 * k + 3] = (v & 7u) | ((unsigned long long)h << 8);
    }
#endif
    BNR_TL_IN(cd, TL_NODE, k == 0);
    int cap = 0;
    double tau2;
    if (mode & 1) {
        if (cd.scal[SC_TAU2N_IT] == (double)P.it) tau2 = cd.scal[SC_TAU2N];
        else {
            double sigma = cd.scal[SC_RR] / 2.0 + cd.scal[SC_SIGQ];
            double shape = (cd.n / 2.0) + (V * (V + 1) / 4.0);
            tau2 = sigma / bnr_gamma(cd.seed, shape, P.it, SITE_TAU2, 0, &cap);
        }
        if (k == 0 && lane == 0) { row[ROW_TAU2] = tau2; cd.scal[SC_TAU] = sqrt(tau2); }
    } else {
        tau2 = row[ROW_TAU2];
        if (k == 0 && lane == 0) cd.scal[SC_TAU] = sqrt(tau2);
    }
    if (!(mode & 2)) { if (cap && lane == 0 && k == 0) atomicAdd((unsigned long long *)&cd.counters[2], 1ull); return; }

    const double Delta = prev[ROW_DELTA];
    const double *pu = prev + cd.o_u, *pg = prev + cd.o_gamma, *pS = prev + cd.o_S;
    if (lane < R) slam[lane] = prev[cd.o_lam + lane];
    if (mode & 4) for (int i = lane; i < R * R; i += 64) sM[i] = prev[cd.o_M + i];
    else for (int i = lane; i < R * R; i += 64) sMinv[i] = cd.Minv[i];
    __syncthreads();

    // which sums does this lane own: index p = lane + 64 m over pairs (x, y), y = x..R (y == R: the c_x sums)
    const int W2 = 2 * R + 1, npair = R * (R + 1) / 2 + R;
    int px[BNR_NODE_MAXSUM], py[BNR_NODE_MAXSUM];
    double acc[BNR_NODE_MAXSUM];
#pragma unroll
    for (int m = 0; m < BNR_NODE_MAXSUM; ++m) {
        int p = lane + 64 * m, x = 0;
        acc[m] = 0.0;
        if (p < npair) { int rem = p; while (rem >= R - x + 1) { rem -= R - x + 1; ++x; } px[m] = x; py[m] = x + rem; }
        else { px[m] = 0; py[m] = 0; }
    }
    const bool xref = cd.xi_ref != 0;
    double ltp = 0.0;                                         // xi_weights = reference: this lane's part of l_top (its staged nodes, in the order of a)
    for (int a0 = 0; a0 < V - 1; a0 += 64) {
        const int a = a0 + lane;
        if (a < V - 1) {
            int l = a < k ? a : a + 1;
            int e = l > k ? bnr_edge_index(V, l, k) : bnr_edge_index(V, k, l);
            double h = pS[e], g = pg[e];
            double *dst = shn + (size_t)lane * W2;
            for (int x = 0; x < R; ++x) { double ux = pu[x + R * l] * slam[x]; dst[x] = ux; dst[R + x] = ux / h; }
            dst[2 * R] = g / h;
            if (xref) { const double th = tau2 * h; ltp += -0.5 * (log(2.0 * BNR_PI) + log(th) + g * g / th); }   // logpdf N(gamma_kl; 0, tau2 h), gibbs.jl:349
        }
        __syncthreads();
        const int na = min(64, V - 1 - a0);
#pragma unroll
        for (int m = 0; m < BNR_NODE_MAXSUM; ++m) {
            if (lane + 64 * m < npair) {
                const double *pa = shn + px[m], *pb = shn + R + py[m];
                double t = acc[m];
                for (int aa = 0; aa < na; ++aa) t += pa[(size_t)aa * W2] * pb[(size_t)aa * W2];
                acc[m] = t;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < BNR_NODE_MAXSUM; ++m) {
        if (lane + 64 * m < npair) {
            if (py[m] == R) sc[px[m]] = acc[m];
            else { sS[px[m] + R * py[m]] = acc[m]; sS[py[m] + R * px[m]] = acc[m]; }
        }
    }
    __syncthreads();

#ifdef BNR_STAMPS
    if (lane == 0 && k < 256) cd.dbg[2000 + 4 * k + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    double logdetM;
    int fail = 0;
    if (mode & 4) {
        // inv(M) and logdet M via Cholesky of M_prev (gibbs.jl:315)
        for (int i = lane; i < R * R; i += 64) sL[i] = sM[i];
        __syncthreads();
        fail = lds_chol(sL, R, lane);
        logdetM = 0.0;
        for (int i = 0; i < R; ++i) logdetM += 2.0 * log(sL[i + R * i]);
        for (int j = 0; j < R; ++j) {
            double b = (lane == j) ? 1.0 : 0.0;
            b = wave_fwd_solve(sL, R, lane, b);
            b = wave_bwd_solve_T(sL, R, lane, b);
            if (lane < R) sMinv[lane + R * j] = b;
        }
        __syncthreads();
    } else logdetM = cd.Minv[R * R];
    // Sigma^-1 = A / tau2 + inv(M), Cholesky with the reference's jitter ladder (gibbs.jl:322-347)
    for (int i = lane; i < R * R; i += 64) sS[i] = sS[i] / tau2 + sMinv[i];
    __syncthreads();
    for (int i = lane; i < R * R; i += 64) sL[i] = sS[i];
    __syncthreads();
    int f2 = lds_chol(sL, R, lane);
    if (f2) {
        if (lane == 0) atomicAdd((unsigned long long *)&cd.counters[0], 1ull);
        __syncthreads();
        for (int i = lane; i < R; i += 64) sS[i + R * i] += 1e-5;
        __syncthreads();
        for (int i = lane; i < R * R; i += 64) sL[i] = sS[i];
        __syncthreads();
        f2 = lds_chol(sL, R, lane);
        if (f2) {
            __syncthreads();
            for (int i = lane; i < R; i += 64) sS[i + R * i] += 4e-5;
            __syncthreads();
            for (int i = lane; i < R * R; i += 64) sL[i] = sS[i];
            __syncthreads();
            f2 = lds_chol(sL, R, lane);
        }
    }
    if (fail || f2) {
        if (lane == 0) { atomicAdd((unsigned long long *)&cd.counters[3], 1ull); atomicAdd((unsigned long long *)&cd.counters[4], 1ull); }
        if (lane < R) row[cd.o_u + lane + R * k] = NAN;
        if (lane == 0) row[cd.o_xi + k] = NAN;
        return;
    }
    // (the R logarithms side by side in R lanes, then added in the order of i: the same sum as one after the other in every lane, a seventh of the dependent log evaluations at R = 7)
    const double lgS = (lane < R) ? 2.0 * log(sL[lane + R * lane]) : 0.0;
    double ldS = 0.0;
    for (int i = 0; i < R; ++i) ldS += bnr_readlane_u(lgS, i);
    // b = c / tau2 ; mu_t = Sigma b (gibbs.jl:364)
    double b = (lane < R) ? sc[lane] / tau2 : 0.0;
    double mt = wave_fwd_solve(sL, R, lane, b);
    mt = wave_bwd_solve_T(sL, R, lane, mt);
    double qf = wave_sum((lane < R) ? b * mt : 0.0);
    double w;
    if (xref) {
        // the reference's two dense (V-1)-dim pdfs (gibbs.jl:349-351) by the determinant lemma and Woodbury
        const double lt = wave_sum(ltp);
        const double lb = lt - 0.5 * (logdetM + ldS) + 0.5 * qf;
        w = bnr_xi_weight_ref(lt, lb, Delta);
    } else {
        double logit = log(Delta) - log1p(-Delta) - 0.5 * (logdetM + ldS) + 0.5 * qf;
        w = 1.0 / (1.0 + exp(logit));
    }
    // update_xi (gibbs.jl:385-402)
    double xi;
    if (w <= 0.0) xi = 1.0;
    else if (w >= 1.0) xi = 0.0;
    else {
        double ua, ub;
        bnr_draw2(cd.seed, P.it, SITE_XI, (uint32_t)k, 0, ua, ub);
        if (isnan(w)) { xi = (ua <= 0.5) ? 1.0 : 0.0; if (lane == 0) atomicAdd((unsigned long long *)&cd.counters[1], 1ull); }
        else xi = (ua <= 1.0 - w) ? 1.0 : 0.0;
    }
    // u_k = xi (mu_t + inv(C.U) z), z ~ N(0, I_R) (gibbs.jl:365-367)
    double z = (lane < R) ? bnr_normal(cd.seed, P.it, SITE_U_Z, (uint32_t)(k * R + lane), 0) : 0.0;
    z = wave_bwd_solve_T(sL, R, lane, z);
    if (lane < R) row[cd.o_u + lane + R * k] = xi * (mt + z);
    if (lane == 0) row[cd.o_xi + k] = xi;
    if (cap && lane == 0 && k == 0) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
#ifdef BNR_STAMPS
    if (lane == 0 && k < 256) cd.dbg[2000 + 4 * k + 2] = __builtin_amdgcn_s_memrealtime();
#endif
    BNR_TL_OUT(cd, TL_NODE);
}

// in-place lower Cholesky of an LDS matrix by ONE wavefront (all 64 lanes call); returns 0 ok / 1 not positive definite
__device__ inline int wave_chol(double *A, int R, int lane)
{
    for (int j = 0; j < R; ++j) {
        bnr_wsync();
        double d = A[j + R * j];
        if (!(d > 0.0) || !isfinite(d)) return 1;
        d = sqrt(d);
        bnr_wsync();
        for (int i = j + lane; i < R; i += 64) A[i + R * j] = (i == j) ? d : A[i + R * j] / d;
        bnr_wsync();
        int m = R - j - 1;
        for (int idx = lane; idx < m * m; idx += 64) {
            int c = j + 1 + idx / m, i = j + 1 + idx % m;
            if (i >= c) A[i + R * c] = A[i + R * c] - A[i + R * j] * A[c + R * j];
        }
    }
    bnr_wsync();
    return 0;
}
// T = inverse of the lower-triangular LDS matrix A (column j by lane j; R <= 32)
__device__ inline void wave_tri_inverse(const double *A, double *T, int R, int lane)
{
    if (lane < R) {
        const int j = lane;
        for (int i = 0; i < R; ++i) {
            double v = 0.0;
            if (i == j) v = 1.0 / A[j + R * j];
            else if (i > j) {
                double sacc = 0.0;
                for (int k = j; k < i; ++k) sacc += A[i + R * k] * T[k + R * j];
                v = -sacc / A[i + R * i];
            }
            T[i + R * j] = v;
        }
    }
    bnr_wsync();
}


// ===================================================================================== the early part of the scalar tail: Delta and M (gibbs.jl:496-499, 516-548)
// update_Delta! needs xi, update_M! needs u and xi: k_node's output of the sweep, not the back-projection's; and nothing in the rest of the tail needs THEM.  Round 6: in a sweep
// they are no longer a phase of k_tail's one workgroup per chain (32 us alone / 58 us beside the Gram's drain, of which this part was 12-20) but a SECOND workgroup of the same
// launch (k_tail, blockIdx.x == 1) that runs beside the first on another CU.  (First cut of the round: one extra workgroup per chain in the launch of the X pass that follows
// k_node -- it hid the work completely for a group, but a chain alone got a 24 us X pass instead of 13: its serial 18 us workgroup was the launch's long pole.)
// The draws are keyed by (iteration, site, element): bitwise the values of rounds 1-5.
//   mask bits: 2 Delta, 4 M, 256 inv(M) and logdet M for the next k_node (cd.Minv).
//   Called by EVERY thread of a workgroup of >= 256 threads (block barriers inside); threads 256.. only take part in the barriers.
//   lds: 4 R^2 + 8 doubles.
#define BNR_TAIL_EARLY (2 | 4 | 256)
__host__ __device__ inline size_t bnr_tail_a_lds_doubles(int R) { return (size_t)4 * R * R + 8; }
// ustage (round 6, second half): R V doubles of LDS, or nullptr.  Psi = I + sum_v u_v u_v' is a sum in the order of v per entry; with u read from the table row the loop
// is V / 4 dependent round trips to memory (four nodes' loads in flight): 25 of them at V = 100 were 15 of this function's 18 us.  Staged once -- one round trip -- the same
// terms are added in the same order out of LDS.
__device__ __forceinline__ void bnr_tail_a(const bnr_dev &cd, const bnr_plan_entry P, int mask, double *lds, int tid, bool mirror = false, double *ustage = nullptr)
{
    // mirror: this is workgroup 1 of a sweep's two-workgroup launch and the row is being copied to the head of the table by workgroup 0 at the same time (purge ring,
    // gibbs.jl:857-860): workgroup 0 leaves Delta and M out of its copy, they are written to the copies from here
    double *ring0 = (mirror && (P.wrap & 1) && P.row != 0) ? cd.trace : nullptr, *ring1 = (mirror && (P.wrap & 1) && (P.wrap & 4)) ? cd.trace + cd.rowlen : nullptr;
    const int R = cd.R, V = cd.V, RR = R * R;
    double *sPsi = lds, *sA = lds + RR, *sT = lds + 2 * RR, *sBm = lds + 3 * RR, *sredA = lds + 4 * RR;     // sredA: 2 x 4 wave partials
    const bool act = tid < 256;
    const int wave = bnr_sgpr(tid >> 6), lane = tid & 63;
    double *row = bnr_sgpr_global(cd.trace + (size_t)P.row * cd.rowlen);
    const double *su_row = row + cd.o_u;
    int cap = 0;
    if (ustage && (mask & 4)) { for (int i = tid; i < R * V; i += (int)blockDim.x) ustage[i] = su_row[i]; }
    // sum xi, #nonzero xi (sums of zeros and ones: exact whatever the order)
    if (act && (mask & (2 | 4))) {
        double sxi = 0.0, snz = 0.0;
        for (int v = tid; v < V; v += 256) { double x = row[cd.o_xi + v]; sxi += x; snz += (!(fabs(x) <= 0.1)) ? 1.0 : 0.0; }
        sxi = wave_sum(sxi); snz = wave_sum(snz);
        if (lane == 0) { sredA[wave] = sxi; sredA[4 + wave] = snz; }
    }
    // Psi = I + sum_v u_v u_v' (gibbs.jl:516-525), sequential over v per entry (the reference's order); u from the table row (k_node has just written it)
    if (ustage && (mask & 4)) {
        __syncthreads();
        if (act) {
            for (int idx = tid; idx < RR; idx += 256) {
                const int a = idx % R, b = idx / R;
                double sacc = (a == b) ? 1.0 : 0.0;
                int v = 0;
                for (; v + 3 < V; v += 4) {
                    const double a0 = ustage[a + R * v], b0 = ustage[b + R * v], a1 = ustage[a + R * (v + 1)], b1 = ustage[b + R * (v + 1)];
                    const double a2 = ustage[a + R * (v + 2)], b2 = ustage[b + R * (v + 2)], a3 = ustage[a + R * (v + 3)], b3 = ustage[b + R * (v + 3)];
                    sacc += a0 * b0; sacc += a1 * b1; sacc += a2 * b2; sacc += a3 * b3;
                }
                for (; v < V; ++v) sacc += ustage[a + R * v] * ustage[b + R * v];
                sPsi[idx] = sacc;
                sA[idx] = sacc;
            }
        }
    } else
    if (act && (mask & 4)) {
        for (int idx = tid; idx < RR; idx += 256) {
            const int a = idx % R, b = idx / R;
            double sacc = (a == b) ? 1.0 : 0.0;
            int v = 0;
            for (; v + 3 < V; v += 4) {                 // four nodes' loads in flight, the terms added one after the other in the order of v
                const double a0 = su_row[a + R * v], b0 = su_row[b + R * v], a1 = su_row[a + R * (v + 1)], b1 = su_row[b + R * (v + 1)];
                const double a2 = su_row[a + R * (v + 2)], b2 = su_row[b + R * (v + 2)], a3 = su_row[a + R * (v + 3)], b3 = su_row[b + R * (v + 3)];
                sacc += a0 * b0; sacc += a1 * b1; sacc += a2 * b2; sacc += a3 * b3;
            }
            for (; v < V; ++v) sacc += su_row[a + R * v] * su_row[b + R * v];
            sPsi[idx] = sacc;
            sA[idx] = sacc;
        }
    }
    __syncthreads();
    double sxi = 0.0, snz = 0.0;
    if (mask & (2 | 4)) for (int w = 0; w < 4; ++w) { sxi += sredA[w]; snz += sredA[4 + w]; }
    sxi = bnr_sgpr_f64(sxi); snz = bnr_sgpr_f64(snz);
    const double df = cd.nu + snz;
    // independent work on separate wavefronts
    if (act && wave == 0 && (mask & 2)) {                                        // Delta (gibbs.jl:496-499, 130-140)
        double a = cd.aDelta + sxi, b = cd.bDelta + ((double)V - sxi);
        double g = 0.0;
        if (a > 0.0 && b > 0.0 && lane < 2) g = bnr_gamma(cd.seed, lane == 0 ? a : b, P.it, SITE_DELTA, (uint32_t)lane, &cap);
        double g1 = bnr_readlane_c(g, 0), g2 = bnr_readlane_c(g, 1);
        if (lane == 0) {
            double out;
            if (a > 0.0 && b > 0.0) out = g1 / (g1 + g2);
            else if (a > 0.0) out = 1.0;
            else if (b > 0.0) out = 0.0;
            else { double ua, ub; bnr_draw2(cd.seed, P.it, SITE_DELTA_COIN, 0, 0, ua, ub); out = (ua < 0.5) ? 0.0 : 1.0; }
            row[ROW_DELTA] = out;
            if (ring0) ring0[ROW_DELTA] = out;
            if (ring1) ring1[ROW_DELTA] = out;
        }
    }
    if (act && wave == 1 && (mask & 4)) {                                        // Bartlett diagonal: chi-square draws
        for (int j = lane; j < R; j += 64) sBm[j + R * j] = sqrt(2.0 * bnr_gamma(cd.seed, 0.5 * (df - j), P.it, SITE_M_CHI, (uint32_t)j, &cap));
    }
    if (act && wave == 2 && (mask & 4)) {                                        // Bartlett strictly lower: normals; upper: 0
#pragma unroll 1
        for (int idx = lane; idx < RR; idx += 64) {
            int i = idx % R, j = idx / R;
            if (i > j) sBm[idx] = bnr_normal(cd.seed, P.it, SITE_M_N, (uint32_t)(i * R + j), 0);
            else if (i < j) sBm[idx] = 0.0;
        }
    }
    if (act && wave == 3 && (mask & 4)) {                                        // C = chol(Psi), retry ladder gibbs.jl:529-543
        int f = wave_chol(sA, R, lane);
        if (f) {
            if (lane == 0) atomicAdd((unsigned long long *)&cd.counters[0], 1ull);
            for (int idx = lane; idx < RR; idx += 64) sA[idx] = sPsi[idx] + ((idx % R == idx / R) ? 1e-5 : 0.0);
            f = wave_chol(sA, R, lane);
            if (f && lane == 0) { atomicAdd((unsigned long long *)&cd.counters[3], 1ull); atomicAdd((unsigned long long *)&cd.counters[5], 1ull); }
        }
        for (int idx = lane; idx < RR; idx += 64) { int a = idx % R, b = idx / R; if (a < b) sA[idx] = 0.0; }
    }
    __syncthreads();
    // wavefront 0, wave-level sync: M ~ InverseWishart(df, Psi) = (C A^-T)(C A^-T)', then inv(M), logdet M
    if (act && wave == 0 && (mask & (4 | 256))) {
        if (mask & 4) {
            wave_tri_inverse(sBm, sT, R, lane);                                   // T = A^-1
            for (int idx = lane; idx < RR; idx += 64) {                           // B = C T' -> sPsi
                int a = idx % R, b = idx / R;
                double sacc = 0.0;
                for (int k = 0; k < R; ++k) sacc += sA[a + R * k] * sT[b + R * k];
                sPsi[idx] = sacc;
            }
            bnr_wsync();
            for (int idx = lane; idx < RR; idx += 64) {                           // M = B B'
                int a = idx % R, b = idx / R;
                double sacc = 0.0;
                for (int k = 0; k < R; ++k) sacc += sPsi[a + R * k] * sPsi[b + R * k];
                row[cd.o_M + idx] = sacc;
                if (ring0) ring0[cd.o_M + idx] = sacc;
                if (ring1) ring1[cd.o_M + idx] = sacc;
                sBm[idx] = sacc;
            }
        } else {
            for (int idx = lane; idx < RR; idx += 64) sBm[idx] = row[cd.o_M + idx];
        }
        bnr_wsync();
        if (mask & 256) {
            // inv(M) = Lm^-T Lm^-1 with Lm = chol(M) (gibbs.jl:315 computes inv(M); same matrix, triangular-inverse route)
            for (int idx = lane; idx < RR; idx += 64) sA[idx] = sBm[idx];
            int f = wave_chol(sA, R, lane);
            if (f && lane == 0) { atomicAdd((unsigned long long *)&cd.counters[3], 1ull); atomicAdd((unsigned long long *)&cd.counters[6], 1ull); }
            const double lgm = (lane < R) ? 2.0 * log(sA[lane + R * lane]) : 0.0;      // (side by side, added in the order of i: see k_node)
            double ldm = 0.0;
            for (int i = 0; i < R; ++i) ldm += bnr_readlane_u(lgm, i);
            wave_tri_inverse(sA, sT, R, lane);                                    // Linv (lower)
            for (int idx = lane; idx < RR; idx += 64) {
                int a = idx % R, b = idx / R, k0 = a > b ? a : b;
                double sacc = 0.0;
                for (int k = k0; k < R; ++k) sacc += sT[k + R * a] * sT[k + R * b];
                cd.Minv[idx] = sacc;
            }
            if (lane == 0) cd.Minv[RR] = ldm;
        }
    }
    if (cap) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
}

// ===================================================================================== k_xpass
// One pass over X.  grid = nblk_x blocks of 256 threads; block b owns columns [b*chunk, (b+1)*chunk).
//   W_e  = lowtri(u_new' diag(lam_prev) u_new)_e               (gibbs.jl:421)           -> Wbuf
//   sz_e = sqrt(S_prev,e) * z1_e   (Delta_gamma1 = tau * sz)   (gibbs.jl:429)           -> sz
//   PW[b][i] = sum_{e in chunk} X[i,e] W_e ;  PA[b][i] = sum X[i,e] sz_e                 (gibbs.jl:432-433)
// which: bit0 -> W/PW, bit1 -> sz/PA, bit2 -> PG = partial X*gamma(row `P.prev` if bit3 else row P.row)
template <class SRC>
__global__ __launch_bounds__(256) void k_xpass(const SRC chain_src, int s, int which, int nchains)
{
    // 1-D grid = round_up(blocks, 8) x chains, decoded like k_gram / k_backproj (chains that read the same columns of X are neighbours on one XCD)
    extern __shared__ double sh[];
    const int gid = blockIdx.x;
    const int gx = gid & 7, gr = gid >> 3;
    const int bid = (gr / nchains) * 8 + gx;
    const bnr_dev &cd = chain_src.at(gr % nchains);
    if (bid >= cd.nblk_x) return;
    BNR_TL_IN(cd, TL_XPASS, bid == 0);
    double *sW = sh, *sZ = sh + cd.chunk_x, *sG = sh + 2 * cd.chunk_x;
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    const double *row = cd.trace + (size_t)P.row * cd.rowlen;
    const double *prev = cd.trace + (size_t)P.prev * cd.rowlen;
    const int R = cd.R;
    const int e0 = bid * cd.chunk_x;
    const int ne = min(cd.chunk_x, cd.q - e0);
    const double *grow = (which & 8) ? prev : row;
    for (int t = threadIdx.x; t < cd.chunk_x; t += blockDim.x) {
        double w = 0.0, zz = 0.0, g = 0.0;
        int e = e0 + t;
        if (t < ne) {
            if (which & 1) { w = edge_W(row + cd.o_u, prev + cd.o_lam, R, cd.el[e], cd.ek[e]); cd.Wbuf[e] = w; }
            if (which & 2) { zz = sqrt(prev[cd.o_S + e]) * bnr_normal(cd.seed, P.it, SITE_G_Z1, (uint32_t)e, 0); cd.sz[e] = zz; }
            if (which & 4) g = grow[cd.o_gamma + e];
        }
        sW[t] = w; sZ[t] = zz; sG[t] = g;
    }
    __syncthreads();
    const size_t ld = cd.n_pad;
    for (int i = threadIdx.x; i < cd.n_pad; i += blockDim.x) {
        double aw = 0.0, aa = 0.0, ag = 0.0;
        // the same fused multiply-adds in the same order from either image of X (a byte converts exactly)
#define BNR_XPASS_BODY(XP)                                                                                          \
        if ((which & 7) == 3) {                                                                                     \
            _Pragma("unroll 4") for (int t = 0; t < ne; ++t) { double x = (double)(XP)[(size_t)t * ld]; aw = fma(x, sW[t], aw); aa = fma(x, sZ[t], aa); } \
        } else {                                                                                                    \
            for (int t = 0; t < ne; ++t) {                                                                          \
                double x = (double)(XP)[(size_t)t * ld];                                                            \
                aw = fma(x, sW[t], aw); aa = fma(x, sZ[t], aa); ag = fma(x, sG[t], ag);                             \
            }                                                                                                       \
        }
        if (cd.X8) { const unsigned char *xp = cd.X8 + (size_t)e0 * ld + i; BNR_XPASS_BODY(xp) }
        else { const double *xp = cd.X + (size_t)e0 * ld + i; BNR_XPASS_BODY(xp) }
        if (which & 1) bnr_st8<BNR_ST_XPASS>(cd.PW + (size_t)bid * ld + i, aw);
        if (which & 2) bnr_st8<BNR_ST_XPASS>(cd.PA + (size_t)bid * ld + i, aa);
        if (which & 4) cd.PG[(size_t)bid * ld + i] = ag;
    }
    BNR_TL_OUT(cd, TL_XPASS);
}

// k_xpass for a lockstep group whose members share the model matrix (chains of one fit: bnr_chain_create_like): ONE workgroup handles a
// column chunk and a slice of 256 rows for up to eight chains at once -- an element of X is loaded once and enters 16 fused multiply-adds
// (two GEMV partials per chain) instead of being fetched again by every chain's own workgroup.  Per chain the same products in the same
// order (columns of the chunk ascending), the same partial vectors PW / PA: bitwise k_xpass.  Eight chains read an eighth of the
// bytes from the L2s, and the factorization's panel steps that run beside this kernel keep their memory latency (a dependent launch
// beside a streaming kernel: 21 us instead of 6.6, tools/interfere_probe.hip).  which = 3 only (W and sqrt(S) z1).
//   grid = nblk_x x ceil(n_pad / 256), 256 threads, dynamic LDS = 2 x 8 x chunk_x doubles.
__global__ __launch_bounds__(256) void k_xpass_group(const bnr_many chain_src, int s, int nchains)
{
    extern __shared__ double sh[];
    const int wg = blockIdx.x;
    const bnr_dev &c0 = chain_src.at(0);                  // the geometry and the shared X, index maps
    const int rs = (c0.n_pad + 255) / 256, bid = wg / rs, slice = wg % rs, tid = threadIdx.x;
    const int chunk = c0.chunk_x, e0 = bid * chunk, ne = min(chunk, c0.q - e0), R = c0.R;
    const size_t ld = c0.n_pad;
    double *sW = sh, *sZ = sh + 8 * chunk;                 // [chain][column of the chunk]
    __shared__ double *s_pw[8], *s_pa[8];
    const int i = slice * 256 + tid;
    const bool live = i < c0.n_pad;                        // n_pad is a multiple of 64: the last slice may be short
    const int ic = live ? i : 0;
    for (int cb = 0; cb < nchains; cb += 8) {
        const int nc = min(8, nchains - cb);
        __syncthreads();
        for (int it = tid; it < nc * chunk; it += 256) {
            const int c = it / chunk, t = it - c * chunk;
            const bnr_dev &cd = chain_src.at(cb + c);
            const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
            const double *row = cd.trace + (size_t)P.row * cd.rowlen, *prev = cd.trace + (size_t)P.prev * cd.rowlen;
            double w = 0.0, zz = 0.0;
            if (t < ne) {
                const int e = e0 + t;
                w = edge_W(row + cd.o_u, prev + cd.o_lam, R, cd.el[e], cd.ek[e]);
                zz = sqrt(prev[cd.o_S + e]) * bnr_normal(cd.seed, P.it, SITE_G_Z1, (uint32_t)e, 0);
                if (slice == 0) { cd.Wbuf[e] = w; cd.sz[e] = zz; }
            }
            sW[c * chunk + t] = w; sZ[c * chunk + t] = zz;
        }
        if (tid < nc) { const bnr_dev &cd = chain_src.at(cb + tid); s_pw[tid] = cd.PW; s_pa[tid] = cd.PA; }
        __syncthreads();
        double aw[8], aa[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { aw[c] = 0.0; aa[c] = 0.0; }
#define BNR_XG_BODY(XP)                                                                                   \
        for (int t0 = 0; t0 < ne; t0 += 16) {                                                             \
            double xv[16];                                                                                \
            _Pragma("unroll") for (int u = 0; u < 16; ++u) xv[u] = (double)(XP)[(size_t)(t0 + u < ne ? t0 + u : ne - 1) * ld]; \
            _Pragma("unroll") for (int u = 0; u < 16; ++u) {                                              \
                if (t0 + u < ne) {                                                                        \
                    _Pragma("unroll") for (int c = 0; c < 8; ++c)                                         \
                        if (c < nc) { aw[c] = fma(xv[u], sW[c * chunk + t0 + u], aw[c]); aa[c] = fma(xv[u], sZ[c * chunk + t0 + u], aa[c]); } \
                }                                                                                         \
            }                                                                                             \
        }
        if (c0.X8) { const unsigned char *xp = c0.X8 + (size_t)e0 * ld + ic; BNR_XG_BODY(xp) }
        else { const double *xp = c0.X + (size_t)e0 * ld + ic; BNR_XG_BODY(xp) }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < nc && live) { bnr_st8<BNR_ST_XPASS>(s_pw[c] + (size_t)bid * ld + i, aw[c]); bnr_st8<BNR_ST_XPASS>(s_pa[c] + (size_t)bid * ld + i, aa[c]); }
    }
}

// ===================================================================================== k_gram
// G = X diag(S_prev) X'  (the n x n matrix of gibbs.jl:434 without the identity; tau cancels: Xt tau2 D Xt' = X D X').
// v_mfma_f64_16x16x4_f64, D = A*B + C with A[m][k] (lane l: m = l&15, k = l>>4), B[k][n] (k = l>>4, n = l&15),
// C[m][n]: lane l holds rows m = (l>>4) + 4*reg, column n = l&15.
// Here m indexes the tile's COLUMN (j) and n its ROW (i): A = X[j-rows], B = S_e X[i-rows], so that a lane's results are
// consecutive in i and the tile is written column-major (i fastest) with coalesced 128-byte segments.
// Workgroup = KG x 256 threads on one 64x64 tile of the LOWER triangle: KG K-groups x (2x2 waves of 32x32), the K-groups reduced through LDS.
// The f64 MFMA pipe issues one v_mfma_f64_16x16x4_f64 per 64 cycles per SIMD from a single wave (profiles/round5_mfma_f64_peak.txt); several
// waves per SIMD are there to hide the loop's staging work (global -> LDS -> fragments) and its barrier, not to raise the issue rate
// (the round-1 figures that once stood here, "139 / 103 / 92 cycles per MFMA at 1 / 2 / 4 waves", were a microbenchmark artefact).
// blockIdx.y = K slice across workgroups (split-K partials, summed by k_gram_reduce).
// Buffer loads: SGPR resource (base address) + 32-bit lane byte offset + SGPR byte offset.  The Gram loops advance the scalar offset only:
// no address arithmetic on the vector ALU (global_load with a loop-variant scalar base is selected as a 64-bit vector add per load).
typedef int bnr_i4 __attribute__((ext_vector_type(4)));
typedef int bnr_i2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bnr_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, 0x7FFFFFFF, 0x00020000);     // raw buffer, no stride, 2 GiB window, gfx9 data format word
}
__device__ __forceinline__ bnr_d2 bnr_bufload_d2(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    return __builtin_bit_cast(bnr_d2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, 0));
}
__device__ __forceinline__ double bnr_bufload_f64(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, soff, 0));
}
// A Gram workgroup has stored its partial tile: count it for the tile's column (the factorization checks the count before its
// first read of the column).  k_gram / k_gram8 are consumed after the kernel boundary: one relaxed atomic, no fence.
// Only the factorization experiments of rounds 3-4 that ran beside the Gram read the counts (tools/experiments/): the library does not
// count at all (round 3 did, on every launch: one agent-scope atomic per workgroup on 8 words per chain).
__device__ __forceinline__ void bnr_gram_count(const bnr_dev &cd, int tj)
{
    (void)cd; (void)tj;
}
#define BNR_GRAM_KB 16                // columns of X per staged batch (4 MFMA k-steps): one barrier per 16 MFMAs of a wave
// The Gram loops issue the loads of batch b + 2 while batch b is computed and never clamp: the last trips of a K-group read up to
// BNR_GRAM_LOOKAHEAD batches past its slice -- the next slice's columns, or past q_pad.  Both X (columns) and every trace row behind S
// (entries) are therefore followed by BNR_GRAM_PREFETCH_COLS zeros that nothing ever writes (bnr_chain_create); what is loaded there is
// stored to LDS and never used by a compute step, but it must be addressable and finite-times-zero must stay out of the sums.
#define BNR_GRAM_LOOKAHEAD 2
#define BNR_GRAM_PREFETCH_COLS 64
static_assert((BNR_GRAM_LOOKAHEAD + 1) * BNR_GRAM_KB <= BNR_GRAM_PREFETCH_COLS, "zero padding behind X and S must cover the Gram loops' prefetch distance (a half batch + two whole ones)");
// Span in bytes that ONE K-group's buffer resource must address (base = first column of its slice): its columns, the prefetch
// distance and the per-lane offset (at most 16 columns of n_pad rows).  The resource is a 2 GiB window with 32-bit scalar offsets:
// the host raises the K split until this fits (bnr_host_gram_plan; ADVICE r5: n = 14 000 with V >= 280 used to overflow silently).
__host__ __device__ inline long long bnr_gram_span_bytes(int n_pad, int kchunk, int kg)
{
    return ((long long)(kchunk / kg) + BNR_GRAM_PREFETCH_COLS + 16) * (long long)n_pad * 8;
}

// LDS-staged K loop.  Per K-group (4 waves = 256 threads) and batch of 16 columns: the j-side panel X[j-rows, 16 cols] and
// the S-scaled i-side panel travel global -> registers (16-byte loads, issued one whole batch ahead) -> LDS image
// [col][64 rows], and come back as MFMA fragments with ds_read_b64.  The image is unpadded; odd columns store their two
// 16-row halves swapped (row ^ 16), which puts the four columns of a fragment read on disjoint banks (the same
// conflict-free pattern a padded stride of 80 gives, in 20 % less LDS: 32 KiB per K-group, two workgroups per CU).
// One register set, two LDS buffers: after the barrier a wave first writes batch b+1 (loaded during batch b-1), re-issues
// the loads of batch b+2, then computes batch b.
// KG = K-groups per workgroup.  KG = 2: 512 threads and 64 KiB of LDS, TWO workgroups per CU, so that the prologue (first
// loads), the K-group reduction and the store of one workgroup overlap with the MFMA loop of its neighbour when a launch
// runs for several rounds (lockstep groups).  KG = 4: 1024 threads, one workgroup per CU.
// Grid (1-D) = round_up(tasks, 8) x chains.  Workgroup id -> XCD label id % 8 (round-robin dispatch), and within one
// XCD's sequence the chains of a lockstep group are innermost: the 8 (or C) workgroups that need the same panels of X
// (same tile, same K slice, different S) run next to each other on the same XCD and share them through its L2.
// a partial-tile element goes to memory through the L2 (BNR_ST_GRAM; consumed after the kernel boundary, on other XCDs).  The stores stay behind this helper: with
// "out[idx] = ..." written out in the task bodies the compiler schedules all six Gram kernels differently (profiles/kernel_variants_cleanup.txt)
__device__ __forceinline__ void bnr_gstore(double *p, double v) { bnr_st8<BNR_ST_GRAM>(p, v); }
// what a Gram task needs besides the chain's S row and its partial-tile buffer: equal for all members of a lockstep group
struct bnr_gram_geom { const double *X; int n_pad, q_pad, ksplit, q, ntile; };
__device__ __forceinline__ bnr_gram_geom bnr_geom_of(const bnr_dev &cd) { return bnr_gram_geom{cd.X, cd.n_pad, cd.q_pad, cd.ksplit, cd.q, cd.ntile}; }
// one (tile t = (ti, tj), K slice ks) task of the Gram with 16-column batches: KG x 256 threads, sred = KG x 32 KiB of LDS
template <int KG>
__device__ __forceinline__ void bnr_gram16_task(const bnr_gram_geom &cd, const double *Sp, double *Gpart, int t, int ti, int tj, int ks, double *sred)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kg = wave >> 2, wi = (wave >> 1) & 1, wj = wave & 1;
    const int kchunk = cd.q_pad / cd.ksplit;          // multiple of 8 KG (host guarantees)
    const int ksub = kchunk / KG;                     // multiple of 8
    const int eb = ks * kchunk + kg * ksub;
    const int nfull = ksub / BNR_GRAM_KB;             // whole batches; ksub % 16 == 8 leaves one half batch
    const bool half = (ksub % BNR_GRAM_KB) != 0;
    const size_t ld = cd.n_pad;
    const int li = lane & 15, lk = lane >> 4;
    // staging: this thread moves rows (2 rp, 2 rp + 1) of columns c and c + 8 of both panels.  Addresses = wave-uniform base
    // of the batch (SGPRs, advanced by scalar adds) + a per-lane offset that never changes
    const int tg = threadIdx.x & 255, c = tg >> 5, rp = tg & 31;
    // (32-bit BYTE offsets: scalar base + zero-extended lane offset is the addressing form of global_load with an SGPR base; 16 columns of
    // n_pad <= 16 384 rows stay below 4 GiB)
    const unsigned offI = 8u * ((unsigned)(ti * BNR_GT + 2 * rp) + (unsigned)c * (unsigned)ld), offJ = 8u * ((unsigned)(tj * BNR_GT + 2 * rp) + (unsigned)c * (unsigned)ld);
    const unsigned off8 = 8u * 8u * (unsigned)ld, offS = 8u * (unsigned)c;
    const double *xb = bnr_sgpr_global(cd.X + (size_t)eb * ld);        // uniform: first column of this K-group, pinned to scalar registers (see bnr_gram8_task)
    const double *sb = bnr_sgpr_global(Sp + eb);                       // uniform; S is followed by q_pad - q + BNR_GRAM_PREFETCH_COLS zeros in every trace row: no clamp
    const int PANEL = BNR_GRAM_KB * BNR_GT;                            // doubles per panel (16 columns x 64 rows)
    double *stg = sred + (size_t)kg * (4 * PANEL);                     // [buf][I|J][col][row ^ swizzle]
    const int woff = c * BNR_GT + ((2 * rp) ^ ((c & 1) << 4));         // columns c and c + 8 have the same parity
    // fragment rows of this lane: column 4 k2 + lk has parity lk & 1
    const int sw = (lk & 1) << 4;
    const int ra0 = (wj * 32 + li) ^ sw, ra1 = (wj * 32 + 16 + li) ^ sw, rb0 = (wi * 32 + li) ^ sw, rb1 = (wi * 32 + 16 + li) ^ sw;
    bnr_d4 c00 = {0, 0, 0, 0}, c01 = {0, 0, 0, 0}, c10 = {0, 0, 0, 0}, c11 = {0, 0, 0, 0};   // c[jt][it]
    bnr_d2 ri0, ri1, rj0, rj1;
    double sv0, sv1;
    const __amdgpu_buffer_rsrc_t rX = bnr_rsrc(xb), rS = bnr_rsrc(sb);
    const int bstep = BNR_GRAM_KB * (int)ld * 8;                       // bytes per batch (scalar)
#define BNR_GRAM_LOAD(BIDX)                                                                               \
    do {                                                                                                  \
        const int so_ = (BIDX) * bstep;                                                                   \
        sv0 = bnr_bufload_f64(rS, offS, (BIDX) * (BNR_GRAM_KB * 8)); sv1 = bnr_bufload_f64(rS, offS + 64u, (BIDX) * (BNR_GRAM_KB * 8)); \
        ri0 = bnr_bufload_d2(rX, offI, so_); ri1 = bnr_bufload_d2(rX, offI + off8, so_);                  \
        rj0 = bnr_bufload_d2(rX, offJ, so_); rj1 = bnr_bufload_d2(rX, offJ + off8, so_);                  \
    } while (0)
#define BNR_GRAM_STORE(BUF)                                                                               \
    do {                                                                                                  \
        double *nx_ = stg + (size_t)(BUF) * (2 * PANEL);                                                  \
        *(bnr_d2 *)(nx_ + woff) = ri0 * sv0;                                                          \
        *(bnr_d2 *)(nx_ + 8 * BNR_GT + woff) = ri1 * sv1;                                             \
        *(bnr_d2 *)(nx_ + PANEL + woff) = rj0;                                                            \
        *(bnr_d2 *)(nx_ + PANEL + 8 * BNR_GT + woff) = rj1;                                               \
    } while (0)
#define BNR_GRAM_COMPUTE(BUF, K2A, K2B, DIAG)                                                                 \
    do {                                                                                                  \
        const double *bufI = stg + (size_t)(BUF) * (2 * PANEL), *bufJ = bufI + PANEL;                     \
        _Pragma("unroll") for (int k2 = (K2A); k2 < (K2B); ++k2) {                                        \
            const int kk = (4 * k2 + lk) * BNR_GT;                                                        \
            double a0 = bufJ[kk + ra0], a1 = bufJ[kk + ra1];                                              \
            double b0 = bufI[kk + rb0], b1 = bufI[kk + rb1];                                              \
            c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);                             \
            c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);                             \
            if (!(DIAG)) c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);                \
            c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);                             \
        }                                                                                                 \
    } while (0)
    // batches past the end of the slice read the following columns or the zero-padded tail of X (the host allocates
    // q_pad + BNR_GRAM_PREFETCH_COLS columns); they are stored but never used by a compute step
    BNR_GRAM_LOAD(0);
    BNR_GRAM_STORE(0);
    BNR_GRAM_LOAD(1);
    __syncthreads();
    if (ti == tj && wi == 0 && wj == 1) {
        // the 32 x 32 block above the diagonal of a diagonal tile is read by nobody (k_gram_reduce copies it into the strictly upper
        // part of E, which the factorization never touches): its two waves only take part in the staging and leave zeros
        // (measured against computing it: 5.6 % of the launch's MFMAs at ntile = 8; 8 chains 216.5 -> 212.6 us per launch, 401.7 -> 396.6 us
        // per sweep, together with the 3 instead of 4 MFMAs per k-step of the diagonal waves below)
        int b = 0;
        for (; b + 1 < nfull; b += 2) {
            BNR_GRAM_STORE(1); BNR_GRAM_LOAD(b + 2); __syncthreads();
            BNR_GRAM_STORE(0); BNR_GRAM_LOAD(b + 3); __syncthreads();
        }
        if (b < nfull) { BNR_GRAM_STORE(1); BNR_GRAM_LOAD(b + 2); __syncthreads(); }
        if (half) __syncthreads();
    } else if (ti == tj && wi == wj) {
        // a diagonal 32 x 32 block: its upper 16 x 16 tile (c10: columns 16.., rows ..15) is read by nobody either -- three MFMAs per k-step
        // (two batches per trip, the buffer parity a literal: LDS addresses are "lane base + immediate", no address VALU in the loop)
#define BNR_GRAM_BATCH_L(B, PAR, DIAG)                                                                    \
        do {                                                                                              \
            BNR_GRAM_COMPUTE(PAR, 0, 2, DIAG);                                                            \
            BNR_GRAM_STORE((PAR) ^ 1);                                                                    \
            BNR_GRAM_LOAD((B) + 2);                                                                       \
            BNR_GRAM_COMPUTE(PAR, 2, 4, DIAG);                                                            \
            __syncthreads();                                                                              \
        } while (0)
        int b = 0;
        for (; b + 1 < nfull; b += 2) { BNR_GRAM_BATCH_L(b, 0, true); BNR_GRAM_BATCH_L(b + 1, 1, true); }
        if (b < nfull) BNR_GRAM_BATCH_L(b, 0, true);
        if (half) { if (nfull & 1) BNR_GRAM_COMPUTE(1, 0, 2, true); else BNR_GRAM_COMPUTE(0, 0, 2, true); __syncthreads(); }
    } else {
    // first half of the batch, then the staging work of the next one (batch b+1; its buffer was released by the last barrier), then the
    // second half: the wait for the loads issued one batch ago and the LDS writes sit behind 8 MFMAs already in flight (measured: +4 %
    // over staging first)
    int b = 0;
    for (; b + 1 < nfull; b += 2) { BNR_GRAM_BATCH_L(b, 0, false); BNR_GRAM_BATCH_L(b + 1, 1, false); }
    if (b < nfull) BNR_GRAM_BATCH_L(b, 0, false);
    if (half) { if (nfull & 1) BNR_GRAM_COMPUTE(1, 0, 2, false); else BNR_GRAM_COMPUTE(0, 0, 2, false); __syncthreads(); }
    }
    // tile element (i,j) lives at [j*64 + i]; this lane: j = wj*32 + jt*16 + (lane>>4) + 4 r, i = wi*32 + it*16 + (lane&15)
    double *mine = sred + (size_t)kg * (BNR_GT * BNR_GT);
    const int jb = wj * 32 + (lane >> 4), ib = wi * 32 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mine[(jb + 4 * r) * BNR_GT + ib] = c00[r];
        mine[(jb + 4 * r) * BNR_GT + ib + 16] = c01[r];
        mine[(jb + 16 + 4 * r) * BNR_GT + ib] = c10[r];
        mine[(jb + 16 + 4 * r) * BNR_GT + ib + 16] = c11[r];
    }
    __syncthreads();
    double *out = Gpart + ((size_t)ks * (cd.ntile * (cd.ntile + 1) / 2) + t) * (BNR_GT * BNR_GT);
#pragma unroll
    for (int idx = threadIdx.x; idx < BNR_GT * BNR_GT; idx += KG * 256) {
        if (KG == 4) bnr_gstore(out + idx, (sred[idx] + sred[BNR_GT * BNR_GT + idx]) + (sred[2 * BNR_GT * BNR_GT + idx] + sred[3 * BNR_GT * BNR_GT + idx]));
        else bnr_gstore(out + idx, sred[idx] + sred[BNR_GT * BNR_GT + idx]);
    }
}
template <class SRC, int KG>
__global__ __launch_bounds__(KG * 256, 4 / KG) void k_gram(const SRC chain_src, int s, int nchains)
{
    const int gid = blockIdx.x, gx = gid & 7, gr = gid >> 3;
    const int gchain = gr % nchains, gslot = (gr / nchains) * 8 + gx;      // gslot: position in the one-chain task map
    const bnr_dev &cd = chain_src.at(gchain);
    __shared__ double sred[KG * BNR_GT * BNR_GT];     // staging buffers during the loop, then the K-group reduction
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    const double *Sp = cd.trace + (size_t)P.prev * cd.rowlen + cd.o_S;
    // the task map's extent is padded to a multiple of 8 so that id % 8 labels the XCD
    if (gslot >= cd.ksplit * (cd.ntile * (cd.ntile + 1) / 2)) return;
    const int task = cd.gmap[gslot];
    int t = task & 0xFFFF, ti = 0;
    const int ks = task >> 16;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    int tj = t - ti * (ti + 1) / 2;
    BNR_TL_IN(cd, TL_GRAM, gslot == 0);
    bnr_gram16_task<KG>(bnr_geom_of(cd), Sp, cd.Gpart, t, ti, tj, ks, sred);
    bnr_gram_count(cd, tj);
    BNR_TL_OUT(cd, TL_GRAM);
}

// k_gram8: the same Gram, the same task map, the same summation order per element (bitwise the same partial tiles) -- for SIX
// wavefronts per SIMD.  What the extra waves buy is cover for the loop's staging and VALU work and for its barrier per batch (every VALU
// instruction issued between f64 MFMAs takes 6-14 cycles from the matrix pipe, tools/mfma_f64_mix.hip; the pipe itself issues at the spec
// rate of 64 cycles per MFMA from ONE wave -- the round-1 "issue rate grows with the waves per SIMD" was a microbenchmark artefact,
// profiles/round5_mfma_f64_peak.txt).  Three 512-thread workgroups per CU = 6 waves per SIMD: __launch_bounds__(512, 6) -- the second
// argument is the minimum number of WAVES PER SIMD, not of blocks per CU -- caps the kernel at 80 VGPRs (78 used, no spills), and
// batches of 8 columns keep a workgroup at 32 KiB of LDS (half the staging registers and half the image of k_gram's 16:
// 2 K-groups x 2 buffers x [I | J] x 8 x 64 doubles; a barrier per 8 MFMAs of a wave), with a K-group reduction that needs one tile
// of LDS instead of two (K-group 1 parks its tile, K-group 0 adds its registers and stores).  Eight waves per SIMD (64 VGPRs through
// buffer descriptors) brought nothing more (profiles/round2_experiments_notes.txt D).
// one (tile t = (ti, tj), K slice ks) task of the Gram with 8-column batches: 512 threads, sred = 32 KiB of LDS.
// clk: where the stamps build records both clocks around the K loop (nullptr: nowhere)
__device__ __forceinline__ void bnr_gram8_task(const bnr_gram_geom &cd, const double *Sp, double *Gpart, int t, int ti, int tj, int ks, double *sred, unsigned long long *clk = nullptr)
{
    constexpr int KG = 2, KB = 8;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int kg = wave >> 2, wi = (wave >> 1) & 1, wj = wave & 1;
    const int kchunk = cd.q_pad / cd.ksplit;          // multiple of 8 KG (host guarantees)
    const int ksub = kchunk / KG;                     // multiple of 8
    const int eb = ks * kchunk + kg * ksub;
    const int nbatch = ksub / KB;
    const size_t ld = cd.n_pad;
    const int li = lane & 15, lk = lane >> 4;
    // staging: this thread moves rows (2 rp, 2 rp + 1) of column c of both panels
    const int tg = tid & 255, c = tg >> 5, rp = tg & 31;
    // per-lane offsets inside a batch are small (8 columns): 32-bit, so that the loads use the scalar-base + 32-bit-offset form
    // (in BYTES: scalar base + zero-extended 32-bit lane offset is the addressing form of global_load with an SGPR base)
    const unsigned offI = 8u * ((unsigned)(ti * BNR_GT + 2 * rp) + (unsigned)c * (unsigned)ld), offJ = 8u * ((unsigned)(tj * BNR_GT + 2 * rp) + (unsigned)c * (unsigned)ld);
    const unsigned offS = 8u * (unsigned)c;
    // wave-uniform bases pinned to scalar registers: the loads below are "scalar base + constant 32-bit lane offset" and the loop carries no
    // address VALU at all (round 5, tools/mfma_f64_mix.hip: every VALU instruction issued between f64 MFMAs takes 6-14 cycles from the
    // matrix pipe, LDS / VMEM / SALU instructions and barriers take none; the loop used to carry 15 VALU instructions per 8 MFMAs)
    const double *xb = bnr_sgpr_global(cd.X + (size_t)eb * ld);
    const double *sb = bnr_sgpr_global(Sp + eb);       // S is followed by q_pad - q + BNR_GRAM_PREFETCH_COLS zeros in every trace row (bnr_chain_create): no clamp; X is zero there
    constexpr int PANEL = KB * BNR_GT;                 // doubles per panel (8 columns x 64 rows)
    // LDS image of a K-group: [buf][I|J][col][row ^ swizzle].  A lane's five positions in it (its staging slot, and rows ra0, ra1 of J and rb0, rb1 of I
    // in column lk) are formed once, as LDS pointers, and made opaque: every LDS address of the loops is then one of these five registers + an
    // immediate, in the trips and in the odd batch behind them alike (left to itself the compiler forms the addresses of the odd batch again from
    // the row numbers, which then stay live across the loop -- three registers more than the 80 there are)
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) bnr_d2 lds_d2;
    const int sw = (lk & 1) << 4;
    lds_f64 *const stg = (lds_f64 *)sred + kg * (4 * PANEL);
    lds_f64 *pw = stg + c * BNR_GT + ((2 * rp) ^ ((c & 1) << 4));
    lds_f64 *pa0 = stg + PANEL + lk * BNR_GT + ((wj * 32 + li) ^ sw), *pa1 = stg + PANEL + lk * BNR_GT + ((wj * 32 + 16 + li) ^ sw);
    lds_f64 *pb0 = stg + lk * BNR_GT + ((wi * 32 + li) ^ sw), *pb1 = stg + lk * BNR_GT + ((wi * 32 + 16 + li) ^ sw);
    asm volatile("" : "+v"(pw), "+v"(pa0), "+v"(pa1), "+v"(pb0), "+v"(pb1));
    bnr_d4 c00 = {0, 0, 0, 0}, c01 = {0, 0, 0, 0}, c10 = {0, 0, 0, 0}, c11 = {0, 0, 0, 0};   // c[jt][it]
    // two staging register sets, the set of a batch = its parity: batch b + 2 is loaded at the TOP of batch b into the set that batch b's own
    // columns left in the middle of batch b - 1, and goes to LDS between the two k-steps of batch b + 1.  A load therefore leads the store that
    // consumes it by a batch and a half (12 MFMAs of a wave, 9 on a diagonal block), and the wait in front of the store is for batch b + 2 only,
    // with batch b + 3 still in flight: never a wait for everything.  (With one set -- first k-step, store, load, second k-step -- the compiler
    // gave the second half of its two-batch trip registers of the MFMA operands, sank those loads behind the half's last MFMA and opened the
    // next trip with s_waitcnt vmcnt(0) right behind the barrier: tools/gram_loop_sched.py, profiles/gram_prefetch_distance.txt.)
    bnr_d2 ri0, rj0, ri1, rj1;
    double sv0, sv1;
    const __amdgpu_buffer_rsrc_t rX = bnr_rsrc(xb), rS = bnr_rsrc(sb);
    const int bstep = KB * (int)ld * 8;                // bytes per batch (scalar)
#define BNR_G8_LOAD(SET, BIDX)                                                               \
    do {                                                                                      \
        sv##SET = bnr_bufload_f64(rS, offS, (BIDX) * (KB * 8));                               \
        ri##SET = bnr_bufload_d2(rX, offI, (BIDX) * bstep);                                   \
        rj##SET = bnr_bufload_d2(rX, offJ, (BIDX) * bstep);                                   \
    } while (0)
#define BNR_G8_STORE(SET, BUF)                                                                \
    do {                                                                                      \
        *(lds_d2 *)(pw + (BUF) * (2 * PANEL)) = ri##SET * sv##SET;                            \
        *(lds_d2 *)(pw + (BUF) * (2 * PANEL) + PANEL) = rj##SET;                              \
    } while (0)
    // the fragments of both k-steps of a batch (the two columns of a lane, lk and lk + 4, come with one ds_read2st64_b64 per fragment row)
#define BNR_G8_READ(BUF)                                                                      \
    constexpr int o0_ = (BUF) * (2 * PANEL), o1_ = o0_ + 4 * BNR_GT;                          \
    const double a00 = pa0[o0_], a01 = pa0[o1_], a10 = pa1[o0_], a11 = pa1[o1_];              \
    const double b00 = pb0[o0_], b01 = pb0[o1_], b10 = pb1[o0_], b11 = pb1[o1_]
#define BNR_G8_MFMA(K2, DIAG)                                                                 \
    do {                                                                                      \
        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0##K2, b0##K2, c00, 0, 0, 0);             \
        c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0##K2, b1##K2, c01, 0, 0, 0);             \
        if (!(DIAG)) c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1##K2, b0##K2, c10, 0, 0, 0); \
        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1##K2, b1##K2, c11, 0, 0, 0);             \
    } while (0)
    // batches past the end of the slice read the following columns or the zero-padded tail of X (q_pad + BNR_GRAM_PREFETCH_COLS columns are
    // allocated); they are stored but never used by a compute step
    BNR_G8_LOAD(0, 0);
    BNR_G8_STORE(0, 0);
    BNR_G8_LOAD(1, 1);
    __syncthreads();
#ifdef BNR_STAMPS
    // both clocks around the K loop: shader cycles / 100 MHz ticks = the clock the PRODUCT kernel's loop runs at (tools/stamps_gram_clock.py)
    if (clk && tid == 0) { clk[0] = __builtin_amdgcn_s_memtime(); clk[1] = __builtin_amdgcn_s_memrealtime(); }
#endif
    // batch B of parity PAR: the loads of batch B + 2, the first k-step, the staging of batch B + 1 (its buffer was released by the last barrier),
    // the second k-step.  Two batches per trip with the parity a literal: every LDS address is "lane base + immediate", the register sets have
    // names.  The scheduling barriers keep the compiler from moving the loads down or the stores to a barrier's side (nothing crosses them).
#define BNR_G8_BATCH_L(B, PAR, NPAR, DIAG)                                                    \
    do {                                                                                      \
        BNR_G8_LOAD(PAR, (B) + 2);                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        BNR_G8_READ(PAR);                                                                     \
        BNR_G8_MFMA(0, DIAG);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        BNR_G8_STORE(NPAR, NPAR);                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        BNR_G8_MFMA(1, DIAG);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        __syncthreads();                                                                      \
    } while (0)
#define BNR_G8_BATCH_DEAD(B, PAR, NPAR)                                                       \
    do {                                                                                      \
        BNR_G8_LOAD(PAR, (B) + 2);                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        BNR_G8_STORE(NPAR, NPAR);                                                             \
        __syncthreads();                                                                      \
    } while (0)
    if (ti == tj && wi == 0 && wj == 1) {
        // dead block of a diagonal tile (see bnr_gram16_task): staging and barriers only, zeros out
        int b = 0;
        for (; b + 1 < nbatch; b += 2) { BNR_G8_BATCH_DEAD(b, 0, 1); BNR_G8_BATCH_DEAD(b + 1, 1, 0); }
        if (b < nbatch) BNR_G8_BATCH_DEAD(b, 0, 1);
    } else if (ti == tj && wi == wj) {
        // a diagonal 32 x 32 block: three MFMAs per k-step (see bnr_gram16_task)
        int b = 0;
        for (; b + 1 < nbatch; b += 2) { BNR_G8_BATCH_L(b, 0, 1, true); BNR_G8_BATCH_L(b + 1, 1, 0, true); }
        if (b < nbatch) BNR_G8_BATCH_L(b, 0, 1, true);
    } else {
        int b = 0;
        for (; b + 1 < nbatch; b += 2) { BNR_G8_BATCH_L(b, 0, 1, false); BNR_G8_BATCH_L(b + 1, 1, 0, false); }
        if (b < nbatch) BNR_G8_BATCH_L(b, 0, 1, false);
    }
#ifdef BNR_STAMPS
    if (clk && tid == 0) { clk[2] = __builtin_amdgcn_s_memtime(); clk[3] = __builtin_amdgcn_s_memrealtime(); }
#endif
    // tile element (i,j) lives at [j*64 + i]; this lane: j = wj*32 + jt*16 + (lane>>4) + 4 r, i = wi*32 + it*16 + (lane&15)
    // (formed from an opaque copy of the thread index: nothing of the epilogue's addressing is kept in registers across the loops)
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));
    const int jb = ((tid_e >> 6) & 1) * 32 + ((tid_e & 63) >> 4), ib = ((tid_e >> 7) & 1) * 32 + (tid_e & 15);
    if (kg == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sred[(jb + 4 * r) * BNR_GT + ib] = c00[r];
            sred[(jb + 4 * r) * BNR_GT + ib + 16] = c01[r];
            sred[(jb + 16 + 4 * r) * BNR_GT + ib] = c10[r];
            sred[(jb + 16 + 4 * r) * BNR_GT + ib + 16] = c11[r];
        }
    }
    __syncthreads();
    if (kg == 0) {
        double *out = Gpart + ((size_t)ks * (cd.ntile * (cd.ntile + 1) / 2) + t) * (BNR_GT * BNR_GT);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bnr_gstore(out + (jb + 4 * r) * BNR_GT + ib, c00[r] + sred[(jb + 4 * r) * BNR_GT + ib]);
            bnr_gstore(out + (jb + 4 * r) * BNR_GT + ib + 16, c01[r] + sred[(jb + 4 * r) * BNR_GT + ib + 16]);
            bnr_gstore(out + (jb + 16 + 4 * r) * BNR_GT + ib, c10[r] + sred[(jb + 16 + 4 * r) * BNR_GT + ib]);
            bnr_gstore(out + (jb + 16 + 4 * r) * BNR_GT + ib + 16, c11[r] + sred[(jb + 16 + 4 * r) * BNR_GT + ib + 16]);
        }
    }
}
template <class SRC>
__global__ __launch_bounds__(512, 6) void k_gram8(const SRC chain_src, int s, int nchains)
{
    const int gid = blockIdx.x, gx = gid & 7, gr = gid >> 3;
    const int gchain = gr % nchains, gslot = (gr / nchains) * 8 + gx;
    const bnr_dev &cd = chain_src.at(gchain);
    __shared__ double sred[BNR_GT * BNR_GT];          // 32 KiB: staging buffers during the loop, then K-group 1's tile
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    const double *Sp = cd.trace + (size_t)P.prev * cd.rowlen + cd.o_S;
    if (gslot >= cd.ksplit * (cd.ntile * (cd.ntile + 1) / 2)) return;
    const int task = cd.gmap[gslot];
    int t = task & 0xFFFF, ti = 0;
    const int ks = task >> 16;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    int tj = t - ti * (ti + 1) / 2;
    BNR_TL_IN(cd, TL_GRAM, gslot == 0);
#ifdef BNR_STAMPS
    bnr_gram8_task(bnr_geom_of(cd), Sp, cd.Gpart, t, ti, tj, ks, sred, gslot < 256 ? cd.dbg + 2048 + 4 * gslot : nullptr);
#else
    bnr_gram8_task(bnr_geom_of(cd), Sp, cd.Gpart, t, ti, tj, ks, sred);
#endif
    bnr_gram_count(cd, tj);
    BNR_TL_OUT(cd, TL_GRAM);
}

// ===================================================================================== the Gram of a BINARY model matrix on the i8 matrix pipe
// (reference: docs/src/man/inputdata.md:5-10 -- the inputs are 0/1 adjacency data --, X_new = Matrix{eltype(T)} gibbs.jl:917, the
// product Xtau tau2 D Xtau' of gibbs.jl:434.)  With x in {0, 1}:  G[i][j] = sum_k x_ik x_jk S_k.
//   k_sdigits   S_k = sum_{l < L} d_l[k] 256^(L - 1 - l) 2^(e - 8 L + 2) + r_k,  d_l in -128..127 (balanced base-256 digits),  2^e > max S,
//               0 <= r_k < 2^(e - 8 L + 2)   (an (8 L - 2)-bit fixed point image of S under the exponent of its largest entry: entries far below the largest lose
//               relative precision, G does not -- see the bound)
//   k_gram_i8   T_l = X diag(d_l) X' EXACTLY in i32 (v_mfma_i32_16x16x64_i8; A = the byte mask of the j rows = -x, B = mask AND digits = x d of the
//               i rows; |T_l| <= 128 kchunk), then G = - sum_l T_l 256^(L - 1 - l) 2^(e - 8 L + 2) by Horner in f64 (L roundings of relative size 2^-53).
// Error against the exact Gram (S rounded to nearest since round 6): |G_exact - G| <= q 2^(e - 8 L + 1) <= 4 q 2^(-8 L) max_k S_k, and max |G| >= max_k S_k as soon as the column of the largest S
// has a one: relative to max |G| at most 8 q 2^(-8 L) -- L = 7 up to q = 9007 (5.6e-13 at q = 5050), L = 8 beyond (2e-14 at q = 45150): below 1e-12, the size of
// the f64 path's own rounding.  Same tasks, K slices and partial-tile layout as k_gram8: the reduction in launch 0 of the factorization does not know the difference.
// The loop (tools/gram_i8_lab.hip, profiles/round5_gram_i8.txt): X tiles staged through LDS in full 128-byte lines (direct 16-byte fragment loads were bound by
// the CU's vector-memory path: every tile row fetched by two waves, half a line at a time), a wave = 16 i rows x all 64 j rows (ONE masked B fragment per plane for
// four MFMAs); what bounds it now is LDS bandwidth (per k-step and wave five 1 KiB fragment reads + L digit reads for 4 L MFMAs of 16 cycles).
// Measured: 8 chains at n = 500, V = 100: 50 us per launch + 6 us for the digits against 190 us on the f64 pipe.
__global__ void k_x_mask(const unsigned char *X8, int n, int n_pad, int q, int kchunk, int kcp, int kslab, unsigned char *XM, int *not_binary)
{
    // one thread per (row, 16-byte group) of XM; X8 is column-major (leading dimension n_pad): a one-off transpose at chain creation
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ng = kslab / 16;
    if (idx >= (size_t)n_pad * ng) return;
    const int i = (int)(idx / ng), g = (int)(idx % ng);
    const int ks = (16 * g) / kcp, kk0 = (16 * g) % kcp;
    bnr_i4 out = {0, 0, 0, 0};
    bool bad = false;
    for (int b = 0; b < 16; ++b) {
        const int kk = kk0 + b, k = ks * kchunk + kk;
        unsigned v = 0;
        if (i < n && kk < kchunk && k < q) v = X8[(size_t)i + (size_t)n_pad * k];
        if (v > 1u) bad = true;
        if (v) out[b >> 2] |= 0xFF << (8 * (b & 3));
    }
    *(bnr_i4 *)(XM + (size_t)i * kslab + 16 * (size_t)g) = out;
    if (bad) *not_binary = 1;
}
// one (tile, K slice) task per 256-thread workgroup; dynamic LDS = 2 buffers x [I tile | J tile] x 64 rows x 144 bytes + L x kcp bytes of digits
#define BNR_I8_RS 144                                         // bytes per staged row: 128 (two k-steps) + 16 of padding -- conflict-free ds_read_b128 fragments
#define BNR_I8_TB (64 * BNR_I8_RS)
__host__ __device__ inline size_t bnr_i8_lds_bytes(int L, int kcp) { return (size_t)4 * BNR_I8_TB + (size_t)L * kcp; }
// lane BASE + L of every row of 16 lanes to the whole row (DPP row_newbcast: gfx90a and later); L is a loop constant after unrolling
template <int BASE>
__device__ __forceinline__ int bnr_row_bcast(int v, const int l)
{
    switch (BASE + l) {
    case 0: return __builtin_amdgcn_update_dpp(0, v, 0x150, 0xF, 0xF, false);
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x151, 0xF, 0xF, false);
    case 2: return __builtin_amdgcn_update_dpp(0, v, 0x152, 0xF, 0xF, false);
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x153, 0xF, 0xF, false);
    case 4: return __builtin_amdgcn_update_dpp(0, v, 0x154, 0xF, 0xF, false);
    case 5: return __builtin_amdgcn_update_dpp(0, v, 0x155, 0xF, 0xF, false);
    case 6: return __builtin_amdgcn_update_dpp(0, v, 0x156, 0xF, 0xF, false);
    case 7: return __builtin_amdgcn_update_dpp(0, v, 0x157, 0xF, 0xF, false);
    case 8: return __builtin_amdgcn_update_dpp(0, v, 0x158, 0xF, 0xF, false);
    case 9: return __builtin_amdgcn_update_dpp(0, v, 0x159, 0xF, 0xF, false);
    case 10: return __builtin_amdgcn_update_dpp(0, v, 0x15A, 0xF, 0xF, false);
    case 11: return __builtin_amdgcn_update_dpp(0, v, 0x15B, 0xF, 0xF, false);
    case 12: return __builtin_amdgcn_update_dpp(0, v, 0x15C, 0xF, 0xF, false);
    case 13: return __builtin_amdgcn_update_dpp(0, v, 0x15D, 0xF, 0xF, false);
    case 14: return __builtin_amdgcn_update_dpp(0, v, 0x15E, 0xF, 0xF, false);
    default: return __builtin_amdgcn_update_dpp(0, v, 0x15F, 0xF, 0xF, false);
    }
}
template <class SRC, int L>
__global__ __launch_bounds__(256, 2) void k_gram_i8(const SRC chain_src, int s, int nchains)
{
    const int gid = blockIdx.x, gx = gid & 7, gr = gid >> 3;
    const int gchain = gr % nchains, gslot = (gr / nchains) * 8 + gx;      // the task map of k_gram / k_gram8 (XCD-aware, chains of a group innermost)
    const bnr_dev &cd = chain_src.at(gchain);
    const int ntl = cd.ntile * (cd.ntile + 1) / 2;
    if (gslot >= cd.ksplit * ntl) return;
    const int task = cd.gmap[gslot];
    int t = task & 0xFFFF, ti = 0;
    const int ks = task >> 16;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    extern __shared__ bnr_i4 smem_i8[];
    unsigned char *sX = (unsigned char *)smem_i8;             // [buf][I | J][64 rows][144]
    bnr_i4 *sDig = (bnr_i4 *)(sX + 4 * BNR_I8_TB);            // [l][kcp / 16]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ln = lane & 15, lq = lane >> 4;
    const int ng = cd.kcp / 16;
    for (int idx = tid; idx < L * ng; idx += 256) {
        const int l = idx / ng, g = idx % ng;
        sDig[idx] = *(const bnr_i4 *)(cd.Sdig + (size_t)l * cd.kslab + (size_t)ks * cd.kcp + 16 * g);
    }
    // staging: thread -> rows tid / 8 and tid / 8 + 32 of both tiles, 16-byte column tid % 8 of the 128-byte batch (eight lanes = one full line of a row)
    const int srow = tid >> 3, scol = tid & 7;
    const unsigned char *gI = cd.XM + (size_t)(ti * BNR_GT + srow) * cd.kslab + (size_t)ks * cd.kcp + 16 * scol;
    const unsigned char *gJ = cd.XM + (size_t)(tj * BNR_GT + srow) * cd.kslab + (size_t)ks * cd.kcp + 16 * scol;
    const size_t r32 = (size_t)32 * cd.kslab;
    const int soff = srow * BNR_I8_RS + 16 * scol;
    bnr_i4 r0 = {0, 0, 0, 0}, r1 = r0, r2 = r0, r3 = r0;
    const int nbatch = cd.kcp / 128, nb = nbatch + ((cd.kcp % 128) ? 1 : 0);       // kcp is a multiple of 64: a last HALF batch is possible
    auto load = [&](int b) {
        const int o = 128 * b;
        if (b < nbatch || scol < 4) { r0 = *(const bnr_i4 *)(gI + o); r1 = *(const bnr_i4 *)(gI + r32 + o); r2 = *(const bnr_i4 *)(gJ + o); r3 = *(const bnr_i4 *)(gJ + r32 + o); }
    };
    auto store = [&](int buf) {
        unsigned char *d = sX + buf * 2 * BNR_I8_TB + soff;
        *(bnr_i4 *)d = r0; *(bnr_i4 *)(d + 32 * BNR_I8_RS) = r1; *(bnr_i4 *)(d + BNR_I8_TB) = r2; *(bnr_i4 *)(d + BNR_I8_TB + 32 * BNR_I8_RS) = r3;
    };
    // wave w: the 16 i rows 16 w .. 16 w + 15 (ONE masked B fragment per digit plane) x all 64 j rows (four A fragments, the raw mask = -x)
    bnr_i4 acc[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[l][a] = bnr_i4{0, 0, 0, 0};
    load(0); store(0);
    if (nb > 1) load(1);
    __syncthreads();
    const int fa = ln * BNR_I8_RS + 16 * lq + BNR_I8_TB, fb = (wave * 16 + ln) * BNR_I8_RS + 16 * lq;
    for (int b = 0; b < nb; ++b) {
        const unsigned char *xb = sX + (b & 1) * 2 * BNR_I8_TB;
        const int nk = (b < nbatch) ? 2 : 1;
        // ALL digits of the batch in ONE LDS read: lane (row lq, position p = l + 8 kk) fetches the 16 bytes of plane l, k-step kk for its row -- 7 or 8 planes x 2 k-steps x
        // 4 rows = the 64 lanes.  (Round 5 read them plane by plane and k-step by k-step with all 64 lanes: L reads per k-step of 1 KiB each for 4 x 16 distinct bytes, which
        // is what bound the kernel -- VERDICT r5 next 4; a read by four lanes only still costs the LDS pipe a whole pass.)
        bnr_i4 dgall;
        {
            const int pl = ln & 7, pk = ln >> 3, lcl = pl < L ? pl : L - 1;
            int gi = (2 * b + pk) * 4 + lq;
            gi = gi < ng ? gi : ng - 1;
            dgall = sDig[lcl * ng + gi];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (kk >= nk) break;
            const bnr_i4 a0 = *(const bnr_i4 *)(xb + fa + 64 * kk), a1 = *(const bnr_i4 *)(xb + fa + 16 * BNR_I8_RS + 64 * kk);
            const bnr_i4 a2 = *(const bnr_i4 *)(xb + fa + 32 * BNR_I8_RS + 64 * kk), a3 = *(const bnr_i4 *)(xb + fa + 48 * BNR_I8_RS + 64 * kk);
            const bnr_i4 b0 = *(const bnr_i4 *)(xb + fb + 64 * kk);
#pragma unroll
            for (int l = 0; l < L; ++l) {
                // the digits of plane l and this k-step for row lq of 16 lanes sit in lane l + 8 kk of that row (dgall, read once per batch below): a DPP row broadcast
                // inside the masking AND hands them to the row -- v_and_b32 row_newbcast, the same vector instruction count as a plain AND
                bnr_i4 m0;
                if (kk == 0) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) m0[d] = b0[d] & bnr_row_bcast<0>(dgall[d], l);
                } else {
#pragma unroll
                    for (int d = 0; d < 4; ++d) m0[d] = b0[d] & bnr_row_bcast<8>(dgall[d], l);
                }
                acc[l][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, m0, acc[l][0], 0, 0, 0);
                acc[l][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, m0, acc[l][1], 0, 0, 0);
                acc[l][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, m0, acc[l][2], 0, 0, 0);
                acc[l][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a3, m0, acc[l][3], 0, 0, 0);
            }
            if (kk == 0 && b + 1 < nb) { store((b + 1) & 1); if (b + 2 < nb) load(b + 2); }   // batch b+1 into the buffer the last barrier released, batch b+2 into the registers
        }
        __syncthreads();
    }
    // acc[l][jt][r]: j = jt 16 + 4 lq + r, i = 16 wave + ln, holding -T_l (the A operand was -x); tile element (i, j) at [j 64 + i]
    const double sc = -cd.scal[SC_I8SCALE];
    double *out = cd.Gpart + ((size_t)ks * ntl + t) * (BNR_GT * BNR_GT);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = (double)acc[0][jt][r];
#pragma unroll
            for (int l = 1; l < L; ++l) v = v * 256.0 + (double)acc[l][jt][r];
            bnr_gstore(out + (jt * 16 + 4 * lq + r) * BNR_GT + wave * 16 + ln, v * sc);
        }
}

// E = extended matrix of the factorization, (2 n_pad + 32) x n_pad, column-major, leading dimension ldE:
//     rows [0, n_pad)            G + I  (lower triangle)                      -> L
//     rows [n_pad, 2 n_pad)      Y = I                                        -> L^-T   (back substitution becomes a GEMV)
//     rows [2 n_pad, 2 n_pad+32) unused padding
// k_gram_reduce: G = sum_ks partial + I into the lower tiles of E, and Y = I.  grid = (lower tiles, 4), 256 threads.
__host__ __device__ inline int bnr_ldE(int n_pad) { return 2 * n_pad + BNR_NB; }

// Kernels of the sweep's critical chain (reduction, panel steps, solve, back-projection) raise the issue priority of every wave with their
// first instruction: the scalar branch of the sweep runs beside them on another queue, and a young wave that lands on a SIMD where older
// waves of k_tail / k_node keep the VALU busy is otherwise served last (tools/interfere_probe.hip: a chain of 16 dependent 5 us launches
// takes 8.3 instead of 6.6 us per link beside eight 1024-thread VALU-bound workgroups, 13.9 instead of 7.7 with 1096 workgroups per link;
// with s_setprio 3 it is 6.6 / 7.9 again, and beside a streaming kernel 13 instead of 21 us).
#define BNR_CRITICAL_PATH() __builtin_amdgcn_s_setprio(3)
template <class SRC>
__global__ __launch_bounds__(256) void k_gram_reduce(const SRC chain_src, int s)
{
    BNR_CRITICAL_PATH();
    const bnr_dev &cd = chain_src.get();
    // grid = (lower tiles, 8): each workgroup sums 512 elements (one 16-byte pair per thread) of one tile over the K slices
    int t = blockIdx.x, ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    int tj = t - ti * (ti + 1) / 2;
    const int ntl = cd.ntile * (cd.ntile + 1) / 2;
    const size_t ld = bnr_ldE(cd.n_pad), tsz = BNR_GT * BNR_GT;
    const int idx = blockIdx.y * 512 + 2 * threadIdx.x;            // even: (idx, idx+1) are two consecutive rows i
    const double *src = cd.Gpart + (size_t)t * tsz + idx;
    bnr_d2 acc = {0.0, 0.0};
    int ks = 0;
    for (; ks + 3 < cd.ksplit; ks += 4) {
        bnr_d2 v0 = *(const bnr_d2 *)(src + (size_t)ks * ntl * tsz), v1 = *(const bnr_d2 *)(src + (size_t)(ks + 1) * ntl * tsz);
        bnr_d2 v2 = *(const bnr_d2 *)(src + (size_t)(ks + 2) * ntl * tsz), v3 = *(const bnr_d2 *)(src + (size_t)(ks + 3) * ntl * tsz);
        acc += v0; acc += v1; acc += v2; acc += v3;
    }
    for (; ks < cd.ksplit; ++ks) acc += *(const bnr_d2 *)(src + (size_t)ks * ntl * tsz);
    const int i = ti * BNR_GT + idx % BNR_GT, j = tj * BNR_GT + idx / BNR_GT;
    if (i == j) acc[0] += 1.0;
    if (i + 1 == j) acc[1] += 1.0;
    bnr_st16<BNR_ST_LAUNCH0>(cd.E + (size_t)i + ld * j, acc);
    // Y = I (all n_pad x n_pad entries), spread over the whole grid, 16 bytes per store
    const int nwg = gridDim.x * gridDim.y, wg = blockIdx.x * gridDim.y + blockIdx.y, np = cd.n_pad;
    for (size_t e = ((size_t)wg * 256 + threadIdx.x) * 2; e < (size_t)np * np; e += (size_t)nwg * 512) {
        int r = (int)(e % np), c = (int)(e / np);
        if (r / BNR_NB > c / BNR_NB) continue;             // below the diagonal block Y = L^-T is never written and never read (k_solve_w, k_solve_a4)
        bnr_d2 v = {(r == c) ? 1.0 : 0.0, (r + 1 == c) ? 1.0 : 0.0};
        bnr_st16<BNR_ST_LAUNCH0>(cd.E + (size_t)(np + r) + ld * c, v);
    }
    if (threadIdx.x == 0) cd.stamp[blockIdx.x * 8 + blockIdx.y] = cd.plan[cd.pbase[0] + s].it;
    if (blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x <= cd.ntile) cd.gprog[threadIdx.x] = 0u;   // all of G has been consumed
}

// ===================================================================================== blocked Cholesky + solve
// (G + I) a4 = b,  b = a1 - a3  (gibbs.jl:434; the reference's generic `\` is an LU solve of this SPD system).
// Right-looking blocked Cholesky of E, NB = 32, ONE launch per panel with lookahead 1 (k_chol_step(p), p = 0..nbk-1).
// Every block row of E (matrix rows, identity rows, the b block) runs the same code:
//   role A (nbk + 1 panel workgroups): apply panel p-1's update to the blocks (p,p) and (rho,p) by f64 MFMA -- the two blocks of
//       panel p-1 it needs are fetched once per workgroup, cooperatively, into LDS and the fragments come from there --, then the
//       workgroup's FOUR waves sweep the 64 x 32 register-resident panel [E_pp ; E_rho,p] as a pipeline, eight columns each
//       (bnr_panel_sweep_pipe): a wave first applies the columns that the waves in front publish in LDS, its multipliers
//       taken by DPP row broadcast out of one LDS read per column, then walks its own eight pivots (bnr_sweepN: pivot chain on
//       scalars, rsqrt = v_rsq_f64 + one third-order step, rank-1 updates by v_readlane broadcasts) and publishes each column.
//       Lanes 0-31 redo the diagonal block in every workgroup: no cross-workgroup hand-off inside a launch.
//   role B (update workgroups): E[rho,j] -= L[rho,p-1] L[j,p-1]' for every block column j >= p+1, by f64 MFMA.
// k_chol_step2 (two panels per launch, large n) keeps the sweep of ONE wave per panel, 16 columns at a time (bnr_sweep16 = bnr_sweepN<16>).
// k_solve_gemv: a4 = Y w, then the n-vector bookkeeping for X gamma_new.
__device__ __forceinline__ double bnr_readlane(double v, int srclane)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, srclane);
    hi = __builtin_amdgcn_readlane(hi, srclane);
    return __hiloint2double(hi, lo);
}
#define BNR_LP (BNR_NB + 1)
__host__ __device__ inline int bnr_chol_npanel(int nbk, int p) { (void)p; return nbk + 1; }
__host__ __device__ inline int bnr_chol_ntile(int nbk, int p)
{
    if (p == 0) return 0;
    int m = nbk - (p + 1);
    return m * (m + 1) / 2 + m * p;              // matrix tiles + p identity block rows per column
}
__host__ __device__ inline int bnr_chol_nsuper(int nbk, int p)   // 64 x 64 super blocks of the same trailing update
{
    if (p == 0) return 0;
    int ms = (nbk - (p + 1) + 1) / 2;
    return ms * (ms + 1) / 2 + ms * ((p + 1) / 2);
}

// 16x16 tile of  C - A B'  over K = 32:  C[m][n], m <-> column, n <-> row (n = lane & 15 is contiguous in memory).
//   colrows: &E[first column-side row, kc]   (the rows of L[j-block, p-1] that give the tile's 16 columns)
//   rowrows: &E[first row-side row, kc]      (the rows of L[rho-block, p-1] that give the tile's 16 rows)
__device__ __forceinline__ bnr_d4 bnr_tile_update(const double *colrows, const double *rowrows, size_t ld, int lane, bnr_d4 c)
{
    const int ln = lane & 15, lk = lane >> 4;
    double av[8], bv[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        av[ks] = colrows[(size_t)ln + ld * (size_t)(4 * ks + lk)];
        bv[ks] = rowrows[(size_t)ln + ld * (size_t)(4 * ks + lk)];
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[ks], bv[ks], c, 0, 0, 0);
    return c;
}

#define BNR_L1S 80            // LDS column stride of the 64 x 16 half-panel handed to the MFMA update of k_chol_step2 (conflict-free fragments)
// ----------------------------------------------------------------------------------------- round 6: the panel sweep as a pipeline of the four waves
// One wave walking all 32 pivots with all the rank-1 updates of the columns to their right (rounds 1-5) left three of the workgroup's four SIMDs idle: 45 instructions
// per pivot at one issue per 4 cycles, 2 x 3 000 cycles, + 1 200 for an MFMA update between the two 16-column halves.  Here every wave owns
// EIGHT of the 32 columns (lane = row: lanes 0..31 the diagonal block, 32..63 the own block) and the waves form a pipeline over the columns:
//   wave w first applies the finished columns 0 .. 8w-1 to its own eight as they show up in LDS (sL: one 64-row column per pivot, published by the wave that owns
//   it the moment it is scaled), two columns per trip, the next trip's four LDS reads in flight; then it walks its own eight pivots (bnr_sweepN<8>: the pivot chain on
//   wave-uniform scalars, the rank-1 updates reach at most seven columns to the right) and publishes each column.
// The pivot chain runs through the four waves in turn; what a wave's predecessors publish while they are the chain is applied by the waves behind, off the chain.
// Nothing is ordered by barriers: a column that is not there yet shows as a NaN with a payload no arithmetic produces (sL is filled with it before the panel is
// staged), every lane checks its own row and a wave vote says "all 64 rows there" -- which is the whole column, multipliers included.  The polls are bounded: a
// column that never shows up (it cannot, short of a fault) ends the wait after BNR_PIPE_SPINS polls and reports the panel as failed.
// Per element the updates arrive in column order except for the swap inside bnr_sweepN (k-2 before k-3): deterministic, independent of timing; NOT the summation
// order of the one-wave sweep's MFMA mid update, so the factor differs from the round-5 build's in the last bits (the parity bar is rtol 1e-6 against the CPU restatement of the reference, tests/).
#define BNR_PIPE_SPINS (1 << 16)
#define BNR_PIPE_SENT_HI 0x7FF8DEAD
__device__ __forceinline__ double bnr_canon_nan(double v) { return v == v ? v : __hiloint2double(0x7FF80000, 0); }
struct alignas(16) bnr_panelp_lds {
    double sD[BNR_NB * BNR_LP], sB[BNR_NB * BNR_LP];
    double sL[BNR_NB][64];
};
__device__ __forceinline__ unsigned bnr_lds_addr(const void *p) { return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void *)p; }
// Register-resident sweep of N panel columns, lane = row (64 rows): column j's pivot sits in lane COFF + j.  The next two columns are updated at once through
// v_readlane broadcasts, the remaining ones one step later, their multipliers taken from the previous column's register by v_readlane as well (no LDS round trip
// per pivot).  PUB: 0 nothing, 2 every finished column goes to pub_addr + 512 j bytes (LDS, lane = row)
struct bnr_no_hook { __device__ __forceinline__ void operator()() const {} };
// (hook: called once, behind the issue of the first pivot's v_rsq_f64 -- multiply-adds of the wave's columns 2 .. N - 1 that are still pending run in that shadow)
template <int N, int COFF, int PUB, class HOOK = bnr_no_hook>
__device__ __forceinline__ int bnr_sweepN(double (&a)[N], int lane, unsigned pub_addr, HOOK hook = HOOK())
{
    int bad = 0;
    double lprev = 0.0;
    // The only truly sequential part of the factorization is the chain pivot -> 1/sqrt -> next pivot.  It is kept on
    // wave-uniform scalars: with s1 = a[j+1] and s2 = a[j] at row j+1 (read by v_readlane BEFORE column j is scaled, i.e.
    // off the chain), l_{j+1,j} = s2 rinv and the next pivot is fma(-l, l, s1) -- exactly the operations the vector
    // update performs on that lane, so the results are bitwise those of the plain column sweep, but the chain per pivot is
    // rsq + one third-order step + 2 operations instead of also scaling the column, broadcasting it and updating the next one.
    double piv = bnr_readlane(a[0], COFF);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double tk[N];
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (j + 1 < N) { s1 = bnr_readlane(a[j + 1], COFF + j + 1); s2 = bnr_readlane(a[j], COFF + j + 1); }
        if (j + 2 < N) s3 = bnr_readlane(a[j], COFF + j + 2);
        if (!(piv > 0.0)) bad = 1;                       // not positive definite: NaNs from here on, reported by the caller
        // the reciprocal square root is started first: the wave issues in order, so the v_rsq_f64 (quarter rate, long latency)
        // runs while the broadcasts below are read
        double y = __builtin_amdgcn_rsq(piv);
        if (j == 0) hook();
        // the multipliers l_{k,j-1} of the lagged update come from the previous column's register by v_readlane (wave-uniform scalars):
        // no LDS write -> wait -> read round trip per pivot
        if (j >= 1) {
#pragma unroll
            for (int k = j + 2; k < N; ++k) tk[k] = bnr_readlane(lprev, COFF + k);
        }
        // v_rsq_f64 is good to 2^-24 (tools/rsq_precision.hip); ONE third-order step y (1 + e/2 + 3 e^2/8), e = 1 - x y^2,
        // gives 1.2 ulp -- what two Newton steps give -- in 5 instead of 8 operations and depth 4 instead of 6
        const double e = fma(-(piv * y), y, 1.0);
        const double rinv = fma(y * e, fma(0.375, e, 0.5), y);
        const double t1 = s2 * rinv;                     // l_{j+1,j}
        piv = fma(-t1, t1, s1);                          // next pivot
        double lj = a[j] * rinv;
        a[j] = lj;
        // (the publishing store names the next pivot as an in/out operand: without such a tie the scheduler walks the whole pivot chain first and sinks all N stores
        // behind it -- the waves behind would see the columns only when this wave is done)
        if (PUB == 2) asm volatile("ds_write_b64 %1, %2 offset:%3" : "+v"(piv) : "v"(pub_addr), "v"(lj), "n"(512 * j) : "memory");
        if (j + 1 < N) a[j + 1] = fma(-lj, t1, a[j + 1]);
        if (j + 2 < N) a[j + 2] = fma(-lj, s3 * rinv, a[j + 2]);
        if (j >= 1) {
#pragma unroll
            for (int k = j + 2; k < N; ++k) a[k] = fma(-lprev, tk[k], a[k]);
        }
        lprev = lj;
    }
    return bad;
}
// the one-wave sweep of 16 columns that k_chol_step2 keeps: nothing published
template <int COFF>
__device__ __forceinline__ int bnr_sweep16(double (&a)[16], int lane) { return bnr_sweepN<16, COFF, 0>(a, lane, 0u); }
template <int W>
__device__ __forceinline__ int bnr_pipe_wave(bnr_panelp_lds &sh, int lane, double *dst, size_t ld, unsigned long long *ph = nullptr)
{
#ifdef BNR_STAMPS
#define BNR_PPH(i) do { if (ph && lane == 0) ph[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BNR_PPH(i) do { } while (0)
#endif
    constexpr int C0 = 8 * W;
    const int rr = lane & 31;
    const double *src = (lane < 32) ? sh.sD : sh.sB;
    double a[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] = src[rr + BNR_LP * (C0 + c)];
    int bad = 0;
    // The columns of the waves in front, two per trip: this lane's row of both columns and their eight multipliers each -- rows C0 .. C0 + 7 of the column.  The
    // multipliers reach the lanes by DPP: one ds_read_b64 per column puts them into lanes 0 .. 7 of every row of 16 lanes (lane q of a row reads row C0 + (q & 7): eight
    // distinct addresses in 64 bytes, conflict-free), and the multiply-add takes its multiplier as "lane n of my row" (v_fmac_f64 with the DPP control row_newbcast:n,
    // the one DPP mode of 64-bit operands).  The four reads of the NEXT trip are in flight under this trip's sixteen multiply-adds.
    // What lost against it (profiles/round6_experiments_notes.txt):
    //   lane-uniform ds_read_b128 of the multipliers (the same address in every lane): 9 KiB through the LDS pipe per column pair instead of 2 KiB -- a lane-uniform
    //   read costs its full 1 KiB pass -- and 32 VGPRs of multipliers instead of 4; bitwise the same values (same products, same fused multiply-adds in the same order);
    //   multipliers by v_readlane out of the column's register: 16 + 16 v_readlane_b32 per column pair made a trip 420-500 cycles -- the waves behind fell a whole block of
    //   columns behind the chain and every hand-over waited 1 300 cycles for them.
#define BNR_PIPE_HERE(X0, X1) __all(__double2hiint(X0) != BNR_PIPE_SENT_HI && __double2hiint(X1) != BNR_PIPE_SENT_HI)
    // (OFF: byte offset of the column pair relative to the running addresses vc / vm)
    unsigned vc = bnr_lds_addr(&sh.sL[0][lane]), vm = bnr_lds_addr(&sh.sL[0][C0 + (lane & 7)]);
    double x0 = 0.0, x1 = 0.0, m0 = 0.0, m1 = 0.0, y0 = 0.0, y1 = 0.0, q0 = 0.0, q1 = 0.0;
    // (the reads are followed by an empty statement that names the accumulators: the multiply-adds that follow in the source stay behind the reads; the wait names
    // them too: the multiply-adds of the trip before stay in front of it, under the reads in flight)
#define BNR_DPP_READ4(X0, X1, M0, M1, OFF)                                                                                                                   \
    do { asm volatile("ds_read_b64 %0, %4 offset:%6\n\tds_read_b64 %1, %4 offset:%7\n\tds_read_b64 %2, %5 offset:%6\n\tds_read_b64 %3, %5 offset:%7"          \
                 : "=&v"(X0), "=&v"(X1), "=&v"(M0), "=&v"(M1) : "v"(vc), "v"(vm), "n"(OFF), "n"((OFF) + 512) : "memory");                                    \
         asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])); } while (0)
#define BNR_DPP_WAIT4(X0, X1, M0, M1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(X0), "+v"(X1), "+v"(M0), "+v"(M1), "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) :: "memory")
    // (not volatile: the scheduler places them by their operands -- behind the wait that names the registers, in front of whatever reads the column)
#define BNR_DPP_FMA(C, MM, X) asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(a[C]) : "v"(MM), "v"(X), "n"(C))
#define BNR_DPP_APPLY(CFROM, X0, X1, M0, M1)                                                                                                                 \
    do { _Pragma("unroll") for (int c_ = (CFROM); c_ < 8; ++c_) {                                                                                            \
             switch (c_) {                                                                                                                                   \
             case 0: BNR_DPP_FMA(0, M0, X0); BNR_DPP_FMA(0, M1, X1); break; case 1: BNR_DPP_FMA(1, M0, X0); BNR_DPP_FMA(1, M1, X1); break;                     \
             case 2: BNR_DPP_FMA(2, M0, X0); BNR_DPP_FMA(2, M1, X1); break; case 3: BNR_DPP_FMA(3, M0, X0); BNR_DPP_FMA(3, M1, X1); break;                     \
             case 4: BNR_DPP_FMA(4, M0, X0); BNR_DPP_FMA(4, M1, X1); break; case 5: BNR_DPP_FMA(5, M0, X0); BNR_DPP_FMA(5, M1, X1); break;                     \
             case 6: BNR_DPP_FMA(6, M0, X0); BNR_DPP_FMA(6, M1, X1); break; default: BNR_DPP_FMA(7, M0, X0); BNR_DPP_FMA(7, M1, X1); break; } } } while (0)
    // one trip: the pair at OFF is in flight into (X0, X1, M0, M1); wait, read again until it is there, start the next pair's reads, apply
#define BNR_DPP_TRIP(X0, X1, M0, M1, OFF, Y0, Y1, Q0, Q1)                                                                \
    do {                                                                                                                \
        BNR_DPP_WAIT4(X0, X1, M0, M1);                                                                                  \
        if (!BNR_PIPE_HERE(X0, X1)) {                                                                                   \
            int spins = 0;                                                                                              \
            do {                                                                                                        \
                if (++spins > BNR_PIPE_SPINS) { bad = 1; break; }                                                       \
                BNR_DPP_READ4(X0, X1, M0, M1, OFF);                                                                     \
                BNR_DPP_WAIT4(X0, X1, M0, M1);                                                                          \
            } while (!BNR_PIPE_HERE(X0, X1));                                                                           \
        }                                                                                                               \
        BNR_DPP_READ4(Y0, Y1, Q0, Q1, (OFF) + 1024);                                                                    \
        BNR_DPP_APPLY(0, X0, X1, M0, M1);                                                                               \
    } while (0)
    if (W > 0) {
        // C0 / 2 trips (4, 8, 12): all but the last in pairs through the rolled loop + one more; the LAST pair is the hand-over of the pivot chain to this wave: the moment it
        // is there the own columns 0 and 1 are brought up to date and the pivot chain starts; the other twelve multiply-adds run in the shadow of the first pivot's v_rsq_f64
        constexpr int NT = C0 / 2;
        BNR_DPP_READ4(x0, x1, m0, m1, 0);
#pragma unroll 1
        for (int t = 0; t + 2 < NT; t += 2) {
            BNR_DPP_TRIP(x0, x1, m0, m1, 0, y0, y1, q0, q1);
            BNR_DPP_TRIP(y0, y1, q0, q1, 1024, x0, x1, m0, m1);
            vc += 2048; vm += 2048;
        }
        BNR_DPP_TRIP(x0, x1, m0, m1, 0, y0, y1, q0, q1);                  // trip NT - 2; the hand-over pair's reads go out under its multiply-adds
        BNR_DPP_WAIT4(y0, y1, q0, q1);
        if (!BNR_PIPE_HERE(y0, y1)) {
            int spins = 0;
            do {
                if (++spins > BNR_PIPE_SPINS) { bad = 1; break; }
                BNR_DPP_READ4(y0, y1, q0, q1, 1024);
                BNR_DPP_WAIT4(y0, y1, q0, q1);
            } while (!BNR_PIPE_HERE(y0, y1));
        }
        BNR_DPP_FMA(0, q0, y0); BNR_DPP_FMA(0, q1, y1); BNR_DPP_FMA(1, q0, y0); BNR_DPP_FMA(1, q1, y1);
    }
    if (W == 1) BNR_PPH(3);
    if (W == 3) BNR_PPH(6);
    bad |= bnr_sweepN<8, C0, (W < 3 ? 2 : 0)>(a, lane, bnr_lds_addr(&sh.sL[C0][lane]), [&]() { if (W > 0) BNR_DPP_APPLY(2, y0, y1, q0, q1); });
    if (W == 0) BNR_PPH(2);
    if (W == 1) BNR_PPH(4);
    if (W == 2) BNR_PPH(5);
    if (W == 3) BNR_PPH(7);
    if (dst && lane >= 32) {
#pragma unroll
        for (int c = 0; c < 8; ++c) bnr_st8<BNR_ST_PANEL>(dst + (size_t)rr + ld * (size_t)(C0 + c), a[c]);
    }
    return bad;
}
// Sweep of the 64 x 32 panel [D ; B] by one workgroup of 256 threads: D = updated, unfactored diagonal block, B = own block, both handed over as the MFMA
// accumulator fragments (mt, nt) of the four waves.  The swept own block B L_D^-T goes to dst (E, leading dimension ld) straight from the sweeping waves' registers
// (lane = row: coalesced 256-byte stores); the factored diagonal block is not produced -- nobody needs it later.  Returns 1 in the waves that met a non-positive
// pivot (any wave may)
__device__ __forceinline__ int bnr_panel_sweep_pipe(bnr_panelp_lds &sh, const bnr_d4 &cD, const bnr_d4 &cB, int tid, double *dst, size_t ld, unsigned long long *ph = nullptr)
{
    const int wave = tid >> 6, lane = tid & 63, mt = wave >> 1, nt = wave & 1, ln = lane & 15, lq = lane >> 4;
#ifdef BNR_STAMPS
    if (ph && tid == 0) ph[0] = __builtin_amdgcn_s_memtime();
#endif
    {
        const double sent = __hiloint2double(BNR_PIPE_SENT_HI, 0);
        double *sl = &sh.sL[0][0];
#pragma unroll
        for (int i = 0; i < 6; ++i) sl[tid + 256 * i] = sent;      // columns 0..23: what the waves 0..2 will publish
    }
    // every NaN of the panel is staged as the canonical quiet NaN: data (a NaN loaded into S or X, its payload carried through the Gram and the updates) can
    // then never alias the "not there yet" mark, whose payload no arithmetic on canonical NaNs produces -- a NaN panel fails at once instead of after the polls
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sh.sD[(nt * 16 + ln) + BNR_LP * (mt * 16 + lq + 4 * r)] = bnr_canon_nan(cD[r]);
        sh.sB[(nt * 16 + ln) + BNR_LP * (mt * 16 + lq + 4 * r)] = bnr_canon_nan(cB[r]);
    }
    __syncthreads();
#ifdef BNR_STAMPS
    if (ph && tid == 0) ph[1] = __builtin_amdgcn_s_memtime();
#endif
    if (wave == 0) return bnr_pipe_wave<0>(sh, lane, dst, ld, ph);
    if (wave == 1) return bnr_pipe_wave<1>(sh, lane, dst, ld, ph);
    if (wave == 2) return bnr_pipe_wave<2>(sh, lane, dst, ld, ph);
    return bnr_pipe_wave<3>(sh, lane, dst, ld, ph);
}
// First touch of G + I: the 32 x 32 block (rho, c), rho >= c, as MFMA accumulator fragments -- NT x NT tiles of 16 x 16 starting at
// tile (at0, bt0) (columns at, rows bt; lane: row 16 bt + ln, columns 16 at + lq + 4 r) -- with the K-slice partials summed per
// element in k_gram_reduce's order (ks ascending from 0.0, then + 1 on the diagonal).  The loop runs over the K slices with
// all elements of a lane in flight per slice (the partial tiles come from HBM: one element at a time would cost ksplit x 16
// dependent round trips).
// (both callers pass NT = 1; written out for one tile the same sums compile to other instructions in k_chol_step, profiles/kernel_variants_cleanup.txt)
template <int NT>
__device__ __forceinline__ void bnr_gsum_frag(const bnr_dev &cd, int rho, int c, int at0, int bt0, int ln, int lq, bnr_d4 (&out)[NT][NT])
{
    const int ti = rho >> 1, tj = c >> 1, ntl = cd.ntile * (cd.ntile + 1) / 2;
    const size_t tsz = BNR_GT * BNR_GT, plane = (size_t)ntl * tsz;
    const double *src = cd.Gpart + (size_t)(ti * (ti + 1) / 2 + tj) * tsz + (size_t)((c & 1) * BNR_NB + 16 * at0 + lq) * BNR_GT + (rho & 1) * BNR_NB + 16 * bt0 + ln;
#pragma unroll
    for (int at = 0; at < NT; ++at)
#pragma unroll
        for (int bt = 0; bt < NT; ++bt) out[at][bt] = bnr_d4{0.0, 0.0, 0.0, 0.0};
    // KU slices per round, all in flight; a slice past the last one is read again from the last plane and enters as + 0.0, which
    // changes nothing (the running sum is never -0.0)
    constexpr int KU = NT == 1 ? 8 : 4;
    const int klast = cd.ksplit - 1;
    for (int ks0 = 0; ks0 < cd.ksplit; ks0 += KU) {
        bnr_d4 v[KU][NT][NT];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const size_t po = (size_t)(ks0 + u < klast ? ks0 + u : klast) * plane;
#pragma unroll
            for (int at = 0; at < NT; ++at)
#pragma unroll
                for (int bt = 0; bt < NT; ++bt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[u][at][bt][r] = *(src + po + (size_t)(16 * at + 4 * r) * BNR_GT + 16 * bt);
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
#pragma unroll
            for (int at = 0; at < NT; ++at)
#pragma unroll
                for (int bt = 0; bt < NT; ++bt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[at][bt][r] += (ks0 + u <= klast) ? v[u][at][bt][r] : 0.0;
        }
    }
    if (rho == c) {
#pragma unroll
        for (int at = 0; at < NT; ++at)
#pragma unroll
            for (int bt = 0; bt < NT; ++bt)
#pragma unroll
                for (int r = 0; r < 4; ++r) if (16 * (bt0 + bt) + ln == 16 * (at0 + at) + lq + 4 * r) out[at][bt][r] += 1.0;
    }
}
// The work of EPW k_gram_reduce workgroups (tile t, the eighths part0 .. part0 + EPW - 1; g0 = 8 t + part0, EPW divides 8) done by ONE workgroup of launch 0 of the
// factorization (fuse0): the same sums in the same order, a share of Y = I and the same stamp words -- except what launch 0's own panel workgroups produce at the
// same time: the first 32 columns of E's matrix part (they read the partial tiles themselves and write the swept blocks) and the block Y[0:32, 0:32].
// The launch is a chain of round trips per workgroup, not a stream (profiles/launch0_reduce.txt): every workgroup carries the panel role's registers and LDS, so four
// of them share a CU.  Hence fewer, fatter workgroups, and nothing that does not depend on the partial tiles waits for them: a thread issues the loads of all its
// slices -- EPW eighths x KB slices of 16 bytes, at most 16 in flight = 64 VGPRs, well inside the panel role's count -- then its Y = I stores and the gprog reset,
// and only then waits and adds, every element in ascending ks from +0.0 (k_gram_reduce's order), K splits above KB in batches of KB (8; 4 with four eighths, for the
// 64 VGPRs).
template <int EPW>
__device__ __forceinline__ void bnr_reduce_parts(const bnr_dev &cd, int g0, int nwg, int wg, int s)
{
    constexpr int KB = EPW == 4 ? 4 : 8;
    const int tid = threadIdx.x, t = g0 >> 3, part0 = g0 & 7;
    const int ntl = cd.ntile * (cd.ntile + 1) / 2, ksplit = cd.ksplit;
    const size_t ld = (size_t)2 * cd.n_pad + BNR_NB, tsz = BNR_GT * BNR_GT, plane = (size_t)ntl * tsz;
    const double *src = cd.Gpart + (size_t)t * tsz + part0 * 512 + 2 * tid;
    bnr_d2 v[KB][EPW], acc[EPW];
    // the stamp's iteration number is two dependent loads: the first goes out in front of the slice loads (volatile: it stays there), the second behind them, once
    // the first is back -- loads return in order, so neither waits for a slice nor holds the stamp up at the end.  Nothing but the compiler's present scheduling
    // holds that order and no test can see it: written as one expression behind the slice loads both round trips sat in front of the Y stores again
    // (profiles/launch0_reduce.txt, 6c).  After a compiler change look at the role's disassembly, or at slot 7 of step 0 in a -DBNR_STAMPS build.
    const int pb = *(const volatile int *)cd.pbase;
    // (ks < ksplit is wave-uniform: scalar branches round the loads, which stay in flight across them)
#define BNR_RP_LOAD(KS0)                                                                                                          \
    _Pragma("unroll") for (int u = 0; u < KB; ++u) {                                                                              \
        _Pragma("unroll") for (int e = 0; e < EPW; ++e) v[u][e] = bnr_d2{0.0, 0.0};                                               \
        if ((KS0) + u < ksplit) {                                                                                                 \
            _Pragma("unroll") for (int e = 0; e < EPW; ++e) v[u][e] = *(const bnr_d2 *)(src + (size_t)((KS0) + u) * plane + e * 512); \
        }                                                                                                                         \
    }
    BNR_RP_LOAD(0)
    const unsigned int it = cd.plan[pb + s].it;
    const int np = cd.n_pad;
    for (size_t e = ((size_t)wg * 256 + tid) * 2; e < (size_t)np * np; e += (size_t)nwg * 512) {
        const int r = (int)(e % np), c = (int)(e / np);
        if ((r < BNR_NB && c < BNR_NB) || r / BNR_NB > c / BNR_NB) continue;   // (below the diagonal block Y is never written and never read)
        bnr_d2 y = {(r == c) ? 1.0 : 0.0, (r + 1 == c) ? 1.0 : 0.0};
        bnr_st16<BNR_ST_LAUNCH0>(cd.E + (size_t)(np + r) + ld * c, y);
    }
    if (wg == 0 && tid <= cd.ntile) cd.gprog[tid] = 0u;
#pragma unroll
    for (int e = 0; e < EPW; ++e) acc[e] = bnr_d2{0.0, 0.0};
    for (int ks0 = 0;;) {
#pragma unroll
        for (int u = 0; u < KB; ++u)
            if (ks0 + u < ksplit) {
#pragma unroll
                for (int e = 0; e < EPW; ++e) acc[e] += v[u][e];
            }
        ks0 += KB;
        if (ks0 >= ksplit) break;
        BNR_RP_LOAD(ks0)
    }
#undef BNR_RP_LOAD
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
#pragma unroll
    for (int e = 0; e < EPW; ++e) {
        const int idx = (part0 + e) * 512 + 2 * tid;
        const int i = ti * BNR_GT + idx % BNR_GT, j = tj * BNR_GT + idx / BNR_GT;
        if (i == j) acc[e][0] += 1.0;
        if (i + 1 == j) acc[e][1] += 1.0;
        if (j >= BNR_NB) bnr_st16<BNR_ST_LAUNCH0>(cd.E + (size_t)i + ld * j, acc[e]);
    }
    if (tid < EPW) cd.stamp[g0 + tid] = it;                  // one word per eighth, as k_gram_reduce writes them
#ifdef BNR_STAMPS
    if (tid == 0) atomicMax((unsigned long long *)&cd.dbg[7], (unsigned long long)__builtin_amdgcn_s_memrealtime());     // slot 7 of step 0: the latest reduction workgroup's end
#endif
}
// (__launch_bounds__(256, BNR_CHOL_WG_PER_CU): four waves per SIMD, i.e. at most 128 VGPRs.  Without it bnr_one takes 126 and bnr_many 128, but bnr_few took 130 once the
// reduction role changed, against 128 before -- three waves per SIMD instead of four at every step p >= 2 of a group.  With it all three take 126, no scratch.)
// BNR_CHOL_WG_PER_CU: workgroups of k_chol_step (four waves, one per SIMD) that share a CU.  The launch bound holds the registers to it, the static assertion in
// the kernel the LDS (160 KiB per CU); the host's choice for launch 0 (reduce_epw_default) counts a round of workgroups with the same number.
#define BNR_CHOL_WG_PER_CU 4
template <class SRC>
__global__ __launch_bounds__(256, BNR_CHOL_WG_PER_CU) void k_chol_step(const SRC chain_src, int p, int s, int tpw, int spw, int fuse0)
{
    BNR_CRITICAL_PATH();
#ifdef BNR_STAMPS
    const unsigned long long t_entry = __builtin_amdgcn_s_memtime();       // before anything is read, the kernel's arguments included
#endif
    const bnr_dev &cd = chain_src.get_x();               // grid = (chains, workgroups): blockIdx.x = chain, blockIdx.y = workgroup
    __shared__ bnr_panelp_lds sh;
    static_assert(sizeof(sh.sL) == 2 * BNR_NB * BNR_NB * sizeof(double), "the two fetched blocks of panel p - 1 live where the sweep's published columns will be");
    static_assert(BNR_CHOL_WG_PER_CU * sizeof(bnr_panelp_lds) <= 160 * 1024, "BNR_CHOL_WG_PER_CU workgroups must fit a CU's LDS");
    double (*sPO)[BNR_NB * BNR_NB] = (double (*)[BNR_NB * BNR_NB])&sh.sL[0][0];   // (no LDS of their own: the update workgroups of the launch carry the same static allocation)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nbk = cd.n_pad / BNR_NB;
    const size_t ld = bnr_ldE(cd.n_pad);
    const int npanel = bnr_chol_npanel(nbk, p);
    const int pc = p * BNR_NB, kc = pc - BNR_NB;
    const int mt = wave >> 1, nt = wave & 1;               // this wave's 16x16 tile of a 32x32 block: columns mt, rows nt
    const int ln = lane & 15, lq = lane >> 4;
    double *E = cd.E;
    if (SRC::whole && p == 0 && (int)blockIdx.y >= npanel) {               // (bnr_few: steps p >= 2 only, and no Gram in its descriptor)
        // ------------------------------------------------ launch 0 with fuse0: the reduction of the Gram's K-split partial tiles, beside the first panel
        // (tpw = the eighths of a tile per workgroup: 1, 2 or 4, the host's choice per launch)
        const int wg = (int)blockIdx.y - npanel, nwg = (int)gridDim.y - npanel;
        if (SRC::lone || tpw == 1) bnr_reduce_parts<1>(cd, wg, nwg, wg, s);      // (a chain alone: one eighth each whatever tpw says -- only that copy is compiled into its kernel)
        else if (tpw == 4) bnr_reduce_parts<4>(cd, 4 * wg, nwg, wg, s);
        else bnr_reduce_parts<2>(cd, 2 * wg, nwg, wg, s);
        return;
    }
    if ((int)blockIdx.y >= npanel) {
        // ------------------------------------------------ role B: E[rho,j] -= L[rho,p-1] L[j,p-1]'
        const int m = nbk - (p + 1);
        if (tpw == 0) {
            // large trailing matrix: one workgroup per 64 x 64 super block (2 x 2 blocks), one 32 x 32 block per wave as
            // 2 x 2 MFMA tiles -- half the fragment loads per MFMA and a quarter of the workgroups; every element still sees
            // the same eight MFMA steps in the same order, so the result is bitwise that of the small-block path
            const int ms = (m + 1) / 2, ntri = ms * (ms + 1) / 2, nsup = bnr_chol_nsuper(nbk, p);
            // spw super blocks per workgroup (host: as many as it takes for the update workgroups to fit the CUs the panel
            // workgroups leave free -- a sweeping wave that shares its SIMD with MFMA work of another workgroup runs 20 % slower)
            for (int u = 0; u < spw; ++u) {
                int t = ((int)blockIdx.y - npanel) * spw + u, R0, C0;
                if (t >= nsup) break;
                bool ident = false;
                if (t < ntri) {
                    int ti = 0;
                    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
                    int tj = t - ti * (ti + 1) / 2;
                    R0 = p + 1 + 2 * ti; C0 = p + 1 + 2 * tj;
                } else {
                    t -= ntri;
                    const int ps = (p + 1) / 2;
                    C0 = p + 1 + 2 * (t / ps); R0 = nbk + 2 * (t % ps);
                    ident = true;
                }
                const int rho = R0 + (wave >> 1), j = C0 + (wave & 1);
                const bool ok = j < nbk && (ident ? (rho - nbk < p) : (rho < nbk && rho >= j));
                if (!ok) continue;
                double *cp = E + (size_t)(rho * BNR_NB + ln) + ld * (size_t)(j * BNR_NB + lq);
                bnr_d4 c[2][2];                                   // [column tile][row tile]
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) c[a][b][r] = cp[(size_t)(16 * b) + ld * (size_t)(16 * a + 4 * r)];
                const double *colrows = E + (size_t)(j * BNR_NB) + ld * (size_t)kc, *rowrows = E + (size_t)(rho * BNR_NB) + ld * (size_t)kc;
                double av[2][8], bv[2][8];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const size_t o = (size_t)ln + ld * (size_t)(4 * ks + lq);
                    av[0][ks] = colrows[o]; av[1][ks] = colrows[o + 16];
                    bv[0][ks] = rowrows[o]; bv[1][ks] = rowrows[o + 16];
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b) c[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[a][ks], bv[b][ks], c[a][b], 0, 0, 0);
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int r = 0; r < 4; ++r) bnr_st8<BNR_ST_UPDATE>(cp + (size_t)(16 * b) + ld * (size_t)(16 * a + 4 * r), c[a][b][r]);
            }
#ifdef BNR_STAMPS
            if (tid == 0) atomicMax((unsigned long long *)&cd.dbg[p * 8 + 7], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
            return;
        }
        // few blocks: tpw of them per workgroup, each wave one 16 x 16 tile of every block
        const int ntri = m * (m + 1) / 2, ntot = bnr_chol_ntile(nbk, p);
        const int t0 = ((int)blockIdx.y - npanel) * tpw;
        for (int tt = 0; tt < tpw && t0 + tt < ntot; ++tt) {
            int t = t0 + tt, rho, j;
            if (t < ntri) {
                int ti = 0;
                while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
                int tj = t - ti * (ti + 1) / 2;
                rho = p + 1 + ti; j = p + 1 + tj;
            } else {
                t -= ntri;
                j = p + 1 + t / p;
                rho = nbk + t % p;                         // identity block row
            }
            double *cp = E + (size_t)(rho * BNR_NB + nt * 16 + ln) + ld * (size_t)(j * BNR_NB + mt * 16 + lq);
            bnr_d4 c;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = cp[ld * (size_t)(4 * r)];
            c = bnr_tile_update(E + (size_t)(j * BNR_NB + mt * 16) + ld * (size_t)kc, E + (size_t)(rho * BNR_NB + nt * 16) + ld * (size_t)kc, ld, lane, c);
#pragma unroll
            for (int r = 0; r < 4; ++r) bnr_st8<BNR_ST_UPDATE>(cp + ld * (size_t)(4 * r), c[r]);
        }
#ifdef BNR_STAMPS
        if (tid == 0) atomicMax((unsigned long long *)&cd.dbg[p * 8 + 7], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
        return;
    }
    // ---------------------------------------------------- role A: panel workgroup
    const int b = blockIdx.y;
    if (p == (fuse0 ? 1 : 0) && b == 0) {
        // cheap safety net for the two-branch schedule: every reduction workgroup of THIS sweep (k_gram_reduce, or launch 0's with fuse0) must have finished
        const unsigned int it = cd.plan[cd.pbase[0] + s].it;
        const int nred = 8 * (cd.ntile * (cd.ntile + 1) / 2);
        for (int w = tid; w < nred; w += blockDim.x)
            if (cd.stamp[w] != it) atomicAdd((unsigned long long *)&cd.counters[8], 1ull);
    }
#ifdef BNR_STAMPS
#define BNR_STAMP(slot) do { if (b == 0 && tid == 0) cd.dbg[p * 8 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BNR_STAMP(slot) do { } while (0)
#endif
    BNR_STAMP(0);
#ifdef BNR_STAMPS
    if (tid == 0) {                                        // s_memrealtime (100 MHz, the same on every XCD): slot 1 = start of panel workgroup 0, 6 = latest panel start, 5 / 7 = latest panel / update end (tools/stamps_spread.py)
        const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
        if (b == 0) cd.dbg[p * 8 + 1] = rt;
        atomicMax((unsigned long long *)&cd.dbg[p * 8 + 6], rt);
    }
#endif
    int rho;                                               // own block row
    if (b < nbk - p) rho = p + b;                          // matrix rows p..nbk-1
    else rho = nbk + (b - (nbk - p));                      // identity block rows 0..p
    bnr_d4 cD, cB;
    if (p == 0 && fuse0) {
        // first touch of column block 0: the K-slice partials summed here (k_gram_reduce's order), the identity block row generated
        bnr_d4 t1[1][1];
        bnr_gsum_frag<1>(cd, 0, 0, mt, nt, ln, lq, t1);
        cD = t1[0][0];
        if (rho < nbk) { bnr_gsum_frag<1>(cd, rho, 0, mt, nt, ln, lq, t1); cB = t1[0][0]; }
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) cB[r] = (nt * 16 + ln == mt * 16 + lq + 4 * r) ? 1.0 : 0.0;
        }
    } else {
        const double *dp = E + (size_t)(pc + nt * 16 + ln) + ld * (size_t)(pc + mt * 16 + lq);
        const double *bp = E + (size_t)(rho * BNR_NB + nt * 16 + ln) + ld * (size_t)(pc + mt * 16 + lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) { cD[r] = dp[ld * (size_t)(4 * r)]; cB[r] = bp[ld * (size_t)(4 * r)]; }
#ifdef BNR_STAMPS           // (wave 0 of panel workgroup 0: entry of the kernel | its loads are back | its MFMAs are done -- words 3800 + 4 p of the debug buffer, tools/stamps_steps.py)
        if (b == 0 && tid == 0 && p < 24) cd.dbg[3800 + 4 * p] = t_entry;
#endif
        if (p > 0) {
            // The K = 32 update of both blocks with panel p - 1: the two 32 x 32 blocks of that panel it needs -- P = L[p, p-1] and O = L[own, p-1] -- are fetched ONCE per
            // workgroup, 16 bytes per lane and whole columns per quarter wave, into LDS; the MFMA fragments come from there.  (Fragments straight from memory: every wave
            // fetched its three sets itself, 24 eight-byte loads per lane, each a quarter line of four columns -- 64 KB through the CU's 64 B/clk vector-memory path where
            // 32 KB are distinct, 3 100 cycles until the loads were back; profiles/round6_experiments_notes.txt J.)  Same products in the same order: bitwise the same blocks.
            // Image: column c at 32 c doubles, the two 16-row halves of the odd columns swapped: a fragment read (16 rows x columns 4 ks + (0, 1) per half wave) covers all banks once.
            const int fc = tid >> 4, fr = (tid & 15) * 2;                       // this thread: rows fr, fr + 1 of the columns fc and fc + 16
            const double *gP = E + (size_t)(pc + fr) + ld * (size_t)(kc + fc), *gO = E + (size_t)(rho * BNR_NB + fr) + ld * (size_t)(kc + fc);
            const bnr_d2 p0 = *(const bnr_d2 *)gP, p1 = *(const bnr_d2 *)(gP + ld * 16), o0 = *(const bnr_d2 *)gO, o1 = *(const bnr_d2 *)(gO + ld * 16);
            const int wo = (fr ^ ((fc & 1) << 4)) + 32 * fc;
            *(bnr_d2 *)&sPO[0][wo] = p0; *(bnr_d2 *)&sPO[0][wo + 512] = p1;
            *(bnr_d2 *)&sPO[1][wo] = o0; *(bnr_d2 *)&sPO[1][wo + 512] = o1;
            __syncthreads();
#ifdef BNR_STAMPS
            if (b == 0 && tid == 0 && p < 24) cd.dbg[3800 + 4 * p + 1] = __builtin_amdgcn_s_memtime();
#endif
            const int lk = lane >> 4;
            double av[8], b1[8], b2[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int c = 4 * ks + lk, sw = (c & 1) << 4;
                av[ks] = sPO[0][((mt * 16 + ln) ^ sw) + 32 * c]; b1[ks] = sPO[0][((nt * 16 + ln) ^ sw) + 32 * c]; b2[ks] = sPO[1][((nt * 16 + ln) ^ sw) + 32 * c];
            }
            __syncthreads();                    // every wave has its fragments in registers: the sweep may write its "not there yet" marks over the two blocks
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) cD = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[ks], b1[ks], cD, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) cB = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[ks], b2[ks], cB, 0, 0, 0);
#ifdef BNR_STAMPS
            { double chk = cD[3] + cB[3]; asm volatile("" :: "v"(chk)); if (b == 0 && tid == 0 && p < 24) cd.dbg[3800 + 4 * p + 2] = __builtin_amdgcn_s_memtime(); }
#endif
        }
    }
    BNR_STAMP(2);
    // (the factored diagonal block L_pp is needed by nobody after this launch and is NOT written back: every panel workgroup of
    // this launch reads the unfactored block (p,p) whenever it happens to start)
    double *dst = rho != p ? E + (size_t)(rho * BNR_NB) + ld * (size_t)pc : nullptr;
#ifdef BNR_STAMPS
    const int bad = bnr_panel_sweep_pipe(sh, cD, cB, tid, dst, ld, b == 0 ? cd.dbg + 128 + p * 8 : nullptr);
#else
    const int bad = bnr_panel_sweep_pipe(sh, cD, cB, tid, dst, ld);
#endif
    if (bad && lane == 0) bnr_flag_gfail(cd);
    BNR_STAMP(3);
    BNR_STAMP(4);
#ifdef BNR_STAMPS
    if (lane == 0) atomicMax((unsigned long long *)&cd.dbg[p * 8 + 5], (unsigned long long)__builtin_amdgcn_s_memrealtime());      // (every wave: with the four-wave sweep, bnr_panel_sweep_pipe, wave 3 is the last one)
    if (b == 0 && tid == 192 && p < 48) { cd.dbg[3900 + 2 * p] = __builtin_amdgcn_s_memrealtime(); cd.dbg[3901 + 2 * p] = __builtin_amdgcn_s_memtime(); }      // the LAST wave of panel workgroup 0 on both clocks (tools/stamps_steps.py: which clock do the panel steps run at?)
#endif
}

// ----------------------------------------------------------------------------------------- two panels per launch
// k_chol_step2(P), P = 0..nbk/2-1: the right-looking factorization of k_chol_step with the panels a = 2P and b = 2P+1 handled by ONE
// launch -- the same operations on every element in the same order (bitwise the same E), half the launches on the critical
// path (8 instead of 16 at n = 500: a launch boundary plus the first round trip to L2 cost ~3 us each, and the panel chain is a
// third of the sweep).
//   role A (nbk workgroups: matrix block rows >= 2P+2, identity rows 0..2P+1), per workgroup and in this order:
//     0. blocks (a,a), (b,a), (b,b), (own,a), (own,b) <- pending updates of the panels 2P-2 and 2P-1 (MFMA, fragments from L2);
//     1. wave 0 sweeps [(a,a) ; (own,a)], wave 1 sweeps [(a,a) ; (b,a)] at the same time (block row b of panel a is needed by
//        everybody and redone by everybody, like the diagonal block);
//     2. (b,b) -= L_ba L_ba', (own,b) -= L_own,a L_ba'   (MFMA from LDS: panel a's update of panel b's columns);
//     3. wave 0 sweeps [(b,b) ; (own,b)].
//   role B: E[rho,j] -= L[rho,2P-2] L[j,2P-2]' + L[rho,2P-1] L[j,2P-1]' (in that order) for j >= 2P+2: the trailing update of the
//     previous launch's two panels, beside role A (look-ahead as before).
struct bnr_panel2_lds {
    double sDaa[BNR_NB * BNR_LP], sDba[BNR_NB * BNR_LP], sDbb[BNR_NB * BNR_LP], sOa[BNR_NB * BNR_LP], sOb[BNR_NB * BNR_LP];
    double pad_[2][2][BNR_NB];          // unread (once the lagged multipliers of bnr_sweep16 travelled through it): kept so that sL1 and with it the ds offsets of k_chol_step2 stay where they are
    double sL1[2][16 * BNR_L1S];
};
// one half-sweep helper: registers <- LDS panel [D ; B] (lane = row), columns c0..c0+15
__device__ __forceinline__ void bnr_panel_load16(double (&a)[16], const double *sD, const double *sB, int lane, int c0)
{
    const double *src = (lane < 32) ? sD : sB;
    const int rr = lane & 31;
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = src[rr + BNR_LP * (c0 + c)];
}
// 16 x 16 tile (columns mt, rows nt) of  C - A B'  with K = 32 from LDS blocks (row + BNR_LP * col): A = rows of `colside`, B = rows of `rowside`
__device__ __forceinline__ void bnr_lds_tile_update(double *sC, const double *colside, const double *rowside, int mt, int nt, int ln, int lq)
{
    bnr_d4 c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = sC[(nt * 16 + ln) + BNR_LP * (mt * 16 + lq + 4 * r)];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-colside[(mt * 16 + ln) + BNR_LP * (4 * ks + lq)], rowside[(nt * 16 + ln) + BNR_LP * (4 * ks + lq)], c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) sC[(nt * 16 + ln) + BNR_LP * (mt * 16 + lq + 4 * r)] = c[r];
}
// second-half update of a swept half panel:  X[rowb.., 16:32] -= L[rowb.., 0:16] L[16:32, 0:16]'  for the 16 rows rowb.. of block sX,
// L from the 64-row image sL1 (rows 0..31 diagonal block, 32..63 own block); lrow = row of the tile inside sL1
__device__ __forceinline__ void bnr_mid_tile(double *sX, int rowb, const double *sL1, int lrow, int ln, int lq)
{
    bnr_d4 c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = sX[(rowb + ln) + BNR_LP * (16 + lq + 4 * r)];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const double av = sL1[(4 * ks + lq) * BNR_L1S + 16 + ln];            // column side: rows 16..31 of the diagonal part
        const double bv = sL1[(4 * ks + lq) * BNR_L1S + lrow + ln];          // row side
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(-av, bv, c, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sX[(rowb + ln) + BNR_LP * (16 + lq + 4 * r)] = c[r];
}
// lazy = 1 (variant 3): the read-modify-write of the whole trailing matrix happens at the ODD launches only, with the four panels of the
// two launches before (K = 128); an EVEN launch only brings the next launch's two panel columns up to date (panels of the launch
// before, K = 64).  Every element still sees the panels in ascending order, eight MFMA k-steps each: bitwise the same E with half the
// trailing traffic.
__host__ __device__ inline int bnr_chol2_nsuper(int nbk, int P, int lazy = 0)     // 64 x 64 super blocks of launch P's trailing update
{
    if (P == 0) return 0;
    const int m = nbk - 2 * P - 2, ms = (m + 1) / 2;
    if (m <= 0) return 0;
    if (lazy && !(P & 1)) return ms + P;                 // the super column of the next launch's panels only
    return ms * (ms + 1) / 2 + ms * P;
}
// One wave's 32 x 32 block (rho, j) of the trailing matrix <- - sum over the NQ pending panels q0.. of L[rho,q] L[j,q]' (ascending q, eight MFMA
// k-steps each); the block and all NQ panels' fragments are requested before the first MFMA.
template <int NQ>
__device__ __forceinline__ void bnr_super_update(double *E, size_t ld, int rho, int j, int q0, int ln, int lq)
{
    double *cp = E + (size_t)(rho * BNR_NB + ln) + ld * (size_t)(j * BNR_NB + lq);
    bnr_d4 c[2][2];                                   // [column tile][row tile]
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r) c[at][bt][r] = cp[(size_t)(16 * bt) + ld * (size_t)(16 * at + 4 * r)];
    double av[NQ][2][8], bv[NQ][2][8];
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int kc = (q0 + qq) * BNR_NB;
        const double *colrows = E + (size_t)(j * BNR_NB) + ld * (size_t)kc, *rowrows = E + (size_t)(rho * BNR_NB) + ld * (size_t)kc;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const size_t o = (size_t)ln + ld * (size_t)(4 * ks + lq);
            av[qq][0][ks] = colrows[o]; av[qq][1][ks] = colrows[o + 16];
            bv[qq][0][ks] = rowrows[o]; bv[qq][1][ks] = rowrows[o + 16];
        }
    }
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int at = 0; at < 2; ++at)
#pragma unroll
                for (int bt = 0; bt < 2; ++bt) c[at][bt] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[qq][at][ks], bv[qq][bt][ks], c[at][bt], 0, 0, 0);
#pragma unroll
    for (int at = 0; at < 2; ++at)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
            for (int r = 0; r < 4; ++r) cp[(size_t)(16 * bt) + ld * (size_t)(16 * at + 4 * r)] = c[at][bt][r];
}
template <class SRC>
__global__ __launch_bounds__(256, 1) void k_chol_step2(const SRC chain_src, int P, int s, int spw, int lazy)
{
    BNR_CRITICAL_PATH();
    const bnr_dev &cd = chain_src.get_x();               // grid = (chains, workgroups)
    __shared__ bnr_panel2_lds sh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nbk = cd.n_pad / BNR_NB;
    const size_t ld = bnr_ldE(cd.n_pad);
    const int a = 2 * P, b = a + 1, pa = a * BNR_NB, pb = b * BNR_NB;
    const int ln = lane & 15, lq = lane >> 4;
    double *E = cd.E;
    if ((int)blockIdx.y >= nbk) {
        // ------------------------------------------------ role B: trailing update with the panels 2P-2 and 2P-1, 64 x 64 super blocks
        const int m = nbk - 2 * P - 2, ms = (m + 1) / 2, nsup = bnr_chol2_nsuper(nbk, P, lazy);
        const bool near = lazy && !(P & 1);
        const int ntri = near ? ms : ms * (ms + 1) / 2;
        const int q0 = (lazy && (P & 1) && a >= 4) ? a - 4 : a - 2, nq = a - q0;      // pending panels q0 .. a-1
        for (int u = 0; u < spw; ++u) {
            int t = ((int)blockIdx.y - nbk) * spw + u, R0, C0;
            if (t >= nsup) break;
            bool ident = false;
            if (t < ntri) {
                int ti = 0, tj = 0;
                if (near) ti = t;
                else {
                    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
                    tj = t - ti * (ti + 1) / 2;
                }
                R0 = a + 2 + 2 * ti; C0 = a + 2 + 2 * tj;
            } else {
                t -= ntri;
                C0 = a + 2 + 2 * (t / P); R0 = nbk + 2 * (t % P);
                ident = true;
            }
            const int rho = R0 + (wave >> 1), j = C0 + (wave & 1);
            const bool ok = j < nbk && (ident ? (rho - nbk < a) : (rho < nbk && rho >= j));
            if (!ok) continue;
            if (nq == 4) bnr_super_update<4>(E, ld, rho, j, q0, ln, lq);
            else bnr_super_update<2>(E, ld, rho, j, q0, ln, lq);
        }
        return;
    }
    // ---------------------------------------------------- role A
    const int bi = blockIdx.y;
    if (P == 0 && bi == 0) {
        // cheap safety net for the two-branch schedule: every k_gram_reduce workgroup of THIS sweep must have finished
        const unsigned int it = cd.plan[cd.pbase[0] + s].it;
        const int nred = 8 * (cd.ntile * (cd.ntile + 1) / 2);
        for (int w = tid; w < nred; w += blockDim.x)
            if (cd.stamp[w] != it) atomicAdd((unsigned long long *)&cd.counters[8], 1ull);
    }
    // own block row: matrix rows 2P+2.., then identity rows 0..2P+1
    const int nmat = nbk - b - 1;
    const int R = bi < nmat ? b + 1 + bi : nbk + (bi - nmat);
    const bool only_b = bi >= nmat && (bi - nmat) == b;        // identity row b: block (b, a) of Y is zero and stays zero, only panel b applies
    {
        // 0. the five blocks as MFMA tiles (wave = tile: columns mt, rows nt) with the pending updates of the panels 2P-2, 2P-1
        const int mt = wave >> 1, nt = wave & 1;
        bnr_d4 cAA, cBA, cBB, cOA, cOB;
        const size_t orow = (size_t)(nt * 16 + ln), ocol = ld * (size_t)(mt * 16 + lq);
        const double *pAA = E + (size_t)pa + orow + ld * (size_t)pa + ocol, *pBA = E + (size_t)pb + orow + ld * (size_t)pa + ocol;
        const double *pBB = E + (size_t)pb + orow + ld * (size_t)pb + ocol;
        const double *pOA = E + (size_t)(R * BNR_NB) + orow + ld * (size_t)pa + ocol, *pOB = E + (size_t)(R * BNR_NB) + orow + ld * (size_t)pb + ocol;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t o = ld * (size_t)(4 * r);
            cAA[r] = pAA[o]; cBA[r] = pBA[o]; cBB[r] = pBB[o]; cOA[r] = pOA[o]; cOB[r] = pOB[o];
        }
        if (P > 0) {
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                const size_t kc = ld * (size_t)((a - 2 + qq) * BNR_NB);
                // fragments of L[., q]: column sides of block columns a and b (rows mt), row sides of block rows a, b, own (rows nt)
                double ca[8], cb[8], ra[8], rb[8], ro[8];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const size_t o = kc + (size_t)ln + ld * (size_t)(4 * ks + lq);
                    ca[ks] = E[(size_t)(pa + mt * 16) + o]; cb[ks] = E[(size_t)(pb + mt * 16) + o];
                    ra[ks] = E[(size_t)(pa + nt * 16) + o]; rb[ks] = E[(size_t)(pb + nt * 16) + o];
                    ro[ks] = E[(size_t)(R * BNR_NB + nt * 16) + o];
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    cAA = __builtin_amdgcn_mfma_f64_16x16x4f64(-ca[ks], ra[ks], cAA, 0, 0, 0);
                    cBA = __builtin_amdgcn_mfma_f64_16x16x4f64(-ca[ks], rb[ks], cBA, 0, 0, 0);
                    cBB = __builtin_amdgcn_mfma_f64_16x16x4f64(-cb[ks], rb[ks], cBB, 0, 0, 0);
                    cOA = __builtin_amdgcn_mfma_f64_16x16x4f64(-ca[ks], ro[ks], cOA, 0, 0, 0);
                    cOB = __builtin_amdgcn_mfma_f64_16x16x4f64(-cb[ks], ro[ks], cOB, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (nt * 16 + ln) + BNR_LP * (mt * 16 + lq + 4 * r);
            sh.sDaa[o] = cAA[r]; sh.sDba[o] = cBA[r]; sh.sDbb[o] = cBB[r]; sh.sOa[o] = cOA[r]; sh.sOb[o] = cOB[r];
        }
    }
    __syncthreads();
    int bad = 0;
    double a1[16], a2[16];
    const int rr = lane & 31;
    // 1. panel a: wave 0 on [Daa ; Oa], wave 1 on [Daa ; Dba]
    double *sBw = wave == 0 ? sh.sOa : sh.sDba;
    if (wave < 2) {
        bnr_panel_load16(a1, sh.sDaa, sBw, lane, 0);
        bad = bnr_sweep16<0>(a1, lane);
#pragma unroll
        for (int c = 0; c < 16; ++c) sh.sL1[wave][c * BNR_L1S + lane] = a1[c];
    }
    __syncthreads();
    // second halves: the diagonal rows once (waves 0, 1: one tile each), the own rows of the two panels by waves 2 and 3
    if (wave < 2) bnr_mid_tile(sh.sDaa, wave * 16, sh.sL1[0], wave * 16, ln, lq);
    else {
        double *sX = wave == 2 ? sh.sOa : sh.sDba;
        bnr_mid_tile(sX, 0, sh.sL1[wave - 2], 32, ln, lq);
        bnr_mid_tile(sX, 16, sh.sL1[wave - 2], 48, ln, lq);
    }
    __syncthreads();
    if (wave < 2) {
        bnr_panel_load16(a2, sh.sDaa, sBw, lane, 16);
        bad |= bnr_sweep16<16>(a2, lane);
        if (lane >= 32) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { sBw[rr + BNR_LP * c] = a1[c]; sBw[rr + BNR_LP * (16 + c)] = a2[c]; }
        }
    }
    __syncthreads();
    // 2. panel a's update of panel b's columns:  Dbb -= L_ba L_ba',  Ob -= L_own,a L_ba'   (two tiles per wave)
    {
        const int mt = wave >> 1, nt = wave & 1;
        bnr_lds_tile_update(sh.sDbb, sh.sDba, sh.sDba, mt, nt, ln, lq);
        bnr_lds_tile_update(sh.sOb, sh.sDba, sh.sOa, mt, nt, ln, lq);
    }
    __syncthreads();
    // 3. panel b: wave 0 on [Dbb ; Ob], the second half updated by all four waves
    if (wave == 0) {
        bnr_panel_load16(a1, sh.sDbb, sh.sOb, lane, 0);
        bad |= bnr_sweep16<0>(a1, lane);
#pragma unroll
        for (int c = 0; c < 16; ++c) sh.sL1[0][c * BNR_L1S + lane] = a1[c];
    }
    __syncthreads();
    bnr_mid_tile(wave < 2 ? sh.sDbb : sh.sOb, (wave & 1) * 16, sh.sL1[0], 16 * wave, ln, lq);
    __syncthreads();
    if (wave == 0) {
        bnr_panel_load16(a2, sh.sDbb, sh.sOb, lane, 16);
        bad |= bnr_sweep16<16>(a2, lane);
        if (lane >= 32) {
#pragma unroll
            for (int c = 0; c < 16; ++c) { sh.sOb[rr + BNR_LP * c] = a1[c]; sh.sOb[rr + BNR_LP * (16 + c)] = a2[c]; }
        }
    }
    __syncthreads();
    if (bad && tid == 0) bnr_flag_gfail(cd);
    // the swept own blocks; the diagonal blocks and block row b of panel a are needed by nobody later
    {
        const int r = tid & 31, c0 = tid >> 5;
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            const int c = c0 + 8 * mm;
            if (!only_b) E[(size_t)(R * BNR_NB + r) + ld * (size_t)(pa + c)] = sh.sOa[r + BNR_LP * c];
            E[(size_t)(R * BNR_NB + r) + ld * (size_t)(pb + c)] = sh.sOb[r + BNR_LP * c];
        }
    }
}

// Right-hand side: finishes the GEMVs of k_xpass and forms b = a1 - a3 (gibbs.jl:432-434):
//   a1 = (y - X W - mu_prev)/tau, a3 = X sz + z2  (note (X/tau) Delta_gamma1 = X sz).
// grid = n_pad/64 blocks of 256 threads: 64 rows x 4 partial groups; fixed summation order (deterministic).
template <class SRC>
__global__ __launch_bounds__(256) void k_rhs(const SRC chain_src, int s)
{
    const bnr_dev &cd = chain_src.get();
    __shared__ double sw[4][64], sa[4][64];
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    const double *prev = cd.trace + (size_t)P.prev * cd.rowlen;
    const double tau = cd.scal[SC_TAU], mu = prev[ROW_MU];
    const int n = cd.n;
    const size_t ld = cd.n_pad;
    const int il = threadIdx.x & 63, g = threadIdx.x >> 6, i = blockIdx.x * 64 + il;
    BNR_TL_IN(cd, TL_RHS, blockIdx.x == 0);
    double xw = 0.0, xs = 0.0;
    const int nb = cd.nblk_x;
    // (the partials of a row are added in ascending block order whatever the batch size: 16 + 16 loads in flight per round trip instead of 8 + 8 -- the kernel is
    // a chain of dependent round trips at the end of the scalar branch, which for a chain alone ends AFTER the factorization)
    int b = g;
    for (; b + 60 < nb; b += 64) {
        double w[16], a[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { w[u] = cd.PW[(size_t)(b + 4 * u) * ld + i]; a[u] = cd.PA[(size_t)(b + 4 * u) * ld + i]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) { xw += w[u]; xs += a[u]; }
    }
    for (; b + 12 < nb; b += 16) {
        double w[4], a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { w[u] = cd.PW[(size_t)(b + 4 * u) * ld + i]; a[u] = cd.PA[(size_t)(b + 4 * u) * ld + i]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { xw += w[u]; xs += a[u]; }
    }
    for (; b < nb; b += 4) { xw += cd.PW[(size_t)b * ld + i]; xs += cd.PA[(size_t)b * ld + i]; }
    sw[g][il] = xw; sa[g][il] = xs;
    __syncthreads();
    if (g == 0) {
        xw = (sw[0][il] + sw[1][il]) + (sw[2][il] + sw[3][il]);
        xs = (sa[0][il] + sa[1][il]) + (sa[2][il] + sa[3][il]);
        double z2 = (i < n) ? bnr_normal(cd.seed, P.it, SITE_G_Z2, (uint32_t)i, 0) : 0.0;
        double bb = (i < n) ? ((cd.y[i] - xw - mu) / tau - (xs + z2)) : 0.0;
        bnr_st8<BNR_ST_RHS>(cd.xw + i, xw); bnr_st8<BNR_ST_RHS>(cd.a3 + i, xs);          // a3 buffer keeps X sz (without z2)
        bnr_st8<BNR_ST_RHS>(cd.bw + i, bb);    // b, kept for the bookkeeping after the solve
    }
    BNR_TL_OUT(cd, TL_RHS);
}
// Solve with Y = L^-T (rows [n_pad, 2 n_pad) of E, upper triangular, column-major): a4 = Y (Y' b).
// The factorization itself never sees b, so the scalar branch of the sweep (tail, node, X W pass, k_rhs) only has to be
// finished here, not before the Cholesky.
// k_solve_w: w_c = sum_{r <= c} Y[r,c] b_r  -- one wavefront per column c (contiguous).  grid = n_pad/4 blocks of 256.
template <class SRC>
__global__ __launch_bounds__(256) void k_solve_w(const SRC chain_src)
{
    BNR_CRITICAL_PATH();
    const bnr_dev &cd = chain_src.get();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, np = cd.n_pad;
    const int c = blockIdx.x * 4 + wave;
    BNR_TL_IN(cd, TL_SOLVE_W, blockIdx.x == 0);
    const size_t ld = bnr_ldE(np);
    const double *col = cd.E + (size_t)np + ld * (size_t)c;
    const int rend = (c / BNR_NB + 1) * BNR_NB;            // entries below the diagonal block are exactly zero
    double acc = 0.0;
    for (int r = lane; r < rend; r += 64) acc = fma(col[r], cd.bw[r], acc);
    acc = wave_sum(acc);
    if (lane == 0) bnr_st8<BNR_ST_RHS>(cd.wv + c, acc);
    if (blockIdx.x == 0 && threadIdx.x == 0 && cd.counters[9]) {    // (see bnr_flag_gfail: the healthy path reads one word off the solve's own chain)
        cd.counters[9] = 0;
        atomicAdd((unsigned long long *)&cd.counters[3], 1ull); atomicAdd((unsigned long long *)&cd.counters[7], 1ull);
    }
    BNR_TL_OUT(cd, TL_SOLVE_W);
}
// k_solve_a4: a4_r = sum_{c >= block(r)} Y[r,c] w_c, then X gamma_new = X W + tau X sz + tau G a4, G a4 = b - a4
// (no third pass over X).  grid = nbk blocks (one per block row), 1024 threads = 32 rows x 32 column groups.
template <class SRC>
__global__ __launch_bounds__(1024) void k_solve_a4(const SRC chain_src)
{
    BNR_CRITICAL_PATH();
    const bnr_dev &cd = chain_src.get();
    extern __shared__ double shs[];                         // n_pad (w) + 32*33 partials
    double *swv = shs, *spart = shs + cd.n_pad;
    const int np = cd.n_pad, tid = threadIdx.x;
    const size_t ld = bnr_ldE(np);
    const int rb = blockIdx.x, rl = tid & 31, cg = tid >> 5;
    const int cstart = rb * BNR_NB;
    BNR_TL_IN(cd, TL_SOLVE_A4, rb == 0);
    for (int c = cstart + tid; c < np; c += 1024) swv[c] = cd.wv[c];
    __syncthreads();
    const double *yrow = cd.E + (size_t)(np + rb * BNR_NB + rl);
    double acc0 = 0.0, acc1 = 0.0;
    int c = cstart + cg;
    for (; c + 32 < np; c += 64) { acc0 = fma(yrow[ld * (size_t)c], swv[c], acc0); acc1 = fma(yrow[ld * (size_t)(c + 32)], swv[c + 32], acc1); }
    if (c < np) acc0 = fma(yrow[ld * (size_t)c], swv[c], acc0);
    spart[cg * 33 + rl] = acc0 + acc1;
    __syncthreads();
    if (tid < 32) {
        double a4 = 0.0;
#pragma unroll
        for (int g = 0; g < 32; ++g) a4 += spart[g * 33 + tid];
        const int r = rb * BNR_NB + tid;
        const double tau = cd.scal[SC_TAU], bb = cd.bw[r];
        bnr_st8<BNR_ST_RHS>(cd.a4 + r, a4);
        bnr_st8<BNR_ST_RHS>(cd.xg + r, (r < cd.n) ? (cd.xw[r] + tau * cd.a3[r] + tau * (bb - a4)) : 0.0);
    }
    BNR_TL_OUT(cd, TL_SOLVE_A4);
}

// ===================================================================================== k_backproj
// grid = nblk_bp blocks of 256 threads; block owns chunk_bp (<= 32) consecutive edges.
// flags bit0: compute gamma (else read from row); bit1: draw S (else read from row); bit2: partial sums.
//   gamma_e = W_e + tau (sz_e + S_prev,e x_e' a4)                           (gibbs.jl:435-436)
//   S_e ~ GIG(1/2, chi = (gamma_e - W_e)^2 / tau2, psi = theta_prev)         (gibbs.jl:454-458, gig.jl)
//   Psum[b][0] = sum_e S_e ; Psum[b][1+3r+c] = sum_e logpdf(Normal(W_c,e, sqrt(tau2 S_e)), gamma_e)  (gibbs.jl:603-605)
// Back-projection x_e' a4: one wavefront per column, two columns in flight, a4 in LDS, DPP wave reduction.
template <class SRC>
__global__ __launch_bounds__(256) void k_backproj(const SRC chain_src, int s, int flags, int nchains, int nslot)
{
    BNR_CRITICAL_PATH();
    // 1-D grid = round_up(blocks, 8) x chains, decoded like k_gram: the workgroups of the group's chains that read the same
    // 32 columns of X are neighbours on the same XCD and share them through its L2
    const int gid = blockIdx.x, gx = gid & 7, gr = gid >> 3;
    const int bid = (gr / nchains) * 8 + gx;               // this chain's block: 32 consecutive edges
    const bnr_dev &cd = chain_src.at(gr % nchains);
    if (bid >= cd.nblk_bp) return;
    extern __shared__ double sh[];          // n_pad (a4) + 64 (dots)
    double *sa = sh, *sdot = sh + cd.n_pad;
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    double *row = cd.trace + (size_t)P.row * cd.rowlen;
    const double *prev = cd.trace + (size_t)P.prev * cd.rowlen;
    const int R = cd.R, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int e0 = bid * cd.chunk_bp, ne = min(cd.chunk_bp, cd.q - e0);
    const size_t ld = cd.n_pad;
    const double tau2 = row[ROW_TAU2], tau = sqrt(tau2);
#ifdef BNR_STAMPS
#define BNR_BSTAMP(slot) do { if (tid == 0 && bid == 7) cd.dbg[320 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BNR_BSTAMP(slot) do { } while (0)
#endif
    BNR_BSTAMP(0);
#ifdef BNR_STAMPS
    if (tid == 0 && bid < 1800) cd.dbg[400 + 2 * bid] = __builtin_amdgcn_s_memrealtime();
#endif
    BNR_TL_IN(cd, (flags & 3) ? TL_BACKPROJ : TL_PSUM, bid == 0);
    // u[r,l] u[r,k] of this block's edges for the Lambda log-likelihoods at the end: requested now, so that the dependent
    // global loads (edge -> nodes -> u) are in flight behind the dot products instead of in front of the final sums
    __shared__ double sdr[BNR_RMAX * 33];
    if (flags & 4) {
        const double *un0 = row + cd.o_u;
        for (int idx = tid; idx < R * 32; idx += blockDim.x) {
            const int r = idx >> 5, ee = idx & 31;
            double v = 0.0;
            if (ee < ne) { const int l0 = cd.el[e0 + ee], k0 = cd.ek[e0 + ee]; v = un0[r + R * l0] * un0[r + R * k0]; }
            sdr[r * 33 + ee] = v;
        }
    }
    if (flags & 1) {
        for (int i = tid; i < cd.n_pad; i += blockDim.x) sa[i] = cd.a4[i];
        __syncthreads();
        // four columns of X per wave and trip where the host asks for it (flags bit 8; round 5: launches of one chain and large q -- one chain at the headline
        // shape 184.3 -> 182.5 us per sweep, config 5 x 8 chains 2 127 -> 2 103; the headline group of 8 stays at two: 380.5 vs 382.6): twice the loads in flight
        // per wave, half the dependent trips through memory -- every column's dot product is accumulated over the rows in the same order either way (bitwise
        // the same gamma)
        if (flags & 256)
        for (int t = wave; t < ne; t += 16) {
            const int t2 = t + 4, t3 = t + 8, t4 = t + 12;
            const size_t oc = (size_t)(e0 + t) * ld, od = (size_t)(e0 + (t2 < ne ? t2 : t)) * ld, oe = (size_t)(e0 + (t3 < ne ? t3 : t)) * ld, of = (size_t)(e0 + (t4 < ne ? t4 : t)) * ld;
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            if (cd.X8) {
                const unsigned char *xc = cd.X8 + oc, *xd = cd.X8 + od, *xe = cd.X8 + oe, *xf = cd.X8 + of;
#pragma unroll 4
                for (int i = lane; i < cd.n_pad; i += 64) { double av = sa[i]; acc0 = fma((double)xc[i], av, acc0); acc1 = fma((double)xd[i], av, acc1); acc2 = fma((double)xe[i], av, acc2); acc3 = fma((double)xf[i], av, acc3); }
            } else {
                const double *xc = cd.X + oc, *xd = cd.X + od, *xe = cd.X + oe, *xf = cd.X + of;
#pragma unroll 4
                for (int i = lane; i < cd.n_pad; i += 64) { double av = sa[i]; acc0 = fma(xc[i], av, acc0); acc1 = fma(xd[i], av, acc1); acc2 = fma(xe[i], av, acc2); acc3 = fma(xf[i], av, acc3); }
            }
            acc0 = wave_sum(acc0); acc1 = wave_sum(acc1); acc2 = wave_sum(acc2); acc3 = wave_sum(acc3);
            if (lane == 0) { sdot[t] = acc0; if (t2 < ne) sdot[t2] = acc1; if (t3 < ne) sdot[t3] = acc2; if (t4 < ne) sdot[t4] = acc3; }
        }
        else
        for (int t = wave; t < ne; t += 8) {
            const int t2 = t + 4;
            const size_t oc = (size_t)(e0 + t) * ld, od = (size_t)(e0 + (t2 < ne ? t2 : t)) * ld;
            double acc0 = 0.0, acc1 = 0.0;
            if (cd.X8) {
                const unsigned char *xc = cd.X8 + oc, *xd = cd.X8 + od;
#pragma unroll 4
                for (int i = lane; i < cd.n_pad; i += 64) { double av = sa[i]; acc0 = fma((double)xc[i], av, acc0); acc1 = fma((double)xd[i], av, acc1); }
            } else {
                const double *xc = cd.X + oc, *xd = cd.X + od;
#pragma unroll 4
                for (int i = lane; i < cd.n_pad; i += 64) { double av = sa[i]; acc0 = fma(xc[i], av, acc0); acc1 = fma(xd[i], av, acc1); }
            }
            acc0 = wave_sum(acc0); acc1 = wave_sum(acc1);
            if (lane == 0) { sdot[t] = acc0; if (t2 < ne) sdot[t2] = acc1; }
        }
    }
    __syncthreads();
    BNR_BSTAMP(1);
#ifdef BNR_STAMPS
    if (tid == 0 && bid < 1000) cd.dbg[2000 + bid] = __builtin_amdgcn_s_memrealtime();
#endif
    // update_D! (gibbs.jl:454-458): the rejection attempts of one GIG draw are independent given their counter, so several
    // attempts of every edge are evaluated side by side (half-wave = 32 edges x one attempt) and the first accepted one is
    // taken -- the same draw as the sequential loop of bnr_gig, in ~1 round instead of 3-5 dependent ones.  nslot (host) = 8
    // while the launch is latency-bound (few blocks: one chain at moderate q; all four waves), 2 when it is throughput-bound
    // (a lockstep group, or q large: wave 0 only) -- speculative attempts that are thrown away then cost what they save
    // (n=500, V=300: 58 vs 46 us per launch with 8 slots).
    // The two rejection samplers (ratio of uniforms / concave envelope: kinds 2 and 3 of bnr_gig_setup) are long, different instruction streams, and the 32
    // edges of a block usually need both: in ONE wave they run back to back.  The active waves are therefore split by kind -- the first half evaluates setup and
    // attempts of the kind-2 edges only, the second half those of the kind-3 edges -- and every edge is still drawn by exactly the arithmetic of bnr_gig.
    // nslot (host) = 2 x active waves: 4 (one wave per kind, two attempts per edge and round) or 8 (two waves per kind, four attempts).
    __shared__ double s_val[8][32];
    __shared__ int s_acc[8][32];
    int cap = 0;
    // nslot = 2 (throughput-bound launches: a lockstep group, large q): wave 0 alone draws, both kinds, two attempts per edge and round -- a second drawing
    // wave per block costs such a launch more than the shorter chain saves (8 chains: 391 vs 385 us per sweep; one chain: 180.0 vs 181.9 with the split)
    const bool split = nslot >= 4;
    const int nw = split ? nslot >> 1 : 1;                 // active waves
    const int nsk = split ? nw : 2;                        // attempt slots per edge and round: (nw / 2 waves of the edge's kind) x 2 half-waves
    // the wave that draws alone (and keeps the results) rotates with the block: the drawing waves of the blocks that share a CU then sit on different SIMDs
    const int dw = split ? 0 : (bid & 3);
    if (split ? wave >= nw : wave != dw) return;
    const int mykind = wave < (nw >> 1) ? 2 : 3, kw = split ? wave - (mykind == 3 ? (nw >> 1) : 0) : 0;
    const int el32 = lane & 31, slot = kw * 2 + (lane >> 5);
    const int e = e0 + el32;
    const bool act = el32 < ne, keeper = wave == dw && lane < 32;   // keeper: the lane that stores the edge's results and carries them into the sums
    double gam = 0.0, Snew = 1.0, W = 0.0;
    if (act) {
        W = cd.Wbuf[e];
        if (flags & 1) {
            double Sp = prev[cd.o_S + e];
            gam = tau * (cd.sz[e] + Sp * sdot[el32]) + W;
            if (keeper) bnr_st8<BNR_ST_BACKPROJ>(row + cd.o_gamma + e, gam);
        } else gam = row[cd.o_gamma + e];
    }
    if (flags & 2) {
        const double g = gam - W, chi = (g * g) / tau2, psi = prev[ROW_THETA];
        const int kind = act ? bnr_gig_kind(0.5, chi, psi) : 4;
        const bool loop = kind == 2 || kind == 3, mine = split ? kind == mykind : loop;
        bnr_gig_ctx gc;
        gc.kind = 4;
        if (mine || (keeper && act && !loop)) bnr_gig_setup(gc, 0.5, chi, psi);
        bool done = !loop;
        for (uint32_t base = 0; base < BNR_MAX_ATTEMPTS; base += (uint32_t)nsk) {
            double v = 0.0;
            const bool ok = mine && !done && bnr_gig_try(gc, cd.seed, P.it, (uint32_t)e, base + (uint32_t)slot, v);
            if (mine) { s_acc[slot][el32] = ok ? 1 : 0; s_val[slot][el32] = v; }       // (an edge's slots are written by the waves of its kind only)
            // (one drawing wave: its two half-waves meet through LDS with wave-level synchronisation only -- the other waves of the block have left, and a block-wide
            // vote must not be asked of a block whose wave 0 is gone)
            if (split) __syncthreads(); else bnr_wsync();
            if (!done) {
#pragma unroll
                for (int a = 7; a >= 0; --a) if (a < nsk && s_acc[a][el32]) { Snew = s_val[a][el32]; done = true; }   // lowest accepted attempt wins
            }
            if (split) { if (!__syncthreads_or(done ? 0 : 1)) break; }
            else { bnr_wsync(); if (__ballot(!done) == 0ull) break; }
        }
        if (split ? __syncthreads_or(done ? 0 : 1) != 0 : __ballot(!done) != 0ull) {   // attempt cap, as bnr_gig: the fallback value comes from the wave that holds the setup
            if (mine && !done && slot == 0) s_val[0][el32] = gc.alpha * gc.xm;
            if (split) __syncthreads(); else bnr_wsync();
            if (!done) { cap = 1; Snew = s_val[0][el32]; }
        }
        if (keeper && act && !loop) Snew = bnr_gig_degenerate(gc, cd.seed, chi, psi, P.it, (uint32_t)e, &cap);
        if (keeper && act) bnr_st8<BNR_ST_BACKPROJ>(row + cd.o_S + e, Snew);
    } else if (act) Snew = row[cd.o_S + e];
    if (wave != dw) return;
    BNR_BSTAMP(2);
    if (!(flags & 4)) { if (cap && lane < 32) atomicAdd((unsigned long long *)&cd.counters[2], 1ull); return; }
    double *ps = cd.Psum + (size_t)bid * (1 + 3 * R);
    // per-edge terms go through LDS ([term][lane], lane-contiguous) and lane j then sums term j over the 32 edges in a
    // fixed order: one pass instead of 3R+1 wave reductions
    double *st = sh;                                  // reuse the a4 staging area: (3R + 1) x 33 doubles <= n_pad + 64
    const double *lamp = prev + cd.o_lam;
    const double sd = sqrt(tau2 * Snew), lsd = log(sd) + 0.5 * log(2.0 * BNR_PI);
    if (lane < 32) {
        st[lane] = act ? Snew : 0.0;
        for (int r = 0; r < R; ++r) {
            double dr = sdr[r * 33 + lane];
            double lr = lamp[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double Wc = W + (bnr_lambda_value(c) - lr) * dr;
                double zz = (gam - Wc) / sd;
                st[(1 + 3 * r + c) * 33 + lane] = act ? (-0.5 * zz * zz - lsd) : 0.0;
            }
        }
    }
    bnr_wsync();
    for (int j = lane; j < 1 + 3 * R; j += 64) {
        double acc = 0.0;
#pragma unroll 8
        for (int e2 = 0; e2 < 32; ++e2) acc += st[j * 33 + e2];
        bnr_st8<BNR_ST_BACKPROJ>(ps + j, acc);
    }
    BNR_BSTAMP(3);
#ifdef BNR_STAMPS
    if (lane == 0 && bid < 1800) cd.dbg[401 + 2 * bid] = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) atomicMax((unsigned long long *)&cd.dbg[4000 + 4 * ((flags & 3) ? TL_BACKPROJ : TL_PSUM) + 2], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
    if (cap && lane < 32) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
}

// ===================================================================================== k_tail
// One block of BNR_TAIL_THREADS threads per chain.  mask bits: 1 theta, 2 Delta, 4 M, 8 mu, 16 Lambda, 32 pi, 64 carried sums (rr, sig_q for
// the next tau2), 128 ring wrap copy, 256 inv(M)/logdet M for the next k_node, 512 pre-draw the next tau2.
// When a bit is clear the value already in `row` is kept.
// xg_src: 0 = cd.xg (from k_solve_gemv); 1 = sum of the PG partials (X*gamma by k_xpass bit2).
// Independent scalar draws sit on different wavefronts so that their long scalar sampler code runs concurrently.
// Round 6: in a sweep the launch has TWO workgroups per chain (grid.x = 2): workgroup 0 runs the bits 1 | 8 | 16 | 32 | 64 | 128 | 512 -- what needs the back-projection's
// output --, workgroup 1 Delta, M and inv(M) (bits 2, 4, 256: bnr_tail_a above) beside it.  With grid.x = 1 (the hooks, a loaded or initialised row) bnr_tail_a runs here first.

#define BNR_TAIL_U_LDS 15360     // doubles of u (R x V) that k_tail stages in LDS (120 KB); a larger u is read from the trace row (same values, same order of operations)
#define BNR_TAIL_THREADS 512   // 8 wavefronts: the seven role waves of phase 3 + one; two per SIMD, so the kernel may use 256 vector registers (no spills: with
                               // 1024 threads it had 128 and spilled) and fits a CU beside other resident workgroups instead of needing an empty one.
                               // NOT a tunable: the block-wide reductions of k_tail (sum of squared residuals, sig_q, the mu / tau2 sums) stride by the thread
                               // count, so another value changes their last bits (the tables then differ from this build's by rounding; round 3's 1024-thread
                               // build differs from this one in exactly that way -- within 1e-9 of each other and of the CPU restatement the tests check against, not bit for bit)
static_assert(BNR_TAIL_THREADS == 512, "k_tail's reductions depend on its thread count: see the note above");
// (ULDS: u staged in LDS -- the kernel of rounds 1-5 -- or read from the table row (R V beyond BNR_TAIL_U_LDS): two instantiations, so that the common one carries neither the
// test nor the second copy of the loops)
template <class SRC, bool ULDS = true>
__global__ __launch_bounds__(BNR_TAIL_THREADS) void k_tail(const SRC chain_src, int s, int mask, int xg_src)
{
    const bnr_dev &cd = chain_src.get();
    extern __shared__ double su_lds[];           // R x V: u of this row (staged once for the q pass) -- where it fits the LDS budget (BNR_TAIL_U_LDS), else read from the row --, then bnr_tail_a's 4 R^2 + 8 doubles
    __shared__ double sred[3 * 16];
    __shared__ double sll[3 * BNR_RMAX + 1], slam[BNR_RMAX], spi[3 * BNR_RMAX], spow[BNR_RMAX];
    __shared__ double sval[8];
    __shared__ int sflag[2];
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    if (P.wrap & 2) return;                      // placeholder entry in front of the first sweep of a run
    // (the row pointers are the same for the whole workgroup: pinned to scalar registers -- as vector values they lived through the whole
    // kernel, and the register allocator spilled them and the thread id around the inlined samplers: 32 bytes of scratch per lane in round 3)
    double *row = bnr_sgpr_global(cd.trace + (size_t)P.row * cd.rowlen);
    const double *prev = bnr_sgpr_global((const double *)(cd.trace + (size_t)P.prev * cd.rowlen));
    const int R = cd.R, V = cd.V, q = cd.q, n = cd.n, tid = threadIdx.x, wave = bnr_sgpr((int)(threadIdx.x >> 6)), lane = tid & 63, nw = blockDim.x >> 6;
    const double tau2 = bnr_sgpr_f64(row[ROW_TAU2]);
    int cap = 0;
#ifdef BNR_STAMPS
#define BNR_TSTAMP(slot) do { if (tid == 0) cd.dbg[256 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define BNR_TSTAMP(slot) do { } while (0)
#endif
    BNR_TSTAMP(0);
    if (gridDim.x == 2) {
        // a sweep's launch: workgroup 1 of the chain does Delta, M, inv(M) (what needs only k_node's output), workgroup 0 the rest, side by side
        if (blockIdx.x == 1) { BNR_TL_IN(cd, TL_TAIL_A, true); if (mask & BNR_TAIL_EARLY) bnr_tail_a(cd, P, mask, su_lds, tid, (mask & 128) != 0, ULDS ? su_lds + bnr_tail_a_lds_doubles(R) : nullptr); BNR_TL_OUT(cd, TL_TAIL_A); return; }
        BNR_TL_IN(cd, TL_TAIL, true);
        mask &= ~BNR_TAIL_EARLY;
    } else if (mask & BNR_TAIL_EARLY) {            // one workgroup for everything (hooks, a loaded or initialised row): the early part first
        bnr_tail_a(cd, P, mask, su_lds + (ULDS ? (size_t)R * V : 0), tid, false, ULDS ? su_lds : nullptr);     // (u staged where the late part will stage it again)
        if (!(mask & ~BNR_TAIL_EARLY)) return;
        __syncthreads();
    }
    if (tid < R) slam[tid] = row[cd.o_lam + tid];
    if (tid >= BNR_TAIL_THREADS - 64 && tid - (BNR_TAIL_THREADS - 64) < R) spow[tid - (BNR_TAIL_THREADS - 64)] = pow((double)(tid - (BNR_TAIL_THREADS - 64) + 1), cd.eta);     // (r + 1)^eta of pi's Dirichlet parameters: a constant of the chain, evaluated beside the reductions instead of in front of pi's draws
    if (tid == 0) { sval[1] = row[ROW_MU]; sflag[0] = 0; sflag[1] = 0; }
    constexpr bool u_lds = ULDS;
    if (u_lds) for (int i = tid; i < R * V; i += blockDim.x) su_lds[i] = row[cd.o_u + i];
    const double *su_row = row + cd.o_u;          // (the two sources stay two pointers with their own address spaces: one pointer selected at run time is a generic one, and the
                                                  // q pass below then reads u by flat loads -- config 5, one chain: 414 instead of 396 us per sweep)

    // ---- phase 1: reductions.  Psum partials (32 lanes per output, fixed order); X gamma from the PG partials
    if (mask & (1 | 16)) {
        const int nout = 1 + 3 * R, j = tid >> 5, t = tid & 31, ngrp = blockDim.x >> 5;
        for (int jj = j; jj < nout; jj += ngrp) {
            double a0 = 0.0, a1 = 0.0;
            int b = t;
            for (; b + 32 < cd.nblk_bp; b += 64) { a0 += cd.Psum[(size_t)b * nout + jj]; a1 += cd.Psum[(size_t)(b + 32) * nout + jj]; }
            if (b < cd.nblk_bp) a0 += cd.Psum[(size_t)b * nout + jj];
            double a = half_wave_sum(a0 + a1);
            if (t == 0) sll[jj] = a;             // sll[0] = sum S, sll[1 + 3r + c] = log-likelihood sums
        }
    }
    if ((mask & (8 | 64)) && (xg_src & 255) == 1) {
        for (int i = tid; i < cd.n_pad; i += blockDim.x) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            int b = 0;
            for (; b + 3 < cd.nblk_x; b += 4) {
                a0 += cd.PG[(size_t)b * cd.n_pad + i]; a1 += cd.PG[(size_t)(b + 1) * cd.n_pad + i];
                a2 += cd.PG[(size_t)(b + 2) * cd.n_pad + i]; a3 += cd.PG[(size_t)(b + 3) * cd.n_pad + i];
            }
            for (; b < cd.nblk_x; ++b) a0 += cd.PG[(size_t)b * cd.n_pad + i];
            cd.xg[i] = (a0 + a1) + (a2 + a3);
        }
    }
    __syncthreads();
    BNR_TSTAMP(1);
    // sum (y - X gamma): block reduction (per-thread partial sums stride by the thread count, then the waves in order)
    double sres = 0.0;
    if (mask & 8) {
        for (int i = tid; i < n; i += blockDim.x) sres += cd.y[i] - cd.xg[i];
        sres = wave_sum(sres);
        if (lane == 0) sred[32 + wave] = sres;
    }
    __syncthreads();
    if (mask & 8) { sres = 0.0; for (int w = 0; w < nw; ++w) sres += sred[32 + w]; }
    // (the same in every lane from here on: scalar registers -- the samplers inlined below need the vector ones)
    sres = bnr_sgpr_f64(sres);
    BNR_TSTAMP(2);
    // ---- phase 3 (round 6): two chains of work side by side, no block barrier between the draws and the pass over the edges.
    //   every wavefront: mu (one normal) and lambda (R categorical draws) evaluated REDUNDANTLY -- the same counters, the same values in every wave -- so that
    //     the pass over the edges for the next tau2's sums, which needs both, starts without waiting for anybody (wave 0 writes them to the row);
    //   wavefront 0:     the Gamma variates of theta (lane 0) and of the NEXT tau2 (lane 1: it does not depend on the sums it will scale) in one
    //     divergence-free call, then pi;
    //   wavefronts 1..7: rr and sig_q (the partition of rows and edges over 448 threads is what rounds 4-5 had: the same sums bit for bit).
    double mu = sval[1];
    if (mask & 8) {                                                               // mu (gibbs.jl:565-570)
        mu = sres / n + sqrt(tau2 / n) * bnr_normal(cd.seed, P.it, SITE_MU, 0, 0);
        if (tid == 0) row[ROW_MU] = mu;
    }
    if ((mask & 16) && lane < R) {                                                // Lambda (gibbs.jl:586-636)
        int r = lane;
        double l0 = sll[1 + 3 * r], l1 = sll[2 + 3 * r], l2 = sll[3 + 3 * r];
        double pmax = fmax(l0, fmax(l1, l2));
        double w0 = prev[cd.o_pi + r] * exp(l0 - pmax), w1 = prev[cd.o_pi + r + R] * exp(l1 - pmax), w2 = prev[cd.o_pi + r + 2 * R] * exp(l2 - pmax);
        double ua, ub;
        bnr_draw2(cd.seed, P.it, SITE_LAMBDA, (uint32_t)r, 0, ua, ub);
        double lv = bnr_lambda_value(bnr_categorical3(w0, w1, w2, ua));
        slam[r] = lv;                                                             // (every wave stores the same values)
        if (wave == 0) row[cd.o_lam + r] = lv;
    }
    bnr_wsync();
    double g_tau = 1.0;
    if (wave == 0 && 3 * R + 2 <= 64) {
        // ONE pass of the Gamma sampler for everything wave 0 draws: lanes 0 .. 3R-1 the variates of pi (gibbs.jl:620-636), lane 3R theta's (476-479), lane 3R+1 the NEXT
        // tau2's (267-277) -- the same counters and shapes as one after the other (bitwise the same values), one walk through the sampler's code instead of two
        const int t = lane;
        const bool is_pi = (mask & 32) && t < 3 * R, th = t == 3 * R && (mask & 1), tn = t == 3 * R + 1 && (mask & 512);
        double shp = 1.0; uint32_t it_ = P.it, site_ = SITE_PI, el_ = 0;
        if (is_pi) {
            const int r = t / 3, c = t % 3;
            const double lam = slam[r], base = spow[r];
            if (lam == 1.0) shp = (c == 0) ? base : (c == 1 ? 2.0 : 1.0);
            else if (lam == 0.0) shp = (c == 0) ? base + 1.0 : 1.0;
            else shp = (c == 0) ? base : (c == 1 ? 1.0 : 2.0);
            el_ = (uint32_t)(3 * r + c);
        } else if (th) { shp = cd.zeta + (V * (V + 1)) / 2.0; site_ = SITE_THETA; }
        else if (tn) { shp = (n / 2.0) + (V * (V + 1) / 4.0); it_ = P.it + 1u; site_ = SITE_TAU2; }
        double g = 1.0;
        if (is_pi || th || tn) g = bnr_gamma(cd.seed, shp, it_, site_, el_, &cap);
        if (is_pi) spi[t] = g;
        if (th) row[ROW_THETA] = g * (2.0 / (2.0 * cd.iota + sll[0]));
        g_tau = bnr_readlane_u(g, 3 * R + 1);
        bnr_wsync();
        if ((mask & 32) && t < 3 * R) { const int r = t / 3, c = t % 3; row[cd.o_pi + r + R * c] = spi[t] / (spi[3 * r] + spi[3 * r + 1] + spi[3 * r + 2]); }
    } else
    if (wave == 0) {
        if (mask & (1 | 512)) {                                                   // theta (gibbs.jl:476-479) and the variate of the next tau2 (gibbs.jl:267-277)
            const bool th = lane == 0 && (mask & 1), tn = lane == 1 && (mask & 512);
            double g = 1.0;
            if (th || tn) g = bnr_gamma(cd.seed, th ? cd.zeta + (V * (V + 1)) / 2.0 : (n / 2.0) + (V * (V + 1) / 4.0), th ? P.it : P.it + 1u, th ? SITE_THETA : SITE_TAU2, 0, &cap);
            if (th) row[ROW_THETA] = g * (2.0 / (2.0 * cd.iota + sll[0]));
            g_tau = bnr_readlane_c(g, 1);
        }
        if (mask & 32) {                                                          // pi (gibbs.jl:620-636)
            for (int t0 = 0; t0 < 3 * R; t0 += 64) {
                int t = t0 + lane;
                if (t < 3 * R) {
                    int r = t / 3, c = t % 3;
                    double lam = slam[r];
                    double base = spow[r];
                    double alpha;
                    if (lam == 1.0) alpha = (c == 0) ? base : (c == 1 ? 2.0 : 1.0);
                    else if (lam == 0.0) alpha = (c == 0) ? base + 1.0 : 1.0;
                    else alpha = (c == 0) ? base : (c == 1 ? 1.0 : 2.0);
                    spi[t] = bnr_gamma(cd.seed, alpha, P.it, SITE_PI, (uint32_t)(3 * r + c), &cap);
                }
            }
            bnr_wsync();
            for (int t0 = 0; t0 < 3 * R; t0 += 64) {
                int t = t0 + lane;
                if (t < 3 * R) { int r = t / 3, c = t % 3; row[cd.o_pi + r + R * c] = spi[t] / (spi[3 * r] + spi[3 * r + 1] + spi[3 * r + 2]); }
            }
        }
    }
    BNR_TSTAMP(3);
    BNR_TSTAMP(4);
    // ---- carried sums for the next update_tau2! (gibbs.jl:270-273): rr = |y - mu - X gamma|^2,
    //      sig_q = sum_e ((gamma_e - W(u,lam)_e)^2 / 2) / S_e  with the NEW lambda; optionally the next tau2
    if (mask & 64) {
        double racc = 0.0, qacc = 0.0;
        if (wave != 0) {                          // (wavefront 0 stays out: the partition of the edges over 448 threads fixes the sums' last bits)
            const int t = tid - 64, nt = blockDim.x - 64;
            for (int i = t; i < n; i += nt) { double rv = cd.y[i] - mu - cd.xg[i]; racc += rv * rv; }
            // four edges of a thread in flight per trip (their index / gamma / S loads are independent; one edge per trip is one round trip to memory per edge:
            // 100 trips at q = 45 150 made this pass 100 of k_tail's 152 us there, and 11 trips at q = 5 050 were a third of the kernel once nothing hid them),
            // the terms added in the same order as one by one
#define BNR_TAIL_QPASS(SU)                                                                                                     \
            {                                                                                                                  \
                int e = t;                                                                                                     \
                for (; e + 3 * nt < q; e += 4 * nt) {                                                                          \
                    int l4[4], k4[4]; double g4[4], s4[4];                                                                     \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j) { const int ej = e + j * nt; l4[j] = cd.el[ej]; k4[j] = cd.ek[ej]; g4[j] = row[cd.o_gamma + ej]; s4[j] = row[cd.o_S + ej]; } \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j) { const double g = g4[j] - edge_W(SU, slam, R, l4[j], k4[j]); qacc += ((g * g) / 2.0) / s4[j]; } \
                }                                                                                                              \
                {                                    /* the last, ragged trip: up to three edges, in flight together as well */  \
                    int l4[3], k4[3]; double g4[3], s4[3];                                                                     \
                    _Pragma("unroll") for (int j = 0; j < 3; ++j) { const int ej = e + j * nt, ec = ej < q ? ej : 0; l4[j] = cd.el[ec]; k4[j] = cd.ek[ec]; g4[j] = row[cd.o_gamma + ec]; s4[j] = row[cd.o_S + ec]; } \
                    _Pragma("unroll") for (int j = 0; j < 3; ++j) if (e + j * nt < q) { const double g = g4[j] - edge_W(SU, slam, R, l4[j], k4[j]); qacc += ((g * g) / 2.0) / s4[j]; } \
                }                                                                                                              \
            }
            if (u_lds) BNR_TAIL_QPASS(su_lds)
            else BNR_TAIL_QPASS(su_row)
        }
        racc = wave_sum(racc); qacc = wave_sum(qacc);
        __syncthreads();
        if (lane == 0) { sred[wave] = racc; sred[16 + wave] = qacc; }
        __syncthreads();
        BNR_TSTAMP(5);
        if (tid == 0) {
            racc = 0.0; qacc = 0.0;
            for (int w = 0; w < nw; ++w) { racc += sred[w]; qacc += sred[16 + w]; }
            cd.scal[SC_RR] = racc; cd.scal[SC_SIGQ] = qacc;
            if (mask & 512) {
                double sigma = racc / 2.0 + qacc;
                cd.scal[SC_TAU2N] = sigma / g_tau;
                cd.scal[SC_TAU2N_IT] = (double)(P.it + 1u);
            } else cd.scal[SC_TAU2N_IT] = -1.0;
        }
    }
    // ---- purge ring (gibbs.jl:857-860): copy_table!(state, 1, j)
    if ((mask & 128) && (P.wrap & 1)) {
        __syncthreads();
        double *dst = cd.trace;
        // (two workgroups per chain: Delta and M of this row are being written by workgroup 1 right now -- it writes them to the copies itself, they are left out here)
        const bool two = gridDim.x == 2;
        const int m0 = cd.o_M, m1 = cd.o_M + R * R;
        if (row != dst) for (int i = tid; i < cd.rowlen; i += blockDim.x) if (!two || !(i == ROW_DELTA || (i >= m0 && i < m1))) dst[i] = row[i];
        if (P.wrap & 4) {                        // purge_burn == 1: the state sits in the hidden scratch row, rows 1 AND 2 get it
            double *dst2 = cd.trace + cd.rowlen;
            for (int i = tid; i < cd.rowlen; i += blockDim.x) if (!two || !(i == ROW_DELTA || (i >= m0 && i < m1))) dst2[i] = row[i];
        }
    }
    BNR_TSTAMP(6);
    if (gridDim.x == 2) BNR_TL_OUT(cd, TL_TAIL);
    if (cap) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
}

// advances the plan base after a batch of sweeps (last node of the captured graph)
__global__ void k_advance(const bnr_dev *cds, int by) { if (threadIdx.x == 0) ((int *)cds[blockIdx.x].pbase)[0] += by; }   // grid = chains
// the members' plans of a run call arrive in ONE staged copy and are handed out on the device (a copy per member cost ~20 us each on the stream)
__global__ void k_scatter_plans(const bnr_dev *cds, const bnr_plan_entry *staged, int stride, int count)
{
    bnr_plan_entry *dst = (bnr_plan_entry *)cds[blockIdx.x].plan;
    const bnr_plan_entry *src = staged + (size_t)blockIdx.x * stride;
    for (int e = threadIdx.x; e < count; e += blockDim.x) dst[e] = src[e];
}
__global__ void k_nop() { }
// the event counters of all members of a launch into one block (one device -> host copy per run call); grid = chains, 16 threads
__global__ void k_gather_counters(const bnr_dev *cds, long long *out) { out[blockIdx.x * 16 + threadIdx.x] = cds[blockIdx.x].counters[threadIdx.x]; }
__global__ void k_setbase(const bnr_dev *cds, int v) { if (threadIdx.x == 0) ((int *)cds[blockIdx.x].pbase)[0] = v; }

// ===================================================================================== k_init_prior
// initialize_variables! (gibbs.jl:191-224) into row 0.  One block of 256 threads.
__global__ __launch_bounds__(256) void k_init_prior(bnr_dev cd)
{
    __shared__ double sT[3 * BNR_RMAX], sA[BNR_RMAX * BNR_RMAX], sTi[BNR_RMAX * BNR_RMAX], slam[BNR_RMAX];
    double *row = cd.trace;
    const int R = cd.R, V = cd.V, q = cd.q, tid = threadIdx.x;
    const uint32_t it = 1;
    int cap = 0;
    double eta = cd.eta;
    if (eta <= 1.0) eta = 1.01;                       // local-only reset (gibbs.jl:193-196)
    if (tid == 0) { row[ROW_THETA] = 0.5; row[ROW_DELTA] = 0.5; row[ROW_MU] = 1.0; row[ROW_TAU2] = 1.0; }
    for (int e = tid; e < q; e += blockDim.x) {
        double ua, ub;
        bnr_draw2(cd.seed, it, SITE_INIT_S, (uint32_t)e, 0, ua, ub);
        row[cd.o_S + e] = -(0.5 / 2.0) * log(ua);
    }
    if (tid < 3 * R) {
        int r = tid / 3, c = tid % 3;
        double alpha = (c == 0) ? pow((double)(r + 1), eta) : 1.0;
        sT[tid] = bnr_gamma(cd.seed, alpha, it, SITE_INIT_PI, (uint32_t)(3 * r + c), &cap);
    }
    __syncthreads();
    if (tid < 3 * R) {
        int r = tid / 3, c = tid % 3;
        row[cd.o_pi + r + R * c] = sT[tid] / (sT[3 * r] + sT[3 * r + 1] + sT[3 * r + 2]);
    }
    __syncthreads();
    if (tid < R) {
        double ua, ub;
        bnr_draw2(cd.seed, it, SITE_INIT_LAM, (uint32_t)tid, 0, ua, ub);
        double lv = bnr_lambda_value(bnr_categorical3(row[cd.o_pi + tid], row[cd.o_pi + tid + R], row[cd.o_pi + tid + 2 * R], ua));
        row[cd.o_lam + tid] = lv; slam[tid] = lv;
    }
    for (int v = tid; v < V; v += blockDim.x) {
        double ua, ub;
        bnr_draw2(cd.seed, it, SITE_INIT_XI, (uint32_t)v, 0, ua, ub);
        row[cd.o_xi + v] = (ua <= 0.5) ? 1.0 : 0.0;
    }
    // M ~ InverseWishart(nu, I): M = T' T... (C = I): B = T', M = B B' with T = A^-1
    for (int idx = tid; idx < R * R; idx += blockDim.x) {
        int i = idx % R, j = idx / R;
        double v = 0.0;
        if (i == j) v = sqrt(2.0 * bnr_gamma(cd.seed, 0.5 * (cd.nu - j), it, SITE_INIT_M_CHI, (uint32_t)j, &cap));
        else if (i > j) v = bnr_normal(cd.seed, it, SITE_INIT_M_N, (uint32_t)(i * R + j), 0);
        sA[idx] = v;
    }
    __syncthreads();
    if (tid < R) {
        int j = tid;
        for (int i = 0; i < R; ++i) {
            double v = 0.0;
            if (i == j) v = 1.0 / sA[j + R * j];
            else if (i > j) {
                double sacc = 0.0;
                for (int k = j; k < i; ++k) sacc += sA[i + R * k] * sTi[k + R * j];
                v = -sacc / sA[i + R * i];
            }
            sTi[i + R * j] = v;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < R * R; idx += blockDim.x) {
        int a = idx % R, b = idx / R;       // B[a,k] = T[k,a] ; M[a,b] = sum_k T[k,a] T[k,b]
        double sacc = 0.0;
        for (int k = 0; k < R; ++k) sacc += sTi[k + R * a] * sTi[k + R * b];
        row[cd.o_M + idx] = sacc;
    }
    for (int idx = tid; idx < R * V; idx += blockDim.x) {
        int r = idx % R, v = idx / R;
        row[cd.o_u + idx] = bnr_normal(cd.seed, it, SITE_INIT_U, (uint32_t)(v * R + r), 0);
    }
    __syncthreads();
    for (int e = tid; e < q; e += blockDim.x) {
        double W = edge_W(row + cd.o_u, slam, R, cd.el[e], cd.ek[e]);
        row[cd.o_gamma + e] = W + sqrt(1.0 * row[cd.o_S + e]) * bnr_normal(cd.seed, it, SITE_INIT_GAMMA, (uint32_t)e, 0);
    }
    if (cap) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
}

// ===================================================================================== model matrix from the caller's element type
// X[i, e] (f64, leading dimension n_pad) from the host layout uploaded as it is: either the n x q matrix X_new of
// generate_samples! in its own element type (gibbs.jl:917: Matrix{eltype(T)} -- Bool for adjacency data), or the n adjacency
// matrices themselves (V x V column-major, one after the other): setup_X! on the device (gibbs.jl:239-247), row i =
// lower_triangle(A_i), i.e. edge e <-> (l >= k) reads A_i[l, k] (utils.jl:50-55).  grid = (ceil(n/64), edges), 64 threads.
template <typename T>
__global__ void k_x_convert(const T *raw, bool from_matrices, int n, int V, int q, int n_pad, const int *ek, const int *el, double *X, unsigned char *X8, int *not_bytes)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    for (int e = blockIdx.y; e < q; e += gridDim.y) {
        const T v = from_matrices ? raw[(size_t)i * V * V + (size_t)el[e] + (size_t)V * ek[e]] : raw[(size_t)i + (size_t)n * e];
        X[(size_t)i + (size_t)n_pad * e] = (double)v;
        if (X8) {
            const unsigned char b = (unsigned char)v;
            if ((T)b != v) bad = true;                            // not a whole number in 0..255: the byte image is dropped by the host
            X8[(size_t)i + (size_t)n_pad * e] = b;
        }
    }
    if (bad) *not_bytes = 1;
}

// ===================================================================================== table transposes
// out[r + ldo*d] = trace[(first + r)*rowlen + off + d]   (device row-major -> reference iteration-fastest; ldo = nrows for one chain's window,
// the pooled draw count where the windows of several chains lie side by side in a column)
__global__ void k_fetch_cols(const double *trace, int rowlen, int off, int ncols, int first, int nrows, double *out, long long ldo)
{
    __shared__ double tile[32][33];
    int d0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int r = r0 + j, d = d0 + threadIdx.x;
        tile[j][threadIdx.x] = (r < nrows && d < ncols) ? trace[(size_t)(first + r) * rowlen + off + d] : 0.0;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int d = d0 + j, r = r0 + threadIdx.x;
        if (r < nrows && d < ncols) out[(size_t)r + (size_t)ldo * d] = tile[threadIdx.x][j];
    }
}
__global__ void k_load_cols(double *trace, int rowlen, int off, int ncols, int first, int nrows, const double *in)
{
    __shared__ double tile[32][33];
    int d0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int d = d0 + j, r = r0 + threadIdx.x;
        tile[j][threadIdx.x] = (r < nrows && d < ncols) ? in[(size_t)r + (size_t)nrows * d] : 0.0;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        int r = r0 + j, d = d0 + threadIdx.x;
        if (r < nrows && d < ncols) trace[(size_t)(first + r) * rowlen + off + d] = tile[threadIdx.x][j];
    }
}

// ===================================================================================== k_rhat_stats
// First half of rhat() (convergence.jl:4-65) for one chain: per parameter p in [gamma(q) | xi(V)], mean and corrected
// variance of the first and the last floor(nsamp/2) of rows first..first+nsamp-1.  out: [mean0 | var0 | mean1 | var1] x np
__global__ void k_rhat_stats(bnr_dev cd, int first, int nsamp, double *out)
{
    const int np = cd.q + cd.V;
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int off = (p < cd.q) ? cd.o_gamma + p : cd.o_xi + (p - cd.q);
    const int h = nsamp / 2;
    for (int half = 0; half < 2; ++half) {
        int r0 = first + (half == 0 ? 0 : nsamp - h);
        double sacc = 0.0;
        for (int r = 0; r < h; ++r) sacc += cd.trace[(size_t)(r0 + r) * cd.rowlen + off];
        double mean = sacc / h, v = 0.0;
        for (int r = 0; r < h; ++r) { double d = cd.trace[(size_t)(r0 + r) * cd.rowlen + off] - mean; v += d * d; }
        out[(size_t)(2 * half) * np + p] = mean;
        out[(size_t)(2 * half + 1) * np + p] = v / (h - 1);
    }
}

// ===================================================================================== k_summary
// Device side of Summary(results) (gibbs.jl:1214-1250): per edge e the posterior mean of gamma_e over the sampled rows and
// two order statistics (the k_lo-th and k_hi-th smallest, 1-based: the reference indexes the sorted column at
// round(nsamp*lower) and round(nsamp*upper)); per node the mean of xi.  Only 3q + V numbers leave the GPU instead of the
// nsamp x q gamma trace.
// `buf` holds the window transposed by k_fetch_cols: column p (gamma_0..gamma_{q-1}, then xi_0..xi_{V-1}) is contiguous,
// nsamp doubles.  One workgroup of 256 threads per column.  Exact selection by MSD radix counting on the order-preserving
// 64-bit image of the doubles: 6 passes (11,11,11,11,11,9 bits) of a 2048-bin LDS histogram per statistic.
__global__ __launch_bounds__(256) void k_summary(const double *buf, int nsamp, int q, int k_lo, int k_hi, double *mean, double *lo, double *hi)
{
    __shared__ unsigned int hist[2048];
    __shared__ unsigned int part[256];
    __shared__ double red[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_k;
    const int p = blockIdx.x, tid = threadIdx.x;
    const double *col = buf + (size_t)p * nsamp;
    // mean: fixed summation order (thread-strided partial sums, then a tree)
    double acc = 0.0;
    for (int i = tid; i < nsamp; i += 256) acc += col[i];
    red[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    if (tid == 0) mean[p] = red[0] / nsamp;
    if (p >= q) return;                                  // xi columns: mean only
    for (int stat = 0; stat < 2; ++stat) {
        if (tid == 0) { s_prefix = 0ull; s_k = stat == 0 ? k_lo : k_hi; }
        __syncthreads();
        int shift = 64;
        for (int pass = 0; pass < 6; ++pass) {
            const int bits = pass < 5 ? 11 : 9;
            shift -= bits;
            const unsigned long long prefix = s_prefix;
            const unsigned long long himask = shift + bits >= 64 ? 0ull : (~0ull << (shift + bits));
            for (int b = tid; b < 2048; b += 256) hist[b] = 0u;
            __syncthreads();
            for (int i = tid; i < nsamp; i += 256) {
                unsigned long long key = bnr_key_of(col[i]);
                if ((key & himask) == prefix) atomicAdd(&hist[(unsigned int)((key >> shift) & ((1u << bits) - 1u))], 1u);
            }
            __syncthreads();
            // find the bin that holds the s_k-th smallest of the surviving elements: 8 bins per thread, scan over threads
            unsigned int mysum = 0;
            for (int b = 0; b < 8; ++b) mysum += hist[tid * 8 + b];
            part[tid] = mysum;
            __syncthreads();
            for (int off = 1; off < 256; off <<= 1) {
                unsigned int v = tid >= off ? part[tid - off] : 0u;
                __syncthreads();
                part[tid] += v;
                __syncthreads();
            }
            const unsigned int incl = part[tid], excl = incl - mysum;
            const int k = s_k;
            __syncthreads();
            if ((unsigned int)k > excl && (unsigned int)k <= incl) {       // exactly one thread
                unsigned int run = excl;
                for (int b = 0; b < 8; ++b) {
                    unsigned int cnt = hist[tid * 8 + b];
                    if ((unsigned int)k <= run + cnt) { s_prefix = prefix | ((unsigned long long)(tid * 8 + b) << shift); s_k = k - (int)run; break; }
                    run += cnt;
                }
            }
            __syncthreads();
        }
        if (tid == 0) (stat == 0 ? lo : hi)[p] = bnr_double_of(s_prefix);
        __syncthreads();
    }
}

// ===================================================================================== k_acov
// Per-chain part of an effective-sample-size estimate (an addition to the reference, which only has split-Rhat:
// convergence.jl): for column p of the transposed window (see k_summary) and each half h of the window -- the same halves
// split-Rhat uses -- the mean, the variance (ddof 1) and the autocovariances at lags 0..L-1 (1/n normalisation).
// out: [half][2 + L][np] = mean, var, acov_0 .. acov_{L-1}.  One workgroup of 256 threads per (column, half): thread t owns
// lags t, t+256, ...; every sum runs over the samples in their order (deterministic).
__global__ __launch_bounds__(256) void k_acov(const double *buf, int nsamp, int np, int L, double *out)
{
    __shared__ double red[256];
    const int p = blockIdx.x, half = blockIdx.y, tid = threadIdx.x;
    const int h = nsamp / 2;
    const double *x = buf + (size_t)p * nsamp + (half == 0 ? 0 : nsamp - h);
    double acc = 0.0;
    for (int i = tid; i < h; i += 256) acc += x[i];
    red[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    const double mean = red[0] / h;
    __syncthreads();
    double *o = out + (size_t)half * (2 + L) * np + p;
    for (int lag = tid; lag < L; lag += 256) {
        double sacc = 0.0;
        for (int i = 0; i + lag < h; ++i) sacc += (x[i] - mean) * (x[i + lag] - mean);
        o[(size_t)(2 + lag) * np] = sacc / h;
        if (lag == 0) { o[0] = mean; o[(size_t)np] = sacc / (h - 1); }
    }
}

// ----------------------------------------------------------------------------------------- kernels added late in round 5, kept BEHIND the others: the order of the
// definitions is the order of the kernels in the code object, and a chain alone lost 1 % (k_chol_step 6.72 -> 6.83 us per launch) when they sat in the middle of it
// k_xpass_group2: k_xpass_group for long column chunks (chunk_x > 64: large q).  The column loop for NC members, straight-line: 16 columns of X in flight, the 2 NC multipliers of a column (W and sqrt(S) z1 of every member) contiguous
// in LDS (sWZ[column][member][2]: four 16-byte reads per column for eight members).  Round 5: the earlier form -- run-time member count tested inside the unrolled loops, one
// 8-byte LDS read per multiply-add -- waited for LDS in front of every multiply-add: 15.8 us of the kernel's 21 (in-kernel stamps, alone on the chip) for 2 x 16 columns.
template <int NC, class XT>
__device__ __forceinline__ void bnr_xg_columns(const XT *xp, size_t ld, int ne, const double *sWZ, double (&aw)[8], double (&aa)[8])
{
    int t0 = 0;
    for (; t0 + 16 <= ne; t0 += 16) {
        XT xv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) xv[u] = xp[(size_t)(t0 + u) * ld];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const double x = (double)xv[u];
            const bnr_d2 *o = (const bnr_d2 *)(sWZ + (size_t)(t0 + u) * 16);
#pragma unroll
            for (int c = 0; c < NC; ++c) { const bnr_d2 wz = o[c]; aw[c] = fma(x, wz[0], aw[c]); aa[c] = fma(x, wz[1], aa[c]); }
        }
    }
    for (; t0 < ne; ++t0) {
        const double x = (double)xp[(size_t)t0 * ld];
        const bnr_d2 *o = (const bnr_d2 *)(sWZ + (size_t)t0 * 16);
#pragma unroll
        for (int c = 0; c < NC; ++c) { const bnr_d2 wz = o[c]; aw[c] = fma(x, wz[0], aw[c]); aa[c] = fma(x, wz[1], aa[c]); }
    }
}
template <class XT>
__device__ __forceinline__ void bnr_xg_dispatch(int nc, const XT *xp, size_t ld, int ne, const double *sWZ, double (&aw)[8], double (&aa)[8])
{
    switch (nc) {
    case 1: bnr_xg_columns<1>(xp, ld, ne, sWZ, aw, aa); break;
    case 2: bnr_xg_columns<2>(xp, ld, ne, sWZ, aw, aa); break;
    case 3: bnr_xg_columns<3>(xp, ld, ne, sWZ, aw, aa); break;
    case 4: bnr_xg_columns<4>(xp, ld, ne, sWZ, aw, aa); break;
    case 5: bnr_xg_columns<5>(xp, ld, ne, sWZ, aw, aa); break;
    case 6: bnr_xg_columns<6>(xp, ld, ne, sWZ, aw, aa); break;
    case 7: bnr_xg_columns<7>(xp, ld, ne, sWZ, aw, aa); break;
    default: bnr_xg_columns<8>(xp, ld, ne, sWZ, aw, aa); break;
    }
}
template <int LATE>     // (a template only so that the kernel is emitted behind the others, with the instantiations: see the note above)
__global__ __launch_bounds__(256) void k_xpass_group2(const bnr_many chain_src, int s, int nchains)
{
    extern __shared__ double sh[];
    const int wg = blockIdx.x;
    const bnr_dev &c0 = chain_src.at(0);                  // the geometry and the shared X, index maps
    const int rs = (c0.n_pad + 255) / 256, bid = wg / rs, slice = wg % rs, tid = threadIdx.x;
    const int chunk = c0.chunk_x, e0 = bid * chunk, ne = min(chunk, c0.q - e0), R = c0.R;
    const size_t ld = c0.n_pad;
    double *sWZ = sh;                                      // [column of the chunk][member][W, sqrt(S) z1]
    __shared__ double *s_pw[8], *s_pa[8];
    const int i = slice * 256 + tid;
    const bool live = i < c0.n_pad;                        // n_pad is a multiple of 64: the last slice may be short
    const int ic = live ? i : 0;
    for (int cb = 0; cb < nchains; cb += 8) {
        const int nc = min(8, nchains - cb);
        __syncthreads();
        for (int it = tid; it < nc * chunk; it += 256) {
            const int c = it / chunk, t = it - c * chunk;
            const bnr_dev &cd = chain_src.at(cb + c);
            const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
            const double *row = cd.trace + (size_t)P.row * cd.rowlen, *prev = cd.trace + (size_t)P.prev * cd.rowlen;
            double w = 0.0, zz = 0.0;
            if (t < ne) {
                const int e = e0 + t;
                w = edge_W(row + cd.o_u, prev + cd.o_lam, R, cd.el[e], cd.ek[e]);
                zz = sqrt(prev[cd.o_S + e]) * bnr_normal(cd.seed, P.it, SITE_G_Z1, (uint32_t)e, 0);
                if (slice == 0) { cd.Wbuf[e] = w; cd.sz[e] = zz; }
            }
            sWZ[(size_t)t * 16 + 2 * c] = w; sWZ[(size_t)t * 16 + 2 * c + 1] = zz;
        }
        if (tid < nc) { const bnr_dev &cd = chain_src.at(cb + tid); s_pw[tid] = cd.PW; s_pa[tid] = cd.PA; }
        __syncthreads();
        double aw[8], aa[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { aw[c] = 0.0; aa[c] = 0.0; }
        if (c0.X8) bnr_xg_dispatch(nc, c0.X8 + (size_t)e0 * ld + ic, ld, ne, sWZ, aw, aa);
        else bnr_xg_dispatch(nc, c0.X + (size_t)e0 * ld + ic, ld, ne, sWZ, aw, aa);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < nc && live) { bnr_st8<BNR_ST_XPASS>(s_pw[c] + (size_t)bid * ld + i, aw[c]); bnr_st8<BNR_ST_XPASS>(s_pa[c] + (size_t)bid * ld + i, aa[c]); }
    }
}

// ------------------------------------------------------------------------------------- the draws of k_backproj64
// One rejection sampler (KIND 2: ratio of uniforms, 3: concave envelope) for the edges of one wave, one edge per lane (`mine`: this lane's edge is of that kind).  Every such lane
// runs bnr_gig_setup and attempt 0 of its edge.  The lanes whose attempt 0 is rejected are compacted (ballot + prefix count) into a list of open edges, and the fields of their
// bnr_gig_ctx that bnr_gig_try reads go to LDS (copied, not recomputed).  In every further round the wave's 64 lanes are dealt over the m open edges, A = the largest power of
// two <= 64 / m (at most 16) attempts each: lane l evaluates attempt base + l mod A of open edge l / A.  bnr_gig_try is a pure function of (ctx, seed, it, elem, k) and every open
// edge has been refused the attempts below `base`, so the lowest accepted index of a round is the first accepted attempt of bnr_gig's loop -- the same draw bit for bit, in ~2
// rounds of one instruction stream instead of as many dependent attempts as the unluckiest of 64 edges needs.  Bounded by BNR_MAX_ATTEMPTS with bnr_gig's fallback.
// Wave-level synchronisation only (sc / sres / sopen belong to this wave).
#define BNR_BP_NF 11                                      // staged fields per edge: the larger of the two sets below
#define BNR_BP64_STATIC_LDS ((2 * BNR_BP_NF * 64 + 3 * 64) * sizeof(double) + 2 * 64 * sizeof(int))     // k_backproj64's static arrays (the staging of both drawing waves)
template <int KIND>
__device__ __forceinline__ void bnr_bp_stage(double (*sc)[64], int slot, const bnr_gig_ctx &c)
{
    sc[0][slot] = c.alpha; sc[1][slot] = c.xm;
    if (KIND == 2) { sc[2][slot] = c.ulo; sc[3][slot] = c.uhi; sc[4][slot] = c.xoff; sc[5][slot] = c.t; sc[6][slot] = c.s; sc[7][slot] = c.nc; }
    else { sc[2][slot] = c.omega; sc[3][slot] = c.Atot; sc[4][slot] = c.A0; sc[5][slot] = c.A1; sc[6][slot] = c.x0; sc[7][slot] = c.k0; sc[8][slot] = c.k1; sc[9][slot] = c.k2; sc[10][slot] = c.x0l; }
}
template <int KIND>
__device__ __forceinline__ void bnr_bp_unstage(bnr_gig_ctx &c, const double (*sc)[64], int slot, double lambda)
{
    c.kind = KIND; c.lambda_old = lambda; c.lambda = lambda < 0.0 ? -lambda : lambda; c.half = (c.lambda == 0.5) ? 1 : 0;       // what bnr_gig_setup stores for this lambda
    c.alpha = sc[0][slot]; c.xm = sc[1][slot];
    if (KIND == 2) { c.ulo = sc[2][slot]; c.uhi = sc[3][slot]; c.xoff = sc[4][slot]; c.t = sc[5][slot]; c.s = sc[6][slot]; c.nc = sc[7][slot]; }
    else { c.omega = sc[2][slot]; c.Atot = sc[3][slot]; c.A0 = sc[4][slot]; c.A1 = sc[5][slot]; c.x0 = sc[6][slot]; c.k0 = sc[7][slot]; c.k1 = sc[8][slot]; c.k2 = sc[9][slot]; c.x0l = sc[10][slot]; }
}
template <int KIND>
__device__ __forceinline__ double bnr_bp_draw(bool mine, double chi, double psi, uint64_t seed, uint32_t it, int e0, int lane, double (*sc)[64], double *sres, int *sopen, int *cap)
{
    double Snew = 1.0;
    bool open = false;
    bnr_gig_ctx c;
    if (mine) {
        bnr_gig_setup(c, 0.5, chi, psi);
        c.kind = KIND;                                    // (bnr_gig_kind said so: bnr_gig_try's other sampler drops out)
        double out;
        if (bnr_gig_try(c, seed, it, (uint32_t)(e0 + lane), 0u, out)) Snew = out; else open = true;
    }
    const unsigned long long om = __ballot(open), below = (1ull << lane) - 1ull;
    int m = __popcll(om);                                 // open edges (the same number in every lane)
    if (m == 0) return Snew;
    if (open) { bnr_bp_stage<KIND>(sc, lane, c); sopen[__popcll(om & below)] = lane; }
    bnr_wsync();
    uint32_t base = 1u;
    while (m > 0 && base < BNR_MAX_ATTEMPTS) {
        const int lg = m <= 4 ? 4 : (m <= 8 ? 3 : (m <= 16 ? 2 : (m <= 32 ? 1 : 0))), A = 1 << lg;
        const int j = lane >> lg, a = lane & (A - 1);
        const uint32_t k = base + (uint32_t)a;
        const bool has = j < m;
        const int src = has ? sopen[j] : 0;
        if (has) bnr_bp_unstage<KIND>(c, sc, src, 0.5);   // (a lane without an edge reads no staging slot: slot 0 may never have been written)
        double out = 0.0;
        const bool ok = has && k < BNR_MAX_ATTEMPTS && bnr_gig_try(c, seed, it, (uint32_t)(e0 + src), k, out);
        const unsigned grp = (unsigned)(__ballot(ok) >> (j << lg)) & ((1u << A) - 1u);        // the accepted attempts of this lane's edge
        if (ok && a == __ffs(grp) - 1) sres[src] = out;                                        // the lowest accepted attempt wins
        const bool still = has && a == 0 && grp == 0u;
        const unsigned long long sm = __ballot(still);
        bnr_wsync();                                      // every lane has read its entry of the list before the list is rewritten
        if (still) sopen[__popcll(sm & below)] = src;
        m = __popcll(sm);
        base += (uint32_t)A;
        bnr_wsync();
    }
    if (m > 0) {                                          // attempt cap, as bnr_gig
        if (lane < m) {
            const int src = sopen[lane];
            bnr_bp_unstage<KIND>(c, sc, src, 0.5);
            if (cap) *cap = 1;
            sres[src] = c.alpha * c.xm;
        }
        bnr_wsync();
    }
    if (open) Snew = sres[lane];
    return Snew;
}

// ===================================================================================== k_backproj64
// The back-projection of a lockstep group and of launches of many rounds of workgroups: there the launch is bound by the vector instructions of the GIG draws, and k_backproj's
// drawing wave spends its 64 lanes on 32 edges (a speculative second attempt per edge and round that is thrown away whenever the first is accepted, one GIG setup and one pass
// of the 3R + 1 terms per 32 edges, both rejection samplers back to back in one wave).  Here a workgroup owns 64 consecutive edges (two chunks of the Psum table) and two of
// its waves draw, one sampler each and one edge per lane: the setup and attempt 0 of every edge once, then only the refused edges' further attempts, packed over the wave's
// lanes (bnr_bp_draw above: at the headline state 31 % of the first attempts are refused and a workgroup needs 1-2 packed rounds, against the 3.6 dependent attempts of the
// unluckiest of 64 edges).  The terms are spread over the four waves by factor, the sums over the block's threads.
// Per edge the same arithmetic as k_backproj: the same per-lane row sums and wave reduction (gamma), the first accepted attempt of bnr_gig (S), the same terms summed per chunk
// of 32 edges in the same order (Psum) -- bitwise the same tables.  A chain alone at moderate q keeps k_backproj (latency-bound: four drawing waves per 32 edges are shorter).
// flags bit 2 -> partial sums; gamma and S always.  grid = round_up(ceil(nblk_bp / 2), 8) x chains.
template <class SRC>
__global__ __launch_bounds__(256) void k_backproj64(const SRC chain_src, int s, int flags, int nchains)
{
    BNR_CRITICAL_PATH();
    const int gid = blockIdx.x, gx = gid & 7, gr = gid >> 3;
    const int pid = (gr / nchains) * 8 + gx;               // this chain's pair of chunks
    const bnr_dev &cd = chain_src.at(gr % nchains);
    if (2 * pid >= cd.nblk_bp) return;
    BNR_TL_IN(cd, TL_BACKPROJ, pid == 0);
    const int R = cd.R, n_pad = cd.n_pad, nterm = 1 + 3 * R;
    extern __shared__ double sh[];                          // a4 | 64 dots | u products R x 65 | terms (3R + 1) x 65
    double *sa = sh, *sdot = sa + n_pad, *sdr = sdot + 64, *st = sdr + R * 65;
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    double *row = cd.trace + (size_t)P.row * cd.rowlen;
    const double *prev = cd.trace + (size_t)P.prev * cd.rowlen;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int e0 = pid * 64, ne = min(64, cd.q - e0);
    const size_t ld = cd.n_pad;
    const double tau2 = row[ROW_TAU2], tau = sqrt(tau2), psi = prev[ROW_THETA];
    if (flags & 4) {
        const double *un0 = row + cd.o_u;
        for (int idx = tid; idx < R * 64; idx += 256) {
            const int r = idx >> 6, ee = idx & 63;
            double v = 0.0;
            if (ee < ne) { const int l0 = cd.el[e0 + ee], k0 = cd.ek[e0 + ee]; v = un0[r + R * l0] * un0[r + R * k0]; }
            sdr[r * 65 + ee] = v;
        }
    }
    for (int i = tid; i < n_pad; i += 256) sa[i] = cd.a4[i];
    __syncthreads();
    // dot products: wave w the columns w, w + 4, ..., four in flight
    for (int t = wave; t < ne; t += 16) {
        const int t2 = t + 4, t3 = t + 8, t4 = t + 12;
        const size_t oc = (size_t)(e0 + t) * ld, od = (size_t)(e0 + (t2 < ne ? t2 : t)) * ld, oe = (size_t)(e0 + (t3 < ne ? t3 : t)) * ld, of = (size_t)(e0 + (t4 < ne ? t4 : t)) * ld;
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        if (cd.X8) {
            const unsigned char *xc = cd.X8 + oc, *xd = cd.X8 + od, *xe = cd.X8 + oe, *xf = cd.X8 + of;
#pragma unroll 4
            for (int i = lane; i < n_pad; i += 64) { double av = sa[i]; acc0 = fma((double)xc[i], av, acc0); acc1 = fma((double)xd[i], av, acc1); acc2 = fma((double)xe[i], av, acc2); acc3 = fma((double)xf[i], av, acc3); }
        } else {
            const double *xc = cd.X + oc, *xd = cd.X + od, *xe = cd.X + oe, *xf = cd.X + of;
#pragma unroll 4
            for (int i = lane; i < n_pad; i += 64) { double av = sa[i]; acc0 = fma(xc[i], av, acc0); acc1 = fma(xd[i], av, acc1); acc2 = fma(xe[i], av, acc2); acc3 = fma(xf[i], av, acc3); }
        }
        acc0 = wave_sum(acc0); acc1 = wave_sum(acc1); acc2 = wave_sum(acc2); acc3 = wave_sum(acc3);
        if (lane == 0) { sdot[t] = acc0; if (t2 < ne) sdot[t2] = acc1; if (t3 < ne) sdot[t3] = acc2; if (t4 < ne) sdot[t4] = acc3; }
    }
    __syncthreads();
    // update_D! (gibbs.jl:454-458).  Two waves draw, one rejection sampler each (bnr_bp_draw above): wave w2 the workgroup's ratio-of-uniforms edges (kind 2 of bnr_gig_setup) and
    // the draws without a loop of their own (kinds 0, 1, 4), wave w3 its concave-envelope edges (kind 3) -- bnr_gig_kind decides, as in k_backproj.  The two rotate with the
    // workgroup and sit two waves apart: on different SIMDs, and the drawing waves of the workgroups that share a CU spread over all four.  All four waves stay to the last
    // barrier of the block (no block-wide barrier is asked of a block one of whose waves has left) and share the terms and the sums behind it.
    __shared__ double s_ctx[2][BNR_BP_NF][64];
    __shared__ double s_res[2][64], s_S[64];
    __shared__ int s_open[2][64];
    const int w2 = pid & 3, w3 = (pid + 2) & 3;
    const int e = e0 + lane;
    const bool act = lane < ne;
    double gam = 0.0, W = 0.0;
    if (act) {
        W = cd.Wbuf[e];
        const double Sp = prev[cd.o_S + e];
        gam = tau * (cd.sz[e] + Sp * sdot[lane]) + W;
        if (wave == w2) bnr_st8<BNR_ST_BACKPROJ>(row + cd.o_gamma + e, gam);
    }
    if (wave == w2 || wave == w3) {
        int cap = 0;
        const double g = gam - W, chi = (g * g) / tau2;
        const int kind = act ? bnr_gig_kind(0.5, chi, psi) : -1;
        if (wave == w2) {
            double Snew = bnr_bp_draw<2>(kind == 2, chi, psi, cd.seed, P.it, e0, lane, s_ctx[0], s_res[0], s_open[0], &cap);
            if (act && kind != 2 && kind != 3) {
                bnr_gig_ctx gc;
                bnr_gig_setup(gc, 0.5, chi, psi);
                Snew = bnr_gig_degenerate(gc, cd.seed, chi, psi, P.it, (uint32_t)e, &cap);
            }
            if (kind != 3) { s_S[lane] = Snew; if (act) bnr_st8<BNR_ST_BACKPROJ>(row + cd.o_S + e, Snew); }
        } else {
            const double Snew = bnr_bp_draw<3>(kind == 3, chi, psi, cd.seed, P.it, e0, lane, s_ctx[1], s_res[1], s_open[1], &cap);
            if (kind == 3) { s_S[lane] = Snew; bnr_st8<BNR_ST_BACKPROJ>(row + cd.o_S + e, Snew); }
        }
        if (cap) atomicAdd((unsigned long long *)&cd.counters[2], 1ull);
    }
    if (!(flags & 4)) { BNR_TL_OUT(cd, TL_BACKPROJ); return; }
    __syncthreads();                                       // every edge's S is in s_S
    // the partial sums of update_theta! / update_Lambda! (gibbs.jl:476, 603-605): every lane its edge's terms -- wave w those of the factors w, w + 4, ... --, then one thread per
    // chunk and term sums the term over the chunk's 32 edges in k_backproj's order
    const double Snew = s_S[lane];
    const double sd = sqrt(tau2 * Snew), lsd = log(sd) + 0.5 * log(2.0 * BNR_PI);
    const double *lamp = prev + cd.o_lam;
    if (wave == w2) st[lane] = act ? Snew : 0.0;
    for (int r = wave; r < R; r += 4) {
        const double dr = sdr[r * 65 + lane], lr = lamp[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double Wc = W + (bnr_lambda_value(c) - lr) * dr;
            const double zz = (gam - Wc) / sd;
            st[(1 + 3 * r + c) * 65 + lane] = act ? (-0.5 * zz * zz - lsd) : 0.0;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * nterm; idx += 256) {
        const int half = idx >= nterm ? 1 : 0, j = idx - half * nterm, chunk = 2 * pid + half;
        if (chunk < cd.nblk_bp) {
            double acc = 0.0;
#pragma unroll 8
            for (int e2 = 0; e2 < 32; ++e2) acc += st[j * 65 + 32 * half + e2];
            bnr_st8<BNR_ST_BACKPROJ>(cd.Psum + (size_t)chunk * nterm + j, acc);
        }
    }
    BNR_TL_OUT(cd, TL_BACKPROJ);
}

// (k_sdigits grew in the third session -- several workgroups per chain -- and moved here with the late kernels: see the note above)
template <class SRC, int L>
__global__ __launch_bounds__(1024) void k_sdigits(const SRC chain_src, int s)
{
    const bnr_dev &cd = chain_src.get_x();                    // grid = (chains, slices): every workgroup finds the largest S itself (q values out of the L2: the maximum does
                                                              // not depend on who computes it) and converts its slice of the entries -- one workgroup per chain took 38 us at
                                                              // q = 45 150 on the critical chain in front of the i8 Gram (round 5, third session)
    const int tid = threadIdx.x;
    const bnr_plan_entry P = cd.plan[cd.pbase[0] + s];
    const double *S = cd.trace + (size_t)P.prev * cd.rowlen + cd.o_S;
    __shared__ double red[16];
    __shared__ int s_nonfinite;
    if (tid == 0) s_nonfinite = 0;
    __syncthreads();                                          // the flag is cleared before any wave can set it
    double m = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    int k = tid;
    for (; k + 3072 < cd.q; k += 4096) { m = fmax(m, S[k]); m1 = fmax(m1, S[k + 1024]); m2 = fmax(m2, S[k + 2048]); m3 = fmax(m3, S[k + 3072]); }
    for (; k < cd.q; k += 1024) m = fmax(m, S[k]);
    // a NaN or an infinite S_k: fmax drops the NaN and the fixed-point image of either is meaningless -- the f64 Gram would carry it into G + I and the factorization
    // would report it; the same report from here.  Found from the sum of x - x over the entries (0 for every finite x, NaN for NaN and +-Inf): a second pass
    // over q values that sit in the L2
    {
        double z = 0.0;
        for (int kk2 = tid; kk2 < cd.q; kk2 += 1024) { const double v = S[kk2]; z += v - v; }
        if (!(z == 0.0)) atomicOr(&s_nonfinite, 1);
    }
    m = fmax(fmax(m, m1), fmax(m2, m3));
    m = fmax(m, __shfl_xor(m, 32)); m = fmax(m, __shfl_xor(m, 16)); m = fmax(m, __shfl_xor(m, 8));
    m = fmax(m, __shfl_xor(m, 4)); m = fmax(m, __shfl_xor(m, 2)); m = fmax(m, __shfl_xor(m, 1));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < 16; ++w) m = fmax(m, red[w]);
    if (s_nonfinite) {                                        // reported like a factorization that met a non-finite G + I (status 3, "G+I"); the digits below are then of no interest
        if (tid == 0) bnr_flag_gfail(cd);
        m = 1.0;
    }
    int e;
    (void)frexp(m, &e);                                       // m = f 2^e with f in [0.5, 1): every S_k < 2^e
    constexpr int BITS = 8 * L - 2;                           // S_k up < 2^BITS <= 2^62: the top digit stays below 64, a carry cannot overflow it
    const double up = ldexp(1.0, BITS - e);
    if (tid == 0 && blockIdx.y == 0) cd.scal[SC_I8SCALE] = ldexp(1.0, e - BITS);
    const int kchunk = cd.q_pad / cd.ksplit;
    for (int idx = (int)blockIdx.y * 1024 + tid; idx < cd.kslab; idx += (int)gridDim.y * 1024) {
        const int ks = idx / cd.kcp, kk = idx % cd.kcp, k = ks * kchunk + kk;
        unsigned long long N = 0;
        if (kk < kchunk && k < cd.q && !s_nonfinite) N = (unsigned long long)(S[k] * up + 0.5);     // rounded to nearest (the top digit has the headroom): |G_exact - G| <= q 2^(e - 8 L + 1), two-sided
        // balanced base-256 digits, least significant first: a byte >= 128 stands for byte - 256 and carries one into the next
        unsigned carry = 0;
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
            const unsigned b = (unsigned)((N >> (8 * (L - 1 - l))) & 255ull) + carry;
            carry = b >= 128u ? 1u : 0u;
            cd.Sdig[(size_t)l * cd.kslab + idx] = (unsigned char)(b & 255u);
        }
    }
}

// ===================================================================================== k_wsummary (chain stacking, ABI 16; an addition to the reference)
// Outside the sweep, with k_summary whose companion it is; behind every kernel of the sweep, so that none of them moves.
// k_wsummary: the mean and two order statistics of one staged column (see k_summary: column p of `buf`, leading dimension ld) under chain
// weights w_0 .. w_{K-1} (Yao, Vehtari & Gelman 2022): the column holds K segments of nsamp draws, chain k's in rows k nsamp ..
//   mean = sum_k w_k m_k, k ascending from 0.0, m_k = the mean of segment k in k_summary's order (256 thread-strided partial sums, the tree,
//          one division by nsamp): bit for bit bnr_chain_summary's mean of chain k;
//   the statistic of T (= (double)r / (double)K for a pooled rank r, divided on the host) = the draw x with the smallest bnr_key_of key for
//          which W(x) = sum_k w_k (double)c_k(x) >= T, c_k(x) = #{draws of chain k with key <= key(x)}; every product and every addition
//          rounded on its own (-ffp-contract=off), k ascending from 0.0.  Where W never reaches T (round-off at r = K nsamp): the largest draw
//          among the chains with w_k > 0.
// W is non-decreasing in the key also in floating point (each term is a monotone function of an integer count, and a rounded addition is
// monotone), so an MSD radix descent finds the draw exactly: per pass one integer histogram per chain in LDS (K x 2^bits counters; integer
// atomics only, nothing depends on their order), turned into per-chain inclusive prefix counts by one wave per chain (lane-owned runs, a
// shuffle scan), then every bin's W from `below_k` (the chain's draws under the current prefix) + its prefix count, and the first bin with
// W >= T by an integer atomicMin.  Digits: 10 bits for K <= 8 (7 passes: 6 x 10 + 4), 8 bits above (8 passes); 8192 counters = 32 KiB either
// way.  A column with a NaN draw is NaN in every output.  Columns p >= q get the mean only; mean, lo / hi (a pair) may be NULL.
// The digit width is the template parameter (the launcher picks it from K); a template also so that its code is emitted where it is
// instantiated, behind the sweep's kernels at the end of bnr_hip.hip.  One workgroup of 256 threads per column; results do not depend on the grid.  K <= BNR_STACK_MAX_CHAINS (include/bnr_hip.h); the weights by value (bnr_wsum_weights, bnr_internal.h).
template <int BITS>
__global__ __launch_bounds__(256) void k_wsummary(const double *buf, long long ld, int nsamp, int K, bnr_wsum_weights wt, int q, double T_lo, double T_hi,
                                                  double *mean, double *lo, double *hi)
{
    __shared__ unsigned int hist[8192];
    __shared__ double red[256];
    __shared__ double sw[BNR_STACK_MAX_CHAINS];
    __shared__ unsigned int below[BNR_STACK_MAX_CHAINS];
    __shared__ unsigned long long s_prefix, s_max;
    __shared__ int s_bin;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *col = buf + (size_t)p * (size_t)ld;
    if (tid < K) sw[tid] = wt.w[tid];
    // the means of the segments, each in k_summary's order, and their weighted sum; a NaN anywhere
    double wm = 0.0;
    int bad = 0;
    for (int k = 0; k < K; ++k) {
        const double *seg = col + (size_t)k * nsamp;
        double acc = 0.0;
        for (int i = tid; i < nsamp; i += 256) { const double v = seg[i]; bad |= v != v; acc += v; }
        __syncthreads();
        red[tid] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
        wm = wm + sw[k] * (red[0] / nsamp);
    }
    bad = __syncthreads_or(bad);
    if (tid == 0 && mean) mean[p] = bad ? NAN : wm;
    if (p >= q || !lo) return;
    if (bad) {
        if (tid == 0) { lo[p] = NAN; hi[p] = NAN; }
        return;
    }
    constexpr int bits0 = BITS;                          // 10 for K <= 8, 8 above: K 2^BITS <= 8192 counters
    for (int stat = 0; stat < 2; ++stat) {
        const double T = stat == 0 ? T_lo : T_hi;
        double wall = 0.0;                                   // W of the largest draw
        for (int k = 0; k < K; ++k) wall = wall + sw[k] * (double)nsamp;
        if (!(wall >= T)) {                                  // never reached: the largest draw among the chains with w_k > 0
            if (tid == 0) s_max = 0ull;
            __syncthreads();
            unsigned long long mx = 0ull;
            for (int k = 0; k < K; ++k) {
                if (!(sw[k] > 0.0)) continue;
                const double *seg = col + (size_t)k * nsamp;
                for (int i = tid; i < nsamp; i += 256) { const unsigned long long key = bnr_key_of(seg[i]); mx = key > mx ? key : mx; }
            }
            atomicMax(&s_max, mx);
            __syncthreads();
            if (tid == 0) (stat == 0 ? lo : hi)[p] = bnr_double_of(s_max);
            __syncthreads();
            continue;
        }
        if (tid == 0) s_prefix = 0ull;
        if (tid < K) below[tid] = 0u;
        __syncthreads();
        int shift = 64;
        while (shift > 0) {
            const int bits = shift < bits0 ? shift : bits0, nb = 1 << bits;
            const unsigned long long himask = shift >= 64 ? 0ull : (~0ull << shift);
            shift -= bits;
            const unsigned long long prefix = s_prefix;
            for (int b = tid; b < K * nb; b += 256) hist[b] = 0u;
            if (tid == 0) s_bin = nb;
            __syncthreads();
            for (int k = 0; k < K; ++k) {
                const double *seg = col + (size_t)k * nsamp;
                unsigned int *h = hist + k * nb;
                for (int i = tid; i < nsamp; i += 256) {
                    const unsigned long long key = bnr_key_of(seg[i]);
                    if ((key & himask) == prefix) atomicAdd(&h[(unsigned int)(key >> shift) & (unsigned int)(nb - 1)], 1u);
                }
            }
            __syncthreads();
            // per chain the inclusive prefix counts over the bins: wave wv takes the chains wv, wv + 4, ..; a lane owns `per` consecutive bins
            const int per = (nb + 63) / 64;
            for (int k = wv; k < K; k += 4) {
                unsigned int *h = hist + k * nb;
                const int b0 = lane * per, b1 = min(nb, b0 + per);
                unsigned int run = 0u;
                for (int b = b0; b < b1; ++b) run += h[b];
                unsigned int incl = run;
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned int v = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += v;
                }
                unsigned int c = incl - run;
                for (int b = b0; b < b1; ++b) { c += h[b]; h[b] = c; }
            }
            __syncthreads();
            // the first bin whose W reaches T
            for (int b = tid; b < nb; b += 256) {
                double W = 0.0;
                for (int k = 0; k < K; ++k) W = W + sw[k] * (double)(below[k] + hist[k * nb + b]);
                if (W >= T) { atomicMin(&s_bin, b); break; }    // (W is non-decreasing in b: this thread's later bins reach T as well)
            }
            __syncthreads();
            const int bin = s_bin < nb ? s_bin : nb - 1;         // (always < nb: the last bin's W is the W that reached T one level up)
            __syncthreads();
            if (tid < K && bin > 0) below[tid] += hist[tid * nb + bin - 1];
            if (tid == 0) s_prefix = prefix | ((unsigned long long)bin << shift);
            __syncthreads();
        }
        if (tid == 0) (stat == 0 ? lo : hi)[p] = bnr_double_of(s_prefix);
        __syncthreads();
    }
}
