// bnr_device.h -- what the sweep kernels (bnr_kernels.h) and the posterior-analysis kernels (bnr_analysis_kernels.h) share: the chain descriptor, the
// row layout, the wave / workgroup sums, the order-preserving key image of a double.  Device helpers and plain structs only: no __global__ function
// lives here, so that no kernel is emitted into both code objects of the library.
#pragma once
#include "bnr_rng.h"

struct bnr_plan_entry { uint32_t it; int32_t row; int32_t prev; int32_t wrap; };   // rows 0-based; wrap: 1 copy the row to row 0 (purge ring), 2 placeholder, 4 also to row 1

struct bnr_dev {
    // sizes
    int n, n_pad, V, R, q, q_pad, tot;
    // row layout (offsets in doubles)
    int o_xi, o_lam, o_pi, o_M, o_u, o_gamma, o_S, rowlen;
    // hyper
    double eta, zeta, iota, aDelta, bDelta, nu;
    uint64_t seed;
    // inputs
    const double *X, *y;
    const unsigned char *X8;     // X once more as BYTES (same padded layout) when the caller's model matrix is 0..255-valued (Bool adjacency
                                 // data, gibbs.jl:907-918): the two bandwidth-bound passes over X read an eighth of the bytes; nullptr otherwise
    const int *ek, *el;          // edge e -> column node k, row node l (l >= k)
    // binary model matrix (every entry 0 or 1: the reference's adjacency data, docs/src/man/inputdata.md:5-10): the Gram on the i8 matrix pipe
    const unsigned char *XM;     // [n_pad][kslab] row-major byte MASK of X (0xFF where X = 1): column k = ks kchunk + kk at byte ks kcp + kk of a row
                                 // (every K slice padded with zeros to a multiple of 64 columns = one v_mfma_i32_16x16x64_i8 step); nullptr: no such image
    unsigned char *Sdig;         // [i8L][kslab] the balanced base-256 digits of the chain's S in the same column order (k_sdigits), its scale in scal[SC_I8SCALE]
    int kcp, kslab, i8L;         // padded K slice, bytes per row of XM, number of digit planes (7 or 8)
    int xi_ref;                  // model option "xi_weights": 0 log-space node weights (default), 1 the reference's pdf ratio (k_node; in the padding in front of trace)
    // state
    double *trace;
    const bnr_plan_entry *plan;
    const int *pbase;            // plan[pbase[0] + s] is the entry of slot s (lets a captured graph be replayed)
    // work
    double *Wbuf, *sz;           // q_pad each
    double *PW, *PA;             // nblk_x x n_pad GEMV partials (X W, X sz)
    double *PG;                  // nblk_x x n_pad GEMV partials (X gamma, refresh path)
    int nblk_x, chunk_x;
    double *Gpart, *E;           // Gram partial tiles; E = extended matrix of the factorization (see k_gram_reduce)
    int ksplit, ntile, gram_kg;  // ntile = n_pad/64; gram_kg = K-groups per k_gram workgroup (2 or 4)
    const int *gmap;             // k_gram: workgroup id -> (tile | ks << 16), XCD-aware (K slice x on the workgroups of XCD label x)
    double *a3, *xw, *a4, *res, *xg, *bw, *wv;   // n_pad each (bw: right-hand side b = a1 - a3; wv: w = L^-1 b)
    double *scal;                // [0]=rr (sum res^2), [1]=sig_q (sum (g^2/2)/S), [2]=tau (sqrt tau2 of current row), [3..4] pre-drawn tau2
    double *Minv;                // R*R + 1: inv(M) and logdet M of the state the next k_node reads (written by k_tail)
    double *Psum;                // nblk_bp x (1+3R) partial sums from k_backproj
    int nblk_bp, chunk_bp;
    long long *counters;         // [0] jitter, [1] nan_w, [2] sampler cap, [3] chol fail, [4..7] where, [8] branch-order violations,
                                 // [9] the G + I factorization of the running gamma update failed (bnr_flag_gfail; counted once by k_solve_w)
    unsigned long long *dbg;     // in-kernel s_memtime stamps (diagnostics only; never read by any kernel)
    unsigned int *stamp;         // one word per k_gram_reduce workgroup: iteration id of the Gram it finished (checked by k_chol_step)
    // Left from the factorization experiments of rounds 3-4 (tools/experiments/), read by no kernel: gprog = ntile + 4 words that k_gram_reduce and launch 0 of
    // k_chol_step zero every sweep; gmapc, dfctl = always null.  They stay in the descriptor because taking them (and the two stores) out changes the register
    // allocation of k_chol_step and k_gram_reduce (profiles/sweep_cleanup_codeobject.txt): that wants a timing of its own.
    unsigned int *gprog;
    const int *gmapc;
    unsigned int *dfctl;
};

enum { ROW_TAU2 = 0, ROW_THETA = 1, ROW_DELTA = 2, ROW_MU = 3 };
enum { SC_RR = 0, SC_SIGQ = 1, SC_TAU = 2, SC_TAU2N = 3, SC_TAU2N_IT = 4, SC_I8SCALE = 8 };   // TAU2N: tau2 pre-drawn by k_tail for iteration id TAU2N_IT

// ----------------------------------------------------------------------------------------- helpers
// Sum over the 64 lanes of a wavefront, result in every lane.  Four DPP butterfly steps inside each row of 16 lanes
// (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) and a fixed-order sum of the four row totals through SGPRs
// (v_readlane): no LDS permutes on the latency path, and a summation order that does not depend on the data.
__device__ __forceinline__ double bnr_dpp_f64(double v, const int ctrl_sel)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    if (ctrl_sel == 0) { lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true); }
    else if (ctrl_sel == 1) { lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true); }
    else if (ctrl_sel == 2) { lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true); }
    else { lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true); }
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bnr_readlane_c(double v, const int srclane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane), hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
    v += bnr_dpp_f64(v, 0);
    v += bnr_dpp_f64(v, 1);
    v += bnr_dpp_f64(v, 2);
    v += bnr_dpp_f64(v, 3);
    return (bnr_readlane_c(v, 0) + bnr_readlane_c(v, 16)) + (bnr_readlane_c(v, 32) + bnr_readlane_c(v, 48));
}
// wave-level LDS hand-off: a ds_write is not ordered before later ds_reads of the same wave without this wait (measured)
__device__ __forceinline__ void bnr_wsync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }
// sum over each aligned group of 32 lanes (result in every lane of the group)
__device__ __forceinline__ double half_wave_sum(double v)
{
    v += bnr_dpp_f64(v, 0);
    v += bnr_dpp_f64(v, 1);
    v += bnr_dpp_f64(v, 2);
    v += bnr_dpp_f64(v, 3);
    double lo = bnr_readlane_c(v, 0) + bnr_readlane_c(v, 16), hi = bnr_readlane_c(v, 32) + bnr_readlane_c(v, 48);
    return ((threadIdx.x & 32) == 0) ? lo : hi;
}
__device__ __forceinline__ double block_sum(double v, double *sh /* >= blockDim/64 doubles */)
{
    v = wave_sum(v);
    int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += sh[i];
    __syncthreads();
    return s;
}

typedef double bnr_d4 __attribute__((ext_vector_type(4)));
typedef double bnr_d2 __attribute__((ext_vector_type(2)));

// The order-preserving 64-bit image of a double (k_summary, k_rank, k_hdi).
// The order is the one the reference's sort uses (Julia's isless) and numpy's: numbers by value (-Inf first, +Inf last; -0 below +0, which
// compare equal), then every NaN, whatever its sign or payload.  All NaNs share the top key, so a rank that falls among them reports a NaN
// (the one bnr_double_of makes of the top key), and the sign-bit NaNs x86 produces (inf - inf, 0 / 0) in a loaded table cannot sort below the
// numbers as their bit image would.  NaN-free columns get the same keys as before.
__device__ __forceinline__ unsigned long long bnr_key_of(double v)
{
    if (v != v) return ~0ull;
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double bnr_double_of(unsigned long long k)
{
    unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)u);
}
