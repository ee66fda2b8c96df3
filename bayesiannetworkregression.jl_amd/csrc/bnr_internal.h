// bnr_internal.h -- what the two translation units of libbnr_hip.so share on the host: bnr_hip.hip (the sweep, tables, convergence messages, options)
// and bnr_analysis.hip (the posterior analysis).  Declarations, plain structs and two macros; every function declared here is defined in bnr_hip.hip.
#pragma once
#include "../../include/bnr_hip.h"
#include "bnr_device.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
// the message of bnr_last_error() (thread-local, one object for the whole library); returns code
int fail(int code, const std::string &msg);
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(BNR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

// Where and how sweeps are issued: ONE chain, or a lockstep group of equally shaped chains whose kernels are launched
// together (blockIdx.z = member).  Kernels read their chain's bnr_dev from the device array `cds`.
struct bnr_exec {
    int device = 0;
    int ncu = 256;                                      // compute units of the device
    int nb = 1;                                         // chains issued together
    bnr_dev *cds = nullptr;                             // device array of nb structs
    const bnr_dev *shape = nullptr;                     // host struct of member 0 (sizes are equal for all members)
    hipStream_t stream = nullptr, stream2 = nullptr;   // stream2: the Gram branch of a sweep
    std::vector<hipEvent_t> fj;                         // fork/join events
    size_t fj_next = 0;
    int overlap = 1;
    int gram_variant = 0;                               // 0: chosen per launch; 8 / 16: k_gram8 / k_gram forced (tests, experiments)
    int fuse_reduce = -1;                               // -1 / 1: launch 0 of the one-panel factorization also sums the Gram's K-split partials (no k_gram_reduce launch); 0: separate pass
    int reduce_epw = 0;                                 // eighths of a partial tile per reduction workgroup of that launch 0: 0 chosen per launch (reduce_epw_default); 1, 2, 4 forced (tests, measurements)
    int group_xpass = -1;                               // -1 / 1: a group whose members share X runs the X pass with one workgroup per chunk for all chains; 0: per chain
    bnr_plan_entry *gplan_pin = nullptr, *gplan_dev = nullptr;   // groups: the members' plans of a run call, staged for one copy
    int gplan_cap = 0;                                  // entries per member in there
    int wide_backproj = -1;                              // 1: k_backproj64 (64 edges per workgroup, one sampler per drawing wave, packed retries); -1: a group with more chunks than CUs, a chain alone at large q (launch_backproj)
    int split_sums = -1;                                 // 1: the back-projection's partial sums as a launch of their own in front of the scalar tail (off the critical chain)
    int spw_cap = 1;                                    // super blocks per update workgroup of the factorization, at most (round 6: 1 -- with the four-wave panel sweep (bnr_panel_sweep_pipe) one block each is the shorter launch: 8 chains 369.4 against 372-374 us per sweep; rounds 3-5 packed up to 4 behind the single sweeping wave)
    // Round 6: WHEN the scalar branch's kernels start is part of the schedule (profiles/round6_experiments_notes.txt A): inside the two-branch sweep they are ordered behind
    // points of the critical chain by events (graph edges), instead of starting whenever the dispatcher lets the second queue in.
    int tail_after = -2;                                // k_tail(s-1) waits for: -1 nothing (rounds 1-5), 0 the Gram of sweep s; -2: default by size (tail_after_default)
    int node_after = -2;                                // k_node(s) waits for factorization launch number node_after (0-based; -1 nothing); -2: default by size (node_after_default)
    int factor_variant = -1;                            // -1: chosen by size; 0: right-looking k_chol_step (+ k_gram_reduce); 2 / 3: two panels per launch (k_chol_step2), 3 with the K = 128 trailing update
    int use_graph = 1, graph_k = 16;                     // (round 5: 16, was 8 -- between two graph launches the GPU idles ~30 us: 640 sweeps 382.2 -> 380.1 us each, 20 sweeps = 16 + 4 instead of 8 + 8 + 4)
    struct rung { int k; hipGraph_t graph; hipGraphExec_t gexec; };
    std::vector<rung> ladder;                           // captured graphs of graph_k, graph_k/2, ..., 1 sweeps: any batch is replayed
    bnr_dev *cds_pin = nullptr;                         // pinned staging of the members' descriptors
    long long *status_dev = nullptr, *status_pin = nullptr;   // nb x 16: the members' event counters, gathered once per run call
    int64_t n_replayed = 0, n_eager = 0;                // sweeps issued by graph replay / eagerly since the last run call began
    // profiling
    int profiling = 0;
    std::vector<hipEvent_t> ev;  // pairs around k_gram
    double t_gram_us = 0, t_iter_us = 0, t_gram_acc = 0;
    int64_t n_gram = 0, n_iter = 0;
};

// read-only device inputs of a fit (model matrix, response, edge maps, Gram task map): shared by the chains created
// with bnr_chain_create_like, freed with the last of them
struct bnr_inputs {
    std::vector<void *> bufs;
    ~bnr_inputs() { for (void *p : bufs) (void)hipFree(p); }
};

struct bnr_chain {
    bnr_dev d{};
    std::shared_ptr<bnr_inputs> in;
    bnr_exec x;                  // issues this chain alone
    int device = 0;
    std::vector<void *> allocs;
    bnr_plan_entry *plan_dev = nullptr, *plan_pin = nullptr;
    int plan_cap = 0;
    int64_t iter = 0;            // global iteration id of the last drawn row
    int carried_row = -1;        // 0-based row whose (rr, sig_q) are in d.scal; -1 = invalid
    int next_row = 0;            // 1-based j the next run call would write
    bool pending = false;
    long long *counters_host = nullptr;
    int *pbase_dev = nullptr;
    size_t trace_bytes = 0;
    struct bnr_group *group = nullptr;   // lockstep group this chain belongs to (at most one)
    const unsigned char *x8_kept = nullptr;   // the byte image of X (also while option "byte_x" is 0); nullptr: the input had none
    const unsigned char *xm_kept = nullptr;   // the byte MASK of a 0/1 model matrix for the i8 Gram (also while option "gram_i8" is 0); nullptr: the input was not binary
    long long cap_seen = 0;      // sampler-cap events already reported (the device counter is cumulative: a capped draw is reported by the call it happened in, once)
    int predict_block_rows = 0;  // tunable "predict_block_rows": rows per block of bnr_chain_predict / bnr_chain_loglik_stats (0: automatic)
    int summary_block_cols = 0;  // tunable "summary_block_cols": parameter columns per staging block of the Summary calls (0: automatic)
    int rank_block_cols = 0;     // tunable "rank_block_cols": parameter columns per staging block of the rank-normalised diagnostics (0: automatic)
    int cov_block_cols = 0;      // tunable "cov_block_cols": edge columns per staging block and per Gram block of bnr_chains_cov (0: automatic)
};

struct bnr_group {
    std::vector<bnr_chain *> m;
    bnr_exec x;                  // issues all members together
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
// the first failure of a launch (or of a noted HIP call of the launch helpers) since the last check, reported under `what`
int check_launch(const char *what);

// device temporaries of one call, freed on every path (zeroed on the chain's stream, see dev_alloc; zero = false: a staging buffer that is
// written whole before it is read)
struct dev_tmp {
    std::vector<void *> p;
    ~dev_tmp() { for (void *q : p) (void)hipFree(q); }
    template <typename T>
    int alloc(T **out, size_t count, hipStream_t st, bool zero = true)
    {
        void *q = nullptr;
        HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
        p.push_back(q);
        if (zero) HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(count, 1) * sizeof(T), st));
        *out = (T *)q;
        return BNR_OK;
    }
};
// The results of one call: k columns of m doubles on the device (zeroed), brought to the host in one copy.  fetch: the copy and the sync on st
// (a failure is reported as "<call>: ..."), the launch check under the kernel's name, then column j into dst[j] where that is not NULL
struct result_slab {
    double *d = nullptr;
    size_t m = 0;
    int k = 0;
    int alloc(dev_tmp &tmp, int cols, size_t rows, hipStream_t st) { k = cols; m = rows; return tmp.alloc(&d, (size_t)k * m, st); }
    double *col(int j) const { return d + (size_t)j * m; }
    int fetch(hipStream_t st, const char *call, const char *kernel, std::initializer_list<double *> dst) const
    {
        std::vector<double> host((size_t)k * m);
        hipError_t e = hipMemcpyAsync(host.data(), d, sizeof(double) * host.size(), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(BNR_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e));
        if (int rc = check_launch(kernel)) return rc;
        size_t j = 0;
        for (double *p : dst) { if (p) memcpy(p, host.data() + j * m, sizeof(double) * m); ++j; }
        return BNR_OK;
    }
};

// Where the model matrix comes from: the n x q matrix X_new of generate_samples! (gibbs.jl:917-918) in one of the element types
// the reference accepts (Matrix{eltype(T)}: Bool, Int, Float64 ...), or the vector of n adjacency matrices itself, vectorised on
// the device (setup_X!, gibbs.jl:239-247: row i = lower_triangle(X[i]), utils.jl:40-57).
struct x_source {
    const void *X = nullptr;               // n x q column-major (mats == nullptr)
    const void *const *mats = nullptr;     // n pointers to V x V column-major matrices
    int dtype = BNR_F64;
};
size_t dtype_size(int t);
// k_x_convert on `rows` rows of raw (on the device, host layout, element type dtype; mats: V x V matrices) into the f64 matrix Xd of leading
// dimension ld; an integer type also fills the byte image X8 (nullable), not_bytes (nullable) is raised by an entry that is no byte
void launch_x_convert(int dtype, const void *raw, bool mats, int rows, const bnr_dev &d, int ld, double *Xd, unsigned char *X8, int *not_bytes, hipStream_t st);

// k_fetch_cols, k_summary, k_acov and k_wsummary live among the sweep kernels (table I/O and bnr_chain_ess_stats use them too): bnr_analysis.hip launches them through
// these.  fetch_cols: rows first .. first + nrows - 1 (0-based) of the trace columns off .. off + ncols - 1 into out, column-major with leading dimension ldo;
// summary: one workgroup per column of buf (the first q of them get the order statistics); acov: np series of nsamp draws, both halves, L lags
void launch_fetch_cols(hipStream_t st, const double *trace, int rowlen, int off, int ncols, int first, int nrows, double *out, long long ldo);
void launch_summary(hipStream_t st, int cols, const double *buf, int nsamp, int q, int k_lo, int k_hi, double *mean, double *lo, double *hi);
void launch_acov(hipStream_t st, const double *buf, int nsamp, int np, int L, double *out);
// k_wsummary (chain stacking, ABI 16) lives beside k_summary: `cols` staged columns of leading dimension ld, each K segments of nsamp draws, under the
// chain weights wt (by value); the first q columns get the statistics of the pooled ranks k_lo, k_hi (T = rank / K); mean, lo / hi may be NULL
struct bnr_wsum_weights { double w[BNR_STACK_MAX_CHAINS]; };
void launch_wsummary(hipStream_t st, int cols, const double *buf, long long ld, int nsamp, int K, const bnr_wsum_weights &wt, int q, int k_lo, int k_hi,
                     double *mean, double *lo, double *hi);
#pragma GCC visibility pop
