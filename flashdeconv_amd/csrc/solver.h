// Internal interface of the BCD solve driver (solver.cpp).
#pragma once
#include <functional>
#include <vector>

#include "fdx_graph.h"
#include "fdx_internal.h"
#include "fdx_kernels.h"

namespace fdx {

struct SolveProblem {
    const fdx_graph* graph = nullptr;
    const double* H = nullptr;     // device (K, ldh) type-major
    long long ldh = 0;
    const double* XtX = nullptr;   // device (K, K)
    double* beta[2] = {nullptr, nullptr};  // device (K, ld) type-major double buffer
    long long ld = 0;
    int K = 0;                     // planes of H / beta, order of XtX (solver_padded_K of the cell types: pad types are all zero)
    int K_real = 0;                // cell types (0: = K); beta0 = 1 / K_real on the first K_real planes
    double YtY = 0.0;
    double lambda = 0.0;
    double rho_eff = 0.0;          // rho * mean(diag XtX)
    int max_iter = 100;
    double tol = 1e-4;
    int verbose = 0;
    int init_beta = 1;             // fill beta[0] with 1/K and clear the pad rows
    int beta0_virtual = 0;         // init_beta == 0 only: the caller cleared the pad rows of BOTH buffers but did not write 1/K into
                                   // beta[0] - the first sweep takes the constant instead of reading it (tiled kernel, no pad types);
                                   // where that kernel does not apply, solver_run writes the start vector itself
    int compute_objective = 1;
    int first_chunk = 4;
};

struct SolveResult {
    int result_buffer = 0;         // index into SolveProblem::beta holding the final abundances
    int n_iterations = 0;
    int converged = 0;
    double final_change = 0.0;
    double final_objective = 0.0;
    double sweep_ms = 0.0;
    std::vector<int> objective_iters;
    std::vector<double> objectives;
    std::vector<double> rel_changes;
};

int solver_init_beta(double* beta, long long ld, long long n_fill, int K, hipStream_t st, int K_planes = 0);   // K_planes > K: the rest zero
int solver_pad_square(const double* A, int K, double* B, int KP, hipStream_t st);   // B (KP, KP) = A (K, K) bordered with zeros
// zero the pad columns [n_used, ld) of a type-major (K, ld) array
int solver_zero_pad(double* b, long long ld, long long n_used, int K, hipStream_t st);
// The four sums of the objective on the device (out4_dev); the sharded driver all-reduces them across ranks.
int solver_objective_partials(const fdx_graph& g, const double* beta, long long ld, const double* H, long long ldh,
                              const double* XtX, int K, double* scratch_partials, double* out4_dev, hipStream_t st);
int solver_objective(const fdx_graph& g, const double* beta, long long ld, const double* H, long long ldh,
                     const double* XtX, int K, double YtY, double lambda, double rho_eff, double* scratch_partials,
                     double* scratch_out4, double* obj_host, hipStream_t st);
int solver_run(const SolveProblem& p, SolveResult* res, hipStream_t st);

// ---- pieces the single-GPU solve (solver_run) and the sharded one (comm.cpp) share
// The graph's part of a sweep's arguments: ELL arrays, sizes and - for a tiled graph - the tile fields (honour_no_tiled: unless
// FDX_NO_TILED asks for the global-gather sweep).  Everything else is left zero for the caller.
BcdSweepArgs sweep_args_for_graph(const fdx_graph& g, bool honour_no_tiled);
// Scratch of the sweeps that are not register-resident (more than 64 types outside 72 / 80 / 88 / 96): the LDS-resident sweep reads
// XtX with its rows padded to 16 (queued on st; scratch_ld stays 0), the generic one keeps the abundances in 2 K planes of scratch_ld
int sweep_scratch_prepare(const double* XtX, int K, int n_slices, DevBuf* scratch, size_t* scratch_ld, hipStream_t st);
// diag_mean = mean(diag XtX): rho_eff = rho * diag_mean (core/solver.py:359-360); auto_tune_lambda (core/spatial.py:181-190):
// alpha * diag_mean / max(mean degree, 1), alpha = 0.005
double xtx_diag_mean(const double* XtX_host, int K);
double auto_lambda(double diag_mean, double mean_degree);
// compute_objective (core/solver.py:269-284) from its four sums <H,beta>, beta' XtX beta, smoothness, |beta|_1
inline double objective_from_sums(const double* r4, double YtY, double lambda, double rho_eff) {
    return 0.5 * (YtY - 2.0 * r4[0] + r4[1]) + 0.5 * lambda * r4[2] + rho_eff * r4[3];
}

// The max slots of every iteration and, behind them, the rel_change trace: one device block, one fill (queued by init)
struct SweepStats {
    DevBuf block;
    unsigned long long* stats = nullptr;
    double* rel_change = nullptr;
    int init(int max_iter, hipStream_t st);
};
struct LoopResult {
    int n_iter = 0;                       // iteration + 1 (solver.py:422); 0 when max_iter == 0
    bool converged = false;
    const double* rel_changes = nullptr;  // n_iter values, pinned scratch of this thread: valid until the next loop
    double sweep_ms = 0.0;                // GPU time of the queued iterations only (host read-back gaps between chunks excluded)
};
// The chunked iteration driver: queue_iteration(it, last_of_chunk) queues iteration it on st; chunks of first_chunk, then
// 4, 8, 16, 32, 32, ... iterations, the rel_change trace read back once per chunk with the first n_ahead iterations of the next
// chunk queued before the host waits for it.  The stopping rule is solver.py:409-413 on the trace.
int solver_loop(const SweepStats& s, int max_iter, double tol, int first_chunk, int n_ahead,
                const std::function<int(int, bool)>& queue_iteration, LoopResult* res, hipStream_t st);

}  // namespace fdx
