/*
 * pgo.h -- C-ABI of the MI355X-native SE(2) pose-graph optimisation backend.
 *
 * Drop-in boundary for the one hot path of Sergimech/GraphSLAM: the src/graph
 * node's Levenberg-Marquardt solve over Pose2 prior + between factors, which
 * the reference performs in-process through GTSAM (/root/reference paths):
 *
 *   graph.cpp:58,86      initial.insert(Key, Pose2)             -> pgo_add_vertex
 *   graph.cpp:57         graph.add(PriorFactor<Pose2>(...))      -> pgo_add_prior
 *   graph.cpp:87-92,     graph.add(BetweenFactor<Pose2>(...))    -> pgo_add_edge
 *            106-111
 *   graph.cpp:45,83,103  noiseModel::Gaussian::Covariance(Q)     -> the cov[9] argument
 *   graph.hpp:45-58      covariance_to_eigen: row-major float64[9] -> same layout
 *   graph.cpp:119        LevenbergMarquardtOptimizer(graph, initial).optimize()
 *                                                                -> pgo_optimize
 *   graph.cpp:123-125    poses_opti.at<Pose2>(id).x()/y()/theta() -> pgo_get_pose(s)
 *   graph.cpp:130        initial = poses_opti (warm start)       -> in-place update
 *   graph.cpp:60,94,112  graph.nrFactors()                       -> pgo_num_factors
 *
 * Plain C types only: no exceptions, no torch types, caller buffers are
 * borrowed for the duration of a call.  Keys are 64-bit like gtsam::Key
 * (the reference's int8 ids, Factor.msg:1-2, wrap after 127).
 * A handle is single-threaded (like the reference's one ROS spinner,
 * graph.cpp:214); distinct handles are independent; each owns one HIP stream.
 */
#ifndef PGO_H
#define PGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGO_ABI_VERSION 6   /* 6: pgo_stats.handoff_retries / transport / part_transport
                                 (round 6); 5: the hybrid mode's partition-group
                                 communicator, pgo_debug_poison_fronts */

/* ---- status codes (GTSAM exception each one replaces) -------------------- */
#define PGO_OK 0
#define PGO_E_ARG (-1)           /* null handle / bad size                          */
#define PGO_E_DUP_KEY (-2)       /* gtsam::ValuesKeyAlreadyExists  (Values::insert) */
#define PGO_E_NO_KEY (-3)        /* gtsam::ValuesKeyDoesNotExist   (Values::at, or a
                                    factor on a key never inserted, at optimize)    */
#define PGO_E_BAD_COV (-4)       /* covariance not positive definite (LLT failure)   */
#define PGO_E_INDETERMINANT (-5) /* gtsam::IndeterminantLinearSystemException (GN)  */
#define PGO_E_NONFINITE (-6)     /* non-finite input or error                       */
#define PGO_E_HIP (-7)           /* HIP runtime failure (pgo_last_error has text)   */
#define PGO_E_NO_DEVICE (-8)     /* no usable MI355X / HIP device                   */
#define PGO_E_NOMEM (-9)
#define PGO_E_BAD_EDGE (-10)     /* between factor with key1 == key2                */
#define PGO_E_COMM (-11)         /* inter-rank exchange failed (RCCL / host callback) */
#define PGO_E_NOT_ENOUGH (-12)   /* closest_keyframe: no more keyframes than `skip`
                                    (the service returns false, graph.cpp:170-171) */
#define PGO_NO_KEY UINT64_MAX    /* batched search: the query has no candidate      */
#define PGO_W_MAXITER 1          /* informational: stopped at max_iterations        */

/* ---- algorithms / solvers ------------------------------------------------ */
#define PGO_ALG_LM 0             /* gtsam::LevenbergMarquardtOptimizer (graph.cpp:119) */
#define PGO_ALG_GN 1             /* gtsam::GaussNewtonOptimizer                      */
#define PGO_SOLVER_PCG 0         /* block-Jacobi preconditioned CG on the 3x3 BSR H  */
#define PGO_SOLVER_CHOLESKY 1    /* supernodal multifrontal Cholesky on the GPU (exact,
                                    like GTSAM's multifrontal elimination)          */

typedef struct pgo_graph pgo_graph;

#define PGO_ORDERING_ND 0        /* multilevel nested dissection of the pose graph
                                    (default: balanced elimination tree, C3 half
                                    the flops of minimum degree)                   */
#define PGO_ORDERING_AMD 1       /* approximate minimum degree                       */

typedef struct {
  int device;        /* HIP device ordinal (default 0) */
  int ordering;      /* fill-reducing ordering of the Cholesky solver, computed once
                        per graph structure (GTSAM: COLAMD every solve) [PGO_ORDERING_ND] */
  int reserved[6];
} pgo_opts;

typedef struct {
  /* gtsam::NonlinearOptimizerParams (defaults in brackets) */
  int max_iterations;           /* [100]  */
  double relative_error_tol;    /* [1e-5] */
  double absolute_error_tol;    /* [1e-5] */
  double error_tol;             /* [0]    */
  /* gtsam::LevenbergMarquardtParams */
  double lambda_initial;        /* [1e-5] */
  double lambda_factor;         /* [10]   */
  double lambda_upper_bound;    /* [1e5]  */
  double lambda_lower_bound;    /* [0]    */
  double min_model_fidelity;    /* [1e-3] */
  int use_fixed_lambda_factor;  /* [1]    */
  int algorithm;                /* [PGO_ALG_LM] */
  /* linear solver (the GPU replacement for GTSAM's multifrontal Cholesky) */
  int linear_solver;            /* [PGO_SOLVER_CHOLESKY] */
  double pcg_relative_tol;      /* stop when r'M^-1 r <= tol^2 * r0'M^-1 r0 [1e-10] */
  int pcg_max_iterations;       /* [20000] */
  int pcg_check_interval;       /* iterations enqueued between convergence reads [32] */
  int max_outer;                /* >0: stop after this many linearisations [0] */
  int profile_every;            /* >0: time every k-th PCG SpMV launch and every
                                   linearisation with HIP events on the handle's
                                   stream (pgo_stats.kernel_*) [0] */
  int use_graphs;               /* replay the captured factor+solve hipGraph [1] */
  int lambda_lanes;             /* Cholesky LM: consecutive lambda tries solved in
                                   one batched factor + solve on this GPU (the plan
                                   holds a numeric workspace per lane; every launch
                                   carries the lanes as grid dimension y, so the
                                   latency-bound top of the elimination tree costs
                                   about one pass for all lanes).  Speculative
                                   lambda search (see pgo_comm_*): results are
                                   those of 1 lane bit for bit [1] */
  int multi_gpu;                /* with a communicator of size > 1 (pgo_comm_*):
                                   PGO_MULTI_SPECULATIVE -- every rank solves
                                   different lambda tries of GTSAM's sequence;
                                   PGO_MULTI_PARTITION -- every try's
                                   factorisation is split: each rank factors
                                   its subtrees of the elimination tree, the
                                   subtree roots' Schur complements are
                                   all-gathered (the boundary reduction) and
                                   the top separators' columns are dealt to
                                   the ranks (each factored panel broadcast by
                                   its rank); composes with lambda_lanes;
                                   PGO_MULTI_HYBRID -- both: the ranks form
                                   groups, each group splits every
                                   factorisation over its partition-group
                                   communicator (pgo_comm_init_*_part) and the
                                   groups run the speculative search over the
                                   main communicator (one rank of every group
                                   each) [PGO_MULTI_SPECULATIVE] */
} pgo_params;

#define PGO_MULTI_SPECULATIVE 0
#define PGO_MULTI_PARTITION 1
#define PGO_MULTI_HYBRID 2

typedef struct {
  int status;                   /* PGO_OK / PGO_W_MAXITER / error                 */
  int iterations;               /* accepted steps (gtsam iterations())            */
  int inner_iterations;         /* lambda tries (LM) / steps (GN)                 */
  int linearizations;
  double initial_error;         /* graph.error(initial) = 0.5 chi^2               */
  double final_error;
  long long pcg_iterations;     /* summed over all solves                          */
  double ms_total;              /* wall time inside pgo_optimize                   */
  double ms_upload;             /* host->device graph upload (0 when resident)     */
  double ms_linearize;          /* device time of linearisation kernels            */
  double ms_solve;              /* device time of PCG                              */
  double ms_update;             /* retract + error + model-decrease kernels        */
  double kernel_spmv_ms;        /* summed device time of the timed SpMV launches   */
  long long kernel_spmv_count;  /* number of timed SpMV launches                   */
  double kernel_linearize_ms;   /* summed device time of the linearisation kernel  */
  long long kernel_linearize_count;
  double kernel_syrk_ms;        /* summed device time of Schur-update (MFMA) launches
                                   of the profiled factorisations                  */
  long long kernel_syrk_count;  /* profiled factorisations                         */
  double syrk_flops;            /* Schur-update flops of one factorisation         */
  double factor_flops;          /* flops of one numeric factorisation              */
  long long kernel_syrk_launches; /* timed Schur-update launches (all profiled
                                   factorisations)                                  */
  /* multi-GPU speculative lambda search (pgo_comm_*; zero / 1 on one rank) */
  int lambda_rounds;            /* lambda rounds: one parallel try on every rank    */
  int ranks;                    /* ranks that took part                             */
  long long solves;             /* linear solves this rank performed (incl. the
                                   speculative tries GTSAM's sequence never reached) */
  double ms_comm;               /* wall time in the all-gathers and broadcasts      */
  /* profiled factorisations (profile_every > 0, eager launches): device time from
     the first to the last launch of chol_factor / of the triangular solves,
     summed; per-kernel detail in pgo_get_kernel_profile */
  double ms_factor_profiled;
  double ms_solve_profiled;
  int stop_reason;              /* PGO_STOP_* : why the outer loop ended          */
  /* graph-replayed factorisations (use_graphs, every unprofiled one): summed
     device time of the factorisation graphs and the algorithmic flops they
     performed (lanes x one factorisation's flops) */
  double ms_factor_graph;
  double factor_graph_flops;
  /* the solver's plan on this call (the per-registration re-solve): 0 reused,
     1 same fronts / new H assembly (appended factors inside the existing fill),
     2 re-planned on the previous ordering with the appended poses inserted,
     3 full analysis (first call, or too much appended), 4 appended poses
     added to the plan incrementally (eliminated last, rows added along their
     fill paths to the root; PGO_NO_PLAN_APPEND=1 disables); ms_plan its
     host+upload ms */
  int plan_update;
  double ms_plan;
  /* how the device graph was brought up to date on this call: 0 resident, 1
     full upload, 2 appended in place (new keyframes / factors after the
     previous ones: the live re-solve); its host+upload time is ms_upload */
  int upload_kind;
  /* factorisations re-run because an in-launch hand-off timed out (a workgroup
     starved on a time-sliced GPU: the poll gives up after
     PGO_HANDOFF_TIMEOUT_MS and the try is run once more before the optimize
     fails with PGO_E_HIP).  0 in a healthy run; the parity tests assert it. */
  int handoff_retries;
  /* the transport of the handle's communicators on this call: PGO_TRANSPORT_*
     (main communicator; part_transport: the hybrid's partition group) */
  int transport;
  int part_transport;
} pgo_stats;

#define PGO_TRANSPORT_NONE 0     /* no communicator (one rank)                     */
#define PGO_TRANSPORT_RCCL 1     /* RCCL over xGMI                                 */
#define PGO_TRANSPORT_HOST 2     /* the caller's host callbacks (gloo in tests)    */

/* pgo_stats.stop_reason.  GTSAM reports every one of these as convergence
   (an LM that gives up leaves the values unchanged, so checkConvergence sees a
   zero decrease); the library tells them apart. */
#define PGO_STOP_CONVERGED 0     /* checkConvergence: relative / absolute decrease, error tol */
#define PGO_STOP_LAMBDA_BOUND 1  /* LM gave up: lambda reached lambda_upper_bound, no step accepted */
#define PGO_STOP_MAX_ITER 2      /* max_iterations accepted steps                   */
#define PGO_STOP_MAX_OUTER 3     /* pgo_params.max_outer linearisations              */
#define PGO_STOP_SMALL_CHANGE 4  /* tryLambda: |cost change| < relative_error_tol * error */
#define PGO_STOP_ERROR 5         /* error status (singular GN system, HIP, comm)    */

/* ---- lifetime ------------------------------------------------------------ */
pgo_graph *pgo_create(const pgo_opts *opts);        /* NULL opts: device 0 */
void pgo_destroy(pgo_graph *g);
const char *pgo_last_error(const pgo_graph *g);
const char *pgo_status_string(int status);
int pgo_abi_version(void);
void pgo_default_params(pgo_params *p);

/* ---- graph construction (graph.cpp:27-113) ------------------------------- */
/* Values::insert(key, Pose2(x, y, theta)); duplicate key -> PGO_E_DUP_KEY */
int pgo_add_vertex(pgo_graph *g, uint64_t key, double x, double y, double theta);
int pgo_add_vertices(pgo_graph *g, size_t n, const uint64_t *keys, const double *xyt);
/* graph.add(PriorFactor<Pose2>(key, pose, Covariance(cov))), cov row-major 3x3 */
int pgo_add_prior(pgo_graph *g, uint64_t key, const double pose[3], const double cov[9]);
/* graph.add(BetweenFactor<Pose2>(k1, k2, z, Covariance(cov))) */
int pgo_add_edge(pgo_graph *g, uint64_t k1, uint64_t k2, const double z[3], const double cov[9]);
/* bulk form; cov_stride 9 = one covariance per edge, 0 = one shared covariance */
int pgo_add_edges(pgo_graph *g, size_t n, const uint64_t *k1, const uint64_t *k2,
                  const double *z, const double *cov, int cov_stride);

/* ---- robust losses on between factors --------------------------------------
   gtsam::noiseModel::Robust::Create(mEstimator, Gaussian::Covariance(cov)) on a
   BetweenFactor<Pose2> (GTSAM >= 4.1 mEstimator definitions).  With the
   whitened residual norm r = sqrt(e^T Omega e) and the parameter k > 0:

     loss                     rho(r)                          w(r) = rho'(r) / r
     PGO_LOSS_NONE            r^2 / 2                         1
     PGO_LOSS_HUBER           r^2 / 2            if r <= k    1           if r <= k
                              k (r - k / 2)      otherwise    k / r       otherwise
     PGO_LOSS_CAUCHY          (k^2 / 2) log1p(r^2 / k^2)      1 / (1 + r^2 / k^2)
     PGO_LOSS_GEMAN_MCCLURE   (k^2 / 2) r^2 / (k^2 + r^2)     k^4 / (k^2 + r^2)^2

   The graph error (pgo_error, pgo_stats.initial_error / final_error, the
   trace's candidate error, LM's cost change) is the sum of rho(r) over the
   between factors plus the priors' e^T Omega e / 2.  The linearisation is
   iteratively reweighted least squares (Robust::WhitenSystem): the factor
   enters H and g with Omega replaced by w(r) Omega, r at the linearisation
   point; the model decrease is -(g'd + d'H d / 2) on that H and g, and LM's
   guard against a vanishing model decrease compares it with the linearised
   error sum of w r^2 / 2.  Marginal covariances and the diagnostics below use
   the weighted H.  Every m-estimator weight is continuous and in (0, 1] (a
   fixed weight, pgo_set_edge_weights below, may also be 0); priors take no
   loss.  pgo_add_edge(s) is PGO_LOSS_NONE, and a graph whose factors are all
   PGO_LOSS_NONE at weight 1 computes what it did before, bit for bit. */
#define PGO_LOSS_NONE 0
#define PGO_LOSS_HUBER 1
#define PGO_LOSS_CAUCHY 2
#define PGO_LOSS_GEMAN_MCCLURE 3
/* pgo_add_edge with a loss; an unknown loss, a non-finite k, or k <= 0 with a
   loss other than PGO_LOSS_NONE -> PGO_E_ARG */
int pgo_add_edge_robust(pgo_graph *g, uint64_t k1, uint64_t k2, const double z[3], const double cov[9],
                        int loss, double k);
/* bulk form; loss_stride 0 = one shared (loss[0], k[0]), 1 = one per edge */
int pgo_add_edges_robust(pgo_graph *g, size_t n, const uint64_t *k1, const uint64_t *k2,
                         const double *z, const double *cov, int cov_stride,
                         const int *loss, const double *k, int loss_stride);
/* w(r) of the between factors [first, first + n) in insertion order at the
   current values (device; 1.0 for PGO_LOSS_NONE): a caller rejects the loop
   closures whose weight ends low */
int pgo_get_edge_weights(pgo_graph *g, size_t first, size_t n, double *out);

/* ---- fixed weights on between factors ---------------------------------------
   w in [0, 1], finite; the factors [first, first + n) in insertion order must be
   PGO_LOSS_NONE (else PGO_E_ARG; a range past the last factor -> PGO_E_ARG).
   The factor's error becomes w r^2 / 2 and it enters H and g with Omega replaced
   by w Omega, whatever the values; w == 1 makes it a plain Gaussian factor again.
   pgo_get_edge_weights returns w exactly.  A values-only change: the Cholesky
   plan, the captured graphs and the ordering stay.  This is how a caller acts
   on a loop closure found to be wrong: weight 0 takes it out of every later
   solve.  With weights of 0 H may be singular: pgo_marginal_covariances* and
   Gauss-Newton then return PGO_E_INDETERMINANT as for any singular H, and
   LM's damping copes.  A graph whose weights are all back at 1 (and without a
   loss) takes the Gaussian kernels again and computes what a handle that never
   had weights computes, bit for bit. */
int pgo_set_edge_weights(pgo_graph *g, size_t first, size_t n, const double *w);

/* ---- graduated non-convexity (GNC) ------------------------------------------
   Yang, Antonante, Tzoumas, Carlone, "Graduated Non-Convexity for Robust
   Spatial Perception", RA-L 2020; GTSAM >= 4.1 GncOptimizer.  The candidate
   between factors (the ones that may be outliers) get weights in [0, 1] that an
   outer loop alternates with weighted least-squares solves while the surrogate
   of the robust cost goes from convex to the target (mu); it needs no good
   start.  With c^2 = barc_sq and r^2 = e' Omega e of a candidate:

     row 0     one inner pgo_optimize(g, inner) with all candidate weights 1;
               prev_cost = its final error.  No candidates: stop there.
     sweep     rmax_sq = the largest r^2 over the candidates at the result;
               GM:  mu = max(1, 2 rmax_sq / c^2)
               TLS: mu = c^2 / (2 rmax_sq - c^2); not positive or not finite:
                    stop with all weights 1 (PGO_GNC_STOP_ALL_INLIERS)
     t = 1 .. max_iterations
       weights at the current values (one device sweep):
               GM:  w = (mu c^2 / (r^2 + mu c^2))^2
               TLS: lo = mu / (mu + 1) c^2, up = (mu + 1) / mu c^2;
                    w = 1 (r^2 <= lo), 0 (r^2 >= up), else
                    sqrt(c^2 mu (mu + 1) / r^2) - mu
       inner pgo_optimize, warm-started from the current values
       cost = pgo_error (the weighted error)
       stop when  GM: |mu - 1| < 1e-3;  TLS: no candidate weight strictly
               between weights_tol and 1 - weights_tol (both PGO_GNC_STOP_MU);
               or |cost - prev_cost| / max(prev_cost, 1e-7) < relative_cost_tol
               (PGO_GNC_STOP_COST)
       else    GM: mu = max(1, mu / mu_step);  TLS: mu *= mu_step;
               prev_cost = cost
     final     a read-only sweep counts the candidates with r^2 > c^2
               (pgo_gnc_stats.outliers)

   Not GncOptimizer to the letter: every inner solve starts from the previous
   result, as in the paper (GTSAM 4.1 restarts from the initial values), and
   barc_sq is one number on r^2 (GTSAM: a per-factor threshold on the factor
   error).  Unverified against GTSAM itself.

   Candidates must be PGO_LOSS_NONE and a graph with any factor under an
   m-estimator loss -> PGO_E_ARG; a communicator of more than one rank ->
   PGO_E_ARG (one rank only); an unknown loss, barc_sq <= 0, mu_step <= 1,
   max_iterations < 0, a negative or non-finite tolerance -> PGO_E_ARG.  Fixed
   weights the candidates hold on entry are reset to 1; the other factors keep
   theirs.  An inner optimize that fails ends the call with its status: the
   values are those of the last successful inner solve and the candidates'
   weights are 1 again.  pgo_get_trace keeps describing the last inner
   optimize. */
#define PGO_GNC_GM 0    /* Geman-McClure surrogate, mu decreases to 1 */
#define PGO_GNC_TLS 1   /* truncated least squares, mu increases, weights end 0 / 1 */
typedef struct {
  int loss;                  /* [PGO_GNC_GM] */
  double barc_sq;            /* c^2, the inlier threshold on r^2 = e' Omega e
                                [11.344866730144373 = chi2inv(0.99, 3)] */
  double mu_step;            /* [1.4] */
  int max_iterations;        /* outer iterations [100] */
  double relative_cost_tol;  /* [1e-5] */
  double weights_tol;        /* TLS: a weight within this of 0 or 1 is binary [1e-4] */
  int keep_weights;          /* 1: the candidates keep their final weights as fixed
                                weights (pgo_set_edge_weights); 0: they are plain
                                again [1] */
} pgo_gnc_params;

#define PGO_GNC_STOP_MU 0             /* GM: mu reached 1; TLS: every weight binary */
#define PGO_GNC_STOP_COST 1           /* relative cost change below relative_cost_tol */
#define PGO_GNC_STOP_MAX_ITER 2
#define PGO_GNC_STOP_NO_CANDIDATES 3  /* the call was one pgo_optimize */
#define PGO_GNC_STOP_ALL_INLIERS 4    /* TLS: no candidate beyond the threshold after row 0 */
#define PGO_GNC_STOP_ERROR 5          /* an inner optimize failed */

typedef struct {
  int status;                /* PGO_OK / PGO_W_MAXITER (outer limit) / error          */
  int stop_reason;           /* PGO_GNC_STOP_*                                        */
  int outer_iterations;      /* weight updates, row 0 not counted                     */
  int candidates;
  int outliers;              /* candidates with r^2 > c^2 at the final values         */
  long long inner_tries;     /* lambda tries, summed over all inner solves            */
  long long linearizations;  /* ... and their linearisations                          */
  double mu_initial, mu_final;     /* NaN when no weight update ran                   */
  double initial_error;      /* pgo_error on entry (all candidate weights 1)          */
  double final_cost;         /* the weighted error at the final values                */
  double ms_total, ms_inner, ms_weights;   /* host wall: the call, the inner
                                optimizes, the sweeps with their read-backs           */
} pgo_gnc_stats;

void pgo_gnc_default_params(pgo_gnc_params *p);
/* idx: n insertion indices of the between factors that may be outliers (no
   duplicates); idx NULL: every between factor; n == 0 with idx != NULL: none.
   inner NULL: pgo_default_params; gnc NULL: pgo_gnc_default_params; stats may
   be NULL. */
int pgo_optimize_gnc(pgo_graph *g, const pgo_params *inner, const pgo_gnc_params *gnc,
                     size_t n, const size_t *idx, pgo_gnc_stats *stats);
/* One row of 8 doubles per inner solve of the last pgo_optimize_gnc, row 0
   first: mu (NaN in row 0), cost after the inner solve, sum of the candidates'
   weights, weights strictly between weights_tol and 1 - weights_tol, the
   largest candidate r^2 of the row's sweep (row 0: the sweep at its result),
   inner lambda tries, inner accepted steps, inner stop_reason (PGO_STOP_*).
   Returns the row count (rows beyond cap are not written). */
int pgo_get_gnc_trace(const pgo_graph *g, double *out, int cap);

/* ---- optimisation (graph.cpp:119, write-back :122-130) ------------------- */
/* Runs the optimiser from the handle's current values and replaces them with
 * the result (the reference's `initial = poses_opti`).  NULL params: defaults. */
int pgo_optimize(pgo_graph *g, const pgo_params *params, pgo_stats *stats);

/* Per-iteration record of the last pgo_optimize: one row of 8
 * doubles per lambda try GTSAM's sequence reached (LM) or per step (GN):
 *   accepted steps so far (LM: before this try; GN: after the step), lambda,
 *   solved (1/0), linear model decrease -(g'd + d'H d / 2) (NaN: not solved /
 *   GN), error at the candidate (+inf: not evaluated), model fidelity,
 *   accepted (1/0), wall ms since pgo_optimize entry when the outcome was known.
 * The columns match the oracle's trace (oracle/pgo_oracle.h) plus the ms.
 * Returns the row count (rows beyond cap are not written). */
int pgo_get_trace(const pgo_graph *g, double *out, int cap);

/* Profiled factorisations of the last pgo_optimize (pgo_params.profile_every
 * > 0): per kernel family f (0 <= f < returned count, name from
 * pgo_kernel_family_name) out[5 f ..] = launches, summed device ms (dispatch
 * events), algorithmic flops, algorithmic HBM bytes, 0. */
int pgo_get_kernel_profile(const pgo_graph *g, double *out, int cap);
const char *pgo_kernel_family_name(int f);

/* ---- values access ------------------------------------------------------- */
int pgo_get_pose(pgo_graph *g, uint64_t key, double out[3]);           /* Values::at */
/* keys NULL: all poses in insertion order (out holds 3*n doubles) */
int pgo_get_poses(pgo_graph *g, size_t n, const uint64_t *keys, double *out);
/* Values::update: overwrite current values (keys NULL: insertion order) */
int pgo_set_poses(pgo_graph *g, size_t n, const uint64_t *keys, const double *xyt);
/* Device-side copy of the current values into a snapshot slot / back (no PCIe
 * traffic): re-run a solve from the same initial values (graph.cpp:130 keeps
 * `initial` around the same way). */
int pgo_save_values(pgo_graph *g);
int pgo_restore_values(pgo_graph *g);
size_t pgo_num_factors(const pgo_graph *g);   /* graph.nrFactors() */
size_t pgo_num_vertices(const pgo_graph *g);  /* initial.size()    */
/* graph.error(values) = 0.5 sum e^T Omega e at the current values (device);
 * rho(r) for a between factor with a robust loss (see above). */
int pgo_error(pgo_graph *g, double *err);

/* ---- marginals ------------------------------------------
   gtsam::Marginals(graph, values).marginalCovariance(key) (graph.cpp:120,
   126-127, commented out in the reference; eigen_to_covariance graph.hpp:60-68):
   the 3x3 covariance of each pose in its tangent space (x, y, theta), i.e. the
   pose's block of H^-1 with H = J'Omega J linearised at the current values (no
   damping).  out: n x 9 doubles, row-major.  A singular H (a component without
   prior) returns PGO_E_INDETERMINANT, as GTSAM's Cholesky throws. */
int pgo_marginal_covariances(pgo_graph *g, size_t n, const uint64_t *keys, double *out);

/* gtsam::Marginals(graph, values) once, then marginalCovariance(key) for every
   key (graph.cpp:120,126-127), in one pass: one undamped factorisation, then
   the entries of H^-1 on the factor's pattern (the selected inverse) top-down
   over the fronts -- about twice the factorisation's flops for all poses.
   cov:  9 doubles per vertex, insertion order, row-major.  This is the vertex's
         block of H^-1, the same definition as pgo_marginal_covariances: H at the
         current values, undamped, the weighted H under a robust loss.
   edge_cross (may be NULL): 9 doubles per between factor, insertion order.  It
         is the block of H^-1 with the rows of k1 and the columns of k2,
         row-major.  Together with cov[k1] and cov[k2] it is the factor's 6x6
         joint marginal (a loop closure's Mahalanobis gate).
   Singular H -> PGO_E_INDETERMINANT.
   A factor on a key never inserted -> PGO_E_NO_KEY.
   cov NULL with vertices present -> PGO_E_ARG.
   A graph with no vertex -> PGO_OK. */
int pgo_marginal_covariances_all(pgo_graph *g, double *cov, double *edge_cross);

/* ---- linear initialisation (LAGO-style) -----------------------------------
   Initial values from the graph alone, in two linear solves, so that LM
   (pgo_optimize) starts inside the basin of convergence instead of at the
   dead-reckoned values.  The handle's current values are not an input: the
   result does not depend on them.

   Tree (host).  In every connected component the root is the first vertex, in
   insertion order, that carries a prior; its tree orientation is the angle of
   that vertex's first prior.  A FIFO breadth-first search, every vertex
   scanning its between factors in insertion order whichever end it is, gives
   each vertex a tree orientation thetaT: parent's + delta_e over a factor
   (parent, vertex), parent's - delta_e over (vertex, parent), with delta_e =
   atan2(sin z_theta, cos z_theta); thetaT is not wrapped.  Then per between
   factor k_e = rint((thetaT[k2] - thetaT[k1] - delta_e) / 2 pi) and per prior
   k_q = rint((thetaT[v] - theta_q) / 2 pi) fix the 2 pi ambiguities.
   Stage 1 (device): the orientations minimise
     sum_e w_e (th_k2 - th_k1 - delta_e - 2 pi k_e)^2 + sum_q w_q (th_v - theta_q - 2 pi k_q)^2,
   w the information of the angle with the translation marginalised out.
   Stage 2 (device): the positions minimise the graph's Gaussian error
   (pgo_error without a loss) with every orientation held at stage 1's: the
   exact minimiser, one linear solve.
   Both systems have the sparsity of H and run through the Cholesky solver's
   plan (one undamped factorisation and solve each).  The result replaces the
   handle's values; a following pgo_optimize starts from it.

   Not GTSAM's lago::initialize to the letter: the spanning tree is the
   breadth-first one (GTSAM: the odometric path or a minimum spanning tree),
   stage 2 applies no orientation correction, and the priors are used as given
   (GTSAM adds an anchor).  Robust losses are ignored in both stages, as if
   every factor were PGO_LOSS_NONE, and the initialiser is not robust itself:
   a wrong loop closure enters both solves at full weight.

   A component without a prior -> PGO_E_INDETERMINANT before any device work; a
   non-positive pivot in either solve -> PGO_E_INDETERMINANT; a factorisation
   whose in-launch hand-off timed out -> PGO_E_HIP (it is never re-run inside
   the call, so a success has no hidden retry); the values are then as they
   were on entry.  A factor on a key never inserted ->
   PGO_E_NO_KEY.  No vertex -> PGO_OK.  With a communicator of more than one
   rank every rank runs the call on its own one-rank plan and gets the same
   bits.  pgo_optimize never calls it. */
typedef struct {
  int status, components, tree_depth;  /* tree_depth: edges on the longest root-to-vertex tree path */
  long long wraps;                     /* sum |k_e| */
  double error_before, error_after;    /* pgo_error before / after */
  double ms_total, ms_tree, ms_orient, ms_trans;  /* wall; host BFS; each stage's assembly+factor+solve */
} pgo_init_stats;
int pgo_initialize_linear(pgo_graph *g, pgo_init_stats *stats);   /* stats may be NULL */

/* ---- loop-closure candidate search -----------------------
   The closest_keyframe service (graph.cpp:146-178): among the vertices in
   insertion order except the last `skip` (keyframes_to_skip_in_loop_closing,
   graph.cpp:15, = 10), the one whose current (x, y) is nearest to (x, y):
   distance sqrt((x2-x1)^2 + (y2-y1)^2) as the reference forms it, ties to the
   earliest inserted.  Fewer than skip + 1 vertices -> PGO_E_NOT_ENOUGH. */
int pgo_closest_keyframe(pgo_graph *g, double x, double y, int skip, uint64_t *key, double *dist);
/* Batched: for every query key (vertex i in insertion order) the service's
   answer when that key was keyframes.back(): query = its current (x, y),
   candidates = the vertices inserted before it except the last skip - 1 of
   them (indices [0, i + 1 - skip)).  No candidate: key PGO_NO_KEY, dist +inf. */
int pgo_closest_keyframes(pgo_graph *g, size_t q, const uint64_t *query_keys, int skip, uint64_t *keys_out,
                          double *dist_out);
/* device time (ms) of the last scan / batch search kernel launch */
int pgo_debug_search_ms(pgo_graph *g, double *scan_ms, double *batch_ms);

/* ---- scan registration: Generalized-ICP -----------------
   The scanner node's gicp() (scanner/src/scanner.cpp:35-74):
   pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ> with PCL's default
   parameters, setInputSource(current scan) / setInputTarget(keyframe scan),
   align(), hasConverged(), getFitnessScore(), getFinalTransformation(), then
   make_Delta and compute_covariance (scanner.hpp) and the keyframe rule
   (converged && fitness > converged_fitness_threshold = 0.1).  A batch of B
   independent registrations (pair b: source cloud b -> target cloud b) runs as
   one launch, one workgroup per registration.  Clouds are float xyz triplets,
   concatenated (src: sum(src_n) x 3, tgt: sum(tgt_n) x 3), 1 .. 4096 points
   each; guess: B x 16 row-major initial transforms (NULL = identity, as
   align(output) without a guess).  The optimiser restates PCL's GICP with
   Gauss-Newton where PCL runs BFGS (DESIGN.md "Scan registration"). */
typedef struct pgo_gicp pgo_gicp;
typedef struct {
  int max_iterations;                 /* 200   (GICP's max_iterations_) */
  int k_correspondences;              /* 20    neighbours per covariance, <= 32 */
  double gicp_epsilon;                /* 1e-3  smallest covariance eigenvalue */
  double max_correspondence_distance; /* 5     (squared: 25) */
  double transformation_epsilon;      /* 5e-4  translation-column change to stop */
  double rotation_epsilon;            /* 2e-3  rotation-element change to stop */
  int max_inner_iterations;           /* 20    optimiser steps per correspondence set */
} pgo_gicp_params;
typedef struct {
  double T[16];      /* getFinalTransformation(), row-major, source -> target frame */
  int converged;     /* hasConverged() (PCL sets it at max_iterations too) */
  int iterations;    /* correspondence rounds */
  double fitness;    /* getFitnessScore(): mean squared nearest-target distance */
  double delta[3];   /* make_Delta: T(0,3), T(1,3), atan(T(1,0) / T(0,0)) */
  double cov[9];     /* compute_covariance(0.1, 0.1, 0.1, delta), row-major */
  int keyframe;      /* converged && fitness > 0.1 (scanner.cpp:55-58) */
  int inner_iterations; /* optimiser steps over all rounds */
} pgo_gicp_result;
void pgo_gicp_default_params(pgo_gicp_params *p);
pgo_gicp *pgo_gicp_create(int device);
void pgo_gicp_destroy(pgo_gicp *h);
const char *pgo_gicp_last_error(const pgo_gicp *h);
int pgo_gicp_align_batch(pgo_gicp *h, int B, const float *src, const int *src_n, const float *tgt,
                         const int *tgt_n, const double *guess, const pgo_gicp_params *params,
                         pgo_gicp_result *out);
/* device time (ms) of the last batch (covariance + registration kernels) */
int pgo_gicp_debug_ms(const pgo_gicp *h, double *ms);

/* ---- occupancy-grid map from keyframe scans --------------------------------
   The reference keeps every keyframe's sensor_msgs/LaserScan next to its
   optimised pose (Keyframe.msg: scan, pose_opti), publishes them on
   /graph/keyframes and leaves the overlay to rviz; its simulated world
   (willow.pgm) is an occupancy image.  A pgo_map handle stores laser scans keyed
   like vertices and ray-casts them into an occupancy grid at given poses, on
   the GPU: one workgroup per scan, lanes over beams.  Its own device ordinal
   and stream, grow-only device buffers, no device touched before the first
   render or read (like pgo_gicp).

   Grid.  width x height cells of `resolution` metres, row-major, data[row *
   width + col]; cell (col, row) covers [origin_x + col res, origin_x + (col +
   1) res) x [origin_y + row res, origin_y + (row + 1) res): the
   nav_msgs/OccupancyGrid layout with an identity origin orientation.  Two int32
   planes, hit and miss.
   World -> cell.  col = floor((wx - origin_x) / resolution), row likewise, in
   fp64.  A scan whose pose is not finite, or whose sensor cell has |col| or
   |row| >= 2^30, is skipped whole (pgo_map_stats.scans_skipped).
   Beam i of a scan at pose (x, y, theta) -- the scan frame is the keyframe
   pose, the reference has no laser offset: r = (double)ranges[i], a = theta +
   (angle_min + i angle_increment).  NaN or r < range_min: skipped.  r >=
   range_max (+inf included): a no-return; with clear_no_return it is traced to
   d = range_max and every cell on it, the last included, gets miss += 1;
   without, it is skipped.  Otherwise d = r: every cell of the line but the last
   gets miss += 1, the last hit += 1.  End point (x + d cos a, y + d sin a).
   Line.  The classic all-octant integer Bresenham from the sensor's cell to the
   end point's cell, max(dx, dy) + 1 cells:
     dx = |x1 - x0|, dy = |y1 - y0|, sx = x1 > x0 ? 1 : -1, sy = y1 > y0 ? 1 : -1,
     err = dx - dy;  loop: visit (x, y); stop at (x1, y1); e2 = 2 err;
     if (e2 > -dy) { err -= dy; x += sx; }  if (e2 < dx) { err += dx; y += sy; }
   A visited cell outside the grid is skipped on its own and the walk goes on.
   Sensor cell == end cell: only the hit (or the one miss) is counted.
   Occupancy.  n = hit + miss; n == 0: -1 (unknown); else L = clamp(l_occ hit +
   l_free miss, l_min, l_max), p = 1 - 1 / (1 + exp(L)), value rint(100 p) in
   0 .. 100.  The log odds are clamped ONCE, at the end, not after every beam:
   this is deliberate, it makes the map independent of the order of scans and
   beams (a per-update clamp, as in the usual recursive filter, does not
   commute).
   Reproducibility.  The counts are integer sums (integer atomics only, no
   floating-point atomics anywhere): the same inputs give the same planes bit
   for bit in any scan insertion order and any launch shape.  A cell's count
   wraps past 2^31 - 1 updates (PGO_MAP_ACCUMULATE renders add up).

   Errors, all host-side before any device work.  PGO_E_ARG: resolution or an
   origin coordinate not finite, resolution <= 0; width or height < 1, width *
   height > 2^28; a non-finite l_*, l_min > l_max; a scan with n outside 1 ..
   4096, range_min < 0, range_max <= range_min, range_max / resolution > 32768
   (this bounds every beam's loop), a non-finite angle (the last beam's
   included), more than 2^31 - 1 beams in all; a scan range past the stored
   scans.  PGO_E_DUP_KEY: a scan key already stored.  PGO_E_NONFINITE: a
   non-finite host pose.  PGO_E_NO_DEVICE: only at a render or a read. */
typedef struct pgo_map pgo_map;
typedef struct {
  double resolution;     /* metres per cell [0.05] */
  double origin_x, origin_y;   /* world position of the corner of cell (0, 0) [0, 0] */
  int width, height;     /* cells [0: must be set] */
  double l_occ, l_free;  /* log odds of one hit / one miss [0.85, -0.4] */
  double l_min, l_max;   /* the final clamp [-2, 3.5] */
  int clear_no_return;   /* trace the beams without a return as free space [1] */
} pgo_map_params;
typedef struct {
  int status;
  long long scans, scans_skipped;   /* scans of the call; of them skipped whole */
  long long beams;                  /* beams of the scans not skipped = the next three */
  long long beams_return, beams_no_return, beams_skipped;   /* no_return counts them
                                       whether clear_no_return traces them or not */
  long long updates;                /* sum of hit + miss over the grid after the call */
  long long known_cells;            /* cells with hit + miss > 0 after the call */
  double ms_total;                  /* host wall time of the call */
  double ms_upload;                 /* host wall: staging and copies of new scans and poses */
  double ms_render;                 /* device events: the render kernel (with the pose gather) */
  double ms_finalize;               /* device events: counts -> occupancy and the reductions */
} pgo_map_stats;
void pgo_map_default_params(pgo_map_params *p);
pgo_map *pgo_map_create(int device, const pgo_map_params *p);   /* no device touched yet; NULL on bad params */
void pgo_map_destroy(pgo_map *m);
const char *pgo_map_last_error(const pgo_map *m);
/* the scan is copied; keys are the graph's vertex keys */
int pgo_map_add_scan(pgo_map *m, uint64_t key, int n, const float *ranges, double angle_min,
                     double angle_increment, double range_min, double range_max);
size_t pgo_map_num_scans(const pgo_map *m);
#define PGO_MAP_ACCUMULATE 1   /* do not clear the planes first */
/* poses from the host: scans [first, first + n) in insertion order, xyt 3 per scan;
   stats may be NULL */
int pgo_map_render(pgo_map *m, size_t first, size_t n, const double *xyt, int flags, pgo_map_stats *st);
/* every scan at the pose of its key among g's current device values, gathered on
   the device without a round trip over PCIe (g on another device -> PGO_E_ARG; a
   scan key that is no vertex -> PGO_E_NO_KEY before any device work) */
int pgo_map_render_graph(pgo_map *m, pgo_graph *g, int flags, pgo_map_stats *st);
/* the planes after the last render (zero before the first), width * height each;
   either may be NULL */
int pgo_map_get_counts(pgo_map *m, int32_t *hit, int32_t *miss);
/* width * height values: -1 unknown, 0 .. 100 */
int pgo_map_get_occupancy(pgo_map *m, int8_t *out);
/* Diagnostics only (the map benchmark script reads it; pgo_map_stats has no
   field for it): device time (ms) of the last render's clear pass, 0 under
   PGO_MAP_ACCUMULATE */
int pgo_map_debug_ms(const pgo_map *m, double *ms_clear);
/* Host-only, no handle: the line inline the render kernel runs, from (x0, y0) to
   (x1, y1): xy[2 k], xy[2 k + 1] = the k-th cell, up to cap cells.  Returns the
   cell count. */
int pgo_debug_map_line(int x0, int y0, int x1, int y1, int *xy, int cap);
/* Host-only: side, in cells, of the square near-field window of the miss plane
   the render kernel accumulates in LDS around the sensor cell (cells sx - side /
   2 .. sx + side / 2 - 1, likewise in y) */
int pgo_debug_map_window(void);

/* ---- multi-GPU: speculative lambda search ---------------------
   One process per GPU, every rank holding the same graph and values.  Where
   GTSAM's LM (graph.cpp:119) tries lambda, lambda*f, lambda*f^2, ... one after
   another until a try is accepted, the ranks of a communicator solve the next
   `size` tries of that sequence at once (rank r: the r-th), all-gather the
   outcomes (error, model decrease), apply GTSAM's accept rule in sequence order
   and take the first accepted candidate from the rank that computed it
   (broadcast of N poses).  Accepted steps, lambdas and values are bitwise those
   of the one-GPU run; the wall time of a linearisation drops from its number of
   lambda tries to ceil(tries / size) factorisations.
   Transports: RCCL over xGMI (pgo_comm_init_rccl; rank 0 makes the id with
   pgo_comm_unique_id and the caller distributes its bytes), or the caller's
   own host transport (pgo_comm_init_host).  Every rank must call pgo_optimize
   with the same params. */
typedef struct {
  void *ctx;
  int rank, size;
  /* out[size * bytes] = every rank's in[bytes], rank order; 0 on success */
  int (*allgather)(void *ctx, const void *in, void *out, size_t bytes);
  /* buf[bytes] of rank `root` to every rank, in place; 0 on success */
  int (*broadcast)(void *ctx, void *buf, size_t bytes, int root);
} pgo_host_comm;

/* ncclGetUniqueId; returns the id size in bytes (128) or < 0 */
int pgo_comm_unique_id(void *out, size_t cap);
/* ncclCommInitRank on the handle's device (collective: all ranks call it) */
int pgo_comm_init_rccl(pgo_graph *g, const void *unique_id, size_t id_bytes, int rank, int size);
int pgo_comm_init_host(pgo_graph *g, const pgo_host_comm *comm);
int pgo_comm_free(pgo_graph *g);
/* rank / size of the handle's communicator (0 / 1 without one) */
int pgo_comm_rank(const pgo_graph *g, int *rank, int *size);
/* PGO_MULTI_HYBRID: the partition group's communicator (the ranks that split
   one factorisation; collective over the group), RCCL or host transport; the
   main communicator then holds one rank of every group (the same position in
   each).  Set it up BEFORE the main communicator: a main init binds the
   group set up since the previous main init and frees an older one, so a
   main communicator replaced without pgo_comm_free never runs with a stale
   group.  A bound group of one rank makes PGO_MULTI_HYBRID the speculative
   search alone; none bound with a main communicator of > 1 rank ->
   PGO_E_ARG.  pgo_comm_free frees both. */
int pgo_comm_init_rccl_part(pgo_graph *g, const void *unique_id, size_t id_bytes, int rank, int size);
int pgo_comm_init_host_part(pgo_graph *g, const pgo_host_comm *comm);
int pgo_comm_part_rank(const pgo_graph *g, int *rank, int *size);
/* exchange check (no solve): all-gather of (rank, size, rank^2, 1) and a
   broadcast from rank size-1; PGO_OK when every rank saw the right data.  The
   host transport needs no GPU. */
int pgo_comm_selftest(pgo_graph *g);

/* ---- diagnostics (parity tests; device results at the current values) ---- */
/* H diagonal blocks (9 doubles row-major per vertex, insertion order), the
 * off-diagonal block H_{k1,k2} = J1^T Omega of every between factor (9 per
 * factor, insertion order), gradient g = J^T Omega e (3 per vertex), error. */
int pgo_debug_linearize(pgo_graph *g, double *hdiag, double *hoff, double *grad, double *err);
/* The same four outputs from the Cholesky-mode linearisation (owner blocks in
 * factor order, the path pgo_optimize takes with PGO_SOLVER_CHOLESKY). */
int pgo_debug_linearize_cholesky(pgo_graph *g, double *hdiag, double *hoff, double *grad, double *err);
/* y = (H + lambda I) x at the current linearisation (x, y: 3 per vertex) */
int pgo_debug_spmv(pgo_graph *g, double lambda, const double *x, double *y);
/* Diagnostics: device time of one replay of the captured factorisation graph
 * of `lanes` lambda lanes (lambda_l = 1e-5 10^l) at the current linearisation,
 * averaged over `reps` back-to-back replays (HIP events on the handle's
 * stream); PGO_ABLATE (families to leave out) applies at capture. */
int pgo_debug_factor_time(pgo_graph *g, int lanes, int reps, double *ms);
/* Diagnostics (tests): NaN into every element of the Cholesky workspace
 * (all lambda lanes) that a factorisation must write before it reads it --
 * the fronts' lower trapezoids, the frontal vectors, the diagonal inverses --
 * so a later optimize equals a clean run bit for bit only if no stale element
 * is ever read.  Needs the workspace (an optimize with the Cholesky solver). */
int pgo_debug_poison_fronts(pgo_graph *g);
/* delta = PCG solve of (H + lambda I) delta = -g at the current values */
int pgo_debug_solve(pgo_graph *g, double lambda, const pgo_params *params, double *delta,
                    int *pcg_iterations);
/* Host-only symbolic analysis of the current graph (no device needed):
 * out[0..11] = supernodes, levels, nnz(L), factor flops, Schur-update flops,
 * front doubles, launches per factorisation, launches per solve, max front,
 * trsm tasks, syrk tiles, small fronts; out[12..15] = update-matrix tiles formed
 * by their first Schur update instead of the tile assembly (PGO_FUSE_UPDATE=0:
 * none): all, with a child rectangle, with more than 16 of them, clipped by
 * their front's edge; from out[16], 6 per level (leaves first):
 * fronts, max m, max 64-blocks, panel steps, small fronts, syrk tiles. */
int pgo_debug_plan(pgo_graph *g, double *out, int cap);
/* Host-only: the digest of the plan of the current graph for rank `part_rank`
 * of `part_size` (1, 0: the one-rank plan), planned as pgo_debug_partition
 * plans it.  Returns S, the number of sections; out[0..S) = one 64-bit FNV-1a
 * hash per section of the plan (fronts and storage, partition and exchange
 * layout, level records, factor task lists, solve task lists, assembly,
 * selected inversion), then 20 counters of the scheduler's branches the plan
 * took (csrc/pgo_plan_digest.h), filled up to cap.  Two plans are the same
 * exactly when their sections agree. */
int pgo_debug_plan_digest(pgo_graph *g, int part_size, int part_rank, uint64_t *out, int cap);

/* Host-only: the selected-inversion pass of pgo_marginal_covariances_all as
 * the plan of the graph as it stands schedules it (cap >= 4).  out[0] kernel
 * launches of the pass (read-out included), out[1] its algorithmic flops,
 * out[2] doubles of device workspace beside the factorisation's (Z in the
 * fronts' layout, the panel scratch, the partial products, the read-out
 * buffer; 0 would be an in-place pass), out[3] levels; from out[4] the
 * launches of each level, leaves first. */
int pgo_debug_selinv_plan(pgo_graph *g, double *out, int cap);
/* Host-only, no device: pgo_initialize_linear's spanning tree.  parent: the
 * tree parent of every vertex (insertion index, -1 for a root); k_edge: k_e per
 * between factor, insertion order; k_prior: k_q per prior, insertion order.
 * Arrays are filled up to their caps.  Returns the vertex count, or
 * PGO_E_INDETERMINANT (a component without a prior) / PGO_E_NO_KEY. */
int pgo_debug_init_tree(pgo_graph *g, int *parent, long long *k_edge, long long *k_prior, size_t cap_v,
                        size_t cap_e, size_t cap_p);
/* Device: the assembled linear system of stage 1 or 2 of pgo_initialize_linear
 * in pgo_debug_linearize's layout: hdiag 9 per vertex, hoff the block (k1, k2)
 * of every between factor, 9 each, insertion order, rhs 3 per vertex.  Stage 1
 * fills the theta slot (the (x, y) slots an identity), stage 2 the (x, y) slots;
 * stage 2 is assembled at the handle's current orientations.  The values stay. */
int pgo_debug_init_system(pgo_graph *g, int stage, double *hdiag, double *hoff, double *rhs);
/* Host-only, no handle: the optimiser's control (the lambda sequence, the
 * accept / stop rules, the lane rule, the counters) driven as pgo_optimize
 * drives it over `ranks` x `lanes` tries per round, on recorded tries instead
 * of a device.  Linearisation i holds the tries [lin_ptr[i], lin_ptr[i + 1])
 * of `tries`, 3 doubles each: solved (1/0), error at the candidate, linear
 * model decrease (the trace's columns 2, 4, 3); lin_err (NULL: the error
 * itself) is the linearised error per linearisation that the guard against a
 * vanishing model decrease compares with.  A try past the recorded ones of
 * its linearisation is speculative: its outcome is a poison that would be
 * accepted if the control ever walked it.  adapt_mode: PGO_LANES_ADAPT;
 * params->profile_every > 0: every such factorisation runs one lane alone.
 * Returns the trace's row count and writes up to trace_cap rows of 7 doubles
 * (pgo_get_trace's without the wall ms).  out (out_cap >= 11): iterations,
 * inner iterations, linearisations, status, stop reason, final lambda, lambda
 * factor and error, lambda rounds, 1 if the control asked for a linearisation
 * past the recorded ones, accepted tries; then (rank, lane) of each accepted
 * try as out_cap allows. */
int pgo_debug_lm_replay(const pgo_params *params, double initial_error, int ranks, int lanes,
                        int adapt_mode, int n_lin, const int *lin_ptr, const double *tries,
                        const double *lin_err, double *trace, int trace_cap, double *out, int out_cap);
/* Host-only, no handle: the GNC outer loop's control (the initial mu, the mu
 * schedule, the stop rules) driven as pgo_optimize_gnc drives it, on recorded
 * rows instead of a device.  Row 0 is the plain inner solve: cost[0] its final
 * error, rmax_sq[0] the sweep at its result; row r >= 1: cost[r] after the
 * inner solve of outer iteration r, nonbinary[r] the non-binary weights of its
 * sweep (rmax_sq[r] is recorded only).  mu_out[r]: the mu of row r (NaN in row
 * 0).  Returns the rows the control walked (1 when it stops after row 0);
 * *stop_out the PGO_GNC_STOP_* reason, -1 when the control asked for a row past
 * the recorded ones.  initial_error is reported by the driver and read by no
 * rule.  Bad params -> PGO_E_ARG. */
int pgo_debug_gnc_control(const pgo_gnc_params *params, double initial_error, int rows,
                          const double *rmax_sq, const double *cost, const double *nonbinary,
                          double *mu_out, int *stop_out);
/* Host-only, no handle: w[i] = the GNC weight of r2[i] under `loss` at mu and
 * barc_sq -- the inline the sweep kernel runs. */
int pgo_debug_gnc_weight(int loss, double mu, double barc_sq, size_t n, const double *r2, double *w);
/* Device: the GNC weights sweep once at the current values over the n
 * candidates idx (NULL: every between factor), as pgo_optimize_gnc runs it.
 * w_all (may be NULL): one weight per between factor in insertion order,
 * non-candidates reading as 1.  stats5: max r^2, sum of the weights, weights
 * strictly between 1e-4 and 1 - 1e-4, candidates with r^2 > barc_sq,
 * candidates.  write != 0: the candidates hold their weights afterwards as
 * fixed weights (pgo_set_edge_weights); write == 0: the graph is as it was. */
int pgo_debug_gnc_sweep(pgo_graph *g, int loss, double mu, double barc_sq, size_t n, const size_t *idx,
                        int write, double *w_all, double *stats5);
/* Host-only: the subtree partition the PGO_MULTI_PARTITION factorisation
 * uses over `size` ranks: owner[s] per supernode (rank, -1 = top front;
 * returns the supernode count, arrays filled up to cap) and out[0..size+1] =
 * per-rank subtree flops, then the top's flops; then (as cap allows)
 * out[size+1 .. 2 size+1] = per-rank flops with the distributed top (subtrees
 * + the rank's top columns + the top work every rank repeats) and
 * out[2 size+1] = that repeated work, out[2 size+2] = the exchange points
 * (panel broadcast rounds) per factorisation and out[2 size+3] = the doubles
 * they broadcast per lambda lane. */
int pgo_debug_partition(pgo_graph *g, int size, int *owner, double *out, int cap);
/* Host-only: the supernodal elimination tree (parent per supernode, -1 root);
 * returns the supernode count. */
int pgo_debug_parents(pgo_graph *g, int *parent, int cap);
/* Host-only: the Cholesky solver's fill-reducing ordering of the poses
 * (perm[k] = insertion index of the k-th eliminated pose), n = vertex count.
 * bench.py hands it to the CPU restatement so both factor the same fill. */
int pgo_debug_ordering(pgo_graph *g, int32_t *perm, size_t n);
/* per supernode of the same host-only plan: pivot columns w, rows m, level
   (height in the elimination tree); returns the supernode count (arrays are
   filled up to cap entries) or a negative status */
int pgo_debug_fronts(pgo_graph *g, int *w, int *m, int *level, int cap);
/* Host-only, no device: the sub-group widths the row kernels of the graph as it
   stands are instantiated with.  G (4, 8, 16 or 32 lanes per vertex row, from
   the mean row length 2 E / n): k_linearize, k_pcg_spmv, k_spmv,
   k_model_decrease; G1 (from the mean side-1 list length E / n):
   k_linearize_side1. */
int pgo_debug_row_lanes(pgo_graph *g, int *G, int *G1);

#ifdef __cplusplus
}
#endif
#endif /* PGO_H */
