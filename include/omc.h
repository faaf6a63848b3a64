/* omc.h -- C ABI of the MI355X node-relaxation engine (libomc_hip.so).
 *
 * Drop-in boundary for the per-B&B-node hot path of OptimalMatrixCompletion.jl.  The reference has no FFI
 * today; the seam is four plain-Julia call sites in the driver (OMC.jl = /root/reference/src/
 * OptimalMatrixCompletion.jl):
 *     relaxation            OMC.jl:747-754   -> matrix_completion_SDP_relaxation   OMC.jl:1431-1943
 *     master feasibility    OMC.jl:814       -> matrix_completion_master_feasible  OMC.jl:1261-1277
 *     altmin                OMC.jl:540-546, 875-881 -> alternating_minimization    OMC.jl:1979-2279
 *     separation            OMC.jl:971-983   -> create_matrix_cut_child_nodes      OMC.jl:2466-2477
 *     objective             OMC.jl:565, 925  -> evaluate_objective                 OMC.jl:2330-2359
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows the Julia
 * `ccall` shim a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every matrix is COLUMN-MAJOR fp64 (Julia `Matrix{Float64}` layout);
 *   - the caller owns every input and output array; the library keeps no host pointer after a call returns;
 *   - device copies of A / mask live in the handle (they are constant for a whole B&B run, OMC.jl:470-471);
 *   - return value: 0 = ok; < 0 = invalid argument (the reference's `error(...)` checks, OMC.jl:1455-1477,
 *     2337-2348, 2433-2462); > 0 = HIP runtime error code.  Message via omc_last_error().  Nothing unwinds
 *     across the boundary.
 *   - safe to call from one host thread per handle; the batch entry point is the source of parallelism.
 */
#ifndef OMC_H
#define OMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMC_VERSION 100

/* termination status, mapped on the MOI statuses the driver branches on (OMC.jl:780-785, 809-812, 841) */
#define OMC_OPTIMAL 0        /* MOI.OPTIMAL / LOCALLY_SOLVED: gap and feasibility tolerances met        */
#define OMC_SLOW_PROGRESS 1  /* MOI.SLOW_PROGRESS: iteration cap reached, values available              */
#define OMC_TIME_LIMIT 2     /* MOI.TIME_LIMIT: time limit reached, values available                    */
#define OMC_INFEASIBLE 3     /* MOI.INFEASIBLE family: "feasible" = false (OMC.jl:1921-1935)            */
#define OMC_CUTOFF 4         /* MOI.OBJECTIVE_LIMIT: the node's rigorous dual_bound exceeds the cutoff of omc_relax_set_cutoff; values
                                available as they stand (not converged), as for OMC_SLOW_PROGRESS              */

/* disjunctive_cuts_type (OMC.jl:150, 1456) */
#define OMC_CUT_LINEAR 0
#define OMC_CUT_LINEAR2 1
#define OMC_CUT_LINEAR3 2
/* direction strings of a cut (OMC.jl:34, 2481-2491) */
#define OMC_DIR_LEFT 0
#define OMC_DIR_MIDDLE 1
#define OMC_DIR_RIGHT 2
#define OMC_DIR_INNER_LEFT 3
#define OMC_DIR_INNER_RIGHT 4
/* disjunctive_cuts_breakpoints (OMC.jl:151, 2466-2477) */
#define OMC_SMALLEST_1_EIGVEC 1
#define OMC_SMALLEST_2_EIGVEC 2

/* error classes (negative return values) */
#define OMC_ERR_INVALID_ENUM (-1)   /* OMC.jl:1456-1462, 2433-2446 */
#define OMC_ERR_DIMENSION (-2)      /* OMC.jl:240-254, 1465-1477, 2337-2348 */
#define OMC_ERR_ARGUMENT (-3)
#define OMC_ERR_UNSUPPORTED (-4)    /* valid in the reference, not built yet (see DESIGN.md scope table) */
#define OMC_ERR_NO_DEVICE (-5)
#define OMC_ERR_COMM (-6)           /* RCCL not loadable / communicator not initialised / a collective failed */
#define OMC_ERR_ALLOC (-7)          /* the buffers of the Shor-mode certificates do not fit the device (nothing is staged) */

typedef struct omc_instance omc_instance; /* opaque handle: device copies of A, mask, index lists, workspaces */

/* solver parameters of the relaxation (all have defaults via omc_relax_params_default) */
typedef struct omc_relax_params {
  double eps_gap;      /* stop when objective - dual_bound <= eps_gap * max(1,|objective|)   (1e-6)  */
  double eps_feas;     /* and cone residual <= eps_feas * sqrt(n+k)                          (1e-7)  */
  int max_iters;       /* iteration cap -> OMC_SLOW_PROGRESS                                 (3000)  */
                       /*   base mode stops at the first check at or after it; Shor mode checks at the cap itself */
  int check_every;     /* certificate evaluated every this many iterations                   (25)    */
  double rho_scale;    /* penalty = rho_scale * gamma/2 ||A_Omega||^2 / (m (1+gamma k/n)^2)  (1.0)   */
  double rho_f_ratio;  /* penalty of the per-column blocks relative to the cone blocks       (0.1)   */
  double relax;        /* over-relaxation                                                    (1.6)   */
  double time_limit;   /* seconds (OMC.jl:752, 1489)                                         (3600)  */
  int reference_quirk_q1; /* 1: linear3/right piece exactly as OMC.jl:1675; 0: secant        (1)     */
  int breakpoints;     /* OMC_SMALLEST_1_EIGVEC / _2_ : which separation vector to return    (1)     */
  int stall_checks;    /* stop with OMC_SLOW_PROGRESS after this many stationary checks      (8)     */
  int bump_max;        /* penalty bumps per node (0 = off): rho *= bump_factor when the primal   (2)     */
  double bump_ratio;   /*   residual exceeds bump_ratio x the dual residual at a check ...      (4.0)   */
  double bump_factor;  /*                                                                       (4.0)   */
  int bump_after;      /*   ... from this iteration on, at least bump_window checks apart       (100)   */
  int bump_window;     /*                                                                       (4)     */
  int slots;           /* nodes relaxed concurrently (continuous batching); 0 = min(B, 256)       (0)     */
  int accel;           /* 1: Anderson acceleration of the ADMM fixed-point map (type II, safeguarded) (0)  */
  int aa_mem;          /*   differences kept (<= 10)                                                 (10)    */
  int aa_every;        /*   an extrapolated point every this many iterations                         (10)    */
  int aa_start;        /*   first iteration that records history                                     (50)    */
  double aa_reg;       /*   Tikhonov weight of the least squares, relative to mean diag              (1e-10) */
  double aa_safeguard; /*   the point is kept when the next fixed-point residual <= this x the last  (1.0)   */
  int first_wins;      /* 1: the batch ends at the first check at which some node is OPTIMAL; the others are
                          returned as they stand (SLOW_PROGRESS, values available).  Penalty autotune.  (0)     */
  int early_stop_after;     /* a node whose gap, at the geometric rate it closed over the last checks, needs more than       */
  double early_stop_factor; /*   early_stop_factor x the checks left before max_iters is returned as OMC_SLOW_PROGRESS at once
                                 (eight consecutive predictions, from iteration early_stop_after on); 0 = off   (400, 1.5) */
} omc_relax_params;

void omc_relax_params_default(omc_relax_params* p);

const char* omc_last_error(void);
int omc_version(void);
int omc_device_count(void);

/* Upload (A, indices, gamma) once.  Replaces nothing in the reference (it passes A/indices to every call,
 * OMC.jl:747-754); sizes are checked as OMC.jl:240-254 does.  `mask` is n*m bytes (0/1), column-major.   */
int omc_instance_create(int n, int m, int k, const double* A, const uint8_t* mask, double gamma, int device,
                        omc_instance** out);
/* Same, with Julia's BitMatrix storage: packed UInt64 chunks, column-major bit order, LSB first. */
int omc_instance_create_bits(int n, int m, int k, const double* A, const uint64_t* chunks, double gamma,
                             int device, omc_instance** out);
void omc_instance_destroy(omc_instance* h);

/* ---- relaxation: matrix_completion_SDP_relaxation (OMC.jl:1431-1943), disjunctive mode -----------------
 * B nodes at once.  Node b carries L[b] cuts; cuts of all nodes are concatenated:
 *   cut_x    n      doubles per cut   (breakpoint vector,            OMC.jl:34 tuple element 1)
 *   cut_Uhat n*k    doubles per cut   (parent's U, column-major,     tuple element 2)
 *   cut_dir  k      int8 per cut      (OMC_DIR_* codes,              tuple element 3)
 * U_lower / U_upper: n*k doubles per node, or NULL for the reference defaults (OMC.jl:1442-1449).
 * Outputs (any matrix pointer may be NULL to skip the copy):
 *   objective[b]   recomputed from primal values as OMC.jl:1880-1896 does
 *   dual_bound[b]  certified lower bound on the relaxation optimum (reference quirk Q2: the reference uses
 *                  the primal value as node bound; this engine returns both)
 *   status[b], iters[b]
 *   Y n*n, U n*k, X n*m, Theta m*m per node  (OMC.jl:1897-1900)
 *   lambda_min[2*b..]: two smallest eigenvalues of U U' - Y      (OMC.jl:1274, 2467-2470)
 *   breakpoint_x n per node: separation vector per params->breakpoints (OMC.jl:2466-2477), sign fixed so that
 *                  its largest-magnitude entry is positive
 *   solve_time[b]: seconds of device time attributed to the batch (same value for every node of the batch)
 */
int omc_relax_batch(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                    const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                    const double* U_upper, double* objective, double* dual_bound, int* status, int* iters,
                    double* Y, double* U, double* X, double* Theta, double* lambda_min, double* breakpoint_x,
                    double* solve_time);

/* The same call split in three so that a caller (bench.py) can time the device-resident part alone:
 * stage = host->device of the node descriptors, solve = kernels only, fetch = device->host of results.   */
int omc_relax_stage(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                    const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                    const double* U_upper);
/* Optional: per-node penalty scales for the NEXT omc_relax_stage / omc_relax_batch with the same B (consumed by it).
 * Lets one batch try several penalties on the root (autotune) or give children their parent's value. */
int omc_set_node_rho_scales(omc_instance* h, int B, const double* rho_scale);
int omc_relax_solve(omc_instance* h);
/* ---- warm start from the parent's state (an addition of the engine; the reference cold-starts every model, OMC.jl:1482) ----------------------
 * A child is its parent plus one cut.  omc_state_pool_create reserves `capacity` final states on the device (about 24 n^2 + 8 (n k + |Omega| + m
 * + 16 n) bytes each: 0.27 MB at 100 x 100); it empties the pool and drops a Shor extension reserved earlier.  omc_relax_set_warm applies to
 * the NEXT omc_relax_stage / omc_relax_batch (or omc_relax_stage_shor / omc_relax_batch_shor, see below) with the same B and is consumed by
 * it: node b starts from pool entry load_from[b] (-1 or NULL: cold start) and its final state is stored in entry save_to[b] (-1 or NULL: not
 * stored).  The caller owns the numbering (e.g. a ring).  A warm node keeps its own base penalty (the parent's scaled duals are rescaled),
 * inherits Y, the duals of the two full cones, the column multipliers and the tracked block of the cone; the result is the same convex
 * program's optimum (same certificate), reached in fewer iterations.  An entry saved during a solve can be loaded by a later stage (or by
 * a node appended later), not by a node of the same staged batch.
 *
 * Shor mode.  omc_state_pool_reserve_shor(h, nq_max), called after omc_state_pool_create, extends every entry by the Shor state of a node
 * with at most nq_max minors: X, W, the multipliers of the paraboloids and of the order-(n+m) cone, Theta, and per minor the 15 duals of its
 * order-5 block and its five lifted values -- 8 (3 n m + m^2 + (n + m)^2 + 2 m + 20 nq_max) bytes per entry plus a 32-byte header (per-minor
 * arrays are stored with stride nq_max).  Calling it again reallocates and invalidates every entry; OMC_ERR_ARGUMENT without a pool or for
 * nq_max < 0; when the device cannot hold it the HIP out-of-memory code is returned and the pool stays as it was.  With the reservation the
 * next omc_relax_stage_shor / omc_relax_batch_shor honours omc_relax_set_warm (rank k = 1); without it the indices are ignored.  Rank k > 1
 * batches never use them (neither those the base engine serves nor those of the knob OMC_SHOR_EXPLICIT).
 * The library keeps, per entry, which mode saved it and a signature of the node's lists; the signature is set when the saving node is
 * harvested (a node that never finishes leaves the entry as it was).  At stage time load_from[b] is treated as -1 when the entry is empty,
 * was saved by the other mode (also in omc_relax_stage and omc_relax_append: a base node never starts from a Shor-mode state), holds more
 * than nq_max minors, or fails omc_shor_warm_compat against node b's lists; save_to[b] is treated as -1 when node b has more than nq_max
 * minors.  A node that loads starts from the parent's X, W, Theta and multipliers (rescaled to its own penalty); the blocks of minors the
 * parent did not have start with zero duals and rank-one lifted values from X; the eigen-state of the order-(n+m) cone starts cold.
 *   omc_shor_warm_compat      pure host function (no handle, no device): 1 for identical (minor list, SOC list) pairs, 2 when the parent's
 *                             minor list is a strict prefix of the child's and both SOC lists are the complement shorthand (n_soc = -1),
 *                             0 otherwise.  Lists in the wire format of omc_relax_stage_shor.
 *   omc_last_shor_warm_stats  out[4] of the last staged Shor batch, nodes appended to it included (omc_relax_append_shor applies the same
 *                             filter and adds to the counts): nodes loaded with an identical list, loaded through a prefix, loads
 *                             refused, states saved (counted as the nodes are harvested).
 *   omc_state_pool_fetch_shor the point of a Shor-mode entry, unscaled: *nq minors, X (n*m), Theta (m*m), V (5 per minor, as
 *                             omc_relax_fetch_shor_V); NULL pointers are skipped; OMC_ERR_ARGUMENT for an empty or base-mode entry. */
int omc_state_pool_create(omc_instance* h, int capacity);
int omc_state_pool_reserve_shor(omc_instance* h, int64_t nq_max);
int omc_relax_set_warm(omc_instance* h, int B, const int* load_from, const int* save_to);
int omc_shor_warm_compat(int64_t n_parent, const int64_t* parent_idx, int64_t n_soc_parent, const int64_t* parent_soc, int64_t n_child,
                         const int64_t* child_idx, int64_t n_soc_child, const int64_t* child_soc);
int omc_last_shor_warm_stats(omc_instance* h, int64_t out[4]);
int omc_state_pool_fetch_shor(omc_instance* h, int entry, int64_t* nq, double* X, double* Theta, double* V);
/* Asynchronous form of omc_relax_solve: submit returns at once (the solve runs on a worker thread of the library), poll reports
 * progress (running flag, nodes harvested so far, nodes staged), wait joins and returns the solve's return code (message via
 * omc_last_error on the waiting thread).  The reference's loop is serial (OMC.jl:700-719); with this the host can prepare the next
 * batch -- pop, prune (OMC.jl:1220-1244), build children -- while the device relaxes the current one.  One solve in flight per handle;
 * between submit and wait only omc_relax_poll may be called on the handle. */
int omc_relax_submit(omc_instance* h);
/* Appending nodes to a staged or RUNNING batch: the reference's loop pops from a queue that the children of relaxed nodes keep filling
 * (OMC.jl:700-719, 2520-2542); a staged batch was closed until round 3.  omc_relax_reserve(h, extra_nodes, max_cuts) makes the NEXT
 * omc_relax_stage size its per-node arrays for extra_nodes more nodes with at most max_cuts cuts each (default U bounds, same cut type and
 * parameters as the staged batch).  omc_relax_append(h, B, L, cut_x, cut_Uhat, cut_dir, load_from, save_to) adds B nodes in the wire format of
 * omc_relax_stage (load_from / save_to: warm-start pool entries as in omc_relax_set_warm, or NULL): before the solve starts, or while a
 * submitted solve is running -- the loop hands them to free slots at its next check -- and is refused once that solve has ended (the end is
 * decided under the same lock, so a node is either relaxed or refused, never lost).  Results: omc_relax_fetch returns every node, appended
 * ones behind the staged ones in the order they were appended.  A Shor batch takes omc_relax_append_shor instead (below). */
/* omc_relax_fetch_done: results of the nodes finished since the last call, in the order they finished -- callable while the submitted solve is
 * running (the other half of a queue-driven host loop: OMC.jl:700-719 pops, relaxes and pushes the children of one node at a time).
 * node_ids[i] indexes the staged + appended nodes; per node: U (n*k), lambda_min (2), breakpoint_x (n), Y (n*n) as in omc_relax_fetch (NULL: skipped). */
int omc_relax_fetch_done(omc_instance* h, int max_nodes, int* node_ids, double* objective, double* dual_bound, int* status, int* iters,
                         double* U, double* lambda_min, double* breakpoint_x, double* Y, int* n_out);
/* omc_relax_hold(h, 1) after staging: the submitted solve waits for omc_relax_append when it runs dry instead of ending (until omc_relax_hold(h, 0)
 * or the time limit of the parameters). */
int omc_relax_hold(omc_instance* h, int on);
/* Objective cutoff: the upper bound a branch-and-bound driver holds (its incumbent).  A node whose rigorous dual bound exceeds it at a
 * certificate check is pruned whatever it would converge to, so it ends there with status OMC_CUTOFF and dual_bound > cutoff (the cutoff as
 * read at that check; the comparison is strict and the engine adds no tolerance of its own).  The test comes after the OMC_OPTIMAL and
 * OMC_INFEASIBLE tests of the check and before stall, iteration cap and time limit; with kept certificates the node exports the multipliers
 * of the check that proved the prune.  A property of the handle: it applies to the staged batch, to every later batch and to appended nodes
 * until it is set again; +inf (the default) is off and then no node behaves differently; -inf and finite values are accepted, NaN or a NULL
 * handle returns OMC_ERR_ARGUMENT.  omc_relax_set_cutoff may be called at any time and from any thread, also between omc_relax_submit and
 * omc_relax_wait: it then takes effect at the first certificate check that starts after the call returns (one 8-byte copy on a stream of its
 * own; the running kernels read the value through a pointer).  A node that has already been returned is not revisited.
 * omc_last_cutoff_stats, of the last (or running) solve: out[0] nodes that ended OMC_CUTOFF, out[1] the sum of their iterations, out[2] calls
 * of omc_relax_set_cutoff taken while that solve ran, out[3] 0. */
int omc_relax_set_cutoff(omc_instance* h, double cutoff);
int omc_relax_get_cutoff(omc_instance* h, double* cutoff);
int omc_last_cutoff_stats(omc_instance* h, int64_t out[4]);
int omc_relax_reserve(omc_instance* h, int extra_nodes, int max_cuts);
int omc_relax_append(omc_instance* h, int B, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                     const int* load_from, const int* save_to);
/* Children by reference: the children of a finished node without a round trip of its cut list (create_matrix_cut_child_nodes,
 * OMC.jl:2520-2542).  A child is its parent plus one cut whose x is the parent's breakpoint_x and whose Uhat is the parent's U -- the two
 * vectors omc_relax_fetch_done copies back -- so its descriptor (2k + 1 new rows, at most one new column of the row basis) is built on the
 * device from the parent's, bit for bit what omc_relax_append builds on the host from the full cut list.  Base (disjunctive) mode.
 *   omc_branch_plan   (host only, no handle, no device) the children of one node: dirs[c * k + j] = direction code of child c in column j,
 *       the Cartesian product of the cut type's codes with the FIRST column varying fastest (Iterators.product; linear: left, right;
 *       linear2: left, middle, right; linear3: left, inner_left, inner_right, right), *n_children = 2^k, 3^k or 4^k of them.
 *       OMC_ERR_INVALID_ENUM for a bad cut type; OMC_ERR_ARGUMENT for NULL, k outside 1..8 or capacity < *n_children (which is still set).
 *   omc_relax_append_children   adds C nodes, child c = node parent_id[c] + one cut (x = that node's breakpoint_x, Uhat = its U, directions
 *       dirs[c * k ..]); load_from / save_to as in omc_relax_append (or NULL).  It is omc_relax_append for nodes given by reference: same
 *       lock and end-of-batch decision, descriptors before the node counter, same stream, same handling of the pool indices, the batch's
 *       default penalty.  The children get the consecutive ids *first_child_id ... in the order given and are ordinary appended nodes for
 *       every later call, this one included.  Before omc_relax_submit or while a submitted (or held) solve runs.  Every refusal is decided
 *       on the host before anything is written, leaves the batch as it was and names its cause: nothing staged, C <= 0, parent_id / dirs /
 *       first_child_id NULL: OMC_ERR_ARGUMENT; a Shor-mode batch: OMC_ERR_UNSUPPORTED; a parent that omc_relax_fetch_done has not returned
 *       (nor an ended solve harvested), the solve has ended, beyond the node capacity of omc_relax_reserve, a child with more cuts than
 *       Lmax, more rows than Rmax (R_parent + 2k + 1) or possibly more basis columns than rmax (min(n, r_parent + 1), r an upper bound
 *       the handle keeps per node), a pool index beyond the pool: OMC_ERR_ARGUMENT; a direction code the staged cut type does not have:
 *       OMC_ERR_INVALID_ENUM; n > 4096: OMC_ERR_UNSUPPORTED.  The strides are those fixed when the batch was staged (omc_relax_reserve).
 *   omc_relax_fetch_descriptor   one node's staged descriptor as the kernels read it, whole strides with their padding (tests, diagnostics):
 *       R, r, L (1 each); rkind, rcut, rbi, rbj, rrhs (Rmax); rcoef (Rmax * k); cutx (Lmax * n); Q (n * rmax).  Any pointer may be NULL.
 *       Rmax and rmax: omc_last_solver_info [7], [3]; Lmax = max(1, most cuts of a staged node, max_cuts of omc_relax_reserve).
 *       OMC_ERR_ARGUMENT for an id that is not a node of the batch. */
int omc_branch_plan(int cut_type, int k, int capacity, int8_t* dirs, int* n_children);
int omc_relax_append_children(omc_instance* h, int C, const int* parent_id, const int8_t* dirs, const int* load_from, const int* save_to,
                              int* first_child_id);
int omc_relax_fetch_descriptor(omc_instance* h, int node_id, int* R, int* rkind, int* rcut, int* rbi, int* rbj, double* rcoef, double* rrhs,
                               int* L, double* cutx, int* r, double* Q);
int omc_relax_poll(omc_instance* h, int* running, int* nodes_done, int* nodes_total);
int omc_relax_wait(omc_instance* h);
int omc_relax_fetch(omc_instance* h, double* objective, double* dual_bound, int* status, int* iters, double* Y,
                    double* U, double* X, double* Theta, double* lambda_min, double* breakpoint_x,
                    double* solve_time);

/* ---- relaxation with add_Shor_valid_inequalities = true (rank k = 1): OMC.jl:1431-1453 (keyword), 1503-1525 (W, V1, V2, V3),
 * 1755-1779 (rotated cones, Theta_jj = sum_i W_ij, one order-5 PSD block per minor), 1838-1846 (objective), called at OMC.jl:747-754 with
 * node.Shor_info = BBNodeShorInfo(constraints_indexes, SOC_constraints_indexes) (OMC.jl:37-40).
 *   n_shor[b]   number of minors of node b; shor_idx: their (i1, i2, j1, j2) tuples, 1-based Int64, 4 per minor, all nodes concatenated
 *               (node.Shor_info.constraints_indexes as Julia stores a Vector{NTuple{4,Int}});
 *   n_soc[b]    number of SOC coordinates of node b; soc_idx: (i, j) 1-based Int64 pairs concatenated (SOC_constraints_indexes);
 *               n_soc[b] = -1 (then the node contributes nothing to soc_idx) means "every coordinate that occurs in none of the node's
 *               minors" -- what the reference's driver always passes (OMC.jl:656-673, 2508-2517) -- without shipping n*m pairs per node.
 * Nodes with identical lists share one index structure on the device (the static mode hands every node the same list).
 * Everything else as omc_relax_stage; then omc_relax_solve / omc_relax_submit / _wait and omc_relax_fetch as usual (X and Theta are
 * the explicit variables of the Shor program), plus omc_relax_fetch_shor for W (OMC.jl:1908) and omc_relax_fetch_shor_V for V1, V2, V3.  Status, objective (recomputed as OMC.jl:1960-1967 does) and the certified dual bound as in the base mode.
 * Rank k > 1 (Xt, Wt, H, per-layer blocks, one order-(k+1) block per coordinate: OMC.jl:1491-1494, 1526-1551, 1780-1827): reference quirk Q5 -- the slack
 * that H cancels in W = sum Wt + 2 sum H makes every per-layer order-5 block satisfiable, so in that form the minors do not constrain (X, W); the
 * program has the value of the same program without its order-5 blocks and with W >= X^2 kept on their coordinates.  That program is what is solved
 * (same outputs); the lifted variables Xt, Wt, H, V1..V3 of the reference's result are an explicit extension of (X, W) (closed form, INTEGRATION.md;
 * the host mirror api.py builds it), checked against the reference's full constraint set in the tests. */
int omc_relax_stage_shor(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                         const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                         const double* U_upper, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc,
                         const int64_t* soc_idx);
int omc_relax_fetch_shor(omc_instance* h, double* W /* n*m per node, may be NULL */);
/* The lifted products the order-5 blocks use (results["V1"], ["V2"], ["V3"], OMC.jl:1909-1911, restricted to the entries that occur in a
 * block): 5 doubles per minor, in the node's minor order -- V1[i1,(j1,j2)], V1[i2,(j1,j2)], V2[(i1,i2),j1], V2[(i1,i2),j2],
 * V3[(i1,i2),(j1,j2)] -- nodes concatenated with stride 5 * max_b n_shor[b].  Kept only when requested BEFORE staging
 * (omc_set_shor_keep_V(h, 1): the copy costs 40 bytes per minor and node). */
int omc_set_shor_keep_V(omc_instance* h, int keep);
int omc_relax_fetch_shor_V(omc_instance* h, double* V);
int omc_relax_batch_shor(omc_instance* h, int B, const omc_relax_params* params, int cut_type, const int* L,
                         const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower,
                         const double* U_upper, const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc,
                         const int64_t* soc_idx, double* objective, double* dual_bound, int* status, int* iters, double* Y,
                         double* U, double* X, double* Theta, double* W, double* lambda_min, double* breakpoint_x,
                         double* solve_time);
/* penalties of the Shor-mode splitting, in the scaled variables (defaults 0.05, 0 = automatic per list: 75 n m / (4 n_shor) clamped to
 * [0.25, 40], 2; params->rho_scale multiplies rho) */
int omc_set_shor_penalties(omc_instance* h, double rho, double r4, double r5);
/* Appending nodes to a staged or RUNNING Shor batch (rank k = 1): the Shor form of omc_relax_reserve / omc_relax_append / omc_relax_fetch_done.
 *   omc_relax_reserve_shor(h, nq_max, extra_lists)  with omc_relax_reserve(h, extra_nodes, max_cuts) applies to the NEXT omc_relax_stage_shor and is
 *       consumed by it: the per-slot strides become nqmax = max(staged, nq_max) minors and max(staged, 2 nqmax) V1 / V2 keys, the group table
 *       gets extra_lists more entries, the per-node outputs (X, W, Theta, V when kept) are sized for staged + extra_nodes nodes.  Device memory
 *       on top of the staged batch: extra_lists x (4 (20 nq_max + n m + m + 3) + align16(n m + m) + 80) bytes of index room, 8 (2 n m + m^2
 *       + 5 nqmax [V kept]) bytes per extra node, and per slot 368 bytes per minor of stride (V3 and the three 15-entry arrays of the
 *       order-5 blocks) and 16 bytes per V1 / V2 key of stride, beyond what the staged lists need.
 *       Negative arguments: OMC_ERR_ARGUMENT.  Without this call a Shor batch is staged exactly as before (omc_relax_reserve alone gives room
 *       for nodes that carry a list the batch already knows).
 *   omc_relax_append_shor  adds B nodes in the wire format of omc_relax_stage_shor (default U bounds; load_from / save_to as in
 *       omc_relax_append, or NULL) before the solve or while a submitted solve runs; same lock and end-of-batch decision as omc_relax_append,
 *       so a node is either relaxed or refused.  A node whose (minor list, SOC list) pair the batch already knows -- staged or appended --
 *       shares that list's index structure and uses no list capacity (the reference's static mode needs extra_lists = 0); a new list takes one
 *       of the extra_lists.  Warm-start indices pass the filter of omc_relax_stage_shor and are counted into omc_last_shor_warm_stats, which
 *       accumulates over the batch.  Refused with OMC_ERR_ARGUMENT and a message naming the limit: nothing staged or the batch is not in Shor
 *       mode (omc_relax_append in turn refuses Shor batches); the solve has ended; beyond the node capacity; more cuts than reserved; a new list
 *       longer than nqmax; a new list when the list capacity is used up; warm-start indices without a pool that has its Shor extension; the
 *       argument errors of omc_relax_stage_shor.  Rank k > 1: OMC_ERR_UNSUPPORTED (a batch the base engine serves takes omc_relax_append).
 *       A refused call leaves the batch as it was.  Not recycled: the group of a list stays for the life of the batch.
 *   omc_relax_fetch_done_shor  X (n*m), W (n*m), Theta (m*m) per id, for node ids that omc_relax_fetch_done has already returned, while the
 *       solve runs (NULL pointers are skipped): the values omc_relax_fetch / omc_relax_fetch_shor give for the node after the solve.  An id out
 *       of range or not yet returned: OMC_ERR_ARGUMENT.
 * After the solve omc_relax_fetch, omc_relax_fetch_shor and omc_relax_fetch_shor_V (stride 5 nqmax) return every node, appended ones behind the
 * staged ones. */
int omc_relax_reserve_shor(omc_instance* h, int64_t nq_max, int extra_lists);
int omc_relax_append_shor(omc_instance* h, int B, const int* L, const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir,
                          const int64_t* n_shor, const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx,
                          const int* load_from, const int* save_to);
int omc_relax_fetch_done_shor(omc_instance* h, int n_ids, const int* node_ids, double* X, double* W, double* Theta);

/* ---- certificates: the multipliers behind a node's dual_bound, exported so that a host can re-evaluate the bound on its own -------------------
 * No counterpart in the reference (quirk Q2: it takes the primal value as node bound).  Base (disjunctive) mode, rank k <= 8, every cut type,
 * default or caller-supplied U bounds.  Off by default; with it off nothing is allocated and no kernel is added to a solve.
 *
 * Rows of a node, in this order (OMC.jl:1558-1683; the order of omc_relax_stage's host code and of the multipliers lam below):
 *   trace                          tr Y <= k                                                                     (1 row; its lam entry is unused)
 *   box, j = 0..k-1 outer, i inner -U_ij <= -lower_ij where lower_ij > -1 (`lo`), then U_ij <= upper_ij where upper_ij < 1 (`hi`)
 *   per cut l, per column j        x'U_j <= hi_j, then -x'U_j <= -lo_j  (piece table OMC.jl:1580-1678), and after the k columns the
 *   aggregated row                 x'Y x - sum_j slope_j x'U_j <= sum_j intercept_j                              (OMC.jl:1680-1683)
 * Every row reads <CY_r, Y> + <CU_r, U> <= rhs_r with CY_r = x x' for an aggregated row and 0 otherwise (the trace row stays in the simple set).
 * Q (n x r, orthonormal columns) spans the columns of every CU_r: modified Gram-Schmidt, twice, over the normalised nonzero columns in row
 * order, a vector kept when what is left of it exceeds 1e-10.
 *
 * Certificate of a node:
 *   Lam    nnz doubles, the instance's order (columns in order, observed rows ascending): the exact multipliers alpha_j = (I + gamma Y[O,O])^-1 a_j
 *          of the check (k_colprox mode 1); as a matrix Lam is n x m, zero off the support
 *   lam    R doubles (>= 0), one per row
 *   Q, r   the row basis
 *   Psi3   order r + k, symmetric, column-major with leading dimension r + k: rho [[Q3_11, Q3_12], [Q3_12', Q3_22]], Q3 = P_+(M3) - M3 the
 *          multiplier direction of the small cone [Q'YQ Q'U; U'Q I] >= 0, rho the penalty in force at that check
 *   bound  the value these multipliers give:
 *            M     = -gamma/2 Lam Lam' + sum_{aggregated rows} lam_r x_r x_r' - Q Psi3[0:r,0:r] Q'
 *            c_j   = (Q' sum_{r != trace} lam_r CU_r)_j - 2 Psi3[0:r, r+j]                                         (j = 0..k-1)
 *            bound = <A, Lam> - 1/2 ||Lam||_F^2 + sum_{i<k} min(eig_i(M), 0) - sum_j ||c_j|| - sum_{r != trace} lam_r rhs_r - tr Psi3[r:, r:]
 *          (eig_i ascending).  It is a lower bound on the relaxation optimum for ANY Lam with support in Omega, lam >= 0 and Psi3 >= 0:
 *          Fenchel's inequality for f, weak duality for the rows and the cone, and the minimum of the Lagrangian over the superset
 *          {0 <= Y <= I, tr Y <= k} x {||(Q'U)_j|| <= 1}.
 * Snapshot rule: a node's dual_bound is the largest RIGOROUS bound over its checks, which need not be the last one.  With certificates kept,
 * the check that raises the reported bound copies its multipliers (with the penalty of that check, before a bump decided at the same check
 * rescales anything), so the certificate fetched for a node is the one of the check that gave its dual_bound.
 *
 *   omc_relax_keep_certificates   on != 0: the omc_relax_stage calls that follow keep them (per slot 8 (2 + nnz + Rmax + (rmax + k)^2) + 8 bytes,
 *       per node of the capacity -- staged + omc_relax_reserve -- out[4] of omc_certificate_plan at the staged strides).  Refused
 *       (OMC_ERR_ARGUMENT) while a submitted solve runs.  While it is on omc_relax_stage_shor returns OMC_ERR_UNSUPPORTED (unless
 *       omc_relax_keep_shor_certificates is on: Shor mode has a layout and a switch of its own, below).
 *   omc_relax_fetch_certificate   for node ids that omc_relax_fetch_done has returned (while the solve runs) or that the ended solve has
 *       harvested (everything omc_relax_fetch returns).  Output i belongs to node_ids[i]; strides nnz (Lam), Rmax (lam), n * rmax (Q),
 *       (rmax + k)^2 (Psi3), with Rmax = info[7] and rmax = info[3] of omc_last_solver_info; R[i] and r[i] say how much of a stride is used (Q:
 *       n * r[i] doubles, Psi3: (r[i] + k)^2, both at the head of the stride).  Any output may be NULL.  OMC_ERR_ARGUMENT with a message for
 *       a batch staged without certificates, an id out of range or not finished, and a node that never reached a rigorous check.
 *   omc_certificate_plan          host only, no handle: out[6] = strides of Lam, lam, Q, Psi3 in doubles, bytes the arena holds per node, rmax --
 *       for nodes with at most max_cuts cuts and nonstandard_box_rows box rows beyond the k (k + 1) / 2 of the default bounds:
 *       Rmax = 1 + k (k + 1) / 2 + nonstandard_box_rows + max_cuts (2 k + 1), rmax = max(1, min(n, k + nonstandard_box_rows + max_cuts)).
 *       These are what a batch of such nodes is staged with unless its row vectors are linearly dependent (then rmax is smaller).
 *   omc_dual_bound_batch          the bound above for B nodes and caller-supplied multipliers, on the device: rows and Q on the host as
 *       omc_relax_stage builds them, the matrix M and the constants by a kernel of its own (Lam Lam' on the matrix cores for n > 144), the k
 *       smallest eigenvalues by the eigen-kernel a relaxation uses at order n.  The multipliers are evaluated as given (nothing is clamped).
 *       Strides: nnz, Rmax = the largest row count of the B nodes, n * rmax and (rmax + k)^2 with rmax = max(1, largest r of the B nodes);
 *       Psi3 per node as above (order r + k at the head of its stride), NULL = zero.  Q_out (n * rmax per node) and r_out (B) may be NULL.
 *       With Lam, lam, Psi3 and bound all NULL only Q_out / r_out are written, without a device call: a caller gets the basis first and
 *       forms Psi3 in it.  Stages nothing and leaves a staged batch as it is; refused while a submitted solve runs. */
int omc_relax_keep_certificates(omc_instance* h, int on);
int omc_relax_fetch_certificate(omc_instance* h, int n_ids, const int* node_ids, double* Lam, double* lam, int* R, double* Q, int* r,
                                double* Psi3, double* bound);
int omc_certificate_plan(int n, int k, int nnz, int max_cuts, int nonstandard_box_rows, int64_t* out);
int omc_dual_bound_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L, const double* cut_x,
                         const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower, const double* U_upper, const double* Lam,
                         const double* lam, const double* Psi3, double* Q_out, int* r_out, double* bound);

/* ---- Shor-mode certificates: the multipliers behind the dual_bound of a node relaxed with omc_relax_stage_shor, rank k = 1 --------------------
 * A switch of its own, independent of omc_relax_keep_certificates: with only that one on, omc_relax_stage_shor still returns
 * OMC_ERR_UNSUPPORTED; with this one on it stages, whatever the other says; this one has no effect on omc_relax_stage.  Rank k > 1 with this
 * switch on: omc_relax_stage_shor returns OMC_ERR_UNSUPPORTED (quirk Q5 makes the minors vacuous there).  Off by default; with it off nothing is
 * allocated, no kernel is added and a solve returns what it returned before, bit for bit.
 *
 * Certificate of a node.  All values in the engine's scaled variables (it solves the program of scale * A, whose optimum is scale^2 times the
 * node's), taken at the check that gave the node's dual_bound (the snapshot rule above, with the penalty of that check):
 *   scale  1 double
 *   bound  the reported (unscaled) dual_bound, bit for bit
 *   lam, Q, r, Psi3  as in the base certificate (rows and basis of the node; k = 1)
 *   Gam    15 doubles per minor: the corrected symmetric multiplier Gamma'_q of the order-5 block (rows: the constant 1, (i1,j1), (i1,j2),
 *          (i2,j1), (i2,j2)), upper triangle packed by columns -- (0,0)=0, (0,1)=1, (1,1)=2, (0,2)=3, (1,2)=4, (2,2)=5, (0,3)=6, (1,3)=7,
 *          (2,3)=8, (3,3)=9, (0,4)=10, (1,4)=11, (2,4)=12, (3,4)=13, (4,4)=14 -- stored entry-major: Gam[e * nq_stride + q], q in the order
 *          of the node's minor list, nq_stride the batch's stride (largest staged list, or nq_max of omc_relax_reserve_shor if larger)
 *   zeta   m doubles: max(rho r5 nu5_j, 0), the admissible multiplier of column j's paraboloid before the W-stationarity raises it
 *   xi     n x m column-major: the point at which the paraboloids are linearised
 *   Xbar   n x m column-major: the tangent point of the quadratic objective term
 *   nq     the node's own minor count
 * No Lam: Shor mode has no column multipliers of that kind; the dense multiplier of the order-(n+m) cone follows from the fields above.
 * The minor list and the SOC list are the caller's; the library does not hand them back.
 * Every field is an INPUT to a formula that gives a valid lower bound for any values (certificate.py: shor_dual_bound makes them admissible
 * first -- PSD part of every block, zeta and lam clamped at 0, PSD part of Psi3 -- then spreads what fails to cancel in V1 / V2 / V3, raises
 * zeta to what the W-stationarity needs, and returns -inf where mu_j = cT_j - zeta_j <= 0 meets a nonzero phi_j).  It is not a claim: nothing has
 * to be believed about how the library produced it.
 *
 * Memory: the arena holds out[7] of omc_shor_certificate_plan per node of the capacity (staged + omc_relax_reserve), 120 bytes per minor of
 * the stride plus 8 (2 n m + m + Rmax + (rmax + 1)^2) + 16; every slot holds out[8], the same plus 16.  At BASELINE config 3 (200 x 200,
 * 632 732 minors) that is about 76 MB per node and per slot.  OMC_ERR_ALLOC if it does not fit; the layout is not compressed.
 *
 *   omc_relax_keep_shor_certificates   on != 0: the omc_relax_stage_shor / omc_relax_batch_shor calls that follow keep them.  Refused
 *       (OMC_ERR_ARGUMENT) while a submitted solve runs.
 *   omc_relax_fetch_shor_certificate   for node ids that omc_relax_fetch_done has returned (while the solve runs) or any node after the solve,
 *       staged or appended (omc_relax_append_shor).  Output i belongs to node_ids[i]; strides 1 (scale, bound, R, r, nq), Rmax (lam), n * rmax
 *       (Q), (rmax + 1)^2 (Psi3), 15 * nq_stride (Gam), m (zeta), n * m (xi, Xbar); *nq_stride receives the stride.  Any output may be NULL.
 *       OMC_ERR_ARGUMENT with a message for a batch staged without the switch, an id out of range or not finished, and a node that never
 *       reached a rigorous check.
 *   omc_shor_certificate_plan          host only, no handle: out[10] = strides in doubles of lam, Q, Psi3, Gam, zeta, xi, Xbar, bytes the arena
 *       holds per node, bytes per slot, rmax (Rmax and rmax as omc_certificate_plan computes them).  OMC_ERR_UNSUPPORTED for k > 1. */
int omc_relax_keep_shor_certificates(omc_instance* h, int on);
int omc_relax_fetch_shor_certificate(omc_instance* h, int n_ids, const int* node_ids, double* scale, double* bound, double* lam, int* R, double* Q,
                                     int* r, double* Psi3, double* Gam, double* zeta, double* xi, double* Xbar, int* nq, int64_t* nq_stride);
int omc_shor_certificate_plan(int n, int m, int k, int64_t nq_stride, int max_cuts, int nonstandard_box_rows, int64_t* out);

/* ---- the Shor-mode bound of caller-supplied multipliers, on the device (rank 1) ---------------------------------------------------------
 * omc_shor_dual_bound_batch evaluates, for B nodes, the formula that certificate.py gives for a Shor-mode certificate (evaluate_shor for
 * sanitise = 0, shor_dual_bound for sanitise = 1).  Nodes, cuts and U bounds in the wire format of omc_dual_bound_batch; the lists in the wire
 * format of omc_relax_stage_shor (n_soc[b] = -1: every coordinate outside the minors); the multipliers in the layout of
 * omc_relax_fetch_shor_certificate, so that a fetched certificate goes straight back in: scale (1 per node), lam (stride Rmax), Psi3 (order
 * r + 1 at the head of a stride (rmax + 1)^2; NULL = zero), Gam (entry-major, Gam[b * 15 * nq_stride + e * nq_stride + q]; may be NULL when
 * every n_shor[b] is 0), zeta (stride m), xi and Xbar (stride n * m, column-major).  Rmax and rmax are taken over the B nodes as
 * omc_dual_bound_batch takes them, and the row basis is the one its query form returns.
 *   sanitise = 0  the multipliers as they are: spread of the V residuals with the shift by ||E||_F, the further shift by max(0, -lambda_min) of
 *                 the shifted block, zeta raised to what the W-stationarity needs, mu, phi, M, the rows, the smallest eigenvalue, ||c||.
 *   sanitise = 1  zeta clamped at 0 on the type-0/1 columns, lam clamped at 0, Psi3 replaced by its PSD part, and the blocks taken in two ways --
 *                 minus their negative part, and as given -- each followed by the steps above; the larger value is returned.
 * bound[b] is in the node's own scale (divided by scale^2) and is -INFINITY exactly where the formula is: a scale that is not positive and
 * finite (decided on the host: no view of that node reaches the device), mu_j <= 0 meeting a nonzero phi_j, anything not finite on the way.
 * defects (5 per node, may be NULL): gam_min_eig, v_residual, min_zeta (type-0/1 columns), min_lam, psi_min_eig of the input as given; the
 * first two are NaN for a node that was refused on the host and 0 for an empty list.  terms (4 per node, may be NULL), in the scaled
 * variables, of the evaluation that was returned: the constant, min(eig_0(M), 0), ||c||, min_j mu_j (bound scale^2 = constant + second - third);
 * NaN for a node refused on the host.
 * It stages nothing and uses buffers of its own: a staged or finished batch and its fetchable results stay exactly as they were.  Identical
 * (minor list, SOC list) pairs within a call share one index structure.  A node's result does not depend on B, on its position or on the
 * other nodes of the call.
 * OMC_ERR_ARGUMENT before any device call: NULL handle, B <= 0, a missing array, nq_stride below the largest n_shor[b], the list errors of
 * omc_relax_stage_shor, a solve in flight on the handle.  OMC_ERR_UNSUPPORTED: k > 1, 2^28 minors or more, n m >= 2^30.  OMC_ERR_ALLOC: the
 * buffers do not fit the device.
 *
 * omc_shor_dual_bound_plan (host only, no handle): the device bytes a call needs.  With nqs = nq_stride, nmb = ceil(nqs / 256), NP = n rounded
 * up to 16, nn4 = n^2 rounded up to 4, Rmax = 2 + nonstandard_box_rows + 3 max_cuts, rmax = max(1, min(n, 1 + nonstandard_box_rows +
 * max_cuts)), Lmax = max(max_cuts, 1), ps = (rmax + 1)^2, S = doubles of the eigen-kernel's slab at order n (0 where it works in LDS):
 *   node = 8 (1 + 15 nqs + m + 2 n m) + 8 (15 nqs [sanitise] + nmb) + 4 + 4 (20 nqs + n m + m + 3) + ((n m + m + 15) & ~15) + 120
 *          (the multipliers; the blocks minus their negative part and the per-block minima; the group index; one list's index structure)
 *   view = 8 (12 nqs + 2 nmb + n m + 2 m) + 4 m + 8 + 8 (2 NP^2 + nn4 + S) + 8 (2 Rmax + Lmax n + n rmax) + 8 (Rmax + ps + n rmax + n + 5)
 *          + 4 (4 Rmax + 9)
 *          (key residuals, the 8-plane scratch, partials, the dense multiplier, column constants and flags; matrices and slab; descriptors;
 *          lam, Psi3 and scratch of the assembly; its ints)
 * out[0] = node + ways * view (ways = 2 with sanitise, else 1), out[1] = B out[0], out[2] = node, out[3] = view, out[4] = ways, out[5] = S,
 * out[6] = Rmax, out[7] = rmax.  An upper bound: shared lists and nodes refused on the host need less.  OMC_ERR_UNSUPPORTED for k > 1 and
 * beyond the size limits above.
 * omc_last_shor_dual_bound_ms: event time of the kernels of the handle's last omc_shor_dual_bound_batch call, copies excluded. */
int omc_shor_dual_bound_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L, const double* cut_x,
                              const double* cut_Uhat, const int8_t* cut_dir, const double* U_lower, const double* U_upper, const int64_t* n_shor,
                              const int64_t* shor_idx, const int64_t* n_soc, const int64_t* soc_idx, int sanitise, int64_t nq_stride,
                              const double* scale, const double* lam, const double* Psi3, const double* Gam, const double* zeta, const double* xi,
                              const double* Xbar, double* bound, double* defects, double* terms);
int omc_shor_dual_bound_plan(int n, int m, int k, int B, int64_t nq_stride, int max_cuts, int nonstandard_box_rows, int sanitise, int64_t* out);
int omc_last_shor_dual_bound_ms(omc_instance* h, double* ms);

/* ---- the index structure of one Shor list, built on the host or on the device -------------------------------------------
 * Every Shor-mode entry point turns a node's list (nq tuples (i1, i2, j1, j2), 1-based, and its SOC list: n_soc = -1 for every entry, 0, or
 * n_soc pairs (i, j)) into the arrays its kernels index by.  The knob OMC_SHOR_INDEX_DEVICE_MIN = N > 0 (omc_tuning_set; default 0: every
 * list on the host) builds the lists with at least N minors on the device in omc_relax_stage_shor, omc_relax_append_shor and
 * omc_shor_dual_bound_batch; the arrays are bit-identical to the host's, the refusals and their messages the same.  Rank k > 1 always takes
 * the host path.  A staged batch keeps the value the knob had at its stage call.
 *
 * omc_shor_index_build: one list's structure, returned to host arrays.  where = 0: the host builder, where = 1: the device builder, whatever
 * the knob says.  Any output may be NULL; the arrays the caller gives hold at least
 *   mi 4 nq, kid 4 nq (both SoA, 0-based), cptr n m + 1, cent 4 nq, v1ptr 2 nq + 1, v1ent 2 nq, v2ptr 2 nq + 1, v2ent 2 nq, slackrow m ints ;
 *   eclass n m, ctype m bytes
 * of which nv1 + 1 / nv2 + 1 entries of v1ptr / v2ptr are written.  counts[4] = nq, nv1, nv2, kernels launched (0 on the host); r4: the
 * list's block penalty; hash: FNV-1a of its tuples.  It stages nothing and leaves a staged batch untouched.  OMC_ERR_ARGUMENT: NULL handle,
 * where not 0 / 1, a solve in flight on the handle, the list errors of omc_relax_stage_shor.  OMC_ERR_UNSUPPORTED: where = 1 with k > 1 (for
 * k > 1 the host gives the structure without minors of quirk Q5), 2^28 minors or more, n m >= 2^30.
 *
 * omc_shor_index_plan (host only, no device): what the shape fixes.  out[0..3] = 8-bit radix passes of the V1, V2, coordinate and duplicate
 * sorts (from the largest key the shape allows), out[4] = bytes of sort scratch for a list of nq minors, out[5] = ints (20 nq + n m + m + 3)
 * and out[6] = bytes (n m + m rounded up to 16) one built list takes in the staging room, out[7] = kernels launched per list (without the
 * scatter of explicit SOC pairs, one per chunk of max(n m, 1024) pairs), out[8] = items one workgroup sorts per pass.
 *
 * omc_last_shor_index_stats: out[5] = lists built on the host, lists built on the device, host milliseconds, device milliseconds (as the
 * caller sees them, waits included) since the last omc_relax_stage_shor call began, kernels launched by the last device build. */
int omc_shor_index_build(omc_instance* h, int where, int64_t nq, const int64_t* shor_idx, int64_t n_soc, const int64_t* soc_idx, int64_t* counts,
                         double* r4, uint64_t* hash, int* mi, int* kid, int* cptr, int* cent, int* v1ptr, int* v1ent, int* v2ptr, int* v2ent,
                         int* slackrow, uint8_t* eclass, uint8_t* ctype);
int omc_shor_index_plan(int n, int m, int64_t nq, int64_t* out);
int omc_last_shor_index_stats(omc_instance* h, double* out);

/* ---- alternating_minimization (OMC.jl:1979-2279), disjunctive mode, B problems at once, rank k <= 8 --------
 * U_initial n*k per problem; cuts as above (only the per-cut bounds on v = U'x are imposed, OMC.jl:2047-2093);
 * k > 1 adds the pair cones ||U_j1 +- U_j2|| <= sqrt 2 of OMC.jl:2029-2045.
 * Outputs: U n*k, V k*m, converged, n_iters, objectives (max_iters doubles per problem, NaN padded).
 * time_limit (seconds, OMC.jl:1999-2003, 2186-2189): <= 0 solves nothing (n_iters 0).  A positive limit is checked on the device's clock
 * at the top of every iteration, per problem; the first iteration always runs.  A problem stopped by the clock returns converged 0, n_iters =
 * iterations completed, U and V of the last completed iteration and every objective recorded.  Not enforced where the device does not
 * report its clock rate, and for limits that are not finite.                                                */
int omc_altmin_batch(omc_instance* h, int B, int cut_type, int reference_quirk_q1, const int* L,
                     const double* cut_x, const double* cut_Uhat, const int8_t* cut_dir, const double* U_initial,
                     double eps, int max_iters, double time_limit, double* U, double* V, int* converged,
                     int* n_iters, double* objectives, double* solve_time);

/* evaluate_objective(U * V) of the LAST omc_altmin_batch call (OMC.jl:920 `X_local = U * V`, 925-927), computed on the device from the
 * factors inside the altmin kernel: the driver compares it with the incumbent without forming X; X is built for the winner only. */
int omc_altmin_master_objectives(omc_instance* h, int B, double* objective);
/* The launch plan of omc_altmin_batch for problems of size n x m, rank k with at most max_cuts cuts per problem, computed on the host (no
 * device call, no handle).  nolds != 0: as under OMC_ALTMIN_NOLDS=1.  out[4] = kernel variant (1: rank 1, 2: ranks 2 - 4, 3: ranks 5 - 8),
 * dynamic LDS bytes of the launch (0 with the slab), bytes of global slab per problem (0 with LDS), rows of model_U per problem (Rmax).
 * OMC_ERR_UNSUPPORTED for k > 8, OMC_ERR_ARGUMENT for sizes that are not positive. */
int omc_altmin_plan(int n, int m, int k, int max_cuts, int nolds, int64_t* out);

/* ---- evaluate_objective (OMC.jl:2330-2359) for B matrices X (n*m each) --------------------------------- */
int omc_evaluate_objective(omc_instance* h, int B, const double* X, double* objective);

/* ---- separation / feasibility on caller-supplied (Y, U): OMC.jl:1272-1277 and 2466-2477 -----------------
 * eigvals[2*b..] two smallest eigenvalues of U U' - Y; x n per problem; feasible[b] = eigvals[0] >= -1e-6.
 * These four entry points return OMC_ERR_ARGUMENT for B <= 0.  The exact zero matrix (U U' = Y; Y = 0; X = 0) has eigenvalues 0, is
 * feasible, and gives the first coordinate vector as x and the first k coordinate vectors as U. */
int omc_separation_batch(omc_instance* h, int B, int breakpoints, const double* Y, const double* U,
                         double* eigvals, double* x, int* feasible);

/* ---- rounding glue: svd(M).U[:,1:k] of the symmetric PSD Y (OMC.jl:873) -------------------------------- */
int omc_round_Y_batch(omc_instance* h, int B, const double* Y, double* U_rounded);
/* svd(X).U[:, 1:k] for B matrices X (n x m, column-major): the rank-k rounding of an incumbent or of the zero-filled A
 * (OMC.jl:524, 564, 921).  Gram product X X' on the matrix cores, then the k dominant eigenvectors; sign as omc_round_Y_batch. */
int omc_left_singular_batch(omc_instance* h, int B, const double* X, double* U_out);

/* ---- the cone projections on their own (OMC.jl:1554-1556 are the cones they serve) -----------------------
 * Spectral clip of B symmetric matrices of order N (column-major, N*N doubles each):
 * P = V diag(min(max(lambda, lo), hi)) V'.  lo = 0, hi = +inf is the projection on the PSD cone; lo = 0, hi = 1 the clip of
 * 0 <= Y <= I.  evals (B*N, ascending) and V (B*N*N, columns in the order of evals) may be NULL.  V0 (may be NULL): an
 * orthonormal starting basis per matrix, e.g. the V of an earlier call on a nearby matrix (the solver's warm start).
 * algo: 0 = what a relaxation at this order uses under the instance's knobs, 1 = single-workgroup kernels, 2 = multi-workgroup.
 * N is independent of the instance's n and m; N >= 2; OMC_ERR_UNSUPPORTED above 4096.  The kernels clip at 0 from below:
 * OMC_ERR_UNSUPPORTED for lo != 0, and for evals / V where the single-workgroup path is the cold kernel, which returns P only
 * (orders 129 - 144 and above 1024). */
int omc_psd_project_batch(omc_instance* h, int B, int N, const double* M, double lo, double hi, int algo,
                          const double* V0, double* P, double* evals, double* V);
/* The column prox of the ADMM iteration on its own (block F of DESIGN.md section 3.1), for B inputs at once, through the launcher a
 * relaxation uses.  mode 0 (prox): per column j with observed rows O, B_j = I + gamma (Y[O,O] - gamma/(2 rho_f) a_old a_old'), cp = gamma^2 /
 * (2 rho_f); s >= 0 with ||(B_j + cp s I)^-1 a_j||^2 = s and alpha = (B_j + cp s I)^-1 a_j.  Y is the matrix whose blocks enter B_j (2 Y - Yp of
 * the iteration).  mode 1 (exact multipliers of the certificate): alpha = (I + gamma Y[O,O])^-1 a_j, objcol = a_j'alpha / 2, c0col = a_j'alpha -
 * ||alpha||^2 / 2; objcol = 1e300 where the factorization fails.
 * algo: 0 = the solver's dispatch under the instance's knobs; 1 = the dispatch without k_colprox_block (as under an OMC_COLPROX_BLOCK_MIN above
 * every column: k_colprox_pair, k_colprox_wide, k_colprox); 2 = k_colprox_block for every non-empty column whatever its length (no pair kernel).
 * Y: B*n*n column-major.  alpha_old: B*nnz (NULL = zeros), rho_f: B, s0: B*m starting values of s (NULL = cold) -- mode 0 only.  Outputs: alpha
 * (B*nnz); s (B*m, mode 0); objcol, c0col (B*m, mode 1); nfact (B*m, may be NULL): factorizations per column, -1 where the kernel that ran the
 * column does not count them (k_colprox_pair, k_colprox_wide) and for empty columns.  The nnz order is the instance's: columns in order,
 * observed rows ascending.  OMC_ERR_ARGUMENT (before any device call) for a NULL handle, a mode or algo out of range, B <= 0 or a missing
 * array.  Restages the instance: a staged batch is gone afterwards. */
int omc_column_prox_batch(omc_instance* h, int B, int mode, int algo, const double* Y, const double* alpha_old, const double* rho_f,
                          const double* s0, double* alpha, double* s, double* objcol, double* c0col, int* nfact);
/* The exact projection on the linear rows of the ADMM iteration (step 4 of k_global) on its own, for B problems at once, one wave each:
 * lam = argmin 1/2 l'G l - c'l over l >= 0, by the active-set method warm-started from lam0 (NULL = zeros).  G: B matrices R x R with
 * leading dimension Rmax (B*Rmax*Rmax doubles); c, lam0, lam: B*Rmax.  which: 0 = the routines the alternating-minimisation kernels use
 * (wave_nnqp), 1 = the ones k_global runs (wave_nnqp_g); the two give the same bits.  overflow (B): 1 where the passive set reached its
 * capacity of 64 rows with a violated row still outside it -- lam is then not the exact projection.  OMC_ERR_ARGUMENT (before any device
 * call) for a NULL handle or array, which out of range, B <= 0, or R outside 1..Rmax.  Does not touch a staged batch. */
int omc_row_project_batch(omc_instance* h, int B, int R, int Rmax, int which, const double* G, const double* c, const double* lam0,
                          double* lam, int* overflow);
/* Launch plan of k_colprox_block for columns of at most cmax observed rows (cmax <= n) under OMC_COLPROX_BLOCK_MIN = block_min, computed on the
 * host from the layout the kernel uses (no device call, no handle).  out[5] = the longest column whose tiles live in LDS; dynamic LDS bytes of
 * the launch that holds a column of cmax rows; its global slab in doubles (0: the tiles are in LDS); workgroups per CU by LDS; 1 if a column
 * of cmax rows is a block column (0: cmax < block_min, or beyond the kernel -- then the three numbers before are 0). */
int omc_colprox_plan(int n, int cmax, int block_min, int64_t* out);
/* out[5] of the multi-workgroup eigen-kernels in the last omc_relax_solve (base cone and big cone of Shor mode together), or of the last
 * omc_psd_project_batch (either algo): calls, most sweeps of one call (at the last check of a solve), calls that used up their sweep
 * budget without meeting the stop rule, most sweeps of one call overall, device microseconds of the last omc_psd_project_batch
 * (the kernels alone, transfers outside; 0 after a solve) */
int omc_last_cone_multi_stats(omc_instance* h, int64_t* out);
/* Separation, rounding and the left singular vectors (omc_separation_batch, omc_round_Y_batch, omc_left_singular_batch, and the separation
 * launch of every harvest of omc_relax_solve) on the multi-workgroup eigen-kernels: the plan at order n under OMC_PLAIN_MULTI_MIN =
 * plain_multi_min, from the layout the kernels use (host only, no device call, no handle).  out[6] = 1 if the order takes the path
 * (n >= max(145, plain_multi_min) and n <= 4096), rows padded to 16 (NP), columns padded to whole pairs of 16-column blocks (Ncp), blocks nb =
 * Ncp / 16, bytes of the per-slot slab, launches per call (30 (nb - 1) + 4).  The five numbers describe the layout at order n whether or not
 * the order takes the path. */
int omc_plain_multi_plan(int n, int plain_multi_min, int64_t* out);
/* Rotation threshold and stop rule of that path, on the relative cross product of two columns: a pair above it is rotated, a sweep that met
 * nothing above it is the last.  The cold kernel's threshold (1e-14). */
double omc_plain_multi_tau(void);
/* out[4] of that path: calls (matrices decomposed), most sweeps of one call, calls that used up the 30 sweeps without meeting the stop rule,
 * device microseconds of the eigen-kernel launches -- of the last omc_separation_batch, omc_round_Y_batch or omc_left_singular_batch (all
 * zero where the cold kernel ran), or of the harvests of the last omc_relax_solve (microseconds 0).  Counters of their own:
 * omc_last_cone_multi_stats keeps counting clip and certificate calls only. */
int omc_last_plain_multi_stats(omc_instance* h, int64_t* out);
/* The sweep budget omc_relax_solve gives the next multi-workgroup calls of a cone at a certificate check.  interval_max: most sweeps of
 * one call since the last check, 0 when that interval had no call.  What the last interval needed + 2, at most the full bound (30); the
 * full bound after an interval without a call (the next call starts from a stale basis). */
int omc_cone_multi_budget(int interval_max);
/* What omc_relax_solve does with the finished slots at a certificate check (host arithmetic only, no device call, no handle).
 * nlive: slots whose node keeps running; nfin: finished slots not yet harvested; pending: 1 when nodes wait for a slot; check_index: the
 * number of this check (from 1); async_min_live: live slots from which the harvest kernels run beside the next interval (<= 0: never).
 * NONE: the finished slots stay parked.  SYNC: harvest, wait, book and refill before the next iteration.  ASYNC: enqueue the harvest kernels
 * and go on; the bookkeeping and the refill happen at the next check.  With pending nodes a harvest falls on every third check, on every
 * check when fewer than 256 slots are live; without, on every twelfth; always when nothing is live. */
#define OMC_HARVEST_NONE 0
#define OMC_HARVEST_SYNC 1
#define OMC_HARVEST_ASYNC 2
int omc_harvest_plan(int nlive, int nfin, int pending, int check_index, int async_min_live);

/* ---- Shor minors ------------------------------------------------------------------------------------------
 * generate_rank1_matrix_completion_Shor_constraints_indexes (OMC.jl:2545-2612): the 2 x 2 minors (i1 < i2, j1 < j2) whose
 * four cells hold exactly p observed entries, for every p of `num_entries_present` in turn (values outside 0..4
 * contribute nothing, as in the reference), in the reference's push order; tuples are 1-based Int64, 4 per minor.
 *   omc_shor_count   : number of minors per list element.
 *   omc_shor_indexes : *count = total; the tuples are written only when out != NULL and capacity >= total.           */
int omc_shor_count(omc_instance* h, int n_classes, const int* num_entries_present, int64_t* count_per_class);
int omc_shor_indexes(omc_instance* h, int n_classes, const int* num_entries_present, int64_t capacity, int64_t* out,
                     int64_t* count);
/* generate_violated_Shor_minors (OMC.jl:2614-2640).  X is the reference's Array{Float64,3} of size (k, n, m)
 * (X[t,i,j] at t + k*(i + n*j)); `existing` = 4*n_existing Int64 (1-based) already imposed minors (setdiff!, OMC.jl:2626).
 * Output: the min(n_minors, #candidates) minors with the largest score sum_t |X[t,i1,j1] X[t,i2,j2] - X[t,i1,j2] X[t,i2,j1]|,
 * ordered as Julia orders (score, tuple) pairs with rev = true (ties: larger tuple first).                           */
int omc_violated_shor_minors(omc_instance* h, const double* X, int n_classes, const int* num_entries_present,
                             int64_t n_existing, const int64_t* existing, int n_minors, double* scores,
                             int64_t* minors, int* n_out);
/* device milliseconds and candidate count of the last omc_shor_indexes / omc_violated_shor_minors call */
int omc_shor_last_stats(omc_instance* h, double* ms, int64_t* candidates);
/* How the last omc_violated_shor_minors call selected: out[0] = 1 if it streamed (no key per candidate in memory; taken when 16 bytes per
 * candidate exceed the knob OMC_SHOR_SELECT_KB, default 1 GiB, 0 = never), out[1] = tiles of row pairs it walked, out[2] = compactions of
 * the survivor buffer, out[3] = bytes of candidate keys (materialised: 16 per candidate) or of the survivor buffer (streamed:
 * max(budget, 16 (K + 8192 + largest candidate count of one row pair)), K the number of minors returned) it asked the device for.  The
 * output scratch of the select, 16 (K + 8192 + 16) bytes on either path, is not included.  The results do not depend on the path. */
int omc_shor_last_select_stats(omc_instance* h, int64_t out[4]);

/* ---- multi-GPU: node-parallel B&B, one process per GPU ------------------------------------------------------
 * Nodes are independent given (A, indices, gamma): every rank holds its own omc_instance on its own device and relaxes its shard
 * of the popped nodes.  The only exchange of the loop (OMC.jl:700-1073: tree.best_upper_bound at 725 / 797 / 1225, the global
 * lower bound at 1207-1218) is a 16-byte MIN all-reduce of {incumbent upper bound, smallest open lower bound} per round, and --
 * only when the incumbent improved -- a broadcast of the new X from the rank that found it.  RCCL (librccl, loaded on first use)
 * over xGMI; the communicator lives in the handle.
 *   omc_comm_unique_id   : rank 0 creates the 128-byte id; the host language distributes it to the other ranks (any channel).
 *   omc_comm_init        : collective over all ranks, after every rank has created its instance on its device.
 *   omc_allreduce_bounds : in place; *owner (may be NULL) = smallest rank whose local ub equals the global minimum.
 *   omc_bcast_incumbent  : X (n*m, column-major) from rank `root` to every rank.
 *   omc_allgather_records: the small per-node records (status, objective, bound, eigenvalues, breakpoint vector, U) of every rank.       */
#define OMC_COMM_ID_BYTES 128
int omc_comm_unique_id(void* id_out);
int omc_comm_init(omc_instance* h, int rank, int world_size, const void* id);
int omc_allreduce_bounds(omc_instance* h, double* ub, double* lb, int* owner);
int omc_bcast_incumbent(omc_instance* h, int root, double* X);
/* all-gather of the per-node records a host driver needs on every rank to grow the same tree (OMC.jl:700-719 sees every relaxed node): `cnt` rows of
 * `width` doubles from this rank (counts may differ between ranks); out = rows of rank 0, rank 1, ... ; counts[r] = rows of rank r.  With this the
 * Julia host needs no second transport (MPI) beside the library's communicator. */
int omc_allgather_records(omc_instance* h, const double* rows, int cnt, int width, double* out, int out_capacity_rows, int* counts);
int omc_comm_destroy(omc_instance* h);

/* per-kernel accounting of the last omc_relax_solve: launches and HIP-event milliseconds per kernel class */
#define OMC_KERNEL_COLPROX 0
#define OMC_KERNEL_CONE 1
#define OMC_KERNEL_GLOBAL 2
#define OMC_KERNEL_CHECK 3
#define OMC_KERNEL_SETUP 4
#define OMC_KERNEL_SMALL 5
#define OMC_KERNEL_ACCEL 6
#define OMC_KERNEL_CONESUB 7   /* k_cone_sub: the cone block by tracking the dominant 16-dimensional subspace */
#define OMC_KERNEL_CHECK_COL 8     /* certificate: exact f(Y) (one factorization per column, k_colprox mode 1) */
#define OMC_KERNEL_CHECK_BUILD 9   /* certificate: Lagrangian matrix and constants (k_check_build) */
#define OMC_KERNEL_HARVEST 10      /* finished slots: feasible U, separation eigenvector (OMC.jl:2466-2477), copy to the per-node outputs */
#define OMC_KERNEL_SHOR_BIGCONE 11 /* Shor mode: PSD projection of the order-(n+m) matrix [Y X; X' Theta] */
#define OMC_KERNEL_SHOR_MINORS 12  /* Shor mode: order-5 blocks (projection in registers, duals) and the shared V1, V2, V3 */
#define OMC_KERNEL_SHOR_COLS 13    /* Shor mode: per-column step (paraboloid, X, W, Theta, duals of the big cone) */
#define OMC_KERNEL_NCLASS 14      /* OMC_KERNEL_CHECK = eigenvalues of the Lagrangian matrix + decisions */
/* info[8]: solve seconds, total Jacobi sweeps of k_cone, rho, r_max, LDS flags (cone, global, small), R_max */
int omc_last_solver_info(omc_instance* h, double* info);
/* Workgroups per CU that the HIP runtime reports (hipOccupancyMaxActiveBlocksPerMultiprocessor) for the iteration kernels, at the block
 * size and the dynamic LDS of the geometry last staged on this instance (error before the first stage).  out[OMC_RES_N]; -1 = the kernel is
 * not launched at this geometry.  A residency lost to registers or LDS shows here, not only in a profile.  No counterpart in the reference. */
#define OMC_RES_CONE_SUB 0        /* k_cone_sub<0>: the cone block */
#define OMC_RES_CONE_SUB_CERT 1   /* k_cone_sub<1>: certificate estimator */
#define OMC_RES_CONE_SUB_SEP 2    /* k_cone_sub<2>: separation vector */
#define OMC_RES_GLOBAL 3          /* k_global, LDS or L2-resident variant as planned */
#define OMC_RES_SMALL 4           /* k_small, likewise */
#define OMC_RES_COLPROX_PAIR 5
#define OMC_RES_COLPROX_WIDE 6
#define OMC_RES_COLPROX 7         /* one column per wave */
#define OMC_RES_CONE_WS 8         /* the k_cone_ws variant in use */
#define OMC_RES_CONE 9            /* k_cone (cold Jacobi) */
#define OMC_RES_N 10
int omc_kernel_residency(omc_instance* h, int* out);
/* out[8] of the last omc_relax_solve: calls of k_cone_sub, its power steps, calls that fell back to the full eigendecomposition,
 * seedings of the tracked subspace by the full kernel, fall-backs by cause (more than 12 positive Ritz values, step cap, Cholesky
 * breakdown), Rayleigh-Ritz passes */
int omc_last_subspace_stats(omc_instance* h, int64_t* out);
/* the same eight counters for the order-(n+m) cone of the last Shor-mode solve */
int omc_last_shor_subspace_stats(omc_instance* h, int64_t* out);
/* Tuning / diagnostic knobs (OMC_STREAMS, OMC_GRAPH_MAX, OMC_NO_COLPROX_PAIR, ...: the table is OMC_KNOBS in omc_api.cpp, each knob documented
 * at its field of struct Tuning).  The library reads the environment at omc_instance_create and nowhere else; omc_tuning_set overrides one knob of an
 * instance (value NULL restores its default; an unknown name is refused), omc_tuning_reload_env reads the environment again.  No counterpart in the reference (its knobs are the
 * Mosek parameters of OMC.jl:1482-1500). */
int omc_tuning_set(omc_instance* h, const char* name, const char* value);
int omc_tuning_reload_env(omc_instance* h);
/* diagnostic builds (-DOMC_STAMPS) only: accumulated s_memtime ticks per kernel phase of node 0; zeros otherwise */
int omc_debug_stamps(omc_instance* h, double* out32);
/* diagnostic builds only: per-slot counters, out[c * slots + b]: c = 0 colprox wave cycles, 1 factorizations, 2 cone cycles,
 * 3 cone calls, 4 global cycles, 5 small cycles (zeros otherwise) */
int omc_debug_diag(omc_instance* h, double* out);
/* accepted / rejected extrapolated points of the node last relaxed in every slot (diagnostics; needs accel = 1) */
int omc_debug_aa(omc_instance* h, int* accepted, int* rejected);
/* last primal / dual ADMM residuals of every node of the staged batch (diagnostics) */
int omc_debug_residuals(omc_instance* h, double* rp, double* rd);
/* ms of OMC_KERNEL_SETUP is the time of k_setup and of k_setup_gram (the rows' Gram matrix, which k_setup formed itself before it became a
 * kernel of its own beside the harvest): the work the class always timed.  launches and units count k_setup only. */
int omc_last_kernel_stats(omc_instance* h, int64_t* launches /*NCLASS*/, double* ms /*NCLASS*/,
                          int64_t* units /*NCLASS*/);
/* Host time of the last omc_relax_solve between its iterations (steady_clock on the solving thread), by piece: milliseconds and how often the
 * piece ran.  A check: the wait for its kernels and the done flags, the bookkeeping up to the decision what to harvest, the new slot list, the
 * drain of the timing events (after the next iteration has been enqueued).  A harvest: the first flags upload, enqueueing its kernels, the wait
 * for them with the second upload, the pool / queue bookkeeping, enqueueing the setup.  The last two are whole events: from the end of a check's
 * wait to the next iteration's enqueue (without / with a harvest).  After an asynchronous harvest (omc_harvest_plan) harvest_wait has no event
 * and harvest_book / setup_enqueue are stamped at the next check.  The last two entries are counts only (ms 0).  No counterpart in the reference. */
#define OMC_HOST_CHECK_WAIT 0
#define OMC_HOST_CHECK_SCAN 1
#define OMC_HOST_LIST 2
#define OMC_HOST_EVENT_DRAIN 3
#define OMC_HOST_HARVEST_FLAGS 4
#define OMC_HOST_HARVEST_ENQUEUE 5
#define OMC_HOST_HARVEST_WAIT 6
#define OMC_HOST_HARVEST_BOOK 7
#define OMC_HOST_SETUP_ENQUEUE 8
#define OMC_HOST_CHECK_TOTAL 9
#define OMC_HOST_HARVEST_TOTAL 10
#define OMC_HOST_ASYNC_HARVESTS 11   /* count only: harvests whose kernels ran beside the next interval (booked and refilled at the next check) */
#define OMC_HOST_QUIET_INTERVALS 12  /* count only: check intervals whose iterations enqueued the full eigen-kernel once instead of twice */
#define OMC_HOST_BODY_RECORDS 13     /* count only: event records the iterations enqueued on their streams (timing, fork, joins) */
#define OMC_HOST_BODY_WAITS 14       /* count only: stream waits the iterations enqueued (fork, joins, the wait for the main stream, the check's wait) */
#define OMC_HOST_NPHASE 15
int omc_last_host_phases(omc_instance* h, double* ms /*NPHASE*/, int64_t* count /*NPHASE*/);

#ifdef __cplusplus
}
#endif
#endif /* OMC_H */
