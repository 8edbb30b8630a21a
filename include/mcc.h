/*
 * mcc.h -- C ABI of the MI355X multi-camera bundle-adjustment hot path (libmcc.so).
 *
 * Drop-in boundary for MultiCameraCalibration::optimizeExtrinsics and its per-iteration
 * linearisation seam in the reference (yulong314/multi_camera_calibration):
 *
 *   mcc_create ........... replaces the problem state the reference keeps in _edgeList /
 *                          _vertexList / _objectPointsForEachCamera / _imagePointsForEachCamera /
 *                          _cameraMatrix / _distortCoeffs / _xi (include/opencv2/ccalib/
 *                          multicalib.hpp:207-214, mymulticalib.hpp:122-126, doubleSide.hpp:128-130)
 *                          once loadImages()+initialize() have built it.
 *   mcc_linearize_solve .. replaces the virtual computeJacobianExtrinsic(x, JTJ_inv, JTE, deltaX)
 *                          (multicalib.hpp:176 -> src/multicalib.cpp:593-703,
 *                          mymulticalib.hpp:164 -> src/mymulticalib.cpp:668-818,
 *                          doubleSide.hpp:133 -> src/doubleSide.cpp:434-581): one linearisation and
 *                          the normal-equation solve; JTJ_inv is never materialised.
 *   mcc_optimize ......... replaces the loop of optimizeExtrinsics (multicalib.hpp:155 ->
 *                          src/multicalib.cpp:462-507): undamped Gauss-Newton with the
 *                          0.95^(k+1) step factor and float32 state, driven on the device.
 *   mcc_project_error .... replaces the virtual computeProjectError(x) (multicalib.hpp:188 ->
 *                          src/multicalib.cpp:895-1006, src/mymulticalib.cpp:820-939,
 *                          src/doubleSide.cpp:640-769): per-edge float32 error sums in reference
 *                          order and the reference's meanReProjError.
 *   mcc_comm_* ........... multi-GPU: photo vertices sharded over ranks, one RCCL all-reduce of the
 *                          reduced camera system per Gauss-Newton step (no reference counterpart).
 *
 * Conventions: every function returns 0 on success or a negative MCC_E* code; the message is
 * in mcc_last_error() (thread-local).  Nothing throws across the ABI.  Inputs are deep-copied
 * to the device by mcc_create; output pointers are caller-allocated host memory.  One
 * mcc_problem per host thread; calls on one problem are serialised by the caller (the
 * reference is single-threaded and non-reentrant, src/multicalib.cpp:120).
 */
#ifndef MCC_H
#define MCC_H

#ifdef __cplusplus
extern "C" {
#endif

#define MCC_OK 0
#define MCC_EINVAL (-1)     /* bad argument / unsupported configuration          */
#define MCC_EHIP (-2)       /* HIP runtime error                                 */
#define MCC_ENOTPD (-3)     /* a normal-equation block is not positive definite  */
#define MCC_ECOMM (-4)      /* RCCL error                                        */
#define MCC_ENOMEM (-5)
#define MCC_ETIMEOUT (-6)   /* a device-side wait timed out (the m > 30 warm-solve helper)     */

/* Camera model / class semantics the linearisation follows. */
#define MCC_MODEL_PINHOLE 0     /* MyMultiCameraCalibration, cv::projectPoints (k1..k6,p1,p2,s1..s4) */
#define MCC_MODEL_OMNI 1        /* MultiCameraCalibration base class, cv::omnidir::projectPoints    */
#define MCC_MODEL_DOUBLESIDE 2  /* DoubleSideCalibration (pinhole), fixed cameras + ds transform    */

#define MCC_FRONT 0             /* MultiCameraCalibration::FRONT_PATTERN (multicalib.hpp:82) */
#define MCC_BACK 1              /* MultiCameraCalibration::BACK_PATTERN                      */

/* TermCriteria types as the reference tests them (src/multicalib.cpp:475-477). */
#define MCC_CRIT_COUNT 1
#define MCC_CRIT_EPS 2
#define MCC_CRIT_COUNT_EPS 3

typedef struct mcc_problem mcc_problem;

/* Problem description in the reference's layout.  Camera vertices 0..n_cams-1 (camera 0 is the
 * identity and is not optimised), photo vertices n_cams.. are given as photo indices
 * 0..n_photos-1.  Edges are in reference order (_edgeList).  Parameters follow buildParas
 * (src/multicalib.cpp:422-440): [cam1..cam(C-1), photo0..] x (rvec, tvec), or for DOUBLESIDE
 * (src/doubleSide.cpp:233-261): [ds, photo0..].  n_photos >= 1 and n_edges >= 1 (MCC_EINVAL
 * otherwise: the reference's mean error is 0/0 without observations).  A camera without
 * observations is accepted (a photo shard of a multi-GPU problem may lack one); if the whole
 * problem leaves one unobserved the solve reports MCC_ENOTPD.  At most 22 cameras
 * (global block m <= 128, the reduced solve's LDS-resident matrix) and 1024 corners per edge. */
typedef struct mcc_desc {
    int model;
    int n_cams, n_photos, n_edges;
    const int *edge_cam;     /* [E] camera vertex                                  */
    const int *edge_photo;   /* [E] photo index                                    */
    const int *edge_side;    /* [E] MCC_FRONT / MCC_BACK (NULL = all front)        */
    const int *edge_off;     /* [E] first corner of the edge in obj/img            */
    const int *edge_n;       /* [E] corners of the edge                            */
    const float *obj;        /* [3*corners] object points, float32                 */
    const float *img;        /* [2*corners] observed corners, float32              */
    int nd;                  /* distortion coefficients per camera: pinhole 4/5/8/12, omni 4 */
    const float *K;          /* [9*n_cams] camera matrices (row-major), float32     */
    const float *D;          /* [nd*n_cams] distortion, float32                    */
    const float *xi;         /* [n_cams] Mei xi (OMNI), else NULL                  */
    const double *ds_pose;   /* [16] PINHOLE: doubleSideTransform (CV_64F 4x4), used by BACK edges */
    const float *cam_pose;   /* [16*n_cams] DOUBLESIDE: fixed camera poses (CV_32F 4x4)            */
    int device;              /* HIP device ordinal                                 */
} mcc_desc;

int mcc_create(mcc_problem **out, const mcc_desc *desc);
void mcc_destroy(mcc_problem *p);
const char *mcc_last_error(void);

int mcc_nparams(const mcc_problem *p);            /* P of this (local) problem              */
int mcc_global_dim(const mcc_problem *p);         /* m: 6(C-1), or 6 for DOUBLESIDE         */

int mcc_set_params(mcc_problem *p, const float *x, int n);
int mcc_get_params(mcc_problem *p, float *x, int n);

/* One linearisation + normal-equation solve at the current parameters (no update).
 * delta[P], jte[P] (either may be NULL): the reference's deltaX and JTE. */
int mcc_linearize_solve(mcc_problem *p, double *delta, double *jte);

/* optimizeExtrinsics' loop (without the final computeProjectError).  x_inout[P] holds the
 * initial float32 parameters and receives the result.  iters / last_change may be NULL. */
int mcc_optimize(mcc_problem *p, int crit_type, int max_count, double eps, float *x_inout,
                 int *iters, double *last_change);

/* n unconditional Gauss-Newton iterations on the device-resident parameters, enqueued
 * asynchronously (bench / throughput path).  Use mcc_synchronize to wait.  The first call after
 * any other entry point switches the device state to free-running (one host round trip);
 * back-to-back calls only enqueue. */
int mcc_step(mcc_problem *p, int n);
int mcc_synchronize(mcc_problem *p);
/* Wait for the enqueued steps, then report a device-side failure they hit (MCC_ECOMM: a peer
 * exchange timed out; MCC_ENOTPD: a normal-equation block was not positive definite).  A
 * failing step sets the device loop's stop flag (the final solve of the step does, or the peer
 * exchange on a timeout), so the free-running steps after it are no-ops; a throughput caller
 * checks this once after its timed window (outside it: one small device-to-host copy).  The
 * error stays in the device state until an entry point rewrites it (mcc_set_params,
 * mcc_optimize, mcc_linearize_solve); after mcc_check has reported it, the next mcc_step also
 * rewrites it and continues from the current parameters. */
int mcc_check(mcc_problem *p);

/* computeProjectError(x): edge_err[E] (reference edge order, may be NULL), mean. */
int mcc_project_error(mcc_problem *p, const float *x, float *edge_err, double *mean);
/* the same with the quantities the reference prints (src/mymulticalib.cpp:898-937): each corner's
 * float32 L2 error corner_err[corners] (reference corner order: errorsVector, for the standard
 * deviation), totalError (the float32 sum of the per-edge sums in edge order) and totalNPoints
 * (2N per pinhole edge, N per omnidirectional one); every output may be NULL. */
int mcc_project_error_detail(mcc_problem *p, const float *x, float *edge_err, float *corner_err,
                             float *total_error, long long *total_points, double *mean);

/* ---- multi-GPU (RCCL over xGMI).  All ranks hold the same cameras and disjoint photo sets;
 * x of a rank is [global block, its photos].  The global block stays identical on all ranks. */
#define MCC_UNIQUE_ID_BYTES 128
int mcc_comm_unique_id(unsigned char *id /* [128] */);
int mcc_comm_init(mcc_problem *p, const unsigned char *id, int nranks, int rank);
/* greedy balance of photos over ranks by corner count (descending); rank_of_photo[n_photos] */
int mcc_partition_photos(int n_photos, int n_edges, const int *edge_photo, const int *edge_n,
                         int nranks, int *rank_of_photo);
/* collective helpers on the problem's communicator (device-side, blocking); over the peer
 * transport when it is on or when there is no RCCL communicator */
int mcc_comm_allreduce_max(mcc_problem *p, double *v);
int mcc_comm_barrier(mcc_problem *p);

/* ---- peer transport: the step's only exchange without RCCL.  The final arriving workgroup of
 * every rank writes its packed reduced camera system into every peer's inbox (device memory
 * mapped by IPC, over xGMI) in LL words (32 data bits + 32-bit epoch per 8-B store) and sums all
 * ranks' systems in rank order, so every rank solves identical bits in the same kernel; no
 * all-reduce launch and no k_solve launch per step.  Collective, in this order on every rank:
 *   mcc_peer_handle(p, h)            -> this rank's inbox handle; exchange them (file, MPI, ...)
 *   mcc_peer_init(p, all, n, rank)   -> maps the peers, runs a two-round handshake (all ranks
 *                                       agree: MCC_OK on every rank, or MCC_ECOMM on every rank)
 * after which the steps use it (mcc_peer_enable(p, 0) falls back to the RCCL communicator).
 * Works across devices and for several ranks on one device (no RCCL needed).  A rank that does
 * not deliver within MCC_PEER_TIMEOUT_MS (default 30000) fails the step with MCC_ECOMM. */
#define MCC_PEER_HANDLE_BYTES 64
#define MCC_PEER_MAX_RANKS 64
int mcc_peer_handle(mcc_problem *p, unsigned char *handle /* [64] */);
int mcc_peer_init(mcc_problem *p, const unsigned char *handles /* [64 * nranks], rank order */, int nranks,
                  int rank);
int mcc_peer_enable(mcc_problem *p, int on);

/* ---- diagnostics / measurement */
/* the warm solves since mcc_create: out[5] = {solves by refinement with the previous system's inverse,
 * refinement corrections in them, refinements that did not converge (the direct elimination ran
 * instead), direct solves for want of an inverse (an optimisation's first step(s), or the previous
 * system was not positive definite), steps that had to wait for the inverse's producer}.
 * m > 30 split step: k_solve refines with the inverse a resident helper kernel computes while the step
 * linearises; it waits for the helper as long as needed, up to MCC_WARM_TIMEOUT_MS (default 10000),
 * after which the step fails with MCC_ETIMEOUT.  m <= 30 (MCC_SMALL_WARM, default on; single GPU or the
 * peer transport): a spare workgroup of the step's linearisation launch inverts the previous system,
 * and the final solve refines with it (the fused step: with the previous launch's, two updates stale);
 * the last field counts fused steps whose final arriver waited for the spare to acknowledge its inputs,
 * with the same MCC_WARM_TIMEOUT_MS bound; the m <= 30 counters run only with MCC_SOLVE_STATS=1 at
 * mcc_create (their atomics cost ~0.5 us per fused step).  All zero when the problem takes the direct
 * elimination only
 * (m > 96, MCC_WARM=0, MCC_SMALL_WARM=0, RCCL on the fused step).  Which solve a step takes depends on
 * the systems only, never on timing. */
int mcc_solve_stats(mcc_problem *p, long long *out);
/* the last mcc_optimize as its caller saw it: host_ms[4] = {setup (parameters in, state reset), steps
 * (graph launches of kGraphSteps = 8 steps and the host's stop-test poll after each), finish (the
 * pending photo update flushed, parameters out), the whole call} in wall milliseconds; *device_ms =
 * HIP events from before the first step launch to after the last launched step; *launched = steps
 * launched (the ones after the stop test fired return at once); *iters = updates made; *polls = host
 * round trips to the stop test. */
int mcc_optimize_profile(mcc_problem *p, double *host_ms, double *device_ms, int *launched, int *iters,
                         int *polls);
/* per-corner float32 residuals fl32(obs - proj) at x, reference corner order [2*corners] */
int mcc_debug_residuals(mcc_problem *p, const float *x, float *res);
/* test only: the warm solves' injected delays and wait bound, as MCC_SPARE_DELAY_US / MCC_WARM_DELAY_US /
 * MCC_WARM_TIMEOUT_MS set them at mcc_create (a negative argument keeps the current value); the captured
 * step graphs are rebuilt.  Lets a test fail a step by a timeout and then run the same handle again. */
int mcc_debug_delays(mcc_problem *p, double spare_delay_us, double warm_delay_us, double warm_timeout_ms);
/* test / measurement: the m > 30 dense solve alone (k_solve's elimination), x = S^-1 r for a
 * packed SPD system [S upper triangle row-major, m(m+1)/2 | r, m] on `device`; with reps > 0 the
 * average device time of `reps` back-to-back launches (one workgroup each) in *us_per_solve; with
 * stamps (64 entries) the elimination's per-phase s_memtime stamps of the first launch. */
int mcc_debug_solve(int device, int m, const double *packed, double *x, int reps, double *us_per_solve,
                    long long *stamps);
/* average device time (ms) per launch of the linearisation kernel over the last
 * mcc_timing_begin/mcc_timing_end window (HIP events on the problem's stream), and launches.
 * Fused single-GPU problems (m <= 30 and at most two photos per CU: one kernel per step) time
 * the whole window of graph-launched steps with two events; split-step problems record an event
 * pair around the linearisation kernels (k_group, or k_prep + k_edge + k_photo) of every step and
 * one around the whole step, launched eagerly behind a ~5 ms device-side delay kernel, so that the
 * whole window is queued before the GPU reaches it and runs back to back (no host launch latency
 * between the kernels inside the event pairs). */
int mcc_timing_begin(mcc_problem *p);
int mcc_timing_end(mcc_problem *p, double *lin_ms_per_launch, double *step_ms, int *launches);
/* per-step time distribution: n_windows windows of `steps` free-running steps each, enqueued back to
 * back (graph-launched as mcc_step launches them) with a HIP event between windows; ms_per_window[i]
 * is window i's device time (a leading window, which would include the idle gap before the first
 * launch, is run and dropped).  *graph_launched = 1 when the steps ran as graphs. */
int mcc_timing_windows(mcc_problem *p, int n_windows, int steps, double *ms_per_window, int *graph_launched);
/* split-step problems: average device time (ms) per launch of the linearisation kernels alone
 * (k_group, or k_prep + k_edge + k_photo), `launches` of them in ONE captured graph bracketed by two
 * HIP events on the problem's stream -- the kernels back to back as the step graphs run them, with
 * no event between them (events recorded inside a captured graph carry no timestamps on HIP).  Each
 * launch re-applies the pending photo update and rewrites its operands (Y', z'), so the parameters and
 * those operands are restored after the window: the next step continues the trajectory it would have
 * taken without the probe (the Schur slots and photo sums the probe leaves are outputs the next step
 * rewrites before reading).  MCC_EINVAL for a fused-step problem. */
int mcc_timing_linearize(mcc_problem *p, int launches, double *ms_per_launch);
/* average time (ms) of the step's data-path exchange over the same window, and the exchanges:
 * RCCL all-reduces by HIP event pairs around each ncclAllReduce, the peer transport by the
 * device's own s_memrealtime ticks from the first send to the rank-ordered sums (in-kernel, so
 * it includes waiting for the slowest rank).  0 exchanges on a single rank. */
int mcc_timing_exchange(mcc_problem *p, double *ms_per_exchange, int *exchanges);
/* diagnostic build only (libmcc_diag.so, -DMCC_DIAG): first call arms per-phase s_memtime
 * stamps (k_linearize; split step: k_photo per group, k_prep, k_edge rows), later calls copy
 * [32 * n_photos] stamps (then k_schur's [8 * grid]) out
 * (others: MCC_EINVAL) */
int mcc_debug_stamps(mcc_problem *p, long long *out, int n);
/* static facts about the problem for roofline accounting */
int mcc_problem_stats(const mcc_problem *p, long long *corners, long long *edges,
                      long long *photos, long long *alg_bytes_per_step);
/* which step the problem runs: *split_step = 0 for the fused single-kernel step (m <= 30 and at
 * most two photo workgroups per CU, or MCC_FUSED=1), 2 for the split step with its linearisation
 * as one group kernel (k_group, k_schur, [k_solve]), 3 for that group kernel with the reduction and
 * the m <= 30 solve folded into its launch (one k_group launch per step; MCC_GFOLD=0 gives 2), 1 for
 * the split step's three-kernel form
 * (k_prep, k_edge, k_photo, k_schur, [k_solve]; MCC_GROUP=0); *photo_groups = the groups'
 * workgroups (split step).  The choice
 * depends on the device's CU count (fused iff m <= 30 and n_photos <= 2 x CUs: 512 on MI355X), and
 * the two paths sum the normal equations in different orders, so the last FP64 bits of a step (and
 * in rare cases a float32 ulp of the state) depend on the device model; MCC_FUSED pins it. */
int mcc_problem_path(const mcc_problem *p, int *split_step, int *photo_groups);

/* ---- pose seeding: cv::solvePnP (SOLVEPNP_ITERATIVE) as host/pnp.cpp restates it, for a whole batch
 * of corner views in one launch (one wavefront per view, the Levenberg-Marquardt loop on the device).
 * The sequence and the LM policy are mcc::pnp::solvePnP's (include/mcc_pnp.hpp); the Jacobian is
 * analytic where the host takes central differences, so the two agree at the minimum, not bit for bit.
 * A view's result depends on that view only, never on the rest of the batch.  Pinhole model of
 * cv::projectPoints with D = k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]: nd is 0, 4, 5, 8 or 12.  At
 * most 1024 corners per view. */
typedef struct mcc_pnp_desc {
    int n_views;
    const int *view_off;     /* [n_views+1] corner offsets                          */
    const double *obj;       /* [3*corners] object points                           */
    const double *img;       /* [2*corners] observed corners (pixels)               */
    const int *view_cam;     /* [n_views] camera of each view, or NULL (camera 0)   */
    int n_cams;
    const double *K;         /* [9*n_cams] camera matrices (row-major)              */
    const double *D;         /* [nd*n_cams] distortion (may be NULL when nd is 0)   */
    int nd;
    int max_iter;            /* LM iterations at most (the host's is 50); 0 = return the closed-form initial pose */
    int device;
} mcc_pnp_desc;

#define MCC_PNP_SOLVED 0       /* rvec, tvec and rms (pixels) are set                               */
#define MCC_PNP_TOO_FEW 1      /* fewer than 4 points, or fewer than 6 off a plane: rms is -1       */
#define MCC_PNP_DEGENERATE 2   /* collinear points, a rank-deficient homography or a non-finite result: rms is -1 */

/* rvec[3*n_views], tvec[3*n_views], rms[n_views], status[n_views] (MCC_PNP_*); a view that is not
 * solved gets a zero pose and never fails the batch.  MCC_EINVAL, before any device work, for a null
 * pointer, n_views <= 0, a view_off that decreases, an nd outside the set, a view_cam out of range or
 * a view of more than 1024 corners.  device_ms (may be NULL): the launch alone, by HIP events. */
int mcc_solve_pnp_batch(const mcc_pnp_desc *d, double *rvec, double *tvec, double *rms, int *status,
                        double *device_ms);

/* ---- pinhole intrinsics: cv::calibrateCamera for one camera.  The returned K, D and view poses are
 * the least-squares minimum of the reprojection error through cv::projectPoints' model (k1 k2 p1 p2
 * [k3 [k4 k5 k6]]; no thin-prism or tilt terms), found by Levenberg-Marquardt on the device: one
 * wavefront per view, the block-arrow elimination per trial, sums in view order (two calls give the
 * same bits).  Bit parity with OpenCV is not claimed.  Flags carry cv::CALIB_*'s values; any other bit
 * is MCC_EINVAL. */
#define MCC_CALIB_USE_INTRINSIC_GUESS 1
#define MCC_CALIB_FIX_ASPECT_RATIO 2      /* fx = a fy with a = fx / fy of the input K; only fy is free */
#define MCC_CALIB_FIX_PRINCIPAL_POINT 4
#define MCC_CALIB_ZERO_TANGENT_DIST 8     /* p1 = p2 = 0, fixed */
#define MCC_CALIB_FIX_FOCAL_LENGTH 16
#define MCC_CALIB_FIX_K1 32
#define MCC_CALIB_FIX_K2 64
#define MCC_CALIB_FIX_K3 128
#define MCC_CALIB_FIX_K4 2048
#define MCC_CALIB_FIX_K5 4096
#define MCC_CALIB_FIX_K6 8192
#define MCC_CALIB_RATIONAL_MODEL 16384    /* k4 k5 k6 are free (nd = 8); without it they keep their input values */

#define MCC_CALIB_CONVERGED 0   /* |x_new - x_old| / |x_old| < eps after an accepted step          */
#define MCC_CALIB_COUNT 1       /* max_count accepted steps                                         */
#define MCC_CALIB_STALLED 2     /* ten rejected trials in a row; the best parameters are returned   */

typedef struct mcc_calib_desc {
    int n_views;
    const int *view_off;     /* [n_views+1] corner offsets; 4 to 1024 corners per view */
    const double *obj;       /* [3*corners] object points                              */
    const double *img;       /* [2*corners] observed corners (pixels)                  */
    int image_width, image_height;
    int flags;               /* MCC_CALIB_*                                            */
    int nd;                  /* 4, 5 or 8 distortion coefficients (4: k3 stays 0)      */
    int crit_type;           /* MCC_CRIT_*; cv::calibrateCamera's default is COUNT_EPS, 30, DBL_EPSILON */
    int max_count;           /* accepted steps at most (MCC_CRIT_EPS alone: 1000)      */
    double eps;
    int device;
    int *trials;             /* out, may be NULL: trials run (one k_pc_lin + k_pc_try pair each, accepted or not) */
} mcc_calib_desc;

/* The 0/1 mask of free slots over fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 that flags and nd give (under
 * FIX_ASPECT_RATIO fx is 0: it follows fy).  MCC_EINVAL for an unknown flag bit or a bad nd. */
int mcc_calib_mask(int flags, int nd, int *mask /* [12] */);

/* cv::initCameraMatrix2D: the closed-form K (Zhang's constraints on every view's homography, principal
 * point at the image centre) for planar targets; host only.  aspect_ratio > 0 forces fx = aspect_ratio fy,
 * 0 leaves both free.  Uses n_views, view_off, obj, img and the image size of the descriptor.  MCC_EINVAL
 * when an object point has Z != 0; MCC_ENOTPD when the views do not determine the focal lengths. */
int mcc_init_camera_matrix(const mcc_calib_desc *d, double aspect_ratio, double *K /* [9] */);

/* K[9] and D[nd] are in/out: the start with USE_INTRINSIC_GUESS (which a non-planar target requires),
 * otherwise only the aspect ratio under FIX_ASPECT_RATIO is read from them and the start is
 * mcc_init_camera_matrix's K with zero distortion (a fixed slot then stays at that start).  The pose seeds are one internal mcc_solve_pnp_batch.  rvec[3*n_views], tvec[3*n_views],
 * view_rms[n_views] (each view's RMS over its corners), rms = sqrt(sum |e|^2 / corners), iterations
 * (accepted steps), status (MCC_CALIB_*) and device_ms (HIP events around the whole loop, the host's reads of
 * the loop state between batches of trials included) may each be NULL.
 * MCC_EINVAL, before any device work, for a null pointer, n_views <= 0, a view_off that decreases, a view
 * of fewer than 4 or more than 1024 corners, a bad nd, an unknown flag bit, a zero focal length under
 * FIX_ASPECT_RATIO, or Z != 0 without a guess. */
int mcc_calibrate_camera(const mcc_calib_desc *d, double *K, double *D, double *rvec, double *tvec,
                         double *view_rms, double *rms, int *iterations, int *status, double *device_ms);

/* ---- pinhole stereo pair: cv::stereoCalibrate.  View v is seen by both cameras (img1, img2: the same
 * corners in the same order); camera 2 sees it at R2 = R R_v, t2 = R t_v + T, where (R_v, t_v) is its pose in
 * camera 1 and R = exp(om).  The unknowns are the poses, the rig (om, T) and 12 intrinsic slots per camera:
 * 30 global slots om T | fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 of camera 1 | the same of camera 2.  The
 * result is the least-squares minimum of both cameras' reprojection error through cv::projectPoints' model
 * under the flags, by mcc_calibrate_camera's Levenberg-Marquardt policy on the device (sums in view order:
 * two calls give the same bits).  Bit parity with OpenCV is not claimed.
 * Flags: the MCC_CALIB_* above, applied to both cameras (under FIX_ASPECT_RATIO each camera's fx follows its
 * own fy by its own input ratio), and the three below; any other bit is MCC_EINVAL. */
#define MCC_CALIB_FIX_INTRINSIC 256              /* all 24 intrinsic slots stay at their input values */
#define MCC_CALIB_SAME_FOCAL_LENGTH 512          /* camera 2's fx, fy follow camera 1's; the start is the inputs' mean */
#define MCC_CALIB_USE_EXTRINSIC_GUESS (1 << 22)  /* R, T on input are the rig's start */

typedef struct mcc_stereo_calib_desc {
    int n_views;
    const int *view_off;     /* [n_views+1] corner offsets; 4 to 1024 corners per view */
    const double *obj;       /* [3*corners] object points                              */
    const double *img1;      /* [2*corners] camera 1's corners (pixels)                */
    const double *img2;      /* [2*corners] camera 2's                                 */
    int image_width, image_height;
    int flags;               /* MCC_CALIB_*                                            */
    int nd;                  /* 4, 5 or 8 distortion coefficients, both cameras        */
    int crit_type;           /* MCC_CRIT_*; cv::stereoCalibrate's default is COUNT_EPS, 30, 1e-6 */
    int max_count;           /* accepted steps at most (MCC_CRIT_EPS alone: 1000)      */
    double eps;
    int device;
    int *trials;             /* out, may be NULL: trials run (one k_ps_lin + k_ps_try pair each, accepted or not) */
} mcc_stereo_calib_desc;

/* The 0/1 mask of free slots over the 30 global slots, and for every slot the slot it follows (-1: none):
 * fx follows its camera's fy under FIX_ASPECT_RATIO; under SAME_FOCAL_LENGTH camera 2's fy follows camera
 * 1's fy and its fx camera 1's fx (or its own fy by its own ratio with FIX_ASPECT_RATIO).  A slot that
 * follows another is not free.  Host only.  MCC_EINVAL for an unknown flag bit or a bad nd. */
int mcc_stereo_calib_mask(int flags, int nd, int *mask /* [30] */, int *tie /* [30] */);

/* The rig's start from both cameras' poses of every view (rvec, tvec [3*n_views] each), cv::stereoCalibrate's
 * rule: the component-wise median over the views of the rotation vector of R_2v R_1v^T and of
 * t_2v - R_2v R_1v^T t_1v (the middle value, or the mean of the middle two).  Near a half turn the views' vectors
 * are first moved to one side of pi (r and r (1 - 2 pi / |r|) are the same rotation), so |om| may exceed pi; away
 * from it the result is the plain median.  Host only. */
int mcc_stereo_init_extrinsics(int n_views, const double *rvec1, const double *tvec1, const double *rvec2,
                               const double *tvec2, double *om /* [3] */, double *T /* [3] */);

/* E[9] = [T]x R and F[9] = K2^-T E K1^-1, scaled so that F[8] = 1 when it is not 0, as mcc_stereo_calibrate
 * returns them (each may be NULL).  Host only. */
int mcc_stereo_epipolar(const double *R /* [9] */, const double *T /* [3] */, const double *K1 /* [9] */,
                        const double *K2 /* [9] */, double *E, double *F);

/* K1[9], D1[nd], K2[9], D2[nd] are in/out.  With FIX_INTRINSIC or USE_INTRINSIC_GUESS they are the start
 * and both cameras' pose seeds come from one internal mcc_solve_pnp_batch; otherwise two internal
 * mcc_calibrate_camera calls (the per-camera flags, the caller's criteria) give the intrinsics and the seeds,
 * and only the aspect ratio under FIX_ASPECT_RATIO is read from K1, K2.  The rig starts at R[9], T[3] with
 * USE_EXTRINSIC_GUESS, else at mcc_stereo_init_extrinsics'; the view poses start at camera 1's.
 * Out, each may be NULL: R[9], T[3], E[9] = [T]x R, F[9] = K2^-T E K1^-1 scaled to F[8] = 1 when that is
 * not 0 (E and F on the host), rvec / tvec [3*n_views] (camera 1's), view_rms[2*n_views] (view v's RMS in
 * camera 1, then in camera 2), rms = sqrt(sum |e|^2 / (2 corners)), iterations, status (MCC_CALIB_*),
 * device_ms.  MCC_EINVAL, before any device work, for a null pointer, n_views < 1, a view of fewer than 4
 * or more than 1024 corners, a bad nd, an unknown flag bit, a zero focal length in K1 or K2 under
 * FIX_INTRINSIC or FIX_ASPECT_RATIO, or USE_EXTRINSIC_GUESS without R and T; a view without a pose seed
 * fails the call with its index and camera. */
int mcc_stereo_calibrate(const mcc_stereo_calib_desc *d, double *K1, double *D1, double *K2, double *D2,
                         double *R, double *T, double *E, double *F, double *rvec, double *tvec,
                         double *view_rms, double *rms, int *iterations, int *status, double *device_ms);

/* ---- pinhole rectification: cv::undistortPoints, cv::initUndistortRectifyMap + cv::remap, cv::undistort and
 * cv::stereoRectify through cv::projectPoints' model, for the K, D, R, T that mcc_calibrate_camera and
 * mcc_stereo_calibrate return.  DESIGN.md 7i states every rule; where it and OpenCV differ, it is the
 * specification.
 *
 * D = k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] with nd in {0, 4, 5, 8, 12} as in mcc_pnp_desc; D == NULL or
 * nd == 0 is zero distortion; the tilted sensor (nd = 14) is MCC_EINVAL.  K, R and P are row-major doubles:
 * K and R 3 x 3, P with ld doubles per row (3, or 4 for the 3 x 4 P1 / P2 of mcc_stereo_rectify: only its
 * first three columns are read).  R == NULL is the identity; P == NULL is the identity for points and K for
 * maps.  Images are 8-bit with 1 or 3 interleaved channels and a row stride in bytes; bytes of a destination
 * row past width * channels are never written.
 *
 * MCC_EINVAL with a message, before any device work, for a null required pointer, n < 0, a size that is not
 * positive or is above 32767, channels other than 1 or 3, a stride shorter than a row, a bad nd, ld or map
 * type, a zero focal length, a singular P R, or iterations outside 1..1000. */

/* the map types of include/mcc_omnidir.h (MCC_OMNI_MAP_*) under model-neutral names; the encoding is the one
 * documented there: MCC_MAP_FLOAT is two float[width * height] (u, v); MCC_MAP_FIXED is CV_16SC2 + CV_16UC1,
 * with iu = cvRound(32 u), iv = cvRound(32 v): map1 = ((short)(iu >> 5), (short)(iv >> 5)) -- the cast wraps --
 * and map2 = (iv & 31) * 32 + (iu & 31) */
#define MCC_MAP_FLOAT 1
#define MCC_MAP_FIXED 2

#define MCC_CALIB_ZERO_DISPARITY 1024   /* cv::CALIB_ZERO_DISPARITY (mcc_stereo_rectify) */

/* cv::undistortPoints: n pixels src[2n] -> dst[2n].  Per point x0 = (u - cx) / fx, y0 = (v - cy) / fy, then
 * `iterations` rounds of the fixed-point inverse of the distortion (x, y) <- ((x0, y0) - tangential and prism
 * terms at (x, y)) / radial factor at (x, y), then (X, Y, W) = R (x, y, 1), (x, y) = (X, Y) / W, then
 * (P00 x + P01 y + P02, P10 x + P11 y + P12) / (P20 x + P21 y + P22).  mcc_solve_pnp_batch uses 20 rounds;
 * OpenCV's 5 leave about 1e-2 px on a camera with k1 = -0.25.  n == 0 touches nothing.  device_ms (may be
 * NULL): the kernel alone, by HIP events. */
int mcc_undistort_points(int n, const double *src, const double *K, const double *D, int nd, const double *R,
                         const double *P, int ld, int iterations, int device, double *dst, double *device_ms);

/* cv::initUndistortRectifyMap for a width x height destination: pixel (j, i) reads the source at
 * u = fx xd + cx, v = fy yd + cy, where (xd, yd) is the distortion of (X, Y) / W, (X, Y, W) = (P R)^-1 (j, i, 1)
 * (the inverse on the host).  MCC_MAP_FLOAT writes two float[width * height], MCC_MAP_FIXED
 * short[2 * width * height] and unsigned short[width * height].  device_ms as above. */
int mcc_init_undistort_rectify_map(const double *K, const double *D, int nd, const double *R, const double *P,
                                   int ld, int width, int height, int map_type, int device, void *map1,
                                   void *map2, double *device_ms);

/* cv::stereoRectify; host only, no device call.  Camera 2 sees a point X of camera 1's frame at R X + T
 * (mcc_stereo_calibrate's R, T).  flags is 0 or MCC_CALIB_ZERO_DISPARITY; alpha < 0 keeps the focal length
 * (no scaling), 0 <= alpha <= 1 scales between "only valid pixels" (0) and "every source pixel kept" (1);
 * new_width == 0 takes the image size.  Out, each may be NULL: R1[9], R2[9] (camera frame -> rectified frame),
 * P1[12], P2[12] (3 x 4), Q[16] (disparity to depth: Q (x, y, d, 1) ~ the point in camera 1's rectified frame,
 * d = x1 - x2, or y1 - y2 for a vertical pair), roi1[4], roi2[4] (x, y, width, height of the all-valid
 * region).  The baseline lies along x or along y of the rectified frame, whichever is nearer: P2[3] or P2[7]
 * carries T f.  MCC_EINVAL also for T = 0, alpha > 1 and an unknown flag. */
int mcc_stereo_rectify(const double *K1, const double *D1, const double *K2, const double *D2, int nd,
                       int width, int height, const double *R, const double *T, int flags, double alpha,
                       int new_width, int new_height, double *R1, double *R2, double *P1, double *P2,
                       double *Q, int *roi1, int *roi2);

/* cv::undistort / the remap of a rectified view in one call: the MCC_MAP_FIXED maps of (K, D, R, Knew) for
 * new_w x new_h are built on the device, never leave it, and the image goes through cv::remap's INTER_LINEAR
 * with BORDER_CONSTANT 0 (the kernel of mcc_omnidir_remap).  Knew == NULL is K; new_w == 0 takes the source
 * size. */
int mcc_undistort_image(const unsigned char *src, int src_w, int src_h, int channels, long long src_stride,
                        const double *K, const double *D, int nd, const double *R, const double *Knew, int ld,
                        int new_w, int new_h, int device, unsigned char *dst, long long dst_stride);

/* The per-frame case: the fixed-point maps are built once at create and stay on the device with the source
 * and destination images; every remap call is one upload, one kernel, one download. */
typedef struct mcc_pinrect mcc_pinrect;

typedef struct mcc_pinrect_desc {
    const double *K;       /* [9]                                                 */
    const double *D;       /* [nd] or NULL                                        */
    int nd;
    const double *R;       /* [9] or NULL                                         */
    const double *P;       /* [3 * ld] or NULL (K)                                */
    int ld;                /* doubles per row of P: 3 or 4                        */
    int dst_width, dst_height;
    int src_width, src_height;
    int channels;          /* 1 or 3                                              */
    int device;            /* HIP device ordinal                                  */
} mcc_pinrect_desc;

int mcc_pinrect_create(mcc_pinrect **out, const mcc_pinrect_desc *desc);
void mcc_pinrect_destroy(mcc_pinrect *h);
int mcc_pinrect_remap(mcc_pinrect *h, const unsigned char *src, long long src_stride, unsigned char *dst,
                      long long dst_stride);

/* ---- pinhole reconstruction: cv::reprojectImageTo3D, and a rectified pair to depth (stereoReconstruct for the
 * K, D, R, T of mcc_stereo_calibrate).  DESIGN.md 7j states every rule and is the specification. */
#define MCC_DISP_FLOAT 1     /* float pixels                                                             */
#define MCC_DISP_FIXED16 2   /* short pixels, disparity x 16 as the matcher writes it                    */

/* cv::reprojectImageTo3D: per pixel (x, y) with float disparity d, (X, Y, Z, W) = Q (x, y, (double)d, 1) in float64
 * with the four terms of a row summed left to right and no fused multiply-add; points[(y width + x) 3 ..] =
 * (float)(X / W), (float)(Y / W), (float)(Z / W).  W == 0 gives the IEEE inf or NaN, never a fault (a NaN
 * is stored as the quiet NaN 0x7FC00000).  A MCC_DISP_FIXED16 pixel is
 * converted as (float)d / 16.0f (exact) -- THIS DIFFERS FROM OpenCV, which takes a CV_16S disparity raw and leaves the
 * division by 16 to the caller.  With handle_missing != 0 every pixel whose d is not above the minimum of the whole
 * image gets Z = 10000.0f (OpenCV's bigZ), X and Y as above; a NaN disparity does not take part in the minimum.
 * stride_bytes is the distance between rows, a multiple of the pixel size.  device_ms (may be NULL): the kernels alone,
 * by HIP events.  MCC_EINVAL, before any device work, for a null pointer, a bad type, a size that is not positive or
 * above 32767, or a stride shorter than a row or not a multiple of the pixel size. */
int mcc_reproject_image_to_3d(const void *disparity, int disparity_type, int width, int height,
                              long long stride_bytes, const double *Q /* [16] */, int handle_missing, int device,
                              float *points /* [height*width*3] */, double *device_ms);

/* the point types of include/mcc_omnidir.h (MCC_OMNI_XYZRGB, MCC_OMNI_XYZ) under model-neutral names */
#define MCC_XYZRGB 1   /* 6 floats per point: x y z r g b */
#define MCC_XYZ 2      /* 3 floats per point              */

/* A rectified pinhole pair to depth, resident on the device for a stream of frame pairs.  create runs
 * mcc_stereo_rectify on the host and builds both cameras' MCC_MAP_FIXED maps on the device; compute uploads the
 * pair and runs the remap twice, the semi-global matcher of mcc_omnidir_sgbm (include/mcc_omnidir.h; d = x1 - x2 >= 0,
 * no minDisparity, uniquenessRatio or speckle filter), the float disparity d16 / 16.0f (-1 where there is no match;
 * a black pixel gets no special value), mcc_reproject_image_to_3d's kernel with Q and no missing-value handling,
 * and the compacted cloud.
 *
 * The cloud: a pixel is a point iff d > 0, W is finite and not 0, Z / W > 0 (in float64), max_z <= 0 or
 * Z / W <= max_z, and !use_roi or the pixel lies in roi1.  Points come in mcc_omnirecon's order (columns first, then
 * rows), 3 or 6 floats each: the pixel's dense point, then for MCC_XYZRGB the three channels of rectified image 1 (a
 * 1-channel value three times).
 *
 * Camera order: after rectification camera 2 must lie to the right of camera 1 (below it for a vertical pair), i.e.
 * the component of R2 T along the baseline must be negative; otherwise create is MCC_EINVAL and says to swap.
 *
 * A vertical pair (mcc_stereo_rectify puts the baseline along y) is rectified into the TRANSPOSED frame: the
 * rectified images are new_height wide and new_width high, so that the matcher sees a horizontal pair.  The maps
 * are built from P1, P2 with rows 0 and 1 swapped, Q has columns 0 and 1 swapped, the rois are transposed, and every
 * output (images, disparity, dense points, cloud order) is in that frame; mcc_pinrecon_info reports these. */
typedef struct mcc_pinrecon mcc_pinrecon;

typedef struct mcc_pinrecon_desc {
    const double *K1, *D1, *K2, *D2;        /* [9], [nd] or NULL, as mcc_stereo_rectify          */
    int nd;
    const double *R, *T;                    /* [9], [3]                                          */
    int src_width, src_height, channels;    /* both cameras; channels 1 or 3                     */
    int rectify_flags;                      /* 0 or MCC_CALIB_ZERO_DISPARITY                     */
    double alpha;                           /* as mcc_stereo_rectify                             */
    int new_width, new_height;              /* 0: the source size                                */
    int num_disparities, sad_window_size;   /* as mcc_omnidir_sgbm                               */
    int point_type;                         /* MCC_XYZRGB or MCC_XYZ                             */
    int use_roi;                            /* cloud only inside roi1                            */
    double max_z;                           /* <= 0: no limit                                    */
    int device;
} mcc_pinrecon_desc;

/* what the handle rectifies with, in the frame of its outputs (for a vertical pair the transposed one) */
typedef struct mcc_pinrecon_geometry {
    double R1[9], R2[9], P1[12], P2[12], Q[16];
    int roi1[4], roi2[4];                   /* x, y, width, height                               */
    int width, height;                      /* of the rectified images, the disparity and points */
    int transposed;                         /* 1 for a vertical pair                             */
} mcc_pinrecon_geometry;

/* MCC_EINVAL with a message, before any device work, for everything mcc_stereo_rectify and mcc_omnidir_sgbm refuse
 * (sizes, channels, num_disparities not a multiple of 16 or above 256 or not below the matched width, an even
 * window, 93 channels window^2 > 32767, a cost volume above MCC_OMNI_SGBM_MAX_COST_BYTES), nd = 14, a bad point type
 * and the camera order. */
int mcc_pinrecon_create(mcc_pinrecon **out, const mcc_pinrecon_desc *desc);
void mcc_pinrecon_destroy(mcc_pinrecon *h);
int mcc_pinrecon_info(const mcc_pinrecon *h, mcc_pinrecon_geometry *geometry);

/* One pair.  Out: disparity (float [height*width]), rec1, rec2 (the rectified images, strides in bytes); disparity16
 * (the matcher's short [height*width], -16 where there is no match), points (float [height*width*3]) and cloud may
 * be NULL (cloud only with capacity 0).  capacity counts points; *n_points is the number of points of the cloud.  If
 * it exceeds capacity the call is MCC_EINVAL, *n_points still holds it and cloud is untouched. */
int mcc_pinrecon_compute(mcc_pinrecon *h, const unsigned char *image1, long long stride1,
                         const unsigned char *image2, long long stride2, float *disparity, short *disparity16,
                         unsigned char *rec1, long long rec1_stride, unsigned char *rec2, long long rec2_stride,
                         float *points, float *cloud, long long capacity, long long *n_points);

/* device milliseconds per pair over n_frames back-to-back computes (every kernel, no transfer) on resident random
 * frames, by HIP events */
int mcc_pinrecon_time(mcc_pinrecon *h, int n_frames, double *ms_per_frame);

/* A handle used once.  Both images' sizes and channel counts are given so that a mismatch, between them or with
 * desc, is refused; geometry (may be NULL) is filled before the pair is computed, so that a caller can size its
 * outputs from a first call that fails for a too small capacity. */
int mcc_stereo_reconstruct(const unsigned char *image1, int width, int height, int channels, long long stride1,
                           const unsigned char *image2, int width2, int height2, int channels2, long long stride2,
                           const mcc_pinrecon_desc *desc, mcc_pinrecon_geometry *geometry, float *disparity,
                           short *disparity16, unsigned char *rec1, long long rec1_stride, unsigned char *rec2,
                           long long rec2_stride, float *points, float *cloud, long long capacity,
                           long long *n_points);

/* The cloud rule on the host, through the very function the count and the write kernel compile: the cloud of a float
 * disparity [height*width] under Q, with the dense points computed as mcc_reproject_image_to_3d does.  rec1 (packed
 * rows, may be NULL with MCC_XYZ) gives the colours, roi (may be NULL: no roi) is x, y, width, height.  Capacity as
 * mcc_pinrecon_compute.  No device call. */
int mcc_pinrecon_host_cloud(const float *disparity, int width, int height, const double *Q,
                            const unsigned char *rec1, int channels, int point_type, const int *roi, double max_z,
                            float *cloud, long long capacity, long long *n_points);

#ifdef __cplusplus
}
#endif
#endif
