/*
 * vo_hip.h -- C ABI of libvo_hip.so: the MI355X (gfx950) implementation of the
 * projective-ICP hot path of lucanunz/Visual-odometry.
 *
 * Every entry point replaces one interface of the reference (cited as
 * <file>:<line> under the reference tree).  The reference has no FFI: its
 * "plugin API" for this path is two C++ classes (Camera, PICPSolver) and a few
 * free functions; include/vo/ *.hpp re-create those on top of this ABI.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ / torch types.
 *  - matrices are COLUMN-major, exactly the memory of the Eigen objects the
 *    reference passes around (defs.h:7-29): K = Eigen::Matrix3f (9 floats),
 *    T/X = Eigen::Isometry3f (4x4, 16 floats).
 *  - point arrays are the contiguous storage of the reference's std::vectors:
 *    Vector3fVector -> float[3n], Vector2fVector -> float[2n],
 *    Vector10fVector -> float[10n], IntPairVector -> int32_t[2n] (first,second).
 *  - functions return 0 (VO_OK) or a negative vo_status; vo_last_error() gives
 *    the message of the last failure on the calling thread.
 *  - unless the name ends in _dev, array arguments are HOST pointers: inputs
 *    are copied to the GPU, outputs copied back, and the call returns when the
 *    outputs are valid.  *_dev variants take DEVICE pointers (memory from
 *    vo_dev_alloc or any hipMalloc), enqueue on the context's stream and do not
 *    synchronise; counts are then produced in device memory.  Device arrays
 *    must start on an 8-byte boundary (hipMalloc gives 256; a sub-array at an
 *    even element offset keeps it): rows and index pairs move as 8-byte pieces.
 *  - a vo_ctx and the handles created from it must be used by one host thread
 *    at a time (the reference objects are not thread-safe either).
 *  - there is NO CPU fallback: every entry point fails with VO_ERR_NO_DEVICE if
 *    no gfx950 device can be used.
 */
#ifndef VO_HIP_H
#define VO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_HIP_ABI_VERSION 1

typedef enum vo_status {
  VO_OK = 0,
  VO_ERR_INVALID_ARG = -1,
  VO_ERR_NO_DEVICE = -2,
  VO_ERR_HIP = -3,
  VO_ERR_OUT_OF_MEMORY = -4,
  VO_ERR_BAD_INDEX = -5,   /* a correspondence index is outside its array */
  VO_ERR_NOT_READY = -6    /* e.g. one_round before set_points */
} vo_status;

typedef struct vo_ctx vo_ctx;     /* one per (device, stream) */
typedef struct vo_picp vo_picp;   /* device twin of a PICPSolver */

int vo_abi_version(void);
const char *vo_last_error(void);

/* ---- context ----------------------------------------------------------- */
/* stream: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL
 * to let the context create its own non-blocking stream. */
int vo_ctx_create(int device, void *stream, vo_ctx **out);
/* Handles made on a context (vo_picp, vo_graph, vo_kdtree) should be destroyed before it.  If one outlives its
 * context anyway, every use of it fails with VO_ERR_INVALID_ARG and its destroy still releases what it owns;
 * destroying a context twice is refused. */
int vo_ctx_destroy(vo_ctx *ctx);
int vo_ctx_synchronize(vo_ctx *ctx);
void *vo_ctx_stream(vo_ctx *ctx);
int vo_ctx_device(vo_ctx *ctx);
/* name of the device ("gfx950...") and number of compute units */
int vo_ctx_device_info(vo_ctx *ctx, char *name, int name_len, int *n_cu);

/* ---- hipGraph capture of a sequence of *_dev calls -------------------------------- */
/* Everything enqueued on the context's stream between begin and end (only *_dev entry
 * points: no host copies, no synchronisation, and every buffer the sequence needs must
 * already have been sized by a previous identical call) becomes one replayable graph:
 * a whole frame (match, join, transform, n rounds, triangulate = ~80 launches) then
 * costs one launch on the host.  Device pointers and counts are baked in; data and
 * device-side counts may change between replays.  A graph (like a vo_picp or a vo_event)
 * must be destroyed before the context it was made on.  Between begin and end every entry
 * point that copies host memory, allocates or waits (the forms without _dev, vo_ctx_synchronize,
 * vo_dev_alloc ...) and every *_dev call that would have to grow a workspace is refused with
 * VO_ERR_NOT_READY / VO_ERR_HIP before it touches the stream: the capture stays valid. */
typedef struct vo_graph vo_graph;
int vo_ctx_begin_capture(vo_ctx *ctx);
int vo_ctx_end_capture(vo_ctx *ctx, vo_graph **out);
int vo_graph_launch(vo_graph *g);          /* on the stream of the context it was captured on */
int vo_graph_destroy(vo_graph *g);

/* Ordering between contexts (= streams) of one device.  Work enqueued on one context can be made to
 * wait for a point in another context's stream without blocking the host: e.g. uploads or the
 * matcher of frame t+1 (it depends on the appearances alone) on a second context while frame t runs on
 * the first (pipeline.py: SequencePipeline(overlap_match=True); measured in DESIGN.md section 5). */
typedef struct vo_event vo_event;
int vo_event_create(vo_ctx *ctx, vo_event **out);
int vo_event_record(vo_event *ev, vo_ctx *ctx);      /* marks the current end of ctx's stream */
int vo_ctx_wait_event(vo_ctx *ctx, vo_event *ev);    /* later work on ctx waits for the marked point */
int vo_event_destroy(vo_event *ev);

/* device memory helpers for callers without a HIP runtime of their own */
int vo_dev_alloc(vo_ctx *ctx, size_t bytes, void **dptr);
int vo_dev_free(vo_ctx *ctx, void *dptr);
int vo_memcpy_h2d(vo_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes); /* synchronous */
int vo_memcpy_d2h(vo_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* synchronous */

/* ---- Camera::projectPoints (camera.cpp:16-37; projectPoint camera.h:25-37) */
/* out_uv has room for n points.  keep_indices!=0: *n_out = n and invalid
 * points are (-1,-1); keep_indices==0: valid points only, input order kept.
 * *n_inside = the reference's return value (number of points inside). */
int vo_project_points(vo_ctx *ctx, int rows, int cols, int z_near, int z_far, const float K[9],
                      const float T[16], const float *world_xyz, int n, int keep_indices,
                      float *out_uv, int *n_out, int *n_inside);
/* device form: d_counts[0] = n_out, d_counts[1] = n_inside */
int vo_project_points_dev(vo_ctx *ctx, int rows, int cols, int z_near, int z_far, const float K[9],
                          const float T[16], const float *d_world_xyz, int n, int keep_indices,
                          float *d_out_uv, int *d_counts);

/* ---- PICPSolver (picp_solver.h:18-79, picp_solver.cpp) ----------------- */
/* ctor: threshold 1000, damping 1, min inliers 0 (picp_solver.cpp:6-14).  Damping has no setter -- as in the reference -- and the
 * default mode's unpivoted 6x6 solve relies on it: H = sum(lambda J^T J) + 1 * I is positive definite whatever the frame holds. */
int vo_picp_create(vo_ctx *ctx, vo_picp **out);
int vo_picp_destroy(vo_picp *s);
/* init(camera, world, image) (picp_solver.cpp:16-23).  The reference stores
 * raw pointers to the caller's vectors; this copies them to the GPU. */
int vo_picp_set_camera(vo_picp *s, int rows, int cols, int z_near, int z_far, const float K[9],
                       const float T[16]);
int vo_picp_set_points(vo_picp *s, const float *world_xyz, int n_world, const float *meas_uv,
                       int n_meas);
/* borrowed device arrays; must stay valid until the next set_points* call */
int vo_picp_set_points_dev(vo_picp *s, const float *d_world_xyz, int n_world,
                           const float *d_meas_uv, int n_meas);
int vo_picp_set_pose(vo_picp *s, const float T[16]);            /* camera.h:50 */
/* same from a 4x4 in device memory: takes effect at the next one_round/solve call, on
 * the stream, with no host sync (d_T16 must stay valid until then) */
int vo_picp_set_pose_dev(vo_picp *s, const float *d_T16);
int vo_picp_set_kernel_threshold(vo_picp *s, float thr);        /* picp_solver.h:35 */
int vo_picp_get_kernel_threshold(vo_picp *s, float *thr);       /* picp_solver.h:33 */
/* oneRound(correspondences, keep_outliers) (picp_solver.cpp:98-112):
 * pairs = (measurement index, world index).  Enqueues one Gauss-Newton
 * iteration -- ONE kernel launch -- and returns without waiting; the
 * pose/statistics getters are the synchronisation points, and the first of
 * them after a run of calls enqueues the launch that finishes the last round
 * (its 6x6 solve, H, b, statistics): a loop of oneRound calls followed by
 * camera(), as vo_complete.cpp:163-168, costs one launch per call plus one.
 * Like the reference (picp_solver.cpp:62) every call honours the array it is
 * given: the pairs are compared IN FULL (memcmp) with the host copy of what is
 * on the GPU and uploaded again when anything differs, so editing the vector in
 * place between two rounds is seen.  When the array has the length of the
 * packed one the round is enqueued first and the comparison runs while the GPU
 * works; a difference then repeats that round on the new pairs (it had written
 * nothing a repeat does not overwrite).  Once two calls in a row have matched --
 * the reference's loop -- a call enqueues its round and up to seven more as ONE
 * graph launch (captured the third time a launch geometry asks for it; the last
 * window of a run is cut to the remembered length of the previous run), and the
 * calls that follow only compare and claim theirs; rounds
 * that ran ahead and are not claimed (the loop ended, the pairs / points /
 * parameters changed) are ignored or repeated, never seen: every result is the
 * one a closed solve of the counted rounds gives.  VO_PICP_RUN_AHEAD=0..14 in the
 * environment (read by vo_picp_create) bounds the look-ahead; at most that many
 * rounds of GPU time are spent for nothing per loop.  As in the reference it cannot fail on
 * "too few inliers" (min_num_inliers is 0 with no setter). */
int vo_picp_one_round(vo_picp *s, const int32_t *pairs, int n_pairs, int keep_outliers);
/* Bookkeeping of the above (any pointer may be NULL): rounds enqueued whose finishing launch is still to come, calls
 * enqueued ahead of their comparison since the handle was made, and how many of those had to be repeated. */
int vo_picp_chain_info(vo_picp *s, int *open_rounds, unsigned long long *speculative, unsigned long long *repeated);
/* n_iters x oneRound with no host round trip in between */
int vo_picp_solve(vo_picp *s, const int32_t *pairs, int n_pairs, int keep_outliers, int n_iters);
/* Explicit form of the same, for callers that iterate on one fixed set: hand the pairs over once
 * (always uploaded), then run rounds on them with no per-call comparison at all. */
int vo_picp_set_correspondences(vo_picp *s, const int32_t *pairs, int n_pairs);
int vo_picp_rounds(vo_picp *s, int keep_outliers, int n_iters);
/* Launch-graph bookkeeping of a handle (any pointer may be NULL): whether multi-round solves are replayed from a captured
 * hipGraph (1) or issued as plain launches (0: VO_PICP_GRAPH=0, or a capture failed), how many graphs are cached, and how
 * many captures failed.  A failed capture does not fail the solve -- the same kernels run as plain launches -- but it is
 * reported once through vo_last_error() and counted here instead of passing unnoticed. */
int vo_picp_graph_info(vo_picp *s, int *use_graph, int *n_graphs, int *n_failures);
/* How the multi-round solves of a handle were submitted since it was made (either pointer may be NULL): replayed from a
 * captured hipGraph behind a plain launch of round 0, or as plain launches throughout.  A handle submits plainly the solves
 * that take a tail form at an M it has learned (every launch of such a solve is a real round, and plain launches leave no
 * gap between two solves that a replayed graph leaves), under VO_PICP_TAIL_SUBMIT=plain, and wherever it has no graph
 * (VO_PICP_GRAPH=0, a failed capture).  Solves of fewer than two rounds, solves in reference-order arithmetic and solves
 * captured into a caller's graph are counted in neither.  Results are the same bytes in both forms.  (voe_: like every
 * entry point added since the set of vo_* names was closed.) */
int voe_picp_submit_info(vo_picp *s, unsigned long long *graph_solves, unsigned long long *plain_solves);
/* Reference-order arithmetic (off by default).  on != 0: every later round of this handle is computed
 * with the reference's own rounding -- per-correspondence terms unfused, (J0r*J0c + J1r*J1c)*lambda,
 * H / b / chi summed sequentially in correspondence order (picp_solver.cpp:62-95), Eigen's pivoted
 * LDLT with true divisions (:109), sin/cos in double rounded to float (utils.h:16-78) -- so pose,
 * H, b, chi and the inlier count are BIT-IDENTICAL to the reference's scalar float32 arithmetic
 * (as restated by oracle/: tests/test_gpu_exact.py).  One workgroup, all rounds in one launch:
 * a few microseconds per round at the <= 127 points per frame of the reference's dataset, 0.18 ms
 * per round at 50k (the serial chain of 50 000 dependent float adds).  The default (fast) mode differs from it by rounding only (tree reduction,
 * one FMA per product, Newton-refined hardware reciprocals, unpivoted LDLT, float sincos): a gate or chi^2 decision can differ
 * from the reference's only for a correspondence whose reference-order value lies within a few ulp of the gate -- measured on
 * correspondences planted at every gate (tests/test_gpu_gates.py, same pose in): <= 2 ulp for the depth gates, <= 3.7 for the
 * image gates, <= 276 ulp of the threshold for chi^2 (3e-5 relative); the test holds 4 / 8 / 1024. */
int vo_picp_set_exact(vo_picp *s, int on);
/* device pairs; d_n_pairs (may be NULL) points at a device int that overrides
 * n_pairs (<= n_pairs), so the output of the join kernel can be consumed
 * without a host round trip. */
int vo_picp_solve_dev(vo_picp *s, const int32_t *d_pairs, int n_pairs, const int *d_n_pairs,
                      int keep_outliers, int n_iters);
int vo_picp_get_pose(vo_picp *s, float T[16]);                  /* camera(), picp_solver.h:41 */
int vo_picp_get_pose_dev(vo_picp *s, float *d_T16);             /* async copy on the stream */
/* device address of the solver's own 4x4 pose (column-major), valid for the life of the
 * handle and rewritten by every solve: lets a consumer kernel read the result in place
 * (rounds of vo_picp_one_round reach it with the next getter call -- this one included).
 * Behind the 16 floats lie five ints, the cycle report of the last vo_picp_solve / vo_picp_solve_dev / vo_picp_rounds of
 * more than one workgroup: [0], [1] internal; [2] detected_at, [3] period, [4] skipped.  Within a solve a round is a
 * deterministic map of the pose, so once the pose after round k equals, bit for bit, the pose after an earlier round j,
 * the rounds that follow repeat earlier ones and their launches return at once -- the results are the bytes of the full
 * solve.  detected_at: the launch that found the repeat, k + 1 (0: none); period: k - j; skipped: launches that returned
 * at once.  Read them once the stream has drained (vo_memcpy_d2h does).  VO_PICP_CYCLE=0 in the environment (read per
 * call) turns the detection off.
 * Behind the five ints lie the 64 x 12 floats of the pose history, and behind those four ints about the tail launch, the one
 * launch that may stand for the rounds behind round 16 of such a solve: [0] the last solve used it, [1] the real rounds that
 * ran inside it (0 where the pose had repeated before), [2] a workgroup of it gave up waiting for the others -- the getters
 * then fail with VO_ERR_HIP instead of returning numbers --, [3] internal.  VO_PICP_TAIL=0 keeps a launch per round.
 * Behind those four ints lie two counters of the handle's tail launches and then, written by tail launches only (so they
 * describe the last solve that had one: check [0] above first): how that launch closed the solve -- 1 from partial rows an
 * earlier launch had left in the ring, 2 after computing the last round's rows again (VO_PICP_TAIL_RING=0 forces this), 3 at
 * the end of its loop of real rounds, 4 in the round that computed the repeating pose (the early form of the launch, whose
 * workgroups find the repeat themselves: a handle takes it behind 32 consecutive solves that repeated, VO_PICP_TAIL_EARLY=0 in
 * the environment keeps it from that, =1 adds the form to a forced VO_PICP_TAIL_FROM; read per call) -- and the M it ran with (rounds 1 .. M had launches of their own; a handle lowers M to
 * where its solves repeat, VO_PICP_TAIL_FROM sets it per call).  Such a solve has no finishing launch. */
int vo_picp_pose_dev_ptr(vo_picp *s, const float **d_T16);
int vo_picp_get_stats(vo_picp *s, float *chi_inliers, float *chi_outliers, int *num_inliers); /* :44-50 */
/* H (6x6 col-major, damping included, as _H after oneRound) and b of the last round */
int vo_picp_get_system(vo_picp *s, float H[36], float b[6]);

/* Batched solver: n_problems independent (camera, points, pairs) problems,
 * every one iterated n_iters times inside one launch.  Arrays are DEVICE
 * pointers; problem p uses world[p*world_stride..], meas[p*meas_stride..],
 * pairs[p*pairs_stride..] (strides in elements of the respective type:
 * points, points, pairs) and n_pairs[p] pairs.  All share rows/cols/z/K/thr.
 * d_T0: n_problems initial poses (16 floats each) or NULL for identity;
 * d_T_out: n_problems final poses; d_stats_out (may be NULL): per problem
 * {chi_inliers, chi_outliers, (float)num_inliers, (float)n_bad} -- n_bad = pairs of the problem whose
 * index lies outside its point arrays: they are dropped (the single-problem entry points report the same
 * condition as VO_ERR_BAD_INDEX from their getters). */
/* Two forms, same results up to the summation order of H and b: one workgroup per problem with all rounds
 * inside one launch (many problems: streaming bound), or one launch per round with many workgroups per
 * problem (a few problems: the single-problem kernels with the problem as a grid dimension; 2.5x faster at one
 * problem of 50k, equal at ~10).  form 0 (default) picks by a cost model, 1 / 2 force one.
 * With one workgroup per problem and at most 0.65 problems per CU (and >= 18 432 correspondences of capacity per problem)
 * the launch has one workgroup per CU and the waves of those without a problem take work off the others' every round
 * (csrc/picp.hip, picp_batch_shared_kernel: 1.9x at 32 problems of 50k, 1.1x at 128; beyond, the problems' own
 * workgroups already draw what the memory side delivers).  The result does not depend on when, or whether, a helper
 * wave runs; problems with the same data in one call get the same bits.  VO_PICP_SHARE=0 in the environment turns it off.
 * vo_picp_batch_info: what the context's LAST batched call ran as -- 1 one launch per round, 2 one workgroup per problem,
 * 3 reference-order arithmetic, 4 one workgroup per problem with helpers (0: no call yet) -- and its workgroups per
 * launch.  Either pointer may be NULL. */
int vo_picp_batch_set_form(vo_ctx *ctx, int form);
int vo_picp_batch_info(vo_ctx *ctx, int *form, int *workgroups);
/* Test support.  With VO_PICP_HELP_SCHEDULE="mode,mod,rem,round[,polls]" in the environment a form-4 call runs an
 * instantiation of its kernel that makes chosen helper waves (or problems' own workgroups) late or absent by script
 * (csrc/picp.hip; modes none, leave, stall, home-stall) and records, per problem: the chunks its own workgroup ended up
 * computing itself (bit j: chunk j), its number of chunks, and how many of its helper waves returned before their last
 * round.  The results of the call must be those of the undisturbed call bit for bit.  vo_picp_batch_help_info waits for
 * the context's stream and copies that record of the LAST batched call out (n_problems entries each, any pointer may be
 * NULL); VO_ERR_INVALID_ARG when that call did not run so, or n_problems is not its problem count. */
int vo_picp_batch_help_info(vo_ctx *ctx, int n_problems, unsigned long long *own_chunks, int *n_chunks, int *left_early);
int vo_picp_solve_batch_dev(vo_ctx *ctx, int n_problems, int rows, int cols, int z_near, int z_far,
                            const float K[9], float kernel_threshold, int keep_outliers,
                            const float *d_world_xyz, size_t world_stride, const float *d_meas_uv,
                            size_t meas_stride, const int32_t *d_pairs, size_t pairs_stride,
                            const int *d_n_pairs, const float *d_T0, int n_iters, float *d_T_out,
                            float *d_stats_out);

/* ---- compute_correspondences_images (vo_complete.cpp:12-49) ------------ */
/* Exact nearest neighbour within `radius` in the 10-D appearance space,
 * replacing TreeNode_::bestMatchFull (eigen_kdtree.h:90-115): the larger set
 * is searched (ties: a1), the smaller set queries in ascending index, a hit
 * needs squared distance < radius*radius (strict), pairs are emitted as
 * (index in a1, index in a2).  Exact-distance ties go to the lowest index.
 * out_pairs has room for min(n1,n2) pairs. */
/* All variants return identical pairs.  mode 0 (default): pick by size and frame count; 1: scan every
 * (query, tree point) pair; 2: counting-sort both sets into 1024 buckets along the two appearance
 * components of largest spread and scan only the buckets within the radius (LDS-tiled); 3: counting-sort
 * both sets into a 4-D grid of cells no narrower than the radius and visit, per query, the <= 81 cells
 * around it (about 25 candidates per query on uniform appearances); 4 / 5: first answer every query that has a
 * bitwise copy in the tree (appearances are copied from frame to frame; a copy is at distance 0, the minimum) through
 * hash tables cut by hash, then run 2 / 3 for the remaining queries only -- what mode 0 does from 8 frames per call on
 * at the sizes where it sorts (sets of up to 204 800 points; beyond, 2 / 3 alone).  In mode 5 a frame that is left with
 * FEW open queries (at most 1/16 of its queries, and 2560: the new landmarks of a tracking frame) does not sort its tree at
 * all: the open queries are ordered by cell and the tree is streamed once past them.  Matcher stage of 200 x 50k frames:
 * 0.52 ms when every query has a copy, 0.73 at 1 % open, 0.80 at 5 %, 1.27 at 25 % (profiles/r05_bench_line.json); mode 3
 * alone 1.10; data WITHOUT any copies is noticed from eight sampled queries per frame and skips the tables and the lookup
 * (1.29 ms) -- and, in mode 0, the NEXT calls leave the pass out altogether (1.10 ms): what the previous call found travels to
 * the host behind the stream, "no frame took the pass" twice in a row switches it off for 16 calls, a sample query that the search finds at
 * distance 0 switches it on again at once, vo_match_set_mode() forgets what was learnt.  Partly copied data (10 - 90 % of
 * the queries without a copy) pays 0.05 - 0.2 ms for the pass -- ask for mode 3 there. */
int vo_match_set_mode(vo_ctx *ctx, int mode);
int vo_match_appearances(vo_ctx *ctx, const float *a1, int n1, const float *a2, int n2,
                         float radius, int32_t *out_pairs, int *n_out);
int vo_match_appearances_dev(vo_ctx *ctx, const float *d_a1, int n1, const float *d_a2, int n2,
                             float radius, int32_t *d_out_pairs, int *d_n_out);

/* ---- TreeNode_::fullSearch (eigen_kdtree.h:56-71) for a whole query set -- */
/* Every tree point within `radius` of each query (squared distance < radius*radius, strict, as
 * bruteForceSearch brute_force_search.h:3-20), exactly -- the same 4-D cell search as matcher mode 3.
 * CSR result: query i owns indices[offsets[i] .. offsets[i+1]) (tree indices; the order inside one query's
 * list is unspecified, as it is in the reference, where it follows the tree traversal).  `capacity` = room
 * in `indices`; *n_total = hits found.  If n_total > capacity the call fails with VO_ERR_INVALID_ARG and
 * offsets/n_total tell the caller how much room to bring.  Unlike the matcher the roles are explicit: the
 * first set is searched whatever the sizes.  The approximate modes of the reference (fastSearch,
 * bestMatchFast: descend one side of each PCA split) depend on its tree: vo_kdtree_* below; their
 * answers are subsets of this call's / of vo_match_appearances'.  Sets of up to 1 835 008 points each (1024 slices of the
 * level-1 sort); the device arrays on 8-byte boundaries like every device entry point. */
int vo_radius_search(vo_ctx *ctx, const float *tree_app, int n_tree, const float *query_app, int n_q,
                     float radius, int32_t *offsets, int32_t *indices, int capacity, int *n_total);
/* device form: d_offsets[n_q + 1]; d_offsets[n_q] = hits found (also when > capacity: the surplus is dropped) */
int vo_radius_search_dev(vo_ctx *ctx, const float *d_tree_app, int n_tree, const float *d_query_app,
                         int n_q, float radius, int32_t *d_offsets, int32_t *d_indices, int capacity);

/* ---- TreeNode_ in its approximate modes (eigen_kdtree.h:18-52,75-85) ------------------------ */
/* bestMatchFast and fastSearch descend ONE side of every PCA split plane and brute-force the leaf they reach: their
 * answers depend on the tree (split directions, order of the points inside a leaf), so the tree is a handle.
 * vo_kdtree_create builds it on the host like the TreeNode_ constructor (:18-38; mean/covariance in float in array
 * order, eigen_covariance.h:5-43 with a double Jacobi for the eigen-solver -- the split normal's sign is fixed by
 * convention (largest-magnitude component positive), which Eigen's SelfAdjointEigenSolver does not promise: every leaf
 * holds the same SET of points as the reference's up to the solver's sign / degeneracy, the order inside a leaf (and with
 * it bestMatchFast's first-minimum tie and fastSearch's result order) may differ --, the two-pointer partition of split.h:8-34,
 * recursion while a node holds >= max_points_in_leaf points; a node whose points all fall on one side becomes a leaf --
 * the reference recurses forever there) and uploads it; queries run on the GPU, one lane per query.  points: host
 * float[10n] (the reference's 11-vectors carry the index in slot 0; here the index is implicit).  Neither mode is used
 * by an executable of the reference; the exact modes are vo_match_appearances (bestMatchFull) and vo_radius_search
 * (fullSearch), whose answers do not depend on any tree. */
typedef struct vo_kdtree vo_kdtree;
int vo_kdtree_create(vo_ctx *ctx, const float *points_app, int n, int max_points_in_leaf, vo_kdtree **out);
int vo_kdtree_destroy(vo_kdtree *tree);       /* before the context it was made on */
int vo_kdtree_info(vo_kdtree *tree, int *n_points, int *n_nodes, int *n_leaves);
/* bestMatchFast (:75-85) for every query: out_index[i] = index (in points_app) of the closest point OF THE QUERY'S LEAF
 * with squared distance < radius*radius (strict; the first minimum in leaf order), or -1 */
int vo_kdtree_best_match_fast(vo_kdtree *tree, const float *query_app, int n_q, float radius, int32_t *out_index);
int vo_kdtree_best_match_fast_dev(vo_kdtree *tree, const float *d_query_app, int n_q, float radius, int32_t *d_out_index);
/* fastSearch (:40-52) for every query, CSR like vo_radius_search: query i owns indices[offsets[i] .. offsets[i+1]), the
 * points of its leaf within the radius IN LEAF ORDER (the order bruteForceSearch pushes them, brute_force_search.h:3-20);
 * n_total > capacity: VO_ERR_INVALID_ARG with offsets / n_total filled in */
int vo_kdtree_fast_search(vo_kdtree *tree, const float *query_app, int n_q, float radius, int32_t *offsets,
                          int32_t *indices, int capacity, int *n_total);
int vo_kdtree_fast_search_dev(vo_kdtree *tree, const float *d_query_app, int n_q, float radius, int32_t *d_offsets,
                              int32_t *d_indices, int capacity);

/* ---- extract_correspondences_world (vo_complete.cpp:52-66) ------------- */
/* For each image pair (ref,cur) in order, the FIRST world pair (ref',w) with
 * ref'==ref gives (cur,w); image pairs without partner are dropped.
 * out_pairs has room for n_img pairs. */
int vo_join_correspondences(vo_ctx *ctx, const int32_t *img_pairs, int n_img,
                            const int32_t *world_pairs, int n_world, int32_t *out_pairs,
                            int *n_out);
/* device form; the counts may come from device memory (NULL -> use n_img / n_world);
 * n_ref = size of the reference index space (all .first values < n_ref). */
int vo_join_correspondences_dev(vo_ctx *ctx, const int32_t *d_img_pairs, int n_img,
                                const int *d_n_img, const int32_t *d_world_pairs, int n_world,
                                const int *d_n_world, int n_ref, int32_t *d_out_pairs,
                                int *d_n_out);

/* ---- Isometry3f * point set (PointCloud.h:77-82, vo_daKnown.cpp:144) --- */
int vo_transform_points(vo_ctx *ctx, const float T[16], const float *in_xyz, int n,
                        float *out_xyz);
/* device form: the isometry comes from the host (T) or, when d_T16 is non-NULL, from device
 * memory (column-major 4x4, e.g. vo_picp_pose_dev_ptr of the previous frame's solve -- the
 * X_curr * triangulated_pc of vo_complete.cpp:159 with no host round trip); d_n (may be NULL)
 * points at a device count <= n. */
int vo_transform_points_dev(vo_ctx *ctx, const float T[16], const float *d_T16,
                            const float *d_in_xyz, int n, const int *d_n, float *d_out_xyz);

/* ---- triangulate_points (utils.cpp:51-134; triangulate_point :36-49) --- */
/* pairs = (index in p1, index in p2); X = pose of the first camera in the
 * frame of the second.  Survivors are written densely in input order:
 * out_xyz[k], out_pairs[k] = (index in p2, k) (may be NULL: overload v1),
 * out_app[k] = app2[index in p2] when app2/out_app are non-NULL (overload
 * v3).  Output arrays have room for n pairs.  Returns the count in *n_out. */
int vo_triangulate(vo_ctx *ctx, const float K[9], const float X[16], const int32_t *pairs, int n,
                   const float *p1_uv, int n1, const float *p2_uv, int n2, const float *app2,
                   float *out_xyz, int32_t *out_pairs, float *out_app, int *n_out);
int vo_triangulate_dev(vo_ctx *ctx, const float K[9], const float X[16], const float *d_X16,
                       const int32_t *d_pairs, int n, const int *d_n, const float *d_p1_uv, int n1,
                       const float *d_p2_uv, int n2, const float *d_app2, float *d_out_xyz,
                       int32_t *d_out_pairs, float *d_out_app, int *d_n_out);

/* ---- estimate_transform (epipolar_utils.cpp:176-213) --------------------- */
/* Relative pose of the first camera in the frame of the second from >= 8 image correspondences
 * pairs = (index in p1, index in p2): normalised 8-point fundamental (:103-144, normalisation over
 * ALL n1 / n2 points, :48-65), E = K^T F K, the four (R, +-t) candidates (:146-174) and the
 * cheirality vote -- how many correspondences triangulate under each candidate (the triangulation kernel's per-pair
 * arithmetic, counted) -- which keeps the first candidate with the most survivors.  Host linear algebra in double.
 * As in the reference t is read off R*E un-normalised (:163-164): |t| is the singular value
 * of E, which is what fixes the scale of a monocular sequence.  Fewer than 8 pairs:
 * VO_ERR_INVALID_ARG (the reference prints and exits, :105-108). */
int vo_estimate_transform(vo_ctx *ctx, const float K[9], const int32_t *pairs, int n,
                          const float *p1_uv, int n1, const float *p2_uv, int n2, float X_out[16]);
/* The same from arrays in device memory -- the matcher's pairs and the two images as they lie in HBM; *d_n_pairs (or
 * NULL) <= n_max pairs are live.  The sums over the correspondences run on the GPU (epi.hip): per-axis maxima of both
 * images (:50-56), the 45 distinct entries of A^T A in double (:114-126), and the cheirality vote of all four candidates in
 * one launch; the 9 x 9 eigen-solve and the decomposition of E stay on the host in double.  Two small read-backs;
 * X_out on the host.  (vo_estimate_transform is this after three uploads.) */
int vo_estimate_transform_dev(vo_ctx *ctx, const float K[9], const int32_t *d_pairs, int n_max, const int *d_n_pairs,
                              const float *d_p1_uv, int n1, const float *d_p2_uv, int n2, float X_out[16]);

/* ---- estimate_transform behind RANSAC (robust initialisation) ---------------- */
/* The same pose as vo_estimate_transform, computed on the largest consensus set of n_hypotheses minimal
 * 8-point fits instead of on every pair, so that mismatched pairs do not bias it.
 *
 * Sampling (reproducible bit for bit outside the library).  n = live pairs, all arithmetic on uint64:
 *   splitmix64(x): x += 0x9E3779B97F4A7C15; z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *   draw(h, j)   = ((splitmix64(seed ^ ((h << 20) | j)) >> 32) * n) >> 32          j = 0, 1, 2, ... 63
 * The sample of hypothesis h is the first 8 DISTINCT values of draw(h, 0), draw(h, 1), ...; fewer than 8 within
 * j < 64 leaves the hypothesis invalid.  Its F solves the 8 x 9 system of those pairs' normalised points (the
 * normalisation of vo_estimate_transform: per-axis maxima of ALL n1 / n2 points) in double, projected to rank 2,
 * un-normalised (F = T1^T F T2) and scaled to unit Frobenius norm; a (near-)singular system leaves it invalid.
 * Scoring: pair (u1, v1) <-> (u2, v2), x1 = (u1, v1, 1), x2 = (u2, v2, 1), e = x1^T F x2,
 *   d^2 = e^2 / ((F x2)_0^2 + (F x2)_1^2 + (F^T x1)_0^2 + (F^T x1)_1^2)       (Sampson distance, pixels^2)
 * is an inlier iff d^2 < threshold_px^2 (strict; a zero denominator or a NaN is an outlier).  The winner has the most
 * inliers, ties going to the lowest h.
 * Refit: the winner's inlier pairs, in their original order, go through vo_estimate_transform_dev -- X_out is bit
 * for bit what vo_estimate_transform returns for those pairs.  inlier_mask (n entries, or NULL) marks them;
 * *n_inliers (or NULL) counts them.  Refused: fewer than 8 pairs or a winner with fewer than 8 inliers
 * (VO_ERR_INVALID_ARG), a bad index (VO_ERR_BAD_INDEX), n_hypotheses outside 1 .. 65536, a threshold that is not
 * positive and finite, a call during a graph capture. */
typedef struct vo_ransac_params {
  int      n_hypotheses;   /* 1 .. 65536 */
  float    threshold_px;   /* Sampson distance in pixels, > 0 and finite */
  uint64_t seed;
} vo_ransac_params;

int vo_estimate_transform_ransac(vo_ctx *ctx, const float K[9], const int32_t *pairs, int n,
                                 const float *p1_uv, int n1, const float *p2_uv, int n2,
                                 const vo_ransac_params *params, float X_out[16],
                                 uint8_t *inlier_mask /* n entries or NULL */, int *n_inliers /* or NULL */);
/* The same from arrays in device memory (as vo_estimate_transform_dev): *d_n_pairs (or NULL) <= n_max pairs are
 * live, pairs beyond them are never sampled and get mask 0.  d_inlier_mask: n_max bytes of device memory, or NULL.
 * d_hypothesis_counts: n_hypotheses ints of device memory, or NULL -- every hypothesis's inlier count, -1 for an
 * invalid one.  One read-back after the selection, then the refit's two; X_out and *n_inliers on the host. */
int vo_estimate_transform_ransac_dev(vo_ctx *ctx, const float K[9], const int32_t *d_pairs, int n_max,
                                     const int *d_n_pairs, const float *d_p1_uv, int n1, const float *d_p2_uv, int n2,
                                     const vo_ransac_params *params, float X_out[16],
                                     uint8_t *d_inlier_mask /* n_max or NULL */,
                                     int32_t *d_hypothesis_counts /* n_hypotheses or NULL */,
                                     int *n_inliers /* host, or NULL */);

/* ---- P3P RANSAC in front of the tracking solve (robust tracking) ------------- */
/* A camera pose T (world in camera, column-major 4x4, what vo_picp_set_pose[_dev] takes) from the largest consensus
 * set of n_hypotheses minimal P3P fits over 2D-3D pairs, and those pairs: the start and the input of a PICP solve
 * that mismatched pairs cannot pull.  pairs = (meas_idx, world_idx), the solver's orientation; params as above.
 *
 * Sampling: draw(h, j) of vo_estimate_transform_ransac (n = live pairs).  The sample of hypothesis h is the first 4
 *   DISTINCT values of draw(h, 0), draw(h, 1), ... within j < 64 (fewer: the hypothesis is invalid), s0 .. s3.
 * Minimal solve, in double, on s0, s1, s2: world points P1, P2, P3; bearings j_k = K^-1 (u, v, 1) normalised to unit
 *   length (K^-1 in double of the float K: any K).  Grunert's solution (Haralick et al. 1994, "Review and analysis of
 *   solutions of the three point perspective pose estimation problem"): a^2 = |P2-P3|^2, b^2 = |P1-P3|^2,
 *   c^2 = |P1-P2|^2, cos(alpha) = j2.j3, cos(beta) = j1.j3, cos(gamma) = j1.j2; the distances along the bearings
 *   are s1, s2 = u s1, s3 = v s1, v a real root of Grunert's quartic A4 v^4 + A3 v^3 + A2 v^2 + A1 v + A0 (the paper's
 *   coefficients), u = ((-1 + (a^2-c^2)/b^2) v^2 - 2 ((a^2-c^2)/b^2) cos(beta) v + 1 + (a^2-c^2)/b^2)
 *   / (2 (cos(gamma) - v cos(alpha))), s1^2 = b^2 / (1 + v^2 - 2 v cos(beta)).  The roots are taken in closed form
 *   (Ferrari) and refined by two Newton steps on the quartic.  A root is a solution when v > 0, u > 0, s1^2 > 0, all
 *   finite; its R, t is the rigid motion taking P1, P2, P3 onto the camera points s_k j_k (the triangles are
 *   congruent up to rounding).  Among the solutions the hypothesis is the one whose projection of the 4th sample's
 *   world point lies closest to its measurement (squared pixels, +inf for a depth <= 0), ties going to the smaller v.
 *   Invalid (count -1): fewer than 4 distinct draws, a degenerate world triangle (|(P2-P1) x (P3-P1)| <=
 *   1e-9 |P2-P1| |P3-P1|), A4 = 0 or a non-finite coefficient, no solution.  The pose is then rounded to float.
 * Scoring, in float with that pose: pair (m, w) is an inlier iff Camera::projectPoint of world point w succeeds
 *   (depth in [z_near, z_far], pixel in [0, cols-1] x [0, rows-1]) and the squared reprojection error
 *   |projection - measurement m|^2 < threshold_px^2 (strict).  The winner has the most inliers, ties to the lowest h.
 * Output: the winner's pose, its inlier pairs compacted in their ORIGINAL order, their count. */
#define VO_POSE_RANSAC_OK            0
#define VO_POSE_RANSAC_FEW_PAIRS     1   /* fewer than 4 live pairs */
#define VO_POSE_RANSAC_NO_HYPOTHESIS 2   /* every hypothesis invalid */
#define VO_POSE_RANSAC_FEW_INLIERS   3   /* the winner has fewer than 6 inliers */
#define VO_POSE_RANSAC_BAD_INDEX     4   /* a live pair indexes outside its array (takes precedence over 1-3) */
/* Host form: refuses the cases 1-3 (VO_ERR_INVALID_ARG) and 4 (VO_ERR_BAD_INDEX, checked on the host first), a
 * call during a graph capture and the parameter errors of vo_estimate_transform_ransac.  T_out: column-major 4x4;
 * inlier_mask (n entries, or NULL) marks the winner's inliers; *n_inliers (or NULL) counts them. */
int vo_estimate_pose_ransac(vo_ctx *ctx, int rows, int cols, int z_near, int z_far, const float K[9],
                            const float *world_xyz, int n_world, const float *meas_uv, int n_meas,
                            const int32_t *pairs, int n, const vo_ransac_params *params, float T_out[16],
                            uint8_t *inlier_mask /* n entries or NULL */, int *n_inliers /* or NULL */);
/* Device form: every argument array and every output in device memory, no host synchronisation: capturable
 * (vo_ctx_begin_capture) once a call with the same n_max and n_hypotheses has sized the context's workspace; a
 * capture that would need a bigger one is refused (VO_ERR_NOT_READY).  *d_n_pairs (or NULL) <= n_max pairs are
 * live; pairs beyond them are never sampled and get mask 0.  As it cannot refuse at run time, cases 1-4 FALL BACK:
 * *d_status = their code, d_T16_out = the identity and EVERY live pair goes to d_inlier_pairs / *d_n_inliers / the
 * mask, so that vo_picp_set_pose_dev(d_T16_out) + vo_picp_solve_dev(d_inlier_pairs, n_max, d_n_inliers) is then
 * exactly the plain solve from the identity.  Otherwise *d_status = 0.  d_T16_out: 16 floats; d_inlier_pairs:
 * n_max pairs; d_inlier_mask: n_max bytes or NULL; d_hypothesis_counts: n_hypotheses ints or NULL (-1 invalid). */
int vo_estimate_pose_ransac_dev(vo_ctx *ctx, int rows, int cols, int z_near, int z_far, const float K[9],
                                const float *d_world_xyz, int n_world, const float *d_meas_uv, int n_meas,
                                const int32_t *d_pairs, int n_max, const int *d_n_pairs,
                                const vo_ransac_params *params, float *d_T16_out, int32_t *d_inlier_pairs,
                                int *d_n_inliers, uint8_t *d_inlier_mask /* or NULL */,
                                int32_t *d_hypothesis_counts /* or NULL */, int *d_status);
/* Batched form: n_problems independent problems in one call -- 3 memsets and 7 launches whatever their number, the
 * problem being a grid dimension -- for callers with many frames per call.  Problem p reads d_world_xyz + p * world_stride
 * points (n_world of them valid indices), d_meas_uv + p * meas_stride pixels (n_meas valid) and d_pairs + p * pairs_stride
 * pairs, of which d_n_pairs[p] <= pairs_stride are live (d_n_pairs = NULL: pairs_stride in every problem).  Strides count
 * ELEMENTS (points, pixels, pairs), the convention of vo_picp_solve_batch_dev.
 * CONTRACT: problem p's pose d_T16_out[p], status d_status[p], inlier pairs d_inlier_pairs + p * pairs_stride, count
 * d_n_inliers[p], mask d_inlier_mask + p * pairs_stride and hypothesis counts d_hypothesis_counts + p * n_hypotheses are
 * BIT FOR BIT what vo_estimate_pose_ransac_dev returns for that problem alone with n_max = pairs_stride and the same
 * params; every problem uses params->seed unchanged.  The fallbacks 1-4 are per problem and mean what they mean there: a
 * bad index in one problem leaves every other problem's status alone.
 * Hence vo_picp_solve_batch_dev(..., d_pairs = d_inlier_pairs, pairs_stride, d_n_pairs = d_n_inliers, d_T0 = d_T16_out,
 * ...) is robust batched tracking, and a problem that fell back is the plain problem from the identity.
 * Capturable under the single form's rule: once a call with the same n_problems, pairs_stride and n_hypotheses has sized
 * the context's workspace; a capture that would need a bigger one is refused (VO_ERR_NOT_READY).
 * Refused (VO_ERR_INVALID_ARG): the single form's parameter errors, n_problems < 1 or > 65535, a world or measurement
 * stride smaller than its count, pairs_stride < 1, a NULL required pointer (only d_n_pairs, d_inlier_mask and
 * d_hypothesis_counts may be NULL). */
int vo_estimate_pose_ransac_batch_dev(vo_ctx *ctx, int n_problems, int rows, int cols, int z_near, int z_far,
                                      const float K[9], const float *d_world_xyz, size_t world_stride, int n_world,
                                      const float *d_meas_uv, size_t meas_stride, int n_meas,
                                      const int32_t *d_pairs, size_t pairs_stride, const int *d_n_pairs /* or NULL */,
                                      const vo_ransac_params *params, float *d_T16_out /* [P][16] */,
                                      int32_t *d_inlier_pairs /* stride pairs_stride */, int *d_n_inliers /* [P] */,
                                      uint8_t *d_inlier_mask /* [P][pairs_stride] or NULL */,
                                      int32_t *d_hypothesis_counts /* [P][n_hypotheses] or NULL */, int *d_status /* [P] */);

/* ---- non-linear refit of the relative pose (Gauss-Newton on the Sampson error) ---- */
/* Refines a relative pose X (column-major 4x4, p_cur = X p_ref: what vo_estimate_transform[_ransac] returns) over 2D-2D
 * pairs = (index in p1, index in p2).  Opt-in: no other entry point calls it.  All arithmetic in double.
 *
 * Residual.  Pair (i, j): x1 = (u1, v1, 1) pixel i of p1 (reference image), x2 = (u2, v2, 1) pixel j of p2 (current
 *   image).  With R, t of X, th = t / |t| and [v]x the cross-product matrix,
 *     F = K^-T R^T [th]x^T K^-1          (K^-1 in double of the float K: any invertible K)
 *   so that x1^T F x2 = 0 for a true pair (the orientation of vo_estimate_transform_ransac), and
 *     r = x1^T F x2 / sqrt((F x2)_0^2 + (F x2)_1^2 + (F^T x1)_0^2 + (F^T x1)_1^2)        (Sampson distance, pixels).
 *   A pair whose denominator is zero or whose r is not finite is SKIPPED.
 * Parameters (5).  d = (w0, w1, w2, a, b):  R <- exp([w]x) R;  th <- normalise(th + a b1 + b b2), with
 *   b1 = normalise(th x e_k), k the axis of the smallest |th_k| (the lowest k on ties), b2 = th x b1.
 *   |t| of the input is kept as a double factor: the scale is gauge, t_out = |t| th.
 *   exp([w]x) = I + A W + B W^2, A = sin(|w|)/|w|, B = 2 sin^2(|w|/2)/|w|^2 (series 1 - |w|^2/6, 1/2 - |w|^2/24
 *   below |w|^2 = 1e-16).
 * Weight.  Huber on |r| with huber_px (0: none): w = 1 for |r| <= huber_px, else huber_px / |r|.  Cost = sum w r^2.
 * A round.  J = d r / d d at d = 0 (analytic); H = sum w J^T J, g = sum w J^T r over the pairs taking part; H d = -g
 *   solved by LDL^T without pivoting -- a pivot that is not > 1e-12 x the largest diagonal entry of H is SINGULAR --
 *   and the update above applied.  Plain Gauss-Newton: no damping, no line search.  After n_rounds rounds one more
 *   accumulation evaluates the final cost.  The sums are taken per workgroup of 256 POSITIONS of the pair array and
 *   added in workgroup order: no atomics, so the result is a function of the positions, the mask and the live count
 *   alone -- the same bits on every call, and whatever n_max >= the live count is.
 * Taking part.  Position p < live count takes part when mask is NULL or mask[p] != 0, its indices lie inside the point
 *   arrays (checked before anything is loaded) and it is not skipped.  n_used counts those, n_bad the marked positions
 *   with an index outside its array, n_skipped every other live position (unmarked, or skipped):
 *   n_used + n_skipped + n_bad = live count.  The three counts and cost_before are those of the INPUT pose.
 * Accept rule.  The refined pose is written (rounded to float, last row 0 0 0 1) when every round's solve was valid, the
 *   final accumulation used as many pairs as the first and the final cost is <= the initial cost.  Otherwise X_out is
 *   X_in bit for bit.  cost_after is the cost of the pose written (= cost_before when not accepted); rounds the number
 *   of updates applied before the refit ended.
 * Status.  Precedence: BAD_INDEX, then BAD_INPUT, then FEW_PAIRS (all three found at the input pose, before any round),
 *   then SINGULAR (the first round that meets it ends the refit), then COST_ROSE. */
#define VO_EPI_REFINE_OK         0
#define VO_EPI_REFINE_FEW_PAIRS  1   /* fewer than 8 pairs used at the input pose */
#define VO_EPI_REFINE_SINGULAR   2   /* a round's 5 x 5 system was singular */
#define VO_EPI_REFINE_COST_ROSE  3   /* the final cost is above the initial one (or pairs dropped out on the way) */
#define VO_EPI_REFINE_BAD_INPUT  4   /* |t| of X_in is zero or not finite (takes precedence over 1-3) */
#define VO_EPI_REFINE_BAD_INDEX  5   /* a marked live pair indexes outside its array (takes precedence over 1-4) */
typedef struct vo_epi_refine_params {
  int   n_rounds;   /* 1 .. 100 */
  float huber_px;   /* >= 0 and finite; 0: no Huber weight */
} vo_epi_refine_params;
typedef struct vo_epi_refine_stats {
  int32_t status;                  /* VO_EPI_REFINE_* */
  int32_t rounds;                  /* updates applied */
  int32_t n_used, n_skipped, n_bad;
  int32_t reserved;                /* 0 */
  double  cost_before, cost_after;
} vo_epi_refine_stats;
/* Device form: arrays, pose out and statistics in device memory (d_stats 8-byte aligned), nothing read back,
 * 2 (n_rounds + 1) launches on the context's stream: capturable (vo_ctx_begin_capture) once a call with the same n_max
 * has sized the context's workspace; a capture that would need a bigger one is refused (VO_ERR_NOT_READY).
 * *d_n_pairs (or NULL) <= n_max pairs are live.  d_mask (n_max bytes, or NULL): only marked positions take part -- the
 * d_inlier_mask of vo_estimate_transform_ransac_dev feeds the refit without a compaction.  The start pose is X_in
 * (host: copied into the launch arguments) or d_X_in (device; may be d_X_out): exactly one of them.  As it cannot
 * refuse at run time, every status other than OK falls back to X_out = X_in and the call still returns VO_OK.
 * Refused (VO_ERR_INVALID_ARG): a NULL required pointer, n_max < 1, a negative point count, n_rounds outside 1 .. 100,
 * huber_px negative or not finite, both or neither of X_in / d_X_in, a singular K, a misaligned device array. */
int vo_refine_transform_dev(vo_ctx *ctx, const float K[9], const int32_t *d_pairs, int n_max,
                            const int *d_n_pairs /* or NULL */, const uint8_t *d_mask /* n_max or NULL */,
                            const float *d_p1_uv, int n1, const float *d_p2_uv, int n2,
                            const float X_in[16] /* host, or NULL */, const float *d_X_in /* device, or NULL */,
                            const vo_epi_refine_params *params, float *d_X_out, vo_epi_refine_stats *d_stats);
/* Host form: three (with a mask four) uploads, the device call, one read-back of the 64 bytes of the pose and the
 * statistics.  Same results bit for bit, same refusals, and not during a graph capture.  The status words are
 * reported in stats_out (required), not as errors: the call returns VO_OK with X_out = X_in for them. */
int vo_refine_transform(vo_ctx *ctx, const float K[9], const int32_t *pairs, int n,
                        const uint8_t *mask /* n entries or NULL */, const float *p1_uv, int n1,
                        const float *p2_uv, int n2, const float X_in[16], const vo_epi_refine_params *params,
                        float X_out[16], vo_epi_refine_stats *stats_out);

/* ---- many independent frame pairs at once (throughput form of vo_complete.cpp:156-173) ---- */
/* For each of n_frames independent frame pairs: match -> join -> X_prev * model -> n_iters rounds
 * from the identity -> triangulate, every stage one batched launch (frame = a grid dimension) and
 * the solver the batched kernel of vo_picp_solve_batch_dev.  All frames share the set sizes, the
 * camera and the solver settings; per-frame counts are produced in device memory.  All pointers
 * are DEVICE pointers; frame f of an array lives at base + f * (items per frame).  Enqueues on
 * the context's stream and returns. */
typedef struct vo_frame_batch {
  int n_frames;
  int n_ref, n_cur;              /* points in every reference / current image */
  int n_model, n_model_pairs;    /* model points and (ref index, model index) pairs per frame */
  const float *ref_app, *cur_app;   /* [n_frames][n_ref|n_cur][10] */
  const float *ref_pts, *cur_pts;   /* [n_frames][n_ref|n_cur][2] */
  const float *model;               /* [n_frames][n_model][3] */
  const int32_t *model_pairs;       /* [n_frames][n_model_pairs][2] */
  const float *X_prev;              /* [n_frames][16] column-major, or NULL for identity */
  int rows, cols, z_near, z_far;
  float K[9];
  float kernel_threshold;
  int keep_outliers;
  int n_iters;
  float radius;                     /* appearance radius (0.1 in the reference) */
  /* outputs; q = min(n_ref, n_cur) items of room per frame */
  int32_t *matches;                 /* [n_frames][q][2]  (ref index, cur index) */
  int32_t *joined;                  /* [n_frames][q][2]  (cur index, model index) */
  float *model_moved;               /* [n_frames][n_model][3]  X_prev * model, or NULL: the moved cloud is not wanted -- the solver
                                     * then moves the points it gathers itself (same arithmetic, one pass and 12 B per model point less) */
  float *poses;                     /* [n_frames][16] */
  float *stats;                     /* [n_frames][4]: chi_inliers, chi_outliers, num_inliers, bad-index pairs dropped (may be NULL) */
  float *tri_xyz;                   /* [n_frames][q][3] */
  int32_t *tri_pairs;               /* [n_frames][q][2]  (cur index, slot) */
  float *tri_app;                   /* [n_frames][q][10] or NULL */
  int *counts;                      /* [3][n_frames]: matches, joined pairs, triangulated points */
} vo_frame_batch;
int vo_frames_batch_dev(vo_ctx *ctx, const vo_frame_batch *batch);
/* The same call for frames of DIFFERENT sizes -- the reference's own sequence has 14..127 points per frame
 * (vo_complete.cpp:150-157 runs the loop body on whatever each measurement file holds).  The counts of `batch` are then the
 * capacities (= the strides between frames); frame f really holds sizes->n_ref[f] <= n_ref and n_cur[f] <= n_cur points and
 * n_model_pairs[f] <= n_model_pairs model pairs (device int arrays of n_frames entries).  Every frame picks its own tree --
 * its larger set, the reference image on ties -- exactly like the single-frame call (vo_complete.cpp:15-20); the matcher
 * runs its full scan or, from the sizes on where sorting pays, the cell-hash search.  Outputs, counts and strides as above. */
typedef struct vo_frame_sizes {
  const int *n_ref, *n_cur, *n_model_pairs;
} vo_frame_sizes;
int vo_frames_batch_ragged_dev(vo_ctx *ctx, const vo_frame_batch *batch, const vo_frame_sizes *sizes);
/* The many-frames call with robust tracking (batched form), composed of the stages above:
 * match -> join -> X_prev * model -> vo_estimate_pose_ransac_batch_dev on (moved cloud, cur_pts, joined, counts[1]) ->
 * the solve of vo_picp_solve_batch_dev from the winners on the pairs handed on -> triangulate with the final pose.
 * `batch` and `sizes` (or NULL: uniform sizes) are those of the two calls above and every output of `batch` keeps its
 * meaning: joined / counts[1] hold EVERY joined pair, the filtered ones go to `track`.  The moved cloud is always written
 * (the RANSAC gather reads it): into batch->model_moved when given, else into the context's workspace.  Per frame,
 * status / n_tracked / tracked_pairs / T_winner are d_status / d_n_inliers / d_inlier_pairs / d_T16_out of the batched
 * RANSAC, bit for bit; a frame that fell back (status 1-4) is solved as the plain call solves it. */
typedef struct vo_frame_track {
  vo_ransac_params ransac;
  int     *status;         /* [n_frames] VO_POSE_RANSAC_* */
  int     *n_tracked;      /* [n_frames] pairs handed to the solve */
  int32_t *tracked_pairs;  /* [n_frames][q][2] or NULL */
  float   *T_winner;       /* [n_frames][16] or NULL */
} vo_frame_track;
int vo_frames_batch_track_dev(vo_ctx *ctx, const vo_frame_batch *batch, const vo_frame_sizes *sizes /* or NULL */,
                              const vo_frame_track *track);
/* The matcher alone for n_frames pairs of appearance sets: frame f = d_a1 + f*cap1*10 (d_n1[f] <= cap1 rows) against
 * d_a2 + f*cap2*10 (d_n2[f] <= cap2 rows); d_n1 = d_n2 = NULL: every frame holds cap1 / cap2 rows.  d_out_pairs: [n_frames][min(cap1, cap2)][2] (ref index, cur index), d_n_out[f] = pairs found.  Replaces
 * n_frames calls of compute_correspondences_images (vo_complete.cpp:12-49): the up-front matching of a whole sequence. */
int vo_match_appearances_batch_dev(vo_ctx *ctx, int n_frames, const float *d_a1, int cap1, const int *d_n1,
                                   const float *d_a2, int cap2, const int *d_n2, float radius, int32_t *d_out_pairs,
                                   int *d_n_out);

/* ---- the map (PointCloud.h:52-66; vo_complete.cpp:145-147,175-176,181-183) ---------------------------------------
 * PointCloudVector<3> `map` of vo_complete, resident on the GPU.  map.update(cloud) is the reference's upsert keyed by
 * EXACT equality of the ten appearance floats (operator==: -0 equals +0, a row with a NaN equals nothing, itself
 * included): for every point of the cloud, in order, the first entry with an equal appearance gets the point, otherwise
 * the pair is appended (and found by later points of the same cloud).  Equivalent, and what the kernels compute
 * (map.hip): every class of equal appearances keeps the appearance bits of its first occurrence ever and the point of
 * its last occurrence so far; new classes are appended in the order of their first occurrence in the cloud; NaN rows
 * are always appended.  O(cloud) per update through a hash table of first occurrences (the reference: O(cloud x map)).
 * All calls are enqueued on the context's stream; only vo_map_size / vo_map_read / vo_map_get_history wait.
 * The arrays grow by themselves (a stream synchronisation and a copy when they do: give vo_map_create the capacity a
 * run will need to avoid it; growing is refused inside a graph capture).
 *
 * A CAPTURED UPDATE (vo_map_update_dev between vo_ctx_begin_capture and vo_ctx_end_capture) is admitted while the host's
 * bound of the size says that its n_max rows fit, and refused (VO_ERR_NOT_READY) otherwise; the graph's replays add
 * entries the host does not count.  So, once an update of a map has been captured, calls OUTSIDE a capture no longer
 * trust that bound: vo_map_update[_dev] asks the device for the size first (a stream synchronisation per call) and grows
 * the map when the rows would not fit, vo_map_transform and vo_map_refine_batch_dev reach every entry (they size their
 * work by the capacity).  The graph names the arrays it was captured on: do not replay it after the map has grown.
 *
 * A CALL CAPTURED ON A MAP.  The calls that work on the map's own entries -- vo_map_transform, vo_map_refine_batch_dev,
 * vo_map_refine_poses_batch_dev, vo_map_adjust_batch_dev, vox_map_bundle_batch_dev, voe_map_cull_batch_dev -- size their
 * launches by the host's bound when they are enqueued outside a capture (they run at once: the bound holds), and BY THE
 * CAPACITY when they are enqueued inside one, whatever has been captured before: the graph may hold an update BEHIND the
 * call (the per-frame shape { window call ; vo_map_update_dev }), whose replays add entries before the call's next replay
 * runs, and every replay must see the map it finds.  Their workspaces that are indexed by entry are ALLOCATED for the
 * capacity by every call, eager ones too, so that "one eager call of the same shape, then capture" never has to grow
 * one; an array the caller passes per entry (status, verdict, remap, records) must have room for the size the map can
 * have when a replay runs.  The rule is MapBound of csrc/map_checks.h (launch_bound, alloc_bound).  voe_map_align_dev and
 * voe_map_merge_dev take n_max = voe_map_size_bound(src) at the time of the call, as their header says: captured in front
 * of src's first captured update they see at most that many of its entries (voe_map_covis_batch_dev checks its words
 * against the bound of that time and reads the size itself).
 *
 * OVERFLOW.  A replayed update cannot grow the map.  What then does not fit is dropped: the map holds what the
 * reference's map holds cut to `capacity` entries -- the classes with the earliest first occurrence in the cloud stay,
 * entries already there still take their new points -- and a dropped class is forgotten: sent again it is a new class
 * (and dropped again while the map is full).  Every dropped entry is counted; from then on vo_map_size and vo_map_read
 * fail with VO_ERR_BAD_INDEX and name the running count (vo_map_size still sets *n), until vo_map_clear; so does every
 * host form that reads the size first (vo_map_refine).  The entries, vo_map_dev_ptrs, vo_map_lookup and every *_dev form
 * (lookup, localisation, the refinements, adjustment, bundle, cull, grow, covisibility, alignment and merge) stay valid on
 * the entries the map kept: a dropped class is a miss (tests/test_gpu_map_states.py). */
typedef struct vo_map vo_map;
int vo_map_create(vo_ctx *ctx, int capacity, vo_map **out);
int vo_map_destroy(vo_map *m);
int vo_map_clear(vo_map *m);                                   /* empty map, history = identity */
/* map.update(T * cloud): d_xyz [n_max][3], d_app [n_max][10] (8-byte aligned), *d_n_rows (or NULL) <= n_max rows are
 * live, d_T16 (or NULL: identity) a column-major 4x4 in device memory applied to every point -- `history *
 * triangulated_pc` of vo_complete.cpp:175 with d_T16 = vo_map_history_dev_ptr() -- as PointCloud.h:77-82 does. */
int vo_map_update_dev(vo_map *m, const float *d_xyz, const float *d_app, int n_max, const int *d_n_rows, const float *d_T16);
int vo_map_update(vo_map *m, const float *xyz, const float *app, int n, const float T16[16] /* or NULL */);   /* host arrays */
/* the `history` isometry of vo_complete, kept on the device: reset = X^-1 (vo_complete.cpp:146), step = history * X^-1
 * (:176), both from a pose in device memory (e.g. vo_picp_pose_dev_ptr), in the reference's float arithmetic */
int vo_map_history_reset_dev(vo_map *m, const float *d_X16);
int vo_map_history_step_dev(vo_map *m, const float *d_X16);
int vo_map_history_dev_ptr(vo_map *m, const float **d_T16);
int vo_map_get_history(vo_map *m, float T16[16]);
int vo_map_transform(vo_map *m, const float T16[16]);           /* map = H * map (vo_complete.cpp:183), in place */
int vo_map_size(vo_map *m, int *n);
/* copies min(size, capacity) entries to the host (either array may be NULL); *n_out = size */
int vo_map_read(vo_map *m, float *xyz, float *app, int capacity, int *n_out);
/* the arrays in device memory (entries [0, *d_size)); they move when the map grows */
int vo_map_dev_ptrs(vo_map *m, const float **d_xyz, const float **d_app, const int **d_size);

/* ---- reading the map by appearance (an extension: the reference never reads its map back) --------------------------
 * LOOKUP.  For every live query row (ten floats) the index of the entry map.update() would have found for it: the first
 * entry whose appearance compares equal under operator== on ten floats (-0 equals +0; a row with a NaN equals nothing, so
 * a NaN query finds nothing and a NaN entry is never found), or none.  A read-only probe of the table the updates keep
 * (no atomics, nothing written to the map), then a count / scan / scatter by QUERY index: 3 launches, and a result that is
 * a function of the data alone.  A lookup never grows or changes the map.
 * d_app [n_max][10] (8-byte aligned), *d_n_rows (or NULL) <= n_max rows are live.  Outputs, all in device memory:
 *   d_pairs_out       [n_max][2]  the hits compacted in query order as (query index, entry index) -- the solver's
 *                                 (meas_idx, world_idx) orientation against the map's own arrays (vo_map_dev_ptrs)
 *   *d_n_out                      their count
 *   d_xyz_out         [n_max][3]  or NULL: the point of hit k, gathered in the same order
 *   d_local_pairs_out [n_max][2]  or NULL: (query index, k) -- the same hits indexing d_xyz_out, so that a consumer works on
 *                                 a per-frame point array
 *   d_entry_out       [n_max]     or NULL: per query POSITION the entry, or -1 (also for the positions behind the live rows)
 * Items behind the count are left as they were.
 * Capturable (vo_ctx_begin_capture) once a call of the same shape (n_max, n_frames, with or without d_entry_out) has sized
 * the map's lookup scratch; a capture that would have to grow it is refused (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): a null map or required pointer, appearance rows / pair arrays not 8-byte aligned, a
 * negative count, n_frames outside 1 .. 65535, more than 2^30 rows in one call. */
int vo_map_lookup_dev(vo_map *m, const float *d_app, int n_max, const int *d_n_rows /* or NULL */, int32_t *d_pairs_out,
                      int *d_n_out, float *d_xyz_out /* or NULL */, int32_t *d_local_pairs_out /* or NULL */,
                      int32_t *d_entry_out /* or NULL */);
/* n_frames frames against ONE map in the same 3 launches (the frame is a grid dimension): frame f's rows lie at
 * d_app + 10 * f * app_stride floats (app_stride in ROWS, >= n_max), d_n_rows[f] (or, NULL, n_max) of them live; its
 * outputs lie f * n_max items further (pairs, points, entries) and its count is d_n_out[f].  CONTRACT: frame f's outputs
 * are BIT FOR BIT those of vo_map_lookup_dev on that frame alone. */
int vo_map_lookup_batch_dev(vo_map *m, int n_frames, const float *d_app, size_t app_stride, int n_max,
                            const int *d_n_rows /* [n_frames] or NULL */, int32_t *d_pairs_out, int *d_n_out /* [n_frames] */,
                            float *d_xyz_out /* or NULL */, int32_t *d_local_pairs_out /* or NULL */,
                            int32_t *d_entry_out /* or NULL */);
/* host arrays in, host arrays out (any of xyz_out, entry_out may be NULL; pairs_out has room for n pairs); waits */
int vo_map_lookup(vo_map *m, const float *app, int n, int32_t *pairs_out, int *n_out, float *xyz_out /* or NULL */,
                  int32_t *entry_out /* or NULL */);

/* NEAREST.  The lookup's sibling for appearances that were computed, not copied: for every live row the NEAREST entry
 * within a radius, and the frames' rows CANONICALISED -- every matched row gets the 40 bytes of its entry -- so that the
 * exact lookup above, and with it every map call built on it, finds exactly the association the nearest search decided.
 * (The voe_ names are declared here and not in a ninth extension header: vo_hip.h is a declaring header of the voe_
 * namespace like the eight it includes, and these calls belong next to vo_map_lookup*.  DESIGN.md section 4.23.)
 * Rules; every output is a function of the data alone:
 *   1. d2(q, e) is the matcher's decision: in float32 the unfused left-to-right sum over components 0..9 of (e_k - q_k)^2;
 *      r2 = radius * radius in float32.
 *   2. The best entry of a row has the smallest d2 among the entries with d2 < r2 (strict, and taken only where it evaluates
 *      true: a NaN or an infinity in the row or in the entry never matches).  Exact ties go to the lowest entry index.
 *   3. ratio != 0: with d2_2 the smallest d2 over the OTHER entries with d2 < r2, the row is AMBIGUOUS iff such an entry exists
 *      and d2_best < (ratio * ratio) * d2_2 is false (both products float32).  A second candidate beyond the radius does not count.
 *   4. unique != 0, per frame: among the rows that passed rule 3 an entry keeps the row with the smallest d2, ties to the lowest
 *      row; the others are DISPLACED.  With unique == 0 two rows on one entry are two matches.
 *   5. d_status_out per row POSITION, in this precedence: NOT_LIVE (behind the live count), NAN_ROW (a live row with a NaN),
 *      NO_ENTRY (nothing within the radius), AMBIGUOUS, DISPLACED, MATCHED.  d_entry_out is the entry where MATCHED and -1
 *      otherwise (also behind the live rows, as the lookup writes it); d_dist2_out holds d2_best where MATCHED / AMBIGUOUS /
 *      DISPLACED and +inf otherwise.
 *   6. d_app_out, live rows only (rows behind the count are left as they were): MATCHED the entry's 40 bytes; NO_ENTRY and
 *      NAN_ROW the row's own 40 bytes (they stay the open rows voe_map_grow works on); AMBIGUOUS and DISPLACED the row's own
 *      bytes with component 0 replaced by the quiet NaN 0x7FC00000 (no map call associates such a row, grow opens no track on
 *      it).  d_app_out == d_app is allowed.  CONTRACT: vo_map_lookup_batch_dev on d_app_out returns, at every position of
 *      every frame, the bytes of d_entry_out.  (Two corners where rule 2 and operator== part: a row holding an infinity that
 *      compares equal to an entry, and a radius whose float32 square is 0, are NO_ENTRY here and hits of the lookup.)
 *   7. *d_stats: the counts of rule 5 over all frames, and n_entries, the size the device holds.
 * Frames, app_stride (in rows, >= n_max), d_n_rows and the 8-byte alignment of the rows are the lookup's.  The map is never
 * written and nothing is read back; the launches are a fixed sequence that depends on (n_frames, n_max, the capacity, unique)
 * alone, no launch waits for another workgroup.  The index of the map is built by every call and kept by none.  Capturable
 * once a call of the same shape (n_frames, n_max, unique) has sized the map's workspace; a capture that would have to grow
 * it is refused (VO_ERR_NOT_READY) before anything is enqueued.  Frame f of the batched call is bit for bit the single call.
 * Refused (VO_ERR_INVALID_ARG): the lookup's refusals for the frames; a null params or d_entry_out; a radius that is not
 * finite or <= 0; a ratio that is not finite or outside {0} u (0, 1]; unique outside 0 / 1; reserved != 0; an int32 / float32
 * output off a 4-byte boundary, d_app_out or d_stats off an 8-byte one; d_app_out overlapping d_app without being d_app. */
#define VOE_MAP_NEAREST_MATCHED   0
#define VOE_MAP_NEAREST_NO_ENTRY  1
#define VOE_MAP_NEAREST_AMBIGUOUS 2
#define VOE_MAP_NEAREST_DISPLACED 3
#define VOE_MAP_NEAREST_NAN_ROW   4
#define VOE_MAP_NEAREST_NOT_LIVE  5
typedef struct voe_map_nearest_params { float radius; float ratio; int unique; int reserved; } voe_map_nearest_params;   /* 16 bytes */
typedef struct voe_map_nearest_stats  { int n_frames, n_entries, n_live, n_matched, n_no_entry, n_ambiguous, n_displaced, n_nan; } voe_map_nearest_stats; /* 32 bytes */
int voe_map_nearest_batch_dev(vo_map *m, int n_frames, const float *d_app, size_t app_stride, int n_max,
                              const int *d_n_rows /* [n_frames] or NULL */, const voe_map_nearest_params *p,
                              int32_t *d_entry_out   /* [n_frames][n_max] */,
                              int32_t *d_status_out  /* [n_frames][n_max] or NULL */,
                              float   *d_dist2_out   /* [n_frames][n_max] or NULL */,
                              float   *d_app_out     /* frames laid out as d_app (same stride), or NULL; may be d_app itself */,
                              voe_map_nearest_stats *d_stats /* or NULL */);
int voe_map_nearest_dev(vo_map *m, const float *d_app, int n_max, const int *d_n_rows /* or NULL */, const voe_map_nearest_params *p,
                        int32_t *d_entry_out, int32_t *d_status_out /* or NULL */, float *d_dist2_out /* or NULL */,
                        float *d_app_out /* or NULL */, voe_map_nearest_stats *d_stats /* or NULL */);
/* host arrays in ([n_frames][n_max][10], n_rows [n_frames] or NULL), host arrays out (any but entry_out may be NULL;
 * app_out may be app itself); waits */
int voe_map_nearest(vo_map *m, int n_frames, const float *app, const int *n_rows /* or NULL */, int n_max,
                    const voe_map_nearest_params *p, int32_t *entry_out, int32_t *status_out, float *dist2_out, float *app_out,
                    voe_map_nearest_stats *stats_out);

/* GUIDED.  NEAREST's sibling for a tracker that has a pose prior (the last pose, a motion model, the bundle's result): the
 * candidates of a row are restricted to the entries whose projection under the frame's prior falls within radius_px of the
 * row's pixel -- "projective" association: it tells landmarks that look alike apart by where they must appear.  What it
 * costs follows the density of the projections: every entry in a row's window is tested -- about one where the window is
 * selective (a tracker's local map), hundreds where a dense map projects into the image, and then NEAREST is the faster
 * call (DESIGN.md section 4.24 has the measurements).  The outputs follow NEAREST's convention, so the exact lookup and
 * every call built on it consume the association unchanged (vo_map_localise* with n_hypotheses == 0 and d_T0 = the prior is
 * the consumer this call exists for).  DESIGN.md section 4.24.
 * d_T16 [n_frames][16]: the priors, column-major, p_cam = T p_map, in DEVICE memory (a pose produced on the device feeds
 * the call without a read-back); K [9] column-major on the host; d_uv / uv_stride (pixels) and d_app / app_stride (rows) as
 * in vo_map_localise_batch_dev, both strides >= n_max.  Rules; every output is a function of the data alone:
 *   1. PIXEL.  The pixel of entry e in frame f is Camera::projectPoint in the reference's float32 order (project_point of
 *      vo_math.h; the library is built with contraction off): pc = R p + t, ph = K pc, inv = 1 / ph.z, u = ph.x * inv,
 *      v = ph.y * inv, every three-term sum as x0 + (x1 + x2).  The entry is IN VIEW iff pc.z > 0 and not
 *      (pc.z > z_far || pc.z < z_near).  The image gate of projectPoint is deliberately NOT applied: under a prior that is
 *      off by a few pixels an entry just outside the image may be the row's landmark, and rule 2 already bounds where a
 *      candidate can lie.
 *   2. PIXEL GATE.  g2 = (u_e - u_row)^2 + (v_e - v_row)^2 in float32, unfused, left to right.  e is GATED for the row iff it
 *      is in view and g2 < radius_px * radius_px (the product float32; strict, and taken only where it evaluates true: a NaN
 *      or an infinity in the pose, the entry's point, the projection or the row's pixel never gates).
 *   3. CANDIDATES.  d2 is NEAREST's rule 1, r2 = radius * radius; the candidates of a row are the gated entries with d2 < r2.
 *   4. DECISION.  NEAREST's rules 2 to 4 word for word over the candidates: best is the smallest d2, exact ties to the lowest
 *      entry; ratio is taken against the second-best CANDIDATE (an entry outside the pixel gate or the radius does not count);
 *      unique is per frame, ties to the lowest row.
 *   5. STATUSES.  VOE_MAP_GUIDED_* = VOE_MAP_NEAREST_*, the same precedence (NO_ENTRY: no candidate).  d_entry_out and
 *      d_dist2_out as in NEAREST; d_pix2_out holds g2 of the best candidate where MATCHED / AMBIGUOUS / DISPLACED and +inf
 *      otherwise.
 *   6. CANONICAL ROWS.  d_app_out is NEAREST's rule 6 exactly, the quiet NaN 0x7FC00000 in component 0 of AMBIGUOUS and
 *      DISPLACED rows included; d_app_out == d_app is allowed.  CONTRACT: vo_map_lookup_batch_dev on d_app_out returns, at
 *      every position of every frame, the bytes of d_entry_out.  (The same two corners: a row holding an infinity that compares
 *      equal to an entry, and a radius whose float32 square is 0, are NO_ENTRY here and hits of the lookup.  The window adds
 *      a third of the same kind: a row that compares EQUAL to an entry which is not gated for it -- a copied appearance
 *      whose landmark the prior puts elsewhere -- is NO_ENTRY here, keeps its bytes by NEAREST's rule 6, and is a hit of the
 *      lookup.  A measured appearance never is such a copy; a caller that feeds copies and wants the window to hold
 *      replaces component 0 of its NO_ENTRY rows as rule 6 does for AMBIGUOUS ones.)
 *   7. STATISTICS.  The counts of rule 5 over all frames, n_entries (the size the device holds), n_in_view (the sum over the
 *      frames of the entries in view) and n_gated (the (live row, entry) pairs that pass rule 2): integer sums, exact in any
 *      order.
 *   8. The map is never written and nothing is read back; no float atomics; no launch waits for another workgroup; the
 *      launches are a fixed sequence that depends on (n_frames, n_max, the capacity, unique) alone.  The index (per frame: the
 *      entries in view, sorted into a pixel grid) is built by every call and kept by none.  The host's bound of the size is
 *      not the size (MapBound, map_checks.h): the kernels read the size from the device; captured, the call is sized by the
 *      capacity.  Capturable once a call of the same shape (n_frames, n_max, unique) has sized the map's workspace; a capture
 *      that would have to grow it is refused (VO_ERR_NOT_READY) before anything is enqueued.  Frame f of the batched call is
 *      bit for bit the single call.
 *   9. Refused (VO_ERR_INVALID_ARG): the lookup's refusals for the frames; a null params, d_entry_out, d_uv, d_T16 or K;
 *      radius_px or radius not finite or <= 0; a ratio outside {0} u (0, 1]; unique outside 0 / 1; z_far < z_near; reserved
 *      != 0; uv_stride or app_stride below n_max; d_uv, d_app_out or d_stats off an 8-byte boundary, a 4-byte output or the
 *      poses off a 4-byte one; d_app_out overlapping d_app without being d_app. */
#define VOE_MAP_GUIDED_MATCHED   0
#define VOE_MAP_GUIDED_NO_ENTRY  1
#define VOE_MAP_GUIDED_AMBIGUOUS 2
#define VOE_MAP_GUIDED_DISPLACED 3
#define VOE_MAP_GUIDED_NAN_ROW   4
#define VOE_MAP_GUIDED_NOT_LIVE  5
typedef struct voe_map_guided_params { float radius_px; float radius; float ratio; int32_t unique; int32_t z_near; int32_t z_far; int32_t reserved[2]; } voe_map_guided_params;   /* 32 bytes */
typedef struct voe_map_guided_stats  { int32_t n_frames, n_entries, n_live, n_matched, n_no_entry, n_ambiguous, n_displaced, n_nan; int64_t n_in_view, n_gated; } voe_map_guided_stats; /* 48 bytes */
int voe_map_guided_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                             size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                             const float *d_T16 /* [n_frames][16] */, const voe_map_guided_params *p,
                             int32_t *d_entry_out   /* [n_frames][n_max] */,
                             int32_t *d_status_out  /* [n_frames][n_max] or NULL */,
                             float   *d_dist2_out   /* [n_frames][n_max] or NULL */,
                             float   *d_pix2_out    /* [n_frames][n_max] or NULL */,
                             float   *d_app_out     /* frames laid out as d_app (same stride), or NULL; may be d_app itself */,
                             voe_map_guided_stats *d_stats /* or NULL */);
int voe_map_guided_dev(vo_map *m, const float K[9], const float *d_uv, const float *d_app, int n_max, const int *d_n_rows /* or NULL */,
                       const float *d_T16 /* [16] */, const voe_map_guided_params *p, int32_t *d_entry_out,
                       int32_t *d_status_out /* or NULL */, float *d_dist2_out /* or NULL */, float *d_pix2_out /* or NULL */,
                       float *d_app_out /* or NULL */, voe_map_guided_stats *d_stats /* or NULL */);
/* host arrays in (uv [n_frames][n_max][2], app [n_frames][n_max][10], n_rows [n_frames] or NULL, T16 [n_frames][16]), host
 * arrays out (any but entry_out may be NULL; app_out may be app itself); waits */
int voe_map_guided(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows /* or NULL */,
                   int n_max, const float *T16, const voe_map_guided_params *p, int32_t *entry_out, int32_t *status_out,
                   float *dist2_out, float *pix2_out, float *app_out, voe_map_guided_stats *stats_out);

/* LOCALISATION.  The pose of a camera in the map from one frame alone: T (column-major 4x4, p_cam = T * p_map, the
 * convention of vo_picp_set_pose).  d_uv [n_max][2] pixels and d_app [n_max][10] appearances of the frame, *d_n_rows (or
 * NULL) <= n_max of them live.  Steps, all enqueued on the context's stream, no host round trip:
 *   1. vo_map_lookup_dev with gathered points: world = d_xyz_out [n_max][3], pairs = d_local_pairs_out (query index, k).
 *   2. params->n_hypotheses > 0: vo_estimate_pose_ransac_dev on them (n_world = n_meas = n_max) -- global, no prior needed.
 *      params->n_hypotheses == 0: no RANSAC; d_T0 is REQUIRED, every hit is handed on and the start is T0 (tracking
 *      against the map with a prior).  threshold_px and seed are then not read.
 *   3. n_iters >= 1 PICP rounds (kernel_threshold, keep_outliers = 0) from the winner's pose on its inliers, or from T0 on
 *      every hit, on a solver the map handle owns (created by the first call, which must lie outside a capture).
 *   4. one finishing launch decides the status on the device and writes d_T16_out and *d_stats.
 * Status (vo_map_localise_stats.status), in this order of precedence:
 *   FEW_MATCHES   fewer than 6 hits
 *   NO_CONSENSUS  the RANSAC fell back (its codes 1-3; BAD_INDEX cannot occur, the pairs come from the lookup)
 *   NOT_FINITE    the solved pose holds a NaN or an infinity
 *   FEW_INLIERS   the solver's final inlier count is below min_inliers
 *   OK            otherwise: d_T16_out is the solved pose.
 * When the status is not OK, d_T16_out is T0 BIT FOR BIT when d_T0 was given and the identity otherwise; the statistics
 * are still those of the steps that ran.  The call returns VO_OK either way: a lost frame is a status, not an error.
 * CONTRACT.  The call is a composition plus the finishing launch; it adds no arithmetic of its own.  d_T16_out (status
 * OK) and the statistics equal BIT FOR BIT what the caller gets from the explicit sequence of public calls on the lookup's
 * outputs: vo_map_lookup_dev -> vo_estimate_pose_ransac_dev -> vo_picp_set_camera / vo_picp_set_kernel_threshold /
 * vo_picp_set_points_dev(d_xyz_out, n_max, d_uv, n_max) / vo_picp_set_pose_dev(winner or T0) / vo_picp_solve_dev(pairs
 * handed on, n_max, their device count, 0, n_iters) -> vo_picp_get_pose_dev and vo_picp_get_stats.
 * Capturable once a call of the same shape (n_max, n_hypotheses, camera, threshold) has run outside a capture.
 * Refused (VO_ERR_INVALID_ARG): the lookup's refusals, n_max < 1, n_iters < 1, min_inliers < 0, a singular K, d_T0
 * missing with n_hypotheses == 0, n_hypotheses < 0 or > 65536, with n_hypotheses > 0 a threshold that is not positive and
 * finite, d_uv / d_stats not 8-byte aligned. */
#define VO_MAP_LOCALISE_OK           0
#define VO_MAP_LOCALISE_FEW_MATCHES  1
#define VO_MAP_LOCALISE_NO_CONSENSUS 2
#define VO_MAP_LOCALISE_FEW_INLIERS  3
#define VO_MAP_LOCALISE_NOT_FINITE   4
typedef struct vo_map_localise_stats {
  int32_t status;           /* VO_MAP_LOCALISE_* */
  int32_t n_rows;           /* live rows of the frame */
  int32_t n_hits;           /* rows found in the map */
  int32_t ransac_status;    /* VO_POSE_RANSAC_* (0 when n_hypotheses == 0) */
  int32_t ransac_inliers;   /* pairs handed to the solver: the winner's inliers, every hit on a fallback or without RANSAC */
  int32_t num_inliers;      /* the solver's inlier count after the last round */
  float   chi_inliers, chi_outliers;   /* its two chi^2 sums */
} vo_map_localise_stats;
int vo_map_localise_dev(vo_map *m, int rows, int cols, int z_near, int z_far, const float K[9], const float *d_uv,
                        const float *d_app, int n_max, const int *d_n_rows /* or NULL */, const vo_ransac_params *params,
                        float kernel_threshold, int n_iters, int min_inliers, const float *d_T0 /* 16 floats, or NULL */,
                        float *d_T16_out, vo_map_localise_stats *d_stats);
/* n_frames frames against one map in one call: vo_map_lookup_batch_dev (world stride = n_max, so that the public batched
 * calls compose unchanged) -> vo_estimate_pose_ransac_batch_dev -> vo_picp_solve_batch_dev (n_meas = uv_stride there) ->
 * the finishing launch with the frame as grid dimension.  Frame f reads d_uv + 2 * f * uv_stride floats and d_app + 10 * f *
 * app_stride floats (strides in pixels / rows, both >= n_max), d_n_rows[f] (or n_max) rows, d_T0 + 16 f; it writes
 * d_T16_out + 16 f and d_stats[f].  CONTRACT: bit for bit the explicit batched composition of those public calls.  Against
 * vo_map_localise_dev on the frame alone: hits, RANSAC status, winner and inlier set are bit for bit equal; the solved pose
 * agrees within the 1e-4 stated between the single and the batched solver (their summation orders differ), so the status
 * agrees on every frame whose solver inlier count is not within 1 of min_inliers.  A lost frame leaves its neighbours'
 * outputs alone.  Refusals: those of the single form and of the calls it is composed of. */
int vo_map_localise_batch_dev(vo_map *m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9],
                              const float *d_uv, size_t uv_stride, const float *d_app, size_t app_stride, int n_max,
                              const int *d_n_rows /* [n_frames] or NULL */, const vo_ransac_params *params,
                              float kernel_threshold, int n_iters, int min_inliers, const float *d_T0 /* [n_frames][16] or NULL */,
                              float *d_T16_out /* [n_frames][16] */, vo_map_localise_stats *d_stats /* [n_frames] */);
/* host arrays: uv [n][2], app [n][10], T0 (16 floats, or NULL); two or three uploads, the device call, one read-back of
 * pose and statistics.  Same results bit for bit; returns VO_OK with the status in *stats_out (required). */
int vo_map_localise(vo_map *m, int rows, int cols, int z_near, int z_far, const float K[9], const float *uv,
                    const float *app, int n, const vo_ransac_params *params, float kernel_threshold, int n_iters,
                    int min_inliers, const float T0[16] /* or NULL */, float T_out[16], vo_map_localise_stats *stats_out);

/* REFINEMENT (structure-only adjustment: the poses are fixed, the points move).  Every entry of the map is re-estimated
 * from ALL the rows of n_frames frames that see it, by Gauss-Newton on the reprojection error.  Frame f: pixels d_uv + 2 f
 * uv_stride floats, appearances d_app + 10 f app_stride floats (strides in pixels / rows, both >= n_max), d_n_rows[f] (or
 * n_max) live rows, pose d_T16 + 16 f (column-major 4x4, p_cam = T p_map).  Everything is enqueued on the context's stream:
 * vo_map_lookup_batch_dev with the entry of every query position, the observation lists by entry (count, scan, scatter,
 * order), ONE launch that runs all rounds of every landmark, one launch for the statistics.  The ordering pass compares every
 * observation with the others of its landmark: it is meant for a few to a few thousand observations per landmark, and a
 * landmark seen by n rows costs n^2 reads (n = 10^5: 10^10, about a second of the device).  RULES:
 *   observation  a live row (frame f, position i) whose lookup returns the entry; its key is f * n_max + i; a landmark
 *                consumes its observations in ascending key order; two rows of one frame that hit one entry are two
 *                observations.
 *   cost         sum of rho(e), e = proj(K, T_f p) - uv with q = K p_cam, u = q0 / q2, v = q1 / q2 (the full K; no image or
 *                depth gate: camera z > 0 is a status, below).  huber_px == 0: rho = |e|^2.  huber_px > 0: the Huber cost,
 *                rho = |e|^2 up to |e| = huber_px and huber_px (2 |e| - huber_px) beyond, minimised by IRLS with the weight
 *                w = min(1, huber_px / |e|).
 *   round        H = sum w J^T J + damping I, b = sum w J^T e, p <- p - H^-1 b; the 3x3 solve is an LDL^T in natural order;
 *                sums, solve and p are double; p is rounded to float32 once, after the last round.  n_rounds == 0
 *                evaluates cost and status and writes nothing.
 *   status       per entry, in this order of precedence:
 *                UNSEEN      no observation
 *                FEW_OBS     1 .. min_obs - 1 observations
 *                NOT_FINITE  a sum of some evaluation, the step or the point is not finite, or a pivot is not > 0 (the
 *                            landmark stops there)
 *                BEHIND      at the start, in some round or at the end an observation has camera z that is not > 0
 *                COST_ROSE   the cost of the float32-rounded final point is larger than the cost of the point found
 *                OK          otherwise: the 12 bytes of the point are replaced.  Every other status leaves them bit for bit.
 * d_status_out [map size] (or NULL) receives the status of every entry; with d_xyz_out [map size][3] the map is NOT written
 * and d_xyz_out holds every entry's point, refined or not; *d_stats (8-byte aligned) the census.  cost_before / cost_after
 * are sums over the OK landmarks in double, taken in a fixed order (entries e, e + 1024, ... in entry order into partial sum
 * e mod 1024, the partial sums in order; tests/map_refine_restatement.py sums in the same order, the landmarks' own costs
 * differ from float64 numpy in the last bits).  Every output is a function of the data alone: three calls give the same bytes.
 * Capturable once a call of the same shape (n_frames, n_max, on a map no smaller) has sized the workspace; a capture that
 * would have to grow it is refused (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): the lookup's refusals, n_rounds < 0, min_obs < 2, a negative or non-finite huber_px or
 * damping, a singular K, a null map / K / params / d_T16 / d_stats (d_uv, d_app with n_max > 0), a stride below n_max,
 * d_uv / d_app / d_stats not 8-byte aligned. */
#define VO_MAP_REFINE_OK          0   /* the point was replaced */
#define VO_MAP_REFINE_UNSEEN      1   /* no observation */
#define VO_MAP_REFINE_FEW_OBS     2   /* 1 .. min_obs-1 observations */
#define VO_MAP_REFINE_BEHIND      3   /* at the start, in some round or at the end, an observation has camera z that is not > 0 */
#define VO_MAP_REFINE_NOT_FINITE  4   /* a non-finite sum, a pivot that is not > 0, a non-finite step or point */
#define VO_MAP_REFINE_COST_ROSE   5   /* final cost > initial cost */
typedef struct vo_map_refine_params { int32_t n_rounds; int32_t min_obs; float huber_px; float damping; } vo_map_refine_params;
typedef struct vo_map_refine_stats  { int32_t n_entries, n_obs; int32_t by_status[6]; double cost_before, cost_after; } vo_map_refine_stats;
int vo_map_refine_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride,
                            const float *d_app, size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                            const float *d_T16 /* [n_frames][16], p_cam = T p_map */, const vo_map_refine_params *params,
                            int32_t *d_status_out /* [map size] or NULL */, float *d_xyz_out /* [map size][3] or NULL: NULL = in place */,
                            vo_map_refine_stats *d_stats);
/* host arrays: uv [n_frames][n_max][2], app [n_frames][n_max][10], n_rows [n_frames] (or NULL), T16 [n_frames][16];
 * status_out [vo_map_size] (or NULL).  Uploads, the device call in place, one read-back; the same results bit for bit. */
int vo_map_refine(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows,
                  int n_max, const float *T16, const vo_map_refine_params *params, int32_t *status_out,
                  vo_map_refine_stats *stats_out);

/* FUSE.  Duplicate landmarks of the map found and taken out: two entries that are each other's nearest in appearance AND
 * lie within a radius in space are one landmark entered twice (a revisit under GUIDED whose pixel gate failed and that
 * voe_map_grow appended; a voe_map_merge(KEEP_DST) of two maps with independently measured descriptors).  The step behind
 * the loop chain: voe_map_loops -> voe_pose_graph -> voe_map_apply_correction -> FUSE -> vox_map_bundle.  Appearance alone
 * cannot decide the pairs where appearances repeat; DESIGN.md section 4.25 has the experiment.  (Declared here by the rule
 * NEAREST states.)  Rules; every output is a function of the data alone:
 *   1. GATES.  d2(a, b) is NEAREST's rule 1 between two entries: the float32, unfused, left-to-right sum over components
 *      0..9 of (b_k - a_k)^2; it is bit-symmetric.  g2(a, b) = ((dx * dx + dy * dy) + dz * dz) of the two points in float32,
 *      unfused.  b != a is a CANDIDATE of a iff d2 < radius * radius and g2 < radius_xyz * radius_xyz (both products
 *      float32, both tests strict and taken only where they evaluate true).  An entry with a NaN or an infinity in its
 *      point or in its appearance is NOT_FINITE: it is nobody's candidate and has none.
 *   2. PARTNER.  The candidate with the smallest d2, exact ties to the lowest entry index (NEAREST's rule 2).
 *      d_partner_out[a] is it, or -1; d_dist2_out[a] and d_gap2_out[a] hold its d2 and g2, or +inf.
 *   3. MUTUAL PAIR.  a < b form a PAIR iff partner[a] == b and partner[b] == a.  An entry is in at most one pair.  Chains
 *      are not followed: a caller that wants them fuses again.
 *   4. VETO.  With veto_shared_frame != 0 (frames given), a pair is a CONFLICT iff some frame has a live row whose exact
 *      lookup hits a and one whose exact lookup hits b: a landmark is seen once per frame, two entries seen together are
 *      two landmarks.  Decided on the ordered observation lists of REFINEMENT (key f * n_max + i, ascending) by a merge
 *      walk of the two lists.
 *   5. VERDICT per old entry (d_verdict_out), in this precedence: NOT_FINITE, ALONE (no candidate), NOT_MUTUAL, CONFLICT
 *      (both ends), SURVIVOR (the lower index of a pair), ABSORBED (the higher).
 *   6. EFFECT.  The survivor keeps its 40 appearance bytes and its place in the order.  Its point keeps its 12 bytes
 *      (position == 0) or becomes, per component, float32((double(p_a) + double(p_b)) * 0.5) (position == 1).  ABSORBED
 *      entries are dropped exactly as voe_map_cull drops: stable compaction through a staging area, header and table
 *      rebuilt.  d_remap_out[old] is the new index of the entry, for an ABSORBED entry the new index of its survivor; it is
 *      never -1.  The map afterwards is the map vo_map_update of the survivors, in order, into a cleared map would have built.
 *   7. ROWS.  With frames and d_app_out given, every live row whose exact lookup BEFORE the fuse hits an ABSORBED entry gets
 *      the survivor's 40 bytes; every other live row gets its own bytes from d_app; rows behind the live count are left as
 *      they were.  d_app_out == d_app is allowed.  CONTRACT: vo_map_lookup_batch_dev on d_app_out after the call returns,
 *      position for position, remap[the lookup of d_app before the call] (-1 stays -1).  Two rows of one frame may then hit
 *      one entry; every window call counts that as two observations.
 *   8. dry_run != 0: every per-entry output and *d_stats are written as they would be; the map, its table, its header,
 *      d_app and d_app_out keep every byte.
 *   9. CALL STATUS (stats.status).  OK: something was absorbed (or would be under dry_run).  NOTHING_FUSED: every byte of
 *      the map, its table and its header is left (the compaction and the rebuild still run and return at once behind a
 *      device flag), and the live rows of d_app_out are those of d_app.
 *  10. n_frames == 0 with NULL d_app and d_n_rows means "no frames": there is no veto and no row is rewritten.
 *  11. *d_stats: n_before / n_after the sizes, n_pairs the pairs fused, n_conflicts the pairs vetoed, n_rows_rewritten the
 *      rows of rule 7 that hit an ABSORBED entry (counted with or without d_app_out), by_verdict the census of rule 5,
 *      n_gated the ordered pairs (a, b), a != b, neither NOT_FINITE, with g2 < radius_xyz * radius_xyz: an integer, exact
 *      in any order.
 * The index -- a uniform 3-D grid over the bounding box of the finite points, cells at least 1.001 radius_xyz wide -- is
 * built by every call and kept by none, and no result depends on it.  Everything runs on the context's stream, nothing is
 * read back, the launches are a fixed sequence that depends on (n_frames, n_max, the capacity) alone, no launch waits for
 * another workgroup, every atomic is an integer one.  The size is read on the device.  Capturable once a call of the same
 * shape has sized the workspaces; a capture that would have to grow one is refused (VO_ERR_NOT_READY) before anything is
 * enqueued; a captured call is launched for the capacity (A CALL CAPTURED ON A MAP).  The per-entry outputs have room for
 * the size the map has when the call runs (voe_map_size_bound bounds it).
 * Refused (VO_ERR_INVALID_ARG): the lookup's refusals for the frames, when frames are given; a null params or d_stats; a
 * radius_xyz, then a radius, that is not finite or <= 0; position, veto_shared_frame or dry_run outside 0 / 1; reserved
 * != 0; veto_shared_frame or d_app_out without frames; an int32 / float32 output off a 4-byte boundary, d_app_out or
 * d_stats off an 8-byte one; d_app_out overlapping d_app without being d_app. */
#define VOE_MAP_FUSE_NOT_FINITE 0
#define VOE_MAP_FUSE_ALONE      1
#define VOE_MAP_FUSE_NOT_MUTUAL 2
#define VOE_MAP_FUSE_CONFLICT   3
#define VOE_MAP_FUSE_SURVIVOR   4
#define VOE_MAP_FUSE_ABSORBED   5
#define VOE_MAP_FUSE_OK            0
#define VOE_MAP_FUSE_NOTHING_FUSED 1
typedef struct voe_map_fuse_params { float radius_xyz; float radius; int32_t position; int32_t veto_shared_frame; int32_t dry_run; int32_t reserved[3]; } voe_map_fuse_params;   /* 32 bytes */
typedef struct voe_map_fuse_stats  { int32_t status, n_before, n_after, n_pairs, n_conflicts, n_rows_rewritten; int32_t by_verdict[6]; int64_t n_gated; } voe_map_fuse_stats; /* 56 bytes */
int voe_map_fuse_batch_dev(vo_map *m, int n_frames, const float *d_app /* or NULL: no frames */, size_t app_stride, int n_max,
                           const int *d_n_rows /* [n_frames] or NULL */, const voe_map_fuse_params *p,
                           int32_t *d_partner_out /* [map size] or NULL */, float *d_dist2_out /* [map size] or NULL */,
                           float *d_gap2_out /* [map size] or NULL */, int32_t *d_verdict_out /* [map size] or NULL */,
                           int32_t *d_remap_out /* [map size] or NULL */,
                           float *d_app_out /* frames laid out as d_app (same stride), or NULL; may be d_app itself */,
                           voe_map_fuse_stats *d_stats);
/* host arrays in ([n_frames][n_max][10], n_rows [n_frames] or NULL; n_frames == 0 and app NULL: no frames), host arrays out
 * (per-entry arrays [vo_map_size], any may be NULL; app_out may be app itself; stats_out required); uploads, the device
 * call, one read-back, the same bytes; waits */
int voe_map_fuse(vo_map *m, int n_frames, const float *app, const int *n_rows /* or NULL */, int n_max,
                 const voe_map_fuse_params *p, int32_t *partner_out, float *dist2_out, float *gap2_out, int32_t *verdict_out,
                 int32_t *remap_out, float *app_out, voe_map_fuse_stats *stats_out);

/* KEYFRAMES.  Which frames to keep at all: a frame is redundant when enough of the landmarks it sees are also seen by enough
 * other kept frames (ORB-SLAM's keyframe culling), and redundant frames are dropped one at a time, the most redundant first,
 * because each drop changes the counts of the others.  Like voe_map_window_dev (vo_map_covis.h) the call reads the bit rows
 * ALONE -- d_bits [n_frames][n_words] as voe_map_covis_batch_dev writes them; n_frames, n_words, d_n_rows and n_max mean
 * what they mean there -- and the map is there for the stream and the workspaces: it is neither read nor written.  Every
 * output is an integer and EXACT; no floating point number is formed.  RULES:
 *   1. FLAGS.  d_flags [n_frames] bytes (or NULL: all FREE): VOE_MAP_KEYFRAMES_FREE, _PROTECTED (never dropped) or _GONE --
 *      dropped by an earlier call: its row is ignored, it observes nothing, and it counts as dropped in rule 4.  So a caller
 *      can run the call again on old bit rows.  The host form refuses a byte above 2; the device form, which cannot, treats
 *      such a frame as PROTECTED.
 *   2. QUANTITIES.  seen[f]: the population count of row f; it never changes.  cnt[e]: the frames that are neither GONE nor
 *      dropped so far and whose row has bit e.  red[f]: the bits e of row f with cnt[e] - 1 >= min_observers.
 *   3. CANDIDATE.  f is a candidate iff it is FREE and not dropped, seen[f] >= min_seen,
 *      1000 red[f] >= share_permille seen[f] (int64), and rule 4 holds.
 *   4. GAP (max_gap > 0 only).  With a the nearest frame below f that is neither GONE nor dropped (-1 if none) and b the
 *      nearest above (n_frames if none): b - a - 1 <= max_gap.  The frames are in time order: this bounds the run of missing
 *      frames in the odometry chain.
 *   5. LOOP.  While fewer than max_dropped frames are dropped and a candidate exists, the BEST candidate is dropped: the
 *      highest share red / seen, compared by cross-multiplication in int64; ties go to the lowest frame.  Then cnt follows.
 *      max_dropped == 0 is the analysis alone: nothing is dropped and every verdict is reported.
 *   6. MONOTONE.  red[f] only falls and runs of missing frames only grow: a frame that has once failed the share test or
 *      the gap test is never a candidate again.  The kernels stop reading the rows of such frames during the loop.
 *   7. VERDICT, d_verdict_out [n_frames], the first that holds at the final state: GONE; DROPPED; PROTECTED; EMPTY --
 *      seen < min_seen; NEEDED -- the share test fails; GAP -- the share test passes and rule 4 blocks; LEFT -- still a
 *      candidate, because max_dropped was reached.  The verdict of a PROTECTED or GONE frame is the number of its flag.
 *   8. OUTPUTS.  d_n_rows_out [n_frames]: the frame's live rows (d_n_rows[f], or n_max), 0 for DROPPED and GONE frames --
 *      what vox_map_bundle_batch_dev, vo_map_adjust_batch_dev, vo_map_refine_batch_dev, voe_map_cull_batch_dev,
 *      voe_map_grow_batch_dev and voe_map_loops_batch_dev take over the SAME frame arrays with no gather: a frame with 0 live
 *      rows has no observation.  d_keep_out [n_frames] bytes: 0 for DROPPED and GONE, 1 otherwise.  d_step_out: the step at
 *      which the frame was dropped, or -1.  d_order_out (or NULL): the dropped frames in drop order, then -1.  d_seen_out,
 *      d_red_out: for a dropped frame seen and red at its own step, for every other frame at the final state, for a GONE
 *      frame 0.
 *   9. *d_stats: n_frames; n_kept: neither DROPPED nor GONE; n_dropped; n_gone; n_protected; n_needed; n_blocked: GAP and
 *      LEFT; n_empty.
 * Everything is enqueued on the context's stream and nothing is read back.  The launches are a fixed sequence that depends
 * on (n_frames, n_words, max_dropped) alone -- two per step; the steps behind the last drop return at once on a device flag --,
 * no launch waits for another workgroup, the only atomic is an integer atomicAdd.  Capturable once a call of the same shape
 * (n_frames, n_words) on this map has sized the workspace; a capture that would have to grow it is refused
 * (VO_ERR_NOT_READY) before anything is enqueued.  params is a host value, read when the call is made.
 * Refused (VO_ERR_INVALID_ARG): n_frames outside 1 .. VOE_MAP_COVIS_MAX_FRAMES; n_words < 1 or above 2^26 (a row's count
 * fits an int32); n_max < 0; a null d_bits, params, d_stats or output other than d_order_out; a d_stats that is not 8-byte
 * aligned; min_observers < 1; share_permille outside 0 .. 1000; min_seen < 1; max_gap < 0; max_dropped outside
 * 0 .. VOE_MAP_KEYFRAMES_MAX_STEPS; reserved != 0; in the host form a flag byte above 2. */
#define VOE_MAP_KEYFRAMES_FREE      0     /* flags */
#define VOE_MAP_KEYFRAMES_PROTECTED 1     /* flag and verdict */
#define VOE_MAP_KEYFRAMES_GONE      2     /* flag and verdict */
#define VOE_MAP_KEYFRAMES_LEFT      0     /* verdicts */
#define VOE_MAP_KEYFRAMES_DROPPED   3
#define VOE_MAP_KEYFRAMES_EMPTY     4
#define VOE_MAP_KEYFRAMES_NEEDED    5
#define VOE_MAP_KEYFRAMES_GAP       6
#define VOE_MAP_KEYFRAMES_MAX_STEPS 1024  /* two launches per step: a choice, not a measured limit */
typedef struct voe_map_keyframes_params { int32_t min_observers, share_permille, min_seen, max_gap, max_dropped; int32_t reserved[3]; } voe_map_keyframes_params;   /* 32 bytes */
typedef struct voe_map_keyframes_stats  { int32_t n_frames, n_kept, n_dropped, n_gone, n_protected, n_needed, n_blocked, n_empty; } voe_map_keyframes_stats;   /* 32 bytes */
int voe_map_keyframes_dev(vo_map *m, int n_frames, int n_words, const uint32_t *d_bits, const int *d_n_rows /* [n_frames] or NULL */,
                          int n_max, const uint8_t *d_flags /* [n_frames] or NULL */, const voe_map_keyframes_params *params,
                          int32_t *d_verdict_out /* [n_frames] */, int *d_n_rows_out /* [n_frames] */, uint8_t *d_keep_out /* [n_frames] */,
                          int32_t *d_step_out /* [n_frames] */, int32_t *d_order_out /* [n_frames] or NULL */,
                          int32_t *d_seen_out /* [n_frames] */, int32_t *d_red_out /* [n_frames] */,
                          voe_map_keyframes_stats *d_stats /* 8-byte aligned */);
/* host arrays (n_rows, flags and order_out may be NULL).  Uploads, the device call, one read-back; the same bytes. */
int voe_map_keyframes(vo_map *m, int n_frames, int n_words, const uint32_t *bits, const int *n_rows, int n_max, const uint8_t *flags,
                      const voe_map_keyframes_params *params, int32_t *verdict_out, int *n_rows_out, uint8_t *keep_out,
                      int32_t *step_out, int32_t *order_out, int32_t *seen_out, int32_t *red_out, voe_map_keyframes_stats *stats_out);

/* PRUNE.  One wrong observation taken back.  An association is the 40 appearance bytes of a frame's row; voe_map_nearest,
 * voe_map_guided and voe_map_fuse write them, a Huber weight only makes a wrong one count less, and voe_map_cull can only drop
 * the whole landmark.  This call judges every observation of the window on its own (ORB-SLAM erases observations over chi^2 or
 * with non-positive depth after every local bundle) and hands back rows from which the bad ones are gone -- with two guards,
 * because a row that disagrees with the map may be right: the landmark may be wrong (vo_map_refine's job) or the frame's pose
 * (vo_map_refine_poses').  The chain: nearest / guided -> localise -> bundle -> PRUNE -> bundle -> cull.  Frames, pixels,
 * appearances, d_n_rows, strides, K and d_T16 mean what they mean in voe_map_cull_batch_dev (vo_map_cull.h).  THE MAP, ITS TABLE
 * AND ITS HEADER ARE NEVER WRITTEN.  Every output is a function of the data alone.  RULES:
 *   1. OBSERVATION.  Exactly vo_map_refine's: a live row whose exact lookup returns an entry, with key f * n_max + i.  A
 *      landmark's list is in ascending key.
 *   2. TERMS.  Per observation, in double: sq = |e|^2 and the camera z, by the device function of voe_map_cull (score_obs) and
 *      therefore with its bits.  No Huber weight and no gate apply.
 *   3. HARD TESTS, which need no context.  NOT_FINITE: sq or z is not finite.  BEHIND: z > 0 is false.
 *   4. DUPLICATE, only with unique != 0.  Among the observations of one (entry, frame) that passed rule 3 the one with the
 *      smallest (sq, key) stays; the others are DUPLICATE.
 *   5. ELIGIBLE: the observation passed rules 3 and 4.  n_el: the eligible observations of a landmark.
 *   6. SOFT TESTS, on eligible observations only; HIGH_ERROR goes before RELATIVE.
 *      HIGH_ERROR: max_err_px > 0 and sq > max_err_px^2 (the threshold widened to double, then squared; no square root).
 *      RELATIVE: rel_factor > 0, n_el >= rel_min_obs, sq > rel_factor^2 * med and sq > rel_floor_px^2 (both widened, then
 *      squared; one double product with med).  med is the LOWER MEDIAN: the element of rank (n_el - 1) / 2 (integer division)
 *      of the eligible sq in ascending order -- an exact selection, so no order of evaluation can show.
 *   7. LANDMARK GUARD.  n_soft: the landmark's HIGH_ERROR plus RELATIVE.  If n_soft * 1000 > max_share_landmark * n_el (int64)
 *      the landmark is at fault: every soft observation of it becomes LANDMARK_AT_FAULT and is KEPT.  1000 switches the guard
 *      off; 0 names every landmark with a soft observation.
 *   8. FRAME GUARD, after rule 7.  n_el_f: the frame's eligible observations; n_soft_f: those still HIGH_ERROR or RELATIVE.  If
 *      n_soft_f * 1000 > max_share_frame * n_el_f the frame is at fault: its soft observations become FRAME_AT_FAULT and are
 *      KEPT.  1000 switches it off.
 *   9. STATUS per row POSITION: the VOE_MAP_PRUNE_* below.  NOT_LIVE: the row lies behind the live count.  MISS: live, no entry.
 *      A row is PRUNED when its status is 3 .. 7.
 *  10. OUTPUTS.  d_entry_out [n_frames][n_max]: the entry where the status is 0, 8 or 9; -1 elsewhere, also behind the live
 *      rows.  d_status_out (or NULL): rule 9.  d_sq_out (double, or NULL): sq where the row is an observation, +inf elsewhere.
 *      d_app_out (or NULL; laid out like d_app, and it may BE d_app): live rows only; a pruned row gets its own bytes with
 *      component 0 replaced by the quiet NaN 0x7FC00000 -- NEAREST's rule 6: no map call associates such a row and
 *      voe_map_grow opens no track on it --, every other row its own bytes.  d_landmark_out [size] (or NULL): n_obs, n_el,
 *      n_soft (rule 7's), n_pruned (the landmark's rows with a final status 3 .. 7), at_fault, and med_sq -- 0 where RELATIVE
 *      was not evaluated.  d_frame_out [n_frames] (or NULL): n_obs, n_el, n_soft (rule 8's), at_fault.  *d_stats: n_frames,
 *      n_entries (the map's size), the ten status counts over all positions, n_landmarks_at_fault, n_frames_at_fault, n_obs
 *      (the statuses other than 1 and 2) and n_pruned: integer sums.
 *  11. CONTRACT.  vo_map_lookup_batch_dev on d_app_out returns the bytes of d_entry_out at every position of every frame.  With
 *      rel_factor == 0 and both guards at 1000 a second call on d_app_out prunes nothing, and -- every remaining test being a
 *      matter of the row, or of the rows of one frame on one entry -- frame f of the batched call is bit for bit the single
 *      call on frame f (the landmark records excepted: they count the window).  With a guard or RELATIVE on, neither is
 *      claimed: a pruned row leaves its landmark and its frame, so shares and medians move.
 * Everything is enqueued on the context's stream and nothing is read back.  The launches are a fixed sequence that depends on
 * the shape (n_frames, n_max and the map's bound) alone, no launch waits for another workgroup, and the only atomics are
 * integer ones.  Capturable under the rules of the other map calls: a first call of the shape sizes the workspaces; a capture
 * that would have to grow one is refused (VO_ERR_NOT_READY) before anything is enqueued.  params is a host value, read when the
 * call is made.
 * Refused (VO_ERR_INVALID_ARG): the cull's refusals for the frames (n_frames outside 1 .. 65535, n_max < 0, null pixels or
 * appearances with n_max > 0, d_uv, d_app or d_stats off an 8-byte boundary, a stride below n_max or too large, a singular K,
 * more than 2^30 rows, a null K, d_T16 or d_stats); null params or d_entry_out; max_err_px, rel_factor or rel_floor_px negative
 * or not finite; rel_min_obs < 3; a share outside 0 .. 1000; unique outside 0 / 1; reserved != 0; an int32 output off a 4-byte
 * boundary; d_sq_out, d_app_out, d_landmark_out or d_frame_out off an 8-byte one; d_app_out overlapping d_app without being
 * d_app.  NOT refused: all tests off -- max_err_px == 0, rel_factor == 0 and unique == 0 still runs rule 3. */
#define VOE_MAP_PRUNE_KEPT              0
#define VOE_MAP_PRUNE_NOT_LIVE          1
#define VOE_MAP_PRUNE_MISS              2
#define VOE_MAP_PRUNE_NOT_FINITE        3
#define VOE_MAP_PRUNE_BEHIND            4
#define VOE_MAP_PRUNE_DUPLICATE         5
#define VOE_MAP_PRUNE_HIGH_ERROR        6
#define VOE_MAP_PRUNE_RELATIVE          7
#define VOE_MAP_PRUNE_LANDMARK_AT_FAULT 8
#define VOE_MAP_PRUNE_FRAME_AT_FAULT    9
typedef struct voe_map_prune_params { float max_err_px, rel_factor, rel_floor_px; int32_t rel_min_obs, unique, max_share_landmark, max_share_frame, reserved; } voe_map_prune_params;   /* 32 bytes */
typedef struct voe_map_prune_landmark { int32_t n_obs, n_el, n_soft, n_pruned, at_fault, reserved; double med_sq; } voe_map_prune_landmark;   /* 32 bytes */
typedef struct voe_map_prune_frame { int32_t n_obs, n_el, n_soft, at_fault; } voe_map_prune_frame;   /* 16 bytes */
typedef struct voe_map_prune_stats { int32_t n_frames, n_entries, by_status[10], n_landmarks_at_fault, n_frames_at_fault, n_obs, n_pruned; } voe_map_prune_stats;   /* 64 bytes */
int voe_map_prune_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                            size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */, const float *d_T16,
                            const voe_map_prune_params *params, int32_t *d_entry_out /* [n_frames][n_max] */,
                            int32_t *d_status_out /* [n_frames][n_max] or NULL */, double *d_sq_out /* [n_frames][n_max] or NULL */,
                            float *d_app_out /* like d_app, d_app itself, or NULL */, voe_map_prune_landmark *d_landmark_out /* [size] or NULL */,
                            voe_map_prune_frame *d_frame_out /* [n_frames] or NULL */, voe_map_prune_stats *d_stats /* 8-byte aligned */);
/* one frame: n_frames 1, both strides n_max */
int voe_map_prune_dev(vo_map *m, const float K[9], const float *d_uv, const float *d_app, int n_max, const int *d_n_rows, const float *d_T16,
                      const voe_map_prune_params *params, int32_t *d_entry_out, int32_t *d_status_out, double *d_sq_out, float *d_app_out,
                      voe_map_prune_landmark *d_landmark_out, voe_map_prune_frame *d_frame_out, voe_map_prune_stats *d_stats);
/* host arrays, n_max rows per frame (every output but entry_out may be NULL; landmark_out holds the map's size of records).
 * Uploads, the device call, one read-back; the same bytes. */
int voe_map_prune(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows /* or NULL */, int n_max,
                  const float *T16, const voe_map_prune_params *params, int32_t *entry_out, int32_t *status_out, double *sq_out, float *app_out,
                  voe_map_prune_landmark *landmark_out, voe_map_prune_frame *frame_out, voe_map_prune_stats *stats_out);

#ifdef __cplusplus
}
#endif

/* motion-only refinement of a window's poses on the map's cost and its alternation with vo_map_refine: a header of its own */
#include "vo_map_adjust.h"
#include "vo_map_bundle.h"
#include "vo_map_cull.h"
#include "vo_map_align.h"
#include "vo_map_covis.h"
#include "vo_map_grow.h"
#include "vo_pose_graph.h"
#include "vo_map_loops.h"
#endif /* VO_HIP_H */
