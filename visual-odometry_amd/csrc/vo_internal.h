// vo_internal.h -- declarations shared by the translation units of libvo_hip.so
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "vo_math.h"
#include "lm_pcg.h"

// records the message vo_last_error() returns on this thread and hands `code` back (capi.hip)
int vo_fail(int code, const char* fmt, ...);
extern "C" __attribute__((visibility("hidden"))) int vo_ctx_capturing(struct vo_ctx* ctx);   // 1 while a graph capture is in progress on the context (capi.hip)
extern "C" __attribute__((visibility("hidden"))) int vo_ctx_alive(struct vo_ctx* ctx);       // 0 once the context has been destroyed (handles may outlive it)
extern "C" __attribute__((visibility("hidden"))) unsigned long long vo_ctx_id(struct vo_ctx* ctx);   // unique id of a live context (0: not alive): addresses get recycled, ids do not

namespace vo {

// ---- workspaces ------------------------------------------------------------
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
// Carves a workspace into 256-aligned blocks in the order they are taken; `bytes` is the running size.  The base may be
// null: the blocks are then null too and the walk only measures, so a layout function is also its own size function.
struct WsCarver {
  char* base;
  size_t bytes = 0;
  explicit WsCarver(void* ws) : base(static_cast<char*>(ws)) {}
  template <class T>
  T* take(size_t block_bytes) {
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += up256(block_bytes);
    return p;
  }
  // `off` bytes into a block taken before (a null block stays null)
  template <class T>
  static T* within(void* block, size_t off) { return block ? reinterpret_cast<T*>(static_cast<char*>(block) + off) : nullptr; }
};

// ---- PICP ------------------------------------------------------------------
#ifndef VO_PICP_BLOCK
#define VO_PICP_BLOCK 256
#endif
constexpr int PICP_BLOCK = VO_PICP_BLOCK;   // threads per workgroup of the single-problem kernels (256, 512 or 1024: DESIGN.md section 4.1)
constexpr int PICP_PSTRIDE = 32;      // floats per workgroup partial (NACC padded)
constexpr int PICP_MAX_BLOCKS = 2048; // grid cap (grid-stride beyond it)
#ifndef VO_PICP_REPLICAS
#define VO_PICP_REPLICAS 2
#endif
// Copies of the workgroup partial rows.  Every workgroup of a launch reads ALL the rows the previous launch wrote -- 196
// workgroups fetching the same 25 KB at the same instant from the memory side (the rows come from all eight XCDs): with two
// copies (a writer stores its row twice, a reader takes copy blockIdx.x % 2) the round of the 50k headline takes 4.48-4.50
// instead of 4.57-4.58 us; four copies 4.50, eight 4.55 (the stores), three 4.63 (the modulo).
constexpr int PICP_REPLICAS = VO_PICP_REPLICAS;
// Slots of the round-to-round hand-off (workgroup partial rows, pose): round `it` reads slot (it - 1) % PICP_SLOTS and writes
// slot it % PICP_SLOTS.  Two would do for rounds enqueued one at a time; more let vo_picp_one_round enqueue up to PICP_SLOTS - 2
// rounds AHEAD of its caller (capi.hip) without touching the slot of the last counted round.  Sixteen, with windows of eight
// rounds: consecutive windows of a loop then start at two alternating slots only, i.e. TWO launch graphs serve a loop.
#ifndef VO_PICP_SLOTS
#define VO_PICP_SLOTS 16
#endif
constexpr int PICP_SLOTS = VO_PICP_SLOTS;     // a power of two
constexpr int PICP_BATCH_BLOCK = 768;   // 12 waves: 3 per SIMD, 168 VGPRs each (room for load double-buffering)
constexpr int PICP_BATCH_LDS_TRIPS = 2;   // trips of the batched solver held in LDS across rounds (2 x 60 KiB)

// Solver parameters, resident in device memory so that a captured graph of
// iteration launches stays valid when the camera / threshold / count change.
struct PicpParams {
  CamK cam;
  float thr;
  float damping;
  int keep_outliers;
  int n_corr;
};

// Cycle detection of a launch-per-round solve (picp.hip, "rounds whose pose has already occurred").  The control block is
// reset by round 0 of every solve and written by the detector workgroup alone.  Its state is ONE word, the first launch
// that skips: PICP_CYCLE_RUN while every round runs, d + 1 once the detector of launch d has found a repeat -- the
// workgroups of launch d itself, which read the word while the detector writes it, take either value as "run".
constexpr int PICP_HIST = 64;                  // poses kept (a power of two, at most a wave's lanes): repeats up to 63 rounds back are seen
constexpr int PICP_CYCLE_RUN = 0x7fffffff;
struct PicpCycle {
  int skip_from;       // launches it >= skip_from skip (state SKIP), PICP_CYCLE_RUN: none does (state RUN)
  int target;          // round whose pose (hist[target % PICP_HIST]) is the pose of the last round launch
  int detected_at;     // reporting: launch that first found a repeat (0: none), the repeat's period, launches skipped
  int period;
  int skipped;
};

// The tail launch of a launch-per-round solve (picp.hip, picp_tail_kernel): rounds PICP_TAIL_FROM + 1 .. last share ONE launch.
// After a detected repeat that launch does the last round's work from the history and nothing else; where nothing has repeated
// yet it runs the rounds in a loop, with a grid barrier over all its workgroups between two rounds.  VO_PICP_TAIL_FROM in the
// environment overrides the index per call (>= 1), VO_PICP_TAIL=0 switches the form off per call.
constexpr int PICP_TAIL_FROM = 16;
// what a workgroup waits at most at the grid barrier before it gives the solve up (a safety net: the host only picks the form
// where every workgroup of the launch has a CU to itself), in ticks of the constant 100 MHz clock: 100 ms
constexpr unsigned long long PICP_TAIL_WAIT_TICKS = 10ull * 1000 * 1000;
// The tail launch's words.  They lie BEHIND the history (the offsets of the control block and of the history are part of the
// documented layout, include/vo_hip.h) and are zeroed with the control block by round 0 of every solve.
struct PicpTail {
  int used;            // reporting: the last solve went through the tail launch
  int rounds;          // reporting: real rounds (rows summed, system solved) that ran inside it
  int aborted;         // a workgroup waited PICP_TAIL_WAIT_TICKS at the barrier: the solve's results are void (the getters report it)
  int bar;             // the barrier's monotonic arrival counter
};
// How the tail launches of a handle went, counted over its life (never reset): the launch's workgroup 0 adds one to `straight`
// (it took the skip path) or to `looped` (real rounds ran inside it, each several times the price of a launched round) and
// copies the new count into the handle's host-visible report, from which the host decides the form of later solves without
// ever waiting for the device (capi.hip, picp_tail_policy).
struct PicpTailTally {
  int straight;
  int looped;
};
// The tail launch also CLOSES the solve (there is no finishing launch behind it): its workgroup 0 does the finishing launch's
// work -- the rows of round N - 1 summed, the system solved, pose[0], T16, H, b, statistics -- in one of four ways:
//   RING       state SKIP and the rows launch `target` stored still lie in the ring (picp_tail_ring_holds): they ARE the rows
//              launch N - 1 would store, so nothing is linearised; every other workgroup returns behind the control word;
//   RECOMPUTED state SKIP, slot overwritten (or VO_PICP_TAIL_RING=0): every workgroup linearises with hist[target], stores its
//              row, arrives on PicpTail::bar and leaves; workgroup 0 waits for all arrivals;
//   LOOPED     the launch ran round N - 1 as a real round at the end of its loop: closed like RECOMPUTED.
// The words lie behind the tally so that no earlier offset moves; like the tally they are written by tail launches only and
// never reset: `how` and `m` describe the last solve THAT HAD a tail launch (PicpTail::used tells whether the last solve did).
//   EARLY      (the early form of the launch, below) state RUN, and the workgroups found the repeat themselves in the round that
//              computed the repeating pose: closed from the sums in hand, from the ring, or recomputed, with nobody waiting for
//              a detector.
constexpr int PICP_CLOSE_NONE = 0, PICP_CLOSE_RING = 1, PICP_CLOSE_RECOMPUTED = 2, PICP_CLOSE_LOOPED = 3, PICP_CLOSE_EARLY = 4;
struct PicpTailClose {
  int how;             // PICP_CLOSE_*
  int m;               // the M that solve ran with (rounds 1 .. M had launches of their own)
  int run;             // consecutive tail launches of this handle that took the skip path, since the last one with real rounds
  int max_detected;    // the largest detected_at among them
};
// The rows launch `target` stored in slot target % PICP_SLOTS are intact when launch skip_from - 1, the last one that stored
// rows, has not come round to that slot: it wrote slot (skip_from - 1) % PICP_SLOTS last, launch target + PICP_SLOTS would
// have been the first to overwrite.  (target >= j and skip_from = k + 2 for a repeat pose k = pose j: a period of 14 or less
// always holds.)  target = 0 is included: the gathering round stores the same 30 sums as any round plus the dropped-pair
// tally in slots 30 and 31, which the closing -- like the FINISH instantiation of a solve of two or more rounds -- never sums.
__host__ __device__ inline bool picp_tail_ring_holds(int skip_from, int target) {
  return target >= 0 && skip_from - 1 - target < PICP_SLOTS;
}
// The early form of the tail launch (picp.hip, picp_tail_kernel<.., EARLY>): in state RUN every workgroup of in-launch round
// `it` compares the pose it has just computed, pose `it`, and the pose it started from, pose it - 1, with the history itself.
//   hits_new  bit l: pose `it` equals the pose of round it - 1 - l      (l = 0 .. PICP_HIST - 2; l = 0 is the old pose)
//   hits_old  bit l: pose it - 1 equals the pose of round it - 2 - l    (the window the detector of launch `it` looks through)
// The FIRST repeat is the old pose's where it has one -- the detector workgroup of the same round finds exactly that one and
// stores the same words --, the new pose's otherwise; the most recent match wins, as in picp_cycle_detect.  Answers whether
// there is one, and then pose k = pose j.
__host__ __device__ inline bool picp_tail_first_repeat(unsigned long long hits_new, unsigned long long hits_old, int it, int* k, int* j) {
  if (hits_old) { *k = it - 1; *j = it - 1 - (__builtin_ctzll(hits_old) + 1); return true; }
  if (hits_new) { *k = it; *j = it - (__builtin_ctzll(hits_new) + 1); return true; }
  return false;
}
// What the launch-per-round solve makes of the repeat pose k = pose j (picp_cycle_detect in launch k + 1; last = N - 1 is the
// last round launch): it skips where a launch is left to skip; then launches from k + 2 on skip, and the pose of round `last`
// is the pose of round `target`.
struct PicpSkip {
  int detected_at, period, skipped, target, skip_from;
};
__host__ __device__ inline bool picp_cycle_skips(int k, int last) { return k + 2 < last; }
__host__ __device__ inline PicpSkip picp_cycle_skip(int k, int j, int last) {
  const int period = k - j;
  return PicpSkip{k + 1, period, last - 2 - k, j + (last - j) % period, k + 2};
}
// the host's report (pinned memory, launch_picp_rounds' tail_report): [0], [1] the tally's two counts; [2] run << 16 |
// max_detected (each saturating at 0xffff) in ONE word, so that the host never reads a torn pair; [3] behind a launch that ran
// real rounds: looped << 16 | the last round it ran (first + real - 1, saturating), the count's low half as a consistency tag
constexpr int PICP_TAIL_REPORT_WORDS = 4;
// the host lowers M only once this many consecutive tail launches have taken the skip path (capi.hip, picp_tail_policy)
constexpr int PICP_TAIL_LEARN = 8;
// ... and takes the early form, at M = largest detected_at - 2, once this many have: that M leaves no margin round, so it asks
// for four times the witnesses
constexpr int PICP_TAIL_EARLY_LEARN = 32;

// Solver state in device memory.
struct PicpState {
  float pose[PICP_SLOTS][12];   // ring (slot = round % PICP_SLOTS; slot 0 also holds the finished pose): R (col-major 3x3) then t
  float H[36];         // last round, damping included (col-major)
  float b[6];
  float chi_in, chi_out;
  int n_in;
  int n_bad;           // correspondences whose indices were out of range (dropped)
  float T16[16];       // pose after the last solve as a column-major 4x4 (written by the finish launch)
  PicpCycle cyc;       // directly behind T16: include/vo_hip.h documents this layout at vo_picp_pose_dev_ptr
  float hist[PICP_HIST][12];    // hist[k % PICP_HIST]: the pose after round k of this solve (pose[k % PICP_SLOTS] when it was written)
  PicpTail tail;       // directly behind the history
  PicpTailTally tally;
  PicpTailClose close; // behind the tally (the offsets before it are pinned by tests and by include/vo_hip.h)
#ifdef VO_STAMPS
  // diagnostic build only (make STAMPS=1 -> libvo_hip_stamps.so, tools/stamp_rounds.py):
  // s_memtime at phase boundaries of workgroup 0, per round
  unsigned long long stamps[128][8];
#endif
};

// packed correspondences: five SoA arrays of `cap` floats each (x,y,z,u,v)
struct PackedCorr {
  float* base;
  size_t cap;
  __host__ __device__ const float* arr(int k) const { return base + (size_t)k * cap; }
  __host__ __device__ float* arr(int k) { return base + (size_t)k * cap; }
};

// d_T0 (may be null): column-major 4x4 in device memory that becomes the solver's pose
hipError_t launch_picp_pack(hipStream_t st, const int32_t* d_pairs, const int* d_n, int n_max,
                            const float* d_world, int n_world, const float* d_meas, int n_meas,
                            PackedCorr pk, PicpParams* d_params, PicpState* d_state, const float* d_T0);

// What round 0 of a solve gathers (the arguments of launch_picp_pack): with `on` it does what launch_picp_pack does -- and the
// memset of n_bad: the tally of dropped pairs travels in the partial rows, the next launch stores it -- before it linearises;
// without, the packed arrays are taken as they are.
struct PicpGather {
  const int32_t* pairs = nullptr;
  const int* d_n = nullptr;
  int n_max = 0;
  const float* world = nullptr;
  int n_world = 0;
  const float* meas = nullptr;
  int n_meas = 0;
  const float* T0 = nullptr;
  int on = 0;
};
// Enqueue n_iters Gauss-Newton rounds (n_iters+1 launches).  d_partials holds
// PICP_REPLICAS * PICP_SLOTS * round_up(grid,256) * PICP_PSTRIDE floats, zero-initialised.
// part: the whole solve, round 0 alone, or everything behind round 0 -- the host replays the latter as a captured graph behind
// a plain launch of round 0, whose arguments are the caller's and change from call to call.  The parts exist where the rounds
// are launches of their own (picp_rounds_chain(grid)).
// cycle: launches behind round 0 carry the detector workgroup and skip rounds whose pose has already occurred in this solve
// (picp.hip, picp_cycle_detect); results are the same bytes either way.
// tail_from: 0, or the index M of the last round with a launch of its own -- rounds M + 1 .. n_iters - 1 are then ONE launch of
// grid + 1 workgroups that must all be resident together (picp_tail_from decides; picp.hip, picp_tail_kernel).
constexpr int PICP_WHOLE = 0, PICP_ROUND0 = 1, PICP_AFTER_ROUND0 = 2;
hipError_t launch_picp_rounds(hipStream_t st, PicpParams* d_params, PicpState* d_state,
                              PackedCorr pk, float* d_partials, int grid, int n_iters, bool pinhole,
                              bool keep_outliers, const PicpGather& g = PicpGather{}, int part = PICP_WHOLE, bool cycle = false,
                              int tail_from = 0, int* tail_report = nullptr, bool tail_ring = true, bool tail_early = false);
// the tail form's M for a solve of n_iters rounds on `grid` workgroups (picp_grid_for), or 0 where the solve keeps a
// launch per round: too few rounds, no cycle detection, the form switched off, or a grid that would not leave every workgroup
// of the tail launch -- the detector included -- a CU of its own.  Reads VO_PICP_TAIL and VO_PICP_TAIL_FROM; *forced (may be
// null) tells whether either of them asks for the form explicitly (VO_PICP_TAIL=1, or any VO_PICP_TAIL_FROM).
// tail_report (launch_picp_rounds): PICP_TAIL_REPORT_WORDS host-visible ints (above), or null.  tail_ring: false forces the
// RECOMPUTED closing where RING would do (VO_PICP_TAIL_RING=0, read per call by picp_tail_ring_enabled: tests and the A/B).
// m_default: the M to use where VO_PICP_TAIL_FROM does not set one (the handle's learned M: picp_tail_policy).
// tail_early: the tail launch is the early form (VO_PICP_TAIL_EARLY, read per call by picp_tail_early_env: 1 adds it to a
// forced M, 0 keeps the host from choosing it, -1: not set).
int picp_tail_from(int grid, int n_iters, bool cycle, int n_cu, bool* forced = nullptr, int m_default = PICP_TAIL_FROM);
bool picp_tail_ring_enabled();
int picp_tail_early_env();

int picp_grid_for(int n_corr, int n_cu);

// A chain of rounds whose finishing launch is deferred (vo_picp_one_round): round `it` is one launch; launch_picp_finish
// closes a chain of n_rounds.  picp_rounds_chain(grid): false when launch_picp_rounds runs this size as ONE launch anyway
// (a single workgroup: picp_small_kernel), which leaves nothing to defer.
bool picp_rounds_chain(int grid);
hipError_t launch_picp_chain_round(hipStream_t st, const PicpParams* d_params, PicpState* d_state, PackedCorr pk,
                                   float* d_partials, int grid, int it, bool pinhole, bool keep_outliers);
hipError_t launch_picp_finish(hipStream_t st, const PicpParams* d_params, PicpState* d_state, PackedCorr pk,
                              float* d_partials, int grid, int n_rounds);

// Reference-order solver (bit-identical to the reference's scalar arithmetic): n_iters rounds in one launch of one
// workgroup; reads the packed correspondences and P->n_corr, leaves pose / T16 / H / b / statistics in *d_state.
hipError_t launch_picp_exact(hipStream_t st, const PicpParams* d_params, PicpState* d_state, PackedCorr pk,
                             int n_iters);

struct BatchArgs {
  CamK cam;
  float thr, damping;
  int keep_outliers;
  int n_iters;
  int n_problems;
  const float* world; size_t world_stride;   // strides in points
  const float* meas; size_t meas_stride;
  const int32_t* pairs; size_t pairs_stride; // stride in pairs
  const int* n_pairs;
  const float* T0;     // n_problems x 16 or null
  float* T_out;        // n_problems x 16
  float* stats_out;    // n_problems x 4 or null
  float* packed;       // workspace: n_problems x 5 x cap floats
  size_t cap;          // per-array capacity (multiple of 4)
  int n_world, n_meas; // bounds for index checks (per problem)
  // launch-per-round form only (a few problems, many workgroups each): per-problem state and partial buffers
  PicpState* states;   // n_problems, or null (one-workgroup-per-problem kernel)
  float* partials;     // n_problems x 2 x round_up(grid,256) x PICP_PSTRIDE floats, zero-padded rows
  const PicpParams* params;   // device copy of (cam, thr, damping, keep_outliers); n_corr unused
  int grid;            // workgroups per problem
  int pack_gx;         // workgroups per problem of the gather pass
  int* n_bad;          // n_problems counters (zeroed by the caller): correspondences dropped for a bad index, or null
  int exact;           // reference-order form (picp_exact_kernel): one workgroup per problem, sequential sums
  int help_sched;      // test hook (VO_PICP_HELP_SCHEDULE, picp.hip: help_env): scripted late or absent waves, packed (help_sched_*
                       //   below).  Mode 0 takes the product instantiation, any other the one with the hooks compiled in.
  const float* X_world;  // n_problems x 16 (column-major) or null: the gather applies X * p to every world point it fetches
                         //   (X_curr * triangulated_pc of vo_complete.cpp:159 without the pass that writes the moved cloud)
  int prepacked;         // the packed arrays are already filled (the join's writing pass gathered through its own pairs:
                         //   launch_join_batch with a sink): no gather pass
  int help_polls;        // test hook, mode home-stall: the polls a helper wave of a stalled home has for the withheld pose
  // fewer problems than CUs (picp_batch_shared_kernel): the workgroups beyond n_problems take trips off the problems' own
  unsigned long long* help_words;   // picp_help_words(n_problems, n_cu) tagged words, zeroed by launch_picp_batch; null: form off
  int help_grid;         // workgroups of the launch (n_problems + helpers), 0: form off
  int help_rows;         // partial rows in help_words
  int help_absent;       // test hook (VO_PICP_HELP_ABSENT=1): the helper waves leave at once, the homes stand in for all of them
  int help_keep, help_g, help_slack10;   // 0: the kernel's own choice (experiments: VO_PICP_HELP_KEEP / _G / _SLACK): trips a home keeps,
                         //   wave-trips per chunk, a helper's overhead per round in tenths of a trip
};
// The two test-hook words sit where the struct had padding: the kernels' hidden arguments follow it in the kernarg segment,
// so its size is part of the instruction stream of every kernel that takes it.
static_assert(sizeof(BatchArgs) == 272, "BatchArgs grew: the offsets of the hidden kernel arguments move in every kernel that takes it");
// help_sched: mode | mod << 4 | rem << 12 | round << 20
enum { HELP_SCHED_OFF = 0, HELP_SCHED_NONE = 1, HELP_SCHED_LEAVE = 2, HELP_SCHED_STALL = 3, HELP_SCHED_HOME_STALL = 4 };
constexpr int HELP_SCHED_MAX_MOD = 255, HELP_SCHED_MAX_ROUND = 4095;
inline int help_sched_pack(int mode, int mod, int rem, int round) { return mode | mod << 4 | rem << 12 | round << 20; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int help_sched_mode(int s) { return s & 15; }
hipError_t launch_picp_batch(hipStream_t st, const BatchArgs& a);
// the shared form: whether it serves this call, and what it needs (rows of 32 words, then 16 words per problem)
bool picp_batch_shares(int n_problems, size_t cap, int n_iters, int n_cu);
int picp_help_rows(int n_problems, int n_cu);
void picp_help_args(BatchArgs& a, unsigned long long* words, int n_cu);     // words null: form off
inline size_t picp_help_words(int n_problems, int n_cu) { return (size_t)picp_help_rows(n_problems, n_cu) * 32 + (size_t)n_problems * 16; }
#if defined(__HIPCC__)
// What the gather does for correspondence i of problem p: (measurement m, world point w) -> packed x, y, z, u, v; an index
// outside its array leaves the marker and is counted (picp_batch_pack_kernel and the join's writing pass share this).
// in two halves, so that a caller can request the point and the pixel before it knows the slot they go to
struct PackedItem { float x, y, z, u, v; };
__device__ __forceinline__ PackedItem batch_pack_load(const BatchArgs& a, int p, const Pose& Xw, int m, int w) {
  const float* world = a.world + 3 * (size_t)p * a.world_stride;
  const float* meas = a.meas + 2 * (size_t)p * a.meas_stride;
  PackedItem it{__int_as_float((int)VO_DROPPED_BITS), 0.f, 0.f, 0.f, 0.f};
  if (m >= 0 && m < a.n_meas && w >= 0 && w < a.n_world) {
    it.x = world[3 * (size_t)w]; it.y = world[3 * (size_t)w + 1]; it.z = world[3 * (size_t)w + 2];
    if (a.X_world) { const float px = it.x, py = it.y, pz = it.z; pose_apply(Xw, px, py, pz, it.x, it.y, it.z); }   // PointCloud.h:80, as transform_batch_kernel
    it.u = meas[2 * (size_t)m]; it.v = meas[2 * (size_t)m + 1];
  } else if (a.n_bad) {
    atomicAdd(&a.n_bad[p], 1);        // dropped (marker) and counted: reported in stats_out[4p + 3]
  }
  return it;
}
__device__ __forceinline__ void batch_pack_store(const BatchArgs& a, int p, size_t i, const PackedItem& it) {
  float* dst = a.packed + (size_t)p * 5 * a.cap;
  dst[i] = it.x; dst[a.cap + i] = it.y; dst[2 * a.cap + i] = it.z; dst[3 * a.cap + i] = it.u; dst[4 * a.cap + i] = it.v;
}
__device__ __forceinline__ void batch_pack_item(const BatchArgs& a, int p, const Pose& Xw, size_t i, int m, int w) {
  batch_pack_store(a, p, i, batch_pack_load(a, p, Xw, m, w));
}
__device__ __forceinline__ Pose batch_pack_pose(const BatchArgs& a, int p) {
  Pose Xw;
#pragma unroll
  for (int k = 0; k < 9; ++k) Xw.R[k] = (k % 4 == 0) ? 1.f : 0.f;
  Xw.t[0] = Xw.t[1] = Xw.t[2] = 0.f;
  if (a.X_world) {
    float t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = a.X_world[16 * (size_t)p + k];
    Xw = pose_from_T16(t);
  }
  return Xw;
}
#endif
// when is the launch-per-round form the faster one?  (measured: DESIGN.md section 4.1)
bool picp_batch_prefers_rounds(int n_problems, size_t cap, int n_iters, int n_cu);

// ---- frame-major grids ------------------------------------------------------------------------------
// A batched kernel runs `nb` workgroups for each of `n_frames` frames.  Launched as grid (nb, n_frames) consecutive
// workgroups of one frame are dealt round-robin over the 8 XCDs, so the frame's gather targets (its points, appearances,
// index tables: 0.2 .. 2 MB) are pulled into every XCD's L2.  From 8 frames on the launch is 1-D instead
// (frame_grid) and frame_block() maps blockIdx.x so that all workgroups of a frame share blockIdx.x mod 8, i.e. one XCD
// and its L2 (observed placement; speed only, nothing depends on it).
struct FrameBlock { int f, b, nb; bool live; };
#if defined(__HIPCC__)
__device__ __forceinline__ FrameBlock frame_block(int nb, int n_frames) {
  FrameBlock r;
  if (n_frames < 8) { r.f = (int)blockIdx.y; r.b = (int)blockIdx.x; r.nb = nb; r.live = true; return r; }
  const unsigned L = blockIdx.x, s = L >> 3;
  r.f = (int)(s / (unsigned)nb) * 8 + (int)(L & 7u);
  r.b = (int)(s % (unsigned)nb);
  r.nb = nb;
  r.live = r.f < n_frames;
  return r;
}
#endif
inline dim3 frame_grid(int nb, int n_frames) {
  return n_frames < 8 ? dim3((unsigned)nb, (unsigned)n_frames) : dim3(8u * (unsigned)((n_frames + 7) / 8) * (unsigned)nb);
}

// ---- geometry / matcher / join (geom.hip, match.hip) -------------------------
struct Workspace;  // scratch owned by the context

// d_scratch: compaction_scratch_ints(n) ints (per-workgroup counts / offsets)
size_t compaction_scratch_ints(int n);
size_t join_scratch_bytes(int n_img, int n_frames);      // d_scratch of launch_join[_batch]
size_t triangulate_scratch_bytes(int n, int n_frames);   // d_scratch of launch_triangulate[_batch]
hipError_t launch_project_points(hipStream_t st, const CamK& cam, const Pose& T, const float* d_world,
                                 int n, int keep_indices, float* d_out_uv, int* d_counts,
                                 int* d_scratch);

hipError_t launch_transform_points(hipStream_t st, const Pose& T, const float* d_in, int n,
                                   const int* d_n, float* d_out);
hipError_t launch_transform_points_devpose(hipStream_t st, const float* d_T16, const float* d_in, int n,
                                           const int* d_n, float* d_out);

hipError_t launch_triangulate(hipStream_t st, const float K[9], const Pose* X_host,
                              const float* d_X16, const int32_t* d_pairs, int n, const int* d_n,
                              const float* d_p1, int n1, const float* d_p2, int n2,
                              const float* d_app2, float* d_out_xyz, int32_t* d_out_pairs,
                              float* d_out_app, int* d_n_out, int* d_scratch);

hipError_t launch_join(hipStream_t st, const int32_t* d_img, int n_img, const int* d_n_img,
                       const int32_t* d_world, int n_world, const int* d_n_world, int n_ref,
                       int32_t* d_out, int* d_n_out, unsigned long long* d_table /* n_ref words */,
                       int* d_scratch);

// How one matcher call searches: the full scan (no workspace), the bucket-pruned scan or the cell-hash search, and whether the
// exact-duplicate pass ("hash-first", match.hip) runs in front of a sorted search, which then only sees the queries the pass
// left open.  capi.hip (match_plan) turns the public mode 0..5 into a plan; nothing below it sees the mode.  The workspace of a
// plan holds match_workspace_bytes(plan, nt, nq, n_frames) bytes: the pass's block first, then the search's.
enum class MatchSearch { Scan, Buckets, Cells };
struct MatchPlan {
  MatchSearch search = MatchSearch::Scan;
  bool hash_first = false;
};
// after a call that ran the exact-duplicate pass on d_prune_ws: *d_out = 1 when at least one frame took it
hipError_t launch_match_hint(hipStream_t st, const void* d_prune_ws, int n_frames, int* d_out);
// after a call that ran WITHOUT the pass: *d_out = 1 when one of eight sample queries of some frame found its match at distance 0
hipError_t launch_match_hint_from_best(hipStream_t st, const unsigned long long* d_best, size_t best_stride, int nq_cap,
                                       const int* d_n1, const int* d_n2, int n_frames, int* d_out);
size_t match_pruned_workspace_bytes(int nt, int nq, int n_frames);
size_t match_cells_workspace_bytes(int nt, int nq, int n_frames);
size_t match_hash_workspace_bytes(int nt, int n_frames);
bool match_cells_supported(int nt, int nq);   // set sizes the cell-hash search takes (beyond: the bucket-pruned scan)
bool match_hash_supported(int nt, int n_frames);   // tree sizes the exact-duplicate pass takes (beyond: the general search alone)
inline size_t match_workspace_bytes(MatchPlan p, int nt, int nq, int n_frames) {
  return (p.hash_first ? match_hash_workspace_bytes(nt, n_frames) : 0) +
         (p.search == MatchSearch::Cells     ? match_cells_workspace_bytes(nt, nq, n_frames)
          : p.search == MatchSearch::Buckets ? match_pruned_workspace_bytes(nt, nq, n_frames) : 0);
}
// n_frames frames of identical set sizes, frame f at base + f*stride (strides in floats / pairs);
// d_best: n_frames*min(n1,n2) keys; d_scratch: n_frames * compaction_scratch_ints(min(n1,n2)) ints; d_n_out[n_frames]
// d_n1 / d_n2 (both or neither): ragged frames -- frame f holds d_n1[f] <= n1 and d_n2[f] <= n2 points (n1, n2 are then the
// capacities, the strides must be >= them) and picks its own tree (its larger set); the full scan or the cell-hash search
// d_prune_ws: the plan's workspace (null: the full scan whatever the plan says)
hipError_t launch_match_batch(hipStream_t st, const float* d_a1, int n1, size_t a1_stride, const float* d_a2, int n2,
                              size_t a2_stride, float radius, int32_t* d_out_pairs, size_t out_stride, int* d_n_out,
                              unsigned long long* d_best, int* d_scratch, int n_cu, void* d_prune_ws, int n_frames,
                              MatchPlan plan, const int* d_n1 = nullptr, const int* d_n2 = nullptr);
hipError_t launch_transform_batch(hipStream_t st, const float* d_T16, const float* d_in, int n, size_t stride,
                                  float* d_out, int n_frames);
hipError_t launch_triangulate_batch(hipStream_t st, const float K[9], const Pose* X_host, const float* d_X16,
                                    const int32_t* d_pairs, int n, const int* d_n, const float* d_p1, int n1,
                                    const float* d_p2, int n2, const float* d_app2, float* d_out_xyz,
                                    int32_t* d_out_pairs, float* d_out_app, int* d_n_out, int* d_scratch, int n_frames,
                                    size_t pairs_stride, size_t p1_stride, size_t p2_stride, size_t out_stride);
// sink (or null): the batched solver's arguments -- the writing pass then also gathers every pair it emits into the solver's
// packed arrays (what picp_batch_pack_kernel would do from the pairs it has just written); the caller sets sink->prepacked.
// join_fuses_gather(): whether launch_join_batch will honour a sink at these sizes (the one-launch form of small frames does not).
bool join_fuses_gather(int n_img, int n_world, int n_ref);
hipError_t launch_join_batch(hipStream_t st, const int32_t* d_img, int n_img, const int* d_n_img,
                             const int32_t* d_world, int n_world, const int* d_n_world, int n_ref, int32_t* d_out,
                             int* d_n_out, unsigned long long* d_table, int* d_scratch, int n_frames, size_t img_stride,
                             size_t world_stride, size_t out_stride, const BatchArgs* sink = nullptr);

// in-place exclusive scan of nb ints per frame (one workgroup per frame), total to total[frame] (and total2[frame])
hipError_t launch_scan(hipStream_t st, int* counts, int nb, int* total, int* total2 = nullptr, int n_frames = 1,
                       size_t counts_stride = 0);
// TreeNode_::fullSearch for every query (workspace: match_cells_workspace_bytes(nt, nq, 1))
hipError_t launch_radius_search(hipStream_t st, const float* d_tree, int nt, const float* d_qry, int nq, float radius,
                                int* d_offsets, int32_t* d_indices, int capacity, void* ws);

hipError_t launch_match(hipStream_t st, const float* d_a1, int n1, const float* d_a2, int n2,
                        float radius, int32_t* d_out_pairs, int* d_n_out,
                        unsigned long long* d_best /* min(n1,n2) u64 */, int* d_scratch, int n_cu,
                        void* d_prune_ws, MatchPlan plan);

// ---- the map on the device (map.hip) ------------------------------------------------------------------
struct MapDev {
  float* pts = nullptr;                 // [cap][3]
  float* app = nullptr;                 // [cap][10]
  unsigned long long* table = nullptr;  // [tcap] open addressing, (tag << 32) | entry
  int* last = nullptr;                  // [tcap]
  int* hdr = nullptr;                   // [0] size [1] base of the last update [2] its rows [3] rows dropped for lack of room (never, unless misused)
  unsigned tcap = 0;                    // a power of two, >= 2 * cap
  int cap = 0;
};
size_t map_scratch_ints(int n_max);
// PointCloudVector<3>::update(T * cloud) (PointCloud.h:52-66,77-82); d_T16 / d_n may be null; d_scratch: map_scratch_ints(n_max) ints.
// d_guard (or null): a device flag read when the launches RUN -- where it is 0 they return at once and the map, its table and
// its header keep every byte (voe_map_grow)
hipError_t launch_map_update(hipStream_t st, const MapDev& m, const float* d_xyz, const float* d_app, int n_max, const int* d_n,
                             const float* d_T16, int* d_scratch, const int* d_guard = nullptr);
// empties the table, enters entries 0 .. size-1.  d_guard (or null): a device flag read when the launches RUN -- where it is 0
// the same launches return at once and the table keeps every byte (voe_map_cull: a fixed sequence of launches, whatever the data)
hipError_t launch_map_rehash(hipStream_t st, const MapDev& m, int size_bound, const int* d_guard = nullptr);
hipError_t launch_map_history(hipStream_t st, float* d_hist16, const float* d_X16, int reset);
hipError_t launch_map_transform(hipStream_t st, const MapDev& m, const Pose& T, int size_bound);
// The read-only lookup (vo_map_lookup*): frame f's rows at q_app + f * q_stride floats, d_n[f] (or n_max) of them live.
struct MapLookupArgs {
  const float* app; const float* pts;   // the map's entries
  const unsigned long long* table; const int* hdr; unsigned tmask; int cap;
  const float* q_app; size_t q_stride;  // floats between frames
  int n_max; const int* d_n; int n_frames;
  int nb;                               // workgroups of 256 rows per frame
  int* counts; size_t counts_stride;    // per-workgroup hit counts -> offsets
  int* ent;                             // [n_frames][n_max] entry of every query position, -1: none
  int32_t* pairs;                       // [n_frames][n_max][2] (query index, entry), or null
  int32_t* local_pairs;                 // [n_frames][n_max][2] (query index, k), or null
  float* xyz;                           // [n_frames][n_max][3] point of hit k, or null
};
// d_scratch: map_lookup_scratch_ints(n_max, n_frames, d_entries == null) ints.  3 launches whatever n_frames is.
size_t map_lookup_scratch_ints(int n_max, int n_frames, bool with_entries);
hipError_t launch_map_lookup(hipStream_t st, const MapDev& m, const float* d_app, size_t app_stride_rows, int n_max, const int* d_n,
                             int n_frames, int32_t* d_pairs, int* d_n_out, float* d_xyz, int32_t* d_local_pairs, int32_t* d_entries,
                             int* d_scratch);
// The last launch of vo_map_localise*_dev: status, pose handed out and statistics of every frame.
struct MapLocaliseFinish {
  int n_frames, n_max; const int* d_n;
  const int* n_hits;                    // [n_frames]
  const int* ransac_status;             // [n_frames], or null (no RANSAC ran)
  const int* n_handed;                  // [n_frames] pairs handed to the solver
  const PicpState* state;               // the single solver's state, or null: the batched solver's outputs below
  const float* T_solved;                // [n_frames][16]
  const float* stats4;                  // [n_frames][4] of vo_picp_solve_batch_dev
  const float* T0;                      // [n_frames][16], or null
  int min_inliers;
  float* T_out;                         // [n_frames][16]
  int* stats;                           // [n_frames][8]: vo_map_localise_stats
};
hipError_t launch_map_localise_finish(hipStream_t st, const MapLocaliseFinish& a);

// ---- a map and a window of frames, as the adjustment kernels see them (map_refine.hip, map_pose_refine.hip, map_bundle.hip,
// map_cull.hip): embedded in their four argument blocks ----
constexpr int MAP_WG = 256;             // threads per workgroup of these kernels = entries per block of the list offsets
constexpr int MAP_ROW = 16;             // lanes per landmark of the landmark kernels: one DPP row
struct MapView {
  float* pts; int* hdr; int cap, bound; // the map; bound >= its size (the launches are sized by it, the kernels read the size itself)
  const float* uv; size_t uv_stride;    // [n_frames] rows of pixels, uv_stride pixels between frames
  int n_max, n_frames;
  const float* T16;                     // [n_frames][16] column-major, p_cam = T p_map: the poses as they come in
  double K[9];                          // column-major
  __device__ __forceinline__ int size() const {
    int M = hdr[0];
    M = M < cap ? M : cap;
    return M < bound ? M : bound;
  }
  // number k of frame f's pose as 12 numbers: R column-major, then t
  __device__ __forceinline__ float pose_at(int f, int k) const { return T16[16 * (size_t)f + (k % 3) + 4 * (k / 3)]; }
  template <class S>
  __device__ __forceinline__ void load_pose(int f, S Rt[12]) const {
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = (S)pose_at(f, k);
  }
  // the observation with the key f * n_max + i: its frame, and its pixel into m
  __device__ __forceinline__ int decode(int key, float2& m) const {
    const int f = key / n_max, i = key - f * n_max;
    m = reinterpret_cast<const float2*>(uv)[(size_t)f * uv_stride + i];
    return f;
  }
};
// workgroups of a 16-lanes-per-landmark kernel: 4 waves per SIMD are resident, i.e. 4 workgroups of 256 threads per CU; that many
// stride over the batches of 16 landmarks (map_refine.hip stages the poses once per resident workgroup)
inline unsigned landmark_grid(int bound, int n_cu) {
  const int n_batches = ((bound > 0 ? bound : 1) + MAP_WG / MAP_ROW - 1) / (MAP_WG / MAP_ROW), cap = 4 * (n_cu > 0 ? n_cu : 256);
  return (unsigned)(n_batches < cap ? n_batches : cap);
}

// ---- structure-only refinement of the map's points (map_refine.hip, vo_map_refine*) ---------------------------------
// The workspace of one call: `bound` >= the map's size (the launches are sized by it, the kernels read the size itself).
struct MapRefineWs {
  int32_t* ent;        // [n_frames][n_max] the lookup's entry per query position
  int32_t* pairs;      // [n_frames][n_max][2] the lookup's pairs; afterwards the two key arrays below live here
  int *tmp, *keys;     // [n_frames * n_max] keys as scattered / every entry's segment in ascending order
  int* n_hits;         // [n_frames] (the lookup's counts)
  int *cnt, *cur;      // [bound] observations per entry -> offset inside its block of 256 entries; scatter cursors = the counts
  int* blk;            // [ceil(bound / 256)] block totals -> block offsets
  int* total;          // [1] observations in all
  int32_t* status;     // [bound] (the caller's d_status_out takes its place when given)
  double* cost;        // [bound][2] cost before / after
  size_t bytes;
  // where entry e's segment of the ordered lists begins
  __device__ __forceinline__ int offset(int e) const { return cnt[e] + blk[e / MAP_WG]; }
};
MapRefineWs map_refine_layout(void* base, int n_frames, int n_max, int bound);
struct MapRefineArgs {
  MapRefineWs w;
  MapView v;
  int n_rounds, min_obs;
  double huber, damping;
  int32_t* status;                      // [size]
  float* xyz_out;                       // [size][3] or null: in place
  void* stats;                          // vo_map_refine_stats
};
// after the lookup has filled w.ent: lists (memset, count, offsets, scan, scatter, order), the refinement, the statistics
hipError_t launch_map_refine(hipStream_t st, const MapRefineArgs& a, int n_cu);

// a double moved between lanes by a DPP control (two 32-bit moves; no LDS traffic)
template <int CTRL>
__device__ __forceinline__ double refine_dpp(double x) {
  const long long b = __double_as_longlong(x);
  int lo = (int)b, hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
// the sum over the 16 lanes of a DPP row, the same bits in every lane: the neighbour in the quad (quad_perm [1,0,3,2]), the
// other pair of the quad (quad_perm [2,3,0,1]), the mirrored half row, the mirrored row.  Every step adds two values that both
// lanes of a pair hold, and a + b = b + a bit for bit.
template <class Op>
__device__ __forceinline__ double refine_row_reduce(double x, Op op) {
  x = op(x, refine_dpp<0xB1>(x));
  x = op(x, refine_dpp<0x4E>(x));
  x = op(x, refine_dpp<0x141>(x));
  return op(x, refine_dpp<0x140>(x));
}
__device__ __forceinline__ double refine_row_sum(double x) { return refine_row_reduce(x, [](double a, double b) { return a + b; }); }
// (fmax and fmin are exact and commutative too)
__device__ __forceinline__ double refine_row_max(double x) { return refine_row_reduce(x, [](double a, double b) { return fmax(a, b); }); }
__device__ __forceinline__ double refine_row_min(double x) { return refine_row_reduce(x, [](double a, double b) { return fmin(a, b); }); }
// whether `flag` is set in any of the 16 lanes of this thread's DPP row (called by whole waves)
__device__ __forceinline__ bool refine_row_any(bool flag) {
  const int shift = (threadIdx.x & 63) & ~(MAP_ROW - 1);     // this row's bits in a ballot of the wave
  return ((__ballot(flag) >> shift) & ((1ull << MAP_ROW) - 1ull)) != 0ull;
}

// The sums of N terms over a frame's workgroup of MAP_WG threads: the DPP tree inside every row of 16 lanes, the 16 row sums
// through LDS (s_row: 16 rows of LD >= N doubles), thread k < N adds term k in row order into s_tot[k]; afterwards every thread
// holds the same bits.  Two barriers: the first publishes s_row, the second publishes s_tot -- and frees s_row for the next call,
// whose own first barrier lies between a thread's reads of s_tot here and anybody's next write to it.  With ANY the second one
// also tells whether `flag` was set in any thread.
template <int N, int LD, bool ANY = false>
__device__ __forceinline__ bool frame_reduce(double (&acc)[N], double (*s_row)[LD], double* s_tot, bool flag = false) {
  static_assert(N <= LD, "a row of s_row holds the N terms");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = refine_row_sum(acc[k]);
  if ((tid & (MAP_ROW - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_row[tid / MAP_ROW][k] = acc[k];
  }
  __syncthreads();
  if (tid < N) {
    double s = s_row[0][tid];
#pragma unroll
    for (int w = 1; w < MAP_WG / MAP_ROW; ++w) s += s_row[w][tid];
    s_tot[tid] = s;
  }
  bool any = false;
  if (ANY) any = __syncthreads_or(flag) != 0;
  else __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = s_tot[k];
  return any;
}

// The census of the two refinements' statistics kernels, by ONE workgroup of NT threads: int32 n_items, n_obs, by_status[6];
// double cost_before, cost_after over the items of status 0.  Thread t takes the items t, t + NT, ... in that order, thread 0 adds
// the NT partial sums in thread order: a fixed order, whatever the scheduling, and no float atomics.  n_obs: *obs_total, or with
// SUM_OBS the sum of obs_each[item].
template <int NT, bool SUM_OBS>
__device__ __forceinline__ void status_census(int n_items, const int32_t* status, const double* cost, const int* obs_each,
                                              const int* obs_total, void* stats) {
  constexpr int NC = SUM_OBS ? 7 : 6;
  __shared__ double s_c0[NT], s_c1[NT];
  __shared__ int s_n[NC];
  if (threadIdx.x < NC) s_n[threadIdx.x] = 0;
  __syncthreads();
  int n[NC] = {};
  double c0 = 0.0, c1 = 0.0;
  for (int j = threadIdx.x; j < n_items; j += NT) {
    const int s = status[j];
#pragma unroll
    for (int k = 0; k < 6; ++k) n[k] += s == k;
    if (SUM_OBS) n[NC - 1] += obs_each[j];
    if (s == 0) { c0 += cost[2 * (size_t)j]; c1 += cost[2 * (size_t)j + 1]; }
  }
  s_c0[threadIdx.x] = c0; s_c1[threadIdx.x] = c1;
#pragma unroll
  for (int k = 0; k < NC; ++k) if (n[k]) atomicAdd(&s_n[k], n[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int t = 0; t < NT; ++t) { t0 += s_c0[t]; t1 += s_c1[t]; }
    int* si = static_cast<int*>(stats);
    si[0] = n_items; si[1] = SUM_OBS ? s_n[NC - 1] : *obs_total;
    for (int k = 0; k < 6; ++k) si[2 + k] = s_n[k];
    double* sd = reinterpret_cast<double*>(si + 8);
    sd[0] = t0; sd[1] = t1;
  }
}

// ---- motion-only refinement of the frames' poses on the same cost (map_pose_refine.hip, vo_map_refine_poses*) --------
struct MapPoseWs {
  int32_t* ent;        // [n_frames][n_max] the lookup's entry per query position (null without the lookup)
  int32_t* pairs;      // [n_frames][n_max][2] the lookup's pairs (not read; null without the lookup)
  int* n_hits;         // [n_frames] (the lookup's counts; not read; null without the lookup)
  int32_t* status;     // [n_frames] (the caller's d_status_out takes its place when given)
  int* n_obs;          // [n_frames]
  double* cost;        // [n_frames][2] cost before / after
  size_t bytes;
};
// with_lookup: room for the lookup's own outputs (ent, pairs, n_hits); without it they are null and the caller brings the entries
MapPoseWs map_pose_layout(void* base, int n_frames, int n_max, bool with_lookup);
struct MapPoseArgs {
  const int32_t* ent;                   // [n_frames][n_max]: -1 or the entry (also -1 behind the live rows)
  int* n_obs; double* cost;             // of the workspace
  MapView v;                            // (v.T16: the poses that come in)
  float* T_out;                         // [n_frames][16] the poses that go out; may be the same array as v.T16
  const uint8_t* fixed;                 // [n_frames] or null
  int n_rounds, min_obs;
  double huber, damping;
  int32_t* status;                      // [n_frames]
  double* H_out;                        // [n_frames][36] or null
  void* stats;                          // vo_map_pose_refine_stats
};
// after the lookup has filled `ent`: one workgroup per frame runs all rounds, then the statistics
hipError_t launch_map_pose_refine(hipStream_t st, const MapPoseArgs& a);

// ---- joint adjustment of poses and points by matrix-free Schur PCG (map_bundle.hip, vox_map_bundle*) ----------------
// The observation lists of the point half alone (memset, count, offsets, scan, scatter, order): what launch_map_refine runs
// before its refinement kernel, for callers that traverse the lists themselves.
hipError_t launch_map_refine_lists(hipStream_t st, const MapRefineWs& w, int n_frames, int n_max, int bound);
// the control block of a call: the driver's (lm_pcg.h; `bad`: a pivot of some V_j or D_f is not > 0; `dead`: NOT_FINITE, BEHIND
// or NOTHING_FREE) and the census
struct alignas(8) MapBundleCtl : LmCtl { int n_free_frames, n_free_points, n_obs; };
static_assert(sizeof(MapBundleCtl) == 88, "the size the workspace has always given it");
struct MapBundleWs {
  double *T, *Tc;                       // [n_frames][12] state / candidate: R column-major, then t
  double *P, *Pc;                       // [bound][3] state / candidate
  double *Vinv, *gj, *tj;               // [bound][6] (damped V_j)^-1, upper triangle; [bound][3] g_j; [bound][3] pass A's t_j
  double *U, *D;                        // [n_frames][21] damped U_f / D_f, upper triangles row by row
  double *r, *x, *z, *p, *q;            // [n_frames][6] the PCG vectors; q = S p
  double *pq, *fcost;                   // [n_frames] p_f . q_f / the frame's cost of the last evaluation
  int *fflag, *n_obs;                   // [n_frames] 1: some camera z not > 0 in the last evaluation / observations
  int32_t *pose_status, *point_status;  // [n_frames], [bound]
  MapBundleCtl* ctl;
  size_t bytes;
};
MapBundleWs map_bundle_layout(void* base, int n_frames, int bound);
struct MapBundleArgs {
  MapRefineWs l;                        // the lookup's entries and the ordered lists (map_refine_layout)
  MapBundleWs w;
  MapView v;
  float* T_out;                         // [n_frames][16] the free frames' poses go back here: the array of v.T16
  const uint8_t* fixed;
  int n_rounds, n_cg, min_obs_pose, min_obs_point;
  double cg_tol, lambda0, huber;
  int32_t *pose_status_out, *point_status_out;        // or null
  void* rounds_out;                     // [n_rounds] vox_map_bundle_round, or null
  void* stats;                          // vox_map_bundle_stats
};
// after the lookup has filled l.ent: the lists, then the fixed sequence of 3 (n_cg + 2) launches per round
hipError_t launch_map_bundle(hipStream_t st, const MapBundleArgs& a, int n_cu);

// ---- culling of landmarks (map_cull.hip, voe_map_cull*; include/vo_map_cull.h holds the rules) ----------------------------
struct MapCullWs {
  int32_t *verdict, *remap;             // [bound] (the caller's arrays take their places when given)
  int* rank;                            // [bound] the keep flag, then the survivor's rank inside its block of 256 entries (-1: dropped)
  int* blk;                             // [ceil(bound / 256)] survivors per block -> block offsets
  float *stage_pts, *stage_app;         // [bound][3], [bound][10] the survivors, compacted, before they are copied back
  int* ctl;                             // [0] size before [1] survivors [2] 1: the map changes (something dropped and no dry run)
  size_t bytes;
};
MapCullWs map_cull_layout(void* base, int bound);
struct MapCullArgs {
  MapRefineWs l;                        // the lookup's entries and the ordered lists (map_refine_layout)
  MapCullWs w;
  MapView v;
  float* app;                           // the map's appearances, compacted with its points
  int min_obs, min_frames, drop_unseen, dry_run;
  double max_mean_sq, max_sq, cos_thr;  // squared thresholds (0: off); cos_thr means something when parallax != 0
  int parallax;
  int32_t *verdict, *remap;             // the caller's or the workspace's
  void* entry_out;                      // [size] voe_map_cull_entry, or null
  void* stats;                          // voe_map_cull_stats
};
// after the lookup has filled l.ent: the lists, score, count, scan, scatter into the staging area, copy back, header; the caller
// then enqueues launch_map_rehash guarded by w.ctl + 2, and launch_map_cull_stats
hipError_t launch_map_cull(hipStream_t st, const MapCullArgs& a, int n_cu);
hipError_t launch_map_cull_stats(hipStream_t st, const MapCullArgs& a);
// the compaction alone, for a caller that has written the keep flags into w.rank itself (voe_map_fuse*): count, scan, scatter into
// the staging area, copy back, header.  Reads a.v (pts, hdr, cap, bound), a.w, a.app, a.dry_run; writes a.remap and w.ctl.
__attribute__((visibility("hidden"))) hipError_t launch_map_cull_compact(hipStream_t st, const MapCullArgs& a);

// ---- landmarks added from the frames' unmapped tracks (map_grow.hip, voe_map_grow*; include/vo_map_grow.h holds the rules) ----
// rows = n_frames * n_max query positions (R below: rows, at least 1); a track is numbered below R
struct MapGrowWs {
  int32_t* hit;                         // [R] the map's entry per query position (the lookup's own output)
  int* ocode;                           // [R] an open row's rank inside its block of 256 positions; -1 not live, -2 NaN appearance, -3 a hit
  int* oblk;                            // [ceil(R / 256)] open rows per block -> block offsets
  float* oapp;                          // [R][10] the open rows' appearances, compacted in key order: the cloud of the private update
  int32_t* otrack;                      // [R] the track of compacted open row j (the private lookup's own output)
  int32_t *verdict, *entry;             // [R] per track: what the track kernel decided, then the final verdict / the entry or -1
  float* xyz;                           // [R][3] per track: the chosen point (before that: the private update's cloud points, never meant)
  int *rank, *blk;                      // [R] 1: the track would be added -> its rank inside its block of 256 tracks (-1: not); [ceil(R / 256)]
  float *stage_pts, *stage_app;         // [A][3], [A][10] the ADDED tracks in track order, A = min(max_added, R): the cloud of the append
  int *upd, *look;                      // scratch of the private update (map_scratch_ints(R)) and of the private lookup
  MapDev priv;                          // the tracks' own first-occurrence table: an empty map filled by launch_map_update of oapp
  int* ctl;                             // [0] open rows [1] (the private lookup's hits) [2] tracks that qualify [3] added [4] size before
                                        // [5] 1: the map changes (something is added and no dry run)
  size_t bytes;
};
MapGrowWs map_grow_layout(void* base, size_t rows, int stage_rows, unsigned tcap);
struct MapGrowArgs {
  MapRefineWs l;                        // the tracks' ordered lists (map_refine_layout with bound R): l.ent holds the TRACK of every position
  MapGrowWs w;
  MapView v;                            // the frames; v.hdr is the PRIVATE header, so that v.size() is the number of tracks; v.pts unused
  const float* app; size_t app_stride;  // the frames' appearances, floats between frames
  const int* d_n;                       // or null
  const int* map_hdr; int map_cap;      // the map that grows
  double Kinv[9];                       // column-major (invert_k)
  int n_rounds, min_obs, min_frames;
  double huber, damping;
  double max_mean_sq, max_sq, cos_thr;  // as in MapCullArgs
  int parallax;
  int max_added, dry_run, track_cap;    // max_added: already resolved (never 0)
  int32_t* row_out;                     // [n_frames][n_max] or null
  void* track_out;                      // [track_cap] voe_map_grow_track, or null
  void* stats;                          // voe_map_grow_stats
};
// after the lookup has filled w.hit: open rows -> compaction -> private update and lookup -> lists -> tracks -> ranks -> staging.
// The caller then enqueues launch_map_update of (w.stage_pts, w.stage_app, w.ctl + 3 rows) guarded by w.ctl + 5, and launch_map_grow_finish.
hipError_t launch_map_grow(hipStream_t st, const MapGrowArgs& a, int n_cu);
hipError_t launch_map_grow_finish(hipStream_t st, const MapGrowArgs& a);

// ---- covisibility of frames and the window chosen from it (map_covis.hip, voe_map_covis* / voe_map_window*;
// include/vo_map_covis.h holds the rules).  All integers. ----
struct MapCovisWs {
  int32_t* pairs;                       // [n_frames][n_max][2] the lookup's compacted hits (not read afterwards)
  int32_t* ent;                         // [n_frames][n_max] the lookup's entry per position
  int* n_hits;                          // [n_frames] the lookup's counts
  int* row_pop;                         // [n_frames] entries a frame sees
  int* part;                            // [ceil(n_words / 256)] entries seen by any frame, per block of words
  size_t bytes;
};
MapCovisWs map_covis_layout(void* base, int n_frames, int n_max, int n_words);
struct MapCovisArgs {
  MapCovisWs w;
  const int* hdr; int cap;              // the map's size word and capacity
  int n_frames, n_max, n_words;
  const int* d_n;                       // [n_frames] or null
  uint32_t* bits;                       // [n_frames][n_words]
  int32_t* counts;                      // [n_frames][n_frames] or null
  void* stats;                          // voe_map_covis_stats
};
// after the lookup has filled w.ent and w.n_hits: memset of the bits, bit pass, count pass (when counts are wanted), the rows'
// population counts, the union's, the statistics
hipError_t launch_map_covis(hipStream_t st, const MapCovisArgs& a);
// its first two steps alone, for a caller that wants the bit rows and nothing else (voe_map_loops*): reads w.ent only
hipError_t launch_map_covis_bits(hipStream_t st, const MapCovisArgs& a);
struct MapWindowWs {
  int* cnt;                             // [n_frames] c(g), then s(h)
  int32_t* order;                       // [n_frames] (the caller's array takes its place when given)
  uint32_t* uni;                        // [n_words] (likewise)
  int* part;                            // [ceil(n_words / 256)] population count of the union per block of words
  int* ctl;                             // [0] n_free [1] n_candidates [2] query_seen
  size_t bytes;
};
MapWindowWs map_window_layout(void* base, int n_frames, int n_words);
struct MapWindowArgs {
  MapWindowWs w;
  int n_frames, n_words, n_max;
  const uint32_t* bits;
  const int* d_n;                       // [n_frames] or null
  int query, k_free, k_fixed, min_shared;
  int32_t* role; int* n_rows_out; uint8_t* fixed_out;
  int32_t* order;                       // the caller's or the workspace's
  uint32_t* uni;                        // the caller's or the workspace's
  void* stats;                          // voe_map_window_stats
};
hipError_t launch_map_window(hipStream_t st, const MapWindowArgs& a);

// ---- two maps: similarity by 3-point RANSAC and the merge (map_align.hip, voe_map_align* / voe_map_merge*; include/vo_map_align.h
// holds the rules) ----
constexpr int ALIGN_FS = 16;            // floats per model: M = c R column-major [0, 9), t [9, 12), [12] = 1 valid / 0 invalid
constexpr int ALIGN_SUMS = 6;           // doubles per block of the first pass: sum a, sum b
constexpr int ALIGN_MOMS = 10;          // doubles per block of the second pass: sum db da^T (row-major), sum |da|^2
struct MapAlignCtl {                    // written by single threads of the one-workgroup kernels
  float cur[ALIGN_FS];                  // the model whose inliers the next mask pass takes (the winner's, then the refits')
  float win[ALIGN_FS];                  // the winner's minimal model
  float ref[ALIGN_FS];                  // the last valid refit
  float fin[ALIGN_FS];                  // the model handed out
  double scale_cur, scale_win, scale_ref, scale_fin;
  int n, win_h, win_cnt, n_valid;       // matches, the winner (-1: none) and its count, valid hypotheses
  int alive;                            // 1 while the refits go on
  int have_ref;                         // 1 once a refit was valid
  int cnt_cur;                          // inliers of the last mask pass
  int status, kept, n_fin;              // decided: the status, refit_kept, the final count
};
struct MapAlignArgs {
  const float* src_pts;                 // src's points
  float* bxyz;                          // [n_max][3] dst's point of match k (the lookup's gather)
  const int32_t* pairs; const int* d_n; int n_max;      // the lookup's pairs and count
  int n_hyp, with_scale, n_refits, min_inliers; unsigned long long seed; float thr2;
  float4* pa; float2* pb;               // [n_max] (a0, a1, a2, b0), (b1, b2)
  float* hyp; double* hyp_scale;        // [n_hyp][ALIGN_FS], [n_hyp]
  int* counts;                          // [n_hyp] the caller's or the workspace's
  uint8_t* mask_out;                    // [n_max] the caller's, or null
  int* blk;                             // [nb] inliers per block of the last mask pass
  double *sums, *moms, *rms;            // [nb][ALIGN_SUMS], [nb][ALIGN_MOMS], [nb]
  MapAlignCtl* ctl;
  float* S16_out; void* stats;
  int nb;
};
MapAlignArgs map_align_layout(void* ws, int n_max, int n_hyp, size_t* bytes);
// after the lookup has filled pairs, *d_n and bxyz: 2 memsets and 7 + 3 n_refits + 2 (n_refits > 0) launches
hipError_t launch_map_align(hipStream_t st, const MapAlignArgs& a);

struct MapMergeWs {
  int32_t* ent;                         // [n_max] the lookup before the merge: dst entry of src entry i, -1
  int32_t* pairs;                       // [n_max][2] (the lookups' compacted pairs: not handed out)
  int* blk;                             // [nb] misses per block -> offsets
  float *stage_pts, *stage_app;         // [n_max][3], [n_max][10] the misses, compacted
  int* ctl;                             // [0] dst's size before [1] src entries found before [2] misses [3] hits of the remap lookup
  size_t bytes;
};
MapMergeWs map_merge_layout(void* ws, int n_max);
// ctl[0] <- dst's size (before the lookup and the update are enqueued)
hipError_t launch_map_merge_begin(hipStream_t st, const MapMergeWs& w, const int* dst_hdr);
// KEEP_DST, after the lookup has filled w.ent: the misses of src's rows compacted in order into the staging area, their count in ctl[2]
hipError_t launch_map_merge_misses(hipStream_t st, const MapMergeWs& w, const float* src_pts, const float* src_app, const int* src_hdr, int n_max);
hipError_t launch_map_merge_stats(hipStream_t st, const MapMergeWs& w, const int* src_hdr, const int* dst_hdr, int n_max, void* stats);

// ---- epipolar initialisation, device half (epi.hip) ------------------------------------------------------
size_t epi_workspace_bytes();
// maxima of both point sets + the 45 sums of A^T A + the number of rows / of pairs with a bad index, into ws:
// [0,16) four float maxima  [16,32) int info[0] = rows used, info[1] = bad pairs  [32,48) vote counts  [64,424) 45 doubles
hipError_t launch_epi_front(hipStream_t st, const int32_t* d_pairs, int n_max, const int* d_n, const float* d_p1, int n1,
                            const float* d_p2, int n2, void* ws);
hipError_t launch_epi_vote(hipStream_t st, const float K[9], const Pose X[4], const int32_t* d_pairs, int n_max, const int* d_n,
                           const float* d_p1, int n1, const float* d_p2, int n2, void* ws);
// the per-axis maxima of both point sets alone (epi_max_kernel) into out[4], which the caller has zeroed
hipError_t launch_epi_maxima(hipStream_t st, const float* d_p1, int n1, const float* d_p2, int n2, unsigned* out);

// ---- Gauss-Newton refit of the relative pose on the Sampson error (epi_refine.hip) ---------------------------
constexpr int REFINE_ROW = 24;  // doubles per workgroup row: 15 of J^T w J (upper triangle, row-major), 5 of J^T w r, the cost,
                                // then the counts of pairs used / skipped / with a bad index
struct RefineState {            // head of the workspace; written by the step kernel alone
  double R[9];                  // row-major
  double th[3];                 // translation direction
  double tn;                    // |t| of the input
  double cost0, cost1;          // cost at the input pose / of the pose handed out
  int status, rounds, used0, skipped0, bad0, pad;
  float X_in[16];               // the input's bits, handed back when the refit is not accepted
};
struct RefineArgs {
  const int32_t* pairs; int n_max; const int* d_n;
  const uint8_t* mask;          // per position, or null
  const float* p1; int n1;
  const float* p2; int n2;
  double Kinv[9];               // K^-1 in double, ROW-major
  float X_in[16];               // column-major; read when d_X_in is null
  const float* d_X_in;
  int n_rounds; double huber;   // 0: no Huber weight
  RefineState* st; double* partials; int grid;      // set by launch_epi_refine
  float* X_out; void* stats;    // 16 floats; vo_epi_refine_stats
};
size_t epi_refine_workspace_bytes(int n_max);
// 2 (n_rounds + 1) launches, no memset, no read-back
hipError_t launch_epi_refine(hipStream_t st, RefineArgs a, void* ws);

// ---- RANSAC in front of the epipolar initialisation (ransac.hip) --------------------------------------------
struct RansacArgs {
  const int32_t* pairs; int n_max; const int* d_n;
  const float* p1; int n1;
  const float* p2; int n2;
  int n_hyp; unsigned long long seed; float thr2;
  int* info;                  // [0] live pairs  [1] pairs with a bad index  [2] winner (-1: none)  [3] its count  [4] inliers compacted
  unsigned* maxima;           // [4] per-axis maxima of p1, p2 (float bits)
  float4* pts;                // [n_max] (u1, v1, u2, v2) of the live pairs
  float* F;                   // [n_hyp][12]: F row-major, [9] = 1 valid / 0 invalid
  int* counts;                // [n_hyp] inliers per hypothesis, -1 invalid
  uint8_t* mask;              // [n_max] the winner's inliers
  int* blk;                   // per-workgroup counts of the compaction
  int32_t* out_pairs;         // [n_max][2] the winner's inlier pairs, in their original order
};
size_t ransac_workspace_bytes(int n_max, int n_hyp);
// the workspace's arrays (ws may be null: only *bytes, the size, means something then); the caller fills in the inputs and may
// point counts / mask elsewhere
RansacArgs ransac_layout(void* ws, int n_max, int n_hyp, size_t* bytes = nullptr);
hipError_t launch_ransac(hipStream_t st, const RansacArgs& a);

// ---- P3P RANSAC in front of the tracking solve (pose_ransac.hip) ------------------------------------------
struct PoseRansacArgs {
  const int32_t* pairs; int n_max; const int* d_n;   // (meas_idx, world_idx)
  const float* world; int n_world;
  const float* meas; int n_meas;
  CamK cam;                   // K (float, column-major), image size and depth range of the projection gates
  double Kinv[9];             // K^-1 in double, column-major
  int n_hyp; unsigned long long seed; float thr2;
  int* info;                  // [0] live pairs  [1] pairs with a bad index  [2] winner (-1: none)  [3] its count  [4] status
  float4* pts;                // [n_max] (world x, y, z, measured u) of the live pairs
  float* pv;                  // [n_max] measured v
  float* poses;               // [n_hyp][16]: R column-major [0, 9), t [9, 12), [12] = 1 valid / 0 invalid
  int* counts;                // [n_hyp] inliers per hypothesis, -1 invalid
  uint8_t* mask;              // [n_max] the pairs handed on: the winner's inliers, or every live pair on a fallback
  int* blk;                   // per-workgroup counts of the compaction
  int32_t* out_pairs;         // [n_max][2] the pairs handed on, in their original order
  int* n_out;                 // their count
  float* T_out;               // [16] column-major: the winner's pose, or the identity on a fallback
  int* status;                // the status code (as info[4]), or null
};
size_t pose_ransac_workspace_bytes(int n_max, int n_hyp);
// the workspace's arrays (ws, *bytes: as ransac_layout); the caller fills in the inputs and the outputs and may point counts /
// mask elsewhere
PoseRansacArgs pose_ransac_layout(void* ws, int n_max, int n_hyp, size_t* bytes = nullptr);
hipError_t launch_pose_ransac(hipStream_t st, const PoseRansacArgs& a);
// the batched form: `a` holds problem 0's arrays and the settings all problems share; problem p's inputs and outputs lie p
// strides (in elements: points, pixels, pairs) further, its workspace arrays p x (n_max | n_hyp | nb) items further
struct PoseRansacBatchArgs {
  PoseRansacArgs a;
  size_t world_stride, meas_stride, pairs_stride;
  int nb;                     // workgroups of 256 pairs per problem = the stride of blk
  int n_problems;
};
size_t pose_ransac_batch_workspace_bytes(int n_problems, int n_max, int n_hyp);
// the workspace's arrays (ws, *bytes: as ransac_layout); the caller fills in the inputs, the strides and the outputs and may
// point counts / mask elsewhere
PoseRansacBatchArgs pose_ransac_batch_layout(void* ws, int n_problems, int n_max, int n_hyp, size_t* bytes = nullptr);
hipError_t launch_pose_ransac_batch(hipStream_t st, const PoseRansacBatchArgs& b);

// ---- the pose graph over similarities (pose_graph.hip, voe_pose_graph*) ------------------------------------------------------
constexpr int POSE_GRAPH_REC = 30;      // doubles of an edge's record: M_A, t_A, c_A, t_E, the seven weights, the seven residuals
// the control block of a call: the driver's (lm_pcg.h; `bad`: a pivot of JACOBI is not > 0; `dead`: NOT_FINITE, NOTHING_FREE or
// NO_EDGES) and the census
struct alignas(8) PoseGraphCtl : LmCtl { int n_free, n_active, n_live; };
static_assert(sizeof(PoseGraphCtl) == 88, "the size the workspace has always given it");
struct PoseGraphWs {
  int *cnt, *cur;                       // [n_frames] incidences per frame -> offset inside its block of 256 frames; scatter cursors = the counts
  double *T, *Tc;                       // [n_frames][12] state / candidate: M column-major, then t
  double* rec;                          // [n_edges][POSE_GRAPH_REC] the edges' records at the state
  double *ecost, *ecost_c, *es2_start;  // [n_edges][2] (s^2, its cost) at the state / of the last evaluation of Tc; [n_edges] s^2 of the start
  double* y;                            // [n_edges][7]
  double *r, *x, *z, *p, *q, *tmp;      // [n_frames][7] the PCG vectors; q = (H + lambda diag H) p; tmp: CHAIN between its two sums
  double *pq, *H, *W;                   // [n_frames] p_f . q_f; [n_frames][28] H_ff, upper triangle row by row; [n_frames][3] CHAIN's W_f
  int *blk, *total;                     // [ceil(n_frames / 256)] block totals -> block offsets; [1] incidences in all
  int *lst_tmp, *keys;                  // [2 n_edges] incidences (2 e + side) as scattered / every frame's segment in ascending order
  int32_t *estatus, *fstat;             // [n_edges] VOE_POSE_GRAPH_EDGE_*; [n_frames] active / held / isolated
  PoseGraphCtl* ctl;
  size_t bytes;
};
PoseGraphWs pose_graph_layout(void* base, int n_frames, int n_edges);
struct PoseGraphArgs {
  PoseGraphWs w;
  int n_frames, n_edges;
  float* S16;                           // [n_frames][16] in and, for the active frames, out
  const int32_t* edges;                 // [n_edges][2]
  const float* Z16;                     // [n_edges][16]
  const float* weights;                 // [n_edges][3] or null
  const uint8_t* fixed;                 // [n_frames] or null
  int n_rounds, n_cg, with_scale, precond;
  double cg_tol, lambda0, huber;
  int32_t* edge_status_out;             // or null
  double* edge_cost_out;                // or null
  void* rounds_out;                     // [n_rounds] voe_pose_graph_round, or null
  void* stats;                          // voe_pose_graph_stats
};
// the lists, the start, then the fixed sequence of 3 (n_cg + 2) launches per round, the rounding and the verdict
hipError_t launch_pose_graph(hipStream_t st, const PoseGraphArgs& a);


// ---- a trajectory's correction carried into the map (pose_graph.hip, voe_map_apply_correction*) ------------------------------
constexpr int MAP_APPLY_NO_KEY = 0x7f7f7f7f;     // what a memset of 0x7f leaves: above every key f * n_max + i (at most 2^30)
struct MapApplyArgs {
  const int32_t* ent;                   // [n_frames][n_max] the lookup's entry per query position, -1: none
  int* key;                             // [bound] the smallest key that sees the entry (set to MAP_APPLY_NO_KEY before the launches)
  float* pts; const int* hdr; int cap, bound;
  int n_frames, n_max;
  const float *S_old, *S_new;           // [n_frames][16] column-major
  int dry_run;
  int32_t* ref_frame_out;               // [size] or null
  int* stats;                           // voe_map_apply_stats, zeroed before the launches
};
// the keys (an integer atomicMin: exact), then the move of every entry and the statistics
hipError_t launch_map_apply_correction(hipStream_t st, const MapApplyArgs& a);

// ---- loop edges found and measured in the map (map_loops.hip, voe_map_loops*; include/vo_map_loops.h holds the rules) --------
constexpr int MAP_LOOPS_MAX_FRAMES = 4096;      // VOE_MAP_COVIS_MAX_FRAMES: a histogram row fits a workgroup's LDS
// the workspace of one call: `bound` >= the map's size, L = max_loops
struct MapLoopsWs {
  int32_t* pairs;                       // [n_frames][n_max][2] the lookup's compacted hits (not read afterwards)
  int32_t* ent;                         // [n_frames][n_max] the lookup's entry per position
  int* n_hits;                          // [n_frames] the lookup's counts
  int* key;                             // [bound] the smallest key per entry (MapApplyArgs::key)
  int32_t* ref;                         // [32 * words(bound)] the reference frame per entry (the caller's array takes its place when given)
  int* apply_stats;                     // [4] what the shared move kernel reports (not handed out)
  uint32_t* bits;                       // [n_frames][words(bound)] sees(f, e)
  int32_t* cand;                        // [n_frames][2] (i, c) of every frame's candidate; i == -1: none
  int32_t* slots;                       // [L][4] (i, j, c, 0); i == -1: EMPTY
  int* ctl;                             // [0] n_candidates [1] n_survivors [2] n_slots
  float* world;                         // [L][n_max][3] the gathered points
  float* uv;                            // [L][n_max][2] frame j's pixels
  int32_t* lpairs;                      // [L][n_max][2] (row, k)
  int* n_pairs;                         // [L]
  int32_t* handed;                      // [L][n_max][2] the RANSAC's inlier pairs
  int *n_handed, *rstat;                // [L]
  float *T_start, *T_solved, *stats4;   // [L][16], [L][16], [L][4]
  size_t bytes;
};
MapLoopsWs map_loops_layout(void* base, int n_frames, int n_max, int bound, int max_loops);
struct MapLoopsArgs {
  MapLoopsWs w;
  const float* pts; const int* hdr; int cap, bound;      // the map: read only
  int n_frames, n_max, n_words;
  const float* uv; size_t uv_stride; const int* d_n;
  const float* S16;                     // [n_frames][16]
  int gap, ref_window, min_shared, separation, max_loops, min_inliers;
  float w_loop[3];
  const int32_t* ref;                   // w.ref or the caller's
  int32_t* hist;                        // [n_frames][n_frames] the caller's, or null: a row lives in its workgroup's LDS
  int32_t* edges; float* Z16; float* weights; void* loops; void* stats;      // the outputs
};
// behind the lookup, the reference frames and the bit rows: histogram + candidate per frame, the choice, the slots' pairs
hipError_t launch_map_loops_find(hipStream_t st, const MapLoopsArgs& a);
// behind the two public calls: status, edge, record and statistics
hipError_t launch_map_loops_finish(hipStream_t st, const MapLoopsArgs& a);

// ---- the nearest entry within a radius and the canonical rows (map_nearest.hip, voe_map_nearest*; vo_hip.h holds the rules) ---
constexpr int NEAREST_NC = 32;                                          // cells per grid component, at most
constexpr int NEAREST_CELLS = NEAREST_NC * NEAREST_NC * NEAREST_NC * NEAREST_NC;
constexpr size_t NEAREST_CLAIM_BYTES = (size_t)256 << 20;               // the claim words of one group of frames (unique)
// the workspace of one call: `cap` the map's capacity (the index is allocated for it: "one eager call, then capture")
struct MapNearestWs {
  void* grid;                           // the grid of this call (NearestGrid, map_nearest.hip): 256 bytes
  int* counts;                          // [NEAREST_CELLS + 1] entries per cell, then the cells' cursors
  int* starts;                          // [NEAREST_CELLS + 1] first record of every cell; [n_cells] = records in all
  int* bsum;                            // [1024] the counts' sums per block of 2048 cells
  uint2* rec;                           // [cap] (filter word, entry), ordered by cell
  int32_t* best;                        // [n_frames][n_max] the best entry, -1: none
  uint32_t* d2;                         // [n_frames][n_max] the bits of its distance
  int32_t* st;                          // [n_frames][n_max] the status so far
  unsigned long long* claim;            // [group][cap] the smallest (distance bits, row) per entry, or null (unique == 0)
  int group;                            // frames per group of claim words
  size_t bytes;
};
__attribute__((visibility("hidden"))) MapNearestWs map_nearest_layout(void* base, int n_frames, int n_max, int cap, bool unique);
struct MapNearestArgs {
  MapNearestWs w;
  const float* app; const int* hdr; int cap, bound;      // the map: read only
  const float* q_app; size_t q_stride;  // floats between frames
  int n_frames, n_max; const int* d_n;
  float radius, ratio; int unique;
  int32_t* entry; int32_t* status; float* dist2; float* app_out; int* stats;      // the outputs (all but entry may be null)
};
// (the two helpers the host path shares with map_nearest.hip stay out of the dynamic symbol table)
// memset of the counts (and of *stats) -> grid -> count -> two scan launches -> place -> search -> per group of frames
// { memset of the claim words, claim, resolve } when unique -> finish
__attribute__((visibility("hidden"))) hipError_t launch_map_nearest(hipStream_t st, const MapNearestArgs& a);
// the pieces voe_map_guided* takes from it unchanged: { memset of the claim words, claim, resolve } for the frames [f0, f0 + gf)
// (a.w.claim holds at least gf * cap words), and the finish (entry, status, distance, canonical rows, the eight counts)
__attribute__((visibility("hidden"))) hipError_t launch_nearest_unique(hipStream_t st, const MapNearestArgs& a, int f0, int gf);
__attribute__((visibility("hidden"))) hipError_t launch_nearest_finish(hipStream_t st, const MapNearestArgs& a);

// ---- the nearest entry among those that project near the row's pixel under a pose prior (map_guided.hip, voe_map_guided*) ------
constexpr int GUIDED_NC = 64;                                           // cells per side of a frame's pixel grid, at most
constexpr int GUIDED_CELLS = GUIDED_NC * GUIDED_NC;
// What one group of frames may occupy: per frame a 12-byte record and an 8-byte claim word per entry of the capacity, and the
// two cell tables.  128 MiB is half the 256 MiB Infinity Cache: the records a group's place kernel writes are what its search
// reads next, and the other half is left to what the search streams beside them (the appearance rows of the survivors, the
// frames' rows and pixels), so that a group's index is read from the cache and not from HBM.
constexpr size_t GUIDED_GROUP_BYTES = (size_t)128 << 20;
struct GuidedRec { float u, v; int32_t e; };                            // an entry in view of one frame: its pixel and its index
struct MapGuidedWs {
  MapNearestWs n;                       // best / d2 / st per row, the claim words and the group (the index fields stay null)
  void* grids;                          // [group] the frames' grids (GuidedGrid, map_guided.hip): 32 bytes each
  int* counts;                          // [group][GUIDED_CELLS + 1] records per cell, then the cells' cursors
  int* starts;                          // [group][GUIDED_CELLS + 1] first record of every cell (relative to the frame's records)
  GuidedRec* rec;                       // [group][cap] ordered by cell
  size_t bytes;
};
__attribute__((visibility("hidden"))) MapGuidedWs map_guided_layout(void* base, int n_frames, int n_max, int cap, bool unique);
struct MapGuidedArgs {
  MapGuidedWs w;
  MapNearestArgs n;                     // the map's appearances, the frames' rows, radius / ratio / unique, the outputs nearest has
  const float* pts;                     // the map's points: read only
  const float* uv; size_t uv_stride;    // floats between frames
  const float* T16;                     // [n_frames][16] the priors
  float K[9];
  float radius_px; int z_near, z_far;
  float* pix2;                          // or null
  unsigned long long* stats64;          // n_in_view, n_gated behind the eight counts, or null
};
// memset of the statistics -> per group of frames { memset of the counts, box, count, starts, place, search, and when unique
// { memset of the claim words, claim, resolve } } -> finish
__attribute__((visibility("hidden"))) hipError_t launch_map_guided(hipStream_t st, const MapGuidedArgs& a);

// ---- duplicate landmarks fused: mutual nearest in space and appearance (map_fuse.hip, voe_map_fuse*; vo_hip.h holds the rules) ----
constexpr int FUSE_NC = 128;                                            // cells per axis of the call's 3-D grid, at most
constexpr int FUSE_CELLS = FUSE_NC * FUSE_NC * FUSE_NC;
constexpr int FUSE_SCAN = 2048;                                         // cells per block of the scan
constexpr int FUSE_SCAN_BLOCKS = (FUSE_CELLS + 1 + FUSE_SCAN - 1) / FUSE_SCAN;
// the words the kernels add into, zeroed with the cell counts: [0..5] by_verdict [6] pairs [7] conflicts [8] rows rewritten
// [10..11] n_gated (64 bits) [12..14] the box's upper corner as order-preserving keys
constexpr int FUSE_ACC = 16;
// the workspace of one call: `cap` the map's capacity (allocated for it: "one eager call, then capture")
struct MapFuseWs {
  void* grid;                           // the grid of this call (FuseGrid, map_fuse.hip): 64 bytes
  unsigned* box_lo;                     // [4] the box's lower corner as order-preserving keys (memset to 0xFF)
  int* acc;                             // [FUSE_ACC], directly in front of counts: one memset clears both
  int* counts;                          // [FUSE_CELLS + 1] records per cell, then the cells' cursors
  int* starts;                          // [FUSE_CELLS + 1] first record of every cell; [n_cells] = records in all
  int* bsum;                            // [FUSE_SCAN_BLOCKS] the counts' sums per block of cells
  float4* rec;                          // [cap] {x, y, z, entry}, ordered by cell: the finite entries
  int32_t* fin;                         // [cap] 1: the entry is finite
  int32_t *partner, *verdict, *remap;   // [cap] (the caller's arrays take their places when given)
  size_t bytes;
};
__attribute__((visibility("hidden"))) MapFuseWs map_fuse_layout(void* base, int cap);
struct MapFuseArgs {
  MapFuseWs w;
  MapRefineWs l;                        // with frames: the lookup's entries and the ordered lists (map_refine_layout)
  float* pts; const float* app; const int* hdr; int cap, bound;      // the map (a survivor's point is written with position == 1)
  int frames;                           // 1: frames are given
  const float* q_app; size_t q_stride;  // floats between frames
  int n_frames, n_max; const int* d_n;
  float radius_xyz, radius; int position, veto, dry_run;
  int32_t *partner, *verdict, *remap;   // the caller's or the workspace's
  float *dist2, *gap2;                  // or null
  float* app_out;                       // or null
  const int* cull_ctl;                  // MapCullWs::ctl of the compaction: [0] size before [1] survivors
  void* stats;                          // voe_map_fuse_stats
};
// memsets -> box -> grid -> count -> two scan launches -> place -> search -> (with frames: the observation lists) -> verdict ->
// rows.  The caller then enqueues launch_map_cull_compact on w.rank = the keep flags the verdict kernel wrote into `rank`,
// launch_map_rehash behind the compaction's flag, and launch_map_fuse_finish (the absorbed entries' remap, the statistics).
__attribute__((visibility("hidden"))) hipError_t launch_map_fuse(hipStream_t st, const MapFuseArgs& a, int* rank);
__attribute__((visibility("hidden"))) hipError_t launch_map_fuse_finish(hipStream_t st, const MapFuseArgs& a);

// ---- keyframes chosen: redundant frames dropped one at a time (map_keyframes.hip, voe_map_keyframes*; vo_hip.h holds the rules;
// the bit-sliced counters and the candidate tests are keyframes_rules.h).  All integers. ----
struct MapKeyframesWs {
  uint32_t* planes;                     // [P][n_words] bit p of the count of live frames that see the 32 entries of a word
  int* seen;                            // [n_frames] population count of the row, 0 for a GONE frame
  int* red;                             // [n_frames] the accumulator of a step: zero between steps
  uint8_t* live;                        // [n_frames] 1: neither GONE nor dropped
  uint8_t* poss;                        // [n_frames] 1: FREE, live, seen >= min_seen, and no share or gap test failed so far
  int32_t* order;                       // [n_frames] (the caller's array takes its place when given)
  int* ctl;                             // [0] done [1] frames dropped [2] the frame the last step dropped, or -1
  size_t bytes;
};
__attribute__((visibility("hidden"))) MapKeyframesWs map_keyframes_layout(void* base, int n_frames, int n_words);
struct MapKeyframesArgs {
  MapKeyframesWs w;
  int n_frames, n_words, n_max, n_planes;
  const uint32_t* bits;
  const int* d_n;                       // [n_frames] or null
  const uint8_t* flags;                 // [n_frames] or null
  int min_observers, share_permille, min_seen, max_gap, max_dropped;
  int32_t* verdict; int* n_rows_out; uint8_t* keep; int32_t* step;
  int32_t* order;                       // the caller's or the workspace's
  int32_t *seen_out, *red_out;
  void* stats;                          // voe_map_keyframes_stats
};
// frames -> planes -> max_dropped x { count over the possible candidates, select } -> count over every live frame -> finish.
// The steps behind the device's done flag return at once.
__attribute__((visibility("hidden"))) hipError_t launch_map_keyframes(hipStream_t st, const MapKeyframesArgs& a);

// ---- single observations pruned, with a guard per landmark and per frame (map_prune.hip, voe_map_prune*; vo_hip.h holds the
// rules, prune_rules.h the integer decisions).  The lookup's entries and the ordered lists live in the refinement's workspace. ----
struct MapPruneWs {
  double* sq_list;                      // [n_frames * n_max] |e|^2 in LIST order, for the lists of more than 16 observations
  int* st_list;                         // [n_frames * n_max] the status so far, in list order, for the same lists
  int* row_st;                          // [n_frames][n_max] the status before rule 8 at every position that is an observation
  int* fpart;                           // [n_frames][nb][4] observations, eligible and soft ones of a workgroup's 256 rows
  int* cpart;                           // [n_frames][nb][16] the census of a finishing workgroup: ten status counts, observations, pruned, frame named
  size_t bytes;
};
__attribute__((visibility("hidden"))) int map_prune_blocks(int n_max);      // nb: workgroups per frame of the two frame kernels
__attribute__((visibility("hidden"))) MapPruneWs map_prune_layout(void* base, int n_frames, int n_max);
struct MapPruneArgs {
  MapRefineWs l;                        // the lookup's entries and the ordered lists (map_refine_layout)
  MapPruneWs w;
  MapView v;
  const float* app; size_t app_stride;  // the frames' appearance rows, app_stride rows between frames
  const int* d_n;                       // [n_frames] or null
  int nb;
  double max_sq, rf2, floor2;           // max_err_px^2 (0: off), rel_factor^2, rel_floor_px^2, each widened before it is squared
  int rel_on, rel_min_obs, unique, share_landmark, share_frame;
  int32_t *entry_out, *status_out;      // [n_frames][n_max]; status_out or null
  double* sq_out;                       // [n_frames][n_max] or null
  float* app_out;                       // laid out like app, or null; may be app itself
  void *landmark_out, *frame_out;       // [size] voe_map_prune_landmark, [n_frames] voe_map_prune_frame, or null
  int* stats;                           // voe_map_prune_stats: sixteen 4-byte words
};
// after the lookup has filled l.ent: a memset of the statistics, the lists, the landmark kernel, the frame counts, the finish, the statistics
__attribute__((visibility("hidden"))) hipError_t launch_map_prune(hipStream_t st, const MapPruneArgs& a, int n_cu);

}  // namespace vo
