// capi_map.hip -- the map's half of the extern "C" boundary (vo_hip.h: vo_map_*; vo_map_adjust.h, vo_map_bundle.h, vo_map_cull.h,
// vo_map_align.h, vo_map_covis.h, vo_map_grow.h, vo_map_loops.h; voe_map_nearest*, voe_map_guided*, voe_map_fuse*, voe_map_keyframes* and voe_map_prune* of vo_hip.h itself) and the pose graph's (vo_pose_graph.h).  Host-side plumbing only, like capi.hip: no kernel lives here.
#include <limits.h>
#include <string.h>

#include "capi_internal.h"
#include "keyframes_rules.h"

using namespace vo;

// ---- the map (PointCloudVector<3>::update + the history chain of vo_complete.cpp:145-147,175-176,183) ---------------------------
struct vo_map {
  vo_ctx* ctx = nullptr;
  unsigned long long ctx_id = 0;
  MapDev d;
  DevBuf scratch;
  float* hist = nullptr;        // [0,16) the history isometry, [16,32) staging of a host isometry (vo_map_update)
  MapBound bd;                  // the host's bound of the size and its transitions (map_checks.h); bd.cap follows d.cap
  DevBuf up_xyz{true}, up_app{true};   // staging of vo_map_update.  keeps_state: the host's rows, between their upload and the update's launches
  DevBuf look_ws;               // vo_map_lookup*: per-workgroup counts, entries per query position
  DevBuf loc_ws;                // vo_map_localise*: what passes from stage to stage (hits, gathered points, winner, pairs handed on)
  vo_picp* solver = nullptr;    // vo_map_localise[_dev]: made by the first call
  DevBuf ref_ws;                // vo_map_refine*: the entries seen, the observation lists, status and cost per entry
  DevBuf pose_ws;               // vo_map_refine_poses*: the entries seen, status, observation count and cost per frame
  DevBuf bundle_ws;             // vox_map_bundle*: the state in double, the blocks and the PCG vectors (the lists live in ref_ws)
  DevBuf cull_ws;               // voe_map_cull*: verdict, remap, ranks, the staging area of the survivors (the lists live in ref_ws)
  DevBuf align_ws;              // voe_map_align* (on dst): gathered pairs, hypotheses, counts, the blocks' sums
  DevBuf merge_ws;              // voe_map_merge* (on dst): the lookup's entries, the staging area of the misses
  DevBuf covis_ws;              // voe_map_covis*: the lookup's pairs, counts and entries, the population counts per frame and per block of words
  DevBuf window_ws;             // voe_map_window*: the counts against the query row and against the union, the order, the union
  DevBuf grow_ws;               // voe_map_grow*: the open rows, the tracks' private table, verdicts, the staging area (the lists live in ref_ws)
  DevBuf loops_ws{true};        // keeps_state: the gathered problems of the last call, handed out by voe_map_loops_problems_dev (loops_last).  voe_map_loops*: the lookup's arrays, keys, reference frames, bit rows, candidates, slots, the gathered problems
  DevBuf nearest_ws;            // voe_map_nearest*: the call's index of the map (grid, start table, records), best / distance / status per row, the claim words
  DevBuf fuse_ws;               // voe_map_fuse*: the call's 3-D grid of the map (cell tables, records), finite flags, partner / verdict / remap (compaction: cull_ws; lists: ref_ws)
  DevBuf guided_ws;             // voe_map_guided*: per frame of a group the grid, the cell tables and the records; best / distance / status per row, the claim words
  DevBuf keyframes_ws;          // voe_map_keyframes*: the bit planes of the counts, seen / red / live / possible per frame, the order, the control words
  DevBuf prune_ws;              // voe_map_prune*: |e|^2 and status in list order, the status per row position, the frames' partial counts and census words (the lists live in ref_ws)
  MapLoopsWs loops_last{};      // ... as the last call laid it out (voe_map_loops_problems_dev); bytes == 0: no call yet
};

constexpr int MAP_MAX_ENTRIES = 1 << 29;      // 2.5 x that many table slots still fit 32 bits
static unsigned map_tcap_for(int cap) {
  unsigned t = 1024;
  while (t < 2u * (unsigned)cap + 2u * ((unsigned)cap >> 2)) t <<= 1;      // at most 40 % full (cap <= MAP_MAX_ENTRIES: t <= 2^31)
  return t;
}

static void map_free_arrays(MapDev& d) {
  if (d.pts) (void)hipFree(d.pts);
  if (d.app) (void)hipFree(d.app);
  if (d.table) (void)hipFree(d.table);
  if (d.last) (void)hipFree(d.last);
  d.pts = d.app = nullptr; d.table = nullptr; d.last = nullptr;
}

static int map_alloc_arrays(MapDev& d, int cap) {      // (the caller tells the map's MapBound: on_arrays)
  d.cap = cap; d.tcap = map_tcap_for(cap);
  VO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d.pts), sizeof(float) * 3 * (size_t)cap));
  VO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d.app), sizeof(float) * 10 * (size_t)cap));
  VO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d.table), sizeof(unsigned long long) * (size_t)d.tcap));
  VO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d.last), sizeof(int) * (size_t)d.tcap));
  return VO_OK;
}

// what bounds the size where the host must not wait (MapBound, map_checks.h), and what sizes the launches of a call on the
// map's own entries enqueued now: inside a capture the capacity, since the graph may append behind the call
static int map_bound(const vo_map* m) { return m->bd.bound(); }
static int map_launch_bound(const vo_map* m) { return m->bd.launch_bound(m->ctx->capturing); }

// room for n more entries: the bound the host keeps (size_ub grows by a cloud's row count per update) is refreshed from
// the device only when it would pass the capacity, and the arrays grow only when the true size would.  A map whose update
// has been captured asks the device every time outside a capture; inside one nobody can ask, and the bound decides as before.
static int map_reserve(vo_map* m, int n) {
  vo_ctx* c = m->ctx;
  if (m->bd.room_known(c->capturing, n)) return VO_OK;
  if (c->capturing) return vo_fail(VO_ERR_NOT_READY, "vo_map: the map would have to grow inside a graph capture (create it with the capacity it will need)");
  int size = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&size, m->d.hdr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  m->bd.on_size_read(size);
  if ((long long)size + n <= m->d.cap) return VO_OK;
  long long want = 2ll * m->d.cap;
  if (want < (long long)size + n) want = (long long)size + n + ((long long)size + n) / 2;
  if ((long long)size + n > MAP_MAX_ENTRIES) return vo_fail(VO_ERR_INVALID_ARG, "vo_map: more than 2^29 entries");
  if (want > MAP_MAX_ENTRIES) want = MAP_MAX_ENTRIES;
  MapDev old = m->d;
  MapDev nd = old;
  nd.pts = nd.app = nullptr; nd.table = nullptr; nd.last = nullptr;
  if (int r = map_alloc_arrays(nd, (int)want)) { map_free_arrays(nd); return r; }
  if (size > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(nd.pts, old.pts, sizeof(float) * 3 * (size_t)size, hipMemcpyDeviceToDevice, c->stream));
    VO_HIP_CHECK(hipMemcpyAsync(nd.app, old.app, sizeof(float) * 10 * (size_t)size, hipMemcpyDeviceToDevice, c->stream));
  }
  VO_HIP_CHECK(launch_map_rehash(c->stream, nd, size));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  map_free_arrays(old);
  m->d = nd;
  m->bd.on_arrays(nd.cap);
  return VO_OK;
}

#define VO_MAP_LIVE(m) \
  do { VO_REQUIRE(m, "null map"); VO_REQUIRE(ctx_alive((m)->ctx, (m)->ctx_id), "the context this map was made on has been destroyed"); } while (0)

int vo_map_create(vo_ctx* c, int capacity, vo_map** out) {
  VO_REQUIRE(c && out, "null argument");
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(capacity >= 0 && capacity <= MAP_MAX_ENTRIES, "bad capacity (at most 2^29 entries)");
  *out = nullptr;
  if (int r = set_device(c)) return r;
  vo_map* m = new vo_map();
  m->ctx = c; m->ctx_id = c->id;
  const int cap = capacity < 1024 ? 1024 : capacity;
  int rc = map_alloc_arrays(m->d, cap);
  m->bd.on_arrays(cap);
  if (rc == VO_OK && hipMalloc(reinterpret_cast<void**>(&m->d.hdr), 64) != hipSuccess) rc = vo_fail(VO_ERR_OUT_OF_MEMORY, "vo_map_create: out of device memory");
  if (rc == VO_OK && hipMalloc(reinterpret_cast<void**>(&m->hist), sizeof(float) * 32) != hipSuccess) rc = vo_fail(VO_ERR_OUT_OF_MEMORY, "vo_map_create: out of device memory");
  if (rc != VO_OK) { (void)hipGetLastError(); map_free_arrays(m->d); if (m->d.hdr) (void)hipFree(m->d.hdr); if (m->hist) (void)hipFree(m->hist); delete m; return rc; }
  *out = m;
  return vo_map_clear(m);
}

int vo_map_destroy(vo_map* m) {
  if (!m) return VO_OK;
  if (ctx_alive(m->ctx, m->ctx_id)) {
    VO_NOT_CAPTURING(m->ctx);
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
  } else {
    (void)hipDeviceSynchronize();
  }
  map_free_arrays(m->d);
  if (m->d.hdr) (void)hipFree(m->d.hdr);
  if (m->hist) (void)hipFree(m->hist);
  m->scratch.release(); m->up_xyz.release(); m->up_app.release(); m->look_ws.release(); m->loc_ws.release(); m->ref_ws.release(); m->pose_ws.release(); m->bundle_ws.release(); m->cull_ws.release(); m->align_ws.release(); m->merge_ws.release(); m->covis_ws.release(); m->window_ws.release(); m->grow_ws.release(); m->loops_ws.release(); m->nearest_ws.release(); m->guided_ws.release(); m->fuse_ws.release(); m->keyframes_ws.release(); m->prune_ws.release();
  if (m->solver) (void)vo_picp_destroy(m->solver);
  delete m;
  return VO_OK;
}

int vo_map_clear(vo_map* m) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(hipMemsetAsync(m->d.hdr, 0, 64, c->stream));
  VO_HIP_CHECK(launch_map_rehash(c->stream, m->d, 0));
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  VO_HIP_CHECK(hipMemcpyAsync(m->hist, I, sizeof(I), hipMemcpyHostToDevice, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  m->bd.on_clear();
  return VO_OK;
}

int vo_map_update_dev(vo_map* m, const float* d_xyz, const float* d_app, int n_max, const int* d_n, const float* d_T16) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(n_max >= 0 && n_max <= MAP_MAX_ENTRIES && (n_max == 0 || (d_xyz && d_app)), "bad cloud");
  VO_REQUIRE(aligned8(d_app), "device appearance rows must be 8-byte aligned");
  if (n_max == 0) return VO_OK;
  vo_ctx* c = m->ctx;
  if (int r = set_device(c)) return r;
  if (int r = map_reserve(m, n_max)) return r;
  VO_HIP_CHECK(m->scratch.ensure(sizeof(int) * map_scratch_ints(n_max), c->stream));
  VO_HIP_CHECK(launch_map_update(c->stream, m->d, d_xyz, d_app, n_max, d_n, d_T16, m->scratch.as<int>()));
  m->bd.on_update(n_max, c->capturing);
  return VO_OK;
}

int vo_map_update(vo_map* m, const float* xyz, const float* app, int n, const float T16[16]) {
  VO_MAP_LIVE(m);
  VO_NOT_CAPTURING(m->ctx);
  VO_REQUIRE(n >= 0 && (n == 0 || (xyz && app)), "bad cloud");
  if (n == 0) return VO_OK;
  vo_ctx* c = m->ctx;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, m->up_xyz, xyz, sizeof(float) * 3 * (size_t)n)) return r;
  if (int r = upload(c, m->up_app, app, sizeof(float) * 10 * (size_t)n)) return r;
  if (T16) VO_HIP_CHECK(hipMemcpyAsync(m->hist + 16, T16, sizeof(float) * 16, hipMemcpyHostToDevice, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));          // the host arrays may go away after the call
  return vo_map_update_dev(m, m->up_xyz.as<float>(), m->up_app.as<float>(), n, nullptr, T16 ? m->hist + 16 : nullptr);
}

int vo_map_history_reset_dev(vo_map* m, const float* d_X16) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(d_X16, "null pose");
  if (int r = set_device(m->ctx)) return r;
  VO_HIP_CHECK(launch_map_history(m->ctx->stream, m->hist, d_X16, 1));
  return VO_OK;
}

int vo_map_history_step_dev(vo_map* m, const float* d_X16) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(d_X16, "null pose");
  if (int r = set_device(m->ctx)) return r;
  VO_HIP_CHECK(launch_map_history(m->ctx->stream, m->hist, d_X16, 0));
  return VO_OK;
}

int vo_map_history_dev_ptr(vo_map* m, const float** d_T16) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(d_T16, "null argument");
  *d_T16 = m->hist;
  return VO_OK;
}

int vo_map_get_history(vo_map* m, float T16[16]) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(T16, "null argument");
  VO_NOT_CAPTURING(m->ctx);
  if (int r = set_device(m->ctx)) return r;
  VO_HIP_CHECK(hipMemcpyAsync(T16, m->hist, sizeof(float) * 16, hipMemcpyDeviceToHost, m->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return VO_OK;
}

int vo_map_size(vo_map* m, int* n) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(n, "null argument");
  VO_NOT_CAPTURING(m->ctx);
  if (int r = set_device(m->ctx)) return r;
  int h[4] = {0, 0, 0, 0};
  VO_HIP_CHECK(hipMemcpyAsync(h, m->d.hdr, sizeof(h), hipMemcpyDeviceToHost, m->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  m->bd.on_size_read(h[0]);
  *n = h[0];
  if (h[3] > 0) return vo_fail(VO_ERR_BAD_INDEX, "vo_map: %d entries were dropped for lack of room", h[3]);
  return VO_OK;
}

int vo_map_read(vo_map* m, float* xyz, float* app, int capacity, int* n_out) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(capacity >= 0 && n_out, "bad arguments");
  int n = 0;
  if (int r = vo_map_size(m, &n)) return r;
  *n_out = n;
  const int k = n < capacity ? n : capacity;
  if (k > 0 && xyz) VO_HIP_CHECK(hipMemcpyAsync(xyz, m->d.pts, sizeof(float) * 3 * (size_t)k, hipMemcpyDeviceToHost, m->ctx->stream));
  if (k > 0 && app) VO_HIP_CHECK(hipMemcpyAsync(app, m->d.app, sizeof(float) * 10 * (size_t)k, hipMemcpyDeviceToHost, m->ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  return VO_OK;
}

int vo_map_transform(vo_map* m, const float T16[16]) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(T16, "null argument");
  if (int r = set_device(m->ctx)) return r;
  VO_HIP_CHECK(launch_map_transform(m->ctx->stream, m->d, pose_from_T16(T16), map_launch_bound(m)));
  return VO_OK;
}

int vo_map_dev_ptrs(vo_map* m, const float** d_xyz, const float** d_app, const int** d_size) {
  VO_MAP_LIVE(m);
  if (d_xyz) *d_xyz = m->d.pts;
  if (d_app) *d_app = m->d.app;
  if (d_size) *d_size = m->d.hdr;
  return VO_OK;
}

// ---- reading the map by appearance: the lookup (map.hip) and the localisation composed of it, the P3P RANSAC and the PICP
// solvers.  The localisation calls go through the PUBLIC entry points of the stages, in the order the header's contract names.
// the lookup's refusals, of the frames' appearances (no pixels, no camera) and of its pair and count arrays; `own_out`: those
// arrays are the caller's own workspace's (the covisibility), there and aligned by construction
static int map_lookup_check(const MapFrames& f, bool own_out, const int32_t* d_pairs = nullptr, const int* d_n_out = nullptr,
                            const int32_t* d_local = nullptr) {
  const char* fn = "vo_map_lookup";
  if (f.n_frames < 1 || f.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, f.n_frames);
  if (f.n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if ((!own_out && (!d_n_out || (f.n_max > 0 && !d_pairs))) || (f.n_max > 0 && !f.d_app)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(f.d_app, d_pairs, d_local)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device appearance rows and pair arrays must be 8-byte aligned", fn);
  if (f.n_frames > 1 && f.app_stride < (size_t)f.n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: app_stride %zu is smaller than n_max %d", fn, f.app_stride, f.n_max);
  if (f.app_stride >= 0x7fffffff / 10 || (long long)f.n_max * f.n_frames > (1ll << 30))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  return VO_OK;
}

static size_t lookup_scratch_bytes(const MapFrames& f, bool gather) { return sizeof(int) * map_lookup_scratch_ints(f.n_max, f.n_frames, gather); }

static int map_lookup(vo_map* m, const MapFrames& f, int32_t* d_pairs, int* d_n_out, float* d_xyz, int32_t* d_local, int32_t* d_entries) {
  VO_MAP_LIVE(m);
  if (int r = map_lookup_check(f, false, d_pairs, d_n_out, d_local)) return r;
  vo_ctx* c = m->ctx;
  const size_t need = lookup_scratch_bytes(f, d_entries == nullptr);
  if (c->capturing && m->look_ws.cap < need)
    return vo_fail(VO_ERR_NOT_READY, "vo_map_lookup: the scratch would have to grow inside a graph capture (make one call with %d frame(s) "
                                  "of n_max %d before capturing)", f.n_frames, f.n_max);
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->look_ws.ensure(need, c->stream));
  VO_HIP_CHECK(launch_map_lookup(c->stream, m->d, f.d_app, f.app_stride, f.n_max, f.d_n, f.n_frames, d_pairs, d_n_out, d_xyz, d_local, d_entries,
                                 m->look_ws.as<int>()));
  return VO_OK;
}

int vo_map_lookup_dev(vo_map* m, const float* d_app, int n_max, const int* d_n, int32_t* d_pairs, int* d_n_out, float* d_xyz,
                      int32_t* d_local, int32_t* d_entries) {
  return map_lookup(m, MapFrames{1, nullptr, nullptr, 0, d_app, (size_t)(n_max > 0 ? n_max : 0), n_max, d_n}, d_pairs, d_n_out, d_xyz, d_local, d_entries);
}

int vo_map_lookup_batch_dev(vo_map* m, int n_frames, const float* d_app, size_t app_stride, int n_max, const int* d_n, int32_t* d_pairs,
                            int* d_n_out, float* d_xyz, int32_t* d_local, int32_t* d_entries) {
  return map_lookup(m, MapFrames{n_frames, nullptr, nullptr, 0, d_app, app_stride, n_max, d_n}, d_pairs, d_n_out, d_xyz, d_local, d_entries);
}

// the lookup of every frame of a window into arrays of the caller's workspace (no points gathered, the entry per row kept)
static int lookup_window(vo_map* m, const MapFrames& f, int32_t* pairs, int* n_hits, int32_t* ent) {
  return f.n_max > 0 ? vo_map_lookup_batch_dev(m, f.n_frames, f.d_app, f.app_stride, f.n_max, f.d_n, pairs, n_hits, nullptr, nullptr, ent) : VO_OK;
}

int vo_map_lookup(vo_map* m, const float* app, int n, int32_t* pairs_out, int* n_out, float* xyz_out, int32_t* entry_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(n >= 0 && n_out && (n == 0 || (app && pairs_out)), "bad arguments");
  *n_out = 0;
  if (n == 0) return VO_OK;
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], app, sizeof(float) * 10 * (size_t)n)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 2 * (size_t)n, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(float) * 3 * (size_t)n, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(int32_t) * (size_t)n + 128, c->stream));
  if (int r = ensure_counts(c)) return r;
  if (int r = vo_map_lookup_dev(m, c->in[0].as<float>(), n, nullptr, c->out[0].as<int32_t>(), c->counts.as<int>(),
                                xyz_out ? c->out[1].as<float>() : nullptr, nullptr, entry_out ? c->out[2].as<int32_t>() : nullptr))
    return r;
  int k = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&k, c->counts.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (k < 0 || k > n) return vo_fail(VO_ERR_HIP, "vo_map_lookup: unexpected count %d", k);
  if (k > 0) VO_HIP_CHECK(hipMemcpyAsync(pairs_out, c->out[0].p, sizeof(int32_t) * 2 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  if (k > 0 && xyz_out) VO_HIP_CHECK(hipMemcpyAsync(xyz_out, c->out[1].p, sizeof(float) * 3 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  if (entry_out) VO_HIP_CHECK(hipMemcpyAsync(entry_out, c->out[2].p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  *n_out = k;
  return VO_OK;
}

static_assert(sizeof(vo_map_localise_stats) == 32, "the finishing kernel writes eight 4-byte words per frame");

// what passes from stage to stage, per frame, in the map's workspace (256-byte aligned blocks)
struct LocaliseWs {
  int32_t *pairs, *local, *handed;   // [F][n_max][2]: (query, entry), (query, k), the pairs handed to the solver
  float* xyz;                        // [F][n_max][3] gathered points
  int *n_hits, *n_handed, *rstat;    // [F]
  float *T_start, *T_solved, *stats4;   // [F][16], [F][16], [F][4]
  size_t bytes;
};
static LocaliseWs localise_layout(void* base, int n_frames, int n_max) {
  LocaliseWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames, N = (size_t)n_max;
  w.pairs = c.take<int32_t>(8 * F * N);
  w.local = c.take<int32_t>(8 * F * N);
  w.handed = c.take<int32_t>(8 * F * N);
  w.xyz = c.take<float>(12 * F * N);
  w.n_hits = c.take<int>(4 * F);
  w.n_handed = c.take<int>(4 * F);
  w.rstat = c.take<int>(4 * F);
  w.T_start = c.take<float>(64 * F);
  w.T_solved = c.take<float>(64 * F);
  w.stats4 = c.take<float>(16 * F);
  w.bytes = c.bytes;
  return w;
}

static int localise_check(const char* fn, const MapFrames& f, const vo_ransac_params* params, int n_iters, int min_inliers, const float* d_T0,
                          const float* d_T16, const vo_map_localise_stats* d_stats) {
  if (!(f.K && f.d_uv && f.d_app && params && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (f.n_max < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_max must be positive", fn);
  if (n_iters < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_iters must be positive", fn);
  if (min_inliers < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative min_inliers", fn);
  if (!aligned8(f.d_uv, f.d_app, d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  if (params->n_hypotheses == 0) {
    if (!d_T0) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_hypotheses == 0 (no RANSAC) needs the prior d_T0", fn);
  } else if (int r = ransac_check_params(params)) {
    return r;
  }
  double Kinv[9];
  if (!invert_k(f.K, Kinv)) return vo_fail(VO_ERR_INVALID_ARG, "%s: K is singular", fn);
  return VO_OK;
}

int vo_map_localise_dev(vo_map* m, int rows, int cols, int z_near, int z_far, const float K[9], const float* d_uv, const float* d_app,
                        int n_max, const int* d_n, const vo_ransac_params* params, float thr, int n_iters, int min_inliers,
                        const float* d_T0, float* d_T16, vo_map_localise_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vo_map_localise_dev";
  if (int r = localise_check(fn, MapFrames{1, K, d_uv, (size_t)n_max, d_app, (size_t)n_max, n_max, d_n}, params, n_iters, min_inliers, d_T0, d_T16, d_stats)) return r;
  vo_ctx* c = m->ctx;
  const size_t need = localise_layout(nullptr, 1, n_max).bytes;
  if (int r = capture_growth_check(c->capturing, fn, {{m->loc_ws.cap, need}, {m->solver ? 1u : 0u, 1}}, "n_max %d", n_max)) return r;      // (the solver is made by the first call)
  if (int r = set_device(c)) return r;
  if (!m->solver) { if (int r = vo_picp_create(c, &m->solver)) return r; }
  VO_HIP_CHECK(m->loc_ws.ensure(need, c->stream));
  const LocaliseWs w = localise_layout(m->loc_ws.p, 1, n_max);
  // 1. the lookup, with the hits' points gathered
  if (int r = vo_map_lookup_dev(m, d_app, n_max, d_n, w.pairs, w.n_hits, w.xyz, w.local, nullptr)) return r;
  // 2. the start pose and the pairs handed on
  const bool ransac = params->n_hypotheses > 0;
  if (ransac) {
    if (int r = vo_estimate_pose_ransac_dev(c, rows, cols, z_near, z_far, K, w.xyz, n_max, d_uv, n_max, w.local, n_max, w.n_hits, params,
                                            w.T_start, w.handed, w.n_handed, nullptr, nullptr, w.rstat))
      return r;
  }
  // 3. the rounds (vo_picp_set_camera / _set_kernel_threshold without the pose upload: the pose comes from device memory)
  vo_picp* s = m->solver;
  picp_set_camera_threshold(s, rows, cols, z_near, z_far, K, thr);
  if (int r = vo_picp_set_points_dev(s, w.xyz, n_max, d_uv, n_max)) return r;
  if (int r = vo_picp_set_pose_dev(s, ransac ? w.T_start : d_T0)) return r;
  if (int r = vo_picp_solve_dev(s, ransac ? w.handed : w.local, n_max, ransac ? w.n_handed : w.n_hits, 0, n_iters)) return r;
  // 4. status, pose, statistics
  MapLocaliseFinish f{};
  f.n_frames = 1; f.n_max = n_max; f.d_n = d_n; f.n_hits = w.n_hits; f.ransac_status = ransac ? w.rstat : nullptr;
  f.n_handed = ransac ? w.n_handed : w.n_hits; f.state = picp_state_dev(s); f.T0 = d_T0; f.min_inliers = min_inliers;
  f.T_out = d_T16; f.stats = reinterpret_cast<int*>(d_stats);
  VO_HIP_CHECK(launch_map_localise_finish(c->stream, f));
  return VO_OK;
}

int vo_map_localise_batch_dev(vo_map* m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9], const float* d_uv,
                              size_t uv_stride, const float* d_app, size_t app_stride, int n_max, const int* d_n,
                              const vo_ransac_params* params, float thr, int n_iters, int min_inliers, const float* d_T0, float* d_T16,
                              vo_map_localise_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vo_map_localise_batch_dev";
  if (int r = localise_check(fn, MapFrames{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n}, params, n_iters, min_inliers, d_T0, d_T16, d_stats)) return r;
  VO_REQUIRE(n_frames >= 1 && n_frames <= 65535, "n_frames outside 1 .. 65535 (the frame is a grid dimension)");
  VO_REQUIRE(uv_stride >= (size_t)n_max && app_stride >= (size_t)n_max, "a stride is smaller than n_max");
  VO_REQUIRE(uv_stride < 0x7fffffff, "stride too large");
  vo_ctx* c = m->ctx;
  const size_t need = localise_layout(nullptr, n_frames, n_max).bytes;
  if (int r = capture_growth_check(c->capturing, fn, {{m->loc_ws.cap, need}}, "%d frames of n_max %d", n_frames, n_max)) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->loc_ws.ensure(need, c->stream));
  const LocaliseWs w = localise_layout(m->loc_ws.p, n_frames, n_max);
  if (int r = vo_map_lookup_batch_dev(m, n_frames, d_app, app_stride, n_max, d_n, w.pairs, w.n_hits, w.xyz, w.local, nullptr)) return r;
  const bool ransac = params->n_hypotheses > 0;
  if (ransac) {
    if (int r = vo_estimate_pose_ransac_batch_dev(c, n_frames, rows, cols, z_near, z_far, K, w.xyz, (size_t)n_max, n_max, d_uv, uv_stride,
                                                  n_max, w.local, (size_t)n_max, w.n_hits, params, w.T_start, w.handed, w.n_handed,
                                                  nullptr, nullptr, w.rstat))
      return r;
  }
  if (int r = vo_picp_solve_batch_dev(c, n_frames, rows, cols, z_near, z_far, K, thr, 0, w.xyz, (size_t)n_max, d_uv, uv_stride,
                                      ransac ? w.handed : w.local, (size_t)n_max, ransac ? w.n_handed : w.n_hits,
                                      ransac ? w.T_start : d_T0, n_iters, w.T_solved, w.stats4))
    return r;
  MapLocaliseFinish f{};
  f.n_frames = n_frames; f.n_max = n_max; f.d_n = d_n; f.n_hits = w.n_hits; f.ransac_status = ransac ? w.rstat : nullptr;
  f.n_handed = ransac ? w.n_handed : w.n_hits; f.state = nullptr; f.T_solved = w.T_solved; f.stats4 = w.stats4; f.T0 = d_T0;
  f.min_inliers = min_inliers; f.T_out = d_T16; f.stats = reinterpret_cast<int*>(d_stats);
  VO_HIP_CHECK(launch_map_localise_finish(c->stream, f));
  return VO_OK;
}

int vo_map_localise(vo_map* m, int rows, int cols, int z_near, int z_far, const float K[9], const float* uv, const float* app, int n,
                    const vo_ransac_params* params, float thr, int n_iters, int min_inliers, const float T0[16], float T_out[16],
                    vo_map_localise_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && uv && app && params && T_out && stats_out, "null argument");
  VO_REQUIRE(n >= 1, "n must be positive");
  if (int r = set_device(c)) return r;
  if (int r = upload(c, c->in[0], uv, sizeof(float) * 2 * (size_t)n)) return r;
  if (int r = upload(c, c->in[1], app, sizeof(float) * 10 * (size_t)n)) return r;
  if (T0)
    if (int r = upload(c, c->in[2], T0, sizeof(float) * 16)) return r;
  VO_HIP_CHECK(c->out[2].ensure(128, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));          // the host arrays may go away after the call
  struct { float T[16]; vo_map_localise_stats s; } h;
  static_assert(sizeof(h) == 96, "pose and statistics come back in one copy");
  char* d_res = c->out[2].as<char>();
  if (int r = vo_map_localise_dev(m, rows, cols, z_near, z_far, K, c->in[0].as<float>(), c->in[1].as<float>(), n, nullptr, params, thr,
                                  n_iters, min_inliers, T0 ? c->in[2].as<float>() : nullptr, reinterpret_cast<float*>(d_res),
                                  reinterpret_cast<vo_map_localise_stats*>(d_res + 64)))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  memcpy(T_out, h.T, sizeof(h.T));
  *stats_out = h.s;
  return VO_OK;
}

// ---- the calls that take a window of frames (MapFrames, map_checks.h): what they share ---------------------------------------
// the workspaces of a window call inside a capture (capture_growth_check): asked before the call's lookup is enqueued
static int window_growth_check(const vo_map* m, const char* fn, const MapFrames& f, std::initializer_list<WsNeed> ws) {
  return capture_growth_check(m->ctx->capturing, fn, ws, "%d frames of n_max %d on this map", f.n_frames, f.n_max);
}

// the map and the frames as the adjustment kernels see them (MapView, vo_internal.h), with the poses that come in
static void fill_map(MapView& v, const vo_map* m) { v.pts = m->d.pts; v.hdr = m->d.hdr; v.cap = m->d.cap; v.bound = map_launch_bound(m); }
static void fill_frames(MapView& v, const MapFrames& f, const float* d_T16) {
  v.uv = f.d_uv; v.uv_stride = f.uv_stride; v.n_max = f.n_max; v.n_frames = f.n_frames; v.T16 = d_T16;
  for (int k = 0; k < 9; ++k) v.K[k] = f.K[k];
}

// The begin step of a host-pointer window call, after the call's own null checks: the refusals of the frames `h` (host arrays,
// n_max rows per frame; K null: a call without pixels, poses and camera), the uploads into the context's staging buffers in[0..4]
// -- pixels, appearances, poses, row counts, the mask --, the map's size where the call wants it (asking also waits: the host
// arrays may go away after the call), and the same frames over the staging buffers in `dev`.
static int upload_window(const char* fn, vo_map* m, const MapFrames& h, const float* T16, const uint8_t* fixed, int* size, MapFrames* dev) {
  vo_ctx* c = m->ctx;
  const bool cam = h.K != nullptr;
  if (h.n_frames < 1 || h.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames outside 1 .. 65535", fn);
  if (h.n_max < 0 || (h.n_max > 0 && !((h.d_uv || !cam) && h.d_app))) return vo_fail(VO_ERR_INVALID_ARG, "%s: bad frames", fn);
  if ((long long)h.n_max * h.n_frames > (1ll << 30)) return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  if (int r = set_device(c)) return r;
  const size_t F = (size_t)h.n_frames, rows = F * (size_t)h.n_max;
  const auto up = [c](bool wanted, DevBuf& b, const void* src, size_t bytes) { return wanted ? upload(c, b, src, bytes) : (int)VO_OK; };
  if (int r = up(cam, c->in[0], h.d_uv, sizeof(float) * 2 * rows)) return r;
  if (int r = up(true, c->in[1], h.d_app, sizeof(float) * 10 * rows)) return r;
  if (int r = up(cam, c->in[2], T16, sizeof(float) * 16 * F)) return r;
  if (int r = up(h.d_n != nullptr, c->in[3], h.d_n, sizeof(int) * F)) return r;
  if (int r = up(fixed != nullptr, c->in[4], fixed, F)) return r;
  if (size)
    if (int r = vo_map_size(m, size)) return r;
  *dev = MapFrames{h.n_frames, h.K, cam ? c->in[0].as<float>() : nullptr, (size_t)h.n_max, c->in[1].as<float>(), (size_t)h.n_max, h.n_max,
                   h.d_n ? c->in[3].as<int>() : nullptr};
  return VO_OK;
}

// ---- the nearest entry within a radius and the canonical rows (map_nearest.hip; include/vo_hip.h, NEAREST) ---------------------
static_assert(sizeof(voe_map_nearest_params) == 16 && sizeof(voe_map_nearest_stats) == 32, "the finishing kernel writes eight 4-byte words");

int voe_map_nearest_batch_dev(vo_map* m, int n_frames, const float* d_app, size_t app_stride, int n_max, const int* d_n,
                              const voe_map_nearest_params* p, int32_t* d_entry_out, int32_t* d_status_out, float* d_dist2_out,
                              float* d_app_out, voe_map_nearest_stats* d_stats) {
  const char* fn = "voe_map_nearest_batch_dev";
  const MapFrames f{n_frames, nullptr, nullptr, 0, d_app, app_stride, n_max, d_n};
  if (int r = map_nearest_check(fn, f, p, MapNearestPtrs{d_entry_out, d_status_out, d_dist2_out, d_app_out, d_stats})) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  // the index is allocated for the capacity (MapBound::alloc_bound) and the launches are sized by the launch bound: inside a
  // capture the capacity, because the graph may append behind the call; the kernels read the size from the device
  MapNearestWs w = map_nearest_layout(nullptr, n_frames, n_max, m->bd.alloc_bound(), p->unique != 0);
  if (int r = capture_growth_check(c->capturing, fn, {{m->nearest_ws.cap, w.bytes}}, "%d frames of n_max %d and unique %d on this map", n_frames, n_max, p->unique))
    return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->nearest_ws.ensure(w.bytes, c->stream));
  MapNearestArgs a{};
  a.w = map_nearest_layout(m->nearest_ws.p, n_frames, n_max, m->bd.alloc_bound(), p->unique != 0);
  a.app = m->d.app; a.hdr = m->d.hdr; a.cap = m->d.cap; a.bound = map_launch_bound(m);
  a.q_app = d_app; a.q_stride = 10 * app_stride; a.n_frames = n_frames; a.n_max = n_max; a.d_n = d_n;
  a.radius = p->radius; a.ratio = p->ratio; a.unique = p->unique;
  a.entry = d_entry_out; a.status = d_status_out; a.dist2 = d_dist2_out; a.app_out = d_app_out; a.stats = reinterpret_cast<int*>(d_stats);
  VO_HIP_CHECK(launch_map_nearest(c->stream, a));
  return VO_OK;
}

int voe_map_nearest_dev(vo_map* m, const float* d_app, int n_max, const int* d_n, const voe_map_nearest_params* p, int32_t* d_entry_out,
                        int32_t* d_status_out, float* d_dist2_out, float* d_app_out, voe_map_nearest_stats* d_stats) {
  return voe_map_nearest_batch_dev(m, 1, d_app, (size_t)(n_max > 0 ? n_max : 0), n_max, d_n, p, d_entry_out, d_status_out, d_dist2_out, d_app_out, d_stats);
}

int voe_map_nearest(vo_map* m, int n_frames, const float* app, const int* n_rows, int n_max, const voe_map_nearest_params* p,
                    int32_t* entry_out, int32_t* status_out, float* dist2_out, float* app_out, voe_map_nearest_stats* stats_out) {
  const char* fn = "voe_map_nearest";
  if (!p || !entry_out) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or d_entry_out", fn);
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  MapFrames f;
  if (int r = upload_window(fn, m, MapFrames{n_frames, nullptr, nullptr, 0, app, 0, n_max, n_rows}, nullptr, nullptr, nullptr, &f)) return r;
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));            // the host arrays may go away after the call
  const size_t rows = (size_t)n_frames * (size_t)n_max, d2_bytes = (sizeof(float) * rows + 7) & ~(size_t)7;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * rows + 8, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * rows + 8, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(d2_bytes + sizeof(voe_map_nearest_stats), c->stream));
  voe_map_nearest_stats* d_stats = reinterpret_cast<voe_map_nearest_stats*>(static_cast<char*>(c->out[2].p) + d2_bytes);
  // the canonical rows are written in place over the staged rows (d_app_out == d_app)
  if (int r = voe_map_nearest_batch_dev(m, n_frames, f.d_app, f.app_stride, n_max, f.d_n, p, c->out[0].as<int32_t>(), c->out[1].as<int32_t>(),
                                        c->out[2].as<float>(), app_out && rows > 0 ? c->in[1].as<float>() : nullptr, d_stats))
    return r;
  if (rows > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(entry_out, c->out[0].p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, c->stream));
    if (status_out) VO_HIP_CHECK(hipMemcpyAsync(status_out, c->out[1].p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, c->stream));
    if (dist2_out) VO_HIP_CHECK(hipMemcpyAsync(dist2_out, c->out[2].p, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
    if (app_out) VO_HIP_CHECK(hipMemcpyAsync(app_out, c->in[1].p, sizeof(float) * 10 * rows, hipMemcpyDeviceToHost, c->stream));
  }
  if (stats_out) VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_stats, sizeof(voe_map_nearest_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- the nearest entry among those that project near the row's pixel under a prior (map_guided.hip; include/vo_hip.h, GUIDED) ----
static_assert(sizeof(voe_map_guided_params) == 32 && sizeof(voe_map_guided_stats) == 48, "the kernels write eight 4-byte words and two 8-byte ones");

int voe_map_guided_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                             size_t app_stride, int n_max, const int* d_n, const float* d_T16, const voe_map_guided_params* p,
                             int32_t* d_entry_out, int32_t* d_status_out, float* d_dist2_out, float* d_pix2_out, float* d_app_out,
                             voe_map_guided_stats* d_stats) {
  const char* fn = "voe_map_guided_batch_dev";
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  if (int r = map_guided_check(fn, f, p, MapGuidedPtrs{d_T16, d_entry_out, d_status_out, d_dist2_out, d_pix2_out, d_app_out, d_stats})) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  // allocated for the capacity, launched for the launch bound, the size read on the device: as voe_map_nearest_batch_dev
  const MapGuidedWs need = map_guided_layout(nullptr, n_frames, n_max, m->bd.alloc_bound(), p->unique != 0);
  if (int r = capture_growth_check(c->capturing, fn, {{m->guided_ws.cap, need.bytes}}, "%d frames of n_max %d and unique %d on this map", n_frames, n_max, p->unique))
    return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->guided_ws.ensure(need.bytes, c->stream));
  MapGuidedArgs a{};
  a.w = map_guided_layout(m->guided_ws.p, n_frames, n_max, m->bd.alloc_bound(), p->unique != 0);
  a.n.w = a.w.n;
  a.n.app = m->d.app; a.n.hdr = m->d.hdr; a.n.cap = m->d.cap; a.n.bound = map_launch_bound(m);
  a.n.q_app = d_app; a.n.q_stride = 10 * app_stride; a.n.n_frames = n_frames; a.n.n_max = n_max; a.n.d_n = d_n;
  a.n.radius = p->radius; a.n.ratio = p->ratio; a.n.unique = p->unique;
  a.n.entry = d_entry_out; a.n.status = d_status_out; a.n.dist2 = d_dist2_out; a.n.app_out = d_app_out; a.n.stats = reinterpret_cast<int*>(d_stats);
  a.pts = m->d.pts; a.uv = d_uv; a.uv_stride = 2 * uv_stride; a.T16 = d_T16;
  for (int k = 0; k < 9; ++k) a.K[k] = K[k];
  a.radius_px = p->radius_px; a.z_near = p->z_near; a.z_far = p->z_far;
  a.pix2 = d_pix2_out; a.stats64 = d_stats ? reinterpret_cast<unsigned long long*>(d_stats) + 4 : nullptr;
  VO_HIP_CHECK(launch_map_guided(c->stream, a));
  return VO_OK;
}

int voe_map_guided_dev(vo_map* m, const float K[9], const float* d_uv, const float* d_app, int n_max, const int* d_n, const float* d_T16,
                       const voe_map_guided_params* p, int32_t* d_entry_out, int32_t* d_status_out, float* d_dist2_out, float* d_pix2_out,
                       float* d_app_out, voe_map_guided_stats* d_stats) {
  const size_t stride = (size_t)(n_max > 0 ? n_max : 0);
  return voe_map_guided_batch_dev(m, 1, K, d_uv, stride, d_app, stride, n_max, d_n, d_T16, p, d_entry_out, d_status_out, d_dist2_out, d_pix2_out, d_app_out, d_stats);
}

int voe_map_guided(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max,
                   const float* T16, const voe_map_guided_params* p, int32_t* entry_out, int32_t* status_out, float* dist2_out,
                   float* pix2_out, float* app_out, voe_map_guided_stats* stats_out) {
  const char* fn = "voe_map_guided";
  if (!p || !entry_out || !T16 || !K) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params, entry_out, T16 or K", fn);
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  MapFrames f;
  if (int r = upload_window(fn, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, nullptr, nullptr, &f)) return r;
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));            // the host arrays may go away after the call
  const size_t rows = (size_t)n_frames * (size_t)n_max, w_bytes = (sizeof(float) * rows + 7) & ~(size_t)7;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * rows + 8, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * rows + 8, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(2 * w_bytes + sizeof(voe_map_guided_stats), c->stream));
  float* d_pix2 = reinterpret_cast<float*>(static_cast<char*>(c->out[2].p) + w_bytes);
  voe_map_guided_stats* d_stats = reinterpret_cast<voe_map_guided_stats*>(static_cast<char*>(c->out[2].p) + 2 * w_bytes);
  // the canonical rows are written in place over the staged rows (d_app_out == d_app)
  if (int r = voe_map_guided_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(), p,
                                       c->out[0].as<int32_t>(), c->out[1].as<int32_t>(), c->out[2].as<float>(), d_pix2,
                                       app_out && rows > 0 ? c->in[1].as<float>() : nullptr, d_stats))
    return r;
  if (rows > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(entry_out, c->out[0].p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, c->stream));
    if (status_out) VO_HIP_CHECK(hipMemcpyAsync(status_out, c->out[1].p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, c->stream));
    if (dist2_out) VO_HIP_CHECK(hipMemcpyAsync(dist2_out, c->out[2].p, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
    if (pix2_out) VO_HIP_CHECK(hipMemcpyAsync(pix2_out, d_pix2, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
    if (app_out) VO_HIP_CHECK(hipMemcpyAsync(app_out, c->in[1].p, sizeof(float) * 10 * rows, hipMemcpyDeviceToHost, c->stream));
  }
  if (stats_out) VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_stats, sizeof(voe_map_guided_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- structure-only refinement: the lookup of every frame, then the launches of map_refine.hip ----------------------------
static_assert(sizeof(vo_map_refine_params) == 16 && sizeof(vo_map_refine_stats) == 48, "the statistics kernel writes eight 4-byte words and two doubles");

// the point half's workspace, sized and laid out, and the lookup of every frame into it
static int refine_prepare(const char* fn, vo_map* m, const MapFrames& f, MapRefineWs* out) {
  vo_ctx* c = m->ctx;
  // (allocated for the capacity, laid out and launched for the bound: MapBound::alloc_bound)
  const size_t need = map_refine_layout(nullptr, f.n_frames, f.n_max, m->bd.alloc_bound()).bytes;
  if (int r = window_growth_check(m, fn, f, {{m->ref_ws.cap, need}, {m->look_ws.cap, f.n_max > 0 ? lookup_scratch_bytes(f, false) : 0}})) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->ref_ws.ensure(need, c->stream));
  MapRefineWs w = map_refine_layout(m->ref_ws.p, f.n_frames, f.n_max, map_launch_bound(m));
  if (int r = lookup_window(m, f, w.pairs, w.n_hits, w.ent)) return r;
  *out = w;
  return VO_OK;
}

// the point half's launches on a prepared workspace
static int refine_run(vo_map* m, const MapRefineWs& w, const MapFrames& f, const float* d_T16, const MapRounds& r, int32_t* d_status_out,
                      float* d_xyz_out, vo_map_refine_stats* d_stats) {
  vo_ctx* c = m->ctx;
  MapRefineArgs a{};
  a.w = w;
  fill_map(a.v, m);
  fill_frames(a.v, f, d_T16);
  a.n_rounds = r.n_rounds; a.min_obs = r.min_obs; a.huber = r.huber_px; a.damping = *r.damping;
  a.status = d_status_out ? d_status_out : w.status;
  a.xyz_out = d_xyz_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_refine(c->stream, a, c->n_cu));
  return VO_OK;
}

int vo_map_refine_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                            size_t app_stride, int n_max, const int* d_n, const float* d_T16, const vo_map_refine_params* params,
                            int32_t* d_status_out, float* d_xyz_out, vo_map_refine_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vo_map_refine_batch_dev";
  if (!(K && params && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  const MapRounds rounds{params->n_rounds, INT_MAX, params->min_obs, 2, params->huber_px, &params->damping};
  if (int r = map_frames_check(fn, f, d_stats, &rounds)) return r;
  MapRefineWs w;
  if (int r = refine_prepare(fn, m, f, &w)) return r;
  return refine_run(m, w, f, d_T16, rounds, d_status_out, d_xyz_out, d_stats);
}

int vo_map_refine(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max,
                  const float* T16, const vo_map_refine_params* params, int32_t* status_out, vo_map_refine_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, nullptr, &size, &f)) return r;
  VO_HIP_CHECK(c->out[2].ensure(sizeof(vo_map_refine_stats) + 16, c->stream));
  if (status_out) VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * (size_t)(size > 0 ? size : 1), c->stream));
  if (int r = vo_map_refine_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(), params,
                                      status_out ? c->out[1].as<int32_t>() : nullptr, nullptr, c->out[2].as<vo_map_refine_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(vo_map_refine_stats), hipMemcpyDeviceToHost, c->stream));
  if (status_out && size > 0) VO_HIP_CHECK(hipMemcpyAsync(status_out, c->out[1].p, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- motion-only refinement and the alternation of the two halves (map_pose_refine.hip) ------------------------------------
static_assert(sizeof(vo_map_pose_refine_params) == 16 && sizeof(vo_map_pose_refine_stats) == 48 && sizeof(vo_map_adjust_params) == 28 &&
              sizeof(vo_map_adjust_stats) == 96, "the statistics kernels write eight 4-byte words and two doubles each");

// the pose half's workspace; with `ent` (the entries of a lookup already made for these frames) no lookup is enqueued
static int pose_prepare(const char* fn, vo_map* m, const MapFrames& f, int32_t* ent, MapPoseWs* out) {
  vo_ctx* c = m->ctx;
  MapPoseWs w = map_pose_layout(nullptr, f.n_frames, f.n_max, !ent);
  if (int r = window_growth_check(m, fn, f, {{m->pose_ws.cap, w.bytes}, {m->look_ws.cap, !ent && f.n_max > 0 ? lookup_scratch_bytes(f, false) : 0}})) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->pose_ws.ensure(w.bytes, c->stream));
  w = map_pose_layout(m->pose_ws.p, f.n_frames, f.n_max, !ent);
  if (ent) w.ent = ent;
  else if (int r = lookup_window(m, f, w.pairs, w.n_hits, w.ent)) return r;
  *out = w;
  return VO_OK;
}

static int pose_run(vo_map* m, const MapPoseWs& w, const MapFrames& f, const float* d_T_in, const uint8_t* d_fixed, const MapRounds& r,
                    float* d_T_out, int32_t* d_status_out, double* d_H_out, vo_map_pose_refine_stats* d_stats) {
  vo_ctx* c = m->ctx;
  MapPoseArgs a{};
  a.ent = w.ent; a.n_obs = w.n_obs; a.cost = w.cost;
  fill_map(a.v, m);
  fill_frames(a.v, f, d_T_in);
  a.T_out = d_T_out; a.fixed = d_fixed;
  a.n_rounds = r.n_rounds; a.min_obs = r.min_obs; a.huber = r.huber_px; a.damping = *r.damping;
  a.status = d_status_out ? d_status_out : w.status;
  a.H_out = d_H_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_pose_refine(c->stream, a));
  return VO_OK;
}

int vo_map_refine_poses_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                                  size_t app_stride, int n_max, const int* d_n, const float* d_T16_in, const uint8_t* d_fixed,
                                  const vo_map_pose_refine_params* params, float* d_T16_out, int32_t* d_status_out, double* d_H_out,
                                  vo_map_pose_refine_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vo_map_refine_poses_batch_dev";
  if (!(K && params && d_T16_in && d_T16_out && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(d_H_out)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  const MapRounds rounds{params->n_rounds, VO_MAP_ADJUST_MAX_ROUNDS, params->min_obs, 3, params->huber_px, &params->damping};
  if (int r = map_frames_check(fn, f, d_stats, &rounds)) return r;
  MapPoseWs w;
  if (int r = pose_prepare(fn, m, f, nullptr, &w)) return r;
  return pose_run(m, w, f, d_T16_in, d_fixed, rounds, d_T16_out, d_status_out, d_H_out, d_stats);
}

int vo_map_adjust_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                            size_t app_stride, int n_max, const int* d_n, float* d_T16, const uint8_t* d_fixed,
                            const vo_map_adjust_params* p, int32_t* d_pose_status_out, int32_t* d_point_status_out,
                            vo_map_adjust_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vo_map_adjust_batch_dev";
  if (!(K && p && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (p->n_sweeps < 1 || p->n_sweeps > VO_MAP_ADJUST_MAX_ROUNDS) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_sweeps outside 1 .. %d", fn, VO_MAP_ADJUST_MAX_ROUNDS);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  const MapRounds pose{p->pose_rounds, VO_MAP_ADJUST_MAX_ROUNDS, p->min_obs_pose, 3, p->huber_px, &p->damping},
                  point{p->point_rounds, VO_MAP_ADJUST_MAX_ROUNDS, p->min_obs_point, 2, p->huber_px, &p->damping};
  if (int r = map_frames_check(fn, f, d_stats, &pose)) return r;
  if (int r = map_rounds_check(fn, point)) return r;
  if (int r = window_growth_check(m, fn, f, {{m->pose_ws.cap, map_pose_layout(nullptr, n_frames, n_max, false).bytes}})) return r;      // (before the point half enqueues its lookup)
  MapRefineWs rw;
  MapPoseWs pw;
  if (int r = refine_prepare(fn, m, f, &rw)) return r;        // the one lookup: both halves read rw.ent
  if (int r = pose_prepare(fn, m, f, rw.ent, &pw)) return r;
  for (int s = 0; s < p->n_sweeps; ++s) {
    if (int r = pose_run(m, pw, f, d_T16, d_fixed, pose, d_T16, d_pose_status_out, nullptr, &d_stats[s].poses)) return r;
    if (int r = refine_run(m, rw, f, d_T16, point, d_point_status_out, nullptr, &d_stats[s].points)) return r;
  }
  return VO_OK;
}

int vo_map_refine_poses(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max,
                        float* T16, const uint8_t* fixed, const vo_map_pose_refine_params* params, int32_t* status_out, double* H_out,
                        vo_map_pose_refine_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  MapFrames f;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, fixed, nullptr, &f)) return r;   // (no size wanted)
  const size_t F = (size_t)n_frames;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(double) * 36 * F, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * F, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(vo_map_pose_refine_stats) + 16, c->stream));
  if (H_out) VO_HIP_CHECK(hipMemcpyAsync(c->out[0].p, H_out, sizeof(double) * 36 * F, hipMemcpyHostToDevice, c->stream));
  if (int r = vo_map_refine_poses_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(),
                                            fixed ? c->in[4].as<uint8_t>() : nullptr, params, c->in[2].as<float>(),
                                            status_out ? c->out[1].as<int32_t>() : nullptr, H_out ? c->out[0].as<double>() : nullptr,
                                            c->out[2].as<vo_map_pose_refine_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(vo_map_pose_refine_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(T16, c->in[2].p, sizeof(float) * 16 * F, hipMemcpyDeviceToHost, c->stream));
  if (status_out) VO_HIP_CHECK(hipMemcpyAsync(status_out, c->out[1].p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, c->stream));
  if (H_out) VO_HIP_CHECK(hipMemcpyAsync(H_out, c->out[0].p, sizeof(double) * 36 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

int vo_map_adjust(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max, float* T16,
                  const uint8_t* fixed, const vo_map_adjust_params* params, int32_t* pose_status_out, int32_t* point_status_out,
                  vo_map_adjust_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  VO_REQUIRE(params->n_sweeps >= 1 && params->n_sweeps <= VO_MAP_ADJUST_MAX_ROUNDS, "n_sweeps outside 1 .. 65536");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, fixed, &size, &f)) return r;
  const size_t F = (size_t)n_frames, S = (size_t)params->n_sweeps;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * F, c->stream));
  if (point_status_out) VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * (size_t)(size > 0 ? size : 1), c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(vo_map_adjust_stats) * S + 16, c->stream));
  if (int r = vo_map_adjust_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(),
                                      fixed ? c->in[4].as<uint8_t>() : nullptr, params, pose_status_out ? c->out[0].as<int32_t>() : nullptr,
                                      point_status_out ? c->out[1].as<int32_t>() : nullptr, c->out[2].as<vo_map_adjust_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(vo_map_adjust_stats) * S, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(T16, c->in[2].p, sizeof(float) * 16 * F, hipMemcpyDeviceToHost, c->stream));
  if (pose_status_out) VO_HIP_CHECK(hipMemcpyAsync(pose_status_out, c->out[0].p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, c->stream));
  if (point_status_out && size > 0)
    VO_HIP_CHECK(hipMemcpyAsync(point_status_out, c->out[1].p, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- joint adjustment by matrix-free Schur PCG (map_bundle.hip; include/vo_map_bundle.h: the vox_ namespace) ---------------
static_assert(sizeof(vox_map_bundle_params) == 28 && sizeof(vox_map_bundle_round) == 40 && sizeof(vox_map_bundle_stats) == 48,
              "the records of include/vo_map_bundle.h as the kernels write them");

int vox_map_bundle_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                             size_t app_stride, int n_max, const int* d_n, float* d_T16, const uint8_t* d_fixed,
                             const vox_map_bundle_params* p, int32_t* d_pose_status_out, int32_t* d_point_status_out,
                             vox_map_bundle_round* d_rounds_out, vox_map_bundle_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "vox_map_bundle_batch_dev";
  if (!(K && p && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(d_rounds_out)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  const MapRounds rounds{p->n_rounds, VOX_MAP_BUNDLE_MAX_STEPS, p->min_obs_pose, 3, p->huber_px, nullptr};
  if (int r = map_frames_check(fn, f, d_stats, &rounds)) return r;
  if (p->min_obs_point < 2) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_obs_point must be at least 2", fn);
  if (p->n_cg < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_cg must be at least 1", fn);
  if (!(p->cg_tol >= 0.f && p->cg_tol <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: cg_tol must be finite and not negative", fn);
  if (!(p->lambda0 >= 0.f && p->lambda0 <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: lambda0 must be finite and not negative", fn);
  if ((long long)p->n_rounds * ((long long)p->n_cg + 2) > VOX_MAP_BUNDLE_MAX_STEPS)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_rounds * (n_cg + 2) above %d (the launches of a call are a fixed sequence)", fn, VOX_MAP_BUNDLE_MAX_STEPS);
  vo_ctx* c = m->ctx;
  const int bound = map_launch_bound(m);
  const size_t need = map_bundle_layout(nullptr, n_frames, m->bd.alloc_bound()).bytes;
  if (int r = window_growth_check(m, fn, f, {{m->bundle_ws.cap, need}})) return r;      // (before the lookup is enqueued)
  MapRefineWs rw;
  if (int r = refine_prepare(fn, m, f, &rw)) return r;        // the one lookup of the call
  VO_HIP_CHECK(m->bundle_ws.ensure(need, c->stream));
  MapBundleArgs a{};
  a.l = rw; a.w = map_bundle_layout(m->bundle_ws.p, n_frames, bound);
  fill_map(a.v, m);
  fill_frames(a.v, f, d_T16);
  a.T_out = d_T16; a.fixed = d_fixed;
  a.n_rounds = p->n_rounds; a.n_cg = p->n_cg; a.min_obs_pose = p->min_obs_pose; a.min_obs_point = p->min_obs_point;
  a.cg_tol = p->cg_tol; a.lambda0 = p->lambda0; a.huber = p->huber_px;
  a.pose_status_out = d_pose_status_out; a.point_status_out = d_point_status_out; a.rounds_out = d_rounds_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_bundle(c->stream, a, c->n_cu));
  return VO_OK;
}

int vox_map_bundle(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max, float* T16,
                   const uint8_t* fixed, const vox_map_bundle_params* params, int32_t* pose_status_out, int32_t* point_status_out,
                   vox_map_bundle_round* rounds_out, vox_map_bundle_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  VO_REQUIRE(params->n_rounds >= 0 && params->n_rounds <= VOX_MAP_BUNDLE_MAX_STEPS, "n_rounds outside 0 .. 65536");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, fixed, &size, &f)) return r;
  const size_t F = (size_t)n_frames, S = (size_t)params->n_rounds;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * F, c->stream));
  if (point_status_out) VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * (size_t)(size > 0 ? size : 1), c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(vox_map_bundle_stats) + sizeof(vox_map_bundle_round) * S + 16, c->stream));
  vox_map_bundle_stats* d_st = c->out[2].as<vox_map_bundle_stats>();
  vox_map_bundle_round* d_rd = reinterpret_cast<vox_map_bundle_round*>(d_st + 1);
  if (int r = vox_map_bundle_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(),
                                       fixed ? c->in[4].as<uint8_t>() : nullptr, params, pose_status_out ? c->out[0].as<int32_t>() : nullptr,
                                       point_status_out ? c->out[1].as<int32_t>() : nullptr, rounds_out && S ? d_rd : nullptr, d_st))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_st, sizeof(vox_map_bundle_stats), hipMemcpyDeviceToHost, c->stream));
  if (rounds_out && S) VO_HIP_CHECK(hipMemcpyAsync(rounds_out, d_rd, sizeof(vox_map_bundle_round) * S, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(T16, c->in[2].p, sizeof(float) * 16 * F, hipMemcpyDeviceToHost, c->stream));
  if (pose_status_out) VO_HIP_CHECK(hipMemcpyAsync(pose_status_out, c->out[0].p, sizeof(int32_t) * F, hipMemcpyDeviceToHost, c->stream));
  if (point_status_out && size > 0)
    VO_HIP_CHECK(hipMemcpyAsync(point_status_out, c->out[1].p, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- culling of landmarks (map_cull.hip; include/vo_map_cull.h: the voe_ namespace) ---------------------------------------
static_assert(sizeof(voe_map_cull_params) == 28 && sizeof(voe_map_cull_entry) == 48 && sizeof(voe_map_cull_stats) == 48,
              "the records of include/vo_map_cull.h as the kernels write them");

static int cull_check_params(const char* fn, const voe_map_cull_params* p) {
  if (p->min_obs < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_obs must be at least 1", fn);
  if (p->min_frames < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_frames must be at least 1", fn);
  if (!(p->max_rms_px >= 0.f && p->max_rms_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_rms_px must be finite and not negative", fn);
  if (!(p->max_err_px >= 0.f && p->max_err_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_err_px must be finite and not negative", fn);
  if (!(p->min_parallax_deg >= 0.f && p->min_parallax_deg < 180.f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_parallax_deg must be in [0, 180)", fn);
  return VO_OK;
}

int voe_map_cull_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                           size_t app_stride, int n_max, const int* d_n, const float* d_T16, const voe_map_cull_params* p,
                           int32_t* d_verdict_out, int32_t* d_remap_out, voe_map_cull_entry* d_entry_out, voe_map_cull_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "voe_map_cull_batch_dev";
  if (!(K && p && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(d_entry_out)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  if (int r = map_frames_check(fn, f, d_stats)) return r;
  if (int r = cull_check_params(fn, p)) return r;
  vo_ctx* c = m->ctx;
  const int bound = map_launch_bound(m);
  const size_t need = map_cull_layout(nullptr, m->bd.alloc_bound()).bytes;
  if (int r = window_growth_check(m, fn, f, {{m->cull_ws.cap, need}})) return r;        // (before the lookup is enqueued)
  MapRefineWs rw;
  if (int r = refine_prepare(fn, m, f, &rw)) return r;        // the one lookup of the call
  VO_HIP_CHECK(m->cull_ws.ensure(need, c->stream));
  MapCullArgs a{};
  a.l = rw; a.w = map_cull_layout(m->cull_ws.p, bound);
  fill_map(a.v, m);
  fill_frames(a.v, f, d_T16);
  a.app = m->d.app;
  a.min_obs = p->min_obs; a.min_frames = p->min_frames; a.drop_unseen = p->drop_unseen != 0; a.dry_run = p->dry_run != 0;
  a.max_mean_sq = (double)p->max_rms_px * (double)p->max_rms_px;
  a.max_sq = (double)p->max_err_px * (double)p->max_err_px;
  a.parallax = p->min_parallax_deg > 0.f;
  a.cos_thr = a.parallax ? cos((double)p->min_parallax_deg * 3.14159265358979323846 / 180.0) : 1.0;
  a.verdict = d_verdict_out ? d_verdict_out : a.w.verdict;
  a.remap = d_remap_out ? d_remap_out : a.w.remap;
  a.entry_out = d_entry_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_cull(c->stream, a, c->n_cu));
  VO_HIP_CHECK(launch_map_rehash(c->stream, m->d, bound, a.w.ctl + 2));
  VO_HIP_CHECK(launch_map_cull_stats(c->stream, a));
  return VO_OK;
}

int voe_map_cull(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max,
                 const float* T16, const voe_map_cull_params* params, int32_t* verdict_out, int32_t* remap_out,
                 voe_map_cull_entry* entry_out, voe_map_cull_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, nullptr, &size, &f)) return r;
  const size_t S = (size_t)(size > 0 ? size : 1);
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 2 * S, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(voe_map_cull_entry) * S, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(voe_map_cull_stats) + 16, c->stream));
  int32_t* d_verdict = c->out[0].as<int32_t>();
  int32_t* d_remap = d_verdict + S;
  if (int r = voe_map_cull_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(), params,
                                     verdict_out ? d_verdict : nullptr, remap_out ? d_remap : nullptr,
                                     entry_out ? c->out[1].as<voe_map_cull_entry>() : nullptr, c->out[2].as<voe_map_cull_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(voe_map_cull_stats), hipMemcpyDeviceToHost, c->stream));
  if (size > 0) {
    if (verdict_out) VO_HIP_CHECK(hipMemcpyAsync(verdict_out, d_verdict, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
    if (remap_out) VO_HIP_CHECK(hipMemcpyAsync(remap_out, d_remap, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
    if (entry_out) VO_HIP_CHECK(hipMemcpyAsync(entry_out, c->out[1].p, sizeof(voe_map_cull_entry) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  }
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  m->bd.on_host_cull(stats_out->n_kept, params->dry_run != 0);
  return VO_OK;
}

// ---- duplicate landmarks fused: mutual nearest in space and appearance (map_fuse.hip; include/vo_hip.h, FUSE) ----------------
static_assert(sizeof(voe_map_fuse_params) == 32 && sizeof(voe_map_fuse_stats) == 56, "the finishing kernel writes twelve 4-byte words and one 8-byte one");

int voe_map_fuse_batch_dev(vo_map* m, int n_frames, const float* d_app, size_t app_stride, int n_max, const int* d_n,
                           const voe_map_fuse_params* p, int32_t* d_partner_out, float* d_dist2_out, float* d_gap2_out,
                           int32_t* d_verdict_out, int32_t* d_remap_out, float* d_app_out, voe_map_fuse_stats* d_stats) {
  const char* fn = "voe_map_fuse_batch_dev";
  const MapFrames f{n_frames, nullptr, nullptr, 0, d_app, app_stride, n_max, d_n};
  if (int r = map_fuse_check(fn, f, p, MapFusePtrs{d_partner_out, d_dist2_out, d_gap2_out, d_verdict_out, d_remap_out, d_app_out, d_stats})) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  const bool frames = map_fuse_has_frames(f);
  // allocated for the capacity, launched for the launch bound, the size read on the device: as voe_map_nearest_batch_dev
  const int bound = map_launch_bound(m);
  const size_t need = map_fuse_layout(nullptr, m->bd.alloc_bound()).bytes, need_cull = map_cull_layout(nullptr, m->bd.alloc_bound()).bytes;
  if (int r = capture_growth_check(c->capturing, fn, {{m->fuse_ws.cap, need}, {m->cull_ws.cap, need_cull}}, "%d frames of n_max %d on this map", n_frames, n_max))
    return r;                                               // (before the lookup is enqueued)
  MapRefineWs rw{};
  if (frames) {
    if (int r = refine_prepare(fn, m, f, &rw)) return r;    // the one lookup of the call: the entry of every row BEFORE the fuse
  } else if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->fuse_ws.ensure(need, c->stream));
  VO_HIP_CHECK(m->cull_ws.ensure(need_cull, c->stream));
  // the compaction is the cull's (launch_map_cull_compact): its workspace, its view of the map, the keep flags in its `rank`
  MapCullArgs k{};
  k.w = map_cull_layout(m->cull_ws.p, bound);
  fill_map(k.v, m);
  k.app = m->d.app; k.dry_run = p->dry_run != 0;
  MapFuseArgs a{};
  a.w = map_fuse_layout(m->fuse_ws.p, m->bd.alloc_bound());
  a.l = rw;
  a.pts = m->d.pts; a.app = m->d.app; a.hdr = m->d.hdr; a.cap = m->d.cap; a.bound = bound;
  a.frames = frames; a.q_app = d_app; a.q_stride = 10 * app_stride; a.n_frames = n_frames; a.n_max = n_max; a.d_n = d_n;
  a.radius_xyz = p->radius_xyz; a.radius = p->radius; a.position = p->position; a.veto = p->veto_shared_frame; a.dry_run = p->dry_run;
  a.partner = d_partner_out ? d_partner_out : a.w.partner;
  a.verdict = d_verdict_out ? d_verdict_out : a.w.verdict;
  a.remap = d_remap_out ? d_remap_out : a.w.remap;
  a.dist2 = d_dist2_out; a.gap2 = d_gap2_out; a.app_out = d_app_out; a.cull_ctl = k.w.ctl; a.stats = d_stats;
  k.verdict = a.verdict; k.remap = a.remap;
  VO_HIP_CHECK(launch_map_fuse(c->stream, a, k.w.rank));
  VO_HIP_CHECK(launch_map_cull_compact(c->stream, k));
  VO_HIP_CHECK(launch_map_rehash(c->stream, m->d, bound, k.w.ctl + 2));
  VO_HIP_CHECK(launch_map_fuse_finish(c->stream, a));
  return VO_OK;
}

int voe_map_fuse(vo_map* m, int n_frames, const float* app, const int* n_rows, int n_max, const voe_map_fuse_params* p, int32_t* partner_out,
                 float* dist2_out, float* gap2_out, int32_t* verdict_out, int32_t* remap_out, float* app_out, voe_map_fuse_stats* stats_out) {
  const char* fn = "voe_map_fuse";
  if (!p || !stats_out) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or stats_out", fn);
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  const bool frames = n_frames != 0 || app || n_rows;
  MapFrames f{0, nullptr, nullptr, 0, nullptr, 0, n_max, nullptr};
  int size = 0;
  if (frames) {
    if (int r = upload_window(fn, m, MapFrames{n_frames, nullptr, nullptr, 0, app, 0, n_max, n_rows}, nullptr, nullptr, &size, &f)) return r;
  } else {
    if (app_out) return vo_fail(VO_ERR_INVALID_ARG, "%s: app_out without frames", fn);
    if (int r = vo_map_size(m, &size)) return r;
  }
  const size_t S = (size_t)(size > 0 ? size : 1), rows = frames ? (size_t)n_frames * (size_t)n_max : 0;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 5 * S, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(voe_map_fuse_stats) + 8, c->stream));
  int32_t* d_partner = c->out[0].as<int32_t>();
  float* d_dist2 = reinterpret_cast<float*>(d_partner + S);
  float* d_gap2 = d_dist2 + S;
  int32_t* d_verdict = d_partner + 3 * S;
  int32_t* d_remap = d_partner + 4 * S;
  // the rows are rewritten in place over the staged rows (d_app_out == d_app)
  if (int r = voe_map_fuse_batch_dev(m, n_frames, f.d_app, f.app_stride, n_max, f.d_n, p, partner_out ? d_partner : nullptr,
                                     dist2_out ? d_dist2 : nullptr, gap2_out ? d_gap2 : nullptr, verdict_out ? d_verdict : nullptr,
                                     remap_out ? d_remap : nullptr, app_out && rows > 0 ? c->in[1].as<float>() : nullptr,
                                     c->out[2].as<voe_map_fuse_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(voe_map_fuse_stats), hipMemcpyDeviceToHost, c->stream));
  if (size > 0) {
    const size_t b = sizeof(int32_t) * (size_t)size;
    if (partner_out) VO_HIP_CHECK(hipMemcpyAsync(partner_out, d_partner, b, hipMemcpyDeviceToHost, c->stream));
    if (dist2_out) VO_HIP_CHECK(hipMemcpyAsync(dist2_out, d_dist2, b, hipMemcpyDeviceToHost, c->stream));
    if (gap2_out) VO_HIP_CHECK(hipMemcpyAsync(gap2_out, d_gap2, b, hipMemcpyDeviceToHost, c->stream));
    if (verdict_out) VO_HIP_CHECK(hipMemcpyAsync(verdict_out, d_verdict, b, hipMemcpyDeviceToHost, c->stream));
    if (remap_out) VO_HIP_CHECK(hipMemcpyAsync(remap_out, d_remap, b, hipMemcpyDeviceToHost, c->stream));
  }
  if (app_out && rows > 0) VO_HIP_CHECK(hipMemcpyAsync(app_out, c->in[1].p, sizeof(float) * 10 * rows, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  m->bd.on_host_cull(stats_out->n_after, p->dry_run != 0);
  return VO_OK;
}

// ---- landmarks added from the frames' unmapped tracks (map_grow.hip; include/vo_map_grow.h) ---------------------------------
static_assert(sizeof(voe_map_grow_params) == 40 && sizeof(voe_map_grow_track) == 80 && sizeof(voe_map_grow_stats) == 96,
              "the records of include/vo_map_grow.h as the kernels write them");

int voe_map_grow_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                           size_t app_stride, int n_max, const int* d_n, const float* d_T16, const voe_map_grow_params* p,
                           int32_t* d_row_out, voe_map_grow_track* d_track_out, int track_cap, voe_map_grow_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "voe_map_grow_batch_dev";
  if (!(K && p && d_T16 && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  const MapRounds rounds{p->n_rounds, INT_MAX, p->min_obs, 2, p->huber_px, &p->damping};
  if (int r = map_frames_check(fn, f, d_stats, &rounds)) return r;
  if (int r = map_grow_check(fn, p, d_track_out, track_cap)) return r;
  vo_ctx* c = m->ctx;
  const size_t rows = (size_t)n_frames * (size_t)n_max;
  if (rows > (size_t)MAP_MAX_ENTRIES) return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^29 rows in one call (every row may be a track of its own)", fn);
  const int R = (int)(rows ? rows : 1);
  const int room = map_grow_room(p, n_frames, n_max), stage = room < R ? room : R;
  const bool dry = p->dry_run != 0;
  const unsigned tcap = map_tcap_for(R);
  // the workspaces: the lists over the TRACKS (bounded by the rows), the call's own, the lookup's and the append's scratch
  const size_t need_l = map_refine_layout(nullptr, n_frames, n_max, R).bytes, need_g = map_grow_layout(nullptr, rows, stage, tcap).bytes;
  if (int r = window_growth_check(m, fn, f, {{m->ref_ws.cap, need_l}, {m->grow_ws.cap, need_g}, {m->look_ws.cap, n_max > 0 ? lookup_scratch_bytes(f, false) : 0},
                                             {m->scratch.cap, sizeof(int) * map_scratch_ints(stage)}})) return r;      // (before anything is enqueued)
  if (int r = set_device(c)) return r;
  if (!dry)
    if (int r = map_reserve(m, room)) return r;               // the map grows here, on the host, or the capture is refused
  VO_HIP_CHECK(m->ref_ws.ensure(need_l, c->stream));
  VO_HIP_CHECK(m->grow_ws.ensure(need_g, c->stream));
  VO_HIP_CHECK(m->scratch.ensure(sizeof(int) * map_scratch_ints(stage), c->stream));
  MapGrowArgs a{};
  a.l = map_refine_layout(m->ref_ws.p, n_frames, n_max, R);
  a.w = map_grow_layout(m->grow_ws.p, rows, stage, tcap);
  if (int r = lookup_window(m, f, a.l.pairs, a.l.n_hits, a.w.hit)) return r;      // the one lookup of the map
  a.v.pts = nullptr; a.v.hdr = a.w.priv.hdr; a.v.cap = R; a.v.bound = R;          // (the tracks, not the map: MapGrowArgs)
  fill_frames(a.v, f, d_T16);
  a.app = d_app; a.app_stride = 10 * app_stride; a.d_n = d_n;
  a.map_hdr = m->d.hdr; a.map_cap = m->d.cap;
  if (!invert_k(K, a.Kinv)) return vo_fail(VO_ERR_INVALID_ARG, "%s: K is singular", fn);      // (never: map_frames_check asked)
  a.n_rounds = p->n_rounds; a.min_obs = p->min_obs; a.min_frames = p->min_frames; a.huber = p->huber_px; a.damping = p->damping;
  a.max_mean_sq = (double)p->max_rms_px * (double)p->max_rms_px;
  a.max_sq = (double)p->max_err_px * (double)p->max_err_px;
  a.parallax = p->min_parallax_deg > 0.f;
  a.cos_thr = a.parallax ? cos((double)p->min_parallax_deg * 3.14159265358979323846 / 180.0) : 1.0;
  a.max_added = room; a.dry_run = dry; a.track_cap = track_cap;
  a.row_out = d_row_out; a.track_out = d_track_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_grow(c->stream, a, c->n_cu));
  // the append: vo_map_update_dev's launches on the staging area, returning at once where nothing is added or under dry_run
  VO_HIP_CHECK(launch_map_update(c->stream, m->d, a.w.stage_pts, a.w.stage_app, stage, a.w.ctl + 3, nullptr, m->scratch.as<int>(), a.w.ctl + 5));
  VO_HIP_CHECK(launch_map_grow_finish(c->stream, a));
  m->bd.on_grow(room, c->capturing, dry);
  return VO_OK;
}

int voe_map_grow(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max,
                 const float* T16, const voe_map_grow_params* params, int32_t* row_out, voe_map_grow_track* track_out, int track_cap,
                 voe_map_grow_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && T16 && params && stats_out, "null argument");
  VO_REQUIRE(track_cap >= 0 && !(track_out && track_cap == 0), "bad track_cap");
  MapFrames f;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, nullptr, nullptr, &f)) return r;
  const size_t rows = (size_t)n_frames * (size_t)n_max;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * (rows ? rows : 1), c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(voe_map_grow_track) * (size_t)(track_cap > 0 ? track_cap : 1), c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(voe_map_grow_stats) + 16, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));              // the host arrays may go away after the call
  if (track_out) VO_HIP_CHECK(hipMemsetAsync(c->out[1].p, 0, sizeof(voe_map_grow_track) * (size_t)track_cap, c->stream));      // (records beyond n_tracks)
  if (int r = voe_map_grow_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(), params,
                                     row_out ? c->out[0].as<int32_t>() : nullptr, track_out ? c->out[1].as<voe_map_grow_track>() : nullptr, track_cap,
                                     c->out[2].as<voe_map_grow_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(voe_map_grow_stats), hipMemcpyDeviceToHost, c->stream));
  if (row_out && rows) VO_HIP_CHECK(hipMemcpyAsync(row_out, c->out[0].p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, c->stream));
  if (track_out) VO_HIP_CHECK(hipMemcpyAsync(track_out, c->out[1].p, sizeof(voe_map_grow_track) * (size_t)track_cap, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  m->bd.on_host_grow(stats_out->n_after, params->dry_run != 0);
  return VO_OK;
}

// ---- two maps: alignment by 3-point similarity RANSAC and the merge (map_align.hip; include/vo_map_align.h) ----------------
static_assert(sizeof(voe_map_align_params) == 32 && sizeof(voe_map_align_stats) == 48 && sizeof(voe_map_merge_stats) == 16,
              "the records of include/vo_map_align.h as the kernels write them");

int voe_map_size_bound(vo_map* m, int* n_max_out) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(n_max_out, "null argument");
  *n_max_out = map_bound(m);
  return VO_OK;
}

static int two_maps_check(const char* fn, const vo_map* dst, const vo_map* src) {
  if (!dst || !src) return vo_fail(VO_ERR_INVALID_ARG, "%s: null map", fn);
  if (dst == src) return vo_fail(VO_ERR_INVALID_ARG, "%s: src and dst are one map", fn);
  if (!ctx_alive(dst->ctx, dst->ctx_id) || !ctx_alive(src->ctx, src->ctx_id))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: the context a map was made on has been destroyed", fn);
  if (dst->ctx != src->ctx) return vo_fail(VO_ERR_INVALID_ARG, "%s: the maps live on different contexts", fn);
  return VO_OK;
}

static int align_check_params(const char* fn, const voe_map_align_params* p) {
  if (!p) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (p->n_hypotheses < 1 || p->n_hypotheses > 65536) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_hypotheses outside 1 .. 65536", fn);
  if (p->n_refits < 0 || p->n_refits > VOE_MAP_ALIGN_MAX_REFITS)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_refits outside 0 .. %d (the launches of a call are a fixed sequence)", fn, VOE_MAP_ALIGN_MAX_REFITS);
  if (p->min_inliers < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_inliers must not be negative", fn);
  if (!(p->threshold > 0.f && p->threshold <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: threshold must be positive and finite", fn);
  return VO_OK;
}

int voe_map_align_dev(vo_map* dst, vo_map* src, const voe_map_align_params* p, float* d_S16_out, int32_t* d_pairs_out, int* d_n_matches,
                      uint8_t* d_inlier_mask, int32_t* d_hypothesis_counts, voe_map_align_stats* d_stats) {
  const char* fn = "voe_map_align_dev";
  if (int r = two_maps_check(fn, dst, src)) return r;
  if (int r = align_check_params(fn, p)) return r;
  if (!(d_S16_out && d_pairs_out && d_n_matches && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(d_pairs_out, d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_pairs_out and d_stats must be 8-byte aligned", fn);
  vo_ctx* c = dst->ctx;
  const int n_max = map_bound(src);
  size_t bytes = 0;
  (void)map_align_layout(nullptr, n_max, p->n_hypotheses, &bytes);
  if (int r = capture_growth_check(c->capturing, fn, {{dst->align_ws.cap, bytes}}, "these maps and %d hypotheses", p->n_hypotheses)) return r;      // (before the lookup is enqueued)
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(dst->align_ws.ensure(bytes, c->stream));
  MapAlignArgs a = map_align_layout(dst->align_ws.p, n_max, p->n_hypotheses, nullptr);
  // the matches: the public lookup, on dst, of src's appearances
  if (int r = vo_map_lookup_dev(dst, src->d.app, n_max, src->d.hdr, d_pairs_out, d_n_matches, a.bxyz, nullptr, nullptr)) return r;
  a.src_pts = src->d.pts; a.pairs = d_pairs_out; a.d_n = d_n_matches;
  a.with_scale = p->with_scale != 0; a.n_refits = p->n_refits; a.min_inliers = p->min_inliers; a.seed = p->seed;
  a.thr2 = p->threshold * p->threshold;
  if (d_hypothesis_counts) a.counts = d_hypothesis_counts;
  a.mask_out = d_inlier_mask;
  a.S16_out = d_S16_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_align(c->stream, a));
  return VO_OK;
}

int voe_map_align(vo_map* dst, vo_map* src, const voe_map_align_params* p, float S16_out[16], int32_t* pairs_out, int* n_matches_out,
                  uint8_t* mask_out, int32_t* counts_out, voe_map_align_stats* stats_out) {
  const char* fn = "voe_map_align";
  if (int r = two_maps_check(fn, dst, src)) return r;
  vo_ctx* c = dst->ctx;
  VO_NOT_CAPTURING(c);
  if (int r = align_check_params(fn, p)) return r;
  VO_REQUIRE(S16_out && stats_out, "null argument");
  if (int r = set_device(c)) return r;
  int size = 0;
  if (int r = vo_map_size(src, &size)) return r;              // (the bound becomes the size, unless an update of src was captured)
  const size_t n = (size_t)(map_bound(src) > 0 ? map_bound(src) : 1), H = (size_t)p->n_hypotheses;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * 2 * n, c->stream));
  VO_HIP_CHECK(c->out[1].ensure(up256(n) + sizeof(int32_t) * H, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(256, c->stream));
  uint8_t* d_mask = c->out[1].as<uint8_t>();
  int32_t* d_counts = reinterpret_cast<int32_t*>(d_mask + up256(n));
  float* d_S = c->out[2].as<float>();
  int* d_nm = reinterpret_cast<int*>(d_S + 16);
  voe_map_align_stats* d_st = reinterpret_cast<voe_map_align_stats*>(d_S + 32);
  if (int r = voe_map_align_dev(dst, src, p, d_S, c->out[0].as<int32_t>(), d_nm, mask_out ? d_mask : nullptr, counts_out ? d_counts : nullptr, d_st))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(S16_out, d_S, sizeof(float) * 16, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_st, sizeof(voe_map_align_stats), hipMemcpyDeviceToHost, c->stream));
  if (size > 0) {
    if (pairs_out) VO_HIP_CHECK(hipMemcpyAsync(pairs_out, c->out[0].p, sizeof(int32_t) * 2 * (size_t)size, hipMemcpyDeviceToHost, c->stream));
    if (mask_out) VO_HIP_CHECK(hipMemcpyAsync(mask_out, d_mask, (size_t)size, hipMemcpyDeviceToHost, c->stream));
  }
  if (counts_out) VO_HIP_CHECK(hipMemcpyAsync(counts_out, d_counts, sizeof(int32_t) * H, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (n_matches_out) *n_matches_out = stats_out->n_matches;
  return VO_OK;
}

int voe_map_merge_dev(vo_map* dst, vo_map* src, const float* d_S16, int policy, int32_t* d_remap_out, voe_map_merge_stats* d_stats) {
  const char* fn = "voe_map_merge_dev";
  if (int r = two_maps_check(fn, dst, src)) return r;
  if (policy != VOE_MAP_MERGE_TAKE_SRC && policy != VOE_MAP_MERGE_KEEP_DST) return vo_fail(VO_ERR_INVALID_ARG, "%s: unknown policy %d", fn, policy);
  if (!d_stats) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  vo_ctx* c = dst->ctx;
  const int n_max = map_bound(src);
  const MapMergeWs lay = map_merge_layout(nullptr, n_max);
  const size_t look = sizeof(int) * map_lookup_scratch_ints(n_max, 1, false), upd = sizeof(int) * map_scratch_ints(n_max);
  if (int r = capture_growth_check(c->capturing, fn, {{dst->merge_ws.cap, lay.bytes}, {dst->look_ws.cap, look}, {dst->scratch.cap, upd}}, "these maps")) return r;      // (before anything is enqueued)
  if (int r = set_device(c)) return r;
  if (int r = map_reserve(dst, n_max)) return r;              // dst grows here, on the host, or the capture is refused
  VO_HIP_CHECK(dst->merge_ws.ensure(lay.bytes, c->stream));
  const MapMergeWs w = map_merge_layout(dst->merge_ws.p, n_max);
  VO_HIP_CHECK(launch_map_merge_begin(c->stream, w, dst->d.hdr));
  // the lookup before the merge: which src entries dst holds already
  if (int r = vo_map_lookup_dev(dst, src->d.app, n_max, src->d.hdr, w.pairs, w.ctl + 1, nullptr, nullptr, w.ent)) return r;
  if (policy == VOE_MAP_MERGE_TAKE_SRC) {
    if (int r = vo_map_update_dev(dst, src->d.pts, src->d.app, n_max, src->d.hdr, d_S16)) return r;
  } else {
    VO_HIP_CHECK(launch_map_merge_misses(c->stream, w, src->d.pts, src->d.app, src->d.hdr, n_max));
    if (int r = vo_map_update_dev(dst, w.stage_pts, w.stage_app, n_max, w.ctl + 2, d_S16)) return r;
  }
  if (d_remap_out)
    if (int r = vo_map_lookup_dev(dst, src->d.app, n_max, src->d.hdr, w.pairs, w.ctl + 3, nullptr, nullptr, d_remap_out)) return r;
  VO_HIP_CHECK(launch_map_merge_stats(c->stream, w, src->d.hdr, dst->d.hdr, n_max, d_stats));
  return VO_OK;
}

int voe_map_merge(vo_map* dst, vo_map* src, const float S16[16], int policy, int32_t* remap_out, voe_map_merge_stats* stats_out) {
  const char* fn = "voe_map_merge";
  if (int r = two_maps_check(fn, dst, src)) return r;
  vo_ctx* c = dst->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(stats_out, "null argument");
  if (int r = set_device(c)) return r;
  int size = 0;
  if (int r = vo_map_size(src, &size)) return r;
  const size_t n = (size_t)(map_bound(src) > 0 ? map_bound(src) : 1);
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * n, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(256, c->stream));
  float* d_S = c->out[2].as<float>();
  voe_map_merge_stats* d_st = reinterpret_cast<voe_map_merge_stats*>(d_S + 16);
  if (S16) {
    VO_HIP_CHECK(hipMemcpyAsync(d_S, S16, sizeof(float) * 16, hipMemcpyHostToDevice, c->stream));
    VO_HIP_CHECK(hipStreamSynchronize(c->stream));            // the host array may go away after the call
  }
  if (int r = voe_map_merge_dev(dst, src, S16 ? d_S : nullptr, policy, remap_out ? c->out[0].as<int32_t>() : nullptr, d_st)) return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_st, sizeof(voe_map_merge_stats), hipMemcpyDeviceToHost, c->stream));
  if (remap_out && size > 0) VO_HIP_CHECK(hipMemcpyAsync(remap_out, c->out[0].p, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  dst->bd.on_host_merge(stats_out->n_dst_after);
  return VO_OK;
}

// ---- covisibility of frames and the window chosen from it (map_covis.hip; include/vo_map_covis.h) --------------------------
static_assert(sizeof(voe_map_covis_stats) == 32 && sizeof(voe_map_window_params) == 16 && sizeof(voe_map_window_stats) == 32,
              "the records of include/vo_map_covis.h as the kernels write them");

// the refusals that need no map come first: they are the same on a machine without a device
// (dev: d_stats is a device pointer, written as 8-byte pieces)
static int covis_check(const char* fn, int n_frames, int n_words, const void* d_bits, const void* d_stats, bool dev) {
  if (n_frames < 1 || n_frames > VOE_MAP_COVIS_MAX_FRAMES)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. %d", fn, n_frames, VOE_MAP_COVIS_MAX_FRAMES);
  if (n_words < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_words must be at least 1", fn);
  if (!d_bits || !d_stats) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (dev && !aligned8(d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_stats must be 8-byte aligned", fn);
  return VO_OK;
}

int voe_map_covis_batch_dev(vo_map* m, int n_frames, const float* d_app, size_t app_stride, int n_max, const int* d_n, int n_words,
                            uint32_t* d_bits_out, int32_t* d_counts_out, voe_map_covis_stats* d_stats) {
  const char* fn = "voe_map_covis_batch_dev";
  if (int r = covis_check(fn, n_frames, n_words, d_bits_out, d_stats, true)) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  const MapFrames f{n_frames, nullptr, nullptr, 0, d_app, app_stride, n_max, d_n};
  if (int r = map_lookup_check(f, true)) return r;            // the lookup's own refusals, before anything is sized
  if ((long long)32 * n_words < (long long)map_bound(m))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: %d words hold fewer bits than the map's size bound %d", fn, n_words, map_bound(m));
  MapCovisWs w = map_covis_layout(nullptr, n_frames, n_max, n_words);
  if (int r = capture_growth_check(c->capturing, fn, {{m->covis_ws.cap, w.bytes}, {m->look_ws.cap, n_max > 0 ? lookup_scratch_bytes(f, false) : 0}},
                                   "%d frames of n_max %d and %d words on this map", n_frames, n_max, n_words))      // (before the lookup is enqueued)
    return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->covis_ws.ensure(w.bytes, c->stream));
  w = map_covis_layout(m->covis_ws.p, n_frames, n_max, n_words);
  if (int r = lookup_window(m, f, w.pairs, w.n_hits, w.ent)) return r;      // the one lookup of the call
  MapCovisArgs a{};
  a.w = w; a.hdr = m->d.hdr; a.cap = m->d.cap;
  a.n_frames = n_frames; a.n_max = n_max; a.n_words = n_words; a.d_n = d_n;
  a.bits = d_bits_out; a.counts = d_counts_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_covis(c->stream, a));
  return VO_OK;
}

int voe_map_covis(vo_map* m, int n_frames, const float* app, const int* n_rows, int n_max, int n_words, uint32_t* bits_out,
                  int32_t* counts_out, voe_map_covis_stats* stats_out) {
  const char* fn = "voe_map_covis";
  if (int r = covis_check(fn, n_frames, n_words, bits_out, stats_out, false)) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  MapFrames f;
  int size = 0;
  if (int r = upload_window(fn, m, MapFrames{n_frames, nullptr, nullptr, 0, app, 0, n_max, n_rows}, nullptr, nullptr, &size, &f)) return r;
  const size_t F = (size_t)n_frames, W = (size_t)n_words;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(uint32_t) * F * W, c->stream));
  if (counts_out) VO_HIP_CHECK(c->out[1].ensure(sizeof(int32_t) * F * F, c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(voe_map_covis_stats) + 16, c->stream));
  if (int r = voe_map_covis_batch_dev(m, n_frames, f.d_app, f.app_stride, n_max, f.d_n, n_words, c->out[0].as<uint32_t>(),
                                      counts_out ? c->out[1].as<int32_t>() : nullptr, c->out[2].as<voe_map_covis_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(bits_out, c->out[0].p, sizeof(uint32_t) * F * W, hipMemcpyDeviceToHost, c->stream));
  if (counts_out) VO_HIP_CHECK(hipMemcpyAsync(counts_out, c->out[1].p, sizeof(int32_t) * F * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(voe_map_covis_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// (have_out: the role, row count and mask arrays are all given)
static int window_check(const char* fn, int n_frames, int n_words, const void* d_bits, int n_max, const voe_map_window_params* p,
                        bool have_out, const void* d_stats, bool dev) {
  if (int r = covis_check(fn, n_frames, n_words, d_bits, d_stats, dev)) return r;
  if (!(p && have_out)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (p->query < 0 || p->query >= n_frames) return vo_fail(VO_ERR_INVALID_ARG, "%s: query %d outside the %d frames", fn, p->query, n_frames);
  if (p->k_free < 1 || p->k_free > n_frames) return vo_fail(VO_ERR_INVALID_ARG, "%s: k_free outside 1 .. n_frames", fn);
  if (p->k_fixed < 0 || p->k_fixed > n_frames) return vo_fail(VO_ERR_INVALID_ARG, "%s: k_fixed outside 0 .. n_frames", fn);
  if (p->min_shared < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_shared must be at least 1", fn);
  return VO_OK;
}

int voe_map_window_dev(vo_map* m, int n_frames, int n_words, const uint32_t* d_bits, const int* d_n, int n_max,
                       const voe_map_window_params* p, int32_t* d_role_out, int* d_n_rows_out, uint8_t* d_fixed_out, int32_t* d_order_out,
                       uint32_t* d_union_out, voe_map_window_stats* d_stats) {
  const char* fn = "voe_map_window_dev";
  if (int r = window_check(fn, n_frames, n_words, d_bits, n_max, p, d_role_out && d_n_rows_out && d_fixed_out, d_stats, true)) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  MapWindowWs w = map_window_layout(nullptr, n_frames, n_words);
  if (int r = capture_growth_check(c->capturing, fn, {{m->window_ws.cap, w.bytes}}, "%d frames and %d words on this map", n_frames, n_words)) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->window_ws.ensure(w.bytes, c->stream));
  MapWindowArgs a{};
  a.w = map_window_layout(m->window_ws.p, n_frames, n_words);
  a.n_frames = n_frames; a.n_words = n_words; a.n_max = n_max; a.bits = d_bits; a.d_n = d_n;
  a.query = p->query; a.k_free = p->k_free; a.k_fixed = p->k_fixed; a.min_shared = p->min_shared;
  a.role = d_role_out; a.n_rows_out = d_n_rows_out; a.fixed_out = d_fixed_out;
  a.order = d_order_out ? d_order_out : a.w.order;
  a.uni = d_union_out ? d_union_out : a.w.uni;
  a.stats = d_stats;
  VO_HIP_CHECK(launch_map_window(c->stream, a));
  return VO_OK;
}

int voe_map_window(vo_map* m, int n_frames, int n_words, const uint32_t* bits, const int* n_rows, int n_max,
                   const voe_map_window_params* p, int32_t* role_out, int* n_rows_out, uint8_t* fixed_out, int32_t* order_out,
                   uint32_t* union_out, voe_map_window_stats* stats_out) {
  const char* fn = "voe_map_window";
  if (int r = window_check(fn, n_frames, n_words, bits, n_max, p, role_out && n_rows_out && fixed_out, stats_out, false)) return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  if (int r = set_device(c)) return r;
  const size_t F = (size_t)n_frames, W = (size_t)n_words;
  if (int r = upload(c, c->in[0], bits, sizeof(uint32_t) * F * W)) return r;
  if (n_rows)
    if (int r = upload(c, c->in[3], n_rows, sizeof(int) * F)) return r;
  // one block of outputs: role, n_rows, order [F] ints each, the union [W], the statistics, the mask [F] bytes
  const size_t o_role = 0, o_rows = up256(4 * F), o_order = o_rows + up256(4 * F), o_union = o_order + up256(4 * F), o_stats = o_union + up256(4 * W),
               o_fixed = o_stats + 256, total = o_fixed + up256(F);
  VO_HIP_CHECK(c->out[0].ensure(total, c->stream));
  char* d = c->out[0].as<char>();
  if (int r = voe_map_window_dev(m, n_frames, n_words, c->in[0].as<uint32_t>(), n_rows ? c->in[3].as<int>() : nullptr, n_max, p,
                                 reinterpret_cast<int32_t*>(d + o_role), reinterpret_cast<int*>(d + o_rows), reinterpret_cast<uint8_t*>(d + o_fixed),
                                 order_out ? reinterpret_cast<int32_t*>(d + o_order) : nullptr,
                                 union_out ? reinterpret_cast<uint32_t*>(d + o_union) : nullptr, reinterpret_cast<voe_map_window_stats*>(d + o_stats)))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(role_out, d + o_role, 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(n_rows_out, d + o_rows, 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(fixed_out, d + o_fixed, F, hipMemcpyDeviceToHost, c->stream));
  if (order_out) VO_HIP_CHECK(hipMemcpyAsync(order_out, d + o_order, 4 * F, hipMemcpyDeviceToHost, c->stream));
  if (union_out) VO_HIP_CHECK(hipMemcpyAsync(union_out, d + o_union, 4 * W, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d + o_stats, sizeof(voe_map_window_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- keyframes chosen from the bit rows (map_keyframes.hip; include/vo_hip.h: KEYFRAMES) --------------------------------------
static_assert(sizeof(voe_map_keyframes_params) == 32 && sizeof(voe_map_keyframes_stats) == 32,
              "the records of include/vo_hip.h (KEYFRAMES) as the kernels write them");

int voe_map_keyframes_dev(vo_map* m, int n_frames, int n_words, const uint32_t* d_bits, const int* d_n, int n_max, const uint8_t* d_flags,
                          const voe_map_keyframes_params* p, int32_t* d_verdict_out, int* d_n_rows_out, uint8_t* d_keep_out, int32_t* d_step_out,
                          int32_t* d_order_out, int32_t* d_seen_out, int32_t* d_red_out, voe_map_keyframes_stats* d_stats) {
  const char* fn = "voe_map_keyframes_dev";
  if (int r = map_keyframes_check(fn, n_frames, n_words, n_max, nullptr, p,
                                  MapKeyframesPtrs{d_bits, d_verdict_out, d_n_rows_out, d_keep_out, d_step_out, d_order_out, d_seen_out, d_red_out, d_stats}, true))
    return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  MapKeyframesWs w = map_keyframes_layout(nullptr, n_frames, n_words);
  if (int r = capture_growth_check(c->capturing, fn, {{m->keyframes_ws.cap, w.bytes}}, "%d frames and %d words on this map", n_frames, n_words)) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->keyframes_ws.ensure(w.bytes, c->stream));
  MapKeyframesArgs a{};
  a.w = map_keyframes_layout(m->keyframes_ws.p, n_frames, n_words);
  a.n_frames = n_frames; a.n_words = n_words; a.n_max = n_max; a.n_planes = keyframes_planes(n_frames);
  a.bits = d_bits; a.d_n = d_n; a.flags = d_flags;
  a.min_observers = p->min_observers; a.share_permille = p->share_permille; a.min_seen = p->min_seen; a.max_gap = p->max_gap; a.max_dropped = p->max_dropped;
  a.verdict = d_verdict_out; a.n_rows_out = d_n_rows_out; a.keep = d_keep_out; a.step = d_step_out;
  a.order = d_order_out ? d_order_out : a.w.order;
  a.seen_out = d_seen_out; a.red_out = d_red_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_keyframes(c->stream, a));
  return VO_OK;
}

int voe_map_keyframes(vo_map* m, int n_frames, int n_words, const uint32_t* bits, const int* n_rows, int n_max, const uint8_t* flags,
                      const voe_map_keyframes_params* p, int32_t* verdict_out, int* n_rows_out, uint8_t* keep_out, int32_t* step_out,
                      int32_t* order_out, int32_t* seen_out, int32_t* red_out, voe_map_keyframes_stats* stats_out) {
  const char* fn = "voe_map_keyframes";
  if (int r = map_keyframes_check(fn, n_frames, n_words, n_max, flags, p,
                                  MapKeyframesPtrs{bits, verdict_out, n_rows_out, keep_out, step_out, order_out, seen_out, red_out, stats_out}, false))
    return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  if (int r = set_device(c)) return r;
  const size_t F = (size_t)n_frames, W = (size_t)n_words;
  if (int r = upload(c, c->in[0], bits, sizeof(uint32_t) * F * W)) return r;
  if (n_rows)
    if (int r = upload(c, c->in[3], n_rows, sizeof(int) * F)) return r;
  if (flags)
    if (int r = upload(c, c->in[4], flags, F)) return r;
  // one block of outputs: verdict, n_rows, step, order, seen, red [F] ints each, the statistics, the keep bytes [F]
  const size_t col = up256(4 * F), o_stats = 6 * col, o_keep = o_stats + 256, total = o_keep + up256(F);
  VO_HIP_CHECK(c->out[0].ensure(total, c->stream));
  char* d = c->out[0].as<char>();
  auto ints = [&](int k) { return reinterpret_cast<int32_t*>(d + k * col); };
  if (int r = voe_map_keyframes_dev(m, n_frames, n_words, c->in[0].as<uint32_t>(), n_rows ? c->in[3].as<int>() : nullptr, n_max,
                                    flags ? c->in[4].as<uint8_t>() : nullptr, p, ints(0), reinterpret_cast<int*>(ints(1)),
                                    reinterpret_cast<uint8_t*>(d + o_keep), ints(2), order_out ? ints(3) : nullptr, ints(4), ints(5),
                                    reinterpret_cast<voe_map_keyframes_stats*>(d + o_stats)))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(verdict_out, ints(0), 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(n_rows_out, ints(1), 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(step_out, ints(2), 4 * F, hipMemcpyDeviceToHost, c->stream));
  if (order_out) VO_HIP_CHECK(hipMemcpyAsync(order_out, ints(3), 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(seen_out, ints(4), 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(red_out, ints(5), 4 * F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(keep_out, d + o_keep, F, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d + o_stats, sizeof(voe_map_keyframes_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- single observations pruned (map_prune.hip; include/vo_hip.h: PRUNE) -------------------------------------------------------
static_assert(sizeof(voe_map_prune_params) == 32 && sizeof(voe_map_prune_landmark) == 32 && sizeof(voe_map_prune_frame) == 16 &&
                  sizeof(voe_map_prune_stats) == 64,
              "the records of include/vo_hip.h (PRUNE) as the kernels write them");

int voe_map_prune_batch_dev(vo_map* m, int n_frames, const float K[9], const float* d_uv, size_t uv_stride, const float* d_app,
                            size_t app_stride, int n_max, const int* d_n, const float* d_T16, const voe_map_prune_params* p,
                            int32_t* d_entry_out, int32_t* d_status_out, double* d_sq_out, float* d_app_out,
                            voe_map_prune_landmark* d_landmark_out, voe_map_prune_frame* d_frame_out, voe_map_prune_stats* d_stats) {
  const char* fn = "voe_map_prune_batch_dev";
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  if (int r = map_prune_check(fn, f, p, MapPrunePtrs{d_T16, d_entry_out, d_status_out, d_sq_out, d_app_out, d_landmark_out, d_frame_out, d_stats}))
    return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  // the call's own workspace is indexed by row alone; the lists (ref_ws) are allocated for the capacity and laid out for the
  // launch bound by refine_prepare, as for the cull
  const size_t need = map_prune_layout(nullptr, n_frames, n_max).bytes;
  if (int r = window_growth_check(m, fn, f, {{m->prune_ws.cap, need}})) return r;       // (before the lookup is enqueued)
  MapRefineWs rw;
  if (int r = refine_prepare(fn, m, f, &rw)) return r;        // the one lookup of the call
  VO_HIP_CHECK(m->prune_ws.ensure(need, c->stream));
  MapPruneArgs a{};
  a.l = rw; a.w = map_prune_layout(m->prune_ws.p, n_frames, n_max);
  fill_map(a.v, m);
  fill_frames(a.v, f, d_T16);
  a.app = d_app; a.app_stride = app_stride; a.d_n = d_n; a.nb = map_prune_blocks(n_max);
  a.max_sq = (double)p->max_err_px * (double)p->max_err_px;
  a.rf2 = (double)p->rel_factor * (double)p->rel_factor;
  a.floor2 = (double)p->rel_floor_px * (double)p->rel_floor_px;
  a.rel_on = p->rel_factor > 0.f; a.rel_min_obs = p->rel_min_obs; a.unique = p->unique;
  a.share_landmark = p->max_share_landmark; a.share_frame = p->max_share_frame;
  a.entry_out = d_entry_out; a.status_out = d_status_out; a.sq_out = d_sq_out; a.app_out = d_app_out;
  a.landmark_out = d_landmark_out; a.frame_out = d_frame_out; a.stats = reinterpret_cast<int*>(d_stats);
  VO_HIP_CHECK(launch_map_prune(c->stream, a, c->n_cu));
  return VO_OK;
}

int voe_map_prune_dev(vo_map* m, const float K[9], const float* d_uv, const float* d_app, int n_max, const int* d_n, const float* d_T16,
                      const voe_map_prune_params* p, int32_t* d_entry_out, int32_t* d_status_out, double* d_sq_out, float* d_app_out,
                      voe_map_prune_landmark* d_landmark_out, voe_map_prune_frame* d_frame_out, voe_map_prune_stats* d_stats) {
  const size_t stride = (size_t)(n_max > 0 ? n_max : 0);
  return voe_map_prune_batch_dev(m, 1, K, d_uv, stride, d_app, stride, n_max, d_n, d_T16, p, d_entry_out, d_status_out, d_sq_out, d_app_out,
                                 d_landmark_out, d_frame_out, d_stats);
}

int voe_map_prune(vo_map* m, int n_frames, const float K[9], const float* uv, const float* app, const int* n_rows, int n_max, const float* T16,
                  const voe_map_prune_params* p, int32_t* entry_out, int32_t* status_out, double* sq_out, float* app_out,
                  voe_map_prune_landmark* landmark_out, voe_map_prune_frame* frame_out, voe_map_prune_stats* stats_out) {
  const char* fn = "voe_map_prune";
  if (!(K && T16)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!p || !entry_out) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or entry_out", fn);
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  MapFrames f;
  int size = 0;
  if (int r = upload_window(fn, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, T16, nullptr, &size, &f)) return r;
  // one block of outputs: entries and statuses [rows] ints each, |e|^2 [rows] doubles, the landmarks' and the frames' records,
  // the statistics.  The rows that go out are written in place over the staged rows (d_app_out == d_app).
  const size_t F = (size_t)n_frames, rows = F * (size_t)n_max, S = (size_t)(size > 0 ? size : 1);
  const size_t col = up256(4 * rows), o_sq = 2 * col, o_lm = o_sq + up256(8 * rows), o_fr = o_lm + up256(sizeof(voe_map_prune_landmark) * S),
               o_stats = o_fr + up256(sizeof(voe_map_prune_frame) * F), total = o_stats + 256;
  VO_HIP_CHECK(c->out[0].ensure(total, c->stream));
  char* d = c->out[0].as<char>();
  if (int r = voe_map_prune_batch_dev(m, n_frames, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(), p,
                                      reinterpret_cast<int32_t*>(d), status_out ? reinterpret_cast<int32_t*>(d + col) : nullptr,
                                      sq_out ? reinterpret_cast<double*>(d + o_sq) : nullptr, app_out && rows > 0 ? c->in[1].as<float>() : nullptr,
                                      landmark_out ? reinterpret_cast<voe_map_prune_landmark*>(d + o_lm) : nullptr,
                                      frame_out ? reinterpret_cast<voe_map_prune_frame*>(d + o_fr) : nullptr,
                                      reinterpret_cast<voe_map_prune_stats*>(d + o_stats)))
    return r;
  if (rows > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(entry_out, d, 4 * rows, hipMemcpyDeviceToHost, c->stream));
    if (status_out) VO_HIP_CHECK(hipMemcpyAsync(status_out, d + col, 4 * rows, hipMemcpyDeviceToHost, c->stream));
    if (sq_out) VO_HIP_CHECK(hipMemcpyAsync(sq_out, d + o_sq, 8 * rows, hipMemcpyDeviceToHost, c->stream));
    if (app_out) VO_HIP_CHECK(hipMemcpyAsync(app_out, c->in[1].p, sizeof(float) * 10 * rows, hipMemcpyDeviceToHost, c->stream));
  }
  if (landmark_out && size > 0)
    VO_HIP_CHECK(hipMemcpyAsync(landmark_out, d + o_lm, sizeof(voe_map_prune_landmark) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  if (frame_out) VO_HIP_CHECK(hipMemcpyAsync(frame_out, d + o_fr, sizeof(voe_map_prune_frame) * F, hipMemcpyDeviceToHost, c->stream));
  if (stats_out) VO_HIP_CHECK(hipMemcpyAsync(stats_out, d + o_stats, sizeof(voe_map_prune_stats), hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- the pose graph over similarities (pose_graph.hip; include/vo_pose_graph.h) -- a context and no map ----------------------
static_assert(sizeof(voe_pose_graph_params) == 28 && sizeof(voe_pose_graph_round) == 40 && sizeof(voe_pose_graph_stats) == 48,
              "the records of include/vo_pose_graph.h as the kernels write them");

int voe_pose_graph_dev(vo_ctx* c, int n_frames, float* d_S16, int n_edges, const int32_t* d_edges, const float* d_Z16,
                       const float* d_weights, const uint8_t* d_fixed, const voe_pose_graph_params* p, int32_t* d_edge_status_out,
                       double* d_edge_cost_out, voe_pose_graph_round* d_rounds_out, voe_pose_graph_stats* d_stats) {
  const char* fn = "voe_pose_graph_dev";
  VO_REQUIRE(c, "null context");
  VO_REQUIRE(ctx_alive(c), "the context has been destroyed");
  if (int r = pose_graph_check(fn, n_frames, n_edges, PoseGraphPtrs{d_S16, d_edges, d_Z16, d_weights, d_edge_status_out, d_edge_cost_out, d_rounds_out, d_stats}, p))
    return r;
  const size_t need = pose_graph_layout(nullptr, n_frames, n_edges).bytes;
  if (int r = capture_growth_check(c->capturing, fn, {{c->pose_graph_ws.cap, need}}, "at least %d frames and %d edges", n_frames, n_edges)) return r;
  if (!c->capturing)
    if (int r = set_device(c)) return r;
  VO_HIP_CHECK(c->pose_graph_ws.ensure(need, c->stream));
  PoseGraphArgs a{};
  a.w = pose_graph_layout(c->pose_graph_ws.p, n_frames, n_edges);
  a.n_frames = n_frames; a.n_edges = n_edges;
  a.S16 = d_S16; a.edges = d_edges; a.Z16 = d_Z16; a.weights = d_weights; a.fixed = d_fixed;
  a.n_rounds = p->n_rounds; a.n_cg = p->n_cg; a.with_scale = p->with_scale != 0; a.precond = p->preconditioner;
  a.cg_tol = p->cg_tol; a.lambda0 = p->lambda0; a.huber = p->huber;
  a.edge_status_out = d_edge_status_out; a.edge_cost_out = d_edge_cost_out; a.rounds_out = d_rounds_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_pose_graph(c->stream, a));
  return VO_OK;
}

int voe_pose_graph(vo_ctx* c, int n_frames, float* S16, int n_edges, const int32_t* edges, const float* Z16, const float* weights,
                   const uint8_t* fixed, const voe_pose_graph_params* params, int32_t* edge_status_out, double* edge_cost_out,
                   voe_pose_graph_round* rounds_out, voe_pose_graph_stats* stats_out) {
  const char* fn = "voe_pose_graph";
  VO_REQUIRE(c, "null context");
  VO_REQUIRE(ctx_alive(c), "the context has been destroyed");
  VO_NOT_CAPTURING(c);
  alignas(8) static const char aligned_stand_in[8] = {};      // the host's own arrays need no device alignment: the staging has it
  if (int r = pose_graph_check(fn, n_frames, n_edges, PoseGraphPtrs{S16 ? aligned_stand_in : nullptr, edges ? aligned_stand_in : nullptr,
                                                                    Z16 ? aligned_stand_in : nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                    stats_out ? aligned_stand_in : nullptr}, params))
    return r;
  if (int r = set_device(c)) return r;
  const size_t F = (size_t)n_frames, E = (size_t)n_edges, R = (size_t)params->n_rounds;
  if (int r = upload(c, c->in[0], S16, sizeof(float) * 16 * F)) return r;
  if (int r = upload(c, c->in[1], edges, sizeof(int32_t) * 2 * E)) return r;
  if (int r = upload(c, c->in[2], Z16, sizeof(float) * 16 * E)) return r;
  if (weights)
    if (int r = upload(c, c->in[3], weights, sizeof(float) * 3 * E)) return r;
  if (fixed)
    if (int r = upload(c, c->in[4], fixed, F)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * (E ? E : 1), c->stream));
  VO_HIP_CHECK(c->out[1].ensure(sizeof(double) * (E ? E : 1), c->stream));
  VO_HIP_CHECK(c->out[2].ensure(sizeof(voe_pose_graph_stats) + sizeof(voe_pose_graph_round) * R + 16, c->stream));
  voe_pose_graph_stats* d_st = c->out[2].as<voe_pose_graph_stats>();
  voe_pose_graph_round* d_rd = reinterpret_cast<voe_pose_graph_round*>(d_st + 1);
  if (int r = voe_pose_graph_dev(c, n_frames, c->in[0].as<float>(), n_edges, E ? c->in[1].as<int32_t>() : nullptr, E ? c->in[2].as<float>() : nullptr,
                                 weights ? c->in[3].as<float>() : nullptr, fixed ? c->in[4].as<uint8_t>() : nullptr, params,
                                 edge_status_out ? c->out[0].as<int32_t>() : nullptr, edge_cost_out ? c->out[1].as<double>() : nullptr,
                                 rounds_out && R ? d_rd : nullptr, d_st))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d_st, sizeof(voe_pose_graph_stats), hipMemcpyDeviceToHost, c->stream));
  if (rounds_out && R) VO_HIP_CHECK(hipMemcpyAsync(rounds_out, d_rd, sizeof(voe_pose_graph_round) * R, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(S16, c->in[0].p, sizeof(float) * 16 * F, hipMemcpyDeviceToHost, c->stream));
  if (edge_status_out && E) VO_HIP_CHECK(hipMemcpyAsync(edge_status_out, c->out[0].p, sizeof(int32_t) * E, hipMemcpyDeviceToHost, c->stream));
  if (edge_cost_out && E) VO_HIP_CHECK(hipMemcpyAsync(edge_cost_out, c->out[1].p, sizeof(double) * E, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- the correction carried into the map (pose_graph.hip; include/vo_pose_graph.h): the lookup, the keys, the move -------------
static_assert(sizeof(voe_map_apply_stats) == 16, "the move kernel writes four 4-byte words");

int voe_map_apply_correction_batch_dev(vo_map* m, int n_frames, const float* d_uv, size_t uv_stride, const float* d_app, size_t app_stride,
                                       int n_max, const int* d_n, const float* d_S16_old, const float* d_S16_new, int dry_run,
                                       int32_t* d_ref_frame_out, voe_map_apply_stats* d_stats) {
  VO_MAP_LIVE(m);
  const char* fn = "voe_map_apply_correction_batch_dev";
  (void)d_uv; (void)uv_stride;
  if (int r = map_apply_check(fn, n_frames, d_app, app_stride, n_max, d_S16_old, d_S16_new, d_ref_frame_out, d_stats)) return r;
  const MapFrames f{n_frames, nullptr, nullptr, (size_t)n_max, d_app, app_stride, n_max, d_n};
  MapRefineWs w;
  if (int r = refine_prepare(fn, m, f, &w)) return r;         // the one lookup of the call (and the capture rule of the workspaces)
  MapApplyArgs a{};
  a.ent = w.ent; a.key = w.cnt;
  a.pts = m->d.pts; a.hdr = m->d.hdr; a.cap = m->d.cap; a.bound = map_launch_bound(m);
  a.n_frames = n_frames; a.n_max = n_max; a.S_old = d_S16_old; a.S_new = d_S16_new; a.dry_run = dry_run != 0;
  a.ref_frame_out = d_ref_frame_out; a.stats = reinterpret_cast<int*>(d_stats);
  VO_HIP_CHECK(launch_map_apply_correction(m->ctx->stream, a));
  return VO_OK;
}

int voe_map_apply_correction(vo_map* m, int n_frames, const float* uv, const float* app, const int* n_rows, int n_max, const float* S16_old,
                             const float* S16_new, int dry_run, int32_t* ref_frame_out, voe_map_apply_stats* stats_out) {
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  (void)uv;
  VO_REQUIRE(S16_old && S16_new && stats_out, "null argument");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(__func__, m, MapFrames{n_frames, nullptr, nullptr, 0, app, 0, n_max, n_rows}, nullptr, nullptr, &size, &f)) return r;
  const size_t F = (size_t)n_frames;
  if (int r = upload(c, c->in[2], S16_old, sizeof(float) * 16 * F)) return r;
  if (int r = upload(c, c->in[5], S16_new, sizeof(float) * 16 * F)) return r;
  VO_HIP_CHECK(c->out[0].ensure(sizeof(int32_t) * (size_t)(size > 0 ? size : 1), c->stream));
  VO_HIP_CHECK(c->out[2].ensure(64, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));          // the host arrays may go away after the call
  if (int r = voe_map_apply_correction_batch_dev(m, n_frames, nullptr, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n, c->in[2].as<float>(),
                                                 c->in[5].as<float>(), dry_run, ref_frame_out ? c->out[0].as<int32_t>() : nullptr,
                                                 c->out[2].as<voe_map_apply_stats>()))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, c->out[2].p, sizeof(voe_map_apply_stats), hipMemcpyDeviceToHost, c->stream));
  if (ref_frame_out && size > 0)
    VO_HIP_CHECK(hipMemcpyAsync(ref_frame_out, c->out[0].p, sizeof(int32_t) * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}

// ---- loop edges found and measured in the map (map_loops.hip; include/vo_map_loops.h) ------------------------------------------
static_assert(sizeof(voe_map_loops_params) == 72 && sizeof(voe_map_loop_record) == 40 && sizeof(voe_map_loops_stats) == 32,
              "the records of include/vo_map_loops.h as the kernels write them");

int voe_map_loops_batch_dev(vo_map* m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9], const float* d_uv,
                            size_t uv_stride, const float* d_app, size_t app_stride, int n_max, const int* d_n, const float* d_S16,
                            const voe_map_loops_params* p, int32_t* d_edges_out, float* d_Z16_out, float* d_weights_out,
                            voe_map_loop_record* d_loops_out, int32_t* d_hist_out, int32_t* d_ref_frame_out, voe_map_loops_stats* d_stats) {
  const char* fn = "voe_map_loops_batch_dev";
  // the refusals that need no map come first: they are the same on a machine without a device
  if (int r = map_loops_check(fn, n_frames, MapLoopsPtrs{d_S16, d_edges_out, d_Z16_out, d_weights_out, d_loops_out, d_hist_out, d_ref_frame_out, d_stats}, p))
    return r;
  VO_MAP_LIVE(m);
  const MapFrames f{n_frames, K, d_uv, uv_stride, d_app, app_stride, n_max, d_n};
  if (p->ransac.n_hypotheses == 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_hypotheses == 0 (a loop has no prior pose to start from)", fn);
  if (int r = localise_check(fn, f, &p->ransac, p->n_iters, p->min_inliers, nullptr, d_Z16_out, reinterpret_cast<const vo_map_localise_stats*>(d_stats)))
    return r;
  VO_REQUIRE(uv_stride >= (size_t)n_max && app_stride >= (size_t)n_max, "a stride is smaller than n_max");
  VO_REQUIRE(uv_stride < 0x7fffffff, "stride too large");
  if (int r = map_lookup_check(f, true)) return r;            // the lookup's own refusals, before anything is sized
  vo_ctx* c = m->ctx;
  const int L = p->max_loops;
  const size_t need = map_loops_layout(nullptr, n_frames, n_max, m->bd.alloc_bound(), L).bytes;      // (for the capacity: MapBound::alloc_bound)
  if (int r = window_growth_check(m, fn, f, {{m->loops_ws.cap, need}, {m->look_ws.cap, lookup_scratch_bytes(f, false)}})) return r;
  if (int r = set_device(c)) return r;
  VO_HIP_CHECK(m->loops_ws.ensure(need, c->stream));
  const int bound = map_launch_bound(m);
  const MapLoopsWs w = map_loops_layout(m->loops_ws.p, n_frames, n_max, bound, L);
  m->loops_last = w;
  // 1. the one lookup of the call
  if (int r = lookup_window(m, f, w.pairs, w.n_hits, w.ent)) return r;
  // 2. the reference frames: the launches of voe_map_apply_correction as a dry run with new == old -- nothing can move
  int32_t* ref = d_ref_frame_out ? d_ref_frame_out : w.ref;
  MapApplyArgs ap{};
  ap.ent = w.ent; ap.key = w.key;
  ap.pts = m->d.pts; ap.hdr = m->d.hdr; ap.cap = m->d.cap; ap.bound = bound;
  ap.n_frames = n_frames; ap.n_max = n_max; ap.S_old = d_S16; ap.S_new = d_S16; ap.dry_run = 1;
  ap.ref_frame_out = ref; ap.stats = w.apply_stats;
  VO_HIP_CHECK(launch_map_apply_correction(c->stream, ap));
  // 3. the covisibility's bit rows
  const int n_words = bound > 32 ? (int)(((long long)bound + 31) / 32) : 1;
  MapCovisArgs cv{};
  cv.w.ent = w.ent; cv.hdr = m->d.hdr; cv.cap = m->d.cap;
  cv.n_frames = n_frames; cv.n_max = n_max; cv.n_words = n_words; cv.d_n = d_n; cv.bits = w.bits;
  VO_HIP_CHECK(launch_map_covis_bits(c->stream, cv));
  // 4. histogram, candidates, choice, the slots' problems
  MapLoopsArgs a{};
  a.w = w;
  a.pts = m->d.pts; a.hdr = m->d.hdr; a.cap = m->d.cap; a.bound = bound;
  a.n_frames = n_frames; a.n_max = n_max; a.n_words = n_words;
  a.uv = d_uv; a.uv_stride = uv_stride; a.d_n = d_n; a.S16 = d_S16;
  a.gap = p->gap; a.ref_window = p->ref_window; a.min_shared = p->min_shared; a.separation = p->separation; a.max_loops = L;
  a.min_inliers = p->min_inliers;
  for (int k = 0; k < 3; ++k) a.w_loop[k] = p->w_loop[k];
  a.ref = ref; a.hist = d_hist_out;
  a.edges = d_edges_out; a.Z16 = d_Z16_out; a.weights = d_weights_out; a.loops = d_loops_out; a.stats = d_stats;
  VO_HIP_CHECK(launch_map_loops_find(c->stream, a));
  // 5. the measurement: the two public batched calls over the slots, at constant strides of n_max
  const size_t N = (size_t)n_max;
  if (int r = vo_estimate_pose_ransac_batch_dev(c, L, rows, cols, z_near, z_far, K, w.world, N, n_max, w.uv, N, n_max, w.lpairs, N, w.n_pairs, &p->ransac,
                                                w.T_start, w.handed, w.n_handed, nullptr, nullptr, w.rstat))
    return r;
  if (int r = vo_picp_solve_batch_dev(c, L, rows, cols, z_near, z_far, K, p->kernel_threshold, 0, w.world, N, w.uv, N, w.handed, N, w.n_handed, w.T_start,
                                      p->n_iters, w.T_solved, w.stats4))
    return r;
  // 6. status, edge, record, statistics
  VO_HIP_CHECK(launch_map_loops_finish(c->stream, a));
  return VO_OK;
}

int voe_map_loops_problems_dev(vo_map* m, voe_map_loops_problems* out) {
  VO_MAP_LIVE(m);
  VO_REQUIRE(out, "null argument");
  const MapLoopsWs& w = m->loops_last;
  if (w.bytes == 0) return vo_fail(VO_ERR_NOT_READY, "%s: no voe_map_loops call has been made on this map", __func__);
  *out = voe_map_loops_problems{w.world, w.uv, w.lpairs, w.n_pairs, w.cand, w.handed, w.n_handed, w.T_solved, w.stats4};
  return VO_OK;
}

int voe_map_loops(vo_map* m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9], const float* uv, const float* app,
                  const int* n_rows, int n_max, const float* S16, const voe_map_loops_params* p, int32_t* edges_out, float* Z16_out,
                  float* weights_out, voe_map_loop_record* loops_out, int32_t* hist_out, int32_t* ref_frame_out, voe_map_loops_stats* stats_out) {
  const char* fn = "voe_map_loops";
  alignas(8) static const char stand_in[8] = {};      // the host's own arrays need no device alignment: the staging has it
  const auto si = [](const void* q) { return q ? (const void*)stand_in : nullptr; };
  if (int r = map_loops_check(fn, n_frames, MapLoopsPtrs{si(S16), si(edges_out), si(Z16_out), si(weights_out), si(loops_out), nullptr, nullptr, si(stats_out)}, p))
    return r;
  VO_MAP_LIVE(m);
  vo_ctx* c = m->ctx;
  VO_NOT_CAPTURING(c);
  VO_REQUIRE(K && uv && app, "null argument");
  MapFrames f;
  int size = 0;
  if (int r = upload_window(fn, m, MapFrames{n_frames, K, uv, 0, app, 0, n_max, n_rows}, S16, nullptr, &size, &f)) return r;
  const size_t F = (size_t)n_frames, L = (size_t)p->max_loops, M = (size_t)(size > 0 ? size : 1);
  // one block of outputs: edges, Z, weights, records, statistics, then the histogram and the reference frames
  const size_t o_edges = 0, o_Z = o_edges + up256(8 * L), o_w = o_Z + up256(64 * L), o_rec = o_w + up256(12 * L), o_stats = o_rec + up256(40 * L),
               o_hist = o_stats + 256, o_ref = o_hist + up256(hist_out ? 4 * F * F : 0), total = o_ref + up256(ref_frame_out ? 4 * M : 0);
  VO_HIP_CHECK(c->out[0].ensure(total, c->stream));
  char* d = c->out[0].as<char>();
  if (int r = voe_map_loops_batch_dev(m, n_frames, rows, cols, z_near, z_far, K, f.d_uv, f.uv_stride, f.d_app, f.app_stride, n_max, f.d_n,
                                      c->in[2].as<float>(), p, reinterpret_cast<int32_t*>(d + o_edges), reinterpret_cast<float*>(d + o_Z),
                                      reinterpret_cast<float*>(d + o_w), reinterpret_cast<voe_map_loop_record*>(d + o_rec),
                                      hist_out ? reinterpret_cast<int32_t*>(d + o_hist) : nullptr,
                                      ref_frame_out ? reinterpret_cast<int32_t*>(d + o_ref) : nullptr, reinterpret_cast<voe_map_loops_stats*>(d + o_stats)))
    return r;
  VO_HIP_CHECK(hipMemcpyAsync(edges_out, d + o_edges, 8 * L, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(Z16_out, d + o_Z, 64 * L, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(weights_out, d + o_w, 12 * L, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(loops_out, d + o_rec, 40 * L, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipMemcpyAsync(stats_out, d + o_stats, sizeof(voe_map_loops_stats), hipMemcpyDeviceToHost, c->stream));
  if (hist_out) VO_HIP_CHECK(hipMemcpyAsync(hist_out, d + o_hist, 4 * F * F, hipMemcpyDeviceToHost, c->stream));
  if (ref_frame_out && size > 0) VO_HIP_CHECK(hipMemcpyAsync(ref_frame_out, d + o_ref, 4 * (size_t)size, hipMemcpyDeviceToHost, c->stream));
  VO_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VO_OK;
}
