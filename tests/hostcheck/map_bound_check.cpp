// map_bound_check -- the host's bound of a map's size (visual-odometry_amd/csrc/map_checks.h: MapBound) next to a brute-force model
// of the size the device holds, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_bound_check.cpp -o map_bound_check && ./map_bound_check      (ends with "map_bound_check: all ok")
// The model does what capi_map.hip does around every transition (map_reserve before an update, a grow or a merge; vo_map_size in
// front of the host forms) and what the kernels do to the size: an update of n rows appends between 0 and n entries, never past
// the capacity (the rest is dropped and counted), a cull leaves some of them, a replay of a captured graph does all of that
// again with the host looking away.  After EVERY event: bound() >= the true size.  After every event in which the host reads the
// size: size_ub == the true size, and bound() == it unless an update has been captured (then bound() is the capacity).  When a
// call on the map's own entries RUNS -- at once if eager, at each replay if captured -- the launch bound it was enqueued with is
// >= the size at that moment.  The last one is what the rule "inside a capture the capacity" is for: the scripted sequence shows
// that the bound() of the capture's moment would have been too small from the second replay of { window call ; update } on.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "map_checks.h"

int vo_fail(int code, const char*, ...) { return code; }

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...) \
  do { ++g_checks; if (!(cond)) { ++g_bad; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Op { int kind, n, launch_bound, old_rule_bound; };      // kind 0: update / grow of at most n entries, 1: a call on the map's entries
struct Graph { std::vector<Op> ops; int cap_at_capture; };

struct Model {
  MapBound bd;
  long long size = 0, dropped = 0;      // what the device holds
  int cap = 0;
  bool capturing = false;
  Graph cur;
  std::vector<Graph> graphs;
  std::mt19937 rng;
  int old_rule_short = 0;               // replays in which the bound() of the capture's moment was below the size
  explicit Model(int capacity, unsigned seed) : rng(seed) { cap = capacity; bd.on_arrays(cap); }

  int upto(int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)(n + 1)); }
  void after(const char* what) { CHECK(bd.bound() >= size, "%s: bound %d, size %lld", what, bd.bound(), size); CHECK(bd.cap == cap, "%s: cap", what); }
  void host_read(const char* what) {    // vo_map_size: the stream idle, the header read
    bd.on_size_read((int)size);
    CHECK(bd.size_ub == size, "%s: size_ub %lld, size %lld", what, bd.size_ub, size);
    CHECK(bd.replayable ? bd.bound() == cap : bd.bound() == size, "%s: bound %d after a read of %lld", what, bd.bound(), size);
  }
  void append(int k) {                  // the device's side of an update: what does not fit is dropped and counted
    const long long room = cap - size, take = k < room ? k : room;
    size += take; dropped += k - take;
  }
  // map_reserve(m, n): false = refused (inside a capture the map would have to grow)
  bool reserve(int n) {
    if (bd.room_known(capturing, n)) return true;
    if (capturing) return false;
    bd.on_size_read((int)size);
    if (size + n <= cap) return true;
    long long want = 2ll * cap;
    if (want < size + n) want = size + n + (size + n) / 2;
    cap = (int)want; bd.on_arrays(cap);
    for (Graph& g : graphs) g.cap_at_capture = -1;      // (a graph must not run after the arrays moved: vo_hip.h)
    return true;
  }
  void clear() { if (capturing) return; size = 0; dropped = 0; bd.on_clear(); after("clear"); }
  void update(int n, bool grow = false, bool dry = false) {      // vo_map_update_dev / voe_map_grow_batch_dev
    if (!dry && !reserve(n)) { after("refused update"); return; }
    if (capturing) cur.ops.push_back(Op{0, dry ? 0 : n, 0, 0});
    else if (!dry) append(upto(n));
    if (grow) bd.on_grow(n, capturing, dry); else bd.on_update(n, capturing);
    after(grow ? "grow" : "update");
  }
  void window_call() {                  // refinement, pose refinement, bundle, cull (dry here), transform: _dev forms
    const int L = bd.launch_bound(capturing);
    if (capturing) cur.ops.push_back(Op{1, 0, L, bd.bound()});
    else CHECK(L >= size, "eager window call: launch bound %d, size %lld", L, size);
    CHECK(bd.alloc_bound() >= L, "workspace allocation below the launch bound");
    after("window call");
  }
  void dev_cull() { if (capturing) return; size = upto((int)size); after("cull_dev"); }      // the host learns nothing
  void host_cull(bool dry) { if (capturing) return; host_read("host cull"); const int k = dry ? (int)size : upto((int)size); size = k; bd.on_host_cull(k, dry); after("host cull"); if (!bd.replayable) CHECK(bd.bound() == size, "host cull: bound"); }
  void host_grow(int room, bool dry) {
    if (capturing) return;
    if (!dry && !reserve(room)) return;
    if (!dry) append(upto(room));
    bd.on_grow(room, false, dry);
    bd.on_host_grow((int)size, dry);
    after("host grow");
    if (!bd.replayable && !dry) CHECK(bd.bound() == size, "host grow: bound %d size %lld", bd.bound(), size);
  }
  void host_merge(Model& src) {         // voe_map_merge(dst = this, src)
    if (capturing || src.capturing) return;
    src.host_read("merge: src");
    const int n_max = src.bd.bound();
    if (!reserve(n_max)) return;
    append(upto((int)src.size));
    bd.on_update(n_max, false);
    bd.on_host_merge((int)size);
    after("host merge");
    if (!bd.replayable) CHECK(bd.bound() == size, "host merge: bound");
  }
  void begin() { if (!capturing) { capturing = true; cur = Graph{{}, cap}; } }
  void end() { if (capturing) { capturing = false; graphs.push_back(cur); after("end capture"); } }
  void replay(size_t g) {               // the host sees nothing of it
    if (capturing || g >= graphs.size() || graphs[g].cap_at_capture != cap) return;
    for (const Op& op : graphs[g].ops) {
      if (op.kind == 0) append(upto(op.n));
      else {
        CHECK(op.launch_bound >= size, "replayed window call: launch bound %d, size %lld", op.launch_bound, size);
        if (op.old_rule_bound < size) ++old_rule_short;
      }
    }
    after("replay");
  }
};

int main() {
  // ---- scripted: the per-frame graph { window call ; update of 300 rows } on a map of capacity 1024 holding 300 entries ----
  {
    Model m(1024, 1);
    m.update(300); m.size = 300;        // (every row a new entry)
    m.window_call();                    // the eager warm-up
    m.begin(); m.window_call(); m.update(300); m.end();
    CHECK(m.graphs[0].ops[0].launch_bound == 1024 && m.graphs[0].ops[0].old_rule_bound == 300, "the capture bakes in the capacity");
    for (int k = 0; k < 3; ++k) { const long long before = m.size; m.replay(0); m.size = before + 300 > 1024 ? 1024 : before + 300; }
    CHECK(m.old_rule_short == 2, "bound() at the capture would have been short in replays 2 and 3, was in %d", m.old_rule_short);
    CHECK(m.bd.bound() == 1024 && m.size == 1024, "after the replays");
    m.host_read("scripted");
    m.window_call();
    std::printf("scripted { window call ; update }: the capture's bound() short in %d of 3 replays, the launch bound in none -> %s\n", m.old_rule_short, g_bad ? "FAILED" : "ok");
  }
  // ---- scripted: the states of tests/map_states.py ----
  {
    Model m(4096, 2);
    m.update(300); m.size = 300; CHECK(m.bd.bound() == 300, "exact");
    m.update(1); m.size = 300; CHECK(m.bd.bound() == 301, "slack_1");
    m.update(299); m.size = 300; CHECK(m.bd.bound() == 600, "slack");
    m.host_read("slack"); CHECK(m.bd.bound() == 300, "a read puts the bound back on the size");
    Model r(1024, 3);
    r.update(300); r.size = 300; r.begin(); r.update(300); r.end();
    CHECK(r.bd.bound() == 1024 && r.bd.size_ub == 600, "replayed: the capacity, the host counted 600");
    r.clear(); CHECK(r.bd.bound() == 1024, "a cleared map whose update was captured keeps the capacity as its bound");
    std::printf("scripted states -> %s\n", g_bad ? "FAILED" : "ok");
  }
  // ---- seeded random sequences of every event ----
  long long events = 0;
  for (unsigned seed = 1; seed <= 400; ++seed) {
    Model a(seed % 3 ? 1024 : 64, seed), b(256, seed + 1000);
    std::mt19937 pick(seed * 7919u);
    for (int step = 0; step < 300; ++step, ++events) {
      Model& m = (pick() & 7) ? a : b;
      const int n = 1 + (int)(pick() % 400);
      switch (pick() % 16) {
        case 0: m.clear(); break;
        case 1: case 2: m.update(n); break;
        case 3: m.update(n, true, (pick() & 1) != 0); break;
        case 4: m.begin(); break;
        case 5: m.end(); break;
        case 6: case 7: case 8: m.replay(pick() % (m.graphs.size() + 1)); break;
        case 9: case 10: m.window_call(); break;
        case 11: m.dev_cull(); break;
        case 12: m.host_cull((pick() & 3) == 0); break;
        case 13: m.host_grow(n, (pick() & 3) == 0); break;
        case 14: if (!m.capturing) m.host_read("read"); break;
        default: a.host_merge(b); break;
      }
    }
    a.end(); b.end();
  }
  std::printf("%lld random events over 400 seeds, %d checks -> %s\n", events, g_checks, g_bad ? "FAILED" : "ok");
  if (g_bad) { std::printf("map_bound_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_bound_check: all ok\n");
  return 0;
}
