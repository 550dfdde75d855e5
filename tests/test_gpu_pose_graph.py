"""voe_pose_graph* on the device against the float64 restatement (tests/pose_graph_restatement.py), case by case
(tests/pose_graph_cases.py): statuses, whole-number statistics, the accept pattern and the PCG iteration counts equal; costs to
1e-9 relative; the stored state, per active frame, within the ceiling in sqrt(d^T H_ff d) -- 4 x the distance between the
restatement's forward-order and reversed-order runs (profiles/pose_graph_budget.json, measured on the CPU alone and re-measured
by tests/test_pose_graph_cpu.py) plus half an ulp of each stored float32 entry carried through |H_ff|.  Then bytes: three calls,
the host form, capture and replay, what a status other than OK leaves, held frames."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pose_graph_cases as Cc
import pose_graph_restatement as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "pose_graph_budget.json")))["cases"]


class Dev:
    """a case's arrays on the device and voe_pose_graph_dev on them"""

    def __init__(self, vo, ctx, case):
        self.vo, self.ctx, self.case = vo, ctx, case
        self.S0 = np.ascontiguousarray(np.asarray(case["S"], np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
        self.F = len(self.S0)
        e = np.asarray(case["edges"], np.int32).reshape(-1, 2)
        self.E = len(e)
        Z = np.ascontiguousarray(np.asarray(case["Z"], np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
        self.R = int(case["n_rounds"])
        self.d_S = ctx.to_device(self.S0)
        self.d_e = ctx.to_device(e) if self.E else 0
        self.d_Z = ctx.to_device(Z) if self.E else 0
        self.d_w = ctx.to_device(np.asarray(case["weights"], np.float32)) if case["weights"] is not None and self.E else 0
        self.d_fixed = ctx.to_device(np.asarray(case["fixed"], np.uint8)) if case["fixed"] is not None else 0
        self.d_es, self.d_ec = ctx.alloc(4 * max(self.E, 1) + 16), ctx.alloc(8 * max(self.E, 1) + 16)
        self.d_rounds, self.d_stats = ctx.alloc(40 * max(self.R, 1) + 16), ctx.alloc(64)
        self.prm = vo.PoseGraphParams(self.R, int(case["n_cg"]), float(case["cg_tol"]), float(case["lambda0"]), float(case["huber"]),
                                      int(bool(case["with_scale"])), P.PRECONDITIONER.index(case["preconditioner"]))

    def reset(self):
        self.ctx.h2d(self.d_S, self.S0)
        self.ctx.h2d(self.d_es, np.full(max(self.E, 1) + 4, -7, np.int32))
        self.ctx.h2d(self.d_ec, np.full(max(self.E, 1) + 2, -7.0, np.float64))
        self.ctx.h2d(self.d_rounds, np.full(10 * max(self.R, 1) + 4, -7, np.int32))
        self.ctx.h2d(self.d_stats, np.full(16, -7, np.int32))

    def call(self, outputs=True):
        v = lambda d: C.c_void_p(d) if d else None
        return self.ctx.lib.voe_pose_graph_dev(self.ctx.h, C.c_int(self.F), v(self.d_S), C.c_int(self.E), v(self.d_e), v(self.d_Z), v(self.d_w),
                                               v(self.d_fixed), C.byref(self.prm), v(self.d_es if outputs else 0), v(self.d_ec if outputs else 0),
                                               v(self.d_rounds if outputs else 0), v(self.d_stats))

    def read(self, d, shape, dtype):
        a = np.zeros(shape, dtype)
        self.ctx.d2h(a, d)
        return a

    def results(self):
        """(S16 (F, 16), edge status, edge cost, the rounds' records, the stats' bytes) as the device holds them"""
        self.ctx.synchronize()
        return (self.read(self.d_S, (self.F, 16), np.float32), self.read(self.d_es, self.E, np.int32), self.read(self.d_ec, self.E, np.float64),
                self.read(self.d_rounds, self.R, self.vo.POSE_GRAPH_ROUND_DTYPE), self.read(self.d_stats, 48, np.uint8))

    def got(self, res):
        st = self.vo.PoseGraphStats()
        C.memmove(C.byref(st), res[4].ctypes.data, 48)
        return dict(S_out=res[0].reshape(-1, 4, 4).transpose(0, 2, 1), stats=st.as_dict(), edge_status=res[1], edge_cost=res[2], rounds=res[3])

    def close(self):
        for d in (self.d_S, self.d_e, self.d_Z, self.d_w, self.d_fixed, self.d_es, self.d_ec, self.d_rounds, self.d_stats):
            if d:
                self.ctx.free(d)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(Cc.CASES))
def test_against_float64_and_every_form(vo, ctx, name):
    case, ref = Cc.CASES[name], Cc.reference(name)
    d = Dev(vo, ctx, case)
    try:
        runs = []
        for _ in range(3):                                    # three calls from the same start: the same bytes
            d.reset()
            assert d.call() == 0, ctx.lib.vo_last_error()
            runs.append(d.results())
        assert _same(runs[1], runs[0]) and _same(runs[2], runs[0])
        got, log = d.got(runs[0]), []
        for r in got["rounds"]:                               # every figure before anything is asserted
            print(f"{name}: round cost {r['cost']:.12g} -> {r['cost_candidate']:.12g}, lambda {r['lambda']:.3g}, {r['cg_iterations']} iterations, "
                  f"|r|/|r0| {r['residual']:.3g}, accepted {r['accepted']}")
        print(f"{name}: {vo.POSE_GRAPH_STATUS[got['stats']['status']]} (restatement {P.STATUS[ref['status']]}), cost "
              f"{got['stats']['cost_before']:.12g} -> {got['stats']['cost_after']:.12g} (restatement {ref['stats']['cost_before']:.12g} -> "
              f"{ref['stats']['cost_after']:.12g})")
        bad = Cc.compare(name, got, reach_of=np.full(d.F, BUDGET[name]["reach_max"]), log=log)
        print("\n".join(log))
        assert bad == [], bad
        if not (ref["status"] == 0 and ref["stats"]["n_accepted"] > 0):       # nothing but OK writes: every byte of d_S16 as it was
            assert runs[0][0].tobytes() == d.S0.tobytes()
        if case["fixed"] is not None:                         # held frames keep their 64 bytes
            held = np.asarray(case["fixed"]).astype(bool)
            assert runs[0][0][held].tobytes() == d.S0[held].tobytes()
        # without the optional outputs: the same state and statistics
        d.reset()
        assert d.call(outputs=False) == 0
        again = d.results()
        assert again[0].tobytes() == runs[0][0].tobytes() and again[4].tobytes() == runs[0][4].tobytes()
        # the host form from the same start
        hS, hst, hrounds, hes, hec = vo.pose_graph(case["S"], case["edges"], case["Z"], case["weights"], case["fixed"], ctx=ctx,
                                                   **{k: case[k] for k in P.DEFAULT})
        assert np.ascontiguousarray(hS.transpose(0, 2, 1)).reshape(-1, 16).tobytes() == runs[0][0].tobytes()
        assert hes.tobytes() == runs[0][1].tobytes() and hec.tobytes() == runs[0][2].tobytes() and hrounds.tobytes() == runs[0][3].tobytes()
        assert repr(hst) == repr(got["stats"])                # (repr: a NaN cost equals itself)
    finally:
        d.close()


def test_the_false_loop_has_the_largest_edge_cost(vo, ctx):
    case = Cc.FALSE_LOOP
    _, st, _, es, ec = vo.pose_graph(case["S"], case["edges"], case["Z"], case["weights"], case["fixed"], ctx=ctx, **{k: case[k] for k in P.DEFAULT})
    assert st["status"] == 0 and not es.any()
    assert int(np.argmax(ec)) == Cc.FALSE_LOOP_EDGE


def test_capture_and_replay(vo, ctx):
    lib = ctx.lib
    d = Dev(vo, ctx, Cc.CASES["held_middle_257"])
    try:
        d.reset()
        assert d.call() == 0
        eager = d.results()
        g = C.c_void_p()
        d.reset()
        ctx.synchronize()
        assert lib.vo_ctx_begin_capture(ctx.h) == 0
        rc = d.call()
        assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) == 0 and rc == 0, lib.vo_last_error()
        for _ in range(2):
            d.reset()
            assert lib.vo_graph_launch(g) == 0
            assert _same(d.results(), eager)
        assert lib.vo_graph_destroy(g) == 0
        # a graph larger than any call has sized: refused inside a capture before anything is enqueued
        big_case, _ = Cc.graph(3000, [(0, 2999)], seed=1)
        big = Dev(vo, ctx, dict(big_case, **dict(P.DEFAULT, n_rounds=1, n_cg=1)))
        try:
            big.reset()
            ctx.synchronize()
            assert lib.vo_ctx_begin_capture(ctx.h) == 0
            assert big.call() == -6 and b"capture" in lib.vo_last_error()
            assert lib.vo_ctx_end_capture(ctx.h, C.byref(g)) in (0, -3)
            if g.value:
                assert lib.vo_graph_destroy(g) == 0
        finally:
            big.close()
    finally:
        d.close()


def test_refusals(vo, ctx):
    d = Dev(vo, ctx, Cc.CASES["n3"])
    try:
        d.reset()
        E = -1                                                # VO_ERR_INVALID_ARG
        keep = d.prm
        for field, value in (("n_rounds", -1), ("n_cg", 0), ("cg_tol", -1.0), ("lambda0", float("nan")), ("huber", float("inf")), ("preconditioner", 2)):
            d.prm = vo.PoseGraphParams(*[getattr(keep, k) for k, _ in keep._fields_])
            setattr(d.prm, field, value)
            assert d.call() == E, field
        d.prm = keep
        S, d.d_S = d.d_S, 0
        assert d.call() == E and b"null argument" in ctx.lib.vo_last_error()
        d.d_S = S + 2
        assert d.call() == E and b"aligned" in ctx.lib.vo_last_error()
        d.d_S = S
        F, d.F = d.F, 0
        assert d.call() == E and b"n_frames" in ctx.lib.vo_last_error()
        d.F = F
        assert d.results()[0].tobytes() == d.S0.tobytes()     # a refusal enqueues nothing
        assert d.call() == 0
    finally:
        d.close()
