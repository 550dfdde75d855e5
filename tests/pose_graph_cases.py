"""The named cases of voe_pose_graph* that the CPU and the GPU test share: the smallest graphs at which the kernels can go wrong
(the scan's block edges, the lane lists' edges, every status, every kind of skipped edge, both preconditioners).  A case is the
keyword arguments of pose_graph_restatement.run / vo.pose_graph.  Everything is drawn from seeded generators of its own."""
import numpy as np

import pose_graph_restatement as P


def _rot(w):
    return P.rot_xyz(np.asarray(w, np.float64))


def _sim(c, w, t):
    S = np.eye(4)
    S[:3, :3] = c * _rot(w)
    S[:3, 3] = t
    return S


def truth(F, radius=4.0, turns=1.0):
    """a camera that goes round a circle (and comes back when turns >= 1), looking along its path: p_cam = S p_world, rigid"""
    S = np.zeros((F, 4, 4))
    for k in range(F):
        a = 2 * np.pi * turns * k / max(F - 1, 1)
        R = _rot([0.1 * np.sin(a), a, 0.0])
        c = np.array([radius * np.cos(a), 0.2 * np.sin(2 * a), radius * np.sin(a)])
        S[k] = np.eye(4)
        S[k, :3, :3] = R
        S[k, :3, 3] = -R @ c
    return S


def graph(F, loops=(), seed=1, drift=0.003, noise=0.004, rot_noise=0.002, t_noise=0.002, scale=True, loop_gap=None, drop=(), turns=1.0, perturb=0.0):
    """odometry edges k -> k + 1 with a scale drift per step and noise, ground-truth loop edges, the drifted chain as the start"""
    rng = np.random.default_rng(seed)
    gt = truth(F, turns=turns)
    edges, Z = [], []
    S = [gt[0].copy()]
    for k in range(F - 1):
        rel = gt[k + 1] @ np.linalg.inv(gt[k])
        c = np.exp(drift + noise * rng.standard_normal()) if scale else 1.0
        z = _sim(c, rot_noise * rng.standard_normal(3), t_noise * rng.standard_normal(3)) @ rel
        S.append(z @ S[-1])
        if k not in drop:
            edges.append((k, k + 1))
            Z.append(z)
    if loop_gap is not None:
        loops = list(loops) + [(k, k + loop_gap) for k in range(0, F - loop_gap, max(loop_gap // 2, 1))]
    for i, j in loops:
        edges.append((i, j))
        Z.append(gt[j] @ np.linalg.inv(gt[i]))
    for k in range(1, F):                                    # (off the chain: otherwise a graph without loops starts at its optimum)
        if perturb:
            S[k] = _sim(np.exp(perturb * rng.standard_normal()) if scale else 1.0, perturb * rng.standard_normal(3), perturb * rng.standard_normal(3)) @ S[k]
    fixed = np.zeros(F, np.uint8)
    fixed[0] = 1
    return dict(S=np.array(S, np.float32), edges=np.array(edges, np.int32).reshape(-1, 2), Z=np.array(Z, np.float32).reshape(-1, 4, 4),
                weights=None, fixed=fixed), gt


# PCG iterations of a case unless it says otherwise.  Two runs of the restatement that differ only in the order of the sums over
# the edges drift apart as the iterations go on (conjugate gradients lose their orthogonality as they converge: on the
# "weighted" graph 3e-16 of the candidate's cost after 2 iterations, 1e-14 after 4, 4e-11 after 6, 9e-7 after 8 under CHAIN), so a
# comparison to 1e-9 can tell a right kernel from a wrong one only while the iterations are few.  Four exercise every launch of
# an iteration four times; "cg8" and the example-data descent of the CPU test run the default eight.
N_CG = 4


def _case(g, **kw):
    d = dict(g)
    d.update(P.DEFAULT)
    d.update(n_cg=N_CG)
    d.update(kw)
    return d


def _chain(F, **kw):
    loops = [(0, F - 1)] if F > 2 else []
    if F > 40:
        loops += [(1, F - 2), (F // 3, F - 1 - F // 3)]
    return _case(graph(F, loops, seed=F)[0], n_rounds=3, **kw)


def _hub(deg):
    """frame 3 with exactly `deg` incident edges: its two odometry edges and deg - 2 loops, in both directions"""
    F = deg + 6
    others = [k for k in range(F) if abs(k - 3) > 1][:deg - 2]
    g, gt = graph(F, [(0, F - 1)], seed=100 + deg)
    e, Z = list(map(tuple, g["edges"])), list(g["Z"])
    for n, k in enumerate(others):
        i, j = (3, k) if n % 2 == 0 else (k, 3)
        e.append((i, j))
        Z.append(gt[j] @ np.linalg.inv(gt[i]))
    g.update(edges=np.array(e, np.int32), Z=np.array(Z, np.float32))
    return _case(g, n_rounds=3)


def _duplicates():
    g, gt = graph(12, [(0, 11), (1, 10)], seed=7)
    e, Z = list(map(tuple, g["edges"])), list(g["Z"])
    for k in (2, 5, len(g["edges"]) - 1):                    # the same edge again, and once more the other way round
        e.append(e[k])
        Z.append(Z[k])
        e.append((e[k][1], e[k][0]))
        Z.append(np.linalg.inv(np.asarray(Z[k], np.float64)))
    g.update(edges=np.array(e, np.int32), Z=np.array(Z, np.float32))
    return _case(g, n_rounds=3)


def _skipped():
    g, _ = graph(10, [(0, 9)], seed=9)
    E = len(g["edges"])
    e = np.concatenate([g["edges"], [(-1, 3), (2, 10), (4, 4), (1, 5), (2, 6), (3, 7), (5, 8)]]).astype(np.int32)
    Z = np.concatenate([g["Z"], np.tile(np.eye(4, dtype=np.float32), (7, 1, 1))])
    w = np.ones((E + 7, 3), np.float32)
    w[E + 3] = (1, -1, 1)
    w[E + 4] = (np.nan, 1, 1)
    w[E + 5] = (0, 0, 0)
    w[E + 6] = (1, np.inf, 1)
    g.update(edges=e, Z=Z, weights=w)
    return _case(g, n_rounds=1), E


def _false_loop():
    g, gt = graph(30, [(0, 29), (1, 28), (2, 27)], seed=11)
    e, Z = list(map(tuple, g["edges"])), list(g["Z"])
    e.append((5, 20))
    Z.append(_sim(1.0, [0.0, 0.3, 0.0], [0.5, 0.0, 0.3]) @ gt[20] @ np.linalg.inv(gt[5]))
    g.update(edges=np.array(e, np.int32), Z=np.array(Z, np.float32))
    return _case(g, n_rounds=6, huber=0.05), len(e) - 1


def _nan_z():
    g, _ = graph(8, [(0, 7)], seed=13)
    g["Z"][3, 1, 2] = np.nan
    return _case(g, n_rounds=2)


def _zero_scale_weight():
    """no edge weighs the scale part: the scale is still held by the translations (the last column of G and of Ad)"""
    g, _ = graph(8, [(0, 7)], seed=15)
    g["weights"] = np.tile(np.array([1, 1, 0], np.float32), (len(g["edges"]), 1))
    return _case(g, n_rounds=3, preconditioner="JACOBI")


def _far_start():
    """a start far from the optimum and no damping to begin with: the first steps overshoot and are rejected"""
    g, _ = graph(20, [(0, 19), (2, 17)], seed=17, rot_noise=0.25, t_noise=0.4, noise=0.2)
    return _case(g, n_rounds=10, lambda0=0.0)


def _bad_pivot():
    """only the scale is weighted: the translation and rotation diagonals of every H_ff are exactly 0, so JACOBI's first pivot is
    exactly 0 -- no round is formed, lambda goes up by 10 each time, status NO_STEP, S16 is not written"""
    g, _ = graph(8, [(0, 7)], seed=15)
    g["weights"] = np.tile(np.array([0, 0, 1], np.float32), (len(g["edges"]), 1))
    return _case(g, n_rounds=2, preconditioner="JACOBI")


def _first_round_rejected():
    """one undamped round from a start twice as far as far_start's: 4 PCG iterations, the candidate at 1181.12 against 586.09,
    rejected, status NO_STEP"""
    g, _ = graph(20, [(0, 19), (2, 17)], seed=18, rot_noise=0.5, t_noise=0.8, noise=0.4)
    return _case(g, n_rounds=1, lambda0=0.0)


SKIPPED, N_GOOD_BEFORE_SKIPPED = _skipped()
FALSE_LOOP, FALSE_LOOP_EDGE = _false_loop()

CASES = {
    "n1": _case(dict(S=truth(1).astype(np.float32), edges=np.array([[0, 0]], np.int32), Z=np.eye(4, dtype=np.float32)[None], weights=None,
                     fixed=None), n_rounds=2),
    "n2": _case(graph(2, [], seed=2, perturb=0.05)[0], n_rounds=2),
    "n3": _case(graph(3, [(0, 2)], seed=3, perturb=0.05)[0], n_rounds=2, cg_tol=1e-9),
    "n255": _chain(255),
    "n256": _chain(256),
    "n257": _chain(257),
    "n513": _chain(513),
    "n513_jacobi": _chain(513, preconditioner="JACOBI"),
    "hub15": _hub(15),
    "hub16": _hub(16),
    "hub17": _hub(17),
    "hub65": _hub(65),
    "hub17_jacobi": dict(_hub(17), preconditioner="JACOBI"),
    "no_edges": _case(dict(graph(5, [], seed=3)[0], edges=np.zeros((0, 2), np.int32), Z=np.zeros((0, 4, 4), np.float32)), n_rounds=2),
    "duplicates": _duplicates(),
    "held_middle": _case(dict(graph(40, [(0, 39), (3, 36)], seed=4)[0], fixed=(np.arange(40) % 20 == 0).astype(np.uint8)), n_rounds=3),
    "held_middle_257": _case(dict(graph(300, [(0, 299), (3, 290)], seed=5)[0], fixed=np.isin(np.arange(300), (0, 100, 255, 256, 257)).astype(np.uint8)), n_rounds=3),
    "none_held": _case(dict(graph(30, [(0, 29), (2, 27)], seed=6)[0], fixed=None), n_rounds=3),
    "cg8": _case(dict(graph(30, [(0, 29), (2, 27)], seed=6)[0]), n_rounds=1, n_cg=8),
    "all_held": _case(dict(graph(6, [(0, 5)], seed=8)[0], fixed=np.ones(6, np.uint8)), n_rounds=2),
    "missing_odometry": _case(graph(30, [(0, 29), (8, 13)], seed=10, drop=(10,))[0], n_rounds=3),
    "rigid": _case(graph(30, [(0, 29), (2, 27)], seed=12, scale=False)[0], n_rounds=3, with_scale=False),
    "rigid_jacobi": _case(graph(30, [(0, 29), (2, 27)], seed=12, scale=False)[0], n_rounds=3, with_scale=False, preconditioner="JACOBI"),
    "false_loop": FALSE_LOOP,
    "nan_z": _nan_z(),
    "skipped": SKIPPED,
    "rounds0": _case(graph(20, [(0, 19)], seed=14)[0], n_rounds=0),
    "cg1": _case(graph(20, [(0, 19)], seed=14)[0], n_rounds=4, n_cg=1),
    "zero_scale_weight_jacobi": _zero_scale_weight(),
    "far_start": _far_start(),
    # the driver's branches that no other case runs: a pivot that is not > 0, and a call whose only round is rejected.  Its `nostep`
    # branch (p.q not > 0 at the first iteration) and status COST_ROSE stay without a case: no input is known that reaches them
    # without the restatement's own decision being marginal.
    "bad_pivot_jacobi": _bad_pivot(),
    "first_round_rejected": _first_round_rejected(),
    "jacobi_small": _case(graph(20, [(0, 19)], seed=14)[0], n_rounds=3, preconditioner="JACOBI"),
    "weighted": _case(dict(graph(25, [(0, 24), (1, 23)], seed=16)[0]), n_rounds=3),
}
_w = np.ones((len(CASES["weighted"]["edges"]), 3), np.float32)
CASES["weighted"]["weights"] = _w * np.array([2.0, 3.0, 1.5], np.float32)
_w = _w.copy()
_w[-2:] = (4.0, 9.0, 2.0)
_w[::3, 1] = 2.5
CASES["weighted_jacobi"] = dict(CASES["weighted"], weights=_w, preconditioner="JACOBI")

_REF = {}


def reference(name, **kw):
    """the restatement's run of a case, computed once and shared (callers must not change it); kw: reverse / fault"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _REF:
        _REF[key] = P.run(**CASES[name], **kw)
    return _REF[key]


def reach(name):
    """per frame: the distance between the forward-order and the reversed-order run of the restatement, in the forward run's blocks"""
    fwd, rev = reference(name), reference(name, reverse=True)
    d = P.step_between(fwd["state"], rev["state"])
    return np.sqrt(np.maximum(np.einsum("fa,fab,fb->f", d, fwd["H"], d), 0.0))


def ceiling(name, S_kept, reach_of=None):
    """per frame: 4 x that distance plus half an ulp of each stored entry carried through |H_ff|.  No device value goes into it
    but the stored state whose ulps are taken.  reach_of: the recorded distances (profiles/pose_graph_budget.json) instead of a
    fresh measurement."""
    r = reach(name) if reach_of is None else np.asarray(reach_of)
    return 4.0 * r + P.half_ulp(reference(name), S_kept)


EVAL = 1e-13


def compare(name, got, reach_of=None, log=None):
    """What the GPU test asserts of a call's outputs `got` (S_out F x 4 x 4 float32, stats dict, rounds records, edge_status,
    edge_cost) against the restatement's run of the case; returns the list of differences (empty: the call passes).
      statuses, whole-number statistics, the accept pattern, the PCG iteration counts, the lambdas' decades: equal
      costs: 1e-9 relative, plus what the double arithmetic of one evaluation can move a residual that is itself only rounding
      (EVAL: a few hundred ulps of double at coordinates of order 10 -- an edge at its optimum has |r| ~ 1e-7 from the float32 inputs,
      computed as a difference of numbers of order 1 to 10): |r| by EVAL, an edge's s^2 by 2 s EVAL + EVAL^2, a total over E edges by
      2 sqrt(cost E) EVAL + E EVAL^2; the costs of the ROUNDED state (cost_after, edge_cost of a call that wrote) may also move by what half
      an ulp of every stored entry moves a residual: |r| by s, s^2 = sum over the frames of (2 x the half-ulp term)^2, a cost of
      |r|^2 by 2 sqrt(cost) s + s^2
      the stored state: frames that are not ACTIVE keep their 64 bytes; an ACTIVE frame lies within ceiling() of the restatement's
      double state, in sqrt(d^T H_ff d)"""
    ref, case = reference(name), CASES[name]
    bad = []
    S_in = np.asarray(case["S"], np.float32).reshape(-1, 4, 4)
    S_out = np.asarray(got["S_out"], np.float32).reshape(-1, 4, 4)
    for k in ("status", "n_frames", "n_edges", "n_live_edges", "n_free_frames", "n_active_frames", "n_accepted"):
        if int(got["stats"][k]) != int(ref["stats"][k]):
            bad.append((k, got["stats"][k], ref["stats"][k]))
    wrote = ref["status"] == 0 and ref["stats"]["n_accepted"] > 0
    hu = P.half_ulp(ref, S_out)
    s = np.sqrt(((2 * hu[ref["kind"] == P.ACTIVE]) ** 2).sum()) if wrote else 0.0

    n_e = max(len(ref["edge_cost"]), 1)

    def close(a, b, slack=0.0, terms=n_e):
        if not (np.isfinite(a) and np.isfinite(b)):
            return bool(np.isnan(a) and np.isnan(b)) or a == b
        return abs(a - b) <= 1e-9 * abs(b) + slack + 2 * np.sqrt(abs(b) * terms) * EVAL + terms * EVAL * EVAL

    if not close(got["stats"]["cost_before"], ref["stats"]["cost_before"]):
        bad.append(("cost_before", got["stats"]["cost_before"], ref["stats"]["cost_before"]))
    ca = ref["stats"]["cost_after"]
    if not close(got["stats"]["cost_after"], ca, (2 * np.sqrt(ca) * s + s * s) if np.isfinite(ca) else 0.0):
        bad.append(("cost_after", got["stats"]["cost_after"], ca))
    if len(got["rounds"]) != len(ref["rounds"]):
        bad.append(("rounds", len(got["rounds"]), len(ref["rounds"])))
    for k, (g, r) in enumerate(zip(got["rounds"], ref["rounds"])):
        if int(g["accepted"]) != r["accepted"] or int(g["cg_iterations"]) != r["cg_iterations"]:
            bad.append(("round", k, int(g["accepted"]), int(g["cg_iterations"]), r["accepted"], r["cg_iterations"]))
        if not (close(g["cost"], r["cost"]) and close(g["cost_candidate"], r["cost_candidate"]) and abs(g["lambda"] - r["lam"]) <= 1e-12 * r["lam"]):
            bad.append(("round costs", k, float(g["cost"]), float(g["cost_candidate"]), float(g["lambda"]), r["cost"], r["cost_candidate"], r["lam"]))
    if not np.array_equal(np.asarray(got["edge_status"]), ref["edge_status"]):
        bad.append(("edge_status",))
    for e, (a, b) in enumerate(zip(np.asarray(got["edge_cost"]), ref["edge_cost"])):
        if not close(a, b, (2 * np.sqrt(b) * s + s * s) if np.isfinite(b) else 0.0, terms=1):
            bad.append(("edge_cost", e, float(a), float(b)))
    keep = ref["kind"] != P.ACTIVE if wrote else np.ones(len(S_in), bool)
    if S_out[keep].tobytes() != S_in[keep].tobytes():
        bad.append(("bytes of frames the call must not write",))
    if wrote:
        dist, ceil = P.distance(ref, S_out), ceiling(name, S_out, reach_of)
        act = ref["kind"] == P.ACTIVE
        if not np.all(S_out[act][:, 3] == np.array([0, 0, 0, 1], np.float32)):
            bad.append(("bottom row",))
        worst = int(np.argmax(np.where(act, dist / np.maximum(ceil, 1e-300), 0.0)))
        if log is not None:
            log.append(f"{name}: worst frame {worst}: {dist[worst]:.3g} = {dist[worst] / max(ceil[worst], 1e-300):.3g} of the ceiling {ceil[worst]:.3g}")
        if not np.all(dist[act] <= ceil[act]):
            bad.append(("state", worst, float(dist[worst]), float(ceil[worst])))
    return bad


def as_got(run):
    """a restatement run in the shape compare() takes"""
    return dict(S_out=run["S_out"], stats=run["stats"], edge_status=run["edge_status"], edge_cost=run["edge_cost"],
                rounds=[dict(r, **{"lambda": r["lam"]}) for r in run["rounds"]])


# ---- the example trajectory (121 frames), drifted as the issue's prototype drifted it ----
EXAMPLE_LOOPS = ((0, 103), (0, 104), (1, 104), (2, 105))
EXAMPLE_SEED = 1


def example_graph(seed=EXAMPLE_SEED):
    """ground-truth poses of the example data; odometry edges with a scale drift of 0.3 % per step, 0.4 % noise and 2 mrad /
    2 mm noise, chained into the start; four ground-truth loop edges; frame 0 held.  Returns (case arguments, ground truth)."""
    import map_refine_restatement as R
    gt = np.array(R.example_problem()["poses"], np.float64)
    rng = np.random.default_rng(seed)
    F = len(gt)
    edges, Z, S = [], [], [gt[0].copy()]
    for k in range(F - 1):
        z = _sim(np.exp(0.003 + 0.004 * rng.standard_normal()), 0.002 * rng.standard_normal(3), 0.002 * rng.standard_normal(3)) @ gt[k + 1] @ np.linalg.inv(gt[k])
        S.append(z @ S[-1])
        edges.append((k, k + 1))
        Z.append(z)
    for i, j in EXAMPLE_LOOPS:
        edges.append((i, j))
        Z.append(gt[j] @ np.linalg.inv(gt[i]))
    fixed = np.zeros(F, np.uint8)
    fixed[0] = 1
    return _case(dict(S=np.array(S, np.float32), edges=np.array(edges, np.int32), Z=np.array(Z, np.float32), weights=None, fixed=fixed), n_cg=8), gt


def centre_errors(S, gt):
    """distance of every camera centre -M^-1 t from the ground truth's"""
    S, gt = np.asarray(S, np.float64).reshape(-1, 4, 4), np.asarray(gt, np.float64).reshape(-1, 4, 4)
    c = lambda A: -np.einsum("fij,fj->fi", np.linalg.inv(A[:, :3, :3]), A[:, :3, 3])
    return np.linalg.norm(c(S) - c(gt), axis=1)
