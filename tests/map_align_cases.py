"""The cases shared by tests/test_map_align_cpu.py (which asserts the conditions the GPU comparison rests on and writes
profiles/map_align_budget.json) and tests/test_gpu_map_align.py (which runs them on the device).

A case is a dict: dst_pts (Md, 3) float32, dst_app (Md, 10), src_pts (Ms, 3), src_app (Ms, 10) -- the entries of two maps, each
array what vo_map_update builds from itself (appearances distinct, NaN rows apart) --, params (tests/map_align_restatement.py:
DEFAULT) and, where a similarity was planted, truth = (c, R, t) with p_dst = c R p_src + t."""
import functools
import json
import os

import numpy as np

import map_align_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "profiles", "map_align_budget.json")


def _params(**kw):
    return dict(A.DEFAULT, **kw)


def rotation(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def inverse_moved(dst_pts, c, R, t):
    """src with p_dst = c R p_src + t, rounded to float32"""
    return ((np.asarray(dst_pts, np.float64) - t) @ R / c).astype(np.float32)


def appearances(rng, n):
    return rng.uniform(-1, 1, (n, 10)).astype(np.float32)


def planted(n_shared, rng_seed, c=1.7, angle=0.6, t=(0.5, -1.0, 2.0), n_src_only=0, n_dst_only=0, n_pushed=0, noise=0.0, extent=5.0,
            dst_pts=None, **params):
    """n_shared landmarks of a random scene in both maps, src moved by the inverse of (c, R, t) and permuted; entries of one map
    alone; n_pushed of the shared ones pushed by +-0.2 ... 0.4 per coordinate (in dst's units) in src; Gaussian noise on src"""
    rng = np.random.default_rng(rng_seed)
    R = rotation(rng.normal(size=3), angle)
    t = np.asarray(t, np.float64)
    pts = rng.uniform(-extent, extent, (n_shared, 3)) if dst_pts is None else np.asarray(dst_pts, np.float64)
    app = appearances(rng, n_shared + n_src_only + n_dst_only)
    dst_pts32 = np.concatenate([pts, rng.uniform(-extent, extent, (n_dst_only, 3))]).astype(np.float32)
    dst_app = np.concatenate([app[:n_shared], app[n_shared + n_src_only:]])
    moved = dst_pts32[:n_shared].astype(np.float64)
    pushed = np.sort(rng.choice(n_shared, n_pushed, replace=False)) if n_pushed else np.zeros(0, int)
    moved[pushed] += rng.uniform(0.2, 0.4, (n_pushed, 3)) * rng.choice([-1.0, 1.0], (n_pushed, 3))
    if noise:
        moved += rng.normal(0, noise, moved.shape)
    src_pts = np.concatenate([inverse_moved(moved, c, R, t), rng.uniform(-extent, extent, (n_src_only, 3)).astype(np.float32)])
    src_app = app[: n_shared + n_src_only]
    perm = rng.permutation(len(src_pts))
    inv = np.argsort(perm)
    return dict(dst_pts=dst_pts32, dst_app=dst_app, src_pts=src_pts[perm], src_app=src_app[perm], params=_params(**params),
                truth=(c, R, t), pushed_src=np.sort(inv[pushed]), shared_src=np.sort(inv[:n_shared]))


def example():
    """src = world.dat mapped by the inverse of c = 2.7, 0.9 rad about a random axis, t = (1.5, -4, 0.75), rounded to float32,
    permuted and 50 entries short; 40 of the rest pushed by +-0.2 ... 0.4.  Threshold 0.05, 64 hypotheses."""
    import map_refine_restatement as R
    P = R.example_problem()
    world, app = np.asarray(P["world_pts"], np.float32), np.asarray(P["world_app"], np.float32)
    rng = np.random.default_rng(11)
    c, Rm, t = 2.7, rotation(rng.normal(size=3), 0.9), np.array([1.5, -4.0, 0.75])
    keep = np.sort(rng.permutation(len(world))[:-50])
    pushed = np.sort(rng.choice(len(keep), 40, replace=False))
    moved = world[keep].astype(np.float64)
    moved[pushed] += rng.uniform(0.2, 0.4, (40, 3)) * rng.choice([-1.0, 1.0], (40, 3))
    perm = rng.permutation(len(keep))
    inv = np.argsort(perm)
    return dict(dst_pts=world, dst_app=app, src_pts=inverse_moved(moved, c, Rm, t)[perm], src_app=app[keep][perm],
                params=_params(threshold=0.05, n_hypotheses=64, seed=1), truth=(c, Rm, t), pushed_src=np.sort(inv[pushed]),
                shared_src=np.arange(len(keep)))


def planar():
    rng = np.random.default_rng(21)
    p = rng.uniform(-4, 4, (200, 3))
    p[:, 2] = 0.5 * p[:, 0] - 0.25 * p[:, 1] + 1.0              # one plane, tilted
    return planted(200, 22, dst_pts=p, n_pushed=10)


def collinear():
    """src's shared points on one line, exactly (small integers times (1, 2, 3) / 8): Sigma has rank 1 for every sample"""
    rng = np.random.default_rng(31)
    k = rng.permutation(400)[:60].astype(np.float64) - 200
    a = (k[:, None] * np.array([1.0, 2.0, 3.0]) / 8).astype(np.float32)
    R, t = rotation([1, 1, 0], 0.4), np.array([0.25, 0.5, -1.0])
    app = appearances(rng, 60)
    return dict(dst_pts=(1.5 * a.astype(np.float64) @ R.T + t).astype(np.float32), dst_app=app, src_pts=a, src_app=app, params=_params())


def coincident():
    rng = np.random.default_rng(32)
    app = appearances(rng, 40)
    return dict(dst_pts=rng.uniform(-3, 3, (40, 3)).astype(np.float32), dst_app=app, src_pts=np.tile(np.float32([1, 2, 3]), (40, 1)),
                src_app=app, params=_params())


def disjoint():
    c = planted(0, 33, n_src_only=50, n_dst_only=70)
    return c


def two():
    return planted(2, 34, n_src_only=20, n_dst_only=20)


def nan_case():
    """a shared landmark whose src point is NaN; NaN appearances on both sides (never matched); -0 against +0 (matched)"""
    c = planted(60, 35, n_src_only=5, n_dst_only=5, threshold=0.01)
    s = c["shared_src"]
    c["src_pts"][s[7], 1] = np.nan                             # among the matches: never an inlier, its samples invalid
    k = s[20]                                                  # a shared landmark: zeros in its appearance, of either sign
    e = int(np.flatnonzero((c["dst_app"] == c["src_app"][k]).all(1))[0])
    c["dst_app"][e, 3] = 0.0; c["src_app"][k, 3] = -0.0
    c["dst_app"][e, 8] = -0.0; c["src_app"][k, 8] = 0.0
    j = s[33]                                                  # shared until its appearance gets a NaN: then in no match
    c["src_app"][j, 0] = np.nan
    c["dst_app"][int(np.flatnonzero((c["dst_app"][:, 1:] == c["src_app"][s[40], 1:]).all(1))[0]), 9] = np.nan
    c["nan_point"], c["signed_zero"], c["nan_app_src"], c["nan_app_dst_of"] = int(s[7]), int(k), int(j), int(s[40])
    return c


def tie():
    """clean data and a generous threshold: every valid hypothesis counts every pair, the lowest h wins"""
    return planted(50, 36, threshold=0.05, n_refits=0)


def noisy():
    return planted(400, 37, noise=0.005, threshold=0.05, n_refits=2)


def refit_rejected():
    """30 exact pairs (group A), 25 shifted by +0.9 threshold along x (B) and 10 by -0.95 threshold (C), in src: a sample inside
    A counts all 65; its refit moves towards B by 0.2 threshold, C falls out (1.15 threshold), 55 < 65: the guard keeps the
    minimal model"""
    thr = 0.05
    c = planted(65, 38, c=1.0, angle=0.3, threshold=thr, n_refits=1, seed=3)
    _, R, t = c["truth"]
    s = c["shared_src"]
    order = np.argsort(c["src_app"][s][:, 0])                  # a fixed choice of the groups
    B, C = s[order[30:55]], s[order[55:]]
    x = R.T @ np.array([1.0, 0.0, 0.0])                        # a shift of dst's x, in src
    p = c["src_pts"].astype(np.float64)
    p[B] -= 0.9 * thr * x
    p[C] += 0.95 * thr * x
    c["src_pts"] = p.astype(np.float32)
    c["groups"] = (s[order[:30]], B, C)
    return c


def far():
    """|t| ~ 1e3 against a scene of extent 1"""
    return planted(500, 39, c=1.0, angle=1.1, t=(1000.0, -700.0, 400.0), extent=1.0, n_pushed=20, threshold=0.01, with_scale=1)


def rigid():
    return planted(300, 40, c=1.0, n_pushed=15, with_scale=0, n_src_only=10)


def sized(n_matches, n_hyp=64, n_miss=7, seed=50):
    """n_matches shared landmarks (a tenth pushed, from 16 on), n_miss entries of src alone"""
    return planted(n_matches, seed + n_matches, n_src_only=n_miss, n_dst_only=3, n_pushed=n_matches // 10 if n_matches >= 16 else 0,
                   n_hypotheses=n_hyp)


CASES = {
    "example": example, "rigid": rigid, "planar": planar, "collinear": collinear, "coincident": coincident, "disjoint": disjoint, "two": two,
    "nan": nan_case, "tie": tie, "noisy": noisy, "refit_rejected": refit_rejected, "far": far,
    **{f"matches_{n}": functools.partial(sized, n) for n in (3, 4, 255, 256, 257, 1023, 1024, 1025)},
    **{f"hyps_{h}": functools.partial(sized, 300, h) for h in (1, 63, 64, 65)},
    "src_65537": functools.partial(sized, 65537 - 7, 64, 7),
}
MERGE_CASES = {                                               # (case, n_miss): the misses at the block edges of the compaction
    **{f"miss_{k}": functools.partial(sized, 300, 64, k) for k in (0, 255, 256, 257)},
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return (CASES.get(name) or MERGE_CASES[name])()


def case(name):
    """a fresh copy (the arrays may be written)"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _case(name).items()}


@functools.lru_cache(maxsize=None)
def _reference(name, reverse):
    return A.run(_case(name), reverse=reverse)


def reference(name, reverse=False):
    return _reference(name, bool(reverse))


def spreads(name):
    """dict(S, scale, rms): forward against reversed summation"""
    f, r = reference(name), reference(name, True)
    return dict(S=float(np.abs(f["S"].astype(np.float64) - r["S"].astype(np.float64)).max()), scale=abs(f["scale"] - r["scale"]),
                rms=abs(f["rms"] - r["rms"]))


def budget_record(name):
    r = reference(name)
    rec = dict(r["stats"])
    rec["spread"] = spreads(name)
    rec["apriori"] = r["budget"] if r["budget"] is not None else dict(S=0.0, scale=0.0, rms=0.0)
    return rec


def ceilings(rec):
    """dict(S, scale, rms): 4 x the spread + 2 x the a-priori bound (the caller adds S's float32 ulp)"""
    return {k: 4 * rec["spread"][k] + 2 * rec["apriori"][k] for k in ("S", "scale", "rms")}


def load_budget():
    return json.load(open(BUDGET))["cases"]
