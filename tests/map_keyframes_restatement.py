"""NumPy restatement of voe_map_keyframes* (include/vo_hip.h, KEYFRAMES: rules 1-9): the literal loop on unpacked bits, with plain
integer counts per entry -- no bit planes, no chunks, nothing of the device's decomposition.  Python integers do the cross-products.
`run` also records, per step, which frames were candidates (`candidates`), for the monotonicity check; `replay` verifies every drop
of a result from the outputs alone; `compare` is what the GPU test uses; `FAULTS` are planted against it."""
import numpy as np

import map_covis_restatement as V

VERDICT = ("LEFT", "PROTECTED", "GONE", "DROPPED", "EMPTY", "NEEDED", "GAP")
LEFT, PROTECTED, GONE, DROPPED, EMPTY, NEEDED, GAP = range(7)
FREE = 0                                                      # the flags: FREE, PROTECTED = 1, GONE = 2
MAX_STEPS = 1024
STATS = ("n_frames", "n_kept", "n_dropped", "n_gone", "n_protected", "n_needed", "n_blocked", "n_empty")
KEYS = ("verdict", "n_rows", "keep", "step", "order", "seen", "red")
FAULTS = ("tie_to_highest", "float_share", "counts_not_updated")


def gap_ok(live, f, max_gap):
    F = len(live)
    a = f - 1
    while a >= 0 and not live[a]:
        a -= 1
    b = f + 1
    while b < F and not live[b]:
        b += 1
    return b - a - 1 <= max_gap


def state(B, live, min_observers):
    """(cnt per entry, red per frame) for the live frames `live`; red of a frame that is not live is 0"""
    cnt = B[live].sum(0).astype(np.int64)
    red = (B & (cnt - 1 >= min_observers)[None, :]).sum(1).astype(np.int64)
    return cnt, np.where(live, red, 0)


def tests(f, flags, live, seen, red, min_seen, share_permille, max_gap):
    """(free and live, seen enough, share passes, gap passes) of frame f"""
    return (flags[f] == FREE and bool(live[f]), int(seen[f]) >= min_seen, 1000 * int(red[f]) >= share_permille * int(seen[f]),
            max_gap <= 0 or gap_ok(live, f, max_gap))


def run(bits, flags=None, min_observers=3, share_permille=900, min_seen=1, max_gap=0, max_dropped=MAX_STEPS, n_rows=None, n_max=0, fault=None):
    """dict(verdict, n_rows, keep, step, order, seen, red, stats, candidates: per step the list of candidate frames -- one more
    list than drops when the loop ended for lack of a candidate)"""
    B = V.unpack_bits(bits)
    F = len(B)
    flags = np.zeros(F, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    gone = flags == GONE
    B = B & ~gone[:, None]                                    # a GONE frame's row is ignored
    rows_in = np.full(F, int(n_max), np.int32) if n_rows is None else np.asarray(n_rows, np.int32)
    seen = B.sum(1).astype(np.int64)
    live = ~gone
    counted = live.copy()                                     # (fault counts_not_updated: the counts keep the dropped rows)
    step = np.full(F, -1, np.int32)
    order = np.full(F, -1, np.int32)
    seen_out, red_out = np.zeros(F, np.int32), np.zeros(F, np.int32)
    history, k = [], 0
    while k < max_dropped:
        _, red = state(B, counted, min_observers)
        cand = [f for f in range(F) if all(tests(f, flags, live, seen, red, min_seen, share_permille, max_gap))]
        history.append(cand)
        if not cand:
            break
        if fault == "float_share":
            key = [np.float32(red[f]) / np.float32(seen[f]) for f in cand]
            best = cand[int(np.argmax(key))]                  # the first of the equal float shares
        else:
            best = cand[0]
            for f in cand[1:]:                                # the highest share by cross-multiplication; ties: the lowest frame
                l, r = int(red[f]) * int(seen[best]), int(red[best]) * int(seen[f])
                if l > r or (fault == "tie_to_highest" and l == r):
                    best = f
        step[best], order[k] = k, best
        seen_out[best], red_out[best] = seen[best], red[best]
        live[best] = False
        if fault != "counts_not_updated":
            counted[best] = False
        k += 1
    _, red = state(B, counted, min_observers)
    red = np.where(live, red, 0)
    verdict = np.zeros(F, np.int32)
    for f in range(F):
        free, enough, share, gap = tests(f, flags, live, seen, red, min_seen, share_permille, max_gap)
        verdict[f] = (GONE if gone[f] else DROPPED if step[f] >= 0 else PROTECTED if flags[f] != FREE else EMPTY if not enough
                      else NEEDED if not share else GAP if not gap else LEFT)
        if step[f] < 0:
            seen_out[f], red_out[f] = seen[f], red[f]
    out = (verdict == GONE) | (verdict == DROPPED)
    count = lambda *v: int(np.isin(verdict, v).sum())
    stats = dict(n_frames=F, n_kept=F - count(DROPPED, GONE), n_dropped=count(DROPPED), n_gone=count(GONE), n_protected=count(PROTECTED),
                 n_needed=count(NEEDED), n_blocked=count(GAP, LEFT), n_empty=count(EMPTY))
    return dict(verdict=verdict, n_rows=np.where(out, 0, rows_in).astype(np.int32), keep=(~out).astype(np.uint8), step=step, order=order,
                seen=seen_out, red=red_out, stats=stats, candidates=history)


def compare(a, b):
    """the keys in which two results differ: what the GPU test asserts to be empty"""
    return [k for k in KEYS if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()] + (["stats"] if a["stats"] != b["stats"] else [])


def monotone(r):
    """rule 6 on a run's history: a frame that is no candidate at a step is none at any later step"""
    for k in range(1, len(r["candidates"])):
        if not set(r["candidates"][k]) <= set(r["candidates"][k - 1]):
            return False
    return True


def replay(bits, r, flags=None, min_observers=3, share_permille=900, min_seen=1, max_gap=0, max_dropped=MAX_STEPS):
    """Verifies a result from its outputs alone (order, step, seen, red, verdict, keep): at every step the dropped frame passes
    every test on counts recomputed from scratch, no candidate goes before it, and its recorded seen / red are those of that step;
    after the last drop either the budget is spent or no candidate is left, and the verdicts are those of the final state.
    Returns the list of complaints (empty: the result obeys the rules)."""
    B = V.unpack_bits(bits)
    F = len(B)
    flags = np.zeros(F, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    gone = flags == GONE
    B = B & ~gone[:, None]
    seen = B.sum(1).astype(np.int64)
    live = ~gone
    bad = []
    drops = [int(f) for f in r["order"] if f >= 0]
    if len(drops) > max_dropped or sorted(drops) != sorted(np.nonzero(r["step"] >= 0)[0].tolist()) or (np.asarray(r["order"])[len(drops):] != -1).any():
        bad.append("order")
    for k, f in enumerate(drops):
        _, red = state(B, live, min_observers)
        if r["step"][f] != k or not all(tests(f, flags, live, seen, red, min_seen, share_permille, max_gap)):
            bad.append(f"step {k}: frame {f} is no candidate")
        if r["seen"][f] != seen[f] or r["red"][f] != red[f]:
            bad.append(f"step {k}: record of frame {f}")
        for g in range(F):
            if g != f and all(tests(g, flags, live, seen, red, min_seen, share_permille, max_gap)):
                l, m = int(red[g]) * int(seen[f]), int(red[f]) * int(seen[g])
                if l > m or (l == m and g < f):
                    bad.append(f"step {k}: frame {g} goes before {f}")
        live[f] = False
    _, red = state(B, live, min_observers)
    left = [f for f in range(F) if all(tests(f, flags, live, seen, red, min_seen, share_permille, max_gap))]
    if left and len(drops) < max_dropped:
        bad.append("candidates left with budget to spare")
    for f in range(F):
        free, enough, share, gap = tests(f, flags, live, seen, red, min_seen, share_permille, max_gap)
        v = (GONE if gone[f] else DROPPED if f in drops else PROTECTED if flags[f] != FREE else EMPTY if not enough else NEEDED if not share
             else GAP if not gap else LEFT)
        if r["verdict"][f] != v or r["keep"][f] != (v not in (GONE, DROPPED)):
            bad.append(f"verdict of frame {f}")
        if f not in drops and (r["seen"][f] != seen[f] or r["red"][f] != (0 if gone[f] else red[f])):
            bad.append(f"final seen / red of frame {f}")
    return bad
