"""NumPy restatement of voe_map_covis* and voe_map_window* (include/vo_map_covis.h), written from the header's rules.

Everything is an integer, so every comparison against the device is exact.  sees(f, e) comes from the lookup of
tests/map_localise_restatement.py through tests/map_refine_restatement.observation_lists (the entry per live row of every frame);
the counts are an integer matrix product of the sees-matrix with its transpose; the window is the header's text: candidates,
ranks by (count descending, frame ascending), the union of the free rows, the fixed frames ranked the same way."""
import numpy as np

import map_refine_restatement as R

OUTSIDE, FREE, FIXED = range(3)
OK, NO_FIXED, QUERY_UNSEEN = range(3)


def words_for(size):
    return max((int(size) + 31) // 32, 1)


def sees_matrix(map_app, frames, n_rows=None, n_max=None):
    """(sees (F, M) bool, hits per frame (F,), the entries per frame): frames are [(uv, app)] as in the refinement"""
    M = len(np.asarray(map_app, np.float32).reshape(-1, 10))
    _, _, ents = R.observation_lists(map_app, frames, n_rows=n_rows, n_max=n_max)
    S = np.zeros((len(frames), M), bool)
    hits = np.zeros(len(frames), np.int64)
    for f, ent in enumerate(ents):
        hit = ent[ent >= 0]
        S[f, hit] = True                                      # two rows on one entry see it once
        hits[f] = len(hit)                                    # ... and are two hits
    return S, hits, ents


def pack_bits(S, n_words):
    """bit e & 31 of word e >> 5 of row f is S[f, e]; every other bit of the n_words words is 0"""
    F, M = S.shape
    assert 32 * n_words >= M
    wide = np.zeros((F, 32 * n_words), bool)
    wide[:, :M] = S
    B = (wide.reshape(F, n_words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2)      # (distinct bits: the sum is the OR)
    return B.astype(np.uint32)


def unpack_bits(B):
    B = np.asarray(B, np.uint32)
    return ((B[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(B.shape[:-1] + (32 * B.shape[-1],))


def covis(map_app, frames, n_rows=None, n_max=None, n_words=None, want_counts=True):
    """dict(bits (F, W) uint32, counts (F, F) int32 or None, stats, sees (F, M) bool)"""
    S, hits, _ = sees_matrix(map_app, frames, n_rows, n_max)
    F, M = S.shape
    W = words_for(M) if n_words is None else int(n_words)
    I = S.astype(np.int64)
    C = I @ I.T
    stats = dict(n_frames=F, n_entries=M, n_hits=int(hits.sum()), n_seen=int(np.trace(C)), n_entries_seen=int(S.any(0).sum()))
    return dict(bits=pack_bits(S, W), counts=C.astype(np.int32) if want_counts else None, stats=stats, sees=S)


def ranked(count, eligible):
    """the eligible frames in the order (count descending, frame ascending)"""
    idx = [int(g) for g in np.nonzero(eligible)[0]]
    return sorted(idx, key=lambda g: (-int(count[g]), g))


def window(bits, query, k_free=8, k_fixed=8, min_shared=15, n_rows=None, n_max=0):
    """dict(role, n_rows, fixed, order, union, stats, c, s) -- c and s are the counts the two rankings used"""
    B = unpack_bits(bits)
    F = len(B)
    live = np.full(F, int(n_max), np.int32) if n_rows is None else np.asarray(n_rows, np.int32)
    c = (B & B[query]).sum(1)
    seen = int(B[query].sum())
    role = np.zeros(F, np.int32)
    order = np.full(F, -1, np.int32)
    eligible = (c >= min_shared) & (np.arange(F) != query)
    if seen == 0:
        eligible[:] = False
    cand = ranked(c, eligible)
    free = ([query] + cand[: k_free - 1]) if seen > 0 else []
    role[free] = FREE
    U = np.zeros(B.shape[1], bool)
    for f in free:
        U |= B[f]
    s = (B & U).sum(1)
    fixed_cand = ranked(s, (role != FREE) & (s >= min_shared))
    held = fixed_cand[:k_fixed]
    role[held] = FIXED
    order[: len(free) + len(held)] = free + held
    status = QUERY_UNSEEN if seen == 0 else NO_FIXED if len(held) == 0 else OK
    stats = dict(status=status, n_free=len(free), n_fixed=len(held), n_candidates=len(cand), n_fixed_candidates=len(fixed_cand),
                 n_points=int(U.sum()), query_seen=seen)
    union = pack_bits(U[None, :], np.asarray(bits).shape[1])[0]
    return dict(role=role, n_rows=np.where(role != OUTSIDE, live, 0).astype(np.int32), fixed=(role != FREE).astype(np.uint8), order=order,
                union=union, stats=stats, c=c, s=s)
