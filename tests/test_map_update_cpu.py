"""tests/map_update_cases.py on the CPU: the numpy restatement of map_hash / map_home_slot against the host build of vo_math.h
(the definitions map.hip compiles), bit for bit; every property the builders claim; cut_update against the literal double loop
cut the same way.  Without the first of these the adversarial rows of tests/test_gpu_map_update.py could lose their power
(a changed hash makes them ordinary rows) without any test noticing."""
import ctypes as C

import numpy as np

import map_update_cases as U
from oracle import vo_pipeline as P
from test_hostcheck import hc, p  # noqa: F401  (the fixture that builds tests/hostcheck)


def _odd_rows(rng, n):
    """rows of every kind of float: ordinary, +-0, subnormals, +-inf, huge and tiny magnitudes, NaNs, raw bit patterns"""
    a = rng.uniform(-1, 1, (n, 10)).astype(np.float32)
    kind = rng.integers(0, 12, (n, 10))
    a[kind == 0] = np.float32(0.0)
    a[kind == 1] = np.float32(-0.0)
    sub = (rng.integers(1, 1 << 23, (n, 10)).astype(np.uint32) | (rng.integers(0, 2, (n, 10)).astype(np.uint32) << np.uint32(31))).view(np.float32)
    a[kind == 2] = sub[kind == 2]
    a[kind == 3] = np.where(rng.random((n, 10)) < 0.5, np.float32(np.inf), np.float32(-np.inf))[kind == 3]
    a[kind == 4] = (rng.uniform(-1, 1, (n, 10)) * 3e38).astype(np.float32)[kind == 4]
    a[kind == 5] = (rng.uniform(-1, 1, (n, 10)) * 1e-37).astype(np.float32)[kind == 5]
    raw = rng.integers(0, 1 << 32, (n, 10), dtype=np.uint64).astype(np.uint32).view(np.float32)
    rows = rng.random(n) < 0.05                                  # whole rows of raw bits: NaN patterns among them
    a[rows] = raw[rows]
    a[rng.random(n) < 0.02, 7] = np.nan
    return a


def test_restatement_equals_the_host_build_bit_for_bit(hc):
    rng = np.random.default_rng(71)
    n = 100000
    a = _odd_rows(rng, n)
    a[:1000, :] = np.where(rng.random((1000, 10)) < 0.5, np.float32(0.0), np.float32(-0.0))     # rows of zeros of either sign
    assert np.isinf(a).any() and np.isnan(a).any() and (a == 0).any()
    assert ((np.abs(a) < 1.17e-38) & (a != 0)).any() and (np.abs(a[np.isfinite(a)]) > 1e38).any()
    h = np.zeros(n, np.uint32); nan = np.zeros(n, np.int32)
    hc.hc_map_hash(p(a), C.c_int(n), p(h), p(nan))
    assert np.array_equal(h, U.map_hash(a))
    assert np.array_equal(nan != 0, U.has_nan(a))
    assert len(set(h[:1000].tolist())) == 1                      # -0 hashes as +0
    for tmask in (0xFFF, 0x3FFF, 0xFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 1023):
        s = np.zeros(n, np.uint32)
        hc.hc_map_home_slot(p(h), C.c_int(n), C.c_uint32(tmask), p(s))
        assert np.array_equal(s, U.map_home_slot(h, tmask))
    # the table's word order: unequal rows of the builders are unequal for the host build's operator== too
    fam = U.tag_family(rng, 5)
    for i in range(5):
        for j in range(5):
            assert hc.hc_map_rows_equal(p(fam[i]), p(fam[j])) == (1 if i == j else 0)
    assert hc.hc_map_rows_equal(p(fam[0]), p(U.flip_zeros(fam)[0])) == 1
    assert hc.hc_map_rows_equal(p(U.nan_copy(fam)[0]), p(U.nan_copy(fam)[0])) == 0


def test_builders_keep_what_they_promise():
    rng = np.random.default_rng(72)
    for K in (4, 6, 17):
        fam = U.tag_family(rng, K)
        assert fam.shape == (K, 10) and fam.dtype == np.float32
        U.check_family(fam)
        U.check_zero_flip(fam, U.flip_zeros(fam))
        nc = U.nan_copy(fam)
        assert U.has_nan(nc).all() and (np.isnan(nc).sum(axis=1) == 1).all()
        assert (nc[:, :U.NAN_AT] == fam[:, :U.NAN_AT]).all() and (nc[:, U.NAN_AT + 1:] == fam[:, U.NAN_AT + 1:]).all()
    fams = [U.tag_family(rng, 4) for _ in range(20)]
    assert len({int(U.map_hash(f)[0]) for f in fams}) == 20      # families differ from each other
    for n in (32, 40):
        ch = U.slot_chain(rng, n)
        U.check_chain(ch)
        U.check_zero_flip(ch, U.flip_zeros(ch))
        wr = U.wrap_chain(rng, n)
        U.check_chain(wr, wrap=True)
        U.check_zero_flip(wr, U.flip_zeros(wr))
        # what the wrap means: n rows probing linearly from one of the last 8 slots claim slots over the end of every table size
        for lg in range(U.LOG_T_MIN, U.LOG_T_MAX + 1):
            tcap = 1 << lg
            taken = set()
            for s in U.map_home_slot(U.map_hash(wr), tcap - 1).tolist():
                while s in taken:
                    s = (s + 1) & (tcap - 1)
                taken.add(s)
            assert 0 in taken and tcap - 1 in taken
    # the properties are properties: a family with one foreign row, a chain with a stray, are told apart
    bad = U.tag_family(rng, 4); bad[3, 0] += np.float32(0.5)
    stray = np.concatenate([U.slot_chain(rng, 32)[:31], U.tag_family(rng, 4)[:1]])
    for check, rows in ((U.check_family, bad), (U.check_chain, stray)):
        try:
            check(rows)
        except AssertionError:
            continue
        raise AssertionError("a broken case passed its check")


def test_cut_update_equals_the_literal_loops_cut():
    rng = np.random.default_rng(73)
    fam = U.tag_family(rng, 6)
    ch = U.slot_chain(rng, 32)
    pool = np.concatenate([np.round(rng.uniform(-1, 1, (120, 10)), 1).astype(np.float32), fam, U.flip_zeros(fam), ch, U.nan_copy(fam)])
    for cap in (40, 97, 10 ** 6):
        m = P.Map()
        lit_p, lit_a = [], []
        total = 0
        for step in range(6):
            n = [30, 50, 1, 80, 0, 64][step]
            app = pool[rng.integers(0, len(pool), n)]
            pts = rng.normal(0, 1, (n, 3)).astype(np.float32)
            cut = U.cut_update(m, pts, app, cap)
            P.literal_update(lit_p, lit_a, list(pts), list(app))
            lit_cut = max(0, len(lit_p) - cap)
            del lit_p[cap:]; del lit_a[cap:]
            assert cut == lit_cut
            total += cut
            assert len(m.pts) == len(lit_p) <= cap
            assert np.array(m.pts, np.float32).tobytes() == np.array(lit_p, np.float32).tobytes()
            assert np.array(m.app, np.float32).tobytes() == np.array(lit_a, np.float32).tobytes()
        assert (total > 0) == (cap < 10 ** 6)
