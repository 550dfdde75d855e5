"""picp_round_body keeps arithmetic, operand order and summation order when its instruction stream is rearranged (the
pose-independent work moved ahead of the first wait, the staging in an LDS array of its own, the straight-line linearisation
where the grid covers the call): every solve returns the bytes recorded in tests/golden/picp_round_bits.json, which
tools/round_bits.py wrote on the commit named in that file, before the rearrangement.

Cases of tests/picp_cases.py as tests/test_gpu_round_rows.py selects them: 257 pairs (2 partial rows), 8 193 (33 rows, a
partial row group), 65 537 (a second pass of 256 rows) and 300 001 (the grid cap, threads loop: not the straight-line path);
1, 2 and 18 rounds each (gathering round -> tally round -> plain rounds and the wrap of the 16-slot ring).  Pose, H, b, the
chi^2 sums and the inlier count are compared as bytes; any differing byte fails.  (256 pairs and below take the one-launch
form, which test_gpu_more.py::test_small_problem_form_equals_the_round_kernels holds to the round kernels.)"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import round_bits as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(rb.FIXTURE) as f:
        rec = json.load(f)
    assert len(rec["commit"]) == 40, rec["commit"]
    assert tuple(rec["sizes"]) == rb.SIZES and tuple(rec["rounds"]) == rb.ROUNDS, (rec["sizes"], rec["rounds"])
    return rec


@pytest.mark.parametrize("n", rb.SIZES, ids=[f"{n}-pairs" for n in rb.SIZES])
def test_round_bits_are_the_recorded_ones(vo, ctx, recorded, n):
    got = rb.solve_bits(vo, ctx, n)
    want = recorded["cases"][str(n)]
    diff = []
    for k in rb.ROUNDS:
        g, w = got[str(k)], want[str(k)]
        assert sorted(g) == sorted(w) == ["H", "T", "b", "chi_in", "chi_out", "n_in"]
        for key in sorted(w):
            same = g[key] == w[key]
            print(f"{n} pairs, {k} rounds, {key}: {'same bytes' if same else 'DIFFERS ' + g[key] + ' recorded ' + w[key]}")
            if not same:
                diff.append((k, key))
    assert not diff, f"{n} pairs: bytes differ from those of commit {recorded['commit'][:12]} in (rounds, array) {diff}"
