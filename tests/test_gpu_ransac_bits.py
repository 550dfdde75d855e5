"""The code both RANSAC front ends share (ransac_common.h: the scoring tile, the mask tail, the scatter, the selection) keeps
every output bit when it is moved or restated: each call returns what tests/golden/ransac_bits.json records, which
tools/ransac_bits.py wrote on the commit named in that file, with each front end still carrying its own copy of those kernels.

Cases (n_hyp, live pairs, n_max) and what is recorded: tools/ransac_bits.py.  Array outputs are compared by the SHA-256 of
their bytes, scalars as they are; a difference in the inputs' hash is reported as that (the input generator changed), before
any output is looked at.  (The batched P3P form is held to the single form bit for bit by
test_gpu_pose_ransac_batch.py::test_bit_identity_at_the_edges.)"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ransac_bits as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(rb.FIXTURE) as f:
        rec = json.load(f)
    assert len(rec["commit"]) == 40, rec["commit"]
    assert sorted(rec["cases"]["epipolar"]) == sorted(map(rb.cid, rb.EPI_CASES))
    assert sorted(rec["cases"]["p3p"]) == sorted(map(rb.cid, rb.POSE_CASES))
    return rec


@pytest.fixture(scope="module")
def data(vo):
    return rb.inputs(vo)


def _compare(front, case, got, want, commit):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    assert got["inputs"] == want["inputs"], f"{front} {case}: the inputs differ from the recorded ones (the generator changed, not a kernel)"
    diff = []
    for key in sorted(want):
        same = got[key] == want[key]
        print(f"{front} {case}, {key}: {'same' if same else 'DIFFERS ' + str(got[key]) + ' recorded ' + str(want[key])}")
        if not same:
            diff.append(key)
    assert not diff, f"{front} {case}: {diff} differ from those of commit {commit[:12]}"


@pytest.mark.parametrize("case", rb.EPI_CASES, ids=rb.cid)
def test_epipolar_bits_are_the_recorded_ones(vo, ctx, recorded, data, case):
    _compare("epipolar", case, rb.epi_bits(vo, ctx, data["epi"], case), recorded["cases"]["epipolar"][rb.cid(case)], recorded["commit"])


@pytest.mark.parametrize("case", rb.POSE_CASES, ids=rb.cid)
def test_p3p_bits_are_the_recorded_ones(vo, ctx, recorded, data, case):
    want = recorded["cases"]["p3p"][rb.cid(case)]
    _compare("p3p", case, rb.pose_bits(vo, ctx, data["pose"], case), want, recorded["commit"])
    if case == (64, 3, 256):
        assert want["status"] != 0 and want["n_pairs"] == 3          # the fallback: every live pair handed on
