"""A solve in the fast mode gathers its correspondences in its first round (picp_gather_round_kernel) instead of a gather
launch and a memset of its own in front of the rounds; VO_PICP_GATHER=0 keeps the separate launches.  Same arithmetic on the
same values by construction: pose, H, b, both chi sums, the inlier count and the bad-index error must agree BIT FOR BIT
between the two routes -- around the workgroup and grid-cap edges, with and without outliers kept, for the pinhole and the
general camera, for one round (the finishing launch takes the tally of dropped pairs), two and nine, for host pairs and for
device pairs with a device count below the array length behind a pending pose reset."""
import json
import os
import subprocess
import sys

import pytest

import gather_cases as cases

pytestmark = pytest.mark.gpu

VO_ERR_BAD_INDEX = -5


@pytest.fixture(scope="module")
def runs():
    res = {}
    for gather in ("1", "0"):
        env = dict(os.environ, VO_PICP_GATHER=gather)
        r = subprocess.run([sys.executable, cases.__file__], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[gather] = json.loads(r.stdout.strip().splitlines()[-1])
    return res


@pytest.mark.parametrize("keep", ["drop", "keep"])
@pytest.mark.parametrize("camera", ["pinhole", "general"])
@pytest.mark.parametrize("n", cases.SIZES)
def test_gathering_round_equals_the_separate_gather(runs, n, camera, keep):
    key = "%d/%s/%s/" % (n, camera, keep)
    fused = {k[len(key):]: v for k, v in runs["1"].items() if k.startswith(key)}
    apart = {k[len(key):]: v for k, v in runs["0"].items() if k.startswith(key)}
    assert len(fused) == 2 * len(cases.ITERS) + 4 and fused.keys() == apart.keys()
    for name in fused:
        assert fused[name] == apart[name], (key, name)
    assert fused["solve9"] == fused["rounds9"]                  # one call of nine rounds = nine calls of one (the separate gather)
    for name in ("bad", "bad1"):
        assert fused[name][0] == "error" and fused[name][1] == VO_ERR_BAD_INDEX and "3 correspondence" in fused[name][2], fused[name]
    assert all(v[0] != "error" for k, v in fused.items() if not k.startswith("bad"))
