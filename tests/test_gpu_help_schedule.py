"""The hand-off between helper waves and the problems' own workgroups in the batched solver's shared form (csrc/picp.hip,
picp_batch_shared_kernel) under SCRIPTED late and absent waves.  The design's claim: whichever wave ends
up computing a chunk, and whenever, not a bit of the result changes, and every wait ends.  VO_PICP_HELP_SCHEDULE takes the
kernel's instantiation with the scheduling hooks and makes chosen waves late or absent in a fixed order of events (no clock,
no second kernel holding CUs); vo_picp_batch_help_info reads back what happened.  The reference of every case is the same
call on the product instantiation with no schedule set.

The worker (tests/help_schedule_cases.py) is ONE child process that runs all schedules and prints one JSON line; it is
started once, under a timeout that is a cap (a stuck call fails the test instead of stalling the suite), not a measurement.
When it expires or the child fails, every test here fails and nothing is started again.
Measured on an MI355X: the worker takes 0.5 s for its 276 solver calls and two frames calls (0.4 s of it the solver calls;
context creation and imports not counted), this file 1.4 s under pytest.

Problem sets (picp_cases.Batch, 30 000 pairs per frame, 12 rounds): 24 equal problems, 3 equal problems, 40 ragged sizes
(0, 3, both sides of every multiple of a trip a home may keep, whole problems; a trip is 3072 pairs).  Asserted from the chunk counts read back:
some problem has more than 32 chunks (bits of s_late[1]), some an odd number (the last pair of rows a home wave polls in its
two half-waves has one half without a row), some none; the ragged set has problems longer than 3 pairs on both sides of
what a home keeps, one of them with a single chunk.

What every case asserts
 1. poses and the four statistics of every problem equal the reference's BYTE FOR BYTE, and the call ran as form 4;
 2. the script did what it says.  Chunk j of problem p belongs to helper wave g = row0(p) + j of the launch, row0 the
    exclusive prefix sum of the chunk counts read back (the kernel's s_chunkpre).  sched(p) = { j : g % mod == rem }.
    leave (mod, rem, R):  a scheduled wave returns at the head of round R, so its row of round R never exists; the home polls
      HELP_POLLS_HOME times in round R and sets the chunk's `own` bit (if it had not before).  Hence own >= sched(p).  A bit
      outside sched(p) needs a wave that was late by itself; in the equal-size sets, where every wave has the chunk length the
      partition was sized for, own == sched(p) exactly.  Every scheduled wave leaves once (counted at its return, or earlier
      had it fallen behind by itself), a wave outside the script leaves early only if it fell behind by itself, which gives
      it an `own` bit: |sched(p)| <= left <= |sched(p)| + |own minus sched(p)|, i.e. left == |sched(p)| in the equal sets.
    stall (mod, rem, R):  a scheduled wave computes round R and stores its row only once the pose word carries tag
      min(R + 2, rounds), which the home writes after round min(R + 1, rounds - 1): the home has finished round R without
      the row, so own >= sched(p) as above.  If R is not the last round, the wave then polls for the pose of round R + 1,
      finds a tag beyond it and leaves: left as for leave.  If R is the last round, the wave's loop ends with the store and
      it does not leave early: left == 0 in the equal sets (<= |own minus sched(p)| in general).
    home-stall (mod, rem, R >= 1):  a scheduled home (p % mod == rem) that has chunks holds the pose of round R back until
      its count of leavers has reached its chunk count: every helper wave of the problem polls for that pose (64 polls), finds
      none and leaves -- or had left before, counted as well -- and no wave can have finished, since finishing needs the
      pose of round R.  So left == chunk count exactly.  In round R no row arrives: own == all chunk-count bits.
 3. with VO_PICP_HELP_ABSENT=1 (hooks instantiation, nothing scheduled) every `own` mask is full and nobody left early
    (the waves return before their loop);
 4. in the "none" case the masks are read but not asserted: they depend on timing.
For the instantiations that keep outliers the threshold (2.0) really leaves outliers: asserted from the reference's
chi_outliers and inlier counts, so that a wrong stand-in of the statistics round would show there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import help_schedule_cases as cases

pytestmark = pytest.mark.gpu

TIMEOUT_S = 300          # a cap, not a measurement


@pytest.fixture(scope="module")
def run():
    env = {k: v for k, v in os.environ.items() if k not in cases.ENV}
    r = subprocess.run([sys.executable, cases.__file__], capture_output=True, text=True, env=env, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("help_schedule worker: %.1f s in all, %.1f s in the %d solver calls" % (out["wall_s"], out["wall_solver_s"],
                                                                                 len(out["cases"]) + len(out["ref"])))
    return out


def popcount(x):
    return bin(int(x)).count("1")


def scheduled_masks(nchunk, mod, rem):
    row0 = np.concatenate([[0], np.cumsum(nchunk)[:-1]])
    return [sum(1 << j for j in range(int(k)) if (int(r0) + j) % mod == rem) for r0, k in zip(row0, nchunk)]


def check_script(rec, sch, equal, iters):
    """point 2 and 3 of the module docstring for one call's record"""
    mode, mod, rem, rnd = sch
    own, nchunk, left = rec["own"], rec["nchunk"], rec["left"]
    full = [(1 << k) - 1 for k in nchunk]
    print(mode, mod, rem, rnd, "nchunk", nchunk, "own", [hex(x) for x in own], "left", left)
    if mode == "none":
        return
    if mode == "absent":
        assert own == full and not any(left)
        return
    if mode == "home-stall":
        for p, k in enumerate(nchunk):
            if p % mod == rem:
                assert own[p] == full[p] and left[p] == k, (p, hex(own[p]), left[p], k)
        return
    sched = scheduled_masks(nchunk, mod, rem)
    for p in range(len(nchunk)):
        assert own[p] & ~full[p] == 0 and own[p] & sched[p] == sched[p], (p, hex(own[p]), hex(sched[p]))
        if equal:
            assert own[p] == sched[p], (p, hex(own[p]), hex(sched[p]))
        leavers = 0 if (mode == "stall" and rnd == iters - 1) else popcount(sched[p])
        assert leavers <= left[p] <= leavers + popcount(own[p] & ~sched[p]), (p, left[p], leavers, hex(own[p]), hex(sched[p]))


def test_sets_reach_the_edges(run):
    """more than 32 chunks, an odd count, none -- from the counts read back; the ragged set on both sides of a home's keep"""
    counts = {s: run["cases"][cases.case_name(s, "pinhole-drop", ("none", 1, 0, 0))]["nchunk"] for s in cases.SETS}
    print(counts)
    assert max(counts["p3"]) > 32
    assert any(k % 2 == 1 for k in counts["p24"] + counts["p3"] + counts["ragged"])
    assert any(k == 0 for k in counts["ragged"])
    sizes = run["sizes"]["ragged"]
    assert any(k == 0 and n > 3 for k, n in zip(counts["ragged"], sizes)) and any(k == 1 for k in counts["ragged"])
    for inst in cases.INSTANCES:                 # the partition is a function of the sizes alone
        for s in cases.SETS:
            for sch in cases.schedules(inst):
                assert run["cases"][cases.case_name(s, inst, sch)]["nchunk"] == counts[s]


@pytest.mark.parametrize("inst", [i for i in cases.INSTANCES if i.endswith("keep")])
@pytest.mark.parametrize("s", list(cases.SETS))
def test_keep_threshold_leaves_outliers(run, s, inst):
    ref = run["ref"]["%s/%s" % (s, inst)]
    S = np.frombuffer(bytes.fromhex(ref["S"]), np.float32).reshape(-1, 4)
    sizes = np.array(run["sizes"][s])
    big = sizes >= 1000
    print(S[big])
    assert big.any() and (S[big, 1] > 0).all() and (S[big, 2] < sizes[big]).all() and (S[big, 2] > 0).all()


@pytest.mark.parametrize("s,inst,sch", cases.all_cases(), ids=[cases.case_name(*c) for c in cases.all_cases()])
def test_schedule(run, s, inst, sch):
    rec, ref = run["cases"][cases.case_name(s, inst, sch)], run["ref"]["%s/%s" % (s, inst)]
    assert ref["form"] == 4 and rec["form"] == 4 and rec["wgs"] == ref["wgs"] > len(run["sizes"][s])
    assert rec["T"] == ref["T"], "poses differ from the undisturbed call"
    assert rec["S"] == ref["S"], "statistics differ from the undisturbed call"
    check_script(rec, sch, s in cases.EQUAL, cases.ITERS)


def test_frames_call_under_a_schedule(run):
    """vo_frames_batch_dev, 40 frames x 20 000 points, leave (2, 1) at round 1 in its solver stage: poses, statistics and
    counts byte for byte those of the undisturbed call; every frame joins all its points, so the set is an equal-size one"""
    ref, rec = run["frames"]["ref"], run["frames"]["leave"]
    assert ref["form"] == 4 and rec["form"] == 4 and rec["wgs"] == ref["wgs"] > 40
    for k in ("T", "S", "counts"):
        assert rec[k] == ref[k], k
    assert len(set(rec["n_joined"])) == 1 and sum(rec["nchunk"]) > 0
    check_script(rec, ("leave", 2, 1, 1), True, 20)
