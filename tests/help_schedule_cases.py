"""Worker of tests/test_gpu_help_schedule.py: ONE process that runs every scripted schedule of the batched solver's helper
waves (csrc/picp.hip, picp_batch_shared_kernel<.., HOOKS = true>, VO_PICP_HELP_SCHEDULE) on cuda:0 and prints one JSON line:
per case the poses and statistics as bytes, the form the call ran as, and the record the hooks left (per problem: the `own`
mask of its home, its chunk count, the helper waves that left early).  The case list below is shared with the test, which
starts this file once, under a timeout, and asserts on the line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g  # noqa: E402

N, ITERS = 30000, 12
SEED = 7600
ENV = ("VO_PICP_SHARE", "VO_PICP_HELP_KEEP", "VO_PICP_HELP_G", "VO_PICP_HELP_SLACK", "VO_PICP_HELP_ABSENT", "VO_PICP_HELP_SCHEDULE")
# 0, a few, both sides of every multiple of a trip (768 x 4 = 3072 pairs) a home may keep -- at 4 trips, which these sets
# get, down to the float4 group: 12 288 pairs leave no chunk, 12 289 none either (whole groups only), 12 292 one chunk of one
# group, 12 800 one full chunk, 12 804 two --, whole problems
RAGGED = [0, 3, 1000, 3071, 3072, 3076, 6143, 6144, 6148, 9215, 9216, 9217, 9220, 12287, 12288, 12289, 12292, 12293, 12544, 12799,
          12800, 12801, 12804, 13000, 15000, 15359, 15360, 15364, 18431, 18432, 18435, 20000, 22001, 25601, 29999, 10 ** 9, 10 ** 9,
          12292, 3, 0]
SETS = {"p24": [10 ** 9] * 24, "p3": [10 ** 9] * 3, "ragged": RAGGED}
EQUAL = ("p24", "p3")
INSTANCES = ("pinhole-drop", "pinhole-keep", "general-drop", "general-keep")
PAIRS = ((1, 0), (2, 0), (2, 1), (3, 1), (64, 37))
HOME_POLLS = 64          # polls a helper wave of a stalled home has for the withheld pose
# drop: every pair an inlier; keep: a threshold at four times the pixel noise's mean chi^2 (0.5 px per axis), which leaves
# 2-5 % of the pairs as outliers at the converged pose (the test asserts that from the reference call's statistics)
THR = {"drop": 10000.0, "keep": 2.0}


def schedules(inst):
    """(mode, mod, rem, round) of every scheduled case of an instantiation; "none" and "absent" run the hooks instantiation
    with nothing scheduled (absent: with VO_PICP_HELP_ABSENT=1)"""
    full = inst == "pinhole-drop"
    out = [("none", 1, 0, 0), ("absent", 1, 0, 0)]
    for mode in ("leave", "stall"):
        for mod, rem in (PAIRS if full else ((2, 1), (3, 1))):
            for rnd in ((0, 1, 10, 11) if full else (1, 11)):
                out.append((mode, mod, rem, rnd))
    for mod, rem in ((1, 0), (2, 1)):
        for rnd in (1, 11):
            out.append(("home-stall", mod, rem, rnd))
    return out


def case_name(s, inst, sch):
    return "%s/%s/%s-%d-%d-r%d" % ((s, inst) + tuple(sch))


def all_cases():
    return [(s, inst, sch) for s in SETS for inst in INSTANCES for sch in schedules(inst)]


def set_schedule(sch):
    for k in ENV:
        os.environ.pop(k, None)
    if sch is None:
        return
    mode, mod, rem, rnd = sch
    if mode == "absent":
        os.environ["VO_PICP_HELP_ABSENT"] = "1"
    os.environ["VO_PICP_HELP_SCHEDULE"] = "none" if mode in ("none", "absent") else "%s,%d,%d,%d,%d" % (mode, mod, rem, rnd, HOME_POLLS)


def main():
    from picp_cases import Batch, general_K
    vo = g.load_package()
    ctx = vo.Context(0)
    t0 = time.time()
    out = {"cases": {}, "ref": {}, "sizes": {}}
    for s, sizes in SETS.items():
        for cam in ("pinhole", "general"):
            b = Batch(vo, ctx, N, sizes, seed=SEED)
            if cam == "general":
                K = general_K(b.K)
                b.close()
                b = Batch(vo, ctx, N, sizes, seed=SEED, K=K)
            out["sizes"][s] = b.sizes.tolist()
            for policy in ("drop", "keep"):
                inst = cam + "-" + policy

                def call(sch):
                    set_schedule(sch)
                    T, S, form, wgs = b.run(ITERS, THR[policy], policy == "keep")
                    rec = dict(T=T.tobytes().hex(), S=S.tobytes().hex(), form=form, wgs=wgs)
                    if sch is not None:
                        own, nchunk, left = ctx.picp_batch_help_info(b.P)
                        rec.update(own=[int(x) for x in own], nchunk=nchunk.tolist(), left=left.tolist())
                    set_schedule(None)
                    return rec

                out["ref"]["%s/%s" % (s, inst)] = call(None)
                for sch in schedules(inst):
                    out["cases"][case_name(s, inst, sch)] = call(sch)
            b.close()
    out["wall_solver_s"] = time.time() - t0

    # one vo_frames_batch_dev call whose solver stage runs with helper waves (the size of
    # test_gpu_shared.py::test_frames_call_with_helpers_in_its_solver_stage), undisturbed and under leave (2, 1) at round 1
    NF, F, FITERS = 20000, 40, 20
    distinct = [vo.synth.frame_pair(NF, seed=7400 + p) for p in range(5)]
    fps = [distinct[i % 5] for i in range(F)]
    bp = vo.BatchPipeline(ctx, lambda lo, hi: fps[lo:hi], n_iters=FITERS, n_frames=F, upload_block=20)
    frames = {}
    for name, sch in (("ref", None), ("leave", ("leave", 2, 1, 1))):
        set_schedule(sch)
        bp.run()
        ctx.synchronize()
        rec = dict(T=bp.poses().tobytes().hex(), S=bp.stats().tobytes().hex(), counts=bp.counts().tobytes().hex(),
                   n_joined=bp.counts()[1].tolist())
        f_, w_ = C.c_int(), C.c_int()
        assert ctx.lib.vo_picp_batch_info(ctx.h, C.byref(f_), C.byref(w_)) == 0
        rec.update(form=f_.value, wgs=w_.value)
        if sch is not None:
            own, nchunk, left = ctx.picp_batch_help_info(F)
            rec.update(own=[int(x) for x in own], nchunk=nchunk.tolist(), left=left.tolist())
        set_schedule(None)
        frames[name] = rec
    bp.close()
    out["frames"] = frames
    out["wall_s"] = time.time() - t0
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
