"""A PICP round is one dependency chain (rows home -> sums -> solve -> linearisation -> reduction -> row stored) on a CU that
runs one wave per SIMD: every instruction behind the first wait on a partial row costs its issue latency on that chain, so
what depends on the thread index and the arguments alone belongs in front of that wait (picp_round_body).  Left
alone the compiler sinks it next to its use.  This reads, out of the assembly hipcc produces for gfx950 with the library's own
flags (the model is test_round_loads_cpu.py: same flags, same kernels):

  * no scalar load behind the first wait on a vector load: the parameter block is fetched under the rows, not after them;
  * three workgroup barriers in a round that linearises (staging, two of the reduction): the staging of the row sums has an
    LDS array of its own, and the barrier that let the reduction reuse it is gone;
  * no scratch, and less LDS than the 37 904 B of the layout in which the reduction's rows held one row per THREAD.

Printed per kernel (for DESIGN 4.1's table): the instructions listed between the last v_readlane_b32 -- the new pose
leaving the lanes that composed it -- and the first v_rcp_f32 behind it -- the projection of the linearisation --, VGPRs,
LDS and scratch bytes."""
import os
import re
import subprocess

import pytest

from test_round_loads_cpu import CSRC, HIPCC, kernel_bodies, makefile_flags, reads_partial_rows

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")

PARENT_LDS = 37904          # bytes of picp_round_kernel<true, false, ...> before the staging got its own array


def kernel_resources(asm):
    """{mangled name: {vgpr, sgpr, lds, scratch, spills}} from the amdhsa.kernels metadata of a device assembly"""
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"^  - (?=\.agpr_count:)", meta, flags=re.M)[1:]:
        def field(key, blk=blk):
            return int(re.search(r"^\s*\." + key + r":\s+(\d+)", blk, re.M).group(1))
        name = re.search(r"^\s*\.name:\s+(\S+)", blk, re.M).group(1)
        out[name] = dict(vgpr=field("vgpr_count"), sgpr=field("sgpr_count"), lds=field("group_segment_fixed_size"),
                         scratch=field("private_segment_fixed_size"), spills=field("vgpr_spill_count") + field("sgpr_spill_count"))
    return out


def finishes(name):
    """FINISH is the second flag of picp_round_kernel / picp_round_batch_kernel and the first of picp_tally_round_kernel"""
    if "picp_tally_round_kernel" in name:
        return re.search(r"picp_tally_round_kernelILb1E", name) is not None
    return re.search(r"kernelILb1ELb1E", name) is not None


def scalar_loads_behind_first_wait(body):
    seen_wait, late = False, []
    for ins in body:
        if ins.startswith("s_waitcnt") and "vmcnt" in ins:
            seen_wait = True
        elif seen_wait and ins.startswith(("s_load_", "s_buffer_load_")):
            late.append(ins)
    return late


def pose_to_projection(body):
    """instructions listed between the last v_readlane_b32 and the first v_rcp_f32 behind it, or None without such a pair"""
    lanes = [k for k, ins in enumerate(body) if ins.startswith("v_readlane_b32")]
    if not lanes:
        return None
    rcps = [k for k, ins in enumerate(body) if ins.startswith("v_rcp_f32") and k > lanes[-1]]
    return rcps[0] - lanes[-1] - 1 if rcps else None


@pytest.fixture(scope="module")
def picp_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("picp_chain_asm") / "picp.s")
    subprocess.check_call([HIPCC, *makefile_flags(), "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "picp.hip")])
    with open(out) as f:
        return f.read()


def test_pose_independent_work_is_off_the_round_chain(picp_asm):
    bodies = {k: v for k, v in kernel_bodies(picp_asm).items() if reads_partial_rows(k)}
    res = kernel_resources(picp_asm)
    assert sum("picp_round_kernelILb1E" in k for k in bodies) >= 5, sorted(bodies)
    assert sum("picp_tally_round_kernel" in k for k in bodies) >= 5, sorted(bodies)
    assert sum("picp_round_batch_kernelILb1E" in k for k in bodies) >= 1, sorted(bodies)
    late, barriers, lds, scratch = {}, {}, {}, {}
    for k in sorted(bodies):
        body, r = bodies[k], res[k]
        nbar = sum(ins.startswith("s_barrier") for ins in body)
        gap = pose_to_projection(body)
        print(f"{'finish' if finishes(k) else 'round ':6s} pose -> projection {str(gap):>4s} instructions, {nbar} barriers, {r['vgpr']:3d} VGPRs, {r['sgpr']:3d} SGPRs, "
              f"{r['lds']:5d} B LDS, {r['scratch']} B scratch: {k}")
        if scalar_loads_behind_first_wait(body):
            late[k] = scalar_loads_behind_first_wait(body)
        if not finishes(k) and nbar != 3:
            barriers[k] = nbar
        if r["lds"] >= PARENT_LDS:
            lds[k] = r["lds"]
        if r["scratch"] != 0 or r["spills"] != 0:
            scratch[k] = (r["scratch"], r["spills"])
    assert not late, late
    assert not barriers, barriers
    assert not scratch, scratch
    assert not lds, lds
