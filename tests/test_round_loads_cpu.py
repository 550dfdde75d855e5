"""The partial-row fetch at the head of a PICP round (picp_round_body, step (1)) is eight independent 16-B loads per thread
and pass of 256 rows.  They cost ONE memory round trip only if all eight are issued before the wave first waits on a vector
load: a wave issues in order, so a wait in front of load 3 chains a second trip behind the first.  This reads
the order out of the assembly hipcc produces for gfx950 with the library's own flags; nothing else about the instruction
stream is asserted.  (Before the scheduling barrier between the loads and their adds every kernel below had two.)"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "visual-odometry_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")


def makefile_flags():
    """CXXFLAGS as csrc/Makefile expands them (so a change of the build's flags is followed)"""
    out = subprocess.check_output(["make", "-s", "-C", CSRC, "--no-print-directory", "--eval=print-cxxflags: ; @echo $(CXXFLAGS)",
                                   "print-cxxflags"], text=True)
    flags = out.split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


def kernel_bodies(asm):
    """{mangled name: [instruction lines]} of every kernel (an .amdhsa_kernel directive names them) in a device assembly"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    bodies, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m and m.group(1) in names:
            cur = bodies.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        s = line.split(";", 1)[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s and not s.startswith(".") and not s.endswith(":"):
            cur.append(s)
    return bodies


def reads_partial_rows(name):
    """the instantiations that run step (1): picp_round_kernel<PRE = true, ...>, picp_round_batch_kernel<PRE = true, ...> and
    every picp_tally_round_kernel (PRE is fixed to true there; its first flag is FINISH)"""
    for k in ("picp_round_kernel", "picp_round_batch_kernel"):
        if re.search(r"\d+" + k + "ILb1E", name):
            return True
    return re.search(r"\d+picp_tally_round_kernelILb[01]E", name) is not None


def row_loads_before_first_wait(body):
    n = 0
    for ins in body:
        if ins.startswith("s_waitcnt") and "vmcnt" in ins:
            return n
        if ins.startswith("global_load_dwordx4"):
            n += 1
    return n


@pytest.fixture(scope="module")
def picp_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("picp_asm") / "picp.s")
    subprocess.check_call([HIPCC, *makefile_flags(), "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "picp.hip")])
    with open(out) as f:
        return f.read()


def test_all_row_loads_of_a_pass_are_issued_before_the_first_wait(picp_asm):
    bodies = {k: v for k, v in kernel_bodies(picp_asm).items() if reads_partial_rows(k)}
    counts = {k: row_loads_before_first_wait(v) for k, v in bodies.items()}
    for k in sorted(counts):
        print(f"{counts[k]:2d} row loads before the first vmcnt wait, {len(bodies[k]):5d} instructions: {k}")
    # 4 camera / outlier forms + FINISH of the round kernel, 4 + 1 of the tally kernel, the batch kernel's forms
    assert sum("picp_round_kernelILb1E" in k for k in counts) >= 5, sorted(counts)
    assert sum("picp_tally_round_kernel" in k for k in counts) >= 5, sorted(counts)
    assert sum("picp_round_batch_kernelILb1E" in k for k in counts) >= 1, sorted(counts)
    short = {k: c for k, c in counts.items() if c < 8}
    assert not short, short
