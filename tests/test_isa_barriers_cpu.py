"""Build-time guard for the barrier structure of the pipelined two-product kernels (csrc/gcr_pairs_loop.h): the gfx950
assembly of every instantiation is scanned (scripts/exp/check_barrier_waits.py) for
  * an LDS instruction between the last `s_waitcnt lgkmcnt(0)` and an `s_barrier` (a ring slot re-used too early), and
  * in the 512-thread form, a barrier that sits inside an EXEC-masked (possibly divergent) region: the two wave groups' extra
    barriers are only sound under branches the compiler has proven uniform (s_cbranch_scc* / vcc*).
A compiler change that breaks either shows up here, in the CPU suite, instead of as a hang on the GPU box.

The checker examines infonce_pipe_kernel only.  Its instantiations are made by two translation units,
csrc/gcr_infonce_flash.hip and csrc/gcr_bce.hip; csrc/gcr_infonce.hip, the third unit built on the same headers, holds none
(its 512-thread infonce_fwd_e_kernel has one barrier per tile outside any group-dependent branch and is NOT examined, as
before the source was split).  All three are compiled and scanned, and which of them hold a 512-thread infonce_pipe_kernel
is read from the assembly itself, so no such kernel goes unscanned when an instantiation moves."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recommendation_amd", "csrc")
UNITS = ("gcr_infonce.hip", "gcr_infonce_flash.hip", "gcr_bce.hip")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_pipe_kernel_barriers_are_waited_for_and_uniformly_guarded(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # every unit that includes the kernel templates is one of UNITS
    users = {f for f in os.listdir(CSRC) if f.endswith(".hip") and "gcr_pairs" in open(os.path.join(CSRC, f)).read()}
    assert users == set(UNITS)
    procs = []
    for unit in UNITS:
        asm = tmp_path / (unit[:-4] + ".s")
        cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
               "-I", CSRC, os.path.join(CSRC, unit), "-o", str(asm)]
        procs.append((unit, asm, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    pipe_kernels, eight_wave_units, fwd_e_eight = 0, [], 0
    for unit, asm, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out[-2000:]
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "exp", "check_barrier_waits.py"), str(asm)],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert chk.returncode == 0, (unit, chk.stdout)
        labels = re.findall(r"^(_Z\w+):", asm.read_text(), flags=re.M)
        pipe_kernels += sum("infonce_pipe_kernel" in l for l in labels)
        fwd_e_eight += sum("infonce_fwd_e_kernel" in l and l.rstrip("_").find("ELi8EE") >= 0 for l in labels)
        if any("infonce_pipe_kernel" in l and l.rstrip("_").find("ELi8EE") >= 0 for l in labels):
            eight_wave_units.append(unit)
            # the scan did find (and pass) the guarded barriers
            assert "'barriers_in_8wave_branches'" in chk.stdout, (unit, chk.stdout)
    assert eight_wave_units, "no unit holds a 512-thread infonce_pipe_kernel"
    assert pipe_kernels == 46 and fwd_e_eight == 1                      # every instantiation of the loop was scanned
