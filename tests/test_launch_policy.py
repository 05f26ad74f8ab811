"""The launch policy of the solve kernels (faster_amd/csrc/fh_policy.hpp: a pure host function, no HIP) checked on the CPU by
tests/cpp/test_launch_policy.cpp: the three regimes (alone / beside others / more launches outstanding than hardware queues) for 0, 1, 3,
4 and 13 other launches against 1, 4 and 16 queues and at the boundary others + 1 == queues; the unchanged choices of the first two
regimes; no launch order below 2048 units; the waiting-workgroup rule on both sides of 8 units per CU; every explicit fh_sched field
against its automatic value; and the queue count: FASTERHIP_HW_QUEUES before GPU_MAX_HW_QUEUES before 4, clamped to 1..32, an
unparsable value counting as absent."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_policy_table():
    exe = os.path.join(ROOT, "tests", "cpp", "test_launch_policy")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "faster_amd", "csrc", "fh_policy.hpp"), os.path.join(ROOT, "include", "fasterhip.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]
    assert int(r.stdout.split()[1]) > 250
