"""The protocol of the guarded scratch areas (decaf377_amd/csrc/scratch_area.hpp), without a GPU.

tests/cpp/scratch_area_host.cpp compiles the header against a fake runtime of its own -- it defines the ten runtime entry points
the header calls, logs every call and backs blocks and events with malloc/free -- and asserts the protocol on the log and on the
area's fields: nothing is called within capacity; growth drains the guard, then frees, then allocates, to the capacity of each
area's rule; a guard that has seen a capture retires instead and frees with destroy(); growth is refused inside a capture; a
failed hipMalloc or hipFree leaves the area {null, 0}; GuardScope waits and records as it should.  The program is built plain
and with -fsanitize=address,undefined and run as an ordinary program, the latter with leak checking on: a block freed twice or
never is the sanitizer's finding.  The GPU tests of the same areas (test_sums_streams_gpu.py, test_batch_scratch_gpu.py)
cannot tell a drain from the wait hipFree performs on its own; the call log can."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decaf377_amd", "csrc")
PROG = os.path.join(ROOT, "tests", "cpp", "scratch_area_host.cpp")


@pytest.fixture(scope="module")
def programs():
    """The host program plain and under AddressSanitizer + UBSan, compiled side by side; neither links the HIP runtime."""
    outs = {"plain": os.path.join(ROOT, "tests", "cpp", "scratch_area_host"), "san": os.path.join(ROOT, "tests", "cpp", "scratch_area_host_san")}
    common = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, PROG]
    cmds = {"plain": ["g++", "-O2"] + common + ["-o", outs["plain"]],
            "san": ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + common + ["-o", outs["san"]]}
    srcs = [PROG, os.path.join(CSRC, "scratch_area.hpp"), os.path.join(ROOT, "include", "decaf377_amd.h")]
    stale = lambda o: not os.path.exists(o) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs)
    procs = {k: subprocess.Popen(cmds[k]) for k in cmds if stale(outs[k])}
    for k, pr in procs.items():
        assert pr.wait() == 0, cmds[k]
    return outs


@pytest.mark.parametrize("build", ["plain", "san"])
def test_the_protocol_on_a_fake_runtime(programs, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([programs[build]], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout[-2000:], r.stderr[-2000:])


def test_the_program_does_not_link_the_runtime(programs):
    for build, path in programs.items():
        needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
        assert "amdhip64" not in needed and "hsa-runtime" not in needed, build


def test_the_header_includes_nothing_of_the_device_code():
    """scratch_area.hpp needs the runtime's API header, the error codes and the C library, and nothing else of csrc/."""
    import re
    text = open(os.path.join(CSRC, "scratch_area.hpp")).read()
    quoted = re.findall(r'#include\s+"([^"]+)"', text)
    assert quoted == ["../../include/decaf377_amd.h"], quoted
    assert "hip/hip_runtime_api.h" in re.findall(r"#include\s+<([^>]+)>", text) and "<hip/hip_runtime.h>" not in text
