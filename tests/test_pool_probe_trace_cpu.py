"""The frame pool's placement probe (jsplayer_amd/csrc/jsp_pool.cpp), pinned without a GPU: tests/pool_probe/trace.cpp scripts the two measurements
the probe rests on, watches every memory call of the stub HIP runtime under tests/tsan/ and prints what the probe did, group by group (a group is a run
of pools in one process: the probe remembers the form that won).  tests/golden/pool_probe_trace.txt is that output as recorded from the commit BEFORE
jsp_pool_create was taken apart (when the whole of it was one function in jsp_api.cpp); the code of today must reproduce it byte for byte, under
AddressSanitizer and UBSan with leak detection, and leave no allocation outstanding after any pool.

    python tests/test_pool_probe_trace_cpu.py [TREE]    prints the trace of the sources under TREE (default: this tree), built with the harness of this one
"""
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pool_probe_trace.txt")
HOST_LAYERS = ["jsp_api", "jsp_pool", "jsp_shard", "msv1_codec", "msv1_host", "sp_codec", "sp_entropy", "sp_host", "sp_models"]   # tools/tsan_cpu.sh's list
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]


def build(out, tree=ROOT):
    """The product's host layers from `tree`, the stubs and the trace program from this tree; at most 4 compilers at a time."""
    csrc, stubs = os.path.join(tree, "jsplayer_amd", "csrc"), os.path.join(ROOT, "tests", "tsan")
    inc = ["-I" + stubs, "-I" + csrc, "-I" + os.path.join(tree, "include")]
    units = [os.path.join(csrc, f + ".cpp") for f in HOST_LAYERS if os.path.exists(os.path.join(csrc, f + ".cpp"))]
    units += [os.path.join(stubs, "hip_stub.cpp"), os.path.join(stubs, "kernel_stubs.cpp"), os.path.join(ROOT, "tests", "pool_probe", "trace.cpp")]

    def compile_one(src):
        obj = os.path.join(out, os.path.basename(src)[:-4] + ".o")
        subprocess.run(["g++", *FLAGS, "-DJSP_STUB_NO_POOL_RATES", *inc, "-c", src, "-o", obj], check=True, timeout=900)
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:
        objs = list(pool.map(compile_one, units))
    exe = os.path.join(out, "trace")
    # (the sanitizer runtimes linked in statically: the program starts whatever the environment preloads)
    subprocess.run(["g++", *FLAGS, "-static-libasan", "-static-libubsan", *objs, "-o", exe, "-ldl"], check=True, timeout=900)
    return exe


def run_groups(exe, names=None):
    """(trace text, [(group, exit status)]): every recorded group (or those named) in a fresh process, leak detection on."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for k in [k for k in env if k.startswith("JSP_POOL_PROBE")]:
        del env[k]
    names = names or subprocess.run([exe, "--list"], check=True, stdout=subprocess.PIPE, env=env, timeout=60).stdout.decode().split()
    text, status = "", []
    for name in names:
        res = subprocess.run([exe, name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
        text += res.stdout.decode(errors="replace")
        status.append((name, res.returncode))
    return text, status


@pytest.fixture(scope="module")
def trace_exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    return build(str(tmp_path_factory.mktemp("pool_probe")))


def test_pool_probe_trace_matches_the_record(trace_exe):
    text, status = run_groups(trace_exe)
    assert all(rc == 0 for _, rc in status), (status, text[-3000:])
    assert "Sanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert len(status) >= 16
    golden = open(GOLDEN).read()
    if text != golden:
        got, want = text.splitlines(), golden.splitlines()
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail("the trace left the record at line %d:\n  recorded: %s\n  now:      %s" % (at + 1, want[at][:400] if at < len(want) else "<end>", got[at][:400] if at < len(got) else "<end>"))


def test_failures_the_recorded_commit_did_not_survive(trace_exe):
    """Not in the record, because the recorded commit behaved otherwise: it leaked the frames of a pool that is not probed when a later frame's
    allocation failed, and its hold limit for a negative JSP_POOL_PROBE_HOLD_GB was undefined (a cast of a negative double to an unsigned number).
    The trace program ends with status 3 when anything is outstanding after a pool."""
    text, status = run_groups(trace_exe, ["new_failures"])
    assert status == [("new_failures", 0)] and "Sanitizer" not in text and "runtime error" not in text, text[-3000:]
    pools = text.split("\npool ")[1:]
    assert len(pools) == 3 and all(p.rstrip().endswith("outstanding: 0 allocations, 0 physical") for p in pools), text
    assert "hipMalloc (12288 bytes): a3; hipMemset (12288 bytes): a3+0\n" in pools[0] and "hipMalloc (12288 bytes) FAILS" in pools[0] and "hipFree x4: a0+0 a1+0 a2+0 a3+0" in pools[0], pools[0]
    assert " failed: hipMalloc(&d, bytes) failed: stub HIP error (FILE:LINE)" in pools[0], pools[0]
    assert "hipMalloc (256 bytes) FAILS" in pools[1] and " failed: hipMalloc(" in pools[1] and "store rate #" not in pools[1], pools[1]
    assert "hold limit 2147483648 " in pools[2] and " 3 attempts" in pools[2], pools[2]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        text, status = run_groups(build(d, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT))
    sys.stdout.write(text)
    sys.exit(0 if all(rc == 0 for _, rc in status) else 1)
