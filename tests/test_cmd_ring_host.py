"""No GPU needed: how a group call crosses from the caller's thread to a rank's worker (csrc/host/cmd_ring.hpp) -- a task with inline storage,
the single-producer ring that carries it, the workers' barrier -- compiles without HIP.  A stand-alone program runs all three under
ThreadSanitizer and under AddressSanitizer + UndefinedBehaviorSanitizer; the rest of this file is about what group.cpp no longer holds."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evplp_amd", "csrc")
SANITIZERS = {"thread": ["-fsanitize=thread"], "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _read(*parts):
    return open(os.path.join(CSRC, *parts)).read()


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_ring_task_and_barrier_under_sanitizers(tmp_path, sanitizer):
    """tools/host_fuzz/cmd_ring_check.cpp: one producer and four consumers, 200 000 tasks each of three state sizes, in order and exactly once,
    through full rings and through sleeping consumers; 2 x 100 000 tasks whose state holds a shared pointer and counts its copies; the
    barrier's verdict over 100 000 generations of 2, 3 and 8 parties"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / ("cmd_ring_check_" + sanitizer))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread"] + SANITIZERS[sanitizer] + ["-I" + os.path.join(CSRC, "host"), "-o", exe,
                                                                                  os.path.join(ROOT, "tools", "host_fuzz", "cmd_ring_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.match(r"tasks (\d+) full_waits (\d+) sleeps (\d+) generations (\d+) constructed (\d+) destroyed (\d+)", r.stdout)
    assert m, r.stdout
    tasks, full_waits, sleeps, generations, constructed, destroyed = map(int, m.groups())
    # no path was skipped: every task ran, the producer met full rings, consumers slept and were woken, every copy of a state was destroyed
    assert tasks == 4 * 200000 + 2 * 100000 and full_waits > 0 and sleeps > 0 and generations == 300000, r.stdout
    assert constructed == destroyed and constructed >= 3 * 100000, r.stdout


def test_the_ring_is_host_only_and_group_cpp_holds_no_slots():
    hdr = _read("host", "cmd_ring.hpp")
    assert not re.search(r"hip/|hip_runtime|\bhip[A-Z]\w*|__global__|__device__", hdr), "cmd_ring.hpp names no HIP header and no HIP call"
    assert "context.hpp" not in hdr and "evplp_context" not in hdr and "kernels.h" not in hdr
    assert all(not inc.endswith((".h", ".hpp")) for inc in re.findall(r"#include [<\"]([^>\"]+)[>\"]", hdr)), "standard headers only"
    assert hdr.index("#pragma GCC visibility push(hidden)") < hdr.index("class Task") < hdr.index("struct Ring") < hdr.index("struct SpinBarrier") < hdr.index("#pragma GCC visibility pop")
    # the parent's memory orders
    assert "tail.store(t + 1, std::memory_order_seq_cst)" in hdr and "head.store(h + 1, std::memory_order_release)" in hdr
    assert hdr.index("task.reset();") < hdr.index("head.store(h + 1, std::memory_order_release)"), "a slot goes back only once its task's state is destroyed"
    assert "constexpr int kRing = 64;" in hdr and "constexpr int kSpinBeforeSleep = 200000;" in hdr
    grp = _read("group.cpp")
    assert '#include "host/cmd_ring.hpp"' in grp
    for needle in ("cmd.i[", "cmd.f[", "cmd.u[", ".p0", ".p1", "OP_", "switch (cmd.op", "struct Cmd", "struct SpinBarrier"):
        assert needle not in grp, needle
    # a slot is no larger than the positional record was, and the check program fills a task to group.cpp's capacity
    assert "static_assert(sizeof(Task) <= 176" in grp
    capacity = re.search(r"constexpr size_t kTaskBytes = (\d+);", grp).group(1)
    assert ("constexpr size_t kCapacity = %s;" % capacity) in open(os.path.join(ROOT, "tools", "host_fuzz", "cmd_ring_check.cpp")).read()


def test_each_idiom_of_the_group_is_stated_once():
    grp = _read("group.cpp")
    assert len(re.findall(r"\bok\(\) const \{", grp)) == 1 and len(re.findall(r"\bvoid hip_fail\(hipError_t", grp)) == 1
    assert not re.search(r"auto (ok|hip_fail) =", grp)
    assert grp.count("hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP, hipGetErrorString(e))") == 1, "the workers' HIP failures go through Worker::hip_fail"
    # "a failed group takes no new command": post_all and post_one, and nobody else
    assert grp.count("if (g->failed.load(std::memory_order_acquire)) { drain(g); return group_status(g); }") == 2
    assert grp.count("static int post_one(") == 1 and grp.count("post_one(g, ") == 4, "post_pass, present_ex, noise_fold, synchronize_rank"
    # the mesh / refit / tree wrappers: drain, rank 0's check, its message
    assert grp.count('g->set_error("%s", g->ctx[0]->error)') == 2, "rank0_refuses, and the temporal info of evplp_group_denoise_temporal"
    assert grp.count("rank0_refuses(g, ") == 11
    assert grp.count("launch_assemble_strips(") == 1 and grp.count("g->strip_floats / ((size_t)c->st.W * 3)") == 1 and grp.count("assemble_strips(g, ") == 3
    # a collective is named by the wrapper that posts it, and t_exchange belongs to the exchanges
    assert grp.count("w.t_exchange +=") == 1 and grp.count("w->t_exchange +=") == 2, "a command's `always` stage; the reduction and the noise pool"
    for name in ("exchange_strips", "exchange_records", "exchange_denoise"):
        assert grp.count("static void %s(Worker &w" % name) == 1, name


def test_nothing_of_the_ring_is_exported(evplp):
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    exported = subprocess.run(["nm", "-D", "--defined-only", evplp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in exported.splitlines() if line.strip()]
    assert "evplp_group_create" in names
    for name in names:
        assert not re.search(r"4Ring|4Task|11SpinBarrier|cmd_ring|6Worker", name), name
    # the C ABI is what include/evplp.h declares, as before
    assert set(evplp._SIGNATURES) <= set(names)
    assert evplp.lib().evplp_abi_version() == 5
