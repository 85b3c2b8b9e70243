"""Moving scenes without a GPU: the seven entry points of evplp_update_mesh / evplp_refit_accel (exported, bound, declared, refusing null
handles; the ABI version unchanged) and the refit's level plan, evplp_refit_levels, on hand-written 64-byte node arrays: whatever the storage
order, every node's inner children lie in strictly lower levels, and an array that is not a tree is refused at once."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_update_mesh", "evplp_refit_accel", "evplp_refit_info", "evplp_refit_levels", "evplp_debug_accel", "evplp_group_update_mesh", "evplp_group_refit_accel")
LEAF = -1            # ~0: leaf block 0 with one triangle (any negative reference but NO_CHILD is a leaf)


def tree(evplp, children):
    """64-byte nodes from [(c0, c1)]; the boxes do not matter to the plan"""
    n = np.zeros(len(children), evplp.ACCEL_NODE)
    for i, (a, b) in enumerate(children):
        n[i]["c0"], n[i]["c1"] = a, b
    return n


def check_plan(evplp, nodes, height, order, begin):
    """the levels partition the nodes, each level holds one height, and inner children sit in strictly lower levels"""
    n = len(nodes)
    assert begin[0] == 0 and begin[-1] == n and np.all(np.diff(begin) > 0)
    assert sorted(order.tolist()) == list(range(n))
    level = np.zeros(n, np.int64)
    for l in range(len(begin) - 1):
        level[order[begin[l]:begin[l + 1]]] = l
    assert np.array_equal(level, height)
    for s in ("c0", "c1"):
        inner = nodes[s] >= 0
        assert np.all(level[nodes[s][inner]] < level[inner])
    has_inner = (nodes["c0"] >= 0) | (nodes["c1"] >= 0)
    assert np.all((level == 0) == ~has_inner)


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    v = np.zeros((3, 3), np.float32)
    buf = np.zeros(16, np.int32)
    assert L.evplp_update_mesh(None, 0, v.ctypes.data, 3) == evplp.ERR_INVALID
    assert L.evplp_refit_accel(None) == evplp.ERR_INVALID
    assert L.evplp_refit_info(None, None, None, None) == evplp.ERR_INVALID
    assert L.evplp_debug_accel(None, 0, buf.ctypes.data, 64) == evplp.ERR_INVALID
    assert L.evplp_group_update_mesh(None, 0, v.ctypes.data, 3) == evplp.ERR_INVALID
    assert L.evplp_group_refit_accel(None) == evplp.ERR_INVALID
    assert L.evplp_refit_levels(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for m in ("update_mesh", "refit_accel", "refit_info", "debug_accel"):
        assert callable(getattr(evplp.Context, m)), m
    for m in ("update_mesh", "refit_accel"):
        assert callable(getattr(evplp.Group, m)), m
    assert callable(evplp.refit_levels) and callable(evplp.Context.refit_levels)


def test_the_header_states_the_rules():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("While any mesh is dirty EVERY pass is refused", "evplp_build_accel on a dirty context is the full rebuild",
                   "has no leaf to go to: evplp_refit_accel returns EVPLP_ERR_INVALID, the context stays dirty",
                   "A refit leaves the accumulators, the noise moments and the adaptive records alone", "one launch per height of the tree"):
        assert needle in hdr, needle


def test_a_wrapper_root_is_one_level(evplp):
    nodes = tree(evplp, [(LEAF, evplp.NO_CHILD)])
    h, order, begin = evplp.refit_levels(nodes)
    assert h.tolist() == [0] and order.tolist() == [0] and begin.tolist() == [0, 1]


def test_storage_order_does_not_matter(evplp):
    """root -> (a, b), a -> (leaf, c), b -> (leaf, leaf), c -> (leaf, leaf): three levels, stored parents first and children first"""
    parents_first = tree(evplp, [(1, 2), (LEAF, 3), (~4, ~8), (~12, ~17)])                  # root 0, a 1, b 2, c 3
    # the same tree with the root still node 0 and everything else reversed: a 3, b 2, c 1 -- children in front of their parents
    children_first = tree(evplp, [(3, 2), (~12, ~17), (~4, ~8), (LEAF, 1)])
    h0, o0, b0 = evplp.refit_levels(parents_first)
    h1, o1, b1 = evplp.refit_levels(children_first)
    check_plan(evplp, parents_first, h0, o0, b0)
    check_plan(evplp, children_first, h1, o1, b1)
    assert len(b0) == len(b1) == 4
    # per node of the TREE: root 2, a 1, b 0, c 0
    assert h0.tolist() == [2, 1, 0, 0] and h1.tolist() == [2, 0, 0, 1]
    assert b0.tolist() == b1.tolist() == [0, 2, 3, 4]
    assert o0.tolist() == [2, 3, 1, 0] and o1.tolist() == [1, 2, 3, 0]


def test_a_forty_deep_chain(evplp):
    nodes = tree(evplp, [(LEAF, i + 1) for i in range(39)] + [(LEAF, ~4)])
    h, order, begin = evplp.refit_levels(nodes)
    check_plan(evplp, nodes, h, order, begin)
    assert len(begin) == 41 and h.tolist() == list(range(39, -1, -1)) and order.tolist() == list(range(39, -1, -1))
    with pytest.raises(evplp.EvplpError):
        evplp.refit_levels(nodes, level_capacity=39)
    assert len(evplp.refit_levels(nodes, level_capacity=40)[2]) == 41


def random_tree(evplp, n, seed):
    """a random binary tree over n inner nodes, stored in a random order but for the root (node 0)"""
    rng = np.random.RandomState(seed)
    name = np.concatenate([[0], 1 + rng.permutation(n - 1)])              # tree node k is stored as name[k]
    kids = [[LEAF, LEAF] for _ in range(n)]
    free = [(0, 0), (0, 1)]
    for k in range(1, n):
        p, s = free.pop(rng.randint(len(free)))
        kids[p][s] = k
        free += [(k, 0), (k, 1)]
    for p, s in free:
        if rng.rand() < 0.1:
            kids[p][s] = evplp.NO_CHILD
    stored = [None] * n
    for k in range(n):
        stored[name[k]] = tuple(int(name[c]) if c >= 0 else c for c in kids[k])
    return tree(evplp, stored)


def test_children_lie_in_strictly_lower_levels_on_a_random_tree(evplp):
    nodes = random_tree(evplp, 200, seed=5)
    h, order, begin = evplp.refit_levels(nodes)
    check_plan(evplp, nodes, h, order, begin)
    assert 8 <= len(begin) - 1 <= 64
    again = evplp.refit_levels(nodes)
    assert all(np.array_equal(a, b) for a, b in zip((h, order, begin), again))      # deterministic


@pytest.mark.parametrize("name, children", [
    ("a child index >= nnodes", [(1, 2), (LEAF, LEAF)]),
    ("a self-loop", [(0, LEAF)]),
    ("a self-loop below the root", [(1, LEAF), (1, LEAF)]),
    ("a two-node cycle", [(1, LEAF), (LEAF, 0)]),
    ("a two-node cycle below the root", [(1, LEAF), (2, LEAF), (LEAF, 1)]),
    ("a node with two parents", [(1, 2), (3, LEAF), (LEAF, 3), (LEAF, LEAF)]),
    ("the same child twice", [(1, 1), (LEAF, LEAF)]),
])
def test_what_is_not_a_tree_is_refused_promptly(evplp, name, children):
    nodes = tree(evplp, children)
    n = len(nodes)
    h, o, b = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(65, np.int32)
    t0 = time.perf_counter()
    rc = evplp.lib().evplp_refit_levels(nodes.ctypes.data, n, h.ctypes.data, o.ctypes.data, b.ctypes.data, 64)
    assert rc == evplp.ERR_INVALID, name
    assert time.perf_counter() - t0 < 1.0, name
    with pytest.raises(evplp.EvplpError):
        evplp.refit_levels(nodes)


def test_too_small_a_capacity_and_bad_arguments_are_refused(evplp):
    nodes = tree(evplp, [(1, 2), (LEAF, 3), (~4, ~8), (~12, ~17)])
    with pytest.raises(evplp.EvplpError):
        evplp.refit_levels(nodes, level_capacity=2)
    assert len(evplp.refit_levels(nodes, level_capacity=3)[2]) == 4
    h, o, b = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(8, np.int32)
    L = evplp.lib()
    assert L.evplp_refit_levels(nodes.ctypes.data, 0, h.ctypes.data, o.ctypes.data, b.ctypes.data, 4) == evplp.ERR_INVALID
    assert L.evplp_refit_levels(nodes.ctypes.data, 4, None, o.ctypes.data, b.ctypes.data, 4) == evplp.ERR_INVALID
    assert L.evplp_refit_levels(nodes.ctypes.data, 4, h.ctypes.data, o.ctypes.data, b.ctypes.data, 0) == evplp.ERR_INVALID


def test_the_plan_under_asan_and_ubsan(tmp_path):
    """a stand-alone host program (tools/host_fuzz/refit_levels_fuzz.cpp): 200 000 seeded node arrays, most of them not trees"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "refit_levels_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tools", "host_fuzz", "refit_levels_fuzz.cpp"), os.path.join(ROOT, "evplp_amd", "csrc", "host", "refit_levels.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"plans (\d+) refused (\d+)", r.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 10000, r.stdout
