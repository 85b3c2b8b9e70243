"""The tree's quality figure without a GPU: the five entry points of evplp_accel_quality / evplp_set_refit_policy (exported, bound, declared,
refusing null handles; the ABI version unchanged) and evplp_accel_cost, the host statement of the SAH cost, on hand-written 64-byte node arrays
whose answers are written down, on a random tree of three chunks against math.fsum of the same terms, and on arrays that are not trees."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_accel_cost", "evplp_accel_quality", "evplp_set_refit_policy", "evplp_group_accel_quality", "evplp_group_set_refit_policy")
F = np.float32
KEYS = ("cost", "root_area", "inner_area", "leaf_pair_area", "leaf_tri_area")


def leaf(block, cnt):
    return ~((block << 2) | (cnt - 1))


def node(evplp, c0, c1, box0=None, box1=None):
    """one 64-byte node; box = (centre, half-size) or None for an absent child's (0, -3e38)"""
    n = np.zeros(1, evplp.ACCEL_NODE)[0]
    n["c0"], n["c1"] = c0, c1
    for s, b in enumerate((box0, box1)):
        ctr, hal = b if b is not None else ((0, 0, 0), (-3.0e38,) * 3)
        n["ctr"][:, s], n["hal"][:, s] = ctr, hal
    return n


def tree(evplp, nodes):
    return np.array(nodes, evplp.ACCEL_NODE)


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    q = evplp.AccelQuality()
    out = (C.c_double * 5)()
    assert L.evplp_accel_quality(None, C.byref(q)) == evplp.ERR_INVALID
    assert L.evplp_set_refit_policy(None, 1.5, -1) == evplp.ERR_INVALID
    assert L.evplp_group_accel_quality(None, C.byref(q)) == evplp.ERR_INVALID
    assert L.evplp_group_set_refit_policy(None, 1.5, -1) == evplp.ERR_INVALID
    assert L.evplp_accel_cost(None, 1, out) == evplp.ERR_INVALID
    nodes = tree(evplp, [node(evplp, leaf(0, 1), evplp.NO_CHILD, ((0, 0, 0), (1, 1, 1)))])
    assert L.evplp_accel_cost(nodes.ctypes.data, 1, None) == evplp.ERR_INVALID
    assert L.evplp_accel_cost(nodes.ctypes.data, 0, out) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for m in ("accel_quality", "set_refit_policy"):
        assert callable(getattr(evplp.Context, m)) and callable(getattr(evplp.Group, m)), m
    assert callable(evplp.accel_cost)


def test_the_struct_and_the_weights_match_the_sources(evplp, tmp_path):
    """the ctypes mirror against the header (a C program prints sizeof / offsetof), and the two weights against their one definition"""
    assert C.sizeof(evplp.AccelQuality) == 72
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evplp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(struct evplp_accel_quality), '
                   'offsetof(struct evplp_accel_quality, built_cost), offsetof(struct evplp_accel_quality, reached_nodes), offsetof(struct evplp_accel_quality, policy_rebuilds), '
                   'offsetof(struct evplp_accel_quality, last_action)); return 0; }\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    Q = evplp.AccelQuality
    assert got == [C.sizeof(Q), Q.built_cost.offset, Q.reached_nodes.offset, Q.policy_rebuilds.offset, Q.last_action.offset]
    types = open(os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")).read()
    assert len(re.findall(r"kCostNodeVisit = 15\.0, kCostPairTest = 40\.0;", types)) == 1
    for f in ("kernels.h", "bvh_gpu.hip", "context.cpp", "scene_motion.cpp", os.path.join("host", "accel_cost.cpp")):
        text = open(os.path.join(ROOT, "evplp_amd", "csrc", f)).read()
        assert not re.search(r"kCost(NodeVisit|PairTest)\s*=", text), f
    assert (evplp.COST_NODE_VISIT, evplp.COST_PAIR_TEST) == (15.0, 40.0)


def test_the_header_states_the_rules():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("still counts in its leaf's cnt, because the walk still tests it", "the call is no longer free of host waits",
                   "198 ms with the SAH builder, 13.9 ms with the device LBVH", "a policy rebuild leaves accumulators, noise moments and adaptive records alone",
                   "max_cost_ratio = 0 switches the policy off, which is the default", "tree cost (after a call)", "refit_prepare makes them"):
        assert needle in hdr, needle


def test_a_root_that_is_one_leaf(evplp):
    """half-sizes (1, 2, 3): a = 8 (2 + 6 + 3) = 88 = the box's own area; three triangles are two pairs"""
    q = evplp.accel_cost(tree(evplp, [node(evplp, leaf(0, 3), evplp.NO_CHILD, ((5, 6, 7), (1, 2, 3)))]))
    assert q == {"cost": 15.0 + 40.0 * 2, "root_area": 88.0, "inner_area": 0.0, "leaf_pair_area": 176.0, "leaf_tri_area": 264.0, "reached_nodes": 1}


def test_the_empty_tree_costs_nothing(evplp):
    q = evplp.accel_cost(tree(evplp, [node(evplp, evplp.NO_CHILD, evplp.NO_CHILD)]))
    assert q == {"cost": 0.0, "root_area": 0.0, "inner_area": 0.0, "leaf_pair_area": 0.0, "leaf_tri_area": 0.0, "reached_nodes": 1}


def three_nodes(evplp):
    """root -> (a, b) with unit half-sizes at x = -1 and x = +1: a = 24 each, union 4 x 2 x 2 = area 40.
    a: leaves of 1 and 2 triangles, half-sizes (.5, .5, .5) -> 6 and (1, .5, .5) -> 10
    b: leaves of 3 and 4 triangles, half-sizes (.5, 1, 1) -> 16 and (.25, .5, 1) -> 7"""
    return [node(evplp, 1, 2, ((-1, 0, 0), (1, 1, 1)), ((1, 0, 0), (1, 1, 1))),
            node(evplp, leaf(0, 1), leaf(1, 2), ((-1.5, 0, 0), (.5, .5, .5)), ((-1, 0, 0), (1, .5, .5))),
            node(evplp, leaf(2, 3), leaf(3, 4), ((1, 0, 0), (.5, 1, 1)), ((1.5, 0, 0), (.25, .5, 1)))]


THREE = {"cost": (15.0 * (40 + 48) + 40.0 * (6 * 1 + 10 * 1 + 16 * 2 + 7 * 2)) / 40, "root_area": 40.0, "inner_area": 48.0,
         "leaf_pair_area": 6.0 * 1 + 10 * 1 + 16 * 2 + 7 * 2, "leaf_tri_area": 6.0 * 1 + 10 * 2 + 16 * 3 + 7 * 4, "reached_nodes": 3}


def test_three_nodes_with_leaf_counts_one_to_four(evplp):
    assert THREE["leaf_pair_area"] == 62.0 and THREE["leaf_tri_area"] == 102.0 and THREE["cost"] == 95.0
    assert evplp.accel_cost(tree(evplp, three_nodes(evplp))) == THREE
    # raw bytes are accepted as well
    assert evplp.accel_cost(tree(evplp, three_nodes(evplp)).view(np.uint8)) == THREE


def test_an_absent_child_adds_nothing(evplp):
    """b's second child taken away: its reference is NO_CHILD and its half-size -3e38, whose products would be 9e76"""
    n = three_nodes(evplp)
    n[2] = node(evplp, leaf(2, 3), evplp.NO_CHILD, ((1, 0, 0), (.5, 1, 1)))
    q = evplp.accel_cost(tree(evplp, n))
    assert q == {"cost": (15.0 * 88 + 40.0 * 48) / 40, "root_area": 40.0, "inner_area": 48.0, "leaf_pair_area": 48.0, "leaf_tri_area": 74.0, "reached_nodes": 3}
    # ... and the root's own absent child is left out of the union: the root box is a's alone
    n[0] = node(evplp, 1, evplp.NO_CHILD, ((-1, 0, 0), (1, 1, 1)))
    q = evplp.accel_cost(tree(evplp, n))
    assert q == {"cost": (15.0 * 48 + 40.0 * 16) / 24, "root_area": 24.0, "inner_area": 24.0, "leaf_pair_area": 16.0, "leaf_tri_area": 26.0, "reached_nodes": 2}
    # a leaf whose triangles have all lost their area keeps its reference and has an empty box: nothing either
    n = three_nodes(evplp)
    n[2]["hal"][:, 1] = -3.0e38
    assert evplp.accel_cost(tree(evplp, n))["leaf_tri_area"] == 74.0


def test_a_node_the_root_does_not_reach_is_ignored(evplp):
    n = three_nodes(evplp) + [node(evplp, leaf(9, 4), leaf(10, 4), ((0, 0, 0), (100, 100, 100)), ((0, 0, 0), (50, 50, 50)))]
    assert evplp.accel_cost(tree(evplp, n)) == THREE
    n = three_nodes(evplp)
    n.insert(1, node(evplp, leaf(9, 4), evplp.NO_CHILD, ((0, 0, 0), (100, 100, 100))))      # in the middle of the array: a is node 2, b node 3
    n[0]["c0"], n[0]["c1"] = 2, 3
    assert evplp.accel_cost(tree(evplp, n)) == THREE


def random_tree(evplp, n, seed):
    """a random binary tree over n inner nodes, stored in a random order but for the root (test_refit_host.py's), with random boxes and leaf counts"""
    rng = np.random.RandomState(seed)
    name = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    kids = [[None, None] for _ in range(n)]
    free = [(0, 0), (0, 1)]
    for k in range(1, n):
        p, s = free.pop(rng.randint(len(free)))
        kids[p][s] = int(name[k])
        free += [(k, 0), (k, 1)]
    for p, s in free:
        kids[p][s] = evplp.NO_CHILD if rng.rand() < 0.1 else leaf(rng.randint(1000), 1 + rng.randint(4))
    nodes = np.zeros(n, evplp.ACCEL_NODE)
    for k in range(n):
        i = name[k]
        nodes[i]["c0"], nodes[i]["c1"] = kids[k]
        nodes[i]["ctr"] = rng.uniform(-10, 10, (3, 2)).astype(F)
        nodes[i]["hal"] = rng.uniform(1e-3, 5, (3, 2)).astype(F)
        for s in range(2):
            if kids[k][s] == evplp.NO_CHILD:
                nodes[i]["ctr"][:, s], nodes[i]["hal"][:, s] = 0, -3.0e38
    return nodes


def fsum_cost(evplp, nodes):
    """the same terms (fp64 from the fp32 half-sizes, the three products added in the same order), summed exactly"""
    _, order, _ = evplp.refit_levels(nodes, level_capacity=len(nodes))
    inner, pair, tri = [], [], []
    for i in order:
        for s, ref in enumerate((int(nodes[i]["c0"]), int(nodes[i]["c1"]))):
            hx, hy, hz = (float(h) for h in nodes[i]["hal"][:, s])
            if ref == evplp.NO_CHILD or min(hx, hy, hz) < 0:
                continue
            a = 8.0 * (hx * hy + hy * hz + hz * hx)
            if ref >= 0:
                inner.append(a)
            else:
                cnt = (~ref & 3) + 1
                pair.append(a * ((cnt + 1) >> 1)); tri.append(a * cnt)
    lo, hi = [], []
    for s, ref in enumerate((int(nodes[0]["c0"]), int(nodes[0]["c1"]))):
        if ref != evplp.NO_CHILD and nodes[0]["hal"][:, s].min() >= 0:
            lo.append(nodes[0]["ctr"][:, s].astype(np.float64) - nodes[0]["hal"][:, s].astype(np.float64))
            hi.append(nodes[0]["ctr"][:, s].astype(np.float64) + nodes[0]["hal"][:, s].astype(np.float64))
    root = 0.0
    if lo:
        dx, dy, dz = (float(v) for v in np.max(hi, axis=0) - np.min(lo, axis=0))
        root = 2.0 * (dx * dy + dy * dz + dz * dx)
    i, p, t = math.fsum(inner), math.fsum(pair), math.fsum(tri)
    return {"cost": (15.0 * (root + i) + 40.0 * p) / root if root > 0 else 0.0, "root_area": root, "inner_area": i, "leaf_pair_area": p, "leaf_tri_area": t,
            "reached_nodes": len(order)}


def within_the_bound(got, want):
    """Every term is positive, a running or pairwise sum of n of them is off by at most (n - 1) 2^-53 of the sum to first order, and no sum here
    has more than reached + 1 terms; the cost adds four roundings of its own.  reached * 2^-52 covers that from six nodes on."""
    assert got["reached_nodes"] == want["reached_nodes"]
    tol = got["reached_nodes"] * 2.0 ** -52
    assert got["root_area"] == want["root_area"]                                       # (no sum: the same few operations)
    for k in KEYS:
        assert abs(got[k] - want[k]) <= tol * want[k], (k, got[k], want[k])


def test_a_random_tree_of_three_chunks_against_fsum(evplp):
    nodes = random_tree(evplp, 600, seed=3)
    got, want = evplp.accel_cost(nodes), fsum_cost(evplp, nodes)
    assert got["reached_nodes"] == 600 > 2 * 256 and want["inner_area"] > 0 and want["leaf_tri_area"] > want["leaf_pair_area"] > 0
    within_the_bound(got, want)
    assert evplp.accel_cost(nodes) == got                                              # deterministic
    # a chain deeper than any walk's stack is still a tree to the host function
    chain = [node(evplp, leaf(i, 2), i + 1, ((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1))) for i in range(99)] + [node(evplp, leaf(99, 2), leaf(100, 1), ((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1)))]
    assert evplp.accel_cost(tree(evplp, chain)) == {"cost": (15.0 * (24 + 99 * 24) + 40.0 * 101 * 24) / 24, "root_area": 24.0, "inner_area": 99 * 24.0,
                                                    "leaf_pair_area": 101 * 24.0, "leaf_tri_area": (2 * 100 + 1) * 24.0, "reached_nodes": 100}


@pytest.mark.parametrize("name, children", [
    ("a child index >= nnodes", [(1, 2), (-1, -1)]),
    ("a self-loop", [(0, -1)]),
    ("a two-node cycle below the root", [(1, -1), (2, -1), (-1, 1)]),
    ("a node with two parents", [(1, 2), (3, -1), (-1, 3), (-1, -1)]),
    ("the same child twice", [(1, 1), (-1, -1)]),
])
def test_what_is_not_a_tree_is_refused_promptly(evplp, name, children):
    nodes = tree(evplp, [node(evplp, a, b, ((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1))) for a, b in children])
    out = (C.c_double * 5)()
    t0 = time.perf_counter()
    rc = evplp.lib().evplp_accel_cost(nodes.ctypes.data, len(nodes), out)
    assert rc == evplp.ERR_INVALID, name
    assert time.perf_counter() - t0 < 1.0, name
    with pytest.raises(evplp.EvplpError):
        evplp.accel_cost(nodes)
    with pytest.raises(evplp.EvplpError):                                              # (what evplp_refit_levels refuses)
        evplp.refit_levels(nodes)


def test_the_cost_under_asan_and_ubsan(tmp_path):
    """a stand-alone host program (tools/host_fuzz/accel_cost_fuzz.cpp): 20 000 seeded node arrays, half of them trees of up to 700 nodes"""
    from test_kernel_resources import HIPCC
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    if shutil.which("g++") is None or not os.path.isdir(rocm_include):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "accel_cost_fuzz")
    host = os.path.join(ROOT, "evplp_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-isystem", rocm_include, "-o", exe, os.path.join(ROOT, "tools", "host_fuzz", "accel_cost_fuzz.cpp"), os.path.join(host, "accel_cost.cpp"), os.path.join(host, "refit_levels.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"costs (\d+) refused (\d+)", r.stdout)
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) > 2000, r.stdout
