"""The numpy replay of the walks' stacks (walk_replay.py) on hand-made trees with written-down answers, and the oracle on the two
Morton-chain scenes (scenes.morton_chain, scenes.morton_chain_full) before tests/test_gpu_deep_trees.py relies on either.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_api as oa
import scenes
import walk_replay as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = "leaf"


def make_nodes(spec):
    """Binary nodes in pre-order from nested pairs: (left, right) an inner node, None an absent child, "leaf" or ("leaf", zlo, zhi) a leaf
    whose box is [-1, 1] x [-1, 1] x [zlo, zhi]; an inner node's box is the union of its children's."""
    nodes = []
    leaves = [0]

    def is_leaf(s):
        return s == L or (len(s) == 3 and s[0] == L)

    def box_of(s):
        if s is None:
            return None
        if is_leaf(s):
            z = (0.0, 1.0) if s == L else s[1:]
            return np.array([[-1, -1, z[0]], [1, 1, z[1]]], np.float64)
        a, b = (box_of(c) for c in s)
        if a is None or b is None:
            return a if b is None else b
        return np.array([np.minimum(a[0], b[0]), np.maximum(a[1], b[1])])

    def emit(s):
        i = len(nodes); nodes.append(np.zeros((), wr.NODE))
        for k, c in enumerate(s):
            if c is None:
                ref = wr.NO_CHILD; nodes[i]["hal"][:, k] = -3.0e38
            else:
                b = box_of(c)
                nodes[i]["ctr"][:, k] = 0.5 * (b[0] + b[1]); nodes[i]["hal"][:, k] = 0.5 * (b[1] - b[0]) * 1.0001
                if is_leaf(c):
                    ref = ~(leaves[0] << 2); leaves[0] += 1
                else:
                    ref = emit(c)
            nodes[i]["c0" if k == 0 else "c1"] = ref
        return i
    emit(spec)
    return np.array(nodes, wr.NODE)


def chain(four_wide_levels, side, z=False):
    """a chain of 2 k - 1 inner nodes (k four-wide levels, the last one two leaves); with z, a leaf lies the nearer along +z the deeper it hangs"""
    n = 2 * four_wide_levels - 1
    leaf = (lambda j: (L, 100.0 - j, 100.5 - j)) if z else (lambda j: L)
    s = (leaf(n), leaf(n + 1))
    for j in range(n - 2, -1, -1):
        s = (s, leaf(j)) if side == "left" else (leaf(j), s)
    return s


def balanced(four_wide_levels):
    s = L
    for _ in range(2 * four_wide_levels):
        s = (s, s)
    return s


@pytest.mark.parametrize("spec, entries", [
    ((L, None), 0),                                         # a single wrapped leaf: nothing is ever pushed
    ((L, L), 1),                                            # one of two leaves waits
    (((L, L), None), 1),                                    # an absent child: two grandchildren, not four
    ((((L, L), (L, L)), None), 2),                          # ... and under it one inner node waits while the other's leaf waits
    (chain(2, "left"), 3), (chain(3, "left"), 5), (chain(4, "left"), 7),        # 2 per level (a leaf, a leaf) + 1 at the end
    (chain(2, "right"), 3), (chain(3, "right"), 5), (chain(4, "right"), 7),
    (balanced(1), 3), (balanced(2), 6), (balanced(3), 9), (balanced(4), 12),    # 3 per level
])
def test_worst_case_entries_on_hand_made_trees(spec, entries):
    nodes = make_nodes(spec)
    assert wr.worst_case_entries(nodes) == entries
    assert wr.worst_case_entries(wr.four_wide(nodes)) == entries


def test_four_wide_nodes_of_a_hand_made_tree():
    nodes = make_nodes((((L, 0.0, 1.0), (L, 2.0, 3.0)), (L, 4.0, 5.0)))
    n4 = wr.four_wide(nodes)
    assert n4["child"][0].tolist() == [~0, ~4, ~8, wr.NO_CHILD]
    assert np.allclose(n4["lo"][0, 2, :3], [0.0, 2.0, 4.0], atol=1e-3) and np.allclose(n4["hi"][0, 2, :3], [1.0, 3.0, 5.0], atol=1e-3)
    assert (n4["lo"][0, :, 3] > n4["hi"][0, :, 3]).all(), "an absent child has lo > hi"
    assert wr.tree_levels(nodes) == 3


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("levels", [2, 3, 4, 9])
def test_replay_reaches_the_worst_case_on_a_chain(side, levels):
    """Every box is entered and the rest of the chain is always the nearest: each visit leaves its two leaves on the stack."""
    n4 = wr.four_wide(make_nodes(chain(levels, side, z=True)))
    want = 2 * levels - 1
    assert wr.worst_case_entries(n4) == want
    assert wr.replay_closest(n4, [0.1, 0.2, -1.0], [0.001, 0.002, 1.0], 1e-4) == want
    # the other way round the leaves come first, nearest first, and the chain waits: one entry fewer at the end, where nothing waits
    assert wr.replay_closest(n4, [0.1, 0.2, 300.0], [0.001, 0.002, -1.0], 1e-4) == 2
    assert wr.replay_closest(n4, [5.0, 5.0, -1.0], [0.0, 0.0, 1.0], 1e-4) == 0, "a ray that misses the root pushes nothing"


def test_replay_stays_within_the_worst_case_for_random_rays():
    rng = np.random.RandomState(3)

    def grow(d):
        if d == 0 or rng.rand() < 0.15:
            z = float(rng.rand() * 4.0)
            return (L, z, z + 0.2 + float(rng.rand()))
        return (grow(d - 1), grow(d - 1))
    nodes = make_nodes((grow(7), grow(7)))
    n4 = wr.four_wide(nodes)
    worst = wr.worst_case_entries(n4)
    o = (rng.rand(1000, 3) * [3.0, 3.0, 8.0] - [1.5, 1.5, 2.0]).astype(np.float32)
    d = rng.randn(1000, 3).astype(np.float32)
    sp = wr.replay_closest(n4, o, d, 1e-4)
    assert sp.max() <= worst and sp.max() >= 4 and (sp == 0).any()
    # one ray at a time gives what the batch gives
    for k in range(0, 1000, 97):
        assert wr.replay_closest(n4, o[k], d[k], 1e-4) == sp[k]
    # the packet walk pushes at most one entry per binary level
    for k in range(0, 1000, 64):
        assert wr.replay_packet(nodes, o[k], d[k:k + 64]) <= wr.tree_levels(nodes) - 1


def test_packet_replay_on_a_chain():
    nodes = make_nodes(chain(3, "left", z=True))                    # five inner nodes
    dirs = np.array([[0.001, 0.002, 1.0], [0.002, -0.001, 1.0]], np.float32)
    assert wr.replay_packet(nodes, [0.1, 0.2, -1.0], dirs) == 5     # every node: both children wanted
    assert wr.replay_packet(nodes, [5.0, 5.0, -1.0], dirs) == 0
    assert wr.replay_packet(nodes, [0.1, 0.2, -1.0], dirs, active=[False, False]) == 0


def test_light_tracing_lds_entries_default():
    text = open(os.path.join(ROOT, "evplp_amd", "csrc", "kernels.h")).read()
    m = re.search(r"#ifndef EVPLP_LT_STACK\s*\n#define EVPLP_LT_STACK (\d+)", text)
    assert m and int(m.group(1)) == wr.LT_LDS_ENTRIES == 20


SCENES = {"A": scenes.morton_chain, "B": scenes.morton_chain_full}


@pytest.fixture(scope="module", params=["A", "B"])
def chain_scene(request, oracle):
    sd = SCENES[request.param]()
    return request.param, sd, oa.Scene(sd)


def brute_closest(oracle, verts, o, d, tmin=1e-4, tmax=3e38):
    """nearest hit over all triangles by the triangle predicate alone; ties keep the lowest index (the loop ascends, the test is strict)"""
    best, bt = -1, tmax
    t, b, g = (C.c_float() for _ in range(3))
    for k in range(verts.shape[0]):
        v = verts[k]
        if oracle.evo_tri_test(oa.ptr(v[0:3]), oa.ptr(v[3:6]), oa.ptr(v[6:9]), oa.ptr(o), oa.ptr(d), tmin, 3e38, C.byref(t), C.byref(b), C.byref(g)):
            if t.value < bt:
                best, bt = k, t.value
    return best, bt


def test_the_scenes_are_what_they_claim(chain_scene):
    name, sd, s = chain_scene
    v = s.verts.reshape(-1, 3, 3)
    ctr = 0.5 * (v.min(axis=1) + v.max(axis=1))
    assert ctr.min(axis=0).tolist() == [0.0, 0.0, -2.0] and ctr.max(axis=0)[1:].tolist() == [1.0, 2.0], "the box the LBVH builders quantise"
    assert ctr.max(axis=0)[0] == (np.float32(1.04) if name == "A" else 1.0)
    sheets = sd.meshes[sd.sheet_mesh]["idx"].shape[0]
    assert sheets == (105 if name == "A" else 290) and sd.light_count == 2
    if name == "B":
        # every cluster: one box centre, and a Morton code of its own with one bit beside the shared top z bit
        first = v.shape[0] - sheets
        c = ctr[first:].reshape(58, 5, 3).astype(np.float64)
        assert (c == c[:, :1]).all()
        q = np.floor((c[:, 0] - [0, 0, -2]) / [1, 1, 4] * 2 ** 21).astype(np.int64)
        assert (q[:, 2] >= 2 ** 20).all()
        q[:, 2] -= 2 ** 20
        assert sorted(np.count_nonzero(q, axis=1).tolist()) == [0] + [1] * 57
        bits = q.sum(axis=1)
        assert (bits & (bits - 1) == 0).all() and len({tuple(r) for r in q.tolist()}) == 58


def test_oracle_stack_on_the_chain_scenes(chain_scene):
    """evo_closest / evo_occluded keep stack[128] and pop one node to push two: levels + 1 entries at most.  The restated tree can differ
    from the oracle's by a rounding in a bin index, which moves a triangle to a sibling; a factor of two covers that."""
    _, _, s = chain_scene
    assert 2 * (wr.oracle_tree_levels(s.verts) + 1) <= 128


def test_oracle_walks_match_brute_force_on_the_chain_scenes(chain_scene, oracle):
    _, sd, s = chain_scene
    rng = np.random.RandomState(8)
    rays = []
    for k in range(24):                                             # along +z and -z through the whole stack of sheets, slightly off axis
        x, y = rng.rand(2) * 1.2 - 0.1
        rays.append(([x, y, -1.5], [0.01 * rng.randn(), 0.01 * rng.randn(), 1.0]))
        rays.append(([x, y, 1.5], [0.01 * rng.randn(), 0.01 * rng.randn(), -1.0]))
    rays.append(([0.0, 0.0, -1.5], [0.0, 0.0, 1.0])); rays.append(([0.25, 0.5, 1.5], [0.0, 0.0, -1.0]))     # and exactly on it
    for k in range(80):
        rays.append((rng.rand(3) * [6, 6, 4] - [3, 3, 2], rng.randn(3)))
    t, b, g = (C.c_float() for _ in range(3))
    hits = 0
    for o, d in rays:
        o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
        tri = oracle.evo_closest(s.h, oa.ptr(o), oa.ptr(d), 1e-4, 3e38, 0, C.byref(t), C.byref(b), C.byref(g))
        best, bt = brute_closest(oracle, s.verts, o, d)
        assert tri == best and (tri < 0 or t.value == bt), (o, d, tri, best)
        hits += tri >= 0
        for far in (0.5, 1.0 - 1e-4, 50.0):
            assert oracle.evo_occluded(s.h, oa.ptr(o), oa.ptr(d), 1e-4, far) == oracle.evo_occluded_brute(s.h, oa.ptr(o), oa.ptr(d), 1e-4, far)
    assert hits > len(rays) // 2
