"""Tree rotations without a GPU: the entry points of evplp_optimize_accel / evplp_set_refit_rotations (exported, bound, declared, refusing
null handles; the ABI version unchanged) and evplp_rotate_tree, the host twin of the rotating refit sweep -- against a brute-force numpy
restatement of the rule reference for reference, against the properties a rotated tree must keep (the level condition's three consequences
among them), on hand-made cases with one written-down answer each, its four-wide stack need against evplp_build_accel's sweep and a
recursive restatement, and the "rotations" key of the technique JSON's "animation" block."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import rotate_restate as rr
import scenes
from rotate_restate import NO, F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_optimize_accel", "evplp_set_refit_rotations", "evplp_rotation_info", "evplp_rotate_tree", "evplp_group_optimize_accel", "evplp_group_set_refit_rotations")
PASSES = 3


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    n = C.c_int32(0)
    assert L.evplp_optimize_accel(None, 1, C.byref(n)) == evplp.ERR_INVALID
    assert L.evplp_set_refit_rotations(None, 1) == evplp.ERR_INVALID
    assert L.evplp_rotation_info(None, None, None, None, None) == evplp.ERR_INVALID
    assert L.evplp_group_optimize_accel(None, 1, C.byref(n)) == evplp.ERR_INVALID
    assert L.evplp_group_set_refit_rotations(None, 1) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for m in ("optimize_accel", "set_refit_rotations"):
        assert callable(getattr(evplp.Context, m)) and callable(getattr(evplp.Group, m)), m
    assert callable(evplp.Context.rotation_info) and callable(evplp.rotate_tree)
    # the twin's own refusals
    nodes, ti, v = rr.random_tree(evplp, 9, seed=1)
    for passes in (0, 9, -1):
        with pytest.raises(evplp.EvplpError):
            evplp.rotate_tree(nodes, ti, v, passes)
    bad = nodes.copy(); bad[0]["c0"] = 0                                      # a self-loop
    with pytest.raises(evplp.EvplpError):
        evplp.rotate_tree(bad, ti, v, 1)
    with pytest.raises(evplp.EvplpError):                                     # levels that are no schedule: everything on one level
        evplp.rotate_tree(nodes, ti, v, 1, level=np.zeros(len(nodes), np.int32))


def test_the_header_and_the_sources_state_the_rule_once():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("level(A) < level(B)", "ties keep the first candidate", "it is no longer free of host waits", "0 = off, the default",
                   "sets evplp_accel_quality's last_action to 3", "12 B per node"):
        assert needle in hdr, needle
    csrc = os.path.join(ROOT, "evplp_amd", "csrc")
    types = open(os.path.join(csrc, "evplp_types.h")).read()
    assert types.count("inline int rotate_choice(") == 1
    fn = types[types.index("inline int rotate_choice("):]
    fn = fn[:fn.index("\n}\n")]
    assert "#pragma clang fp contract(off)" in fn and "fma" not in fn and fn.count("ploc_distance(") == 2
    for f in ("bvh_gpu.hip", os.path.join("host", "rotate.cpp")):                # both sides decide with it, and with nothing else
        text = open(os.path.join(csrc, f)).read()
        assert text.count("rotate_choice(") == 1, f
    assert "ploc_distance" not in open(os.path.join(csrc, "host", "rotate.cpp")).read()


# ---- 1: the twin against the brute-force restatement
def inputs(evplp):
    out = []
    for leaves, seed in ((2, 1), (3, 2), (4, 3), (5, 4), (9, 5), (17, 6), (40, 7), (97, 8), (200, 9)):
        out.append((f"random, {leaves} leaves", rr.random_tree(evplp, leaves, seed)))
    out.append(("a pure chain", rr.chain(evplp, 30)))
    out.append(("absent children", rr.random_tree(evplp, 60, seed=11, absent=0.2)))
    out.append(("a leaf with an empty box", rr.random_tree(evplp, 40, seed=12, empty_leaf=True)))
    return out


def test_the_twin_equals_the_brute_force_restatement(evplp):
    total = 0
    for name, (nodes, ti, v) in inputs(evplp):
        level, _, _ = evplp.refit_levels(nodes, level_capacity=len(nodes))
        children = np.stack([nodes["c0"], nodes["c1"]], axis=1)
        brute = rr.Brute(children, ti, v, level)
        counts = []
        for p in range(1, PASSES + 1):
            counts.append(brute.sweep())
            got = evplp.rotate_tree(nodes, ti, v, p)
            assert np.array_equal(got["children"], brute.children()), f"{name}: references after pass {p}"
            assert got["rotations"] == counts, f"{name}: rotations per pass"
            assert got["need0"] == brute.need(0), f"{name}: the root's stack need after pass {p}"
            for i in brute.order:
                lo, hi = brute.box(i)
                assert np.array_equal(got["boxes"][i], np.concatenate([lo, hi]).astype(F)), f"{name}: box of node {i} after pass {p}"
        print(f"{name}: {len(nodes)} nodes, rotations per pass {counts}")
        total += sum(counts)
        if name in ("random, 200 leaves", "a pure chain", "absent children", "a leaf with an empty box"):
            assert counts[0] > 0, f"{name}: nothing rotates, the case shows nothing"
    assert total > 100


# ---- 2: what every pass keeps
def chain_scene_tree(evplp, builder):
    """scenes.morton_chain's geometry under the host PLOC twin's tree, or under the radix tree of its Morton keys (what the LBVH builders
    make of it: a chain of two dozen levels; test_ploc_host.py's restatement), flattened to 64-byte nodes"""
    from test_ploc_host import karras, morton_order
    sd = scenes.morton_chain()
    soup = sd.triangle_soup()[0].astype(F).reshape(-1, 9)
    if builder == "ploc":
        order, children, _ = evplp.ploc_tree(soup)
    else:
        order, keys, _, _ = morton_order(soup)
        children = karras(keys)
    nodes, ti = rr.flatten_binary(evplp, order, children)
    return nodes, ti, soup


def test_every_pass_keeps_the_tree_the_plan_and_the_depth_and_shrinks_the_metric(evplp):
    cases = inputs(evplp) + [("morton chain under PLOC", chain_scene_tree(evplp, "ploc")), ("morton chain under the radix tree", chain_scene_tree(evplp, "radix"))]
    rotated_somewhere = 0
    for name, (nodes, ti, v) in cases:
        n = len(nodes)
        level, order, begin = evplp.refit_levels(nodes, level_capacity=n)
        depth0 = rr.depth_of(np.stack([nodes["c0"], nodes["c1"]], axis=1))
        assert depth0 == len(begin) - 1
        # the state before: the twin's boxes of the unrotated tree are those of a pass that may not rotate -- every node on its own level 0 .. n - 1
        # cannot be had, so the boxes come from the brute force
        brute = rr.Brute(np.stack([nodes["c0"], nodes["c1"]], axis=1), ti, v, level)
        boxes = np.zeros((n, 6), F)
        for i in brute.order:
            boxes[i] = np.concatenate(brute.box(i))
        state, cur = {"children": brute.children(), "boxes": boxes}, nodes
        for p in range(6):
            got = evplp.rotate_tree(cur, ti, v, 1, level=level)                 # one more pass over the plan the tree was given at the start
            took = got["rotations"][0]
            cur = rr.check_kept(evplp, cur, level, state, got, took > 0)
            assert rr.depth_of(got["children"]) <= depth0, f"{name}: pass {p} made a path longer"
            state = got
            rotated_somewhere += took
            if took == 0:
                break
        # several passes in one call are the same passes
        many = evplp.rotate_tree(nodes, ti, v, 4)
        step, cur2 = [], nodes
        for p in range(4):
            g = evplp.rotate_tree(cur2, ti, v, 1, level=level)
            step.append(g["rotations"][0]); cur2 = g["nodes"]
        assert many["rotations"] == step and np.array_equal(many["children"], g["children"]), name
        print(f"{name}: {n} nodes, {len(begin) - 1} levels, rotations {many['rotations']}")
        if name == "morton chain under the radix tree":
            assert len(begin) - 1 >= 20 and many["rotations"][0] > 0, "the chain scene is no chain, or nothing rotates on it"
    assert rotated_somewhere > 100


# ---- 3: hand-made cases.  A leaf L(x, w) is one triangle spanning [x, x + w] x [0, 1] x [0, 1]: area(ex, 1, 1) = 2 ex + 1, all exact in fp32.
def hand(evplp, spec):
    """spec: [(c0, c1)] where a child is a node index or ('L', x, w)"""
    soup = rr.Soup()
    kids = [tuple(c if isinstance(c, int) else soup.add([rr.tri_of_box((c[1], 0, 0), (c[1] + c[2], 1, 1))]) for c in pair) for pair in spec]
    ti, v = soup.arrays()
    return rr.node_array(evplp, kids), ti, v


def L(x, w=1):
    return ("L", x, w)


def test_hand_made_level_refusal(evplp):
    """root -> (A, B), A = {L(0), L(1)} = [0, 2], area 5; B = {L(2), L(20)} = [2, 21], area 39.  Candidate (0, 1) -- A down, L(20) up, L(2)
    stays -- gains 39 - area([0, 3]) = 39 - 7 = 32; (0, 0) gains 39 - area([0, 21]) = -4; (1, .) move B under A and lose.  But A and B are
    both on plan level 0: level(A) < level(B) fails both ways and NOTHING is taken.  Under the plan (root 2, A 0, B 1) -- as valid a schedule --
    (0, 1) is taken: root = (L(20), B), B = (L(2), A)."""
    nodes, ti, v = hand(evplp, [(1, 2), (L(0), L(1)), (L(2), L(20))])
    got = evplp.rotate_tree(nodes, ti, v, 2)
    assert got["rotations"] == [0, 0] and np.array_equal(got["children"], np.stack([nodes["c0"], nodes["c1"]], axis=1))
    got = evplp.rotate_tree(nodes, ti, v, 1, level=[2, 0, 1])
    l20, l2 = int(nodes[2]["c1"]), int(nodes[2]["c0"])
    assert got["rotations"] == [1] and got["children"].tolist() == [[l20, 2], [int(nodes[1]["c0"]), int(nodes[1]["c1"])], [l2, 1]]
    assert got["boxes"][2].tolist() == [0, 0, 0, 3, 1, 1] and got["boxes"][0].tolist() == [0, 0, 0, 21, 1, 1]


def test_hand_made_tie_keeps_the_first_candidate(evplp):
    """root -> (A = L(10), B = {L(0), L(20)}): area(B) = 43; A u L(20) = [10, 21] and A u L(0) = [0, 11] both have area 23: candidates (0, 0) and
    (0, 1) both gain 20, and A is a leaf, so (1, .) do not exist.  The first, (0, 0), is taken: L(0) moves up, B = (A, L(20))."""
    nodes, ti, v = hand(evplp, [(L(10), 1), (L(0), L(20))])
    a, l0, l20 = int(nodes[0]["c0"]), int(nodes[1]["c0"]), int(nodes[1]["c1"])
    got = evplp.rotate_tree(nodes, ti, v, 1)
    assert got["rotations"] == [1] and got["children"].tolist() == [[l0, 1], [a, l20]]
    assert got["boxes"][1].tolist() == [10, 0, 0, 21, 1, 1]


def test_hand_made_gain_zero_is_not_taken(evplp):
    """root -> (A = L(0, 21), B = {L(0), L(20)}): A u K is [0, 21] = B's own box whichever child stays, so both gains are 43 - 43 = 0"""
    nodes, ti, v = hand(evplp, [(L(0, 21), 1), (L(0), L(20))])
    got = evplp.rotate_tree(nodes, ti, v, 3)
    assert got["rotations"] == [0, 0, 0] and np.array_equal(got["children"], np.stack([nodes["c0"], nodes["c1"]], axis=1))
    # ... and the smallest positive gain is: A one float shorter on the right, K = L(0) -> area([0, 21 - ulp]) < 43
    nodes, ti, v = hand(evplp, [(L(0, float(np.nextafter(F(21), F(0)))), 1), (L(0), L(20))])
    assert evplp.rotate_tree(nodes, ti, v, 1)["rotations"] == [1]


# ---- 4: the four-wide stack need
def test_the_stack_need_is_build_accels_sweep_and_the_recursive_restatement(evplp):
    for leaves, seed in ((2, 1), (7, 2), (33, 3), (150, 4)):
        nodes, ti, v = rr.random_tree(evplp, leaves, seed, absent=0.1, ordered=True, same_box=True)       # every gain is 0: nothing rotates
        got = evplp.rotate_tree(nodes, ti, v, 2)
        children = np.stack([nodes["c0"], nodes["c1"]], axis=1)
        assert got["rotations"] == [0, 0] and np.array_equal(got["children"], children)
        assert got["need0"] == rr.backward_need(children), leaves
    for name, (nodes, ti, v) in inputs(evplp):
        got = evplp.rotate_tree(nodes, ti, v, PASSES)
        level, _, _ = evplp.refit_levels(nodes, level_capacity=len(nodes))
        assert got["need0"] == rr.Brute(got["children"], ti, v, level).need(0), name


def test_the_twin_under_asan_and_ubsan(tmp_path):
    """a stand-alone host program (tools/host_fuzz/rotate_fuzz.cpp): 20 000 seeded node arrays, a quarter of them no trees"""
    import shutil
    import subprocess
    from test_kernel_resources import HIPCC
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    if shutil.which("g++") is None or not os.path.isdir(rocm_include):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "rotate_fuzz")
    host = os.path.join(ROOT, "evplp_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-isystem", rocm_include, "-o", exe, os.path.join(ROOT, "tools", "host_fuzz", "rotate_fuzz.cpp"), os.path.join(host, "rotate.cpp"), os.path.join(host, "refit_levels.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"rotated (\d+) refused (\d+) rotations (\d+)", r.stdout)
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) > 2000 and int(m.group(3)) > 5000, r.stdout


# ---- 5: the "rotations" key of the "animation" block (tests/test_transform_host.py's way)
W, H = 96, 64
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _render(evplp, path, overrides=None):
    err = C.create_string_buffer(1024)
    rc = evplp.lib().evplp_render_json(str(path).encode(), overrides.encode() if overrides else None, 0, err, 1024)
    return rc, err.value.decode()


def _anim(**kw):
    block = {"frames": 2, "tracks": [{"mesh": 0, "matrices": [EYE] * 2}]}
    block.update(kw)
    return json.dumps({"animation": block})


@pytest.fixture
def technique_file(evplp, tmp_path):
    root = json.load(open(evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)))
    root["photonfam"]["timeLimitMs"] = 1e9
    root["photonfam"]["numMaxIteration"] = 2
    jp = tmp_path / "photonfam.json"
    jp.write_text(json.dumps(root))
    return jp


def test_the_rotations_key_is_refused_by_name_and_accepted_in_range(evplp, technique_file, tmp_path):
    for bad in (-1, 9, 2.5, "2", True, [2], 1e10):
        rc, msg = _render(evplp, technique_file, _anim(rotations=bad))
        assert rc == evplp.ERR_PARSE and "animation.rotations" in msg, (bad, rc, msg)
    written = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".pfm", ".ppm", ".png", ".exr"))
    assert not written, written
    # in range: past validation -- whatever a plain animation of this file comes to on this machine, these come to as well
    rc_plain, msg_plain = _render(evplp, technique_file, _anim())
    for good in (0, 1, 8, 2.0):
        rc, msg = _render(evplp, technique_file, _anim(rotations=good))
        assert rc != evplp.ERR_PARSE and rc == rc_plain, (good, rc, msg, rc_plain, msg_plain)
