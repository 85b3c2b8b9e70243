"""The PLOC builder without a GPU: evplp_ploc_tree, the host twin of the device builder EVPLP_BVH_PLOC_GPU (exported, bound, declared, refusing
what it must), against a brute-force restatement of the algorithm in numpy fp32 written here (same Morton key, same distance, same tie rule), on
the edge cases where a wrong tie rule loops or pairs what is not mutual, in the pairing phase where the answer is known, and against a Karras
radix tree of the same keys under the SAH cost of DESIGN section 6b.  The helpers that turn a tree into nested tuples serve test_gpu_ploc.py too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MAX_LEAF = 4


def soup(seed, n_boxes, tess):
    return scenes.box_room(seed=seed, n_boxes=n_boxes, tess=tess, aspect=1.5).triangle_soup()[0]


@pytest.fixture(scope="module")
def room490():
    return soup(3, 6, 2)


@pytest.fixture(scope="module")
def room1198():
    return soup(11, 7, 3)


# ---- the restatement
def has_area(v9):
    """meshBound's rule in fp32, every operation on its own"""
    v = np.asarray(v9, F).reshape(-1, 9)
    a, b = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        area = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    return (area > 0) & (area <= F(3.4028235e38))


def expand21(v):
    v = v & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(s))) & np.uint64(m)
    return v


def morton_order(v9):
    """(the valid triangles in Morton order, equal keys in triangle order; their keys; boxes lo, hi of ALL triangles)"""
    T = np.asarray(v9, F).reshape(-1, 3, 3)
    lo, hi = T.min(1), T.max(1)
    ids = np.nonzero(has_area(v9))[0]
    if len(ids) == 0:
        return ids.astype(np.int32), np.zeros(0, np.uint64), lo, hi
    c = F(0.5) * (lo[ids] + hi[ids])
    clo, chi = c.min(0), c.max(0)
    ext = np.maximum(chi - clo, F(1e-30))
    t = np.clip((c.astype(np.float64) - clo.astype(np.float64)) / ext.astype(np.float64), 0.0, 1.0)
    q = np.minimum(t * 2097152.0, 2097151.0).astype(np.uint64)
    k = (expand21(q[:, 0]) << np.uint64(2)) | (expand21(q[:, 1]) << np.uint64(1)) | expand21(q[:, 2])
    o = np.argsort(k, kind="stable")
    return ids[o].astype(np.int32), k[o], lo, hi


def distances(lo, hi, i, j0, j1):
    """d(i, j) for j in [j0, j1]: fp32 arrays, one rounding per operation, (ex ey + ey ez) + ez ex"""
    e = np.maximum(np.maximum(hi[i], hi[j0:j1 + 1]) - np.minimum(lo[i], lo[j0:j1 + 1]), F(0))
    assert e.dtype == F
    return e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]


def brute_ploc(v9, radius, search_iterations=128):
    """(order, children [n - 1, 2], iterations): the builder's steps, an O(c r) loop per iteration"""
    order, _, tlo, thi = morton_order(v9)
    n = len(order)
    ref, lo, hi = [~p for p in range(n)], tlo[order].copy(), thi[order].copy()
    children = np.zeros((max(n - 1, 0), 2), np.int32)
    it = 0
    while len(ref) > 1:
        c = len(ref)
        if it < search_iterations:
            nn = []
            for i in range(c):
                j0, j1 = max(0, i - radius), min(c - 1, i + radius)
                d = distances(lo, hi, i, j0, j1)
                d[i - j0] = np.inf
                cand = [j for j in range(j0, j1 + 1) if j != i]
                best = cand[0]
                for j in cand[1:]:                                        # ties keep the lowest j
                    if d[j - j0] < d[best - j0]:
                        best = j
                nn.append(best)
        else:
            nn = [i ^ 1 if (i ^ 1) < c else i for i in range(c)]
        lower = [nn[i] > i and nn[nn[i]] == i for i in range(c)]
        m, rank = sum(lower), 0
        assert m >= 1, "an iteration without a mutual pair"
        nref, nlo, nhi = [], [], []
        for i in range(c):
            j = nn[i]
            if j != i and nn[j] == i and j < i:
                continue
            if lower[i]:
                idx = c - 1 - m + rank
                rank += 1
                children[idx] = (ref[i], ref[j])
                nref.append(idx); nlo.append(np.minimum(lo[i], lo[j])); nhi.append(np.maximum(hi[i], hi[j]))
            else:
                nref.append(ref[i]); nlo.append(lo[i]); nhi.append(hi[i])
        ref, lo, hi = nref, np.array(nlo, F), np.array(nhi, F)
        it += 1
    return order, children, it


# ---- trees as data
def check_tree(children, n):
    """every inner index 0 .. n - 2 once as a child, except 0; every leaf once; all of it reachable from node 0"""
    if n <= 1:
        assert len(children) == 0
        return
    assert children.shape == (n - 1, 2)
    flat = children.ravel()
    inner, leaves = flat[flat >= 0], ~flat[flat < 0]
    assert sorted(inner.tolist()) == list(range(1, n - 1)), "inner nodes as children"
    assert sorted(leaves.tolist()) == list(range(n)), "leaves as children"
    seen, stack = 0, [0]
    while stack:
        i = stack.pop()
        seen += 1
        stack.extend(int(c) for c in children[i] if c >= 0)
    assert seen == n - 1
    assert all(int(c) > i for i in range(n - 1) for c in children[i] if c >= 0), "a child's index is above its parent's"


def subtree_info(children, n):
    """(triangle count, binary height, kept-node height) per inner node; children have higher indices than their parents"""
    cnt, hb, hk = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    for i in range(n - 2, -1, -1):
        l, r = (int(x) for x in children[i])
        cnt[i] = (1 if l < 0 else cnt[l]) + (1 if r < 0 else cnt[r])
        hb[i] = 1 + max(0 if l < 0 else hb[l], 0 if r < 0 else hb[r])
        hk[i] = max(0 if l < 0 else hk[l], 0 if r < 0 else hk[r]) + (1 if cnt[i] > MAX_LEAF else 0)
    return cnt, hb, hk


def nested(order, children):
    """the collapsed tree as nested (left, right) tuples, a sorted tuple of ORIGINAL triangles per leaf block (subtrees of <= 4 triangles)"""
    n = len(order)
    if n == 0:
        return ()
    if n == 1:
        return (int(order[0]),)
    cnt, _, _ = subtree_info(children, n)
    done = {}
    for i in range(n - 2, -1, -1):                                           # children first
        if cnt[i] <= MAX_LEAF:
            tris, stack = [], [i]
            while stack:
                for c in children[stack.pop()]:
                    if c < 0:
                        tris.append(int(order[~int(c)]))
                    else:
                        stack.append(int(c))
            done[i] = tuple(sorted(tris))
        else:
            done[i] = tuple((int(order[~int(c)]),) if c < 0 else done[int(c)] for c in children[i])
    return done[0]


def karras(keys):
    """the radix tree of the keys made unique by their position (what hierarchy_kernel builds): children [n - 1, 2], parents before children"""
    n = len(keys)
    u = [(int(k) << 32) | p for p, k in enumerate(keys)]
    children, todo, nxt = [], [(0, 0, n - 1)], 1
    children.append([0, 0])
    while todo:
        i, a, b = todo.pop()
        bit = (u[a] ^ u[b]).bit_length() - 1
        lo_, hi_ = a, b                                                      # last position whose key agrees with the first above `bit`
        while lo_ < hi_:
            mid = (lo_ + hi_ + 1) // 2
            if (u[a] ^ u[mid]) >> bit == 0:
                lo_ = mid
            else:
                hi_ = mid - 1
        for s, (x, y) in enumerate(((a, lo_), (lo_ + 1, b))):
            if x == y:
                children[i][s] = ~x
            else:
                children.append([0, 0]); children[i][s] = nxt
                todo.append((nxt, x, y)); nxt += 1
    return np.array(children, np.int32).reshape(-1, 2)


def sah_cost(order, children, tlo, thi):
    """DESIGN section 6b on UNPADDED boxes, leaves of <= 4 triangles: (15 (root + kept inner children) + 40 sum(leaf area x pairs)) / root, in fp64"""
    n = len(order)
    cnt, _, _ = subtree_info(children, n)
    lo, hi = np.zeros((n - 1, 3)), np.zeros((n - 1, 3))
    box = lambda c: (tlo[order[~c]].astype(np.float64), thi[order[~c]].astype(np.float64)) if c < 0 else (lo[c], hi[c])
    for i in range(n - 2, -1, -1):
        (al, ah), (bl, bh) = box(int(children[i][0])), box(int(children[i][1]))
        lo[i], hi[i] = np.minimum(al, bl), np.maximum(ah, bh)
    area = lambda l, h: 2.0 * float((h - l)[0] * (h - l)[1] + (h - l)[1] * (h - l)[2] + (h - l)[2] * (h - l)[0])
    root, inner, pair = area(lo[0], hi[0]), 0.0, 0.0
    stack = [0]
    while stack:
        i = stack.pop()
        for c in (int(x) for x in children[i]):
            k = 1 if c < 0 else int(cnt[c])
            a = area(*box(c))
            if k <= MAX_LEAF:
                pair += a * ((k + 1) >> 1)
            else:
                inner += a; stack.append(c)
    return (15.0 * (root + inner) + 40.0 * pair) / root


def copies(k):
    tri = np.array([0.1, 0.2, 0.3, 1.1, 0.2, 0.4, 0.3, 1.2, 0.5], F)
    return np.tile(tri, (k, 1))


def strip(n, seed=1):
    """n separate triangles of one shape along x at uneven spacing (distinct Morton keys, in index order)"""
    rng = np.random.default_rng(seed)
    base = np.array([[0, 0, 0], [0.4, 0, 0], [0, 0.4, 0.1]], F)
    return np.stack([(base + np.array([k + 0.5 * rng.random(), 0, 0], F)).reshape(9) for k in range(n)]).astype(F) if n else np.zeros((0, 9), F)


# ---- the symbol
def test_the_entry_point_is_exported_bound_declared_and_refuses(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    assert hasattr(lib, "evplp_ploc_tree") and "evplp_ploc_tree" in evplp._SIGNATURES
    assert re.search(r"\bint\s+evplp_ploc_tree\s*\(", hdr)
    assert re.search(r"EVPLP_BVH_PLOC_GPU\s*=\s*4\b", hdr) and evplp.BVH_PLOC_GPU == 4
    types = open(os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")).read()
    assert re.search(r"kPlocRadius = (\d+), kPlocMaxRadius = 32, kPlocSearchIterations = 128;", types)
    assert int(re.search(r"kPlocRadius = (\d+)", types).group(1)) == evplp.PLOC_RADIUS and evplp.PLOC_MAX_RADIUS == 32 and evplp.PLOC_SEARCH_ITERATIONS == 128
    L = evplp.lib()
    v = strip(5)
    order, children, it = np.zeros(5, np.int32), np.zeros(8, np.int32), C.c_int32(0)
    args = lambda **kw: [kw.get("v", v.ctypes.data), 5, kw.get("r", 16), kw.get("s", 128), kw.get("o", order.ctypes.data), kw.get("c", children.ctypes.data), kw.get("i", C.byref(it))]
    assert L.evplp_ploc_tree(*args()) == 5
    for bad in (dict(v=None), dict(o=None), dict(c=None), dict(i=None), dict(r=0), dict(r=33), dict(r=-1), dict(s=-1), dict(s=129)):
        assert L.evplp_ploc_tree(*args(**bad)) == evplp.ERR_INVALID, bad
    assert L.evplp_ploc_tree(v.ctypes.data, -1, 16, 128, order.ctypes.data, children.ctypes.data, C.byref(it)) == evplp.ERR_INVALID
    assert L.evplp_ploc_tree(*args(r=1)) == 5 and L.evplp_ploc_tree(*args(r=32)) == 5
    with pytest.raises(evplp.EvplpError):
        evplp.ploc_tree(v, radius=33)
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)


# ---- the reference
@pytest.mark.parametrize("radius", [1, 2, 16])
def test_the_twin_equals_the_restatement(evplp, room490, radius):
    assert room490.shape[0] == 490
    order, children, it = evplp.ploc_tree(room490, radius)
    want_order, want_children, want_it = brute_ploc(room490, radius)
    assert np.array_equal(order, want_order)
    assert it == want_it and it <= 128 + 9
    assert np.array_equal(children, want_children)
    check_tree(children, len(order))


def test_the_tree_is_valid_and_the_same_twice(evplp, room1198):
    a = evplp.ploc_tree(room1198)
    b = evplp.ploc_tree(room1198.copy())
    n = len(a[0])
    assert n == int(has_area(room1198).sum()) and sorted(a[0].tolist()) == np.nonzero(has_area(room1198))[0].tolist()
    check_tree(a[1], n)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- edges
@pytest.mark.parametrize("n", [0, 1, 2, 5])
@pytest.mark.parametrize("radius", [1, 16, 32])
def test_small_inputs_and_windows_that_cover_everything(evplp, n, radius):
    v = strip(n)
    order, children, it = evplp.ploc_tree(v, radius)
    assert order.tolist() == list(range(n))
    check_tree(children, n)
    want = brute_ploc(v, radius)
    assert np.array_equal(children, want[1]) and it == want[2]
    assert it == 0 if n < 2 else 1 <= it <= n - 1
    if n == 2:
        assert children.tolist() == [[~0, ~1]] and it == 1


@pytest.mark.parametrize("radius", [1, 2, 16, 32])
def test_sixty_four_copies_of_one_triangle(evplp, radius):
    """every key and every distance ties: position 0 and 1 are the one mutual pair of every iteration"""
    v = copies(64)
    order, children, it = evplp.ploc_tree(v, radius)
    assert order.tolist() == list(range(64))
    check_tree(children, 64)
    want = brute_ploc(v, radius)
    assert np.array_equal(children, want[1]) and it == want[2] == 63
    _, hb, _ = subtree_info(children, 64)
    assert hb[0] == 63


def test_a_triangle_without_area_is_left_out(evplp):
    v = strip(7)
    v[3, 3:6] = v[3, 0:3]; v[3, 6:9] = v[3, 0:3]
    order, children, it = evplp.ploc_tree(v, 2)
    assert order.tolist() == [0, 1, 2, 4, 5, 6]
    check_tree(children, 6)
    keep = np.array([0, 1, 2, 4, 5, 6])
    o2, c2, it2 = evplp.ploc_tree(v[keep], 2)
    assert np.array_equal(children, c2) and it == it2 and np.array_equal(keep[o2], order)
    assert np.array_equal(children, brute_ploc(v, 2)[1])
    assert evplp.ploc_tree(np.zeros((3, 9), F))[0].size == 0                       # nothing valid at all


# ---- the pairing phase
def test_pure_pairing_gives_the_known_tree(evplp, room490):
    order, children, it = evplp.ploc_tree(strip(5), 16, 0)
    assert it == 3 and children.tolist() == [[1, ~4], [2, 3], [~0, ~1], [~2, ~3]]
    for v in (room490, strip(33), strip(64)):
        order, children, it = evplp.ploc_tree(v, 16, 0)
        n = len(order)
        lg = (n - 1).bit_length()
        check_tree(children, n)
        _, hb, _ = subtree_info(children, n)
        assert it == lg and hb[0] == lg, (n, it, hb[0])
        # iteration k pairs neighbours: the leaves under every node are a run of positions, in order
        spans = {}
        for i in range(n - 2, -1, -1):
            (a0, a1), (b0, b1) = ((~int(c), ~int(c)) if c < 0 else spans[int(c)] for c in children[i])
            assert b0 == a1 + 1
            spans[i] = (a0, b1)
        assert spans[0] == (0, n - 1)
        assert np.array_equal(children, brute_ploc(v, 16, 0)[1])


def test_three_search_iterations_then_pairing(evplp, room490):
    order, children, it = evplp.ploc_tree(room490, 16, 3)
    check_tree(children, len(order))
    assert it <= 3 + 9
    want = brute_ploc(room490, 16, 3)
    assert np.array_equal(children, want[1]) and it == want[2]


# ---- the cost
def test_the_ploc_tree_costs_less_than_the_radix_tree(evplp, room1198):
    order, children, it = evplp.ploc_tree(room1198, 16)
    want_order, keys, tlo, thi = morton_order(room1198)
    assert np.array_equal(order, want_order) and len(order) == 1198
    ploc = sah_cost(order, children, tlo, thi)
    radix_children = karras(keys)
    check_tree(radix_children, len(order))
    radix = sah_cost(order, radix_children, tlo, thi)
    print(f"PLOC r = 16: cost {ploc:.3f}, radix tree {radix:.3f}, ratio {ploc / radix:.4f}, {it} iterations")
    assert ploc < radix, (ploc, radix)


# ---- the sanitisers
def test_the_twin_under_asan_and_ubsan(tmp_path):
    """a stand-alone host program (tools/host_fuzz/ploc_check.cpp): the edge cases above at every radius and iteration count, and 300 random soups"""
    import shutil
    import subprocess
    from test_kernel_resources import HIPCC
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    if shutil.which("g++") is None or not os.path.isdir(rocm_include):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "ploc_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-isystem", rocm_include, "-o", exe, os.path.join(ROOT, "tools", "host_fuzz", "ploc_check.cpp"), os.path.join(ROOT, "evplp_amd", "csrc", "host", "ploc.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"trees (\d+) refused (\d+)", r.stdout)
    assert m and int(m.group(1)) > 400 and int(m.group(2)) == 9, r.stdout
