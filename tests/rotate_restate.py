"""Helpers of the tree-rotation tests (test_rotate_host.py, test_gpu_rotate.py): small trees with real triangles under their leaves, a
brute-force numpy restatement of the rule of evplp_optimize_accel / evplp_rotate_tree (include/evplp.h), the four-wide stack need restated
recursively and as evplp_build_accel's backward sweep, and the properties a rotated tree must keep.  No GPU, no test in here."""
import math

import numpy as np

F = np.float32
NO = -2 ** 31
EMPTY = (np.full(3, 3.0e38, F), np.full(3, -3.0e38, F))


def leaf(block, cnt):
    return ~((block << 2) | (cnt - 1))


def tri_of_box(lo, hi):
    """one triangle whose bounding box is [lo, hi] exactly"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    return np.array([lo[0], lo[1], lo[2], hi[0], hi[1], lo[2], lo[0], hi[1], hi[2]], F)


class Soup:
    """leaf blocks with their triangles: add(boxes) -> the leaf reference"""

    def __init__(self):
        self.tri_index, self.verts = [], []

    def add(self, tris):
        block = len(self.tri_index) // 4
        for k in range(4):
            if k < len(tris):
                self.tri_index.append(len(self.verts)); self.verts.append(np.asarray(tris[k], F))
            else:
                self.tri_index.append(-1)
        return leaf(block, len(tris))

    def arrays(self):
        return np.array(self.tri_index, np.int32), np.array(self.verts, F).reshape(-1, 9)


def node_array(evplp, children):
    n = np.zeros(len(children), evplp.ACCEL_NODE)
    for i, (a, b) in enumerate(children):
        n[i]["c0"], n[i]["c1"] = a, b
    return n


def random_tree(evplp, leaves, seed, absent=0.0, empty_leaf=False, ordered=False, same_box=False):
    """a random binary tree with `leaves` leaf slots (some absent), stored in a random order but for the root (ordered: in pre-order), with
    random boxes of one to four triangles under every leaf; returns (nodes, tri_index, verts9)"""
    rng = np.random.RandomState(seed)
    n = max(leaves - 1, 1)
    kids = [[None, None] for _ in range(n)]
    free = [(0, 0), (0, 1)]
    for k in range(1, n):
        p, s = free.pop(rng.randint(len(free)))
        kids[p][s] = k
        free += [(k, 0), (k, 1)]
    soup = Soup()
    for j, (p, s) in enumerate(free):
        if (leaves == 1 and j == 1) or rng.rand() < absent:
            kids[p][s] = NO
            continue
        ctr, half = rng.uniform(0, 10, 3), rng.uniform(0.05, 0.8, 3)
        if same_box:
            ctr, half = np.full(3, 5.0), np.full(3, 0.5)
        lo, hi = (ctr - half).astype(F), (ctr + half).astype(F)
        tris = [tri_of_box(lo, hi)] + [rng.uniform(lo, hi, (3, 3)).astype(F).reshape(9) for _ in range(rng.randint(4))]
        if empty_leaf and j == len(free) // 2:
            tris = [np.tile(lo, 3).astype(F)]                              # a triangle without area: the leaf's box is empty
        kids[p][s] = soup.add(tris)
    if ordered:                                                            # pre-order: a depth-first numbering from the root
        name, stack = {}, [0]
        while stack:
            k = stack.pop(); name[k] = len(name)
            stack += [c for c in reversed(kids[k]) if c is not None and c >= 0]
        name = [name[k] for k in range(n)]
    else:
        name = np.concatenate([[0], 1 + rng.permutation(n - 1)]).tolist()
    stored = [None] * n
    for k in range(n):
        stored[name[k]] = tuple(int(name[c]) if c >= 0 else int(c) for c in kids[k])
    ti, v = soup.arrays()
    return node_array(evplp, stored), ti, v


def chain(evplp, n, seed=2):
    """a pure chain: node i = (a leaf, node i + 1); the leaves lie in a random order along x"""
    rng = np.random.RandomState(seed)
    soup = Soup()
    xs = rng.permutation(n + 1).astype(F) * F(1.5)
    refs = [soup.add([tri_of_box((x, 0, 0), (x + 1, 1, 1))]) for x in xs]
    kids = [(refs[i], i + 1) for i in range(n - 1)] + [(refs[n - 1], refs[n])]
    ti, v = soup.arrays()
    return node_array(evplp, kids), ti, v


# ---- the rule, restated by brute force: every box from the triangles under it, every time
def area(lo, hi):
    e = np.maximum((hi - lo).astype(F), F(0))
    return F(F(F(e[0] * e[1]) + F(e[1] * e[2])) + F(e[2] * e[0]))


def has_area(v):
    a, b = (v[3:6] - v[0:3]).astype(F), (v[6:9] - v[0:3]).astype(F)
    c = np.array([F(a[1] * b[2]) - F(a[2] * b[1]), F(a[2] * b[0]) - F(a[0] * b[2]), F(a[0] * b[1]) - F(a[1] * b[0])], F)
    with np.errstate(over="ignore"):
        ar = np.sqrt(F(F(F(c[0] * c[0]) + F(c[1] * c[1])) + F(c[2] * c[2])))
    return bool(ar > 0 and np.isfinite(ar))


class Brute:
    def __init__(self, children, tri_index, verts9, level):
        self.kids = [[int(a), int(b)] for a, b in children]
        self.ti, self.v = np.asarray(tri_index), np.asarray(verts9, F).reshape(-1, 9)
        self.level = [int(x) for x in level]
        self.order = sorted((i for i in range(len(self.kids)) if self.level[i] >= 0), key=lambda i: (self.level[i], i))
        self.live = [has_area(t) for t in self.v]

    def box(self, ref):
        if ref == NO:
            return EMPTY
        if ref < 0:
            blk, cnt = (~ref) >> 2, ((~ref) & 3) + 1
            tris = [t for t in self.ti[4 * blk:4 * blk + cnt] if t >= 0 and self.live[t]]
            if not tris:
                return EMPTY
            pts = self.v[tris].reshape(-1, 3)
            return pts.min(0), pts.max(0)
        (alo, ahi), (blo, bhi) = self.box(self.kids[ref][0]), self.box(self.kids[ref][1])
        return np.minimum(alo, blo), np.maximum(ahi, bhi)

    def lvl(self, ref):
        return self.level[ref] if ref >= 0 else -1

    def sweep(self):
        """one pass; returns the rotations taken"""
        taken = 0
        for n in self.order:
            c = self.kids[n]
            best, best_gain = None, F(0)
            for s in (0, 1):
                a, b = c[s], c[1 - s]
                if a == NO or b < 0 or not self.lvl(a) < self.lvl(b):
                    continue
                for q in (0, 1):
                    g, k = self.kids[b][q], self.kids[b][1 - q]
                    if g == NO or k == NO:
                        continue
                    boxes = [self.box(r) for r in (a, g, k)]
                    if any((hi < lo).any() for lo, hi in boxes):
                        continue
                    (alo, ahi), _, (klo, khi) = boxes
                    blo, bhi = self.box(b)
                    gain = F(area(blo, bhi) - area(np.minimum(alo, klo), np.maximum(ahi, khi)))
                    if gain > best_gain:
                        best, best_gain = (s, q), gain
            if best is not None:
                s, q = best
                a, b = c[s], c[1 - s]
                c[s], self.kids[b][q] = self.kids[b][q], a
                taken += 1
        return taken

    def need(self, i):
        """the four-wide walk's stack need of node i, recursively"""
        g = []
        for ch in self.kids[i]:
            g += self.kids[ch] if ch >= 0 else [ch]
        g = [x for x in g if x != NO]
        return max(len(g) - 1, 0) + max([self.need(x) for x in g if x >= 0] + [0])

    def children(self):
        return np.array(self.kids, np.int32)


def backward_need(children):
    """evplp_build_accel's sweep over a pre-ordered node array (children behind their parents); returns need[0]"""
    n = len(children)
    need = [0] * n
    for i in range(n - 1, -1, -1):
        g = []
        for ch in children[i]:
            ch = int(ch)
            if ch >= 0:
                assert ch > i, "not pre-ordered"
                g += [int(children[ch][0]), int(children[ch][1])]
            elif ch != NO:
                g.append(ch)
        g = [x for x in g if x != NO]
        need[i] = max(len(g) - 1, 0) + max([need[x] for x in g if x >= 0] + [0])
    return need[0]


# ---- what a rotated tree keeps
def leaf_refs(children, reached):
    return sorted(int(r) for i in reached for r in children[i] if r < 0 and r != NO)


def depth_of(children):
    """inner nodes on the longest path from the root"""
    d, stack = 0, [(0, 1)]
    while stack:
        i, k = stack.pop()
        d = max(d, k)
        stack += [(int(c), k + 1) for c in children[i] if c >= 0]
    return d


def inner_area_sum(children, boxes, reached):
    """the decision metric: the fp32 areas of the inner nodes' exact boxes, summed exactly"""
    return math.fsum(float(area(boxes[i][:3], boxes[i][3:])) for i in reached if not (boxes[i][3:] < boxes[i][:3]).any())


def check_kept(evplp, nodes_before, level, before, after, rotated):
    """before / after: dicts with children and boxes of two consecutive states of one tree (after: evplp.rotate_tree's result)"""
    n = len(nodes_before)
    raw = np.ascontiguousarray(nodes_before).view(np.uint8).reshape(-1, 64).copy()
    raw[:, 48:56] = np.ascontiguousarray(after["children"]).view(np.uint8).reshape(n, 8)
    h0, o0, _ = evplp.refit_levels(nodes_before, level_capacity=n)
    h1, o1, _ = evplp.refit_levels(raw, level_capacity=n)                    # permutation: still a tree ...
    assert sorted(o0.tolist()) == sorted(o1.tolist()), "the reached node set changed"
    assert leaf_refs(before["children"], o0) == leaf_refs(after["children"], o1), "the leaf references changed"
    for i in o1:                                                             # level order: the plan is still a schedule
        for c in after["children"][i]:
            if c >= 0:
                assert level[c] < level[i], (i, int(c))
    assert depth_of(after["children"]) <= int(max(level[i] for i in o1)) + 1, "a path is longer than the plan has levels"
    m0, m1 = inner_area_sum(before["children"], before["boxes"], o0), inner_area_sum(after["children"], after["boxes"], o1)
    if rotated:
        assert m1 < m0, (m0, m1)
    else:
        assert np.array_equal(before["children"], after["children"]), "a pass that took nothing changed a reference"
        assert m1 == m0
    return raw.reshape(-1).view(evplp.ACCEL_NODE)


def restate_structure(evplp, nodes, nodes4, ti, soup, pad):
    """What a refit writes for this topology, in numpy fp32 (tests/test_gpu_refit.py's restatement of set_box, the boxes and node4_kernel),
    against the downloaded bytes: every child box is the exact min / max of the live triangles under it, padded once; every four-wide node
    holds its binary node's grandchildren."""
    def set_box(lo, hi):
        lo, hi = (lo - pad).astype(F), (hi + pad).astype(F)
        c = (F(0.5) * (lo + hi)).astype(F)
        h = np.maximum(hi - c, c - lo).astype(F)
        return c, ((h + np.abs(h) * F(1e-6)).astype(F) + F(1e-30)).astype(F)

    def bits(a):
        return np.ascontiguousarray(a, F).view(np.uint32)

    _, order, _ = evplp.refit_levels(nodes, level_capacity=len(nodes))
    live = [has_area(t) for t in soup]
    lo, hi = np.zeros((len(nodes), 3), F), np.zeros((len(nodes), 3), F)
    done = np.zeros(len(nodes), bool)
    pending = list(order)
    while pending:                                                          # children before parents, whatever the levels are by now
        rest = []
        for i in pending:
            kids = [int(nodes[i]["c0"]), int(nodes[i]["c1"])]
            if any(ch >= 0 and not done[ch] for ch in kids):
                rest.append(i); continue
            blo, bhi = EMPTY[0].copy(), EMPTY[1].copy()
            for s, ch in enumerate(kids):
                if ch == NO:
                    assert np.all(nodes[i]["ctr"][:, s] == 0) and np.all(nodes[i]["hal"][:, s] == F(-3.0e38))
                    continue
                if ch >= 0:
                    clo, chi = lo[ch], hi[ch]
                else:
                    blk, cnt = (~ch) >> 2, ((~ch) & 3) + 1
                    tris = [t for t in ti[4 * blk:4 * blk + cnt] if t >= 0 and live[t]]
                    pts = soup[tris].reshape(-1, 3)
                    clo, chi = (pts.min(0), pts.max(0)) if tris else EMPTY
                ctr, hal = set_box(clo, chi)
                assert np.array_equal(bits(nodes[i]["ctr"][:, s]), bits(ctr)) and np.array_equal(bits(nodes[i]["hal"][:, s]), bits(hal)), (i, s, ch)
                blo, bhi = np.minimum(blo, clo), np.maximum(bhi, chi)
            lo[i], hi[i], done[i] = blo, bhi, True
        assert len(rest) < len(pending)
        pending = rest
    ctr, hal = nodes["ctr"], nodes["hal"]
    for i in range(len(nodes)):
        child = np.full(4, NO, np.int64); wlo = np.full((3, 4), 3.0e38, F); whi = np.full((3, 4), -3.0e38, F)
        for s, ch in enumerate((int(nodes[i]["c0"]), int(nodes[i]["c1"]))):
            if ch >= 0:
                child[2 * s], child[2 * s + 1] = nodes[ch]["c0"], nodes[ch]["c1"]
                wlo[:, 2 * s:2 * s + 2], whi[:, 2 * s:2 * s + 2] = ctr[ch] - hal[ch], ctr[ch] + hal[ch]
            elif ch != NO:
                child[2 * s] = ch
                wlo[:, 2 * s], whi[:, 2 * s] = ctr[i][:, s] - hal[i][:, s], ctr[i][:, s] + hal[i][:, s]
        assert np.array_equal(nodes4[i]["child"], child), i
        assert np.array_equal(bits(nodes4[i]["lo"]), bits(wlo)) and np.array_equal(bits(nodes4[i]["hi"]), bits(whi)), i
        assert not nodes4[i]["pad"].any()
    return len(order)


def flatten_binary(evplp, order, children):
    """evplp_ploc_tree's binary tree (one triangle per leaf) as 64-byte nodes over leaf blocks of up to four triangles, the way the device
    builder collapses it; returns (nodes, tri_index)"""
    n = len(order)
    count = {}

    def cnt(r):
        if r < 0:
            return 1
        if r not in count:
            count[r] = cnt(int(children[r][0])) + cnt(int(children[r][1]))
        return count[r]

    def positions(r):
        return [~r] if r < 0 else positions(int(children[r][0])) + positions(int(children[r][1]))

    soup_ti, out, ids = [], [], {}

    def block(r):
        ps = positions(r)
        b = len(soup_ti) // 4
        soup_ti.extend([int(order[p]) for p in ps] + [-1] * (4 - len(ps)))
        return leaf(b, len(ps))

    def emit(r):
        i = len(out); out.append(None)
        refs = []
        for c in (int(children[r][0]), int(children[r][1])):
            refs.append(emit(c) if cnt(c) > 4 else block(c))
        out[i] = tuple(refs)
        return i

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 100))
    if n <= 4:
        out.append((block(0) if n > 1 else leaf(0, 1), NO))
        if n == 1:
            soup_ti.extend([int(order[0]), -1, -1, -1])
    else:
        emit(0)
    return node_array(evplp, out), np.array(soup_ti, np.int32)
