"""Plain numpy replays of the BVH walks' stack use, from the node arrays a context downloads (Context.debug_accel(0) for the binary
nodes, debug_accel(4) for the four-wide ones).  No triangle is tested anywhere here: a ray's far bound stays where it started, so a
replayed ray enters at least the children the kernel's ray enters, in the same order as long as the kernel's ray has not hit yet.

  worst_case_entries(nodes)                the largest stack any ray can reach in closest_lane4, over all orders of descent
  replay_closest(nodes4, o, d, tmin)       closest_lane4's own order for given rays: the largest sp of each
  replay_packet(nodes, o, dirs)            the binary packet walk (closest_wave / occluded_wave) for one wave: the largest sp
  four_wide(nodes)                         bvh_gpu.hip's node4_kernel on the host (for hand-made trees)
  oracle_tree_levels(verts9)               the levels of the oracle's own tree (its walks keep stack[128])

Arithmetic: the kernels' slab tests are fma(plane, 1/d, -(o/d)) in fp32 with the hardware reciprocal (1 ulp).  Here the reciprocal is
the IEEE one and the fma is a product and a sum in fp64 rounded once more to fp32: the two can differ in the last bit of an entry
distance, which moves a ray that grazes a box edge and nothing else.
"""
import numpy as np

NO_CHILD = -2 ** 31
NODE = np.dtype([("ctr", np.float32, (3, 2)), ("hal", np.float32, (3, 2)), ("c0", np.int32), ("c1", np.int32), ("pad", np.int32, 2)])
NODE4 = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.int32, 4), ("pad", np.int32, 4)])
BIG = np.float32(3.0e38)
LT_LDS_ENTRIES = 20          # kernels.h EVPLP_LT_STACK: light tracing keeps this many entries in LDS, the rest in its global column


def four_wide(nodes):
    """node4[i] of binary node i: an inner child is replaced by its own two children, a leaf or an absent child stays (slots 2 s, 2 s + 1
    belong to child s)."""
    out = np.zeros(len(nodes), NODE4)
    out["child"] = NO_CHILD; out["lo"] = BIG; out["hi"] = -BIG
    for i, b in enumerate(nodes):
        for s, ch in enumerate((int(b["c0"]), int(b["c1"]))):
            if ch >= 0:
                c = nodes[ch]
                for q, g in enumerate((int(c["c0"]), int(c["c1"]))):
                    out["child"][i, 2 * s + q] = g
                    out["lo"][i, :, 2 * s + q] = c["ctr"][:, q] - c["hal"][:, q]
                    out["hi"][i, :, 2 * s + q] = c["ctr"][:, q] + c["hal"][:, q]
            elif ch != NO_CHILD:
                out["child"][i, 2 * s] = ch
                out["lo"][i, :, 2 * s] = b["ctr"][:, s] - b["hal"][:, s]
                out["hi"][i, :, 2 * s] = b["ctr"][:, s] + b["hal"][:, s]
    return out


def _children4(nodes):
    """(n, 4) child references of the four-wide walk, from four-wide nodes or from binary ones"""
    if "child" in (nodes.dtype.names or ()):
        return np.asarray(nodes["child"], np.int64)
    return np.asarray(four_wide(nodes)["child"], np.int64)


def worst_case_entries(nodes):
    """The largest number of entries closest_lane4's stack can hold on this tree.  A visit of a node with m present children leaves
    m - 1 of them on the stack and goes on with one; any of them can be that one (the order depends on the ray), and the stack is
    deepest when the one taken first is an inner node that is itself at its worst: W(i) = m - 1 + max(0, max W(inner child))."""
    ch = _children4(nodes)
    memo = {}

    def worst(i, seen):
        if i in memo:
            return memo[i]
        assert i not in seen, "the node array is not a tree"
        present = [int(c) for c in ch[i] if c != NO_CHILD]
        best = 0
        for first in present:
            if first >= 0:
                best = max(best, worst(first, seen | {i}))
        memo[i] = max(len(present) - 1, 0) + best
        return memo[i]
    return worst(0, frozenset()) if len(ch) else 0


def _rcp(d):
    d = np.asarray(d, np.float32)
    a = np.where(np.abs(d) < np.float32(1e-30), np.copysign(np.float32(1e-30), d), d).astype(np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / a).astype(np.float32)


def _fma(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def replay_closest(nodes4, o, d, tmin, tmax=3.0e38, cap=512):
    """closest_lane4 without its leaves: slab tests of the four stored boxes against [tmin, tmax], nearest first through the kernel's
    sorting network (ties keep the network's order), push c[3], c[2], c[1], descend into c[0]; a leaf is dropped where the kernel would
    test it.  o, d: (3,) or (n, 3).  Returns the largest sp of every ray (an int for one ray)."""
    one = np.ndim(o) == 1
    o = np.atleast_2d(np.asarray(o, np.float32)); d = np.atleast_2d(np.asarray(d, np.float32))
    n = o.shape[0]
    lo_all, hi_all, ch_all = nodes4["lo"], nodes4["hi"], nodes4["child"].astype(np.int64)
    inv = _rcp(d)
    with np.errstate(invalid="ignore", over="ignore"):
        noi = (-(o * inv)).astype(np.float32)
    tmin = np.float32(tmin); tmax = np.float32(tmax)
    stack = np.full((n, cap), NO_CHILD, np.int64)
    sp = np.zeros(n, np.int64); top = np.zeros(n, np.int64)
    cur = np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    while alive.any():
        inner = np.nonzero(alive & (cur >= 0))[0]
        leaf = np.nonzero(alive & (cur < 0))[0]
        # a leaf (or nothing): the kernel tests it, then pops
        if leaf.size:
            empty = sp[leaf] == 0
            alive[leaf[empty]] = False
            go = leaf[~empty]
            sp[go] -= 1
            cur[go] = stack[go, sp[go]]
        if inner.size:
            i = cur[inner]
            lo, hi = lo_all[i], hi_all[i]                       # (m, 3, 4)
            iv, no = inv[inner][:, :, None], noi[inner][:, :, None]
            t0, t1 = _fma(lo, iv, no), _fma(hi, iv, no)
            near, far = np.fmin(t0, t1), np.fmax(t0, t1)
            tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], tmin))
            tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), np.fmin(far[:, 2], tmax))
            c = ch_all[i].copy()
            with np.errstate(invalid="ignore"):
                miss = ~(tn <= tf) | (c == NO_CHILD)
            tn = np.where(miss, BIG, tn); c[miss] = NO_CHILD
            for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                sw = tn[:, b] < tn[:, a]
                ta, tb = np.where(sw, tn[:, b], tn[:, a]), np.where(sw, tn[:, a], tn[:, b])
                ca, cb = np.where(sw, c[:, b], c[:, a]), np.where(sw, c[:, a], c[:, b])
                tn[:, a], tn[:, b], c[:, a], c[:, b] = ta, tb, ca, cb
            for q in (3, 2, 1):
                push = c[:, q] != NO_CHILD
                r = inner[push]
                assert (sp[r] < cap).all(), "replay_closest: raise cap"
                stack[r, sp[r]] = c[push, q]
                sp[r] += 1
            top[inner] = np.maximum(top[inner], sp[inner])
            have = c[:, 0] != NO_CHILD
            cur[inner[have]] = c[have, 0]
            rest = inner[~have]
            empty = sp[rest] == 0
            alive[rest[empty]] = False
            go = rest[~empty]
            sp[go] -= 1
            cur[go] = stack[go, sp[go]]
    return int(top[0]) if one else top


def replay_packet(nodes, o, dirs, tmin=0.0, tmax=3.0e38, active=None):
    """The binary packet walk of one wave (closest_wave, occluded_wave) without its leaves: a node's two children are tested for
    every lane in centre / half-size form; when lanes want both children the one more lanes enter first goes first (ties: child 0) and
    the other is pushed.  o: (3,) shared or (lanes, 3); dirs: (lanes, 3); active: lanes that take part.  Returns the largest sp."""
    dirs = np.atleast_2d(np.asarray(dirs, np.float32))
    o = np.broadcast_to(np.asarray(o, np.float32), dirs.shape)
    active = np.ones(len(dirs), bool) if active is None else np.asarray(active, bool)
    if not active.any():
        return 0
    inv = _rcp(dirs); av = np.abs(inv)
    with np.errstate(invalid="ignore", over="ignore"):
        no = (-(o * inv)).astype(np.float32)
    tmin = np.float32(tmin)
    bt = np.where(active, np.float32(tmax), np.float32(-1.0)).astype(np.float32)
    stack, top, cur = [], 0, 0
    visits = 0
    while True:
        while cur >= 0:
            visits += 1
            assert visits <= 4 * len(nodes) + 4, "replay_packet: the node array is not a tree"
            nd = nodes[cur]
            ax = _fma(nd["ctr"][None, :, :], inv[:, :, None], no[:, :, None])           # (lanes, 3, 2)
            en = _fma(nd["hal"][None, :, :], -av[:, :, None], ax)
            ex = _fma(nd["hal"][None, :, :], av[:, :, None], ax)
            tn = np.fmax(np.fmax(en[:, 0], en[:, 1]), np.fmax(en[:, 2], tmin))          # (lanes, 2)
            tf = np.fmin(np.fmin(ex[:, 0], ex[:, 1]), np.fmin(ex[:, 2], bt[:, None]))
            with np.errstate(invalid="ignore"):
                h = tn <= tf
            h0, h1 = h[:, 0], h[:, 1]
            c0, c1 = int(nd["c0"]), int(nd["c1"])
            if not h0.any() and not h1.any():
                cur = stack.pop() if stack else NO_CHILD
            elif not h0.any():
                cur = c1
            elif not h1.any():
                cur = c0
            else:
                with np.errstate(invalid="ignore"):
                    p0 = int((h0 & (~h1 | (tn[:, 0] <= tn[:, 1]))).sum()); p1 = int((h1 & (~h0 | (tn[:, 1] < tn[:, 0]))).sum())
                first0 = p0 >= p1
                stack.append(c1 if first0 else c0); top = max(top, len(stack))
                cur = c0 if first0 else c1
        if cur == NO_CHILD or not stack:
            return top
        cur = stack.pop()


def tree_levels(nodes):
    """levels of a binary node array, leaves included (what accel_info()["depth"] reports for the host builders)"""
    def lv(i):
        return 1 + max([lv(int(c)) if c >= 0 else 1 for c in (nodes["c0"][i], nodes["c1"][i]) if c != NO_CHILD] or [0])
    return lv(0)


def oracle_tree_levels(verts9):
    """The oracle's private tree (oracle/evplp_oracle.c build_rec: top-down binned SAH over centroids, 12 bins, leaves of at most four
    triangles, equal halves by index where no plane separates) restated in fp32; returns its number of levels.  evo_closest and
    evo_occluded pop one node and push its two children, so their stack[128] holds at most levels + 1 entries."""
    f = np.float32
    v = np.asarray(verts9, f).reshape(-1, 3, 3)
    tlo, thi = v.min(axis=1), v.max(axis=1)
    cen = (f(0.5) * (tlo + thi)).astype(f)
    NB = 12

    def area(lo, hi):
        dx, dy, dz = (hi - lo).astype(f)
        return f(f(f(dx * dy) + f(dy * dz)) + f(dz * dx))

    def rec(ids):
        if len(ids) <= 4:
            return 1
        clo, chi = cen[ids].min(axis=0), cen[ids].max(axis=0)
        best, baxis, bbin = f(3.0e38), -1, -1
        for axis in range(3):
            ext = f(chi[axis] - clo[axis])
            if not ext > 0:
                continue
            scale = f(f(NB) / ext)
            b = np.minimum(((cen[ids, axis] - clo[axis]).astype(f) * scale).astype(f).astype(np.int64), NB - 1)
            for split in range(NB - 1):
                l, r = ids[b <= split], ids[b > split]
                if not len(l) or not len(r):
                    continue
                cost = f(f(area(tlo[l].min(axis=0), thi[l].max(axis=0)) * f(len(l))) + f(area(tlo[r].min(axis=0), thi[r].max(axis=0)) * f(len(r))))
                if cost < best:
                    best, baxis, bbin = cost, axis, split
        if baxis >= 0:
            scale = f(f(NB) / f(chi[baxis] - clo[baxis]))
            b = np.minimum(((cen[ids, baxis] - clo[baxis]).astype(f) * scale).astype(f).astype(np.int64), NB - 1)
            l, r = ids[b <= bbin], ids[b > bbin]
        if baxis < 0 or not len(l) or not len(r):
            l, r = ids[:len(ids) // 2], ids[len(ids) // 2:]
        return 1 + max(rec(l), rec(r))
    return rec(np.arange(len(v)))


def primary_rays(sd, W, H, jitter=(0.0, 0.0)):
    """origin (3,) and directions (H, W, 3) of the frame's jittered primary rays, as the primary pass sets them up (pixel centres through
    the camera basis; fp32, not normalised)"""
    f = np.float32
    eye, at, up = (np.asarray(v, f) for v in (sd.cam_origin, sd.cam_lookat, sd.cam_up))
    fw = at - eye; fw = (fw / np.sqrt((fw * fw).sum(dtype=f))).astype(f)
    s = np.cross(fw, up).astype(f); s = (s / np.sqrt((s * s).sum(dtype=f))).astype(f)
    u = np.cross(s, fw).astype(f)
    th = f(np.tan(f(sd.fovy) / f(2.0)))
    cx = ((np.arange(W, dtype=f) + f(0.5)) / f(W) * f(2.0) - f(1.0) - f(jitter[0])) * f(sd.aspect) * th
    cy = ((np.arange(H, dtype=f) + f(0.5)) / f(H) * f(2.0) - f(1.0) - f(jitter[1])) * th
    d = s[None, None, :] * cx[None, :, None] + u[None, None, :] * cy[:, None, None] + fw[None, None, :]
    return eye, d.astype(f)
