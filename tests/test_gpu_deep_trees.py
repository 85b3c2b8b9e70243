"""Deep trees against the per-lane walk stacks, their spill, the packet walks' 64 entries and the refit's level plan.

scenes.morton_chain (A) and scenes.morton_chain_full (B) make the LBVH builders produce chains: B's host LBVH has about 60 levels, a
four-wide stack of about 90 entries that a ray along +z fills to within a few entries, 70 entries beyond the 20 that light tracing keeps
in LDS.  Every test that launches a walk first downloads the tree, restates the stack bound independently (walk_replay.py), replays the
rays it is about to trace and asserts that they fit: a bound that is too small fails here, on the host, before any kernel runs.
"B20" is scene B with 20 triangles per cluster instead of 5: the SAH tree of B itself never holds more than 21 entries for these rays, the
SAH tree of B20 reaches the spill as well."""
import copy

import numpy as np
import pytest

import oracle_api as oa
import scenes
import walk_replay as wr
from test_gpu_parity import assert_image_close, rel_l2

pytestmark = pytest.mark.gpu

W, H = 64, 48
N, P = 200, 4
SEED = 7
JITTER = (0.003, -0.002)
BUILDERS = {0: "lbvh", 1: "sah", 2: "sbvh", 3: "gpu", 4: "ploc"}
MAX_LEVELS = 62                         # evplp_build_accel refuses deeper trees (kMaxDepth - 2): the packet walks keep 64 entries
SPILL = wr.LT_LDS_ENTRIES + 4           # a ray that reaches this sp has written and read back at least four entries of its global column
F = np.float32


def say(*a):
    print("[deep trees]", *a, flush=True)


class Deep:
    """one scene with the oracle's results, computed once"""

    def __init__(self, sd):
        self.sd = sd
        self.osc = oa.Scene(sd)
        self.records = self.osc.trace_light_paths(SEED, N, P)
        self._gbuf = None

    @property
    def gbuf(self):
        if self._gbuf is None:
            self._gbuf = self.osc.primary(W, H, JITTER)
        return self._gbuf


def first_segments(records):
    """origin, direction and validity of every path's first segment, from the oracle's records (record 1 keeps the negated direction)"""
    r = records.reshape(N, P)
    return r["pos"][:, 0].copy(), (-r["flux_dir"][:, 1]).astype(F), r["flags"][:, 1] != 0


@pytest.fixture(scope="module")
def deep(oracle):
    made = {}

    def get(name):
        if name not in made:
            sd = {"A": lambda: scenes.morton_chain(aspect=W / H), "B": lambda: scenes.morton_chain_full(aspect=W / H),
                  "B20": lambda: scenes.morton_chain_full(per=20, aspect=W / H)}[name]()
            made[name] = Deep(sd)
        return made[name]
    return get


def context(evplp, sd, builder, npaths=N):
    c = evplp.Context(W, H, npaths, npaths, P, bvh_builder=builder, deterministic=True)
    sd.upload(c)
    return c


def generic_bound(depth):
    return 3 * ((depth + 1) // 2) + 4


def preflight(c, what):
    """The tree as it is on the device against every bound the walks rely on; returns its figures.  No walk has run when this returns."""
    info = c.accel_info()
    nodes, n4 = c.debug_accel(0), c.debug_accel(4)
    assert np.array_equal(n4["child"], wr.four_wide(nodes)["child"]), f"{what}: the four-wide nodes are not the binary nodes' grandchildren"
    worst = wr.worst_case_entries(n4)
    levels = wr.tree_levels(nodes)
    generic = generic_bound(info["depth"])
    entries = info["stack4_entries"]
    if entries > 0:
        assert entries == worst + 2, f"{what}: stack4_entries {entries}, the tree's worst case is {worst} (+ 2)"
    allocated = min(entries, generic) if entries > 0 else generic               # kernels.h lane_stack_bytes4 / lt_overflow_entries
    assert worst <= allocated, f"{what}: a ray can hold {worst} entries, the walks get {allocated} (stack4_entries {entries}, generic {generic})"
    assert levels <= info["depth"] <= MAX_LEVELS, f"{what}: {levels} levels, reported depth {info['depth']}"
    return dict(info=info, nodes=nodes, n4=n4, worst=worst, levels=levels, generic=generic, allocated=allocated)


# ---- a. the bound
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["A", "B"])
def test_stack_bound_of_the_tree_that_was_built(evplp, deep, name, builder):
    with context(evplp, deep(name).sd, builder) as c:
        f = preflight(c, f"{name} {BUILDERS[builder]}")
    info = f["info"]
    # what the frame's own rays would hold on this tree: the per-lane walk for every primary ray, the packet walk for every 8 x 8 tile
    eye, dirs = wr.primary_rays(deep(name).sd, W, H, JITTER)
    sp = wr.replay_closest(f["n4"], np.broadcast_to(eye, (W * H, 3)), dirs.reshape(-1, 3), 0.1, 100.0)
    packet = max(wr.replay_packet(f["nodes"], eye, dirs[y:y + 8, x:x + 8].reshape(-1, 3), 0.1, 100.0) for y in range(0, H, 8) for x in range(0, W, 8))
    say(f"a. scene {name} builder {BUILDERS[builder]} -> ran {info['builder']}: nodes {info['nodes']} depth {info['depth']} levels {f['levels']} "
        f"stack4_entries {info['stack4_entries']} worst case {f['worst']} generic {f['generic']} | primary rays: per-lane sp {sp.min()} .. {sp.max()}, packet sp {packet}")
    assert sp.max() <= f["worst"] and packet <= f["levels"] - 1 <= MAX_LEVELS
    if builder <= 2:
        assert info["builder"] == BUILDERS[builder], "a host builder fell back"
        assert info["stack4_entries"] == f["worst"] + 2, "the host builders store their nodes in pre-order: the tree's own bound applies"
    else:
        assert info["builder"] in (BUILDERS[builder], "sah"), info          # (a device tree deeper than 62 levels is rebuilt by SAH on the host)
    if builder == 0 and name == "B":
        assert 59 <= info["depth"] <= 62 and info["stack4_entries"] >= 60
    if builder == 0 and name == "A":
        assert info["stack4_entries"] >= 30


# ---- b. light tracing through the spill
def spill_preflight(c, d, what):
    f = preflight(c, what)
    o, dirs, ok = first_segments(d.records)
    sp = np.zeros(N, np.int64)
    sp[ok] = wr.replay_closest(f["n4"], o[ok], dirs[ok], 1e-4)
    assert sp.max() <= f["worst"] <= f["allocated"], f"{what}: a replayed first segment holds {sp.max()} entries"
    f["sp"] = sp
    say(f"b. {what} (ran {f['info']['builder']}): depth {f['info']['depth']} stack4_entries {f['info']['stack4_entries']} first segments: largest sp {sp.max()}, "
        f"{int((sp >= SPILL).sum())} of {N} paths reach sp >= {SPILL}")
    return f


@pytest.mark.parametrize("name, builder", [(n, b) for n in ("A", "B") for b in BUILDERS] + [("B20", 0), ("B20", 1)])
def test_light_tracing_through_the_spill(evplp, deep, name, builder):
    d = deep(name)
    ref = d.records
    assert (ref["flags"].reshape(N, P)[:, 1] != 0).sum() > N // 2 and (ref["flags"].reshape(N, P)[:, 2] != 0).sum() > N // 4
    with context(evplp, d.sd, builder) as c:
        f = spill_preflight(c, d, f"scene {name} builder {BUILDERS[builder]}")
        if builder == 0 and name in ("A", "B"):
            assert f["info"]["builder"] == "lbvh" and (f["sp"] >= SPILL).sum() * 2 >= N, "the chain no longer drives half of the paths into the spill"
        if builder == 1 and name == "B20":
            assert f["info"]["builder"] == "sah" and (f["sp"] >= SPILL).any(), "no path reaches the spill on the SAH tree"
        c.trace_light_paths(SEED)
        got = c.download(evplp.BUF_RECORDS)
        assert np.array_equal(got["flags"], ref["flags"]), "path structure differs (closest hit)"
        assert got.tobytes() == ref.tobytes()
        # sliced: 70 + 130 paths, neither a multiple of 64 -- other strides, other lane offsets, the same columns
        c.upload(evplp.BUF_RECORDS, np.zeros_like(got))
        c.trace_light_paths(SEED, 0, 70)
        c.trace_light_paths(SEED, 70, 130)
        assert c.download(evplp.BUF_RECORDS).tobytes() == ref.tobytes(), "the sliced trace differs"


def test_the_spill_column_grows_with_the_launch_and_with_the_tree(evplp, deep):
    a, b = deep("A"), deep("B")
    with context(evplp, a.sd, 0) as c:
        spill_preflight(c, a, "scene A lbvh, before scene B")
        c.trace_light_paths(SEED)
        assert c.download(evplp.BUF_RECORDS).tobytes() == a.records.tobytes()
    with context(evplp, b.sd, 0) as c:                          # a fresh context, a deeper tree
        spill_preflight(c, b, "scene B lbvh, after scene A")
        c.trace_light_paths(SEED, 0, 64)                        # one wave's columns ...
        first = c.download(evplp.BUF_RECORDS)
        assert first[:64 * P].tobytes() == b.records[:64 * P].tobytes()
        c.trace_light_paths(SEED)                               # ... then four waves': the area is allocated again
        assert c.download(evplp.BUF_RECORDS).tobytes() == b.records.tobytes()
        c.upload(evplp.BUF_RECORDS, np.zeros_like(first))
        c.trace_light_paths(SEED, 64, N - 64)                   # and a smaller launch inside the larger area, from a path_begin > 0
        c.trace_light_paths(SEED, 0, 64)
        assert c.download(evplp.BUF_RECORDS).tobytes() == b.records.tobytes()


# ---- c. independent of any tree
@pytest.mark.parametrize("name", ["A", "B"])
def test_deep_walk_hits_are_the_brute_force_hits(evplp, deep, oracle, name):
    """Every used record i >= 1 lies where the brute-force closest hit over all triangles (the triangle predicate alone, tmin = 1e-4, ties
    to the lowest index) puts it: o + d t in fp32, from record i - 1 along the negated flux direction of record i."""
    import ctypes as C
    d = deep(name)
    with context(evplp, d.sd, 0) as c:
        spill_preflight(c, d, f"scene {name} lbvh")
        c.trace_light_paths(SEED)
        rec = c.download(evplp.BUF_RECORDS).reshape(N, P)
    verts = d.osc.verts
    t, b, g = (C.c_float() for _ in range(3))
    checked = 0
    for p in range(N):
        for i in range(1, P):
            if rec["flags"][p, i] == 0:
                continue
            o = np.ascontiguousarray(rec["pos"][p, i - 1]); dr = np.ascontiguousarray(-rec["flux_dir"][p, i])
            best, bt = -1, 3e38
            for k in range(verts.shape[0]):
                v = verts[k]
                if oracle.evo_tri_test(oa.ptr(v[0:3]), oa.ptr(v[3:6]), oa.ptr(v[6:9]), oa.ptr(o), oa.ptr(dr), 1e-4, 3e38, C.byref(t), C.byref(b), C.byref(g)):
                    if t.value < bt:
                        best, bt = k, t.value
            assert best >= 0, (p, i)
            want = (o + (dr * F(bt)).astype(F)).astype(F)
            assert rec["pos"][p, i].tobytes() == want.tobytes(), (p, i, best, rec["pos"][p, i], want)
            checked += 1
    assert checked > N


# ---- d. path tracer and light-path windows on the deep tree
def upload_inputs(c, evplp, gbuf, records):
    for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), gbuf):
        pad = np.zeros((c.local_rows, W, 4), np.float32); pad[:H] = plane
        c.upload(b, pad)
    c.upload(evplp.BUF_RECORDS, records)


def other_path_share(g, r):
    return (np.abs(g - r) > 2e-4 * np.maximum(np.abs(r), 1e-3 * r.max())).any(-1)


def test_path_tracer_and_lvc_gather_fill_the_lds_stack(evplp, deep):
    """Scene B: the host LBVH tree (the deep one), the SAH tree and the device LBVH tree give the same bytes, and those agree with the
    oracle under test_gpu_parity's rules (test_path_trace, test_gather_lvc_window).  Should the share of pixels that took another path
    pass that test's 8e-3 on this scene, the share measured on the SAH tree (the shallow one) plus one pixel in a thousand bounds the deep
    tree's.  Measured on an MI355X: no pixel of 3 072 took another path on any of the three trees (share 0.0), primary rays hold 85 .. 86
    of the 89 entries of the host LBVH tree."""
    d = deep("B")
    gbuf, cam = d.gbuf, d.sd.cam_origin
    lvc = dict(camera_pos=cam, mis_mode=1, pdf_mc=0.35, photon_radius=0.05, num_light_paths=N, num_vpl_light_paths=N // 4, photons_per_path=P,
               do_accumulate=0, rng_seed=9)
    eye, dirs = wr.primary_rays(d.sd, W, H, JITTER)
    out = {}
    for builder in (0, 1, 3):
        with context(evplp, d.sd, builder) as c:
            f = preflight(c, f"scene B {BUILDERS[builder]}")
            sp = wr.replay_closest(f["n4"], np.broadcast_to(eye, (W * H, 3)), dirs.reshape(-1, 3), 0.1, 100.0)
            say(f"d. scene B builder {BUILDERS[builder]} (ran {f['info']['builder']}): depth {f['info']['depth']} stack4_entries {f['info']['stack4_entries']} "
                f"LDS entries {f['allocated']} primary rays: sp {sp.min()} .. {sp.max()}")
            assert sp.max() <= f["worst"] <= f["allocated"]
            if builder == 0:
                e = f["info"]["stack4_entries"]
                assert f["info"]["builder"] == "lbvh" and f["allocated"] == e
                assert e - 4 <= sp.max() <= e - 2, f"primary rays reach {sp.max()} of {e} entries: the stack is not filled"
            upload_inputs(c, evplp, gbuf, d.records)
            c.clear_accumulators()
            for seed in (3, 4):
                c.path_trace(cam, seed, 3, accumulate=True)
            pt = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
            st = c.pass_stats(evplp.PASS_PATH_TRACE)
            c.clear_accumulators()
            c.gather_lvc(evplp.frame_params(**lvc))
            out[builder] = (pt, c.download(evplp.BUF_VPL_ACCUM)[:H].copy(), st, c.pass_stats(evplp.PASS_GATHER_LVC)["pairs"])
    for builder in (0, 3):
        assert out[builder][0].tobytes() == out[1][0].tobytes(), f"path_trace: the {BUILDERS[builder]} tree differs from the SAH tree"
        assert out[builder][1].tobytes() == out[1][1].tobytes(), f"gather_lvc: the {BUILDERS[builder]} tree differs from the SAH tree"
    ref, _ = d.osc.path_trace(cam, 3, 3, W, H, gbuf)
    ref, n2 = d.osc.path_trace(cam, 4, 3, W, H, gbuf, out=ref)
    assert ref[..., :3].max() > 0
    r = ref[..., :3]
    share = {b: float(other_path_share(out[b][0][..., :3], r).mean()) for b in out}
    say(f"d. path tracer: share of pixels that took another path: sah {share[1]:.5f} lbvh {share[0]:.5f} device lbvh {share[3]:.5f}")
    limit = 8e-3 if share[1] <= 8e-3 else share[1] + 1e-3
    for b in out:
        g = out[b][0][..., :3]
        st = out[b][2]
        assert st["pairs"] == n2 == int((gbuf[0][..., 3] != 0).sum()) and st["rays"] >= n2
        if b != 1:
            assert share[b] <= limit, f"{BUILDERS[b]}: {share[b]:.5f} of the pixels took another path (SAH tree: {share[1]:.5f})"
        ok = ~other_path_share(g, r)
        assert rel_l2(g[ok], r[ok]) <= 1e-5
        assert abs(float(g.sum()) / float(r.sum()) - 1.0) <= 5e-3
    want, pairs = d.osc.gather(oa.frame_params(**lvc), W, H, gbuf, d.records, lvc=True)
    assert want[..., :3].max() > 0
    for b in out:
        assert out[b][3] == pairs > 0
        assert_image_close(out[b][1][..., :3], want[..., :3], what=f"gather_lvc on the {BUILDERS[b]} tree")


# ---- e. packet walks one or two levels under their limit
def test_packet_walks_on_the_deepest_tree(evplp, deep, monkeypatch):
    d = deep("B")
    kw = dict(camera_pos=d.sd.cam_origin, mis_mode=0, num_light_paths=N, num_vpl_light_paths=N, photons_per_path=P)
    eye, dirs = wr.primary_rays(d.sd, W, H, JITTER)
    want, pairs = d.osc.gather(oa.frame_params(**kw), W, H, d.gbuf, d.records)
    images = {}
    for cuts in ("1", "0"):
        monkeypatch.delenv("EVPLP_CUTS", raising=False)
        if cuts == "0":
            monkeypatch.setenv("EVPLP_CUTS", "0")
        with context(evplp, d.sd, 0) as c:
            f = preflight(c, "scene B lbvh")
            assert f["info"]["builder"] == "lbvh" and 59 <= f["info"]["depth"] <= MAX_LEVELS
            # a packet pushes at most one entry per level of inner nodes, whatever its rays: the shadow packets of the gather too
            assert f["levels"] - 1 <= MAX_LEVELS
            top = max(wr.replay_packet(f["nodes"], eye, dirs[y:y + 8, x:x + 8].reshape(-1, 3), 0.1, 100.0) for y in range(0, H, 8) for x in range(0, W, 8))
            assert top <= f["levels"] - 1 <= MAX_LEVELS
            if cuts == "1":
                say(f"e. scene B lbvh: depth {f['info']['depth']} packet walks of the primary tiles: largest sp {top}")
                assert top >= f["levels"] - 4, "the primary packets no longer walk the whole chain"
            c.primary(JITTER, clear_light=True)
            got = [c.download(b)[:H] for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG, evplp.BUF_LIGHT)]
            for k, (a, b) in enumerate(zip(got, d.gbuf)):
                assert a.tobytes() == b.tobytes(), f"EVPLP_CUTS={cuts}: primary plane {k} differs from the oracle's"
            c.upload(evplp.BUF_RECORDS, d.records)
            c.clear_accumulators()
            c.gather_vpl(evplp.frame_params(**kw))
            images[cuts] = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
            assert c.pass_stats(evplp.PASS_GATHER_VPL)["pairs"] == pairs > 0
    assert (d.gbuf[1][..., 2] < 0).mean() > 0.8 and (d.gbuf[4][..., 0] > 0).any(), "sheets nearly everywhere, the light in view"
    img = images["1"]
    assert np.array_equal((img[..., :3] > 0).any(axis=-1), (want[..., :3] > 0).any(axis=-1)), "lit pixels differ: a shadow packet went wrong"
    assert (want[..., :3] > 0).any()
    assert np.abs(img[..., :3].astype(np.float64) - want[..., :3]).max() <= 2e-4 * np.abs(want[..., :3]).max()
    assert images["0"].tobytes() == img.tobytes(), "the gather from the root differs from the gather from the entry cuts"


# ---- f. refit at the level plan's limit
def test_refit_of_the_deepest_tree(evplp, deep):
    d = deep("B")
    moved = copy.deepcopy(d.sd)
    m = moved.meshes[moved.sheet_mesh]
    m["verts"] = (m["verts"] + np.array([0.03, -0.02, 0.05], F)).astype(F)
    moved.triangle_soup()
    with context(evplp, moved, 1) as c:                          # the moved scene, built afresh (SAH: any tree gives these bytes)
        preflight(c, "moved scene B sah")
        c.primary(JITTER, clear_light=True)
        c.trace_light_paths(SEED)
        want = [c.download(b)[:H].copy() for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_LIGHT)]
        want_records = c.download(evplp.BUF_RECORDS).copy()
    assert want_records.tobytes() == oa.Scene(moved).trace_light_paths(SEED, N, P).tobytes()
    assert want_records.tobytes() != d.records.tobytes(), "the motion is not visible"
    with context(evplp, d.sd, 0) as c:
        before = preflight(c, "scene B lbvh")
        assert before["info"]["builder"] == "lbvh" and 59 <= before["info"]["depth"] <= MAX_LEVELS
        c.update_mesh(d.sd.sheet_mesh, m["verts"])
        c.refit_accel()
        after = preflight(c, "scene B lbvh, refitted")
        assert np.array_equal(after["n4"]["child"], before["n4"]["child"]) and after["worst"] == before["worst"]
        info = c.refit_info()
        say(f"f. scene B lbvh: depth {before['info']['depth']}, refit levels {info['levels']}")
        assert info["refits"] == 1 and info["levels"] == after["levels"] - 1, (info, after["levels"])
        o, dirs, ok = first_segments(want_records)
        sp = wr.replay_closest(after["n4"], o[ok], dirs[ok], 1e-4)
        assert sp.max() <= after["worst"] <= after["allocated"] and (sp >= SPILL).sum() * 2 >= N
        c.primary(JITTER, clear_light=True)
        c.trace_light_paths(SEED)
        got = [c.download(b)[:H] for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_LIGHT)]
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.tobytes() == b.tobytes(), f"refit: G-buffer plane {k} differs from a fresh build's"
        assert c.download(evplp.BUF_RECORDS).tobytes() == want_records.tobytes(), "refit: light-path records differ from a fresh build's"
