"""The photon splat's binning against a float64 brute force over every (pixel, photon) pair, on the hostile sets of tests/splat_hostile.py.

Per case, in modes 0, 3 and 5, with deterministic and plain contexts: the pair count of pass_stats equals the float64 count exactly;
pixels without an inside photon are exactly 0 (padding rows included); every compared pixel is within
    sum_k (K 2^-24 kappa_k + 2^-22 lam_k) |val_k| + n 2^-24 sum_k |val_k| + n 1e-20,     K = K_GPU_SPLAT
(the bar of test_gather_whole_set); a second pass with clear = False doubles the image; every tile's bin wanted at least as many entries
as photons have an inside pixel in it (evplp_debug_splat_bins), so that a lost entry points at its tile, and exactly the entries that the
float64 restatement of photon_rect and box_within predicts; and the paths the case was built
for were taken (segment overflow, the large-rectangle list, the re-run after a bin overflowed the context's own stride).  dense_bins and
seg_overflow also run with EVPLP_BIN_STRIDE = 2 and with the MIXED tile launch forced (heavy list of 2048 and of 2 tiles): byte for byte
the default's image on deterministic contexts, within the bar otherwise.  buckets_ragged_132x68 also runs as two row strips of 8 rows,
and four frames run under the proxy footprint against the oracle's ray / triangle count over the icosphere.

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_splat_hostile.py` prints them): every pair count exact, every tile's bin
entries equal to the prediction, error / bar at its worst (K = K_GPU_SPLAT = 18) in modes 0 / 3 / 5, the same to three digits on
deterministic and plain contexts and under every variant:
    seg_overflow 0.190 / 0.191 / 0.036 (big_count of group 1: 77 - 79)      big_rects 0.182 / 0.170 / 0.146 (big_count 24 + 19 = 43)
    near_plane 0.124 / 0.059 / 0.033                                        off_screen 0.150 / 0.140 / 0.045
    buckets_ragged_132x68 0.167 / 0.194 / 0.058 (the same in two strips)    buckets_ragged_260x36 0.214 / 0.276 / 0.064
    record_edges 0.107 / 0.111 / 0.025                                      dense_bins 0.257 / 0.264 / 0.034 (fullest bin 1100 > 256 slots)
    depth_edges 0.190 / 0.163 / 0.034                                       far_coordinates 0.248 / 0.267 / 0.079
Proxy footprint, fragments (equal to the oracle's): 2686, 3447, 3061 and 1765 for the two buckets_ragged frames, near_plane and off_screen.
Deliberately wrong kernels, each tried once on a scratch build the same day, and the tests of this file that failed:
  * segment overflow without the push to big_list: test_case and test_variants of seg_overflow (29202 pairs for 40105)
  * every large rectangle culled, photon_reach2's guard 0: test_case of big_rects, near_plane and depth_edges -- by the predicted entries
    alone (tile 0 of big_rects: 3 for 9): with correct tile boxes the cull loses no pair, which is why the un-culled class is predicted exactly
  * zlo = vz - r without the clamp to 0.1: test_case of near_plane and depth_edges, again by the entries (17 for 3 in tile 0): the
    rectangles only grow
  * the predecessor of a chunk's first record from slot 0: test_case of record_edges, dense_bins and seg_overflow (and their variants), by the bar
  * tile boxes with W / 8 tile columns: test_case of both buckets_ragged frames and big_rects, test_strips, test_proxy_footprint (pairs lost)
  * base += 64 in the four-wave loop: test_case and test_variants of dense_bins (133248 pairs for 40653)
"""
import numpy as np
import pytest

import oracle_api as oa
import shading_domain as sd
import splat_hostile as sh
from test_gpu_parity import assert_image_close, rel_l2
from test_gpu_shading_domain import K_GPU_SPLAT

pytestmark = pytest.mark.gpu

PLANES = ("BUF_GBUF_POSITION", "BUF_GBUF_NORMAL", "BUF_GBUF_DIFFUSE", "BUF_GBUF_PHONG")
VARIANTS = {
    "default": {},
    "stride2": {"EVPLP_BIN_STRIDE": "2"},
    "mixed2048": {"EVPLP_TILE_HEAVY": "4", "EVPLP_TILE_MIXED_TRIGGER": "0", "EVPLP_TILE_HEAVY_CAP": "2048"},
    "mixed2": {"EVPLP_TILE_HEAVY": "4", "EVPLP_TILE_MIXED_TRIGGER": "0", "EVPLP_TILE_HEAVY_CAP": "2"},
}
ENV = ("EVPLP_BIN_STRIDE", "EVPLP_TILE_HEAVY", "EVPLP_TILE_MIXED_TRIGGER", "EVPLP_TILE_HEAVY_CAP", "EVPLP_TILE_MIXED", "EVPLP_SPLIT_MIN")


@pytest.fixture(scope="module")
def floor():
    return sd.floor_scene()


@pytest.fixture(scope="module", params=sh.NAMES)
def case(request, oracle):
    c = sh.case(request.param)
    for mode in sh.MODES:
        c.reference(mode)
    return c


def make_context(evplp, floor, c, deterministic, **kw):
    """a context with the case's camera, G-buffer and records (the environment is read when the context is created)"""
    ctx = evplp.Context(c.W, c.H, c.nlp, c.nlp, c.P, bvh_builder=evplp.BVH_SAH, deterministic=deterministic, **kw)
    floor.upload(ctx)
    ctx.set_camera(c.cam["origin"], c.cam["lookat"], c.cam["up"], c.cam["fovy"], c.cam["aspect"])
    ctx.primary(c.jitter)                           # (the splat projects photons through the camera of the frame)
    rows = ctx.global_rows()
    for b, plane in zip(PLANES, c.gbuf):
        pad = np.zeros((ctx.local_rows, c.W, 4), np.float32)
        pad[rows < c.H] = plane[rows[rows < c.H]]
        ctx.upload(getattr(evplp, b), pad)
    ctx.upload(evplp.BUF_RECORDS, c.records)
    return ctx, rows


def splat(evplp, ctx, c, mode, clear=True, **kw):
    ctx.splat_photons(evplp.frame_params(**c.params(mode), **kw), clear=clear)
    return ctx.download(evplp.BUF_PHOTON_ACCUM), ctx.pass_stats(evplp.PASS_SPLAT)


def check_image(c, ref, got, rows, what):
    """untouched pixels exactly 0, compared pixels within the bar; returns error / bar at its worst"""
    assert np.isfinite(got).all(), what
    inimg = rows < c.H
    assert np.all(got[~inimg] == 0.0), what + ": a padding row was written"
    g, r = got[inimg], rows[inimg]
    assert np.all(g[..., 3] == 0.0), what
    stray = np.argwhere((g[..., :3] != 0.0).any(-1) & (ref.n[r] == 0))
    assert stray.size == 0, f"{what}: {len(stray)} pixels without an inside photon were written, first (x, y) = ({stray[0][1]}, {r[stray[0][0]]})"
    worst, y, x, ch = c.worst(ref, g[..., :3], K_GPU_SPLAT, rows=r)
    if worst > 1.0:
        ly = int(np.flatnonzero(r == y)[0])
        raise AssertionError(f"{what}: {c.blame(ref, y, x)}; channel {ch}: got {g[ly, x, ch]!r}, float64 {ref.total[y, x, ch]!r}, error / bar {worst:.3g}")
    return worst


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "plain"])
@pytest.mark.parametrize("mode", sh.MODES)
def test_case(evplp, floor, case, monkeypatch, mode, deterministic):
    c = case
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    ref = c.reference(mode)
    what = f"{c.name} mode {mode} {'deterministic' if deterministic else 'plain'}"
    ctx, rows = make_context(evplp, floor, c, deterministic)
    with ctx:
        got, st = splat(evplp, ctx, c, mode)
        big, cursor = ctx.debug_splat_bins()
        twice, st2 = splat(evplp, ctx, c, mode, clear=False)
    assert st["pairs"] == c.pairs == st2["pairs"], (what, st["pairs"], st2["pairs"], c.pairs)
    worst = check_image(c, ref, got, rows, what)
    assert np.allclose(twice[..., :3], 2 * got[..., :3], rtol=1e-6, atol=1e-9), what + ": the second pass does not add"
    # path evidence
    cursor = cursor[:c.tiles_y].reshape(-1)
    short = np.flatnonzero(cursor < c.tile_need)
    assert short.size == 0, (f"{what}: tile {int(short[0])} ({int(short[0]) % c.tiles_x}, {int(short[0]) // c.tiles_x}) has {int(cursor[short[0]])} bin entries, "
                             f"{int(c.tile_need[short[0]])} photons have a pixel in it")
    # ... and exactly the predicted entries (the predictions have their margins; a photon that overflows its segment takes the same tiles)
    wrong = np.flatnonzero(cursor != c.entries_per_tile)
    assert wrong.size == 0, f"{what}: tile {int(wrong[0])} has {int(cursor[wrong[0]])} bin entries, predicted {int(c.entries_per_tile[wrong[0]])}; {wrong.size} tiles differ"
    fullest = st["nodes"] >> 32
    assert fullest == int(cursor.max()), (what, fullest, int(cursor.max()))
    if c.name == "seg_overflow":
        assert all(c.path[i] == "lds" for i in range(256, 512)) and big[1] >= c.seg_overflow_min[1] > 0, (what, big, c.seg_overflow_min)
    if c.name == "big_rects":
        assert int(big.sum()) == c.big_predicted, (what, big, c.big_predicted)
    if c.name == "dense_bins":
        stride = sh.default_stride(c.n, c.tiles_x * c.tiles_y)
        assert int(cursor.max()) >= 1100 > stride, (what, int(cursor.max()), stride)       # (the context began with `stride` slots: the pass ran again)
    print(f"\n{what}: {c.pairs} pairs, worst error / bar {worst:.3f} (K = {K_GPU_SPLAT}); big_count {big.tolist()}, bin entries {int(cursor.sum())} "
          f"(predicted {int(c.entries_per_tile.sum())} + segment overflow), fullest bin {fullest}")


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "plain"])
@pytest.mark.parametrize("mode", sh.MODES)
@pytest.mark.parametrize("name", ["dense_bins", "seg_overflow"])
def test_variants(evplp, floor, oracle, monkeypatch, name, mode, deterministic):
    """the re-run after an overflow and the MIXED tile launch: the same pairs; the same bytes where the accumulation is in record order"""
    c = sh.case(name)
    ref = c.reference(mode)
    images, worst = {}, {}
    for variant, env in VARIANTS.items():
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        what = f"{name} mode {mode} {'deterministic' if deterministic else 'plain'} {variant}"
        ctx, rows = make_context(evplp, floor, c, deterministic)
        with ctx:
            got, st = splat(evplp, ctx, c, mode)
        assert st["pairs"] == c.pairs, (what, st["pairs"], c.pairs)
        worst[variant] = check_image(c, ref, got, rows, what)
        images[variant] = got
    if deterministic:
        for variant in VARIANTS:
            assert images[variant].tobytes() == images["default"].tobytes(), f"{name} mode {mode}: {variant} differs from the default"
    print(f"\n{name} mode {mode} {'deterministic' if deterministic else 'plain'}: worst error / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("mode", sh.MODES)
def test_strips(evplp, floor, oracle, monkeypatch, mode):
    """buckets_ragged_132x68 as two row strips of 8 rows (local_tile_row): the ranks' pairs add up, each rank's rows meet the bar"""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    c = sh.case("buckets_ragged_132x68")
    ref = c.reference(mode)
    pairs, seen, worst = 0, np.zeros(c.H, int), 0.0
    for rank in (0, 1):
        ctx, rows = make_context(evplp, floor, c, True, strip_rank=rank, strip_count=2, strip_rows=8)
        with ctx:
            got, st = splat(evplp, ctx, c, mode)
        pairs += st["pairs"]
        seen[rows[rows < c.H]] += 1
        assert st["pairs"] == int(ref.n[rows[rows < c.H]].sum()), (rank, st["pairs"])
        worst = max(worst, check_image(c, ref, got, rows, f"strips mode {mode} rank {rank}"))
    assert np.all(seen == 1) and pairs == c.pairs, (pairs, c.pairs)
    print(f"\nbuckets_ragged_132x68 in two strips, mode {mode}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("name", ["buckets_ragged_132x68", "buckets_ragged_260x36", "near_plane", "off_screen"])
def test_proxy_footprint(evplp, floor, oracle, monkeypatch, name):
    """EVPLP_FOOTPRINT_PROXY in mode 1 against the oracle's count over the generated icosphere: equal pairs, fragments and images by the rule
    of test_photon_splat_proxy_meshes"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    c = sh.case(name)
    cam = oa.Camera()
    for k in ("origin", "lookat", "up"):
        setattr(cam, k, (oa.C.c_float * 3)(*c.cam[k]))
    cam.fovy, cam.aspect = c.cam["fovy"], c.cam["aspect"]
    ideal, proxy, ost = oa.splat_proxy(oa.frame_params(**c.params(1)), cam, c.W, c.H, c.gbuf, c.records)
    assert int(ost[0]) == c.pairs
    ctx, rows = make_context(evplp, floor, c, True)
    with ctx:
        ctx.set_splat_proxy()
        got, st = splat(evplp, ctx, c, 1, splat_footprint="proxy")
    got = got[:c.H]
    assert st["pairs"] == c.pairs, (name, st["pairs"], c.pairs)
    assert abs(st["rays"] - int(ost[3])) <= max(1, int(ost[3]) // 50000), (name, st["rays"], ost)
    if st["rays"] == int(ost[3]):
        assert_image_close(got[..., :3], proxy[..., :3], what=f"proxy {name}")
    else:
        assert rel_l2(got[..., :3], proxy[..., :3]) <= 1e-3
    print(f"\n{name} proxy footprint: {st['rays']} fragments (oracle {int(ost[3])}), {c.pairs} pairs")
