"""evplp_denoise on uploaded hostile planes, at every parameter, against two references; the temporal stage at non-default parameters and
with a non-finite sample; the JSON keys and the group by value.

tests/denoise_hostile.py builds the planes (seven families, three ragged frames, rows past H that are surfaces by their planes and hold
1e30 or NaN), drives the library on them and holds the references: restate(), the fp32 restatement in the kernels' operation order, and
statement64(), include/evplp.h in float64.  tests/test_denoise_hostile_host.py proves the cases and measures the bars without a GPU:
against restate() max(1e-4, 8 x the sensitivity of the case to the last bits of exp / pow / sqrt) -- 1e-4 for every case -- and against
statement64() 4 x the distance between the two references (1.5e-6 to 3.7e-6; denoise_hostile.bars).  Errors are rel_err's: |got - want| /
max(|want|, 1e-6 max |want|) over the filtered pixels.

The non-finite rule (include/evplp.h: a pixel whose u or s is not finite in fp32 is not filtered).  Before it, one tap with u = +Inf had
weight 0 and contributed 0 * Inf = NaN to every pixel whose footprint reached it, at every pass, and the temporal stage blended a
non-finite history value for ever.  test_nonfinite_pixels_stay_alone and test_temporal_nonfinite_sample_leaves_no_trace fail on a
library without the rule (measured on the parent commit: 111 of the 771 pixels of nonfinite-37x21 with a finite composite and variance
come out non-finite, and the +Inf pixel enters the history with length 1).

Measured on one MI355X at the defaults: against restate() 0 (holes-5x3) to 1.12e-6 (smooth-259x13); against statement64() 2.9e-7 to
9.5e-7 under bars of 1.5e-6 to 3.7e-6.  Mutations of the library, each built once and run against this file once:
  `y < st.H` dropped from denoise_prepare_kernel    every case of test_every_family_and_frame_at_the_defaults, the parameter and scale tests
  the light test reading .x only                    the three holes cases, test_scale_light_scale_and_mask_emitter
  gp = gs instead of gs / gw                        ten of the eleven default cases (not zero_variance), the parameter and scale tests
  sigma_normal's override assigned to sigma_l       test_parameters_reach_the_kernel_by_value, test_json_denoise_keys_by_value

5 x 3 (smaller than one 5 x 5 footprint) is accepted by evplp_create, with 8 plane rows: no larger stand-in is needed."""
import json

import numpy as np
import pytest

import denoise_hostile as dh
import temporal_restate as tr

pytestmark = pytest.mark.gpu

f32 = np.float32
RESTATE_NAMES = dict(levels="levels", sigma_luminance="sigma_l", sigma_normal="sigma_n", sigma_position="sigma_x")
ALL_FOUR = dict(levels=2, sigma_luminance=8.0, sigma_normal=16.0, sigma_position=0.05)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def references(case, r, kw=None, f64=False):
    """(restate's image, its filtered pixels, statement64's image or None) on what the library handed out for call r"""
    kw = kw or {}
    args = (r["rgb"], r["var"]) + tuple(r["planes"][:4]) + (r["planes"][4], r["radius"], case.H)
    want, filt = dh.restate(*args, **{RESTATE_NAMES[k]: v for k, v in kw.items()})
    want64 = dh.statement64(*args, **kw)[0] if f64 else None
    return want, filt, want64


def check_call(case, r, kw=None, bar=1e-4):
    """what every call must meet: restate() on the filtered pixels, the composite bit for bit elsewhere, two identical calls"""
    H = case.H
    want, filt, _ = references(case, r, kw)
    got = r["den"]
    m = filt[:H]
    err = dh.rel_err(got[:H][m], want[:H][m])
    print(f"\n{case.family}-{case.W}x{H} {kw or ''}: against restate {err:.3g} (bar {bar:.3g}), {int(m.sum())} filtered pixels")
    assert np.isfinite(got[:H][m]).all()
    assert err < bar, err
    assert same(got[~filt], r["rgb"][~filt])                                  # unfiltered, emitter and every row past H: the composite's bits
    assert same(got, r["den2"])
    return want, filt


@pytest.fixture(scope="module")
def smooth(evplp):
    """smooth at 37 x 21 under every parameter set, one at a time and all four together, on one context"""
    sets = [{}] + [dict(levels=v) for v in (1, 2, 7, 10)] + [dict(sigma_luminance=v) for v in (0.5, 64.0)] + \
           [dict(sigma_normal=v) for v in (0.5, 1.0, 1024.0)] + [dict(sigma_position=v) for v in (1e-4, 10.0)] + [ALL_FOUR]
    case = dh.make_case("smooth", 37, 21)
    return case, sets, dh.drive(evplp, case, [(None, 1.0, False, kw) for kw in sets])


@pytest.mark.parametrize("case_key", dh.CASES, ids=dh.case_id)
def test_every_family_and_frame_at_the_defaults(evplp, case_key):
    family, W, H = case_key
    case = dh.make_case(*case_key)
    r = dh.drive(evplp, case)[0]
    for given, got in zip(dh.guides(case) + (case.light,), r["planes"]):
        assert np.array_equal(given, got, equal_nan=True)
    sens, to64 = dh.bars(case_key)
    want, filt = check_call(case, r, bar=max(1e-4, 8 * sens))
    share = filt[:H].mean()
    assert (0.2 < share < 0.95) if family == "holes" else share > 0.9
    assert not filt[H:].any() and (case.pos[H:, :, 3] == 1).all()
    if family in dh.F64_FAMILIES:
        want64 = references(case, r, f64=True)[2]
        m = filt[:H]
        err64 = dh.rel_err(r["den"][:H][m], want64[:H][m])
        print(f"against statement64 {err64:.3g} (bar {4 * to64:.3g})")
        assert err64 < 4 * to64, (err64, to64)
    # nothing from the rows past H reaches an image row: the same image rows with those rows made harmless give the same bytes
    if family in ("smooth", "holes"):
        tame = dh.make_case(*case_key)
        for p in dh.guides(tame) + (tame.photon,) + tuple(tame.sums):
            p[H:] = 0.0
        assert same(dh.drive(evplp, tame)[0]["den"][:H], r["den"][:H])
    if family != "nonfinite":
        assert np.isfinite(r["den"][:H]).all()
        assert not same(r["den"][:H][filt[:H]], r["rgb"][:H][filt[:H]]), "the filter did nothing"
    if family == "holes":
        y, x = case.marks["isolated"]
        assert filt[y, x] and filt[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() == 1                # (alone in its 3 x 3: g_p is its own s)
        assert all(filt[p] for p in case.marks["corners"])
    if family == "zero_variance":
        # beyond the mirror: neither colour moves toward the other
        assert r["var"][:H].max() == 0
        assert (np.abs(r["den"][:H].astype(np.float64) - r["rgb"][:H]) <= 1e-6 * r["rgb"][:H]).all()
    if family == "normals":
        zero = case.marks["zero_normal"]
        assert np.abs(r["den"][:H][zero] - r["rgb"][:H][zero]).max() <= 2.0 ** -22 * r["rgb"][:H][zero].max()


def test_parameters_reach_the_kernel_by_value(smooth):
    case, sets, runs = smooth
    for kw, r in zip(sets, runs):
        check_call(case, r, kw)
    # levels 1, levels 2, the default and each non-default sigma: pairwise different bytes
    distinct = [i for i, kw in enumerate(sets) if kw in ({}, dict(levels=1), dict(levels=2)) or (len(kw) == 1 and "levels" not in kw)]
    assert len(distinct) == 10
    images = [runs[i]["den"].tobytes() for i in distinct]
    assert len(set(images)) == len(images)
    assert runs[sets.index(ALL_FOUR)]["den"].tobytes() not in images
    # levels 7 and 10 reach steps of 64 and 512, past the frame: the taps that remain are the centre's
    assert len({runs[sets.index(dict(levels=v))]["den"].tobytes() for v in (1, 2, 7, 10)}) >= 3


def test_scale_light_scale_and_mask_emitter(evplp):
    case = dh.make_case("holes", 37, 21)
    B = case.folds
    calls = [(1.0 / B, 1.0, False, {}), (1.0 / B, 0.5, True, {}), (2.0 / B, 0.0, False, {})]
    runs = dh.drive(evplp, case, calls)
    for (scale, ls, me, _), r in zip(calls, runs):
        want, filt = check_call(case, r)
        # every other pixel is resolve(scale, scale, light_scale, mask_emitter) bit for bit (check_call); and that composite is the one meant
        rgb, var = dh.host_inputs(case, scale, ls, me)
        assert same(r["rgb"][:case.H], rgb[:case.H]) and same(r["var"][:case.H], var[:case.H])
    emit = case.marks["emitters"]
    H = case.H
    assert not same(runs[0]["den"][:H][emit[0]], runs[1]["den"][:H][emit[0]])            # R-lit pixels: masked and at half the light
    assert (runs[1]["den"][:H][emit[0]][:, 1:] == 0).all()                               # ... the sums hidden, G and B of the light are 0
    assert (runs[1]["den"][:H][emit[1]][:, 0] > 0).all()                                 # G-only light: light.x = 0 hides nothing
    assert same(runs[2]["den"][:H][emit[2]], (f32(2.0 / B) * case.sums[-1][:H, :, :3][emit[2]]))     # light_scale 0: the sums alone
    assert np.allclose(runs[2]["den"][:H][filt[:H]], 2.0 * runs[0]["den"][:H][filt[:H]], rtol=1e-5)   # the filter is scale-covariant


def test_nonfinite_pixels_stay_alone(evplp):
    case = dh.make_case("nonfinite", 37, 21)
    H = case.H
    r = dh.drive(evplp, case)[0]
    bad = np.zeros((case.rows, case.W), bool)
    for y, x in case.marks["bad"]:
        bad[y, x] = True
    own_finite = np.isfinite(r["rgb"]).all(-1) & np.isfinite(r["var"]).all(-1)
    own_finite[H:] = False
    for kind in ("inf", "nan", "variance"):
        assert not any(own_finite[p] for p in case.marks["kinds"][kind]), kind
    assert all(own_finite[p] for p in case.marks["kinds"]["overflow"])
    poisoned = int((~np.isfinite(r["den"]).all(-1) & own_finite).sum())
    print(f"\n{poisoned} of {int(own_finite.sum())} pixels with a finite composite and variance have a non-finite output")
    assert poisoned == 0
    assert same(r["den"][bad], r["rgb"][bad])                                    # each of them is the composite, bit for bit
    masked = dh.drive(evplp, dh.make_case("nonfinite", 37, 21, masked=True))[0]
    assert same(masked["den"][:H][~bad[:H]], r["den"][:H][~bad[:H]])             # and was never a tap


# ---- the temporal stage (tests/test_gpu_temporal.py's box room and helpers)
def _temporal():
    import test_gpu_temporal as tt
    return tt


def ridged_box(lift=0.15):
    """test_gpu_temporal's box room with the centre vertex of every face of the moving box pushed outwards by 0.15 of the face's shorter
    edge.  Every surface of the box room is axis-aligned, so N_prev . n_q is 0 or 1 there and no value of normal_cos in (0, 1) can be told
    from another (measured on test_gpu_temporal's own sequence: 5775 pixels reprojected at 0.5 and at 0.999 alike).  A face is now four
    facets that meet at ridges with cosines of 0.74 to 0.95.  A pixel next to a ridge still finds a tap on its own facet, so the COUNT of
    reprojected pixels moves only where a facet comes into view that was hidden one frame ago and lies within sigma_position R of its
    neighbour's plane: the sequence therefore turns the box by 1.3 rad where test_gpu_temporal turns it by 0.15 (measured: 5762 reprojected
    at 0.5, 5753 at 0.999; at 0.15 rad the ridged box still gives 5775 twice)."""
    tt = _temporal()
    box = tt.make_box()
    for i in tt.BOX_MESHES:
        v = box.meshes[i]["verts"]
        assert v.shape == (9, 3)                                   # a 2 x 2 quad grid: vertex 4 is the face's centre
        e1, e2 = v[2] - v[0], v[6] - v[0]
        n = np.cross(e1, e2)
        v[4] += f32(lift * min(np.linalg.norm(e1), np.linalg.norm(e2))) * (n / np.linalg.norm(n)).astype(f32)
    box.triangle_soup()
    return box


@pytest.fixture(scope="module")
def moved_box(evplp):
    """test_gpu_temporal's moved-box sequence (on ridged_box) at two parameter sets: frame 0, the box moved, frame 1, frame 2 (nothing moves:
    the frame at which max_history = 2 differs from the default); per frame the library's stage and the restatement's"""
    tt = _temporal()
    box = ridged_box()
    cam = tt.camera_of(box)
    s = 1.0 / tt.ITERS
    m = tt.box_matrix(box, 1.3, (-0.9, 0.7, 0.0))                  # (1.3 rad: see ridged_box)
    out = {}
    for name, kw in (("loose", dict(normal_cos=0.5, max_history=2)), ("tight", dict(normal_cos=0.999))):
        frames = []
        with evplp.Context(tt.W, tt.H, 1, 1, 1) as c:
            box.upload(c); c.noise_track(True); c.temporal_enable(True)
            pose = tt.Pose(box)
            tt.render(evplp, c, box.cam_origin, 0)
            c.denoise_temporal(s, **kw)
            hist = tt.planes(evplp, c)
            for f in (1, 2):
                prev_soup = pose.soup()
                if f == 1:
                    pose.move(evplp, c, m)
                tt.render(evplp, c, box.cam_origin, f)
                inp = tt.inputs(evplp, c, s)
                debug = c.temporal_download(evplp.TEMPORAL_DEBUG_HIT)
                got, info = c.denoise_temporal(s, **kw)
                wp, wn = tr.prev_pose(debug, prev_soup.reshape(-1, 3, 3))
                want_out, want_hist, want_info, filt, a = tt.expect(inp, (wp, wn), hist, cam, cam, **kw)
                frames.append(dict(got=got, info=info, planes=tt.planes(evplp, c), want_out=want_out, want_hist=want_hist, want_info=want_info, filt=filt))
                hist = frames[-1]["planes"]
        out[name] = frames
    return out


@pytest.mark.parametrize("name", ["loose", "tight"])
def test_temporal_parameters_by_value(moved_box, name):
    tt = _temporal()
    for f, fr in enumerate(moved_box[name], 1):
        hu, hp, hn = fr["planes"]
        want_out, want_hist, want_info, info = fr["want_out"], fr["want_hist"], fr["want_info"], fr["info"]
        assert same(hp, want_hist[1]) and same(hn, want_hist[2]) and same(hu, want_out), (name, f)
        assert (info["filtered"], info["reprojected"], info["disoccluded"], info["history_sum"]) == \
            (want_info["filtered"], want_info["n_reprojected"], want_info["disoccluded"], want_info["history_sum"]), (name, f)
        assert want_info["n_reprojected"] > 1000
    lengths = moved_box[name][1]["planes"][2][..., 3][moved_box[name][1]["filt"]]
    assert lengths.max() == (2 if name == "loose" else 3) and (lengths == lengths.max()).mean() > 0.5        # max_history = 2 holds frame 2 at 2


def test_temporal_normal_cos_changes_the_reprojected_count(moved_box):
    loose, tight = (moved_box[k][0]["info"]["reprojected"] for k in ("loose", "tight"))
    print(f"\nreprojected in frame 1: normal_cos 0.5 -> {loose}, 0.999 -> {tight}")
    assert loose > tight


def test_temporal_nonfinite_sample_leaves_no_trace(evplp):
    tt = _temporal()
    box = tt.make_box()
    s = 1.0 / tt.ITERS
    with evplp.Context(tt.W, tt.H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        tt.render(evplp, c, box.cam_origin, 0)
        pos, light = c.download(evplp.BUF_GBUF_POSITION), c.download(evplp.BUF_LIGHT)
        y, x = tt.H // 2, tt.W // 2
        while not (pos[y, x, 3] != 0 and not light[y, x, :3].any()):
            x += 1
        acc = c.download(evplp.BUF_VPL_ACCUM)
        photon = c.download(evplp.BUF_PHOTON_ACCUM)
        assert np.isfinite(acc[:tt.H]).all() and np.isfinite(photon[:tt.H]).all()
        acc[y, x, 0] = np.inf
        c.upload(evplp.BUF_VPL_ACCUM, acc)
        out, info = c.denoise_temporal(s)
        hu, hp, hn = tt.planes(evplp, c)
        assert np.isposinf(out[y, x, 0])                                            # the composite, as it is
        assert hp[y, x, 3] == 0 and hn[y, x, 3] == 0, "the non-finite pixel entered the history"
        others = np.ones(hp.shape[:2], bool); others[y, x] = False; others[tt.H:] = False
        assert np.isfinite(out[others]).all() and np.isfinite(hu[others]).all()
        near = hp[y - 2:y + 3, x - 2:x + 3, 3] != 0
        assert near.sum() >= 12                                                     # (it had filtered neighbours to poison)
        for f in (1, 2):
            tt.render(evplp, c, box.cam_origin, f)
            out, info = c.denoise_temporal(s)
            hu, hp, hn = tt.planes(evplp, c)
            assert np.isfinite(out[:tt.H]).all() and np.isfinite(hu[:tt.H]).all(), f
            assert hp[y, x, 3] == 1 and hn[y, x, 3] == f, f                         # starts again at 1 in the first clean frame
            assert hn[y, x + 1, 3] == f + 1 or hp[y, x + 1, 3] == 0


# ---- the JSON keys and the group, by value
def test_json_denoise_keys_by_value(evplp, tmp_path):
    """a "denoise" block with every key non-default writes the image Context.denoise gives with those arguments on the same run (compared
    as test_gpu_temporal.test_json_temporal_and_rng_advance compares its API sequence)"""
    import scenes
    from test_gpu_transform import H as TH, W as TW, PT, _scene_dir
    d = _scene_dir(evplp, tmp_path, "keys", "pt")
    block = {"filename": "d.pfm", "levels": 2, "sigmaLuminance": 8, "sigmaNormal": 16, "sigmaPosition": 0.05}
    evplp.render_json(str(d / "room.json"), json.dumps({"noise": {"filename": "n.json", "batchIterations": 1}, "denoise": block}))
    written = evplp.load_pfm(str(d / "d.pfm"))
    sd, _ = scenes.load_obj_scene(str(d / "room.json"))
    rng, iters = PT["rngOffset"], PT["numMaxIteration"]
    with evplp.Context(TW, TH, 1, 1, 1) as c:
        c.load_scene_json(str(d / "room.json")); c.noise_track(True)
        c.clear_accumulators()
        jit = evplp.jitter_sequence(rng, iters, TW, TH)
        for i in range(iters):
            c.primary(tuple(jit[i])); c.path_trace(sd.cam_origin, rng + i, PT["numMaxBounces"], accumulate=True); c.noise_fold(1)
        img = c.denoise(1.0 / iters, **ALL_FOUR)
        plain = c.denoise(1.0 / iters)
        one_off = [c.denoise(1.0 / iters, **{**ALL_FOUR, k: 0}) for k in ALL_FOUR]          # each key back at its default
    assert np.array_equal(np.flipud(img[:TH]), written)
    assert not np.array_equal(img, plain) and all(not np.array_equal(img, o) for o in one_off)


@pytest.mark.parametrize("n", [2, 3])
def test_group_strips_with_parameters(evplp, n):
    """evplp_group_denoise on n row strips with every parameter non-default: the single context's bytes (box room, pt, 90 x 50)"""
    tt = _temporal()
    w, h, iters = 90, 50, 3
    box = tt.make_box(w, h)
    jit = evplp.jitter_sequence(0, iters, w, h)

    def run(runner):
        runner.clear_accumulators(); runner.noise_track(True)
        for i in range(iters):
            runner.primary(tuple(jit[i])); runner.path_trace(box.cam_origin, i, 3, accumulate=True); runner.noise_fold(1)
        return runner.denoise(1.0 / iters, **ALL_FOUR)[:h], runner.denoise(1.0 / iters)[:h]

    with evplp.Context(w, h, 1, 1, 1) as c:
        box.upload(c)
        one, one_default = run(c)
    assert not same(one, one_default)
    with evplp.Group(w, h, 1, 1, 1, n, devices=[0] * n, deterministic=True) as g:
        for r in range(n):
            box.upload(g.rank(r))
        got, got_default = run(g)
    assert same(got, one) and same(got_default, one_default)
