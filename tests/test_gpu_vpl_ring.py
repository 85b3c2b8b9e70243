"""The VPL gather with entry cuts reads a VPL's record from the LDS ring its cut slot streams through (kernels_gather.hip, EVPLP_VPL_RING):
lanes 16-21 of the slot's DMA instruction bring the 96 bytes along, and the step shades with operands from LDS.  The walks from the root
(EVPLP_CUTS=0) still fetch the record with scalar loads -- the independent statement of the same fetch.  Here the two are compared bit for
bit on crafted inputs: a G-buffer from the oracle whose pixels carry three material classes, and records whose flux is a distinct function
of the record's index, so that a step shaded with another record's bytes -- its ring neighbour's, 128 records on -- changes the image.

The reference of every case is the gather from the root at ONE split per wavefront: that item folds nothing, so the dropped top level of the
k-split fold (the launcher no longer allocates it) is checked against a sum that never had one.  One case is also held against the oracle's
gather with test_gpu_parity.py's bars, so that the file does not rest on the library alone."""
import functools
import math

import numpy as np
import pytest

import oracle_api as oa
import scenes
from test_gpu_parity import assert_image_close

pytestmark = pytest.mark.gpu

NPATHS, P = 80, 4                        # 320 record slots: up to 300 usable, three per split of 128
SLOTS = NPATHS * P
FRAMES = [(8, 8), (24, 16), (40, 24)]    # one tile; 3 x 2 tiles (ragged 2 x 2 cut groups); 5 x 3 tiles (a partial last tile-group column and row)
COUNTS = [0, 1, 127, 128, 129, 257, 300]  # splits with 0 .. 3 VPLs: shorter than, as long as and longer than the ring is deep; empty splits beside full ones


@functools.lru_cache(maxsize=None)
def frame_inputs(w, h):
    """(room, oracle scene, G-buffer with crafted materials, record pool) of a frame size"""
    room = scenes.box_room(seed=3, n_boxes=5, tess=2, aspect=w / h)
    osc = oa.Scene(room)
    gbuf = [p.copy() for p in osc.primary(w, h, (0.003, -0.002))[:4]]
    # material class of a pixel: 0 Lambertian, 1 a Phong lobe (e != 0), 2 rho_s != 0 with e = 0 -- mixed within every tile
    yy, xx = np.mgrid[0:h, 0:w]
    cls = (xx + 2 * yy) % 3
    gbuf[2][..., :3] = np.stack([0.3 + 0.05 * (xx % 5), 0.6 - 0.04 * (yy % 7), 0.45 + 0.0 * xx], -1).astype(np.float32)
    rs = np.stack([0.30 + 0.01 * (xx % 3), 0.25 + 0.0 * xx, 0.20 + 0.02 * (yy % 2)], -1).astype(np.float32)
    gbuf[3][..., :3] = np.where((cls != 0)[..., None], rs, np.float32(0.0))
    gbuf[3][..., 3] = np.where(cls == 1, np.float32(12.0), np.float32(0.0))
    assert (gbuf[0][..., 3] != 0).any()
    pool = osc.trace_light_paths(5, NPATHS, P)
    pool = pool[(pool["flags"] & 1) != 0]
    assert pool.shape[0] >= 64
    return room, osc, gbuf, pool


def crafted_records(pool, usable):
    """SLOTS records on the pool's surface points; every field that is shaded with depends on the record's index; `usable` of them usable,
    scattered over the slots (the compaction keeps their order).  The first usable one is an emitter's own VPL: it lights the room alone."""
    rec = np.zeros(SLOTS, dtype=pool.dtype)
    j = np.arange(SLOTS)
    src = pool[j % pool.shape[0]]
    for f in ("pos", "normal", "flux_dir"):
        rec[f] = src[f]
    cls = j % 3                                   # as the pixels: Lambertian / Phong lobe / rho_s != 0 with e = 0
    rec["flux"] = 40.0 * ((0.5 + j / SLOTS)[:, None] * np.array([1.0, 0.8, 0.6]) + np.stack([0 * j, 0.01 * (j % 5), 0.02 * (j % 3)], -1)).astype(np.float32)
    rec["rho_d"] = np.stack([0.2 + 0.002 * j, 0.7 - 0.001 * j, 0.5 + 0.0 * j], -1).astype(np.float32)
    rec["rho_s"] = np.where((cls != 0)[:, None], np.stack([0.3 + 0.001 * j, 0.2 + 0.0 * j, 0.1 + 0.002 * (j % 50)], -1), 0.0).astype(np.float32)
    rec["phong_exp"] = np.where(cls == 1, 4.0 + (j % 9), 0.0).astype(np.float32)
    rec["p_select_lambert"] = np.where(cls == 0, 1.0, 0.55 + 0.001 * (j % 100)).astype(np.float32)
    assert len({tuple(f) for f in rec["flux"]}) == SLOTS
    rec["flags"] = 2                              # a photon only: not gathered
    order = np.random.RandomState(7).permutation(SLOTS)
    order = np.concatenate([[0], order[order != 0]])      # slot 0: the first record of the first light path, on the emitter
    rec["flags"][np.sort(order[:usable])] |= 1
    return rec


def frame_kw(osc, mode):
    return dict(camera_pos=osc.sd.cam_origin, mis_mode=mode, pdf_mc=0.35, clamping_value=0.02, photon_radius=0.05, num_light_paths=NPATHS,
                num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=0, rng_seed=5)


def gather_once(evplp, monkeypatch, w, h, usable, mode, k, cuts):
    room, osc, gbuf, pool = frame_inputs(w, h)
    rec = crafted_records(pool, usable)
    monkeypatch.delenv("EVPLP_GATHER_K", raising=False)
    if cuts:
        monkeypatch.delenv("EVPLP_CUTS", raising=False)
    else:
        monkeypatch.setenv("EVPLP_CUTS", "0")
    with evplp.Context(w, h, NPATHS, NPATHS, P, gather_splits_per_wave=k) as c:
        room.upload(c)
        for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), gbuf):
            pad = np.zeros((c.local_rows, w, 4), np.float32); pad[:h] = plane
            c.upload(b, pad)
        c.upload(evplp.BUF_RECORDS, rec)
        c.clear_accumulators()
        c.gather_vpl(evplp.frame_params(**frame_kw(osc, mode)))
        img = c.download(evplp.BUF_VPL_ACCUM)[:h].copy()
        st = c.pass_stats(evplp.PASS_GATHER_VPL)
    return img, (st["rays"], st["shaded"], st["usable"])


_REFERENCE = {}


def reference(evplp, monkeypatch, w, h, usable, mode):
    """from the root, one split per wavefront: computed once per (frame, records, mode), shared by the cases that differ in k only"""
    key = (w, h, usable, mode)
    if key not in _REFERENCE:
        img, st = gather_once(evplp, monkeypatch, w, h, usable, mode, 1, cuts=False)
        img.setflags(write=False)
        _REFERENCE[key] = (img, st)
    return _REFERENCE[key]


def check_against_root(evplp, monkeypatch, w, h, usable, mode, k):
    ref, ref_st = reference(evplp, monkeypatch, w, h, usable, mode)
    got, st = gather_once(evplp, monkeypatch, w, h, usable, mode, k, cuts=True)
    assert ref_st[2] == usable and st[2] == usable
    if usable > 0:
        assert ref[..., :3].max() > 0 and ref_st[0] > 0 and ref_st[1] > 0, "the reference shades nothing: the case checks nothing"
    else:
        assert not ref.any() and ref_st[:2] == (0, 0)
    assert np.isfinite(got).all()
    assert st[:2] == ref_st[:2], f"shadow rays / unoccluded pairs {st[:2]} with cuts, {ref_st[:2]} from the root"
    diff = int((got.view(np.uint32) != ref.view(np.uint32)).any(-1).sum())
    assert got.tobytes() == ref.tobytes(), f"{diff} of {w * h} pixels differ between the ring's records and the scalar fetch"


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("usable", COUNTS)
def test_ring_records_against_the_scalar_fetch_over_record_counts(evplp, monkeypatch, usable, k):
    check_against_root(evplp, monkeypatch, 24, 16, usable, 1, k)


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("frame", [FRAMES[0], FRAMES[2]], ids=lambda f: f"{f[0]}x{f[1]}")
def test_ring_records_against_the_scalar_fetch_over_frames(evplp, monkeypatch, frame, k):
    check_against_root(evplp, monkeypatch, frame[0], frame[1], 300, 1, k)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
def test_ring_records_against_the_scalar_fetch_in_every_mis_mode(evplp, monkeypatch, mode):
    check_against_root(evplp, monkeypatch, 40, 24, 257, mode, 2)


def test_every_branch_of_the_shading_runs_in_the_cases_above():
    """three material classes among the pixels of every tile and among the records of every split"""
    for w, h in FRAMES:
        _, _, gbuf, pool = frame_inputs(w, h)
        rs, e = gbuf[3][..., :3], gbuf[3][..., 3]
        for ty in range(0, h, 8):
            for tx in range(0, w, 8):
                t_rs, t_e = rs[ty:ty + 8, tx:tx + 8].reshape(-1, 3), e[ty:ty + 8, tx:tx + 8].reshape(-1)
                glossy = (t_rs != 0).any(-1)
                assert (~glossy).any() and (glossy & (t_e != 0)).any() and (glossy & (t_e == 0)).any()
    rec = crafted_records(frame_inputs(24, 16)[3], 300)
    u = rec[(rec["flags"] & 1) != 0]
    glossy = (u["rho_s"] != 0).any(-1)
    assert (~glossy).sum() > 50 and (glossy & (u["phong_exp"] != 0)).sum() > 50 and (glossy & (u["phong_exp"] == 0)).sum() > 50
    assert (u["rho_s"][glossy][:, 0] > 1e-6).all()      # (the MIS weights' own test of the lobe, on rho_s.x)


@pytest.mark.parametrize("mode", [1, 5])
def test_ring_records_against_the_oracle(evplp, monkeypatch, mode):
    w, h, usable = 40, 24, 300
    room, osc, gbuf, pool = frame_inputs(w, h)
    rec = crafted_records(pool, usable)
    got, st = gather_once(evplp, monkeypatch, w, h, usable, mode, 2, cuts=True)
    fp = oa.frame_params(**frame_kw(osc, mode))
    ref, pairs = osc.gather(fp, w, h, gbuf, rec)
    assert st[2] == usable
    assert st[:2] == osc.gather_counts(fp, w, gbuf, rec, np.arange(h))
    assert ref[..., :3].max() > 0
    assert_image_close(got[..., :3], ref[..., :3], what=f"ring gather, mode {mode}")
