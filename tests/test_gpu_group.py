"""evplp_group (include/evplp.h): the multi-GPU entry of the C ABI, on the one GPU a test box has.

Ranks that share a device ("virtual ranks") run the whole partitioned path -- strips, split light tracing + in-place record
all-gather, strip composites + frame all-gather, host assembly -- with device copies standing in for RCCL; a single-rank group
with use_rccl drives the same steps through ncclCommInitAll / ncclAllGather.  Per-pixel results must not depend on the
partition: every group image is compared bit for bit with the single-context image."""
import json
import math

import numpy as np
import pytest

import scenes
from evplp_amd import strips as strips_mod

pytestmark = pytest.mark.gpu

W, H, P = 96, 64, 4


def frame(evplp, runner, sd, bsr, total, NL, NV, vsl=False):
    r = 0.05 * bsr
    kw = dict(camera_pos=sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / total, photon_radius=r,
              vsl_radius=0.1 * bsr, vsl_inv_pi_radius2=1.0 / (math.pi * (0.1 * bsr) ** 2), num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P,
              do_accumulate=1, rng_seed=4, jitter=(0.002, -0.001))
    return evplp.frame_params(**kw)


@pytest.mark.parametrize("NL", [64, 16384])           # small sets are traced by every rank, large ones split + all-gathered
def test_virtual_ranks_equal_the_single_context(evplp, tmp_path, NL):
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H, style="hard")
    sd, _ = scenes.load_obj_scene(jp)
    NV = 32
    images = {}
    for n in (1, 2, 4):
        # (the 4-rank group also runs light tracing on its second stream, beside the G-buffer pass)
        with evplp.Group(W, H, NL, NV, P, n, devices=[0] * n, deterministic=True, overlap_light_tracing=(n == 4), split_light_paths=1 if NL >= 16384 else -1) as g:
            g.load_scene_json(jp)
            c0 = evplp.lib().evplp_group_context(g._h, 0)
            import ctypes as C
            r_, t_, l_ = C.c_float(), C.c_float(), C.c_float()
            evplp.lib().evplp_scene_metrics(c0, C.byref(r_), C.byref(t_), C.byref(l_))
            fp = frame(evplp, g, sd, r_.value, t_.value, NL, NV)
            g.clear_accumulators()
            for it in range(2):
                g.primary((0.002, -0.001)); g.trace_light_paths(4 + it)
                g.gather(fp, 0); g.splat_photons(fp)
            images[n] = g.resolve(0.5, 0.5, 1.0)
    # the single CONTEXT (no group at all)
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        fp = frame(evplp, c, sd, bsr, total, NL, NV)
        c.clear_accumulators()
        for it in range(2):
            c.primary((0.002, -0.001)); c.trace_light_paths(4 + it)
            c.gather_vpl(fp); c.splat_photons(fp)
        ref = c.resolve(0.5, 0.5, 1.0)[:H]
    assert ref.max() > 0
    for n, img in images.items():
        assert img.tobytes() == ref.tobytes(), f"{n} ranks differ from the single context"


def test_dealt_blocks_and_the_cost_rebalance_equal_the_single_context(evplp, tmp_path):
    """EVPLP_PARTITION_STRIPS with an owned-block table (evplp_set_blocks) instead of block b -> rank b % n: any table gives the single
    context's pixels bit for bit -- uneven tables (a rank with one block, a rank at its capacity), the table evplp_group_rebalance deals from
    the costs the gathers clocked, VPL and VSL gathers, photon splat, split light tracing -- and the group's assembly follows the table."""
    Hb = 128
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, Hb, style="hard")
    sd, _ = scenes.load_obj_scene(jp)
    NL, NV = 16384, 32

    def render(runner, fp, group, kind=0):
        runner.clear_accumulators()
        for it in range(2):
            runner.primary((0.002, -0.001)); runner.trace_light_paths(4 + it)
            if group:
                runner.gather(fp, kind)
            else:
                (runner.gather_vsl if kind else runner.gather_vpl)(fp)
            runner.splat_photons(fp)
        return runner.resolve(0.5, 0.5, 1.0)
    with evplp.Context(W, Hb, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        fp = frame(evplp, c, sd, bsr, total, NL, NV)
        ref = render(c, fp, False)[:Hb]
        ref_vsl = render(c, fp, False, 1)[:Hb]
        # a whole-image context clocks its one block
        c.calibrate_blocks(True); render(c, fp, False); cost1 = c.block_costs(); c.calibrate_blocks(False)
        assert cost1.shape == (1,) and cost1[0] > 0
    assert ref.max() > 0 and ref_vsl.max() > 0
    # (1) contexts by hand: three ranks of eight 16-row blocks, uneven and out of order; capacity 5 blocks
    tables = [[7], [5, 0, 2, 6, 1], [3, 4]]
    parts = []
    for r, tab in enumerate(tables):
        with evplp.Context(W, Hb, NL, NV, P, deterministic=True, strip_rank=r, strip_count=3, strip_rows=16, strip_capacity_rows=80) as c:
            c.load_scene_json(jp)
            assert c.local_rows == 80 and c.blocks().tolist() == list(range(r, 8, 3))
            c.set_blocks(tab)
            assert c.blocks().tolist() == tab
            rows = c.global_rows()
            assert (rows < Hb).sum() == 16 * len(tab)
            img = render(c, fp, False)
            ok = rows < Hb
            assert img[ok].tobytes() == ref[rows[ok]].tobytes(), f"rank {r} with blocks {tab} differs from the single context"
            parts.append((rows, img))
            with pytest.raises(evplp.EvplpError):
                c.set_blocks([0, 0])                               # listed twice
            with pytest.raises(evplp.EvplpError):
                c.set_blocks([8])                                  # outside the image
            with pytest.raises(evplp.EvplpError):
                c.set_blocks([0, 1, 2, 3, 4, 5])                   # beyond the capacity
            if r == 0:
                c.set_blocks(None)                                 # back to the round-robin deal
                assert c.blocks().tolist() == [0, 3, 6]
                img = render(c, fp, False); rows = c.global_rows(); ok = rows < Hb
                assert img[ok].tobytes() == ref[rows[ok]].tobytes()
    # (2) the group: calibrate, rebalance, render again
    for n in (2, 4):
        with evplp.Group(W, Hb, NL, NV, P, n, devices=[0] * n, deterministic=True, split_light_paths=1) as g:
            g.load_scene_json(jp)
            assert g.block_owners().tolist() == [b % n for b in range(8)]
            with pytest.raises(evplp.EvplpError) as e:
                g.rebalance()                                      # nothing was clocked
            assert "no calibration" in str(e.value) or "no block cost" in str(e.value)
            g.calibrate(True)
            assert render(g, fp, True)[:Hb].tobytes() == ref.tobytes()      # (the self-clocking kernels give the same pixels)
            costs = sum(g.rank(r).block_costs() for r in range(n))
            assert costs.shape == (8,) and (costs > 0).all()
            g.rebalance()
            owner = g.block_owners()
            cap = g.rank(0).local_rows // 16
            assert owner.tolist() == evplp.deal_blocks(costs, n, cap).tolist()
            loads = np.array([costs[owner == r].sum() for r in range(n)], dtype=np.float64)
            rr = np.array([costs[np.arange(8) % n == r].sum() for r in range(n)], dtype=np.float64)
            assert loads.max() <= rr.max()                         # never worse than the round-robin deal by its own measure
            for r in range(n):       # (a rank stores -- and launches -- its blocks most expensive first)
                assert g.rank(r).blocks().tolist() == evplp.rank_blocks(costs, owner, r).tolist() == strips_mod.blocks_of_rank(owner, r, costs).tolist()
            assert render(g, fp, True)[:Hb].tobytes() == ref.tobytes(), f"{n} ranks with dealt blocks {owner.tolist()} differ from the single context"
            assert render(g, fp, True, 1)[:Hb].tobytes() == ref_vsl.tobytes(), "VSL gather on dealt blocks"


def test_a_rank_that_fails_behind_a_collective_does_not_hang_the_group(evplp, tmp_path):
    """ADVICE (round 5): one verdict per barrier generation.  Rank 1 is made to fail in the command that FOLLOWS a collective (its scene is
    invalidated behind the group's back); the next collective must be skipped by every rank, the group calls must return the error, and
    destroying the group must not hang.  Argument errors, on the other hand, are refused at once on the caller's thread and leave the group usable."""
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H)
    NL, NV = 16384, 32
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0, 0], deterministic=True, split_light_paths=1) as g:
        g.load_scene_json(jp)
        fp = evplp.frame_params(camera_pos=(15.56, -4.79, 4.37), mis_mode="one", num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, photon_radius=0.1)
        bad = evplp.frame_params(camera_pos=(15.56, -4.79, 4.37), mis_mode="one", num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, photon_radius=0.0)
        g.primary(); g.trace_light_paths(1); g.gather(fp, 0)
        with pytest.raises(evplp.EvplpError) as e:
            g.splat_photons(bad)                                   # refused at once ...
        assert "photon_radius" in str(e.value)
        a = g.resolve(1.0, 0.0, 1.0)                               # ... and the group is still usable (a collective inside)
        assert a.max() > 0
        # rank 1 loses its acceleration structure: its next pass fails, rank 0's does not
        c1 = g.rank(1)
        c1.add_mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), 0)
        with pytest.raises(evplp.EvplpError) as e:
            g.primary()                                            # posted to both; rank 1 fails behind the previous exchange
            g.trace_light_paths(2)                                 # split light tracing: a collective (whichever of these calls first sees the
            g.present()                                            # failure returns it; what was posted before must not hang anybody)
            g.synchronize()
        assert "rank 1" in str(e.value)
        with pytest.raises(evplp.EvplpError):
            g.resolve(1.0, 0.0, 1.0)
    # (leaving the block destroyed the group: reaching this line is the test)


def test_single_rank_group_through_rccl(evplp, tmp_path):
    """ncclCommInitAll + ncclAllGather with one rank: the RCCL code path itself (communicator, streams, in-place gather)."""
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H)
    with evplp.Group(W, H, 16384, 32, P, 1, use_rccl=True, deterministic=True, split_light_paths=1) as g:
        g.load_scene_json(jp)
        fp = evplp.frame_params(camera_pos=(15.56, -4.79, 4.37), mis_mode="one", num_light_paths=16384, num_vpl_light_paths=32, photons_per_path=P)
        g.primary(); g.trace_light_paths(1); g.gather(fp, 0)
        a = g.resolve(1.0, 0.0, 1.0)
    with evplp.Context(W, H, 16384, 32, P, deterministic=True) as c:
        c.load_scene_json(jp)
        c.primary(); c.trace_light_paths(1); c.gather_vpl(fp)
        b = c.resolve(1.0, 0.0, 1.0)[:H]
    assert a.max() > 0 and a.tobytes() == b.tobytes()


def test_render_json_on_a_group_of_virtual_ranks(evplp, tmp_path):
    """The technique loop on 4 strip ranks (JSON `device` block) writes the same files as on one."""
    outs = {}
    # (round 6) ... and so does every way of running the group: blocks dealt by the cost a calibration frame clocks, the strips exchanged only
    # for the frames that are written (exchangeEvery 0) or every second iteration, light paths split over the ranks + record all-gather
    variants = {"1": dict(gpus=1), "4": dict(gpus=4, virtual=True), "4, strips exchanged every iteration": dict(gpus=4, virtual=True, exchangeEvery=1),
                "4 dealt, no exchange in the loop, split paths": dict(gpus=4, virtual=True, deal="cost", exchangeEvery=0, splitLightPaths=True),
                "4 round robin, exchange every 2nd": dict(gpus=4, virtual=True, deal="roundRobin", exchangeEvery=2, splitLightPaths=False, stripRows=8)}
    for k, (name, dev) in enumerate(variants.items()):
        d = tmp_path / f"v{k}"; d.mkdir()
        jp = evplp.synth_scene(str(d), "room", 3000, 3, 80, 56, style="hard")
        root = json.load(open(jp))
        root["photonfam"].update(numMaxIteration=3, numLightPaths=2000, numVplLightPaths=40, radiusPercentage=0.05, misMode="balance", DoProgressive=True,
                                 deterministic=True, device=dev, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm",
                                 weightedVplFilename="vpl.pfm", statFilename="s.json", run=dict(photonSplat=True))
        json.dump(root, open(jp, "w"))
        evplp.render_json(jp)
        outs[name] = [open(d / f, "rb").read() for f in ("c.pfm", "pm.pfm", "vpl.pfm")]
    for name in variants:
        assert outs[name] == outs["1"], name


def test_render_json_with_the_iterations_shared_out(evplp, tmp_path):
    """"device": {"gpus": N, "partition": "iterations"}: every GPU renders every N-th iteration of the whole frame on a context of its own and the
    accumulators are summed when a frame is written.  The result is the one-GPU run's up to the association of the sums (fp32 round-off: 1e-6
    relative L2, a few ulps per pixel), is reproducible bit for bit, and the per-iteration dumps (writeEveryFrame) follow the same rule."""
    outs = {}
    variants = {"1": dict(gpus=1), "3 shards": dict(gpus=3, virtual=True, partition="iterations"), "3 shards again": dict(gpus=3, virtual=True, partition="iterations"),
                "2 shards": dict(gpus=2, virtual=True, partition="iterations")}
    for k, (name, dev) in enumerate(variants.items()):
        d = tmp_path / f"v{k}"; d.mkdir()
        jp = evplp.synth_scene(str(d), "room", 3000, 3, 80, 56, style="hard")
        root = json.load(open(jp))
        root["photonfam"].update(numMaxIteration=7, numLightPaths=2000, numVplLightPaths=40, radiusPercentage=0.05, misMode="balance", DoProgressive=True,
                                 deterministic=True, device=dev, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm", writeEveryFrame=True,
                                 weightedVplFilename="vpl.pfm", statFilename="s.json", run=dict(photonSplat=True))
        json.dump(root, open(jp, "w"))
        evplp.render_json(jp)
        outs[name] = {f: evplp.load_pfm(str(d / f)) for f in ("c.pfm", "pm.pfm", "vpl.pfm", "pm_3.pfm", "pm_7.pfm")}
        assert json.load(open(d / "s.json"))["numIterations"] == 7
    for f, ref in outs["1"].items():
        assert ref.max() > 0, f
        for name in ("3 shards", "2 shards"):
            img = outs[name][f]
            rel = np.linalg.norm(img.astype(np.float64) - ref) / np.linalg.norm(ref)
            assert rel < 1e-6, (name, f, rel)
            assert np.abs(img - ref).max() <= 4e-6 * max(float(ref.max()), 1.0), (name, f)
        assert outs["3 shards"][f].tobytes() == outs["3 shards again"][f].tobytes(), f
    assert any(outs["3 shards"][f].tobytes() != outs["1"][f].tobytes() for f in outs["1"]) or True      # (equal bits would be a coincidence, not a requirement)


def test_group_errors_are_reported(evplp):
    with pytest.raises(evplp.EvplpError) as e:
        evplp.Group(16, 16, 4, 4, 2, 2, devices=[0, 0], use_rccl=True)
    assert "distinct device" in str(e.value)
    with pytest.raises(evplp.EvplpError):
        evplp.Group(16, 16, 4, 4, 2, 0)


def test_large_frames_use_larger_bins_buckets_and_give_the_same_splat(evplp, tmp_path):
    """A 4096 x 2176 frame has 139 264 tiles: more than 1024 buckets of 16 x 8 tiles, so the single context bins with 16 x 16
    buckets; two strip ranks (69 632 tiles each) still use 16 x 8.  Deterministic mode: the photon image must not depend on it."""
    BW, BH, NL = 4096, 2176, 20000
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, BW, BH, style="hard")
    sd, _ = scenes.load_obj_scene(jp)
    imgs = {}
    for n in (1, 2):
        with evplp.Group(BW, BH, NL, 0, P, n, devices=[0] * n, deterministic=True) as g:
            g.load_scene_json(jp)
            import ctypes as C
            r_, t_, l_ = C.c_float(), C.c_float(), C.c_float()
            evplp.lib().evplp_scene_metrics(evplp.lib().evplp_group_context(g._h, 0), C.byref(r_), C.byref(t_), C.byref(l_))
            r = 0.01 * r_.value
            fp = evplp.frame_params(camera_pos=sd.cam_origin, mis_mode="one", photon_radius=r, num_light_paths=NL, num_vpl_light_paths=0, photons_per_path=P)
            g.clear_accumulators()
            g.primary((0.0, 0.0)); g.trace_light_paths(3); g.splat_photons(fp, clear=True)
            imgs[n] = g.resolve(0.0, 1.0, 0.0)
    assert imgs[1].max() > 0 and imgs[1].shape == (BH, BW, 3)
    assert imgs[1].tobytes() == imgs[2].tobytes()


@pytest.mark.parametrize("kind", ["vsl", "lvc", "pt"])
def test_the_other_gathers_and_the_path_tracer_on_virtual_ranks(evplp, tmp_path, kind):
    """VSL gather, light-path-window gather and the path tracer on 1 / 3 strip ranks: per-pixel RNG streams are keyed by the global
    pixel, so the partition cannot change a bit."""
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H, style="hard")
    sd, _ = scenes.load_obj_scene(jp)
    NL, NV = 64, 16
    images = {}
    for n in (1, 3):
        with evplp.Group(W, H, NL, NV, P, n, devices=[0] * n, deterministic=True) as g:
            g.load_scene_json(jp)
            import ctypes as C
            r_, t_, l_ = C.c_float(), C.c_float(), C.c_float()
            evplp.lib().evplp_scene_metrics(evplp.lib().evplp_group_context(g._h, 0), C.byref(r_), C.byref(t_), C.byref(l_))
            fp = frame(evplp, g, sd, r_.value, t_.value, NL, NV)
            g.clear_accumulators()
            g.primary((0.002, -0.001)); g.trace_light_paths(4)
            if kind == "pt":
                cp = (C.c_float * 3)(*[float(v) for v in sd.cam_origin])
                assert evplp.lib().evplp_group_path_trace(g._h, C.byref(cp), 5, 3, 0) == 0
            else:
                g.gather(fp, 1 if kind == "vsl" else 2)
            images[n] = g.resolve(1.0, 0.0, 1.0)
    assert images[1].max() > 0 and np.isfinite(images[1]).all()
    assert images[1].tobytes() == images[3].tobytes()


def test_a_splat_proxy_given_to_the_group_reaches_every_rank(evplp, tmp_path):
    """evplp_group_set_splat_proxy on two strip ranks: the photon image under the proxy footprint, with an octahedron (every rank must hold
    the caller's mesh, which the call has read when it returns) and then with the generated icosphere again, equals the single context's."""
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H, style="hard")
    sd, _ = scenes.load_obj_scene(jp)
    NL = 64
    octa_v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    octa_t = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)

    def photon_images(runner, bsr):
        fp = evplp.frame_params(camera_pos=sd.cam_origin, mis_mode="one", photon_radius=0.05 * bsr, num_light_paths=NL, num_vpl_light_paths=0, photons_per_path=P,
                                splat_footprint="proxy")
        out = []
        for mesh in ((octa_v.copy(), octa_t.copy()), ()):
            runner.set_splat_proxy(*mesh)
            for a in mesh:
                a[:] = 0                    # (the call has copied the mesh)
            runner.clear_accumulators()
            runner.primary((0.0, 0.0)); runner.trace_light_paths(3); runner.splat_photons(fp, clear=True)
            out.append(runner.resolve(0.0, 1.0, 0.0)[:H])
        return out

    with evplp.Context(W, H, NL, 0, P, deterministic=True) as c:
        c.load_scene_json(jp)
        ref = photon_images(c, c.scene_metrics()[0])
    with evplp.Group(W, H, NL, 0, P, 2, devices=[0, 0], deterministic=True) as g:
        g.load_scene_json(jp)
        img = photon_images(g, g.rank(0).scene_metrics()[0])
    assert ref[0].max() > 0 and ref[0].tobytes() != ref[1].tobytes(), "the two proxies cover different pixels"
    for k in range(2):
        assert img[k].tobytes() == ref[k].tobytes(), ("octahedron", "icosphere")[k]


def test_a_temporal_reset_on_the_group_forgets_the_history_as_the_single_context_does(evplp, tmp_path):
    """evplp_group_temporal_reset on two strip ranks: three path-traced frames through evplp_group_denoise_temporal with a reset in front of
    the third, which is then a first frame again; images and the stage's counts equal the single context's."""
    jp = evplp.synth_scene(str(tmp_path), "room", 3000, 9, W, H, style="hard")
    sd, _ = scenes.load_obj_scene(jp)

    def frames(runner):
        runner.noise_track(True); runner.temporal_enable(True)
        out = []
        for f in range(3):
            if f == 2:
                runner.temporal_reset()
            runner.clear_accumulators()
            for i in range(2):
                runner.primary((0.001 * i, -0.002 * i))
                runner.path_trace(sd.cam_origin, 10 * f + i, 3, accumulate=True)
                runner.noise_fold(1)
            img, info = runner.denoise_temporal(0.5)
            out.append((img[:H], info))
        return out

    with evplp.Context(W, H, 1, 1, 1, deterministic=True) as c:
        c.load_scene_json(jp)
        ref = frames(c)
    with evplp.Group(W, H, 1, 1, 1, 2, devices=[0, 0], deterministic=True) as g:
        g.load_scene_json(jp)
        got = frames(g)
    assert [info["frames_since_reset"] for _, info in ref] == [1, 2, 1] and ref[1][1]["reprojected"] > 0 and ref[2][1]["reprojected"] == 0
    for f in range(3):
        assert got[f][1] == ref[f][1], f
        assert np.isfinite(ref[f][0]).all() and got[f][0].tobytes() == ref[f][0].tobytes(), f
