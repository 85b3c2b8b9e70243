"""Ray queries through an evplp_group: three virtual ranks on one GPU, in both partitions.  Scene and tree are replicated, rank r traces rays
[r n / 3, (r + 1) n / 3) into the caller's arrays, and the output equals one context's byte for byte -- for n = 1 000, for n = 2 (a rank
without a ray) and for n = 0.  A refusal comes on the caller's thread and the group still renders afterwards."""
import numpy as np
import pytest

import scenes
from test_gpu_ray_query import F, H, NP, P, W, context, free_points, rays_of, unit

pytestmark = pytest.mark.gpu

RANKS = 3


@pytest.mark.parametrize("partition", ["strips", "iterations"])
def test_three_ranks_give_one_contexts_bytes_and_a_refusal_leaves_the_group_rendering(evplp, partition):
    room = scenes.box_room(seed=3, n_boxes=6, tess=2, aspect=W / H)
    rng = np.random.RandomState(21)
    rays = rays_of(free_points(rng, 1000), unit(rng, 1000), 1e-4, rng.uniform(0.5, 20.0, 1000).astype(F))
    rays[333, 4:7] = 0.0                                         # an invalid ray at a rank's border
    with context(evplp, room) as c:
        want = {(n, f): c.trace_closest(rays[:n], f) for n in (1000, 2, 0) for f in (0, 1, 2)}
        want_o = {n: c.trace_occluded(rays[:n]) for n in (1000, 2, 0)}
    assert (want[1000, 0]["triangle"] >= 0).any() and (want[1000, 0]["triangle"] == -1).any() and want[1000, 0]["triangle"][333] == -2
    with evplp.Group(W, H, NP, NP, P, RANKS, devices=[0] * RANKS, deterministic=True, partition=partition) as g:
        for r in range(RANKS):
            room.upload(g.rank(r))
        for n in (1000, 2, 0):
            for f in (0, 1, 2):
                assert g.trace_closest(rays[:n], f).tobytes() == want[n, f].tobytes(), (n, f)
            assert g.trace_occluded(rays[:n]).tobytes() == want_o[n].tobytes(), n
        assert g.trace_closest(rays, 0, order=True).tobytes() == want[1000, 0].tobytes()
        # refused on the caller's thread: no worker has failed, the group goes on
        for call in (lambda: g.trace_closest(rays, 3), lambda: g.trace_closest(rays, -1)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_group_trace_closest" in str(e.value)
        L = evplp.lib()
        hits = np.full(1000 * 16, 0x5A, np.uint8); out = np.full(1000, 0x5A, np.uint8)
        assert L.evplp_group_trace_closest(g._h, rays.ctypes.data, -1, 0, 0, hits.ctypes.data) == evplp.ERR_INVALID
        assert L.evplp_group_trace_closest(g._h, None, 1000, 0, 0, hits.ctypes.data) == evplp.ERR_INVALID
        assert L.evplp_group_trace_occluded(g._h, rays.ctypes.data, 1000, 2, out.ctypes.data) == evplp.ERR_INVALID
        assert L.evplp_group_trace_occluded(g._h, rays.ctypes.data, 1000, 0, None) == evplp.ERR_INVALID
        assert (hits == 0x5A).all() and (out == 0x5A).all()
        g.transform_mesh(11, [1, 0, 0, 0.3, 0, 1, 0, 0.2, 0, 0, 1, 0.7])
        with pytest.raises(evplp.EvplpError) as e:                # a dirty scene, as every pass refuses it
            g.trace_occluded(rays)
        assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        g.refit_accel()
        moved = g.trace_closest(rays)
        assert moved.tobytes() != want[1000, 0].tobytes()
        g.primary((0.0, 0.0), 1)
        img = g.resolve(0.0, 0.0, 1.0)
        assert img.shape == (H, W, 3) and np.isfinite(img).all()
        assert g.trace_closest(rays).tobytes() == moved.tobytes()
