"""What a free-standing batch of rays costs (evplp_trace_closest_device / evplp_trace_occluded_device) beside the project's own walks.
One process, the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), the camera rays of a 1920 x 1080 frame on the
device, `reps` repetitions after `warmup`, HIP events on the stream the context launches on; the three batches take turns inside every
repetition, so that whatever else the machine does falls on all of them alike.

  (a) the rays in pixel order,
  (b) the same rays shuffled (seeded),
  (c) the shuffled rays with the ordering pass (EVPLP_QUERY_ORDER): its key kernel and its sort are inside the measured interval.

For each: Mrays/s of closest hit and of occlusion, median with p10 - p90.  Beside them, in the same run: evplp_primary of the same frame (the
packet walk from the eye's entry cuts) and evplp_trace_light_paths of 300 000 paths (per ray traced: the oracle-checked record structure says
how many segments a path had).  The one decision the figures carry is the binding's default for `order` (evplp_amd.QUERY_ORDER_DEFAULT): on
only if (c) beats (b) by more than the spread of (b) over its own repetitions.

usage: python tools/query_times.py [--reps N] [--warmup N] [--tris N] [--width N] [--height N] [--paths N]"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402
import walk_replay as wr  # noqa: E402

P = 4
F = np.float32


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]       # noqa: E731
    return statistics.median(xs), q(0.1), q(0.9)


def timed(fn):
    """HIP-event time of fn's launches in ms (fn enqueues on torch's current stream, which the context was given)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--paths", type=int, default=300000)
    a = ap.parse_args()
    Wd, Ht = a.width, a.height
    with tempfile.TemporaryDirectory() as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, Wd, Ht, style="hard"))
    ntri = sum(m["idx"].shape[0] for m in sd.meshes)
    eye, dirs = wr.primary_rays(sd, Wd, Ht)
    n = Wd * Ht
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = eye; rays[:, 3] = 1e-4; rays[:, 4:7] = dirs.reshape(-1, 3); rays[:, 7] = 3.0e38
    perm = np.random.RandomState(7).permutation(n)
    # (torch's default stream is the null stream, which evplp_set_stream reads as "the context's own": a stream of torch's making carries
    # the launches, the events around them and the copies that read the results)
    stream = torch.cuda.Stream()
    with ev.Context(Wd, Ht, a.paths, 1024, P) as c, torch.cuda.stream(stream):
        sd.upload(c)
        c.set_stream(stream.cuda_stream)
        info = c.accel_info()
        print(f"scene: {ntri} triangles, builder {info['builder']}, depth {info['depth']}, stack4_entries {info['stack4_entries']}; {n} camera rays ({Wd} x {Ht}), "
              f"{(n + ev.QUERY_CHUNK_RAYS - 1) // ev.QUERY_CHUNK_RAYS} launches of at most {ev.QUERY_CHUNK_RAYS} rays per batch; {a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90)")
        pixel, shuffled = torch.from_numpy(rays).cuda(), torch.from_numpy(rays[perm]).cuda()
        batches = [("(a) pixel order", pixel, False), ("(b) shuffled", shuffled, False), ("(c) shuffled + ordering pass", shuffled, True)]
        # the answers agree before anything is timed: the ordering pass and the shuffle change no hit
        ref = c.trace_closest(pixel).cpu().numpy()
        for name, t, order in batches[1:]:
            got = c.trace_closest(t, order=order).cpu().numpy()
            assert np.array_equal(got, ref[perm]), name
        hit = (ref[:, 3] >= 0).mean()
        occ = c.trace_occluded(pixel).cpu().numpy()
        assert np.array_equal(occ == 1, ref[:, 3] >= 0)
        times = {(name, k): [] for name, _, _ in batches for k in ("closest", "occluded")}
        primary, light, light_rays = [], [], 0
        jitter = (0.0, 0.0)
        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            for name, t, order in batches:
                ms = timed(lambda: c.trace_closest(t, order=order))
                if keep:
                    times[name, "closest"].append(ms)
                ms = timed(lambda: c.trace_occluded(t, order=order))
                if keep:
                    times[name, "occluded"].append(ms)
            ms = timed(lambda: c.primary(jitter, clear_light=True))
            if keep:
                primary.append(ms)
            ms = timed(lambda: c.trace_light_paths(3 + rep))
            if keep:
                light.append(ms)
        c.synchronize()
        rec = c.download(ev.BUF_RECORDS).reshape(a.paths, P)
        # a path traces one ray per record behind its first, and one more where it ended early on a miss or an absorbing hit: at least the
        # filled records behind the first -- the figure below counts those (a lower bound of the rays, so an upper bound of the time per ray)
        light_rays = int((rec["flags"][:, 1:] != 0).sum())
        print(f"camera rays that hit: {100 * hit:.1f} %")
        print(f"{'batch':32s} {'closest hit  Mrays/s':>34s} {'occlusion  Mrays/s':>34s} {'closest ms':>12s} {'occlusion ms':>12s}")
        rate = {}
        for name, _, _ in batches:
            cells = []
            for k in ("closest", "occluded"):
                med, lo, hi = spread(times[name, k])
                rate[name, k] = (n / med / 1e3, n / hi / 1e3, n / lo / 1e3)
                cells.append("%9.1f  (%.1f - %.1f)" % rate[name, k])
            print(f"{name:32s} {cells[0]:>34s} {cells[1]:>34s} {spread(times[name, 'closest'])[0]:12.3f} {spread(times[name, 'occluded'])[0]:12.3f}")
        med, lo, hi = spread(primary)
        print(f"evplp_primary of the same frame: {med:.3f} ms ({lo:.3f} - {hi:.3f}) = {n / med / 1e3:.1f} M pixels/s (two walks per pixel where the light is in view)")
        med, lo, hi = spread(light)
        print(f"evplp_trace_light_paths, {a.paths} paths: {med:.3f} ms ({lo:.3f} - {hi:.3f}); at least {light_rays} rays traced: {light_rays / med / 1e3:.1f} Mrays/s, {1e6 * med / light_rays:.3f} ns per ray")
        for k in ("closest", "occluded"):
            b, cc = rate["(b) shuffled", k], rate["(c) shuffled + ordering pass", k]
            gain, width = cc[0] - b[0], b[2] - b[1]
            print(f"ordering pass, {k}: (c) - (b) = {gain:+.1f} Mrays/s against a p10 - p90 spread of (b) of {width:.1f}: {'beats it' if gain > width else 'does not beat it'}")


if __name__ == "__main__":
    main()
