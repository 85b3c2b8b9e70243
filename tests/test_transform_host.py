"""No GPU needed: the arithmetic and the surface of evplp_transform_mesh.  transform_point (evplp_types.h) is the one function that moves a
point -- on the host copy of a mesh, in refit_transform_kernel, and in evplp_transform_points, which hands it to callers and to this test.
It is restated here in numpy fp32, three products and three sums per row, each rounded on its own; a restatement that rounds once (fp64,
then to fp32: what a fused multiply-add chain would give on many inputs) must differ, or the test could not see a contraction."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_transform_mesh", "evplp_group_transform_mesh", "evplp_transform_points")
F = np.float32


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    types = open(os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")).read()
    assert re.search(r"__host__ __device__ inline void transform_point\(const float m\[12\], const float p\[3\], float out\[3\]\)", types)
    L = evplp.lib()
    m = np.eye(3, 4, dtype=F)
    p = np.zeros((2, 3), F)
    assert L.evplp_transform_mesh(None, 0, m.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_group_transform_mesh(None, 0, m.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_transform_points(None, p.ctypes.data, p.ctypes.data, 2) == evplp.ERR_INVALID
    assert L.evplp_transform_points(m.ctypes.data, None, p.ctypes.data, 2) == evplp.ERR_INVALID
    assert L.evplp_transform_points(m.ctypes.data, p.ctypes.data, None, 2) == evplp.ERR_INVALID
    assert L.evplp_transform_points(m.ctypes.data, p.ctypes.data, p.ctypes.data, -1) == evplp.ERR_INVALID
    assert L.evplp_transform_points(m.ctypes.data, None, None, 0) == evplp.OK
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    assert callable(evplp.Context.transform_mesh) and callable(evplp.Group.transform_mesh) and callable(evplp.transform_points)


def test_the_header_states_the_contract():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("Transforms do NOT compose", "a coordinate of -0.0 becomes +0.0", "evplp_update_mesh sets a new rest pose and forgets the matrix",
                   "a transformed coordinate that is not finite", "A singular matrix is legal", "ONE launch per refit",
                   "a context that never transforms allocates none of it", "rest pose (after a call)"):
        assert needle in hdr, needle


# ---- the arithmetic
def restate_fp32(m, p):
    """out[r] = ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3]: every product and every sum an np.float32 operation"""
    m = np.asarray(m, F).reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    for r in range(3):
        a, b, c = m[r, 0] * x, m[r, 1] * y, m[r, 2] * z
        assert a.dtype == F and b.dtype == F and c.dtype == F
        out[:, r] = ((a + b) + c) + m[r, 3]
    return out


def restate_rounded_once(m, p):
    m = np.asarray(m, F).reshape(3, 4).astype(np.float64)
    q = p.astype(np.float64)
    return (q @ m[:, :3].T + m[:, 3]).astype(F)


def points():
    rng = np.random.default_rng(20)
    tiny = np.finfo(F).tiny
    parts = [rng.uniform(-10, 10, (60000, 3)),
             rng.uniform(-1, 1, (10000, 3)) * 1e18, rng.uniform(-1, 1, (10000, 3)) * 1e-18,
             rng.uniform(-1, 1, (10000, 3)) * tiny,                                            # subnormals
             rng.choice([0.0, -0.0, 1.0, -1.0, tiny / 8, -tiny / 8, 1e18, -1e-18], (10000, 3))]   # +-0 against everything else
    p = np.concatenate(parts).astype(F)
    assert p.shape == (100000, 3) and np.isfinite(p).all()
    assert (np.signbit(p) & (p == 0)).any() and ((p != 0) & (np.abs(p) < tiny)).any() and (np.abs(p) > 1e17).any()
    return p


def matrices():
    c, s = math.cos(math.radians(25.0)), math.sin(math.radians(25.0))
    return {"identity": np.eye(3, 4), "translation": [1, 0, 0, 0.35, 0, 1, 0, -0.2, 0, 0, 1, 0.0],
            "rotation": [c, -s, 0, 1.25, s, c, 0, -0.75, 0, 0, 1, 0], "non-uniform scale": [1.4, 0, 0, 0, 0, 0.7, 0, 0, 0, 0, 3.1, -0.5],
            "a zero row": [0.3, 0.2, -0.9, 2.0, 0, 0, 0, 0, 1.1, -0.4, 0.6, 1e-18], "zero": np.zeros(12),
            "general": [0.3, 0.2, -0.9, 2.0, -0.7, 0.11, 0.5, -3.0, 1.1, -0.4, 0.6, 0.125], "large": [1e18, -3e17, 2e18, 1.0, 1e-18, 2e-18, -1e-18, 1e-30, 1, 1, 1, 1]}


def test_transform_points_is_the_fp32_restatement_bit_for_bit(evplp):
    p = points()
    seen_a_difference = 0
    for name, m in matrices().items():
        m = np.asarray(m, F).reshape(12)
        got = evplp.transform_points(m, p)
        assert got.dtype == F and got.shape == p.shape
        want = restate_fp32(m, p)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        once = restate_rounded_once(m, p)
        seen_a_difference += int((got.view(np.uint32) != once.view(np.uint32)).sum())
        if name in ("rotation", "general"):
            assert (got.view(np.uint32) != once.view(np.uint32)).any(), f"{name}: rounding once gives the same bits -- the test could not see a fused operation"
    assert seen_a_difference > 1000
    # the identity keeps every bit but the sign of a zero
    ident = evplp.transform_points(np.eye(3, 4, dtype=F), p)
    zero = p == 0
    assert np.array_equal(ident.view(np.uint32)[~zero], p.view(np.uint32)[~zero])
    assert not ident.view(np.uint32)[zero].any(), "-0.0 becomes +0.0 under the identity"
    # in place
    q = p.copy()
    m = np.asarray(matrices()["general"], F)
    assert evplp.lib().evplp_transform_points(m.ctypes.data, q.ctypes.data, q.ctypes.data, q.shape[0]) == evplp.OK
    assert np.array_equal(q.view(np.uint32), restate_fp32(m, p).view(np.uint32))


# ---- the "animation" block of the technique JSON: refused by key name before any group exists (as tests/test_denoise_host.py's block)
W, H = 96, 64
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _render(evplp, path, overrides=None):
    err = C.create_string_buffer(1024)
    rc = evplp.lib().evplp_render_json(str(path).encode(), overrides.encode() if overrides else None, 0, err, 1024)
    return rc, err.value.decode()


@pytest.fixture
def scene_file(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)


def _technique_file(scene_file, tmp_path, technique):
    root = json.load(open(scene_file))
    root["photonfam"]["timeLimitMs"] = 1e9
    root["photonfam"]["numMaxIteration"] = 2
    if technique == "pt":
        root["pt"] = {"rngOffset": 0, "numMaxIteration": 2, "timeLimitMs": 1e9, "frameMode": "accumulate", "outputFilename": "pt.pfm",
                      "statFilename": "pt.json", "useJitter": True, "useStat": True, "numSamplePerPixel": 1, "numMaxBounces": 3}
        root.pop("photonfam")
    elif technique == "lvcphotonfam":
        root["lvcphotonfam"] = root.pop("photonfam")
    jp = tmp_path / f"{technique}.json"
    jp.write_text(json.dumps(root))
    return jp, len(root["scene"])


def _anim(frames=2, tracks=None, **kw):
    block = {"frames": frames, "tracks": [{"mesh": 0, "matrices": [EYE] * 2}] if tracks is None else tracks}
    block.update(kw)
    return json.dumps({"animation": block})


@pytest.mark.parametrize("technique", ["photonfam", "lvcphotonfam", "pt"])
def test_bad_animation_blocks_are_refused_before_any_gpu_work(evplp, scene_file, tmp_path, technique):
    jp, n_objects = _technique_file(scene_file, tmp_path, technique)
    two = [EYE] * 2
    nan = [EYE, EYE[:11] + [1e300]]                                          # (no fp32 number; JSON has no NaN)
    cases = [
        (json.dumps({"animation": 3}), ["animation"]),
        (_anim(frames=0), ["animation.frames"]),
        (_anim(frames=-2), ["animation.frames"]),
        (json.dumps({"animation": {"tracks": []}}), ["animation.frames"]),
        (_anim(tracks=[{"matrices": two}]), ["animation.tracks[0]", "object", "mesh"]),
        (_anim(tracks=[{"mesh": 0, "object": 0, "matrices": two}]), ["animation.tracks[0]", "object", "mesh"]),
        (_anim(tracks=[{"mesh": -1, "matrices": two}]), ["animation.tracks[0].mesh", "out of range"]),
        (_anim(tracks=[{"mesh": 10 ** 6, "matrices": two}]), ["animation.tracks[0].mesh", "out of range"]),
        (_anim(tracks=[{"object": n_objects, "matrices": two}]), ["animation.tracks[0].object", "out of range"]),
        (_anim(tracks=[{"object": -1, "matrices": two}]), ["animation.tracks[0].object", "out of range"]),
        (_anim(tracks=[{"object": "chair", "matrices": two}]), ["animation.tracks[0].object", "arealight"]),
        (_anim(tracks=[{"mesh": 0, "matrices": [EYE]}]), ["animation.tracks[0].matrices"]),
        (_anim(tracks=[{"mesh": 0, "matrices": [EYE] * 3}]), ["animation.tracks[0].matrices"]),
        (_anim(tracks=[{"mesh": 0}]), ["animation.tracks[0].matrices"]),
        (_anim(tracks=[{"mesh": 0, "matrices": [EYE, EYE[:11]]}]), ["animation.tracks[0].matrices[1]"]),
        (_anim(tracks=[{"mesh": 0, "matrices": [EYE, EYE[:11] + ["x"]]}]), ["animation.tracks[0].matrices[1]"]),
        (_anim(tracks=[{"mesh": 0, "matrices": nan}]), ["animation.tracks[0].matrices[1]", "finite"]),
        (_anim(tracks=[{"mesh": 0, "matrices": two}, {"mesh": 0, "matrices": two}]), ["animation.tracks[1]", "two of the animation.tracks"]),
        (_anim(tracks=[{"object": 0, "matrices": two}, {"mesh": 0, "matrices": two}]), ["animation.tracks[1]", "two of the animation.tracks"]),
        (json.dumps({"animation": {"frames": 2, "tracks": [{"mesh": 0, "matrices": two}]}, "timeLimitMs": 500}), ["animation", "timeLimitMs"]),
        (json.dumps({"animation": {"frames": 2, "tracks": [{"mesh": 0, "matrices": two}]}, "numMaxIteration": 0}), ["animation", "numMaxIteration"]),
        (_anim(refitPolicy={"maxCostRatio": -1}), ["animation.refitPolicy.maxCostRatio"]),
        (_anim(refitPolicy={"maxCostRatio": 1.5, "rebuildBuilder": "best"}), ["animation.refitPolicy.rebuildBuilder"]),
        # (evplp_set_refit_policy refuses PLOC as a rebuild builder, include/evplp.h: the block says so before any group exists)
        (_anim(refitPolicy={"maxCostRatio": 1.5, "rebuildBuilder": "ploc"}), ["animation.refitPolicy.rebuildBuilder", "bvhBuilder"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    written = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".pfm", ".ppm", ".png", ".exr"))
    assert not written, written


@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_a_valid_animation_block_gets_past_validation(evplp, scene_file, tmp_path, technique):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_transform.py)")
    jp, n_objects = _technique_file(scene_file, tmp_path, technique)
    rc_plain, msg_plain = _render(evplp, jp)
    tracks = [{"object": 0, "matrices": [EYE] * 2}, {"object": "arealight", "matrices": [EYE] * 2}]
    rc, msg = _render(evplp, jp, _anim(tracks=tracks, refitPolicy={"maxCostRatio": 1.5, "rebuildBuilder": "gpu"}))
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "animation" not in msg, msg
