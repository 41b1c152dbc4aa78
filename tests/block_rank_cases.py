"""Frames for tests/test_gpu_block_rank.py: the smallest shapes at which ranking a workgroup's 512 pixels together
(pbr_balanced.h) can go wrong, each shaded in both modes by a context that ranks per block where the vote allows it
and by one that ranks per wave everywhere (PBR_RANK_PER_WAVE=1).

Run in-process against the product library, and as a child process (`python tests/block_rank_cases.py OUT.npz`)
against the bounds-checked build (PBR_LIB_PATH), which then also stores the pbr_debug_bounds report of every pass.
A workgroup is a 64x8-pixel tile; wave w of it shades tile rows 2w and 2w + 1.
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("faithful", "exact")
RANKINGS = {"block": {"PBR_BALANCED_MIN": "1"}, "wave": {"PBR_BALANCED_MIN": "1", "PBR_RANK_PER_WAVE": "1"}}
CLASSES = ("gbuffer", "output", "coverage", "texel", "light", "lds")


def _scene(rng, w, h, n_lights):
    """Pixels in z >= 0 with random unit normals, lights in z <= 0: every pixel and light inside the fast window."""
    n = w * h
    pos = np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.uniform(0, 10, n)], 1)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    planes = np.zeros((15, h, w), np.float32)
    planes[0:3] = pos.T.reshape(3, h, w)
    planes[3:6] = nrm.T.reshape(3, h, w)
    planes[6:9] = rng.uniform(0, 1, (3, h, w))
    planes[9] = rng.uniform(0, 1, (h, w))
    planes[10] = rng.uniform(0, 1, (h, w))
    planes[11] = 1.0
    lights = np.zeros((n_lights, 12), np.float32)
    lights[:, 0:3] = rng.uniform(0, 100, (n_lights, 3))
    lights[:, 8:11] = np.stack([rng.uniform(-20, 20, n_lights), rng.uniform(-20, 20, n_lights),
                                rng.uniform(-20, 0, n_lights)], 1)
    return planes, lights


def _shape(w, h, seed, nl=64):
    planes, lights = _scene(np.random.default_rng(seed), w, h, nl)
    return {"planes": planes, "lights": lights}


def _background_wave():
    """64x16, two workgroups; coverage makes wave 1 of the lower one (rows 10-11) background: that workgroup's vote
    fails and its three other waves rank alone, the upper workgroup ranks together."""
    c = _shape(64, 16, 31)
    cov = np.ones((16, 64), np.uint8)
    cov[10:12] = 0
    c["coverage"] = cov
    return c


def _rows_differ():
    """One workgroup whose waves differ as much as they can: rows 0-1 face every light (64 live each: the lights are
    all at smaller z), rows 2-3 face away from all (0 live), rows 4-7 random. Wave 0's records go to the other waves'
    slots as second pixels and wave 1's come to wave 0 as first pixels."""
    c = _shape(64, 8, 32)
    c["planes"][3:6, 0:2] = np.array([0.0, 0.0, -1.0], np.float32)[:, None, None]
    c["planes"][3:6, 2:4] = np.array([0.0, 0.0, 1.0], np.float32)[:, None, None]
    return c


def _lights(n):
    return _shape(128, 8, 100 + n, n)


def _redo_across_waves():
    """Pixels that leave the fast window for a live item, in wave 3 (rows 6-7) of the first of two workgroups, with
    normals that keep most lights live, so their records rank high and are evaluated by low threads of the workgroup:
    * (5, 6): light 0 lies 0.005 in front of it (inside the faithful distance window of 0.01, decided in pass 1);
    * (9, 7): eye, pixel and light 1 are collinear along x with the pixel between them, so L = -V exactly and
      |V + L| = 0 (a NaN length in pass 2's Newton sqrt);
    * (20, 6): the eye is straight above it along z and light 2 straight below but for 2^-30 in y (the pixel's and the
      eye's y are 2^-20 and the light's 2^-20 + 2^-30, all inside the fast window's "0 or >= 2^-20", so
      l = (0, 2^-30, -7) exactly): |V + L| = 2^-30 / 7, nonzero and below the 2^-30 window.
    For the last two the evaluating lane's `fail` flag has to come back to the owner with the result. All three must
    be redone on the exact path, whichever lane evaluated them (exact mode: the last two; 0.005 is inside its distance
    window of 2^-20)."""
    c = _shape(128, 8, 33)
    nrm = np.array([-0.5, 0.0, -0.75 ** 0.5], np.float32)
    c["planes"][0:3, 6, 5] = (1.0, 2.0, 3.0)
    c["planes"][3:6, 6, 5] = nrm
    c["lights"][0, 8:11] = c["planes"][0:3, 6, 5] + np.float32(0.005) * nrm
    y0 = 2.0 ** -20
    c["planes"][0:3, 7, 9] = (1.0, y0, 3.0)
    c["planes"][3:6, 7, 9] = nrm
    c["lights"][1, 8:11] = (-6.0, y0, 3.0)
    c["planes"][0:3, 6, 20] = (6.0, y0, 1.0)
    c["planes"][3:6, 6, 20] = nrm
    c["lights"][2, 8:11] = (6.0, y0 + 2.0 ** -30, -6.0)
    c["eye"] = (6.0, y0, 3.0)
    c["min_redo"] = {"faithful": 3, "exact": 2}
    return c


def _outside_window():
    """Three workgroups; one pixel of wave 2 of the middle one lies outside the fast window (|x| > 2^20), so that wave
    leaves the balanced path: the middle workgroup ranks per wave, its neighbours per block."""
    c = _shape(192, 8, 34)
    c["planes"][0, 4, 64 + 17] = 3.0e6
    c["min_redo"] = {"faithful": 1, "exact": 1}
    return c


def cases():
    """{name: {planes, lights, [eye], [coverage], [min_redo]}}"""
    out = {
        "64x8": _shape(64, 8, 21),       # one workgroup
        "128x8": _shape(128, 8, 22),     # two: nothing may leak between them
        "70x11": _shape(70, 11, 23),     # partial workgroups (lanes and waves outside the frame) beside full ones
        "203x37": _shape(203, 37, 24),
        "background_wave": _background_wave(),
        "rows_differ": _rows_differ(),
        "redo_across_waves": _redo_across_waves(),
        "outside_window": _outside_window(),
    }
    for n in (1, 31, 32, 33, 64):  # mask-word boundaries; PBR_BALANCED_MIN=1 takes every count to the balanced kernels
        out[f"lights{n}"] = _lights(n)
    return out


def pass_constants(case, mode):
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import PassConstants

    kw = {"eye_pos_w": tuple(case["eye"])} if "eye" in case else {}
    return PassConstants(num_point_lights=len(case["lights"]), lights_array=case["lights"],
                         flags=N.PBR_FLAG_FAITHFUL if mode == "faithful" else 0, **kw)


def _context(env_vars):
    from physically_based_renderer_amd.renderer import ShadingContext

    saved = {k: os.environ.get(k) for k in ("PBR_BALANCED_MIN", "PBR_RANK_PER_WAVE")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env_vars)
    try:
        return ShadingContext(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(report_bounds: bool):
    """{ranking.case.mode: frame, + '.kernel': the kernel launched, + '.stats': the pass statistics (sorted by name)}
    and, with report_bounds, + '.bounds': the last offending index per class, -1 where the class was clean."""
    import torch

    from physically_based_renderer_amd import envmap
    from physically_based_renderer_amd.renderer import GBuffer

    dev = torch.device("cuda", 0)
    sky = envmap.procedural_sky_rgba16()
    results = {}
    for ranking, env_vars in RANKINGS.items():
        ctx = _context(env_vars)
        if report_bounds:
            ctx.debug_bounds(reset=True)
        for name, case in cases().items():
            gb = GBuffer.from_host(case["planes"], dev)
            for mode in MODES:
                ctx.set_pass(pass_constants(case, mode))
                if "coverage" in case:
                    ctx.set_sky_map(sky)
                    out = ctx.shade_frame(gb, coverage=torch.from_numpy(case["coverage"]).to(dev))
                else:
                    out = ctx.shade(gb)
                torch.cuda.synchronize()
                key = f"{ranking}.{name}.{mode}"
                results[key] = np.ascontiguousarray(out.cpu().numpy())
                results[key + ".kernel"] = np.array(ctx.last_kernel())
                st = ctx.pass_stats()
                results[key + ".stats"] = np.array([int(st[k]) for k in sorted(st)], np.int64)
                if report_bounds:
                    bad = ctx.debug_bounds(reset=True)
                    results[key + ".bounds"] = np.array([bad.get(n, -1) for n in CLASSES], np.int64)
        ctx.close()
    return results


if __name__ == "__main__":
    res = run(report_bounds=True)
    np.savez(sys.argv[1], **{k.replace(".", "__"): v for k, v in res.items()})
    print(f"block_rank_cases: {sum(1 for k in res if k.endswith('.bounds'))} passes", flush=True)
