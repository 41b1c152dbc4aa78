"""The case table and frame builder of tests/test_gpu_ibl_paths.py, shared with tools/ab_frames.py.

WorldToSkyUV's pair forms (csrc/libm_f32_x2.h) run a main path for ordinary normals and patch the rest -- a zero
component, the exponent-gap shortcuts, a quotient at or above 2^25, |N.y| == 1 -- inside a wave-uniform branch;
special normals (NaN, out of the window, |N.y| > 1) take the scalar functions, and only waves without a special
element use the branch-free texel wrap. The frames here put every such case into the first element of a pixel pair,
into the second, and into both, each time beside an ordinary partner, in tiny frames of one to four 128-pixel wave
tiles (64 x 2 pixels each).
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((64, 2), (64, 8), (70, 3))  # (width, height): one tile, four tiles, a ragged one (two tiles across)
LIGHT_COUNTS = (24, 8, 0)            # balanced tile kernels (both modes' thresholds are below 24) | uniform | lean
ORDINARY = (0.48, 0.6, -0.64)        # the partner: every component ordinary, |N| = 1 to rounding


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _ulp(x, k):
    """x moved by k units in the last place (x finite, nonzero; k small)."""
    b = np.array([x], np.float32).view(np.int32)[0]
    return np.array([b + (k if x > 0 else -k)], np.int32).view(np.float32)[0]


def case_table():
    """[(name, (nx, ny, nz))] as float32 triples."""
    nz0 = np.float32(-0.0)
    cases = []
    axes = {"+y": (0, 1, 0), "-y": (0, -1, 0), "+x": (1, 0, 0), "-x": (-1, 0, 0), "+z": (0, 0, 1), "-z": (0, 0, -1)}
    for name, n in axes.items():
        cases.append((f"axis{name}", tuple(np.float32(c) for c in n)))
        cases.append((f"axis{name},-0", tuple(np.float32(c) if c else nz0 for c in n)))
    # atanf's row boundaries: atan2f(t, 1) with t at 7/16, 11/16, 19/16, 39/16 and both neighbours
    for t in (7 / 16, 11 / 16, 19 / 16, 39 / 16):
        for k in (-1, 0, 1):
            cases.append((f"row{t:.4f}{k:+d}ulp", (np.float32(1.0), np.float32(0.25), _ulp(np.float32(t), k))))
    # the largest exponent gap the fast-path window (2^-20 .. 16) admits, both ways and with x < 0
    tiny, big = np.float32(2.0 ** -19), np.float32(16.0)
    cases += [("gap z/x=2^-23", (big, np.float32(0.25), tiny)), ("gap z/x=2^23", (tiny, np.float32(0.25), big)),
              ("gap z/x=-2^-23", (-big, np.float32(0.25), tiny))]
    # outside the fast-path window (2^-30): the exact path's pixel; k = -30 is an exponent-gap shortcut for x < 0
    cases += [("out z=2^-30,x=1", (np.float32(1.0), np.float32(0.0), np.float32(2.0 ** -30))),
              ("out z=2^-30,x=-1", (np.float32(-1.0), np.float32(0.0), np.float32(2.0 ** -30)))]
    # asinf's regimes: |N.y| at 0.5, 0.975 (0x3f79999a) and 1, each with both neighbours, both signs
    for name, y in (("0.5", np.float32(0.5)), ("0.975", _f(0x3F79999A)), ("1", np.float32(1.0))):
        for k in (-1, 0, 1):
            for s in (1, -1):
                cases.append((f"ny={'-' if s < 0 else ''}{name}{k:+d}ulp",
                              (np.float32(0.6), np.float32(s) * _ulp(y, k), np.float32(0.3))))
    cases += [("ny>1", (np.float32(0.1), np.float32(1.5), np.float32(0.2))),
              ("ny<-1", (np.float32(0.1), np.float32(-2.0), np.float32(0.2)))]
    nan = np.float32(np.nan)
    cases += [("nan x", (nan, np.float32(0.5), np.float32(0.5))), ("nan y", (np.float32(0.5), nan, np.float32(0.5))),
              ("nan z", (np.float32(0.5), np.float32(0.5), nan))]
    return cases


def placements():
    """[(case name, placement, normal of element 0, normal of element 1)] for every case in the first element, the
    second, and both."""
    part = tuple(np.float32(c) for c in ORDINARY)
    out = []
    for name, n in case_table():
        out += [(name, "first", n, part), (name, "second", part, n), (name, "both", n, n)]
    return out


def frames(seed=20241):
    """[(label, planes (15, H, W) float32, pair names (H, W // 2))]: for every size as many frames as it takes to
    hold every (case, placement) pair once; a frame's remaining pairs repeat the list from its start. Everything but
    the normals is random inside the fast-path window."""
    pl = placements()
    out = []
    for w, h in SIZES:
        per_frame = (w // 2) * h
        n_frames = -(-len(pl) // per_frame)
        for f in range(n_frames):
            rng = np.random.default_rng(seed + 1000 * w + 10 * h + f)
            p = np.zeros((15, h, w), np.float32)
            p[0:3] = rng.uniform(-5.0, 5.0, (3, h, w))
            p[6:9] = rng.uniform(0.05, 1.0, (3, h, w))       # albedo
            p[9] = rng.uniform(0.0, 1.0, (h, w))             # metallic
            p[10] = rng.uniform(0.05, 1.0, (h, w))           # roughness
            p[11] = rng.uniform(0.2, 1.0, (h, w))            # ao
            p[12:15] = rng.uniform(0.02, 1.0, (3, h, w))     # F0 plane
            names = np.empty((h, w // 2), object)
            for y in range(h):
                for i in range(w // 2):
                    name, where, n0, n1 = pl[(f * per_frame + y * (w // 2) + i) % len(pl)]
                    p[3:6, y, 2 * i] = n0
                    p[3:6, y, 2 * i + 1] = n1
                    names[y, i] = f"{name}/{where}"
            out.append((f"{w}x{h}#{f}", p, names))
    return out


def lights(n, seed=7):
    """(n, 12) point lights around the pixels (positions in the window, in range of most pixels)."""
    rng = np.random.default_rng(seed)
    arr = np.zeros((max(n, 1), 12), np.float32)
    arr[:, 0:3] = rng.uniform(2.0, 12.0, (max(n, 1), 3))
    arr[:, 3] = 64.0
    arr[:, 4:7] = (0.0, -1.0, 0.0)
    arr[:, 8:11] = rng.uniform(-9.0, 9.0, (max(n, 1), 3))
    return arr[:n] if n else None


def coverage(w, h):
    """The coverage plane of the frame-path runs: background (0) on a sparse lattice, so that some pairs have one
    element that is not shaded geometry (special or not) beside a live one."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 3 * yy) % 11 != 0).astype(np.uint8)


def env_maps():
    """{name: (h, w, 4) uint16}: the Chelsea 360 x 180 map and 1 x 1, 2 x 1, 3 x 2 maps whose texels are all
    distinct in every channel (a wrong wrap changes the result)."""
    from physically_based_renderer_amd import envmap

    maps = {"chelsea": envmap.load_chelsea_stairs_env()}
    for w, h in ((1, 1), (2, 1), (3, 2)):
        t = np.zeros((h, w, 4), np.uint16)
        for y in range(h):
            for x in range(w):
                i = y * w + x
                t[y, x] = (4000 + 9000 * i, 60000 - 7000 * i, 15000 + 5000 * ((i * 5) % 7), 65535)
        maps[f"{w}x{h}"] = t
    return maps


def pass_constants(n_point, faithful):
    from physically_based_renderer_amd import _native as N
    from physically_based_renderer_amd.renderer import PassConstants

    flags = N.PBR_FLAG_F0_PLANE | N.PBR_FLAG_APPLY_AO | (N.PBR_FLAG_FAITHFUL if faithful else 0)
    return PassConstants(eye_pos_w=(0.5, 2.0, -10.0), num_point_lights=n_point, flags=flags,
                         ambient_mode=N.PBR_AMBIENT_IBL_DIFFUSE, lights_array=lights(n_point))


def shade_case(ctx, device, planes, n_point, faithful, env):
    """One frame through the kernel family of `n_point` (see LIGHT_COUNTS): (frame (H, W, 4) float32, pass stats,
    kernel name). 8 lights go through the frame path (coverage + sky pass), which keeps the pair kernel with uniform
    loops off the lean kernel."""
    import torch

    from physically_based_renderer_amd.renderer import GBuffer

    pc = pass_constants(n_point, faithful)
    ctx.set_pass(pc)
    ctx.set_env_map(env)
    gb = GBuffer.from_host(planes, device)
    if n_point == 8:
        ctx.set_sky_map(env)
        h, w = planes.shape[1:]
        cov = torch.from_numpy(coverage(w, h)).to(device)
        out = ctx.shade_frame(gb, coverage=cov)
    else:
        out = ctx.shade(gb)
    torch.cuda.synchronize(device)
    return out.cpu().numpy(), ctx.pass_stats(), ctx.last_kernel()


def oracle_case(planes, n_point, env):
    """The CPU oracle's frame for shade_case's inputs (mode-independent)."""
    from oracle import oracle as O

    pc = pass_constants(n_point, False)
    ops = O.OraclePass(eye=tuple(pc.eye_pos_w), ambient=tuple(pc.ambient_light), fresnel_r0=tuple(pc.fresnel_r0),
                       opacity=pc.opacity, n_point=n_point, ambient_mode=pc.ambient_mode, use_f0_plane=True,
                       apply_ao=True)
    la = pc.light_array() if n_point else None
    if n_point == 8:
        h, w = planes.shape[1:]
        return O.shade_frame(list(planes), ops, la, env, env, coverage(w, h))
    return O.shade(list(planes), ops, la, env, n_threads=4)
