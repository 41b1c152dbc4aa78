"""The case table of tests/test_gpu_strength_range.py: light strengths and ambient colours over the float range.

The other GPU tests draw strengths from a few decades around 1. The kernels' rescaled and reordered forms (brdf_x2's
QUARTER form, brdf_faithful_x2's s * (att * N.L / 4), the faithful finish's hardware reciprocal) are exact, or inside
their bound, only while no intermediate is subnormal or overflows where the reference's does not, and host gates
(pbr_context.hip, pbr_set_pass) keep the passes outside those ranges on the exact uniform loop. The frames here sweep
the scale 2^k of every strength (and of the constant ambient colour) across those gates, with lights 0.3 units in
front of and behind chosen pixels, so that s * att overflows at the high end, where the reference's back-faced term
(X * inf) * 0 is NaN, and is subnormal at the low end. tests/test_strength_range_cases.py checks on the CPU oracle
alone that the table holds what it is meant to hold.
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((256, 8), (70, 3))  # sixteen full waves (64 x 2 pixels each) | a ragged frame, two tiles across
# Scales 2^k: subnormal strengths; both sides of the faithful sum window (2^-100, 2^100); both sides of the lower
# edges of the host gates (2^-34, 2^-25) and of their upper edge (2^50); s * att overflowing at 0.3 units and at one.
K = (-140, -126, -115, -101, -99, -64, -30, 0, 30, 50, 51, 99, 101, 113, 120, 127)
AMBIENT_K = tuple(sorted(K + (-100, 60, 61, 126)))  # ... and the edges of reinhard's division window
N_POINT = 24
N_NEAR = 6          # lights 0-2: 0.3 in front of a chosen pixel; lights 3-5: 0.3 behind one
NEAR_DIST = 0.3
MIXED = (2, 12, 4)  # the mixed pass: directional, point (the first 12 of the 24: the near lights among them), spot
SLAB = (4.4, 5.6)   # the z range of every point and spot light (see frame())

# The host gates of pbr_set_pass restated (physically_based_renderer_amd/csrc/pbr_context.hip, the named constants):
QUARTER_STRENGTH_LO = 2.0 ** -34   # kQuarterStrengthLo: the exact balanced items, |s| == 0 or >= this ...
QUARTER_STRENGTH_HI = 2.0 ** 50    # kQuarterStrengthHi: ... and <= this
FAITHFUL_STRENGTH_LO = 2.0 ** -25  # kFaithfulStrengthLo: PBR_FLAG_FAITHFUL, every strength component 0 or >= this ...
FAITHFUL_STRENGTH_HI = 2.0 ** 50   # kFaithfulStrengthHi: ... and <= this
FAITHFUL_AMBIENT_HI = 2.0 ** 100   # kFaithfulAmbientHi: ... and every constant ambient component <= this


def in_gate(values, lo, hi):
    """Every value is 0 or has a magnitude in [lo, hi]."""
    a = np.abs(np.asarray(values, np.float64))
    return bool(np.all((a == 0.0) | ((a >= lo) & (a <= hi))))


def near_pixels(w, h):
    """[(y, x)] * 6: the pixels of the three front and the three back near lights, in different waves (a wave is 64
    columns x 2 rows) and in both elements of a pixel pair (even and odd x)."""
    if (w, h) == (256, 8):
        return [(0, 10), (3, 101), (6, 200), (1, 75), (4, 130), (7, 255)]
    if (w, h) == (70, 3):
        return [(0, 4), (1, 37), (2, 68), (0, 51), (1, 12), (2, 69)]
    raise ValueError((w, h))


def frame(w, h, seed=4243):
    """planes (15, h, w) float32: positions uniform in [-10, 10]^2 x [0, 10], unit normals, albedo in [0.05, 1],
    roughness in [0.2, 1] (bounds the specular factor), metallic 0 for a quarter of the pixels, 1 for a quarter,
    uniform for the rest, AO 1.

    Five pixels in twelve face up (within ~7 degrees of +z), five in twelve face down, a sixth take normals uniform on
    the sphere, and every point light lies in the slab SLAB of z: an upward pixel above the slab and a downward one
    below it see no light, so that a good share of every frame is unlit (check 4 of the CPU test) although six of the
    lights sit inside the cloud of pixels. The near pixels are moved into the slab.

    The seed keeps the exact mode's one documented residue out of the table (pow5_light's correctly
    rounded x^5 where glibc's powf is 1 ulp off; whether that ulp reaches the output depends on the roundings after
    it, hence on k): with 4242 one channel of the mixed 256 x 8 frame differed by 1 ulp at k = -126 and nowhere else,
    on the GPU and from the CPU oracle alike once its powf(x, 5) was replaced by the fp64 products; with this seed that
    oracle variant equals the oracle at every k, light set and ambient of the table."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    n = w * h
    p = np.zeros((15, h, w), np.float32)
    p[0:2] = rng.uniform(-10.0, 10.0, (2, h, w))
    p[2] = rng.uniform(0.0, 10.0, (h, w))
    kind = rng.integers(0, 12, n)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cone = nrm.copy()
    cone[:, 2] = np.abs(cone[:, 2]) + 8.0  # the cone around +z
    cone /= np.linalg.norm(cone, axis=1, keepdims=True)
    nrm = np.where((kind < 5)[:, None], cone, nrm)
    nrm = np.where(((kind >= 5) & (kind < 10))[:, None], cone * np.array([1.0, 1.0, -1.0]), nrm)
    p[3:6] = nrm.T.reshape(3, h, w)
    p[6:9] = rng.uniform(0.05, 1.0, (3, h, w))
    q = rng.integers(0, 4, (h, w))
    p[9] = np.where(q == 0, 0.0, np.where(q == 1, 1.0, rng.uniform(0.0, 1.0, (h, w))))
    p[10] = rng.uniform(0.2, 1.0, (h, w))
    p[11] = 1.0
    for y, x in near_pixels(w, h):
        p[2, y, x] = rng.uniform(4.8, 5.2)
    return p


def pow2(k):
    """2^k as a float32 (k >= -149), formed from two normal powers so that no libm pow sees a subnormal."""
    return np.float32(2.0 ** (k // 2)) * np.float32(2.0 ** (k - k // 2))


def mantissa(i, c):
    """1 + j / 16: m * 2^k is exact for every k >= -145, subnormal values included."""
    return 1.0 + ((5 * i + 3 * c) % 16) / 16.0


def point_lights(planes, k, negative):
    """(24, 12) float32 point lights with strengths mantissa * 2^k. Lights 0-2 sit NEAR_DIST along +N from the first
    three near pixels, lights 3-5 along -N from the other three; the rest are random in [-10, 10]^2 x SLAB. Light 7 has a
    zero channel; with `negative` (exact-mode passes only: a negative strength turns PBR_FLAG_FAITHFUL off) light 9 has
    a negative one."""
    h, w = planes.shape[1:]
    rng = np.random.default_rng(977 + w)
    arr = np.zeros((N_POINT, 12), np.float32)
    arr[:, 3] = 64.0
    arr[:, 4:7] = (0.0, -1.0, 0.0)
    arr[:, 8] = rng.uniform(-10.0, 10.0, N_POINT)
    arr[:, 9] = rng.uniform(-10.0, 10.0, N_POINT)
    arr[:, 10] = rng.uniform(SLAB[0], SLAB[1], N_POINT)
    for j, (y, x) in enumerate(near_pixels(w, h)):
        side = np.float32(NEAR_DIST if j < 3 else -NEAR_DIST)
        arr[j, 8:11] = planes[0:3, y, x] + side * planes[3:6, y, x]
    scale = pow2(k)
    for i in range(N_POINT):
        for c in range(3):
            arr[i, c] = np.float32(mantissa(i, c)) * scale
    arr[7, 1] = 0.0
    if negative:
        arr[9, 2] = -arr[9, 2]
    return arr


def mixed_lights(planes, k, negative):
    """(18, 12): two directional lights (from above, so that downward pixels keep to the point and spot lights), the
    first twelve point lights, four spot lights in the slab aimed along +-x / +-y with the power 64 whose cone
    underflows off axis."""
    nd, npt, ns = MIXED
    pts = point_lights(planes, k, negative)
    arr = np.zeros((nd + npt + ns, 12), np.float32)
    arr[:, 3] = 64.0
    arr[nd:nd + npt] = pts[:npt]
    arr[0, 4:7] = (-0.6, 0.0, -0.8)   # L = -Direction
    arr[1, 4:7] = (0.28, -0.0, -0.96)
    dirs = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -0.6, 0.8))
    spots = ((-14.0, 1.0, 5.0), (13.0, -2.0, 4.7), (0.5, -15.0, 5.3), (-3.0, 12.0, 4.5))
    for j in range(ns):
        arr[nd + npt + j, 4:7] = dirs[j]
        arr[nd + npt + j, 8:11] = spots[j]
    for i in list(range(nd)) + list(range(nd + npt, nd + npt + ns)):
        arr[i, 0:3] = pts[12 + (i % 12), 0:3]  # strengths of the point lights the mixed pass leaves out
    return arr


def lit_mask(planes, lights, n_dir=0):
    """(h, w) bool: some light reaches the pixel (N.L > 0 and, for point and spot lights, within the range of 100)."""
    P = planes[0:3].astype(np.float64)
    Nn = planes[3:6].astype(np.float64)
    lit = np.zeros(planes.shape[1:], bool)
    for i, L in enumerate(lights.astype(np.float64)):
        if i < n_dir:
            lit |= np.einsum("chw,c->hw", Nn, -L[4:7]) > 0.0
        else:
            l = L[8:11][:, None, None] - P
            lit |= ((Nn * l).sum(0) > 0.0) & ((l * l).sum(0) <= 1.0e4)
    return lit


def near_radiance(planes, lights):
    """(6, h, w) float32: s.x * att of the near lights as the reference forms it in float32 (att = 1 / max(d, 0.01)^2),
    0 beyond the range."""
    out = []
    for L in lights[:N_NEAR]:
        l = L[8:11][:, None, None].astype(np.float32) - planes[0:3]
        d = np.sqrt((l * l).sum(0, dtype=np.float32)).astype(np.float32)
        dm = np.maximum(d, np.float32(0.01))
        att = (np.float32(1.0) / (dm * dm)).astype(np.float32)
        out.append(np.where(d > 100.0, np.float32(0.0), (L[0] * att).astype(np.float32)))
    return np.stack(out)


# name: (context key, pass flags added, light set, expected kernel at k = 0 by mode, has a faithful loop).
# Context keys (contexts() of the GPU test): bal PBR_BALANCED_MIN=1 | uniform PBR_BALANCED_MIN=0 PBR_LEAN=0 |
# lean PBR_BALANCED_MIN=0 | px1 PBR_PIXELS_PER_THREAD=1 (bounds_cases.LAYOUTS).
def families():
    from physically_based_renderer_amd import _native as N

    cull = N.PBR_FLAG_TILED_CULLING
    return {
        "balanced": ("bal", 0, "points", {"exact": ("shade_tile_kernel", ", 2>"), "faithful": ("shade_tile_kernel", ", 1>")}, True),
        "uniform": ("uniform", 0, "points", {"exact": ("shade_tile_kernel", ", 0>"), "faithful": ("shade_tile_kernel", ", 0>")}, True),
        "lean": ("lean", 0, "points", {"exact": ("shade_lean_kernel", ", false>"), "faithful": ("shade_lean_kernel", ", true>")}, True),
        "culled_lean": ("lean", cull, "points", {"exact": ("shade_lean_kernel", "true, false>"), "faithful": ("shade_lean_kernel", "true, true>")}, True),
        "culled_uniform": ("uniform", cull, "points", {"exact": ("shade_tile_kernel", "true, 0>"), "faithful": ("shade_tile_kernel", "true, 0>")}, True),
        # the one-pixel kernel has no faithful loop: PBR_FLAG_FAITHFUL leaves its frames exact
        "px1": ("px1", 0, "points", {"exact": ("shade_tile1_kernel", "<0, false, false, false>"), "faithful": ("shade_tile1_kernel", "<0, false, false, false>")}, False),
        "mixed": ("lean", 0, "mixed", {"exact": ("shade_lean_kernel", ", false>"), "faithful": ("shade_lean_kernel", ", true>")}, True),
    }


CONTEXT_ENV = {
    "bal": {"PBR_BALANCED_MIN": "1"},
    "uniform": {"PBR_BALANCED_MIN": "0", "PBR_LEAN": "0"},
    "lean": {"PBR_BALANCED_MIN": "0"},
    "px1": {"PBR_BALANCED_MIN": "0", "PBR_PIXELS_PER_THREAD": "1"},
}


def light_set(planes, which, k, negative):
    """(lights (n, 12), (n_dir, n_point, n_spot))."""
    if which == "points":
        return point_lights(planes, k, negative), (0, N_POINT, 0)
    return mixed_lights(planes, k, negative), MIXED


def pass_constants(lights, counts, flags, ambient=(0.0, 0.0, 0.0)):
    """The sweep's passes use ambient (0, 0, 0): the default 0.03 would swamp every tiny sum."""
    from physically_based_renderer_amd.renderer import PassConstants

    nd, npt, ns = counts
    return PassConstants(ambient_light=tuple(float(a) for a in ambient), num_dir_lights=nd, num_point_lights=npt,
                         num_spot_lights=ns, flags=flags, lights_array=lights if nd + npt + ns else None)


def oracle_frame(planes, lights, counts, ambient=(0.0, 0.0, 0.0), ref=False):
    """The CPU oracle's frame (mode-independent); `ref`: the reference's own shader (oracle/_ref) instead."""
    from oracle import oracle as O

    nd, npt, ns = counts
    ops = O.OraclePass(ambient=tuple(float(a) for a in ambient), n_dir=nd, n_point=npt, n_spot=ns)
    la = lights if nd + npt + ns else None
    return O.shade_ref(list(planes), ops, la, None) if ref else O.shade(list(planes), ops, la, None, n_threads=4)


def ambient_colour(k):
    s = pow2(k)
    return tuple(np.float32(m) * s for m in (1.0, 1.25, 1.5))


def ambient_table():
    """[(name, size, planes, ambient colour, k or None)]: the constant ambient (1, 1.25, 1.5) * 2^k over AMBIENT_K in
    both frames, and the 256 x 8 frame with albedo 2^100 in rows 4-5 and 2^127 in rows 6-7 under the default 0.03 (the
    ambient term reaches 2^126 through the albedo alone)."""
    rows = []
    for w, h in SIZES:
        p = frame(w, h)
        for k in AMBIENT_K:
            rows.append((f"ambient2^{k}", (w, h), p, ambient_colour(k), k))
    w, h = SIZES[0]
    p = frame(w, h).copy()
    p[6:9, 4:6] = np.float32(2.0 ** 100)
    p[6:9, 6:8] = np.float32(2.0 ** 127)
    rows.append(("albedo2^100,2^127", (w, h), p, (np.float32(0.03),) * 3, None))
    return rows
