"""The numpy restatement of the anisotropic resolve (tests/resolve_aniso_reference.py) against the rule of DESIGN.md
§11, "Anisotropic filter". No device."""
import numpy as np
import pytest

import resolve_aniso_reference as RA
import resolve_cases as C
import resolve_mip_cases as MC
import resolve_mip_reference as RM
import resolve_reference as R
from oracle import oracle as O
from physically_based_renderer_amd.renderer import Material

F = np.float32


def same(got, want):
    return all(O.bit_equal(g, w).all() if g.dtype != np.uint8 else np.array_equal(g, w) for g, w in zip(got, want))


def ramp_footprints(h, w, du, dv):
    attrs = MC.ramp_attributes(h, w, du, dv)
    return attrs, RM.footprints(attrs[12], attrs[13], np.zeros((h, w), np.uint16))


@pytest.mark.parametrize("major", ["x", "y"])
def test_tap_count_at_integer_ratios_is_the_ratio(major):
    """A 64 x 64 map under k texels per pixel along one axis and 1 along the other: N = k for every k in 1 .. 16."""
    for k in range(1, 17):
        long, short = k / 64.0, 1.0 / 64.0
        _, d = ramp_footprints(4, 6, long if major == "x" else short, short if major == "x" else long)
        pmax2, pmin2, du, dv = RA.footprint_axes(*d, 64, 64)
        assert (pmax2 == F(k * k)).all() and (pmin2 == 1).all()
        assert (RA.tap_count(pmax2, pmin2, 16) == k).all(), k
        if k > 1:  # the step of the major axis, in UV units
            assert (du == (F(long) if major == "x" else 0)).all() and (dv == (0 if major == "x" else F(long))).all()


def test_tap_count_one_ulp_above_a_square_is_the_next_and_the_cap_holds():
    one = np.ones(1, F)
    for k in range(1, 16):
        above = np.nextafter(F(k * k), F(np.inf)) * one
        assert RA.tap_count(above, one, 16)[0] == k + 1
        assert RA.tap_count(F(k * k) * one, one, 16)[0] == k
    for m in range(1, 17):
        assert RA.tap_count(F(1.0e6) * one, one, m)[0] == m               # the cap
        assert RA.tap_count(F(9.0) * one, one, m)[0] == min(m, 3)
        assert RA.tap_count(F(np.nan) * one, one, m)[0] == 1              # NaN: every comparison is false
        assert RA.tap_count(one, F(np.nan) * one, m)[0] == 1
        assert RA.tap_count(one, 0 * one, m)[0] == m                      # a zero minor axis under a non-zero major one
        assert RA.tap_count(0 * one, 0 * one, m)[0] == 1                  # both zero
        assert RA.tap_count(F(np.inf) * one, F(np.inf) * one, m)[0] == 1  # inf > inf is false


def test_y_major_needs_a_strictly_longer_y_axis_and_nan_is_x_major():
    z = np.zeros(3, F)
    dudx = np.array([2.0, 2.0, np.nan], F) / F(64)
    dvdy = np.array([2.0, 3.0, 5.0], F) / F(64)
    pmax2, pmin2, du, dv = RA.footprint_axes(dudx, z, z, dvdy, 64, 64)
    assert pmax2[0] == 4 and pmin2[0] == 4 and du[0] == dudx[0] and dv[0] == 0   # a tie: x
    assert pmax2[1] == 9 and pmin2[1] == 4 and du[1] == 0 and dv[1] == dvdy[1]   # y
    assert np.isnan(pmax2[2]) and pmin2[2] == 25 and np.isnan(du[2]) and dv[2] == 0  # ry > NaN is false: x
    assert RA.tap_count(pmax2, pmin2, 16).tolist() == [1, 2, 1]


def test_level_of_the_8_to_1_ramp_falls_by_one_per_doubling_of_the_taps():
    """64 x 64 texels, 8 per pixel along x and 1 along y: M = 8, 4, 2, 1 land exactly on levels 0, 1, 2, 3, f = 0."""
    _, d = ramp_footprints(4, 6, 8.0 / 64, 1.0 / 64)
    for m, level in ((8, 0), (4, 1), (2, 2), (1, 3), (16, 0)):
        n, l0, l1, f, lod = RA.lod(*d, 64, 64, 7, 0.0, m)
        assert (n == min(m, 8)).all() and (lod == level).all() and (l0 == level).all() and (f == 0).all(), m
    n, l0, l1, f, lod = RA.lod(*d, 64, 64, 7, 1.5, 4)   # the bias adds after the division
    assert (lod == 2.5).all() and (l0 == 2).all() and (l1 == 3).all() and (f == 0.5).all()
    n, l0, l1, f, lod = RA.lod(*d, 16, 32, 6, 0.0, 8)   # per texture: 2 texels along x, 0.5 along y: N = 4, r2 = 0.25
    assert (n == 4).all() and (lod == 0).all()


def test_level_from_r2_is_the_trilinear_rules():
    rng = np.random.default_rng(5)
    dudx = (rng.uniform(0, 4, 4000) ** 3).astype(F) / F(64)
    dudx[:4] = [0.0, np.inf, np.nan, 1.0 / 64]
    z = np.zeros_like(dudx)
    with np.errstate(all="ignore"):
        ax = dudx * F(64)
        r2 = ax * ax + z * z
    for bias in (0.0, -0.75, 1.5, 40.0):
        for a, b in zip(RA.lod_from_r2(r2, 7, bias), RM.lod(dudx, z, z, z, 64, 64, 7, bias)):
            assert O.bit_equal(a, b).all()
        n, *rest = RA.lod(dudx, z, z, z, 64, 64, 7, bias, 1)
        assert (n == 1).all()
        for a, b in zip(rest, RM.lod(dudx, z, z, z, 64, 64, 7, bias)):
            assert O.bit_equal(a, b).all()


def test_tap_offsets_are_antisymmetric_centred_and_exact_for_powers_of_two():
    for n in range(1, 17):
        t = RA.tap_offsets(n)
        assert t.dtype == F and t.shape == (n,)
        assert (t == -t[::-1]).all() and (np.diff(t) > 0).all()
        assert abs(float(t[-1]) - float(t[0]) - (n - 1) / n) < 1e-6   # spans (N - 1) / N of the axis
        if n & (n - 1) == 0:
            assert (t.astype(np.float64) * (2 * n) == 2 * np.arange(n) + 1 - n).all()
    assert RA.tap_offsets(1).tolist() == [0.0]
    assert RA.tap_offsets(8).tolist() == [-0.4375, -0.3125, -0.1875, -0.0625, 0.0625, 0.1875, 0.3125, 0.4375]


@pytest.fixture(scope="module")
def table():
    return MC.table()


@pytest.fixture(scope="module")
def chains(table):
    return [RM.build_mips(t) for t in table[1]]


@pytest.mark.parametrize("bias", [0.0, 1.5])
def test_max_anisotropy_1_is_the_trilinear_resolve(table, chains, bias):
    """The special UVs (NaN, +-inf, 3e9, texel edges) with valid partners through every material: bit for bit."""
    mats, texs = table
    attrs, ids = MC.special_attributes(12, 70, len(mats), seed=70)
    want = RM.resolve_mip(attrs, ids, mats, texs, bias, chains=chains)
    assert same(RA.resolve_aniso(attrs, ids, mats, texs, 1, bias, chains=chains), want)
    # and with any M on ids that alternate pixel by pixel: every footprint is +0, N = 1 at every pixel
    ids = C.checker_ids(12, 70, len(mats))
    want = RM.resolve_mip(attrs, ids, mats, texs, bias, chains=chains)
    assert same(RA.resolve_aniso(attrs, ids, mats, texs, 16, bias, chains=chains), want)
    if bias == 0.0:
        assert same(want, R.resolve(attrs, ids, mats, texs, R.LINEAR))


def test_a_pixel_with_one_tap_is_the_trilinear_pixel_and_the_count_is_per_texture(table, chains):
    """Material 7 (every map another size) under 4 : 1 texels of the 64 x 64 map: the square maps take 4 taps, the
    16 x 32 specular map (1 : 0.5 texels) 2, the 256 x 1 normal map (16 : 1/64) 8 = M (u0 and the steps are exact in
    fp32). The same frame with equal steps in texels of the square maps: one tap there, and those planes are the
    trilinear ones."""
    mats, texs = table
    h, w = 6, 8
    ids = np.full((h, w), 7, np.uint16)
    attrs = MC.ramp_attributes(h, w, 4.0 / 64, 1.0 / 64, u0=0.125)
    d = RM.footprints(attrs[12], attrs[13], ids)
    count = lambda t: RA.lod(*d, texs[t].shape[1], texs[t].shape[0], len(chains[t]), 0.0, 8)[0]
    assert (count(5) == 4).all() and (count(8) == 4).all() and (count(7) == 2).all() and (count(3) == 8).all()
    attrs = MC.ramp_attributes(h, w, 3.0 / 64, 3.0 / 64, u0=0.125)
    d = RM.footprints(attrs[12], attrs[13], ids)
    assert (count(5) == 1).all() and (count(7) == 2).all()
    got = RA.resolve_aniso(attrs, ids, mats, texs, 8, 0.25, chains=chains)
    want = RM.resolve_mip(attrs, ids, mats, texs, 0.25, chains=chains)
    assert O.bit_equal(got[0][6:10], want[0][6:10]).all()           # albedo (64 x 64), metallic (128 x 128): N = 1
    assert not O.bit_equal(got[0][12:15], want[0][12:15]).all()     # F0 from the 16 x 32 map: N = 2


def bilinear_scalar(tex, u, v):
    """The level-0 linear-wrap bilinear of one (u, v), written out with float32 scalars."""
    h, w = tex.shape[0], tex.shape[1]
    x, y = F(F(u) * F(w)) - F(0.5), F(F(v) * F(h)) - F(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = F(x - x0f), F(y - y0f)
    x0, y0 = int(x0f) % w, int(y0f) % h
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    out = []
    for c in range(tex.shape[2]):
        t = lambda yy, xx: F(F(tex[yy, xx, c]) / F(255.0))
        top = F(t(y0, x0) + F(fx * F(t(y0, x1) - t(y0, x0))))
        bottom = F(t(y1, x0) + F(fx * F(t(y1, x1) - t(y1, x0))))
        out.append(F(top + F(fy * F(bottom - top))))
    return out


def test_8_to_1_ramp_at_8_taps_is_the_mean_of_eight_level_0_bilinears():
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    mats = [Material(flags=C.D, tex=(0, -1, -1, -1, -1, -1))]
    h, w = 8, 16
    attrs = MC.ramp_attributes(h, w, 8.0 / 64, 1.0 / 64, u0=0.03125, v0=0.25)
    ids = np.zeros((h, w), np.uint16)
    got = RA.resolve_aniso(attrs, ids, mats, [tex], 8, 0.0)[0][6:9]
    want = np.empty((3, h, w), F)
    for y in range(h):
        for x in range(w):
            u, v = attrs[12, y, x], attrs[13, y, x]
            s = None
            for i in range(8):
                t = F(F(2 * i + 1 - 8) / F(16))
                b = bilinear_scalar(tex, F(u + F(t * F(0.125))), F(v + F(t * F(0.0))))
                s = b if s is None else [F(s[c] + b[c]) for c in range(3)]
            want[:, y, x] = [F(s[c] / F(8)) for c in range(3)]
    assert O.bit_equal(got, want).all()
    trilinear = RM.resolve_mip(attrs, ids, mats, [tex], 0.0)[0][6:9]   # level 3 alone
    differ = ~O.bit_equal(got, trilinear)
    print(f"8:1 ramp: {differ.sum()} of {differ.size} albedo values differ from the trilinear result")
    assert differ.any()
