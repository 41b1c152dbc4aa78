"""The diffuse-IBL ambient's rare and special normals on the GPU (csrc/shade_pixel.h ambient_ibl_pair).

WorldToSkyUV's pair forms run a main path for ordinary normals; a zero component, an exponent-gap shortcut, a
quotient at or above 2^25 and |N.y| == 1 are patched inside a wave-uniform branch; NaN, out-of-window components and
|N.y| > 1 take the scalar functions; waves without a special element use a branch-free texel wrap.
tests/ibl_path_cases.py puts every such case into the first element of a pixel pair, the second, and both, beside an
ordinary partner, in frames of one to four wave tiles (64x2, 64x8, and the ragged 70x3), and this test shades them

  * with 24 point lights (both modes' wave-balanced tile kernels), 8 (the frame path with a coverage plane and the
    sky pass: the pair kernel's uniform loops, and pairs with an element that is not shaded geometry) and 0 (the
    lean kernel), diffuse-IBL ambient throughout;
  * with the Chelsea 360x180 env map and with 1x1, 2x1 and 3x2 maps of all-distinct texels, where a wrong wrap
    changes the value.

Exact mode must be bit-identical to the CPU oracle, NaN where it has NaN; faithful mode within the north-star 1e-5
with the same NaN pattern, and the pass statistics must account for every pixel and light term. The oracle's frames
are computed once per module; test_oracle_case_table checks on the CPU alone that every case gives the finite or NaN
value its kind implies.
"""
import numpy as np
import pytest

import ibl_path_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5  # north_star


@pytest.fixture(scope="module")
def frames():
    return C.frames()


@pytest.fixture(scope="module")
def envs():
    return C.env_maps()


@pytest.fixture(scope="module")
def oracle_frames(frames, envs):
    """{(frame label, light count, env name): the oracle's frame}, computed once."""
    return {(label, n, name): C.oracle_case(p, n, env)
            for label, p, _ in frames for n in C.LIGHT_COUNTS for name, env in envs.items()}


def expect_nan(name):
    """Whether the case `name` (ibl_path_cases.case_table) gives NaN: a NaN component, or |N.y| > 1 (asinf's
    (x - x) / (x - x)); 1 + 1 ulp is above 1."""
    return name.startswith(("nan", "ny>1", "ny<-1")) or name in ("ny=1+1ulp", "ny=-1+1ulp")


def test_oracle_case_table(frames, envs, oracle_frames):
    """CPU only: every case pixel of the oracle's frames is finite, or NaN exactly where its kind says so, and
    its ordinary partner is finite. Also: the frames together hold every (case, placement) at every size."""
    want = {f"{n}/{w}" for n, w, _, _ in C.placements()}
    for w, h in C.SIZES:
        seen = {v for label, _, names in frames if label.startswith(f"{w}x{h}#") for v in names.ravel()}
        assert seen == want, (w, h)
    for label, p, names in frames:
        for name in envs:
            ref = oracle_frames[(label, 0, name)]
            for (y, i), tag in np.ndenumerate(names):
                case, where = tag.rsplit("/", 1)
                for e in (0, 1):
                    is_case = where == "both" or (where == "first") == (e == 0)
                    nan = np.isnan(ref[y, 2 * i + e, :3]).any()
                    assert nan == (is_case and expect_nan(case)), (label, name, tag, e, ref[y, 2 * i + e])


@pytest.mark.parametrize("n_point", C.LIGHT_COUNTS)
@pytest.mark.parametrize("mode", ["exact", "faithful"])
def test_ibl_paths_equal_the_oracle(n_point, mode, frames, envs, oracle_frames, shading_ctx, gpu):
    want_kernel = {24: "shade_tile_kernel", 8: "shade_tile_kernel", 0: "shade_lean_kernel"}[n_point]
    for label, p, names in frames:
        h, w = p.shape[1:]
        for name, env in envs.items():
            got, st, kernel = C.shade_case(shading_ctx, gpu, p, n_point, mode == "faithful", env)
            ref = oracle_frames[(label, n_point, name)]
            e = O.rel_err(got, ref)
            print(f"{label} {n_point} lights env {name} {mode}: max_rel={e.max():.3g} "
                  f"bit_exact={O.bit_equal(got, ref).mean():.6f} exact_pixels={st['exact_pixels']} kernel={kernel}")
            assert want_kernel in kernel, kernel
            if n_point == 24:
                assert kernel.endswith((", 1>", ", 2>")), kernel  # a wave-balanced variant (BAL != 0)
            elif n_point == 8:
                assert kernel.endswith(", 0>"), kernel            # the pair kernel's uniform loops
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            if mode == "exact":
                bad = np.argwhere(~O.bit_equal(got, ref).all(axis=-1))
                assert bad.size == 0, [(int(y), int(x), names[y, x // 2]) for y, x in bad[:8]]
            else:
                assert e.max() <= REL_TOL
            geo = int(C.coverage(w, h).sum()) if n_point == 8 else w * h
            assert st["geometry_pixels"] == geo
            if n_point == 24:  # balanced lists: only the terms that pass the backface and range tests
                assert 0 < st["light_terms"] <= n_point * geo
            else:
                assert st["light_terms"] == n_point * geo
