"""Host checks (no GPU) of the inputs of tests/test_gpu_frontend_shapes.py and tests/test_gpu_raster_scale.py: every
case reaches the code it is named for -- list lengths, box sizes, block counts, prefix ties, magnitudes, computed from
tests/raster_reference.py's vertex stage and the box of DESIGN.md §12 -- the restatements obey §11's and §12's rules at
the new shapes, and the odd-width and band cases can tell a kernel that invents a quad partner from one that does not."""
import numpy as np
import pytest

import frontend_shape_cases as FS
import raster_cases as C
import raster_clip_reference as CR
import raster_reference as R
import raster_scale_cases as SC
import resolve_aniso_reference as RA
import resolve_mip_cases as MC
import resolve_mip_reference as RM
from oracle import oracle as O

F = np.float32


@pytest.fixture(scope="module")
def table():
    return MC.table()


@pytest.fixture(scope="module")
def chains(table):
    return [RM.build_mips(t) for t in table[1]]


# ---- B: the scale cases reach what they name ------------------------------------------------------------------------

def test_many_large_lists_more_than_the_striding_workgroups():
    m, d, v = SC.many_large()
    plain = SC.listed(SC.boxes(m, d, v))
    assert len(plain) == SC.N_SLIVERS >= SC.LARGE_GRID_X + 1 and all(b[4] * b[5] > SC.SMALL_PIXELS for b in plain)
    for n in (SC.LARGE_GRID_X, SC.LARGE_GRID_X + 1):  # the cut scenes list exactly 1,024 and 1,025
        assert len(SC.listed(SC.boxes(m, SC.cut_to(d, n), v))) == n
    m, d, v = SC.many_large(clip=True)
    clipped = SC.listed(SC.boxes(m, d, v, clip=True))
    second = [b for b in clipped if b[1] == 1]
    assert len(clipped) >= SC.LARGE_GRID_X + 1 and len(second) >= 50, (len(clipped), len(second))
    assert any(i >= SC.LARGE_GRID_X for i, b in enumerate(clipped) if b[1] == 1)  # a second piece on the second trip
    stats, clip = CR.rasterize(m, d, v)[3:5]
    assert clip["clipped_near"] == SC.N_SLIVERS // 10 and clip["clip_pieces"] == 2 * clip["clipped_near"]
    assert stats["skipped_near"] == stats["skipped_guard_band"] == 0


def test_many_large_fragments_are_the_sum_over_bands():
    m, d, v = SC.many_large()
    full = R.rasterize(m, d, v)
    bands = [R.rasterize(m, d, v.rows(r0, r1)) for r0, r1 in FS.UNEVEN_BANDS]
    assert full[3]["fragments"] == sum(b[3]["fragments"] for b in bands) > 100000
    assert O.bit_equal(np.concatenate([b[0] for b in bands], 1), full[0]).all()


def test_tri_counts_straddle_the_setup_workgroup():
    for n in (255, 256, 257):
        m, d, v = SC.tri_counts(n)
        assert R.rasterize(m, d, v)[3]["triangles"] == n
    assert all(b[4] * b[5] <= SC.SMALL_PIXELS for b in SC.boxes(*SC.tri_counts(257)))


def test_box_threshold_boxes_have_exactly_the_listed_sizes():
    m, d, v = SC.box_threshold()
    full = SC.boxes(m, d, v)
    assert [b[2:] for b in full] == [tuple(b) for b in SC.BOXES] and [b[0] for b in full] == list(range(len(SC.BOXES)))
    sizes = [b[4] * b[5] for b in full]
    assert sizes == [64, 64, 64, 64, 65, 65, 65, 66, 64]  # 33x2 is the smallest two-row box above 64
    x, _, bw, _ = SC.BOXES[8]
    assert x + SC.UNCUT_WIDTH[8] > v.width and x + bw == v.width  # cut from 160 pixels to 64 by the right frame edge
    for r0, r1 in SC.BOX_BANDS:  # a band's box is the full frame's cut to the band's rows
        want = [(b[0], 0, b[2], max(b[3], r0), b[4], min(b[3] + b[5], r1) - max(b[3], r0)) for b in full
                if max(b[3], r0) < min(b[3] + b[5], r1)]
        assert SC.boxes(m, d, v.rows(r0, r1)) == want, (r0, r1)
    for t, (r0, r1) in SC.LARGE_TO_SMALL:  # large in the full frame, small and not empty in its band
        in_band = [b for b in SC.boxes(m, d, v.rows(r0, r1)) if b[0] == t]
        assert sizes[t] > SC.SMALL_PIXELS and len(in_band) == 1 and 0 < in_band[0][4] * in_band[0][5] <= SC.SMALL_PIXELS
    assert (r0, r1) in SC.BOX_BANDS


def test_offset_blocks_has_more_blocks_than_slabs_off_the_grid():
    m, d, v = SC.offset_blocks()
    big, small = SC.boxes(m, d, v)
    nbx, nby = SC.blocks(big)
    assert (nbx, nby) == (3, 17) and nbx * nby > SC.LARGE_SLABS and nbx > 1
    assert big[2] % SC.BLOCK_W != 0 and big[3] % SC.BLOCK_H != 0  # the box's origin is off the 64x4 grid
    assert small[4] * small[5] > SC.SMALL_PIXELS and SC.blocks(small)[0] > 1
    for r0, r1 in SC.OFFSET_BANDS:
        b = SC.boxes(m, d, v.rows(r0, r1))[0]
        assert SC.blocks(b)[0] == 3 and b[3] == max(r0, 5)


def test_many_draws_prefix_has_ties_first_last_and_in_runs_of_two():
    m, d, v = SC.many_draws()
    p = SC.tri_prefix(d)
    assert len(d) == SC.N_DRAWS and p[0] == p[1] and p[-1] == p[-2] and p[-1] == R.rasterize(m, d, v)[3]["triangles"]
    runs = [k for k in range(len(p) - 2) if p[k] == p[k + 1] == p[k + 2]]
    assert len(runs) >= 40 and any(0 < p[k] < p[-1] for k in runs)
    assert {dr.index_count for dr in d} == {0, 3, 6} and {dr.cull for dr in d} == {0, 1}
    assert len({dr.first_index for dr in d}) > 3 and len({dr.material for dr in d}) == 11
    ids = R.rasterize(m, d, v)[1]
    assert len(set(np.unique(ids).tolist()) - {R.NONE}) >= 8  # many draws are visible, not one
    empty = SC.many_draws(all_empty=True)
    planes, ids, depth, stats = R.rasterize(*empty)
    assert SC.tri_prefix(empty[1]).max() == 0 and stats == dict.fromkeys(R.STAT_NAMES, 0)
    assert (ids == R.NONE).all() and (depth == 1).all()
    background = R.rasterize(empty[0], [], empty[2])
    assert O.bit_equal(planes, background[0]).all()


def test_guard_scale_reaches_2_to_the_40_on_a_covered_pixel():
    m, d, v = SC.guard_scale()
    W, H = v.width, v.height
    planes, ids, depth, stats = R.rasterize(m, d, v)
    assert stats["skipped_guard_band"] == 1 and stats["skipped_near"] == stats["zero_area"] == 0
    assert 0.05 < (ids != R.NONE).mean() < 1.0  # part of the frame is covered, part is background
    vs = R.vertex_stage(m[0].vertices, d[0], v)
    assert np.flatnonzero(vs["guard"]).tolist() == [3 * SC.BEYOND + 1]  # the contrast triangle's vertex alone
    # 32,767.9 px: inside the band after the float32 round trip through ndc (an ulp there is 1 / 256 px), and drawn
    assert abs(int(np.abs(vs["X"]).max()) - round(32767.9 * 256)) <= 2 and int(np.abs(vs["X"]).max()) < 2 ** 23
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    largest = 0
    for t in range(3):
        X, Y = [int(vs["X"][3 * t + k]) for k in range(3)], [int(vs["Y"][3 * t + k]) for k in range(3)]
        A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        if A < 0:
            X[1], X[2], Y[1], Y[2], A = X[2], X[1], Y[2], Y[1], -A
        assert A >= 2 ** 44
        E = R._edge_values(R._edges(X, Y), x, y)
        covered = (E[0] > 0) & (E[1] > 0) & (E[2] > 0)
        assert 0 < covered.sum() < W * H, t  # each triangle covers part of the frame
        largest = max(largest, max(int(np.abs(e[covered]).max()) for e in E))
    assert largest >= 2 ** 40
    m, d, v = SC.guard_scale(clip=True)
    cstats, clip = CR.rasterize(m, d, v)[3:5]
    assert clip["clipped_near"] == 1 and cstats["fragments"] > 0


# ---- the rules at the new shapes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [(71, 37), (63, 5)], ids=FS.frame_id)
def test_closed_fan_and_split_quad_cover_every_pixel_once(frame):
    W, H = frame
    for name in ("fan", "split_quad"):
        m, d, v = C.case(name, W, H)
        y0, y1 = 2, H - 5
        if name == "split_quad" and H < 8:  # the case's own quad needs 8 rows: the same quad from the top row down
            y0, y1 = 0, H - 2
            m, d = C.one_draw([(3.5, 0.5, 1), (W - 6.5, 0.5, 1), (W - 6.5, H - 1.5, 1),
                               (3.5, 0.5, 1), (W - 6.5, H - 1.5, 1), (3.5, H - 1.5, 1)], W, H, 2)
        counts = np.zeros((H, W), np.int64)
        stats = R.rasterize(m, d, v, coverage_counts=counts)[3]
        assert counts.max() == 1 and stats["fragments"] == counts.sum() > 0, name
        ys, xs = np.nonzero(counts)
        if name == "split_quad":  # the union is the rectangle of pixel centres [3.5, W - 6.5) x [y0 + 0.5, y1 + 0.5)
            assert counts[y0:y1, 3:W - 7].all() and counts.sum() == (y1 - y0) * (W - 10)
        else:  # the union is the rim polygon: every row's covered pixels are one run, the centre pixel among them
            assert counts[H // 2, W // 2] == 1
            for r in np.unique(ys):
                run = xs[ys == r]
                assert run.max() - run.min() + 1 == run.size


@pytest.mark.parametrize("frame", FS.ODD_FRAMES, ids=FS.frame_id)
def test_last_column_of_an_odd_width_has_no_x_footprint(frame):
    W, H = frame
    attrs, ids = FS.ramp_case(H, W, 8, FS.ALL_FLAGS)
    dudx, dvdx, dudy, dvdy = RM.footprints(attrs[12], attrs[13], ids)
    for d in (dudx, dvdx):
        assert (d[:, W - 1].view(np.uint32) == 0).all()  # +0.0f, bits and all
    if W > 1:
        assert (dudx[:, :W - 1] == F(8.0 / 64.0)).all()
    if H % 2:
        assert (dvdy[H - 1].view(np.uint32) == 0).all()


def test_a_frame_of_one_column_has_level_lod_bias_everywhere(table, chains):
    """One column: no x partner anywhere; the ramps' 1 texel per pixel in y leaves r2 at 1, not above it."""
    for W, H in ((1, 1), (1, 9)):
        attrs, ids = FS.ramp_case(H, W, 8, 13)
        d = RM.footprints(attrs[12], attrs[13], ids)
        for bias in FS.BIASES:
            assert (RM.lod(*d, 64, 64, len(chains[2]), bias)[3] == F(bias)).all()
            n, _, _, _, lod = RA.lod(*d, 64, 64, len(chains[2]), bias, 16)  # a zero minor axis takes every tap
            assert (n[H - 1] == 1).all() and (n[:H - 1] == 16).all() and (lod == F(bias)).all()


# ---- A: the cases can fail ------------------------------------------------------------------------------------------

RAMPS = [(f, t, m) for f in FS.ODD_FRAMES for t in FS.RAMP_TEXELS for m in FS.RAMP_MATERIALS]


@pytest.mark.parametrize("frame,texels,material", RAMPS, ids=[f"{FS.frame_id(f)}-{t}-m{m}" for f, t, m in RAMPS])
def test_the_last_column_of_every_ramp_case_tells_an_invented_partner(table, chains, frame, texels, material):
    """Per ramp case, trilinear and anisotropic: the restatement's last column differs from its own column W - 2 or
    from the restatement on the frame widened by the padding column (the issue's condition); and it differs from the
    widened frame's in every case, so a kernel that read the padding column as a partner fails each of them."""
    W, H = frame
    attrs, ids = FS.ramp_case(H, W, texels, material)
    wide = FS.widened(attrs, ids)
    assert (wide[1][:, W] == material).all() and np.isfinite(wide[0][:, :, W]).all()
    if W > 1:  # the padding column continues the ramp
        assert O.bit_equal(wide[0][12, :, W], F(0.125) + F(W) * F(texels / 64.0)).all()
    for bias in FS.BIASES:
        want = RM.resolve_mip(attrs, ids, *table, bias, chains=chains)
        own, other = FS.last_column_tells(want, RM.resolve_mip(*wide, *table, bias, chains=chains))
        assert own or other, ("mip", bias)
        assert other, ("mip", bias)
    for m in FS.ANISOTROPIES:
        want = RA.resolve_aniso(attrs, ids, *table, m, 0.0, chains=chains)
        own, other = FS.last_column_tells(want, RA.resolve_aniso(*wide, *table, m, 0.0, chains=chains))
        assert own or other, ("aniso", m)
        assert other, ("aniso", m)


def test_the_last_row_of_a_band_that_ends_inside_the_frame_differs_from_the_frame(table, chains):
    W, H = FS.BIG
    for name, (attrs, ids) in FS.band_cases(H, W).items():
        full_mip = RM.resolve_mip(attrs, ids, *table, 0.0, chains=chains)
        full_aniso = RA.resolve_aniso(attrs, ids, *table, 8, 0.0, chains=chains)
        for r0, r1 in FS.INNER_BANDS:
            assert r0 % 2 == 0 and (r1 - r0) % 2 == 1 and r1 < H
            assert (ids[r1] == ids[r1 - 1]).all()  # the row below exists, with the same ids
            band = RM.resolve_mip(attrs[:, r0:r1], ids[r0:r1], *table, 0.0, chains=chains)
            assert O.bit_equal(band[0][:, :-1], full_mip[0][:, r0:r1 - 1]).all(), (name, r0, r1)
            assert not O.bit_equal(band[0][:, -1], full_mip[0][:, r1 - 1]).all(), (name, r0, r1)
            band = RA.resolve_aniso(attrs[:, r0:r1], ids[r0:r1], *table, 8, 0.0, chains=chains)
            assert O.bit_equal(band[0][:, :-1], full_aniso[0][:, r0:r1 - 1]).all(), (name, r0, r1)
            assert not O.bit_equal(band[0][:, -1], full_aniso[0][:, r1 - 1]).all(), (name, r0, r1)
        r0, r1 = FS.LAST_BAND  # even start, ends with the frame: the frame's rows
        band = RM.resolve_mip(attrs[:, r0:r1], ids[r0:r1], *table, 0.0, chains=chains)
        assert r1 == H and O.bit_equal(band[0], full_mip[0][:, r0:r1]).all(), name
