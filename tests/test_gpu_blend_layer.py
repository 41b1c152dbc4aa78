"""pbr_blend_layer on the GPU (csrc/blend_layer.h; the transparent PSO's output merger, PBRApp.cpp:831-842): both
destination formats bit for bit -- bytes for RGBA8_UNORM -- against the numpy float32 restatement of
tests/blend_layer_reference.py, padding and uncovered pixels included. A library without the entry point fails every
test here (the binding raises); none is skipped."""
import numpy as np
import pytest
import torch

import blend_layer_reference as BR
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu

ALPHAS = np.array([0, 0.1, 0.5, 1, -0.25, 1.5, np.nan], np.float32)
COLOURS = np.array([0, 0.3, 1, 2.5, np.nan, np.inf], np.float32)
W, H = 71, 13  # an odd width, two tiles across and down; 923 pixels: every (alpha, colour) pair many times over


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


def inputs(w=W, h=H, seed=0):
    """src, alpha, coverage, and both destinations on the host: every alpha against every colour in every channel,
    about a third of the pixels uncovered, and a destination with every byte / a spread of floats (a NaN and an inf
    among them, under covered and uncovered pixels)."""
    rng = np.random.default_rng(seed)
    i = np.arange(w * h).reshape(h, w)
    alpha = ALPHAS[i % 7]
    src = np.stack([COLOURS[(i // 7 + c) % 6] for c in range(3)] + [rng.normal(size=(h, w)).astype(np.float32)], -1)
    coverage = rng.choice(np.array([0, 1, 255], np.uint8), size=(h, w))
    dst8 = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    dst32 = rng.uniform(-0.5, 2.0, (h, w, 4)).astype(np.float32)
    dst32[1, 3], dst32[2, 5], dst32[4, 4] = np.nan, np.inf, -0.0
    assert (coverage == 0).any() and (coverage != 0).any()
    return src, alpha, coverage, dst8, dst32


def embed(a, row_elems, offset, dev, fill):
    """``a`` (h, w[, 4]) inside a flat sentinel-filled device buffer: rows ``row_elems`` elements apart, the first
    element at ``offset``. Returns (the view, the whole buffer)."""
    h = a.shape[0]
    flat = torch.full((offset + h * row_elems + 8,), fill, dtype=torch.from_numpy(a).dtype, device=dev)
    strides = (row_elems, 4, 1) if a.ndim == 3 else (row_elems, 1)
    view = flat.as_strided(a.shape, strides, offset)
    view.copy_(torch.from_numpy(a).to(dev))
    return view, flat


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(ctx, gpu, fmt8, src_off, dst_off, pad, rows=None):
    """One blend through buffers with the given element offsets and ``pad`` extra pixels per row; the whole
    destination buffer must equal the same buffer with the restatement's result embedded."""
    src, alpha, coverage, dst8, dst32 = inputs()
    dst = dst8 if fmt8 else dst32
    s_v, _ = embed(src, (W + pad) * 4, src_off, gpu, -7.0)
    a_v, _ = embed(alpha, W + pad + 2, 1, gpu, -7.0)
    c_v, _ = embed(coverage, W + pad + 4, 3, gpu, 9)
    fill = 0x5A if fmt8 else -12345.25
    dst_off = dst_off * 4 if fmt8 else dst_off  # an RGBA8 pixel is one 4-byte element: offsets in pixels
    d_v, d_flat = embed(dst, (W + pad) * 4, dst_off, gpu, fill)
    r0, r1 = (0, H) if rows is None else rows
    want = dst.copy()
    want[r0:r1] = BR.blend(src[r0:r1], alpha[r0:r1], coverage[r0:r1], dst[r0:r1])
    w_v, w_flat = embed(want, (W + pad) * 4, dst_off, gpu, fill)
    ctx.blend_layer(s_v[r0:r1], a_v[r0:r1], c_v[r0:r1], d_v[r0:r1], width=W, height=r1 - r0)
    torch.cuda.synchronize()
    got, exp = bits(d_flat), bits(w_flat)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:6].tolist()}: {got[bad[:6]]} != {exp[bad[:6]]}"
    return want


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgba32f", "rgba8"])
def test_aligned_layout_equals_the_restatement(ctx, gpu, fmt8):
    """16-byte aligned source and destination, no padding: the 16-byte accesses. Covered pixels change, uncovered
    pixels keep their bytes."""
    want = run(ctx, gpu, fmt8, 0, 0, 0)
    src, alpha, coverage, dst8, dst32 = inputs()
    dst = dst8 if fmt8 else dst32
    same = bits(torch.from_numpy(want)) == bits(torch.from_numpy(dst))
    assert same[coverage == 0].all() and not same[coverage != 0].all()
    if not fmt8:  # out.a = a, bit for bit, a NaN's included
        assert (want[..., 3].view(np.uint32)[coverage != 0] == alpha.view(np.uint32)[coverage != 0]).all()


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgba32f", "rgba8"])
@pytest.mark.parametrize("src_off,dst_off,pad", [(1, 0, 1), (0, 3, 2), (2, 1, 3), (4, 4, 1)])
def test_unaligned_pointers_and_padded_strides(ctx, gpu, fmt8, src_off, dst_off, pad):
    """Pointers that are only 4-byte aligned (element offsets 1, 2, 3 of the 16-byte grid; 4 is aligned again) and rows
    with padding: the scalar path; the padding and the buffer's ends keep their sentinel."""
    run(ctx, gpu, fmt8, src_off, dst_off, pad)


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgba32f", "rgba8"])
def test_a_row_band_leaves_the_other_rows(ctx, gpu, fmt8):
    for rows in ((0, 3), (3, 4), (4, H)):
        run(ctx, gpu, fmt8, 0, 0, 1, rows=rows)


def test_the_restatement_on_values_worked_by_hand():
    """The numpy side against numbers that need no code: a = 0.5 over d = 1, s = 0.3 -> 0.65; RGBA8: d = 255, s = 2.5
    (clamped to 1), a = 1.5 (clamped to 1) -> 255; a = NaN -> alpha byte 0 and colour = d."""
    one = lambda v, dt=np.float32: np.full((1, 1), v, dt)  # noqa: E731
    src = np.array([[[0.3, 2.5, np.nan, 9.0]]], np.float32)
    out = BR.blend(src, one(0.5), one(1, np.uint8), np.ones((1, 1, 4), np.float32))
    assert out[0, 0, 0] == np.float32(0.3) * np.float32(0.5) + np.float32(0.5) and out[0, 0, 3] == np.float32(0.5)
    assert np.isnan(out[0, 0, 2])
    d8 = np.full((1, 1, 4), 255, np.uint8)
    assert BR.blend(src, one(1.5), one(1, np.uint8), d8)[0, 0].tolist() == [77, 255, 0, 255]  # 0.3 * 255 + 0.5 = 77.0
    assert BR.blend(src, one(np.nan), one(1, np.uint8), d8)[0, 0].tolist() == [255, 255, 255, 0]
    assert BR.blend(src, one(0.5), one(0, np.uint8), d8)[0, 0].tolist() == [255, 255, 255, 255]


def test_bad_arguments_are_refused(ctx, gpu):
    src, alpha, coverage, dst8, dst32 = (torch.from_numpy(a).to(gpu) for a in inputs())
    lib, h = ctx.lib, ctx.handle
    b, f = N.BlendSource(), N.FrameDesc()
    b.src, b.src_row_stride = src.data_ptr(), W
    b.alpha, b.alpha_row_stride = alpha.data_ptr(), W
    b.coverage, b.coverage_row_stride = coverage.data_ptr(), W
    f.out, f.out_row_stride, f.format = dst32.data_ptr(), W, N.PBR_OUTPUT_RGBA32F
    import ctypes

    call = lambda w=W, hh=H: lib.pbr_blend_layer(h, ctypes.byref(b), ctypes.byref(f), w, hh, None)  # noqa: E731
    assert call() == N.PBR_OK
    assert call(0, 0) == N.PBR_OK  # an empty rectangle: nothing to do
    for field, obj in (("src", b), ("alpha", b), ("coverage", b), ("out", f)):
        keep = getattr(obj, field)
        setattr(obj, field, None)
        assert call() == N.PBR_ERR_INVALID_ARGUMENT, field
        setattr(obj, field, keep)
    f.format = 7
    assert call() == N.PBR_ERR_INVALID_ARGUMENT
    f.format = N.PBR_OUTPUT_RGBA32F
    b.alpha_row_stride = W - 1
    assert call() == N.PBR_ERR_INVALID_ARGUMENT
    b.alpha_row_stride = W
    b.src = src.data_ptr() + 2  # not 4-byte aligned
    assert call() == N.PBR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
