"""pbr_msaa_resolve on the GPU (csrc/msaa_resolve.h) against the numpy restatement of
tests/raster_msaa_reference.py, bit for bit in both formats (oracle.bit_equal: NaN patterns equal). A library without
the entry point fails every test here (the binding raises); none is skipped."""
import ctypes

import numpy as np
import pytest
import torch

import raster_msaa_reference as M
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import ShadingContext

pytestmark = pytest.mark.gpu

COLOURS = np.array([0.0, 0.3, 1.0, 2.5, np.nan, np.inf, 1e-40], np.float32)  # the last one a denormal
OWNERS = (0x00, 0xE4, 0x44, 0x50)
SENTINEL = np.float32(-12345.25)
W, H = 67, 9  # an odd width, more than one 64 x 4 tile in both directions


@pytest.fixture(scope="module")
def ctx(gpu):
    c = ShadingContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs():
    """Four slot frames over COLOURS and random values, and an owner plane with OWNERS and random bytes."""
    rng = np.random.default_rng(61)
    frames = COLOURS[rng.integers(0, len(COLOURS), (4, H, W, 4))]
    mix = rng.random((4, H, W, 4)) < 0.4
    frames[mix] = rng.uniform(-0.5, 1.5, int(mix.sum())).astype(np.float32)
    owner = rng.integers(0, 256, (H, W)).astype(np.uint8)
    named = rng.random((H, W)) < 0.6
    owner[named] = np.array(OWNERS, np.uint8)[rng.integers(0, 4, int(named.sum()))]
    for j, o in enumerate(OWNERS):  # every colour under every named owner byte, in slot frames 0 .. 3 in turn
        for i, c in enumerate(COLOURS):
            owner[j, i] = o
            frames[:, j, i] = np.roll(COLOURS, i)[:4, None]
    return frames, owner


def on_device(frames, offset_floats=0, stride=None):
    """The frames in one buffer each, `offset_floats` floats past a 16-byte boundary, rows `stride` pixels apart."""
    out = []
    n, h, w, _ = frames.shape
    stride = w if stride is None else stride
    for f in frames:
        buf = torch.full((h * stride * 4 + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
        view = buf[offset_floats:offset_floats + h * stride * 4].view(h, stride, 4)
        view[:, :w] = torch.from_numpy(np.ascontiguousarray(f)).cuda()
        out.append(view)
    return out


def check(got, frames, owner, n_slots, fmt, what):
    want = M.resolve(frames, owner, n_slots, fmt)
    if fmt == M.RGBA8:
        assert np.array_equal(got, want), f"{what}: differs at {np.argwhere(got != want)[:4].tolist()}"
    else:
        eq = O.bit_equal(got, want)
        assert eq.all(), f"{what}: differs at {np.argwhere(~eq)[:4].tolist()}"


@pytest.mark.parametrize("n_slots", [1, 2, 3, 4])
@pytest.mark.parametrize("fmt", [M.RGBA32F, M.RGBA8])
def test_resolve_equals_the_restatement(ctx, inputs, n_slots, fmt):
    """Every colour under every owner byte, for n_slots 1 .. 4: a sample whose owner is >= n_slots contributes zero,
    and the pointers of the slots past n_slots are NULL."""
    frames, owner = inputs
    slots = on_device(frames)
    dfmt = N.PBR_OUTPUT_RGBA8_UNORM if fmt == M.RGBA8 else N.PBR_OUTPUT_RGBA32F
    got = ctx.msaa_resolve(slots[:n_slots] + [None] * (4 - n_slots), torch.from_numpy(owner).cuda(), fmt=dfmt,
                           n_slots=n_slots)
    torch.cuda.synchronize()
    check(got.cpu().numpy(), frames, owner, n_slots, fmt, f"n_slots {n_slots}")
    if n_slots < 4:
        assert (((owner >> 6) & 3) >= n_slots).any()


def test_four_equal_colours_give_the_colour(ctx):
    """Random float32 bit patterns, a row of denormals among them: one fragment in every sample returns its colour bit
    for bit (values whose fourfold overflows excepted), whatever the owner byte."""
    rng = np.random.default_rng(62)
    c = rng.integers(0, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    c[1] = rng.integers(1, 2 ** 23, (W, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    owner = rng.integers(0, 256, (H, W)).astype(np.uint8)
    slot = on_device(c[None])[0]
    got = ctx.msaa_resolve([slot] * 4, torch.from_numpy(owner).cuda()).cpu().numpy()
    with np.errstate(all="ignore"):
        fits = np.abs(c.astype(np.float64) * 4) <= np.finfo(np.float32).max
    assert O.bit_equal(got[fits], c[fits]).all() and fits.mean() > 0.9
    assert O.bit_equal(got, M.resolve([c] * 4, owner, 4)).all()
    zero = np.zeros((H, W), np.uint8)
    assert O.bit_equal(ctx.msaa_resolve([slot], torch.from_numpy(zero).cuda()).cpu().numpy()[fits], c[fits]).all()


@pytest.mark.parametrize("fmt", [M.RGBA32F, M.RGBA8])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_alignment_strides_and_padding(ctx, inputs, offset, fmt):
    """Slot frames at every 4-byte offset of the 16-byte grid (offset 0: the 16-byte accesses), the output likewise,
    padded row strides everywhere; the padding of the output stays untouched."""
    frames, owner = inputs
    slots = on_device(frames, offset_floats=offset, stride=W + 3)
    assert slots[0].data_ptr() % 16 == 4 * offset
    downer = torch.full((H, W + 5), 0xA5, dtype=torch.uint8, device="cuda")
    downer[:, :W] = torch.from_numpy(owner).cuda()
    if fmt == M.RGBA8:
        buf = torch.full((H, W + 2, 4), 0x5A, dtype=torch.uint8, device="cuda")
        out, pad = buf, 0x5A
    else:
        buf = torch.full((H * (W + 2) * 4 + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
        out, pad = buf[offset:offset + H * (W + 2) * 4].view(H, W + 2, 4), SENTINEL
    ctx.msaa_resolve(slots, downer, out=out, width=W, height=H)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    check(got[:, :W], frames, owner, 4, fmt, f"offset {offset}")
    assert (got[:, W:] == pad).all()
    if fmt == M.RGBA32F:
        host = buf.cpu().numpy()
        assert (host[:offset] == SENTINEL).all() and (host[offset + H * (W + 2) * 4:] == SENTINEL).all()
    for s in slots:  # the sources are only read
        assert (s.cpu().numpy()[:, W:] == SENTINEL).all()


def test_argument_errors(ctx, inputs):
    """n_slots outside 1 .. 4, a NULL slot below n_slots, a NULL owner or output, strides below the width, an unknown
    format: PBR_ERR_INVALID_ARGUMENT; an empty rectangle is PBR_OK and writes nothing."""
    frames, owner = inputs
    slots = on_device(frames)
    downer = torch.from_numpy(owner).cuda()
    out = torch.full((H, W, 4), float(SENTINEL), dtype=torch.float32, device="cuda")

    def call(n_slots=4, slot0=slots[0].data_ptr(), own=downer.data_ptr(), dst=out.data_ptr(), slot_stride=W,
             owner_stride=W, out_stride=W, fmt=N.PBR_OUTPUT_RGBA32F, w=W, h=H):
        src = N.MsaaResolveSource()
        src.slots[:] = [slot0] + [s.data_ptr() for s in slots[1:]]
        src.slot_row_stride, src.n_slots, src.owner, src.owner_row_stride = slot_stride, n_slots, own, owner_stride
        f = N.FrameDesc()
        f.out, f.out_row_stride, f.format = dst, out_stride, fmt
        return ctx.lib.pbr_msaa_resolve(ctx.handle, ctypes.byref(src), ctypes.byref(f), w, h, None)

    for kw in (dict(n_slots=0), dict(n_slots=5), dict(slot0=None), dict(own=None), dict(dst=None),
               dict(slot_stride=W - 1), dict(owner_stride=W - 1), dict(out_stride=W - 1), dict(fmt=77), dict(w=-1),
               dict(slot0=slots[0].data_ptr() + 2)):
        assert call(**kw) == N.PBR_ERR_INVALID_ARGUMENT, kw
    assert call(w=0) == N.PBR_OK and call(h=0) == N.PBR_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call() == N.PBR_OK
    torch.cuda.synchronize()
    check(out.cpu().numpy(), frames, owner, 4, M.RGBA32F, "after the refusals")
