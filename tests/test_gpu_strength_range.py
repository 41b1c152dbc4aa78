"""Light strengths and the constant ambient colour from subnormal values to the top of the float range, through every
kernel family (tests/strength_range_cases.py has the table, tests/test_strength_range_cases.py shows on the CPU that
it holds the cases).

Exact mode (flags 0): bit-identical to the same pass under PBR_FLAG_EXACT_ONLY and to the CPU oracle, NaN for NaN, at
every scale. PBR_FLAG_FAITHFUL: the oracle's NaN pattern and 1e-5 per channel at every scale; at k = 0 the mode ran;
outside the host's strength and ambient window (pbr_context.hip, pbr_set_pass: kFaithfulStrengthLo / Hi,
kFaithfulAmbientHi) the pass stays exact. The exact wave-balanced kernel runs exactly when every point strength is
inside the quarter gate (kQuarterStrengthLo / Hi). Every (family, size, k) prints one line; a case collects what fails
over all k before it asserts, so that one run shows every scale.
"""
import os

import numpy as np
import pytest
import torch

import strength_range_cases as C
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd.renderer import GBuffer, ShadingContext

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5  # the north-star bar
FAMILIES = C.families()


@pytest.fixture(scope="module")
def contexts(gpu):
    """{key: ShadingContext} with the settings of C.CONTEXT_ENV (pbr_context_create reads them), built the way
    test_gpu_balanced.ctx_pair builds its pair."""
    made = {}
    names = sorted({k for env in C.CONTEXT_ENV.values() for k in env})
    saved = {k: os.environ.get(k) for k in names}
    try:
        for key, env in C.CONTEXT_ENV.items():
            for k in names:
                os.environ.pop(k, None)
            os.environ.update(env)
            made[key] = ShadingContext(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield made
    for ctx in made.values():
        ctx.close()


class Table:
    """Frames, their G-buffers on the device and the oracle's frames, each made once per module."""

    def __init__(self, device):
        self.device = device
        self.planes = {size: C.frame(*size) for size in C.SIZES}
        self.gb = {size: GBuffer.from_host(p, device) for size, p in self.planes.items()}
        self.refs = {}

    def oracle(self, size, which, k, negative):
        key = (size, which, k, negative)
        if key not in self.refs:
            lights, counts = C.light_set(self.planes[size], which, k, negative)
            ref = C.oracle_frame(self.planes[size], lights, counts)
            ref.setflags(write=False)
            self.refs[key] = ref
        return self.refs[key]


@pytest.fixture(scope="module")
def table(gpu):
    return Table(gpu)


def shade(ctx, gb, pc):
    """(frame, kernel name, exact_pixels)."""
    ctx.set_pass(pc)
    out = ctx.shade(gb)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ctx.last_kernel(), ctx.pass_stats()["exact_pixels"]


def named(kernel, want):
    prefix, suffix = want
    return kernel.startswith(prefix + "<") and kernel.endswith(suffix)


def faithful_kernel(family, kernel):
    """True / False where the kernel's name tells whether the faithful loop is compiled in and selected, else None (the
    uniform pair kernel and the one-pixel kernel carry the mode as an argument).

    For the families that give None (uniform, culled_uniform, px1) "outside the window the pass is exact" rests on the
    frame having the exact mode's bits alone, which a faithful loop can also produce by coincidence where its sums are
    redone anyway (k = 50 .. 120 on the build before the gates: only k = -30 and k = 127 told the two apart there).
    One host flag (pbr_context.hip, faithful_pass_ok) selects the mode for every family, and the lean and balanced
    families, whose names are asserted, show that it is off."""
    if kernel.startswith("shade_lean_kernel<"):
        return kernel.endswith(", true>")
    if family == "balanced":
        return kernel.endswith(", 1>")
    return None


def line(family, size, k, mode, kernel, got, ref, n_exact):
    e = O.rel_err(got, ref)
    print(f"{family:14s} {size[0]}x{size[1]} k={k} {mode}: {kernel} max_rel={e.max():.3g} "
          f"bit_exact={O.bit_equal(got, ref).mean():.4f} exact_pixels={n_exact}")
    return e


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", list(FAMILIES))
def test_exact_mode_over_strength_scales(family, size, contexts, table):
    """flags 0 with strengths m 2^k (one channel 0, one negative): the bits of PBR_FLAG_EXACT_ONLY and of the oracle at
    every k; the intended kernel at k = 0; the exact balanced kernel exactly inside the quarter gate."""
    key, add, which, kernels, _ = FAMILIES[family]
    ctx, gb, planes = contexts[key], table.gb[size], table.planes[size]
    bad = []
    for k in C.K:
        lights, counts = C.light_set(planes, which, k, True)
        ref = table.oracle(size, which, k, True)
        got, kernel, n_exact = shade(ctx, gb, C.pass_constants(lights, counts, add))
        only, _, _ = shade(ctx, gb, C.pass_constants(lights, counts, add | N.PBR_FLAG_EXACT_ONLY))
        line(family, size, k, "exact", kernel, got, ref, n_exact)
        if not O.bit_equal(got, only).all():
            bad.append(f"k={k}: {int((~O.bit_equal(got, only)).sum())} channels differ from EXACT_ONLY ({kernel})")
        if not O.bit_equal(got, ref).all():
            where = np.argwhere(~O.bit_equal(got, ref))
            bad.append(f"k={k}: {len(where)} channels differ from the oracle ({kernel}), first (y, x, c) "
                       f"{[tuple(int(i) for i in w) for w in where[:3]]}: {[float(got[tuple(w)]) for w in where[:3]]} vs "
                       f"{[float(ref[tuple(w)]) for w in where[:3]]}")
        if k == 0 and not named(kernel, kernels["exact"]):
            bad.append(f"k=0 ran {kernel}")
        if family == "balanced":
            inside = C.in_gate(lights[:, 0:3], C.QUARTER_STRENGTH_LO, C.QUARTER_STRENGTH_HI)
            if kernel.endswith(", 2>") != inside:
                bad.append(f"k={k}: {kernel}, strengths inside the quarter gate: {inside}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", list(FAMILIES))
def test_faithful_mode_over_strength_scales(family, size, contexts, table):
    """PBR_FLAG_FAITHFUL with strengths m 2^k >= 0 (one channel 0): the oracle's NaN pattern and 1e-5 at every k; at
    k = 0 the faithful loop ran (the one-pixel kernel has none: its frames stay exact); outside the host's strength
    window the frame is the exact mode's, from a kernel without the faithful loop."""
    key, add, which, kernels, has_loop = FAMILIES[family]
    ctx, gb, planes = contexts[key], table.gb[size], table.planes[size]
    bad = []
    for k in C.K:
        lights, counts = C.light_set(planes, which, k, False)
        ref = table.oracle(size, which, k, False)
        fast, kernel, n_exact = shade(ctx, gb, C.pass_constants(lights, counts, add | N.PBR_FLAG_FAITHFUL))
        exact, _, _ = shade(ctx, gb, C.pass_constants(lights, counts, add))
        e = line(family, size, k, "faithful", kernel, fast, ref, n_exact)
        same = bool(O.bit_equal(fast, exact).all())
        if not np.array_equal(np.isnan(fast), np.isnan(ref)):
            bad.append(f"k={k}: NaN in {int(np.isnan(fast).sum())} channels, the oracle has {int(np.isnan(ref).sum())}"
                       f" ({kernel})")
        if not e.max() <= REL_TOL:
            bad.append(f"k={k}: max_rel {e.max():.3g} in {int((e > REL_TOL).sum())} channels ({kernel})")
        if k == 0:
            if not named(kernel, kernels["faithful"]):
                bad.append(f"k=0 ran {kernel}")
            if has_loop and (same or n_exact >= planes.shape[1] * planes.shape[2]):
                bad.append(f"k=0: the faithful loop did not run (exact_pixels {n_exact})")
            if not has_loop and not same:
                bad.append("k=0: a kernel without a faithful loop left the exact mode's bits")
        if not C.in_gate(lights[:, 0:3], C.FAITHFUL_STRENGTH_LO, C.FAITHFUL_STRENGTH_HI):
            if not same:
                bad.append(f"k={k}: outside the strength window, yet not the exact mode's frame ({kernel})")
            if faithful_kernel(family, kernel):
                bad.append(f"k={k}: outside the strength window, yet {kernel}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n_lights", [0, C.N_POINT])
def test_ambient_scales(n_lights, contexts, table):
    """The constant ambient (1, 1.25, 1.5) 2^k and the huge-albedo rows, without lights (lean kernel) and with 24
    (balanced tile kernels): exact mode as above; faithful within 1e-5 with the oracle's NaN pattern, and exact from a
    kernel without the faithful loop where the ambient is above the host's bound."""
    family, ctx = ("lean", contexts["lean"]) if n_lights == 0 else ("balanced", contexts["bal"])
    bad = []
    for name, size, planes, ambient, k in C.ambient_table():
        gb = table.gb[size] if k is not None else GBuffer.from_host(planes, table.device)
        lights, counts = (C.light_set(planes, "points", 0, False) if n_lights else (None, (0, 0, 0)))
        ref = C.oracle_frame(planes, lights, counts, ambient)
        got, kernel, n_exact = shade(ctx, gb, C.pass_constants(lights, counts, 0, ambient))
        only, _, _ = shade(ctx, gb, C.pass_constants(lights, counts, N.PBR_FLAG_EXACT_ONLY, ambient))
        line(family, size, name, "exact", kernel, got, ref, n_exact)
        if not O.bit_equal(got, only).all():
            bad.append(f"{name} {size}: {int((~O.bit_equal(got, only)).sum())} channels differ from EXACT_ONLY")
        if not O.bit_equal(got, ref).all():
            bad.append(f"{name} {size}: {int((~O.bit_equal(got, ref)).sum())} channels differ from the oracle")
        fast, kernel, n_exact = shade(ctx, gb, C.pass_constants(lights, counts, N.PBR_FLAG_FAITHFUL, ambient))
        e = line(family, size, name, "faithful", kernel, fast, ref, n_exact)
        if not np.array_equal(np.isnan(fast), np.isnan(ref)):
            bad.append(f"{name} {size} faithful: NaN in {int(np.isnan(fast).sum())} channels, the oracle has "
                       f"{int(np.isnan(ref).sum())} ({kernel})")
        if not e.max() <= REL_TOL:
            bad.append(f"{name} {size} faithful: max_rel {e.max():.3g} in {int((e > REL_TOL).sum())} channels ({kernel})")
        if k == 0:
            want = FAMILIES[family][3]["faithful"]
            if not named(kernel, want) or O.bit_equal(fast, got).all():
                bad.append(f"{name} {size}: the faithful mode did not run ({kernel})")
        if max(float(a) for a in ambient) > C.FAITHFUL_AMBIENT_HI:
            if not O.bit_equal(fast, got).all():
                bad.append(f"{name} {size}: ambient above the bound, yet not the exact mode's frame ({kernel})")
            if faithful_kernel(family, kernel):
                bad.append(f"{name} {size}: ambient above the bound, yet {kernel}")
    assert not bad, "\n".join(bad)
