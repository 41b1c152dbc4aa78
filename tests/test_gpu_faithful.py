"""PBR_FLAG_FAITHFUL (tolerance mode): hardware-reciprocal divisions in the well-conditioned BRDF terms.

Bar (north_star): |gpu - cpu| <= 1e-5 * |cpu| per RGBA channel against the CPU oracle of the reference
math. The mode is not bit-identical by design, so each test also shows that it ran (some channels differ
from the exact default) or, where its host preconditions fail, that the pass stayed exact (bit-identical
to the default mode).
"""
import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden, oracle_pass_from_constants
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import GBuffer, PassConstants

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5


def with_flags(pc, add=0, remove=0):
    return PassConstants(**{**pc.__dict__, "flags": (pc.flags | add) & ~remove})


def shade(ctx, gb, pc, env):
    ctx.set_pass(pc)
    if env is not None:
        ctx.set_env_map(env)
    out = ctx.shade(gb)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# cfg4: 256 lights under tiled culling (each wave counts its ~5 surviving terms against the bound's 64)
# on a normal-mapped material plane (the faithful loop's non-lean variant).
@pytest.mark.parametrize("cid,size,row_step,active", [(2, None, 1, True), (3, None, 8, True), (4, None, 8, True),
                                                      (3, (1024, 128), 1, True)])
def test_faithful_config_within_tolerance(cid, size, row_step, active, shading_ctx, gpu):
    cfg = S.CONFIGS[cid] if size is None else S.CONFIGS[cid].with_size(*size)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    env = S.env_map() if pc.ambient_mode == N.PBR_AMBIENT_IBL_DIFFUSE else None
    gb = GBuffer.from_host(planes, gpu)
    fast = shade(shading_ctx, gb, with_flags(pc, N.PBR_FLAG_FAITHFUL), env)
    exact = shade(shading_ctx, gb, pc, env)
    ref = O.shade(list(np.ascontiguousarray(planes[:, ::row_step])), oracle_pass_from_constants(pc),
                  pc.light_array(), env, n_threads=16)
    e = O.rel_err(fast[::row_step], ref)
    same = O.bit_equal(fast, exact).mean()
    print(f"{cfg.name} {cfg.width}x{cfg.height}: faithful max_rel={e.max():.3g} "
          f"bit-identical to exact {same:.4f}")
    assert e.max() <= REL_TOL
    if active:
        assert same < 1.0  # the faithful loop ran
    assert O.rel_err(exact[::row_step], ref).max() <= REL_TOL


@pytest.mark.parametrize("cid", [3, 4])
def test_full_frame_faithful_parity(cid, shading_ctx, gpu):
    """The benchmark's mode over EVERY row of the full 3840x2160 frame -- config 3 (64 point lights + IBL,
    wave-balanced faithful lists: the headline kernel) and config 4 (256 lights, tiled culling, F0 plane) --
    against the oracle on 16 host threads: max relative error <= 1e-5 per channel, NaN exactly where the oracle
    has NaN. bench.py refuses to print a throughput for a frame that misses this bar (parity_failures)."""
    cfg = S.CONFIGS[cid]
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = with_flags(S.scene_pass(cfg), N.PBR_FLAG_FAITHFUL)
    env = S.env_map() if pc.ambient_mode == N.PBR_AMBIENT_IBL_DIFFUSE else None
    gb = GBuffer.from_host(planes, gpu)
    got = shade(shading_ctx, gb, pc, env)
    del gb
    ref = O.shade(list(planes), oracle_pass_from_constants(pc), pc.light_array(), env, n_threads=16)
    assert got.shape == ref.shape == (cfg.height, cfg.width, 4)
    e = O.rel_err(got, ref)
    print(f"{cfg.name} full frame, faithful mode: max_rel={e.max():.3g} "
          f"bit-identical {O.bit_equal(got, ref).mean():.4f}")
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert e.max() <= REL_TOL


@pytest.mark.parametrize("name", golden_names())
def test_faithful_golden_vectors(name, shading_ctx, gpu, env_map):
    """The golden fixtures (edge pixels with NaN/inf/subnormals/|N| > 1 included): waves outside the
    mode's conditions stay exact, the rest are within the tolerance."""
    from test_gpu_parity import pass_from_meta

    planes, lights, meta, expected = load_golden(name)
    pc = with_flags(pass_from_meta(meta, lights), N.PBR_FLAG_FAITHFUL)
    gb = GBuffer.from_host(planes, gpu)
    got = shade(shading_ctx, gb, pc, env_map if meta["env"] else None)
    e = O.rel_err(got, expected)
    print(f"{name}: faithful max_rel={e.max():.3g}")
    assert e.max() <= REL_TOL
    assert np.array_equal(np.isnan(got), np.isnan(expected))


@pytest.mark.parametrize("case", ["negative_strength", "negative_ambient", "exact_only", "65_lights",
                                  "culled_100_lights_in_range", "tiny_strength", "huge_strength", "huge_ambient"])
def test_faithful_preconditions_keep_the_pass_exact(case, shading_ctx, gpu):
    """Where a light term could be negative (strength, ambient), the sum is longer than the bound
    allows (> 64 lights), a strength is outside [2^-25, 2^50] (a product of the rearranged term underflows,
    or the reference's radiance overflows) or the constant ambient above 2^100 (the finish's reciprocal
    underflows) the error bound does not hold: the host turns the mode off and the frame
    equals the default (exact) mode bit for bit."""
    import dataclasses

    cfg = S.CONFIGS[2].with_size(512, 64)
    if case == "65_lights":
        cfg = dataclasses.replace(cfg, n_lights=65)
    if case == "culled_100_lights_in_range":  # every wave keeps all 100 lights: > 64 summed terms
        cfg = dataclasses.replace(cfg, n_lights=100, flags=N.PBR_FLAG_TILED_CULLING)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    if case == "negative_strength":
        arr = pc.light_array().copy()
        arr[3, 1] = -1.0
        pc = PassConstants(**{**pc.__dict__, "lights_array": arr})
    elif case in ("tiny_strength", "huge_strength"):
        arr = pc.light_array().copy()
        arr[3, 1] = 1.0e-30 if case == "tiny_strength" else 1.0e30
        pc = PassConstants(**{**pc.__dict__, "lights_array": arr})
    elif case == "negative_ambient":
        pc = PassConstants(**{**pc.__dict__, "ambient_light": (0.03, -0.01, 0.03)})
    elif case == "huge_ambient":
        pc = PassConstants(**{**pc.__dict__, "ambient_light": (0.03, 2.0 ** 101, 0.03)})
    extra = N.PBR_FLAG_EXACT_ONLY if case == "exact_only" else 0
    gb = GBuffer.from_host(planes, gpu)
    exact = shade(shading_ctx, gb, with_flags(pc, extra), None)
    fast = shade(shading_ctx, gb, with_flags(pc, N.PBR_FLAG_FAITHFUL | extra), None)
    assert O.bit_equal(fast, exact).all()


def test_faithful_negative_albedo_waves_stay_exact(shading_ctx, gpu):
    """Per-wave condition: a pixel pair with a negative albedo or F0 > 1 keeps its wave on the exact loop."""
    cfg = S.CONFIGS[2].with_size(256, 16)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    planes = planes.copy()
    # every wave (64x2 pixels) gets one pixel with a negative albedo channel
    planes[7, ::2, ::64] = -0.25
    gb = GBuffer.from_host(planes, gpu)
    exact = shade(shading_ctx, gb, pc, None)
    fast = shade(shading_ctx, gb, with_flags(pc, N.PBR_FLAG_FAITHFUL), None)
    assert O.bit_equal(fast, exact).all()


def _adversarial_scene(seed, w=512, h=128, n_lights=64):
    """Pixels on the specular peak of one light each (N = normalize(V + L_k), roughness 0..0.1: the
    ill-conditioned GGX regime), grazing views (N.V ~ 1e-3), metallic 0/1, albedo 0/tiny/1, light
    strengths over six decades, 20 % of the lights spot lights with sharp cones."""
    rng = np.random.default_rng(seed)
    n = w * h
    eye = np.array([0.0, 0.0, -5.0])
    pos = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0, 8, n)], 1)
    lpos = np.stack([rng.uniform(-20, 20, n_lights), rng.uniform(-20, 20, n_lights), rng.uniform(-20, 5, n_lights)], 1)
    v = eye - pos
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    k = np.arange(n) % n_lights
    l = lpos[k] - pos
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    nrm = v + l
    kind = rng.integers(0, 4, n)
    graze = kind == 1  # N nearly perpendicular to V
    t = np.cross(v[graze], rng.normal(size=(graze.sum(), 3)))
    nrm[graze] = t + 1e-3 * v[graze] * np.linalg.norm(t, axis=1, keepdims=True)
    rand = kind == 2
    nrm[rand] = rng.normal(size=(rand.sum(), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    planes = np.zeros((15, h, w), np.float32)
    planes[0:3] = pos.T.reshape(3, h, w)
    planes[3:6] = nrm.T.reshape(3, h, w)
    metal = rng.choice([0.0, 1.0, 0.5], n, p=[0.4, 0.4, 0.2])
    alb = rng.uniform(0, 1, (n, 3))
    alb[rng.random(n) < 0.1] = 1e-6
    alb[(rng.random(n) < 0.05) & (metal == 0.0)] = 0.0  # F0 = lerp(0.04, 0, 0) stays nonzero: lean waves
    planes[6:9] = alb.T.reshape(3, h, w)
    planes[9] = metal.reshape(h, w)
    planes[10] = np.where(rng.random(n) < 0.7, rng.uniform(0, 0.1, n), rng.uniform(0, 1, n)).reshape(h, w)
    planes[11] = 1.0
    lights = np.zeros((n_lights, 12), np.float32)
    lights[:, 0:3] = 10.0 ** rng.uniform(-3, 3, (n_lights, 3))
    lights[:, 3] = rng.uniform(1, 200, n_lights)  # spot power
    d = rng.normal(size=(n_lights, 3))
    lights[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    lights[:, 8:11] = lpos
    n_spot = n_lights // 5
    return planes, lights, n_lights - n_spot, n_spot


@pytest.mark.parametrize("seed,ambient_mode", [(1, 0), (2, 1), (3, 0)])
def test_faithful_adversarial_peaks_and_grazing(seed, ambient_mode, shading_ctx, gpu, env_map):
    planes, lights, n_point, n_spot = _adversarial_scene(seed)
    pc = PassConstants(eye_pos_w=(0.0, 0.0, -5.0), ambient_light=(0.0, 0.0, 0.0) if seed == 3 else (0.03, 0.03, 0.03),
                       num_point_lights=n_point, num_spot_lights=n_spot, ambient_mode=ambient_mode,
                       lights_array=lights)
    env = env_map if ambient_mode else None
    gb = GBuffer.from_host(planes, gpu)
    fast = shade(shading_ctx, gb, with_flags(pc, N.PBR_FLAG_FAITHFUL), env)
    exact = shade(shading_ctx, gb, pc, env)
    ref = O.shade(list(planes), oracle_pass_from_constants(pc), pc.light_array(), env, n_threads=16)
    e = O.rel_err(fast, ref)
    same = O.bit_equal(fast, exact).mean()
    print(f"adversarial seed {seed}: faithful max_rel={e.max():.3g} (p99.99 {np.quantile(e, 0.9999):.3g}), "
          f"bit-identical to exact {same:.4f}")
    assert e.max() <= REL_TOL
    assert same < 0.9  # the faithful loop ran on these waves
    assert O.rel_err(exact, ref).max() <= REL_TOL
