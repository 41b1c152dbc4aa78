"""GPU parity: the gfx950 kernel (through the C ABI) against the CPU oracle and the golden vectors.

Tolerance (north_star): |gpu - cpu| <= 1e-5 * |cpu| per RGBA channel, fp32, NaN == NaN. The kernel
uses the oracle's operation order, no FMA contraction and correctly rounded div/sqrt, and evaluates
atan2f/asinf/powf with glibc's own algorithms (csrc/libm_f32.h), so nearly all channels are
bit-identical; the residue comes from the per-light pow(x, 5) off the grazing band, where the kernel
uses a correctly rounded fp64 x^5 instead of glibc's powf (pbr_device_math.h, pow5_light: <= 1.2e-6).
Culled vs unculled and band vs full-frame comparisons are required to be bit-identical.
"""
import os

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden, oracle_pass_from_constants, oracle_pass_from_meta
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import scenes as S
from physically_based_renderer_amd.renderer import GBuffer, PassConstants, ShadingContext

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5


def pass_from_meta(meta, lights):
    flags = (N.PBR_FLAG_F0_PLANE if meta["use_f0_plane"] else 0) | (N.PBR_FLAG_APPLY_AO if meta["apply_ao"] else 0)
    return PassConstants(eye_pos_w=meta["eye"], ambient_light=meta["ambient"], fresnel_r0=meta["fresnel_r0"],
                         opacity=meta["opacity"], num_dir_lights=meta["n_dir"], num_point_lights=meta["n_point"],
                         num_spot_lights=meta["n_spot"], ambient_mode=meta["ambient_mode"], flags=flags,
                         lights_array=lights)


def gpu_shade(ctx, planes, pc, env, device):
    ctx.set_pass(pc)
    if env is not None:
        ctx.set_env_map(env)
    gb = GBuffer.from_host(planes, device)
    out = ctx.shade(gb)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def report(name, got, ref):
    e = O.rel_err(got, ref)
    exact = O.bit_equal(got, ref).mean()
    print(f"{name}: max_rel={e.max():.3g} bit_exact={exact:.6f} n={ref.size}")
    return e


@pytest.mark.parametrize("name", golden_names())
def test_golden_vectors_on_gpu(name, shading_ctx, gpu, env_map):
    planes, lights, meta, expected = load_golden(name)
    pc = pass_from_meta(meta, lights)
    got = gpu_shade(shading_ctx, planes, pc, env_map if meta["env"] else None, gpu)
    e = report(name, got, expected)
    assert e.max() <= REL_TOL
    assert np.array_equal(np.isnan(got), np.isnan(expected))


def config_parity(ctx, device, cfg, row_step=1, n_threads=16, env=None):
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    env = S.env_map() if pc.ambient_mode == N.PBR_AMBIENT_IBL_DIFFUSE else None
    got = gpu_shade(ctx, planes, pc, env, device)[::row_step]
    ref = O.shade(list(np.ascontiguousarray(planes[:, ::row_step])), oracle_pass_from_constants(pc),
                  pc.light_array(), env, n_threads=n_threads)
    return got, ref, pc


@pytest.mark.parametrize("cid,size,row_step", [(1, None, 1), (2, (640, 96), 1), (3, (512, 64), 1),
                                               (4, (1024, 256), 1), (2, None, 1), (3, None, 16), (4, None, 16),
                                               (5, (8192, 64), 1)])
def test_config_parity(cid, size, row_step, shading_ctx, gpu):
    cfg = S.CONFIGS[cid] if size is None else S.CONFIGS[cid].with_size(*size)
    got, ref, _ = config_parity(shading_ctx, gpu, cfg, row_step)
    e = report(f"{cfg.name} {cfg.width}x{cfg.height} step{row_step}", got, ref)
    assert e.max() <= REL_TOL


@pytest.mark.parametrize("cid", [3, 4])
def test_full_frame_exact_mode_parity(cid, shading_ctx, gpu):
    """The default (exact) mode over EVERY row of the full 3840x2160 config-3 frame (64 point lights + IBL,
    wave-balanced exact lists) and config-4 frame (256 lights, tiled culling, F0 plane), against the oracle
    on 16 host threads: bit-identical but for the documented per-light x^5 residue (pow5_light, <= 1.2e-6 of
    that light's diffuse term)."""
    cfg = S.CONFIGS[cid]
    got, ref, pc = config_parity(shading_ctx, gpu, cfg, 1)
    assert not pc.flags & N.PBR_FLAG_FAITHFUL
    e = report(f"{cfg.name} full frame, exact mode", got, ref)
    assert got.shape == (cfg.height, cfg.width, 4)
    assert O.bit_equal(got, ref).mean() >= 0.99999
    assert e.max() <= 1.2e-6


def test_tiled_culling_is_bit_exact(shading_ctx, gpu):
    cfg = S.CONFIGS[4]
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    assert pc.flags & N.PBR_FLAG_TILED_CULLING
    gb = GBuffer.from_host(planes, gpu)
    shading_ctx.set_pass(pc)
    culled = shading_ctx.shade(gb).clone()
    kept, tiles = shading_ctx.cull_stats()
    pc_full = PassConstants(**{**pc.__dict__, "flags": pc.flags & ~N.PBR_FLAG_TILED_CULLING})
    shading_ctx.set_pass(pc_full)
    full = shading_ctx.shade(gb)
    torch.cuda.synchronize()
    assert O.bit_equal(culled.cpu().numpy(), full.cpu().numpy()).all()
    tile_w, tile_h = cull_tile()
    assert tiles == ((cfg.width + tile_w - 1) // tile_w) * ((cfg.height + tile_h - 1) // tile_h)
    mean_kept = kept / tiles
    print(f"cfg4 tiled culling: {mean_kept:.2f} of {cfg.n_lights} lights per {tile_w}x{tile_h} tile")
    assert 0 < mean_kept < cfg.n_lights / 4


def cull_tile():
    """The culling unit: one wave64's pixels (64x2 pairs) or one 32x8 workgroup (one-pixel layout)."""
    return (32, 8) if os.environ.get("PBR_PIXELS_PER_THREAD") == "1" else (64, 2)


def host_tile_survivors(planes, lights, tile_w, tile_h):
    """The kernel's per-tile range test (shade_light_loops.h, stage_chunk) emulated in float32: box
    distance per axis with maxNum, (dx*dx + dy*dy) + dz*dz rounded per operation, <= 100.01f^2."""
    h, w = planes.shape[1:]
    th, tw = -(-h // tile_h), -(-w // tile_w)
    pad = np.full((3, th * tile_h, tw * tile_w), np.nan, np.float32)
    pad[:, :h, :w] = planes[0:3]
    t = pad.reshape(3, th, tile_h, tw, tile_w)
    lo = np.nanmin(t, axis=(2, 4)).reshape(3, -1)
    hi = np.nanmax(t, axis=(2, 4)).reshape(3, -1)
    r2 = np.float32(100.01) * np.float32(100.01)
    total = 0
    for lp in lights[:, 8:11].astype(np.float32):
        d = [np.maximum(np.maximum(lo[i] - lp[i], lp[i] - hi[i]), np.float32(0)) for i in range(3)]
        total += int(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= r2).sum())
    return total, th * tw


def test_cull_stats_equal_host_emulation(shading_ctx, gpu):
    """pbr_last_cull_stats (one count per tile, summed on the host) equals the range test emulated on
    the host, at the full config-4 size and on a ragged frame."""
    tile_w, tile_h = cull_tile()
    for cfg in (S.CONFIGS[4], S.CONFIGS[4].with_size(1000, 203)):
        planes, _ = S.fill_gbuffer_host(cfg)
        pc = S.scene_pass(cfg)
        shading_ctx.set_pass(pc)
        shading_ctx.shade(GBuffer.from_host(planes, gpu))
        kept, tiles = shading_ctx.cull_stats()
        want_kept, want_tiles = host_tile_survivors(planes, pc.light_array(), tile_w, tile_h)
        assert (kept, tiles) == (want_kept, want_tiles), cfg.name


def test_odd_row_stride_and_unaligned_planes(shading_ctx, gpu, env_map):
    """Input rows wider than the frame (odd stride) and planes starting 4 bytes off an 8-byte
    boundary: the pair kernel's scalar-load path. Compared with the oracle on the packed planes."""
    cfg = S.CONFIGS[3].with_size(101, 37)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    ref = O.shade(list(planes), oracle_pass_from_constants(pc), pc.light_array(), env_map, n_threads=8)
    shading_ctx.set_pass(pc)
    shading_ctx.set_env_map(env_map)
    big = np.full((15, 37, 103), np.nan, np.float32)  # row stride 103: odd
    for c0 in (0, 1):  # c0 = 1: every plane starts 4 bytes off an 8-byte boundary
        big[:] = np.nan
        big[:, :, c0:c0 + 101] = planes
        dev = torch.from_numpy(big).to(gpu)
        view = GBuffer(dev[:, :, c0:], width=101)
        assert view.row_stride == 103
        got = shading_ctx.shade(view).cpu().numpy()
        assert report(f"stride 103, column offset {c0}", got, ref).max() <= REL_TOL


def test_culling_with_nonfinite_positions(shading_ctx, gpu):
    cfg = S.CONFIGS[4].with_size(256, 64)
    planes, _ = S.fill_gbuffer_host(cfg)
    planes[0, 3, 5] = np.nan
    planes[2, 40, 200] = np.inf
    pc = S.scene_pass(cfg)
    got = gpu_shade(shading_ctx, planes, pc, None, gpu)
    ref = O.shade(list(planes), oracle_pass_from_constants(pc), pc.light_array(), None, n_threads=8)
    assert report("cfg4 nonfinite", got, ref).max() <= REL_TOL


def test_f0_plane_equals_metallic_workflow(shading_ctx, gpu):
    cfg = S.CONFIGS[2].with_size(512, 64)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    a = gpu_shade(shading_ctx, planes, pc, None, gpu)
    pc_f0 = PassConstants(**{**pc.__dict__, "flags": pc.flags | N.PBR_FLAG_F0_PLANE})
    b = gpu_shade(shading_ctx, planes, pc_f0, None, gpu)
    assert O.bit_equal(a, b).all()


def test_row_band_equals_full_frame(shading_ctx, gpu):
    cfg = S.CONFIGS[3].with_size(640, 200)
    pc = S.scene_pass(cfg)
    shading_ctx.set_pass(pc)
    shading_ctx.set_env_map(S.env_map())
    full = shading_ctx.shade(S.build_gbuffer(cfg, gpu)).cpu().numpy()
    r0, r1 = 37, 151  # not tile aligned
    band = shading_ctx.shade(S.build_gbuffer(cfg, gpu, r0, r1)).cpu().numpy()
    assert O.bit_equal(band, full[r0:r1]).all()


def test_many_lights_cross_chunks(shading_ctx, gpu, env_map):
    rng = np.random.default_rng(5)
    h, w = 40, 100  # partial tiles on both axes
    p = np.zeros((15, h, w), np.float32)
    p[0:3] = rng.uniform(-30, 30, (3, h, w))
    n = rng.normal(size=(3, h, w))
    p[3:6] = n / np.linalg.norm(n, axis=0)
    p[6:15] = rng.uniform(0, 1, (9, h, w))
    nd, npt, ns = 300, 700, 300
    L = np.zeros((nd + npt + ns, 12), np.float32)
    L[:, 0:3] = rng.uniform(0, 30, (len(L), 3))
    L[:, 3] = rng.uniform(1, 64, len(L))
    d = rng.normal(size=(len(L), 3))
    L[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    L[:, 8:11] = rng.uniform(-150, 150, (len(L), 3))
    for flags in (0, N.PBR_FLAG_TILED_CULLING | N.PBR_FLAG_APPLY_AO):
        pc = PassConstants(num_dir_lights=nd, num_point_lights=npt, num_spot_lights=ns,
                           ambient_mode=N.PBR_AMBIENT_IBL_DIFFUSE, flags=flags, lights_array=L)
        got = gpu_shade(shading_ctx, p, pc, env_map, gpu)
        ref = O.shade(list(p), oracle_pass_from_constants(pc), L, env_map, n_threads=8)
        assert report(f"1300 lights flags={flags}", got, ref).max() <= REL_TOL


def test_strided_output_and_empty(shading_ctx, gpu):
    cfg = S.CONFIGS[2].with_size(96, 24)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    shading_ctx.set_pass(pc)
    gb = GBuffer.from_host(planes, gpu)
    big = torch.full((24, 128, 4), -1.0, device=gpu)
    shading_ctx.shade(gb, big)
    ref = gpu_shade(shading_ctx, planes, pc, None, gpu)
    b = big.cpu().numpy()
    assert O.bit_equal(b[:, :96], ref).all()
    assert (b[:, 96:] == -1.0).all()  # nothing written past the row
    empty = GBuffer(torch.zeros((15, 0, 96), device=gpu))
    shading_ctx.shade(empty, torch.empty((0, 96, 4), device=gpu))


def test_error_paths(gpu):
    ctx = ShadingContext(0)
    gb = GBuffer(torch.zeros((15, 8, 8), device=gpu))
    with pytest.raises(N.PbrError) as ei:
        ctx.shade(gb)
    assert ei.value.status == -6  # PBR_ERR_NOT_READY: no pass yet
    ctx.set_pass(PassConstants(ambient_mode=N.PBR_AMBIENT_IBL_DIFFUSE))
    with pytest.raises(N.PbrError) as ei:
        ctx.shade(gb)
    assert ei.value.status == -6  # IBL without an environment map
    with pytest.raises(N.PbrError) as ei:
        ctx.set_pass(PassConstants(flags=1 << 10))
    assert ei.value.status == -1
    with pytest.raises(N.PbrError):
        ctx.set_pass(PassConstants(num_point_lights=N.PBR_MAX_LIGHTS + 1,
                                   lights_array=np.zeros((N.PBR_MAX_LIGHTS + 1, 12), np.float32)))
    ctx.close()


def adversarial_planes(rng, h, w):
    """Values straddling every fast-path window edge: +-0, subnormals, 2^+-20, 2^+-60, 2^+-96,
    huge, inf, NaN, mixed with ordinary scene values."""
    def field(scale, n_special=0.08):
        base = rng.uniform(-scale, scale, (h, w)).astype(np.float32)
        m = rng.uniform(size=(h, w))
        e = rng.integers(-140, 125, (h, w)).astype(np.float64)
        wild = (np.sign(rng.uniform(-1, 1, (h, w))) * rng.uniform(1, 2, (h, w)) * np.exp2(e)).astype(np.float32)
        base = np.where(m < 0.25, wild, base)
        for k, v in enumerate([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -20, 2.0 ** -21, 2.0 ** 20, 1.0, 1e-45]):
            base = np.where((m >= 0.25 + k * n_special / 10) & (m < 0.25 + (k + 1) * n_special / 10),
                            np.float32(v), base)
        return base

    p = np.zeros((15, h, w), np.float32)
    for i in range(3):
        p[i] = field(30.0)
    n = rng.normal(size=(3, h, w))
    n = (n / np.linalg.norm(n, axis=0)).astype(np.float32)
    sel = rng.uniform(size=(h, w)) < 0.3
    for i in range(3):
        p[3 + i] = np.where(sel, field(2.0), n[i])
    for i in range(6, 15):
        p[i] = np.where(rng.uniform(size=(h, w)) < 0.3, field(1.5), rng.uniform(0, 1, (h, w))).astype(np.float32)
    return p


@pytest.mark.parametrize("seed", range(8))
def test_fast_path_is_bit_identical_to_exact_only(seed, shading_ctx, gpu, env_map):
    """The exact fast division/sqrt path must reproduce the compiler's IEEE sequences bit for bit,
    on ordinary and adversarial inputs, for every light type and both ambient modes. Seeds 6-7: scene
    G-buffers (waves on the lean loop) lit by lights outside the per-light window (flag set by
    pbr_set_pass), which must send their pixels to the exact re-pass."""
    rng = np.random.default_rng(100 + seed)
    h, w = 64, 256
    if seed >= 6:
        cfg = S.CONFIGS[[3, 4][seed - 6]].with_size(w, h)
        p, _ = S.fill_gbuffer_host(cfg)
        L = S.scene_pass(cfg).light_array()[:40].copy()
        nd, npt, ns = 4, 30, 6
        L[:nd, 4:7] = rng.normal(size=(nd, 3))
        L[1, 4:7] = (1e-30, 0.5, 0.0)  # directional: a component below 2^-20
        L[2, 4:7] = (20.0, -1.0, 0.0)  # above 16
        L[nd + 3, 8:11] = (2.0 ** 21, 0.0, 1.0)  # point: beyond 2^20
        L[nd + 7, 8:11] = (1e-40, 3.0, 2.0)  # subnormal component
        L[nd + npt + 1, 8:11] = (2.0 ** -25, 1.0, 1.0)
    elif seed < 2:
        cfg = S.CONFIGS[[3, 4][seed]].with_size(w, h)
        p, _ = S.fill_gbuffer_host(cfg)
        pc = S.scene_pass(cfg)
        nd, npt, ns = pc.num_dir_lights, pc.num_point_lights, pc.num_spot_lights
        L = pc.light_array()
    else:
        p = adversarial_planes(rng, h, w)
        nd, npt, ns = 5, 40, 9
        L = np.zeros((nd + npt + ns, 12), np.float32)
        L[:, 0:3] = rng.uniform(0, 50, (len(L), 3))
        L[:, 3] = rng.uniform(0, 64, len(L))
        L[:, 4:7] = rng.normal(size=(len(L), 3))
        L[:, 8:11] = rng.uniform(-40, 40, (len(L), 3))
        wild = rng.uniform(size=(len(L), 3)) < 0.2
        L[:, 8:11] = np.where(wild, (2.0 ** rng.integers(-30, 30, (len(L), 3))).astype(np.float32), L[:, 8:11])
        L[:nd, 4:7] = np.where(rng.uniform(size=(nd, 3)) < 0.3, np.float32(0.0), L[:nd, 4:7])
    for mode in (N.PBR_AMBIENT_CONSTANT, N.PBR_AMBIENT_IBL_DIFFUSE):
        for flags in (0, N.PBR_FLAG_TILED_CULLING | N.PBR_FLAG_F0_PLANE):
            pc = PassConstants(num_dir_lights=nd, num_point_lights=npt, num_spot_lights=ns, ambient_mode=mode,
                               flags=flags, lights_array=L, eye_pos_w=(0.5, 1.0, -5.0))
            fast = gpu_shade(shading_ctx, p, pc, env_map, gpu)
            pc_exact = PassConstants(**{**pc.__dict__, "flags": flags | N.PBR_FLAG_EXACT_ONLY})
            exact = gpu_shade(shading_ctx, p, pc_exact, env_map, gpu)
            eq = O.bit_equal(fast, exact)
            assert eq.all(), f"seed {seed} mode {mode} flags {flags}: {int((~eq).sum())} channels differ"
            if seed >= 2 and mode == 0 and flags == 0:
                ref = O.shade(list(p), O.OraclePass(eye=(0.5, 1.0, -5.0), n_dir=nd, n_point=npt, n_spot=ns),
                              L, None, n_threads=8)
                finite = np.isfinite(ref) & np.isfinite(fast)
                e = O.rel_err(fast[finite], ref[finite])
                print(f"adversarial seed {seed}: max_rel (finite) {e.max():.3g}, "
                      f"nan-pattern agreement {np.mean(np.isnan(fast) == np.isnan(ref)):.6f}")


def test_ibl_near_poles_and_seam(shading_ctx, gpu, env_map):
    """WorldToSkyUV (LightingUtil.hlsl:216-225) is ill-conditioned at the poles (asin' -> inf as
    |N.y| -> 1) and at the atan2 seam (N.z -> 0, N.x < 0): a one-ulp libm difference there moves the
    texel coordinate by up to 1.6e-4 relative, and at grazing N.V the Fresnel kD = 1 - F cancels
    (one ulp of pow(x, 5) -> up to 1e-4). With no lights every transcendental on this path is glibc's
    algorithm (csrc/libm_f32.h), so the frame must be the oracle's bit for bit."""
    rng = np.random.default_rng(77)
    h, w = 64, 512
    n_px = h * w
    eps = (np.sign(rng.uniform(-1, 1, (2, n_px))) * 10.0 ** rng.uniform(-7, -1, (2, n_px)))
    pole = np.stack([eps[0], np.where(rng.uniform(size=n_px) < 0.5, 1.0, -1.0), eps[1]])
    seam = np.stack([-rng.uniform(0.05, 1, n_px), rng.uniform(-1, 1, n_px), eps[1]])
    rand = rng.normal(size=(3, n_px))
    pick = rng.integers(0, 3, n_px)
    n = np.where(pick == 0, pole, np.where(pick == 1, seam, rand))
    n = (n / np.linalg.norm(n, axis=0)).astype(np.float32)
    n[:, :64] = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [-1.0, 0.0, -0.0]] * 16,
                         np.float32).T  # exact poles and the seam itself, both signs of zero
    p = np.zeros((15, h, w), np.float32)
    p[0:3] = rng.uniform(-5, 5, (3, h, w))
    p[3:6] = n.reshape(3, h, w)
    p[6:15] = rng.uniform(0, 1, (9, h, w))
    for flags in (0, N.PBR_FLAG_APPLY_AO):
        pc = PassConstants(ambient_mode=N.PBR_AMBIENT_IBL_DIFFUSE, flags=flags, eye_pos_w=(0.0, 0.0, -10.0))
        got = gpu_shade(shading_ctx, p, pc, env_map, gpu)
        ref = O.shade(list(p), oracle_pass_from_constants(pc), None, env_map, n_threads=8)
        report(f"IBL poles/seam flags={flags}", got, ref)
        assert O.bit_equal(got, ref).all()


@pytest.mark.parametrize("flags", [0, N.PBR_FLAG_FAITHFUL])
def test_range_cut_at_100_on_gpu(flags, shading_ctx, gpu):
    """`if (d > 100) return 0` (LightingUtil.hlsl:131) through the kernel's exact 0/1 range factor
    (pbr_device_math_x2.h, in_range01): pixels 100 + k * 2^-17 from the light, k in [-8, 8), straddle the
    cut. Exact mode: bit-identical to the oracle; faithful mode: within 1e-5, and every pixel the oracle
    leaves unlit equals the no-light frame of the same mode."""
    w = 16
    p = np.zeros((O.NUM_PLANES, 1, w), np.float32)
    p[0, 0, :] = -np.arange(-8, 8, dtype=np.float32) * np.float32(2.0 ** -17)  # l.x = 100 + k ulp(100)
    p[3] = 1.0  # N faces +x, towards the light
    p[6:9] = 0.5
    p[10] = 0.5
    p[11] = 1.0
    lights = np.array([[1e4, 1e4, 1e4, 64.0, 0, 0, 1, 0, 100.0, 0, 0, 0]], np.float32)

    def pass_with(n_point):
        return PassConstants(eye_pos_w=(50.0, 0.0, -5.0), ambient_light=(0.03, 0.03, 0.03), num_point_lights=n_point,
                             flags=flags, lights_array=lights if n_point else None)

    pc = pass_with(1)
    got = gpu_shade(shading_ctx, p, pc, None, gpu)
    ref = O.shade(list(p), oracle_pass_from_constants(pc), pc.light_array())
    base_ref = O.shade(list(p), oracle_pass_from_constants(pass_with(0)), None)
    base_gpu = gpu_shade(shading_ctx, p, pass_with(0), None, gpu)
    unlit = np.all(ref[0] == base_ref[0], axis=-1)
    assert 0 < unlit.sum() < w  # both sides of the cut are present
    if flags == 0:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    else:
        assert O.rel_err(got, ref).max() <= REL_TOL
    assert np.array_equal(got[0, unlit].view(np.uint32), base_gpu[0, unlit].view(np.uint32))
    assert not np.any(np.all(got[0, ~unlit] == base_gpu[0, ~unlit], axis=-1))


SPOT_ADVERSARIAL = {  # name -> (SpotPower, Direction): cone factors the light window cannot see
    "negative_power_c0": (-2.0, (1.0, 0.0, 0.0)),      # pow(0, -2) = +inf
    "nan_power": (float("nan"), (-0.5, 0.0, 0.0)),     # pow(0.5, NaN) = NaN
    "non_unit_dir": (200.0, (-2.0, 0.0, 0.0)),         # pow(2, 200) = +inf in fp32
    "unit_sharp": (64.0, (-1.0, 0.0, 0.0)),            # a well-behaved cone, for contrast
}


@pytest.mark.parametrize("flags", [0, N.PBR_FLAG_FAITHFUL])
@pytest.mark.parametrize("case", sorted(SPOT_ADVERSARIAL))
def test_spot_range_cut_with_nonfinite_cone(case, flags, shading_ctx, gpu):
    """ComputeSpotLight returns 0 beyond d > 100 *before* its pow (LightingUtil.hlsl:154, 163), so a cone
    factor that is inf or NaN must not leak into out-of-range pixels (inf * 0 = NaN). Pixels straddle the cut
    at 100 + k * 2^-17; exact mode must be the oracle's bit for bit, faithful mode within 1e-5 (NaN == NaN),
    and every pixel the oracle leaves unlit must equal the no-light frame."""
    power, direction = SPOT_ADVERSARIAL[case]
    w = 16
    p = np.zeros((O.NUM_PLANES, 1, w), np.float32)
    p[0, 0, :] = -np.arange(-8, 8, dtype=np.float32) * np.float32(2.0 ** -17)
    p[3] = 1.0
    p[6:9] = 0.5
    p[10] = 0.5
    p[11] = 1.0
    lights = np.array([[1e3, 1e3, 1e3, power, *direction, 0, 100.0, 0, 0, 0]], np.float32)

    def pass_with(n_spot):
        return PassConstants(eye_pos_w=(50.0, 0.0, -5.0), ambient_light=(0.03, 0.03, 0.03), num_spot_lights=n_spot,
                             flags=flags, lights_array=lights if n_spot else None)

    pc = pass_with(1)
    got = gpu_shade(shading_ctx, p, pc, None, gpu)
    ref = O.shade(list(p), oracle_pass_from_constants(pc), pc.light_array())
    base = gpu_shade(shading_ctx, p, pass_with(0), None, gpu)
    base_ref = O.shade(list(p), oracle_pass_from_constants(pass_with(0)), None)
    unlit = np.all(O.bit_equal(ref[0], base_ref[0]), axis=-1)
    assert 0 < unlit.sum() < w
    if flags == 0:
        assert O.bit_equal(got, ref).all()
    else:
        assert O.rel_err(got, ref).max() <= REL_TOL
    assert O.bit_equal(got[0, unlit], base[0, unlit]).all()


def test_tensors_on_another_device_are_rejected(shading_ctx, gpu):
    """renderer.ShadingContext hands raw pointers to the kernel: planes / out / coverage that do not live on
    the context's device are refused before the C ABI is called."""
    shading_ctx.set_pass(PassConstants())
    host = GBuffer(torch.zeros((15, 8, 8)))
    with pytest.raises(ValueError):
        shading_ctx.shade(host)
    dev = GBuffer(torch.zeros((15, 8, 8), device=gpu))
    with pytest.raises(ValueError):
        shading_ctx.shade(dev, torch.empty((8, 8, 4)))
    with pytest.raises(ValueError):
        shading_ctx.shade_frame(dev, coverage=torch.ones((8, 8), dtype=torch.uint8))


@pytest.mark.parametrize("mode", ["faithful", "exact"])
def test_config5_full_frame_rank_bands_and_oracle_rows(mode, shading_ctx, gpu):
    """BASELINE config 5 at its full size on one GPU: the whole 8192 x 8192 frame (4 GB of planes in HBM); each of
    the eight 8192 x 1024 rank bands (dist.band_rows, N = 8) shaded on its own through the band's pointers, as a
    rank of the multi-GPU run does, must equal the same rows of the whole frame bit for bit; and rows on and
    around every band edge plus a row inside each band must match the CPU oracle within the north-star 1e-5 (the
    exact mode also >= 99.999% of channels bit-identical; measured: one channel in 1.3 M differs, by 6e-8)."""
    from physically_based_renderer_amd import dist as D

    cfg = S.CONFIGS[5]
    planes_host = torch.empty((N.NUM_PLANES, cfg.height, cfg.width), dtype=torch.float32, pin_memory=True)
    S.fill_gbuffer_host(cfg, out=planes_host.numpy(), n_threads=16)
    planes = planes_host.numpy()
    gb = GBuffer(planes_host.to(gpu))
    pc = S.scene_pass(cfg)
    pc.flags = (int(pc.flags) & ~N.PBR_FLAG_FAITHFUL) | (N.PBR_FLAG_FAITHFUL if mode == "faithful" else 0)
    env = S.env_map()
    shading_ctx.set_pass(pc)
    shading_ctx.set_env_map(env)
    whole = shading_ctx.shade(gb)
    band_out = torch.empty((1024, cfg.width, 4), dtype=torch.float32, device=gpu)
    rows = []
    for b in D.all_bands(cfg.height, 8):
        assert b.rows == 1024
        shading_ctx.shade(gb.rows(b.row_begin, b.row_end), band_out)
        assert torch.equal(band_out.view(torch.int32), whole[b.row_begin:b.row_end].view(torch.int32)), b
        rows += [b.row_begin, b.row_begin + 1, b.row_begin + 517, b.row_end - 2, b.row_end - 1]
    got = whole[rows].cpu().numpy()
    del gb, whole
    torch.cuda.synchronize()
    ref = O.shade(list(np.ascontiguousarray(planes[:, rows])), oracle_pass_from_constants(pc), pc.light_array(),
                  env, n_threads=16)
    e = report(f"cfg5 8192x8192 {mode}: {len(rows)} rows", got, ref)
    assert e.max() <= REL_TOL
    if mode == "exact":  # bit-identical but for the per-light x^5 residue (<= 1.2e-6 of a term)
        assert O.bit_equal(got, ref).mean() >= 0.99999


def test_row_interleaved_gbuffer_layout(shading_ctx, gpu, env_map):
    """Planes interleaved by row ((H, 15, W) memory viewed as (15, H, W)) shade to the same bits as the
    plane-major layout: the kernel follows the plane bases and row stride it is given."""
    cfg = S.CONFIGS[3].with_size(256, 32)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    shading_ctx.set_pass(pc)
    shading_ctx.set_env_map(env_map)
    want = shading_ctx.shade(GBuffer.from_host(planes, gpu))
    inter = torch.from_numpy(np.ascontiguousarray(planes.transpose(1, 0, 2))).to(gpu).permute(1, 0, 2)
    got = shading_ctx.shade(GBuffer(inter))
    torch.cuda.synchronize()
    assert O.bit_equal(got.cpu().numpy(), want.cpu().numpy()).all()
