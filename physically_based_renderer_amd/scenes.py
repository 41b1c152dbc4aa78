"""The BASELINE.json configurations as G-buffer scenes (host fill through ``pbr_gbuffer_fill``).

    1  256x256,   1 point light, rustediron sphere (CPU plumbing case)
    2  1920x1080, 8 point lights, rustediron material
    3  3840x2160, 64 point lights + diffuse IBL (Chelsea_Stairs)      <- the bench workload
    4  3840x2160, 256 point lights, tiled light culling, *_1K materials, F0 plane
    5  8192x8192, 64 point lights + IBL, row bands across GPUs + RCCL gather

plus REFERENCE_SCENE: the reference's own 58-sphere scene under its 4 directional lights,
ray-cast from a camera, with background pixels for the sky pass.

All inputs are synthetic but deterministic functions of (global pixel, seed); see DESIGN.md.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from . import _native as N
from . import envmap
from .renderer import Attributes, Draw, GBuffer, Material, Mesh, PassConstants, View

ASSET_DIR = envmap.ASSET_DIR


@dataclass(frozen=True)
class SceneConfig:
    cid: int
    name: str
    kind: int
    width: int
    height: int
    n_lights: int
    ambient_mode: int
    flags: int
    seed: int
    camera: Optional[tuple] = None  # (eye xyz, target xyz, fov_y) for the reference scene; None = its default

    def with_size(self, width: int, height: int) -> "SceneConfig":
        return replace(self, width=width, height=height)

    def with_camera(self, eye, target, fov_y: float = float(np.pi / 4)) -> "SceneConfig":
        return replace(self, camera=(tuple(eye), tuple(target), float(fov_y)))


CONFIGS = {
    1: SceneConfig(1, "cfg1_256x256_sphere_rustediron_1pt", N.PBR_SCENE_SPHERE_RUSTEDIRON, 256, 256, 1,
                   N.PBR_AMBIENT_CONSTANT, 0, 0x5EED0001),
    2: SceneConfig(2, "cfg2_1920x1080_rustediron_8pt", N.PBR_SCENE_RANDOM_COVERED, 1920, 1080, 8,
                   N.PBR_AMBIENT_CONSTANT, 0, 0x5EED0002),
    3: SceneConfig(3, "cfg3_3840x2160_64pt_ibl_chelsea", N.PBR_SCENE_RANDOM_COVERED, 3840, 2160, 64,
                   N.PBR_AMBIENT_IBL_DIFFUSE, 0, 0x5EED0003),
    4: SceneConfig(4, "cfg4_3840x2160_256pt_tiled_materials", N.PBR_SCENE_PLANE_MATERIALS, 3840, 2160, 256,
                   N.PBR_AMBIENT_CONSTANT, N.PBR_FLAG_F0_PLANE | N.PBR_FLAG_TILED_CULLING, 0x5EED0004),
    5: SceneConfig(5, "cfg5_8192x8192_64pt_ibl_rowbands", N.PBR_SCENE_RANDOM_COVERED, 8192, 8192, 64,
                   N.PBR_AMBIENT_IBL_DIFFUSE, 0, 0x5EED0005),
}


# The reference scene (PBRApp.cpp:964-973, 1016-1068), F0 resolved into the plane by the fill. Its
# default camera is BuildCamera's (eye (0, 0, -5) looking down +z, PBRApp.cpp:652-659); OVERVIEW_CAMERA
# backs off to show all 58 spheres.
REFERENCE_SCENE = SceneConfig(0, "reference_58_spheres", N.PBR_SCENE_REFERENCE_SPHERES, 1280, 720, 4,
                              N.PBR_AMBIENT_CONSTANT, N.PBR_FLAG_F0_PLANE, 0x5EED0000)
OVERVIEW_CAMERA = ((0.0, -7.0, -30.0), (0.0, -7.0, 0.0), float(np.pi / 4))


class Assets:
    """Texture tiles committed under assets/ (tools/make_assets.py), kept alive for the C fill."""

    _instance: Optional["Assets"] = None

    def __init__(self):
        rust = np.load(os.path.join(ASSET_DIR, "rustediron_256.npz"))
        mats = np.load(os.path.join(ASSET_DIR, "materials_1k_64.npz"))
        self.rust_metallic = np.ascontiguousarray(rust["metallic"], np.uint8)
        self.rust_roughness = np.ascontiguousarray(rust["roughness"], np.uint8)
        self.mat_albedo = np.ascontiguousarray(mats["albedo"], np.uint8)
        self.mat_specular = np.ascontiguousarray(mats["specular"], np.uint8)
        self.mat_roughness = np.ascontiguousarray(mats["roughness"], np.uint8)
        self.mat_metallic = np.ascontiguousarray(mats["metallic"], np.uint8)
        self.mat_has_metallic = np.ascontiguousarray(mats["has_metallic"], np.uint8)
        self.mat_normal = np.ascontiguousarray(mats["normal"], np.uint8)
        self.material_names = [str(s) for s in mats["names"]]
        self.env = envmap.load_chelsea_stairs_env()
        a = N.SceneAssets()
        a.rust_metallic = self.rust_metallic.ctypes.data
        a.rust_roughness = self.rust_roughness.ctypes.data
        a.rust_size = self.rust_metallic.shape[0]
        a.mat_albedo = self.mat_albedo.ctypes.data
        a.mat_specular = self.mat_specular.ctypes.data
        a.mat_roughness = self.mat_roughness.ctypes.data
        a.mat_metallic = self.mat_metallic.ctypes.data
        a.mat_has_metallic = self.mat_has_metallic.ctypes.data
        a.mat_normal = self.mat_normal.ctypes.data
        a.num_materials = self.mat_albedo.shape[0]
        a.mat_size = self.mat_albedo.shape[1]
        self.c = a

    @classmethod
    def get(cls) -> "Assets":
        if cls._instance is None:
            cls._instance = Assets()
        return cls._instance


def _scene_desc(cfg: SceneConfig, assets: Assets) -> N.SceneDesc:
    d = N.SceneDesc()
    d.kind, d.width, d.height, d.seed = cfg.kind, cfg.width, cfg.height, cfg.seed
    d.assets = ctypes.pointer(assets.c)
    if cfg.camera is not None:
        cam = N.Camera()
        cam.eye[:] = [float(v) for v in cfg.camera[0]]
        cam.target[:] = [float(v) for v in cfg.camera[1]]
        cam.fov_y = float(cfg.camera[2])
        d._camera_keep = cam  # the pointer below must not outlive it
        d.camera = ctypes.pointer(cam)
    return d


def fill_gbuffer_host(cfg: SceneConfig, row_begin: int = 0, row_end: Optional[int] = None,
                      out: Optional[np.ndarray] = None, n_threads: int = 0):
    """Host planes (15, rows, width) for rows [row_begin, row_end); returns (planes, covered_px)."""
    assets = Assets.get()
    row_end = cfg.height if row_end is None else row_end
    rows = row_end - row_begin
    if rows < 0 or row_begin < 0 or row_end > cfg.height:
        raise N.PbrError(-1, "pbr_gbuffer_fill", f"rows [{row_begin}, {row_end}) outside [0, {cfg.height})")
    if out is None:
        out = np.empty((N.NUM_PLANES, rows, cfg.width), np.float32)
    if rows == 0:
        return out, 0
    assert out.dtype == np.float32 and out.shape[0] == N.NUM_PLANES and out.shape[1] >= rows
    assert out.strides[2] == 4 and out.strides[0] % 4 == 0
    ptrs = (ctypes.c_void_p * N.NUM_PLANES)(*[out[i].ctypes.data for i in range(N.NUM_PLANES)])
    nt = n_threads or min(16, os.cpu_count() or 1)
    d = _scene_desc(cfg, assets)
    covered = N.lib().pbr_gbuffer_fill(ctypes.byref(d), row_begin, row_end, ptrs, out.strides[1] // 4, nt)
    N.check(int(covered), "pbr_gbuffer_fill")
    return out, int(covered)


def fill_gbuffer_host_coverage(cfg: SceneConfig, row_begin: int = 0, row_end: Optional[int] = None,
                               n_threads: int = 0):
    """(planes (15, rows, width) float32, coverage (rows, width) uint8: 1 geometry / 0 background)."""
    assets = Assets.get()
    row_end = cfg.height if row_end is None else row_end
    rows = row_end - row_begin
    if rows < 0 or row_begin < 0 or row_end > cfg.height:
        raise N.PbrError(-1, "pbr_gbuffer_fill_coverage", f"rows [{row_begin}, {row_end}) outside [0, {cfg.height})")
    out = np.empty((N.NUM_PLANES, rows, cfg.width), np.float32)
    cov = np.empty((rows, cfg.width), np.uint8)
    if rows == 0:
        return out, cov
    ptrs = (ctypes.c_void_p * N.NUM_PLANES)(*[out[i].ctypes.data for i in range(N.NUM_PLANES)])
    nt = n_threads or min(16, os.cpu_count() or 1)
    d = _scene_desc(cfg, assets)
    r = N.lib().pbr_gbuffer_fill_coverage(ctypes.byref(d), row_begin, row_end, ptrs, cfg.width, cov.ctypes.data,
                                          cfg.width, nt)
    N.check(int(r), "pbr_gbuffer_fill_coverage")
    return out, cov


def scene_pass(cfg: SceneConfig) -> PassConstants:
    """Pass constants + light list of a config (pbr_scene_pass), with its ambient mode and flags."""
    assets = Assets.get()
    d = _scene_desc(cfg, assets)
    lights = (N.Light * max(cfg.n_lights, 1))()
    p = N.PassDesc()
    N.check(N.lib().pbr_scene_pass(ctypes.byref(d), cfg.n_lights, lights, ctypes.byref(p)), "pbr_scene_pass")
    arr = np.frombuffer(lights, dtype=np.float32).reshape(-1, 12)[: cfg.n_lights].copy()
    pc = PassConstants.from_c(p, arr)
    pc.ambient_mode = cfg.ambient_mode
    pc.flags = int(pc.flags) | cfg.flags
    return pc


def build_gbuffer(cfg: SceneConfig, device, row_begin: int = 0, row_end: Optional[int] = None,
                  n_threads: int = 0) -> GBuffer:
    """Fill rows on the host (pinned staging) and upload them; returns the device G-buffer."""
    import torch

    row_end = cfg.height if row_end is None else row_end
    rows = row_end - row_begin
    staging = torch.empty((N.NUM_PLANES, rows, cfg.width), dtype=torch.float32, pin_memory=True)
    fill_gbuffer_host(cfg, row_begin, row_end, out=staging.numpy(), n_threads=n_threads)
    dev = staging.to(device, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    return GBuffer(dev)


def _tile_materials(assets: Assets, textures: list) -> list:
    """The seven *_1K sets (PBRApp.cpp:1270-1463) as textured materials: diffuse, specular, roughness and normal
    maps, a metalness map where the set has one (else g_Metallic = 0). Their maps are appended to ``textures``."""
    mats = []
    for m in range(assets.mat_albedo.shape[0]):
        base = len(textures)
        textures += [assets.mat_albedo[m], assets.mat_specular[m], assets.mat_metallic[m], assets.mat_roughness[m],
                     assets.mat_normal[m]]
        has_metal = bool(assets.mat_has_metallic[m])
        flags = (N.PBR_MAT_DIFFUSE_TEXTURE | N.PBR_MAT_SPECULAR_TEXTURE | N.PBR_MAT_ROUGHNESS_TEXTURE |
                 N.PBR_MAT_NORMAL_TEXTURE | (N.PBR_MAT_METALLIC_TEXTURE if has_metal else 0))
        mats.append(Material(metallic=0.0, flags=flags,
                             tex=(base, base + 1, base + 2 if has_metal else -1, base + 3, base + 4, -1)))
    return mats


def scene_materials(cfg: SceneConfig):
    """(materials, textures) for :meth:`ShadingContext.set_materials`, indexed by the material ids of
    :func:`fill_attributes_host`: config 4's seven textured sets; the reference scene's 58 spheres (49 red
    constants, PBRApp.cpp:964-973; rusted iron with its metallic and roughness maps; the copper constants; the
    seven tiles, PBRApp.cpp:1016-1068)."""
    assets = Assets.get()
    textures: list = []
    if cfg.kind == N.PBR_SCENE_PLANE_MATERIALS:
        return _tile_materials(assets, textures), textures
    if cfg.kind != N.PBR_SCENE_REFERENCE_SPHERES:
        raise ValueError("scene_materials: config 4 and the reference scene only")
    f = np.float32
    mats = [Material(diffuse_albedo=(1.0, 0.0, 0.0), roughness=float(f(i % 7) / f(6.0)),
                     metallic=float(f(1.0) - f(i // 7) / f(6.0))) for i in range(49)]
    textures += [assets.rust_metallic, assets.rust_roughness]
    mats.append(Material(diffuse_albedo=(0.5, 0.5, 0.5), tex=(-1, -1, 0, 1, -1, -1),
                         flags=N.PBR_MAT_METALLIC_TEXTURE | N.PBR_MAT_ROUGHNESS_TEXTURE))
    mats.append(Material(diffuse_albedo=(0.95, 0.64, 0.54), metallic=1.0, roughness=0.35))
    mats += _tile_materials(assets, textures)
    return mats, textures


def fill_attributes_host(cfg: SceneConfig, row_begin: int = 0, row_end: Optional[int] = None, n_threads: int = 0):
    """Host attribute planes (14, rows, width) float32 and material ids (rows, width) uint16 for rows
    [row_begin, row_end) (pbr_attributes_fill): the interpolated VertexOut the G-buffer fill consumes in place."""
    assets = Assets.get()
    row_end = cfg.height if row_end is None else row_end
    rows = row_end - row_begin
    if rows < 0 or row_begin < 0 or row_end > cfg.height:
        raise N.PbrError(-1, "pbr_attributes_fill", f"rows [{row_begin}, {row_end}) outside [0, {cfg.height})")
    out = np.empty((N.NUM_ATTRIBUTE_PLANES, rows, cfg.width), np.float32)
    mat = np.empty((rows, cfg.width), np.uint16)
    if rows == 0:
        return out, mat
    ptrs = (ctypes.c_void_p * N.NUM_ATTRIBUTE_PLANES)(*[out[i].ctypes.data for i in range(N.NUM_ATTRIBUTE_PLANES)])
    nt = n_threads or min(16, os.cpu_count() or 1)
    d = _scene_desc(cfg, assets)
    r = N.lib().pbr_attributes_fill(ctypes.byref(d), row_begin, row_end, ptrs, mat.ctypes.data, cfg.width, nt)
    N.check(int(r), "pbr_attributes_fill")
    return out, mat


def build_attributes(cfg: SceneConfig, device, row_begin: int = 0, row_end: Optional[int] = None,
                     n_threads: int = 0) -> Attributes:
    """Fill rows of attributes on the host and upload them; :meth:`ShadingContext.resolve` makes the G-buffer."""
    planes, mat = fill_attributes_host(cfg, row_begin, row_end, n_threads)
    return Attributes.from_host(planes, mat, device)


# ---- Geometry for the device rasteriser (ShadingContext.rasterize) ------------------------------------

def uv_sphere(slices: int = 64, stacks: int = 32, radius: float = 1.0) -> Mesh:
    """A UV sphere in the frame the analytic fill uses: theta = atan2(z, x) in [0, 2 pi], phi the
    angle from +y, P = r (sin phi cos theta, cos phi, sin phi sin theta); N = P / r, UV = (theta / 2 pi, phi / pi),
    T = dP/dtheta = (-P.z, 0, P.x), B = cross(N, T). (stacks + 1) rings of (slices + 1) vertices (the seam column is
    doubled so that u runs to 1); the pole quads keep their one triangle with area. Triangles are wound so that the
    outside is the front face under D3D's default (clockwise seen from outside, left-handed)."""
    if slices < 3 or stacks < 2:
        raise ValueError("uv_sphere: at least 3 slices and 2 stacks")
    j, i = np.meshgrid(np.arange(stacks + 1), np.arange(slices + 1), indexing="ij")
    theta, phi = 2.0 * np.pi * i / slices, np.pi * j / stacks
    n = np.stack([np.sin(phi) * np.cos(theta), np.cos(phi), np.sin(phi) * np.sin(theta)], -1)
    p = radius * n
    t = np.stack([-p[..., 2], np.zeros_like(phi), p[..., 0]], -1)
    b = np.cross(n, t)
    uv = np.stack([i / slices, j / stacks], -1)
    vertices = np.concatenate([p, n, t, b, uv], -1).reshape(-1, 14).astype(np.float32)
    ring = slices + 1
    tris = []
    for r in range(stacks):
        for c in range(slices):
            v00, v01, v10, v11 = r * ring + c, r * ring + c + 1, (r + 1) * ring + c, (r + 1) * ring + c + 1
            if r != 0:  # the top ring is one point: v00 == v01 in space
                tris.append((v00, v01, v10))
            if r != stacks - 1:  # so is the bottom ring
                tris.append((v01, v11, v10))
    idx = np.array(tris, np.uint32)
    # orient: cross(e1, e2) along the outward normal is the front face in a left-handed frame
    pos = vertices[:, 0:3].astype(np.float64)
    e1, e2 = pos[idx[:, 1]] - pos[idx[:, 0]], pos[idx[:, 2]] - pos[idx[:, 0]]
    flip = np.einsum("ij,ij->i", np.cross(e1, e2), pos[idx].sum(1)) < 0
    idx[flip] = idx[flip][:, [0, 2, 1]]
    return Mesh(vertices, idx.reshape(-1))


def translation(x: float, y: float, z: float) -> tuple:
    """A row-vector world matrix (the translation in the last row)."""
    m = np.eye(4, dtype=np.float32)
    m[3, 0:3] = (x, y, z)
    return tuple(m.ravel().tolist())


def look_at_view(eye, target, fov_y: float, width: int, height: int, near: float = 0.1, far: float = 100.0) -> View:
    """The :class:`View` of a left-handed look-at camera with world up (0, 1, 0) and a D3D perspective projection
    (depth 0 at ``near``, 1 at ``far``; BuildCamera's 0.1 and 100, PBRApp.cpp:654), row vectors: ``view_proj`` =
    view x projection, and the background basis of the same camera as pbr_attributes_fill builds it."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.array([f[2], 0.0, -f[0]])  # cross(up, forward)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    t, aspect = np.tan(0.5 * fov_y), width / height
    view = np.eye(4)
    view[0:3, 0], view[0:3, 1], view[0:3, 2] = r, u, f
    view[3, 0:3] = (-r @ eye, -u @ eye, -f @ eye)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = 1.0 / (aspect * t), 1.0 / t
    proj[2, 2], proj[2, 3], proj[3, 2] = far / (far - near), 1.0, -near * far / (far - near)
    vp = (view @ proj).astype(np.float32)
    return View(view_proj=tuple(vp.ravel().tolist()), width=int(width), height=int(height),
                eye=tuple(eye.astype(np.float32).tolist()), bg_right=tuple((r * t * aspect).astype(np.float32).tolist()),
                bg_up=tuple((u * t).astype(np.float32).tolist()), bg_forward=tuple(f.astype(np.float32).tolist()))


def reference_sphere_centres() -> list:
    """(x, y) of the reference scene's 58 unit spheres on z = 0, in material order (scene_materials): the 7 x 7 red
    grid (PBRApp.cpp:964-973, 1016-1022), then rust, copper and the seven tiles on y = 0 (PBRApp.cpp:1023-1068)."""
    grid = [((i % 7) * 2.5 - 7.5, -(i // 7) * 2.5 - 2.5) for i in range(49)]
    return grid + [(x, 0.0) for x in (0.0, -2.5, -5.0, -7.5, -10.0, 2.5, 5.0, 7.5, 10.0)]


def reference_scene_draws(slices: int = 64, stacks: int = 32):
    """(meshes, draws) of the reference scene for :meth:`ShadingContext.rasterize`: one UV sphere, 58 draws, draw i
    with material i. The facets are not the analytic spheres of pbr_attributes_fill."""
    draws = [Draw(mesh=0, material=i, world=translation(x, y, 0.0)) for i, (x, y) in enumerate(reference_sphere_centres())]
    return [uv_sphere(slices, stacks)], draws


def reference_scene_view(cfg: SceneConfig) -> View:
    """The :class:`View` of a reference-scene config's camera (None = BuildCamera's default)."""
    eye, target, fov = cfg.camera or ((0.0, 0.0, -5.0), (0.0, 0.0, 0.0), float(np.pi / 4))
    return look_at_view(eye, target, fov, cfg.width, cfg.height)


def env_map() -> np.ndarray:
    return Assets.get().env
