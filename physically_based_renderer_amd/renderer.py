"""Host-side mirror of the reference's shading interface, over the C ABI of libpbrshade.so.

The reference drives its pixel shader through D3D12: per-frame constants in ``PassConstants``
(``Source/App/FrameResource.h:19-44``) holding ``Light Lights[MaxLights]`` (``d3dUtil.h:144-152``),
per-material constants (``Material.h:10-29``), then ``DrawIndexedInstanced`` (``PBRApp.cpp:1133``).
Here the same roles are:

  =====================================  ==============================================
  reference                              this module
  =====================================  ==============================================
  ``Light`` (strength/spotpower/dir/pos)  :class:`Light` (same fields, same defaults)
  ``PassConstants`` + light-count defines :class:`PassConstants`
  ``UpdateMainPassCB`` / ``CopyData``     :meth:`ShadingContext.set_pass`
  sky_env SRV (t1)                        :meth:`ShadingContext.set_env_map`
  sky_box SRV (t0) + Skybox.hlsl pass     :meth:`ShadingContext.set_sky_map`, ``coverage``
  ``DrawIndexedInstanced(PS)``            :meth:`ShadingContext.shade`
  PS + sky dome into the R8G8B8A8 target  :meth:`ShadingContext.shade_frame`
  =====================================  ==============================================

PyTorch is used only for device memory and streams. Every shading call runs the gfx950 kernel;
there is no CPU path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N


@dataclass
class Light:
    """``struct Light`` (LightingUtil.hlsl:9-17) with the C++ defaults of d3dUtil.h:144-152."""
    strength: Sequence[float] = (0.5, 0.5, 0.5)
    spot_power: float = 64.0
    direction: Sequence[float] = (0.0, -1.0, 0.0)
    position: Sequence[float] = (0.0, 0.0, 0.0)

    def to_c(self) -> N.Light:
        c = N.Light()
        c.strength[:] = [float(v) for v in self.strength]
        c.spot_power = float(self.spot_power)
        c.direction[:] = [float(v) for v in self.direction]
        c.position[:] = [float(v) for v in self.position]
        return c


@dataclass
class PassConstants:
    """Shading subset of cbPass / cbMaterial (Core.hlsl:35-81) plus the NUM_*_LIGHTS defines.

    ``lights`` are ordered directional, point, spot (ComputeLighting, LightingUtil.hlsl:176-199);
    alternatively pass ``lights_array`` as an (n, 12) float32 array in the 48-byte layout.
    """
    eye_pos_w: Sequence[float] = (0.0, 0.0, -5.0)
    ambient_light: Sequence[float] = (0.03, 0.03, 0.03)
    fresnel_r0: Sequence[float] = (0.04, 0.04, 0.04)
    opacity: float = 1.0
    num_dir_lights: int = 0
    num_point_lights: int = 0
    num_spot_lights: int = 0
    ambient_mode: int = N.PBR_AMBIENT_CONSTANT
    flags: int = 0
    lights: Sequence[Light] = field(default_factory=list)
    lights_array: Optional[np.ndarray] = None

    @property
    def num_lights(self) -> int:
        return self.num_dir_lights + self.num_point_lights + self.num_spot_lights

    def light_array(self) -> np.ndarray:
        if self.lights_array is not None:
            arr = np.ascontiguousarray(self.lights_array, dtype=np.float32).reshape(-1, 12)
        else:
            arr = np.zeros((len(self.lights), 12), np.float32)
            for i, L in enumerate(self.lights):
                arr[i, 0:3] = L.strength
                arr[i, 3] = L.spot_power
                arr[i, 4:7] = L.direction
                arr[i, 8:11] = L.position
        if arr.shape[0] < self.num_lights:
            raise ValueError(f"{self.num_lights} lights declared, {arr.shape[0]} given")
        return arr

    def to_c(self, keepalive: list) -> N.PassDesc:
        p = N.PassDesc()
        p.eye_pos_w[:] = [float(v) for v in self.eye_pos_w]
        p.ambient_light[:] = [float(v) for v in self.ambient_light]
        p.fresnel_r0[:] = [float(v) for v in self.fresnel_r0]
        p.opacity = float(self.opacity)
        p.num_dir_lights = int(self.num_dir_lights)
        p.num_point_lights = int(self.num_point_lights)
        p.num_spot_lights = int(self.num_spot_lights)
        p.ambient_mode = int(self.ambient_mode)
        p.flags = int(self.flags)
        arr = self.light_array()
        keepalive.append(arr)
        p.lights = ctypes.cast(arr.ctypes.data, ctypes.POINTER(N.Light)) if arr.size else None
        return p

    @classmethod
    def from_c(cls, p: N.PassDesc, lights: np.ndarray) -> "PassConstants":
        return cls(eye_pos_w=tuple(p.eye_pos_w), ambient_light=tuple(p.ambient_light),
                   fresnel_r0=tuple(p.fresnel_r0), opacity=p.opacity, num_dir_lights=p.num_dir_lights,
                   num_point_lights=p.num_point_lights, num_spot_lights=p.num_spot_lights,
                   ambient_mode=p.ambient_mode, flags=p.flags, lights_array=np.array(lights, np.float32))


class GBuffer:
    """Structure-of-arrays G-buffer: one (15, H, row_stride) fp32 tensor, plane order
    pos xyz, normal xyz, albedo rgb, metallic, roughness, ao, f0 rgb (pbr_gbuffer_soa), and, for the
    ALPHA_TEST permutation (PBR_FLAG_ALPHA_TEST), an (H, row_stride) opacity plane with the same row stride."""

    def __init__(self, planes: torch.Tensor, width: Optional[int] = None, opacity: Optional[torch.Tensor] = None):
        if planes.dim() != 3 or planes.shape[0] != N.NUM_PLANES or planes.dtype != torch.float32:
            raise ValueError("planes must be a (15, H, W) float32 tensor")
        if planes.stride(2) != 1:
            raise ValueError("planes rows must be contiguous")
        if opacity is not None and (opacity.dim() != 2 or opacity.dtype != torch.float32 or
                                    opacity.shape[0] != planes.shape[1] or opacity.shape[1] < planes.shape[2] or
                                    opacity.stride(1) != 1 or opacity.stride(0) != planes.stride(1) or
                                    opacity.device != planes.device):
            raise ValueError("opacity must be an (H, W) float32 plane with the planes' row stride and device")
        self.planes = planes
        self.opacity = opacity
        self.height = planes.shape[1]
        self.width = planes.shape[2] if width is None else width
        self.row_stride = planes.stride(1)

    @classmethod
    def from_host(cls, planes: np.ndarray, device, opacity: Optional[np.ndarray] = None) -> "GBuffer":
        t = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32))
        o = None if opacity is None else torch.from_numpy(np.ascontiguousarray(opacity, dtype=np.float32)).to(device)
        return cls(t.to(device), opacity=o)

    def rows(self, r0: int, r1: int) -> "GBuffer":
        """A row band (a view: shading it writes only those rows)."""
        return GBuffer(self.planes[:, r0:r1, :], self.width, None if self.opacity is None else self.opacity[r0:r1])

    def to_c(self) -> N.GBufferSoA:
        g = N.GBufferSoA()
        base = self.planes.data_ptr()
        ps = self.planes.stride(0) * 4
        ptr = [base + i * ps for i in range(N.NUM_PLANES)]
        g.pos_w[:] = ptr[0:3]
        g.normal_w[:] = ptr[3:6]
        g.albedo[:] = ptr[6:9]
        g.metallic, g.roughness, g.ao = ptr[9], ptr[10], ptr[11]
        g.f0[:] = ptr[12:15]
        g.width, g.height, g.row_stride = int(self.width), int(self.height), int(self.row_stride)
        g.opacity = None if self.opacity is None else self.opacity.data_ptr()
        return g


@dataclass
class Material:
    """``Material`` / ``MaterialProperties`` (Material.h:10-69) as PS reads them before the light loop
    (Core.hlsl:64-81, Default.hlsl:79-116): the constants with the reference's defaults, the permutation as
    ``flags`` (``N.PBR_MAT_*``) and ``tex``, indices into the texture list of :meth:`ShadingContext.set_materials`
    in the order diffuse, specular, metallic, roughness, normal, opacity (-1: unused)."""
    diffuse_albedo: Sequence[float] = (1.0, 1.0, 1.0)
    metallic: float = 0.0
    fresnel_r0: Sequence[float] = (0.04, 0.04, 0.04)
    roughness: float = 1.0
    opacity: float = 1.0
    flags: int = 0
    tex: Sequence[int] = (-1, -1, -1, -1, -1, -1)

    def to_c(self) -> N.MaterialDesc:
        m = N.MaterialDesc()
        m.diffuse_albedo[:] = [float(v) for v in self.diffuse_albedo]
        m.metallic = float(self.metallic)
        m.fresnel_r0[:] = [float(v) for v in self.fresnel_r0]
        m.roughness = float(self.roughness)
        m.opacity = float(self.opacity)
        m.flags = int(self.flags)
        m.tex[:] = [int(v) for v in self.tex]
        return m


class Attributes:
    """The interpolated ``VertexOut`` (Default.hlsl:12-20) per pixel on the device: one (14, H, row_stride) fp32
    tensor, plane order pos xyz, normal xyz, tangent xyz, bitangent xyz, uv (pbr_attributes_soa), and an
    (H, row_stride) 16-bit material id plane with the same row stride (``N.PBR_MATERIAL_NONE`` = background)."""

    def __init__(self, planes: torch.Tensor, material: torch.Tensor, width: Optional[int] = None):
        if planes.dim() != 3 or planes.shape[0] != N.NUM_ATTRIBUTE_PLANES or planes.dtype != torch.float32:
            raise ValueError("planes must be a (14, H, W) float32 tensor")
        if planes.stride(2) != 1:
            raise ValueError("planes rows must be contiguous")
        if (material.dim() != 2 or material.element_size() != 2 or material.is_floating_point() or
                material.shape[0] != planes.shape[1] or material.shape[1] < planes.shape[2] or
                material.stride(1) != 1 or material.stride(0) != planes.stride(1) or
                material.device != planes.device):
            raise ValueError("material must be an (H, W) 16-bit integer plane with the planes' row stride and device")
        self.planes = planes
        self.material = material
        self.depth: Optional[torch.Tensor] = None  # set by ShadingContext.rasterize
        self.height = planes.shape[1]
        self.width = planes.shape[2] if width is None else width
        self.row_stride = planes.stride(1)

    @classmethod
    def from_host(cls, planes: np.ndarray, material: np.ndarray, device) -> "Attributes":
        t = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32))
        # torch has no portable uint16: the ids travel as the same bits in int16
        m = torch.from_numpy(np.ascontiguousarray(material, dtype=np.uint16).view(np.int16))
        return cls(t.to(device), m.to(device))

    def rows(self, r0: int, r1: int) -> "Attributes":
        """A row band (a view)."""
        return Attributes(self.planes[:, r0:r1, :], self.material[r0:r1], self.width)

    def to_c(self) -> N.AttributesSoA:
        a = N.AttributesSoA()
        base = self.planes.data_ptr()
        ps = self.planes.stride(0) * 4
        ptr = [base + i * ps for i in range(N.NUM_ATTRIBUTE_PLANES)]
        a.pos_w[:] = ptr[0:3]
        a.normal_w[:] = ptr[3:6]
        a.tangent_w[:] = ptr[6:9]
        a.bitangent_w[:] = ptr[9:12]
        a.tex_coord[:] = ptr[12:14]
        a.material = self.material.data_ptr()
        a.width, a.height, a.row_stride = int(self.width), int(self.height), int(self.row_stride)
        return a


IDENTITY4 = tuple(np.eye(4, dtype=np.float32).ravel().tolist())


def _matrix16(m) -> list:
    a = np.asarray(m, dtype=np.float32).reshape(-1)
    if a.size != 16:
        raise ValueError("a matrix is 16 floats, row-major")
    return a.tolist()


@dataclass
class Mesh:
    """One indexed triangle list on the host (pbr_mesh_desc): ``vertices`` (n, 14) float32 in the reference's
    ``Vertex`` order (FrameResource.h:46-52: Pos, Normal, Tangent, Bitangent, TexCoord), ``indices`` uint32."""
    vertices: np.ndarray
    indices: np.ndarray

    def __post_init__(self):
        self.vertices = np.ascontiguousarray(self.vertices, dtype=np.float32).reshape(-1, 14)
        self.indices = np.ascontiguousarray(self.indices, dtype=np.uint32).reshape(-1)


@dataclass
class Draw:
    """One render item (pbr_draw; RenderItem + DrawIndexedInstanced, PBRApp.cpp:1103-1134). Matrices are row-major
    and multiply a row vector, as ``mul(v, M)`` in Default.hlsl:27-42. ``index_count`` None: to the mesh's end."""
    mesh: int = 0
    material: int = 0
    world: Sequence[float] = IDENTITY4
    tex_transform: Sequence[float] = IDENTITY4
    mat_transform: Sequence[float] = IDENTITY4
    cull: int = 0  # 0 = back faces culled (D3D12_DEFAULT), 1 = none
    first_index: int = 0
    index_count: Optional[int] = None

    def to_c(self, meshes: Sequence[Mesh] = ()) -> N.DrawDesc:
        d = N.DrawDesc()
        d.mesh, d.first_index, d.material, d.cull = int(self.mesh), int(self.first_index), int(self.material), int(self.cull)
        if self.index_count is None:
            if not 0 <= self.mesh < len(meshes):
                raise ValueError("Draw.index_count is None and the mesh is unknown")
            d.index_count = int(meshes[self.mesh].indices.size) - int(self.first_index)
        else:
            d.index_count = int(self.index_count)
        d.world[:] = _matrix16(self.world)
        d.tex_transform[:] = _matrix16(self.tex_transform)
        d.mat_transform[:] = _matrix16(self.mat_transform)
        return d


@dataclass
class View:
    """pbr_raster_view: ``view_proj`` (row-major, row vectors, depth 0..1), the full frame's size, the row band the
    targets hold, and the background basis: a pixel without a fragment gets
    ``normalize(bg_forward + sx * bg_right + sy * bg_up)`` as its direction (scenes.look_at_view makes one)."""
    view_proj: Sequence[float]
    width: int
    height: int
    eye: Sequence[float] = (0.0, 0.0, 0.0)
    bg_right: Sequence[float] = (1.0, 0.0, 0.0)
    bg_up: Sequence[float] = (0.0, 1.0, 0.0)
    bg_forward: Sequence[float] = (0.0, 0.0, 1.0)
    row_begin: int = 0
    row_end: Optional[int] = None

    def rows(self, r0: int, r1: int) -> "View":
        """The same view over rows [r0, r1) of the frame."""
        from dataclasses import replace
        return replace(self, row_begin=int(r0), row_end=int(r1))

    def to_c(self) -> N.RasterView:
        v = N.RasterView()
        v.view_proj[:] = _matrix16(self.view_proj)
        v.width, v.height = int(self.width), int(self.height)
        v.row_begin = int(self.row_begin)
        v.row_end = int(self.height if self.row_end is None else self.row_end)
        v.eye[:] = [float(x) for x in self.eye]
        v.bg_right[:] = [float(x) for x in self.bg_right]
        v.bg_up[:] = [float(x) for x in self.bg_up]
        v.bg_forward[:] = [float(x) for x in self.bg_forward]
        return v


def _stream_handle(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream)


class ShadingContext:
    """One ``pbr_context`` on one device."""

    def __init__(self, device: int = 0):
        self.lib = N.lib()
        self.device = int(device)
        h = ctypes.c_void_p()
        N.check(self.lib.pbr_context_create(self.device, ctypes.byref(h)), "pbr_context_create")
        self._h = h
        self.pass_constants: Optional[PassConstants] = None

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h:
            self.lib.pbr_context_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_pass(self, pc: PassConstants, stream=None) -> None:
        keep: list = []
        p = pc.to_c(keep)
        N.check(self.lib.pbr_set_pass(self._h, ctypes.byref(p), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_set_pass", self._h)
        self.pass_constants = pc

    def _set_texture(self, name: str, texels: np.ndarray, stream) -> None:
        if texels.dtype == np.uint16:
            fn, t = name, np.ascontiguousarray(texels)
        elif texels.dtype == np.float32:
            fn, t = name + "_f32", np.ascontiguousarray(texels)
        else:
            raise ValueError(f"{name}: texels must be uint16 (R16G16B16A16_UNORM) or float32 RGBA")
        if t.ndim != 3 or t.shape[2] != 4:
            raise ValueError(f"{name}: texels must be (h, w, 4)")
        N.check(getattr(self.lib, fn)(self._h, t.ctypes.data, t.shape[1], t.shape[0],
                                      ctypes.c_void_p(_stream_handle(stream))), fn, self._h)

    def set_env_map(self, texels: np.ndarray, stream=None) -> None:
        """IBL environment (g_SkyArray[1]): (h, w, 4) uint16 UNORM or float32 (e.g. a decoded .hdr)."""
        self._set_texture("pbr_set_env_map", texels, stream)

    def set_sky_map(self, texels: np.ndarray, stream=None) -> None:
        """Sky texture (g_SkyArray[0]) sampled for background pixels: uint16 UNORM or float32 RGBA."""
        self._set_texture("pbr_set_sky_map", texels, stream)

    def set_materials(self, materials: Sequence[Material], textures: Sequence[np.ndarray] = (), stream=None) -> None:
        """Upload the material table and its textures (pbr_set_materials; BuildMaterials / LoadTextures,
        PBRApp.cpp:892-963, 1196-1463). ``textures``: uint8 arrays, (h, w) or (h, w, c) with c in {1, 3, 4}."""
        tex = []
        for t in textures:
            t = np.asarray(t)
            if t.dtype != np.uint8 or t.ndim not in (2, 3):
                raise ValueError("textures must be uint8 arrays of shape (h, w) or (h, w, channels)")
            tex.append(np.ascontiguousarray(t if t.ndim == 3 else t[:, :, None]))
        mats = (N.MaterialDesc * max(len(materials), 1))(*[m.to_c() for m in materials])
        descs = (N.TextureDesc * max(len(tex), 1))()
        for d, t in zip(descs, tex):
            d.texels, d.height, d.width, d.channels = t.ctypes.data, t.shape[0], t.shape[1], t.shape[2]
        N.check(self.lib.pbr_set_materials(self._h, mats, len(materials), descs, len(tex),
                                           ctypes.c_void_p(_stream_handle(stream))), "pbr_set_materials", self._h)

    def resolve(self, attrs: Attributes, filter: int = N.PBR_FILTER_POINT, out=None, stream=None):
        """The first half of PS (Default.hlsl:50-116) on the device (pbr_resolve_materials): ``attrs`` and the
        materials of :meth:`set_materials` into a G-buffer, asynchronously. Returns ``(GBuffer, coverage)``: the
        G-buffer carries the resolved opacity plane and feeds :meth:`shade` / :meth:`shade_frame` as it is (set the
        pass with ``PBR_FLAG_F0_PLANE``); ``coverage`` is the (H, W) uint8 plane of ``shade_frame``. ``out``: a
        ``GBuffer`` or a ``(GBuffer, coverage)`` pair to write into (an absent opacity or coverage plane is not
        written); default: fresh tensors."""
        gb, coverage, t = self._resolve_targets(attrs, out)
        a = attrs.to_c()
        N.check(self.lib.pbr_resolve_materials(self._h, ctypes.byref(a), ctypes.byref(t), int(filter),
                                               ctypes.c_void_p(_stream_handle(stream))),
                "pbr_resolve_materials", self._h)
        return gb, coverage

    def _resolve_targets(self, attrs: Attributes, out):
        """``out`` of :meth:`resolve` / :meth:`resolve_mip` as ``(GBuffer, coverage, pbr_gbuffer_targets)``."""
        self._check_device(attrs.planes, attrs.material)
        dev = attrs.planes.device
        if out is None:
            gb = GBuffer(torch.empty((N.NUM_PLANES, attrs.height, attrs.width), dtype=torch.float32, device=dev),
                         opacity=torch.empty((attrs.height, attrs.width), dtype=torch.float32, device=dev))
            coverage = torch.empty((attrs.height, attrs.width), dtype=torch.uint8, device=dev)
        elif isinstance(out, GBuffer):
            gb, coverage = out, None
        else:
            gb, coverage = out
        self._check_device(gb.planes, gb.opacity, coverage)
        if gb.height < attrs.height or gb.width < attrs.width:
            raise ValueError("out is smaller than the attributes")
        t = N.GBufferTargets()
        ps = gb.planes.stride(0) * 4
        t.planes[:] = [gb.planes.data_ptr() + i * ps for i in range(N.NUM_PLANES)]
        t.opacity = None if gb.opacity is None else gb.opacity.data_ptr()
        t.row_stride = int(gb.row_stride)
        if coverage is not None:
            if coverage.dtype != torch.uint8 or coverage.dim() != 2 or coverage.stride(1) != 1:
                raise ValueError("coverage must be a (H, W) uint8 tensor with contiguous rows")
            if coverage.shape[0] < attrs.height or coverage.shape[1] < attrs.width:
                raise ValueError("coverage is smaller than the attributes")
            t.coverage = coverage.data_ptr()
            t.coverage_row_stride = coverage.stride(0)
        return gb, coverage, t

    def generate_mips(self, stream=None) -> None:
        """Build the mip chains of the current material table's textures on the device (pbr_generate_mips; the
        MipLevels of the reference's textures, PBRApp.cpp:701, :1171-1178). Call it after every
        :meth:`set_materials` whose table :meth:`resolve_mip` is to sample; synchronises ``stream``."""
        N.check(self.lib.pbr_generate_mips(self._h, ctypes.c_void_p(_stream_handle(stream))), "pbr_generate_mips",
                self._h)

    def resolve_mip(self, attrs: Attributes, lod_bias: float = 0.0, out=None, stream=None):
        """:meth:`resolve` with the mip-mapped trilinear filter on the five material maps
        (pbr_resolve_materials_mip): the level of detail of a pixel comes from the differences of its UV
        inside its 2 x 2 pixel quad, plus ``lod_bias``. Needs :meth:`generate_mips`. A row band of ``attrs`` must start
        on an even row of the frame and have an even height or end with the frame. Returns what :meth:`resolve`
        returns."""
        gb, coverage, t = self._resolve_targets(attrs, out)
        a = attrs.to_c()
        N.check(self.lib.pbr_resolve_materials_mip(self._h, ctypes.byref(a), ctypes.byref(t), float(lod_bias),
                                                   ctypes.c_void_p(_stream_handle(stream))),
                "pbr_resolve_materials_mip", self._h)
        return gb, coverage

    def resolve_aniso(self, attrs: Attributes, max_anisotropy: int = 8, lod_bias: float = 0.0, out=None, stream=None):
        """:meth:`resolve_mip` with the anisotropic filter on the five material maps (pbr_resolve_materials_aniso;
        DESIGN.md §11; the reference's sampler has maxAnisotropy 8): per texture, up to ``max_anisotropy`` (1 .. 16)
        bilinear taps along the longer of the pixel's two footprint axes, at the level of detail of the shorter one.
        With ``max_anisotropy`` 1 it is :meth:`resolve_mip` bit for bit. Needs :meth:`generate_mips`; the band rule is
        :meth:`resolve_mip`'s. Returns what :meth:`resolve` returns."""
        gb, coverage, t = self._resolve_targets(attrs, out)
        a = attrs.to_c()
        N.check(self.lib.pbr_resolve_materials_aniso(self._h, ctypes.byref(a), ctypes.byref(t), float(lod_bias),
                                                     int(max_anisotropy), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_resolve_materials_aniso", self._h)
        return gb, coverage

    def set_meshes(self, meshes: Sequence[Mesh], stream=None) -> None:
        """Upload the meshes :meth:`rasterize` draws from (pbr_set_meshes; the vertex / index buffer uploads of
        BuildShapeGeometry). An index outside its mesh raises ``PbrError(PBR_ERR_INVALID_ARGUMENT)``."""
        meshes = list(meshes)
        descs = (N.MeshDesc * max(len(meshes), 1))()
        for d, m in zip(descs, meshes):
            d.vertices, d.indices = m.vertices.ctypes.data, m.indices.ctypes.data
            d.n_vertices, d.n_indices = m.vertices.shape[0], m.indices.size
        N.check(self.lib.pbr_set_meshes(self._h, descs, len(meshes), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_set_meshes", self._h)
        self.meshes = meshes

    def rasterize(self, draws: Sequence[Draw], view: View, out=None, stream=None,
                  clip_near: bool = False, alpha_test: bool = False) -> Attributes:
        """VS and the rasteriser on the device (pbr_rasterize): ``draws`` in order under ``view`` into
        the attribute planes :meth:`resolve` consumes, asynchronously. ``out``: an ``Attributes`` holding the view's
        row band, or an ``(Attributes, depth)`` pair with an (H, row_stride) float32 depth plane; default: fresh
        tensors. The result carries the depth plane as ``.depth`` (None when ``out`` had none). ``clip_near``
        (pbr_rasterize_flags with PBR_RASTER_CLIP_NEAR): triangles that cross the near plane are clipped against it
        and drawn, not skipped (step 2a). ``alpha_test`` (PBR_RASTER_ALPHA_TEST; needs :meth:`set_materials`): the
        fragments of draws whose material has PBR_MAT_ALPHA_TEST are discarded before the depth update where the
        opacity texture's texel is below the threshold, so what lies behind a cut-out shows (step 6a)."""
        flags = (N.PBR_RASTER_CLIP_NEAR if clip_near else 0) | (N.PBR_RASTER_ALPHA_TEST if alpha_test else 0)
        return self.rasterize_flags(draws, view, flags if flags else None, out=out, stream=stream)

    def rasterize_flags(self, draws: Sequence[Draw], view: View, flags, out=None, stream=None) -> Attributes:
        """:meth:`rasterize` through pbr_rasterize_flags with the given ``flags`` word (0: the same result as
        pbr_rasterize; an unknown bit raises ``PbrError(PBR_ERR_INVALID_ARGUMENT)``); ``flags`` None: pbr_rasterize."""
        return self._rasterize(draws, view, flags, out, stream)

    def _rasterize(self, draws, view, flags, out, stream, layer=None) -> Attributes:
        """The three rasterising entry points behind one target set-up; ``layer``: a filled ``N.RasterLayer``."""
        v = view.to_c()
        attrs, depth, t = self._raster_targets(view, v, out)
        meshes = getattr(self, "meshes", ())
        c_draws = (N.DrawDesc * max(len(draws), 1))(*[d.to_c(meshes) for d in draws])
        if layer is not None:
            N.check(self.lib.pbr_rasterize_layer(self._h, c_draws, len(draws), ctypes.byref(v), ctypes.byref(t),
                                                 int(flags), ctypes.byref(layer),
                                                 ctypes.c_void_p(_stream_handle(stream))), "pbr_rasterize_layer", self._h)
        elif flags is None:
            N.check(self.lib.pbr_rasterize(self._h, c_draws, len(draws), ctypes.byref(v), ctypes.byref(t),
                                           ctypes.c_void_p(_stream_handle(stream))), "pbr_rasterize", self._h)
        else:
            N.check(self.lib.pbr_rasterize_flags(self._h, c_draws, len(draws), ctypes.byref(v), ctypes.byref(t),
                                                 int(flags), ctypes.c_void_p(_stream_handle(stream))),
                    "pbr_rasterize_flags", self._h)
        attrs.depth = depth
        return attrs

    def _raster_targets(self, view, v, out):
        """``out`` of a rasterising call as ``(Attributes, depth, pbr_raster_targets)``; ``v``: ``view.to_c()``."""
        rows = v.row_end - v.row_begin
        dev = torch.device("cuda", self.device)
        if out is None:
            attrs = Attributes(torch.empty((N.NUM_ATTRIBUTE_PLANES, max(rows, 0), view.width), dtype=torch.float32, device=dev),
                               torch.empty((max(rows, 0), view.width), dtype=torch.int16, device=dev))
            depth = torch.empty((max(rows, 0), view.width), dtype=torch.float32, device=dev)
        elif isinstance(out, Attributes):
            attrs, depth = out, None
        else:
            attrs, depth = out
        self._check_device(attrs.planes, attrs.material, depth)
        if attrs.height < rows or attrs.width < view.width:
            raise ValueError("out is smaller than the view's band")
        if depth is not None and (depth.dtype != torch.float32 or depth.dim() != 2 or depth.stride(1) != 1 or
                                  depth.shape[0] < rows or depth.stride(0) != attrs.row_stride):
            raise ValueError("depth must be an (H, W) float32 plane with the attribute planes' row stride")
        t = N.RasterTargets()
        ps = attrs.planes.stride(0) * 4
        t.planes[:] = [attrs.planes.data_ptr() + i * ps for i in range(N.NUM_ATTRIBUTE_PLANES)]
        t.material = attrs.material.data_ptr()
        t.depth = None if depth is None else depth.data_ptr()
        t.row_stride = int(attrs.row_stride)
        return attrs, depth, t

    def raster_stats(self, stream=None) -> dict:
        """pbr_last_raster_stats of the last :meth:`rasterize` on ``stream`` (synchronises it): triangles,
        backface_culled, zero_area, skipped_near, skipped_guard_band, fragments."""
        st = N.RasterStats()
        N.check(self.lib.pbr_last_raster_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_raster_stats", self._h)
        return {name: getattr(st, name) for name, _ in N.RasterStats._fields_}

    def raster_clip_stats(self, stream=None) -> dict:
        """pbr_last_raster_clip_stats of the last :meth:`rasterize` on ``stream`` (synchronises it): clipped_near,
        clip_pieces; zeros after a call without ``clip_near``."""
        st = N.RasterClipStats()
        N.check(self.lib.pbr_last_raster_clip_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_raster_clip_stats", self._h)
        return {name: getattr(st, name) for name, _ in N.RasterClipStats._fields_}

    def raster_alpha_stats(self, stream=None) -> dict:
        """pbr_last_raster_alpha_stats of the last :meth:`rasterize` on ``stream`` (synchronises it): alpha_tested,
        alpha_discarded; zeros after a call without ``alpha_test``."""
        st = N.RasterAlphaStats()
        N.check(self.lib.pbr_last_raster_alpha_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_raster_alpha_stats", self._h)
        return {name: getattr(st, name) for name, _ in N.RasterAlphaStats._fields_}

    def rasterize_layer(self, draws: Sequence[Draw], view: View, depth_in: torch.Tensor,
                        prim_in: Optional[torch.Tensor] = None, flags: int = 0, out=None,
                        prim_out: Optional[torch.Tensor] = None, stream=None):
        """One layer of the transparent pass (pbr_rasterize_layer): per pixel the fragment of
        ``draws`` with the smallest primitive ordinal among those at or past the floor ``prim_in`` ((H, row_stride)
        int32 on the device; None: 0 everywhere, the first layer) and with z below ``depth_in`` ((H, row_stride)
        float32). Returns ``(Attributes, prim_out)``: the attributes carry the new depth plane as ``.depth`` (the
        winner's z; ``depth_in``'s value where the layer has no fragment, where the material is PBR_MATERIAL_NONE),
        ``prim_out`` is the floor for the next layer. ``out``: an ``(Attributes, depth)`` pair; its depth plane may be
        ``depth_in`` itself and ``prim_out`` may be ``prim_in``. Every layer of a sequence must pass the same ``draws``:
        the ordinals are the call's own. ``flags``: 0 or PBR_RASTER_CLIP_NEAR."""
        v = view.to_c()
        rows = max(v.row_end - v.row_begin, 0)
        dev = torch.device("cuda", self.device)
        stride = depth_in.stride(0) if depth_in.dim() == 2 else view.width
        if out is None:
            out = (Attributes(torch.empty((N.NUM_ATTRIBUTE_PLANES, rows, stride), dtype=torch.float32, device=dev),
                              torch.empty((rows, stride), dtype=torch.int16, device=dev), width=view.width),
                   torch.empty((rows, stride), dtype=torch.float32, device=dev))
        if isinstance(out, Attributes) or out[1] is None:
            raise ValueError("a layer needs a depth plane: out must be an (Attributes, depth) pair")
        if prim_out is None:
            prim_out = torch.empty((rows, stride), dtype=torch.int32, device=dev)
        self._check_device(depth_in, prim_in, prim_out)
        for name, p, dtype in (("depth_in", depth_in, torch.float32), ("prim_in", prim_in, torch.int32),
                               ("prim_out", prim_out, torch.int32)):
            if p is not None and (p.dtype != dtype or p.dim() != 2 or p.stride(1) != 1 or p.shape[0] < rows or
                                  p.shape[1] < view.width or p.stride(0) != out[0].row_stride):
                raise ValueError(f"{name} must be an (H, W) {dtype} plane with the attribute planes' row stride")
        layer = N.RasterLayer()
        layer.depth_in = depth_in.data_ptr()
        layer.prim_in = None if prim_in is None else prim_in.data_ptr()
        layer.prim_out = prim_out.data_ptr()
        return self._rasterize(draws, view, flags, out, stream, layer=layer), prim_out

    def raster_layer_stats(self, stream=None) -> dict:
        """pbr_last_raster_layer_stats of the last rasterisation on ``stream`` (synchronises it): layer_fragments, the
        visibility updates a :meth:`rasterize_layer` issued (0: the layer is empty); zeros after any other call."""
        st = N.RasterLayerStats()
        N.check(self.lib.pbr_last_raster_layer_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_raster_layer_stats", self._h)
        return {name: getattr(st, name) for name, _ in N.RasterLayerStats._fields_}

    def blend_layer(self, src: torch.Tensor, alpha: torch.Tensor, coverage: torch.Tensor, frame: torch.Tensor,
                    width: Optional[int] = None, height: Optional[int] = None, stream=None) -> torch.Tensor:
        """The transparent PSO's blend (pbr_blend_layer; PBRApp.cpp:831-842) of a shaded layer over ``frame``, in
        place and asynchronously: where ``coverage`` ((H, >=W) uint8) is nonzero, colour = src * a + frame * (1 - a) and
        alpha = a, with a from ``alpha`` ((H, >=W) float32: the resolved opacity plane). ``src``: (H, >=W, 4) float32;
        ``frame``: (H, >=W, 4) float32 (RGBA32F) or uint8 (RGBA8_UNORM: inputs clamped to [0, 1], NaN -> 0). Pixels
        with coverage 0 are neither read nor written in ``frame``."""
        self._check_device(src, alpha, coverage, frame)
        if frame.dtype == torch.uint8:
            fmt = N.PBR_OUTPUT_RGBA8_UNORM
        elif frame.dtype == torch.float32:
            fmt = N.PBR_OUTPUT_RGBA32F
        else:
            raise ValueError("frame must be float32 (RGBA32F) or uint8 (RGBA8_UNORM)")
        for name, t in (("src", src), ("frame", frame)):
            if t.dim() != 3 or t.shape[2] != 4 or t.stride(2) != 1 or t.stride(1) != 4:
                raise ValueError(f"{name} must be (H, W, 4) with contiguous pixels")
        if src.dtype != torch.float32:
            raise ValueError("src must be float32")
        if alpha.dtype != torch.float32 or alpha.dim() != 2 or alpha.stride(1) != 1:
            raise ValueError("alpha must be a (H, W) float32 plane with contiguous rows")
        if coverage.dtype != torch.uint8 or coverage.dim() != 2 or coverage.stride(1) != 1:
            raise ValueError("coverage must be a (H, W) uint8 tensor with contiguous rows")
        h = min(src.shape[0], frame.shape[0]) if height is None else int(height)
        w = min(src.shape[1], frame.shape[1]) if width is None else int(width)
        for t in (src, alpha, coverage, frame):
            if t.shape[0] < h or t.shape[1] < w:
                raise ValueError("a plane is smaller than the blended rectangle")
        b = N.BlendSource()
        b.src, b.src_row_stride = src.data_ptr(), src.stride(0) // 4
        b.alpha, b.alpha_row_stride = alpha.data_ptr(), alpha.stride(0)
        b.coverage, b.coverage_row_stride = coverage.data_ptr(), coverage.stride(0)
        f = N.FrameDesc()
        f.out = frame.data_ptr()
        f.out_row_stride = frame.stride(0) // 4
        f.format = int(fmt)
        N.check(self.lib.pbr_blend_layer(self._h, ctypes.byref(b), ctypes.byref(f), w, h,
                                         ctypes.c_void_p(_stream_handle(stream))), "pbr_blend_layer", self._h)
        return frame

    def draw_transparent(self, draws: Sequence[Draw], view: View, depth: torch.Tensor, frame: torch.Tensor, *,
                         flags: int = 0, filter: int = N.PBR_FILTER_POINT, max_layers: int = 8, stream=None,
                         mip_lod_bias: Optional[float] = None, max_anisotropy: Optional[int] = None):
        """The reference's transparent pass (RenderLayer::Transparent, PBRApp.cpp:313-316) over a finished frame:
        layer after layer, :meth:`rasterize_layer` -> :meth:`resolve` -> :meth:`shade` -> :meth:`blend_layer`, until a
        layer is empty or ``max_layers`` layers were blended. ``depth``: the (H, row_stride) float32 depth plane of the
        opaque and alpha-tested layers (1 where they drew nothing), updated in place to the depth after the pass;
        ``frame``: the (H, W, 4) float32 or uint8 frame of the view's band, blended in place. The pass of
        :meth:`set_pass` shades every layer (set ``PBR_FLAG_F0_PLANE``, as for any resolved G-buffer). Each layer
        re-runs the vertex transform and the setup and shades the whole band. Returns ``(layers, stopped_on_empty)``:
        how many layers were blended and whether the loop ended on an empty layer (False: ``max_layers`` was reached
        and more may remain). Synchronises ``stream`` once per layer, to read the layer's counter. ``mip_lod_bias``: when
        not None, every layer goes through :meth:`resolve_mip` with that bias (``filter`` is then not used; needs
        :meth:`generate_mips`; the view's band must then start on an even row and have an even height or end with the
        frame). ``max_anisotropy``: when not None, every layer goes through :meth:`resolve_aniso` with that tap limit,
        under the bias ``mip_lod_bias`` (0 when that is None) and the same rule for the band."""
        v = view.to_c()
        rows = max(v.row_end - v.row_begin, 0)
        dev = torch.device("cuda", self.device)
        stride = depth.stride(0)
        attrs = Attributes(torch.empty((N.NUM_ATTRIBUTE_PLANES, rows, stride), dtype=torch.float32, device=dev),
                           torch.empty((rows, stride), dtype=torch.int16, device=dev), width=view.width)
        prim = torch.empty((rows, stride), dtype=torch.int32, device=dev)
        gb = GBuffer(torch.empty((N.NUM_PLANES, rows, view.width), dtype=torch.float32, device=dev),
                     opacity=torch.empty((rows, view.width), dtype=torch.float32, device=dev))
        coverage = torch.empty((rows, view.width), dtype=torch.uint8, device=dev)
        shaded = torch.empty((rows, view.width, 4), dtype=torch.float32, device=dev)
        for k in range(int(max_layers)):
            self.rasterize_layer(draws, view, depth, prim if k else None, flags, out=(attrs, depth), prim_out=prim,
                                 stream=stream)
            if self.raster_layer_stats(stream)["layer_fragments"] == 0:
                return k, True
            if max_anisotropy is not None:
                self.resolve_aniso(attrs, max_anisotropy, 0.0 if mip_lod_bias is None else mip_lod_bias,
                                   out=(gb, coverage), stream=stream)
            elif mip_lod_bias is None:
                self.resolve(attrs, filter, out=(gb, coverage), stream=stream)
            else:
                self.resolve_mip(attrs, mip_lod_bias, out=(gb, coverage), stream=stream)
            self.shade(gb, shaded, stream=stream)
            self.blend_layer(shaded, gb.opacity, coverage, frame, width=view.width, height=rows, stream=stream)
        return int(max_layers), False

    def msaa_rasterize(self, draws: Sequence[Draw], view: View, flags: int = 0, surface: Optional[torch.Tensor] = None,
                       stream=None) -> torch.Tensor:
        """Vertex stage, setup and coverage at four samples per pixel (pbr_msaa_rasterize),
        asynchronously. ``surface``: a (4, rows, row_stride) int64 tensor on the device holding the view's band,
        sample-major; default: a fresh one with row_stride = width. Every word is set to all ones, then lowered to
        ``(bits(z) << 32) | triangle ordinal`` of the fragment the sample shows. Returns the surface. ``flags`` must be
        0 (PBR_RASTER_CLIP_NEAR and PBR_RASTER_ALPHA_TEST raise ``PbrError(PBR_ERR_UNSUPPORTED)``)."""
        v = view.to_c()
        if surface is None:
            surface = torch.empty((4, max(v.row_end - v.row_begin, 0), view.width), dtype=torch.int64,
                                  device=torch.device("cuda", self.device))
        sf = self._msaa_surface(surface, v)
        meshes = getattr(self, "meshes", ())
        c_draws = (N.DrawDesc * max(len(draws), 1))(*[d.to_c(meshes) for d in draws])
        N.check(self.lib.pbr_msaa_rasterize(self._h, c_draws, len(draws), ctypes.byref(v), int(flags), ctypes.byref(sf),
                                            ctypes.c_void_p(_stream_handle(stream))), "pbr_msaa_rasterize", self._h)
        return surface

    def _msaa_surface(self, surface: torch.Tensor, v) -> N.MsaaSurface:
        self._check_device(surface)
        rows = max(v.row_end - v.row_begin, 0)
        if (surface.dtype != torch.int64 or surface.dim() != 3 or surface.shape[0] != 4 or surface.shape[1] != rows or
                surface.shape[2] < v.width or surface.stride(2) != 1 or surface.stride(0) != rows * surface.stride(1)):
            raise ValueError("surface must be a (4, rows, >= width) int64 tensor whose planes follow one another")
        sf = N.MsaaSurface()
        sf.visibility, sf.row_stride = surface.data_ptr(), surface.stride(1)
        return sf

    def msaa_fragments(self, draws: Sequence[Draw], view: View, surface: torch.Tensor, slot: int, flags: int = 0,
                       out=None, owner: Optional[torch.Tensor] = None, stream=None):
        """Slot ``slot`` (0 .. 3) of every pixel out of ``surface`` (pbr_msaa_fragments): the fragment's attributes at
        the pixel centre, its material and depth; the background planes and PBR_MATERIAL_NONE where the pixel has no
        such slot or the fragment is the background. ``draws`` and ``view`` must be those of :meth:`msaa_rasterize`.
        ``out`` as for :meth:`rasterize`; ``owner``: a (rows, >= width) uint8 plane that receives the owner byte
        (the same for every slot), default a fresh one; pass ``False`` to write none. Returns ``(Attributes, owner)``
        with the depth plane as ``.depth``."""
        v = view.to_c()
        sf = self._msaa_surface(surface, v)
        attrs, depth, t = self._raster_targets(view, v, out)
        rows = max(v.row_end - v.row_begin, 0)
        if owner is None:
            owner = torch.empty((rows, view.width), dtype=torch.uint8, device=torch.device("cuda", self.device))
        elif owner is False:
            owner = None
        if owner is not None:
            self._check_device(owner)
            if (owner.dtype != torch.uint8 or owner.dim() != 2 or owner.stride(1) != 1 or owner.shape[0] < rows or
                    owner.shape[1] < view.width):
                raise ValueError("owner must be a (rows, >= width) uint8 plane with contiguous rows")
        meshes = getattr(self, "meshes", ())
        c_draws = (N.DrawDesc * max(len(draws), 1))(*[d.to_c(meshes) for d in draws])
        N.check(self.lib.pbr_msaa_fragments(self._h, c_draws, len(draws), ctypes.byref(v), int(flags), ctypes.byref(sf),
                                            int(slot), ctypes.byref(t),
                                            None if owner is None else ctypes.c_void_p(owner.data_ptr()),
                                            0 if owner is None else owner.stride(0),
                                            ctypes.c_void_p(_stream_handle(stream))), "pbr_msaa_fragments", self._h)
        attrs.depth = depth
        return attrs, owner

    def msaa_stats(self, stream=None) -> dict:
        """pbr_last_msaa_stats of the last :meth:`msaa_fragments` on ``stream`` (synchronises it): ``slot_pixels``, a
        list of the band's pixels in which slot 0 .. 3 exists; zeros after any other rasterising call."""
        st = N.MsaaStats()
        N.check(self.lib.pbr_last_msaa_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_msaa_stats", self._h)
        return {"slot_pixels": [int(x) for x in st.slot_pixels]}

    def msaa_resolve(self, slots: Sequence[Optional[torch.Tensor]], owner: torch.Tensor,
                     out: Optional[torch.Tensor] = None, fmt: int = N.PBR_OUTPUT_RGBA32F, n_slots: Optional[int] = None,
                     width: Optional[int] = None, height: Optional[int] = None, stream=None) -> torch.Tensor:
        """The multisample resolve (pbr_msaa_resolve), asynchronously: per pixel and channel
        ``((c0 + c1) + (c2 + c3)) * 0.25`` with ``c_s`` the pixel of the slot frame that owns sample s by ``owner``
        (0 where that slot is >= ``n_slots``). ``slots``: up to four (H, >= W, 4) float32 frames with one row stride
        (entries past ``n_slots``, default ``len(slots)``, may be None); ``out``: (H, >= W, 4) float32 (RGBA32F) or
        uint8 (RGBA8_UNORM: every sample goes through the UNORM8 encoding first), default a fresh frame of ``fmt``."""
        slots = list(slots)
        n = len(slots) if n_slots is None else int(n_slots)
        self._check_device(owner, out, *slots)
        live = [s for s in slots[:max(n, 0)] if s is not None]
        for s in live:
            if s.dtype != torch.float32 or s.dim() != 3 or s.shape[2] != 4 or s.stride(2) != 1 or s.stride(1) != 4:
                raise ValueError("a slot frame must be (H, W, 4) float32 with contiguous pixels")
        if not live or any(s.stride(0) != live[0].stride(0) for s in live):
            raise ValueError("the slot frames need one row stride, and slot 0 must be there")
        if owner.dtype != torch.uint8 or owner.dim() != 2 or owner.stride(1) != 1:
            raise ValueError("owner must be a (H, W) uint8 plane with contiguous rows")
        h = min(live[0].shape[0], owner.shape[0]) if height is None else int(height)
        w = min(live[0].shape[1], owner.shape[1]) if width is None else int(width)
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.uint8 if fmt == N.PBR_OUTPUT_RGBA8_UNORM else torch.float32,
                              device=owner.device)
        if out.dtype == torch.uint8:
            fmt = N.PBR_OUTPUT_RGBA8_UNORM
        elif out.dtype == torch.float32:
            fmt = N.PBR_OUTPUT_RGBA32F
        else:
            raise ValueError("out must be float32 (RGBA32F) or uint8 (RGBA8_UNORM)")
        if out.dim() != 3 or out.shape[2] != 4 or out.stride(2) != 1 or out.stride(1) != 4:
            raise ValueError("out must be (H, W, 4) with contiguous pixels")
        for t in live + [owner, out]:
            if t.shape[0] < h or t.shape[1] < w:
                raise ValueError("a plane is smaller than the resolved rectangle")
        src = N.MsaaResolveSource()
        src.slots[:] = [None if s is None else s.data_ptr() for s in (slots + [None] * 4)[:4]]
        src.slot_row_stride = live[0].stride(0) // 4
        src.n_slots = n
        src.owner, src.owner_row_stride = owner.data_ptr(), owner.stride(0)
        f = N.FrameDesc()
        f.out = out.data_ptr()
        f.out_row_stride = out.stride(0) // 4
        f.format = int(fmt)
        N.check(self.lib.pbr_msaa_resolve(self._h, ctypes.byref(src), ctypes.byref(f), w, h,
                                          ctypes.c_void_p(_stream_handle(stream))), "pbr_msaa_resolve", self._h)
        return out

    def draw_msaa(self, draws: Sequence[Draw], view: View, *, filter: int = N.PBR_FILTER_POINT,
                  mip_lod_bias: Optional[float] = None, max_anisotropy: Optional[int] = None,
                  fmt: int = N.PBR_OUTPUT_RGBA32F, out: Optional[torch.Tensor] = None, stream=None):
        """``draws`` under ``view`` with four samples per pixel (the reference's m_4xMsaaState): :meth:`msaa_rasterize`,
        then for every slot some pixel has :meth:`msaa_fragments` -> :meth:`resolve` (``filter``; ``mip_lod_bias`` /
        ``max_anisotropy`` choose :meth:`resolve_mip` / :meth:`resolve_aniso` as in :meth:`draw_transparent`, with its
        rule for the band) -> :meth:`shade_frame` with the slot's coverage plane, so background fragments get the sky,
        into RGBA32F; then :meth:`msaa_resolve` into ``out`` (default: a fresh frame of ``fmt``). The pass of
        :meth:`set_pass` shades every slot (set ``PBR_FLAG_F0_PLANE``); every slot shades the whole band. Returns
        ``(frame, slots)`` with ``slots`` the number of slots shaded. Synchronises ``stream`` once, to read the slot
        counters."""
        v = view.to_c()
        rows = max(v.row_end - v.row_begin, 0)
        dev = torch.device("cuda", self.device)
        if rows == 0 or view.width == 0:  # an empty band: nothing to draw
            dtype = torch.uint8 if fmt == N.PBR_OUTPUT_RGBA8_UNORM else torch.float32
            return (torch.empty((rows, view.width, 4), dtype=dtype, device=dev) if out is None else out), 0
        surface = self.msaa_rasterize(draws, view, stream=stream)
        attrs = Attributes(torch.empty((N.NUM_ATTRIBUTE_PLANES, rows, view.width), dtype=torch.float32, device=dev),
                           torch.empty((rows, view.width), dtype=torch.int16, device=dev))
        gb = GBuffer(torch.empty((N.NUM_PLANES, rows, view.width), dtype=torch.float32, device=dev),
                     opacity=torch.empty((rows, view.width), dtype=torch.float32, device=dev))
        coverage = torch.empty((rows, view.width), dtype=torch.uint8, device=dev)
        owner, n_slots, shaded = None, 1, []
        k = 0
        while k < n_slots:
            _, written = self.msaa_fragments(draws, view, surface, k, out=attrs, owner=None if k == 0 else False,
                                             stream=stream)
            if k == 0:
                owner = written
                pixels = self.msaa_stats(stream)["slot_pixels"]
                n_slots = max(1, sum(1 for p in pixels if p > 0))
            if max_anisotropy is not None:
                self.resolve_aniso(attrs, max_anisotropy, 0.0 if mip_lod_bias is None else mip_lod_bias,
                                   out=(gb, coverage), stream=stream)
            elif mip_lod_bias is None:
                self.resolve(attrs, filter, out=(gb, coverage), stream=stream)
            else:
                self.resolve_mip(attrs, mip_lod_bias, out=(gb, coverage), stream=stream)
            shaded.append(self.shade_frame(gb, coverage=coverage, fmt=N.PBR_OUTPUT_RGBA32F, stream=stream))
            k += 1
        frame = self.msaa_resolve(shaded, owner, out=out, fmt=fmt, width=view.width, height=rows, stream=stream)
        return frame, n_slots

    def _check_device(self, *tensors) -> None:
        """Every tensor handed to the kernel must live on this context's device: a foreign pointer would be
        dereferenced by the kernel (peer access or a fault)."""
        want = torch.device("cuda", self.device)
        for t in tensors:
            if t is not None and t.device != want:
                raise ValueError(f"tensor on {t.device}, but this ShadingContext shades on {want}")

    def shade(self, gb: GBuffer, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """Shade every pixel of ``gb`` into ``out`` ((H, >=W, 4) fp32 on the device), asynchronously."""
        self._check_device(gb.planes, gb.opacity, out)
        if out is None:
            out = torch.empty((gb.height, gb.width, 4), dtype=torch.float32, device=gb.planes.device)
        if out.dtype != torch.float32 or out.dim() != 3 or out.shape[2] != 4 or out.stride(2) != 1 or out.stride(1) != 4:
            raise ValueError("out must be (H, W, 4) float32 with contiguous pixels")
        if out.shape[0] < gb.height or out.shape[1] < gb.width:
            raise ValueError("out is smaller than the G-buffer")
        g = gb.to_c()
        N.check(self.lib.pbr_shade_gbuffer(self._h, ctypes.byref(g), ctypes.c_void_p(out.data_ptr()),
                                           out.stride(0) // 4, ctypes.c_void_p(_stream_handle(stream))),
                "pbr_shade_gbuffer", self._h)
        return out

    def shade_frame(self, gb: GBuffer, out: Optional[torch.Tensor] = None, coverage: Optional[torch.Tensor] = None,
                    fmt: int = N.PBR_OUTPUT_RGBA32F, stream=None) -> torch.Tensor:
        """Shade ``gb`` with the sky pass on background pixels (``coverage`` == 0; (H, >=W) uint8 on the
        device) into ``out``: (H, W, 4) float32 for RGBA32F or (H, W, 4) uint8 for RGBA8_UNORM."""
        self._check_device(gb.planes, gb.opacity, out, coverage)
        dev = gb.planes.device
        if fmt == N.PBR_OUTPUT_RGBA8_UNORM:
            dtype, px_bytes = torch.uint8, 4
        elif fmt == N.PBR_OUTPUT_RGBA32F:
            dtype, px_bytes = torch.float32, 16
        else:
            raise ValueError("unknown output format")
        if out is None:
            out = torch.empty((gb.height, gb.width, 4), dtype=dtype, device=dev)
        if out.dtype != dtype or out.dim() != 3 or out.shape[2] != 4 or out.stride(2) != 1 or out.stride(1) != 4:
            raise ValueError("out must be (H, W, 4) with contiguous pixels of the format's dtype")
        if out.shape[0] < gb.height or out.shape[1] < gb.width:
            raise ValueError("out is smaller than the G-buffer")
        f = N.FrameDesc()
        f.out = out.data_ptr()
        f.out_row_stride = out.stride(0) // 4
        f.format = int(fmt)
        if coverage is not None:
            if coverage.dtype != torch.uint8 or coverage.dim() != 2 or coverage.stride(1) != 1:
                raise ValueError("coverage must be a (H, W) uint8 tensor with contiguous rows")
            if coverage.shape[0] < gb.height or coverage.shape[1] < gb.width:
                raise ValueError("coverage is smaller than the G-buffer")
            f.coverage = coverage.data_ptr()
            f.coverage_row_stride = coverage.stride(0)
        g = gb.to_c()
        N.check(self.lib.pbr_shade_frame(self._h, ctypes.byref(g), ctypes.byref(f),
                                         ctypes.c_void_p(_stream_handle(stream))), "pbr_shade_frame", self._h)
        return out

    def pass_stats(self, stream=None) -> dict:
        """pbr_last_pass_stats of the last pass on ``stream`` as a dict (workgroups, culled, cull_tiles,
        cull_tile_lights, exact_pixels, light_terms, geometry_pixels, backface_tests)."""
        st = N.PassStats()
        N.check(self.lib.pbr_last_pass_stats(self._h, ctypes.byref(st), ctypes.c_void_p(_stream_handle(stream))),
                "pbr_last_pass_stats", self._h)
        return {name: getattr(st, name) for name, _ in N.PassStats._fields_}

    def last_kernel(self, stream=None) -> str:
        """pbr_last_pass_kernel: the kernel the last pass on ``stream`` launched, as rocprofv3 names it without
        its argument list ("" before the first pass)."""
        fn = getattr(self.lib, "pbr_last_pass_kernel", None)  # absent only from older A/B builds (PBR_LIB_PATH)
        return "" if fn is None else (fn(self._h, ctypes.c_void_p(_stream_handle(stream))) or b"").decode()

    def debug_bounds(self, reset: bool = True) -> dict:
        """pbr_debug_bounds of a bounds-checked build (PBR_DEBUG_BOUNDS, loaded through PBR_LIB_PATH): synchronises
        the device and returns {class name: last offending index} for every violated index class (empty: none),
        then clears the flags when ``reset``. Raises PbrError(PBR_ERR_UNSUPPORTED) on a product build."""
        flags = (ctypes.c_uint32 * 16)()
        N.check(self.lib.pbr_debug_bounds(self._h, flags, int(reset)), "pbr_debug_bounds", self._h)
        names = ("gbuffer", "output", "coverage", "texel", "light", "lds", "raster", "mesh")
        return {n: int(flags[8 + c]) for c, n in enumerate(names) if flags[c]}

    def cull_stats(self, stream=None):
        """(sum of surviving point/spot lights over tiles, tiles) of the last pass ((0, 0) unless it culled)."""
        s, t = ctypes.c_int64(), ctypes.c_int64()
        N.check(self.lib.pbr_last_cull_stats(self._h, ctypes.byref(s), ctypes.byref(t),
                                             ctypes.c_void_p(_stream_handle(stream))), "pbr_last_cull_stats", self._h)
        return s.value, t.value
