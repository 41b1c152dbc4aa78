// frontend_kernels.h -- internal launch interface between the C-ABI layer (pbr_frontend.hip) and the front end's gfx950
// kernels (frontend_kernels.hip): the material resolve and the rasteriser, which produce the G-buffer the shading
// kernels (shade_kernels.h) consume.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbr {

// ---- Material resolve (material_resolve.h; pbr_resolve_materials) ----------------------------------------------
// pbr_material_flags.
constexpr uint32_t kMatDiffuseTexture = 1u << 0, kMatSpecularTexture = 1u << 1, kMatMetallicTexture = 1u << 2,
                   kMatRoughnessTexture = 1u << 3, kMatNormalTexture = 1u << 4, kMatAlphaTest = 1u << 5;

// One texture of a material record: its first texel in the context's RGBA8 texel buffer and its size.
struct MaterialTex {
    uint32_t offset;
    int32_t w, h;
};
// The device copy of a pbr_material: constants, permutation flags and the six texture slots (diffuse, specular,
// metallic, roughness, normal, opacity); an unused slot is {0, 1, 1} and is never sampled.
struct MaterialRec {
    float diffuse[3];
    float metallic;
    float fresnel[3];
    float roughness;
    float opacity;
    uint32_t flags;
    MaterialTex tex[6];
};

struct ResolveArgs {
    const float* attr[14];     // pbr_attributes_soa order: pos xyz, normal xyz, tangent xyz, bitangent xyz, uv
    const uint16_t* material;  // ids; >= n_materials = background
    float* plane[15];          // pbr_gbuffer_soa order
    float* opacity;            // or nullptr
    uint8_t* coverage;         // or nullptr
    int width, height;
    int64_t in_stride, out_stride, cov_stride;
    const MaterialRec* table;
    int n_materials;
    const uint32_t* texels;    // every texture, RGBA8
    int64_t n_texels;
    bool linear;               // PBR_FILTER_LINEAR (else point)
    bool vec;  // every plane 8-byte aligned, ids 4-byte, coverage 2-byte, every stride even: paired accesses
};
hipError_t launch_resolve_materials(const ResolveArgs& a, hipStream_t stream);

// ---- Rasteriser (raster.h; pbr_rasterize) ---------------------------------------------------------
// One draw on the device: its constants and where its data is.
struct RasterDraw {
    float world[16], tex[16], mat[16];  // row-major, mul(v, M)
    uint32_t vtx_src;     // the mesh's first vertex in the context's vertex buffer
    uint32_t idx_src;     // the draw's first index in the context's index buffer
    uint32_t rec_base;    // the draw's first transformed-vertex record
    uint32_t n_vertices;  // of the mesh
    uint32_t material, cull;
    uint32_t pad[2];
};
// One transformed vertex of a draw: VS (Default.hlsl:27-42) and the viewport, DESIGN.md §12 steps 1-3.
// kVertexOutside (written by a near-clipping call only, step 2a): PosH.z is not >= 0; such a vertex's X, Y, z and rw
// are never read.
constexpr uint32_t kVertexNear = 1u, kVertexGuard = 2u, kVertexOutside = 4u;
struct RasterVertex {
    int32_t X, Y;    // window position in 1/256 pixel
    float z, rw;     // ndc.z and 1 / PosH.w
    float a[14];     // PosW, NormalW, TangentW, BitangentW, TexCoord
    uint32_t flags;  // kVertexNear: w not > 0; kVertexGuard: beyond the guard band or not finite; kVertexOutside
    uint32_t pad;
};
// Counters of a call, unsigned 64-bit words in device memory (pbr_raster_stats, pbr_raster_clip_stats,
// pbr_raster_alpha_stats; kRasterLarge: the large-triangle list's length). The first eight keep their slots.
enum RasterCounter { kRasterLarge = 0, kRasterCulled, kRasterZeroArea, kRasterNear, kRasterGuard, kRasterFragments,
                     kRasterClipped, kRasterClipPieces, kRasterAlphaTested, kRasterAlphaDiscarded,
                     kRasterCounters = 10 };

struct RasterArgs {
    const float* vertices;    // the mesh set: 14 floats per vertex
    const uint32_t* indices;
    int64_t n_src_vertices, n_src_indices;
    const RasterDraw* draws;
    const uint32_t* tri_prefix;  // n_draws + 1: triangles before draw d
    const uint32_t* rec_prefix;  // n_draws + 1: vertex records before draw d
    int n_draws;
    uint32_t n_tris, n_records;
    RasterVertex* records;
    unsigned long long* vis;       // (row_end - row_begin) * width visibility words
    uint2* large;                  // n_large slots: (triangle, its 64 x 4 block count | piece << 31)
    unsigned long long* counters;  // kRasterCounters
    float view_proj[16];
    int width, height, row_begin, row_end;
    float eye[3], right[3], up[3], fwd[3];
    float* plane[14];
    uint16_t* material;
    float* depth;  // or nullptr
    int64_t stride;
    bool vec;  // every plane 8-byte aligned, ids 4-byte, an even stride: paired stores
    // Appended for pbr_rasterize_flags, so that the fields above keep their kernel-argument offsets.
    bool clip_near;    // PBR_RASTER_CLIP_NEAR: the launches below start the kernels' clipping instantiations
    float4* posh;      // clip_near: PosH of every vertex record (n_records); else nullptr
    int64_t n_large;   // slots of `large`: n_tris, 2 n_tris when clip_near (a clipped triangle has up to two pieces)
    // Appended for PBR_RASTER_ALPHA_TEST (step 6a), read by the ALPHA instantiations only.
    const MaterialRec* table;  // the context's material table
    int n_materials;
    const uint32_t* texels;    // every texture, RGBA8
    int64_t n_texels;
    bool alpha_test;   // some draw's material has kMatAlphaTest: setup and large launch their ALPHA instantiations
};
// The stages of pbr_rasterize, each one launch (none when it has nothing to do): the vertex transform, the triangle
// setup with the small triangles' coverage, the large triangles' coverage, the per-pixel resolve. With a.clip_near
// each launches its near-clipping instantiation; with a.alpha_test the setup and the
// large-triangle stage launch their alpha-testing instantiations (step 6a).
hipError_t launch_raster_vertices(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_setup(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_large(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_resolve(const RasterArgs& a, hipStream_t stream);

// PBR_DEBUG_BOUNDS builds only (pbr_debug_bounds.h): point this unit's kernels at the device's bounds-flag buffer.
hipError_t debug_bounds_publish_frontend(uint32_t* buf);

}  // namespace pbr
