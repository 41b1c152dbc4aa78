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

// ---- Mip chains and the trilinear resolve (material_resolve.h; pbr_generate_mips, pbr_resolve_materials_mip) ------
// The chains of a material table live beside it, in a resource of their own: level 0 of a texture stays where the
// upload put it (MaterialRec::tex), its levels 1 .. L-1 are consecutive MaterialTex entries of a level table whose
// offsets count dwords of the chains' own texel buffer. A material finds its chains through a table parallel to the
// material table: five MipSlot per material, in MaterialRec::tex order (the opacity map is only ever tapped at
// level 0); an unused slot is {0, 1}.
struct MipSlot {
    uint32_t first;  // the level table entry of level 1
    int32_t levels;  // L = floor(log2(max(W0, H0))) + 1
};
// One texture in one launch of the generation: where the level before it and the new level are, and how many texels
// of the launch come before this texture's.
struct MipGen {
    uint32_t src, dst;  // first texel of either level in its buffer
    int32_t sw, sh, dw, dh;
    uint32_t first;
    uint32_t pad;
};
struct MipGenArgs {
    const MipGen* gen;  // the textures that have this level, `first` ascending
    int n;
    uint32_t n_out;       // texels of the launch
    const uint32_t* src;  // level 1: the upload's texel buffer; later levels: the chains'
    int64_t n_src;
    uint32_t* dst;
    int64_t n_dst;
};
hipError_t launch_generate_mip_level(const MipGenArgs& a, hipStream_t stream);

struct ResolveMipArgs {
    ResolveArgs r;  // r.linear is not read
    const MipSlot* slots;  // 5 * r.n_materials
    const MaterialTex* levels;
    int64_t n_levels;
    const uint32_t* mip_texels;
    int64_t n_mip_texels;
    float lod_bias;
};
hipError_t launch_resolve_materials_mip(const ResolveMipArgs& a, hipStream_t stream);

// ---- The anisotropic resolve (material_resolve.h; pbr_resolve_materials_aniso) -----------------------------------
// The trilinear call's arguments, unchanged, and the largest tap count of a sample.
struct ResolveAnisoArgs {
    ResolveMipArgs m;
    int32_t max_aniso;  // 1 .. 16
};
hipError_t launch_resolve_materials_aniso(const ResolveAnisoArgs& a, hipStream_t stream);

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
// pbr_raster_alpha_stats, pbr_raster_layer_stats; kRasterLarge: the large-triangle list's length). The first ten keep
// their slots.
enum RasterCounter { kRasterLarge = 0, kRasterCulled, kRasterZeroArea, kRasterNear, kRasterGuard, kRasterFragments,
                     kRasterClipped, kRasterClipPieces, kRasterAlphaTested, kRasterAlphaDiscarded,
                     kRasterLayerFragments, kRasterSlotPixels /* four words: pbr_msaa_stats */,
                     kRasterCounters = kRasterSlotPixels + 4 };

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
    // Appended for pbr_rasterize_layer (step 7a), read by the PEEL instantiations only. The three planes have the
    // targets' row stride and point at row `row_begin`; depth_in may be `depth`, prim_in may be prim_out.
    const float* depth_in;     // d_(k-1): a fragment is eligible only with z < depth_in
    const uint32_t* prim_in;   // the floor f_(k-1): ... and with an ordinal >= it; nullptr: 0 everywhere
    uint32_t* prim_out;        // f_k: the winner's ordinal + 1, 0xFFFFFFFF without a winner
    bool peel;         // a layer call: setup, large and resolve launch their PEEL instantiations (never with alpha_test)
};
// The stages of pbr_rasterize, each one launch (none when it has nothing to do): the vertex transform, the triangle
// setup with the small triangles' coverage, the large triangles' coverage, the per-pixel resolve. With a.clip_near
// each launches its near-clipping instantiation; with a.alpha_test the setup and the
// large-triangle stage launch their alpha-testing instantiations (step 6a); with a.peel the setup, the large-triangle
// stage and the resolve launch their layer instantiations (step 7a).
hipError_t launch_raster_vertices(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_setup(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_large(const RasterArgs& a, hipStream_t stream);
hipError_t launch_raster_resolve(const RasterArgs& a, hipStream_t stream);

// ---- Layer blend (blend_layer.h; pbr_blend_layer) -------------------------------------------------
// The output-merger blend of the transparent PSO (PBRApp.cpp:831-842): SRC_ALPHA / INV_SRC_ALPHA on colour, ONE / ZERO
// on alpha, of a shaded layer over a frame, on the pixels the layer covers.
struct BlendArgs {
    const float* src;         // RGBA32F, 4 floats per pixel
    const float* alpha;       // fp32 plane: the layer's opacity
    const uint8_t* coverage;  // the layer's coverage: 0 = the destination pixel is neither read nor written
    void* out;                // RGBA32F or RGBA8
    int64_t src_stride, out_stride;  // pixels
    int64_t alpha_stride, cov_stride;  // elements
    int width, height;
    int format;  // kBlendRgba32f / kBlendRgba8
    bool vec;    // src and (RGBA32F) out 16-byte aligned: one 16-byte access per pixel
};
constexpr int kBlendRgba32f = 0, kBlendRgba8 = 1;
hipError_t launch_blend_layer(const BlendArgs& a, hipStream_t stream);

// ---- Four samples per pixel (raster.h, msaa_resolve.h; pbr_msaa_*) -------------------------
// A multisampled call's arguments: those of a rasterisation (r.vis is not used; r.plane, r.material, r.depth and
// r.stride only by the fragments stage) and the caller's visibility surface: four planes, sample-major, of
// (r.row_end - r.row_begin) rows of vis_stride words.
struct MsaaArgs {
    RasterArgs r;
    unsigned long long* vis;
    int64_t vis_stride;    // words per row, >= r.width
    int slot;              // the fragments stage: 0 .. 3
    uint8_t* owner;        // the fragments stage: the owner plane, or nullptr
    int64_t owner_stride;  // bytes
};
// The sample-coverage instantiations of the setup and large-triangle stages, and the fragments stage that takes the
// resolve's place: one launch each (none when it has nothing to do).
hipError_t launch_msaa_setup(const MsaaArgs& a, hipStream_t stream);
hipError_t launch_msaa_large(const MsaaArgs& a, hipStream_t stream);
hipError_t launch_msaa_fragments(const MsaaArgs& a, hipStream_t stream);

// The multisample resolve of up to four shaded slot frames through the owner plane (pbr_msaa_resolve).
struct MsaaResolveArgs {
    const float* slots[4];  // RGBA32F frames; slots[k] is read only for k < n_slots
    int64_t slot_stride;    // pixels
    int n_slots;            // 1 .. 4
    const uint8_t* owner;
    int64_t owner_stride;   // bytes
    void* out;              // RGBA32F or RGBA8
    int64_t out_stride;     // pixels
    int width, height;
    int format;  // kBlendRgba32f / kBlendRgba8
    bool vec;    // every slot frame and (RGBA32F) out 16-byte aligned: one 16-byte access per pixel and frame
};
hipError_t launch_msaa_resolve(const MsaaResolveArgs& a, hipStream_t stream);

// PBR_DEBUG_BOUNDS builds only (pbr_debug_bounds.h): point this unit's kernels at the device's bounds-flag buffer.
hipError_t debug_bounds_publish_frontend(uint32_t* buf);

}  // namespace pbr
