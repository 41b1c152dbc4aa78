/*
 * pbr_shade.h -- C ABI of the MI355X (gfx950) G-buffer shading library, libpbrshade.so.
 *
 * Drop-in for the hot path of trevordblack/Physically_Based_Renderer: the per-pixel Cook-Torrance
 * pixel shader PS (Source/Shaders/Default.hlsl:47-161) and everything it calls in
 * Source/Shaders/LightingUtil.hlsl:35-225, which the reference runs by DrawIndexedInstanced
 * (Source/App/PBRApp.cpp:1133) inside PBRApp::Draw (PBRApp.cpp:245-352). The D3D12 rasteriser
 * front-end is replaced by a flat structure-of-arrays G-buffer the caller fills (pbr_gbuffer_fill
 * below does it on the host for the benchmark scenes).
 *
 * Conventions (mirroring the reference's HRESULT/ThrowIfFailed checking, d3dUtil.h:156-163):
 *   - every function returns int: 0 = PBR_OK, negative = pbr_status; no exception crosses the ABI;
 *   - the caller owns every buffer passed in; the library never frees them;
 *   - device work is stream-ordered and asynchronous on the hipStream_t given (NULL = default
 *     stream); a context is bound to one device and is reentrant across streams, like the
 *     reference's 3-deep frame-resource ring (FrameResource.h:111-140, PBRApp.cpp:220-243): every
 *     pbr_set_pass uploads into its own device light slot, a pass reads the slot of the
 *     pbr_set_pass before it and waits (stream-side) for that upload when it was made on another
 *     stream, and a slot or texture is overwritten only after the queued passes that read it, on
 *     whatever stream they run. Host calls on one context are serialised by its mutex; the host
 *     order of pbr_set_pass and pbr_shade_* calls decides which pass a shade uses. Contexts expect a
 *     small, long-lived set of streams: the first call on a new stream synchronises the device once,
 *     and past 16 streams the context forgets all but its last one then. Let a stream's passes
 *     finish before destroying it (a new stream may reuse its handle value). A light slot or
 *     texture that grows (more lights than the slot held, a larger map) is released and
 *     reallocated in stream order on the calling stream (hipFreeAsync / hipMallocAsync after
 *     stream-side waits for its readers): no device synchronisation. pbr_set_env_map and
 *     pbr_set_sky_map synchronise their own stream (the host texels may be released on return),
 *     and pbr_set_pass may wait on the host for the upload that last used its staging slot: call
 *     them outside a graph capture. pbr_shade_* on a stream the context already knows queues only
 *     stream-ordered work (event records and waits, the kernel).
 * Plain C types only (hipStream_t is passed as void*).
 */
#ifndef PBR_SHADE_H
#define PBR_SHADE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBR_ABI_VERSION 9
#define PBR_MAX_LIGHTS 4096 /* the reference's cbuffer holds MAX_LIGHTS = 16 (LightingUtil.hlsl:7) */

typedef enum pbr_status {
    PBR_OK = 0,
    PBR_ERR_INVALID_ARGUMENT = -1,
    PBR_ERR_NO_DEVICE = -2,
    PBR_ERR_OUT_OF_MEMORY = -3,
    PBR_ERR_LAUNCH = -4,
    PBR_ERR_HIP = -5,
    PBR_ERR_NOT_READY = -6, /* shade called before pbr_set_pass / IBL without pbr_set_env_map */
    PBR_ERR_UNSUPPORTED = -7
} pbr_status;

/* One light, byte-identical to the reference cbuffer element `Light` (LightingUtil.hlsl:9-17,
 * C++ mirror d3dUtil.h:144-152): 48 bytes, float4-aligned. Lights of a pass are ordered
 * directional [0, n_dir), point [n_dir, n_dir+n_point), spot [.., +n_spot) as ComputeLighting
 * expects (LightingUtil.hlsl:176-199). */
typedef struct pbr_light {
    float strength[3];
    float spot_power;   /* spot only */
    float direction[3]; /* directional / spot only */
    float pad0;
    float position[3];  /* point / spot only */
    float pad1;
} pbr_light;

typedef enum pbr_ambient_mode {
    PBR_AMBIENT_CONSTANT = 0,   /* g_AmbientLight * albedo: the active reference code, Default.hlsl:150 */
    PBR_AMBIENT_IBL_DIFFUSE = 1 /* the diffuse-IBL block of Default.hlsl:140-149 (commented out there) */
} pbr_ambient_mode;

enum pbr_pass_flags {
    PBR_FLAG_F0_PLANE = 1u << 0,    /* F0 from the G-buffer (SPECULAR_TEXTURE permutation, Default.hlsl:91-92);
                                       otherwise F0 = lerp(fresnel_r0, albedo, metallic) (Default.hlsl:94-95) */
    PBR_FLAG_APPLY_AO = 1u << 1,    /* extension: ambient *= AO. The reference never reads its AO slot. */
    PBR_FLAG_TILED_CULLING = 1u << 2, /* per-tile range culling of point/spot lights; output is
                                         bit-identical to the unculled pass ("exact culling") */
    PBR_FLAG_EXACT_ONLY = 1u << 3,    /* validation mode: never take the exact fast division/sqrt path
                                         ("exact fast path"); output is bit-identical, slower */
    PBR_FLAG_FAITHFUL = 1u << 4,      /* tolerance mode (ABI 4): the well-conditioned divisions of the BRDF
                                         (NDF, Smith G1(N.L), specular denominator, diffuse / PI,
                                         attenuation) use the hardware reciprocal (<= 1 ulp) instead of
                                         correct rounding; the ill-conditioned GGX chain and Fresnel stay
                                         exact. Output within 1e-5 relative of the reference evaluation
                                         (the north-star bar; bound 6.1e-6, tiled and wave-balanced passes
                                         6.4e-6; measured 6.3e-7), not bit-identical.
                                         Applies where every light term is >= 0 and the sum is short:
                                         <= 64 lights (with PBR_FLAG_TILED_CULLING: <= 64 surviving lights,
                                         counted per wave), every strength component of every light 0 or in
                                         [2^-25, 2^50] (outside it a product of the rearranged term underflows
                                         or the reference's own overflows to NaN), a constant ambient and
                                         env texels in [0, 2^100] (checked on the host), albedo
                                         >= 0 and F0 in [0, 1] (checked per wave); elsewhere the pass stays
                                         exact. */
    PBR_FLAG_ALPHA_TEST = 1u << 5     /* ABI 6: the ALPHA_TEST permutation (alphaTestedPS, PBRApp.cpp:750-765,
                                         Default.hlsl:111-113): fragOpacity = the G-buffer's opacity plane;
                                         a pixel with fragOpacity - 0.1f < 0 is discarded (its output is left
                                         untouched), others get alpha = fragOpacity. Sky pixels are not tested. */
};

/* Per-frame constants: the shading subset of cbPass (Core.hlsl:35-61, FrameResource.h:19-44) and
 * cbMaterial (Core.hlsl:64-81, Material.h:10-29). */
typedef struct pbr_pass_desc {
    float eye_pos_w[3];     /* g_CameraPosW */
    float ambient_light[3]; /* g_AmbientLight.rgb */
    float fresnel_r0[3];    /* g_FresnelR0 (default 0.04) */
    float opacity;          /* g_Opacity -> output alpha (default 1) */
    int32_t num_dir_lights;   /* NUM_DIR_LIGHTS   (Core.hlsl:1-3)  */
    int32_t num_point_lights; /* NUM_POINT_LIGHTS (Core.hlsl:5-7)  */
    int32_t num_spot_lights;  /* NUM_SPOT_LIGHTS  (Core.hlsl:9-11) */
    int32_t ambient_mode;     /* pbr_ambient_mode */
    uint32_t flags;           /* pbr_pass_flags */
    const pbr_light* lights;  /* HOST pointer, num_dir+num_point+num_spot lights */
} pbr_pass_desc;

/* Structure-of-arrays G-buffer in DEVICE memory: one fp32 plane per channel, `row_stride`
 * elements between rows. Replaces the interpolated VertexOut + texture fetches of PS
 * (Default.hlsl:12-20, 79-116): N is the final (normal-mapped) normal, F0 optional. */
typedef struct pbr_gbuffer_soa {
    const float* pos_w[3];    /* PosW x, y, z */
    const float* normal_w[3]; /* N x, y, z */
    const float* albedo[3];   /* diffuseAlbedo r, g, b */
    const float* metallic;
    const float* roughness;
    const float* ao;          /* read only with PBR_FLAG_APPLY_AO; may be NULL otherwise */
    const float* f0[3];       /* read only with PBR_FLAG_F0_PLANE; may be NULL otherwise */
    int32_t width;
    int32_t height;
    int64_t row_stride;       /* elements; >= width */
    const float* opacity;     /* ABI 6: read only with PBR_FLAG_ALPHA_TEST (the opacity map, Default.hlsl:112);
                                 may be NULL otherwise */
} pbr_gbuffer_soa;

typedef struct pbr_context pbr_context;

/* Replaces device creation + root signature / PSO build (d3dApp.cpp:437-501, PBRApp.cpp:607-650,
 * 776-881). `device` is a HIP device ordinal. */
int pbr_context_create(int device, pbr_context** out_ctx);
int pbr_context_destroy(pbr_context* ctx);

/* Replaces UpdateMainPassCB + UploadBuffer::CopyData (PBRApp.cpp:455-502, UploadBuffer.h:53):
 * uploads the light list and constants, stream-ordered; `pass` may be reused on return. */
int pbr_set_pass(pbr_context* ctx, const pbr_pass_desc* pass, void* stream);

/* Replaces loading + binding the environment SRV (PBRApp.cpp:1205-1210, t0-t1): an R16G16B16A16_UNORM
 * texture, `texels` = HOST pointer to width*height*4 u16, row-major. Sampled with linear-wrap
 * filtering (g_SamLinearWrap, PBRApp.cpp:1157-1162) by the IBL_DIFFUSE ambient. */
int pbr_set_env_map(pbr_context* ctx, const uint16_t* texels, int32_t width, int32_t height, void* stream);

/* Replaces DrawIndexedInstanced(PS) (PBRApp.cpp:1133, Default.hlsl:47-161): shades every pixel of
 * `gb` with the current pass into `out_rgba` (DEVICE, fp32 RGBA, out_row_stride PIXELS between rows).
 * Asynchronous on `stream`. Pixels are independent, so a caller can shade a row band by offsetting
 * the plane pointers (multi-GPU row tiles). */
int pbr_shade_gbuffer(pbr_context* ctx, const pbr_gbuffer_soa* gb, float* out_rgba, int64_t out_row_stride,
                      void* stream);

/* ---- Frame composition: sky pass, output format, HDR textures (ABI 2) -------------------------- */

/* Output pixel formats. RGBA32F is what pbr_shade_gbuffer writes. RGBA8_UNORM is the reference's
 * back buffer (DXGI_FORMAT_R8G8B8A8_UNORM, d3dApp.h:124; presented by PBRApp::Draw, PBRApp.cpp:274-279),
 * converted with the D3D FLOAT -> UNORM rule: NaN -> 0, clamp to [0, 1], c * 255 + 0.5, truncate. */
typedef enum pbr_output_format {
    PBR_OUTPUT_RGBA32F = 0,
    PBR_OUTPUT_RGBA8_UNORM = 1
} pbr_output_format;

typedef struct pbr_frame_desc {
    void* out;                   /* DEVICE: RGBA32F 16 B/px (16-byte aligned) or RGBA8 4 B/px (4-byte aligned) */
    int64_t out_row_stride;      /* pixels between output rows, >= width */
    int32_t format;              /* pbr_output_format */
    int32_t pad0;
    /* Optional DEVICE coverage plane, one byte per pixel, `coverage_row_stride` bytes per row:
     * nonzero = geometry (shaded by PS, Default.hlsl:47-161); 0 = background, which gets the sky pass
     * of Skybox.hlsl:37-49 instead (the reference draws the sky dome where no geometry wrote depth,
     * PBRApp.cpp:319-320, 856-875). For a background pixel the G-buffer normal planes hold the sky
     * sample direction (the sky dome's interpolated local position, Skybox.hlsl:24); its other planes
     * are not used. NULL = every pixel is geometry. */
    const uint8_t* coverage;
    int64_t coverage_row_stride;
} pbr_frame_desc;

/* The sky texture g_SkyArray[0] (PBRApp.cpp:1200-1204, sampled by Skybox.hlsl:45 with g_SamLinearWrap):
 * R16G16B16A16_UNORM, HOST texels as pbr_set_env_map. Required when a frame has background pixels. */
int pbr_set_sky_map(pbr_context* ctx, const uint16_t* texels, int32_t width, int32_t height, void* stream);

/* fp32 RGBA variants of pbr_set_env_map / pbr_set_sky_map (HOST width*height*4 floats, e.g. a decoded
 * RGBE .hdr environment, Assets/<set>/<set>_Env.hdr): the texels are used as given, no UNORM decode. */
int pbr_set_env_map_f32(pbr_context* ctx, const float* texels, int32_t width, int32_t height, void* stream);
int pbr_set_sky_map_f32(pbr_context* ctx, const float* texels, int32_t width, int32_t height, void* stream);

/* pbr_shade_gbuffer with the frame options above, in one pass over the G-buffer (the sky and the
 * format conversion are fused into the shading kernel). Asynchronous on `stream`. */
int pbr_shade_frame(pbr_context* ctx, const pbr_gbuffer_soa* gb, const pbr_frame_desc* frame, void* stream);

/* Tiled-culling statistics of the last pass on `stream` (synchronises that stream; see
 * pbr_last_pass_stats for which pass), zeros when that pass did not cull:
 * total surviving point/spot lights summed over the culling tiles that hold geometry, and the number
 * of those tiles. A culling tile is one wave64's pixels (64x2 in the default pixel-pair layout, 32x8
 * workgroups in the one-pixel layout). The kernel writes per-workgroup counts (no atomics); this
 * call sums them on the host. */
int pbr_last_cull_stats(pbr_context* ctx, int64_t* sum_tile_lights, int64_t* num_tiles, void* stream);

/* Statistics of the last shading pass of the context (new; the reference has no counterpart). */
typedef struct pbr_pass_stats {
    int64_t workgroups;       /* workgroups of the pass (64x8-pixel tiles; 32x8 in the one-pixel layout) */
    int64_t culled;           /* 1 when the pass ran tiled culling, else 0 */
    int64_t cull_tiles;       /* culling tiles with geometry (0 without culling) */
    int64_t cull_tile_lights; /* surviving point/spot lights summed over those tiles (0 without culling) */
    int64_t exact_pixels;     /* geometry pixels whose light sum the exact path re-evaluated (inputs or
                                 intermediates outside the fast-path window; every geometry pixel with
                                 PBR_FLAG_EXACT_ONLY) */
    /* ABI 5: the work the light loops executed (what a FLOP count of the pass may credit). */
    int64_t light_terms;      /* (geometry pixel, light) terms evaluated: every light of the pass in the
                                 uniform loop, the survivors of the culling tile under PBR_FLAG_TILED_CULLING,
                                 the live (front-facing, in the wave-balanced lists) point lights plus the
                                 directional ones in a wave-balanced pass. The exact re-pass of
                                 exact_pixels is not counted. */
    int64_t geometry_pixels;  /* pixels shaded by PS (the coverage plane's non-zero pixels; all without one) */
    int64_t backface_tests;   /* wave-balanced passes: (pixel, point light) back-face tests of the list
                                 build (4 FMAs each); 0 otherwise */
} pbr_pass_stats;

/* Fill *out with the statistics of the last pbr_shade_gbuffer / pbr_shade_frame call on `stream`
 * (synchronises `stream`). Each stream keeps its own record, so passes on other streams never mix
 * into it; if the context has not shaded on `stream`, the context's last pass on any stream is
 * reported, and `stream` must then be ordered after that pass. All zero before the first pass.
 * The kernel writes one record per wave (workgroup in the one-pixel layout); this call sums them. */
int pbr_last_pass_stats(pbr_context* ctx, pbr_pass_stats* out, void* stream);

/* ABI 7: the kernel the last pass on `stream` launched (the same fallback as pbr_last_pass_stats), as the
 * profiler names it without its argument list, e.g. "shade_tile_kernel<1, false, false, false, 1>"
 * (the wave-balanced faithful lists) or "shade_lean_kernel<0, true, false, true, true>"; "" before the first
 * pass. The string is owned by the context and stays valid until the next pass on that stream. */
const char* pbr_last_pass_kernel(pbr_context* ctx, void* stream);

/* ABI 8: the bounds-checked kernel build (PBR_DEBUG_BOUNDS=1: `make -C physically_based_renderer_amd/csrc
 * debug-bounds`: physically_based_renderer_amd/_lib/debug_bounds/libpbrshade.so), the analogue of the reference's D3D12 debug layer
 * (d3dApp.cpp:443-444). Its kernels check every G-buffer, output, coverage, texel and light index (and the
 * wave-balanced lists' LDS indices) against the launch's extents; a violation is recorded, not trapped, and the
 * access is redirected to index 0. Synchronises the context's device, then copies its flags into `flags`
 * (16 words, may be NULL): flags[c] != 0 when index class c was violated (0 G-buffer, 1 output, 2 coverage,
 * 3 texel, 4 light, 5 LDS list), flags[8 + c] the last offending index; `reset` != 0 clears them. Every pass since
 * the first context on the device (or the last reset) counts. PBR_ERR_UNSUPPORTED from a product build. */
int pbr_debug_bounds(pbr_context* ctx, uint32_t* flags, int reset);

/* ---- Device material resolve: interpolated attributes + material textures -> G-buffer ----------
 * The first half of PS (Default.hlsl:50-116): normalize(pin.NormalW), the material texture fetches behind the
 * *_TEXTURE permutation defines, the F0 resolve, NormalSampleToWorldSpace and the ALPHA_TEST opacity fetch, run on
 * the device so that a caller with real geometry hands over its interpolated VertexOut (Default.hlsl:12-20) and gets
 * a pbr_gbuffer_soa back without a host round trip.
 * These entry points are additive: PBR_ABI_VERSION stays 9, and a caller that may meet an older library detects them
 * by symbol (dlsym), as for pbr_last_pass_kernel. */

enum pbr_material_flags { /* a permutation's defines (Default.hlsl:79-116, PBRApp.cpp:892-963) as bits */
    PBR_MAT_DIFFUSE_TEXTURE = 1u << 0,   /* DIFFUSE_TEXTURE:   albedo    = tex[0].rgb, else diffuse_albedo */
    PBR_MAT_SPECULAR_TEXTURE = 1u << 1,  /* SPECULAR_TEXTURE:  F0        = tex[1].rgb, else lerp(fresnel_r0, albedo, metallic) */
    PBR_MAT_METALLIC_TEXTURE = 1u << 2,  /* METALLIC_TEXTURE:  metallic  = tex[2].r,   else metallic */
    PBR_MAT_ROUGHNESS_TEXTURE = 1u << 3, /* ROUGHNESS_TEXTURE: roughness = tex[3].r,   else roughness */
    PBR_MAT_NORMAL_TEXTURE = 1u << 4,    /* NORMAL_TEXTURE:    N = NormalSampleToWorldSpace(tex[4].rgb, ...), else NormalW */
    PBR_MAT_ALPHA_TEST = 1u << 5         /* ALPHA_TEST:        opacity   = tex[5].r (always point-wrap, Default.hlsl:112),
                                            else opacity */
};

#define PBR_MATERIAL_NONE 0xFFFFu /* material id of a background pixel (any id >= the table's count is one too) */

/* One material: the members of cbMaterial PS reads before the light loop (Core.hlsl:64-81, Material.h:10-29) and
 * the permutation it is drawn with. tex[k] indexes the texture list of pbr_set_materials (the reference's
 * g_TextureArray slots 0-4 and 11, Default.hlsl:80-112); -1 = unused. */
typedef struct pbr_material {
    float diffuse_albedo[3]; /* g_DiffuseAlbedo */
    float metallic;          /* g_Metallic */
    float fresnel_r0[3];     /* g_FresnelR0 */
    float roughness;         /* g_Roughness */
    float opacity;           /* g_Opacity */
    uint32_t flags;          /* pbr_material_flags */
    int32_t tex[6];          /* diffuse, specular, metallic, roughness, normal, opacity */
} pbr_material;

/* A UNORM8 texture in HOST memory: width*height*channels bytes, row-major, 1, 3 or 4 channels
 * (a 1-channel texture read as .rgb replicates .r). A texel decodes as (float)u8 / 255.0f. */
typedef struct pbr_texture_desc {
    const uint8_t* texels;
    int32_t width;
    int32_t height;
    int32_t channels;
    int32_t pad0;
} pbr_texture_desc;

/* Texture filters of the resolve. The reference samples its material maps with g_SamAnisotropicWrap
 * (Default.hlsl:80-105); anisotropic filtering stays parity-unpinned, so the caller picks one of
 * the two filters this library pins bit for bit. */
typedef enum pbr_texture_filter {
    PBR_FILTER_POINT = 0, /* texel (wrap(floorf(u * W)), wrap(floorf(v * H))) */
    PBR_FILTER_LINEAR = 1 /* the linear-wrap bilinear of the environment lookup, per channel */
} pbr_texture_filter;

/* Uploads the material table and its textures (replaces BuildMaterials / LoadTextures, PBRApp.cpp:892-963,
 * 1196-1463). Same rules as pbr_set_env_map: the host data may be released on return, the previous table is
 * released only after the queued resolves that read it (on any stream), call it outside a graph capture.
 * PBR_ERR_INVALID_ARGUMENT: a flag whose tex slot is -1 or >= n_textures, channels not 1, 3 or 4, a non-positive
 * texture size, n_materials >= 0xFFFF. */
int pbr_set_materials(pbr_context* ctx, const pbr_material* materials, int32_t n_materials,
                      const pbr_texture_desc* textures, int32_t n_textures, void* stream);

/* The interpolated VertexOut (Default.hlsl:12-20) per pixel, DEVICE planes, plus the material id of the object
 * that covers the pixel. One `row_stride` (elements) for all fifteen planes. */
typedef struct pbr_attributes_soa {
    const float* pos_w[3];       /* PosW */
    const float* normal_w[3];    /* NormalW, not normalised (a background pixel: the sky direction) */
    const float* tangent_w[3];   /* TangentW */
    const float* bitangent_w[3]; /* BitangentW */
    const float* tex_coord[2];   /* TexCoord */
    const uint16_t* material;    /* index into the material table; PBR_MATERIAL_NONE = background */
    int32_t width;
    int32_t height;
    int64_t row_stride;          /* elements; >= width */
} pbr_attributes_soa;

/* Where the resolve writes: the 15 planes of a pbr_gbuffer_soa (pos xyz, normal xyz, albedo rgb, metallic,
 * roughness, ao, f0 rgb), the opacity plane and the coverage bytes pbr_shade_frame consumes. DEVICE memory. */
typedef struct pbr_gbuffer_targets {
    float* planes[15];
    float* opacity;              /* may be NULL */
    uint8_t* coverage;           /* may be NULL; 1 = geometry, 0 = background */
    int64_t row_stride;          /* elements, planes and opacity; >= width */
    int64_t coverage_row_stride; /* bytes; >= width when coverage is given */
} pbr_gbuffer_targets;

/* Default.hlsl:50-116 for every pixel of `attrs` into `targets`, asynchronously on `stream`; `filter` is a
 * pbr_texture_filter. Position passes through, AO is 1, the F0 plane is always written (shade the result with
 * PBR_FLAG_F0_PLANE: one pass then carries objects of different permutations). A background pixel gets its
 * NormalW unchanged in the normal planes, albedo 0, metallic 0, roughness 1, F0 0.04, opacity 1, coverage 0, and
 * reads no table entry or texel. Rows are independent: a row band resolved through offset pointers equals the same
 * rows of the full frame. Not a shading pass: pbr_last_pass_stats / _kernel are unchanged by it.
 * PBR_ERR_NOT_READY before pbr_set_materials. */
int pbr_resolve_materials(pbr_context* ctx, const pbr_attributes_soa* attrs, const pbr_gbuffer_targets* targets,
                          int32_t filter, void* stream);

/* ---- Mip chains and the trilinear filter (additive: PBR_ABI_VERSION stays 9, detect by symbol) ----
 * The reference samples every material map with g_SamAnisotropicWrap over texture->Resource->GetDesc().MipLevels
 * levels (PBRApp.cpp:701, :1171-1178; Default.hlsl:80-105). The isotropic trilinear filter over chains this library
 * builds itself is pinned bit for bit ("Mip chains and the trilinear filter", which fixes every
 * operation); the anisotropic filter over the same chains is pbr_resolve_materials_aniso below, pinned the same way.
 *
 * pbr_generate_mips builds the chains of every texture of the current material table on the device, the counterpart of
 * the mips a DDS carries or a loader generates. Level 0 is the uploaded texture; level l >= 1 is
 * max(1, W_(l-1) >> 1) x max(1, H_(l-1) >> 1), down to 1 x 1, each byte channel (alpha included) of a texel
 * (a + b + c + d + 2) >> 2 of the texels of level l-1 at columns 2x, min(2x+1, W_(l-1)-1) and rows 2y,
 * min(2y+1, H_(l-1)-1), from the stored bytes of that level. The chains belong to the table they were built from: a
 * later pbr_set_materials invalidates them. Same rules as pbr_set_materials: the previous chains are released only
 * after the queued resolves that read them (on any stream), `stream` is synchronised before the call returns, call it
 * outside a graph capture. PBR_ERR_NOT_READY before pbr_set_materials. */
int pbr_generate_mips(pbr_context* ctx, void* stream);

/* pbr_resolve_materials with the trilinear filter on the five material maps (diffuse, specular, metallic, roughness,
 * normal); the PBR_MAT_ALPHA_TEST opacity stays the level-0 point-wrap tap, everything else is pbr_resolve_materials's.
 * For a geometry pixel (x, y) of the call with material m: the horizontal partner is (x^1, y), the vertical one
 * (x, y^1); a partner is valid when it lies inside the call's width and height and its material id is m. dudx, dvdx =
 * u, v at (x|1, y) minus at (x&~1, y), dudy, dvdy = at (x, y|1) minus at (x, y&~1); an invalid partner makes its pair
 * +0 (no helper pixels across a silhouette or a material edge: level 0, the sharp choice). Per sampled texture of
 * W x H texels and L levels: r2 = max((dudx W)^2 + (dvdx H)^2, (dudy W)^2 + (dvdy H)^2); lod = (r2 > 1 ? 0.5 *
 * (exponent(r2) + mantissa(r2) * 2^-23) : 0) + lod_bias, clamped to [0, L-1]; the result is the lerp, by lod's
 * fraction, of PBR_FILTER_LINEAR's bilinear at levels floor(lod) and min(floor(lod) + 1, L-1). With lod 0 it is
 * PBR_FILTER_LINEAR's result bit for bit.
 * Quads are aligned to the call's row 0 and column 0: a row band resolved through offset pointers equals the same
 * rows of the full frame iff it starts on an even frame row and has an even height or ends with the frame.
 * PBR_ERR_NOT_READY before pbr_generate_mips, and again after a pbr_set_materials until the chains are generated
 * anew; PBR_ERR_INVALID_ARGUMENT also for a lod_bias that is NaN or infinite. */
int pbr_resolve_materials_mip(pbr_context* ctx, const pbr_attributes_soa* attrs, const pbr_gbuffer_targets* targets,
                              float lod_bias, void* stream);

/* ---- Anisotropic filter (additive: PBR_ABI_VERSION stays 9, detect by symbol) ----
 * pbr_resolve_materials_mip with the anisotropic filter on the five material maps (the reference's sampler is
 * D3D12_FILTER_ANISOTROPIC with maxAnisotropy = 8, PBRApp.cpp:1171-1178); DESIGN.md §11, "Anisotropic filter", fixes
 * every operation. Partners, validity, dudx, dvdx, dudy, dvdy, quad alignment and the band rule are
 * pbr_resolve_materials_mip's; the PBR_MAT_ALPHA_TEST opacity stays the level-0 point-wrap tap. Per sampled texture of
 * W x H texels and L levels, with M = max_anisotropy, in fp32, every operation rounded once:
 *   rx = (dudx W)^2 + (dvdx H)^2, ry = (dudy W)^2 + (dvdy H)^2; ymajor = ry > rx (false for NaN);
 *   pmax2, pmin2 = the larger and the smaller of the two; (du, dv) = (dudy, dvdy) when ymajor, else (dudx, dvdx).
 *   N = 1; for k = 1 .. M-1 ascending: if pmax2 > (float)(k k) * pmin2 then N = k + 1 -- the smallest n with
 *   pmax2 <= n^2 pmin2, at most M; NaN gives 1, both lengths zero give 1, a zero minor axis under a non-zero major
 *   one gives M.
 *   r2 = N > 1 ? pmax2 / (float)(N N) : pmax2; lod, the levels l0 and l1 and the fraction f from r2 as in
 *   pbr_resolve_materials_mip.
 *   Taps: N == 1: (u, v) itself; else for i = 0 .. N-1: t_i = (float)(2 i + 1 - N) / (float)(2 N),
 *   (u + t_i * du, v + t_i * dv).
 *   Per level l of (l0, l1): s_l = PBR_FILTER_LINEAR's bilinear of level l at tap 0, plus tap 1, ..., plus tap N-1, in
 *   that order; c_l = N > 1 ? s_l / (float)N : s_l. The sample is c_l0 + f * (c_l1 - c_l0); level l1 is not read when
 *   f == 0.
 * With max_anisotropy = 1, and at any pixel and texture where N == 1, the result is pbr_resolve_materials_mip's bit for
 * bit. The major axis is the longer of the two screen-axis footprints (the form of GL's anisotropic-filter extension),
 * not the major axis of the footprint ellipse.
 * PBR_ERR_INVALID_ARGUMENT for max_anisotropy outside 1 .. 16 (D3D12's range) and for a lod_bias that is NaN or
 * infinite; PBR_ERR_NOT_READY as pbr_resolve_materials_mip. */
int pbr_resolve_materials_aniso(pbr_context* ctx, const pbr_attributes_soa* attrs, const pbr_gbuffer_targets* targets,
                                float lod_bias, int32_t max_anisotropy, void* stream);

/* ---- Device rasteriser: indexed triangle meshes -> interpolated attributes ----------------------
 * VS (Default.hlsl:22-45) and the fixed-function rasteriser behind DrawIndexedInstanced (PBRApp.cpp:1133) under the
 * reference's PSO state (CD3DX12_RASTERIZER_DESC(D3D12_DEFAULT), CD3DX12_DEPTH_STENCIL_DESC(D3D12_DEFAULT),
 * PBRApp.cpp:793-795; CULL_MODE_NONE for the transparent, alpha-tested and sky PSOs, :843-859), on the device: indexed
 * triangle lists in, the planes of a pbr_attributes_soa out, which pbr_resolve_materials consumes (which
 * fixes the semantics operation by operation: top-left rule on an 8-bit subpixel grid, one sample per pixel, depth
 * test LESS against a buffer cleared to 1, perspective-correct attributes). pbr_rasterize does not clip: a triangle with
 * a vertex whose w is not > 0 is skipped whole. pbr_rasterize_flags with PBR_RASTER_CLIP_NEAR clips every triangle
 * against the near plane z = 0 first, as the fixed-function pipeline does, so a floor under the eye, a wall beside it
 * or a sphere around it are drawn; the far plane stays a per-fragment test. Additive like the
 * resolve: PBR_ABI_VERSION stays 9, detect by symbol. */

/* One mesh in HOST memory: vertices in the reference's `Vertex` order (FrameResource.h:46-52), 14 floats each (Pos 3,
 * Normal 3, Tangent 3, Bitangent 3, TexCoord 2), and a triangle list of 32-bit indices. */
typedef struct pbr_mesh_desc {
    const float* vertices;   /* n_vertices * 14 floats */
    const uint32_t* indices; /* n_indices, each < n_vertices */
    int32_t n_vertices;
    int32_t n_indices;
} pbr_mesh_desc;

/* Uploads the meshes pbr_rasterize draws from (replaces BuildShapeGeometry's vertex / index buffer uploads). Same
 * rules as pbr_set_materials: the host data may be reused on return, the previous set is released in stream order
 * after the queued rasterisations that read it (on any stream), call it outside a graph capture.
 * PBR_ERR_INVALID_ARGUMENT: a null pointer (of a non-empty array), a negative count, an index >= n_vertices (the
 * indices are validated here, once, on the host). */
int pbr_set_meshes(pbr_context* ctx, const pbr_mesh_desc* meshes, int32_t n_meshes, void* stream);

/* One render item (RenderItem + DrawIndexedInstanced, PBRApp.cpp:1103-1134). Matrices are row-major and multiply a
 * row vector from the right, as mul(v, M) does in Default.hlsl:27-42. */
typedef struct pbr_draw {
    int32_t mesh;        /* index into the set of pbr_set_meshes */
    int32_t first_index; /* StartIndexLocation */
    int32_t index_count; /* IndexCount: a multiple of 3, first_index + index_count <= the mesh's n_indices */
    uint16_t material;   /* written to the material plane where the draw is visible */
    uint16_t cull;       /* 0 = back faces culled (D3D12_DEFAULT), 1 = none */
    float world[16];         /* g_World */
    float tex_transform[16]; /* g_TexTransform */
    float mat_transform[16]; /* g_MatTransform */
} pbr_draw;

typedef struct pbr_raster_view {
    float view_proj[16]; /* g_ViewProj; depth 0..1 */
    int32_t width;       /* the full frame: pixel values depend on the global (x, y) only */
    int32_t height;
    int32_t row_begin;   /* the targets hold rows [row_begin, row_end) of the frame */
    int32_t row_end;
    /* Background pixels (no fragment) get the layout pbr_attributes_fill gives them: with sx = (2x+1)/width - 1 and
     * sy = 1 - (2y+1)/height, d = normalize(bg_forward + sx * bg_right + sy * bg_up) in the normal planes and
     * eye + 100 d in the position planes (bg_right and bg_up carry the tangent of the half field of view). */
    float eye[3];
    float bg_right[3];
    float bg_up[3];
    float bg_forward[3];
} pbr_raster_view;

/* Where the rasteriser writes, DEVICE memory: the 14 planes of a pbr_attributes_soa in its order, the material id
 * plane, and optionally the depth plane (z of the visible fragment, 1 for the background). One row stride; plane
 * pointers point at row `row_begin`. */
typedef struct pbr_raster_targets {
    float* planes[14];
    uint16_t* material;
    float* depth;       /* may be NULL */
    int64_t row_stride; /* elements; >= width */
} pbr_raster_targets;

/* Rasterises `draws` in order into `targets`, asynchronously on `stream`; `draws` may be reused on return. Every pixel
 * of the band is written. The result is independent of execution order (nearest z wins, equal z goes to the earlier
 * triangle in draw order then index order) and of the band: a band equals the same rows of the full frame. Not a
 * shading pass: pbr_last_pass_stats / _cull_stats / _kernel are unchanged by it.
 * PBR_ERR_NOT_READY before pbr_set_meshes; PBR_ERR_INVALID_ARGUMENT for a bad mesh id or index range, an index_count
 * that is no multiple of 3, a cull mode other than 0 or 1, more than 2^32 - 2 triangles in the call. */
int pbr_rasterize(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                  const pbr_raster_targets* targets, void* stream);

typedef struct pbr_raster_stats {
    int64_t triangles;          /* submitted */
    int64_t backface_culled;    /* signed area < 0 under cull 0 */
    int64_t zero_area;          /* signed area == 0 on the subpixel grid */
    int64_t skipped_near;       /* a vertex whose w is not > 0: not drawn. Under PBR_RASTER_CLIP_NEAR: triangles with
                                 * every vertex in front of z = 0, and triangles or pieces left with such a vertex */
    int64_t skipped_guard_band; /* a vertex beyond +-2^23 subpixels, or not finite: not drawn */
    int64_t fragments;          /* (triangle, pixel) pairs that passed coverage and 0 <= z < 1 */
} pbr_raster_stats;

/* The counters of the last pbr_rasterize on `stream` (synchronises `stream`, like pbr_last_cull_stats); zeros when
 * the context has not rasterised on that stream. */
int pbr_last_raster_stats(pbr_context* ctx, pbr_raster_stats* out, void* stream);

/* pbr_rasterize with options. flags == 0 is pbr_rasterize, bit for bit, statistics included.
 * PBR_RASTER_CLIP_NEAR: a vertex is inside iff PosH.z >= 0 (NaN is outside, -0 inside). A triangle with three inside
 * vertices is drawn as by pbr_rasterize; one with none is counted in skipped_near; one with 1 or 2 is cut at z = 0
 * into 1 or 2 pieces, each new vertex computed along its edge from the inside end to the outside end (so that two
 * triangles sharing a crossing edge get the identical vertex and the clipped mesh stays watertight). A piece is then a
 * triangle like any other -- the w > 0 rule, viewport, guard band, area, culling, coverage and the counters of those
 * names apply to it -- except that it keeps its source triangle's place in the equal-depth order; `triangles` counts
 * source triangles, so triangles + clip_pieces - clipped_near = the triangles and pieces that reach coverage +
 * backface_culled + zero_area + skipped_near + skipped_guard_band. Arguments, stream rules, errors and scratch as pbr_rasterize; an unknown flag bit, or more than
 * 2^31 - 1 triangles in a clipping call: PBR_ERR_INVALID_ARGUMENT.
 * PBR_RASTER_ALPHA_TEST (RenderLayer::AlphaTested, PBRApp.cpp:308-311; clip(fragOpacity - 0.1f), Default.hlsl:111-113;
 * detect by the symbol pbr_last_raster_alpha_stats, PBR_ABI_VERSION stays 9): the fragments of every draw whose
 * `material` is below the table's count and whose pbr_material has PBR_MAT_ALPHA_TEST are tested before the depth
 * update: the fragment's TexCoord is interpolated as the resolve kernel does for the pixel, the opacity texture's texel
 * is the point-wrap tap pbr_resolve_materials takes, and with (float)red / 255.0f - 0.1f < 0.0f (bytes 0..25) the
 * fragment is discarded: it takes no part in the depth test, so whatever lies behind it, geometry or background, shows.
 * Fragments of other draws (a material id >= the table's count included) are never tested. Needs pbr_set_materials
 * (PBR_ERR_NOT_READY before it); the call reads the material table and the texels under pbr_resolve_materials's rules:
 * a later pbr_set_materials on any stream releases them after the queued rasterisations that read them.
 * pbr_raster_stats.fragments keeps counting discarded fragments. The flag combines with PBR_RASTER_CLIP_NEAR. Bit 1 is
 * not assigned: a flags word with it is refused like any unknown bit. */
enum { PBR_RASTER_CLIP_NEAR = 1u << 0, PBR_RASTER_ALPHA_TEST = 1u << 2 };
int pbr_rasterize_flags(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                        const pbr_raster_targets* targets, uint32_t flags, void* stream);

typedef struct pbr_raster_clip_stats {
    int64_t clipped_near; /* source triangles with 1 or 2 vertices in front of z = 0 */
    int64_t clip_pieces;  /* triangles emitted for them (1 or 2 each) */
} pbr_raster_clip_stats;

/* The clipping counters of the last rasterisation on `stream` (synchronises it, like pbr_last_raster_stats); zeros
 * after an unflagged call and when the context has not rasterised on that stream. */
int pbr_last_raster_clip_stats(pbr_context* ctx, pbr_raster_clip_stats* out, void* stream);

typedef struct pbr_raster_alpha_stats {
    int64_t alpha_tested;    /* fragments (coverage passed, 0 <= z < 1) of tested draws: those that reached the test */
    int64_t alpha_discarded; /* those the test killed: depth updates issued = fragments - alpha_discarded */
} pbr_raster_alpha_stats;

/* The alpha-test counters of the last rasterisation on `stream` (synchronises it, like pbr_last_raster_clip_stats);
 * zeros after a call without PBR_RASTER_ALPHA_TEST and when the context has not rasterised on that stream. */
int pbr_last_raster_alpha_stats(pbr_context* ctx, pbr_raster_alpha_stats* out, void* stream);

/* ---- The transparent layer: ordered peel and blend (RenderLayer::Transparent, PBRApp.cpp:313-316, 829-844) -------
 * The transparent PSO is the opaque one with CULL_MODE_NONE and blending: depth stays LESS with writes on, the pixel
 * shader stays opaquePS (no alpha test, output alpha g_Opacity). At one pixel the fragments of the transparent draws
 * arrive in primitive order; one with z below the depth buffer is blended over the colour and becomes the depth, every
 * other is dropped: the blended fragments are the strict running minima of z in primitive order. pbr_rasterize_layer
 * extracts that sequence one fragment per pixel per call: layer k is, per pixel, the fragment
 * with the smallest primitive ordinal among those with ordinal >= floor and z < depth_in; the call writes its
 * attributes, its z as the new depth and its ordinal + 1 as the next floor. Each layer goes through
 * pbr_resolve_materials and a shading call unchanged and is blended over the frame by pbr_blend_layer. Additive:
 * PBR_ABI_VERSION stays 9, detect by the symbol pbr_rasterize_layer. */
typedef struct pbr_raster_layer {
    const float* depth_in;   /* DEVICE, required: the depth before this layer (the opaque and alpha-tested layers' depth
                              * plane for the first layer, 1 where they drew nothing); the targets' row stride and band */
    const uint32_t* prim_in; /* DEVICE: the floor plane the previous layer wrote; NULL = 0 everywhere (the first layer) */
    uint32_t* prim_out;      /* DEVICE, required: the floor for the next layer */
} pbr_raster_layer;

/* One layer. Arguments as pbr_rasterize_flags, plus `layer`; targets->depth is required. targets->depth may alias
 * layer->depth_in and prim_out may alias prim_in: the coverage kernels only read the inputs, and the per-pixel resolve,
 * which runs after them in stream order, reads and writes only its own pixel. A fragment (coverage passed, 0 <= z < 1,
 * as for pbr_rasterize) is eligible iff its ordinal >= floor(x, y) and z < depth_in(x, y) (a NaN depth_in: never). A
 * pixel with an eligible fragment gets the attributes and material of the one with the smallest ordinal, its z in the
 * depth plane and its ordinal + 1 in prim_out. A pixel without one gets the background planes and PBR_MATERIAL_NONE (so
 * the resolve gives it coverage 0), depth_in's value passed through in the depth plane, and 0xFFFFFFFF in prim_out:
 * no later layer has an eligible fragment there. After the last layer the depth plane holds, bit for bit, what the
 * depth buffer holds after the reference's transparent pass. The ordinals are the call's own -- draw order, then
 * index order; the pieces of a clipped triangle share theirs -- so every layer of a sequence must pass the same draw
 * list. `flags`: PBR_RASTER_CLIP_NEAR is accepted; PBR_RASTER_ALPHA_TEST is refused with PBR_ERR_INVALID_ARGUMENT (the
 * transparent PSO runs no alpha test), as are unknown bits and bit 1. PBR_ERR_INVALID_ARGUMENT also for a null `layer`,
 * depth_in, prim_out or targets->depth, or one of the planes not 4-byte aligned. pbr_raster_stats keeps its meanings:
 * `fragments` counts coverage passed and 0 <= z < 1, eligible or not. */
int pbr_rasterize_layer(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                        const pbr_raster_targets* targets, uint32_t flags, const pbr_raster_layer* layer, void* stream);

typedef struct pbr_raster_layer_stats {
    int64_t layer_fragments; /* eligible fragments: the visibility updates issued. 0 = the layer is empty: stop */
} pbr_raster_layer_stats;

/* The layer counter of the last rasterisation on `stream` (synchronises it, like pbr_last_raster_stats); zeros after
 * a call other than pbr_rasterize_layer and when the context has not rasterised on that stream. */
int pbr_last_raster_layer_stats(pbr_context* ctx, pbr_raster_layer_stats* out, void* stream);

/* A shaded layer, DEVICE memory: its colour, its alpha and where it has fragments. */
typedef struct pbr_blend_source {
    const float* src;            /* RGBA32F, 4-byte aligned (16-byte aligned: one access per pixel); .a is not read */
    int64_t src_row_stride;      /* pixels, >= width */
    const float* alpha;          /* the opacity plane pbr_resolve_materials wrote (without an opacity map: the
                                  * material's `opacity`, g_Opacity, which opaquePS outputs as alpha) */
    int64_t alpha_row_stride;    /* elements, >= width */
    const uint8_t* coverage;     /* the coverage plane pbr_resolve_materials wrote for the layer */
    int64_t coverage_row_stride; /* bytes, >= width */
} pbr_blend_source;

/* The output-merger blend of the transparent PSO (PBRApp.cpp:831-842: colour SRC_ALPHA / INV_SRC_ALPHA, alpha
 * ONE / ZERO, both op ADD) of `source` over `dst` (out, out_row_stride and format are used; RGBA32F `out` may be only
 * 4-byte aligned here), width x height pixels, asynchronously on `stream`. Per pixel with nonzero coverage, with a the
 * alpha value and s the source colour: RGBA32F: out.c = (s.c * a) + (d.c * (1.0f - a)), each operation rounded once,
 * out.a = a. RGBA8_UNORM: d.c = (float)byte / 255.0f, s.c and a first clamped to [0, 1] with NaN -> 0 (the fixed-point
 * render-target rule), the same expression, all four results encoded with the FLOAT -> UNORM rule of pbr_output_format.
 * A pixel with coverage 0 is neither read nor written in `dst`. Not a shading pass: the pass statistics stay.
 * Departure from the reference: this blends over the finished opaque + sky frame. The reference draws its sky after
 * the transparent layer, so a transparent fragment over empty background blends there with the grey clear colour and
 * then hides the sky -- an artefact of its draw order that is not reproduced. */
int pbr_blend_layer(pbr_context* ctx, const pbr_blend_source* source, const pbr_frame_desc* dst, int32_t width,
                    int32_t height, void* stream);

/* ---- Four samples per pixel: sample coverage, fragments and the multisample resolve (m_4xMsaaState,
 * SampleDesc.Count = 4: PBRApp.cpp:800-801, d3dApp.cpp:202-203, :382-384, :540-541) -------------------------------
 * Vertices are snapped to 1/256 pixel and D3D's standard 4-sample positions are multiples of 1/16 pixel, so a sample
 * lies on the grid and its coverage is as exact as a pixel centre's. Sample s of pixel (x, y)
 * is at (x + 0.5 + dx_s / 16, y + 0.5 + dy_s / 16) with (dx, dy) = (-2, -6), (6, -2), (-6, 2), (2, 6). Coverage
 * (top-left rule), the interpolated z and the range test 0 <= z < 1 are pbr_rasterize's, evaluated at the sample; per
 * sample the nearest fragment wins, an equal z goes to the earlier triangle. The samples of a pixel that the same
 * triangle won are one *fragment*, as are those that nothing won (the background fragment): a pixel has 1 to 4
 * fragments, numbered as *slots* in the order of their lowest sample, so slot 0 owns sample 0. Shading is per pixel and
 * fragment: slot k's attributes are pbr_rasterize's interpolation for that triangle at the pixel CENTRE, inside the
 * triangle or not (no clamp, no centroid adjustment: D3D's default for inputs without `centroid`, which Default.hlsl
 * does not use). The caller hands every slot that exists to pbr_resolve_materials and a shading call, unchanged, and
 * pbr_msaa_resolve averages the four samples of each pixel. The pattern is D3D's standard one; the reference asks for
 * quality level m_4xMsaaQuality - 1, which is vendor-defined. Additive: PBR_ABI_VERSION stays 9, detect by the symbol
 * pbr_msaa_rasterize. */
typedef struct pbr_msaa_surface {
    uint64_t* visibility; /* DEVICE, 8-byte aligned: 4 planes, sample-major, of (row_end - row_begin) rows of row_stride
                           * words: word (s, y - row_begin, x) = (bits(z) << 32) | triangle ordinal of the fragment
                           * sample s of pixel (x, y) shows, all ones for none. The high word is the sample's depth. */
    int64_t row_stride;   /* words; >= width */
} pbr_msaa_surface;

/* Vertex stage, setup and per-sample coverage of `draws` into `surface`, asynchronously on `stream`. The call first
 * sets all 4 * rows * row_stride words of the surface to all ones, the padding words included. `flags` must be 0:
 * PBR_RASTER_CLIP_NEAR and PBR_RASTER_ALPHA_TEST return PBR_ERR_UNSUPPORTED; unknown bits and bit 1 are
 * PBR_ERR_INVALID_ARGUMENT, as are a NULL surface, a NULL or misaligned `visibility` and a row_stride below the width.
 * Otherwise arguments, readiness and stream rules are pbr_rasterize's, and the result is as independent of execution
 * order and of the band. pbr_last_raster_stats keeps its meanings, except that `fragments` counts (triangle, sample)
 * pairs. */
int pbr_msaa_rasterize(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                       uint32_t flags, const pbr_msaa_surface* surface, void* stream);

/* Slot `slot` (0 .. 3, else PBR_ERR_INVALID_ARGUMENT) of every pixel of the band out of `surface`, into `targets` as
 * pbr_rasterize writes them: the fragment's attributes at the pixel centre, its draw's material and, in the optional
 * depth plane, the high word of the key of the slot's lowest sample. A background fragment, and a slot the pixel does
 * not have, get the background planes, PBR_MATERIAL_NONE and depth 1. Every pixel of the band is written in every
 * call. `owner` (DEVICE, may be NULL; owner_row_stride bytes per row, >= width) receives per pixel
 * sum over s of slot(s) << 2s; it is the same for every slot. The call runs the vertex stage again, so `draws` and `view`
 * must be those of the pbr_msaa_rasterize call that filled the surface (a key whose ordinal is past the list is taken
 * as background). `flags` as pbr_msaa_rasterize. The counters of pbr_last_raster_stats stay those of the stream's last
 * rasterising call. */
int pbr_msaa_fragments(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                       uint32_t flags, const pbr_msaa_surface* surface, int32_t slot, const pbr_raster_targets* targets,
                       uint8_t* owner, int64_t owner_row_stride, void* stream);

typedef struct pbr_msaa_stats {
    int64_t slot_pixels[4]; /* pixels of the band in which slot k exists; [0] is the band's pixel count. A caller shades
                             * slots 0 .. the last k with slot_pixels[k] > 0 */
} pbr_msaa_stats;

/* Computed by every pbr_msaa_fragments call, whatever its slot (synchronises `stream`, like pbr_last_raster_stats);
 * zeros after any other rasterising call and when the context has not rasterised on that stream. */
int pbr_last_msaa_stats(pbr_context* ctx, pbr_msaa_stats* out, void* stream);

/* The shaded slots of a frame, DEVICE memory. */
typedef struct pbr_msaa_resolve_source {
    const float* slots[4];    /* RGBA32F frames, 4-byte aligned (all 16-byte aligned: one access per pixel and frame);
                               * slots[k] is read only for k < n_slots and may be NULL past it */
    int64_t slot_row_stride;  /* pixels, >= width; one stride for every slot frame */
    int32_t n_slots;          /* 1 .. 4 */
    const uint8_t* owner;     /* the owner plane pbr_msaa_fragments wrote */
    int64_t owner_row_stride; /* bytes, >= width */
} pbr_msaa_resolve_source;

/* The multisample resolve into `dst` (out, out_row_stride and format are used, as by pbr_blend_layer), width x height
 * pixels, asynchronously on `stream`. With c_s the pixel of the slot frame that owns sample s, (owner >> 2s) & 3 -- 0 in
 * every channel when that slot is >= n_slots -- per channel, alpha included:
 * RGBA32F: out = ((c_0 + c_1) + (c_2 + c_3)) * 0.25f, each operation rounded once; pairwise, so a pixel whose samples
 * all belong to one fragment gets that fragment's colour bit for bit. RGBA8_UNORM: each sample first holds
 * unorm8(clamp(c_s)), as a UNORM8 multisampled target stores it (the clamp of pbr_blend_layer, NaN -> 0; the
 * FLOAT -> UNORM rule of pbr_output_format); d_s = (float)byte / 255.0f, the same expression, and the rule again.
 * Every pixel of the rectangle is written. Not a shading pass: the pass statistics stay. */
int pbr_msaa_resolve(pbr_context* ctx, const pbr_msaa_resolve_source* source, const pbr_frame_desc* dst, int32_t width,
                     int32_t height, void* stream);

/* ---- Host G-buffer fill (replaces the VS + rasteriser front-end, Default.hlsl:22-45) ---------- */

typedef enum pbr_scene_kind {
    PBR_SCENE_SPHERE_RUSTEDIRON = 1, /* BASELINE config 1: ray-cast unit sphere, rustediron metal/rough */
    PBR_SCENE_RANDOM_COVERED = 2,    /* configs 2, 3, 5: fully covered synthetic G-buffer */
    PBR_SCENE_PLANE_MATERIALS = 4,   /* config 4: plane y = 0 seen top-down, seven *_1K material sets */
    PBR_SCENE_REFERENCE_SPHERES = 5  /* the reference's own scene: 49 red spheres + 9 textured spheres
                                        (PBRApp.cpp:964-973, 1016-1068) under its 4 directional lights */
} pbr_scene_kind;

/* A left-handed look-at camera with world up (0, 1, 0), like Camera (Camera.cpp:104-112). */
typedef struct pbr_camera {
    float eye[3];
    float target[3];
    float fov_y; /* radians */
    float pad0;
} pbr_camera;

/* Host-side texture tiles the scenes sample (owned by the caller). */
typedef struct pbr_scene_assets {
    const uint8_t* rust_metallic;  /* rust_size^2 u8 gray */
    const uint8_t* rust_roughness; /* rust_size^2 u8 gray */
    int32_t rust_size;
    const uint8_t* mat_albedo;     /* [num_materials][mat_size][mat_size][3] */
    const uint8_t* mat_specular;   /* [num_materials][mat_size][mat_size][3] */
    const uint8_t* mat_roughness;  /* [num_materials][mat_size][mat_size]    */
    const uint8_t* mat_metallic;   /* [num_materials][mat_size][mat_size]    */
    const uint8_t* mat_has_metallic; /* [num_materials] */
    const uint8_t* mat_normal;     /* [num_materials][mat_size][mat_size][3] */
    int32_t num_materials;
    int32_t mat_size;
} pbr_scene_assets;

typedef struct pbr_scene_desc {
    int32_t kind;         /* pbr_scene_kind */
    int32_t width;        /* full-frame size: pixel values depend on the global (x, y) only, */
    int32_t height;       /* never on how rows are partitioned across calls or ranks */
    uint64_t seed;
    const pbr_scene_assets* assets;
    const pbr_camera* camera; /* kind 5 only; NULL = the reference's initial camera: eye (0, 0, -5) looking
                                 down +z, fovY pi/4 (BuildCamera, PBRApp.cpp:652-659) */
} pbr_scene_desc;

/* Fills rows [row_begin, row_end) of the full frame into HOST planes laid out like
 * pbr_gbuffer_soa (15 planes in the order pos xyz, normal xyz, albedo rgb, metallic, roughness,
 * ao, f0 rgb; `planes[i]` points at row `row_begin`; `row_stride` elements). Returns the number of
 * covered (non-background) pixels, or a negative pbr_status. */
int64_t pbr_gbuffer_fill(const pbr_scene_desc* scene, int32_t row_begin, int32_t row_end, float* const* planes,
                         int64_t row_stride, int32_t n_threads);

/* pbr_gbuffer_fill that also writes the coverage plane pbr_shade_frame consumes: one byte per pixel,
 * 1 = geometry, 0 = background (config 1's sky around the sphere; the other scenes are fully covered).
 * Background pixels get the view direction in their normal planes (the sky dome point they see). */
int64_t pbr_gbuffer_fill_coverage(const pbr_scene_desc* scene, int32_t row_begin, int32_t row_end,
                                  float* const* planes, int64_t row_stride, uint8_t* coverage,
                                  int64_t coverage_stride, int32_t n_threads);

/* The attribute half of pbr_gbuffer_fill for PBR_SCENE_PLANE_MATERIALS and PBR_SCENE_REFERENCE_SPHERES (other
 * kinds: PBR_ERR_UNSUPPORTED): rows [row_begin, row_end) of the interpolated VertexOut (Default.hlsl:12-20) into 14
 * HOST planes in pbr_attributes_soa order (pos xyz, normal xyz, tangent xyz, bitangent xyz, uv) and the material id
 * plane, both with `row_stride` elements per row. Material ids index the table of scenes.scene_materials (config 4:
 * the cell's *_1K set; the reference scene: the sphere's index, PBR_MATERIAL_NONE for the background, whose normal
 * planes carry the view direction). pbr_resolve_materials of the result is the device counterpart of the fill.
 * Returns the number of covered pixels, or a negative pbr_status. */
int64_t pbr_attributes_fill(const pbr_scene_desc* scene, int32_t row_begin, int32_t row_end, float* const* planes14,
                            uint16_t* material, int64_t row_stride, int32_t n_threads);

/* The light list and pass constants of a benchmark scene (`n_lights` point lights; kind 1 uses one
 * light at (20, 20, -20), strength 100, PBRApp.cpp:490-491; kind 5 uses the reference's four
 * directional lights, PBRApp.cpp:480-487, and needs n_lights == 4). `pass->lights` is set to `lights`. */
int pbr_scene_pass(const pbr_scene_desc* scene, int32_t n_lights, pbr_light* lights, pbr_pass_desc* pass);

const char* pbr_strerror(int status);
/* Last HIP error string recorded by the context (empty if none). */
const char* pbr_last_error(const pbr_context* ctx);
int pbr_abi_version(void);
/* ABI 9: what the library was built from, as JSON: {"abi": 9, "units": [{"unit", "sources_sha", "flavor", "cflags",
 * "switches": {...}}, ...]} -- one record per compilation unit (pbr_context, pbr_frontend, shade_kernels,
 * shade_kernels_bal, frontend_kernels, gbuffer_fill): the stamp of the sources it was compiled from (sha256 of the csrc sources, the Makefile and this header, first
 * 16 hex digits), the build flavor ("product" for the Makefile's default target without EXTRA flags; "debug_bounds",
 * "asan", "custom: ...", "variant: ..." otherwise), its extra compiler flags and every build switch's value. A program
 * that quotes a measurement can check it ran the product build of a given checkout. Static storage. */
const char* pbr_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* PBR_SHADE_H */
