// pbr_frontend.hip -- the front end's half of the C ABI of include/pbr/pbr_shade.h: material and mesh upload, the
// material resolve and the rasteriser. Host code only; the kernels live in frontend_kernels.hip, the context and the
// ordering protocol in pbr_context.hip (pbr_context_impl.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "pbr_context_impl.h"
#include "pbr_debug_bounds.h"
#include "pbr_build_info.h"

extern "C" __attribute__((used, visibility("default"))) const char pbr_unit_info_pbr_frontend[] =
    PBR_UNIT_INFO("pbr_frontend", PBR_BI_SWITCH(PBR_DEBUG_BOUNDS));

static size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// Replace both buffers of `r` (a set that is uploaded as a whole) by copies of the host arrays src0 and src1.
static int replace_pair(Entry& en, Resource& r, const void* src0, size_t bytes0, const void* src1, size_t bytes1,
                        const char* what) {
    return replace_buffers(en, r, true, bytes0, bytes1, what, [&] {
        hipError_t e = hipMemcpyAsync(*r.mem[0], src0, bytes0, hipMemcpyHostToDevice, en.s);
        if (e == hipSuccess) e = hipMemcpyAsync(*r.mem[1], src1, bytes1, hipMemcpyHostToDevice, en.s);
        return e == hipSuccess ? PBR_OK : fail_hip(en.ctx, e, (std::string(what) + " copy").c_str());
    });
}

// ---- Material resolve (Default.hlsl:50-116 on the device; material_resolve.h) ----------------------------------------

extern "C" {

int pbr_set_materials(pbr_context* ctx, const pbr_material* materials, int32_t n_materials,
                      const pbr_texture_desc* textures, int32_t n_textures, void* stream) {
    if (!ctx || n_materials < 0 || n_materials >= (int32_t)PBR_MATERIAL_NONE || n_textures < 0)
        return PBR_ERR_INVALID_ARGUMENT;
    if ((n_materials > 0 && !materials) || (n_textures > 0 && !textures)) return PBR_ERR_INVALID_ARGUMENT;
    // Texture placement in the one RGBA8 buffer; per texture at most 2^26 texels (as the env maps), 2^28 in all.
    std::vector<pbr::MaterialTex> place((size_t)n_textures);
    int64_t total = 0;
    for (int32_t i = 0; i < n_textures; ++i) {
        const pbr_texture_desc& t = textures[i];
        if (!t.texels || t.width <= 0 || t.height <= 0) return PBR_ERR_INVALID_ARGUMENT;
        if (t.channels != 1 && t.channels != 3 && t.channels != 4) return PBR_ERR_INVALID_ARGUMENT;
        const int64_t n = (int64_t)t.width * t.height;
        if (n > (1ll << 26) || total + n > (1ll << 28)) return PBR_ERR_INVALID_ARGUMENT;
        place[(size_t)i] = pbr::MaterialTex{(uint32_t)total, t.width, t.height};
        total += n;
    }
    constexpr uint32_t known = PBR_MAT_DIFFUSE_TEXTURE | PBR_MAT_SPECULAR_TEXTURE | PBR_MAT_METALLIC_TEXTURE |
                               PBR_MAT_ROUGHNESS_TEXTURE | PBR_MAT_NORMAL_TEXTURE | PBR_MAT_ALPHA_TEST;
    // tex[] slot of each flag bit: g_TextureArray 0 diffuse, 1 specular, 2 metallic, 3 roughness, 4 normal, 11 opacity
    static const int slot_of_bit[6] = {0, 1, 2, 3, 4, 5};
    std::vector<pbr::MaterialRec> recs((size_t)(n_materials > 0 ? n_materials : 1));
    std::memset(recs.data(), 0, sizeof(pbr::MaterialRec) * recs.size());
    std::vector<int32_t> slot_tex((size_t)n_materials * 6, -1);
    for (int32_t i = 0; i < n_materials; ++i) {
        const pbr_material& m = materials[i];
        if (m.flags & ~known) return PBR_ERR_INVALID_ARGUMENT;
        pbr::MaterialRec& r = recs[(size_t)i];
        for (int c = 0; c < 3; ++c) r.diffuse[c] = m.diffuse_albedo[c], r.fresnel[c] = m.fresnel_r0[c];
        r.metallic = m.metallic;
        r.roughness = m.roughness;
        r.opacity = m.opacity;
        r.flags = m.flags;
        for (int k = 0; k < 6; ++k) r.tex[k] = pbr::MaterialTex{0u, 1, 1};
        for (int b = 0; b < 6; ++b) {
            if (!(m.flags & (1u << b))) continue;
            const int32_t t = m.tex[slot_of_bit[b]];
            if (t < 0 || t >= n_textures) return PBR_ERR_INVALID_ARGUMENT;
            r.tex[slot_of_bit[b]] = place[(size_t)t];
            slot_tex[(size_t)i * 6 + (size_t)slot_of_bit[b]] = t;
        }
    }
    // Repack to RGBA8: one aligned dword per tap whatever the channel count; a gray texture replicates .r.
    std::vector<uint32_t> texels((size_t)(total > 0 ? total : 1), 0u);
    for (int32_t i = 0; i < n_textures; ++i) {
        const pbr_texture_desc& t = textures[i];
        uint32_t* dst = texels.data() + place[(size_t)i].offset;
        const size_t n = (size_t)t.width * (size_t)t.height;
        for (size_t k = 0; k < n; ++k) {
            const uint8_t* p = t.texels + k * (size_t)t.channels;
            const uint32_t r = p[0], g = t.channels == 1 ? p[0] : p[1], b = t.channels == 1 ? p[0] : p[2],
                           a = t.channels == 4 ? p[3] : 255u;
            dst[k] = r | (g << 8) | (b << 16) | (a << 24);
        }
    }

    Entry en(ctx);
    if (const int rc = en.open(stream, "pbr_set_materials stream")) return rc;
    pbr_context::Materials& mt = ctx->mats;
    mt.set = false;
    ctx->mips.set = false;  // the chains belong to the table they were built from (pbr_generate_mips)
    // The old table and texels may still be read by queued resolves: released after them, in stream order.
    if (const int rc = replace_pair(en, mt.use, recs.data(), sizeof(pbr::MaterialRec) * recs.size(), texels.data(),
                                    sizeof(uint32_t) * texels.size(), "pbr_set_materials"))
        return rc;
    mt.n = n_materials;
    mt.n_texels = (int64_t)texels.size();
    mt.flags.resize((size_t)n_materials);
    for (int32_t i = 0; i < n_materials; ++i) mt.flags[(size_t)i] = materials[i].flags;
    mt.place = std::move(place);
    mt.slot_tex = std::move(slot_tex);
    mt.set = true;
    return PBR_OK;
}

int pbr_generate_mips(pbr_context* ctx, void* stream) {
    if (!ctx) return PBR_ERR_INVALID_ARGUMENT;
    Entry en(ctx);
    const pbr_context::Materials& mt = ctx->mats;
    if (!mt.set) return PBR_ERR_NOT_READY;
    // The level table: levels 1 .. L-1 of every texture, texture after texture, W_l = max(1, W_(l-1) >> 1) and H_l alike
    // down to 1 x 1. The chains hold fewer texels than the upload (at most 2^28), so offsets stay inside 32 bits.
    const size_t nt = mt.place.size();
    std::vector<pbr::MaterialTex> levels;
    std::vector<pbr::MipSlot> chain(nt);
    int64_t total = 0;
    int max_levels = 1;
    for (size_t t = 0; t < nt; ++t) {
        int32_t w = mt.place[t].w, h = mt.place[t].h;
        chain[t].first = (uint32_t)levels.size();
        chain[t].levels = 1;
        while (w > 1 || h > 1) {
            w = std::max(1, w >> 1);
            h = std::max(1, h >> 1);
            levels.push_back(pbr::MaterialTex{(uint32_t)total, w, h});
            total += (int64_t)w * h;
            ++chain[t].levels;
        }
        max_levels = std::max(max_levels, (int)chain[t].levels);
    }
    // The materials' slots, in MaterialRec::tex order without the opacity map.
    const size_t nm = (size_t)mt.n;
    std::vector<pbr::MipSlot> slots(std::max<size_t>(nm * 5, 1), pbr::MipSlot{0u, 1});
    for (size_t i = 0; i < nm; ++i)
        for (size_t k = 0; k < 5; ++k)
            if (const int32_t t = mt.slot_tex[i * 6 + k]; t >= 0) slots[i * 5 + k] = chain[(size_t)t];
    // One launch per level index over the textures that have it: its table, and the texels before each texture.
    std::vector<pbr::MipGen> gen;
    std::vector<size_t> gen_begin((size_t)max_levels + 1, 0);
    std::vector<uint32_t> gen_texels((size_t)max_levels, 0u);
    for (int l = 1; l < max_levels; ++l) {
        gen_begin[(size_t)l] = gen.size();
        uint32_t first = 0;
        for (size_t t = 0; t < nt; ++t) {
            if (chain[t].levels <= l) continue;
            const pbr::MaterialTex& src = l == 1 ? mt.place[t] : levels[chain[t].first + (size_t)l - 2];
            const pbr::MaterialTex& dst = levels[chain[t].first + (size_t)l - 1];
            gen.push_back(pbr::MipGen{src.offset, dst.offset, src.w, src.h, dst.w, dst.h, first, 0u});
            first += (uint32_t)dst.w * (uint32_t)dst.h;
        }
        gen_texels[(size_t)l] = first;
    }
    gen_begin[(size_t)max_levels] = gen.size();
    const size_t off_levels = align_up(sizeof(pbr::MipSlot) * slots.size(), 256);
    const size_t off_gen = off_levels + align_up(sizeof(pbr::MaterialTex) * levels.size(), 256);
    const size_t table_bytes = off_gen + std::max<size_t>(sizeof(pbr::MipGen) * gen.size(), 4);
    const size_t texel_count = (size_t)std::max<int64_t>(total, 1);

    if (const int rc = en.open(stream, "pbr_generate_mips stream")) return rc;
    pbr_context::Mips& mp = ctx->mips;
    mp.set = false;
    // The old chains may still be read by queued resolves: released after them, in stream order. The level launches
    // read the upload's texels under pbr_resolve_materials's rules.
    const int rc = replace_buffers(en, mp.use, true, table_bytes, sizeof(uint32_t) * texel_count, "pbr_generate_mips", [&] {
        char* d = mp.d_tables;
        hipError_t e = hipMemcpyAsync(d, slots.data(), sizeof(pbr::MipSlot) * slots.size(), hipMemcpyHostToDevice, en.s);
        if (e == hipSuccess && !levels.empty())
            e = hipMemcpyAsync(d + off_levels, levels.data(), sizeof(pbr::MaterialTex) * levels.size(),
                               hipMemcpyHostToDevice, en.s);
        if (e == hipSuccess && !gen.empty())
            e = hipMemcpyAsync(d + off_gen, gen.data(), sizeof(pbr::MipGen) * gen.size(), hipMemcpyHostToDevice, en.s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_generate_mips copy");
        e = before_read(ctx->mats.use, en.s, en.si);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_generate_mips order");
        for (int l = 1; l < max_levels; ++l) {
            pbr::MipGenArgs g{};
            g.gen = reinterpret_cast<const pbr::MipGen*>(d + off_gen) + gen_begin[(size_t)l];
            g.n = (int)(gen_begin[(size_t)l + 1] - gen_begin[(size_t)l]);
            g.n_out = gen_texels[(size_t)l];
            g.src = l == 1 ? mt.d_texels : mp.d_texels;
            g.n_src = l == 1 ? mt.n_texels : total;
            g.dst = mp.d_texels;
            g.n_dst = total;
            e = pbr::launch_generate_mip_level(g, en.s);
            if (e != hipSuccess) return fail_hip(ctx, e, "generate_mip_level_kernel launch", PBR_ERR_LAUNCH);
        }
        return after_launch(ctx, en.si, en.s, "pbr_generate_mips record");
    });
    if (rc) return rc;
    mp.d_slots = reinterpret_cast<const pbr::MipSlot*>(mp.d_tables);
    mp.d_levels = reinterpret_cast<const pbr::MaterialTex*>(mp.d_tables + off_levels);
    mp.n_levels = (int64_t)levels.size();
    mp.n_texels = total;
    mp.set = true;
    return PBR_OK;
}

// The argument checks pbr_resolve_materials and pbr_resolve_materials_mip share, and the launch arguments they fill.
static bool resolve_shape_ok(const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg) {
    if (at->width < 0 || at->height < 0 || at->row_stride < at->width || tg->row_stride < at->width) return false;
    return !(tg->coverage && tg->coverage_row_stride < at->width);
}
static int resolve_args(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, pbr::ResolveArgs& a) {
    const float* in[14] = {at->pos_w[0],     at->pos_w[1],     at->pos_w[2],       at->normal_w[0],    at->normal_w[1],
                           at->normal_w[2],  at->tangent_w[0], at->tangent_w[1],   at->tangent_w[2],   at->bitangent_w[0],
                           at->bitangent_w[1], at->bitangent_w[2], at->tex_coord[0], at->tex_coord[1]};
    a.vec = (at->row_stride % 2) == 0 && (tg->row_stride % 2) == 0;
    if (!planes_ok(in, 14, 4, a.vec)) return PBR_ERR_INVALID_ARGUMENT;
    std::copy(in, in + 14, a.attr);
    if (!at->material || !aligned(at->material, 2)) return PBR_ERR_INVALID_ARGUMENT;
    a.material = at->material;
    a.vec = a.vec && aligned(at->material, 4);
    if (!planes_ok(tg->planes, 15, 4, a.vec)) return PBR_ERR_INVALID_ARGUMENT;
    std::copy(tg->planes, tg->planes + 15, a.plane);
    if (tg->opacity && !aligned(tg->opacity, 4)) return PBR_ERR_INVALID_ARGUMENT;
    a.opacity = tg->opacity;
    a.coverage = tg->coverage;
    a.vec = a.vec && aligned(tg->opacity, 8) && aligned(tg->coverage, 2) &&
            (!tg->coverage || (tg->coverage_row_stride % 2) == 0);
    a.width = at->width;
    a.height = at->height;
    a.in_stride = at->row_stride;
    a.out_stride = tg->row_stride;
    a.cov_stride = tg->coverage ? tg->coverage_row_stride : 0;
    a.table = ctx->mats.d_table;
    a.n_materials = ctx->mats.n;
    a.texels = ctx->mats.d_texels;
    a.n_texels = debug_bounds_skew() ? 0 : ctx->mats.n_texels;
    return PBR_OK;
}

int pbr_resolve_materials(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, int32_t filter,
                          void* stream) {
    if (!ctx || !at || !tg || !resolve_shape_ok(at, tg)) return PBR_ERR_INVALID_ARGUMENT;
    if (filter != PBR_FILTER_POINT && filter != PBR_FILTER_LINEAR) return PBR_ERR_INVALID_ARGUMENT;
    Entry en(ctx);
    if (!ctx->mats.set) return PBR_ERR_NOT_READY;
    if (at->width == 0 || at->height == 0) return PBR_OK;  // empty frame: nothing is read or written
    pbr::ResolveArgs a{};
    if (const int rc = resolve_args(ctx, at, tg, a)) return rc;
    a.linear = filter == PBR_FILTER_LINEAR;

    if (const int rc = en.open(stream, "pbr_resolve_materials stream")) return rc;
    hipError_t e = before_read(ctx->mats.use, en.s, en.si);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_resolve_materials order");
    e = pbr::launch_resolve_materials(a, en.s);
    if (e != hipSuccess) return fail_hip(ctx, e, "resolve_materials_kernel launch", PBR_ERR_LAUNCH);
    // Not a shading pass: the stream's statistics record, its kernel name and the context's last pass stay as they
    // are; only the event that orders a later pbr_set_materials after this read is recorded.
    return after_launch(ctx, en.si, en.s, "pbr_resolve_materials record");
}

}  // extern "C"

// pbr_resolve_materials_mip and pbr_resolve_materials_aniso: one validation, one bookkeeping of the two resources read
// (the material table with its texels, the chains); `launch` starts the call's kernel on the filled arguments.
template <class Launch>
static int resolve_mip_call(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, float lod_bias,
                            void* stream, const char* call, const char* kernel, Launch launch) {
    if (!ctx || !at || !tg || !resolve_shape_ok(at, tg) || !std::isfinite(lod_bias)) return PBR_ERR_INVALID_ARGUMENT;
    Entry en(ctx);
    const pbr_context::Mips& mp = ctx->mips;
    if (!ctx->mats.set || !mp.set) return PBR_ERR_NOT_READY;
    if (at->width == 0 || at->height == 0) return PBR_OK;  // empty frame: nothing is read or written
    pbr::ResolveMipArgs a{};
    if (const int rc = resolve_args(ctx, at, tg, a.r)) return rc;
    a.slots = mp.d_slots;
    a.levels = mp.d_levels;
    a.n_levels = mp.n_levels;
    a.mip_texels = mp.d_texels;
    a.n_mip_texels = mp.n_texels;
    a.lod_bias = lod_bias;

    const std::string name(call);
    if (const int rc = en.open(stream, (name + " stream").c_str())) return rc;
    hipError_t e = before_read(ctx->mats.use, en.s, en.si);
    if (e == hipSuccess) e = before_read(ctx->mips.use, en.s, en.si);
    if (e != hipSuccess) return fail_hip(ctx, e, (name + " order").c_str());
    e = launch(a, en.s);
    if (e != hipSuccess) return fail_hip(ctx, e, (std::string(kernel) + " launch").c_str(), PBR_ERR_LAUNCH);
    // Not a shading pass, as pbr_resolve_materials.
    return after_launch(ctx, en.si, en.s, (name + " record").c_str());
}

extern "C" {

int pbr_resolve_materials_mip(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, float lod_bias,
                              void* stream) {
    return resolve_mip_call(ctx, at, tg, lod_bias, stream, "pbr_resolve_materials_mip", "resolve_materials_mip_kernel",
                            [](const pbr::ResolveMipArgs& a, hipStream_t s) { return pbr::launch_resolve_materials_mip(a, s); });
}

int pbr_resolve_materials_aniso(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, float lod_bias,
                                int32_t max_anisotropy, void* stream) {
    if (max_anisotropy < 1 || max_anisotropy > 16) return PBR_ERR_INVALID_ARGUMENT;  // D3D12's MaxAnisotropy range
    return resolve_mip_call(ctx, at, tg, lod_bias, stream, "pbr_resolve_materials_aniso", "resolve_materials_aniso_kernel",
                            [max_anisotropy](const pbr::ResolveMipArgs& a, hipStream_t s) {
                                return pbr::launch_resolve_materials_aniso(pbr::ResolveAnisoArgs{a, max_anisotropy}, s);
                            });
}

}  // extern "C"

// ---- Rasteriser (VS + the fixed-function rasteriser on the device; raster.h) --------------------------

namespace {

constexpr int32_t kRasterMaxSide = 32768;  // frame width and height: keeps every block and pixel count inside 32 bits

// The calling stream's pinned staging with room for `bytes`, free to be written: waits (on the host) for the upload
// that last read it.
hipError_t raster_staging(StreamState::Raster& r, size_t bytes) {
    hipError_t e = hipSuccess;
    if (r.staged_pending) {
        e = hipEventSynchronize(r.staged);
        if (e != hipSuccess) return e;
        r.staged_pending = false;
    }
    if (!r.staged) {
        e = hipEventCreateWithFlags(&r.staged, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    if (bytes > r.h_capacity) {
        if (r.h) (void)hipHostFree(r.h);
        r.h = nullptr;
        r.h_capacity = 0;
        const size_t cap = align_up(bytes + bytes / 2, 4096);
        e = hipHostMalloc(reinterpret_cast<void**>(&r.h), cap, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        r.h_capacity = cap;
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int pbr_set_meshes(pbr_context* ctx, const pbr_mesh_desc* meshes, int32_t n_meshes, void* stream) {
    if (!ctx || n_meshes < 0 || (n_meshes > 0 && !meshes)) return PBR_ERR_INVALID_ARGUMENT;
    std::vector<pbr_context::MeshPlace> place((size_t)n_meshes);
    int64_t nv = 0, ni = 0;
    for (int32_t i = 0; i < n_meshes; ++i) {
        const pbr_mesh_desc& m = meshes[i];
        if (m.n_vertices < 0 || m.n_indices < 0) return PBR_ERR_INVALID_ARGUMENT;
        if ((m.n_vertices > 0 && !m.vertices) || (m.n_indices > 0 && !m.indices)) return PBR_ERR_INVALID_ARGUMENT;
        for (int32_t k = 0; k < m.n_indices; ++k)
            if (m.indices[k] >= (uint32_t)m.n_vertices) return PBR_ERR_INVALID_ARGUMENT;
        place[(size_t)i] = pbr_context::MeshPlace{(uint32_t)nv, (uint32_t)m.n_vertices, (uint32_t)ni, (uint32_t)m.n_indices};
        nv += m.n_vertices;
        ni += m.n_indices;
        if (nv > (1ll << 27) || ni > (1ll << 31)) return PBR_ERR_INVALID_ARGUMENT;  // 7.5 GB of vertices, 8 GB of indices
    }
    std::vector<float> vertices((size_t)(nv > 0 ? nv * 14 : 1), 0.0f);
    std::vector<uint32_t> indices((size_t)(ni > 0 ? ni : 1), 0u);
    for (int32_t i = 0; i < n_meshes; ++i) {
        const pbr_mesh_desc& m = meshes[i];
        if (m.n_vertices > 0)
            std::memcpy(vertices.data() + (size_t)place[(size_t)i].vtx_base * 14, m.vertices,
                        sizeof(float) * 14 * (size_t)m.n_vertices);
        if (m.n_indices > 0)
            std::memcpy(indices.data() + place[(size_t)i].idx_base, m.indices, sizeof(uint32_t) * (size_t)m.n_indices);
    }

    Entry en(ctx);
    if (const int rc = en.open(stream, "pbr_set_meshes stream")) return rc;
    pbr_context::Meshes& ms = ctx->meshes;
    ms.set = false;
    // The old buffers may still be read by queued rasterisations: released after them, in stream order.
    if (const int rc = replace_pair(en, ms.use, vertices.data(), sizeof(float) * vertices.size(), indices.data(),
                                    sizeof(uint32_t) * indices.size(), "pbr_set_meshes"))
        return rc;
    ms.n_vertices = nv;
    ms.n_indices = ni;
    ms.place = std::move(place);
    ms.set = true;
    return PBR_OK;
}

}  // extern "C"

namespace {

// What a multisampled call adds to a rasterisation: the caller's surface and, for pbr_msaa_fragments (slot >= 0), the
// slot and the owner plane. slot < 0: pbr_msaa_rasterize, which has no targets.
struct MsaaCall {
    const pbr_msaa_surface* surface;
    int32_t slot;
    uint8_t* owner;
    int64_t owner_stride;
};

// pbr_rasterize (flags 0), pbr_rasterize_flags, with `layer` pbr_rasterize_layer, and with `msaa` pbr_msaa_rasterize and
// pbr_msaa_fragments. `marks` (development, pbr_debug_rasterize_timed): six events
// recorded around the five stages -- clears and table upload, vertex transform, setup with the small triangles'
// coverage, large triangles, resolve.
int rasterize_impl(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                   const pbr_raster_targets* tg, uint32_t flags, void* stream, hipEvent_t* marks,
                   const pbr_raster_layer* layer = nullptr, const MsaaCall* msaa = nullptr) {
    const bool coverage_only = msaa && msaa->slot < 0;  // pbr_msaa_rasterize: nothing but the surface is written
    if (!ctx || !view || (!tg && !coverage_only) || n_draws < 0 || (n_draws > 0 && !draws))
        return PBR_ERR_INVALID_ARGUMENT;
    if (flags & ~(uint32_t)(PBR_RASTER_CLIP_NEAR | PBR_RASTER_ALPHA_TEST)) return PBR_ERR_INVALID_ARGUMENT;
    if (msaa) {  // no clip piece as a fragment identity and no per-pixel alpha test under multisampling yet
        if (flags != 0u) return PBR_ERR_UNSUPPORTED;
        const pbr_msaa_surface* sf = msaa->surface;
        if (!sf || !sf->visibility || !aligned(sf->visibility, 8) || sf->row_stride < view->width)
            return PBR_ERR_INVALID_ARGUMENT;
        if (!coverage_only && (msaa->slot > 3 || (msaa->owner && msaa->owner_stride < view->width)))
            return PBR_ERR_INVALID_ARGUMENT;
    }
    if (layer) {  // the transparent PSO runs no alpha test; the layer's planes and the depth plane are required
        if (flags & PBR_RASTER_ALPHA_TEST) return PBR_ERR_INVALID_ARGUMENT;
        if (!layer->depth_in || !layer->prim_out || !tg->depth) return PBR_ERR_INVALID_ARGUMENT;
        if (!aligned(layer->depth_in, 4) || !aligned(layer->prim_in, 4) || !aligned(layer->prim_out, 4))
            return PBR_ERR_INVALID_ARGUMENT;
    }
    const bool clip_near = (flags & PBR_RASTER_CLIP_NEAR) != 0;
    if (view->width < 0 || view->height < 0 || view->width > kRasterMaxSide || view->height > kRasterMaxSide)
        return PBR_ERR_INVALID_ARGUMENT;
    if (view->row_begin < 0 || view->row_begin > view->row_end || view->row_end > view->height)
        return PBR_ERR_INVALID_ARGUMENT;
    if (tg && tg->row_stride < view->width) return PBR_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n_draws; ++i) {
        const pbr_draw& d = draws[i];
        if (d.mesh < 0 || d.first_index < 0 || d.index_count < 0 || d.index_count % 3 != 0 || d.cull > 1)
            return PBR_ERR_INVALID_ARGUMENT;
    }
    pbr::RasterArgs a{};
    if (tg) {
        a.vec = (tg->row_stride % 2) == 0;
        if (!planes_ok(tg->planes, 14, 4, a.vec)) return PBR_ERR_INVALID_ARGUMENT;
        std::copy(tg->planes, tg->planes + 14, a.plane);
        if (!tg->material || !aligned(tg->material, 2)) return PBR_ERR_INVALID_ARGUMENT;
        if (tg->depth && !aligned(tg->depth, 4)) return PBR_ERR_INVALID_ARGUMENT;
        a.material = tg->material;
        a.depth = tg->depth;
        a.vec = a.vec && aligned(tg->material, 4) && aligned(tg->depth, 8);
        a.stride = tg->row_stride;
    }
    if (layer) {
        a.peel = true;
        a.depth_in = layer->depth_in;
        a.prim_in = layer->prim_in;
        a.prim_out = layer->prim_out;
        a.vec = a.vec && aligned(layer->prim_out, 8);
    }
    a.width = view->width;
    a.height = view->height;
    a.row_begin = view->row_begin;
    a.row_end = view->row_end;
    std::memcpy(a.view_proj, view->view_proj, sizeof(a.view_proj));
    for (int c = 0; c < 3; ++c)
        a.eye[c] = view->eye[c], a.right[c] = view->bg_right[c], a.up[c] = view->bg_up[c], a.fwd[c] = view->bg_forward[c];

    Entry en(ctx);
    const pbr_context::Meshes& ms = ctx->meshes;
    if (!ms.set) return PBR_ERR_NOT_READY;
    // PBR_RASTER_ALPHA_TEST: the alpha-testing kernels run, and the call reads the material table and the texels,
    // only when some draw's material is tested; the flag alone costs nothing on a scene without cut-outs.
    const pbr_context::Materials& mt = ctx->mats;
    if ((flags & PBR_RASTER_ALPHA_TEST) && !mt.set) return PBR_ERR_NOT_READY;
    bool alpha_test = false;
    if (flags & PBR_RASTER_ALPHA_TEST)
        for (int32_t i = 0; i < n_draws && !alpha_test; ++i)
            alpha_test = draws[i].material < (uint32_t)mt.n && (mt.flags[draws[i].material] & PBR_MAT_ALPHA_TEST) != 0;
    uint64_t n_tris = 0, n_records = 0;
    for (int32_t i = 0; i < n_draws; ++i) {
        const pbr_draw& d = draws[i];
        if ((size_t)d.mesh >= ms.place.size()) return PBR_ERR_INVALID_ARGUMENT;
        const pbr_context::MeshPlace& mp = ms.place[(size_t)d.mesh];
        if ((uint64_t)d.first_index + (uint64_t)d.index_count > (uint64_t)mp.n_indices) return PBR_ERR_INVALID_ARGUMENT;
        n_tris += (uint64_t)d.index_count / 3u;
        n_records += mp.n_vertices;
    }
    if (n_tris > 0xFFFFFFFEull || n_records > 0x7FFFFFFFull) return PBR_ERR_INVALID_ARGUMENT;
    // A clipped triangle lists up to two pieces: the list's length stays inside 32 bits.
    if (clip_near && n_tris > 0x7FFFFFFFull) return PBR_ERR_INVALID_ARGUMENT;
    const int band_h = view->row_end - view->row_begin;
    if (view->width == 0 || band_h == 0) return PBR_OK;  // an empty band: nothing is read or written

    if (const int rc = en.open(stream, "pbr_rasterize stream")) return rc;
    const hipStream_t s = en.s;
    const int si = en.si;
    hipError_t e = hipSuccess;
    StreamState::Raster& rs = ctx->streams[si].raster;

    // The draw table: the records, then the triangle and vertex-record prefixes.
    const size_t nd = (size_t)n_draws;
    const size_t table_bytes = sizeof(pbr::RasterDraw) * nd + sizeof(uint32_t) * 2 * (nd + 1);
    e = raster_staging(rs, table_bytes);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize staging");
    pbr::RasterDraw* h_draws = reinterpret_cast<pbr::RasterDraw*>(rs.h);
    uint32_t* h_tri = reinterpret_cast<uint32_t*>(rs.h + sizeof(pbr::RasterDraw) * nd);
    uint32_t* h_rec = h_tri + (nd + 1);
    uint32_t tri = 0, rec = 0;
    for (size_t i = 0; i < nd; ++i) {
        const pbr_draw& d = draws[i];
        const pbr_context::MeshPlace& mp = ms.place[(size_t)d.mesh];
        pbr::RasterDraw& r = h_draws[i];
        std::memcpy(r.world, d.world, sizeof(r.world));
        std::memcpy(r.tex, d.tex_transform, sizeof(r.tex));
        std::memcpy(r.mat, d.mat_transform, sizeof(r.mat));
        r.vtx_src = mp.vtx_base;
        r.idx_src = mp.idx_base + (uint32_t)d.first_index;
        r.rec_base = rec;
        r.n_vertices = mp.n_vertices;
        r.material = d.material;
        r.cull = d.cull;
        r.pad[0] = r.pad[1] = 0u;
        h_tri[i] = tri;
        h_rec[i] = rec;
        tri += (uint32_t)d.index_count / 3u;
        rec += mp.n_vertices;
    }
    h_tri[nd] = tri;
    h_rec[nd] = rec;

    // Device scratch of this stream: counters | draw table | vertex records | large list | visibility words, and for
    // a near-clipping call | PosH of every record, with a large list of two slots per triangle (16 bytes per record
    // and 8 per triangle more).
    const size_t n_large = (size_t)n_tris * (clip_near ? 2u : 1u);
    const size_t off_table = 256;
    const size_t off_records = off_table + align_up(table_bytes, 256);
    const size_t off_large = off_records + align_up(sizeof(pbr::RasterVertex) * (size_t)n_records, 256);
    const size_t off_vis = off_large + align_up(sizeof(uint2) * n_large, 256);
    // (a multisampled call's visibility words are the caller's surface)
    const size_t vis_bytes = msaa ? 0 : sizeof(unsigned long long) * (size_t)band_h * (size_t)view->width;
    const size_t off_posh = off_vis + align_up(vis_bytes, 256);
    const size_t need = clip_near ? off_posh + sizeof(float4) * (size_t)n_records : off_vis + vis_bytes;
    const bool regrown = need > rs.capacity;
    if (need > rs.capacity) {  // grown in stream order: the stream's earlier rasterisations finish with the old block
        if (rs.d) {
            e = hipFreeAsync(rs.d, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize release");
        }
        rs.d = nullptr;
        rs.capacity = 0;
        e = hipMallocAsync(reinterpret_cast<void**>(&rs.d), need, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize hipMalloc");
        rs.capacity = need;
    }
    rs.d_counters = reinterpret_cast<unsigned long long*>(rs.d);
    a.counters = rs.d_counters;
    a.draws = reinterpret_cast<const pbr::RasterDraw*>(rs.d + off_table);
    a.tri_prefix = reinterpret_cast<const uint32_t*>(rs.d + off_table + sizeof(pbr::RasterDraw) * nd);
    a.rec_prefix = a.tri_prefix + (nd + 1);
    a.records = reinterpret_cast<pbr::RasterVertex*>(rs.d + off_records);
    a.large = reinterpret_cast<uint2*>(rs.d + off_large);
    a.vis = reinterpret_cast<unsigned long long*>(rs.d + off_vis);
    a.clip_near = clip_near;
    a.posh = clip_near ? reinterpret_cast<float4*>(rs.d + off_posh) : nullptr;
    a.n_large = (int64_t)n_large;
    a.n_draws = n_draws;
    a.n_tris = (uint32_t)n_tris;
    a.n_records = (uint32_t)n_records;
    a.vertices = ms.d_vertices;
    a.indices = ms.d_indices;
    a.n_src_vertices = ms.n_vertices;
    a.n_src_indices = debug_bounds_skew() ? 0 : ms.n_indices;
    a.alpha_test = alpha_test;
    if (alpha_test) {
        a.table = mt.d_table;
        a.n_materials = mt.n;
        a.texels = mt.d_texels;
        a.n_texels = debug_bounds_skew() ? 0 : mt.n_texels;
    }

    e = before_read(ctx->meshes.use, s, si);
    // A reader of the material table and the texels like pbr_resolve_materials: a later pbr_set_materials on any stream
    // releases them after this call (after_launch below records the event it waits for).
    if (e == hipSuccess && alpha_test) e = before_read(ctx->mats.use, s, si);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize order");
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    (void)mark(0);
    // pbr_msaa_fragments counts slot_pixels only: the other counters stay those of the stream's last rasterising call
    // (zeros when this call is the stream's first, or found the scratch too small).
    const bool keep_counters = msaa && !coverage_only && rs.ran && !regrown;
    if (keep_counters)
        e = hipMemsetAsync(rs.d_counters + pbr::kRasterSlotPixels, 0, sizeof(unsigned long long) * 4, s);
    else
        e = hipMemsetAsync(rs.d, 0, sizeof(unsigned long long) * pbr::kRasterCounters, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rs.d + off_table, rs.h, table_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(rs.staged, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize upload");
    rs.staged_pending = true;
    if (msaa) {
        pbr::MsaaArgs m{};
        a.vis = nullptr;
        m.r = a;
        m.vis = reinterpret_cast<unsigned long long*>(msaa->surface->visibility);
        m.vis_stride = msaa->surface->row_stride;
        m.slot = msaa->slot;
        m.owner = msaa->owner;
        m.owner_stride = msaa->owner_stride;
        if (coverage_only) {
            e = hipMemsetAsync(m.vis, 0xFF, sizeof(unsigned long long) * 4 * (size_t)band_h * (size_t)m.vis_stride, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "pbr_msaa_rasterize clear");
        }
        e = pbr::launch_raster_vertices(a, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "raster_vertex_kernel launch", PBR_ERR_LAUNCH);
        if (coverage_only) {
            e = pbr::launch_msaa_setup(m, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "raster_setup_msaa_kernel launch", PBR_ERR_LAUNCH);
            e = pbr::launch_msaa_large(m, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "raster_large_msaa_kernel launch", PBR_ERR_LAUNCH);
        } else {
            // slot 0 exists in every pixel: its count is the band's (at most 2^30, the low half of the cleared word)
            e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rs.d_counters + pbr::kRasterSlotPixels),
                                  band_h * view->width, 1, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "pbr_msaa_fragments count");
            e = pbr::launch_msaa_fragments(m, s);
            if (e != hipSuccess) return fail_hip(ctx, e, "raster_fragments_msaa_kernel launch", PBR_ERR_LAUNCH);
        }
        if (!keep_counters) rs.triangles = (int64_t)n_tris;
        rs.ran = true;
        return after_launch(ctx, si, s, "pbr_msaa record");
    }
    e = hipMemsetAsync(a.vis, 0xFF, vis_bytes, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize clear");
    (void)mark(1);
    e = pbr::launch_raster_vertices(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "raster_vertex_kernel launch", PBR_ERR_LAUNCH);
    (void)mark(2);
    e = pbr::launch_raster_setup(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "raster_setup_kernel launch", PBR_ERR_LAUNCH);
    (void)mark(3);
    e = pbr::launch_raster_large(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "raster_large_kernel launch", PBR_ERR_LAUNCH);
    (void)mark(4);
    e = pbr::launch_raster_resolve(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "raster_resolve_kernel launch", PBR_ERR_LAUNCH);
    (void)mark(5);
    rs.triangles = (int64_t)n_tris;
    rs.ran = true;
    // Not a shading pass: the stream's statistics record and kernel name stay; only the event that orders a later
    // pbr_set_meshes after this read is recorded.
    return after_launch(ctx, si, s, "pbr_rasterize record");
}

}  // namespace

extern "C" {

int pbr_rasterize(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                  const pbr_raster_targets* targets, void* stream) {
    return rasterize_impl(ctx, draws, n_draws, view, targets, 0u, stream, nullptr);
}

int pbr_rasterize_flags(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                        const pbr_raster_targets* targets, uint32_t flags, void* stream) {
    return rasterize_impl(ctx, draws, n_draws, view, targets, flags, stream, nullptr);
}

int pbr_rasterize_layer(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                        const pbr_raster_targets* targets, uint32_t flags, const pbr_raster_layer* layer, void* stream) {
    if (!layer) return PBR_ERR_INVALID_ARGUMENT;
    return rasterize_impl(ctx, draws, n_draws, view, targets, flags, stream, nullptr, layer);
}

}  // extern "C"

// The counters of the last rasterisation on `stream` into h (synchronises it) and its triangle count; *ran false (and
// nothing read) when the context has not rasterised on that stream.
static int read_raster_counters(pbr_context* ctx, void* stream, unsigned long long h[pbr::kRasterCounters],
                                int64_t* triangles, bool* ran, const char* what) {
    *ran = false;
    Entry en(ctx);
    if (const int rc = en.device(stream)) return rc;
    const StreamState* st = nullptr;
    for (const StreamState& c : ctx->streams)
        if (c.stream == en.s && c.raster.ran) st = &c;
    if (!st) return PBR_OK;
    hipError_t e = hipMemcpyAsync(h, st->raster.d_counters, sizeof(unsigned long long) * pbr::kRasterCounters,
                                  hipMemcpyDeviceToHost, en.s);
    if (e == hipSuccess) e = hipStreamSynchronize(en.s);
    if (e != hipSuccess) return fail_hip(ctx, e, what);
    *triangles = st->raster.triangles;
    *ran = true;
    return PBR_OK;
}

extern "C" {

int pbr_last_raster_stats(pbr_context* ctx, pbr_raster_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_raster_stats{};
    unsigned long long h[pbr::kRasterCounters] = {};
    int64_t triangles = 0;
    bool ran = false;
    if (const int rc = read_raster_counters(ctx, stream, h, &triangles, &ran, "pbr_last_raster_stats")) return rc;
    if (!ran) return PBR_OK;
    out->triangles = triangles;
    out->backface_culled = (int64_t)h[pbr::kRasterCulled];
    out->zero_area = (int64_t)h[pbr::kRasterZeroArea];
    out->skipped_near = (int64_t)h[pbr::kRasterNear];
    out->skipped_guard_band = (int64_t)h[pbr::kRasterGuard];
    out->fragments = (int64_t)h[pbr::kRasterFragments];
    return PBR_OK;
}

int pbr_last_raster_clip_stats(pbr_context* ctx, pbr_raster_clip_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_raster_clip_stats{};
    unsigned long long h[pbr::kRasterCounters] = {};  // every call clears them: zeros after an unflagged one
    int64_t triangles = 0;
    bool ran = false;
    if (const int rc = read_raster_counters(ctx, stream, h, &triangles, &ran, "pbr_last_raster_clip_stats")) return rc;
    out->clipped_near = (int64_t)h[pbr::kRasterClipped];
    out->clip_pieces = (int64_t)h[pbr::kRasterClipPieces];
    return PBR_OK;
}

int pbr_last_raster_alpha_stats(pbr_context* ctx, pbr_raster_alpha_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_raster_alpha_stats{};
    unsigned long long h[pbr::kRasterCounters] = {};  // every call clears them: zeros unless fragments were tested
    int64_t triangles = 0;
    bool ran = false;
    if (const int rc = read_raster_counters(ctx, stream, h, &triangles, &ran, "pbr_last_raster_alpha_stats")) return rc;
    out->alpha_tested = (int64_t)h[pbr::kRasterAlphaTested];
    out->alpha_discarded = (int64_t)h[pbr::kRasterAlphaDiscarded];
    return PBR_OK;
}

int pbr_last_raster_layer_stats(pbr_context* ctx, pbr_raster_layer_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_raster_layer_stats{};
    unsigned long long h[pbr::kRasterCounters] = {};  // every call clears them: zeros unless the call was a layer's
    int64_t triangles = 0;
    bool ran = false;
    if (const int rc = read_raster_counters(ctx, stream, h, &triangles, &ran, "pbr_last_raster_layer_stats")) return rc;
    out->layer_fragments = (int64_t)h[pbr::kRasterLayerFragments];
    return PBR_OK;
}

int pbr_msaa_rasterize(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                       uint32_t flags, const pbr_msaa_surface* surface, void* stream) {
    const MsaaCall call{surface, -1, nullptr, 0};
    return rasterize_impl(ctx, draws, n_draws, view, nullptr, flags, stream, nullptr, nullptr, &call);
}

int pbr_msaa_fragments(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                       uint32_t flags, const pbr_msaa_surface* surface, int32_t slot, const pbr_raster_targets* targets,
                       uint8_t* owner, int64_t owner_row_stride, void* stream) {
    if (slot < 0 || slot > 3) return PBR_ERR_INVALID_ARGUMENT;
    const MsaaCall call{surface, slot, owner, owner_row_stride};
    return rasterize_impl(ctx, draws, n_draws, view, targets, flags, stream, nullptr, nullptr, &call);
}

int pbr_last_msaa_stats(pbr_context* ctx, pbr_msaa_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_msaa_stats{};
    unsigned long long h[pbr::kRasterCounters] = {};  // every other call clears them: zeros unless it was a fragments call
    int64_t triangles = 0;
    bool ran = false;
    if (const int rc = read_raster_counters(ctx, stream, h, &triangles, &ran, "pbr_last_msaa_stats")) return rc;
    for (int k = 0; k < 4; ++k) out->slot_pixels[k] = (int64_t)h[pbr::kRasterSlotPixels + k];
    return PBR_OK;
}

// The multisample resolve of the shaded slots of a frame (msaa_resolve.h).
int pbr_msaa_resolve(pbr_context* ctx, const pbr_msaa_resolve_source* src, const pbr_frame_desc* dst, int32_t width,
                     int32_t height, void* stream) {
    if (!ctx || !src || !dst || width < 0 || height < 0) return PBR_ERR_INVALID_ARGUMENT;
    if (dst->format != PBR_OUTPUT_RGBA32F && dst->format != PBR_OUTPUT_RGBA8_UNORM) return PBR_ERR_INVALID_ARGUMENT;
    if (src->n_slots < 1 || src->n_slots > 4 || !src->owner || !dst->out || !aligned(dst->out, 4))
        return PBR_ERR_INVALID_ARGUMENT;
    if (src->slot_row_stride < width || src->owner_row_stride < width || dst->out_row_stride < width)
        return PBR_ERR_INVALID_ARGUMENT;
    pbr::MsaaResolveArgs a{};
    a.format = dst->format == PBR_OUTPUT_RGBA8_UNORM ? pbr::kBlendRgba8 : pbr::kBlendRgba32f;
    a.vec = a.format == pbr::kBlendRgba8 || aligned(dst->out, 16);
    for (int k = 0; k < src->n_slots; ++k) {
        if (!src->slots[k] || !aligned(src->slots[k], 4)) return PBR_ERR_INVALID_ARGUMENT;
        a.slots[k] = src->slots[k];
        a.vec = a.vec && aligned(src->slots[k], 16);
    }
    Entry en(ctx);
    if (width == 0 || height == 0) return PBR_OK;  // an empty frame: nothing is read or written
    a.slot_stride = src->slot_row_stride;
    a.n_slots = src->n_slots;
    a.owner = src->owner;
    a.owner_stride = src->owner_row_stride;
    a.out = dst->out;
    a.out_stride = dst->out_row_stride;
    a.width = width;
    a.height = height;
    // Not a shading pass and a reader of no context resource, as pbr_blend_layer.
    if (const int rc = en.device(stream)) return rc;
    const hipError_t e = pbr::launch_msaa_resolve(a, en.s);
    return e == hipSuccess ? PBR_OK : fail_hip(ctx, e, "msaa_resolve_kernel launch", PBR_ERR_LAUNCH);
}

// The transparent PSO's output-merger blend of a shaded layer over the frame (blend_layer.h).
int pbr_blend_layer(pbr_context* ctx, const pbr_blend_source* src, const pbr_frame_desc* dst, int32_t width,
                    int32_t height, void* stream) {
    if (!ctx || !src || !dst || width < 0 || height < 0) return PBR_ERR_INVALID_ARGUMENT;
    if (dst->format != PBR_OUTPUT_RGBA32F && dst->format != PBR_OUTPUT_RGBA8_UNORM) return PBR_ERR_INVALID_ARGUMENT;
    if (!src->src || !src->alpha || !src->coverage || !dst->out) return PBR_ERR_INVALID_ARGUMENT;
    if (!aligned(src->src, 4) || !aligned(src->alpha, 4) || !aligned(dst->out, 4)) return PBR_ERR_INVALID_ARGUMENT;
    if (src->src_row_stride < width || src->alpha_row_stride < width || src->coverage_row_stride < width ||
        dst->out_row_stride < width)
        return PBR_ERR_INVALID_ARGUMENT;
    Entry en(ctx);
    if (width == 0 || height == 0) return PBR_OK;  // an empty frame: nothing is read or written
    pbr::BlendArgs a{};
    a.src = src->src;
    a.alpha = src->alpha;
    a.coverage = src->coverage;
    a.out = dst->out;
    a.src_stride = src->src_row_stride;
    a.alpha_stride = src->alpha_row_stride;
    a.cov_stride = src->coverage_row_stride;
    a.out_stride = dst->out_row_stride;
    a.width = width;
    a.height = height;
    a.format = dst->format == PBR_OUTPUT_RGBA8_UNORM ? pbr::kBlendRgba8 : pbr::kBlendRgba32f;
    a.vec = aligned(src->src, 16) && (a.format == pbr::kBlendRgba8 || aligned(dst->out, 16));
    // Not a shading pass and a reader of no context resource: the stream's statistics record, its kernel name and the
    // ordering events stay as they are.
    if (const int rc = en.device(stream)) return rc;
    const hipError_t e = pbr::launch_blend_layer(a, en.s);
    return e == hipSuccess ? PBR_OK : fail_hip(ctx, e, "blend_layer_kernel launch", PBR_ERR_LAUNCH);
}

}  // extern "C"

// Development (tools/raster_bench.py; not in the public header): one pbr_rasterize_flags with HIP events between its
// stages; synchronises `stream` and writes the milliseconds of the clears and table upload, the vertex transform, the
// setup with the small triangles' coverage, the large triangles' coverage and the per-pixel resolve into ms5.
extern "C" int pbr_debug_rasterize_flags_timed(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws,
                                               const pbr_raster_view* view, const pbr_raster_targets* targets,
                                               uint32_t flags, void* stream, float* ms5) {
    if (!ctx || !ms5) return PBR_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipEvent_t ev[6] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    int rc = e == hipSuccess ? rasterize_impl(ctx, draws, n_draws, view, targets, flags, stream, ev) : PBR_ERR_HIP;
    if (rc == PBR_OK && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = PBR_ERR_HIP;
    for (int i = 0; i < 5; ++i) {
        ms5[i] = 0.0f;
        if (rc == PBR_OK && hipEventElapsedTime(&ms5[i], ev[i], ev[i + 1]) != hipSuccess) rc = PBR_ERR_HIP;
    }
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    return rc;
}

// The same for pbr_rasterize_layer.
extern "C" int pbr_debug_rasterize_layer_timed(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws,
                                               const pbr_raster_view* view, const pbr_raster_targets* targets,
                                               uint32_t flags, const pbr_raster_layer* layer, void* stream,
                                               float* ms5) {
    if (!ctx || !ms5 || !layer) return PBR_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipEvent_t ev[6] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    int rc = e == hipSuccess ? rasterize_impl(ctx, draws, n_draws, view, targets, flags, stream, ev, layer) : PBR_ERR_HIP;
    if (rc == PBR_OK && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = PBR_ERR_HIP;
    for (int i = 0; i < 5; ++i) {
        ms5[i] = 0.0f;
        if (rc == PBR_OK && hipEventElapsedTime(&ms5[i], ev[i], ev[i + 1]) != hipSuccess) rc = PBR_ERR_HIP;
    }
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    return rc;
}

// The same for pbr_rasterize.
extern "C" int pbr_debug_rasterize_timed(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws,
                                         const pbr_raster_view* view, const pbr_raster_targets* targets, void* stream,
                                         float* ms5) {
    return pbr_debug_rasterize_flags_timed(ctx, draws, n_draws, view, targets, 0u, stream, ms5);
}
