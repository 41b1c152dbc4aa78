// raster.h -- VS (Default.hlsl:22-45) and the rasteriser behind DrawIndexedInstanced (PBRApp.cpp:1133) on the device:
// indexed triangle lists in, the 14 planes of a pbr_attributes_soa, the material plane and the depth plane out
// (pbr_rasterize and its flagged, layer and multisampled forms, include/pbr/pbr_shade.h; DESIGN.md §12 fixes every
// operation). A source of frontend_kernels.hip, which is compiled with the canonical fp32 flags: no contraction,
// correctly rounded / and sqrt.
//
// Stages: four launches, stream-ordered, none waiting on another workgroup.
//   1. Vertex (raster_vertex_kernel): one lane per (draw, vertex): VS, the perspective division, the viewport and the
//      snap to 1/256 pixel into a RasterVertex record.
//   2. Setup (raster_setup_kernel; raster_setup_clip_kernel; raster_setup_msaa_kernel): one lane per triangle:
//      tri_setup (the skip tests; tri_area: the signed area in int64 and culling), tri_box clipped to the band. A
//      triangle whose box holds at most kSmallPixels pixels is rasterised by its lane; the others go to the large
//      list through one atomic per wave (append_large).
//   3. Large (raster_large_kernel; raster_large_msaa_kernel): a workgroup per listed triangle (grid-stride over the
//      list) and kLargeSlabs workgroups across its 64 x 4 pixel blocks; a block every point of which some edge
//      function rejects (its maximum over the block's corners is negative) is skipped. So one triangle over the
//      whole frame is spread over kLargeSlabs workgroups, and 10^5 sub-pixel triangles never reach this kernel.
//   4. Resolve (raster_resolve_kernel; raster_fragments_msaa_kernel): per pixel, on the material resolve's 64 x 8 tile,
//      a pixel pair per lane: the visibility word names the winning triangle; its records are fetched again, the edge
//      functions and barycentrics recomputed with the operations of the coverage test, the attributes interpolated
//      (perspective_weights, interpolate) and stored.
// Stages 2 and 3 meet in raster_point<Mode> (steps 5-7 for a pixel centre: edge_at_centre, covered, barycentrics,
// interpolate_z, the depth range, the mode's test, the key), which returns one result word (kFragment, kFragTested,
// kFragDiscarded, kFragUpdate) that one Counts sums; the setup lanes reach it through raster_small<Mode>. Visibility is
// one 64-bit word per band pixel, cleared to all ones and lowered by a global 64-bit atomicMin: the smallest key wins
// whatever the execution order.
//
// Variants: each is a template parameter of the kernels it reaches, selected with `if constexpr`, and the launch
// functions turn the call's runtime flags into them (with_bool, with_mode). An unflagged pbr_rasterize launches the
// all-false instantiations, which carry nothing of the others. The setup and large kernels' (ALPHA, PEEL) is the
// Mode of their points (mode_of): Plain, Alpha or Peel.
//   CLIP   (PBR_RASTER_CLIP_NEAR; step 2a; vertex, setup, large, resolve) the vertex stage also stores PosH (16 bytes
//          per record) and marks the vertices with PosH.z not >= 0 as outside. A triangle with 1 or 2 inside vertices
//          becomes 1 or 2 pieces whose new vertices -- the crossings of its edges with z = 0, each computed from the
//          inside vertex to the outside one and taken through project() -- are never stored: setup, large and the
//          resolve rebuild a piece from the triangle's ordinal and the piece's number with the same operations
//          (piece_setup), so the resolve reproduces the key's z bits as it does for an unclipped triangle. A large-list
//          entry carries the piece's number in the top bit of its block count (a block count is below 2^23: frames
//          are at most 32,768 on a side).
//   ALPHA  (PBR_RASTER_ALPHA_TEST and some draw with a PBR_MAT_ALPHA_TEST material; step 6a; Default.hlsl:111-113;
//          setup, large; Mode::Alpha) a fragment of a tested draw interpolates its TexCoord with the resolve's
//          operations, fetches the material resolve's point-wrap tap of the opacity texture and, with
//          opacity - 0.1 < 0, issues no visibility update. The winner is still the key's triangle.
//   PEEL   (pbr_rasterize_layer; step 7a; RenderLayer::Transparent, PBRApp.cpp:313-316: depth LESS with writes on,
//          blending; setup, large, resolve; Mode::Peel; never with ALPHA) a fragment is eligible iff its
//          ordinal is at least the pixel's floor and its z is below the incoming depth; the key is
//          (ordinal << 32) | bits(z) instead of (bits(z) << 32) | ordinal, so the earliest eligible fragment in
//          submission order wins -- the next one the D3D depth test would accept. The resolve writes that fragment's
//          attributes, its z as the new depth and its ordinal + 1 as the next floor; a pixel without one keeps the
//          incoming depth and gets the floor 0xFFFFFFFF.
//   VEC    (resolve, fragments) every plane is 8-byte aligned with an even stride: a lane stores its pair at once.
//   Four samples per pixel (pbr_msaa_rasterize, pbr_msaa_fragments; step 7b; the three *_msaa kernels, whose MsaaArgs
//          hold the caller's surface; raster_pixel_samples) steps 5-7 at the four sample points of a pixel into one
//          word per (sample, pixel), sample-major; boxes and the block rejection reach kSampleReach further. The
//          fragments stage takes the resolve's place: the samples of a pixel with the same triangle are one fragment,
//          numbered as slots by their lowest sample; a slot's attributes are step 8 at the pixel centre, covered
//          or not.
//
// What is still written more than once, and why: a helper that a kernel calls is simplified on its own before it is
// inlined, and the schedule of the kernel follows. Every sharing below was compiled and compared with
// tools/isa_compare.py (profiles/raster_once/); it stays apart where it changed a kernel, because the kernels of an
// unflagged pbr_rasterize must stay instruction for instruction what every earlier measurement timed, and the changed
// kernels of the other calls have not been timed on a device.
//   - steps 2-3 in raster_vertex_kernel and project() (vertex_calls_project.txt: 304 -> 323 instructions);
//   - step 4's end in piece_setup and tri_area (piece_setup_calls_tri_area.txt: the ten CLIP kernels change);
//   - steps 5-7 in raster_pixel_samples and raster_point (samples_in_point_routine.txt: both *_msaa coverage kernels
//     change); the unflagged setup kernel's small-box loop (small_loop_as_function.txt);
//   - the setup and large flows and the tile's pair store of the *_msaa kernels (kernel_body_as_function.txt,
//     pair_store_as_function.txt: a kernel body moved into a function, verbatim, changes all of them);
//   - l_i rw_i before perspective_weights (weights_with_products.txt: the helper that also forms the products changes
//     the resolve kernels by 0 or 1 instruction).
#pragma once

#include <type_traits>

#include "pbr_device_math.h"
#include "frontend_kernels.h"
#include "material_resolve.h"

namespace pbr {

namespace raster {

constexpr int kSmallPixels = 64;   // clipped bounding boxes up to this many pixels: rasterised by the setup lane
constexpr int kLargeSlabs = 32;    // workgroups across one large triangle's blocks
constexpr int kLargeGridX = 1024;  // workgroups (x) striding over the large list
constexpr int kBlockW = 64, kBlockH = 4;
constexpr int kSamples = 4;
constexpr int kSampleReach = 96;  // no sample is further from its pixel's centre, in subpixels, along either axis

// What a point's fragment has to pass and which key it writes (the header comment); the 1x kernels' (ALPHA, PEEL).
enum class Mode { Plain, Alpha, Peel };
constexpr Mode mode_of(bool alpha, bool peel) { return alpha ? Mode::Alpha : (peel ? Mode::Peel : Mode::Plain); }

// mul(v, M)[j] for a row vector: the 4-wide dot ((x + y) + z) + w, M row-major.
__device__ __forceinline__ float mul4(float x, float y, float z, float w, const float* m, int j) {
    return ((x * m[j] + y * m[4 + j]) + z * m[8 + j]) + w * m[12 + j];
}
// mul(v, (float3x3)M)[j].
__device__ __forceinline__ float mul3(float x, float y, float z, const float* m, int j) {
    return (x * m[j] + y * m[4 + j]) + z * m[8 + j];
}

// The draw that holds element g of a prefix-summed range: the largest d with prefix[d] <= g (g < prefix[n]).
__device__ __forceinline__ int find_draw(const uint32_t* prefix, int n, uint32_t g) {
    int lo = 0, hi = n;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (prefix[PBR_BOUNDS((int64_t)mid, (int64_t)n + 1, kBoundsRaster)] <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Steps 2-3 on a piece's new vertex (piece_setup): the near test on w, the three divisions, the viewport, the snap to
// 1/256 pixel and the guard band, operation for operation what raster_vertex_kernel does to a submitted vertex (which
// keeps them written out: profiles/raster_once/vertex_calls_project.txt).
struct Projected {
    int X, Y;
    float z, rw;
    uint32_t flags;  // kVertexNear | kVertexGuard
};
__device__ __forceinline__ Projected project(const RasterArgs& a, float x, float y, float z, float w) {
    Projected o;
    uint32_t flags = w > 0.0f ? 0u : kVertexNear;  // NaN: near
    const float nx = x / w, ny = y / w, nz = z / w;
    const float xs = (nx * 0.5f + 0.5f) * (float)a.width, ys = (0.5f - ny * 0.5f) * (float)a.height;
    const float tx = xs * 256.0f, ty = ys * 256.0f;
    const bool inside = fabsf(tx) < 0x1p23f && fabsf(ty) < 0x1p23f;  // false for NaN and inf
    if (!inside) flags |= kVertexGuard;
    o.X = inside ? (int)rintf(tx) : 0;
    o.Y = inside ? (int)rintf(ty) : 0;
    o.z = nz;
    o.rw = 1.0f / w;
    o.flags = flags;
    return o;
}

// kTriClipped (CLIP only): 1 or 2 vertices are outside: the triangle is drawn as its pieces. kTriNone: no triangle.
enum TriStatus { kTriDraw = 0, kTriNear, kTriGuard, kTriZeroArea, kTriCulled, kTriClipped, kTriNone };

// A triangle after setup: its vertices' records and snapped positions in the order every
// later step uses (1 and 2 exchanged for a back face drawn under cull none), the positive area, the draw.
struct Tri {
    uint32_t rec[3];
    int X[3], Y[3];
    long long A;
    int draw;
};

// Step 4's end on the snapped positions of s: the signed area in int64, the zero-area and cull tests and, for a back
// face drawn under cull none, the exchange of vertices 1 and 2 in s.
__device__ __forceinline__ TriStatus tri_area(const RasterDraw& dr, Tri& s) {
    long long A = (long long)(s.X[1] - s.X[0]) * (long long)(s.Y[2] - s.Y[0]) -
                  (long long)(s.X[2] - s.X[0]) * (long long)(s.Y[1] - s.Y[0]);
    if (A == 0) return kTriZeroArea;
    if (A < 0) {
        if (dr.cull == 0u) return kTriCulled;
        const uint32_t r1 = s.rec[1];
        s.rec[1] = s.rec[2];
        s.rec[2] = r1;
        const int x1 = s.X[1], y1 = s.Y[1];
        s.X[1] = s.X[2], s.Y[1] = s.Y[2];
        s.X[2] = x1, s.Y[2] = y1;
        A = -A;
    }
    s.A = A;
    return kTriDraw;
}

// CLIP: `outside` receives the mask of the vertices (in index order) marked kVertexOutside; with none of them the
// triangle is set up as without CLIP, with all three it is kTriNear (step 2a: n = 0), otherwise kTriClipped with
// s.rec in index order and s.draw set (piece_setup goes on from there).
template <bool CLIP = false>
__device__ __forceinline__ TriStatus tri_setup(const RasterArgs& a, uint32_t t, Tri& s, uint32_t* outside = nullptr) {
    const int d = find_draw(a.tri_prefix, a.n_draws, t);
    s.draw = d;
    const RasterDraw& dr = a.draws[PBR_BOUNDS((int64_t)d, (int64_t)a.n_draws, kBoundsRaster)];
    const uint32_t k = t - a.tri_prefix[PBR_BOUNDS((int64_t)d, (int64_t)a.n_draws + 1, kBoundsRaster)];
    const int64_t i0 = (int64_t)dr.idx_src + 3 * (int64_t)k;
    uint32_t flags = 0;
    [[maybe_unused]] uint32_t mask = 0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint32_t idx = a.indices[PBR_BOUNDS(i0 + v, a.n_src_indices, kBoundsMesh)];
        s.rec[v] = dr.rec_base + idx;
        const RasterVertex& r = a.records[PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster)];
        s.X[v] = r.X;
        s.Y[v] = r.Y;
        flags |= r.flags;
        if constexpr (CLIP) mask |= ((r.flags / kVertexOutside) & 1u) << v;
    }
    if constexpr (CLIP) {
        *outside = mask;
        if (mask == 7u) return kTriNear;
        if (mask != 0u) return kTriClipped;
    }
    if (flags & kVertexNear) return kTriNear;
    if (flags & kVertexGuard) return kTriGuard;
    return tri_area(dr, s);
}

// The pixels that have a point within `reach` subpixels of their centre, along both axes, inside the triangle's
// bounding box, clipped to the band; false when there are none. Reach 0: the pixels whose centres can lie inside the triangle.
// Reach kSampleReach: those with a sample that can; conservative: every point that near counts, sample or not.
struct Box {
    int x0, x1, y0, y1;  // inclusive
};
__device__ __forceinline__ bool tri_box(const RasterArgs& a, const Tri& s, int reach, Box& b) {
    const int minx = min(s.X[0], min(s.X[1], s.X[2])), maxx = max(s.X[0], max(s.X[1], s.X[2]));
    const int miny = min(s.Y[0], min(s.Y[1], s.Y[2])), maxy = max(s.Y[0], max(s.Y[1], s.Y[2]));
    // 256 p + 128 + reach >= min and 256 p + 128 - reach <= max
    //   <=>  p in [ceil((min - 128 - reach) / 256), floor((max - 128 + reach) / 256)]
    b.x0 = max((minx - (128 + reach) + 255) >> 8, 0);
    b.x1 = min((maxx - (128 - reach)) >> 8, a.width - 1);
    b.y0 = max((miny - (128 + reach) + 255) >> 8, a.row_begin);
    b.y1 = min((maxy - (128 - reach)) >> 8, a.row_end - 1);
    return b.x0 <= b.x1 && b.y0 <= b.y1;
}

// Edge e of the triangle runs from vertex (e + 1) % 3 to vertex (e + 2) % 3: E0 = 1->2, E1 = 2->0, E2 = 0->1.
struct Edges {
    int dx[3], dy[3], xa[3], ya[3];
    bool top_left[3];
};
__device__ __forceinline__ void tri_edges(const Tri& s, Edges& e) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int va = (k + 1) % 3, vb = (k + 2) % 3;
        e.dx[k] = s.X[vb] - s.X[va];
        e.dy[k] = s.Y[vb] - s.Y[va];
        e.xa[k] = s.X[va];
        e.ya[k] = s.Y[va];
        e.top_left[k] = e.dy[k] < 0 || (e.dy[k] == 0 && e.dx[k] > 0);
    }
}
// E = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa) at the point (px, py) of the subpixel grid, exact in int64; and at the
// centre of pixel (x, y), which is (256 x + 128, 256 y + 128).
__device__ __forceinline__ long long edge_at(const Edges& e, int k, int px, int py) {
    return (long long)e.dx[k] * (long long)(py - e.ya[k]) - (long long)e.dy[k] * (long long)(px - e.xa[k]);
}
__device__ __forceinline__ long long edge_at_centre(const Edges& e, int k, int x, int y) {
    return edge_at(e, k, 256 * x + 128, 256 * y + 128);
}
__device__ __forceinline__ bool covered(const Edges& e, const long long E[3]) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) in = in && (E[k] > 0 || (E[k] == 0 && e.top_left[k]));
    return in;
}
// l_i = (float)E_i / (float)A: the conversions round to nearest.
__device__ __forceinline__ void barycentrics(const long long E[3], long long A, float l[3]) {
    const float fa = (float)A;
#pragma unroll
    for (int k = 0; k < 3; ++k) l[k] = (float)E[k] / fa;
}
__device__ __forceinline__ float interpolate_z(const float l[3], const float z[3]) {
    return ((l[0] * z[0] + l[1] * z[1]) + l[2] * z[2]) + 0.0f;
}

// Step 8's weights from p_i = l_i rw_i: q_i = p_i / ((p0 + p1) + p2); and a value interpolated with them.
__device__ __forceinline__ void perspective_weights(const float p[3], float q[3]) {
    const float sum = (p[0] + p[1]) + p[2];
#pragma unroll
    for (int v = 0; v < 3; ++v) q[v] = p[v] / sum;
}
__device__ __forceinline__ float interpolate(const float q[3], float a0, float a1, float a2) {
    return (q[0] * a0 + q[1] * a1) + q[2] * a2;
}

__device__ __forceinline__ void load_z(const RasterArgs& a, const Tri& s, float z[3]) {
#pragma unroll
    for (int v = 0; v < 3; ++v) z[v] = a.records[PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster)].z;
}

// ---- Alpha test (step 6a; Mode::Alpha) ----
// What the test needs of a triangle (or piece): whether its draw is tested, the opacity texture of the draw's material
// record, and 1 / w and TexCoord of the three vertices in setup's order. Filled only for a tested draw.
struct AlphaTri {
    bool tested;
    MaterialTex tex;
    float rw[3], u[3], v[3];
};

// The draw's material: tested iff its id is inside the table and the record has PBR_MAT_ALPHA_TEST. UNIFORM: the draw
// is the same over the wave, so the record is read through a wave-uniform index (scalar loads, a uniform branch).
template <bool UNIFORM>
__device__ __forceinline__ void alpha_material(const RasterArgs& a, int draw, AlphaTri& al) {
    uint32_t id = a.draws[PBR_BOUNDS((int64_t)draw, (int64_t)a.n_draws, kBoundsRaster)].material;
    if constexpr (UNIFORM) id = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
    al.tested = false;
    if (id < (uint32_t)a.n_materials) {
        const MaterialRec& m = a.table[PBR_BOUNDS((int64_t)id, (int64_t)a.n_materials, kBoundsTexel)];
        if (m.flags & kMatAlphaTest) {
            al.tested = true;
            al.tex = m.tex[5];
        }
    }
}

// rw and TexCoord of a submitted triangle's vertices: their records'.
__device__ __forceinline__ void alpha_vertices(const RasterArgs& a, const Tri& s, AlphaTri& al) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const RasterVertex& r = a.records[PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster)];
        al.rw[v] = r.rw;
        al.u[v] = r.a[12];
        al.v[v] = r.a[13];
    }
}

// The test of one fragment: TexCoord with the operations of step 8 (the resolve's), the resolve's point-wrap tap of the
// opacity texture, clip(opacity - 0.1f) (Default.hlsl:111-113). True: the fragment is discarded.
__device__ __forceinline__ bool alpha_discards(const RasterArgs& a, const AlphaTri& al, const float l[3]) {
    float p[3], q[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) p[v] = l[v] * al.rw[v];
    perspective_weights(p, q);
    const float tu = interpolate(q, al.u[0], al.u[1], al.u[2]);
    const float tv = interpolate(q, al.v[0], al.v[1], al.v[2]);
    const float o = resolve::unorm8(resolve::tap_point(a.texels, a.n_texels, al.tex, tu, tv), 0);
    return o - 0.1f < 0.0f;
}

// ---- One point (steps 5-7) ----
// Sample sm of a pixel is at (256 x + 128 + sample_dx(sm), 256 y + 128 + sample_dy(sm)): (-2, -6), (6, -2), (-6, 2),
// (2, 6) sixteenths of a pixel from the centre, D3D's standard pattern, which lies on the 1/256 grid.
__device__ __forceinline__ int sample_dx(int s) { return s == 0 ? -32 : (s == 1 ? 96 : (s == 2 ? -96 : 32)); }
__device__ __forceinline__ int sample_dy(int s) { return s == 0 ? -96 : (s == 1 ? -32 : (s == 2 ? 32 : 96)); }

// What became of a point. kFragment: a fragment exists (covered, z in [0, 1)). Mode::Alpha: kFragTested: it reached
// the alpha test; kFragDiscarded: the test discarded it (no visibility update). Mode::Peel: kFragUpdate: it was
// eligible and issued a visibility update.
constexpr uint32_t kFragment = 1u, kFragTested = 2u, kFragDiscarded = 4u, kFragUpdate = 2u;

// A lane's (or workgroup's) counts of those results; a mode counts its own bits. kFragTested and kFragUpdate are the
// same bit and share the field `bit1`: a kernel has one mode, and a call with ALPHA and PEEL together would need a bit
// and a field of its own for the updates (the kernels' static_asserts refuse that pair today; a fourth field changes
// the layer setup kernel: profiles/raster_once/counts_with_four_fields.txt).
struct Counts {
    uint32_t frags = 0, bit1 = 0, discarded = 0;
    static_assert(kFragTested == kFragUpdate, "bit1 counts one of them: separate them before a mode has both");
    __device__ __forceinline__ uint32_t tested() const { return bit1; }   // Mode::Alpha
    __device__ __forceinline__ uint32_t updates() const { return bit1; }  // Mode::Peel
    template <Mode M>
    __device__ __forceinline__ void add(uint32_t r) {
        if constexpr (M == Mode::Alpha) {
            frags += r & 1u;
            bit1 += (r >> 1) & 1u;
            discarded += r >> 2;
        } else if constexpr (M == Mode::Peel) {
            frags += r & 1u;
            bit1 += r / kFragUpdate;
        } else {
            frags += r;
        }
    }
};

// Coverage, the depth range, the mode's test and the visibility update at the centre of pixel (x, y) for triangle (or
// piece) s with ordinal prim; the result word.
// Mode::Alpha: step 6a, with al, between the depth range and the update.
// Mode::Peel: the eligibility test there, and the key's halves exchanged: (ordinal << 32) | bits(z), so the smallest
// eligible ordinal wins. A fragment is eligible iff z < depth_in (a NaN depth_in: never) and prim >= the floor.
// depth_in and prim_in are read only after coverage and the depth range passed; both only read here (the resolve,
// later in stream order, is what may overwrite them).
template <Mode M>
__device__ __forceinline__ uint32_t raster_point(const RasterArgs& a, const Tri& s, const Edges& e, const float z[3],
                                                 const AlphaTri* al, uint32_t prim, int x, int y) {
    const long long E[3] = {edge_at_centre(e, 0, x, y), edge_at_centre(e, 1, x, y), edge_at_centre(e, 2, x, y)};
    if (!covered(e, E)) return 0u;
    float l[3];
    barycentrics(E, s.A, l);
    const float zf = interpolate_z(l, z);
    if (!(zf >= 0.0f && zf < 1.0f)) return 0u;  // depth clip and LESS against 1; NaN: no fragment
    uint32_t r = kFragment;
    if constexpr (M == Mode::Alpha) {
        if (al->tested) {
            r |= kFragTested;
            if (alpha_discards(a, *al, l)) return r | kFragDiscarded;
        }
    }
    [[maybe_unused]] const int band_h = a.row_end - a.row_begin;
    if constexpr (M == Mode::Peel) {
        const int64_t i = PBR_BOUNDS_PIXEL((int64_t)(y - a.row_begin) * a.stride + x, a.width, band_h, a.stride, 1,
                                           kBoundsRaster);
        if (!(zf < a.depth_in[i])) return kFragment;
        if (a.prim_in != nullptr && prim < a.prim_in[i]) return kFragment;
    }
    unsigned long long key;
    if constexpr (M == Mode::Peel)
        key = ((unsigned long long)prim << 32) | (unsigned long long)__float_as_uint(zf);
    else
        key = ((unsigned long long)__float_as_uint(zf) << 32) | (unsigned long long)prim;
    [[maybe_unused]] const int64_t n_vis = (int64_t)band_h * a.width;
    atomicMin(a.vis + PBR_BOUNDS((int64_t)(y - a.row_begin) * a.width + x, n_vis, kBoundsRaster), key);
    if constexpr (M == Mode::Peel) return kFragment | kFragUpdate;
    return r;
}

// raster_point<Mode::Plain> at the four samples of pixel (x, y), into the caller's surface; the sample fragments that
// exist (0 .. 4). (Apart from raster_point: profiles/raster_once/samples_in_point_routine.txt.)
__device__ __forceinline__ uint32_t raster_pixel_samples(const MsaaArgs& m, const Tri& s, const Edges& e,
                                                         const float z[3], uint32_t prim, int x, int y) {
    const RasterArgs& a = m.r;
    const int band_h = a.row_end - a.row_begin;
    const int64_t plane = (int64_t)band_h * m.vis_stride;
    const int64_t i = PBR_BOUNDS_PIXEL((int64_t)(y - a.row_begin) * m.vis_stride + x, a.width, band_h, m.vis_stride, 1,
                                       kBoundsRaster);
    uint32_t frags = 0;
#pragma unroll
    for (int sm = 0; sm < kSamples; ++sm) {
        const int px = 256 * x + 128 + sample_dx(sm), py = 256 * y + 128 + sample_dy(sm);
        const long long E[3] = {edge_at(e, 0, px, py), edge_at(e, 1, px, py), edge_at(e, 2, px, py)};
        if (!covered(e, E)) continue;
        float l[3];
        barycentrics(E, s.A, l);
        const float zf = interpolate_z(l, z);
        if (!(zf >= 0.0f && zf < 1.0f)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(zf) << 32) | (unsigned long long)prim;
        atomicMin(m.vis + sm * plane + i, key);
        ++frags;
    }
    return frags;
}

// The coverage of a triangle (or piece) with a small box, by its setup lane (the unflagged setup kernel keeps its
// loop written out: profiles/raster_once/small_loop_as_function.txt).
template <Mode M>
__device__ __forceinline__ void raster_small(const RasterArgs& a, const Tri& s, const Box& b, const float z[3],
                                             const AlphaTri* al, uint32_t prim, Counts& n) {
    Edges e;
    tri_edges(s, e);
    if constexpr (M == Mode::Plain) {  // one sum per piece: profiles/raster_once/small_loop_plain_sum.txt
        uint32_t frags = 0;
        for (int y = b.y0; y <= b.y1; ++y)
            for (int x = b.x0; x <= b.x1; ++x) frags += raster_point<M>(a, s, e, z, al, prim, x, y);
        n.frags += frags;
    } else {
        for (int y = b.y0; y <= b.y1; ++y)
            for (int x = b.x0; x <= b.x1; ++x) n.add<M>(raster_point<M>(a, s, e, z, al, prim, x, y));
    }
}

// ---- Near-plane clipping (step 2a) ----
// A piece of a clipped triangle after setup: s as for a triangle, with s.rec[v] the submitted vertex that piece
// vertex v is (recb[v] == s.rec[v]) or the inside end of the edge whose crossing with z = 0 it is (recb[v]: the outside
// end); t, ndc z and 1 / w of the three vertices, in s's order.
struct Piece {
    Tri s;
    uint32_t recb[3];
    float t[3], z[3], rw[3];
};

__device__ __forceinline__ uint32_t pick3(const uint32_t r[3], int i) { return i == 0 ? r[0] : (i == 1 ? r[1] : r[2]); }

// Pieces of a triangle with n inside vertices: 0, 1, 2 (and the triangle itself for 3).
__device__ __forceinline__ int clip_pieces(uint32_t outside) {
    const int n = 3 - (int)__popc(outside);
    return n < 2 ? n : (n == 2 ? 2 : 1);
}

// Piece `piece` of the triangle `src` that tri_setup<true> returned kTriClipped for, with `outside` its mask: the
// vertices of rule 2a.4, steps 2-3 on the new ones, then step 4 on the piece. With i the inside vertex of n = 1 or the
// outside vertex of n = 2 and (i, j, k) in cyclic index order: n = 1: (v_i, c_ij, c_ik); n = 2: piece 0 (c_ji, v_j, v_k),
// piece 1 (c_ji, v_k, c_ki), c_ab the crossing computed from inside a to outside b.
__device__ __forceinline__ TriStatus piece_setup(const RasterArgs& a, const Tri& src, uint32_t outside, int piece,
                                                 Piece& P) {
    const bool one_inside = __popc(outside) == 2;
    const uint32_t odd = one_inside ? (~outside & 7u) : outside;  // one bit
    const int i = odd == 1u ? 0 : (odd == 2u ? 1 : 2);
    const uint32_t ri = pick3(src.rec, i), rj = pick3(src.rec, (i + 1) % 3), rk = pick3(src.rec, (i + 2) % 3);
    Tri& s = P.s;
    if (one_inside) {
        s.rec[0] = ri, s.rec[1] = ri, s.rec[2] = ri;
        P.recb[0] = ri, P.recb[1] = rj, P.recb[2] = rk;
    } else if (piece == 0) {
        s.rec[0] = rj, s.rec[1] = rj, s.rec[2] = rk;
        P.recb[0] = ri, P.recb[1] = rj, P.recb[2] = rk;
    } else {
        s.rec[0] = rj, s.rec[1] = rk, s.rec[2] = rk;
        P.recb[0] = ri, P.recb[1] = rk, P.recb[2] = ri;
    }
    s.draw = src.draw;
    uint32_t flags = 0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (P.recb[v] == s.rec[v]) {  // a submitted, inside vertex: its record
            const RasterVertex& r = a.records[PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster)];
            s.X[v] = r.X;
            s.Y[v] = r.Y;
            P.z[v] = r.z;
            P.rw[v] = r.rw;
            P.t[v] = 0.0f;
            flags |= r.flags;
        } else {  // the crossing, from the inside vertex to the outside one
            const float4 pa = a.posh[PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster)];
            const float4 pb = a.posh[PBR_BOUNDS((int64_t)P.recb[v], (int64_t)a.n_records, kBoundsRaster)];
            const float t = pa.z / (pa.z - pb.z);
            const Projected c = project(a, pa.x + t * (pb.x - pa.x), pa.y + t * (pb.y - pa.y), 0.0f,
                                        pa.w + t * (pb.w - pa.w));
            s.X[v] = c.X;
            s.Y[v] = c.Y;
            P.z[v] = c.z;
            P.rw[v] = c.rw;
            P.t[v] = t;
            flags |= c.flags;
        }
    }
    if (flags & kVertexNear) return kTriNear;
    if (flags & kVertexGuard) return kTriGuard;
    // (step 4's end again, with the piece's own per-vertex values: calling tri_area changes the ten CLIP kernels,
    // profiles/raster_once/piece_setup_calls_tri_area.txt, and they have not been timed against the parent)
    long long A = (long long)(s.X[1] - s.X[0]) * (long long)(s.Y[2] - s.Y[0]) -
                  (long long)(s.X[2] - s.X[0]) * (long long)(s.Y[1] - s.Y[0]);
    if (A == 0) return kTriZeroArea;
    if (A < 0) {
        if (a.draws[PBR_BOUNDS((int64_t)s.draw, (int64_t)a.n_draws, kBoundsRaster)].cull == 0u) return kTriCulled;
        const uint32_t r1 = s.rec[1], b1 = P.recb[1];
        s.rec[1] = s.rec[2], P.recb[1] = P.recb[2];
        s.rec[2] = r1, P.recb[2] = b1;
        const int x1 = s.X[1], y1 = s.Y[1];
        s.X[1] = s.X[2], s.Y[1] = s.Y[2];
        s.X[2] = x1, s.Y[2] = y1;
        const float t1 = P.t[1], z1 = P.z[1], w1 = P.rw[1];
        P.t[1] = P.t[2], P.z[1] = P.z[2], P.rw[1] = P.rw[2];
        P.t[2] = t1, P.z[2] = z1, P.rw[2] = w1;
        A = -A;
    }
    s.A = A;
    return kTriDraw;
}

// rw and TexCoord of a piece's vertices (step 6a): the piece's rw; a new vertex's TexCoord is a + t (b - a) of its
// edge's ends, the operation resolve_clipped interpolates it with.
__device__ __forceinline__ void alpha_piece_vertices(const RasterArgs& a, const Piece& P, AlphaTri& al) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const RasterVertex& ra = a.records[PBR_BOUNDS((int64_t)P.s.rec[v], (int64_t)a.n_records, kBoundsRaster)];
        const RasterVertex& rb = a.records[PBR_BOUNDS((int64_t)P.recb[v], (int64_t)a.n_records, kBoundsRaster)];
        const bool submitted = P.recb[v] == P.s.rec[v];
        al.rw[v] = P.rw[v];
        al.u[v] = submitted ? ra.a[12] : ra.a[12] + P.t[v] * (rb.a[12] - ra.a[12]);
        al.v[v] = submitted ? ra.a[13] : ra.a[13] + P.t[v] * (rb.a[13] - ra.a[13]);
    }
}

// Sum over the wave, then one atomic from its first lane. Every lane of the wave calls it.
__device__ __forceinline__ void count_wave(unsigned long long* counter, uint32_t mine) {
    unsigned long long v = mine;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63u) == 0u && v != 0ull) atomicAdd(counter, v);
}
__device__ __forceinline__ void count_ballot(unsigned long long* counter, bool mine) {
    const uint64_t m = __ballot(mine);
    if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// Appends the wave's large triangles (or pieces: `piece` in the top bit of the block count) to the list: one atomic
// per wave. Every lane of the wave calls it.
__device__ __forceinline__ void append_large(const RasterArgs& a, bool large, const Box& b, uint32_t t, uint32_t piece,
                                             int64_t slots) {
    const uint64_t m = __ballot(large);
    if (m != 0ull) {
        const uint32_t lane = threadIdx.x & 63u;
        const int leader = (int)__builtin_ctzll(m);
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(a.counters + kRasterLarge, (unsigned long long)__popcll(m));
        base = __shfl(base, leader, 64);
        if (large) {  // the triangle and its block count: a workgroup whose slab has no block of it skips it unread
            const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            const uint32_t nb = ((uint32_t)(b.x1 - b.x0) / kBlockW + 1u) * ((uint32_t)(b.y1 - b.y0) / kBlockH + 1u);
            a.large[PBR_BOUNDS((int64_t)base + rank, slots, kBoundsRaster)] = make_uint2(t, nb | (piece << 31));
        }
    }
}

}  // namespace raster

// Stage 1: VS (Default.hlsl:27-42), the perspective division, the viewport and the snap.
// CLIP: PosH is kept as well, and a vertex with PosH.z not >= 0 (NaN included; -0.0f is inside) is marked outside.
template <bool CLIP>
__global__ __launch_bounds__(256) void raster_vertex_kernel(const RasterArgs a) {
    using namespace raster;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n_records) return;
    const int d = find_draw(a.rec_prefix, a.n_draws, g);
    const RasterDraw& dr = a.draws[PBR_BOUNDS((int64_t)d, (int64_t)a.n_draws, kBoundsRaster)];
    const uint32_t v = g - a.rec_prefix[PBR_BOUNDS((int64_t)d, (int64_t)a.n_draws + 1, kBoundsRaster)];
    const float* in = a.vertices + 14 * PBR_BOUNDS((int64_t)dr.vtx_src + (int64_t)v, a.n_src_vertices, kBoundsMesh);
    RasterVertex o;
    float pw[4], ph[4], tc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pw[j] = mul4(in[0], in[1], in[2], 1.0f, dr.world, j);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.a[j] = pw[j];
        o.a[3 + j] = mul3(in[3], in[4], in[5], dr.world, j);
        o.a[6 + j] = mul3(in[6], in[7], in[8], dr.world, j);
        o.a[9 + j] = mul3(in[9], in[10], in[11], dr.world, j);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ph[j] = mul4(pw[0], pw[1], pw[2], pw[3], a.view_proj, j);
#pragma unroll
    for (int j = 0; j < 4; ++j) tc[j] = mul4(in[12], in[13], 0.0f, 1.0f, dr.tex, j);
    o.a[12] = mul4(tc[0], tc[1], tc[2], tc[3], dr.mat, 0);
    o.a[13] = mul4(tc[0], tc[1], tc[2], tc[3], dr.mat, 1);

    const float w = ph[3];  // steps 2-3 (project() holds the same operations for a piece's new vertex)
    uint32_t flags = w > 0.0f ? 0u : kVertexNear;  // NaN: near
    const float nx = ph[0] / w, ny = ph[1] / w, nz = ph[2] / w;
    const float xs = (nx * 0.5f + 0.5f) * (float)a.width, ys = (0.5f - ny * 0.5f) * (float)a.height;
    const float tx = xs * 256.0f, ty = ys * 256.0f;
    const bool inside = fabsf(tx) < 0x1p23f && fabsf(ty) < 0x1p23f;  // false for NaN and inf
    if (!inside) flags |= kVertexGuard;
    o.X = inside ? (int)rintf(tx) : 0;
    o.Y = inside ? (int)rintf(ty) : 0;
    o.z = nz;
    o.rw = 1.0f / w;
    o.flags = flags;
    if constexpr (CLIP) {
        if (!(ph[2] >= 0.0f)) o.flags |= kVertexOutside;
        a.posh[PBR_BOUNDS((int64_t)g, (int64_t)a.n_records, kBoundsRaster)] = make_float4(ph[0], ph[1], ph[2], ph[3]);
    }
    o.pad = 0u;
    a.records[PBR_BOUNDS((int64_t)g, (int64_t)a.n_records, kBoundsRaster)] = o;
}

// Stage 2: setup of every triangle, the statistics, the small triangles' coverage, the large list. ALPHA (a call with
// PBR_RASTER_ALPHA_TEST some draw of which has a tested material): each lane has its own triangle, so the material
// record is read per lane, and rw and TexCoord only by the lane of a small triangle of a tested draw. PEEL (a layer
// call, pbr_rasterize_layer; never with ALPHA): the small triangles' fragments take the eligibility test of step 7a.
template <bool ALPHA, bool PEEL>
__global__ __launch_bounds__(256) void raster_setup_kernel(const RasterArgs a) {
    static_assert(!(ALPHA && PEEL), "a layer call runs no alpha test");
    using namespace raster;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool valid = t < a.n_tris;
    Tri s;
    TriStatus st = kTriZeroArea;
    if (valid) st = tri_setup(a, t, s);
    count_ballot(a.counters + kRasterCulled, valid && st == kTriCulled);
    count_ballot(a.counters + kRasterZeroArea, valid && st == kTriZeroArea);
    count_ballot(a.counters + kRasterNear, valid && st == kTriNear);
    count_ballot(a.counters + kRasterGuard, valid && st == kTriGuard);
    Box b{0, -1, 0, -1};
    const bool draw = valid && st == kTriDraw && tri_box(a, s, 0, b);
    const long long npix = draw ? (long long)(b.x1 - b.x0 + 1) * (long long)(b.y1 - b.y0 + 1) : 0;
    const bool small = draw && npix <= kSmallPixels, large = draw && !small;

    constexpr Mode M = mode_of(ALPHA, PEEL);
    Counts n;
    if constexpr (M == Mode::Alpha) {
        if (small) {
            float z[3];
            load_z(a, s, z);
            AlphaTri al;
            alpha_material<false>(a, s.draw, al);
            if (al.tested) alpha_vertices(a, s, al);
            raster_small<M>(a, s, b, z, &al, t, n);
        }
        count_wave(a.counters + kRasterAlphaTested, n.tested());
        count_wave(a.counters + kRasterAlphaDiscarded, n.discarded);
    } else if constexpr (M == Mode::Peel) {
        if (small) {
            float z[3];
            load_z(a, s, z);
            raster_small<M>(a, s, b, z, nullptr, t, n);
        }
        count_wave(a.counters + kRasterLayerFragments, n.updates());
    } else if (small) {
        Edges e;
        tri_edges(s, e);
        float z[3];
        load_z(a, s, z);
        for (int y = b.y0; y <= b.y1; ++y)
            for (int x = b.x0; x <= b.x1; ++x) n.add<M>(raster_point<M>(a, s, e, z, nullptr, t, x, y));
    }
    count_wave(a.counters + kRasterFragments, n.frags);

    append_large(a, large, b, t, 0u, (int64_t)a.n_tris);
}

// Stage 2 with near clipping: the lane of a clipped triangle walks its (at most two) pieces; each is counted,
// rasterised or listed as a submitted triangle would be. Both rounds of the piece loop are taken by every lane, so the
// wave-wide ballots and sums inside it see the whole wave. ALPHA: as in raster_setup_kernel; a piece takes the test with
// its own rw and its new vertices' TexCoord. PEEL: as in raster_setup_kernel; the pieces of a triangle share its ordinal.
template <bool ALPHA, bool PEEL>
__global__ __launch_bounds__(256) void raster_setup_clip_kernel(const RasterArgs a) {
    static_assert(!(ALPHA && PEEL), "a layer call runs no alpha test");
    using namespace raster;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    Tri src;
    uint32_t outside = 0;
    TriStatus st = kTriNone;
    if (t < a.n_tris) st = tri_setup<true>(a, t, src, &outside);
    const bool clipped = st == kTriClipped;
    const int n_pieces = clipped ? clip_pieces(outside) : (st == kTriDraw ? 1 : 0);
    count_ballot(a.counters + kRasterClipped, clipped);
    count_wave(a.counters + kRasterClipPieces, clipped ? (uint32_t)n_pieces : 0u);
    // what the triangle itself adds to the skip counters; its pieces add theirs below
    uint32_t culled = st == kTriCulled, zero = st == kTriZeroArea, near = st == kTriNear, guard = st == kTriGuard;
    constexpr Mode M = mode_of(ALPHA, PEEL);
    Counts n;
    for (int p = 0; p < 2; ++p) {
        Piece P;
        Box b{0, -1, 0, -1};
        TriStatus ps = kTriNone;
        if (p < n_pieces) {
            if (clipped) {
                ps = piece_setup(a, src, outside, p, P);
                culled += ps == kTriCulled, zero += ps == kTriZeroArea, near += ps == kTriNear, guard += ps == kTriGuard;
            } else {
                P.s = src;
                ps = kTriDraw;
            }
        }
        const bool draw = ps == kTriDraw && tri_box(a, P.s, 0, b);
        const long long npix = draw ? (long long)(b.x1 - b.x0 + 1) * (long long)(b.y1 - b.y0 + 1) : 0;
        const bool small = draw && npix <= kSmallPixels, large = draw && !small;
        if (small) {
            if (!clipped) load_z(a, P.s, P.z);
            if constexpr (M == Mode::Alpha) {
                AlphaTri al;
                alpha_material<false>(a, P.s.draw, al);
                if (al.tested) {
                    if (clipped)
                        alpha_piece_vertices(a, P, al);
                    else
                        alpha_vertices(a, P.s, al);
                }
                raster_small<M>(a, P.s, b, P.z, &al, t, n);
            } else {
                raster_small<M>(a, P.s, b, P.z, nullptr, t, n);
            }
        }
        append_large(a, large, b, t, (uint32_t)p, a.n_large);
    }
    count_wave(a.counters + kRasterCulled, culled);
    count_wave(a.counters + kRasterZeroArea, zero);
    count_wave(a.counters + kRasterNear, near);
    count_wave(a.counters + kRasterGuard, guard);
    count_wave(a.counters + kRasterFragments, n.frags);
    if constexpr (M == Mode::Alpha) {
        count_wave(a.counters + kRasterAlphaTested, n.tested());
        count_wave(a.counters + kRasterAlphaDiscarded, n.discarded);
    }
    if constexpr (M == Mode::Peel) count_wave(a.counters + kRasterLayerFragments, n.updates());
}

// Stage 3: the large triangles. blockIdx.x strides over the list, blockIdx.y over the triangle's 64 x 4 blocks; a wave
// is one row of a block. All control flow outside the pixel test is uniform over the workgroup. CLIP: an entry names a
// triangle or, with the piece's number in the top bit of its block count, a piece of a clipped one.
// ALPHA: the workgroup's triangle has one draw, so its material record and the "tested" decision are wave-uniform: the
// record arrives by scalar loads and the test's branch is uniform; only the texel fetch is per lane.
// PEEL (never with ALPHA): a lane reads depth_in and the floor of its own pixel, after coverage and the depth range
// passed; the lanes of a wave are adjacent in x, so these are coalesced 4-byte loads.
template <bool CLIP, bool ALPHA, bool PEEL>
__global__ __launch_bounds__(256) void raster_large_kernel(const RasterArgs a) {
    static_assert(!(ALPHA && PEEL), "a layer call runs no alpha test");
    using namespace raster;
    const unsigned long long listed = a.counters[kRasterLarge];
    const uint32_t slots = CLIP ? (uint32_t)a.n_large : a.n_tris;
    const uint32_t n_large = listed < (unsigned long long)slots ? (uint32_t)listed : slots;
    constexpr Mode M = mode_of(ALPHA, PEEL);
    Counts n;
    for (uint32_t i = blockIdx.x; i < n_large; i += gridDim.x) {
        const uint2 entry = a.large[PBR_BOUNDS((int64_t)i, (int64_t)slots, kBoundsRaster)];
        const uint32_t blocks = CLIP ? entry.y & 0x7FFFFFFFu : entry.y;
        if (blockIdx.y >= blocks) continue;
        const uint32_t t = entry.x;
        Tri s;
        Box b;
        float z[3];
        [[maybe_unused]] AlphaTri al;
        if constexpr (CLIP) {
            uint32_t outside = 0;
            const TriStatus st = tri_setup<true>(a, t, s, &outside);
            if constexpr (ALPHA) alpha_material<true>(a, s.draw, al);
            if (st == kTriClipped) {
                Piece P;
                if (piece_setup(a, s, outside, (int)(entry.y >> 31), P) != kTriDraw) continue;  // never, as below
                s = P.s;
#pragma unroll
                for (int v = 0; v < 3; ++v) z[v] = P.z[v];
                if constexpr (ALPHA)
                    if (al.tested) alpha_piece_vertices(a, P, al);
            } else {
                if (st != kTriDraw) continue;
                load_z(a, s, z);
                if constexpr (ALPHA)
                    if (al.tested) alpha_vertices(a, s, al);
            }
            if (!tri_box(a, s, 0, b)) continue;
        } else {
            if (tri_setup(a, t, s) != kTriDraw || !tri_box(a, s, 0, b)) continue;  // never: the setup kernel listed it
        }
        const uint32_t nbx = (uint32_t)(b.x1 - b.x0) / kBlockW + 1u, nby = (uint32_t)(b.y1 - b.y0) / kBlockH + 1u;
        const uint32_t nb = nbx * nby;
        if (blockIdx.y >= nb) continue;
        Edges e;
        tri_edges(s, e);
        if constexpr (!CLIP) load_z(a, s, z);
        if constexpr (!CLIP && ALPHA) {
            alpha_material<true>(a, s.draw, al);
            if (al.tested) alpha_vertices(a, s, al);
        }
        for (uint32_t blk = blockIdx.y; blk < nb; blk += gridDim.y) {
            const int X0 = b.x0 + (int)(blk % nbx) * kBlockW, Y0 = b.y0 + (int)(blk / nbx) * kBlockH;
            const int X1 = min(X0 + kBlockW - 1, b.x1), Y1 = min(Y0 + kBlockH - 1, b.y1);
            bool reject = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) {  // an edge function is linear: its maximum over the block is at a corner
                const long long m = max(max(edge_at_centre(e, k, X0, Y0), edge_at_centre(e, k, X1, Y0)),
                                        max(edge_at_centre(e, k, X0, Y1), edge_at_centre(e, k, X1, Y1)));
                reject = reject || m < 0;
            }
            if (reject) continue;
            const int x = X0 + (int)(threadIdx.x & 63u), y = Y0 + (int)(threadIdx.x >> 6);
            if (x <= X1 && y <= Y1) n.add<M>(raster_point<M>(a, s, e, z, &al, t, x, y));
        }
    }
    count_wave(a.counters + kRasterFragments, n.frags);
    if constexpr (M == Mode::Alpha) {
        count_wave(a.counters + kRasterAlphaTested, n.tested());
        count_wave(a.counters + kRasterAlphaDiscarded, n.discarded);
    }
    if constexpr (M == Mode::Peel) count_wave(a.counters + kRasterLayerFragments, n.updates());
}

namespace raster {

// Step 9: a pixel without a fragment.
__device__ __forceinline__ void background_pixel(const RasterArgs& a, int x, int y, float out[14], uint32_t& material,
                                                 float& depth) {
    const float sx = (float)(2 * x + 1) / (float)a.width - 1.0f;
    const float sy = 1.0f - (float)(2 * y + 1) / (float)a.height;
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (a.fwd[c] + sx * a.right[c]) + sy * a.up[c];
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float n = d[c] / len;
        out[3 + c] = n;
        out[c] = a.eye[c] + n * 100.0f;
    }
#pragma unroll
    for (int k = 6; k < 14; ++k) out[k] = 0.0f;
    material = 0xFFFFu;
    depth = 1.0f;
}

// Step 2a.8: the winner is a clipped triangle: its lowest-numbered piece that covers the pixel centre with a z in
// [0, 1) whose bits are the key's; the attributes from that piece's vertices, a new vertex's as a + t (b - a) from its
// edge's inside end a to its outside end b. False when no piece qualifies (never: one of them wrote the key).
__device__ __forceinline__ bool resolve_clipped(const RasterArgs& a, const Tri& src, uint32_t outside,
                                                unsigned long long key, int x, int y, float out[14],
                                                uint32_t& material, float& depth) {
    const int n_pieces = clip_pieces(outside);
    for (int piece = 0; piece < n_pieces; ++piece) {
        Piece P;
        if (piece_setup(a, src, outside, piece, P) != kTriDraw) continue;
        Edges e;
        tri_edges(P.s, e);
        const long long E[3] = {edge_at_centre(e, 0, x, y), edge_at_centre(e, 1, x, y), edge_at_centre(e, 2, x, y)};
        if (!covered(e, E)) continue;
        float l[3], p[3], q[3];
        barycentrics(E, P.s.A, l);
        const float zf = interpolate_z(l, P.z);
        if (!(zf >= 0.0f && zf < 1.0f) || __float_as_uint(zf) != (uint32_t)(key >> 32)) continue;
        depth = zf;
#pragma unroll
        for (int v = 0; v < 3; ++v) p[v] = l[v] * P.rw[v];
        perspective_weights(p, q);
        const RasterVertex *ra[3], *rb[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            ra[v] = a.records + PBR_BOUNDS((int64_t)P.s.rec[v], (int64_t)a.n_records, kBoundsRaster);
            rb[v] = a.records + PBR_BOUNDS((int64_t)P.recb[v], (int64_t)a.n_records, kBoundsRaster);
        }
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            float av[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const float fa = ra[v]->a[k], fb = rb[v]->a[k];
                av[v] = P.recb[v] == P.s.rec[v] ? fa : fa + P.t[v] * (fb - fa);
            }
            out[k] = interpolate(q, av[0], av[1], av[2]);
        }
        material = a.draws[PBR_BOUNDS((int64_t)P.s.draw, (int64_t)a.n_draws, kBoundsRaster)].material;
        return true;
    }
    return false;
}

// One pixel of the band: the winner's attributes (step 8) or the background (step 9). PEEL: the visibility word of a
// layer call holds the ordinal in its high half and the z bits in its low half; exchanged, it is the word the steps
// below know (all ones stays all ones).
template <bool CLIP, bool PEEL>
__device__ __forceinline__ void resolve_pixel(const RasterArgs& a, int x, int y, float out[14], uint32_t& material,
                                              float& depth) {
    [[maybe_unused]] const int64_t n_vis = (int64_t)(a.row_end - a.row_begin) * a.width;
    unsigned long long key = a.vis[PBR_BOUNDS((int64_t)(y - a.row_begin) * a.width + x, n_vis, kBoundsRaster)];
    if constexpr (PEEL) key = (key << 32) | (key >> 32);
    Tri s;
    if constexpr (CLIP) {
        uint32_t outside = 0;
        const TriStatus st = key == ~0ull ? kTriNone : tri_setup<true>(a, (uint32_t)key, s, &outside);
        if (st == kTriClipped && resolve_clipped(a, s, outside, key, x, y, out, material, depth)) return;
        if (st != kTriDraw) {
            background_pixel(a, x, y, out, material, depth);
            return;
        }
    } else {
        if (key == ~0ull || tri_setup(a, (uint32_t)key, s) != kTriDraw) {  // (a winner always sets up as drawn)
            background_pixel(a, x, y, out, material, depth);
            return;
        }
    }
    Edges e;
    tri_edges(s, e);
    const long long E[3] = {edge_at_centre(e, 0, x, y), edge_at_centre(e, 1, x, y), edge_at_centre(e, 2, x, y)};
    float l[3], p[3], q[3];
    barycentrics(E, s.A, l);
    const RasterVertex* r[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) r[v] = a.records + PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster);
    const float z[3] = {r[0]->z, r[1]->z, r[2]->z};
    depth = interpolate_z(l, z);  // the key's z: the same operations on the same values
#pragma unroll
    for (int v = 0; v < 3; ++v) p[v] = l[v] * r[v]->rw;
    perspective_weights(p, q);
#pragma unroll
    for (int k = 0; k < 14; ++k) out[k] = interpolate(q, r[0]->a[k], r[1]->a[k], r[2]->a[k]);
    material = a.draws[PBR_BOUNDS((int64_t)s.draw, (int64_t)a.n_draws, kBoundsRaster)].material;
}

// Step 7a's end at band pixel (x, yb), plane offset oi: with a winner (its depth is already the winner's z) the next
// floor is its ordinal + 1; without one the depth is depth_in's value passed through and the floor 0xFFFFFFFF, which
// no ordinal reaches.
__device__ __forceinline__ void peel_pixel(const RasterArgs& a, int x, int yb, int64_t oi, float& depth,
                                           uint32_t& floor) {
    const int band_h = a.row_end - a.row_begin;
    [[maybe_unused]] const int64_t n_vis = (int64_t)band_h * a.width;
    const unsigned long long key = a.vis[PBR_BOUNDS((int64_t)yb * a.width + x, n_vis, kBoundsRaster)];
    if (key != ~0ull) {
        floor = (uint32_t)(key >> 32) + 1u;
    } else {
        depth = a.depth_in[PBR_BOUNDS_PIXEL(oi, a.width, band_h, a.stride, 1, kBoundsRaster)];
        floor = 0xFFFFFFFFu;
    }
}

}  // namespace raster

// Stage 4: per pixel, the material resolve's tile: 256 threads over 64 x 8 pixels, a pixel pair per lane, 8-byte
// plane stores when VEC. PEEL (step 7a): a pixel without a winner keeps depth_in's value as its depth, and every
// pixel writes its next floor to prim_out. A lane reads depth_in (which may be the depth plane) at its own pixels only,
// before it stores them.
template <bool VEC, bool CLIP, bool PEEL>
__global__ __launch_bounds__(256) void raster_resolve_kernel(const RasterArgs a) {
    using namespace raster;
    const int band_h = a.row_end - a.row_begin;
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 31u) * 2;
    const int yb = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);  // row of the band
    const bool in0 = yb < band_h && x < a.width, in1 = yb < band_h && x + 1 < a.width;
    float v0[14], v1[14], z0 = 1.0f, z1 = 1.0f;
    uint32_t m0 = 0xFFFFu, m1 = 0xFFFFu;
    if (in0) resolve_pixel<CLIP, PEEL>(a, x, a.row_begin + yb, v0, m0, z0);
    if (in1) resolve_pixel<CLIP, PEEL>(a, x + 1, a.row_begin + yb, v1, m1, z1);
    const int64_t oi = (int64_t)yb * a.stride + x;
    [[maybe_unused]] uint32_t f0 = 0xFFFFFFFFu, f1 = 0xFFFFFFFFu;
    if constexpr (PEEL) {
        if (in0) peel_pixel(a, x, yb, oi, z0, f0);
        if (in1) peel_pixel(a, x + 1, yb, oi + 1, z1, f1);
    }
    if (VEC && in1) {
        const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, band_h, a.stride, 2, kBoundsOutput);
#pragma unroll
        for (int k = 0; k < 14; ++k) *reinterpret_cast<float2*>(a.plane[k] + i) = make_float2(v0[k], v1[k]);
        *reinterpret_cast<uint32_t*>(a.material + i) = m0 | (m1 << 16);
        if (a.depth) *reinterpret_cast<float2*>(a.depth + i) = make_float2(z0, z1);
        if constexpr (PEEL) *reinterpret_cast<uint2*>(a.prim_out + i) = make_uint2(f0, f1);
    } else {
        if (in0) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, band_h, a.stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 14; ++k) a.plane[k][i] = v0[k];
            a.material[i] = (uint16_t)m0;
            if (a.depth) a.depth[i] = z0;
            if constexpr (PEEL) a.prim_out[i] = f0;
        }
        if (in1) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi + 1, a.width, band_h, a.stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 14; ++k) a.plane[k][i] = v1[k];
            a.material[i] = (uint16_t)m1;
            if (a.depth) a.depth[i] = z1;
            if constexpr (PEEL) a.prim_out[i] = f1;
        }
    }
}

namespace raster {

// A runtime flag as a compile-time one: f(std::true_type) or f(std::false_type).
template <class F>
void with_bool(bool flag, F&& f) {
    if (flag)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// The call's mode likewise, as the kernels' (ALPHA, PEEL): a layer call runs no alpha test, so (true, true) is never
// named and never instantiated.
template <class F>
void with_mode(const RasterArgs& a, F&& f) {
    if (a.peel)
        f(std::false_type{}, std::true_type{});
    else
        with_bool(a.alpha_test, [&](auto alpha) { f(alpha, std::false_type{}); });
}

}  // namespace raster

hipError_t launch_raster_vertices(const RasterArgs& a, hipStream_t stream) {
    if (a.n_records == 0u) return hipSuccess;
    const dim3 grid((a.n_records + 255u) / 256u);
    raster::with_bool(a.clip_near, [&](auto clip) {
        hipLaunchKernelGGL((raster_vertex_kernel<decltype(clip)::value>), grid, dim3(256), 0, stream, a);
    });
    return hipGetLastError();
}

hipError_t launch_raster_setup(const RasterArgs& a, hipStream_t stream) {
    if (a.n_tris == 0u) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)a.n_tris + 255u) / 256u));
    raster::with_mode(a, [&](auto alpha, auto peel) {
        constexpr bool ALPHA = decltype(alpha)::value, PEEL = decltype(peel)::value;
        if (a.clip_near)
            hipLaunchKernelGGL((raster_setup_clip_kernel<ALPHA, PEEL>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((raster_setup_kernel<ALPHA, PEEL>), grid, dim3(256), 0, stream, a);
    });
    return hipGetLastError();
}

hipError_t launch_raster_large(const RasterArgs& a, hipStream_t stream) {
    if (a.n_tris == 0u) return hipSuccess;
    const uint32_t gx = a.n_tris < (uint32_t)raster::kLargeGridX ? a.n_tris : (uint32_t)raster::kLargeGridX;
    const dim3 grid(gx, raster::kLargeSlabs);
    raster::with_bool(a.clip_near, [&](auto clip) {
        raster::with_mode(a, [&](auto alpha, auto peel) {
            constexpr bool CLIP = decltype(clip)::value, ALPHA = decltype(alpha)::value, PEEL = decltype(peel)::value;
            hipLaunchKernelGGL((raster_large_kernel<CLIP, ALPHA, PEEL>), grid, dim3(256), 0, stream, a);
        });
    });
    return hipGetLastError();
}

hipError_t launch_raster_resolve(const RasterArgs& a, hipStream_t stream) {
    const int band_h = a.row_end - a.row_begin;
    if (a.width <= 0 || band_h <= 0) return hipSuccess;
    const dim3 grid((a.width + 63) / 64, (band_h + 7) / 8);
    raster::with_bool(a.vec, [&](auto vec) {
        raster::with_bool(a.clip_near, [&](auto clip) {
            raster::with_bool(a.peel, [&](auto peel) {
                constexpr bool VEC = decltype(vec)::value, CLIP = decltype(clip)::value, PEEL = decltype(peel)::value;
                hipLaunchKernelGGL((raster_resolve_kernel<VEC, CLIP, PEEL>), grid, dim3(256), 0, stream, a);
            });
        });
    });
    return hipGetLastError();
}

// ---- Four samples per pixel (step 7b; pbr_msaa_rasterize, pbr_msaa_fragments) -------------------------------------
// Coverage and depth are steps 5-6 at the four sample points of a pixel, D3D's standard pattern in 1/16 pixel, which
// lies on the 1/256 grid; visibility is step 7's key lowered by atomicMin into one word per (sample, pixel) of the
// caller's surface, sample-major. The setup and large kernels follow raster_setup_kernel<false, false> and
// raster_large_kernel<false, false, false> with the sample box (tri_box with kSampleReach) and the sample routine
// (profiles/raster_once/kernel_body_as_function.txt keeps the flows apart).
// Stage 2 for samples: raster_setup_kernel's flow with the sample box: a triangle whose box of pixels with reachable
// samples holds at most kSmallPixels pixels is rasterised by its lane (at most 4 kSmallPixels sample tests), the others
// are listed. A triangle that covers a sample but no pixel centre has an empty centre box and a non-empty sample box.
__global__ __launch_bounds__(256) void raster_setup_msaa_kernel(const MsaaArgs m) {
    using namespace raster;
    const RasterArgs& a = m.r;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool valid = t < a.n_tris;
    Tri s;
    TriStatus st = kTriZeroArea;
    if (valid) st = tri_setup(a, t, s);
    count_ballot(a.counters + kRasterCulled, valid && st == kTriCulled);
    count_ballot(a.counters + kRasterZeroArea, valid && st == kTriZeroArea);
    count_ballot(a.counters + kRasterNear, valid && st == kTriNear);
    count_ballot(a.counters + kRasterGuard, valid && st == kTriGuard);
    Box b{0, -1, 0, -1};
    const bool draw = valid && st == kTriDraw && tri_box(a, s, kSampleReach, b);
    const long long npix = draw ? (long long)(b.x1 - b.x0 + 1) * (long long)(b.y1 - b.y0 + 1) : 0;
    const bool small = draw && npix <= kSmallPixels, large = draw && !small;
    uint32_t frags = 0;
    if (small) {
        Edges e;
        tri_edges(s, e);
        float z[3];
        load_z(a, s, z);
        for (int y = b.y0; y <= b.y1; ++y)
            for (int x = b.x0; x <= b.x1; ++x) frags += raster_pixel_samples(m, s, e, z, t, x, y);
    }
    count_wave(a.counters + kRasterFragments, frags);
    append_large(a, large, b, t, 0u, (int64_t)a.n_tris);
}

// Stage 3 for samples: raster_large_kernel<false, false, false>'s flow over the sample box. A block is skipped when
// some edge function is negative at the four corners of the rectangle that holds every sample point of the block (the
// block's corner pixel centres moved outwards by kSampleReach): linear, so negative at every sample of the block.
__global__ __launch_bounds__(256) void raster_large_msaa_kernel(const MsaaArgs m) {
    using namespace raster;
    const RasterArgs& a = m.r;
    const unsigned long long listed = a.counters[kRasterLarge];
    const uint32_t slots = a.n_tris;
    const uint32_t n_large = listed < (unsigned long long)slots ? (uint32_t)listed : slots;
    uint32_t frags = 0;
    for (uint32_t i = blockIdx.x; i < n_large; i += gridDim.x) {
        const uint2 entry = a.large[PBR_BOUNDS((int64_t)i, (int64_t)slots, kBoundsRaster)];
        if (blockIdx.y >= entry.y) continue;
        const uint32_t t = entry.x;
        Tri s;
        Box b;
        if (tri_setup(a, t, s) != kTriDraw || !tri_box(a, s, kSampleReach, b)) continue;  // never: setup listed it
        const uint32_t nbx = (uint32_t)(b.x1 - b.x0) / kBlockW + 1u, nby = (uint32_t)(b.y1 - b.y0) / kBlockH + 1u;
        const uint32_t nb = nbx * nby;
        if (blockIdx.y >= nb) continue;
        Edges e;
        tri_edges(s, e);
        float z[3];
        load_z(a, s, z);
        for (uint32_t blk = blockIdx.y; blk < nb; blk += gridDim.y) {
            const int X0 = b.x0 + (int)(blk % nbx) * kBlockW, Y0 = b.y0 + (int)(blk / nbx) * kBlockH;
            const int X1 = min(X0 + kBlockW - 1, b.x1), Y1 = min(Y0 + kBlockH - 1, b.y1);
            const int px0 = 256 * X0 + 128 - kSampleReach, px1 = 256 * X1 + 128 + kSampleReach;
            const int py0 = 256 * Y0 + 128 - kSampleReach, py1 = 256 * Y1 + 128 + kSampleReach;
            bool reject = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const long long mx = max(max(edge_at(e, k, px0, py0), edge_at(e, k, px1, py0)),
                                         max(edge_at(e, k, px0, py1), edge_at(e, k, px1, py1)));
                reject = reject || mx < 0;
            }
            if (reject) continue;
            const int x = X0 + (int)(threadIdx.x & 63u), y = Y0 + (int)(threadIdx.x >> 6);
            if (x <= X1 && y <= Y1) frags += raster_pixel_samples(m, s, e, z, t, x, y);
        }
    }
    count_wave(a.counters + kRasterFragments, frags);
}

namespace raster {

// One pixel of slot m.slot: the four keys, the slots and the owner byte; the slot's planes (step 8 at the pixel
// centre with the triangle of the slot's lowest sample, the depth that sample's key carries) or, for a background
// fragment or a slot the pixel does not have, step 9's. Returns the pixel's slot count (1 .. 4).
__device__ __forceinline__ int fragments_pixel(const MsaaArgs& m, int x, int y, float out[14], uint32_t& material,
                                               float& depth, uint32_t& owner) {
    const RasterArgs& a = m.r;
    const int band_h = a.row_end - a.row_begin;
    const int64_t plane = (int64_t)band_h * m.vis_stride;
    const int64_t i = PBR_BOUNDS_PIXEL((int64_t)(y - a.row_begin) * m.vis_stride + x, a.width, band_h, m.vis_stride, 1,
                                       kBoundsRaster);
    unsigned long long key[kSamples];
#pragma unroll
    for (int sm = 0; sm < kSamples; ++sm) key[sm] = m.vis[sm * plane + i];
    // the low word names the fragment: a triangle's ordinal (below 2^32 - 1), or all ones for the background
    const uint32_t id0 = (uint32_t)key[0], id1 = (uint32_t)key[1], id2 = (uint32_t)key[2], id3 = (uint32_t)key[3];
    const int s1 = id1 == id0 ? 0 : 1;
    int n = s1 + 1;
    const int s2 = id2 == id0 ? 0 : (id2 == id1 ? s1 : n++);
    const int s3 = id3 == id0 ? 0 : (id3 == id1 ? s1 : (id3 == id2 ? s2 : n++));
    owner = (uint32_t)s1 << 2 | (uint32_t)s2 << 4 | (uint32_t)s3 << 6;
    // the slot's lowest sample: slot k first appears at sample >= k
    unsigned long long k64 = ~0ull;
    if (m.slot == 0)
        k64 = key[0];
    else if (s1 == m.slot)
        k64 = key[1];
    else if (s2 == m.slot)
        k64 = key[2];
    else if (s3 == m.slot)
        k64 = key[3];
    Tri s;
    // (a winner always sets up as drawn; an ordinal past the list -- a surface of another draw list -- is not followed)
    if (k64 == ~0ull || (uint32_t)k64 >= a.n_tris || tri_setup(a, (uint32_t)k64, s) != kTriDraw) {
        background_pixel(a, x, y, out, material, depth);
        return n;
    }
    Edges e;
    tri_edges(s, e);
    const long long E[3] = {edge_at_centre(e, 0, x, y), edge_at_centre(e, 1, x, y), edge_at_centre(e, 2, x, y)};
    float l[3], p[3], q[3];
    barycentrics(E, s.A, l);  // at the centre, inside the triangle or not: no clamp
    const RasterVertex* r[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) r[v] = a.records + PBR_BOUNDS((int64_t)s.rec[v], (int64_t)a.n_records, kBoundsRaster);
    depth = __uint_as_float((uint32_t)(k64 >> 32));
#pragma unroll
    for (int v = 0; v < 3; ++v) p[v] = l[v] * r[v]->rw;
    perspective_weights(p, q);
#pragma unroll
    for (int k = 0; k < 14; ++k) out[k] = interpolate(q, r[0]->a[k], r[1]->a[k], r[2]->a[k]);
    material = a.draws[PBR_BOUNDS((int64_t)s.draw, (int64_t)a.n_draws, kBoundsRaster)].material;
    return n;
}

}  // namespace raster

// The fragments stage, on the resolve's tile: 256 threads over 64 x 8 pixels, a pixel pair per lane, 8-byte plane
// stores when VEC. slot_pixels of slots 1 .. 3: per wave and slot one ballot per pixel of the pair and one atomic.
template <bool VEC>
__global__ __launch_bounds__(256) void raster_fragments_msaa_kernel(const MsaaArgs m) {
    using namespace raster;
    const RasterArgs& a = m.r;
    const int band_h = a.row_end - a.row_begin;
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 31u) * 2;
    const int yb = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);  // row of the band
    const bool in0 = yb < band_h && x < a.width, in1 = yb < band_h && x + 1 < a.width;
    float v0[14], v1[14], z0 = 1.0f, z1 = 1.0f;
    uint32_t m0 = 0xFFFFu, m1 = 0xFFFFu, o0 = 0u, o1 = 0u;
    int n0 = 0, n1 = 0;
    if (in0) n0 = fragments_pixel(m, x, a.row_begin + yb, v0, m0, z0, o0);
    if (in1) n1 = fragments_pixel(m, x + 1, a.row_begin + yb, v1, m1, z1, o1);
    // (slot 0 exists in every pixel: the host stores the band's pixel count. A wave of one-fragment pixels -- nearly
    // every wave -- then issues no atomic; one per wave on the same word would serialise the whole launch.)
#pragma unroll
    for (int k = 1; k < kSamples; ++k) {
        const uint64_t b0 = __ballot(n0 > k), b1 = __ballot(n1 > k);
        if ((threadIdx.x & 63u) == 0u && (b0 | b1) != 0ull)
            atomicAdd(a.counters + kRasterSlotPixels + k, (unsigned long long)(__popcll(b0) + __popcll(b1)));
    }
    const int64_t oi = (int64_t)yb * a.stride + x;
    if (VEC && in1) {
        const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, band_h, a.stride, 2, kBoundsOutput);
#pragma unroll
        for (int k = 0; k < 14; ++k) *reinterpret_cast<float2*>(a.plane[k] + i) = make_float2(v0[k], v1[k]);
        *reinterpret_cast<uint32_t*>(a.material + i) = m0 | (m1 << 16);
        if (a.depth) *reinterpret_cast<float2*>(a.depth + i) = make_float2(z0, z1);
    } else {
        if (in0) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi, a.width, band_h, a.stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 14; ++k) a.plane[k][i] = v0[k];
            a.material[i] = (uint16_t)m0;
            if (a.depth) a.depth[i] = z0;
        }
        if (in1) {
            const int64_t i = PBR_BOUNDS_PIXEL(oi + 1, a.width, band_h, a.stride, 1, kBoundsOutput);
#pragma unroll
            for (int k = 0; k < 14; ++k) a.plane[k][i] = v1[k];
            a.material[i] = (uint16_t)m1;
            if (a.depth) a.depth[i] = z1;
        }
    }
    if (m.owner != nullptr) {
        const int64_t wi = (int64_t)yb * m.owner_stride + x;
        if (in0) m.owner[PBR_BOUNDS_PIXEL(wi, a.width, band_h, m.owner_stride, 1, kBoundsOutput)] = (uint8_t)o0;
        if (in1) m.owner[PBR_BOUNDS_PIXEL(wi + 1, a.width, band_h, m.owner_stride, 1, kBoundsOutput)] = (uint8_t)o1;
    }
}

hipError_t launch_msaa_setup(const MsaaArgs& m, hipStream_t stream) {
    if (m.r.n_tris == 0u) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)m.r.n_tris + 255u) / 256u));
    hipLaunchKernelGGL(raster_setup_msaa_kernel, grid, dim3(256), 0, stream, m);
    return hipGetLastError();
}

hipError_t launch_msaa_large(const MsaaArgs& m, hipStream_t stream) {
    if (m.r.n_tris == 0u) return hipSuccess;
    const uint32_t gx = m.r.n_tris < (uint32_t)raster::kLargeGridX ? m.r.n_tris : (uint32_t)raster::kLargeGridX;
    hipLaunchKernelGGL(raster_large_msaa_kernel, dim3(gx, raster::kLargeSlabs), dim3(256), 0, stream, m);
    return hipGetLastError();
}

hipError_t launch_msaa_fragments(const MsaaArgs& m, hipStream_t stream) {
    const int band_h = m.r.row_end - m.r.row_begin;
    if (m.r.width <= 0 || band_h <= 0) return hipSuccess;
    const dim3 grid((m.r.width + 63) / 64, (band_h + 7) / 8);
    raster::with_bool(m.r.vec, [&](auto vec) {
        hipLaunchKernelGGL((raster_fragments_msaa_kernel<decltype(vec)::value>), grid, dim3(256), 0, stream, m);
    });
    return hipGetLastError();
}

}  // namespace pbr
