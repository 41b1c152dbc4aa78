// pbr_context_impl.h -- the context behind the C ABI, shared by its two host units: pbr_context.hip (lifetime, passes,
// textures, shading, statistics) and pbr_frontend.hip (materials, meshes, resolve, rasteriser). Internal: nothing here
// is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "pbr/pbr_shade.h"
#include "shade_kernels.h"
#include "frontend_kernels.h"

#pragma GCC visibility push(hidden)

// What the context keeps per caller stream (the cross-stream ordering protocol is written out in pbr_context.hip).
struct StreamState {
    hipStream_t stream = nullptr;
    hipEvent_t last_pass = nullptr;  // multi-stream contexts: recorded after every launch on `stream`
    // Statistics of the last pass on this stream: one record of pbr::kStatsPerBlock int32 per statistics slot
    // (one per wave in the pair layout, per workgroup in the one-pixel layout; pbr::StatField), summed on the
    // host by pbr_last_pass_stats / pbr_last_cull_stats. Written only by this stream's passes, so a pass never
    // overwrites the record of a pass on another stream.
    int32_t* d_stats = nullptr;
    int64_t stats_capacity = 0;  // slots
    int64_t tiles = 0, slots = 0;
    bool culled = false;
    std::string kernel;  // the last pass's kernel (pbr_last_pass_kernel)
    // pbr_rasterize on this stream (raster.h): its device scratch -- counters, the draw table, the transformed vertex
    // records, the large-triangle list, the visibility words -- grown in stream order on this stream, and the pinned
    // staging of the draw table with the event of its last upload. A stream has its own, so rasterisations queued on
    // two streams never share scratch.
    struct Raster {
        char* d = nullptr;
        size_t capacity = 0;
        char* h = nullptr;  // pinned
        size_t h_capacity = 0;
        hipEvent_t staged = nullptr;
        bool staged_pending = false;
        unsigned long long* d_counters = nullptr;  // inside d
        int64_t triangles = 0;
        bool ran = false;
    };
    Raster raster;
};

// The ordering record of one device resource and the (at most two) device buffers it owns. It can only be built into
// its context's list, which forget_readers and pbr_context_destroy walk: a new resource needs no edit of either.
struct Resource {
    std::vector<int> readers;  // StreamState indices that launched a pass reading it since the last write
    int writer = -1;           // StreamState index of the stream that wrote it last (-1: none / host-complete)
    hipEvent_t written = nullptr;  // recorded on the writer's stream after the write
    void** mem[2];             // the owner's device pointers (stream-ordered pool); [1] may be null
    template <class A, class B = void>
    Resource(std::vector<Resource*>& list, A** a, B** b = nullptr)
        : mem{reinterpret_cast<void**>(a), reinterpret_cast<void**>(b)} {
        list.push_back(this);
    }
    Resource(const Resource&) = delete;
};

struct pbr_context {
    int device = 0;
    std::vector<StreamState> streams;
    std::vector<Resource*> resources;  // every Resource below, in declaration order
    // Lights: a ring of device slots (3 float4 per light), each fed from its own pinned staging copy so a host
    // pass struct can be reused as soon as pbr_set_pass returns. Every pbr_set_pass takes the next slot; a
    // launch reads the slot of the pass it was queued with, so setting frame k+1's pass (on any stream) never
    // overwrites the lights a queued frame k reads.
    static constexpr int kSlots = 4;
    struct LightSlot {
        float4* d = nullptr;
        int capacity = 0;
        pbr_light* h = nullptr;        // pinned staging, PBR_MAX_LIGHTS records
        hipEvent_t copied = nullptr;   // the staging -> device copy
        bool copy_pending = false;
        Resource use;
        explicit LightSlot(std::vector<Resource*>& l) : use(l, &d) {}
    };
    LightSlot slots[kSlots]{LightSlot(resources), LightSlot(resources), LightSlot(resources), LightSlot(resources)};
    int cur_slot = -1;
    int next_slot = 0;
    // Textures: the environment (IBL, g_SkyArray[1]) and the sky (g_SkyArray[0]), each kept as fp32
    // RGBA on the device (decoded once from R16G16B16A16_UNORM, or uploaded as fp32).
    struct Texture {
        uint16_t* d_u16 = nullptr;  // UNORM16 upload staging
        float4* d = nullptr;
        int w = 0, h = 0, capacity = 0;
        bool faithful_ok = true;  // every texel in [0, kFaithfulAmbientHi], none NaN (PBR_FLAG_FAITHFUL precondition for the IBL)
        Resource use;
        explicit Texture(std::vector<Resource*>& l) : use(l, &d_u16, &d) {}
    };
    Texture env{resources}, sky{resources};
    // The material table and its textures (pbr_set_materials; read by pbr_resolve_materials and by a
    // pbr_rasterize_flags with PBR_RASTER_ALPHA_TEST): the records and one RGBA8 texel buffer holding every texture,
    // replaced as a whole; the records' flags stay on the host as well, where the rasteriser looks whether a call
    // draws a tested material at all.
    struct Materials {
        pbr::MaterialRec* d_table = nullptr;
        uint32_t* d_texels = nullptr;
        int n = 0;
        int64_t n_texels = 0;
        std::vector<uint32_t> flags;  // n
        // What pbr_generate_mips builds the chains from: where each texture of the upload is, and the texture of each
        // material's six slots (6 n; -1: unused).
        std::vector<pbr::MaterialTex> place;
        std::vector<int32_t> slot_tex;
        bool set = false;
        Resource use;
        explicit Materials(std::vector<Resource*>& l) : use(l, &d_table, &d_texels) {}
    };
    Materials mats{resources};
    // The mip chains of the material table's textures (pbr_generate_mips; read by pbr_resolve_materials_mip), a resource
    // of their own: one block holding the materials' MipSlot table and, behind it, the level table (then the launch
    // tables of the generation), and the texel buffer of the levels >= 1. They belong to the table they were built
    // from: pbr_set_materials clears `set`.
    struct Mips {
        char* d_tables = nullptr;
        uint32_t* d_texels = nullptr;
        const pbr::MipSlot* d_slots = nullptr;      // inside d_tables
        const pbr::MaterialTex* d_levels = nullptr;  // inside d_tables
        int64_t n_levels = 0, n_texels = 0;
        bool set = false;
        Resource use;
        explicit Mips(std::vector<Resource*>& l) : use(l, &d_tables, &d_texels) {}
    };
    Mips mips{resources};
    // The meshes pbr_rasterize draws from (pbr_set_meshes): every mesh's vertices in one buffer, every index in
    // another, replaced as a whole; the placement of each mesh stays on the host.
    struct MeshPlace {
        uint32_t vtx_base, n_vertices, idx_base, n_indices;
    };
    struct Meshes {
        float* d_vertices = nullptr;
        uint32_t* d_indices = nullptr;
        int64_t n_vertices = 0, n_indices = 0;
        std::vector<MeshPlace> place;
        bool set = false;
        Resource use;
        explicit Meshes(std::vector<Resource*>& l) : use(l, &d_vertices, &d_indices) {}
    };
    Meshes meshes{resources};
    // Current pass.
    pbr::PassArgs pass{};
    int ambient_mode = 0;
    uint32_t flags = 0;
    bool pass_set = false;
    bool faithful_pass_ok = false;  // light strengths and the constant ambient inside PBR_FLAG_FAITHFUL's windows (pbr_set_pass)
    bool faithful_count_terms = false;  // > 64 lights (culled pass): the kernel counts summed terms per wave
    int last_stream = -1;  // StreamState index of the context's last pass (pbr_last_pass_stats fallback)
    // Wave-balanced point-light lists (pbr_balanced.h) for untiled passes with at least this many point lights
    // and no spot lights; -1: the measured crossover of the mode (kBalancedMinFaithful / kBalancedMinExact);
    // PBR_BALANCED_MIN overrides both (0 disables).
    int balanced_min = -1;
    bool rank_per_wave = false;  // PBR_RANK_PER_WAVE: the balanced kernels rank per wave in every workgroup (development)
    bool points_flag_ok = false;  // pbr_set_pass: every point light inside the fast-path window
    bool points_quarter_ok = false;  // ... and every point strength inside the quarter gate (the exact balanced items' 4x radiance)
    int pixels_per_thread = 2;  // kernel layout: packed pixel pairs (measured faster); PBR_PIXELS_PER_THREAD=1 overrides
    bool lean = true;  // uniform-loop passes without a sky pass use the lean pair kernel (PBR_LEAN=0: off)
    std::string last_error;
    std::mutex mu;
};

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Defined in pbr_context.hip, where each one's contract is written.
int fail_hip(pbr_context* ctx, hipError_t e, const char* what, int status = PBR_ERR_HIP);
int stream_index(pbr_context* ctx, hipStream_t s, hipError_t& e);
hipError_t before_write(pbr_context* ctx, Resource& r, hipStream_t w, int wi);
hipError_t free_after_readers(pbr_context* ctx, Resource& r, void* p, hipStream_t w, int wi);
hipError_t after_write(Resource& r, hipStream_t w, int wi);
hipError_t before_read(Resource& r, hipStream_t s, int si);
int after_launch(pbr_context* ctx, int si, hipStream_t s, const char* what);
bool debug_bounds_skew();

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Every one of the n plane pointers is non-null and `min_align`-aligned; `vec` is cleared unless all are 8-byte aligned.
template <class T>
bool planes_ok(T* const* p, int n, uintptr_t min_align, bool& vec) {
    for (int i = 0; i < n; ++i) {
        if (!p[i] || !aligned(p[i], min_align)) return false;
        vec = vec && aligned(p[i], 8);
    }
    return true;
}

// What an entry point holds while it touches the context: the context's lock from construction; from open() on, the
// context's device as the current one, the caller's stream and its StreamState index. A call that validates or
// answers PBR_ERR_NOT_READY from context state does so between the two, before it touches the device.
struct Entry {
    pbr_context* ctx;
    std::lock_guard<std::mutex> lk;
    std::optional<DeviceGuard> g;
    hipStream_t s = nullptr;
    int si = -1;
    explicit Entry(pbr_context* c) : ctx(c), lk(c->mu) {}
    // The device and the stream handle only: for calls that look a StreamState up and must not create one.
    int device(void* stream) {
        g.emplace(ctx->device);
        s = static_cast<hipStream_t>(stream);
        return g->ok ? PBR_OK : PBR_ERR_NO_DEVICE;
    }
    int open(void* stream, const char* what) {
        if (const int rc = device(stream)) return rc;
        hipError_t e = hipSuccess;
        si = stream_index(ctx, s, e);
        return si < 0 ? fail_hip(ctx, e, what) : PBR_OK;
    }
};

// Replace or rewrite the two device buffers of `r` on the entry's stream, synchronously with respect to the host
// sources. With `realloc`: the old pair is released after its readers, in stream order (free_after_readers), and a
// pair of bytes0 and bytes1 is allocated on the stream. Then `copies()` queues the caller's copies (PBR_OK, or its
// status), ordered after the queued passes of any stream that read the old contents; the stream is synchronised, so the
// host sources may be released on return and later passes on any stream see the new contents. `what` names the call in
// last_error, followed by the step that failed.
template <class Copies>
int replace_buffers(Entry& en, Resource& r, bool realloc, size_t bytes0, size_t bytes1, const std::string& what,
                    Copies copies) {
    hipError_t e = hipSuccess;
    if (realloc) {
        e = free_after_readers(en.ctx, r, *r.mem[0], en.s, en.si);
        if (e == hipSuccess && *r.mem[1]) e = hipFreeAsync(*r.mem[1], en.s);
        if (e != hipSuccess) return fail_hip(en.ctx, e, (what + " release").c_str());
        *r.mem[0] = *r.mem[1] = nullptr;
        e = hipMallocAsync(r.mem[0], bytes0, en.s);
        if (e == hipSuccess) e = hipMallocAsync(r.mem[1], bytes1, en.s);
        if (e != hipSuccess) return fail_hip(en.ctx, e, (what + " hipMalloc").c_str());
    }
    e = before_write(en.ctx, r, en.s, en.si);  // in place: no reader is left after a release
    if (e != hipSuccess) return fail_hip(en.ctx, e, (what + " order").c_str());
    if (const int rc = copies()) return rc;
    e = hipStreamSynchronize(en.s);
    if (e != hipSuccess) return fail_hip(en.ctx, e, (what + " copy").c_str());
    r.writer = -1;
    return PBR_OK;
}

#pragma GCC visibility pop
