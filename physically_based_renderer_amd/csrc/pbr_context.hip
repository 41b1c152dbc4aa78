// pbr_context.hip -- the C ABI of include/pbr/pbr_shade.h: context lifetime, pass/env upload and
// the shade entry point. Host code only; the kernels live in shade_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include <new>
#include <string>

#include "pbr/pbr_shade.h"
#include "shade_kernels.h"
#include "pbr_debug_bounds.h"
#include "pbr_build_info.h"

// The build records of the library's units (pbr_build_info.h). Weak: a profiling build compiles the balanced kernels
// into shade_kernels.hip's unit, so shade_kernels_bal's record is then absent (null) and not listed.
extern "C" {
extern const char pbr_unit_info_shade_kernels[] __attribute__((weak));
extern const char pbr_unit_info_shade_kernels_bal[] __attribute__((weak));
extern const char pbr_unit_info_gbuffer_fill[] __attribute__((weak));
__attribute__((used)) const char pbr_unit_info_pbr_context[] =
    PBR_UNIT_INFO("pbr_context", PBR_BI_SWITCH(PBR_DEBUG_BOUNDS));
}

namespace {

// ---- Strength and ambient gates of pbr_set_pass -------------------------------------------------------------------
// The rescaled and reordered forms of the light term are the reference's only while no intermediate is subnormal, or
// overflows, where the reference's own is not. The factor bounds used below are the project's (pbr_device_math.h,
// fast_window_ok; pbr_device_math_x2.h, brdf_x2): an in-range point light's attenuation 1 / max(d, 0.01)^2 lies in
// [1e-4, 1e4] = [2^-13.3, 2^13.3] (beyond the range it is exactly 0); in a lean wave the per-channel factor
// Y = kD albedo / PI + spec of a term has kD albedo 0 or >= 2^-68 and spec = NDF G F / (4 N.V N.L + 0.001) 0 or
// >= 2^-30 x 2^-45 / 2^2.01 (the NDF G window, the F bound, the denominator's maximum), so with albedo >= 0 and F0 <= 1 (kD albedo >= 0:
// no cancellation) Y is 0 or >= 2^-78, and Y <= 2^57.1; N.L / 4 is 0 or >= 2^-110.
//
// The exact wave-balanced items (brdf_x2's QUARTER form, pbr_balanced.h) stage 4 s and evaluate
// (Y (4 s att)) (N.L / 4) for the reference's (Y (s att)) N.L. The last product rounds the same real number either
// way once its operands are exact multiples of four of one another, so the two forms differ only where 4 s, s att or
// Y (s att) is not scaled exactly:
//  * Hi: |s| <= 2^50 keeps Y 4 s att below 2^57.1 x 2^52 x 2^13.3 < 2^126: no overflow the reference does not have;
//  * Lo: |s| >= 2^-34 keeps |s att| >= 2^-47.3 and |Y (s att)| >= 2^-78 x 2^-47.3 > 2^-126 wherever it is not 0: every
//    product is normal in the reference's order, so its 4x is exact. (Found at 2^-115 and below by
//    tests/test_gpu_strength_range.py: s att subnormal in the reference, normal in the 4x form.)
//    NOT covered (residues): the pixel window admits albedo and F0 components of either sign up to 1024.
//    A negative albedo channel, or F0 > 1 (albedo > 1 on a metal: kD < 0), gives kD albedo / PI the sign opposite to
//    spec, and Y may cancel down to one ulp of its operands, 2^-101. Covering that takes |s| >= 2^-11.7 (Y (s att) >=
//    2^-101 x 2^-25), which would take every pass with a strength below 5e-4 off the balanced kernel; the gate stays at
//    2^-34, and for such a pixel the bit-identity of strengths in [2^-34, 2^-11.7) is not proved.
// Passes outside the gate run the uniform exact loop.
constexpr float kQuarterStrengthLo = 0x1p-34f, kQuarterStrengthHi = 0x1p50f;

// PBR_FLAG_FAITHFUL forms X (s (att N.L / 4)) per term, skips back-faced items (pbr_balanced.h) and keeps a pixel
// whose sum is 0 or inside [2^-100, 2^100] (shade_kernels.hip, the sum window). Every strength component of every
// light kind must be 0 or inside [Lo, Hi]:
//  * Hi = 2^50: X s att <= 2^57.1 x 2^50 x 2^13.3 stays finite, so the reference's (X (s att)) N.L is not NaN for a
//    term with N.L = 0 (inf x 0), which the faithful loops evaluate as s x 0 = 0 or skip. (A strength of 3e38 half a
//    unit behind a pixel made the reference's pixel NaN and the faithful one finite.)
//  * Lo = 2^-25: s (att N.L / 4) >= 2^-25 x 2^-13.3 x 2^-110 > 2^-149 for every live term, so the product never
//    underflows to 0 and a pixel the reference lights cannot come out with a kept sum of exactly 0 (with a
//    subnormal strength and X in the hundreds it did). Where that product is subnormal, att N.L / 4 < 2^-101, so
//    N.L < 2^-85 and the specular factor is below 2^30.1 N.L: X <= 2^10.4 is the diffuse factor alone, the term's
//    absolute error is <= 2^10.4 x 2^-150, and 64 such terms move a kept sum (>= 2^-100) by less than 2^-33 of it.
//    What remains is a term within the mode's relative error of the rounding boundary 2^-150 itself.
//    The attenuation bound is the point lights' (a directional light's is 1). A SPOT light's att also carries the cone
//    pow(c, SpotPower), which can be arbitrarily small: there the product can still underflow, or lose bits where the
//    reference's s att is normal, whatever Lo is. The sum window redoes such a pixel unless the sum is kept (exactly 0, or
//    lifted past 2^-100 by a strength near Hi): NOT covered by this gate (residues; not measured).
constexpr float kFaithfulStrengthLo = 0x1p-25f, kFaithfulStrengthHi = 0x1p50f;

// The faithful finish's Reinhard is c x v_rcp_f32(c + 1) (shade_kernels.hip, reinhard_faithful), and gfx950's v_rcp_f32
// returns 0 where the reciprocal is subnormal (c + 1 >= 2^126: the output was 0 where the reference has ~1). The light
// sum is within 2^100 (the sum window) and an in-window albedo within 2^10, so a constant ambient colour within 2^100
// keeps c + 1 below 2^111. The IBL ambient is kD (irradiance albedo) with kD in [0, 1] in a faithful wave (F0 in [0, 1])
// and the irradiance a convex combination of texels, so the same bound on every texel of an fp32 environment map does
// the same (pbr_set_env_map tracks it beside the sign; UNORM16 texels are <= 1). (Out-of-window albedos already send
// their pixels to the exact finish. The AO plane of PBR_FLAG_APPLY_AO multiplies the ambient term per pixel and is not
// windowed: a value above 2^15 is outside this bound)
constexpr float kFaithfulAmbientHi = 0x1p100f;

inline bool zero_or_within(float x, float lo, float hi) {
    const float a = std::fabs(x);
    return a == 0.0f || (a >= lo && a <= hi);  // false for NaN
}

}  // namespace

// Cross-stream ordering of the context's device resources (the reference's 3-deep FrameResource ring,
// FrameResource.h:111-140, PBRApp.cpp:220-243, is the same idea on D3D12 fences). A resource -- a light slot,
// the env map, the sky map -- remembers which streams have queued a pass reading it since it was last written
// and which stream wrote it (with an event after the write):
//   * before it is overwritten on stream w, w waits (stream-side, no host synchronisation) for the last pass of
//     every other stream that read it -- each stream's `last_pass` event, recorded after its launches;
//     waiting for a later pass of that stream is merely early;
//   * a pass on stream s that reads it waits for the write's event once, unless s wrote it.
// A context used from one stream records nothing per launch (every reader is the writer's stream). The first
// launch on a second stream synchronises the device once, so the earlier single-stream passes are complete and
// need no event; from then on each launch records its stream's last_pass.
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

// After the stream's work is complete (a device synchronisation): give back what a StreamState owns.
static void release_stream_state(StreamState& st) {
    if (st.last_pass) (void)hipEventDestroy(st.last_pass);
    if (st.d_stats) (void)hipFree(st.d_stats);
    if (st.raster.staged) (void)hipEventDestroy(st.raster.staged);
    if (st.raster.h) (void)hipHostFree(st.raster.h);
    if (st.raster.d) (void)hipFreeAsync(st.raster.d, nullptr);
    st = StreamState{};
}

struct Resource {
    std::vector<int> readers;  // StreamState indices that launched a pass reading it since the last write
    int writer = -1;           // StreamState index of the stream that wrote it last (-1: none / host-complete)
    hipEvent_t written = nullptr;  // recorded on the writer's stream after the write
};

struct pbr_context {
    int device = 0;
    std::vector<StreamState> streams;
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
    };
    LightSlot slots[kSlots];
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
    };
    Texture env, sky;
    // The material table and its textures (pbr_set_materials; read by pbr_resolve_materials): the records and one
    // RGBA8 texel buffer holding every texture, replaced as a whole.
    struct Materials {
        pbr::MaterialRec* d_table = nullptr;
        uint32_t* d_texels = nullptr;
        int n = 0;
        int64_t n_texels = 0;
        bool set = false;
        Resource use;
    };
    Materials mats;
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
    };
    Meshes meshes;
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
    bool points_flag_ok = false;  // pbr_set_pass: every point light inside the fast-path window
    bool points_quarter_ok = false;  // ... and every point strength inside the quarter gate (the exact balanced items' 4x radiance)
    int pixels_per_thread = 2;  // kernel layout: packed pixel pairs (measured faster); PBR_PIXELS_PER_THREAD=1 overrides
    bool lean = true;  // uniform-loop passes without a sky pass use the lean pair kernel (PBR_LEAN=0: off)
    std::string last_error;
    std::mutex mu;
};

namespace {

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

int fail_hip(pbr_context* ctx, hipError_t e, const char* what, int status = PBR_ERR_HIP) {
    if (ctx) {
        ctx->last_error = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
    }
    return e == hipErrorOutOfMemory ? PBR_ERR_OUT_OF_MEMORY : status;
}

bool is_ambient_mode(int m) { return m == PBR_AMBIENT_CONSTANT || m == PBR_AMBIENT_IBL_DIFFUSE; }

void forget_readers(pbr_context* ctx);

// PBR_DEBUG_BOUNDS builds (pbr_debug_bounds.h): one bounds-flag buffer per device, allocated, cleared and published
// to the kernels by the first context created on it; product builds have none.
constexpr int kBoundsMaxDevices = 64;
constexpr size_t kBoundsBytes = sizeof(uint32_t) * 2 * pbr::kBoundsClasses;
std::mutex g_bounds_mu;
uint32_t* g_bounds_buf[kBoundsMaxDevices] = {};

hipError_t arm_bounds(int dev) {  // current device = dev
    if (!PBR_DEBUG_BOUNDS) return hipSuccess;
    if (dev < 0 || dev >= kBoundsMaxDevices) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_bounds_mu);
    if (g_bounds_buf[dev]) return hipSuccess;
    uint32_t* b = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b), kBoundsBytes);
    if (e == hipSuccess) e = hipMemset(b, 0, kBoundsBytes);
    if (e == hipSuccess) e = pbr::debug_bounds_publish(b);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        g_bounds_buf[dev] = b;
    else if (b)
        (void)hipFree(b);
    return e;
}

// PBR_DEBUG_BOUNDS_SKEW=1 (bounds-checked builds): the output extent the checks use is one column narrower than
// the frame, so every pass must report class 1 -- the negative control of tests/test_gpu_debug_bounds.py.
bool debug_bounds_skew() {
    static const bool skew = [] {
        const char* e = std::getenv("PBR_DEBUG_BOUNDS_SKEW");
        return PBR_DEBUG_BOUNDS && e != nullptr && std::atoi(e) != 0;
    }();
    return skew;
}

// Streams a context tracks at once. Contexts expect a small, long-lived set of streams (a FrameResource-style
// ring); a caller that keeps creating new ones pays one device synchronisation per new stream, and past this
// bound the table is pruned at that synchronisation, so it never grows without limit.
constexpr size_t kMaxStreams = 16;

// The StreamState of `s` (created on first use). Caller holds ctx->mu and the device guard. A new stream
// beside existing ones: the device is synchronised once, so every pass queued so far is complete and no
// resource has a pending reader (the single-stream passes recorded no event). A full table is pruned then to the
// context's last pass stream (whose statistics pbr_last_pass_stats falls back to): the others' records go, which
// is safe as nothing of theirs is in flight. A destroyed stream whose handle value a new stream reuses is taken for
// the old one; the contract (pbr_shade.h) asks callers to let a stream's passes finish before destroying it.
int stream_index(pbr_context* ctx, hipStream_t s, hipError_t& e) {
    for (size_t i = 0; i < ctx->streams.size(); ++i)
        if (ctx->streams[i].stream == s) return (int)i;
    if (!ctx->streams.empty()) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) return -1;
        forget_readers(ctx);
        if (ctx->streams.size() >= kMaxStreams) {
            std::vector<StreamState> keep;
            for (size_t i = 0; i < ctx->streams.size(); ++i) {
                StreamState& st = ctx->streams[i];
                if ((int)i == ctx->last_stream) {
                    keep.push_back(std::move(st));
                    continue;
                }
                release_stream_state(st);
            }
            ctx->last_stream = keep.empty() ? -1 : 0;
            ctx->streams = std::move(keep);
        }
    }
    StreamState st;
    st.stream = s;
    // device-scope release: only other streams of this device (and host waits before a free) observe it
    e = hipEventCreateWithFlags(&st.last_pass, hipEventDisableTiming | hipEventReleaseToDevice);
    if (e != hipSuccess) return -1;
    ctx->streams.push_back(st);
    return (int)ctx->streams.size() - 1;
}

// Order a write of `r` on stream `w` (index wi) after every pass of another stream that read it.
hipError_t before_write(pbr_context* ctx, Resource& r, hipStream_t w, int wi) {
    for (int i : r.readers) {
        if (i == wi) continue;  // same stream: already ordered
        const hipError_t e = hipStreamWaitEvent(w, ctx->streams[i].last_pass, 0);
        if (e != hipSuccess) return e;
    }
    r.readers.clear();
    return hipSuccess;
}

// Release the memory `p` of resource `r`, which is growing, in stream order on `w` (index wi): `w` waits (stream-side)
// for the last pass of every other stream that read `r` and for a write of `r` queued on another stream, then the
// memory goes back to the device's pool with hipFreeAsync. Nothing blocks the host or an unrelated stream, and the
// sequence is legal inside a graph capture of `w`. A context used from one stream has every reader on `w` itself (a
// second stream's first launch synchronises the device and clears the records, stream_index), so stream order alone
// covers them; a multi-stream context records each stream's `last_pass` after every launch. Those events outlive the
// caller's stream handles, so a reader stream destroyed after its passes finished (the contract, pbr_shade.h) is never
// touched. The resources are allocated with hipMallocAsync on the writing stream for the same reason.
hipError_t free_after_readers(pbr_context* ctx, Resource& r, void* p, hipStream_t w, int wi) {
    hipError_t e = before_write(ctx, r, w, wi);
    if (e == hipSuccess && r.writer >= 0 && r.writer != wi) e = hipStreamWaitEvent(w, r.written, 0);
    if (e == hipSuccess && p) e = hipFreeAsync(p, w);
    return e;
}

// Record the write of `r` on stream `w` (index wi).
hipError_t after_write(Resource& r, hipStream_t w, int wi) {
    if (!r.written) {
        const hipError_t e = hipEventCreateWithFlags(&r.written, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    r.writer = wi;
    return hipEventRecord(r.written, w);
}

// A pass on stream `s` (index si) is about to read `r`: order it after the write, once per stream.
hipError_t before_read(Resource& r, hipStream_t s, int si) {
    for (int i : r.readers)
        if (i == si) return hipSuccess;
    if (r.writer >= 0 && r.writer != si) {
        const hipError_t e = hipStreamWaitEvent(s, r.written, 0);
        if (e != hipSuccess) return e;
    }
    r.readers.push_back(si);
    return hipSuccess;
}

// After a device synchronisation: every queued read and write of the context's resources is complete.
void forget_readers(pbr_context* ctx) {
    for (pbr_context::LightSlot& sl : ctx->slots) {
        sl.use.readers.clear();
        sl.use.writer = -1;
    }
    for (pbr_context::Texture* t : {&ctx->env, &ctx->sky}) {
        t->use.readers.clear();
        t->use.writer = -1;
    }
    ctx->mats.use.readers.clear();
    ctx->mats.use.writer = -1;
    ctx->meshes.use.readers.clear();
    ctx->meshes.use.writer = -1;
}

}  // namespace

extern "C" {

int pbr_abi_version(void) { return PBR_ABI_VERSION; }

const char* pbr_build_info(void) {
    static const std::string info = [] {
        std::string r = "{\"abi\": " + std::to_string(PBR_ABI_VERSION) + ", \"units\": [";
        bool first = true;
        for (const char* u : {pbr_unit_info_pbr_context, pbr_unit_info_shade_kernels, pbr_unit_info_shade_kernels_bal,
                              pbr_unit_info_gbuffer_fill}) {
            if (u == nullptr) continue;
            r += first ? "" : ", ";
            r += u;
            first = false;
        }
        return r + "]}";
    }();
    return info.c_str();
}

const char* pbr_strerror(int status) {
    switch (status) {
        case PBR_OK: return "ok";
        case PBR_ERR_INVALID_ARGUMENT: return "invalid argument";
        case PBR_ERR_NO_DEVICE: return "no HIP device";
        case PBR_ERR_OUT_OF_MEMORY: return "out of device memory";
        case PBR_ERR_LAUNCH: return "kernel launch failed";
        case PBR_ERR_HIP: return "HIP runtime error";
        case PBR_ERR_NOT_READY: return "pass or environment map not set";
        case PBR_ERR_UNSUPPORTED: return "unsupported";
        default: return "unknown status";
    }
}

const char* pbr_last_error(const pbr_context* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int pbr_context_create(int device, pbr_context** out_ctx) {
    if (!out_ctx) return PBR_ERR_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return PBR_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return PBR_ERR_INVALID_ARGUMENT;
    pbr_context* ctx = new (std::nothrow) pbr_context();
    if (!ctx) return PBR_ERR_OUT_OF_MEMORY;
    ctx->device = device;
    if (const char* e = std::getenv("PBR_PIXELS_PER_THREAD")) ctx->pixels_per_thread = std::atoi(e) == 1 ? 1 : 2;
    if (const char* e = std::getenv("PBR_BALANCED_MIN")) ctx->balanced_min = std::atoi(e);
    if (const char* e = std::getenv("PBR_LEAN")) ctx->lean = std::atoi(e) != 0;
    DeviceGuard g(device);
    if (!g.ok) {
        delete ctx;
        return PBR_ERR_NO_DEVICE;
    }
    hipError_t e = arm_bounds(device);
    for (int i = 0; e == hipSuccess && i < pbr_context::kSlots; ++i) {
        e = hipHostMalloc(reinterpret_cast<void**>(&ctx->slots[i].h), sizeof(pbr_light) * PBR_MAX_LIGHTS,
                          hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->slots[i].copied, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        pbr_context_destroy(ctx);
        return e == hipErrorOutOfMemory ? PBR_ERR_OUT_OF_MEMORY : PBR_ERR_HIP;
    }
    *out_ctx = ctx;
    return PBR_OK;
}

int pbr_context_destroy(pbr_context* ctx) {
    if (!ctx) return PBR_ERR_INVALID_ARGUMENT;
    {
        DeviceGuard g(ctx->device);
        (void)hipDeviceSynchronize();
        // Light slots and textures come from the stream-ordered pool (hipMallocAsync): returned the same way, after
        // the synchronisation above, and the pool's frees completed by the one below.
        for (pbr_context::LightSlot& sl : ctx->slots) {
            if (sl.copied) (void)hipEventDestroy(sl.copied);
            if (sl.h) (void)hipHostFree(sl.h);
            if (sl.d) (void)hipFreeAsync(sl.d, nullptr);
            if (sl.use.written) (void)hipEventDestroy(sl.use.written);
        }
        for (pbr_context::Texture* t : {&ctx->env, &ctx->sky}) {
            if (t->d_u16) (void)hipFreeAsync(t->d_u16, nullptr);
            if (t->d) (void)hipFreeAsync(t->d, nullptr);
            if (t->use.written) (void)hipEventDestroy(t->use.written);
        }
        if (ctx->mats.d_table) (void)hipFreeAsync(ctx->mats.d_table, nullptr);
        if (ctx->mats.d_texels) (void)hipFreeAsync(ctx->mats.d_texels, nullptr);
        if (ctx->mats.use.written) (void)hipEventDestroy(ctx->mats.use.written);
        if (ctx->meshes.d_vertices) (void)hipFreeAsync(ctx->meshes.d_vertices, nullptr);
        if (ctx->meshes.d_indices) (void)hipFreeAsync(ctx->meshes.d_indices, nullptr);
        if (ctx->meshes.use.written) (void)hipEventDestroy(ctx->meshes.use.written);
        for (StreamState& st : ctx->streams) release_stream_state(st);
        (void)hipDeviceSynchronize();
    }
    delete ctx;
    return PBR_OK;
}

int pbr_set_pass(pbr_context* ctx, const pbr_pass_desc* pass, void* stream) {
    if (!ctx || !pass) return PBR_ERR_INVALID_ARGUMENT;
    const int nd = pass->num_dir_lights, np = pass->num_point_lights, ns = pass->num_spot_lights;
    if (nd < 0 || np < 0 || ns < 0) return PBR_ERR_INVALID_ARGUMENT;
    const long long n = (long long)nd + np + ns;
    if (n > PBR_MAX_LIGHTS) return PBR_ERR_INVALID_ARGUMENT;
    if (n > 0 && !pass->lights) return PBR_ERR_INVALID_ARGUMENT;
    if (!is_ambient_mode(pass->ambient_mode)) return PBR_ERR_INVALID_ARGUMENT;
    const uint32_t known =
        PBR_FLAG_F0_PLANE | PBR_FLAG_APPLY_AO | PBR_FLAG_TILED_CULLING | PBR_FLAG_EXACT_ONLY | PBR_FLAG_FAITHFUL |
        PBR_FLAG_ALPHA_TEST;
    if (pass->flags & ~known) return PBR_ERR_INVALID_ARGUMENT;

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "pbr_set_pass stream");
    // The next slot of the ring: its staging copy must have left the host buffer, and its device copy is
    // overwritten only after the queued passes that read it (stream-side waits, before_write).
    const int slot = ctx->next_slot;
    pbr_context::LightSlot& sl = ctx->slots[slot];
    if (sl.copy_pending) {
        e = hipEventSynchronize(sl.copied);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass staging wait");
        sl.copy_pending = false;
    }
    if (n > sl.capacity) {
        // Growing: the old buffer may still be read by queued passes (released after them, in stream order).
        if (sl.d) {
            e = free_after_readers(ctx, sl.use, sl.d, s, si);
            if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass slot release");
            sl.d = nullptr;
            sl.capacity = 0;
        }
        int cap = 64;
        while (cap < n) cap *= 2;
        e = hipMallocAsync(reinterpret_cast<void**>(&sl.d), sizeof(pbr_light) * (size_t)cap, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass hipMalloc");
        sl.capacity = cap;
    }
    bool points_ok = true;  // every point light's fast-path flag is set (the balanced pass needs it)
    bool quarter_ok = true;  // ... and every point strength is inside the quarter gate (kQuarterStrengthLo / Hi)
    if (n > 0) {
        std::memcpy(sl.h, pass->lights, sizeof(pbr_light) * (size_t)n);
        // The kernel's per-light fast-path flag travels in the unused pad1 of the uploaded copy
        // (the caller's array is not touched): directional L = -Direction components, point / spot
        // positions, each 0 or |x| in [2^-20, 16] / [2^-20, 2^20] (pbr_device_math.h, light_window_ok),
        // and a finite point / spot strength.
        for (long long i = 0; i < n; ++i) {
            pbr_light& L = sl.h[i];
            const bool directional = i < nd;
            const float* c = directional ? L.direction : L.position;
            const float hi = directional ? 16.0f : 0x1p20f;
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                const float a = std::fabs(c[k]);
                ok = ok && (a == 0.0f || (a >= 0x1p-20f && a <= hi));
                // point / spot: a finite strength, so that an out-of-range lane's zero-attenuated
                // contribution is +-0 (pbr_device_math_x2.h, point_or_spot_x2)
                if (!directional) ok = ok && std::isfinite(L.strength[k]);
            }
            L.pad1 = ok ? 1.0f : 0.0f;
            if (i >= nd && i < nd + np) {
                points_ok = points_ok && ok;
                for (int k = 0; k < 3; ++k)
                    quarter_ok = quarter_ok && zero_or_within(L.strength[k], kQuarterStrengthLo, kQuarterStrengthHi);
            }
        }
        e = before_write(ctx, sl.use, s, si);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass order");
        e = hipMemcpyAsync(sl.d, sl.h, sizeof(pbr_light) * (size_t)n, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass copy");
        e = hipEventRecord(sl.copied, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass record");
        sl.copy_pending = true;
        e = after_write(sl.use, s, si);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_pass record");
    }
    ctx->cur_slot = slot;
    ctx->next_slot = (slot + 1) % pbr_context::kSlots;
    pbr::PassArgs& p = ctx->pass;
    for (int i = 0; i < 3; ++i) {
        p.eye[i] = pass->eye_pos_w[i];
        p.ambient[i] = pass->ambient_light[i];
        p.fresnel_r0[i] = pass->fresnel_r0[i];
    }
    p.opacity = pass->opacity;
    p.eye_ok = 1;
    for (int i = 0; i < 3; ++i) {  // the fast-path window of the (uniform) eye: 0 or |x| in [2^-20, 2^20]
        const float a = std::fabs(pass->eye_pos_w[i]);
        if (!(a == 0.0f || (a >= 0x1p-20f && a <= 0x1p20f))) p.eye_ok = 0;
    }
    p.n_dir = nd;
    p.n_point = np;
    p.n_spot = ns;
    // PBR_FLAG_FAITHFUL's error bound needs every term of the light sum >= 0
    // (pbr_device_math_x2.h, brdf_faithful_x2): non-negative strengths inside the strength window
    // (kFaithfulStrengthLo / Hi: NaN and infinities fail it) and a constant ambient in [0, kFaithfulAmbientHi];
    // and at most 64 summed terms, since the sum's rounding drift grows by <= 1 ulp per term --
    // with tiled culling the kernel counts each wave's surviving lights (faithful mode 2).
    ctx->faithful_count_terms = n > 64;
    bool faithful_ok = n <= 64 || (pass->flags & PBR_FLAG_TILED_CULLING) != 0;
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const float st = pass->lights[i].strength[k];
            faithful_ok = faithful_ok && (st == 0.0f || (st >= kFaithfulStrengthLo && st <= kFaithfulStrengthHi));
        }
    if (pass->ambient_mode == PBR_AMBIENT_CONSTANT)
        for (int k = 0; k < 3; ++k)
            faithful_ok = faithful_ok && pass->ambient_light[k] >= 0.0f && pass->ambient_light[k] <= kFaithfulAmbientHi;
    ctx->faithful_pass_ok = faithful_ok;
    ctx->points_flag_ok = points_ok;
    ctx->points_quarter_ok = points_ok && quarter_ok;
    ctx->ambient_mode = pass->ambient_mode;
    ctx->flags = pass->flags;
    ctx->pass_set = true;
    return PBR_OK;
}

}  // extern "C"

namespace {

// Upload a width x height RGBA texture (UNORM16 -> decoded on the device, or fp32 as given) into slot
// `t`. Synchronous with respect to the host buffer: it may be released on return.
int set_texture(pbr_context* ctx, pbr_context::Texture& t, const void* texels, bool unorm16, int32_t width,
                int32_t height, void* stream, const char* what) {
    if (!ctx || !texels || width <= 0 || height <= 0) return PBR_ERR_INVALID_ARGUMENT;
    if ((long long)width * height > (1ll << 26)) return PBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n = width * height;
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, what);
    if (n > t.capacity) {
        // Growing: the old texture may still be read by queued passes (released after them, in stream order).
        e = free_after_readers(ctx, t.use, t.d_u16, s, si);
        if (e == hipSuccess && t.d) e = hipFreeAsync(t.d, s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
        t.d_u16 = nullptr;
        t.d = nullptr;
        t.capacity = 0;
        e = hipMallocAsync(reinterpret_cast<void**>(&t.d_u16), sizeof(uint16_t) * 4 * (size_t)n, s);
        if (e == hipSuccess) e = hipMallocAsync(reinterpret_cast<void**>(&t.d), sizeof(float4) * (size_t)n, s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
        t.capacity = n;
    }
    // Replaced in place: after the queued passes (of any stream) that read the old texels.
    e = before_write(ctx, t.use, s, si);
    if (e != hipSuccess) return fail_hip(ctx, e, what);
    if (unorm16) {
        e = hipMemcpyAsync(t.d_u16, texels, sizeof(uint16_t) * 4 * (size_t)n, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
        e = pbr::launch_decode_unorm16(t.d_u16, t.d, n, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "decode_unorm16_kernel", PBR_ERR_LAUNCH);
    } else {
        e = hipMemcpyAsync(t.d, texels, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
    }
    e = hipStreamSynchronize(s);  // the (pageable) host texels may be released on return
    if (e != hipSuccess) return fail_hip(ctx, e, what);
    t.use.writer = -1;  // complete: later passes on any stream see the new texels
    t.w = width;
    t.h = height;
    t.faithful_ok = true;  // UNORM16 texels are in [0, 1]
    if (!unorm16) {
        const float* f = static_cast<const float*>(texels);
        for (size_t i = 0; i < 4 * (size_t)n && t.faithful_ok; ++i)
            t.faithful_ok = f[i] >= 0.0f && f[i] <= kFaithfulAmbientHi;  // false for NaN
    }
    return PBR_OK;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int shade(pbr_context* ctx, const pbr_gbuffer_soa* gb, const pbr_frame_desc* fr, void* stream) {
    if (!ctx || !gb || !fr) return PBR_ERR_INVALID_ARGUMENT;
    if (gb->width < 0 || gb->height < 0 || gb->row_stride < gb->width || fr->out_row_stride < gb->width)
        return PBR_ERR_INVALID_ARGUMENT;
    if (fr->format != PBR_OUTPUT_RGBA32F && fr->format != PBR_OUTPUT_RGBA8_UNORM) return PBR_ERR_INVALID_ARGUMENT;
    if (fr->coverage && fr->coverage_row_stride < gb->width) return PBR_ERR_INVALID_ARGUMENT;
    // Everything below reads context state that pbr_set_pass / pbr_set_*_map write under the same
    // mutex: the launch arguments are built (and the kernel queued) in one critical section, so a
    // concurrent set_pass can never tear them.
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->pass_set) return PBR_ERR_NOT_READY;
    if (gb->width == 0 || gb->height == 0) return PBR_OK;  // empty frame: nothing is read or written
    if (!fr->out) return PBR_ERR_INVALID_ARGUMENT;
    if (!aligned(fr->out, fr->format == PBR_OUTPUT_RGBA8_UNORM ? 4 : 16)) return PBR_ERR_INVALID_ARGUMENT;
    const bool f0_plane = (ctx->flags & PBR_FLAG_F0_PLANE) != 0;
    const bool apply_ao = (ctx->flags & PBR_FLAG_APPLY_AO) != 0;
    const bool cull = (ctx->flags & PBR_FLAG_TILED_CULLING) != 0;
    for (int i = 0; i < 3; ++i)
        if (!gb->pos_w[i] || !gb->normal_w[i] || !gb->albedo[i]) return PBR_ERR_INVALID_ARGUMENT;
    if (!gb->metallic || !gb->roughness) return PBR_ERR_INVALID_ARGUMENT;
    if (apply_ao && !gb->ao) return PBR_ERR_INVALID_ARGUMENT;
    if (f0_plane && (!gb->f0[0] || !gb->f0[1] || !gb->f0[2])) return PBR_ERR_INVALID_ARGUMENT;
    const bool alpha_test = (ctx->flags & PBR_FLAG_ALPHA_TEST) != 0;
    if (alpha_test && !gb->opacity) return PBR_ERR_INVALID_ARGUMENT;
    if (ctx->ambient_mode == PBR_AMBIENT_IBL_DIFFUSE && !ctx->env.d) return PBR_ERR_NOT_READY;
    if (fr->coverage && !ctx->sky.d) return PBR_ERR_NOT_READY;  // background pixels need the sky map

    pbr::LaunchArgs a{};
    const float* planes[15] = {gb->pos_w[0], gb->pos_w[1], gb->pos_w[2], gb->normal_w[0], gb->normal_w[1],
                               gb->normal_w[2], gb->albedo[0], gb->albedo[1], gb->albedo[2], gb->metallic,
                               gb->roughness, gb->ao, gb->f0[0], gb->f0[1], gb->f0[2]};
    for (int i = 0; i < 15; ++i) a.gb.plane[i] = planes[i] ? planes[i] : planes[0];
    a.gb.plane[15] = alpha_test ? gb->opacity : planes[0];
    a.gb.alpha_test = alpha_test;
    a.gb.width = gb->width;
    a.gb.height = gb->height;
    a.gb.row_stride = gb->row_stride;
    a.gb.pairs_aligned = (gb->row_stride % 2) == 0;
    for (int i = 0; i < 16; ++i)
        if (!aligned(a.gb.plane[i], 8)) a.gb.pairs_aligned = false;
    a.ps = ctx->pass;
    a.ps.env_w = ctx->env.w;
    a.ps.env_h = ctx->env.h;
    a.ps.sky_w = ctx->sky.w;
    a.ps.sky_h = ctx->sky.h;
    a.lights = ctx->cur_slot >= 0 ? ctx->slots[ctx->cur_slot].d : nullptr;
    a.env = ctx->env.d;
    a.frame.out = fr->out;
    a.frame.out_stride = fr->out_row_stride;
    a.frame.format = fr->format == PBR_OUTPUT_RGBA8_UNORM ? pbr::kOutRgba8 : pbr::kOutRgba32f;
    a.frame.coverage = fr->coverage;
    a.frame.coverage_stride = fr->coverage_row_stride;
    a.frame.sky = ctx->sky.d;
    a.frame.width = gb->width - (debug_bounds_skew() ? 1 : 0);
    a.frame.height = gb->height;
    a.ambient_mode = ctx->ambient_mode;
    a.f0_plane = f0_plane;
    a.apply_ao = apply_ao;
    a.cull = cull;
    a.exact_only = (ctx->flags & PBR_FLAG_EXACT_ONLY) != 0;
    a.ps.faithful = (ctx->flags & PBR_FLAG_FAITHFUL) && !a.exact_only && ctx->faithful_pass_ok &&
                    (ctx->ambient_mode != PBR_AMBIENT_IBL_DIFFUSE || ctx->env.faithful_ok);
    if (a.ps.faithful && ctx->faithful_count_terms) a.ps.faithful = 2;
    a.pixels_per_thread = ctx->pixels_per_thread;
    // Wave-balanced point-light lists: untiled pair-kernel passes with no spot lights, every point light inside
    // the fast-path window; faithful (1) or exact (2, and no directional lights either) -- the exact variant
    // keeps the reference's order per pixel (bit-identical), the faithful one re-associates.
    // Point-light count from which the balanced lists win (same-box sweeps, 1080p and 4K): the
    // faithful loop between 20 (uniform faster) and 24 lights, the exact loop between 16 and 20.
    constexpr int kBalancedMinFaithful = 22, kBalancedMinExact = 18;
    const int bal_min = ctx->balanced_min >= 0 ? ctx->balanced_min
                        : a.ps.faithful == 1   ? kBalancedMinFaithful
                                               : kBalancedMinExact;
    const bool bal_ok = !cull && a.pixels_per_thread == 2 && bal_min > 0 && ctx->points_flag_ok &&
                        a.ps.n_spot == 0 && a.ps.n_point >= bal_min && a.ps.n_point <= pbr::kBalMaxLights;
    a.ps.balanced = !bal_ok                                                ? 0
                    : a.ps.faithful == 1                                   ? 1
                    : a.ps.faithful == 0 && !a.exact_only && a.ps.n_dir == 0 && ctx->points_quarter_ok ? 2
                                                                           : 0;

    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "shade stream");
    StreamState& st = ctx->streams[si];
    {
        const int64_t tiles = pbr::shade_tile_count(gb->width, gb->height, a.pixels_per_thread);
        const int64_t slots = tiles * pbr::shade_stat_slots_per_tile(a.pixels_per_thread);
        if (slots > st.stats_capacity) {
            // Growing: only this stream's passes write the buffer (stream order covers them).
            if (st.d_stats) {
                e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail_hip(ctx, e, "pass stats sync");
                (void)hipFree(st.d_stats);
                st.d_stats = nullptr;
                st.stats_capacity = 0;
            }
            e = hipMalloc(&st.d_stats, pbr::kStatsPerBlock * sizeof(int32_t) * (size_t)slots);
            if (e != hipSuccess) return fail_hip(ctx, e, "pass stats hipMalloc");
            st.stats_capacity = slots;
        }
        st.tiles = tiles;
        st.slots = slots;
        st.culled = cull;
        a.tile_kept = st.d_stats;
        // The lean pair kernel: uniform light loops (no balanced lists), no sky pass, the fast paths enabled.
        a.lean = ctx->lean && a.pixels_per_thread == 2 && a.ps.balanced == 0 && !fr->coverage && !a.exact_only;
    }
    // Order the pass after the writes of what it reads (lights, textures) made on other streams.
    const bool reads_lights = ctx->cur_slot >= 0 && a.ps.n_dir + a.ps.n_point + a.ps.n_spot > 0;
    if (reads_lights) e = before_read(ctx->slots[ctx->cur_slot].use, s, si);
    if (e == hipSuccess && ctx->ambient_mode == PBR_AMBIENT_IBL_DIFFUSE) e = before_read(ctx->env.use, s, si);
    if (e == hipSuccess && fr->coverage) e = before_read(ctx->sky.use, s, si);
    if (e != hipSuccess) return fail_hip(ctx, e, "shade order");
    e = pbr::launch_shade(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "shade_tile_kernel launch", PBR_ERR_LAUNCH);
    st.kernel = pbr::launched_kernel(a);
    if (ctx->streams.size() > 1) {
        e = hipEventRecord(st.last_pass, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "shade record");
    }
    ctx->last_stream = si;
    return PBR_OK;
}

}  // namespace

extern "C" {

int pbr_set_env_map(pbr_context* ctx, const uint16_t* texels, int32_t width, int32_t height, void* stream) {
    return ctx ? set_texture(ctx, ctx->env, texels, true, width, height, stream, "pbr_set_env_map")
               : PBR_ERR_INVALID_ARGUMENT;
}

int pbr_set_env_map_f32(pbr_context* ctx, const float* texels, int32_t width, int32_t height, void* stream) {
    return ctx ? set_texture(ctx, ctx->env, texels, false, width, height, stream, "pbr_set_env_map_f32")
               : PBR_ERR_INVALID_ARGUMENT;
}

int pbr_set_sky_map(pbr_context* ctx, const uint16_t* texels, int32_t width, int32_t height, void* stream) {
    return ctx ? set_texture(ctx, ctx->sky, texels, true, width, height, stream, "pbr_set_sky_map")
               : PBR_ERR_INVALID_ARGUMENT;
}

int pbr_set_sky_map_f32(pbr_context* ctx, const float* texels, int32_t width, int32_t height, void* stream) {
    return ctx ? set_texture(ctx, ctx->sky, texels, false, width, height, stream, "pbr_set_sky_map_f32")
               : PBR_ERR_INVALID_ARGUMENT;
}

int pbr_shade_gbuffer(pbr_context* ctx, const pbr_gbuffer_soa* gb, float* out_rgba, int64_t out_row_stride,
                      void* stream) {
    pbr_frame_desc fr{};
    fr.out = out_rgba;
    fr.out_row_stride = out_row_stride;
    fr.format = PBR_OUTPUT_RGBA32F;
    return shade(ctx, gb, &fr, stream);
}

int pbr_shade_frame(pbr_context* ctx, const pbr_gbuffer_soa* gb, const pbr_frame_desc* frame, void* stream) {
    return shade(ctx, gb, frame, stream);
}

}  // extern "C"

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

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "pbr_set_materials stream");
    pbr_context::Materials& mt = ctx->mats;
    // The old table and texels may still be read by queued resolves: released after them, in stream order.
    e = free_after_readers(ctx, mt.use, mt.d_table, s, si);
    if (e == hipSuccess && mt.d_texels) e = hipFreeAsync(mt.d_texels, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_materials release");
    mt.d_table = nullptr;
    mt.d_texels = nullptr;
    mt.set = false;
    e = hipMallocAsync(reinterpret_cast<void**>(&mt.d_table), sizeof(pbr::MaterialRec) * recs.size(), s);
    if (e == hipSuccess) e = hipMallocAsync(reinterpret_cast<void**>(&mt.d_texels), sizeof(uint32_t) * texels.size(), s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_materials hipMalloc");
    e = hipMemcpyAsync(mt.d_table, recs.data(), sizeof(pbr::MaterialRec) * recs.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(mt.d_texels, texels.data(), sizeof(uint32_t) * texels.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the staging copies above are released on return
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_materials copy");
    mt.use.writer = -1;  // complete: later resolves on any stream see the new table
    mt.n = n_materials;
    mt.n_texels = (int64_t)texels.size();
    mt.set = true;
    return PBR_OK;
}

int pbr_resolve_materials(pbr_context* ctx, const pbr_attributes_soa* at, const pbr_gbuffer_targets* tg, int32_t filter,
                          void* stream) {
    if (!ctx || !at || !tg) return PBR_ERR_INVALID_ARGUMENT;
    if (at->width < 0 || at->height < 0 || at->row_stride < at->width || tg->row_stride < at->width)
        return PBR_ERR_INVALID_ARGUMENT;
    if (filter != PBR_FILTER_POINT && filter != PBR_FILTER_LINEAR) return PBR_ERR_INVALID_ARGUMENT;
    if (tg->coverage && tg->coverage_row_stride < at->width) return PBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->mats.set) return PBR_ERR_NOT_READY;
    if (at->width == 0 || at->height == 0) return PBR_OK;  // empty frame: nothing is read or written
    pbr::ResolveArgs a{};
    const float* in[14] = {at->pos_w[0],     at->pos_w[1],     at->pos_w[2],       at->normal_w[0],    at->normal_w[1],
                           at->normal_w[2],  at->tangent_w[0], at->tangent_w[1],   at->tangent_w[2],   at->bitangent_w[0],
                           at->bitangent_w[1], at->bitangent_w[2], at->tex_coord[0], at->tex_coord[1]};
    a.vec = (at->row_stride % 2) == 0 && (tg->row_stride % 2) == 0;
    for (int i = 0; i < 14; ++i) {
        if (!in[i] || !aligned(in[i], 4)) return PBR_ERR_INVALID_ARGUMENT;
        a.attr[i] = in[i];
        a.vec = a.vec && aligned(in[i], 8);
    }
    if (!at->material || !aligned(at->material, 2)) return PBR_ERR_INVALID_ARGUMENT;
    a.material = at->material;
    a.vec = a.vec && aligned(at->material, 4);
    for (int i = 0; i < 15; ++i) {
        if (!tg->planes[i] || !aligned(tg->planes[i], 4)) return PBR_ERR_INVALID_ARGUMENT;
        a.plane[i] = tg->planes[i];
        a.vec = a.vec && aligned(tg->planes[i], 8);
    }
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
    a.n_texels = ctx->mats.n_texels;
    a.linear = filter == PBR_FILTER_LINEAR;

    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "pbr_resolve_materials stream");
    e = before_read(ctx->mats.use, s, si);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_resolve_materials order");
    e = pbr::launch_resolve_materials(a, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "resolve_materials_kernel launch", PBR_ERR_LAUNCH);
    // Not a shading pass: the stream's statistics record, its kernel name and the context's last pass stay as they
    // are; only the event that orders a later pbr_set_materials after this read is recorded.
    if (ctx->streams.size() > 1) {
        e = hipEventRecord(ctx->streams[si].last_pass, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_resolve_materials record");
    }
    return PBR_OK;
}

}  // extern "C"

// ---- Rasteriser (VS + the fixed-function rasteriser on the device; raster.h) --------------------------

namespace {

constexpr int32_t kRasterMaxSide = 32768;  // frame width and height: keeps every block and pixel count inside 32 bits

size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

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

    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "pbr_set_meshes stream");
    pbr_context::Meshes& ms = ctx->meshes;
    // The old buffers may still be read by queued rasterisations: released after them, in stream order.
    e = free_after_readers(ctx, ms.use, ms.d_vertices, s, si);
    if (e == hipSuccess && ms.d_indices) e = hipFreeAsync(ms.d_indices, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_meshes release");
    ms.d_vertices = nullptr;
    ms.d_indices = nullptr;
    ms.set = false;
    e = hipMallocAsync(reinterpret_cast<void**>(&ms.d_vertices), sizeof(float) * vertices.size(), s);
    if (e == hipSuccess) e = hipMallocAsync(reinterpret_cast<void**>(&ms.d_indices), sizeof(uint32_t) * indices.size(), s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_meshes hipMalloc");
    e = hipMemcpyAsync(ms.d_vertices, vertices.data(), sizeof(float) * vertices.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ms.d_indices, indices.data(), sizeof(uint32_t) * indices.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the staging copies above are released on return
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_set_meshes copy");
    ms.use.writer = -1;  // complete: later rasterisations on any stream see the new set
    ms.n_vertices = nv;
    ms.n_indices = ni;
    ms.place = std::move(place);
    ms.set = true;
    return PBR_OK;
}

}  // extern "C"

namespace {

// pbr_rasterize. `marks` (development, pbr_debug_rasterize_timed): six events recorded around the five stages --
// clears and table upload, vertex transform, setup with the small triangles' coverage, large triangles, resolve.
int rasterize_impl(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                   const pbr_raster_targets* tg, void* stream, hipEvent_t* marks) {
    if (!ctx || !view || !tg || n_draws < 0 || (n_draws > 0 && !draws)) return PBR_ERR_INVALID_ARGUMENT;
    if (view->width < 0 || view->height < 0 || view->width > kRasterMaxSide || view->height > kRasterMaxSide)
        return PBR_ERR_INVALID_ARGUMENT;
    if (view->row_begin < 0 || view->row_begin > view->row_end || view->row_end > view->height)
        return PBR_ERR_INVALID_ARGUMENT;
    if (tg->row_stride < view->width) return PBR_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n_draws; ++i) {
        const pbr_draw& d = draws[i];
        if (d.mesh < 0 || d.first_index < 0 || d.index_count < 0 || d.index_count % 3 != 0 || d.cull > 1)
            return PBR_ERR_INVALID_ARGUMENT;
    }
    pbr::RasterArgs a{};
    a.vec = (tg->row_stride % 2) == 0;
    for (int i = 0; i < 14; ++i) {
        if (!tg->planes[i] || !aligned(tg->planes[i], 4)) return PBR_ERR_INVALID_ARGUMENT;
        a.plane[i] = tg->planes[i];
        a.vec = a.vec && aligned(tg->planes[i], 8);
    }
    if (!tg->material || !aligned(tg->material, 2)) return PBR_ERR_INVALID_ARGUMENT;
    if (tg->depth && !aligned(tg->depth, 4)) return PBR_ERR_INVALID_ARGUMENT;
    a.material = tg->material;
    a.depth = tg->depth;
    a.vec = a.vec && aligned(tg->material, 4) && aligned(tg->depth, 8);
    a.stride = tg->row_stride;
    a.width = view->width;
    a.height = view->height;
    a.row_begin = view->row_begin;
    a.row_end = view->row_end;
    std::memcpy(a.view_proj, view->view_proj, sizeof(a.view_proj));
    for (int c = 0; c < 3; ++c)
        a.eye[c] = view->eye[c], a.right[c] = view->bg_right[c], a.up[c] = view->bg_up[c], a.fwd[c] = view->bg_forward[c];

    std::lock_guard<std::mutex> lk(ctx->mu);
    const pbr_context::Meshes& ms = ctx->meshes;
    if (!ms.set) return PBR_ERR_NOT_READY;
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
    const int band_h = view->row_end - view->row_begin;
    if (view->width == 0 || band_h == 0) return PBR_OK;  // an empty band: nothing is read or written

    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const int si = stream_index(ctx, s, e);
    if (si < 0) return fail_hip(ctx, e, "pbr_rasterize stream");
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

    // Device scratch of this stream: counters | draw table | vertex records | large list | visibility words.
    const size_t off_table = 256;
    const size_t off_records = off_table + align_up(table_bytes, 256);
    const size_t off_large = off_records + align_up(sizeof(pbr::RasterVertex) * (size_t)n_records, 256);
    const size_t off_vis = off_large + align_up(sizeof(uint2) * (size_t)n_tris, 256);
    const size_t vis_bytes = sizeof(unsigned long long) * (size_t)band_h * (size_t)view->width;
    const size_t need = off_vis + vis_bytes;
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
    a.n_draws = n_draws;
    a.n_tris = (uint32_t)n_tris;
    a.n_records = (uint32_t)n_records;
    a.vertices = ms.d_vertices;
    a.indices = ms.d_indices;
    a.n_src_vertices = ms.n_vertices;
    a.n_src_indices = ms.n_indices;

    e = before_read(ctx->meshes.use, s, si);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize order");
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    (void)mark(0);
    e = hipMemsetAsync(rs.d, 0, sizeof(unsigned long long) * pbr::kRasterCounters, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rs.d + off_table, rs.h, table_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(rs.staged, s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize upload");
    rs.staged_pending = true;
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
    if (ctx->streams.size() > 1) {
        e = hipEventRecord(ctx->streams[si].last_pass, s);
        if (e != hipSuccess) return fail_hip(ctx, e, "pbr_rasterize record");
    }
    return PBR_OK;
}

}  // namespace

extern "C" {

int pbr_rasterize(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws, const pbr_raster_view* view,
                  const pbr_raster_targets* targets, void* stream) {
    return rasterize_impl(ctx, draws, n_draws, view, targets, stream, nullptr);
}

int pbr_last_raster_stats(pbr_context* ctx, pbr_raster_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    *out = pbr_raster_stats{};
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const StreamState* st = nullptr;
    for (const StreamState& c : ctx->streams)
        if (c.stream == s && c.raster.ran) st = &c;
    if (!st) return PBR_OK;
    unsigned long long h[pbr::kRasterCounters] = {};
    hipError_t e = hipMemcpyAsync(h, st->raster.d_counters, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_last_raster_stats");
    out->triangles = st->raster.triangles;
    out->backface_culled = (int64_t)h[pbr::kRasterCulled];
    out->zero_area = (int64_t)h[pbr::kRasterZeroArea];
    out->skipped_near = (int64_t)h[pbr::kRasterNear];
    out->skipped_guard_band = (int64_t)h[pbr::kRasterGuard];
    out->fragments = (int64_t)h[pbr::kRasterFragments];
    return PBR_OK;
}

}  // extern "C"

namespace {

// Sum the statistics records of the last pass on `stream` (or, if the context never launched on that stream,
// of its last pass on any stream: the caller's stream is then ordered after it by contract).
int sum_pass_stats(pbr_context* ctx, pbr_pass_stats* out, void* stream, const char* what) {
    *out = pbr_pass_stats{};
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int si = -1;
    for (size_t i = 0; i < ctx->streams.size(); ++i)
        if (ctx->streams[i].stream == s && ctx->streams[i].tiles > 0) si = (int)i;
    if (si < 0) si = ctx->last_stream;
    if (si < 0 || ctx->streams[si].tiles == 0) return PBR_OK;  // no pass yet (or an empty frame)
    const StreamState& st = ctx->streams[si];
    std::vector<int32_t> h(pbr::kStatsPerBlock * (size_t)st.slots);
    hipError_t e = hipMemcpyAsync(h.data(), st.d_stats, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(ctx, e, what);
    out->workgroups = st.tiles;
    out->culled = st.culled ? 1 : 0;
    for (size_t t = 0; t < h.size(); t += pbr::kStatsPerBlock) {
        out->cull_tile_lights += h[t + pbr::kStatCullKept];
        out->cull_tiles += h[t + pbr::kStatCullTiles];
        out->exact_pixels += h[t + pbr::kStatExactPixels];
        out->light_terms += h[t + pbr::kStatLightTerms];
        out->geometry_pixels += h[t + pbr::kStatGeometryPixels];
        out->backface_tests += h[t + pbr::kStatBackfaceTests];
    }
    return PBR_OK;
}

}  // namespace

extern "C" {

int pbr_last_cull_stats(pbr_context* ctx, int64_t* sum_tile_lights, int64_t* num_tiles, void* stream) {
    if (!ctx || !sum_tile_lights || !num_tiles) return PBR_ERR_INVALID_ARGUMENT;
    *sum_tile_lights = 0;
    *num_tiles = 0;
    pbr_pass_stats st;
    const int rc = sum_pass_stats(ctx, &st, stream, "pbr_last_cull_stats");
    if (rc != PBR_OK) return rc;
    *sum_tile_lights = st.cull_tile_lights;
    *num_tiles = st.cull_tiles;
    return PBR_OK;
}

int pbr_last_pass_stats(pbr_context* ctx, pbr_pass_stats* out, void* stream) {
    if (!ctx || !out) return PBR_ERR_INVALID_ARGUMENT;
    return sum_pass_stats(ctx, out, stream, "pbr_last_pass_stats");
}

const char* pbr_last_pass_kernel(pbr_context* ctx, void* stream) {
    if (!ctx) return "";
    std::lock_guard<std::mutex> lk(ctx->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int si = -1;
    for (size_t i = 0; i < ctx->streams.size(); ++i)
        if (ctx->streams[i].stream == s && ctx->streams[i].tiles > 0) si = (int)i;
    if (si < 0) si = ctx->last_stream;
    return si < 0 ? "" : ctx->streams[si].kernel.c_str();
}

int pbr_debug_bounds(pbr_context* ctx, uint32_t* flags, int reset) {
    if (!ctx) return PBR_ERR_INVALID_ARGUMENT;
    if (!PBR_DEBUG_BOUNDS) return PBR_ERR_UNSUPPORTED;
    DeviceGuard g(ctx->device);
    uint32_t* b = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_bounds_mu);
        b = g_bounds_buf[ctx->device];
    }
    if (!g.ok || !b) return PBR_ERR_NOT_READY;
    uint32_t h[2 * pbr::kBoundsClasses];
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h, b, kBoundsBytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(b, 0, kBoundsBytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail_hip(ctx, e, "pbr_debug_bounds");
    if (flags) std::memcpy(flags, h, kBoundsBytes);
    return PBR_OK;
}

}  // extern "C"

// Development (tools/raster_bench.py; not in the public header): one pbr_rasterize with HIP events between its stages;
// synchronises `stream` and writes the milliseconds of the clears and table upload, the vertex transform, the setup
// with the small triangles' coverage, the large triangles' coverage and the per-pixel resolve into ms5.
extern "C" int pbr_debug_rasterize_timed(pbr_context* ctx, const pbr_draw* draws, int32_t n_draws,
                                         const pbr_raster_view* view, const pbr_raster_targets* targets, void* stream,
                                         float* ms5) {
    if (!ctx || !ms5) return PBR_ERR_INVALID_ARGUMENT;
    DeviceGuard g(ctx->device);
    if (!g.ok) return PBR_ERR_NO_DEVICE;
    hipEvent_t ev[6] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    int rc = e == hipSuccess ? rasterize_impl(ctx, draws, n_draws, view, targets, stream, ev) : PBR_ERR_HIP;
    if (rc == PBR_OK && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = PBR_ERR_HIP;
    for (int i = 0; i < 5; ++i) {
        ms5[i] = 0.0f;
        if (rc == PBR_OK && hipEventElapsedTime(&ms5[i], ev[i], ev[i + 1]) != hipSuccess) rc = PBR_ERR_HIP;
    }
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    return rc;
}

// Development: the balanced pass's per-phase clock sums of a PBR_BAL_PROFILE build (not in the public header).
extern "C" int pbr_debug_bal_profile(unsigned long long* out8, int reset) {
    return pbr::debug_bal_profile(out8, reset != 0) == hipSuccess ? 0 : -1;
}

// Development: per-wave clock stamps of a PBR_WAVE_TIMELINE build into a device buffer of cap_waves * 8 words.
extern "C" int pbr_debug_wave_timeline(void* dev_buf, long long cap_waves) {
    return pbr::debug_wave_timeline(static_cast<unsigned long long*>(dev_buf), cap_waves) == hipSuccess ? 0 : -1;
}
