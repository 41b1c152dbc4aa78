// pbr_context.hip -- the C ABI of include/pbr/pbr_shade.h: context lifetime, pass/env upload and
// the shade entry point (the front end's entry points are in pbr_frontend.hip). Host code only; the kernels live in
// shade_kernels.hip and shade_kernels_bal.hip (shade_kernels.h is the interface).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "pbr_context_impl.h"
#include "pbr_debug_bounds.h"
#include "pbr_build_info.h"

// The build records of the library's units (pbr_build_info.h). Weak: a library linked without one of the units lists
// the records it has (an absent one is null).
extern "C" {
extern const char pbr_unit_info_shade_kernels[] __attribute__((weak));
extern const char pbr_unit_info_shade_kernels_bal[] __attribute__((weak));
extern const char pbr_unit_info_frontend_kernels[] __attribute__((weak));
extern const char pbr_unit_info_pbr_frontend[] __attribute__((weak));
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
// whose sum is 0 or inside [2^-100, 2^100] (shade_light_loops.h, lighting_fast's sum window). Every strength component of every
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

// The faithful finish's Reinhard is c x v_rcp_f32(c + 1) (shade_pixel.h, reinhard_faithful), and gfx950's v_rcp_f32
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
// (StreamState, Resource and the context itself: pbr_context_impl.h.)

// After the stream's work is complete (a device synchronisation): give back what a StreamState owns.
static void release_stream_state(StreamState& st) {
    if (st.last_pass) (void)hipEventDestroy(st.last_pass);
    if (st.d_stats) (void)hipFree(st.d_stats);
    if (st.raster.staged) (void)hipEventDestroy(st.raster.staged);
    if (st.raster.h) (void)hipHostFree(st.raster.h);
    if (st.raster.d) (void)hipFreeAsync(st.raster.d, nullptr);
    st = StreamState{};
}

int fail_hip(pbr_context* ctx, hipError_t e, const char* what, int status) {
    if (ctx) {
        ctx->last_error = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
    }
    return e == hipErrorOutOfMemory ? PBR_ERR_OUT_OF_MEMORY : status;
}

static bool is_ambient_mode(int m) { return m == PBR_AMBIENT_CONSTANT || m == PBR_AMBIENT_IBL_DIFFUSE; }

// PBR_DEBUG_BOUNDS builds (pbr_debug_bounds.h): one bounds-flag buffer per device, allocated, cleared and published
// to the kernels by the first context created on it; product builds have none.
constexpr int kBoundsMaxDevices = 64;
constexpr size_t kBoundsBytes = sizeof(uint32_t) * 2 * pbr::kBoundsClasses;
static std::mutex g_bounds_mu;
static uint32_t* g_bounds_buf[kBoundsMaxDevices] = {};

static hipError_t arm_bounds(int dev) {  // current device = dev
    if (!PBR_DEBUG_BOUNDS) return hipSuccess;
    if (dev < 0 || dev >= kBoundsMaxDevices) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_bounds_mu);
    if (g_bounds_buf[dev]) return hipSuccess;
    uint32_t* b = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b), kBoundsBytes);
    if (e == hipSuccess) e = hipMemset(b, 0, kBoundsBytes);
    if (e == hipSuccess) e = pbr::debug_bounds_publish(b);
    if (e == hipSuccess) e = pbr::debug_bounds_publish_frontend(b);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
        g_bounds_buf[dev] = b;
    else if (b)
        (void)hipFree(b);
    return e;
}

// PBR_DEBUG_BOUNDS_SKEW=1 (bounds-checked builds): the extents the checks use are too small -- the output extent of a
// pass one column narrower than the frame, the texel count of a resolve and the index count of a rasterisation 0 -- so
// every pass must report class "output", every textured resolve "texel" and every rasterisation "mesh": the negative
// controls of tests/test_gpu_debug_bounds.py. Only the checks read those extents; a flagged index is replaced by 0,
// which every one of those buffers holds.
bool debug_bounds_skew() {
    static const bool skew = [] {
        const char* e = std::getenv("PBR_DEBUG_BOUNDS_SKEW");
        return PBR_DEBUG_BOUNDS && e != nullptr && std::atoi(e) != 0;
    }();
    return skew;
}

// After a device synchronisation: every queued read and write of the context's resources is complete.
static void forget_readers(pbr_context* ctx) {
    for (Resource* r : ctx->resources) {
        r->readers.clear();
        r->writer = -1;
    }
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

// A launch on stream `s` (index si) has been queued: record the stream's last_pass, which orders a later write of
// what the launch read after it, once the context tracks more than one stream.
int after_launch(pbr_context* ctx, int si, hipStream_t s, const char* what) {
    if (ctx->streams.size() > 1) {
        const hipError_t e = hipEventRecord(ctx->streams[si].last_pass, s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
    }
    return PBR_OK;
}

extern "C" {

int pbr_abi_version(void) { return PBR_ABI_VERSION; }

const char* pbr_build_info(void) {
    static const std::string info = [] {
        std::string r = "{\"abi\": " + std::to_string(PBR_ABI_VERSION) + ", \"units\": [";
        bool first = true;
        for (const char* u : {pbr_unit_info_pbr_context, pbr_unit_info_pbr_frontend, pbr_unit_info_shade_kernels,
                              pbr_unit_info_shade_kernels_bal, pbr_unit_info_frontend_kernels,
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
    if (const char* e = std::getenv("PBR_RANK_PER_WAVE")) ctx->rank_per_wave = std::atoi(e) != 0;
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
        // The resources' buffers come from the stream-ordered pool (hipMallocAsync): returned the same way, after
        // the synchronisation above, and the pool's frees completed by the one below.
        for (Resource* r : ctx->resources) {
            for (void** m : r->mem)
                if (m && *m) (void)hipFreeAsync(*m, nullptr);
            if (r->written) (void)hipEventDestroy(r->written);
        }
        for (pbr_context::LightSlot& sl : ctx->slots) {  // the ring's host side
            if (sl.copied) (void)hipEventDestroy(sl.copied);
            if (sl.h) (void)hipHostFree(sl.h);
        }
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

    Entry en(ctx);
    if (const int rc = en.open(stream, "pbr_set_pass stream")) return rc;
    const hipStream_t s = en.s;
    const int si = en.si;
    hipError_t e = hipSuccess;
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
    Entry en(ctx);
    if (const int rc = en.open(stream, what)) return rc;
    const int n = width * height;
    const size_t bytes_u16 = sizeof(uint16_t) * 4 * (size_t)n, bytes_f32 = sizeof(float4) * (size_t)n;
    // Growing: the old texture may still be read by queued passes (released after them, in stream order); otherwise
    // it is replaced in place.
    const bool grow = n > t.capacity;
    if (grow) t.capacity = 0;
    const int rc = replace_buffers(en, t.use, grow, bytes_u16, bytes_f32, what, [&] {
        hipError_t e = unorm16 ? hipMemcpyAsync(t.d_u16, texels, bytes_u16, hipMemcpyHostToDevice, en.s)
                               : hipMemcpyAsync(t.d, texels, bytes_f32, hipMemcpyHostToDevice, en.s);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
        if (unorm16) e = pbr::launch_decode_unorm16(t.d_u16, t.d, n, en.s);
        return e == hipSuccess ? PBR_OK : fail_hip(ctx, e, "decode_unorm16_kernel", PBR_ERR_LAUNCH);
    });
    if (rc != PBR_OK) return rc;
    if (grow) t.capacity = n;
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

int shade(pbr_context* ctx, const pbr_gbuffer_soa* gb, const pbr_frame_desc* fr, void* stream) {
    if (!ctx || !gb || !fr) return PBR_ERR_INVALID_ARGUMENT;
    if (gb->width < 0 || gb->height < 0 || gb->row_stride < gb->width || fr->out_row_stride < gb->width)
        return PBR_ERR_INVALID_ARGUMENT;
    if (fr->format != PBR_OUTPUT_RGBA32F && fr->format != PBR_OUTPUT_RGBA8_UNORM) return PBR_ERR_INVALID_ARGUMENT;
    if (fr->coverage && fr->coverage_row_stride < gb->width) return PBR_ERR_INVALID_ARGUMENT;
    // Everything below reads context state that pbr_set_pass / pbr_set_*_map write under the same
    // mutex: the launch arguments are built (and the kernel queued) in one critical section, so a
    // concurrent set_pass can never tear them.
    Entry en(ctx);
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
    if (a.ps.balanced != 0 && ctx->rank_per_wave) a.ps.balanced |= pbr::kBalRankPerWave;

    if (const int rc = en.open(stream, "shade stream")) return rc;
    const hipStream_t s = en.s;
    const int si = en.si;
    hipError_t e = hipSuccess;
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
    if (const int rc = after_launch(ctx, si, s, "shade record")) return rc;
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

namespace {

// The StreamState index of the last pass on `s` or, if the context never launched on that stream, of its last pass on
// any stream (the caller's stream is then ordered after it by contract); -1: none.
int pass_stream(const pbr_context* ctx, hipStream_t s) {
    int si = -1;
    for (size_t i = 0; i < ctx->streams.size(); ++i)
        if (ctx->streams[i].stream == s && ctx->streams[i].tiles > 0) si = (int)i;
    return si < 0 ? ctx->last_stream : si;
}

// Sum the statistics records of that pass.
int sum_pass_stats(pbr_context* ctx, pbr_pass_stats* out, void* stream, const char* what) {
    *out = pbr_pass_stats{};
    Entry en(ctx);
    if (const int rc = en.device(stream)) return rc;
    const int si = pass_stream(ctx, en.s);
    if (si < 0 || ctx->streams[si].tiles == 0) return PBR_OK;  // no pass yet (or an empty frame)
    const StreamState& st = ctx->streams[si];
    std::vector<int32_t> h(pbr::kStatsPerBlock * (size_t)st.slots);
    hipError_t e = hipMemcpyAsync(h.data(), st.d_stats, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, en.s);
    if (e == hipSuccess) e = hipStreamSynchronize(en.s);
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
    const int si = pass_stream(ctx, static_cast<hipStream_t>(stream));
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

// Development: the balanced pass's per-phase clock sums of a PBR_BAL_PROFILE build (not in the public header).
extern "C" int pbr_debug_bal_profile(unsigned long long* out8, int reset) {
    return pbr::debug_bal_profile(out8, reset != 0) == hipSuccess ? 0 : -1;
}

// Development: per-wave clock stamps of a PBR_WAVE_TIMELINE build into a device buffer of cap_waves * 8 words.
extern "C" int pbr_debug_wave_timeline(void* dev_buf, long long cap_waves) {
    return pbr::debug_wave_timeline(static_cast<unsigned long long*>(dev_buf), cap_waves) == hipSuccess ? 0 : -1;
}
