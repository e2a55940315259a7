// The launch-order contract of the C ABI (include/rt_amd.h: "one launch in flight per context", "queued behind frames in flight") checked on
// the host, without a GPU and without the HIP runtime (CPU only; test infrastructure).  The library's host translation units are linked
// with two stand-ins:
//   - a fake runtime, below: the few dozen HIP functions those files call.  Device memory is heap memory (so the sanitizers see every copy
//     and fill), copies and fills are carried out at once, and every call is logged with its stream, its event and the ranges it reads and
//     writes;
//   - recording kernel launchers (launcher_recorders.h), which log a launch's stream and the buffers its argument block names.
// A checker computes happens-before over that log with vector clocks, one component per stream and one for the host, from
//   stream order; record -> wait-event edges; host waits (event / stream / device synchronize, blocking copies, hipFree, which waits for
//   the device: DevBuf::grow relies on it)
// and reports
//   - two accesses to one allocation, at least one a write, that are not ordered (the context's scratch: ticket counter, per-frame planes,
//     denoise records, camera table, tile lists, tile order and costs, the cull plane, the query records, an update's scratch; a scene's
//     blob, objects and triangle order under an update; the caller's buffers; the two timing events as one-word buffers);
//   - a range that leaves its allocation;
//   - host memory handed to an asynchronous copy (ViewsState::host, the pinned tile lists, locals) that is rewritten or released before
//     a host wait covers the copy: the copy's source is compared with a snapshot, and probed for poisoning, when the wait arrives;
//   - a pinned buffer released with such a copy pending; a timing event read before the host waited for it;
//   - a refused call that queued work or moved the context's launched / last_stream / have_timing.
// The driver runs the fixed sequences of tests/test_gpu_streams.py's cases and seeded random sequences of every entry point over 1-3
// streams (created non-blocking, like PyTorch's: the null stream does not wait for them) and 1-2 contexts, with sizes that regrow buffers
// and a tile-list cache of 3 entries instead of 64, so that entries are recycled, and regrown, under pending launches.
// Built with -DORDER_CHECK_NO_WAITS the fake hipStreamWaitEvent does nothing: the checker must then report violations
// (tests/test_launch_order.py asserts both outcomes).
//   order_host_check <seed> <iterations>     exit status 0 and "sanitizers silent", or 3 and the violations
#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define ORDER_POISONED(p, n) (__asan_region_is_poisoned(const_cast<void *>(static_cast<const void *>(p)), (n)) != nullptr)
#else
#define ORDER_POISONED(p, n) false
#endif

#include "rt_internal.h"

#include "launcher_recorders.h"

// ---- the log and the checker -----------------------------------------------------------------------------------------------------------
namespace {

constexpr int MAX_TIMELINES = 512;        // the host (0), the null stream (1), the caller's streams and every pipelined frame's stream
using Clock = std::array<uint32_t, MAX_TIMELINES>;

struct Access {
    int tl;                   // the timeline of the operation ...
    uint32_t c;               // ... and its number there: it happens before an operation with clock v iff v[tl] >= c
    size_t lo, hi;
    bool write;
    const char *op, *what;
    std::string call;
};

struct Alloc {
    size_t bytes = 0;
    bool device = true, caller = false;
    std::vector<Access> acc;
};

struct FakeEvent {
    bool timing = false, recorded = false;
    Clock at{};
    std::vector<Access> acc;  // a timing event's records, as writes of one word
};

struct FakeStream { int tl; };

struct PendingCopy {          // host memory an asynchronous copy reads or writes until a host wait covers it
    int tl;
    uint32_t c;
    const unsigned char *host;
    size_t bytes;
    bool from_host;
    std::vector<unsigned char> snapshot;
    std::string call;
};

Clock g_host{};                                   // what the host has waited for
std::vector<Clock> g_streams(2);                  // [tl]; 0 is not used, 1 is the null stream
std::map<uintptr_t, Alloc> g_allocs;              // by base address
std::vector<PendingCopy> g_pending;
std::string g_call = "(setup)";                   // the entry point the driver is in
bool g_caller_alloc = false;                      // the driver is allocating one of the caller's buffers
long g_ops = 0, g_violations = 0, g_accesses = 0, g_frees_waited = 0, g_launch_count = 0, g_lists_recycled = 0, g_lists_regrown = 0;
bool g_in_tile_list_call = false;                 // the driver is in a call that hands a tile list to the context's cache
std::mt19937 g_plan_rng(99);

std::set<std::string> g_named;                    // the buffers that reported violations have named
bool g_first_of_its_buffer = false;

// the first twelve are printed, and behind them the first one of every buffer not named yet
void violation(const char *fmt, ...)
{
    if (++g_violations > 12 && !g_first_of_its_buffer) return;
    std::fprintf(stderr, "order violation: ");
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "\n");
}

void join(Clock &into, const Clock &from) { for (int i = 0; i < MAX_TIMELINES; i++) into[i] = std::max(into[i], from[i]); }

int timeline(hipStream_t s) { return s ? reinterpret_cast<FakeStream *>(s)->tl : 1; }

// the next operation on `s`: behind what the stream holds and what the host has seen
Clock &enqueue(hipStream_t s)
{
    const int t = timeline(s);
    Clock &c = g_streams[(size_t)t];
    join(c, g_host);
    c[(size_t)t]++;
    g_ops++;
    return c;
}

bool host_has_waited_for(int tl, uint32_t c) { return g_host[(size_t)tl] >= c; }

void note(std::vector<Access> &list, const Clock &now, int tl, size_t lo, size_t hi, bool write, const char *op, const char *what)
{
    g_accesses++;
    for (size_t i = 0; i < list.size();) {
        Access &p = list[i];
        if (host_has_waited_for(p.tl, p.c)) { list[i] = list.back(); list.pop_back(); continue; }      // before everything still to come
        const bool ordered = now[(size_t)p.tl] >= p.c;
        if (p.lo < hi && lo < p.hi && (p.write || write) && !ordered) {
            g_first_of_its_buffer = g_named.insert(what).second;
            violation("%s %s [%zu, %zu) by %s in %s (stream %d) is not ordered behind %s %s [%zu, %zu) by %s in %s (stream %d)", write ? "write of" : "read of", what, lo, hi,
                      op, g_call.c_str(), tl, p.write ? "the write of" : "the read of", p.what, p.lo, p.hi, p.op, p.call.c_str(), p.tl);
            g_first_of_its_buffer = false;
        }
        if (ordered && p.lo >= lo && p.hi <= hi && (write || !p.write)) { list[i] = list.back(); list.pop_back(); continue; }   // the new access stands for it
        i++;
    }
    list.push_back(Access{tl, now[(size_t)tl], lo, hi, write, op, what, g_call});
}

Alloc *find_alloc(const void *p, uintptr_t *base)
{
    auto it = g_allocs.upper_bound((uintptr_t)p);
    if (it == g_allocs.begin()) return nullptr;
    --it;
    if ((uintptr_t)p >= it->first + it->second.bytes && !((uintptr_t)p == it->first && it->second.bytes == 0)) return nullptr;
    *base = it->first;
    return &it->second;
}

// `bytes` at `p` used by the operation with clock `now` on timeline `tl`; true: device memory (or pinned memory) of a known allocation
bool use(const Clock &now, int tl, const void *p, size_t bytes, bool write, const char *op, const char *what)
{
    if (!p || bytes == 0) return false;
    uintptr_t base = 0;
    Alloc *a = find_alloc(p, &base);
    if (!a) return false;
    const size_t lo = (uintptr_t)p - base;
    if (lo + bytes > a->bytes) {
        violation("%s: %s [%zu, %zu) by %s leaves its allocation of %zu bytes", g_call.c_str(), what, lo, lo + bytes, op, a->bytes);
        return true;
    }
    if (a->device) note(a->acc, now, tl, lo, lo + bytes, write, op, what);
    return a->device;
}

void check_pending(bool all)
{
    for (size_t i = 0; i < g_pending.size();) {
        PendingCopy &p = g_pending[i];
        if (!all && !host_has_waited_for(p.tl, p.c)) { i++; continue; }
        if (ORDER_POISONED(p.host, p.bytes))
            violation("host memory of an asynchronous copy queued in %s was released before a host wait covered the copy", p.call.c_str());
        else if (p.from_host && std::memcmp(p.host, p.snapshot.data(), p.bytes) != 0)
            violation("host memory of an asynchronous upload queued in %s was rewritten before a host wait covered the copy", p.call.c_str());
        g_pending[i] = std::move(g_pending.back());
        g_pending.pop_back();
    }
}

void host_waits_for(const Clock &c) { join(g_host, c); check_pending(false); }
void host_waits_for_device() { for (size_t t = 1; t < g_streams.size(); t++) join(g_host, g_streams[t]); check_pending(false); }

// a copy or a fill on `stream`, carried out at once
hipError_t copy(void *dst, const void *src, size_t bytes, hipStream_t stream, const char *op, bool blocking)
{
    if (bytes == 0) return hipSuccess;
    Clock &now = enqueue(stream);
    const int tl = timeline(stream);
    const bool src_dev = use(now, tl, src, bytes, false, op, "copy source"), dst_dev = use(now, tl, dst, bytes, true, op, "copy destination");
    std::memmove(dst, src, bytes);
    if (blocking) { host_waits_for(now); return hipSuccess; }
    if (!src_dev) {
        const unsigned char *h = static_cast<const unsigned char *>(src);
        g_pending.push_back(PendingCopy{tl, now[(size_t)tl], h, bytes, true, std::vector<unsigned char>(h, h + bytes), g_call});
    }
    if (!dst_dev) g_pending.push_back(PendingCopy{tl, now[(size_t)tl], static_cast<const unsigned char *>(dst), bytes, false, {}, g_call});
    return hipSuccess;
}

hipError_t fill(void *dst, int value, size_t bytes, hipStream_t stream, const char *op, bool blocking)
{
    if (bytes == 0) return hipSuccess;
    Clock &now = enqueue(stream);
    use(now, timeline(stream), dst, bytes, true, op, "fill");
    std::memset(dst, value, bytes);
    if (blocking) host_waits_for(now);
    return hipSuccess;
}

hipError_t allocate(void **p, size_t bytes, bool device)
{
    *p = std::calloc(bytes ? bytes : 1, 1);
    if (!*p) return hipErrorOutOfMemory;
    Alloc a;
    a.bytes = bytes;
    a.device = device;
    a.caller = g_caller_alloc;
    g_allocs[(uintptr_t)*p] = std::move(a);
    return hipSuccess;
}

}  // namespace

hipError_t rec::launch(const char *kernel, hipStream_t stream, std::initializer_list<Use> uses)
{
    Clock &now = enqueue(stream);
    g_launch_count++;
    for (const Use &u : uses) use(now, timeline(stream), u.p, u.bytes, u.write, kernel, u.what);
    return hipSuccess;
}

size_t rec::extent(const void *p)
{
    uintptr_t base = 0;
    const Alloc *a = find_alloc(p, &base);
    return a ? a->bytes - ((uintptr_t)p - base) : 0;
}

void rec::fill_plan(float *tile_error, uint32_t *tile_active, int num_tiles)
{
    for (int t = 0; t < num_tiles; t++) {
        tile_active[t] = g_plan_rng() % 3 == 0 ? 1u + g_plan_rng() % 64u : 0u;
        tile_error[t] = (float)(g_plan_rng() % 1000) / 1000.0f;
    }
}

// ---- the fake runtime: what the library's host translation units call ------------------------------------------------------------------
extern "C" {

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int)
{
    std::memset(prop, 0, sizeof *prop);
    prop->multiProcessorCount = 256;
    prop->totalGlobalMem = (size_t)1 << 30;        // small: rt_max_batch_frames stays at 32 for the images here
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "an error of the fake runtime"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipPeekAtLastError(void) { return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipDeviceCanAccessPeer(int *can, int, int) { *can = 0; return hipSuccess; }
hipError_t hipDeviceEnablePeerAccess(int, unsigned int) { return hipErrorNotSupported; }

hipError_t hipMalloc(void **p, size_t bytes) { return allocate(p, bytes, true); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return allocate(p, bytes, false); }

// waits for the device, then releases: what DevBuf::grow relies on.  Counted where it mattered: the buffer had an access the host had not waited for.
hipError_t hipFree(void *p)
{
    if (!p) return hipSuccess;
    auto it = g_allocs.find((uintptr_t)p);
    if (it == g_allocs.end() || !it->second.device) { violation("%s: hipFree of %p, which hipMalloc did not return", g_call.c_str(), p); return hipErrorInvalidValue; }
    for (const Access &a : it->second.acc)
        if (!host_has_waited_for(a.tl, a.c)) { g_frees_waited++; break; }
    host_waits_for_device();
    g_allocs.erase(it);
    std::free(p);
    return hipSuccess;
}

// does NOT wait here (the stricter reading): a pinned buffer goes only once the host has waited for the copies that read it
hipError_t hipHostFree(void *p)
{
    if (!p) return hipSuccess;
    auto it = g_allocs.find((uintptr_t)p);
    if (it == g_allocs.end() || it->second.device) { violation("%s: hipHostFree of %p, which hipHostMalloc did not return", g_call.c_str(), p); return hipErrorInvalidValue; }
    if (g_in_tile_list_call) g_lists_regrown++;     // (DevList::clear inside a call: a recycled entry too small for its new list)
    const unsigned char *lo = static_cast<const unsigned char *>(p), *hi = lo + it->second.bytes;
    for (const PendingCopy &c : g_pending)
        if (c.host >= lo && c.host < hi && !host_has_waited_for(c.tl, c.c))
            violation("%s: a pinned buffer is released while the upload queued in %s may still read it", g_call.c_str(), c.call.c_str());
    g_pending.erase(std::remove_if(g_pending.begin(), g_pending.end(), [&](const PendingCopy &c) { return c.host >= lo && c.host < hi; }), g_pending.end());
    g_allocs.erase(it);
    std::free(p);
    return hipSuccess;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { return copy(dst, src, bytes, nullptr, "hipMemcpy", true); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s) { return copy(dst, src, bytes, s, "hipMemcpyAsync", false); }
hipError_t hipMemcpyPeerAsync(void *dst, int, const void *src, int, size_t bytes, hipStream_t s) { return copy(dst, src, bytes, s, "hipMemcpyPeerAsync", false); }
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t s)
{
    for (size_t y = 0; y < height; y++) (void)copy(static_cast<char *>(dst) + y * dpitch, static_cast<const char *>(src) + y * spitch, width, s, "hipMemcpy2DAsync", false);
    return hipSuccess;
}
hipError_t hipMemset(void *dst, int value, size_t bytes) { return fill(dst, value, bytes, nullptr, "hipMemset", true); }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s) { return fill(dst, value, bytes, s, "hipMemsetAsync", false); }
hipError_t hipMemsetD16Async(hipDeviceptr_t dst, unsigned short value, size_t count, hipStream_t s)
{
    const hipError_t e = fill((void *)dst, 0, count * 2, s, "hipMemsetD16Async", false);
    for (size_t i = 0; i < count; i++) static_cast<unsigned short *>((void *)dst)[i] = value;
    return e;
}

static hipError_t new_stream(hipStream_t *s)
{
    if (g_streams.size() >= (size_t)MAX_TIMELINES) { std::fprintf(stderr, "order check: out of timelines\n"); std::exit(2); }
    *s = reinterpret_cast<hipStream_t>(new FakeStream{(int)g_streams.size()});
    g_streams.emplace_back();
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return new_stream(s); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { return new_stream(s); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    if (!s) return hipErrorInvalidHandle;
    delete reinterpret_cast<FakeStream *>(s);      // (its timeline stays: what ran on it is still in the log)
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { host_waits_for(g_streams[(size_t)timeline(s)]); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { host_waits_for_device(); return hipSuccess; }

static hipError_t new_event(hipEvent_t *e, bool timing)
{
    FakeEvent *f = new FakeEvent();
    f->timing = timing;
    *e = reinterpret_cast<hipEvent_t>(f);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return new_event(e, true); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int flags) { return new_event(e, !(flags & hipEventDisableTiming)); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    delete reinterpret_cast<FakeEvent *>(e);       // (waits already queued on it took its clock along)
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    FakeEvent *f = reinterpret_cast<FakeEvent *>(e);
    if (!f) return hipErrorInvalidHandle;
    Clock &now = enqueue(s);
    if (f->timing) note(f->acc, now, timeline(s), 0, 1, true, "hipEventRecord", "timing event");
    f->at = now;
    f->recorded = true;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int)
{
    FakeEvent *f = reinterpret_cast<FakeEvent *>(e);
    if (!f) return hipErrorInvalidHandle;
    g_ops++;
#if !defined(ORDER_CHECK_NO_WAITS)
    if (f->recorded) join(g_streams[(size_t)timeline(s)], f->at);
#else
    (void)s;
#endif
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    FakeEvent *f = reinterpret_cast<FakeEvent *>(e);
    if (!f) return hipErrorInvalidHandle;
    // fill_dev_list's waits (rt_capi.cpp), one per recycled entry: on ev_up before its pinned copy is rewritten, or on ev before an entry too
    // small is freed.  (In these calls nothing else waits for an event: ordinary launches only queue waits.)
    if (g_in_tile_list_call) g_lists_recycled++;
    if (f->recorded) host_waits_for(f->at);
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    FakeEvent *a = reinterpret_cast<FakeEvent *>(start), *b = reinterpret_cast<FakeEvent *>(stop);
    if (!a || !b || !a->recorded || !b->recorded) return hipErrorInvalidHandle;
    for (FakeEvent *f : {a, b})
        for (int t = 1; t < MAX_TIMELINES; t++)
            if (f->at[(size_t)t] > g_host[(size_t)t]) { violation("%s: a timing event is read before the host waited for it", g_call.c_str()); return hipErrorNotReady; }
    *ms = 1.0f;
    return hipSuccess;
}

}  // extern "C"

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
namespace {

#define REQUIRE(cond)                                                                                              \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "order check: %s failed in %s (line %d)\n", #cond, g_call.c_str(), __LINE__); std::exit(2); } \
    } while (0)

constexpr int MAX_W = 96, MAX_H = 64, MAX_PX = MAX_W * MAX_H, MAX_VIEWS = 4, MAX_RAYS = 4096 + 17;
constexpr int MESH_TRIS = 60, MAX_MULTI = 1024 + 17;       // the mesh scene's one mesh (object 0); rays of a multi-hit call (RT_MULTIHIT_MAX records each)

template <class T> T *caller_alloc(size_t n)
{
    void *p = nullptr;
    g_caller_alloc = true;
    REQUIRE(hipMalloc(&p, n * sizeof(T)) == hipSuccess);
    g_caller_alloc = false;
    return static_cast<T *>(p);
}

// the buffers of a caller who works on one stream: whatever touches them is ordered through that stream
struct CallerBuffers {
    float *frame, *prev, *frames, *compact, *origins, *directions, *tmax, *depth, *normal, *albedo, *ray, *ao, *tile_error, *half_a, *half_b, *denoised;
    float *triangles, *winding, *sdf, *radius, *query_tris;
    int32_t *object, *counts;
    rt_hit *hits, *multi_hits;
    rt_nearest *nearest;
    rt_sweep *sweeps;
    rt_overlap_id *ids;           // MAX_MULTI queries of an overlap call, RT_OVERLAP_MAX ids (and segments) each
    rt_tri_segment *segments;
    unsigned char *spare;         // where the caller copies an answer to (as large as the largest: the multi-hit records)
    uint8_t *occluded, *visibility, *rgba, *inside;
    uint16_t *ao_count, *budget;
    uint32_t *count, *tile_active;
    std::vector<void *> all;
    void create()
    {
        auto f = [&](size_t n) { float *p = caller_alloc<float>(n); all.push_back(p); return p; };
        frame = f(3 * MAX_PX); prev = f(3 * MAX_PX); frames = f((size_t)MAX_VIEWS * 3 * MAX_PX); compact = f(3 * MAX_PX + 192 * 8);
        origins = f(3 * MAX_RAYS); directions = f(3 * MAX_RAYS); tmax = f(MAX_RAYS);
        depth = f(MAX_PX); normal = f(3 * MAX_PX); albedo = f(3 * MAX_PX); ray = f(3 * MAX_PX); ao = f(MAX_PX); tile_error = f(MAX_PX / 64 + 64);
        half_a = f(3 * MAX_PX); half_b = f(3 * MAX_PX); denoised = f(3 * MAX_PX);
        triangles = f(9 * MESH_TRIS); winding = f(MAX_RAYS); sdf = f(MAX_RAYS); radius = f(MAX_RAYS); query_tris = f(9 * MAX_MULTI);
        sweeps = caller_alloc<rt_sweep>(MAX_RAYS); ids = caller_alloc<rt_overlap_id>((size_t)MAX_MULTI * RT_OVERLAP_MAX);
        segments = caller_alloc<rt_tri_segment>((size_t)MAX_MULTI * RT_OVERLAP_MAX);
        for (void *p : {(void *)sweeps, (void *)ids, (void *)segments}) all.push_back(p);
        counts = caller_alloc<int32_t>(MAX_RAYS); multi_hits = caller_alloc<rt_hit>((size_t)MAX_MULTI * RT_MULTIHIT_MAX); nearest = caller_alloc<rt_nearest>(MAX_RAYS);
        spare = caller_alloc<unsigned char>((size_t)MAX_MULTI * RT_MULTIHIT_MAX * sizeof(rt_hit)); inside = caller_alloc<uint8_t>(MAX_RAYS);
        for (void *p : {(void *)counts, (void *)multi_hits, (void *)nearest, (void *)spare, (void *)inside}) all.push_back(p);
        object = caller_alloc<int32_t>(MAX_PX); hits = caller_alloc<rt_hit>(MAX_RAYS);
        occluded = caller_alloc<uint8_t>(MAX_RAYS); visibility = caller_alloc<uint8_t>(MAX_PX); rgba = caller_alloc<uint8_t>(4 * MAX_PX);
        ao_count = caller_alloc<uint16_t>(MAX_PX); budget = caller_alloc<uint16_t>(MAX_PX);
        count = caller_alloc<uint32_t>(MAX_PX); tile_active = caller_alloc<uint32_t>(MAX_PX / 64 + 64);
        for (void *p : {(void *)object, (void *)hits, (void *)occluded, (void *)visibility, (void *)rgba, (void *)ao_count, (void *)budget, (void *)count, (void *)tile_active}) all.push_back(p);
    }
    void destroy() { for (void *p : all) REQUIRE(hipFree(p) == hipSuccess); all.clear(); }
};

struct World {
    std::mt19937 rng;
    hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};     // [0] is the null stream
    CallerBuffers bufs[4];
    int n_streams = 1;
    rt_ctx *ctx[2] = {nullptr, nullptr};
    rt_scene *plain[2] = {nullptr, nullptr}, *mesh[2] = {nullptr, nullptr}, *textured[2] = {nullptr, nullptr};
    rt_sky *sky[2] = {nullptr, nullptr};
    int n_ctx = 1;
    rt_scene_builder *b_plain = nullptr, *b_mesh = nullptr, *b_textured = nullptr;
    long calls = 0, refused = 0;

    int pick(int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); }

    void build_scenes()
    {
        rt_material m;
        const float grey[3] = {0.5f, 0.5f, 0.5f};
        rt_material_standard(&m, grey, 0.2f);
        REQUIRE(rt_scene_builder_create(&b_plain) == RT_OK && rt_scene_builder_create(&b_mesh) == RT_OK);
        for (int i = 0; i < 3; i++) {
            const float c[3] = {-0.6f + 0.6f * (float)i, 0.0f, 2.0f};
            REQUIRE(rt_scene_add_sphere(b_plain, c, 0.3f, &m) == RT_OK);
        }
        std::vector<float> tris;
        for (int i = 0; i < 60 * 9; i++) tris.push_back(-1.0f + 2.0f * (float)(rng() % 1000) / 1000.0f + (i % 3 == 2 ? 2.5f : 0.0f));
        REQUIRE(rt_scene_add_mesh(b_mesh, tris.data(), 60, &m) == RT_OK);
        const float c[3] = {0.0f, 1.0f, 2.0f};
        REQUIRE(rt_scene_add_sphere(b_mesh, c, 0.2f, &m) == RT_OK);
        // a sphere whose material wants texture coordinates: a multi-hit query on it runs its second kernel
        rt_material squares;
        const float dark[3] = {0.1f, 0.1f, 0.1f};
        rt_material_checkerboard(&squares, grey, dark, 8, 0.0f);
        REQUIRE(rt_scene_builder_create(&b_textured) == RT_OK && rt_scene_add_sphere(b_textured, c, 0.5f, &squares) == RT_OK);
    }

    void create_ctx(int k)
    {
        g_call = "rt_ctx_create";
        REQUIRE(rt_ctx_create(0, &ctx[k]) == RT_OK);
        ctx[k]->tile_lists.cap = 3;         // (64 in the library: the driver has some 25 distinct lists, and recycling an entry under pending work is what is to be seen)
        REQUIRE(rt_scene_commit(ctx[k], b_plain, &plain[k]) == RT_OK && rt_scene_commit(ctx[k], b_mesh, &mesh[k]) == RT_OK);
        REQUIRE(rt_scene_commit(ctx[k], b_textured, &textured[k]) == RT_OK && textured[k]->flat.objects[0].need_uv);
        REQUIRE(mesh[k]->flat.objects[0].type == RT_OBJ_MESH && mesh[k]->flat.num_tris == MESH_TRIS);
        const std::vector<float> faces(6 * 4 * 4 * 3, 0.5f);
        REQUIRE(rt_sky_create(ctx[k], 4, faces.data(), &sky[k]) == RT_OK);
    }

    // with work pending: the context's members must go in an order that waits first
    void destroy_ctx(int k)
    {
        g_call = "rt_ctx_destroy";
        rt_scene_destroy(plain[k]);
        rt_scene_destroy(mesh[k]);
        rt_scene_destroy(textured[k]);
        sky[k]->ctx = nullptr;              // (detached: rt_sky_destroy would wait for the context first, and what is to be seen is the context going with work pending)
        rt_ctx_destroy(ctx[k]);
        rt_sky_destroy(sky[k]);
        ctx[k] = nullptr;
    }

    void setup(int streams_wanted, int contexts)
    {
        n_streams = streams_wanted;
        n_ctx = contexts;
        for (int s = 1; s < n_streams; s++) REQUIRE(hipStreamCreateWithFlags(&streams[s], hipStreamNonBlocking) == hipSuccess);
        for (int s = 0; s < n_streams; s++) bufs[s].create();
        for (int k = 0; k < n_ctx; k++) create_ctx(k);
    }

    void teardown()
    {
        for (int k = 0; k < n_ctx; k++) destroy_ctx(k);
        g_call = "(teardown)";
        REQUIRE(hipDeviceSynchronize() == hipSuccess);
        for (int s = 0; s < n_streams; s++) bufs[s].destroy();
        for (int s = 1; s < n_streams; s++) { REQUIRE(hipStreamDestroy(streams[s]) == hipSuccess); streams[s] = nullptr; }
        check_pending(true);
    }

    // ---- one call of every entry point.  k: the context, s: the caller's stream (and its buffers), mesh: which scene, w x h: the image
    struct Shape { int k, s, w, h; bool mesh; };
    rt_camera cam_of(const Shape &c, float dx = 0.0f)
    {
        rt_camera cam;
        const float pos[3] = {dx, 0.0f, 0.0f};
        rt_camera_make(c.w, c.h, pos, 1.0f, 0.1f, 0.0f, 0.0f, 0.0f, &cam);
        return cam;
    }
    rt_scene *scene_of(const Shape &c) { return c.mesh ? mesh[c.k] : plain[c.k]; }
    std::vector<uint32_t> some_tiles(const Shape &c, int which)
    {
        const int n = ((c.w + 7) / 8) * ((c.h + 7) / 8);
        std::vector<uint32_t> list;
        for (int t = which % 2; t < n; t += which == 4 ? 1 : 2) list.push_back((uint32_t)t);      // 4: every tile - more than an entry made for a short list holds
        if (which >= 2) std::reverse(list.begin(), list.end());
        if (list.empty()) list.push_back(0u);       // (an image of one tile)
        return list;
    }
    rt_render_settings settings(int spp) { return rt_render_settings{spp, 4, 1, {0.5f, 0.7f, 1.0f}}; }

    void expect_ok(rt_status st, const Shape &c)
    {
        calls++;
        if (st != RT_OK) { std::fprintf(stderr, "order check: %s failed: %s\n", g_call.c_str(), rt_last_error(ctx[c.k])); std::exit(2); }
    }

    // what the caller does around a call on its stream: produce the inputs ahead of it, consume the outputs behind it
    void caller_touches(const Shape &c, bool before)
    {
        CallerBuffers &b = bufs[c.s];
        if (before) REQUIRE(hipMemsetAsync(b.frame, 0, (size_t)c.w * c.h * 12, streams[c.s]) == hipSuccess);
        else REQUIRE(hipMemcpyAsync(b.prev, b.frame, (size_t)c.w * c.h * 12, hipMemcpyDeviceToDevice, streams[c.s]) == hipSuccess);
    }

    void render_device(const Shape &c, int spec, int spp)
    {
        g_call = "rt_render_device";
        CallerBuffers &b = bufs[c.s];
        const rt_camera cam = cam_of(c);
        const rt_render_settings rs = settings(spp);
        rt_tile_spec t = rt_sched::whole_image_spec();
        std::vector<uint32_t> list;
        if (spec == 1) { t.band_rows = 16; t.band_stride = 2; t.band_first = pick(0, 1); t.compact = pick(0, 1); }
        if (spec >= 2) { list = some_tiles(c, spec - 2); t.tile_list = list.data(); t.num_tiles = (int32_t)list.size(); t.compact = pick(0, 1); }
        caller_touches(c, true);
        g_in_tile_list_call = spec >= 2;
        expect_ok(rt_render_device(ctx[c.k], scene_of(c), &cam, &rs, pick(-99, 99999), pick(0, 3), &t, pick(0, 1) ? b.prev : nullptr, t.compact ? b.compact : b.frame, streams[c.s]), c);
        g_in_tile_list_call = false;
        caller_touches(c, false);
    }
    void render_batch(const Shape &c, int spec, int spp)
    {
        g_call = "rt_render_device_batch";
        const rt_camera cam = cam_of(c);
        const rt_render_settings rs = settings(spp);
        rt_tile_spec t = rt_sched::whole_image_spec();
        std::vector<uint32_t> list;
        if (spec >= 2) { list = some_tiles(c, spec - 2); t.tile_list = list.data(); t.num_tiles = (int32_t)list.size(); }
        const int32_t times[4] = {5, 6, 7, 8};
        caller_touches(c, true);
        g_in_tile_list_call = spec >= 2;
        expect_ok(rt_render_device_batch(ctx[c.k], scene_of(c), &cam, &rs, times, pick(1, 4), pick(0, 2), &t, bufs[c.s].frame, streams[c.s]), c);
        g_in_tile_list_call = false;
        caller_touches(c, false);
    }
    bool frame_submit(const Shape &c, int spp)
    {
        g_call = "rt_frame_submit";
        if (rt_frames_pending(ctx[c.k]) >= ctx[c.k]->pipe.depth) return false;
        const rt_camera cam = cam_of(c);
        const rt_render_settings rs = settings(spp);
        expect_ok(rt_frame_submit(ctx[c.k], scene_of(c), &cam, &rs, pick(0, 9999), nullptr), c);
        return true;
    }
    bool frame_collect(int k, int s, bool discard)
    {
        g_call = "rt_frame_collect";
        if (rt_frames_pending(ctx[k]) <= 0) return false;
        const rt_sched::Layout &L = ctx[k]->pipe.slots[ctx[k]->pipe.order[0]].layout;
        const Shape c{k, s, L.width, L.height, false};
        if (!discard) caller_touches(c, true);
        expect_ok(rt_frame_collect(ctx[k], pick(0, 3), discard ? nullptr : bufs[s].frame, streams[s]), c);
        if (!discard) caller_touches(c, false);
        return true;
    }
    void render_views(const Shape &c, int n, bool accumulate, float dx)
    {
        g_call = "rt_render_views_device";
        std::vector<rt_camera> cams;
        for (int i = 0; i < n; i++) cams.push_back(cam_of(c, dx + 0.1f * (float)i));
        const int32_t times[MAX_VIEWS] = {1, 2, 3, 4};
        const rt_render_settings rs = settings(3);
        expect_ok(rt_render_views_device(ctx[c.k], scene_of(c), cams.data(), times, n, &rs, accumulate, accumulate ? pick(0, 2) : 0, bufs[c.s].frames, streams[c.s]), c);
    }
    void render_sky(const Shape &c, int n, bool accumulate, float dx)
    {
        g_call = "rt_render_sky_device";
        std::vector<rt_camera> cams;
        for (int i = 0; i < n; i++) cams.push_back(cam_of(c, dx + 0.1f * (float)i));
        const int32_t times[MAX_VIEWS] = {1, 2, 3, 4};
        const rt_render_settings rs = settings(3);
        expect_ok(rt_render_sky_device(ctx[c.k], scene_of(c), sky[c.k], cams.data(), times, n, &rs, accumulate, accumulate ? pick(0, 2) : 0, bufs[c.s].frames, streams[c.s]), c);
    }
    void render_budget(const Shape &c, int list_kind, bool with_count)
    {
        g_call = "rt_render_budget_device";
        CallerBuffers &b = bufs[c.s];
        const rt_camera cam = cam_of(c);
        const rt_render_settings rs = settings(0);
        rt_tile_spec t = rt_sched::whole_image_spec();
        std::vector<uint32_t> list;
        if (list_kind >= 0) { list = some_tiles(c, list_kind); t.tile_list = list.data(); t.num_tiles = (int32_t)list.size(); }
        g_in_tile_list_call = list_kind >= 0;
        expect_ok(rt_render_budget_device(ctx[c.k], scene_of(c), &cam, &rs, 77, list_kind >= 0 ? &t : nullptr, b.budget, with_count ? b.count : nullptr, b.frame, streams[c.s]), c);
        g_in_tile_list_call = false;
    }
    void adaptive_plan(const Shape &c)
    {
        g_call = "rt_adaptive_plan_device";
        CallerBuffers &b = bufs[c.s];
        rt_adaptive_params p;
        rt_adaptive_params_default(&p);
        expect_ok(rt_adaptive_plan_device(ctx[c.k], c.w, c.h, b.half_a, b.half_b, b.count, &p, b.budget, b.tile_error, b.tile_active, streams[c.s]), c);
    }
    void trace_rays(const Shape &c, int n)
    {
        g_call = "rt_trace_rays_device";
        CallerBuffers &b = bufs[c.s];
        expect_ok(rt_trace_rays_device(ctx[c.k], scene_of(c), b.origins, b.directions, n, b.hits, streams[c.s]), c);
    }
    // what the caller does around a query on its stream: write `in` ahead of it, copy `out` away behind it
    void caller_writes(const Shape &c, void *in, size_t bytes) { REQUIRE(hipMemsetAsync(in, 0, bytes, streams[c.s]) == hipSuccess); }
    void caller_reads(const Shape &c, const void *out, size_t bytes) { REQUIRE(hipMemcpyAsync(bufs[c.s].spare, out, bytes, hipMemcpyDeviceToDevice, streams[c.s]) == hipSuccess); }

    // the mesh scene's mesh rebuilt from the caller's vertices: the scene blob is rewritten under whatever reads it, and the view's cull plane goes stale
    void update_mesh(const Shape &c)
    {
        g_call = "rt_scene_update_mesh_device";
        caller_writes(c, bufs[c.s].triangles, (size_t)MESH_TRIS * 36);
        expect_ok(rt_scene_update_mesh_device(ctx[c.k], mesh[c.k], 0, bufs[c.s].triangles, MESH_TRIS, streams[c.s]), c);
    }
    void nearest_points(const Shape &c, int n, bool limits)
    {
        g_call = "rt_nearest_points_device";
        CallerBuffers &b = bufs[c.s];
        caller_writes(c, b.origins, (size_t)n * 12);
        expect_ok(rt_nearest_points_device(ctx[c.k], scene_of(c), b.origins, limits ? b.tmax : nullptr, n, b.nearest, streams[c.s]), c);
        caller_reads(c, b.nearest, (size_t)n * sizeof(rt_nearest));
    }
    // which: 0 the plain scene, 1 the mesh scene, 2 the one whose sphere wants texture coordinates (with k > 0: the second kernel)
    void trace_multi(const Shape &c, int which, int n, int k, bool with_counts)
    {
        g_call = "rt_trace_rays_multi_device";
        CallerBuffers &b = bufs[c.s];
        rt_scene *sc = which == 2 ? textured[c.k] : which == 1 ? mesh[c.k] : plain[c.k];
        caller_writes(c, b.directions, (size_t)n * 12);
        expect_ok(rt_trace_rays_multi_device(ctx[c.k], sc, b.origins, b.directions, pick(0, 1) ? b.tmax : nullptr, n, k, k > 0 ? b.multi_hits : nullptr,
                                             with_counts || k == 0 ? b.counts : nullptr, streams[c.s]), c);
        if (k > 0) caller_reads(c, b.multi_hits, (size_t)n * (size_t)k * sizeof(rt_hit));
        else caller_reads(c, b.counts, (size_t)n * 4);
    }
    void winding_numbers(const Shape &c, int n, bool solids, int outputs)
    {
        g_call = "rt_winding_numbers_device";
        CallerBuffers &b = bufs[c.s];
        caller_writes(c, b.origins, (size_t)n * 12);
        expect_ok(rt_winding_numbers_device(ctx[c.k], scene_of(c), b.origins, n, solids ? RT_WINDING_SOLIDS : 0, outputs & 1 ? b.winding : nullptr, outputs & 2 ? b.inside : nullptr,
                                            streams[c.s]), c);
        if (outputs & 1) caller_reads(c, b.winding, (size_t)n * 4);
        if (outputs & 2) caller_reads(c, b.inside, (size_t)n);
    }
    // own_records: the caller's record buffer; without it the records are the context's, grown behind a wait when n outgrows them
    void signed_distance(const Shape &c, int n, bool own_records, bool limits)
    {
        g_call = "rt_signed_distance_device";
        CallerBuffers &b = bufs[c.s];
        caller_writes(c, b.origins, (size_t)n * 12);
        expect_ok(rt_signed_distance_device(ctx[c.k], scene_of(c), b.origins, limits ? b.tmax : nullptr, n, own_records ? b.nearest : nullptr, b.sdf, streams[c.s]), c);
        caller_reads(c, b.sdf, (size_t)n * 4);
        if (own_records) caller_reads(c, b.nearest, (size_t)n * sizeof(rt_nearest));
    }
    // the nearest-surface records between the two launches are the context's, as in signed_distance without own_records
    void sweep_spheres(const Shape &c, int n, bool limits)
    {
        g_call = "rt_sweep_spheres_device";
        CallerBuffers &b = bufs[c.s];
        caller_writes(c, b.origins, (size_t)n * 12);
        caller_writes(c, b.radius, (size_t)n * 4);
        expect_ok(rt_sweep_spheres_device(ctx[c.k], scene_of(c), b.origins, b.directions, b.radius, limits ? b.tmax : nullptr, n, b.sweeps, streams[c.s]), c);
        caller_reads(c, b.sweeps, (size_t)n * sizeof(rt_sweep));
    }
    // outputs: 1 the counts, 2 the bytes; k == 0 with the bytes alone is the kernels' any-only mode
    void overlap_boxes(const Shape &c, int n, int k, int outputs)
    {
        g_call = "rt_overlap_boxes_device";
        CallerBuffers &b = bufs[c.s];
        caller_writes(c, b.origins, (size_t)n * 12);
        caller_writes(c, b.directions, (size_t)n * 12);
        expect_ok(rt_overlap_boxes_device(ctx[c.k], scene_of(c), b.origins, b.directions, n, k, k > 0 ? b.ids : nullptr, outputs & 1 ? b.counts : nullptr,
                                          outputs & 2 ? b.inside : nullptr, streams[c.s]), c);
        if (k > 0) caller_reads(c, b.ids, (size_t)n * (size_t)k * sizeof(rt_overlap_id));
        if (outputs & 1) caller_reads(c, b.counts, (size_t)n * 4);
        if (outputs & 2) caller_reads(c, b.inside, (size_t)n);
    }
    void overlap_triangles(const Shape &c, int n, int k, int outputs, bool with_segments)
    {
        g_call = "rt_overlap_triangles_device";
        CallerBuffers &b = bufs[c.s];
        const bool segs = with_segments && k > 0;
        caller_writes(c, b.query_tris, (size_t)n * 36);
        expect_ok(rt_overlap_triangles_device(ctx[c.k], scene_of(c), b.query_tris, n, k, k > 0 ? b.ids : nullptr, outputs & 1 ? b.counts : nullptr,
                                              outputs & 2 ? b.inside : nullptr, segs ? b.segments : nullptr, streams[c.s]), c);
        if (k > 0) caller_reads(c, b.ids, (size_t)n * (size_t)k * sizeof(rt_overlap_id));
        if (segs) caller_reads(c, b.segments, (size_t)n * (size_t)k * sizeof(rt_tri_segment));
        if (outputs & 1) caller_reads(c, b.counts, (size_t)n * 4);
        if (outputs & 2) caller_reads(c, b.inside, (size_t)n);
    }
    void render_aov(const Shape &c)
    {
        g_call = "rt_render_aov_device";
        CallerBuffers &b = bufs[c.s];
        const rt_camera cam = cam_of(c);
        const float sky[3] = {1.0f, 1.0f, 1.0f};
        expect_ok(rt_render_aov_device(ctx[c.k], scene_of(c), &cam, sky, b.depth, b.normal, pick(0, 1) ? b.albedo : nullptr, b.object, b.ray, streams[c.s]), c);
    }
    void occluded_rays(const Shape &c, int n, bool limits)
    {
        g_call = "rt_occluded_rays_device";
        CallerBuffers &b = bufs[c.s];
        expect_ok(rt_occluded_rays_device(ctx[c.k], scene_of(c), b.origins, b.directions, limits ? b.tmax : nullptr, n, b.occluded, streams[c.s]), c);
    }
    void render_visibility(const Shape &c)
    {
        g_call = "rt_render_visibility_device";
        const rt_camera cam = cam_of(c);
        const float light[3] = {0.0f, 3.0f, 1.0f};
        expect_ok(rt_render_visibility_device(ctx[c.k], scene_of(c), &cam, light, 1e-3f, bufs[c.s].visibility, streams[c.s]), c);
    }
    void render_ao(const Shape &c)
    {
        g_call = "rt_render_ao_device";
        CallerBuffers &b = bufs[c.s];
        const rt_camera cam = cam_of(c);
        expect_ok(rt_render_ao_device(ctx[c.k], scene_of(c), &cam, 4, 0.5f, 1e-3f, 5, b.ao_count, b.ao, streams[c.s]), c);
    }
    void denoise(const Shape &c, bool in_place)
    {
        g_call = "rt_denoise_device";
        CallerBuffers &b = bufs[c.s];
        rt_denoise_params p;
        rt_denoise_params_default(&p);
        p.iterations = pick(1, 3);
        expect_ok(rt_denoise_device(ctx[c.k], c.w, c.h, b.frame, b.normal, b.depth, b.object, b.albedo, &p, in_place ? b.frame : b.denoised, streams[c.s]), c);
    }
    void to_rgba8(const Shape &c)
    {
        g_call = "rt_to_rgba8_device";
        expect_ok(rt_to_rgba8_device(ctx[c.k], bufs[c.s].frame, c.w, c.h, bufs[c.s].rgba, streams[c.s]), c);
    }
    void tiles_copy(const Shape &c, int list_kind, bool to_frame)
    {
        g_call = "rt_tiles_copy_device";
        const std::vector<uint32_t> list = some_tiles(c, list_kind);
        g_in_tile_list_call = true;
        expect_ok(rt_tiles_copy_device(ctx[c.k], bufs[c.s].compact, bufs[c.s].frame, c.w, c.h, list.data(), (int32_t)list.size(), to_frame, streams[c.s]), c);
        g_in_tile_list_call = false;
    }

    // the host-buffer forms: the null stream and blocking copies
    void host_form(const Shape &c, int which)
    {
        static std::vector<float> f((size_t)MAX_VIEWS * 3 * MAX_PX), g(3 * MAX_PX), d(MAX_PX), rays(6 * MAX_RAYS, 1.0f);
        static std::vector<int32_t> obj(MAX_PX);
        static std::vector<uint32_t> cnt(MAX_PX);
        static std::vector<uint16_t> bud(MAX_PX, 2), aoc(MAX_PX);
        static std::vector<uint8_t> bytes(std::max(MAX_PX, MAX_RAYS));
        static std::vector<rt_hit> hits(MAX_RAYS);
        const rt_camera cam = cam_of(c);
        const rt_render_settings rs = settings(2);
        const float v3[3] = {0.5f, 2.0f, 1.0f};
        int32_t fn = pick(0, 2);
        const int32_t times[5] = {3, 1, 4, 1, 5};
        rt_ctx *x = ctx[c.k];
        rt_scene *sc = scene_of(c);
        rt_adaptive_params ap;
        rt_adaptive_params_default(&ap);
        ap.pilot_spp = 2; ap.step_spp = 2; ap.max_spp = 16; ap.max_passes = pick(0, 3);
        rt_adaptive_stats stats;
        rt_denoise_params dp;
        rt_denoise_params_default(&dp);
        dp.iterations = 2;
        switch (which) {
            case 0: g_call = "rt_render"; expect_ok(rt_render(x, sc, &cam, &rs, 11, &fn, f.data()), c); break;
            case 1: g_call = "rt_render_frames"; expect_ok(rt_render_frames(x, sc, &cam, &rs, times, pick(1, 5), &fn, f.data()), c); break;
            case 2: g_call = "rt_trace_rays"; expect_ok(rt_trace_rays(x, sc, rays.data(), rays.data() + 3 * MAX_RAYS, pick(1, MAX_RAYS), hits.data()), c); break;
            case 3: g_call = "rt_render_aov"; expect_ok(rt_render_aov(x, sc, &cam, v3, d.data(), g.data(), nullptr, obj.data(), nullptr), c); break;
            case 4: g_call = "rt_occluded_rays"; expect_ok(rt_occluded_rays(x, sc, rays.data(), rays.data() + 3 * MAX_RAYS, pick(0, 1) ? rays.data() : nullptr, pick(1, MAX_RAYS), bytes.data()), c); break;
            case 5: g_call = "rt_render_visibility"; expect_ok(rt_render_visibility(x, sc, &cam, v3, 1e-3f, bytes.data()), c); break;
            case 6: g_call = "rt_render_ao"; expect_ok(rt_render_ao(x, sc, &cam, 3, 1.0f, 0.0f, 9, aoc.data(), d.data()), c); break;
            case 7: g_call = "rt_denoise"; expect_ok(rt_denoise(x, c.w, c.h, f.data(), g.data(), d.data(), obj.data(), nullptr, &dp, f.data() + 3 * MAX_PX), c); break;
            case 8: g_call = "rt_render_budget"; expect_ok(rt_render_budget(x, sc, &cam, &rs, 5, nullptr, bud.data(), cnt.data(), f.data()), c); break;
            case 9: {
                g_call = "rt_render_views";
                std::vector<rt_camera> cams(3, cam);
                const int acc = pick(0, 1);
                if (!acc) fn = 0;
                expect_ok(rt_render_views(x, sc, cams.data(), times, 3, &rs, acc, &fn, f.data()), c);
                break;
            }
            case 10: g_call = "rt_render_adaptive"; expect_ok(rt_render_adaptive(x, sc, &cam, &rs, 3, &ap, bufs[c.s].frame, bufs[c.s].count, &stats, streams[c.s]), c); break;
            case 11: g_call = "rt_render_adaptive_host"; expect_ok(rt_render_adaptive_host(x, sc, &cam, &rs, 3, &ap, f.data(), cnt.data(), &stats), c); break;
            case 12: {
                g_call = "rt_frame_collect_host";
                if (rt_frames_pending(x) <= 0) break;
                const rt_sched::Layout &L = x->pipe.slots[x->pipe.order[0]].layout;
                if (!L.whole_frame()) break;
                expect_ok(rt_frame_collect_host(x, &fn, pick(0, 3) ? f.data() : nullptr), c);
                break;
            }
            case 13: {
                g_call = "rt_tile_costs";
                std::vector<uint32_t> ids(200), cost(200), peak(200);
                int32_t n = 0;
                (void)rt_tile_costs(x, ids.data(), cost.data(), peak.data(), 200, &n);        // (refused when no launch has measured: either is fine)
                calls++;
                break;
            }
            case 14: {
                g_call = "rt_last_kernel_ms";
                float ms = 0.0f;
                if (x->have_timing) expect_ok(rt_last_kernel_ms(x, &ms), c);
                break;
            }
            case 15: g_call = "rt_ctx_synchronize"; expect_ok(rt_ctx_synchronize(x), c); break;
            default: g_call = "rt_frame_wait"; expect_ok(rt_frame_wait(x), c); break;
        }
    }

    // calls the library refuses: they must leave the context's place in the launch order alone and queue nothing
    void refused_call(const Shape &c)
    {
        rt_ctx *x = ctx[c.k];
        CallerBuffers &b = bufs[c.s];
        const bool launched = x->launched, timing = x->have_timing;
        const hipStream_t last = x->last_stream;
        const long ops = g_ops;
        const int pending = x->pipe.pending;
        rt_camera cam = cam_of(c), bad = cam;
        bad.width = 0;
        const rt_render_settings rs = settings(2);
        rt_scene *other = n_ctx > 1 ? plain[1 - c.k] : nullptr;
        rt_denoise_params dp;
        rt_denoise_params_default(&dp);
        dp.iterations = 99;
        rt_adaptive_params ap;
        rt_adaptive_params_default(&ap);
        ap.step_spp = 0;
        rt_tile_spec bands = rt_sched::whole_image_spec();
        bands.band_stride = 2;
        const int32_t t1[1] = {1};
        rt_status st = RT_OK;
        g_call = "a refused call";
        switch (pick(0, 20)) {
            case 0: st = rt_render_device(x, scene_of(c), &bad, &rs, 1, 0, nullptr, nullptr, b.frame, streams[c.s]); break;
            case 1: st = rt_render_device(x, other, &cam, &rs, 1, 0, nullptr, nullptr, b.frame, streams[c.s]); break;
            case 2: st = rt_render_device_batch(x, scene_of(c), &cam, &rs, t1, 33, 0, nullptr, b.frame, streams[c.s]); break;
            case 3: st = rt_trace_rays_device(x, scene_of(c), nullptr, b.directions, 5, b.hits, streams[c.s]); break;
            case 4: st = rt_occluded_rays_device(x, scene_of(c), b.origins, b.directions, nullptr, -1, b.occluded, streams[c.s]); break;
            case 5: st = rt_render_ao_device(x, scene_of(c), &cam, 0, 1.0f, 0.0f, 1, b.ao_count, b.ao, streams[c.s]); break;
            case 6: st = rt_denoise_device(x, c.w, c.h, b.frame, b.normal, b.depth, nullptr, nullptr, &dp, b.denoised, streams[c.s]); break;
            case 7: st = rt_adaptive_plan_device(x, c.w, c.h, b.half_a, b.half_b, b.count, &ap, b.budget, b.tile_error, b.tile_active, streams[c.s]); break;
            case 8: st = rt_render_budget_device(x, scene_of(c), &cam, &rs, 1, &bands, b.budget, nullptr, b.frame, streams[c.s]); break;
            case 9: st = rt_render_views_device(x, scene_of(c), &cam, t1, 0, &rs, 0, 0, b.frames, streams[c.s]); break;
            case 10: st = rt_render_visibility_device(x, scene_of(c), &cam, nullptr, 0.0f, b.visibility, streams[c.s]); break;
            case 11: st = rt_render_sky_device(x, scene_of(c), nullptr, &cam, t1, 1, &rs, 0, 0, b.frames, streams[c.s]); break;
            case 12: st = rt_scene_update_mesh_device(x, mesh[c.k], 0, b.triangles, MESH_TRIS + 1, streams[c.s]); break;
            case 13: st = rt_nearest_points_device(x, scene_of(c), b.origins, nullptr, 5, nullptr, streams[c.s]); break;
            case 14: st = rt_trace_rays_multi_device(x, scene_of(c), b.origins, b.directions, nullptr, 5, RT_MULTIHIT_MAX + 1, b.multi_hits, b.counts, streams[c.s]); break;
            case 15: st = rt_winding_numbers_device(x, scene_of(c), b.origins, 5, 99, b.winding, nullptr, streams[c.s]); break;
            case 16: st = rt_signed_distance_device(x, scene_of(c), b.origins, nullptr, 5, (rt_nearest *)((char *)b.nearest + 8), b.sdf, streams[c.s]); break;
            case 17: st = rt_sweep_spheres_device(x, scene_of(c), b.origins, b.directions, nullptr, nullptr, 5, b.sweeps, streams[c.s]); break;
            case 18: st = rt_overlap_boxes_device(x, scene_of(c), b.origins, b.directions, 5, 0, nullptr, nullptr, nullptr, streams[c.s]); break;
            case 19: st = rt_overlap_triangles_device(x, scene_of(c), b.query_tris, 5, 0, nullptr, b.counts, nullptr, b.segments, streams[c.s]); break;
            default: st = rt_tiles_copy_device(x, b.compact, b.frame, c.w, c.h, nullptr, 3, 1, streams[c.s]); break;
        }
        refused++;
        if (st == RT_OK) violation("a call with bad arguments was accepted");
        if (x->launched != launched || x->last_stream != last || x->have_timing != timing || x->pipe.pending != pending)
            violation("a refused call moved the context's place in the launch order (launched / last_stream / have_timing / pending frames)");
        if (g_ops != ops) violation("a refused call queued %ld operations", g_ops - ops);
    }

    Shape shape(int k, int s, bool with_mesh, int w = 72, int h = 40) { return Shape{k, s, w, h, with_mesh}; }

    // ---- the fixed sequences: tests/test_gpu_streams.py's cases (c), (d), (e), here without a sleep - nothing ever completes on its own, so every
    // call is "pending" until the host waits
    void fixed_sequences()
    {
        for (int m = 0; m < 2; m++) {
            const bool mm = m != 0;
            const Shape a = shape(0, 1, mm), b = shape(0, 2, mm), big = shape(0, 2, mm, MAX_W, MAX_H), small = shape(0, 1, mm, 24, 16);
            // (c) another stream, same context: a pair per shared piece of scratch
            render_device(a, 0, 4); trace_rays(b, MAX_RAYS);                                         // ticket counter
            render_views(a, 3, true, 0.0f); render_batch(b, 0, 2); render_views(a, 2, true, 0.0f);  // per-frame planes
            render_views(a, 3, false, 0.0f); render_views(b, 2, false, 0.5f);                        // camera table and its upload
            denoise(a, false); denoise(small, true); denoise(big, false);                            // denoise records
            render_budget(a, 0, true); tiles_copy(b, 1, true); render_device(b, 2, 2);               // tile-list cache
            tiles_copy(b, 0, false); tiles_copy(b, 2, true); tiles_copy(b, 4, true);                 // ... whose entries are recycled under the pending launches
            render_ao(a); occluded_rays(b, 777, true); render_visibility(a);
            adaptive_plan(a); render_budget(b, -1, false);
            nearest_points(a, 900, true); trace_multi(b, m, 500, 3, true);                           // the ticket counter again, through the later families
            trace_multi(a, 2, MAX_MULTI, RT_MULTIHIT_MAX, false); trace_multi(b, 2, 200, 0, true); winding_numbers(a, 700, true, 3);
            // a sweep behind and ahead of a nearest-surface call on its stream, and of a signed-distance call on the other one: the sweep's two
            // launches and the signed distance's two hand their records on through the context's one buffer, which the growing counts regrow
            nearest_points(a, 300, true); sweep_spheres(a, 300, true); nearest_points(a, 350, false);
            signed_distance(b, 400, false, true); sweep_spheres(a, 500, false); signed_distance(b, 450, false, false);
            overlap_boxes(b, 300, 0, 2); overlap_boxes(a, MAX_MULTI, RT_OVERLAP_MAX, 3);             // (k == 0 and the bytes alone: any-only)
            overlap_triangles(b, 200, 4, 1, true); overlap_triangles(a, 100, 0, 2, false); sweep_spheres(b, 64, true);
            signed_distance(b, 600, false, true); signed_distance(a, MAX_RAYS, false, false);        // the context's records, regrown under the pending pair
            signed_distance(b, 100, true, true); winding_numbers(b, 50, false, 2);
            render_sky(a, 3, true, 0.0f); render_sky(b, 2, false, 0.5f); render_views(a, 2, false, 0.0f);
            // the cull plane of the mesh scene's view: computed, reused on its stream, reused on another, stale after an update; and the scene
            // blob rewritten between launches that read it on other streams
            render_device(a, 0, 2); render_device(a, 0, 2); render_device(b, 0, 2); update_mesh(a); render_device(b, 0, 2);
            trace_rays(a, 300); update_mesh(b); nearest_points(a, 40, false); update_mesh(shape(0, 3, mm)); render_batch(b, 0, 2);
            render_aov(a); host_form(shape(0, 0, mm), 3);                                            // a device form, then the family's host form
            trace_rays(a, 100); host_form(shape(0, 0, mm), 2);
            render_views(a, 2, false, 0.0f); host_form(shape(0, 0, mm), 9);
            denoise(a, false); host_form(shape(0, 0, mm), 7);
            render_budget(a, 1, true); host_form(shape(0, 0, mm), 8);
            render_device(a, 0, 40); host_form(shape(0, 0, mm), 0);                                  // (40 spp: a mesh scene's new view runs a pilot)
            // (d) behind frames in flight
            REQUIRE(frame_submit(a, 4) && frame_submit(a, 4));
            const Shape third = shape(0, 3, mm);
            trace_rays(third, 500); denoise(third, false); render_budget(third, 0, true); render_views(third, 2, true, 0.0f); render_ao(third);
            update_mesh(third); signed_distance(third, 2000, false, false); trace_multi(third, 2, 64, 2, true); render_sky(third, 2, true, 0.0f);
            sweep_spheres(third, 700, true); overlap_boxes(third, 65, 2, 0); overlap_triangles(third, 129, RT_OVERLAP_MAX, 3, true);
            REQUIRE(frame_collect(0, 1, false) && frame_collect(0, 1, false));
            REQUIRE(frame_submit(a, 4));
            render_device(shape(0, 2, mm, 40, 24), 0, 40);                                           // another view while a frame is in flight
            REQUIRE(frame_collect(0, 2, false));
            // (e) regrow under pending work
            denoise(small, false); denoise(big, false);
            render_batch(small, 0, 2); render_batch(big, 0, 2);
            render_views(small, 2, true, 0.0f); render_views(big, 4, true, 0.0f);
            host_form(shape(0, 0, mm, 24, 16), 2); trace_rays(a, 50); host_form(shape(0, 0, mm), 2);
            g_call = "(the caller waits)";
            REQUIRE(hipDeviceSynchronize() == hipSuccess);
        }
    }

    void random_sequence(int iterations)
    {
        const int sizes[5][2] = {{72, 40}, {24, 16}, {MAX_W, MAX_H}, {37, 21}, {8, 8}};
        for (int it = 0; it < iterations; it++) {
            const int z = pick(0, 4);
            const Shape c = shape(pick(0, n_ctx - 1), pick(0, n_streams - 1), pick(0, 1) != 0, sizes[z][0], sizes[z][1]);
            const int spp = pick(0, 9) == 0 ? 40 : pick(1, 4);
            switch (pick(0, 32)) {
                case 0: case 1: render_device(c, pick(0, 6), spp); break;
                case 2: render_batch(c, pick(0, 1) ? 0 : pick(2, 6), spp); break;
                case 3: case 4: frame_submit(shape(c.k, c.s, c.mesh), spp); break;      // (one image size: the view stays, so frames overlap)
                case 5: case 6: frame_collect(c.k, c.s, pick(0, 5) == 0); break;
                case 7: render_views(c, pick(1, MAX_VIEWS), pick(0, 1) != 0, 0.1f * (float)pick(0, 3)); break;
                case 8: render_budget(c, pick(-1, 4), pick(0, 1) != 0); break;
                case 9: adaptive_plan(c); break;
                case 10: trace_rays(c, pick(1, MAX_RAYS)); break;
                case 11: render_aov(c); break;
                case 12: occluded_rays(c, pick(1, MAX_RAYS), pick(0, 1) != 0); break;
                case 13: render_visibility(c); break;
                case 14: render_ao(c); break;
                case 15: denoise(c, pick(0, 1) != 0); break;
                case 16: to_rgba8(c); break;
                case 17: tiles_copy(c, pick(0, 4), pick(0, 1) != 0); break;
                case 18: case 19: host_form(c, pick(0, 16)); break;
                case 20: case 21: refused_call(c); break;
                case 22: render_sky(c, pick(1, MAX_VIEWS), pick(0, 1) != 0, 0.1f * (float)pick(0, 3)); break;
                case 23: update_mesh(c); break;
                case 24: nearest_points(c, pick(1, MAX_RAYS), pick(0, 1) != 0); break;
                case 25: trace_multi(c, pick(0, 2), pick(1, MAX_MULTI), pick(0, 2) == 0 ? 0 : pick(1, RT_MULTIHIT_MAX), pick(0, 1) != 0); break;
                case 26: winding_numbers(c, pick(1, MAX_RAYS), pick(0, 1) != 0, pick(1, 3)); break;
                case 27: signed_distance(c, pick(1, MAX_RAYS), pick(0, 1) != 0, pick(0, 1) != 0); break;
                case 28: sweep_spheres(c, pick(1, MAX_RAYS), pick(0, 1) != 0); break;
                case 29: { const int k = pick(0, 2) == 0 ? 0 : pick(1, RT_OVERLAP_MAX); overlap_boxes(c, pick(1, MAX_MULTI), k, k > 0 ? pick(0, 3) : pick(1, 3)); break; }
                case 30: { const int k = pick(0, 2) == 0 ? 0 : pick(1, RT_OVERLAP_MAX); overlap_triangles(c, pick(1, MAX_MULTI), k, k > 0 ? pick(0, 3) : pick(1, 3), pick(0, 1) != 0); break; }
                case 31:
                    g_call = "(the caller waits for its stream)";
                    REQUIRE(hipStreamSynchronize(streams[c.s]) == hipSuccess);
                    break;
                default:
                    if (pick(0, 9) == 0) { destroy_ctx(c.k); create_ctx(c.k); }
                    else if (rt_frames_pending(ctx[c.k]) == 0) { g_call = "rt_frame_depth"; REQUIRE(rt_frame_depth(ctx[c.k], pick(1, RT_PIPELINE_DEPTH)) == RT_OK); }
                    break;
            }
        }
    }
};

}  // namespace

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const int iterations = argc > 2 ? std::atoi(argv[2]) : 2000;
    long calls = 0, refused = 0;
    {
        World w;
        w.rng.seed(seed);
        w.build_scenes();
        w.setup(4, 1);
        w.fixed_sequences();
        w.teardown();
        // the same pairs over two contexts (case (f)) and everything else at random: 1-3 caller streams beside the null stream, 1-2 contexts
        for (int round = 0; round < 4; round++) {
            w.setup(2 + (int)((seed + (unsigned)round) % 3u), 1 + round % 2);
            w.random_sequence(iterations / 4);
            w.teardown();
        }
        calls = w.calls;
        refused = w.refused;
        rt_scene_builder_destroy(w.b_plain);
        rt_scene_builder_destroy(w.b_mesh);
        rt_scene_builder_destroy(w.b_textured);
    }
    if (!g_allocs.empty()) violation("%zu allocations were never released", g_allocs.size());
    std::printf("launch order: %ld calls (%ld refused), %ld launches, %ld operations and %ld accesses logged, %ld buffers released on the strength of hipFree's wait, "
                "%ld tile-list entries recycled (%ld of them regrown)\n", calls, refused, g_launch_count, g_ops, g_accesses, g_frees_waited, g_lists_recycled, g_lists_regrown);
    if (g_violations) {
        std::printf("launch order: %ld violations\n", g_violations);
        return 3;
    }
    std::printf("launch order: no violation, sanitizers silent\n");
    return 0;
}
