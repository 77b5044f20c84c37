// multi_shim.cpp -- a recording runtime behind csrc/rt_multi.cpp: the 22 hip*, 7 nccl* and 22 rt_* functions that file calls, without a GPU
// (tests/tools/multi_calls_lab.py links it with rt_multi.cpp and multi_calls_main.cpp into one stand-alone program).
//
//   memory   device and pinned memory are host memory: every copy really copies (the sparse path reads its 16-byte headers back), every
//            ncclRecv copies what the ncclSend in front of it named, and every range is checked against its allocation
//   contexts rt_create / rt_local_rows / rt_max_local_rows keep the band-cyclic row rule (rank q owns the rows y with (y / band_rows) % world == q);
//            rt_pack_sparse writes the header { (3 * rank + 1) % (cap + 1), 0, 0, 0 }; every other rt_* call only logs
//   log      one line per call that enqueues, synchronises or sets a context's state: name, current device, then what it was given.  Streams,
//            events and buffers are numbered by FIRST USE in the log (buffers also carry their device and size), never by creation order or
//            address, and creating / releasing calls are not logged: setup and teardown may run in any order, but any change in what is enqueued,
//            on which stream, in which order, on which current device, with which offsets and sizes changes the log
//   ledger   every stream, event, allocation, communicator and context is released exactly once, on its own device, never used afterwards,
//            and only once every stream with work on it has been synchronised; communicators go first and streams last
//   failures "the k-th call of function F fails": shim_fail("F", k), or MULTI_SHIM_FAIL=F:k read by shim_reset
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mi355rt.h"

namespace {

enum Kind { MEM, PINNED, EVENT, STREAM, COMM, CTX };
const char *const KIND_NAME[] = {"memory", "pinned memory", "event", "stream", "communicator", "context"};

struct Obj { // what a handle of any kind points to; it outlives its release, so a later use is seen and not a wild read
    Kind kind;
    int device;
    size_t size = 0; // MEM, PINNED
    void *base = nullptr;
    bool alive = true, busy = false; // STREAM: work enqueued since the last hipStreamSynchronize
    int id = -1;                     // order of first use in the log
    uint32_t rank = 0;               // COMM, CTX
};

struct Shim {
    int n_devices = 4, device = 0;
    std::vector<std::unique_ptr<Obj>> objs;
    std::map<uintptr_t, Obj *> mem;                 // live allocations by base address
    std::vector<std::pair<uintptr_t, Obj *>> freed; // released ones (an address may come back: live ones are looked up first)
    struct External { uintptr_t base; size_t size; std::string name; };
    std::vector<External> external;
    int next_id[3] = {0, 0, 0}; // MEM + PINNED, EVENT, STREAM
    std::vector<std::string> log, bad;
    std::map<std::string, int> calls;
    std::string fail_fn;
    int fail_k = 0;
    bool torn = false; // a release has been seen: from here on nothing but releases
    bool comm_phase_over = false, stream_phase = false;
    std::deque<std::pair<const void *, size_t>> sends;
    std::string last_error;
} g;

void say(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g.log.push_back(buf);
}

void violation(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g.bad.push_back(buf);
}

bool injected(const char *fn)
{
    const int k = ++g.calls[fn];
    return g.fail_fn == fn && k == g.fail_k;
}

Obj *make(Kind kind, int device)
{
    g.objs.emplace_back(new Obj{kind, device});
    return g.objs.back().get();
}

// a stream / event / communicator / context handle is the address of its Obj
Obj *handle(const void *h, Kind kind, const char *fn)
{
    for (const auto &o : g.objs)
        if (o.get() == h && o->kind == kind) {
            if (!o->alive) violation("%s: uses a released %s", fn, KIND_NAME[kind]);
            return o.get();
        }
    violation("%s: %p is no %s of this runtime", fn, h, KIND_NAME[kind]);
    return nullptr;
}

std::string S(hipStream_t s, const char *fn, bool enqueues = true)
{
    if (!s) return "s-null";
    Obj *o = handle(s, STREAM, fn);
    if (!o) return "s?";
    if (o->id < 0) o->id = g.next_id[2]++;
    if (enqueues) o->busy = true;
    return "s#" + std::to_string(o->id);
}

std::string E(hipEvent_t e, const char *fn)
{
    Obj *o = handle(e, EVENT, fn);
    if (!o) return "e?";
    if (o->id < 0) o->id = g.next_id[1]++;
    return "e#" + std::to_string(o->id);
}

// "d<device>:<allocation bytes>#<first use>+<offset>" (pinned memory: "pin:..."), a registered caller buffer by its name, "null"
std::string B(const void *p, size_t bytes, const char *fn)
{
    if (!p) return "null";
    const uintptr_t a = (uintptr_t) p;
    auto it = g.mem.upper_bound(a);
    if (it != g.mem.begin()) {
        --it;
        Obj *o = it->second;
        if (a < it->first + o->size) {
            if (a + bytes > it->first + o->size) violation("%s: %zu bytes at offset %zu of an allocation of %zu", fn, bytes, (size_t) (a - it->first), o->size);
            if (o->id < 0) o->id = g.next_id[0]++;
            char buf[96];
            if (o->kind == PINNED) snprintf(buf, sizeof(buf), "pin:%zu#%d+%zu", o->size, o->id, (size_t) (a - it->first));
            else snprintf(buf, sizeof(buf), "d%d:%zu#%d+%zu", o->device, o->size, o->id, (size_t) (a - it->first));
            return buf;
        }
    }
    for (const auto &x : g.external)
        if (a >= x.base && a < x.base + x.size) {
            if (a + bytes > x.base + x.size) violation("%s: %zu bytes at offset %zu of the caller's %s (%zu bytes)", fn, bytes, (size_t) (a - x.base), x.name.c_str(), x.size);
            return x.name + "+" + std::to_string(a - x.base);
        }
    for (const auto &f : g.freed)
        if (a >= f.first && a < f.first + f.second->size) {
            violation("%s: uses released memory", fn);
            return "released";
        }
    violation("%s: %p is in no allocation of this runtime", fn, p);
    return "unknown";
}

bool readable(const std::string &name) { return name != "null" && name != "released" && name != "unknown"; }

// releases: exactly once, on the object's own device, behind a synchronise of every stream with work on it; communicators first, streams last
void release(Obj *o, const char *fn)
{
    if (!o) return;
    if (!o->alive) {
        violation("%s: a %s is released twice", fn, KIND_NAME[o->kind]);
        return;
    }
    if (!g.torn)
        for (const auto &s : g.objs)
            if (s->kind == STREAM && s->alive && s->busy) violation("%s: a %s is released while a stream has work that was never synchronised", fn, KIND_NAME[o->kind]);
    g.torn = true;
    if ((o->kind == MEM || o->kind == EVENT || o->kind == STREAM) && o->device != g.device)
        violation("%s: a %s of device %d is released with device %d current", fn, KIND_NAME[o->kind], o->device, g.device);
    if (o->kind == COMM && g.comm_phase_over) violation("%s: a communicator is released after contexts, memory or events", fn);
    if (o->kind != COMM) g.comm_phase_over = true;
    if (o->kind != STREAM && g.stream_phase) violation("%s: a %s is released after a stream", fn, KIND_NAME[o->kind]);
    if (o->kind == STREAM) g.stream_phase = true;
    o->alive = false;
}

hipError_t alloc(void **out, size_t bytes, Kind kind)
{
    void *p = calloc(bytes ? bytes : 1, 1);
    if (!p) return hipErrorOutOfMemory;
    Obj *o = make(kind, g.device);
    o->size = bytes;
    o->base = p;
    g.mem[(uintptr_t) p] = o;
    *out = p;
    return hipSuccess;
}

hipError_t unalloc(void *p, Kind kind, const char *fn)
{
    if (!p) return hipSuccess;
    auto it = g.mem.find((uintptr_t) p);
    if (it == g.mem.end() || it->second->kind != kind) {
        violation("%s: %p is no live %s", fn, p, KIND_NAME[kind]);
        return hipErrorInvalidValue;
    }
    release(it->second, fn);
    g.freed.emplace_back(it->first, it->second);
    g.mem.erase(it);
    free(p);
    return hipSuccess;
}

const char *kind_name(hipMemcpyKind k)
{
    return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : k == hipMemcpyHostToHost ? "H2H" : "default";
}

// host memory of the caller (an array handed to rt_set_scene_multi, the result of a _host call) is not checked; device and pinned memory is
std::string host_or_dev(const void *p, size_t bytes, bool is_host, const char *fn)
{
    if (!is_host) return B(p, bytes, fn);
    const uintptr_t a = (uintptr_t) p;
    auto it = g.mem.upper_bound(a);
    if (it != g.mem.begin() && a < std::prev(it)->first + std::prev(it)->second->size) return B(p, bytes, fn);
    for (const auto &x : g.external)
        if (a >= x.base && a < x.base + x.size) return B(p, bytes, fn);
    return "host";
}

#define FAIL_HIP(fn) \
    if (injected(fn)) return hipErrorUnknown

} // namespace

struct rt_ctx {
    Obj *obj;
    uint32_t width, height, rank, world, band_rows, format, n_objects;
    uint32_t local_rows() const
    {
        uint32_t n = 0;
        for (uint32_t y = 0; y < height; y++) n += (y / band_rows) % world == rank;
        return n;
    }
    uint32_t max_local_rows() const
    {
        uint32_t best = 0;
        for (uint32_t q = 0; q < world; q++) {
            uint32_t n = 0;
            for (uint32_t y = 0; y < height; y++) n += (y / band_rows) % world == q;
            best = n > best ? n : best;
        }
        return best;
    }
};

namespace {
std::vector<std::unique_ptr<rt_ctx>> g_ctx;

std::string C(const rt_ctx *c, const char *fn)
{
    if (!c || !handle(c->obj, CTX, fn)) return "ctx?";
    return "ctx[" + std::to_string(c->rank) + "]";
}
} // namespace

// ---- the lab's side ---------------------------------------------------------------------------------------------------------------------
extern "C" void shim_fail(const char *fn, int k)
{
    g.fail_fn = fn ? fn : "";
    g.fail_k = k;
    g.calls.clear();
}

extern "C" void shim_reset(int n_devices)
{
    for (auto &m : g.mem) free((void *) m.first);
    g = Shim();
    g_ctx.clear();
    g.n_devices = n_devices;
    if (const char *e = getenv("MULTI_SHIM_FAIL")) {
        const char *colon = strchr(e, ':');
        if (colon) {
            g.fail_fn.assign(e, colon);
            g.fail_k = atoi(colon + 1);
        }
    }
}

extern "C" void shim_external(const void *p, size_t bytes, const char *name) { g.external.push_back({(uintptr_t) p, bytes, name}); }

extern "C" void shim_note(const char *text) { g.log.push_back(text); }

extern "C" int shim_calls(const char *fn) { return g.calls[fn]; }

// the ledger's verdict as log lines; the number of complaints
extern "C" int shim_ledger(void)
{
    for (const auto &o : g.objs)
        if (o->alive) violation("a %s of device %d was never released", KIND_NAME[o->kind], o->device);
    if (!g.sends.empty() && g.fail_fn.empty()) violation("an ncclSend without its ncclRecv");
    if (g.bad.empty()) g.log.push_back("ledger: clean");
    for (const std::string &b : g.bad) g.log.push_back("ledger: " + b);
    return (int) g.bad.size();
}

extern "C" void shim_print(FILE *f) // (no file: the lines are dropped)
{
    for (const std::string &l : g.log)
        if (f) fprintf(f, "%s\n", l.c_str());
    g.log.clear();
}

// ---- hip --------------------------------------------------------------------------------------------------------------------------------
extern "C" {

const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorInvalidValue ? "invalid argument" : "injected failure"; }

hipError_t hipGetDeviceCount(int *n)
{
    FAIL_HIP("hipGetDeviceCount");
    *n = g.n_devices;
    return hipSuccess;
}

hipError_t hipGetDevice(int *d)
{
    FAIL_HIP("hipGetDevice");
    *d = g.device;
    return hipSuccess;
}

hipError_t hipSetDevice(int d)
{
    FAIL_HIP("hipSetDevice");
    if (d < 0 || d >= g.n_devices) return hipErrorInvalidValue;
    g.device = d;
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    FAIL_HIP("hipStreamCreateWithFlags");
    *s = (hipStream_t) make(STREAM, g.device);
    return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t s)
{
    release(handle(s, STREAM, "hipStreamDestroy"), "hipStreamDestroy");
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s)
{
    FAIL_HIP("hipStreamSynchronize");
    say("hipStreamSynchronize dev=%d %s", g.device, S(s, "hipStreamSynchronize", false).c_str());
    if (Obj *o = s ? handle(s, STREAM, "hipStreamSynchronize") : nullptr) o->busy = false;
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    FAIL_HIP("hipStreamWaitEvent");
    const std::string sn = S(s, "hipStreamWaitEvent"), en = E(e, "hipStreamWaitEvent");
    say("hipStreamWaitEvent dev=%d %s %s", g.device, sn.c_str(), en.c_str());
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    FAIL_HIP("hipEventCreateWithFlags");
    *e = (hipEvent_t) make(EVENT, g.device);
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *e)
{
    FAIL_HIP("hipEventCreate");
    *e = (hipEvent_t) make(EVENT, g.device);
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t e)
{
    release(handle(e, EVENT, "hipEventDestroy"), "hipEventDestroy");
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    FAIL_HIP("hipEventRecord");
    const std::string en = E(e, "hipEventRecord"), sn = S(s, "hipEventRecord");
    say("hipEventRecord dev=%d %s %s", g.device, en.c_str(), sn.c_str());
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t e)
{
    FAIL_HIP("hipEventSynchronize");
    say("hipEventSynchronize dev=%d %s", g.device, E(e, "hipEventSynchronize").c_str());
    return hipSuccess;
}

hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    FAIL_HIP("hipEventElapsedTime");
    const std::string an = E(a, "hipEventElapsedTime"), bn = E(b, "hipEventElapsedTime");
    say("hipEventElapsedTime dev=%d %s %s", g.device, an.c_str(), bn.c_str());
    *ms = 1.0f;
    return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t bytes)
{
    FAIL_HIP("hipMalloc");
    return alloc(p, bytes, MEM);
}

hipError_t hipFree(void *p) { return unalloc(p, MEM, "hipFree"); }

hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
    FAIL_HIP("hipHostMalloc");
    return alloc(p, bytes, PINNED);
}

hipError_t hipHostFree(void *p) { return unalloc(p, PINNED, "hipHostFree"); }

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    FAIL_HIP("hipMemcpyAsync");
    const std::string sn = S(s, "hipMemcpyAsync");
    const std::string dn = host_or_dev(dst, bytes, kind == hipMemcpyDeviceToHost, "hipMemcpyAsync"), rn = host_or_dev(src, bytes, kind == hipMemcpyHostToDevice, "hipMemcpyAsync");
    say("hipMemcpyAsync dev=%d %s dst=%s src=%s bytes=%zu %s", g.device, sn.c_str(), dn.c_str(), rn.c_str(), bytes, kind_name(kind));
    if (readable(dn) && readable(rn)) memmove(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    FAIL_HIP("hipMemcpy");
    const std::string dn = host_or_dev(dst, bytes, kind == hipMemcpyDeviceToHost, "hipMemcpy"), rn = host_or_dev(src, bytes, kind == hipMemcpyHostToDevice, "hipMemcpy");
    say("hipMemcpy dev=%d dst=%s src=%s bytes=%zu %s", g.device, dn.c_str(), rn.c_str(), bytes, kind_name(kind));
    if (readable(dn) && readable(rn)) memmove(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s)
{
    FAIL_HIP("hipMemcpy2DAsync");
    const std::string sn = S(s, "hipMemcpy2DAsync");
    const size_t dspan = height ? dpitch * (height - 1) + width : 0, sspan = height ? spitch * (height - 1) + width : 0;
    const std::string dn = B(dst, dspan, "hipMemcpy2DAsync"), rn = B(src, sspan, "hipMemcpy2DAsync");
    say("hipMemcpy2DAsync dev=%d %s dst=%s dpitch=%zu src=%s spitch=%zu width=%zu height=%zu %s", g.device, sn.c_str(), dn.c_str(), dpitch, rn.c_str(), spitch, width, height,
        kind_name(kind));
    if (readable(dn) && readable(rn))
        for (size_t y = 0; y < height; y++) memmove((char *) dst + y * dpitch, (const char *) src + y * spitch, width);
    return hipSuccess;
}

hipError_t hipMemcpyPeerAsync(void *dst, int ddev, const void *src, int sdev, size_t bytes, hipStream_t s)
{
    FAIL_HIP("hipMemcpyPeerAsync");
    const std::string sn = S(s, "hipMemcpyPeerAsync");
    const std::string dn = B(dst, bytes, "hipMemcpyPeerAsync"), rn = B(src, bytes, "hipMemcpyPeerAsync");
    say("hipMemcpyPeerAsync dev=%d %s dst=%s on %d src=%s on %d bytes=%zu", g.device, sn.c_str(), dn.c_str(), ddev, rn.c_str(), sdev, bytes);
    if (readable(dn) && readable(rn)) memmove(dst, src, bytes);
    return hipSuccess;
}

// ---- rccl -------------------------------------------------------------------------------------------------------------------------------
const char *ncclGetErrorString(ncclResult_t r) { return r == ncclSuccess ? "no error" : "injected failure"; }

ncclResult_t ncclCommInitAll(ncclComm_t *comms, int n, const int *devs)
{
    if (injected("ncclCommInitAll")) return ncclInternalError;
    for (int i = 0; i < n; i++) {
        Obj *o = make(COMM, devs[i]);
        o->rank = (uint32_t) i;
        comms[i] = (ncclComm_t) o;
    }
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t c)
{
    release(handle(c, COMM, "ncclCommDestroy"), "ncclCommDestroy");
    return ncclSuccess;
}

ncclResult_t ncclGroupStart(void)
{
    if (injected("ncclGroupStart")) return ncclInternalError;
    say("ncclGroupStart dev=%d", g.device);
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd(void)
{
    say("ncclGroupEnd dev=%d", g.device); // (logged even when it is the call that fails: the group was closed)
    if (injected("ncclGroupEnd")) return ncclInternalError;
    return ncclSuccess;
}

static std::string comm_name(ncclComm_t c, const char *fn)
{
    Obj *o = handle(c, COMM, fn);
    return o ? "comm[" + std::to_string(o->rank) + "]" : "comm?";
}

ncclResult_t ncclSend(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t c, hipStream_t s)
{
    if (injected("ncclSend")) return ncclInternalError;
    const std::string cn = comm_name(c, "ncclSend"), sn = S(s, "ncclSend"), bn = B(buf, count, "ncclSend");
    say("ncclSend dev=%d %s %s buf=%s bytes=%zu%s to %d", g.device, cn.c_str(), sn.c_str(), bn.c_str(), count, type == ncclInt8 ? "" : " (not int8)", peer);
    g.sends.emplace_back(readable(bn) ? buf : nullptr, count);
    return ncclSuccess;
}

ncclResult_t ncclRecv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t c, hipStream_t s)
{
    if (injected("ncclRecv")) return ncclInternalError;
    const std::string cn = comm_name(c, "ncclRecv"), sn = S(s, "ncclRecv"), bn = B(buf, count, "ncclRecv");
    say("ncclRecv dev=%d %s %s buf=%s bytes=%zu%s from %d", g.device, cn.c_str(), sn.c_str(), bn.c_str(), count, type == ncclInt8 ? "" : " (not int8)", peer);
    if (g.sends.empty()) {
        violation("ncclRecv: no ncclSend in front of it");
    } else {
        if (g.sends.front().second != count) violation("ncclRecv: %zu bytes for an ncclSend of %zu", count, g.sends.front().second);
        else if (g.sends.front().first && readable(bn)) memmove(buf, g.sends.front().first, count);
        g.sends.pop_front();
    }
    return ncclSuccess;
}

// ---- libmi355rt.so ----------------------------------------------------------------------------------------------------------------------
const char *rt_last_error(void) { return g.last_error.c_str(); }
void rt_set_last_error(const char *message) { g.last_error = message ? message : ""; }

#define FAIL_RT(fn)                                                \
    if (injected(fn)) {                                            \
        rt_set_last_error(fn ": injected failure");                \
        return RT_ERR_DEVICE;                                      \
    }

int rt_create(rt_ctx **out, const rt_scene_desc *scene, const rt_config *cfg)
{
    FAIL_RT("rt_create");
    if (hipSetDevice(cfg->device) != hipSuccess) return RT_ERR_DEVICE; // (the library's own rt_create leaves the context's device current too)
    g_ctx.emplace_back(new rt_ctx{make(CTX, cfg->device), scene->width, scene->height, cfg->rank, cfg->world, cfg->band_rows, cfg->format, scene->n_objects});
    g_ctx.back()->obj->rank = cfg->rank;
    *out = g_ctx.back().get();
    return RT_OK;
}

int rt_destroy(rt_ctx *c)
{
    if (!c) return RT_OK;
    release(handle(c->obj, CTX, "rt_destroy"), "rt_destroy");
    g.device = c->obj->device; // (rt_destroy makes the context's device current)
    return RT_OK;
}

int rt_local_rows(const rt_ctx *c, uint32_t *n)
{
    *n = c->local_rows();
    return RT_OK;
}

int rt_max_local_rows(const rt_ctx *c, uint32_t *n)
{
    *n = c->max_local_rows();
    return RT_OK;
}

size_t rt_sparse_msg_bytes(uint32_t format, uint32_t cap) { return ((16 + 4 * (size_t) cap + 15) & ~(size_t) 15) + (size_t) cap * 256 * (format == RT_FMT_RGBA8 ? 4 : 16); }

size_t rt_sparse_stamp_bytes(rt_ctx *c) { return 4 * (size_t) ((c->width + 15) / 16) * ((c->height + 15) / 16); }

static size_t pixel_bytes(const rt_ctx *c) { return c->format == RT_FMT_RGBA8 ? 4 : 16; }

int rt_render(rt_ctx *c, const double *, void *fb, void *stream, float *ms)
{
    FAIL_RT("rt_render");
    const std::string cn = C(c, "rt_render"), bn = B(fb, (size_t) c->local_rows() * c->width * pixel_bytes(c), "rt_render"), sn = S((hipStream_t) stream, "rt_render");
    say("rt_render dev=%d %s fb=%s %s%s", g.device, cn.c_str(), bn.c_str(), sn.c_str(), ms ? " timed" : "");
    return RT_OK;
}

int rt_pack_sparse(rt_ctx *c, const void *fb, void *msg, uint32_t cap, void *stream)
{
    FAIL_RT("rt_pack_sparse");
    const uint32_t count = (3u * c->rank + 1u) % (cap + 1u);
    const size_t used = rt_sparse_msg_bytes(c->format, cap) - (size_t) (cap - count) * 256 * pixel_bytes(c);
    const std::string cn = C(c, "rt_pack_sparse"), fn = B(fb, 0, "rt_pack_sparse"), mn = B(msg, used, "rt_pack_sparse"), sn = S((hipStream_t) stream, "rt_pack_sparse");
    say("rt_pack_sparse dev=%d %s fb=%s msg=%s cap=%u %s", g.device, cn.c_str(), fn.c_str(), mn.c_str(), cap, sn.c_str());
    if (readable(mn)) {
        const uint32_t head[4] = {count, 0u, 0u, 0u};
        memcpy(msg, head, sizeof(head));
    }
    return RT_OK;
}

int rt_assemble(rt_ctx *c, const void *gathered, void *full, void *stream)
{
    FAIL_RT("rt_assemble");
    const size_t slot = (size_t) c->max_local_rows() * c->width * pixel_bytes(c);
    const std::string cn = C(c, "rt_assemble"), gn = B(gathered, slot * c->world, "rt_assemble"), fn = B(full, (size_t) c->height * c->width * pixel_bytes(c), "rt_assemble"),
                      sn = S((hipStream_t) stream, "rt_assemble");
    say("rt_assemble dev=%d %s gathered=%s full=%s %s", g.device, cn.c_str(), gn.c_str(), fn.c_str(), sn.c_str());
    return RT_OK;
}

int rt_assemble_planes(rt_ctx *c, const void *gathered, size_t stride, void *full, uint32_t elem, void *stream)
{
    FAIL_RT("rt_assemble_planes");
    const std::string cn = C(c, "rt_assemble_planes"), gn = B(gathered, stride * c->world, "rt_assemble_planes"), fn = B(full, (size_t) c->height * c->width * elem, "rt_assemble_planes"),
                      sn = S((hipStream_t) stream, "rt_assemble_planes");
    say("rt_assemble_planes dev=%d %s gathered=%s stride=%zu full=%s elem=%u %s", g.device, cn.c_str(), gn.c_str(), stride, fn.c_str(), elem, sn.c_str());
    return RT_OK;
}

int rt_assemble_sparse(rt_ctx *c, const void *msgs, uint32_t cap, void *full, void *stream)
{
    FAIL_RT("rt_assemble_sparse");
    const std::string cn = C(c, "rt_assemble_sparse"), gn = B(msgs, rt_sparse_msg_bytes(c->format, cap) * c->world, "rt_assemble_sparse"),
                      fn = B(full, (size_t) c->height * c->width * pixel_bytes(c), "rt_assemble_sparse"), sn = S((hipStream_t) stream, "rt_assemble_sparse");
    say("rt_assemble_sparse dev=%d %s msgs=%s cap=%u full=%s %s", g.device, cn.c_str(), gn.c_str(), cap, fn.c_str(), sn.c_str());
    return RT_OK;
}

int rt_assemble_sparse_incremental(rt_ctx *c, const void *msgs, uint32_t cap, void *full, void *stamps, uint32_t tag, void *stream)
{
    FAIL_RT("rt_assemble_sparse_incremental");
    const std::string cn = C(c, "rt_assemble_sparse_incremental"), gn = B(msgs, rt_sparse_msg_bytes(c->format, cap) * c->world, "rt_assemble_sparse_incremental"),
                      fn = B(full, (size_t) c->height * c->width * pixel_bytes(c), "rt_assemble_sparse_incremental"),
                      tn = B(stamps, rt_sparse_stamp_bytes(c), "rt_assemble_sparse_incremental"), sn = S((hipStream_t) stream, "rt_assemble_sparse_incremental");
    say("rt_assemble_sparse_incremental dev=%d %s msgs=%s cap=%u full=%s stamps=%s tag=%u %s", g.device, cn.c_str(), gn.c_str(), cap, fn.c_str(), tn.c_str(), tag, sn.c_str());
    return RT_OK;
}

int rt_set_ssaa_threshold(rt_ctx *c, float tau)
{
    FAIL_RT("rt_set_ssaa_threshold");
    say("rt_set_ssaa_threshold dev=%d %s %g", g.device, C(c, "rt_set_ssaa_threshold").c_str(), tau);
    return RT_OK;
}

int rt_set_ssaa_geometry(rt_ctx *c, float min_cos)
{
    FAIL_RT("rt_set_ssaa_geometry");
    say("rt_set_ssaa_geometry dev=%d %s %g", g.device, C(c, "rt_set_ssaa_geometry").c_str(), min_cos);
    return RT_OK;
}

int rt_set_scene(rt_ctx *c, const rt_scene_update *u, void *stream)
{
    FAIL_RT("rt_set_scene");
    const std::string cn = C(c, "rt_set_scene"), sn = S((hipStream_t) stream, "rt_set_scene");
    const std::string a = B(u->coefs, 0, "rt_set_scene"), b = B(u->light_p, 0, "rt_set_scene"), d = B(u->reflection, 0, "rt_set_scene"), e = B(u->albedo, 0, "rt_set_scene"),
                      f = B(u->light_color, 0, "rt_set_scene");
    say("rt_set_scene dev=%d %s coefs=%s light_p=%s reflection=%s albedo=%s light_color=%s %s", g.device, cn.c_str(), a.c_str(), b.c_str(), d.c_str(), e.c_str(), f.c_str(), sn.c_str());
    return RT_OK;
}

int rt_set_scene_status(rt_ctx *c, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index)
{
    FAIL_RT("rt_set_scene_status");
    say("rt_set_scene_status dev=%d %s", g.device, C(c, "rt_set_scene_status").c_str());
    *applied = 2;
    *rejected = 0;
    *reason = 0;
    *index = 0;
    return RT_OK;
}

int rt_render_gbuffer(rt_ctx *c, const double *, int32_t *object, double *t, float *normal, void *stream, float *ms)
{
    FAIL_RT("rt_render_gbuffer");
    const size_t px = (size_t) c->local_rows() * c->width;
    const std::string cn = C(c, "rt_render_gbuffer"), on = B(object, px * 4, "rt_render_gbuffer"), tn = B(t, px * 8, "rt_render_gbuffer"), nn = B(normal, px * 16, "rt_render_gbuffer"),
                      sn = S((hipStream_t) stream, "rt_render_gbuffer");
    say("rt_render_gbuffer dev=%d %s object=%s t=%s normal=%s %s%s", g.device, cn.c_str(), on.c_str(), tn.c_str(), nn.c_str(), sn.c_str(), ms ? " timed" : "");
    if (ms) *ms = 1.0f;
    return RT_OK;
}

static std::string rect_name(const uint32_t *r)
{
    if (!r) return "all";
    char buf[64];
    snprintf(buf, sizeof(buf), "%u,%u,%u,%u", r[0], r[1], r[2], r[3]);
    return buf;
}

int rt_object_extents(rt_ctx *c, const double *, const uint32_t *rect, rt_object_extent *out, void *stream, float *ms)
{
    FAIL_RT("rt_object_extents");
    const std::string cn = C(c, "rt_object_extents"), on = B(out, sizeof(rt_object_extent) * c->n_objects, "rt_object_extents"), sn = S((hipStream_t) stream, "rt_object_extents");
    say("rt_object_extents dev=%d %s rect=%s out=%s %s%s", g.device, cn.c_str(), rect_name(rect).c_str(), on.c_str(), sn.c_str(), ms ? " timed" : "");
    return RT_OK;
}

int rt_object_extents_host(rt_ctx *c, const double *, const uint32_t *rect, rt_object_extent *, void *stream)
{
    FAIL_RT("rt_object_extents_host");
    const std::string cn = C(c, "rt_object_extents_host"), sn = S((hipStream_t) stream, "rt_object_extents_host");
    say("rt_object_extents_host dev=%d %s rect=%s %s", g.device, cn.c_str(), rect_name(rect).c_str(), sn.c_str());
    return RT_OK;
}

int rt_merge_object_extents(rt_ctx *c, const rt_object_extent *parts, uint32_t n_parts, rt_object_extent *out, void *stream)
{
    FAIL_RT("rt_merge_object_extents");
    const size_t bytes = sizeof(rt_object_extent) * c->n_objects;
    const std::string cn = C(c, "rt_merge_object_extents"), pn = B(parts, bytes * n_parts, "rt_merge_object_extents"), on = B(out, bytes, "rt_merge_object_extents"),
                      sn = S((hipStream_t) stream, "rt_merge_object_extents");
    say("rt_merge_object_extents dev=%d %s parts=%s n=%u out=%s %s", g.device, cn.c_str(), pn.c_str(), n_parts, on.c_str(), sn.c_str());
    return RT_OK;
}

} // extern "C"
