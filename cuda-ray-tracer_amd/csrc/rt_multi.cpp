// rt_multi.cpp -- several GPUs of one node behind ONE call (libmi355rt_multi.so; declared in include/mi355rt.h).
//
// The reference is single-GPU (src/update-cuda.cu:160-190); BASELINE.json's north star adds row tiling across the GPUs
// of a node with a gather to one GPU as the only exchange step.  This layer puts that underneath the
// update() boundary (include/update.h:6-8): one process, one context per (device, part), rows band-cyclic over all
// contexts, every device renders its parts on its own stream, finished parts travel to the root device over RCCL
// (ncclSend / ncclRecv in one group per part, xGMI point to point) on a second stream per device while the next part
// renders, and the root restores row order with rt_assemble.  No collective touches the rendering itself.
//
//   transport   distinct devices            RCCL: ncclCommInitAll over the device list, one communicator per device
//               the same device n times     device-to-device copies on the comm streams: the whole choreography (bands,
//                                           offsets, events, reassembly) on a one-GPU box, without RCCL
//               one device, SELF_EXCHANGE   RCCL with one rank that sends its rows to itself: the RCCL calls on a one-GPU box
//
// Everything is enqueue-only unless timing is requested; rt_multi_wait() / rt_multi_stream() order later work.  The exception is
// RT_MULTI_SPARSE: only tiles that are not pure background travel, and how many there are is only known once a context has
// rendered, so the host waits for each context's 16-byte message header before it enqueues that message's transfer.
//
// Beyond frames (DESIGN.md section 21 has the stream and event order of each call): scene updates on every context in its own frame
// order (rt_set_scene_multi), the root's context 0 for the queries that depend on no row ownership (rt_multi_query_ctx), and the
// G-buffer planes and object extents of all contexts gathered on the root (rt_render_gbuffer_multi, rt_object_extents_multi) and
// rebuilt / merged there by rt_planes.hip's two kernels.
//
// One copy of each rule ("Host code: one copy of each rule"): owning members (rt_multi_destroy synchronises and deletes), one Gather
// per gathered thing (frames, planes, extents), gather_part for a part's way to the root.  What is enqueued, on which stream and device and
// in which order, is pinned call by call for every layout by tests/test_multi_calls_host.py.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mi355rt.h"

// A weak reference: the recording runtime this file is also linked against without a GPU (tests/tools/multi_shim.cpp) holds the entry points of the
// recorded call orders, which were not extended by this one; libmi355rt.so always defines it.
extern "C" int rt_reorder_scene(rt_ctx *ctx, void *stream) __attribute__((weak));

namespace {

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    rt_set_last_error(buf);
    return code;
}

// a failed HIP call is RT_ERR_DEVICE and named by its own text -- or by `what`, the HIP call inside an owning member's alloc / create
#define M_TRY(what, call)                                                                               \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(e_)); \
    } while (0)
#define M_HIP(call) M_TRY(#call, call)
#define M_NCCL(call)                                                                                      \
    do {                                                                                                  \
        ncclResult_t r_ = (call);                                                                         \
        if (r_ != ncclSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #call, ncclGetErrorString(r_)); \
    } while (0)
// "run on device r": what follows is enqueued with device r of the list current.  Nothing is restored on the way -- every entry point
// leaves with the device it came with (DeviceRestore)
#define ON_DEVICE(r) M_HIP(hipSetDevice(m->dev[r]))

enum Transport { DIRECT = 0, LOCAL_COPY = 1, RCCL = 2 };

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// every entry point moves the calling thread from device to device; it leaves with the device it came with
struct DeviceRestore : NoCopy {
    int d = -1;
    DeviceRestore() { if (hipGetDevice(&d) != hipSuccess) d = -1; }
    ~DeviceRestore() { if (d >= 0) (void) hipSetDevice(d); }
};

// What the object owns, one wrapper per kind (the shapes of rt_capi.cpp's, plus the device: this layer has several).  Each converts to the raw handle.
template <typename H, hipError_t (*Release)(H)>
struct Owned : NoCopy { // a handle of device `dev`, which is current when it is created; to release it that device is made current again, and nothing is restored
    H h = nullptr;
    int device = -1;
    ~Owned()
    {
        if (!h) return;
        (void) hipSetDevice(device);
        (void) Release(h);
    }
    operator H() const { return h; }
};
struct DevMem : Owned<void *, hipFree> {
    hipError_t alloc(int dev, size_t bytes) { device = dev; return hipMalloc(&h, bytes); }
    char *at(size_t offset) const { return (char *) h + offset; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(int dev) { device = dev; return hipEventCreateWithFlags(&h, hipEventDisableTiming); }
    hipError_t create_timing(int dev) { device = dev; return hipEventCreate(&h); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(int dev) { device = dev; return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};
struct Pinned : NoCopy { // host memory
    void *p = nullptr;
    ~Pinned() { if (p) (void) hipHostFree(p); }
    hipError_t alloc(size_t bytes, unsigned flags) { return hipHostMalloc(&p, bytes, flags); }
};
struct Context : NoCopy {
    rt_ctx *c = nullptr;
    ~Context() { if (c) (void) rt_destroy(c); } // (rt_destroy makes the context's device current itself)
    operator rt_ctx *() const { return c; }
};
struct Comms : NoCopy { // ncclCommInitAll makes them all at once
    std::vector<ncclComm_t> c;
    ~Comms() { for (ncclComm_t x : c) if (x) (void) ncclCommDestroy(x); }
    ncclComm_t operator[](size_t r) const { return c[r]; }
};

struct Piece { // `bytes` of context q's, from its own device to the root's
    uint32_t q;
    const void *src;
    void *dst;
    size_t bytes;
};

constexpr size_t PLANE_ELEM[3] = {4, 8, 16};

// One gathered thing -- frames, G-buffer planes (three buffers each), extents: what context q writes travels from its own buffer to its slot on
// the root or, where it need not travel, is written into the slot directly.
struct Gather {
    std::vector<DevMem> local[3]; // [world] what context q writes, on its own device (no memory: it writes into its slot on the root)
    DevMem gathered[3];           // root device: [world] slots, rank-major
    size_t slot[3] = {0, 0, 0};   // bytes from slot to slot
    std::vector<Event> done, sent; // [world] context q has written its buffer; it has left the buffer
    Event arrived, assembled;      // root: every part is in its slot (frames and planes); the call's last kernel has read the slots
    bool ready = false, have_assembled = false;

    void lists(uint32_t world, int buffers) // (without their memory and events: whoever sets a Gather up creates them, and names them in its messages)
    {
        for (int k = 0; k < buffers; k++) local[k] = std::vector<DevMem>(world);
        done = std::vector<Event>(world);
        sent = std::vector<Event>(world);
    }
    char *slot_of(uint32_t q, int k = 0) const { return gathered[k].at((size_t) q * slot[k]); }
    void *target(uint32_t q, int k = 0) const { return local[k][q] ? local[k][q].h : slot_of(q, k); } // where context q writes
};

} // namespace

struct rt_multi {
    uint32_t n = 0, parts = 1, world = 1; // devices, parts per device, contexts = n * parts
    uint32_t width = 0, height = 0;
    size_t pixel_bytes = 16, slot_bytes = 0, full_bytes = 0;
    Transport transport = DIRECT;
    bool self_exchange = false;
    bool bandwise = false;            // RT_MULTI_BANDWISE: rows travel band by band straight to their place in the full frame; no rank-major slots, no rt_assemble
    bool sparse = false;              // RT_MULTI_SPARSE: every context packs its rows into a sparse message; only the used prefix travels
    uint32_t cap = 0;                 // sparse: tiles per message = the tiles of the largest context (no message can overflow)
    size_t msg_bytes = 0, head_bytes = 0, tile_bytes = 0; // sparse: message stride in the root's slots, header + id array, one tile
    uint32_t next_tag = 0;            // sparse: frame tag of the next incremental assembly into `full` (0 = repaint everything)
    uint64_t last_sent = 0, last_dense = 0; // rt_multi_last_transfer
    uint32_t band_rows = 16, max_rows = 0;
    std::vector<uint32_t> rows;       // [world] local rows of context q
    std::vector<int> dev;             // [n]
    void *last_full = nullptr;        // where the last frame went (rt_render_multi's root_full_fb, or `full`): what rt_multi_download reads
    bool in_flight_failed = false;    // a call failed after part of it had been enqueued: events, receive slots and scenes are in an unknown state
    uint32_t n_objects = 0, n_lights = 0;
    size_t sc_off[5] = {0, 0, 0, 0, 0}, sc_len[5] = {0, 0, 0, 0, 0};
    bool have_scene_event = false;
    std::vector<Piece> pieces;        // gather_part's list of the current part (reserved once: no allocation per call)
    // What the object owns, released in reverse order: communicators, contexts, memory and events, streams.
    std::vector<Stream> s_render, s_comm; // [n]
    Event ev_t0, ev_t1;
    // frames: the rows of context q (sparse: its message) and the root's [world] slots of max_local_rows rows (sparse: of one message) each
    Gather frames;
    DevMem full;                      // root device: [height][width] pixels
    std::vector<Event> ev_hdr;        // sparse: [world] the message header of context q has reached h_hdr
    Pinned h_hdr;                     // sparse: [world][4] message headers of the current frame
    DevMem stamps;                    // sparse: rt_assemble_sparse_incremental's stamps for `full`
    // rt_set_scene_multi: one pinned host copy of the five arrays (coefs, light_p, reflection, albedo, light_color back to back), one device copy per device
    Pinned h_scene;
    std::vector<DevMem> d_scene;      // [n]
    std::vector<Event> ev_scene;      // [n] behind the last update's last kernel on device r
    // rt_render_gbuffer_multi: plane k = object (4 bytes), t (8), normal (16); only owned rows travel, and a context without rows has no buffer
    Gather planes;
    // rt_object_extents_multi: [n_objects] records per context; `assembled` is "merged"
    Gather extents;
    DevMem extents_merged;            // the _host form's result on the root
    std::vector<Context> ctx;         // [world], context q = part * n + r lives on device r and is rank q of `world`
    Comms comm;                       // [n] (RCCL only)
};

namespace {

// any early return between the first enqueue of a call and its end leaves uploads / sends / receives / events half issued
struct CallGuard {
    rt_multi *m;
    bool armed, ok = false;
    ~CallGuard() { if (armed && !ok) m->in_flight_failed = true; }
};

int refuse_failed(const rt_multi *m, const char *who)
{
    if (!m->in_flight_failed) return RT_OK;
    return fail(RT_ERR_DEVICE, "%s: an earlier call on this object failed with part of it enqueued; destroy it and create a new one", who);
}

// do the rows (message, planes, records) of context q leave its device buffer for the root's?
bool travels(const rt_multi *m, uint32_t q)
{
    const uint32_t r = q % m->n;
    return m->transport == RCCL ? (r != 0 || m->self_exchange) : (m->transport == LOCAL_COPY && r != 0);
}

// `ms` of a timed entry point: the device time on the root's render stream between the two calls (timer_end waits for it); nothing when ms is null
int timer_begin(rt_multi *m, const float *ms)
{
    if (ms) M_HIP(hipEventRecord(m->ev_t0, m->s_render[0]));
    return RT_OK;
}

int timer_end(rt_multi *m, float *ms)
{
    if (!ms) return RT_OK;
    M_HIP(hipEventRecord(m->ev_t1, m->s_render[0]));
    M_HIP(hipEventSynchronize(m->ev_t1));
    M_HIP(hipEventElapsedTime(ms, m->ev_t0, m->ev_t1));
    return RT_OK;
}

// a failure inside an RCCL group still closes the group before the call returns; the first error is the one reported
int close_group(ncclResult_t in_group, uint32_t part, const char *what)
{
    const ncclResult_t closed = ncclGroupEnd();
    if (in_group != ncclSuccess) return fail(RT_ERR_DEVICE, "ncclSend / ncclRecv of part %u%s failed: %s", part, what, ncclGetErrorString(in_group));
    M_NCCL(closed);
    return RT_OK;
}

// m->pieces, one part's, go to the root on the comm streams while the next part renders: one RCCL group of send / receive pairs, or device
// copies on the senders' comm streams; then every sending context's "sent" event, for which the root's comm stream waits where the copy
// ran on another stream.  The pieces of one context are adjacent.  `what` completes "... of part p<what> failed".
int gather_part(rt_multi *m, Gather &g, uint32_t part, const char *what)
{
    const std::vector<Piece> &pc = m->pieces;
    if (m->transport == RCCL) {
        M_NCCL(ncclGroupStart());
        ncclResult_t in_group = ncclSuccess;
        for (size_t i = 0; i < pc.size() && in_group == ncclSuccess; i++) {
            const uint32_t r = pc[i].q % m->n;
            in_group = ncclSend(pc[i].src, pc[i].bytes, ncclInt8, 0, m->comm[r], m->s_comm[r]);
            if (in_group == ncclSuccess) in_group = ncclRecv(pc[i].dst, pc[i].bytes, ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
        }
        if (int rc = close_group(in_group, part, what)) return rc;
    } else {
        for (const Piece &c : pc) // (copies travel between entries of a list that repeats ONE device, and that device is current)
            M_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, m->s_comm[c.q % m->n]));
    }
    for (size_t i = 0; i < pc.size(); i++) {
        const uint32_t q = pc[i].q, r = q % m->n;
        if (i && pc[i - 1].q == q) continue;
        ON_DEVICE(r);
        M_HIP(hipEventRecord(g.sent[q], m->s_comm[r]));
        if (m->transport != RCCL) {
            ON_DEVICE(0);
            M_HIP(hipStreamWaitEvent(m->s_comm[0], g.sent[q], 0));
        }
    }
    return RT_OK;
}

// root: everything has arrived on its comm stream -> whatever follows on its render stream sees it
int arrived_on_root(rt_multi *m, Gather &g)
{
    ON_DEVICE(0);
    M_HIP(hipEventRecord(g.arrived, m->s_comm[0]));
    M_HIP(hipStreamWaitEvent(m->s_render[0], g.arrived, 0));
    return RT_OK;
}

} // namespace

extern "C" int rt_multi_destroy(rt_multi *m)
{
    if (!m) return RT_OK;
    DeviceRestore restore;
    for (size_t r = 0; r < m->s_render.size(); r++) { // nothing is released while a stream may still use it
        (void) hipSetDevice(m->dev[r]);
        if (m->s_render[r]) (void) hipStreamSynchronize(m->s_render[r]);
        if (m->s_comm[r]) (void) hipStreamSynchronize(m->s_comm[r]);
    }
    delete m;
    return RT_OK;
}

static int create_impl(rt_multi *m, const rt_scene_desc *sd, const int *devices, uint32_t n, uint32_t band_rows, uint32_t parts, uint32_t flags, uint32_t format)
{
    m->n = n;
    m->parts = parts;
    m->world = n * parts;
    m->width = sd->width;
    m->height = sd->height;
    m->pixel_bytes = format == RT_FMT_RGBA8 ? 4 : 16;
    m->self_exchange = (flags & RT_MULTI_SELF_EXCHANGE) != 0;
    m->bandwise = (flags & RT_MULTI_BANDWISE) != 0;
    m->sparse = (flags & RT_MULTI_SPARSE) != 0;
    m->band_rows = band_rows;
    m->n_objects = sd->n_objects;
    m->n_lights = sd->n_lights;
    m->dev.assign(devices, devices + n);
    bool all_same = true, all_distinct = true;
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = a + 1; b < n; b++) {
            if (devices[a] == devices[b]) all_distinct = false;
            else all_same = false;
        }
    if (n > 1 && !all_same && !all_distinct) return fail(RT_ERR_INVALID, "rt_create_multi: the device list must be all distinct (RCCL) or one device repeated (rehearsal on one GPU)");
    m->transport = n == 1 ? (m->self_exchange ? RCCL : DIRECT) : (all_distinct ? RCCL : LOCAL_COPY);

    m->pieces.reserve(3u * n);
    std::vector<Stream> render(n), comm(n); // (both lists exist before the object shows either: rt_multi_destroy walks them together)
    m->s_render = std::move(render);
    m->s_comm = std::move(comm);
    for (uint32_t r = 0; r < n; r++) {
        M_HIP(hipSetDevice(devices[r]));
        M_TRY("hipStreamCreateWithFlags(&m->s_render[r], hipStreamNonBlocking)", m->s_render[r].create(devices[r]));
        M_TRY("hipStreamCreateWithFlags(&m->s_comm[r], hipStreamNonBlocking)", m->s_comm[r].create(devices[r]));
    }
    Gather &g = m->frames;
    g.lists(m->world, 1);
    m->ctx = std::vector<Context>(m->world);
    m->ev_hdr = std::vector<Event>(m->world);
    for (uint32_t q = 0; q < m->world; q++) {
        const uint32_t r = q % n;
        rt_config cfg{};
        cfg.device = devices[r];
        cfg.rank = q;
        cfg.world = m->world;
        cfg.band_rows = band_rows;
        cfg.flags = flags & ~(RT_MULTI_SELF_EXCHANGE | RT_MULTI_BANDWISE | RT_MULTI_SPARSE);
        cfg.format = format;
        int rc = rt_create(&m->ctx[q].c, sd, &cfg);
        if (rc != RT_OK) return rc;
        M_HIP(hipSetDevice(devices[r]));
        M_TRY("hipEventCreateWithFlags(&m->ev_rendered[q], hipEventDisableTiming)", g.done[q].create(devices[r]));
        M_TRY("hipEventCreateWithFlags(&m->ev_sent[q], hipEventDisableTiming)", g.sent[q].create(devices[r]));
        if (m->sparse) M_TRY("hipEventCreateWithFlags(&m->ev_hdr[q], hipEventDisableTiming)", m->ev_hdr[q].create(devices[r]));
    }
    rt_max_local_rows(m->ctx[0], &m->max_rows);
    m->rows.assign(m->world, 0);
    for (uint32_t q = 0; q < m->world; q++) rt_local_rows(m->ctx[q], &m->rows[q]);
    if (m->bandwise && m->world == 1 && m->transport == DIRECT) m->bandwise = false; // (one context renders in place: nothing travels)
    if (m->sparse && m->world == 1 && m->transport == DIRECT) m->sparse = false;
    g.slot[0] = m->slot_bytes = (size_t) m->max_rows * sd->width * m->pixel_bytes;
    m->full_bytes = (size_t) sd->height * sd->width * m->pixel_bytes;
    M_HIP(hipSetDevice(devices[0]));
    M_TRY("hipMalloc(&m->full, m->full_bytes ? m->full_bytes : 16)", m->full.alloc(devices[0], m->full_bytes ? m->full_bytes : 16));
    if (m->sparse) {
        // one message per context, of one capacity for all (rt_assemble_sparse's stride): the tiles of the largest context
        m->cap = ((sd->width + 15u) / 16u) * ((m->max_rows + 15u) / 16u);
        g.slot[0] = m->msg_bytes = rt_sparse_msg_bytes(format, m->cap);
        m->tile_bytes = (size_t) 256u * m->pixel_bytes;
        m->head_bytes = m->msg_bytes - (size_t) m->cap * m->tile_bytes; // { count, overflow, 0, 0 } + ids[cap], padded to 16 bytes
        M_TRY("hipMalloc(&m->gathered, m->msg_bytes * m->world)", g.gathered[0].alloc(devices[0], m->msg_bytes * m->world));
        const size_t stamp_bytes = rt_sparse_stamp_bytes(m->ctx[0]);
        M_TRY("hipMalloc(&m->stamps, stamp_bytes ? stamp_bytes : 16)", m->stamps.alloc(devices[0], stamp_bytes ? stamp_bytes : 16));
        M_TRY("hipHostMalloc((void **) &m->h_hdr, sizeof(uint32_t) * 4u * m->world, hipHostMallocDefault)", m->h_hdr.alloc(sizeof(uint32_t) * 4u * m->world, hipHostMallocDefault));
    } else if ((m->world > 1 || m->transport == RCCL) && !m->bandwise) {
        M_TRY("hipMalloc(&m->gathered, m->slot_bytes * m->world + 16)", g.gathered[0].alloc(devices[0], m->slot_bytes * m->world + 16));
    }
    // rows (messages) that have to travel get a buffer on their own device; the others are rendered (packed) into their slot on the root
    for (uint32_t q = 0; q < m->world; q++) {
        const uint32_t r = q % n;
        if (!m->bandwise && !travels(m, q)) continue; // (bandwise: the root's own rows are strided in the frame too)
        M_HIP(hipSetDevice(devices[r]));
        if (m->sparse) M_TRY("hipMalloc(&m->msg[q], m->msg_bytes)", g.local[0][q].alloc(devices[r], m->msg_bytes));
        else M_TRY("hipMalloc(&m->local[q], m->slot_bytes ? m->slot_bytes : 16)", g.local[0][q].alloc(devices[r], m->slot_bytes ? m->slot_bytes : 16));
    }
    M_HIP(hipSetDevice(devices[0]));
    M_TRY("hipEventCreateWithFlags(&m->ev_gathered, hipEventDisableTiming)", g.arrived.create(devices[0]));
    M_TRY("hipEventCreateWithFlags(&m->ev_assembled, hipEventDisableTiming)", g.assembled.create(devices[0]));
    M_TRY("hipEventCreate(&m->ev_t0)", m->ev_t0.create_timing(devices[0]));
    M_TRY("hipEventCreate(&m->ev_t1)", m->ev_t1.create_timing(devices[0]));
    if (m->transport == RCCL) {
        m->comm.c.assign(n, nullptr);
        M_NCCL(ncclCommInitAll(m->comm.c.data(), (int) n, devices));
    }
    return RT_OK;
}

extern "C" int rt_create_multi(rt_multi **out, const rt_scene_desc *scene, const int *devices, uint32_t n_devices, uint32_t band_rows, uint32_t parts,
                               uint32_t flags, uint32_t format)
{
    if (!out || !scene || !devices) return fail(RT_ERR_INVALID, "rt_create_multi: null argument");
    *out = nullptr;
    if (n_devices == 0 || n_devices > 64) return fail(RT_ERR_INVALID, "rt_create_multi: %u devices", n_devices);
    if (parts == 0) parts = 1;
    if (parts > 16) return fail(RT_ERR_INVALID, "rt_create_multi: %u parts per device (at most 16)", parts);
    if (flags & RT_FLAG_SIMPLE) return fail(RT_ERR_INVALID, "rt_create_multi: not available with RT_FLAG_SIMPLE");
    if ((flags & RT_MULTI_SPARSE) && (flags & RT_MULTI_BANDWISE))
        return fail(RT_ERR_INVALID, "rt_create_multi: RT_MULTI_SPARSE and RT_MULTI_BANDWISE exclude each other (tiles travel as messages, or rows band by band)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_ERR_NO_DEVICE, "rt_create_multi: no HIP device available; this library has no CPU fallback");
    for (uint32_t r = 0; r < n_devices; r++)
        if (devices[r] < 0 || devices[r] >= ndev) return fail(RT_ERR_INVALID, "rt_create_multi: device %d out of range (%d devices)", devices[r], ndev);
    rt_multi *m = new (std::nothrow) rt_multi();
    if (!m) return fail(RT_ERR_NOMEM, "out of memory");
    DeviceRestore restore;
    int rc;
    try {
        rc = create_impl(m, scene, devices, n_devices, band_rows ? band_rows : 16, parts, flags, format);
    } catch (const std::bad_alloc &) {
        rc = fail(RT_ERR_NOMEM, "rt_create_multi: out of host memory");
    }
    if (rc != RT_OK) { // whatever exists of the object releases itself
        std::string keep = rt_last_error();
        rt_multi_destroy(m);
        rt_set_last_error(keep.c_str());
        return rc;
    }
    *out = m;
    return RT_OK;
}

// Every device renders part p on its render stream, into the context's own buffer once the previous frame's rows have left it, or straight into
// its slot on the root; the comm stream of the device waits for the rows.  m->pieces: the slots that travel whole (the dense frame's).
static int render_part(rt_multi *m, const double cam[16], uint32_t p)
{
    Gather &g = m->frames;
    m->pieces.clear();
    for (uint32_t r = 0; r < m->n; r++) {
        const uint32_t q = p * m->n + r;
        ON_DEVICE(r);
        if (g.local[0][q]) M_HIP(hipStreamWaitEvent(m->s_render[r], g.sent[q], 0));
        int rc = rt_render(m->ctx[q], cam, g.target(q), m->s_render[r], nullptr);
        if (rc != RT_OK) return rc;
        M_HIP(hipEventRecord(g.done[q], m->s_render[r]));
        M_HIP(hipStreamWaitEvent(m->s_comm[r], g.done[q], 0));
        if (g.local[0][q] && !m->bandwise) m->pieces.push_back({q, g.local[0][q], g.slot_of(q), m->slot_bytes});
    }
    return RT_OK;
}

// One device, several contexts or self-exchange, dense: every context's whole slot travels and rt_assemble restores row order.
static int frame_dense(rt_multi *m, const double cam[16], void *full)
{
    Gather &g = m->frames;
    // the root's receive slots are free again once the previous frame has been reassembled out of them
    if (g.have_assembled)
        for (uint32_t r = 0; r < m->n; r++) {
            ON_DEVICE(r);
            if (m->transport != RCCL || r == 0) M_HIP(hipStreamWaitEvent(m->s_comm[r], g.assembled, 0));
            if (r == 0 || m->transport == LOCAL_COPY) M_HIP(hipStreamWaitEvent(m->s_render[r], g.assembled, 0));
        }
    for (uint32_t p = 0; p < m->parts; p++) {
        if (int rc = render_part(m, cam, p)) return rc;
        // ... and part p travels on the comm streams while part p + 1 renders
        if (int rc = gather_part(m, g, p, "")) return rc;
    }
    if (int rc = arrived_on_root(m, g)) return rc;
    int rc = rt_assemble(m->ctx[0], g.gathered[0], full, m->s_render[0]);
    if (rc != RT_OK) return rc;
    M_HIP(hipEventRecord(g.assembled, m->s_render[0]));
    g.have_assembled = true;
    return RT_OK;
}

// RT_MULTI_SPARSE.  Every context renders into its own buffer (rt_render keeps the wave-per-block schedule, rt_render_sparse would not) and packs it
// into a message that holds all of its tiles.  All parts are enqueued first, so the devices keep rendering while the host waits for
// the headers; then each part's messages travel, exactly their used prefix, into the root's [world][msg_bytes] receive slots.
// Contexts whose rows need not travel pack straight into their slot on the root's render stream, behind the previous frame's
// reassembly out of it.
static int frame_sparse(rt_multi *m, const double cam[16], void *full, bool into_own, uint64_t *sent)
{
    Gather &g = m->frames;
    uint32_t *const h_hdr = (uint32_t *) m->h_hdr.p;
    if (g.have_assembled) // the receive slots are free again once the previous frame has been reassembled out of them
        for (uint32_t r = 0; r < m->n; r++)
            if (m->transport != RCCL || r == 0) {
                ON_DEVICE(r);
                M_HIP(hipStreamWaitEvent(m->s_comm[r], g.assembled, 0));
            }
    for (uint32_t p = 0; p < m->parts; p++)
        for (uint32_t r = 0; r < m->n; r++) {
            const uint32_t q = p * m->n + r;
            ON_DEVICE(r);
            if (g.local[0][q]) M_HIP(hipStreamWaitEvent(m->s_render[r], g.sent[q], 0)); // the previous frame's message has left this buffer
            int rc = rt_render(m->ctx[q], cam, nullptr, m->s_render[r], nullptr);
            if (rc == RT_OK) rc = rt_pack_sparse(m->ctx[q], nullptr, g.target(q), m->cap, m->s_render[r]);
            if (rc != RT_OK) return rc;
            M_HIP(hipMemcpyAsync(h_hdr + 4u * q, g.target(q), 16, hipMemcpyDeviceToHost, m->s_render[r]));
            M_HIP(hipEventRecord(m->ev_hdr[q], m->s_render[r]));
        }
    *sent = 0;
    for (uint32_t p = 0; p < m->parts; p++) {
        m->pieces.clear();
        for (uint32_t r = 0; r < m->n; r++) { // the host waits for this part's headers (not for the devices)
            const uint32_t q = p * m->n + r;
            M_HIP(hipEventSynchronize(m->ev_hdr[q]));
            const uint32_t count = h_hdr[4u * q], overflow = h_hdr[4u * q + 1u];
            if (overflow || count > m->cap) return fail(RT_ERR_DEVICE, "rt_render_multi: context %u packed %u tiles into a message of %u", q, count, m->cap);
            const size_t bytes = m->head_bytes + (size_t) count * m->tile_bytes;
            *sent += bytes;
            if (!g.local[0][q]) continue;
            ON_DEVICE(r);
            M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_hdr[q], 0));
            m->pieces.push_back({q, g.local[0][q], g.slot_of(q), bytes});
        }
        if (int rc = gather_part(m, g, p, "")) return rc;
    }
    // (the slots packed in place are on the root's render stream already)
    if (int rc = arrived_on_root(m, g)) return rc;
    int rc;
    if (!into_own) {
        rc = rt_assemble_sparse(m->ctx[0], g.gathered[0], m->cap, full, m->s_render[0]);
    } else { // the object's own buffer keeps the previous frame: only tiles that lost their content are repainted
        rc = rt_assemble_sparse_incremental(m->ctx[0], g.gathered[0], m->cap, full, m->stamps, m->next_tag, m->s_render[0]);
        if (rc == RT_OK) m->next_tag = m->next_tag >= 0xFFFFFFFEu ? 1u : m->next_tag + 1u;
    }
    if (rc != RT_OK) return rc;
    M_HIP(hipEventRecord(g.assembled, m->s_render[0]));
    g.have_assembled = true;
    return RT_OK;
}

// RT_MULTI_BANDWISE.  Rows go band by band straight to where they belong in the full frame ("band-wise ncclRecv straight into final
// row offsets"): band j of context q is rows (j W + q) B ... of the frame.  No rank-major receive slots and no reassembly pass over the
// frame on the root.  Between distinct devices: one ncclSend / ncclRecv pair per band, all bands of a part in one group; rows that are
// already on the root device (and every row in the one-GPU rehearsal) take ONE strided device copy per context -- a different operation
// from gather_part's, issued inside the same group and in rank order with the pairs, so this path keeps a loop of its own.
static int frame_bandwise(rt_multi *m, const double cam[16], void *full)
{
    Gather &g = m->frames;
    const size_t row_bytes = (size_t) m->width * m->pixel_bytes, band_bytes = row_bytes * m->band_rows;
    const size_t dst_pitch = band_bytes * m->world;
    const bool by_rccl = m->transport == RCCL;
    for (uint32_t p = 0; p < m->parts; p++) {
        if (int rc = render_part(m, cam, p)) return rc;
        if (by_rccl) M_NCCL(ncclGroupStart());
        ncclResult_t in_group = ncclSuccess;
        hipError_t copy_err = hipSuccess;
        for (uint32_t r = 0; r < m->n && in_group == ncclSuccess && copy_err == hipSuccess; r++) {
            const uint32_t q = p * m->n + r;
            const uint32_t full_bands = m->rows[q] / m->band_rows, tail_rows = m->rows[q] - full_bands * m->band_rows;
            const char *src0 = g.local[0][q].at(0);
            char *dst0 = (char *) full + (size_t) q * band_bytes; // context q's band j starts dst_pitch * j further on
            if (by_rccl && travels(m, q)) {
                for (uint32_t j = 0; j * m->band_rows < m->rows[q] && in_group == ncclSuccess; j++) {
                    const size_t bytes = j < full_bands ? band_bytes : (size_t) tail_rows * row_bytes;
                    in_group = ncclSend(src0 + (size_t) j * band_bytes, bytes, ncclInt8, 0, m->comm[r], m->s_comm[r]);
                    if (in_group == ncclSuccess) in_group = ncclRecv(dst0 + (size_t) j * dst_pitch, bytes, ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
                }
            } else { // same device as the frame: one strided copy (and one more for a last, shorter band)
                (void) hipSetDevice(m->dev[r]);
                if (full_bands) copy_err = hipMemcpy2DAsync(dst0, dst_pitch, src0, band_bytes, band_bytes, full_bands, hipMemcpyDeviceToDevice, m->s_comm[r]);
                if (copy_err == hipSuccess && tail_rows)
                    copy_err = hipMemcpyAsync(dst0 + (size_t) full_bands * dst_pitch, src0 + (size_t) full_bands * band_bytes, (size_t) tail_rows * row_bytes, hipMemcpyDeviceToDevice,
                                              m->s_comm[r]);
            }
        }
        if (by_rccl)
            if (int rc = close_group(in_group, p, "")) return rc;
        if (copy_err != hipSuccess) return fail(RT_ERR_DEVICE, "band copy of part %u failed: %s", p, hipGetErrorString(copy_err));
        for (uint32_t r = 0; r < m->n; r++) {
            const uint32_t q = p * m->n + r;
            ON_DEVICE(r);
            M_HIP(hipEventRecord(g.sent[q], m->s_comm[r]));
            if (r != 0 || !by_rccl) { // what ran on another comm stream than the root's: the root's comm stream waits for it
                ON_DEVICE(0);
                M_HIP(hipStreamWaitEvent(m->s_comm[0], g.sent[q], 0));
            }
        }
    }
    return arrived_on_root(m, g); // the frame is complete for whatever follows on the root's render stream
}

extern "C" int rt_render_multi(rt_multi *m, const double cam[16], void *root_full_fb, float *ms)
{
    if (!m || !cam) return fail(RT_ERR_INVALID, "rt_render_multi: null argument");
    if (int rc = refuse_failed(m, "rt_render_multi")) return rc;
    DeviceRestore restore;
    void *full = root_full_fb ? root_full_fb : m->full.h;
    CallGuard guard{m, true};
    ON_DEVICE(0);
    if (int rc = timer_begin(m, ms)) return rc;
    uint64_t sent = m->full_bytes; // the dense transports deliver every context's rows
    int rc;
    if (m->world == 1 && m->transport == DIRECT) rc = rt_render(m->ctx[0], cam, full, m->s_render[0], nullptr); // one device, one part: the frame is this context's rows
    else if (m->sparse) rc = frame_sparse(m, cam, full, !root_full_fb, &sent);
    else if (m->bandwise) rc = frame_bandwise(m, cam, full);
    else rc = frame_dense(m, cam, full);
    if (rc != RT_OK) return rc;
    if (int rc_t = timer_end(m, ms)) return rc_t;
    m->last_full = full;
    m->last_sent = sent;
    m->last_dense = m->full_bytes;
    guard.ok = true;
    return RT_OK;
}

extern "C" int rt_multi_wait(rt_multi *m)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_wait: null argument");
    DeviceRestore restore;
    ON_DEVICE(0);
    M_HIP(hipStreamSynchronize(m->s_render[0]));
    return RT_OK;
}

extern "C" void *rt_multi_fb(rt_multi *m) { return m ? m->full.h : nullptr; }

extern "C" void *rt_multi_stream(rt_multi *m) { return m ? (void *) m->s_render[0].h : nullptr; }

extern "C" int rt_multi_download(rt_multi *m, void *host_dst, size_t bytes)
{
    if (!m || !host_dst) return fail(RT_ERR_INVALID, "rt_multi_download: null argument");
    if (bytes > m->full_bytes) return fail(RT_ERR_INVALID, "rt_multi_download: %zu bytes requested, the frame holds %zu", bytes, m->full_bytes);
    DeviceRestore restore;
    ON_DEVICE(0);
    if (!m->last_full) return fail(RT_ERR_INVALID, "rt_multi_download: no frame has been rendered yet");
    M_HIP(hipStreamSynchronize(m->s_render[0]));
    M_HIP(hipMemcpy(host_dst, m->last_full, bytes, hipMemcpyDeviceToHost)); // (the caller's own buffer when the last frame was rendered into one)
    return RT_OK;
}

extern "C" int rt_multi_last_transfer(const rt_multi *m, uint64_t *bytes_sent, uint64_t *bytes_dense)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_last_transfer: null argument");
    if (bytes_sent) *bytes_sent = m->last_sent;
    if (bytes_dense) *bytes_dense = m->last_dense;
    return RT_OK;
}

extern "C" int rt_multi_set_ssaa_threshold(rt_multi *m, float tau)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_set_ssaa_threshold: null argument");
    for (rt_ctx *c : m->ctx) { // (every context refuses the same way: NaN, or no RT_FLAG_SSAA_ADAPTIVE -- the first one answers for all)
        const int rc = rt_set_ssaa_threshold(c, tau);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

extern "C" int rt_multi_set_ssaa_geometry(rt_multi *m, float min_cos)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_set_ssaa_geometry: null argument");
    for (rt_ctx *c : m->ctx) { // (as above: NaN, or no RT_FLAG_SSAA_GEOMETRY -- the first context answers for all)
        const int rc = rt_set_ssaa_geometry(c, min_cos);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

extern "C" int rt_multi_info(const rt_multi *m, uint32_t *n_contexts, uint32_t *transport)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_info: null argument");
    if (n_contexts) *n_contexts = m->world;
    if (transport) *transport = (uint32_t) m->transport;
    return RT_OK;
}

// ---- scene updates, G-buffer, extents and the query context ---------------------------------------------
// MI355RT_DEBUG_MULTI_FAIL=<q> (tests): rt_set_scene_multi fails on the host in front of context q, as a launch that fails there would
static int debug_fail_at()
{
    const char *e = getenv("MI355RT_DEBUG_MULTI_FAIL");
    return (e && *e) ? atoi(e) : -1;
}

extern "C" int rt_set_scene_multi(rt_multi *m, const rt_scene_update *host)
{
    if (!m || !host) return fail(RT_ERR_INVALID, "rt_set_scene_multi: null argument");
    if (int rc = refuse_failed(m, "rt_set_scene_multi")) return rc;
    const void *src[5] = {host->coefs, host->light_p, host->reflection, host->albedo, host->light_color};
    if (!src[0] && !src[1] && !src[2] && !src[3] && !src[4]) return fail(RT_ERR_INVALID, "rt_set_scene_multi: all five arrays are null");
    if (m->n_objects == 0u && (host->coefs || host->reflection || host->albedo)) return fail(RT_ERR_INVALID, "rt_set_scene_multi: an object array for a scene without objects");
    if (m->n_lights == 0u && (host->light_p || host->light_color)) return fail(RT_ERR_INVALID, "rt_set_scene_multi: a light array for a scene without lights");
    DeviceRestore restore;
    if (!m->h_scene.p) { // first use: the FP64 arrays first, so every array is aligned to its type
        const size_t no = m->n_objects, nl = m->n_lights;
        const size_t len[5] = {sizeof(double) * RT_NCOEF * no, sizeof(double) * 3 * nl, sizeof(float) * no, sizeof(float) * 3 * no, sizeof(float) * 3 * nl};
        size_t off = 0;
        for (int k = 0; k < 5; k++) {
            m->sc_off[k] = off;
            m->sc_len[k] = len[k];
            off += len[k];
        }
        m->d_scene = std::vector<DevMem>(m->n);
        m->ev_scene = std::vector<Event>(m->n);
        for (uint32_t r = 0; r < m->n; r++) {
            ON_DEVICE(r);
            M_TRY("hipMalloc((void **) &m->d_scene[r], off)", m->d_scene[r].alloc(m->dev[r], off));
            M_TRY("hipEventCreateWithFlags(&m->ev_scene[r], hipEventDisableTiming)", m->ev_scene[r].create(m->dev[r]));
        }
        M_TRY("hipHostMalloc((void **) &m->h_scene, off, hipHostMallocPortable)", m->h_scene.alloc(off, hipHostMallocPortable)); // (last: its presence says the rest exists)
    }
    if (m->have_scene_event) // the previous call's uploads and kernels have read the pinned block and the device copies
        for (uint32_t r = 0; r < m->n; r++) M_HIP(hipEventSynchronize(m->ev_scene[r]));
    for (int k = 0; k < 5; k++)
        if (src[k]) memcpy((char *) m->h_scene.p + m->sc_off[k], src[k], m->sc_len[k]);
    CallGuard guard{m, false};
    const int fail_at = debug_fail_at();
    for (uint32_t r = 0; r < m->n; r++) {
        ON_DEVICE(r);
        const DevMem &d = m->d_scene[r];
        for (int k = 0; k < 5; k++)
            if (src[k]) M_HIP(hipMemcpyAsync(d.at(m->sc_off[k]), (const char *) m->h_scene.p + m->sc_off[k], m->sc_len[k], hipMemcpyHostToDevice, m->s_render[r]));
        rt_scene_update u{};
        u.coefs = src[0] ? (const double *) d.at(m->sc_off[0]) : nullptr;
        u.light_p = src[1] ? (const double *) d.at(m->sc_off[1]) : nullptr;
        u.reflection = src[2] ? (const float *) d.at(m->sc_off[2]) : nullptr;
        u.albedo = src[3] ? (const float *) d.at(m->sc_off[3]) : nullptr;
        u.light_color = src[4] ? (const float *) d.at(m->sc_off[4]) : nullptr;
        for (uint32_t p = 0; p < m->parts; p++) {
            const uint32_t q = p * m->n + r;
            if ((int) q == fail_at) return fail(RT_ERR_DEVICE, "rt_set_scene_multi: MI355RT_DEBUG_MULTI_FAIL names context %u", q);
            const int rc = rt_set_scene(m->ctx[q], &u, m->s_render[r]);
            if (rc != RT_OK) return rc;
            guard.armed = true; // from here on the contexts may hold different scenes
        }
        ON_DEVICE(r);
        M_HIP(hipEventRecord(m->ev_scene[r], m->s_render[r]));
    }
    m->have_scene_event = true;
    guard.ok = true;
    return RT_OK;
}

// rt_reorder_scene on every context, device by device on its render stream: behind an earlier rt_set_scene_multi, in front of later frames
extern "C" int rt_reorder_scene_multi(rt_multi *m)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_reorder_scene_multi: null argument");
    if (int rc = refuse_failed(m, "rt_reorder_scene_multi")) return rc;
    if (!rt_reorder_scene) return fail(RT_ERR_DEVICE, "rt_reorder_scene_multi: this runtime has no rt_reorder_scene");
    DeviceRestore restore;
    CallGuard guard{m, false};
    for (uint32_t r = 0; r < m->n; r++) {
        ON_DEVICE(r);
        for (uint32_t p = 0; p < m->parts; p++) {
            const int rc = rt_reorder_scene(m->ctx[p * m->n + r], m->s_render[r]);
            if (rc != RT_OK) return rc;
            guard.armed = true; // from here on the contexts may hold different orders (no result depends on that, but a launch failed: the object is done)
        }
    }
    guard.ok = true;
    return RT_OK;
}

extern "C" int rt_multi_set_scene_status(rt_multi *m, uint64_t *applied, uint64_t *rejected, uint32_t *reason, uint32_t *index)
{
    if (!m) return fail(RT_ERR_INVALID, "rt_multi_set_scene_status: null argument");
    if (int rc = refuse_failed(m, "rt_multi_set_scene_status")) return rc;
    DeviceRestore restore;
    uint64_t a0 = 0, r0 = 0;
    uint32_t why0 = 0, idx0 = 0;
    for (uint32_t q = 0; q < m->world; q++) {
        uint64_t a = 0, r = 0;
        uint32_t why = 0, idx = 0;
        const int rc = rt_set_scene_status(m->ctx[q], &a, &r, &why, &idx);
        if (rc != RT_OK) return rc;
        if (q == 0) {
            a0 = a, r0 = r, why0 = why, idx0 = idx;
        } else if (a != a0 || r != r0 || why != why0 || idx != idx0) {
            m->in_flight_failed = true;
            return fail(RT_ERR_DEVICE, "rt_multi_set_scene_status: context %u reports %llu applied / %llu rejected (reason %u at index %u), context 0 %llu / %llu (reason %u at index %u)",
                        q, (unsigned long long) a, (unsigned long long) r, why, idx, (unsigned long long) a0, (unsigned long long) r0, why0, idx0);
        }
    }
    if (applied) *applied = a0;
    if (rejected) *rejected = r0;
    if (reason) *reason = why0;
    if (index) *index = idx0;
    return RT_OK;
}

extern "C" rt_ctx *rt_multi_query_ctx(rt_multi *m)
{
    if (!m) {
        (void) fail(RT_ERR_INVALID, "rt_multi_query_ctx: null argument");
        return nullptr;
    }
    return m->ctx[0];
}

// first use of rt_render_gbuffer_multi: events, the root's receive slots and the buffers of the contexts whose rows travel.  A failure half way leaves
// the object failed: what exists is released with the object, and nothing else may use it.
static int planes_setup(rt_multi *m)
{
    Gather &g = m->planes;
    if (g.ready) return RT_OK;
    CallGuard guard{m, true};
    g.lists(m->world, 3);
    for (int k = 0; k < 3; k++) g.slot[k] = (size_t) m->max_rows * m->width * PLANE_ELEM[k];
    for (uint32_t q = 0; q < m->world; q++) {
        ON_DEVICE(q % m->n);
        M_TRY("hipEventCreateWithFlags(&m->g_ev_rendered[q], hipEventDisableTiming)", g.done[q].create(m->dev[q % m->n]));
        M_TRY("hipEventCreateWithFlags(&m->g_ev_sent[q], hipEventDisableTiming)", g.sent[q].create(m->dev[q % m->n]));
        if (!travels(m, q) || m->rows[q] == 0u) continue; // (a context without rows renders and sends nothing)
        for (int k = 0; k < 3; k++)
            M_TRY("hipMalloc(&m->g_local[k][q], (size_t) m->rows[q] * m->width * PLANE_ELEM[k])", g.local[k][q].alloc(m->dev[q % m->n], (size_t) m->rows[q] * m->width * PLANE_ELEM[k]));
    }
    ON_DEVICE(0);
    for (int k = 0; k < 3; k++) M_TRY("hipMalloc(&m->g_gathered[k], m->g_slot[k] * m->world + 16)", g.gathered[k].alloc(m->dev[0], g.slot[k] * m->world + 16));
    M_TRY("hipEventCreateWithFlags(&m->g_ev_gathered, hipEventDisableTiming)", g.arrived.create(m->dev[0]));
    M_TRY("hipEventCreateWithFlags(&m->g_ev_assembled, hipEventDisableTiming)", g.assembled.create(m->dev[0]));
    g.ready = guard.ok = true;
    return RT_OK;
}

extern "C" int rt_render_gbuffer_multi(rt_multi *m, const double cam[16], int32_t *root_object, double *root_t, float *root_normal, float *ms)
{
    if (!m || !cam) return fail(RT_ERR_INVALID, "rt_render_gbuffer_multi: null argument");
    if (!root_object && !root_t && !root_normal) return fail(RT_ERR_INVALID, "rt_render_gbuffer_multi: all three planes are null");
    if (int rc = refuse_failed(m, "rt_render_gbuffer_multi")) return rc;
    DeviceRestore restore;
    void *root[3] = {root_object, root_t, root_normal};
    if (m->world == 1 && m->transport == DIRECT) { // one device, one part: the planes are this context's rows
        return rt_render_gbuffer(m->ctx[0], cam, root_object, root_t, root_normal, m->s_render[0], ms);
    }
    if (int rc = planes_setup(m)) return rc;
    Gather &g = m->planes;
    CallGuard guard{m, false};
    ON_DEVICE(0);
    if (int rc = timer_begin(m, ms)) return rc;
    // the root's receive slots and the travelling contexts' buffers are free again once the previous call's planes have been reassembled
    if (g.have_assembled)
        for (uint32_t r = 0; r < m->n; r++) {
            ON_DEVICE(r);
            M_HIP(hipStreamWaitEvent(m->s_comm[r], g.assembled, 0));
            M_HIP(hipStreamWaitEvent(m->s_render[r], g.assembled, 0));
        }
    for (uint32_t p = 0; p < m->parts; p++) {
        m->pieces.clear();
        for (uint32_t r = 0; r < m->n; r++) { // every device runs the pass for part p on its render stream, behind its scene updates and frames
            const uint32_t q = p * m->n + r;
            if (m->rows[q] == 0u) continue;
            ON_DEVICE(r);
            void *dst[3];
            for (int k = 0; k < 3; k++) dst[k] = root[k] ? g.target(q, k) : nullptr;
            const int rc = rt_render_gbuffer(m->ctx[q], cam, (int32_t *) dst[0], (double *) dst[1], (float *) dst[2], m->s_render[r], nullptr);
            if (rc != RT_OK) return rc; // (a per-context refusal: every context gives it, so the first one does, with nothing enqueued)
            guard.armed = true;
            M_HIP(hipEventRecord(g.done[q], m->s_render[r]));
            M_HIP(hipStreamWaitEvent(m->s_comm[r], g.done[q], 0));
            for (int k = 0; k < 3; k++) // (all three planes of a context have a buffer of their own, or none: only its owned rows travel)
                if (root[k] && g.local[k][q]) m->pieces.push_back({q, g.local[k][q], g.slot_of(q, k), (size_t) m->rows[q] * m->width * PLANE_ELEM[k]});
        }
        // ... and part p's rows travel on the comm streams while part p + 1 runs
        if (int rc = gather_part(m, g, p, "'s planes")) return rc;
    }
    // -> reassemble the requested planes on the root's render stream
    if (int rc = arrived_on_root(m, g)) return rc;
    guard.armed = true;
    for (int k = 0; k < 3; k++) {
        if (!root[k]) continue;
        const int rc = rt_assemble_planes(m->ctx[0], g.gathered[k], g.slot[k], root[k], (uint32_t) PLANE_ELEM[k], m->s_render[0]);
        if (rc != RT_OK) return rc;
    }
    M_HIP(hipEventRecord(g.assembled, m->s_render[0]));
    g.have_assembled = true;
    if (int rc = timer_end(m, ms)) return rc;
    guard.ok = true;
    return RT_OK;
}

// first use of the extents calls: [world][n_objects] records on the root, and the records of the contexts whose results travel (as planes_setup)
static int extents_setup(rt_multi *m)
{
    Gather &g = m->extents;
    if (g.ready) return RT_OK;
    CallGuard guard{m, true};
    g.slot[0] = sizeof(rt_object_extent) * (size_t) m->n_objects;
    g.lists(m->world, 1);
    for (uint32_t q = 0; q < m->world; q++) {
        ON_DEVICE(q % m->n);
        M_TRY("hipEventCreateWithFlags(&m->x_ev_done[q], hipEventDisableTiming)", g.done[q].create(m->dev[q % m->n]));
        M_TRY("hipEventCreateWithFlags(&m->x_ev_sent[q], hipEventDisableTiming)", g.sent[q].create(m->dev[q % m->n]));
        if (travels(m, q)) M_TRY("hipMalloc(&m->x_local[q], bytes)", g.local[0][q].alloc(m->dev[q % m->n], g.slot[0]));
    }
    ON_DEVICE(0);
    M_TRY("hipMalloc(&m->x_parts, bytes * m->world)", g.gathered[0].alloc(m->dev[0], g.slot[0] * m->world));
    M_TRY("hipMalloc(&m->x_merged, bytes)", m->extents_merged.alloc(m->dev[0], g.slot[0]));
    M_TRY("hipEventCreateWithFlags(&m->x_ev_merged, hipEventDisableTiming)", g.assembled.create(m->dev[0]));
    g.ready = guard.ok = true;
    return RT_OK;
}

// Not gather_part: the records go by a peer copy also between distinct devices (no RCCL group for 40 bytes per object), and it is the root's RENDER
// stream that waits for every copy -- the merge runs there, and no comm stream of the root is involved.
static int extents_multi(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *root_dev_out, float *ms)
{
    if (m->n_objects == 0u) { // (a scene without objects: the contexts enqueue nothing, and neither does the merge)
        const int rc = rt_object_extents(m->ctx[0], cam, rect, root_dev_out, m->s_render[0], nullptr); // ... but they still refuse what they refuse
        if (rc == RT_OK && ms) *ms = 0.0f;
        return rc;
    }
    if (int rc = extents_setup(m)) return rc;
    Gather &g = m->extents;
    CallGuard guard{m, false};
    ON_DEVICE(0);
    if (int rc = timer_begin(m, ms)) return rc;
    if (g.have_assembled) // the previous call's merge has read the root's records, hence every copy has left its context's buffer
        for (uint32_t r = 0; r < m->n; r++) {
            ON_DEVICE(r);
            M_HIP(hipStreamWaitEvent(m->s_render[r], g.assembled, 0));
        }
    for (uint32_t p = 0; p < m->parts; p++)
        for (uint32_t r = 0; r < m->n; r++) {
            const uint32_t q = p * m->n + r;
            ON_DEVICE(r);
            const int rc = rt_object_extents(m->ctx[q], cam, rect, (rt_object_extent *) g.target(q), m->s_render[r], nullptr);
            if (rc != RT_OK) return rc; // (a per-context refusal: the first context gives it, with nothing enqueued)
            guard.armed = true;
            if (!g.local[0][q]) continue; // written in place on the root's render stream
            M_HIP(hipEventRecord(g.done[q], m->s_render[r]));
            M_HIP(hipStreamWaitEvent(m->s_comm[r], g.done[q], 0));
            if (m->dev[r] == m->dev[0]) M_HIP(hipMemcpyAsync(g.slot_of(q), g.local[0][q], g.slot[0], hipMemcpyDeviceToDevice, m->s_comm[r]));
            else M_HIP(hipMemcpyPeerAsync(g.slot_of(q), m->dev[0], g.local[0][q], m->dev[r], g.slot[0], m->s_comm[r]));
            M_HIP(hipEventRecord(g.sent[q], m->s_comm[r]));
            ON_DEVICE(0);
            M_HIP(hipStreamWaitEvent(m->s_render[0], g.sent[q], 0));
        }
    ON_DEVICE(0);
    const int rc = rt_merge_object_extents(m->ctx[0], (const rt_object_extent *) g.gathered[0].h, m->world, root_dev_out, m->s_render[0]);
    if (rc != RT_OK) return rc;
    M_HIP(hipEventRecord(g.assembled, m->s_render[0]));
    g.have_assembled = true;
    if (int rc_t = timer_end(m, ms)) return rc_t;
    guard.ok = true;
    return RT_OK;
}

extern "C" int rt_object_extents_multi(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *root_dev_out, float *ms)
{
    if (!m || !cam || !root_dev_out) return fail(RT_ERR_INVALID, "rt_object_extents_multi: null argument");
    if ((uintptr_t) root_dev_out & 7u) return fail(RT_ERR_INVALID, "rt_object_extents_multi: the output must be 8-byte aligned");
    if (int rc = refuse_failed(m, "rt_object_extents_multi")) return rc;
    DeviceRestore restore;
    return extents_multi(m, cam, rect, root_dev_out, ms);
}

extern "C" int rt_object_extents_multi_host(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *out_host)
{
    if (!m || !cam || !out_host) return fail(RT_ERR_INVALID, "rt_object_extents_multi_host: null argument");
    if (int rc = refuse_failed(m, "rt_object_extents_multi_host")) return rc;
    DeviceRestore restore;
    if (m->n_objects == 0u) return rt_object_extents_host(m->ctx[0], cam, rect, out_host, m->s_render[0]); // (nothing to merge; it still refuses what it refuses)
    if (int rc = extents_setup(m)) return rc; // (extents_merged exists from here on)
    // extents_merged is read by the blocking copy below before this call returns, so no later call can overwrite it early
    if (int rc = extents_multi(m, cam, rect, (rt_object_extent *) m->extents_merged.h, nullptr)) return rc;
    ON_DEVICE(0);
    M_HIP(hipMemcpyAsync(out_host, m->extents_merged, sizeof(rt_object_extent) * (size_t) m->n_objects, hipMemcpyDeviceToHost, m->s_render[0]));
    M_HIP(hipStreamSynchronize(m->s_render[0]));
    return RT_OK;
}
