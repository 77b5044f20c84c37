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
// Beyond frames (the second half of this file; DESIGN.md section 21 has the stream and event order of each call): scene updates on every
// context in its own frame order (rt_set_scene_multi), the root's context 0 for the queries that depend on no row ownership
// (rt_multi_query_ctx), and the G-buffer planes and object extents of all contexts gathered on the root with the dense frame's
// choreography (rt_render_gbuffer_multi, rt_object_extents_multi) and rebuilt / merged there by rt_planes.hip's two kernels.
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

#define M_HIP(call)                                                                                      \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define M_NCCL(call)                                                                                      \
    do {                                                                                                  \
        ncclResult_t r_ = (call);                                                                         \
        if (r_ != ncclSuccess) return fail(RT_ERR_DEVICE, "%s failed: %s", #call, ncclGetErrorString(r_)); \
    } while (0)

enum Transport { DIRECT = 0, LOCAL_COPY = 1, RCCL = 2 };

// every entry point moves the calling thread from device to device; it leaves with the device it came with
struct DeviceRestore {
    int d = -1;
    DeviceRestore() { if (hipGetDevice(&d) != hipSuccess) d = -1; }
    ~DeviceRestore() { if (d >= 0) (void) hipSetDevice(d); }
    DeviceRestore(const DeviceRestore &) = delete;
    DeviceRestore &operator=(const DeviceRestore &) = delete;
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
    size_t msg_bytes = 0, head_bytes = 0, tile_bytes = 0; // sparse: message stride in `gathered`, header + id array, one tile
    std::vector<void *> msg;          // sparse: [world] message of context q on its own device (NULL: it packs straight into its receive slot)
    std::vector<hipEvent_t> ev_hdr;   // sparse: [world] the message header of context q has reached h_hdr
    uint32_t *h_hdr = nullptr;        // sparse: pinned host [world][4] message headers of the current frame
    void *stamps = nullptr;           // sparse: rt_assemble_sparse_incremental's stamps for `full`
    uint32_t next_tag = 0;            // sparse: frame tag of the next incremental assembly into `full` (0 = repaint everything)
    uint64_t last_sent = 0, last_dense = 0; // rt_multi_last_transfer
    uint32_t band_rows = 16;
    std::vector<uint32_t> rows;       // [world] local rows of context q (bandwise)
    std::vector<int> dev;              // [n]
    std::vector<rt_ctx *> ctx;         // [world], context q = part * n + r lives on device r and is rank q of `world`
    std::vector<hipStream_t> s_render, s_comm; // [n]
    std::vector<void *> local;         // [world] rows of context q on its own device (NULL where it renders into the root's slot)
    std::vector<hipEvent_t> ev_rendered, ev_sent; // [world]
    std::vector<ncclComm_t> comm;      // [n] (RCCL only)
    void *gathered = nullptr;          // root device: [world][max_local_rows][width] pixels, rank-major
    void *full = nullptr;              // root device: [height][width] pixels
    hipEvent_t ev_gathered = nullptr, ev_assembled = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    bool have_assembled = false;
    void *last_full = nullptr;         // where the last frame went (rt_render_multi's root_full_fb, or `full`): what rt_multi_download reads
    bool in_flight_failed = false;     // a frame failed after part of it had been enqueued: events and receive slots are in an unknown state
    // rt_set_scene_multi: one pinned host copy of the five arrays (coefs, light_p, reflection, albedo, light_color back to back), one device copy per device
    uint32_t n_objects = 0, n_lights = 0;
    size_t sc_off[5] = {0, 0, 0, 0, 0}, sc_len[5] = {0, 0, 0, 0, 0}, sc_bytes = 0;
    unsigned char *h_scene = nullptr;
    std::vector<unsigned char *> d_scene; // [n]
    std::vector<hipEvent_t> ev_scene;     // [n] behind the last update's last kernel on device r
    bool have_scene_event = false;
    // rt_render_gbuffer_multi: plane k = object (4 bytes), t (8), normal (16); the dense frame's choreography with events of its own
    std::vector<void *> g_local[3];       // [world] rows of context q that travel, on its own device (NULL where it renders into the root's slot)
    void *g_gathered[3] = {nullptr, nullptr, nullptr}; // root device: [world][max_local_rows][width] elements, rank-major
    size_t g_slot[3] = {0, 0, 0};
    std::vector<hipEvent_t> g_ev_rendered, g_ev_sent; // [world]
    hipEvent_t g_ev_gathered = nullptr, g_ev_assembled = nullptr;
    bool g_ready = false, g_have_assembled = false;
    uint32_t max_rows = 0;
    // rt_object_extents_multi: [world][n_objects] records on the root, the records of the contexts whose results travel on their own device
    std::vector<void *> x_local;          // [world]
    void *x_parts = nullptr, *x_merged = nullptr;
    std::vector<hipEvent_t> x_ev_done, x_ev_sent; // [world]
    hipEvent_t x_ev_merged = nullptr;
    bool x_ready = false, x_have_merged = false;
};

namespace {

// any early return between the first enqueue of a call and its end leaves uploads / sends / receives / events half issued
struct CallGuard {
    rt_multi *m;
    bool armed = false, ok = false;
    ~CallGuard() { if (armed && !ok) m->in_flight_failed = true; }
};

constexpr size_t PLANE_ELEM[3] = {4, 8, 16};

// do the rows (planes, records) of context q leave its device buffer for the root's, as the dense frame's do?
bool travels(const rt_multi *m, uint32_t q)
{
    const uint32_t r = q % m->n;
    return m->transport == RCCL ? (r != 0 || m->self_exchange) : (m->transport == LOCAL_COPY && r != 0);
}

} // namespace

extern "C" int rt_multi_destroy(rt_multi *m)
{
    if (!m) return RT_OK;
    DeviceRestore restore;
    for (uint32_t r = 0; r < m->n; r++) {
        (void) hipSetDevice(m->dev[r]);
        if (r < m->s_render.size() && m->s_render[r]) (void) hipStreamSynchronize(m->s_render[r]);
        if (r < m->s_comm.size() && m->s_comm[r]) (void) hipStreamSynchronize(m->s_comm[r]);
    }
    for (size_t r = 0; r < m->comm.size(); r++)
        if (m->comm[r]) (void) ncclCommDestroy(m->comm[r]);
    for (uint32_t q = 0; q < m->ctx.size(); q++) {
        const uint32_t r = q % m->n;
        (void) hipSetDevice(m->dev[r]);
        if (m->ctx[q]) (void) rt_destroy(m->ctx[q]);
        if (q < m->local.size() && m->local[q]) (void) hipFree(m->local[q]);
        if (q < m->ev_rendered.size() && m->ev_rendered[q]) (void) hipEventDestroy(m->ev_rendered[q]);
        if (q < m->ev_sent.size() && m->ev_sent[q]) (void) hipEventDestroy(m->ev_sent[q]);
        if (q < m->msg.size() && m->msg[q]) (void) hipFree(m->msg[q]);
        if (q < m->ev_hdr.size() && m->ev_hdr[q]) (void) hipEventDestroy(m->ev_hdr[q]);
        for (int k = 0; k < 3; k++)
            if (q < m->g_local[k].size() && m->g_local[k][q]) (void) hipFree(m->g_local[k][q]);
        if (q < m->x_local.size() && m->x_local[q]) (void) hipFree(m->x_local[q]);
        for (const std::vector<hipEvent_t> *v : {&m->g_ev_rendered, &m->g_ev_sent, &m->x_ev_done, &m->x_ev_sent})
            if (q < v->size() && (*v)[q]) (void) hipEventDestroy((*v)[q]);
    }
    for (uint32_t r = 0; r < m->n; r++) {
        (void) hipSetDevice(m->dev[r]);
        if (r < m->d_scene.size() && m->d_scene[r]) (void) hipFree(m->d_scene[r]);
        if (r < m->ev_scene.size() && m->ev_scene[r]) (void) hipEventDestroy(m->ev_scene[r]);
    }
    if (m->n) (void) hipSetDevice(m->dev[0]);
    if (m->gathered) (void) hipFree(m->gathered);
    if (m->full) (void) hipFree(m->full);
    if (m->stamps) (void) hipFree(m->stamps);
    if (m->h_hdr) (void) hipHostFree(m->h_hdr);
    if (m->h_scene) (void) hipHostFree(m->h_scene);
    for (void *p : {m->g_gathered[0], m->g_gathered[1], m->g_gathered[2], m->x_parts, m->x_merged})
        if (p) (void) hipFree(p);
    for (hipEvent_t e : {m->ev_gathered, m->ev_assembled, m->ev_t0, m->ev_t1, m->g_ev_gathered, m->g_ev_assembled, m->x_ev_merged})
        if (e) (void) hipEventDestroy(e);
    for (uint32_t r = 0; r < m->n; r++) {
        (void) hipSetDevice(m->dev[r]);
        if (r < m->s_render.size() && m->s_render[r]) (void) hipStreamDestroy(m->s_render[r]);
        if (r < m->s_comm.size() && m->s_comm[r]) (void) hipStreamDestroy(m->s_comm[r]);
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

    m->ctx.assign(m->world, nullptr);
    m->local.assign(m->world, nullptr);
    m->ev_rendered.assign(m->world, nullptr);
    m->ev_sent.assign(m->world, nullptr);
    m->msg.assign(m->world, nullptr);
    m->ev_hdr.assign(m->world, nullptr);
    m->s_render.assign(n, nullptr);
    m->s_comm.assign(n, nullptr);
    for (uint32_t r = 0; r < n; r++) {
        M_HIP(hipSetDevice(devices[r]));
        M_HIP(hipStreamCreateWithFlags(&m->s_render[r], hipStreamNonBlocking));
        M_HIP(hipStreamCreateWithFlags(&m->s_comm[r], hipStreamNonBlocking));
    }
    uint32_t max_rows = 0;
    for (uint32_t q = 0; q < m->world; q++) {
        const uint32_t r = q % n;
        rt_config cfg{};
        cfg.device = devices[r];
        cfg.rank = q;
        cfg.world = m->world;
        cfg.band_rows = band_rows;
        cfg.flags = flags & ~(RT_MULTI_SELF_EXCHANGE | RT_MULTI_BANDWISE | RT_MULTI_SPARSE);
        cfg.format = format;
        int rc = rt_create(&m->ctx[q], sd, &cfg);
        if (rc != RT_OK) return rc;
        M_HIP(hipSetDevice(devices[r]));
        M_HIP(hipEventCreateWithFlags(&m->ev_rendered[q], hipEventDisableTiming));
        M_HIP(hipEventCreateWithFlags(&m->ev_sent[q], hipEventDisableTiming));
        if (m->sparse) M_HIP(hipEventCreateWithFlags(&m->ev_hdr[q], hipEventDisableTiming));
        if (q == 0) rt_max_local_rows(m->ctx[0], &max_rows);
    }
    m->rows.assign(m->world, 0);
    for (uint32_t q = 0; q < m->world; q++) rt_local_rows(m->ctx[q], &m->rows[q]);
    if (m->bandwise && m->world == 1 && m->transport == DIRECT) m->bandwise = false; // (one context renders in place: nothing travels)
    if (m->sparse && m->world == 1 && m->transport == DIRECT) m->sparse = false;
    m->max_rows = max_rows;
    m->slot_bytes = (size_t) max_rows * sd->width * m->pixel_bytes;
    m->full_bytes = (size_t) sd->height * sd->width * m->pixel_bytes;
    M_HIP(hipSetDevice(devices[0]));
    M_HIP(hipMalloc(&m->full, m->full_bytes ? m->full_bytes : 16));
    if (m->sparse) {
        // one message per context, of one capacity for all (rt_assemble_sparse's stride): the tiles of the largest context
        m->cap = ((sd->width + 15u) / 16u) * ((max_rows + 15u) / 16u);
        m->msg_bytes = rt_sparse_msg_bytes(format, m->cap);
        m->tile_bytes = (size_t) 256u * m->pixel_bytes;
        m->head_bytes = m->msg_bytes - (size_t) m->cap * m->tile_bytes; // { count, overflow, 0, 0 } + ids[cap], padded to 16 bytes
        M_HIP(hipMalloc(&m->gathered, m->msg_bytes * m->world));
        const size_t stamp_bytes = rt_sparse_stamp_bytes(m->ctx[0]);
        M_HIP(hipMalloc(&m->stamps, stamp_bytes ? stamp_bytes : 16));
        M_HIP(hipHostMalloc((void **) &m->h_hdr, sizeof(uint32_t) * 4u * m->world, hipHostMallocDefault));
        for (uint32_t q = 0; q < m->world; q++) { // messages that travel get a buffer on their own device; the others are packed into their receive slot
            const uint32_t r = q % n;
            const bool travels = m->transport == RCCL ? (r != 0 || m->self_exchange) : (m->transport == LOCAL_COPY && r != 0);
            if (!travels) continue;
            M_HIP(hipSetDevice(devices[r]));
            M_HIP(hipMalloc(&m->msg[q], m->msg_bytes));
        }
        M_HIP(hipSetDevice(devices[0]));
    }
    if ((m->world > 1 || m->transport == RCCL) && !m->bandwise && !m->sparse) M_HIP(hipMalloc(&m->gathered, m->slot_bytes * m->world + 16));
    for (uint32_t q = 0; q < m->world && !m->sparse; q++) { // rows that have to travel get a buffer on their own device
        const uint32_t r = q % n;
        const bool travels = m->bandwise || (m->transport == RCCL ? (r != 0 || m->self_exchange) : (m->transport == LOCAL_COPY && r != 0)); // (bandwise: the root's own rows are strided in the frame too)
        if (!travels) continue;
        M_HIP(hipSetDevice(devices[r]));
        M_HIP(hipMalloc(&m->local[q], m->slot_bytes ? m->slot_bytes : 16));
    }
    M_HIP(hipSetDevice(devices[0]));
    M_HIP(hipEventCreateWithFlags(&m->ev_gathered, hipEventDisableTiming));
    M_HIP(hipEventCreateWithFlags(&m->ev_assembled, hipEventDisableTiming));
    M_HIP(hipEventCreate(&m->ev_t0));
    M_HIP(hipEventCreate(&m->ev_t1));
    if (m->transport == RCCL) {
        m->comm.assign(n, nullptr);
        M_NCCL(ncclCommInitAll(m->comm.data(), (int) n, devices));
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
    if (rc != RT_OK) {
        std::string keep = rt_last_error();
        rt_multi_destroy(m);
        rt_set_last_error(keep.c_str());
        return rc;
    }
    *out = m;
    return RT_OK;
}

extern "C" int rt_render_multi(rt_multi *m, const double cam[16], void *root_full_fb, float *ms)
{
    if (!m || !cam) return fail(RT_ERR_INVALID, "rt_render_multi: null argument");
    if (m->in_flight_failed) return fail(RT_ERR_DEVICE, "rt_render_multi: an earlier frame of this object failed with part of it enqueued; destroy it and create a new one");
    DeviceRestore restore;
    const uint32_t n = m->n, P = m->parts;
    void *full = root_full_fb ? root_full_fb : m->full;
    struct FailGuard { // any early return between here and the end leaves sends / receives / events half issued
        rt_multi *m;
        bool ok = false;
        ~FailGuard() { if (!ok) m->in_flight_failed = true; }
    } guard{m};
    M_HIP(hipSetDevice(m->dev[0]));
    if (ms) M_HIP(hipEventRecord(m->ev_t0, m->s_render[0]));
    uint64_t sent = m->full_bytes; // the dense transports deliver every context's rows
    if (m->world == 1 && m->transport == DIRECT) { // one device, one part: the frame is this context's rows
        int rc = rt_render(m->ctx[0], cam, full, m->s_render[0], nullptr);
        if (rc != RT_OK) return rc;
    } else if (m->sparse) {
        // Every context renders into its own buffer (rt_render keeps the wave-per-block schedule, rt_render_sparse would not) and packs it
        // into a message that holds all of its tiles.  All parts are enqueued first, so the devices keep rendering while the host waits for
        // the headers; then each part's messages travel, exactly their used prefix, into the root's [world][msg_bytes] receive slots.
        // Contexts whose rows need not travel pack straight into their slot on the root's render stream, behind the previous frame's
        // reassembly out of it.
        if (m->have_assembled) // the receive slots are free again once the previous frame has been reassembled out of them
            for (uint32_t r = 0; r < n; r++)
                if (m->transport != RCCL || r == 0) {
                    M_HIP(hipSetDevice(m->dev[r]));
                    M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_assembled, 0));
                }
        for (uint32_t p = 0; p < P; p++)
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                M_HIP(hipSetDevice(m->dev[r]));
                if (m->msg[q]) M_HIP(hipStreamWaitEvent(m->s_render[r], m->ev_sent[q], 0)); // the previous frame's message has left this buffer
                void *dst = m->msg[q] ? m->msg[q] : (char *) m->gathered + (size_t) q * m->msg_bytes;
                int rc = rt_render(m->ctx[q], cam, nullptr, m->s_render[r], nullptr);
                if (rc == RT_OK) rc = rt_pack_sparse(m->ctx[q], nullptr, dst, m->cap, m->s_render[r]);
                if (rc != RT_OK) return rc;
                M_HIP(hipMemcpyAsync(m->h_hdr + 4u * q, dst, 16, hipMemcpyDeviceToHost, m->s_render[r]));
                M_HIP(hipEventRecord(m->ev_hdr[q], m->s_render[r]));
            }
        sent = 0;
        std::vector<size_t> bytes(n);
        for (uint32_t p = 0; p < P; p++) {
            for (uint32_t r = 0; r < n; r++) { // the host waits for this part's headers (not for the devices)
                const uint32_t q = p * n + r;
                M_HIP(hipEventSynchronize(m->ev_hdr[q]));
                const uint32_t count = m->h_hdr[4u * q], overflow = m->h_hdr[4u * q + 1u];
                if (overflow || count > m->cap) return fail(RT_ERR_DEVICE, "rt_render_multi: context %u packed %u tiles into a message of %u", q, count, m->cap);
                bytes[r] = m->head_bytes + (size_t) count * m->tile_bytes;
                sent += bytes[r];
                if (m->msg[q]) {
                    M_HIP(hipSetDevice(m->dev[r]));
                    M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_hdr[q], 0));
                }
            }
            if (m->transport == RCCL) {
                M_NCCL(ncclGroupStart());
                ncclResult_t in_group = ncclSuccess; // a failure inside the group still closes it before this call returns
                for (uint32_t r = 0; r < n && in_group == ncclSuccess; r++) {
                    const uint32_t q = p * n + r;
                    if (!m->msg[q]) continue;
                    in_group = ncclSend(m->msg[q], bytes[r], ncclInt8, 0, m->comm[r], m->s_comm[r]);
                    if (in_group == ncclSuccess)
                        in_group = ncclRecv((char *) m->gathered + (size_t) q * m->msg_bytes, bytes[r], ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
                }
                const ncclResult_t closed = ncclGroupEnd();
                if (in_group != ncclSuccess) return fail(RT_ERR_DEVICE, "ncclSend / ncclRecv of part %u failed: %s", p, ncclGetErrorString(in_group));
                M_NCCL(closed);
            } else if (m->transport == LOCAL_COPY) {
                for (uint32_t r = 1; r < n; r++) {
                    const uint32_t q = p * n + r;
                    M_HIP(hipSetDevice(m->dev[r]));
                    M_HIP(hipMemcpyAsync((char *) m->gathered + (size_t) q * m->msg_bytes, m->msg[q], bytes[r], hipMemcpyDeviceToDevice, m->s_comm[r]));
                }
            }
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                if (!m->msg[q]) continue;
                M_HIP(hipSetDevice(m->dev[r]));
                M_HIP(hipEventRecord(m->ev_sent[q], m->s_comm[r]));
                if (m->transport == LOCAL_COPY) { // the copy ran on the sender's comm stream: the root's comm stream waits for it
                    M_HIP(hipSetDevice(m->dev[0]));
                    M_HIP(hipStreamWaitEvent(m->s_comm[0], m->ev_sent[q], 0));
                }
            }
        }
        // root: everything has arrived on its comm stream (the slots packed in place are on the render stream already) -> reassemble there
        M_HIP(hipSetDevice(m->dev[0]));
        M_HIP(hipEventRecord(m->ev_gathered, m->s_comm[0]));
        M_HIP(hipStreamWaitEvent(m->s_render[0], m->ev_gathered, 0));
        int rc;
        if (root_full_fb) {
            rc = rt_assemble_sparse(m->ctx[0], m->gathered, m->cap, full, m->s_render[0]);
        } else { // the object's own buffer keeps the previous frame: only tiles that lost their content are repainted
            rc = rt_assemble_sparse_incremental(m->ctx[0], m->gathered, m->cap, full, m->stamps, m->next_tag, m->s_render[0]);
            if (rc == RT_OK) m->next_tag = m->next_tag >= 0xFFFFFFFEu ? 1u : m->next_tag + 1u;
        }
        if (rc != RT_OK) return rc;
        M_HIP(hipEventRecord(m->ev_assembled, m->s_render[0]));
        m->have_assembled = true;
    } else if (m->bandwise) {
        // Rows go band by band straight to where they belong in the full frame ("band-wise ncclRecv straight into final row
        // offsets"): band j of context q is rows (j W + q) B ... of the frame.  No rank-major receive slots and no reassembly pass over the
        // frame on the root.  Between distinct devices: one ncclSend / ncclRecv pair per band, all bands of a part in one group; rows that are
        // already on the root device (and every row in the one-GPU rehearsal) take ONE strided device copy per context.
        const size_t row_bytes = (size_t) m->width * m->pixel_bytes, band_bytes = row_bytes * m->band_rows;
        const size_t dst_pitch = band_bytes * m->world;
        for (uint32_t p = 0; p < P; p++) {
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                M_HIP(hipSetDevice(m->dev[r]));
                M_HIP(hipStreamWaitEvent(m->s_render[r], m->ev_sent[q], 0)); // the previous frame's rows have left this buffer
                int rc = rt_render(m->ctx[q], cam, m->local[q], m->s_render[r], nullptr);
                if (rc != RT_OK) return rc;
                M_HIP(hipEventRecord(m->ev_rendered[q], m->s_render[r]));
                M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_rendered[q], 0));
            }
            const bool by_rccl = m->transport == RCCL;
            if (by_rccl) M_NCCL(ncclGroupStart());
            ncclResult_t in_group = ncclSuccess;
            hipError_t copy_err = hipSuccess;
            for (uint32_t r = 0; r < n && in_group == ncclSuccess && copy_err == hipSuccess; r++) {
                const uint32_t q = p * n + r;
                const uint32_t full_bands = m->rows[q] / m->band_rows, tail_rows = m->rows[q] - full_bands * m->band_rows;
                char *dst0 = (char *) full + (size_t) q * band_bytes; // context q's band j starts dst_pitch * j further on
                if (by_rccl && (r != 0 || m->self_exchange)) {
                    for (uint32_t j = 0; j * m->band_rows < m->rows[q] && in_group == ncclSuccess; j++) {
                        const size_t bytes = j < full_bands ? band_bytes : (size_t) tail_rows * row_bytes;
                        in_group = ncclSend((const char *) m->local[q] + (size_t) j * band_bytes, bytes, ncclInt8, 0, m->comm[r], m->s_comm[r]);
                        if (in_group == ncclSuccess) in_group = ncclRecv(dst0 + (size_t) j * dst_pitch, bytes, ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
                    }
                } else { // same device as the frame: one strided copy (and one more for a last, shorter band)
                    (void) hipSetDevice(m->dev[r]);
                    if (full_bands) copy_err = hipMemcpy2DAsync(dst0, dst_pitch, m->local[q], band_bytes, band_bytes, full_bands, hipMemcpyDeviceToDevice, m->s_comm[r]);
                    if (copy_err == hipSuccess && tail_rows)
                        copy_err = hipMemcpyAsync(dst0 + (size_t) full_bands * dst_pitch, (const char *) m->local[q] + (size_t) full_bands * band_bytes, (size_t) tail_rows * row_bytes,
                                                  hipMemcpyDeviceToDevice, m->s_comm[r]);
                }
            }
            if (by_rccl) {
                const ncclResult_t closed = ncclGroupEnd(); // (a failure inside the group still closes it before this call returns)
                if (in_group != ncclSuccess) return fail(RT_ERR_DEVICE, "ncclSend / ncclRecv of part %u failed: %s", p, ncclGetErrorString(in_group));
                M_NCCL(closed);
            }
            if (copy_err != hipSuccess) return fail(RT_ERR_DEVICE, "band copy of part %u failed: %s", p, hipGetErrorString(copy_err));
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                M_HIP(hipSetDevice(m->dev[r]));
                M_HIP(hipEventRecord(m->ev_sent[q], m->s_comm[r]));
                if (r != 0 || !by_rccl) { // what ran on another comm stream than the root's: the root's comm stream waits for it
                    M_HIP(hipSetDevice(m->dev[0]));
                    M_HIP(hipStreamWaitEvent(m->s_comm[0], m->ev_sent[q], 0));
                }
            }
        }
        M_HIP(hipSetDevice(m->dev[0]));
        M_HIP(hipEventRecord(m->ev_gathered, m->s_comm[0]));
        M_HIP(hipStreamWaitEvent(m->s_render[0], m->ev_gathered, 0)); // the frame is complete for whatever follows on the root's render stream
    } else {
        // the root's receive slots are free again once the previous frame has been reassembled out of them
        if (m->have_assembled)
            for (uint32_t r = 0; r < n; r++) {
                M_HIP(hipSetDevice(m->dev[r]));
                if (m->transport != RCCL || r == 0) M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_assembled, 0));
                if (r == 0 || m->transport == LOCAL_COPY) M_HIP(hipStreamWaitEvent(m->s_render[r], m->ev_assembled, 0));
            }
        for (uint32_t p = 0; p < P; p++) {
            // every device renders part p on its render stream; rows that stay on the root go straight into their slot
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                M_HIP(hipSetDevice(m->dev[r]));
                void *dst = m->local[q] ? m->local[q] : (char *) m->gathered + (size_t) q * m->slot_bytes;
                if (m->local[q]) M_HIP(hipStreamWaitEvent(m->s_render[r], m->ev_sent[q], 0)); // the previous frame's rows have left this buffer
                int rc = rt_render(m->ctx[q], cam, dst, m->s_render[r], nullptr);
                if (rc != RT_OK) return rc;
                M_HIP(hipEventRecord(m->ev_rendered[q], m->s_render[r]));
                M_HIP(hipStreamWaitEvent(m->s_comm[r], m->ev_rendered[q], 0));
            }
            // ... and part p travels on the comm streams while part p + 1 renders
            if (m->transport == RCCL) {
                M_NCCL(ncclGroupStart());
                ncclResult_t in_group = ncclSuccess; // a failure inside the group still closes it before this call returns
                for (uint32_t r = 0; r < n && in_group == ncclSuccess; r++) {
                    const uint32_t q = p * n + r;
                    if (!m->local[q]) continue;
                    in_group = ncclSend(m->local[q], m->slot_bytes, ncclInt8, 0, m->comm[r], m->s_comm[r]);
                    if (in_group == ncclSuccess)
                        in_group = ncclRecv((char *) m->gathered + (size_t) q * m->slot_bytes, m->slot_bytes, ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
                }
                const ncclResult_t closed = ncclGroupEnd();
                if (in_group != ncclSuccess) return fail(RT_ERR_DEVICE, "ncclSend / ncclRecv of part %u failed: %s", p, ncclGetErrorString(in_group));
                M_NCCL(closed);
            } else if (m->transport == LOCAL_COPY) {
                for (uint32_t r = 1; r < n; r++) {
                    const uint32_t q = p * n + r;
                    M_HIP(hipMemcpyAsync((char *) m->gathered + (size_t) q * m->slot_bytes, m->local[q], m->slot_bytes, hipMemcpyDeviceToDevice, m->s_comm[r]));
                }
            }
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t q = p * n + r;
                if (!m->local[q]) continue;
                M_HIP(hipSetDevice(m->dev[r]));
                M_HIP(hipEventRecord(m->ev_sent[q], m->s_comm[r]));
                if (m->transport == LOCAL_COPY) { // the copy ran on the sender's comm stream: the root's comm stream waits for it
                    M_HIP(hipSetDevice(m->dev[0]));
                    M_HIP(hipStreamWaitEvent(m->s_comm[0], m->ev_sent[q], 0));
                }
            }
        }
        // root: everything has arrived on its comm stream -> reassemble on its render stream
        M_HIP(hipSetDevice(m->dev[0]));
        M_HIP(hipEventRecord(m->ev_gathered, m->s_comm[0]));
        M_HIP(hipStreamWaitEvent(m->s_render[0], m->ev_gathered, 0));
        int rc = rt_assemble(m->ctx[0], m->gathered, full, m->s_render[0]);
        if (rc != RT_OK) return rc;
        M_HIP(hipEventRecord(m->ev_assembled, m->s_render[0]));
        m->have_assembled = true;
    }
    if (ms) {
        M_HIP(hipEventRecord(m->ev_t1, m->s_render[0]));
        M_HIP(hipEventSynchronize(m->ev_t1));
        M_HIP(hipEventElapsedTime(ms, m->ev_t0, m->ev_t1));
    }
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
    M_HIP(hipSetDevice(m->dev[0]));
    M_HIP(hipStreamSynchronize(m->s_render[0]));
    return RT_OK;
}

extern "C" void *rt_multi_fb(rt_multi *m) { return m ? m->full : nullptr; }

extern "C" void *rt_multi_stream(rt_multi *m) { return m ? (void *) m->s_render[0] : nullptr; }

extern "C" int rt_multi_download(rt_multi *m, void *host_dst, size_t bytes)
{
    if (!m || !host_dst) return fail(RT_ERR_INVALID, "rt_multi_download: null argument");
    if (bytes > m->full_bytes) return fail(RT_ERR_INVALID, "rt_multi_download: %zu bytes requested, the frame holds %zu", bytes, m->full_bytes);
    DeviceRestore restore;
    M_HIP(hipSetDevice(m->dev[0]));
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
static int refuse_failed(const rt_multi *m, const char *who)
{
    if (!m->in_flight_failed) return RT_OK;
    return fail(RT_ERR_DEVICE, "%s: an earlier call on this object failed with part of it enqueued; destroy it and create a new one", who);
}

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
    if (!m->h_scene) { // first use: the FP64 arrays first, so every array is aligned to its type
        const size_t no = m->n_objects, nl = m->n_lights;
        const size_t len[5] = {sizeof(double) * RT_NCOEF * no, sizeof(double) * 3 * nl, sizeof(float) * no, sizeof(float) * 3 * no, sizeof(float) * 3 * nl};
        size_t off = 0;
        for (int k = 0; k < 5; k++) {
            m->sc_off[k] = off;
            m->sc_len[k] = len[k];
            off += len[k];
        }
        m->sc_bytes = off;
        m->d_scene.assign(m->n, nullptr);
        m->ev_scene.assign(m->n, nullptr);
        for (uint32_t r = 0; r < m->n; r++) {
            M_HIP(hipSetDevice(m->dev[r]));
            M_HIP(hipMalloc((void **) &m->d_scene[r], off));
            M_HIP(hipEventCreateWithFlags(&m->ev_scene[r], hipEventDisableTiming));
        }
        M_HIP(hipHostMalloc((void **) &m->h_scene, off, hipHostMallocPortable)); // (last: its presence says the rest exists)
    }
    if (m->have_scene_event) // the previous call's uploads and kernels have read the pinned block and the device copies
        for (uint32_t r = 0; r < m->n; r++) M_HIP(hipEventSynchronize(m->ev_scene[r]));
    for (int k = 0; k < 5; k++)
        if (src[k]) memcpy(m->h_scene + m->sc_off[k], src[k], m->sc_len[k]);
    CallGuard guard{m};
    const int fail_at = debug_fail_at();
    for (uint32_t r = 0; r < m->n; r++) {
        M_HIP(hipSetDevice(m->dev[r]));
        const unsigned char *d = m->d_scene[r];
        for (int k = 0; k < 5; k++)
            if (src[k]) M_HIP(hipMemcpyAsync(m->d_scene[r] + m->sc_off[k], m->h_scene + m->sc_off[k], m->sc_len[k], hipMemcpyHostToDevice, m->s_render[r]));
        rt_scene_update u{};
        u.coefs = src[0] ? (const double *) (d + m->sc_off[0]) : nullptr;
        u.light_p = src[1] ? (const double *) (d + m->sc_off[1]) : nullptr;
        u.reflection = src[2] ? (const float *) (d + m->sc_off[2]) : nullptr;
        u.albedo = src[3] ? (const float *) (d + m->sc_off[3]) : nullptr;
        u.light_color = src[4] ? (const float *) (d + m->sc_off[4]) : nullptr;
        for (uint32_t p = 0; p < m->parts; p++) {
            const uint32_t q = p * m->n + r;
            if ((int) q == fail_at) return fail(RT_ERR_DEVICE, "rt_set_scene_multi: MI355RT_DEBUG_MULTI_FAIL names context %u", q);
            const int rc = rt_set_scene(m->ctx[q], &u, m->s_render[r]);
            if (rc != RT_OK) return rc;
            guard.armed = true; // from here on the contexts may hold different scenes
        }
        M_HIP(hipSetDevice(m->dev[r]));
        M_HIP(hipEventRecord(m->ev_scene[r], m->s_render[r]));
    }
    m->have_scene_event = true;
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

// first use of rt_render_gbuffer_multi: events, the root's receive slots and the buffers of the contexts whose rows travel
static int gbuffer_setup(rt_multi *m)
{
    if (m->g_ready) return RT_OK;
    const bool gathers = m->world > 1 || m->transport == RCCL;
    m->g_ev_rendered.assign(m->world, nullptr);
    m->g_ev_sent.assign(m->world, nullptr);
    for (int k = 0; k < 3; k++) {
        m->g_local[k].assign(m->world, nullptr);
        m->g_slot[k] = (size_t) m->max_rows * m->width * PLANE_ELEM[k];
    }
    for (uint32_t q = 0; q < m->world && gathers; q++) {
        M_HIP(hipSetDevice(m->dev[q % m->n]));
        M_HIP(hipEventCreateWithFlags(&m->g_ev_rendered[q], hipEventDisableTiming));
        M_HIP(hipEventCreateWithFlags(&m->g_ev_sent[q], hipEventDisableTiming));
        if (!travels(m, q) || m->rows[q] == 0u) continue; // (a context without rows renders and sends nothing)
        for (int k = 0; k < 3; k++) M_HIP(hipMalloc(&m->g_local[k][q], (size_t) m->rows[q] * m->width * PLANE_ELEM[k]));
    }
    M_HIP(hipSetDevice(m->dev[0]));
    for (int k = 0; k < 3 && gathers; k++) M_HIP(hipMalloc(&m->g_gathered[k], m->g_slot[k] * m->world + 16));
    M_HIP(hipEventCreateWithFlags(&m->g_ev_gathered, hipEventDisableTiming));
    M_HIP(hipEventCreateWithFlags(&m->g_ev_assembled, hipEventDisableTiming));
    m->g_ready = true;
    return RT_OK;
}

extern "C" int rt_render_gbuffer_multi(rt_multi *m, const double cam[16], int32_t *root_object, double *root_t, float *root_normal, float *ms)
{
    if (!m || !cam) return fail(RT_ERR_INVALID, "rt_render_gbuffer_multi: null argument");
    if (!root_object && !root_t && !root_normal) return fail(RT_ERR_INVALID, "rt_render_gbuffer_multi: all three planes are null");
    if (int rc = refuse_failed(m, "rt_render_gbuffer_multi")) return rc;
    DeviceRestore restore;
    const uint32_t n = m->n, P = m->parts;
    void *root[3] = {root_object, root_t, root_normal};
    if (m->world == 1 && m->transport == DIRECT) { // one device, one part: the planes are this context's rows
        return rt_render_gbuffer(m->ctx[0], cam, root_object, root_t, root_normal, m->s_render[0], ms);
    }
    if (int rc = gbuffer_setup(m)) {
        m->in_flight_failed = true; // (half of the buffers exist: rt_multi_destroy frees them, nothing else may use them)
        return rc;
    }
    CallGuard guard{m};
    M_HIP(hipSetDevice(m->dev[0]));
    if (ms) M_HIP(hipEventRecord(m->ev_t0, m->s_render[0]));
    // the root's receive slots and the travelling contexts' buffers are free again once the previous call's planes have been reassembled
    if (m->g_have_assembled)
        for (uint32_t r = 0; r < n; r++) {
            M_HIP(hipSetDevice(m->dev[r]));
            M_HIP(hipStreamWaitEvent(m->s_comm[r], m->g_ev_assembled, 0));
            M_HIP(hipStreamWaitEvent(m->s_render[r], m->g_ev_assembled, 0));
        }
    for (uint32_t p = 0; p < P; p++) {
        for (uint32_t r = 0; r < n; r++) { // every device runs the pass for part p on its render stream, behind its scene updates and frames
            const uint32_t q = p * n + r;
            if (m->rows[q] == 0u) continue;
            M_HIP(hipSetDevice(m->dev[r]));
            void *dst[3];
            for (int k = 0; k < 3; k++)
                dst[k] = !root[k] ? nullptr : (m->g_local[k][q] ? m->g_local[k][q] : (void *) ((char *) m->g_gathered[k] + (size_t) q * m->g_slot[k]));
            const int rc = rt_render_gbuffer(m->ctx[q], cam, (int32_t *) dst[0], (double *) dst[1], (float *) dst[2], m->s_render[r], nullptr);
            if (rc != RT_OK) return rc; // (a per-context refusal: every context gives it, so the first one does, with nothing enqueued)
            guard.armed = true;
            M_HIP(hipEventRecord(m->g_ev_rendered[q], m->s_render[r]));
            M_HIP(hipStreamWaitEvent(m->s_comm[r], m->g_ev_rendered[q], 0));
        }
        // ... and part p's rows travel on the comm streams while part p + 1 runs
        if (m->transport == RCCL) {
            M_NCCL(ncclGroupStart());
            ncclResult_t in_group = ncclSuccess; // a failure inside the group still closes it before this call returns
            for (uint32_t r = 0; r < n && in_group == ncclSuccess; r++) {
                const uint32_t q = p * n + r;
                for (int k = 0; k < 3 && in_group == ncclSuccess; k++) {
                    if (!root[k] || !m->g_local[k][q]) continue;
                    const size_t bytes = (size_t) m->rows[q] * m->width * PLANE_ELEM[k];
                    in_group = ncclSend(m->g_local[k][q], bytes, ncclInt8, 0, m->comm[r], m->s_comm[r]);
                    if (in_group == ncclSuccess)
                        in_group = ncclRecv((char *) m->g_gathered[k] + (size_t) q * m->g_slot[k], bytes, ncclInt8, (int) r, m->comm[0], m->s_comm[0]);
                }
            }
            const ncclResult_t closed = ncclGroupEnd();
            if (in_group != ncclSuccess) return fail(RT_ERR_DEVICE, "ncclSend / ncclRecv of part %u's planes failed: %s", p, ncclGetErrorString(in_group));
            M_NCCL(closed);
        } else if (m->transport == LOCAL_COPY) {
            for (uint32_t r = 1; r < n; r++) {
                const uint32_t q = p * n + r;
                for (int k = 0; k < 3; k++) {
                    if (!root[k] || !m->g_local[k][q]) continue;
                    M_HIP(hipMemcpyAsync((char *) m->g_gathered[k] + (size_t) q * m->g_slot[k], m->g_local[k][q], (size_t) m->rows[q] * m->width * PLANE_ELEM[k],
                                         hipMemcpyDeviceToDevice, m->s_comm[r]));
                }
            }
        }
        for (uint32_t r = 0; r < n; r++) {
            const uint32_t q = p * n + r;
            if (!m->g_local[0][q]) continue; // (all three planes of a context travel, or none)
            M_HIP(hipSetDevice(m->dev[r]));
            M_HIP(hipEventRecord(m->g_ev_sent[q], m->s_comm[r]));
            if (m->transport == LOCAL_COPY) { // the copy ran on the sender's comm stream: the root's comm stream waits for it
                M_HIP(hipSetDevice(m->dev[0]));
                M_HIP(hipStreamWaitEvent(m->s_comm[0], m->g_ev_sent[q], 0));
            }
        }
    }
    // root: everything has arrived on its comm stream -> reassemble the requested planes on its render stream
    M_HIP(hipSetDevice(m->dev[0]));
    M_HIP(hipEventRecord(m->g_ev_gathered, m->s_comm[0]));
    M_HIP(hipStreamWaitEvent(m->s_render[0], m->g_ev_gathered, 0));
    guard.armed = true;
    for (int k = 0; k < 3; k++) {
        if (!root[k]) continue;
        const int rc = rt_assemble_planes(m->ctx[0], m->g_gathered[k], m->g_slot[k], root[k], (uint32_t) PLANE_ELEM[k], m->s_render[0]);
        if (rc != RT_OK) return rc;
    }
    M_HIP(hipEventRecord(m->g_ev_assembled, m->s_render[0]));
    m->g_have_assembled = true;
    if (ms) {
        M_HIP(hipEventRecord(m->ev_t1, m->s_render[0]));
        M_HIP(hipEventSynchronize(m->ev_t1));
        M_HIP(hipEventElapsedTime(ms, m->ev_t0, m->ev_t1));
    }
    guard.ok = true;
    return RT_OK;
}

// first use of the extents calls: [world][n_objects] records on the root, and the records of the contexts whose results travel
static int extents_setup(rt_multi *m)
{
    if (m->x_ready) return RT_OK;
    const size_t bytes = sizeof(rt_object_extent) * (size_t) m->n_objects;
    m->x_local.assign(m->world, nullptr);
    m->x_ev_done.assign(m->world, nullptr);
    m->x_ev_sent.assign(m->world, nullptr);
    for (uint32_t q = 0; q < m->world; q++) {
        M_HIP(hipSetDevice(m->dev[q % m->n]));
        M_HIP(hipEventCreateWithFlags(&m->x_ev_done[q], hipEventDisableTiming));
        M_HIP(hipEventCreateWithFlags(&m->x_ev_sent[q], hipEventDisableTiming));
        if (travels(m, q)) M_HIP(hipMalloc(&m->x_local[q], bytes));
    }
    M_HIP(hipSetDevice(m->dev[0]));
    M_HIP(hipMalloc(&m->x_parts, bytes * m->world));
    M_HIP(hipMalloc(&m->x_merged, bytes));
    M_HIP(hipEventCreateWithFlags(&m->x_ev_merged, hipEventDisableTiming));
    m->x_ready = true;
    return RT_OK;
}

static int extents_multi(rt_multi *m, const double cam[16], const uint32_t rect[4], rt_object_extent *root_dev_out, float *ms)
{
    if (m->n_objects == 0u) { // (a scene without objects: the contexts enqueue nothing, and neither does the merge)
        const int rc = rt_object_extents(m->ctx[0], cam, rect, root_dev_out, m->s_render[0], nullptr); // ... but they still refuse what they refuse
        if (rc == RT_OK && ms) *ms = 0.0f;
        return rc;
    }
    if (int rc = extents_setup(m)) {
        m->in_flight_failed = true;
        return rc;
    }
    CallGuard guard{m};
    const size_t bytes = sizeof(rt_object_extent) * (size_t) m->n_objects;
    M_HIP(hipSetDevice(m->dev[0]));
    if (ms) M_HIP(hipEventRecord(m->ev_t0, m->s_render[0]));
    if (m->x_have_merged) // the previous call's merge has read the root's records, hence every copy has left its context's buffer
        for (uint32_t r = 0; r < m->n; r++) {
            M_HIP(hipSetDevice(m->dev[r]));
            M_HIP(hipStreamWaitEvent(m->s_render[r], m->x_ev_merged, 0));
        }
    for (uint32_t p = 0; p < m->parts; p++)
        for (uint32_t r = 0; r < m->n; r++) {
            const uint32_t q = p * m->n + r;
            M_HIP(hipSetDevice(m->dev[r]));
            void *slot = (char *) m->x_parts + (size_t) q * bytes;
            const int rc = rt_object_extents(m->ctx[q], cam, rect, (rt_object_extent *) (m->x_local[q] ? m->x_local[q] : slot), m->s_render[r], nullptr);
            if (rc != RT_OK) return rc; // (a per-context refusal: the first context gives it, with nothing enqueued)
            guard.armed = true;
            if (!m->x_local[q]) continue; // written in place on the root's render stream
            M_HIP(hipEventRecord(m->x_ev_done[q], m->s_render[r]));
            M_HIP(hipStreamWaitEvent(m->s_comm[r], m->x_ev_done[q], 0));
            if (m->dev[r] == m->dev[0]) M_HIP(hipMemcpyAsync(slot, m->x_local[q], bytes, hipMemcpyDeviceToDevice, m->s_comm[r]));
            else M_HIP(hipMemcpyPeerAsync(slot, m->dev[0], m->x_local[q], m->dev[r], bytes, m->s_comm[r]));
            M_HIP(hipEventRecord(m->x_ev_sent[q], m->s_comm[r]));
            M_HIP(hipSetDevice(m->dev[0]));
            M_HIP(hipStreamWaitEvent(m->s_render[0], m->x_ev_sent[q], 0));
        }
    M_HIP(hipSetDevice(m->dev[0]));
    const int rc = rt_merge_object_extents(m->ctx[0], (const rt_object_extent *) m->x_parts, m->world, root_dev_out, m->s_render[0]);
    if (rc != RT_OK) return rc;
    M_HIP(hipEventRecord(m->x_ev_merged, m->s_render[0]));
    m->x_have_merged = true;
    if (ms) {
        M_HIP(hipEventRecord(m->ev_t1, m->s_render[0]));
        M_HIP(hipEventSynchronize(m->ev_t1));
        M_HIP(hipEventElapsedTime(ms, m->ev_t0, m->ev_t1));
    }
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
    if (int rc = extents_setup(m)) {
        m->in_flight_failed = true;
        return rc;
    }
    // x_merged is read by the blocking copy below before this call returns, so no later call can overwrite it early
    if (int rc = extents_multi(m, cam, rect, (rt_object_extent *) m->x_merged, nullptr)) return rc;
    M_HIP(hipSetDevice(m->dev[0]));
    M_HIP(hipMemcpyAsync(out_host, m->x_merged, sizeof(rt_object_extent) * (size_t) m->n_objects, hipMemcpyDeviceToHost, m->s_render[0]));
    M_HIP(hipStreamSynchronize(m->s_render[0]));
    return RT_OK;
}
