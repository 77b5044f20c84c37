// multi_calls_main.cpp -- the scripts of the recorded call order (tests/tools/multi_calls_lab.py; DESIGN.md, "Host code: one copy of each rule"):
// csrc/rt_multi.cpp driven through its C ABI on top of the recording runtime of multi_shim.cpp, one section of output per script.
//   == steady/<layout>_<transport>_<format> ==   the whole script of one object, then the ledger
//   == fail/<name> ==                            one injected failure: the log, the return code, the error text of the failed and of the next call
//   == create/<function> ==                      rt_create_multi with the k-th call of <function> failing, k = 1 ... until it succeeds: the code, the ledger and,
//                                                in any order, the error texts (create_sparse/: an RT_MULTI_SPARSE object; setup/: the first scene update,
//                                                G-buffer and extents call of an object, which set their buffers and events up)
// Lines that start with "~ " are checked by their own rule and are not part of a fixture.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "mi355rt.h"

extern "C" {
void shim_reset(int n_devices);
void shim_fail(const char *fn, int k);
void shim_external(const void *p, size_t bytes, const char *name);
void shim_note(const char *text);
int shim_calls(const char *fn);
int shim_ledger(void);
void shim_print(FILE *f);
}

namespace {

struct Layout {
    const char *name;
    int devices[4];
    uint32_t n, parts, band, flags, width, height;
};
const Layout LAYOUTS[] = {
    {"direct", {0}, 1, 1, 16, 0, 33, 37},          {"parts", {0}, 1, 3, 8, 0, 33, 37},      {"copy", {0, 0}, 2, 2, 8, 0, 33, 37},
    {"self", {0}, 1, 1, 16, RT_MULTI_SELF_EXCHANGE, 33, 37}, {"rccl", {0, 1, 2}, 3, 2, 8, 0, 33, 37}, {"ten", {0, 0}, 2, 5, 4, 0, 129, 31},
};

const Layout &layout(const char *name)
{
    for (const Layout &l : LAYOUTS)
        if (!strcmp(l.name, name)) return l;
    abort();
}

constexpr uint32_t N_OBJECTS = 3, N_LIGHTS = 2;
constexpr size_t MAX_PIXELS = 129 * 37;
alignas(16) unsigned char fb[MAX_PIXELS * 16], plane_object[MAX_PIXELS * 4], plane_t[MAX_PIXELS * 8], plane_normal[MAX_PIXELS * 16];
alignas(16) rt_object_extent extents_dev[N_OBJECTS], extents_host[N_OBJECTS];
double coefs[N_OBJECTS * RT_NCOEF], light_p[N_LIGHTS * 3], cam[16];
float reflection[N_OBJECTS], albedo[N_OBJECTS * 3], light_color[N_LIGHTS * 3];
uint8_t light_is_spherical[N_LIGHTS];

void note(const char *fmt, ...)
{
    char buf[1400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    shim_note(buf);
}

int returned(int rc)
{
    if (rc == RT_OK) note("< 0");
    else note("< %d \"%s\"", rc, rt_last_error());
    return rc;
}

rt_multi *create(const Layout &l, uint32_t mode, uint32_t format, int *rc_out = nullptr)
{
    rt_scene_desc sd{};
    sd.width = l.width;
    sd.height = l.height;
    sd.vertical_fov = 1.0;
    sd.max_reflections = 2;
    sd.n_objects = N_OBJECTS;
    sd.n_lights = N_LIGHTS;
    sd.coefs = coefs;
    sd.reflection = reflection;
    sd.albedo = albedo;
    sd.light_is_spherical = light_is_spherical;
    sd.light_p = light_p;
    sd.light_color = light_color;
    rt_multi *m = nullptr;
    const int rc = rt_create_multi(&m, &sd, l.devices, l.n, l.band, l.parts, l.flags | mode, format);
    if (rc_out) *rc_out = rc;
    return m;
}

void begin(const char *section)
{
    shim_reset(4);
    shim_external(fb, sizeof(fb), "fb");
    shim_external(plane_object, sizeof(plane_object), "object");
    shim_external(plane_t, sizeof(plane_t), "t");
    shim_external(plane_normal, sizeof(plane_normal), "normal");
    shim_external(extents_dev, sizeof(extents_dev), "extents");
    printf("== %s ==\n", section);
}

int bad = 0;

void end(rt_multi *m)
{
    if (m) {
        note("> rt_multi_destroy");
        returned(rt_multi_destroy(m));
    }
    bad += shim_ledger();
    shim_print(stdout);
}

int frame(rt_multi *m, void *into, bool timed)
{
    float ms = 0.0f;
    note("> rt_render_multi into %s%s", into ? "the caller's buffer" : "its own", timed ? ", timed" : "");
    const int rc = returned(rt_render_multi(m, cam, into, timed ? &ms : nullptr));
    uint64_t sent = 0, dense = 0;
    if (rc == RT_OK && rt_multi_last_transfer(m, &sent, &dense) == RT_OK) note("  sent %llu of %llu bytes", (unsigned long long) sent, (unsigned long long) dense);
    return rc;
}

void steady(const char *layout_name, uint32_t mode, uint32_t format)
{
    const Layout &l = layout(layout_name);
    char section[96];
    snprintf(section, sizeof(section), "steady/%s_%s_%s", l.name, mode == RT_MULTI_BANDWISE ? "bandwise" : mode == RT_MULTI_SPARSE ? "sparse" : "dense",
             format == RT_FMT_RGBA8 ? "rgba8" : "rgba32f");
    begin(section);
    int rc = 0;
    rt_multi *m = create(l, mode, format, &rc);
    if (!m) {
        note("rt_create_multi: %d \"%s\"", rc, rt_last_error());
        bad++;
        return end(nullptr);
    }
    uint32_t contexts = 0, transport = 0;
    rt_multi_info(m, &contexts, &transport);
    note("%u contexts, transport %u", contexts, transport);
    frame(m, nullptr, false);
    frame(m, nullptr, false);
    frame(m, fb, false);
    frame(m, nullptr, true);
    rt_scene_update all{coefs, reflection, albedo, light_p, light_color}, one{};
    one.albedo = albedo;
    note("> rt_set_scene_multi, all arrays");
    returned(rt_set_scene_multi(m, &all));
    note("> rt_set_scene_multi, albedo");
    returned(rt_set_scene_multi(m, &one));
    uint64_t applied = 0, rejected = 0;
    uint32_t reason = 0, index = 0;
    note("> rt_multi_set_scene_status");
    returned(rt_multi_set_scene_status(m, &applied, &rejected, &reason, &index));
    float ms = 0.0f;
    note("> rt_render_gbuffer_multi, three planes");
    returned(rt_render_gbuffer_multi(m, cam, (int32_t *) plane_object, (double *) plane_t, (float *) plane_normal, nullptr));
    note("> rt_render_gbuffer_multi, t, timed");
    returned(rt_render_gbuffer_multi(m, cam, nullptr, (double *) plane_t, nullptr, &ms));
    const uint32_t rect[4] = {1, 2, 20, 30};
    note("> rt_object_extents_multi");
    returned(rt_object_extents_multi(m, cam, nullptr, extents_dev, nullptr));
    note("> rt_object_extents_multi, rect, timed");
    returned(rt_object_extents_multi(m, cam, rect, extents_dev, &ms));
    note("> rt_object_extents_multi_host");
    returned(rt_object_extents_multi_host(m, cam, nullptr, extents_host));
    frame(m, nullptr, false);
    end(m);
}

// the failed call has been made: the next calls on the object, then destroy and the ledger
void after_failure(rt_multi *m)
{
    shim_fail(nullptr, 0);
    uint64_t applied = 0, rejected = 0;
    uint32_t reason = 0, index = 0;
    note("> rt_multi_set_scene_status");
    returned(rt_multi_set_scene_status(m, &applied, &rejected, &reason, &index));
    const int rc = rt_render_multi(m, cam, nullptr, nullptr); // (its refusal is the one text a refactor was allowed to reword)
    note("~ rt_render_multi: %d \"%s\"", rc, rt_last_error());
    end(m);
}

void fail_in(const char *section, const char *layout_name, const char *fn, int k, int call)
{
    begin(section);
    rt_multi *m = create(layout(layout_name), 0, RT_FMT_RGBA32F);
    if (!m) abort();
    if (fn) shim_fail(fn, k);
    else setenv("MI355RT_DEBUG_MULTI_FAIL", "1", 1);
    if (call == 0) {
        frame(m, nullptr, false);
    } else if (call == 1) {
        note("> rt_render_gbuffer_multi, three planes");
        returned(rt_render_gbuffer_multi(m, cam, (int32_t *) plane_object, (double *) plane_t, (float *) plane_normal, nullptr));
    } else {
        rt_scene_update one{};
        one.albedo = albedo;
        note("> rt_set_scene_multi, albedo");
        returned(rt_set_scene_multi(m, &one));
    }
    unsetenv("MI355RT_DEBUG_MULTI_FAIL");
    after_failure(m);
}

void create_failures(const char *fn, uint32_t mode)
{
    char section[96];
    snprintf(section, sizeof(section), "create%s/%s", mode == RT_MULTI_SPARSE ? "_sparse" : "", fn);
    for (int k = 1; k < 1000; k++) {
        begin(section);
        shim_fail(fn, k);
        int rc = 0;
        rt_multi *m = create(layout("rccl"), mode, RT_FMT_RGBA32F, &rc);
        const int made = shim_calls(fn);
        shim_fail(nullptr, 0);
        if (m) {
            note("k=%d: created after %d calls", k, made);
            rt_multi_destroy(m);
        } else {
            note("k=%d: %d \"%s\"", k, rc, rt_last_error());
        }
        bad += shim_ledger();
        shim_print(stdout);
        if (m) return;
    }
    abort();
}

// the first use of the scene update, the G-buffer and the extents sets their buffers and events up: the k-th call of `fn` fails there
void setup_failures(const char *fn)
{
    char section[96];
    snprintf(section, sizeof(section), "setup/%s", fn);
    for (int k = 1; k < 1000; k++) {
        begin(section);
        rt_multi *m = create(layout("rccl"), 0, RT_FMT_RGBA32F);
        if (!m) abort();
        shim_fail(fn, k);
        rt_scene_update one{};
        one.albedo = albedo;
        int rc = rt_set_scene_multi(m, &one);
        const char *who = "rt_set_scene_multi";
        if (rc == RT_OK) rc = rt_render_gbuffer_multi(m, cam, (int32_t *) plane_object, (double *) plane_t, (float *) plane_normal, nullptr), who = "rt_render_gbuffer_multi";
        if (rc == RT_OK) rc = rt_object_extents_multi_host(m, cam, nullptr, extents_host), who = "rt_object_extents_multi_host";
        shim_fail(nullptr, 0);
        const std::string text = rc == RT_OK ? "" : rt_last_error();
        rt_multi_destroy(m);
        shim_print(nullptr); // (the calls themselves are pinned by the steady scripts)
        if (rc == RT_OK) note("k=%d: all set up", k);
        else note("k=%d: %s %d \"%s\"", k, who, rc, text.c_str());
        bad += shim_ledger();
        shim_print(stdout);
        if (rc == RT_OK) return;
    }
    abort();
}

} // namespace

int main()
{
    for (int i = 0; i < 16; i++) cam[i] = i % 5 == 0 ? 1.0 : 0.0;
    for (const char *name : {"direct", "parts", "copy", "self", "rccl", "ten"}) steady(name, 0, RT_FMT_RGBA32F);
    steady("rccl", 0, RT_FMT_RGBA8);
    for (const char *name : {"copy", "self", "rccl"}) {
        steady(name, RT_MULTI_BANDWISE, RT_FMT_RGBA32F);
        steady(name, RT_MULTI_SPARSE, RT_FMT_RGBA32F);
    }
    fail_in("fail/render_third_context", "rccl", "rt_render", 3, 0);
    fail_in("fail/send_second_frame", "rccl", "ncclSend", 2, 0);
    fail_in("fail/send_second_gbuffer", "rccl", "ncclSend", 2, 1);
    fail_in("fail/group_end", "rccl", "ncclGroupEnd", 1, 0);
    fail_in("fail/debug_multi_fail_copy", "copy", nullptr, 0, 2);
    for (const char *fn : {"hipMalloc", "hipEventCreateWithFlags", "rt_create", "hipStreamCreateWithFlags", "hipEventCreate"}) create_failures(fn, 0);
    for (const char *fn : {"hipMalloc", "hipHostMalloc"}) create_failures(fn, RT_MULTI_SPARSE);
    for (const char *fn : {"hipMalloc", "hipEventCreateWithFlags", "hipHostMalloc"}) setup_failures(fn);
    return bad ? 1 : 0;
}
