// cubic_lab_rays.h -- one (ray, degree-3 object) test as the degree-3 labs exchange it (test infrastructure).
// tests/tools/cubic_guard_lab.cpp forms the records from the oracle (lab_enumerate); tests/tools/cubic_device_lab.hip runs them on the
// device; tests/tools/cubic_device_lab.py restates the layout for numpy.
#pragma once
#include <cstdint>

// Primary rays carry the object's Taylor record (rt_math.hpp: CubicAt) at the frame's origin, formed on the host the way rt_render forms
// FrameArgs::cub_rec (LAB_HAS_REC); shadow and bounce rays leave it to the lab, which forms it at the ray's origin as the kernels do per lane.
struct LabRay {
    double o[3], d[3];
    double max_t;      // what the caller compares the root with (1e6 for a nearest hit, the light's for a shadow ray)
    double rec[10];
    int32_t obj;       // index of the object in the scene
    int32_t flags;     // LAB_DECIDE: a shadow ray (only "EPS < t < max_t?" is asked)
};
enum { LAB_DECIDE = 1, LAB_HAS_REC = 2 };

// where the test comes from: kind 0 primary, 1 shadow (of the primary hit, light `light`), 2 the first bounce of a mirror hit
struct LabWhere {
    int32_t kind, x, y, light;
};
static_assert(sizeof(LabRay) == 144 && sizeof(LabWhere) == 16, "layout restated in cubic_device_lab.py");
