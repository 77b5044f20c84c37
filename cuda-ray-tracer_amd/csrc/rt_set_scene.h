// rt_set_scene.h -- what the host (rt_capi.cpp) hands to the scene-update kernel (rt_set_scene.hip) and reads back from it.
#ifndef RT_SET_SCENE_H
#define RT_SET_SCENE_H

#include <stdint.h>

#include "rt_scene_dev.h"

// rt_set_scene_status's reason codes (include/mi355rt.h, RT_SCENE_REJECT_*)
#define RT_SCENE_REJECT_CLASS 1u
#define RT_SCENE_REJECT_BOUND 2u
#define RT_SCENE_REJECT_MIRROR 3u
#define RT_SCENE_REJECT_CUBIC 4u
#define RT_SCENE_REJECT_LIGHT 5u

// a small device block owned by the context; the kernel's thread 0 is its only writer
struct SetSceneStatus {
    unsigned long long applied, rejected; // updates committed / refused since rt_create
    uint32_t reason, index;               // of the most recent refusal
    uint32_t last;                        // the most recent update: 0 none yet, 1 applied, 2 rejected
    uint32_t pad;
};
static_assert(sizeof(SetSceneStatus) == 32, "SetSceneStatus layout");

struct SetSceneArgs {
    unsigned char *blob;       // the context's scene blob (FrameArgs: [DevObject][UsEntry][GqEntry][LinEntry][uint32][MatEntry])
    DevLight *lights;          // [DevLight x n_lights][LightK x n_lights]
    SetSceneStatus *status;
    const double *coefs;       // [n_obj][20]      raw descriptor arrays in device memory; NULL = keep what the context holds
    const float *reflection;   // [n_obj]
    const float *albedo;       // [n_obj][3]
    const double *light_p;     // [n_lights][3]
    const float *light_color;  // [n_lights][3]
    uint32_t n_obj, n_lights;
    uint32_t n_us, n_gq, n_lin;
    uint32_t off_us, off_gq, off_lin, off_mat;
    uint32_t has_mirror;       // FrameArgs::has_mirror of the context: must not change
    uint32_t n_chunks;         // RT_FLAG_STREAM_CULL contexts (rt_get_stream_cull): the 64-entry chunks of the unit-sphere table, and their bounds;
    UsEntry *bounds;           // 0 / NULL elsewhere
};

#endif
