// scene_image_lab.cpp -- the whole scene image of csrc/rt_scene_image.hpp as bytes, for the tests that compare it with what a context
// holds on the device (rt_debug_scene_blob).  Part of tests/tools/scene_pack_lab.py's library.
#include <cstring>

#include "rt_scene_image.hpp"
#include "scene_pack_lab.h"

// the image as a context with these rt_config flags holds it, [blob][DevLight x n][LightK x n] (rt_debug_scene_blob's layout); returns its size
extern "C" uint64_t lab_scene_image(const LabDesc *sd, uint32_t flags, unsigned char *out, uint64_t cap)
{
    FrameArgs fa{};
    const rtp::SceneImage im = rtp::scene_image(lab_desc(sd), flags, fa);
    const size_t nb = im.blob.size(), nl = sizeof(DevLight) * im.lights.size(), nk = sizeof(LightK) * im.lightk.size();
    if (!out || cap < nb + nl + nk) return nb + nl + nk;
    std::memcpy(out, im.blob.data(), nb);
    if (nl) std::memcpy(out + nb, im.lights.data(), nl);
    if (nk) std::memcpy(out + nb + nl, im.lightk.data(), nk);
    return nb + nl + nk;
}
