// pick_driver.cpp -- a minimal headless "host" that picks: scene.h + update.h (reference src/ray-tracer.cpp:152,215,226,245 call
// sequence) plus mi355rt_update_pick of libmi355rt_update.so, i.e. what a mouse-click handler of an interactive host calls.
//   pick_driver <scene.yml> <width> <height> <x0> <y0> [<x1> <y1> ...]
// renders one frame with the start-up camera (identity), then prints one line per pixel, bits preserved:
//   <x> <y> <object> <t> <point x> <point y> <point z> <normal x> <normal y> <normal z>        (%d for integers, %a for the rest)
// A call the back end refuses prints "refused <code>" for that pixel.  Before the frame is drawn the same entry point must refuse:
// the driver checks that and exits 1 otherwise.
#include <cstdio>
#include <cstdlib>

#include "mi355rt.h"
#include "scene-exception.h"
#include "update.h"

extern "C" int mi355rt_update_pick(unsigned int x, unsigned int y, rt_hit *out);

int main(int argc, char **argv)
{
    if (argc < 6 || (argc - 4) % 2 != 0) {
        std::fprintf(stderr, "usage: %s scene.yml W H x y [x y ...]\n", argv[0]);
        return 2;
    }
    Scene scene;
    try {
        scene = Scene::load_from_file(argv[1]);
    } catch (const SceneException &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    scene.px_width = (unsigned) std::atoi(argv[2]);
    scene.px_height = (unsigned) std::atoi(argv[3]);
    rt_hit h{};
    if (mi355rt_update_pick(0, 0, &h) != RT_ERR_INVALID) { // no back end yet
        std::fprintf(stderr, "mi355rt_update_pick before init_update was not refused\n");
        return 1;
    }
    init_update(42, scene);
    if (mi355rt_update_pick(0, 0, &h) != RT_ERR_INVALID) { // no frame yet: no camera to pick with
        std::fprintf(stderr, "mi355rt_update_pick before the first update() was not refused\n");
        return 1;
    }
    (void) update(glm::dmat4(1.0));
    for (int i = 4; i + 1 < argc; i += 2) {
        const unsigned x = (unsigned) std::strtoul(argv[i], nullptr, 10), y = (unsigned) std::strtoul(argv[i + 1], nullptr, 10);
        const int rc = mi355rt_update_pick(x, y, &h);
        if (rc != RT_OK) {
            std::printf("%u %u refused %d\n", x, y, rc);
            continue;
        }
        std::printf("%u %u %d %a %a %a %a %a %a %a\n", x, y, (int) h.object, h.t, h.point[0], h.point[1], h.point[2], (double) h.normal[0], (double) h.normal[1],
                    (double) h.normal[2]);
    }
    cleanup_update();
    return 0;
}
