// ref_driver.cpp -- frame driver for a build of the REFERENCE's own CPU path (test infrastructure).
//
// oracle/Makefile.ref links this file with the reference's update-cpu.cpp, surface.cpp, light.cpp and
// scene-exception.cpp, compiled unmodified against the stand-in headers of oracle/ref_shim/, into
// oracle/_ref/ref_frames_{O2,O0}.  Nothing here computes a pixel: it builds a Scene through the
// reference's factories, calls init_update() / update() and writes update-cpu.cpp's g_data.
//
//   ref_frames <job file> <out file>
//
// Job file (little endian, written by tests/tools/ref_binary.py):
//   char[8] "RTREFFRM"
//   u32 width, height, max_reflections, n_objects, n_lights, n_cameras
//   f64 vertical_fov (radians, as Scene::vertical_fov holds it)    f32 bg_color[3]
//   n_objects x { u32 kind; f64 a[20]; f32 reflection_ratio; f32 color[3] }
//       kind 0 polynomial: a = the 20 coefficients in the order of SurfaceCoefs
//            1 sphere:     a[0..2] centre, a[3] radius        -> SurfaceCoefs::sphere
//            2 plane:      a[0..2] origin, a[3..5] normal     -> SurfaceCoefs::plane
//            3 dingDong:   a[0..2] origin                     -> SurfaceCoefs::dingDong
//            4 clebsch, 5 cayley                              -> SurfaceCoefs::clebsch / cayley
//   n_lights x { u32 kind; f32 intensity; f64 v[3]; f32 color[3] }
//       kind 0 as stored: is_spherical = (intensity != 0), p = v, light_color = color
//            1 directional: v = direction -> LightSource::directional(intensity, v, color)
//            2 spherical:   v = position  -> LightSource::spherical(intensity, v, color)
//   n_cameras x f64[16], column-major dmat4
// Out file: n_cameras x height x width x 3 float32, row 0 = bottom, as update() leaves g_data.
// Exit code 3 with the SceneException's text on stderr when a factory rejects its arguments.
//
// Object::Object is defined here as the plain member initialiser it is: the reference defines it in
// src/scene.cpp next to its YAML loader, which needs yaml-cpp and is not built.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scene-exception.h"
#include "scene.h"
#include "update.h"

extern std::vector<float> g_data; // src/update-cpu.cpp

Object::Object(SurfaceCoefs surface, float reflection_ratio, const glm::vec3 &color)
    : surface{surface}, reflection_ratio{reflection_ratio}, color{color}
{}

static FILE *g_in;

template <typename T>
static T rd()
{
    T v;
    if (fread(&v, sizeof(T), 1, g_in) != 1) {
        fprintf(stderr, "ref_frames: job file too short\n");
        exit(2);
    }
    return v;
}

// Every value goes through a named local before it reaches a constructor: the evaluation order of
// function arguments is unspecified, and rd() has a side effect.
static glm::dvec3 rd_dvec3(const double *a)
{
    const double x = a[0], y = a[1], z = a[2];
    return glm::dvec3(x, y, z);
}

static glm::vec3 rd_vec3()
{
    const float x = rd<float>();
    const float y = rd<float>();
    const float z = rd<float>();
    return glm::vec3(x, y, z);
}

int main(int argc, char **argv)
{
    if (argc != 3 || !(g_in = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: ref_frames <job file> <out file>\n");
        return 2;
    }
    char magic[8];
    if (fread(magic, 1, 8, g_in) != 8 || memcmp(magic, "RTREFFRM", 8) != 0) {
        fprintf(stderr, "ref_frames: not a frame job\n");
        return 2;
    }
    Scene scene;
    scene.px_width = rd<uint32_t>();
    scene.px_height = rd<uint32_t>();
    scene.max_reflections = rd<uint32_t>();
    const uint32_t n_objects = rd<uint32_t>();
    const uint32_t n_lights = rd<uint32_t>();
    const uint32_t n_cameras = rd<uint32_t>();
    scene.vertical_fov = rd<double>();
    scene.bg_color = rd_vec3();
    try {
        for (uint32_t i = 0; i < n_objects; i++) {
            const uint32_t kind = rd<uint32_t>();
            double a[20];
            for (int k = 0; k < 20; k++) a[k] = rd<double>();
            const float reflection_ratio = rd<float>();
            const glm::vec3 color = rd_vec3();
            SurfaceCoefs s{};
            switch (kind) {
            case 0: memcpy(&s, a, sizeof(a)); break;
            case 1: s = SurfaceCoefs::sphere(rd_dvec3(a), a[3]); break;
            case 2: s = SurfaceCoefs::plane(rd_dvec3(a), rd_dvec3(a + 3)); break;
            case 3: s = SurfaceCoefs::dingDong(rd_dvec3(a)); break;
            case 4: s = SurfaceCoefs::clebsch(); break;
            case 5: s = SurfaceCoefs::cayley(); break;
            default: fprintf(stderr, "ref_frames: object kind %u\n", kind); return 2;
            }
            scene.objects.push_back(Object(s, reflection_ratio, color));
        }
        for (uint32_t i = 0; i < n_lights; i++) {
            const uint32_t kind = rd<uint32_t>();
            const float intensity = rd<float>();
            double v[3];
            for (int k = 0; k < 3; k++) v[k] = rd<double>();
            const glm::vec3 color = rd_vec3();
            LightSource light{};
            switch (kind) {
            case 0: light.is_spherical = intensity != 0.0f; light.p = rd_dvec3(v); light.light_color = color; break;
            case 1: light = LightSource::directional(intensity, rd_dvec3(v), color); break;
            case 2: light = LightSource::spherical(intensity, rd_dvec3(v), color); break;
            default: fprintf(stderr, "ref_frames: light kind %u\n", kind); return 2;
            }
            scene.lights.push_back(light);
        }
    } catch (const SceneException &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    static_assert(sizeof(SurfaceCoefs) == 20 * sizeof(double), "SurfaceCoefs is 20 doubles");

    FILE *out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "ref_frames: cannot write %s\n", argv[2]);
        return 2;
    }
    init_update(0, scene);
    for (uint32_t c = 0; c < n_cameras; c++) {
        glm::dmat4 cam;
        for (int col = 0; col < 4; col++)
            for (int row = 0; row < 4; row++) cam[col][row] = rd<double>();
        update(cam);
        if (fwrite(g_data.data(), sizeof(float), g_data.size(), out) != g_data.size()) return 2;
    }
    fclose(out);
    cleanup_update();
    return 0;
}
