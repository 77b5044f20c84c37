// ref_units.cpp -- the REFERENCE's per-ray functions and factories, one call per input row (test
// infrastructure).
//
// oracle/Makefile.ref compiles this file against the reference's header-only surface_impl.h and
// light_impl.h (host code: their __device__ macro is guarded) and links the reference's surface.cpp,
// light.cpp and scene-exception.cpp, with the stand-in headers of oracle/ref_shim/, into
// oracle/_ref/ref_units_{O2,O0}.  Every number comes out of a reference function; this file only moves
// rows in and out.  It is a separate program from ref_frames because the two headers define their
// functions non-inline, so only one translation unit of a program may include them.
//
//   ref_units <job file> <out file>
//
// Job file (little endian): char[8] "RTREFUNI", u32 op, u32 k, u64 n, then n rows of k float64.
// Out file: n rows of m float64.  float32 inputs and outputs travel widened to float64, which is exact.
//   op  function                         input row (k)                                   output row (m)
//    1  intersect_ray                    coef[20] origin[3] dir[3]                 (26)  t                    (1)
//    2  normal_vector                    coef[20] pos[3]                           (23)  n[3]                 (3)
//    3  shadow_ray                       is_spherical p[3] surface_point[3]         (7)  dir[3] (float) max_t (4)
//    4  surface_color                    is_spherical p[3] light_color[3] point[3]
//                                        norm[3] object_color[3]                   (16)  rgb[3] (float)       (3)
//    5  reflect_ray                      dir[3] normal[3]                           (6)  out[3]               (3)
//    6  SurfaceCoefs::sphere             centre[3] radius                           (4)  coef[20]            (20)
//    7  SurfaceCoefs::plane              origin[3] normal[3]                        (6)  coef[20]            (20)
//    8  SurfaceCoefs::dingDong           origin[3]                                  (3)  coef[20]            (20)
//    9  SurfaceCoefs::clebsch            (one unused value)                         (1)  coef[20]            (20)
//   10  SurfaceCoefs::cayley             (one unused value)                         (1)  coef[20]            (20)
//   11  LightSource::directional         intensity dir[3] color[3]                  (7)  is_spherical p[3] light_color[3] (7)
//   12  LightSource::spherical           intensity pos[3] color[3]                  (7)  the same             (7)
// Exit code 3 with the SceneException's text on stderr when a factory rejects its arguments.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scene-exception.h"
#include "surface_impl.h"
#include "light_impl.h"

static glm::dvec3 d3(const double *a)
{
    const double x = a[0], y = a[1], z = a[2];
    return glm::dvec3(x, y, z);
}

static glm::vec3 f3(const double *a)
{
    const float x = (float) a[0], y = (float) a[1], z = (float) a[2];
    return glm::vec3(x, y, z);
}

static SurfaceCoefs coefs(const double *a)
{
    static_assert(sizeof(SurfaceCoefs) == 20 * sizeof(double), "SurfaceCoefs is 20 doubles");
    SurfaceCoefs s;
    memcpy(&s, a, sizeof(s));
    return s;
}

static LightSource light(const double *a, bool with_color)
{
    LightSource l{};
    l.is_spherical = a[0] != 0.0;
    l.p = d3(a + 1);
    if (with_color) l.light_color = f3(a + 4);
    return l;
}

static void put3(double *o, const glm::dvec3 &v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static void put3(double *o, const glm::vec3 &v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static void put_coefs(double *o, const SurfaceCoefs &s) { memcpy(o, &s, sizeof(s)); }

static void put_light(double *o, const LightSource &l)
{
    o[0] = l.is_spherical ? 1.0 : 0.0;
    put3(o + 1, l.p);
    put3(o + 4, l.light_color);
}

static const struct { uint32_t k, m; } SHAPE[13] = {{0, 0}, {26, 1}, {23, 3}, {7, 4}, {16, 3}, {6, 3}, {4, 20}, {6, 20},
                                                    {3, 20}, {1, 20}, {1, 20}, {7, 7}, {7, 7}};

int main(int argc, char **argv)
{
    FILE *in;
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) {
        fprintf(stderr, "usage: ref_units <job file> <out file>\n");
        return 2;
    }
    char magic[8];
    uint32_t op = 0, k = 0;
    uint64_t n = 0;
    if (fread(magic, 1, 8, in) != 8 || memcmp(magic, "RTREFUNI", 8) != 0 || fread(&op, 4, 1, in) != 1 || fread(&k, 4, 1, in) != 1 ||
        fread(&n, 8, 1, in) != 1 || op < 1 || op > 12 || k != SHAPE[op].k) {
        fprintf(stderr, "ref_units: not a unit job, or a row length that does not fit its op\n");
        return 2;
    }
    const uint32_t m = SHAPE[op].m;
    std::vector<double> x((size_t) n * k), y((size_t) n * m);
    if (fread(x.data(), sizeof(double), x.size(), in) != x.size()) {
        fprintf(stderr, "ref_units: job file too short\n");
        return 2;
    }
    try {
        for (uint64_t i = 0; i < n; i++) {
            const double *a = &x[(size_t) i * k];
            double *o = &y[(size_t) i * m];
            switch (op) {
            case 1: o[0] = intersect_ray(coefs(a), d3(a + 20), d3(a + 23)); break;
            case 2: put3(o, normal_vector(coefs(a), d3(a + 20))); break;
            case 3: {
                double max_t = 0;
                const glm::vec3 dir = shadow_ray(light(a, false), d3(a + 4), max_t);
                put3(o, dir);
                o[3] = max_t;
                break;
            }
            case 4: put3(o, surface_color(light(a, true), d3(a + 7), d3(a + 10), f3(a + 13))); break;
            case 5: put3(o, reflect_ray(d3(a), d3(a + 3))); break;
            case 6: put_coefs(o, SurfaceCoefs::sphere(d3(a), a[3])); break;
            case 7: put_coefs(o, SurfaceCoefs::plane(d3(a), d3(a + 3))); break;
            case 8: put_coefs(o, SurfaceCoefs::dingDong(d3(a))); break;
            case 9: put_coefs(o, SurfaceCoefs::clebsch()); break;
            case 10: put_coefs(o, SurfaceCoefs::cayley()); break;
            case 11: put_light(o, LightSource::directional((float) a[0], d3(a + 1), f3(a + 4))); break;
            case 12: put_light(o, LightSource::spherical((float) a[0], d3(a + 1), f3(a + 4))); break;
            }
        }
    } catch (const SceneException &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(y.data(), sizeof(double), y.size(), out) != y.size()) {
        fprintf(stderr, "ref_units: cannot write %s\n", argv[2]);
        return 2;
    }
    fclose(out);
    return 0;
}
