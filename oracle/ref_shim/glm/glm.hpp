// glm/glm.hpp -- stand-in for glm, used ONLY by oracle/Makefile.ref to compile the reference's CPU
// path (update-cpu.cpp, surface.cpp, light.cpp, scene-exception.cpp) into oracle/_ref/.  Test
// infrastructure, like everything under oracle/.
//
// The reference does not vendor glm and none is installed, so the operations its CPU path uses are
// stated here with glm's names and glm's operation order, after the product's own host header
// (cuda-ray-tracer_amd/host/glm_min/glm/glm.hpp):
//     dot(vec3)      = (x*x' + y*y') + z*z'
//     normalize(v)   = v * (1 / sqrt(dot(v, v)))
//     mat4 * vec4    = (m[0]*v.x + m[1]*v.y) + (m[2]*v.z + m[3]*v.w)
//     min(x, y)      = (y < x) ? y : x          max(x, y) = (x < y) ? y : x
//     vec / scalar   = component / scalar       (no reciprocal)
// One difference from glm_min: vec3(vec4) is IMPLICIT here, as in a real glm without
// GLM_FORCE_EXPLICIT_CTOR -- the reference's update() assigns a dvec4 to a dvec3.
// That this order is a real glm's is an assumption; everything else the
// binaries under oracle/_ref/ compute is the reference's own text.
#ifndef ORACLE_REF_SHIM_GLM_HPP
#define ORACLE_REF_SHIM_GLM_HPP

#include <cmath>
#include <cstddef>

namespace glm {

enum qualifier { packed_highp, defaultp = packed_highp };

template <int L, typename T, qualifier Q = defaultp>
struct vec;

template <typename T, qualifier Q>
struct vec<3, T, Q> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    constexpr vec() : x(0), y(0), z(0) {}
    constexpr explicit vec(T s) : x(s), y(s), z(s) {}
    constexpr vec(T a, T b_, T c) : x(a), y(b_), z(c) {}
    template <typename U, qualifier P>
    constexpr vec(const vec<3, U, P> &v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
    template <typename U, qualifier P>
    constexpr vec(const vec<4, U, P> &v); // implicit: see the header comment
    T &operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    const T &operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    vec &operator+=(const vec &o) { x += o.x; y += o.y; z += o.z; return *this; }
    vec &operator-=(const vec &o) { x -= o.x; y -= o.y; z -= o.z; return *this; }
    vec &operator*=(T s) { x *= s; y *= s; z *= s; return *this; }
};

template <typename T, qualifier Q>
struct vec<4, T, Q> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    union { T w, a; };
    constexpr vec() : x(0), y(0), z(0), w(0) {}
    constexpr explicit vec(T s) : x(s), y(s), z(s), w(s) {}
    constexpr vec(T a_, T b_, T c, T d) : x(a_), y(b_), z(c), w(d) {}
    constexpr vec(const vec<3, T, Q> &v, T d) : x(v.x), y(v.y), z(v.z), w(d) {}
    T &operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    const T &operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};

template <typename T, qualifier Q>
template <typename U, qualifier P>
constexpr vec<3, T, Q>::vec(const vec<4, U, P> &v)
    : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z))
{}

#define REF_SHIM_V3 vec<3, T, Q>
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator+(const REF_SHIM_V3 &a, const REF_SHIM_V3 &b) { return REF_SHIM_V3(a.x + b.x, a.y + b.y, a.z + b.z); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator-(const REF_SHIM_V3 &a, const REF_SHIM_V3 &b) { return REF_SHIM_V3(a.x - b.x, a.y - b.y, a.z - b.z); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator*(const REF_SHIM_V3 &a, const REF_SHIM_V3 &b) { return REF_SHIM_V3(a.x * b.x, a.y * b.y, a.z * b.z); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator/(const REF_SHIM_V3 &a, const REF_SHIM_V3 &b) { return REF_SHIM_V3(a.x / b.x, a.y / b.y, a.z / b.z); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator*(const REF_SHIM_V3 &a, T s) { return REF_SHIM_V3(a.x * s, a.y * s, a.z * s); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator*(T s, const REF_SHIM_V3 &a) { return REF_SHIM_V3(s * a.x, s * a.y, s * a.z); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator/(const REF_SHIM_V3 &a, T s) { return REF_SHIM_V3(a.x / s, a.y / s, a.z / s); }
template <typename T, qualifier Q> constexpr REF_SHIM_V3 operator-(const REF_SHIM_V3 &a) { return REF_SHIM_V3(-a.x, -a.y, -a.z); }
#undef REF_SHIM_V3

#define REF_SHIM_V4 vec<4, T, Q>
template <typename T, qualifier Q> constexpr REF_SHIM_V4 operator+(const REF_SHIM_V4 &a, const REF_SHIM_V4 &b) { return REF_SHIM_V4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
template <typename T, qualifier Q> constexpr REF_SHIM_V4 operator*(const REF_SHIM_V4 &a, T s) { return REF_SHIM_V4(a.x * s, a.y * s, a.z * s, a.w * s); }
#undef REF_SHIM_V4

template <int C, int R, typename T, qualifier Q = defaultp>
struct mat;

// column-major 4x4, m[col][row]
template <typename T, qualifier Q>
struct mat<4, 4, T, Q> {
    typedef vec<4, T, Q> col_type;
    col_type value[4];
    constexpr mat() : value{col_type(1, 0, 0, 0), col_type(0, 1, 0, 0), col_type(0, 0, 1, 0), col_type(0, 0, 0, 1)} {}
    col_type &operator[](int i) { return value[i]; }
    const col_type &operator[](int i) const { return value[i]; }
};

template <typename T, qualifier Q>
constexpr vec<4, T, Q> operator*(const mat<4, 4, T, Q> &m, const vec<4, T, Q> &v)
{
    return (m[0] * v.x + m[1] * v.y) + (m[2] * v.z + m[3] * v.w);
}

typedef vec<3, float> vec3;
typedef vec<3, double> dvec3;
typedef vec<4, float> vec4;
typedef vec<4, double> dvec4;
typedef mat<4, 4, double> dmat4;

template <typename T, qualifier Q> constexpr T dot(const vec<3, T, Q> &a, const vec<3, T, Q> &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <typename T, qualifier Q> constexpr T length2(const vec<3, T, Q> &a) { return dot(a, a); }
template <typename T, qualifier Q> inline vec<3, T, Q> normalize(const vec<3, T, Q> &v) { return v * (static_cast<T>(1) / std::sqrt(dot(v, v))); }
template <typename T> constexpr T min(T a, T b) { return (b < a) ? b : a; }
template <typename T> constexpr T max(T a, T b) { return (a < b) ? b : a; }
template <typename T, qualifier Q> constexpr vec<3, T, Q> min(const vec<3, T, Q> &a, const vec<3, T, Q> &b) { return vec<3, T, Q>(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
using std::pow;

} // namespace glm

#endif
