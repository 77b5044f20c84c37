// rt_ray_sort_key.hpp -- the key rt_sort_rays orders caller-supplied rays by (include/mi355rt.h, "Sorting rays"), and the
// sizes of its radix sort.  This header IS the definition of the key: the kernels (rt_sort_rays.hip) and the host lab
// (tests/tools/ray_sort_lab.cpp) compile it, the lab's numpy restatement is held to it bit for bit.
//
// A wave of the culled ray kernels (RT_FLAG_STREAM_CULL_RAYS) stages a chunk when ANY of its 64 rays reaches the chunk's bound, so what
// the order has to bring together is rays that start near each other and run the same way:
//   class     0 where rtm::ray_bound(o, d).cull (rt_ray_bound.hpp: the predicate of the culled kernels, not restated), else 1.  A class-1
//             ray is one nothing can be culled for -- its wave stages every chunk -- and its key is RSK_CLASS1: such rays stand together
//             at the end, in input order, and spoil at most one mixed wave.
//   box       lo, hi: the per-axis minimum and maximum of the class-0 origins, each taken after + 0.0 (so -0.0 and +0.0 are one value).
//   origin    per axis q = clamp(floor((o - lo) / (hi - lo) * 16), 0, 15), 0 where hi == lo; mo = the 12-bit Morton code of (qx, qy, qz),
//             x in the lowest bit of every triple.
//   direction n = d / (|dx| + |dy| + |dz|), the octahedral fold: where n.z < 0, (u, v) = ((1 - |n.y|) sign(n.x), (1 - |n.x|) sign(n.y)) with
//             sign(0) = +1, else (u, v) = (n.x, n.y); qu = clamp(floor((u * 0.5 + 0.5) * 512), 0, 511), qv likewise; md = the 18-bit Morton
//             code of (qu, qv), u in the lowest bit of every pair.
//   key       mo << 18 | md, 30 bits.
// All arithmetic is FP64 and must not be contracted: rt_sort_rays.hip is compiled once with -ffp-contract=off and serves strict and FAST
// contexts alike, the lab compiles with the same switch.  Every operation is one IEEE operation (division included), so host and device
// agree bit for bit.
#ifndef RT_RAY_SORT_KEY_HPP
#define RT_RAY_SORT_KEY_HPP

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_ray_bound.hpp" // ray_bound: the class

namespace rtm {

// the split of the 30 bits (the tests read it from here)
constexpr uint32_t RSK_ORIGIN_BITS = 4u; // per axis, three axes
constexpr uint32_t RSK_DIR_BITS = 9u;    // per axis, two axes
constexpr uint32_t RSK_CLASS1 = 0x80000000u;
static_assert(3u * RSK_ORIGIN_BITS + 2u * RSK_DIR_BITS == 30u, "the class-0 key has 30 bits");

// the radix sort of rt_sort_rays.hip: 8-bit digits; one workgroup of RS_THREADS lanes ranks a tile of RS_TILE (key, index) pairs per pass,
// in RS_ITEMS rounds of RS_THREADS consecutive pairs; one scan workgroup covers RS_SCAN_CHUNK entries of the digit-major histogram table
// (that many tiles of one digit) in one step
constexpr uint32_t RS_DIGIT_BITS = 8u, RS_DIGITS = 1u << RS_DIGIT_BITS, RS_PASSES = 32u / RS_DIGIT_BITS;
constexpr uint32_t RS_THREADS = 256u, RS_WAVES = RS_THREADS / 64u;
constexpr uint32_t RS_ITEMS = 8u, RS_TILE = RS_THREADS * RS_ITEMS;
constexpr uint32_t RS_SCAN_ITEMS = 8u, RS_SCAN_CHUNK = RS_THREADS * RS_SCAN_ITEMS;
static_assert(RS_DIGITS == RS_THREADS, "one lane per digit scans the tile's sub-block counts");

constexpr size_t RS_ALIGN = 256u; // every part of the work space starts on a multiple of this
constexpr uint32_t RS_MAX_LEVELS = 4u; // 2^32 / RS_TILE tiles x 256 digits = 2^29 entries = RS_SCAN_CHUNK^2.64

// ---- the work space of rt_sort_rays (host side: the launcher and the lab lay it out with this one function) ----------------------------------
// header (the six box words) | keys A | idx A | keys B | idx B | table = level 0 of the scan [256][tiles] | level 1 | ...: level k + 1 holds
// one sum per RS_SCAN_CHUNK entries of level k, the last level fits one chunk.  All offsets in bytes from the aligned base.
struct SortLayout {
    size_t tiles;
    size_t keys_a, idx_a, keys_b, idx_b;
    uint32_t levels;
    size_t level_off[RS_MAX_LEVELS], level_len[RS_MAX_LEVELS];
    size_t bytes; // with the slack that aligning the caller's pointer can take
};

inline size_t rs_align_up(size_t v) { return (v + RS_ALIGN - 1u) / RS_ALIGN * RS_ALIGN; }

inline SortLayout sort_layout(uint32_t n)
{
    SortLayout l{};
    l.tiles = ((size_t) n + RS_TILE - 1u) / RS_TILE;
    const size_t words = rs_align_up((size_t) n * sizeof(uint32_t));
    size_t at = RS_ALIGN;
    l.keys_a = at, at += words;
    l.idx_a = at, at += words;
    l.keys_b = at, at += words;
    l.idx_b = at, at += words;
    size_t len = l.tiles * RS_DIGITS;
    for (l.levels = 0; l.levels < RS_MAX_LEVELS; len = (len + RS_SCAN_CHUNK - 1u) / RS_SCAN_CHUNK) {
        l.level_off[l.levels] = at, l.level_len[l.levels] = len, at += rs_align_up(len * sizeof(uint32_t));
        l.levels++;
        if (len <= RS_SCAN_CHUNK) break;
    }
    l.bytes = at + RS_ALIGN;
    return l;
}

// the box of the class-0 origins; empty: lo = +inf, hi = -inf (no key reads it then)
struct RayKeyBox {
    double lo[3], hi[3];
};

// The order-preserving image of a double's bits as an unsigned integer (a < b <=> image(a) < image(b) for every pair that is not NaN): what
// the box kernel's 64-bit integer minimum and maximum atomics work on.
__device__ __forceinline__ uint64_t rsk_image(uint64_t bits) { return bits ^ ((bits >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull); }
__device__ __forceinline__ uint64_t rsk_unimage(uint64_t img) { return img ^ ((img >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull); }

// the low `bits` bits of v, each moved to every `step`-th place
__device__ __forceinline__ uint32_t rsk_spread(uint32_t v, uint32_t bits, uint32_t step)
{
    uint32_t r = 0u;
    for (uint32_t b = 0; b < bits; b++) r |= ((v >> b) & 1u) << (step * b);
    return r;
}

// floor(x * cells) clamped to a cell index; x is in [0, 1] up to rounding
__device__ __forceinline__ uint32_t rsk_cell(double x, uint32_t cells)
{
    const double f = floor(x * (double) cells);
    return f >= (double) (cells - 1u) ? cells - 1u : (f > 0.0 ? (uint32_t) f : 0u);
}

__device__ __forceinline__ bool ray_sort_class0(const D3 &o, const D3 &d) { return ray_bound(o, d).cull; }

__device__ __forceinline__ uint32_t ray_sort_key(const D3 &o, const D3 &d, const RayKeyBox &box)
{
    if (!ray_sort_class0(o, d)) return RSK_CLASS1;
    const double oc[3] = {o.x + 0.0, o.y + 0.0, o.z + 0.0};
    uint32_t mo = 0u;
    for (int a = 0; a < 3; a++) {
        const double w = box.hi[a] - box.lo[a];
        const uint32_t q = box.hi[a] == box.lo[a] ? 0u : rsk_cell((oc[a] - box.lo[a]) / w, 1u << RSK_ORIGIN_BITS);
        mo |= rsk_spread(q, RSK_ORIGIN_BITS, 3u) << a;
    }
    const double s = (fabs(d.x) + fabs(d.y)) + fabs(d.z);
    const double nx = d.x / s, ny = d.y / s, nz = d.z / s;
    double u = nx, v = ny;
    if (nz < 0.0) {
        u = (1.0 - fabs(ny)) * (nx < 0.0 ? -1.0 : 1.0);
        v = (1.0 - fabs(nx)) * (ny < 0.0 ? -1.0 : 1.0);
    }
    const uint32_t qu = rsk_cell(u * 0.5 + 0.5, 1u << RSK_DIR_BITS), qv = rsk_cell(v * 0.5 + 0.5, 1u << RSK_DIR_BITS);
    const uint32_t md = rsk_spread(qu, RSK_DIR_BITS, 2u) | (rsk_spread(qv, RSK_DIR_BITS, 2u) << 1);
    return (mo << (2u * RSK_DIR_BITS)) | md;
}

} // namespace rtm

#endif
