// rt_reorder_scene.hip -- rt_reorder_scene (include/mi355rt.h, "Scene updates"): the unit-sphere table the device
// holds NOW put into the order rtp::stream_cull_image (rt_scene_image.hpp) would choose for it -- bounded spheres first by the Morton key
// of their centres over the box of those centres, ties by `orig`, the others behind them by `orig` -- and the chunk bounds rebuilt, so
// that a culling context whose spheres rt_set_scene has mixed is again, byte for byte, a fresh context on the scene it holds.
//
// Compiled ONCE, with -ffp-contract=off, like rt_set_scene.hip and rt_sort_rays.hip: the key (rtp::stream_cull_key, rt_scene_pack.hpp) and
// the bounds (rtp::pack_chunk_bound) are the functions rt_create packs with on the host, and the host reproduces the bytes.  Kernels
// only: no allocation, no host read-back, no wait; every launch below is decided by (n_us, n_obj, max_grid), all fixed at rt_create.
//
// Stages (the work space's layout is reorder_layout's):
//   box      init_box_kernel sets the six box words to the reduction identities; box_kernel reduces the centres (-k / 2) of a workgroup's
//            bounded entries and merges them with 64-bit integer minimum / maximum atomics on the order-preserving image of the doubles'
//            bits (rtm::rsk_image, as rt_sort_rays.hip does): minimum and maximum do not depend on the order of arrival.  The host's
//            sequential < / > can differ from this only in the sign of a zero, which no key depends on (rt_scene_pack.hpp).
//   keys     keys_kernel: one lane per entry: the entry's 64 bytes to the copy in the work space, and its item
//            (key low word, key high word, orig, slot) -- one 16-byte vector.
//   sort     an LSD radix sort of the items by the number (key : orig), 8-bit digits, lowest first: the bytes of `orig` that n_obj - 1 has
//            (objects' indices are below n_obj, so the higher bytes are zero in every item and a pass over them would move nothing), then
//            the 8 bytes of the key.  Every pass is stable, so after the last one the items ascend by (key, orig): `orig` IS the lowest
//            digits, the sequence the sort starts from does not matter, and since no two entries share an `orig` the order is total --
//            the one sequence std::sort's comparator (key, then orig) allows.  Per pass: histogram_kernel counts a tile's digits into
//            table[digit][tile]; the exclusive scan of that digit-major table (reduce_chunks_kernel up the levels, scan_chunks_kernel down
//            them) gives the first place of every (digit, tile); scatter_kernel ranks a tile's items in input order -- round after
//            round of 256 consecutive items, inside a round wave after wave, inside a wave by a match of the digit over ballots -- and
//            stores them.  The only atomics are the histogram's integer adds in LDS.  A place is table + counts of items that exist, so
//            it is below n by construction: the histogram and the scatter read the same items.
//   permute  permute_kernel: t_us[s] = copy[item[s].slot], four lanes per entry, one 16-byte load and store each.
//   bounds   bounds_kernel: one thread per 64-entry chunk calls pack_chunk_bound, as phase 3 of set_scene_kernel does.
//
// Grids: one workgroup per 256 entries, per tile, per scan chunk or per 64 chunks, at most max_grid of them, each looping with a
// workgroup-uniform trip count (the rule of rt_ray_kernels.hpp).  The passes are rt_sort_rays.hip's, written again for 16-byte items:
// sharing them through a header would have to leave that file's code object byte for byte what it is.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include <cstdint>

#include "rt_ray_sort_key.hpp" // rsk_image / rsk_unimage: the order-preserving integer image of a double
#include "rt_scene_dev.h"
#include "rt_scene_pack.hpp"

namespace {

constexpr uint32_t RO_DIGIT_BITS = 8u, RO_DIGITS = 1u << RO_DIGIT_BITS;
constexpr uint32_t RO_THREADS = 256u, RO_WAVES = RO_THREADS / 64u;
constexpr uint32_t RO_ITEMS = 8u, RO_TILE = RO_THREADS * RO_ITEMS;                 // one workgroup ranks a tile of 2048 items per pass
constexpr uint32_t RO_SCAN_ITEMS = 8u, RO_SCAN_CHUNK = RO_THREADS * RO_SCAN_ITEMS; // one scan workgroup covers 2048 table entries
constexpr uint32_t RO_MAX_LEVELS = 4u;                                             // 2^32 / RO_TILE tiles x 256 digits = 2^29 entries < RO_SCAN_CHUNK^3
constexpr uint32_t RO_BOUND_THREADS = 64u;
constexpr size_t RO_ALIGN = 256u;
static_assert(RO_DIGITS == RO_THREADS, "one lane per digit scans the tile's sub-block counts");
static_assert(sizeof(UsEntry) == 64, "an entry moves as four 16-byte vectors");

// box words | items A | items B | the copy of the table | table = level 0 of the scan [256][tiles] | level 1 | ...: level k + 1 holds one sum
// per RO_SCAN_CHUNK entries of level k, the last level fits one chunk.  Offsets in bytes from the aligned base; sized from n_us alone.
struct ReorderLayout {
    size_t tiles;
    size_t items_a, items_b, copy;
    uint32_t levels;
    size_t level_off[RO_MAX_LEVELS], level_len[RO_MAX_LEVELS];
    size_t bytes; // with the slack that aligning the pointer can take
};

size_t align_up(size_t v) { return (v + RO_ALIGN - 1u) / RO_ALIGN * RO_ALIGN; }

ReorderLayout reorder_layout(uint32_t n)
{
    ReorderLayout l{};
    l.tiles = ((size_t) n + RO_TILE - 1u) / RO_TILE;
    size_t at = RO_ALIGN;
    l.items_a = at, at += align_up((size_t) n * sizeof(uint4));
    l.items_b = at, at += align_up((size_t) n * sizeof(uint4));
    l.copy = at, at += align_up((size_t) n * sizeof(UsEntry));
    size_t len = l.tiles * RO_DIGITS;
    for (l.levels = 0; l.levels < RO_MAX_LEVELS; len = (len + RO_SCAN_CHUNK - 1u) / RO_SCAN_CHUNK) {
        l.level_off[l.levels] = at, l.level_len[l.levels] = len, at += align_up(len * sizeof(uint32_t));
        l.levels++;
        if (len <= RO_SCAN_CHUNK) break;
    }
    l.bytes = at + RO_ALIGN;
    return l;
}

uint32_t grid_for(size_t items, uint32_t max_grid) { return (uint32_t) (items < max_grid ? items : (max_grid ? max_grid : 1u)); }

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// an item: x, y = the key's low and high word, z = orig, w = the entry's slot in the copy; its digit for byte d of the number (key : orig),
// d = 0 .. 3 the bytes of orig, 4 .. 11 those of the key
__device__ __forceinline__ uint32_t digit_of(const uint4 &it, uint32_t d)
{
    const uint32_t word = d < 4u ? it.z : (d < 8u ? it.x : it.y);
    return (word >> ((d & 3u) * RO_DIGIT_BITS)) & (RO_DIGITS - 1u);
}

// ---- box ----------------------------------------------------------------------------------------------------------------------------------
// box words: [0..2] the images of lo, [3..5] the images of hi
__global__ __launch_bounds__(64) void init_box_kernel(unsigned long long *__restrict__ box)
{
    if (threadIdx.x < 6u) box[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFFFFFFFFFull : 0ull;
}

__global__ __launch_bounds__(RO_THREADS) void box_kernel(const UsEntry *__restrict__ t_us, size_t n, unsigned long long *__restrict__ box)
{
    __shared__ uint64_t part[RO_WAVES][6];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t acc[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
    for (size_t first = (size_t) blockIdx.x * RO_THREADS; first < n; first += (size_t) gridDim.x * RO_THREADS) {
        const size_t i = first + tid;
        if (i < n) {
            const UsEntry &e = t_us[i];
            if (e.r < INFINITY) {
                const double c[3] = {-0.5 * e.kx, -0.5 * e.ky, -0.5 * e.kz};
                for (int a = 0; a < 3; a++) {
                    const uint64_t img = rtm::rsk_image((uint64_t) __double_as_longlong(c[a]));
                    acc[a] = umin64(acc[a], img);
                    acc[3 + a] = umax64(acc[3 + a], img);
                }
            }
        }
    }
    for (int a = 0; a < 6; a++) {
        uint64_t v = acc[a];
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t other = (uint64_t) __shfl_xor((unsigned long long) v, off, 64);
            v = a < 3 ? umin64(v, other) : umax64(v, other);
        }
        if (lane == 0u) part[wave][a] = v;
    }
    __syncthreads();
    if (tid < 6u) {
        uint64_t v = part[0][tid];
        for (uint32_t w = 1; w < RO_WAVES; w++) v = tid < 3u ? umin64(v, part[w][tid]) : umax64(v, part[w][tid]);
        if (tid < 3u)
            atomicMin(box + tid, (unsigned long long) v);
        else
            atomicMax(box + tid, (unsigned long long) v);
    }
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------
// (no bounded entry: the words are still the identities, lo = NaN images that no key reads -- every entry's key is ~0)
__global__ __launch_bounds__(RO_THREADS) void keys_kernel(const UsEntry *__restrict__ t_us, size_t n, const unsigned long long *__restrict__ box_words,
                                                          UsEntry *__restrict__ copy, uint4 *__restrict__ items)
{
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = __longlong_as_double((long long) rtm::rsk_unimage(box_words[a]));
        hi[a] = __longlong_as_double((long long) rtm::rsk_unimage(box_words[3 + a]));
    }
    for (size_t i = (size_t) blockIdx.x * RO_THREADS + threadIdx.x; i < n; i += (size_t) gridDim.x * RO_THREADS) {
        const UsEntry e = t_us[i];
        const uint64_t key = rtp::stream_cull_key(e, lo, hi);
        copy[i] = e;
        items[i] = make_uint4((uint32_t) key, (uint32_t) (key >> 32), e.orig, (uint32_t) i);
    }
}

// ---- one pass of the sort -------------------------------------------------------------------------------------------------------------------
// table[digit * tiles + tile] = how many of the tile's items have that digit
__global__ __launch_bounds__(RO_THREADS) void histogram_kernel(const uint4 *__restrict__ items, size_t n, size_t tiles, uint32_t d, uint32_t *__restrict__ table)
{
    __shared__ uint32_t hist[RO_DIGITS];
    const uint32_t tid = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        hist[tid] = 0u;
        __syncthreads();
        const size_t base = tile * RO_TILE;
        for (uint32_t j = 0; j < RO_ITEMS; j++) {
            const size_t i = base + (size_t) j * RO_THREADS + tid;
            if (i < n) atomicAdd(&hist[digit_of(items[i], d)], 1u); // (an integer sum: the order of arrival does not show)
        }
        __syncthreads();
        table[(size_t) tid * tiles + tile] = hist[tid];
        __syncthreads();
    }
}

// the exclusive scan of one value per lane over the workgroup; total: the sum of all 256
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t) off) incl += up;
    }
    if (lane == 63u) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
    for (uint32_t w = 0; w < RO_WAVES; w++) {
        const uint32_t s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads(); // (wave_sums is free again)
    return before + incl - v;
}

// sums[chunk] = the sum of the chunk's entries of data[0 .. len)
__global__ __launch_bounds__(RO_THREADS) void reduce_chunks_kernel(const uint32_t *__restrict__ data, size_t len, size_t chunks, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wave_sums[RO_WAVES];
    const uint32_t tid = threadIdx.x;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const size_t at = chunk * RO_SCAN_CHUNK + (size_t) tid * RO_SCAN_ITEMS;
        uint32_t s = 0u;
        for (uint32_t k = 0; k < RO_SCAN_ITEMS; k++)
            if (at + k < len) s += data[at + k];
        uint32_t total;
        block_exclusive_scan(s, wave_sums, total);
        if (tid == 0u) sums[chunk] = total;
    }
}

// data[0 .. len) becomes its exclusive scan: chunk by chunk, each from offs[chunk] (the scanned level above; NULL: one chunk, from 0)
__global__ __launch_bounds__(RO_THREADS) void scan_chunks_kernel(uint32_t *__restrict__ data, size_t len, size_t chunks, const uint32_t *__restrict__ offs)
{
    __shared__ uint32_t wave_sums[RO_WAVES];
    const uint32_t tid = threadIdx.x;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const size_t at = chunk * RO_SCAN_CHUNK + (size_t) tid * RO_SCAN_ITEMS;
        uint32_t v[RO_SCAN_ITEMS], s = 0u;
        for (uint32_t k = 0; k < RO_SCAN_ITEMS; k++) {
            v[k] = at + k < len ? data[at + k] : 0u;
            s += v[k];
        }
        uint32_t total;
        uint32_t run = block_exclusive_scan(s, wave_sums, total) + (offs ? offs[chunk] : 0u);
        for (uint32_t k = 0; k < RO_SCAN_ITEMS; k++) {
            if (at + k < len) data[at + k] = run;
            run += v[k];
        }
    }
}

// The tile's items to their places.  Round j takes the items base + j * 256 + tid; sub-block (j, wave) is 64 consecutive items.  count[j * 4
// + wave][digit] first holds how many items of the sub-block have the digit (written by the lowest lane that has it), then -- one lane per
// digit running over the sub-blocks in input order from table[digit][tile] -- the place of the sub-block's first such item.
__global__ __launch_bounds__(RO_THREADS) void scatter_kernel(const uint4 *__restrict__ in, size_t n, size_t tiles, uint32_t d, const uint32_t *__restrict__ table,
                                                             uint4 *__restrict__ out)
{
    __shared__ uint32_t count[RO_ITEMS * RO_WAVES][RO_DIGITS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (uint32_t s = 0; s < RO_ITEMS * RO_WAVES; s++) count[s][tid] = 0u;
        __syncthreads();
        const size_t base = tile * RO_TILE;
        uint32_t rank[RO_ITEMS], dg[RO_ITEMS];
        for (uint32_t j = 0; j < RO_ITEMS; j++) {
            const size_t i = base + (size_t) j * RO_THREADS + tid;
            const bool live = i < n;
            dg[j] = live ? digit_of(in[i], d) : 0u;
            uint64_t same = __ballot(live); // the lanes of this wave that hold an item with this lane's digit
            for (uint32_t b = 0; b < RO_DIGIT_BITS; b++) {
                const bool bit = (dg[j] >> b) & 1u;
                const uint64_t set = __ballot(bit);
                same &= bit ? set : ~set;
            }
            rank[j] = (uint32_t) __popcll(same & below);
            if (live && rank[j] == 0u) count[j * RO_WAVES + wave][dg[j]] = (uint32_t) __popcll(same);
        }
        __syncthreads();
        uint32_t run = table[(size_t) tid * tiles + tile];
        for (uint32_t s = 0; s < RO_ITEMS * RO_WAVES; s++) {
            const uint32_t c = count[s][tid];
            count[s][tid] = run;
            run += c;
        }
        __syncthreads();
        for (uint32_t j = 0; j < RO_ITEMS; j++) {
            const size_t i = base + (size_t) j * RO_THREADS + tid;
            if (i < n) {
                const size_t at = (size_t) count[j * RO_WAVES + wave][dg[j]] + rank[j];
                out[at] = in[i]; // (read again: eight items would be 32 registers a lane held across the barriers)
            }
        }
        __syncthreads();
    }
}

// ---- permute and bounds -----------------------------------------------------------------------------------------------------------------------
// t_us[s] = copy[order[s].w]: four lanes per entry, each one 16-byte vector of it
__global__ __launch_bounds__(RO_THREADS) void permute_kernel(const uint4 *__restrict__ order, size_t n, const uint4 *__restrict__ copy, uint4 *__restrict__ t_us)
{
    const size_t vectors = n * 4u;
    for (size_t j = (size_t) blockIdx.x * RO_THREADS + threadIdx.x; j < vectors; j += (size_t) gridDim.x * RO_THREADS) {
        const uint32_t slot = reinterpret_cast<const uint32_t *>(order)[j | 3u]; // (item j >> 2, word 3)
        t_us[j] = copy[(size_t) slot * 4u + (j & 3u)];
    }
}

__global__ __launch_bounds__(RO_BOUND_THREADS) void bounds_kernel(const UsEntry *__restrict__ t_us, uint32_t n, uint32_t n_chunks, UsEntry *__restrict__ bounds)
{
    for (uint32_t c = blockIdx.x * RO_BOUND_THREADS + threadIdx.x; c < n_chunks; c += gridDim.x * RO_BOUND_THREADS) {
        const uint32_t first = 64u * c, m = n - first < 64u ? n - first : 64u;
        UsEntry b;
        rtp::pack_chunk_bound(b, t_us + first, m, c);
        bounds[c] = b;
    }
}

} // namespace

extern "C" size_t rt_reorder_scene_work_size(uint32_t n_us) { return n_us ? reorder_layout(n_us).bytes : 0u; }

// t_us: the n_us entries of the blob's unit-sphere table (16-byte aligned); bounds: the ceil(n_us / 64) chunk bounds; work: at least
// rt_reorder_scene_work_size(n_us) bytes; n_us > 0, every orig < n_obj
extern "C" hipError_t rt_launch_reorder_scene(void *t_us_, uint32_t n_us, uint32_t n_obj, void *bounds, void *work, uint32_t max_grid, hipStream_t stream)
{
    const size_t n = n_us;
    if (n == 0u || n_obj == 0u) return hipErrorInvalidValue;
    const ReorderLayout l = reorder_layout(n_us);
    unsigned char *base = (unsigned char *) (((uintptr_t) work + RO_ALIGN - 1u) / RO_ALIGN * RO_ALIGN);
    UsEntry *t_us = (UsEntry *) t_us_;
    unsigned long long *box = (unsigned long long *) base;
    uint4 *items[2] = {(uint4 *) (base + l.items_a), (uint4 *) (base + l.items_b)};
    UsEntry *copy = (UsEntry *) (base + l.copy);
    uint32_t *level[RO_MAX_LEVELS];
    size_t chunks[RO_MAX_LEVELS];
    for (uint32_t k = 0; k < l.levels; k++) {
        level[k] = (uint32_t *) (base + l.level_off[k]);
        chunks[k] = (l.level_len[k] + RO_SCAN_CHUNK - 1u) / RO_SCAN_CHUNK;
    }
    const dim3 block(RO_THREADS), per_entry(grid_for((n + RO_THREADS - 1u) / RO_THREADS, max_grid)), per_tile(grid_for(l.tiles, max_grid));

    hipLaunchKernelGGL(init_box_kernel, dim3(1), dim3(64), 0, stream, box);
    hipLaunchKernelGGL(box_kernel, per_entry, block, 0, stream, t_us, n, box);
    hipLaunchKernelGGL(keys_kernel, per_entry, block, 0, stream, t_us, n, box, copy, items[0]);
    // the digits, lowest first: the bytes of orig that n_obj - 1 has, then the key's eight
    uint32_t digits[12], n_digits = 0u;
    for (uint32_t top = n_obj - 1u, d = 0u; d == 0u || (top >> (d * RO_DIGIT_BITS)) != 0u; d++) {
        digits[n_digits++] = d;
        if (d == 3u) break;
    }
    for (uint32_t d = 4u; d < 12u; d++) digits[n_digits++] = d;
    uint32_t cur = 0u;
    for (uint32_t pass = 0; pass < n_digits; pass++, cur ^= 1u) {
        const uint4 *in = items[cur];
        uint4 *out = items[cur ^ 1u];
        const uint32_t d = digits[pass];
        hipLaunchKernelGGL(histogram_kernel, per_tile, block, 0, stream, in, n, l.tiles, d, level[0]);
        for (uint32_t k = 0; k + 1u < l.levels; k++)
            hipLaunchKernelGGL(reduce_chunks_kernel, dim3(grid_for(chunks[k], max_grid)), block, 0, stream, level[k], l.level_len[k], chunks[k], level[k + 1u]);
        for (uint32_t k = l.levels; k-- > 0u;)
            hipLaunchKernelGGL(scan_chunks_kernel, dim3(grid_for(chunks[k], max_grid)), block, 0, stream, level[k], l.level_len[k], chunks[k],
                               k + 1u < l.levels ? level[k + 1u] : nullptr);
        hipLaunchKernelGGL(scatter_kernel, per_tile, block, 0, stream, in, n, l.tiles, d, level[0], out);
    }
    hipLaunchKernelGGL(permute_kernel, dim3(grid_for((n * 4u + RO_THREADS - 1u) / RO_THREADS, max_grid)), block, 0, stream, items[cur], n, (const uint4 *) copy, (uint4 *) t_us);
    const uint32_t n_chunks = (n_us + 63u) / 64u;
    hipLaunchKernelGGL(bounds_kernel, dim3(grid_for((n_chunks + RO_BOUND_THREADS - 1u) / RO_BOUND_THREADS, max_grid)), dim3(RO_BOUND_THREADS), 0, stream, t_us, n_us, n_chunks,
                       (UsEntry *) bounds);
    return hipGetLastError();
}
