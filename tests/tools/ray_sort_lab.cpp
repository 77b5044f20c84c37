// ray_sort_lab.cpp -- host lab behind rt_sort_rays (test infrastructure).  Two things:
//   * csrc/rt_ray_sort_key.hpp compiled for the host: the box and the keys of a set of rays, as the device forms them (lab_box, lab_keys);
//   * a plain C++ restatement of the sort of csrc/rt_sort_rays.hip over the header's constants and the header's work-space layout: the
//     per-tile histogram, the levelled exclusive scan of the digit-major table, the scatter that ranks a tile's pairs round by round, wave
//     by wave and by a match over ballots.  Every load and store goes through the one work buffer of sort_layout(n).bytes and the output
//     arrays of n words, at the device's offsets, so an index the device would get wrong is an access outside a heap block here: the
//     stand-alone program (-DRAY_SORT_LAB_MAIN, built with -fsanitize=address,undefined) runs the adversarial key sets under the
//     sanitizers and compares with std::stable_sort.
// Built and driven by tests/tools/ray_sort_lab.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "rt_ray_sort_key.hpp"

using namespace rtm;

extern "C" void lab_sort_constants(uint32_t out[8])
{
    out[0] = RS_TILE, out[1] = RS_SCAN_CHUNK, out[2] = RSK_ORIGIN_BITS, out[3] = RSK_DIR_BITS;
    out[4] = RSK_CLASS1, out[5] = RS_PASSES, out[6] = RS_THREADS, out[7] = RS_ITEMS;
}

extern "C" uint64_t lab_work_bytes(uint32_t n) { return n ? sort_layout(n).bytes : 0u; }

// rays: [n][6] doubles.  out: lo[3], hi[3]; +inf / -inf for a set without class-0 rays.
extern "C" void lab_box(uint64_t n, const double *rays, double *out)
{
    uint64_t lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull}; // the device's words and identities
    bool any = false;
    for (uint64_t i = 0; i < n; i++) {
        const double *r = rays + 6 * i;
        if (!ray_sort_class0(D3{r[0], r[1], r[2]}, D3{r[3], r[4], r[5]})) continue;
        any = true;
        for (int a = 0; a < 3; a++) {
            const double oc = r[a] + 0.0;
            uint64_t bits;
            memcpy(&bits, &oc, 8);
            const uint64_t img = rsk_image(bits);
            lo[a] = img < lo[a] ? img : lo[a];
            hi[a] = img > hi[a] ? img : hi[a];
        }
    }
    for (int a = 0; a < 3; a++) {
        const uint64_t l = rsk_unimage(lo[a]), h = rsk_unimage(hi[a]);
        memcpy(out + a, &l, 8);
        memcpy(out + 3 + a, &h, 8);
        if (!any) out[a] = INFINITY, out[3 + a] = -INFINITY;
    }
}

extern "C" void lab_keys(uint64_t n, const double *rays, uint32_t *keys)
{
    RayKeyBox box;
    double b[6];
    lab_box(n, rays, b);
    for (int a = 0; a < 3; a++) box.lo[a] = b[a], box.hi[a] = b[3 + a];
    for (uint64_t i = 0; i < n; i++) {
        const double *r = rays + 6 * i;
        keys[i] = ray_sort_key(D3{r[0], r[1], r[2]}, D3{r[3], r[4], r[5]}, box);
    }
}

// ---- the sort, restated -----------------------------------------------------------------------------------------------------------------------
namespace {

struct Emu {
    size_t n;
    SortLayout l;
    std::vector<unsigned char> work; // exactly the bytes the device is promised (from its aligned base on)
    uint32_t *at(size_t off) { return reinterpret_cast<uint32_t *>(work.data() + off); }

    void histogram(const uint32_t *keys, uint32_t shift, uint32_t *table)
    {
        for (size_t tile = 0; tile < l.tiles; tile++) {
            uint32_t hist[RS_DIGITS] = {0};
            for (uint32_t j = 0; j < RS_ITEMS; j++)
                for (uint32_t tid = 0; tid < RS_THREADS; tid++) {
                    const size_t i = tile * RS_TILE + (size_t) j * RS_THREADS + tid;
                    if (i < n) hist[(keys[i] >> shift) & (RS_DIGITS - 1u)]++;
                }
            for (uint32_t tid = 0; tid < RS_THREADS; tid++) table[(size_t) tid * l.tiles + tile] = hist[tid];
        }
    }

    void reduce_chunks(const uint32_t *data, size_t len, size_t chunks, uint32_t *sums)
    {
        for (size_t chunk = 0; chunk < chunks; chunk++) {
            uint32_t total = 0u;
            for (uint32_t tid = 0; tid < RS_THREADS; tid++) {
                const size_t a = chunk * RS_SCAN_CHUNK + (size_t) tid * RS_SCAN_ITEMS;
                for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++)
                    if (a + k < len) total += data[a + k];
            }
            sums[chunk] = total;
        }
    }

    void scan_chunks(uint32_t *data, size_t len, size_t chunks, const uint32_t *offs)
    {
        for (size_t chunk = 0; chunk < chunks; chunk++) {
            uint32_t before = offs ? offs[chunk] : 0u; // block_exclusive_scan's result for lane tid, plus the chunk's offset
            for (uint32_t tid = 0; tid < RS_THREADS; tid++) {
                const size_t a = chunk * RS_SCAN_CHUNK + (size_t) tid * RS_SCAN_ITEMS;
                uint32_t v[RS_SCAN_ITEMS], s = 0u;
                for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++) v[k] = a + k < len ? data[a + k] : 0u, s += v[k];
                uint32_t run = before;
                for (uint32_t k = 0; k < RS_SCAN_ITEMS; k++) {
                    if (a + k < len) data[a + k] = run;
                    run += v[k];
                }
                before += s;
            }
        }
    }

    void scatter(const uint32_t *keys_in, const uint32_t *idx_in, uint32_t shift, const uint32_t *table, uint32_t *keys_out, uint32_t *idx_out)
    {
        std::vector<uint32_t> count((size_t) RS_ITEMS * RS_WAVES * RS_DIGITS), rank((size_t) RS_ITEMS * RS_THREADS);
        for (size_t tile = 0; tile < l.tiles; tile++) {
            std::fill(count.begin(), count.end(), 0u);
            const size_t base = tile * RS_TILE;
            for (uint32_t j = 0; j < RS_ITEMS; j++)
                for (uint32_t wave = 0; wave < RS_WAVES; wave++) {
                    uint32_t dg[64];
                    uint64_t live = 0ull, set[RS_DIGIT_BITS] = {0ull};
                    for (uint32_t lane = 0; lane < 64u; lane++) { // the ballots of the wave
                        const size_t i = base + (size_t) j * RS_THREADS + wave * 64u + lane;
                        dg[lane] = i < n ? (keys_in[i] >> shift) & (RS_DIGITS - 1u) : 0u;
                        if (i < n) live |= 1ull << lane;
                        for (uint32_t b = 0; b < RS_DIGIT_BITS; b++)
                            if ((dg[lane] >> b) & 1u) set[b] |= 1ull << lane;
                    }
                    for (uint32_t lane = 0; lane < 64u; lane++) {
                        uint64_t same = live;
                        for (uint32_t b = 0; b < RS_DIGIT_BITS; b++) same &= ((dg[lane] >> b) & 1u) ? set[b] : ~set[b];
                        const uint32_t r = (uint32_t) __builtin_popcountll(same & ((1ull << lane) - 1ull));
                        rank[(size_t) j * RS_THREADS + wave * 64u + lane] = r;
                        if (((live >> lane) & 1ull) && r == 0u) count[((size_t) j * RS_WAVES + wave) * RS_DIGITS + dg[lane]] = (uint32_t) __builtin_popcountll(same);
                    }
                }
            for (uint32_t tid = 0; tid < RS_THREADS; tid++) {
                uint32_t run = table[(size_t) tid * l.tiles + tile];
                for (uint32_t s = 0; s < RS_ITEMS * RS_WAVES; s++) {
                    const uint32_t c = count[(size_t) s * RS_DIGITS + tid];
                    count[(size_t) s * RS_DIGITS + tid] = run;
                    run += c;
                }
            }
            for (uint32_t j = 0; j < RS_ITEMS; j++)
                for (uint32_t tid = 0; tid < RS_THREADS; tid++) {
                    const size_t i = base + (size_t) j * RS_THREADS + tid;
                    if (i >= n) continue;
                    const uint32_t d = (keys_in[i] >> shift) & (RS_DIGITS - 1u);
                    const size_t to = (size_t) count[((size_t) j * RS_WAVES + (tid >> 6)) * RS_DIGITS + d] + rank[(size_t) j * RS_THREADS + tid];
                    keys_out[to] = keys_in[i]; // (a heap block of exactly n words: a place at or beyond n is the sanitizer's to report)
                    idx_out[to] = idx_in[i];
                }
        }
    }
};

} // namespace

// keys: [n]; perm, keys_out: [n] each.  The launcher's sequence (rt_launch_sort_rays) from the keys on.
extern "C" int lab_radix_sort(uint32_t n, const uint32_t *keys, uint32_t *perm, uint32_t *keys_out)
{
    if (n == 0u) return 1;
    Emu e;
    e.n = n;
    e.l = sort_layout(n);
    e.work.assign(e.l.bytes - RS_ALIGN, 0xA5); // (the slack that aligning the caller's pointer may take is not the kernels')
    uint32_t *keys_a = e.at(e.l.keys_a), *idx_a = e.at(e.l.idx_a), *keys_b = e.at(e.l.keys_b), *idx_b = e.at(e.l.idx_b);
    uint32_t *level[RS_MAX_LEVELS];
    size_t chunks[RS_MAX_LEVELS];
    for (uint32_t k = 0; k < e.l.levels; k++) level[k] = e.at(e.l.level_off[k]), chunks[k] = (e.l.level_len[k] + RS_SCAN_CHUNK - 1u) / RS_SCAN_CHUNK;
    std::vector<uint32_t> out_keys(n), out_perm(n); // heap blocks of their own, as the caller's arrays are
    for (size_t i = 0; i < n; i++) keys_b[i] = keys[i], idx_b[i] = (uint32_t) i;
    const uint32_t *kin = keys_b, *iin = idx_b;
    for (uint32_t pass = 0; pass < RS_PASSES; pass++) {
        const bool last = pass + 1u == RS_PASSES;
        uint32_t *kout = last ? out_keys.data() : ((pass & 1u) ? keys_b : keys_a);
        uint32_t *iout = last ? out_perm.data() : ((pass & 1u) ? idx_b : idx_a);
        const uint32_t shift = pass * RS_DIGIT_BITS;
        e.histogram(kin, shift, level[0]);
        for (uint32_t k = 0; k + 1u < e.l.levels; k++) e.reduce_chunks(level[k], e.l.level_len[k], chunks[k], level[k + 1u]);
        for (uint32_t k = e.l.levels; k-- > 0u;) e.scan_chunks(level[k], e.l.level_len[k], chunks[k], k + 1u < e.l.levels ? level[k + 1u] : nullptr);
        e.scatter(kin, iin, shift, level[0], kout, iout);
        kin = kout, iin = iout;
    }
    memcpy(perm, out_perm.data(), sizeof(uint32_t) * (size_t) n);
    memcpy(keys_out, out_keys.data(), sizeof(uint32_t) * (size_t) n);
    return 0;
}

#ifdef RAY_SORT_LAB_MAIN
// The stand-alone program: adversarial key sets at the sizes the GPU tests use and beyond one scan chunk of tiles, against std::stable_sort.
static std::vector<uint32_t> key_set(int kind, uint32_t n)
{
    std::vector<uint32_t> k(n);
    uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t) kind;
    for (uint32_t i = 0; i < n; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t r = (uint32_t) (s >> 33);
        switch (kind) {
            case 0: k[i] = 0x12345u; break;                                 // all equal
            case 1: k[i] = (i & 1u) ? 0x00ABCDEFu : 0x2F000001u; break;      // two alternating
            case 2: k[i] = (r & 0x3Fu) << 24; break;                        // the top digit only
            case 3: k[i] = 0x15A5A500u | (r & 0xFFu); break;                // the lowest digit only
            case 4: k[i] = (uint32_t) (((uint64_t) i << 30) / n); break;    // already sorted
            case 5: k[i] = (uint32_t) (((uint64_t) (n - 1u - i) << 30) / n); break; // reverse sorted
            case 6: k[i] = (r % 4u == 0u) ? RSK_CLASS1 : (r & 0x3FFFFFFFu); break; // a quarter class 1
            case 7: k[i] = RSK_CLASS1; break;                               // all class 1
            default: k[i] = r & 0x3FFFFFFFu; break;                         // random 30-bit keys
        }
    }
    return k;
}

// With an argument: also one size whose scan has three levels (more than RS_SCAN_CHUNK^2 table entries; some 34 million keys).
int main(int argc, char **)
{
    const uint32_t T = RS_TILE, W = RS_SCAN_CHUNK;
    std::vector<uint32_t> sizes = {1u, 63u, 64u, 65u, T - 1u, T, T + 1u, 2u * T + 1u, 8u * T, 8u * T + 1u, 1u << 20, W * T / 8u + 1u};
    if (argc > 1) sizes.push_back(W / RS_DIGITS * W * T + 1u);
    int bad = 0;
    for (uint32_t n : sizes)
        for (int kind = 0; kind < 9; kind++) {
            if (n >= (1u << 20) && kind != 8 && kind != 1) continue; // (the large sizes twice per scan shape)
            const std::vector<uint32_t> k = key_set(kind, n);
            std::vector<uint32_t> perm(n), ks(n), want(n);
            if (lab_radix_sort(n, k.data(), perm.data(), ks.data())) return 2;
            std::iota(want.begin(), want.end(), 0u);
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
            bool ok = perm == want;
            for (uint32_t i = 0; ok && i < n; i++) ok = ks[i] == k[perm[i]];
            if (!ok) bad++, printf("ray_sort_lab: n = %u, key set %d: differs from std::stable_sort\n", n, kind);
        }
    printf("ray_sort_lab: %zu sizes x 9 key sets, scan levels at the largest size %u, %d differ\n", sizes.size(), sort_layout(sizes.back()).levels, bad);
    return bad ? 1 : 0;
}
#endif
