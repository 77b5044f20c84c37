// rt_group_bounds.hip -- the group bounds of an RT_FLAG_STREAM_CULL_GROUPS context rebuilt on the device (include/mi355rt.h, "Grouped
// chunk bounds"): group G's bound is rtp::pack_chunk_bound over chunk bounds 64 G .. with orig = G, the function and
// the bytes of rtp::stream_group_image (rt_scene_image.hpp) on the host.  The host enqueues it behind rt_launch_set_scene and behind
// rt_launch_reorder_scene, which rebuild the chunk bounds it reads; neither of those files knows about groups.
//
// Compiled ONCE, with -ffp-contract=off, like rt_set_scene.hip and rt_reorder_scene.hip: the bounds are the scene's, not the variant's.
// One kernel, no allocation, no host read-back, no wait: capturable.  One thread per group; a group's members are 64 consecutive 64-byte
// records, read once.
#include <hip/hip_runtime.h>
#include "rt_launch.h" // the launcher below, as the host sees it
#include <cstdint>

#include "rt_scene_dev.h"
#include "rt_scene_pack.hpp"

namespace {

constexpr uint32_t GB_THREADS = 64u, GB_FANOUT = 64u;

__global__ __launch_bounds__(GB_THREADS) void group_bounds_kernel(const UsEntry *__restrict__ bounds, uint32_t n_chunks, uint32_t n_groups, UsEntry *__restrict__ groups)
{
    const uint32_t G = blockIdx.x * GB_THREADS + threadIdx.x;
    if (G >= n_groups) return;
    const uint32_t first = GB_FANOUT * G, m = n_chunks - first < GB_FANOUT ? n_chunks - first : GB_FANOUT;
    UsEntry b;
    rtp::pack_chunk_bound(b, bounds + first, m, G);
    groups[G] = b;
}

} // namespace

// bounds: the n_chunks chunk bounds as the stream holds them at this point; groups: ceil(n_chunks / 64) records to write
extern "C" hipError_t rt_launch_group_bounds(const void *bounds, uint32_t n_chunks, void *groups, hipStream_t stream)
{
    if (n_chunks == 0u) return hipSuccess;
    if (!bounds || !groups) return hipErrorInvalidValue;
    const uint32_t n_groups = (n_chunks + GB_FANOUT - 1u) / GB_FANOUT;
    hipLaunchKernelGGL(group_bounds_kernel, dim3((n_groups + GB_THREADS - 1u) / GB_THREADS), dim3(GB_THREADS), 0, stream, (const UsEntry *) bounds, n_chunks, n_groups,
                       (UsEntry *) groups);
    return hipGetLastError();
}
