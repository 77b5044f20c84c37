// reorder_lab.cpp -- the key the unit-sphere table of a culling context is ordered by (csrc/rt_scene_pack.hpp: rtp::stream_cull_key), compiled
// for the host exactly as rt_create compiles it: what the kernel of rt_reorder_scene calls on the device.  Driver: tests/tools/reorder_lab.py.
#include <cstdint>

#include "rt_scene_pack.hpp"

// entries: n UsEntry records (64 bytes each); lo, hi: the box; out: n keys
extern "C" void lab_stream_cull_keys(uint64_t n, const UsEntry *entries, const double *lo, const double *hi, uint64_t *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = rtp::stream_cull_key(entries[i], lo, hi);
}
