// er_adaptive.h -- launch wrappers of the adaptive-sampling kernels (er_adaptive.hip; include/eleven_hip.h er_adaptive_set).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct DevScene;

// Words of a tile list as the adaptive kernels keep it: [0] tile count, [1] largest error among the tiles kept (float bits; -1 if
// none was tested), [ER_AD_LIST ..] the tiles in ascending order.  A list of `tiles` tiles takes ER_AD_LIST + tiles words.
#define ER_AD_LIST 2u

// `list` is a device tile list in that layout and `count` its tile count (list[0]).
// snap[i * 64 + lane] <- BEAUTY rgb of pixel `lane` of the i-th tile, .w = its samples-plane value (bits); one wave per tile
void er_launch_adaptive_snapshot(const DevScene& S, const uint32_t* list, uint32_t count, float4* snap, hipStream_t stream);
// The convergence test of the tiles of `list` against their snapshot: tile_error[tile] <- E (or -1: no testable pixel), keep[i] <- 1
// iff the i-th tile stays active; then the compaction of the kept tiles into `out`, another list (keep: `count` words).
void er_launch_adaptive_test(const DevScene& S, const uint32_t* list, uint32_t count, const float4* snap, float threshold, float* tile_error,
                             uint32_t* keep, uint32_t* out, hipStream_t stream);
