// partition_plan.h — the index arithmetic of the stable partition (partition.h)
// that route_plan.h, group_plan.h and match_plan.h share. Plain C++ without
// HIP headers, as they are: the host probes compile it.
#pragma once

#include <stdint.h>

#include "extent.h"

namespace onc {

ONC_HD inline uint64_t tile_count(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }
// The scratch holds the tiles' counts bin-major: one scan over it in memory
// order is the stable order of the elements (bin, then tile, then rank).
ONC_HD inline uint64_t bin_count_at(uint32_t bin, uint64_t tile, uint64_t tiles) { return uint64_t(bin) * tiles + tile; }

}  // namespace onc
