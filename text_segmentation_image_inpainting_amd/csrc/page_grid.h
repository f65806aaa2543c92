// The K8 tile geometry of a page (include/tsii_hip.h, "page pipeline"), shared by pipeline.hip and regions.hip.
#pragma once
#include "tsii_common.h"

namespace tsii {

struct PageGrid {
    int h, w, tile, halo, s, ty, tx;
};
static inline PageGrid make_grid(int h, int w, int tile, int halo) {
    PageGrid g;
    g.h = h; g.w = w; g.tile = tile; g.halo = halo; g.s = tile - 2 * halo;
    g.ty = cdiv(h, g.s); g.tx = cdiv(w, g.s);
    return g;
}
static inline bool grid_ok(int h, int w, int tile, int halo) {
    return h > 0 && w > 0 && tile > 0 && tile % 32 == 0 && halo >= 0 && tile - 2 * halo > 0 &&
           (int64_t)h * w < (1ll << 31) - 4 && (int64_t)cdiv(h, tile - 2 * halo) * cdiv(w, tile - 2 * halo) * tile * (tile / 4) < (1ll << 31);
}

}  // namespace tsii
