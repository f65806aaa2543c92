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

// What the kernels that walk the tile cores in rectangles of bw x bh pixels, one block each, launch on (the finish kernel of hull.hip,
// the apply kernels of region_ring.h): nbx x nby rectangles per core, napply blocks in all.  With counts the cores are the grid's;
// without, cores of 2^20 pixels a side with no tile behind them.
struct ApplyGrid {
    PageGrid g;
    int nbx, nby;
    int64_t napply;
};
static inline ApplyGrid make_apply_grid(int h, int w, int tile, int halo, const int* core_count, int bw, int bh) {
    ApplyGrid a;
    if (core_count != nullptr) a.g = make_grid(h, w, tile, halo);
    else {
        a.g.h = h; a.g.w = w; a.g.tile = a.g.s = 1 << 20; a.g.halo = 0;
        a.g.ty = (int)cdiv64(h, a.g.s); a.g.tx = (int)cdiv64(w, a.g.s);
    }
    a.nbx = cdiv(a.g.s < w ? a.g.s : w, bw); a.nby = cdiv(a.g.s < h ? a.g.s : h, bh);
    a.napply = (int64_t)a.g.ty * a.g.tx * a.nbx * a.nby;
    return a;
}
// the counts of all cores to 0 (nothing to do without counts); false: the memset did not start
static inline bool clear_core_count(int* core_count, const PageGrid& g, hipStream_t st) {
    return core_count == nullptr || hipMemsetAsync(core_count, 0, sizeof(int) * (size_t)g.ty * g.tx, st) == hipSuccess;
}

}  // namespace tsii
