// What the host checks of the kernels over an enhanced suffix array share: the launch loop and the min tree.  A check defines
// TC_FM_MS_HOST_CHECK, includes its kernel header (which brings csrc/tc_fm_ms.hpp) and then this one.
#pragma once
#include "check_common.hpp"

// the lanes of a grid, one after another (a workgroup is one lane under TC_FM_MS_HOST_CHECK)
template <class F>
static void launch(u64 grid, F &&kernel) {
    for (fm_ms_block = 0; fm_ms_block < grid; fm_ms_block++) kernel();
}

// the min tree over `count` words, by the library's kernel level over level, in a block of exactly `words` entries.  The words
// of level 0 stay where the check keeps them.  view() points into this object: take it from the tree's final place.
struct MinTree {
    u32 off[FM_MS_MAXLEV + 1], cnt[FM_MS_MAXLEV + 1];
    u32 nlev = 0, words = 0, lf = 0;
    std::unique_ptr<u32[]> lmin;
    FmMsTree view(const u32 *level0) const {
        FmMsTree T;
        T.lcp = level0; T.lmin = lmin.get(); T.s_off = off; T.s_cnt = cnt; T.nlev = nlev; T.lf = lf;
        return T;
    }
};
static MinTree min_tree_of(const u32 *level0, u32 count, u32 lf) {
    MinTree t;
    t.lf = lf;
    t.nlev = fm_ms_tree_shape(count, lf, t.off, t.cnt, &t.words);
    t.lmin = block<u32>(t.words);
    const u32 *src = level0;
    for (u32 k = 1; k <= t.nlev; k++) {
        u32 *dst = t.lmin.get() + t.off[k];
        launch((t.cnt[k] + 3u) & ~3u, [&] { fm_lmin_kernel(src, t.cnt[k - 1], lf, dst, t.cnt[k]); });
        src = dst;
    }
    return t;
}
