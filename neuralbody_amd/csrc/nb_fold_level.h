// nb_fold_level.h — a sample's place in one pyramid level, in the folded first layer's own arithmetic: shared by the march
// (nb_march_fold.hip: boxes, trilinear weights) and the last-sample fix-up (nb_march_fixup.hip), which must index and weight
// the same voxels bit for bit.
#pragma once
#include "nb_march_common.h"

namespace nbm {

// unnorm_clamped (nb_march_common.h) with the level's (float)(size - 1) and (float)size + 1 given
__device__ __forceinline__ float unnorm_s(float gcoord, float fm1, float fp1) {
    const float i = __fmul_rn(__fdiv_rn(__fadd_rn(gcoord, 1.f), 2.f), fm1);
    return fminf(fmaxf(i, -2.f), fp1);
}

// the lane's pyramid level (part): sizes, unnormalisation constants, index grid, first U row
struct Lvl {
    int D, H, W;
    float fmx, fmy, fmz, fpx, fpy, fpz;
    const int *grid;
    int rbase;
};
struct LvlIdx {
    float ix, iy, iz;
    int x0, y0, z0;
};
__device__ __forceinline__ LvlIdx level_index(const Lvl &lv, const GridCoord &g) {
    LvlIdx q;
    q.ix = unnorm_s(g.gw, lv.fmx, lv.fpx);
    q.iy = unnorm_s(g.gh, lv.fmy, lv.fpy);
    q.iz = unnorm_s(g.gd, lv.fmz, lv.fpz);
    q.x0 = (int)floorf(q.ix);
    q.y0 = (int)floorf(q.iy);
    q.z0 = (int)floorf(q.iz);
    return q;
}

}  // namespace nbm
