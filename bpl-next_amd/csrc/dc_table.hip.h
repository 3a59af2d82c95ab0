// dc_table.hip.h -- the league table of one simulation, shared by dc_season and dc_tournament's group
// stage: three rows (points, GF, GA) of TABLE_MAX_TEAMS in LDS, private to a wave, booked by
// lane = fixture with integer LDS atomics (two lanes may share a slot), read back and ranked by
// lane = slot.  Order: points, goal difference, goals for (all descending), then the slot's tie-break
// word (dc_sampler.hip.h) descending, then slot ascending -- counted over wave-uniform readlanes, no
// sort.  The callers place dcr::wave_lds_order() between storing, booking and loading: none is implied.
#pragma once
#include "dc_sampler.hip.h"   // dcr::readlane_u64

namespace dctab {

constexpr int TABLE_MAX_TEAMS = 64;   // one lane per slot
struct Row { int32_t pts, gf, ga; };
// (points, GD + 2^31), (GF, tie-break word): the host bounds keep every field in 32 bits
struct Keys { unsigned long long k1, k2; };

// lane's entry of rows[3][stride] -- the caller's init[3, n] or the wave's table (zero for an inactive lane)
__device__ __forceinline__ Row load_row(const int32_t* rows, int stride, int lane, bool active) {
    return Row{active ? rows[lane] : 0, active ? rows[stride + lane] : 0, active ? rows[2 * stride + lane] : 0};
}
__device__ __forceinline__ void store_row(int32_t* tab, int lane, bool active, const Row& r) {
    if (active) {
        tab[lane] = r.pts;
        tab[TABLE_MAX_TEAMS + lane] = r.gf;
        tab[2 * TABLE_MAX_TEAMS + lane] = r.ga;
    }
}
// a match hs v as that ended x : y
__device__ __forceinline__ void book(int32_t* tab, int hs, int as, int x, int y, int win, int draw, int loss) {
    int32_t *tp = tab, *tf = tab + TABLE_MAX_TEAMS, *ta = tab + 2 * TABLE_MAX_TEAMS;
    atomicAdd(&tp[hs], x > y ? win : x == y ? draw : loss);
    atomicAdd(&tp[as], y > x ? win : x == y ? draw : loss);
    atomicAdd(&tf[hs], x);
    atomicAdd(&tf[as], y);
    atomicAdd(&ta[hs], y);
    atomicAdd(&ta[as], x);
}
__device__ __forceinline__ Keys rank_keys(const Row& r, uint32_t r0) {
    return Keys{((unsigned long long)(uint32_t)r.pts << 32) | (uint32_t)((r.gf - r.ga) ^ (int32_t)0x80000000),
                ((unsigned long long)(uint32_t)r.gf << 32) | r0};
}
// (the ranking loops stay in the kernels, predicate and all: in a helper they lost their scalar loop counter)
}  // namespace dctab
