// dc_h2h.hip.h -- head-to-head tie-breaks (tiebreak="head_to_head" of simulate_season, match_leverage and
// simulate_tournament): the per-pair record of one simulation and the ranking that uses it.  dc_season,
// dc_leverage_sim and dc_tournament are templates over the tie-break; their H2H = true instantiations add the
// three statements below (pair_reset, pair_book, pair_rank) to the one simulate-and-rank loop.  Under one key
// simulation j is therefore the same in both modes up to the ranking: the same draw j mod S, the same threefry
// blocks (j, f), scorelines, points and tie-break word (tests/test_gpu_h2h.py compares them bit for bit).
//
// The pair matrix: pair[i][k] = points i took from k << 16 | goals i scored against k, over every match
// between the two -- those already played (pair_init, from the host) and those of this simulation.  One u32
// per ordered pair, n rows of `pitch` = n | 1 words in DYNAMIC LDS, private to a wave.  The host bounds every
// half to 16 bits before any launch (played + remaining meetings x the largest value of a match), so the goals
// never carry into the points.
//   reset    lane = column: row by row from pair_init (zero without one), at the start of EVERY simulation;
//   booking  lane = fixture: one integer LDS atomic per side per match (a pair can meet twice in a simulation,
//            two lanes can share a cell);
//   ranking  lane = slot i walks the wave-uniform slots k: where k is level on points (and of the same group)
//            it adds pair[i][k]'s halves and pair[k][i]'s goals -- the mini-table over ALL slots level with
//            i, formed once.  pair[i][k] has lane stride = pitch, which is odd: the 64 lanes fall into
//            distinct banks (a pitch of 64 would put them all into one); pair[k][i] has lane stride 1.
// Order: points, head-to-head points, head-to-head goal difference, head-to-head goals, overall goal
// difference, overall goals for (all descending), the tie-break word descending, slot ascending.  Two slots
// compare on the head-to-head keys only when level on points, and then they share the mini-table, so the
// lexicographic compare is a total order.  The callers place dcr::wave_lds_order() between reset, booking and
// reading, as for the table rows.
//
// LDS: a wave's matrix is 4 n (n | 1) bytes -- 1680 B at n = 20, 9408 B at n = 48, 16 640 B at n = 64.  Up to
// H2H_SMALL_TEAMS slots a workgroup has four waves as in the overall order, above it two, so that the dynamic
// part stays below 38 KB and a workgroup's total below 64 KB (DESIGN.md §21 has the occupancy).
// Integer atomics only, every add commutative: the outputs are bit-identical whatever the schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_sampler.hip.h"     // dcr::readlane_u64
#include "dc_table.hip.h"       // dctab::Row, TABLE_MAX_TEAMS

namespace dch {

constexpr int H2H_MAX_WAVES = 4;
constexpr int H2H_SMALL_TEAMS = 48;      // more slots than this: two waves per workgroup
constexpr int H2H_BLOCKS_PER_CU = 4;
constexpr uint32_t H2H_HALF = 0xFFFFu;   // a half of a pair record
constexpr int H2H_MAX_GOALS = 255;       // dcr::sample_scoreline's cap

struct PairArgs {
    const uint32_t* init;   // DEVICE u32 [n, n] or null (all zero); the diagonal is never read
    int pitch;              // n | 1
};

inline int waves_for(int n) { return n <= H2H_SMALL_TEAMS ? H2H_MAX_WAVES : 2; }
inline int pitch_for(int n) { return n | 1; }
inline size_t lds_bytes(int n) { return (size_t)waves_for(n) * n * pitch_for(n) * sizeof(uint32_t); }
// the largest dynamic part (n = H2H_SMALL_TEAMS with four waves, n = 64 with two) on top of the largest static
// part (dc_season<true>: 20 KB) stays within the 64 KB every launch may ask for without an attribute
static_assert(H2H_MAX_WAVES * H2H_SMALL_TEAMS * (H2H_SMALL_TEAMS | 1) * 4 + 20 * 1024 <= 64 * 1024, "four-wave matrices");
static_assert(2 * dctab::TABLE_MAX_TEAMS * (dctab::TABLE_MAX_TEAMS | 1) * 4 + 20 * 1024 <= 64 * 1024, "two-wave matrices");

__device__ __forceinline__ void pair_reset(uint32_t* pair, const PairArgs& H, int n, int lane) {
    if (lane < n)
        for (int i = 0; i < n; ++i) pair[i * H.pitch + lane] = H.init ? H.init[i * n + lane] : 0u;
}
// a match hs v as that ended x : y
__device__ __forceinline__ void pair_book(uint32_t* pair, int pitch, int hs, int as, int x, int y, int win, int draw,
                                          int loss) {
    const uint32_t hp = (uint32_t)(x > y ? win : x == y ? draw : loss), ap = (uint32_t)(y > x ? win : x == y ? draw : loss);
    atomicAdd(&pair[hs * pitch + as], (hp << 16) | (uint32_t)x);
    atomicAdd(&pair[as * pitch + hs], (ap << 16) | (uint32_t)y);
}
// lane = slot: the number of slots ahead of it (GROUPED: of its group) under the eight keys
template <bool GROUPED>
__device__ __forceinline__ int pair_rank(const uint32_t* pair, int pitch, int n, int lane, bool slot_lane,
                                         const dctab::Row& row, uint32_t r0, int group) {
    int32_t hp = 0, hgf = 0, hga = 0;   // against the slots level on points
    for (int k = 0; k < n; ++k) {
        const int32_t pk = __builtin_amdgcn_readlane(row.pts, k);
        const int gk = GROUPED ? __builtin_amdgcn_readlane(group, k) : 0;
        if (slot_lane && k != lane && pk == row.pts && (!GROUPED || gk == group)) {
            const uint32_t w = pair[lane * pitch + k], v = pair[k * pitch + lane];
            hp += (int32_t)(w >> 16);
            hgf += (int32_t)(w & H2H_HALF);
            hga += (int32_t)(v & H2H_HALF);
        }
    }
    // (points, head-to-head points), (head-to-head GD + 2^31, head-to-head goals), (GD + 2^31, GF), word
    const unsigned long long k1 = ((unsigned long long)(uint32_t)row.pts << 32) | (uint32_t)hp;
    const unsigned long long k2 = ((unsigned long long)(uint32_t)((hgf - hga) ^ (int32_t)0x80000000) << 32) | (uint32_t)hgf;
    const unsigned long long k3 =
        ((unsigned long long)(uint32_t)((row.gf - row.ga) ^ (int32_t)0x80000000) << 32) | (uint32_t)row.gf;
    int ahead = 0;
    for (int k = 0; k < n; ++k) {
        const unsigned long long o1 = dcr::readlane_u64(k1, k), o2 = dcr::readlane_u64(k2, k), o3 = dcr::readlane_u64(k3, k);
        const uint32_t ok = (uint32_t)__builtin_amdgcn_readlane((int)r0, k);
        const int gk = GROUPED ? __builtin_amdgcn_readlane(group, k) : 0;
        const bool better =
            o1 > k1 ||
            (o1 == k1 && (o2 > k2 || (o2 == k2 && (o3 > k3 || (o3 == k3 && (ok > r0 || (ok == r0 && k < lane)))))));
        ahead += ((!GROUPED || gk == group) && better) ? 1 : 0;
    }
    return ahead;
}

}  // namespace dch
