// dc_gpts_sim_kernel.hip.inc -- the text of dc_gpts_sim<H2H, ET>, included twice by dc_group_points.hip.h: as dc_gpts_sim (DCT_SIM_ALLOC
// false, the kernel it always was) and as points_alloc_sim (DCT_SIM_ALLOC true: the bracket is filled through a
// best-of-rest allocation table, dct::alloc_slot).  Two kernels and not a runtime branch: DESIGN.md section 42.
// Included twice more by dc_tournament_live_queries.hip.h with DCT_SIM_LIVE defined (matches in play and weighted
// draws, DESIGN.md section 44): the kernel then takes dct::LiveCup V, which every other inclusion holds as a dummy.
template <bool H2H, bool ET>
#ifdef DCT_SIM_LIVE
// (matches in play and weighted draws: dc_tournament_live_queries.hip.h; the second bound as for the dctl simulators)
__global__ __launch_bounds__(64 * GPTS_WAVES, dct::LIVE_SIM_WAVES_PER_SIMD) void DCT_SIM_NAME(
        dct::TournamentArgs A, dch::PairArgs H, dck::KnockoutArgs K, GptsArgs P, dct::LiveCup V) {
    using namespace dct;
    constexpr bool LIVE = true;
#else
__global__ __launch_bounds__(64 * GPTS_WAVES) void DCT_SIM_NAME(dct::TournamentArgs A, dch::PairArgs H,
                                                               dck::KnockoutArgs K, GptsArgs P) {
    using namespace dct;
    constexpr bool LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
#endif
    constexpr bool ALLOC = DCT_SIM_ALLOC;   // (read by dc_tournament_sim_play.hip.inc)
    constexpr bool GROUPS_ONLY = true;
#include "dc_tournament_sim_enter.hip.inc"
    for (int c = (int)blockIdx.x * nw + wave; c < P.nc; c += waves) {
        const long long j = P.j0 + c;
        int s;
        if constexpr (LIVE) s = live_draw(A, V, j, lane);   // the scan's selection, or j mod S without weights
        else s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        const auto on_fixture = [](int, int, int, int, int) { return 0u; };
        const auto on_block = [](int, uint32_t) {};
        const auto on_fixtures_done = [] {};
        const auto on_match = [](int, int, int, int, int) {};
#include "dc_tournament_sim_play.hip.inc"
        // ---- the record, lane = slot (pos < Z and rest_rank < B: the places of a group and the ranks of the rest
        // are permutations; the host has bounded the points axis)
        if (slot_lane) {
            const uint32_t st = stg[lane];
            const uint32_t top = pos == 0 ? 1u << (A.rounds + 1) : 0u;
            const uint32_t set = (((1u << st) - 1u) | top) & 0xFFu;
            const uint32_t v = (uint32_t)(row.pts - P.points_min) & 0xFFu;
            const uint32_t d = (uint32_t)(min(max(row.gf - row.ga, -P.cap), P.cap) + P.cap);
            const uint32_t rr = rest ? (uint32_t)rest_rank : GPTS_NO_REST;
            P.slot[(size_t)lane * P.chunk + c] = v | ((uint32_t)pos << 8) | (d << 11) | (set << 16) | (rr << 24);
            if (pos < P.Z) P.place[((size_t)my_group * P.Z + pos) * P.chunk + c] = (uint8_t)v;
            if (rest && P.best > 0 && rest_rank < P.B) P.rank[(size_t)rest_rank * P.chunk + c] = (uint16_t)(v | (d << 8));
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
#include "dc_tournament_sim_leave.hip.inc"
}
