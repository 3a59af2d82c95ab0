// dc_paths_sim_kernel.hip.inc -- the text of dc_paths_sim<H2H, ET>, included twice by dc_paths.hip.h: as dc_paths_sim (DCT_SIM_ALLOC
// false, the kernel it always was) and as paths_alloc_sim (DCT_SIM_ALLOC true: the bracket is filled through a
// best-of-rest allocation table, dct::alloc_slot).  Two kernels and not a runtime branch: DESIGN.md section 42.
// Included twice more by dc_tournament_live_queries.hip.h with DCT_SIM_LIVE defined (matches in play and weighted
// draws, DESIGN.md section 44): the kernel then takes dct::LiveCup V, which every other inclusion holds as a dummy.
template <bool H2H, bool ET>
#ifdef DCT_SIM_LIVE
// (matches in play and weighted draws: dc_tournament_live_queries.hip.h; the second bound as for the dctl simulators)
__global__ __launch_bounds__(64 * PATHS_WAVES, dct::LIVE_SIM_WAVES_PER_SIMD) void DCT_SIM_NAME(
        dct::TournamentArgs A, dch::PairArgs H, dck::KnockoutArgs K, PathsArgs P, dct::LiveCup V) {
    using namespace dct;
    constexpr bool LIVE = true;
#else
__global__ __launch_bounds__(64 * PATHS_WAVES) void DCT_SIM_NAME(dct::TournamentArgs A, dch::PairArgs H,
                                                                 dck::KnockoutArgs K, PathsArgs P) {
    using namespace dct;
    constexpr bool LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
#endif
    constexpr bool ALLOC = DCT_SIM_ALLOC;   // (read by dc_tournament_sim_play.hip.inc)
    constexpr bool GROUPS_ONLY = false;
#include "dc_tournament_sim_enter.hip.inc"
    for (int c = (int)blockIdx.x * nw + wave; c < P.nc; c += waves) {
        const long long j = P.j0 + c;
        int s;
        if constexpr (LIVE) s = live_draw(A, V, j, lane);   // the scan's selection, or j mod S without weights
        else s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        uint32_t* rec = P.match + (size_t)c * (nb - 1);
        // (the callables capture what they read by value: with `lane` and `P` captured by reference in on_block the
        // head-to-head kernels of OTHER files came out with other code -- DESIGN.md, "The tournament family's shared paths")
        const auto on_fixture = [](int, int p, int hs, int x, int y) -> uint32_t {
            // (x, y) is in the home orientation: turned back to the listed one.  Bit 0: the first-listed side wins, bit 1:
            // the second
            const bool listed = hs == p;
            return ((listed ? x > y : y > x) ? 1u : 0u) | ((listed ? y > x : x > y) ? 2u : 0u);
        };
        const auto on_block = [lane, c, ball = P.ball, chunk = P.chunk](int b, uint32_t mark) {
            const unsigned long long fb = __ballot(mark & 1u), sb = __ballot(mark & 2u);
            if (lane == 0) {
                unsigned long long* at = ball + ((size_t)b * chunk + c) * 2;
                at[0] = fb;
                at[1] = sb;
            }
        };
        const auto on_fixtures_done = [] {};
        const auto on_match = [rec](int k, int p, int q, int win, int how) {
            rec[k] = (uint32_t)p | ((uint32_t)q << 8) | ((uint32_t)win << 16) | ((uint32_t)how << 24);
        };
#include "dc_tournament_sim_play.hip.inc"
        if (slot_lane) {
            const uint32_t st = stg[lane];
            P.slot[(size_t)c * n + lane] = (uint8_t)(st | ((uint32_t)pos << 4));
            P.tset[(size_t)c * n + lane] = (uint8_t)((1u << st) - 1u);
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
#include "dc_tournament_sim_leave.hip.inc"
}
