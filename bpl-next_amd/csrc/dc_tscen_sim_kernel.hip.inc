// dc_tscen_sim_kernel.hip.inc -- the text of dc_tscen_sim<H2H, ET>, included twice by dc_tscen.hip.h: as dc_tscen_sim (DCT_SIM_ALLOC
// false, the kernel it always was) and as scen_alloc_sim (DCT_SIM_ALLOC true: the bracket is filled through a
// best-of-rest allocation table, dct::alloc_slot).  Two kernels and not a runtime branch: DESIGN.md section 42.
// Included twice more by dc_tournament_live_queries.hip.h with DCT_SIM_LIVE defined (matches in play and weighted
// draws, DESIGN.md section 44): the kernel then takes dct::LiveCup V, which every other inclusion holds as a dummy.
template <bool H2H, bool ET>
#ifdef DCT_SIM_LIVE
// (matches in play and weighted draws: dc_tournament_live_queries.hip.h; the second bound as for the dctl simulators)
__global__ __launch_bounds__(64 * TSCEN_WAVES, dct::LIVE_SIM_WAVES_PER_SIMD) void DCT_SIM_NAME(
        dct::TournamentArgs A, dch::PairArgs H, dck::KnockoutArgs K, TscenArgs P, dct::LiveCup V) {
    using namespace dct;
    constexpr bool LIVE = true;
#else
__global__ __launch_bounds__(64 * TSCEN_WAVES) void DCT_SIM_NAME(dct::TournamentArgs A, dch::PairArgs H,
                                                                 dck::KnockoutArgs K, TscenArgs P) {
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
        uint32_t cell = 0u;   // class x stride of this lane's key fixtures, over all blocks of the list
        const auto on_fixture = [&cell, fix_code = P.fix_code](int f, int p, int hs, int x, int y) -> uint32_t {
            // (x, y) is in the home orientation: a host listed second was swapped in
            const int margin = hs == p ? x - y : y - x;
            const uint32_t code = fix_code[f];
            const int cap = (int)(code >> dcsc::CODE_CAP_SHIFT);   // (0 for a fixture that is no key)
            cell += (uint32_t)(cap - min(max(margin, -cap), cap)) * (code & ((1u << dcsc::CODE_CAP_SHIFT) - 1u));
            return 0u;
        };
        const auto on_block = [](int, uint32_t) {};
        const auto on_fixtures_done = [&cell] { cell = dcsc::wave_sum_u32(cell); };   // once per simulation
        const auto on_match = [](int, int, int, int, int) {};
#include "dc_tournament_sim_play.hip.inc"
        if (lane == 0) P.scen[c] = cell;
        if (slot_lane) {
            const uint32_t st = stg[lane];
            // bits 0..R: the stage's targets; bit R + 1: first in its group
            const uint32_t top = groups && pos == 0 ? 1u << (A.rounds + 1) : 0u;
            P.tset[(size_t)lane * P.chunk + c] = (uint8_t)(((1u << st) - 1u) | top);
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
#include "dc_tournament_sim_leave.hip.inc"
}
