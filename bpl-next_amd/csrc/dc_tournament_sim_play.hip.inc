// dc_tournament_sim_play.hip.inc -- one simulation of a recording tournament kernel by one wave, as text (see
// dc_tournament_sim.hip.h): the group fixtures (lane = fixture), the table read back, the tie-break block, the group
// position by the head-to-head or the overall order, the best-of-rest rank, the bracket fill and the knockout rounds
// (lane = match) under either rule -- dc_tournament's, statement for statement.  Reads the scaffold's names, the draw
// s and the simulation ju (LIVE: also j and V), and calls the kernel's on_fixture, on_block, on_fixtures_done and
// on_match.  Leaves the lane's pos, rest, rest_rank and row, and every slot's stage in stg[]; the kernel reads stg and
// then orders the wave's LDS (dcr::wave_lds_order) before its next simulation.
// LIVE (dc_tournament_live_queries.hip.h; read through `if constexpr` only): the fixture loop goes on over the matches
// in play, and lane 0 stores the draw when asked.
    int pos = 0, rest = 0, rest_rank = 0;   // group position, "placed advance + 1", the rank among those
    dctab::Row row{};                       // the lane's row of the final group table
    int my_stage = 1;
    if (groups) {
        // ---- group matches, lane = fixture (the trip count is the wave's: on_block takes every lane)
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        // (LIVE: the list goes on with the V.L matches in play, fixture nf + m from its state -- one loop over the
        // concatenated list, so a block that holds both kinds is handed to on_block once)
        int nt = nf;
        if constexpr (LIVE) nt += V.L;
        for (int base = 0, b = 0; base < nt; base += 64, ++b) {
            const int f = base + lane;
            uint32_t mark = 0u;   // what on_fixture says of the lane's fixture, 0 for a lane without one
            if (f < nf) {
                const uint32_t sl = A.fix[f];
                const int p = (int)(sl & 0xFFu);
                int hs, as, x, y;
                play(A, sinfo, s, ju, (uint32_t)f, p, (int)(sl >> 8), &hs, &as, &x, &y);
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                mark = on_fixture(f, p, hs, x, y);
            }
            if constexpr (LIVE) {
                if (f >= nf && f < nt) {
                    int hs, as, x, y;
                    play_live(A, V, sinfo, s, j, f - nf, &hs, &as, &x, &y);
                    const int p = (int)(A.fix[f] & 0xFFu);
                    dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                    if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                    mark = on_fixture(f, p, hs, x, y);
                }
            }
            on_block(b, mark);
        }
        on_fixtures_done();
        dcr::wave_lds_order();
        row = dctab::load_row(table, TOURNAMENT_MAX_TEAMS, lane, slot_lane);
        if constexpr (!H2H) dcr::wave_lds_order();
        // ---- ranking, lane = slot
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        if constexpr (H2H) {
            pos = dch::pair_rank<true>(pair, H.pitch, n, lane, slot_lane, row, r0, my_group);
            dcr::wave_lds_order();
        }
        const dctab::Keys Q = dctab::rank_keys(row, r0);
        if constexpr (!H2H) {
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                const int gk = __builtin_amdgcn_readlane(my_group, k);
                const bool better = o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)));
                pos += (gk == my_group && better) ? 1 : 0;
            }
        }
        rest = slot_lane && pos == advance ? 1 : 0;
        for (int k = 0; k < n; ++k) {
            const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
            const int rk = __builtin_amdgcn_readlane(rest, k);
            const bool better = o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)));
            rest_rank += (rk && better) ? 1 : 0;
        }
        int code = -1;
        if (slot_lane && pos < advance) code = TOURNAMENT_MAX_GROUP * my_group + pos;
        else if (rest) code = 128 + rest_rank;
        int bpos = code >= 0 && code < TOURNAMENT_CODES ? (int)code_pos[code] : 0xFF;
        if constexpr (ALLOC) {
            // an allocation table (the *_alloc_sim kernels): dc_tournament's fill, without the slot histogram
            const bool through = rest && bpos < nb;
            const int slot = alloc_slot(A, &alloc_words()[wave], lane, through, my_group);
            if (through) bpos = slot < TOURNAMENT_MAX_GROUPS ? (int)code_pos[128 + slot] : 0xFF;
        }
        my_stage = bpos < nb ? 1 : 0;
        if (bpos < nb) br[bpos] = (uint8_t)lane;
    } else if (lane < nb) {
        br[lane] = (uint8_t)first_slot;
    }
    if (slot_lane) stg[lane] = (uint8_t)my_stage;
    dcr::wave_lds_order();
    // ---- knockout rounds, lane = match
    int k0 = 0;
    for (int r = 0; r < A.rounds; ++r) {
        const int M = nb >> (r + 1);
        int win = 0;
        if (lane < M) {
            const int p = br[2 * lane], q = br[2 * lane + 1];
            const uint32_t ctr = KNOCKOUT_COUNTER | ((uint32_t)(k0 + lane) << 5);
            int how = 0;
            if constexpr (ET) {
                win = dck::decide(A, K, sinfo, s, ju, ctr, p, q, (K.legs_mask >> r) & 1u, &how);
                atomicAdd(&dck::decided_hist()[r * dck::DECIDED_KINDS + how], 1u);
            } else {
                win = p;   // after TOURNAMENT_ATTEMPTS level attempts the first-listed side goes through
                for (int t = 0; t < TOURNAMENT_ATTEMPTS; ++t) {
                    int hs, as, x, y;
                    play(A, sinfo, s, ju, ctr | (uint32_t)t, p, q, &hs, &as, &x, &y);
                    if (x != y) {
                        win = x > y ? hs : as;
                        break;
                    }
                }
            }
            on_match(k0 + lane, p, q, win, how);
        }
        dcr::wave_lds_order();   // every lane has read its pair before entry m is overwritten
        if (lane < M) {
            br[lane] = (uint8_t)win;
            stg[win] = (uint8_t)(r + 2);
        }
        dcr::wave_lds_order();
        k0 += M;
    }
    if constexpr (LIVE) {
        if (V.sim_draw && lane == 0) V.sim_draw[j] = s;
    }
