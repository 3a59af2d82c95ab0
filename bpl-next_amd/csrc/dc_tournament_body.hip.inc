// dc_tournament_body.hip.inc -- the one body of the tournament kernels, included by dc_tournament.hip.h into
// dct::dc_tournament<H2H> (ET = false), dct::dc_tournament_et<H2H> (ET = true) and the cup_alloc pair (ALLOC), and by
// dc_tournament_live.hip.h into the eight dctl kernels (LIVE: matches in play and weighted draws).  It reads the
// including kernel's `TournamentArgs A`, `dch::PairArgs H`, `dck::KnockoutArgs K`, `LiveCup V` and the flags H2H, ET,
// ALLOC and LIVE, the flags through `if constexpr` only.  Text rather than a shared device function, so that every
// kernel reads its own argument block in place: inside a force-inlined function the redraw kernels' code moved
// (DESIGN.md section 23), as included text it is the code they had before the extra-time rule, instruction for
// instruction.
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist_stage[TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES];
    __shared__ uint32_t hist_pos[TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP];
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[TOURNAMENT_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : TOURNAMENT_WAVES;
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES; i += blockDim.x) hist_stage[i] = 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP; i += blockDim.x) hist_pos[i] = 0u;
    if constexpr (ET) {
        if (threadIdx.x < dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS) dck::decided_hist()[threadIdx.x] = 0u;
    }
    if constexpr (ALLOC) {
        for (int i = threadIdx.x; i < TOURNAMENT_MAX_GROUPS * TOURNAMENT_MAX_GROUPS; i += blockDim.x) alloc_hist()[i] = 0u;
    }
    if constexpr (H2H) {
        // a two-wave workgroup's 128 threads do not cover the 192 codes
        for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS; i += blockDim.x) sinfo[i] = i < n ? A.slot_info[i] : 0u;
        for (int i = threadIdx.x; i < TOURNAMENT_CODES; i += blockDim.x)
            code_pos[i] = A.n_groups ? A.code_pos[i] : (uint8_t)0xFF;
    } else {
        if (threadIdx.x < TOURNAMENT_MAX_TEAMS) sinfo[threadIdx.x] = threadIdx.x < n ? A.slot_info[threadIdx.x] : 0u;
        if (threadIdx.x < TOURNAMENT_CODES) code_pos[threadIdx.x] = A.n_groups ? A.code_pos[threadIdx.x] : (uint8_t)0xFF;
    }
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;   // (not formed in the overall order: even unused it changed the compiled code)
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    uint8_t* br = bracket[wave];
    uint8_t* stg = stage[wave];
    const bool slot_lane = lane < n;
    const bool groups = A.n_groups > 0;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane && groups);
    const int my_group = slot_lane ? (int)(sinfo[lane] >> 25) : -1;
    const int first_slot = !groups && lane < nb ? (int)A.first_round[lane] : 0;
    const int advance = A.advance;   // (best_of_rest lives in code_pos: ranks beyond it map to no position)

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        int s;
        if constexpr (LIVE) s = live_draw(A, V, j, lane);   // the scan's selection, or j mod S without weights
        else s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        int my_stage = 1;
        if (groups) {
            // ---- group matches, lane = fixture
            dctab::store_row(table, lane, slot_lane, init);
            if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
            dcr::wave_lds_order();
            for (int f = lane; f < nf; f += 64) {
                const uint32_t sl = A.fix[f];
                int hs, as, x, y;
                play(A, sinfo, s, ju, (uint32_t)f, (int)(sl & 0xFFu), (int)(sl >> 8), &hs, &as, &x, &y);
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            }
            if constexpr (LIVE) {
                // ---- the matches in play, lane = match: fixture F + m of the concatenated list from its state
                for (int m = lane; m < V.L; m += 64) {
                    int hs, as, x, y;
                    play_live(A, V, sinfo, s, j, m, &hs, &as, &x, &y);
                    dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                    if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                }
            }
            dcr::wave_lds_order();
            const dctab::Row row = dctab::load_row(table, TOURNAMENT_MAX_TEAMS, lane, slot_lane);
            // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
            if constexpr (!H2H) dcr::wave_lds_order();
            // ---- ranking, lane = slot: the group position, among the slots of the same group
            uint32_t r0 = 0u, r1;
            if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
            int pos = 0;
            if constexpr (H2H) {
                pos = dch::pair_rank<true>(pair, H.pitch, n, lane, slot_lane, row, r0, my_group);
                dcr::wave_lds_order();
            }
            const dctab::Keys K = dctab::rank_keys(row, r0);   // (after pair_rank: the place it compiles the same from)
            if constexpr (!H2H) {
                // (written out: in a helper the loop lost its scalar counter, dc_table.hip.h)
                for (int k = 0; k < n; ++k) {
                    const unsigned long long o1k = dcr::readlane_u64(K.k1, k), o2k = dcr::readlane_u64(K.k2, k);
                    const int gk = __builtin_amdgcn_readlane(my_group, k);
                    const bool better = o1k > K.k1 || (o1k == K.k1 && (o2k > K.k2 || (o2k == K.k2 && k < lane)));
                    pos += (gk == my_group && better) ? 1 : 0;
                }
            }
            // best of the rest: the slots placed advance + 1, ranked across the groups by the overall keys
            const int rest = slot_lane && pos == advance ? 1 : 0;
            int rest_rank = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(K.k1, k), o2k = dcr::readlane_u64(K.k2, k);
                const int rk = __builtin_amdgcn_readlane(rest, k);
                const bool better = o1k > K.k1 || (o1k == K.k1 && (o2k > K.k2 || (o2k == K.k2 && k < lane)));
                rest_rank += (rk && better) ? 1 : 0;
            }
            // ---- bracket resolution: a qualifier's code -> its first-round position
            int code = -1;
            if (slot_lane && pos < advance) code = TOURNAMENT_MAX_GROUP * my_group + pos;
            else if (rest) code = 128 + rest_rank;
            int bpos = code >= 0 && code < TOURNAMENT_CODES ? (int)code_pos[code] : 0xFF;
            if constexpr (ALLOC) {
                // an allocation table (the cup_alloc kernels): the qualifying thirds' groups select a row, and
                // ("best", k) is the row's slot k instead of the k-th best by rank.  A ranked position means "among
                // the best best_of_rest": code_pos holds no other rank
                const bool through = rest && bpos < nb;
                const int slot = alloc_slot(A, &alloc_words()[wave], lane, through, my_group);
                if (through) {
                    bpos = slot < TOURNAMENT_MAX_GROUPS ? (int)code_pos[128 + slot] : 0xFF;
                    if (slot < TOURNAMENT_MAX_GROUPS) atomicAdd(&alloc_hist()[my_group * TOURNAMENT_MAX_GROUPS + slot], 1u);
                }
            }
            my_stage = bpos < nb ? 1 : 0;
            if (bpos < nb) br[bpos] = (uint8_t)lane;
            if (slot_lane) atomicAdd(&hist_pos[lane * TOURNAMENT_MAX_GROUP + pos], 1u);
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
                if constexpr (ET) {
                    int how;
                    win = dck::decide(A, K, sinfo, s, ju, ctr, p, q, (K.legs_mask >> r) & 1u, &how);
                    atomicAdd(&dck::decided_hist()[r * dck::DECIDED_KINDS + how], 1u);
                    if (K.sim_decided) K.sim_decided[(size_t)j * (nb - 1) + k0 + lane] = (uint8_t)how;
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
            }
            dcr::wave_lds_order();   // every lane has read its pair before entry m is overwritten
            if (lane < M) {
                br[lane] = (uint8_t)win;
                stg[win] = (uint8_t)(r + 2);
            }
            dcr::wave_lds_order();
            k0 += M;
        }
        if (slot_lane) {
            const int st = stg[lane];
            atomicAdd(&hist_stage[lane * TOURNAMENT_STAGES + st], 1u);
            if (A.sim_stage) A.sim_stage[(size_t)j * n + lane] = (uint8_t)st;
        }
        if constexpr (LIVE) {
            if (V.sim_draw && lane == 0) V.sim_draw[j] = s;
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < n * TOURNAMENT_STAGES; i += blockDim.x) {
        const uint32_t v = hist_stage[i];
        if (v) atomicAdd(&A.stage_counts[i], (unsigned long long)v);
    }
    for (int i = threadIdx.x; i < n * TOURNAMENT_MAX_GROUP; i += blockDim.x) {
        const uint32_t v = hist_pos[i];
        if (v) atomicAdd(&A.pos_counts[i], (unsigned long long)v);
    }
    if constexpr (ET) {
        if (threadIdx.x < A.rounds * dck::DECIDED_KINDS) {
            const uint32_t v = dck::decided_hist()[threadIdx.x];
            if (v) atomicAdd(&K.decided_counts[threadIdx.x], (unsigned long long)v);
        }
    }
    if constexpr (ALLOC) {
        for (int i = threadIdx.x; i < TOURNAMENT_MAX_GROUPS * TOURNAMENT_MAX_GROUPS; i += blockDim.x) {
            const uint32_t v = alloc_hist()[i];
            if (v) atomicAdd(&alloc_counts(A)[i], (unsigned long long)v);
        }
    }
