// dc_tournament_sim_enter.hip.inc -- the per-workgroup scaffold of a recording tournament kernel, as text (see
// dc_tournament_sim.hip.h).  Reads A, H and the flags H2H, ET, GROUPS_ONLY and LIVE; ends with a barrier.
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[SIM_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[SIM_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[SIM_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63;
    int wave = threadIdx.x >> 6;
    // (LIVE: the wave's index, and with it the simulation, the draw and the wave's LDS rows, is handed to the scalar
    // unit: held per lane these wave-uniform values cost the vector registers the conditional sampler needs)
    if constexpr (LIVE) wave = __builtin_amdgcn_readfirstlane(wave);
    const int nw = H2H ? (int)(blockDim.x >> 6) : SIM_WAVES;
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    if constexpr (ET) {
        if (threadIdx.x < dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS) dck::decided_hist()[threadIdx.x] = 0u;
    }
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS; i += blockDim.x) sinfo[i] = i < n ? A.slot_info[i] : 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_CODES; i += blockDim.x)
        code_pos[i] = GROUPS_ONLY || A.n_groups ? A.code_pos[i] : (uint8_t)0xFF;
    __syncthreads();


    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    uint8_t* br = bracket[wave];
    uint8_t* stg = stage[wave];
    const bool slot_lane = lane < n;
    const bool groups = GROUPS_ONLY || A.n_groups > 0;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane && groups);
    const int my_group = slot_lane ? (int)(sinfo[lane] >> 25) : -1;
    const int first_slot = !groups && lane < nb ? (int)A.first_round[lane] : 0;
    const int advance = A.advance;
    const int waves = (int)gridDim.x * nw;   // the stride of a wave over the simulations
