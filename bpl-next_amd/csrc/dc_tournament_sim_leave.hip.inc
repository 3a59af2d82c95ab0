// dc_tournament_sim_leave.hip.inc -- the workgroup's ET histogram into K.decided_counts, as text (see
// dc_tournament_sim.hip.h)
    if constexpr (ET) {
        __syncthreads();
        if (threadIdx.x < A.rounds * dck::DECIDED_KINDS) {
            const uint32_t v = dck::decided_hist()[threadIdx.x];
            if (v) atomicAdd(&K.decided_counts[threadIdx.x], (unsigned long long)v);
        }
    }
