// ccx_split_step.hip -- CollectiveCrossingEnv.step cut at the reference's own seam (collectivecrossing.py:188-261), for
// callers that put BATCHED USER CODE between the halves (array-form reward / termination / truncation strategies):
//   step_begin_kernel   :188-212  step_count += 1, the ordered move resolution, deactivation on arrival.  Writes x, y,
//                                 active, step_count; touches no flag and no output.
//   step_finish_kernel  :214-259  rewards, terminateds, truncateds (the caller's arrays, or the handle's built-in rules),
//                                 the flags, the emission set, the observation rows, __all__, optional auto-reset.
// Both are one launch each on the handle's stream: no host synchronisation, no allocation, graph-capturable.
//
// Mapping (as everywhere in libccx): one LANE per agent slot, an env inside one lane group of G = 2^glog >= N lanes of ONE
// wave, so every per-env reduction (__all__, "is my target occupied") is a ballot masked to the group.  glog is a runtime
// value here: three kernels serve every config (begin, finish x {16-byte, 8-byte row units}).
//
// begin resolves the moves with the reference's own serial loop, one move rank per iteration for all envs of the wave at
// once: the mover's packed proposal travels by one cross-lane read, the other ACTIVE agents of its env compare it with
// their cell, one ballot says "occupied" (collectivecrossing.py:536-541).  N iterations of ~10 instructions: nothing to
// stage, no LDS tables, so it serves every legal grid (W, H <= 100) -- a launch of this kind is bound by its latency
// floor, not by the loop.  Legality of a cell is the reference's arithmetic (:509-534, the rule the cell table is built
// from: ccx_step_rule.h cell_ok).
//
// finish takes the lane layout of the observe kernel (ccx_kernels.hip), the handle's launch shape and its u16 address
// table: the rows of a wave's envs are ONE contiguous region written by emit_obs, the staged 16-byte row writer.  The
// small per-agent outputs (f64 reward, flag byte, term_present byte) are staged in LDS in OUTPUT order and written by
// consecutive lanes -- 8 bytes per lane for the rewards, the byte streams as packed dwords where the wave's region is
// 4-byte aligned -- so a wave writes contiguous runs instead of N-of-G lane patterns.  The cell word (flag bits, reward
// class, terminated bit incl. ccx_set_terminated_table) comes from the handle's cell table in global memory: one 8-byte
// load per lane from a table of at most 85 KB that stays in L2.
//
// Counters: begin adds moves and arrivals, finish env / agent / live steps and episodes, each into the partial slot of its
// OWN wave index.  The two kernels cut the batch into waves differently (begin: ceil_log2(N) lane groups, 64 >> glog envs
// per wave; finish: the handle's launch shape), so a slot does not belong to one env group -- the slots are only summed.
// A malformed move order (only reachable with invalid input, counted by ccx_set_check_inputs): a slot named twice moves
// at most once (named again after it was blocked it tries again), an order byte >= N names no agent and moves nothing
// (whatever its low bits are).  The other envs of the wave are not affected.
#include "ccx_rollout_dev.h"

namespace ccx {

namespace {

// bits of a 64-lane ballot that belong to this lane's group (left in place: only compared with zero / counted)
__device__ __forceinline__ uint64_t split_group_mask(int glog, int lane) {
    if (glog >= 6) return ~0ull;
    const int G = 1 << glog;
    return ((1ull << G) - 1ull) << (lane & ~(G - 1));
}

constexpr uint32_t kSmallStageBytes = 64u * 8u + 64u + 64u;   // per wave: f64 reward, flag byte, term_present byte

}  // namespace

__global__ void __launch_bounds__(256)
step_begin_kernel(const KParams p, const KState st, const uint8_t* __restrict__ actions,
                  const uint8_t* __restrict__ order, const int glog, unsigned long long* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int G = 1 << glog, EW = 64 >> glog, N = p.N;
    const int g = lane >> glog, i = lane & (G - 1), gbase = g << glog;
    const int env = wave * EW + g;
    const bool valid_env = env < p.E;
    const bool valid = valid_env && i < N;
    const size_t idx = valid ? (size_t)env * (size_t)N + (size_t)i : 0u;

    int x = st.x[idx], y = st.y[idx];
    uint32_t act = st.active[idx] != 0 ? 1u : 0u;
    uint32_t a = actions[idx];
    uint32_t o = order ? (uint32_t)order[idx] : (uint32_t)i;      // slot of the agent that moves i-th
    if (!valid) { act = 0u; a = CCX_K_ABSENT; o = (uint32_t)i; }

    // :371-376 the proposal, from the cell the agent stands on when its turn comes (only its own move changes that)
    const int nx = x + (a == 0u ? 1 : 0) - (a == 2u ? 1 : 0);
    const int ny = y + (a == 1u ? 1 : 0) - (a == 3u ? 1 : 0);
    uint32_t ok = (act != 0u && a < 4u && cell_ok(p, nx, ny)) ? 1u : 0u;   // (wait / absent / bad bytes: no move)
    const uint32_t prop = ((uint32_t)nx & 0xFFu) | (((uint32_t)ny & 0xFFu) << 8);
    uint32_t cur = ((uint32_t)x & 0xFFu) | (((uint32_t)y & 0xFFu) << 8);
    const uint64_t gm = split_group_mask(glog, lane);
    uint32_t moved = 0u;

    for (int k = 0; k < N; ++k) {                                // :197-202 in the order of action_dict
        const uint32_t slot = order ? (uint32_t)__shfl((int)o, gbase + k, 64) : (uint32_t)k;
        const bool named = slot < (uint32_t)N;                   // (a bad order byte >= N names no agent: nothing moves)
        const int src = gbase + (named ? (int)slot : 0);
        uint32_t pk = (uint32_t)__shfl((int)(prop | (ok << 16)), src, 64);
        if (!named) pk = 0u;
        const uint32_t target = pk & 0xFFFFu;
        const bool occupied_by_me = act != 0u && cur == target && lane != src;   // :536-541: any OTHER ACTIVE agent
        const uint64_t occ = __builtin_amdgcn_ballot_w64(occupied_by_me) & gm;
        if (lane == src && (pk >> 16) != 0u && occ == 0ull) {    // :408
            cur = target;
            moved = 1u;
            ok = 0u;                                             // (a slot named twice by a bad order moves once)
        }
    }
    x = (int)(cur & 0xFFu);
    y = (int)(cur >> 8);
    // :210-212 deactivate arrivals
    const bool dest = y == (i < p.Nb ? p.bdy : p.edy);
    const bool arrive = act != 0u && dest;
    if (dest) act = 0u;
    const uint64_t moved_b = __builtin_amdgcn_ballot_w64(moved != 0u);
    const uint64_t arrive_b = __builtin_amdgcn_ballot_w64(arrive);
    if (valid) {
        st.x[idx] = x;
        st.y[idx] = y;
        st.active[idx] = (uint8_t)act;
        if (i == 0) st.step_count[env] += 1;                     // :188
    }
    if (counters && wave * EW < p.E) {
        unsigned long long* slot = counters + kCounterTotals + (size_t)wave * kCounterSlot;
        if (lane == 4 && moved_b) atomicAdd(slot + 4, (unsigned long long)__builtin_popcountll(moved_b));
        if (lane == 5 && arrive_b) atomicAdd(slot + 5, (unsigned long long)__builtin_popcountll(arrive_b));
    }
}

template <bool PAIR>
__global__ void __launch_bounds__(512)
step_finish_kernel(const KParams p, const KState st, const unsigned long long* __restrict__ cell_info,
                   const double* __restrict__ u_reward, const int8_t* __restrict__ u_term,
                   const uint8_t* __restrict__ u_trunc, const KOut out, uint8_t* __restrict__ term_present,
                   const int glog, const int auto_reset, const uint8_t* __restrict__ pool,
                   unsigned long long* __restrict__ counters) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = (int)(threadIdx.x >> 6);
    const int wave = (int)blockIdx.x * p.waves_per_block + wib;
    const int G = 1 << glog, N = p.N, L = 6 + 4 * N;
    const int g = lane >> glog, i = lane & (G - 1);
    const int env0 = wave * p.EW, env = env0 + g;
    const bool valid_env = g < p.EW && env < p.E;
    const bool valid = valid_env && i < N;
    const size_t idx = valid ? (size_t)env * (size_t)N + (size_t)i : 0u;
    const size_t env_ld = valid_env ? (size_t)env : 0u;
    // LDS: [WSlot x waves][u16 obs address table][small-output staging x waves]
    WaveLds* wl = reinterpret_cast<WaveLds*>(smem) + wib;
    const uint32_t table_bytes = (((uint32_t)p.units_per_wave + 2u) * 2u + 15u) & ~15u;
    uint16_t* table = reinterpret_cast<uint16_t*>(smem + sizeof(WaveLds) * (size_t)p.waves_per_block);
    unsigned char* small = smem + sizeof(WaveLds) * (size_t)p.waves_per_block + table_bytes + (size_t)wib * kSmallStageBytes;
    double* rew_s = reinterpret_cast<double*>(small);
    uint8_t* af_s = small + 512;
    uint8_t* tp_s = small + 576;
    if (out.obs) {
        build_obs_table<0>(table, p);
        init_wave_consts(wl, p, lane);
    }

    // ---- the state after begin, the caller's arrays, the agent's cell word -----------------------------------------
    const int x = st.x[idx], y = st.y[idx];
    const uint32_t act = st.active[idx] != 0 ? 1u : 0u;
    const uint32_t term0 = st.terminated[idx] != 0 ? 1u : 0u, trunc0 = st.truncated[idx] != 0 ? 1u : 0u;
    const int stepc = st.step_count[env_ld];
    const int episode0 = st.episode[env_ld];
    const double ur = u_reward ? u_reward[idx] : 0.0;
    const int ut = u_term ? (int)u_term[idx] : 0;
    const uint32_t uu = u_trunc ? (uint32_t)u_trunc[idx] : 0u;
    const int Wp = p.W + 3;
    const uint32_t cells = (uint32_t)(Wp * (p.H + 3));
    const uint32_t cell = valid ? (uint32_t)cell_index(x, y, Wp) : 0u;
    const unsigned long long ci = cell_info[cell];
    const uint32_t ilo = (uint32_t)ci, ihi = (uint32_t)(ci >> 32);
    const bool boarding = i < p.Nb;
    const uint32_t tsh = cell_tsh(boarding), tsh2 = cell_tsh2(boarding);
    const uint64_t gm = split_group_mask(glog, lane);

    // ---- :214-227 the three strategies against the PRE-step flags ---------------------------------------------------
    const uint32_t live = (valid && (term0 | trunc0) == 0u) ? 1u : 0u;          // rewards.py:64, truncateds.py:56
    double r;
    if (u_reward) {
        r = ur;
    } else if (p.off_rtab) {                                                     // position-only user reward (ccx_set_reward_table)
        r = p.reward_table[(boarding ? 0u : cells) + cell];
    } else {
        r = cell_reward(ilo, ihi, tsh, tsh2, reward_class_a(p), p.r_door, p.r_area, p.r_f);
    }
    r = reward_if_live(r, live);
    uint32_t t1, present;
    if (u_term) {
        t1 = ut == 1 ? 1u : 0u;
        present = ut != -1 ? 1u : 0u;                                            // -1: the strategy returned None
    } else {
        const uint32_t tind = cell_terminated(ilo, tsh);                        // terminateds.py:66-82 / the user's table
        const uint64_t ndest_b = __builtin_amdgcn_ballot_w64(valid && tind == 0u) & gm;
        t1 = p.term_mode == CCX_K_TERM_ALL ? (ndest_b == 0ull ? 1u : 0u) : tind;
        present = 1u;
    }
    if (!valid) { t1 = 0u; present = 0u; }
    const uint32_t u1 = live & (u_trunc ? (uu != 0u ? 1u : 0u) : (stepc >= p.max_steps ? 1u : 0u));
    // ---- :256-259 __all__: all(values) over the entries that exist, False for an empty dict ----------------------------
    const uint64_t pres_b = __builtin_amdgcn_ballot_w64(present != 0u) & gm;
    const uint64_t tbad_b = __builtin_amdgcn_ballot_w64(present != 0u && t1 == 0u) & gm;
    const uint64_t live_b = __builtin_amdgcn_ballot_w64(live != 0u);
    const uint64_t ubad_b = __builtin_amdgcn_ballot_w64(live != 0u && u1 == 0u) & gm;
    const uint32_t ef = ((pres_b != 0ull && tbad_b == 0ull) ? CCX_K_EF_ALL_TERM : 0u) |
                        (((live_b & gm) != 0ull && ubad_b == 0ull) ? CCX_K_EF_ALL_TRUNC : 0u);
    const bool may_reset = valid_env && auto_reset != 0 && pool != nullptr && p.pool_size > 0;
    const uint32_t efw = env_flag_byte(ef, may_reset ? (uint32_t)CCX_K_EF_RESET : 0u);
    const bool do_reset = (efw & CCX_K_EF_RESET) != 0u;
    // ---- :229-254 flags applied once, the emission set, the flag byte ---------------------------------------------------
    const uint32_t out2 = t1 | (u1 << 1);
    const uint32_t af = agent_flag_byte(out2, term0 | (trunc0 << 1), ilo, tsh, act);   // (stored for lanes with an agent only)
    const float4 me = make_float4((float)x, (float)y, boarding ? 0.0f : 1.0f, (float)act);

    // ---- stage: the row writer's float4 per lane, the small outputs in OUTPUT order ---------------------------------
    wl->slot[lane] = valid ? me : make_float4(0.0f, 0.0f, boarding ? 0.0f : 1.0f, 0.0f);
    if (valid) {
        const int q = g * N + i;
        rew_s[q] = r;
        af_s[q] = (uint8_t)af;
        tp_s[q] = (uint8_t)present;
    }
    __syncthreads();

    int envs_here = p.E - env0;
    envs_here = envs_here < 0 ? 0 : (envs_here > p.EW ? p.EW : envs_here);
    const int count = envs_here * N;                                             // agent slots of this wave's envs (<= 64)
    const size_t base = (size_t)env0 * (size_t)N;
    if (count > 0) {
        if (out.reward && lane < count) out.reward[base + lane] = rew_s[lane];
        auto bytes_out = [&](uint8_t* dst, const uint8_t* src) {
            uint8_t* d = dst + base;
            if (((reinterpret_cast<uintptr_t>(d) | (uintptr_t)count) & 3u) == 0u) {   // wave-uniform: packed dwords
                if (lane < (count >> 2)) reinterpret_cast<uint32_t*>(d)[lane] = reinterpret_cast<const uint32_t*>(src)[lane];
            } else if (lane < count) {
                d[lane] = src[lane];
            }
        };
        if (out.agent_flags) bytes_out(out.agent_flags, af_s);
        if (term_present) bytes_out(term_present, tp_s);
        if (out.env_flags && valid_env && i == 0) out.env_flags[env] = (uint8_t)efw;
        if (out.obs_compact && valid) reinterpret_cast<v4f*>(out.obs_compact)[idx] = v4f{me.x, me.y, me.z, me.w};
        if (out.obs) {
            const int units = envs_here * N * (3 + 2 * N);
            emit_obs<PAIR>(wl, table, reinterpret_cast<char*>(out.obs + base * (size_t)L), 0, PAIR ? (units >> 1) : units, lane);
        }
    }

    // ---- state: the flags; an env that raised __all__ restarts from its pool entry (ccx.h: ccx_set_reset_pool) ----------
    if (valid) {
        if (do_reset) {
            const size_t pi = (size_t)pool_entry((unsigned long long)(p.env_offset + env), (unsigned long long)(uint32_t)(episode0 + 1),
                                                 (unsigned long long)p.pool_stride, (unsigned long long)p.pool_size);
            const uint8_t* src = pool + (pi * (size_t)N + (size_t)i) * 2u;
            st.x[idx] = src[0];
            st.y[idx] = src[1];
            st.active[idx] = 1;
            st.terminated[idx] = 0;
            st.truncated[idx] = 0;
        } else {
            st.terminated[idx] = (uint8_t)(term0 | t1);
            st.truncated[idx] = (uint8_t)(trunc0 | u1);
        }
    }
    if (do_reset && i == 0) {
        st.episode[env] = episode0 + 1;
        st.step_count[env] = 0;
    }
    if (counters && count > 0) {
        const uint64_t slot0_b = __builtin_amdgcn_ballot_w64(valid_env && i == 0);
        const uint64_t reset_b = __builtin_amdgcn_ballot_w64(do_reset && i == 0);
        unsigned long long v = 0;
        if (lane == 0) v = (unsigned long long)__builtin_popcountll(slot0_b);
        if (lane == 1) v = (unsigned long long)__builtin_popcountll(slot0_b) * (unsigned long long)N;
        if (lane == 2) v = (unsigned long long)__builtin_popcountll(live_b);
        if (lane == 3) v = (unsigned long long)__builtin_popcountll(reset_b);
        if (lane < 4 && v) atomicAdd(counters + kCounterTotals + (size_t)wave * kCounterSlot + lane, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
hipError_t launch_step_begin(hipStream_t stream, const KParams& p, const KState& st, int glog, const uint8_t* actions,
                             const uint8_t* order, unsigned long long* counters) {
    const int ew = 64 >> glog;
    const long long waves = ((long long)p.E + ew - 1) / ew;
    const long long blocks = (waves + 3) / 4;
    if (blocks < 1 || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(step_begin_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, st, actions, order, glog, counters);
    return hipGetLastError();
}

size_t step_finish_lds_bytes(const KParams& p) {
    const size_t table = ((((size_t)p.units_per_wave + 2u) * 2u) + 15u) & ~(size_t)15u;
    return (size_t)p.waves_per_block * (sizeof(WaveLds) + kSmallStageBytes) + table;
}

hipError_t launch_step_finish(const LaunchShape& ls, hipStream_t stream, const KParams& p, const KState& st,
                              const unsigned long long* cell_info, const double* reward, const int8_t* terminated,
                              const uint8_t* truncated, const KOut& out, uint8_t* term_present, int auto_reset,
                              const uint8_t* pool, unsigned long long* counters) {
    if (p.EW < 1 || p.waves_per_block < 1 || p.waves_per_block > 8) return hipErrorInvalidValue;
    const long long waves = ((long long)p.E + p.EW - 1) / p.EW;
    const long long blocks = (waves + p.waves_per_block - 1) / p.waves_per_block;
    const size_t lds = step_finish_lds_bytes(p);
    if (blocks < 1 || blocks > 0x7FFFFFFFll || lds > 64u * 1024u) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(64u * (unsigned)p.waves_per_block);
    if ((p.N % 2) == 0)
        hipLaunchKernelGGL((step_finish_kernel<true>), grid, block, lds, stream, p, st, cell_info, reward, terminated,
                           truncated, out, term_present, ls.glog, auto_reset, pool, counters);
    else
        hipLaunchKernelGGL((step_finish_kernel<false>), grid, block, lds, stream, p, st, cell_info, reward, terminated,
                           truncated, out, term_present, ls.glog, auto_reset, pool, counters);
    return hipGetLastError();
}

}  // namespace ccx
