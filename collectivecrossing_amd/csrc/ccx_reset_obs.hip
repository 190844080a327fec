// ccx_reset_obs.hip -- CCX_RESET_OBS, the stand-alone fix-up kernel (include/ccx.h): behind a launch (or a whole call) that
// wrote observation rows with auto-reset, every (step s, env e) whose env-flag byte carries CCX_EF_RESET gets the rows of the
// RESTARTED state at obs[s][e] / obs_compact[s][e]; the terminal rows the step wrote there move to final_obs[s][e] /
// final_compact[s][e] where a side buffer is bound.  Rows of pairs without CCX_EF_RESET are neither read nor written.
//
// One wave per env.  The wave walks env_flags[0..K)[e] in chunks of 64 steps (one flag byte per lane), counts the env's
// restarts, and derives the episode ordinal each restart OPENED from the handle's episode[e] AFTER the launch:
//     ordinal(s) = episode[e] - (restarts at steps > s)
// -- the state is the only place the episode counter lives, and the flags say how it got there.  The pool entry is the
// cursor of ccx_set_reset_pool, (global_env + ordinal * stride) mod P.  For every restart the wave stages the placement as a
// WSlot (float4 per agent + the row constants, as the observe kernel does) and copies the env's row region out of it with
// emit_obs -- the gather of ccx_observe / ccx_expand_observations: 16-byte stores, 8-byte ones for an odd agent count --
// through the handle's u16 address table (its first N (3 + 2N) units are those of an env at lane group 0, whatever the
// launch shape).  The terminal rows are read and written to the side buffer FIRST and the wave waits for those loads
// (their stores consume them) before the restarted rows go to the same addresses.
// The compact rows need no such wait: lane a loads compact[s][e][a], stores it to the side buffer and then overwrites the
// very 16 bytes it loaded -- one lane, one address, program order, and the first store consumes the load.  The rows differ:
// emit_obs stores through inline assembly the compiler cannot see into, so the wait that retires the copy loop's loads is
// written out.
// The flag bytes are read twice (count, then walk): ceil(K / 64) one-byte loads per lane and pass, E apart -- K E bytes per
// pass against K E N L 4 bytes of rows the launch wrote.  Its cost is not measured yet (profiles/reset_obs_timing.py).
// Offsets are 64-bit: K E N L exceeds 2^31 for long rollouts.
#include "ccx_rollout_dev.h"

namespace ccx {

constexpr int kResetObsWaves = 4;    // envs (waves) per workgroup

template <bool PAIR>
__global__ void __launch_bounds__(64 * kResetObsWaves)
reset_obs_kernel(const int E, const int N, const int Nb, const int K, const int dc, const int div, const int dl, const int dr,
                 const uint8_t* __restrict__ env_flags,          // u8 [K][E]
                 const int32_t* __restrict__ episode,            // i32 [E]: the state's counter AFTER the launch
                 const uint8_t* __restrict__ pool, const unsigned long long pool_size, const unsigned long long pool_stride,
                 const unsigned long long env_offset_mod_pool,
                 const uint16_t* __restrict__ obs_table,         // u16 LDS source address per float2 unit (ccx_kernels.h)
                 float* __restrict__ obs, float* __restrict__ obs_compact,             // [K][E][N][L], [K][E][N][4] or null
                 float* __restrict__ final_obs, float* __restrict__ final_compact) {   // same shapes, or null
    __shared__ __align__(16) WaveLds lds[kResetObsWaves];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int env = (int)blockIdx.x * kResetObsWaves + wib;
    if (env >= E) return;                                        // (wave-uniform; no workgroup barrier below)
    WaveLds* const wl = &lds[wib];
    struct { int dc, div, dl, dr; } cst{dc, div, dl, dr};
    init_wave_consts(wl, cst, lane);
    // restarts of this env in the whole launch
    uint32_t total = 0;
    for (int s0 = 0; s0 < K; s0 += 64) {
        const int s = s0 + lane;
        const uint32_t f = s < K ? (uint32_t)env_flags[(size_t)s * (size_t)E + (size_t)env] : 0u;
        total += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((f & CCX_K_EF_RESET) != 0u));
    }
    if (total == 0u) return;
    const uint32_t ep_after = (uint32_t)episode[env];
    const int L = 6 + 4 * N;
    const size_t row_floats = (size_t)N * (size_t)L;             // one env-step's rows
    const int units = N * (3 + 2 * N) >> (PAIR ? 1 : 0);         // vector units of them
    uint32_t seen = 0;                                           // restarts at earlier steps
    for (int s0 = 0; s0 < K; s0 += 64) {
        const int sl = s0 + lane;
        const uint32_t f = sl < K ? (uint32_t)env_flags[(size_t)sl * (size_t)E + (size_t)env] : 0u;
        uint64_t b = __builtin_amdgcn_ballot_w64((f & CCX_K_EF_RESET) != 0u);
        while (b != 0) {
            const int s = s0 + __builtin_ctzll(b);
            b &= b - 1;
            seen += 1u;
            const uint32_t ordinal = ep_after - (total - seen);  // the episode this restart opened
            const unsigned long long pi = pool_entry(env_offset_mod_pool + (unsigned long long)env, ordinal, pool_stride, pool_size);
            const size_t se = (size_t)s * (size_t)E + (size_t)env;
            float4 me = make_float4(0.0f, 0.0f, lane < Nb ? 0.0f : 1.0f, 1.0f);
            if (lane < N) {
                const uint8_t* src = pool + ((size_t)pi * (size_t)N + (size_t)lane) * 2u;
                me.x = (float)src[0];
                me.y = (float)src[1];
            }
            if (obs_compact != nullptr && lane < N) {
                float4* const c = reinterpret_cast<float4*>(obs_compact) + se * (size_t)N + (size_t)lane;
                if (final_compact != nullptr) reinterpret_cast<float4*>(final_compact)[se * (size_t)N + (size_t)lane] = *c;
                *c = me;
            }
            if (obs != nullptr) {
                wl->slot[lane] = me;
                char* const dst = reinterpret_cast<char*>(obs + se * row_floats);
                if (final_obs != nullptr) {
                    char* const fin = reinterpret_cast<char*>(final_obs + se * row_floats);
                    for (int q = lane; q < units; q += 64) {
                        if constexpr (PAIR) *reinterpret_cast<float4*>(fin + (size_t)q * 16) = *reinterpret_cast<const float4*>(dst + (size_t)q * 16);
                        else *reinterpret_cast<float2*>(fin + (size_t)q * 8) = *reinterpret_cast<const float2*>(dst + (size_t)q * 8);
                    }
                }
                // the terminal rows have been read (and the slot written) before the restarted rows overwrite them
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                emit_obs<PAIR>(wl, obs_table, dst, 0, units, lane);
                wave_lds_sync();                                 // the slot is rewritten by the env's next restart
            }
        }
    }
}

hipError_t launch_reset_obs(hipStream_t stream, const KParams& p, const KState& st, int K, const uint8_t* env_flags,
                            const uint8_t* pool, float* obs, float* obs_compact, float* final_obs, float* final_compact) {
    if (K < 1 || !env_flags || !pool || p.pool_size <= 0 || (!obs && !obs_compact)) return hipErrorInvalidValue;
    const unsigned long long P = (unsigned long long)p.pool_size;
    const dim3 grid((unsigned)((p.E + kResetObsWaves - 1) / kResetObsWaves)), block(64 * kResetObsWaves);
    const unsigned long long stride = (unsigned long long)p.pool_stride, off = (unsigned long long)(p.env_offset % p.pool_size);
    if ((p.N % 2) == 0)
        hipLaunchKernelGGL(reset_obs_kernel<true>, grid, block, 0, stream, p.E, p.N, p.Nb, K, p.dc, p.div, p.dl, p.dr, env_flags,
                           (const int32_t*)st.episode, pool, P, stride, off, p.obs_table, obs, obs_compact, final_obs, final_compact);
    else
        hipLaunchKernelGGL(reset_obs_kernel<false>, grid, block, 0, stream, p.E, p.N, p.Nb, K, p.dc, p.div, p.dl, p.dr, env_flags,
                           (const int32_t*)st.episode, pool, P, stride, off, p.obs_table, obs, obs_compact, final_obs, final_compact);
    return hipGetLastError();
}

}  // namespace ccx
