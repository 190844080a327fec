// ccx_rollout_body.inc -- the body of ccx::rollout_kernel / rollout_kernel_v128 (ccx_kernels.hip includes it twice:
// the two entry points differ in a register-budget attribute only, and routing the body through a device function
// changed the code of the hot instantiation -- C2 0.863 vs 0.897 of the HBM peak in one call).  In scope: the template
// parameters GLOG, PAIR, OUTM, OCC, PLAIN and the kernel arguments p, st, cell_info, actions, order, K, auto_reset,
// pool, out, counters, policy_arg, actions_out.
    constexpr bool OUT = OUTM != 0, EDGE = OUTM >= 2, VARLEAD = OUTM == 3;
    // (see ccx_kernels.hip: every kernel argument is read from the kernel-argument segment where it is used; the by-value
    // parameters of the signature only define that segment's layout)
    rollout_kernarg_prefetch();
    KParamsC& p = rollout_kernarg_params();
    KernargTailC& KA = rollout_kernarg_tail();
    const int K = KA.K;   // (shadows nothing: the signature names it K_by_value)
    const int policy = PLAIN ? 0 : KA.policy;
    using mask_t = typename GroupMask<GLOG>::type;
    constexpr int G = 1 << GLOG;
    extern __shared__ __align__(16) unsigned char smem[];

    CCX_T(0);
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform -> SGPR
    const int tpb = p.waves_per_block;                                  // tiles per block
    const int role = OUT ? wib / tpb : 0;                               // 0 sim, 1.. writers
    const int tile_in_block = OUT ? wib - role * tpb : wib;
    // XCD-aware tile mapping: workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each
    // with its own L2 and path to memory.  Workgroups of one XCD take ADJACENT tiles, so an XCD
    // writes one contiguous eighth of every step's output slab instead of every eighth chunk --
    // the pace at which the output stream collapses moves from ~740 to ~700 ns per env-step on C2
    // (profiles/scratch/tile_times.py, DESIGN.md 3.6).
    // tile_map: 0 = XCD-contiguous (above); v >= 1 = groups of 2^(v-1) adjacent tiles per XCD, dealt
    // round-robin (1 = the plain blockIdx -> tile mapping): with the tiles phased in tile order
    // (pace_phase 1) the chip writes ONE window that sweeps through the slab, fed by all eight XCDs,
    // while the small partial-line outputs of a group still meet in one L2.
    int bid = blockIdx.x;
    if (p.tile_map == 0u) {
        const int nb = gridDim.x, xcd = blockIdx.x & 7, q8 = nb >> 3, r8 = nb & 7;
        bid = xcd * q8 + (xcd < r8 ? xcd : r8) + (int)(blockIdx.x >> 3);
    } else if (p.tile_map > 1u) {
        const uint32_t m = p.tile_map - 1u, span = 8u << m, b = blockIdx.x;
        if (b < (gridDim.x / span) * span)       // (a tail that does not fill a span keeps the plain mapping)
            bid = (int)((b & ~(span - 1u)) + ((b & 7u) << m) + ((b >> 3) & ((1u << m) - 1u)));
    }
    const int tile = (bid + (int)p.block_base) * tpb + tile_in_block;
    const int g = lane >> GLOG;
    const int i = lane & (G - 1);
    const int gbase = g << GLOG;
    const int env0 = tile * p.EW;                 // first env of this tile
    const int env = env0 + g;
    const bool valid_env = (g < p.EW) && (env < p.E);
    const bool valid = valid_env && (i < p.N);
    const uint32_t validbit = in_vgpr(valid ? 1u : 0u);   // (an opaque 0/1: keeps the compiler from folding it into lane-mask logic on the SALU)
    const int N = p.N;
    const int L = 6 + 4 * N;
    const size_t EN = (size_t)p.E * N;
    const size_t idx = (size_t)env * N + i;
    const bool boarding = i < p.Nb;
    const uint32_t tsh = cell_tsh(boarding);      // type-specific nibble of the cell word (ccx_step_rule.h)
    const uint32_t tsh2 = cell_tsh2(boarding);    // type-specific half of the distance word
    const int Wp = p.W + 3;

    // LDS carve-up: [cell table][tile 0 .. tile tpb-1][u16 obs table]; offsets from the host
    const uint32_t cells = (uint32_t)(Wp * (p.H + 3));
    unsigned long long* cinfo = reinterpret_cast<unsigned long long*>(smem);
    unsigned char* tbase = smem + p.off_tiles + (uint32_t)tile_in_block * p.tile_stride;
    uint32_t* xch = reinterpret_cast<uint32_t*>(tbase);
    uint32_t* stage = reinterpret_cast<uint32_t*>(tbase + kStageOff);
    const uint32_t stage_mask = p.stage_slots - 1u;
    uint16_t* table = reinterpret_cast<uint16_t*>(smem + p.off_table);
    const bool want_obs = OUT && KA.out.obs != nullptr;
    // Prologue: both host-built tables come from global memory (L2-resident after the first
    // workgroup).  The first chunk of each is requested before anything else so that ONE memory
    // latency covers both and the LDS zeroing below; small grids (C2: 143 cells, 609 table words)
    // need nothing more.
    const uint32_t tw = want_obs ? (((uint32_t)p.units_per_wave + 2u) >> 1) : 0u;   // u16 pairs of the obs table
    const uint32_t* tsrc = reinterpret_cast<const uint32_t*>(p.obs_table);
    const unsigned long long c_first = threadIdx.x < cells ? KA.cell_info[threadIdx.x] : 0ull;
    uint32_t t_first[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t w = threadIdx.x + (uint32_t)r * blockDim.x;
        t_first[r] = w < tw ? tsrc[w] : 0u;
    }
    // The sim waves request their state and the first burst of actions HERE, behind the tables' first chunks and in front
    // of the barrier: the tables, the state and the actions then share ONE memory round trip.  Requested after the barrier
    // (as rounds 1-2 did) a single-step launch is a chain of three dependent round trips of 1.2-1.6 us each
    // (profiles/scratch/tstamps.py: tables 1.64 us, state 1.2 us, step 0.7 us, write-back 1.3 us).
    // Plain straight-line loads from a clamped index, by every wave (a writer wave's copies hit the lines its sim wave
    // asks for): inside an `if (valid)` block the compiler folds the first uses -- and with them the waits -- into the
    // block, in front of the loads that follow.
    const size_t idx_ld = valid ? idx : (size_t)0;
    const int env_ld = valid_env ? env : 0;
    const int s_x = KA.st.x[idx_ld], s_y = KA.st.y[idx_ld];
    const uint32_t s_active = KA.st.active[idx_ld], s_term = KA.st.terminated[idx_ld], s_trunc = KA.st.truncated[idx_ld];
    const int s_stepc = KA.st.step_count[env_ld], s_episode = KA.st.episode[env_ld];
    // ---- actions: bursts of kActBatch steps, 4 bits per step ----------------------------------
    // One s_waitcnt vmcnt per burst instead of one per step.  Every load of a burst is UNCONDITIONAL and the burst is
    // ONE straight line: lanes without an agent read slot 0's byte (never used: such lanes count as terminated), steps
    // past the end of the launch re-read its last step (never unpacked) -- the per-lane byte offset is clamped to the
    // last step's (a launch stays below 4 GiB per stream, run_rollout).  A predicated load cost ~14 instructions on the
    // sim wave's one-instruction-per-4.4-clocks budget, 14 of a step's ~160, against 3 now (add, min, load); and a
    // second code path for the last, partial burst made the compiler merge the two paths' registers behind a
    // `s_waitcnt vmcnt(0)` -- a full memory round trip at the start of EVERY burst.
    // (the move-order / policy instantiations are short of SGPRs, not of VGPRs: base and stride live in VGPRs there)
    const uint8_t* const act_base = PLAIN ? KA.actions : (const uint8_t*)(uintptr_t)in_vgpr((unsigned long long)(uintptr_t)KA.actions);
    const uint32_t EN32a = PLAIN ? (uint32_t)EN : in_vgpr((uint32_t)EN);
    uint32_t act_off = (uint32_t)idx_ld;
    const uint32_t act_lim = (uint32_t)idx_ld + (uint32_t)(K - 1) * EN32a;
    uint32_t araw[kActBatch];
    auto fetch_actions = [&](int) {
#pragma unroll
        for (int d = 0; d < kActBatch; ++d) {
            araw[d] = (uint32_t)act_base[act_off];
            const uint32_t nx = act_off + EN32a;
            act_off = nx < act_lim ? nx : act_lim;
        }
    };
    if (!policy) fetch_actions(0);
    if constexpr (OCC) {   // zero the occupancy / proposal tables of every tile of the block
        for (int ti = 0; ti < tpb; ++ti) {
            uint32_t* occ = reinterpret_cast<uint32_t*>(smem + p.off_tiles + (uint32_t)ti * p.tile_stride + p.off_occ);
            for (uint32_t w = threadIdx.x; w < p.occ_words; w += blockDim.x) occ[w] = 0u;
        }
    }
    if (OUT && threadIdx.x < (uint32_t)tpb * 16u) {
        // hand-off words of every tile of the block: sequence = 0, progress of the writers = 0, of unused slots = "far ahead"
        const uint32_t ti = threadIdx.x >> 4, k = threadIdx.x & 15u;
        uint32_t* sw = reinterpret_cast<uint32_t*>(smem + p.off_tiles + ti * p.tile_stride + kSyncOff);
        sw[k] = (k >= kSyncProg + (uint32_t)p.writers && k < kSyncProg + 8u) ? 0x7FFFFFFFu : 0u;
    }
    if (threadIdx.x < cells) cinfo[threadIdx.x] = c_first;
    for (uint32_t t = threadIdx.x + blockDim.x; t < cells; t += blockDim.x) cinfo[t] = KA.cell_info[t];
    {
        uint32_t* tdst = reinterpret_cast<uint32_t*>(table);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint32_t w = threadIdx.x + (uint32_t)r * blockDim.x;
            if (w < tw) tdst[w] = t_first[r];
        }
        for (uint32_t w = threadIdx.x + 3u * blockDim.x; w < tw; w += blockDim.x) tdst[w] = tsrc[w];
    }
    // terminated | truncated << 1 as the state arrays held them at kernel entry; lanes without an agent count as done.
    // Consumed HERE, in front of the barrier, by every wave: the sim wave writes the arrays back in its epilogue, which it
    // can only reach after this barrier -- a writer wave that read them behind the barrier (rounds 1-2) raced with that
    // write-back in launches of a step or two (seen once the prologue got faster: wrong LIVE bits, at random).
    const uint32_t tt_entry = in_vgpr(valid ? ((s_term != 0u ? 1u : 0u) | (s_trunc != 0u ? 2u : 0u)) : 1u);
    CCX_T(1);
    __syncthreads();  // tables are read-only / zeroed from here on
    CCX_T(2);

    int envs_here = p.E - env0;
    envs_here = envs_here < 0 ? 0 : (envs_here > p.EW ? p.EW : envs_here);
    const int units = envs_here * N * (3 + 2 * N);
    const int n4 = PAIR ? (units >> 1) : units;     // vector units (16 B or 8 B) of the obs region

    // =========================================================================================
    // WRITER waves: reward, flag bytes, observation rows of every step (reference :214-261).
    // Writer w of nw takes the store iterations it = w, w + nw, ...; writer 0 also writes the
    // reward and the flag bytes.
    // =========================================================================================
    if constexpr (OUT) {
        if (role > 0) {
            const int w = role - 1, nw = p.writers;
            // (shapes that batch two steps per row-writer iteration give every writer TWO staging slots: ws_per_writer)
            const uint32_t wsw = p.ws_per_writer;
            WSlot* wl = reinterpret_cast<WSlot*>(tbase + p.off_ws) + (uint32_t)w * wsw;
            init_wave_consts(wl, p, lane);
            if (wsw > 1u) init_wave_consts(wl + 1, p, lane);
            const float type_f = boarding ? 0.0f : 1.0f;  // observations.py:85
            // reward constants (rewards.py:44-182): class 1/2/3 -> rA/rB/rC, class 0 -> sd * rF
            const double rA = in_vgpr(reward_class_a(p));
            const double rB = in_vgpr(p.r_door);
            const double rC = in_vgpr(p.r_area);
            const double rF = in_vgpr(p.r_f);
            // User reward table (ccx_set_reward_table; position-only RewardFunction plugins): the entry of (my type, the cell my
            // hand-off word points at) lies this far behind the cell word; 0 = no table.  Handles with user tables launch the
            // instantiations that are not PLAIN: the plain ones -- the bench line, ordinary RL stepping -- carry none of this
            // (a first version inside them cost the rollouts without observation rows 12-17 %: every instruction on the reward
            // writer's chain counts there, and so did the code size of further loop copies; profiles/scratch/calls/r04_call1[0-2].sh)
            const uint32_t rt_add = PLAIN ? 0u : (p.off_rtab ? p.off_rtab + (boarding ? 0u : cells * 8u) : 0u);
            // wave-uniform base pointers advanced per step on the scalar unit + per-lane 32-bit
            // byte offsets that never change
            // Without observation rows the row writers have nothing to do while writer 0's chain (hand-off word -> cell
            // word -> flag byte, reward, compact row: ~125 instructions and four stores per step) is what such rollouts
            // wait for (0.34 us per env-step next to the sim wave's 0.27): writer 1 then takes the rewards (its own copy
            // of the terminated / truncated pair, the cell word, the f64 multiply, one store) off writer 0.
            const bool split_small = !want_obs && nw > 1;                       // wave-uniform
            const bool small_out = (w == 0) || (split_small && w == 1);
            // Small outputs: a constant base (re-read from the kernel-argument segment where it is used) + a 32-bit byte
            // offset per lane that advances by the stream's stride every step -- no 64-bit pointer per stream on the
            // scalar unit.  The host cuts a rollout into launches that stay below 4 GiB per output stream (run_rollout).
            uint32_t rew_off = (uint32_t)idx * 8u, af_off = (uint32_t)idx, ef_off = (uint32_t)env, cmp_off = (uint32_t)idx * 16u;
            const uint32_t EN32 = (uint32_t)EN;
            // which small outputs this wave writes: wave-uniform flags
            const bool has_rew = (split_small ? w == 1 : w == 0) && KA.out.reward != nullptr;
            const bool has_af = w == 0 && KA.out.agent_flags != nullptr;
            const bool has_ef = w == 0 && KA.out.env_flags != nullptr, has_act = w == 0 && KA.actions_out != nullptr;
            if constexpr (!PLAIN) {
                if (has_rew && p.off_rtab) {
                    // the table itself: f64 [2][cells] behind the cell table, staged by the wave that reads it (tiles of one
                    // workgroup write the same values to the same words)
                    double* rt = reinterpret_cast<double*>(smem + p.off_rtab);
                    for (uint32_t t = (uint32_t)lane; t < 2u * cells; t += 64u) rt[t] = p.reward_table[t];
                    wave_lds_sync();
                }
            }
            // compact observation: the (x, y, type, active) of this lane's agent, 16 bytes per agent-step
            // instead of the 16N + 24 of the DefaultObservation rows that repeat it N times
            const bool has_cmp = w == 0 && KA.out.obs_compact != nullptr;
            typedef __attribute__((address_space(1))) char gchar;
            char* obs_s = reinterpret_cast<char*>(KA.out.obs) + (size_t)env0 * N * L * 4;
            const size_t obs_stride = EN * (size_t)L * 4;
            // Store iterations are laid out on 128-byte lines of GLOBAL memory, not from the start of
            // the tile's region: a region that starts mid-line (most agent counts; N = 50: 41200 B
            // per env) would otherwise make every 1-KiB wave store straddle two partially written
            // lines (measured 4.1 vs 6.1 TB/s).  `lead` = vector units between the line boundary
            // below the region and its start; constant over the steps when the slab stride is a
            // multiple of 128 bytes (else 0: the old, region-relative layout).
            const uint32_t vbytes = PAIR ? 16u : 8u;
            const uint32_t lead = __builtin_amdgcn_readfirstlane(
                ((obs_stride & 127u) == 0 && want_obs)
                    ? (uint32_t)(reinterpret_cast<uintptr_t>(obs_s) & 127u) / vbytes : 0u);
            obs_s -= lead * vbytes;                       // line-aligned base; unit q lives at (q + lead)
            const int n4l = n4 + (int)lead;               // one past the last slot of the shifted layout
            // my store iterations: it0, it0 + it_step, ... below it_end (one iteration = 64 vector units)
            const int total_its = (n4l + 63) >> 6;
            // each writer takes one contiguous share of the region (+0.5 % on C3 / C5 under pacing; interleaving
            // the writers' 1-KiB iterations instead was +1 % on C3 with 3 writers, -1..2 % on C5-50, and the
            // run-time stride cost the single-writer C2 path 3-5 %: not kept)
            // Small batches (p.writer0_small): writer 0 keeps to the small outputs (reward, flag bytes, compact
            // rows, chosen actions) and the other writers share the observation rows -- with both on one wave
            // that wave takes as long as the sim wave and the tile waits on it (stamps, 2048 envs: writer 0
            // 1180 clocks of work per step next to the sim's 1200).
            const int first_obs_writer = (p.writer0_small && nw > 1) ? 1 : 0;
            const int nwo = nw - first_obs_writer, wo = w - first_obs_writer;
            const bool my_obs = want_obs && wo >= 0;
            const int per_w = (total_its + nwo - 1) / nwo;
            const int it0 = wo >= 0 ? wo * per_w : total_its;
            constexpr int it_step = 1;
            const int it_end = (it0 + per_w) < total_its ? (it0 + per_w) : total_its;
            // Edge iterations.  A region that does not begin / end on a 128-byte line (N = 50: rows of 824 bytes)
            // shares its first and last line with the neighbouring tiles' regions: two partial writes of one
            // line from two workgroups.  Streamed (`nt`) they reach memory as two partial-line writes; written
            // with plain stores the first and the last iteration of a region stay in L2, where the halves
            // merge (the grouped tile map keeps neighbours on one XCD) -- C5-50 0.83 -> 0.86 of the HBM peak,
            // aligned shapes (C2, C3, C5-64) have no edge iteration and take the unchanged path.
            const int edge_first = (EDGE && lead != 0u && it0 == 0) ? 0 : -1;
            const int edge_last = (EDGE && (((uint32_t)n4l * vbytes) & 127u) != 0u && it_end == total_its) ? total_its - 1 : -1;
            uint32_t edge_mask = 0;   // over my register-cached iterations
            if (EDGE && my_obs) {
                if (edge_first >= 0) edge_mask |= 1u;
                if (edge_last >= it0 && edge_last - it0 < kFastObsIters) edge_mask |= 1u << (edge_last - it0);
            }
            edge_mask = __builtin_amdgcn_readfirstlane(edge_mask);
            // LDS source addresses (absolute, 32-bit) of this lane's first kFastObsIters observation stores
            const uint32_t wl_abs = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem + p.off_tiles +
                                    (uint32_t)tile_in_block * p.tile_stride + p.off_ws + (uint32_t)w * wsw * (uint32_t)sizeof(WSlot);
            uint32_t oa0[kFastObsIters], oa1[kFastObsIters];
#pragma unroll
            for (int j = 0; j < kFastObsIters; ++j) {
                const uint32_t q = (uint32_t)(lane + 64 * (it0 + it_step * j)) - lead;   // wraps below the region
                oa0[j] = oa1[j] = wl_abs + kCstOff + 16u;
                if (my_obs && (it0 + it_step * j) < it_end && q < (uint32_t)n4) {
                    if constexpr (PAIR) {
                        const uint32_t t = reinterpret_cast<const uint32_t*>(table)[q];
                        oa0[j] = wl_abs + (t & 0xFFFFu);
                        oa1[j] = wl_abs + (t >> 16);
                    } else {
                        oa0[j] = wl_abs + table[q];
                    }
                }
            }
            // Which of my register-cached iterations this lane takes part in: iteration 0 may lose the lanes below `lead`,
            // from iteration 1 on the valid ones are a prefix.  Kept as two per-lane numbers and compared inside the step loop
            // (one v_cmp per store) -- as loop-invariant lane masks they were ten SGPR pairs that did not fit and were
            // re-read through v_readlane for every store.
            uint32_t v_ok0 = 0, v_jmax = 1;
#pragma unroll
            for (int j = 0; j < kFastObsIters; ++j) {
                const uint32_t q = (uint32_t)(lane + 64 * (it0 + it_step * j)) - lead;
                const bool vj = my_obs && !VARLEAD && (it0 + it_step * j) < it_end && q < (uint32_t)n4;
                if (j == 0) v_ok0 = vj ? 1u : 0u;
                else v_jmax += vj ? 1u : 0u;
            }
            const uint32_t q0_off = (uint32_t)(lane + 64 * it0) * vbytes;       // byte offset of my first iteration
            const uint32_t q0_off_4k = q0_off + 4096u, q0_off_8k = q0_off + 8192u;   // (store immediates reach 4095 bytes)
            const char* sbase = reinterpret_cast<const char*>(wl);
            const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
            const uint32_t sync_abs = lds0 + p.off_tiles + (uint32_t)tile_in_block * p.tile_stride + kSyncOff;
            typedef __attribute__((address_space(3))) uint32_t lds_u32;
            const bool flags_mode = p.hand_flags != 0u;       // wave-uniform
            uint32_t seen = 0;                                // steps the sim wave has staged, as far as this wave knows
#ifdef CCX_DIAG_WAITS   // diagnostic build (profiles/scratch/waits.py): who waits for whom?
            uint32_t diag_polls = 0, diag_waited_steps = 0, diag_pairs = 0;
#endif
            // writer 0 assembles the per-agent flag byte and keeps the pair (terminated, truncated << 1) the reference
            // keeps in Agent.terminated / .truncated (types.py:63-73); the sim wave only reports what a step raises
            uint32_t tt_w = tt_entry;                         // (the pair at kernel entry, read in front of the barrier)
            CCX_STAMP_DECL;

            // A writer's step is a chain of LDS round trips (hand-off word -> cell word -> its own staging slot -> the gather);
            // two of them are taken off that chain.  (1) While the sim wave is known to be ahead (the cached sequence number
            // says so: the case in which THIS wave is what the tile waits for) the next step's word is requested during
            // the current step.  (2) A wave that only writes observation rows needs (x, y) of the cell, nothing else of its
            // word: x and y come from the cell's address by one multiply-high (KParams::wp_magic) instead of a table read.
            uint32_t hw_nx = 0;
            bool have_nx = false;                             // wave-uniform
            // (kernel arguments used inside the loop are read HERE: a scalar load in the loop body shares the LDS wait
            // counter and would serialise the wave on every step)
            const uint32_t wp_magic = p.wp_magic, E32 = (uint32_t)p.E, wvm = p.writer_vmcnt;
            const uint32_t Wp_w = PLAIN ? (uint32_t)Wp : in_vgpr((uint32_t)Wp);   // (!PLAIN: short of SGPRs -- a VGPR operand, not a spill reload per step)
            // Where the small outputs go.  Plain instantiations (VGPRs to spare): one 64-bit address per lane and stream,
            // advanced on the vector unit -- no scalar state at all.  Policy / move-order instantiations (at their 128 VGPRs):
            // the stream's base in SGPRs + the 32-bit lane offset.
            gchar* const b_rew = PLAIN ? nullptr : (gchar*)KA.out.reward;
            gchar* const b_af = PLAIN ? nullptr : (gchar*)KA.out.agent_flags;
            gchar* const b_ef = PLAIN ? nullptr : (gchar*)KA.out.env_flags;
            gchar* const b_act = PLAIN ? nullptr : (gchar*)KA.actions_out;
            gchar* const b_cmp = PLAIN ? nullptr : (gchar*)KA.out.obs_compact;
            uintptr_t a_rew = 0, a_af = 0, a_ef = 0, a_cmp = 0;      // (actions_out only exists in policy rollouts: never PLAIN)
            if constexpr (PLAIN) {
                a_rew = in_vgpr(reinterpret_cast<uintptr_t>(KA.out.reward) + rew_off);
                a_af = in_vgpr(reinterpret_cast<uintptr_t>(KA.out.agent_flags) + af_off);
                a_ef = in_vgpr(reinterpret_cast<uintptr_t>(KA.out.env_flags) + ef_off);
                a_cmp = in_vgpr(reinterpret_cast<uintptr_t>(KA.out.obs_compact) + cmp_off);
            }
            // The loop exists five times (a generic lambda instantiated with compile-time roles): for the two roles of a
            // role-split tile -- writer 0 (small outputs only) and the row writers (observation rows only) -- and once with
            // the roles decided at run time (single writers, writers that share everything).  With the roles tested inside the loop a step of a writer carried ~15 wave-uniform
            // branches (15-20 clocks each).
            // two steps per row-writer iteration: shapes with a second staging slot, every iteration register-cached
            const bool pair_ok = wsw > 1u && (it_end - it0) <= kFastObsIters;     // wave-uniform
            auto writer_loop = [&](auto small_c, auto rows_c, auto flags_c, auto pairs_c) {
                constexpr int SMALL_C = decltype(small_c)::value, ROWS_C = decltype(rows_c)::value, FLAGS_C = decltype(flags_c)::value;
                constexpr bool PAIRS_C = decltype(pairs_c)::value != 0 && ROWS_C == 1 && SMALL_C == 0;   // (its own copy: the one-step loop stays as it was)
                const bool small_l = SMALL_C == 2 ? small_out : SMALL_C == 1;   // (2 = decided at run time)
                const bool rows_l = ROWS_C == 2 ? my_obs : ROWS_C == 1;
                const bool flags_l = FLAGS_C == 2 ? flags_mode : FLAGS_C == 1;
                for (int s = 0; s < K; ++s) {
                    // the sim wave has staged step s: in flags mode its sequence word says so (looked at only when this
                    // wave has caught up), else both sides meet at a barrier once per step
                    uint32_t hw;                                  // hand-off word (ccx_kernels.h: kHw*)
                    if (have_nx) {
                        hw = hw_nx;
                    } else {
                        if (flags_l) {
    #ifdef CCX_DIAG_WAITS
                            if (seen <= (uint32_t)s) ++diag_waited_steps;
    #endif
                            while (seen <= (uint32_t)s) {
                                seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(
                                    (lds_u32*)(uintptr_t)(sync_abs + 4u * kSyncSeq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                                if (seen > (uint32_t)s) break;
    #ifdef CCX_DIAG_WAITS
                                ++diag_polls;
    #endif
                                __builtin_amdgcn_s_sleep(1);
                            }
                            wave_lds_sync();
                        } else {
                            lds_barrier();
                        }
                        hw = stage[((uint32_t)s & stage_mask) * 64 + lane];
                    }
                    have_nx = flags_l && s + 1 < K && seen > (uint32_t)(s + 1);
                    if (have_nx) hw_nx = stage[((uint32_t)(s + 1) & stage_mask) * 64 + lane];
                    // Row writers of shapes with two staging slots take TWO steps per iteration whenever the sim wave is
                    // that far ahead: a row writer's step is a fixed chain (hand-off word -> slot -> gather -> stores,
                    // ~95 instructions, ~0.3 us) whatever its share of the rows, and it is what small batches wait for.
                    uint32_t hw_b = 0;
                    bool pair = false;
                    if constexpr (PAIRS_C) {
                        pair = have_nx;                                 // wave-uniform
                        if (pair) {
                            hw_b = hw_nx;
                            have_nx = s + 2 < K && seen > (uint32_t)(s + 2);
                            if (have_nx) hw_nx = stage[((uint32_t)(s + 2) & stage_mask) * 64 + lane];
                        }
                    }
                    // progress word (LDS executes a wave's instructions in order: the slots have been read when this lands);
                    // the sim wave looks at it before it reuses a slot of the ring
                    wave_lds_sync();
                    __hip_atomic_store((lds_u32*)(uintptr_t)(sync_abs + 4u * (kSyncProg + (uint32_t)w)),
                                       (uint32_t)s + (pair ? 1u : 0u) + (have_nx ? 2u : 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    // the agent's cell: writer 0 reads its word from the shared geometry table (reward class, distance term,
                    // info bits; this wave has the time for the read), the row writers only need x and y
                    uint32_t ilo, ihi = 0;
                    if (small_l) {
                        const unsigned long long cw =
                            *(__attribute__((address_space(3))) const unsigned long long*)(uintptr_t)(hw & kHwCellMask);
                        ilo = (uint32_t)cw;
                        ihi = (uint32_t)(cw >> 32);
                    } else {
                        const uint32_t cidx = ((hw & kHwCellMask) - lds0) >> 3;         // cell index in the padded grid
                        const uint32_t y1 = __umulhi(cidx, wp_magic), x1 = cidx - y1 * Wp_w;
                        ilo = cell_xy_bytes(x1 - 1u, y1 - 1u);                           // (bytes 2 and 3, as in the table)
                    }
                    CCX_STAMP(0);                        // wait for the sim wave
                    const uint32_t efw = (hw >> kHwEfShift) & 7u, act_w = (hw >> kHwActShift) & 1u;
                    // The flag byte (ccx_step_rule.h: agent_flag_byte).  From the sim wave: the flags this step raises
                    // (terminated, truncated), active, the action.  Here: this wave's copy of the pair BEFORE the step, the cell word.
                    const uint32_t out2 = (hw >> kHwOut2Shift) & 3u;
                    const uint32_t af = agent_flag_byte(out2, tt_w, ilo, tsh, act_w);
                    tt_w = (efw & CCX_K_EF_RESET) ? 0u : (tt_w | out2);
                    if (rows_l || has_cmp) {
                        // (x, y) are bytes 2 and 3 of the cell word: v_cvt_f32_ubyte2 / ubyte3
                        const float4 me = make_float4((float)cell_x(ilo), (float)cell_y(ilo), type_f,
                                                      (float)((af >> 6) & 1u));
                        if (rows_l) wl->slot[lane] = me;
                        if constexpr (PAIRS_C) {
                            if (pair) {   // the second step's float4 goes to the writer's second staging slot
                                const uint32_t cidx_b = ((hw_b & kHwCellMask) - lds0) >> 3;
                                const uint32_t yb = __umulhi(cidx_b, wp_magic), xb = cidx_b - yb * Wp_w;
                                wl[1].slot[lane] = make_float4((float)(xb - 1u), (float)(yb - 1u), type_f,
                                                               (float)((hw_b >> kHwActShift) & 1u));
                            }
                        }
                        if (has_cmp) {
                            if (valid) *(__attribute__((address_space(1))) v4f*)(PLAIN ? (gchar*)a_cmp : b_cmp + cmp_off) = v4f{me.x, me.y, me.z, me.w};
                            if constexpr (PLAIN) a_cmp += EN32 * 16u;
                            else cmp_off += EN32 * 16u;
                        }
                    }
                    if (small_l) {
                        // rewards.py:44-182.  Distances are integers and the reference negates the
                        // INTEGER before the one f64 multiply, so d == 0 gives +0.0 (never -0.0).
                        if (has_rew) {
                            // (= cell_reward, inline: the call took <3,1,2,1,1> from 7 to 8 SGPR spills, <3,0,2,0,1> from 7 to 9)
                            const uint32_t cls = cell_class(ilo, tsh);
                            const int sd = cell_distance(ihi, tsh2);
                            double r = (double)sd * rF;
                            r = (cls == 1u) ? rA : r;
                            r = (cls == 2u) ? rB : r;
                            r = (cls == 3u) ? rC : r;
                            if constexpr (!PLAIN) {
                                if (rt_add)   // position-only user reward: one f64 per (type, cell)
                                    r = *(__attribute__((address_space(3))) const double*)(uintptr_t)((hw & kHwCellMask) + rt_add);
                            }
                            r = reward_if_live(r, af & 0x04u);
                            if (valid) *(__attribute__((address_space(1))) double*)(PLAIN ? (gchar*)a_rew : b_rew + rew_off) = r;
                        }
                        if (valid) {
                            if (has_af) *(__attribute__((address_space(1))) uint8_t*)(PLAIN ? (gchar*)a_af : b_af + af_off) = (uint8_t)af;
                            if (has_ef && i == 0) *(__attribute__((address_space(1))) uint8_t*)(PLAIN ? (gchar*)a_ef : b_ef + ef_off) = (uint8_t)efw;
                            if (has_act)
                                *(__attribute__((address_space(1))) uint8_t*)(b_act + af_off) = (uint8_t)(hw >> kHwActionShift);
                        }
                        if constexpr (PLAIN) {
                            a_rew += EN32 * 8u;
                            a_af += EN32;
                            a_ef += E32;
                        } else {
                            rew_off += EN32 * 8u;
                            af_off += EN32;
                            ef_off += E32;
                        }
                    }
                    CCX_STAMP(1);                        // reward + flag bytes
                    if (rows_l) {
                        const uint32_t ok0_l = in_vgpr(v_ok0), jmax_l = in_vgpr(v_jmax);
                        wave_lds_sync();
                        // (one step's rows: gather from the staging slot OFF bytes behind the writer's first one, store, advance)
                        auto emit_rows = [&](auto off_c) {
                            constexpr uint32_t OFF = decltype(off_c)::value;
                            // all LDS reads of a batch first (idle lanes read the constant slot), so the
                            // wave pays one LDS latency per batch, then the stores
                            typedef __attribute__((address_space(3))) const v2f lds_f2;
                            auto one_batch = [&](auto j0c) {
                                constexpr int J0 = decltype(j0c)::value;
                                if ((it0 + it_step * J0) < it_end) {
                                    v2f va[kObsBatch], vb[kObsBatch];
        #pragma unroll
                                    for (int j = 0; j < kObsBatch; ++j) {
                                        va[j] = *(lds_f2*)(uintptr_t)(oa0[J0 + j] + OFF);
                                        if constexpr (PAIR) vb[j] = *(lds_f2*)(uintptr_t)(oa1[J0 + j] + OFF);
                                    }
                                    const uint32_t em = EDGE ? (edge_mask >> J0) & ((1u << kObsBatch) - 1u) : 0u;   // wave-uniform
                                    auto one_store = [&](auto jc) {
                                        constexpr int J = J0 + decltype(jc)::value, JL = decltype(jc)::value;
                                        constexpr uint32_t BYTES = (uint32_t)J * 64u * (PAIR ? 16u : 8u);   // offset of iteration J from my first
                                        constexpr int IMM = (int)(BYTES & 4095u);
                                        const uint32_t voff = BYTES < 4096u ? q0_off : BYTES < 8192u ? q0_off_4k : q0_off_8k;
                                        if (J == 0 ? (ok0_l != 0u) : ((uint32_t)J < jmax_l)) {
                                            const bool edge = EDGE && ((em >> JL) & 1u);
                                            if constexpr (PAIR) {
                                                v4f v = {va[JL].x, va[JL].y, vb[JL].x, vb[JL].y};
                                                if (edge) *reinterpret_cast<v4f*>(obs_s + (q0_off + BYTES)) = v;
                                                else store_obs_at<IMM>(v, obs_s, voff);
                                            } else {
                                                if (edge) *reinterpret_cast<v2f*>(obs_s + (q0_off + BYTES)) = va[JL];
                                                else store_obs_at<IMM>(va[JL], obs_s, voff);
                                            }
                                        }
                                    };
                                    one_store(std::integral_constant<int, 0>{});
                                    one_store(std::integral_constant<int, 1>{});
                                    one_store(std::integral_constant<int, 2>{});
                                    one_store(std::integral_constant<int, 3>{});
                                    one_store(std::integral_constant<int, 4>{});
                                    static_assert(kObsBatch == 5, "one_store is spelled out five times");
                                }
                            };
                            if constexpr (VARLEAD) {
                                // OUTM 3: the slab stride is NOT a multiple of 128 bytes (a batch size off rows_alignment(): 50 agents x
                                // 1004 envs), so the region's place within its line moves from step to step.  `lead`, the line base, the
                                // iteration count and the edge iterations are worked out per STEP and every iteration takes its source
                                // address from the table (the register-cached addresses of the first ten assume one lead per launch);
                                // the region-relative stores of round 1 ran such batches at half the rate (profiles/r04_c5_scan.txt).
                                const uint32_t lead_s = __builtin_amdgcn_readfirstlane((uint32_t)(reinterpret_cast<uintptr_t>(obs_s) & 127u) / vbytes);
                                char* const base_s = obs_s - lead_s * vbytes;
                                const int n4l_s = n4 + (int)lead_s, total_s = (n4l_s + 63) >> 6;
                                const int it_end_s = it_end == total_its ? total_s : it_end;      // (the last writer takes the extra iteration)
                                const int e_first = (lead_s != 0u && it0 == 0) ? 0 : -1;
                                const int e_last = ((((uint32_t)n4l_s * vbytes) & 127u) != 0u && it_end == total_its) ? total_s - 1 : -1;
                                for (int it = it0; it < it_end_s; it += it_step) {
                                    const int ql = lane + 64 * it;
                                    const uint32_t q = (uint32_t)ql - lead_s;
                                    if (q >= (uint32_t)n4) continue;
                                    const bool plain_st = it == e_last || it == e_first;      // wave-uniform: a line shared with the neighbouring tile
                                    if constexpr (PAIR) {
                                        const uint32_t t = reinterpret_cast<const uint32_t*>(table)[q];
                                        float2 a2 = *reinterpret_cast<const float2*>(sbase + OFF + (t & 0xFFFFu));
                                        float2 b2 = *reinterpret_cast<const float2*>(sbase + OFF + (t >> 16));
                                        v4f v = {a2.x, a2.y, b2.x, b2.y};
                                        if (plain_st) *reinterpret_cast<v4f*>(base_s + (size_t)ql * 16) = v;
                                        else store_obs(v, reinterpret_cast<v4f*>(base_s + (size_t)ql * 16));
                                    } else {
                                        const float2 v2 = *reinterpret_cast<const float2*>(sbase + OFF + table[q]);
                                        if (plain_st) *reinterpret_cast<float2*>(base_s + (size_t)ql * 8) = v2;
                                        else store_obs(v2, reinterpret_cast<float2*>(base_s + (size_t)ql * 8));
                                    }
                                }
                            } else {
                            one_batch(std::integral_constant<int, 0>{});
                            one_batch(std::integral_constant<int, kObsBatch>{});
                            static_assert(kFastObsIters == 2 * kObsBatch, "one_batch is spelled out twice");
                            // beyond the register-cached iterations: table-driven
                            for (int it = it0 + it_step * kFastObsIters; it < it_end; it += it_step) {
                                const int ql = lane + 64 * it;
                                const uint32_t q = (uint32_t)ql - lead;
                                if (q >= (uint32_t)n4) continue;
                                if constexpr (PAIR) {
                                    const uint32_t t = reinterpret_cast<const uint32_t*>(table)[q];
                                    float2 a2 = *reinterpret_cast<const float2*>(sbase + OFF + (t & 0xFFFFu));
                                    float2 b2 = *reinterpret_cast<const float2*>(sbase + OFF + (t >> 16));
                                    v4f v = {a2.x, a2.y, b2.x, b2.y};
                                    if (EDGE && it == edge_last) *reinterpret_cast<v4f*>(obs_s + (size_t)ql * 16) = v;
                                    else store_obs(v, reinterpret_cast<v4f*>(obs_s + (size_t)ql * 16));
                                } else {
                                    const float2 v2 = *reinterpret_cast<const float2*>(sbase + OFF + table[q]);
                                    if (EDGE && it == edge_last) *reinterpret_cast<float2*>(obs_s + (size_t)ql * 8) = v2;
                                    else store_obs(v2, reinterpret_cast<float2*>(obs_s + (size_t)ql * 8));
                                }
                            }
                            }   // (!VARLEAD)
        #ifndef CCX_SAME_SLAB   /* diagnostic: every step overwrites slab 0 (L2-resident) */
                            obs_s += obs_stride;
        #endif
                        };
                        emit_rows(std::integral_constant<uint32_t, 0u>{});
                        if constexpr (PAIRS_C) {
                            if (pair) emit_rows(std::integral_constant<uint32_t, (uint32_t)sizeof(WSlot)>{});
                        }
                        wave_lds_sync();
                    }
                    CCX_STAMP(2);                        // observation gather + stores
                    // store throttle: many small tiles oversubscribe the HBM write queues and the drain
                    // rate of the whole chip drops (measured: DESIGN.md 3.6); bounding the stores a
                    // writer keeps in flight keeps the memory side in its efficient regime
                    {   // (opaque inside the loop: else the eleven threshold tests of wait_vm_at_most become eleven loop-invariant
                        // SGPR pairs that are spilled and re-read every step -- for a throttle that is off in most shapes)
                        uint32_t wv = wvm;
                        asm volatile("" : "+s"(wv));
                        if (wv) wait_vm_at_most(wv);
                    }
                    if constexpr (PAIRS_C) {
                        if (pair) ++s;                                  // this iteration took steps s and s + 1
    #ifdef CCX_DIAG_WAITS
                        if (pair) ++diag_pairs;
    #endif
                    }
                }
            };
            typedef std::integral_constant<int, 0> c0_t;
            typedef std::integral_constant<int, 1> c1_t;
            typedef std::integral_constant<int, 2> c2_t;
            if (small_out && !my_obs) {   // (writer 0 of a role-split tile is what compact / no-observation rollouts wait for:
                                          //  its two hand-off modes are compiled apart as well, +10 % there)
                if (flags_mode) writer_loop(c1_t{}, c0_t{}, c1_t{}, c0_t{});
                else writer_loop(c1_t{}, c0_t{}, c0_t{}, c0_t{});
            } else if (!small_out && my_obs) {
                if (pair_ok && flags_mode) writer_loop(c0_t{}, c1_t{}, c1_t{}, c1_t{});   // two steps per iteration where possible
                else writer_loop(c0_t{}, c1_t{}, c2_t{}, c0_t{});
            } else {
                writer_loop(c2_t{}, c2_t{}, c2_t{}, c0_t{});
            }
            if (w == 0) { CCX_STAMP_FLUSH(KA.counters, 4); }
            if (w == nw - 1) CCX_T(7);      // (the last writer of tile 0: all its stores acknowledged)
#ifdef CCX_DIAG_WAITS   // counters[8 + 2w] += steps on which writer w found nothing staged yet, [9 + 2w] += its empty polls (w < 3)
            if (KA.counters && lane == 0 && w < 3) {
                atomicAdd(&KA.counters[8 + 2 * w], (unsigned long long)diag_waited_steps);
                atomicAdd(&KA.counters[9 + 2 * w], (unsigned long long)diag_polls);
                if (w == 1) atomicAdd(&KA.counters[6], (unsigned long long)diag_pairs);   // two-step iterations of writer 1
            }
#endif
            return;
        }
    }

    // =========================================================================================
    // SIM wave: the state transition (reference phases :188-212, :219-241 and the auto-reset)
    // =========================================================================================
    // One env-step of a tile is ONE dependent chain on ONE wavefront (512 tiles on 1024 SIMDs: nothing else runs on
    // this SIMD), so what counts is the latency of that chain, not instruction throughput.  On gfx950 a dependent VALU
    // op costs ~5 clocks, but every VALU -> SALU -> branch hop costs 30-50 and an LDS round trip 50-100
    // (profiles/scratch/ilat.hip).  The step is therefore written as straight-line VALU code: lane masks are consumed
    // by VALU instructions (v_cndmask on the compare's own SGPR pair), counters are scalar popcounts of ballots that
    // the SALU adds in the shadow of VALU work, and the two rare events of a step -- a move-order chain longer than two
    // links, an env restart -- are ONE scalar branch each whose condition was computed well before it is tested.
    // The wave issues ahead of the writer waves (priority 0) wherever they meet -- the same SIMD, the LDS, the scalar cache.
    __builtin_amdgcn_s_setprio(3);
    constexpr uint32_t msz = sizeof(mask_t);
    constexpr uint32_t TS = (GLOG == 6) ? 1u : 0u;     // a table entry {occ, prp} is 8 bytes (32-bit masks) or 16
    typedef mask_t mask2_t __attribute__((ext_vector_type(2)));
    const mask_t full = full_mask<GLOG>();
    const mask_t lo_m = low_mask<mask_t>(i);
    const mask_t later_m = ~lo_m & ~(mask_t(1) << i);
    const uint32_t gsh = (uint32_t)lane & ~(uint32_t)(G - 1);      // first lane of my env's lane group
    // Occupancy / proposal bit table of this lane's env: one entry {occ, prp} of move-rank masks per cell of the
    // padded grid (+ one dump entry).  Agents with nothing to publish OR their bit into the env's dump entry; lanes
    // WITHOUT an agent (half-empty waves of small batches, padded lane groups) get dump entries of their own on the top
    // border row (y = -1, never occupied): 32+ lanes hammering one word with same-address LDS atomics cost such tiles
    // 10 % per step, while steering the few idle agents of an env to its one dump entry is cheaper than letting them OR
    // a zero into their own cells.
    // All LDS traffic of the step loop goes through 32-bit LDS addresses (address_space(3) accesses: no generic-pointer
    // arithmetic, no `+ base` per access); lds0 = where the dynamic LDS segment starts (0: the kernel has no static LDS).
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const uint32_t cells1 = cells + 1u;
    const uint32_t g_tab = (g < p.EW) ? (uint32_t)g : 0u;   // lanes beyond the tile's envs use env 0's table (zeros only)
    const uint32_t tab_abs = lds0 + p.off_tiles + (uint32_t)tile_in_block * p.tile_stride + p.off_occ + g_tab * cells1 * 2u * msz;
    const uint32_t tab_rel = tab_abs - (lds0 << TS);         // table entry of the cell whose word sits at c8: tab_rel + (c8 << TS)
    const uint32_t dump_addr = tab_abs + ((valid ? cells : (uint32_t)(lane % Wp)) << (3u + TS));
    auto lds_or = [](uint32_t addr, mask_t bits) {
        __hip_atomic_fetch_or((__attribute__((address_space(3))) mask_t*)(uintptr_t)addr, bits, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_WAVEFRONT);
    };
    auto lds_mask_st = [](uint32_t addr, mask_t v) { *(__attribute__((address_space(3))) mask_t*)(uintptr_t)addr = v; };
    auto lds_cell = [](int addr) { return *(__attribute__((address_space(3))) const unsigned long long*)(uintptr_t)(uint32_t)addr; };

    // ---- state -> registers ------------------------------------------------------------------
    // position = byte offset of the agent's cell in the per-cell geometry table (cell index x 8): the cell word, the
    // table entry and the target of a move are all one add away
    int c8 = (int)lds0 + cell_origin(Wp) * 8;   // LDS address of the word of cell (0,0)
    int stepc = 0, episode = 0;
    uint32_t act = 0;                         // 0/1
    uint32_t tt = 1u;                         // terminated | truncated << 1; lanes without an agent count as done
    if (valid) {   // (loaded in front of the prologue's barrier)
        c8 = (int)lds0 + ((s_y + 1) * Wp + s_x + 1) * 8;   // = cell_index(s_x, s_y, Wp), inline: the call changed all 32 <3,..> instantiations
        act = s_active != 0u;
        tt = tt_entry;
    }
    if (valid_env) {
        stepc = s_stepc;
        episode = s_episode;
    }
    // steps left before truncation, minus one: negative from the step on which step_count reaches max_steps (truncateds.py:56)
    int left1 = p.max_steps - 1 - stepc;   // (max_steps_m1 is defined further down)
    unsigned long long ci = lds_cell(c8);
    uint32_t ilo = (uint32_t)ci;   // (the low word: legality bits, info bits, destination flags, x / y; the writers look the rest up)
    const bool term_all = p.term_mode == CCX_K_TERM_ALL;          // wave-uniform

    // move deltas in the padded grid x 8 (bytes of the geometry table), one int16 per action 0..3 (actions.py:18-24);
    // action 4 (wait / absent) wraps to entry 0 of the 64-bit shift -- harmless: its legality bit (bit 4 of the cell
    // word) is always 0, so the neighbour that is looked at is never entered
    const unsigned long long lut64 = (unsigned long long)(uint16_t)8 | ((unsigned long long)(uint16_t)(Wp * 8) << 16) |
                                     ((unsigned long long)(uint16_t)(-8) << 32) |
                                     ((unsigned long long)(uint16_t)(-Wp * 8) << 48);

    // reset-pool cursor of this env: entry (global_env + episode*total) mod P, advanced by
    // total mod P per episode; the NEXT placement is prefetched right after every reset and only
    // decoded when it is consumed (so no wait sits behind the load).
    uint32_t pool_idx = 0, pnext = 0;
    int pcell8 = (int)lds0 + cell_origin(Wp) * 8;
    bool pnext_pending = false;   // pnext holds a load that has not been decoded into pcell8 yet
    const bool use_pool = KA.auto_reset && KA.pool != nullptr && p.pool_size > 0;
    const uint32_t pool_size = (uint32_t)p.pool_size, pool_stride = (uint32_t)p.pool_stride;
    if (use_pool && valid) {
        pool_idx = (uint32_t)pool_entry((unsigned long long)(p.env_offset + env), (unsigned long long)(episode + 1),
                                        (unsigned long long)p.pool_stride, (unsigned long long)p.pool_size);
        pnext = *reinterpret_cast<const uint16_t*>(KA.pool + ((size_t)pool_idx * N + i) * 2);
        pnext_pending = true;
    }
    const uint64_t may_reset_b = __builtin_amdgcn_ballot_w64(use_pool && valid_env);   // lanes of envs that may restart
    const uint64_t slot0_b = __builtin_amdgcn_ballot_w64(valid_env && i == 0);         // one lane per env of the tile
    const uint32_t reset_bit = use_pool ? (uint32_t)CCX_K_EF_RESET : 0u;     // wave-uniform

    // (kernel arguments the step loop needs are read HERE, once: a scalar load inside the loop shares the LDS wait counter)
    const uint32_t rng_lo = p.rng_lo, rng_hi = p.rng_hi, eps_thr = p.eps_thr, genv = (uint32_t)(p.env_offset + env);
    const int max_steps_m1 = p.max_steps - 1;
    const GreedyGeo geo{p.div, p.dc, p.bdy, p.edy};
    const bool has_order = PLAIN ? false : KA.order != nullptr;   // wave-uniform
    const uint8_t* ord_p = KA.order + idx;

    // throughput counters.  Arrivals need no per-step work at all: an agent stops being active only by arriving
    // (:210-212) and becomes active again only by a restart, so arrivals = active at the start - active at the end +
    // inactive agents re-activated by restarts.
    uint32_t c_moves = 0, c_live = 0, c_episodes = 0;      // c_moves / c_live: per-lane, summed over the wave at the end
    auto add_mask = [](uint32_t& acc, uint64_t lane_mask) {   // acc += (my bit of lane_mask): ONE v_addc_co with the mask as carry-in
        asm("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(acc) : "s"(lane_mask) : "vcc");
    };
    uint32_t c_arrivals = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(act != 0));
    CCX_STAMP_DECL;

    // (the first burst of actions was requested in front of the prologue's barrier)
    CCX_T(3);

    // ---- sim -> writer hand-off (ccx_kernels.h: HandOff) -----------------------------------------------------------
    // flags mode: a ring of p.stage_slots slots, a sequence word the sim wave bumps after every slot it has written and
    // one progress word per writer wave: neither side ever waits on a barrier; the sim wave only checks (with a read it
    // issued at the top of the step) that the slowest writer is less than a ring behind.
    const uint32_t sync_abs = lds0 + p.off_tiles + (uint32_t)tile_in_block * p.tile_stride + kSyncOff;
    auto sync_ld = [](uint32_t addr) {
        return __hip_atomic_load((__attribute__((address_space(3))) uint32_t*)(uintptr_t)addr, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto sync_st = [](uint32_t addr, uint32_t v) {
        __hip_atomic_store((__attribute__((address_space(3))) uint32_t*)(uintptr_t)addr, v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    const uint32_t prog_addr = sync_abs + 4u * (kSyncProg + ((uint32_t)lane & 7u));
    const uint32_t stage_abs = lds0 + p.off_tiles + (uint32_t)tile_in_block * p.tile_stride + kStageOff + (uint32_t)lane * 4u;
    const bool flags_mode = OUT && p.hand_flags != 0u;          // wave-uniform
    // (pinned in VGPRs where the budget allows: the plain instantiations; the policy / move-order ones are at their 128)
    const uint32_t seq_addr = PLAIN ? in_vgpr(sync_abs + 4u * kSyncSeq) : sync_abs + 4u * kSyncSeq;
    uint32_t seq_v = PLAIN ? in_vgpr(0u) : 0u;                   // steps staged so far (what the sequence word holds)

    // ---- step pacing: a smooth, absolute schedule for the output stream (DESIGN.md 3.6) ----------
    uint32_t pace = 0, pace_base = 0, pace_floor = 0, pace_skip = 0;
    unsigned long long pace_t0 = 0, pace_due = 0;   // ticks, ticks x 256 since t0
    if (launch_is_paced(p.pace_state != nullptr, want_obs, K, p.pace_min_k)) {   // (short launches: not worth the load)
        // pace_state: [0], [1] = the pace slots (one is read, the other collects this launch's votes),
        // [2] = floor: the pace just above the last collapse; it decays by 0.1 % per launch at first
        // and twice as fast after every 8 further launches without a collapse ([3] counts them), so
        // that a transient (the first milliseconds of a process collapse at paces that are fine
        // later) does not hold the pace up for long while a persistent cliff is approached slowly;
        // [4]..[7] = cliff memory (below)
        const uint32_t voted = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + p.pace_slot);
        const uint32_t floor_fp = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 2);
        pace_base = __builtin_amdgcn_readfirstlane(voted > floor_fp ? voted : floor_fp);
        pace_floor = __builtin_amdgcn_readfirstlane(floor_fp);
        // The common pace is per workgroup for a FULL device (p.resident_blocks at once).  A grid of
        // more workgroups runs in rounds; the workgroups of a partial last round share the same
        // memory among fewer, so their schedule is proportionally faster (else 1024 workgroups on 768
        // slots would spend their second round at a third of the drain rate).
        pace = pace_base;
        const bool one_round = (p.launch_flags & CCX_K_LAUNCH_ROUND) != 0u;    // (this launch is one round of a larger grid)
        if (p.resident_blocks && (one_round || gridDim.x > p.resident_blocks)) {
            const uint32_t first = one_round ? 0u : (blockIdx.x / p.resident_blocks) * p.resident_blocks;
            const uint32_t left = gridDim.x - first;
            if (left < p.resident_blocks) {
                pace = (uint32_t)(((unsigned long long)pace_base * left) / p.resident_blocks);
                pace = pace ? pace : 1u;
            }
        }
        if (launch_is_adaptive(p.pace_state != nullptr, p.pace_adapt != 0u, want_obs, K, p.pace_min_k, p.adapt_min_k) && tile == 0 && lane == 0) {
            p.pace_state[p.pace_slot ^ 1u] = 0u;               // the votes of this launch are collected here
            const uint32_t streak = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 3);
            // Cliff memory: the collapsed tiles of the previous launch left its pace in [6].  A collapse
            // within 3 % of the one before ([4]) confirms where the cliff of this box and shape is ([5]
            // counts confirmations); from then on the floor starts 1.6 % above it and is let down slowly and
            // steadily (rates below, no acceleration), so the controller sits 0.5-1.5 % above a cliff it
            // knows instead of walking back into it every 15-20 launches.  Collapses during the first 16 launches of a
            // controller do not count (a process collapses at paces that are fine a few milliseconds later).
            // The cliff is a sharp threshold of the chip (profiles/r02_lag_trace_*.txt: 3 % below it two launches in
            // five lose 20 %, 1 % above it one in fifty does), so once it is known there is little to probe for:
            // 0.024 % per launch after two confirmations, 0.012 % after four.
            const uint32_t mark = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 6);
            uint32_t confirmed = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 5);
            const uint32_t launches = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 7);
            if (mark) {
                const uint32_t cliff = *reinterpret_cast<volatile const uint32_t*>(p.pace_state + 4);
                const uint32_t gap = mark > cliff ? mark - cliff : cliff - mark;
                if (launches >= 16u) confirmed = (cliff && gap < (cliff >> 5)) ? (confirmed < 8u ? confirmed + 1u : 8u) : 1u;
                p.pace_state[4] = mark;
                p.pace_state[5] = confirmed;
                p.pace_state[6] = 0u;
            }
            p.pace_state[7] = launches < 100000u ? launches + 1u : launches;
            // a confirmed cliff: the floor need not sit 2.5 % above it (the margin for an unknown one), 1.6 % will
            // do, and it is let down very slowly, without acceleration
            uint32_t fl = floor_fp;
            if (mark && confirmed >= 2u && fl > mark + (mark >> 6)) fl = mark + (mark >> 6);
            const uint32_t sh = confirmed >= 4u ? 13u : confirmed >= 2u ? 12u : 10u - (streak >= 32u ? 4u : streak >> 3);
            p.pace_state[2] = fl - (fl >> sh);
            p.pace_state[3] = streak < 1000u ? streak + 1u : streak;
        }
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pace_t0)::"memory");
        if (p.pace_phase) {
            // tunable: the tiles of a round do not start their steps together but spread over the step
            // period -- 1: in tile order (the chip then writes one narrow window that sweeps through the
            // step's slab), 2: hashed.  Only the tile's own t0 moves; the schedule and the controller's
            // lateness test are relative to it.
            // (a launch that is one round of a larger grid phases its own tiles over the period, however many they are)
            const bool round_launch = (p.launch_flags & CCX_K_LAUNCH_ROUND) != 0u;
            const uint32_t per_round = (round_launch || !p.resident_blocks ? gridDim.x : p.resident_blocks) * (uint32_t)tpb;
            const uint32_t tr = ((uint32_t)tile - (round_launch ? p.block_base * (uint32_t)tpb : 0u)) % per_round;
            uint32_t frac16;
            if (p.pace_phase == 1u) {
                frac16 = (tr << 16) / per_round;                       // one window for the whole chip
            } else if (p.pace_phase == 3u) {
                const uint32_t per_xcd = per_round >> 3;               // one window per XCD (tile_map 0)
                frac16 = per_xcd ? ((tr % per_xcd) << 16) / per_xcd : 0u;
            } else {
                frac16 = __brev(tr * 2654435761u) & 0xFFFFu;
            }
            pace_t0 += ((unsigned long long)pace * frac16) >> 24;
        }
    }

    int s = 0;
    uint32_t wprog = 0x7FFFFFFFu;
#ifdef CCX_DIAG_WAITS
    uint32_t diag_lag_steps = 0, diag_lag_spins = 0;
#endif
    for (int s0 = 0; s0 < K; s0 += kActBatch) {
        // the burst issued one batch ago is consumed here: ONE vmcnt wait per kActBatch steps.
        // Actions are clamped to 0..4 (4 = wait; 255 = absent and anything else: no move).
        uint32_t apk[2] = {0, 0};
#pragma unroll
        for (int d = 0; d < kActBatch; ++d) {
            const uint32_t a4 = araw[d] < 4u ? araw[d] : 4u;
            apk[d >> 3] |= a4 << (4 * (d & 7));
        }
        unsigned long long acur = in_vgpr((unsigned long long)apk[0] | ((unsigned long long)apk[1] << 32));
        if (pnext_pending) {   // decode behind the wait that just happened: costs nothing
            // (= cell_of_placement(pnext, Wp), inline here and below: the call cost 10 of 16 v128<3,..> an SGPR spill)
            pcell8 = (int)lds0 + ((int)(pnext >> 8) * Wp + (int)(pnext & 0xFFu) + Wp + 1) * 8;
            pnext_pending = false;
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the next burst BEHIND the wait above
        if (!policy && s0 + kActBatch < K) fetch_actions(s0 + kActBatch);
        __builtin_amdgcn_sched_barrier(0);
        const int dmax = __builtin_amdgcn_readfirstlane((K - s0) < kActBatch ? (K - s0) : kActBatch);
        // hand-off ring: how far have the writer waves got?  Asked once per burst (and again only when the answer is
        // too old to prove that a slot is free); a step compares its own number with that possibly stale value
        if constexpr (OUT) wprog = sync_ld(prog_addr);   // (barrier mode too: the writers publish their progress in both)
        // the action of a step is unpacked during the step before it (in the shadow of that step's LDS round trip)
        uint32_t a_cur = (uint32_t)acur & 0xFu, sh_cur = a_cur << 4;
        acur >>= 4;

        for (int d = 0; d < dmax; ++d, ++s) {
            if (pace) {   // env-step s is due at t0 + s * pace; a late tile does not wait (it catches up)
                const unsigned long long due = pace_t0 + (pace_due >> 8);
                pace_due += pace;
                if (pace_skip) {
                    --pace_skip;             // clearly behind schedule a moment ago: do not even look
                } else {
                    unsigned long long now;
                    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
                    // reading the clock stalls the step chain (scalar-memory round trip): a tile that is
                    // more than half a step behind (batches too small to be memory-bound, or a collapse)
                    // checks again only three steps later
                    if ((long long)(now - due) > (long long)(pace >> 9)) pace_skip = 3;
#ifdef CCX_LAG_TRACE   // diagnostic (profiles/scratch/lag_trace.py): how far behind its schedule is this tile, step by step
                    if (p.lag_trace && lane == 0 && tile % p.lag_every == 0 && tile / p.lag_every < 16 && s < 4096)
                        p.lag_trace[(tile / p.lag_every) * 4096 + s] = (int)(long long)(now - due);
#endif
                    while ((long long)(due - now) > 0) {
                        __builtin_amdgcn_s_sleep(1);
                        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
                    }
                }
            }
            uint32_t a = a_cur;


            // ---- move rank of this agent (dict order of action_dict, collectivecrossing.py:197)
            int rank = i;
            if (has_order) {
                uint32_t ok_ = valid ? (uint32_t)*ord_p : (uint32_t)i;  // agent moved i-th
                ord_p += EN;
                xch[gbase + (ok_ & (G - 1))] = (uint32_t)i;
                wave_lds_sync();
                rank = (int)xch[lane];
                wave_lds_sync();
            }
            const mask_t mybit = mask_t(1) << rank;
            const uint32_t ca = act ? tab_rel + ((uint32_t)c8 << TS) : dump_addr;   // my occupancy word

            // ---- 0. policy-driven rollout: the reference's GreedyPolicy(epsilon = 0) picks the action
            //         from the pre-step state (greedy_policy.py:33-449).  The occupancy bits are
            //         published first; a direction is free if the current cell's word says the
            //         neighbour is enterable and no other active agent's bit sits on it.
            uint32_t a_out = a;
            const bool occ_policy = policy == CCX_K_POLICY_GREEDY || policy == CCX_K_POLICY_WAITING;
            if (policy == CCX_K_POLICY_RANDOM) {
                // uniform random actions drawn ON THE DEVICE (SURVEY 8b: ccx_rollout's rng_seed): a counter-based
                // hash of (seed, global env, episode, step of the episode, agent slot), so the stream of an env does
                // not depend on how launches are split or on the world size
                const uint32_t asked = tt == 0u;
                const uint32_t r = random_action(rng_lo, rng_hi, genv, (uint32_t)episode, (uint32_t)(max_steps_m1 - left1), (uint32_t)i);
                a = asked ? r : 4u;
                a_out = asked ? r : (uint32_t)CCX_K_ABSENT;
            }
            if (occ_policy) {
                // which of my four neighbour cells hold another ACTIVE agent right now (greedy_policy.py:238-264 via
                // _is_move_valid -> _is_position_occupied, collectivecrossing.py:536-541)
                uint32_t busy;
                if constexpr (OCC) {
                    lds_or(ca, mybit);
                    wave_lds_sync();
                    busy = neighbours_busy<mask_t, TS>(tab_rel + ((uint32_t)c8 << TS), Wp);
                    wave_lds_sync();
                } else {
                    // grids whose occupancy tables exceed the LDS (round 4: policy rollouts no longer need them): every agent
                    // posts its cell in the exchange tile and compares its four neighbours with its env's entries, O(G)
                    const uint32_t me = ((uint32_t)c8 - lds0) >> 3;
                    xch[lane] = act ? me : 0x8000u;                 // (inactive agents block nobody; cell indices stay below 2^15)
                    wave_lds_sync();
                    const uint32_t n0 = me + 1u, n1 = me + (uint32_t)Wp, n2 = me - 1u, n3 = me - (uint32_t)Wp;
                    busy = 0;
                    for (int k2 = 0; k2 < G; ++k2) {
                        const uint32_t v = xch[gbase + k2];
                        busy |= (v == n0 ? 1u : 0u) | (v == n1 ? 2u : 0u) | (v == n2 ? 4u : 0u) | (v == n3 ? 8u : 0u);
                    }
                    wave_lds_sync();                                // (xch is rewritten by the conflict masks below)
                }
                const uint32_t cand = greedy_candidates(geo, boarding, (int)cell_x(ilo), (int)cell_y(ilo));
                uint32_t pick = greedy_pick(cand, cell_legal4(ilo) & ~busy);
                const uint32_t asked = tt == 0u;   // policy is asked for env.agents only
                if (policy == CCX_K_POLICY_WAITING) {
                    // waiting_policy.py:74-131: boarding agents outside the tram area wait while
                    // a live exiting agent is not on its destination row yet
                    const uint32_t pend = (boarding ? 0u : asked) & (((ilo >> kCellExitingShift) & 1u) ^ 1u);   // (= !cell_at_dest, inline: the call moved every v128<3,..> schedule)
                    const mask_t pend_bits = group_bits<GLOG>(__builtin_amdgcn_ballot_w64(pend != 0), lane);
                    if (boarding && !(ilo & kCellInTram) && pend_bits != 0) pick = 4u;
                }
                if (eps_thr) {
                    // epsilon-greedy (greedy_policy.py:48-59): with probability epsilon one of the VALID actions
                    // of the pre-step state, uniformly; counter-based draws (ccx_kernels.h: explore_action)
                    const uint32_t u = random_word(rng_lo, rng_hi ^ kEpsStream, genv, (uint32_t)episode,
                                                   (uint32_t)(max_steps_m1 - left1), (uint32_t)i);
                    if (u < eps_thr) pick = explore_action(u, cell_legal4(ilo) & ~busy);
                }
                a = asked ? pick : 4u;
                a_out = asked ? pick : (uint32_t)CCX_K_ABSENT;
            }

            left1 -= 1;  // collectivecrossing.py:188: step_count += 1

            // ---- 1. proposal (collectivecrossing.py:371-376, 509-534; :565-588 adds nothing):
            //         legality is a bit of the CURRENT cell's word (bit a; bit 4 is 0: waiting never "moves"); the
            //         target's word is requested now and consumed after the move is decided
            const int np8 = c8 + (int)(int16_t)(uint16_t)(lut64 >> (policy ? (a << 4) : sh_cur));
            const uint32_t ok = (ilo >> a) & act;               // = cell_legal(ilo, a) & act; act is 0/1: only bit 0 survives (inline: the call re-scheduled every instantiation)
            const uint32_t nok = ok ^ 1u;

            // ---- 2. conflict masks over move ranks: Cm = earlier ranks standing on my target,
            //         Pm = earlier ranks proposing my target, H != 0 = cannot move whatever the
            //         earlier ranks do (no legal proposal, or a later rank still on the target)
            unsigned long long pci;
            mask_t Cm, Pm, H;
            mask2_t tt2 = {0, 0};
            uint32_t qa = dump_addr;
            if constexpr (OCC) {
                const uint32_t ta = tab_rel + ((uint32_t)np8 << TS);                   // the target's table entry
                qa = (ok ? ta : dump_addr) + msz;                                      // my proposal word
                pci = lds_cell(np8);
                if (!occ_policy)   // (already published for the scripted policies)
                    lds_or(ca, mybit);
                lds_or(qa, mybit);
                wave_lds_sync();
                tt2 = *(__attribute__((address_space(3))) const mask2_t*)(uintptr_t)ta;   // {occ, prp} of the target
                wave_lds_sync();
            }
            // ---- in the shadow of that round trip (~60 clocks in which independent instructions issue for free): the part
            //      of the tail that does not depend on the move -- liveness (rewards.py:64, truncateds.py:56: neither
            //      terminated nor truncated BEFORE this step), truncation (truncateds.py:40-61) -- the progress of the
            //      writer waves, and the unpacking of the NEXT step's action
            const bool live_lane = tt == 0u;
            const uint64_t live_b = __builtin_amdgcn_ballot_w64(live_lane);
            // (in_vgpr: an empty asm that pins the computation HERE -- the compiler would otherwise sink it behind the
            // branch below, next to its first use, out of the shadow)
            const uint32_t ge_m = in_vgpr((uint32_t)(left1 >> 31));    // all ones from the step that reaches max_steps
            const uint32_t trunc2 = in_vgpr(live_lane ? (ge_m & 2u) : 0u);   // truncated bit of the flag pair
            uint32_t live_grp;                                         // != 0: some agent of my env is live
            if constexpr (GLOG == 6) live_grp = in_vgpr((uint32_t)live_b | (uint32_t)(live_b >> 32));
            else live_grp = in_vgpr((uint32_t)(live_b >> gsh) & (uint32_t)full);
            // hand-off ring: the slot this step will overwrite held step s - p.stage_slots; every writer must have read it
            // (with a barrier per step they always have)
            const uint64_t lag_b = OUT ? __builtin_amdgcn_ballot_w64((int)wprog < s - (int)stage_mask) : 0ull;
            a_cur = (uint32_t)acur & 0xFu;
            sh_cur = a_cur << 4;
            acur >>= 4;
            if constexpr (OCC) {
                const mask_t occ_t = tt2.x, prp_t = tt2.y;
                // ranks are positions in the move order: rank r's masks are compared in RANK space
                const mask_t lo_r = has_order ? low_mask<mask_t>(rank) : lo_m;
                const mask_t later_r = has_order ? (~lo_r & ~mybit) : later_m;
                Cm = occ_t & lo_r;
                Pm = prp_t & lo_r;
                H = (occ_t & later_r) | (mask_t)nok;
            } else {
                // all-pairs through the xch tile, indexed by rank: this lane plays move-rank i.
                // Entries of unused lanes hold cur 0x8000 / prop 0xFFFF and never match.
                pci = lds_cell(np8);
                const uint32_t curkey = act ? ((uint32_t)c8 - lds0) >> 3 : 0x8000u;
                const uint32_t propkey = ok ? ((uint32_t)np8 - lds0) >> 3 : 0xFFFFu;
                xch[gbase + rank] = curkey | (propkey << 16);
                wave_lds_sync();
                const uint32_t myprop = xch[lane] >> 16;
                mask_t call, pall;
                if constexpr (GLOG <= 4) {
                    // both 16-bit compares of an entry in 3 VALU ops: xor with (prop,prop), clamp
                    // each half to 0/1 ("differs"), shift into a packed accumulator
                    const uint32_t mp2 = myprop | (myprop << 16);
                    uint32_t acc = 0;
#pragma unroll
                    for (int k2 = G - 1; k2 >= 0; --k2) {
                        const uint32_t t = xch[gbase + k2] ^ mp2;
                        uint32_t ne;   // per 16-bit half: 1 if it differs, 0 if equal
                        asm("v_pk_min_u16 %0, %1, %2" : "=v"(ne) : "v"(t), "v"(0x00010001u));
                        acc = (acc << 1) | ne;
                    }
                    const uint32_t eq = ~acc;
                    call = (mask_t)(eq & 0xFFFFu) & full;
                    pall = (mask_t)(eq >> 16) & full;
                } else {
                    call = 0;
                    pall = 0;
#pragma unroll
                    for (int k2 = 0; k2 < G; ++k2) {
                        const uint32_t v = xch[gbase + k2];
                        call |= (mask_t)((v & 0xFFFFu) == myprop) << k2;
                        pall |= (mask_t)((v >> 16) == myprop) << k2;
                    }
                }
                wave_lds_sync();  // xch is rewritten next step
                Cm = call & lo_m;
                Pm = pall & lo_m;
                H = (call & later_m) | (mask_t)((myprop + 1u) >> 16);
            }
            CCX_STAMP(0);   // loop top + proposal + conflict masks

            // ---- 3. ballot fixed point over "who moved": rank k moves iff F_k(M) = H | (M & P) | (~M & C) is 0, with M =
            //         the ranks that did move.  Bit k of F depends on bits < k of M only, so the fixed point is unique and
            //         j applications of F to ANY start are exact for every rank whose chain of dependencies is at most
            //         j - 1 links long.  OCC: lane = agent, bits = ranks.  !OCC: lane = rank, bits = ranks.
            uint64_t b, b_prev = 0;
            bool mv_lane;   // (OCC && !has_order: the last compare's own lane mask drives the position update)
            auto group_raw = [&](uint64_t bb) -> mask_t { return GLOG == 6 ? (mask_t)bb : (mask_t)(bb >> gsh); };
            const bool fast_fp = OCC && !has_order;
            if (fast_fp) {
                // lane = rank within the group: M is the group's slice of the ballot (bits above the group are junk that
                // the masks, which only hold bits below my rank, never look at).  Two applications, straight-line.
                const uint64_t b0 = __builtin_amdgcn_ballot_w64((H | Cm) == 0);
                const mask_t M0 = group_raw(b0);
                b_prev = __builtin_amdgcn_ballot_w64((H | (M0 & Pm) | (~M0 & Cm)) == 0);
                const mask_t M1 = group_raw(b_prev);
                mv_lane = (H | (M1 & Pm) | (~M1 & Cm)) == 0;
                b = __builtin_amdgcn_ballot_w64(mv_lane);
            } else {
                b = __builtin_amdgcn_ballot_w64((H | Cm) == 0);
                mv_lane = false;
            }
            if constexpr (OCC) {   // leave the table clean for the next step (queued behind the read; fills the wait for the last ballot)
                lds_mask_st(ca, 0);
                lds_mask_st(qa, 0);
            }
            if (fast_fp) {
                if (((b ^ b_prev) | lag_b) != 0) {   // ONE scalar test for the two rare events of this half of the step
                    if (lag_b != 0) {                // the writer waves are a whole ring behind: wait for them
                        wprog = sync_ld(prog_addr);
#ifdef CCX_DIAG_WAITS
                        if (__builtin_amdgcn_ballot_w64((int)wprog < s - (int)stage_mask) != 0) ++diag_lag_steps;
#endif
                        while (__builtin_amdgcn_ballot_w64((int)wprog < s - (int)stage_mask) != 0) {
                            __builtin_amdgcn_s_sleep(1);
                            wprog = sync_ld(prog_addr);
#ifdef CCX_DIAG_WAITS
                            ++diag_lag_spins;
#endif
                        }
                    }
                    if (b != b_prev) {   // a chain of three or more agents somewhere in the wave: iterate
                        for (int it = 3; it <= N; ++it) {
                            const mask_t M = group_raw(b);
                            mv_lane = (H | (M & Pm) | (~M & Cm)) == 0;
                            const uint64_t b2 = __builtin_amdgcn_ballot_w64(mv_lane);
                            if (b2 == b) break;
                            b = b2;
                        }
                    }
                }
            } else {
                if (lag_b != 0) {
                    wprog = sync_ld(prog_addr);
                    while (__builtin_amdgcn_ballot_w64((int)wprog < s - (int)stage_mask) != 0) {
                        __builtin_amdgcn_s_sleep(1);
                        wprog = sync_ld(prog_addr);
                    }
                }
                const mask_t dep = H ? mask_t(0) : (Cm | Pm);
                if (__builtin_amdgcn_ballot_w64(dep != 0) != 0) {
                    if (OCC) {
                        // ballots are lane(=agent)-indexed here but the masks are rank-indexed:
                        // resolve through the per-rank view kept in xch (rank -> moved bit)
                        for (int it = 1; it < N; ++it) {
                            xch[gbase + rank] = (uint32_t)((b >> lane) & 1ull);
                            wave_lds_sync();
                            mask_t M = 0;
                            for (int k2 = 0; k2 < N; ++k2) M |= (mask_t)xch[gbase + k2] << k2;
                            wave_lds_sync();
                            const uint64_t b2 = __builtin_amdgcn_ballot_w64((H | (M & Pm) | (~M & Cm)) == 0);
                            if (b2 == b) break;
                            b = b2;
                        }
                    } else {
                        for (int it = 1; it < N; ++it) {
                            const mask_t M = group_bits<GLOG>(b, lane);
                            const uint64_t b2 = __builtin_amdgcn_ballot_w64((H | (M & Pm) | (~M & Cm)) == 0);
                            if (b2 == b) break;
                            b = b2;
                        }
                    }
                }
                // OCC: the ballot bit of my own lane; !OCC: the bit of the lane playing my rank
                mv_lane = OCC ? ((b >> lane) & 1ull) != 0 : ((uint32_t)(group_bits<GLOG>(b, lane) >> rank) & 1u) != 0;
            }
            if (mv_lane) {  // collectivecrossing.py:408
                c8 = np8;
                ilo = (uint32_t)pci;
            }
            // (lanes without an agent never move: act = 0 -> ok = 0 -> H != 0)
            add_mask(c_moves, OCC ? b : __builtin_amdgcn_ballot_w64(mv_lane));
            add_mask(c_live, live_b);
            CCX_STAMP(1);   // ballot fixed point + position update

            // ---- 4. tail: deactivate on arrival (:210-212), terminated (terminateds.py:40-82), the pair of flags this
            //         step raises, __all__ (:256-259).  The per-agent flag byte (live, obs, ...) is assembled by writer
            //         wave 0, which keeps its own copy of the terminated / truncated pair.
            const uint32_t dest = cell_at_dest(ilo, tsh);            // :663-683
            act &= ~dest;
            // terminateds[id] as the cell says (terminateds.py:66-82): the destination-row bit for the built-in strategies -- the plain
            // instantiations read nothing else -- or the bit of a position-only user strategy (ccx_set_terminated_table)
            const uint32_t tind = PLAIN ? dest : cell_terminated(ilo, tsh);
            const uint64_t ndest_b = __builtin_amdgcn_ballot_w64((validbit & ~tind) != 0);   // agents whose terminated value is False
            uint32_t ndest_grp;                                      // != 0: some agent of my env is not there yet
            if constexpr (GLOG == 6) ndest_grp = in_vgpr((uint32_t)ndest_b | (uint32_t)(ndest_b >> 32));
            else ndest_grp = in_vgpr((uint32_t)(ndest_b >> gsh) & (uint32_t)full);
            const uint32_t all_dest = in_vgpr(ndest_grp == 0u ? 1u : 0u);   // terminateds.py:40-60 and :256
            const uint32_t term_out = term_all ? all_dest : tind;
            const uint32_t out2 = term_out | trunc2;                 // :229-241: the flags are set once, and stay
            tt |= out2;
            // every live agent truncates at once, so __all__ = (any live) && step_count >= max_steps  (:257)
            const uint32_t ef = in_vgpr(all_dest | ((live_grp != 0u ? 2u : 0u) & ge_m));
            const bool ef_lane = ef != 0u;
            const uint64_t reset_b = __builtin_amdgcn_ballot_w64(ef_lane) & may_reset_b;

            // ---- 5. hand the step to the writer waves
            if constexpr (OUT) {
                // ONE word per lane: where the agent stands (the LDS address of its cell word: the writer looks the word
                // up itself), the flags this step raises, active, the env byte, the action taken
                const uint32_t efw = env_flag_byte(ef, reset_bit);               // CCX_EF_RESET next to a raised __all__ flag
                const uint32_t hw = (uint32_t)c8 | (out2 << kHwOut2Shift) | (act << kHwActShift) | (efw << kHwEfShift) |
                                    (a_out << kHwActionShift);
                *(__attribute__((address_space(3))) uint32_t*)(uintptr_t)(stage_abs + ((uint32_t)s & stage_mask) * kStageSlotBytes) = hw;
                CCX_STAMP(2);   // tail
                seq_v += 1u;
                if (flags_mode) {
                    wave_lds_sync();
                    sync_st(seq_addr, seq_v);       // (every lane writes the same word)
                } else {
                    lds_barrier();
                }
                CCX_STAMP(3);   // hand-off
            }

            // ---- 6. auto-reset from the pool (reset() :97-150 with host-computed placements)
            if (reset_b != 0) {   // wave-uniform: some env of this tile restarts (once per episode)
                const bool do_reset = ((reset_b >> lane) & 1ull) != 0;
                c_episodes += (uint32_t)__builtin_popcountll(reset_b & slot0_b);
                c_arrivals += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(do_reset && valid && act == 0u));
                if (do_reset) {
                    episode += 1;
                    left1 = max_steps_m1;
                    if (valid) {
                        if (pnext_pending) {   // second reset inside one action burst (rare): wait here
                            asm volatile("; rare: reset twice within one action burst");
                            pcell8 = (int)lds0 + ((int)(pnext >> 8) * Wp + (int)(pnext & 0xFFu) + Wp + 1) * 8;
                        }
                        c8 = pcell8;
                        const unsigned long long rci = lds_cell(c8);
                        ilo = (uint32_t)rci;
                        act = 1;
                        tt = 0;
                        pool_idx += pool_stride;
                        if (pool_idx >= pool_size) pool_idx -= pool_size;
                        pnext = *reinterpret_cast<const uint16_t*>(KA.pool + ((size_t)pool_idx * N + i) * 2);
                        pnext_pending = true;
                    }
                }
            }
        }
    }
    c_arrivals -= (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(act != 0));   // (active at the end)
#ifdef CCX_DIAG_WAITS   // counters[14] += steps on which the sim wave had to wait for a writer, [15] += its spins
    if (KA.counters && lane == 0) {
        atomicAdd(&KA.counters[14], (unsigned long long)diag_lag_steps);
        atomicAdd(&KA.counters[15], (unsigned long long)diag_lag_spins);
    }
#endif
    const int stepc_end = max_steps_m1 - left1;
    const uint32_t term = tt & 1u, trunc = tt >> 1;
    // The write-back pointers are re-read from the kernel-argument segment here (rollout_kernarg_tail, ccx_kernels.hip)
    // instead of living through the step loop: as loop-carried values they cost 16 VGPRs (or as many SGPRs) for nothing.
    
    unsigned long long* const ctr = KA.counters;
    CCX_STAMP_FLUSH(ctr, 0);
    CCX_T(4);

    // ---- pace control (DESIGN.md 3.6): every tile compares its elapsed time with the schedule.
    //   on time (<= 1.5 % over)   tile 0 votes for a pace 0.4 % faster (1.6 % while no collapse has
    //                             been seen: quick descent from the conservative start value)
    //   slightly late (<= 5 %)    the memory side is at its limit: vote for pace + half the overshoot
    //   collapse (> 5 %)          the pace was beyond the cliff: vote +3 % and raise the floor to
    //                             2.5 % above this pace, so that the probing does not walk straight
    //                             back into it (the floor decays slowly at first, see above)
    // The slowest vote wins (atomicMax into the slot the next launch reads); only late tiles and
    // tile 0 touch the words, so a healthy launch costs one store.  (A healthy launch has NO late
    // tile: all of them finish within 1 % of the schedule; a collapse delays whole XCDs, 64+ tiles.)
    // The tiles of a partial last round run on a schedule scaled to their number -- an estimate, and one their own step chain
    // may not be able to follow at all (100 003 envs of C2: 107 workgroups in the last round, a tenth of the pace): their
    // lateness says nothing about the memory side.  Tiles whose schedule was scaled below HALF the common pace do not vote.  (Round 4: they did, and drove the common pace of such
    // batches to 3.5 x its value -- 0.27 of the peak for 100 003 envs, 0.67 for 20 000; profiles/r04_multi_round.txt.)
    // Rounds that the host made EQUAL (run_rollout: a grid just above a whole number of rounds is launched in balanced
    // rounds) are at least half full: their scaled schedule is one their tiles can follow, and they are the only voters there
    // are.  (pace vs pace_base says how far the schedule was scaled: nothing new is kept alive across the step loop for this.)
    if (pace && launch_is_adaptive(p.pace_state != nullptr, p.pace_adapt != 0u, want_obs, K, p.pace_min_k, p.adapt_min_k) &&
        2u * pace >= pace_base) {
        unsigned long long now;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
        const unsigned long long elapsed_fp = (now - pace_t0) << 8, planned_fp = (unsigned long long)K * pace;
        const bool late = elapsed_fp > planned_fp + (planned_fp >> 6);
        const bool collapse = elapsed_fp > planned_fp + planned_fp / 20u;
        if ((late || tile == 0) && lane == 0) {
            uint32_t next;                                   // a vote is for the COMMON (full-round) pace
            if (collapse) {
                next = pace_base + pace_base / 33u;
                atomicMax(&p.pace_state[2], pace_base + pace_base / 40u);
                p.pace_state[3] = 0u;
                p.pace_state[6] = pace_base;                 // (every collapsed tile writes the same value)
            } else if (late) {
                // half the relative overshoot, at least 0.5 %
                unsigned long long over16 = ((elapsed_fp - planned_fp) << 16) / planned_fp;   // overshoot x 2^16
                over16 = over16 > 65536ull ? 65536ull : over16;
                uint32_t inc = (uint32_t)(((unsigned long long)pace_base * over16) >> 17);
                const uint32_t lo = pace_base / 200u;
                next = pace_base + (inc < lo ? lo : inc);
            } else {
                next = pace_base - (pace_base >> (pace_floor ? 8 : 6));   // no collapse seen yet: descend quickly
            }
            next = next < p.pace_min_fp ? p.pace_min_fp : (next > p.pace_max_fp ? p.pace_max_fp : next);
            atomicMax(&p.pace_state[p.pace_slot ^ 1u], next);
        }
    }

#ifdef CCX_TILE_TIMES   // diagnostic (profiles/scratch/tile_times.py): elapsed 10-ns ticks of every tile
    if (pace && ctr && lane == 0) {
        unsigned long long now;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
        ctr[kCounterTotals + (size_t)tile * kCounterSlot + 6] = now - pace_t0;
    }
#endif

    CCX_T(5);
    // ---- registers -> state ------------------------------------------------------------------
    // (the lane predicates are re-derived from values the loop keeps anyway -- the opaque `validbit`, the one-lane-per-env
    // ballot -- instead of lane masks that would have to live through the step loop in SGPRs)
    const bool valid_w = in_vgpr(validbit) != 0u;
    const bool slot0_w = ((slot0_b >> lane) & 1ull) != 0;
    if (valid_w) {
        KA.st.x[idx] = (int)cell_x(ilo);
        KA.st.y[idx] = (int)cell_y(ilo);
        KA.st.active[idx] = (uint8_t)act;
        KA.st.terminated[idx] = (uint8_t)term;
        KA.st.truncated[idx] = (uint8_t)trunc;
    }
    if (slot0_w) {
        KA.st.step_count[env] = stepc_end;
        KA.st.episode[env] = episode;
    }
    if (ctr) {
        const uint32_t nenv = (uint32_t)__builtin_popcountll(slot0_b);
        const uint32_t moves = wave_sum_u32(c_moves), lives = wave_sum_u32(c_live);
        const uint32_t arrivals = c_arrivals, eps = c_episodes;   // (wave totals already)
        // One partial slot per tile: every wave adding to the SAME six words costs ~35 us per
        // launch when all tiles finish together (3072 same-address device-scope atomics serialise
        // at the memory side); distinct lines are free.  reduce_counters_kernel sums the slots.
        if (lane == 0 && nenv) {
            unsigned long long* slot = ctr + kCounterTotals + (size_t)tile * kCounterSlot;
            atomicAdd(&slot[0], (unsigned long long)nenv * (unsigned long long)K);
            atomicAdd(&slot[1], (unsigned long long)nenv * (unsigned long long)K * N);
            atomicAdd(&slot[2], (unsigned long long)lives);
            atomicAdd(&slot[3], (unsigned long long)eps);
            atomicAdd(&slot[4], (unsigned long long)moves);
            atomicAdd(&slot[5], (unsigned long long)arrivals);
        }
    }
    CCX_T(6);
