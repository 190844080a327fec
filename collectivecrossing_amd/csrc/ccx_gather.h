// ccx_gather.h -- what the kernels that gather a minibatch of RECORDS share on the device (replay_fetch_kernel, nstep_fetch_kernel,
// minibatch_gather_kernel): the lane layout, the wave's tile, the ring's draw and the emission of the rows.  The layout is
// observe_kernel's with records in the place of envs and the lane-group size a launch argument: a wave takes the EW records
// b0 .. b0 + EW - 1 of the minibatch, lane (g, i) agent i of record b0 + g, and the rows of those records are ONE contiguous
// region of an output, written by ccx_rollout_dev.h's emit_obs out of the wave's tile.  The per-row rules are not here
// (ccx_replay.h, ccx_nstep.h, ccx_minibatch.h); the host side of these launches is ccx_internal.h's.
#pragma once
#include "ccx_replay.h"
#include "ccx_rollout_dev.h"

namespace ccx_gather {

// the lane of a record-gather wave over a minibatch of B records
struct Lane {
    int lane, wib;                     // lane of the wave, wave of the workgroup
    int g, i;                          // record of the wave, agent of the record
    int N;                             // agents of a record (read once: every piece below works on this value)
    long long b0, b;                   // the wave's first record, the lane's
    bool mine;                         // the lane carries an agent of such a record
};

__device__ __forceinline__ Lane lane_of(const ccx::KParams& p, int glog, long long B) {
    Lane l;
    l.lane = threadIdx.x & 63;
    l.wib = threadIdx.x >> 6;
    const long long wave = (long long)blockIdx.x * p.waves_per_block + l.wib;
    l.g = l.lane >> glog;
    l.i = l.lane & ((1 << glog) - 1);
    l.b0 = wave * p.EW;
    l.b = l.b0 + l.g;
    l.N = p.N;
    l.mine = (l.g < p.EW) && (l.b < B) && (l.i < l.N);
    return l;
}

// records of the wave that lie inside the minibatch, 0 .. EW
__device__ __forceinline__ long long records_here(const ccx::KParams& p, const Lane& l, long long B) {
    const long long here = B - l.b0;
    return here < 0 ? 0 : (here > p.EW ? p.EW : here);
}

// floats in front of the wave's rows in an output [B][N][L]
__device__ __forceinline__ size_t rows_before(const Lane& l) {
    const int L = 6 + 4 * l.N;
    return (size_t)l.b0 * (size_t)l.N * (size_t)L;
}

// the wave's tile and the workgroup's address table, carved out of the launch's LDS: the table is copied in and the tile's
// constants are set; both are in LDS after the next __syncthreads()
struct Tile {
    ccx::WaveLds* wl;
    uint16_t* table;
};

__device__ __forceinline__ Tile tile_of(unsigned char* smem, const ccx::KParams& p, const Lane& l) {
    const Tile t{reinterpret_cast<ccx::WaveLds*>(smem) + l.wib, reinterpret_cast<uint16_t*>(smem + sizeof(ccx::WaveLds) * p.waves_per_block)};
    ccx::build_obs_table<0>(t.table, p);
    ccx::init_wave_consts(t.wl, p, l.lane);
    return t;
}

// the record draw b of launch `draws` picks out of a ring of S steps of E envs whose cursor stands at `head`: the two words of
// key (b, draws) on the replay stream and the 128-bit product with the records filled; -1 in an empty ring
__device__ __forceinline__ long long ring_draw(long long b, long long head, long long draws, int S, int E, uint32_t seed_lo,
                                               uint32_t seed_hi) {
    const unsigned long long F = ccx_replay::filled(head, S, E);
    const ccx_replay::Key k = ccx_replay::key_of((unsigned long long)b, (unsigned long long)draws);
    const uint32_t w0 = ccx::random_word(seed_lo, seed_hi ^ ccx::kReplayStream, k.genv, k.episode, k.step, 0u);
    const uint32_t w1 = ccx::random_word(seed_lo, seed_hi ^ ccx::kReplayStream, k.genv, k.episode, k.step, 1u);
    return ccx_replay::index_of(w0, w1, F);
}

// The rows of the wave's records, out of the lane's compact float4s: `me` becomes the lane's row of `obs`, `nx` that of
// `next_obs`; either output may be null.  The tile takes `me`, the rows leave it through emit_obs -- 16-byte stores for PAIR (an
// even agent count), 8-byte ones else --, and the same tile then serves `nx`: a wave's LDS traffic runs in program order, so
// the hand-over needs no workgroup barrier.  Holds the launch's one __syncthreads(): every lane of the workgroup calls it.
template <bool PAIR>
__device__ __forceinline__ void emit_rows(const Tile& t, const ccx::KParams& p, const Lane& l, long long B, float* obs,
                                          float* next_obs, float4 me, float4 nx) {
    const int N = l.N;
    const int units = (int)records_here(p, l, B) * N * (3 + 2 * N);
    const int n = PAIR ? (units >> 1) : units;
    const size_t region = rows_before(l);
    if (obs) t.wl->slot[l.lane] = me;                                    // (two stores, not a select between two structs)
    else t.wl->slot[l.lane] = nx;
    __syncthreads();                                                     // the table and the tile are in LDS
    if (obs) {
        ccx::emit_obs<PAIR>(t.wl, t.table, reinterpret_cast<char*>(obs + region), 0, n, l.lane);
        if (next_obs) {
            ccx::wave_lds_sync();                                        // the tile has been read before it is rewritten
            t.wl->slot[l.lane] = nx;
            ccx::wave_lds_sync();
        }
    }
    if (next_obs) ccx::emit_obs<PAIR>(t.wl, t.table, reinterpret_cast<char*>(next_obs + region), 0, n, l.lane);
}

}  // namespace ccx_gather
