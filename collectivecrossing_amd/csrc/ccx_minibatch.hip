// ccx_minibatch.hip -- CCX_MINIBATCH (include/ccx.h): shuffled on-policy minibatches out of a rollout's own arrays.  ONE kernel
// draws B positions of the epoch's keyed permutation, gathers the records they name and writes the minibatch ppo_loss takes;
// one plain lane behind it advances {epoch, cursor} on the device, so a captured update walks through minibatches and epochs by
// being replayed.  The permutation, the draw, the state and the EMPTY row are ccx_minibatch.h's; the word is ccx_kernels.h's; the
// lane layout and, for the compact form, the wave's tile and the emission of the rows are ccx_gather.h's; the grid is
// ccx_internal.h's: called, not restated.
//
// minibatch_gather_kernel<DRAW, COMPACT, PAIR>: a record-gather wave (ccx_gather.h) -- lane (g, i) is agent i of record b0 + g.
// Every lane of a group works out the record's index for itself (DRAW: the walk of the six-round network; else the caller's
// index[b]), so no lane waits for another's walk.
//   COMPACT: the lane's float4 of the compact record and its six small fields are loaded THROUGH the index, all in flight before
//   the first wait; the small fields are stored, then the tile is set up and emit_rows writes the rows.
//   rows: the wave's region of obs is EW N L contiguous floats, copied in 16-byte units (8-byte for an odd N: a record is then
//   8 mod 16 bytes long).  Workgroup (x, y) copies units y 64 kUnits .. of wave x's region, kUnits per lane: the index of a
//   unit's record comes from the lane that walked it (one ds_bpermute), and the lane's kUnits row loads and six small loads
//   are all issued before the first wait.  Only y = 0 writes the small arrays and index.  An EMPTY row is made in registers.
// minibatch_state_kernel: one lane advances the state BEHIND the launch that read it (replay_head_kernel's pattern).
// minibatch_perm_kernel: pi_c(0 .. M - 1) of a given epoch, a lane per position.
#include "ccx_internal.h"
#include "ccx_gather.h"
#include "ccx_minibatch.h"

using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

static_assert(ccx_minibatch::kStream == ccx::kMinibatchStream, "one constant for the minibatch stream");
static_assert(ccx_minibatch::kEmptyAction == CCX_ACTION_ABSENT, "the empty row's action is the absent one");
static_assert(ccx_minibatch::kValidLive == CCX_AF_LIVE, "valid without a source is GaeResult.valid's live byte");

constexpr int kUnits = 8;                  // rows form: vector units a lane copies (all of them loaded before the first wait)

struct MbSource {                          // the rollout's arrays, [K][E][N] (obs_steps [K][E][N][L] or [K][E][N][4])
    const float* obs0;                     // [E][N][L] / [E][N][4] or null
    const float* obs_steps;                // or null (then no obs output)
    const uint8_t* actions;
    const float* logp;
    const float* advantages;
    const float* returns;
    const uint8_t* masks;                  // or null: 0x1F
    const uint8_t* valid;                  // or null: AF_LIVE
};

struct MbOut {                             // the minibatch, [B][N]
    float* obs;                            // [B][N][L] or null
    uint8_t* actions;
    float* logp;
    float* advantages;
    float* returns;
    uint8_t* masks;
    uint8_t* valid;
    long long* index;                      // [B]
};

struct MbArgs {
    MbSource s;
    MbOut o;
    const long long* index_in;             // [B]: read where !DRAW
    const long long* state;                // {epoch, cursor, 0, 0}: read where DRAW
    long long B, M;
    int E, glog;
    ccx_minibatch::Split sp;
    uint32_t seed_lo, seed_hi;
};

__device__ __forceinline__ uint32_t permuted(uint32_t p, uint32_t M, ccx_minibatch::Split sp, unsigned long long epoch,
                                             uint32_t seed_lo, uint32_t seed_hi) {
    return ccx_minibatch::permute(p, M, sp, epoch, [=](uint32_t right, uint32_t c_lo, uint32_t c_hi, uint32_t r) {
        return ccx::random_word(seed_lo, seed_hi ^ ccx::kMinibatchStream, right, c_lo, c_hi, r);
    }).x;
}

// 8-byte unit t of the rows of the EMPTY record
__device__ __forceinline__ float2 empty_unit(uint32_t t, const ccx::KParams& p) {
    const int kind = ccx_minibatch::empty_unit_kind(t, (uint32_t)p.N);
    if (kind == 1) return make_float2((float)p.dc, (float)p.div);
    if (kind == 2) return make_float2((float)p.dl, (float)p.dr);
    return kind == 3 ? make_float2(-1.0f, -1.0f) : make_float2(0.0f, 0.0f);
}

template <bool DRAW, bool COMPACT, bool PAIR>
__global__ __launch_bounds__(256) void minibatch_gather_kernel(const ccx::KParams p, const MbArgs A) {
    using namespace ccx;
    extern __shared__ __align__(16) unsigned char smem[];
    const ccx_gather::Lane l = ccx_gather::lane_of(p, A.glog, A.B);
    const int lane = l.lane, i = l.i, N = l.N, L = 6 + 4 * N;
    const long long b = l.b;
    const bool mine = l.mine;
    const bool small = mine && blockIdx.y == 0u;                         // (rows form: the other y only copy rows)
    // the record: every lane of a group works it out for itself
    long long idx = -1;
    if (mine) {
        if constexpr (DRAW) {
            const long long epoch = A.state[0], cursor = A.state[1];
            if (ccx_minibatch::drawn(cursor, b, A.M))
                idx = (long long)permuted((uint32_t)(cursor + b), (uint32_t)A.M, A.sp, (unsigned long long)epoch, A.seed_lo, A.seed_hi);
        } else {
            idx = A.index_in[b];
        }
    }
    const bool read = mine && ccx_minibatch::in_rollout(idx, A.M);
    const bool has0 = A.s.obs0 != nullptr;
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint8_t act = ccx_minibatch::kEmptyAction, mk = ccx_minibatch::kEmptyMasks, vl = ccx_minibatch::kEmptyValid;
    float lp = 0.0f, ad = 0.0f, rt = 0.0f;
    if (read && (COMPACT || small)) {                                    // (every load is issued before the first wait)
        const long long at = idx * N + i;
        if constexpr (COMPACT) {
            if (A.o.obs) {
                const ccx_minibatch::RowAt r = ccx_minibatch::row_of(idx, A.E, has0);
                me = reinterpret_cast<const float4*>(r.first ? A.s.obs0 : A.s.obs_steps)[r.at * N + i];
            }
        }
        act = A.s.actions[at];
        lp = A.s.logp[at];
        ad = A.s.advantages[at];
        rt = A.s.returns[at];
        mk = A.s.masks ? A.s.masks[at] : ccx_minibatch::kMasksAll;
        vl = A.s.valid ? A.s.valid[at] : ccx_minibatch::kValidLive;
    }
    const uint32_t here = (uint32_t)ccx_gather::records_here(p, l, A.B);
    const size_t region = ccx_gather::rows_before(l);                    // (both worked out here, ahead of the branch: see DESIGN.md 3.27)
    if constexpr (!COMPACT) {
        if (A.o.obs) {
            using V = std::conditional_t<PAIR, float4, float2>;
            const uint32_t U = ((uint32_t)N * (3u + 2u * (uint32_t)N)) >> (PAIR ? 1 : 0);   // vector units of one record's rows
            const uint32_t units = here * U;
            const uint32_t q0 = blockIdx.y * (64u * kUnits) + (uint32_t)lane;
            const int from = read ? (int)idx : -1;                       // (in [0, M): 31 bits)
            V v[kUnits];
#pragma unroll
            for (int k = 0; k < kUnits; ++k) {
                const uint32_t q = q0 + 64u * (uint32_t)k;
                const bool ok = q < units;
                const uint32_t rec = ok ? q / U : 0u, u = q - rec * U;
                const int j = __shfl(from, (int)(rec << A.glog), 64);     // lane (rec, 0) walked record b0 + rec
                if (ok && j >= 0) {
                    const ccx_minibatch::RowAt r = ccx_minibatch::row_of(j, A.E, has0);
                    const float* src = (r.first ? A.s.obs0 : A.s.obs_steps) + (size_t)r.at * (size_t)N * (size_t)L;
                    v[k] = reinterpret_cast<const V*>(src)[u];
                } else if constexpr (PAIR) {
                    const float2 lo = empty_unit(2u * u, p), hi = empty_unit(2u * u + 1u, p);
                    v[k] = make_float4(lo.x, lo.y, hi.x, hi.y);
                } else {
                    v[k] = empty_unit(u, p);
                }
            }
            V* dst = reinterpret_cast<V*>(A.o.obs + region);
#pragma unroll
            for (int k = 0; k < kUnits; ++k) {
                const uint32_t q = q0 + 64u * (uint32_t)k;
                if (q < units) {
                    if constexpr (PAIR) {
                        const v4f w = {v[k].x, v[k].y, v[k].z, v[k].w};
                        store_obs(w, reinterpret_cast<v4f*>(dst + q));
                    } else {
                        store_obs(v[k], dst + q);
                    }
                }
            }
        }
    }
    if (small) {
        const long long to = b * N + i;
        A.o.actions[to] = act;
        A.o.logp[to] = lp;
        A.o.advantages[to] = ad;
        A.o.returns[to] = rt;
        A.o.masks[to] = mk;
        A.o.valid[to] = vl;
        if (i == 0) A.o.index[b] = idx;
    }
    if constexpr (COMPACT) {                                             // (the tile is set up behind the small stores)
        if (A.o.obs) ccx_gather::emit_rows<PAIR>(ccx_gather::tile_of(smem, p, l), p, l, A.B, A.o.obs, nullptr, me, me);
    }
}

__global__ __launch_bounds__(64) void minibatch_state_kernel(long long* state, const long long B, const long long M) {
    if (threadIdx.x == 0u && blockIdx.x == 0u) {
        const ccx_minibatch::State s = ccx_minibatch::advance(ccx_minibatch::State{state[0], state[1]}, B, M);
        state[0] = s.epoch;
        state[1] = s.cursor;
    }
}

__global__ __launch_bounds__(256) void minibatch_perm_kernel(long long* out, const uint32_t M, const ccx_minibatch::Split sp,
                                                             const unsigned long long epoch, const uint32_t seed_lo,
                                                             const uint32_t seed_hi) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;                   // M < 2^31
    if (t < M) out[t] = (long long)permuted(t, M, sp, epoch, seed_lo, seed_hi);
}

int gather(const char* who, ccx_handle* h, int64_t K, int32_t compact, const MbSource& src, int64_t* state, int64_t B,
           const int64_t* index_in, const MbOut& out, bool draw) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!src.actions || !src.logp || !src.advantages || !src.returns)
        return fail(CCX_EINVAL, "%s: NULL source (only obs0, obs_steps, masks and valid may be NULL)", who);
    if (!out.actions || !out.logp || !out.advantages || !out.returns || !out.masks || !out.valid || !out.index)
        return fail(CCX_EINVAL, "%s: NULL output (only obs may be NULL)", who);
    if (draw ? !state : !index_in) return fail(CCX_EINVAL, "%s: NULL %s", who, draw ? "state" : "index");
    if (K < 1 || K > ccx_minibatch::kMaxRecords / (int64_t)h->E)
        return fail(CCX_EINVAL, "%s: K = %lld out of range (1 <= K * E < 2^31)", who, (long long)K);
    if (int rc = ccxi::check_batch_size(who, h, B)) return rc;
    if (out.obs && !src.obs_steps) return fail(CCX_EINVAL, "%s: an obs output needs obs_steps", who);
    const bool pair = (h->N % 2) == 0;
    if (misaligned(16, compact ? src.obs0 : nullptr, compact ? src.obs_steps : nullptr))
        return fail(CCX_EINVAL, "%s: compact observation arrays must be 16-byte aligned", who);
    if (misaligned(pair ? 16 : 8, out.obs, compact ? nullptr : src.obs0, compact ? nullptr : src.obs_steps))
        return fail(CCX_EINVAL, "%s: observation rows must be 16-byte aligned (8-byte for an odd number of agents)", who);
    if (misaligned(8, state, index_in, out.index)) return fail(CCX_EINVAL, "%s: state and index must be 8-byte aligned", who);
    if (misaligned(4, src.logp, src.advantages, src.returns, out.logp, out.advantages, out.returns))
        return fail(CCX_EINVAL, "%s: logp, advantages and returns must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const ccx::LaunchShape& ls = h->shape;
    const ccx::KParams& p = h->kp;
    dim3 grid, block;
    if (int rc = ccxi::gather_grid(who, h, B, grid, block)) return rc;
    MbArgs A{};
    A.s = src;
    A.o = out;
    A.index_in = reinterpret_cast<const long long*>(index_in);
    A.state = reinterpret_cast<const long long*>(state);
    A.B = B;
    A.M = K * (int64_t)h->E;
    A.E = h->E;
    A.glog = ls.glog;
    A.sp = ccx_minibatch::split_of((uint32_t)A.M);
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi;
    const bool rows = !compact && out.obs;
    const unsigned units_per_wave = ((unsigned)p.EW * (unsigned)h->N * (3u + 2u * (unsigned)h->N)) >> (pair ? 1 : 0);
    const unsigned chunks = rows ? (units_per_wave + 64u * kUnits - 1u) / (64u * kUnits) : 1u;      // at most 17 (64 lanes x 131 units)
    grid.y = chunks;
    with_flags([&](auto drw, auto cmp, auto pr) {
        hipLaunchKernelGGL((minibatch_gather_kernel<decltype(drw)::value, decltype(cmp)::value, decltype(pr)::value>), grid, block,
                           decltype(cmp)::value ? ls.lds_bytes_observe : 0, h->stream, p, A);
    }, draw, compact != 0, pair);
    if (draw)
        hipLaunchKernelGGL(minibatch_state_kernel, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<long long*>(state), (long long)B, (long long)A.M);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // namespace

// the sources and the outputs as the ABI passes them, in the order of MbSource / MbOut
#define CCX_MB_SOURCE_PARAMS const float* obs0_or_null, const float* obs_steps_or_null, const uint8_t* actions, const float* logp, \
                             const float* advantages, const float* returns, const uint8_t* masks_or_null, const uint8_t* valid_or_null
#define CCX_MB_SOURCE_ARGS obs0_or_null, obs_steps_or_null, actions, logp, advantages, returns, masks_or_null, valid_or_null
#define CCX_MB_OUT_PARAMS float* out_obs_or_null, uint8_t* out_actions, float* out_logp, float* out_advantages, float* out_returns, \
                          uint8_t* out_masks, uint8_t* out_valid, int64_t* out_index
#define CCX_MB_OUT_ARGS out_obs_or_null, out_actions, out_logp, out_advantages, out_returns, out_masks, out_valid, \
                        reinterpret_cast<long long*>(out_index)

extern "C" {

int ccx_minibatch_next(ccx_handle* h, int64_t K, int32_t compact, CCX_MB_SOURCE_PARAMS, int64_t* state, int64_t batch, CCX_MB_OUT_PARAMS) {
    return gather("ccx_minibatch_next", h, K, compact, MbSource{CCX_MB_SOURCE_ARGS}, state, batch, nullptr, MbOut{CCX_MB_OUT_ARGS}, true);
}

int ccx_minibatch_fetch(ccx_handle* h, int64_t K, int32_t compact, CCX_MB_SOURCE_PARAMS, int64_t batch, const int64_t* index_in,
                        CCX_MB_OUT_PARAMS) {
    return gather("ccx_minibatch_fetch", h, K, compact, MbSource{CCX_MB_SOURCE_ARGS}, nullptr, batch, index_in, MbOut{CCX_MB_OUT_ARGS}, false);
}

int ccx_minibatch_permutation(ccx_handle* h, int64_t M, int64_t epoch, int64_t* out) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!out) return fail(CCX_EINVAL, "ccx_minibatch_permutation: NULL out");
    if (M < 1 || M > ccx_minibatch::kMaxRecords)
        return fail(CCX_EINVAL, "ccx_minibatch_permutation: M = %lld out of range (1 <= M < 2^31)", (long long)M);
    if (misaligned(8, out)) return fail(CCX_EINVAL, "ccx_minibatch_permutation: out must be 8-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(minibatch_perm_kernel, dim3(ccxi::blocks_of(M)), dim3(256), 0, h->stream, reinterpret_cast<long long*>(out), (uint32_t)M,
                       ccx_minibatch::split_of((uint32_t)M), (unsigned long long)epoch, h->rng_lo, h->rng_hi);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
