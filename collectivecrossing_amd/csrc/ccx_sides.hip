// ccx_sides.hip -- CCX_SIDES (include/ccx.h), forward and fused draw: up to eight heads, each owning a set of agent slots, run
// over the [M][N][L] rows a rollout wrote, in ONE launch and without a gathered copy.  (The backward of one group is
// ccx_sides_backward in ccx_mlp_backward.hip, beside the kernels it shares its final step with.)
//
// The map is ccx_sides.h: the grid is the sum of the groups' ceil(M S / 64) tiles; workgroup w finds its group by a scan of
// the table's prefix counts (w is uniform: scalar work) and carries 64 SELECTED rows of that one group, so the four weight
// pointers are uniform over the workgroup and reach ccx_mlp_tile.h's mlp_tile as they do in ccx_mlp.hip: scalar loads.  The
// tile itself -- waves, chains, layer-2 order -- is mlp_tile, unchanged; PickedRows below is its `Rows`:
//   rows    lane l of every wave computes the flat row m N + a of the tile's l-th selected row (a surplus lane of a tail tile
//           repeats the last one); wave 0 leaves the 64 of them in LDS behind the tile, for the loader and for the y stores.
//   loader  work item p = (row r, piece q) over all threads: with L even a row starts at a multiple of 8 bytes (x is 16-byte
//           aligned and a row is 4 L bytes), so a piece is an 8-byte load -- always the case for observation rows, L = 6 + 4 N;
//           an odd L takes dwords.  Adjacent items are adjacent pieces of one row and adjacent slots are adjacent rows, so a
//           contiguous slot range (a side) reads S L contiguous floats per env-row, every byte once.
//   stores  hidden: the lane's own row; y: item i = r O + o of the tile goes to y[row_r O + o].
// Rows of slots that no group owns are never addressed.  The table travels BY VALUE in the kernel arguments (ccx_adam.hip's
// way): a call needs no host-to-device copy, so it captures.
// The fused draw is ccx_draw.h's small_loads / finish with the Slot taken from the map (slot = m N + a, e = m, a): the same
// code ccx_sample.hip and ccx_mlp.hip run.  Slots that no group owns form one head-less group behind the others; its tiles
// run no layer and store 255 / +0.0 / +0.0.
// The fused Q choice (ccx_sides_q_actions, CCX_DUELING) is the same kernel with ccx_qact.h's from_tile behind the tile.
#include "ccx_draw.h"
#include "ccx_mlp_tile.h"
#include "ccx_qact.h"
#include "ccx_sides.h"

using ccx_draw::DrawArgs;
using ccx_tile::MlpArgs;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

static_assert(sizeof(ccx_sides::Group) == sizeof(ccx_slot_group) && sizeof(ccx_slot_group) == 40, "the table row is 40 bytes");
static_assert(ccx_sides::kMaxGroups == CCX_SIDES_MAX_GROUPS, "one limit");

namespace {

struct SidesArgs {
    ccx_sides::Table tab;
    const float* x;                    // [M][N][L]
    float* y;                          // [M][N][O]; may be null in the fused kernel
    float* hidden;                     // [M][N][H] or null
    long long M;
    int32_t N, L, H, O, activation;
};

// mlp_tile's Rows for 64 selected rows of one group
struct PickedRows {
    int nr;                            // rows of the tile that exist
    long long mine;                    // the flat row of this lane's selected row
    long long* flat;                   // LDS: the flat rows of the tile's 64 selected rows
    __device__ __forceinline__ void begin(const MlpArgs&) const {}
    __device__ __forceinline__ void load_x(const MlpArgs& A, float* lds, uint32_t tid, int T) const {
        if (tid < 64u) flat[tid] = mine;
        __syncthreads();
        const int L = A.L, Lp = L | 1;
        if ((L & 1) == 0) {
            const int L2 = L >> 1;
            for (int p = (int)tid; p < nr * L2; p += T) {
                const uint32_t r = (uint32_t)p / (uint32_t)L2, q = (uint32_t)p - r * (uint32_t)L2;
                const float2 v = reinterpret_cast<const float2*>(A.x + flat[r] * L)[q];
                lds[r * (uint32_t)Lp + 2u * q] = v.x;
                lds[r * (uint32_t)Lp + 2u * q + 1u] = v.y;
            }
        } else {
            for (int p = (int)tid; p < nr * L; p += T) {
                const uint32_t r = (uint32_t)p / (uint32_t)L, k = (uint32_t)p - r * (uint32_t)L;
                lds[r * (uint32_t)Lp + k] = A.x[flat[r] * L + k];
            }
        }
    }
    __device__ __forceinline__ long long row(uint32_t) const { return mine; }
    __device__ __forceinline__ long long y_index(const MlpArgs& A, int i, int o) const { return flat[(i - o) / A.O] * A.O + o; }
};

// What workgroup blockIdx.x carries: its group's row of the table, the tile's row count and this lane's selected row.
struct Tile {
    ccx_sides::Group grp;
    ccx_sides::Row rw;
    int nr;
};
__device__ __forceinline__ Tile tile_of(const SidesArgs& S, uint32_t lane) {
    int g;
    uint32_t tile;
    ccx_sides::locate(S.tab.first, S.tab.num, blockIdx.x, g, tile);
    Tile t;
    t.grp = S.tab.g[g];
    const int sc = ccx_sides::popcount(t.grp.slots);
    t.nr = ccx_sides::tile_rows(S.M, sc, (long long)tile, ccx_sides::kTileRows);
    const ccx_sides::Start st = ccx_sides::start_of((long long)tile * ccx_sides::kTileRows, sc);
    t.rw = ccx_sides::row_of(t.grp.slots, sc, S.N, st, (int)lane < t.nr ? lane : (uint32_t)(t.nr - 1));
    return t;
}

__device__ __forceinline__ MlpArgs head_of(const SidesArgs& S, const ccx_sides::Group& g) {
    return MlpArgs{S.x, g.w1t, g.b1, g.w2, g.b2, S.y, S.hidden, S.M * S.N, S.L, S.H, S.O, S.activation};
}

// the flat rows of the tile sit behind mlp_tile's LDS: lds_floats(...) floats, a multiple of 64
__device__ __forceinline__ long long* flat_rows(float* lds, const SidesArgs& S, bool draw) {
    const int tile = 64 * (S.L | 1), sums = (S.H / ccx_mlp::kGroup + (draw ? 1 : 0)) * 64 * S.O;
    return reinterpret_cast<long long*>(lds + (tile > sums ? tile : sums));
}

__global__ __launch_bounds__(1024) void sides_forward_kernel(const SidesArgs S) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Tile t = tile_of(S, threadIdx.x & 63u);
    ccx_tile::mlp_tile<false>(head_of(S, t.grp), PickedRows{t.nr, t.rw.row, flat_rows(lds, S, false)}, lds);
}

template <bool DET, bool STATS>
__global__ __launch_bounds__(1024) void sides_draw_kernel(const SidesArgs S, const DrawArgs D) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const Tile t = tile_of(S, lane);
    const bool live = first && (int)lane < t.nr;
    if (t.grp.w1t == nullptr) {                                           // (uniform) slots that no group owns
        if (live) {
            D.actions[t.rw.row] = (uint8_t)CCX_ACTION_ABSENT;
            if (STATS) {
                if (D.logp) D.logp[t.rw.row] = 0.0f;
                if (D.entropy) D.entropy[t.rw.row] = 0.0f;
            }
        }
        return;
    }
    const ccx_draw::Slot s{t.rw.row, t.rw.m, t.rw.a};
    ccx_draw::Small v;
    if (first) v = ccx_draw::small_loads<DET>(D, s, D.masks != nullptr);   // wave 0's small loads, in flight under the layers
    const float* y = ccx_tile::mlp_tile<true>(head_of(S, t.grp), PickedRows{t.nr, t.rw.row, flat_rows(lds, S, true)}, lds);
    __syncthreads();
    if (!live) return;
    float l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = y[5 * lane + k];
    ccx_draw::finish<DET, STATS>(D, s, v, l);
}

// sides_draw_kernel with ccx_q_actions' choice (ccx_qact.h) in the place of the softmax draw, as obs_q_kernel of ccx_dueling.hip:
// S.O = 5 takes the tile's outputs as the Q-values, S.O = 6 (DUEL) puts them through the dueling combine first; with DUEL S.y
// is null and the COMBINED values go to q from wave 0's lanes.  Slots that no group owns get 255 / 0, no q and no layer.
template <bool EPS, bool DUEL>
__global__ __launch_bounds__(1024) void obs_q_groups_kernel(const SidesArgs S, const DrawArgs D, const float* epsilon, uint8_t* explored, float* q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const Tile t = tile_of(S, lane);
    const bool live = first && (int)lane < t.nr;
    if (t.grp.w1t == nullptr) {                                           // (uniform) slots that no group owns
        if (live) {
            D.actions[t.rw.row] = (uint8_t)CCX_ACTION_ABSENT;
            if (explored) explored[t.rw.row] = (uint8_t)0;
        }
        return;
    }
    const ccx_draw::Slot s{t.rw.row, t.rw.m, t.rw.a};
    ccx_draw::Small v;
    float eps = 0.0f;
    if (first) {                                                          // wave 0's small loads, in flight under the layers
        v = ccx_draw::small_loads<!EPS>(D, s, D.masks != nullptr);
        if (EPS) eps = epsilon[0];
    }
    const float* y = ccx_tile::mlp_tile<true>(head_of(S, t.grp), PickedRows{t.nr, t.rw.row, flat_rows(lds, S, true)}, lds);
    __syncthreads();
    if (!live) return;
    ccx_qact::from_tile<EPS, DUEL>(D, s, v, y, lane, eps, explored, q ? q + s.slot * 5 : nullptr);
}

// The table of a call from the caller's groups: checked, the prefix counts filled.  `rest`: append the head-less group of
// the slots no group owns (the draw).
int make_table(const char* who, int64_t M, int32_t N, int32_t num_groups, const ccx_slot_group* groups, bool rest, ccx_sides::Table& tab) {
    if (N < 1 || N > 64) return fail(CCX_EINVAL, "%s: N = %d, 1..64 agent slots are required", who, N);
    if (M < 1 || M > ((int64_t)1 << 40)) return fail(CCX_EINVAL, "%s: M = %lld, 1..2^40 env-rows are required", who, (long long)M);
    if (num_groups < 1 || num_groups > ccx_sides::kMaxGroups)
        return fail(CCX_EINVAL, "%s: num_groups = %d, 1..%d groups are required", who, num_groups, ccx_sides::kMaxGroups);
    if (!groups) return fail(CCX_EINVAL, "%s: NULL groups", who);
    uint64_t masks[ccx_sides::kMaxGroups];
    for (int k = 0; k < num_groups; ++k) masks[k] = groups[k].slots;
    int which = 0;
    switch (ccx_sides::check_masks(masks, num_groups, N, which)) {
        case 0: break;
        case 2: return fail(CCX_EINVAL, "%s: group %d owns no slot (an empty mask)", who, which);
        case 3: return fail(CCX_EINVAL, "%s: group %d's mask %#llx has a bit at or above N = %d", who, which, (unsigned long long)masks[which], N);
        default: return fail(CCX_EINVAL, "%s: group %d's mask %#llx overlaps an earlier group's", who, which, (unsigned long long)masks[which]);
    }
    tab = ccx_sides::Table{};
    uint64_t owned = 0;
    int n = 0;
    for (; n < num_groups; ++n) {
        const ccx_slot_group& g = groups[n];
        if (!g.w1t || !g.b1 || !g.w2 || !g.b2) return fail(CCX_EINVAL, "%s: group %d has a NULL parameter array", who, n);
        if (misaligned(4, g.w1t, g.b1, g.w2, g.b2))
            return fail(CCX_EINVAL, "%s: group %d's w1t, b1, w2 and b2 must be 4-byte aligned", who, n);
        tab.g[n] = ccx_sides::Group{g.slots, g.w1t, g.b1, g.w2, g.b2};
        owned |= g.slots;
    }
    const uint64_t all = N >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << N) - 1);
    if (rest && (all & ~owned)) tab.g[n++] = ccx_sides::Group{all & ~owned, nullptr, nullptr, nullptr, nullptr};
    tab.num = n;
    if (ccx_sides::set_first(tab, M, ccx_sides::kTileRows) > 0x7FFFFFFFll)
        return fail(CCX_EINVAL, "%s: M = %lld exceeds the grid (2^31 - 1 workgroups of 64 selected rows)", who, (long long)M);
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_sides_forward(ccx_handle* h, int64_t M, int32_t N, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                      int32_t num_groups, const ccx_slot_group* groups, float* y, float* hidden_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !y) return fail(CCX_EINVAL, "ccx_sides_forward: NULL argument (only hidden may be NULL)");
    if (const int rc = ccx_tile::check_dims("ccx_sides_forward", L, H, O, activation)) return rc;
    SidesArgs S{};
    if (const int rc = make_table("ccx_sides_forward", M, N, num_groups, groups, false, S.tab)) return rc;
    if (misaligned(16, x, hidden_or_null)) return fail(CCX_EINVAL, "ccx_sides_forward: x and hidden must be 16-byte aligned");
    if (misaligned(4, y)) return fail(CCX_EINVAL, "ccx_sides_forward: y must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    S.x = x, S.y = y, S.hidden = hidden_or_null, S.M = M, S.N = N, S.L = L, S.H = H, S.O = O, S.activation = activation;
    const size_t bytes = ccx_tile::lds_floats(L, H, O, false) * sizeof(float) + 64 * sizeof(long long);
    CCX_HIP(ccx_tile::allow_lds(sides_forward_kernel, bytes));
    hipLaunchKernelGGL(sides_forward_kernel, dim3(S.tab.first[S.tab.num]), dim3(64 * (H / ccx_mlp::kGroup)), bytes, h->stream, S);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_sides_sample_actions(ccx_handle* h, int32_t H, int32_t activation, const float* obs, int32_t num_groups,
                             const ccx_slot_group* groups, const uint8_t* masks_or_null, int32_t deterministic, uint8_t* actions,
                             float* logp_or_null, float* entropy_or_null, float* logits_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !actions) return fail(CCX_EINVAL, "ccx_sides_sample_actions: NULL argument (obs and actions are required)");
    const int32_t L = ccx_obs_len(h->N);
    if (const int rc = ccx_tile::check_dims("ccx_sides_sample_actions", L, H, 5, activation)) return rc;
    SidesArgs S{};
    if (const int rc = make_table("ccx_sides_sample_actions", h->E, h->N, num_groups, groups, true, S.tab)) return rc;
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "ccx_sides_sample_actions: obs must be 16-byte aligned");
    if (misaligned(4, logp_or_null, entropy_or_null, logits_or_null))
        return fail(CCX_EINVAL, "ccx_sides_sample_actions: logp, entropy and logits must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    S.x = obs, S.y = logits_or_null, S.hidden = nullptr, S.M = h->E, S.N = h->N, S.L = L, S.H = H, S.O = 5, S.activation = activation;
    const DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, logp_or_null, entropy_or_null);
    const size_t bytes = ccx_tile::lds_floats(L, H, 5, true) * sizeof(float) + 64 * sizeof(long long);
    const dim3 grid(S.tab.first[S.tab.num]), block(64 * (H / ccx_mlp::kGroup));
    const int rc = with_flags([&](auto det, auto stats) -> int {
        constexpr bool DET = decltype(det)::value, STATS = decltype(stats)::value;
        CCX_HIP(ccx_tile::allow_lds(sides_draw_kernel<DET, STATS>, bytes));
        hipLaunchKernelGGL((sides_draw_kernel<DET, STATS>), grid, block, bytes, h->stream, S, D);
        return CCX_OK;
    }, deterministic != 0, logp_or_null || entropy_or_null);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_sides_q_actions(ccx_handle* h, int32_t H, int32_t activation, int32_t O, const float* obs, int32_t num_groups,
                        const ccx_slot_group* groups, const uint8_t* masks_or_null, const float* epsilon_or_null, uint8_t* actions,
                        uint8_t* explored_or_null, float* q_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !actions) return fail(CCX_EINVAL, "ccx_sides_q_actions: NULL argument (obs and actions are required)");
    if (O != 5 && O != 6) return fail(CCX_EINVAL, "ccx_sides_q_actions: O = %d, 5 (plain) or 6 (dueling) is required", (int)O);
    const int32_t L = ccx_obs_len(h->N);
    if (const int rc = ccx_tile::check_dims("ccx_sides_q_actions", L, H, O, activation)) return rc;
    SidesArgs S{};
    if (const int rc = make_table("ccx_sides_q_actions", h->E, h->N, num_groups, groups, true, S.tab)) return rc;
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "ccx_sides_q_actions: obs must be 16-byte aligned");
    if (misaligned(4, epsilon_or_null, q_or_null)) return fail(CCX_EINVAL, "ccx_sides_q_actions: epsilon and q must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    S.x = obs, S.y = O == 6 ? nullptr : q_or_null, S.hidden = nullptr, S.M = h->E, S.N = h->N, S.L = L, S.H = H, S.O = O, S.activation = activation;
    const DrawArgs D = ccx_qact::draw_args(h, masks_or_null, actions);
    const size_t bytes = ccx_tile::lds_floats(L, H, O, true) * sizeof(float) + 64 * sizeof(long long);
    const dim3 grid(S.tab.first[S.tab.num]), block(64 * (H / ccx_mlp::kGroup));
    const int rc = with_flags([&](auto eps, auto duel) -> int {
        constexpr bool EPS = decltype(eps)::value, DUEL = decltype(duel)::value;
        CCX_HIP(ccx_tile::allow_lds(obs_q_groups_kernel<EPS, DUEL>, bytes));
        hipLaunchKernelGGL((obs_q_groups_kernel<EPS, DUEL>), grid, block, bytes, h->stream, S, D, epsilon_or_null, explored_or_null, q_or_null);
        return CCX_OK;
    }, epsilon_or_null != nullptr, O == 6);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
