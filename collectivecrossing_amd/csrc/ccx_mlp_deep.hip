// ccx_mlp_deep.hip -- CCX_MLP_DEEP (include/ccx.h): Linear(L, H1) -> act -> Linear(H1, H2) -> act -> Linear(H2, O) as a fixed
// sequence of f32 operations per row -- the forward as a kernel of its own (ccx_mlp_deep_forward), fused with CCX_SAMPLE
// (ccx_mlp_deep_sample_actions) and with ccx_q_actions' choice (ccx_mlp_deep_q_actions), ONE launch each -- and the six
// parameter gradients (ccx_mlp_deep_backward).  The arithmetic is ccx_mlp.h's and ccx_mlp_grad.h's functions through
// ccx_mlp_deep.h, one operation per line (-ffp-contract=off; `/` is the correctly rounded division, asked for on this unit's
// compile line).
//
// deep_tile.  ccx_mlp_tile.h's mapping, one layer longer: a workgroup takes 64 adjacent rows, lane l of every wave owns row
// l, a wave owns 16 consecutive units of the CURRENT layer, and the workgroup has max(H1, H2) / 16 waves: a wave beyond a
// layer's groups idles through that layer and still reaches every barrier.  The x tile sits in LDS at the odd row stride
// L | 1 (ccx_tile::AdjacentRows loads it).  Layer 2 needs h1 of a row from all H1 / 16 waves, so behind a barrier -- every
// wave has read its x -- wave g writes its 16 units to LDS over the dead x tile at the odd row stride H1 | 1 (the 64 lanes of
// a write or a read: 64 rows, 64 different banks), and behind a second barrier every layer-2 wave runs ccx_mlp.h's chain on
// its row's h1 as layer 1 ran it on x.  x at L = 512 is 131 KB and h1 at H1 = 256 66 KB: side by side they would not fit a
// CU's 160 KB, overlaid they do.  The layer-3 partials [H2 / 16][64][O] go over the dead h1 tile, and the tile's 64 O sums
// are spread over all threads in the flat order of y, as in mlp_tile.  Weights and biases have wave-uniform addresses (the
// wave index comes through readfirstlane) and arrive through scalar loads; the arrays are separate `__restrict__` kernel
// arguments for the reason ccx_mlp_wide.hip gives: hidden1 is stored before w2t is read.
//
// deep_grad_blocks_kernel.  Workgroup (b, s) takes block b of 256 consecutive rows and slice s of 256 4 x 4 tiles of ONE of
// the three products: [x | 1]^T ga1, [hidden1 | 1]^T ga2, grad_y^T [hidden2 | 1].  The block is walked in sub-tiles of R
// rows (ccx_deep::sub_rows); a row's LDS image is ccx_deep::row_image.  Per sub-tile a slice loads what its product needs,
// forms ga2 four units at a time (w3 sits in LDS) and -- the first product only -- ga1: w2t passes through LDS in slabs of 32
// whole rows at the odd pitch H2 + 1, and one (row, unit) item per thread walks the gh1 chain over j ascending along its
// unit's row (the lanes of a wave: different units, different banks; the row's ga2 a broadcast).  Then every thread adds the rows IN ORDER onto its 16
// f64 accumulators.  The partial of element e lands at partials[e][b] in ccx_deep::elements_of's order: two stretches in
// ccx_mlp_grad.h's layout, each finished by ccx_mlp_backward.hip's final kernel as it is (ccxi::head_grad_final_launch).
// Three plain launches for any shape and any data; no atomic, no last-block-done counter.
#include "ccx_mlp_tile.h"
#include "ccx_qact.h"
#include "ccx_mlp_deep.h"

using ccx_draw::DrawArgs;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;
namespace dp = ccx_deep;
namespace mg = ccx_mlp_grad;

namespace {

struct DeepDims {
    long long rows;
    int32_t L, H1, H2, O, activation;
};

__device__ __forceinline__ void activate16(int activation, float (&a)[dp::kGroup]) {
    if (activation == ccx_mlp::kRelu) {
#pragma unroll
        for (int j = 0; j < dp::kGroup; ++j) a[j] = ccx_mlp::relu_spec(a[j]);
    } else {
#pragma unroll
        for (int j = 0; j < dp::kGroup; ++j) a[j] = ccx_mlp::tanh_spec(a[j]);
    }
}

__device__ __forceinline__ void store16(float* p, const float (&a)[dp::kGroup]) {
    float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = make_float4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
}

// The tile of workgroup blockIdx.x: rows 64 b .. 64 b + 63 through the three layers; y, hidden1 and hidden2 written where
// given, and with KEEP the tile's y left in LDS at the returned pointer (valid behind the caller's barrier).
template <bool KEEP>
__device__ __forceinline__ float* deep_tile(const DeepDims& S, const float* x, const float* w1t, const float* b1, const float* w2t,
                                            const float* b2, const float* w3, const float* b3, float* y, float* hidden1,
                                            float* hidden2, float* lds) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int g = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int L = S.L, H1 = S.H1, H2 = S.H2, O = S.O, G1 = H1 / dp::kGroup, G2 = H2 / dp::kGroup;
    const int T = 64 * (G1 > G2 ? G1 : G2), Lp = L | 1, H1p = H1 | 1;
    const ccx_tile::MlpArgs A{x, w1t, b1, w3, b3, y, nullptr, S.rows, L, H1, O, S.activation};
    ccx_tile::AdjacentRows R;
    R.begin(A);
    const int nr = R.nr;
    // 1. the x tile
    R.load_x(A, lds, tid, T);
    __syncthreads();
    // 2. layer 1: this wave's 16 units of the lane's row (surplus lanes of the tail tile repeat its last row)
    float a[dp::kGroup];
    if (g < G1) {
        const uint32_t rl = (int)lane < nr ? lane : (uint32_t)(nr - 1);
        const float* xr = lds + rl * (uint32_t)Lp;
        const float* wg = w1t + dp::kGroup * g;
#pragma unroll
        for (int j = 0; j < dp::kGroup; ++j) a[j] = b1[dp::kGroup * g + j];
#pragma unroll 2
        for (int k = 0; k < L; ++k) ccx_mlp::layer1_step(a, xr[k], wg + (long long)k * H1);
        activate16(S.activation, a);
        if (hidden1 && (int)lane < nr) store16(hidden1 + R.row(lane) * H1 + dp::kGroup * g, a);
    }
    __syncthreads();                                                      // every wave has read its x: the tile may go
    // 3. h1 of the 64 rows over the dead x tile, row `lane` at lane * (H1 | 1)
    float* hr = lds + lane * (uint32_t)H1p;
    if (g < G1) {
#pragma unroll
        for (int j = 0; j < dp::kGroup; ++j) hr[dp::kGroup * g + j] = a[j];
    }
    __syncthreads();
    // 4. layer 2: CCX_MLP's layer-1 chain with h1 in the place of x
    if (g < G2) {
        const float* wg = w2t + dp::kGroup * g;
#pragma unroll
        for (int j = 0; j < dp::kGroup; ++j) a[j] = b2[dp::kGroup * g + j];
#pragma unroll 2
        for (int k = 0; k < H1; ++k) ccx_mlp::layer1_step(a, hr[k], wg + (long long)k * H2);
        activate16(S.activation, a);
        if (hidden2 && (int)lane < nr) store16(hidden2 + R.row(lane) * H2 + dp::kGroup * g, a);
    }
    __syncthreads();                                                      // every wave has read its h1
    // 5. layer 3: the partials of this wave's group, [G2][64][O] in LDS
    const int per = 64 * O;
    if (g < G2) {
        for (int o = 0; o < O; ++o) lds[g * per + (int)lane * O + o] = ccx_mlp::layer2_partial(a, w3 + o * H2 + dp::kGroup * g);
    }
    __syncthreads();
    // 6. the tile's 64 O sums in the flat order of y, over all threads
    float* ykeep = lds + G2 * per;
    const int valid = nr * O;
    for (int i = (int)tid; i < per; i += T) {
        const int o = i % O;
        const float v = ccx_mlp::layer2_sum(b3[o], lds + i, G2, per);
        if (y && i < valid) y[R.y_index(A, i, o)] = v;
        if (KEEP) ykeep[i] = v;
    }
    return ykeep;
}

#define DEEP_ARRAYS                                                                                                              \
    const float *__restrict__ x, const float *__restrict__ w1t, const float *__restrict__ b1, const float *__restrict__ w2t,   \
        const float *__restrict__ b2, const float *__restrict__ w3, const float *__restrict__ b3

__global__ __launch_bounds__(1024) void deep_forward_kernel(const DeepDims S, DEEP_ARRAYS, float* __restrict__ y,
                                                            float* __restrict__ hidden1, float* __restrict__ hidden2) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    deep_tile<false>(S, x, w1t, b1, w2t, b2, w3, b3, y, hidden1, hidden2, lds);
}

// ccx_mlp.hip's fused draw kernel over deep_tile: 64 rows = 64 slots = wave 0's lanes, under ccx_draw.h's slot rule
template <bool DET, bool STATS>
__global__ __launch_bounds__(1024) void deep_draw_kernel(const DeepDims S, DEEP_ARRAYS, float* __restrict__ logits, const DrawArgs D) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    ccx_draw::Small v;
    if (first) v = ccx_draw::small_loads<DET>(D, s, D.masks != nullptr);   // wave 0's small loads, in flight under the layers
    const float* y = deep_tile<true>(S, x, w1t, b1, w2t, b2, w3, b3, logits, nullptr, nullptr, lds);
    __syncthreads();
    if (!first || s.slot >= D.EN) return;
    float l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = y[5 * lane + k];
    ccx_draw::finish<DET, STATS>(D, s, v, l);
}

// ccx_dueling.hip's fused Q kernel over deep_tile: ccx_qact.h's from_tile behind the tile.  With DUEL the tile stores no y
// (the pointer is null): the COMBINED values go to q from wave 0's lanes.
template <bool EPS, bool DUEL>
__global__ __launch_bounds__(1024) void deep_q_kernel(const DeepDims S, DEEP_ARRAYS, float* __restrict__ ytile, const DrawArgs D,
                                                      const float* epsilon, uint8_t* explored, float* q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const bool first = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    ccx_draw::Small v;
    float eps = 0.0f;
    if (first) {
        v = ccx_draw::small_loads<!EPS>(D, s, D.masks != nullptr);
        if (EPS) eps = epsilon[0];
    }
    const float* y = deep_tile<true>(S, x, w1t, b1, w2t, b2, w3, b3, ytile, nullptr, nullptr, lds);
    __syncthreads();
    if (!first || s.slot >= D.EN) return;
    ccx_qact::from_tile<EPS, DUEL>(D, s, v, y, lane, eps, explored, q ? q + s.slot * 5 : nullptr);
}

struct DeepGradArgs {
    const float* x;                    // [rows][L]
    const float* hidden1;              // [rows][H1]
    const float* hidden2;              // [rows][H2]
    const float* grad_y;               // [rows][O]
    const float* w2t;                  // [H1][H2]
    const float* w3;                   // [O][H2]
    double* partials;                  // [elements][B]
    float* grad_a1;                    // [rows][H1] or null
    float* grad_a2;                    // [rows][H2] or null
    long long rows, B;
    int32_t L, H1, H2, O, activation;
    int32_t sub;                       // rows of a sub-tile
    int32_t slab;                      // units of H1 in a w2t slab
    int32_t s1, s2;                    // slices of the first and of the second product
};

__device__ __forceinline__ float4* quad(float* p) { return static_cast<float4*>(__builtin_assume_aligned(p, 16)); }

// A wave-uniform value kept in a vector register from here on (ccx_mlp_wide.hip's device): what the loops below derive from
// the sizes -- strides, the reciprocals of their divisions -- would otherwise all be hoisted into scalar registers, more than
// there are.
template <typename T>
__device__ __forceinline__ T per_lane(T v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(dp::kThreads) void deep_grad_blocks_kernel(const DeepGradArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kT = dp::kThreads;
    const int tid = (int)threadIdx.x;
    const int L = A.L, H1 = A.H1, H2 = A.H2, O = A.O, R = A.sub, H24 = per_lane(H2 / 4), H14 = per_lane(H1 / 4);
    const int Lv = per_lane(L), H1v = per_lane(H1), Ov = per_lane(O);     // (where they divide or are a row stride)
    const dp::RowImage m = dp::row_image(L, H1, H2);
    const int RS = per_lane(m.stride);
    float* w3s = lds + R * RS;
    float* w2s = w3s + O * H2;                                           // the w2t slab (first product only), pitch P
    const int P = per_lane(H2 + 1), H2v = per_lane(H2);
    const long long r0 = (long long)blockIdx.x * mg::kBlockRows, left = A.rows - r0;
    const int nb = left < mg::kBlockRows ? (int)left : mg::kBlockRows;   // (>= 1: the grid has ceil(rows / 256) blocks)
    // this slice's product (uniform for the workgroup) and this thread's tile in it: li / rj = its first left / right index
    const int s = (int)blockIdx.y;
    const int role = s < A.s1 ? 0 : s < A.s1 + A.s2 ? 1 : 2;
    const int t = (s - (role == 0 ? 0 : role == 1 ? A.s1 : A.s1 + A.s2)) * kT + tid;
    const int cols4 = role == 0 ? H14 : role == 1 ? H24 : H24 + 1;
    const int rows_in = role == 0 ? L + 1 : role == 1 ? H1 + 1 : O;
    const int pitch = role == 2 ? H2 + 1 : role == 1 ? H2 : H1;
    const int tiles = ((rows_in + 3) / 4) * cols4;
    const long long base = role == 0 ? 0 : role == 1 ? dp::first_elements(L, H1) : dp::first_elements(L, H1) + mg::second_part(H1, H2);
    const bool live = t < tiles;
    const int li = live ? 4 * (t / cols4) : 0, rj = live ? 4 * (t % cols4) : 0;
    const int loff = (role == 0 ? 0 : role == 1 ? m.h1 : m.gy) + li, roff = (role == 0 ? m.ga1 : role == 1 ? m.ga2 : m.h2) + rj;
    for (int i = tid; i < O * H2; i += kT) w3s[i] = A.w3[i];
    for (int r = tid; r < R; r += kT) {
        lds[r * RS + L] = 1.0f;
        lds[r * RS + m.h1 + H1] = 1.0f;
        lds[r * RS + m.h2 + H2] = 1.0f;
    }
    double acc[mg::kTile][mg::kTile] = {};
    for (int s0 = 0; s0 < nb; s0 += R) {
        const int nr = nb - s0 < R ? nb - s0 : R;
        const long long rs = r0 + s0;
        // 1. what the product needs: grad_y and hidden2 always, hidden1 for the second, x for the first
#pragma unroll 1
        for (int i = tid; i < nr * O; i += kT) {
            const int r = (int)((uint32_t)i / (uint32_t)Ov), o = i - r * Ov;
            lds[r * RS + m.gy + o] = A.grad_y[rs * Ov + i];
        }
        const float4* h24 = reinterpret_cast<const float4*>(A.hidden2) + rs * H24;
#pragma unroll 1
        for (int p = tid; p < nr * H24; p += kT) {
            const int r = (int)((uint32_t)p / (uint32_t)H24), q = p - r * H24;
            *quad(lds + r * RS + m.h2 + 4 * q) = h24[p];
        }
        if (role == 1) {
            const float4* h14 = reinterpret_cast<const float4*>(A.hidden1) + rs * H14;
#pragma unroll 1
            for (int p = tid; p < nr * H14; p += kT) {
                const int r = (int)((uint32_t)p / (uint32_t)H14), q = p - r * H14;
                *quad(lds + r * RS + m.h1 + 4 * q) = h14[p];
            }
        }
        if (role == 0) {
            const float* xs = A.x + rs * Lv;
#pragma unroll 1
            for (int p = tid; p < nr * L; p += kT) {
                const int r = (int)((uint32_t)p / (uint32_t)Lv), k = p - r * Lv;
                lds[r * RS + k] = xs[p];
            }
        }
        __syncthreads();
        if (role < 2) {
            // 2. ga2, four units at a time
#pragma unroll 1
            for (int p = tid; p < nr * H24; p += kT) {
                const int r = (int)((uint32_t)p / (uint32_t)H24), j = 4 * (p - r * H24);
                const float* row = lds + r * RS;
                float g[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) g[c] = mg::ga_unit(A.activation, mg::gh_unit(O, row + m.gy, w3s + j + c, H2), row[m.h2 + j + c]);
                const float4 q = make_float4(g[0], g[1], g[2], g[3]);
                *quad(lds + r * RS + m.ga2 + j) = q;
                if (A.grad_a2 && s == A.s1) reinterpret_cast<float4*>(A.grad_a2)[(rs + r) * H24 + (j >> 2)] = q;
            }
            __syncthreads();
        }
        if (role == 0) {
            // 3. ga1: the gh1 chain of unit i along w2t[i][0 .. H2-1], w2t through LDS in slabs of whole rows
            for (int i0 = 0; i0 < H1; i0 += A.slab) {
                const int sn = H1 - i0 < A.slab ? H1 - i0 : A.slab;
                const float* src = A.w2t + (long long)i0 * H2;
#pragma unroll 1
                for (int q = tid; q < sn * H2; q += kT) {
                    const int ii = (int)((uint32_t)q / (uint32_t)H2v), j = q - ii * H2v;
                    w2s[ii * P + j] = src[q];
                }
                __syncthreads();
#pragma unroll 1
                for (int p = tid; p < nr * sn; p += kT) {
                    const int r = (int)((uint32_t)p / (uint32_t)sn), i = i0 + p - r * sn;
                    const float v = dp::ga1_unit(A.activation, H2, lds + r * RS + m.ga2, w2s + (i - i0) * P, A.hidden1[(rs + r) * H1v + i]);
                    lds[r * RS + m.ga1 + i] = v;
                    if (A.grad_a1 && s == 0) A.grad_a1[(rs + r) * H1v + i] = v;
                }
                __syncthreads();                                         // the slab may be overwritten; behind the last one ga1 is whole
            }
        }
        // 4. the chains: this thread's 16 elements, the sub-tile's rows in ascending order
#pragma unroll 2
        for (int r = 0; r < nr; ++r) {
            const float4 a4 = *quad(lds + r * RS + loff);
            const float4 b4 = *quad(lds + r * RS + roff);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            mg::tile_row(acc, a, b);
        }
        __syncthreads();                                                 // the image may be overwritten
    }
#pragma unroll
    for (int i = 0; i < mg::kTile; ++i) {
#pragma unroll
        for (int j = 0; j < mg::kTile; ++j) {
            if (live && li + i < rows_in && rj + j < pitch)
                A.partials[(base + (long long)(li + i) * pitch + rj + j) * A.B + blockIdx.x] = acc[i][j];
        }
    }
}

int check_dims(const char* who, int32_t L, int32_t H1, int32_t H2, int32_t O, int32_t activation) {
    if (!dp::shape_ok(L, H1, H2, O, activation))
        return fail(CCX_EINVAL, "%s: L = %d, H1 = %d, H2 = %d, O = %d, activation = %d: 1 <= L <= %d, H1 and H2 multiples of 16 in 16..%d, "
                    "1 <= O <= %d and activation 0 (tanh) or 1 (relu) are required", who, L, H1, H2, O, activation, ccx_mlp::kMaxL,
                    ccx_mlp::kMaxH, dp::kMaxO);
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_mlp_deep_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O, int32_t activation, const float* x,
                         const float* w1t, const float* b1, const float* w2t, const float* b2, const float* w3, const float* b3, float* y,
                         float* hidden1_or_null, float* hidden2_or_null) {
    const char* who = "ccx_mlp_deep_forward";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !w1t || !b1 || !w2t || !b2 || !w3 || !b3 || !y) return fail(CCX_EINVAL, "%s: NULL argument (only hidden1 and hidden2 may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, 64, blocks)) return rc;
    if (int rc = check_dims(who, L, H1, H2, O, activation)) return rc;
    if (misaligned(16, x, hidden1_or_null, hidden2_or_null)) return fail(CCX_EINVAL, "%s: x, hidden1 and hidden2 must be 16-byte aligned", who);
    if (misaligned(4, w1t, b1, w2t, b2, w3, b3, y)) return fail(CCX_EINVAL, "%s: w1t, b1, w2t, b2, w3, b3 and y must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const DeepDims S{(long long)rows, L, H1, H2, O, activation};
    const size_t bytes = dp::lds_floats(L, H1, H2, O, false) * sizeof(float);
    CCX_HIP(ccx_tile::allow_lds(deep_forward_kernel, bytes));
    hipLaunchKernelGGL(deep_forward_kernel, dim3(blocks), dim3(64 * dp::waves_of(H1, H2)), bytes, h->stream, S, x, w1t, b1, w2t, b2, w3, b3, y,
                       hidden1_or_null, hidden2_or_null);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_mlp_deep_sample_actions(ccx_handle* h, int32_t H1, int32_t H2, int32_t activation, const float* obs, const float* w1t,
                                const float* b1, const float* w2t, const float* b2, const float* w3, const float* b3,
                                const uint8_t* masks_or_null, int32_t deterministic, uint8_t* actions, float* logp_or_null,
                                float* entropy_or_null, float* logits_or_null) {
    const char* who = "ccx_mlp_deep_sample_actions";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !w1t || !b1 || !w2t || !b2 || !w3 || !b3 || !actions)
        return fail(CCX_EINVAL, "%s: NULL argument (obs, the six parameter arrays and actions are required)", who);
    const int32_t L = ccx_obs_len(h->N);
    const int64_t rows = (int64_t)h->E * h->N;
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, 64, blocks)) return rc;
    if (int rc = check_dims(who, L, H1, H2, 5, activation)) return rc;
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "%s: obs must be 16-byte aligned", who);
    if (misaligned(4, w1t, b1, w2t, b2, w3, b3, logp_or_null, entropy_or_null, logits_or_null))
        return fail(CCX_EINVAL, "%s: the six parameter arrays, logp, entropy and logits must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const DeepDims S{(long long)rows, L, H1, H2, 5, activation};
    const DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, logp_or_null, entropy_or_null);
    const size_t bytes = dp::lds_floats(L, H1, H2, 5, true) * sizeof(float);
    const dim3 grid(blocks), block(64 * dp::waves_of(H1, H2));
    const int rc = with_flags([&](auto det, auto stats) -> int {
        constexpr bool DET = decltype(det)::value, STATS = decltype(stats)::value;
        CCX_HIP(ccx_tile::allow_lds(deep_draw_kernel<DET, STATS>, bytes));
        hipLaunchKernelGGL((deep_draw_kernel<DET, STATS>), grid, block, bytes, h->stream, S, obs, w1t, b1, w2t, b2, w3, b3, logits_or_null, D);
        return CCX_OK;
    }, deterministic != 0, logp_or_null || entropy_or_null);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int ccx_mlp_deep_q_actions(ccx_handle* h, int32_t H1, int32_t H2, int32_t activation, int32_t O, const float* obs, const float* w1t,
                           const float* b1, const float* w2t, const float* b2, const float* w3, const float* b3,
                           const uint8_t* masks_or_null, const float* epsilon_or_null, uint8_t* actions, uint8_t* explored_or_null,
                           float* q_or_null) {
    const char* who = "ccx_mlp_deep_q_actions";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!obs || !w1t || !b1 || !w2t || !b2 || !w3 || !b3 || !actions)
        return fail(CCX_EINVAL, "%s: NULL argument (obs, the six parameter arrays and actions are required)", who);
    if (O != 5 && O != 6) return fail(CCX_EINVAL, "%s: O = %d, 5 (plain) or 6 (dueling) is required", who, (int)O);
    const int32_t L = ccx_obs_len(h->N);
    const int64_t rows = (int64_t)h->E * h->N;
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, 64, blocks)) return rc;
    if (int rc = check_dims(who, L, H1, H2, O, activation)) return rc;
    if (misaligned(16, obs)) return fail(CCX_EINVAL, "%s: obs must be 16-byte aligned", who);
    if (misaligned(4, w1t, b1, w2t, b2, w3, b3, epsilon_or_null, q_or_null))
        return fail(CCX_EINVAL, "%s: the six parameter arrays, epsilon and q must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const DeepDims S{(long long)rows, L, H1, H2, O, activation};
    const DrawArgs D = ccx_qact::draw_args(h, masks_or_null, actions);
    const size_t bytes = dp::lds_floats(L, H1, H2, O, true) * sizeof(float);
    const dim3 grid(blocks), block(64 * dp::waves_of(H1, H2));
    const int rc = with_flags([&](auto eps, auto duel) -> int {
        constexpr bool EPS = decltype(eps)::value, DUEL = decltype(duel)::value;
        CCX_HIP(ccx_tile::allow_lds(deep_q_kernel<EPS, DUEL>, bytes));
        hipLaunchKernelGGL((deep_q_kernel<EPS, DUEL>), grid, block, bytes, h->stream, S, obs, w1t, b1, w2t, b2, w3, b3,
                           DUEL ? nullptr : q_or_null, D, epsilon_or_null, explored_or_null, q_or_null);
        return CCX_OK;
    }, epsilon_or_null != nullptr, O == 6);
    if (rc) return rc;
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int64_t ccx_mlp_deep_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O) {
    return dp::workspace_bytes(rows, L, H1, H2, O);
}

int ccx_mlp_deep_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H1, int32_t H2, int32_t O, int32_t activation, const float* x,
                          const float* hidden1, const float* hidden2, const float* grad_y, const float* w2t, const float* w3,
                          void* workspace, float* grad_w1t, float* grad_b1, float* grad_w2t, float* grad_b2, float* grad_w3,
                          float* grad_b3, float* grad_a1_or_null, float* grad_a2_or_null) {
    const char* who = "ccx_mlp_deep_backward";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !hidden1 || !hidden2 || !grad_y || !w2t || !w3 || !workspace || !grad_w1t || !grad_b1 || !grad_w2t || !grad_b2 || !grad_w3 ||
        !grad_b3)
        return fail(CCX_EINVAL, "%s: NULL argument (only grad_a1 and grad_a2 may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, mg::kBlockRows, blocks)) return rc;
    if (int rc = check_dims(who, L, H1, H2, O, activation)) return rc;
    if (misaligned(16, x, hidden1, hidden2, grad_a1_or_null, grad_a2_or_null))
        return fail(CCX_EINVAL, "%s: x, hidden1, hidden2, grad_a1 and grad_a2 must be 16-byte aligned", who);
    if (misaligned(8, workspace)) return fail(CCX_EINVAL, "%s: workspace must be 8-byte aligned", who);
    if (misaligned(4, grad_y, w2t, w3, grad_w1t, grad_b1, grad_w2t, grad_b2, grad_w3, grad_b3))
        return fail(CCX_EINVAL, "%s: grad_y, w2t, w3 and the six gradients must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    size_t image = 0;
    const int R = dp::sub_rows(L, H1, H2, O, image);
    const size_t bytes = dp::grad_lds_bytes(L, H1, H2, O);
    CCX_HIP(ccx_tile::allow_lds(deep_grad_blocks_kernel, bytes));
    double* ws = static_cast<double*>(workspace);
    const DeepGradArgs A{x, hidden1, hidden2, grad_y, w2t, w3, ws, grad_a1_or_null, grad_a2_or_null, (long long)rows, (long long)blocks,
                         L, H1, H2, O, activation, R, dp::slab_units(H1), (int32_t)dp::slices1(L, H1), (int32_t)dp::slices2(H1, H2)};
    hipLaunchKernelGGL(deep_grad_blocks_kernel, dim3(blocks, dp::grid_y(L, H1, H2, O)), dim3(dp::kThreads), bytes, h->stream, A);
    CCX_HIP(hipGetLastError());
    // the final step, CCX_MLP's kernel on each stretch: (L, H1) with no second part, then (H1, H2, O)
    if (int rc = ccxi::head_grad_final_launch(h, L, H1, 0, ws, (long long)blocks, grad_w1t, grad_b1, nullptr, nullptr)) return rc;
    return ccxi::head_grad_final_launch(h, H1, H2, O, ws + dp::first_elements(L, H1) * (long long)blocks, (long long)blocks, grad_w2t, grad_b2,
                                        grad_w3, grad_b3);
}

}  // extern "C"
