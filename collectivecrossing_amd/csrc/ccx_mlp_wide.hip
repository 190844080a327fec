// ccx_mlp_wide.hip -- CCX_MLP_WIDE (include/ccx.h): CCX_MLP's forward and backward with up to 320 outputs -- the 5 A atom
// logits of a categorical head (CCX_C51).  The rule is CCX_MLP's; the arithmetic is ccx_mlp.h's and ccx_mlp_grad.h's
// functions, one operation per line (-ffp-contract=off; `/` is the correctly rounded division, asked for on this unit's
// compile line).  What is new is where the data lies (ccx_mlp_wide.h states the launch shapes).
//
// wide_forward_kernel.  Layer 1 is ccx_mlp_tile.h's mapping: a workgroup takes 64 adjacent rows and has G = H / 16 waves, lane
// l owns row l, wave g the hidden units of group g (16 accumulators, w1t / b1 / w2 through scalar loads), the x tile in LDS at
// an odd row stride (ccx_tile::AdjacentRows loads it).  Layer 2 cannot keep [G][64][O] partials (1 MB at the limits), so it
// runs over chunks of C consecutive outputs: wave g writes its group's partials of the chunk to LDS as [g][o][65] -- the 64
// lanes of a write adjacent, conflict-free --, and behind a barrier all threads take the chunk's 64 C sums in the flat order
// row * C + o: each adds the G partials in group order onto b2[o] (in a whole chunk the 32 lanes of a read group read 32
// outputs of one row: pitch 65, 32 different banks; the lanes of a partial last chunk straddle rows) and adjacent threads store adjacent dwords of a row of y, whole 128-byte lines where C
// is a multiple of 32 and the row's start allows it.
//
// wide_grad_blocks_kernel.  Workgroup (b, s) takes block b of 256 consecutive rows and slice s of the 4 x 4 output tiles,
// one tile per thread, as ccx_mlp_backward.hip does; a slice lies in ONE part.  A slice of [x | 1]^T ga walks the block in
// sub-tiles of R rows: x to the LDS image, then per slab of S consecutive outputs w2[o0 .. o0 + S) and the rows' grad_y of
// the slab to LDS and every (row, four units) item continues its gh chains (kept in the image's ga slot between slabs, which
// starts as -0.0f, the identity of the addition; o ascending, the order of the rule), then ga from hidden (read once, from
// memory), grad_a if asked (slice 0), and the rows IN ORDER onto the 16 f64 accumulators.  A slice of grad_y^T [hidden | 1] loads hidden and the grad_y columns of its own
// tiles only, and walks the same chains.  The partial of element e lands at partials[e][b]: ccx_mlp_grad.h's layout, so
// the final step is ccx_mlp_backward.hip's head_grad_final_kernel as it is (ccxi::head_grad_final_launch).  No atomic, no
// last-block-done counter.
#include "ccx_mlp_tile.h"
#include "ccx_mlp_wide.h"

using ccx_tile::AdjacentRows;
using ccx_tile::MlpArgs;
using ccxi::fail;
using ccxi::misaligned;
namespace mg = ccx_mlp_grad;
namespace wd = ccx_wide;

namespace {

// The seven arrays are separate `__restrict__` kernel arguments, not members of a by-value struct: the chunk loop below stores
// y and then reads w2 and b2 of the next chunk, and only with the arguments known not to alias does the compiler keep those
// wave-uniform reads on the scalar unit (s_load_dwordx16 / s_load_dword) instead of 64 identical per-lane loads.
__global__ __launch_bounds__(1024) void wide_forward_kernel(const float* __restrict__ x, const float* __restrict__ w1t,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ y,
                                                            float* __restrict__ hidden, long long rows, int32_t L, int32_t H, int32_t O,
                                                            int32_t activation, int32_t C /* outputs of a chunk */) {
    extern __shared__ float lds[];
    const MlpArgs A{x, w1t, b1, w2, b2, y, hidden, rows, L, H, O, activation};
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int g = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int G = H / wd::kGroup, T = G * 64, Lp = L | 1;
    AdjacentRows R;
    R.begin(A);
    const int nr = R.nr;
    // 1. the x tile
    R.load_x(A, lds, tid, T);
    __syncthreads();
    // 2. layer 1: this wave's 16 units of the lane's row (surplus lanes of the tail tile repeat its last row)
    const uint32_t rl = (int)lane < nr ? lane : (uint32_t)(nr - 1);
    const float* xr = lds + rl * (uint32_t)Lp;
    const float* wg = w1t + wd::kGroup * g;
    float a[wd::kGroup];
#pragma unroll
    for (int j = 0; j < wd::kGroup; ++j) a[j] = b1[wd::kGroup * g + j];
#pragma unroll 2
    for (int k = 0; k < L; ++k) ccx_mlp::layer1_step(a, xr[k], wg + (long long)k * H);
    if (activation == ccx_mlp::kRelu) {
#pragma unroll
        for (int j = 0; j < wd::kGroup; ++j) a[j] = ccx_mlp::relu_spec(a[j]);
    } else {
#pragma unroll
        for (int j = 0; j < wd::kGroup; ++j) a[j] = ccx_mlp::tanh_spec(a[j]);
    }
    if (hidden && (int)lane < nr) {
        float4* hp = reinterpret_cast<float4*>(hidden + R.row(lane) * H + wd::kGroup * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) hp[q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    }
    // 3. layer 2, chunk by chunk
    const int per = C * wd::kRowPitch;                                   // floats of one group's partials
    float* mine = lds + g * per + (int)lane;
    float* yrow = y + R.r0 * O;
    for (int c0 = 0; c0 < O; c0 += C) {
        const int cn = O - c0 < C ? O - c0 : C;
        __syncthreads();                                                 // the x tile / the chunk before may go
        const float* w = w2 + (long long)c0 * H + wd::kGroup * g;
#pragma clang loop vectorize(disable) interleave(disable)              // (no copy of the loop for a stride H of 1)
        for (int oc = 0; oc < cn; ++oc) mine[oc * wd::kRowPitch] = ccx_mlp::layer2_partial(a, w + oc * H);
        __syncthreads();
        for (int i = (int)tid; i < 64 * cn; i += T) {
            const int r = i / cn, oc = i - r * cn;
            const float v = ccx_mlp::layer2_sum(b2[c0 + oc], lds + oc * wd::kRowPitch + r, G, per);
            if (r < nr) yrow[(long long)r * O + c0 + oc] = v;
        }
    }
}

struct WideGradArgs {
    const float* x;                    // [rows][L]
    const float* hidden;               // [rows][H]
    const float* grad_y;               // [rows][O]
    const float* w2;                   // [O][H]
    double* partials;                  // [elements][B]
    float* grad_a;                     // [rows][H] or null
    long long rows, B;
    int32_t L, H, O, activation;
    int32_t slab;                      // outputs of a w2 slab
    int32_t rows1, rows2;              // rows of a sub-tile in the two parts
    int32_t slices1;                   // slices of the first part
};

// A wave-uniform value kept in a vector register from here on: what the loops below derive from the sizes -- strides, byte
// offsets, the reciprocals of their divisions -- would otherwise all be hoisted into scalar registers, more than there are.
template <typename T>
__device__ __forceinline__ T per_lane(T v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float4* quad(float* p) { return static_cast<float4*>(__builtin_assume_aligned(p, 16)); }

// the chains of one sub-tile: this thread's 16 elements, the rows in ascending order
__device__ __forceinline__ void chains(double (&acc)[mg::kTile][mg::kTile], float* lds, int nr, int RS, int loff, int roff) {
#pragma unroll 2
    for (int r = 0; r < nr; ++r) {
        const float4 a4 = *quad(lds + r * RS + loff);
        const float4 b4 = *quad(lds + r * RS + roff);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
        mg::tile_row(acc, a, b);
    }
}

__global__ __launch_bounds__(wd::kThreads) void wide_grad_blocks_kernel(const WideGradArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kT = wd::kThreads;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = A.L, H = A.H, H4 = per_lane(H / 4);
    const int O = A.O, Ov = per_lane(O);                                 // (Ov: O where it is a row stride)
    const long long r0 = (long long)blockIdx.x * mg::kBlockRows, left = A.rows - r0;
    const int nb = left < mg::kBlockRows ? (int)left : mg::kBlockRows;   // (>= 1: the grid has ceil(rows / 256) blocks)
    const bool second = (int)blockIdx.y >= A.slices1;
    double acc[mg::kTile][mg::kTile] = {};
    int li, rj;
    bool live;
    if (!second) {
        // ---- a slice of [x | 1]^T ga
        const int S = A.slab, R = A.rows1;
        const wd::FirstImage m = wd::first_image(L, H, S);
        const int RS = per_lane(m.stride);
        float* w2s = lds + per_lane(R * RS);                             // (the offset, not the pointer: LDS stays LDS)
        const int ga_at = per_lane(m.ga), gy_at = per_lane(m.gy);
        const int t = (int)blockIdx.y * kT + tid;
        live = t < (m.ga / 4) * H4;
        const int tr = (int)((uint32_t)t / (uint32_t)H4);
        li = live ? 4 * tr : 0;
        rj = live ? 4 * (t - tr * H4) : 0;
#pragma unroll 1
        for (int r = tid; r < R; r += kT) lds[r * RS + L] = 1.0f;
#pragma unroll 1
        for (int s0 = 0; s0 < nb; s0 += R) {
            const int nr = nb - s0 < R ? nb - s0 : R;
            const long long rs = per_lane(r0 + s0);
            const float* xs = A.x + rs * L;
#pragma unroll 1
            for (int r = wave; r < nr; r += kT / 64) {                    // a wave to a row: no division by L
#pragma unroll 1
                for (int k = lane; k < L; k += 64) lds[r * RS + k] = xs[r * L + k];
#pragma unroll 1
                for (int j = lane; j < H; j += 64) lds[r * RS + ga_at + j] = wd::kChainStart;     // where the gh chains start
            }
#pragma unroll 1
            for (int o0 = 0; o0 < O; o0 += S) {
                const int sn = O - o0 < S ? O - o0 : S;
                const float* wsrc = A.w2 + (long long)o0 * H;
#pragma unroll 1
                for (int i = tid; i < sn * H; i += kT) w2s[i] = wsrc[i];
#pragma unroll 1
                for (int r = wave; r < nr; r += kT / 64) {
#pragma unroll 1
                    for (int o = lane; o < sn; o += 64) lds[r * RS + gy_at + o] = A.grad_y[(rs + r) * Ov + o0 + o];
                }
                __syncthreads();
#pragma unroll 1
                for (int p = tid; p < nr * H4; p += kT) {
                    const int r = (int)((uint32_t)p / (uint32_t)H4), j = 4 * (p - r * H4);
                    float* row = lds + r * RS;
                    float4 q = *quad(row + ga_at + j);
                    float g[4] = {q.x, q.y, q.z, q.w};
                    wd::gh_more4(g, sn, row + gy_at, w2s + j, H);
                    *quad(row + ga_at + j) = make_float4(g[0], g[1], g[2], g[3]);
                }
                __syncthreads();                                         // the slab may be overwritten
            }
            // gh is complete: ga, four units at a time (each item reads and writes its own quad)
#pragma unroll 1
            for (int p = tid; p < nr * H4; p += kT) {
                const int r = (int)((uint32_t)p / (uint32_t)H4), j = 4 * (p - r * H4);
                float* row = lds + r * RS;
                const float4 q = *quad(row + ga_at + j);
                const float4 h = reinterpret_cast<const float4*>(A.hidden)[(rs + r) * H4 + (j >> 2)];
                const float4 v = make_float4(mg::ga_unit(A.activation, q.x, h.x), mg::ga_unit(A.activation, q.y, h.y),
                                             mg::ga_unit(A.activation, q.z, h.z), mg::ga_unit(A.activation, q.w, h.w));
                *quad(row + ga_at + j) = v;
                if (A.grad_a && blockIdx.y == 0) reinterpret_cast<float4*>(A.grad_a)[(rs + r) * H4 + (j >> 2)] = v;
            }
            __syncthreads();
            chains(acc, lds, nr, RS, li, ga_at + rj);
            __syncthreads();                                             // the image may be overwritten
        }
    } else {
        // ---- a slice of grad_y^T [hidden | 1]
        const int R = A.rows2, JT = H4 + 1;
        const wd::SecondImage m = wd::second_image(H, O);
        const int RS = per_lane(m.stride);
        const int u0 = ((int)blockIdx.y - A.slices1) * kT, u = u0 + tid;
        live = u < ((O + 3) / 4) * JT;
        const int c0 = 4 * (u0 / JT);                                    // the slice's first grad_y column
        const int ur = (int)((uint32_t)u / (uint32_t)JT);
        li = live ? 4 * ur : c0;                                         // (an idle thread reads the slice's first quads)
        rj = live ? 4 * (u - ur * JT) : 0;
        const int last = 4 * ((u0 + kT - 1) / JT) + 4, all = (O + 3) & ~3;
        const int nc = (last < all ? last : all) - c0;                   // its columns, a multiple of 4, <= second_columns
#pragma unroll 1
        for (int r = tid; r < R; r += kT) lds[r * RS + H] = 1.0f;
#pragma unroll 1
        for (int s0 = 0; s0 < nb; s0 += R) {
            const int nr = nb - s0 < R ? nb - s0 : R;
            const long long rs = per_lane(r0 + s0);
            const float4* h4 = reinterpret_cast<const float4*>(A.hidden) + rs * H4;
#pragma unroll 1
            for (int p = tid; p < nr * H4; p += kT) {
                const int r = (int)((uint32_t)p / (uint32_t)H4), q = p - r * H4;
                *quad(lds + r * RS + 4 * q) = h4[p];
            }
#pragma unroll 1
            for (int r = wave; r < nr; r += kT / 64) {
#pragma unroll 1
                for (int c = lane; c < nc; c += 64) lds[r * RS + m.gy + c] = c0 + c < O ? A.grad_y[(rs + r) * Ov + c0 + c] : 0.0f;
            }
            __syncthreads();
            chains(acc, lds, nr, RS, m.gy + li - c0, rj);
            __syncthreads();
        }
    }
    // the tile's elements: row a, column c of its part is element base + a * pitch + c (ccx_mlp_grad.h: elements_of)
    const int pitch = second ? H + 1 : H, rows_in = second ? O : L + 1;
    const long long e0 = (second ? mg::second_part(L, H) : 0) + (long long)li * pitch + rj;
#pragma unroll
    for (int i = 0; i < mg::kTile; ++i) {
#pragma unroll
        for (int j = 0; j < mg::kTile; ++j) {
            if (live && li + i < rows_in && rj + j < pitch) A.partials[(e0 + i * pitch + j) * A.B + blockIdx.x] = acc[i][j];
        }
    }
}

int check_dims(const char* who, int32_t L, int32_t H, int32_t O, int32_t activation) {
    if (!wd::shape_ok(L, H, O, activation))
        return fail(CCX_EINVAL, "%s: L = %d, H = %d, O = %d, activation = %d: 1 <= L <= %d, H a multiple of 16 in 16..%d, 1 <= O <= %d and "
                    "activation 0 (tanh) or 1 (relu) are required", who, L, H, O, activation, ccx_mlp::kMaxL, ccx_mlp::kMaxH, wd::kMaxO);
    return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_mlp_wide_forward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                         const float* w1t, const float* b1, const float* w2, const float* b2, float* y, float* hidden_or_null) {
    const char* who = "ccx_mlp_wide_forward";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !w1t || !b1 || !w2 || !b2 || !y) return fail(CCX_EINVAL, "%s: NULL argument (only hidden may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, 64, blocks)) return rc;
    if (int rc = check_dims(who, L, H, O, activation)) return rc;
    if (misaligned(16, x, hidden_or_null)) return fail(CCX_EINVAL, "%s: x and hidden must be 16-byte aligned", who);
    if (misaligned(4, w1t, b1, w2, b2, y)) return fail(CCX_EINVAL, "%s: w1t, b1, w2, b2 and y must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    const size_t bytes = wd::lds_floats(L, H, O) * sizeof(float);
    CCX_HIP(ccx_tile::allow_lds(wide_forward_kernel, bytes));
    hipLaunchKernelGGL(wide_forward_kernel, dim3(blocks), dim3(64 * (H / wd::kGroup)), bytes, h->stream, x, w1t, b1, w2, b2, y,
                       hidden_or_null, (long long)rows, L, H, O, activation, (int32_t)wd::chunk_outputs(H, O));
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

int64_t ccx_mlp_wide_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H, int32_t O) { return wd::workspace_bytes(rows, L, H, O); }

int ccx_mlp_wide_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                          const float* hidden, const float* grad_y, const float* w2, void* workspace, float* grad_w1t, float* grad_b1,
                          float* grad_w2, float* grad_b2, float* grad_a_or_null) {
    const char* who = "ccx_mlp_wide_backward";
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!x || !hidden || !grad_y || !w2 || !workspace || !grad_w1t || !grad_b1 || !grad_w2 || !grad_b2)
        return fail(CCX_EINVAL, "%s: NULL argument (only grad_a may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, mg::kBlockRows, blocks)) return rc;
    if (int rc = check_dims(who, L, H, O, activation)) return rc;
    if (misaligned(16, x, hidden, grad_a_or_null)) return fail(CCX_EINVAL, "%s: x, hidden and grad_a must be 16-byte aligned", who);
    if (misaligned(8, workspace)) return fail(CCX_EINVAL, "%s: workspace must be 8-byte aligned", who);
    if (misaligned(4, grad_y, w2, grad_w1t, grad_b1, grad_w2, grad_b2))
        return fail(CCX_EINVAL, "%s: grad_y, w2, grad_w1t, grad_b1, grad_w2 and grad_b2 must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    size_t b1 = 0, b2 = 0;
    const int R1 = wd::first_rows(L, H, O, b1), R2 = wd::second_rows(H, O, b2);
    const WideGradArgs A{x, hidden, grad_y, w2, static_cast<double*>(workspace), grad_a_or_null, (long long)rows, (long long)blocks,
                         L, H, O, activation, wd::slab_outputs(H, O), R1, R2, (int32_t)wd::first_slices(L, H)};
    hipLaunchKernelGGL(wide_grad_blocks_kernel, dim3(blocks, wd::grid_y(L, H, O)), dim3(wd::kThreads), wd::grad_lds_bytes(L, H, O),
                       h->stream, A);
    return ccxi::head_grad_final_launch(h, L, H, O, static_cast<double*>(workspace), (long long)blocks, grad_w1t, grad_b1, grad_w2, grad_b2);
}

}  // extern "C"
