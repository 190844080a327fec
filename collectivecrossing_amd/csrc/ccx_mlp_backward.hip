// ccx_mlp_backward.hip -- the backward pass of CCX_MLP (include/ccx.h): the gradients of the four parameter arrays from the
// rows, the saved activations and the gradient of the outputs, by a written rule.  The per-row f32 part, the terms of the
// f64 chains are ccx_mlp_grad.h; the final step over the block partials is ccx_tree.h's.
//
// Two launches.  head_grad_blocks_kernel: workgroup (b, s) takes block b of 256 consecutive rows and slice s of the output
// elements.  The elements are cut into 4 x 4 tiles, one tile per thread, 256 tiles per slice: the tiles of
// [x | 1]^T ga (grad_w1t, and grad_b1 as the row of the constant 1) and then those of grad_y^T [hidden | 1] (grad_w2, and
// grad_b2 as the column of the constant 1).  The block is walked in sub-tiles of R rows (64, or fewer where a row is long:
// what fits 64 KB of LDS).  Per sub-tile all threads load x (16-byte pieces, the array's last piece element by element),
// hidden (16-byte pieces) and grad_y into one LDS image -- a row is [x, 1, pad | ga | hidden, 1, pad | grad_y, pad], every
// part at a multiple of four floats -- compute ga four units at a time (w2 sits in LDS for the whole workgroup), and write
// grad_a if asked (slice 0).  Behind a barrier every thread adds the sub-tile's rows IN ORDER onto its 16 f64 accumulators:
// two 16-byte LDS reads (all lanes read the same row, the 16 lanes of a read group different quads: no bank conflict), eight
// conversions, sixteen f64 multiply-adds per row.  A thread owns its elements and walks the rows, so the chain of the rule
// is the loop itself and nothing crosses lanes.  Rows >= M are never walked.  The partial of element e lands at
// partials[e][b].
// head_grad_final_kernel: one wave per element; lane j is place j of ccx_tree.h's final step (contiguous, coalesced reads of
// the element's B partials), the 64 places are halved by ccx_tree.h's butterfly, lane 0 rounds to f32 once and
// stores.  No atomic, no last-block-done counter: a kernel boundary orders the partials.
//
// CCX_SIDES (ccx_sides_backward): the same two launches over the SELECTED rows of one slot group of [M][N][..] arrays
// (ccx_sides.h).  The body of the blocks kernel is one function, grad_blocks, over a `Rows` argument that says where the
// rows of a sub-tile lie: AdjacentRows (rows rs .. rs + nr - 1 of the arrays, the loads above) or PickedRows (block b holds
// selection indices 256 b .. 256 b + 255; per sub-tile the first nr threads leave the flat rows m N + a in LDS, and x -- 8-byte
// pieces when L is even, as in ccx_sides.hip --, hidden, grad_y and grad_a are addressed through them).  The row image, ga,
// the chains and the partials' layout are the same code, so sides_grad_blocks_kernel's partials are those of the gathered
// call and head_grad_final_kernel finishes them as it is.
#include "ccx_internal.h"
#include "ccx_mlp_grad.h"
#include "ccx_mlp_tile.h"                                                // (the shape check only: ccx_tile::check_dims)
#include "ccx_sides.h"

using ccxi::fail;
using ccxi::misaligned;
namespace mg = ccx_mlp_grad;

namespace {

constexpr int kThreads = mg::kThreads;
using mg::RowImage;
using mg::row_image;

struct HeadGradArgs {
    const float* x;                    // [rows][L]
    const float* hidden;               // [rows][H]
    const float* grad_y;               // [rows][O]
    const float* w2;                   // [O][H]
    double* partials;                  // [elements][B]
    float* grad_w1t;                   // [L][H]
    float* grad_b1;                    // [H]
    float* grad_w2;                    // [O][H]
    float* grad_b2;                    // [O]
    float* grad_a;                     // [rows][H] or null
    long long rows, B;
    int32_t L, H, O, activation;
    int32_t sub;                       // rows of a sub-tile
};

// a quad of the LDS image: every part of a row starts at a multiple of four floats and so does the row stride, which the
// compiler cannot see from the run-time sizes
__device__ __forceinline__ float4* quad(float* p) { return static_cast<float4*>(__builtin_assume_aligned(p, 16)); }

// Where the rows of a sub-tile lie.  AdjacentRows: rows rs .. rs + nr - 1 of [rows][..] arrays.
struct AdjacentRows {
    __device__ __forceinline__ void begin(const HeadGradArgs&, long long, int) const {}
    __device__ __forceinline__ void load(const HeadGradArgs& A, float* lds, const RowImage& m, long long rs, int nr, int tid, int L,
                                         int H4, int O, int RS) const {
        // 1. x: 16-byte pieces from rs * L on (16-byte aligned: rs * L is a multiple of 8 floats); the piece that holds the
        //    array's end is read element by element
        const int pieces = (nr * L + 3) / 4;
        const long long rest = (A.rows - rs) * L;                        // floats from the sub-tile's first to the array's end
        const int avail = rest < 4 * pieces ? (int)rest : 4 * pieces;
        const float* xs = A.x + rs * L;
        for (int p = tid; p < pieces; p += kThreads) {
            float v[4];
            if (4 * p + 3 < avail) {
                const float4 q = reinterpret_cast<const float4*>(xs)[p];
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = 4 * p + i < avail ? xs[4 * p + i] : 0.0f;
            }
            uint32_t r = (uint32_t)(4 * p) / (uint32_t)L, k = (uint32_t)(4 * p) - r * (uint32_t)L;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if ((int)r < nr) lds[r * (uint32_t)RS + k] = v[i];
                if (++k == (uint32_t)L) {
                    k = 0;
                    ++r;
                }
            }
        }
        //    hidden: rows are whole pieces
        const float4* h4 = reinterpret_cast<const float4*>(A.hidden) + rs * H4;
        for (int p = tid; p < nr * H4; p += kThreads) {
            const int r = p / H4, q = p - r * H4;
            *quad(lds + r * RS + m.hid + 4 * q) = h4[p];
        }
        //    grad_y
        for (int i = tid; i < nr * O; i += kThreads) {
            const int r = i / O, o = i - r * O;
            lds[r * RS + m.gy + o] = A.grad_y[rs * O + i];
        }
    }
    __device__ __forceinline__ long long row(long long rs, int r) const { return rs + r; }
};

// PickedRows: the sub-tile's rows are selection indices rs .. rs + nr - 1 of one slot group (ccx_sides.h); their flat rows
// m N + a are left in LDS by the first nr threads.  A.rows = M S, the number of selected rows.
struct PickedRows {
    uint64_t slots;
    int32_t S, N;
    long long* flat;                   // LDS [sub]
    __device__ __forceinline__ void begin(const HeadGradArgs&, long long rs, int nr) const {
        const int tid = (int)threadIdx.x;
        if (tid < nr) flat[tid] = ccx_sides::row_of(slots, S, N, ccx_sides::start_of(rs, S), (uint32_t)tid).row;
        __syncthreads();
    }
    __device__ __forceinline__ void load(const HeadGradArgs& A, float* lds, const RowImage& m, long long, int nr, int tid, int L,
                                         int H4, int O, int RS) const {
        // x: a row starts at a multiple of 8 bytes when L is even (x is 16-byte aligned), else dwords
        if ((L & 1) == 0) {
            const int L2 = L >> 1;
            for (int p = tid; p < nr * L2; p += kThreads) {
                const int r = p / L2, q = p - r * L2;
                const float2 v = reinterpret_cast<const float2*>(A.x + flat[r] * L)[q];
                lds[r * RS + 2 * q] = v.x;
                lds[r * RS + 2 * q + 1] = v.y;
            }
        } else {
            for (int p = tid; p < nr * L; p += kThreads) {
                const int r = p / L, k = p - r * L;
                lds[r * RS + k] = A.x[flat[r] * L + k];
            }
        }
        for (int p = tid; p < nr * H4; p += kThreads) {
            const int r = p / H4, q = p - r * H4;
            *quad(lds + r * RS + m.hid + 4 * q) = reinterpret_cast<const float4*>(A.hidden + flat[r] * A.H)[q];
        }
        for (int i = tid; i < nr * O; i += kThreads) {
            const int r = i / O, o = i - r * O;
            lds[r * RS + m.gy + o] = A.grad_y[flat[r] * O + o];
        }
    }
    __device__ __forceinline__ long long row(long long, int r) const { return flat[r]; }
};

template <class Rows>
__device__ __forceinline__ void grad_blocks(const HeadGradArgs& A, const Rows& rows) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = (int)threadIdx.x;
    const int L = A.L, H = A.H, O = A.O, R = A.sub, H4 = H / 4;
    const RowImage m = row_image(L, H, O);
    const int RS = m.stride;
    float* w2s = lds + R * RS;
    const long long r0 = (long long)blockIdx.x * mg::kBlockRows, left = A.rows - r0;
    const int nb = left < mg::kBlockRows ? (int)left : mg::kBlockRows;   // (>= 1: the grid has ceil(rows / 256) blocks)
    // this thread's tile: li / rj = its first left / right index, loff / roff = where those sit in a row's image
    const int KT1 = m.ga / 4, JT2 = H4 + 1, T1 = KT1 * H4, T = T1 + ((O + 3) / 4) * JT2;
    const int t = (int)blockIdx.y * kThreads + tid;
    const bool live = t < T, second = live && t >= T1;
    int li = 0, rj = 0, loff = 0, roff = m.ga;
    if (live && !second) {
        li = 4 * (t / H4);
        rj = 4 * (t % H4);
        loff = li;
        roff = m.ga + rj;
    } else if (second) {
        li = 4 * ((t - T1) / JT2);
        rj = 4 * ((t - T1) % JT2);
        loff = m.gy + li;
        roff = m.hid + rj;
    }
    for (int i = tid; i < O * H; i += kThreads) w2s[i] = A.w2[i];
    for (int r = tid; r < R; r += kThreads) {
        lds[r * RS + L] = 1.0f;
        lds[r * RS + m.hid + H] = 1.0f;
    }
    double acc[mg::kTile][mg::kTile] = {};
    for (int s0 = 0; s0 < nb; s0 += R) {
        const int nr = nb - s0 < R ? nb - s0 : R;
        const long long rs = r0 + s0;                                    // the sub-tile's first row: a multiple of 8
        rows.begin(A, rs, nr);
        rows.load(A, lds, m, rs, nr, tid, L, H4, O, RS);
        __syncthreads();
        // 2. ga, four units at a time
        for (int p = tid; p < nr * H4; p += kThreads) {
            const int r = p / H4, j = 4 * (p - r * H4);
            const float* row = lds + r * RS;
            float g[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                g[c] = mg::ga_unit(A.activation, mg::gh_unit(O, row + m.gy, w2s + j + c, H), row[m.hid + j + c]);
            const float4 q = make_float4(g[0], g[1], g[2], g[3]);
            *quad(lds + r * RS + m.ga + j) = q;
            if (A.grad_a && blockIdx.y == 0) reinterpret_cast<float4*>(A.grad_a)[rows.row(rs, r) * H4 + (j >> 2)] = q;
        }
        __syncthreads();
        // 3. the chains: this thread's 16 elements, the sub-tile's rows in ascending order
#pragma unroll 2
        for (int r = 0; r < nr; ++r) {
            const float4 a4 = *quad(lds + r * RS + loff);
            const float4 b4 = *quad(lds + r * RS + roff);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            mg::tile_row(acc, a, b);
        }
        __syncthreads();                                                 // the image may be overwritten
    }
    // the tile's elements: row a, column c of its part is element base + a * pitch + c (ccx_mlp_grad.h: elements_of)
    const int pitch = second ? H + 1 : H, rows_in = second ? O : L + 1;
    const int e0 = (second ? (L + 1) * H : 0) + li * pitch + rj;
#pragma unroll
    for (int i = 0; i < mg::kTile; ++i) {
#pragma unroll
        for (int j = 0; j < mg::kTile; ++j) {
            if (live && li + i < rows_in && rj + j < pitch) A.partials[(long long)(e0 + i * pitch + j) * A.B + blockIdx.x] = acc[i][j];
        }
    }
}


__global__ __launch_bounds__(kThreads) void head_grad_blocks_kernel(const HeadGradArgs A) {
    grad_blocks(A, AdjacentRows{});
}

// the slot group of a ccx_sides_backward call
struct SideSel {
    uint64_t slots;
    int32_t S, N;
    int32_t flat_at;                   // where the flat rows sit in LDS, in floats (behind w2)
};

__global__ __launch_bounds__(kThreads) void sides_grad_blocks_kernel(const HeadGradArgs A, const SideSel G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    grad_blocks(A, PickedRows{G.slots, G.S, G.N, reinterpret_cast<long long*>(lds + G.flat_at)});
}

__global__ __launch_bounds__(kThreads) void head_grad_final_kernel(const HeadGradArgs A) {
    const int lane = (int)(threadIdx.x & 63u);
    const long long e = (long long)blockIdx.x * (kThreads / 64) + (long long)(threadIdx.x >> 6);
    const int L = A.L, H = A.H, O = A.O;
    if (e >= mg::elements_of(L, H, O)) return;                           // (whole waves: e is the same for a wave's lanes)
    double place[1];
    ccx_tree::strided_partials<1>(A.partials + e * A.B, A.B, lane, place);
    const double s = ccx_tree::halve_wave(place[0]);
    if (lane != 0) return;
    const float v = (float)s;
    long long i;
    const int which = mg::place_of(e, L, H, i);
    (which == 0 ? A.grad_w1t : which == 1 ? A.grad_b1 : which == 2 ? A.grad_w2 : A.grad_b2)[i] = v;
}

// the checks and the two launches of both entry points; `sel`: the slot group of ccx_sides_backward (rows = M S), or null
int backward_launches(const char* who, ccx_handle* h, int64_t rows, const SideSel* sel, int32_t L, int32_t H, int32_t O, int32_t activation,
                      const float* x, const float* hidden, const float* grad_y, const float* w2, void* workspace, float* grad_w1t,
                      float* grad_b1, float* grad_w2, float* grad_b2, float* grad_a_or_null) {
    if (!x || !hidden || !grad_y || !w2 || !workspace || !grad_w1t || !grad_b1 || !grad_w2 || !grad_b2)
        return fail(CCX_EINVAL, "%s: NULL argument (only grad_a may be NULL)", who);
    unsigned blocks = 0;
    if (int rc = ccxi::row_blocks(who, rows, mg::kBlockRows, blocks)) return rc;
    if (int rc = ccx_tile::check_dims(who, L, H, O, activation)) return rc;
    if (misaligned(16, x, hidden, grad_a_or_null)) return fail(CCX_EINVAL, "%s: x, hidden and grad_a must be 16-byte aligned", who);
    if (misaligned(8, workspace)) return fail(CCX_EINVAL, "%s: workspace must be 8-byte aligned", who);
    if (misaligned(4, grad_y, w2, grad_w1t, grad_b1, grad_w2, grad_b2))
        return fail(CCX_EINVAL, "%s: grad_y, w2, grad_w1t, grad_b1, grad_w2 and grad_b2 must be 4-byte aligned", who);
    CCX_HIP(hipSetDevice(h->device));
    size_t bytes = 0;
    const int R = mg::sub_rows(L, H, O, bytes, sel ? sizeof(long long) : 0);
    const HeadGradArgs A{x, hidden, grad_y, w2, static_cast<double*>(workspace), grad_w1t, grad_b1, grad_w2, grad_b2, grad_a_or_null,
                         (long long)rows, (long long)blocks, L, H, O, activation, R};
    const RowImage m = row_image(L, H, O);
    const dim3 grid(blocks, mg::grid_y(L, H, O));
    if (sel) {
        SideSel G = *sel;
        G.flat_at = R * m.stride + O * H;                                // (floats; an even number: the stride and H are multiples of 4)
        hipLaunchKernelGGL(sides_grad_blocks_kernel, grid, dim3(kThreads), bytes, h->stream, A, G);
    } else {
        hipLaunchKernelGGL(head_grad_blocks_kernel, grid, dim3(kThreads), bytes, h->stream, A);
    }
    return ccxi::head_grad_final_launch(h, L, H, O, A.partials, A.B, grad_w1t, grad_b1, grad_w2, grad_b2);
}

}  // namespace

// THE launch of head_grad_final_kernel, for the two entry points above and for another unit's block partials in
// ccx_mlp_grad.h's layout (ccx_mlp_wide.hip): the kernel reads the partials, B, the sizes and the four outputs only
int ccxi::head_grad_final_launch(ccx_handle* h, int32_t L, int32_t H, int32_t O, double* partials, long long B, float* grad_w1t,
                                 float* grad_b1, float* grad_w2, float* grad_b2) {
    HeadGradArgs A{};
    A.partials = partials, A.B = B;
    A.grad_w1t = grad_w1t, A.grad_b1 = grad_b1, A.grad_w2 = grad_w2, A.grad_b2 = grad_b2;
    A.L = L, A.H = H, A.O = O;
    const long long elements = mg::elements_of(L, H, O);
    hipLaunchKernelGGL(head_grad_final_kernel, dim3((unsigned)((elements + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0,
                       h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

extern "C" {

int64_t ccx_mlp_backward_workspace_bytes(int64_t rows, int32_t L, int32_t H, int32_t O) { return mg::workspace_bytes(rows, L, H, O); }

int ccx_mlp_backward(ccx_handle* h, int64_t rows, int32_t L, int32_t H, int32_t O, int32_t activation, const float* x,
                     const float* hidden, const float* grad_y, const float* w2, void* workspace, float* grad_w1t, float* grad_b1,
                     float* grad_w2, float* grad_b2, float* grad_a_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    return backward_launches("ccx_mlp_backward", h, rows, nullptr, L, H, O, activation, x, hidden, grad_y, w2, workspace, grad_w1t, grad_b1,
                             grad_w2, grad_b2, grad_a_or_null);
}

int ccx_sides_backward(ccx_handle* h, int64_t M, int32_t N, uint64_t slots, int32_t L, int32_t H, int32_t O, int32_t activation,
                       const float* x, const float* hidden, const float* grad_y, const float* w2, void* workspace, float* grad_w1t,
                       float* grad_b1, float* grad_w2, float* grad_b2, float* grad_a_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (N < 1 || N > 64) return fail(CCX_EINVAL, "ccx_sides_backward: N = %d, 1..64 agent slots are required", N);
    if (M < 1 || M > ((int64_t)1 << 40)) return fail(CCX_EINVAL, "ccx_sides_backward: M = %lld, 1..2^40 env-rows are required", (long long)M);
    int which = 0;
    switch (ccx_sides::check_masks(&slots, 1, N, which)) {
        case 0: break;
        case 2: return fail(CCX_EINVAL, "ccx_sides_backward: the group owns no slot (an empty mask)");
        default: return fail(CCX_EINVAL, "ccx_sides_backward: the mask %#llx has a bit at or above N = %d", (unsigned long long)slots, N);
    }
    const SideSel sel{slots, ccx_sides::popcount(slots), N, 0};
    return backward_launches("ccx_sides_backward", h, M * sel.S, &sel, L, H, O, activation, x, hidden, grad_y, w2, workspace, grad_w1t,
                             grad_b1, grad_w2, grad_b2, grad_a_or_null);
}

}  // extern "C"
