// ccx_render.hip -- batched rgb_array frames of the board (ccx_render / ccx_render_compact, include/ccx.h: CCX_RENDER).
//
// The output [R][H*cp][W*cp][3] is ONE flat stream of pixels.  Each lane draws 16 consecutive pixels (48 bytes = three
// 16-byte stores, streaming cache policy like the observation rows) whatever frame or row they fall in; a workgroup of B
// lanes covers 16 B pixels and stages the agents of the frames it touches in LDS first:
//   - agents[F][N]: (x | y << 8 | type << 16) per slot, 0xffffffff for an agent that is not drawn;
//   - occupied[F][words]: one bit per grid point (W+1)(H+1) with at least one agent on it;
//   - colour[128]: the static layers' colour for each combination of the 7 membership bits (computed by the
//     workgroup from the geometry in ccx_params, not read from memory).
// Every radius is below half a cell, so the only disc centre that can cover a pixel is its nearest grid point: a pixel
// away from every agent costs one bit test, and only the pixels around an occupied point walk that frame's slots.
#include "ccx_internal.h"
#include "ccx_rollout_dev.h"   // store_obs: the streaming 16-byte store

namespace ccx {
namespace {

constexpr int RENDER_PX_PER_LANE = 16;
constexpr int RENDER_LDS_BUDGET = 64 * 1024;
constexpr uint32_t AGENT_NONE = 0xffffffffu;

// membership bits of a pixel (index of the static colour table)
enum : uint32_t { L_TRAM = 1, L_WAIT = 2, L_EXIT = 4, L_SEATS = 8, L_WALL = 16, L_DOOR = 32, L_GRID = 64 };

constexpr uint32_t rgb(uint32_t hex) { return ((hex >> 16) & 255u) | (hex & 0xff00u) | ((hex & 255u) << 16); }

// out = (a src + (255 - a) dst + 127) / 255 per channel, colours packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t blend(uint32_t dst, uint32_t src, uint32_t a) {
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint32_t s = (src >> (8 * ch)) & 255u, d = (dst >> (8 * ch)) & 255u;
        out |= ((a * s + (255u - a) * d + 127u) / 255u) << (8 * ch);
    }
    return out;
}

struct RenderArgs {
    // geometry (ccx_params), frame size
    int32_t W, H, cp, Wpx, Hpx, div, tl, tr, dl, dr, by, ey;
    int32_t N, nb, E, words;     // words: u32 of the occupancy bitmask per frame
    uint32_t frame_px;           // H*cp * W*cp
    int32_t max_frames;          // frames one workgroup can touch (LDS slots)
    int64_t rows, total_px;
    // sources: state (x, y [E][N], env_ids [rows] or null) or compact rows f32 [rows][N][4]
    const int32_t* x;
    const int32_t* y;
    const int32_t* env_ids;
    const float* compact;
    uint8_t* frames;
};

// static colour of the membership bits `m` (layers 1-7, then the grid when L_GRID)
__device__ uint32_t static_colour(uint32_t m) {
    uint32_t c = rgb(0xf8f9fa);
    if (m & L_TRAM) c = blend(c, rgb(0xe3f2fd), 179);
    if (m & L_WAIT) c = blend(c, rgb(0xfff3e0), 179);
    if (m & L_EXIT) c = blend(c, rgb(0xf44336), 204);
    if (m & L_SEATS) c = blend(c, rgb(0x2196f3), 204);
    if (m & L_WALL) c = blend(c, rgb(0x424242), 230);
    if (m & L_DOOR) c = blend(c, rgb(0x90caf9), 204);
    if (m & L_GRID) c = blend(c, rgb(0x808080), 179);
    return c;
}

// the three discs of every agent on grid point (gx, gy) of the frame, in slot order; (dx, dy) in half pixels
__device__ __forceinline__ uint32_t draw_agents(uint32_t c, const uint32_t* agents, int N, uint32_t key, int dx, int dy,
                                             int cp) {
    const int d25 = 25 * (dx * dx + dy * dy);
    for (int a = 0; a < N; ++a) {
        const uint32_t ag = agents[a];
        if ((ag & 0xffffu) != key) continue;
        const bool exiting = (ag >> 16) & 1u;
        const uint32_t face = exiting ? rgb(0x2196f3) : rgb(0xf44336);
        const uint32_t edge = exiting ? rgb(0x00008b) : rgb(0x8b0000);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int k = 4 - i;
            const uint32_t alpha = i == 0 ? 77u : i == 1 ? 128u : 204u;
            const int kc = k * cp;
            if (d25 > kc * kc) continue;
            const bool ring = kc <= 10 || d25 > (kc - 10) * (kc - 10);
            c = blend(c, ring ? edge : face, alpha);
        }
    }
    return c;
}

template <bool COMPACT>
__global__ __launch_bounds__(256) void render_kernel(const RenderArgs A) {
    extern __shared__ uint32_t lds[];
    uint32_t* const colour = lds;                          // [128]
    uint32_t* const occupied = lds + 128;                  // [F][words]
    uint32_t* const agents = occupied + A.max_frames * A.words;   // [F][N]

    const int64_t wg_px = (int64_t)blockDim.x * RENDER_PX_PER_LANE;
    const int64_t px0 = (int64_t)blockIdx.x * wg_px;
    const int64_t px_end = px0 + wg_px < A.total_px ? px0 + wg_px : A.total_px;
    const int64_t f0 = px0 / A.frame_px;
    const int nf = (int)((px_end - 1) / A.frame_px - f0) + 1;     // <= max_frames (host)
    const int tid = threadIdx.x;

    // ---- stage: colour table, empty bitmasks, then the agents of frames f0 .. f0+nf-1
    if (tid < 128) colour[tid] = static_colour(tid);
    for (int i = tid; i < nf * A.words; i += blockDim.x) occupied[i] = 0u;
    __syncthreads();
    for (int i = tid; i < nf * A.N; i += blockDim.x) {
        const int fi = i / A.N, a = i - fi * A.N;
        const int64_t row = f0 + fi;
        uint32_t ag = AGENT_NONE;
        if constexpr (COMPACT) {
            const float* src = A.compact + ((size_t)row * A.N + a) * 4;
            const float fx = src[0], fy = src[1], ft = src[2];
            if (fx >= 0.0f && fx <= (float)A.W && fy >= 0.0f && fy <= (float)A.H)
                ag = (uint32_t)(int)fx | ((uint32_t)(int)fy << 8) | ((ft != 0.0f ? 1u : 0u) << 16);
        } else {
            const int32_t e = A.env_ids ? A.env_ids[row] : (int32_t)row;
            if (e >= 0 && e < A.E) {
                const int32_t ax = A.x[(size_t)e * A.N + a], ay = A.y[(size_t)e * A.N + a];
                if (ax >= 0 && ax <= A.W && ay >= 0 && ay <= A.H)
                    ag = (uint32_t)ax | ((uint32_t)ay << 8) | ((a >= A.nb ? 1u : 0u) << 16);
            }
        }
        agents[fi * A.N + a] = ag;
        if (ag != AGENT_NONE) {
            const uint32_t bit = (ag >> 8 & 255u) * (uint32_t)(A.W + 1) + (ag & 255u);
            atomicOr(&occupied[fi * A.words + (bit >> 5)], 1u << (bit & 31u));
        }
    }
    __syncthreads();

    const int64_t p = px0 + (int64_t)tid * RENDER_PX_PER_LANE;
    if (p >= px_end) return;

    // ---- geometry in half-pixel units: pixel (r, c) has u = 2c + 1 = 2 cp X and v = 2 cp H - 2r - 1 = 2 cp Y
    const int cp = A.cp, S = 2 * cp;
    const int t = max(1, (cp + 5) / 10);                   // wall thickness in pixels: round(cp / 10), at least 1
    const int u_tram0 = S * A.tl, u_tram1 = S * (A.tr + 1);
    const int u_door0 = cp * (2 * A.dl + 1), u_door1 = cp * (2 * A.dr - 1);
    const bool door = A.dr - A.dl - 1 > 0;
    const bool hwall_l = A.dl > A.tl, hwall_r = A.dr < A.tr;
    const int cw_l = min(max(cp * A.tl - t / 2, 0), A.Wpx - t);      // first column of each vertical wall
    const int cw_r = min(max(cp * (A.tr + 1) - t / 2, 0), A.Wpx - t);
    const int rw_h = min(max(cp * (A.H - A.div) - t / 2, 0), A.Hpx - t);   // first row of the horizontal wall
    const int r_tram_end = cp * (A.H - A.div);                       // rows < this lie above division_y
    const bool grid = cp >= 4;
    const int seats_y = A.by == A.H ? A.H - 1 : A.by;

    uint32_t q = (uint32_t)(p - f0 * (int64_t)A.frame_px);
    int fi = (int)(q / A.frame_px);
    q -= (uint32_t)fi * A.frame_px;
    int r = (int)(q / (uint32_t)A.Wpx);
    int c = (int)q - r * A.Wpx;
    const int n_here = px_end - p < RENDER_PX_PER_LANE ? (int)(px_end - p) : RENDER_PX_PER_LANE;

    // per-row state, refreshed when the walk wraps into the next row
    uint32_t row_bits = 0, row_tram = 0, row_seats = 0, row_door = 0;
    bool row_vwall = false, row_hwall = false;
    int gy = 0, dy = 0;
    auto enter_row = [&]() {
        const int v = S * A.H - 2 * r - 1;
        row_bits = (v < S * A.div ? L_WAIT : 0u) | (A.ey < A.div && v >= S * A.ey && v < S * (A.ey + 1) ? L_EXIT : 0u) |
                   (grid && (r % cp == 0 || r == A.Hpx - 1) ? L_GRID : 0u);
        row_tram = v >= S * A.div ? L_TRAM : 0u;
        row_seats = A.by >= A.div && v >= S * seats_y && v < S * (seats_y + 1) ? L_SEATS : 0u;
        row_door = door && v >= S * A.div && v < S * (A.div + 1) ? L_DOOR : 0u;
        row_vwall = r < r_tram_end;
        row_hwall = r >= rw_h && r < rw_h + t;
        gy = (v + cp) / S;
        dy = v - S * gy;
    };
    enter_row();
    int u = 2 * c + 1;
    int gx = (u + cp) / S;
    int gx_rem = u + cp - gx * S;                          // (u + cp) mod S, advanced by 2 per column
    int c_mod = c % cp;                                    // c mod cp (vertical grid lines)

    uint32_t w[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = 0u;
#pragma unroll
    for (int j = 0; j < RENDER_PX_PER_LANE; ++j) {
        uint32_t col = 0;
        if (j < n_here) {
            const uint32_t tram_c = u >= u_tram0 && u < u_tram1 ? ~0u : 0u;
            const bool wall = (row_vwall && ((c >= cw_l && c < cw_l + t) || (c >= cw_r && c < cw_r + t))) ||
                              (row_hwall && ((hwall_l && u >= u_tram0 && u < u_door0) || (hwall_r && u >= u_door1 && u < u_tram1)));
            uint32_t m = row_bits | (row_tram & tram_c) | (row_seats & tram_c) | (wall ? L_WALL : 0u) |
                         (u >= u_door0 && u < u_door1 ? row_door : 0u) | (grid && (c_mod == 0 || c == A.Wpx - 1) ? L_GRID : 0u);
            const uint32_t bit = (uint32_t)gy * (uint32_t)(A.W + 1) + (uint32_t)gx;
            if (occupied[fi * A.words + (bit >> 5)] >> (bit & 31u) & 1u) {
                col = draw_agents(colour[m & ~L_GRID], agents + fi * A.N, A.N, (uint32_t)gx | ((uint32_t)gy << 8),
                                  u - S * gx, dy, cp);
                if (m & L_GRID) col = blend(col, rgb(0x808080), 179);
            } else {
                col = colour[m];
            }
            // next pixel of the stream
            ++c;
            u += 2;
            gx_rem += 2;
            if (gx_rem >= S) { gx_rem -= S; ++gx; }
            if (++c_mod == cp) c_mod = 0;
            if (c == A.Wpx && j + 1 < n_here) {
                c = 0; u = 1; gx = (1 + cp) / S; gx_rem = 1 + cp - gx * S; c_mod = 0;
                if (++r == A.Hpx) { r = 0; ++fi; }
                enter_row();
            }
        }
        // bytes 3j .. 3j+2 of the lane's 48
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int b = 3 * j + ch;
            w[b >> 2] |= ((col >> (8 * ch)) & 255u) << (8 * (b & 3));
        }
    }

    uint8_t* dst = A.frames + (size_t)p * 3;
    if (n_here == RENDER_PX_PER_LANE) {
        v4f* d4 = reinterpret_cast<v4f*>(dst);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t four[4] = {w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
            store_obs(__builtin_bit_cast(v4f, four), d4 + i);
        }
    } else {                                               // the stream's last, partial lane
        for (int b = 0; b < 3 * n_here; ++b) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

}  // namespace
}  // namespace ccx

using ccxi::fail;

static int render_launch(ccx_handle* h, const int32_t* env_ids, const float* compact, int64_t rows, int cell_px,
                         uint8_t* frames) {
    if (!h || !frames) return fail(CCX_EINVAL, "NULL argument");
    if (cell_px < 1 || cell_px > 64) return fail(CCX_EINVAL, "cell_px = %d outside 1..64", cell_px);
    if (rows < 0) return fail(CCX_EINVAL, "rows = %lld < 0", (long long)rows);
    if (ccxi::misaligned(16, frames)) return fail(CCX_EINVAL, "frames must be 16-byte aligned");
    const ccx_params& P = h->params;
    ccx::RenderArgs A{};
    A.W = P.width; A.H = P.height; A.cp = cell_px; A.Wpx = P.width * cell_px; A.Hpx = P.height * cell_px;
    A.div = P.division_y; A.tl = P.tram_left; A.tr = P.tram_right; A.dl = P.door_left; A.dr = P.door_right;
    A.by = P.boarding_dest_y; A.ey = P.exiting_dest_y;
    A.N = h->N; A.nb = P.num_boarding; A.E = h->E;
    A.words = ((P.width + 1) * (P.height + 1) + 31) / 32;
    A.frame_px = (uint32_t)A.Wpx * (uint32_t)A.Hpx;
    A.rows = rows;
    A.total_px = rows * (int64_t)A.frame_px;
    A.x = h->st.x; A.y = h->st.y; A.env_ids = env_ids; A.compact = compact; A.frames = frames;
    if (rows == 0) return CCX_OK;
    // the widest workgroup whose LDS (colour table, bitmask and agent slots of every frame it can touch) fits
    int lanes = 0;
    size_t lds = 0;
    for (int b = 256; b >= 64; b /= 2) {
        const int64_t span = (int64_t)b * ccx::RENDER_PX_PER_LANE;
        int64_t F = (span - 1) / A.frame_px + 2;
        if (F > rows) F = rows;
        lds = (size_t)(128 + F * (A.words + A.N)) * 4u;
        if (lds <= (size_t)ccx::RENDER_LDS_BUDGET) { lanes = b; A.max_frames = (int32_t)F; break; }
    }
    if (!lanes)
        return fail(CCX_EINVAL, "render: %d agents on frames of %u pixels need more LDS than a workgroup has; use a larger cell_px",
                    A.N, A.frame_px);
    const int64_t wg_px = (int64_t)lanes * ccx::RENDER_PX_PER_LANE;
    const int64_t blocks = (A.total_px + wg_px - 1) / wg_px;
    if (blocks > 0x7fffffffLL) return fail(CCX_EINVAL, "render: %lld rows are too many for one launch", (long long)rows);
    CCX_HIP(hipSetDevice(h->device));
    if (compact)
        hipLaunchKernelGGL(ccx::render_kernel<true>, dim3((uint32_t)blocks), dim3(lanes), lds, h->stream, A);
    else
        hipLaunchKernelGGL(ccx::render_kernel<false>, dim3((uint32_t)blocks), dim3(lanes), lds, h->stream, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CCX_EHIP, "render kernel launch failed: %s", hipGetErrorString(e));
    return CCX_OK;
}

extern "C" int ccx_render(ccx_handle* h, const int32_t* env_ids, int64_t rows, int cell_px, uint8_t* frames) {
    if (h && !env_ids && rows != h->E)
        return fail(CCX_EINVAL, "render without env_ids draws all %d envs: rows = %lld", h->E, (long long)rows);
    return render_launch(h, env_ids, nullptr, rows, cell_px, frames);
}

extern "C" int ccx_render_compact(ccx_handle* h, const float* obs_compact, int64_t rows, int cell_px, uint8_t* frames) {
    if (!obs_compact) return fail(CCX_EINVAL, "NULL argument");
    return render_launch(h, nullptr, obs_compact, rows, cell_px, frames);
}
