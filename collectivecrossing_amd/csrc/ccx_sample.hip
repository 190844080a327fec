// ccx_sample.hip -- CCX_SAMPLE (include/ccx.h): masked categorical actions, their log-probabilities and entropies from a
// network's logits, drawn with the library's own counter-based key.
//
// One lane owns one slot (e, a); a wave takes 64 adjacent slots of the flat [E N] index, a workgroup is one wave.  Nothing
// is per env except the two counters of the key (step_count, episode), read once per lane at e = slot / N.
// Loads.  A wave's logits are 1280 contiguous bytes at a lane stride of 20: read as five dwords per lane every load
// instruction would touch 1280 bytes of lines to deliver 256.  Instead the 80 16-byte pieces are loaded whole (lanes 0-63
// one each, lanes 0-15 a second one: two global_load_dwordx4, every byte fetched once), written to LDS as they are, and each
// lane reads back its five dwords at a stride of 5 dwords: 5 is odd, so the 32 lanes of a ds_read_b32 lane group hit 32
// different banks.  There is one path: every load is unconditional at a clamped index (the tail wave's surplus lanes and
// pieces repeat the last valid ones), so all of a lane's loads are in flight before its first wait.  5 E N floats need not
// be a multiple of 4: the up to three floats behind the last whole piece belong to the array's last slot, whose lane
// fetches them as dwords.  logits must be 16-byte aligned.
// Arithmetic.  exp_spec / log_spec, steps 2-6 and the rule of one live slot (sample_slot) are ccx_softmax.h's (shared with
// ccx_evaluate.hip and ccx_mlp.hip): the header's sequences, one f32 operation per line (-ffp-contract=off; `/` is the correctly rounded division, asked for on this unit's compile
// line).  Everything the rule does not read is SELECTED away before any arithmetic: a NaN at an illegal place or in a dead
// slot never reaches a result.
#include "ccx_internal.h"
#include "ccx_softmax.h"

using ccxi::fail;
using ccx_softmax::entropy_spec;
using ccx_softmax::legal_max_d;
using ccx_softmax::log_spec;
using ccx_softmax::sample_slot;
using ccx_softmax::weights;

namespace {

struct SampleArgs {
    const float* logits;
    const uint8_t* masks;              // read only where MASK
    const uint8_t* terminated;
    const uint8_t* truncated;
    const int32_t* step_count;
    const int32_t* episode;
    uint8_t* actions;
    float* logp;                       // STATS: either may be null
    float* entropy;
    long long EN;
    int32_t E;
    uint32_t N, genv0, seed_lo, seed_hi;   // genv0: low word of env_offset; seed_hi already carries kSampleStream
};

template <bool MASK, bool DET, bool STATS>
__global__ __launch_bounds__(64) void sample_kernel(const SampleArgs A) {
    __shared__ float4 pieces[80];
    const uint32_t lane = threadIdx.x;
    const long long slot = (long long)blockIdx.x * 64 + lane;
    const long long sl = slot < A.EN ? slot : A.EN - 1;                 // the tail wave's surplus lanes load what its last slot loads
    // e = slot / N without a 64-bit division: the workgroup index splits as q N + r (one u32 division, wave-uniform), so
    // 64 b = 64 q N + 64 r, and the rest, 64 r + lane < 64 N + 64 <= 4160, is a second u32 division
    const uint32_t bq = blockIdx.x / A.N, br = blockIdx.x - bq * A.N;
    const uint32_t rest = br * 64u + lane, rq = rest / A.N;
    const long long e = (long long)bq * 64 + rq;
    const uint32_t a = rest - rq * A.N;
    // Every load is unconditional, at a clamped index, and issued before the first wait: the small ones, then the wave's
    // pieces.  Piece indices are clamped to the last WHOLE 16-byte piece of the array (5 E N floats need not be a multiple
    // of 4); the up to three floats behind it belong to the array's last slot, which fetches them itself further down.
    const uint8_t term = A.terminated[sl], trunc = A.truncated[sl];
    const uint32_t mbyte = MASK ? (uint32_t)A.masks[sl] : 0x1Fu;
    uint32_t episode = 0, step = 0;
    if (!DET) {
        const long long el = e < A.E ? e : A.E - 1;
        episode = (uint32_t)A.episode[el];
        step = (uint32_t)A.step_count[el];
    }
    const long long floats = A.EN * 5, last_piece = floats / 4 - 1;
    const float4* src = reinterpret_cast<const float4*>(A.logits);
    const long long p0 = (long long)blockIdx.x * 80 + lane, p1 = (long long)blockIdx.x * 80 + 64 + (lane & 15u);
    const float4 v0 = src[p0 < last_piece ? p0 : last_piece];
    const float4 v1 = src[p1 < last_piece ? p1 : last_piece];          // (lanes 16-63 repeat the lines of lanes 0-15)
    pieces[lane] = v0;
    pieces[64 + (lane & 15u)] = v1;                                     // (the four lanes of an address write the same bytes)
    __syncthreads();
    if (slot >= A.EN) return;
    const float* mine = reinterpret_cast<const float*>(pieces) + 5 * lane;
    float l[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) l[k] = mine[k];
    if (slot == A.EN - 1) {                                             // one lane of the launch, and only where 5 E N % 4 != 0
        const int whole = 5 - (int)(floats & 3);
#pragma unroll
        for (int k = 2; k < 5; ++k)
            if (k >= whole) l[k] = A.logits[slot * 5 + k];
    }
    const bool dead = (term | trunc) != 0;
    const uint32_t m = (mbyte & 0x1Fu) | 0x10u;
    uint32_t u = 0;
    if (!DET) u = ccx::random_word(A.seed_lo, A.seed_hi, A.genv0 + (uint32_t)e, episode, step, a);
    uint32_t action;
    float logp = 0.0f, entropy = 0.0f;
    sample_slot<DET, STATS>(l, m, u, STATS && A.logp != nullptr, STATS && A.entropy != nullptr, action, logp, entropy);
    A.actions[slot] = dead ? (uint8_t)CCX_ACTION_ABSENT : (uint8_t)action;
    if (STATS) {
        if (A.logp) A.logp[slot] = dead ? 0.0f : logp;
        if (A.entropy) A.entropy[slot] = dead ? 0.0f : entropy;
    }
}

template <bool MASK, bool DET>
void launch(bool stats, unsigned blocks, hipStream_t stream, const SampleArgs& A) {
    if (stats)
        hipLaunchKernelGGL((sample_kernel<MASK, DET, true>), dim3(blocks), dim3(64), 0, stream, A);
    else
        hipLaunchKernelGGL((sample_kernel<MASK, DET, false>), dim3(blocks), dim3(64), 0, stream, A);
}

}  // namespace

extern "C" {

int ccx_sample_actions(ccx_handle* h, const float* logits, const uint8_t* masks_or_null, int32_t deterministic, uint8_t* actions,
                       float* logp_or_null, float* entropy_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions) return fail(CCX_EINVAL, "ccx_sample_actions: NULL argument (logits and actions are required)");
    if (reinterpret_cast<uintptr_t>(logits) & 15u) return fail(CCX_EINVAL, "ccx_sample_actions: logits must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    SampleArgs A;
    A.logits = logits;
    A.masks = masks_or_null;
    A.terminated = h->st.terminated;
    A.truncated = h->st.truncated;
    A.step_count = h->st.step_count;
    A.episode = h->st.episode;
    A.actions = actions;
    A.logp = logp_or_null;
    A.entropy = entropy_or_null;
    A.EN = (long long)h->E * h->N;
    A.E = h->E;
    A.N = (uint32_t)h->N;
    A.genv0 = (uint32_t)h->env_offset;
    A.seed_lo = h->rng_lo;
    A.seed_hi = h->rng_hi ^ ccx::kSampleStream;
    const unsigned blocks = (unsigned)((A.EN + 63) / 64);               // E < 2^31, N <= 64: below 2^31
    const bool stats = logp_or_null || entropy_or_null, det = deterministic != 0;
    if (masks_or_null) {
        if (det) launch<true, true>(stats, blocks, h->stream, A);
        else launch<true, false>(stats, blocks, h->stream, A);
    } else {
        if (det) launch<false, true>(stats, blocks, h->stream, A);
        else launch<false, false>(stats, blocks, h->stream, A);
    }
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
