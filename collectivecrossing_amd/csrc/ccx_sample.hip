// ccx_sample.hip -- CCX_SAMPLE (include/ccx.h): masked categorical actions, their log-probabilities and entropies from a
// network's logits, drawn with the library's own counter-based key.
//
// One lane owns one slot (e, a); a wave takes 64 adjacent slots of the flat [E N] index, a workgroup is one wave.  The slot
// rule -- (e, a) of a slot, its small loads, its key, what a dead slot gets -- is ccx_draw.h's (shared with ccx_mlp.hip); the
// logits come through ccx_rows.h's load_rows, where the LDS scheme is explained.  logits must be 16-byte aligned.
// Arithmetic.  exp_spec / log_spec, steps 2-6 and the rule of one live slot (sample_slot) are ccx_softmax.h's (shared with
// ccx_evaluate.hip and ccx_mlp.hip): the header's sequences, one f32 operation per line (-ffp-contract=off; `/` is the correctly rounded division, asked for on this unit's compile
// line).  Everything the rule does not read is SELECTED away before any arithmetic: a NaN at an illegal place or in a dead
// slot never reaches a result.
#include "ccx_draw.h"
#include "ccx_rows.h"

using ccx_draw::DrawArgs;
using ccxi::fail;
using ccxi::misaligned;
using ccxi::with_flags;

namespace {

template <bool MASK, bool DET, bool STATS>
__global__ __launch_bounds__(64) void sample_kernel(const float* logits, const DrawArgs D) {
    __shared__ float4 pieces[80];
    const uint32_t lane = threadIdx.x;
    const ccx_draw::Slot s = ccx_draw::slot_of(D, lane);
    // every load is issued before the first wait: the small ones, then the wave's pieces
    const ccx_draw::Small v = ccx_draw::small_loads<DET>(D, s, MASK);
    const ccx_rows::Wave W = ccx_rows::wave_of(D.EN, blockIdx.x, lane);  // (W.row is s.slot; the small loads clamp for themselves)
    float l[5];
    ccx_rows::load_rows(logits, pieces, W, l);
    if (s.slot >= D.EN) return;
    ccx_draw::finish<DET, STATS>(D, s, v, l);
}

}  // namespace

extern "C" {

int ccx_sample_actions(ccx_handle* h, const float* logits, const uint8_t* masks_or_null, int32_t deterministic, uint8_t* actions,
                       float* logp_or_null, float* entropy_or_null) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!logits || !actions) return fail(CCX_EINVAL, "ccx_sample_actions: NULL argument (logits and actions are required)");
    if (misaligned(16, logits)) return fail(CCX_EINVAL, "ccx_sample_actions: logits must be 16-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    const DrawArgs D = ccx_draw::draw_args(h, masks_or_null, actions, logp_or_null, entropy_or_null);
    const unsigned blocks = (unsigned)((D.EN + 63) / 64);               // E < 2^31, N <= 64: below 2^31
    with_flags([&](auto mask, auto det, auto stats) {
        hipLaunchKernelGGL((sample_kernel<decltype(mask)::value, decltype(det)::value, decltype(stats)::value>), dim3(blocks),
                           dim3(64), 0, h->stream, logits, D);
    }, masks_or_null != nullptr, deterministic != 0, logp_or_null || entropy_or_null);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
