// ccx_adam.hip -- CCX_ADAM (include/ccx.h): one optimiser step over up to 32 f32 tensors -- the global gradient norm by
// CCX_PPO_LOSS's fixed f64 tree, the clip scale, and Adam with decoupled weight decay, the step counter and the running
// bias-correction products in 64 bytes of device memory.  The rule is ccx_adam.h; the tree is ccx_tree.h's.
//
// Three plain launches on the handle's stream:
//   adam_partial_kernel   one workgroup of four waves per block of the padded sequence (256 places of ONE tensor).  The block
//                         finds its tensor by a scan of the table's prefix counts (uniform: scalar work), every thread squares
//                         its place's gradient in f64 (a padding place is +0.0), each wave runs the butterfly of a group, lane
//                         0 leaves the group in LDS and thread 0 writes the block's partial to the workspace.
//   adam_final_kernel     ONE wave: the strided adds over the B partials, the butterfly, then lane 0 makes gn, skip, scale and
//                         the bias corrections, advances `state`, and writes `stats` and the call's scalars (the head of the
//                         workspace).
//   adam_update_kernel    the block mapping of the first; it reads the scalars and applies the per-element rule, or, on a
//                         skip, returns on a uniform branch without a store.
// The table travels BY VALUE in the kernel arguments (32 x 40 bytes): a call needs no host-to-device copy, so it captures.
// No workgroup reads a word that another workgroup of the same launch writes: the partials are written by the first launch
// and read by the second, the scalars and `state` are read and written by the one workgroup of the second, and the third
// only reads the scalars; an element of param / m / v is read and written by the one thread that owns it.  That is why the
// final wave is a launch of its own: folded into the update launch, every workgroup would have to redo it from `state`
// while one of them overwrites `state`.  There is no atomic, no last-block-done counter and no grid synchronisation.
#include "ccx_internal.h"
// (the runtime header first: it defines __forceinline__)
#include "ccx_adam.h"

using ccxi::fail;
using ccxi::misaligned;

static_assert(sizeof(ccx_adam::Tensor) == sizeof(ccx_adam_tensor) && sizeof(ccx_adam_tensor) == 40, "the table row is 40 bytes");
static_assert(sizeof(ccx_adam::State) == 64 && sizeof(ccx_adam::Scalars) == 64, "state and scalars are 64 bytes each");
static_assert(ccx_adam::kMaxTensors == CCX_ADAM_MAX_TENSORS, "one limit");

namespace {

struct AdamArgs {
    ccx_adam::Tensor tab[ccx_adam::kMaxTensors];
    int T;
    int has_clip, has_decay;
    float lr, beta1, beta2, eps, weight_decay, max_grad_norm;
    const float* lr_dev;               // or null
    ccx_adam::State* state;
    ccx_adam::Scalars* scalars;        // the head of the workspace
    double* partials;                  // [B], behind the scalars
    float* stats;
    long long B;
};

__global__ __launch_bounds__(256) void adam_partial_kernel(const AdamArgs A) {
    __shared__ double groups[ccx_tree::kBlockGroups];
    int t;
    long long bt;
    ccx_adam::locate(A.tab, A.T, (long long)blockIdx.x, t, bt);
    const long long numel = A.tab[t].numel;
    const float* grad = A.tab[t].grad;
    const long long place = bt * ccx_adam::kBlockPlaces + threadIdx.x;
    const bool exists = place < numel;
    const float g = grad[exists ? place : numel - 1];                   // surplus threads load what the last place loads
    ccx_tree::block_sums(ccx_adam::square_term(exists, g), groups, A.partials);
}

__global__ __launch_bounds__(64) void adam_final_kernel(const AdamArgs A) {
    const double S = ccx_tree::final_sums(A.partials, A.B);
    if (threadIdx.x == 0u) {
        const float lr = A.lr_dev ? A.lr_dev[0] : A.lr;
        ccx_adam::State st = *A.state;
        ccx_adam::Scalars sc{};
        float stats[4];
        ccx_adam::finals(S, lr, A.beta1, A.beta2, A.weight_decay, A.max_grad_norm, st, sc, stats);
        A.state->pow1 = st.pow1;
        A.state->pow2 = st.pow2;
        A.state->step = st.step;
        A.state->skipped = st.skipped;
        *A.scalars = sc;
#pragma unroll
        for (int k = 0; k < 4; ++k) A.stats[k] = stats[k];
    }
}

__global__ __launch_bounds__(256) void adam_update_kernel(const AdamArgs A) {
    const ccx_adam::Scalars sc = *A.scalars;                            // uniform: what the final wave left
    if (sc.skip != 0u) return;                                          // a skipped step stores nothing
    int t;
    long long bt;
    ccx_adam::locate(A.tab, A.T, (long long)blockIdx.x, t, bt);
    const ccx_adam::Tensor X = A.tab[t];
    const long long place = bt * ccx_adam::kBlockPlaces + threadIdx.x;
    if (place >= X.numel) return;
    float p = X.param[place], m = X.m[place], v = X.v[place];
    ccx_adam::update_element(X.grad[place], p, m, v, sc, A.has_clip != 0, A.has_decay != 0, A.beta1, A.beta2, A.eps);
    X.param[place] = p;
    X.m[place] = m;
    X.v[place] = v;
}

bool finite_nonneg(float v) { return v >= 0.0f && v < __builtin_inff(); }                // (false for NaN)

}  // namespace

extern "C" {

int64_t ccx_adam_workspace_bytes(int32_t num_tensors, const int64_t* numel) {
    if (num_tensors < 1 || num_tensors > ccx_adam::kMaxTensors || !numel) return 0;
    int64_t B = 0;
    for (int32_t k = 0; k < num_tensors; ++k) {
        if (numel[k] < 1 || numel[k] > (int64_t)1 << 40) return 0;
        B += ccx_adam::blocks_of(numel[k]);
    }
    return ccx_adam::kScalarBytes + B * (int64_t)sizeof(double);
}

int ccx_adam_step(ccx_handle* h, int32_t num_tensors, const ccx_adam_tensor* tensors, float lr, const float* lr_dev_or_null,
                  float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, void* state, void* workspace,
                  float* stats) {
    if (!h) return fail(CCX_EINVAL, "NULL handle");
    if (!tensors || !state || !workspace || !stats)
        return fail(CCX_EINVAL, "ccx_adam_step: NULL argument (only lr_dev may be NULL)");
    if (num_tensors < 1 || num_tensors > ccx_adam::kMaxTensors)
        return fail(CCX_EINVAL, "ccx_adam_step: num_tensors must lie in 1..%d, got %d", ccx_adam::kMaxTensors, (int)num_tensors);
    if (!(beta1 >= 0.0f && beta1 < 1.0f)) return fail(CCX_EINVAL, "ccx_adam_step: beta1 must lie in [0, 1), got %g", (double)beta1);
    if (!(beta2 >= 0.0f && beta2 < 1.0f)) return fail(CCX_EINVAL, "ccx_adam_step: beta2 must lie in [0, 1), got %g", (double)beta2);
    if (!(eps > 0.0f && eps < __builtin_inff())) return fail(CCX_EINVAL, "ccx_adam_step: eps must be finite and positive, got %g", (double)eps);
    if (!finite_nonneg(lr)) return fail(CCX_EINVAL, "ccx_adam_step: lr must be finite and not negative, got %g", (double)lr);
    if (!finite_nonneg(weight_decay))
        return fail(CCX_EINVAL, "ccx_adam_step: weight_decay must be finite and not negative, got %g", (double)weight_decay);
    if (!finite_nonneg(max_grad_norm))
        return fail(CCX_EINVAL, "ccx_adam_step: max_grad_norm must be finite and not negative, got %g", (double)max_grad_norm);
    AdamArgs A{};
    int64_t B = 0;
    for (int32_t k = 0; k < num_tensors; ++k) {
        const ccx_adam_tensor& x = tensors[k];
        if (!x.param || !x.grad || !x.m || !x.v) return fail(CCX_EINVAL, "ccx_adam_step: tensor %d has a NULL pointer", (int)k);
        if (x.numel < 1 || x.numel > (int64_t)1 << 40)
            return fail(CCX_EINVAL, "ccx_adam_step: tensor %d: numel must lie in 1..2^40, got %lld", (int)k, (long long)x.numel);
        if (misaligned(16, x.param, x.grad, x.m, x.v))
            return fail(CCX_EINVAL, "ccx_adam_step: tensor %d: param, grad, m and v must be 16-byte aligned", (int)k);
        A.tab[k] = ccx_adam::Tensor{x.param, x.grad, x.m, x.v, (long long)x.numel};
        B += ccx_adam::blocks_of(x.numel);
    }
    if (B > 0x7fffffffLL) return fail(CCX_EINVAL, "ccx_adam_step: %lld blocks of 256 elements exceed a grid of 2^31 - 1", (long long)B);
    if (misaligned(8, state, workspace)) return fail(CCX_EINVAL, "ccx_adam_step: state and workspace must be 8-byte aligned");
    if (misaligned(4, stats, lr_dev_or_null)) return fail(CCX_EINVAL, "ccx_adam_step: stats and lr_dev must be 4-byte aligned");
    CCX_HIP(hipSetDevice(h->device));
    A.T = num_tensors;
    A.has_clip = max_grad_norm > 0.0f;
    A.has_decay = weight_decay != 0.0f;
    A.lr = lr;
    A.beta1 = beta1;
    A.beta2 = beta2;
    A.eps = eps;
    A.weight_decay = weight_decay;
    A.max_grad_norm = max_grad_norm;
    A.lr_dev = lr_dev_or_null;
    A.state = static_cast<ccx_adam::State*>(state);
    A.scalars = static_cast<ccx_adam::Scalars*>(workspace);
    A.partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + ccx_adam::kScalarBytes);
    A.stats = stats;
    A.B = B;
    const dim3 grid((unsigned)B);
    hipLaunchKernelGGL(adam_partial_kernel, grid, dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(adam_final_kernel, dim3(1), dim3(64), 0, h->stream, A);
    hipLaunchKernelGGL(adam_update_kernel, grid, dim3(256), 0, h->stream, A);
    CCX_HIP(hipGetLastError());
    return CCX_OK;
}

}  // extern "C"
