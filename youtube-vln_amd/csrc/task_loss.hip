// Loss kernels of the downstream-task heads (VILBertForVLTasks): row-wise soft-target BCE with logits over a matrix of ANY size -- the
// [N, num_labels] answer logits of vil_prediction (VQA: 3129 labels) and the [N, regions] grounding logits of vision_logit -- with the row
// arg-max and the target at it riding along, because the row is being read anyway (the task's score is the sum of those targets).
// ytvln_bce_*_f32 of loss.hip stays what it is: one workgroup over a flat vector of at most 65536 elements, one scalar pos_weight.
//   term(r,c) = (1 - t) x + (1 + (w(c) - 1) t) softplus(-x)          the expression of bce_fwd_kernel, so the two agree on small inputs
//   loss      = scale * sum(term) / (M C)
// fp32 ONLY, on purpose: both producers write fp32 in every precision mode (SimpleClassifier feeds the fp32 GEMM, ops.row_logit writes fp32
// from fp32 or bf16 hidden states), so there is no bf16 instantiation.
// One 256-thread workgroup per row; plain coalesced 4-byte loads (C = 3129 is odd, and at [512, 3129] the loss moves 13 MB: the launches
// cost more than the bytes, so no vector-width special cases).  No atomics; every summation order is fixed by the shapes alone: fp32 per
// thread in column order, six butterfly levels per wave, (w0 + w1) + (w2 + w3) across the waves, then fp64 over the rows -- per thread in
// row order and a fixed LDS tree, as grad_clip_coef_kernel sums its partials.  Two launches on the same inputs give the same bits.
#include "common.h"
#include <limits.h>

namespace ytvln {
namespace {

__device__ __forceinline__ float softplus_neg(float x) { return log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f); }   // log(1 + exp(-x))
__device__ __forceinline__ float pos_w(const float* __restrict__ pw, int pw_stride, int c) { return pw ? pw[(int64_t)c * pw_stride] : 1.f; }

// the larger logit wins, the LOWER column among equals (torch.argmax's tie rule); a NaN never compares true and is passed over
__device__ __forceinline__ void top_push(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__global__ __launch_bounds__(256) void bce_rows_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ t, int64_t ldt,
                                                           const float* __restrict__ pw, int pw_stride, float* __restrict__ row_loss,
                                                           float* __restrict__ row_hit, int64_t* __restrict__ row_top, int C) {
    __shared__ float sh_s[4], sh_v[4];
    __shared__ int sh_i[4];
    const int row = blockIdx.x;
    const float* xr = x + (int64_t)row * ldx;
    const float* tr = t + (int64_t)row * ldt;
    float acc = 0.f, bv = -INFINITY;
    int bi = INT_MAX;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float xv = xr[c], tv = tr[c];
        const float lw = 1.f + (pos_w(pw, pw_stride, c) - 1.f) * tv;
        acc += (1.f - tv) * xv + lw * softplus_neg(xv);
        top_push(bv, bi, xv, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        top_push(bv, bi, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) { sh_s[threadIdx.x >> 6] = acc; sh_v[threadIdx.x >> 6] = bv; sh_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) top_push(bv, bi, sh_v[w], sh_i[w]);
        if (bi >= C) bi = 0;          // a row without a single comparable logit (all NaN): unspecified by contract, but never out of bounds
        row_loss[row] = (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]);
        row_top[row] = bi;
        row_hit[row] = tr[bi];
    }
}

// out[0] = float(sum(row_loss) * scale / count), out[1] = float(sum(row_hit)): both sums in fp64
__global__ __launch_bounds__(256) void bce_rows_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_hit, int M,
                                                                double scale_over_count, float* __restrict__ out) {
    __shared__ double s[256], h[256];
    double a = 0.0, b = 0.0;
    for (int r = threadIdx.x; r < M; r += 256) { a += (double)row_loss[r]; b += (double)row_hit[r]; }
    s[threadIdx.x] = a; h[threadIdx.x] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { s[threadIdx.x] += s[threadIdx.x + w]; h[threadIdx.x] += h[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = (float)(s[0] * scale_over_count); out[1] = (float)h[0]; }
}

// columns [0, C) only, like ce_bwd_kernel<float>: the caller owns the padding of a wider dx
__global__ __launch_bounds__(256) void bce_rows_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ t, int64_t ldt,
                                                           const float* __restrict__ pw, int pw_stride, float scale_over_count,
                                                           const float* __restrict__ gout, float* __restrict__ dx, int64_t lddx, int C) {
    const int row = blockIdx.x;
    const float* xr = x + (int64_t)row * ldx;
    const float* tr = t + (int64_t)row * ldt;
    float* dr = dx + (int64_t)row * lddx;
    const float coef = gout[0] * scale_over_count;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float xv = xr[c], tv = tr[c];
        const float lw = 1.f + (pos_w(pw, pw_stride, c) - 1.f) * tv;
        const float sg = 1.f / (1.f + expf(xv));   // sigmoid(-x)
        dr[c] = ((1.f - tv) - lw * sg) * coef;
    }
}

inline bool finite_f(float v) { return fabsf(v) < INFINITY; }          // false for a NaN

}  // namespace
}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_bce_rows_fwd_f32(const float* x, int64_t ldx, const float* t, int64_t ldt, const float* pos_weight, int pw_stride,
                                      float scale, float* row_loss, float* row_hit, int64_t* row_top, float* out, int M, int C,
                                      void* stream) {
    YT_REQUIRE(x && t && row_loss && row_hit && row_top && out, "bce_rows_fwd: null pointer");
    YT_REQUIRE(M > 0 && C > 0, "bce_rows_fwd: M = %d, C = %d", M, C);
    YT_REQUIRE(ldx >= C && ldt >= C, "bce_rows_fwd: leading dimension below C = %d (ldx %lld, ldt %lld)", C, (long long)ldx, (long long)ldt);
    YT_REQUIRE(pw_stride == 0 || pw_stride == 1, "bce_rows_fwd: pw_stride %d (0: one scalar, 1: one weight per class)", pw_stride);
    YT_REQUIRE(finite_f(scale), "bce_rows_fwd: scale must be finite, got %g", (double)scale);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(bce_rows_fwd_kernel, dim3(M), dim3(256), 0, s, x, ldx, t, ldt, pos_weight, pw_stride, row_loss, row_hit, row_top, C);
    hipLaunchKernelGGL(bce_rows_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, row_hit, M, (double)scale / ((double)M * (double)C), out);
    YT_LAUNCH_CHECK("bce_rows_fwd");
    return 0;
}

extern "C" int ytvln_bce_rows_bwd_f32(const float* x, int64_t ldx, const float* t, int64_t ldt, const float* pos_weight, int pw_stride,
                                      float scale, const float* gout, float* dx, int64_t lddx, int M, int C, void* stream) {
    YT_REQUIRE(x && t && gout && dx, "bce_rows_bwd: null pointer");
    YT_REQUIRE(M > 0 && C > 0, "bce_rows_bwd: M = %d, C = %d", M, C);
    YT_REQUIRE(ldx >= C && ldt >= C && lddx >= C, "bce_rows_bwd: leading dimension below C = %d (ldx %lld, ldt %lld, lddx %lld)", C,
               (long long)ldx, (long long)ldt, (long long)lddx);
    YT_REQUIRE(pw_stride == 0 || pw_stride == 1, "bce_rows_bwd: pw_stride %d (0: one scalar, 1: one weight per class)", pw_stride);
    YT_REQUIRE(finite_f(scale), "bce_rows_bwd: scale must be finite, got %g", (double)scale);
    hipLaunchKernelGGL(bce_rows_bwd_kernel, dim3(M), dim3(256), 0, as_stream(stream), x, ldx, t, ldt, pos_weight, pw_stride,
                       (float)((double)scale / ((double)M * (double)C)), gout, dx, lddx, C);
    YT_LAUNCH_CHECK("bce_rows_bwd");
    return 0;
}
