// Fused AdamW over flat parameter / gradient / moment arenas (vilbert/optimization.py:141-187, correct_bias=True).
//
// The reference issues ~8 ATen kernels for each of 541 parameter tensors per step; here one launch streams the four
// arenas once: 28 bytes per parameter (read p,g,m,v; write p,m,v), the HBM floor for this update.  Tensors the reference
// skips (grad is None: never-used heads, vilbert_init/optimization.py:143-144) are simply absent from the chunk table,
// so they receive neither state nor decay.  Hyper-parameters live in device memory so a captured hipGraph can be
// replayed while the host updates the learning rate.  The data-parallel bf16 gradient exchange adds a form that reads bf16 gradient sums
// (26 bytes per parameter) and the pack pass that rounds the fp32 arena into its send buffer.  Opt-in global gradient-norm clipping adds one
// streaming pass over the gradients (grad_sumsq_kernel: +4 bytes per parameter, +2 over the bf16 sums), one single-workgroup reduction
// (grad_clip_coef_kernel) and an instantiation of the update that reads its gradient scale from the four-float record that reduction wrote.
// Opt-in LAMB layer-wise trust ratio splits the update into two streaming passes around a per-tensor reduction (lamb_stage1_kernel: 24 bytes
// per parameter, lamb_trust_kernel, lamb_stage2_kernel: 16, 18 with the bf16 copy): 40 bytes per parameter against 28.
// Opt-in EMA of the weights keeps a shadow arena with the offsets of the parameter arena: ema_update_kernel is a launch of its own behind the
// update (12 bytes per parameter; fused into the update it would be 8, at the price of a sixth instantiation of the audited kernels), and
// ema_swap_kernel exchanges parameters and shadow for evaluation (16 bytes per parameter, 18 with the bf16 copy).
// Opt-in per-tensor statistics read p and g once more behind the update (tensor_stats_stage1_kernel: 8 bytes per parameter, 6 with bf16
// gradients) and reduce per tensor (tensor_stats_stage2_kernel): norms, maxima and counts of non-finite elements, one row per arena tensor.
#include "common.h"

namespace ytvln {

struct AdamChunk { int64_t off; int64_t len; float wd; float pad; };
static_assert(sizeof(AdamChunk) == 24, "chunk record layout is part of the ABI");

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float b1, float b2, float eps, float ss, float lrwd) {
    m = m * b1 + (1.0f - b1) * g;              // exp_avg.mul_(beta1).add_(1-beta1, grad)            :166
    v = v * b2 + ((1.0f - b2) * g) * g;        // exp_avg_sq.mul_(beta2).addcmul_(1-beta2, grad, grad) :167
    const float denom = sqrtf(v) + eps;        //                                                      :168
    p = p + (-ss) * (m / denom);               // p.addcdiv_(-step_size, exp_avg, denom)               :176
    if (lrwd != 0.f) p = p + (-lrwd) * p;      // p.add_(-lr*wd, p)  -- decay AFTER the update         :186-187
}

// PB != nullptr: the updated parameter is ALSO written as bf16 (round to nearest even) at the same offset of a bf16 arena -- the weight
// operands of the bf16-resident path (BASELINE configs[4]) are refreshed by the optimizer step itself: +2 bytes per parameter, no cast pass.
__device__ __forceinline__ uint32_t bf16_bits(float f) { return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f); }

// The gradient operand: the fp32 arena, or (GT = uint16_t) the bf16 sums of the data-parallel bf16 exchange at the same offsets -- one 8-byte
// load per 4 elements, 26 bytes per parameter instead of 28.  A bf16 value widens exactly, and it is scaled by `gscale` in the same
// expression as an fp32 one: the update is bit-identical to the fp32 kernel fed float(bf16) gradients.
__device__ __forceinline__ float bf16_to_f32(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ float4 load_g4(const float* g, int64_t i) { return reinterpret_cast<const float4*>(g)[i]; }
__device__ __forceinline__ float4 load_g4(const uint16_t* g, int64_t i) {
    const uint2 u = reinterpret_cast<const uint2*>(g)[i];
    return make_float4(bf16_to_f32(u.x & 0xffffu), bf16_to_f32(u.x >> 16), bf16_to_f32(u.y & 0xffffu), bf16_to_f32(u.y >> 16));
}
__device__ __forceinline__ float load_g1(const float* g, int64_t i) { return g[i]; }
__device__ __forceinline__ float load_g1(const uint16_t* g, int64_t i) { return bf16_to_f32(g[i]); }

// The scalar tail of the fp32 instantiation compiles (fp-contract=fast) to the OTHER contraction of the two moment updates than its float4
// body: m = fma(1-b1, g, m*b1), v = fma((1-b2)*g, g, v*b2).  The bf16 instantiation's tail would pick the body's form, so it spells the fp32
// tail out: both forms then agree bit for bit on every element (tests/test_grad_exchange_bf16_gpu.py pins it).
__device__ __forceinline__ void adam1_tail(float& p, float g, float& m, float& v, float b1, float b2, float eps, float ss, float lrwd) {
    m = __builtin_fmaf(1.0f - b1, g, m * b1);
    v = __builtin_fmaf((1.0f - b2) * g, g, v * b2);
    const float denom = sqrtf(v) + eps;
    p = __builtin_fmaf(-ss, m / denom, p);
    if (lrwd != 0.f) p = __builtin_fmaf(-lrwd, p, p);
}

// CLIP (global gradient-norm clipping, ytvln_adamw_clip): `clip` is the device record {norm, coef, skip, skipped} of grad_clip_coef_kernel.
// skip != 0: the whole launch returns before touching p, m, v or the bf16 copy; otherwise the gradient scale is gscale * coef.  A template
// parameter, not a run-time branch: the CLIP = false instantiations never read `clip` and keep the instruction streams they had before it existed.
// With coef == 1 the product is `gscale` itself and everything after it is the same source: the compiler contracts body and tail as in the
// CLIP = false instantiations (the floating-point instruction mix differs by that one multiply), so the update equals theirs bit for bit on
// every element, tails included (tests/test_grad_clip_gpu.py pins it).
template <typename GT, bool CLIP = false>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ P, const GT* __restrict__ G, float* __restrict__ Mo,
                                                    float* __restrict__ Vo, const AdamChunk* __restrict__ chunks,
                                                    const float* __restrict__ hyper, float gscale, uint16_t* __restrict__ PB,
                                                    const float* __restrict__ clip) {
    if constexpr (CLIP) {
        if (clip[2] != 0.f) return;
        gscale *= clip[1];
    }
    const AdamChunk c = chunks[blockIdx.x];
    const float b1 = hyper[0], b2 = hyper[1], eps = hyper[2], ss = hyper[3], lr = hyper[4];
    const float lrwd = lr * c.wd;
    float* p = P + c.off; const GT* g = G + c.off; float* m = Mo + c.off; float* v = Vo + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    for (int64_t i = threadIdx.x; i < n4; i += 256) {
        float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gv = load_g4(g, i);
        adam1(pv.x, gv.x * gscale, mv.x, vv.x, b1, b2, eps, ss, lrwd);
        adam1(pv.y, gv.y * gscale, mv.y, vv.y, b1, b2, eps, ss, lrwd);
        adam1(pv.z, gv.z * gscale, mv.z, vv.z, b1, b2, eps, ss, lrwd);
        adam1(pv.w, gv.w * gscale, mv.w, vv.w, b1, b2, eps, ss, lrwd);
        reinterpret_cast<float4*>(p)[i] = pv; reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
        if (PB) reinterpret_cast<uint2*>(PB + c.off)[i] = make_uint2(bf16_bits(pv.x) | (bf16_bits(pv.y) << 16), bf16_bits(pv.z) | (bf16_bits(pv.w) << 16));
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) {
        if constexpr (sizeof(GT) == sizeof(float)) adam1(p[i], load_g1(g, i) * gscale, m[i], v[i], b1, b2, eps, ss, lrwd);
        else adam1_tail(p[i], load_g1(g, i) * gscale, m[i], v[i], b1, b2, eps, ss, lrwd);
        if (PB) PB[c.off + i] = (uint16_t)bf16_bits(p[i]);
    }
}

// fp32 -> bf16 (round to nearest even, the conversion of bf16_bits) of the gradient arena over an AdamW chunk table: the send buffer of
// the bf16 exchange.  One workgroup per record, as adamw_kernel, so one launch packs exactly what one update launch reads; 16-byte loads,
// 8-byte stores (offsets are multiples of 4 elements: the bf16 side is 8-byte aligned), four loads in flight per thread.  6 bytes per element.
__global__ __launch_bounds__(256) void grad_pack_bf16_kernel(const float* __restrict__ G, uint16_t* __restrict__ GB,
                                                             const AdamChunk* __restrict__ chunks) {
    const AdamChunk c = chunks[blockIdx.x];
    const float* g = G + c.off; uint16_t* o = GB + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    for (int64_t i = threadIdx.x; i < n4; i += 4 * 256) {
        float4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * 256 < n4) x[k] = reinterpret_cast<const float4*>(g)[i + k * 256];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * 256 < n4)
                reinterpret_cast<uint2*>(o)[i + k * 256] = make_uint2(bf16_bits(x[k].x) | (bf16_bits(x[k].y) << 16),
                                                                      bf16_bits(x[k].z) | (bf16_bits(x[k].w) << 16));
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) o[i] = (uint16_t)bf16_bits(g[i]);
}

// Sum of squares of the gradient the update will read (the fp32 arena, or the bf16 sums of the bf16 exchange at the same offsets) over an
// AdamW chunk table: one workgroup per record, one fp32 partial per record, no atomics.  A thread issues its vector loads eight at a time
// and adds the squares into ONE accumulator in element order (a record of 16384 elements: 64 serial terms per thread), then the workgroup
// sums in a fixed tree: six butterfly levels inside each wave, two across the four waves.  Every order is fixed, so a partial is the
// same bits on every run.  Read-only: 4 bytes per element (2 for bf16).
template <typename GT>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const GT* __restrict__ G, const AdamChunk* __restrict__ chunks,
                                                         float* __restrict__ partials) {
    __shared__ float wsum[4];
    const AdamChunk c = chunks[blockIdx.x];
    const GT* g = G + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < n4; i += 8 * 256) {
        float4 x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (i + k * 256 < n4) ? load_g4(g, i + k * 256) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc = __builtin_fmaf(x[k].x, x[k].x, acc); acc = __builtin_fmaf(x[k].y, x[k].y, acc);
            acc = __builtin_fmaf(x[k].z, x[k].z, acc); acc = __builtin_fmaf(x[k].w, x[k].w, acc);
        }
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) { const float x = load_g1(g, i); acc = __builtin_fmaf(x, x, acc); }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One workgroup: Sigma = the sum of all n partials in fp64 (thread t takes t, t + 256, ... in order, then a fixed halving tree through LDS),
// and the record the clip-aware update reads.  The formula and the non-finite behaviour are torch.nn.utils.clip_grad_norm_'s
// (error_if_nonfinite = False): coef = min(1, max_norm / (norm + 1e-6)) in fp32, a NaN norm gives a NaN coefficient, an infinite one 0;
// max_norm = +inf means "measure, do not clip": coef is exactly 1.  clip[3] counts the skipped steps (exact in fp32 up to 2^24).
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, int64_t n, float gscale, float max_norm,
                                                             int skip_nonfinite, float* __restrict__ clip) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += (double)partials[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)((double)gscale * sqrt(s[0]));
        float coef = 1.0f;
        if (max_norm < INFINITY) {
            coef = max_norm / (norm + 1e-6f);
            if (coef > 1.0f) coef = 1.0f;          // (a NaN stays a NaN, as torch.clamp(max=1) leaves it)
        }
        const bool skip = skip_nonfinite && !(fabsf(norm) < INFINITY);
        *reinterpret_cast<float4*>(clip) = make_float4(norm, coef, skip ? 1.0f : 0.0f, clip[3] + (skip ? 1.0f : 0.0f));
    }
}

// ---- LAMB layer-wise trust ratio (You et al., 2020), opt-in: the AdamW direction rescaled per parameter tensor ----------------------------
//   m, v: the moments of adamw_kernel;   r = b * m / (sqrt(v) + eps) + wd * p   (b: the bias correction, hyper[5]; decay INSIDE the direction)
//   trust(tensor) = ||p|| / ||r|| when wd != 0 and both norms are finite and > 0, else 1;   p -= lr * trust * r
// The norms run over whole tensors, so the update is two streaming passes with a per-tensor reduction between them.  r is not stored:
// stage 2 recomputes it from the p it is about to overwrite and the m, v stage 1 stored (storing r would cost the same bytes and a scratch arena).
// Every product-sum is an explicit fma, so the float4 body, the scalar tail and both stages round alike; no atomics, every summation
// order fixed.  `clip` (may be NULL) is the record of grad_clip_coef_kernel: skip != 0 makes all three launches return before writing anything.
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, float b1, float b2) {
    m = __builtin_fmaf(1.0f - b1, g, m * b1);
    v = __builtin_fmaf((1.0f - b2) * g, g, v * b2);
}
__device__ __forceinline__ float lamb_r(float p, float m, float v, float b, float eps, float wd) {
    return __builtin_fmaf(b, m / (sqrtf(v) + eps), wd * p);
}

// Stage 1: one workgroup per chunk record.  Reads p, g, m, v; writes m, v and two fp32 partials per record, {sum p^2, sum r^2}, accumulated as
// in grad_sumsq_kernel: one accumulator per thread and sum in element order (a record of 16384 elements: 64 serial terms), then six
// butterfly levels inside each wave and two across the four waves.  24 bytes per parameter (22 with bf16 gradients).
template <typename GT>
__global__ __launch_bounds__(256) void lamb_stage1_kernel(const float* __restrict__ P, const GT* __restrict__ G, float* __restrict__ Mo,
                                                          float* __restrict__ Vo, const AdamChunk* __restrict__ chunks,
                                                          const float* __restrict__ hyper, float gscale, const float* __restrict__ clip,
                                                          float2* __restrict__ partials) {
    __shared__ float2 wsum[4];
    if (clip) {
        if (clip[2] != 0.f) return;
        gscale *= clip[1];
    }
    const AdamChunk c = chunks[blockIdx.x];
    const float b1 = hyper[0], b2 = hyper[1], eps = hyper[2], b = hyper[5], wd = c.wd;
    const float* p = P + c.off; const GT* g = G + c.off; float* m = Mo + c.off; float* v = Vo + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    float sp = 0.f, sr = 0.f;
    for (int64_t i = threadIdx.x; i < n4; i += 256) {
        const float4 pv = reinterpret_cast<const float4*>(p)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gv = load_g4(g, i);
        lamb_moments(gv.x * gscale, mv.x, vv.x, b1, b2); lamb_moments(gv.y * gscale, mv.y, vv.y, b1, b2);
        lamb_moments(gv.z * gscale, mv.z, vv.z, b1, b2); lamb_moments(gv.w * gscale, mv.w, vv.w, b1, b2);
        reinterpret_cast<float4*>(m)[i] = mv; reinterpret_cast<float4*>(v)[i] = vv;
        const float rx = lamb_r(pv.x, mv.x, vv.x, b, eps, wd), ry = lamb_r(pv.y, mv.y, vv.y, b, eps, wd);
        const float rz = lamb_r(pv.z, mv.z, vv.z, b, eps, wd), rw = lamb_r(pv.w, mv.w, vv.w, b, eps, wd);
        sp = __builtin_fmaf(pv.x, pv.x, sp); sp = __builtin_fmaf(pv.y, pv.y, sp); sp = __builtin_fmaf(pv.z, pv.z, sp); sp = __builtin_fmaf(pv.w, pv.w, sp);
        sr = __builtin_fmaf(rx, rx, sr); sr = __builtin_fmaf(ry, ry, sr); sr = __builtin_fmaf(rz, rz, sr); sr = __builtin_fmaf(rw, rw, sr);
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) {
        const float pi = p[i];
        float mi = m[i], vi = v[i];
        lamb_moments(load_g1(g, i) * gscale, mi, vi, b1, b2);
        m[i] = mi; v[i] = vi;
        const float r = lamb_r(pi, mi, vi, b, eps, wd);
        sp = __builtin_fmaf(pi, pi, sp); sr = __builtin_fmaf(r, r, sr);
    }
    sp = wave_sum(sp); sr = wave_sum(sr);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = make_float2(sp, sr);
    __syncthreads();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = make_float2((wsum[0].x + wsum[1].x) + (wsum[2].x + wsum[3].x), (wsum[0].y + wsum[1].y) + (wsum[2].y + wsum[3].y));
}

// Trust: one wave per tensor of the class.  `first` holds the first record of each tensor (ntensors + 1 entries: the chunks of a tensor are
// contiguous in a class's table), `rec_tensor` the tensor's index in the arena for every record.  Lane l adds the partials of records
// first[t] + l, + 64, ... in order in fp64, then a fixed butterfly over the 64 lanes.  Writes trust[tensor] and the report row
// {||p||, ||r||, trust, 0}.
__global__ __launch_bounds__(64) void lamb_trust_kernel(const float2* __restrict__ partials, const AdamChunk* __restrict__ chunks,
                                                        const int32_t* __restrict__ first, const int32_t* __restrict__ rec_tensor,
                                                        float* __restrict__ trust, float4* __restrict__ report,
                                                        const float* __restrict__ clip) {
    if (clip && clip[2] != 0.f) return;
    const int lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
    if (hi <= lo) return;
    double sp = 0.0, sr = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 64) {
        const float2 x = partials[i];
        sp += (double)x.x; sr += (double)x.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sp += __shfl_xor(sp, o, 64); sr += __shfl_xor(sr, o, 64); }
    if (threadIdx.x == 0) {
        const double np = sqrt(sp), nr = sqrt(sr);
        float t = 1.0f;
        if (chunks[lo].wd != 0.f && np > 0.0 && np < (double)INFINITY && nr > 0.0 && nr < (double)INFINITY) t = (float)(np / nr);
        const int k = rec_tensor[lo];
        trust[k] = t;
        report[k] = make_float4((float)np, (float)nr, t, 0.f);
    }
}

// Stage 2: one workgroup per chunk record.  Reads p and the m, v of stage 1, recomputes r with stage 1's expression on the same values
// (p is still the pre-update one), applies p -= lr * trust * r and writes p, and bf16(p) when PB != nullptr.  16 bytes per parameter, 18
// with the copy.
__global__ __launch_bounds__(256) void lamb_stage2_kernel(float* __restrict__ P, const float* __restrict__ Mo, const float* __restrict__ Vo,
                                                          uint16_t* __restrict__ PB, const AdamChunk* __restrict__ chunks,
                                                          const float* __restrict__ hyper, const float* __restrict__ trust,
                                                          const int32_t* __restrict__ rec_tensor, const float* __restrict__ clip) {
    if (clip && clip[2] != 0.f) return;
    const AdamChunk c = chunks[blockIdx.x];
    const float eps = hyper[2], lr = hyper[4], b = hyper[5], wd = c.wd;
    const float nlt = -(lr * trust[rec_tensor[blockIdx.x]]);
    float* p = P + c.off; const float* m = Mo + c.off; const float* v = Vo + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    for (int64_t i = threadIdx.x; i < n4; i += 256) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 mv = reinterpret_cast<const float4*>(m)[i], vv = reinterpret_cast<const float4*>(v)[i];
        pv.x = __builtin_fmaf(nlt, lamb_r(pv.x, mv.x, vv.x, b, eps, wd), pv.x);
        pv.y = __builtin_fmaf(nlt, lamb_r(pv.y, mv.y, vv.y, b, eps, wd), pv.y);
        pv.z = __builtin_fmaf(nlt, lamb_r(pv.z, mv.z, vv.z, b, eps, wd), pv.z);
        pv.w = __builtin_fmaf(nlt, lamb_r(pv.w, mv.w, vv.w, b, eps, wd), pv.w);
        reinterpret_cast<float4*>(p)[i] = pv;
        if (PB) reinterpret_cast<uint2*>(PB + c.off)[i] = make_uint2(bf16_bits(pv.x) | (bf16_bits(pv.y) << 16), bf16_bits(pv.z) | (bf16_bits(pv.w) << 16));
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) {
        const float pi = __builtin_fmaf(nlt, lamb_r(p[i], m[i], v[i], b, eps, wd), p[i]);
        p[i] = pi;
        if (PB) PB[c.off + i] = (uint16_t)bf16_bits(pi);
    }
}

// ---- EMA of the weights (timm's ModelEmaV2), opt-in: a shadow arena e with the offsets of the parameter arena ------------------------------
//   e = fma(w, p - e, e)      w = hyper[6] = float32(1 - decay), p: the parameter the update launch before this one just wrote
// The lerp form: p == e gives p - e = 0 and fma(w, 0, e) = e, so a parameter that equals its shadow leaves the shadow's bits alone for every w
// (the one exception is the sign of a zero: p = e = -0 gives +0).  The product-sum is an explicit fma, so the float4 body and the scalar
// tail round alike (the hazard adam1 / adam1_tail document).  One workgroup per chunk record, four 16-byte loads of each arena in flight per
// thread as in grad_pack_bf16_kernel; no LDS, no atomics; elements outside the records are not touched.  `clip` (may be NULL) is the record
// of grad_clip_coef_kernel: skip != 0 makes the launch return before writing anything, as the update it follows did.  Reads p, e; writes e:
// 12 bytes per parameter.
__device__ __forceinline__ float ema1(float p, float e, float w) { return __builtin_fmaf(w, p - e, e); }

__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ P, float* __restrict__ E, const AdamChunk* __restrict__ chunks,
                                                         const float* __restrict__ hyper, const float* __restrict__ clip) {
    if (clip && clip[2] != 0.f) return;
    const AdamChunk c = chunks[blockIdx.x];
    const float w = hyper[6];
    const float* p = P + c.off; float* e = E + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    for (int64_t i = threadIdx.x; i < n4; i += 4 * 256) {
        float4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = i + k * 256 < n4;
            x[k] = in ? reinterpret_cast<const float4*>(p)[i + k * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
            y[k] = in ? reinterpret_cast<const float4*>(e)[i + k * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * 256 < n4)
                reinterpret_cast<float4*>(e)[i + k * 256] = make_float4(ema1(x[k].x, y[k].x, w), ema1(x[k].y, y[k].y, w),
                                                                        ema1(x[k].z, y[k].z, w), ema1(x[k].w, y[k].w, w));
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) e[i] = ema1(p[i], e[i], w);
}

// Exchanges p and e element by element over a chunk table (evaluation with the shadow weights: contents move, every view of the arenas
// stays valid); PB != nullptr: bf16(new p), round to nearest even, is written at the same offsets -- the weight operands of the bf16-resident
// path follow the swap in the same pass.  16 bytes per parameter, 18 with the copy.
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ P, float* __restrict__ E, uint16_t* __restrict__ PB,
                                                       const AdamChunk* __restrict__ chunks) {
    const AdamChunk c = chunks[blockIdx.x];
    float* p = P + c.off; float* e = E + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    for (int64_t i = threadIdx.x; i < n4; i += 4 * 256) {
        float4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = i + k * 256 < n4;
            x[k] = in ? reinterpret_cast<const float4*>(p)[i + k * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
            y[k] = in ? reinterpret_cast<const float4*>(e)[i + k * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k * 256 < n4) {
                reinterpret_cast<float4*>(p)[i + k * 256] = y[k];
                reinterpret_cast<float4*>(e)[i + k * 256] = x[k];
                if (PB) reinterpret_cast<uint2*>(PB + c.off)[i + k * 256] = make_uint2(bf16_bits(y[k].x) | (bf16_bits(y[k].y) << 16),
                                                                                     bf16_bits(y[k].z) | (bf16_bits(y[k].w) << 16));
            }
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) {
        const float x = p[i], y = e[i];
        p[i] = y; e[i] = x;
        if (PB) PB[c.off + i] = (uint16_t)bf16_bits(y);
    }
}

// ---- per-tensor gradient / weight statistics, opt-in: which tensor of the arena went non-finite, and how large everything else is ------------
// Two read-only launches per chunk table behind the update (and the EMA): g is the gradient the update read, p the parameter it wrote.
// An element is finite when its exponent field is not all ones; |x| of a finite x is compared as an integer (for non-negative floats the
// integer order of the bits is the order of the values), so a maximum is one of the inputs bit for bit and NaNs need no special case.
// A non-finite element enters the sum as the square of 0 (fma(0, 0, s) == s exactly), the maximum as 0, and is counted.
__device__ __forceinline__ void stat1(float x, float& ss, uint32_t& mx, int& bad) {
    const uint32_t a = __float_as_uint(x) & 0x7fffffffu;
    const bool fin = a < 0x7f800000u;
    const float xf = fin ? x : 0.f;
    ss = __builtin_fmaf(xf, xf, ss);
    mx = max(mx, fin ? a : 0u);
    bad += fin ? 0 : 1;
}
__device__ __forceinline__ void stat4(const float4& x, float& ss, uint32_t& mx, int& bad) {
    stat1(x.x, ss, mx, bad); stat1(x.y, ss, mx, bad); stat1(x.z, ss, mx, bad); stat1(x.w, ss, mx, bad);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Stage 1: one workgroup per chunk record; reads [off, off + len) of p and g and nothing else (8 bytes per parameter, 6 with bf16 gradients).
// Writes per record the four fp32 partials {sum g^2, max |g|, sum p^2, max |p|} over the finite elements and the two int32 counts of
// non-finite elements of g and of p.  The sums are accumulated as in grad_sumsq_kernel: a thread takes the vectors t, t + 256, ... of the
// record (loads issued four of each arena at a time) and adds the squares into ONE fp32 accumulator per sum in element order (a record of
// 16384 elements: 64 serial fmas per thread), then the workgroup sums in a fixed tree: six butterfly levels inside each wave, two across
// the four waves.  Maxima and counts are exact in any order.  No atomics: a partial is the same bits on every run.
template <typename GT>
__global__ __launch_bounds__(256) void tensor_stats_stage1_kernel(const float* __restrict__ P, const GT* __restrict__ G,
                                                                  const AdamChunk* __restrict__ chunks, float4* __restrict__ partials,
                                                                  int2* __restrict__ bad) {
    __shared__ float2 wsum[4];
    __shared__ uint2 wmax[4];
    __shared__ int2 wbad[4];
    const AdamChunk c = chunks[blockIdx.x];
    const float* p = P + c.off; const GT* g = G + c.off;
    const int64_t n4 = ((c.off & 3) == 0) ? (c.len >> 2) : 0;
    float sg = 0.f, sp = 0.f;
    uint32_t mg = 0u, mp = 0u;
    int bg = 0, bp = 0;
    for (int64_t i = threadIdx.x; i < n4; i += 4 * 256) {
        float4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = i + k * 256 < n4;
            x[k] = in ? load_g4(g, i + k * 256) : make_float4(0.f, 0.f, 0.f, 0.f);
            y[k] = in ? reinterpret_cast<const float4*>(p)[i + k * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { stat4(x[k], sg, mg, bg); stat4(y[k], sp, mp, bp); }
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) { stat1(load_g1(g, i), sg, mg, bg); stat1(p[i], sp, mp, bp); }
    sg = wave_sum(sg); sp = wave_sum(sp);
    mg = wave_max_u32(mg); mp = wave_max_u32(mp);
    bg = wave_sum_i32(bg); bp = wave_sum_i32(bp);
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = make_float2(sg, sp); wmax[threadIdx.x >> 6] = make_uint2(mg, mp); wbad[threadIdx.x >> 6] = make_int2(bg, bp);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = make_float4((wsum[0].x + wsum[1].x) + (wsum[2].x + wsum[3].x),
                                           __uint_as_float(max(max(wmax[0].x, wmax[1].x), max(wmax[2].x, wmax[3].x))),
                                           (wsum[0].y + wsum[1].y) + (wsum[2].y + wsum[3].y),
                                           __uint_as_float(max(max(wmax[0].y, wmax[1].y), max(wmax[2].y, wmax[3].y))));
        bad[blockIdx.x] = make_int2((wbad[0].x + wbad[1].x) + (wbad[2].x + wbad[3].x), (wbad[0].y + wbad[1].y) + (wbad[2].y + wbad[3].y));
    }
}

// Stage 2: one wave per tensor of the table, `first` / `rec_tensor` as in lamb_trust_kernel.  Lane l adds the partials of records
// first[t] + l, + 64, ... in order in fp64 and takes their maxima, then a fixed butterfly over the 64 lanes.  Lane 0 writes the tensor's row
// k = rec_tensor[first[t]]: stats[k] = {gscale * sqrt(sum g^2) evaluated in double and rounded once, float(gscale) * max |g| (one fp32
// product), sqrt(sum p^2), max |p|} and counts[k] = {non-finite g, non-finite p, steps so far with a non-finite g}: the third entry is read,
// incremented and written here, as grad_clip_coef_kernel does for clip[3].
__global__ __launch_bounds__(64) void tensor_stats_stage2_kernel(const float4* __restrict__ partials, const int2* __restrict__ bad,
                                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ rec_tensor,
                                                                 float gscale, float4* __restrict__ stats, int64_t* __restrict__ counts) {
    const int lo = first[blockIdx.x], hi = first[blockIdx.x + 1];
    if (hi <= lo) return;
    double sg = 0.0, sp = 0.0;
    uint32_t mg = 0u, mp = 0u;
    long long bg = 0, bp = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 64) {
        const float4 x = partials[i];
        const int2 b = bad[i];
        sg += (double)x.x; sp += (double)x.z;
        mg = max(mg, __float_as_uint(x.y)); mp = max(mp, __float_as_uint(x.w));
        bg += b.x; bp += b.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sg += __shfl_xor(sg, o, 64); sp += __shfl_xor(sp, o, 64);
        bg += __shfl_xor(bg, o, 64); bp += __shfl_xor(bp, o, 64);
    }
    mg = wave_max_u32(mg); mp = wave_max_u32(mp);
    if (threadIdx.x == 0) {
        const int k = rec_tensor[lo];
        stats[k] = make_float4((float)((double)gscale * sqrt(sg)), gscale * __uint_as_float(mg), (float)sqrt(sp), __uint_as_float(mp));
        int64_t* row = counts + 3 * (int64_t)k;
        row[0] = bg; row[1] = bp; row[2] = row[2] + (bg > 0 ? 1 : 0);
    }
}

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_adamw_f32(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* hyper,
                               float grad_scale, void* stream) {
    YT_REQUIRE(p && g && m && v && chunks && hyper, "adamw: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adamw: arenas must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(adamw_kernel<float>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, g, m, v,
                       reinterpret_cast<const AdamChunk*>(chunks), hyper, grad_scale, (uint16_t*)nullptr, (const float*)nullptr);
    YT_LAUNCH_CHECK("adamw");
    return 0;
}

extern "C" int ytvln_adamw_f32_bf16copy(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                                        const float* hyper, float grad_scale, void* stream) {
    YT_REQUIRE(p && g && m && v && p_bf16 && chunks && hyper, "adamw_bf16copy: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)p_bf16) & 15) == 0, "adamw_bf16copy: arenas must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(adamw_kernel<float>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, g, m, v,
                       reinterpret_cast<const AdamChunk*>(chunks), hyper, grad_scale, p_bf16, (const float*)nullptr);
    YT_LAUNCH_CHECK("adamw_bf16copy");
    return 0;
}

extern "C" int ytvln_adamw_f32_gbf16(float* p, const uint16_t* g_bf16, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                                     const float* hyper, float grad_scale, void* stream) {
    YT_REQUIRE(p && g_bf16 && m && v && chunks && hyper, "adamw_gbf16: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g_bf16 | (uintptr_t)m | (uintptr_t)v | (uintptr_t)p_bf16) & 15) == 0,
               "adamw_gbf16: arenas must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(adamw_kernel<uint16_t>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, g_bf16, m, v,
                       reinterpret_cast<const AdamChunk*>(chunks), hyper, grad_scale, p_bf16, (const float*)nullptr);
    YT_LAUNCH_CHECK("adamw_gbf16");
    return 0;
}

extern "C" int ytvln_grad_pack_bf16(const float* g, uint16_t* g_bf16, const void* chunks, int nchunks, void* stream) {
    YT_REQUIRE(g && g_bf16 && chunks, "grad_pack_bf16: null pointer");
    YT_REQUIRE((((uintptr_t)g | (uintptr_t)g_bf16) & 15) == 0, "grad_pack_bf16: arenas must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(grad_pack_bf16_kernel, dim3(nchunks), dim3(256), 0, as_stream(stream), g, g_bf16,
                       reinterpret_cast<const AdamChunk*>(chunks));
    YT_LAUNCH_CHECK("grad_pack_bf16");
    return 0;
}

extern "C" int ytvln_grad_sumsq(const void* g, int dtype, const void* chunks, int nchunks, float* partials, void* stream) {
    YT_REQUIRE(g && chunks && partials, "grad_sumsq: null pointer");
    YT_REQUIRE(dtype == YTVLN_DT_F32 || dtype == YTVLN_DT_BF16, "grad_sumsq: dtype %d (fp32 or bf16 gradients only)", dtype);
    YT_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)partials & 3) == 0, "grad_sumsq: the gradient arena must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    const AdamChunk* ch = reinterpret_cast<const AdamChunk*>(chunks);
    if (dtype == YTVLN_DT_F32)
        hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3(nchunks), dim3(256), 0, as_stream(stream), reinterpret_cast<const float*>(g), ch, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<uint16_t>, dim3(nchunks), dim3(256), 0, as_stream(stream), reinterpret_cast<const uint16_t*>(g), ch,
                           partials);
    YT_LAUNCH_CHECK("grad_sumsq");
    return 0;
}

extern "C" int ytvln_grad_clip_coef(const float* partials, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float* clip,
                                    void* stream) {
    YT_REQUIRE(clip && (partials || n == 0), "grad_clip_coef: null pointer");
    YT_REQUIRE(n >= 0, "grad_clip_coef: n = %lld", (long long)n);
    YT_REQUIRE(((uintptr_t)clip & 15) == 0, "grad_clip_coef: the clip record must be 16-byte aligned");
    YT_REQUIRE(max_norm > 0.f, "grad_clip_coef: max_norm must be > 0 (+inf: no clipping), got %g", (double)max_norm);      // (false for a NaN)
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, n, grad_scale, max_norm, skip_nonfinite, clip);
    YT_LAUNCH_CHECK("grad_clip_coef");
    return 0;
}

extern "C" int ytvln_adamw_clip(float* p, const void* g, int g_dtype, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                                const float* hyper, float grad_scale, const float* clip, void* stream) {
    YT_REQUIRE(p && g && m && v && chunks && hyper && clip, "adamw_clip: null pointer");
    YT_REQUIRE(g_dtype == YTVLN_DT_F32 || g_dtype == YTVLN_DT_BF16, "adamw_clip: g_dtype %d (fp32 or bf16 gradients only)", g_dtype);
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)p_bf16) & 15) == 0,
               "adamw_clip: arenas must be 16-byte aligned");
    if (nchunks <= 0) return 0;
    const AdamChunk* ch = reinterpret_cast<const AdamChunk*>(chunks);
    if (g_dtype == YTVLN_DT_F32)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(adamw_kernel<float, true>), dim3(nchunks), dim3(256), 0, as_stream(stream), p,
                           reinterpret_cast<const float*>(g), m, v, ch, hyper, grad_scale, p_bf16, clip);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(adamw_kernel<uint16_t, true>), dim3(nchunks), dim3(256), 0, as_stream(stream), p,
                           reinterpret_cast<const uint16_t*>(g), m, v, ch, hyper, grad_scale, p_bf16, clip);
    YT_LAUNCH_CHECK("adamw_clip");
    return 0;
}

extern "C" int ytvln_lamb_stage1(const float* p, const void* g, int g_dtype, float* m, float* v, const void* chunks, int nchunks,
                                 const float* hyper, float grad_scale, const float* clip, float* partials, void* stream) {
    YT_REQUIRE(p && g && m && v && chunks && hyper && partials, "lamb_stage1: null pointer");
    YT_REQUIRE(g_dtype == YTVLN_DT_F32 || g_dtype == YTVLN_DT_BF16, "lamb_stage1: g_dtype %d (fp32 or bf16 gradients only)", g_dtype);
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "lamb_stage1: arenas must be 16-byte aligned");
    YT_REQUIRE(((uintptr_t)partials & 7) == 0, "lamb_stage1: the partials must be 8-byte aligned");
    YT_REQUIRE(nchunks >= 0, "lamb_stage1: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    const AdamChunk* ch = reinterpret_cast<const AdamChunk*>(chunks);
    if (g_dtype == YTVLN_DT_F32)
        hipLaunchKernelGGL(lamb_stage1_kernel<float>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, reinterpret_cast<const float*>(g), m, v,
                           ch, hyper, grad_scale, clip, reinterpret_cast<float2*>(partials));
    else
        hipLaunchKernelGGL(lamb_stage1_kernel<uint16_t>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, reinterpret_cast<const uint16_t*>(g),
                           m, v, ch, hyper, grad_scale, clip, reinterpret_cast<float2*>(partials));
    YT_LAUNCH_CHECK("lamb_stage1");
    return 0;
}

extern "C" int ytvln_lamb_trust(const float* partials, const void* chunks, const int32_t* tensor_first, const int32_t* rec_tensor,
                                int ntensors, float* trust, float* report, const float* clip, void* stream) {
    YT_REQUIRE(partials && chunks && tensor_first && rec_tensor && trust && report, "lamb_trust: null pointer");
    YT_REQUIRE(((uintptr_t)partials & 7) == 0 && ((uintptr_t)report & 15) == 0,
               "lamb_trust: the partials must be 8-byte and the report 16-byte aligned");
    YT_REQUIRE(ntensors >= 0, "lamb_trust: ntensors = %d", ntensors);
    if (ntensors == 0) return 0;
    hipLaunchKernelGGL(lamb_trust_kernel, dim3(ntensors), dim3(64), 0, as_stream(stream), reinterpret_cast<const float2*>(partials),
                       reinterpret_cast<const AdamChunk*>(chunks), tensor_first, rec_tensor, trust, reinterpret_cast<float4*>(report), clip);
    YT_LAUNCH_CHECK("lamb_trust");
    return 0;
}

extern "C" int ytvln_lamb_stage2(float* p, const float* m, const float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                                 const float* hyper, const float* trust, const int32_t* rec_tensor, const float* clip, void* stream) {
    YT_REQUIRE(p && m && v && chunks && hyper && trust && rec_tensor, "lamb_stage2: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)p_bf16) & 15) == 0, "lamb_stage2: arenas must be 16-byte aligned");
    YT_REQUIRE(nchunks >= 0, "lamb_stage2: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(lamb_stage2_kernel, dim3(nchunks), dim3(256), 0, as_stream(stream), p, m, v, p_bf16,
                       reinterpret_cast<const AdamChunk*>(chunks), hyper, trust, rec_tensor, clip);
    YT_LAUNCH_CHECK("lamb_stage2");
    return 0;
}

extern "C" int ytvln_ema_update(const float* p, float* e, const void* chunks, int nchunks, const float* hyper, const float* clip, void* stream) {
    YT_REQUIRE(p && e && chunks && hyper, "ema_update: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)e) & 15) == 0, "ema_update: arenas must be 16-byte aligned");
    YT_REQUIRE(nchunks >= 0, "ema_update: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(256), 0, as_stream(stream), p, e, reinterpret_cast<const AdamChunk*>(chunks),
                       hyper, clip);
    YT_LAUNCH_CHECK("ema_update");
    return 0;
}

extern "C" int ytvln_ema_swap(float* p, float* e, uint16_t* p_bf16, const void* chunks, int nchunks, void* stream) {
    YT_REQUIRE(p && e && chunks, "ema_swap: null pointer");
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)e | (uintptr_t)p_bf16) & 15) == 0, "ema_swap: arenas must be 16-byte aligned");
    YT_REQUIRE(nchunks >= 0, "ema_swap: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(256), 0, as_stream(stream), p, e, p_bf16, reinterpret_cast<const AdamChunk*>(chunks));
    YT_LAUNCH_CHECK("ema_swap");
    return 0;
}

extern "C" int ytvln_tensor_stats_stage1(const float* p, const void* g, int g_dtype, const void* chunks, int nchunks, float* partials,
                                         int32_t* bad, void* stream) {
    YT_REQUIRE(p && g && chunks && partials && bad, "tensor_stats_stage1: null pointer");
    YT_REQUIRE(g_dtype == YTVLN_DT_F32 || g_dtype == YTVLN_DT_BF16, "tensor_stats_stage1: g_dtype %d (fp32 or bf16 gradients only)", g_dtype);
    YT_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)partials) & 15) == 0 && ((uintptr_t)bad & 7) == 0,
               "tensor_stats_stage1: the arenas and the partials must be 16-byte, the counts 8-byte aligned");
    YT_REQUIRE(nchunks >= 0, "tensor_stats_stage1: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    const AdamChunk* ch = reinterpret_cast<const AdamChunk*>(chunks);
    if (g_dtype == YTVLN_DT_F32)
        hipLaunchKernelGGL(tensor_stats_stage1_kernel<float>, dim3(nchunks), dim3(256), 0, as_stream(stream), p, reinterpret_cast<const float*>(g),
                           ch, reinterpret_cast<float4*>(partials), reinterpret_cast<int2*>(bad));
    else
        hipLaunchKernelGGL(tensor_stats_stage1_kernel<uint16_t>, dim3(nchunks), dim3(256), 0, as_stream(stream), p,
                           reinterpret_cast<const uint16_t*>(g), ch, reinterpret_cast<float4*>(partials), reinterpret_cast<int2*>(bad));
    YT_LAUNCH_CHECK("tensor_stats_stage1");
    return 0;
}

extern "C" int ytvln_tensor_stats_stage2(const float* partials, const int32_t* bad, const int32_t* tensor_first, const int32_t* rec_tensor,
                                         int ntensors, float grad_scale, float* stats, int64_t* counts, void* stream) {
    YT_REQUIRE(partials && bad && tensor_first && rec_tensor && stats && counts, "tensor_stats_stage2: null pointer");
    YT_REQUIRE((((uintptr_t)partials | (uintptr_t)stats) & 15) == 0 && (((uintptr_t)bad | (uintptr_t)counts) & 7) == 0,
               "tensor_stats_stage2: the partials and the report rows must be 16-byte, both count buffers 8-byte aligned");
    YT_REQUIRE(ntensors >= 0, "tensor_stats_stage2: ntensors = %d", ntensors);
    if (ntensors == 0) return 0;
    hipLaunchKernelGGL(tensor_stats_stage2_kernel, dim3(ntensors), dim3(64), 0, as_stream(stream), reinterpret_cast<const float4*>(partials),
                       reinterpret_cast<const int2*>(bad), tensor_first, rec_tensor, grad_scale, reinterpret_cast<float4*>(stats), counts);
    YT_LAUNCH_CHECK("tensor_stats_stage2");
    return 0;
}
