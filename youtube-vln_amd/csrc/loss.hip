// Loss kernels of the pre-training / fine-tuning loops (utils/utils_init.py:108-164): ignore-index cross entropy over the
// 30522-way language logits (and the K-way ranking logits with -inf padding), the masked KL of the 1601-way vision head and
// the pos-weighted BCE of the trajectory head.  One workgroup per row streams the row once (online log-sum-exp); the
// scalar reduction is a fixed-order single-workgroup pass, so results are run-to-run deterministic and need no host sync
// (the reference calls .item() here, utils_init.py:127).
#include "common.h"
#include <algorithm>
#include <limits.h>

namespace ytvln {

struct MS { float m, s; };
__device__ __forceinline__ MS ms_combine(MS a, MS b) {
    const float m = fmaxf(a.m, b.m);
    if (m == -INFINITY) return {m, 0.f};
    return {m, a.s * expf(a.m - m) + b.s * expf(b.m - m)};
}
__device__ __forceinline__ MS ms_push(MS a, float x) {
    if (x == -INFINITY) return a;
    if (x <= a.m) return {a.m, a.s + expf(x - a.m)};
    return {x, a.s * expf(a.m - x) + 1.0f};
}
// logits are fp32, or bf16 on the bf16-resident path (BASELINE configs[4]: the decoders write bf16 logits, the gradient goes back as bf16)
__device__ __forceinline__ float lget(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float lget(const uint16_t* p, int64_t i) { return __uint_as_float((uint32_t)p[i] << 16); }

// block-wide (256 threads) log-sum-exp of a row; result valid in all threads
template <typename LT>
__device__ __forceinline__ float block_lse(const LT* __restrict__ row, int V, float* sh /* [8] */) {
    MS a = {-INFINITY, 0.f};
    for (int c = threadIdx.x; c < V; c += 256) a = ms_push(a, lget(row, c));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MS b = {__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)};
        a = ms_combine(a, b);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh[2 * w] = a.m; sh[2 * w + 1] = a.s; }
    __syncthreads();
    MS r = {sh[0], sh[1]};
#pragma unroll
    for (int i = 1; i < 4; ++i) r = ms_combine(r, MS{sh[2 * i], sh[2 * i + 1]});
    return r.m + logf(r.s);
}
__device__ __forceinline__ float block_sum(float v, float* sh /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <typename LT>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const LT* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                     int64_t ignore, float* __restrict__ row_lse, float* __restrict__ row_loss, int V) {
    __shared__ float sh[8];
    const int row = blockIdx.x;
    const int64_t t = target[row];
    if (t == ignore) {          // ~85 % of the masked-LM rows: their loss is 0 and ce_bwd_kernel never reads their log-sum-exp (block-uniform exit)
        if (threadIdx.x == 0) { row_lse[row] = 0.f; row_loss[row] = 0.f; }
        return;
    }
    const LT* x = logits + (int64_t)row * ld;
    const float lse = block_lse(x, V, sh);
    if (threadIdx.x == 0) {
        row_lse[row] = lse;
        // a target outside [0, V) that is not the ignore index (torch's kernel asserts): never read out of bounds, poison the loss
        row_loss[row] = (t == ignore) ? 0.f : (t >= 0 && t < V) ? lse - lget(x, t) : NAN;
    }
}

// out[0] = sum(row_loss) / count, out[1] = count, count = #(target != ignore)  (0/0 = NaN like F.cross_entropy)
__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ target,
                                                          int64_t ignore, int M, float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) { s += row_loss[r]; c += (target[r] != ignore) ? 1.f : 0.f; }
    const float S = block_sum(s, sh);
    const float C = block_sum(c, sh);
    if (threadIdx.x == 0) { out[0] = S / C; out[1] = C; }
}

// DT = float: fp32 logits, fp32 gradient (columns [0, V)).  DT = uint16_t: the bf16-resident path -- bf16 logits, the gradient rounded to bf16
// (RNE) AND zeros in the padding columns [V, ldd), so that the buffer feeds the bf16 GEMMs as a zero-padded operand (YTVLN_GEMM_A_ZERO_PADDED).
__device__ __forceinline__ void grad_store(float* d, int c, float v) { d[c] = v; }
__device__ __forceinline__ void grad_store(uint16_t* d, int c, float v) { d[c] = __builtin_bit_cast(uint16_t, (__bf16)v); }

template <typename DT>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const DT* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                     int64_t ignore, const float* __restrict__ row_lse, const float* __restrict__ out,
                                                     const float* __restrict__ gout, DT* __restrict__ dl, int64_t ldd, int V) {
    const int row = blockIdx.x;
    const int64_t t = target[row];
    DT* d = dl + (int64_t)row * ldd;
    const int Vz = sizeof(DT) == 2 ? (int)ldd : V;          // bf16: the padding is zeroed too
    if (t == ignore) {
        for (int c = threadIdx.x; c < Vz; c += 256) grad_store(d, c, 0.f);
        return;
    }
    const float coef = gout[0] / out[1], lse = row_lse[row];
    const DT* x = logits + (int64_t)row * ld;
    for (int c = threadIdx.x; c < V; c += 256) grad_store(d, c, (expf(lget(x, c) - lse) - (c == t ? 1.f : 0.f)) * coef);
    for (int c = V + threadIdx.x; c < Vz; c += 256) grad_store(d, c, 0.f);
}

template <typename LT>
__global__ __launch_bounds__(256) void kl_fwd_kernel(const LT* __restrict__ pred, int64_t ld, const float* __restrict__ tgt, int64_t ldt,
                                                     const int64_t* __restrict__ mask, float* __restrict__ row_lse,
                                                     float* __restrict__ row_loss, int C) {
    __shared__ float sh[8];
    const int row = blockIdx.x;
    if (mask[row] == 0) {
        if (threadIdx.x == 0) { row_lse[row] = 0.f; row_loss[row] = 0.f; }
        return;
    }
    const LT* x = pred + (int64_t)row * ld;
    const float* t = tgt + (int64_t)row * ldt;
    const float lse = block_lse(x, C, sh);
    float acc = 0.f;   // sum_c t * (log t - (x - lse)), 0 where t == 0 (xlogy semantics of F.kl_div)
    for (int c = threadIdx.x; c < C; c += 256) {
        const float tv = t[c];
        if (tv > 0.f) acc += tv * (logf(tv) - (lget(x, c) - lse));
    }
    const float tot = block_sum(acc, sh) * (float)mask[row];
    if (threadIdx.x == 0) { row_lse[row] = lse; row_loss[row] = tot; }
}

// out[0] = sum(row_loss) / max(1, sum(mask)), out[1] = max(1, sum(mask))   (utils_init.py:126-128)
__global__ __launch_bounds__(256) void kl_finalize_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ mask, int M,
                                                          float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) { s += row_loss[r]; c += (float)mask[r]; }
    const float S = block_sum(s, sh);
    const float Cn = fmaxf(1.f, block_sum(c, sh));
    if (threadIdx.x == 0) { out[0] = S / Cn; out[1] = Cn; }
}

template <typename DT>
__global__ __launch_bounds__(256) void kl_bwd_kernel(const DT* __restrict__ pred, int64_t ld, const float* __restrict__ tgt, int64_t ldt,
                                                     const int64_t* __restrict__ mask, const float* __restrict__ row_lse,
                                                     const float* __restrict__ out, const float* __restrict__ gout,
                                                     DT* __restrict__ dp, int64_t ldd, int C) {
    __shared__ float sh[4];
    const int row = blockIdx.x;
    DT* d = dp + (int64_t)row * ldd;
    const int Cz = sizeof(DT) == 2 ? (int)ldd : C;
    if (mask[row] == 0) {
        for (int c = threadIdx.x; c < Cz; c += 256) grad_store(d, c, 0.f);
        return;
    }
    const DT* x = pred + (int64_t)row * ld;
    const float* t = tgt + (int64_t)row * ldt;
    float ts = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) ts += t[c];
    const float tsum = block_sum(ts, sh);
    const float coef = gout[0] / out[1] * (float)mask[row], lse = row_lse[row];
    for (int c = threadIdx.x; c < C; c += 256) grad_store(d, c, coef * (expf(lget(x, c) - lse) * tsum - t[c]));
    for (int c = C + threadIdx.x; c < Cz; c += 256) grad_store(d, c, 0.f);
}

__device__ __forceinline__ float softplus_neg(float x) { return log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f); }   // log(1+exp(-x))

__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ pw,
                                                      float* __restrict__ out, int n) {
    __shared__ float sh[4];
    const float w = pw ? pw[0] : 1.f;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float lw = 1.f + (w - 1.f) * t[i];
        acc += (1.f - t[i]) * x[i] + lw * softplus_neg(x[i]);
    }
    const float S = block_sum(acc, sh);
    if (threadIdx.x == 0) out[0] = S / (float)n;
}

__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ pw,
                                                      const float* __restrict__ gout, float* __restrict__ dx, int n) {
    const float w = pw ? pw[0] : 1.f, coef = gout[0] / (float)n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float lw = 1.f + (w - 1.f) * t[i];
        const float sg = 1.f / (1.f + expf(x[i]));   // sigmoid(-x)
        dx[i] = ((1.f - t[i]) - lw * sg) * coef;
    }
}

// ---- stats forms: label smoothing and the row arg-max from the pass that computes the log-sum-exp ------------------------------------------
// The arg-max is a total order, so the reduction tree cannot change it: a NaN beats every number (torch.argmax / np.argmax), then the larger
// value wins, then the LOWER column among equals.
struct Top { float v; int i; };
__device__ __forceinline__ void top_push(Top& b, float v, int i) {          // selects, no branches
    const bool vn = v != v, bn = b.v != b.v, lower = i < b.i;
    const bool first = (vn & !bn) | ((vn == bn) & (vn ? lower : ((v > b.v) | ((v == b.v) & lower))));
    b.v = first ? v : b.v;
    b.i = first ? i : b.i;
}
// The same order for one thread's own columns, which come in ascending order: a later column wins only when strictly greater, and the first
// NaN is remembered beside the running maximum.  Starts from {-inf, the thread's first column}, so a row of -inf answers column 0.
__device__ __forceinline__ void scan_push(Top& b, int& nan_i, float x, int c) {
    const bool gt = x > b.v;
    b.v = gt ? x : b.v;
    b.i = gt ? c : b.i;
    nan_i = min(nan_i, x != x ? c : INT_MAX);
}
__device__ __forceinline__ Top scan_done(Top b, int nan_i) { return nan_i != INT_MAX ? Top{NAN, nan_i} : b; }
// ms_push / ms_combine with every rounding spelled out.  Whether `a.s * ea + b.s * eb` becomes two products and a sum, or an fma over one of
// the products, is the compiler's choice per call site, and the stats forms promise block_lse's BITS (label_smoothing = 0 and token_accuracy
// change no bit of a step).  block_lse's sites compile, in all four instantiations, to: fma in ms_push; both products rounded in the six
// butterfly levels and in the first combine of the four-wave chain; fma over a's product in the second; fma over b's product in the third.
// These say so explicitly (contraction off, the fma by name); tests/test_loss_stats_gpu.py holds the two to each other bit for bit.
enum { ROUND_BOTH = 0, FMA_A = 1, FMA_B = 2 };
__device__ __forceinline__ MS ms_push_as(MS a, float x) {
#pragma clang fp contract(off)
    if (x == -INFINITY) return a;
    if (x <= a.m) return {a.m, a.s + expf(x - a.m)};
    return {x, __builtin_fmaf(a.s, expf(a.m - x), 1.0f)};
}
template <int FORM>
__device__ __forceinline__ MS ms_combine_as(MS a, MS b) {
#pragma clang fp contract(off)
    const float m = fmaxf(a.m, b.m);
    if (m == -INFINITY) return {m, 0.f};
    const float ea = expf(a.m - m), eb = expf(b.m - m);
    if (FORM == FMA_A) return {m, __builtin_fmaf(a.s, ea, b.s * eb)};
    if (FORM == FMA_B) return {m, __builtin_fmaf(b.s, eb, a.s * ea)};
    return {m, a.s * ea + b.s * eb};
}

struct ScanShared { float m[4], s[4], sx[4], tv[4]; int nv[4], ti[4]; };
struct RowScan { float lse, sx, nv; Top top; };

// block-wide arg-max; result valid in all threads
__device__ __forceinline__ Top block_top(Top b, ScanShared* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top_push(b, __shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh->tv[threadIdx.x >> 6] = b.v; sh->ti[threadIdx.x >> 6] = b.i; }
    __syncthreads();
    Top r = {sh->tv[0], sh->ti[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) top_push(r, sh->tv[w], sh->ti[w]);
    return r;
}

// One pass over a row: the log-sum-exp in block_lse's order (same per-thread columns, same butterfly, same four-wave chain: same bits), the
// arg-max, and with SUM the sum and the number of the logits that are not -inf.  Valid in all threads.
template <bool SUM, typename LT>
__device__ __forceinline__ RowScan row_scan(const LT* __restrict__ row, int V, ScanShared* sh) {
    MS a = {-INFINITY, 0.f};
    Top b = {-INFINITY, (int)threadIdx.x};
    float sx = 0.f;
    int nv = 0, nan_i = INT_MAX;
    for (int c = threadIdx.x; c < V; c += 256) {
        const float x = lget(row, c);
        a = ms_push_as(a, x);
        scan_push(b, nan_i, x, c);
        if (SUM) { const bool fin = x != -INFINITY; sx += fin ? x : 0.f; nv += fin ? 1 : 0; }
    }
    b = scan_done(b, nan_i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MS o2 = {__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)};
        a = ms_combine_as<ROUND_BOTH>(a, o2);
        top_push(b, __shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64));
        if (SUM) { sx += __shfl_xor(sx, o, 64); nv += __shfl_xor(nv, o, 64); }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh->m[w] = a.m; sh->s[w] = a.s; sh->sx[w] = sx; sh->nv[w] = nv; sh->tv[w] = b.v; sh->ti[w] = b.i; }
    __syncthreads();
    MS r = {sh->m[0], sh->s[0]};
    r = ms_combine_as<ROUND_BOTH>(r, MS{sh->m[1], sh->s[1]});
    r = ms_combine_as<FMA_A>(r, MS{sh->m[2], sh->s[2]});
    r = ms_combine_as<FMA_B>(r, MS{sh->m[3], sh->s[3]});
    Top t = {sh->tv[0], sh->ti[0]};
#pragma unroll
    for (int i = 1; i < 4; ++i) top_push(t, sh->tv[i], sh->ti[i]);
    RowScan out;
    out.lse = r.m + logf(r.s);
    out.sx = SUM ? (sh->sx[0] + sh->sx[1]) + (sh->sx[2] + sh->sx[3]) : 0.f;
    out.nv = SUM ? (float)((sh->nv[0] + sh->nv[1]) + (sh->nv[2] + sh->nv[3])) : 0.f;
    out.top = t;
    return out;
}

// row loss = (1 - eps) (lse - x[t]) + eps (lse - sx / nv): F.cross_entropy(label_smoothing = eps) with the smoothing mass spread over the
// classes that are not -inf (torch spreads it over all V and returns +inf for a -inf padded row).  eps == 0 takes lse - x[t] itself, the bits
// of ce_fwd_kernel.  A row that holds a NaN is poisoned whatever its width (the lse chain alone can lose a NaN next to an empty thread).
template <typename LT>
__global__ __launch_bounds__(256) void ce_stats_fwd_kernel(const LT* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                           int64_t ignore, float eps, float* __restrict__ row_lse, float* __restrict__ row_nv,
                                                           float* __restrict__ row_loss, int64_t* __restrict__ row_top, int V) {
    __shared__ ScanShared sh;
    const int row = blockIdx.x;
    const int64_t t = target[row];
    if (t == ignore) {          // block-uniform exit, as ce_fwd_kernel
        if (threadIdx.x == 0) { row_lse[row] = 0.f; row_nv[row] = 0.f; row_loss[row] = 0.f; row_top[row] = -1; }
        return;
    }
    const LT* x = logits + (int64_t)row * ld;
    const RowScan r = row_scan<true>(x, V, &sh);
    if (threadIdx.x == 0) {
        const bool poisoned = r.top.v != r.top.v;
        float loss = NAN;          // also a target outside [0, V) that is not the ignore index, as ce_fwd_kernel
        if (!poisoned && t >= 0 && t < V) {
            const float nll = r.lse - lget(x, t);
            loss = eps == 0.f ? nll : (1.f - eps) * nll + eps * (r.lse - r.sx / r.nv);
        }
        row_lse[row] = poisoned ? NAN : r.lse;
        row_nv[row] = r.nv;
        row_loss[row] = loss;
        row_top[row] = r.top.i;
    }
}

// out[0], out[1] as ce_finalize_kernel; out[2] = #(non-ignored rows whose arg-max is the target); out[3] = count.  Whole numbers up to 2^24
// are exact in fp32, in any summation order.
__global__ __launch_bounds__(256) void ce_stats_finalize_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ target,
                                                                const int64_t* __restrict__ row_top, int64_t ignore, int M,
                                                                float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.f, c = 0.f, h = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) {
        const int64_t t = target[r];
        s += row_loss[r];
        c += (t != ignore) ? 1.f : 0.f;
        h += (t != ignore && row_top[r] == t) ? 1.f : 0.f;
    }
    const float S = block_sum(s, sh);
    const float C = block_sum(c, sh);
    const float H = block_sum(h, sh);
    if (threadIdx.x == 0) { out[0] = S / C; out[1] = C; out[2] = H; out[3] = C; }
}

// d loss / d x[c] = coef (p_c - (1 - eps) [c == t] - (eps / nv) [x_c != -inf]): a -inf column gets p_c = 0 and no smoothing term.
// Stores as ce_bwd_kernel: fp32 into [0, V), bf16 rounded once with zeros up to ldd.
template <typename DT>
__global__ __launch_bounds__(256) void ce_smooth_bwd_kernel(const DT* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                            int64_t ignore, float eps, const float* __restrict__ row_lse,
                                                            const float* __restrict__ row_nv, const float* __restrict__ out,
                                                            const float* __restrict__ gout, DT* __restrict__ dl, int64_t ldd, int V) {
    const int row = blockIdx.x;
    const int64_t t = target[row];
    DT* d = dl + (int64_t)row * ldd;
    const int Vz = sizeof(DT) == 2 ? (int)ldd : V;
    if (t == ignore) {
        for (int c = threadIdx.x; c < Vz; c += 256) grad_store(d, c, 0.f);
        return;
    }
    const float coef = gout[0] / out[1], lse = row_lse[row], hot = 1.f - eps, smooth = eps / row_nv[row];
    const DT* x = logits + (int64_t)row * ld;
    for (int c = threadIdx.x; c < V; c += 256) {
        const float xv = lget(x, c);
        float g = expf(xv - lse) - (c == t ? hot : 0.f);
        if (xv != -INFINITY) g -= smooth;
        grad_store(d, c, g * coef);
    }
    for (int c = V + threadIdx.x; c < Vz; c += 256) grad_store(d, c, 0.f);
}

// kl_fwd_kernel (same lse, same sum: same bits) with the arg-max of the prediction row riding in the lse pass and the arg-max of the target
// row in the KL pass.  row_top = the prediction's arg-max, row_hit = 1 where the two agree.
template <typename LT>
__global__ __launch_bounds__(256) void kl_stats_fwd_kernel(const LT* __restrict__ pred, int64_t ld, const float* __restrict__ tgt, int64_t ldt,
                                                           const int64_t* __restrict__ mask, float* __restrict__ row_lse,
                                                           float* __restrict__ row_loss, int64_t* __restrict__ row_top,
                                                           float* __restrict__ row_hit, int C) {
    __shared__ ScanShared sh;
    __shared__ float shs[4];
    const int row = blockIdx.x;
    if (mask[row] == 0) {
        if (threadIdx.x == 0) { row_lse[row] = 0.f; row_loss[row] = 0.f; row_top[row] = -1; row_hit[row] = 0.f; }
        return;
    }
    const LT* x = pred + (int64_t)row * ld;
    const float* t = tgt + (int64_t)row * ldt;
    const RowScan r = row_scan<false>(x, C, &sh);
    float acc = 0.f;
    Top tt = {-INFINITY, (int)threadIdx.x};
    int nan_i = INT_MAX;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float tv = t[c];
        if (tv > 0.f) acc = __builtin_fmaf(tv, logf(tv) - (lget(x, c) - r.lse), acc);          // kl_fwd_kernel's `acc += tv * (...)` as it compiles
        scan_push(tt, nan_i, tv, c);
    }
    const float tot = block_sum(acc, shs) * (float)mask[row];
    tt = block_top(scan_done(tt, nan_i), &sh);
    if (threadIdx.x == 0) {
        row_lse[row] = r.lse;
        row_loss[row] = tot;
        row_top[row] = r.top.i;
        row_hit[row] = (r.top.i == tt.i) ? 1.f : 0.f;
    }
}

// out[0], out[1] as kl_finalize_kernel; out[2] = sum(row_hit); out[3] = #(mask != 0), not clamped
__global__ __launch_bounds__(256) void kl_stats_finalize_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ mask,
                                                                const float* __restrict__ row_hit, int M, float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.f, c = 0.f, h = 0.f, n = 0.f;
    for (int r = threadIdx.x; r < M; r += 256) {
        s += row_loss[r];
        c += (float)mask[r];
        h += row_hit[r];
        n += (mask[r] != 0) ? 1.f : 0.f;
    }
    const float S = block_sum(s, sh);
    const float Cn = fmaxf(1.f, block_sum(c, sh));
    const float H = block_sum(h, sh);
    const float N = block_sum(n, sh);
    if (threadIdx.x == 0) { out[0] = S / Cn; out[1] = Cn; out[2] = H; out[3] = N; }
}

constexpr int kStatsMaxRows = 1 << 24;          // hits and counts are whole numbers held in fp32
inline bool smoothing_ok(float eps) { return eps >= 0.f && eps < 1.f; }          // false for a NaN

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_ce_fwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float* row_lse,
                                float* row_loss, float* out, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_loss && out && M > 0 && V > 0 && ld >= V, "ce_fwd: bad argument");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ce_fwd_kernel<float>, dim3(M), dim3(256), 0, s, logits, ld, target, ignore_index, row_lse, row_loss, V);
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, target, ignore_index, M, out);
    YT_LAUNCH_CHECK("ce_fwd");
    return 0;
}

extern "C" int ytvln_ce_fwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float* row_lse,
                                 float* row_loss, float* out, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_loss && out && M > 0 && V > 0 && ld >= V, "ce_fwd_bf16: bad argument");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ce_fwd_kernel<uint16_t>, dim3(M), dim3(256), 0, s, logits, ld, target, ignore_index, row_lse, row_loss, V);
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, target, ignore_index, M, out);
    YT_LAUNCH_CHECK("ce_fwd_bf16");
    return 0;
}

extern "C" int ytvln_ce_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, const float* row_lse,
                                const float* out, const float* gout, float* dlogits, int64_t ldd, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && out && gout && dlogits && M > 0 && V > 0 && ldd >= V, "ce_bwd: bad argument");
    hipLaunchKernelGGL(ce_bwd_kernel<float>, dim3(M), dim3(256), 0, as_stream(stream), logits, ld, target, ignore_index, row_lse, out, gout,
                       dlogits, ldd, V);
    YT_LAUNCH_CHECK("ce_bwd");
    return 0;
}

extern "C" int ytvln_ce_bwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, const float* row_lse,
                                 const float* out, const float* gout, uint16_t* dlogits, int64_t ldd, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && out && gout && dlogits && M > 0 && V > 0 && ldd >= V, "ce_bwd_bf16: bad argument");
    hipLaunchKernelGGL(ce_bwd_kernel<uint16_t>, dim3(M), dim3(256), 0, as_stream(stream), logits, ld, target, ignore_index, row_lse, out, gout,
                       dlogits, ldd, V);
    YT_LAUNCH_CHECK("ce_bwd_bf16");
    return 0;
}

extern "C" int ytvln_kl_fwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                                float* row_loss, float* out, int M, int C, void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && row_loss && out && M > 0 && C > 0, "kl_fwd: bad argument");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(kl_fwd_kernel<float>, dim3(M), dim3(256), 0, s, pred, ld, target, ldt, mask, row_lse, row_loss, C);
    hipLaunchKernelGGL(kl_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, mask, M, out);
    YT_LAUNCH_CHECK("kl_fwd");
    return 0;
}

extern "C" int ytvln_kl_fwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                                 float* row_loss, float* out, int M, int C, void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && row_loss && out && M > 0 && C > 0, "kl_fwd_bf16: bad argument");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(kl_fwd_kernel<uint16_t>, dim3(M), dim3(256), 0, s, pred, ld, target, ldt, mask, row_lse, row_loss, C);
    hipLaunchKernelGGL(kl_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, mask, M, out);
    YT_LAUNCH_CHECK("kl_fwd_bf16");
    return 0;
}

extern "C" int ytvln_kl_bwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask,
                                const float* row_lse, const float* out, const float* gout, float* dpred, int64_t ldd, int M, int C,
                                void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && out && gout && dpred && M > 0 && C > 0, "kl_bwd: bad argument");
    hipLaunchKernelGGL(kl_bwd_kernel<float>, dim3(M), dim3(256), 0, as_stream(stream), pred, ld, target, ldt, mask, row_lse, out, gout, dpred,
                       ldd, C);
    YT_LAUNCH_CHECK("kl_bwd");
    return 0;
}

extern "C" int ytvln_kl_bwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, const float* row_lse,
                                 const float* out, const float* gout, uint16_t* dpred, int64_t ldd, int M, int C, void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && out && gout && dpred && M > 0 && C > 0 && ldd >= C, "kl_bwd_bf16: bad argument");
    hipLaunchKernelGGL(kl_bwd_kernel<uint16_t>, dim3(M), dim3(256), 0, as_stream(stream), pred, ld, target, ldt, mask, row_lse, out, gout, dpred,
                       ldd, C);
    YT_LAUNCH_CHECK("kl_bwd_bf16");
    return 0;
}

extern "C" int ytvln_bce_fwd_f32(const float* x, const float* t, const float* pos_weight, float* out, int n, void* stream) {
    YT_REQUIRE(x && t && out && n > 0 && n <= 65536, "bce_fwd: bad argument (n=%d)", n);
    hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), x, t, pos_weight, out, n);
    YT_LAUNCH_CHECK("bce_fwd");
    return 0;
}

extern "C" int ytvln_bce_bwd_f32(const float* x, const float* t, const float* pos_weight, const float* gout, float* dx, int n,
                                 void* stream) {
    YT_REQUIRE(x && t && gout && dx && n > 0 && n <= 65536, "bce_bwd: bad argument (n=%d)", n);
    hipLaunchKernelGGL(bce_bwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), x, t, pos_weight, gout, dx, n);
    YT_LAUNCH_CHECK("bce_bwd");
    return 0;
}

extern "C" int ytvln_ce_stats_fwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                                      float* row_lse, float* row_aux, float* row_loss, int64_t* row_top, float* out, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_aux && row_loss && row_top && out, "ce_stats_fwd_f32: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && V > 0, "ce_stats_fwd_f32: M = %d (1 .. 2^24), V = %d", M, V);
    YT_REQUIRE(ld >= V, "ce_stats_fwd_f32: leading dimension %lld below V = %d", (long long)ld, V);
    YT_REQUIRE(smoothing_ok(label_smoothing), "ce_stats_fwd_f32: label_smoothing must be in [0, 1), got %g", (double)label_smoothing);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ce_stats_fwd_kernel<float>, dim3(M), dim3(256), 0, s, logits, ld, target, ignore_index, label_smoothing, row_lse, row_aux,
                       row_loss, row_top, V);
    hipLaunchKernelGGL(ce_stats_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, target, row_top, ignore_index, M, out);
    YT_LAUNCH_CHECK("ce_stats_fwd_f32");
    return 0;
}

extern "C" int ytvln_ce_stats_fwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                                       float* row_lse, float* row_aux, float* row_loss, int64_t* row_top, float* out, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_aux && row_loss && row_top && out, "ce_stats_fwd_bf16: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && V > 0, "ce_stats_fwd_bf16: M = %d (1 .. 2^24), V = %d", M, V);
    YT_REQUIRE(ld >= V, "ce_stats_fwd_bf16: leading dimension %lld below V = %d", (long long)ld, V);
    YT_REQUIRE(smoothing_ok(label_smoothing), "ce_stats_fwd_bf16: label_smoothing must be in [0, 1), got %g", (double)label_smoothing);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ce_stats_fwd_kernel<uint16_t>, dim3(M), dim3(256), 0, s, logits, ld, target, ignore_index, label_smoothing, row_lse, row_aux,
                       row_loss, row_top, V);
    hipLaunchKernelGGL(ce_stats_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, target, row_top, ignore_index, M, out);
    YT_LAUNCH_CHECK("ce_stats_fwd_bf16");
    return 0;
}

extern "C" int ytvln_ce_smooth_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                                       const float* row_lse, const float* row_aux, const float* out, const float* gout, float* dlogits, int64_t ldd,
                                       int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_aux && out && gout && dlogits, "ce_smooth_bwd_f32: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && V > 0, "ce_smooth_bwd_f32: M = %d (1 .. 2^24), V = %d", M, V);
    YT_REQUIRE(ld >= V && ldd >= V, "ce_smooth_bwd_f32: leading dimension below V = %d (ld %lld, ldd %lld)", V, (long long)ld, (long long)ldd);
    YT_REQUIRE(smoothing_ok(label_smoothing), "ce_smooth_bwd_f32: label_smoothing must be in [0, 1), got %g", (double)label_smoothing);
    hipLaunchKernelGGL(ce_smooth_bwd_kernel<float>, dim3(M), dim3(256), 0, as_stream(stream), logits, ld, target, ignore_index, label_smoothing,
                       row_lse, row_aux, out, gout, dlogits, ldd, V);
    YT_LAUNCH_CHECK("ce_smooth_bwd_f32");
    return 0;
}

extern "C" int ytvln_ce_smooth_bwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                                        const float* row_lse, const float* row_aux, const float* out, const float* gout, uint16_t* dlogits,
                                        int64_t ldd, int M, int V, void* stream) {
    YT_REQUIRE(logits && target && row_lse && row_aux && out && gout && dlogits, "ce_smooth_bwd_bf16: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && V > 0, "ce_smooth_bwd_bf16: M = %d (1 .. 2^24), V = %d", M, V);
    YT_REQUIRE(ld >= V && ldd >= V, "ce_smooth_bwd_bf16: leading dimension below V = %d (ld %lld, ldd %lld)", V, (long long)ld, (long long)ldd);
    YT_REQUIRE(smoothing_ok(label_smoothing), "ce_smooth_bwd_bf16: label_smoothing must be in [0, 1), got %g", (double)label_smoothing);
    hipLaunchKernelGGL(ce_smooth_bwd_kernel<uint16_t>, dim3(M), dim3(256), 0, as_stream(stream), logits, ld, target, ignore_index, label_smoothing,
                       row_lse, row_aux, out, gout, dlogits, ldd, V);
    YT_LAUNCH_CHECK("ce_smooth_bwd_bf16");
    return 0;
}

extern "C" int ytvln_kl_stats_fwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                                      float* row_loss, int64_t* row_top, float* row_hit, float* out, int M, int C, void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && row_loss && row_top && row_hit && out, "kl_stats_fwd_f32: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && C > 0, "kl_stats_fwd_f32: M = %d (1 .. 2^24), C = %d", M, C);
    YT_REQUIRE(ld >= C && ldt >= C, "kl_stats_fwd_f32: leading dimension below C = %d (ld %lld, ldt %lld)", C, (long long)ld, (long long)ldt);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(kl_stats_fwd_kernel<float>, dim3(M), dim3(256), 0, s, pred, ld, target, ldt, mask, row_lse, row_loss, row_top, row_hit, C);
    hipLaunchKernelGGL(kl_stats_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, mask, row_hit, M, out);
    YT_LAUNCH_CHECK("kl_stats_fwd_f32");
    return 0;
}

extern "C" int ytvln_kl_stats_fwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                                       float* row_loss, int64_t* row_top, float* row_hit, float* out, int M, int C, void* stream) {
    YT_REQUIRE(pred && target && mask && row_lse && row_loss && row_top && row_hit && out, "kl_stats_fwd_bf16: null pointer");
    YT_REQUIRE(M > 0 && M <= kStatsMaxRows && C > 0, "kl_stats_fwd_bf16: M = %d (1 .. 2^24), C = %d", M, C);
    YT_REQUIRE(ld >= C && ldt >= C, "kl_stats_fwd_bf16: leading dimension below C = %d (ld %lld, ldt %lld)", C, (long long)ld, (long long)ldt);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(kl_stats_fwd_kernel<uint16_t>, dim3(M), dim3(256), 0, s, pred, ld, target, ldt, mask, row_lse, row_loss, row_top, row_hit, C);
    hipLaunchKernelGGL(kl_stats_finalize_kernel, dim3(1), dim3(256), 0, s, row_loss, mask, row_hit, M, out);
    YT_LAUNCH_CHECK("kl_stats_fwd_bf16");
    return 0;
}
