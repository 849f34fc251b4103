// Kernels of the downstream-task heads (VILBertForVLTasks / SimpleClassifier, vilbert.py:1457-1535): weight normalisation over a whole matrix
// (dim = None: one scalar gain per matrix) and the Linear with ONE output feature over every region / token row, fused with the dropout in
// front of it and the region-mask term behind it.  Both are HBM-bound streaming kernels: 16 bytes per lane, fp32 arithmetic, no atomics --
// every reduction runs in an order fixed by the shapes alone, so two launches on the same inputs are bit-identical.
#include "common.h"
#include <algorithm>

namespace ytvln {
namespace {

typedef uint16_t bf16_t;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

__device__ __forceinline__ uint32_t bfbits(float f) { return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f); }      // round to nearest even

// ---- weight normalisation --------------------------------------------------------------------------------------------------------------
// Two stages.  Stage 1: workgroup b reduces the contiguous chunk [b * chunk, (b + 1) * chunk) of the flat matrix (lane sums of 16-byte
// vectors, wave shuffle, LDS) into partial[b].  Stage 2 rides in front of the elementwise kernel: every workgroup adds the partials in index
// order (all of them get the same bits) and then scales its own chunk.  chunk is a multiple of 1024 elements, at most 256 chunks.
constexpr int WN_MAX_BLOCKS = 256;
inline int64_t wn_chunk(int64_t n) { return std::max<int64_t>(1024, cdiv(cdiv(n, WN_MAX_BLOCKS), 1024) * 1024); }
inline int wn_blocks(int64_t n) { return (int)std::max<int64_t>(1, cdiv(n, wn_chunk(n))); }

__device__ __forceinline__ float block_sum4(float v, float* red) {          // 4 waves -> one value, in wave order (thread 0 holds it)
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// partial[b] = sum over the chunk of a[i] * b[i]  (b == a: the sum of squares)
__global__ __launch_bounds__(256) void wn_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n, int64_t chunk,
                                                         float* __restrict__ partial) {
    __shared__ float red[4];
    const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = min(n, e0 + chunk);
    const int64_t v0 = e0 >> 2, v1 = e1 >> 2;          // whole 16-byte vectors of the chunk (chunk % 4 == 0: e0 is on the grid)
    float acc = 0.f;
    for (int64_t i = v0 + threadIdx.x; i < v1; i += 256) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
        acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
    }
    const int64_t t = (v1 << 2) + threadIdx.x;          // the last chunk's tail of n % 4 elements
    if (t < e1) acc = fmaf(a[t], b[t], acc);
    const float s = block_sum4(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__device__ __forceinline__ float wn_total(const float* __restrict__ partial, int nb, float* red) {          // index order; the same bits in every workgroup
    if ((int)threadIdx.x < nb) red[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < nb; ++i) s += red[i];
        red[WN_MAX_BLOCKS] = s;
    }
    __syncthreads();
    return red[WN_MAX_BLOCKS];
}

__global__ __launch_bounds__(256) void wn_fwd_kernel(const float* __restrict__ v, const float* __restrict__ g, int64_t n, int64_t chunk,
                                                     const float* __restrict__ partial, int nb, float* __restrict__ w,
                                                     bf16_t* __restrict__ wb, float* __restrict__ stat) {
    __shared__ float red[WN_MAX_BLOCKS + 1];
    const float norm = sqrtf(wn_total(partial, nb, red));
    const float s = g[0] / norm;
    if (blockIdx.x == 0 && threadIdx.x == 0) { stat[0] = norm; stat[1] = s; }
    const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = min(n, e0 + chunk);
    const int64_t v0 = e0 >> 2, v1 = e1 >> 2;
    for (int64_t i = v0 + threadIdx.x; i < v1; i += 256) {
        const float4 x = reinterpret_cast<const float4*>(v)[i];
        const float4 y = make_float4(x.x * s, x.y * s, x.z * s, x.w * s);
        reinterpret_cast<float4*>(w)[i] = y;
        if (wb) reinterpret_cast<uint2*>(wb)[i] = make_uint2(bfbits(y.x) | (bfbits(y.y) << 16), bfbits(y.z) | (bfbits(y.w) << 16));
    }
    const int64_t t = (v1 << 2) + threadIdx.x;
    if (t < e1) {
        const float y = v[t] * s;
        w[t] = y;
        if (wb) wb[t] = (bf16_t)bfbits(y);
    }
}

// dg = <dw, v> / |v|;  dv = s dw - (s <dw, v> / |v|^2) v   with s = g / |v| (stat[1]), |v| = stat[0]
__global__ __launch_bounds__(256) void wn_bwd_kernel(const float* __restrict__ v, const float* __restrict__ dw, const float* __restrict__ stat,
                                                     int64_t n, int64_t chunk, const float* __restrict__ partial, int nb, float* __restrict__ dv,
                                                     float* __restrict__ dg) {
    __shared__ float red[WN_MAX_BLOCKS + 1];
    const float ip = wn_total(partial, nb, red);
    const float norm = stat[0], s = stat[1];
    const float c = s * ip / (norm * norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) dg[0] = ip / norm;
    const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = min(n, e0 + chunk);
    const int64_t v0 = e0 >> 2, v1 = e1 >> 2;
    for (int64_t i = v0 + threadIdx.x; i < v1; i += 256) {
        const float4 x = reinterpret_cast<const float4*>(v)[i], d = reinterpret_cast<const float4*>(dw)[i];
        reinterpret_cast<float4*>(dv)[i] = make_float4(s * d.x - c * x.x, s * d.y - c * x.y, s * d.z - c * x.z, s * d.w - c * x.w);
    }
    const int64_t t = (v1 << 2) + threadIdx.x;
    if (t < e1) dv[t] = s * dw[t] - c * v[t];
}

// ---- row logit ---------------------------------------------------------------------------------------------------------------------------
// One 64-lane wave per row; a lane's vector is 16 bytes of the row: 4 floats or 8 bf16.  The keep-scale of element (r, c) is the one
// ytvln_dropout_f32 applies at flat element r * H + c of the same (rng, site): one Philox draw per group of four elements, whatever ldx.
template <class T> struct RowVec;
template <> struct RowVec<float> {
    static constexpr int W = 4;
    static __device__ __forceinline__ void load(const float* row, int cv, float (&o)[4]) {
        const float4 u = reinterpret_cast<const float4*>(row)[cv];
        o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w;
    }
    static __device__ __forceinline__ void store(float* row, int cv, const float (&o)[4]) {
        reinterpret_cast<float4*>(row)[cv] = make_float4(o[0], o[1], o[2], o[3]);
    }
};
template <> struct RowVec<bf16_t> {
    static constexpr int W = 8;
    static __device__ __forceinline__ void load(const bf16_t* row, int cv, float (&o)[8]) {
        const uint4 u = reinterpret_cast<const uint4*>(row)[cv];
        o[0] = __uint_as_float(u.x << 16); o[1] = __uint_as_float(u.x & 0xffff0000u);
        o[2] = __uint_as_float(u.y << 16); o[3] = __uint_as_float(u.y & 0xffff0000u);
        o[4] = __uint_as_float(u.z << 16); o[5] = __uint_as_float(u.z & 0xffff0000u);
        o[6] = __uint_as_float(u.w << 16); o[7] = __uint_as_float(u.w & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(bf16_t* row, int cv, const float (&o)[8]) {
        reinterpret_cast<uint4*>(row)[cv] = make_uint4(bfbits(o[0]) | (bfbits(o[1]) << 16), bfbits(o[2]) | (bfbits(o[3]) << 16),
                                                       bfbits(o[4]) | (bfbits(o[5]) << 16), bfbits(o[6]) | (bfbits(o[7]) << 16));
    }
};

template <int W>
__device__ __forceinline__ void load_w(const float* __restrict__ w, int cv, float (&o)[W]) {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
        const float4 u = reinterpret_cast<const float4*>(w)[cv * (W / 4) + q];
        o[4 * q] = u.x; o[4 * q + 1] = u.y; o[4 * q + 2] = u.z; o[4 * q + 3] = u.w;
    }
}

// k[e] = keep-scale of the W elements that start at group q0 of the site's flat element space
template <int W>
__device__ __forceinline__ void keep_scale(float (&k)[W], const DropKey& key, uint64_t q0, uint32_t thr, float ik) {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
        const u32x4 b = drop_bits(key, q0 + q);
        k[4 * q] = b.x >= thr ? ik : 0.f; k[4 * q + 1] = b.y >= thr ? ik : 0.f;
        k[4 * q + 2] = b.z >= thr ? ik : 0.f; k[4 * q + 3] = b.w >= thr ? ik : 0.f;
    }
}

template <class T>
__global__ __launch_bounds__(256) void row_logit_fwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ mask,
                                                            float* __restrict__ out, int64_t rows, int H, float p, const int64_t* rng,
                                                            int64_t site) {
    constexpr int W = RowVec<T>::W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HV = H / W, H4 = H >> 2;
    const bool drop = p > 0.f;
    DropKey key = {};
    if (drop) key = make_drop_key(rng, site);
    const uint32_t thr = drop_threshold(p);
    const float ik = 1.0f / (1.0f - p);
    const float b = bias ? bias[0] : 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const T* row = x + r * ldx;
        float acc = 0.f;
        for (int cv = lane; cv < HV; cv += 64) {
            float xv[W], wv[W];
            RowVec<T>::load(row, cv, xv);
            load_w<W>(w, cv, wv);
            if (drop) {
                float k[W];
                keep_scale<W>(k, key, (uint64_t)r * H4 + (uint64_t)cv * (W / 4), thr, ik);
#pragma unroll
                for (int e = 0; e < W; ++e) xv[e] *= k[e];
            }
#pragma unroll
            for (int e = 0; e < W; ++e) acc = fmaf(xv[e], wv[e], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            float o = acc + b;                                          // the reference's association: (dot + bias) + mask term
            if (mask) o = o + (1.0f - mask[r]) * -10000.0f;
            out[r] = o;
        }
    }
}

// Run `blockIdx.x` = rows [run * rpr, (run + 1) * rpr): the waves take its rows round-robin, every lane keeps the sums of its own columns in
// registers; then the four waves' sums are added in wave order through LDS and leave as ONE [H] partial row (+ the run's sum of dy at column H).
constexpr int RL_MAX_RUNS = 1024;
inline int64_t rl_rows_per_run(int64_t rows) { return std::max<int64_t>(16, cdiv(rows, RL_MAX_RUNS)); }
inline int rl_runs(int64_t rows) { return (int)std::max<int64_t>(1, cdiv(rows, rl_rows_per_run(rows))); }
inline int64_t rl_ldp(int H) { return (int64_t)H + 4; }

template <class T, int NV>
__global__ __launch_bounds__(256) void row_logit_bwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                            const float* __restrict__ dy, int64_t rows, int H, float p, const int64_t* rng,
                                                            int64_t site, T* __restrict__ dx, int64_t lddx, float* __restrict__ partial,
                                                            int64_t rpr) {
    constexpr int W = RowVec<T>::W;
    __shared__ float red[2048 + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HV = H / W, H4 = H >> 2;
    const bool drop = p > 0.f;
    DropKey key = {};
    if (drop) key = make_drop_key(rng, site);
    const uint32_t thr = drop_threshold(p);
    const float ik = 1.0f / (1.0f - p);
    float wv[NV][W], acc[NV][W];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int cv = lane + 64 * j;
#pragma unroll
        for (int e = 0; e < W; ++e) { wv[j][e] = 0.f; acc[j][e] = 0.f; }
        if (cv < HV) load_w<W>(w, cv, wv[j]);
    }
    float dsum = 0.f;
    const int64_t r0 = (int64_t)blockIdx.x * rpr, r1 = min(rows, r0 + rpr);
    // the wave's next row is loaded before the current one is worked on: a wave walks its rows one after the other, and without the
    // prefetch every row would pay the full memory latency between its load and its store
    float xn[NV][W];
    auto load_row = [&](int64_t r) {
        const T* row = x + r * ldx;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int cv = lane + 64 * j;
            if (cv < HV) RowVec<T>::load(row, cv, xn[j]);
        }
    };
    if (r0 + wave < r1) load_row(r0 + wave);
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        float xv[NV][W];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
            for (int e = 0; e < W; ++e) xv[j][e] = xn[j][e];
        }
        if (r + 4 < r1) load_row(r + 4);
        const float g = dy[r];
        dsum += g;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int cv = lane + 64 * j;
            if (cv < HV) {
                float k[W], dv[W];
                if (drop) {
                    keep_scale<W>(k, key, (uint64_t)r * H4 + (uint64_t)cv * (W / 4), thr, ik);
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e) k[e] = 1.f;
                }
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const float kg = k[e] * g;
                    acc[j][e] = fmaf(kg, xv[j][e], acc[j][e]);
                    dv[e] = kg * wv[j][e];
                }
                if (dx) RowVec<T>::store(dx + r * lddx, cv, dv);
            }
        }
    }
    for (int s = 0; s < 4; ++s) {          // wave order
        if (wave == s) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int cv = lane + 64 * j;
                if (cv < HV) {
#pragma unroll
                    for (int e = 0; e < W; ++e) red[cv * W + e] = s == 0 ? acc[j][e] : red[cv * W + e] + acc[j][e];
                }
            }
            if (lane == 0) red[H] = s == 0 ? dsum : red[H] + dsum;
        }
        __syncthreads();
    }
    float* prow = partial + (int64_t)blockIdx.x * ((int64_t)H + 4);
    for (int c = threadIdx.x; c <= H; c += 256) prow[c] = red[c];
}

// dw[c] = sum over runs of partial[run, c]; db = the same of column H.  A workgroup of 16 waves owns 64 columns: wave k adds its sixteenth of
// the runs in run order, then wave 0 adds the sixteen sums in wave order -- an order fixed by the number of runs alone.
__global__ __launch_bounds__(1024) void row_logit_reduce_kernel(const float* __restrict__ partial, int nruns, int H, float* __restrict__ dw,
                                                                float* __restrict__ db) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t ld = (int64_t)H + 4;
    const int per = (nruns + 15) / 16;
    const int r0 = wave * per, r1 = min(nruns, r0 + per);
    float s = 0.f;
    if (c <= H) {
#pragma unroll 16
        for (int r = r0; r < r1; ++r) s += partial[r * ld + c];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c <= H) {
        float t = red[0][lane];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k][lane];
        if (c < H) dw[c] = t;
        else if (db) db[0] = t;
    }
}

template <class T>
int row_logit_check(const char* who, const T* x, int64_t ldx, const float* w, int64_t rows, int H, float p, const int64_t* rng) {
    constexpr int W = RowVec<T>::W;
    YT_REQUIRE(rows >= 0, "%s: rows < 0", who);
    YT_REQUIRE(H > 0 && H % W == 0 && H <= 2048, "%s: H=%d unsupported (need H %% %d == 0, H <= 2048)", who, H, W);
    YT_REQUIRE(ldx >= H && ldx % W == 0, "%s: ldx=%lld must be a multiple of %d and >= H", who, (long long)ldx, W);
    YT_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p out of range", who);
    YT_REQUIRE(!(p > 0.f) || rng, "%s: dropout needs rng state", who);
    if (rows == 0) return 0;
    YT_REQUIRE(x && w, "%s: null pointer", who);
    YT_REQUIRE(al16(x) && al16(w), "%s: pointers must be 16-byte aligned", who);
    return 0;
}

template <class T>
int row_logit_fwd(const char* who, const T* x, int64_t ldx, const float* w, const float* bias, const float* mask, float* out, int64_t rows, int H,
                  float p, const int64_t* rng, int64_t site, void* stream) {
    if (int rc = row_logit_check(who, x, ldx, w, rows, H, p, rng)) return rc;
    if (rows == 0) return 0;
    YT_REQUIRE(out, "%s: null pointer", who);
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(rows, 4), 4096);
    hipLaunchKernelGGL(row_logit_fwd_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), x, ldx, w, bias, mask, out, rows, H, p, rng, site);
    YT_LAUNCH_CHECK(who);
    return 0;
}

template <class T>
int row_logit_bwd(const char* who, const T* x, int64_t ldx, const float* w, const float* dy, int64_t rows, int H, float p, const int64_t* rng,
                  int64_t site, T* dx, int64_t lddx, float* dw, float* db, float* workspace, void* stream) {
    constexpr int W = RowVec<T>::W;
    if (int rc = row_logit_check(who, x, ldx, w, rows, H, p, rng)) return rc;
    YT_REQUIRE(dw && al16(dw), "%s: dw must be a 16-byte aligned pointer", who);
    YT_REQUIRE(!dx || (al16(dx) && lddx >= H && lddx % W == 0), "%s: dx must be 16-byte aligned, lddx a multiple of %d and >= H", who, W);
    YT_REQUIRE(rows == 0 || (dy && workspace && al16(workspace)), "%s: null or misaligned dy / workspace", who);
    hipStream_t st = as_stream(stream);
    const int nruns = rows ? rl_runs(rows) : 0;
    if (rows) {
        const int64_t rpr = rl_rows_per_run(rows);
        const int nv = (int)cdiv(H / W, 64);
        if (nv <= 1) hipLaunchKernelGGL((row_logit_bwd_kernel<T, 1>), dim3(nruns), dim3(256), 0, st, x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, workspace, rpr);
        else if (nv <= 2) hipLaunchKernelGGL((row_logit_bwd_kernel<T, 2>), dim3(nruns), dim3(256), 0, st, x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, workspace, rpr);
        else if (nv <= 4) hipLaunchKernelGGL((row_logit_bwd_kernel<T, 4>), dim3(nruns), dim3(256), 0, st, x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, workspace, rpr);
        else if constexpr (W == 4) hipLaunchKernelGGL((row_logit_bwd_kernel<T, 8>), dim3(nruns), dim3(256), 0, st, x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, workspace, rpr);
        YT_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(row_logit_reduce_kernel, dim3((unsigned)cdiv(H + 1, 64)), dim3(1024), 0, st, workspace, nruns, H, dw, db);      // no rows: zeros
    YT_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace
}  // namespace ytvln

using namespace ytvln;

extern "C" int64_t ytvln_weight_norm_workspace_elems(int64_t n) { return n > 0 ? wn_blocks(n) : 0; }

extern "C" int ytvln_weight_norm_fwd_f32(const float* v, const float* g, int64_t n, float* w, uint16_t* w_bf16, float* stat, float* workspace,
                                         void* stream) {
    YT_REQUIRE(n > 0, "weight_norm_fwd: n must be positive");
    YT_REQUIRE(v && g && w && stat && workspace, "weight_norm_fwd: null pointer");
    YT_REQUIRE(al16(v) && al16(w) && (!w_bf16 || al8(w_bf16)), "weight_norm_fwd: v / w must be 16-byte aligned, w_bf16 8-byte aligned");
    const int64_t chunk = wn_chunk(n);
    const int nb = wn_blocks(n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(wn_partial_kernel, dim3(nb), dim3(256), 0, st, v, v, n, chunk, workspace);
    hipLaunchKernelGGL(wn_fwd_kernel, dim3(nb), dim3(256), 0, st, v, g, n, chunk, workspace, nb, w, w_bf16, stat);
    YT_LAUNCH_CHECK("weight_norm_fwd");
    return 0;
}

extern "C" int ytvln_weight_norm_bwd_f32(const float* v, const float* dw, const float* stat, int64_t n, float* dv, float* dg, float* workspace,
                                         void* stream) {
    YT_REQUIRE(n > 0, "weight_norm_bwd: n must be positive");
    YT_REQUIRE(v && dw && stat && dv && dg && workspace, "weight_norm_bwd: null pointer");
    YT_REQUIRE(al16(v) && al16(dw) && al16(dv), "weight_norm_bwd: v / dw / dv must be 16-byte aligned");
    const int64_t chunk = wn_chunk(n);
    const int nb = wn_blocks(n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(wn_partial_kernel, dim3(nb), dim3(256), 0, st, dw, v, n, chunk, workspace);
    hipLaunchKernelGGL(wn_bwd_kernel, dim3(nb), dim3(256), 0, st, v, dw, stat, n, chunk, workspace, nb, dv, dg);
    YT_LAUNCH_CHECK("weight_norm_bwd");
    return 0;
}

extern "C" int64_t ytvln_row_logit_workspace_elems(int64_t rows, int H) { return (rows > 0 && H > 0) ? rl_runs(rows) * rl_ldp(H) : 0; }

extern "C" int ytvln_row_logit_fwd_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* mask, float* out, int64_t rows,
                                       int H, float p, const int64_t* rng, int64_t site, void* stream) {
    return row_logit_fwd<float>("row_logit_fwd_f32", x, ldx, w, bias, mask, out, rows, H, p, rng, site, stream);
}

extern "C" int ytvln_row_logit_fwd_bf16(const uint16_t* x, int64_t ldx, const float* w, const float* bias, const float* mask, float* out,
                                        int64_t rows, int H, float p, const int64_t* rng, int64_t site, void* stream) {
    return row_logit_fwd<uint16_t>("row_logit_fwd_bf16", x, ldx, w, bias, mask, out, rows, H, p, rng, site, stream);
}

extern "C" int ytvln_row_logit_bwd_f32(const float* x, int64_t ldx, const float* w, const float* dy, int64_t rows, int H, float p,
                                       const int64_t* rng, int64_t site, float* dx, int64_t lddx, float* dw, float* db, float* workspace,
                                       void* stream) {
    return row_logit_bwd<float>("row_logit_bwd_f32", x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, dw, db, workspace, stream);
}

extern "C" int ytvln_row_logit_bwd_bf16(const uint16_t* x, int64_t ldx, const float* w, const float* dy, int64_t rows, int H, float p,
                                        const int64_t* rng, int64_t site, uint16_t* dx, int64_t lddx, float* dw, float* db, float* workspace,
                                        void* stream) {
    return row_logit_bwd<uint16_t>("row_logit_bwd_bf16", x, ldx, w, dy, rows, H, p, rng, site, dx, lddx, dw, db, workspace, stream);
}
