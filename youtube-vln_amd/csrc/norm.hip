// HBM-bound kernels of the ViLBERT path: fused (dropout/)residual/LayerNorm forward+backward, the two embedding front
// ends, activation backward, dropout, column reductions and embedding-gradient scatters.
//
// Layout rule for all of them: one 64-lane wave owns one row of H floats, every lane moves 16-byte vectors
// (global_load_dwordx4), the row stays in registers between the two reduction passes (mean, then centred variance as the
// reference computes it, vilbert.py:214-216), so each element is read once and written once.
#include "common.h"
#include <algorithm>

namespace ytvln {

enum { LN_PLAIN = 0, LN_TEXT = 1, LN_IMAGE = 2 };

struct LnArgs {
    // plain
    const void* x; const void* res;          // element type XT of the kernel (float, or bf16 for the bf16-resident path)
    // text embedding
    const int64_t* ids; const int64_t* type_ids; const float* word; const float* pos; const float* type; int T;
    // image embedding
    const float* loc; const float* W5; const float* b5; const float* W4; const float* b4; const float* W2;
    const float* b2; const float* E;
    // common
    const float* gamma; const float* beta; void* y; void* s_out; float* mean; float* rstd;          // y / s_out: element type YT
    int64_t rows; int H; float eps; float p_pre, p_post; const int64_t* rng; int64_t site;
};

// Four consecutive elements of a row as fp32: one 16-byte access for float rows, one 8-byte access for bf16 rows (round to nearest even on
// the way out).  `c4` counts groups of four elements, so the dropout bits (one Philox draw per group) are the same in both precisions.
typedef uint16_t bf16_t;
__device__ __forceinline__ float4 ld4(const float* p, int64_t c4) { return reinterpret_cast<const float4*>(p)[c4]; }
__device__ __forceinline__ float4 ld4(const bf16_t* p, int64_t c4) {
    const uint2 u = reinterpret_cast<const uint2*>(p)[c4];
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ void st4(float* p, int64_t c4, float4 v) { reinterpret_cast<float4*>(p)[c4] = v; }
__device__ __forceinline__ uint32_t bfbits(float f) { return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f); }
__device__ __forceinline__ void st4(bf16_t* p, int64_t c4, float4 v) {
    reinterpret_cast<uint2*>(p)[c4] = make_uint2(bfbits(v.x) | (bfbits(v.y) << 16), bfbits(v.z) | (bfbits(v.w) << 16));
}

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4scale_keep(float4 v, u32x4 b, uint32_t thr, float ik) {
    return make_float4(b.x >= thr ? v.x * ik : 0.f, b.y >= thr ? v.y * ik : 0.f, b.z >= thr ? v.z * ik : 0.f,
                       b.w >= thr ? v.w * ik : 0.f);
}

// Dropout draws of a row kernel.  fp32 rows: one Philox call per 4 elements, 32-bit draws (index row * H/4 + c4).  bf16 rows with
// H % 8 == 0: one call per 8 elements, 16-bit draws (index row * H/8 + c8) -- the scheme of the 16-bytes-per-lane kernels
// (ln_*_bf16x8_kernel).  The scheme is a function of the row type and H ALONE, never of pointer alignment or of which kernel form a
// launch happens to take, so a forward and its backward always regenerate the same mask (the embedding forwards run the 4-wide kernels,
// their backward the 8-wide one).
__device__ __forceinline__ uint32_t drop_threshold16(float p) { return (uint32_t)(p * 65536.0f + 0.5f); }
__device__ __forceinline__ float4 drop4(float4 v, const DropKey& key, uint64_t row, int H4, int c4, bool x8, uint32_t thr, float ik) {
    if (!x8) return f4scale_keep(v, drop_bits(key, row * H4 + c4), thr, ik);
    const u32x4 b = drop_bits(key, row * (uint64_t)(H4 >> 1) + (c4 >> 1));
    const uint32_t w0 = (c4 & 1) ? b.z : b.x, w1 = (c4 & 1) ? b.w : b.y;
    return make_float4((w0 & 0xffffu) >= thr ? v.x * ik : 0.f, (w0 >> 16) >= thr ? v.y * ik : 0.f,
                       (w1 & 0xffffu) >= thr ? v.z * ik : 0.f, (w1 >> 16) >= thr ? v.w * ik : 0.f);
}

template <int NV, int MODE, typename XT = float, typename YT = float>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const LnArgs a) {
    const XT* const xin = reinterpret_cast<const XT*>(a.x);
    const XT* const rin = reinterpret_cast<const XT*>(a.res);
    YT* const yout = reinterpret_cast<YT*>(a.y);
    YT* const sout = reinterpret_cast<YT*>(a.s_out);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H4 = a.H >> 2;
    const float invH = 1.0f / (float)a.H;
    const bool pre = a.p_pre > 0.f, post = a.p_post > 0.f;
    const bool x8 = std::is_same<YT, bf16_t>::value && (a.H % 8 == 0);       // draw scheme: see drop4
    DropKey key = {0, 0, 0, 0};
    uint32_t thr_pre = 0, thr_post = 0;
    float ik_pre = 1.f, ik_post = 1.f;
    if (pre || post) {
        key = make_drop_key(a.rng, a.site);
        thr_pre = x8 ? drop_threshold16(a.p_pre) : drop_threshold(a.p_pre); ik_pre = 1.0f / (1.0f - a.p_pre);
        thr_post = x8 ? drop_threshold16(a.p_post) : drop_threshold(a.p_post); ik_post = 1.0f / (1.0f - a.p_post);
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < a.rows; row += (int64_t)gridDim.x * 4) {
        float4 s[NV];
        float loc[12];
        const float* wrow = nullptr; const float* prow = nullptr; const float* trow = nullptr; const float* erow = nullptr;
        if (MODE == LN_TEXT) {
            wrow = a.word + a.ids[row] * (int64_t)a.H;
            prow = a.pos + (row % a.T) * (int64_t)a.H;
            trow = a.type + (a.type_ids ? a.type_ids[row] : 0) * (int64_t)a.H;
        }
        if (MODE == LN_IMAGE) {
            const float4* lp = reinterpret_cast<const float4*>(a.loc + row * 12);
            const float4 l0 = lp[0], l1 = lp[1], l2 = lp[2];
            loc[0] = l0.x; loc[1] = l0.y; loc[2] = l0.z; loc[3] = l0.w; loc[4] = l1.x; loc[5] = l1.y; loc[6] = l1.z;
            loc[7] = l1.w; loc[8] = l2.x; loc[9] = l2.y; loc[10] = l2.z; loc[11] = l2.w;
            erow = a.E + (int64_t)((long)loc[11]) * a.H;   // .long() truncation, vilbert.py:1364
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = lane + 64 * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c4 < H4) {
                if (MODE == LN_PLAIN) {
                    v = ld4(xin + row * a.H, c4);
                    if (pre) v = drop4(v, key, (uint64_t)row, H4, c4, x8, thr_pre, ik_pre);
                    if (rin) v = f4add(v, ld4(rin + row * a.H, c4));
                } else if (MODE == LN_TEXT) {
                    v = f4add(f4add(reinterpret_cast<const float4*>(wrow)[c4], reinterpret_cast<const float4*>(prow)[c4]),
                              reinterpret_cast<const float4*>(trow)[c4]);
                } else {
                    const int c = c4 << 2;
                    float o[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float* w5 = a.W5 + (c + u) * 5;
                        const float* w4 = a.W4 + (c + u) * 4;
                        const float* w2 = a.W2 + (c + u) * 2;
                        float av = a.b5[c + u], bv = a.b4[c + u], cv = a.b2[c + u];
#pragma unroll
                        for (int q = 0; q < 5; ++q) av = fmaf(w5[q], loc[q], av);
#pragma unroll
                        for (int q = 0; q < 4; ++q) bv = fmaf(w4[q], loc[5 + q], bv);
#pragma unroll
                        for (int q = 0; q < 2; ++q) cv = fmaf(w2[q], loc[9 + q], cv);
                        o[u] = ((av + bv) + cv) + erow[c + u];   // a + b + c + d, vilbert.py:1365
                    }
                    v = f4add(ld4(xin + row * a.H, c4), make_float4(o[0], o[1], o[2], o[3]));
                }
                sum += (v.x + v.y) + (v.z + v.w);
            }
            s[j] = v;
        }
        // a true division: sum * (1 / H) with the rounded reciprocal leaves the mean of a CONSTANT row one ulp off for some H (252, 1020: 2.5 ->
        // 2.5000002), and with eps = 1e-12 that ulp is the whole "variance" -- xhat came out -0.23 instead of 0.  The row sum of a constant row is
        // exact, so the correctly rounded quotient is the constant itself, as in the reference's x.mean(-1).
        const float mu = wave_sum(sum) / (float)a.H;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (lane + 64 * j < H4) {
                const float dx = s[j].x - mu, dy = s[j].y - mu, dz = s[j].z - mu, dw = s[j].w - mu;
                sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        }
        const float var = wave_sum(sq) * invH;
        const float sd = sqrtf(var + a.eps);
        if (lane == 0) {
            if (a.mean) a.mean[row] = mu;
            if (a.rstd) a.rstd[row] = 1.0f / sd;
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = lane + 64 * j;
            if (c4 < H4) {
                if (sout) st4(sout + row * a.H, c4, s[j]);
                const float4 g = reinterpret_cast<const float4*>(a.gamma)[c4], b = reinterpret_cast<const float4*>(a.beta)[c4];
                float4 o = make_float4(g.x * ((s[j].x - mu) / sd) + b.x, g.y * ((s[j].y - mu) / sd) + b.y,
                                       g.z * ((s[j].z - mu) / sd) + b.z, g.w * ((s[j].w - mu) / sd) + b.w);
                if (post) o = drop4(o, key, (uint64_t)row, H4, c4, x8, thr_post, ik_post);
                st4(yout + row * a.H, c4, o);
            }
        }
    }
}

struct LnBwdArgs {
    const void* dy; const void* s; const float* mean; const float* rstd; const float* gamma;      // dy / s: element type XT
    void* ds; void* dx; float* ds_f32; float* partial;                                               // ds / dx: XT; ds_f32: optional fp32 copy of ds
    int64_t rows; int H; int rows_per_block; float p_pre, p_post; const int64_t* rng; int64_t site;
};

template <int NV, typename XT = float>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float red[];   // [4 waves][2][H]
    const XT* const dyin = reinterpret_cast<const XT*>(a.dy);
    const XT* const sin = reinterpret_cast<const XT*>(a.s);
    XT* const dsout = reinterpret_cast<XT*>(a.ds);
    XT* const dxout = reinterpret_cast<XT*>(a.dx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H4 = a.H >> 2;
    const float invH = 1.0f / (float)a.H;
    const bool pre = a.p_pre > 0.f, post = a.p_post > 0.f;
    const bool x8 = std::is_same<XT, bf16_t>::value && (a.H % 8 == 0);       // draw scheme: see drop4
    DropKey key = {0, 0, 0, 0};
    uint32_t thr_pre = 0, thr_post = 0;
    float ik_pre = 1.f, ik_post = 1.f;
    if (pre || post) {
        key = make_drop_key(a.rng, a.site);
        thr_pre = x8 ? drop_threshold16(a.p_pre) : drop_threshold(a.p_pre); ik_pre = 1.0f / (1.0f - a.p_pre);
        thr_post = x8 ? drop_threshold16(a.p_post) : drop_threshold(a.p_post); ik_post = 1.0f / (1.0f - a.p_post);
    }
    float4 dg[NV], db[NV], gm[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        dg[j] = make_float4(0.f, 0.f, 0.f, 0.f); db[j] = dg[j];
        gm[j] = (lane + 64 * j < H4) ? reinterpret_cast<const float4*>(a.gamma)[lane + 64 * j] : dg[j];
    }
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_block;
    const int64_t r1 = min(r0 + a.rows_per_block, a.rows);
    // A wave walks its rows with the loads of the NEXT row issued in front of the arithmetic, the two wave reductions and the stores of the
    // current one (the stores may alias the loads as far as the compiler knows, so it keeps them in program order: without the explicit
    // prefetch a wave has one row of loads in flight, waits, reduces, stores, and only then asks for the next row).
    float4 dn[NV], sn[NV];
    float mun = 0.f, rsn = 0.f;
    auto fetch = [&](int64_t row) __attribute__((always_inline)) {
        mun = a.mean[row]; rsn = a.rstd[row];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = lane + 64 * j;
            if (c4 < H4) { dn[j] = ld4(dyin + row * a.H, c4); sn[j] = ld4(sin + row * a.H, c4); }
        }
    };
    if (r0 + wave < r1) fetch(r0 + wave);
    for (int64_t row = r0 + wave; row < r1; row += 4) {
        const float mu = mun, rs = rsn;
        float4 dc[NV], sc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { dc[j] = dn[j]; sc[j] = sn[j]; }
        if (row + 4 < r1) fetch(row + 4);
        float4 g[NV], xh[NV];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = lane + 64 * j;
            g[j] = make_float4(0.f, 0.f, 0.f, 0.f); xh[j] = g[j];
            if (c4 < H4) {
                float4 d = dc[j];
                if (post) d = drop4(d, key, (uint64_t)row, H4, c4, x8, thr_post, ik_post);
                const float4 sv = sc[j];
                xh[j] = make_float4((sv.x - mu) * rs, (sv.y - mu) * rs, (sv.z - mu) * rs, (sv.w - mu) * rs);
                dg[j].x += d.x * xh[j].x; dg[j].y += d.y * xh[j].y; dg[j].z += d.z * xh[j].z; dg[j].w += d.w * xh[j].w;
                db[j] = f4add(db[j], d);
                g[j] = make_float4(d.x * gm[j].x, d.y * gm[j].y, d.z * gm[j].z, d.w * gm[j].w);
                c1 += (g[j].x + g[j].y) + (g[j].z + g[j].w);
                c2 += (g[j].x * xh[j].x + g[j].y * xh[j].y) + (g[j].z * xh[j].z + g[j].w * xh[j].w);
            }
        }
        c1 = wave_sum(c1) * invH;
        c2 = wave_sum(c2) * invH;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = lane + 64 * j;
            if (c4 < H4) {
                float4 o = make_float4(rs * (g[j].x - c1 - xh[j].x * c2), rs * (g[j].y - c1 - xh[j].y * c2),
                                       rs * (g[j].z - c1 - xh[j].z * c2), rs * (g[j].w - c1 - xh[j].w * c2));
                if (dsout) st4(dsout + row * a.H, c4, o);
                if (a.ds_f32) st4(a.ds_f32 + row * a.H, c4, o);
                if (pre && dxout) st4(dxout + row * a.H, c4, drop4(o, key, (uint64_t)row, H4, c4, x8, thr_pre, ik_pre));
            }
        }
    }
    // cross-wave reduction of the dgamma / dbeta partials, one [2,H] record per block
    float* mine = red + wave * 2 * a.H;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c4 = lane + 64 * j;
        if (c4 < H4) {
            reinterpret_cast<float4*>(mine)[c4] = dg[j];
            reinterpret_cast<float4*>(mine + a.H)[c4] = db[j];
        }
    }
    __syncthreads();
    float* out = a.partial + (int64_t)blockIdx.x * 2 * a.H;
    for (int i = threadIdx.x; i < 2 * a.H; i += 256)
        out[i] = (red[i] + red[2 * a.H + i]) + (red[4 * a.H + i] + red[6 * a.H + i]);
}

// ---- bf16 rows, 16 bytes per lane -----------------------------------------------------------------------------------------------------
// The plain (dropout ->) residual -> LayerNorm of the bf16-resident path moves HALF the bytes of the fp32 kernel, so per byte everything that is
// not a memory access weighs twice: these forms take 8 elements (one 16-byte access) per lane and vector, and draw the hidden-state dropout
// mask from ONE Philox call per 8 elements (16 bits per element: keep iff bits16 >= round(p * 65536); P(drop) = 0.1000061 for p = 0.1).
// Forward and backward regenerate the same mask from (seed, counter, site, row, vector index); the fp32 kernels keep their 32-bit draws.
struct f8 { float v[8]; };
__device__ __forceinline__ uint4 ld8raw(const bf16_t* p, int64_t c8) { return reinterpret_cast<const uint4*>(p)[c8]; }
__device__ __forceinline__ f8 cvt8(const uint4 u) {
    f8 r;
    r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
    r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
    r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
    r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}
__device__ __forceinline__ f8 ld8(const bf16_t* p, int64_t c8) { return cvt8(ld8raw(p, c8)); }
__device__ __forceinline__ void st8(bf16_t* p, int64_t c8, const f8& r) {
    reinterpret_cast<uint4*>(p)[c8] = make_uint4(bfbits(r.v[0]) | (bfbits(r.v[1]) << 16), bfbits(r.v[2]) | (bfbits(r.v[3]) << 16),
                                                 bfbits(r.v[4]) | (bfbits(r.v[5]) << 16), bfbits(r.v[6]) | (bfbits(r.v[7]) << 16));
}
__device__ __forceinline__ f8 ldg8(const float* p, int c8) {
    const float4 a = reinterpret_cast<const float4*>(p)[2 * c8], b = reinterpret_cast<const float4*>(p)[2 * c8 + 1];
    f8 r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void keep8(f8& r, const u32x4 b, uint32_t thr16, float ik) {          // element e keeps iff its 16 random bits >= thr16
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t bits = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
        r.v[e] = bits >= thr16 ? r.v[e] * ik : 0.f;
    }
}

template <int NV>
__global__ __launch_bounds__(256) void ln_fwd_bf16x8_kernel(const LnArgs a) {
    const bf16_t* const xin = reinterpret_cast<const bf16_t*>(a.x);
    const bf16_t* const rin = reinterpret_cast<const bf16_t*>(a.res);
    bf16_t* const yout = reinterpret_cast<bf16_t*>(a.y);
    bf16_t* const sout = reinterpret_cast<bf16_t*>(a.s_out);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H8 = a.H >> 3;
    const float invH = 1.0f / (float)a.H;
    const bool pre = a.p_pre > 0.f, post = a.p_post > 0.f;
    DropKey key = {0, 0, 0, 0};
    uint32_t thr_pre = 0, thr_post = 0;
    float ik_pre = 1.f, ik_post = 1.f;
    if (pre || post) {
        key = make_drop_key(a.rng, a.site);
        thr_pre = drop_threshold16(a.p_pre); ik_pre = 1.0f / (1.0f - a.p_pre);
        thr_post = drop_threshold16(a.p_post); ik_post = 1.0f / (1.0f - a.p_post);
    }
    f8 gm[NV], bt[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (lane + 64 * j < H8) { gm[j] = ldg8(a.gamma, lane + 64 * j); bt[j] = ldg8(a.beta, lane + 64 * j); }
    // next row's loads in front of this row's reductions and stores (see ln_bwd_kernel)
    uint4 xn[NV], rn[NV];
    const int64_t rstep = (int64_t)gridDim.x * 4;
    auto fetch = [&](int64_t row) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) {
                xn[j] = ld8raw(xin + row * a.H, c8);
                if (rin) rn[j] = ld8raw(rin + row * a.H, c8);
            }
        }
    };
    if ((int64_t)blockIdx.x * 4 + wave < a.rows) fetch((int64_t)blockIdx.x * 4 + wave);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < a.rows; row += rstep) {
        uint4 xc[NV], rc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { xc[j] = xn[j]; rc[j] = rn[j]; }
        if (row + rstep < a.rows) fetch(row + rstep);
        f8 s[NV];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) {
                s[j] = cvt8(xc[j]);
                if (pre) keep8(s[j], drop_bits(key, (uint64_t)row * H8 + c8), thr_pre, ik_pre);
                if (rin) {
                    const f8 r = cvt8(rc[j]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[j].v[e] += r.v[e];
                }
#pragma unroll
                for (int e = 0; e < 8; e += 2) sum += s[j].v[e] + s[j].v[e + 1];
            }
        }
        const float mu = wave_sum(sum) / (float)a.H;          // a true division: see ln_fwd_kernel
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (lane + 64 * j < H8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float dd = s[j].v[e] - mu; sq += dd * dd; }
            }
        const float var = wave_sum(sq) * invH;
        const float rs = 1.0f / sqrtf(var + a.eps);
        if (lane == 0) {
            if (a.mean) a.mean[row] = mu;
            if (a.rstd) a.rstd[row] = rs;
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) {
                if (sout) st8(sout + row * a.H, c8, s[j]);
                f8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o.v[e] = gm[j].v[e] * ((s[j].v[e] - mu) * rs) + bt[j].v[e];
                if (post) keep8(o, drop_bits(key, (uint64_t)row * H8 + c8), thr_post, ik_post);
                st8(yout + row * a.H, c8, o);
            }
        }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void ln_bwd_bf16x8_kernel(const LnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float red[];   // [4 waves][2][H]
    const bf16_t* const dyin = reinterpret_cast<const bf16_t*>(a.dy);
    const bf16_t* const sin = reinterpret_cast<const bf16_t*>(a.s);
    bf16_t* const dsout = reinterpret_cast<bf16_t*>(a.ds);
    bf16_t* const dxout = reinterpret_cast<bf16_t*>(a.dx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H8 = a.H >> 3;
    const float invH = 1.0f / (float)a.H;
    const bool pre = a.p_pre > 0.f, post = a.p_post > 0.f;
    DropKey key = {0, 0, 0, 0};
    uint32_t thr_pre = 0, thr_post = 0;
    float ik_pre = 1.f, ik_post = 1.f;
    if (pre || post) {
        key = make_drop_key(a.rng, a.site);
        thr_pre = drop_threshold16(a.p_pre); ik_pre = 1.0f / (1.0f - a.p_pre);
        thr_post = drop_threshold16(a.p_post); ik_post = 1.0f / (1.0f - a.p_post);
    }
    f8 dg[NV], db[NV], gm[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { dg[j].v[e] = 0.f; db[j].v[e] = 0.f; gm[j].v[e] = 0.f; }
        if (lane + 64 * j < H8) gm[j] = ldg8(a.gamma, lane + 64 * j);
    }
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_block;
    const int64_t r1 = min(r0 + a.rows_per_block, a.rows);
    // next row's loads in front of this row's reductions and stores (see ln_bwd_kernel)
    uint4 dn[NV], sn[NV];
    float mun = 0.f, rsn = 0.f;
    auto fetch = [&](int64_t row) __attribute__((always_inline)) {
        mun = a.mean[row]; rsn = a.rstd[row];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) { dn[j] = ld8raw(dyin + row * a.H, c8); sn[j] = ld8raw(sin + row * a.H, c8); }
        }
    };
    if (r0 + wave < r1) fetch(r0 + wave);
    for (int64_t row = r0 + wave; row < r1; row += 4) {
        const float mu = mun, rs = rsn;
        uint4 dc[NV], sc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { dc[j] = dn[j]; sc[j] = sn[j]; }
        if (row + 4 < r1) fetch(row + 4);
        f8 g[NV], xh[NV];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) {
                f8 d = cvt8(dc[j]);
                if (post) keep8(d, drop_bits(key, (uint64_t)row * H8 + c8), thr_post, ik_post);
                const f8 sv = cvt8(sc[j]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    xh[j].v[e] = (sv.v[e] - mu) * rs;
                    dg[j].v[e] += d.v[e] * xh[j].v[e];
                    db[j].v[e] += d.v[e];
                    g[j].v[e] = d.v[e] * gm[j].v[e];
                    c1 += g[j].v[e];
                    c2 += g[j].v[e] * xh[j].v[e];
                }
            }
        }
        c1 = wave_sum(c1) * invH;
        c2 = wave_sum(c2) * invH;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c8 = lane + 64 * j;
            if (c8 < H8) {
                f8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o.v[e] = rs * (g[j].v[e] - c1 - xh[j].v[e] * c2);
                if (dsout) st8(dsout + row * a.H, c8, o);
                if (a.ds_f32) {
                    reinterpret_cast<float4*>(a.ds_f32 + row * a.H)[2 * c8] = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
                    reinterpret_cast<float4*>(a.ds_f32 + row * a.H)[2 * c8 + 1] = make_float4(o.v[4], o.v[5], o.v[6], o.v[7]);
                }
                if (pre && dxout) {
                    keep8(o, drop_bits(key, (uint64_t)row * H8 + c8), thr_pre, ik_pre);
                    st8(dxout + row * a.H, c8, o);
                }
            }
        }
    }
    float* mine = red + wave * 2 * a.H;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c8 = lane + 64 * j;
        if (c8 < H8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { mine[8 * c8 + e] = dg[j].v[e]; mine[a.H + 8 * c8 + e] = db[j].v[e]; }
        }
    }
    __syncthreads();
    float* out = a.partial + (int64_t)blockIdx.x * 2 * a.H;
    for (int i = threadIdx.x; i < 2 * a.H; i += 256)
        out[i] = (red[i] + red[2 * a.H + i]) + (red[4 * a.H + i] + red[6 * a.H + i]);
}

// ---- column reductions --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int64_t ldx, int M, int N,
                                                     float* __restrict__ out, int64_t ldo, int rpb) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int r0 = blockIdx.y * rpb, r1 = min(r0 + rpb, M);
    float acc = 0.f;
    if (c < N)
        for (int r = r0 + rl; r < r1; r += 4) acc += x[(int64_t)r * ldx + c];
    red[rl][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rl == 0 && c < N) {
        const int l = threadIdx.x;
        out[(int64_t)blockIdx.y * ldo + c] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    }
}

// 16-byte variant: a lane owns 4 consecutive columns, a wave sweeps 1 KiB of a row per load, 4 rows in flight per lane.
__global__ __launch_bounds__(256) void colsum_v4_kernel(const float* __restrict__ x, int64_t ldx, int M, int N4,
                                                        float* __restrict__ out, int64_t ldo, int rpb) {
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c4 = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * rpb, r1 = min(r0 + rpb, M);
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    if (c4 < N4) {
        const float4* p = reinterpret_cast<const float4*>(x) + c4;
        const int64_t ld4 = ldx >> 2;
        int r = r0 + rl;
        for (; r + 12 < r1; r += 16) {
            const float4 v0 = p[(int64_t)r * ld4], v1 = p[(int64_t)(r + 4) * ld4], v2 = p[(int64_t)(r + 8) * ld4], v3 = p[(int64_t)(r + 12) * ld4];
            a0 = f4add(a0, v0); a1 = f4add(a1, v1); a2 = f4add(a2, v2); a3 = f4add(a3, v3);
        }
        for (; r < r1; r += 4) a0 = f4add(a0, p[(int64_t)r * ld4]);
    }
    red[rl][lane] = f4add(f4add(a0, a1), f4add(a2, a3));
    __syncthreads();
    if (rl == 0 && c4 < N4)
        reinterpret_cast<float4*>(out + (int64_t)blockIdx.y * ldo)[c4] = f4add(f4add(red[0][lane], red[1][lane]), f4add(red[2][lane], red[3][lane]));
}

__global__ __launch_bounds__(256) void colsum_by_index_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ idx_f, int64_t idx_stride,
                                                              const int64_t* __restrict__ idx_i, int M, int N, int KT,
                                                              float* __restrict__ out, int rpb) {
    extern __shared__ float acc[];   // [4][KT][64]
    const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + l;
    float* mine = acc + (rl * KT) * 64 + l;
    for (int k = 0; k < KT; ++k) mine[k * 64] = 0.f;
    const int r0 = blockIdx.y * rpb, r1 = min(r0 + rpb, M);
    if (c < N)
        for (int r = r0 + rl; r < r1; r += 4) {
            const int k = idx_i ? (int)idx_i[r] : (int)idx_f[(int64_t)r * idx_stride];
            if (k >= 0 && k < KT) mine[k * 64] += x[(int64_t)r * ldx + c];
        }
    __syncthreads();
    if (c < N)
        for (int k = rl; k < KT; k += 4) {
            const float* p = acc + k * 64 + l;
            out[((int64_t)blockIdx.y * KT + k) * N + c] = (p[0] + p[KT * 64]) + (p[2 * KT * 64] + p[3 * KT * 64]);
        }
}

__global__ __launch_bounds__(256) void scatter_add_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const int64_t* __restrict__ idx, int M, int H,
                                                               float* __restrict__ tg, int64_t skip) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x * 4 + wave; r < M; r += gridDim.x * 4) {
        const int64_t k = idx[r];
        if (k == skip) continue;
        float* dst = tg + k * (int64_t)H;
        const float* src = x + (int64_t)r * ldx;
        for (int c = lane; c < H; c += 64) unsafeAtomicAdd(dst + c, src[c]);
    }
}

// Deterministic variant for repeated indices (the word-embedding gradient: a token id occurs many times in a batch): the caller passes
// the indices SORTED (stable) with the permutation that sorted them; the wave that sits on the first position of a run of equal
// indices walks the run in order, accumulates in registers and owns the table row -- no atomics, a fixed summation order.
__global__ __launch_bounds__(256) void scatter_add_rows_sorted_kernel(const float* __restrict__ x, int64_t ldx,
                                                                      const int64_t* __restrict__ sorted_idx, const int64_t* __restrict__ perm,
                                                                      int M, int H, float* __restrict__ tg, int64_t skip) {
    // Work unit = (head of a run, 64-lane column chunk): a long run ([MASK] fills ~12 % of the rows) is walked by H/256 waves side by
    // side, eight row loads in flight at a time; the additions keep the order of the run, so the sums do not depend on the launch shape.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H4 = H >> 2, nchunk = (H4 + 63) >> 6;
    const int64_t units = (int64_t)M * nchunk;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < units; u += (int64_t)gridDim.x * 4) {
        const int i = (int)(u / nchunk), c = (int)(u % nchunk) * 64 + lane;
        const int64_t k = sorted_idx[i];
        if (k == skip || (i > 0 && sorted_idx[i - 1] == k)) continue;          // not the head of a run
        if (c >= H4) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int j = i;
        while (j + 7 < M && sorted_idx[j + 7] == k) {                             // (sorted: rows j .. j+7 all belong to the run)
            float4 a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = reinterpret_cast<const float4*>(x + perm[j + q] * ldx)[c];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = f4add(acc, a[q]);
            j += 8;
        }
        for (; j < M && sorted_idx[j] == k; ++j) acc = f4add(acc, reinterpret_cast<const float4*>(x + perm[j] * ldx)[c]);
        float4* dst = reinterpret_cast<float4*>(tg + k * (int64_t)H) + c;
        *dst = f4add(*dst, acc);
    }
}

// out[j, :] = x[idx[j], :]   (idx < 0 -> zeros).  Row gather for the loss-aware heads (only rows carrying a target go through
// the 30522-way / 1601-way decoders); its backward is scatter_add_rows_kernel.
// Work unit = one 1024-float piece of one output row (a wave moves it as 4 x 16 bytes per lane), so short rows (hidden states in front
// of the loss-aware heads) and very long ones (a whole frame of 36 x 2048-d region features, ytvln.batch.expand_options) both spread
// over the chip.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, int64_t ldx, const int64_t* __restrict__ idx,
                                                          int R, int H, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ppr = (H + 1023) >> 10;                       // pieces per row
    const int64_t pieces = (int64_t)R * ppr;
    for (int64_t pc = (int64_t)blockIdx.x * 4 + wave; pc < pieces; pc += (int64_t)gridDim.x * 4) {
        const int r = (int)(pc / ppr), c0 = (int)(pc % ppr) << 10;
        const int64_t k = idx[r];
        const float* src = x + (k < 0 ? 0 : k) * ldx;
        float* dst = out + (int64_t)r * H;
        if (VEC) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + 4 * (lane + 64 * u);
                if (c < H)
                    *reinterpret_cast<float4*>(dst + c) = k < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(src + c);
            }
        } else {
            for (int c = c0 + lane; c < min(c0 + 1024, H); c += 64) dst[c] = k < 0 ? 0.f : src[c];
        }
    }
}

// ---- elementwise --------------------------------------------------------------------------------------------------
// swish(z) = z * sigmoid(z) (vilbert.py:122-123) and its derivative s + z s (1 - s).  The two halves of the sigmoid, p = e / (1 + e) <= 1/2
// and q = 1 / (1 + e) >= 1/2 with e = exp(-|z|) <= 1, are both formed from the one small exponential: no quotient can become inf / inf or
// 0 * inf, 1 - s carries no cancellation (it IS the other half), and |z| p <= |z| exp(-|z|) < 0.37.  z = -1e4: e = 0, swish = -0.0, derivative 0;
// z = +1e4: swish = z, derivative 1.  expf and the division are the accurate ones (the fp32 kernels owe the reference 1e-6).
__device__ __forceinline__ void sigmoid_halves(float z, float& p, float& q) {
    const float e = expf(-fabsf(z));
    q = 1.0f / (1.0f + e);
    p = e * q;
}
__device__ __forceinline__ float swish_f(float z) {
    float p, q;
    sigmoid_halves(z, p, q);
    return z * (z < 0.f ? p : q);
}
__device__ __forceinline__ float dswish_f(float z) {
    float p, q;
    sigmoid_halves(z, p, q);
    return fmaf(z * p, q, z < 0.f ? p : q);
}
__device__ __forceinline__ float4 swish4(float4 z) { return make_float4(swish_f(z.x), swish_f(z.y), swish_f(z.z), swish_f(z.w)); }
__device__ __forceinline__ float4 mul_dswish4(float4 d, float4 z) {
    return make_float4(d.x * dswish_f(z.x), d.y * dswish_f(z.y), d.z * dswish_f(z.z), d.w * dswish_f(z.w));
}
__device__ __forceinline__ float bf1(const bf16_t* p, int64_t i) { return __uint_as_float((uint32_t)p[i] << 16); }

// y = swish(z), the unfused activation behind a plain GEMM (gelu / relu are GEMM epilogues and never come here).  y == z is allowed: every
// lane reads exactly the elements it writes (no __restrict__ on the pair).  VEC: 16 bytes per lane over the first n & ~3 (fp32) / n & ~7 (bf16)
// elements, block 0 finishes the tail one element per lane; !VEC (a base pointer off the 16-byte grid): one element per lane throughout.
template <bool VEC>
__global__ __launch_bounds__(256) void swish_fwd_kernel(const float* z, float* y, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += step) st4(y, i, swish4(ld4(z, i)));
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const int64_t i = (n4 << 2) + threadIdx.x;
            y[i] = swish_f(z[i]);
        }
    } else {
        for (int64_t i = tid; i < n; i += step) y[i] = swish_f(z[i]);
    }
}

// h = gelu_erf(z): the output of the fp32 GEMM's EPI_GELU epilogue, recomputed from the pre-activation that epilogue wrote to `aux` -- the same
// device function on the same fp32 value, hence the same bits (FFNFn with recompute = "ffn" keeps z only and calls this just before the dW2
// GEMM of its backward).  A pure streaming pass, shaped like swish_fwd_kernel: VEC = 16 bytes per lane over the first n & ~3 elements and block 0
// finishes the tail one element per lane; !VEC (a pointer off the 16-byte grid) = one element per lane throughout.  Nothing is written at or
// past n.  h == z is allowed (every lane reads exactly what it writes).
template <bool VEC>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* z, float* h, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += step) {
            const float4 v = ld4(z, i);
            st4(h, i, make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w)));
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const int64_t i = (n4 << 2) + threadIdx.x;
            h[i] = gelu_erf(z[i]);
        }
    } else {
        for (int64_t i = tid; i < n; i += step) h[i] = gelu_erf(z[i]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void swish_fwd_bf16_kernel(const bf16_t* z, bf16_t* y, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t n8 = n >> 3;
        for (int64_t i = tid; i < n8; i += step) {
            f8 v = ld8(z, i);
#pragma unroll
            for (int j = 0; j < 8; ++j) v.v[j] = swish_f(v.v[j]);
            st8(y, i, v);
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
            const int64_t i = (n8 << 3) + threadIdx.x;
            y[i] = (bf16_t)bfbits(swish_f(bf1(z, i)));
        }
    } else {
        for (int64_t i = tid; i < n; i += step) y[i] = (bf16_t)bfbits(swish_f(bf1(z, i)));
    }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ aux,
                                                      float* __restrict__ dz, int64_t n, int act) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 d = reinterpret_cast<const float4*>(dy)[i], z = reinterpret_cast<const float4*>(aux)[i];
        float4 o;
        if (act == YTVLN_EPI_GELU) o = make_float4(d.x * dgelu_erf(z.x), d.y * dgelu_erf(z.y), d.z * dgelu_erf(z.z), d.w * dgelu_erf(z.w));
        else if (act == YTVLN_ACT_SWISH) o = mul_dswish4(d, z);
        else o = make_float4(z.x > 0.f ? d.x : 0.f, z.y > 0.f ? d.y : 0.f, z.z > 0.f ? d.z : 0.f, z.w > 0.f ? d.w : 0.f);
        reinterpret_cast<float4*>(dz)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        dz[i] = act == YTVLN_EPI_GELU ? dy[i] * dgelu_erf(aux[i]) : act == YTVLN_ACT_SWISH ? dy[i] * dswish_f(aux[i]) : (aux[i] > 0.f ? dy[i] : 0.f);
    }
}

// swish backward for fp32 pointers off the 16-byte grid (views into a larger buffer): one element per lane
__global__ __launch_bounds__(256) void swish_bwd_scalar_kernel(const float* __restrict__ dy, const float* __restrict__ aux, float* __restrict__ dz, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dz[i] = dy[i] * dswish_f(aux[i]);
}

__global__ __launch_bounds__(256) void act_bwd_bf16_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ aux, bf16_t* __restrict__ dz, int64_t n4, int act) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 d = ld4(dy, i), z = ld4(aux, i);
        float4 o;
        if (act == YTVLN_EPI_GELU) o = make_float4(d.x * dgelu_erf(z.x), d.y * dgelu_erf(z.y), d.z * dgelu_erf(z.z), d.w * dgelu_erf(z.w));
        else if (act == YTVLN_ACT_SWISH) o = mul_dswish4(d, z);
        else o = make_float4(z.x > 0.f ? d.x : 0.f, z.y > 0.f ? d.y : 0.f, z.z > 0.f ? d.z : 0.f, z.w > 0.f ? d.w : 0.f);
        st4(dz, i, o);
    }
}

// The swish backward of the bf16-resident path: 16 bytes per lane when the pointers allow it (VEC), one element per lane for the tail and for
// everything else -- the widths of the small heads are not all multiples of 4, which is what the gelu / relu form above asks for.
template <bool VEC>
__global__ __launch_bounds__(256) void swish_bwd_bf16_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ aux, bf16_t* __restrict__ dz, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t n8 = n >> 3;
        for (int64_t i = tid; i < n8; i += step) {
            const f8 d = ld8(dy, i), z = ld8(aux, i);
            f8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o.v[j] = d.v[j] * dswish_f(z.v[j]);
            st8(dz, i, o);
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
            const int64_t i = (n8 << 3) + threadIdx.x;
            dz[i] = (bf16_t)bfbits(bf1(dy, i) * dswish_f(bf1(aux, i)));
        }
    } else {
        for (int64_t i = tid; i < n; i += step) dz[i] = (bf16_t)bfbits(bf1(dy, i) * dswish_f(bf1(aux, i)));
    }
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, float p,
                                                      const int64_t* rng, int64_t site) {
    const DropKey key = make_drop_key(rng, site);
    const uint32_t thr = drop_threshold(p);
    const float ik = 1.0f / (1.0f - p);
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        reinterpret_cast<float4*>(y)[i] = f4scale_keep(reinterpret_cast<const float4*>(x)[i], drop_bits(key, (uint64_t)i), thr, ik);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        y[i] = x[i] * drop_scale1(key, (uint64_t)i, thr, ik);
    }
}

template <int MODE, typename XT = float, typename YT = float>
static int launch_ln(const LnArgs& a, hipStream_t s) {
    const int nv = (int)cdiv(a.H / 4, 64);
    const int grid = (int)std::min<int64_t>(cdiv(a.rows, 4), 4096);
    if (nv <= 1) hipLaunchKernelGGL((ln_fwd_kernel<1, MODE, XT, YT>), dim3(grid), dim3(256), 0, s, a);
    else if (nv <= 2) hipLaunchKernelGGL((ln_fwd_kernel<2, MODE, XT, YT>), dim3(grid), dim3(256), 0, s, a);
    else if (nv <= 4) hipLaunchKernelGGL((ln_fwd_kernel<4, MODE, XT, YT>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ln_fwd_kernel<8, MODE, XT, YT>), dim3(grid), dim3(256), 0, s, a);
    return 0;
}

static inline bool ln_shape_ok(int H) { return H > 0 && H % 4 == 0 && H <= 2048; }
static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_ln_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                                float* s_out, float* mean, float* rstd, int64_t rows, int H, float eps, float p_pre,
                                float p_post, const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(x && gamma && beta && y, "ln_fwd: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "ln_fwd: H=%d unsupported (need H %% 4 == 0, H <= 2048)", H);
    YT_REQUIRE(al16(x) && al16(y) && al16(gamma) && al16(beta) && (!res || al16(res)) && (!s_out || al16(s_out)),
               "ln_fwd: pointers must be 16-byte aligned");
    YT_REQUIRE(p_pre >= 0.f && p_pre < 1.f && p_post >= 0.f && p_post < 1.f, "ln_fwd: dropout p out of range");
    YT_REQUIRE(!(p_pre > 0.f || p_post > 0.f) || rng, "ln_fwd: dropout needs rng state");
    YT_REQUIRE(!(p_pre > 0.f && p_post > 0.f), "ln_fwd: p_pre and p_post both > 0 (the two masks would come from one draw)");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.x = x; a.res = res; a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = p_pre; a.p_post = p_post; a.rng = rng; a.site = site;
    launch_ln<LN_PLAIN>(a, as_stream(stream));
    YT_LAUNCH_CHECK("ln_fwd");
    return 0;
}

extern "C" int ytvln_text_embed_fwd_f32(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos,
                                        const float* type, const float* gamma, const float* beta, float* y, float* s_out,
                                        float* mean, float* rstd, int64_t rows, int T, int H, float eps, float p_post,
                                        const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(ids && word && pos && type && gamma && beta && y, "text_embed_fwd: null pointer");
    YT_REQUIRE(ln_shape_ok(H) && T > 0, "text_embed_fwd: bad shape H=%d T=%d", H, T);
    YT_REQUIRE(al16(word) && al16(pos) && al16(type) && al16(y) && al16(gamma) && al16(beta) && (!s_out || al16(s_out)),
               "text_embed_fwd: pointers must be 16-byte aligned");
    YT_REQUIRE(!(p_post > 0.f) || rng, "text_embed_fwd: dropout needs rng state");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.ids = ids; a.type_ids = type_ids; a.word = word; a.pos = pos; a.type = type; a.T = T;
    a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = 0.f; a.p_post = p_post; a.rng = rng; a.site = site;
    launch_ln<LN_TEXT>(a, as_stream(stream));
    YT_LAUNCH_CHECK("text_embed_fwd");
    return 0;
}

extern "C" int ytvln_image_embed_fwd_f32(const float* img, const float* loc, const float* W5, const float* b5,
                                         const float* W4, const float* b4, const float* W2, const float* b2,
                                         const float* E, const float* gamma, const float* beta, float* y, float* s_out,
                                         float* mean, float* rstd, int64_t rows, int H, float eps, float p_post,
                                         const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(img && loc && W5 && b5 && W4 && b4 && W2 && b2 && E && gamma && beta && y, "image_embed_fwd: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "image_embed_fwd: H=%d unsupported", H);
    YT_REQUIRE(al16(img) && al16(loc) && al16(y) && al16(gamma) && al16(beta) && (!s_out || al16(s_out)),
               "image_embed_fwd: pointers must be 16-byte aligned");
    YT_REQUIRE(!(p_post > 0.f) || rng, "image_embed_fwd: dropout needs rng state");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.x = img; a.loc = loc; a.W5 = W5; a.b5 = b5; a.W4 = W4; a.b4 = b4; a.W2 = W2; a.b2 = b2; a.E = E;
    a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = 0.f; a.p_post = p_post; a.rng = rng; a.site = site;
    launch_ln<LN_IMAGE>(a, as_stream(stream));
    YT_LAUNCH_CHECK("image_embed_fwd");
    return 0;
}

// (768 = three 4-wave workgroups per CU, what the H = 1024 kernel's registers allow: 1008 sixteen-row blocks ran as one full round plus a
//  third of one at a quarter of the occupancy; the 4480-row text launches had 280 blocks = four waves per CU)
extern "C" int ytvln_ln_bwd_blocks(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(768, cdiv(rows, 4))); }

extern "C" int ytvln_ln_bwd_f32(const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma,
                                float* ds, float* dx, float* partial, int64_t rows, int H, float p_pre, float p_post,
                                const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(dy && s && mean && rstd && gamma && ds && partial, "ln_bwd: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "ln_bwd: H=%d unsupported", H);
    YT_REQUIRE(al16(dy) && al16(s) && al16(ds) && al16(gamma) && (!dx || al16(dx)), "ln_bwd: pointers must be 16-byte aligned");
    YT_REQUIRE(!(p_pre > 0.f || p_post > 0.f) || rng, "ln_bwd: dropout needs rng state");
    YT_REQUIRE(!(p_pre > 0.f && p_post > 0.f), "ln_bwd: p_pre and p_post both > 0 (the two masks would come from one draw)");
    YT_REQUIRE(!(p_pre > 0.f) || dx, "ln_bwd: p_pre > 0 needs dx");
    if (rows == 0) return 0;
    LnBwdArgs a;
    a.dy = dy; a.s = s; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.ds = ds; a.dx = dx; a.ds_f32 = nullptr; a.partial = partial;
    a.rows = rows; a.H = H; a.p_pre = p_pre; a.p_post = p_post; a.rng = rng; a.site = site;
    const int nb = ytvln_ln_bwd_blocks(rows);
    a.rows_per_block = (int)cdiv(rows, nb);
    const int nv = (int)cdiv(H / 4, 64);
    const size_t lds = (size_t)8 * H * sizeof(float);
    hipStream_t st = as_stream(stream);
    if (nv <= 1) hipLaunchKernelGGL((ln_bwd_kernel<1>), dim3(nb), dim3(256), lds, st, a);
    else if (nv <= 2) hipLaunchKernelGGL((ln_bwd_kernel<2>), dim3(nb), dim3(256), lds, st, a);
    else if (nv <= 4) hipLaunchKernelGGL((ln_bwd_kernel<4>), dim3(nb), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((ln_bwd_kernel<8>), dim3(nb), dim3(256), lds, st, a);
    YT_LAUNCH_CHECK("ln_bwd");
    return 0;
}

extern "C" int ytvln_colsum_f32(const float* x, int64_t ldx, int M, int N, float* out, int64_t ldo, int rows_per_block,
                                void* stream) {
    YT_REQUIRE(x && out && M >= 0 && N > 0 && rows_per_block > 0, "colsum: bad argument");
    const int nb = (int)std::max<int64_t>(1, cdiv(M, rows_per_block));
    YT_REQUIRE(nb <= 65535, "colsum: too many row blocks (%d)", nb);
    if (N % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out))
        hipLaunchKernelGGL(colsum_v4_kernel, dim3((unsigned)cdiv(N / 4, 64), nb), dim3(256), 0, as_stream(stream), x, ldx, M, N / 4, out,
                           ldo, rows_per_block);
    else
        hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)cdiv(N, 64), nb), dim3(256), 0, as_stream(stream), x, ldx, M, N, out, ldo,
                           rows_per_block);
    YT_LAUNCH_CHECK("colsum");
    return 0;
}

extern "C" int ytvln_colsum_by_index_f32(const float* x, int64_t ldx, const float* idx_f32, int64_t idx_stride,
                                         const int64_t* idx_i64, int M, int N, int KT, float* out, int rows_per_block,
                                         void* stream) {
    YT_REQUIRE(x && out && (idx_f32 || idx_i64), "colsum_by_index: null pointer");
    YT_REQUIRE(KT > 0 && KT <= 32 && N > 0 && rows_per_block > 0, "colsum_by_index: KT=%d must be in 1..32", KT);
    const int nb = (int)std::max<int64_t>(1, cdiv(M, rows_per_block));
    YT_REQUIRE(nb <= 65535, "colsum_by_index: too many row blocks");
    hipLaunchKernelGGL(colsum_by_index_kernel, dim3((unsigned)cdiv(N, 64), nb), dim3(256), (size_t)4 * KT * 64 * sizeof(float),
                       as_stream(stream), x, ldx, idx_f32, idx_stride, idx_i64, M, N, KT, out, rows_per_block);
    YT_LAUNCH_CHECK("colsum_by_index");
    return 0;
}

extern "C" int ytvln_scatter_add_rows_f32(const float* x, int64_t ldx, const int64_t* idx, int M, int H, float* table_grad,
                                          int64_t skip_idx, void* stream) {
    YT_REQUIRE(x && idx && table_grad && H > 0, "scatter_add_rows: bad argument");
    if (M == 0) return 0;
    hipLaunchKernelGGL(scatter_add_rows_kernel, dim3((unsigned)std::min<int64_t>(cdiv(M, 4), 4096)), dim3(256), 0,
                       as_stream(stream), x, ldx, idx, M, H, table_grad, skip_idx);
    YT_LAUNCH_CHECK("scatter_add_rows");
    return 0;
}

extern "C" int ytvln_scatter_add_rows_sorted_f32(const float* x, int64_t ldx, const int64_t* sorted_idx, const int64_t* perm, int M, int H,
                                                 float* table_grad, int64_t skip_idx, void* stream) {
    YT_REQUIRE(x && sorted_idx && perm && table_grad && H > 0 && H % 4 == 0 && ldx % 4 == 0, "scatter_add_rows_sorted: bad argument (H, ldx multiples of 4)");
    YT_REQUIRE(al16(x) && al16(table_grad), "scatter_add_rows_sorted: pointers must be 16-byte aligned");
    if (M == 0) return 0;
    hipLaunchKernelGGL(scatter_add_rows_sorted_kernel, dim3((unsigned)std::min<int64_t>(cdiv((int64_t)M * cdiv(H / 4, 64), 4), 8192)), dim3(256), 0, as_stream(stream), x,
                       ldx, sorted_idx, perm, M, H, table_grad, skip_idx);
    YT_LAUNCH_CHECK("scatter_add_rows_sorted");
    return 0;
}

extern "C" int ytvln_gather_rows_f32(const float* x, int64_t ldx, const int64_t* idx, int R, int H, float* out, void* stream) {
    if (R == 0) return 0;
    YT_REQUIRE(x && idx && out && R > 0 && H > 0 && ldx >= H, "gather_rows: bad argument");
    const dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)R * cdiv(H, 1024), 4), 16384));
    if (H % 4 == 0 && ldx % 4 == 0 && al16(x) && al16(out))
        hipLaunchKernelGGL(gather_rows_kernel<true>, grid, dim3(256), 0, as_stream(stream), x, ldx, idx, R, H, out);
    else
        hipLaunchKernelGGL(gather_rows_kernel<false>, grid, dim3(256), 0, as_stream(stream), x, ldx, idx, R, H, out);
    YT_LAUNCH_CHECK("gather_rows");
    return 0;
}

static inline unsigned ew_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(items, 256), 4096)); }

extern "C" int ytvln_act_bwd_f32(const float* dy, const float* aux, float* dz, int64_t n, int act, void* stream) {
    YT_REQUIRE(dy && aux && dz, "act_bwd: null pointer");
    YT_REQUIRE(act == YTVLN_EPI_GELU || act == YTVLN_EPI_RELU || act == YTVLN_ACT_SWISH, "act_bwd: bad act %d", act);
    const bool aligned = al16(dy) && al16(aux) && al16(dz);
    YT_REQUIRE(aligned || act == YTVLN_ACT_SWISH, "act_bwd: pointers must be 16-byte aligned");
    YT_REQUIRE(n >= 0, "act_bwd: n < 0");
    if (n == 0) return 0;
    if (aligned)
        hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), dy, aux, dz, n, act);
    else
        hipLaunchKernelGGL(swish_bwd_scalar_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), dy, aux, dz, n);
    YT_LAUNCH_CHECK("act_bwd");
    return 0;
}

extern "C" int ytvln_act_fwd_f32(const float* z, float* y, int64_t n, int act, void* stream) {
    YT_REQUIRE(act == YTVLN_ACT_SWISH, "act_fwd: bad act %d (swish only: gelu and relu are GEMM epilogues)", act);
    YT_REQUIRE(n >= 0, "act_fwd: n < 0");
    if (n == 0) return 0;          // (an empty tensor has no address)
    YT_REQUIRE(z && y, "act_fwd: null pointer");
    if (al16(z) && al16(y))
        hipLaunchKernelGGL(swish_fwd_kernel<true>, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), z, y, n);
    else
        hipLaunchKernelGGL(swish_fwd_kernel<false>, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), z, y, n);
    YT_LAUNCH_CHECK("act_fwd");
    return 0;
}

extern "C" int ytvln_gelu_fwd_f32(const float* z, float* h, int64_t n, void* stream) {
    YT_REQUIRE(n >= 0, "gelu_fwd: n < 0");
    if (n == 0) return 0;          // (an empty tensor has no address)
    YT_REQUIRE(z && h, "gelu_fwd: null pointer");
    if (al16(z) && al16(h))
        hipLaunchKernelGGL(gelu_fwd_kernel<true>, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), z, h, n);
    else
        hipLaunchKernelGGL(gelu_fwd_kernel<false>, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), z, h, n);
    YT_LAUNCH_CHECK("gelu_fwd");
    return 0;
}

extern "C" int ytvln_dropout_f32(const float* x, float* y, int64_t n, float p, const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(x && y && rng, "dropout: null pointer");
    YT_REQUIRE(p >= 0.f && p < 1.f, "dropout: p out of range");
    YT_REQUIRE(al16(x) && al16(y), "dropout: pointers must be 16-byte aligned");
    if (n == 0) return 0;
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n / 4, 256), 4096))), dim3(256), 0,
                       as_stream(stream), x, y, n, p, rng, site);
    YT_LAUNCH_CHECK("dropout");
    return 0;
}

// ---- bf16-resident path (BASELINE configs[4]): the same kernels on bf16 rows; statistics, gamma / beta and their gradients stay fp32 --------
extern "C" int ytvln_ln_fwd_bf16(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta, uint16_t* y, uint16_t* s_out,
                                 float* mean, float* rstd, int64_t rows, int H, float eps, float p_pre, float p_post, const int64_t* rng,
                                 int64_t site, void* stream) {
    YT_REQUIRE(x && gamma && beta && y, "ln_fwd_bf16: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "ln_fwd_bf16: H=%d unsupported (need H %% 4 == 0, H <= 2048)", H);
    YT_REQUIRE(al8(x) && al8(y) && al16(gamma) && al16(beta) && (!res || al8(res)) && (!s_out || al8(s_out)), "ln_fwd_bf16: misaligned pointer");
    YT_REQUIRE(p_pre >= 0.f && p_pre < 1.f && p_post >= 0.f && p_post < 1.f, "ln_fwd_bf16: dropout p out of range");
    YT_REQUIRE(!(p_pre > 0.f || p_post > 0.f) || rng, "ln_fwd_bf16: dropout needs rng state");
    YT_REQUIRE(!(p_pre > 0.f && p_post > 0.f), "ln_fwd_bf16: p_pre and p_post both > 0 (the two masks would come from one draw)");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.x = x; a.res = res; a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = p_pre; a.p_post = p_post; a.rng = rng; a.site = site;
    if (H % 8 == 0 && al16(x) && al16(y) && (!res || al16(res)) && (!s_out || al16(s_out))) {          // 16 bytes per lane
        const int nv = (int)cdiv(H / 8, 64);
        const int grid = (int)std::min<int64_t>(cdiv(rows, 4), nv <= 2 ? 1024 : 512);          // one resident round; the waves walk rows with a prefetch
        hipStream_t st = as_stream(stream);
        if (nv <= 1) hipLaunchKernelGGL((ln_fwd_bf16x8_kernel<1>), dim3(grid), dim3(256), 0, st, a);
        else if (nv <= 2) hipLaunchKernelGGL((ln_fwd_bf16x8_kernel<2>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ln_fwd_bf16x8_kernel<4>), dim3(grid), dim3(256), 0, st, a);
    } else {
        launch_ln<LN_PLAIN, bf16_t, bf16_t>(a, as_stream(stream));
    }
    YT_LAUNCH_CHECK("ln_fwd_bf16");
    return 0;
}

extern "C" int ytvln_text_embed_fwd_bf16(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                                         const float* gamma, const float* beta, uint16_t* y, uint16_t* s_out, float* mean, float* rstd,
                                         int64_t rows, int T, int H, float eps, float p_post, const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(ids && word && pos && type && gamma && beta && y, "text_embed_fwd_bf16: null pointer");
    YT_REQUIRE(ln_shape_ok(H) && T > 0, "text_embed_fwd_bf16: bad shape H=%d T=%d", H, T);
    YT_REQUIRE(al16(word) && al16(pos) && al16(type) && al8(y) && al16(gamma) && al16(beta) && (!s_out || al8(s_out)), "text_embed_fwd_bf16: misaligned pointer");
    YT_REQUIRE(!(p_post > 0.f) || rng, "text_embed_fwd_bf16: dropout needs rng state");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.ids = ids; a.type_ids = type_ids; a.word = word; a.pos = pos; a.type = type; a.T = T;
    a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = 0.f; a.p_post = p_post; a.rng = rng; a.site = site;
    launch_ln<LN_TEXT, float, bf16_t>(a, as_stream(stream));
    YT_LAUNCH_CHECK("text_embed_fwd_bf16");
    return 0;
}

extern "C" int ytvln_image_embed_fwd_bf16(const uint16_t* img, const float* loc, const float* W5, const float* b5, const float* W4, const float* b4,
                                          const float* W2, const float* b2, const float* E, const float* gamma, const float* beta, uint16_t* y,
                                          uint16_t* s_out, float* mean, float* rstd, int64_t rows, int H, float eps, float p_post,
                                          const int64_t* rng, int64_t site, void* stream) {
    YT_REQUIRE(img && loc && W5 && b5 && W4 && b4 && W2 && b2 && E && gamma && beta && y, "image_embed_fwd_bf16: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "image_embed_fwd_bf16: H=%d unsupported", H);
    YT_REQUIRE(al8(img) && al16(loc) && al8(y) && al16(gamma) && al16(beta) && (!s_out || al8(s_out)), "image_embed_fwd_bf16: misaligned pointer");
    YT_REQUIRE(!(p_post > 0.f) || rng, "image_embed_fwd_bf16: dropout needs rng state");
    if (rows == 0) return 0;
    LnArgs a = {};
    a.x = img; a.loc = loc; a.W5 = W5; a.b5 = b5; a.W4 = W4; a.b4 = b4; a.W2 = W2; a.b2 = b2; a.E = E;
    a.gamma = gamma; a.beta = beta; a.y = y; a.s_out = s_out; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.H = H; a.eps = eps; a.p_pre = 0.f; a.p_post = p_post; a.rng = rng; a.site = site;
    launch_ln<LN_IMAGE, bf16_t, bf16_t>(a, as_stream(stream));
    YT_LAUNCH_CHECK("image_embed_fwd_bf16");
    return 0;
}

extern "C" int ytvln_ln_bwd_bf16(const uint16_t* dy, const uint16_t* s, const float* mean, const float* rstd, const float* gamma, uint16_t* ds,
                                 uint16_t* dx, float* ds_f32, float* partial, int64_t rows, int H, float p_pre, float p_post, const int64_t* rng,
                                 int64_t site, void* stream) {
    YT_REQUIRE(dy && s && mean && rstd && gamma && (ds || ds_f32) && partial, "ln_bwd_bf16: null pointer");
    YT_REQUIRE(ln_shape_ok(H), "ln_bwd_bf16: H=%d unsupported", H);
    YT_REQUIRE(al8(dy) && al8(s) && (!ds || al8(ds)) && al16(gamma) && (!dx || al8(dx)) && (!ds_f32 || al16(ds_f32)), "ln_bwd_bf16: misaligned pointer");
    YT_REQUIRE(!(p_pre > 0.f || p_post > 0.f) || rng, "ln_bwd_bf16: dropout needs rng state");
    YT_REQUIRE(!(p_pre > 0.f && p_post > 0.f), "ln_bwd_bf16: p_pre and p_post both > 0 (the two masks would come from one draw)");
    YT_REQUIRE(!(p_pre > 0.f) || dx, "ln_bwd_bf16: p_pre > 0 needs dx");
    if (rows == 0) return 0;
    LnBwdArgs a;
    a.dy = dy; a.s = s; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.ds = ds; a.dx = dx; a.ds_f32 = ds_f32; a.partial = partial;
    a.rows = rows; a.H = H; a.p_pre = p_pre; a.p_post = p_post; a.rng = rng; a.site = site;
    const int nb = ytvln_ln_bwd_blocks(rows);
    a.rows_per_block = (int)cdiv(rows, nb);
    const int nv = (int)cdiv(H / 4, 64);
    const size_t lds = (size_t)8 * H * sizeof(float);
    hipStream_t st = as_stream(stream);
    if (H % 8 == 0 && al16(dy) && al16(s) && (!ds || al16(ds)) && (!dx || al16(dx))) {          // 16 bytes per lane (and the 16-bit dropout draws of ln_fwd_bf16x8_kernel)
        const int nv8 = (int)cdiv(H / 8, 64);
        if (nv8 <= 1) hipLaunchKernelGGL((ln_bwd_bf16x8_kernel<1>), dim3(nb), dim3(256), lds, st, a);
        else if (nv8 <= 2) hipLaunchKernelGGL((ln_bwd_bf16x8_kernel<2>), dim3(nb), dim3(256), lds, st, a);
        else hipLaunchKernelGGL((ln_bwd_bf16x8_kernel<4>), dim3(nb), dim3(256), lds, st, a);
        YT_LAUNCH_CHECK("ln_bwd_bf16");
        return 0;
    }
    if (nv <= 1) hipLaunchKernelGGL((ln_bwd_kernel<1, bf16_t>), dim3(nb), dim3(256), lds, st, a);
    else if (nv <= 2) hipLaunchKernelGGL((ln_bwd_kernel<2, bf16_t>), dim3(nb), dim3(256), lds, st, a);
    else if (nv <= 4) hipLaunchKernelGGL((ln_bwd_kernel<4, bf16_t>), dim3(nb), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((ln_bwd_kernel<8, bf16_t>), dim3(nb), dim3(256), lds, st, a);
    YT_LAUNCH_CHECK("ln_bwd_bf16");
    return 0;
}

extern "C" int ytvln_act_bwd_bf16(const uint16_t* dy, const uint16_t* aux, uint16_t* dz, int64_t n, int act, void* stream) {
    YT_REQUIRE(dy && aux && dz, "act_bwd_bf16: null pointer");
    YT_REQUIRE(act == YTVLN_EPI_GELU || act == YTVLN_EPI_RELU || act == YTVLN_ACT_SWISH, "act_bwd_bf16: bad act %d", act);
    hipStream_t st = as_stream(stream);
    if (act == YTVLN_ACT_SWISH) {          // any n, any (2-byte) alignment
        YT_REQUIRE(n >= 0, "act_bwd_bf16: n < 0");
        if (n == 0) return 0;
        if (al16(dy) && al16(aux) && al16(dz)) hipLaunchKernelGGL(swish_bwd_bf16_kernel<true>, dim3(ew_grid(n / 8)), dim3(256), 0, st, dy, aux, dz, n);
        else hipLaunchKernelGGL(swish_bwd_bf16_kernel<false>, dim3(ew_grid(n)), dim3(256), 0, st, dy, aux, dz, n);
        YT_LAUNCH_CHECK("act_bwd_bf16");
        return 0;
    }
    YT_REQUIRE(al8(dy) && al8(aux) && al8(dz) && n % 4 == 0, "act_bwd_bf16: pointers must be 8-byte aligned and n a multiple of 4");
    if (n == 0) return 0;
    hipLaunchKernelGGL(act_bwd_bf16_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n / 4, 256), 4096))), dim3(256), 0,
                       st, dy, aux, dz, n / 4, act);
    YT_LAUNCH_CHECK("act_bwd_bf16");
    return 0;
}

extern "C" int ytvln_act_fwd_bf16(const uint16_t* z, uint16_t* y, int64_t n, int act, void* stream) {
    YT_REQUIRE(act == YTVLN_ACT_SWISH, "act_fwd_bf16: bad act %d (swish only: gelu and relu are GEMM epilogues)", act);
    YT_REQUIRE(n >= 0, "act_fwd_bf16: n < 0");
    if (n == 0) return 0;
    YT_REQUIRE(z && y, "act_fwd_bf16: null pointer");
    if (al16(z) && al16(y))
        hipLaunchKernelGGL(swish_fwd_bf16_kernel<true>, dim3(ew_grid(n / 8)), dim3(256), 0, as_stream(stream), z, y, n);
    else
        hipLaunchKernelGGL(swish_fwd_bf16_kernel<false>, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), z, y, n);
    YT_LAUNCH_CHECK("act_fwd_bf16");
    return 0;
}
