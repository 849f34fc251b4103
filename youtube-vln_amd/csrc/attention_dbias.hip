// Gradient with respect to the per-score attention bias (include/ytvln.h: ytvln_attn_dbias_f32 / _bf16).
//
// The bias is added to the final score, so dBias[n,h,i,j] = dS[n,h,i,j] -- the tile the dQ kernel holds in registers and never stores.
// UNFUSED by design (the tuned forward / backward kernels of attention.hip and attention_bf16.hip stay as they are): this launch recomputes
// two of the backward's five products per 32x32 block of scores,
//     S^T = K . Q^T  -> s = fadd(fadd(fmul(q.k, scale), mask), bias), p = exp(s - lse)          dP^T = V . dO^T
//     dS = p * (keep / (1 - p_drop) * dp - delta)          delta = sum_c dO.O, read from the buffer the backward launch wrote
// and stores one score-sized fp32 tensor.
//
// One wave per (output plane, 32 queries, 32 keys, run of reduced problems), no LDS, no barriers: both products have the fragment layout of
// attention.hip (v_mfma_f32_32x32x2_f32, query = lane & 31, 16 keys down the registers in krow order, the other 16 in the partner half-wave) and
// both operands are a lane's OWN row -- key row lane & 31 of K / V as A, query row lane & 31 of Q / dO as B -- with the contraction over the head
// dimension split between the half-waves in 16-byte granules, so every operand is a plain 16-byte global load (bf16 rows: 8 elements, widened
// exactly).  An output dimension of extent 1 (stride 0) is summed over by the wave itself: the reduced (pair, head) problems r = n * heads + h
// are added into the 16 accumulators in ascending r.  Long reductions ([1,1,Tq,Tk] outputs: N * heads problems) are cut into runs of equal
// length, one wave each, written to a workspace and added in ascending run order by a second launch.  No atomics anywhere: bit-reproducible.
#include "common.h"
#include <algorithm>

namespace ytvln {

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define DB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

struct DbiasArgs {
    const void *q, *k, *v, *dctx;                // fp32 or bf16 rows
    const float *mask, *lse, *delta;
    int64_t ldq, ldk, ldv, ldo;
    int N, heads, Tq, Tk, d;
    float scale, p_drop;
    const int64_t* rng; int64_t site;
    const uint64_t* keep;                        // bf16 with dropout: the forward's keep bits (attention_bf16.hip: battn_fwd_body)
    ytvln_attn_bias bias;                        // forward values (ptr NULL: none)
    ytvln_attn_bias out;                         // gradient record
    float* ws;                                   // partial planes [run][plane][Tq][Tk] when runs > 1
    int red_n, red_h;                            // 1: the output has extent 1 there -> summed over
    int R, L, C;                                 // reduced problems per output plane, run length, runs
    int qtiles, ktiles;
};

// one 16-byte granule of a row as fp32 values (zeros when !ok: the granule is past the head dimension and was clamped to a valid address)
template <class T> struct Gran;
template <> struct Gran<float> {
    static constexpr int E = 4;
    __device__ static __forceinline__ void load(float (&x)[4], const float* __restrict__ p, bool ok) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        x[0] = ok ? v.x : 0.f; x[1] = ok ? v.y : 0.f; x[2] = ok ? v.z : 0.f; x[3] = ok ? v.w : 0.f;
    }
};
template <> struct Gran<uint16_t> {
    static constexpr int E = 8;
    __device__ static __forceinline__ void load(float (&x)[8], const uint16_t* __restrict__ p, bool ok) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[2 * e] = ok ? __uint_as_float(w[e] << 16) : 0.f;
            x[2 * e + 1] = ok ? __uint_as_float(w[e] & 0xFFFF0000u) : 0.f;
        }
    }
};

__device__ __forceinline__ int db_krow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// acc[A row = lane & 31 of arow's tile][B row = lane & 31 of brow's tile] = sum over the head dimension; G granules per row, half-wave `half`
// contracts granules [half * steps, half * steps + steps)
template <class T>
__device__ __forceinline__ f32x16 rows_dot(const T* __restrict__ arow, const T* __restrict__ brow, int G, int half) {
    constexpr int E = Gran<T>::E;
    const int steps = (G + 1) >> 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int s = 0; s < steps; ++s) {          // (wave-uniform trip count: every lane issues every matrix instruction)
        const int g = half * steps + s;
        const bool ok = g < G;
        const int gc = min(g, G - 1) * E;
        float a[E], b[E];
        Gran<T>::load(a, arow + gc, ok);
        Gran<T>::load(b, brow + gc, ok);
#pragma unroll
        for (int e = 0; e < E; ++e) acc = DB_MFMA(a[e], b[e], acc);
    }
    return acc;
}

template <class T, bool DROP>
__global__ __launch_bounds__(64) void attn_dbias_kernel(const DbiasArgs a) {
    constexpr bool BF16 = std::is_same<T, uint16_t>::value;
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    int64_t u = blockIdx.x;
    const int kt = (int)(u % a.ktiles); u /= a.ktiles;
    const int qt = (int)(u % a.qtiles); u /= a.qtiles;
    const int c = (int)(u % a.C); u /= a.C;
    const int PH = a.red_h ? 1 : a.heads;
    const int ho = (int)(u % PH), no = (int)(u / PH);
    const int q0 = qt * 32, j0 = kt * 32;
    const int qi = q0 + l31;
    const int qc = min(qi, a.Tq - 1);               // rows past the end repeat the last row: computed, never stored
    const int kc = min(j0 + l31, a.Tk - 1);         // the key row this lane feeds to the matrix instructions
    const int G = a.d / Gran<T>::E;

    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    DropKey key = {0, 0, 0, 0};
    uint32_t thr = 0; float ik = 1.f;
    if (DROP) {
        ik = 1.0f / (1.0f - a.p_drop);
        if (!BF16) { key = make_drop_key(a.rng, a.site); thr = drop_threshold(a.p_drop); }
    }

    const int r0 = c * a.L, r1 = min(a.R, r0 + a.L);
    for (int r = r0; r < r1; ++r) {
        const int n = a.red_n ? (a.red_h ? r / a.heads : r) : no;
        const int h = a.red_h ? (a.red_n ? r % a.heads : r) : ho;
        const int col0 = h * a.d;
        const T* __restrict__ qrow = (const T*)a.q + ((int64_t)n * a.Tq + qc) * a.ldq + col0;
        const T* __restrict__ grow = (const T*)a.dctx + ((int64_t)n * a.Tq + qc) * a.ldo + col0;
        const T* __restrict__ krow = (const T*)a.k + ((int64_t)n * a.Tk + kc) * a.ldk + col0;
        const T* __restrict__ vrow = (const T*)a.v + ((int64_t)n * a.Tk + kc) * a.ldv + col0;
        const int64_t sidx = ((int64_t)n * a.heads + h) * a.Tq + qc;
        const float lse = a.lse[sidx], dl = a.delta[sidx];
        float Bv[16], Mv[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) { Bv[rr] = 0.f; Mv[rr] = 0.f; }
        if (a.bias.ptr) bias_load16(Bv, bias_plane(a.bias, n, h), (uint32_t)(qc * (int)a.bias.stride_q), (int)a.bias.stride_k, j0, half, a.Tk);
        if (a.mask) {
            const float* __restrict__ mrow = a.mask + (int64_t)n * a.Tk;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) Mv[rr] = mrow[min(j0 + db_krow(rr, half), a.Tk - 1)];
        }
        uint64_t km[16];
        if (DROP && BF16) {
            const uint64_t* __restrict__ kb = a.keep + ((((int64_t)n * a.heads + h) * a.qtiles + qt) * a.ktiles + kt) * 16;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) km[rr] = kb[rr];
        }
        const uint32_t dlo = (uint32_t)(((int64_t)n * a.heads + h) * a.Tq + qi);          // score row id of the dropout hash (attention.hip)

        const f32x16 S = rows_dot<T>(krow, qrow, G, half);
        const f32x16 dP = rows_dot<T>(vrow, grow, G, half);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const float sc = __fadd_rn(__fadd_rn(__fmul_rn(S[rr], a.scale), Mv[rr]), Bv[rr]);
            const float p = __expf(sc - lse);
            float dp = dP[rr];
            if (DROP) {
                bool kp;
                if (BF16) kp = ((km[rr] >> lane) & 1ull) != 0;
                else kp = attn_drop_hash((uint32_t)(j0 + db_krow(rr, half)), dlo, key) >= thr;
                dp = kp ? dp * ik : 0.f;
            }
            acc[rr] += p * (dp - dl);
        }
    }

    // destination plane of this wave: the output itself, or its run's partial plane in the workspace
    float* base; int sq, sk;
    if (a.C > 1) {
        const int64_t planes = (int64_t)(a.red_n ? 1 : a.N) * PH;
        base = a.ws + (((int64_t)c * planes + (int64_t)no * PH + ho) * a.Tq) * a.Tk;
        sq = a.Tk; sk = 1;
    } else {
        base = const_cast<float*>(a.out.ptr) + (int64_t)no * a.out.stride_n + (int64_t)ho * a.out.stride_h;
        sq = (int)a.out.stride_q; sk = (int)a.out.stride_k;
    }
    if (qi >= a.Tq) return;
    const bool vec = sk == 1 && (sq & 3) == 0 && ((uintptr_t)base & 15) == 0;          // wave-uniform
    float* row = base + (uint32_t)(qi * sq);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int j = j0 + 8 * g + 4 * half;          // registers 4g .. 4g+3 are four consecutive keys
        if (vec && j + 3 < a.Tk) {
            *reinterpret_cast<float4*>(row + j) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < a.Tk) row[(uint32_t)((j + e) * sk)] = acc[4 * g + e];
        }
    }
}

// out[plane, i, j] = sum over runs c (ascending) of ws[c][plane][i][j]
__global__ __launch_bounds__(256) void attn_dbias_reduce_kernel(const float* __restrict__ ws, int C, int64_t total, const ytvln_attn_bias out,
                                                                 int PH, int Tq, int Tk) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % Tk);
    int64_t t = e / Tk;
    const int i = (int)(t % Tq); t /= Tq;
    const int ho = (int)(t % PH);
    const int64_t no = t / PH;
    float s = ws[e];
    for (int c = 1; c < C; ++c) s += ws[(int64_t)c * total + e];
    const_cast<float*>(out.ptr)[no * out.stride_n + ho * out.stride_h + (int64_t)i * out.stride_q + (int64_t)j * out.stride_k] = s;
}

// runs of the reduction: shapes only (never the device), so a result does not depend on where it was computed
struct DbiasPlan { int red_n, red_h, R, L, C, qtiles, ktiles; int64_t planes; };
static DbiasPlan dbias_plan(const ytvln_attn_bias& out, int N, int heads, int Tq, int Tk) {
    DbiasPlan p;
    p.red_n = out.stride_n == 0; p.red_h = out.stride_h == 0;
    p.R = (p.red_n ? N : 1) * (p.red_h ? heads : 1);
    p.planes = (int64_t)(p.red_n ? 1 : N) * (p.red_h ? 1 : heads);
    p.qtiles = (int)cdiv(Tq, 32); p.ktiles = (int)cdiv(Tk, 32);
    const int64_t units = p.planes * p.qtiles * p.ktiles;
    int64_t C = 1;
    if (p.R > 16) C = std::min<int64_t>(std::max<int64_t>(cdiv(1024, units), 1), cdiv(p.R, 4));      // >= 1024 waves where >= 4 problems per run allow
    p.L = (int)cdiv(p.R, C);
    p.C = (int)cdiv(p.R, p.L);
    return p;
}

static int dbias_launch(bool bf16, const char* who, const ytvln_attn_problem* pr, const ytvln_attn_bias* bias, const ytvln_attn_bias* out,
                        float* workspace, int64_t workspace_elems, int N, int heads, int d, float scale, const int64_t* rng, void* stream) {
    YT_REQUIRE(pr, "%s: null problem", who);
    YT_REQUIRE(out && out->ptr, "%s: null output", who);
    YT_REQUIRE(N > 0 && heads > 0 && d > 0 && pr->Tq > 0 && pr->Tk > 0, "%s: N, heads, d, Tq and Tk must be positive", who);
    YT_REQUIRE(pr->q && pr->k && pr->v && pr->dctx && pr->lse_in && pr->delta, "%s: null pointer (q, k, v, dctx, lse_in, delta)", who);
    const int gran = bf16 ? 8 : 4;
    if (bf16) YT_REQUIRE(d == 64 || d == 128, "%s: head dim %d unsupported (64 or 128)", who, d);
    else YT_REQUIRE(d % 4 == 0 && d <= 128, "%s: head dim %d unsupported (multiple of 4, <= 128)", who, d);
    YT_REQUIRE(pr->ldq % gran == 0 && pr->ldk % gran == 0 && pr->ldv % gran == 0 && pr->ldo % gran == 0,
               "%s: leading dimensions must be multiples of %d", who, gran);
    YT_REQUIRE((((uintptr_t)pr->q | (uintptr_t)pr->k | (uintptr_t)pr->v | (uintptr_t)pr->dctx) & 15) == 0, "%s: q/k/v/dctx must be 16-byte aligned", who);
    YT_REQUIRE(pr->Tq <= 8192 && pr->Tk <= 8192, "%s: sequence too long", who);
    YT_REQUIRE(pr->p_drop >= 0.f && pr->p_drop < 1.f, "%s: p_drop out of range", who);
    const bool drop = pr->p_drop > 0.f;
    if (bf16) YT_REQUIRE(!drop || (pr->keep && ((uintptr_t)pr->keep & 127) == 0), "%s: dropout needs the keep buffer the forward wrote (128-byte aligned)", who);
    else YT_REQUIRE(!drop || rng, "%s: dropout needs rng state", who);
    if (int rc = check_bias(who, *out, pr->Tq, pr->Tk)) return rc;
    DbiasArgs a{};
    if (bias && bias->ptr) {
        if (int rc = check_bias(who, *bias, pr->Tq, pr->Tk)) return rc;
        a.bias = *bias;
    }
    const DbiasPlan pl = dbias_plan(*out, N, heads, pr->Tq, pr->Tk);
    const int64_t plane_elems = pl.planes * pr->Tq * pr->Tk;
    const int64_t need = pl.C > 1 ? (int64_t)pl.C * plane_elems : 0;
    YT_REQUIRE(need == 0 || (workspace && workspace_elems >= need), "%s: workspace too small (%lld floats, need %lld: ytvln_attn_dbias_workspace_elems)",
               who, (long long)(workspace ? workspace_elems : 0), (long long)need);
    YT_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    const int64_t grid = (int64_t)pl.C * pl.planes * pl.qtiles * pl.ktiles;
    YT_REQUIRE(grid < (1ll << 31), "%s: launch too large", who);

    a.q = pr->q; a.k = pr->k; a.v = pr->v; a.dctx = pr->dctx; a.mask = pr->mask; a.lse = pr->lse_in; a.delta = pr->delta;
    a.ldq = pr->ldq; a.ldk = pr->ldk; a.ldv = pr->ldv; a.ldo = pr->ldo;
    a.N = N; a.heads = heads; a.Tq = pr->Tq; a.Tk = pr->Tk; a.d = d; a.scale = scale; a.p_drop = pr->p_drop;
    a.rng = rng; a.site = pr->site; a.keep = (const uint64_t*)pr->keep;
    a.out = *out; a.ws = workspace;
    a.red_n = pl.red_n; a.red_h = pl.red_h; a.R = pl.R; a.L = pl.L; a.C = pl.C; a.qtiles = pl.qtiles; a.ktiles = pl.ktiles;
    hipStream_t s = as_stream(stream);
    const dim3 g((unsigned)grid), b(64);
    if (bf16) {
        if (drop) hipLaunchKernelGGL((attn_dbias_kernel<uint16_t, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((attn_dbias_kernel<uint16_t, false>), g, b, 0, s, a);
    } else {
        if (drop) hipLaunchKernelGGL((attn_dbias_kernel<float, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((attn_dbias_kernel<float, false>), g, b, 0, s, a);
    }
    YT_LAUNCH_CHECK(who);
    if (pl.C > 1) {
        hipLaunchKernelGGL(attn_dbias_reduce_kernel, dim3((unsigned)cdiv(plane_elems, 256)), dim3(256), 0, s, workspace, pl.C, plane_elems, *out,
                           pl.red_h ? 1 : heads, pr->Tq, pr->Tk);
        YT_LAUNCH_CHECK(who);
    }
    return 0;
}

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_attn_dbias_chunks(const ytvln_attn_bias* out, int N, int heads, int Tq, int Tk) {
    YT_REQUIRE(out && N > 0 && heads > 0 && Tq > 0 && Tk > 0, "attn_dbias_chunks: null record or empty problem");
    return dbias_plan(*out, N, heads, Tq, Tk).C;
}

extern "C" int64_t ytvln_attn_dbias_workspace_elems(const ytvln_attn_bias* out, int N, int heads, int Tq, int Tk) {
    YT_REQUIRE(out && N > 0 && heads > 0 && Tq > 0 && Tk > 0, "attn_dbias_workspace_elems: null record or empty problem");
    const DbiasPlan pl = dbias_plan(*out, N, heads, Tq, Tk);
    return pl.C > 1 ? (int64_t)pl.C * pl.planes * Tq * Tk : 0;
}

extern "C" int ytvln_attn_dbias_f32(const ytvln_attn_problem* p, const ytvln_attn_bias* bias, const ytvln_attn_bias* out, float* workspace,
                                    int64_t workspace_elems, int N, int heads, int d, float scale, const int64_t* rng, void* stream) {
    return dbias_launch(false, "attn_dbias_f32", p, bias, out, workspace, workspace_elems, N, heads, d, scale, rng, stream);
}

extern "C" int ytvln_attn_dbias_bf16(const ytvln_attn_problem* p, const ytvln_attn_bias* bias, const ytvln_attn_bias* out, float* workspace,
                                     int64_t workspace_elems, int N, int heads, int d, float scale, const int64_t* rng, void* stream) {
    return dbias_launch(true, "attn_dbias_bf16", p, bias, out, workspace, workspace_elems, N, heads, d, scale, rng, stream);
}
