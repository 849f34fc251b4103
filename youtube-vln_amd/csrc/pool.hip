// Ragged frame pool -> padded batch in one launch.  The feature readers return variable-length frames
// (n rows of 2048 features, 11 location columns, 1601 class probabilities, n different for every frame); the reference pads every frame to
// `boxes` rows on the host, per frame and per step (utils/dataset/all_dataset.py:294-345).  Here the loader ships the real rows once
// (pool_* [pool_rows, .] + offsets [pool_frames + 1]) and this kernel writes the four padded [slots * boxes, .] tensors of the step,
// option expansion (index [slots], -1 = padding frame) included: every output element is written exactly once, real rows copied, the
// rest exact zeros, column 11 of the boxes = the position of the frame inside its option (all_dataset.py:314 and :331, padding frames too).
//
// Work split: for one slot the source is ONE contiguous run of n pool rows and the destination ONE contiguous [boxes, .] block, so a piece
// of `group` consecutive boxes of a slot is two flat runs per tensor: a copy of the real part and a zero fill of the rest.  One workgroup
// takes one (slot, piece): 448 slots of 527 KB each become 4032 pieces of 59 KB at the bench's shape.  A run goes out in 16-byte stores from
// the first 16-byte boundary of the destination on; the loads are 16 bytes wide where the source is aligned at that point too and four
// dwords otherwise (rows of C = 1601 floats sit on 4-byte boundaries on both sides: most probs runs take that form).  Nothing is read
// outside [0, pool_rows) rows whatever `index` and `offsets` hold: the range check on the pool frame comes before the read of its offsets,
// the check of the offsets before any read of a row.
#include "common.h"
#include <algorithm>

namespace ytvln {

constexpr int POOL_THREADS = 256;
constexpr int POOL_UNROLL = 4;          // 16-byte loads in flight per lane before the first store

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// dst[0, count) = src[0, count).  Any alignment (both at least 4 bytes), whole workgroup.
__device__ __forceinline__ void run_copy(float* __restrict__ dst, const float* __restrict__ src, int64_t count, int tid) {
    if (count <= 0) return;
    const int64_t head = min64(count, (int64_t)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3));
    if (tid < head) dst[tid] = src[tid];
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
    const float* __restrict__ s = src + head;
    const int64_t nvec = (count - head) >> 2;
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s);
        for (int64_t i = tid; i < nvec; i += POOL_THREADS * POOL_UNROLL) {
            float4 v[POOL_UNROLL];
#pragma unroll
            for (int u = 0; u < POOL_UNROLL; ++u)
                if (i + u * POOL_THREADS < nvec) v[u] = s4[i + u * POOL_THREADS];
#pragma unroll
            for (int u = 0; u < POOL_UNROLL; ++u)
                if (i + u * POOL_THREADS < nvec) d4[i + u * POOL_THREADS] = v[u];
        }
    } else {
        for (int64_t i = tid; i < nvec; i += POOL_THREADS * POOL_UNROLL) {
            float4 v[POOL_UNROLL];
#pragma unroll
            for (int u = 0; u < POOL_UNROLL; ++u) {
                const int64_t e = 4 * (i + u * POOL_THREADS);
                if (i + u * POOL_THREADS < nvec) v[u] = make_float4(s[e], s[e + 1], s[e + 2], s[e + 3]);
            }
#pragma unroll
            for (int u = 0; u < POOL_UNROLL; ++u)
                if (i + u * POOL_THREADS < nvec) d4[i + u * POOL_THREADS] = v[u];
        }
    }
    const int64_t done = head + 4 * nvec;
    if (tid < count - done) dst[done + tid] = src[done + tid];
}

// dst[0, count) = value
__device__ __forceinline__ void run_fill(float* __restrict__ dst, int64_t count, float value, int tid) {
    if (count <= 0) return;
    const int64_t head = min64(count, (int64_t)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3));
    if (tid < head) dst[tid] = value;
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
    const int64_t nvec = (count - head) >> 2;
    for (int64_t i = tid; i < nvec; i += POOL_THREADS) d4[i] = make_float4(value, value, value, value);
    const int64_t done = head + 4 * nvec;
    if (tid < count - done) dst[done + tid] = value;
}

// dst[0, count) = 0
__device__ __forceinline__ void run_zero(float* __restrict__ dst, int64_t count, int tid) { run_fill(dst, count, 0.f, tid); }

__global__ __launch_bounds__(POOL_THREADS) void expand_ragged_kernel(
    const float* __restrict__ pool_features, const float* __restrict__ pool_loc, const float* __restrict__ pool_probs,
    const int64_t* __restrict__ offsets, int64_t pool_frames, int64_t pool_rows, const int64_t* __restrict__ index, int64_t slots, int frames,
    int boxes, int F, int L, int C, int group, int pieces, float* __restrict__ out_features, float* __restrict__ out_boxes,
    float* __restrict__ out_probs, int64_t* __restrict__ out_masks, unsigned long long* __restrict__ bad) {
    const int tid = threadIdx.x;
    const int64_t items = slots * (int64_t)pieces;
    // consecutive items on one XCD: the K options of a dataset item mostly show the same pool frames, and their slots are neighbours, so the
    // re-reads of a frame find it in that XCD's L2 (measured: 1.5-3 % at 56 pairs x 288 regions, 0.8 % at 224 x 576, profiles/ragged_pool_xcd_ab.json)
    for (int64_t item = xcd_remap((int)blockIdx.x, (int)gridDim.x); item < items; item += gridDim.x) {
        const int64_t s = item / pieces;
        const int piece = (int)(item - s * pieces);
        const int j0 = piece * group, j1 = (int)min64(boxes, (int64_t)j0 + group);          // this workgroup's boxes of the slot
        const int64_t p = index[s];
        int64_t first = 0;
        int n = 0;
        bool is_bad = p < -1 || p >= pool_frames;
        if (p >= 0 && p < pool_frames) {                                         // the range check comes before any read of offsets
            const int64_t a = offsets[p], b = offsets[p + 1];
            if (a >= 0 && a <= b && b <= pool_rows) {
                first = a;
                n = (int)min64(b - a, boxes);
            } else {
                is_bad = true;
            }
        }
        if (bad && is_bad && piece == 0 && tid == 0) atomicAdd(bad, 1ull);
        const int real = n > j0 ? (n < j1 ? n : j1) - j0 : 0;                      // rows of this piece that exist in the pool
        const int64_t row0 = s * (int64_t)boxes + j0, src0 = first + j0;         // src0 is used only when real > 0: then src0 + real <= pool_rows
        const int rows = j1 - j0;

        run_copy(out_features + row0 * F, pool_features + src0 * F, (int64_t)real * F, tid);
        run_zero(out_features + (row0 + real) * F, (int64_t)(rows - real) * F, tid);
        if (out_probs) {
            run_copy(out_probs + row0 * C, pool_probs + src0 * C, (int64_t)real * C, tid);
            run_zero(out_probs + (row0 + real) * C, (int64_t)(rows - real) * C, tid);
        }
        const float pos = (float)(s % frames);
        for (int64_t e = tid; e < (int64_t)rows * 12; e += POOL_THREADS) {
            const int r = (int)(e / 12), c = (int)(e - (int64_t)r * 12);
            float v = 0.f;
            if (c == 11) v = pos;
            else if (r < real && c < L) v = pool_loc[(src0 + r) * L + c];
            out_boxes[row0 * 12 + e] = v;
        }
        for (int r = tid; r < rows; r += POOL_THREADS) out_masks[row0 + r] = r < real ? 1 : 0;
    }
}

// ---- raw-record pool: the readers' global row and box geometry on the device --------------------------------------------------------
// The pool holds decoded records as they come off the disk (pool_geom [rows, 8] = x1, y1, x2, y2 in pixels, image width, image height,
// featureHeading, featureElevation); what the reference's readers compute per frame on the host (features_reader.py:91-124, :153-179,
// :258-341) happens here: the mean row in pool_global_rows_kernel, the normalised boxes and the orientation columns in the expansion.

constexpr int GLOBAL_THREADS = 64;      // one wave per (frame, column chunk): 8 chunks per frame at F = 2048 in the 16-byte form
constexpr int GLOBAL_UNROLL = 8;        // rows in flight per lane before the first add

// out[p, c] = (((0 + x[a, c]) + x[a+1, c]) + ... + x[b-1, c]) / (float)(b - a), rows a = offsets[p] .. b - 1 in row order: numpy's order for
// mean(axis=0) of a C-contiguous [n, F] array, and part of the contract (no tree, no wave reduction, no atomics).  A lane owns V adjacent
// columns (V = 4: 16-byte loads and stores) and walks the frame's rows, GLOBAL_UNROLL independent loads ahead of the adds that consume them
// in order.  Zero for an empty frame and for offsets out of order or out of range; nothing outside rows [0, pool_rows) is read.
template <int V>
__global__ __launch_bounds__(GLOBAL_THREADS) void pool_global_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ offsets,
                                                                           int64_t pool_frames, int64_t pool_rows, int F, int chunks,
                                                                           float* __restrict__ out) {
    struct alignas(4 * V) Vec { float v[V]; };
    const int64_t items = pool_frames * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t p = item / chunks;
        const int64_t c = ((item - p * chunks) * GLOBAL_THREADS + threadIdx.x) * V;
        if (c >= F) continue;
        const int64_t a = offsets[p], b = offsets[p + 1];
        Vec acc;
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
        if (a >= 0 && a < b && b <= pool_rows) {
            const float* __restrict__ src = x + a * F + c;
            const int64_t n = b - a;
            int64_t r = 0;
            for (; r + GLOBAL_UNROLL <= n; r += GLOBAL_UNROLL) {
                Vec v[GLOBAL_UNROLL];
#pragma unroll
                for (int u = 0; u < GLOBAL_UNROLL; ++u) v[u] = *reinterpret_cast<const Vec*>(src + (r + u) * F);
#pragma unroll
                for (int u = 0; u < GLOBAL_UNROLL; ++u)
#pragma unroll
                    for (int k = 0; k < V; ++k) acc.v[k] += v[u].v[k];
            }
            for (; r < n; ++r) {
                const Vec v = *reinterpret_cast<const Vec*>(src + r * F);
#pragma unroll
                for (int k = 0; k < V; ++k) acc.v[k] += v.v[k];
            }
            const float count = (float)n;
#pragma unroll
            for (int k = 0; k < V; ++k) acc.v[k] = acc.v[k] / count;
        }
        *reinterpret_cast<Vec*>(out + p * F + c) = acc;
    }
}

// One element of the 11 location columns of a REAL row of a slot (features_reader.py:91-124 and :258-282).  g = nullptr: the global region
// (row 0 of the slot), else the row's 8 geometry values.  view = nullptr: the photo readers (orientation columns 1, global 0,1,0,1,0,1),
// else (heading, next heading) of the slot: sin / cos in double on the fp32 angle, rounded once.  All box arithmetic is fp32 with correctly
// rounded division, as numpy does it; no contraction (there is no multiply-add here to contract, the pragma keeps it so).
__device__ __forceinline__ float record_location(const float* __restrict__ g, const double* __restrict__ view, int c) {
#pragma clang fp contract(off)
    if (c < 5) {
        if (!g) return c < 2 ? 0.f : 1.f;
        const float w = g[4], h = g[5];
        if (c < 4) return g[c] / ((c & 1) ? h : w);
        return ((g[2] - g[0]) * (g[3] - g[1])) / (w * h);
    }
    if (!view) return (g || (c & 1) == 0) ? 1.f : 0.f;
    double angle;
    if (c == 7 || c == 8) {
        angle = g ? (double)g[7] : 0.0;
    } else {
        const double turn = view[c < 7 ? 0 : 1];
        angle = g ? (double)(g[6] - (float)turn) : -turn;        // fp32 array minus a Python float: the float is rounded to fp32 first
    }
    double s, co;
    sincos(angle, &s, &co);
    return (float)((c & 1) ? s : co);
}

// expand_ragged_kernel for the raw-record pool: row 0 of a slot is the global region of its frame (pool_global row, uniform probabilities,
// whole-image box), rows 1 .. n-1 are source rows 0 .. n-2 with the box geometry computed from pool_geom; n = min(rows of the frame + 1,
// boxes).  An empty frame is BAD here (the reference raises "Features could not be correctly read").  Same work split, same order of
// the checks: the frame's range before its offsets, the offsets before any row of the pool or of pool_global.
__global__ __launch_bounds__(POOL_THREADS) void expand_records_kernel(
    const float* __restrict__ pool_features, const float* __restrict__ pool_geom, const float* __restrict__ pool_probs,
    const float* __restrict__ pool_global, const int64_t* __restrict__ offsets, int64_t pool_frames, int64_t pool_rows,
    const int64_t* __restrict__ index, const double* __restrict__ view, int64_t slots, int frames, int boxes, int F, int C, int group, int pieces,
    float* __restrict__ out_features, float* __restrict__ out_boxes, float* __restrict__ out_probs, int64_t* __restrict__ out_masks,
    unsigned long long* __restrict__ bad) {
    const int tid = threadIdx.x;
    const int64_t items = slots * (int64_t)pieces;
    const float uniform = (float)(1.0 / (double)C);
    for (int64_t item = xcd_remap((int)blockIdx.x, (int)gridDim.x); item < items; item += gridDim.x) {
        const int64_t s = item / pieces;
        const int piece = (int)(item - s * pieces);
        const int j0 = piece * group, j1 = (int)min64(boxes, (int64_t)j0 + group);
        const int64_t p = index[s];
        int64_t first = 0;
        int n = 0;
        bool is_bad = p < -1 || p >= pool_frames;
        if (p >= 0 && p < pool_frames) {
            const int64_t a = offsets[p], b = offsets[p + 1];
            if (a >= 0 && a < b && b <= pool_rows) {
                first = a;
                n = (int)min64(b - a + 1, boxes);
            } else {
                is_bad = true;
            }
        }
        if (bad && is_bad && piece == 0 && tid == 0) atomicAdd(bad, 1ull);
        const int real = n > j0 ? (n < j1 ? n : j1) - j0 : 0;                      // rows of this piece that are real
        const int lead = (real > 0 && j0 == 0) ? 1 : 0;                            // ... of which the global region
        const int64_t row0 = s * (int64_t)boxes + j0, src0 = first + j0 + lead - 1;   // slot row j shows source row j - 1; used only when real > lead
        const int rows = j1 - j0;

        if (lead) run_copy(out_features + row0 * F, pool_global + p * F, F, tid);
        run_copy(out_features + (row0 + lead) * F, pool_features + src0 * F, (int64_t)(real - lead) * F, tid);
        run_zero(out_features + (row0 + real) * F, (int64_t)(rows - real) * F, tid);
        if (out_probs) {
            if (lead) run_fill(out_probs + row0 * C, C, uniform, tid);
            run_copy(out_probs + (row0 + lead) * C, pool_probs + src0 * C, (int64_t)(real - lead) * C, tid);
            run_zero(out_probs + (row0 + real) * C, (int64_t)(rows - real) * C, tid);
        }
        const float pos = (float)(s % frames);
        const double* __restrict__ turn = view ? view + 2 * s : nullptr;
        for (int64_t e = tid; e < (int64_t)rows * 12; e += POOL_THREADS) {
            const int r = (int)(e / 12), c = (int)(e - (int64_t)r * 12);
            float v = 0.f;
            if (c == 11) v = pos;
            else if (r < real) v = record_location(r < lead ? nullptr : pool_geom + (src0 + (r - lead)) * 8, turn, c);
            out_boxes[row0 * 12 + e] = v;
        }
        for (int r = tid; r < rows; r += POOL_THREADS) out_masks[row0 + r] = r < real ? 1 : 0;
    }
}

// ---- the expansions with the region masking and the bf16 rounding in the same launch ---------------------------------------------------
// What mask_batch does to the padded batch afterwards (randomize_regions_kernel of batch.hip: targets = probs or 1 / C per row, about 1.35 %
// of the feature rows zeroed) and what the bf16-resident model does to the features after that (cast_f32_bf16_kernel) are decisions per ROW
// and a rounding per VALUE: a workgroup settles the decisions of the rows of its piece first (one byte each in LDS), then walks the piece in
// maximal runs of consecutive rows with the same source and decision.  85 % of the real rows are unselected, so most runs are as long as
// those of the kernels above, and the padded probabilities -- written and read once more today only to feed a select -- never exist: pool
// probabilities are read for the selected rows only.

constexpr int POOL_MAX_GROUP = 1024;    // rows per piece the decisions have room for (the entry points' pieces hold at most 32768 / 48 rows)
constexpr int DEC_SEL = 1, DEC_ZERO = 2;

__device__ __forceinline__ uint4 pack_bf16x8(const float4& a, const float4& b) {
    return make_uint4(f2bf(a.x) | (f2bf(a.y) << 16), f2bf(a.z) | (f2bf(a.w) << 16), f2bf(b.x) | (f2bf(b.y) << 16), f2bf(b.z) | (f2bf(b.w) << 16));
}

// run_copy with a bf16 destination: dst[0, count) = bf16(src[0, count)), each value rounded once (f2bf).  dst on any 2-byte, src on any
// 4-byte boundary; 16-byte stores of eight values from the first 16-byte boundary of the destination on, the loads two 16-byte ones where the
// source is aligned at that point and eight dwords otherwise.
__device__ __forceinline__ void run_copy(uint16_t* __restrict__ dst, const float* __restrict__ src, int64_t count, int tid) {
    if (count <= 0) return;
    const int64_t head = min64(count, (int64_t)((8 - ((reinterpret_cast<uintptr_t>(dst) >> 1) & 7)) & 7));
    if (tid < head) dst[tid] = (uint16_t)f2bf(src[tid]);
    uint4* __restrict__ d8 = reinterpret_cast<uint4*>(dst + head);
    const float* __restrict__ s = src + head;
    const int64_t nvec = (count - head) >> 3;
    constexpr int U = POOL_UNROLL / 2;          // the same bytes in flight per lane as the fp32 form
    if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s);
        for (int64_t i = tid; i < nvec; i += POOL_THREADS * U) {
            float4 v[U][2];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i + u * POOL_THREADS < nvec) {
                    v[u][0] = s4[2 * (i + u * POOL_THREADS)];
                    v[u][1] = s4[2 * (i + u * POOL_THREADS) + 1];
                }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i + u * POOL_THREADS < nvec) d8[i + u * POOL_THREADS] = pack_bf16x8(v[u][0], v[u][1]);
        }
    } else {
        for (int64_t i = tid; i < nvec; i += POOL_THREADS * U) {
            float4 v[U][2];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t e = 8 * (i + u * POOL_THREADS);
                if (i + u * POOL_THREADS < nvec) {
                    v[u][0] = make_float4(s[e], s[e + 1], s[e + 2], s[e + 3]);
                    v[u][1] = make_float4(s[e + 4], s[e + 5], s[e + 6], s[e + 7]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i + u * POOL_THREADS < nvec) d8[i + u * POOL_THREADS] = pack_bf16x8(v[u][0], v[u][1]);
        }
    }
    const int64_t done = head + 8 * nvec;
    if (tid < count - done) dst[done + tid] = (uint16_t)f2bf(src[done + tid]);
}

// dst[0, count) = 0 in bf16
__device__ __forceinline__ void run_zero(uint16_t* __restrict__ dst, int64_t count, int tid) {
    if (count <= 0) return;
    const int64_t head = min64(count, (int64_t)((8 - ((reinterpret_cast<uintptr_t>(dst) >> 1) & 7)) & 7));
    if (tid < head) dst[tid] = 0;
    uint4* __restrict__ d8 = reinterpret_cast<uint4*>(dst + head);
    const int64_t nvec = (count - head) >> 3;
    for (int64_t i = tid; i < nvec; i += POOL_THREADS) d8[i] = make_uint4(0u, 0u, 0u, 0u);
    const int64_t done = head + 8 * nvec;
    if (tid < count - done) dst[done + tid] = 0;
}

struct MaskedExpansion {
    const float* pool_features; const float* pool_loc; const float* pool_geom; const float* pool_probs; const float* pool_global;
    const int64_t* offsets; int64_t pool_frames, pool_rows;
    const int64_t* index; const double* view; int64_t slots;
    int frames, boxes, F, L, C, group, pieces;
    const float* p; const int64_t* rng; int64_t site;          // the draws: explicit, or Philox (rng, site), or neither (masking off)
    void* out_features; float* out_boxes; float* out_targets; int64_t* out_masks; int64_t* out_targets_mask;
    unsigned long long* bad;
};

// RECORDS = false: expand_ragged_kernel's rows, true: expand_records_kernel's (global region first, geometry computed); FT = the feature
// output's element.  Same work split, same XCD remap, same order of the checks as those two.
template <bool RECORDS, typename FT>
__global__ __launch_bounds__(POOL_THREADS) void expand_masked_kernel(const MaskedExpansion a) {
    __shared__ unsigned char s_dec[POOL_MAX_GROUP];
    const int tid = threadIdx.x;
    const int boxes = a.boxes, F = a.F, C = a.C, pieces = a.pieces, group = a.group;
    FT* __restrict__ out_features = static_cast<FT*>(a.out_features);
    float* __restrict__ out_targets = a.out_targets;
    const bool masking = a.p || a.rng;
    DropKey key = {0, 0, 0, 0};
    if (!a.p && a.rng) key = make_drop_key(a.rng, a.site);
    const float uni = C > 0 ? 1.0f / (float)C : 0.f;                            // what randomize_regions_kernel writes on an unselected row
    const float uni_global = C > 0 ? (float)(1.0 / (double)C) : 0.f;            // the probabilities of a record slot's global region
    const int64_t items = a.slots * (int64_t)pieces;
    for (int64_t item = xcd_remap((int)blockIdx.x, (int)gridDim.x); item < items; item += gridDim.x) {
        const int64_t s = item / pieces;
        const int piece = (int)(item - s * pieces);
        const int j0 = piece * group, j1 = (int)min64(boxes, (int64_t)j0 + group);
        const int64_t p = a.index[s];
        int64_t first = 0;
        int n = 0;
        bool is_bad = p < -1 || p >= a.pool_frames;
        if (p >= 0 && p < a.pool_frames) {                                       // the range check comes before any read of offsets
            const int64_t lo = a.offsets[p], hi = a.offsets[p + 1];
            if (lo >= 0 && (RECORDS ? lo < hi : lo <= hi) && hi <= a.pool_rows) {
                first = lo;
                n = (int)min64(hi - lo + (RECORDS ? 1 : 0), boxes);
            } else {
                is_bad = true;
            }
        }
        if (a.bad && is_bad && piece == 0 && tid == 0) atomicAdd(a.bad, 1ull);
        const int real = n > j0 ? (n < j1 ? n : j1) - j0 : 0;                      // rows of this piece that are real
        const int lead = (RECORDS && real > 0 && j0 == 0) ? 1 : 0;                 // ... of which the global region
        const int64_t row0 = s * (int64_t)boxes + j0;
        const int64_t src0 = first + j0 - (RECORDS ? 1 : 0);                       // piece row r >= lead shows pool row src0 + r; used only when real > lead
        const int rows = j1 - j0;

        // the decisions of the piece's rows; q = draw * mask as randomize_regions_kernel forms it, so a row that is not real is never selected
        for (int r = tid; r < rows; r += POOL_THREADS) {
            const int m = r < real ? 1 : 0;
            int d = 0;
            if (masking) {
                const float draw = a.p ? a.p[row0 + r] : u01(drop_bits(key, (uint64_t)(row0 + r)).x);
                const float q = draw * (float)m;
                d = (q >= thr_mask() ? DEC_SEL : 0) | (q >= thr_reg_zero() ? DEC_ZERO : 0);
            }
            s_dec[r] = (unsigned char)d;
            a.out_masks[row0 + r] = m;
            if (a.out_targets_mask) a.out_targets_mask[row0 + r] = d & DEC_SEL;
        }
        __syncthreads();

        // features: runs of rows that are copied (real and not zeroed) and runs of zeros (zeroed or padding)
        {
            int r = 0;
            if (lead) {
                if (s_dec[0] & DEC_ZERO) run_zero(out_features + row0 * F, F, tid);
                else run_copy(out_features + row0 * F, a.pool_global + p * F, F, tid);
                r = 1;
            }
            while (r < rows) {
                const bool copy = r < real && !(s_dec[r] & DEC_ZERO);
                int e = r + 1;
                while (e < rows && (e < real && !(s_dec[e] & DEC_ZERO)) == copy) ++e;
                if (copy) run_copy(out_features + (row0 + r) * F, a.pool_features + (src0 + r) * F, (int64_t)(e - r) * F, tid);
                else run_zero(out_features + (row0 + r) * F, (int64_t)(e - r) * F, tid);
                r = e;
            }
        }
        // targets: runs of selected rows (copies of the pool's probabilities) and runs of 1 / C
        if (out_targets) {
            int r = 0;
            if (lead) {
                run_fill(out_targets + row0 * C, C, (s_dec[0] & DEC_SEL) ? uni_global : uni, tid);
                r = 1;
            }
            while (r < rows) {
                const bool sel = (s_dec[r] & DEC_SEL) != 0;
                int e = r + 1;
                while (e < rows && ((s_dec[e] & DEC_SEL) != 0) == sel) ++e;
                if (sel) run_copy(out_targets + (row0 + r) * C, a.pool_probs + (src0 + r) * C, (int64_t)(e - r) * C, tid);
                else run_fill(out_targets + (row0 + r) * C, (int64_t)(e - r) * C, uni, tid);
                r = e;
            }
        }
        const float pos = (float)(s % a.frames);
        const double* __restrict__ turn = (RECORDS && a.view) ? a.view + 2 * s : nullptr;
        for (int64_t e = tid; e < (int64_t)rows * 12; e += POOL_THREADS) {
            const int r = (int)(e / 12), c = (int)(e - (int64_t)r * 12);
            float v = 0.f;
            if (c == 11) v = pos;
            else if (r < real) {
                if (RECORDS) v = record_location(r < lead ? nullptr : a.pool_geom + (src0 + r) * 8, turn, c);
                else if (c < a.L) v = a.pool_loc[(src0 + r) * a.L + c];
            }
            a.out_boxes[row0 * 12 + e] = v;
        }
        __syncthreads();                  // s_dec is rewritten by the next item
    }
}

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_expand_ragged_f32(const float* pool_features, const float* pool_loc, const float* pool_probs, const int64_t* offsets,
                                       int64_t pool_frames, int64_t pool_rows, const int64_t* index, int64_t slots, int frames, int boxes,
                                       int F, int L, int C, float* out_features, float* out_boxes, float* out_probs, int64_t* out_masks,
                                       int64_t* bad, void* stream) {
    YT_REQUIRE(offsets && index && out_features && out_boxes && out_masks, "expand_ragged: null buffer");
    YT_REQUIRE(pool_frames >= 0 && pool_rows >= 0 && slots >= 0 && boxes > 0 && F >= 0 && L >= 0 && C >= 0,
               "expand_ragged: negative size (pool_frames %lld, pool_rows %lld, slots %lld, boxes %d, F %d, L %d, C %d)", (long long)pool_frames,
               (long long)pool_rows, (long long)slots, boxes, F, L, C);
    YT_REQUIRE(frames > 0 && slots % frames == 0, "expand_ragged: slots (%lld) must be a multiple of frames (%d > 0)", (long long)slots, frames);
    YT_REQUIRE(L <= 11, "expand_ragged: L = %d location columns exceed the 11 the boxes hold next to the position column", L);
    YT_REQUIRE((pool_probs != nullptr) == (out_probs != nullptr), "expand_ragged: pool_probs and out_probs go together (both given or both null)");
    YT_REQUIRE(pool_rows == 0 || (pool_features && pool_loc), "expand_ragged: null pool buffer");
    const int64_t widest = std::max<int64_t>(std::max(F, C), 12);
    YT_REQUIRE(slots <= INT64_MAX / boxes && slots * boxes <= INT64_MAX / widest && pool_rows <= INT64_MAX / widest,
               "expand_ragged: element counts overflow");
    if (slots == 0) return 0;
    // pieces of about 32 KB, at least four boxes: enough workgroups to fill the chip, runs long enough to amortise their heads and tails
    const int64_t row_bytes = 4 * ((int64_t)F + 12 + (out_probs ? C : 0));
    const int want = (int)std::min<int64_t>(boxes, std::max<int64_t>(4, 32768 / row_bytes));
    const int pieces = (int)cdiv(boxes, want);
    const int group = (int)cdiv(boxes, pieces);
    YT_REQUIRE(slots <= INT64_MAX / pieces, "expand_ragged: element counts overflow");
    const unsigned grid = (unsigned)std::min<int64_t>(slots * pieces, 1 << 20);
    hipLaunchKernelGGL(expand_ragged_kernel, dim3(grid), dim3(POOL_THREADS), 0, as_stream(stream), pool_features, pool_loc, pool_probs, offsets,
                       pool_frames, pool_rows, index, slots, frames, boxes, F, L, C, group, pieces, out_features, out_boxes, out_probs, out_masks,
                       reinterpret_cast<unsigned long long*>(bad));
    YT_LAUNCH_CHECK("expand_ragged");
    return 0;
}

extern "C" int ytvln_pool_global_rows_f32(const float* pool_features, const int64_t* offsets, int64_t pool_frames, int64_t pool_rows, int F,
                                          float* out_global, void* stream) {
    YT_REQUIRE(offsets && out_global, "pool_global_rows: null buffer");
    YT_REQUIRE(pool_frames >= 0 && pool_rows >= 0 && F >= 0, "pool_global_rows: negative size (pool_frames %lld, pool_rows %lld, F %d)",
               (long long)pool_frames, (long long)pool_rows, F);
    YT_REQUIRE(pool_rows == 0 || pool_features, "pool_global_rows: null pool buffer");
    YT_REQUIRE(F == 0 || (pool_frames <= INT64_MAX / F && pool_rows <= INT64_MAX / F), "pool_global_rows: element counts overflow");
    if (pool_frames == 0 || F == 0) return 0;
    // 16-byte loads and stores where both bases and the row pitch allow them, one column per lane otherwise
    const bool wide = F % 4 == 0 && ((reinterpret_cast<uintptr_t>(pool_features) | reinterpret_cast<uintptr_t>(out_global)) & 15) == 0;
    const int chunks = (int)cdiv(F, GLOBAL_THREADS * (wide ? 4 : 1));
    YT_REQUIRE(pool_frames <= INT64_MAX / chunks, "pool_global_rows: element counts overflow");
    const unsigned grid = (unsigned)std::min<int64_t>(pool_frames * chunks, 1 << 20);
    if (wide)
        hipLaunchKernelGGL(pool_global_rows_kernel<4>, dim3(grid), dim3(GLOBAL_THREADS), 0, as_stream(stream), pool_features, offsets, pool_frames,
                           pool_rows, F, chunks, out_global);
    else
        hipLaunchKernelGGL(pool_global_rows_kernel<1>, dim3(grid), dim3(GLOBAL_THREADS), 0, as_stream(stream), pool_features, offsets, pool_frames,
                           pool_rows, F, chunks, out_global);
    YT_LAUNCH_CHECK("pool_global_rows");
    return 0;
}

extern "C" int ytvln_expand_records_f32(const float* pool_features, const float* pool_geom, const float* pool_probs, const float* pool_global,
                                        const int64_t* offsets, int64_t pool_frames, int64_t pool_rows, const int64_t* index, const double* view,
                                        int64_t slots, int frames, int boxes, int F, int C, float* out_features, float* out_boxes,
                                        float* out_probs, int64_t* out_masks, int64_t* bad, void* stream) {
    YT_REQUIRE(offsets && index && out_features && out_boxes && out_masks, "expand_records: null buffer");
    YT_REQUIRE(pool_frames >= 0 && pool_rows >= 0 && slots >= 0 && boxes > 0 && F >= 0 && C >= 0,
               "expand_records: negative size (pool_frames %lld, pool_rows %lld, slots %lld, boxes %d, F %d, C %d)", (long long)pool_frames,
               (long long)pool_rows, (long long)slots, boxes, F, C);
    YT_REQUIRE(frames > 0 && slots % frames == 0, "expand_records: slots (%lld) must be a multiple of frames (%d > 0)", (long long)slots, frames);
    YT_REQUIRE((pool_probs != nullptr) == (out_probs != nullptr), "expand_records: pool_probs and out_probs go together (both given or both null)");
    YT_REQUIRE(!out_probs || C > 0, "expand_records: probabilities need C > 0 classes (the global region holds 1 / C)");
    YT_REQUIRE(pool_rows == 0 || (pool_features && pool_geom && pool_global), "expand_records: null pool buffer");
    const int64_t widest = std::max<int64_t>(std::max(F, C), 12);
    YT_REQUIRE(slots <= INT64_MAX / boxes && slots * boxes <= INT64_MAX / widest && pool_rows <= INT64_MAX / widest &&
                   pool_frames <= INT64_MAX / widest,
               "expand_records: element counts overflow");
    if (slots == 0) return 0;
    // the pieces of expand_ragged: about 32 KB, at least four boxes
    const int64_t row_bytes = 4 * ((int64_t)F + 12 + (out_probs ? C : 0));
    const int want = (int)std::min<int64_t>(boxes, std::max<int64_t>(4, 32768 / row_bytes));
    const int pieces = (int)cdiv(boxes, want);
    const int group = (int)cdiv(boxes, pieces);
    YT_REQUIRE(slots <= INT64_MAX / pieces, "expand_records: element counts overflow");
    const unsigned grid = (unsigned)std::min<int64_t>(slots * pieces, 1 << 20);
    hipLaunchKernelGGL(expand_records_kernel, dim3(grid), dim3(POOL_THREADS), 0, as_stream(stream), pool_features, pool_geom, pool_probs,
                       pool_global, offsets, pool_frames, pool_rows, index, view, slots, frames, boxes, F, C, group, pieces, out_features,
                       out_boxes, out_probs, out_masks, reinterpret_cast<unsigned long long*>(bad));
    YT_LAUNCH_CHECK("expand_records");
    return 0;
}

// The checks the two masked entry points share behind those of their own pool, then the launch.  `a` arrives complete but for group / pieces.
template <bool RECORDS>
static int launch_masked(const char* who, MaskedExpansion a, int feature_dtype, void* stream) {
    YT_REQUIRE(feature_dtype == YTVLN_DT_F32 || feature_dtype == YTVLN_DT_BF16, "%s: feature_dtype %d (YTVLN_DT_F32 or YTVLN_DT_BF16 only)", who,
               feature_dtype);
    YT_REQUIRE((a.out_targets != nullptr) == (a.out_targets_mask != nullptr),
               "%s: out_targets and out_targets_mask go together (both given or both null)", who);
    YT_REQUIRE(!(a.p || a.rng) || (a.pool_probs && a.out_targets), "%s: masking (p or rng given) needs pool_probs, out_targets and out_targets_mask",
               who);
    YT_REQUIRE(!a.out_targets || a.C > 0, "%s: targets need C > 0 classes (an unselected row holds 1 / C)", who);
    const int64_t widest = std::max<int64_t>(std::max(a.F, a.C), 12);
    YT_REQUIRE(a.slots <= INT64_MAX / a.boxes && a.slots * a.boxes <= INT64_MAX / widest && a.pool_rows <= INT64_MAX / widest &&
                   a.pool_frames <= INT64_MAX / widest,
               "%s: element counts overflow", who);
    if (a.slots == 0) return 0;
    // the pieces of expand_ragged, counted in the bytes this launch writes: about 32 KB, at least four boxes
    const int64_t row_bytes = (feature_dtype == YTVLN_DT_BF16 ? 2 : 4) * (int64_t)a.F + 4 * (12 + (int64_t)(a.out_targets ? a.C : 0));
    const int want = (int)std::min<int64_t>(a.boxes, std::max<int64_t>(4, 32768 / row_bytes));
    a.pieces = (int)cdiv(a.boxes, want);
    a.group = (int)cdiv(a.boxes, a.pieces);
    YT_REQUIRE(a.group <= POOL_MAX_GROUP, "%s: %d rows per piece exceed the %d the kernel decides at once", who, a.group, POOL_MAX_GROUP);
    YT_REQUIRE(a.slots <= INT64_MAX / a.pieces, "%s: element counts overflow", who);
    const unsigned grid = (unsigned)std::min<int64_t>(a.slots * a.pieces, 1 << 20);
    if (feature_dtype == YTVLN_DT_BF16)
        hipLaunchKernelGGL((expand_masked_kernel<RECORDS, uint16_t>), dim3(grid), dim3(POOL_THREADS), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL((expand_masked_kernel<RECORDS, float>), dim3(grid), dim3(POOL_THREADS), 0, as_stream(stream), a);
    YT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int ytvln_expand_ragged_masked(const float* pool_features, const float* pool_loc, const float* pool_probs, const int64_t* offsets,
                                          int64_t pool_frames, int64_t pool_rows, const int64_t* index, int64_t slots, int frames, int boxes,
                                          int F, int L, int C, const float* p, const int64_t* rng, int64_t site, void* out_features,
                                          int feature_dtype, float* out_boxes, float* out_targets, int64_t* out_masks, int64_t* out_targets_mask,
                                          int64_t* bad, void* stream) {
    YT_REQUIRE(offsets && index && out_features && out_boxes && out_masks, "expand_ragged_masked: null buffer");
    YT_REQUIRE(pool_frames >= 0 && pool_rows >= 0 && slots >= 0 && boxes > 0 && F >= 0 && L >= 0 && C >= 0,
               "expand_ragged_masked: negative size (pool_frames %lld, pool_rows %lld, slots %lld, boxes %d, F %d, L %d, C %d)",
               (long long)pool_frames, (long long)pool_rows, (long long)slots, boxes, F, L, C);
    YT_REQUIRE(frames > 0 && slots % frames == 0, "expand_ragged_masked: slots (%lld) must be a multiple of frames (%d > 0)", (long long)slots,
               frames);
    YT_REQUIRE(L <= 11, "expand_ragged_masked: L = %d location columns exceed the 11 the boxes hold next to the position column", L);
    YT_REQUIRE(pool_rows == 0 || (pool_features && pool_loc), "expand_ragged_masked: null pool buffer");
    MaskedExpansion a = {pool_features, pool_loc, nullptr, pool_probs, nullptr, offsets, pool_frames, pool_rows, index, nullptr, slots,
                         frames, boxes, F, L, C, 0, 0, p, rng, site, out_features, out_boxes, out_targets, out_masks, out_targets_mask,
                         reinterpret_cast<unsigned long long*>(bad)};
    return launch_masked<false>("expand_ragged_masked", a, feature_dtype, stream);
}

extern "C" int ytvln_expand_records_masked(const float* pool_features, const float* pool_geom, const float* pool_probs, const float* pool_global,
                                           const int64_t* offsets, int64_t pool_frames, int64_t pool_rows, const int64_t* index, const double* view,
                                           int64_t slots, int frames, int boxes, int F, int C, const float* p, const int64_t* rng, int64_t site,
                                           void* out_features, int feature_dtype, float* out_boxes, float* out_targets, int64_t* out_masks,
                                           int64_t* out_targets_mask, int64_t* bad, void* stream) {
    YT_REQUIRE(offsets && index && out_features && out_boxes && out_masks, "expand_records_masked: null buffer");
    YT_REQUIRE(pool_frames >= 0 && pool_rows >= 0 && slots >= 0 && boxes > 0 && F >= 0 && C >= 0,
               "expand_records_masked: negative size (pool_frames %lld, pool_rows %lld, slots %lld, boxes %d, F %d, C %d)", (long long)pool_frames,
               (long long)pool_rows, (long long)slots, boxes, F, C);
    YT_REQUIRE(frames > 0 && slots % frames == 0, "expand_records_masked: slots (%lld) must be a multiple of frames (%d > 0)", (long long)slots,
               frames);
    YT_REQUIRE(pool_rows == 0 || (pool_features && pool_geom && pool_global), "expand_records_masked: null pool buffer");
    MaskedExpansion a = {pool_features, nullptr, pool_geom, pool_probs, pool_global, offsets, pool_frames, pool_rows, index, view, slots,
                         frames, boxes, F, 0, C, 0, 0, p, rng, site, out_features, out_boxes, out_targets, out_masks, out_targets_mask,
                         reinterpret_cast<unsigned long long*>(bad)};
    return launch_masked<true>("expand_records_masked", a, feature_dtype, stream);
}
