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
