// Packed rows (BertModel.skip_padding): the row plan of a padding mask and the one row mover that serves pack, unpack and both backwards.
//
//   ytvln_rows_plan      flags[rows] (non-zero = valid), capacity -> pack_idx[capacity], unpack_idx[rows], counts[2].  One launch of ONE
//                        workgroup: thread t owns the contiguous run [t * per, (t + 1) * per) of the flag array, counts it, the 1024 counts
//                        go through a block scan (wave scan by shuffles, the 16 wave totals through LDS), and the thread walks its run a
//                        second time handing out packed rows in ascending order.  No atomics, no host sync: the same flags give the same
//                        plan, and the plan is stable (packed row j is the j-th flagged row).
//   ytvln_rows_move_*    out[j, 0:width] = idx[j] in [0, x_rows) ? x[idx[j], 0:width] : 0.  One wave per output row, so the test on idx[j] is
//                        wave-uniform; 16 bytes per lane where both pointers and both leading dimensions allow it (a width that is no
//                        multiple of 16 bytes finishes with an element tail), elements otherwise.  The mapping of a plan is a partial
//                        bijection, so the mover with pack_idx is the adjoint of the mover with unpack_idx: no scatter-add, no memset.
#include "common.h"

namespace ytvln {

constexpr int PLAN_THREADS = 1024;          // one workgroup: 16 waves

__global__ __launch_bounds__(PLAN_THREADS) void rows_plan_kernel(const uint8_t* __restrict__ flags, int64_t rows, int64_t capacity,
                                                                 int64_t* __restrict__ pack_idx, int64_t* __restrict__ unpack_idx,
                                                                 int64_t* __restrict__ counts) {
    __shared__ int wave_total[PLAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (rows + PLAN_THREADS - 1) / PLAN_THREADS;
    const int64_t lo = min((int64_t)tid * per, rows), hi = min(lo + per, rows);
    int mine = 0;          // (rows < 2^31: checked by the entry point)
    for (int64_t i = lo; i < hi; ++i) mine += flags[i] != 0;
    // inclusive scan inside the wave
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PLAN_THREADS / 64; ++w) {
        const int t = wave_total[w];
        if (w < wave) before += t;
        total += t;
    }
    int64_t next = before + incl - mine;          // packed row of this thread's first flagged row
    for (int64_t i = lo; i < hi; ++i) {
        int64_t u = -1;
        if (flags[i] != 0) {
            if (next < capacity) {
                pack_idx[next] = i;
                u = next;
            }
            ++next;
        }
        unpack_idx[i] = u;
    }
    for (int64_t j = total + tid; j < capacity; j += PLAN_THREADS) pack_idx[j] = -1;
    if (tid == 0) {
        counts[0] = total;
        counts[1] = total > capacity ? total - capacity : 0;
    }
}

struct alignas(16) vec16 { uint32_t a, b, c, d; };

// T: the element (float, or uint16_t for bf16 bits).  WIDE: 16-byte accesses for the first `width - width % (16 / sizeof(T))` columns.
template <class T, bool WIDE>
__global__ __launch_bounds__(256) void rows_move_kernel(const T* __restrict__ x, int64_t ldx, int64_t x_rows, const int64_t* __restrict__ idx,
                                                        int64_t out_rows, int width, T* __restrict__ out, int64_t ldo) {
    constexpr int PER = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per output row
    if (j >= out_rows) return;
    const int64_t src = idx[j];
    const bool live = src >= 0 && src < x_rows;                               // wave-uniform
    T* o = out + j * ldo;
    const T* s = x + (live ? src : 0) * ldx;
    int done = 0;
    if (WIDE) {
        const int nvec = width / PER;
        vec16* ov = reinterpret_cast<vec16*>(o);
        const vec16* sv = reinterpret_cast<const vec16*>(s);
        if (live) {
            for (int c = lane; c < nvec; c += 64) ov[c] = sv[c];
        } else {
            const vec16 z = {0u, 0u, 0u, 0u};
            for (int c = lane; c < nvec; c += 64) ov[c] = z;
        }
        done = nvec * PER;
    }
    if (live) {
        for (int c = done + lane; c < width; c += 64) o[c] = s[c];
    } else {
        for (int c = done + lane; c < width; c += 64) o[c] = (T)0;
    }
}

template <class T>
static int rows_move(const char* who, const T* x, int64_t ldx, int64_t x_rows, const int64_t* idx, int64_t out_rows, int width, T* out,
                     int64_t ldo, void* stream) {
    YT_REQUIRE(out_rows >= 0 && x_rows >= 0 && width >= 1, "%s: negative size (x_rows %lld, out_rows %lld, width %d)", who, (long long)x_rows,
               (long long)out_rows, width);
    YT_REQUIRE(ldx >= width && ldo >= width, "%s: leading dimensions (%lld, %lld) below the width %d", who, (long long)ldx, (long long)ldo, width);
    if (out_rows == 0) return 0;
    YT_REQUIRE(x && idx && out, "%s: null pointer", who);
    YT_REQUIRE(out_rows <= (int64_t)4 * 0x7fffffff, "%s: too many rows", who);
    constexpr int PER = 16 / (int)sizeof(T);
    const bool wide = width >= PER && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % 16 == 0 && ldx % PER == 0 && ldo % PER == 0;
    const dim3 grid((unsigned)cdiv(out_rows, 4)), block(256);
    if (wide)
        hipLaunchKernelGGL((rows_move_kernel<T, true>), grid, block, 0, as_stream(stream), x, ldx, x_rows, idx, out_rows, width, out, ldo);
    else
        hipLaunchKernelGGL((rows_move_kernel<T, false>), grid, block, 0, as_stream(stream), x, ldx, x_rows, idx, out_rows, width, out, ldo);
    YT_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace ytvln

extern "C" int ytvln_rows_plan(const uint8_t* flags, int64_t rows, int64_t capacity, int64_t* pack_idx, int64_t* unpack_idx, int64_t* counts,
                               void* stream) {
    using namespace ytvln;
    YT_REQUIRE(rows >= 1 && capacity >= 1, "rows_plan: negative or empty size (rows %lld, capacity %lld)", (long long)rows, (long long)capacity);
    YT_REQUIRE(rows <= 0x7fffffff, "rows_plan: %lld rows (the scan counts in 32 bits)", (long long)rows);
    YT_REQUIRE(flags && pack_idx && unpack_idx && counts, "rows_plan: null pointer");
    hipLaunchKernelGGL(rows_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, as_stream(stream), flags, rows, capacity, pack_idx, unpack_idx, counts);
    YT_LAUNCH_CHECK("rows_plan");
    return 0;
}

extern "C" int ytvln_rows_move_f32(const float* x, int64_t ldx, int64_t x_rows, const int64_t* idx, int64_t out_rows, int width, float* out,
                                   int64_t ldo, void* stream) {
    return ytvln::rows_move<float>("rows_move_f32", x, ldx, x_rows, idx, out_rows, width, out, ldo, stream);
}

extern "C" int ytvln_rows_move_bf16(const uint16_t* x, int64_t ldx, int64_t x_rows, const int64_t* idx, int64_t out_rows, int width, uint16_t* out,
                                    int64_t ldo, void* stream) {
    return ytvln::rows_move<uint16_t>("rows_move_bf16", x, ldx, x_rows, idx, out_rows, width, out, ldo, stream);
}
