// Live-row list of a padding mask, for the weight-gradient GEMMs that contract over the valid rows only (gemm_dma_kernel<..., LIVE>).
//
//   ytvln_live_rows_list   flags[rows] (non-zero = valid) -> idx[rows + 32] (int32), count[1] (int32).  idx[0 .. count) are the valid rows in
//                          ascending order; every entry behind them holds ONE row that is not valid (the first one), so the count padded to
//                          a multiple of 32 -- what the GEMM walks -- ends in entries whose A row is all zero.  (No such row exists when every
//                          row is valid: the tail then holds rows - 1, and a GEMM whose K is a multiple of 32 never reads it.)
//                          One launch of ONE workgroup, the scan of rows_plan_kernel (rows.hip): thread t owns a contiguous run of the flags,
//                          the 1024 run counts go through a block scan, the thread walks its run a second time.  No atomics, no host read,
//                          nothing sized by device data: the same flags give the same list.
//   ytvln_live_rows_perm   the same kernel writing perm[rows] (int32) in place of idx: the valid rows in ascending order, then the rows that are
//                          not valid in ascending order -- a permutation of 0 .. rows-1 whose first `count` entries are idx's -- and count[1].  The row-listed
//                          GEMMs (gemm_dma_kernel<..., ROWS>) compute the positions in front of the count and zero the rows behind it.
//                          A thread's first dead row goes to position total + (rows before its run) - (valid rows before its run).
#include "common.h"

namespace ytvln {

constexpr int LIST_THREADS = 1024;          // one workgroup: 16 waves

__global__ __launch_bounds__(LIST_THREADS) void live_rows_list_kernel(const uint8_t* __restrict__ flags, int rows, int* __restrict__ idx,
                                                                      int* __restrict__ count, int* __restrict__ perm) {
    __shared__ int wave_total[LIST_THREADS / 64];
    __shared__ int wave_first[LIST_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (rows + LIST_THREADS - 1) / LIST_THREADS;
    const int lo = min(tid * per, rows), hi = min(lo + per, rows);
    int mine = 0, first_dead = rows;          // (first_dead: the lowest row of this run that is not valid)
    for (int i = hi - 1; i >= lo; --i) {
        const bool v = flags[i] != 0;
        mine += v;
        first_dead = v ? first_dead : i;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) first_dead = min(first_dead, __shfl_xor(first_dead, o, 64));
    if (lane == 63) wave_total[wave] = incl;
    if (lane == 0) wave_first[wave] = first_dead;
    __syncthreads();
    int before = 0, total = 0, dead = rows;
#pragma unroll
    for (int w = 0; w < LIST_THREADS / 64; ++w) {
        const int t = wave_total[w];
        if (w < wave) before += t;
        total += t;
        dead = min(dead, wave_first[w]);
    }
    if (dead >= rows) dead = rows - 1;
    int next = before + incl - mine;          // list position of this thread's first valid row
    if (perm) {          // (uniform over the launch)
        int next_dead = total + lo - next;
        for (int i = lo; i < hi; ++i) {
            if (flags[i] != 0) perm[next++] = i;
            else perm[next_dead++] = i;
        }
    } else {
        for (int i = lo; i < hi; ++i)
            if (flags[i] != 0) idx[next++] = i;
    }
    if (idx) {
        for (int j = total + tid; j < rows + 32; j += LIST_THREADS) idx[j] = dead;
    }
    if (tid == 0) count[0] = total;
}

}  // namespace ytvln

extern "C" int ytvln_live_rows_list(const uint8_t* flags, int rows, int* idx, int* count, void* stream) {
    using namespace ytvln;
    YT_REQUIRE(rows >= 1 && rows <= 0x7fffffff - 32, "live_rows_list: bad row count %d", rows);
    YT_REQUIRE(flags && idx && count, "live_rows_list: null pointer");
    hipLaunchKernelGGL(live_rows_list_kernel, dim3(1), dim3(LIST_THREADS), 0, as_stream(stream), flags, rows, idx, count, (int*)nullptr);
    YT_LAUNCH_CHECK("live_rows_list");
    return 0;
}

extern "C" int ytvln_live_rows_perm(const uint8_t* flags, int rows, int* perm, int* count, void* stream) {
    using namespace ytvln;
    YT_REQUIRE(rows >= 1 && rows <= 0x7fffffff - 32, "live_rows_perm: bad row count %d", rows);
    YT_REQUIRE(flags && count && perm, "live_rows_perm: null pointer");
    hipLaunchKernelGGL(live_rows_list_kernel, dim3(1), dim3(LIST_THREADS), 0, as_stream(stream), flags, rows, (int*)nullptr, count, perm);
    YT_LAUNCH_CHECK("live_rows_perm");
    return 0;
}
