// On-device batch preparation: the BERT / ViLBERT masking of instruction tokens and region features
// that the reference applies per dataset item on the host (utils/dataset/common.py:213-300), as two HBM-bound kernels over
// the whole [bs*K, ...] batch.  The uniform draws come either from the caller (explicit `p` / `random_tokens`: used to pin the
// kernels bit-for-bit against the reference's functions) or from the library's Philox stream (production).
#include "common.h"
#include <algorithm>
#include <string.h>

namespace ytvln {

// float thresholds exactly as torch compares an fp32 tensor with the reference's Python doubles (scalar -> fp32); thr_mask, thr_reg_zero and
// the uniform draw u01 are in common.h (pool.hip masks regions with them too)
__device__ __forceinline__ float thr_tok_random() { return (float)(0.85 + 0.15 * 0.8); }
__device__ __forceinline__ float thr_tok_keep() { return (float)(0.85 + 0.15 * 0.9); }

// randomize_tokens (common.py:213-270 with mask_action_rate == 0; randomize_tokens_action_kernel below is the other case):  p = U * mask;  p >= 0.85 -> target = token, token = [MASK];
// p >= 0.97 -> token = random id;  p >= 0.985 -> token = original.  targets = -1 elsewhere.
__global__ __launch_bounds__(256) void randomize_tokens_kernel(const int64_t* __restrict__ tokens, const int64_t* __restrict__ mask,
                                                               int64_t n, int vocab, int64_t mask_id, const float* __restrict__ p_in,
                                                               const int64_t* __restrict__ rand_in, const int64_t* __restrict__ rng,
                                                               int64_t site, int64_t* __restrict__ out, int64_t* __restrict__ targets) {
    DropKey key = {0, 0, 0, 0};
    if (!p_in || !rand_in) key = make_drop_key(rng, site);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t tok = tokens[i];
        u32x4 b = {0, 0, 0, 0};
        if (!p_in || !rand_in) b = drop_bits(key, (uint64_t)i);
        const float p = (p_in ? p_in[i] : u01(b.x)) * (float)mask[i];
        const int64_t rnd = rand_in ? rand_in[i] : (int64_t)(b.y % (uint32_t)vocab);
        int64_t t = tok, tg = -1;
        if (p >= thr_mask()) { tg = tok; t = mask_id; }
        if (p >= thr_tok_random()) t = rnd;
        if (p >= thr_tok_keep()) t = tok;
        out[i] = t;
        targets[i] = tg;
    }
}

// randomize_tokens with mask_action_rate > 0 (common.py:234-253): per dataset item (`group` = K*T contiguous tokens) the positions of the
// three action ids are enumerated -- all of a0 in row-major order, then all of a1, then all of a2 (torch.where per id, concatenated): n of
// them -- and m = int(rate * n) ordinals are drawn WITH replacement; a drawn position becomes [MASK] and a target whatever its own p and
// mask say (its p is overwritten with 0.85 * 0.9, below every threshold).  The reference applies the draws one after another and reads the
// tokens it has already written, so a position drawn twice ends with target = [MASK] (repeat_target = 1, what the reference's checkpoints
// were trained with); repeat_target = 0 keeps the word.  Every other position follows randomize_tokens_kernel.
//
// One 256-thread workgroup per item, four phases:
//   1. class totals (64-bit ballot + popcount per wave, wave totals through LDS) -> n, m = (int64)(rate * (double)n) in double, like Python;
//   2. the m draws: hits[ordinal] += 1 in LDS (integer atomics: order-independent, so the result is deterministic);
//   3. a block-wide ORDERED scan over 256-token chunks gives every action position its ordinal = class offset + carry of the earlier
//      chunks + totals of the earlier waves + popcount of the lower lanes;
//   4. (same pass as 3) out / targets of every token.
// Philox counter layout (rng mode).  Per-token draws: site `site`, counter = flat token index, .x -> p, .y -> random id: exactly
// randomize_tokens_kernel, so a token the action step does not touch equals the plain kernel's output at the same stream position.  Action
// draws: site `action_site`, counter = item * (4 * group) + (d >> 2) for draw d, word d & 3 of the block.  m <= ACT_MAX_RATE * n <= 16 * group,
// so d >> 2 < 4 * group and no two items share a counter.  An ordinal is (bits * n) >> 32 of a uniform 32-bit word: every ordinal has
// floor(2^32 / n) or ceil(2^32 / n) preimages, i.e. its probability is within 2^-32 of 1/n (relative bias <= n / 2^32 < 2e-6 at n = 8192).
constexpr int ACT_MAX_GROUP = 8192;        // hits[]: 32 KB of LDS
constexpr double ACT_MAX_RATE = 16.0;      // bounds the draw loop and the counter layout above

__global__ __launch_bounds__(256) void randomize_tokens_action_kernel(
    const int64_t* __restrict__ tokens, const int64_t* __restrict__ mask, int64_t items, int group, int vocab, int64_t mask_id, int64_t a0,
    int64_t a1, int64_t a2, double rate, int repeat_target, const float* __restrict__ p_in, const int64_t* __restrict__ rand_in,
    const int64_t* __restrict__ choice, int64_t cap, const int64_t* __restrict__ rng, int64_t site, int64_t action_site,
    int64_t* __restrict__ out, int64_t* __restrict__ targets, int64_t* __restrict__ counts) {
    __shared__ int s_hits[ACT_MAX_GROUP];
    __shared__ int s_tot[4][3];
    __shared__ int s_scan[2][4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;          // lanes in front of this one
    const bool explicit_draws = p_in && rand_in;
    DropKey key = {0, 0, 0, 0}, akey = {0, 0, 0, 0};
    if (!explicit_draws) { key = make_drop_key(rng, site); akey = make_drop_key(rng, action_site); }

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t base = item * (int64_t)group;
        // 1. totals per class
        int c0 = 0, c1 = 0, c2 = 0;
        for (int b = 0; b < group; b += 256) {
            const int i = b + tid;
            const bool valid = i < group;
            const int64_t tok = valid ? tokens[base + i] : 0;
            c0 += __popcll(__ballot(valid && tok == a0));
            c1 += __popcll(__ballot(valid && tok == a1));
            c2 += __popcll(__ballot(valid && tok == a2));
            if (valid) s_hits[i] = 0;
        }
        if (lane == 0) { s_tot[wave][0] = c0; s_tot[wave][1] = c1; s_tot[wave][2] = c2; }
        __syncthreads();
        const int n0 = s_tot[0][0] + s_tot[1][0] + s_tot[2][0] + s_tot[3][0];
        const int n1 = s_tot[0][1] + s_tot[1][1] + s_tot[2][1] + s_tot[3][1];
        const int n2 = s_tot[0][2] + s_tot[1][2] + s_tot[2][2] + s_tot[3][2];
        const int n = n0 + n1 + n2;                                        // <= group
        const int64_t m = (int64_t)(rate * (double)n);                     // int(rate * n) of Python floats: truncation of the double product
        if (counts && tid == 0) { counts[2 * item] = n; counts[2 * item + 1] = m; }
        // 2. the draws
        if (explicit_draws) {
            const int64_t lim = m < cap ? m : cap;
            for (int64_t d = tid; d < lim; d += 256) {
                const int64_t r = choice[item * cap + d];
                if (r >= 0 && r < n) atomicAdd(&s_hits[(int)r], 1);        // out-of-range values are skipped, never indexed with
            }
        } else {
            const uint64_t q0 = (uint64_t)item * (4ull * (uint64_t)group);
            for (int64_t q = tid; 4 * q < m; q += 256) {
                const u32x4 bits = drop_bits(akey, q0 + (uint64_t)q);
                const uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < m) atomicAdd(&s_hits[(int)(((uint64_t)w[j] * (uint64_t)n) >> 32)], 1);     // < n (m > 0 implies n > 0)
            }
        }
        __syncthreads();
        // 3 + 4. ordered scan and the outputs
        int k0 = 0, k1 = n0, k2 = n0 + n1;                                  // class offset + carry of the chunks done
        for (int b = 0, it = 0; b < group; b += 256, it ^= 1) {
            const int i = b + tid;
            const bool valid = i < group;
            const int64_t g = base + (valid ? i : 0);
            const int64_t tok = valid ? tokens[g] : 0;
            const int cls = !valid ? -1 : tok == a0 ? 0 : tok == a1 ? 1 : tok == a2 ? 2 : -1;
            const uint64_t m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2);
            if (lane == 0) { s_scan[it][wave][0] = __popcll(m0); s_scan[it][wave][1] = __popcll(m1); s_scan[it][wave][2] = __popcll(m2); }
            __syncthreads();              // one barrier per chunk: the next chunk writes the other buffer
            int pre[3] = {0, 0, 0}, tot[3] = {0, 0, 0};
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int v = s_scan[it][w][c];
                    tot[c] += v;
                    if (w < wave) pre[c] += v;
                }
            if (valid) {
                u32x4 bits = {0, 0, 0, 0};
                if (!explicit_draws) bits = drop_bits(key, (uint64_t)g);
                const float p = (explicit_draws ? p_in[g] : u01(bits.x)) * (float)mask[g];
                const int64_t rnd = explicit_draws ? rand_in[g] : (int64_t)(bits.y % (uint32_t)vocab);
                int64_t t = tok, tg = -1;
                if (p >= thr_mask()) { tg = tok; t = mask_id; }
                if (p >= thr_tok_random()) t = rnd;
                if (p >= thr_tok_keep()) t = tok;
                if (cls >= 0) {
                    const int ord = cls == 0 ? k0 + pre[0] + __popcll(m0 & below)
                                  : cls == 1 ? k1 + pre[1] + __popcll(m1 & below)
                                             : k2 + pre[2] + __popcll(m2 & below);
                    const int h = ord < group ? s_hits[ord] : 0;           // ord < n <= group always; the guard keeps the LDS read in bounds
                    if (h > 0) { t = mask_id; tg = (h == 1 || !repeat_target) ? tok : mask_id; }
                }
                out[g] = t;
                targets[g] = tg;
            }
            k0 += tot[0]; k1 += tot[1]; k2 += tot[2];
        }
        __syncthreads();                  // s_hits / s_tot are rewritten by the next item
    }
}

// randomize_regions (common.py:272-300): one wave per region row.  p = U * mask;  p >= 0.85 -> targets = probs, targets_mask = 1
// (else targets = 1/C, 0);  p >= 0.865 -> the 2048-d feature row is zeroed in place.
__global__ __launch_bounds__(256) void randomize_regions_kernel(float* __restrict__ feat, int64_t ldf, const float* __restrict__ probs,
                                                                const int64_t* __restrict__ mask, int64_t rows, int F, int C,
                                                                const float* __restrict__ p_in, const int64_t* __restrict__ rng,
                                                                int64_t site, float* __restrict__ targets, int64_t* __restrict__ tmask) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    DropKey key = {0, 0, 0, 0};
    if (!p_in) key = make_drop_key(rng, site);
    const float uni = 1.0f / (float)C;            // torch.ones_like(probs) / C in fp32
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const float p = (p_in ? p_in[r] : u01(drop_bits(key, (uint64_t)r).x)) * (float)mask[r];
        const bool sel = p >= thr_mask();
        float* trow = targets + r * (int64_t)C;
        const float* prow = probs + r * (int64_t)C;
        for (int c = lane; c < C; c += 64) trow[c] = sel ? prow[c] : uni;
        if (lane == 0) tmask[r] = sel ? 1 : 0;
        if (p >= thr_reg_zero()) {
            float* frow = feat + r * ldf;
            if ((F & 3) == 0 && (ldf & 3) == 0 && ((reinterpret_cast<uintptr_t>(feat) & 15) == 0)) {
                for (int c = lane; c < (F >> 2); c += 64) reinterpret_cast<float4*>(frow)[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                for (int c = lane; c < F; c += 64) frow[c] = 0.f;
            }
        }
    }
}

}  // namespace ytvln

using namespace ytvln;

extern "C" int ytvln_randomize_tokens(const int64_t* tokens, const int64_t* mask, int64_t n, int vocab_size, int64_t mask_token_id,
                                      const float* p, const int64_t* random_tokens, const int64_t* rng, int64_t site,
                                      int64_t* tokens_out, int64_t* targets_out, void* stream) {
    YT_REQUIRE(tokens && mask && tokens_out && targets_out && n >= 0 && vocab_size > 0, "randomize_tokens: bad argument");
    YT_REQUIRE((p && random_tokens) || rng, "randomize_tokens: needs explicit draws (p, random_tokens) or the rng state");
    if (n == 0) return 0;
    hipLaunchKernelGGL(randomize_tokens_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, as_stream(stream), tokens, mask,
                       n, vocab_size, mask_token_id, p, random_tokens, rng, site, tokens_out, targets_out);
    YT_LAUNCH_CHECK("randomize_tokens");
    return 0;
}

extern "C" int ytvln_randomize_tokens_action(const int64_t* tokens, const int64_t* mask, int64_t items, int64_t group, int vocab_size,
                                             int64_t mask_token_id, int64_t action0, int64_t action1, int64_t action2, int64_t rate_bits,
                                             int repeat_target, const float* p, const int64_t* random_tokens, const int64_t* action_choice,
                                             int64_t cap, const int64_t* rng, int64_t site, int64_t action_site, int64_t* tokens_out,
                                             int64_t* targets_out, int64_t* counts, void* stream) {
    YT_REQUIRE(tokens && mask && tokens_out && targets_out, "randomize_tokens_action: null buffer");
    YT_REQUIRE(items >= 0 && group >= 1 && vocab_size > 0, "randomize_tokens_action: bad shape (items %lld, group %lld, vocab %d)",
               (long long)items, (long long)group, vocab_size);
    YT_REQUIRE(group <= ACT_MAX_GROUP, "randomize_tokens_action: group %lld exceeds the limit of %d tokens per item", (long long)group, ACT_MAX_GROUP);
    YT_REQUIRE(items <= (INT64_MAX >> 3) / group, "randomize_tokens_action: items * group overflows");       // 4 * items * group: the action counters
    double rate;
    static_assert(sizeof(rate) == sizeof(rate_bits), "rate crosses the ABI as the bits of a double");
    memcpy(&rate, &rate_bits, sizeof(rate));
    YT_REQUIRE(rate >= 0.0 && rate <= ACT_MAX_RATE, "randomize_tokens_action: rate must be finite and within [0, %g]", ACT_MAX_RATE);   // NaN fails both
    YT_REQUIRE(action0 != action1 && action0 != action2 && action1 != action2, "randomize_tokens_action: the action ids must differ");
    YT_REQUIRE(repeat_target == 0 || repeat_target == 1, "randomize_tokens_action: repeat_target is 0 or 1");
    const bool explicit_draws = p && random_tokens;
    YT_REQUIRE(explicit_draws || rng, "randomize_tokens_action: needs explicit draws (p, random_tokens, action_choice) or the rng state");
    YT_REQUIRE(!explicit_draws || (cap >= 0 && (action_choice || cap == 0)), "randomize_tokens_action: action_choice [items, cap] missing");
    YT_REQUIRE(!explicit_draws || cap == 0 || items <= INT64_MAX / cap, "randomize_tokens_action: items * cap overflows");
    if (items == 0) return 0;
    hipLaunchKernelGGL(randomize_tokens_action_kernel, dim3((unsigned)std::min<int64_t>(items, 65536)), dim3(256), 0, as_stream(stream), tokens, mask,
                       items, (int)group, vocab_size, mask_token_id, action0, action1, action2, rate, repeat_target, explicit_draws ? p : nullptr,
                       explicit_draws ? random_tokens : nullptr, action_choice, cap, rng, site, action_site, tokens_out, targets_out, counts);
    YT_LAUNCH_CHECK("randomize_tokens_action");
    return 0;
}

extern "C" int ytvln_randomize_regions(float* features, int64_t ldf, const float* probs, const int64_t* mask, int64_t rows, int F, int C,
                                       const float* p, const int64_t* rng, int64_t site, float* targets, int64_t* targets_mask,
                                       void* stream) {
    YT_REQUIRE(features && probs && mask && targets && targets_mask && rows >= 0 && F > 0 && C > 0 && ldf >= F, "randomize_regions: bad argument");
    YT_REQUIRE(p || rng, "randomize_regions: needs explicit draws (p) or the rng state");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(randomize_regions_kernel, dim3((unsigned)std::min<int64_t>(cdiv(rows, 4), 8192)), dim3(256), 0, as_stream(stream), features,
                       ldf, probs, mask, rows, F, C, p, rng, site, targets, targets_mask);
    YT_LAUNCH_CHECK("randomize_regions");
    return 0;
}
