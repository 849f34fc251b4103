/*
 * ytvln.h -- C ABI of libytvln.so: the MI355X (gfx950 / CDNA4) kernels behind the ViLBERT hot path of
 * JeremyLinky/YouTube-VLN (forward/backward of vilbert/vilbert.py, the losses of utils/utils_init.py:108-164 and
 * the AdamW step of vilbert/optimization.py:141-187).
 *
 * The reference has no FFI layer of its own: its "plugin API" for this path is the Python class surface of
 * vilbert.vilbert / lily.  Each entry point below therefore cites the reference code whose
 * arithmetic it replaces; the Python modules in youtube-vln_amd/ytvln keep the reference class / argument names and
 * call these through ctypes (see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (PyTorch allocator);
 *     the library never allocates, frees or synchronises;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - row-major fp32 unless stated; `ld*` are leading dimensions in ELEMENTS;
 *   - return value 0 = launched, negative = rejected (bad argument / launch failure); ytvln_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI;
 *   - dropout: Philox4x32-10 keyed by (rng[0] = seed, rng[1] = forward counter) read from DEVICE memory (graph-replay
 *     safe) and by a host-side `site` id; the backward pass regenerates the identical mask from the same triple.
 */
#ifndef YTVLN_H
#define YTVLN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): ytvln_attn_problem carries `keep` (added in round 5 without a bump: a version-1 binding paired with that library passed the
 * check with a struct 8 bytes short), ytvln_attn_problem_size, ytvln_set_host_wait, ytvln_rccl_allreduce_slices (any dtype). */
#define YTVLN_ABI_VERSION 2

int ytvln_version(void);
const char* ytvln_last_error(void);

/* How the HOST waits for the device (hipSetDeviceFlags on `device`; one process per GPU as in utils/distributed.py:63-104, where N ranks share one
 * host): blocking = 1 -> hipDeviceScheduleBlockingSync, a thread that waits in hipStreamSynchronize / hipDeviceSynchronize / hipEventSynchronize
 * sleeps on an interrupt instead of spinning on a core; 0 -> the runtime's default (spin).  Host-side only; no kernel is affected.  Call it
 * before the first stream / event of the process is created (ytvln.misc.set_host_wait does). */
int ytvln_set_host_wait(int device, int blocking);

/* Run-time options: the complete set of switches the library reads (kernel-form selection for tests and experiments; nothing a
 * production run has to touch).  An option starts from the environment variable YTVLN_<NAME> (read at first use) and can be set at any
 * time; INTEGRATION.md section 4 lists every name, default and meaning.  Names may be given with or without the "YTVLN_" prefix.
 *   ytvln_option_count / ytvln_option_name enumerate the table (index 0 .. count-1); set / get return 0, or -1 for an unknown name. */
int ytvln_option_count(void);
const char* ytvln_option_name(int index);
int ytvln_set_option(const char* name, int value);
int ytvln_get_option(const char* name, int* value);

/* activation / epilogue selectors for ytvln_gemm_f32 */
enum {
    YTVLN_EPI_NONE = 0,       /* C = A.B (+bias)                                                             */
    YTVLN_EPI_GELU = 1,       /* aux = A.B + bias (pre-activation, optional) ; C = gelu_erf(aux)  vilbert.py:119 */
    YTVLN_EPI_RELU = 2,       /* C = max(A.B + bias, 0)                                            vilbert.py:832 */
    YTVLN_EPI_MUL_DGELU = 3,  /* C = (A.B) * gelu'(aux)      backward of EPI_GELU through the next Linear        */
    YTVLN_EPI_MUL_DRELU = 4   /* C = (A.B) * (aux > 0)       backward of EPI_RELU (aux = the forward output)     */
};
/* activation selector of the stand-alone activation kernels (ytvln_act_fwd_*, ytvln_act_bwd_*) ONLY, not a GEMM epilogue: ytvln_gemm_f32 /
 * ytvln_gemm_bf16 reject it.  swish(z) = z * sigmoid(z) (vilbert.py:122-123) is unfused by design: y = swish(x W^T + b) is the GEMM with
 * YTVLN_EPI_NONE writing the pre-activation z (kept for the backward, as EPI_GELU keeps aux), then ytvln_act_fwd_*.  Against a fused epilogue
 * that is one extra read and one extra write of [rows, N] per activated projection (8 bytes per element in fp32, 4 in bf16). */
enum {
    YTVLN_ACT_SWISH = 5
};

/* Dense projection on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).  Replaces every nn.Linear / F.linear on the path
 * (vilbert.py:285-287, 322, 352, 365, 555-568, 641-644, 831, 864, 906, 968, 1358 ...) and their autograd backward.
 *   C[M,N] (+)= op(A)[M,K] . op(B)[K,N]
 *   transA = 0: A stored [M,K] (lda >= K)      transA = 1: A stored [K,M] (lda >= M)
 *   transB = 0: B stored [K,N] (ldb >= N)      transB = 1: B stored [N,K] (ldb >= K)   <- nn.Linear weight layout
 *   bias: [N] or NULL.  beta: 0 = overwrite, 1 = accumulate into C.  aux/ldaux: see the epilogue enum (may be NULL).
 *   workspace: optional scratch of ytvln_gemm_workspace_elems(M,N,K,epilogue) floats.  When it is supplied and the output
 *   has too few 128x128 tiles to fill 256 CUs (weight gradients: [out,in] outputs contracted over N*T or N*R rows), the
 *   contraction is split across workgroups and reduced in a fixed order (deterministic split-K); otherwise ignored.
 *   flags: YTVLN_GEMM_A_ZERO_PADDED = the caller guarantees readable ZERO padding behind A's contiguous dimension up to
 *   lda (rounded to 32 for a K-contiguous A with B = [K,N]; to 4 for an M-contiguous A).  It lets the 30522- and 1601-wide
 *   logit gradients (vilbert.py:906, 968 backward) use the LDS-DMA main loop although 30522 % 32 != 0. */
#define YTVLN_GEMM_A_ZERO_PADDED 1
/* opt-in: every fp32 operand value is split exactly into three bf16 terms in registers and each product is accumulated in fp32
 * from the six largest cross terms on the bf16 matrix instruction (error per product ~ one fp32 rounding; LDS-DMA path only,
 * ignored by the generic kernel).  Finite inputs only: an infinite operand value yields NaN (inf - inf in the
 * split) where the native instruction would propagate the infinity. */
#define YTVLN_GEMM_SPLIT_BF16X3 2
int64_t ytvln_gemm_workspace_elems(int M, int N, int K, int epilogue);
/* Introspection (host only, no GPU work): the tile shape and split count the launch planner picks for an aligned problem of this size
 * (transA = 1: M-contiguous A, which excludes the 256-row tiles).  Used by tests and by tools/ to explain a measurement. */
int ytvln_gemm_plan(int M, int N, int K, int transA, int epilogue, int* tile_m, int* tile_n, int* splits);
/* the same for a launch carrying YTVLN_GEMM_SPLIT_BF16X3 (its planner has its own per-tile costs; 256x256 tiles also for transA = 1 and
 * with split-K) */
int ytvln_gemm_plan_x3(int M, int N, int K, int transA, int epilogue, int* tile_m, int* tile_n, int* splits);
int ytvln_gemm_f32(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                   int64_t ldc, const float* bias, float* aux, int64_t ldaux, int M, int N, int K, int epilogue,
                   float beta, float* workspace, int64_t workspace_elems, int flags, void* stream);

/* ytvln_gemm_f32 that ALSO produces a_rowsum[m] = sum_k op(A)[m, k] when it can do so for free: the bias gradient of an nn.Linear
 * (db = sum over rows of dY, vilbert.py:285-287 ... backward) rides on its weight-gradient GEMM dW = dY^T X, whose A operand is dY^T --
 * the workgroups of the first tile column add up the fragments they feed to the matrix cores (fixed order; split-K partials are
 * reduced in split order: deterministic).  *rowsum_done (HOST int) is set to 1 when the sums were produced -- LDS-DMA main loop,
 * M-contiguous fp32 A (transA = 1), K % 32 == 0, no fp32x3 -- and to 0 otherwise (the caller then runs ytvln_colsum_f32).
 * `workspace` as returned by ytvln_gemm_workspace_elems also holds the per-split partial sums. */
int ytvln_gemm_f32_rowsum(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                          int64_t ldc, const float* bias, float* aux, int64_t ldaux, int M, int N, int K, int epilogue,
                          float beta, float* workspace, int64_t workspace_elems, int flags, float* a_rowsum, int* rowsum_done,
                          void* stream);

/* The same projection with the PERSISTENT kernel available (csrc/gemm_sk.hip; the nn.Linear forward and input-gradient GEMMs of
 * vilbert.py:285-287, 322, 352, 365, 555-568, 641-644 with a K-contiguous A): one workgroup per CU walks whole output tiles or --
 * stream-K form -- an equal share of the (tile, k-tile) iteration space, the next piece's operands in flight under the epilogue; partial
 * tiles are added in ascending k order by the workgroup that holds the k = 0 end of the tile (bit-reproducible).
 *   sk_ctl: ytvln_gemm_sk_ctl_elems() uint32 words, ZERO when first used and private to the stream the call is enqueued on (the kernel
 *   leaves it zero); NULL = exactly ytvln_gemm_f32 / ytvln_gemm_f32_rowsum.  workspace (ytvln_gemm_workspace_elems) also holds the
 *   partial tiles.  a_rowsum / rowsum_done: both NULL or both set (as ytvln_gemm_f32_rowsum).  The launch planner decides per shape between
 *   this kernel and the launch-per-tile one (run-time options GEMM_SK, GEMM_SK_TILE, GEMM_SK_GROUPS). */
int64_t ytvln_gemm_sk_ctl_elems(void);
int ytvln_gemm_f32_sk(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                      int64_t ldc, const float* bias, float* aux, int64_t ldaux, int M, int N, int K, int epilogue,
                      float beta, float* workspace, int64_t workspace_elems, int flags, float* a_rowsum, int* rowsum_done,
                      uint32_t* sk_ctl, void* stream);
/* Introspection (host only): does the planner take the persistent kernel for this aligned problem, with which tile, in the whole-tile
 * (*whole_tiles = 1) or the stream-K form, on how many workgroups. */
int ytvln_gemm_sk_plan(int M, int N, int K, int transA, int epilogue, int* use, int* tile_m, int* tile_n, int* whole_tiles,
                       int* workgroups);
/* Weight gradients over the valid rows only.  dW = dY^T X is contracted over the rows of the batch; where a padded row of dY is exactly
 * zero (every Linear of the model: DESIGN.md section 4) its products are 0 * x and need not be formed.
 *   ytvln_live_rows_list: flags[rows] (one byte per row, non-zero = valid) -> idx[rows + 32] (int32) and count[1] (int32), DEVICE memory.
 *   idx[0 .. count) = the valid rows, ascending; every later entry holds one row that is not valid (rows - 1 when all are valid).  One
 *   launch, no atomics, no host read.
 *   ytvln_gemm_f32_live = ytvln_gemm_f32_rowsum (a_rowsum / rowsum_done: both NULL or both set) whose contraction runs over
 *   live_idx[0 .. 32 * ceil(*live_count / 32)): k-tile t is list entries 32t .. 32t+31, the same rows for both operands; split s of the
 *   plan chosen for the full K takes ceil(tiles / splits) live tiles (with fewer than 32 live rows per split: ceil(count / splits) rows each,
 *   as one padded tile, so that a sparse list is summed in short chains over all splits like the unlisted launch sums it), so count = K
 *   reproduces the unlisted launch bit for bit, and nothing on
 *   the host depends on the count (capturable; a replay follows the list in memory).  CONTRACT: rows of op(A)^T = A[k, :] that are not
 *   listed are all zero and B is finite there.  The list is used when transA = 1, transB = 0, K % 32 == 0, the launch takes the native
 *   LDS-DMA loop on 256x256 or 128x128 tiles with a K-chunk of at most 4096 rows per split, and the run-time option GEMM_LIVE_ROWS is
 *   non-zero; any other launch ignores it (same sum, by the contract). */
int ytvln_live_rows_list(const uint8_t* flags, int rows, int* idx, int* count, void* stream);
int ytvln_gemm_f32_live(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                        int64_t ldc, const float* bias, float* aux, int64_t ldaux, int M, int N, int K, int epilogue,
                        float beta, float* workspace, int64_t workspace_elems, int flags, float* a_rowsum, int* rowsum_done,
                        const int* live_idx, const int* live_count, void* stream);
/* Forward and input-gradient projections on the valid rows only (transA = 0: Y = X W^T, dX = dY W).
 *   ytvln_live_rows_perm: flags[rows] as for ytvln_live_rows_list -> perm[rows] (int32) and count[1] (int32), DEVICE memory: the valid rows
 *   ascending, then the rows that are not valid ascending -- a permutation of 0 .. rows-1 whose first `count` entries are that call's idx.
 *   One launch, no atomics, no host read.
 *   ytvln_gemm_f32_rows = ytvln_gemm_f32 whose M dimension runs over the list: position p stands for row row_perm[p] of A, of C and of aux.
 *   Positions 0 .. *row_count-1 are computed exactly as the unlisted launch on the same plan computes those rows (an identity list gives its
 *   bits).  The rows listed behind the count are DEAD: A is not read there, and the launch leaves them defined -- exact zeros in C, and in
 *   aux where YTVLN_EPI_GELU writes its pre-activation, with beta = 0; untouched with beta != 0.  row_perm must be a permutation of
 *   0 .. M-1 (entries are clamped into the matrix).  Both pointers are DEVICE memory and the grid covers the full M, so nothing on the host
 *   depends on the count (capturable).  m_hint (HOST, 0 = M): the number of rows the caller expects to be listed; it replaces M in the
 *   planner's choice of the tile and nowhere else -- a wrong hint costs time, never rows or bits.  Listed launches take 128x128 tiles (with
 *   split-K by list position and a list-aware reduce) or 256x256 tiles; the split count is always the unlisted launch's, so the bits of a
 *   listed row depend neither on the list nor on the hint.  The list is used when transA = 0, fp32 without
 *   YTVLN_GEMM_SPLIT_BF16X3, K % 32 == 0, the operands meet the LDS-DMA path's alignment, and the run-time option GEMM_LIVE_M is
 *   non-zero; any other launch ignores it and computes every row, dead ones included (A must then be readable there).
 *   ytvln_gemm_rows_workspace_elems: workspace for ytvln_gemm_f32_rows at this hint (>= ytvln_gemm_workspace_elems).
 *   ytvln_gemm_rows_plan (host only): the tile and split count a listed launch of this aligned problem takes. */
int ytvln_live_rows_perm(const uint8_t* flags, int rows, int* perm, int* count, void* stream);
int ytvln_gemm_f32_rows(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
                        int64_t ldc, const float* bias, float* aux, int64_t ldaux, int M, int N, int K, int epilogue,
                        float beta, float* workspace, int64_t workspace_elems, int flags, const int* row_perm,
                        const int* row_count, int m_hint, void* stream);
int64_t ytvln_gemm_rows_workspace_elems(int M, int N, int K, int epilogue, int m_hint);
int ytvln_gemm_rows_plan(int M, int N, int K, int epilogue, int m_hint, int* tile_m, int* tile_n, int* splits);
/* Diagnostics: when `buffer` is non-NULL every workgroup of a persistent launch writes 16 s_memrealtime stamps (100 MHz) to
 * buffer[16 * workgroup + i]: 0 start, 1 ticket drawn, 2 first operands in LDS, then (main loop done, epilogue issued) per piece, 15 end.
 * The buffer must hold 16 * 1024 uint64 (a launch has at most 2 workgroups per CU); NULL switches the stamps off (default). */
int ytvln_gemm_probe(unsigned long long* buffer);

/* out[b, n] = sum over the b-th block of `rows_per_block` rows of x[:, n].  out is [ceil(M/rows_per_block), N] with
 * leading dimension ldo (bias gradients, position-embedding gradient, second stage of every column reduction). */
int ytvln_colsum_f32(const float* x, int64_t ldx, int M, int N, float* out, int64_t ldo, int rows_per_block,
                     void* stream);

/* out[b, k, n] = sum over rows r of block b with idx[r] == k of x[r, n], for small tables (KT <= 32): gradient of
 * image_sequence_embeddings (vilbert.py:1364) and token_type_embeddings (:251).  idx_f32 (float indices, as stored in
 * image_loc[..., 11]) or idx_i64 is used, whichever is non-NULL. */
int ytvln_colsum_by_index_f32(const float* x, int64_t ldx, const float* idx_f32, int64_t idx_stride,
                              const int64_t* idx_i64, int M, int N, int KT, float* out, int rows_per_block,
                              void* stream);

/* table_grad[idx[r], :] += x[r, :] (atomic), rows with idx == skip_idx ignored: backward of nn.Embedding with
 * padding_idx (vilbert.py:225-227, 249). */
int ytvln_scatter_add_rows_f32(const float* x, int64_t ldx, const int64_t* idx, int M, int H, float* table_grad,
                               int64_t skip_idx, void* stream);
/* Deterministic form for repeated indices (word-embedding gradient, BertEmbeddings backward, vilbert.py:219-256): `sorted_idx` = the
 * indices in ascending order (stable sort), `perm` = the source row of each sorted position.  One wave owns each run of equal indices:
 * no atomics, fixed summation order -> bit-reproducible training steps. */
int ytvln_scatter_add_rows_sorted_f32(const float* x, int64_t ldx, const int64_t* sorted_idx, const int64_t* perm, int M, int H,
                                      float* table_grad, int64_t skip_idx, void* stream);

/* The bf16-resident path (BASELINE configs[4], ytvln.ops.set_matmul_precision("bf16")): activations, gradients and a bf16 copy of the
 * weights live in HBM as bf16 and every projection reads its operands IN PLACE -- no per-call staging, cast or transpose:
 *   C[M,N] (+)= op(A)[M,K] . op(B)[K,N]   with the transA / transB conventions of ytvln_gemm_f32 (bf16 elements, leading dimensions in elements);
 *   an operand whose contraction index is its row (transA = 1, transB = 0) is gathered from LDS by ds_read_b64_tr_b16.
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16; bias is fp32; the epilogue runs in fp32 and rounds once (RNE) into C, which is bf16
 * (c_dtype = YTVLN_DT_BF16) or fp32 (YTVLN_DT_F32: logits, pooled heads, weight gradients); aux (GELU pre-activation out, GELU' / ReLU' in) is
 * bf16.  workspace: ytvln_gemm_bf16_workspace_elems(M,N,K,epilogue) floats (deterministic split-K of the weight gradients); flags:
 * YTVLN_GEMM_A_ZERO_PADDED as for ytvln_gemm_f32, padding in units of 8 elements.  a_rowsum / rowsum_done (may both be NULL): as
 * ytvln_gemm_f32_rowsum -- row sums of a k-major A (the bias gradient riding on the weight-gradient GEMM), fp32.
 * Operands that are not 16-byte aligned with leading dimensions % 8 == 0 (tiny configurations) run a slow generic kernel: same results. */
int64_t ytvln_gemm_bf16_workspace_elems(int M, int N, int K, int epilogue);
int ytvln_gemm_bf16(const uint16_t* A, int64_t lda, int transA, const uint16_t* B, int64_t ldb, int transB, void* C, int64_t ldc,
                    int c_dtype, const float* bias, uint16_t* aux, int64_t ldaux, int M, int N, int K, int epilogue, float beta,
                    float* workspace, int64_t workspace_elems, int flags, float* a_rowsum, int* rowsum_done, void* stream);
/* Diagnostics: when `buffer` (128 uint32, device) is non-NULL, bf16-output forward-layout launches on the 256x256 tile run an instrumented build of
 * the kernel in which waves 0 and 4 of workgroup `block` record s_memtime (shader cycles, low 32 bits) for k-tiles 8..15 at the eight phase
 * boundaries of each k-tile selected by `mask` (bit 2i: own work of phase i done, bit 2i+1: the barrier behind it released; phases L01 M01
 * L23 M23): buffer[64 * group + 8 * (kt - 8) + point].  NULL switches it off (default).  tools/gemm_bf16_probe.py prints the timeline. */
int ytvln_gemm_bf16_probe(uint32_t* buffer, int block, int mask);
/* out[r][c] = bf16(x[r][c]), round to nearest even: network inputs that arrive as fp32 (the 2048-d region features, once per step) and
 * parameters that are not inside the optimizer's arenas yet (the steps before the first optimizer step). */
int ytvln_cast_f32_bf16(const float* x, int64_t ldx, int64_t rows, int cols, uint16_t* out, int64_t ldo, void* stream);

/* On-device batch preparation: the masking the reference applies per item on the host.
 *   ytvln_randomize_tokens  = randomize_tokens (utils/dataset/common.py:213-270, mask_action_rate = 0):  p = U[0,1) * mask;
 *     p >= 0.85: target = token, token = [MASK];  p >= 0.97: token = random id;  p >= 0.985: token = original;  targets -1 elsewhere.
 *   ytvln_randomize_regions = randomize_regions (common.py:272-300):  p >= 0.85: targets = probs, targets_mask = 1 (else 1/C, 0);
 *     p >= 0.865: the feature row is zeroed IN PLACE.
 *   Draws: explicit (`p`, `random_tokens`; pins the kernels bit-for-bit to the reference functions) or, when those are NULL, the
 *   Philox stream keyed by the device-resident (seed, counter) pair `rng` and `site` (the same state as the dropout kernels).
 *   ytvln_randomize_tokens_action = randomize_tokens with mask_action_rate > 0 (common.py:234-253).  tokens / mask / outputs are
 *     [items, group]: `group` = K*T contiguous tokens of ONE dataset item, 1 <= group <= 8192.  Per item the positions of action0 (row-major),
 *     then of action1, then of action2 are numbered 0..n-1, m = (int64)(rate * (double)n) ordinals are drawn WITH replacement and every drawn
 *     position becomes [MASK] and a target, whatever its p and mask; all other positions follow ytvln_randomize_tokens.  A position drawn more
 *     than once gets target = mask_token_id when repeat_target = 1 (what the reference computes: it reads back the [MASK] it has just
 *     written) or the word when repeat_target = 0.  rate_bits = the IEEE-754 bits of the rate as a double (Python: struct '<q' of '<d'),
 *     0 <= rate <= 16; rate 0 computes exactly ytvln_randomize_tokens.  counts (may be NULL): int64 [items, 2] = (n, m).
 *     Draws: explicit (`p`, `random_tokens` and `action_choice` int64 [items, cap]: the first min(m, cap) entries of a row are read, values
 *     outside [0, n) are skipped; action_choice may be NULL when cap = 0) or, when p / random_tokens are NULL, Philox: the per-token draws of
 *     `site` exactly as ytvln_randomize_tokens lays them out, the ordinals from `action_site` (counter layout: csrc/batch.hip).
 *     One workgroup per item, no global atomics, no host read, deterministic. */
int ytvln_randomize_tokens(const int64_t* tokens, const int64_t* mask, int64_t n, int vocab_size, int64_t mask_token_id,
                           const float* p, const int64_t* random_tokens, const int64_t* rng, int64_t site,
                           int64_t* tokens_out, int64_t* targets_out, void* stream);
int ytvln_randomize_tokens_action(const int64_t* tokens, const int64_t* mask, int64_t items, int64_t group, int vocab_size,
                                  int64_t mask_token_id, int64_t action0, int64_t action1, int64_t action2, int64_t rate_bits,
                                  int repeat_target, const float* p, const int64_t* random_tokens, const int64_t* action_choice,
                                  int64_t cap, const int64_t* rng, int64_t site, int64_t action_site, int64_t* tokens_out,
                                  int64_t* targets_out, int64_t* counts, void* stream);
int ytvln_randomize_regions(float* features, int64_t ldf, const float* probs, const int64_t* mask, int64_t rows, int F, int C,
                            const float* p, const int64_t* rng, int64_t site, float* targets, int64_t* targets_mask, void* stream);

/* Ragged frame pool -> the padded tensors of a step, option expansion included, in one launch (csrc/pool.hip).  The pool holds the real
 * rows of every distinct frame once, frame p in rows offsets[p] .. offsets[p+1]-1 (what the feature readers return, un-padded);
 * `index` names the pool frame shown by each slot = (item, option, position), -1 = padding frame; position f = slot % frames.
 * For slot s, box j in [0, boxes), p = index[s]:
 *   n = min(offsets[p+1] - offsets[p], boxes) when 0 <= p < pool_frames and 0 <= offsets[p] <= offsets[p+1] <= pool_rows, else n = 0;
 *   a p >= pool_frames, a p < -1 or such a pair of offsets out of order / out of range is a BAD slot: bad[0] += 1 when `bad` is given.
 *   The range check on p comes before any read of offsets, the check of the offsets before any read of a row: nothing outside rows
 *   [0, pool_rows) of the pool is read whatever index and offsets hold.
 *   j <  n: the feature and probs rows are copies of pool row offsets[p] + j, out_boxes[:, :L] of pool_loc, columns L..10 = 0, mask 1;
 *   j >= n: exact zeros, mask 0 (the outputs may hold anything on entry: every element is written);
 *   out_boxes[:, 11] = f for EVERY row of every slot, padding frames included (all_dataset.py:314 and :331).
 * No allocation, no host synchronisation, no atomics but the `bad` counter; capturable.  Null required pointers, negative sizes,
 * frames <= 0, slots % frames != 0, L > 11 or only one of pool_probs / out_probs given return a negative code and launch nothing. */
int ytvln_expand_ragged_f32(const float* pool_features,   /* [pool_rows, F]                                   */
                            const float* pool_loc,        /* [pool_rows, L], L <= 11                          */
                            const float* pool_probs,      /* [pool_rows, C] or NULL (then out_probs NULL too) */
                            const int64_t* offsets,       /* [pool_frames + 1], first row of each frame       */
                            int64_t pool_frames, int64_t pool_rows,
                            const int64_t* index,         /* [slots] pool frame per (item, option, position), -1 = padding */
                            int64_t slots, int frames, int boxes, int F, int L, int C,
                            float* out_features,          /* [slots * boxes, F]  */
                            float* out_boxes,             /* [slots * boxes, 12] */
                            float* out_probs,             /* [slots * boxes, C] or NULL */
                            int64_t* out_masks,           /* [slots * boxes]     */
                            int64_t* bad,                 /* NULL or [1], accumulates */
                            void* stream);

/* Raw-record frame pool (csrc/pool.hip): the pool holds decoded records as they come off the disk, frame p in rows
 * offsets[p] .. offsets[p+1]-1 of pool_features [rows, F], pool_probs [rows, C] and
 *   pool_geom [rows, 8] = x1, y1, x2, y2 (pixels), image width, image height of the row's record, featureHeading, featureElevation
 * (0 where the store has none), and what the reference's readers compute on the host happens on the device.
 *
 * ytvln_pool_global_rows_f32: out_global[p, c] = (((0 + x[a, c]) + x[a+1, c]) + ... + x[b-1, c]) / (float)(b - a), a = offsets[p],
 *   b = offsets[p+1], in fp32 and in ROW ORDER: numpy's order for mean(axis=0) of this layout, and part of the contract.  Zero for an
 *   empty frame and for offsets out of order or out of range; nothing outside rows [0, pool_rows) is read.
 *
 * ytvln_expand_records_f32: the outputs, the work split and the "every output element written exactly once" rule of
 *   ytvln_expand_ragged_f32.  A slot showing frame p with n_src rows has n = min(n_src + 1, boxes) real rows:
 *   row 0 = the global region: features pool_global[p], probs (float)(1.0 / C), boxes [0,0,1,1,1, 0,1,0,1,0,1], or with `view`
 *     [0,0,1,1,1, sin(-h), cos(-h), 0, 1, sin(-nh), cos(-nh)] (h, nh = view[s, 0], view[s, 1]; double, rounded once to fp32);
 *   rows 1 .. n-1 = source rows 0 .. n-2: features and probs copied, box columns 0-3 = x1/w, y1/h, x2/w, y2/h, column 4 =
 *     ((x2-x1)*(y2-y1)) / (w*h), all fp32 with correctly rounded division; columns 5-10 = 1, or with `view`
 *     sin(d1), cos(d1), sin(fe), cos(fe), sin(d2), cos(d2) with d1 = fh - (float)h, d2 = fh - (float)nh in fp32, the functions in double
 *     on the fp32 argument, rounded once;
 *   rows n .. boxes-1 and padding slots (index -1): exact zeros, mask 0; column 11 = slot % frames for every row of every slot.
 *   BAD slot (all padding, bad[0] += 1): index out of range, offsets out of order or out of range, or an EMPTY frame.  The range check
 *   on the frame precedes the read of its offsets, the offsets check any read of a row or of pool_global.
 * Both: no allocation, no host synchronisation, capturable; invalid arguments (as for ytvln_expand_ragged_f32) return a negative code
 * and launch nothing. */
int ytvln_pool_global_rows_f32(const float* pool_features,   /* [pool_rows, F]                             */
                               const int64_t* offsets,       /* [pool_frames + 1], first row of each frame */
                               int64_t pool_frames, int64_t pool_rows, int F,
                               float* out_global,            /* [pool_frames, F]                           */
                               void* stream);
int ytvln_expand_records_f32(const float* pool_features,   /* [pool_rows, F]                                   */
                             const float* pool_geom,       /* [pool_rows, 8]                                   */
                             const float* pool_probs,      /* [pool_rows, C] or NULL (then out_probs NULL too) */
                             const float* pool_global,     /* [pool_frames, F] from ytvln_pool_global_rows_f32 */
                             const int64_t* offsets,       /* [pool_frames + 1]                                */
                             int64_t pool_frames, int64_t pool_rows,
                             const int64_t* index,         /* [slots], -1 = padding                            */
                             const double* view,           /* [slots, 2] heading, next heading, or NULL        */
                             int64_t slots, int frames, int boxes, int F, int C,
                             float* out_features,          /* [slots * boxes, F]  */
                             float* out_boxes,             /* [slots * boxes, 12] */
                             float* out_probs,             /* [slots * boxes, C] or NULL */
                             int64_t* out_masks,           /* [slots * boxes]     */
                             int64_t* bad,                 /* NULL or [1], accumulates */
                             void* stream);

/* The two expansions with the region masking of ytvln_randomize_regions and the bf16 rounding of ytvln_cast_f32_bf16 in the SAME launch
 * (csrc/pool.hip): the MVM targets are written once, the features once in the type the model reads, and the padded probabilities are never
 * materialised.  For padded row r = slot * boxes + j, let (feature row, probs row, box columns, m) be what ytvln_expand_ragged_f32 /
 * ytvln_expand_records_f32 write for that row from the same pool, index and view -- same bad-slot rules (an EMPTY record frame is bad), same
 * order of the range checks, same `bad` counter, same column 11.  Then
 *   draw = p[r] when `p` is given, else u01(x word of the Philox block r of (rng, site)) when `rng` is given: the draw
 *          ytvln_randomize_regions takes for flat row r of the same (rng, site);            q = draw * (float)m
 *   sel  = q >= (float)0.85:   out_targets[r, :] = sel ? probs row : 1.0f / (float)C,   out_targets_mask[r] = sel
 *          (the global region of a record slot holds (float)(1.0 / C) when selected)
 *   zero = q >= (float)(0.85 + 0.15 * 0.1):   out_features[r, :] = zero ? exact zeros : feature row
 *   out_boxes and out_masks are the unmasked ones.
 * `p` and `rng` both NULL: masking is off -- features unmasked; out_targets / out_targets_mask, when given, hold 1.0f / (float)C and 0 (what
 *   mask_batch(masked_vision=False) makes of the unfused expansion), and pool_probs, out_targets and out_targets_mask may all be NULL
 *   (inference re-ranking: bf16 features, no probabilities).  Pool probabilities are read for the rows with sel only.
 * feature_dtype = YTVLN_DT_F32: out_features is float [slots * boxes, F].  YTVLN_DT_BF16: uint16_t [slots * boxes, F] (2-byte aligned, F may
 *   be odd), every value rounded once to nearest even with the conversion of ytvln_cast_f32_bf16; zeros stay zeros.  Everything else stays
 *   fp32 / int64.
 * Every output element is written exactly once whatever the outputs held on entry.  No allocation, no host synchronisation, no atomics but
 * the `bad` counter; capturable.  The bad arguments of the unfused entry points, an unknown feature_dtype, masking without pool_probs,
 * out_targets or out_targets_mask, only one of out_targets / out_targets_mask, or targets with C <= 0 return a negative code and launch
 * nothing. */
int ytvln_expand_ragged_masked(const float* pool_features,   /* [pool_rows, F]                                   */
                               const float* pool_loc,        /* [pool_rows, L], L <= 11                          */
                               const float* pool_probs,      /* [pool_rows, C], or NULL with masking off         */
                               const int64_t* offsets,       /* [pool_frames + 1]                                */
                               int64_t pool_frames, int64_t pool_rows,
                               const int64_t* index,         /* [slots], -1 = padding                            */
                               int64_t slots, int frames, int boxes, int F, int L, int C,
                               const float* p,               /* [slots * boxes] explicit draws, or NULL          */
                               const int64_t* rng,           /* (seed, counter) on the device, or NULL           */
                               int64_t site,
                               void* out_features,           /* [slots * boxes, F] of feature_dtype              */
                               int feature_dtype,            /* YTVLN_DT_F32 | YTVLN_DT_BF16                     */
                               float* out_boxes,             /* [slots * boxes, 12]                              */
                               float* out_targets,           /* [slots * boxes, C], or NULL with masking off     */
                               int64_t* out_masks,           /* [slots * boxes]                                  */
                               int64_t* out_targets_mask,    /* [slots * boxes], together with out_targets       */
                               int64_t* bad,                 /* NULL or [1], accumulates                         */
                               void* stream);
int ytvln_expand_records_masked(const float* pool_features,   /* [pool_rows, F]                                   */
                                const float* pool_geom,       /* [pool_rows, 8]                                   */
                                const float* pool_probs,      /* [pool_rows, C], or NULL with masking off         */
                                const float* pool_global,     /* [pool_frames, F] from ytvln_pool_global_rows_f32 */
                                const int64_t* offsets,       /* [pool_frames + 1]                                */
                                int64_t pool_frames, int64_t pool_rows,
                                const int64_t* index,         /* [slots], -1 = padding                            */
                                const double* view,           /* [slots, 2] heading, next heading, or NULL        */
                                int64_t slots, int frames, int boxes, int F, int C,
                                const float* p, const int64_t* rng, int64_t site,
                                void* out_features, int feature_dtype, float* out_boxes, float* out_targets, int64_t* out_masks,
                                int64_t* out_targets_mask, int64_t* bad, void* stream);

/* out[j, :] = x[idx[j], :] (zeros where idx[j] < 0): row gather in front of the loss-aware prediction heads (only rows that
 * carry a masked-language / masked-vision target are decoded; "next" row of SURVEY.md section 8f).  Backward =
 * ytvln_scatter_add_rows_f32 with skip_idx = -1. */
int ytvln_gather_rows_f32(const float* x, int64_t ldx, const int64_t* idx, int R, int H, float* out, void* stream);

/* Packed rows (csrc/rows.hip; BertModel.skip_padding): both streams of the model on the valid rows of a batch only.
 *   ytvln_rows_plan: flags[rows] (one byte per padded row, non-zero = valid), 1 <= rows < 2^31, capacity >= 1 ->
 *     pack_idx[capacity]  the padded row of each packed row: packed row j is the j-th flagged row in ascending order; -1 past the count;
 *     unpack_idx[rows]    the packed row of each padded row: -1 for unflagged rows and for flagged rows that did not fit;
 *     counts[0] = number of flagged rows, counts[1] = number of flagged rows that did not fit (max(counts[0] - capacity, 0)).
 *     One launch of one workgroup, no atomics, no host sync, deterministic.
 *   ytvln_rows_move_f32 / _bf16: out[j, 0:width] = 0 <= idx[j] < x_rows ? x[idx[j], 0:width] : 0 for j < out_rows; x and out have their own
 *     leading dimensions (elements), a column window is the caller's pointer offset, columns of out past `width` are not touched.  width >= 1;
 *     out_rows = 0 succeeds without a launch.  With pack_idx it packs (and is the backward of the unpack), with unpack_idx it unpacks (and
 *     is the backward of the pack): the two index arrays of a plan describe one partial bijection. */
int ytvln_rows_plan(const uint8_t* flags, int64_t rows, int64_t capacity, int64_t* pack_idx, int64_t* unpack_idx, int64_t* counts, void* stream);
int ytvln_rows_move_f32(const float* x, int64_t ldx, int64_t x_rows, const int64_t* idx, int64_t out_rows, int width, float* out, int64_t ldo,
                        void* stream);
int ytvln_rows_move_bf16(const uint16_t* x, int64_t ldx, int64_t x_rows, const int64_t* idx, int64_t out_rows, int width, uint16_t* out,
                         int64_t ldo, void* stream);

/* Fused (dropout ->) residual add -> LayerNorm (-> dropout).  BertLayerNorm, vilbert.py:213-217 (biased variance, eps
 * inside the sqrt) together with the dropout/add that always precedes it (:322-324, :365-367, :641-648) or follows it
 * (:254-255, :1367-1368).
 *   s = (p_pre > 0 ? dropout(x) : x) + (res ? res : 0);  y = gamma * (s - mean) * rstd + beta;  p_post: y = dropout(y)
 * s_out receives s (may alias x; may be NULL when not training), mean/rstd are [rows] (may be NULL).
 * At most ONE of p_pre / p_post may be > 0, in the forward and in the backward, fp32 and bf16: both masks of a call would come from the same
 * (key, site, row, vector) draw -- fully correlated, identical at p_pre == p_post -- so the combination returns an error. */
int ytvln_ln_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y, float* s_out,
                     float* mean, float* rstd, int64_t rows, int H, float eps, float p_pre, float p_post,
                     const int64_t* rng, int64_t site, void* stream);

/* Backward of the above.  ds = dL/ds (gradient w.r.t. the residual input), dx = gradient w.r.t. x (written only when
 * p_pre > 0; otherwise dx == ds and dx may be NULL).  partial is [nblocks, 2, H] (dgamma then dbeta partial sums, to be
 * reduced with ytvln_colsum_f32); nblocks = ytvln_ln_bwd_blocks(rows).  p_pre and p_post both > 0: an error, as in the forward. */
int ytvln_ln_bwd_blocks(int64_t rows);
int ytvln_ln_bwd_f32(const float* dy, const float* s, const float* mean, const float* rstd, const float* gamma,
                     float* ds, float* dx, float* partial, int64_t rows, int H, float p_pre, float p_post,
                     const int64_t* rng, int64_t site, void* stream);

/* BertEmbeddings.forward, vilbert.py:240-256: s = word[ids] + pos[t] + type[tt]; y = dropout(LN(s)). rows = N*T. */
int ytvln_text_embed_fwd_f32(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos,
                             const float* type, const float* gamma, const float* beta, float* y, float* s_out,
                             float* mean, float* rstd, int64_t rows, int T, int H, float eps, float p_post,
                             const int64_t* rng, int64_t site, void* stream);

/* BertImageEmbeddings.forward after the 2048->Hv projection, vilbert.py:1361-1368:
 *   s = img + W5.loc[0:5] + b5 + W4.loc[5:9] + b4 + W2.loc[9:11] + b2 + E32[(int)loc[11]];  y = dropout(LN(s))
 * img is [rows,H] (already contains its own bias), loc is [rows,12]; W5 [H,5], W4 [H,4], W2 [H,2], E [32,H]. */
int ytvln_image_embed_fwd_f32(const float* img, const float* loc, const float* W5, const float* b5, const float* W4,
                              const float* b4, const float* W2, const float* b2, const float* E, const float* gamma,
                              const float* beta, float* y, float* s_out, float* mean, float* rstd, int64_t rows,
                              int H, float eps, float p_post, const int64_t* rng, int64_t site, void* stream);

/* dz = dy * act'(aux) elementwise (act = YTVLN_EPI_GELU: aux is the pre-activation; YTVLN_EPI_RELU: aux is the output; YTVLN_ACT_SWISH: aux is
 * the pre-activation z, act' = s + z s (1 - s) with s = sigmoid(z)).  Pointers 16-byte aligned; YTVLN_ACT_SWISH also takes unaligned ones
 * (one element per lane then). */
int ytvln_act_bwd_f32(const float* dy, const float* aux, float* dz, int64_t n, int act, void* stream);

/* y = act(z) elementwise for the one activation that is not a GEMM epilogue: act = YTVLN_ACT_SWISH, y = z * sigmoid(z) (vilbert.py:122-123; the
 * forward of BertIntermediate / BertPredictionHeadTransform, vilbert.py:351-354, 864-866, with hidden_act = "swish").  Any n >= 0, y == z allowed
 * (in place); 16 bytes per lane when both pointers are 16-byte aligned, one element per lane otherwise.  Finite for every finite input
 * (sigmoid is formed from exp(-|z|) <= 1).  Other values of act are rejected: gelu / relu stay GEMM epilogues. */
int ytvln_act_fwd_f32(const float* z, float* y, int64_t n, int act, void* stream);

/* h = gelu(z) elementwise, z the pre-activation an YTVLN_EPI_GELU launch of ytvln_gemm_f32 wrote to `aux`: the same device function as that
 * epilogue, so h is the epilogue's output bit for bit (activation recomputation, recompute = "ffn": the FFN node keeps z and rebuilds h in its
 * backward).  Any n >= 0 (n = 0 succeeds with NULL pointers), any alignment, h == z allowed; 16 bytes per lane when both pointers are 16-byte
 * aligned, one element per lane otherwise; nothing is written at or past n.  fp32 only: on the bf16-resident path z is stored rounded, and
 * gelu of the rounded z is not the stored h. */
int ytvln_gelu_fwd_f32(const float* z, float* h, int64_t n, void* stream);

/* y = x * keep / (1 - p): nn.Dropout forward and (applied to dy) backward (lily.py:100). */
int ytvln_dropout_f32(const float* x, float* y, int64_t n, float p, const int64_t* rng, int64_t site, void* stream);

/* bf16-resident forms of the five kernels above (BASELINE configs[4]): rows of x / res / y / s_out / dy / s / ds / dx are bf16 (8-byte aligned),
 * the arithmetic is the fp32 one (values widened on load, rounded to nearest even on store), statistics, gamma / beta, their gradient partials and
 * the embedding tables stay fp32; the dropout masks are the SAME as in the fp32 kernels (one Philox draw per group of four elements).
 * ytvln_ln_bwd_bf16: ds / dx may be NULL when the caller only wants ds_f32, an fp32 copy of ds for the embedding-table gradient kernels.
 * ytvln_ln_fwd_bf16 / ytvln_ln_bwd_bf16 refuse p_pre and p_post both > 0 like their fp32 forms. */
int ytvln_ln_fwd_bf16(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta, uint16_t* y, uint16_t* s_out, float* mean,
                      float* rstd, int64_t rows, int H, float eps, float p_pre, float p_post, const int64_t* rng, int64_t site, void* stream);
int ytvln_ln_bwd_bf16(const uint16_t* dy, const uint16_t* s, const float* mean, const float* rstd, const float* gamma, uint16_t* ds, uint16_t* dx,
                      float* ds_f32, float* partial, int64_t rows, int H, float p_pre, float p_post, const int64_t* rng, int64_t site, void* stream);
int ytvln_text_embed_fwd_bf16(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                              const float* gamma, const float* beta, uint16_t* y, uint16_t* s_out, float* mean, float* rstd, int64_t rows,
                              int T, int H, float eps, float p_post, const int64_t* rng, int64_t site, void* stream);
int ytvln_image_embed_fwd_bf16(const uint16_t* img, const float* loc, const float* W5, const float* b5, const float* W4, const float* b4,
                               const float* W2, const float* b2, const float* E, const float* gamma, const float* beta, uint16_t* y,
                               uint16_t* s_out, float* mean, float* rstd, int64_t rows, int H, float eps, float p_post, const int64_t* rng,
                               int64_t site, void* stream);
/* ytvln_act_bwd_bf16: gelu / relu need 8-byte aligned pointers and n % 4 == 0; YTVLN_ACT_SWISH takes any n and alignment.  ytvln_act_fwd_bf16: as
 * ytvln_act_fwd_f32 on bf16 elements (widened on load, fp32 arithmetic, rounded to nearest even on store). */
int ytvln_act_bwd_bf16(const uint16_t* dy, const uint16_t* aux, uint16_t* dz, int64_t n, int act, void* stream);
int ytvln_act_fwd_bf16(const uint16_t* z, uint16_t* y, int64_t n, int act, void* stream);

/* Fused multi-head attention on the fp32 matrix cores, flash-style (scores never reach HBM).  One entry point serves
 * BertSelfAttention (vilbert.py:284-311), BertImageSelfAttention (:413-440) and both directions of BertBiAttention
 * (:577-616):   ctx[n, i, h*d:(h+1)*d] = softmax_j(q_i.k_j * scale + mask[n, j]) (dropout) . v_j
 *   q: rows n*Tq+i, head h at columns h*d.., leading dimension ldq (so packed QKV projections are consumed in place);
 *   k, v likewise with Tk rows per n; mask: additive [N, Tk] (0 / -10000, vilbert.py:1282,1287) or NULL;
 *   lse [N, heads, Tq] receives log-sum-exp of the scaled+masked scores (saved for backward).  d in {32, 64, 128}. */
int ytvln_attn_fwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                       const float* mask, float* ctx, int64_t ldo, float* lse, int N, int heads, int Tq, int Tk,
                       int d, float scale, float p_drop, const int64_t* rng, int64_t site, void* stream);

/* Backward: delta [N,heads,Tq] is scratch (row sums of dctx*ctx).  dq/dk/dv use the same strided layout as q/k/v and
 * are overwritten. */
int ytvln_attn_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                       const float* mask, const float* ctx, const float* dctx, int64_t ldo, const float* lse,
                       float* delta, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int N,
                       int heads, int Tq, int Tk, int d, float scale, float p_drop, const int64_t* rng, int64_t site,
                       void* stream);

/* Both directions of BertBiAttention (vilbert.py:552-618) in ONE launch per kernel: text queries over region keys/values and region
 * queries over text keys/values are independent problems of complementary shape (T x R and R x T); one grid holds the workgroups of
 * both, so the slots one direction's last partial round would leave idle are filled by the other.  Each problem is described like the
 * arguments of ytvln_attn_fwd_f32 / ytvln_attn_bwd_f32 (forward reads q,k,v,mask and writes ctx,lse; backward reads
 * q,k,v,mask,ctx_in,dctx,lse_in and writes delta,dq,dk,dv); N, heads, d, scale and rng are shared. */
typedef struct ytvln_attn_problem {
    const float *q, *k, *v, *mask;
    const float *ctx_in, *dctx, *lse_in;
    float *ctx, *lse, *delta, *dq, *dk, *dv;
    int64_t ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    int32_t Tq, Tk;
    float p_drop;
    int32_t reserved;
    int64_t site;
    void* keep;      /* bf16 entry points with p_drop > 0: the keep decisions of the dropout, ytvln_attn_keep_bytes(N, heads, Tq, Tk) bytes, 128-byte
                        aligned -- WRITTEN by ytvln_attn_fwd_bf16 (16 64-bit lane masks per 32x32 block of scores), READ by ytvln_attn_bwd_bf16 of the
                        same problem; in a two-problem launch BOTH records need one as soon as either has p_drop > 0; ignored by the fp32 entry points (they
                        regenerate the hash) and by launches without dropout (may be NULL) */
} ytvln_attn_problem;
/* sizeof(ytvln_attn_problem) as the LIBRARY was built: a binding asserts it equals its own record size at load time */
int64_t ytvln_attn_problem_size(void);
int ytvln_attn_fwd_pair(const ytvln_attn_problem* a, const ytvln_attn_problem* b, int N, int heads, int d, float scale,
                        const int64_t* rng, void* stream);
int ytvln_attn_bwd_pair(const ytvln_attn_problem* a, const ytvln_attn_problem* b, int N, int heads, int d, float scale,
                        const int64_t* rng, void* stream);
/* The fp32 backward with a workspace for the stored-dS form (option ATTN_W1 bit 3): the dK/dV kernel writes every 32x32 block of dS it forms
 * to `workspace` and the dQ kernel only contracts those blocks with K instead of recomputing them; delta comes from a small pass of its own
 * in front.  dq, dk, dv and delta are bit-identical to ytvln_attn_bwd_f32 / ytvln_attn_bwd_pair.
 * ytvln_attn_bwd_workspace_elems: pure host code -- the floats a launch of that shape uses, N heads ceil32(Tq) ceil32(Tk) summed over its
 * problems (Tq_b = Tk_b = 0: one problem), or 0 when the launch would not take the form (bit 3 of ATTN_W1 clear, d not 64 / 128, a sequence
 * longer than 512, or a launch whose dK/dV runs in the wave-pair form).  `workspace` (16-byte aligned) is scratch: written and read inside the
 * call's own kernels, in stream order.  NULL, or workspace_elems below that count: the recomputing kernels run, exactly as through the entry
 * points above -- never an error. */
int64_t ytvln_attn_bwd_workspace_elems(int N, int heads, int d, int Tq_a, int Tk_a, int Tq_b, int Tk_b);
int ytvln_attn_bwd_ws_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                          const float* mask, const float* ctx, const float* dctx, int64_t ldo, const float* lse,
                          float* delta, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int N,
                          int heads, int Tq, int Tk, int d, float scale, float p_drop, const int64_t* rng, int64_t site,
                          float* workspace, int64_t workspace_elems, void* stream);
int ytvln_attn_bwd_pair_ws(const ytvln_attn_problem* a, const ytvln_attn_problem* b, int N, int heads, int d, float scale,
                           const int64_t* rng, float* workspace, int64_t workspace_elems, void* stream);
/* The same attention for the bf16-resident path (BASELINE configs[4]): in the problem records q, k, v, ctx, ctx_in, dctx, dq, dk, dv point to
 * BF16 tensors (leading dimensions in elements), mask / lse / lse_in / delta stay fp32; every contraction runs on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation and fp32 softmax, the transposed operands (V^T.P^T, K^T.dS^T, Q^T.dS, dO^T.P) are gathered from the row-major LDS
 * tiles by ds_read_b64_tr_b16.  `b` may be NULL (one problem: self-attention) or the second direction of BertBiAttention.  Head dimension
 * 64 or 128. */
int64_t ytvln_attn_keep_bytes(int N, int heads, int Tq, int Tk);
int ytvln_attn_fwd_bf16(const ytvln_attn_problem* a, const ytvln_attn_problem* b, int N, int heads, int d, float scale,
                        const int64_t* rng, void* stream);
int ytvln_attn_bwd_bf16(const ytvln_attn_problem* a, const ytvln_attn_problem* b, int N, int heads, int d, float scale,
                        const int64_t* rng, void* stream);

/* Per-score additive bias: what the reference adds to the scores beside the key mask -- BertBiAttention's co_attention_mask
 * (vilbert.py:581-582 for the text-over-regions direction, read through `.permute(0,1,3,2)`, and :603-604 for regions over text) and any
 * attention_mask that broadcasts against [N, heads, T, T] in BertSelfAttention / BertImageSelfAttention (:294-297, :423-427):
 *     s[n,h,i,j] = fadd(fadd(fmul(q_i.k_j, scale), mask[n,j]), bias[n,h,i,j]),    bias[n,h,i,j] = ptr[n*stride_n + h*stride_h + i*stride_q + j*stride_k]
 * fp32, strides in ELEMENTS: stride_h = 0 broadcasts over heads, stride_n = 0 over pairs, and a transposed view is read in place by swapping
 * stride_q and stride_k (no copy).  Only 4-byte alignment of `ptr` is required.  The caller's contract: every element
 * (n < N, h < heads, i < Tq, j < Tk) addressed through the strides lies inside the allocation -- the library cannot check an extent.
 * Checked: stride_q and stride_k are non-negative and (Tq-1) stride_q + (Tk-1) stride_k < 2^31 (offsets inside a (pair, head) plane are
 * 32-bit); stride_n and stride_h are 64-bit, may have either sign, and fall under the caller's contract alone.  Values
 * are finite or -inf; a query row whose scores are ALL -inf is NaN in the reference and unspecified here.  The forward / backward entry
 * points below treat the bias as a constant; its gradient is a launch of its own, ytvln_attn_dbias_* further down (unfused by design).  A NULL record or a NULL `ptr` means "no bias", so one call serves a pair with one biased side;
 * a launch in which no problem has a bias runs exactly the kernels of the entry points above.  Problems WITH a bias run the two-wave / wave-pair
 * fp32 kernels (never the one-wave forms selected by ATTN_W1) -- decided per launch.  softmax, lse, dropout decisions: unchanged. */
typedef struct ytvln_attn_bias {
    const float* ptr;
    int64_t stride_n, stride_h, stride_q, stride_k;
} ytvln_attn_bias;
/* sizeof(ytvln_attn_bias) as the LIBRARY was built (see ytvln_attn_problem_size) */
int64_t ytvln_attn_bias_size(void);
/* ytvln_attn_fwd_pair / ytvln_attn_bwd_pair (fp32) and ytvln_attn_fwd_bf16 / ytvln_attn_bwd_bf16 with a bias record next to each problem
 * (replaces vilbert.py:577-582, :597-604 and the broadcast adds of :294-297, :423-427).  `b` may be NULL (one problem: self-attention) in all
 * four; N, heads, d must be positive.  In the bf16 forms the bias stays fp32, like mask and lse. */
int ytvln_attn_fwd_bias_f32(const ytvln_attn_problem* a, const ytvln_attn_bias* bias_a, const ytvln_attn_problem* b,
                            const ytvln_attn_bias* bias_b, int N, int heads, int d, float scale, const int64_t* rng, void* stream);
int ytvln_attn_bwd_bias_f32(const ytvln_attn_problem* a, const ytvln_attn_bias* bias_a, const ytvln_attn_problem* b,
                            const ytvln_attn_bias* bias_b, int N, int heads, int d, float scale, const int64_t* rng, void* stream);
int ytvln_attn_fwd_bias_bf16(const ytvln_attn_problem* a, const ytvln_attn_bias* bias_a, const ytvln_attn_problem* b,
                             const ytvln_attn_bias* bias_b, int N, int heads, int d, float scale, const int64_t* rng, void* stream);
int ytvln_attn_bwd_bias_bf16(const ytvln_attn_problem* a, const ytvln_attn_bias* bias_a, const ytvln_attn_problem* b,
                             const ytvln_attn_bias* bias_b, int N, int heads, int d, float scale, const int64_t* rng, void* stream);
/* ytvln_attn_probs_f32 with the bias added to the scores (vilbert.py:585, :607 with use_co_attention_mask: the probabilities the reference
 * returns are the biased ones); `bias` NULL or bias->ptr NULL = ytvln_attn_probs_f32. */
int ytvln_attn_probs_bias_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* mask, const ytvln_attn_bias* bias,
                              const float* lse, float* probs, int N, int heads, int Tq, int Tk, int d, float scale, void* stream);

/* Gradient with respect to the per-score bias (what autograd gives a float attn_mask of torch attention; the reference never trains one).  The
 * bias is added to the final score, so dBias = dS.  UNFUSED by design: a launch of its own recomputes, per 32x32 block of scores on the fp32
 * matrix cores (v_mfma_f32_32x32x2_f32; bf16 operands are widened exactly), two of the backward's five products,
 *     s  = fadd(fadd(fmul(q_i.k_j, scale), mask[n,j]), bias[n,h,i,j])      the forward's score, same roundings
 *     p  = exp(s - lse[n,h,i])          dp = dO_i.v_j          dS[n,h,i,j] = p * (keep/(1 - p_drop) * dp - delta[n,h,i])
 * and stores one score-sized fp32 tensor; the forward / backward kernels and every existing launch are untouched.  `p` is the problem record
 * of the BACKWARD launch of the same problem and the call is enqueued AFTER that launch on the same stream: it reads q, k, v, mask, dctx,
 * lse_in and the delta = sum_c dO.O that launch wrote (plus Tq, Tk, p_drop, site, the leading dimensions).  Dropout decisions are the
 * forward's: _f32 re-draws the hash from (rng, site, element) exactly as ytvln_attn_fwd_f32 does, _bf16 reads the keep bits ytvln_attn_fwd_bf16
 * stored (p->keep).  `bias`: the record of the FORWARD values (NULL or NULL ptr: none was added).  A score with p == 0 (masked key, -inf bias)
 * gets exactly 0.
 *   `out` is described like the bias -- fp32 pointer (WRITTEN, every addressed element) plus element strides over [N or 1, heads or 1, Tq, Tk];
 * checked like a bias (4-byte alignment, non-negative stride_q / stride_k, plane span < 2^31); the addressed elements must not overlap.
 * stride_n == 0 means extent 1 over pairs and stride_h == 0 extent 1 over heads: such a dimension is SUMMED OVER inside the library, in fp32,
 * without atomics and in a fixed order (bit-reproducible): the reduced (pair, head) problems are numbered r = n * heads + h (pair-major) over
 * the reduced dimensions only, cut into ytvln_attn_dbias_chunks(...) runs of equal length (the last one shorter); one wave adds the blocks of a
 * run in ascending r; with more than one run each writes a partial plane to `workspace` and a second launch adds the runs in ascending order.
 *   workspace: ytvln_attn_dbias_workspace_elems(out, N, heads, Tq, Tk) floats = runs x the dense size of the output when runs > 1, else 0 (may
 * be NULL then).  The number of runs depends on the shapes alone, never on the device: 1 when at most 16 problems are summed per output plane
 * ([N,heads,..] always, [N,1,..] up to 16 heads); otherwise as many as bring the launch to 1024 waves, but at least 4 problems per run.
 *   d: _f32 any multiple of 4 up to 128, _bf16 64 or 128 (q, k, v, dctx are bf16 there; mask, lse, delta, bias, out stay fp32). */
int ytvln_attn_dbias_chunks(const ytvln_attn_bias* out, int N, int heads, int Tq, int Tk);
int64_t ytvln_attn_dbias_workspace_elems(const ytvln_attn_bias* out, int N, int heads, int Tq, int Tk);
int ytvln_attn_dbias_f32(const ytvln_attn_problem* p, const ytvln_attn_bias* bias, const ytvln_attn_bias* out, float* workspace,
                         int64_t workspace_elems, int N, int heads, int d, float scale, const int64_t* rng, void* stream);
int ytvln_attn_dbias_bf16(const ytvln_attn_problem* p, const ytvln_attn_bias* bias, const ytvln_attn_bias* out, float* workspace,
                          int64_t workspace_elems, int N, int heads, int d, float scale, const int64_t* rng, void* stream);

/* probs[n,h,i,j] = exp(q_i.k_j*scale + mask - lse): the attention_probs tensor the reference returns when
 * output_all_attention_masks=True (vilbert.py:300, 311).  Diagnostic path, not on the training step. */
int ytvln_attn_probs_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* mask, const float* lse,
                         float* probs, int N, int heads, int Tq, int Tk, int d, float scale, void* stream);

/* F.cross_entropy(logits, target, ignore_index) (utils_init.py:133-135, 141) -- also with -inf padded logits.
 * fwd: row_lse [M], out[0] = mean loss over non-ignored rows (NaN when none, like the reference), out[1] = their count.
 * bwd: dlogits = (softmax - onehot) * gout[0] / count for valid rows, 0 otherwise. */
int ytvln_ce_fwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float* row_lse,
                     float* row_loss, float* out, int M, int V, void* stream);
int ytvln_ce_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, const float* row_lse,
                     const float* out, const float* gout, float* dlogits, int64_t ldd, int M, int V, void* stream);
/* bf16-resident path (BASELINE configs[4]): the same two kernels on BF16 logits (what the decoders write there); the loss, row_lse and out
 * stay fp32; the gradient is bf16 and ZEROS are written to its padding columns [V, ldd), so the buffer feeds ytvln_gemm_bf16 as a zero-padded
 * operand (YTVLN_GEMM_A_ZERO_PADDED) as it stands */
int ytvln_ce_fwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float* row_lse,
                      float* row_loss, float* out, int M, int V, void* stream);
int ytvln_ce_bwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, const float* row_lse,
                      const float* out, const float* gout, uint16_t* dlogits, int64_t ldd, int M, int V, void* stream);

/* Masked KL of utils_init.py:117-128: sum_rows mask * sum_c t*(log t - log_softmax(pred)) / max(1, sum mask). */
int ytvln_kl_fwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask,
                     float* row_lse, float* row_loss, float* out, int M, int C, void* stream);
int ytvln_kl_bwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask,
                     const float* row_lse, const float* out, const float* gout, float* dpred, int64_t ldd, int M,
                     int C, void* stream);
/* bf16 predictions in, bf16 gradient + zeroed padding out, as ytvln_ce_*_bf16 (targets stay fp32) */
int ytvln_kl_fwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                      float* row_loss, float* out, int M, int C, void* stream);
int ytvln_kl_bwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, const float* row_lse,
                      const float* out, const float* gout, uint16_t* dpred, int64_t ldd, int M, int C, void* stream);

/* ---- stats forms of the two losses above: label smoothing and the row arg-max from the same pass (opt-in; fp32 or bf16 logits) ----------
 * ytvln_ce_stats_fwd_*: one workgroup per non-ignored row streams the row ONCE for the log-sum-exp (the bits of ytvln_ce_fwd_*), sx = the
 * sum and nv = the number of its logits that are not -inf, and the arg-max.  Two launches, no atomics, deterministic.
 *   row loss  = (1 - eps) (lse - x[t]) + eps (lse - sx / nv),  eps = label_smoothing in [0, 1)
 *               = F.cross_entropy(label_smoothing = eps) when no logit is -inf; with -inf logits (padded ranking options) the smoothing
 *               mass is spread over the nv other classes only, where torch spreads it over all V and returns +inf.  eps = 0: the bits of
 *               ytvln_ce_fwd_*.  A -inf TARGET logit gives +inf; a target outside [0, V) that is not the ignore index, or a NaN logit, NaN.
 *   row_top[r] = arg-max of row r: the LOWEST index among equal maxima, a NaN counts as the maximum (torch.argmax); -1 for an ignored row
 *   row_aux[r] = nv (read by the backward);  row_lse, row_loss: as ytvln_ce_fwd_*
 *   out[0] = mean loss over the non-ignored rows (NaN when none), out[1] = their count, out[2] = hits = #(non-ignored rows with
 *   row_top == target), out[3] = rows counted = out[1].  hits and counts are whole numbers in fp32: M <= 2^24.
 * ytvln_ce_smooth_bwd_*: dlogits[c] = (p_c - (1 - eps) [c == t] - (eps / nv) [x_c != -inf]) * gout[0] / count, p = softmax; a -inf column
 * gets p_c = 0 and no smoothing term.  Stores as ytvln_ce_bwd_*: fp32 into columns [0, V); bf16 rounded once, zeros up to ldd.  `out` is
 * the forward's.  With eps = 0 it writes what ytvln_ce_bwd_* writes.
 * ytvln_kl_stats_fwd_*: ytvln_kl_fwd_* (same row_lse, row_loss, out[0], out[1] -- ytvln_kl_bwd_* is its backward) plus row_top[r] = arg-max
 * of the prediction row (-1 where mask == 0), row_hit[r] = 1 where it equals the arg-max of the target row (same tie rule) and mask != 0,
 * out[2] = sum(row_hit), out[3] = #(mask != 0), not clamped.
 * All of them: ld (ldt, ldd) >= V; the columns beyond V are never read.  Bad arguments (null pointer, M outside 1 .. 2^24, a leading
 * dimension below V, label_smoothing outside [0, 1) or NaN) return a negative code before anything is launched. */
int ytvln_ce_stats_fwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                           float* row_lse, float* row_aux, float* row_loss, int64_t* row_top, float* out, int M, int V, void* stream);
int ytvln_ce_stats_fwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                            float* row_lse, float* row_aux, float* row_loss, int64_t* row_top, float* out, int M, int V, void* stream);
int ytvln_ce_smooth_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                            const float* row_lse, const float* row_aux, const float* out, const float* gout, float* dlogits, int64_t ldd,
                            int M, int V, void* stream);
int ytvln_ce_smooth_bwd_bf16(const uint16_t* logits, int64_t ld, const int64_t* target, int64_t ignore_index, float label_smoothing,
                             const float* row_lse, const float* row_aux, const float* out, const float* gout, uint16_t* dlogits, int64_t ldd,
                             int M, int V, void* stream);
int ytvln_kl_stats_fwd_f32(const float* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                           float* row_loss, int64_t* row_top, float* row_hit, float* out, int M, int C, void* stream);
int ytvln_kl_stats_fwd_bf16(const uint16_t* pred, int64_t ld, const float* target, int64_t ldt, const int64_t* mask, float* row_lse,
                            float* row_loss, int64_t* row_top, float* row_hit, float* out, int M, int C, void* stream);

/* F.binary_cross_entropy_with_logits(x, t, pos_weight) with mean reduction (utils_init.py:143, 160-161). n <= 65536.
 * pos_weight is a DEVICE scalar or NULL.  bwd writes dx. */
int ytvln_bce_fwd_f32(const float* x, const float* t, const float* pos_weight, float* out, int n, void* stream);
int ytvln_bce_bwd_f32(const float* x, const float* t, const float* pos_weight, const float* gout, float* dx, int n,
                      void* stream);

/* Fused AdamW of vilbert/optimization.py:141-187 over flat arenas.  chunks is a DEVICE array of nchunks records
 * {int64 offset, int64 length, float weight_decay, float pad} (24 bytes); hyper is a DEVICE array
 * {beta1, beta2, eps, step_size = lr*sqrt(1-b2^t)/(1-b1^t), lr} of floats (updated by the host per step; graph-safe).
 *   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= step_size * m/(sqrt(v)+eps);  p -= lr*wd*p   (decay after update)
 * grad_scale multiplies g on the fly (1/world_size after a summed all-reduce). */
int ytvln_adamw_f32(float* p, const float* g, float* m, float* v, const void* chunks, int nchunks, const float* hyper,
                    float grad_scale, void* stream);
/* the same step, ALSO writing bf16(p) (round to nearest even) at the same offsets of a bf16 arena: the weight operands of the bf16-resident
 * path are refreshed by the optimizer step itself (+2 bytes per parameter, no cast pass) */
int ytvln_adamw_f32_bf16copy(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                             const float* hyper, float grad_scale, void* stream);
/* the same step reading bf16 gradients (the bf16 data-parallel exchange: the SUM over ranks, rounded to bf16, at the arena's offsets):
 * g = float(g_bf16) * grad_scale, otherwise bit-identical to ytvln_adamw_f32 fed the widened values.  p_bf16 may be NULL (no weight copy). */
int ytvln_adamw_f32_gbf16(float* p, const uint16_t* g_bf16, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                          const float* hyper, float grad_scale, void* stream);
/* g_bf16[o : o+len] = bf16(g[o : o+len]) (round to nearest even) for every record of an AdamW chunk table: the send buffer of the bf16
 * exchange, one workgroup per record; elements outside the table are not written.  Both bases 16-byte aligned. */
int ytvln_grad_pack_bf16(const float* g, uint16_t* g_bf16, const void* chunks, int nchunks, void* stream);
/* Global gradient-norm clipping fused into the step (the reference has none; torch.nn.utils.clip_grad_norm_ semantics), three launches:
 * ytvln_grad_sumsq -> ytvln_grad_clip_coef -> ytvln_adamw_clip.  No atomics, every summation order fixed: results are reproducible bit
 * for bit.  `dtype` / `g_dtype`: YTVLN_DT_F32 (the fp32 gradient arena) or YTVLN_DT_BF16 (the bf16 sums of the bf16 exchange), nothing else.
 *   partials[i] = sum of g[o : o+len]^2 over record i of an AdamW chunk table, accumulated in fp32: one workgroup and one float per record.
 * g 16-byte aligned; reads 4 (bf16: 2) bytes per element. */
int ytvln_grad_sumsq(const void* g, int dtype, const void* chunks, int nchunks, float* partials, void* stream);
/* Sigma = sum of the n partials (of every table of the step) in fp64, then the DEVICE record clip[0..3] (16-byte aligned):
 *   clip[0] = norm = grad_scale * sqrt(Sigma)          the norm of the gradient AdamW applies (after the 1/world average)
 *   clip[1] = coef = min(1, max_norm / (norm + 1e-6))  exactly 1 when max_norm = +inf (measure only); NaN norm -> NaN, infinite norm -> 0
 *   clip[2] = skip = 1 when skip_nonfinite != 0 and norm is not finite, else 0
 *   clip[3] += skip                                    running count of skipped steps (read, incremented, written here)
 * max_norm > 0 (NaN rejected).  n = 0: norm 0, coef 1, skip 0. */
int ytvln_grad_clip_coef(const float* partials, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float* clip,
                         void* stream);
/* ytvln_adamw_f32 / _bf16copy / _gbf16 in one entry (g_dtype selects the gradient operand, p_bf16 may be NULL) reading `clip`: with
 * clip[2] != 0 the launch leaves p, m, v and p_bf16 untouched; otherwise g is scaled by grad_scale * clip[1].  With clip[1] = 1 and clip[2] = 0
 * it is bit-identical to those three. */
int ytvln_adamw_clip(float* p, const void* g, int g_dtype, float* m, float* v, uint16_t* p_bf16, const void* chunks, int nchunks,
                     const float* hyper, float grad_scale, const float* clip, void* stream);
/* LAMB layer-wise trust ratio (You et al., 2020; the reference has none): the AdamW direction rescaled per parameter tensor, three launches
 * per chunk table: ytvln_lamb_stage1 -> ytvln_lamb_trust -> ytvln_lamb_stage2.  With g = g_in * grad_scale (* clip[1] with a clip record):
 *   m = beta1 m + (1-beta1) g;  v = beta2 v + (1-beta2) g^2;  r = hyper[5] * m / (sqrt(v) + eps) + wd * p    (decay INSIDE the direction)
 *   trust(tensor) = ||p|| / ||r|| when wd != 0 and both norms are finite and > 0, else 1;   p -= lr * trust * r
 * hyper[5] is the bias correction b = sqrt(1-beta2^t)/(1-beta1^t) (1 without it), so hyper[3] = lr * b as for ytvln_adamw_f32.  The norms
 * run over whole tensors.  No atomics, every summation order fixed: results are reproducible bit for bit.  `clip` is the record of
 * ytvln_grad_clip_coef or NULL (no clipping); with clip[2] != 0 all three launches return before writing anything.
 *   stage 1: reads p, g, m, v; writes m, v and, for record i of the table, partials[2i] = sum p^2, partials[2i+1] = sum r^2 (fp32, one
 * workgroup per record; r is not stored).  g_dtype: YTVLN_DT_F32 or YTVLN_DT_BF16, nothing else.  Arenas 16-byte, partials 8-byte aligned.
 * 24 bytes per parameter. */
int ytvln_lamb_stage1(const float* p, const void* g, int g_dtype, float* m, float* v, const void* chunks, int nchunks, const float* hyper,
                      float grad_scale, const float* clip, float* partials, void* stream);
/* One wave per tensor of the table.  The records of a tensor are contiguous in the table: tensor_first[t] is the first record of the
 * table's t-th tensor (ntensors + 1 entries, ascending), rec_tensor[i] the index of record i's tensor in the trust / report buffers.
 * Sums the tensor's partials in fp64 and writes trust[k] and the row report[4k .. 4k+3] = {||p||, ||r||, trust, 0} (16-byte aligned),
 * k = rec_tensor[tensor_first[t]]; wd is read from the tensor's first record. */
int ytvln_lamb_trust(const float* partials, const void* chunks, const int32_t* tensor_first, const int32_t* rec_tensor, int ntensors,
                     float* trust, float* report, const float* clip, void* stream);
/* stage 2: reads p and the m, v stage 1 stored, recomputes r with stage 1's expression (bit-identical), applies
 * p -= lr * trust[rec_tensor[i]] * r and writes p, and bf16(p) into p_bf16 when that is not NULL.  16 bytes per parameter, 18 with the copy. */
int ytvln_lamb_stage2(float* p, const float* m, const float* v, uint16_t* p_bf16, const void* chunks, int nchunks, const float* hyper,
                      const float* trust, const int32_t* rec_tensor, const float* clip, void* stream);
/* EMA of the weights (timm's ModelEmaV2; the reference has none): a shadow arena e with the offsets of the parameter arena, updated by a
 * launch of its own behind the update launches of a chunk table:
 *   e = fma(w, p - e, e)   in fp32, w = hyper[6] = float32(1 - decay), p: the parameter the update just wrote
 * (the lerp form: p == e leaves e bit-unchanged for every w).  `clip` is the record of ytvln_grad_clip_coef or NULL; with clip[2] != 0 (a
 * skipped step) the launch returns before writing anything.  One workgroup per record; elements outside the table are not touched; p is
 * read-only.  Both arenas 16-byte aligned.  12 bytes per parameter. */
int ytvln_ema_update(const float* p, float* e, const void* chunks, int nchunks, const float* hyper, const float* clip, void* stream);
/* Exchanges p[i] and e[i] for every element of the table (evaluation with the shadow weights; two calls are the identity) and, when p_bf16
 * is not NULL, writes p_bf16[i] = bf16(new p[i]) (round to nearest even) at the same offsets.  All arenas 16-byte aligned.  16 bytes per
 * parameter, 18 with the copy. */
int ytvln_ema_swap(float* p, float* e, uint16_t* p_bf16, const void* chunks, int nchunks, void* stream);
/* Per-tensor gradient / weight statistics (the reference has none): two read-only launches per chunk table behind the update launches, so
 * g is the gradient the update read and p the parameter it wrote (unchanged on a skipped step: there is no clip record here, a skipped step
 * reports as any other).  No atomics, every order fixed by the tables alone: two launches on the same inputs give the same bits.  An
 * element is non-finite when it is an infinity or a NaN; sums and maxima run over the finite elements only.
 *   stage 1: one workgroup per record; reads [offset, offset + length) of p and g and nothing else (8 bytes per parameter, 6 with bf16
 * gradients) and writes partials[4i .. 4i+3] = {sum g^2, max |g|, sum p^2, max |p|} (sums accumulated in fp32) and bad[2i], bad[2i+1] = the
 * number of non-finite elements of g and of p in record i.  g_dtype: YTVLN_DT_F32 or YTVLN_DT_BF16, nothing else (bf16 widens exactly).
 * Arenas and partials 16-byte, bad 8-byte aligned. */
int ytvln_tensor_stats_stage1(const float* p, const void* g, int g_dtype, const void* chunks, int nchunks, float* partials, int32_t* bad,
                              void* stream);
/*   stage 2: one wave per tensor of the table (tensor_first, rec_tensor as for ytvln_lamb_trust; any number of records per tensor).  Sums
 * the tensor's partials in fp64 in record order, takes the maxima and writes, with k = rec_tensor[tensor_first[t]],
 *   stats[4k .. 4k+3] = {float(grad_scale * sqrt(sum g^2)) (in double, rounded once), float(grad_scale) * max |g| (one fp32 product),
 *                        float(sqrt(sum p^2)), max |p|}      an empty finite set gives 0 and 0; 16-byte aligned
 *   counts[3k .. 3k+2] = {non-finite elements of g, of p, launches so far in which this tensor had a non-finite g}   int64; the third entry
 * is read, incremented and written here, as ytvln_grad_clip_coef does for clip[3]. */
int ytvln_tensor_stats_stage2(const float* partials, const int32_t* bad, const int32_t* tensor_first, const int32_t* rec_tensor,
                              int ntensors, float grad_scale, float* stats, int64_t* counts, void* stream);

/* ---- heads of the downstream-task model (VILBertForVLTasks / SimpleClassifier, vilbert.py:1457-1535) -------------------------------------
 * None of these uses an atomic: every reduction runs in an order fixed by the shapes alone, so two launches on the same inputs give the
 * same bits.
 *
 * Weight normalisation with dim = None (vilbert.py:1522-1535: weight_norm(nn.Linear(...), dim=None)): w = v g / |v|_F with ONE scalar g (a
 * device pointer) per matrix of n elements.  Forward: stat[0] = |v|_2 over all n elements, stat[1] = g / stat[0], w[i] = v[i] stat[1], and
 * w_bf16[i] (when not NULL, 8-byte aligned) the round-to-nearest-even copy of w[i].  |v| = 0 is not special-cased (the reference yields
 * non-finite values there too).  Backward, from dw = dL/dw and the forward's stat: dg = <dw, v> / |v|, dv = s dw - (s <dw, v> / |v|^2) v with
 * s = stat[1]; dv and dg are plain stores (they may point into gradient-arena slots).  The sums run in two stages -- fixed contiguous chunks
 * per workgroup, then the partials in index order -- through `workspace` of ytvln_weight_norm_workspace_elems(n) floats, which is scratch
 * inside the call.  v, w, dw, dv 16-byte aligned; any n > 0. */
int64_t ytvln_weight_norm_workspace_elems(int64_t n);
int ytvln_weight_norm_fwd_f32(const float* v, const float* g, int64_t n, float* w, uint16_t* w_bf16, float* stat, float* workspace, void* stream);
int ytvln_weight_norm_bwd_f32(const float* v, const float* dw, const float* stat, int64_t n, float* dv, float* dg, float* workspace, void* stream);

/* A Linear with ONE output feature over every row, with the dropout in front of it and the additive region mask behind it
 * (vilbert.py:1517-1518: vision_logit = Linear(v_hidden, 1)(dropout(sequence_output_v)) + (1 - image_attention_mask) * -10000, and
 * linguisic_logit likewise without the mask term):
 *   out[r] = (sum_c k(r,c) x[r,c] w[c] + bias) + (1 - mask[r]) * -10000
 * x is [rows, H] with leading dimension ldx, fp32 or bf16; w is fp32 [H]; bias fp32 [1] or NULL; mask fp32 [rows] of 0 / 1 or NULL; out is
 * fp32 [rows].  k(r,c) is the keep-scale ytvln_dropout_f32 applies at flat element r * H + c of the same (rng, site) -- independent of ldx --
 * and 1 when p == 0 (rng may then be NULL).  One wave per row, 16 bytes per lane, fp32 accumulation.
 * Backward, in one pass over x: dx[r,c] = k(r,c) dy[r] w[c] in x's type (dx may be NULL), dw[c] = sum_r dy[r] k(r,c) x[r,c], db = sum_r dy[r]
 * (db may be NULL); the mask gets no gradient.  The row sums go through `workspace` of ytvln_row_logit_workspace_elems(rows, H) floats: each
 * workgroup owns a contiguous run of rows and writes one partial row, a second kernel adds the partial rows in run order.
 * H % 4 == 0 (fp32) or H % 8 == 0 (bf16), H <= 2048; ldx / lddx multiples of the same granule; x, w, dx, dw, workspace 16-byte aligned;
 * 0 <= p < 1. */
int64_t ytvln_row_logit_workspace_elems(int64_t rows, int H);
int ytvln_row_logit_fwd_f32(const float* x, int64_t ldx, const float* w, const float* bias, const float* mask, float* out, int64_t rows, int H,
                            float p, const int64_t* rng, int64_t site, void* stream);
int ytvln_row_logit_fwd_bf16(const uint16_t* x, int64_t ldx, const float* w, const float* bias, const float* mask, float* out, int64_t rows, int H,
                             float p, const int64_t* rng, int64_t site, void* stream);
int ytvln_row_logit_bwd_f32(const float* x, int64_t ldx, const float* w, const float* dy, int64_t rows, int H, float p, const int64_t* rng,
                            int64_t site, float* dx, int64_t lddx, float* dw, float* db, float* workspace, void* stream);
int ytvln_row_logit_bwd_bf16(const uint16_t* x, int64_t ldx, const float* w, const float* dy, int64_t rows, int H, float p, const int64_t* rng,
                             int64_t site, uint16_t* dx, int64_t lddx, float* dw, float* db, float* workspace, void* stream);

/* ---- losses of the downstream tasks (VQA-style answer classification over vil_prediction, grounding over vision_logit) ------------------
 * Row-wise soft-target BCE with logits over a matrix x[M, C] (fp32, leading dimension ldx) and targets t[M, C] (fp32, ldt), any M * C:
 *   term(r,c) = (1 - t) x + (1 + (w(c) - 1) t) log(1 + exp(-x))        the term of ytvln_bce_fwd_f32
 *   w(c) = pos_weight[c * pw_stride];  pos_weight NULL: w = 1;  pw_stride 0: one DEVICE scalar, 1: one weight per class (torch's pos_weight)
 *   loss = scale * sum(term) / (M C)                                    scale = C: the sum over classes, averaged over the rows
 * fwd, two launches: one workgroup per row streams x and t once and writes row_loss[r], row_top[r] = the LOWEST index of the row's maximum
 * logit (torch.argmax's tie rule) and row_hit[r] = t[r, row_top[r]]; a single workgroup then writes out[0] = float(sum(row_loss) * scale /
 * (M C)) and out[1] = sum(row_hit), both sums in fp64.  A row holding a NaN logit makes the loss NaN; its row_top / row_hit are unspecified
 * (in bounds).  bwd, one launch: dx[r,c] = ((1 - t) - (1 + (w(c) - 1) t) / (1 + exp(x))) * gout[0] * scale / (M C) into columns [0, C) of dx
 * (leading dimension lddx; padding columns are not written); t and pos_weight get no gradient.
 * No atomics, every summation order fixed by the shapes alone: two launches on the same inputs give the same bits.  fp32 only (both
 * producers, SimpleClassifier and ytvln_row_logit_fwd_*, write fp32 in every precision mode).  Plain 4-byte loads and stores: every float
 * pointer 4-byte aligned, row_top 8-byte aligned, any ldx, ldt, lddx >= C.  scale must be finite. */
int ytvln_bce_rows_fwd_f32(const float* x, int64_t ldx, const float* t, int64_t ldt, const float* pos_weight, int pw_stride, float scale,
                           float* row_loss, float* row_hit, int64_t* row_top, float* out, int M, int C, void* stream);
int ytvln_bce_rows_bwd_f32(const float* x, int64_t ldx, const float* t, int64_t ldt, const float* pos_weight, int pw_stride, float scale,
                           const float* gout, float* dx, int64_t lddx, int M, int C, void* stream);

/* ---- data-parallel gradient exchange: RCCL over xGMI ------------------------------------------------------------------------
 * Replaces DistributedDataParallel over NCCL (utils/distributed.py:63-104: init_process_group("nccl") + DDP's bucketed all-reduce).
 * librccl is resolved with dlopen at run time (no link dependency): an explicit path, else a librccl already mapped into the
 * process (PyTorch's own copy -- same HIP runtime, so streams and device pointers interoperate), else the loader's default.
 * A communicator is an opaque handle owned by the caller (the one piece of state that outlives a call); collectives are
 * asynchronous on the stream they are given and operate IN PLACE on device memory; nothing here synchronises or allocates
 * device memory.  The 128-byte unique id is created on rank 0 and carried to the other ranks by the host (env:// store). */
enum { YTVLN_DT_F32 = 0, YTVLN_DT_F64 = 1, YTVLN_DT_BF16 = 2, YTVLN_DT_I64 = 3, YTVLN_DT_U8 = 4 };
enum { YTVLN_RED_SUM = 0, YTVLN_RED_MAX = 1, YTVLN_RED_MIN = 2 };
#define YTVLN_RCCL_UNIQUE_ID_BYTES 128
int ytvln_rccl_load(const char* path);                 /* path may be NULL / "" (see the resolution order above)            */
const char* ytvln_rccl_library_path(void);            /* file the nccl* symbols were bound from ("" before a load)           */
int ytvln_rccl_version(int* version);                  /* NCCL_VERSION_CODE of the loaded library                              */
int ytvln_rccl_unique_id(void* id_out, int64_t bytes); /* ncclGetUniqueId; bytes must be YTVLN_RCCL_UNIQUE_ID_BYTES           */
/* ncclCommInitRank (collective over all `world` ranks; blocks until they all arrive).  device >= 0: hipSetDevice first. */
int ytvln_rccl_init(void** comm_out, const void* id, int64_t id_bytes, int rank, int world, int device);
/* in-place all-reduce of `count` elements; dtype / op from the enums above */
int ytvln_rccl_allreduce(void* comm, void* buf, int64_t count, int dtype, int op, void* stream);
/* SUM all-reduce of `nslices` contiguous slices base[offsets[i] : offsets[i]+counts[i]] (HOST arrays) of one flat fp32 gradient
 * arena as ONE RCCL group: the buckets of an optimizer step without a host round trip between them. */
int ytvln_rccl_allreduce_slices_f32(void* comm, float* base, const int64_t* offsets, const int64_t* counts, int nslices,
                                    void* stream);
/* the same for an arena of any element type of the enum above (offsets / counts in ELEMENTS): with YTVLN_DT_BF16, the opt-in bf16 gradient
 * exchange (ytvln_grad_pack_bf16 -> this -> ytvln_adamw_f32_gbf16) moves half the bytes of the fp32 one over xGMI */
int ytvln_rccl_allreduce_slices(void* comm, void* base, int dtype, const int64_t* offsets, const int64_t* counts, int nslices,
                                void* stream);
/* in-place byte broadcast from `root` (DDP's rank-0 weight broadcast at wrap time) */
int ytvln_rccl_broadcast(void* comm, void* buf, int64_t bytes, int root, void* stream);
int ytvln_rccl_async_error(void* comm);                /* 0 = healthy; negative + ytvln_last_error() otherwise                 */
int ytvln_rccl_destroy(void* comm);                    /* ncclCommDestroy; NULL is a no-op                                     */

#ifdef __cplusplus
}
#endif
#endif /* YTVLN_H */
