/*
 * dsg_debug.h -- the test bench of libdsg.so: every dsg_debug_* and dsg_profile_* entry point, with its structs and selector constants.
 *
 * dsg.h is what an integrator, a trainer or an evaluator binds; nothing there needs this header, and dsg.h does not include it.  The
 * same library exports both sets (diffusesg_amd/lib.py binds both; tests/test_abi.py holds each header to its own export list), and
 * DSG_ABI_VERSION of dsg.h counts the argument lists of both.  Conventions are dsg.h's: 0 on success, a negative dsg_status otherwise;
 * device pointers unless a parameter says HOST; `stream` is a hipStream_t passed as void*.  The hooks are here for the tests and the
 * measurement tools of this repository and may change with them.
 *
 * Ordered by what is hooked: the handle's state, the fp32 forward's kernels, the bf16 / split-bf16 GEMMs and row passes, the bf16 block
 * pipeline, the training kernels, guidance.  Only the first group takes a handle; the others fill a launcher's arguments from their
 * parameters, launch once and synchronise `stream`.
 */
#ifndef DSG_DEBUG_H
#define DSG_DEBUG_H

#include "dsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ======== handle state: taps, poison, the need / dedup / read-out lists, profile ======== */

/* Debug: copy the named stage's activation (e.g. "down0.block0") of the next dsg_denoise call to
 * `dst` (device, capacity in floats).  Token-major [B, T, C]. */
int dsg_debug_tap(dsg_handle h, const char *stage, float *dst, int64_t capacity);
void dsg_debug_clear_taps(dsg_handle h);

/* Test only: fills every scratch buffer that exists on the handle (step tables, training arenas) and in batch size B's workspace (created
 * first if there is none) with `pattern`, on `stream`: 1 zeros, 2 quiet NaN (0x7fc00000; both bf16 halves are NaN too), 3 1.0e30f,
 * 4 finite pseudo-random values of unit scale with random sign, a function of (seed, element index).  A stand-in for stale contents
 * between two calls: every output of every entry point must be bit-identical whatever the pattern (tests/test_workspace_poison.py;
 * the buffer classes are DESIGN.md's "what a forward may assume about its workspace").  The five buffers whose contract is "finite"
 * (x, y, att, hid, stats) take patterns 1, 3 and 4 but not NaN; buffers read as an index, a count, a byte mask, a seed or an address,
 * and the weights, are never written.  Not to be called during stream capture. */
int dsg_debug_poison(dsg_handle h, int32_t B, int32_t pattern, uint64_t seed, void *stream);

/* Masked-token pruning (option "prune_masked", default 1).  Everything a forward returns is masked with the node flags, so on the
 * up path only tokens that share a window with a needed token of the following stage are computed; the lists of needed 8-token runs /
 * windows are derived on the device whenever flags are staged (dsg_denoise, dsg_precond, dsg_sample).  Results are unchanged bit for
 * bit.  Rows nobody reads are left STALE in the workspace activations, so workspace intermediates are only meaningful through
 * dsg_debug_tap -- which, like the split / bf16 modes and 10 x 10 windows, switches the pruning off (dsg_get_option reports what runs).
 * dsg_debug_need_lists copies the lists that the flags last staged for batch B produced to HOST buffers: *n_roles rows of
 * roles [max_roles][8] = {kind (0: list of runs = 8 consecutive token rows, entry b * res * res / 8 + run; 1: list of windows, entry
 * b * nW + window), res, shift, up stage, block (>= 0: a Swin block's proj / MLP rows resp. attention windows; -1: the stage's post_linear
 * rows; -2: its pre_linear / breakup rows, on the coarser grid), count, offset of the entries in lists_out, entries when nothing is
 * masked}.  roles == NULL only returns *n_roles (0 when the configuration is not covered). */
int dsg_debug_need_lists(dsg_handle h, int32_t B, int32_t *roles, int32_t max_roles, int32_t *n_roles, int32_t *lists_out,
                         int64_t lists_cap, void *stream);
/* Pure-window deduplication (option "dedup_masked", default 1).  An 8 x 8 window of the finest level is pure when each of its tokens
 * (i, j) has a padded endpoint.  In the sampler every input of the network is zero at such tokens (the loop's own kernels store the
 * zeros), so all pure windows of a graph leave PatchEmbed and the first, unshifted Swin block with the same 64 rows: one representative
 * per graph is computed, the others are filled by a copy before PatchMerging reads them.  dsg_denoise / dsg_precond take caller
 * tensors and compute every window.  Off wherever "prune_masked" is, and unless PatchEmbed and that block run the fused C = 96 kernels.
 * dsg_debug_dedup_lists copies what the flags last staged for batch B produced to HOST buffers (any but counts may be NULL): counts [4] =
 * entries of wins / runs / copy (-1 each: the configuration has no such lists) and what the batch size's last forward did (-1: it did not
 * deduplicate; 0: the copy moved activation rows; 1: also their LayerNorm partials, which the fused PatchMerging reads); wins (capacity B * nW): unique windows b * nW + w -- every
 * non-pure window and the representative; runs (B * N * N / 8): the same set as 8-token runs; copy (B * nW): the pure windows filled
 * by copy; rep [B]: each graph's representative window b * nW + w, -1 where the graph has no pure window (or the call deduplicates
 * nothing).  What is reported is what was staged: under "dedup_batch" (a sampler call with one
 * representative for the batch) rep holds the same global id b' * nW + w for every graph -- a window of whichever graph b' comes first
 * with a pure window -- wins / runs hold every non-pure window plus that one, and copy holds the pure windows that are filled: all
 * others at the top level of the chain, below it only those under a unique window of the next level.  Under "dedup_table" the same
 * is reported -- rep names the window whose rows come from the table -- although no launch computes that window and the fill writes
 * it: dsg_debug_dedup_launch_lists below reports the lists as the launches iterate them. */
int dsg_debug_dedup_lists(dsg_handle h, int32_t B, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy, int32_t *rep, void *stream);
/* The same for level `level` of the down path (0: exactly dsg_debug_dedup_lists).  A window of level k has 8 x 8 tokens of the grid of
 * res = N >> k tokens per side and covers 8 << k nodes per side; it is pure when no valid pair lies under it (no valid node in its row
 * block, or none in its column block).  wins (capacity B * nW, nW = (res / 8)^2): unique windows b * nW + w; runs (B * res * res / 8): the
 * same set as 8-token runs b * res * res / 8 + i * res / 8 + jr -- the rows PatchMerging into the level and the level's first block
 * compute; copy (B * nW): the pure windows filled by copy; rep [B]: the representatives.  counts [3]: what the batch size's last forward
 * did at that level (-1: no deduplication there; 0: the copy moved rows of the activation and of the skip tensor; 1: also the rows'
 * (sum, sumsq) partials, which the next block or the next PatchMerging reads).  counts [0..2] = -1: the plan has no lists for the level. */
int dsg_debug_dedup_level_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy,
                                int32_t *rep, void *stream);
/* The lists of level `level` as the launches iterate them (same capacities): wins / runs -- what PatchEmbed or the merge into the level
 * and the level's first block compute; copy -- the windows the fill writes.  counts [3]: how the lists were written -- 0 every window
 * unique (dsg_denoise / dsg_precond), 1 one representative per graph, 2 one for the batch, 3 one for the batch, taken from the
 * sampler's table ("dedup_table"): wins / runs then hold the non-pure windows only and copy also holds the window that
 * dsg_debug_dedup_level_lists reports as rep.  For 0 .. 2 the lists are those of dsg_debug_dedup_level_lists. */
int dsg_debug_dedup_launch_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy,
                                 void *stream);
/* Option "dedup_qkv": the lists of level `level`'s second, shifted block as the flags last staged for batch B left them.  runs: the 8-row
 * runs whose q, k, v the split form projects (every non-pure window, plus one source pure window per content class: of the batch where it
 * shares a representative, of each graph otherwise; every window under mode 0).  src [B nW]: for every window b nW + w of the level the
 * window whose rows of the QKV tensor hold its q, k, v (itself when listed).  counts[0] = entries of runs, counts[1] = entries of src,
 * counts[2] = 1 where the device's rule picks the split form for these lists (dsg_debug_qk_split(counts[0], B res^2)), counts[3] = the
 * form the batch size's last forward took at that block: 1 split (the rule, or "dedup_qkv" 2: whatever the share), 0 fused, -1 the block ran without the switch (option off, another
 * kernel path, or the level not deduplicated).  All -1: the plan has no such lists for the level. */
int dsg_debug_dedup_qkv_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *runs, int32_t *src, void *stream);
/* The fused read-out (E = 96) under "prune_masked": it takes the list of its 32-token tiles that hold a valid pair (written with the need
 * lists wherever the flags are staged) and computes them four to a block at the front of its grid; every wave still writes the exact zeros
 * of its own positional tile where that tile holds no valid pair, so each tile is written once and the grid does not depend on the flags.
 * Where the pruning does not run, every wave decides on its positional tile alone.  Bit-identical results either way.
 * This call: the working tiles as the flags last staged for batch B left them.  tiles (room for B N N / 32):
 * ascending ids t of the 32-token tiles [32 t, 32 t + 32) of the flattened [B N N] token index in which some (b, i, j) has
 * flag_i && flag_j.  counts[0] = entries of tiles, counts[1] = the form the batch size's last forward's read-out took: 1 list,
 * 0 positional, -1 no fused read-out yet.  Both -1: the plan has no such list (N % 8 != 0, 10 x 10 windows, or no room for it).
 * The list is not among the records of dsg_debug_need_lists. */
int dsg_debug_readout_tiles(dsg_handle h, int32_t B, int32_t *counts, int32_t *tiles, void *stream);
/* The route the batch size's last forward took through PatchEmbed (forms[0]) and the read-out (forms[1]): 1 the fused kernel
 * (fused_patch_embed96 / fused_readout96, at patch_size 2 their _p2 forms), 0 the chain of assembly, GEMMs and row passes, -1 no
 * forward yet.  The fused forms exist for E = 96 at patch_size 1 and 2 (in_chans <= 64, C_adj <= 32) and follow "fused_patch_embed" /
 * "fused_readout"; debug taps take the read-out's chain; patch_size 4 always runs the chain.  Host only. */
int dsg_debug_patch_forms(dsg_handle h, int32_t B, int32_t forms[2]);

/* Measurement: runs n_iters eager network forwards on the batch-B workspace (whatever inputs the last call left
 * there) with HIP events bracketing every kernel launch on `stream`, and accumulates per kernel class
 * (0 = MFMA GEMM, 1 = window attention, 2 = row kernels (LayerNorm/modulate/heads), 3 = elementwise, 4 = fused
 * narrow-level blocks (attention / MLP / read-out / patch-embed)):
 * total milliseconds, number of launches, algorithmic FLOPs (2*M*N*K; 4*T*W*C for attention).  Arrays of length 5.
 * An event bracket around a single launch includes ~10-15 us of dispatch latency that back-to-back (graph) launches do
 * not pay, so for the dominant kernel (class 0) the kernel also stamps first-block-start / last-block-end on the GPU's
 * 100 MHz constant clock: *gemm_inkernel_ms receives the sum of those in-kernel durations (agrees with rocprofv3). */
int dsg_profile_forward(dsg_handle h, int32_t B, int32_t n_iters, double *ms_by_kind, int64_t *launches_by_kind,
                        double *flops_by_kind, double *gemm_inkernel_ms, void *stream);

/* The shader clock the chip held during the GEMM launches of the last dsg_profile_forward call, in GHz: median over the launches of
 * (block 0's lifetime in s_memtime shader cycles) / (the same lifetime in 100 MHz s_memrealtime ticks).  Dense f32-MFMA streams are
 * power-limited on MI355X: the clock-limited ceiling of a perfect kernel is this clock x 1024 SIMDs x 64 FLOP/clk, not 157.3 TFLOP/s. */
double dsg_profile_clock_ghz(dsg_handle h);

/* ======== the fp32 forward's kernels on their own ======== */

/* The default fp32 path's kernels on their own (test hooks, csrc/kernels.hip; device pointers, synchronise `stream`; DSG_ERR_INVALID
 * when the launcher does not build the form, never an abort).  tests/test_f32_kernels.py compares every output element with float64.
 * dsg_debug_gemm_f32: one launch of the fp32 GEMM in any form its launcher admits.  The struct mirrors the fp32 fields of the
 *   launcher's argument block: C[M,N] = act(LN?(A | A2)[M,K] . W[N,K]^T + bias) (+ res), leading dimensions in floats.
 *     A2 / lda2 / K1   second source for k >= K1 (concat along K); NULL: K1 is ignored
 *     ln_stats [M,2] (mean, rstd) or ln_part [M][ln_nparts][2] (sum, sumsq per 96 columns): LayerNorm without affine on the way in
 *     act              0 none, 1 GELU, 2 SiLU, 3 GELU with the pre-activation kept in C2, 4 product * GELU'(res)
 *     C2 / ldc2        second store (with mod_aff: the value before the modulation)
 *     stats_out        [M][ceil(N/96)][2] (sum, sumsq) of what was stored to C, per column tile
 *     mod_aff          silu(shift + v (1 + scale)) on the value stored to C, (scale, shift) = mod_aff[b mod_ld + mod_off + {n, N + n}],
 *                      b = row / mod_T (mod_ld == 0: one row for the whole batch); needs stats_out
 *     a4_res > 0       PatchMerging gather: A is the fine activation [B a4_res^2, K/4], M = B (a4_res/2)^2, ln_part per fine row
 *     row_list/row_cnt only the 8-row runs listed (device int32, -1 pads to a multiple of 16), *row_cnt of them (device)
 *     reserved         form of a list launch: 0 the kernel's own rule (dsg_debug_gemm_form with the device's CU count), 1 the wide form
 *                      (128-row tiles), 2 the thin form (64-row tiles; same bits).  2 without a list, or for a form that has no thin
 *                      kernel (LayerNorm on the way in), is DSG_ERR_INVALID. */
typedef struct dsg_gemm_f32_args {
    const float *A, *A2, *W, *bias, *ln_stats, *ln_part, *res;
    float *C, *C2;
    const float *mod_aff;
    float *stats_out;
    const int32_t *row_list, *row_cnt;
    int32_t lda, lda2, K1, ln_nparts, ldres, ldc, ldc2, M, N, K, act, mod_ld, mod_off, mod_T, a4_res, reserved;
} dsg_gemm_f32_args;
int dsg_debug_gemm_f32(const dsg_gemm_f32_args *args, void *stream);
/* The list GEMM's form rule, from the function its kernel evaluates on the device-side count: 2 (thin) iff the wide form's
 * ceil(cnt_runs / 16) x ceil(N / 96) tiles would occupy at most half of n_cu compute units, else 1 (wide); n_cu = 0: always 1.  Host only. */
int32_t dsg_debug_gemm_form(int32_t cnt_runs, int32_t N, int32_t n_cu);
/* LayerNorm-1 -> QKV -> window attention in the GEMM's epilogue (8 x 8 and 10 x 10 windows): x [B res^2, K], W [3C, K] (C = 32 heads,
 * q rows pre-scaled by d^-1/2 log2 e), bias [3C], one of ln_stats / ln_part, attn_bias the key-major log2(e)-scaled table
 * [nW | 1][heads][Wp][Wp] (-1e30 in padded key slots); win_list / win_cnt (device, 8 x 8 only): only those windows (b nW + w, -1: none)
 * -> out [B res^2, C]. */
int dsg_debug_qkv_attn_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, int32_t K, const float *x, const float *W,
                           const float *bias, const float *ln_stats, const float *ln_part, int32_t ln_nparts, const float *attn_bias,
                           const int32_t *win_list, const int32_t *win_cnt, float *out, void *stream);
/* window attention, fp32 in and out: qkv [B res^2, 3C] (q pre-scaled), biasT as attn_bias above -> out [B res^2, C] */
int dsg_debug_window_attn_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *biasT,
                              float *out, void *stream);
/* x [M,C] <- x + fc2(GELU(fc1(LN(x)))) in place, C in {96, 192}; W1p / W2p ALREADY in the kernel's fragment order (the index formulas
 * above pack_mlp_weights in csrc/dsg_api.cpp); stats_out [M][2] (sum, sumsq) of the rows written, or NULL; run_list / run_cnt as
 * dsg_gemm_f32_args::row_list (-1 pads to a multiple of 4 at least). */
int dsg_debug_fused_mlp_f32(int32_t M, int32_t C, float *x, const float *gam, const float *bet, const float *W1p, const float *b1,
                            const float *W2p, const float *b2, float *stats_out, const int32_t *run_list, const int32_t *run_cnt,
                            void *stream);
/* the attention half of a C = 96 block in place: x [B res^2, 96] <- x' + proj(window_attention(LN(x'))), x' = premod ? x :
 * silu(shift + x (1 + scale)), (scale | shift) = aff[b aff_ld + aff_off + ...] (aff must be a valid table with premod too; aff_ld and
 * aff_off multiples of 4); windows of at most 64 tokens; Wqp / Wpp ALREADY in
 * fragment order and bqkv with its q part scaled (pack_attn_weights); biasT [nW | 1][3][Wp][Wp]; win_list / win_cnt: only those windows. */
int dsg_debug_fused_attn96_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, float *x, const float *aff, int32_t aff_ld,
                               int32_t aff_off, const float *gam, const float *bet, const float *Wqp, const float *bqkv, const float *biasT,
                               const float *Wpp, const float *bproj, int32_t premod, const int32_t *win_list, const int32_t *win_cnt,
                               void *stream);

/* The fp32 forward's edge and row kernels on their own (test hooks, csrc/kernels.hip; same rules as above; fp32 forms only: no bf16
 * read-out fragments, no bf16 outputs).  tests/test_edge_kernels.py compares every output element with float64.
 * dsg_debug_patch_embed_f32: the fused PatchEmbed (E = 96): input assembly [sc_adj, adj, sc_node(i), node(i), sc_node(j), node(j)] ->
 *   Wp . in + bias -> LayerNorm_96(gam, bet) -> silu(shift + n (1 + scale)), (scale | shift) = aff[b aff_ld + aff_off + ...], and once more
 *   with the row at aff_off2 when aff_off2 >= 0 -> x [B N^2, 96].  Wp: patch_embed.proj.weight zero-padded to [96, Kp] ALREADY in fragment
 *   order (the pe_wp loop of dsg_finalize_weights); Kp 32 or 64; aff_ld and the offsets multiples of 4.  sc_adj / sc_node may be NULL;
 *   has_sc (device int32) NULL: they are used when given; *has_sc == 0: they are not read.  run_list / run_cnt (device): only those runs
 *   of 8 tokens (N % 8 == 0; -1 pads to a multiple of 4 at least).
 * dsg_debug_assemble_f32: the same gathered input on its own, token-major [B N^2, Kp], zero-padded. */
int dsg_debug_patch_embed_f32(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj,
                              const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                              const float *Wp, const float *bias, const float *gam, const float *bet, const float *aff, int32_t aff_ld,
                              int32_t aff_off, int32_t aff_off2, float *x, const int32_t *run_list, const int32_t *run_cnt, void *stream);
int dsg_debug_assemble_f32(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj, const float *node,
                           const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags, float *out, void *stream);
/* the fused read-out (E = 96, c_adj <= 32): x [B N^2, 96] -> out_adj [B, c_adj, N, N] = valid (F2 gelu(Fa LN(x) + fa) + f2), and the pooling
 * pool_ext [B N, 128] = ((1/N) sum_j valid LN(x) | f_i (#valid) / N | 0 ..).  Wfp / W2p: the folded Fa [96, 96] and F2 zero-padded to
 * [32, 96] ALREADY in fragment order (the fap / f2p loops of dsg_finalize_weights); pool_part: scratch [B N][(N + 30) / 32 + 1][96].
 * Rows of x of tokens with !(f_i && f_j) are not read into the result. */
int dsg_debug_readout_f32(int32_t B, int32_t N, int32_t c_adj, const float *x, const float *gam, const float *bet, const float *Wfp, const float *fa,
                          const float *W2p, const float *f2, const uint8_t *flags, float *out_adj, float *pool_part, float *pool_ext, void *stream);
/* the unfused read-out tails.  DSG_HEAD_ADJ: h [B N^2, E] -> out [B, c_out, N, N] = valid (h W^T + bias); DSG_HEAD_POOL: h [B N^2, E] -> out
 * [B N, E] = (1/N) sum_j valid h (W, bias, c_out unused); DSG_HEAD_NODE: h [B N, E] -> out [B, N, c_out] = f_i (h W^T + bias). */
enum { DSG_HEAD_ADJ = 0, DSG_HEAD_POOL = 1, DSG_HEAD_NODE = 2 };
int dsg_debug_head_f32(int32_t kind, int32_t B, int32_t N, int32_t E, int32_t c_out, const float *h, const float *W, const float *bias,
                       const uint8_t *flags, float *out, void *stream);
/* The edge kernels of the patch_size p > 1 forward on their own (csrc/kernels_patch.hip; p in {1, 2, 4} here, N % p == 0, R = N / p).
 * Token t = ti R + tj covers the pixels (p ti + a, p tj + b); rows "in (token, a, b) order" are m = (b_graph R^2 + t) p^2 + a p + b.
 * dsg_debug_assemble_patch_f32: out [B R^2, Kp], column (a p + b) Cin + c = channel c (dsg_debug_assemble_f32's order) of the token's
 *   pixel (a, b), zero from p^2 Cin up to Kp; the node channels are selected by the PIXEL's flag_I && flag_J.
 * dsg_debug_head_patch_f32: DSG_HEAD_ADJ: h [B N^2, E] in (token, a, b) order -> out [B, c_out, N, N] = valid(I, J) ? h W^T + bias : 0;
 *   DSG_HEAD_POOL: h likewise -> out [B N, E] = (1/N) sum_J valid(I, J) h[row(I, J)] (W, bias, c_out unused).  Rows of h at pixels
 *   that are not valid are not read into a result. */
int dsg_debug_assemble_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj,
                                 const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                                 float *out, void *stream);
int dsg_debug_head_patch_f32(int32_t kind, int32_t B, int32_t N, int32_t p, int32_t E, int32_t c_out, const float *h, const float *W,
                             const float *bias, const uint8_t *flags, float *out, void *stream);
/* The fused forms for E = 96, p = 2 (any other p: DSG_ERR_INVALID), weights ALREADY packed as dsg_finalize_weights packs them.
 * dsg_debug_patch_embed_patch_f32: dsg_debug_patch_embed_f32 on the R x R token grid: the four sub-pixel gathers accumulate into one set of
 *   accumulators; Wp [4][3][Kps / 8][64][4]: for sub-pixel sub = 2 a + b the fragment order of dsg_debug_patch_embed_f32 applied to
 *   patch_embed.proj.weight[:, :, a, b] zero-padded to [96, Kps], Kps = 32 | 64 >= in_chans -> x [B R^2, 96].  No run list.
 * dsg_debug_readout_patch_f32: x [B R^2, 96] -> out_adj [B, c_adj, N, N] = valid(I, J) (F2 gelu(Fa[a, b] LN(x)[t] + fa) + f2) and the pooling
 *   pool_ext [B N, 256], row (b, I = 2 ti + a) = (s[ti, 0] | s[ti, 1] | f_I cnt_0 / N | f_I cnt_1 / N | 0 ..) with
 *   s[ti, q] = (1/N) sum_tj f_{2 tj + q} LN(x)[ti, tj] and cnt_q the valid pixel columns of parity q.  Wfp [4][3][12][64][4]: the folded
 *   Fa[a, b] [96, 96] per sub-pixel in dsg_debug_readout_f32's fragment order; fa, W2p, f2 as there; pool_part: scratch
 *   [B R][(R + 30) / 32 + 1][2][96].  Rows of x of tokens without a valid pixel are not read into a result. */
int dsg_debug_patch_embed_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kps, const float *adj,
                                    const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                                    const float *Wp, const float *bias, const float *gam, const float *bet, const float *aff, int32_t aff_ld,
                                    int32_t aff_off, int32_t aff_off2, float *x, void *stream);
int dsg_debug_readout_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, const float *x, const float *gam, const float *bet, const float *Wfp,
                                const float *fa, const float *W2p, const float *f2, const uint8_t *flags, float *out_adj, float *pool_part,
                                float *pool_ext, void *stream);
/* the one-wave-per-row passes; rows of at most 1536 channels, C % 4 == 0; unused pointers NULL.
 *   DSG_ROW_MOD_STATS        x [B t, C] <- silu(shift + x (1 + scale)) in place, stats [B t, 2] = (mean, rstd) of the new row
 *   DSG_ROW_LN_STATS         stats [B t, 2] = (mean, rstd) of x's rows
 *   DSG_ROW_LN_MOD           y = silu(shift + LN(x; g, b) (1 + scale))
 *   DSG_ROW_MERGE_LN         t = fine side: y [B (t/2)^2, 4C] = LN_4C(cat[x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)]; g, b); 4C <= 1536
 *   DSG_ROW_BREAKUP_LN       t = coarse side, C = D: LN_D(x row; g, b), chunk q -> token (2i + (q & 1), 2j + (q >> 1)) of y [B (2t)^2, D/4],
 *                            LN_{D/4}(pg, pb); run_list / run_cnt: only those runs of 8 coarse rows (-1: none)
 *   DSG_ROW_MERGE_NORM_RUNS  t = fine side (t % 16 == 0): the merged rows of the listed runs, y = x rstd - mean rstd with the statistics
 *                            from the four fine rows' ln_part [B t^2][nparts][2]; run_list / run_cnt required
 * (scale | shift) = aff[b aff_ld + aff_off + ...], b = row / t. */
enum { DSG_ROW_MOD_STATS = 0, DSG_ROW_LN_STATS = 1, DSG_ROW_LN_MOD = 2, DSG_ROW_MERGE_LN = 3, DSG_ROW_BREAKUP_LN = 4, DSG_ROW_MERGE_NORM_RUNS = 5 };
int dsg_debug_row_f32(int32_t kind, int32_t B, int32_t t, int32_t C, float *x, const float *g, const float *b, const float *pg, const float *pb,
                      const float *aff, int32_t aff_ld, int32_t aff_off, const float *ln_part, int32_t nparts, float *y, float *stats,
                      const int32_t *run_list, const int32_t *run_cnt, void *stream);
/* the pure-window copies.  Broadcast: every window of copy_list (device, *copy_cnt entries, b nW + w) of x [B res^2, C], skip (or NULL) and
 * stats [B res^2][nparts][2] (or NULL) is filled from window rep[b] (device [B], a global window id; -1: none), or, when mode == 3 (the
 * table mode) from table entry sched[min(step, n_steps - 1)] (clamped to tab_entries - 1): an entry is tab_stride floats with 64 x C rows
 * of x at off_x, of the skip at off_skip and 64 x nparts pairs at off_st, tokens in window order.  tab_base NULL: no table.  sched is a
 * HOST array of n_steps schedule indices; the call builds the device records the kernel reads and frees them before it returns.
 * Harvest: window 0 of each of the first n graphs -> entry g of dst in that layout. */
int dsg_debug_window_broadcast_f32(int32_t B, int32_t res, int32_t C, float *x, float *skip, float *stats, int32_t nparts, const int32_t *copy_list,
                                   const int32_t *copy_cnt, const int32_t *rep, const float *tab_base, int32_t tab_entries, int64_t tab_stride,
                                   int32_t off_x, int32_t off_skip, int32_t off_st, int32_t mode, int32_t step, int32_t n_steps,
                                   const int32_t *sched, void *stream);
int dsg_debug_window_harvest_f32(int32_t n, int32_t res, int32_t C, const float *x, const float *skip, const float *stats, int32_t nparts, float *dst,
                                 int64_t stride, int32_t off_x, int32_t off_skip, int32_t off_st, void *stream);
/* The rule of that switch, from the function the kernels evaluate on the device-side count: 1 (split) iff listed_runs > 0 and the listed
 * rows, 8 per run, are at most half of the M rows.  Host only. */
int32_t dsg_debug_qk_split(int32_t listed_runs, int32_t M);

/* ======== the bf16 / split-bf16 GEMMs and the bf16-tensor row passes ======== */

/* Debug / verification: one GEMM of the library, C[M,N] = act(LN?(A)[M,K] . W[N,K]^T + bias) (+ res), in a chosen arithmetic
 * (mode 0: fp32 MFMA; 1: bf16 operands, fp32 accumulate -- "gemm_bf16"; 2: three-way split bf16 -- "gemm_split"); act 0 none,
 * 1 GELU, 2 SiLU; ln_stats [M,2] (mean, rstd) or NULL.  Device pointers, K % 32 == 0, synchronises `stream`.  Lets a test diff
 * WHOLE output matrices between the arithmetic modes (a rare wrong 16-lane group is invisible to sampled checks). */
int dsg_debug_gemm(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias, const float *ln_stats,
                   const float *res, int32_t act, int32_t mode, float *C, void *stream);

/* The two bf16-MFMA GEMMs on their own (test hooks, csrc/kernels_lp.hip: gemm_bf16_kernel and gemm_split2_kernel; tests/test_lp_kernels.py
 * compares every output element with float64).  dsg_debug_gemm_lp: one launch through launch_gemm_lp DIRECTLY -- a form that launcher
 * refuses is DSG_ERR_INVALID with nothing launched and no output written; there is no fall-back to the fp32 kernel (launch_gemm, and so
 * dsg_debug_gemm, does fall back).  The fields of dsg_gemm_f32_args -- row_list / row_cnt must be NULL and reserved 0: these kernels take
 * no list -- and
 *     mode       1 bf16 operands ("gemm_bf16"), 2 three-way split ("gemm_split"); W is given as fp32 [N,K] and converted inside
 *                (dsg_debug_convert kind 0 / 1), as dsg_debug_gemm does
 *     tile       bf16 kernel only: 0 the launcher's rule, 1 the 128-row tile (K step 64), 2 the 256-row tile (K step 32; needs M >= 256)
 *     a_bf16     A is a bf16 tensor [M, lda], lda in elements and a multiple of 8
 *     c_bf16     C is a bf16 tensor [M, ldc], ldc in elements
 *     tile_used  host int32 or NULL: the block rows of the kernel launched (128 or 256; 0 when refused)
 * fp32 leading dimensions are multiples of 4 floats; K % 32 == 0. */
typedef struct dsg_gemm_lp_args {
    const void *A;
    const float *A2, *W, *bias, *ln_stats, *ln_part, *res;
    void *C;
    float *C2;
    const float *mod_aff;
    float *stats_out;
    const int32_t *row_list, *row_cnt;
    int32_t *tile_used;
    int32_t lda, lda2, K1, ln_nparts, ldres, ldc, ldc2, M, N, K, act, mod_ld, mod_off, mod_T, a4_res, reserved;
    int32_t mode, tile, a_bf16, c_bf16;
} dsg_gemm_lp_args;
int dsg_debug_gemm_lp(const dsg_gemm_lp_args *args, void *stream);
/* The conversion kernels of that file on n elements (device pointers, n in [1, 2^31)): kind 0 fp32 -> bf16 [n], round to nearest even
 * on the integer pipe: bits + 0x7fff + (bit 16), upper half.  Finite values and infinities round as IEEE does (the largest finite
 * values go to inf); a NaN is NOT special-cased: the quiet NaN 0x7fc00000 stays 0x7fc0, but a payload whose upper mantissa bits are all
 * ones carries into the exponent and sign (0x7fff8000 and above -> 0x8000, i.e. -0).  kind 1 fp32 -> three bf16 planes [3][n]
 * (hi | mid | lo, by truncation: hi + mid + lo == the input exactly for 0 and for |x| >= 2^-110; below that, bits under 2^-133, the last
 * bit of a bf16 denormal, are cut; an infinity gives hi = itself and NaN in the other planes).  kind 2 bf16 [n] -> fp32 (exact). */
int dsg_debug_convert(int32_t kind, const void *src, void *dst, int64_t n, void *stream);
/* The bf16-tensor forms of the row passes ("gemm_bf16" mode; tests/test_lp_kernels.py).  y is a bf16 tensor, rounded to nearest even
 * from the fp32 value; x, the parameters and all arithmetic stay fp32.
 *   DSG_ROWLP_MERGE_LN    as DSG_ROW_MERGE_LN, y bf16 [B (t/2)^2, 4C]
 *   DSG_ROWLP_BREAKUP_LN  as DSG_ROW_BREAKUP_LN, y bf16 [B (2t)^2, D/4]; the input row x stays fp32
 *   DSG_ROWLP_LN_BX       x [B t, C] <- silu(shift + x (1 + scale)) in place when aff != NULL (aff_ld == 0: one (scale | shift) row for
 *                         the whole batch), then y bf16 [B t, C] = LayerNorm of the row without affine
 *   DSG_ROWLP_COPY_BX     the same with y = the plain bf16 copy of the (modulated) row */
enum { DSG_ROWLP_MERGE_LN = 0, DSG_ROWLP_BREAKUP_LN = 1, DSG_ROWLP_LN_BX = 2, DSG_ROWLP_COPY_BX = 3 };
int dsg_debug_row_lp(int32_t kind, int32_t B, int32_t t, int32_t C, float *x, const float *g, const float *b, const float *pg, const float *pb,
                     const float *aff, int32_t aff_ld, int32_t aff_off, void *y, const int32_t *run_list, const int32_t *run_cnt, void *stream);
/* window attention as dsg_debug_window_attn_f32 with out (out_bf16) or qkv and out (in_bf16 and out_bf16) as bf16 tensors; bf16 qkv is
 * widened on load and the arithmetic is unchanged.  in_bf16 without out_bf16 is not built: DSG_ERR_INVALID. */
int dsg_debug_window_attn_lp(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const void *qkv, const float *biasT, void *out,
                             int32_t in_bf16, int32_t out_bf16, void *stream);

/* ======== the bf16 block pipeline ======== */

/* The bf16 block pipeline's kernels on their own (test hooks, csrc/kernels_bx.hip; device pointers, synchronise `stream`).
 * dsg_debug_gemm_bx: A [M,K], W [N,K] given as fp32 and rounded to bf16 inside; epilogue pieces as in the forward: bias [N], fp32
 *   residual res [M,N], act (0 | 1 GELU), mod = (scale [N] | shift [N]) of a batch-uniform modulate+SiLU, ln_out (LayerNorm of the
 *   stored row into out_Cb; N in {96,192,384}).  out_C [M,N] fp32 store; out_Cb / out_C2b [M,N]: the bf16 stores widened to fp32
 *   (any may be NULL, not both of out_C / out_Cb).  DSG_ERR_INVALID when the shape is not covered.
 * dsg_debug_attn_bx: window attention on qkv [B*res*res, 3*32*heads] (rounded to bf16 inside; q pre-scaled) with the key-major
 *   log2(e)-scaled bias table [nW|1][heads][Wp][Wp] -> out [B*res*res, 32*heads] (the bf16 result widened).
 * time_iters > 0 with out_ms (host): also the mean HIP-event time of that many back-to-back launches of the kernel (tools/bx_bench.py). */
int dsg_debug_gemm_bx(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias, const float *res, int32_t act,
                      const float *mod, int32_t ln_out, float *out_C, float *out_Cb, float *out_C2b, int32_t time_iters, float *out_ms,
                      void *stream);
int dsg_debug_attn_bx(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *biasT, float *out,
                      int32_t time_iters, float *out_ms, void *stream);
/* Which kernel the three hooks below run where the launcher has more than one for the shape (`kernel`).  DSG_BXK_DEFAULT: what the
 * forward's default options run there -- the first name of each line below.  A name the hook cannot honour for the given shape (another
 * width, another window, a hook that has no such kernel, the LDS-resident kernel with a modulate) is DSG_ERR_INVALID.
 *   C = 384, dsg_debug_mlp_bx and dsg_debug_projmlp_bx:  DSG_BXK_MLP384_DMA   eight waves, pre-arranged weight images streamed by LDS-DMA
 *                                                        DSG_BXK_MLP384_WAVE  the one-wave-per-SIMD kernel of the narrower widths
 *                                                                             (dsg_debug_mlp_bx only)
 *                                                        DSG_BXK_MLP384_R3    round 3's eight-wave kernel, register-staged weights
 *                                                        DSG_BXK_MLP384_SOLO  four waves solo on a chunk-major LDS-DMA ring (mlp384s_bx_kernel)
 *   C = 96, dsg_debug_projmlp_bx:                        DSG_BXK_MLP96_STAGED   the staged kernel
 *                                                        DSG_BXK_MLP96_RESIDENT the LDS-resident persistent kernel (mlp96r_bx_kernel); mod == NULL
 *   10 x 10 windows, dsg_debug_qkv_attn_bx:              DSG_BXK_QA10_WAVE    one wave per (window, head)
 *                                                        DSG_BXK_QA10_HEAD    the block-per-head kernel of the other window sizes */
enum { DSG_BXK_DEFAULT = 0, DSG_BXK_MLP384_DMA = 1, DSG_BXK_MLP384_WAVE = 2, DSG_BXK_MLP384_R3 = 3, DSG_BXK_MLP384_SOLO = 4,
       DSG_BXK_MLP96_STAGED = 5, DSG_BXK_MLP96_RESIDENT = 6, DSG_BXK_QA10_WAVE = 7, DSG_BXK_QA10_HEAD = 8 };
/* the fused QKV projection + window attention kernel on caller-provided operands: xn [B*res*res, C] (C = 32 heads), W [3C, C] (q rows
 * pre-scaled by d^-1/2 log2 e), bias [3C], biasT as above; operands are rounded to bf16 on the way in, out is the bf16 result as fp32.
 * kernel: DSG_BXK_DEFAULT or, at ws == 10, DSG_BXK_QA10_*. */
int dsg_debug_qkv_attn_bx(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *xn, const float *W, const float *bias,
                          const float *biasT, float *out, int32_t kernel, int32_t time_iters, float *out_ms, void *stream);
/* the fused MLP kernel with the attention half's tail in front: x <- [modulate] (x1 + fc2(GELU(fc1(LN(x1))))), x1 = x + att Wp^T + bp;
 * att [M, C], Wp [C, C], W1 [4C, C], W2 [C, 4C] are rounded to bf16 on the way in; x [M, C] fp32 in place; out_mode / out_xn as
 * dsg_debug_mlp_bx.  kernel: DSG_BXK_DEFAULT, at C == 384 DSG_BXK_MLP384_DMA / _R3 / _SOLO, at C == 96 DSG_BXK_MLP96_*. */
int dsg_debug_projmlp_bx(int32_t M, int32_t C, const float *att, float *x, const float *Wp, const float *bp, const float *W1, const float *b1,
                         const float *W2, const float *b2, const float *mod, int32_t out_mode, float *out_xn, int32_t kernel,
                         int32_t time_iters, float *out_ms, void *stream);
/* dsg_debug_mlp_bx: the fused MLP half of a block, x [M,C] <- [modulate] (x + fc2(GELU(fc1(xn)))) in place, with xn [M,C], W1 [4C,C],
 *   W2 [C,4C] given as fp32 and rounded to bf16 inside; mod = (scale [C] | shift [C]) or NULL; out_mode 0 none, 1 LayerNorm of the
 *   stored row, 2 its plain copy -> out_xn [M,C] (the bf16 store widened).  C in {96, 192, 384}.
 *   kernel: DSG_BXK_DEFAULT or, at C == 384, DSG_BXK_MLP384_*. */
int dsg_debug_mlp_bx(int32_t M, int32_t C, const float *xn, float *x, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *mod, int32_t out_mode, float *out_xn, int32_t kernel, int32_t time_iters, float *out_ms, void *stream);

/* The same GEMM and fused-MLP kernels on the caller's OWN tensors (tests/test_bx_forms.py): bf16 tensors are taken as they are, nothing is
 * converted, no scratch sits between the caller and the kernel, and only what the kernel writes is written.  A form the launcher
 * refuses is DSG_ERR_INVALID with nothing launched and nothing written.
 * dsg_debug_gemm_bx_args: launch_gemm_bx on a BxGemm filled field by field.  A [M, lda], A2 [M, lda2] (second source for k >= K1; NULL:
 *   K1 is ignored), W [N, K] bf16; bias [N], res [M, ldres] fp32; C [M, ldc] fp32 (may alias res), Cb [M, ldcb] and C2b [M, ldc2b] bf16
 *   (C2b: the value before the modulate); leading dimensions in elements.  act 0 | 1 GELU.  mod_aff: silu(shift + v (1 + scale)),
 *   (scale, shift) = mod_aff[b mod_ld + mod_off + {n, N + n}], b = row / mod_T; mod_ld == 0: one row for the batch (staged in LDS),
 *   mod_ld > 0: per sample, read in the epilogue; mod_ld and mod_off multiples of 4.  ln_out: Cb = LayerNorm of the stored row.
 *   What the kernel takes on trust from the forward is checked here (DSG_ERR_INVALID): pitches that hold a row, fp32 pitches and the
 *   (scale | shift) offsets in multiples of 4, mod_T >= 1, a per-sample row pitch that holds mod_off + 2N.
 *   geo_used (HOST, may be NULL): the tile geometry launched -- 0 128 x 192 (k chunk 64), 2 256 x 96 (k chunk 32), 3 128 x 384
 *   (k chunk 64) -- or -1 when refused.
 * dsg_debug_mlp_bx_args: launch_mlp_bx.  Exactly one of xn / att (bf16 [M, C]); with att the proj stage (Wp [C, C] bf16, bp) rides in
 *   front.  x [M, C] fp32 in place; W1 [4C, C], W2 [C, 4C] bf16 row-major; xn_out bf16 [M, C] with out_mode 1 (LayerNorm of the stored
 *   row) or 2 (its copy); mod_* as above; kernel: DSG_BXK_* with the meaning and the refusals of dsg_debug_mlp_bx (xn) and
 *   dsg_debug_projmlp_bx (att).  The weight images of the kernels that stream pre-arranged weights are built inside. */
typedef struct dsg_bx_gemm_args {
    const void *A, *A2, *W;
    const float *bias, *res;
    float *C;
    void *Cb, *C2b;
    const float *mod_aff;
    int32_t *geo_used;
    int32_t lda, lda2, K1, ldres, ldc, ldcb, ldc2b, M, N, K, act, mod_ld, mod_off, mod_T, ln_out;
} dsg_bx_gemm_args;
int dsg_debug_gemm_bx_args(const dsg_bx_gemm_args *args, void *stream);
typedef struct dsg_bx_mlp_args {
    const void *xn, *att;
    float *x;
    const void *W1, *W2, *Wp;
    const float *b1, *b2, *bp;
    void *xn_out;
    const float *mod_aff;
    int32_t out_mode, mod_ld, mod_off, mod_T, M, C, kernel;
} dsg_bx_mlp_args;
int dsg_debug_mlp_bx_args(const dsg_bx_mlp_args *args, void *stream);

/* ======== the training kernels ======== */

/* The training kernels on their own (test hooks, csrc/train_kernels.hip; no handle, device pointers, synchronise `stream`;
 * DSG_ERR_INVALID where the launcher refuses the form, DSG_ERR_HIP on a HIP error, never an abort).  tests/test_train_kernels.py
 * compares every output element with float64.
 * dsg_debug_t_gemm: the training step's product launcher, C[M,N] (+)= op(A) op(B) (+ bias[n]); op(A)(m,k) = ta ? A[k lda + m] :
 *   A[m lda + k], op(B)(k,n) = tb ? B[n ldb + k] : B[k ldb + n].  a_colsum [M] (ta && !tb only): also sum_k A[k][m].  res: C = res +
 *   product (res has C's pitch).  act 0 none, 3 c2 = product + bias and C = GELU(c2), 4 C = product * GELU'(res).  force_plain != 0:
 *   the plain kernel only (what DSG_TRAIN_PLAIN_GEMM selects).  route_out (HOST, two values or NULL): [0] the path taken -- 1 the
 *   sampling path's MFMA GEMM, 2 the split-K weight-gradient MFMA kernel + reduction, 3 the plain kernel, 4 the plain kernel with
 *   split-K, 0 refused; [1] the number of K slices. */
int dsg_debug_t_gemm(int32_t ta, int32_t tb, const float *A, int32_t lda, const float *B, int32_t ldb, const float *bias, float *C, int32_t ldc,
                     int32_t M, int32_t N, int32_t K, int32_t accumulate, float *a_colsum, const float *res, int32_t act, float *c2,
                     int32_t force_plain, int32_t *route_out, void *stream);
/* dsg_debug_t_gemm_lp: ONE product in the bf16 mode of the training entries (dsg_train_set_precision; csrc/train_kernels_lp.hip), on
 *   caller buffers with dsg_debug_t_gemm's argument conventions: y = x W^T (ta 0, tb 1), dx = dy W (ta 0, tb 0; B [K, N] contiguous),
 *   dW = dy^T x (ta 1, tb 0).  The bf16 planes of B are built inside for the two activation-side forms.  any_rows != 0 waives the
 *   512-row threshold of the shape rule (the kernels take any row count; the channel rule stays).  route_out (HOST, two values or
 *   NULL): [0] 5 the bf16 GEMM on the weight plane, 6 gemm_tn_bf16_kernel + reduction, 0 not taken; [1] the number of K slices.
 *   A product the bf16 route does not take returns DSG_ERR_INVALID and writes nothing (it never falls back to fp32 here).
 * dsg_debug_t_cast_lp: W [R, Cc] contiguous fp32 -> out_nk [R, Cc] and out_kn [Cc, R] bf16 bit patterns (uint16; either may be NULL),
 *   the plane builder of that mode.
 * dsg_debug_train_routes (HOST out, rows of four int32: token rows, class 0 y / 1 dx / 2 dW, products on the bf16 route, products on
 *   an fp32 route): the covered products of the handle's LAST training entry, grouped by (rows, class); returns the number of groups
 *   (at most `cap` are written).  Products of call sites the mode does not cover are not listed; with the mode off the list is empty. */
int dsg_debug_t_gemm_lp(int32_t ta, int32_t tb, const float *A, int32_t lda, const float *B, int32_t ldb, const float *bias, float *C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, float *a_colsum, const float *res, int32_t act,
                        float *c2, int32_t any_rows, int32_t *route_out, void *stream);
int dsg_debug_t_cast_lp(const float *W, int32_t R, int32_t Cc, uint16_t *out_nk, uint16_t *out_kn, void *stream);
int32_t dsg_debug_train_routes(dsg_handle h, int32_t *out, int32_t cap);
/* window attention of the training block, forward (bwd == 0: qkv [B res^2, 3C], C = 32 heads, table [(2 ws - 1)^2, heads] -> out
 * [B res^2, C]) or backward (d_out [B res^2, C] -> d_qkv [B res^2, 3C] written, d_table ADDED to: the caller zeroes it).
 * S = q k^T / sqrt(32) + table[index][h] (- 100 where the shifted window's regions differ).  force_plain != 0: the scalar kernel. */
int dsg_debug_t_attn(int32_t bwd, int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *table,
                     float *out, const float *d_out, float *d_qkv, float *d_table, int32_t force_plain, void *stream);
/* LayerNorm with affine on x [M, C].  Forward (bwd == 0): y, stats [M][2] = (mean, rstd); with aff [ceil(M/T), 2C] = (scale | shift)
 * the row is modulated first, x' = silu(shift + x (1 + scale)), and written to y_mod.  Backward: stats is read; dx_out = (dx_in ? dx_in
 * : 0) + the LayerNorm backward of dy (dx_in may alias dx_out); d_gamma / d_beta [C] may be NULL (both NULL: the final reduction of their
 * partials is not launched at all).  C % 4 == 0, C <= 1536. */
int dsg_debug_t_ln(int32_t bwd, int32_t M, int32_t C, int32_t T, const float *x, const float *aff, float *y_mod, const float *gamma,
                   const float *beta, float *y, float *stats, const float *dy, const float *dx_in, float *dx_out, float *d_gamma,
                   float *d_beta, void *stream);
/* out = silu(shift_b + x (1 + scale_b)) on x [B T, C], aff [B, 2C] = (scale | shift); backward: out = dx from dy, d_aff [B, 2C] */
int dsg_debug_t_modulate(int32_t bwd, int32_t B, int32_t T, int32_t C, const float *x, const float *aff, const float *dy, float *out,
                         float *d_aff, void *stream);
/* out[n] = sum_m X[m ld + n] */
int dsg_debug_t_colsum(const float *X, int32_t ld, float *out, int32_t M, int32_t N, void *stream);
/* the backward of the input assembly fused with the preconditioning chain (dsg_precond_vjp's last kernel) on its own.  d_tok [B N N, ld]
 * token-major in the assembly's channel order -- self_cond == 0: [adj | node of the row | node of the column]; != 0: [sc_adj | adj |
 * sc_node(row) | node(row) | sc_node(col) | node(col)], of which only the current-value slots are read --, flags [B, N], c_skip / c_in
 * [B] (device), g = dL/dD in D's layouts.  With m the flags:
 *   out_adj[b,c,i,j] = c_skip_b m_i m_j g_adj[b,c,i,j] + c_in_b d_tok[(b,i,j)][adj slot c]
 *   out_node[b,i,c]  = c_skip_b m_i g_node[b,i,c] + c_in_b m_i (sum_j m_j d_tok[(b,i,j)][row slot c] + sum_j m_j d_tok[(b,j,i)][col slot c])
 * No atomics, one summation order: repeated calls give the same bits.  out_* may alias g_*.  Any N; ld >= the channel count. */
int dsg_debug_t_assemble_bwd(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, const float *d_tok, int32_t ld,
                             const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj, const float *g_node,
                             float *out_adj, float *out_node, void *stream);
/* ---- the edges of the training form at patch_size p in {2, 4} on their own (csrc/train_kernels_patch.hip; p = 1 is accepted).  Token
 * t = ti R + tj, R = N / p, covers the pixels (I, J) = (p ti + a, p tj + b); rows "in (token, a, b) order": m = (graph R^2 + t) p^2 + a p + b.
 * Every hook returns DSG_ERR_INVALID for a refused shape before anything is enqueued. */
/* kind DSG_TPACK_PE: W [E, c_in, p, p] (patch_embed.proj.weight) <-> img [E, ld], column (a p + b) c_in + c, ld >= p^2 c_in; pack writes
 * zeros from p^2 c_in up to ld, unpack never reads there.  kind DSG_TPACK_RO0: W [E, c_in, p, p] (read_out.0.weight, [in, out, p, p] with
 * out = c_in) <-> img [E, p^2 c_in], column (a p + b) c_in + o (ld is ignored); pack also writes bias_rep [p^2 c_in] from bias [c_in] when
 * both are given.  unpack != 0: img -> W. */
enum { DSG_TPACK_PE = 0, DSG_TPACK_RO0 = 1 };
int dsg_debug_t_patch_pack(int32_t kind, int32_t unpack, int32_t E, int32_t c_in, int32_t p, int32_t ld, float *W, float *img,
                           const float *bias, float *bias_rep, void *stream);
/* bwd == 0: F[b, c, I, J] = flag_I && flag_J ? oa[m][c] : 0 from oa [B N N, c_adj] in (token, a, b) order; bwd != 0 the transpose:
 * d_oa[m][c] = flag_I && flag_J ? dF[b, c, I, J] : 0.  Exact copies and exact zeros. */
int dsg_debug_t_adj_out_patch(int32_t bwd, int32_t B, int32_t N, int32_t p, int32_t c_adj, const float *oa, const uint8_t *flags, float *F,
                              const float *dF, float *d_oa, void *stream);
/* d_rep[m][e] += flag_I && flag_J ? d_pool[(b, I)][e] / N : 0, d_rep [B N N, E] in (token, a, b) order, d_pool [B N, E] */
int dsg_debug_t_pool_bwd_patch(int32_t B, int32_t N, int32_t p, int32_t E, const float *d_pool, const uint8_t *flags, float *d_rep_acc,
                               void *stream);
/* img [E, ld], ld = (p^2 G rounded up to 32), G = c_adj + 2 c_node: column (a p + b) G + slot holds W[e, src(slot), a, b], src the
 * current-value channel of the slot in the assembly's order (adj | node of the row | node of the column), zeros behind p^2 G.
 * W [E, c_in, p, p] with c_in = (self_cond ? 2 : 1) G.  *ld_out (host, may be NULL) receives ld; img == NULL only reports it. */
int dsg_debug_t_live_cols_patch(int32_t E, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t p, const float *W, float *img,
                                int32_t *ld_out, void *stream);
/* dsg_debug_t_assemble_bwd at patch_size p: d_tok [B R^2, ld] holds per token the p^2 groups of dsg_debug_t_live_cols_patch (columns
 * behind p^2 G are never read); pixel (I, J) reads group (I mod p) p + J mod p of token (I / p, J / p):
 *   out_adj[b,c,I,J] = c_skip_b m_I m_J g_adj[b,c,I,J] + c_in_b d_tok[pixel (I, J)][c]
 *   out_node[b,I,c]  = m_I (c_skip_b g_node[b,I,c] + c_in_b (sum_J m_J d_tok[pixel (I, J)][c_adj + c] + sum_J m_J d_tok[pixel (J, I)][c_adj + c_node + c]))
 * No atomics, one summation order; out_* may alias g_*; node values of padded nodes are never read. */
int dsg_debug_t_assemble_bwd_patch(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, const float *d_tok, int32_t ld,
                                   const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj, const float *g_node,
                                   float *out_adj, float *out_node, void *stream);
/* up to 32 small problems in one launch.  kind: DSG_TGROUP_NT / TN / NN: C_z = op(A_z) op(B_z) (+ bias_z); NN_SUM: ONE C = sum_z A_z B_z
 * (shared M, N, C; bias of problem 0); SUM: out[i] = sum_z C_z[i], i < n_out; COLSUM: C_z[n] = sum_m A_z[m lda + n]; TT is not built
 * and is refused. */
typedef struct dsg_t_prob {
    const float *A, *B, *bias;
    float *C;
    int32_t lda, ldb, ldc, M, N, K;
} dsg_t_prob;
enum { DSG_TGROUP_NT = 0, DSG_TGROUP_TN = 1, DSG_TGROUP_NN = 2, DSG_TGROUP_NN_SUM = 3, DSG_TGROUP_SUM = 4, DSG_TGROUP_COLSUM = 5, DSG_TGROUP_TT = 6 };
int dsg_debug_t_grouped(int32_t kind, int32_t n, const dsg_t_prob *probs, float *out, int32_t n_out, void *stream);

/* the per-graph contraction of dsg_ode_run on its own (test hook, no handle; device pointers, synchronises `stream`): out[b] = the sum
 * over the live entries of graph b of a_j b_j, float64, one fixed order, independent of B and of the graph's position; padded entries
 * are skipped by the flags (NaN there does not reach the sum).  a_adj / b_adj [B,C_adj,N,N], a_node / b_node [B,N,C_node], out [B]. */
int dsg_debug_graph_dot(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *a_adj, const float *a_node, const float *b_adj,
                        const float *b_node, const uint8_t *flags, double *out, void *stream);

/* ======== guidance ======== */

/* The guide kernel of dsg.h's dsg_sample_guided -- x_hat, D, g, c_i, f_b, D~ as defined there -- on its own (test hook, no handle; device pointers, synchronises `stream`): one call's arithmetic on given x_hat, D,
 * flags [B,N], node known mask [B,N,C_node] (NULL: none) and ONE coefficient `coef` in place of c_i; guide->weights is not read.
 * Outputs (each may be NULL): loss [B], grad [B,N,4] = g at the box channels, shift [B,N,4] = f_b coef g, factor [B], norms [B,2] =
 * (||coef g||, ||x_hat - D||; the second is 0 when unclipped), d_guided_node [B,N,C_node] = D~ (0 at padded nodes).  Rows of padded
 * nodes are never read.  Refusals as dsg_sample_guided's, before any launch; dsg_last_error of a NULL handle names the argument. */
int dsg_debug_box_guide(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                        const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_node,
                        const dsg_guide_cfg *guide, float coef, float *loss, float *grad, float *shift, float *factor, float *norms,
                        float *d_guided_node, void *stream);

/* dsg_debug_box_guide with the relation term: `rel` as dsg.h's dsg_sample_guided_rel takes it (NULL or w_rel == 0: the kernel without it), and kinds_out [B,N,N] uint8
 * (DEVICE, may be NULL): the kinds the kernel used, 0 at pairs that are not live (all 0 where the relation variant did not run).
 * d_adj is required with the decoded source; entries of padded rows and columns and of the diagonal are never read. */
int dsg_debug_box_guide_rel(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                            const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_node,
                            const dsg_guide_cfg *guide, float coef, float *loss, float *grad, float *shift, float *factor, float *norms,
                            float *d_guided_node, void *stream, const dsg_rel_cfg *rel, uint8_t *kinds_out);

/* The content kernel of dsg.h's dsg_sample_guided_content on its own (test hook, no handle; device pointers but the descriptor's host
 * arrays; synchronises `stream`): one call's arithmetic on given x_hat, D, flags [B,N], both known masks (mask_adj [B,C_adj,N,N],
 * mask_node [B,N,C_node]; NULL: none) and ONE coefficient `coef` in place of c_i.  Outputs (each may be NULL), K = n_items, Cl =
 * node_chans: loss [B], item_loss [B,K], grad_adj [B,C_adj,N,N], grad_label [B,N,Cl] = g, shift_adj / shift_label = f_b (coef w_content) g
 * as the update subtracts it, factor [B], norms [B,2] = (||coef w_content g||, ||x_hat - D||; the second is 0 when unclipped), best
 * [B,K,2] int32 = the pair (i, j) with the largest pi_k (the lowest flat index i N + j on an exact tie; -1, -1 where P = 0 or the item
 * is inactive), d_guided_adj [B,C_adj,N,N] / d_guided_node [B,N,C_node] = D~ (0 at padded entries).  Padded rows and columns and the
 * adjacency diagonal of D are never read by the kernel.  Refusals as dsg_sample_guided_content's, before any launch; dsg_last_error of a
 * NULL handle names the argument. */
int dsg_debug_content_guide(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                            const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_adj, const uint8_t *mask_node,
                            const dsg_content_cfg *content, float coef, float *loss, float *item_loss, float *grad_adj, float *grad_label,
                            float *shift_adj, float *shift_label, float *factor, float *norms, int32_t *best, float *d_guided_adj,
                            float *d_guided_node, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DSG_DEBUG_H */
