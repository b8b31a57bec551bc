// kernels.h -- launch wrappers of the gfx950 kernels (kernels.hip), used by dsg_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <unordered_map>
#include <vector>

namespace dsg {

// Plan validation (dsg_api.cpp: validate_plan): while this is set on the calling thread, every launcher of the forward path checks
// its arguments and picks its kernel as usual but launches nothing.  A launcher that does not cover a shape returns false -- it never
// terminates the process; the host turns that into DSG_ERR_INVALID at plan time (first use of a batch size / dsg_set_option).
extern thread_local bool g_dry_run;
// Option "batch_invariant" (dsg_api.cpp sets it in front of every GEMM launch): a launcher that would pick its tile from the number of
// rows keeps ONE tile at every size, so that which kernel computes a row never depends on the batch size.  Today that is the bf16
// GEMM's 256x96 / 128x96 choice (kernels_lp.hip: launch_gemm_lp), and in training form -- where only dsg_ode_run sets it -- t_gemm's
// MFMA route from 512 rows on (train_kernels.hip).
extern thread_local bool g_fixed_tiles;
// Test hook of the bf16 GEMM's tile choice (dsg_debug_gemm_lp sets it around its one launch; nothing else writes it): 0 the launcher's
// own rule, 1 the 128x96 tile, 2 the 256x96 tile.  launch_gemm_lp reads it ahead of g_fixed_tiles and its DSG_BF16_* statics, and
// leaves the block rows of the tile it chose in g_lp_tile_rows (128 or 256; meaningful when it returned true).  Both live in kernels_lp.hip.
extern thread_local int g_lp_tile_hook;
extern thread_local int g_lp_tile_rows;
struct GemmArgs;
bool launch_gemm_lp(const GemmArgs &g, hipStream_t s);   // kernels_lp.hip; false: the form is not built (nothing launched)

enum Act { ACT_NONE = 0, ACT_GELU = 1, ACT_SILU = 2,
           // training-form products of the fp32 GEMM only (launch_gemm): GELU whose pre-activation is kept in C2 (the backward needs it);
           // the product multiplied by GELU'(res) -- `res` is that kept pre-activation (the backward through fc2 and the GELU in one pass)
           ACT_GELU_KEEP = 3, ACT_DGELU = 4 };

// geometry of one Swin block's windows
struct WinGeom {
    int res;      // tokens per side
    int ws;       // window side
    int shift;    // cyclic shift (0 or ws/2)
    int heads;
    int C;
};

// C[M,N] = act( pro(A)[M,K] * W[N,K]^T + bias ) (+ res), optionally stored twice.
struct GemmArgs {
    const float *A = nullptr;  int lda = 0;      // rows of K1 floats (k <  K1)
    const float *A2 = nullptr; int lda2 = 0;     // optional second source (k >= K1): concat along K
    int K1 = 0;                                  // == K when A2 is null
    const float *W = nullptr;                    // [N, K] row-major (torch Linear layout)
    const void *Wb = nullptr;                    // the same weight as bf16 [N, K]: non-null selects the bf16-MFMA kernel
    const void *Ws3 = nullptr;                   // the same weight split into three bf16 planes [3][N][K]: split-bf16 kernel
    const float *bias = nullptr;                 // [N] or null
    const float *ln_stats = nullptr;             // [M,2] (mean, rstd): A is replaced by (A-mean)*rstd on the way in; the
                                                 // LayerNorm's gamma/beta must already be folded into W / bias
    const float *res = nullptr; int ldres = 0;   // residual added after the activation, or null
    float *C = nullptr;  int ldc = 0;
    float *C2 = nullptr; int ldc2 = 0;           // optional second destination
    int M = 0, N = 0, K = 0;                     // K % 32 == 0
    int act = ACT_NONE;
    // LayerNorm statistics from per-column-tile partial sums written by the PRODUCING GEMM's epilogue (stats_out below):
    // ln_part [M][ln_nparts][2] = (sum, sum of squares) over 96 columns each; mean/rstd are formed in the prologue
    const float *ln_part = nullptr; int ln_nparts = 0;
    // epilogue extensions of the fp32 kernel (act == ACT_NONE only): the next Swin block's modulate+SiLU
    // x <- silu(shift + x*(1+scale)) applied to the value stored to C (C2 keeps the un-modulated value), with
    // (scale,shift) = mod_aff[b*mod_ld + mod_off + {n, N+n}], b = row / mod_T (mod_ld == 0: one row for the whole batch);
    // and the row statistics of what was stored to C: stats_out [M][ceil(N/96)][2] partial (sum, sumsq) per column tile
    const float *mod_aff = nullptr; int mod_ld = 0, mod_off = 0, mod_T = 1;
    float *stats_out = nullptr;
    // fused QKV projection + window attention (8x8 windows; launch_gemm_qkv_attn): W = qkv weight [3C,K] (q rows pre-scaled),
    // bias = qkv bias [3C]; a block computes q|k|v of ONE head for TWO windows (rows gathered through the window partition /
    // cyclic shift), runs softmax(q k^T + attn_bias) v from LDS and stores the head's 32 output columns to C [M, wg.C]
    // PatchMerging gather in the A path (diffusesg.py:323-332): logical A row m = (b, i, j) of the coarse grid is
    // cat[x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)] of the fine activation g.A [B, a4_res^2, K/4]; no copy is ever
    // materialised.  LayerNorm(4C) statistics come from the four source rows' partials (ln_part, ln_nparts per source row).
    int a4_res = 0;                              // > 0 selects the gather; needs ln_part, no A2
    const float *attn_bias = nullptr;            // [nWt][heads][64][64] key-major, log2(e)-scaled (build_bias_table)
    WinGeom wg{0, 0, 0, 0, 0};
    int attn_batch = 0;
    int batch = 1;                               // > 1: that many independent products in one launch (fp32 kernel, AMODE 2: split-K slices)
    size_t batch_strideA = 0, batch_strideW = 0, batch_strideC = 0;   // floats between consecutive products' operands / outputs
    // masked-token pruning (fp32 kernel, AMODE 3): the launch computes only the rows of the 8-row runs listed in row_list
    // (run r = physical rows 8r .. 8r+7; -1 pads the list to a whole 128-row tile), *row_cnt of them (device-side: grids keep their
    // full size, tiles beyond the count return at once).  One physical row indexes A, A2, res, C, ln_part / ln_stats, stats_out and the
    // mod_aff sample alike.  launch_gemm_qkv_attn: row_list is a list of window indices instead (two per tile).
    const int *row_list = nullptr, *row_cnt = nullptr;
    // thin form of the list GEMM (64-row tiles, see kernels.hip): chosen on the device from *row_cnt by gemm_thin_rule() below.
    // n_cu: the device's multiprocessor count (0: never thin).  form: 0 the rule, 1 always wide, 2 always thin (test hook).
    int n_cu = 0, form = 0;
    // form switch of the deduplicated QKV projection (qk_split_rule below; dsg_api.cpp: run_block): qk_cnt = the device-side count of the
    // level's qk_runs list.  The fused QKV + attention launch over all rows (8 x 8 windows, no window list) returns at once where the rule
    // holds, the LayerNorm list GEMM without activation (the projection over qk_runs) where it does not.  null: no switch
    // qk_M: the rows the rule compares the listed rows with -- the launch's M (a measurement hook passes INT_MAX: split wherever a list exists)
    const int *qk_cnt = nullptr; int qk_M = 0;
    int a_bf16 = 0, c_bf16 = 0;                  // bf16 mode only: A / C are bf16 tensors (lda / ldc in elements); see kernels_lp.hip
    const float *gelu_tab = nullptr;             // filled in by launch_gemm (table-driven GELU of the split kernel)
    unsigned long long *prof = nullptr;          // measurement mode: {min block start, max block end} in 100 MHz ticks
};
bool launch_gemm(const GemmArgs &g, hipStream_t s);   // false: the argument combination is not built (nothing launched)
// The list GEMM's choice between its two forms, written once for the kernel, the launcher's grid and the host's reporting: a launch of
// cnt_runs 8-row runs takes ceil(cnt_runs / 16) x ceil(N / 96) wide (128 x 96) tiles; when those would occupy at most half the CUs, the
// thin form's twice as many 64 x 96 tiles still fit one per CU and each runs 2/3 of the wide tile's MFMA chain.  Above the bound two
// thin blocks per CU would take 4/3 of it.
__host__ __device__ inline bool gemm_thin_rule(int cnt_runs, int N, int n_cu) {
    if (cnt_runs < 0 || N < 1 || n_cu < 1) return false;
    return 2ll * ((cnt_runs + 15) / 16) * ((N + 95) / 96) <= (long long)n_cu;
}
// The form of a shifted block behind a deduplicated first block (option "dedup_qkv"): its QKV projection is row-wise and the fill has
// left most of its input rows as copies, so where the listed rows -- the non-pure windows plus one source pure window per content
// class, 8 rows per run -- are at most half of the M rows, the projection runs over the list and window_attn_map_kernel reads q, k, v
// through the window map (two launches, the attention re-reads w->qkv); above that the fused kernel over all rows is the cheaper form.
__host__ __device__ inline bool qk_split_rule(int listed_runs, int M) {
    return listed_runs > 0 && 2ll * 8 * listed_runs <= (long long)M;
}
// does launch_gemm build the thin form for these arguments?  (row list, no LayerNorm, no activation: the proj / fc2 / reduction shapes)
inline bool gemm_has_thin(const GemmArgs &g) {
    return g.row_list && !g.ln_stats && !g.ln_part && g.act == ACT_NONE && g.a4_res == 0 && !g.Ws3 && !g.Wb && g.batch == 1;
}
// fused LN1 -> QKV -> window attention for 64-token windows (fp32 kernel); returns false if the geometry is not supported
bool launch_gemm_qkv_attn(const GemmArgs &g, hipStream_t s);
// The attention of that launch on its own, from q, k, v rows already in qkv [B * T, 3 C] (the list GEMM over qk_runs wrote them): a block
// loads the tile's rows of its head into the same LDS slabs and runs the fused kernel's attention phase.  Token rows whose unshifted
// window w (b * nW + w) is not listed are read from the same position of window qk_src[b * nW + w].  Blocks return at once unless
// qk_split_rule(*qk_cnt, B * T).  g: as for launch_gemm_qkv_attn (wg, attn_batch, attn_bias, C / ldc the output); false: not built
bool launch_window_attn_map(const GemmArgs &g, const float *qkv, const int *qk_src, hipStream_t s);
void launch_f32_to_bf16(const float *src, void *dst, size_t n, hipStream_t s);

// ---- bf16 block pipeline (kernels_bx.hip; "gemm_bf16" mode): C = epilogue(A[M,K] . W[N,K]^T), A and W bf16 in HBM ----
struct BxGemm {
    const void *A = nullptr;  int lda = 0;        // bf16 [M, K1], leading dimension in elements (multiple of 8)
    const void *A2 = nullptr; int lda2 = 0;       // optional second source for k >= K1 (concat along K); K1 a multiple of the k chunk
    int K1 = 0;
    const void *W = nullptr;                      // bf16 [N, K]
    const float *bias = nullptr;                  // [N] or null
    const float *res = nullptr; int ldres = 0;    // fp32 residual, added after the activation
    float *C = nullptr; int ldc = 0;              // fp32 destination (optional; may alias res)
    void *Cb = nullptr; int ldcb = 0;             // bf16 destination (optional): the stored value, or with ln_out its LayerNorm (no affine)
    void *C2b = nullptr; int ldc2b = 0;           // bf16 copy of the value BEFORE the modulation below (skip connection)
    int M = 0, N = 0, K = 0;                      // K % 8 == 0, N % 4 == 0
    int act = ACT_NONE;                           // ACT_NONE | ACT_GELU
    // the next Swin block's modulate+SiLU applied to the stored value (GemmArgs::mod_* semantics)
    const float *mod_aff = nullptr; int mod_ld = 0, mod_off = 0, mod_T = 1;
    int ln_out = 0;                               // Cb = (v - mean(v)) * rstd(v) over the whole row: N must be 96, 192 or 384 (one tile)
    unsigned long long *dbg = nullptr;            // DSG_BX_EXP == 4 builds only: per-block phase clocks [grid][8] (tools/bx_exp.sh)
};
bool launch_gemm_bx(const BxGemm &g, hipStream_t s);   // false: shape not covered (nothing launched)
int bx_gemm_geo(const BxGemm &g);                      // the launcher's rule on its own: tile geometry 0 / 2 / 3, -1 where it refuses
// x <- [modulate_next] (x + fc2(GELU(fc1(xn)))) in one kernel (mlp_ratio 4, C in {96, 192, 384}); xn = LayerNorm-2 of x as bf16
// (gamma / beta folded into W1 / b1), W1 [4C, C] and W2 [C, 4C] bf16; xn_out (optional) receives the LayerNorm (out_mode 1) or the
// plain bf16 copy (out_mode 2) of the stored row; mod_* as BxGemm.  false: width not covered.
struct BxMlp {
    const void *xn = nullptr; float *x = nullptr;
    const void *W1 = nullptr; const float *b1 = nullptr; const void *W2 = nullptr; const float *b2 = nullptr;
    void *xn_out = nullptr; int out_mode = 0;
    const float *mod_aff = nullptr; int mod_ld = 0, mod_off = 0, mod_T = 1;
    int M = 0, C = 0;
    int wide8 = 1;   // C = 384: 1 the eight-wave LDS-DMA kernel (needs img), 2 round 3's eight-wave kernel, 0 mlp_bx_kernel<384> (one wave per SIMD)
    unsigned long long *dbg = nullptr;   // measurement runs of the debug entry: [grid][8 waves][8] s_memtime stamps (mlp384d_bx_kernel)
    const void *img96 = nullptr; // C = 96 with proj, no modulate: W1 | W2 | Wp in fragment order (launch_mlp96r_image) -> the LDS-resident kernel
    const void *img2 = nullptr;  // C = 384, wide8 = 3: the chunk-major image of mlp384s_bx_kernel (launch_mlp384s_images; same byte count as img)
    int skew = 0;                // mlp384d_bx_kernel: stagger step of the first-round blocks in shader clocks (0: all start together)
    const void *img = nullptr;   // C = 384: W1 | W2 | Wp pre-arranged for mlp384d_bx_kernel (launch_mlp384_images; mlp384_image_bytes())
    // the attention half's tail in front (att != null; xn is then unused): x <- x + att Wp^T + bp first, its LayerNorm feeds fc1
    const void *att = nullptr, *Wp = nullptr; const float *bp = nullptr;
};
bool launch_mlp_bx(const BxMlp &g, hipStream_t s);
// the C = 384 weights in the order mlp384d_bx_kernel's LDS-DMA ring and fragment reads want them: W1b [1536, 384], W2b [384, 1536],
// Wpb [384, 384] (may be null: no proj stage) row-major bf16 -> img (mlp384_image_bytes() bytes)
size_t mlp384_image_bytes();
void launch_mlp384_images(const void *W1b, const void *W2b, const void *Wpb, void *img, hipStream_t s);
size_t mlp96r_image_bytes();
void launch_mlp96r_image(const void *W1b, const void *W2b, const void *Wpb, void *img, hipStream_t s);
void launch_mlp384s_images(const void *W1b, const void *W2b, const void *Wpb, void *img, hipStream_t s);
// x fp32 [B*T, C] -> optional in-place modulate+SiLU (aff != null) -> xn bf16: LayerNorm without affine (ln) or the plain copy
void launch_ln_bx(float *x, const float *aff, int aff_ld, int aff_off, void *xn, int B, int T, int C, bool ln, hipStream_t s);
// window attention on bf16 qkv [B*T, 3C] -> bf16 out [B*T, C]; biasT as launch_window_attn; false: window size not covered
bool launch_attn_bx(const void *qkv, const float *biasT, void *out, int B, const WinGeom &g, hipStream_t s);
// QKV projection + window attention fused (no qkv tensor): xn bf16 [B*T, C] (LayerNorm-1 without affine), W bf16 [3C, C] and bias [3C]
// (gamma / beta and the q scale folded in), biasP = the block's bias tiles in accumulator order as fp16 (launch_bias_permute_bx of the
// [nWt][heads][Wp][Wp] table), out bf16 [B*T, C].  false: window size / width not covered.
struct BxQkvAttn { const void *xn = nullptr, *W = nullptr; const float *bias = nullptr; const void *biasP = nullptr; void *out = nullptr; int B = 0; WinGeom g{0, 0, 0, 0, 0};
                   int variant = 0; const void *Wimg = nullptr; const float *biasF = nullptr; unsigned long long *dbg = nullptr; };   // Wimg: launch_qkv_image of W (the wave-per-unit kernel streams it)
void launch_qkv_image(const void *Wb, void *img, int C, int heads, hipStream_t s);
void launch_bias_permute_f32(const float *biasT, float *out, int n_tiles, int Wp, hipStream_t s);   // biasF: the tiles in accumulator order, fp32   // 10 x 10 windows: 0 one wave per (window, head) (qkv_attn_wx_kernel), 1 one block per (window, head) (qkv_attn_bx_kernel)
bool launch_qkv_attn_bx(const BxQkvAttn &a, hipStream_t s);
void launch_bias_permute_bx(const float *biasT, void *out_fp16, int n_tiles, int Wp, hipStream_t s);
void launch_f32_split3(const float *src, void *dst, size_t n, hipStream_t s);
void launch_bf16_to_f32(const void *src, float *dst, size_t n, hipStream_t s);
// device table of the fused MLP's table-driven GELU; must be called once (outside any stream capture) before the first launch
const float *gelu_table();

// x <- x + fc2(GELU(fc1(LN(x)))) with fragment-major packed weights (pack_mlp_weights in dsg_api.cpp); C in {96,192}
// stats_out (optional): [M][1][2] (sum, sumsq) of the rows written back, in the GEMM epilogue's partial format
void launch_fused_mlp(float *x, const float *gam, const float *bet, const float *W1p, const float *b1, const float *W2p,
                      const float *b2, int M, int C, float *stats_out, hipStream_t s,
                      const int *run_list = nullptr, const int *run_cnt = nullptr);   // run list: only those 8-row runs (GemmArgs::row_list)

// input assembly + 1x1 conv + LayerNorm + modulate+SiLU in one kernel (E = 96, in_chans <= 64); false if unsupported
bool launch_fused_patch_embed96(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                                const uint8_t *flags, const float *Wp, const float *bias, const float *gam, const float *bet,
                                const float *aff, int aff_ld, int aff_off, int aff_off2, float *x, int B, int N, int Ca, int Cn,
                                int self_cond, int Kp, hipStream_t s, void *xn = nullptr,   // aff_off2 >= 0: also apply that block's
                                // modulate+SiLU; xn (bf16 [B*N*N, 96]): also the LayerNorm (no affine) of the stored row (bf16 pipeline)
                                const int *run_list = nullptr, const int *run_cnt = nullptr);   // run list: only those 8-token runs (no xn then)
// final LN + folded read_out/adj-head chain + masked adjacency output, and the LN(x) pooling for the node head (E = 96)
// pool_part [B*N][readout_pool_segments(N)][96]: per-tile partial sums, reduced in fixed order into pool_ext [B*N,128]
int readout_pool_segments(int N);
void launch_fused_readout96(const float *x, const float *gam, const float *bet, const float *Wfp, const float *fa, const float *W2p,
                            const float *f2, const uint8_t *flags, float *out_adj, float *pool_part, float *pool_ext, int B, int N,
                            int Ca, hipStream_t s, bool bf16_frags = false,   // bf16_frags: Wfp / W2p are bf16 fragments (dsg_api.cpp: ro_fapb / ro_f2pb)
                            const int *tile_list = nullptr, const int *tile_cnt = nullptr);   // the list form (NeedPlan::ro_tiles; fp32 fragments only)
// whole attention half of a C=96 Swin block in one kernel (modulate+SiLU, LN1, QKV, window attention, proj, residual);
// windows of at most 64 tokens; packed weights from pack_attn_weights in dsg_api.cpp
void launch_fused_attn96(float *x, const float *aff, int aff_ld, int aff_off, const float *gam, const float *bet, const float *Wqp,
                         const float *bqkv, const float *biasT, const float *Wpp, const float *bproj, int B, const WinGeom &g,
                         bool premod, hipStream_t s,    // premod: x is already modulated by the producing kernel
                         const int *win_list = nullptr, const int *win_cnt = nullptr);   // window list: only those windows (b * nW + w), *win_cnt of them
// qkv [B*T, 3C] token order -> out [B*T, C] token order; biasT [nWt][heads][Wp][Wp] (key-major)
bool launch_window_attn(const float *qkv, const float *biasT, float *out, int B, const WinGeom &g, hipStream_t s, bool out_bf16 = false, bool in_bf16 = false);   // false: not built (nothing launched)

// x <- silu(shift + x*(1+scale)), (scale,shift) = aff[b][off .. off+2C); stats of the new rows
void launch_mod_stats(float *x, const float *aff, int aff_ld, int aff_off, float *stats, int B, int T, int C, hipStream_t s);
// stats[m] = (mean, rstd) of row m
void launch_ln_stats(const float *x, float *stats, int M, int C, hipStream_t s);
// y = silu(shift + LN(x)*(1+scale)) (PatchEmbed tail)
void launch_ln_mod(const float *x, const float *g, const float *b, const float *aff, int aff_ld, int aff_off,
                   float *y, int B, int T, int C, hipStream_t s);
// PatchMerging gather + LN(4C): x [B,res*res,C] -> y [B,(res/2)^2,4C]
void launch_merge_ln(const float *x, const float *g, const float *b, float *y, int B, int res, int C, hipStream_t s, bool out_bf16 = false);
// PatchBreakup middle: LN(D) -> 4 chunks scattered 2x2 -> LN(D/4): y [B,res*res,D] -> z [B,(2res)^2,D/4]
void launch_breakup_ln(const float *y, const float *g, const float *b, const float *pg, const float *pb, float *z,
                       int B, int res, int D, hipStream_t s, bool out_bf16 = false,   // out_bf16: z is a bf16 tensor (y stays fp32)
                       const int *run_list = nullptr, const int *run_cnt = nullptr);   // run list over the COARSE rows of y
// positional embedding of the noise label: pe [B,E]
void launch_noise_pe(const float *c_noise, float *pe, int B, int E, hipStream_t s);
// input assembly: token-major [B*N*N, Kp] (zero padded), channel order of diffusesg.py:792-802
void launch_assemble(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                     const uint8_t *flags, float *out, int B, int N, int Ca, int Cn, int self_cond, int Kp, hipStream_t s);
// adjacency head tail: h [B*N*N, E] -> out [B,Ca,N,N] = mask(h @ W^T + b)
void launch_head_adj(const float *h, const float *W, const float *bias, const uint8_t *flags, float *out,
                     int B, int N, int E, int Ca, hipStream_t s);
// masked mean pooling over j (divided by N): rep [B*N*N, E] -> pool [B*N, E]
void launch_pool(const float *rep, const uint8_t *flags, float *pool, int B, int N, int E, hipStream_t s);
// node head tail: h [B*N, E] -> out [B,N,Cn] = mask(h @ W^T + b)
void launch_head_node(const float *h, const float *W, const float *bias, const uint8_t *flags, float *out,
                      int B, int N, int E, int Cn, hipStream_t s);

// ---- patch_size p > 1 (kernels_patch.hip): token t = ti R + tj of the R = N / p grid covers the pixels (p ti + a, p tj + b); the rows
// of the read-out chain are in (token, a, b) order, row m = (b R^2 + t) p^2 + a p + b.  false: arguments refused (nothing launched) ----
// input assembly: out [B R^2, Kp], k = (a p + b) Cin + c (c in launch_assemble's channel order), zero padded from p^2 Cin
bool launch_assemble_patch(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                           const uint8_t *flags, float *out, int B, int N, int p, int Ca, int Cn, int self_cond, int Kp, hipStream_t s);
// adjacency head tail: h [B N^2, E] rows in (token, a, b) order -> out [B,Ca,N,N] = valid(I, J) ? h @ W^T + b : 0
bool launch_head_adj_patch(const float *h, const float *W, const float *bias, const uint8_t *flags, float *out, int B, int N, int p, int E,
                           int Ca, hipStream_t s);
// masked mean pooling over the N pixels J of node row I: rep [B N^2, E] in (token, a, b) order -> pool [B N, E]
bool launch_pool_patch(const float *rep, const uint8_t *flags, float *pool, int B, int N, int p, int E, hipStream_t s);

// The fused forms for E = 96, p = 2.  PatchEmbed: Wp [4][3][Kps / 8][64] float4, sub-pixel sub = 2 a + b, each launch_fused_patch_embed96's
// fragment order of patch_embed.proj.weight[:, :, a, b] zero-padded to Kps = 32 | 64 >= in_chans; the rest as launch_fused_patch_embed96
// (no xn, no run list); x [B (N/2)^2, 96].
bool launch_fused_patch_embed96_p2(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                                   const uint8_t *flags, const float *Wp, const float *bias, const float *gam, const float *bet,
                                   const float *aff, int aff_ld, int aff_off, int aff_off2, float *x, int B, int N, int Ca, int Cn,
                                   int self_cond, int Kps, hipStream_t s);
// Read-out: x [B (N/2)^2, 96]; Wfp [4][3][12][64] float4: the folded Fa[a, b] per sub-pixel in launch_fused_readout96's fragment order;
// fa, W2p, f2 as there.  pool_part: scratch [B N/2][readout_pool_segments_p2(N)][2][96]; pool_ext [B N, 256]: per node row
// (s[ti, 0] | s[ti, 1] | flag_I cnt_0 / N | flag_I cnt_1 / N | 0 ..), s[ti, q] = (1/N) sum_tj flag_{2 tj + q} LN(x)[ti, tj]
int readout_pool_segments_p2(int N);
bool launch_fused_readout96_p2(const float *x, const float *gam, const float *bet, const float *Wfp, const float *fa, const float *W2p,
                               const float *f2, const uint8_t *flags, float *out_adj, float *pool_part, float *pool_ext, int B, int N,
                               int Ca, hipStream_t s);

// ---- masked-token pruning: device-side need lists (kernels.hip: need_lists_kernel) ----
// A plan is a short program on one sample's set of needed 8-token runs, starting from the last level's output need (runs that hold a
// pair with flag_i && flag_j) and walking the up path backwards.  Lists are compacted over the whole batch: run lists hold
// b * res * res / 8 + run, window lists b * nW + window; list L lives at lists + list_off[L] with room for every entry + 16.
enum NeedKind { NEED_EMIT = 0,      // write the current set (side `res`) as run list `list`
                NEED_WINDOWS = 1,   // windows of the partition (res, shift) holding a needed run -> window list `list` (-1: none);
                                    // the set becomes every run those windows touch
                NEED_PARENT = 2 };  // res = fine side: the set becomes the coarse runs holding a parent (i/2, j/2) of a needed token
struct NeedOp { int kind, res, shift, list; };
constexpr int NEED_MAX_OPS = 40, NEED_MAX_LISTS = 32, NEED_MAX_RUNS = 2048;   // runs of one sample at the finest level: N * N / 8
constexpr int NEED_MAX_DD_UP = 3;   // coarser levels the pure-window deduplication may reach (N <= 128: 16, 8, 4, 2 windows per side)
struct NeedPlan { int n_ops = 0, n_lists = 0; NeedOp op[NEED_MAX_OPS]; int list_off[NEED_MAX_LISTS];
                  // pure-window deduplication (below), levels 0 .. dd_n - 1 of the down path (0: none): level k's unique 8-token runs,
                  // its unique windows and the pure windows that are filled by copy; -1 = the level has no such lists
                  int dd_n = 0, dd_runs[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1}, dd_wins[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1},
                      dd_copy[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1},
                  // option "dedup_qkv" (qk_split_rule above), for a level whose second block is shifted: qk_runs -- the 8-token runs of every
                  // non-pure window plus those of one source pure window per content class (the batch's representative window under
                  // DD_BATCH / DD_TABLE, the graph's first pure window under DD_GRAPH; DD_OFF lists every window); qk_src [B * nW] -- for
                  // every window the window whose rows of the QKV tensor hold its q, k, v: itself when listed, else its class's source
                      qk_runs[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1}, qk_src[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1},
                  // the fused read-out's working tiles (its list form) -- tile t is tokens [32 t, 32 t + 32) of the flattened [B * N * N]
                  // index (a graph is a whole number of tiles: N % 8 == 0), listed when one of them has flag_i && flag_j; -1: no such list
                      ro_tiles = -1; };
static_assert(sizeof(NeedPlan) == sizeof(int) * (2 + 4 * NEED_MAX_OPS + NEED_MAX_LISTS + 1 + 5 * (1 + NEED_MAX_DD_UP) + 1), "NeedPlan is a kernel argument: keep it packed");
// cnt_ps [B][n_lists] scratch, lists / cnt [n_lists] as above; two small launches, to be enqueued wherever the flags are staged
// dedup (a DedupMode) / dd_rep / trim_mask: see below (dd_rep [plan.dd_n][B] + 1 int, the mode; may be null when the plan has no dd_* lists)
enum DedupMode { DD_OFF = 0,      // every window is listed as unique, nothing is copied
                 DD_GRAPH = 1,    // one representative pure window per graph
                 DD_BATCH = 2,    // one for the whole batch ("One representative for the batch" below)
                 DD_TABLE = 3 };  // DD_BATCH with that one taken from a per-step table instead of being computed ("The table" below)
void launch_need_lists(const uint8_t *flags, int B, int N, const NeedPlan &plan, int *cnt_ps, int *lists, int *cnt, hipStream_t s,
                       int dedup = DD_OFF, int *dd_rep = nullptr, int trim_mask = 0);

// ---- pure-window deduplication (option "dedup_masked") ----
// Level k of the down path (k = 0 the finest; res = N >> k tokens per side, width C = E << k) has 8 x 8 windows that cover 8 << k nodes
// per side.  Such a window is PURE when no valid pair lies under it: no valid node in its row block of 8 << k nodes, or none in its
// column block -- at level 0, every token (i, j) of it has a padded endpoint (!(flag_i && flag_j)).  Every pure window of a graph gets
// the same 64 rows from the level's unshifted first block:
//   level 0 -- where the forward's inputs are zero at such tokens, PatchEmbed gives all of them one row;
//   level k >= 1 -- a pure window lies over 2 x 2 pure windows of level k - 1, whose rows are equal window by window behind that level's
//   copy (provided that level has no further, shifted block), and PatchMerging is a row-wise function of the 2 x 2 fine rows;
// and the block sees positions only inside a window.  So one representative per graph (its first pure window, dd_rep[k * B + b] =
// b * nW_k + w, -1: the graph has none) is computed and the others are filled by copy.  need_lists_kernel writes, for every planned
// level and in the formats above (ids b * nW_k + w, runs b * res * res / 8 + run): dd_wins[k] / dd_runs[k] -- every non-pure window
// plus the representative, as windows and as their 8-token runs; dd_copy[k] -- the pure windows other than the representative.
// DD_OFF (the caller does not vouch for the zeros): every window is listed as unique, nothing is copied.
// One representative for the batch (DD_BATCH).  Nothing in the argument above uses the graph index: where every graph also reads the
// same (scale, shift) row (the sampler's batch-uniform sigma, aff_ld = 0), a pure window of graph a and one of graph b get the same 64
// rows at every level.  Level k's representative is then the first pure window of the BATCH in (graph, window) order; dd_rep[k * B + b]
// holds that one global id for every b (-1: no graph has a pure window at level k), the unique lists hold every non-pure window plus
// that one, and the copies read it across graphs.  The representatives of two levels may lie in different graphs.
// trim_mask, bit k: level k's fill lists only the pure windows that lie under a unique window of level k + 1 (a non-pure one or that
// level's representative) -- the only ones anything reads when the merge into level k + 1 runs over that level's run list and the
// up path reads level k's skip through a coarse list (which stays inside non-pure windows below a chain of unshifted single blocks).
// A level without the bit (the top of the chain, whose next reader takes everything) fills every other pure window.  Chain premise:
// every fine window under a unique coarse window is unique or filled, whichever graphs the representatives lie in.
// The table (DD_TABLE, option "dedup_table").  The batch's representative depends on the weights and the step's (scale, shift) row only,
// so the sampler computes it once per schedule index ahead of the loop (PureTab: per index and level the 64 rows of x, of the skip and
// their (sum, sumsq) pairs).  The lists are DD_BATCH's with the representative moved from the unique lists to the fill list: dd_wins /
// dd_runs hold the non-pure windows only, dd_copy every pure window DD_BATCH fills plus the former representative (dd_rep still names
// it), and the fill reads the table entry of the running step's schedule index.  need_lists_kernel leaves the mode the lists were
// written for in dd_rep[dd_n * B], where the fill reads it: the launches are the same for every mode.
// The merge into such a level, over its run list: merged row m = (b, i, j) of y [B * (res / 2)^2, 4 C] = the LayerNorm(4 C) (no affine:
// gamma / beta are folded into the reduction weight) of cat[x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)], statistics from the four
// fine rows' (sum, sumsq) partials ln_part [B * res^2][nparts][2] -- element for element the value the gather form of the GEMM
// (GemmArgs::a4_res) puts into its A tile, so the row-mapped GEMM on y gives that launch's rows bit for bit.  C % 4 == 0, (res / 2) % 8 == 0.
void launch_merge_norm_runs(const float *x, const float *ln_part, int nparts, float *y, int B, int res, int C, const int *run_list,
                            const int *run_cnt, hipStream_t s);
// The copy of level k: rows of x [B * res * res, C], of skip (same shape; null: none -- level 0 has no skip yet) and nparts (sum, sumsq)
// pairs per row of stats (null: none); rep [B] = that level's representatives (global window ids, of any graph).  C % 4 == 0
// tab: where *tab.mode == DD_TABLE every listed window is filled from the table entry of schedule index steps[ctl->step].sched
// instead (base null: no table, the mode is never DD_TABLE).  An entry is `stride` floats: per level 64 x C rows of x at off_x, of
// the skip at off_skip and 64 x nparts pairs at off_st, window tokens in row-major order.  entries = the table's capacity (the index
// is clamped to it, and the step to ctl->n_steps - 1: an eager forward behind a finished run reads the last step's entry)
struct StepRow;
struct RunCtl;
struct PureTabSrc { const float *base = nullptr; size_t stride = 0; int entries = 0, off_x = 0, off_skip = 0, off_st = 0;
                    const StepRow *steps = nullptr; const RunCtl *ctl = nullptr; const int *mode = nullptr; };
void launch_window_broadcast(float *x, float *skip, float *stats, int nparts, int B, int res, int C, const int *copy_list,
                             const int *copy_cnt, const int *rep, hipStream_t s, const PureTabSrc &tab = PureTabSrc());
// Building the table: window 0 of each of the first n graphs -> entry g of dst (the layout above; skip / stats null: not stored)
void launch_window_harvest(const float *x, const float *skip, const float *stats, int nparts, int n, int res, int C, float *dst,
                           size_t stride, int off_x, int off_skip, int off_st, hipStream_t s);

// ---- preconditioning / sampler elementwise kernels (adj and node parts handled in one launch) ----
struct StatePtrs { float *adj; float *node; };
struct CStatePtrs { const float *adj; const float *node; };
struct Dims { int B, N, Ca, Cn; };

// test-only: n_words 32-bit words at p become pattern 1 zeros, 2 quiet NaN (0x7fc00000: both bf16 halves NaN too), 3 1.0e30f, 4 finite
// pseudo-random values of unit scale with random sign, a function of (seed, word index)  (dsg_debug_poison, "debug_alloc_fill")
void launch_debug_fill(void *p, size_t n_words, int pattern, unsigned long long seed, hipStream_t s);

// c_noise[i] = ln(sigma[i])/4
void launch_cnoise(const float *sigmas, float *c_noise, int n, hipStream_t s);
// in = c_in(sigma[b]) * x ; c_noise[b] = ln(sigma[b])/4
void launch_precond_in(CStatePtrs x, const float *sigmas, StatePtrs in, float *c_noise, Dims d, hipStream_t s);
// D = mask(c_skip*x + c_out*F)
void launch_precond_out(CStatePtrs x, CStatePtrs F, const float *sigmas, const uint8_t *flags, StatePtrs D, Dims d, hipStream_t s);
// x0 = mask(eps) * scale (gen_init_sample + initial scaling); eps from `init` or Philox(seed, stream): stream 0 is the
// initial sample, stream i+1 the churn noise of step i (launch_churn)
// base given (the partial-noise start of dsg_sample_walk): x = mask(base + scale * eps); base in the state layouts
// graph_seeds given (device [B]; per-graph noise streams, dsg_sample_seeded / dsg_gen_noise_seeded): the draw of graph b is
// Philox(graph_seeds[b], stream, j), the same generator, with j the element's index INSIDE its graph -- adjacency (c, i, k):
// (c N + i) N + k; node (i, c): Ca N^2 + i Cn + c, i.e. the global index of the unseeded draw at B = 1; `seed` is not read.
// Each of the four combinations launches its own instantiation.
void launch_init(CStatePtrs init, CStatePtrs base, float scale, uint64_t seed, const unsigned long long *graph_seeds, uint32_t stream,
                 const uint8_t *flags, StatePtrs x, Dims d, hipStream_t s);
// the probe of dsg_ode_run drawn on the device: Philox(graph_seeds[b], stream, local index) as launch_init draws it (gaussian), or
// its sign, +1 where the draw is >= 0 and -1 elsewhere (rademacher); 0 at padded entries.  graph_seeds: device [B], required
void launch_probe(bool rademacher, const unsigned long long *graph_seeds, uint32_t stream, const uint8_t *flags, StatePtrs eps, Dims d,
                  hipStream_t s);

// ---- reverse-loop kernels driven by a DEVICE step counter, so that one captured step body can be replayed for every step ----
// Per-step scalars, computed on the host up front exactly as before (dsg_sigma_schedule) and uploaded once per sample() call: one row
// per EXECUTED step.  sched = the schedule index the step runs at -- the row of the per-schedule-index tables (launch_step_row); it
// equals the step counter in the plain loop and repeats in a resampling walk (dsg_sample_walk).
// ms_coef = c_k of the second-order multistep update (launch_multistep_tab); 0 in every row of every other step, where no kernel reads it.
struct StepRow { float noise_coef, sigma, inv_t, inv_tp, h; int sched; float ms_coef; int pad; };
static_assert(sizeof(StepRow) == 32, "StepRow is 32 bytes");
// Per-run control block at a fixed device address: the step counter the kernels index StepRow[] / the noise streams with, and the
// number of executed steps of the run (rows of StepRow[]).
// graph_seeds: null -- one key (`seed`) and the global element index; device [B] (a seeded run) -- per-graph keys and local indices
struct RunCtl { int step; int n_steps; unsigned long long seed; const float *noise_adj; const float *noise_node; const unsigned long long *graph_seeds; };
// x_hat = mask(x + coef[step]*eps), eps = recorded noise[step] (ctl->noise_*) or Philox(seed, step+1) / Philox(graph_seeds[b], step+1)
void launch_churn_tab(CStatePtrs x, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags, StatePtrs xhat, Dims d, hipStream_t s);
// in = c_in(sigma[step]) * x
void launch_precond_in_tab(CStatePtrs x, const StepRow *tab, const RunCtl *ctl, StatePtrs in, Dims d, hipStream_t s);
// D = mask(c_skip*x + c_out*F) at sigma[step]
void launch_precond_out_tab(CStatePtrs x, CStatePtrs F, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags, StatePtrs D, Dims d,
                            hipStream_t s);
// conditional sampling: the same D with a per-element select in front of the store -- mask ? known : c_skip*x + c_out*F (0 at padded
// entries); mask_adj / mask_node uint8 in the state layouts, nonzero = known.  A select, not a blend: known arrives bit-exact in D
struct CMaskPtrs { const uint8_t *adj; const uint8_t *node; };
void launch_precond_out_tab_known(CStatePtrs x, CStatePtrs F, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags, CStatePtrs known,
                                  CMaskPtrs mask, StatePtrs D, Dims d, hipStream_t s);
// autoguidance (dsg_attach_guide): the composite D~ = fadd(D_m, fmul(sm1, fsub(D_m, D_g))) in the store of the same
// skeleton -- D_m and D_g each formed from x and its network's F by the operations of launch_precond_out*, in registers; x, F_main and
// F_guide are read once, no D_m / D_g tensor exists.  sm1 = s - 1 in float32.
// The per-sample form (dsg_precond) takes sm1 where lo <= sigma[b] <= hi and 0 elsewhere; the table forms (the reverse loop) belong
// to a step the host found inside the interval.  known: the select runs on D_m and on D_g, so a known entry is the known value itself
void launch_precond_out_mix(CStatePtrs x, CStatePtrs F_main, CStatePtrs F_guide, const float *sigmas, float sm1, float lo, float hi,
                            const uint8_t *flags, StatePtrs D, Dims d, hipStream_t s);
void launch_precond_out_mix_tab(CStatePtrs x, CStatePtrs F_main, CStatePtrs F_guide, float sm1, const StepRow *tab, const RunCtl *ctl,
                                const uint8_t *flags, StatePtrs D, Dims d, hipStream_t s);
void launch_precond_out_mix_tab_known(CStatePtrs x, CStatePtrs F_main, CStatePtrs F_guide, float sm1, const StepRow *tab, const RunCtl *ctl,
                                      const uint8_t *flags, CStatePtrs known, CMaskPtrs mask, StatePtrs D, Dims d, hipStream_t s);
void launch_euler_tab(CStatePtrs xhat, CStatePtrs D, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags, StatePtrs x, Dims d,
                      hipStream_t s);
void launch_heun_tab(CStatePtrs xhat, CStatePtrs D1, CStatePtrs D2, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags,
                     StatePtrs x, Dims d, hipStream_t s);
// DPM-Solver++ 2M in EDM variables: the Euler update with D replaced by D + ms_coef[step] * (D - Dprev), Dprev = the previous step's D
void launch_multistep_tab(CStatePtrs xhat, CStatePtrs D, CStatePtrs Dprev, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags,
                          StatePtrs x, Dims d, hipStream_t s);
// ---- box guidance through the skip path (guide_kernels.hip; dsg_sample_guided) ----
// What a guided step body reads, at a fixed device address that the body bakes; the run rewrites the contents, so the tables behind
// the pointers may move without invalidating a captured body.  a_o / a_r / a_a: weights of the overlap, region and alignment loss;
// sel [B,N] / region [B,N,4] (x0, y0, x1, y1): the region loss's nodes and rectangles (read only where a_r != 0); coef [T]: c_i per
// SCHEDULE index (dsg_guide_coef); trace [L,B] or null: L(D) of every executed step's stage-1 call; mask_node [B,N,Cn] or null: the
// known mask of a conditioned run -- the shift is zero there
// The relation term (dsg_sample_guided_rel), read only by the kernel's relation variant: a_rel its weight, rel_margin the
// hinge margin; rel_source REL_GIVEN: kinds [B,N,N] uint8 (subject = row, object = column); REL_DECODED: the kinds are decoded from the
// call's adjacency estimate by decode_attr(rel_enc, rel_ntype) and looked up in pred_kind [rel_ntype] (device copy of the caller's table)
struct GuideParams { float a_o, a_r, a_a, tau, clip_ratio; int pad; const uint8_t *sel; const float *region; const float *coef; float *trace;
                     const uint8_t *mask_node;
                     float a_rel, rel_margin; int rel_source, rel_enc, rel_ntype, rel_pad; const uint8_t *kinds; const uint8_t *pred_kind; };
constexpr int GUIDE_MAX_N = 64;
constexpr int REL_NONE = 0, REL_GIVEN = 1, REL_DECODED = 2;   // StepPlan::rel; GuideParams::rel_source holds REL_GIVEN or REL_DECODED
constexpr int REL_KINDS = 8;                                  // 0 none, 1 left of, 2 right of, 3 above, 4 below, 5 inside, 6 contains, 7 on
// ||a_b - b_b||^2 over the live entries of each graph, float64, one fixed order (t_graph_dot's).  false: shape refused (N > GUIDE_MAX_N)
bool launch_graph_diff_norm(CStatePtrs a, CStatePtrs b, const uint8_t *flags, double *out, Dims d, hipStream_t s);
// per-graph outputs of the guide kernel; every pointer but shift may be null.  shift [B,N,4] = f_b c g as the update subtracts it,
// grad [B,N,4] = dL/dD at the box channels, loss [B], factor [B] = f_b, norms [B,2] = (||c g||, ||x_hat - D||; the second 0 without clip)
struct BoxGuideOut { float *shift, *grad, *loss, *factor, *norms; };
// One block per graph: L(D) and g from closed forms, c = P->coef[tab[ctl->step].sched] (tab null: coef_direct), shift zero at known and
// padded entries, f_b = guide.clip_factor from ref_norm2 [B] (launch_graph_diff_norm; null: unclipped, f_b = 1).  stage1: also writes
// the trace row of the executed step.  false: shape refused (N > GUIDE_MAX_N, Cn < 4)
bool launch_box_guide(const GuideParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_node, const uint8_t *flags,
                      const double *ref_norm2, bool stage1, BoxGuideOut o, Dims d, hipStream_t s);
// The same with the relation term L_rel of P (a_rel, rel_*) added: the graph's kinds sit in LDS, given or decoded from D_adj [B,Ca,N,N]
// (rows, columns and the diagonal that are not live are never read); kinds_out [B,N,N] or null: the kinds the kernel used.  A kernel of
// its own: launch_box_guide runs what it ran.  false: shape refused (also D_adj null with the decoded source)
bool launch_box_guide_rel(const GuideParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_adj, const float *D_node,
                          const uint8_t *flags, const double *ref_norm2, bool stage1, BoxGuideOut o, uint8_t *kinds_out, bool decoded, Dims d,
                          hipStream_t s);
// out = valid ? D_node - shift (box channels) : 0  -- D~ on its own, for dsg_debug_box_guide
void launch_box_apply(const float *D_node, const float *shift, const uint8_t *flags, float *out, Dims d, hipStream_t s);
// the update operations reading D~ = D - shift at the box channels of the node estimate (shift buffers [B,N,4] of launch_box_guide);
// instantiations of their own: the unguided kernels carry no extra load or branch
void launch_euler_tab_guided(CStatePtrs xhat, CStatePtrs D, const float *shift, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags,
                             StatePtrs x, Dims d, hipStream_t s);
void launch_heun_tab_guided(CStatePtrs xhat, CStatePtrs D1, CStatePtrs D2, const float *shift1, const float *shift2, const StepRow *tab,
                            const RunCtl *ctl, const uint8_t *flags, StatePtrs x, Dims d, hipStream_t s);
void launch_multistep_tab_guided(CStatePtrs xhat, CStatePtrs D, CStatePtrs Dprev, const float *shift, const float *shift_prev, const StepRow *tab,
                                 const RunCtl *ctl, const uint8_t *flags, StatePtrs x, Dims d, hipStream_t s);
// ---- content guidance (guide_content_kernels.hip; dsg_sample_guided_content) ----
// What a content-guided step body reads, at a fixed device address that the body bakes; the run rewrites the contents.  w: the weight
// of L_content; K items per graph, Cl label channels; subj / obj [B,K,Cl], pred [B,K,Ca], w_spo [B,K,3] (a_s, a_o, a_p): workspace
// copies of the caller's host arrays; coef [T]: c_i per SCHEDULE index; trace [L,B] or null; mask_adj [B,Ca,N,N] / mask_node [B,N,Cn]
// or null: the known masks of a conditioned run -- the shift is zero there
constexpr int CONTENT_MAX_ITEMS = 16;
struct ContentParams { float w, tau, clip_ratio; int K, Cl, pad; const float *subj, *obj, *pred, *w_spo; const float *coef; float *trace;
                       const uint8_t *mask_adj, *mask_node; };
// outputs of the content kernel; every pointer but the two shifts may be null.  shift_adj [B,Ca,N,N] / shift_label [B,N,Cl] = f_b c w g as
// the update subtracts it, grad_* = g, loss [B], item_loss [B,K], factor [B] = f_b, norms [B,2] = (||c w g||, ||x_hat - D||; the second 0
// without clip), best [B,K,2] = the pair with the largest pi_k (lowest flat index among equals; -1, -1: no live pair, inactive item)
struct ContentOut { float *shift_adj, *shift_label, *grad_adj, *grad_label, *loss, *item_loss, *factor, *norms; int *best; };
// One block per graph; c = P->coef[tab[ctl->step].sched] (tab null: coef_direct); f_b from ref_norm2 [B] (launch_graph_diff_norm; null:
// unclipped).  stage1: also writes the trace row of the executed step.  false: shape refused (N > GUIDE_MAX_N, Cn < 5)
// grid_items 0: that one launch; grid_items = K: the grid form -- K x B blocks for the item phase, N^2 / 512 x B blocks for the
// pair-major phase, then one block per graph for the label channels, the norm and the clip; `stats` holds CONTENT_STATS_PER_GRAPH
// doubles per graph between the launches.  The same arithmetic in the same order: the same bits.  content_grid_items(K): the form
// a run takes, 0 or K
constexpr int CONTENT_STAT_DOUBLES = 4 + 4 * 64, CONTENT_GRID_MIN_ITEMS = 1;
constexpr size_t CONTENT_STATS_PER_GRAPH = (size_t)CONTENT_MAX_ITEMS * CONTENT_STAT_DOUBLES + 64 * 64;
int content_grid_items(int K);
bool launch_content_guide(const ContentParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_adj, const float *D_node,
                          const uint8_t *flags, const double *ref_norm2, bool stage1, ContentOut o, int grid_items, double *stats, Dims d,
                          hipStream_t s);
// out = valid ? D - shift : 0 (adjacency entries and label channels) -- D~ on its own, for dsg_debug_content_guide; either output may be null
void launch_content_apply(const float *D_adj, const float *D_node, const float *sh_adj, const float *sh_label, const uint8_t *flags,
                          float *out_adj, float *out_node, int Cl, Dims d, hipStream_t s);
// the content shift of one stage as the update operations read it: adjacency entries and label channels (c < P->Cl) of the node estimate
struct ContentShiftPtrs { const float *adj, *label; };
// the guided updates with both shifts, box [B,N,4] and content: kernels of their own next to the box-only ones above
void launch_euler_tab_guided2(CStatePtrs xhat, CStatePtrs D, const float *shift, ContentShiftPtrs cs, const ContentParams *P, const StepRow *tab,
                              const RunCtl *ctl, const uint8_t *flags, StatePtrs x, Dims d, hipStream_t s);
void launch_heun_tab_guided2(CStatePtrs xhat, CStatePtrs D1, CStatePtrs D2, const float *shift1, const float *shift2, ContentShiftPtrs cs1,
                             ContentShiftPtrs cs2, const ContentParams *P, const StepRow *tab, const RunCtl *ctl, const uint8_t *flags,
                             StatePtrs x, Dims d, hipStream_t s);
void launch_multistep_tab_guided2(CStatePtrs xhat, CStatePtrs D, CStatePtrs Dprev, const float *shift, const float *shift_prev,
                                  ContentShiftPtrs cs, ContentShiftPtrs cs_prev, const ContentParams *P, const StepRow *tab, const RunCtl *ctl,
                                  const uint8_t *flags, StatePtrs x, Dims d, hipStream_t s);
// dst[0..n) = table[tab[step].sched][0..n)  (the (scale,shift) row of the step's schedule index), and ctl->step += 1
void launch_step_row(const float *table, int n, const StepRow *tab, const RunCtl *ctl, float *dst, hipStream_t s);
void launch_step_advance(RunCtl *ctl, hipStream_t s);
// ---- training-time objective and loss, forward only ----
// sigma_b = exp(rnd_b*1.2 - 1.2), weight_b = (sigma^2 + .25)/(sigma*.5)^2, noisy = clean + mask(eps*sigma) (adjacency: the sum
// is masked); rnd / eps: given tensors, or Philox(seed) streams when null (objectives/edm.py:160-180, :239-281)
void launch_train_inputs(CStatePtrs clean, const float *rnd, CStatePtrs eps, uint64_t seed, const uint8_t *flags, float *sigmas,
                         float *weights, StatePtrs noisy, Dims d, hipStream_t s);
// NodeAdjRainbowLoss(reduction='none') + the trainer's bbox IoU term: per-sample losses [B] (rainbow_loss.py:37-101,
// trainer_node_adj.py:130-159); one block per sample, fixed-order reduction
// iou_type: 0 'iou', 1 'giou', 2 'giou_squared', 3 'diou', 4 'ciou' (trainer_node_adj.py:138-153; DSG_IOU_* of dsg.h)
void launch_rainbow_loss(CStatePtrs pred, CStatePtrs tgt, const uint8_t *flags, const float *w, float edge_w, float node_w, float iou_w,
                         int iou_type, float *loss_adj, float *loss_node, Dims d, hipStream_t s);
// ---- training-time block (train_kernels.hip; correctness-first kernels, not on the sampling path) ----
struct TrainBlockParams {   // the 15 parameter tensors of a SwinTransformerBlock, reference layouts ([out, in] linears)
    float *aff_w, *aff_b, *n1_w, *n1_b, *rpb, *qkv_w, *qkv_b, *proj_w, *proj_b, *n2_w, *n2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct TrainBlockArgs {
    int B, res, ws, shift, heads, C, hidden;
    TrainBlockParams W, G;                 // weights (read) and their gradients (written)
    const float *x_in, *emb, *grad_out;    // [B*T, C], [B, 512], [B*T, C] or null (forward only)
    float *x_out, *grad_in, *grad_emb;     // [B*T, C], [B*T, C], [B, 512]
    // saved forward tensors and scratch (caller-allocated): aff / d_aff [B, 2C]; x_mod, xn1, att, x1, xn2, d_x1, t_mc, t_mc2 [M, C];
    // stats1, stats2 [M, 2]; qkv, t_m3c [M, 3C]; pre, hid, t_mh [M, hidden]
    float *aff, *d_aff, *x_mod, *xn1, *att, *x1, *xn2, *d_x1, *t_mc, *t_mc2, *stats1, *stats2, *qkv, *t_m3c, *pre, *hid, *t_mh;
    // whole-network step: a.aff is already filled (one grouped launch for all blocks) and the affine linear's own backward
    // (dW, db, d_emb from a.d_aff) is left to grouped launches at the end
    bool aff_grouped = false;
    // backward without the weight-gradient products (dW, db, d_gamma, d_beta, d_table, and the affine linear's own backward): only
    // grad_in is produced, G is not touched (input gradients, dsg_precond_vjp)
    bool no_wgrad = false;
    // bf16 mode of the covered products (qkv, proj, fc1, fc2: y, dx and dW); null: fp32.  See TrainLp below
    struct TrainLp *lp = nullptr;
};
// a group of small products in one launch (t_gemm_grouped / t_colsum_grouped): C = op(A) op(B) (+ bias)
struct TGemmProb { const float *A, *B, *bias; float *C; int lda, ldb, ldc, M, N, K; };
constexpr int T_GROUP_MAX = 32;
struct TGemmGroup { TGemmProb p[T_GROUP_MAX]; int n = 0; };
void t_gemm_grouped(bool ta, bool tb, bool sum, const TGemmGroup &g, hipStream_t s);   // sum: ONE output = the sum of the products (shared M, N, C)
void t_sum_grouped(const TGemmGroup &g, float *out, int n, hipStream_t s);           // out[i] = sum_z p[z].C[i], i < n (contiguous outputs)
void t_colsum_grouped(const TGemmGroup &g, hipStream_t s);                             // p.C[n] = sum_m p.A[m][n] per problem
bool train_block(const TrainBlockArgs &a, hipStream_t s);            // forward; + backward when a.grad_out is set
bool train_block_backward(const TrainBlockArgs &a, hipStream_t s);   // backward alone, from the tensors the forward left in `a`
// building blocks of the whole-network training step (same file): C (+)= op(A) op(B) (+ bias), column sums, elementwise / row ops
// a_colsum (weight-gradient products, ta && !tb): also out[m] = sum_k A[k][m], the bias gradient that goes with dW = dy^T x
void t_gemm(bool ta, bool tb, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc, int M, int N, int K,
            bool accumulate, hipStream_t s, float *a_colsum = nullptr, const float *res = nullptr, int act = ACT_NONE, float *c2 = nullptr,
            int *route = nullptr, int force_plain = -1, struct TrainLp *lp = nullptr);
// res: C = res + product (same pitch as C); act = ACT_GELU_KEEP: c2 = product + bias, C = GELU(c2); act = ACT_DGELU: C = product * GELU'(res)
// route (test hook, host): route[0] = the path taken -- 1 the sampling GEMM (launch_gemm), 2 gemm_tn_f32_kernel + reduce, 3 the plain
// kernel, 4 the plain kernel with split-K, 0 refused --, route[1] = its slice count S; force_plain >= 0 replaces DSG_TRAIN_PLAIN_GEMM
// ---- bf16 mode of the training products (train_kernels_lp.hip; dsg_train_set_precision) ----
// A call site that is covered passes the entry's TrainLp to t_gemm.  The product then runs with both operands rounded to bf16 (RNE) on
// v_mfma_f32_32x32x16_bf16, fp32 accumulation and an fp32 result, wherever t_lp_rule holds and -- for y = x W^T and dx = dy W -- the
// weight's bf16 plane is in `planes`; everywhere else it silently takes the fp32 route it has without the mode.
//   y  (cls 0, !ta &&  tb): launch_gemm_lp on plane nk = bf16 of W [out, in]
//   dx (cls 1, !ta && !tb): launch_gemm_lp on plane kn = bf16 of W^T [in, out]
//   dW (cls 2,  ta && !tb): gemm_tn_bf16_kernel + t_splitk_reduce; a_colsum from the unrounded fp32 values
// The fused activations (ACT_GELU_KEEP, ACT_DGELU) are finished by t_gelu's elementwise pass.
struct TLpPlane { const void *nk = nullptr, *kn = nullptr; };
struct TLpCount { int rows, cls, n_bf16, n_f32; };   // products of class cls over `rows` tokens that took the bf16 / the fp32 route
struct TrainLp {
    std::unordered_map<const float *, TLpPlane> planes;   // by fp32 weight pointer
    std::vector<TLpCount> counts;
    bool any_rows = false;   // test hook: waive the 512-row threshold (the kernels take any row count)
    bool only = false;       // test hook: a product the bf16 route does not take is refused (nothing launched) instead of run in fp32
    void count(int rows, int cls, bool lp) {
        for (TLpCount &c : counts) if (c.rows == rows && c.cls == cls) { (lp ? c.n_bf16 : c.n_f32)++; return; }
        counts.push_back(TLpCount{rows, cls, lp ? 1 : 0, lp ? 0 : 1});
    }
};
// the shape rule on top of the call sites: what t_gemm's MFMA form takes today -- 512 token rows, both channel extents multiples of 32
inline bool t_lp_rule(size_t rows, int c0, int c1) { return rows >= 512 && c0 > 0 && c1 > 0 && c0 % 32 == 0 && c1 % 32 == 0; }
// false: the bf16 route does not take this product (nothing launched).  route as t_gemm's: 5 launch_gemm_lp, 6 gemm_tn_bf16_kernel + reduce
bool t_gemm_lp(TrainLp &lp, bool ta, bool tb, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc, int M, int N,
               int K, bool accumulate, hipStream_t s, float *a_colsum, const float *res, int act, float *c2, int *route);
// up to T_CAST_MAX weights W [R, Cc] (contiguous fp32) -> bf16 planes nk [R, Cc] and kn [Cc, R] (either may be null), RNE, one launch
struct TCastJob { const float *src; void *nk, *kn; int R, Cc, tile0; };   // tile0: the job's first 32 x 32 tile in the launch's grid
constexpr int T_CAST_MAX = 64;
struct TCastGroup { TCastJob j[T_CAST_MAX]; int n = 0, tiles = 0; };
void t_cast_lp_add(TCastGroup &g, const float *src, void *nk, void *kn, int R, int Cc);   // (the caller flushes a full group)
void t_cast_lp(const TCastGroup &g, hipStream_t s);
// pieces of train_kernels.hip that the bf16 route shares
float *t_scratch_sk(hipStream_t s, size_t need);   // the stream's split-K scratch grown to `need` floats; null: out of memory (marked)
void t_scratch_mark_failed(hipStream_t s);
void t_splitk_reduce(const float *part, float *C, int ldc, int M, int N, int S, bool accumulate, const float *cs_part, float *cs_out, hipStream_t s);
// scratch of the training kernels is kept per stream (train_kernels.hip); a failed allocation is reported here, once
bool t_scratch_failed(hipStream_t s, bool clear);
void t_scratch_release();
void t_colsum(const float *X, int ld, float *out, int M, int N, hipStream_t s);
void t_silu(const float *x, const float *dy, float *out, size_t n, bool bwd, hipStream_t s);
void t_gelu(const float *x, const float *dy, float *out, size_t n, bool bwd, hipStream_t s);
void t_add(float *a, const float *b, size_t n, hipStream_t s);
void t_ln_fwd(const float *x, const float *gam, const float *bet, float *y, float *stats, int M, int C, hipStream_t s);
// dx_out = (dx_in ? dx_in : 0) + LayerNorm backward of dy; d_gamma / d_beta (either may be null) = the affine parameters' gradients
void t_ln_bwd(const float *x, const float *gam, const float *stats, const float *dy, const float *dx_in, float *dx_out, float *d_gamma, float *d_beta,
              int M, int C, hipStream_t s);
void t_modulate(const float *x, const float *aff, const float *dy, float *out, float *d_aff, int B, int T, int C, bool bwd, hipStream_t s);
// test hooks (dsg_debug_t_attn / dsg_debug_t_ln): the file-local launchers; force_plain replaces DSG_TRAIN_PLAIN_ATTN
bool t_attn_debug(bool bwd, const float *qkv, const float *table, float *out, const float *d_out, float *d_qkv, float *d_table, int B, int res,
                  int ws, int shift, int heads, bool force_plain, hipStream_t s);
void t_ln_fwd_mod(const float *x, const float *aff, float *y_mod, const float *gam, const float *bet, float *y, float *stats, int M, int C, int T,
                  hipStream_t s);
void t_regroup(const float *src, float *dst, int B, int res, int C, bool gather, hipStream_t s);
void t_concat(const float *x, const float *skip, float *cat, size_t M, int C, hipStream_t s);
void t_split(const float *dcat, float *dx, float *dskip_acc, size_t M, int C, hipStream_t s);
void t_adj_out(const float *oa, const uint8_t *flags, float *F, const float *dF, float *d_oa, int B, int N, int Ca, bool bwd, hipStream_t s);
void t_pool_bwd(const float *d_pool, const uint8_t *flags, float *d_rep_acc, int B, int N, int E, hipStream_t s);
void t_rowmask(const float *x, const uint8_t *flags, float *y, size_t M, int C, hipStream_t s);
// input gradients of the preconditioned denoiser (dsg_precond_vjp; train_kernels.hip)
// dF = c_out_b mask(g) (the way in); coef [2B] = (c_skip | c_in), formulas as launch_precond_out / launch_precond_in
void t_precond_bwd(const float *g_adj, const float *g_node, const float *sigmas, const uint8_t *flags, float *dF_adj, float *dF_node,
                   float *coef, int B, int N, int Ca, int Cn, hipStream_t s);
// img [E][t_live_cols_width] = the columns of PatchEmbed's W [E, Cin] that see the current adjacency / node values, zero-padded to x32
int t_live_cols_width(int Ca, int Cn);
void t_live_cols(const float *W, int Cin, float *img, int E, int Ca, int Cn, bool self_cond, hipStream_t s);
// backward of launch_assemble fused with the preconditioning chain (formulas at the kernel); false: shape refused (B, N, Ca < 1, a pitch
// below the channel count, or a C_node whose partial sums do not fit LDS: t_assemble_bwd_ok)
bool t_assemble_bwd_ok(int Cn);
bool t_assemble_bwd(const float *d_tok, int ld, const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj,
                    const float *g_node, float *out_adj, float *out_node, int B, int N, int Ca, int Cn, bool self_cond, hipStream_t s);
// the edges of the training form at patch_size p in {2, 4} (train_kernels_patch.hip; p = 1 is accepted and gives the p = 1 layouts).
// Rows of the read-out chain are in (token, a, b) order.  Every launcher returns false on refused arguments, before anything is enqueued.
// patch_embed.proj.weight [E, Cin, p, p] <-> image [E, Kp], column (a p + b) Cin + c, zero-padded (unpack reads the live columns only)
int t_pe_image_width(int Cin, int p);
bool t_pe_pack(const float *W, float *img, int E, int Cin, int p, int Kp, hipStream_t s);
bool t_pe_unpack(const float *img, float *dW, int E, int Cin, int p, int Kp, hipStream_t s);
// read_out.0.weight [in, out, p, p] <-> image [in, p^2 out], column (a p + b) out + o; bias_rep [p^2 out] (may be null)
bool t_ro0_pack(const float *W, const float *bias, float *img, float *bias_rep, int Ei, int Eo, int p, hipStream_t s);
bool t_ro0_unpack(const float *img, float *dW, int Ei, int Eo, int p, hipStream_t s);
bool t_adj_out_patch(const float *oa, const uint8_t *flags, float *F, const float *dF, float *d_oa, int B, int N, int p, int Ca, bool bwd,
                     hipStream_t s);
bool t_pool_bwd_patch(const float *d_pool, const uint8_t *flags, float *d_rep_acc, int B, int N, int p, int E, hipStream_t s);
// img [E][t_live_cols_patch_width]: per sub-pixel group (a p + b) the (adj | row node | column node) slots of the current values
int t_live_cols_patch_width(int Ca, int Cn, int p);
bool t_live_cols_patch(const float *W, int Cin, int p, float *img, int E, int Ca, int Cn, bool self_cond, hipStream_t s);
bool t_assemble_bwd_patch_ok(int Cn);
bool t_assemble_bwd_patch(const float *d_tok, int ld, const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj,
                          const float *g_node, float *out_adj, float *out_node, int B, int N, int p, int Ca, int Cn, hipStream_t s);
// out[b] = sum over the live entries of graph b of a_j b_j (adjacency entries whose two nodes are valid, node entries of valid nodes; the
// flags select, so whatever sits at a padded entry -- t_assemble_bwd leaves anything there -- never reaches the sum), accumulated in
// float64 in one fixed order by one block per graph: no atomics, and a graph's result depends neither on B nor on its position.
// false: shape refused (B, N, Ca or Cn < 1, N beyond the flag row kept in LDS)
bool t_graph_dot(const float *a_adj, const float *a_node, const float *b_adj, const float *b_node, const uint8_t *flags, double *out, int B,
                 int N, int Ca, int Cn, hipStream_t s);
bool t_adam_step(int n,float *const *params, float *const *grads, float *const *m, float *const *v, const int64_t *numel, int step, float lr,
                 float b1, float b2, float eps, float wd, float max_norm, float *host_total_norm, hipStream_t s);
bool t_ema_update(int n, float *const *ema, const float *const *params, const int64_t *numel, float decay, hipStream_t s);

void launch_rainbow_loss_backward(CStatePtrs pred, CStatePtrs tgt, const uint8_t *flags, const float *w, float edge_w, float node_w,
                                  float iou_w, int iou_type, const float *sigmas, StatePtrs grad, StatePtrs gradF, Dims d, hipStream_t s);
// post-decode of the samples; enc_*: 0 'bits', 1 'one_hot', 2 'ddpm' (DSG_ENC_* of dsg.h); node_chans = attribute channels of a node row
void launch_decode(const float *adj, const float *node, const uint8_t *flags, int enc_adj, int enc_node, int n_adj_type, int n_node_type,
                   int node_chans, int32_t *out_adj, int32_t *out_node, float *out_bbox, Dims d, hipStream_t s);
// the inverse: integer graphs (q_adj [B,N,N], q_node [B,N], bbox [B,N,4] in [0,1] or null) -> the network's value space, out_adj
// [B,Ca,N,N], out_node [B,N,Cn] (attribute in the first node_chans channels, bbox in the last four, channels in between 0)
void launch_encode(const int32_t *q_adj, const int32_t *q_node, const float *bbox, const uint8_t *flags, int enc_adj, int enc_node,
                   int n_adj_type, int n_node_type, int node_chans, float *out_adj, float *out_node, Dims d, hipStream_t s);

}  // namespace dsg
