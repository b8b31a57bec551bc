// The test bench of libdsg.so that needs no handle (include/dsg_debug.h): single-kernel hooks over the launchers of kernels.h.  Each fills
// a launcher's argument block from its parameters, launches once and synchronises the stream.  The hooks that read a handle's state
// (taps, poison, the list hooks, dsg_profile_*) and the guide hooks, which share their argument checks with the sampler, are in dsg_api.cpp.
#include "../../include/dsg_debug.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "kernels.h"

using namespace dsg;

namespace {

// how every hook ends: DSG_ERR_INVALID when the launcher did not build the form, DSG_ERR_HIP on a HIP error, both after the synchronise
int debug_finish(bool built, hipStream_t s) {
    const hipError_t e = hipStreamSynchronize(s);
    if (!built) return DSG_ERR_INVALID;
    return (e == hipSuccess && hipGetLastError() == hipSuccess) ? DSG_OK : DSG_ERR_HIP;
}

// the device temporaries of one hook call: freed when the call returns, whichever way.  After a failed allocation ok is false and every
// further get() returns null without allocating: a hook asks for all its buffers, checks ok once and returns DSG_ERR_HIP.
struct Scratch {
    std::vector<void *> bufs;
    bool ok = true;
    void *get(size_t bytes) {
        void *p = nullptr;
        ok = ok && hipMalloc(&p, bytes) == hipSuccess;
        if (ok) bufs.push_back(p);
        return ok ? p : nullptr;
    }
    ~Scratch() { for (void *p : bufs) (void)hipFree(p); }
};

bool mult4(int32_t v) { return v >= 0 && v % 4 == 0; }

}  // namespace

extern "C" {

// ---- the default fp32 path's kernels on their own: DSG_ERR_INVALID when the launcher does not build the form ----
int dsg_debug_gemm_f32(const dsg_gemm_f32_args *a, void *stream) {
    if (!a || !a->A || !a->W || !a->C || a->act < ACT_NONE || a->act > ACT_DGELU) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g;
    g.A = a->A; g.lda = a->lda; g.A2 = a->A2; g.lda2 = a->lda2; g.K1 = a->A2 ? a->K1 : a->K;
    g.W = a->W; g.bias = a->bias;
    g.ln_stats = a->ln_stats; g.ln_part = a->ln_part; g.ln_nparts = a->ln_nparts;
    g.res = a->res; g.ldres = a->ldres; g.C = a->C; g.ldc = a->ldc; g.C2 = a->C2; g.ldc2 = a->ldc2;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    g.mod_aff = a->mod_aff; g.mod_ld = a->mod_ld; g.mod_off = a->mod_off; g.mod_T = a->mod_T > 0 ? a->mod_T : 1;
    g.stats_out = a->stats_out;
    g.a4_res = a->a4_res;
    g.row_list = a->row_list; g.row_cnt = a->row_cnt;
    // `reserved` selects the list GEMM's form: 0 the kernel's rule (with this device's CU count), 1 wide, 2 thin
    if (a->reserved < 0 || a->reserved > 2) return DSG_ERR_INVALID;
    g.form = a->reserved;
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) g.n_cu = n_cu;
    return debug_finish(launch_gemm(g, s), s);
}

int32_t dsg_debug_gemm_form(int32_t cnt_runs, int32_t N, int32_t n_cu) { return gemm_thin_rule(cnt_runs, N, n_cu) ? 2 : 1; }
int32_t dsg_debug_qk_split(int32_t listed_runs, int32_t M) { return qk_split_rule(listed_runs, M) ? 1 : 0; }

// ---- one GEMM in a chosen arithmetic through launch_gemm, which falls back to the fp32 kernel where a bf16 form is not built ----
int dsg_debug_gemm(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias, const float *ln_stats,
                   const float *res, int32_t act, int32_t mode, float *C, void *stream) {
    if (M < 1 || N < 1 || K < 32 || K % 32 != 0 || !A || !W || !C || act < 0 || act > 2 || mode < 0 || mode > 2) return DSG_ERR_INVALID;
    if (!gelu_table()) return DSG_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    void *wlp = mode ? sc.get((size_t)N * K * (mode == 1 ? 2 : 6)) : nullptr;
    if (!sc.ok) return DSG_ERR_HIP;
    if (mode == 1) launch_f32_to_bf16(W, wlp, (size_t)N * K, s);
    if (mode == 2) launch_f32_split3(W, wlp, (size_t)N * K, s);
    GemmArgs g;
    g.A = A; g.lda = K; g.K1 = K; g.K = K; g.M = M; g.N = N; g.W = W; g.bias = bias; g.ln_stats = ln_stats; g.act = act;
    if (res) { g.res = res; g.ldres = N; }
    g.C = C; g.ldc = N;
    if (mode == 1) g.Wb = wlp;
    if (mode == 2) g.Ws3 = wlp;
    return debug_finish(launch_gemm(g, s), s);
}

// ---- the bf16-MFMA GEMMs on their own: launch_gemm_lp directly, so a refused form is an error and never the fp32 kernel ----
int dsg_debug_gemm_lp(const dsg_gemm_lp_args *a, void *stream) {
    if (a && a->tile_used) *a->tile_used = 0;
    if (!a || !a->A || !a->W || !a->C || a->act < ACT_NONE || a->act > ACT_SILU) return DSG_ERR_INVALID;
    if (a->mode < 1 || a->mode > 2 || a->tile < 0 || a->tile > 2 || (a->tile && a->mode == 2) || (a->tile == 2 && a->M < 256)) return DSG_ERR_INVALID;
    if (a->M < 1 || a->N < 1 || a->K < 32 || a->K % 32 != 0 || a->row_list || a->row_cnt || a->reserved != 0) return DSG_ERR_INVALID;
    // what the kernels take on trust from the forward: pitches that hold a row and keep its 16-byte loads aligned
    const int K1 = a->A2 ? a->K1 : a->K;
    if (a->A2 && (K1 < 1 || K1 >= a->K || a->lda2 < a->K - K1 || a->lda2 % 4 != 0)) return DSG_ERR_INVALID;
    if (a->a4_res == 0 && (a->lda < K1 || a->lda % (a->a_bf16 ? 8 : 4) != 0)) return DSG_ERR_INVALID;
    if (a->ldc < a->N || (a->C2 && a->ldc2 < a->N) || (a->res && a->ldres < a->N)) return DSG_ERR_INVALID;
    if ((a->ln_part && a->ln_nparts < 1) || (a->ln_part && a->ln_stats) || (a->mod_aff && !a->stats_out)) return DSG_ERR_INVALID;
    if (!gelu_table()) return DSG_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t nw = (size_t)a->N * a->K;
    Scratch sc;
    void *wlp = sc.get(nw * (a->mode == 1 ? 2 : 6));
    if (!sc.ok) return DSG_ERR_HIP;
    if (a->mode == 1) launch_f32_to_bf16(a->W, wlp, nw, s); else launch_f32_split3(a->W, wlp, nw, s);
    GemmArgs g;
    g.A = static_cast<const float *>(a->A); g.lda = a->lda; g.A2 = a->A2; g.lda2 = a->lda2; g.K1 = K1;
    g.W = a->W; g.bias = a->bias;
    if (a->mode == 1) g.Wb = wlp; else g.Ws3 = wlp;
    g.ln_stats = a->ln_stats; g.ln_part = a->ln_part; g.ln_nparts = a->ln_nparts;
    g.res = a->res; g.ldres = a->ldres; g.C = static_cast<float *>(a->C); g.ldc = a->ldc; g.C2 = a->C2; g.ldc2 = a->ldc2;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    g.mod_aff = a->mod_aff; g.mod_ld = a->mod_ld; g.mod_off = a->mod_off; g.mod_T = a->mod_T > 0 ? a->mod_T : 1;
    g.stats_out = a->stats_out;
    g.a4_res = a->a4_res;
    g.a_bf16 = a->a_bf16 != 0; g.c_bf16 = a->c_bf16 != 0;
    g_lp_tile_hook = a->tile;
    const bool built = launch_gemm_lp(g, s);
    g_lp_tile_hook = 0;
    if (a->tile_used) *a->tile_used = built ? g_lp_tile_rows : 0;
    return debug_finish(built, s);
}

int dsg_debug_convert(int32_t kind, const void *src, void *dst, int64_t n, void *stream) {
    if (kind < 0 || kind > 2 || !src || !dst || n < 1 || n >= ((int64_t)1 << 31)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (kind == 0) launch_f32_to_bf16(static_cast<const float *>(src), dst, (size_t)n, s);
    else if (kind == 1) launch_f32_split3(static_cast<const float *>(src), dst, (size_t)n, s);
    else launch_bf16_to_f32(src, static_cast<float *>(dst), (size_t)n, s);
    return debug_finish(true, s);
}

int dsg_debug_qkv_attn_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, int32_t K, const float *x, const float *W,
                           const float *bias, const float *ln_stats, const float *ln_part, int32_t ln_nparts, const float *attn_bias,
                           const int32_t *win_list, const int32_t *win_cnt, float *out, void *stream) {
    if (B < 1 || res < 1 || ws < 1 || heads < 1 || K < 1 || shift < 0 || shift >= ws || !x || !W || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int C = 32 * heads;
    GemmArgs g;
    g.A = x; g.lda = K; g.K1 = K; g.K = K; g.M = B * res * res; g.N = 3 * C;
    g.W = W; g.bias = bias; g.ln_stats = ln_stats; g.ln_part = ln_part; g.ln_nparts = ln_nparts;
    g.attn_bias = attn_bias; g.wg = WinGeom{res, ws, shift, heads, C}; g.attn_batch = B;
    g.C = out; g.ldc = C;
    g.row_list = win_list; g.row_cnt = win_cnt;
    return debug_finish(launch_gemm_qkv_attn(g, s), s);
}

int dsg_debug_window_attn_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *biasT,
                              float *out, void *stream) {
    if (B < 1 || res < 1 || ws < 1 || heads < 1 || shift < 0 || shift >= ws || !qkv || !biasT || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_window_attn(qkv, biasT, out, B, WinGeom{res, ws, shift, heads, 32 * heads}, s), s);
}

int dsg_debug_fused_mlp_f32(int32_t M, int32_t C, float *x, const float *gam, const float *bet, const float *W1p, const float *b1,
                            const float *W2p, const float *b2, float *stats_out, const int32_t *run_list, const int32_t *run_cnt,
                            void *stream) {
    // launch_fused_mlp builds C = 96 and C = 192 only and launches nothing otherwise; a run list addresses whole 8-row runs
    if (M < 1 || (C != 96 && C != 192) || !x || !gam || !bet || !W1p || !b1 || !W2p || !b2 || (run_list && (!run_cnt || M % 8 != 0)))
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    launch_fused_mlp(x, gam, bet, W1p, b1, W2p, b2, M, C, stats_out, s, run_list, run_cnt);
    return debug_finish(true, s);
}

int dsg_debug_fused_attn96_f32(int32_t B, int32_t res, int32_t ws, int32_t shift, float *x, const float *aff, int32_t aff_ld,
                               int32_t aff_off, const float *gam, const float *bet, const float *Wqp, const float *bqkv, const float *biasT,
                               const float *Wpp, const float *bproj, int32_t premod, const int32_t *win_list, const int32_t *win_cnt,
                               void *stream) {
    // launch_fused_attn96 covers windows of at most 64 tokens (pack_attn_weights packs for nothing else)
    // (aff is required with premod too: the kernel forms the pointers to the sample's rows either way)
    if (B < 1 || res < 1 || ws < 1 || ws * ws > 64 || res % ws != 0 || shift < 0 || shift >= ws || !x || !aff || !gam || !bet || !Wqp ||
        !bqkv || !biasT || !Wpp || !bproj || (win_list && !win_cnt))
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    launch_fused_attn96(x, aff, aff_ld, aff_off, gam, bet, Wqp, bqkv, biasT, Wpp, bproj, B, WinGeom{res, ws, shift, 3, 96}, premod != 0, s,
                        win_list, win_cnt);
    return debug_finish(true, s);
}

// ---- the fp32 forward's edge and row kernels on their own (test hooks; tests/test_edge_kernels.py) ----

int dsg_debug_patch_embed_f32(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj,
                              const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                              const float *Wp, const float *bias, const float *gam, const float *bet, const float *aff, int32_t aff_ld,
                              int32_t aff_off, int32_t aff_off2, float *x, const int32_t *run_list, const int32_t *run_cnt, void *stream) {
    // the kernel gathers (self_cond ? 2 : 1) (c_adj + 2 c_node) channels into Kp / 8 fragments and reads the (scale | shift) rows 16 bytes
    // at a time; a run list addresses 8 consecutive tokens of one row of the grid and comes with its count
    if (B < 1 || N < 1 || c_adj < 1 || c_node < 1 || (Kp != 32 && Kp != 64) || (self_cond ? 2 : 1) * (c_adj + 2 * c_node) > Kp) return DSG_ERR_INVALID;
    if (!adj || !node || !flags || !Wp || !bias || !gam || !bet || !aff || !x) return DSG_ERR_INVALID;
    if (!mult4(aff_ld) || !mult4(aff_off) || (aff_off2 >= 0 && !mult4(aff_off2))) return DSG_ERR_INVALID;
    if (run_list && (!run_cnt || N % 8 != 0)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_fused_patch_embed96(adj, node, sc_adj, sc_node, has_sc, flags, Wp, bias, gam, bet, aff, aff_ld, aff_off, aff_off2, x, B,
                                                   N, c_adj, c_node, self_cond, Kp, s, nullptr, run_list, run_cnt), s);
}

int dsg_debug_assemble_f32(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj, const float *node,
                           const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags, float *out, void *stream) {
    if (B < 1 || N < 1 || c_adj < 1 || c_node < 1 || Kp < (self_cond ? 2 : 1) * (c_adj + 2 * c_node) || !adj || !node || !flags || !out)
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    launch_assemble(adj, node, sc_adj, sc_node, has_sc, flags, out, B, N, c_adj, c_node, self_cond, Kp, s);
    return debug_finish(true, s);
}

int dsg_debug_readout_f32(int32_t B, int32_t N, int32_t c_adj, const float *x, const float *gam, const float *bet, const float *Wfp, const float *fa,
                          const float *W2p, const float *f2, const uint8_t *flags, float *out_adj, float *pool_part, float *pool_ext, void *stream) {
    // the second product's packed weight has 32 output rows: the fold's limit on C_adj (dsg_finalize_weights)
    if (B < 1 || N < 1 || c_adj < 1 || c_adj > 32 || !x || !gam || !bet || !Wfp || !fa || !W2p || !f2 || !flags || !out_adj || !pool_part || !pool_ext)
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    launch_fused_readout96(x, gam, bet, Wfp, fa, W2p, f2, flags, out_adj, pool_part, pool_ext, B, N, c_adj, s, false);
    return debug_finish(true, s);
}

int dsg_debug_head_f32(int32_t kind, int32_t B, int32_t N, int32_t E, int32_t c_out, const float *h, const float *W, const float *bias,
                       const uint8_t *flags, float *out, void *stream) {
    if (B < 1 || N < 1 || E < 1 || !h || !flags || !out || kind < DSG_HEAD_ADJ || kind > DSG_HEAD_NODE) return DSG_ERR_INVALID;
    if (kind != DSG_HEAD_POOL && (c_out < 1 || !W || !bias)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (kind == DSG_HEAD_ADJ) launch_head_adj(h, W, bias, flags, out, B, N, E, c_out, s);
    else if (kind == DSG_HEAD_POOL) launch_pool(h, flags, out, B, N, E, s);
    else launch_head_node(h, W, bias, flags, out, B, N, E, c_out, s);
    return debug_finish(true, s);
}

// ---- the edge kernels of the patch_size > 1 forward (kernels_patch.hip; tests/test_patch_kernels.py) ----

int dsg_debug_assemble_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kp, const float *adj,
                                 const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                                 float *out, void *stream) {
    if ((p != 1 && p != 2 && p != 4) || !adj || !node || !flags || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_assemble_patch(adj, node, sc_adj, sc_node, has_sc, flags, out, B, N, p, c_adj, c_node, self_cond, Kp, s), s);
}

int dsg_debug_head_patch_f32(int32_t kind, int32_t B, int32_t N, int32_t p, int32_t E, int32_t c_out, const float *h, const float *W,
                             const float *bias, const uint8_t *flags, float *out, void *stream) {
    if ((p != 1 && p != 2 && p != 4) || !h || !flags || !out || (kind != DSG_HEAD_ADJ && kind != DSG_HEAD_POOL)) return DSG_ERR_INVALID;
    if (kind == DSG_HEAD_ADJ && (c_out < 1 || !W || !bias)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(kind == DSG_HEAD_ADJ ? launch_head_adj_patch(h, W, bias, flags, out, B, N, p, E, c_out, s)
                                             : launch_pool_patch(h, flags, out, B, N, p, E, s), s);
}

int dsg_debug_patch_embed_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t Kps, const float *adj,
                                    const float *node, const float *sc_adj, const float *sc_node, const int32_t *has_sc, const uint8_t *flags,
                                    const float *Wp, const float *bias, const float *gam, const float *bet, const float *aff, int32_t aff_ld,
                                    int32_t aff_off, int32_t aff_off2, float *x, void *stream) {
    if (p != 2 || !adj || !node || !flags || !Wp || !bias || !gam || !bet || !aff || !x) return DSG_ERR_INVALID;
    if (!mult4(aff_ld) || !mult4(aff_off) || (aff_off2 >= 0 && !mult4(aff_off2))) return DSG_ERR_INVALID;   // 16-byte reads of the (scale | shift) rows
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_fused_patch_embed96_p2(adj, node, sc_adj, sc_node, has_sc, flags, Wp, bias, gam, bet, aff, aff_ld, aff_off, aff_off2, x,
                                                      B, N, c_adj, c_node, self_cond, Kps, s), s);
}

int dsg_debug_readout_patch_f32(int32_t B, int32_t N, int32_t p, int32_t c_adj, const float *x, const float *gam, const float *bet, const float *Wfp,
                                const float *fa, const float *W2p, const float *f2, const uint8_t *flags, float *out_adj, float *pool_part,
                                float *pool_ext, void *stream) {
    if (p != 2 || !x || !gam || !bet || !Wfp || !fa || !W2p || !f2 || !flags || !out_adj || !pool_part || !pool_ext) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_fused_readout96_p2(x, gam, bet, Wfp, fa, W2p, f2, flags, out_adj, pool_part, pool_ext, B, N, c_adj, s), s);
}

int dsg_debug_row_f32(int32_t kind, int32_t B, int32_t t, int32_t C, float *x, const float *g, const float *b, const float *pg, const float *pb,
                      const float *aff, int32_t aff_ld, int32_t aff_off, const float *ln_part, int32_t nparts, float *y, float *stats,
                      const int32_t *run_list, const int32_t *run_cnt, void *stream) {
    // one wave holds a row in 24 registers per lane (ROW_MAXV in kernels.hip): 1536 channels at most, in float4 pieces
    constexpr int ROW_LIMIT = 1536;
    if (B < 1 || t < 1 || C < 4 || C % 4 != 0 || !x) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case DSG_ROW_MOD_STATS:
            if (C > ROW_LIMIT || !aff || !stats || !mult4(aff_ld) || !mult4(aff_off)) return DSG_ERR_INVALID;
            launch_mod_stats(x, aff, aff_ld, aff_off, stats, B, t, C, s);
            break;
        case DSG_ROW_LN_STATS:
            if (C > ROW_LIMIT || !stats) return DSG_ERR_INVALID;
            launch_ln_stats(x, stats, B * t, C, s);
            break;
        case DSG_ROW_LN_MOD:
            if (C > ROW_LIMIT || !g || !b || !aff || !y || aff_ld < 0 || aff_off < 0) return DSG_ERR_INVALID;
            launch_ln_mod(x, g, b, aff, aff_ld, aff_off, y, B, t, C, s);
            break;
        case DSG_ROW_MERGE_LN:      // t = tokens per side of the fine grid; the merged row has 4 C channels
            if (4 * C > ROW_LIMIT || t % 2 != 0 || !g || !b || !y) return DSG_ERR_INVALID;
            launch_merge_ln(x, g, b, y, B, t, C, s, false);
            break;
        case DSG_ROW_BREAKUP_LN:    // t = tokens per side of the coarse grid, C = the row's width D: four chunks of D / 4, each in float4 pieces
            if (C > ROW_LIMIT || C % 16 != 0 || !g || !b || !pg || !pb || !y) return DSG_ERR_INVALID;
            if (run_list && (!run_cnt || (B * t * t) % 8 != 0)) return DSG_ERR_INVALID;
            launch_breakup_ln(x, g, b, pg, pb, y, B, t, C, s, false, run_list, run_cnt);
            break;
        case DSG_ROW_MERGE_NORM_RUNS:   // t = tokens per side of the fine grid; a run is 8 merged rows of one row of the merged grid
            if (t % 16 != 0 || !ln_part || nparts < 1 || !y || !run_list || !run_cnt) return DSG_ERR_INVALID;
            launch_merge_norm_runs(x, ln_part, nparts, y, B, t, C, run_list, run_cnt, s);
            break;
        default: return DSG_ERR_INVALID;
    }
    return debug_finish(true, s);
}

// the row passes' bf16-tensor forms (the fp32 forms: dsg_debug_row_f32 above, dsg_debug_window_attn_f32)
int dsg_debug_row_lp(int32_t kind, int32_t B, int32_t t, int32_t C, float *x, const float *g, const float *b, const float *pg, const float *pb,
                     const float *aff, int32_t aff_ld, int32_t aff_off, void *y, const int32_t *run_list, const int32_t *run_cnt, void *stream) {
    constexpr int ROW_LIMIT = 1536;   // as dsg_debug_row_f32: a wave holds 24 values per lane
    if (B < 1 || t < 1 || C < 4 || C % 4 != 0 || !x || !y) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case DSG_ROWLP_MERGE_LN:
            if (4 * C > ROW_LIMIT || t % 2 != 0 || !g || !b) return DSG_ERR_INVALID;
            launch_merge_ln(x, g, b, static_cast<float *>(y), B, t, C, s, true);
            break;
        case DSG_ROWLP_BREAKUP_LN:
            if (C > ROW_LIMIT || C % 16 != 0 || !g || !b || !pg || !pb) return DSG_ERR_INVALID;
            if (run_list && (!run_cnt || (B * t * t) % 8 != 0)) return DSG_ERR_INVALID;
            launch_breakup_ln(x, g, b, pg, pb, static_cast<float *>(y), B, t, C, s, true, run_list, run_cnt);
            break;
        case DSG_ROWLP_LN_BX:
        case DSG_ROWLP_COPY_BX:
            if (C > ROW_LIMIT || (aff && (!mult4(aff_ld) || !mult4(aff_off)))) return DSG_ERR_INVALID;
            launch_ln_bx(x, aff, aff_ld, aff_off, y, B, t, C, kind == DSG_ROWLP_LN_BX, s);
            break;
        default: return DSG_ERR_INVALID;
    }
    return debug_finish(true, s);
}

int dsg_debug_window_attn_lp(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const void *qkv, const float *biasT, void *out,
                             int32_t in_bf16, int32_t out_bf16, void *stream) {
    if (B < 1 || res < 1 || ws < 1 || heads < 1 || shift < 0 || shift >= ws || !qkv || !biasT || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_finish(launch_window_attn(static_cast<const float *>(qkv), biasT, static_cast<float *>(out), B, WinGeom{res, ws, shift, heads, 32 * heads}, s,
                                           out_bf16 != 0, in_bf16 != 0), s);
}

int dsg_debug_window_broadcast_f32(int32_t B, int32_t res, int32_t C, float *x, float *skip, float *stats, int32_t nparts, const int32_t *copy_list,
                                   const int32_t *copy_cnt, const int32_t *rep, const float *tab_base, int32_t tab_entries, int64_t tab_stride,
                                   int32_t off_x, int32_t off_skip, int32_t off_st, int32_t mode, int32_t step, int32_t n_steps,
                                   const int32_t *sched, void *stream) {
    // windows of 8 x 8 tokens, rows in float4 pieces, statistics in float2 pairs
    if (B < 1 || res < 8 || res % 8 != 0 || C < 4 || C % 4 != 0 || !x || !copy_list || !copy_cnt || (stats && nparts < 1)) return DSG_ERR_INVALID;
    if (mode < DD_OFF || mode > DD_TABLE || (mode == DD_TABLE && !tab_base) || (mode != DD_TABLE && !rep)) return DSG_ERR_INVALID;
    if (tab_base && (tab_entries < 1 || n_steps < 1 || !sched || tab_stride < 0 || tab_stride % 4 != 0 || !mult4(off_x) || !mult4(off_skip) ||
                     off_st < 0 || off_st % 2 != 0))
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    PureTabSrc tab;
    Scratch sc;
    if (tab_base) {   // the small device records the kernel reads: tab.steps[].sched, tab.ctl->step / n_steps, *tab.mode
        std::vector<StepRow> rows((size_t)n_steps);
        for (int i = 0; i < n_steps; i++) { rows[i] = StepRow{0.f, 0.f, 0.f, 0.f, 0.f, sched[i], 0.f, 0}; }
        RunCtl ctl{step, n_steps, 0ull, nullptr, nullptr, nullptr};
        StepRow *d_steps = static_cast<StepRow *>(sc.get(sizeof(StepRow) * rows.size()));
        RunCtl *d_ctl = static_cast<RunCtl *>(sc.get(sizeof(RunCtl)));
        int *d_mode = static_cast<int *>(sc.get(sizeof(int)));
        if (!sc.ok || hipMemcpy(d_steps, rows.data(), sizeof(StepRow) * rows.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_ctl, &ctl, sizeof(RunCtl), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_mode, &mode, sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return DSG_ERR_HIP;
        tab.base = tab_base; tab.stride = (size_t)tab_stride; tab.entries = tab_entries;
        tab.off_x = off_x; tab.off_skip = off_skip; tab.off_st = off_st;
        tab.steps = d_steps; tab.ctl = d_ctl; tab.mode = d_mode;
    }
    launch_window_broadcast(x, skip, stats, nparts, B, res, C, copy_list, copy_cnt, rep, s, tab);
    return debug_finish(true, s);
}

int dsg_debug_window_harvest_f32(int32_t n, int32_t res, int32_t C, const float *x, const float *skip, const float *stats, int32_t nparts, float *dst,
                                 int64_t stride, int32_t off_x, int32_t off_skip, int32_t off_st, void *stream) {
    if (n < 1 || res < 8 || res % 8 != 0 || C < 4 || C % 4 != 0 || !x || !dst || (stats && nparts < 1)) return DSG_ERR_INVALID;
    if (stride < 0 || stride % 4 != 0 || !mult4(off_x) || (skip && !mult4(off_skip)) || (stats && (off_st < 0 || off_st % 2 != 0))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    launch_window_harvest(x, skip, stats, nparts, n, res, C, dst, (size_t)stride, off_x, off_skip, off_st, s);
    return debug_finish(true, s);
}

// ---- the training kernels on their own (test hooks, csrc/train_kernels.hip): no handle, device pointers, one call of the launcher,
// then the stream is synchronised; a form the launcher refuses (it marks the stream's scratch) is DSG_ERR_INVALID, a HIP error
// DSG_ERR_HIP ----
static int debug_t_finish(bool built, hipStream_t s) {
    const hipError_t e = hipStreamSynchronize(s), le = hipGetLastError();
    const bool refused = t_scratch_failed(s, true);
    if (e != hipSuccess || le != hipSuccess) return DSG_ERR_HIP;
    return (built && !refused) ? DSG_OK : DSG_ERR_INVALID;
}

int dsg_debug_t_gemm(int32_t ta, int32_t tb, const float *A, int32_t lda, const float *B, int32_t ldb, const float *bias, float *C, int32_t ldc,
                     int32_t M, int32_t N, int32_t K, int32_t accumulate, float *a_colsum, const float *res, int32_t act, float *c2,
                     int32_t force_plain, int32_t *route_out, void *stream) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1 || lda < 1 || ldb < 1 || ldc < N) return DSG_ERR_INVALID;
    if (act != ACT_NONE && act != ACT_GELU_KEEP && act != ACT_DGELU) return DSG_ERR_INVALID;
    if ((act == ACT_GELU_KEEP && !c2) || (act == ACT_DGELU && !res) || (a_colsum && !(ta && !tb))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int route[2] = {0, 0};
    t_gemm(ta != 0, tb != 0, A, lda, B, ldb, bias, C, ldc, M, N, K, accumulate != 0, s, a_colsum, res, act, c2, route, force_plain != 0 ? 1 : 0);
    if (route_out) { route_out[0] = route[0]; route_out[1] = route[1]; }
    return debug_t_finish(true, s);
}

int dsg_debug_t_cast_lp(const float *W, int32_t R, int32_t Cc, uint16_t *out_nk, uint16_t *out_kn, void *stream) {
    if (!W || R < 1 || Cc < 1 || (!out_nk && !out_kn)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    TCastGroup g;
    t_cast_lp_add(g, W, out_nk, out_kn, R, Cc);
    t_cast_lp(g, s);
    return debug_t_finish(true, s);
}

int dsg_debug_t_gemm_lp(int32_t ta, int32_t tb, const float *A, int32_t lda, const float *B, int32_t ldb, const float *bias, float *C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, float *a_colsum, const float *res, int32_t act,
                        float *c2, int32_t any_rows, int32_t *route_out, void *stream) {
    if (route_out) { route_out[0] = 0; route_out[1] = 0; }
    if (!A || !B || !C || M < 1 || N < 1 || K < 1 || lda < 1 || ldb < 1 || ldc < N) return DSG_ERR_INVALID;
    if (act != ACT_NONE && act != ACT_GELU_KEEP && act != ACT_DGELU) return DSG_ERR_INVALID;
    if ((act == ACT_GELU_KEEP && !c2) || (act == ACT_DGELU && !res) || (a_colsum && !(ta && !tb))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    TrainLp lp;
    lp.any_rows = any_rows != 0; lp.only = true;
    void *planes = nullptr;
    // the weight planes of an activation-side product whose weight is contiguous (anything else the route refuses below)
    if (!ta && ldb == (tb ? K : N) && (size_t)N * K <= ((size_t)32 << 20)) {
        const size_t n = (size_t)N * K;
        if (hipMalloc(&planes, 2 * n * sizeof(uint16_t)) != hipSuccess) return DSG_ERR_HIP;
        uint16_t *nk = static_cast<uint16_t *>(planes), *kn = nk + n;
        TCastGroup g;
        t_cast_lp_add(g, B, nk, kn, tb ? N : K, tb ? K : N);   // B as stored: [N, K] (tb) or [K, N]
        t_cast_lp(g, s);
        lp.planes[B] = TLpPlane{nk, kn};
    }
    int route[2] = {0, 0};
    t_gemm(ta != 0, tb != 0, A, lda, B, ldb, bias, C, ldc, M, N, K, accumulate != 0, s, a_colsum, res, act, c2, route, 0, &lp);
    if (route_out) { route_out[0] = route[0]; route_out[1] = route[1]; }
    const int rc = debug_t_finish(route[0] != 0, s);
    if (planes) (void)hipFree(planes);
    return rc;
}

int dsg_debug_t_attn(int32_t bwd, int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *table,
                     float *out, const float *d_out, float *d_qkv, float *d_table, int32_t force_plain, void *stream) {
    if (B < 1 || ws < 1 || res < ws || res % ws != 0 || ws * ws > 128 || shift < 0 || shift >= ws || heads < 1 || !qkv || !table)
        return DSG_ERR_INVALID;
    if (bwd ? (!d_out || !d_qkv || !d_table) : !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_attn_debug(bwd != 0, qkv, table, out, d_out, d_qkv, d_table, B, res, ws, shift, heads, force_plain != 0, s), s);
}

int dsg_debug_t_ln(int32_t bwd, int32_t M, int32_t C, int32_t T, const float *x, const float *aff, float *y_mod, const float *gamma,
                   const float *beta, float *y, float *stats, const float *dy, const float *dx_in, float *dx_out, float *d_gamma,
                   float *d_beta, void *stream) {
    if (M < 1 || C < 1 || !x || !gamma || !stats) return DSG_ERR_INVALID;
    if (bwd ? (!dy || !dx_out) : (!beta || !y || (aff && (!y_mod || T < 1)))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (bwd) t_ln_bwd(x, gamma, stats, dy, dx_in, dx_out, d_gamma, d_beta, M, C, s);
    else t_ln_fwd_mod(x, aff, y_mod, gamma, beta, y, stats, M, C, aff ? T : 1, s);
    return debug_t_finish(true, s);
}

int dsg_debug_t_modulate(int32_t bwd, int32_t B, int32_t T, int32_t C, const float *x, const float *aff, const float *dy, float *out,
                         float *d_aff, void *stream) {
    if (B < 1 || T < 1 || C < 1 || !x || !aff || !out || (bwd && (!dy || !d_aff))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    t_modulate(x, aff, dy, out, d_aff, B, T, C, bwd != 0, s);
    return debug_t_finish(true, s);
}

int dsg_debug_t_colsum(const float *X, int32_t ld, float *out, int32_t M, int32_t N, void *stream) {
    if (!X || !out || M < 1 || N < 1 || ld < N) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    t_colsum(X, ld, out, M, N, s);
    return debug_t_finish(true, s);
}

int dsg_debug_t_assemble_bwd(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, int32_t self_cond, const float *d_tok, int32_t ld,
                             const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj, const float *g_node,
                             float *out_adj, float *out_node, void *stream) {
    if (!d_tok || !flags || !c_skip || !c_in || !g_adj || !g_node || !out_adj || !out_node) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_assemble_bwd(d_tok, ld, flags, c_skip, c_in, g_adj, g_node, out_adj, out_node, B, N, c_adj, c_node, self_cond != 0, s), s);
}

// ---- the edges of the training form at patch_size > 1 (train_kernels_patch.hip; tests/test_patch_train_kernels.py) ----

int dsg_debug_t_patch_pack(int32_t kind, int32_t unpack, int32_t E, int32_t c_in, int32_t p, int32_t ld, float *W, float *img, const float *bias,
                           float *bias_rep, void *stream) {
    if ((kind != DSG_TPACK_PE && kind != DSG_TPACK_RO0) || !W || !img) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    bool ok;
    if (kind == DSG_TPACK_PE) ok = unpack ? t_pe_unpack(img, W, E, c_in, p, ld, s) : t_pe_pack(W, img, E, c_in, p, ld, s);
    else ok = unpack ? t_ro0_unpack(img, W, E, c_in, p, s) : t_ro0_pack(W, bias, img, bias && bias_rep ? bias_rep : nullptr, E, c_in, p, s);
    return debug_t_finish(ok, s);
}

int dsg_debug_t_adj_out_patch(int32_t bwd, int32_t B, int32_t N, int32_t p, int32_t c_adj, const float *oa, const uint8_t *flags, float *F,
                              const float *dF, float *d_oa, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_adj_out_patch(oa, flags, F, dF, d_oa, B, N, p, c_adj, bwd != 0, s), s);
}

int dsg_debug_t_pool_bwd_patch(int32_t B, int32_t N, int32_t p, int32_t E, const float *d_pool, const uint8_t *flags, float *d_rep_acc,
                               void *stream) {
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_pool_bwd_patch(d_pool, flags, d_rep_acc, B, N, p, E, s), s);
}

int dsg_debug_t_live_cols_patch(int32_t E, int32_t c_adj, int32_t c_node, int32_t self_cond, int32_t p, const float *W, float *img,
                                int32_t *ld_out, void *stream) {
    if (c_adj < 1 || c_node < 1 || (p != 1 && p != 2 && p != 4)) return DSG_ERR_INVALID;
    if (ld_out) *ld_out = t_live_cols_patch_width(c_adj, c_node, p);
    if (!img) return DSG_OK;
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_live_cols_patch(W, (self_cond ? 2 : 1) * (c_adj + 2 * c_node), p, img, E, c_adj, c_node, self_cond != 0, s), s);
}

int dsg_debug_t_assemble_bwd_patch(int32_t B, int32_t N, int32_t p, int32_t c_adj, int32_t c_node, const float *d_tok, int32_t ld,
                                   const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj, const float *g_node,
                                   float *out_adj, float *out_node, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    return debug_t_finish(t_assemble_bwd_patch(d_tok, ld, flags, c_skip, c_in, g_adj, g_node, out_adj, out_node, B, N, p, c_adj, c_node, s), s);
}

int dsg_debug_t_grouped(int32_t kind, int32_t n, const dsg_t_prob *probs, float *out, int32_t n_out, void *stream) {
    if (n < 1 || n > T_GROUP_MAX || !probs || kind < DSG_TGROUP_NT || kind > DSG_TGROUP_TT) return DSG_ERR_INVALID;
    TGemmGroup g;
    g.n = n;
    for (int z = 0; z < n; z++) {
        const dsg_t_prob &p = probs[z];
        if (p.M < 1 || p.N < 1 || !p.C) return DSG_ERR_INVALID;
        if (kind != DSG_TGROUP_SUM && !p.A) return DSG_ERR_INVALID;
        if (kind != DSG_TGROUP_SUM && kind != DSG_TGROUP_COLSUM && (!p.B || p.K < 1)) return DSG_ERR_INVALID;
        if (kind == DSG_TGROUP_NN_SUM && (p.M != probs[0].M || p.N != probs[0].N)) return DSG_ERR_INVALID;
        g.p[z] = TGemmProb{p.A, p.B, p.bias, p.C, p.lda, p.ldb, p.ldc, p.M, p.N, p.K};
    }
    hipStream_t s = (hipStream_t)stream;
    if (kind == DSG_TGROUP_SUM) {
        if (!out || n_out < 1) return DSG_ERR_INVALID;
        t_sum_grouped(g, out, n_out, s);
    } else if (kind == DSG_TGROUP_COLSUM) t_colsum_grouped(g, s);
    else t_gemm_grouped(kind == DSG_TGROUP_TN || kind == DSG_TGROUP_TT, kind == DSG_TGROUP_NT || kind == DSG_TGROUP_TT, kind == DSG_TGROUP_NN_SUM, g, s);
    return debug_t_finish(true, s);
}
int dsg_debug_graph_dot(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *a_adj, const float *a_node, const float *b_adj,
                        const float *b_node, const uint8_t *flags, double *out, void *stream) {
    if (!a_adj || !a_node || !b_adj || !b_node || !flags || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (!t_graph_dot(a_adj, a_node, b_adj, b_node, flags, out, B, N, c_adj, c_node, s)) return DSG_ERR_INVALID;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return DSG_ERR_HIP;
    return DSG_OK;
}
// ---- the bf16 block pipeline's kernels on their own (kernels_bx.hip): fp32 operands are rounded to bf16 into scratch on the way in ----
static float time_launches(hipStream_t s, int iters, const std::function<void()> &launch) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
    for (int i = 0; i < 3; i++) launch();
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; i++) launch();
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / (float)iters;
}

int dsg_debug_gemm_bx(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias, const float *res, int32_t act,
                      const float *mod, int32_t ln_out, float *out_C, float *out_Cb, float *out_C2b, int32_t time_iters, float *out_ms,
                      void *stream) {
    if (M < 1 || N < 1 || K < 8 || !A || !W || (!out_C && !out_Cb)) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    void *ab = sc.get((size_t)M * K * 2), *wb = sc.get((size_t)N * K * 2), *cb = sc.get((size_t)M * N * 2), *c2b = sc.get((size_t)M * N * 2);
    if (!sc.ok) return DSG_ERR_HIP;
    launch_f32_to_bf16(A, ab, (size_t)M * K, s);
    launch_f32_to_bf16(W, wb, (size_t)N * K, s);
    BxGemm g;
    g.A = ab; g.lda = K; g.K = K; g.M = M; g.N = N; g.W = wb; g.bias = bias; g.act = act;
    if (res) { g.res = res; g.ldres = N; }
    if (out_C) { g.C = out_C; g.ldc = N; }
    if (out_Cb) { g.Cb = cb; g.ldcb = N; g.ln_out = ln_out; }
    if (out_C2b) { g.C2b = c2b; g.ldc2b = N; }
    if (mod) { g.mod_aff = mod; g.mod_ld = 0; g.mod_off = 0; g.mod_T = 1; }
    const bool ok = launch_gemm_bx(g, s);
    if (ok && out_Cb) launch_bf16_to_f32(cb, out_Cb, (size_t)M * N, s);
    if (ok && out_C2b) launch_bf16_to_f32(c2b, out_C2b, (size_t)M * N, s);
    if (ok && time_iters > 0 && out_ms) {   // timing: the residual stream is updated in place like in the forward (C aliases res)
        if (g.res && g.C) { g.C = const_cast<float *>(g.res); g.ldc = g.ldres; }
        *out_ms = time_launches(s, time_iters, [&]() { (void)launch_gemm_bx(g, s); });
        if (getenv("DSG_BX_DBG")) {   // phase clocks of a DSG_BX_EXP=4 build (tools/bx_exp.sh): mean over blocks, per tile
            const int nb = 4096;
            unsigned long long *dbg = nullptr;
            if (hipMalloc((void **)&dbg, sizeof(unsigned long long) * 8 * nb) == hipSuccess) {
                (void)hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * 8 * nb, s);
                g.dbg = dbg;
                (void)launch_gemm_bx(g, s);
                std::vector<unsigned long long> hbuf(8 * nb);
                (void)hipMemcpyAsync(hbuf.data(), dbg, sizeof(unsigned long long) * 8 * nb, hipMemcpyDeviceToHost, s);
                (void)hipStreamSynchronize(s);
                double sum[7] = {0, 0, 0, 0, 0, 0, 0};
                int cnt = 0;
                for (int b = 0; b < nb; b++) if (hbuf[8 * b + 6]) { cnt++; for (int i = 0; i < 7; i++) sum[i] += (double)hbuf[8 * b + i]; }
                if (cnt) {
                    const double tiles = sum[5] / cnt;
                    fprintf(stderr, "   bx phases (kclk per tile, mean of %d blocks, %.1f tiles each): mfma+issue %.2f | barrier1 %.2f | wait+refill %.2f | barrier2 %.2f | "
                                    "epilogue %.2f | block total %.2f kclk\n", cnt, tiles, sum[0] / cnt / tiles / 1e3, sum[1] / cnt / tiles / 1e3, sum[2] / cnt / tiles / 1e3,
                            sum[3] / cnt / tiles / 1e3, sum[4] / cnt / tiles / 1e3, sum[6] / cnt / 1e3);
                }
                (void)hipFree(dbg);
                g.dbg = nullptr;
            }
        }
    }
    return debug_finish(ok, s);
}

// BxMlp::wide8 of a C = 384 kernel name (DSG_BXK_DEFAULT: the LDS-DMA kernel); -1: not one
static int mlp384_wide8(int32_t kernel) {
    const bool dma = kernel == DSG_BXK_DEFAULT || kernel == DSG_BXK_MLP384_DMA;
    return dma ? 1 : kernel == DSG_BXK_MLP384_WAVE ? 0 : kernel == DSG_BXK_MLP384_R3 ? 2 : kernel == DSG_BXK_MLP384_SOLO ? 3 : -1;
}

// the two fused-MLP hooks: `in` is xn, or att with the proj stage (Wp, bp) in front; resident96: C = 96 on mlp96r_bx_kernel
static int mlp_bx_hook(int32_t M, int32_t C, const float *in, const float *Wp, const float *bp, float *x, const float *W1, const float *b1,
                       const float *W2, const float *b2, const float *mod, int32_t out_mode, float *out_xn, int wide8, bool resident96,
                       int32_t time_iters, float *out_ms, hipStream_t s) {
    if (M < 1 || !in || !x || !W1 || !b1 || !W2 || !b2 || (out_mode && !out_xn)) return DSG_ERR_INVALID;
    const size_t nx = (size_t)M * C, nw = (size_t)4 * C * C;
    Scratch sc;
    void *ib = sc.get(nx * 2), *wpb = Wp ? sc.get((size_t)C * C * 2) : nullptr, *w1b = sc.get(nw * 2), *w2b = sc.get(nw * 2), *ob = sc.get(nx * 2);
    if (!sc.ok) return DSG_ERR_HIP;
    launch_f32_to_bf16(in, ib, nx, s);
    if (Wp) launch_f32_to_bf16(Wp, wpb, (size_t)C * C, s);
    launch_f32_to_bf16(W1, w1b, nw, s);
    launch_f32_to_bf16(W2, w2b, nw, s);
    BxMlp g;
    if (Wp) { g.att = ib; g.Wp = wpb; g.bp = bp; } else g.xn = ib;
    g.x = x; g.W1 = w1b; g.b1 = b1; g.W2 = w2b; g.b2 = b2; g.M = M; g.C = C;
    if (out_mode) { g.xn_out = ob; g.out_mode = out_mode; }
    g.wide8 = wide8;
    const bool img384 = C == 384 && (wide8 == 1 || wide8 == 3);
    void *imgb = img384 ? sc.get(mlp384_image_bytes()) : (resident96 ? sc.get(mlp96r_image_bytes()) : nullptr);
    if (!sc.ok) return DSG_ERR_HIP;
    if (img384 && wide8 == 1) { launch_mlp384_images(w1b, w2b, wpb, imgb, s); g.img = imgb; }
    if (img384 && wide8 == 3) { launch_mlp384s_images(w1b, w2b, wpb, imgb, s); g.img2 = imgb; }
    if (resident96) { launch_mlp96r_image(w1b, w2b, wpb, imgb, s); g.img96 = imgb; }
    if (mod) { g.mod_aff = mod; g.mod_ld = 0; g.mod_off = 0; g.mod_T = 1; }
    const bool ok = launch_mlp_bx(g, s);
    if (ok && out_mode) launch_bf16_to_f32(ob, out_xn, nx, s);
    if (ok && time_iters > 0 && out_ms) *out_ms = time_launches(s, time_iters, [&]() { (void)launch_mlp_bx(g, s); });   // (x keeps accumulating: timing only)
    if (ok && Wp && C == 384 && g.wide8 == 1 && getenv("DSG_M384_CLK")) {   // dev measurement: phase clocks of one more launch (tools/bx_bench.py)
        const int nb = (M + 127) / 128;
        unsigned long long *dbg = nullptr;
        if (hipMalloc((void **)&dbg, sizeof(unsigned long long) * nb * 128) == hipSuccess) {
            (void)hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * nb * 128, s);
            g.dbg = dbg;
            (void)launch_mlp_bx(g, s);
            std::vector<unsigned long long> hb((size_t)nb * 128);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(hb.data(), dbg, sizeof(unsigned long long) * hb.size(), hipMemcpyDeviceToHost);
            double ph[4] = {0, 0, 0, 0}, tot = 0, iv[2][6] = {{0}};
            for (int b = 0; b < nb; b++)
                for (int w = 0; w < 8; w++) {
                    const unsigned long long *t = hb.data() + ((size_t)b * 8 + w) * 16;
                    for (int k = 0; k < 4; k++) ph[k] += (double)(t[k + 1] - t[k]);
                    tot += (double)(t[4] - t[0]);
                    for (int k = 0; k < 6; k++) iv[w >> 2][k] += (double)(t[6 + k] - t[5 + k]);
                }
            const double n = (double)nb * 8;
            fprintf(stderr, "   mlp384d phases (kclk per wave, mean of %d blocks): proj %.1f | LN + exchange %.1f | chunk-pair loop %.1f | epilogue %.1f | block %.1f\n",
                    nb, ph[0] / n / 1e3, ph[1] / n / 1e3, ph[2] / n / 1e3, ph[3] / n / 1e3, tot / n / 1e3);
            for (int tm = 0; tm < 2; tm++)
                fprintf(stderr, "      pair 8, %s half (clk): fc1 %.0f | wait + barrier %.0f | GELU + exchange %.0f | wait + barrier %.0f | fc2 %.0f | wait + barrier %.0f\n",
                        tm ? "second" : "first", iv[tm][0] / (n / 2), iv[tm][1] / (n / 2), iv[tm][2] / (n / 2), iv[tm][3] / (n / 2), iv[tm][4] / (n / 2), iv[tm][5] / (n / 2));
            (void)hipFree(dbg);
            g.dbg = nullptr;
        }
    }
    if (ok && Wp && C == 384 && g.wide8 == 3 && getenv("DSG_M384_CLK")) {   // dev measurement: phase clocks of one more launch of mlp384s_bx_kernel
        const int nb = (M + 127) / 128;
        unsigned long long *dbg = nullptr;
        if (hipMalloc((void **)&dbg, sizeof(unsigned long long) * nb * 128) == hipSuccess) {
            (void)hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * nb * 128, s);
            g.dbg = dbg;
            (void)launch_mlp_bx(g, s);
            std::vector<unsigned long long> hb((size_t)nb * 128);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(hb.data(), dbg, sizeof(unsigned long long) * hb.size(), hipMemcpyDeviceToHost);
            double ph[4] = {0, 0, 0, 0}, tot = 0, iv[3] = {0, 0, 0};
            for (int b = 0; b < nb; b++)
                for (int w = 0; w < 4; w++) {
                    const unsigned long long *t = hb.data() + ((size_t)b * 8 + w) * 16;
                    for (int k = 0; k < 4; k++) ph[k] += (double)(t[k + 1] - t[k]);
                    tot += (double)(t[4] - t[0]);
                    for (int k = 0; k < 3; k++) iv[k] += (double)(t[6 + k] - t[5 + k]);
                }
            const double n = (double)nb * 4;
            fprintf(stderr, "   mlp384s phases (kclk per wave, mean of %d blocks): prologue %.1f | wait %.1f | chunk loop %.1f | epilogue %.1f | block %.1f\n",
                    nb, ph[0] / n / 1e3, ph[1] / n / 1e3, ph[2] / n / 1e3, ph[3] / n / 1e3, tot / n / 1e3);
            fprintf(stderr, "      chunk 8 (clk): wait + barrier %.0f | fc1(c+1) + GELU(c) %.0f | fc2(c) %.0f\n", iv[0] / n, iv[1] / n, iv[2] / n);
            (void)hipFree(dbg);
            g.dbg = nullptr;
        }
    }
    return debug_finish(ok, s);
}

int dsg_debug_mlp_bx(int32_t M, int32_t C, const float *xn, float *x, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *mod, int32_t out_mode, float *out_xn, int32_t kernel, int32_t time_iters, float *out_ms, void *stream) {
    const int wide8 = mlp384_wide8(kernel);
    if (wide8 < 0 || (kernel != DSG_BXK_DEFAULT && C != 384)) return DSG_ERR_INVALID;
    return mlp_bx_hook(M, C, xn, nullptr, nullptr, x, W1, b1, W2, b2, mod, out_mode, out_xn, wide8, false, time_iters, out_ms, (hipStream_t)stream);
}

int dsg_debug_projmlp_bx(int32_t M, int32_t C, const float *att, float *x, const float *Wp, const float *bp, const float *W1, const float *b1,
                         const float *W2, const float *b2, const float *mod, int32_t out_mode, float *out_xn, int32_t kernel,
                         int32_t time_iters, float *out_ms, void *stream) {
    const bool k96 = kernel == DSG_BXK_MLP96_STAGED || kernel == DSG_BXK_MLP96_RESIDENT, resident96 = kernel == DSG_BXK_MLP96_RESIDENT;
    const int wide8 = k96 ? 1 : mlp384_wide8(kernel);   // the proj form has no one-wave-per-SIMD kernel at C = 384
    if (wide8 < 1 || (k96 ? C != 96 : (kernel != DSG_BXK_DEFAULT && C != 384)) || (resident96 && mod) || !Wp || !bp) return DSG_ERR_INVALID;
    return mlp_bx_hook(M, C, att, Wp, bp, x, W1, b1, W2, b2, mod, out_mode, out_xn, wide8, resident96, time_iters, out_ms, (hipStream_t)stream);
}

// ---- the same kernels on the caller's own bf16 tensors: every field of the launcher's argument block, no scratch in between ----
int dsg_debug_gemm_bx_args(const dsg_bx_gemm_args *a, void *stream) {
    if (a && a->geo_used) *a->geo_used = -1;
    if (!a || !a->A || !a->W || (!a->C && !a->Cb)) return DSG_ERR_INVALID;
    // what the kernel takes on trust from the forward: pitches that hold a row, 16-byte aligned (scale | shift) rows, a sample length
    const int K1 = a->A2 ? a->K1 : a->K;
    if (a->M < 1 || a->N < 1 || a->K < 1 || a->lda < K1 || (a->A2 && (K1 < 1 || K1 >= a->K || a->lda2 < a->K - K1))) return DSG_ERR_INVALID;
    if ((a->C && a->ldc < a->N) || (a->Cb && a->ldcb < a->N) || (a->C2b && a->ldc2b < a->N) || (a->res && a->ldres < a->N)) return DSG_ERR_INVALID;
    if ((a->C && a->ldc % 4 != 0) || (a->res && a->ldres % 4 != 0)) return DSG_ERR_INVALID;
    if (a->mod_aff && (!mult4(a->mod_ld) || !mult4(a->mod_off) || a->mod_T < 1 || (a->mod_ld && a->mod_ld < a->mod_off + 2 * a->N))) return DSG_ERR_INVALID;
    BxGemm g;
    g.A = a->A; g.lda = a->lda; g.A2 = a->A2; g.lda2 = a->lda2; g.K1 = a->K1; g.W = a->W; g.bias = a->bias;
    g.res = a->res; g.ldres = a->ldres; g.C = a->C; g.ldc = a->ldc; g.Cb = a->Cb; g.ldcb = a->ldcb; g.C2b = a->C2b; g.ldc2b = a->ldc2b;
    g.M = a->M; g.N = a->N; g.K = a->K; g.act = a->act;
    g.mod_aff = a->mod_aff; g.mod_ld = a->mod_ld; g.mod_off = a->mod_off; g.mod_T = a->mod_T > 0 ? a->mod_T : 1;
    g.ln_out = a->ln_out;
    const int geo = bx_gemm_geo(g);
    if (geo < 0) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const bool ok = launch_gemm_bx(g, s);
    if (ok && a->geo_used) *a->geo_used = geo;
    return debug_finish(ok, s);
}

int dsg_debug_mlp_bx_args(const dsg_bx_mlp_args *a, void *stream) {
    if (!a || (!a->xn && !a->att) || (a->xn && a->att) || !a->x || !a->W1 || !a->b1 || !a->W2 || !a->b2 || a->M < 1) return DSG_ERR_INVALID;
    if (a->out_mode < 0 || a->out_mode > 2 || (a->out_mode && !a->xn_out)) return DSG_ERR_INVALID;
    const bool proj = a->att != nullptr;
    const int32_t C = a->C, kernel = a->kernel;
    if (C != 96 && C != 192 && C != 384) return DSG_ERR_INVALID;
    int wide8;
    bool resident96 = false;
    if (!proj) {   // dsg_debug_mlp_bx's rule
        wide8 = mlp384_wide8(kernel);
        if (wide8 < 0 || (kernel != DSG_BXK_DEFAULT && C != 384)) return DSG_ERR_INVALID;
    } else {       // dsg_debug_projmlp_bx's rule
        const bool k96 = kernel == DSG_BXK_MLP96_STAGED || kernel == DSG_BXK_MLP96_RESIDENT;
        resident96 = kernel == DSG_BXK_MLP96_RESIDENT;
        wide8 = k96 ? 1 : mlp384_wide8(kernel);
        if (wide8 < 1 || (k96 ? C != 96 : (kernel != DSG_BXK_DEFAULT && C != 384)) || (resident96 && a->mod_aff) || !a->Wp || !a->bp) return DSG_ERR_INVALID;
    }
    if (a->mod_aff && (!mult4(a->mod_ld) || !mult4(a->mod_off) || a->mod_T < 1 || (a->mod_ld && a->mod_ld < a->mod_off + 2 * C))) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    BxMlp g;
    if (proj) { g.att = a->att; g.Wp = a->Wp; g.bp = a->bp; } else g.xn = a->xn;
    g.x = a->x; g.W1 = a->W1; g.b1 = a->b1; g.W2 = a->W2; g.b2 = a->b2; g.M = a->M; g.C = C;
    if (a->out_mode) { g.xn_out = a->xn_out; g.out_mode = a->out_mode; }
    g.wide8 = wide8;
    g.mod_aff = a->mod_aff; g.mod_ld = a->mod_ld; g.mod_off = a->mod_off; g.mod_T = a->mod_T > 0 ? a->mod_T : 1;
    // the weight images of the kernels that stream pre-arranged weights, from the row-major tensors
    Scratch sc;
    const bool img384 = C == 384 && (wide8 == 1 || wide8 == 3);
    void *imgb = img384 ? sc.get(mlp384_image_bytes()) : (resident96 ? sc.get(mlp96r_image_bytes()) : nullptr);
    if (!sc.ok) return DSG_ERR_HIP;
    if (img384 && wide8 == 1) { launch_mlp384_images(a->W1, a->W2, a->Wp, imgb, s); g.img = imgb; }
    if (img384 && wide8 == 3) { launch_mlp384s_images(a->W1, a->W2, a->Wp, imgb, s); g.img2 = imgb; }
    if (resident96) { launch_mlp96r_image(a->W1, a->W2, a->Wp, imgb, s); g.img96 = imgb; }
    return debug_finish(launch_mlp_bx(g, s), s);
}

int dsg_debug_attn_bx(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *qkv, const float *biasT, float *out,
                      int32_t time_iters, float *out_ms, void *stream) {
    if (B < 1 || res < 1 || ws < 1 || res % ws != 0 || heads < 1 || !qkv || !biasT || !out) return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int C = 32 * heads;
    const size_t M = (size_t)B * res * res;
    Scratch sc;
    void *qb = sc.get(M * 3 * C * 2), *ob = sc.get(M * C * 2);
    if (!sc.ok) return DSG_ERR_HIP;
    launch_f32_to_bf16(qkv, qb, M * 3 * C, s);
    const bool ok = launch_attn_bx(qb, biasT, ob, B, WinGeom{res, ws, shift, heads, C}, s);
    if (ok) launch_bf16_to_f32(ob, out, M * C, s);
    if (ok && time_iters > 0 && out_ms)
        *out_ms = time_launches(s, time_iters, [&]() { (void)launch_attn_bx(qb, biasT, ob, B, WinGeom{res, ws, shift, heads, C}, s); });
    return debug_finish(ok, s);
}

int dsg_debug_qkv_attn_bx(int32_t B, int32_t res, int32_t ws, int32_t shift, int32_t heads, const float *xn, const float *W, const float *bias,
                          const float *biasT, float *out, int32_t kernel, int32_t time_iters, float *out_ms, void *stream) {
    if (B < 1 || res < 1 || ws < 1 || res % ws != 0 || heads < 1 || !xn || !W || !bias || !biasT || !out) return DSG_ERR_INVALID;
    if (kernel != DSG_BXK_DEFAULT && ((kernel != DSG_BXK_QA10_WAVE && kernel != DSG_BXK_QA10_HEAD) || ws != 10)) return DSG_ERR_INVALID;
    const int variant = kernel == DSG_BXK_QA10_HEAD ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const int C = 32 * heads, Wp = (ws * ws + 31) / 32 * 32, nW = (res / ws) * (res / ws), nWt = shift > 0 ? nW : 1;
    const size_t M = (size_t)B * res * res, nb = (size_t)nWt * heads * Wp * Wp;
    const bool wave = ws == 10 && variant == 0;   // the wave-per-unit kernel streams an image of W and reads the bias table as fp32
    Scratch sc;
    void *xb = sc.get(M * C * 2), *wb = sc.get((size_t)3 * C * C * 2), *ob = sc.get(M * C * 2), *bp = sc.get(nb * 2);
    if (!sc.ok) return DSG_ERR_HIP;
    launch_f32_to_bf16(xn, xb, M * C, s);
    launch_f32_to_bf16(W, wb, (size_t)3 * C * C, s);
    launch_bias_permute_bx(biasT, bp, nWt * heads, Wp, s);
    BxQkvAttn qa;
    qa.xn = xb; qa.W = wb; qa.bias = bias; qa.biasP = bp; qa.out = ob; qa.B = B; qa.g = WinGeom{res, ws, shift, heads, C};
    qa.variant = variant;
    if (wave) {
        void *qimg = sc.get((size_t)3 * C * C * 2);
        float *bfp = static_cast<float *>(sc.get(nb * 4));
        if (!sc.ok) return DSG_ERR_HIP;
        launch_qkv_image(wb, qimg, C, heads, s);
        qa.Wimg = qimg;
        launch_bias_permute_f32(biasT, bfp, nWt * heads, Wp, s);
        qa.biasF = bfp;
    }
    const bool ok = launch_qkv_attn_bx(qa, s);
    if (ok) launch_bf16_to_f32(ob, out, M * C, s);
    if (ok && time_iters > 0 && out_ms) *out_ms = time_launches(s, time_iters, [&]() { (void)launch_qkv_attn_bx(qa, s); });
    if (ok && ws == 10 && variant == 0 && getenv("DSG_WX_CLK")) {   // dev measurement: phase clocks of one more launch of qkv_attn_wx_kernel
        const int nunits = B * nW * heads, nb = (nunits + 3) / 4;
        unsigned long long *dbg = nullptr;
        if (hipMalloc((void **)&dbg, sizeof(unsigned long long) * nb * 32) == hipSuccess) {
            (void)hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * nb * 32, s);
            qa.dbg = dbg;
            (void)launch_qkv_attn_bx(qa, s);
            qa.dbg = nullptr;
            std::vector<unsigned long long> hb((size_t)nb * 32);
            (void)hipStreamSynchronize(s);
            (void)hipMemcpy(hb.data(), dbg, sizeof(unsigned long long) * hb.size(), hipMemcpyDeviceToHost);
            double ph[4] = {0, 0, 0, 0};
            for (int b = 0; b < nb; b++)
                for (int w = 0; w < 4; w++)
                    for (int k = 0; k < 4; k++) ph[k] += (double)(hb[((size_t)b * 4 + w) * 8 + k + 1] - hb[((size_t)b * 4 + w) * 8 + k]);
            const double n = (double)nb * 4;
            fprintf(stderr, "   qkv_attn_wx phases (kclk per wave, mean of %d blocks): setup + first DMA %.1f | K loop %.1f | q/k/v conversion %.1f | attention + stores %.1f\n",
                    nb, ph[0] / n / 1e3, ph[1] / n / 1e3, ph[2] / n / 1e3, ph[3] / n / 1e3);
            (void)hipFree(dbg);
        }
    }
    return debug_finish(ok, s);
}

}  // extern "C"
