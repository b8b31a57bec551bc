// dsg_api.cpp -- host side of libdsg.so: weight registry, the static launch plan of one network
// forward, preconditioning, and the EDM reverse loop.  Implements include/dsg.h and the hooks of include/dsg_debug.h that need a handle.
//
// Reference mapping (R/ = DiffuseSG/):
//   forward plan      R/model/diffusesg/diffusesg.py:739-830
//   preconditioning   R/model/precond/precond.py:65-110, R/runner/objectives/edm.py:122-126
//   reverse loop      R/runner/mcmc_sampler/edm.py:291-445
#include "../../include/dsg_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <unordered_map>
#include <string>
#include <tuple>
#include <vector>

#include "kernels.h"

using namespace dsg;

#define NOISE_EMB 512
// attention scores are formed directly in the exp2 domain: q carries head_dim^-0.5 * log2(e), the bias/mask tables log2(e)
static const double kLog2e = 1.4426950408889634;
static const double kQScale = 0.17677669529663687 * 1.4426950408889634;

namespace {

struct DevTensor {
    float *p = nullptr;
    std::vector<int64_t> shape;
    int64_t numel = 0;
};

struct WSpec {
    std::string key;
    std::vector<int64_t> shape;
    bool is_index = false;  // relative_position_index: int64 constant, validated and dropped
    bool is_mask = false;   // attn_mask: fp32 constant, accepted and dropped (re-derived)
};

struct BlockPlan {
    std::string prefix;
    int lvl, C, res, ws, shift, heads;
    int aff_off;        // offset of this block's (scale,shift) in the concatenated affine output
    float *biasT = nullptr;  // [nWt][heads][Wp][Wp]
    void *biasP = nullptr;   // the same tiles as fp16 in score-accumulator order (qkv_attn_bx_kernel)
    float *biasF = nullptr;  // ... and as fp32 (qkv_attn_wx_kernel: 10 x 10 windows)
    float *w1p = nullptr, *w2p = nullptr;  // fragment-major packed MLP weights (fused_mlp_kernel), narrow levels only
    float *wqp = nullptr, *wpp = nullptr;  // fragment-major packed qkv / proj weights (fused_attn96_kernel), C == 96 only
    float *bqkv_s = nullptr;               // qkv bias with the q part pre-scaled (fused_attn96_kernel)
    // LayerNorm folded into the consuming linear: W' = W.diag(gamma), b' = b + W.beta (the GEMM's A path then only
    // applies (x-mean)*rstd)
    float *qkv_wf = nullptr, *qkv_bf = nullptr, *fc1_wf = nullptr, *fc1_bf = nullptr;
};

// Every device buffer a handle or one of its workspaces owns, with what a forward may assume about it ("what a forward
// may assume about its workspace"); owned_alloc below is the only hipMalloc of such memory.
//   AC_SCRATCH  float / bf16 data that every entry point writes before it reads
//   AC_FINITE   x, y, att, hid, stats: stale rows may be read into lanes whose results are discarded -- finite, not unread
//   AC_STATE    read as an index, a count, a byte mask, a seed or an address: never filled by the test hooks
//   AC_CONST    weights and what is derived from them
enum AllocClass { AC_SCRATCH = 0, AC_FINITE = 1, AC_STATE = 2, AC_CONST = 3 };
struct AllocRec { void *p; size_t bytes; AllocClass cls; };

struct Workspace {
    int B = 0;
    size_t bytes = 0;
    std::vector<AllocRec> allocs;
    // network forward (fixed addresses: the captured graph reads/writes these)
    float *in_adj, *in_node, *sc_adj, *sc_node, *c_noise, *f_adj, *f_node;
    uint8_t *flags;
    int *has_sc;
    // self-conditioning input the next forward_fixed reads: the fixed buffers + device flag above (dsg_denoise, dsg_precond, the
    // forward-only graph), or -- inside a step body of the reverse loop -- the denoised buffer itself / null, with no flag and
    // no copy, so that a captured step body consists of kernel nodes only
    const float *cur_sc_adj = nullptr, *cur_sc_node = nullptr;
    const int *cur_has_sc = nullptr;
    float *pe, *emb0, *emb, *aff, *tok_in, *x, *y, *qkv, *att, *hid, *stats, *pool, *hn, *pool_ext, *pool_part;
    void *xn = nullptr;   // bf16 [B*T, C]: the normalised input of the next QKV / fc1 GEMM (bf16 block pipeline, kernels_bx.hip)
    float *skips[DSG_MAX_LAYERS];
    // sampler state
    float *x_adj, *x_node, *xh_adj, *xh_node, *sig;
    float *d_adj[3], *d_node[3];
    // conditional sampling (dsg_sample_known): the library's own copy of the caller's known tensors and element masks, state layouts;
    // allocated by the first conditioned call at this batch size.  Captured step bodies bake these addresses, never the caller's
    float *kn_adj = nullptr, *kn_node = nullptr;
    uint8_t *km_adj = nullptr, *km_node = nullptr;
    size_t known_bytes = 0;
    // per-graph noise streams (dsg_sample_seeded / dsg_gen_noise_seeded): the library's copy of the caller's graph seeds, [B];
    // allocated by the first seeded call at this batch size.  RunCtl points at it for the length of a seeded run
    unsigned long long *gseeds = nullptr;
    size_t seeds_bytes = 0;
    // box guidance (dsg_sample_guided): what guided step bodies bake -- the parameter block, one shift buffer [B,N,4] per stage plus the
    // previous step's (the multistep solver), the reference norms [B] -- allocated by the first guided call at this batch size; and the
    // run's tables behind the block's pointers (sel, region, the coefficient table [T], the loss trace [L,B]), which grow without
    // touching a captured body
    GuideParams *g_par = nullptr;
    float *g_shift[3] = {nullptr, nullptr, nullptr};
    double *g_ref = nullptr;
    uint8_t *g_sel = nullptr;
    float *g_region = nullptr, *g_coef = nullptr, *g_trace = nullptr;
    int g_coef_cap = 0;
    size_t g_trace_cap = 0;
    uint8_t *g_kinds = nullptr, *g_predk = nullptr;   // the relation term: the given kinds [B,N,N] / the predicate -> kind table
    int g_predk_cap = 0;
    // content guidance (dsg_sample_guided_content): its parameter block and the full-state shift of every slot (adjacency [B,Ca,N,N],
    // label channels: room for [B,N,Cn-4], used as [B,N,Cl] with the row stride Cl of the run), what the launches of the
    // content kernel's grid form hand over [B,CONTENT_STATS_PER_GRAPH], all baked by content-guided bodies; the run's targets and weights and the trace sit
    // behind the block's pointers and grow without touching a captured body.  Counted in guide_bytes
    ContentParams *c_par = nullptr;
    float *c_shift_adj[3] = {nullptr, nullptr, nullptr}, *c_shift_label[3] = {nullptr, nullptr, nullptr};
    double *c_stats = nullptr;
    float *c_tgt = nullptr, *c_trace = nullptr;
    size_t c_tgt_cap = 0, c_trace_cap = 0;
    size_t guide_bytes = 0;
    // batch-uniform noise level (the sampler): every sample shares one (scale,shift) row, taken from a table that
    // dsg_sample computes once for all steps; aff_ld == 0 broadcasts row 0 of `aff`
    bool uniform = false;
    int aff_ld = 0;
    hipGraphExec_t graph = nullptr, graph_uniform = nullptr;
    hipStream_t cap_stream = nullptr;
    // reverse loop: control block (device step counter, seed, recorded-noise pointers) and the captured step bodies, one
    // per (self-cond slot, output slots, Euler/Heun update, coin of stage 1, coin of stage 2, known, multistep D_prev slot) combination
    // that occurs
    RunCtl *ctl = nullptr;
    struct StepBody { hipGraphExec_t exec; int forwards, guide_forwards; };   // network forwards inside: the handle's own, its guide's
    std::map<int, StepBody> step_graphs;   // key -> captured body
    // autoguidance (dsg_attach_guide): set on the GUIDE handle's workspace for the length of a forward it runs inside its main handle's
    // preconditioned call -- the c_in x the main workspace holds, and the main run's step table and control block (one step counter);
    // null: the workspace's own.  Only kernel-only forwards run under them, never the workspace's forward-only graphs
    const float *ext_in_adj = nullptr, *ext_in_node = nullptr;
    const StepRow *ext_step = nullptr;
    const RunCtl *ext_ctl = nullptr;
    long plan_gen = -1;   // h->plan_gen this workspace's launch plan was last validated against (validate_plan)
    // masked-token pruning: the need lists derived from `flags` whenever they are staged (stage_flags), at fixed addresses -- captured
    // graphs read them -- and this batch size's list offsets; cnt [n_lists], cnt_ps [B][n_lists] scratch of the list kernel
    int *need_lists = nullptr, *need_cnt = nullptr, *need_cnt_ps = nullptr;
    int *dd_rep = nullptr;   // pure-window deduplication: every graph's representative pure window (kernels.h), [dd_n][B] behind cnt_ps
    // what this workspace's last forward did at level k: -1 no deduplication, 0 the copy moved rows of x (levels >= 1: and of the skip) only,
    // 1 also their (sum, sumsq) pairs in `stats` (the block left them for its consumer); dsg_debug_dedup_lists / dsg_debug_dedup_level_lists
    int dd_fwd[1 + NEED_MAX_DD_UP] = {-1, -1, -1, -1};
    // option "dedup_qkv": did the last forward launch the level's second block in its switched form (the fused launch plus the projection
    // over qk_runs and the map attention, the device picking one by qk_split_rule)?  dsg_debug_dedup_qkv_lists
    bool qk_fwd[1 + NEED_MAX_DD_UP] = {false, false, false, false};
    int patch_fwd[2] = {-1, -1};   // the form PatchEmbed / the read-out took in the last forward (1 fused kernel, 0 chain; -1: none yet).  dsg_debug_patch_forms
    int ro_fwd = -1;   // the form the last forward's fused read-out took (1 list, 0 positional; -1: none yet).  dsg_debug_readout_tiles
    // what stage_flags last wrote (dedup_stage_mode below): the DedupMode of the lists, the levels whose fill is trimmed (bit k) and the
    // chain depth the trimming was worked out for -- forward_fixed checks that it reaches exactly that depth
    int dd_mode = DD_OFF, dd_trim = 0, dd_depth = 0;
    // the sampler's table of pure-window rows (option "dedup_table", build_pure_table below): one entry per schedule index, tab_pure_cap
    // of them; allocated by the first sampler call that shares one representative across this batch size, grown like the handle's tab_*
    float *tab_pure = nullptr;
    int tab_pure_cap = 0;
    size_t tab_pure_bytes = 0;
    size_t need_ints = 0;
    NeedPlan need;
};

struct Tap { std::string name; float *dst; int64_t cap; };
struct DevBuf { float *p = nullptr; size_t cap = 0; };   // a handle-owned device buffer that only grows (train_buf); cap in floats

// Masked-token pruning (option "prune_masked"): which need list (kernels.h: NeedPlan) every up-path launch takes.  Built once per
// handle from the up path's geometry (build_prune_plan); -1 = no list, the launch computes everything as before.
struct PruneRole { int kind, res, shift, stage, block, list; };   // kind 0 run list / 1 window list; block >= 0: a Swin block of up stage
                                                                  // `stage`; -1: its post_linear (fine rows); -2: its pre_linear / breakup_ln (coarse rows)
struct PrunePlan {
    bool built = false;
    NeedPlan np;                                                     // list_off is filled per workspace (it depends on the batch size)
    int items[NEED_MAX_LISTS] = {};                                  // entries of each list per sample when nothing is masked
    std::vector<int> rows[DSG_MAX_LAYERS], wins[DSG_MAX_LAYERS];     // per up block: run list of its proj / MLP rows, window list of its attention
    int fine[DSG_MAX_LAYERS], coarse[DSG_MAX_LAYERS];                // per up stage's PatchBreakup: post_linear rows, pre_linear / breakup_ln rows
    std::vector<PruneRole> roles;                                    // the same assignment as a flat table (dsg_debug_need_lists)
};

// The kernel-selection options (dsg_set_option): one int32_t per option, named after it, so that one pointer-to-member type serves
// g_options below -- the table that says what each one is, with its default, DSG_* environment default and range (dsg_create fills these)
struct Options {
    int32_t fused_attn, fused_mlp, fused_mlp_maxc, fused_readout, fused_patch_embed, fused_rowstats, fused_qkv_attn, fused_merge, loop_graph,
        prune_masked, dedup_masked, dedup_levels, dedup_batch, dedup_table, dedup_qkv, batch_invariant, gemm_bf16, gemm_split, bf16_act,
        bf16_pipe, bf16_mlp, bf16_qkv_attn, bf16_proj_mlp, bf16_readout, debug_alloc_fill;
};

}  // namespace

struct dsg_handle_s {
    dsg_config cfg;
    int N, Ca, Cn, E, L, Cin, Kp;
    // patch_size (dsg_create_patch) and the level-0 token resolution R0 = N / P: N is the side of the STATE (flags, adjacency, node rows,
    // the read-out's pixel rows), R0 >> l the side of level l's token grid.  P == 1: R0 == N.  Kp pads P * P * Cin
    int P = 1, R0 = 0;
    std::vector<WSpec> specs;
    std::map<std::string, DevTensor> w;
    bool finalized = false;
    bool ever_finalized = false;                                  // block plans exist and every weight has been set at least once (training entries read raw weights only)
    std::string err;
    // first launch of the current forward whose shape / argument combination no kernel covers ("" = none).  Filled by the launch
    // wrappers below instead of terminating the process; validate_plan() walks a whole forward in a dry run (kernels.h: g_dry_run)
    // when a batch size is first used and whenever an option changes, so the entry points return DSG_ERR_INVALID before any work
    // is enqueued or captured
    std::string plan_err;
    long plan_gen = 0;   // bumped by everything that changes which kernels a forward launches (options, weights, debug taps)
    // derived
    std::vector<BlockPlan> down[DSG_MAX_LAYERS], up[DSG_MAX_LAYERS];
    float *aff_w = nullptr, *aff_b = nullptr;  // concatenated affine linears [aff_n, 512]
    int aff_n = 0, pe_aff_off = 0;
    float *pe_w = nullptr;      // patch_embed.proj padded to [E, Kp]
    float *pe_wp = nullptr;     // the same, fragment-major packed [E/32][Kp/8][64][4] (fused_patch_embed96_kernel)
    float *ro0_w = nullptr;     // read_out.0 transposed to [out,in]
    // folded read-out (E = 96): Fa = F1.W2.W1.W0^T packed fragment-major, fa; F2 padded+packed; node: Gext [E,128]
    float *ro_fap = nullptr, *ro_fa = nullptr, *ro_f2p = nullptr, *ro_gext = nullptr;
    // patch_size 2 (E = 96): pe_wp / ro_fap hold the four sub-pixels' fragment packs (launch_fused_patch_embed96_p2 / _readout96_p2), pe_kps the
    // per-sub-pixel K (in_chans rounded up to 32); ro_gext2[a] [E, 256]: the node fc1 weight of node rows of parity a over pool_ext's columns
    // (G1 F[a, 0] | G1 F[a, 1] | G1 c | G1 c | 0 ..)
    float *ro_gext2[2] = {nullptr, nullptr};
    int pe_kps = 0;
    float *ro_fapb = nullptr, *ro_f2pb = nullptr;   // the same two matrices in the bf16 MFMA's fragment order (fp32 here; their bf16 copies are what runs)
    float *ro0_wf = nullptr, *ro0_bf = nullptr;  // read_out.0 ([out,in]) with the final norm's gamma/beta folded in
    float *merge_wf[DSG_MAX_LAYERS] = {}, *merge_bf[DSG_MAX_LAYERS] = {};   // PatchMerging reduction with its LayerNorm(4C) folded in
    std::vector<AllocRec> derived_allocs;   // freed and rebuilt by every dsg_finalize_weights
    std::vector<AllocRec> allocs;           // everything else the handle itself owns (weights and their copies, tab_*, the train_* arenas)
    unsigned long long debug_fill_count = 0;
    std::map<int, std::unique_ptr<Workspace>> ws;
    Options opt{};   // kernel-selection options (dsg_set_option): dsg_create fills them from g_options -- the defaults, overridden once by DSG_* environment variables
    PrunePlan prune;
    int prof_next_list = -1;          // need list of the next profiled launch (its FLOP figure is scaled by the executed share)
    std::vector<int> prof_list;
    int n_cu = 0;                     // multiprocessor count of the device (read once in dsg_create): the list GEMM's form rule (gemm_thin_rule)
    int prof_next_thin_n = 0;         // N of the next profiled launch if it is a list GEMM with a thin form, else 0
    std::vector<int> prof_thin_n;
    const char *prof_next_form = nullptr;   // the form the next profiled launch was given on the host (" form=..." of its [dsg-prof] line), or null
    std::vector<const char *> prof_form;
    // the next profiled launch belongs to a block with the "dedup_qkv" form switch: the qk_runs list whose count decides, the rows M of the
    // rule, and the form the launch is part of (1 fused, 2 split); list -1: no switch
    struct ProfQk { int list = -1, M = 0, role = 0; };
    ProfQk prof_next_qk;
    std::vector<ProfQk> prof_qk;
    std::vector<std::pair<const float *, size_t>> gemm_weights;   // every fp32 GEMM weight (pointer, numel)
    std::map<const float *, void *> w_bf16;                       // bf16 copies, built when the mode is switched on
    std::map<const float *, void *> w_img96;                      // per C = 96 block (key: its fc1_wf): W1 | W2 | Wp in fragment order for mlp96r_bx_kernel
    std::map<const float *, void *> w_qimg;                       // per block (key: its qkv_wf): the QKV weight in qkv_attn_wx_kernel's streaming order
    std::map<const float *, void *> w_img2;                       // the same weights chunk-major for mlp384s_bx_kernel (bf16_mlp = 5)
    std::map<const float *, void *> w_img;                        // per C = 384 block (key: its fc1_wf): W1 | W2 | Wp pre-arranged for mlp384d_bx_kernel's LDS-DMA ring
    std::map<const float *, void *> w_split;                      // [3][N][K] bf16 planes
    // per-step (scale,shift) table of the sampler (batch-uniform sigma): [cap][aff_n] and its staging buffers
    int tab_cap = 0;
    int tab_step_cap = 0;          // rows of tab_step: one per EXECUTED step (a resampling walk has more of them than schedule indices)
    float *tab_sig = nullptr, *tab_cn = nullptr, *tab_pe = nullptr, *tab_e0 = nullptr, *tab_e1 = nullptr, *tab_aff = nullptr;
    StepRow *tab_step = nullptr;   // per-step scalars of the loop, read by the table-driven sampler kernels
    std::vector<Tap> taps;
    // training form (dsg_train_*): saved-activation arena and backward scratch, owned by the handle and kept between calls
    // (hipMalloc / hipFree of ~10 GB per iteration cost more than a tenth of it); they only grow (train_buf).  train_io: the entries'
    // preconditioned inputs, F and dL/dF; train_vjp: d_tok | W_img | coef of dsg_precond_vjp; train_ode: dsg_ode_run's states, probe,
    // gradient, sigma rows, step table and control block
    DevBuf train_arena, train_scr, train_io, train_vjp, train_ode;
    // bf16 mode of the training entries (dsg_train_set_precision): the mode, the bf16 weight planes of the covered linears -- rebuilt by
    // every entry call in bf16 mode, the parameters may have changed in place -- and the route counts of the last training entry
    int train_precision = DSG_TRAIN_F32;
    int train_patch = 0;   // dsg_train_enable_patch: the training form at patch_size > 1 (no effect at patch_size 1)
    DevBuf train_lp;
    std::vector<TLpCount> train_counts;
    int *train_const = nullptr;                                   // device {0, 1}: the "self-conditioning present" switch of launch_assemble
    // dsg_train_bind_params: parameters the training form reads in place (the optimiser's own device tensors) instead of the handle's copies
    std::unordered_map<std::string, const float *> train_params;
    dsg_sample_stats last_stats{};
    // autoguidance (dsg_attach_guide): the guide handle of this one with its scale s (guide_sm1 = s - 1 in float32) and
    // noise-level interval; guide_of: the handle this one guides.  At most one of the two is set (a guide has no guide)
    dsg_handle guide = nullptr, guide_of = nullptr;
    float guide_scale = 1.f, guide_sm1 = 0.f, guide_lo = 0.f, guide_hi = 0.f;
    int64_t last_guide_forwards = 0;   // the guide's network forwards in the last dsg_sample* call (dsg_guide_forwards)
    int device = -1;                   // the HIP device current at dsg_create
    // per-kernel-class timing (dsg_profile_forward): HIP events bracketing every launch on the launch stream
    bool prof_on = false;          // HIP-event brackets around every launch
    bool prof_stamps = false;      // in-kernel start/end stamps of the GEMM launches (no events: launches stay back to back)
    std::vector<hipEvent_t> prof_events;
    size_t prof_used = 0;
    std::vector<int> prof_kind;
    std::vector<double> prof_flops;
    std::vector<std::string> prof_tag;
    // in-kernel stamps of the dominant kernel (GEMM): one {start,end} pair per launch
    unsigned long long *prof_gemm = nullptr;
    int prof_gemm_cap = 0, prof_gemm_used = 0;
    double prof_clock_ghz = 0.0;   // median over the GEMM launches of the last dsg_profile_forward: shader clock held by block 0
};

namespace {

int fail(dsg_handle h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

// a launcher declined its arguments: remember the first one of this forward (layer / shape in the message)
void plan_fail(dsg_handle h, const char *fmt, ...) {
    if (!h->plan_err.empty()) return;
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    h->plan_err = buf;
}

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(h, DSG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

enum ProfKind { PK_GEMM = 0, PK_ATTN = 1, PK_ROW = 2, PK_ELEM = 3, PK_FUSED = 4, PK_COUNT = 5 };

struct ProfScope {
    dsg_handle h; hipStream_t s;
    ProfScope(dsg_handle h_, hipStream_t s_, int kind, double flops, const char *tag = nullptr) : h(h_), s(s_) {
        const int need_list = h->prof_next_list, thin_n = h->prof_next_thin_n;
        const auto qk = h->prof_next_qk;
        const char *form = h->prof_next_form;
        h->prof_next_form = nullptr;
        h->prof_next_list = -1;
        h->prof_next_thin_n = 0;
        h->prof_next_qk = decltype(h->prof_next_qk)();
        if (!h->prof_on) return;
        while (h->prof_events.size() < h->prof_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) { h->prof_on = false; return; }
            h->prof_events.push_back(e);
        }
        h->prof_kind.push_back(kind);
        h->prof_list.push_back(need_list);
        h->prof_thin_n.push_back(thin_n);
        h->prof_qk.push_back(qk);
        h->prof_form.push_back(form);
        h->prof_flops.push_back(flops);
        h->prof_tag.push_back(tag ? tag : "");
        (void)hipEventRecord(h->prof_events[h->prof_used], s);
    }
    ~ProfScope() {
        if (!h->prof_on) return;
        (void)hipEventRecord(h->prof_events[h->prof_used + 1], s);
        h->prof_used += 2;
    }
};

// the captured step bodies that run a guide's forwards (StepPlan::autoguide, the key's top bit): dropped on attach, on detach and by
// whatever drops the guide's own graphs
constexpr int STEP_KEY_AUTOGUIDE = 1 << 29;
void drop_guided_bodies(dsg_handle h) {
    for (auto &kv : h->ws) {
        auto &m = kv.second->step_graphs;
        for (auto it = m.begin(); it != m.end();)
            if (it->first & STEP_KEY_AUTOGUIDE) { (void)hipGraphExecDestroy(it->second.exec); it = m.erase(it); } else ++it;
    }
}

// captured graphs bake weight pointers, kernel selection and table addresses: drop them whenever one of those changes
void drop_graphs(dsg_handle h) {
    h->plan_gen++;   // ... and the launch plans are validated again before their next use (validate_plan)
    for (auto &kv : h->ws) {
        Workspace *w = kv.second.get();
        if (w->graph) { (void)hipGraphExecDestroy(w->graph); w->graph = nullptr; }
        if (w->graph_uniform) { (void)hipGraphExecDestroy(w->graph_uniform); w->graph_uniform = nullptr; }
        for (auto &g : w->step_graphs) (void)hipGraphExecDestroy(g.second.exec);
        w->step_graphs.clear();
    }
    if (h->guide_of) drop_guided_bodies(h->guide_of);   // ... and a guide's are baked into its main handle's guided step bodies
}

// (r0: the level-0 token resolution, max_node_num / patch_size)
int level_window(const dsg_config &c, int r0, int lvl) {
    const int r = r0 >> lvl;
    return r <= c.window_size ? r : c.window_size;
}
int block_shift(const dsg_config &c, int r0, int lvl, int j) {
    const int r = r0 >> lvl;
    if (r <= c.window_size) return 0;
    return (j % 2 == 0) ? 0 : c.window_size / 2;
}

void add_block_specs(std::vector<WSpec> &s, const std::string &p, int C, int heads, int ws, int res, int shift, int mr) {
    const int64_t W = (int64_t)ws * ws;
    s.push_back({p + ".affine.weight", {2 * C, NOISE_EMB}});
    s.push_back({p + ".affine.bias", {2 * C}});
    s.push_back({p + ".norm1.weight", {C}});
    s.push_back({p + ".norm1.bias", {C}});
    s.push_back({p + ".attn.relative_position_bias_table", {(2 * ws - 1) * (2 * ws - 1), heads}});
    s.push_back({p + ".attn.relative_position_index", {W, W}, true, false});
    s.push_back({p + ".attn.qkv.weight", {3 * C, C}});
    s.push_back({p + ".attn.qkv.bias", {3 * C}});
    s.push_back({p + ".attn.proj.weight", {C, C}});
    s.push_back({p + ".attn.proj.bias", {C}});
    s.push_back({p + ".norm2.weight", {C}});
    s.push_back({p + ".norm2.bias", {C}});
    s.push_back({p + ".mlp.fc1.weight", {mr * C, C}});
    s.push_back({p + ".mlp.fc1.bias", {mr * C}});
    s.push_back({p + ".mlp.fc2.weight", {C, mr * C}});
    s.push_back({p + ".mlp.fc2.bias", {C}});
    if (shift > 0) {
        const int64_t nW = (int64_t)(res / ws) * (res / ws);
        s.push_back({p + ".attn_mask", {nW, W, W}, false, true});
    }
}

// The key list of DiffuseSG(...).state_dict() (diffusesg.py:587-720), same derivation as diffusesg_amd/spec.py
void build_specs(dsg_handle h) {
    const dsg_config &c = h->cfg;
    const int E = c.embed_dim, L = c.num_layers, mr = c.mlp_ratio;
    auto &s = h->specs;
    s.push_back({"patch_embed.affine.weight", {2 * E, NOISE_EMB}});
    s.push_back({"patch_embed.affine.bias", {2 * E}});
    s.push_back({"patch_embed.proj.weight", {E, h->Cin, h->P, h->P}});
    s.push_back({"patch_embed.proj.bias", {E}});
    s.push_back({"patch_embed.norm.weight", {E}});
    s.push_back({"patch_embed.norm.bias", {E}});
    for (int l = 0; l < L; l++) {
        const int C = E << l, res = h->R0 >> l, ws = level_window(c, h->R0, l);
        for (int j = 0; j < c.depths[l]; j++)
            add_block_specs(s, "down_layers." + std::to_string(l) + ".blocks." + std::to_string(j), C, c.num_heads[l], ws, res,
                            block_shift(c, h->R0, l, j), mr);
        if (l < L - 1) {
            const std::string p = "down_layers." + std::to_string(l) + ".downsample";
            s.push_back({p + ".reduction.weight", {2 * C, 4 * C}});
            s.push_back({p + ".norm.weight", {4 * C}});
            s.push_back({p + ".norm.bias", {4 * C}});
        }
    }
    for (int i = 0; i < L; i++) {
        const int l = L - 1 - i;
        const int C = E << l, res = h->R0 >> l, ws = level_window(c, h->R0, l);
        if (i > 0) {
            const int D = 4 * C;
            const std::string p = "up_layers." + std::to_string(i) + ".upsample";
            s.push_back({p + ".pre_linear.weight", {D, D}});
            s.push_back({p + ".norm.weight", {D}});
            s.push_back({p + ".norm.bias", {D}});
            s.push_back({p + ".post_linear.weight", {D / 4, D / 4}});
            s.push_back({p + ".post_norm.weight", {D / 4}});
            s.push_back({p + ".post_norm.bias", {D / 4}});
        }
        for (int j = 0; j < c.depths[l]; j++)
            add_block_specs(s, "up_layers." + std::to_string(i) + ".blocks." + std::to_string(j), C, c.num_heads[l], ws, res,
                            block_shift(c, h->R0, l, j), mr);
    }
    for (int k = 0; k < 3; k++) {
        const int ps = k == 0 ? h->P : 1;   // read_out.0 is the ConvTranspose2d(E, E, p, p)
        s.push_back({"read_out." + std::to_string(k) + ".weight", {E, E, ps, ps}});
        s.push_back({"read_out." + std::to_string(k) + ".bias", {E}});
    }
    s.push_back({"map_layer0.weight", {NOISE_EMB, E}});
    s.push_back({"map_layer0.bias", {NOISE_EMB}});
    s.push_back({"map_layer1.weight", {NOISE_EMB, NOISE_EMB}});
    s.push_back({"map_layer1.bias", {NOISE_EMB}});
    s.push_back({"norm.weight", {E}});
    s.push_back({"norm.bias", {E}});
    s.push_back({"readout_adj_mlp.fc1.weight", {E, E}});
    s.push_back({"readout_adj_mlp.fc1.bias", {E}});
    s.push_back({"readout_adj_mlp.fc2.weight", {c.c_adj, E}});
    s.push_back({"readout_adj_mlp.fc2.bias", {c.c_adj}});
    s.push_back({"readout_node_mlp.fc1.weight", {E, E}});
    s.push_back({"readout_node_mlp.fc1.bias", {E}});
    s.push_back({"readout_node_mlp.fc2.weight", {c.c_node, E}});
    s.push_back({"readout_node_mlp.fc2.bias", {c.c_node}});
}

std::string strip_prefix(const char *key) {
    std::string k(key);
    if (k.rfind("module.", 0) == 0) k = k.substr(7);   // DDP wrapper (sampling_utils.py:47-53)
    if (k.rfind("model.", 0) == 0) k = k.substr(6);    // Precond.model (precond.py:15)
    return k;
}

const float *WT(dsg_handle h, const std::string &key) { return h->w.at(key).p; }

// The one hipMalloc of handle- or workspace-owned memory: records pointer, size and class in `pool`.  Under the test option
// "debug_alloc_fill" a scratch buffer starts as that pattern instead of whatever the allocator returned -- ahead of the caller's own
// creation memsets, which therefore stay effective.  The fill runs on the null stream and is waited for: allocations happen outside
// stream capture, before the call's first launch on the caller's stream
int owned_alloc(dsg_handle h, std::vector<AllocRec> &pool, void **p, size_t bytes, AllocClass cls) {
    bytes = bytes ? bytes : 16;
    HIP_TRY(h, hipMalloc(p, bytes));
    pool.push_back(AllocRec{*p, bytes, cls});
    if (h->opt.debug_alloc_fill && (cls == AC_SCRATCH || cls == AC_FINITE)) {
        launch_debug_fill(*p, bytes / 4, h->opt.debug_alloc_fill, 0x5eedull + h->debug_fill_count++, nullptr);
        HIP_TRY(h, hipStreamSynchronize(nullptr));
    }
    return 0;
}
void owned_free(std::vector<AllocRec> &pool, void *p) {
    if (!p) return;
    for (size_t i = 0; i < pool.size(); i++)
        if (pool[i].p == p) { pool.erase(pool.begin() + i); break; }
    (void)hipFree(p);
}
void owned_free_all(std::vector<AllocRec> &pool) {
    for (auto &r : pool) (void)hipFree(r.p);
    pool.clear();
}

// dense, key-major (transposed) bias+mask table of one block: [nWt][heads][Wp][Wp], entry [key][query]
// bias: relative_position_bias_table[index[query][key]][head] (diffusesg.py:121-124)
// mask: 0 / -100 between different shift regions (diffusesg.py:207-226); padded key slots: -1e30
int build_bias_table(dsg_handle h, BlockPlan &bp) {
    const int ws = bp.ws, W = ws * ws, Wp = ((W + 31) / 32) * 32, heads = bp.heads, res = bp.res, shift = bp.shift;
    const int nwr = res / ws, nWt = shift > 0 ? nwr * nwr : 1;
    const DevTensor &tab = h->w.at(bp.prefix + ".attn.relative_position_bias_table");
    std::vector<float> table(tab.numel);
    HIP_TRY(h, hipMemcpy(table.data(), tab.p, sizeof(float) * tab.numel, hipMemcpyDeviceToHost));
    std::vector<float> out((size_t)nWt * heads * Wp * Wp, 0.f);
    for (int w = 0; w < nWt; w++) {
        const int wi = w / nwr, wj = w % nwr;
        std::vector<int> region(W, 0);
        if (shift > 0)
            for (int p = 0; p < W; p++) {
                const int si = wi * ws + p / ws, sj = wj * ws + p % ws;
                const int ri = si < res - ws ? 0 : (si < res - shift ? 1 : 2);
                const int rj = sj < res - ws ? 0 : (sj < res - shift ? 1 : 2);
                region[p] = 3 * ri + rj;
            }
        for (int hd = 0; hd < heads; hd++) {
            float *o = out.data() + ((size_t)w * heads + hd) * Wp * Wp;
            for (int key = 0; key < Wp; key++)
                for (int q = 0; q < Wp; q++) {
                    float v;
                    if (key >= W) v = -1.0e30f;
                    else if (q >= W) v = 0.f;
                    else {
                        const int qi = q / ws, qj = q % ws, ki = key / ws, kj = key % ws;
                        const int idx = (qi - ki + ws - 1) * (2 * ws - 1) + (qj - kj + ws - 1);
                        v = table[(size_t)idx * heads + hd];
                        if (shift > 0 && region[q] != region[key]) v += -100.0f;
                        v = (float)((double)v * kLog2e);
                    }
                    o[(size_t)key * Wp + q] = v;
                }
        }
    }
    void *p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * out.size(), AC_CONST)) return rc;
    HIP_TRY(h, hipMemcpy(p, out.data(), sizeof(float) * out.size(), hipMemcpyHostToDevice));
    bp.biasT = (float *)p;
    void *pp;
    if (int rc = owned_alloc(h, h->derived_allocs, &pp, sizeof(uint16_t) * out.size(), AC_CONST)) return rc;
    launch_bias_permute_bx(bp.biasT, pp, nWt * heads, Wp, nullptr);
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    bp.biasP = pp;
    if (ws == 10) {
        void *pf;
        if (int rc = owned_alloc(h, h->derived_allocs, &pf, sizeof(float) * out.size(), AC_CONST)) return rc;
        launch_bias_permute_f32(bp.biasT, (float *)pf, nWt * heads, Wp, nullptr);
        HIP_TRY(h, hipStreamSynchronize(nullptr));
        bp.biasF = (float *)pf;
    }
    return 0;
}

// Fragment-major packing for fused_mlp_kernel: every MFMA operand fetch becomes one coalesced 1-KiB wave load.
//   W1p[nt][s][lane][t]    = fc1.weight[32nt + (lane&31)][8s + 4(lane>>5) + t]
//   W2p[nt][ct][g][lane][t] = fc2.weight[32ct + (lane&31)][32nt + 8g + 4(lane>>5) + t]
int pack_mlp_weights(dsg_handle h, BlockPlan &bp) {
    const int C = bp.C, Hd = h->cfg.mlp_ratio * C;
    if (!(C == 96 || C == 192) || h->cfg.mlp_ratio != 4) return 0;
    const int S = C / 8, CT = C / 32, NT = Hd / 32;
    std::vector<float> w1((size_t)Hd * C), w2((size_t)C * Hd), p1((size_t)Hd * C), p2((size_t)C * Hd);
    HIP_TRY(h, hipMemcpy(w1.data(), WT(h, bp.prefix + ".mlp.fc1.weight"), sizeof(float) * w1.size(), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(w2.data(), WT(h, bp.prefix + ".mlp.fc2.weight"), sizeof(float) * w2.size(), hipMemcpyDeviceToHost));
    for (int nt = 0; nt < NT; nt++)
        for (int s = 0; s < S; s++)
            for (int lane = 0; lane < 64; lane++)
                for (int t = 0; t < 4; t++)
                    p1[(((size_t)nt * S + s) * 64 + lane) * 4 + t] = w1[(size_t)(32 * nt + (lane & 31)) * C + 8 * s + 4 * (lane >> 5) + t];
    for (int nt = 0; nt < NT; nt++)
        for (int ct = 0; ct < CT; ct++)
            for (int g = 0; g < 4; g++)
                for (int lane = 0; lane < 64; lane++)
                    for (int t = 0; t < 4; t++)
                        p2[((((size_t)nt * CT + ct) * 4 + g) * 64 + lane) * 4 + t] =
                            w2[(size_t)(32 * ct + (lane & 31)) * Hd + 32 * nt + 8 * g + 4 * (lane >> 5) + t];
    void *p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * p1.size(), AC_CONST)) return rc;
    bp.w1p = (float *)p;
    HIP_TRY(h, hipMemcpy(bp.w1p, p1.data(), sizeof(float) * p1.size(), hipMemcpyHostToDevice));
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * p2.size(), AC_CONST)) return rc;
    bp.w2p = (float *)p;
    HIP_TRY(h, hipMemcpy(bp.w2p, p2.data(), sizeof(float) * p2.size(), hipMemcpyHostToDevice));
    return 0;
}

// W' = W.diag(gamma), b' = b + W.beta for a linear that consumes LayerNorm output (W device [N,K], gamma/beta [K])
int fold_ln(dsg_handle h, const float *W, const float *bias, const float *gamma, const float *beta, int N, int K, float **Wf, float **bf,
            int scaled_rows = 0, double row_scale = 1.0) {
    std::vector<float> w((size_t)N * K), b(N, 0.f), g(K), be(K);
    HIP_TRY(h, hipMemcpy(w.data(), W, sizeof(float) * w.size(), hipMemcpyDeviceToHost));
    if (bias) HIP_TRY(h, hipMemcpy(b.data(), bias, sizeof(float) * N, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(g.data(), gamma, sizeof(float) * K, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(be.data(), beta, sizeof(float) * K, hipMemcpyDeviceToHost));
    for (int n = 0; n < N; n++) {
        double acc = b[n];
        const double rs = n < scaled_rows ? row_scale : 1.0;
        for (int k = 0; k < K; k++) { acc += (double)w[(size_t)n * K + k] * be[k]; w[(size_t)n * K + k] = (float)((double)w[(size_t)n * K + k] * g[k] * rs); }
        b[n] = (float)(acc * rs);
    }
    void *p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * w.size(), AC_CONST)) return rc;
    *Wf = (float *)p;
    HIP_TRY(h, hipMemcpy(p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * N, AC_CONST)) return rc;
    *bf = (float *)p;
    HIP_TRY(h, hipMemcpy(p, b.data(), sizeof(float) * N, hipMemcpyHostToDevice));
    return 0;
}

// Fragment-major packing for fused_attn96_kernel (same two patterns as the MLP):
//   Wqp[nt][s][lane][t]     = qkv.weight[32nt + (lane&31)][8s + 4(lane>>5) + t]      nt = {q,k,v} x head
//   Wpp[hd][ct][g][lane][t] = proj.weight[32ct + (lane&31)][32hd + 8g + 4(lane>>5) + t]
int pack_attn_weights(dsg_handle h, BlockPlan &bp) {
    const int C = bp.C;
    if (C != 96 || bp.ws * bp.ws > 64) return 0;
    const int S = C / 8, CT = C / 32, NT = 3 * C / 32, HD = C / 32;
    std::vector<float> wq((size_t)3 * C * C), wp((size_t)C * C), p1(wq.size()), p2(wp.size());
    HIP_TRY(h, hipMemcpy(wq.data(), WT(h, bp.prefix + ".attn.qkv.weight"), sizeof(float) * wq.size(), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(wp.data(), WT(h, bp.prefix + ".attn.proj.weight"), sizeof(float) * wp.size(), hipMemcpyDeviceToHost));
    for (int nt = 0; nt < NT; nt++)
        for (int s = 0; s < S; s++)
            for (int lane = 0; lane < 64; lane++)
                for (int t = 0; t < 4; t++)
                    p1[(((size_t)nt * S + s) * 64 + lane) * 4 + t] =
                        (float)((double)wq[(size_t)(32 * nt + (lane & 31)) * C + 8 * s + 4 * (lane >> 5) + t] * (nt < HD ? kQScale : 1.0));
    std::vector<float> bq((size_t)3 * C);
    HIP_TRY(h, hipMemcpy(bq.data(), WT(h, bp.prefix + ".attn.qkv.bias"), sizeof(float) * bq.size(), hipMemcpyDeviceToHost));
    for (int n = 0; n < C; n++) bq[n] = (float)((double)bq[n] * kQScale);
    for (int hd = 0; hd < HD; hd++)
        for (int ct = 0; ct < CT; ct++)
            for (int g = 0; g < 4; g++)
                for (int lane = 0; lane < 64; lane++)
                    for (int t = 0; t < 4; t++)
                        p2[((((size_t)hd * CT + ct) * 4 + g) * 64 + lane) * 4 + t] =
                            wp[(size_t)(32 * ct + (lane & 31)) * C + 32 * hd + 8 * g + 4 * (lane >> 5) + t];
    void *p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * p1.size(), AC_CONST)) return rc;
    bp.wqp = (float *)p;
    HIP_TRY(h, hipMemcpy(bp.wqp, p1.data(), sizeof(float) * p1.size(), hipMemcpyHostToDevice));
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * p2.size(), AC_CONST)) return rc;
    bp.wpp = (float *)p;
    HIP_TRY(h, hipMemcpy(bp.wpp, p2.data(), sizeof(float) * p2.size(), hipMemcpyHostToDevice));
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * bq.size(), AC_CONST)) return rc;
    bp.bqkv_s = (float *)p;
    HIP_TRY(h, hipMemcpy(bp.bqkv_s, bq.data(), sizeof(float) * bq.size(), hipMemcpyHostToDevice));
    return 0;
}

const void *bf16_of(dsg_handle h, const float *W) {
    if (!h->opt.gemm_bf16) return nullptr;
    auto it = h->w_bf16.find(W);
    return it == h->w_bf16.end() ? nullptr : it->second;
}

int ensure_bf16_weights(dsg_handle h) {
    for (auto &pw : h->gemm_weights) {
        if (h->w_bf16.count(pw.first)) continue;
        void *q;
        if (int rc = owned_alloc(h, h->allocs, &q, pw.second * 2, AC_CONST)) return rc;
        launch_f32_to_bf16(pw.first, q, pw.second, nullptr);
        h->w_bf16[pw.first] = q;
    }
    // the C = 96 blocks' fc1 / fc2 / proj weights in fragment order for the LDS-resident MLP kernel (launch_mlp96r_image)
    if (h->cfg.mlp_ratio == 4)
        for (int l = 0; l < h->L; l++)
            for (auto *vec : {&h->down[l], &h->up[l]})
                for (auto &b : *vec) {
                    if (b.C != 96 || !b.fc1_wf || h->w_img96.count(b.fc1_wf)) continue;
                    const float *w2 = WT(h, b.prefix + ".mlp.fc2.weight"), *wp = WT(h, b.prefix + ".attn.proj.weight");
                    if (!h->w_bf16.count(b.fc1_wf) || !h->w_bf16.count(w2) || !h->w_bf16.count(wp)) continue;
                    void *q;
                    if (int rc = owned_alloc(h, h->allocs, &q, mlp96r_image_bytes(), AC_CONST)) return rc;
                    launch_mlp96r_image(h->w_bf16[b.fc1_wf], h->w_bf16[w2], h->w_bf16[wp], q, nullptr);
                    h->w_img96[b.fc1_wf] = q;
                }
    // every block's QKV weight once more in the fragment order qkv_attn_wx_kernel streams (launch_qkv_image)
    for (int l = 0; l < h->L; l++)
        for (auto *vec : {&h->down[l], &h->up[l]})
            for (auto &b : *vec) {
                if (!b.qkv_wf || b.ws != 10 || h->w_qimg.count(b.qkv_wf) || !h->w_bf16.count(b.qkv_wf)) continue;
                void *q;
                if (int rc = owned_alloc(h, h->allocs, &q, (size_t)3 * b.C * b.C * 2, AC_CONST)) return rc;
                launch_qkv_image(h->w_bf16[b.qkv_wf], q, b.C, b.heads, nullptr);
                h->w_qimg[b.qkv_wf] = q;
            }
    // the C = 384 blocks' fc1 / fc2 / proj weights once more, in the piece order the LDS-DMA MLP kernel streams and reads them
    if (h->cfg.mlp_ratio == 4)
        for (int l = 0; l < h->L; l++)
            for (auto *vec : {&h->down[l], &h->up[l]})
                for (auto &b : *vec) {
                    if (b.C != 384 || !b.fc1_wf || h->w_img.count(b.fc1_wf)) continue;
                    const float *w2 = WT(h, b.prefix + ".mlp.fc2.weight"), *wp = WT(h, b.prefix + ".attn.proj.weight");
                    if (!h->w_bf16.count(b.fc1_wf) || !h->w_bf16.count(w2) || !h->w_bf16.count(wp)) continue;
                    void *q;
                    if (int rc = owned_alloc(h, h->allocs, &q, mlp384_image_bytes(), AC_CONST)) return rc;
                    launch_mlp384_images(h->w_bf16[b.fc1_wf], h->w_bf16[w2], h->w_bf16[wp], q, nullptr);
                    h->w_img[b.fc1_wf] = q;
                    if (int rc = owned_alloc(h, h->allocs, &q, mlp384_image_bytes(), AC_CONST)) return rc;
                    launch_mlp384s_images(h->w_bf16[b.fc1_wf], h->w_bf16[w2], h->w_bf16[wp], q, nullptr);
                    h->w_img2[b.fc1_wf] = q;
                }
    HIP_TRY(h, hipDeviceSynchronize());
    return 0;
}
const void *img_of(dsg_handle h, const float *fc1_wf) {
    auto it = h->w_img.find(fc1_wf);
    return it == h->w_img.end() ? nullptr : it->second;
}
const void *img2_of(dsg_handle h, const float *fc1_wf) {
    auto it = h->w_img2.find(fc1_wf);
    return it == h->w_img2.end() ? nullptr : it->second;
}

const void *split_of(dsg_handle h, const float *W) {
    if (!h->opt.gemm_split) return nullptr;
    auto it = h->w_split.find(W);
    return it == h->w_split.end() ? nullptr : it->second;
}

int ensure_split_weights(dsg_handle h) {
    for (auto &pw : h->gemm_weights) {
        if (h->w_split.count(pw.first)) continue;
        void *q;
        if (int rc = owned_alloc(h, h->allocs, &q, pw.second * 6, AC_CONST)) return rc;
        launch_f32_split3(pw.first, q, pw.second, nullptr);
        h->w_split[pw.first] = q;
    }
    HIP_TRY(h, hipDeviceSynchronize());
    return 0;
}

// ---- the option table: dsg_create (defaults and DSG_* environment defaults), dsg_set_option, dsg_get_option and dsg_option_info all
// walk it, so an option is one row here plus, where what runs differs from what is stored, one `effective` hook
bool bx_on(dsg_handle h), prune_opts_on(dsg_handle h), dedup_opts_on(dsg_handle h);
int dedup_levels(dsg_handle h);

enum OptEnv { ENV_FLAG, ENV_INT };      // the environment variable, where set: first character != '0'; or atoi
enum OptNorm { NORM_ON, NORM_CLAMP };   // what a value becomes: 0 stays 0 and anything else goes to 1..hi; or lo..hi
// flags.  KEEPS_GRAPHS: the launches and their arguments are the same for every value, so no drop_graphs and no validate_plan;
// STRICT: a value outside lo..hi is refused, not clamped
enum : unsigned { OPT_KEEPS_GRAPHS = 1, OPT_STRICT = 2 };
struct OptRow {
    const char *name, *env;   // env NULL: no environment default
    OptEnv env_parse;
    int32_t dflt;
    OptNorm norm;
    int32_t lo, hi;
    int32_t Options::*field;
    unsigned flags;
    int (*effective)(dsg_handle);   // what dsg_get_option reports; NULL: the stored value
    int32_t normalised(int32_t v) const { return norm == NORM_ON && v == 0 ? 0 : std::min(hi, std::max(norm == NORM_ON ? 1 : lo, v)); }
};
#define OPT_FLAG NORM_ON, 0, 1
#define OPT_WHEN(cond, v) [](dsg_handle h) -> int { return (cond) ? (v) : 0; }
const OptRow g_options[] = {
    // the register-resident fused kernels of the narrow levels; at C = 192 the plain GEMM pair is faster than the one-wave-per-SIMD fused MLP
    {"fused_attn", "DSG_FUSED_ATTN", ENV_FLAG, 1, OPT_FLAG, &Options::fused_attn, 0, nullptr},
    {"fused_mlp", "DSG_FUSED_MLP", ENV_FLAG, 1, OPT_FLAG, &Options::fused_mlp, 0, nullptr},
    {"fused_mlp_maxc", "DSG_FUSED_MLP_MAXC", ENV_INT, 96, NORM_CLAMP, INT32_MIN, INT32_MAX, &Options::fused_mlp_maxc, 0, nullptr},
    {"fused_readout", "DSG_FUSED_READOUT", ENV_FLAG, 1, OPT_FLAG, &Options::fused_readout, 0, nullptr},
    {"fused_patch_embed", "DSG_FUSED_PE", ENV_FLAG, 1, OPT_FLAG, &Options::fused_patch_embed, 0, nullptr},
    {"fused_rowstats", "DSG_FUSED_ROWSTATS", ENV_FLAG, 1, OPT_FLAG, &Options::fused_rowstats, 0, nullptr},   // modulate+SiLU and LayerNorm statistics in the producing GEMM's epilogue (fp32 kernel)
    {"fused_qkv_attn", "DSG_FUSED_QKV_ATTN", ENV_FLAG, 1, OPT_FLAG, &Options::fused_qkv_attn, 0, nullptr},   // QKV projection + 64-token window attention in one kernel (q, k, v never reach HBM)
    {"fused_merge", "DSG_FUSED_MERGE", ENV_FLAG, 1, NORM_ON, 0, 2, &Options::fused_merge, 0, nullptr},   // PatchMerging: gather + LayerNorm(4C) inside the reduction GEMM's A path (no merge_ln kernel); 2: also below the size where it pays (tests force it on)
    {"loop_graph", "DSG_LOOP_GRAPH", ENV_FLAG, 1, OPT_FLAG, &Options::loop_graph, 0, nullptr},   // capture whole step bodies of the reverse loop (0: only the network forward is a graph)
    {"prune_masked", "DSG_PRUNE_MASKED", ENV_FLAG, 1, OPT_FLAG, &Options::prune_masked, 0, OPT_WHEN(prune_opts_on(h), 1)},   // up path: skip rows / windows that only feed masked (padded) tokens (prune_on).  What runs: 0 with debug taps, in the split / bf16 modes, for 10 x 10 windows
    {"dedup_masked", "DSG_DEDUP_MASKED", ENV_FLAG, 1, OPT_FLAG, &Options::dedup_masked, 0, OPT_WHEN(dedup_opts_on(h), 1)},   // down path: compute a graph's identical all-padding windows once (dedup_opts_on).  What runs (in the sampler): 0 wherever the pruning is off, or the fused C = 96 kernels are
    {"dedup_levels", "DSG_DEDUP_LEVELS", ENV_INT, 0, NORM_CLAMP, 0, INT32_MAX, &Options::dedup_levels, 0, dedup_levels},   // how many levels may do so: 0 every qualifying one, 1 the finest only, ...  What runs (in the sampler, where PatchMerging takes its partial-statistics form)
    // ... and once for the whole batch in the sampler: 0 never, 1 from DEDUP_BATCH_MIN graphs, 2 always (dedup_stage_mode).  Acts where the lists
    // are written (stage_flags) and nowhere else: the launches, their grids and the list addresses are the same for every value, so the
    // captured graphs stay -- one captured under either kind of list replays under the other
    {"dedup_batch", "DSG_DEDUP_BATCH", ENV_INT, 1, NORM_CLAMP, 0, 2, &Options::dedup_batch, OPT_KEEPS_GRAPHS, OPT_WHEN(dedup_opts_on(h), h->opt.dedup_batch)},
    // where the batch shares one representative: take it from a per-step table built ahead of the loop (build_pure_table).  Likewise: the step
    // bodies are the same for both values -- the fill launch always carries the table's address (growing the table drops them) and reads
    // on the device which kind of list the last staging wrote
    {"dedup_table", "DSG_DEDUP_TABLE", ENV_FLAG, 1, OPT_FLAG, &Options::dedup_table, OPT_KEEPS_GRAPHS, OPT_WHEN(dedup_opts_on(h) && h->opt.dedup_batch > 0, h->opt.dedup_table)},
    // the shifted block behind a deduplicated first block projects QKV of the copied pure-window rows once (qkv_dedup_at: the blocks that qualify);
    // 2, measurement hook: the split form wherever the lists exist, whatever their share (qk_rule_rows).  The step bodies differ: graphs are dropped
    {"dedup_qkv", "DSG_DEDUP_QKV", ENV_FLAG, 1, NORM_CLAMP, 0, 2, &Options::dedup_qkv, 0, OPT_WHEN(dedup_opts_on(h), h->opt.dedup_qkv)},
    {"batch_invariant", nullptr, ENV_FLAG, 0, OPT_FLAG, &Options::batch_invariant, 0, nullptr},   // every choice of the plan is a function of the geometry and the other options, never of B
    {"gemm_bf16", "DSG_GEMM_BF16", ENV_FLAG, 0, OPT_FLAG, &Options::gemm_bf16, 0, OPT_WHEN(!h->opt.gemm_split, h->opt.gemm_bf16)},   // bf16-MFMA GEMMs (fp32 accumulate) / split-bf16 GEMMs (3 planes, 6 products; fp32-accurate): opt-in precision modes, the second takes precedence
    {"gemm_split", "DSG_GEMM_SPLIT", ENV_FLAG, 0, OPT_FLAG, &Options::gemm_split, 0, nullptr},
    // in the bf16 mode: 1 hidden / attention-output tensors stored as bf16 (bit-identical), 2 also qkv.  Acts whenever round 2's bf16 path is what
    // runs (pipeline off, or a width it does not take)
    {"bf16_act", nullptr, ENV_INT, 2, NORM_CLAMP, 0, 2, &Options::bf16_act, 0, OPT_WHEN(h->opt.gemm_bf16 && !h->opt.gemm_split && !bx_on(h), h->opt.bf16_act)},
    {"bf16_pipe", "DSG_BF16_PIPE", ENV_FLAG, 1, OPT_FLAG, &Options::bf16_pipe, 0, OPT_WHEN(bx_on(h), 1)},   // in that mode: the bf16 block pipeline of kernels_bx.hip (0: round 2's kernels_lp.hip path)
    // in that pipeline: the fused fc1-GELU-fc2 kernels (0: two GEMMs with a bf16 hidden tensor; 1: C <= 192 on 4 waves, C = 384 on 8; 2: C = 384 on the
    // 4-wave kernel too; 3: GEMM pair at C = 384).  The variable is a dev knob: A/B of the C = 384 MLP kernels (1 LDS-DMA, 4 round 3's)
    {"bf16_mlp", "DSG_BF16_MLP", ENV_INT, 1, NORM_CLAMP, 0, 6, &Options::bf16_mlp, 0, OPT_WHEN(bx_on(h), h->opt.bf16_mlp)},
    {"bf16_qkv_attn", "DSG_BF16_QA", ENV_INT, 1, NORM_CLAMP, 0, 3, &Options::bf16_qkv_attn, 0, OPT_WHEN(bx_on(h), h->opt.bf16_qkv_attn)},   // QKV projection + window attention in one kernel (0: GEMM + attn_bx_kernel through a bf16 qkv tensor; dev knob: 2 = the block-per-head kernel)
    {"bf16_proj_mlp", nullptr, ENV_FLAG, 1, OPT_FLAG, &Options::bf16_proj_mlp, 0, OPT_WHEN(bx_on(h) && h->opt.bf16_mlp && h->opt.bf16_proj_mlp, 1)},   // proj + residual + LayerNorm-2 in front of the fused MLP kernel (0: the proj GEMM)
    {"bf16_readout", nullptr, ENV_FLAG, 1, OPT_FLAG, &Options::bf16_readout, 0, OPT_WHEN(bx_on(h) && h->opt.bf16_readout && h->opt.fused_readout, 1)},   // the read-out's two products on the bf16 matrix pipe
    {"debug_alloc_fill", nullptr, ENV_INT, 0, NORM_CLAMP, 0, 4, &Options::debug_alloc_fill, OPT_KEEPS_GRAPHS | OPT_STRICT, nullptr},   // test hook: the pattern every AC_SCRATCH / AC_FINITE allocation is filled with (0: none; launch_debug_fill).  No launch of any entry point changes
};
#undef OPT_FLAG
#undef OPT_WHEN
const int N_OPTIONS = sizeof(g_options) / sizeof(g_options[0]);

const OptRow *find_option(const char *name) {
    for (const OptRow &r : g_options)
        if (strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

}  // namespace

extern "C" {

const char *dsg_version(void) { return "dsg-gfx950 0.4 (fp32 MFMA; ABI 5)"; }
int32_t dsg_abi_version(void) { return DSG_ABI_VERSION; }
// dsg_last_error(NULL): why the last dsg_create on this thread failed (there is no handle to ask then)
static thread_local std::string g_create_err;
// live handles of the process: when the last one is destroyed the per-stream scratch of the handle-less training kernels is released too
// (train_kernels.hip keeps it per hipStream_t and it only grows; a destroyed stream's address may be reused by a later stream)
static std::atomic<int> g_live_handles{0};

int dsg_create(const dsg_config *cfg, dsg_handle *out) { return dsg_create_patch(cfg, 1, out); }

int dsg_create_patch(const dsg_config *cfg, int32_t patch_size, dsg_handle *out) {
    if (!cfg || !out) { g_create_err = "dsg_create: null argument"; return DSG_ERR_INVALID; }
    *out = nullptr;
    g_create_err.clear();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_create_err = "dsg_create: no HIP device (there is no CPU path)"; return DSG_ERR_HIP; }
    auto h = new dsg_handle_s();
    h->cfg = *cfg;
    h->N = cfg->max_node_num; h->Ca = cfg->c_adj; h->Cn = cfg->c_node; h->E = cfg->embed_dim; h->L = cfg->num_layers;
    auto bad = [&](const char *m) { delete h; g_create_err = std::string("dsg_create: ") + m; return DSG_ERR_INVALID; };
    if (h->L < 1 || h->L > DSG_MAX_LAYERS) return bad("num_layers");
    if (h->E % 32 != 0 || h->E < 64) return bad("embed_dim must be a multiple of 32");
    if (cfg->mlp_ratio < 1 || h->N < 1 || h->Ca < 1 || h->Cn < 1) return bad("sizes");
    if (h->N % (1 << (h->L - 1)) != 0) return bad("max_node_num not divisible by 2^(L-1)");
    if (patch_size != 1 && patch_size != 2 && patch_size != 4) return bad("patch_size must be 1, 2 or 4");
    if (h->N % patch_size != 0) return bad("max_node_num not divisible by patch_size");
    h->P = patch_size; h->R0 = h->N / patch_size;
    if (h->P > 1) {
        if (h->R0 % (1 << (h->L - 1)) != 0) return bad("patch_size: max_node_num / patch_size not divisible by 2^(L-1)");
        // the reference's PatchBreakup asserts an even resolution on its input (diffusesg.py:381): the coarsest level's
        if (h->L >= 2 && (h->R0 >> (h->L - 1)) % 2 != 0)
            return bad("patch_size: the coarsest resolution (max_node_num / patch_size) >> (L-1) is odd, the reference's PatchBreakup refuses it");
    }
    for (int l = 0; l < h->L; l++) {
        const int C = h->E << l, res = h->R0 >> l, ws = level_window(*cfg, h->R0, l);
        if (cfg->num_heads[l] * 32 != C) return bad("head_dim must be 32");
        if (res % ws != 0) return bad("resolution not divisible by window");
        if (!(ws == 2 || ws == 4 || ws == 5 || ws == 8 || ws == 10)) return bad("window side must be one of 2, 4, 5, 8, 10");
        if (C > 1536 || (l < h->L - 1 && 4 * C > 1536)) return bad("row wider than 1536 channels");
    }
    h->Cin = (cfg->self_condition ? 2 : 1) * (h->Ca + 2 * h->Cn);
    h->Kp = ((h->P * h->P * h->Cin + 31) / 32) * 32;
    build_specs(h);
    if (!gelu_table()) { delete h; return DSG_ERR_HIP; }
    for (const OptRow &r : g_options) {   // the default, or the environment's: read the row's way and normalised like dsg_set_option's values
        const char *v = r.env ? getenv(r.env) : nullptr;
        h->opt.*r.field = !v ? r.dflt : r.normalised(r.env_parse == ENV_INT ? atoi(v) : v[0] != '0');
    }
    {   // the list GEMM picks its form from how many CUs a launch would fill (kernels.h: gemm_thin_rule); unknown = never thin
        int dev = 0, n_cu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) h->n_cu = n_cu;
        h->device = dev;
    }
    *out = h;
    g_live_handles++;
    return DSG_OK;
}

void dsg_destroy(dsg_handle h) {
    if (!h) return;
    if (h->guide) (void)dsg_detach_guide(h);
    if (h->guide_of) (void)dsg_detach_guide(h->guide_of);
    owned_free_all(h->derived_allocs);
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    drop_graphs(h);
    owned_free_all(h->allocs);   // weights and their copies, prof_gemm, tab_*, tab_step, the train_* arenas, train_const
    for (auto &kv : h->ws) {
        if (kv.second->cap_stream) (void)hipStreamDestroy(kv.second->cap_stream);
        owned_free_all(kv.second->allocs);   // tab_pure and the first-use buffers included
    }
    delete h;
    if (--g_live_handles == 0) { (void)hipDeviceSynchronize(); t_scratch_release(); }
}

const char *dsg_last_error(dsg_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int dsg_num_weight_keys(dsg_handle h) { return h ? (int)h->specs.size() : 0; }
const char *dsg_weight_key(dsg_handle h, int32_t i) {
    if (!h || i < 0 || i >= (int)h->specs.size()) return nullptr;
    return h->specs[i].key.c_str();
}

int dsg_set_weight(dsg_handle h, const char *key, const void *data, const int64_t *shape, int32_t ndim, int32_t is_device) {
    if (!h || !key || !data) return DSG_ERR_INVALID;
    const std::string k = strip_prefix(key);
    const WSpec *sp = nullptr;
    for (auto &s : h->specs) if (s.key == k) { sp = &s; break; }
    if (!sp) return fail(h, DSG_ERR_WEIGHTS, "unexpected key '%s'", key);
    if ((int)sp->shape.size() != ndim) return fail(h, DSG_ERR_WEIGHTS, "rank mismatch for '%s'", key);
    int64_t numel = 1;
    for (int i = 0; i < ndim; i++) {
        if (shape[i] != sp->shape[i]) return fail(h, DSG_ERR_WEIGHTS, "shape mismatch for '%s' (dim %d: %lld vs %lld)", key, i,
                                                  (long long)shape[i], (long long)sp->shape[i]);
        numel *= shape[i];
    }
    DevTensor &t = h->w[k];
    if (sp->is_index || sp->is_mask) {  // constant buffers: re-derived by the library, only registered as present
        t.numel = numel; t.shape = sp->shape;
        return DSG_OK;
    }
    if (!t.p) if (int rc = owned_alloc(h, h->allocs, (void **)&t.p, sizeof(float) * numel, AC_CONST)) return rc;
    HIP_TRY(h, hipMemcpy(t.p, data, sizeof(float) * numel, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    t.numel = numel; t.shape = sp->shape;
    h->finalized = false;
    return DSG_OK;
}

int dsg_finalize_weights(dsg_handle h) {
    if (!h) return DSG_ERR_INVALID;
    for (auto &s : h->specs)
        if (!h->w.count(s.key)) return fail(h, DSG_ERR_WEIGHTS, "missing key '%s' (strict load)", s.key.c_str());
    owned_free_all(h->derived_allocs);
    for (int l = 0; l < DSG_MAX_LAYERS; l++) { h->down[l].clear(); h->up[l].clear(); }
    const dsg_config &c = h->cfg;
    const int E = h->E, L = h->L;
    // block plans + concatenated affine (all (scale,shift) linears of the net in one [aff_n,512] GEMM)
    std::vector<std::string> aff_prefixes;
    int off = 0;
    h->pe_aff_off = off; aff_prefixes.push_back("patch_embed"); off += 2 * E;
    auto mk = [&](const std::string &p, int l, int j) {
        BlockPlan b;
        b.prefix = p; b.lvl = l; b.C = E << l; b.res = h->R0 >> l; b.ws = level_window(c, h->R0, l);
        b.shift = block_shift(c, h->R0, l, j); b.heads = c.num_heads[l]; b.aff_off = off;
        aff_prefixes.push_back(p); off += 2 * b.C;
        return b;
    };
    for (int l = 0; l < L; l++)
        for (int j = 0; j < c.depths[l]; j++)
            h->down[l].push_back(mk("down_layers." + std::to_string(l) + ".blocks." + std::to_string(j), l, j));
    for (int i = 0; i < L; i++)
        for (int j = 0; j < c.depths[L - 1 - i]; j++)
            h->up[i].push_back(mk("up_layers." + std::to_string(i) + ".blocks." + std::to_string(j), L - 1 - i, j));
    h->prune.built = false;
    h->aff_n = off;
    void *p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * (size_t)off * NOISE_EMB, AC_CONST)) return rc;
    h->aff_w = (float *)p;
    if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * (size_t)off, AC_CONST)) return rc;
    h->aff_b = (float *)p;
    {
        size_t o = 0;
        for (auto &pre : aff_prefixes) {
            const DevTensor &w = h->w.at(pre + ".affine.weight"), &b = h->w.at(pre + ".affine.bias");
            HIP_TRY(h, hipMemcpy(h->aff_w + o * NOISE_EMB, w.p, sizeof(float) * w.numel, hipMemcpyDeviceToDevice));
            HIP_TRY(h, hipMemcpy(h->aff_b + o, b.p, sizeof(float) * b.numel, hipMemcpyDeviceToDevice));
            o += b.numel;
        }
    }
    for (int l = 0; l < L; l++) {
        for (auto *vec : {&h->down[l], &h->up[l]})
            for (auto &b : *vec) {
                if (int rc = build_bias_table(h, b)) return rc;
                if (int rc = pack_mlp_weights(h, b)) return rc;
                if (int rc = pack_attn_weights(h, b)) return rc;
                const int C = b.C, Hd = h->cfg.mlp_ratio * C;
                if (int rc = fold_ln(h, WT(h, b.prefix + ".attn.qkv.weight"), WT(h, b.prefix + ".attn.qkv.bias"), WT(h, b.prefix + ".norm1.weight"),
                                     WT(h, b.prefix + ".norm1.bias"), 3 * C, C, &b.qkv_wf, &b.qkv_bf, C, kQScale)) return rc;
                if (int rc = fold_ln(h, WT(h, b.prefix + ".mlp.fc1.weight"), WT(h, b.prefix + ".mlp.fc1.bias"), WT(h, b.prefix + ".norm2.weight"),
                                     WT(h, b.prefix + ".norm2.bias"), Hd, C, &b.fc1_wf, &b.fc1_bf)) return rc;
            }
    }
    for (int l = 0; l + 1 < L; l++) {   // PatchMerging: norm(4C) folded into reduction (no bias in the reference: the folded bias is W.beta)
        const std::string pm = "down_layers." + std::to_string(l) + ".downsample";
        const int C = E << l;
        if (int rc = fold_ln(h, WT(h, pm + ".reduction.weight"), nullptr, WT(h, pm + ".norm.weight"), WT(h, pm + ".norm.bias"), 2 * C, 4 * C,
                             &h->merge_wf[l], &h->merge_bf[l])) return rc;
    }
    // patch_embed.proj [E,Cin,p,p] -> [E,Kp] zero padded, k = (a p + b) Cin + c: launch_assemble_patch's order (p = 1: k = c)
    {
        const int P = h->P, PP = P * P;
        std::vector<float> src((size_t)E * h->Cin * PP), dst((size_t)E * h->Kp, 0.f);
        HIP_TRY(h, hipMemcpy(src.data(), WT(h, "patch_embed.proj.weight"), sizeof(float) * src.size(), hipMemcpyDeviceToHost));
        for (int e = 0; e < E; e++)
            for (int k = 0; k < h->Cin; k++)
                for (int ab = 0; ab < PP; ab++) dst[(size_t)e * h->Kp + (size_t)ab * h->Cin + k] = src[((size_t)e * h->Cin + k) * PP + ab];
        if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * dst.size(), AC_CONST)) return rc;
        h->pe_w = (float *)p;
        HIP_TRY(h, hipMemcpy(h->pe_w, dst.data(), sizeof(float) * dst.size(), hipMemcpyHostToDevice));
        h->pe_wp = nullptr;
        if (E == 96 && h->Kp <= 64 && P == 1) {   // (the fused kernel gathers one pixel per token)
            const int S = h->Kp / 8;
            std::vector<float> pk(dst.size());
            for (int nt = 0; nt < E / 32; nt++)
                for (int sx = 0; sx < S; sx++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int t = 0; t < 4; t++)
                            pk[(((size_t)nt * S + sx) * 64 + lane) * 4 + t] = dst[(size_t)(32 * nt + (lane & 31)) * h->Kp + 8 * sx + 4 * (lane >> 5) + t];
            if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * pk.size(), AC_CONST)) return rc;
            h->pe_wp = (float *)p;
            HIP_TRY(h, hipMemcpy(h->pe_wp, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice));
        }
        h->pe_kps = ((h->Cin + 31) / 32) * 32;
        if (E == 96 && P == 2 && h->pe_kps <= 64) {   // the fused p = 2 kernel: one fragment pack per sub-pixel, each zero-padded to pe_kps
            const int S = h->pe_kps / 8;
            std::vector<float> pk((size_t)4 * E * h->pe_kps, 0.f);
            for (int sub = 0; sub < 4; sub++)
                for (int nt = 0; nt < E / 32; nt++)
                    for (int sx = 0; sx < S; sx++)
                        for (int lane = 0; lane < 64; lane++)
                            for (int t = 0; t < 4; t++) {
                                const int c = 8 * sx + 4 * (lane >> 5) + t;
                                if (c < h->Cin)
                                    pk[((((size_t)sub * 3 + nt) * S + sx) * 64 + lane) * 4 + t] = src[((size_t)(32 * nt + (lane & 31)) * h->Cin + c) * 4 + sub];
                            }
            if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * pk.size(), AC_CONST)) return rc;
            h->pe_wp = (float *)p;
            HIP_TRY(h, hipMemcpy(h->pe_wp, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice));
        }
    }
    // read_out.0 is a ConvTranspose2d: weight [in,out,1,1] (diffusesg.py:706) -> [out,in]
    // patch_size p: [in,out,p,p] -> [p^2 out, in], row (a p + b) E + o, so that one GEMM writes the p^2 pixels of a token side by side:
    // its [B R^2, p^2 E] result read as [B N^2, E] is r0 with rows in (token, a, b) order; the bias repeats per sub-pixel
    {
        const int PP = h->P * h->P;
        std::vector<float> src((size_t)E * E * PP), dst((size_t)PP * E * E), b0(E), b0r((size_t)PP * E);
        HIP_TRY(h, hipMemcpy(src.data(), WT(h, "read_out.0.weight"), sizeof(float) * src.size(), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(b0.data(), WT(h, "read_out.0.bias"), sizeof(float) * E, hipMemcpyDeviceToHost));
        for (int i = 0; i < E; i++)
            for (int o = 0; o < E; o++)
                for (int ab = 0; ab < PP; ab++) dst[((size_t)ab * E + o) * E + i] = src[((size_t)i * E + o) * PP + ab];
        for (int ab = 0; ab < PP; ab++)
            for (int o = 0; o < E; o++) b0r[(size_t)ab * E + o] = b0[o];
        if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * dst.size(), AC_CONST)) return rc;
        h->ro0_w = (float *)p;
        HIP_TRY(h, hipMemcpy(h->ro0_w, dst.data(), sizeof(float) * dst.size(), hipMemcpyHostToDevice));
        const float *bias0 = WT(h, "read_out.0.bias");
        if (PP > 1) {
            if (int rc = owned_alloc(h, h->derived_allocs, &p, sizeof(float) * b0r.size(), AC_CONST)) return rc;
            HIP_TRY(h, hipMemcpy(p, b0r.data(), sizeof(float) * b0r.size(), hipMemcpyHostToDevice));
            bias0 = (const float *)p;
        }
        if (int rc = fold_ln(h, h->ro0_w, bias0, WT(h, "norm.weight"), WT(h, "norm.bias"), PP * E, E, &h->ro0_wf, &h->ro0_bf)) return rc;
    }
    // Folded read-out (E = 96, C_adj <= 32): final-LN output -> read_out.0/1/2 -> readout_adj_mlp.fc1 is affine up to the
    // GELU, and the node head's pooled shared_rep is an affine image of the pooled LN output.  Fold in double precision.
    h->ro_fap = h->ro_fa = h->ro_f2p = h->ro_gext = nullptr;
    h->ro_fapb = h->ro_f2pb = nullptr;
    if (E == 96 && h->Ca <= 32 && h->P == 1) {   // (patch_size > 1 runs the chain: DESIGN.md §15)
        auto dl = [&](const char *k, size_t n) { std::vector<float> v(n); (void)hipMemcpy(v.data(), WT(h, k), sizeof(float) * n, hipMemcpyDeviceToHost); return v; };
        const std::vector<float> r0 = dl("read_out.0.weight", (size_t)E * E), r1 = dl("read_out.1.weight", (size_t)E * E),
                                 r2 = dl("read_out.2.weight", (size_t)E * E), b0 = dl("read_out.0.bias", E), b1 = dl("read_out.1.bias", E),
                                 b2 = dl("read_out.2.bias", E), F1 = dl("readout_adj_mlp.fc1.weight", (size_t)E * E),
                                 f1 = dl("readout_adj_mlp.fc1.bias", E), F2 = dl("readout_adj_mlp.fc2.weight", (size_t)h->Ca * E),
                                 G1 = dl("readout_node_mlp.fc1.weight", (size_t)E * E);
        typedef std::vector<double> dv;
        auto matmul = [&](const dv &X, const dv &Y) { dv Z((size_t)E * E, 0.0); for (int i = 0; i < E; i++) for (int k = 0; k < E; k++) { const double a = X[(size_t)i * E + k]; for (int j = 0; j < E; j++) Z[(size_t)i * E + j] += a * Y[(size_t)k * E + j]; } return Z; };
        auto matvec = [&](const dv &X, const dv &v) { dv z(E, 0.0); for (int i = 0; i < E; i++) for (int k = 0; k < E; k++) z[i] += X[(size_t)i * E + k] * v[k]; return z; };
        dv W0t((size_t)E * E), W1(r1.begin(), r1.end()), W2(r2.begin(), r2.end()), dF1(F1.begin(), F1.end()), dG1(G1.begin(), G1.end());
        for (int i = 0; i < E; i++) for (int o = 0; o < E; o++) W0t[(size_t)o * E + i] = r0[(size_t)i * E + o];  // ConvTranspose2d [in,out]
        const dv A = matmul(W2, matmul(W1, W0t));
        dv t1 = matvec(W1, dv(b0.begin(), b0.end()));
        for (int i = 0; i < E; i++) t1[i] += b1[i];
        dv a = matvec(W2, t1);
        for (int i = 0; i < E; i++) a[i] += b2[i];
        const dv Fa = matmul(dF1, A);
        dv fa = matvec(dF1, a);
        for (int i = 0; i < E; i++) fa[i] += f1[i];
        const dv Gn = matmul(dG1, A), ga = matvec(dG1, a);
        const int S = E / 8;
        std::vector<float> fap((size_t)E * E), f2p((size_t)3 * 4 * 64 * 4, 0.f), gext((size_t)E * 128, 0.f), faf(E);
        for (int nt = 0; nt < 3; nt++)
            for (int sx = 0; sx < S; sx++)
                for (int lane = 0; lane < 64; lane++)
                    for (int t = 0; t < 4; t++)
                        fap[(((size_t)nt * S + sx) * 64 + lane) * 4 + t] = (float)Fa[(size_t)(32 * nt + (lane & 31)) * E + 8 * sx + 4 * (lane >> 5) + t];
        for (int nt = 0; nt < 3; nt++)
            for (int g = 0; g < 4; g++)
                for (int lane = 0; lane < 64; lane++)
                    for (int t = 0; t < 4; t++) {
                        const int c = lane & 31;
                        f2p[(((size_t)nt * 4 + g) * 64 + lane) * 4 + t] = c < h->Ca ? F2[(size_t)c * E + 32 * nt + 8 * g + 4 * (lane >> 5) + t] : 0.f;
                    }
        for (int i = 0; i < E; i++) {
            faf[i] = (float)fa[i];
            for (int k = 0; k < E; k++) gext[(size_t)i * 128 + k] = (float)Gn[(size_t)i * E + k];
            gext[(size_t)i * 128 + 96] = (float)ga[i];
        }
        auto up = [&](const std::vector<float> &v, float **dst) -> int {
            void *q;
            if (int rc = owned_alloc(h, h->derived_allocs, &q, sizeof(float) * v.size(), AC_CONST)) return rc;
            *dst = (float *)q;
            HIP_TRY(h, hipMemcpy(q, v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice));
            return 0;
        };
        if (int rc = up(fap, &h->ro_fap)) return rc;
        if (int rc = up(faf, &h->ro_fa)) return rc;
        if (int rc = up(f2p, &h->ro_f2p)) return rc;
        if (int rc = up(gext, &h->ro_gext)) return rc;
        // bf16-MFMA fragments (32x32x16: lane (row, half) holds 8 k values per k-step; k order 16 s + 8 (j >> 2) + 4 half + (j & 3), the order
        // in which fused_readout96_kernel<true>'s register pairs enumerate LN(x)'s channels / the hidden units)
        std::vector<float> fapb((size_t)3 * 6 * 64 * 8), f2pb((size_t)3 * 2 * 64 * 8, 0.f);
        for (int nt = 0; nt < 3; nt++)
            for (int sx = 0; sx < 6; sx++)
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++)
                        fapb[(((size_t)nt * 6 + sx) * 64 + lane) * 8 + j] =
                            (float)Fa[(size_t)(32 * nt + (lane & 31)) * E + 16 * sx + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)];
        for (int nt = 0; nt < 3; nt++)
            for (int g2 = 0; g2 < 2; g2++)
                for (int lane = 0; lane < 64; lane++)
                    for (int j = 0; j < 8; j++) {
                        const int c = lane & 31;
                        f2pb[(((size_t)nt * 2 + g2) * 64 + lane) * 8 + j] =
                            c < h->Ca ? F2[(size_t)c * E + 32 * nt + 16 * g2 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)] : 0.f;
                    }
        if (int rc = up(fapb, &h->ro_fapb)) return rc;
        if (int rc = up(f2pb, &h->ro_f2pb)) return rc;
    }
    // The same fold at patch_size 2: A = W2 W1, Fa[a, b] = F1 A W0[:, :, a, b]^T per sub-pixel, the constant c = A b0 + W2 b1 + b2
    // (fa = F1 c + f1 is the same for the four), and for the node head G1 A W0[:, :, a, b]^T over the pooled LN(x) of column parity b
    h->ro_gext2[0] = h->ro_gext2[1] = nullptr;
    if (E == 96 && h->Ca <= 32 && h->P == 2) {
        auto dl = [&](const char *k, size_t n) { std::vector<float> v(n); (void)hipMemcpy(v.data(), WT(h, k), sizeof(float) * n, hipMemcpyDeviceToHost); return v; };
        const std::vector<float> r0 = dl("read_out.0.weight", (size_t)E * E * 4), r1 = dl("read_out.1.weight", (size_t)E * E),
                                 r2 = dl("read_out.2.weight", (size_t)E * E), b0 = dl("read_out.0.bias", E), b1 = dl("read_out.1.bias", E),
                                 b2 = dl("read_out.2.bias", E), F1 = dl("readout_adj_mlp.fc1.weight", (size_t)E * E),
                                 f1 = dl("readout_adj_mlp.fc1.bias", E), F2 = dl("readout_adj_mlp.fc2.weight", (size_t)h->Ca * E),
                                 G1 = dl("readout_node_mlp.fc1.weight", (size_t)E * E);
        typedef std::vector<double> dv;
        auto matmul = [&](const dv &X, const dv &Y) { dv Z((size_t)E * E, 0.0); for (int i = 0; i < E; i++) for (int k = 0; k < E; k++) { const double a = X[(size_t)i * E + k]; for (int j = 0; j < E; j++) Z[(size_t)i * E + j] += a * Y[(size_t)k * E + j]; } return Z; };
        auto matvec = [&](const dv &X, const dv &v) { dv z(E, 0.0); for (int i = 0; i < E; i++) for (int k = 0; k < E; k++) z[i] += X[(size_t)i * E + k] * v[k]; return z; };
        const dv W1(r1.begin(), r1.end()), W2(r2.begin(), r2.end()), dF1(F1.begin(), F1.end()), dG1(G1.begin(), G1.end());
        const dv A = matmul(W2, W1);
        dv t1 = matvec(W1, dv(b0.begin(), b0.end()));
        for (int i = 0; i < E; i++) t1[i] += b1[i];
        dv cc = matvec(W2, t1);
        for (int i = 0; i < E; i++) cc[i] += b2[i];
        dv fa = matvec(dF1, cc);
        for (int i = 0; i < E; i++) fa[i] += f1[i];
        const dv ga = matvec(dG1, cc);
        const int S = E / 8;
        std::vector<float> fap((size_t)4 * E * E), f2p((size_t)3 * 4 * 64 * 4, 0.f), faf(E), gx[2] = {std::vector<float>((size_t)E * 256, 0.f), std::vector<float>((size_t)E * 256, 0.f)};
        for (int sub = 0; sub < 4; sub++) {
            dv W0t((size_t)E * E);
            for (int i = 0; i < E; i++) for (int o = 0; o < E; o++) W0t[(size_t)o * E + i] = r0[((size_t)i * E + o) * 4 + sub];   // ConvTranspose2d [in,out,a,b]
            const dv Aab = matmul(A, W0t), Fa = matmul(dF1, Aab), Gn = matmul(dG1, Aab);
            for (int nt = 0; nt < 3; nt++)
                for (int sx = 0; sx < S; sx++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int t = 0; t < 4; t++)
                            fap[((((size_t)sub * 3 + nt) * S + sx) * 64 + lane) * 4 + t] = (float)Fa[(size_t)(32 * nt + (lane & 31)) * E + 8 * sx + 4 * (lane >> 5) + t];
            for (int i = 0; i < E; i++)
                for (int k = 0; k < E; k++) gx[sub >> 1][(size_t)i * 256 + 96 * (sub & 1) + k] = (float)Gn[(size_t)i * E + k];
        }
        for (int nt = 0; nt < 3; nt++)
            for (int g = 0; g < 4; g++)
                for (int lane = 0; lane < 64; lane++)
                    for (int t = 0; t < 4; t++) {
                        const int c = lane & 31;
                        f2p[(((size_t)nt * 4 + g) * 64 + lane) * 4 + t] = c < h->Ca ? F2[(size_t)c * E + 32 * nt + 8 * g + 4 * (lane >> 5) + t] : 0.f;
                    }
        for (int i = 0; i < E; i++) {
            faf[i] = (float)fa[i];
            for (int a = 0; a < 2; a++) gx[a][(size_t)i * 256 + 192] = gx[a][(size_t)i * 256 + 193] = (float)ga[i];
        }
        auto up = [&](const std::vector<float> &v, float **dst) -> int {
            void *q;
            if (int rc = owned_alloc(h, h->derived_allocs, &q, sizeof(float) * v.size(), AC_CONST)) return rc;
            *dst = (float *)q;
            HIP_TRY(h, hipMemcpy(q, v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice));
            return 0;
        };
        if (int rc = up(fap, &h->ro_fap)) return rc;
        if (int rc = up(faf, &h->ro_fa)) return rc;
        if (int rc = up(f2p, &h->ro_f2p)) return rc;
        if (int rc = up(gx[0], &h->ro_gext2[0])) return rc;
        if (int rc = up(gx[1], &h->ro_gext2[1])) return rc;
    }
    drop_graphs(h);   // captured graphs bake weight pointers
    // bf16 copies (opt-in mode): drop stale ones, list every GEMM weight, rebuild if the mode is on
    for (auto &kv : h->w_bf16) owned_free(h->allocs, kv.second);
    h->w_bf16.clear();
    for (auto &kv : h->w_img) owned_free(h->allocs, kv.second);
    h->w_img.clear();
    for (auto &kv : h->w_img2) owned_free(h->allocs, kv.second);
    h->w_img2.clear();
    for (auto &kv : h->w_qimg) owned_free(h->allocs, kv.second);
    h->w_qimg.clear();
    for (auto &kv : h->w_img96) owned_free(h->allocs, kv.second);
    h->w_img96.clear();
    for (auto &kv : h->w_split) owned_free(h->allocs, kv.second);
    h->w_split.clear();
    h->gemm_weights.clear();
    for (auto &kv : h->w)
        if (kv.second.p && kv.second.shape.size() >= 2) h->gemm_weights.push_back({kv.second.p, (size_t)kv.second.numel});
    for (int l = 0; l < L; l++)
        for (auto *vec : {&h->down[l], &h->up[l]})
            for (auto &b : *vec) {
                h->gemm_weights.push_back({b.qkv_wf, (size_t)3 * b.C * b.C});
                h->gemm_weights.push_back({b.fc1_wf, (size_t)c.mlp_ratio * b.C * b.C});
            }
    for (int l = 0; l + 1 < L; l++) h->gemm_weights.push_back({h->merge_wf[l], (size_t)8 * (E << l) * (E << l)});
    h->gemm_weights.push_back({h->aff_w, (size_t)h->aff_n * NOISE_EMB});
    h->gemm_weights.push_back({h->pe_w, (size_t)E * h->Kp});
    h->gemm_weights.push_back({h->ro0_wf, (size_t)h->P * h->P * E * E});
    if (h->ro_gext) h->gemm_weights.push_back({h->ro_gext, (size_t)E * 128});
    if (h->ro_fapb) h->gemm_weights.push_back({h->ro_fapb, (size_t)3 * 6 * 64 * 8});
    if (h->ro_f2pb) h->gemm_weights.push_back({h->ro_f2pb, (size_t)3 * 2 * 64 * 8});
    if (h->opt.gemm_bf16) if (int rc = ensure_bf16_weights(h)) return rc;
    if (h->opt.gemm_split) if (int rc = ensure_split_weights(h)) return rc;
    h->finalized = true;
    h->ever_finalized = true;
    return DSG_OK;
}

}  // extern "C"

namespace {

// rows per sample of the activation buffers x / y / att: the level-0 tokens, or at patch_size > 1 the N^2 pixel rows of the read-out chain
// (p^2 times as many; x and y trade names under the fused PatchMerging, so all three have the size)
size_t act_rows(dsg_handle h) { return h->P > 1 ? (size_t)h->N * h->N : (size_t)h->R0 * h->R0; }

size_t per_sample_floats(dsg_handle h, std::vector<size_t> *parts = nullptr) {
    const size_t T0 = (size_t)h->R0 * h->R0, E = h->E, TA = act_rows(h);
    const size_t sa = (size_t)h->Ca * h->N * h->N, sn = (size_t)h->N * h->Cn;
    std::vector<size_t> v = {
        sa, sn, sa, sn, sa, sn,                  // in, sc, f
        (size_t)E, NOISE_EMB, NOISE_EMB, (size_t)h->aff_n,   // pe, emb0, emb, aff
        T0 * h->Kp,                              // tok_in
        TA * E, TA * E, T0 * E / 2,              // x, y, xn (bf16)
        3 * T0 * E, TA * E,                      // qkv, att
        (size_t)h->cfg.mlp_ratio * T0 * E,       // hid
        2 * T0,                                  // stats
        (size_t)h->N * E, (size_t)h->N * E,      // pool, hn
        (size_t)h->N * (h->P == 2 ? 256 : 128), (size_t)h->N * readout_pool_segments(h->N) * 96,   // pool_ext (p = 2: two parities), pool_part
        sa, sn, sa, sn, 3 * sa, 3 * sn,          // sampler x, xhat, d[3]
    };
    size_t tot = 0;
    for (auto s : v) tot += s;
    for (int l = 0; l < h->L; l++) tot += (T0 * E) >> (l + 1 < h->L ? l + 1 : l);
    if (parts) *parts = v;
    return tot;
}

int validate_plan(dsg_handle h, Workspace *w);
const PrunePlan &prune_plan(dsg_handle h);
int get_workspace(dsg_handle h, int B, Workspace **out) {
    auto it = h->ws.find(B);
    if (it != h->ws.end()) { *out = it->second.get(); return validate_plan(h, *out); }
    auto w = std::make_unique<Workspace>();
    w->B = B;
    const size_t T0 = (size_t)h->R0 * h->R0, E = h->E, TA = act_rows(h);
    const size_t sa = (size_t)B * h->Ca * h->N * h->N, sn = (size_t)B * h->N * h->Cn;
    auto A = [&](float **p, size_t n, AllocClass cls) -> int {
        void *q;
        if (int rc = owned_alloc(h, w->allocs, &q, sizeof(float) * n, cls)) return rc;
        *p = (float *)q; w->bytes += sizeof(float) * n;
        return 0;
    };
#define ALLOC(ptr, n) do { if (int rc = A(&(ptr), (n), AC_SCRATCH)) return rc; } while (0)
#define ALLOC_FINITE(ptr, n) do { if (int rc = A(&(ptr), (n), AC_FINITE)) return rc; } while (0)
    ALLOC(w->in_adj, sa); ALLOC(w->in_node, sn); ALLOC(w->sc_adj, sa); ALLOC(w->sc_node, sn);
    ALLOC(w->f_adj, sa); ALLOC(w->f_node, sn); ALLOC(w->c_noise, B); ALLOC(w->sig, B);
    ALLOC(w->pe, (size_t)B * E); ALLOC(w->emb0, (size_t)B * NOISE_EMB); ALLOC(w->emb, (size_t)B * NOISE_EMB);
    ALLOC(w->aff, (size_t)B * h->aff_n);
    ALLOC(w->tok_in, (size_t)B * T0 * h->Kp);
    ALLOC_FINITE(w->x, (size_t)B * TA * E); ALLOC_FINITE(w->y, (size_t)B * TA * E);
    { float *xn_; ALLOC(xn_, (size_t)B * T0 * E / 2 + 64); w->xn = xn_; }
    ALLOC(w->qkv, (size_t)B * 3 * T0 * E); ALLOC_FINITE(w->att, (size_t)B * TA * E);
    ALLOC_FINITE(w->hid, (size_t)B * h->cfg.mlp_ratio * T0 * E);
    ALLOC_FINITE(w->stats, (size_t)B * 2 * T0);
    ALLOC(w->pool, (size_t)B * h->N * E); ALLOC(w->hn, (size_t)B * h->N * E); ALLOC(w->pool_ext, (size_t)B * h->N * (h->P == 2 ? 256 : 128));
    ALLOC(w->pool_part, (size_t)B * h->N * readout_pool_segments(h->N) * 96);
    for (int l = 0; l < h->L; l++) ALLOC(w->skips[l], ((size_t)B * T0 * E) >> (l + 1 < h->L ? l + 1 : l));
    ALLOC(w->x_adj, sa); ALLOC(w->x_node, sn); ALLOC(w->xh_adj, sa); ALLOC(w->xh_node, sn);
    for (int k = 0; k < 3; k++) { ALLOC(w->d_adj[k], sa); ALLOC(w->d_node[k], sn); }
#undef ALLOC
#undef ALLOC_FINITE
    void *q;
    if (int rc = owned_alloc(h, w->allocs, &q, (size_t)B * h->N, AC_STATE)) return rc;
    w->flags = (uint8_t *)q;
    if (int rc = owned_alloc(h, w->allocs, &q, 16, AC_STATE)) return rc;
    w->has_sc = (int *)q;
    if (int rc = owned_alloc(h, w->allocs, &q, sizeof(RunCtl), AC_STATE)) return rc;
    w->ctl = (RunCtl *)q;
    // masked-token pruning leaves the rows nobody reads untouched: they must never hold anything but finite numbers
    HIP_TRY(h, hipMemset(w->x, 0, sizeof(float) * (size_t)B * TA * E));
    HIP_TRY(h, hipMemset(w->y, 0, sizeof(float) * (size_t)B * TA * E));
    HIP_TRY(h, hipMemset(w->att, 0, sizeof(float) * (size_t)B * TA * E));
    HIP_TRY(h, hipMemset(w->hid, 0, sizeof(float) * (size_t)B * h->cfg.mlp_ratio * T0 * E));
    HIP_TRY(h, hipMemset(w->stats, 0, sizeof(float) * (size_t)B * 2 * T0));
    w->need = prune_plan(h).np;
    if (w->need.n_lists > 0) {
        const int nl = w->need.n_lists;
        size_t off = 0;
        for (int k = 0; k < nl; k++) { w->need.list_off[k] = (int)off; off += (size_t)B * prune_plan(h).items[k] + 16; }
        const bool dd = w->need.dd_n > 0;
        w->need_ints = off + nl + (size_t)B * nl + (size_t)B * w->need.dd_n + (dd ? 1 : 0);   // (+ the mode the lists were written for, behind dd_rep)
        if (int rc = owned_alloc(h, w->allocs, &q, sizeof(int) * w->need_ints, AC_STATE)) return rc;
        HIP_TRY(h, hipMemset(q, 0, sizeof(int) * w->need_ints));   // counts of 0 until the first flags are staged
        w->need_lists = (int *)q; w->need_cnt = w->need_lists + off; w->need_cnt_ps = w->need_cnt + nl;
        if (dd) w->dd_rep = w->need_cnt_ps + (size_t)B * nl;
        w->bytes += sizeof(int) * w->need_ints;
    }
    *out = w.get();
    h->ws[B] = std::move(w);
    return validate_plan(h, *out);
}

void tap(dsg_handle h, const char *name, const float *src, size_t numel, hipStream_t s) {
    if (g_dry_run) return;
    for (auto &t : h->taps)
        if (t.name == name && (int64_t)numel <= t.cap)
            (void)hipMemcpyAsync(t.dst, src, sizeof(float) * numel, hipMemcpyDeviceToDevice, s);
}

// P_GEMM: always exact fp32 (noise embedding / modulation parameters, patch embed, read-out and heads: small, and their
// error would enter every block).  P_GEMM_LP: the Swin-block, PatchMerging and PatchBreakup linears, which the opt-in
// "gemm_bf16" mode runs on bf16 MFMA.
// "gemm_split" (fp32-accurate split-bf16 products) applies to every GEMM and takes precedence over "gemm_bf16".
#define P_GEMM_LP(g) do { (g).Ws3 = split_of(h, (g).W); (g).Wb = (g).Ws3 ? nullptr : bf16_of(h, (g).W); P_GEMM_(g); } while (0)
#define P_GEMM(g) do { (g).Ws3 = split_of(h, (g).W); (g).Wb = nullptr; P_GEMM_(g); } while (0)
#define P_GEMM_(g) do { char tg_[96]; if (h->prof_stamps && h->prof_gemm && h->prof_gemm_used < h->prof_gemm_cap) (g).prof = h->prof_gemm + 4 * (h->prof_gemm_used++); else (g).prof = nullptr; \
    if (h->prof_on) snprintf(tg_, sizeof(tg_), "gemm M=%d N=%d K=%d ln=%d act=%d res=%d", (g).M, (g).N, (g).K, ((g).ln_stats != nullptr) + 2 * ((g).ln_part != nullptr) + 4 * ((g).stats_out != nullptr) + 8 * ((g).mod_aff != nullptr), (g).act, (g).res != nullptr); \
    (g).n_cu = h->n_cu; h->prof_next_thin_n = gemm_has_thin(g) ? (g).N : 0; \
    ProfScope ps_(h, s, PK_GEMM, 2.0 * (double)(g).M * (double)(g).N * (double)(g).K, tg_); \
    g_fixed_tiles = h->opt.batch_invariant; const bool built_ = launch_gemm((g), s); g_fixed_tiles = false; \
    if (!built_) plan_fail(h, "gemm: argument combination not built (M=%d N=%d K=%d ln=%d act=%d res=%d bf16 A/C=%d/%d)", (g).M, (g).N, (g).K, ((g).ln_stats != nullptr) + 2 * ((g).ln_part != nullptr), (g).act, (g).res != nullptr, (g).a_bf16, (g).c_bf16); } while (0)
#define P_KERN(kind, flops, call) do { ProfScope ps_(h, s, (kind), (flops), #call); call; } while (0)

// Row-kernel fusion (fp32 GEMM kernel only; off while debug taps want the un-modulated block outputs): the GEMM that produces
// a block's input also applies that block's modulate+SiLU and leaves per-column-tile (sum, sumsq) partials of the stored rows
// in w->stats, from which the consuming GEMM forms the LayerNorm statistics -- mod_stats / ln_stats launches disappear.
bool rowstats_on(dsg_handle h) { return h->opt.fused_rowstats && !h->opt.gemm_split && h->taps.empty(); }   // fp32 and bf16 GEMM kernels
// does block `nb` take its input pre-modulated?  Generic blocks also read the LN1 partials the producer leaves; the C = 96 fused
// attention kernel only skips its own modulate+SiLU (twice: prologue and shortcut) and keeps computing LN1 itself.
bool wants_premod(dsg_handle h, const BlockPlan *nb) { return nb && rowstats_on(h); }

// ---- masked-token pruning ------------------------------------------------------------------------------------------------
// DiffuseSG.forward masks all it returns with node_flags (diffusesg.py:806-825), window attention does not (:108-139): the down
// path and the coarsest level need every token, but on the way back up a token is needed only if it shares a window with a needed
// token of the next stage.  The plan below walks the up path backwards from the read-out and gives every launch the list of 8-row
// runs (or of windows) it has to compute; the walk stops at the first block whose need is structurally everything (one window, or
// a shifted partition on a 2 x 2 window grid): it and all launches in front of it run as before.  Rows nobody reads are left
// STALE in w->x / y / hid / att / stats, so every final mask must be a select (fused_readout96_kernel), never a product.
void build_prune_plan(dsg_handle h) {
    PrunePlan &P = h->prune;
    P = PrunePlan();
    P.built = true;
    const int L = h->L, N = h->N;
    for (int i = 0; i < DSG_MAX_LAYERS; i++) { P.fine[i] = P.coarse[i] = -1; }
    for (int i = 0; i < L; i++) { P.rows[i].assign(h->up[i].size(), -1); P.wins[i].assign(h->up[i].size(), -1); }
    if (h->P != 1) return;   // the lists are derived from pixel flags at token resolution: no plan at patch_size > 1
    if (N % 8 != 0 || N * N / 8 > NEED_MAX_RUNS) return;
    for (int i = 0; i < L; i++)
        for (auto &b : h->up[i]) if (b.ws != 8 || b.res % 8 != 0) return;   // 10 x 10 windows (COCO): not covered
    NeedPlan np;
    PrunePlan Q = P;
    bool overflow = false, stop = false;
    int cur = -1;   // list that holds the current set, -1: not emitted yet
    auto new_list = [&](int items) { if (np.n_lists >= NEED_MAX_LISTS) { overflow = true; return -1; } Q.items[np.n_lists] = items; return np.n_lists++; };
    auto push = [&](NeedOp op) { if (np.n_ops >= NEED_MAX_OPS) overflow = true; else np.op[np.n_ops++] = op; };
    auto emit = [&](int res) { if (cur < 0) { cur = new_list(res * res / 8); push(NeedOp{NEED_EMIT, res, 0, cur}); } return cur; };
    for (int i = L - 1; i >= 0 && !stop; i--) {
        const int res = N >> (L - 1 - i);
        for (int j = (int)h->up[i].size() - 1; j >= 0; j--) {
            const BlockPlan &b = h->up[i][j];
            Q.rows[i][j] = emit(res);
            Q.roles.push_back(PruneRole{0, res, 0, i, j, Q.rows[i][j]});
            const int nwr = res / 8;
            if (nwr == 1 || (b.shift > 0 && nwr == 2)) { stop = true; break; }   // its attention needs everything
            Q.wins[i][j] = new_list(nwr * nwr);
            push(NeedOp{NEED_WINDOWS, res, b.shift, Q.wins[i][j]});
            Q.roles.push_back(PruneRole{1, res, b.shift, i, j, Q.wins[i][j]});
            cur = -1;
        }
        if (stop || i == 0 || res % 16 != 0) break;
        Q.fine[i] = emit(res);
        Q.roles.push_back(PruneRole{0, res, 0, i, -1, Q.fine[i]});
        push(NeedOp{NEED_PARENT, res, 0, -1});
        cur = -1;
        Q.coarse[i] = emit(res / 2);
        Q.roles.push_back(PruneRole{0, res / 2, 0, i, -2, Q.coarse[i]});
    }
    if (overflow) return;
    // pure-window deduplication (kernels.h): level k = 0, 1, ... of the down path as far as the chain goes, three lists each behind the
    // pruning's (without room for them the chain ends; without level 0 the pruning stands alone).  A level qualifies where its first
    // block is unshifted on 8 x 8 windows of the level's own grid.  Level 0 also is PatchEmbed's: the C = 96 kernels.  Level k >= 1
    // needs the level below deduplicated with that block its only one (a second, shifted block mixes neighbouring windows: behind it
    // pure windows no longer share their rows) and at least 2 x 2 windows (a level of one window has nothing to share: its only
    // window is its own representative).
    for (int k = 0; k < L && k <= NEED_MAX_DD_UP; k++) {
        const int res = N >> k;
        if (h->down[k].empty() || np.n_lists + 3 > NEED_MAX_LISTS) break;
        const BlockPlan &b = h->down[k][0];
        const bool qualifies = b.shift == 0 && b.ws == 8 && b.res == res && (k == 0 ? b.C == 96 : h->down[k - 1].size() == 1 && res % 16 == 0);
        if (!qualifies) break;
        np.dd_wins[k] = new_list((res / 8) * (res / 8));
        np.dd_runs[k] = new_list(res * res / 8);
        np.dd_copy[k] = new_list((res / 8) * (res / 8));
        np.dd_n = k + 1;
        // option "dedup_qkv": a second, shifted block on the level's own 8 x 8 windows (it ends the chain) reads rows that the fill has
        // copied; its QKV projection gets the list of distinct rows and the window map, where the plan has room for the two
        if (h->down[k].size() >= 2 && np.n_lists + 2 <= NEED_MAX_LISTS) {
            const BlockPlan &b1 = h->down[k][1];
            if (b1.shift > 0 && b1.ws == 8 && b1.res == res && res >= 16) {
                np.qk_runs[k] = new_list(res * res / 8);
                np.qk_src[k] = new_list((res / 8) * (res / 8));
            }
        }
    }
    // the read-out's working 32-token tiles (readout_stage), behind everything else (the plan stands without it where there is no room)
    if (np.n_lists < NEED_MAX_LISTS) np.ro_tiles = new_list(N * N / 32);
    P = Q;
    P.np = np;
}
const PrunePlan &prune_plan(dsg_handle h) { if (!h->prune.built) build_prune_plan(h); return h->prune; }
// Decided at plan time.  Off with debug taps (they return whole tensors: the same rule as rowstats_on), in the split / bf16 modes,
// and whenever a launch of the up path is not one of the kernels that take a list.
bool prune_opts_on(dsg_handle h) {
    return h->P == 1 && h->opt.prune_masked && h->taps.empty() && !h->opt.gemm_split && !h->opt.gemm_bf16 && rowstats_on(h) && h->opt.fused_qkv_attn &&
           h->opt.fused_readout && h->ro_fap && prune_plan(h).np.n_lists > 0;
}
bool prune_on(dsg_handle h, const Workspace *w) {
    // (the row-mapped GEMM addresses whole tensors through one buffer descriptor: the widest one must stay below 2 GiB)
    return w->need_lists && prune_opts_on(h) && (size_t)w->B * h->N * h->N * h->E * h->cfg.mlp_ratio * sizeof(float) < 0x7fffffffull;
}
// Does the last block of level l leave row statistics for the partial-statistics form of PatchMerging at this batch size?
// (below ~8k merged rows the reduction GEMM is a single partial wave of tiles and the gather + LayerNorm FMA in its
// long K loop costs more than the small merge_ln launch it replaces: measured 103 vs 81 + 13 us at M = 4096, K = 1536)
bool merge_fused_at(dsg_handle h, int B, int l) {
    const int C = h->E << l, res = h->R0 >> l;
    return l < h->L - 1 && h->opt.fused_merge != 0 && rowstats_on(h) && !h->opt.gemm_bf16 && C % 32 == 0 &&
           (B * res * res / 4 >= 8192 || h->opt.fused_merge > 1 || h->opt.batch_invariant);   // "batch_invariant": the size plays no part
}
// Pure-window deduplication of the down path (options "dedup_masked", "dedup_levels", "dedup_batch"; rule and list formats: kernels.h).
// At a token (i, j) with a padded endpoint fused_patch_embed96_kernel zeroes the node channels itself, and the adjacency channels it
// reads there are zero whenever the state came from the sampler's own kernels (each stores `valid ? ... : 0.f`).  The PatchEmbed
// accumulator of such a token is then the bias, its row depends on nothing but the graph's (scale, shift), and the unshifted first
// block of a level maps every all-padding ("pure") window of a graph to the same 64 rows -- bit for bit, the kernels being
// deterministic and position-blind apart from the position inside the window.  So at level k of the chain the producer (PatchEmbed,
// or the merge into the level) and that block run over the non-pure windows plus ONE pure window per graph, and
// window_broadcast_kernel copies that window's rows (with the skip and the row statistics the next launch reads) to the other pure
// windows before anything else reads them: behind the copy the buffers hold exactly what the full launches would have written.
//
// Who decides what, and when:
// * Plan time (build_prune_plan): which levels CAN deduplicate -- np.dd_n, from the block geometry alone -- and their lists.
// * Options (dedup_opts_on, dedup_levels; what dsg_get_option reports): on only where the pruning is (same kernels, same list
//   machinery) and where PatchEmbed, attention and MLP of level 0's block are the fused C = 96 kernels.  Level k >= 1 also needs the
//   merge into it to be the partial-statistics form of PatchMerging (the "fused_merge" path), which runs over the level's run list
//   (launch_merge_norm_runs + the row-mapped reduction GEMM: the values of the gather GEMM, bit for bit); "dedup_levels" caps the count.
//   Every block kernel of those levels takes a list wherever the pruning is on (prune_opts_on).
// * Per workspace (dedup_chain_depth): how many of those levels a forward at this batch size deduplicates, 0 .. depth - 1.  Whether a
//   batch size takes the partial-statistics merge is merge_fused_at's rule (8192 merged rows, or "fused_merge" 2 / "batch_invariant");
//   a level whose merge is the merge_ln kernel ends the chain.  This is the one predicate of forward_fixed, which asks it once and
//   only checks, launch by launch, that the kernels left what it promised, and of stage_flags, which must know the top level before
//   the lists are written: only the levels under it may trim their fills.
// * Staging time (stage_flags -> dedup_stage_mode), per entry-point call, on the device: an entry point that cannot vouch for the
//   zeros (caller tensors: dsg_denoise, dsg_precond) stages lists that name every window as unique and copy nothing (DD_OFF); the
//   sampler stages one representative per graph (DD_GRAPH) or one for the batch (DD_BATCH, option "dedup_batch"; rule: kernels.h).
//   The per-graph argument never uses the graph index, so it holds across graphs wherever every graph reads the same (scale, shift)
//   row: `uniform_row` is the caller's word that every forward between this staging and the next is batch-uniform (sample_impl: all
//   of them go through precond_tab, which sets w->uniform).  From DEDUP_BATCH_MIN graphs by default: below 16 graphs no down-path
//   list launch of the N = 64 network exceeds half a round of 512 resident GEMM tiles, so fewer rows buy no time there -- and the
//   per-graph lists stay what small batches always had.  Results are bit-identical either way.
//   Where the batch shares one representative the sampler takes it from a table it builds ahead of the loop, one entry per schedule
//   index (DD_TABLE, option "dedup_table", build_pure_table): the window's rows depend on the weights and the step's row only.
//   Trimming (bit k of *trim): level k's fill may leave out what nobody reads only when every later reader of its activation,
//   statistics and skip goes through a list -- level k + 1 is deduplicated by the same forward (its merge takes the run list) and,
//   from level 1 on, the up stage reads the skip through a coarse list (levels 0 .. k then have single unshifted blocks, down and up
//   alike, so that list stays inside non-pure windows).  Without a coarse list the skip is read whole and the level is filled completely.
// * Forward time (forward_fixed): nothing is decided.  The lists are whatever the last staging wrote; under DD_BATCH the forward
//   checks that it runs at the depth they were trimmed for and reads the batch-uniform row.
bool dedup_opts_on(dsg_handle h) {
    if (h->P != 1 || !h->opt.dedup_masked || !prune_opts_on(h) || prune_plan(h).np.dd_n == 0) return false;
    const BlockPlan &b0 = h->down[0][0];
    return h->opt.fused_patch_embed && h->pe_wp && (h->Kp == 32 || h->Kp == 64) && h->opt.fused_attn && b0.wqp && h->opt.fused_mlp && b0.w1p &&
           b0.C <= h->opt.fused_mlp_maxc;
}
// how many levels may deduplicate (option "dedup_levels": 0 = every qualifying one), the finest included; 0 when none does
int dedup_levels(dsg_handle h) {
    if (!dedup_opts_on(h)) return 0;
    int n = 1;
    if (h->opt.fused_merge != 0 && rowstats_on(h) && !h->opt.gemm_bf16)
        while (n < prune_plan(h).np.dd_n && (h->E << (n - 1)) % 32 == 0) n++;
    return h->opt.dedup_levels > 0 ? std::min(n, h->opt.dedup_levels) : n;
}
int dedup_chain_depth(dsg_handle h, const Workspace *w) {
    if (!w->dd_rep || !prune_on(h, w)) return 0;
    const int n = dedup_levels(h);
    int depth = std::min(n, 1);
    while (depth < n && merge_fused_at(h, w->B, depth - 1)) depth++;   // (the plan has made sure of the blocks: build_prune_plan)
    return depth;
}
// Option "dedup_qkv": block j of level l projects QKV over the distinct rows only (run_block, the split form) when it stands directly
// behind the deduplicated first block of a level of this forward's chain -- the fill has just left every pure window of a content class
// with equal rows and statistics --, is shifted (an unshifted block would have been deduplicated whole) and takes the fused QKV +
// attention GEMM on 8 x 8 windows in fp32.  Which form runs is then the device's choice from the staged lists (kernels.h: qk_split_rule).
// the rows the rule compares the listed rows with: the launch's M; "dedup_qkv" 2 (measurement of the rule's bound) takes the split form always
int qk_rule_rows(dsg_handle h, int M) { return h->opt.dedup_qkv == 2 ? 0x7fffffff : M; }
bool qkv_dedup_at(dsg_handle h, const Workspace *w, int l, int j, int depth) {
    if (j != 1 || l >= depth || l > NEED_MAX_DD_UP || !h->opt.dedup_qkv || !dedup_opts_on(h) || w->need.qk_runs[l] < 0 || w->need.qk_src[l] < 0) return false;
    const BlockPlan &b = h->down[l][1];
    return b.shift > 0 && b.ws == 8 && !(h->opt.fused_attn && b.wqp) && h->opt.fused_qkv_attn && !h->opt.gemm_bf16 && !h->opt.gemm_split;
}
constexpr int DEDUP_BATCH_MIN = 16;
int dedup_stage_mode(dsg_handle h, const Workspace *w, bool zero_padded, bool uniform_row, int *trim, int *depth, bool table = false) {
    *trim = 0; *depth = 0;
    if (!zero_padded) return DD_OFF;
    const int d = dedup_chain_depth(h, w);
    if (!uniform_row || d == 0 || h->opt.dedup_batch == 0 || (h->opt.dedup_batch == 1 && w->B < DEDUP_BATCH_MIN)) return DD_GRAPH;
    *depth = d;
    const PrunePlan &pp = prune_plan(h);
    for (int k = 0; k + 1 < d; k++)
        if (k == 0 || pp.coarse[h->L - k] >= 0) *trim |= 1 << k;
    // `table`: the caller has built this call's table of pure-window rows (sample_impl): nothing computes the shared representative
    return table && h->opt.dedup_table && w->tab_pure ? DD_TABLE : DD_BATCH;
}
struct NeedRef { const int *list = nullptr, *cnt = nullptr; int id = -1; };
NeedRef need_ref(dsg_handle h, const Workspace *w, int id) {
    if (id < 0 || !prune_on(h, w)) return NeedRef();
    return NeedRef{w->need_lists + w->need.list_off[id], w->need_cnt + id, id};
}
struct BlockNeed { NeedRef rows, wins; NeedRef qk_runs = NeedRef(), qk_src = NeedRef(); };   // qk_*: qkv_dedup_at
// attach "modulate for block nb + row statistics" to the GEMM that writes nb's input (M rows = B * T tokens of nb's level)
void attach_premod(dsg_handle h, Workspace *w, GemmArgs &g, const BlockPlan *nb) {
    if (!wants_premod(h, nb)) return;
    g.stats_out = w->stats;
    g.mod_aff = w->aff; g.mod_ld = w->aff_ld; g.mod_off = nb->aff_off; g.mod_T = nb->res * nb->res;
}

// One Swin block (diffusesg.py:232-277) on x [B*T, C] in place.  premod: x is already modulated and w->stats holds the LN1
// partials (attach_premod on the producer).  next: the block that consumes this block's output directly (same width), or null.
// want_stats: leave (sum, sumsq) partials of the block's OUTPUT rows in w->stats even without a next block (PatchMerging
// reads them).  Returns what the producer left behind: .premod -- next's input is pre-modulated (+ its LN1 partials);
// .stats_parts -- > 0: partials of the un-modulated output rows with that many pairs per row.
struct BlockOut { bool premod; int stats_parts; };
BlockOut run_block(dsg_handle h, Workspace *w, const BlockPlan &b, bool premod, const BlockPlan *next, bool want_stats, hipStream_t s,
                   const BlockNeed &need = BlockNeed()) {
    const int B = w->B, T = b.res * b.res, C = b.C, M = B * T, Hd = h->cfg.mlp_ratio * C;
    const std::string &p = b.prefix;
    const bool fuse = rowstats_on(h);
    const bool mlp_fused = h->opt.fused_mlp && b.w1p && C <= h->opt.fused_mlp_maxc;
    // bf16 mode: a tensor whose only consumer is the bf16 GEMM (which rounds its A operand to bf16 on the way into LDS) is stored as
    // bf16 by its producer -- same values bit for bit, half the bytes, no conversion in the consumer (kernels_lp.hip ABF / CBF)
    auto bf16_tensor_ok = [&](const float *W, int K) {
        return h->opt.gemm_bf16 && !h->opt.gemm_split && h->opt.bf16_act && K % 64 == 0 && h->taps.empty() && bf16_of(h, W) != nullptr;
    };
    GemmArgs g;
    if (h->opt.fused_attn && b.wqp) {
        // modulate+SiLU, LN1, QKV, window attention, proj and the residual in one register-resident kernel
        WinGeom wg{b.res, b.ws, b.shift, b.heads, C};
        h->prof_next_list = need.wins.id;
        P_KERN(PK_FUSED, 2.0 * (double)M * C * 4.0 * C + 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C,
               launch_fused_attn96(w->x, w->aff, w->aff_ld, b.aff_off, WT(h, p + ".norm1.weight"), WT(h, p + ".norm1.bias"), b.wqp,
                                   b.bqkv_s, b.biasT, b.wpp, WT(h, p + ".attn.proj.bias"), B, wg, premod, s, need.wins.list, need.wins.cnt));
    } else {
        // x <- silu(shift + x*(1+scale)) (also the shortcut), LayerNorm-1 statistics
        if (!premod) P_KERN(PK_ROW, 0.0, launch_mod_stats(w->x, w->aff, w->aff_ld, b.aff_off, w->stats, B, T, C, s));
        g.A = w->x; g.lda = C; g.K1 = C; g.K = C; g.M = M;
        if (premod) { g.ln_part = w->stats; g.ln_nparts = (C + 95) / 96; }
        else g.ln_stats = w->stats;   // gamma/beta of norm1 are folded into qkv_wf / qkv_bf
        g.W = b.qkv_wf; g.bias = b.qkv_bf; g.N = 3 * C;
        WinGeom wg{b.res, b.ws, b.shift, b.heads, C};
        bool attn_done = false, att_bf16 = false;
        if (h->opt.fused_qkv_attn && (b.ws == 8 || b.ws == 10) && !h->opt.gemm_bf16 && !h->opt.gemm_split) {
            // LN1 -> QKV -> softmax(q k^T + bias) v in one kernel: q, k, v of (two windows, one head) stay in LDS
            g.attn_bias = b.biasT; g.wg = wg; g.attn_batch = B; g.C = w->att; g.ldc = C;
            g.row_list = need.wins.list; g.row_cnt = need.wins.cnt;   // (a window list here)
            h->prof_next_list = need.wins.id;
            g.qk_cnt = need.qk_runs.cnt; g.qk_M = qk_rule_rows(h, M);   // "dedup_qkv": this launch returns at once where the split form below runs
            if (need.qk_runs.list) h->prof_next_qk = {need.qk_runs.id, g.qk_M, 1};
            char tg_[96];
            if (h->prof_stamps && h->prof_gemm && h->prof_gemm_used < h->prof_gemm_cap) g.prof = h->prof_gemm + 4 * (h->prof_gemm_used++);
            if (h->prof_on) snprintf(tg_, sizeof(tg_), "gemm+attn M=%d N=%d K=%d ln=%d heads=%d", g.M, g.N, g.K, g.ln_part ? 2 : 1, b.heads);
            ProfScope ps_(h, s, PK_GEMM, 2.0 * (double)M * 3.0 * C * C + 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C, tg_);
            attn_done = launch_gemm_qkv_attn(g, s);
        }
        if (attn_done && need.qk_runs.list) {
            // the split form (qkv_dedup_at; rule and lists: kernels.h): q, k, v of the listed rows -- LayerNorm in the A path from the
            // same statistics, the fused kernel's K order and bias add -- into w->qkv, then the fused kernel's attention phase from there
            // through the window map.  Both launches return at once where the fused launch above runs.
            GemmArgs q;
            q.A = w->x; q.lda = C; q.K1 = C; q.K = C; q.M = M; q.N = 3 * C;
            q.ln_part = g.ln_part; q.ln_nparts = g.ln_nparts; q.ln_stats = g.ln_stats;
            q.W = b.qkv_wf; q.bias = b.qkv_bf; q.C = w->qkv; q.ldc = 3 * C;
            q.row_list = need.qk_runs.list; q.row_cnt = need.qk_runs.cnt; q.qk_cnt = need.qk_runs.cnt; q.qk_M = g.qk_M;
            h->prof_next_list = need.qk_runs.id; h->prof_next_qk = {need.qk_runs.id, g.qk_M, 2};
            P_GEMM(q);
            GemmArgs a = g;
            a.prof = nullptr;
            h->prof_next_qk = {need.qk_runs.id, g.qk_M, 2};
            char ta_[96];
            if (h->prof_on) snprintf(ta_, sizeof(ta_), "attn(map) M=%d C=%d heads=%d", M, C, b.heads);
            ProfScope pa_(h, s, PK_ATTN, 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C, ta_);
            if (!launch_window_attn_map(a, w->qkv, need.qk_src.list, s)) plan_fail(h, "%s: attention through the window map not built", p.c_str());
        }
        if (!attn_done && (need.wins.list || need.qk_runs.list)) plan_fail(h, "%s: fused QKV + window attention with a window list not built", p.c_str());
        if (!attn_done) {
            g.attn_bias = nullptr; g.prof = nullptr; g.row_list = nullptr; g.row_cnt = nullptr;
            g.C = w->qkv; g.ldc = 3 * C;
            att_bf16 = bf16_tensor_ok(WT(h, p + ".attn.proj.weight"), C);
            // level 2: q, k, v leave the QKV GEMM as bf16 too (the attention math stays fp32 on the widened values; this one
            // changes results -- within the bf16 mode's stated bar -- because the fp32 attention kernel is the consumer)
            const bool qkv_bf16 = att_bf16 && h->opt.bf16_act >= 2 && bf16_of(h, b.qkv_wf) != nullptr;
            g.c_bf16 = qkv_bf16;
            P_GEMM_LP(g);
            P_KERN(PK_ATTN, 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C,
                   if (!launch_window_attn(w->qkv, b.biasT, w->att, B, wg, s, att_bf16, qkv_bf16))
                       plan_fail(h, "%s: window attention not built (window %d, C=%d, bf16 in/out=%d/%d)", p.c_str(), b.ws, C, qkv_bf16, att_bf16));
        }
        g = GemmArgs();
        g.A = w->att; g.lda = C; g.K1 = C; g.K = C; g.M = M; g.N = C;
        g.a_bf16 = att_bf16;
        g.W = WT(h, p + ".attn.proj.weight"); g.bias = WT(h, p + ".attn.proj.bias");
        g.res = w->x; g.ldres = C; g.C = w->x; g.ldc = C;
        if (fuse && !mlp_fused) g.stats_out = w->stats;   // LN2 partials of x + proj(...)
        g.row_list = need.rows.list; g.row_cnt = need.rows.cnt; h->prof_next_list = need.rows.id;
        P_GEMM_LP(g);
    }
    if (mlp_fused) {
        // LN2 + fc1 + GELU + fc2 + residual in one kernel, hidden activations never leave the register file
        const bool st = want_stats && fuse;
        h->prof_next_list = need.rows.id;
        P_KERN(PK_FUSED, 4.0 * (double)M * (double)C * (double)Hd,
               launch_fused_mlp(w->x, WT(h, p + ".norm2.weight"), WT(h, p + ".norm2.bias"), b.w1p, WT(h, p + ".mlp.fc1.bias"), b.w2p,
                                WT(h, p + ".mlp.fc2.bias"), M, C, st ? w->stats : nullptr, s, need.rows.list, need.rows.cnt));
        return BlockOut{false, st ? 1 : 0};   // the fused MLP has no modulate epilogue: the next block runs its own mod_stats
    }
    const bool ln2_part = fuse && !(h->opt.fused_attn && b.wqp);   // the proj GEMM above left the partials
    if (!ln2_part) P_KERN(PK_ROW, 0.0, launch_ln_stats(w->x, w->stats, M, C, s));
    g = GemmArgs();
    g.A = w->x; g.lda = C; g.K1 = C; g.K = C; g.M = M; g.N = Hd;
    if (ln2_part) { g.ln_part = w->stats; g.ln_nparts = (C + 95) / 96; }
    else g.ln_stats = w->stats;   // gamma/beta of norm2 are folded into fc1_wf / fc1_bf
    g.W = b.fc1_wf; g.bias = b.fc1_bf; g.act = ACT_GELU;
    g.C = w->hid; g.ldc = Hd;
#ifdef DSG_MEASURE
    // measurement only (DSG_HID_EXP=1, wrong results): a leading dimension of 0 gives the kernels an empty buffer range -- fc1's stores of the
    // 4C-wide hidden tensor are dropped and fc2's loads of it return zeros without memory traffic, every instruction still issues: the
    // upper bound of what a fused fc1 -> GELU -> fc2 kernel could gain by keeping the hidden tensor on the chip (profiles/r4/fp32_upper_bounds.txt).
    // Not in the product build: `make CXXFLAGS+=-DDSG_MEASURE` brings it back for such runs
    static const bool hid_exp = getenv("DSG_HID_EXP") != nullptr;
    if (hid_exp) g.ldc = 0;
#endif
    const bool hid_bf16 = bf16_tensor_ok(WT(h, p + ".mlp.fc2.weight"), Hd) && bf16_of(h, b.fc1_wf) != nullptr;
    g.c_bf16 = hid_bf16;
    g.row_list = need.rows.list; g.row_cnt = need.rows.cnt; h->prof_next_list = need.rows.id;
    P_GEMM_LP(g);
    g = GemmArgs();
    g.A = w->hid; g.lda = Hd; g.K1 = Hd; g.K = Hd; g.M = M; g.N = C;
#ifdef DSG_MEASURE
    if (hid_exp) g.lda = 0;
#endif
    g.a_bf16 = hid_bf16;
    g.W = WT(h, p + ".mlp.fc2.weight"); g.bias = WT(h, p + ".mlp.fc2.bias");
    g.res = w->x; g.ldres = C; g.C = w->x; g.ldc = C;
    attach_premod(h, w, g, next);
    const bool st = !g.stats_out && want_stats && fuse;
    if (st) g.stats_out = w->stats;   // plain row statistics of the output (EPI 1)
    g.row_list = need.rows.list; g.row_cnt = need.rows.cnt; h->prof_next_list = need.rows.id;
    P_GEMM_LP(g);
    return BlockOut{g.mod_aff != nullptr, st ? (C + 95) / 96 : 0};
}

// PositionalEmbedding + map_layer0/1 + all affine linears for `rows` noise labels (diffusesg.py:768-771, :238, :574)
void embed_rows(dsg_handle h, const float *c_noise, int rows, float *pe, float *emb0, float *emb, float *aff, hipStream_t s) {
    const int E = h->E;
    P_KERN(PK_ELEM, 0.0, launch_noise_pe(c_noise, pe, rows, E, s));
    GemmArgs g;
    g.A = pe; g.lda = E; g.K1 = E; g.K = E; g.M = rows; g.N = NOISE_EMB; g.act = ACT_SILU;
    g.W = WT(h, "map_layer0.weight"); g.bias = WT(h, "map_layer0.bias"); g.C = emb0; g.ldc = NOISE_EMB;
    P_GEMM(g);
    g.A = emb0; g.lda = NOISE_EMB; g.K1 = NOISE_EMB; g.K = NOISE_EMB;
    g.W = WT(h, "map_layer1.weight"); g.bias = WT(h, "map_layer1.bias"); g.C = emb;
    P_GEMM(g);
    g = GemmArgs();
    g.A = emb; g.lda = NOISE_EMB; g.K1 = NOISE_EMB; g.K = NOISE_EMB; g.M = rows; g.N = h->aff_n;
    g.W = h->aff_w; g.bias = h->aff_b; g.C = aff; g.ldc = h->aff_n;
    P_GEMM(g);
}

// input assembly + PatchEmbed (diffusesg.py:784-802, 562-577) -> w->x.  Returns true when the first block's modulate+SiLU rode
// along (fused kernel only).  fp32 path: only when that block is the fused C = 96 attention kernel (which then skips it);
// any_first_block: whatever the first block is (the bf16 block pipeline normalises the modulated tensor in its own row pass).
bool patch_embed_stage(dsg_handle h, Workspace *w, bool fp32_rule, hipStream_t s, bool *xn_done = nullptr, const NeedRef &pe_runs = NeedRef()) {
    const dsg_config &c = h->cfg;
    const int B = w->B, N = h->N, E = h->E, T0 = h->R0 * h->R0;   // N: the state's side; T0: level-0 tokens
    GemmArgs g;
    bool pe_done = false, pe_premod = false;
    // (a guide's forward inside its main handle's call reads the main workspace's c_in x)
    const float *in_adj = w->ext_in_adj ? w->ext_in_adj : w->in_adj, *in_node = w->ext_in_node ? w->ext_in_node : w->in_node;
    if (h->opt.fused_patch_embed && h->pe_wp) {
        h->prof_next_list = pe_runs.id;
        ProfScope ps_(h, s, PK_FUSED, 2.0 * (double)B * T0 * E * h->Cin, "launch_fused_patch_embed96");
        // the first block's modulate+SiLU rides along when that block is the fused C = 96 attention kernel (which then skips it)
        const BlockPlan *b0 = h->down[0].empty() ? nullptr : &h->down[0][0];
        pe_premod = wants_premod(h, b0) && (fp32_rule ? (h->opt.fused_attn && b0->wqp) : true);
        if (h->P == 2)
            pe_done = launch_fused_patch_embed96_p2(in_adj, in_node, w->cur_sc_adj, w->cur_sc_node, w->cur_has_sc, w->flags, h->pe_wp,
                                                    WT(h, "patch_embed.proj.bias"), WT(h, "patch_embed.norm.weight"), WT(h, "patch_embed.norm.bias"),
                                                    w->aff, w->aff_ld, h->pe_aff_off, pe_premod ? b0->aff_off : -1, w->x, B, N, h->Ca, h->Cn,
                                                    c.self_condition, h->pe_kps, s);
        else
        pe_done = launch_fused_patch_embed96(in_adj, in_node, w->cur_sc_adj, w->cur_sc_node, w->cur_has_sc, w->flags, h->pe_wp,
                                             WT(h, "patch_embed.proj.bias"), WT(h, "patch_embed.norm.weight"),
                                             WT(h, "patch_embed.norm.bias"), w->aff, w->aff_ld, h->pe_aff_off, pe_premod ? b0->aff_off : -1,
                                             w->x, B, N, h->Ca, h->Cn, c.self_condition, h->Kp, s, (xn_done && pe_premod) ? w->xn : nullptr,
                                             pe_runs.list, pe_runs.cnt);
        if (pe_runs.list && !pe_done) plan_fail(h, "patch_embed: fused kernel with a run list not built (Kp=%d)", h->Kp);
        pe_premod = pe_premod && pe_done;
        if (xn_done) *xn_done = pe_premod;
    }
    if (!g_dry_run) w->patch_fwd[0] = pe_done ? 1 : 0;
    if (!pe_done) {
        if (h->P > 1)   // the p^2 sub-pixels' channels side by side: the strided convolution is the same GEMM over R0^2 tokens
            P_KERN(PK_ELEM, 0.0, if (!launch_assemble_patch(in_adj, in_node, w->cur_sc_adj, w->cur_sc_node, w->cur_has_sc, w->flags, w->tok_in, B,
                                                            N, h->P, h->Ca, h->Cn, c.self_condition, h->Kp, s))
                                     plan_fail(h, "patch_embed: assembly refused (N=%d patch_size=%d Kp=%d)", N, h->P, h->Kp));
        else
            P_KERN(PK_ELEM, 0.0, launch_assemble(in_adj, in_node, w->cur_sc_adj, w->cur_sc_node, w->cur_has_sc, w->flags, w->tok_in, B, N, h->Ca,
                                                 h->Cn, c.self_condition, h->Kp, s));
        g = GemmArgs();
        g.A = w->tok_in; g.lda = h->Kp; g.K1 = h->Kp; g.K = h->Kp; g.M = B * T0; g.N = E;
        g.W = h->pe_w; g.bias = WT(h, "patch_embed.proj.bias"); g.C = w->y; g.ldc = E;
        P_KERN(PK_GEMM, 2.0 * (double)g.M * (double)g.N * (double)h->Cin * h->P * h->P,   // padded K is not algorithmic work
               if (!launch_gemm(g, s)) plan_fail(h, "patch_embed.proj: GEMM not built (M=%d N=%d K=%d)", g.M, g.N, g.K));
        P_KERN(PK_ROW, 0.0, launch_ln_mod(w->y, WT(h, "patch_embed.norm.weight"), WT(h, "patch_embed.norm.bias"), w->aff, w->aff_ld, h->pe_aff_off,
                      w->x, B, T0, E, s));
    }
    return pe_premod;
}

// final norm + read_out + heads (diffusesg.py:758-761, :806-825): w->x -> (f_adj, f_node)
void readout_stage(dsg_handle h, Workspace *w, hipStream_t s) {
    const int B = w->B, N = h->N, E = h->E, T0 = h->R0 * h->R0, PP = h->P * h->P;
    GemmArgs g;
    const int M0 = B * T0, Mp = B * N * N;   // token rows (the final norm, read_out.0's input); pixel rows (everything behind it)
    const bool fused = h->opt.fused_readout && h->ro_fap && h->taps.empty();
    if (!g_dry_run) w->patch_fwd[1] = fused ? 1 : 0;
    if (fused && h->P == 2) {
        // the p = 2 form: LN(x) of 32 tokens held once, the folded chain once per sub-pixel, per-pixel masked stores, pooling partials per
        // (token row, column parity); then the node fc1 over pool_ext [B N, 256] with the row-parity weight: two strided-row launches
        P_KERN(PK_FUSED, 2.0 * (double)Mp * E * (E + 32.0),
               if (!launch_fused_readout96_p2(w->x, WT(h, "norm.weight"), WT(h, "norm.bias"), h->ro_fap, h->ro_fa, h->ro_f2p,
                                              WT(h, "readout_adj_mlp.fc2.bias"), w->flags, w->f_adj, w->pool_part, w->pool_ext, B, N, h->Ca, s))
                   plan_fail(h, "read-out: the fused p = 2 kernel refused N=%d C_adj=%d", N, h->Ca));
        for (int a = 0; a < 2; a++) {
            g = GemmArgs();
            g.A = w->pool_ext + (size_t)a * 256; g.lda = 512; g.K1 = 256; g.K = 256; g.M = B * N / 2; g.N = E; g.act = ACT_GELU;
            g.W = h->ro_gext2[a]; g.bias = WT(h, "readout_node_mlp.fc1.bias"); g.C = w->hn + (size_t)a * E; g.ldc = 2 * E;
            P_GEMM(g);
        }
        P_KERN(PK_ROW, 0.0, launch_head_node(w->hn, WT(h, "readout_node_mlp.fc2.weight"), WT(h, "readout_node_mlp.fc2.bias"), w->flags,
                                             w->f_node, B, N, E, h->Cn, s));
        return;
    }
    if (fused) {
        // the pooling partials of node row r go to slot (32-token tile) - (r N) / 32: where a graph's rows sit relative to the tiles, and with
        // it the order its partials are added in, is the same for every b only if a graph is a whole number of tiles
        if (h->opt.batch_invariant && T0 % 32 != 0)
            plan_fail(h, "batch_invariant: the fused read-out's pooling slots depend on a graph's position in the batch unless N * N is a multiple "
                         "of 32 (N = %d); set \"fused_readout\" = 0 or leave the option off", N);
        // one pass over x: LN, folded read_out+fc1, GELU, fc2, masked adjacency store; pooled LN(x) for the node head
        // (the bf16 block pipeline runs the two products of the read-out on the bf16 matrix pipe as well: option bf16_readout)
        const float *fap_b = (bx_on(h) && h->opt.bf16_readout && h->ro_fapb) ? (const float *)bf16_of(h, h->ro_fapb) : nullptr;
        const float *f2p_b = fap_b ? (const float *)bf16_of(h, h->ro_f2pb) : nullptr;
        const bool ro_bf = fap_b && f2p_b;
        // the list form, wherever the pruning runs and the plan has the list (need_ref): the tiles with a valid pair, packed at the front
        // of the same grid.  "prune_masked" 0, debug taps and the split / bf16 modes keep the positional form
        const NeedRef tiles = ro_bf ? NeedRef() : need_ref(h, w, w->need.ro_tiles);
        if (!g_dry_run) w->ro_fwd = tiles.list ? 1 : 0;
        h->prof_next_list = tiles.id;
        h->prof_next_form = tiles.list ? " form=list" : " form=pos";
        P_KERN(PK_FUSED, 2.0 * (double)M0 * E * (E + 32.0),
               launch_fused_readout96(w->x, WT(h, "norm.weight"), WT(h, "norm.bias"), ro_bf ? fap_b : h->ro_fap, h->ro_fa, ro_bf ? f2p_b : h->ro_f2p,
                                      WT(h, "readout_adj_mlp.fc2.bias"), w->flags, w->f_adj, w->pool_part, w->pool_ext, B, N, h->Ca, s, ro_bf,
                                      tiles.list, tiles.cnt));
        g = GemmArgs();
        g.A = w->pool_ext; g.lda = 128; g.K1 = 128; g.K = 128; g.M = B * N; g.N = E; g.act = ACT_GELU;
        g.W = h->ro_gext; g.bias = WT(h, "readout_node_mlp.fc1.bias"); g.C = w->hn; g.ldc = E;
        P_GEMM(g);
        P_KERN(PK_ROW, 0.0, launch_head_node(w->hn, WT(h, "readout_node_mlp.fc2.weight"), WT(h, "readout_node_mlp.fc2.bias"), w->flags,
                                             w->f_node, B, N, E, h->Cn, s));
        return;
    }
    // faithful chain (diffusesg.py:758-761): final norm, three 1x1 convs
    P_KERN(PK_ROW, 0.0, launch_ln_stats(w->x, w->stats, M0, E, s));
    g = GemmArgs();
    g.A = w->x; g.lda = E; g.K1 = E; g.K = E; g.M = M0; g.N = E;
    g.ln_stats = w->stats;   // final norm's gamma/beta folded into ro0_wf / ro0_bf
    // patch_size p: p^2 E output columns, (a p + b) E + o -- the [M0, p^2 E] result is r0 [Mp, E] with rows in (token, a, b) order
    g.N = PP * E;
    g.W = h->ro0_wf; g.bias = h->ro0_bf; g.C = w->y; g.ldc = PP * E;
    P_GEMM(g);
    g = GemmArgs();
    g.A = w->y; g.lda = E; g.K1 = E; g.K = E; g.M = Mp; g.N = E;
    g.W = WT(h, "read_out.1.weight"); g.bias = WT(h, "read_out.1.bias"); g.C = w->att; g.ldc = E;
    P_GEMM(g);
    g.A = w->att; g.W = WT(h, "read_out.2.weight"); g.bias = WT(h, "read_out.2.bias"); g.C = w->y;
    P_GEMM(g);  // y = shared_rep, token-major
    if (h->P == 1) tap(h, "read_out", w->y, (size_t)M0 * E, s);
    else if (!g_dry_run)   // the tap is in pixel order [B, N^2, E]: un-shuffle the (token, a, b) rows on the way out (debug taps only)
        for (auto &t : h->taps)
            if (t.name == "read_out" && (int64_t)Mp * E <= t.cap)
                for (int ab = 0; ab < PP; ab++)   // sub-pixel (a, b): a strided 3-D copy [B R0][R0][E floats] per pixel row
                    for (int ti = 0; ti < B * h->R0; ti++)
                        (void)hipMemcpy2DAsync(t.dst + (((size_t)ti * h->P + ab / h->P) * N + ab % h->P) * E, sizeof(float) * h->P * E,
                                               w->y + ((size_t)ti * h->R0 * PP + ab) * E, sizeof(float) * PP * E, sizeof(float) * E, h->R0,
                                               hipMemcpyDeviceToDevice, s);
    // adjacency head (diffusesg.py:806-809, :825)
    g.A = w->y; g.W = WT(h, "readout_adj_mlp.fc1.weight"); g.bias = WT(h, "readout_adj_mlp.fc1.bias"); g.act = ACT_GELU;
    g.C = w->att;
    P_GEMM(g);
    if (h->P > 1)   // rows in (token, a, b) order: the store and the pooling carry the map to (I, J) and mask per pixel
        P_KERN(PK_ROW, 0.0, if (!launch_head_adj_patch(w->att, WT(h, "readout_adj_mlp.fc2.weight"), WT(h, "readout_adj_mlp.fc2.bias"), w->flags, w->f_adj,
                                                       B, N, h->P, E, h->Ca, s)) plan_fail(h, "read-out: adjacency head refused (N=%d patch_size=%d)", N, h->P));
    else
        P_KERN(PK_ROW, 0.0, launch_head_adj(w->att, WT(h, "readout_adj_mlp.fc2.weight"), WT(h, "readout_adj_mlp.fc2.bias"), w->flags, w->f_adj, B, N,
                                            E, h->Ca, s));
    // node head (diffusesg.py:812-822)
    if (h->P > 1)
        P_KERN(PK_ELEM, 0.0, if (!launch_pool_patch(w->y, w->flags, w->pool, B, N, h->P, E, s)) plan_fail(h, "read-out: pooling refused (N=%d patch_size=%d)", N, h->P));
    else
        P_KERN(PK_ELEM, 0.0, launch_pool(w->y, w->flags, w->pool, B, N, E, s));
    g = GemmArgs();
    g.A = w->pool; g.lda = E; g.K1 = E; g.K = E; g.M = B * N; g.N = E; g.act = ACT_GELU;
    g.W = WT(h, "readout_node_mlp.fc1.weight"); g.bias = WT(h, "readout_node_mlp.fc1.bias"); g.C = w->hn; g.ldc = E;
    P_GEMM(g);
    P_KERN(PK_ROW, 0.0, launch_head_node(w->hn, WT(h, "readout_node_mlp.fc2.weight"), WT(h, "readout_node_mlp.fc2.bias"), w->flags, w->f_node, B, N,
                     E, h->Cn, s));
}

// ================= the bf16 block pipeline ("gemm_bf16" mode; kernels_bx.hip) =================
// Every tensor a GEMM reads is bf16 in HBM; the residual stream x stays fp32.  State of a level between two launches:
//   BX_RAW   x holds the un-modulated activation
//   BX_MOD   x holds silu(shift + x (1 + scale)) of the block about to run (its shortcut), w->xn is not valid yet
//   BX_READY x as BX_MOD and w->xn = LayerNorm-1 of it without affine (gamma / beta are folded into qkv_wf / qkv_bf)
enum BxState { BX_RAW = 0, BX_MOD = 1, BX_READY = 2 };
// (the pipeline's kernels are built and tested for embed_dim = 96 -- every configuration of the reference; any other width keeps
// round 2's kernels_lp.hip path instead of meeting an uncovered shape half-way through a forward, and get_option reports that)
bool bx_on(dsg_handle h) { return h->opt.gemm_bf16 && !h->opt.gemm_split && h->opt.bf16_pipe && h->E == 96; }

#define P_BX(g, tag)                                                                                                           \
    do {                                                                                                                       \
        char tg_[96];                                                                                                          \
        if (h->prof_on) snprintf(tg_, sizeof(tg_), "gemm_bx %s M=%d N=%d K=%d ln=%d", tag, (g).M, (g).N, (g).K, (g).ln_out);   \
        ProfScope ps_(h, s, PK_GEMM, 2.0 * (double)(g).M * (double)(g).N * (double)(g).K, tg_);                               \
        if (!launch_gemm_bx((g), s)) plan_fail(h, "bf16 pipeline: gemm_bx shape not covered (%s M=%d N=%d K=%d K1=%d ln=%d)", tag, (g).M, (g).N, (g).K, (g).K1, (g).ln_out); \
    } while (0)

bool bx_full_row(int C) { return C == 96 || C == 192 || C == 384; }   // widths a single GEMM tile spans: LayerNorm in the epilogue

// the "produce the next consumer's input" part of a GEMM that writes a level's activation x [M, C]: the next block's modulate+SiLU
// and its LayerNorm-1 as bf16 (full-row widths), or the plain bf16 copy (PatchBreakup reads the un-normalised tensor).  Returns the
// state x / xn are in after the launch plus whatever row pass finish_bx still has to run.
BxState attach_bx_out(dsg_handle h, Workspace *w, BxGemm &g, const BlockPlan *next, bool want_copy) {
    const bool fuse = h->taps.empty();   // taps want the un-modulated block outputs
    if (next && fuse) {
        g.mod_aff = w->aff; g.mod_ld = w->aff_ld; g.mod_off = next->aff_off; g.mod_T = next->res * next->res;
        if (bx_full_row(g.N)) { g.ln_out = 1; g.Cb = w->xn; g.ldcb = g.N; return BX_READY; }
        return BX_MOD;
    }
    if (!next && want_copy) { g.Cb = w->xn; g.ldcb = g.N; }
    return BX_RAW;
}

// One Swin block (diffusesg.py:232-277) on x [B*T, C] in place; `st`: what the producer left (above).  next / want_copy as run_block.
BxState run_block_bx(dsg_handle h, Workspace *w, const BlockPlan &b, BxState st, const BlockPlan *next, bool want_copy, hipStream_t s) {
    const int B = w->B, T = b.res * b.res, C = b.C, M = B * T, Hd = h->cfg.mlp_ratio * C;
    const std::string &p = b.prefix;
    // x <- silu(shift + x (1 + scale)) (also the shortcut) and LayerNorm-1 -> xn, whatever the producer has not done
    if (st == BX_RAW) P_KERN(PK_ROW, 0.0, launch_ln_bx(w->x, w->aff, w->aff_ld, b.aff_off, w->xn, B, T, C, true, s));
    else if (st == BX_MOD) P_KERN(PK_ROW, 0.0, launch_ln_bx(w->x, nullptr, 0, 0, w->xn, B, T, C, true, s));
    BxGemm g;
    WinGeom wg{b.res, b.ws, b.shift, b.heads, C};
    bool fused_qa = false;
    if (h->opt.bf16_qkv_attn && h->taps.empty()) {   // (the qkv tap wants the tensor)
        BxQkvAttn qa;
        qa.xn = w->xn; qa.W = bf16_of(h, b.qkv_wf); qa.bias = b.qkv_bf; qa.biasP = b.biasP; qa.out = w->att; qa.B = B; qa.g = wg;
        { auto it = h->w_qimg.find(b.qkv_wf); qa.Wimg = it == h->w_qimg.end() ? nullptr : it->second; }
        qa.biasF = b.biasF;
        // 10 x 10 windows: 1 the wave-per-unit kernel, 2 the block-per-head kernel (its A/B), 3 wave-per-unit only where a block lies in one window (heads % 4 == 0)
        qa.variant = (h->opt.bf16_qkv_attn == 2 || (h->opt.bf16_qkv_attn == 3 && b.heads % 4 != 0)) ? 1 : 0;
        ProfScope ps_(h, s, PK_ATTN, 2.0 * (double)M * 3.0 * C * C + 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C, "qkv_attn_bx");
        fused_qa = launch_qkv_attn_bx(qa, s);
    }
    if (!fused_qa) {
        g.A = w->xn; g.lda = C; g.K = C; g.M = M; g.N = 3 * C;
        g.W = bf16_of(h, b.qkv_wf); g.bias = b.qkv_bf; g.Cb = w->qkv; g.ldcb = 3 * C;
        P_BX(g, "qkv");
        ProfScope ps_(h, s, PK_ATTN, 4.0 * (double)M * (double)(b.ws * b.ws) * (double)C, "attn_bx");
        if (!launch_attn_bx(w->qkv, b.biasT, w->att, B, wg, s) && !launch_window_attn(w->qkv, b.biasT, w->att, B, wg, s, true, true))
            plan_fail(h, "bf16 pipeline: %s: window attention not built (window %d, C=%d)", p.c_str(), b.ws, C);
    }
    // the fused MLP kernel can take the proj linear, the residual and LayerNorm-2 in front (x + proj(att) never goes to HBM)
    const bool mlp_fused = h->opt.bf16_mlp && h->cfg.mlp_ratio == 4 && (C == 96 || C == 192 || (C == 384 && h->opt.bf16_mlp != 3));
    const bool proj_in_mlp = mlp_fused && h->opt.bf16_proj_mlp && h->taps.empty() && (C == 96 || C == 192 || (C == 384 && (h->opt.bf16_mlp == 1 || h->opt.bf16_mlp == 4 || h->opt.bf16_mlp == 5 || h->opt.bf16_mlp == 6)));
    const bool full = bx_full_row(C);
    if (!proj_in_mlp) {
        g = BxGemm();
        g.A = w->att; g.lda = C; g.K = C; g.M = M; g.N = C;
        g.W = bf16_of(h, WT(h, p + ".attn.proj.weight")); g.bias = WT(h, p + ".attn.proj.bias");
        g.res = w->x; g.ldres = C; g.C = w->x; g.ldc = C;
        if (full) { g.ln_out = 1; g.Cb = w->xn; g.ldcb = C; }   // LayerNorm-2 of x + proj(...) (gamma / beta folded into fc1_wf / fc1_bf)
        P_BX(g, "proj");
        if (!full) P_KERN(PK_ROW, 0.0, launch_ln_bx(w->x, nullptr, 0, 0, w->xn, B, T, C, true, s));
    }
    // fc1 -> GELU -> fc2 -> + residual (-> the next block's modulate / LayerNorm-1) in one kernel, no hidden tensor (measured at COCO
    // B = 512, tools/bx_bench.py: 324 us against 302 + 325 for the GEMM pair at C = 96, 270 against 193 + 196 at C = 192, and at C = 384
    // the eight-wave kernel mlp384_bx 199 against 111 + 152; the four-wave kernel at C = 384 -- option value 2, tests only -- needs
    // 230 + 192 registers, runs one wave per SIMD and loses to the pair: 312 us).  C = 768 (VG's deepest level) keeps the GEMM pair.
    if (mlp_fused) {
        BxMlp m;
        // C = 384: 1 -> the LDS-DMA kernel on pre-arranged weight images (round 4), 4 -> round 3's eight-wave kernel, 2 -> the four-wave one
        m.wide8 = h->opt.bf16_mlp == 2 ? 0 : (h->opt.bf16_mlp == 4 ? 2 : (h->opt.bf16_mlp == 5 ? 3 : 1));
        m.img = C == 384 ? img_of(h, b.fc1_wf) : nullptr;
        m.img2 = C == 384 ? img2_of(h, b.fc1_wf) : nullptr;
        if (C == 96 && h->opt.bf16_mlp == 6) { auto it = h->w_img96.find(b.fc1_wf); m.img96 = it == h->w_img96.end() ? nullptr : it->second; }   // (6: level 0 on the LDS-resident kernel -- measured at par, not the default)
        if (proj_in_mlp) { m.att = w->att; m.Wp = bf16_of(h, WT(h, p + ".attn.proj.weight")); m.bp = WT(h, p + ".attn.proj.bias"); }
        m.xn = w->xn; m.x = w->x; m.W1 = bf16_of(h, b.fc1_wf); m.b1 = b.fc1_bf;
        m.W2 = bf16_of(h, WT(h, p + ".mlp.fc2.weight")); m.b2 = WT(h, p + ".mlp.fc2.bias"); m.M = M; m.C = C;
        BxState out = BX_RAW;
        if (next && h->taps.empty()) {
            m.mod_aff = w->aff; m.mod_ld = w->aff_ld; m.mod_off = next->aff_off; m.mod_T = next->res * next->res;
            m.xn_out = w->xn; m.out_mode = 1; out = BX_READY;
        } else if (!next && want_copy) { m.xn_out = w->xn; m.out_mode = 2; }
        ProfScope ps_(h, s, PK_FUSED, 4.0 * (double)M * (double)C * (double)Hd + (proj_in_mlp ? 2.0 * (double)M * C * C : 0.0), proj_in_mlp ? "proj_mlp_bx" : "mlp_bx");
        if (!launch_mlp_bx(m, s)) plan_fail(h, "bf16 pipeline: %s: fused MLP shape not covered (M=%d C=%d proj=%d)", p.c_str(), M, C, (int)proj_in_mlp);
        return out;
    }
    g = BxGemm();
    g.A = w->xn; g.lda = C; g.K = C; g.M = M; g.N = Hd;
    g.W = bf16_of(h, b.fc1_wf); g.bias = b.fc1_bf; g.act = ACT_GELU; g.Cb = w->hid; g.ldcb = Hd;
    P_BX(g, "fc1");
    g = BxGemm();
    g.A = w->hid; g.lda = Hd; g.K = Hd; g.M = M; g.N = C;
    g.W = bf16_of(h, WT(h, p + ".mlp.fc2.weight")); g.bias = WT(h, p + ".mlp.fc2.bias");
    g.res = w->x; g.ldres = C; g.C = w->x; g.ldc = C;
    const BxState out = attach_bx_out(h, w, g, next, want_copy);
    P_BX(g, "fc2");
    return out;
}

// DiffuseSG.forward in the bf16 block pipeline; same structure (and the same fp32 noise embedding, PatchEmbed, read-out and heads)
// as forward_fixed below
void forward_fixed_bx(dsg_handle h, Workspace *w, hipStream_t s) {
    const int B = w->B, N = h->N, E = h->E, L = h->L, T0 = N * N;
    char name[64];
    BxGemm g;
    w->aff_ld = w->uniform ? 0 : h->aff_n;
    if (!w->uniform) embed_rows(h, w->c_noise, B, w->pe, w->emb0, w->emb, w->aff, s);
    bool xn_done = false;   // the fused PatchEmbed kernel also leaves block 0's LayerNorm-1 input when it applies that block's modulate
    BxState st = patch_embed_stage(h, w, false, s, &xn_done) ? (xn_done ? BX_READY : BX_MOD) : BX_RAW;
    tap(h, "patch_embed", w->x, (size_t)B * T0 * E, s);
    // encoder (diffusesg.py:745-748); skips are stored as bf16 (their only reader is PatchBreakup's pre_linear)
    for (int l = 0; l < L; l++) {
        const int C = E << l, res = N >> l, T = res * res;
        for (size_t j = 0; j < h->down[l].size(); j++) {
            const BlockPlan *next = j + 1 < h->down[l].size() ? &h->down[l][j + 1] : (l == L - 1 && !h->up[0].empty() ? &h->up[0][0] : nullptr);
            st = run_block_bx(h, w, h->down[l][j], st, next, false, s);   // (PatchMerging gathers from the fp32 x: no bf16 copy needed)
            snprintf(name, sizeof(name), "down%d.block%d", l, (int)j);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
        if (l < L - 1) {
            const std::string p = "down_layers." + std::to_string(l) + ".downsample";
            // 2x2 gather + LayerNorm(4C) -> bf16 [B*T/4, 4C] (in w->hid), then the reduction; its epilogue stores the skip copy and
            // prepares the next level's first block
            P_KERN(PK_ROW, 0.0, launch_merge_ln(w->x, WT(h, p + ".norm.weight"), WT(h, p + ".norm.bias"), w->hid, B, res, C, s, true));
            g = BxGemm();
            g.A = w->hid; g.lda = 4 * C; g.K = 4 * C; g.M = B * T / 4; g.N = 2 * C;
            g.W = bf16_of(h, WT(h, p + ".reduction.weight")); g.C = w->x; g.ldc = 2 * C;
            g.C2b = w->skips[l]; g.ldc2b = 2 * C;
            st = attach_bx_out(h, w, g, h->down[l + 1].empty() ? nullptr : &h->down[l + 1][0], false);
            P_BX(g, "merge");
        }
        snprintf(name, sizeof(name), "down%d", l);
        tap(h, name, w->x, l < L - 1 ? (size_t)B * (T / 4) * 2 * C : (size_t)B * T * C, s);
    }
    // decoder (diffusesg.py:751-756)
    for (int i = 0; i < L; i++) {
        const int l = L - 1 - i, C = E << l, res = N >> l, T = res * res;
        if (i > 0) {
            const std::string p = "up_layers." + std::to_string(i) + ".upsample";
            const int D = 4 * C, Tc = T / 4;
            // pre_linear on cat([x, skip]): x's bf16 copy was left in w->xn by the previous level's last block, the skip is bf16
            g = BxGemm();
            g.A = w->xn; g.lda = D / 2; g.K1 = D / 2; g.A2 = w->skips[l]; g.lda2 = D / 2; g.K = D; g.M = B * Tc; g.N = D;
            g.W = bf16_of(h, WT(h, p + ".pre_linear.weight")); g.C = w->hid; g.ldc = D;
            P_BX(g, "pre_linear");
            P_KERN(PK_ROW, 0.0, launch_breakup_ln(w->hid, WT(h, p + ".norm.weight"), WT(h, p + ".norm.bias"), WT(h, p + ".post_norm.weight"),
                              WT(h, p + ".post_norm.bias"), w->y, B, res / 2, D, s, true));
            g = BxGemm();
            g.A = w->y; g.lda = C; g.K = C; g.M = B * T; g.N = C;
            g.W = bf16_of(h, WT(h, p + ".post_linear.weight")); g.C = w->x; g.ldc = C;
            st = attach_bx_out(h, w, g, h->up[i].empty() ? nullptr : &h->up[i][0], false);
            P_BX(g, "post_linear");
            snprintf(name, sizeof(name), "up%d.upsample", i);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
        for (size_t j = 0; j < h->up[i].size(); j++) {
            const BlockPlan *next = j + 1 < h->up[i].size() ? &h->up[i][j + 1] : nullptr;   // then PatchBreakup / the read-out
            st = run_block_bx(h, w, h->up[i][j], st, next, /*want_copy=*/i + 1 < L, s);
            snprintf(name, sizeof(name), "up%d.block%d", i, (int)j);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
        if (h->up[i].empty() && i + 1 < L)   // a level without blocks: PatchBreakup still needs x's bf16 copy
            P_KERN(PK_ROW, 0.0, launch_ln_bx(w->x, nullptr, 0, 0, w->xn, B, T, C, false, s));
    }
    readout_stage(h, w, s);
}

// One entry of the sampler's table of pure-window rows (kernels.h, "The table"; build_pure_table): per level of the plan's chain the 64
// rows of x, from level 1 on the same rows of the skip, and room for the rows' (sum, sumsq) pairs at their widest
struct PureTabLayout { size_t stride = 0; int off_x[1 + NEED_MAX_DD_UP] = {}, off_skip[1 + NEED_MAX_DD_UP] = {}, off_st[1 + NEED_MAX_DD_UP] = {}; };
PureTabLayout pure_tab_layout(dsg_handle h) {
    PureTabLayout t;
    int o = 0;
    for (int k = 0; k < prune_plan(h).np.dd_n; k++) {
        const int C = h->E << k;
        t.off_x[k] = o; o += 64 * C;
        t.off_skip[k] = o; if (k > 0) o += 64 * C;
        t.off_st[k] = o; o += 64 * 2 * ((C + 95) / 96);
    }
    t.stride = (size_t)o;
    return t;
}
// a forward that builds table entries: w->aff holds one staged (scale, shift) row per graph, the forward returns behind the first
// block of level `stop` and stores window 0 of the first n graphs at every level up to there as entries dst[0 .. n)
struct TabBuild { int stop; float *dst; int n; };

// DiffuseSG.forward on the workspace's fixed buffers: (in_adj,in_node,sc_*,flags,c_noise) -> (f_adj,f_node)
// patch_size > 1 runs the fp32 kernels only: the option that cannot run there, or null
const char *patch_refused_option(dsg_handle h) {
    if (h->P == 1) return nullptr;
    return h->opt.gemm_split ? "gemm_split" : h->opt.gemm_bf16 ? "gemm_bf16" : h->opt.batch_invariant ? "batch_invariant" : nullptr;
}

void forward_fixed(dsg_handle h, Workspace *w, hipStream_t s, const TabBuild *tb = nullptr) {
    if (const char *o = patch_refused_option(h)) {
        plan_fail(h, "option \"%s\" is not built at patch_size %d (patch_size > 1 runs the fp32 kernels only)", o, h->P);
        return;
    }
    if (bx_on(h)) { if (tb) plan_fail(h, "dedup_table: no table of pure-window rows in the bf16 pipeline"); else forward_fixed_bx(h, w, s); return; }
    // the fused PatchMerging writes the coarser level into the other activation buffer and swaps the two names; put them back
    // on every exit so that each forward (and each captured graph) starts from the same assignment
    struct SwapGuard { Workspace *w; float *x, *y; ~SwapGuard() { w->x = x; w->y = y; } } swap_guard{w, w->x, w->y};
    const int B = w->B, N = h->R0, E = h->E, L = h->L, T0 = N * N;   // N: the level-0 TOKEN resolution in this function
    char name[64];
    GemmArgs g;
    w->aff_ld = w->uniform ? 0 : h->aff_n;
    if (!w->uniform && !tb) {
        // noise embedding (diffusesg.py:768-771) and every block's (scale,shift) in one GEMM
        embed_rows(h, w->c_noise, B, w->pe, w->emb0, w->emb, w->aff, s);
    }
    const PureTabLayout ptl = pure_tab_layout(h);
    // pure-window deduplication of levels 0 .. depth - 1: the producer of level l's input (PatchEmbed, or the merge into the level) and
    // the level's first block take its unique lists, then the copy fills the other pure windows
    const int depth = dedup_chain_depth(h, w);
    // lists with one representative for the batch were trimmed for one chain depth and hold for batch-uniform forwards only
    if (depth > 0 && (w->dd_mode == DD_BATCH || w->dd_mode == DD_TABLE) && !g_dry_run) {
        if (depth != w->dd_depth) plan_fail(h, "dedup_batch: the forward deduplicates %d levels, the lists were staged for %d", depth, w->dd_depth);
        if (!w->uniform) plan_fail(h, "dedup_batch: a forward with per-sample noise labels under lists shared across the batch");
    }
    const bool pe_premod = patch_embed_stage(h, w, true, s, nullptr, depth > 0 ? need_ref(h, w, w->need.dd_runs[0]) : NeedRef());
    tap(h, "patch_embed", w->x, (size_t)B * T0 * E, s);
    // encoder (diffusesg.py:745-748)
    bool premod = pe_premod;   // is w->x already modulated for the next block (generic blocks: with LN1 partials in w->stats)?
    int merge_parts = 0;       // > 0: w->stats holds partials of the level's final output rows (for the fused PatchMerging)
    for (int l = 0; l < L; l++) {
        const int C = E << l, res = N >> l, T = res * res;
        for (size_t j = 0; j < h->down[l].size(); j++) {
            // the consumer of this block's output: the next block of the level; after the deepest level the first decoder
            // block (no upsample there); otherwise PatchMerging, which takes the un-modulated tensor
            const BlockPlan *next = j + 1 < h->down[l].size() ? &h->down[l][j + 1] : (l == L - 1 && !h->up[0].empty() ? &h->up[0][0] : nullptr);
            // the level's last block leaves row statistics for the fused PatchMerging
            const bool for_merge = !next && merge_fused_at(h, B, l);
            const bool dd = j == 0 && l < depth;   // the level's input came over its run list
            BlockNeed bn = dd ? BlockNeed{need_ref(h, w, w->need.dd_runs[l]), need_ref(h, w, w->need.dd_wins[l])} : BlockNeed();
            const bool qk = qkv_dedup_at(h, w, l, (int)j, depth);
            if (qk) { bn.qk_runs = need_ref(h, w, w->need.qk_runs[l]); bn.qk_src = need_ref(h, w, w->need.qk_src[l]); }
            if (j == 1 && l <= NEED_MAX_DD_UP && !g_dry_run) w->qk_fwd[l] = qk;
            const BlockOut bo = run_block(h, w, h->down[l][j], premod, next, for_merge, s, bn);
            premod = bo.premod; merge_parts = bo.stats_parts;
            // behind the copy x, the skip (level 0 has none yet) and the partials the next launch reads (a following block's LN1 partials
            // of the pre-modulated rows, or the output rows' partials for the next merge) hold what the full launches would have written
            const int parts = bo.premod ? (C + 95) / 96 : bo.stats_parts;
            if (dd) {
                const NeedRef cp = need_ref(h, w, w->need.dd_copy[l]);
                // (lists written under DD_TABLE: from the table entry of the running step; the launch is the same either way)
                PureTabSrc pt;
                if (w->tab_pure && !tb)
                    pt = PureTabSrc{w->tab_pure, ptl.stride, w->tab_pure_cap, ptl.off_x[l], ptl.off_skip[l], ptl.off_st[l], w->ext_step ? w->ext_step : h->tab_step,
                                    w->ext_ctl ? w->ext_ctl : w->ctl,
                                    w->dd_rep + (size_t)w->need.dd_n * B};
                P_KERN(PK_ELEM, 0.0, launch_window_broadcast(w->x, l ? w->skips[l - 1] : nullptr, parts > 0 ? w->stats : nullptr, parts, B, res, C,
                                                             cp.list, cp.cnt, w->dd_rep + (size_t)l * B, s, pt));
                if (tb)
                    P_KERN(PK_ELEM, 0.0, launch_window_harvest(w->x, l ? w->skips[l - 1] : nullptr, parts > 0 ? w->stats : nullptr, parts, tb->n, res, C,
                                                               tb->dst, ptl.stride, ptl.off_x[l], ptl.off_skip[l], ptl.off_st[l], s));
            }
            if (tb && j == 0 && l == tb->stop) {
                if (!dd) plan_fail(h, "dedup_table: level %d is not deduplicated by this forward", l);
                return;
            }
            if (j == 0 && l <= NEED_MAX_DD_UP && !g_dry_run) w->dd_fwd[l] = dd ? (parts > 0 ? 1 : 0) : -1;
            snprintf(name, sizeof(name), "down%d.block%d", l, (int)j);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
        if (l < L - 1) {
            const std::string p = "down_layers." + std::to_string(l) + ".downsample";
            g = GemmArgs();
            g.K1 = 4 * C; g.K = 4 * C; g.M = B * T / 4; g.N = 2 * C;
            // pure-window deduplication of level l + 1: only the merged rows of its unique windows
            const bool dd_next = l + 1 < depth;
            if (dd_next && merge_parts == 0) {   // (dedup_chain_depth promised the partial-statistics merge)
                plan_fail(h, "down%d: deduplicated by the chain depth, but level %d's last block left no merge partials", l + 1, l);
                return;
            }
            if (dd_next) {
                // the gather + LayerNorm(4C) of the listed merged rows into y -- the values the gather form below puts into its A
                // tile -- then the reduction over the same list, in place of the fine level (all of x has been read by then)
                const NeedRef mr = need_ref(h, w, w->need.dd_runs[l + 1]);
                P_KERN(PK_ROW, 0.0, launch_merge_norm_runs(w->x, w->stats, merge_parts, w->y, B, res, C, mr.list, mr.cnt, s));
                g.A = w->y; g.lda = 4 * C;
                g.W = h->merge_wf[l]; g.bias = h->merge_bf[l];
                g.C = w->x; g.ldc = 2 * C;
                g.row_list = mr.list; g.row_cnt = mr.cnt; h->prof_next_list = mr.id;
            } else if (merge_parts > 0) {
                // 2x2 gather, LayerNorm(4C) (statistics from the four source rows' partials, gamma/beta folded into the weight)
                // and the reduction in one GEMM: the merged [B*T/4, 4C] tensor is never written
                g.A = w->x; g.lda = C; g.a4_res = res; g.ln_part = w->stats; g.ln_nparts = merge_parts;
                g.W = h->merge_wf[l]; g.bias = h->merge_bf[l];
                g.C = w->y; g.ldc = 2 * C;   // cannot overwrite x while other tiles still gather from it: write y, then swap
            } else {
                P_KERN(PK_ROW, 0.0, launch_merge_ln(w->x, WT(h, p + ".norm.weight"), WT(h, p + ".norm.bias"), w->y, B, res, C, s));
                g.A = w->y; g.lda = 4 * C;
                g.W = WT(h, p + ".reduction.weight"); g.C = w->x; g.ldc = 2 * C;
            }
            g.C2 = w->skips[l]; g.ldc2 = 2 * C;
            attach_premod(h, w, g, h->down[l + 1].empty() ? nullptr : &h->down[l + 1][0]);   // the skip copy (C2) stays un-modulated
            P_GEMM_LP(g);
            premod = g.mod_aff != nullptr;
            if (dd_next && !premod) plan_fail(h, "down%d: the list form of PatchMerging needs the pre-modulating epilogue", l + 1);   // (mod_stats takes no list)
            if (merge_parts > 0 && !dd_next) std::swap(w->x, w->y);   // the new level's activation lives in the other buffer from here on
            merge_parts = 0;
        }
        snprintf(name, sizeof(name), "down%d", l);
        tap(h, name, w->x, l < L - 1 ? (size_t)B * (T / 4) * 2 * C : (size_t)B * T * C, s);
        // the deepest level's skip is popped and discarded by the first up layer (diffusesg.py:754-755)
    }
    // decoder (diffusesg.py:751-756); with masked-token pruning every launch behind the plan's cut takes its need list
    const PrunePlan &pp = prune_plan(h);
    for (int i = 0; i < L; i++) {
        const int l = L - 1 - i, C = E << l, res = N >> l, T = res * res;
        if (i > 0) {
            const std::string p = "up_layers." + std::to_string(i) + ".upsample";
            const int D = 4 * C, Tc = T / 4;  // coarse tokens, concatenated width
            const NeedRef coarse = need_ref(h, w, pp.coarse[i]), fine = need_ref(h, w, pp.fine[i]);
            g = GemmArgs();                   // pre_linear on cat([x, skip]) without materialising the concat
            g.A = w->x; g.lda = D / 2; g.K1 = D / 2; g.A2 = w->skips[l]; g.lda2 = D / 2; g.K = D; g.M = B * Tc; g.N = D;
            g.W = WT(h, p + ".pre_linear.weight"); g.C = w->hid; g.ldc = D;
            g.row_list = coarse.list; g.row_cnt = coarse.cnt; h->prof_next_list = coarse.id;
            P_GEMM_LP(g);
            P_KERN(PK_ROW, 0.0, launch_breakup_ln(w->hid, WT(h, p + ".norm.weight"), WT(h, p + ".norm.bias"), WT(h, p + ".post_norm.weight"),
                              WT(h, p + ".post_norm.bias"), w->y, B, res / 2, D, s, false, coarse.list, coarse.cnt));
            g = GemmArgs();
            g.A = w->y; g.lda = C; g.K1 = C; g.K = C; g.M = B * T; g.N = C;
            g.W = WT(h, p + ".post_linear.weight"); g.C = w->x; g.ldc = C;
            attach_premod(h, w, g, h->up[i].empty() ? nullptr : &h->up[i][0]);
            g.row_list = fine.list; g.row_cnt = fine.cnt; h->prof_next_list = fine.id;
            P_GEMM_LP(g);
            premod = g.mod_aff != nullptr;
            snprintf(name, sizeof(name), "up%d.upsample", i);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
        for (size_t j = 0; j < h->up[i].size(); j++) {
            const BlockPlan *next = j + 1 < h->up[i].size() ? &h->up[i][j + 1] : nullptr;   // then PatchBreakup / the read-out
            const BlockNeed bn{need_ref(h, w, pp.rows[i][j]), need_ref(h, w, pp.wins[i][j])};
            premod = run_block(h, w, h->up[i][j], premod, next, false, s, bn).premod;
            snprintf(name, sizeof(name), "up%d.block%d", i, (int)j);
            tap(h, name, w->x, (size_t)B * T * C, s);
        }
    }
    readout_stage(h, w, s);
}

// DSG_ERR_INVALID (and the message) if a launcher declined its arguments since the last check
int plan_status(dsg_handle h, Workspace *w) {
    if (h->plan_err.empty()) return 0;
    const std::string m = h->plan_err;
    h->plan_err.clear();
    return fail(h, DSG_ERR_INVALID, "unsupported configuration at batch %d: %s", w->B, m.c_str());
}

// Plan-time shape coverage: walk the whole forward of this workspace's batch size in a dry run -- every launcher checks its arguments
// and picks its instantiation, nothing is enqueued (kernels.h: g_dry_run) -- in both noise-label forms (per-sample rows: dsg_denoise /
// dsg_precond; the sampler's batch-uniform row) and with / without a self-conditioning input.  Runs when a batch size is first used and
// again after anything that changes the kernel selection (dsg_set_option, dsg_finalize_weights, debug taps): an uncovered shape is
// reported as DSG_ERR_INVALID by the entry point before any work is enqueued or captured -- never by terminating the process.
int validate_plan(dsg_handle h, Workspace *w) {
    if (w->plan_gen == h->plan_gen) return 0;
    const bool uni = w->uniform, prof_on = h->prof_on, prof_stamps = h->prof_stamps;
    const float *sca = w->cur_sc_adj, *scn = w->cur_sc_node; const int *hs = w->cur_has_sc;
    h->prof_on = false; h->prof_stamps = false;
    h->plan_err.clear();
    g_dry_run = true;
    for (int v = 0; v < 4; v++) {
        w->uniform = (v & 1) != 0;
        w->cur_sc_adj = (v & 2) ? w->sc_adj : nullptr; w->cur_sc_node = (v & 2) ? w->sc_node : nullptr; w->cur_has_sc = (v & 1) ? nullptr : w->has_sc;
        forward_fixed(h, w, nullptr);
    }
    g_dry_run = false;
    w->uniform = uni; h->prof_on = prof_on; h->prof_stamps = prof_stamps;
    w->cur_sc_adj = sca; w->cur_sc_node = scn; w->cur_has_sc = hs;
    if (int rc = plan_status(h, w)) return rc;
    w->plan_gen = h->plan_gen;
    return 0;
}

// run forward_fixed either eagerly or by replaying a captured graph
int run_forward(dsg_handle h, Workspace *w, bool use_graph, hipStream_t s) {
    // (plan_err: validate_plan has already walked this forward in a dry run, so these checks are the second line of defence)
    if (!use_graph || !h->taps.empty()) { forward_fixed(h, w, s); return plan_status(h, w); }
    hipGraphExec_t &exec = w->uniform ? w->graph_uniform : w->graph;
    if (!exec) {
        if (!w->cap_stream) HIP_TRY(h, hipStreamCreateWithFlags(&w->cap_stream, hipStreamNonBlocking));
        hipGraph_t graph;
        HIP_TRY(h, hipStreamBeginCapture(w->cap_stream, hipStreamCaptureModeThreadLocal));
        forward_fixed(h, w, w->cap_stream);
        HIP_TRY(h, hipStreamEndCapture(w->cap_stream, &graph));
        if (int rc = plan_status(h, w)) { (void)hipGraphDestroy(graph); return rc; }
        hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { exec = nullptr; return fail(h, DSG_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
    }
    HIP_TRY(h, hipGraphLaunch(exec, s));
    h->last_stats.graph_replays++;
    return 0;
}

Dims dims_of(dsg_handle h, int B) { return Dims{B, h->N, h->Ca, h->Cn}; }

int check_ready(dsg_handle h, int B) {
    if (!h) return DSG_ERR_INVALID;
    if (!h->finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (B < 1) return fail(h, DSG_ERR_INVALID, "batch must be >= 1");
    return 0;
}

// node flags into the workspace + the need lists of the masked-token pruning that follow from them (two small launches).  Flags are
// staged once per entry-point call -- never inside a captured step body; the captured graphs read lists and counts from fixed addresses
// zero_padded: the caller vouches that every adjacency / self-conditioning value the forwards of this call read at a pair with a padded
// endpoint is zero (the sampler: its state only ever comes from its own masking kernels) -- the pure-window deduplication's condition
// uniform_row: ... and that every one of those forwards reads the batch-uniform (scale, shift) row: one representative may then serve
// the whole batch (dedup_stage_mode)
// table: ... and that it has built the table of pure-window rows for every schedule index those forwards run at (build_pure_table)
// flags == nullptr: the lists of the flags the workspace holds
int stage_flags(dsg_handle h, Workspace *w, const uint8_t *flags, hipStream_t s, bool zero_padded = false, bool uniform_row = false,
                bool table = false) {
    if (flags) HIP_TRY(h, hipMemcpyAsync(w->flags, flags, (size_t)w->B * h->N, hipMemcpyDeviceToDevice, s));
    w->dd_mode = dedup_stage_mode(h, w, zero_padded, uniform_row, &w->dd_trim, &w->dd_depth, table);
    if (w->need_lists)
        launch_need_lists(w->flags, w->B, h->N, w->need, w->need_cnt_ps, w->need_lists, w->need_cnt, s, w->dd_mode, w->dd_rep, w->dd_trim);
    return 0;
}

// the caller's graph seeds (host, [B]) into the workspace-owned device buffer, allocated by the first seeded call at this batch size.
// Enqueued on the caller's stream; the callers synchronise before they return, so the host array is read while it is still theirs
int stage_seeds(dsg_handle h, Workspace *w, const uint64_t *graph_seeds, hipStream_t s) {
    if (!w->gseeds) {
        void *q;
        if (int rc = owned_alloc(h, w->allocs, &q, sizeof(unsigned long long) * (size_t)w->B, AC_STATE)) return rc;
        w->gseeds = (unsigned long long *)q;
        w->seeds_bytes = sizeof(unsigned long long) * (size_t)w->B;
        w->bytes += w->seeds_bytes;
    }
    HIP_TRY(h, hipMemcpyAsync(w->gseeds, graph_seeds, sizeof(unsigned long long) * (size_t)w->B, hipMemcpyHostToDevice, s));
    return 0;
}

// stage caller tensors into the fixed forward inputs
int stage_inputs(dsg_handle h, Workspace *w, const float *adj, const float *node, const uint8_t *flags, const float *sc_adj,
                 const float *sc_node, hipStream_t s) {
    const size_t sa = sizeof(float) * (size_t)w->B * h->Ca * h->N * h->N, sn = sizeof(float) * (size_t)w->B * h->N * h->Cn;
    if (adj) HIP_TRY(h, hipMemcpyAsync(w->in_adj, adj, sa, hipMemcpyDeviceToDevice, s));
    if (node) HIP_TRY(h, hipMemcpyAsync(w->in_node, node, sn, hipMemcpyDeviceToDevice, s));
    if (flags) if (int rc = stage_flags(h, w, flags, s)) return rc;
    const int has = (sc_adj && sc_node && h->cfg.self_condition) ? 1 : 0;
    if (has) {
        if (sc_adj != w->sc_adj) HIP_TRY(h, hipMemcpyAsync(w->sc_adj, sc_adj, sa, hipMemcpyDeviceToDevice, s));
        if (sc_node != w->sc_node) HIP_TRY(h, hipMemcpyAsync(w->sc_node, sc_node, sn, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(h, hipMemsetAsync(w->has_sc, 0, 16, s));
    if (has) HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)w->has_sc, 1, 1, s));
    w->cur_sc_adj = w->sc_adj; w->cur_sc_node = w->sc_node; w->cur_has_sc = w->has_sc;
    return 0;
}

// NodeAdjPrecond.forward on workspace state: x (xh_adj/xh_node), sigmas (w->sig) -> D (dst), optionally
// mirrored into the fixed self-cond input of the next forward.  sc: current self-cond or null.
// dst.adj == nullptr: stop behind the last forward, F is left in w->f_* (the two legs of an autoguided dsg_precond)
int precond_core(dsg_handle h, Workspace *w, CStatePtrs x, const float *sc_adj, const float *sc_node, bool coin, StatePtrs dst,
                 bool use_graph, hipStream_t s, int64_t *nfe, const float *aff_row = nullptr) {
    const Dims d = dims_of(h, w->B);
    w->uniform = aff_row != nullptr;
    if (aff_row) HIP_TRY(h, hipMemcpyAsync(w->aff, aff_row, sizeof(float) * h->aff_n, hipMemcpyDeviceToDevice, s));
    launch_precond_in(x, w->sig, StatePtrs{w->in_adj, w->in_node}, w->c_noise, d, s);
    if (int rc = stage_inputs(h, w, nullptr, nullptr, nullptr, sc_adj, sc_node, s)) return rc;
    if (h->cfg.self_condition && coin) {  // precond.py:90-98
        if (int rc = run_forward(h, w, use_graph, s)) return rc;
        (*nfe)++;
        // the D of the extra pass becomes the self-cond input (written straight into the fixed sc buffers)
        launch_precond_out(x, CStatePtrs{w->f_adj, w->f_node}, w->sig, w->flags, StatePtrs{w->sc_adj, w->sc_node}, d, s);
        HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)w->has_sc, 1, 1, s));
    }
    if (int rc = run_forward(h, w, use_graph, s)) return rc;
    (*nfe)++;
    if (dst.adj) launch_precond_out(x, CStatePtrs{w->f_adj, w->f_node}, w->sig, w->flags, dst, d, s);
    return 0;
}

// a call of the main handle that its guide refused: the guide's own message, prefixed so that the caller sees which handle it was
int guide_fail(dsg_handle h, dsg_handle g, int rc) { return fail(h, rc, "guide handle: %s", g->err.c_str()); }

// ---- one step of the reverse loop (edm.py:350-427) as a static launch sequence ------------------------------------------
// Everything that changes from step to step is read on the device from StepRow[ctl->step] / the step's (scale,shift) row, so
// the sequence below depends only on the StepPlan and can be captured once per plan and replayed for every step it fits.
struct StepPlan {
    int sc_slot;          // d_* buffer holding the self-conditioning input of stage 1, -1 = None
    int s1, s2;           // d_* buffers receiving the stage-1 / stage-2 denoised outputs
    bool euler;           // Euler update (solver 'euler', or the last step: edm.py:394-396), else Heun
    bool coin1, coin2;    // outcome of the self-conditioning coin of each preconditioned call (precond.py:90)
    bool known = false;   // conditional sampling: every D goes through the known-entry select (w->kn_* / w->km_*)
    int prev = -1;        // second-order multistep step (DSG_SOLVER_DPMPP_2M, row coefficient != 0): d_* buffer holding the previous
                          // step's D, never s1 nor a buffer the step writes; -1 = none, the plain Euler / Heun step
    bool guided = false;  // box guidance (dsg_sample_guided): the guide kernel behind every D, the updates read D~ = D - shift
    bool clip = false;    //   with the norm pass and the clip factor in front of it
    int g1 = 0, g2 = 0;   //   w->g_shift buffers of the stage-1 / stage-2 shift
    int gprev = -1;       //   ... and of the previous step's stage-1 shift where prev >= 0
    int rel = REL_NONE;   //   the relation term (dsg_sample_guided_rel): REL_GIVEN / REL_DECODED select the guide kernel's relation variant
    bool content = false; //   content guidance (dsg_sample_guided_content): the content kernel behind every D too, the updates read both
                          //   shifts; its shift buffers rotate with g1 / g2 / gprev
    bool cclip = false;   //   ... with the content shift's own clip factor
    int cgrid = 0;        //   ... 0: the content kernel's one-block-per-graph form; K: its (graph, item) grid, whose launch bakes K
    bool autoguide = false;   // autoguidance (dsg_attach_guide): every preconditioned call of the step runs the guide's forwards behind
                              // the main network's and stores the composite D~; clear on a step outside the interval, whose body is the plain one
    int key() const {   // prev, then the guidance bits, the relation bits, the content bits, the autoguide bit sit above every older bit: plans without them keep their keys
        return (sc_slot + 1) | (s1 << 2) | (s2 << 4) | ((int)euler << 6) | ((int)coin1 << 7) | ((int)coin2 << 8) | ((int)known << 9) |
               ((prev + 1) << 10) | ((int)guided << 12) | ((int)clip << 13) | (g1 << 14) | (g2 << 16) | ((gprev + 1) << 18) | (rel << 20) |
               ((int)content << 22) | ((int)cclip << 23) | (cgrid << 24) | (autoguide ? STEP_KEY_AUTOGUIDE : 0);
    }
};

// D = mask(c_skip x + c_out F) at sigma[step]; known: with the select of the conditioned loop in front of the store
void precond_out_step(dsg_handle h, Workspace *w, CStatePtrs x, StatePtrs dst, bool known, const Dims &d, hipStream_t s) {
    const CStatePtrs F{w->f_adj, w->f_node};
    if (known) launch_precond_out_tab_known(x, F, h->tab_step, w->ctl, w->flags, CStatePtrs{w->kn_adj, w->kn_node}, CMaskPtrs{w->km_adj, w->km_node}, dst, d, s);
    else launch_precond_out_tab(x, F, h->tab_step, w->ctl, w->flags, dst, d, s);
}

// NodeAdjPrecond.forward at sigma[step] on workspace state x -> dst; forwards run inline on `s` (capturable)
// fwd_graph: replay the captured network forward (round-1 scheme: only the forward is a graph, the loop is host-enqueued)
// known: conditional sampling -- both D writes (the extra self-conditioning pass's too) take the known entries from the workspace
// wg (autoguidance, a guided step): the guide handle's workspace.  Behind the main network's last forward, on the same stream, the
// guide runs NodeAdjPrecond at the same x, sigma, sc and coin outcome -- its forwards read the main workspace's c_in x, its extra
// pass goes through the existing kernel into its own sc_* -- and one kernel forms D_m and D_g from the two F and stores D~.  The
// guide's forwards are always enqueued as kernels, also where the main network's replay its forward-only graph
int precond_tab(dsg_handle h, Workspace *w, CStatePtrs x, const float *sc_adj, const float *sc_node, bool coin, StatePtrs dst,
                hipStream_t s, int *nfe, bool fwd_graph, bool known, Workspace *wg = nullptr, int *gfe = nullptr) {
    const Dims d = dims_of(h, w->B);
    w->uniform = true;
    launch_precond_in_tab(x, h->tab_step, w->ctl, StatePtrs{w->in_adj, w->in_node}, d, s);
    const bool has = sc_adj && sc_node && h->cfg.self_condition;
    if (fwd_graph) {   // the forward-only graph reads the fixed self-cond buffers and the device flag
        if (int rc = stage_inputs(h, w, nullptr, nullptr, nullptr, sc_adj, sc_node, s)) return rc;
    } else {           // kernels only: the forward reads the denoised buffer in place (or nothing)
        w->cur_sc_adj = has ? sc_adj : nullptr; w->cur_sc_node = has ? sc_node : nullptr; w->cur_has_sc = nullptr;
    }
    if (h->cfg.self_condition && coin) {  // precond.py:90-98: the D of the extra pass becomes the self-cond input
        if (int rc = run_forward(h, w, fwd_graph, s)) return rc;
        (*nfe)++;
        precond_out_step(h, w, x, StatePtrs{w->sc_adj, w->sc_node}, known, d, s);
        if (fwd_graph) HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)w->has_sc, 1, 1, s));
        else { w->cur_sc_adj = w->sc_adj; w->cur_sc_node = w->sc_node; }
    }
    if (int rc = run_forward(h, w, fwd_graph, s)) return rc;
    (*nfe)++;
    if (!wg) { precond_out_step(h, w, x, dst, known, d, s); return 0; }
    dsg_handle g = h->guide;
    // on every exit the guide's workspace holds no address of the main handle, and its host-side word on the kind of its next forward
    // is what it was (build_pure_table's FormGuard: an eager forward of the guide on its own may follow)
    struct ExtGuard { Workspace *w; bool uniform; const float *sca, *scn; const int *hs;
                      ~ExtGuard() { w->ext_in_adj = w->ext_in_node = nullptr; w->ext_step = nullptr; w->ext_ctl = nullptr;
                                    w->uniform = uniform; w->cur_sc_adj = sca; w->cur_sc_node = scn; w->cur_has_sc = hs; } }
        ext_guard{wg, wg->uniform, wg->cur_sc_adj, wg->cur_sc_node, wg->cur_has_sc};
    wg->ext_in_adj = w->in_adj; wg->ext_in_node = w->in_node; wg->ext_step = h->tab_step; wg->ext_ctl = w->ctl;
    wg->uniform = true;
    wg->cur_sc_adj = has ? sc_adj : nullptr; wg->cur_sc_node = has ? sc_node : nullptr; wg->cur_has_sc = nullptr;
    const CStatePtrs Fg{wg->f_adj, wg->f_node}, kn{w->kn_adj, w->kn_node};
    const CMaskPtrs km{w->km_adj, w->km_node};
    if (g->cfg.self_condition && coin) {   // the guide's own extra pass, from its own F
        if (int rc = run_forward(g, wg, false, s)) return guide_fail(h, g, rc);
        (*gfe)++;
        if (known) launch_precond_out_tab_known(x, Fg, h->tab_step, w->ctl, w->flags, kn, km, StatePtrs{wg->sc_adj, wg->sc_node}, d, s);
        else launch_precond_out_tab(x, Fg, h->tab_step, w->ctl, w->flags, StatePtrs{wg->sc_adj, wg->sc_node}, d, s);
        wg->cur_sc_adj = wg->sc_adj; wg->cur_sc_node = wg->sc_node;
    }
    if (int rc = run_forward(g, wg, false, s)) return guide_fail(h, g, rc);
    (*gfe)++;
    const CStatePtrs Fm{w->f_adj, w->f_node};
    if (known) launch_precond_out_mix_tab_known(x, Fm, Fg, h->guide_sm1, h->tab_step, w->ctl, w->flags, kn, km, dst, d, s);
    else launch_precond_out_mix_tab(x, Fm, Fg, h->guide_sm1, h->tab_step, w->ctl, w->flags, dst, d, s);
    return 0;
}

// box guidance behind one preconditioned call: the norm pass (with the clip only), then the guide kernel on D -> w->g_shift[slot]
int guide_call(dsg_handle h, Workspace *w, const StepPlan &p, CStatePtrs xh, CStatePtrs D, int slot, bool stage1, const Dims &d, hipStream_t s) {
    if ((p.clip || p.cclip) && !launch_graph_diff_norm(xh, D, w->flags, w->g_ref, d, s)) return fail(h, DSG_ERR_INVALID, "box guidance: shape refused");
    const BoxGuideOut out{w->g_shift[slot], nullptr, nullptr, nullptr, nullptr};
    const bool ok = p.rel != REL_NONE
        ? launch_box_guide_rel(w->g_par, h->tab_step, w->ctl, 0.f, D.adj, D.node, w->flags, p.clip ? w->g_ref : nullptr, stage1, out, nullptr,
                               p.rel == REL_DECODED, d, s)
        : launch_box_guide(w->g_par, h->tab_step, w->ctl, 0.f, D.node, w->flags, p.clip ? w->g_ref : nullptr, stage1, out, d, s);
    if (!ok) return fail(h, DSG_ERR_INVALID, "box guidance: shape refused");
    if (p.content) {   // the content term: a kernel and a full-state shift of its own, clipped on its own against the same norm
        const ContentOut co{w->c_shift_adj[slot], w->c_shift_label[slot], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (!launch_content_guide(w->c_par, h->tab_step, w->ctl, 0.f, D.adj, D.node, w->flags, p.cclip ? w->g_ref : nullptr, stage1, co, p.cgrid,
                                  w->c_stats, d, s))
            return fail(h, DSG_ERR_INVALID, "content guidance: shape refused");
    }
    return 0;
}

int enqueue_step(dsg_handle h, Workspace *w, const StepPlan &p, const float *gt_adj, const float *gt_node, hipStream_t s, int *nfe,
                 int *gfe, bool fwd_graph = false) {
    const Dims d = dims_of(h, w->B);
    Workspace *wg = nullptr;   // a guided step of an autoguided run: the guide's workspace (sample_impl created and staged it)
    if (p.autoguide && !gt_adj) {
        if (h->guide) { auto it = h->guide->ws.find(w->B); if (it != h->guide->ws.end()) wg = it->second.get(); }
        if (!wg) return fail(h, DSG_ERR_STATE, "autoguided step without a staged guide workspace");
    }
    const CStatePtrs xh{w->xh_adj, w->xh_node};
    auto cshift = [&](int slot) { return ContentShiftPtrs{w->c_shift_adj[slot], w->c_shift_label[slot]}; };
    launch_churn_tab(CStatePtrs{w->x_adj, w->x_node}, h->tab_step, w->ctl, w->flags, StatePtrs{w->xh_adj, w->xh_node}, d, s);   // edm.py:355-366
    CStatePtrs D1{gt_adj, gt_node};   // sanity-check mode (edm.py:372-377): the denoiser is bypassed
    if (!gt_adj) {
        launch_step_row(h->tab_aff, h->aff_n, h->tab_step, w->ctl, w->aff, s);   // this step's (scale,shift) row for every block
        if (wg) launch_step_row(h->guide->tab_aff, h->guide->aff_n, h->tab_step, w->ctl, wg->aff, s);   // ... and for every block of the guide, from its own table
        if (int rc = precond_tab(h, w, xh, p.sc_slot >= 0 ? w->d_adj[p.sc_slot] : nullptr, p.sc_slot >= 0 ? w->d_node[p.sc_slot] : nullptr,
                                 p.coin1, StatePtrs{w->d_adj[p.s1], w->d_node[p.s1]}, s, nfe, fwd_graph, p.known, wg, gfe)) return rc;
        D1 = CStatePtrs{w->d_adj[p.s1], w->d_node[p.s1]};
    }
    if (p.guided) if (int rc = guide_call(h, w, p, xh, D1, p.g1, /*stage1=*/true, d, s)) return rc;
    const StatePtrs x{w->x_adj, w->x_node};
    if (p.euler && p.prev >= 0) {   // sanity-check mode: D_prev = D = gt
        const CStatePtrs Dp = gt_adj ? D1 : CStatePtrs{w->d_adj[p.prev], w->d_node[p.prev]};
        if (p.content) launch_multistep_tab_guided2(xh, D1, Dp, w->g_shift[p.g1], w->g_shift[p.gprev], cshift(p.g1), cshift(p.gprev), w->c_par, h->tab_step, w->ctl, w->flags, x, d, s);
        else if (p.guided) launch_multistep_tab_guided(xh, D1, Dp, w->g_shift[p.g1], w->g_shift[p.gprev], h->tab_step, w->ctl, w->flags, x, d, s);
        else launch_multistep_tab(xh, D1, Dp, h->tab_step, w->ctl, w->flags, StatePtrs{w->x_adj, w->x_node}, d, s);
    } else if (p.euler) {
        if (p.content) launch_euler_tab_guided2(xh, D1, w->g_shift[p.g1], cshift(p.g1), w->c_par, h->tab_step, w->ctl, w->flags, x, d, s);
        else if (p.guided) launch_euler_tab_guided(xh, D1, w->g_shift[p.g1], h->tab_step, w->ctl, w->flags, x, d, s);
        else launch_euler_tab(xh, D1, h->tab_step, w->ctl, w->flags, StatePtrs{w->x_adj, w->x_node}, d, s);
    } else {
        CStatePtrs D2 = D1;
        if (!gt_adj) {   // stage 2 re-evaluates at (x_hat, sigma(t_hat)) with self-cond = D1 (edm.py:400-405)
            const bool sc = h->cfg.self_condition;
            if (int rc = precond_tab(h, w, xh, sc ? w->d_adj[p.s1] : nullptr, sc ? w->d_node[p.s1] : nullptr, p.coin2,
                                     StatePtrs{w->d_adj[p.s2], w->d_node[p.s2]}, s, nfe, fwd_graph, p.known, wg, gfe)) return rc;
            D2 = CStatePtrs{w->d_adj[p.s2], w->d_node[p.s2]};
        }
        if (p.guided) {   // stage 2 is evaluated at (x_hat, t_hat) and guided the same way
            if (int rc = guide_call(h, w, p, xh, D2, p.g2, /*stage1=*/false, d, s)) return rc;
            if (p.content) launch_heun_tab_guided2(xh, D1, D2, w->g_shift[p.g1], w->g_shift[p.g2], cshift(p.g1), cshift(p.g2), w->c_par, h->tab_step, w->ctl, w->flags, x, d, s);
            else launch_heun_tab_guided(xh, D1, D2, w->g_shift[p.g1], w->g_shift[p.g2], h->tab_step, w->ctl, w->flags, x, d, s);
        } else launch_heun_tab(xh, D1, D2, h->tab_step, w->ctl, w->flags, StatePtrs{w->x_adj, w->x_node}, d, s);
    }
    launch_step_advance(w->ctl, s);
    return 0;
}

// capture + instantiate the step body of plan p (no-op if it exists).  Called for every plan of a run BEFORE the run's first
// launch: instantiating a new graph while earlier graph launches are still in flight on the caller's stream gave wrong
// trajectories on ROCm 7.2 (tools/loop_graph_ab.py history in DESIGN.md), so nothing is captured mid-flight.
int ensure_step_graph(dsg_handle h, Workspace *w, const StepPlan &p) {
    if (w->step_graphs.count(p.key())) return 0;
    if (!w->cap_stream) HIP_TRY(h, hipStreamCreateWithFlags(&w->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph;
    int n = 0, ng = 0;
    HIP_TRY(h, hipStreamBeginCapture(w->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_step(h, w, p, nullptr, nullptr, w->cap_stream, &n, &ng);
    const hipError_t ec = hipStreamEndCapture(w->cap_stream, &graph);
    if (rc) { if (ec == hipSuccess) (void)hipGraphDestroy(graph); return rc; }
    if (ec != hipSuccess) return fail(h, DSG_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ec));
    hipGraphExec_t exec = nullptr;
    const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, DSG_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    w->step_graphs.emplace(p.key(), Workspace::StepBody{exec, n, ng});
    if (getenv("DSG_GRAPH_VERBOSE")) fprintf(stderr, "[dsg-graph] captured step body key=%d (sc %d s1 %d s2 %d euler %d coins %d%d known %d prev %d): %d forwards\n",
                                             p.key(), p.sc_slot, p.s1, p.s2, (int)p.euler, (int)p.coin1, (int)p.coin2, (int)p.known, p.prev, n);
    return 0;
}

// replay the step body of plan p on the caller's stream
int replay_step(dsg_handle h, Workspace *w, const StepPlan &p, hipStream_t s, int *nfe, int *gfe) {
    auto it = w->step_graphs.find(p.key());
    if (it == w->step_graphs.end()) return fail(h, DSG_ERR_STATE, "step body %d was not captured", p.key());
    HIP_TRY(h, hipGraphLaunch(it->second.exec, s));
    *nfe += it->second.forwards;
    *gfe += it->second.guide_forwards;
    h->last_stats.graph_replays += it->second.forwards;
    return 0;
}

// dsg_sampler_cfg.heun names the solver: 0 Euler, 2 DPM-Solver++ 2M, every other value Heun (it was a truth value once)
bool solver_heun(const dsg_sampler_cfg *c) { return c->heun != DSG_SOLVER_EULER && c->heun != DSG_SOLVER_DPMPP_2M; }
bool solver_2m(const dsg_sampler_cfg *c) { return c->heun == DSG_SOLVER_DPMPP_2M; }

}  // namespace

extern "C" {

size_t dsg_workspace_bytes(dsg_handle h, int32_t B) {
    if (!h || !h->finalized || B < 1) return 0;
    size_t need = 0;   // the need lists of the masked-token pruning: every list + 16 pad entries, counts, per-sample counts
    const PrunePlan &pp = prune_plan(h);
    for (int k = 0; k < pp.np.n_lists; k++) need += sizeof(int) * ((size_t)B * pp.items[k] + 16 + 1 + (size_t)B);
    need += sizeof(int) * ((size_t)B * pp.np.dd_n + (pp.np.dd_n > 0 ? 1 : 0));   // the representative windows of the pure-window deduplication, the lists' mode
    auto it = h->ws.find(B);   // + the known tensors and masks of dsg_sample_known, once a conditioned call has allocated them
    const size_t known = it != h->ws.end() ? it->second->known_bytes : 0;
    const size_t seeds = it != h->ws.end() ? it->second->seeds_bytes : 0;   // + the graph seeds, once a seeded call has allocated them
    const size_t pure = it != h->ws.end() ? it->second->tab_pure_bytes : 0;   // + the table of pure-window rows, once a sampler call has built one
    const size_t guide = it != h->ws.end() ? it->second->guide_bytes : 0;     // + the buffers and tables of box guidance, once a guided call has allocated them
    return sizeof(float) * per_sample_floats(h) * (size_t)B + (size_t)B * h->N + 16 + need + known + seeds + pure + guide;
}

int dsg_set_option(dsg_handle h, const char *name, int32_t value) {
    if (!h || !name) return DSG_ERR_INVALID;
    const OptRow *r = find_option(name);
    if (!r) return fail(h, DSG_ERR_INVALID, "unknown option '%s'", name);
    if ((r->flags & OPT_STRICT) && (value < r->lo || value > r->hi))
        return fail(h, DSG_ERR_INVALID, "debug_alloc_fill is 0 (off) or a pattern 1..4, not %d", value);   // (the one strict row)
    const Options saved = h->opt;   // restored if the new selection cannot run (below)
    h->opt.*r->field = r->normalised(value);
    // patch_size > 1: switching one of the modes it does not build ON is refused here, ahead of the weight copies and whether or not a batch
    // size is in use yet.  Any other change passes -- a mode stored from an environment default is refused by the plan check of the first
    // forward (forward_fixed), and setting it to 0 is how a caller clears it
    const bool patch_mode_on = (r->field == &Options::gemm_split || r->field == &Options::gemm_bf16 || r->field == &Options::batch_invariant) &&
                               (h->opt.*r->field) != 0;
    if (const char *o = patch_mode_on ? patch_refused_option(h) : nullptr) {
        h->opt = saved;
        return fail(h, DSG_ERR_INVALID, "option '%s' = %d rejected: \"%s\" is not built at patch_size %d (patch_size > 1 runs the fp32 kernels only)", name, value, o, h->P);
    }
    if (h->finalized) {   // the precision modes run on copies of the weights
        int rc = 0;
        if (r->field == &Options::gemm_bf16 && h->opt.gemm_bf16) rc = ensure_bf16_weights(h);
        if (r->field == &Options::gemm_split && h->opt.gemm_split) rc = ensure_split_weights(h);
        if (rc) { h->opt = saved; return rc; }
    }
    if (r->flags & OPT_KEEPS_GRAPHS) return DSG_OK;
    drop_graphs(h);   // captured graphs bake the kernel selection
    // plan time: every batch size in use must still be covered by the kernels the new selection launches; if not, the option keeps
    // its old value and the caller gets DSG_ERR_INVALID with the layer / shape in dsg_last_error
    // (a patch_size > 1 handle still holding a refused mode from its environment default has no valid plan whatever this call set: the
    // next forward says so; this call is not blamed for it)
    if (h->finalized && !patch_refused_option(h))
        for (auto &kv : h->ws)
            if (int rc = validate_plan(h, kv.second.get())) {
                const std::string why = h->err;
                h->opt = saved;
                drop_graphs(h);
                return fail(h, rc, "option '%s' = %d rejected: %s", name, value, why.c_str());
            }
    return DSG_OK;
}

int dsg_get_option(dsg_handle h, const char *name, int32_t *value) {
    if (!h || !name || !value) return DSG_ERR_INVALID;
    const OptRow *r = find_option(name);
    if (!r) return fail(h, DSG_ERR_INVALID, "unknown option '%s'", name);
    *value = r->effective ? r->effective(h) : h->opt.*r->field;
    return DSG_OK;
}

// host only, no handle: row `index` of the option table (any out pointer may be NULL); DSG_ERR_INVALID past the end
int dsg_option_info(int32_t index, const char **name, const char **env, int32_t *dflt, int32_t *lo, int32_t *hi) {
    if (index < 0 || index >= N_OPTIONS) return DSG_ERR_INVALID;
    const OptRow &r = g_options[index];
    if (name) *name = r.name;
    if (env) *env = r.env;
    if (dflt) *dflt = r.dflt;
    if (lo) *lo = r.lo;
    if (hi) *hi = r.hi;
    return DSG_OK;
}

// test hook (include/dsg.h): every existing AC_SCRATCH / AC_FINITE buffer of the handle and of batch size B's workspace becomes
// `pattern`; AC_STATE and AC_CONST buffers are never touched.  NaN is not written into the AC_FINITE buffers: their contract is "finite"
int dsg_debug_poison(dsg_handle h, int32_t B, int32_t pattern, uint64_t seed, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (pattern < 1 || pattern > 4) return fail(h, DSG_ERR_INVALID, "pattern is 1 (zeros), 2 (NaN), 3 (1e30) or 4 (random), not %d", pattern);
    hipStream_t s = (hipStream_t)stream;
    Workspace *w;
    if (int rc = get_workspace(h, B, &w)) return rc;
    unsigned long long k = 0;
    for (const std::vector<AllocRec> *pool : {&h->allocs, &w->allocs})
        for (const AllocRec &r : *pool) {
            k++;
            if (r.cls != AC_SCRATCH && r.cls != AC_FINITE) continue;
            if (r.cls == AC_FINITE && pattern == 2) continue;
            launch_debug_fill(r.p, r.bytes / 4, pattern, seed * 0x100000001b3ull + k, s);
        }
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_gen_noise(dsg_handle h, int32_t B, const uint8_t *flags, uint64_t seed, uint32_t noise_stream, float *out_adj,
                  float *out_node, void *stream) {
    if (!h || B < 1) return fail(h, DSG_ERR_INVALID, "batch must be >= 1");
    if (!flags || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    launch_init(CStatePtrs{nullptr, nullptr}, CStatePtrs{nullptr, nullptr}, 1.0f, seed, nullptr, noise_stream, flags, StatePtrs{out_adj, out_node},
                dims_of(h, B), (hipStream_t)stream);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_gen_noise_seeded(dsg_handle h, int32_t B, const uint8_t *flags, const uint64_t *graph_seeds, uint32_t noise_stream, float *out_adj,
                         float *out_node, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!flags || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    if (!graph_seeds) return fail(h, DSG_ERR_INVALID, "dsg_gen_noise_seeded needs graph_seeds (host, one per graph); graph_seeds is NULL");
    hipStream_t s = (hipStream_t)stream;
    Workspace *w;
    if (int rc = get_workspace(h, B, &w)) return rc;
    if (int rc = stage_seeds(h, w, graph_seeds, s)) return rc;
    launch_init(CStatePtrs{nullptr, nullptr}, CStatePtrs{nullptr, nullptr}, 1.0f, 0, w->gseeds, noise_stream, flags, StatePtrs{out_adj, out_node},
                dims_of(h, B), s);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));   // the seeds are the caller's host memory
    return DSG_OK;
}

int dsg_debug_tap(dsg_handle h, const char *stage, float *dst, int64_t capacity) {
    if (!h || !stage || !dst) return DSG_ERR_INVALID;
    h->taps.push_back({stage, dst, capacity});
    h->plan_gen++;   // taps switch the row-kernel fusions off: the launch plan changes
    return DSG_OK;
}
void dsg_debug_clear_taps(dsg_handle h) { if (h) { h->taps.clear(); h->plan_gen++; } }

int dsg_denoise(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, const float *noise_labels,
                const float *sc_adj, const float *sc_node, float *out_adj, float *out_node, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!adj || !node || !flags || !noise_labels || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    Workspace *w;
    if (int rc = get_workspace(h, B, &w)) return rc;
    if (int rc = stage_inputs(h, w, adj, node, flags, sc_adj, sc_node, s)) return rc;
    w->uniform = false;
    HIP_TRY(h, hipMemcpyAsync(w->c_noise, noise_labels, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    if (int rc = run_forward(h, w, false, s)) return rc;
    const size_t sa = sizeof(float) * (size_t)B * h->Ca * h->N * h->N, sn = sizeof(float) * (size_t)B * h->N * h->Cn;
    HIP_TRY(h, hipMemcpyAsync(out_adj, w->f_adj, sa, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(out_node, w->f_node, sn, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_precond(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, const float *sigmas,
                const float *sc_adj, const float *sc_node, int32_t coin, float *out_adj, float *out_node, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!adj || !node || !flags || !sigmas || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    Workspace *w;
    if (int rc = get_workspace(h, B, &w)) return rc;
    dsg_handle g = h->guide;
    Workspace *wg = nullptr;
    if (g) {   // (refused by the guide before anything is enqueued)
        if (int rc = check_ready(g, B)) return guide_fail(h, g, rc);
        if (int rc = get_workspace(g, B, &wg)) return guide_fail(h, g, rc);
    }
    if (int rc = stage_flags(h, w, flags, s)) return rc;
    HIP_TRY(h, hipMemcpyAsync(w->sig, sigmas, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    int64_t nfe = 0;
    const CStatePtrs x{adj, node};
    if (int rc = precond_core(h, w, x, sc_adj, sc_node, coin != 0, g ? StatePtrs{nullptr, nullptr} : StatePtrs{out_adj, out_node}, false, s, &nfe))
        return rc;
    if (g) {
        // the guide's leg at the same x, sigmas, sc and coin outcome, behind the main network's on the same stream; sigmas are per
        // sample here, so the guide always runs and the store selects s_b - 1 per sample
        if (int rc = stage_flags(g, wg, flags, s)) return guide_fail(h, g, rc);
        if (hipMemcpyAsync(wg->sig, sigmas, sizeof(float) * B, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, DSG_ERR_HIP, "guide handle: copy of sigmas failed");
        if (int rc = precond_core(g, wg, x, sc_adj, sc_node, coin != 0, StatePtrs{nullptr, nullptr}, false, s, &nfe)) return guide_fail(h, g, rc);
        launch_precond_out_mix(x, CStatePtrs{w->f_adj, w->f_node}, CStatePtrs{wg->f_adj, wg->f_node}, w->sig, h->guide_sm1, h->guide_lo, h->guide_hi,
                               w->flags, StatePtrs{out_adj, out_node}, dims_of(h, B), s);
    }
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

// Host-side schedule.  Mirrors the reference's fp32 scalar-tensor arithmetic op by op (edm.py:318-323,
// :355-369); this file is compiled with -ffp-contract=off so no product is fused into a subtraction.
int dsg_sigma_schedule(const dsg_sampler_cfg *c, double *sigma_steps, float *t_hat, float *noise_coef, float *h_step) {
    if (!c || c->num_steps < 1) return DSG_ERR_INVALID;
    const int T = c->num_steps;
    std::vector<float> t(T + 1);
    const double a = std::pow(c->sigma_max, 1.0 / c->rho), b = std::pow(c->sigma_min, 1.0 / c->rho);
    for (int i = 0; i < T; i++) {
        const double frac = T > 1 ? (double)i / (double)(T - 1) : 0.0;
        const double sg = std::pow(a + frac * (b - a), c->rho);
        if (sigma_steps) sigma_steps[i] = sg;
        t[i] = (float)sg;
    }
    t[T] = 0.f;
    // python: min(S_churn / num_steps, np.sqrt(2) - 1) in double, cast to fp32 when multiplied with t_cur
    const float gamma_on = (float)std::fmin((double)c->S_churn / (double)T, std::sqrt(2.0) - 1.0);
    for (int i = 0; i < T; i++) {
        const float tc = t[i];
        const float gamma = (c->S_min <= tc && tc <= c->S_max) ? gamma_on : 0.f;
        volatile float gt = gamma * tc;
        volatile float th = tc + gt;
        volatile float th2 = th * th, tc2 = tc * tc;
        volatile float diff = th2 - tc2;
        volatile float rt = std::sqrt(diff > 0.f ? diff : 0.f);
        volatile float nz = rt * c->S_noise;
        if (t_hat) t_hat[i] = th;
        if (noise_coef) noise_coef[i] = nz;
        if (h_step) h_step[i] = t[i + 1] - th;
    }
    return DSG_OK;
}

// Host-side walk over the schedule (include/dsg.h): which schedule index every executed step runs at, and its churn coefficient.
// A repeated pass of a block [b, e) begins with the state at t_e; the jump back to t_b (variance t_b^2 - t_e^2) and the step's own
// churn (variance nz_b^2) are independent Gaussians, i.e. one: a single coefficient, evaluated in double and rounded once.
int32_t dsg_walk_steps(const dsg_sampler_cfg *c, const dsg_walk_cfg *wk, int32_t *sched_idx, float *noise_coef, int32_t cap) {
    if (!c || !wk || c->num_steps < 1) return DSG_ERR_INVALID;
    const int T = c->num_steps;
    const int s = wk->start_step, j = wk->jump_len, r = wk->n_resample, lo = wk->resample_lo;
    const int hi = wk->resample_hi <= 0 ? T : wk->resample_hi;
    if (s < 0 || s >= T || j < 1 || r < 1 || lo < s || hi < lo || hi > T) return DSG_ERR_INVALID;
    const int64_t L = (int64_t)T - s + (int64_t)(r - 1) * (hi - lo);
    if (L > DSG_WALK_MAX_STEPS) return DSG_ERR_INVALID;
    if (!sched_idx && !noise_coef) return (int32_t)L;
    if (cap < L) return DSG_ERR_INVALID;
    std::vector<double> sg(T);
    std::vector<float> nz(T);
    dsg_sigma_schedule(c, sg.data(), nullptr, nz.data(), nullptr);
    int k = 0;
    auto emit = [&](int i, float coef) {
        if (sched_idx) sched_idx[k] = i;
        if (noise_coef) noise_coef[k] = coef;
        k++;
    };
    for (int i = s; i < lo; i++) emit(i, nz[i]);
    for (int b = lo; b < hi; b += j) {
        const int e = b + j < hi ? b + j : hi;
        const double tb = (double)(float)sg[b], te = e == T ? 0.0 : (double)(float)sg[e], nb = (double)nz[b];
        const float jump = (float)std::sqrt(tb * tb - te * te + nb * nb);
        for (int pass = 0; pass < r; pass++)
            for (int i = b; i < e; i++) emit(i, (pass > 0 && i == b) ? jump : nz[i]);
    }
    for (int i = hi; i < T; i++) emit(i, nz[i]);
    return (int32_t)L;
}

// Host-side coefficients of the second-order multistep update (include/dsg.h): c_k of every executed step of the walk, 0 where the
// step is the Euler step.  In double on the widened fp32 levels, rounded once.
int32_t dsg_multistep_coef(const dsg_sampler_cfg *c, const dsg_walk_cfg *wk, float *coef, int32_t cap) {
    const dsg_walk_cfg trivial{0, 1, 1, 0, 0, {0, 0, 0}};
    if (!wk) wk = &trivial;
    const int32_t L = dsg_walk_steps(c, wk, nullptr, nullptr, 0);
    if (L < 0) return L;
    const int T = c->num_steps;
    std::vector<double> sg(T);
    std::vector<float> nz(T);
    dsg_sigma_schedule(c, sg.data(), nullptr, nz.data(), nullptr);
    if (solver_2m(c))   // the update extrapolates D along the probability-flow ODE: a level that draws churn noise breaks the history
        for (int i = 0; i < T; i++) if (nz[i] != 0.f) return DSG_ERR_INVALID;
    if (!coef) return L;
    if (cap < L) return DSG_ERR_INVALID;
    std::vector<int32_t> sched(L);
    std::vector<float> jump(L);
    dsg_walk_steps(c, wk, sched.data(), jump.data(), L);
    for (int k = 0; k < L; k++) {
        const int i = sched[k];
        coef[k] = 0.f;
        if (!solver_2m(c) || k == 0 || i == T - 1 || sched[k - 1] != i - 1 || jump[k] != 0.f) continue;
        const double tp = (double)(float)sg[i - 1], tc = (double)(float)sg[i], tn = (double)(float)sg[i + 1];
        coef[k] = (float)(std::log(tc / tn) / (2.0 * std::log(tp / tc)));
    }
    return L;
}

}  // extern "C"

namespace {

// the caller's known tensors and element masks of a conditioned run
struct KnownArgs { const float *adj, *node; const uint8_t *mask_adj, *mask_node; };

// The table of pure-window rows (option "dedup_table").  The representative window that a batch shares at every level of
// the chain is a function of the weights and of the step's (scale, shift) row: its inputs are zero whatever the sample holds.  So it is
// computed here for all T schedule indices, before the loop, by the down path itself: pseudo-batches of B all-padding graphs -- graph
// g of a chunk reads row c0 + g of tab_aff, per-sample (aff_ld = aff_n) -- staged per graph (every graph's window 0 is its one unique
// window at every level), run as far as the first block of the top chain level, window 0 of every graph harvested level by level.
// Enqueued eagerly on the caller's stream behind embed_rows; leaves flags, lists and inputs of the pseudo-batch in the workspace:
// the caller stages its own flags again.  Grows like the tab_* buffers (the step bodies bake the address).
int build_pure_table(dsg_handle h, Workspace *w, int T, hipStream_t s) {
    const int B = w->B, depth = dedup_chain_depth(h, w);
    const PureTabLayout ptl = pure_tab_layout(h);
    if (depth < 1 || ptl.stride == 0) return fail(h, DSG_ERR_STATE, "dedup_table: no chain to build a table for");
    if (w->tab_pure_cap < T) {
        drop_graphs(h);
        w->bytes -= w->tab_pure_bytes;
        owned_free(w->allocs, w->tab_pure);
        w->tab_pure = nullptr; w->tab_pure_cap = 0; w->tab_pure_bytes = 0;
        if (int rc = owned_alloc(h, w->allocs, (void **)&w->tab_pure, sizeof(float) * ptl.stride * (size_t)T, AC_SCRATCH)) return rc;
        w->tab_pure_cap = T;
        w->tab_pure_bytes = sizeof(float) * ptl.stride * (size_t)T;
        w->bytes += w->tab_pure_bytes;
    }
    const size_t sa = (size_t)B * h->Ca * h->N * h->N, sn = (size_t)B * h->N * h->Cn;
    // the pseudo-batch's forwards are per-sample ones without a self-conditioning input; the workspace's host-side word on the kind
    // of its next forward goes back to what it was on every exit: a call whose step bodies are all replayed sets none of it again,
    // and an eager forward behind that call (dsg_profile_forward) must find the sampler's batch-uniform form
    struct FormGuard { Workspace *w; bool uniform; const float *sca, *scn; const int *hs;
                       ~FormGuard() { w->uniform = uniform; w->cur_sc_adj = sca; w->cur_sc_node = scn; w->cur_has_sc = hs; } }
        form_guard{w, w->uniform, w->cur_sc_adj, w->cur_sc_node, w->cur_has_sc};
    HIP_TRY(h, hipMemsetAsync(w->flags, 0, (size_t)B * h->N, s));
    if (int rc = stage_flags(h, w, nullptr, s, /*zero_padded=*/true, /*uniform_row=*/false)) return rc;
    HIP_TRY(h, hipMemsetAsync(w->in_adj, 0, sizeof(float) * sa, s));
    HIP_TRY(h, hipMemsetAsync(w->in_node, 0, sizeof(float) * sn, s));
    w->cur_sc_adj = nullptr; w->cur_sc_node = nullptr; w->cur_has_sc = nullptr;
    w->uniform = false;
    const size_t row = sizeof(float) * (size_t)h->aff_n;
    for (int c0 = 0; c0 < T; c0 += B) {
        const int n = std::min(B, T - c0);
        HIP_TRY(h, hipMemcpyAsync(w->aff, h->tab_aff + (size_t)c0 * h->aff_n, row * n, hipMemcpyDeviceToDevice, s));
        for (int g = n; g < B; g++)   // a short last chunk: the other graphs repeat its last row (computed, not harvested)
            HIP_TRY(h, hipMemcpyAsync(w->aff + (size_t)g * h->aff_n, h->tab_aff + (size_t)(T - 1) * h->aff_n, row, hipMemcpyDeviceToDevice, s));
        const TabBuild tb{depth - 1, w->tab_pure + (size_t)c0 * ptl.stride, n};
        forward_fixed(h, w, s, &tb);
        if (int rc = plan_status(h, w)) return rc;
    }
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// One run of the reverse loop, as dsg_sample, dsg_sample_known, dsg_sample_walk and dsg_sample_seeded describe it.
// walk == nullptr: the trivial walk (every schedule index once, from pure noise); base (a walk's partial-noise start) only reaches the
// initial state.  graph_seeds != nullptr: per-graph noise streams, `seed` then only draws the coins.  known.adj == nullptr: unconditioned.
struct SampleArgs {
    const dsg_sampler_cfg *cfg; const dsg_walk_cfg *walk; int32_t B; const uint8_t *flags;
    CStatePtrs init, base, noise; const uint8_t *coins; uint64_t seed; const uint64_t *graph_seeds;
    CStatePtrs gt; KnownArgs known;
    const dsg_guide_cfg *guide = nullptr; float *loss_trace = nullptr;   // box guidance (dsg_sample_guided); null: the unguided loop
    const dsg_rel_cfg *rel = nullptr;                                    // ... and its relation term (dsg_sample_guided_rel); null or w_rel == 0: none
    const dsg_content_cfg *content = nullptr; float *content_trace = nullptr;   // content guidance (dsg_sample_guided_content); null: none
    struct Snapshots { const int32_t *steps; int32_t n; float *adj, *node; } snapshots;
    StatePtrs outputs; dsg_sample_stats *stats; hipStream_t stream;
};

// all four known tensors or none (required: all four)
int known_args(dsg_handle h, const char *entry, bool required, const KnownArgs &k) {
    const int n = (k.adj != nullptr) + (k.node != nullptr) + (k.mask_adj != nullptr) + (k.mask_node != nullptr);
    if (n == 4 || (n == 0 && !required)) return 0;
    return fail(h, DSG_ERR_INVALID, "%s needs known_adj, known_node, mask_adj and mask_node%s (%s is NULL)", entry,
                required ? "" : " all given or all NULL", !k.adj ? "known_adj" : !k.node ? "known_node" : !k.mask_adj ? "mask_adj" : "mask_node");
}

// what the host works out before the device sees the run; its vectors are the source of async copies and live until the run's synchronise
struct SamplePlan {
    int T = 0, L = 0;              // schedule indices, executed steps
    float x0_scale = 0.f;          // sigma the initial state is drawn at
    std::vector<float> t_hat;      // [T] sigma of every schedule index
    std::vector<StepRow> rows;     // [L] the loop's scalars
    RunCtl ctl{};                  // the control block (graph_seeds: set once the seeds are staged)
    std::vector<StepPlan> plans;   // [L] the static launch sequence of every step
    int precond_calls = 0;
    bool use_graph = false;
    std::vector<float> guide_coef; // [T] c_i of a guided run
    GuideParams gpar{};            // ... and its parameter block (device pointers: set once the tables are staged)
    ContentParams cpar{};          // the content term's block, likewise
    bool autoguide = false;        // some step of the run is autoguided (dsg_attach_guide): the guide's workspace and tables are staged
};

// the checks of a guide descriptor that need no device; `why` names the argument.  Cn < 0: not known here
bool guide_cfg_ok(const dsg_guide_cfg *g, int N, int Cn, bool need_weights, std::string &why) {
    char buf[256];
    auto no = [&](const char *fmt, double v) { snprintf(buf, sizeof(buf), fmt, v); why = buf; return false; };
    if (!g) return no("guide is NULL", 0);
    if (Cn >= 0 && Cn < 4) return no("box guidance needs C_node >= 4 (the last four node channels are the box); C_node is %g", Cn);
    if (N > GUIDE_MAX_N) return no("box guidance keeps a graph's boxes on chip: N = %g is beyond 64", N);
    if (!std::isfinite(g->w_overlap)) return no("guide->w_overlap = %g is not finite", g->w_overlap);
    if (!std::isfinite(g->w_region)) return no("guide->w_region = %g is not finite", g->w_region);
    if (!std::isfinite(g->w_align)) return no("guide->w_align = %g is not finite", g->w_align);
    if (g->w_align != 0.f && !(g->tau > 0.f && std::isfinite(g->tau))) return no("guide->tau = %g must be positive (w_align is not 0)", g->tau);
    if (g->w_region != 0.f && (!g->sel || !g->region)) return no("guide->sel / guide->region are required with w_region = %g", g->w_region);
    if (!(g->clip_ratio >= 0.f)) return no("guide->clip_ratio = %g must be >= 0, or DSG_GUIDE_CLIP_NONE", g->clip_ratio);
    if (need_weights && !g->weights) return no("guide->weights is NULL (host, one weight per schedule index)", 0);
    return true;
}

// the checks of a relation descriptor that need no device; `why` names the argument.  Ca: the adjacency channels the decode would read
bool rel_cfg_ok(const dsg_rel_cfg *r, int Ca, std::string &why) {
    char buf[256];
    auto no = [&](const char *fmt, double v) { snprintf(buf, sizeof(buf), fmt, v); why = buf; return false; };
    if (!std::isfinite(r->w_rel)) return no("rel->w_rel = %g is not finite", r->w_rel);
    if (!(r->margin >= 0.f && std::isfinite(r->margin))) return no("rel->margin = %g must be >= 0 and finite", r->margin);
    if (r->source != DSG_REL_GIVEN && r->source != DSG_REL_DECODED) return no("rel->source = %g is neither DSG_REL_GIVEN (0) nor DSG_REL_DECODED (1)", r->source);
    if (r->source == DSG_REL_GIVEN) {
        if (r->w_rel != 0.f && !r->kinds) return no("rel->kinds is NULL (device, [B,N,N]) with the given source and w_rel = %g", r->w_rel);
        return true;
    }
    if (!r->pred_kind) return no("rel->pred_kind is NULL (host, one kind per predicate) with the decoded source", 0);
    if (r->n_adj_type < 1) return no("rel->n_adj_type = %g must be >= 1", r->n_adj_type);
    if (r->encoding < DSG_ENC_BITS || r->encoding > DSG_ENC_DDPM) return no("rel->encoding = %g must be DSG_ENC_BITS, DSG_ENC_ONE_HOT or DSG_ENC_DDPM", r->encoding);
    // the channel counts an encoding implies, as dsg_decode checks them
    if ((r->encoding == DSG_ENC_ONE_HOT && Ca != r->n_adj_type) || (r->encoding == DSG_ENC_DDPM && Ca != 1) ||
        (r->encoding == DSG_ENC_BITS && (Ca > 30 || (1 << Ca) < r->n_adj_type)))
        return no("rel->encoding with rel->n_adj_type = %g does not fit the adjacency channels", r->n_adj_type);
    for (int k = 0; k < r->n_adj_type; k++)
        if (r->pred_kind[k] >= REL_KINDS) { snprintf(buf, sizeof(buf), "rel->pred_kind[%d] = %d is above 7 (DSG_REL_ON)", k, (int)r->pred_kind[k]); why = buf; return false; }
    return true;
}
// the checks of a content descriptor that need no device; `why` names the argument
bool content_cfg_ok(const dsg_content_cfg *c, int B, int N, int Ca, int Cn, std::string &why) {
    char buf[256];
    auto no = [&](const char *fmt, double v) { snprintf(buf, sizeof(buf), fmt, v); why = buf; return false; };
    if (!std::isfinite(c->w_content)) return no("content->w_content = %g is not finite", c->w_content);
    if (!(c->tau > 0.f && std::isfinite(c->tau))) return no("content->tau = %g must be positive and finite", c->tau);
    if (!(c->clip_ratio >= 0.f)) return no("content->clip_ratio = %g must be >= 0, or DSG_GUIDE_CLIP_NONE", c->clip_ratio);
    if (c->n_items < 1 || c->n_items > DSG_CONTENT_MAX_ITEMS) return no("content->n_items = %g must be 1..16 (DSG_CONTENT_MAX_ITEMS)", c->n_items);
    if (Cn < 5 || c->node_chans < 1 || c->node_chans > Cn - 4) return no("content->node_chans = %g must be 1..C_node-4 (the label channels of a node row)", c->node_chans);
    if (N > GUIDE_MAX_N) return no("content guidance keeps a graph's pair tile on chip: N = %g is beyond 64", N);
    if (!c->subj) return no("content->subj is NULL (host, [B,K,node_chans])", 0);
    if (!c->obj) return no("content->obj is NULL (host, [B,K,node_chans])", 0);
    if (!c->pred) return no("content->pred is NULL (host, [B,K,C_adj])", 0);
    if (!c->w_spo) return no("content->w_spo is NULL (host, [B,K,3])", 0);
    const size_t bk = (size_t)B * c->n_items;
    for (size_t i = 0; i < bk * c->node_chans; i++) {
        if (!std::isfinite(c->subj[i])) return no("content->subj holds a target that is not finite (entry %g)", (double)i);
        if (!std::isfinite(c->obj[i])) return no("content->obj holds a target that is not finite (entry %g)", (double)i);
    }
    for (size_t i = 0; i < bk * Ca; i++) if (!std::isfinite(c->pred[i])) return no("content->pred holds a target that is not finite (entry %g)", (double)i);
    for (size_t i = 0; i < bk * 3; i++)
        if (!(c->w_spo[i] >= 0.f && std::isfinite(c->w_spo[i]))) return no("content->w_spo holds a weight that is negative or not finite (entry %g)", (double)i);
    return true;
}
// the part of the parameter block that a relation descriptor fills (pointers: set once staged); returns the plan's relation source
int rel_params(const dsg_rel_cfg *r, GuideParams &g) {
    if (!r || r->w_rel == 0.f) return REL_NONE;
    g.a_rel = r->w_rel; g.rel_margin = r->margin;
    g.rel_source = r->source == DSG_REL_DECODED ? REL_DECODED : REL_GIVEN;
    g.rel_enc = r->encoding; g.rel_ntype = r->n_adj_type;
    return g.rel_source;
}

// Host plan: argument checks, walk, schedule, coins, rows and step plans.  No HIP call.
int plan_sample(dsg_handle h, const SampleArgs &a, SamplePlan &p) {
    const dsg_sampler_cfg *cfg = a.cfg;
    if (int rc = check_ready(h, a.B)) return rc;
    if (!cfg || !a.flags || !a.outputs.adj || !a.outputs.node) return fail(h, DSG_ERR_INVALID, "null argument");
    if ((a.init.adj == nullptr) != (a.init.node == nullptr)) return fail(h, DSG_ERR_INVALID, "init_adj/init_node must both be given");
    if ((a.noise.adj == nullptr) != (a.noise.node == nullptr)) return fail(h, DSG_ERR_INVALID, "noise_adj/noise_node must both be given");
    if ((a.gt.adj == nullptr) != (a.gt.node == nullptr)) return fail(h, DSG_ERR_INVALID, "gt_adj/gt_node must both be given");
    if ((a.base.adj == nullptr) != (a.base.node == nullptr)) return fail(h, DSG_ERR_INVALID, "base_adj/base_node must both be given");
    const int T = p.T = cfg->num_steps;
    if (T < 1) return fail(h, DSG_ERR_INVALID, "num_steps < 1");
    // the walk: schedule index and churn coefficient of every executed step (the trivial walk: 0..T-1 with the schedule's own)
    const dsg_walk_cfg trivial{0, 1, 1, 0, 0, {0, 0, 0}};
    const dsg_walk_cfg *walk = a.walk ? a.walk : &trivial;
    const int32_t L = p.L = dsg_walk_steps(cfg, walk, nullptr, nullptr, 0);
    if (L < 0)
        return fail(h, DSG_ERR_INVALID, "bad walk: start_step %d, jump_len %d, n_resample %d, resample range [%d, %d) with num_steps %d "
                    "(need 0 <= start_step < T, jump_len >= 1, n_resample >= 1, start_step <= lo <= hi <= T, at most %d executed steps)",
                    walk->start_step, walk->jump_len, walk->n_resample, walk->resample_lo, walk->resample_hi <= 0 ? T : walk->resample_hi, T,
                    DSG_WALK_MAX_STEPS);
    if (walk->start_step > 0 && !a.base.adj)
        return fail(h, DSG_ERR_INVALID, "start_step %d > 0 needs base_adj / base_node (the graph the run starts from)", walk->start_step);
    std::vector<int32_t> sched(L);
    std::vector<float> coef(L), ms_coef(L);
    dsg_walk_steps(cfg, walk, sched.data(), coef.data(), L);
    if (dsg_multistep_coef(cfg, walk, ms_coef.data(), L) != L)   // the walk is good: what is left is a level with churn noise
        return fail(h, DSG_ERR_INVALID, "solver dpmpp_2m (heun = %d) needs a schedule that draws no churn noise at any level: set S_churn = 0 "
                    "(S_churn is %g)", DSG_SOLVER_DPMPP_2M, (double)cfg->S_churn);
    std::vector<float> nz(T), hs(T);
    std::vector<double> sg(T);
    p.t_hat.resize(T);
    dsg_sigma_schedule(cfg, sg.data(), p.t_hat.data(), nz.data(), hs.data());
    p.x0_scale = (float)sg[walk->start_step];   // x0 = init * sigma(t0) (edm.py:326, :346-347); a start past 0 has a base: x = base + t_s * eps
    // preconditioned calls of the walk: two per Heun step, one where the step is the Euler step to 0 (index T - 1); Euler and multistep: one
    int ncalls = 0;
    for (int k = 0; k < L; k++) ncalls += (solver_heun(cfg) && sched[k] != T - 1) ? 2 : 1;
    std::vector<uint8_t> coin_buf(ncalls, 0);
    if (a.coins) memcpy(coin_buf.data(), a.coins, ncalls);
    else if (h->cfg.self_condition) {
        std::mt19937_64 gen(a.seed ^ 0x9E3779B97F4A7C15ull);
        for (int i = 0; i < ncalls; i++) coin_buf[i] = (gen() >> 63) & 1;
    }
    p.rows.resize(L);
    for (int k = 0; k < L; k++) {
        const int i = sched[k];
        volatile float t_prime = p.t_hat[i] + hs[i];  // alpha = 1 (edm.py:391)
        p.rows[k] = StepRow{coef[k], p.t_hat[i], 1.0f / p.t_hat[i], 1.0f / t_prime, hs[i], i, ms_coef[k], 0};
    }
    p.ctl = RunCtl{0, L, (unsigned long long)a.seed, a.noise.adj, a.noise.node, nullptr};   // nothing sticky: rewritten by every run
    p.use_graph = cfg->use_graph != 0 && !a.gt.adj && h->taps.empty();
    // the static plan of every executed step (edm.py:350-427): buffer rotation (it simply continues across a jump: the
    // self-conditioning input is the last denoised estimate, whichever level it came from), Euler/Heun/multistep update, the pre-drawn coins
    const bool gt = a.gt.adj != nullptr;
    p.plans.resize(L);
    int call = 0;
    int sc_slot = -1;  // which d_* buffer holds the current self-cond, -1 = None
    int last_s1 = -1;  // which d_* buffer the previous step's D went to (a network without self-conditioning keeps no sc_slot)
    auto free_slot = [&](int s0, int s1) { for (int k = 0; k < 3; k++) if (k != s0 && k != s1) return k; return 0; };
    for (int i = 0; i < L; i++) {
        StepPlan &q = p.plans[i];
        q.sc_slot = sc_slot;
        // a multistep step (coefficient != 0, so never the first) reads the previous step's D: the self-conditioning input where the
        // network has one (the D of a fired coin's extra pass goes to w->sc_*, not there), else the previous s1; s1 avoids both.
        // Every other step is planned as ever (prev = -1).  Sanity-check mode: no slot is read, D_prev = D = gt
        if (ms_coef[i] != 0.f) q.prev = gt ? 0 : (h->cfg.self_condition ? sc_slot : last_s1);
        q.s1 = free_slot(sc_slot, q.prev);
        q.s2 = free_slot(q.s1, -1);
        q.euler = !solver_heun(cfg) || sched[i] == T - 1;   // edm.py:394-396
        q.known = a.known.adj != nullptr;
        q.coin1 = !gt && coin_buf[call] != 0;
        q.coin2 = !gt && !q.euler && coin_buf[call + 1] != 0;
        if (!gt) call += q.euler ? 1 : 2;
        if (!gt && h->cfg.self_condition) sc_slot = q.euler ? q.s1 : q.s2;   // edm.py:423-424: sc <- last denoised
        if (!gt) last_s1 = q.s1;
    }
    p.precond_calls = call;
    // autoguidance: sigma is batch-uniform in the loop, so the host decides per schedule index, from the float32 t_hat, whether the step
    // is guided.  Scale 1 or a level outside the interval: the bit stays clear and the step is the plain one, no guide forward at all
    if (h->guide && !gt && h->guide_sm1 != 0.f)
        for (int i = 0; i < L; i++) {
            const float t = p.t_hat[sched[i]];
            p.plans[i].autoguide = t >= h->guide_lo && t <= h->guide_hi;
            p.autoguide = p.autoguide || p.plans[i].autoguide;
        }
    if (a.guide) {   // box guidance: refusals, the coefficient table, the shift buffers of every step
        std::string why;
        if (!guide_cfg_ok(a.guide, h->N, h->Cn, /*need_weights=*/true, why)) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided: %s", why.c_str());
        if (gt && (a.known.adj || a.graph_seeds)) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided: gt_adj / gt_node (sanity-check mode) go with neither known_* nor graph_seeds");
        p.guide_coef.resize(T);
        if (dsg_guide_coef(cfg, a.guide->weights, p.guide_coef.data(), T) != T)
            return fail(h, DSG_ERR_INVALID, "dsg_sample_guided: guide->weights holds a weight that is not finite");
        const bool clip = !std::isinf(a.guide->clip_ratio);
        int last_g = -1;   // the shift buffer of the previous step's stage 1
        for (int i = 0; i < L; i++) {
            StepPlan &q = p.plans[i];
            q.guided = true; q.clip = clip;
            q.g1 = free_slot(last_g, -1);
            q.g2 = free_slot(q.g1, last_g);
            q.gprev = q.prev >= 0 ? last_g : -1;
            last_g = q.g1;
        }
        p.gpar = GuideParams{a.guide->w_overlap, a.guide->w_region, a.guide->w_align, a.guide->tau, clip ? a.guide->clip_ratio : 0.f, 0,
                             nullptr, nullptr, nullptr, nullptr, nullptr};
        if (a.rel) {
            if (!rel_cfg_ok(a.rel, h->Ca, why)) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided_rel: %s", why.c_str());
            const int rel = rel_params(a.rel, p.gpar);
            for (int i = 0; i < L; i++) p.plans[i].rel = rel;
        }
        if (a.content) {   // the content term rides on the guided plan: the same coefficients, the same slot rotation
            if (!content_cfg_ok(a.content, a.B, h->N, h->Ca, h->Cn, why)) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided_content: %s", why.c_str());
            const bool cclip = !std::isinf(a.content->clip_ratio);
            const int cgrid = content_grid_items(a.content->n_items);
            for (int i = 0; i < L; i++) { p.plans[i].content = true; p.plans[i].cclip = cclip; p.plans[i].cgrid = cgrid; }
            p.cpar = ContentParams{a.content->w_content, a.content->tau, cclip ? a.content->clip_ratio : 0.f, a.content->n_items,
                                   a.content->node_chans, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        }
    }
    return 0;
}

// Initial state.  Every state the loop's forwards read (x_hat, the denoised estimates, the known-entry select) is stored as
// `valid ? ... : 0.f` by the elementwise skeleton (Init, Churn, PrecondOut and the update operations): zero at padded pairs whatever
// the caller passed ... and every forward of the loop goes through precond_tab: one sigma, one (scale, shift) row for the whole batch
int initial_state(dsg_handle h, Workspace *w, const SampleArgs &a, const SamplePlan &p, hipStream_t s) {
    if (int rc = stage_flags(h, w, a.flags, s, /*zero_padded=*/true, /*uniform_row=*/true)) return rc;
    if (a.graph_seeds) if (int rc = stage_seeds(h, w, a.graph_seeds, s)) return rc;
    launch_init(a.init, a.base, p.x0_scale, a.seed, a.graph_seeds ? w->gseeds : nullptr, 0u, w->flags, StatePtrs{w->x_adj, w->x_node},
                dims_of(h, a.B), s);
    return 0;
}

// Step tables on the device: the loop's scalars (StepRow) and, since sigma is batch-uniform (edm.py:371), one noise embedding +
// (scale,shift) row per step for all blocks, computed once for all steps in three GEMMs with M = T
int pure_window_table(dsg_handle h, Workspace *w, const SampleArgs &a, const SamplePlan &p, hipStream_t s);
// the per-schedule-index tables of handle h: its noise embedding and (scale, shift) rows at the run's levels
int noise_tables(dsg_handle h, const SamplePlan &p, hipStream_t s) {
    const int T = p.T;
    if (h->tab_cap < T) {
        drop_graphs(h);   // the captured step bodies bake the table addresses
        for (float **q : {&h->tab_sig, &h->tab_cn, &h->tab_pe, &h->tab_e0, &h->tab_e1, &h->tab_aff}) { owned_free(h->allocs, *q); *q = nullptr; }
        h->tab_cap = 0;
        const std::pair<float **, size_t> tabs[] = {{&h->tab_sig, (size_t)T}, {&h->tab_cn, (size_t)T}, {&h->tab_pe, (size_t)T * h->E},
                                                    {&h->tab_e0, (size_t)T * NOISE_EMB}, {&h->tab_e1, (size_t)T * NOISE_EMB},
                                                    {&h->tab_aff, (size_t)T * h->aff_n}};
        for (auto &t : tabs) if (int rc = owned_alloc(h, h->allocs, (void **)t.first, sizeof(float) * t.second, AC_SCRATCH)) return rc;
        h->tab_cap = T;
    }
    HIP_TRY(h, hipMemcpyAsync(h->tab_sig, p.t_hat.data(), sizeof(float) * T, hipMemcpyHostToDevice, s));
    launch_cnoise(h->tab_sig, h->tab_cn, T, s);
    embed_rows(h, h->tab_cn, T, h->tab_pe, h->tab_e0, h->tab_e1, h->tab_aff, s);
    return 0;
}

int step_tables(dsg_handle h, Workspace *w, const SampleArgs &a, SamplePlan &p, hipStream_t s) {
    const int L = p.L;
    if (h->tab_step_cap < L) {   // one row per executed step: its own capacity, the tables above stay at one row per schedule index
        drop_graphs(h);
        owned_free(h->allocs, h->tab_step);
        h->tab_step = nullptr; h->tab_step_cap = 0;
        if (int rc = owned_alloc(h, h->allocs, (void **)&h->tab_step, sizeof(StepRow) * (size_t)L, AC_STATE)) return rc;
        h->tab_step_cap = L;
    }
    if (a.graph_seeds) p.ctl.graph_seeds = w->gseeds;
    HIP_TRY(h, hipMemcpyAsync(h->tab_step, p.rows.data(), sizeof(StepRow) * L, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(w->ctl, &p.ctl, sizeof(RunCtl), hipMemcpyHostToDevice, s));
    if (a.gt.adj) return 0;   // sanity-check mode: no forward reads a table
    return noise_tables(h, p, s);
}

// Autoguidance: what the guide's forwards of this run read, staged in the guide handle's workspace before any body is captured -- the
// flags and their lists, the guide's own (scale, shift) table from its own affine linears on the same schedule, its table of pure-window
// rows.  The step table and the control block are the main handle's
int stage_autoguide(dsg_handle g, Workspace *wg, const SampleArgs &a, const SamplePlan &p, hipStream_t s) {
    if (int rc = stage_flags(g, wg, a.flags, s, /*zero_padded=*/true, /*uniform_row=*/true)) return rc;
    if (int rc = noise_tables(g, p, s)) return rc;
    return pure_window_table(g, wg, a, p, s);
}

// Pure-window table: where the batch shares one representative pure window per level, that window comes from a table with one entry
// per schedule index, built now from the rows of tab_aff; then the caller's flags again, with lists that leave the window to the fill.
// DSG_TABLE_VERBOSE (measurement): HIP events around the build of this call
int pure_window_table(dsg_handle h, Workspace *w, const SampleArgs &a, const SamplePlan &p, hipStream_t s) {
    if (a.gt.adj || !h->opt.dedup_table || w->dd_mode != DD_BATCH) return 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (getenv("DSG_TABLE_VERBOSE")) {
        HIP_TRY(h, hipEventCreate(&ev[0]));
        HIP_TRY(h, hipEventCreate(&ev[1]));
        HIP_TRY(h, hipEventRecord(ev[0], s));
    }
    int rc = build_pure_table(h, w, p.T, s);
    if (!rc) rc = stage_flags(h, w, a.flags, s, /*zero_padded=*/true, /*uniform_row=*/true, /*table=*/true);
    float ms = 0.f;
    if (!rc && ev[1] && hipEventRecord(ev[1], s) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
        hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
        fprintf(stderr, "[dsg-table] B=%d T=%d: table of pure-window rows built in %.1f us (%zu bytes)\n", a.B, p.T, ms * 1e3, w->tab_pure_bytes);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return rc;
}

// Known staging: the known tensors and masks move into workspace-owned buffers: conditioned step bodies bake these addresses and must
// not reference caller memory.  Staged on the caller's stream ahead of the run's synchronise, i.e. before any body is captured
int stage_known(dsg_handle h, Workspace *w, const KnownArgs &known, hipStream_t s) {
    if (!known.adj) return 0;
    const size_t sa = (size_t)w->B * h->Ca * h->N * h->N, sn = (size_t)w->B * h->N * h->Cn;
    if (!w->kn_adj) {
        void *q;
        if (int rc = owned_alloc(h, w->allocs, &q, sizeof(float) * sa, AC_SCRATCH)) return rc;
        w->kn_adj = (float *)q;
        if (int rc = owned_alloc(h, w->allocs, &q, sizeof(float) * sn, AC_SCRATCH)) return rc;
        w->kn_node = (float *)q;
        if (int rc = owned_alloc(h, w->allocs, &q, sa, AC_STATE)) return rc;
        w->km_adj = (uint8_t *)q;
        if (int rc = owned_alloc(h, w->allocs, &q, sn, AC_STATE)) return rc;
        w->km_node = (uint8_t *)q;
        w->known_bytes = (sizeof(float) + 1) * (sa + sn);
        w->bytes += w->known_bytes;
    }
    HIP_TRY(h, hipMemcpyAsync(w->kn_adj, known.adj, sizeof(float) * sa, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(w->kn_node, known.node, sizeof(float) * sn, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(w->km_adj, known.mask_adj, sa, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(w->km_node, known.mask_node, sn, hipMemcpyDeviceToDevice, s));
    return 0;
}

// Guide staging: sel, region, the coefficient table and the parameter block move into workspace-owned memory, on the caller's stream
// ahead of the run's synchronise; guided step bodies bake the block's address and the shift / norm buffers, never caller memory
int stage_guide(dsg_handle h, Workspace *w, const SampleArgs &a, SamplePlan &p, hipStream_t s) {
    if (!a.guide) return 0;
    const size_t bn = (size_t)w->B * h->N;
    void *q;
    auto grow = [&](void **dst, size_t bytes, size_t old_bytes, AllocClass cls) {
        owned_free(w->allocs, *dst); *dst = nullptr;
        if (int rc = owned_alloc(h, w->allocs, dst, bytes, cls)) return rc;
        w->guide_bytes += bytes - old_bytes; w->bytes += bytes - old_bytes;
        return 0;
    };
    if (!w->g_par) {
        if (int rc = grow(&(q = nullptr), sizeof(GuideParams), 0, AC_STATE)) return rc;
        w->g_par = (GuideParams *)q;
        for (int k = 0; k < 3; k++) { if (int rc = grow(&(q = nullptr), sizeof(float) * bn * 4, 0, AC_SCRATCH)) return rc; w->g_shift[k] = (float *)q; }
        if (int rc = grow(&(q = nullptr), sizeof(double) * (size_t)w->B, 0, AC_SCRATCH)) return rc;
        w->g_ref = (double *)q;
        if (int rc = grow(&(q = nullptr), bn, 0, AC_STATE)) return rc;
        w->g_sel = (uint8_t *)q;
        if (int rc = grow(&(q = nullptr), sizeof(float) * bn * 4, 0, AC_SCRATCH)) return rc;
        w->g_region = (float *)q;
    }
    if (w->g_coef_cap < p.T) {
        if (int rc = grow(&(q = w->g_coef), sizeof(float) * (size_t)p.T, sizeof(float) * (size_t)w->g_coef_cap, AC_SCRATCH)) return rc;
        w->g_coef = (float *)q; w->g_coef_cap = p.T;
    }
    const size_t trace_n = (size_t)p.L * w->B;
    if (a.loss_trace && w->g_trace_cap < trace_n) {
        if (int rc = grow(&(q = w->g_trace), sizeof(float) * trace_n, sizeof(float) * w->g_trace_cap, AC_SCRATCH)) return rc;
        w->g_trace = (float *)q; w->g_trace_cap = trace_n;
    }
    if (a.guide->w_region != 0.f) {
        HIP_TRY(h, hipMemcpyAsync(w->g_sel, a.guide->sel, bn, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(w->g_region, a.guide->region, sizeof(float) * bn * 4, hipMemcpyDeviceToDevice, s));
    }
    if (p.gpar.rel_source == REL_GIVEN) {   // the kinds, like sel / region; a_rel != 0 here (rel_params)
        const size_t bnn = bn * h->N;
        if (!w->g_kinds) { if (int rc = grow(&(q = nullptr), bnn, 0, AC_STATE)) return rc; w->g_kinds = (uint8_t *)q; }
        HIP_TRY(h, hipMemcpyAsync(w->g_kinds, a.rel->kinds, bnn, hipMemcpyDeviceToDevice, s));
        p.gpar.kinds = w->g_kinds;
    } else if (p.gpar.rel_source == REL_DECODED) {   // the table: the caller's host array outlives the run's synchronise
        if (w->g_predk_cap < p.gpar.rel_ntype) {
            if (int rc = grow(&(q = w->g_predk), (size_t)p.gpar.rel_ntype, (size_t)w->g_predk_cap, AC_STATE)) return rc;
            w->g_predk = (uint8_t *)q; w->g_predk_cap = p.gpar.rel_ntype;
        }
        HIP_TRY(h, hipMemcpyAsync(w->g_predk, a.rel->pred_kind, (size_t)p.gpar.rel_ntype, hipMemcpyHostToDevice, s));
        p.gpar.pred_kind = w->g_predk;
    }
    HIP_TRY(h, hipMemcpyAsync(w->g_coef, p.guide_coef.data(), sizeof(float) * (size_t)p.T, hipMemcpyHostToDevice, s));
    p.gpar.sel = w->g_sel; p.gpar.region = w->g_region; p.gpar.coef = w->g_coef;
    p.gpar.trace = a.loss_trace ? w->g_trace : nullptr;
    p.gpar.mask_node = a.known.adj ? w->km_node : nullptr;   // stage_known ran: the workspace's copy
    HIP_TRY(h, hipMemcpyAsync(w->g_par, &p.gpar, sizeof(GuideParams), hipMemcpyHostToDevice, s));
    if (!a.content) return 0;
    // the content term: block and shift buffers once, the targets and weights of this run behind the block's pointers
    const size_t sa = bn * h->N * h->Ca, sl = bn * (size_t)(h->Cn - 4);
    if (!w->c_par) {   // the block is allocated last: a call after a failed allocation starts over instead of launching on null buffers
        for (int k = 0; k < 3; k++) {
            if (!w->c_shift_adj[k]) { if (int rc = grow(&(q = nullptr), sizeof(float) * sa, 0, AC_SCRATCH)) return rc; w->c_shift_adj[k] = (float *)q; }
            if (!w->c_shift_label[k]) { if (int rc = grow(&(q = nullptr), sizeof(float) * sl, 0, AC_SCRATCH)) return rc; w->c_shift_label[k] = (float *)q; }
        }
        if (!w->c_stats) {
            if (int rc = grow(&(q = nullptr), sizeof(double) * (size_t)w->B * CONTENT_STATS_PER_GRAPH, 0, AC_SCRATCH)) return rc;
            w->c_stats = (double *)q;
        }
        if (int rc = grow(&(q = nullptr), sizeof(ContentParams), 0, AC_STATE)) return rc;
        w->c_par = (ContentParams *)q;
    }
    const size_t bk = (size_t)w->B * p.cpar.K, n_lab = bk * p.cpar.Cl, n_pred = bk * h->Ca, n_tgt = 2 * n_lab + n_pred + 3 * bk;
    if (w->c_tgt_cap < n_tgt) {
        if (int rc = grow(&(q = w->c_tgt), sizeof(float) * n_tgt, sizeof(float) * w->c_tgt_cap, AC_SCRATCH)) return rc;
        w->c_tgt = (float *)q; w->c_tgt_cap = n_tgt;
    }
    if (a.content_trace && w->c_trace_cap < trace_n) {
        if (int rc = grow(&(q = w->c_trace), sizeof(float) * trace_n, sizeof(float) * w->c_trace_cap, AC_SCRATCH)) return rc;
        w->c_trace = (float *)q; w->c_trace_cap = trace_n;
    }
    float *t_subj = w->c_tgt, *t_obj = t_subj + n_lab, *t_pred = t_obj + n_lab, *t_w = t_pred + n_pred;
    HIP_TRY(h, hipMemcpyAsync(t_subj, a.content->subj, sizeof(float) * n_lab, hipMemcpyHostToDevice, s));   // the caller's host arrays outlive the run's synchronise
    HIP_TRY(h, hipMemcpyAsync(t_obj, a.content->obj, sizeof(float) * n_lab, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(t_pred, a.content->pred, sizeof(float) * n_pred, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(t_w, a.content->w_spo, sizeof(float) * 3 * bk, hipMemcpyHostToDevice, s));
    p.cpar.subj = t_subj; p.cpar.obj = t_obj; p.cpar.pred = t_pred; p.cpar.w_spo = t_w;
    p.cpar.coef = w->g_coef;
    p.cpar.trace = a.content_trace ? w->c_trace : nullptr;
    p.cpar.mask_adj = a.known.adj ? w->km_adj : nullptr;
    p.cpar.mask_node = a.known.adj ? w->km_node : nullptr;
    HIP_TRY(h, hipMemcpyAsync(w->c_par, &p.cpar, sizeof(ContentParams), hipMemcpyHostToDevice, s));
    return 0;
}

// Loop: every step body captured before the first launch, then replay (or enqueue), snapshots, outputs, stats
int run_loop(dsg_handle h, Workspace *w, const SampleArgs &a, const SamplePlan &p, hipStream_t s) {
    const size_t sa = (size_t)a.B * h->Ca * h->N * h->N, sn = (size_t)a.B * h->N * h->Cn;
    const bool step_graphs = p.use_graph && h->opt.loop_graph;
    if (step_graphs)
        for (int i = 0; i < p.L; i++) if (int rc = ensure_step_graph(h, w, p.plans[i])) return rc;   // at most ten distinct bodies
    int snap_k = 0, nfe = 0, gfe = 0;
    for (int i = 0; i < p.L; i++) {
        if (step_graphs) { if (int rc = replay_step(h, w, p.plans[i], s, &nfe, &gfe)) return rc; }
        else if (int rc = enqueue_step(h, w, p.plans[i], a.gt.adj, a.gt.node, s, &nfe, &gfe, p.use_graph)) return rc;
        // interim snapshots (edm.py:429-432)
        while (snap_k < a.snapshots.n && a.snapshots.steps && a.snapshots.steps[snap_k] == i) {
            if (a.snapshots.adj) HIP_TRY(h, hipMemcpyAsync(a.snapshots.adj + (size_t)snap_k * sa, w->x_adj, sizeof(float) * sa, hipMemcpyDeviceToDevice, s));
            if (a.snapshots.node) HIP_TRY(h, hipMemcpyAsync(a.snapshots.node + (size_t)snap_k * sn, w->x_node, sizeof(float) * sn, hipMemcpyDeviceToDevice, s));
            snap_k++;
        }
    }
    HIP_TRY(h, hipMemcpyAsync(a.outputs.adj, w->x_adj, sizeof(float) * sa, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(a.outputs.node, w->x_node, sizeof(float) * sn, hipMemcpyDeviceToDevice, s));
    if (a.guide && a.loss_trace) HIP_TRY(h, hipMemcpyAsync(a.loss_trace, w->g_trace, sizeof(float) * (size_t)p.L * a.B, hipMemcpyDeviceToDevice, s));
    if (a.content && a.content_trace) HIP_TRY(h, hipMemcpyAsync(a.content_trace, w->c_trace, sizeof(float) * (size_t)p.L * a.B, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipGetLastError());
    h->last_stats.precond_calls = p.precond_calls;
    h->last_stats.net_forwards = nfe;
    h->last_guide_forwards = gfe;
    if (a.stats) *a.stats = h->last_stats;
    return DSG_OK;
}

int sample_impl(dsg_handle h, const SampleArgs &a) {
    SamplePlan p;
    if (int rc = plan_sample(h, a, p)) return rc;
    hipStream_t s = a.stream;
    Workspace *w;
    if (int rc = get_workspace(h, a.B, &w)) return rc;
    dsg_handle g = p.autoguide ? h->guide : nullptr;
    Workspace *wg = nullptr;   // the guide's workspace: created, and its launch plan validated, before anything is enqueued
    if (g) {
        if (int rc = check_ready(g, a.B)) return guide_fail(h, g, rc);
        if (int rc = get_workspace(g, a.B, &wg)) return guide_fail(h, g, rc);
    }
    h->last_stats = dsg_sample_stats{};
    h->last_guide_forwards = 0;
    if (int rc = initial_state(h, w, a, p, s)) return rc;
    if (int rc = step_tables(h, w, a, p, s)) return rc;
    if (int rc = pure_window_table(h, w, a, p, s)) return rc;
    if (g) if (int rc = stage_autoguide(g, wg, a, p, s)) return guide_fail(h, g, rc);
    if (int rc = stage_known(h, w, a.known, s)) return rc;
    if (int rc = stage_guide(h, w, a, p, s)) return rc;
    HIP_TRY(h, hipStreamSynchronize(s));  // the plan's host vectors (and the caller's seeds) must outlive their async copies; once per sample() call
    return run_loop(h, w, a, p, s);
}

}  // namespace

extern "C" {

int dsg_sample(dsg_handle h, const dsg_sampler_cfg *cfg, int32_t B, const uint8_t *flags, const float *init_adj,
               const float *init_node, const float *noise_adj, const float *noise_node, const uint8_t *coins, uint64_t seed,
               const float *gt_adj, const float *gt_node, const int32_t *snap_steps, int32_t n_snap, float *snap_adj,
               float *snap_node, float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream) {
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.gt = {gt_adj, gt_node};
    return sample_impl(h, a);
}

int dsg_sample_known(dsg_handle h, const dsg_sampler_cfg *cfg, int32_t B, const uint8_t *flags, const float *init_adj,
                     const float *init_node, const float *noise_adj, const float *noise_node, const uint8_t *coins, uint64_t seed,
                     const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                     const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node, float *out_adj, float *out_node,
                     dsg_sample_stats *stats, void *stream) {
    if (!h) return DSG_ERR_INVALID;
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.known = {known_adj, known_node, mask_adj, mask_node};
    if (int rc = known_args(h, "dsg_sample_known", /*required=*/true, a.known)) return rc;
    return sample_impl(h, a);
}

int dsg_sample_walk(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                    const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                    const float *noise_adj, const float *noise_node, const uint8_t *coins, uint64_t seed,
                    const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                    const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node, float *out_adj, float *out_node,
                    dsg_sample_stats *stats, void *stream) {
    if (!h) return DSG_ERR_INVALID;
    if (!walk) return fail(h, DSG_ERR_INVALID, "dsg_sample_walk needs a walk (walk is NULL)");
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.walk = walk;
    a.base = {base_adj, base_node};
    a.known = {known_adj, known_node, mask_adj, mask_node};
    if (int rc = known_args(h, "dsg_sample_walk", /*required=*/false, a.known)) return rc;
    return sample_impl(h, a);
}

int dsg_sample_seeded(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                      const uint64_t *graph_seeds, uint64_t coin_seed,
                      const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                      const float *noise_adj, const float *noise_node, const uint8_t *coins,
                      const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                      const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node, float *out_adj, float *out_node,
                      dsg_sample_stats *stats, void *stream) {
    if (!h) return DSG_ERR_INVALID;
    if (!graph_seeds) return fail(h, DSG_ERR_INVALID, "dsg_sample_seeded needs graph_seeds (host, one per graph); graph_seeds is NULL");
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = coin_seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.walk = walk;
    a.base = {base_adj, base_node};
    a.graph_seeds = graph_seeds;
    a.known = {known_adj, known_node, mask_adj, mask_node};
    if (int rc = known_args(h, "dsg_sample_seeded", /*required=*/false, a.known)) return rc;
    return sample_impl(h, a);
}

int32_t dsg_guide_coef(const dsg_sampler_cfg *cfg, const float *weights, float *coef, int32_t cap) {
    if (!cfg || !weights || !coef || cfg->num_steps < 1 || cap < cfg->num_steps) return DSG_ERR_INVALID;
    const int T = cfg->num_steps;
    std::vector<float> t_hat(T), nz(T), hs(T);
    std::vector<double> sg(T);
    if (dsg_sigma_schedule(cfg, sg.data(), t_hat.data(), nz.data(), hs.data()) != DSG_OK) return DSG_ERR_INVALID;
    for (int i = 0; i < T; i++) {
        if (!std::isfinite(weights[i])) return DSG_ERR_INVALID;
        // evaluated in double on the float32 level and rounded once, like dsg_multistep_coef: within half an ulp of the real value (the
        // same formula float32 operation by operation strays up to 3.5 ulp)
        const double t = (double)t_hat[i];
        coef[i] = (float)((double)weights[i] * t * t * (0.25 / (t * t + 0.25)));
    }
    return T;
}

int dsg_sample_guided(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                      const uint64_t *graph_seeds, uint64_t coin_seed,
                      const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                      const float *noise_adj, const float *noise_node, const uint8_t *coins,
                      const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                      const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                      const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                      float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream) {
    if (!h) return DSG_ERR_INVALID;
    if (!guide) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided needs a guide descriptor (guide is NULL)");
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = coin_seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.walk = walk;
    a.base = {base_adj, base_node};
    a.graph_seeds = graph_seeds;
    a.known = {known_adj, known_node, mask_adj, mask_node};
    a.gt = {gt_adj, gt_node};
    a.guide = guide; a.loss_trace = loss_trace;
    if (int rc = known_args(h, "dsg_sample_guided", /*required=*/false, a.known)) return rc;
    return sample_impl(h, a);
}

int dsg_sample_guided_rel(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                          const uint64_t *graph_seeds, uint64_t coin_seed,
                          const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                          const float *noise_adj, const float *noise_node, const uint8_t *coins,
                          const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                          const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                          const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                          float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream, const dsg_rel_cfg *rel) {
    if (!h) return DSG_ERR_INVALID;
    if (!guide) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided_rel needs a guide descriptor (guide is NULL)");
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = coin_seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.walk = walk;
    a.base = {base_adj, base_node};
    a.graph_seeds = graph_seeds;
    a.known = {known_adj, known_node, mask_adj, mask_node};
    a.gt = {gt_adj, gt_node};
    a.guide = guide; a.loss_trace = loss_trace;
    a.rel = rel;
    if (int rc = known_args(h, "dsg_sample_guided_rel", /*required=*/false, a.known)) return rc;
    return sample_impl(h, a);
}

int dsg_sample_guided_content(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                              const uint64_t *graph_seeds, uint64_t coin_seed,
                              const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                              const float *noise_adj, const float *noise_node, const uint8_t *coins,
                              const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                              const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                              const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                              float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream, const dsg_rel_cfg *rel,
                              const dsg_content_cfg *content, float *content_trace) {
    if (!h) return DSG_ERR_INVALID;
    if (!guide) return fail(h, DSG_ERR_INVALID, "dsg_sample_guided_content needs a guide descriptor (guide is NULL)");
    SampleArgs a{};
    a.cfg = cfg; a.B = B; a.flags = flags; a.init = {init_adj, init_node}; a.noise = {noise_adj, noise_node}; a.coins = coins; a.seed = coin_seed;
    a.snapshots = {snap_steps, n_snap, snap_adj, snap_node}; a.outputs = {out_adj, out_node}; a.stats = stats; a.stream = (hipStream_t)stream;
    a.walk = walk;
    a.base = {base_adj, base_node};
    a.graph_seeds = graph_seeds;
    a.known = {known_adj, known_node, mask_adj, mask_node};
    a.gt = {gt_adj, gt_node};
    a.guide = guide; a.loss_trace = loss_trace;
    a.rel = rel;
    if (content && content->w_content != 0.f) { a.content = content; a.content_trace = content_trace; }   // else: dsg_sample_guided_rel itself
    if (int rc = known_args(h, "dsg_sample_guided_content", /*required=*/false, a.known)) return rc;
    return sample_impl(h, a);
}

int dsg_debug_content_guide(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                            const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_adj, const uint8_t *mask_node,
                            const dsg_content_cfg *content, float coef, float *loss, float *item_loss, float *grad_adj, float *grad_label,
                            float *shift_adj, float *shift_label, float *factor, float *norms, int32_t *best, float *d_guided_adj,
                            float *d_guided_node, void *stream) {
    std::string why;
    const char *me = "dsg_debug_content_guide: ";
    if (B < 1 || N < 1 || c_adj < 1) { g_create_err = std::string(me) + "B, N and c_adj must be >= 1"; return DSG_ERR_INVALID; }
    if (!content) { g_create_err = std::string(me) + "content is NULL"; return DSG_ERR_INVALID; }
    if (!content_cfg_ok(content, B, N, c_adj, c_node, why)) { g_create_err = me + why; return DSG_ERR_INVALID; }
    if (!std::isfinite(coef)) { g_create_err = std::string(me) + "coef is not finite"; return DSG_ERR_INVALID; }
    const bool clip = !std::isinf(content->clip_ratio);
    if (!d_adj || !d_node || !flags || (clip && (!xhat_adj || !xhat_node))) { g_create_err = std::string(me) + "null argument (d_adj, d_node, flags; with a clip also xhat_adj, xhat_node)"; return DSG_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const Dims d{B, N, c_adj, c_node};
    const int K = content->n_items, Cl = content->node_chans;
    const size_t bk = (size_t)B * K, n_lab = bk * Cl, n_pred = bk * c_adj, n_tgt = 2 * n_lab + n_pred + 3 * bk;
    const size_t sa = (size_t)B * c_adj * N * N, sl = (size_t)B * N * Cl;
    ContentParams *d_par = nullptr; double *d_ref = nullptr, *d_st = nullptr; float *d_tgt = nullptr, *d_sa = nullptr, *d_sl = nullptr;
    const int cgrid = content_grid_items(K);
    hipError_t e = hipMalloc((void **)&d_par, sizeof(ContentParams));
    if (e == hipSuccess) e = hipMalloc((void **)&d_ref, sizeof(double) * (size_t)B);
    if (e == hipSuccess) e = hipMalloc((void **)&d_tgt, sizeof(float) * n_tgt);
    if (e == hipSuccess) e = hipMalloc((void **)&d_sa, sizeof(float) * sa);
    if (e == hipSuccess) e = hipMalloc((void **)&d_sl, sizeof(float) * sl);
    if (e == hipSuccess && cgrid) e = hipMalloc((void **)&d_st, sizeof(double) * (size_t)B * CONTENT_STATS_PER_GRAPH);
    float *t_subj = d_tgt, *t_obj = d_tgt + n_lab, *t_pred = d_tgt + 2 * n_lab, *t_w = d_tgt + 2 * n_lab + n_pred;
    if (e == hipSuccess) e = hipMemcpyAsync(t_subj, content->subj, sizeof(float) * n_lab, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(t_obj, content->obj, sizeof(float) * n_lab, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(t_pred, content->pred, sizeof(float) * n_pred, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(t_w, content->w_spo, sizeof(float) * 3 * bk, hipMemcpyHostToDevice, s);
    const ContentParams par{content->w_content, content->tau, clip ? content->clip_ratio : 0.f, K, Cl, 0, t_subj, t_obj, t_pred, t_w, nullptr, nullptr,
                            mask_adj, mask_node};
    if (e == hipSuccess) e = hipMemcpyAsync(d_par, &par, sizeof(ContentParams), hipMemcpyHostToDevice, s);
    bool ok = e == hipSuccess;
    if (ok && clip) ok = launch_graph_diff_norm(CStatePtrs{xhat_adj, xhat_node}, CStatePtrs{d_adj, d_node}, flags, d_ref, d, s);
    if (ok) ok = launch_content_guide(d_par, nullptr, nullptr, coef, d_adj, d_node, flags, clip ? d_ref : nullptr, false,
                                      ContentOut{d_sa, d_sl, grad_adj, grad_label, loss, item_loss, factor, norms, best}, cgrid, d_st, d, s);
    if (ok && (d_guided_adj || d_guided_node)) launch_content_apply(d_adj, d_node, d_sa, d_sl, flags, d_guided_adj, d_guided_node, Cl, d, s);
    if (ok && shift_adj) e = hipMemcpyAsync(shift_adj, d_sa, sizeof(float) * sa, hipMemcpyDeviceToDevice, s);
    if (ok && e == hipSuccess && shift_label) e = hipMemcpyAsync(shift_label, d_sl, sizeof(float) * sl, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(s);   // par and the caller's arrays are host sources of async copies: wait before they leave scope
    (void)hipFree(d_par); (void)hipFree(d_ref); (void)hipFree(d_tgt); (void)hipFree(d_sa); (void)hipFree(d_sl); (void)hipFree(d_st);
    if (e != hipSuccess || es != hipSuccess) { g_create_err = me + std::string(hipGetErrorString(e != hipSuccess ? e : es)); return DSG_ERR_HIP; }
    if (!ok) { g_create_err = std::string(me) + "shape refused"; return DSG_ERR_INVALID; }
    return DSG_OK;
}

int dsg_debug_box_guide(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                        const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_node,
                        const dsg_guide_cfg *guide, float coef, float *loss, float *grad, float *shift, float *factor, float *norms,
                        float *d_guided_node, void *stream) {
    std::string why;
    if (B < 1 || N < 1 || c_adj < 1) { g_create_err = "dsg_debug_box_guide: B, N and c_adj must be >= 1"; return DSG_ERR_INVALID; }
    if (!guide_cfg_ok(guide, N, c_node, /*need_weights=*/false, why)) { g_create_err = "dsg_debug_box_guide: " + why; return DSG_ERR_INVALID; }
    if (!std::isfinite(coef)) { g_create_err = "dsg_debug_box_guide: coef is not finite"; return DSG_ERR_INVALID; }
    const bool clip = !std::isinf(guide->clip_ratio);
    if (!d_node || !flags || (clip && (!xhat_adj || !xhat_node || !d_adj))) { g_create_err = "dsg_debug_box_guide: null argument (d_node, flags; with a clip also xhat_adj, xhat_node, d_adj)"; return DSG_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const Dims d{B, N, c_adj, c_node};
    const GuideParams par{guide->w_overlap, guide->w_region, guide->w_align, guide->tau, clip ? guide->clip_ratio : 0.f, 0,
                          guide->sel, guide->region, nullptr, nullptr, mask_node};
    GuideParams *d_par = nullptr; double *d_ref = nullptr; float *d_shift = nullptr;
    hipError_t e = hipMalloc((void **)&d_par, sizeof(GuideParams));
    if (e == hipSuccess) e = hipMalloc((void **)&d_ref, sizeof(double) * (size_t)B);
    if (e == hipSuccess) e = hipMalloc((void **)&d_shift, sizeof(float) * (size_t)B * N * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_par, &par, sizeof(GuideParams), hipMemcpyHostToDevice, s);
    bool ok = e == hipSuccess;
    if (ok && clip) ok = launch_graph_diff_norm(CStatePtrs{xhat_adj, xhat_node}, CStatePtrs{d_adj, d_node}, flags, d_ref, d, s);
    if (ok) ok = launch_box_guide(d_par, nullptr, nullptr, coef, d_node, flags, clip ? d_ref : nullptr, false, BoxGuideOut{d_shift, grad, loss, factor, norms}, d, s);
    if (ok && d_guided_node) launch_box_apply(d_node, d_shift, flags, d_guided_node, d, s);
    if (ok && shift) e = hipMemcpyAsync(shift, d_shift, sizeof(float) * (size_t)B * N * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(s);   // par is a host source of an async copy: wait before it leaves scope
    (void)hipFree(d_par); (void)hipFree(d_ref); (void)hipFree(d_shift);
    if (e != hipSuccess || es != hipSuccess) { g_create_err = std::string("dsg_debug_box_guide: ") + hipGetErrorString(e != hipSuccess ? e : es); return DSG_ERR_HIP; }
    if (!ok) { g_create_err = "dsg_debug_box_guide: shape refused"; return DSG_ERR_INVALID; }
    return DSG_OK;
}

int dsg_debug_box_guide_rel(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *xhat_adj, const float *xhat_node,
                            const float *d_adj, const float *d_node, const uint8_t *flags, const uint8_t *mask_node,
                            const dsg_guide_cfg *guide, float coef, float *loss, float *grad, float *shift, float *factor, float *norms,
                            float *d_guided_node, void *stream, const dsg_rel_cfg *rel, uint8_t *kinds_out) {
    std::string why;
    const char *me = "dsg_debug_box_guide_rel: ";
    if (B < 1 || N < 1 || c_adj < 1) { g_create_err = std::string(me) + "B, N and c_adj must be >= 1"; return DSG_ERR_INVALID; }
    if (!guide_cfg_ok(guide, N, c_node, /*need_weights=*/false, why)) { g_create_err = me + why; return DSG_ERR_INVALID; }
    if (rel && !rel_cfg_ok(rel, c_adj, why)) { g_create_err = me + why; return DSG_ERR_INVALID; }
    if (!std::isfinite(coef)) { g_create_err = std::string(me) + "coef is not finite"; return DSG_ERR_INVALID; }
    const bool clip = !std::isinf(guide->clip_ratio);
    GuideParams par{guide->w_overlap, guide->w_region, guide->w_align, guide->tau, clip ? guide->clip_ratio : 0.f, 0,
                    guide->sel, guide->region, nullptr, nullptr, mask_node};
    const int src = rel_params(rel, par);
    if (!d_node || !flags || (clip && (!xhat_adj || !xhat_node || !d_adj))) { g_create_err = std::string(me) + "null argument (d_node, flags; with a clip also xhat_adj, xhat_node, d_adj)"; return DSG_ERR_INVALID; }
    if (src == REL_DECODED && !d_adj) { g_create_err = std::string(me) + "d_adj is NULL: the decoded source reads the adjacency estimate"; return DSG_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const Dims d{B, N, c_adj, c_node};
    GuideParams *d_par = nullptr; double *d_ref = nullptr; float *d_shift = nullptr; uint8_t *d_tab = nullptr;
    hipError_t e = hipMalloc((void **)&d_par, sizeof(GuideParams));
    if (e == hipSuccess) e = hipMalloc((void **)&d_ref, sizeof(double) * (size_t)B);
    if (e == hipSuccess) e = hipMalloc((void **)&d_shift, sizeof(float) * (size_t)B * N * 4);
    if (src == REL_GIVEN) par.kinds = rel->kinds;
    if (src == REL_DECODED) {
        if (e == hipSuccess) e = hipMalloc((void **)&d_tab, (size_t)rel->n_adj_type);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tab, rel->pred_kind, (size_t)rel->n_adj_type, hipMemcpyHostToDevice, s);
        par.pred_kind = d_tab;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_par, &par, sizeof(GuideParams), hipMemcpyHostToDevice, s);
    bool ok = e == hipSuccess;
    if (ok && clip) ok = launch_graph_diff_norm(CStatePtrs{xhat_adj, xhat_node}, CStatePtrs{d_adj, d_node}, flags, d_ref, d, s);
    const BoxGuideOut out{d_shift, grad, loss, factor, norms};
    if (ok && src != REL_NONE)
        ok = launch_box_guide_rel(d_par, nullptr, nullptr, coef, d_adj, d_node, flags, clip ? d_ref : nullptr, false, out, kinds_out, src == REL_DECODED, d, s);
    else if (ok) {
        ok = launch_box_guide(d_par, nullptr, nullptr, coef, d_node, flags, clip ? d_ref : nullptr, false, out, d, s);
        if (ok && kinds_out) e = hipMemsetAsync(kinds_out, 0, (size_t)B * N * N, s);
    }
    if (ok && d_guided_node) launch_box_apply(d_node, d_shift, flags, d_guided_node, d, s);
    if (ok && e == hipSuccess && shift) e = hipMemcpyAsync(shift, d_shift, sizeof(float) * (size_t)B * N * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(s);   // par and the table are host sources of async copies: wait before they leave scope
    (void)hipFree(d_par); (void)hipFree(d_ref); (void)hipFree(d_shift); (void)hipFree(d_tab);
    if (e != hipSuccess || es != hipSuccess) { g_create_err = me + std::string(hipGetErrorString(e != hipSuccess ? e : es)); return DSG_ERR_HIP; }
    if (!ok) { g_create_err = std::string(me) + "shape refused"; return DSG_ERR_INVALID; }
    return DSG_OK;
}

int dsg_profile_forward(dsg_handle h, int32_t B, int32_t n_iters, double *ms_by_kind, int64_t *launches_by_kind,
                        double *flops_by_kind, double *gemm_inkernel_ms_out, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!ms_by_kind || !launches_by_kind || !flops_by_kind || n_iters < 1) return fail(h, DSG_ERR_INVALID, "null argument");
    auto it = h->ws.find(B);
    if (it == h->ws.end()) return fail(h, DSG_ERR_STATE, "no workspace for batch %d: run dsg_denoise/dsg_sample first", B);
    hipStream_t s = (hipStream_t)stream;
    Workspace *w = it->second.get();
    for (int k = 0; k < PK_COUNT; k++) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; flops_by_kind[k] = 0.0; }
    if (!h->prof_gemm) {
        h->prof_gemm_cap = 512;
        if (int rc = owned_alloc(h, h->allocs, (void **)&h->prof_gemm, sizeof(unsigned long long) * 4 * h->prof_gemm_cap, AC_STATE)) return rc;
    }
    std::vector<unsigned long long> stamps(4 * h->prof_gemm_cap);   // per launch: {min start, max end, block-0 shader cycles, block-0 ticks}
    std::vector<double> clocks;
    double gemm_inkernel_ms = 0.0;
    // pass A: in-kernel stamps only -- the launches run back to back exactly as in the sampler loop
    for (int iter = 0; iter < n_iters; iter++) {
        for (int i = 0; i < h->prof_gemm_cap; i++) { stamps[4 * i] = ~0ull; stamps[4 * i + 1] = 0ull; stamps[4 * i + 2] = 0ull; stamps[4 * i + 3] = 0ull; }
        HIP_TRY(h, hipMemcpyAsync(h->prof_gemm, stamps.data(), sizeof(unsigned long long) * stamps.size(), hipMemcpyHostToDevice, s));
        h->prof_gemm_used = 0;
        h->prof_stamps = true;
        forward_fixed(h, w, s);
        h->prof_stamps = false;
        HIP_TRY(h, hipStreamSynchronize(s));
        if (int rc = plan_status(h, w)) return rc;   // (lists staged under other options: run the entry point again first)
        HIP_TRY(h, hipMemcpy(stamps.data(), h->prof_gemm, sizeof(unsigned long long) * stamps.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < h->prof_gemm_used; i++) {
            if (stamps[4 * i + 1] > stamps[4 * i]) gemm_inkernel_ms += (double)(stamps[4 * i + 1] - stamps[4 * i]) * 1e-5;  // 100 MHz ticks
            if (stamps[4 * i + 3] > 200) clocks.push_back((double)stamps[4 * i + 2] / (double)stamps[4 * i + 3] * 0.1);   // GHz, blocks > 2 us
            if (iter == n_iters - 1 && getenv("DSG_PROFILE_VERBOSE") && stamps[4 * i + 3] > 0)
                fprintf(stderr, "[dsg-clock] gemm launch %2d: block 0 held %.3f GHz over %.1f us\n", i,
                        (double)stamps[4 * i + 2] / (double)stamps[4 * i + 3] * 0.1, (double)stamps[4 * i + 3] * 0.01);
        }
    }
    std::sort(clocks.begin(), clocks.end());
    h->prof_clock_ghz = clocks.empty() ? 0.0 : clocks[clocks.size() / 2];
    // pass B: HIP-event brackets around every launch (per-class breakdown; each bracket includes dispatch latency)
    for (int iter = 0; iter < n_iters; iter++) {
        h->prof_on = true; h->prof_used = 0; h->prof_kind.clear(); h->prof_flops.clear(); h->prof_tag.clear(); h->prof_list.clear(); h->prof_thin_n.clear(); h->prof_qk.clear(); h->prof_form.clear();
        forward_fixed(h, w, s);
        const bool ok = h->prof_on;
        h->prof_on = false;
        HIP_TRY(h, hipStreamSynchronize(s));
        if (!ok) return fail(h, DSG_ERR_HIP, "hipEventCreate failed");
        // a pruned launch ran only its need list's share of the rows: its FLOP figure is what was executed, not the full shape
        std::vector<int> need_cnt(w->need.n_lists > 0 ? w->need.n_lists : 1, 0);
        if (w->need_lists) HIP_TRY(h, hipMemcpy(need_cnt.data(), w->need_cnt, sizeof(int) * w->need.n_lists, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h->prof_kind.size(); i++) {
            const int nl = h->prof_list[i];
            if (nl >= 0 && nl < w->need.n_lists) h->prof_flops[i] *= (double)need_cnt[nl] / ((double)B * (double)prune_plan(h).items[nl]);
            {   // the launches of the form that the "dedup_qkv" switch did not take returned at once
                const auto &qk = h->prof_qk[i];
                if (qk.list >= 0 && qk.list < w->need.n_lists && (qk_split_rule(need_cnt[qk.list], qk.M) ? 2 : 1) != qk.role) h->prof_flops[i] = 0.0;
            }
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, h->prof_events[2 * i], h->prof_events[2 * i + 1]));
            if (iter == n_iters - 1 && getenv("DSG_PROFILE_VERBOSE")) {
                // a list GEMM with a thin form names the form its blocks chose: the kernel's rule on the count read back above
                const char *form = h->prof_form[i] ? h->prof_form[i] : "";
                if (nl >= 0 && nl < w->need.n_lists && h->prof_thin_n[i] > 0)
                    form = gemm_thin_rule(need_cnt[nl], h->prof_thin_n[i], h->n_cu) ? " form=thin" : " form=wide";
                // a block with the "dedup_qkv" switch names the form its blocks chose (qk_split_rule on the count read back above)
                const auto &qk = h->prof_qk[i];
                if (qk.list >= 0 && qk.list < w->need.n_lists) form = qk_split_rule(need_cnt[qk.list], qk.M) ? " form=split" : " form=fused";
                fprintf(stderr, "[dsg-prof] %8.1f us %7.2f TF  %.60s%s\n", ms * 1e3, h->prof_flops[i] / (ms * 1e-3) / 1e12, h->prof_tag[i].c_str(), form);
            }
            ms_by_kind[h->prof_kind[i]] += ms;
            launches_by_kind[h->prof_kind[i]] += 1;
            flops_by_kind[h->prof_kind[i]] += h->prof_flops[i];
        }
    }
    if (gemm_inkernel_ms_out) *gemm_inkernel_ms_out = gemm_inkernel_ms;
    return DSG_OK;
}

int dsg_debug_need_lists(dsg_handle h, int32_t B, int32_t *roles, int32_t max_roles, int32_t *n_roles, int32_t *lists_out,
                         int64_t lists_cap, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!n_roles) return fail(h, DSG_ERR_INVALID, "null argument");
    auto it = h->ws.find(B);
    if (it == h->ws.end()) return fail(h, DSG_ERR_STATE, "no workspace for batch %d: run dsg_denoise/dsg_sample first", B);
    Workspace *w = it->second.get();
    const PrunePlan &pp = prune_plan(h);
    *n_roles = w->need_lists ? (int32_t)pp.roles.size() : 0;
    if (!w->need_lists || !roles) return DSG_OK;
    if (max_roles < *n_roles) return fail(h, DSG_ERR_INVALID, "room for %d roles needed", *n_roles);
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> all(w->need_ints);
    HIP_TRY(h, hipMemcpy(all.data(), w->need_lists, sizeof(int) * w->need_ints, hipMemcpyDeviceToHost));
    const int *cnt = all.data() + (w->need_cnt - w->need_lists);
    int64_t off = 0;
    for (size_t r = 0; r < pp.roles.size(); r++) {
        const PruneRole &ro = pp.roles[r];
        const int n = cnt[ro.list];
        int32_t *row = roles + 8 * r;
        row[0] = ro.kind; row[1] = ro.res; row[2] = ro.shift; row[3] = ro.stage; row[4] = ro.block; row[5] = n; row[6] = (int32_t)off;
        row[7] = B * pp.items[ro.list];
        if (lists_out) {
            if (off + n > lists_cap) return fail(h, DSG_ERR_INVALID, "lists_out too small");
            memcpy(lists_out + off, all.data() + w->need.list_off[ro.list], sizeof(int) * (size_t)n);
        }
        off += n;
    }
    return DSG_OK;
}

}  // extern "C"

namespace {

// launch_side: the device lists as they are -- what the launches and the fill iterate; counts[3] = the DedupMode they were written for.
// Otherwise the unique windows and the fills by meaning: under DD_TABLE the window the table stands for (rep) is listed with the unique
// windows and runs, where DD_BATCH computes it, and not with the fills
int dedup_level_lists(dsg_handle h, int32_t B, int32_t level, bool launch_side, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy,
                      int32_t *rep, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!counts || level < 0) return fail(h, DSG_ERR_INVALID, "null argument or negative level");
    auto it = h->ws.find(B);
    if (it == h->ws.end()) return fail(h, DSG_ERR_STATE, "no workspace for batch %d: run dsg_denoise/dsg_sample first", B);
    Workspace *w = it->second.get();
    counts[0] = counts[1] = counts[2] = -1;
    counts[3] = level <= NEED_MAX_DD_UP ? w->dd_fwd[level] : -1;
    if (!w->dd_rep || level >= w->need.dd_n) return DSG_OK;
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> all(w->need_ints);
    HIP_TRY(h, hipMemcpy(all.data(), w->need_lists, sizeof(int) * w->need_ints, hipMemcpyDeviceToHost));
    const int *cnt = all.data() + (w->need_cnt - w->need_lists);
    const int ids[3] = {w->need.dd_wins[level], w->need.dd_runs[level], w->need.dd_copy[level]};
    int32_t *dst[3] = {wins, runs, copy};
    for (int k = 0; k < 3; k++) {
        counts[k] = cnt[ids[k]];
        if (dst[k]) memcpy(dst[k], all.data() + w->need.list_off[ids[k]], sizeof(int) * (size_t)counts[k]);
    }
    const int *reps = all.data() + (w->dd_rep - w->need_lists);
    const int mode = reps[(size_t)w->need.dd_n * B], r = reps[(size_t)level * B];
    if (rep) memcpy(rep, reps + (size_t)level * B, sizeof(int) * (size_t)B);
    if (launch_side) { counts[3] = mode; return DSG_OK; }
    if (mode == DD_TABLE && r >= 0) {
        const int res = h->N >> level, nwr = res / 8, nW = nwr * nwr, b = r / nW, v = r - b * nW;
        if (wins) wins[counts[0]] = r;
        counts[0] += 1;
        for (int p = 0; p < 8; p++)
            if (runs) runs[counts[1] + p] = b * res * nwr + ((v / nwr) * 8 + p) * nwr + v % nwr;
        counts[1] += 8;
        const int *cl = all.data() + w->need.list_off[ids[2]];
        int n = 0;
        for (int k = 0; k < counts[2]; k++)
            if (cl[k] != r) { if (copy) copy[n] = cl[k]; n++; }
        counts[2] = n;
    }
    return DSG_OK;
}

}  // namespace

extern "C" {

int dsg_debug_dedup_level_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy,
                                int32_t *rep, void *stream) {
    return dedup_level_lists(h, B, level, false, counts, wins, runs, copy, rep, stream);
}

int dsg_debug_dedup_launch_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy,
                                 void *stream) {
    return dedup_level_lists(h, B, level, true, counts, wins, runs, copy, nullptr, stream);
}

int dsg_debug_dedup_qkv_lists(dsg_handle h, int32_t B, int32_t level, int32_t *counts, int32_t *runs, int32_t *src, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!counts || level < 0) return fail(h, DSG_ERR_INVALID, "null argument or negative level");
    auto it = h->ws.find(B);
    if (it == h->ws.end()) return fail(h, DSG_ERR_STATE, "no workspace for batch %d: run dsg_denoise/dsg_sample first", B);
    Workspace *w = it->second.get();
    counts[0] = counts[1] = counts[2] = counts[3] = -1;
    if (!w->dd_rep || level >= w->need.dd_n || w->need.qk_runs[level] < 0 || w->need.qk_src[level] < 0) return DSG_OK;
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> all(w->need_ints);
    HIP_TRY(h, hipMemcpy(all.data(), w->need_lists, sizeof(int) * w->need_ints, hipMemcpyDeviceToHost));
    const int *cnt = all.data() + (w->need_cnt - w->need_lists);
    const int res = h->N >> level;
    counts[0] = cnt[w->need.qk_runs[level]];
    counts[1] = cnt[w->need.qk_src[level]];
    counts[2] = qk_split_rule(counts[0], B * res * res) ? 1 : 0;
    counts[3] = w->qk_fwd[level] ? (qk_split_rule(counts[0], qk_rule_rows(h, B * res * res)) ? 1 : 0) : -1;
    if (runs) memcpy(runs, all.data() + w->need.list_off[w->need.qk_runs[level]], sizeof(int) * (size_t)counts[0]);
    if (src) memcpy(src, all.data() + w->need.list_off[w->need.qk_src[level]], sizeof(int) * (size_t)counts[1]);
    return DSG_OK;
}

int dsg_debug_readout_tiles(dsg_handle h, int32_t B, int32_t *counts, int32_t *tiles, void *stream) {
    if (int rc = check_ready(h, B)) return rc;
    if (!counts) return fail(h, DSG_ERR_INVALID, "null argument");
    auto it = h->ws.find(B);
    if (it == h->ws.end()) return fail(h, DSG_ERR_STATE, "no workspace for batch %d: run dsg_denoise/dsg_sample first", B);
    Workspace *w = it->second.get();
    counts[0] = counts[1] = -1;
    if (!w->need_lists || w->need.ro_tiles < 0) return DSG_OK;
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> all(w->need_ints);
    HIP_TRY(h, hipMemcpy(all.data(), w->need_lists, sizeof(int) * w->need_ints, hipMemcpyDeviceToHost));
    counts[0] = all[(w->need_cnt - w->need_lists) + w->need.ro_tiles];
    counts[1] = w->ro_fwd;
    if (tiles) memcpy(tiles, all.data() + w->need.list_off[w->need.ro_tiles], sizeof(int) * (size_t)counts[0]);
    return DSG_OK;
}

int dsg_debug_patch_forms(dsg_handle h, int32_t B, int32_t forms[2]) {
    if (!h || !forms) return DSG_ERR_INVALID;
    auto it = h->ws.find(B);
    forms[0] = it == h->ws.end() ? -1 : it->second->patch_fwd[0];
    forms[1] = it == h->ws.end() ? -1 : it->second->patch_fwd[1];
    return DSG_OK;
}

int dsg_debug_dedup_lists(dsg_handle h, int32_t B, int32_t *counts, int32_t *wins, int32_t *runs, int32_t *copy, int32_t *rep, void *stream) {
    return dsg_debug_dedup_level_lists(h, B, 0, counts, wins, runs, copy, rep, stream);
}

int32_t dsg_affine_width(dsg_handle h) { return (h && h->finalized) ? h->aff_n : 0; }

int dsg_noise_embed(dsg_handle h, int32_t rows, const float *c_noise, float *out_pe, float *out_emb, float *out_aff, void *stream) {
    if (!h || !h->finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (rows < 1 || !c_noise) return fail(h, DSG_ERR_INVALID, "rows / c_noise");
    hipStream_t s = (hipStream_t)stream;
    float *tmp = nullptr;   // pe | emb0 | emb | aff
    const size_t n_pe = (size_t)rows * h->E, n_e = (size_t)rows * NOISE_EMB, n_a = (size_t)rows * h->aff_n;
    if (int rc = owned_alloc(h, h->allocs, (void **)&tmp, sizeof(float) * (n_pe + 2 * n_e + n_a), AC_SCRATCH)) return rc;   // this call's own
    float *pe = tmp, *emb0 = pe + n_pe, *emb = emb0 + n_e, *aff = emb + n_e;
    embed_rows(h, c_noise, rows, pe, emb0, emb, aff, s);
    hipError_t e = hipSuccess;
    if (out_pe) e = hipMemcpyAsync(out_pe, pe, sizeof(float) * n_pe, hipMemcpyDeviceToDevice, s);
    if (out_emb && e == hipSuccess) e = hipMemcpyAsync(out_emb, emb, sizeof(float) * n_e, hipMemcpyDeviceToDevice, s);
    if (out_aff && e == hipSuccess) e = hipMemcpyAsync(out_aff, aff, sizeof(float) * n_a, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    owned_free(h->allocs, tmp);
    HIP_TRY(h, e);
    return DSG_OK;
}

int dsg_train_inputs(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *clean_adj, const float *clean_node,
                     const uint8_t *flags, const float *rnd_sigma, const float *eps_adj, const float *eps_node, uint64_t seed,
                     float *out_sigmas, float *out_weights, float *out_noisy_adj, float *out_noisy_node, void *stream) {
    if (B < 1 || N < 1 || c_adj < 1 || c_node < 1 || !clean_adj || !clean_node || !flags || !out_sigmas || !out_weights ||
        !out_noisy_adj || !out_noisy_node || ((eps_adj == nullptr) != (eps_node == nullptr)))
        return DSG_ERR_INVALID;
    launch_train_inputs(CStatePtrs{clean_adj, clean_node}, rnd_sigma, CStatePtrs{eps_adj, eps_node}, seed, flags, out_sigmas, out_weights,
                        StatePtrs{out_noisy_adj, out_noisy_node}, Dims{B, N, c_adj, c_node}, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DSG_OK : DSG_ERR_HIP;
}

int dsg_rainbow_loss(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *pred_adj, const float *pred_node,
                     const float *target_adj, const float *target_node, const uint8_t *flags, const float *loss_weight,
                     float edge_loss_weight, float node_loss_weight, float iou_loss_weight, int32_t iou_loss_type, float *out_loss_adj,
                     float *out_loss_node, void *stream) {
    if (B < 1 || N < 1 || c_adj < 1 || c_node < 1 || !pred_adj || !pred_node || !target_adj || !target_node || !flags || !out_loss_adj ||
        !out_loss_node || (iou_loss_weight != 0.f && c_node < 4) || iou_loss_type < DSG_IOU_IOU || iou_loss_type > DSG_IOU_CIOU)
        return DSG_ERR_INVALID;
    launch_rainbow_loss(CStatePtrs{pred_adj, pred_node}, CStatePtrs{target_adj, target_node}, flags, loss_weight, edge_loss_weight,
                        node_loss_weight, iou_loss_weight, iou_loss_type, out_loss_adj, out_loss_node, Dims{B, N, c_adj, c_node},
                        (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DSG_OK : DSG_ERR_HIP;
}

int dsg_rainbow_loss_backward(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *pred_adj, const float *pred_node,
                              const float *target_adj, const float *target_node, const uint8_t *flags, const float *loss_weight,
                              float edge_loss_weight, float node_loss_weight, float iou_loss_weight, int32_t iou_loss_type,
                              const float *sigmas, float *out_grad_adj, float *out_grad_node, float *out_grad_F_adj, float *out_grad_F_node,
                              void *stream) {
    if (B < 1 || N < 1 || c_adj < 1 || c_node < 1 || !pred_adj || !pred_node || !target_adj || !target_node || !flags || !out_grad_adj ||
        !out_grad_node || (iou_loss_weight != 0.f && c_node < 4) || ((out_grad_F_adj || out_grad_F_node) && !sigmas) ||
        iou_loss_type < DSG_IOU_IOU || iou_loss_type > DSG_IOU_CIOU)
        return DSG_ERR_INVALID;
    launch_rainbow_loss_backward(CStatePtrs{pred_adj, pred_node}, CStatePtrs{target_adj, target_node}, flags, loss_weight,
                                 edge_loss_weight, node_loss_weight, iou_loss_weight, iou_loss_type, sigmas, StatePtrs{out_grad_adj, out_grad_node},
                                 StatePtrs{out_grad_F_adj, out_grad_F_node}, Dims{B, N, c_adj, c_node}, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? DSG_OK : DSG_ERR_HIP;
}

}  // extern "C"

// ---- training form: what one block and the whole network share ----
namespace {
// the training form (weight and input gradients, the ODE encoder) at patch_size > 1 is handle state, off by default
// (dsg_train_enable_patch), and runs fp32 products only: refused before any other check and before anything is enqueued
static int patch_training_gate(dsg_handle h, const char *entry) {
    if (h->P == 1) return DSG_OK;
    if (!h->train_patch)
        return fail(h, DSG_ERR_INVALID, "%s: the training form is not built at patch_size %d (patch_size > 1 covers the sampling entries only) "
                    "until dsg_train_enable_patch(h, 1) switches it on", entry, h->P);
    if (h->train_precision == DSG_TRAIN_BF16)
        return fail(h, DSG_ERR_INVALID, "%s: the training form at patch_size %d (dsg_train_enable_patch) runs fp32 products only: "
                    "dsg_train_set_precision(h, DSG_TRAIN_BF16) is not built there", entry, h->P);
    return DSG_OK;
}

struct TArena {   // bump allocator over one device buffer; without a base it only sizes (every get returns null)
    float *base = nullptr; size_t off = 0;
    float *get(size_t n) { n = (n + 63) / 64 * 64; float *p = base ? base + off : nullptr; off += n; return p; }
};
}  // namespace

// a handle-owned device buffer of at least `need` floats (grown after draining the stream that may still read the old one)
static float *train_buf(dsg_handle h, DevBuf &b, size_t need, hipStream_t s) {
    if (need > b.cap) {
        if (b.p) { (void)hipStreamSynchronize(s); owned_free(h->allocs, b.p); }
        b = DevBuf{};
        if (owned_alloc(h, h->allocs, (void **)&b.p, sizeof(float) * need, AC_SCRATCH) != 0) { b.p = nullptr; return nullptr; }
        b.cap = need;
    }
    return b.p;
}

// `carve` hands out a buffer's regions; it runs twice, over no memory to get the size and then over the grown buffer, so that the size
// and the layout cannot disagree.  false: out of memory
template <class Carve> static bool train_carve(dsg_handle h, DevBuf &b, hipStream_t s, Carve carve) {
    TArena A;
    carve(A);
    if (!train_buf(h, b, A.off, s)) return false;
    A = TArena{b.p, 0};
    carve(A);
    return true;
}

// the 15 parameter tensors of a SwinTransformerBlock: state-dict names below the block's prefix and their slots in a.W / a.G
static const char *const kBlockParamNames[15] = {"affine.weight", "affine.bias", "norm1.weight", "norm1.bias", "attn.relative_position_bias_table",
                                                 "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                                                 "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"};
static float *TrainBlockParams::*const kBlockParamSlots[15] = {
    &TrainBlockParams::aff_w, &TrainBlockParams::aff_b, &TrainBlockParams::n1_w, &TrainBlockParams::n1_b, &TrainBlockParams::rpb,
    &TrainBlockParams::qkv_w, &TrainBlockParams::qkv_b, &TrainBlockParams::proj_w, &TrainBlockParams::proj_b, &TrainBlockParams::n2_w,
    &TrainBlockParams::n2_b, &TrainBlockParams::fc1_w, &TrainBlockParams::fc1_b, &TrainBlockParams::fc2_w, &TrainBlockParams::fc2_b};

// geometry of block `b` at batch B, and its parameters / gradient buffers as weight(name) / grad(name) resolve them
template <class FW, class FG> static void bind_block(TrainBlockArgs &a, const BlockPlan &b, int B, int mlp_ratio, FW weight, FG grad) {
    a.B = B; a.res = b.res; a.ws = b.ws; a.shift = b.shift; a.heads = b.heads; a.C = b.C; a.hidden = mlp_ratio * b.C;
    for (int i = 0; i < 15; i++) { a.W.*kBlockParamSlots[i] = weight(kBlockParamNames[i]); a.G.*kBlockParamSlots[i] = grad(kBlockParamNames[i]); }
}

// the tensors a block's forward saves for its backward
static void carve_block_saved(TArena &A, TrainBlockArgs &a) {
    const size_t M = (size_t)a.B * a.res * a.res, C = a.C, H = a.hidden;
    a.aff = A.get((size_t)a.B * 2 * C); a.d_aff = A.get((size_t)a.B * 2 * C);
    a.x_mod = A.get(M * C); a.xn1 = A.get(M * C); a.att = A.get(M * C); a.x1 = A.get(M * C); a.xn2 = A.get(M * C);
    a.stats1 = A.get(M * 2); a.stats2 = A.get(M * 2); a.qkv = A.get(M * 3 * C); a.pre = A.get(M * H); a.hid = A.get(M * H);
}

extern "C" int dsg_block_train(dsg_handle h, const char *block, int32_t B, const float *x_in, const float *emb, const float *grad_out, float *x_out,
                    float *grad_in, float *grad_emb, int32_t n_params, const char *const *names, float *const *grad_params, void *stream) {
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (!block || B < 1 || !x_in || !emb || !x_out) return fail(h, DSG_ERR_INVALID, "null argument");
    const BlockPlan *bp = nullptr;
    for (int l = 0; l < h->L; l++)
        for (auto *vec : {&h->down[l], &h->up[l]})
            for (auto &b : *vec) if (b.prefix == block) bp = &b;
    if (!bp) return fail(h, DSG_ERR_INVALID, "no block '%s'", block);
    const bool bwd_args = grad_in && grad_emb && names && grad_params;
    const char *no_weight = nullptr, *no_grad = nullptr;
    TrainBlockArgs a{};
    auto weight = [&](const char *name) -> float * {
        auto it = h->w.find(bp->prefix + "." + name); if (it == h->w.end()) { if (!no_weight) no_weight = name; return nullptr; } return it->second.p; };
    auto grad = [&](const char *name) -> float * {
        float *dst = nullptr;
        if (grad_out && bwd_args) for (int k = 0; k < n_params; k++) if (names[k] && !strcmp(names[k], name)) dst = grad_params[k];
        if (!dst && !no_grad) no_grad = name;
        return dst;
    };
    bind_block(a, *bp, B, h->cfg.mlp_ratio, weight, grad);
    if (no_weight) return fail(h, DSG_ERR_STATE, "weight '%s.%s' is not loaded", block, no_weight);
    if (grad_out && !bwd_args) return fail(h, DSG_ERR_INVALID, "backward needs grad_in, grad_emb and the parameter gradient buffers");
    if (grad_out && no_grad) return fail(h, DSG_ERR_INVALID, "no gradient buffer for '%s'", no_grad);
    a.x_in = x_in; a.emb = emb; a.grad_out = grad_out; a.x_out = x_out; a.grad_in = grad_in; a.grad_emb = grad_emb;
    DevBuf scratch;   // this call's own: the saved tensors and the backward's scratch, freed below
    const bool fits = train_carve(h, scratch, (hipStream_t)stream, [&](TArena &A) {
        const size_t M = (size_t)B * a.res * a.res, C = a.C, H = a.hidden;
        carve_block_saved(A, a);
        a.d_x1 = A.get(M * C); a.t_mc = A.get(M * C); a.t_mc2 = A.get(M * C); a.t_m3c = A.get(M * 3 * C); a.t_mh = A.get(M * H);
    });
    if (!fits) return fail(h, DSG_ERR_HIP, "out of memory");
    const bool ok = train_block(a, (hipStream_t)stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    owned_free(h->allocs, scratch.p);
    HIP_TRY(h, e);
    if (t_scratch_failed((hipStream_t)stream, true)) return fail(h, DSG_ERR_HIP, "out of memory (training scratch of this stream)");
    if (!ok) return fail(h, DSG_ERR_HIP, "train_block failed (window larger than 128 tokens or a launch error)");
    return DSG_OK;
}

// ---- whole-network training step: forward in training form + backward to every parameter (correctness-first kernels) ----
// The entries below build a TrainNet (parameters bound, buffers carved: nothing enqueued), then run train_forward, their own launches
// on its outputs, and train_backward, all on the caller's stream.
namespace {
struct TrainLin { float *w, *b, *dw, *db; };   // a module's weight and bias and, when weight gradients are asked for, their gradient buffers
struct TrainBufs {   // saved activations outside the blocks
    float *pe, *m0, *s0, *m1, *emb, *d_emb, *pe_demb, *tok, *pe_lin, *pe_ln, *pe_stats, *pe_aff, *pe_daff, *x0;
    float *mcat[8], *mnrm[8], *mstats[8], *mout[8];                                          // PatchMerging per level
    float *ucat[8], *uy[8], *un[8], *ustats[8], *usc[8], *upn[8], *upstats[8], *uout[8];   // PatchBreakup per up layer
    float *fy, *fstats, *z1, *z2, *rep, *ha_pre, *ha, *oa, *pool, *hn_pre, *hn, *on;
    float *d_skip[8];
    float *pe_img, *pe_dimg, *ro_img, *ro_dimg, *ro_bias;   // patch_size > 1: the per-call weight images of PatchEmbed and read_out.0 and their gradients
};
struct TrainStage { TrainBlockArgs a; float *x_out, *d_emb; };
struct TrainNet {
    int B, N, E, L, Ca, Cn, Cin, self_condition;
    int P, R0, Kp;                    // patch_size, the level-0 token resolution N / P, and the width of PatchEmbed's input rows (P == 1: Cin)
    size_t M0;                        // B R0 R0: tokens of level 0
    size_t Mp;                        // B N N: pixel rows of the read-out chain, (token, a, b) order at P > 1 (P == 1: M0)
    std::vector<TrainStage> stages;   // the blocks in execution order: encoder level l is [first[l], first[l + 1]), up layer i starts at first[L + i]
    int first[2 * DSG_MAX_LAYERS + 1];
    bool grouped;                     // every `affine` linear of the network in one grouped launch (at most T_GROUP_MAX - 1 blocks)
    // the modules outside the blocks; mrg_*: PatchMerging after encoder level l, up_*: PatchBreakup before up layer i (no biases but the norms')
    TrainLin map0, map1, pe, pe_norm, pe_aff, norm, ro0, ro1, ro2, adj1, adj2, node1, node2;
    TrainLin mrg_norm[8], mrg_red[8], up_pre[8], up_norm[8], up_pn[8], up_post[8];
    TrainBufs Bf;
    int skip_res[8], skip_C[8];       // the tensor at the end of encoder level l (after its merging, if any): the decoder's skip input
    const int *has_sc;                // device 0 / 1: the "self-conditioning present" switch of launch_assemble
    const float *xL;                  // the last block's output, left by train_forward for train_backward
    float *t_mh, *t_m3c, *t_w, *t_mc, *t_mc2, *d_x, *d_y;   // backward scratch
    TrainLp *lp;                      // bf16 mode of the covered products (train_lp_begin); null: fp32 everywhere
};
struct TrainInputs { const float *adj, *node; const uint8_t *flags; const float *c_noise, *sc_adj, *sc_node; };
// input-gradient mode (dsg_precond_vjp): the backward carries dL/d(activation) only -- no dW / db product, no affine or noise-embedding
// backward, no parameter gradient buffer -- and ends in d_tok [B N N, ld] = d_pe_lin W_img, the gradient of the live columns of the
// assembled input (img [E][ld]: scratch for the weight image of t_live_cols; patch_size > 1: the p^2 groups of t_live_cols_patch)
struct TrainInputGrad { float *d_tok, *img; int ld; };
enum TrainBackward { TRAIN_WEIGHT_GRADS, TRAIN_INPUT_GRADS };
}  // namespace

// saved activations of the whole network (pointers only: no lookup, nothing rebuilt)
static void train_net_carve(TrainNet &net, TArena &A) {
    TrainBufs &Bf = net.Bf;
    const int B = net.B, N = net.N, E = net.E, L = net.L;
    const size_t M0 = net.M0, Mp = net.Mp;
    auto carve_stages = [&](int g) {
        for (int k = net.first[g]; k < net.first[g + 1]; k++) {
            TrainStage &st = net.stages[k];
            carve_block_saved(A, st.a);
            st.x_out = A.get((size_t)B * st.a.res * st.a.res * st.a.C); st.d_emb = A.get((size_t)B * NOISE_EMB);
        }
    };
    Bf.pe = A.get((size_t)B * E); Bf.m0 = A.get((size_t)B * NOISE_EMB); Bf.s0 = A.get((size_t)B * NOISE_EMB);
    Bf.m1 = A.get((size_t)B * NOISE_EMB); Bf.emb = A.get((size_t)B * NOISE_EMB); Bf.d_emb = A.get((size_t)B * NOISE_EMB);
    Bf.pe_demb = A.get((size_t)B * NOISE_EMB);
    Bf.tok = A.get(M0 * net.Kp); Bf.pe_lin = A.get(M0 * E); Bf.pe_ln = A.get(M0 * E); Bf.pe_stats = A.get(M0 * 2);
    Bf.pe_aff = A.get((size_t)B * 2 * E); Bf.pe_daff = A.get((size_t)B * 2 * E); Bf.x0 = A.get(M0 * E);
    int res = net.R0, C = E;
    for (int l = 0; l < L; l++) {
        carve_stages(l);
        if (l < L - 1) {
            const size_t M2 = (size_t)B * (res / 2) * (res / 2);
            Bf.mcat[l] = A.get(M2 * 4 * C); Bf.mnrm[l] = A.get(M2 * 4 * C); Bf.mstats[l] = A.get(M2 * 2); Bf.mout[l] = A.get(M2 * 2 * C);
            res /= 2; C *= 2;
        }
        net.skip_res[l] = res; net.skip_C[l] = C;
        Bf.d_skip[l] = A.get((size_t)B * res * res * C);
    }
    for (int i = 0; i < L; i++) {
        if (i > 0) {
            const size_t Mi = (size_t)B * res * res; const int D = 2 * C, Co = D / 4;
            Bf.ucat[i] = A.get(Mi * D); Bf.uy[i] = A.get(Mi * D); Bf.un[i] = A.get(Mi * D); Bf.ustats[i] = A.get(Mi * 2);
            Bf.usc[i] = A.get(Mi * 4 * Co); Bf.upn[i] = A.get(Mi * 4 * Co); Bf.upstats[i] = A.get(Mi * 4 * 2); Bf.uout[i] = A.get(Mi * 4 * Co);
            res *= 2; C /= 2;
        }
        carve_stages(L + i);
    }
    Bf.fy = A.get(M0 * E); Bf.fstats = A.get(M0 * 2); Bf.z1 = A.get(Mp * E); Bf.z2 = A.get(Mp * E); Bf.rep = A.get(Mp * E);
    Bf.ha_pre = A.get(Mp * E); Bf.ha = A.get(Mp * E); Bf.oa = A.get(Mp * net.Ca);
    Bf.pool = A.get((size_t)B * N * E); Bf.hn_pre = A.get((size_t)B * N * E); Bf.hn = A.get((size_t)B * N * E); Bf.on = A.get((size_t)B * N * net.Cn);
    Bf.pe_img = Bf.pe_dimg = Bf.ro_img = Bf.ro_dimg = Bf.ro_bias = nullptr;
    if (net.P > 1) {
        const size_t PP = (size_t)net.P * net.P;
        Bf.pe_img = A.get((size_t)E * net.Kp); Bf.pe_dimg = A.get((size_t)E * net.Kp);
        Bf.ro_img = A.get(PP * E * E); Bf.ro_dimg = A.get(PP * E * E); Bf.ro_bias = A.get(PP * E);
    }
}

// Validates, binds every parameter (and, with `weight_grads`, every gradient buffer of names / grad_params) once, and carves the
// handle's arena and backward scratch for batch B.  Nothing is enqueued; a buffer that has to grow is freed after `s` has drained.
static int train_net_build(dsg_handle h, TrainNet &net, int32_t B, const float *sc_adj, const float *sc_node, bool weight_grads,
                           int32_t n_params, const char *const *names, float *const *grad_params, hipStream_t s) {
    if (h->cfg.self_condition && ((sc_adj == nullptr) != (sc_node == nullptr))) return fail(h, DSG_ERR_INVALID, "self-conditioning needs both tensors or none");
    const int L = h->L;
    net.B = B; net.N = h->N; net.E = h->E; net.L = L; net.Ca = h->Ca; net.Cn = h->Cn; net.Cin = h->Cin;
    net.self_condition = h->cfg.self_condition; net.P = h->P; net.R0 = h->R0;
    net.Kp = h->P > 1 ? t_pe_image_width(h->Cin, h->P) : h->Cin;
    net.M0 = (size_t)B * h->R0 * h->R0; net.Mp = (size_t)B * h->N * h->N;
    if (!h->train_const) {
        const int zo[2] = {0, 1};
        if (int rc = owned_alloc(h, h->allocs, (void **)&h->train_const, sizeof(zo), AC_STATE)) return rc;
        HIP_TRY(h, hipMemcpy(h->train_const, zo, sizeof(zo), hipMemcpyHostToDevice));
    }
    net.has_sc = h->train_const + ((h->cfg.self_condition && sc_adj) ? 1 : 0);
    std::unordered_map<std::string, float *> gmap;
    if (weight_grads) for (int k = 0; k < n_params; k++) if (names[k] && grad_params[k]) gmap[names[k]] = grad_params[k];
    std::string missing;
    auto Wt = [&](const std::string &k) -> float * {
        if (!h->train_params.empty()) { auto bt = h->train_params.find(k); if (bt != h->train_params.end()) return const_cast<float *>(bt->second); }
        auto it = h->w.find(k); if (it == h->w.end()) { if (missing.empty()) missing = k; return nullptr; } return it->second.p; };
    auto Gd = [&](const std::string &k) -> float * { if (!weight_grads) return nullptr; auto it = gmap.find(k); if (it == gmap.end()) { if (missing.empty()) missing = "grad:" + k; return nullptr; } return it->second; };
    for (int g = 0; g < 2 * L; g++) {
        net.first[g] = (int)net.stages.size();
        for (const BlockPlan &b : g < L ? h->down[g] : h->up[g - L]) {
            net.stages.emplace_back();
            bind_block(net.stages.back().a, b, B, h->cfg.mlp_ratio, [&](const char *name) { return Wt(b.prefix + "." + name); },
                       [&](const char *name) { return Gd(b.prefix + "." + name); });
        }
    }
    net.first[2 * L] = (int)net.stages.size();
    net.grouped = (int)net.stages.size() + 1 <= T_GROUP_MAX;
    for (TrainStage &st : net.stages) st.a.aff_grouped = net.grouped;
    auto lin = [&](const std::string &p, bool bias = true) {
        return TrainLin{Wt(p + ".weight"), bias ? Wt(p + ".bias") : nullptr, Gd(p + ".weight"), bias ? Gd(p + ".bias") : nullptr}; };
    net.map0 = lin("map_layer0"); net.map1 = lin("map_layer1"); net.pe = lin("patch_embed.proj"); net.pe_norm = lin("patch_embed.norm");
    net.pe_aff = lin("patch_embed.affine"); net.norm = lin("norm"); net.ro0 = lin("read_out.0"); net.ro1 = lin("read_out.1");
    net.ro2 = lin("read_out.2"); net.adj1 = lin("readout_adj_mlp.fc1"); net.adj2 = lin("readout_adj_mlp.fc2");
    net.node1 = lin("readout_node_mlp.fc1"); net.node2 = lin("readout_node_mlp.fc2");
    for (int l = 0; l < L - 1; l++) {
        const std::string p = "down_layers." + std::to_string(l) + ".downsample.";
        net.mrg_norm[l] = lin(p + "norm"); net.mrg_red[l] = lin(p + "reduction", false);
    }
    for (int i = 1; i < L; i++) {
        const std::string p = "up_layers." + std::to_string(i) + ".upsample.";
        net.up_pre[i] = lin(p + "pre_linear", false); net.up_norm[i] = lin(p + "norm"); net.up_pn[i] = lin(p + "post_norm");
        net.up_post[i] = lin(p + "post_linear", false);
    }
    if (!missing.empty()) return fail(h, DSG_ERR_INVALID, "missing tensor '%s'", missing.c_str());
    // the saved-activation arena and the backward scratch belong to the handle and are kept between calls.  Scratch: three of the
    // widest tensors, level 0's [M0, 4E] (every level has M C constant up to the 2x of merging), and four of [M0, 2E]
    // (patch_size > 1: the read-out chain's [Mp, E] and [Mp, Ca] gradients pass through the same regions)
    const size_t wide = std::max(net.M0 * (size_t)(4 * net.E), net.P > 1 ? net.Mp * (size_t)std::max(net.E, net.Ca) : (size_t)0);
    const size_t two = std::max(net.M0 * (size_t)net.E * 2, net.P > 1 ? net.Mp * (size_t)net.E : (size_t)0);
    if (!train_carve(h, h->train_arena, s, [&](TArena &A) { train_net_carve(net, A); A.get(16); }) ||
        !train_carve(h, h->train_scr, s, [&](TArena &A) {
            net.t_mh = A.get(wide); net.t_m3c = A.get(wide); net.t_w = A.get(wide); net.t_mc = A.get(two); net.t_mc2 = A.get(two);
            net.d_x = A.get(two); net.d_y = A.get(two + 4096);
        }))
        return fail(h, DSG_ERR_HIP, "out of memory");
    return DSG_OK;
}

// y [M, out] = x [M, in] W^T + bias (W [out, in]); its backward: dW = dy^T x and db = colsum(dy) when `wg`, dx = dy W when dx is given
// lp: the call site is covered by the bf16 mode (downsample.reduction, upsample.pre_linear / post_linear; the blocks' four through a.lp)
static void lin_fwd(const float *x, const float *W, const float *bias, float *y, size_t M, int in, int out, hipStream_t s, TrainLp *lp = nullptr) {
    t_gemm(false, true, x, in, W, in, bias, y, out, (int)M, out, in, false, s, nullptr, nullptr, ACT_NONE, nullptr, nullptr, -1, lp);
}
static void lin_bwd(bool wg, const float *x, const float *W, const float *dy, float *dx, float *dW, float *db, size_t M, int in, int out,
                    hipStream_t s, TrainLp *lp = nullptr) {
    if (wg) t_gemm(true, false, dy, out, x, in, nullptr, dW, in, out, in, (int)M, false, s, db, nullptr, ACT_NONE, nullptr, nullptr, -1, lp);
    if (dx) t_gemm(false, false, dy, out, W, in, nullptr, dx, in, (int)M, in, out, false, s, nullptr, nullptr, ACT_NONE, nullptr, nullptr, -1, lp);
}

// bf16 mode of a training entry: carves the handle's plane buffer and enqueues the casts of every covered weight whose products the
// shape rule admits at this batch size -- W [out, in] for y = x W^T, W^T [in, out] for dx = dy W -- in grouped launches, and hands the
// planes to the covered call sites (net.lp, a.lp).  The parameters are read in place and may have changed since the last call, so
// nothing is kept between calls.  With the mode off nothing is enqueued and net.lp stays null.  false: out of memory
static bool train_lp_begin(dsg_handle h, TrainNet &net, TrainLp &lp, hipStream_t s) {
    h->train_counts.clear();
    if (h->train_precision != DSG_TRAIN_BF16) return true;
    struct Job { const float *w; int out, in; };
    std::vector<Job> jobs;
    auto add = [&](const float *w, size_t rows, int in, int out) { if (w && t_lp_rule(rows, in, out)) jobs.push_back(Job{w, out, in}); };
    for (const TrainStage &st : net.stages) {
        const TrainBlockArgs &a = st.a;
        const size_t M = (size_t)a.B * a.res * a.res;
        add(a.W.qkv_w, M, a.C, 3 * a.C); add(a.W.proj_w, M, a.C, a.C); add(a.W.fc1_w, M, a.C, a.hidden); add(a.W.fc2_w, M, a.hidden, a.C);
    }
    int res = net.R0, C = net.E;
    for (int l = 0; l < net.L - 1; l++) {   // merging after encoder level l: [M / 4, 4C] -> 2C
        res /= 2;
        add(net.mrg_red[l].w, (size_t)net.B * res * res, 4 * C, 2 * C);
        C *= 2;
    }
    for (int i = 1; i < net.L; i++) {       // breakup before up layer i: pre_linear [Mi, D] -> D at the coarse grid, post_linear [4 Mi, D / 4] at the fine one
        const size_t Mi = (size_t)net.B * res * res; const int D = 2 * C;
        add(net.up_pre[i].w, Mi, D, D); add(net.up_post[i].w, 4 * Mi, D / 4, D / 4);
        res *= 2; C /= 2;
    }
    std::vector<unsigned short *> at(jobs.size());
    const bool fits = jobs.empty() || train_carve(h, h->train_lp, s, [&](TArena &A) {   // (no job: every covered product stays fp32, and is counted)
        for (size_t k = 0; k < jobs.size(); k++) at[k] = reinterpret_cast<unsigned short *>(A.get((size_t)jobs[k].out * jobs[k].in));   // two bf16 planes in out * in floats
    });
    if (!fits) return false;
    TCastGroup g;
    for (size_t k = 0; k < jobs.size(); k++) {
        const size_t n = (size_t)jobs[k].out * jobs[k].in;
        if (lp.planes.count(jobs[k].w)) continue;   // (a tensor bound twice)
        lp.planes[jobs[k].w] = TLpPlane{at[k], at[k] + n};
        t_cast_lp_add(g, jobs[k].w, at[k], at[k] + n, jobs[k].out, jobs[k].in);
        if (g.n == T_CAST_MAX) { t_cast_lp(g, s); g = TCastGroup{}; }
    }
    t_cast_lp(g, s);
    net.lp = &lp;
    for (TrainStage &st : net.stages) st.a.lp = &lp;
    return true;
}
static void train_lp_end(dsg_handle h, const TrainLp &lp) { h->train_counts = lp.counts; }

// F = network(in) in training form, every activation the backward needs left in the arena; false: a block refused to launch
static bool train_forward(TrainNet &net, const TrainInputs &in, StatePtrs out_F, hipStream_t s) {
    const TrainBufs &Bf = net.Bf;
    const int B = net.B, N = net.N, E = net.E, L = net.L, Ca = net.Ca, Cn = net.Cn, Cin = net.Cin, P = net.P, PP = P * P, T0 = net.R0 * net.R0;
    const size_t M0 = net.M0, Mp = net.Mp;
    bool ok = true;
    launch_noise_pe(in.c_noise, Bf.pe, B, E, s);
    lin_fwd(Bf.pe, net.map0.w, net.map0.b, Bf.m0, B, E, NOISE_EMB, s);
    t_silu(Bf.m0, nullptr, Bf.s0, (size_t)B * NOISE_EMB, false, s);
    lin_fwd(Bf.s0, net.map1.w, net.map1.b, Bf.m1, B, NOISE_EMB, NOISE_EMB, s);
    t_silu(Bf.m1, nullptr, Bf.emb, (size_t)B * NOISE_EMB, false, s);
    if (P > 1) {   // the p^2 sub-pixels' channels side by side against the weight image of this call's raw weight: the strided convolution
        ok = launch_assemble_patch(in.adj, in.node, in.sc_adj, in.sc_node, net.has_sc, in.flags, Bf.tok, B, N, P, Ca, Cn, net.self_condition, net.Kp, s) &&
             t_pe_pack(net.pe.w, Bf.pe_img, E, Cin, P, net.Kp, s);
        lin_fwd(Bf.tok, Bf.pe_img, net.pe.b, Bf.pe_lin, M0, net.Kp, E, s);
    } else {
        launch_assemble(in.adj, in.node, in.sc_adj, in.sc_node, net.has_sc, in.flags, Bf.tok, B, N, Ca, Cn, net.self_condition, Cin, s);
        lin_fwd(Bf.tok, net.pe.w, net.pe.b, Bf.pe_lin, M0, Cin, E, s);
    }
    t_ln_fwd(Bf.pe_lin, net.pe_norm.w, net.pe_norm.b, Bf.pe_ln, Bf.pe_stats, (int)M0, E, s);
    if (net.grouped) {
        // every `affine` linear of the network (PatchEmbed + all blocks) hangs off emb: one grouped launch
        TGemmGroup gf;
        gf.p[gf.n++] = TGemmProb{Bf.emb, net.pe_aff.w, net.pe_aff.b, Bf.pe_aff, NOISE_EMB, NOISE_EMB, 2 * E, B, 2 * E, NOISE_EMB};
        for (const TrainStage &st : net.stages)
            gf.p[gf.n++] = TGemmProb{Bf.emb, st.a.W.aff_w, st.a.W.aff_b, st.a.aff, NOISE_EMB, NOISE_EMB, 2 * st.a.C, B, 2 * st.a.C, NOISE_EMB};
        t_gemm_grouped(false, true, false, gf, s);
    } else {   // more blocks than one group holds: PatchEmbed's here, each block's own in train_block
        lin_fwd(Bf.emb, net.pe_aff.w, net.pe_aff.b, Bf.pe_aff, B, NOISE_EMB, 2 * E, s);
    }
    t_modulate(Bf.pe_ln, Bf.pe_aff, nullptr, Bf.x0, nullptr, B, T0, E, false, s);
    const float *x = Bf.x0, *skip[8] = {};
    int res = net.R0, C = E;
    auto run_blocks = [&](int g) {
        for (int k = net.first[g]; k < net.first[g + 1]; k++) {
            TrainStage &st = net.stages[k];
            st.a.x_in = x; st.a.emb = Bf.emb; st.a.x_out = st.x_out; st.a.grad_out = nullptr;
            ok = ok && train_block(st.a, s);
            x = st.x_out;
        }
    };
    for (int l = 0; l < L; l++) {
        run_blocks(l);
        if (l < L - 1) {
            const size_t M2 = (size_t)B * (res / 2) * (res / 2);
            t_regroup(x, Bf.mcat[l], B, res, C, true, s);
            t_ln_fwd(Bf.mcat[l], net.mrg_norm[l].w, net.mrg_norm[l].b, Bf.mnrm[l], Bf.mstats[l], (int)M2, 4 * C, s);
            lin_fwd(Bf.mnrm[l], net.mrg_red[l].w, nullptr, Bf.mout[l], M2, 4 * C, 2 * C, s, net.lp);
            x = Bf.mout[l]; res /= 2; C *= 2;
        }
        skip[l] = x;
    }
    for (int i = 0; i < L; i++) {
        if (i > 0) {
            const size_t Mi = (size_t)B * res * res; const int D = 2 * C, Co = D / 4;
            t_concat(x, skip[L - 1 - i], Bf.ucat[i], Mi, C, s);
            lin_fwd(Bf.ucat[i], net.up_pre[i].w, nullptr, Bf.uy[i], Mi, D, D, s, net.lp);
            t_ln_fwd(Bf.uy[i], net.up_norm[i].w, net.up_norm[i].b, Bf.un[i], Bf.ustats[i], (int)Mi, D, s);
            t_regroup(Bf.un[i], Bf.usc[i], B, 2 * res, Co, false, s);   // scatter: fine [4 Mi, Co] <- coarse [Mi, 4 Co]
            t_ln_fwd(Bf.usc[i], net.up_pn[i].w, net.up_pn[i].b, Bf.upn[i], Bf.upstats[i], (int)(4 * Mi), Co, s);
            lin_fwd(Bf.upn[i], net.up_post[i].w, nullptr, Bf.uout[i], 4 * Mi, Co, Co, s, net.lp);
            x = Bf.uout[i]; res *= 2; C /= 2;
        }
        run_blocks(L + i);
    }
    net.xL = x;
    t_ln_fwd(x, net.norm.w, net.norm.b, Bf.fy, Bf.fstats, (int)M0, E, s);
    if (P > 1) {   // [M0, p^2 E] = fy img: read as [Mp, E] it is z1 with rows in (token, a, b) order
        ok = ok && t_ro0_pack(net.ro0.w, net.ro0.b, Bf.ro_img, Bf.ro_bias, E, E, P, s);
        t_gemm(false, false, Bf.fy, E, Bf.ro_img, PP * E, Bf.ro_bias, Bf.z1, PP * E, (int)M0, PP * E, E, false, s);
    } else t_gemm(false, false, Bf.fy, E, net.ro0.w, E, net.ro0.b, Bf.z1, E, (int)M0, E, E, false, s);   // ConvTranspose2d: [in, out]
    lin_fwd(Bf.z1, net.ro1.w, net.ro1.b, Bf.z2, Mp, E, E, s);
    lin_fwd(Bf.z2, net.ro2.w, net.ro2.b, Bf.rep, Mp, E, E, s);
    lin_fwd(Bf.rep, net.adj1.w, net.adj1.b, Bf.ha_pre, Mp, E, E, s);
    t_gelu(Bf.ha_pre, nullptr, Bf.ha, Mp * E, false, s);
    lin_fwd(Bf.ha, net.adj2.w, net.adj2.b, Bf.oa, Mp, E, Ca, s);
    if (P > 1) {
        ok = ok && t_adj_out_patch(Bf.oa, in.flags, out_F.adj, nullptr, nullptr, B, N, P, Ca, false, s) &&
             launch_pool_patch(Bf.rep, in.flags, Bf.pool, B, N, P, E, s);
    } else {
        t_adj_out(Bf.oa, in.flags, out_F.adj, nullptr, nullptr, B, N, Ca, false, s);
        launch_pool(Bf.rep, in.flags, Bf.pool, B, N, E, s);
    }
    lin_fwd(Bf.pool, net.node1.w, net.node1.b, Bf.hn_pre, (size_t)B * N, E, E, s);
    t_gelu(Bf.hn_pre, nullptr, Bf.hn, (size_t)B * N * E, false, s);
    lin_fwd(Bf.hn, net.node2.w, net.node2.b, Bf.on, (size_t)B * N, E, Cn, s);
    t_rowmask(Bf.on, in.flags, out_F.node, (size_t)B * N, Cn, s);
    return ok;
}

// from dF = dL/dF of the forward just run on `net`: TRAIN_WEIGHT_GRADS fills every gradient buffer bound in net.G; TRAIN_INPUT_GRADS
// (with `ig`) carries activation gradients only and ends in ig->d_tok.  false: a launch was refused
static bool train_backward(TrainNet &net, TrainBackward mode, const uint8_t *flags, CStatePtrs dF, const TrainInputGrad *ig, hipStream_t s) {
    const bool wg = mode == TRAIN_WEIGHT_GRADS;
    const TrainBufs &Bf = net.Bf;
    const int B = net.B, N = net.N, E = net.E, L = net.L, Ca = net.Ca, Cn = net.Cn, Cin = net.Cin, P = net.P, PP = P * P, T0 = net.R0 * net.R0;
    const size_t M0 = net.M0, Mp = net.Mp;
    float *const t_mh = net.t_mh, *const t_m3c = net.t_m3c, *const t_w = net.t_w, *const t_mc = net.t_mc, *const t_mc2 = net.t_mc2;
    auto skip_size = [&](int l) { return (size_t)B * net.skip_res[l] * net.skip_res[l] * net.skip_C[l]; };
    hipError_t e0 = (net.grouped || !wg) ? hipSuccess : hipMemsetAsync(Bf.d_emb, 0, sizeof(float) * (size_t)B * NOISE_EMB, s);
    for (int l = 0; l < L && e0 == hipSuccess; l++) e0 = hipMemsetAsync(Bf.d_skip[l], 0, sizeof(float) * skip_size(l), s);
    bool ok = e0 == hipSuccess;
    // heads
    float *d_on = t_mc, *d_hn = t_mc2, *d_pool = net.d_x, *d_rep = net.d_y;
    t_rowmask(dF.node, flags, d_on, (size_t)B * N, Cn, s);
    lin_bwd(wg, Bf.hn, net.node2.w, d_on, d_hn, net.node2.dw, net.node2.db, (size_t)B * N, E, Cn, s);
    t_gelu(Bf.hn_pre, d_hn, d_hn, (size_t)B * N * E, true, s);
    lin_bwd(wg, Bf.pool, net.node1.w, d_hn, d_pool, net.node1.dw, net.node1.db, (size_t)B * N, E, E, s);
    float *d_oa = t_m3c, *d_ha = t_mh;
    if (P > 1) ok = ok && t_adj_out_patch(nullptr, flags, nullptr, dF.adj, d_oa, B, N, P, Ca, true, s);
    else t_adj_out(nullptr, flags, nullptr, dF.adj, d_oa, B, N, Ca, true, s);
    lin_bwd(wg, Bf.ha, net.adj2.w, d_oa, d_ha, net.adj2.dw, net.adj2.db, Mp, E, Ca, s);
    t_gelu(Bf.ha_pre, d_ha, d_ha, Mp * E, true, s);
    lin_bwd(wg, Bf.rep, net.adj1.w, d_ha, d_rep, net.adj1.dw, net.adj1.db, Mp, E, E, s);
    if (P > 1) ok = ok && t_pool_bwd_patch(d_pool, flags, d_rep, B, N, P, E, s);
    else t_pool_bwd(d_pool, flags, d_rep, B, N, E, s);
    // read_out.2, .1 (Conv2d [out,in]) and .0 (ConvTranspose2d [in,out]), final norm
    float *d_z2 = t_mh, *d_z1 = t_m3c, *d_fy = t_w;
    lin_bwd(wg, Bf.z2, net.ro2.w, d_rep, d_z2, net.ro2.dw, net.ro2.db, Mp, E, E, s);
    lin_bwd(wg, Bf.z1, net.ro1.w, d_z2, d_z1, net.ro1.dw, net.ro1.db, Mp, E, E, s);
    if (P > 1) {   // d_z1 viewed [M0, p^2 E] against the weight image of the forward; the bias sees every pixel row
        if (wg) {
            t_gemm(true, false, Bf.fy, E, d_z1, PP * E, nullptr, Bf.ro_dimg, PP * E, E, PP * E, (int)M0, false, s);
            ok = ok && t_ro0_unpack(Bf.ro_dimg, net.ro0.dw, E, E, P, s);
            t_colsum(d_z1, E, net.ro0.db, (int)Mp, E, s);
        }
        t_gemm(false, true, d_z1, PP * E, Bf.ro_img, PP * E, nullptr, d_fy, E, (int)M0, E, PP * E, false, s);
    } else {
        if (wg) {
            t_gemm(true, false, Bf.fy, E, d_z1, E, nullptr, net.ro0.dw, E, E, E, (int)M0, false, s);    // dW [in,out] = y^T dz
            t_colsum(d_z1, E, net.ro0.db, (int)M0, E, s);
        }
        t_gemm(false, true, d_z1, E, net.ro0.w, E, nullptr, d_fy, E, (int)M0, E, E, false, s);        // dy = dz W^T
    }
    // blocks / up / down in reverse; dcur: the running gradient wrt the current activation (size up to M0*E*2), ping-pong with dnext
    float *dcur = net.d_x, *dnext = net.d_y;
    t_ln_bwd(net.xL, net.norm.w, Bf.fstats, d_fy, nullptr, dcur, net.norm.dw, net.norm.db, (int)M0, E, s);
    auto run_blocks = [&](int g) {
        for (int k = net.first[g + 1] - 1; k >= net.first[g]; k--) {
            TrainStage &st = net.stages[k];
            TrainBlockArgs &a = st.a;
            a.grad_out = dcur; a.grad_in = dnext; a.grad_emb = st.d_emb;
            a.d_x1 = t_w; a.t_mc = t_mc; a.t_mc2 = t_mc2; a.t_m3c = t_m3c; a.t_mh = t_mh;
            a.no_wgrad = !wg;
            ok = ok && train_block_backward(a, s);
            if (!net.grouped && wg) t_add(Bf.d_emb, st.d_emb, (size_t)B * NOISE_EMB, s);
            std::swap(dcur, dnext);
        }
    };
    int res = net.R0, C = E;
    for (int i = L - 1; i >= 0; i--) {
        run_blocks(L + i);
        if (i > 0) {
            // here res, C are the FINE values (after the breakup); the coarse input had res/2, 2C per source
            const int rc = res / 2, Cc = 2 * C; const size_t Mi = (size_t)B * rc * rc; const int D = 2 * Cc, Co = D / 4;
            float *d_upn = t_mh, *d_usc = t_m3c, *d_un = t_w, *d_uy = t_mh, *d_cat = t_m3c;
            lin_bwd(wg, Bf.upn[i], net.up_post[i].w, dcur, d_upn, net.up_post[i].dw, nullptr, 4 * Mi, Co, Co, s, net.lp);
            t_ln_bwd(Bf.usc[i], net.up_pn[i].w, Bf.upstats[i], d_upn, nullptr, d_usc, net.up_pn[i].dw, net.up_pn[i].db, (int)(4 * Mi), Co, s);
            t_regroup(d_usc, d_un, B, res, Co, true, s);   // transpose of the scatter = gather
            t_ln_bwd(Bf.uy[i], net.up_norm[i].w, Bf.ustats[i], d_un, nullptr, d_uy, net.up_norm[i].dw, net.up_norm[i].db, (int)Mi, D, s);
            lin_bwd(wg, Bf.ucat[i], net.up_pre[i].w, d_uy, d_cat, net.up_pre[i].dw, nullptr, Mi, D, D, s, net.lp);
            t_split(d_cat, dnext, Bf.d_skip[L - 1 - i], Mi, Cc, s);
            std::swap(dcur, dnext);
            res = rc; C = Cc;
        }
    }
    for (int l = L - 1; l >= 0; l--) {
        // the tensor at the end of encoder level l (after its merging, if any) also fed the decoder as skip[l]
        t_add(dcur, Bf.d_skip[l], skip_size(l), s);
        if (l < L - 1) {
            const int rf = res * 2, Cf = C / 2; const size_t M2 = (size_t)B * res * res;
            float *d_nrm = t_mh, *d_cat = t_m3c;
            lin_bwd(wg, Bf.mnrm[l], net.mrg_red[l].w, dcur, d_nrm, net.mrg_red[l].dw, nullptr, M2, 4 * Cf, 2 * Cf, s, net.lp);
            t_ln_bwd(Bf.mcat[l], net.mrg_norm[l].w, Bf.mstats[l], d_nrm, nullptr, d_cat, net.mrg_norm[l].dw, net.mrg_norm[l].db, (int)M2, 4 * Cf, s);
            t_regroup(d_cat, dnext, B, rf, Cf, false, s);   // transpose of the gather = scatter back to the fine grid
            std::swap(dcur, dnext);
            res = rf; C = Cf;
        }
        run_blocks(l);
    }
    // PatchEmbed: modulate <- LN <- 1x1 conv (the inputs are leaves of the training entries; dsg_precond_vjp goes on to them)
    float *d_pe_ln = dnext, *d_pe_lin = t_mh;
    t_modulate(Bf.pe_ln, Bf.pe_aff, dcur, d_pe_ln, Bf.pe_daff, B, T0, E, true, s);
    if (!wg) {
        // (sigma is not differentiated: the affine linears' own backward feeds parameter gradients and d_emb only)
    } else if (net.grouped) {
        // the affine linears' own backward, all at once: dWa_z = d_aff_z^T emb, d_ba_z = colsum(d_aff_z), d_emb = sum_z d_aff_z Wa_z
        TGemmGroup gw, gb, ge;
        // (d_emb: every product into its own [B, 512] buffer -- 16 x 2 tiles per product fill the chip, one shared output would
        // leave it to 32 blocks -- then one ordered sum)
        auto add = [&](const float *d_aff, const float *Wa, float *dWa, float *dba, float *d_emb_z, int C2) {
            gw.p[gw.n++] = TGemmProb{d_aff, Bf.emb, nullptr, dWa, C2, NOISE_EMB, NOISE_EMB, C2, NOISE_EMB, B};
            gb.p[gb.n++] = TGemmProb{d_aff, nullptr, nullptr, dba, C2, 0, 0, B, C2, 0};
            ge.p[ge.n++] = TGemmProb{d_aff, Wa, nullptr, d_emb_z, C2, NOISE_EMB, NOISE_EMB, B, NOISE_EMB, C2};
        };
        add(Bf.pe_daff, net.pe_aff.w, net.pe_aff.dw, net.pe_aff.db, Bf.pe_demb, 2 * E);
        for (const TrainStage &st : net.stages) add(st.a.d_aff, st.a.W.aff_w, st.a.G.aff_w, st.a.G.aff_b, st.d_emb, 2 * st.a.C);
        t_gemm_grouped(true, false, false, gw, s);
        t_colsum_grouped(gb, s);
        t_gemm_grouped(false, false, false, ge, s);
        t_sum_grouped(ge, Bf.d_emb, B * NOISE_EMB, s);
    } else {   // each block has added its own d_emb above; PatchEmbed's affine accumulates into the same sum
        t_gemm(true, false, Bf.pe_daff, 2 * E, Bf.emb, NOISE_EMB, nullptr, net.pe_aff.dw, NOISE_EMB, 2 * E, NOISE_EMB, B, false, s);
        t_colsum(Bf.pe_daff, 2 * E, net.pe_aff.db, B, 2 * E, s);
        t_gemm(false, false, Bf.pe_daff, 2 * E, net.pe_aff.w, NOISE_EMB, nullptr, Bf.d_emb, NOISE_EMB, B, NOISE_EMB, 2 * E, true, s);
    }
    t_ln_bwd(Bf.pe_lin, net.pe_norm.w, Bf.pe_stats, d_pe_ln, nullptr, d_pe_lin, net.pe_norm.dw, net.pe_norm.db, (int)M0, E, s);
    if (!wg) {
        // d_tok = d_pe_lin W_img: only the columns of the current adjacency / node values, the weight image zero-padded to x32 columns
        // (sigma is not differentiated: no noise-embedding backward)
        if (P > 1) ok = ok && t_live_cols_patch(net.pe.w, Cin, P, ig->img, E, Ca, Cn, net.self_condition != 0, s);
        else t_live_cols(net.pe.w, Cin, ig->img, E, Ca, Cn, net.self_condition != 0, s);
        t_gemm(false, false, d_pe_lin, E, ig->img, ig->ld, nullptr, ig->d_tok, ig->ld, (int)M0, ig->ld, E, false, s);
    } else {
        if (P > 1) {   // the gradient of the weight image, then back to [E, Cin, p, p]
            lin_bwd(wg, Bf.tok, Bf.pe_img, d_pe_lin, nullptr, Bf.pe_dimg, net.pe.db, M0, net.Kp, E, s);
            ok = ok && t_pe_unpack(Bf.pe_dimg, net.pe.dw, E, Cin, P, net.Kp, s);
        } else lin_bwd(wg, Bf.tok, net.pe.w, d_pe_lin, nullptr, net.pe.dw, net.pe.db, M0, Cin, E, s);
        // noise embedding: emb = silu(map1(silu(map0(pe))))
        float *d_m1 = t_mc, *d_s0 = t_mc2;
        t_silu(Bf.m1, Bf.d_emb, d_m1, (size_t)B * NOISE_EMB, true, s);
        lin_bwd(wg, Bf.s0, net.map1.w, d_m1, d_s0, net.map1.dw, net.map1.db, B, NOISE_EMB, NOISE_EMB, s);
        t_silu(Bf.m0, d_s0, d_s0, (size_t)B * NOISE_EMB, true, s);
        lin_bwd(wg, Bf.pe, net.map0.w, d_s0, nullptr, net.map0.dw, net.map0.db, B, E, NOISE_EMB, s);
    }
    return ok;
}

// the end of every entry: everything is queued on the caller's stream and every buffer involved outlives the call (caller's or the
// handle's), so there is no synchronisation here -- the host runs ahead into the optimiser step's launches
static int train_finish(dsg_handle h, bool ok, hipStream_t s) {
    HIP_TRY(h, hipGetLastError());
    if (!ok) return fail(h, DSG_ERR_HIP, "a training kernel failed to launch");
    if (t_scratch_failed(s, true)) return fail(h, DSG_ERR_HIP, "out of memory (training scratch of this stream)");
    return DSG_OK;
}

extern "C" {

int dsg_train_grads(dsg_handle h, int32_t B, const float *in_adj, const float *in_node, const uint8_t *flags, const float *c_noise,
                    const float *sc_adj, const float *sc_node, const float *grad_F_adj, const float *grad_F_node, float *out_F_adj,
                    float *out_F_node, int32_t n_params, const char *const *names, float *const *grad_params, void *stream) {
    // the training form reads the raw weights only, so weights re-uploaded after an optimiser step need no re-packing here
    // (dsg_finalize_weights must have run once: block plans); the sampling-path entries still insist on `finalized`
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (int rc = patch_training_gate(h, "dsg_train_grads")) return rc;
    if (B < 1 || !in_adj || !in_node || !flags || !c_noise || !out_F_adj || !out_F_node) return fail(h, DSG_ERR_INVALID, "null argument");
    const bool bwd = grad_F_adj != nullptr;
    if (bwd && (!grad_F_node || !names || !grad_params)) return fail(h, DSG_ERR_INVALID, "backward needs both output gradients and the parameter gradient buffers");
    hipStream_t s = (hipStream_t)stream;
    TrainNet net{};
    const int rc = train_net_build(h, net, B, sc_adj, sc_node, bwd, n_params, names, grad_params, s);
    if (rc != DSG_OK) return rc;
    TrainLp lp;
    if (!train_lp_begin(h, net, lp, s)) return fail(h, DSG_ERR_HIP, "out of memory");
    bool ok = train_forward(net, TrainInputs{in_adj, in_node, flags, c_noise, sc_adj, sc_node}, StatePtrs{out_F_adj, out_F_node}, s);
    if (ok && bwd) ok = train_backward(net, TRAIN_WEIGHT_GRADS, flags, CStatePtrs{grad_F_adj, grad_F_node}, nullptr, s);
    train_lp_end(h, lp);
    return train_finish(h, ok, s);
}

// the preconditioned entries' handle-owned io buffer: c_in x, c_noise, the network's F, dL/dD and dL/dF
namespace {
struct TrainIo { float *in_a, *in_n, *cn, *F_a, *F_n, *dD_a, *dD_n, *dF_a, *dF_n; };
}
static bool train_io(dsg_handle h, int B, hipStream_t s, TrainIo &io) {
    const size_t na = (size_t)B * h->Ca * h->N * h->N, nn = (size_t)B * h->N * h->Cn;
    return train_carve(h, h->train_io, s, [&](TArena &A) {
        io.in_a = A.get(na); io.in_n = A.get(nn); io.cn = A.get(B); io.F_a = A.get(na); io.F_n = A.get(nn);
        io.dD_a = A.get(na); io.dD_n = A.get(nn); io.dF_a = A.get(na); io.dF_n = A.get(nn);
    });
}

int dsg_train_step_grads(dsg_handle h, int32_t B, const float *noisy_adj, const float *noisy_node, const uint8_t *flags, const float *sigmas,
                         const float *sc_adj, const float *sc_node, const float *target_adj, const float *target_node,
                         const float *loss_weight, float edge_loss_weight, float node_loss_weight, float iou_loss_weight,
                         int32_t iou_loss_type, float *out_D_adj, float *out_D_node, float *out_loss_adj, float *out_loss_node,
                         int32_t n_params, const char *const *names, float *const *grad_params, void *stream) {
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (int rc = patch_training_gate(h, "dsg_train_step_grads")) return rc;
    if (iou_loss_type < DSG_IOU_IOU || iou_loss_type > DSG_IOU_CIOU) return fail(h, DSG_ERR_INVALID, "iou_loss_type %d", iou_loss_type);
    if (B < 1 || !noisy_adj || !noisy_node || !flags || !sigmas || !target_adj || !target_node || !out_D_adj || !out_D_node || !out_loss_adj ||
        !out_loss_node)
        return fail(h, DSG_ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims_of(h, B);
    const CStatePtrs noisy{noisy_adj, noisy_node}, target{target_adj, target_node}, D{out_D_adj, out_D_node};
    const bool want_grads = names && grad_params && n_params > 0;
    TrainIo io;
    if (!train_io(h, B, s, io)) return fail(h, DSG_ERR_HIP, "out of memory");
    launch_precond_in(noisy, sigmas, StatePtrs{io.in_a, io.in_n}, io.cn, d, s);   // c_in * x, c_noise = ln(sigma)/4
    TrainNet net{};
    const int rc = train_net_build(h, net, B, sc_adj, sc_node, want_grads, n_params, names, grad_params, s);
    if (rc != DSG_OK) return rc;
    TrainLp lp;
    if (!train_lp_begin(h, net, lp, s)) return fail(h, DSG_ERR_HIP, "out of memory");
    bool ok = train_forward(net, TrainInputs{io.in_a, io.in_n, flags, io.cn, sc_adj, sc_node}, StatePtrs{io.F_a, io.F_n}, s);
    if (ok) {
        // D = mask(c_skip x + c_out F) (precond.py:101-104); per-sample losses; with gradients: dL/dD and dL/dF = c_out dL/dD
        launch_precond_out(noisy, CStatePtrs{io.F_a, io.F_n}, sigmas, flags, StatePtrs{out_D_adj, out_D_node}, d, s);
        launch_rainbow_loss(D, target, flags, loss_weight, edge_loss_weight, node_loss_weight, iou_loss_weight, iou_loss_type, out_loss_adj,
                            out_loss_node, d, s);
        if (want_grads)
            launch_rainbow_loss_backward(D, target, flags, loss_weight, edge_loss_weight, node_loss_weight, iou_loss_weight, iou_loss_type, sigmas,
                                         StatePtrs{io.dD_a, io.dD_n}, StatePtrs{io.dF_a, io.dF_n}, d, s);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && want_grads) ok = train_backward(net, TRAIN_WEIGHT_GRADS, flags, CStatePtrs{io.dF_a, io.dF_n}, nullptr, s);
    train_lp_end(h, lp);
    return train_finish(h, ok, s);
}

int dsg_train_self_cond(dsg_handle h, int32_t B, const float *noisy_adj, const float *noisy_node, const uint8_t *flags, const float *sigmas,
                        float *out_sc_adj, float *out_sc_node, void *stream) {
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (int rc = patch_training_gate(h, "dsg_train_self_cond")) return rc;
    if (B < 1 || !noisy_adj || !noisy_node || !flags || !sigmas || !out_sc_adj || !out_sc_node) return fail(h, DSG_ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims_of(h, B);
    TrainIo io;
    if (!train_io(h, B, s, io)) return fail(h, DSG_ERR_HIP, "out of memory");
    launch_precond_in(CStatePtrs{noisy_adj, noisy_node}, sigmas, StatePtrs{io.in_a, io.in_n}, io.cn, d, s);
    TrainNet net{};
    int rc = train_net_build(h, net, B, nullptr, nullptr, false, 0, nullptr, nullptr, s);
    if (rc != DSG_OK) return rc;
    TrainLp lp;
    if (!train_lp_begin(h, net, lp, s)) return fail(h, DSG_ERR_HIP, "out of memory");
    const bool ok = train_forward(net, TrainInputs{io.in_a, io.in_n, flags, io.cn, nullptr, nullptr}, StatePtrs{io.F_a, io.F_n}, s);
    train_lp_end(h, lp);
    if ((rc = train_finish(h, ok, s)) != DSG_OK) return rc;
    launch_precond_out(CStatePtrs{noisy_adj, noisy_node}, CStatePtrs{io.F_a, io.F_n}, sigmas, flags, StatePtrs{out_sc_adj, out_sc_node}, d, s);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_precond_vjp(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, const float *sigmas,
                    const float *sc_adj, const float *sc_node, const float *grad_D_adj, const float *grad_D_node, dsg_grad_fn fn, void *user,
                    float *out_D_adj, float *out_D_node, float *out_grad_adj, float *out_grad_node, void *stream) {
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (int rc = patch_training_gate(h, "dsg_precond_vjp")) return rc;
    if (B < 1 || !adj || !node || !flags || !sigmas || !out_D_adj || !out_D_node || !out_grad_adj || !out_grad_node)
        return fail(h, DSG_ERR_INVALID, "null argument");
    if ((grad_D_adj == nullptr) != (grad_D_node == nullptr)) return fail(h, DSG_ERR_INVALID, "grad_D_adj and grad_D_node go together");
    if ((fn != nullptr) == (grad_D_adj != nullptr)) return fail(h, DSG_ERR_INVALID, "give either the callback or grad_D_adj / grad_D_node, not %s", fn ? "both" : "neither");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims_of(h, B);
    const int N = h->N, Ca = h->Ca, Cn = h->Cn, E = h->E, P = h->P;
    const size_t M0 = (size_t)B * h->R0 * h->R0;
    // refused before anything is enqueued: what the last kernel (t_assemble_bwd) cannot take
    if (!(P > 1 ? t_assemble_bwd_patch_ok(Cn) : t_assemble_bwd_ok(Cn)) || (size_t)B * N > 0x7fffffffu)
        return fail(h, DSG_ERR_INVALID, "input gradients are not built for C_node %d (partial sums beyond LDS) or B * N = %zu", Cn, (size_t)B * N);
    const int Np = P > 1 ? t_live_cols_patch_width(Ca, Cn, P) : t_live_cols_width(Ca, Cn);
    TrainIo io;
    TrainInputGrad ig{nullptr, nullptr, Np};
    float *coef = nullptr;   // c_skip [B] | c_in [B], left by t_precond_bwd for t_assemble_bwd
    if (!train_io(h, B, s, io) ||
        !train_carve(h, h->train_vjp, s, [&](TArena &A) { ig.d_tok = A.get(M0 * Np); ig.img = A.get((size_t)E * Np); coef = A.get(2 * (size_t)B); }))
        return fail(h, DSG_ERR_HIP, "out of memory");
    launch_precond_in(CStatePtrs{adj, node}, sigmas, StatePtrs{io.in_a, io.in_n}, io.cn, d, s);
    TrainNet net{};
    int rc = train_net_build(h, net, B, sc_adj, sc_node, false, 0, nullptr, nullptr, s);
    if (rc != DSG_OK) return rc;
    bool ok = train_forward(net, TrainInputs{io.in_a, io.in_n, flags, io.cn, sc_adj, sc_node}, StatePtrs{io.F_a, io.F_n}, s);
    const float *g_a = grad_D_adj, *g_n = grad_D_node;
    if (ok) {
        launch_precond_out(CStatePtrs{adj, node}, CStatePtrs{io.F_a, io.F_n}, sigmas, flags, StatePtrs{out_D_adj, out_D_node}, d, s);
        if (fn) {   // the callee enqueues g = dL/dD into the gradient outputs, which the last kernel below turns into the result in place
            const int cb_rc = fn(user, out_D_adj, out_D_node, out_grad_adj, out_grad_node);
            if (cb_rc != 0) {
                (void)hipGetLastError();   // a launch error so far is this call's, not the next one's
                return fail(h, DSG_ERR_INVALID, "the gradient callback returned %d: no backward kernel was launched", cb_rc);
            }
            g_a = out_grad_adj; g_n = out_grad_node;
        }
        t_precond_bwd(g_a, g_n, sigmas, flags, io.dF_a, io.dF_n, coef, B, N, Ca, Cn, s);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok) ok = train_backward(net, TRAIN_INPUT_GRADS, flags, CStatePtrs{io.dF_a, io.dF_n}, &ig, s);
    if ((rc = train_finish(h, ok, s)) != DSG_OK) return rc;
    if (!(P > 1 ? t_assemble_bwd_patch(ig.d_tok, Np, flags, coef, coef + B, g_a, g_n, out_grad_adj, out_grad_node, B, N, P, Ca, Cn, s)
                : t_assemble_bwd(ig.d_tok, Np, flags, coef, coef + B, g_a, g_n, out_grad_adj, out_grad_node, B, N, Ca, Cn, false, s)))
        return fail(h, DSG_ERR_INVALID, "the assemble backward refused B %d, N %d, C_adj %d, C_node %d, pitch %d", B, N, Ca, Cn, Np);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

// Host-side plan of an ODE run (include/dsg.h): the evaluation levels in execution order and the quadrature weights of int n(t)/t dt.
// h = b - a is the fp32 difference the step table holds; the weights are formed in double from the widened fp32 values.
int32_t dsg_ode_evals(const dsg_sampler_cfg *c, const dsg_ode_cfg *ode, float *t_eval, double *weight, int32_t cap) {
    if (!c || !ode || c->num_steps < 2) return DSG_ERR_INVALID;
    if (ode->direction != DSG_ODE_ENCODE && ode->direction != DSG_ODE_DECODE) return DSG_ERR_INVALID;
    if (ode->probe < DSG_ODE_PROBE_NONE || ode->probe > DSG_ODE_PROBE_GAUSSIAN) return DSG_ERR_INVALID;
    if (solver_2m(c)) return DSG_ERR_INVALID;
    const int T = c->num_steps;
    std::vector<float> t(T), nz(T);
    dsg_sigma_schedule(c, nullptr, t.data(), nz.data(), nullptr);
    for (int i = 0; i < T; i++) if (nz[i] != 0.f) return DSG_ERR_INVALID;
    const bool heun = solver_heun(c);
    const int32_t n = (heun ? 2 : 1) * (T - 1);
    if (!t_eval && !weight) return n;
    if (cap < n) return DSG_ERR_INVALID;
    int e = 0;
    for (int j = 0; j < T - 1; j++) {
        const int k = ode->direction == DSG_ODE_ENCODE ? T - 1 - j : j;
        const float a = t[k], b = ode->direction == DSG_ODE_ENCODE ? t[k - 1] : t[k + 1];
        volatile float hs = b - a;
        const double ah = std::fabs((double)hs);
        if (t_eval) t_eval[e] = a;
        if (weight) weight[e] = heun ? ah / (2.0 * (double)a) : ah / (double)a;
        e++;
        if (heun) {
            if (t_eval) t_eval[e] = b;
            if (weight) weight[e] = ah / (2.0 * (double)b);
            e++;
        }
    }
    return n;
}

// The probability-flow ODE between the schedule's levels (include/dsg.h).  Every evaluation is dsg_precond_vjp's chain on the state the
// run holds: precond_in, the training-form forward, precond_out, and with a probe the backward of eps, the assemble backward with a
// ZERO c_skip array (what it writes is then the network part c_in c_out J_F^T eps alone) and the per-graph contraction with eps.  The
// updates are the sampler's Euler / Heun element operations on a StepRow table of this run's (a, b) pairs, driven by a device step
// counter.  Everything is enqueued on `stream`; the only synchronisation is the one the host seed array needs.
int dsg_ode_run(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_ode_cfg *ode, int32_t B, const uint8_t *flags, const float *x_adj,
                const float *x_node, const uint64_t *graph_seeds, const float *probe_adj, const float *probe_node, float *out_adj,
                float *out_node, float *out_probe_adj, float *out_probe_node, double *out_net_trace, void *stream) {
    if (!h || !h->ever_finalized) return fail(h, DSG_ERR_STATE, "weights not finalized");
    if (int rc = patch_training_gate(h, "dsg_ode_run")) return rc;
    if (!cfg || !ode || B < 1 || !flags || !x_adj || !x_node || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null argument");
    if (cfg->num_steps < 2) return fail(h, DSG_ERR_INVALID, "dsg_ode_run needs num_steps >= 2 (it steps between the schedule's levels; num_steps is %d)", cfg->num_steps);
    if (solver_2m(cfg)) return fail(h, DSG_ERR_INVALID, "dsg_ode_run has no multistep solver (heun = %d): use DSG_SOLVER_EULER or DSG_SOLVER_HEUN", DSG_SOLVER_DPMPP_2M);
    if (ode->direction != DSG_ODE_ENCODE && ode->direction != DSG_ODE_DECODE) return fail(h, DSG_ERR_INVALID, "direction %d", ode->direction);
    if (ode->probe < DSG_ODE_PROBE_NONE || ode->probe > DSG_ODE_PROBE_GAUSSIAN) return fail(h, DSG_ERR_INVALID, "probe %d", ode->probe);
    const int32_t n_evals = dsg_ode_evals(cfg, ode, nullptr, nullptr, 0);
    if (n_evals < 0)   // everything else was checked above: what is left is a level with churn noise
        return fail(h, DSG_ERR_INVALID, "dsg_ode_run follows the probability-flow ODE and needs a schedule that draws no churn noise at any level: "
                    "set S_churn = 0 (S_churn is %g)", (double)cfg->S_churn);
    const bool probing = ode->probe != DSG_ODE_PROBE_NONE;
    if ((probe_adj == nullptr) != (probe_node == nullptr)) return fail(h, DSG_ERR_INVALID, "probe_adj and probe_node go together");
    if ((out_probe_adj == nullptr) != (out_probe_node == nullptr)) return fail(h, DSG_ERR_INVALID, "out_probe_adj and out_probe_node go together");
    if (probing && !probe_adj && !graph_seeds) return fail(h, DSG_ERR_INVALID, "a probe needs graph_seeds (host, one per graph) or recorded probe_adj / probe_node");
    if (probing && !out_net_trace) return fail(h, DSG_ERR_INVALID, "a probe needs out_net_trace (device, [n_evals = %d, B] doubles)", n_evals);
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims_of(h, B);
    const int N = h->N, Ca = h->Ca, Cn = h->Cn, E = h->E, P = h->P;
    const size_t M0 = (size_t)B * h->R0 * h->R0, na = (size_t)B * Ca * N * N, nn = (size_t)B * N * Cn;
    if (!(P > 1 ? t_assemble_bwd_patch_ok(Cn) : t_assemble_bwd_ok(Cn)) || (size_t)B * N > 0x7fffffffu)
        return fail(h, DSG_ERR_INVALID, "input gradients are not built for C_node %d (partial sums beyond LDS) or B * N = %zu", Cn, (size_t)B * N);
    const bool heun = solver_heun(cfg);
    const int n_steps = cfg->num_steps - 1;
    // host tables: the evaluation levels as [n_evals, B] sigma rows, the (a, b) pairs as StepRow rows
    std::vector<float> t_eval(n_evals), sig((size_t)n_evals * B);
    dsg_ode_evals(cfg, ode, t_eval.data(), nullptr, n_evals);
    for (int e = 0; e < n_evals; e++) for (int b = 0; b < B; b++) sig[(size_t)e * B + b] = t_eval[e];
    std::vector<float> lv(cfg->num_steps);
    dsg_sigma_schedule(cfg, nullptr, lv.data(), nullptr, nullptr);
    std::vector<StepRow> rows(n_steps);
    for (int j = 0; j < n_steps; j++) {
        const int k = ode->direction == DSG_ODE_ENCODE ? cfg->num_steps - 1 - j : j;
        const float a = lv[k], b = ode->direction == DSG_ODE_ENCODE ? lv[k - 1] : lv[k + 1];
        volatile float hs = b - a;
        rows[j] = StepRow{0.f, a, 1.0f / a, 1.0f / b, hs, k, 0.f, 0};
    }
    // buffers: the training entries' io and vjp regions, and this entry's own
    const int Np = P > 1 ? t_live_cols_patch_width(Ca, Cn, P) : t_live_cols_width(Ca, Cn);
    TrainIo io;
    TrainInputGrad ig{nullptr, nullptr, Np};
    float *coef = nullptr, *zero = nullptr, *sig_d = nullptr, *tab_f = nullptr, *ctl_f = nullptr, *seeds_f = nullptr;
    StatePtrs x{}, xp{}, D1{}, D2{}, eps{}, g{};
    auto state = [&](TArena &A, bool on) { StatePtrs p{nullptr, nullptr}; if (on) { p.adj = A.get(na); p.node = A.get(nn); } return p; };
    if (!train_io(h, B, s, io) ||
        !train_carve(h, h->train_vjp, s, [&](TArena &A) { ig.d_tok = A.get(M0 * Np); ig.img = A.get((size_t)E * Np); coef = A.get(2 * (size_t)B); }) ||
        !train_carve(h, h->train_ode, s, [&](TArena &A) {
            x = state(A, true); D1 = state(A, true); xp = state(A, heun); D2 = state(A, heun); eps = state(A, probing); g = state(A, probing);
            zero = A.get(B); sig_d = A.get((size_t)n_evals * B); tab_f = A.get((size_t)n_steps * (sizeof(StepRow) / sizeof(float)));
            ctl_f = A.get((sizeof(RunCtl) + sizeof(float) - 1) / sizeof(float)); seeds_f = A.get(2 * (size_t)B);
        }))
        return fail(h, DSG_ERR_HIP, "out of memory");
    StepRow *tab = (StepRow *)tab_f;
    RunCtl *ctl = (RunCtl *)ctl_f;
    unsigned long long *seeds_d = (unsigned long long *)seeds_f;
    TrainNet net{};
    int rc = train_net_build(h, net, B, nullptr, nullptr, false, 0, nullptr, nullptr, s);
    if (rc != DSG_OK) return rc;
    // uploads, once
    const RunCtl ctl_h{0, n_steps, 0ull, nullptr, nullptr, nullptr};
    HIP_TRY(h, hipMemcpyAsync(sig_d, sig.data(), sizeof(float) * sig.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(tab, rows.data(), sizeof(StepRow) * rows.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(ctl, &ctl_h, sizeof(RunCtl), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(zero, 0, sizeof(float) * B, s));
    if (probing && !probe_adj) HIP_TRY(h, hipMemcpyAsync(seeds_d, graph_seeds, sizeof(unsigned long long) * (size_t)B, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));   // the tables above are this call's host memory, the seeds the caller's
    // the start state, masked; the probe
    launch_init(CStatePtrs{x_adj, x_node}, CStatePtrs{nullptr, nullptr}, 1.0f, 0, nullptr, 0u, flags, x, d, s);
    if (probing) {
        if (probe_adj) launch_init(CStatePtrs{probe_adj, probe_node}, CStatePtrs{nullptr, nullptr}, 1.0f, 0, nullptr, 0u, flags, eps, d, s);
        else launch_probe(ode->probe == DSG_ODE_PROBE_RADEMACHER, seeds_d, DSG_ODE_PROBE_STREAM, flags, eps, d, s);
        if (out_probe_adj) {
            HIP_TRY(h, hipMemcpyAsync(out_probe_adj, eps.adj, sizeof(float) * na, hipMemcpyDeviceToDevice, s));
            HIP_TRY(h, hipMemcpyAsync(out_probe_node, eps.node, sizeof(float) * nn, hipMemcpyDeviceToDevice, s));
        }
    }
    const CStatePtrs ceps{eps.adj, eps.node};
    bool ok = hipGetLastError() == hipSuccess;
    g_fixed_tiles = h->opt.batch_invariant;   // the training-form GEMMs: one route at every batch size (t_gemm)
    // D = D(at, level e) into `dst`; with a probe also row e of the traces
    auto evaluate = [&](CStatePtrs at, int e, StatePtrs dst) {
        const float *sg = sig_d + (size_t)e * B;
        launch_precond_in(at, sg, StatePtrs{io.in_a, io.in_n}, io.cn, d, s);
        ok = ok && train_forward(net, TrainInputs{io.in_a, io.in_n, flags, io.cn, nullptr, nullptr}, StatePtrs{io.F_a, io.F_n}, s);
        if (!ok) return;
        launch_precond_out(at, CStatePtrs{io.F_a, io.F_n}, sg, flags, dst, d, s);
        if (!probing) return;
        t_precond_bwd(ceps.adj, ceps.node, sg, flags, io.dF_a, io.dF_n, coef, B, N, Ca, Cn, s);
        ok = ok && train_backward(net, TRAIN_INPUT_GRADS, flags, CStatePtrs{io.dF_a, io.dF_n}, &ig, s);
        ok = ok && (P > 1 ? t_assemble_bwd_patch(ig.d_tok, Np, flags, zero, coef + B, ceps.adj, ceps.node, g.adj, g.node, B, N, P, Ca, Cn, s)
                          : t_assemble_bwd(ig.d_tok, Np, flags, zero, coef + B, ceps.adj, ceps.node, g.adj, g.node, B, N, Ca, Cn, false, s));
        ok = ok && t_graph_dot(ceps.adj, ceps.node, g.adj, g.node, flags, out_net_trace + (size_t)e * B, B, N, Ca, Cn, s);
    };
    const CStatePtrs cx{x.adj, x.node}, cxp{xp.adj, xp.node}, cD1{D1.adj, D1.node}, cD2{D2.adj, D2.node};
    for (int j = 0, e = 0; j < n_steps && ok; j++) {
        evaluate(cx, e++, D1);
        if (!ok) break;
        if (heun) {
            launch_euler_tab(cx, cD1, tab, ctl, flags, xp, d, s);                  // x' = x_a + h f(x_a, a)
            evaluate(cxp, e++, D2);
            if (!ok) break;
            launch_heun_tab(cx, cD1, cD2, tab, ctl, flags, x, d, s);               // x_b = x_a + (h / 2)(f(x_a, a) + f(x', b)), in place
        } else launch_euler_tab(cx, cD1, tab, ctl, flags, x, d, s);                // in place: an element is read, then written, by one thread
        launch_step_advance(ctl, s);
    }
    g_fixed_tiles = false;
    if ((rc = train_finish(h, ok, s)) != DSG_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(out_adj, x.adj, sizeof(float) * na, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(out_node, x.node, sizeof(float) * nn, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_train_enable_patch(dsg_handle h, int32_t on) {
    if (!h) return DSG_ERR_INVALID;
    h->train_patch = on != 0;
    return DSG_OK;
}

int32_t dsg_train_patch_enabled(dsg_handle h) { return h ? h->train_patch : 0; }

int dsg_train_set_precision(dsg_handle h, int32_t mode) {
    if (!h) return DSG_ERR_INVALID;
    if (mode != DSG_TRAIN_F32 && mode != DSG_TRAIN_BF16) return fail(h, DSG_ERR_INVALID, "training precision %d (DSG_TRAIN_F32 = 0 or DSG_TRAIN_BF16 = 1)", mode);
    h->train_precision = mode;
    return DSG_OK;
}

// ---- autoguidance ----
int dsg_attach_guide(dsg_handle h, dsg_handle guide, float scale, float sigma_lo, float sigma_hi) {
    if (!h) return DSG_ERR_INVALID;
    if (!guide) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide is NULL");
    if (guide == h) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide is the handle itself (guide == h)");
    if (guide->guide) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide has a guide of its own (one level only)");
    if (h->guide_of) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: h is itself the guide of another handle (one level only)");
    if (guide->guide_of && guide->guide_of != h) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide is already attached to another handle");
    if (!guide->finalized) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide is not finalized (dsg_finalize_weights)");
    if (guide->N != h->N) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide's max_node_num %d differs from %d", guide->N, h->N);
    if (guide->Ca != h->Ca) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide's c_adj %d differs from %d", guide->Ca, h->Ca);
    if (guide->Cn != h->Cn) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide's c_node %d differs from %d", guide->Cn, h->Cn);
    if ((guide->cfg.self_condition != 0) != (h->cfg.self_condition != 0))
        return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide's self_condition %d differs from %d", guide->cfg.self_condition, h->cfg.self_condition);
    if (guide->device != h->device) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: guide was created on device %d, h on device %d", guide->device, h->device);
    if (!std::isfinite(scale)) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: scale = %g is not finite", (double)scale);
    if (std::isnan(sigma_lo)) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: sigma_lo is NaN");
    if (std::isnan(sigma_hi)) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: sigma_hi is NaN");
    if (sigma_lo > sigma_hi) return fail(h, DSG_ERR_INVALID, "dsg_attach_guide: sigma_lo = %g is above sigma_hi = %g", (double)sigma_lo, (double)sigma_hi);
    if (h->guide) (void)dsg_detach_guide(h);
    drop_guided_bodies(h);
    h->guide = guide; guide->guide_of = h;
    volatile float sm1 = scale - 1.0f;   // float32, one rounding
    h->guide_scale = scale; h->guide_sm1 = sm1; h->guide_lo = sigma_lo; h->guide_hi = sigma_hi;
    return DSG_OK;
}

int dsg_detach_guide(dsg_handle h) {
    if (!h) return DSG_ERR_INVALID;
    if (!h->guide) return DSG_OK;
    drop_guided_bodies(h);
    h->guide->guide_of = nullptr;
    h->guide = nullptr;
    h->guide_scale = 1.f; h->guide_sm1 = 0.f; h->guide_lo = 0.f; h->guide_hi = 0.f;
    return DSG_OK;
}

int dsg_guide_info(dsg_handle h, dsg_handle *guide, float *scale, float *sigma_lo, float *sigma_hi) {
    if (!h) return DSG_ERR_INVALID;
    if (guide) *guide = h->guide;
    if (scale) *scale = h->guide_scale;
    if (sigma_lo) *sigma_lo = h->guide_lo;
    if (sigma_hi) *sigma_hi = h->guide_hi;
    return DSG_OK;
}

int dsg_guide_forwards(dsg_handle h, int64_t *n) {
    if (!h) return DSG_ERR_INVALID;
    if (!n) return fail(h, DSG_ERR_INVALID, "dsg_guide_forwards: n is NULL");
    *n = h->last_guide_forwards;
    return DSG_OK;
}

int dsg_train_get_precision(dsg_handle h, int32_t *mode) {
    if (!h || !mode) return fail(h, DSG_ERR_INVALID, "null argument");
    *mode = h->train_precision;
    return DSG_OK;
}

int32_t dsg_debug_train_routes(dsg_handle h, int32_t *out, int32_t cap) {
    if (!h || cap < 0 || (cap > 0 && !out)) return DSG_ERR_INVALID;
    const int32_t n = (int32_t)h->train_counts.size();
    for (int32_t k = 0; k < n && k < cap; k++) {
        const TLpCount &c = h->train_counts[k];
        out[4 * k] = c.rows; out[4 * k + 1] = c.cls; out[4 * k + 2] = c.n_bf16; out[4 * k + 3] = c.n_f32;
    }
    return n;
}

int dsg_train_bind_params(dsg_handle h, int32_t n_params, const char *const *names, const float *const *params) {
    if (!h || n_params < 0 || (n_params > 0 && (!names || !params))) return fail(h, DSG_ERR_INVALID, "null argument");
    h->train_params.clear();
    for (int k = 0; k < n_params; k++) {
        if (!names[k] || !params[k]) { h->train_params.clear(); return fail(h, DSG_ERR_INVALID, "null entry %d", k); }
        const std::string key = strip_prefix(names[k]);
        bool known = false;
        for (auto &sp : h->specs) if (sp.key == key) { known = !sp.is_index && !sp.is_mask; break; }
        if (!known) { h->train_params.clear(); return fail(h, DSG_ERR_WEIGHTS, "unexpected key '%s'", names[k]); }
        h->train_params[key] = params[k];
    }
    return DSG_OK;
}

int dsg_adam_step(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                  const int64_t *numel, int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                  float *out_total_norm, void *stream) {
    if (n_tensors < 1 || !params || !grads || !exp_avg || !exp_avg_sq || !numel || step < 1) return DSG_ERR_INVALID;
    for (int i = 0; i < n_tensors; i++) if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || numel[i] < 1) return DSG_ERR_INVALID;
    return t_adam_step(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, step, lr, beta1, beta2, eps, weight_decay, max_grad_norm,
                       out_total_norm, (hipStream_t)stream) ? DSG_OK : DSG_ERR_HIP;
}

int dsg_ema_update(int32_t n_tensors, float *const *ema, const float *const *params, const int64_t *numel, float decay, void *stream) {
    if (n_tensors < 1 || !ema || !params || !numel) return DSG_ERR_INVALID;
    for (int i = 0; i < n_tensors; i++) if (!ema[i] || !params[i] || numel[i] < 1) return DSG_ERR_INVALID;
    return t_ema_update(n_tensors, ema, params, numel, decay, (hipStream_t)stream) ? DSG_OK : DSG_ERR_HIP;
}

double dsg_profile_clock_ghz(dsg_handle h) { return h ? h->prof_clock_ghz : 0.0; }

int dsg_decode(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, int32_t edge_encoding,
               int32_t node_encoding, int32_t n_adj_type, int32_t n_node_type, int32_t node_chans, int32_t *out_adj, int32_t *out_node,
               float *out_bbox, void *stream) {
    if (!h || B < 1 || !adj || !node || !flags || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    if (edge_encoding < DSG_ENC_BITS || edge_encoding > DSG_ENC_DDPM || node_encoding < DSG_ENC_BITS || node_encoding > DSG_ENC_DDPM)
        return fail(h, DSG_ERR_INVALID, "encoding must be DSG_ENC_BITS, DSG_ENC_ONE_HOT or DSG_ENC_DDPM");
    if (n_adj_type < 2 || n_node_type < 2) return fail(h, DSG_ERR_INVALID, "fewer than two types");   // attribute_code.py:132
    if (node_chans < 1 || node_chans > h->Cn || (out_bbox && h->Cn < node_chans + 4)) return fail(h, DSG_ERR_INVALID, "node_chans");
    // the channel counts an encoding implies (sg_utils.py:348-409): one channel per type, or a single one
    if ((edge_encoding == DSG_ENC_ONE_HOT && h->Ca != n_adj_type) || (edge_encoding == DSG_ENC_DDPM && h->Ca != 1) ||
        (edge_encoding == DSG_ENC_BITS && (h->Ca > 30 || (1 << h->Ca) < n_adj_type)))
        return fail(h, DSG_ERR_INVALID, "edge encoding %d with %d types does not fit %d adjacency channels", edge_encoding, n_adj_type, h->Ca);
    if ((node_encoding == DSG_ENC_ONE_HOT && node_chans != n_node_type) || (node_encoding == DSG_ENC_DDPM && node_chans != 1) ||
        (node_encoding == DSG_ENC_BITS && (node_chans > 30 || (1 << node_chans) < n_node_type)))
        return fail(h, DSG_ERR_INVALID, "node encoding %d with %d types does not fit %d attribute channels", node_encoding, n_node_type, node_chans);
    launch_decode(adj, node, flags, edge_encoding, node_encoding, n_adj_type, n_node_type, node_chans, out_adj, out_node, out_bbox,
                  dims_of(h, B), (hipStream_t)stream);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_encode(dsg_handle h, int32_t B, const int32_t *q_adj, const int32_t *q_node, const float *bbox, const uint8_t *flags,
               int32_t edge_encoding, int32_t node_encoding, int32_t n_adj_type, int32_t n_node_type, int32_t node_chans, float *out_adj,
               float *out_node, void *stream) {
    if (!h || B < 1) return fail(h, DSG_ERR_INVALID, "batch must be >= 1");
    if (!q_adj || !q_node || !flags || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    if (edge_encoding < DSG_ENC_BITS || edge_encoding > DSG_ENC_DDPM || node_encoding < DSG_ENC_BITS || node_encoding > DSG_ENC_DDPM)
        return fail(h, DSG_ERR_INVALID, "encoding must be DSG_ENC_BITS, DSG_ENC_ONE_HOT or DSG_ENC_DDPM");
    if (n_adj_type < 2 || n_node_type < 2) return fail(h, DSG_ERR_INVALID, "fewer than two types");
    if (node_chans < 1 || node_chans > h->Cn || (bbox && h->Cn < node_chans + 4))
        return fail(h, DSG_ERR_INVALID, "node_chans %d does not fit C_node %d%s", node_chans, h->Cn, bbox ? " with four bbox channels" : "");
    // the channel counts an encoding implies, as dsg_decode checks them
    if ((edge_encoding == DSG_ENC_ONE_HOT && h->Ca != n_adj_type) || (edge_encoding == DSG_ENC_DDPM && h->Ca != 1) ||
        (edge_encoding == DSG_ENC_BITS && (h->Ca > 30 || (1 << h->Ca) < n_adj_type)))
        return fail(h, DSG_ERR_INVALID, "edge encoding %d with %d types does not fit %d adjacency channels", edge_encoding, n_adj_type, h->Ca);
    if ((node_encoding == DSG_ENC_ONE_HOT && node_chans != n_node_type) || (node_encoding == DSG_ENC_DDPM && node_chans != 1) ||
        (node_encoding == DSG_ENC_BITS && (node_chans > 30 || (1 << node_chans) < n_node_type)))
        return fail(h, DSG_ERR_INVALID, "node encoding %d with %d types does not fit %d attribute channels", node_encoding, n_node_type, node_chans);
    launch_encode(q_adj, q_node, bbox, flags, edge_encoding, node_encoding, n_adj_type, n_node_type, node_chans, out_adj, out_node,
                  dims_of(h, B), (hipStream_t)stream);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}

int dsg_decode_bits(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, int32_t n_adj_type,
                    int32_t n_node_type, int32_t node_bits, int32_t *out_adj, int32_t *out_node, float *out_bbox, void *stream) {
    if (!h || B < 1 || !adj || !node || !flags || !out_adj || !out_node) return fail(h, DSG_ERR_INVALID, "null tensor");
    if (node_bits < 1 || node_bits > h->Cn || (out_bbox && h->Cn < node_bits + 4)) return fail(h, DSG_ERR_INVALID, "node_bits");
    launch_decode(adj, node, flags, DSG_ENC_BITS, DSG_ENC_BITS, n_adj_type, n_node_type, node_bits, out_adj, out_node, out_bbox, dims_of(h, B),
                  (hipStream_t)stream);
    HIP_TRY(h, hipGetLastError());
    return DSG_OK;
}


}  // extern "C"
