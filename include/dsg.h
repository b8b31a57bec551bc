/*
 * dsg.h -- C ABI of libdsg.so: the MI355X (gfx950) scene-graph diffusion sampler.
 *
 * The reference (ubc-vision/DiffuseSG) has no FFI layer; its seam for this path is three
 * Python callables.  Each entry point below names the reference interface it
 * replaces (R/ = DiffuseSG/ in the reference tree):
 *
 *   dsg_denoise  <->  DiffuseSG.forward                R/model/diffusesg/diffusesg.py:765
 *   dsg_precond  <->  NodeAdjPrecond.forward           R/model/precond/precond.py:65
 *   dsg_sample   <->  NodeAdjEDMSampler.sample         R/runner/mcmc_sampler/edm.py:291
 *   dsg_set_weight / dsg_finalize_weights <-> load_model(strict=True)  R/utils/sampling_utils.py:34
 *   dsg_create   <->  get_network's DiffuseSG(...) ctor kwargs         R/utils/learning_utils.py:47-64
 *
 * Conventions
 *   - return 0 on success, a negative dsg_status otherwise; dsg_last_error(h) has the message.
 *   - plain pointers and sizes only.  All tensor arguments are DEVICE pointers to contiguous
 *     fp32 (flags: uint8) in the reference's layouts:
 *        adj   [B, C_adj, N, N]     node  [B, N, C_node]     flags [B, N] (1 = valid node)
 *     (the reference squeezes singleton channel dims; the memory layout is unchanged).
 *   - the caller owns every I/O buffer; the library owns packed weights and its workspace and
 *     never mutates an input.  One handle per device, not re-entrant.  All work is enqueued on
 *     the caller's stream (`stream` is a hipStream_t passed as void*; NULL = default stream).
 *     Training entries: the saved-activation arena and backward scratch belong to the handle; the small scratch of the
 *     handle-less kernels (split-K partials, column sums, the optimiser's tables) is kept per STREAM, so two streams never
 *     share a buffer; an allocation failure anywhere is reported as DSG_ERR_HIP, never by terminating the process.
 *   - there is no CPU fallback: every entry point fails with DSG_ERR_HIP if the device is missing.
 */
#ifndef DSG_H
#define DSG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSG_MAX_LAYERS 8
/* Generation of this header's argument lists; dsg_abi_version() returns the one the library was built with.  A binding compares the two
 * at load time (diffusesg_amd/lib.py does): round 3 inserted `iou_loss_type` into three entries, and a caller built against the older
 * header would otherwise pass shifted arguments without any error.  History: 1-3 = rounds 1-3 (unversioned), 4 = round 4
 * (dsg_decode with an encoding argument, dsg_abi_version, dsg_last_error(NULL)).  dsg_sample_seeded, dsg_gen_noise_seeded and the option
 * "batch_invariant" were added without touching an existing argument list: still 4; so were the single-kernel test hooks,
 * dsg_ode_run / dsg_ode_evals, dsg_guide_cfg / dsg_sample_guided / dsg_guide_coef, dsg_rel_cfg / dsg_sample_guided_rel, and
 * dsg_option_info.  5 = the test and measurement hooks moved to dsg_debug.h (the same library exports them, this header no longer
 * declares them) and three bf16-pipeline hooks there took a `kernel` argument.  The number covers both headers.  dsg_content_cfg /
 * dsg_sample_guided_content (and its test hook) were added without touching an existing argument list: still 5. */
#define DSG_ABI_VERSION 5

typedef enum {
    DSG_OK = 0,
    DSG_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    DSG_ERR_WEIGHTS = -2,   /* unknown key, shape mismatch, or missing tensor at finalize */
    DSG_ERR_HIP = -3,       /* HIP runtime error (no device, out of memory, launch failure) */
    DSG_ERR_STATE = -4      /* call order violated (e.g. denoise before finalize_weights) */
} dsg_status;

typedef struct dsg_handle_s *dsg_handle;

/* Mirrors the kwargs of DiffuseSG(...) as passed by get_network (learning_utils.py:47-64). */
typedef struct dsg_config {
    int32_t max_node_num;              /* img_size (N); patch_size is 1 under dsg_create, dsg_create_patch takes it */
    int32_t c_adj;                     /* out_chans_adj */
    int32_t c_node;                    /* out_chans_node */
    int32_t embed_dim;                 /* feature_dims[-1], 96 */
    int32_t num_layers;                /* len(depths) */
    int32_t depths[DSG_MAX_LAYERS];
    int32_t num_heads[DSG_MAX_LAYERS]; /* [3,6,12,24]; head_dim must be 32 */
    int32_t window_size;
    int32_t mlp_ratio;                 /* 4 */
    int32_t self_condition;            /* train.self_cond */
} dsg_config;

/* Mirrors NodeAdjEDMSampler.__init__ (edm.py:236-255) for discretization='edm', schedule='linear',
 * scaling='none' (the only combination get_mc_sampler builds, sampling_utils.py:15-23). */
#define DSG_SOLVER_EULER 0
#define DSG_SOLVER_HEUN 1
#define DSG_SOLVER_DPMPP_2M 2          /* second-order multistep (DPM-Solver++ 2M): one forward per step, see dsg_multistep_coef */
typedef struct dsg_sampler_cfg {
    int32_t num_steps;
    int32_t heun;                      /* the solver, DSG_SOLVER_*: 0 'euler', 1 'heun', 2 'dpmpp_2m'; any other nonzero value is 'heun' */
    float S_churn, S_min, S_max, S_noise;
    double sigma_min, sigma_max, rho;  /* 0.002, 80, 7 */
    int32_t use_graph;                 /* 1: replay captured hipGraphs: whole step bodies of the loop (churn, preconditioning, the
                                          network forwards, the Euler/Heun/multistep update; per-step scalars come from a device table
                                          indexed by a device step counter), or with option "loop_graph" = 0 only the network
                                          forward; 0: every kernel is launched eagerly */
    int32_t reserved;
} dsg_sampler_cfg;

/* Counters of the last dsg_sample / dsg_sample_known / dsg_sample_walk call. */
typedef struct dsg_sample_stats {
    int64_t precond_calls;             /* 2T-1 (heun) or T (euler, dpmpp_2m); of a walk: 2 per executed Heun step whose index is not T-1,
                                          else 1 */
    int64_t net_forwards;              /* precond_calls + number of coins that fired */
    int64_t graph_replays;             /* network forwards that ran from replayed graphs (== net_forwards with use_graph) */
} dsg_sample_stats;

int dsg_create(const dsg_config *cfg, dsg_handle *out);   /* == dsg_create_patch(cfg, 1, out) */
/* The reference's `patch_size` (p in {1, 2, 4}; N % p == 0): the U-Net runs on R x R tokens, R = N / p; token t = ti R + tj covers the
 * pixels (I, J) = (p ti + a, p tj + b), 0 <= a, b < p.  Level l has resolution R >> l; windows and shifts are clipped at that
 * resolution.  States, flags and every entry point's tensors keep their [B, C, N, N] / [B, N, C] shapes.  Weights:
 *   patch_embed.proj.weight [E, Cin, p, p]   (Conv2d, stride p: y[t, e] = bias[e] + sum_{c,a,b} W[e, c, a, b] img[c, p ti + a, p tj + b])
 *   read_out.0.weight       [E, E, p, p]     (ConvTranspose2d, [in, out, a, b]: r0[(I, J), o] = b0[o] + sum_i LN(x)[t, i] W0[i, o, a, b])
 * Inside the library the rows of the read-out chain stay in (token, a, b) order; adjacency outputs and the node pooling are masked per
 * pixel by flag_I && flag_J, and the node mean is over the N pixels of a row.
 * At p > 1: with two levels or more the coarsest resolution R >> (L - 1) must be even (the reference's PatchBreakup asserts it on its
 * input) -- DSG_ERR_INVALID otherwise; "prune_masked" / "dedup_masked" report 0 (their lists are derived at pixel resolution);
 * "gemm_split", "gemm_bf16" and "batch_invariant" are refused (dsg_set_option keeps the old value; a handle created under such an
 * environment default is refused by its first forward until the option is set to 0); "fused_patch_embed" / "fused_readout" select the
 * fused E = 96 kernels at p = 2 (in_chans <= 64, C_adj <= 32; default) or the chain of kernels, p = 4 always runs the chain; and
 * dsg_train_grads, dsg_train_step_grads, dsg_train_self_cond, dsg_precond_vjp and dsg_ode_run return DSG_ERR_INVALID (messages name
 * patch_size) until dsg_train_enable_patch switches the training form on for the handle. */
int dsg_create_patch(const dsg_config *cfg, int32_t patch_size, dsg_handle *out);
void dsg_destroy(dsg_handle h);
/* h == NULL: the reason the last dsg_create on the calling thread failed (there is no handle to ask then) */
const char *dsg_last_error(dsg_handle h);
const char *dsg_version(void);
int32_t dsg_abi_version(void);   /* DSG_ABI_VERSION of the header the library was built from */

/* `key` is the reference state-dict name, with or without the 'model.' prefix of the precond
 * wrapper (precond.py:15) and/or the 'module.' prefix of DDP (sampling_utils.py:47-53).
 * `data` is fp32 (int64 for relative_position_index, which is validated and dropped);
 * is_device != 0 means `data` is a device pointer. */
int dsg_set_weight(dsg_handle h, const char *key, const void *data, const int64_t *shape, int32_t ndim,
                   int32_t is_device);
/* Packs derived tables; fails with DSG_ERR_WEIGHTS naming the first missing tensor (strict=True). */
int dsg_finalize_weights(dsg_handle h);
/* Number of state-dict keys expected / names, to let a binding iterate them. */
int dsg_num_weight_keys(dsg_handle h);
const char *dsg_weight_key(dsg_handle h, int32_t i);

/* Device bytes the library holds for batch size B (activations + sampler state; + the known tensors and masks of dsg_sample_known
 * once a conditioned call has run at that batch size; + the 8 B bytes of graph seeds once a seeded call has). */
size_t dsg_workspace_bytes(dsg_handle h, int32_t B);

/* DiffuseSG.forward: noise_labels[B] = c_noise; sc_adj / sc_node may be NULL (zeros). */
int dsg_denoise(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags,
                const float *noise_labels, const float *sc_adj, const float *sc_node,
                float *out_adj, float *out_node, void *stream);

/* NodeAdjPrecond.forward with precond='edm'.  `coin` is the outcome of the reference's
 * `np.random.rand() < 0.5` (precond.py:90), drawn by the caller. */
int dsg_precond(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags,
                const float *sigmas, const float *sc_adj, const float *sc_node, int32_t coin,
                float *out_adj, float *out_node, void *stream);

/* NodeAdjEDMSampler.sample.
 *   init_adj/init_node  NULL: drawn on device (Philox, `seed`), masked (gen_init_sample, edm.py:257-289)
 *   noise_adj [T,B,C_adj,N,N], noise_node [T,B,N,C_node]  NULL: churn noise drawn on device
 *   coins [precond calls] host pointer, one byte per preconditioned call in call order;
 *         NULL: Bernoulli(0.5) from a host generator seeded with `seed`
 *   gt_adj/gt_node non-NULL: sanity-check mode (edm.py:372-377), the denoiser is bypassed
 *   snap_steps/snap_adj/snap_node: optional interim snapshots (edm.py:429-432): after step
 *         snap_steps[k] the state is copied to slot k of snap_adj / snap_node (device) */
int dsg_sample(dsg_handle h, const dsg_sampler_cfg *cfg, int32_t B, const uint8_t *flags,
               const float *init_adj, const float *init_node,
               const float *noise_adj, const float *noise_node,
               const uint8_t *coins, uint64_t seed,
               const float *gt_adj, const float *gt_node,
               const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
               float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream);

/* Conditional sampling: dsg_sample with some entries of the result given (scene-graph completion; with all labels and relations
 * given and the boxes free, layout generation).  Not in the reference; it is its sanity-check mode (edm.py:372-377, gt_adj / gt_node
 * above: the denoiser's output replaced EVERYWHERE, the state converges to it) applied per entry.  Wherever mask_* is nonzero the
 * denoised estimate D is known_* -- selected, not blended, so the value arrives bit-exact -- and the network's elsewhere.  Known entries
 * of the state then follow known + t * eps, a draw of the forward marginal at every noise level: the network sees them as noisy
 * context, and the last step (Euler to t = 0) lands them on the known values.  The select sits in the kernel that writes D, for the
 * stage-1 D, the stage-2 D and the D of the extra self-conditioning pass of a fired coin alike, so the self-conditioning input of the
 * next forward carries the known values too; no extra pass over the state, no extra launch.
 *   known_adj [B,C_adj,N,N], known_node [B,N,C_node] fp32, mask_adj / mask_node uint8 of the same shapes (nonzero = known): device
 *         pointers, all four required (DSG_ERR_INVALID otherwise).  known_* at padded nodes or where the mask is 0 is ignored.
 *   everything else -- init, churn noise, coins, seed, snapshots, stats, use_graph / "loop_graph" -- as dsg_sample, which this call
 *         equals bit for bit when no entry is known; with every entry known it equals dsg_sample(gt_* = known_*).
 * The four tensors are copied (on `stream`) into buffers of the batch-B workspace, allocated by the first conditioned call for that
 * batch size and freed with the handle: captured step bodies never reference caller memory, and the caller may reuse its buffers as
 * soon as the call returns.  Conditioned and unconditioned step bodies are captured separately; nothing is remembered between
 * calls -- the next dsg_sample is unconditioned.  dsg_workspace_bytes(h, B) includes these 5 * (C_adj N N + N C_node) * B bytes
 * from that first conditioned call on (before it, and for batch sizes never sampled conditionally, it does not). */
int dsg_sample_known(dsg_handle h, const dsg_sampler_cfg *cfg, int32_t B, const uint8_t *flags,
                     const float *init_adj, const float *init_node,
                     const float *noise_adj, const float *noise_node,
                     const uint8_t *coins, uint64_t seed,
                     const float *known_adj, const float *known_node,
                     const uint8_t *mask_adj, const uint8_t *mask_node,
                     const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                     float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream);

/* A walk over the noise levels: which schedule indices a run executes, in which order.  The schedule of dsg_sigma_schedule has
 * indices 0..T-1 with levels t_0 > ... > t_{T-1}, and t_T = 0.  Indices in [start_step, lo) and [hi, T) are executed once, in order;
 * [lo, hi) is cut into blocks [b, e) of jump_len indices (the last one may be shorter) and each block is executed n_resample times in a
 * row (RePaint-style resampling: go down a few levels, diffuse back up, go down again -- the generated and the known part get time
 * to agree).  Between two passes the state, which is at t_e, is diffused forward to t_b by ONE Gaussian of variance t_b^2 - t_e^2 (the
 * composition of the forward steps in between, not jump_len single steps).  L = T - start_step + (n_resample - 1)(hi - lo) steps are
 * executed; the walk is batch-uniform, as sigma is.  {0, 1, 1, 0, 0} is the trivial walk: dsg_sample's. */
#define DSG_WALK_MAX_STEPS (1 << 20)   /* cap on L */
typedef struct dsg_walk_cfg {
    int32_t start_step;                /* s: first schedule index executed, 0 <= s < T */
    int32_t jump_len;                  /* j >= 1: length of a resampled block */
    int32_t n_resample;                /* r >= 1: times each block is executed; 1 = no resampling */
    int32_t resample_lo;               /* blocks partition [lo, hi), starting at lo; s <= lo <= hi <= T */
    int32_t resample_hi;               /* <= 0 means T */
    int32_t reserved[3];
} dsg_walk_cfg;

/* The walk as the loop executes it -- host-only, as dsg_sigma_schedule exposes the schedule.  Returns L, or a negative dsg_status
 * (DSG_ERR_INVALID: a violated range above, L > DSG_WALK_MAX_STEPS, or cap < L with an output array given).  sched_idx [L]: the schedule
 * index of executed step k.  noise_coef [L]: the coefficient of its churn draw -- the schedule's noise_coef[sched_idx[k]], the very
 * float, except at the first step of a repeated pass of a block [b, e): there the jump-back noise is merged into the churn draw (two
 * independent Gaussians are one), coef = (float)sqrt((double)t_b^2 - (double)t_e^2 + (double)noise_coef[b]^2) on the widened fp32
 * schedule values, t_e = 0 where the block ends the schedule.  The step is still evaluated at t_hat_b.  Either array may be NULL. */
int32_t dsg_walk_steps(const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t *sched_idx, float *noise_coef, int32_t cap);

/* The second-order multistep solver, heun = DSG_SOLVER_DPMPP_2M: DPM-Solver++ 2M (Lu et al. 2022) in EDM variables, sigma(t) = t,
 * lambda = -ln t.  An executed step k at schedule index i, with no noise drawn in front of it, is the Euler step on an estimate
 * extrapolated from the previous step's:
 *     x_next = mask(x_hat + h (x_hat - D~) / t_hat),   D~ = D + c_k (D - D_prev),   c_k = ln(t_i / t_{i+1}) / (2 ln(t_{i-1} / t_i)).
 * One preconditioned call per executed step: coins, precond_calls and cost are the Euler solver's.  c_k = 0 -- the Euler step itself,
 * the same kernel and the same captured step body as under DSG_SOLVER_EULER, bit for bit -- where there is no usable history:
 *   - k = 0 (a partial-noise start included);
 *   - schedule index T-1, the step to t = 0 (the usual lower-order final step; ln is undefined there);
 *   - the previous executed step was not schedule index i-1;
 *   - the step's noise_coef (dsg_walk_steps) is nonzero: the first step of a repeated pass of a resampling walk.
 * The solver follows the probability-flow ODE, so a schedule that draws churn noise at any level (dsg_sigma_schedule's noise_coef) is
 * refused with DSG_ERR_INVALID, by this function and by the dsg_sample* calls before anything is launched: use S_churn = 0.  Walks
 * (resampling, partial-noise start) and known entries are allowed; at a known entry D = D_prev = known, so D~ = known exactly and
 * the last step still lands on it.  In the sanity-check mode D_prev = D = gt.
 * This helper is host-only: returns L, as dsg_walk_steps does, or a negative status: DSG_ERR_INVALID for a bad walk, cap < L with coef
 * given, or churn noise with the multistep solver.  walk == NULL is the trivial walk.  coef [L]: c_k, evaluated in double on the widened fp32 levels
 * (float)sigma_steps[.] and rounded once to float -- the values the loop puts into its step table; all 0 for the other solvers. */
int32_t dsg_multistep_coef(const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, float *coef, int32_t cap);

/* dsg_sample_known along a walk, optionally from a partial-noise start.  dsg_sample and dsg_sample_known are the trivial walk of the
 * same loop; a walk changes which rows the loop's tables hold, not the step: the captured step bodies, the launches per executed step
 * and their cost are the plain loop's (the jump-back noise rides in the step's churn draw: no extra pass over the state, no extra
 * launch).  Randomness is indexed by EXECUTED step k = 0..L-1: Philox stream k + 1 (stream 0 stays the initial sample), recorded
 * churn noise noise_adj [L,B,C_adj,N,N] / noise_node [L,B,N,C_node], coins one per preconditioned call in executed order (a Heun
 * step at schedule index T-1 is the Euler step to 0 on every pass); snap_steps counts executed steps.  Self-conditioning carries over
 * a jump unchanged: its input is the last denoised estimate, whichever level it came from.
 *   known_* / mask_*: all four given -- everything said about dsg_sample_known holds (workspace copies, nothing sticky, separate
 *         conditioned step bodies) -- or all four NULL: an unconditioned walk.  Anything in between is DSG_ERR_INVALID.
 *   base_adj [B,C_adj,N,N], base_node [B,N,C_node] (both or neither): the partial-noise start (SDEdit-style variation / editing).  The
 *         run begins at index start_step with x = mask(base + t_s * eps), eps = init_* or stream 0 as ever; base_* holds value-space
 *         tensors (what dsg_encode writes), is read once before the loop and never by a step body.  NULL is allowed only with
 *         start_step = 0 and is dsg_sample's pure-noise start, bit for bit; start_step > 0 without a base is DSG_ERR_INVALID.  With
 *         a mask as well, making the base agree with known_* at known entries is the caller's business: the loop pulls known entries
 *         to known_* whatever the base says, but the first steps then see a context that is not a draw of its forward marginal.
 * The step table has L rows, the per-level tables (noise embedding, the blocks' (scale, shift) rows) stay at T rows and are reached
 * through each row's schedule index.  A call whose L outgrows the step table reallocates it and drops the captured step bodies. */
int dsg_sample_walk(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk, int32_t B, const uint8_t *flags,
                    const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                    const float *noise_adj, const float *noise_node, const uint8_t *coins, uint64_t seed,
                    const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                    const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                    float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream);

/* The library's device noise streams (Philox4x32-10 keyed by `seed`, Box-Muller): what dsg_sample draws when it is handed
 * NULL init / NULL churn noise.  noise_stream 0 = the initial sample of gen_init_sample (edm.py:257-289: randn, rows and
 * columns of padded nodes zeroed, NOT yet scaled by sigma(t0)); noise_stream i+1 = the churn noise of step i (the
 * randn_like draws of edm.py:361-364).  Writes mask(eps) in the layouts above.  dsg_sample(init = this output) is
 * bit-identical to dsg_sample(init = NULL) with the same seed, so a caller that needs the unscaled init back
 * (nodes_ls[0] of edm.py:326-337) draws it here first. */
int dsg_gen_noise(dsg_handle h, int32_t B, const uint8_t *flags, uint64_t seed, uint32_t noise_stream,
                  float *out_adj, float *out_node, void *stream);

/* Per-graph noise streams: every graph of the batch has its own 64-bit key, and the draw for graph b, stream r, element j is the
 * generator above, unchanged, as Philox(graph_seeds[b], r, j) with j the element's index INSIDE its graph:
 *     adjacency entry (c, i, k): j = (c N + i) N + k        node entry (i, c): j = C_adj N^2 + i C_node + c
 * -- the global index of the unseeded stream at B = 1, so dsg_gen_noise_seeded(B = 1, {s}) is dsg_gen_noise(B = 1, s) bit for bit, and
 * row b of a seeded batch is the B = 1 draw of graph_seeds[b] whatever B is and wherever the graph sits.  Streams as above (0: initial
 * sample, k + 1: churn draw of executed step k, a walk's merged jump-back noise included); padded entries draw nothing and are 0.
 * graph_seeds: HOST pointer, [B], required (NULL is DSG_ERR_INVALID).  It is copied, on `stream`, into a device buffer of the batch-B
 * workspace, allocated by the first seeded call at that batch size (dsg_workspace_bytes counts its 8 B bytes from then on); the call
 * synchronises `stream` before it returns.  Needs finalized weights (it uses the workspace). */
int dsg_gen_noise_seeded(dsg_handle h, int32_t B, const uint8_t *flags, const uint64_t *graph_seeds /* host */,
                         uint32_t noise_stream, float *out_adj, float *out_node, void *stream);

/* dsg_sample_walk drawing from the per-graph streams: the same loop, and everything said above about walks, known entries, the
 * multistep solver, snapshots, stats and captured step bodies holds (a seeded run replays the same bodies, one graph launch per step).
 * Two differences:
 *   - noise: init (stream 0, also of a partial-noise start) and churn draws come from Philox(graph_seeds[b], stream, local index), see
 *         dsg_gen_noise_seeded.  Precedence is unchanged: given init_* win over stream 0, recorded noise_* over the churn streams.
 *   - coins: coins == NULL draws them from `coin_seed`, by the generator and formula dsg_sample uses for `seed`.  The coin is one draw
 *         per preconditioned call shared by the whole batch (precond.py:90): part of a run's identity, not of a graph's.
 * Hence dsg_sample_seeded(B = 1, graph_seeds = {s}, coin_seed = s) equals dsg_sample(B = 1, seed = s) bit for bit.  With the option
 * "batch_invariant" = 1 a graph's result depends on the weights, its flags row, its seed, the coin sequence, cfg / walk, its own known
 * row and the handle's options -- not on B, its position, the other graphs.
 *   walk == NULL: the trivial walk.  graph_seeds: host, [B], required; copied to the workspace on `stream` ahead of the synchronise
 *   the loop's set-up already has.  Nothing is sticky: the next dsg_sample is unseeded. */
int dsg_sample_seeded(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk /* NULL: trivial walk */,
                      int32_t B, const uint8_t *flags,
                      const uint64_t *graph_seeds /* host, [B], required */, uint64_t coin_seed,
                      const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                      const float *noise_adj, const float *noise_node, const uint8_t *coins,
                      const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                      const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                      float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream);

/* Box guidance through the skip path, inside the loop.  Per preconditioned call at schedule index i, noise level
 * t = t_hat[i], input x_hat and estimate D (after the valid mask and, in a conditioned run, the known select):
 *     b      = D_node[..., C_node-4:] * 0.5 + 0.5, read as (cx, cy, w, h)              (dsg_decode's boxes)
 *     L      = w_overlap L_overlap + w_region L_region + w_align L_align               (diffusesg_amd/guide.py's three box losses, always
 *              with the node flags; the region loss with one rectangle per selected node)
 *     g      = dL/dD_node: zero outside the four box channels and at padded nodes; relu passes where its argument is > 0, minimum and
 *              maximum split a tie evenly (torch autograd's conventions)
 *     c_i    = weights[i] * t^2 * c_skip(t),  c_skip = 0.25 / (t^2 + 0.25)             (dsg_guide_coef: one float32 per schedule index)
 *     shift  = c_i g, zero at node entries whose known mask is set: known entries win and stay bit-exact
 *     f_b    = shift-norm clip: 1 if ||shift_b|| <= clip_ratio ||x_hat_b - D_b||, else that bound over ||shift_b|| (both 2-norms per
 *              graph, the second over the graph's whole state; fixed-order float64 sums, no atomics, independent of B)
 *     D~     = D - f_b shift
 * and the solver's update reads D~ wherever it reads D: Euler, both Heun stages, and the multistep extrapolation D~ + c (D~ - D~_prev).
 * The self-conditioning input of the next call stays D, and the D of a fired coin's extra pass is not shifted.  This is the guidance of
 * guide.guided_sample with the network's Jacobian dropped from dD/dx_hat = c_skip I + c_out dF/dx_hat: an approximation, exact where
 * that Jacobian vanishes, at the cost of one small kernel per call (two with the clip) and no backward.
 *   w_*: loss weights (finite); tau > 0 wherever w_align != 0; clip_ratio >= 0, or DSG_GUIDE_CLIP_NONE (any +infinity): unclipped, no norm
 *   pass is launched; sel [B,N] uint8 / region [B,N,4] (x0, y0, x1, y1): DEVICE, required where w_region != 0, else unread -- node n of
 *   graph b contributes where sel is set and the node is valid; weights [T]: HOST, finite, one w_i per SCHEDULE index (a walk's executed
 *   step finds its entry through its schedule index).  sel / region / the coefficients are copied into workspace memory on `stream`
 *   ahead of the run's synchronise (dsg_workspace_bytes counts them once allocated): step bodies never reference caller memory. */
typedef struct dsg_guide_cfg {
    float w_overlap, w_region, w_align;
    float tau;
    float clip_ratio;
    int32_t reserved;         /* 0 */
    const uint8_t *sel;
    const float *region;
    const float *weights;
} dsg_guide_cfg;
#define DSG_GUIDE_CLIP_NONE (__builtin_inff())

/* c_i [T] as the guided loop stages them: w_i t^2 * 0.25 / (t^2 + 0.25), t = the float32 t_hat[i] of dsg_sigma_schedule, evaluated in
 * double and rounded once to float (as dsg_multistep_coef does): within half an ulp of the real value.  Host-only.  Returns T, or DSG_ERR_INVALID (null argument, num_steps < 1, cap < T, a non-finite weight). */
int32_t dsg_guide_coef(const dsg_sampler_cfg *cfg, const float *weights /* host [T] */, float *coef /* host [T] */, int32_t cap);

/* dsg_sample_seeded's loop and argument list with the guidance above.  graph_seeds == NULL: one noise stream over the batch keyed by
 * `coin_seed`, which then is dsg_sample_walk's `seed` (noise and coins).  gt_adj / gt_node (both or neither): dsg_sample's sanity-check
 * mode, the guide then runs on gt; not together with known_* or graph_seeds.  loss_trace: DEVICE [L,B] or NULL -- L(D) of the stage-1
 * call of every executed step.  Guided step bodies are captured bodies of their own: an unguided run enqueues exactly what it did, and
 * with every weights[i] = 0 the result equals the unguided run's.
 * Refused with DSG_ERR_INVALID before anything is launched, the message naming the argument: guide == NULL, guide->weights == NULL,
 * C_node < 4, N > 64, tau <= 0 with w_align != 0, w_region != 0 without sel / region, a non-finite weight, a negative or NaN clip_ratio,
 * and everything dsg_sample_seeded refuses (the multistep solver on a schedule with churn among it). */
int dsg_sample_guided(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk /* NULL: trivial walk */,
                      int32_t B, const uint8_t *flags,
                      const uint64_t *graph_seeds /* host, [B], or NULL */, uint64_t coin_seed,
                      const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                      const float *noise_adj, const float *noise_node, const uint8_t *coins,
                      const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                      const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                      const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                      float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream);

/* Box guidance: spatial relations between node pairs.  A fourth loss on the boxes above, L = ... + w_rel L_rel, read from
 * ordered node pairs: entry (i, j) of a kind matrix has SUBJECT i (the row) and OBJECT j (the column).  With the lines of a box in
 * guide.py's order (l, cx, r, t, cy, bt; y grows downwards), h(v) = relu(v)^2 and m = margin >= 0, the pair adds
 *     0 none          0                         1 LEFT_OF   h(cx_i - cx_j + m)       2 RIGHT_OF  h(cx_j - cx_i + m)
 *     3 ABOVE         h(cy_i - cy_j + m)        4 BELOW     h(cy_j - cy_i + m)
 *     5 INSIDE        h(l_j - l_i) + h(r_i - r_j) + h(t_j - t_i) + h(bt_i - bt_j)         6 CONTAINS  INSIDE with i and j exchanged
 *     7 ON            (bt_i - t_j)^2 + h(l_j - cx_i) + h(cx_i - r_j)
 * and L_rel is the sum over graphs and ordered pairs i != j of valid nodes; (i, j) and (j, i) count on their own, kinds above 7 are
 * none.  h is C1: a pair exactly on a hinge adds exactly 0 to loss and gradient, and no tie convention is needed.  Gradients are
 * closed forms in float64, rounded once; fixed-order sums, no atomics, nothing depends on B.
 *   source DSG_REL_GIVEN: kinds [B,N,N] uint8, DEVICE, copied into workspace memory like sel / region.
 *   source DSG_REL_DECODED: at every preconditioned call entry (i, j) of the D_adj the guide is handed (after the valid mask and the
 *     known select; gt in the sanity-check mode) is decoded to an integer predicate by dsg_decode's rule for `encoding` (DSG_ENC_*) and
 *     `n_adj_type`, and its kind is pred_kind[predicate]; pred_kind [n_adj_type] uint8, HOST, copied once per run.  A NaN under
 *     DSG_ENC_DDPM decodes to none.  Rows, columns and the diagonal that are not live are never read.  The kinds are constants of the
 *     call: no gradient flows through the decode thresholds, and g stays zero outside the box channels. */
#define DSG_REL_GIVEN 0
#define DSG_REL_DECODED 1
#define DSG_REL_NONE 0
#define DSG_REL_LEFT_OF 1
#define DSG_REL_RIGHT_OF 2
#define DSG_REL_ABOVE 3
#define DSG_REL_BELOW 4
#define DSG_REL_INSIDE 5
#define DSG_REL_CONTAINS 6
#define DSG_REL_ON 7
typedef struct dsg_rel_cfg {
    float w_rel, margin;
    int32_t source;            /* DSG_REL_GIVEN 0, DSG_REL_DECODED 1 */
    int32_t encoding;          /* DSG_ENC_* of the adjacency (decoded source) */
    int32_t n_adj_type;        /* number of predicates = entries of pred_kind (decoded source) */
    int32_t reserved;          /* 0 */
    const uint8_t *kinds;      /* DEVICE [B,N,N] (given source) */
    const uint8_t *pred_kind;  /* HOST [n_adj_type], entries 0..7 (decoded source) */
} dsg_rel_cfg;

/* dsg_sample_guided with the relation term.  rel == NULL or rel->w_rel == 0: dsg_sample_guided itself -- the same plan keys, the same
 * captured bodies, the same bits.  Otherwise the guide kernel's relation variant runs behind every preconditioned call, in step bodies
 * of their own.  Refused with DSG_ERR_INVALID before anything is launched, the message naming the argument: a non-finite w_rel, a
 * negative or NaN margin, a source outside {0, 1}, kinds == NULL with the given source and w_rel != 0; with the decoded source
 * pred_kind == NULL, n_adj_type < 1, a table entry above 7, an unknown encoding or one that does not fit the adjacency channels (as
 * dsg_decode); and everything dsg_sample_guided refuses. */
int dsg_sample_guided_rel(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk /* NULL: trivial walk */,
                          int32_t B, const uint8_t *flags,
                          const uint64_t *graph_seeds /* host, [B], or NULL */, uint64_t coin_seed,
                          const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                          const float *noise_adj, const float *noise_node, const uint8_t *coins,
                          const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                          const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                          const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                          float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream, const dsg_rel_cfg *rel);

/* Content guidance: steer samples to contain given triplets.  A loss on the LABEL channels of the node estimate (the
 * first Cl = node_chans <= C_node - 4 channels of a row; the box comes last, as in dsg_decode / dsg_encode) and on the adjacency
 * estimate, a soft minimum over all node slots so that the caller picks none.  Graph b has K = n_items items; item k is three targets in
 * value space (dsg_encode's codes: s_k [Cl] the subject's label, o_k [Cl] the object's, p_k [C_adj] the predicate) and three weights
 * a_s, a_o, a_p >= 0; all three 0: the item is inactive.  With Dn = D_node[..., :Cl], Da = D_adj (the estimate the guide is handed: after
 * the valid mask and the known select; gt in the sanity-check mode) and the sums over the live ordered pairs (i, j), i != j, both nodes
 * valid, P of them:
 *     d_k(i,j) = a_s sum_c (Dn[i,c] - s_k[c])^2 + a_o sum_c (Dn[j,c] - o_k[c])^2 + a_p sum_c (Da[c,i,j] - p_k[c])^2
 *     L_k      = -tau log((1/P) sum_(i,j) exp(-d_k(i,j) / tau))          (max-subtracted; min d_k <= L_k <= min d_k + tau log P)
 *     L        = sum_k L_k                                                (a graph with P = 0 contributes exactly 0 and a zero gradient)
 *     pi_k     = softmax over the live pairs of -d_k / tau
 *     g_adj[c,i,j] = sum_k pi_k(i,j) 2 a_p (Da[c,i,j] - p_k[c])
 *     g_node[i,c]  = sum_k (sum_j pi_k(i,j)) 2 a_s (Dn[i,c] - s_k[c]) + (sum_j pi_k(j,i)) 2 a_o (Dn[i,c] - o_k[c])     (c < Cl, else 0)
 * a_o = a_p = 0 is "some node has this label", a_s = a_o = 0 "some pair carries this predicate".  Everything is evaluated in float64
 * from the float32 inputs and rounded once; fixed-order sums, no atomics, nothing depends on B.  Then, with c_i of dsg_guide_coef (the
 * schedule weights stay in guide->weights),
 *     shift = (c_i * w_content) g, zero at entries whose mask_adj / mask_node bit is set (known entries win and stay bit-exact), at padded
 *             rows and columns, on the adjacency diagonal and at node channels >= Cl
 *     f_b   = the content shift's OWN clip factor: dsg_guide_cfg's form on the same ||x_hat_b - D_b||, against content->clip_ratio
 *     D~    = D - f_b shift
 * Box channels and label channels are disjoint: the box shift and the content shift never meet in one entry, and the two families are
 * clipped independently.  Padded rows and columns and the diagonal are chosen by selects and never read.  The network's Jacobian is
 * dropped as in dsg_sample_guided: an approximation, and nothing is claimed about sample quality.
 *   subj / obj [B,K,Cl], pred [B,K,C_adj], w_spo [B,K,3] (a_s, a_o, a_p): HOST, so that they can be checked; copied into workspace
 *   memory on `stream` ahead of the run's synchronise (dsg_workspace_bytes counts the buffers once allocated). */
#define DSG_CONTENT_MAX_ITEMS 16
typedef struct dsg_content_cfg {
    float w_content;      /* weight of L_content; 0: the term is off */
    float tau;            /* > 0 */
    float clip_ratio;     /* >= 0, or DSG_GUIDE_CLIP_NONE */
    int32_t n_items;      /* K, 1..DSG_CONTENT_MAX_ITEMS */
    int32_t node_chans;   /* Cl, 1..C_node-4 */
    int32_t reserved;     /* 0 */
    const float *subj;    /* HOST [B,K,Cl] */
    const float *obj;     /* HOST [B,K,Cl] */
    const float *pred;    /* HOST [B,K,C_adj] */
    const float *w_spo;   /* HOST [B,K,3] (a_s,a_o,a_p), finite, >= 0 */
} dsg_content_cfg;

/* dsg_sample_guided_rel with the content term.  content == NULL or content->w_content == 0: dsg_sample_guided_rel itself -- the same plan
 * keys, the same captured bodies, the same bits.  Otherwise the content kernel runs behind every preconditioned call next to the box
 * guide, in step bodies of their own, and the updates read both shifts.  content_trace: DEVICE [L,B] or NULL -- L_content(D) of the
 * stage-1 call of every executed step.  A content-only run passes a guide whose loss weights are all 0.
 * Refused with DSG_ERR_INVALID before anything is launched, the message naming the argument: a non-finite w_content, tau <= 0 or NaN, a
 * negative or NaN clip_ratio, n_items or node_chans out of range, a null array, a non-finite target, a negative or non-finite weight,
 * N > 64, and everything dsg_sample_guided_rel refuses. */
int dsg_sample_guided_content(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_walk_cfg *walk /* NULL: trivial walk */,
                              int32_t B, const uint8_t *flags,
                              const uint64_t *graph_seeds /* host, [B], or NULL */, uint64_t coin_seed,
                              const float *init_adj, const float *init_node, const float *base_adj, const float *base_node,
                              const float *noise_adj, const float *noise_node, const uint8_t *coins,
                              const float *known_adj, const float *known_node, const uint8_t *mask_adj, const uint8_t *mask_node,
                              const int32_t *snap_steps, int32_t n_snap, float *snap_adj, float *snap_node,
                              const dsg_guide_cfg *guide, const float *gt_adj, const float *gt_node, float *loss_trace,
                              float *out_adj, float *out_node, dsg_sample_stats *stats, void *stream, const dsg_rel_cfg *rel,
                              const dsg_content_cfg *content, float *content_trace /* DEVICE [L,B] or NULL */);

/* sigma_steps (fp64, edm.py:84-88) and the fp32 per-step scalars the loop uses; out arrays of
 * length num_steps.  Host-only helper, exposed so bindings/tests can inspect the schedule. */
int dsg_sigma_schedule(const dsg_sampler_cfg *cfg, double *sigma_steps, float *t_hat, float *noise_coef,
                       float *h_step);

/* Kernel selection.  One entry per option, in the order of the library's table (dsg_option_info below); "env": the DSG_* environment
 * variable that replaces the default of every handle created in the process -- read as a flag (first character not '0') unless the
 * entry says integer, and brought into the option's range like a value passed here.  A flag option stores value != 0.
 * The narrow levels (C = 96 / 192) have register-resident fused kernels; each can be switched off to fall back to the generic GEMM +
 * attention + row-kernel path (all combinations are parity-tested):
 *   "fused_attn" (default 1; env DSG_FUSED_ATTN): the C = 96 attention block.
 *   "fused_mlp" (default 1; env DSG_FUSED_MLP): the fused MLP, at widths up to
 *   "fused_mlp_maxc" (96 | 192, default 96, stored as given; env DSG_FUSED_MLP_MAXC, integer).
 *   "fused_readout" (default 1; env DSG_FUSED_READOUT).
 *   "fused_patch_embed" (default 1; env DSG_FUSED_PE).
 *   "fused_rowstats" (default 1; env DSG_FUSED_ROWSTATS): modulate+SiLU and LayerNorm statistics in the producing GEMM's epilogue instead
 *       of row kernels.
 *   "fused_qkv_attn" (default 1; env DSG_FUSED_QKV_ATTN): 8x8 / 10x10 windows: QKV projection + window attention in one kernel, q/k/v
 *       never reach HBM.
 *   "fused_merge" (0..2, default 1; env DSG_FUSED_MERGE): PatchMerging's 2x2 gather + LayerNorm(4C) inside the reduction GEMM's A path;
 *       1: where it pays (>= 8192 merged rows), 2 (or more): at every size, 0: merge_ln kernel.
 *   "loop_graph" (default 1; env DSG_LOOP_GRAPH): the reverse loop -- 1: dsg_sample replays one captured hipGraph per step (a handful of
 *       distinct step bodies: first / steady / last step x the two self-conditioning coins); 0: the round-1 scheme, only the network
 *       forward is a graph.
 *   "prune_masked" (default 1; env DSG_PRUNE_MASKED): the up path computes only rows / windows that can reach an unmasked output (the
 *       lists: the need-list hook of dsg_debug.h); 0: every row.  Bit-identical results either way.
 *   "dedup_masked" (default 1; env DSG_DEDUP_MASKED; acts in the sampler entry points only, and only where "prune_masked" does): a
 *       graph's level-0 windows that hold nothing but padded pairs are computed once through PatchEmbed and the first Swin block and
 *       copied (the lists: the dedup-list hooks of dsg_debug.h); 0: every window is computed.  Bit-identical results either way.
 *   "dedup_levels" (>= 0, default 0 = every qualifying level; env DSG_DEDUP_LEVELS, integer): how many levels "dedup_masked" may reach, the finest
 *       included; 1: PatchEmbed and level 0's first block only.  Level k >= 1 qualifies when level k - 1 does and has no second
 *       (shifted) block, its own first block is unshifted on at least 2 x 2 windows of 8 x 8, and the PatchMerging into it is the partial-statistics form ("fused_merge" where
 *       it applies: 8192 merged rows, or value 2, or "batch_invariant"): that merge then computes only the merged rows of the level's
 *       unique windows, the first block runs over the same lists, and a copy fills the other pure windows of the activation, of the
 *       skip tensor and of the row statistics (the per-level dedup-list hook of dsg_debug.h).  dsg_get_option reports the number of levels that
 *       deduplicate under the present options (0: none).  Bit-identical results whatever the value.
 *   "dedup_batch" (0..2, default 1; env DSG_DEDUP_BATCH, integer; acts in the sampler entry points only, where sigma -- and with it every block's
 *       (scale, shift) row -- is the same for the whole batch): the pure windows of ALL graphs of a batch share one computed
 *       representative per level, the batch's first pure window, and a level below the top of the chain fills only the pure windows
 *       that a unique window of the next level lies over (nothing reads the others).  0: one representative per graph.  1: across the
 *       batch from 16 graphs on, per graph below -- below 16 graphs no list launch of the N = 64 network's down path exceeds half a
 *       round of resident GEMM tiles, so fewer rows buy no time there.  2: across the batch at every size.  dsg_denoise / dsg_precond
 *       (per-sample noise labels, caller tensors) list every window as unique whatever the value.  dsg_get_option reports the value in
 *       force (0 wherever "dedup_masked" is off).  The captured step bodies are the same for every value, so changing the option
 *       keeps them.  Bit-identical results whatever the value.
 *   "dedup_table" (default 1; env DSG_DEDUP_TABLE; acts only where "dedup_batch" shares one representative across the batch): that
 *       window's rows depend on the weights and on the step's (scale, shift) row only, so a sampler call computes them once per
 *       schedule index before its loop -- with the down path itself, on all-padding pseudo-batches of B indices -- into a table in the
 *       workspace (per index and level 64 rows of the activation, of the skip tensor and their row statistics; VG shape: about 330 KB
 *       per index, counted by dsg_workspace_bytes once built), and the fill writes the window from the entry of the running step like
 *       every other pure window; no launch of the loop computes it.  0: the batch's first pure window is computed in every forward.
 *       The captured step bodies are the same for both values (a device-side word written with the lists selects the fill's source),
 *       so changing the option keeps them.  dsg_get_option reports whether it would act.  Bit-identical results either way.
 *   "dedup_qkv" (0..2, default 1; env DSG_DEDUP_QKV gives 0 or 1; acts only where "dedup_masked" does): the shifted block right behind a
 *       deduplicated first block projects QKV of the copied pure-window rows once (the lists: the dedup-QKV hook of dsg_debug.h); 2, a
 *       measurement hook: the split form wherever the lists exist, whatever their share; 0: the fused form everywhere.  Changing it
 *       drops the captured graphs.  Bit-identical results whatever the value.
 *   "batch_invariant" (default 0): 1 -- every choice the plan makes (which kernel, which tile, fused or not, any summation order) is a
 *       function of the network geometry and the other options only, never of the batch size: PatchMerging is fused wherever "fused_merge"
 *       is on, at every size, and the bf16 GEMM of the "gemm_bf16" / bf16_pipe = 0 path keeps its 128 x 96 tile.  A sample's result then
 *       does not depend on B or on its position.  A geometry whose fused read-out would place a graph's pooling partials by
 *       its position (N * N not a multiple of 32) is refused with DSG_ERR_INVALID.  Holds on the default fp32 path and under "gemm_bf16";
 *       not under "gemm_split", whose kernel orders a row's partial products by the row's index mod 64.  0: the previous behaviour, bit for bit.
 * Precision modes (default: exact fp32 MFMA everywhere):
 *   "gemm_bf16" (default 0; env DSG_GEMM_BF16) = 1: the block/merge/breakup GEMMs on bf16 MFMA with operands rounded to bf16 (activations,
 *       LayerNorm, softmax and the sampler stay fp32) -- BASELINE config 5; parity against the fp32 oracle then holds to 1.5e-2 RMS /
 *       5e-2 max-abs of the output scale, not 1e-4.  "gemm_split" takes precedence if both are set (dsg_get_option then reports 0).
 *   "gemm_split" (default 0; env DSG_GEMM_SPLIT) = 1: every GEMM as six bf16-MFMA partial products of hi/mid/lo (3 x bf16 = 24-bit)
 *       operand splits with fp32 accumulation -- fp32-level accuracy, the 1e-4 parity bar still holds; 1.3-1.6x faster GEMMs (power-bound).
 *   "bf16_act" (0 / 1 / 2, default 2; acts only with "gemm_bf16"): 1 -- tensors whose only consumer is the bf16 GEMM (the MLP's
 *       hidden activations, the attention output) are stored as bf16 by their producer; the consumer rounds its A operand to bf16
 *       anyway, so results are bit-identical to 0, with half the bytes and no conversion in the consumer.  2 -- q, k, v are
 *       stored as bf16 as well; the attention arithmetic stays fp32 on the widened values, results move within the mode's bar.
 *   "bf16_pipe" (default 1; env DSG_BF16_PIPE; acts only with "gemm_bf16"): the bf16 block pipeline -- a Swin block is two kernels with
 *       bf16 tensors between them; its kernel choices (all parity-tested, same bar) are the four options below, reported as 0 wherever
 *       the pipeline does not run:
 *   "bf16_mlp" (0..6, default 1; env DSG_BF16_MLP, integer): 1 fused fc1-GELU-fc2 (C = 384: eight waves, weight images streamed by
 *       LDS-DMA), 4 round 3's eight-wave kernel, 5 the one-wave-per-SIMD LDS-DMA kernel, 6 = 1 with level 0 on the LDS-resident kernel,
 *       2 four waves at every width, 3 GEMM pair at C = 384, 0 GEMM pairs.
 *   "bf16_qkv_attn" (0..3, default 1; env DSG_BF16_QA, integer): 1 QKV projection + window attention in one kernel (10 x 10 windows: one
 *       wave per (window, head)), 2 the block-per-head kernel everywhere, 3 the former only where a block of four units lies in one
 *       window, 0 GEMM + attention kernel.
 *   "bf16_proj_mlp" (default 1): 1 proj + residual + LayerNorm-2 in front of the MLP kernel.
 *   "bf16_readout" (default 1): 1 the read-out on the bf16 pipe.
 * Test only:
 *   "debug_alloc_fill" (0..4, default 0; any other value is refused with DSG_ERR_INVALID): while p = 1..4, every scratch buffer the
 *       handle or a workspace allocates from then on is filled with pattern p (the patterns of the poison hook, dsg_debug.h) right after its allocation, ahead of
 *       the library's own creation memsets -- a stand-in for whatever the allocator returns.  Index / state buffers and weights are
 *       never filled.  No launch of any entry point changes.
 * Except for "dedup_batch", "dedup_table" and "debug_alloc_fill", setting an option drops the captured graphs and, once the weights are
 * finalized, checks every batch size in use against the kernels the new selection launches: if one is not covered the whole option set
 * stays as it was and the call returns DSG_ERR_INVALID with the layer / shape in dsg_last_error. */
int dsg_set_option(dsg_handle h, const char *name, int32_t value);
/* The value an option currently has on this handle (what the next forward will run with), whichever way it was set
 * (dsg_set_option or a DSG_* environment default): measurement code reports the precision mode from here. */
int dsg_get_option(dsg_handle h, const char *name, int32_t *value);
/* Row `index` (0, 1, ...) of the option table, without a handle or a device: the option's name, its environment variable (NULL: none),
 * its default and the range lo..hi that values are brought into (flags: 0..1).  Any out pointer may be NULL.  DSG_ERR_INVALID past
 * the end of the table. */
int dsg_option_info(int32_t index, const char **name, const char **env, int32_t *dflt, int32_t *lo, int32_t *hi);

/* On-device post-decode of the samples (sampler_node_adj.py:222-285) for the reference's three attribute encodings
 * (`--edge_encoding` / `--node_encoding`; R/utils/attribute_code.py:13 attribute_converter(..., out_encoding='int')):
 *   DSG_ENC_BITS     clamp(-1,1) -> > 0 -> MSB-first integer (bin2dec, :319) -> clamp to [0, n_type-1]
 *   DSG_ENC_ONE_HOT  clamp -> +-1 threshold at 0 -> argmax over the channels (:212-237): the first positive channel, 0 if none
 *   DSG_ENC_DDPM     clamp -> the class whose interval (lo_i, hi_i] of width 2/(n_type-1) around -1 + 2i/(n_type-1) holds the
 *                    value (:121-177; the reference's double-precision thresholds compared in fp32), -1 for NaN
 * Rows / columns of padded nodes and the adjacency diagonal are 0.  adj [B,C_adj,N,N] (C_adj = bits | n_adj_type | 1), node
 * [B,N,C_node]: the first node_chans channels are the attribute (bits | n_node_type | 1), the last four the bounding box when
 * out_bbox != NULL (-> *0.5+0.5, masked; :201-209).  Needs the handle only for N / C_adj / C_node (no weights). */
enum { DSG_ENC_BITS = 0, DSG_ENC_ONE_HOT = 1, DSG_ENC_DDPM = 2 };
int dsg_decode(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, int32_t edge_encoding,
               int32_t node_encoding, int32_t n_adj_type, int32_t n_node_type, int32_t node_chans,
               int32_t *out_adj /*[B,N,N]*/, int32_t *out_node /*[B,N]*/, float *out_bbox /*[B,N,4] or NULL*/, void *stream);
/* dsg_decode with both encodings 'bits' (the README's recipe) */
int dsg_decode_bits(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags,
                    int32_t n_adj_type, int32_t n_node_type, int32_t node_bits,
                    int32_t *out_adj /*[B,N,N]*/, int32_t *out_node /*[B,N]*/, float *out_bbox /*[B,N,4] or NULL*/,
                    void *stream);

/* The inverse of dsg_decode: integer graphs -> the network's value space, the on-device attribute_converter(in_encoding = 'int',
 * out_encoding = ...) (R/utils/attribute_code.py:240-304) -- what dsg_sample_known takes as known_adj / known_node:
 *   DSG_ENC_BITS     MSB-first binary digits (dec2bin, :307) -> 2 b - 1
 *   DSG_ENC_ONE_HOT  2 onehot - 1 over the n_type channels
 *   DSG_ENC_DDPM     2 i / (n_type - 1) - 1, float32 op by op like the reference's tensor arithmetic
 * q_adj [B,N,N], q_node [B,N] int32 in [0, n_type - 1]; bbox [B,N,4] fp32 in [0,1] or NULL.  out_adj [B,C_adj,N,N]; out_node [B,N,C_node]:
 * the attribute in the first node_chans channels, (bbox - 0.5) * 2 (R/utils/dataloader.py:168) in the last four when bbox != NULL, 0 in
 * any channel in between.  Rows / columns of padded nodes are 0; the adjacency diagonal is encoded like every other entry (the
 * reference masks with the node flags only).  Channel counts are checked like dsg_decode's.  Needs the handle only for N / C_adj /
 * C_node (no weights). */
int dsg_encode(dsg_handle h, int32_t B, const int32_t *q_adj, const int32_t *q_node, const float *bbox /*[B,N,4] or NULL*/,
               const uint8_t *flags, int32_t edge_encoding, int32_t node_encoding, int32_t n_adj_type, int32_t n_node_type,
               int32_t node_chans, float *out_adj /*[B,C_adj,N,N]*/, float *out_node /*[B,N,C_node]*/, void *stream);

/* The noise-conditioning path on its own (test / inspection hook for SURVEY fixture G1): PositionalEmbedding -> map_layer0/1 with
 * SiLU (R/model/diffusesg/diffusesg.py:507-513, :768-771) -> every `affine` linear (:238, :574) for `rows` noise labels c_noise
 * (device, [rows]).  out_pe [rows, embed_dim], out_emb [rows, 512], out_aff [rows, dsg_affine_width(h)] (any may be NULL):
 * (scale | shift) of patch_embed, then of down_layers[l].blocks[j], then of up_layers[i].blocks[j] -- the table dsg_sample builds
 * once per call for all its steps. */
int dsg_noise_embed(dsg_handle h, int32_t rows, const float *c_noise, float *out_pe, float *out_emb, float *out_aff, void *stream);
int32_t dsg_affine_width(dsg_handle h);

/* ---- a training iteration: objective, loss, loss backward (no handle: these only need the tensor dimensions), then
 * the network in training form with its backward, the optimiser step and the EMA update further down.
 * Return DSG_OK / DSG_ERR_INVALID / DSG_ERR_HIP.
 *
 * dsg_train_inputs <-> NodeAdjEDMObjectiveGenerator.get_input_output   R/runner/objectives/edm.py:160-180, :239-281
 *   (precond = sigma_dist = 'edm', symmetric_noise = False: learning_utils.py:25-29)
 *   sigma_b = exp(rnd_b*1.2 - 1.2); weight_b = (sigma^2 + 0.25)/(0.5 sigma)^2;
 *   noisy_adj = mask(clean_adj + eps_adj*sigma_b); noisy_node = clean_node + mask(eps_node*sigma_b)
 *   rnd_sigma [B] / eps_adj / eps_node: the N(0,1) draws (device pointers) or NULL = the library's Philox streams of `seed`. */
int dsg_train_inputs(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *clean_adj, const float *clean_node,
                     const uint8_t *flags, const float *rnd_sigma, const float *eps_adj, const float *eps_node, uint64_t seed,
                     float *out_sigmas, float *out_weights, float *out_noisy_adj, float *out_noisy_node, void *stream);
/* iou_loss_type of the trainer's bounding-box term (R/runner/trainer/trainer_node_adj.py:138-153; `--iou_loss_type`, the reference's
 * README trains with 'giou', its YAMLs default to 'iou'): 'iou' = -(torchvision.ops.box_iou)^2; the others are torchvision.ops'
 * generalized_ / distance_ / complete_box_iou_loss(reduction='none') ('giou_squared' squares the first).  torchvision is an
 * un-vendored dependency of the reference and absent from this image: those four are restated from its published algorithm. */
enum { DSG_IOU_IOU = 0, DSG_IOU_GIOU = 1, DSG_IOU_GIOU_SQUARED = 2, DSG_IOU_DIOU = 3, DSG_IOU_CIOU = 4 };
/* dsg_rainbow_loss <-> NodeAdjRainbowLoss.forward(reduction='none')    R/loss/rainbow_loss.py:37-101
 *   plus the trainer's bounding-box term (iou_loss_type: DSG_IOU_*)    R/runner/trainer/trainer_node_adj.py:130-159
 *   (last four node channels; weight 0 switches it off).  Outputs: per-sample losses [B]; the step's scalar loss is
 *   mean(out_loss_adj) + mean(out_loss_node) (trainer_node_adj.py:167). */
int dsg_rainbow_loss(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *pred_adj, const float *pred_node,
                     const float *target_adj, const float *target_node, const uint8_t *flags, const float *loss_weight,
                     float edge_loss_weight, float node_loss_weight, float iou_loss_weight, int32_t iou_loss_type, float *out_loss_adj,
                     float *out_loss_node, void *stream);
/* dsg_rainbow_loss_backward: first stage of loss.backward() of a training step   R/runner/trainer/trainer_node_adj.py:163-170
 *   loss = mean_b(loss_adj) + mean_b(loss_node) with the terms of dsg_rainbow_loss (IoU term through autograd's clamp / max / min
 *   rules).  out_grad_* = dL/d(preconditioned outputs), layouts of pred_*.  With sigmas [B] (may be NULL) also
 *   out_grad_F_* = dL/d(raw network outputs F) = c_out(sigma_b) * out_grad_*   (D = mask(c_skip x + c_out F), precond.py:101-104).
 *   (dsg_train_step_grads chains this with the network's own backward.) */
int dsg_rainbow_loss_backward(int32_t B, int32_t N, int32_t c_adj, int32_t c_node, const float *pred_adj, const float *pred_node,
                              const float *target_adj, const float *target_node, const uint8_t *flags, const float *loss_weight,
                              float edge_loss_weight, float node_loss_weight, float iou_loss_weight, int32_t iou_loss_type,
                              const float *sigmas, float *out_grad_adj, float *out_grad_node, float *out_grad_F_adj, float *out_grad_F_node,
                              void *stream);

/* One SwinTransformerBlock in training form: forward x_out = block(x_in, emb) (R/model/diffusesg/diffusesg.py:232-277 with
 * WindowAttention :108-139 and Mlp :19-25) and, when grad_out != NULL, its backward as torch.autograd derives it -- the first
 * building block of the network backward.  Kernels: csrc/train_kernels.hip -- products, weight gradients and the
 * attention forward / backward on fp32 MFMA, row passes HBM-bound; pinned to the reference's autograd by tests/golden/block_backward.npz.
 *   block: state-dict prefix of the block, e.g. "down_layers.0.blocks.1".  x_in, x_out, grad_out, grad_in: [B, T, C] token-major
 *   (the reference's [B, L, C]); emb, grad_emb: [B, 512] (the mapped noise embedding, dsg_noise_embed).  names[i] (relative to the
 *   prefix: "affine.weight", "affine.bias", "norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.qkv.weight",
 *   "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
 *   "mlp.fc2.weight", "mlp.fc2.bias") -> grad_params[i] (device, the parameter's shape); all 15 are required with grad_out. */
int dsg_block_train(dsg_handle h, const char *block, int32_t B, const float *x_in, const float *emb, const float *grad_out, float *x_out,
                    float *grad_in, float *grad_emb, int32_t n_params, const char *const *names, float *const *grad_params, void *stream);

/* The whole network in training form: F = DiffuseSG.forward(in_adj, in_node, flags, c_noise, sc_adj, sc_node)
 * (R/model/diffusesg/diffusesg.py:765-830) and, when grad_F_adj != NULL, the gradient of every parameter for the upstream gradients
 * dL/dF (e.g. from dsg_rainbow_loss_backward) -- what loss.backward() of a training step leaves in the parameters' .grad
 * (R/runner/trainer/trainer_node_adj.py:163-170), pinned by tests/golden/train_backward.npz.  MFMA products, weight gradients
 * and attention since round 3 (csrc/train_kernels.hip; measured rates: DESIGN.md §4).  dsg_finalize_weights must have run once; weights
 * set afterwards (an optimiser step) are used as they are -- the training form reads the raw tensors only.
 *   in_adj [B,C_adj,N,N], in_node [B,N,C_node]: the preconditioned inputs c_in(sigma) * noisy (precond.py:100); c_noise [B];
 *   sc_*: the self-conditioning inputs (constants: the reference detaches them) or NULL; out_F_*: the raw network outputs;
 *   names[i] (state-dict keys of all parameters) -> grad_params[i] (device buffers of the parameters' shapes, overwritten).
 *   Like every entry that takes a stream, the work is only ENQUEUED when the call returns (round 2 synchronised at the end of this one). */
int dsg_train_grads(dsg_handle h, int32_t B, const float *in_adj, const float *in_node, const uint8_t *flags, const float *c_noise,
                    const float *sc_adj, const float *sc_node, const float *grad_F_adj, const float *grad_F_node, float *out_F_adj,
                    float *out_F_node, int32_t n_params, const char *const *names, float *const *grad_params, void *stream);

/* One training iteration up to and including loss.backward() (R/runner/trainer/trainer_node_adj.py:96-170, 'edm' objective):
 * D = NodeAdjPrecond(noisy, sigmas) with the network in training form, per-sample losses as dsg_rainbow_loss, and -- when the gradient
 * buffers are given -- the gradient of  loss_adj.mean() + loss_node.mean()  for every parameter.  sc_*: the detached self-conditioning
 * inputs (precond.py:90-98; the Python mirror draws the coin and computes them with dsg_precond) or NULL.  The caller supplies the
 * objective's tensors (dsg_train_inputs); dsg_adam_step / dsg_ema_update below finish the iteration, gradient averaging across
 * ranks is the host's (diffusesg_amd.dist.all_reduce_mean over RCCL). */
int dsg_train_step_grads(dsg_handle h, int32_t B, const float *noisy_adj, const float *noisy_node, const uint8_t *flags, const float *sigmas,
                         const float *sc_adj, const float *sc_node, const float *target_adj, const float *target_node,
                         const float *loss_weight, float edge_loss_weight, float node_loss_weight, float iou_loss_weight,
                         int32_t iou_loss_type, float *out_D_adj, float *out_D_node, float *out_loss_adj, float *out_loss_node,
                         int32_t n_params, const char *const *names, float *const *grad_params, void *stream);

/* The no-grad pass of a self-conditioning training step (precond.py:92-98): D = NodeAdjPrecond(noisy, sigmas) with NO self-conditioning
 * input, computed by the network in TRAINING form -- i.e. from the raw parameters (dsg_train_bind_params / dsg_set_weight), without the
 * sampling path's derived weights, which an optimiser step invalidates (dsg_finalize_weights costs several forwards).  out_sc_* are the
 * masked D tensors the caller then passes to dsg_train_step_grads as sc_adj / sc_node. */
int dsg_train_self_cond(dsg_handle h, int32_t B, const float *noisy_adj, const float *noisy_node, const uint8_t *flags, const float *sigmas,
                        float *out_sc_adj, float *out_sc_node, void *stream);

/* Vector-Jacobian product of the preconditioned denoiser with respect to its noisy input: D = NodeAdjPrecond.forward(adj, node, sigmas)
 * with the network in training form (fp32 whatever the precision options; the bits dsg_train_self_cond gives when sc is NULL), then
 * out_grad_adj = dL/d adj [B,C_adj,N,N] and out_grad_node = dL/d node [B,N,C_node] for the cotangent g = dL/dD.  sc_adj / sc_node: the
 * self-conditioning inputs, constants (not differentiated; both or NULL); sigma is not differentiated either.  The backward runs
 * without any weight-gradient product.  The adjacency gradient at padded pairs is NOT zero (the network reads the unmasked adjacency
 * input); the node gradient of padded nodes is.
 * g is either given (grad_D_adj / grad_D_node, device, D's layouts: a cotangent that does not depend on D) or produced by `fn`, which
 * is called once between the forward and the backward: D_* are out_D_* (already enqueued on `stream`), and the callee ENQUEUES work on
 * the same stream that fills g_* (device, D's layouts; they are out_grad_*, used as staging and overwritten with the result).  A nonzero
 * return aborts the call before any backward launch: DSG_ERR_INVALID.  Exactly one of fn and grad_D_* must be given (DSG_ERR_INVALID
 * otherwise).  DSG_ERR_STATE before dsg_finalize_weights.  The work is only enqueued; arena and scratch are the training entries'. */
typedef int (*dsg_grad_fn)(void *user, const float *D_adj, const float *D_node, float *g_adj, float *g_node);
int dsg_precond_vjp(dsg_handle h, int32_t B, const float *adj, const float *node, const uint8_t *flags, const float *sigmas /*[B]*/,
                    const float *sc_adj, const float *sc_node, const float *grad_D_adj, const float *grad_D_node, dsg_grad_fn fn, void *user,
                    float *out_D_adj, float *out_D_node, float *out_grad_adj, float *out_grad_node, void *stream);

/* ---- Probability-flow ODE between the noise levels: the latent of a graph, and its log-likelihood under the model.
 * Levels: t_0 > ... > t_{T-1}, the t_hat of dsg_sigma_schedule for a cfg whose schedule draws no noise (any nonzero noise_coef:
 *   DSG_ERR_INVALID, as for the dpmpp_2m solver -- use S_churn = 0).  T >= 2.  t_max = t_0, t_min = t_{T-1}, sigma_d = 0.5.
 * Velocity: f(x, t) = mask((x - D(x, t)) / t), D the TRAINING-FORM preconditioned denoiser with the self-conditioning inputs NULL -- the
 *   bits dsg_train_self_cond gives.  That holds for a network built with self_condition = 1 as well: the ODE is defined on the branch
 *   without self-conditioning.
 * Directions: DSG_ODE_ENCODE steps from a = t_k to b = t_{k-1}, k = T-1 ... 1 (data at t_min -> latent at t_max); DSG_ODE_DECODE from
 *   a = t_k to b = t_{k+1}, k = 0 ... T-2, and ends at t_min: there is no step to 0.  h = b - a (fp32).
 * Solvers (cfg->heun): DSG_SOLVER_EULER x_b = x_a + h f(x_a, a), T-1 evaluations; DSG_SOLVER_HEUN -- here the true trapezoid, not the
 *   sampler's form -- x' = x_a + h f(x_a, a), x_b = x_a + (h/2)(f(x_a, a) + f(x', b)), 2(T-1) evaluations; DSG_SOLVER_DPMPP_2M:
 *   DSG_ERR_INVALID.  The state arithmetic is the sampler's Euler / Heun element operations, fp32 op by op, on a step table of these
 *   (a, b) pairs.
 * Probe (Hutchinson's estimator of the divergence): one eps per graph, fixed for the whole run, zero at padded entries.  Recorded
 *   (probe_adj / probe_node, device, D's layouts; masked on the way in; they win over graph_seeds) or drawn on the device from
 *   graph_seeds (HOST, [B]): DSG_ODE_PROBE_GAUSSIAN is exactly dsg_gen_noise_seeded(graph_seeds, noise_stream = DSG_ODE_PROBE_STREAM),
 *   DSG_ODE_PROBE_RADEMACHER is +1 where that draw is >= 0 and -1 elsewhere.  The stream lies above every churn stream of a walk.
 * Net trace: at every evaluation (x, t), row k of out_net_trace (device, [n_evals, B] doubles) receives
 *       n_b = sum over the live entries j of graph b of eps_j (J_D^T eps - c_skip(t) eps)_j = c_in c_out eps^T J_F eps,
 *   c_skip = sigma_d^2 / (t^2 + sigma_d^2).  The c_skip term is never formed and subtracted (at t = 0.002 that would cancel seven
 *   digits): the assemble backward runs with a zero c_skip array and writes the network part alone.  The sum is float64, in one fixed
 *   order, over live entries selected by the flags (the adjacency gradient at padded pairs is not zero).
 * Log-likelihood (assembled by the caller in float64; diffusesg_amd.ode.assemble_logp): with d_b = C_adj n_b^2 + C_node n_b live
 *   entries, x_max / x_min the states at t_max / t_min (whichever is input and whichever output), and w_k of dsg_ode_evals,
 *       log p_{t_min}(x_min) = -(d/2) ln(2 pi t_max^2) - |x_max|^2 / (2 t_max^2) + (d/2) ln((t_max^2 + sigma_d^2) / (t_min^2 + sigma_d^2))
 *                              - sum_k w_k n_k.
 *   The term d t / (t^2 + sigma_d^2) of the divergence is integrated in closed form (the third term); only the network part is
 *   integrated numerically, by the solver's own quadrature.  The prior is the sampler's N(0, t_max^2 I); for data N(0, s^2 I) the
 *   expression equals log N(x; 0, (s^2 + t_min^2) I) up to (d/2) ln(t_max^2 / (s^2 + t_max^2)), the known prior mismatch.  A graph
 *   with no valid node: latent 0, traces 0, log p = 0.
 * dsg_ode_run: x_* the state at the start level, out_* the state at the end level; out_probe_* (optional, both or none) the probe
 *   used; out_net_trace required iff probe != DSG_ODE_PROBE_NONE.  With probe = NONE no backward runs and the end state is bit-identical
 *   to the run with a probe.  With the option "batch_invariant" a graph's end state and traces are the same bits alone or in a batch.
 *   Refused before anything is launched: the above, what dsg_precond_vjp refuses (C_node beyond the assemble backward; DSG_ERR_STATE
 *   before dsg_finalize_weights), a probe with neither seeds nor recorded tensors, half a recorded probe, a missing out_net_trace.
 *   The run is enqueued on `stream` with one synchronisation, after the uploads of its tables and ahead of the first launch; buffers
 *   belong to the handle (the training entries' arena and scratch included) and are freed with it.
 * dsg_ode_evals: host-only, as dsg_walk_steps is.  Returns n_evals or a negative status: a refusal above, or cap < n_evals with
 *   an array given. t_eval [n_evals]: the evaluation levels in execution order; weight [n_evals]: w_k -- Euler |h|/a at its one
 *   evaluation, Heun |h|/(2a) at stage 1 and |h|/(2b) at stage 2 -- in double from the widened fp32 values.  Either may be NULL. */
#define DSG_ODE_ENCODE 0
#define DSG_ODE_DECODE 1
#define DSG_ODE_PROBE_NONE 0
#define DSG_ODE_PROBE_RADEMACHER 1
#define DSG_ODE_PROBE_GAUSSIAN 2
#define DSG_ODE_PROBE_STREAM 0x0DE00000u   /* > DSG_WALK_MAX_STEPS + 1: never a churn stream */
typedef struct dsg_ode_cfg {
    int32_t direction;                 /* DSG_ODE_ENCODE / DSG_ODE_DECODE */
    int32_t probe;                     /* DSG_ODE_PROBE_* */
    int32_t reserved[6];
} dsg_ode_cfg;
int dsg_ode_run(dsg_handle h, const dsg_sampler_cfg *cfg, const dsg_ode_cfg *ode, int32_t B, const uint8_t *flags,
                const float *x_adj, const float *x_node, const uint64_t *graph_seeds /* host [B] */,
                const float *probe_adj, const float *probe_node, float *out_adj, float *out_node,
                float *out_probe_adj, float *out_probe_node, double *out_net_trace /* device [n_evals, B] */, void *stream);
int32_t dsg_ode_evals(const dsg_sampler_cfg *cfg, const dsg_ode_cfg *ode, float *t_eval, double *weight, int32_t cap);

/* Let the training-form entries (dsg_train_grads, dsg_train_step_grads, dsg_train_self_cond) read these parameters IN PLACE: names[i]
 * (state-dict key) -> params[i] (device tensor of the parameter's shape, e.g. the tensor the optimiser updates), instead of the
 * handle's own copies -- no upload per iteration.  The caller keeps the tensors alive and unchanged in address until the next call of
 * this function; n_params = 0 clears the binding.  Keys not bound fall back to the handle's copy.  The sampling-path entries are not
 * affected: they use what dsg_set_weight + dsg_finalize_weights installed. */
int dsg_train_bind_params(dsg_handle h, int32_t n_params, const char *const *names, const float *const *params);

/* Precision of the training entries' large matrix products (mixed precision: fp32 master weights, fp32 accumulation, bf16 operands).
 * The mode is handle state, off by default, and acts on dsg_train_grads, dsg_train_step_grads and dsg_train_self_cond only;
 * dsg_precond_vjp, dsg_ode_run and every sampling entry are the same bits whatever it is.  Setting it enqueues nothing, invalidates
 * nothing and touches neither the options nor the packed weights.  It is not an option: no dsg_set_option key, no environment variable.
 * DSG_TRAIN_BF16: the three products of the four linears of every Swin block (attn.qkv, attn.proj, mlp.fc1, mlp.fc2), of
 *   downsample.reduction and of upsample.pre_linear / post_linear -- y = x W^T, dx = dy W, dW = dy^T x -- round both operands to bf16
 *   (nearest even), accumulate in fp32 on the bf16 matrix pipe and store fp32, wherever the product has at least 512 token rows and
 *   channel extents that are multiples of 32; a covered product of any other shape silently stays on its fp32 route.  db = colsum(dy)
 *   is formed from the unrounded fp32 dy.  Everything else stays fp32: PatchEmbed, the read-out chain and both heads, the noise
 *   embedding and every `affine` linear, window attention, LayerNorm / modulate / GELU, loss, all saved activations (the arena keeps
 *   its size), the gradient buffers, clip / Adam / EMA.  No loss scaling: bf16 has fp32's exponent range.
 *   The parameters are read in place and may change between calls, so every entry call in this mode re-rounds the covered weights into
 *   handle-owned bf16 planes (both orientations) before its first product; nothing is cached across calls.
 * dsg_train_set_precision: DSG_ERR_INVALID for any other value, the old mode kept.  Handles with patch_size > 1 accept the setter and
 *   keep refusing the training entries (with dsg_train_enable_patch on as well: the bf16 products are not built at patch_size > 1).  No trained weights exist for this model offline: nothing is claimed about the convergence or
 *   the quality of models trained in this mode. */
#define DSG_TRAIN_F32  0   /* default */
#define DSG_TRAIN_BF16 1
int dsg_train_set_precision(dsg_handle h, int32_t mode);
int dsg_train_get_precision(dsg_handle h, int32_t *mode);

/* The training form at patch_size > 1 (dsg_create_patch with p in {2, 4}): handle state, OFF by default -- a fresh handle refuses
 * dsg_train_grads, dsg_train_step_grads, dsg_train_self_cond, dsg_precond_vjp and dsg_ode_run as the first check of each entry, with a
 * message naming the entry, patch_size and this function.  on != 0 switches it on, 0 off again; accepted at any patch size and without
 * effect at patch_size 1 (the same bits either way).  Setting it enqueues nothing and touches neither the options nor the packed weights.
 * Once on, the five entries compute at p > 1 what they compute at p = 1, on R x R tokens (R = N / p): the raw weights are read in place
 * in the reference's layouts -- patch_embed.proj.weight [E, Cin, p, p], read_out.0.weight [E, E, p, p] ([in, out, a, b]) -- and packed
 * per call into weight images; their gradients arrive in those layouts; every mask is per pixel (flag_I && flag_J), the node mean is
 * over the N pixels of a row, exact zeros at masked entries of the outputs, of dL/dF and of the node gradient.
 * fp32 only: with dsg_train_set_precision(h, DSG_TRAIN_BF16) the five entries return DSG_ERR_INVALID with a message naming both
 * settings.  Still refused at p > 1 whatever this is: "gemm_split", "gemm_bf16", "batch_invariant"; pruning and deduplication stay off.
 * dsg_train_patch_enabled: the stored value (0 for a NULL handle). */
int dsg_train_enable_patch(dsg_handle h, int32_t on);
int32_t dsg_train_patch_enabled(dsg_handle h);

/* ---- Autoguidance (Karras et al. 2024, "Guiding a diffusion model with a bad version of itself") ----
 * A main handle h can have a second, weaker network -- the guide handle -- attached, with a scale s and a noise-level interval
 * [sigma_lo, sigma_hi].  While attached, a preconditioned call of h at (x, sigma, sc, coin) is the composite
 *     D_m = NodeAdjPrecond_h(x, sigma, sc, coin)      as without a guide, h's own extra self-conditioning pass included
 *     D_g = NodeAdjPrecond_guide(x, sigma, sc, coin)  the same x, sigma, sc and coin OUTCOME; the guide's extra pass is its own
 *     s_b = s where sigma_lo <= sigma_b <= sigma_hi, else 1
 *     D~  = fadd(D_m, fmul(s_b - 1, fsub(D_m, D_g)))  float32, one rounding per operation (s - 1 rounded once); exactly 0 at masked entries
 * and every D the reverse loop reads, stores or hands on is D~: both Heun stages, the multistep extrapolation, the next call's
 * self-conditioning input of BOTH networks, and the tensor the box / relation / content guide kernels are handed.  With known entries
 * the select runs on D_m and D_g, so a known entry arrives bit-exact.  This is what the reference's sampler computes when it is given
 * one nn.Module that wraps two NodeAdjPrecond and forces one coin per call on both.
 * Acts on dsg_precond (per-sample sigmas: the guide always runs, s_b is selected per sample) and on every dsg_sample* entry -- plain,
 * known, walk, seeded, guided, guided_rel, guided_content -- with all three solvers, step graphs on and off; the sanity-check mode
 * bypasses the denoiser and is unchanged.  In the loop sigma is batch-uniform: a step is guided iff the float32 t_hat of its schedule
 * index (dsg_sigma_schedule) lies in the interval; a step outside it, and every step of a run with s == 1, runs no guide forward at all
 * and replays the plain captured step body.  The guide's forwards are enqueued behind the main network's on the same stream.
 * Does NOT act on dsg_denoise, the training entries (dsg_train_*), dsg_precond_vjp or dsg_ode_run: they are the same bits attached or not.
 * The attachment is handle state (like dsg_train_set_precision): no option, no environment variable.
 * dsg_attach_guide: DSG_ERR_INVALID, nothing changed and nothing enqueued, the message naming the argument, for guide == h; a guide
 *   that has a guide of its own (or h being a guide, or the guide serving another handle); a guide that is not finalized; a different
 *   max_node_num, c_adj, c_node or self_condition; a handle created on another device; a scale that is not finite; a NaN bound or
 *   sigma_lo > sigma_hi (-INFINITY / INFINITY: every level).  Everything else may differ: embed_dim, depths, heads, window, patch_size,
 *   weights, options.  Attaching over an existing attachment replaces it.  An entry call whose option combination the guide cannot run
 *   (batch_invariant on a patch_size > 1 guide, ...) fails before anything is enqueued with the guide's own message behind "guide handle: ".
 * dsg_detach_guide: back to the plain handle (no guide attached: DSG_OK).  dsg_destroy of either handle detaches first.
 * dsg_guide_info: the attachment (guide NULL, scale 1, bounds 0 when there is none); any output pointer may be NULL.
 * dsg_guide_forwards: the GUIDE's network forwards in the last dsg_sample* call of h.  dsg_sample_stats keeps its layout and its
 *   counters keep counting the main network only.
 * Non-re-entrancy extends to the guide: while attached, the guide handle is busy whenever h is -- no call on the guide from another
 * thread or stream while a call on h runs; between calls of h the guide may be used on its own.
 * Nothing is claimed about sample quality: no trained weights exist for this model offline. */
int dsg_attach_guide(dsg_handle h, dsg_handle guide, float scale, float sigma_lo, float sigma_hi);
int dsg_detach_guide(dsg_handle h);
int dsg_guide_info(dsg_handle h, dsg_handle *guide, float *scale, float *sigma_lo, float *sigma_hi);
int dsg_guide_forwards(dsg_handle h, int64_t *n);

/* The rest of a training iteration (R/runner/trainer/trainer_node_adj.py:170-175), on caller-owned device tensors, no handle:
 * dsg_adam_step <-> nn.utils.clip_grad_norm_(parameters, max_norm) followed by torch.optim.Adam.step()  (utils/learning_utils.py:137-140:
 *   betas (0.9, 0.999), eps 1e-8, L2 weight_decay; gradients are scaled in place by the clip coefficient like the reference;
 *   `step` counts from 1; max_grad_norm <= 0 switches clipping off).  out_total_norm (host, may be NULL): the norm before clipping.
 * dsg_ema_update <-> ema_pytorch's EMA.update_moving_average: ema <- ema + (param - ema)(1 - decay).  ema_pytorch is an un-vendored,
 *   unpinned dependency of the reference (setup/requirements.txt:20) and absent here: parity unpinned; the decay schedule is restated
 *   from its published algorithm in diffusesg_amd/train.py::EMAHip. */
int dsg_adam_step(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                  const int64_t *numel, int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                  float *out_total_norm, void *stream);
int dsg_ema_update(int32_t n_tensors, float *const *ema, const float *const *params, const int64_t *numel, float decay, void *stream);

/* ---- Sample evaluation (no handle): the reference's SceneGraphEvaluator (R/evaluation/bbox_metrics.py), which
 * sg_go_sampling (R/runner/sampler/sampler_node_adj.py:446-600) and R/helper/eval_sg_samples.py run on the CPU after sampling.
 * Kernels: csrc/eval_kernels.hip; Python: diffusesg_amd/evaluate.py (SceneGraphEvaluatorHip); pinned by tests/golden/eval_metrics.npz.
 * Device pointers, caller's stream; all float64 sums run in a fixed order (repeated calls are bit-identical).
 *
 * Bounding-box F1 matrix (compute_bbox_f1 <-> measure_two_sets_of_bboxes, bbox_metrics.py:64-115):
 *   boxes [S, N, 4] fp32 x1 y1 x2 y2, classes [S, N] int32, flags [S, N] uint8.  A box counts when its flag is set and
 *   x1 >= 0, y1 >= 0, x2 > 0, y2 > 0 and 0 <= class < n_classes.  Generated and reference sets share N (pad with flag 0).
 *   QUIRK kept from the reference: each box is its own "image" named after its NODE INDEX (imageName = str(i)), so the generated
 *   box of node i can only match the reference box of node i, and only within one class; a pair of scenes is not matched up to a
 *   permutation of its nodes.  IoU is Pascal VOC's with "+1" areas, float32 op by op.
 *   weights: [W, n_classes] float64 class-weight table (W <= 8), or NULL for the unweighted mean (W must be 1 then); each pair
 *   normalises them over the union of both scenes' classes (a zero sum there gives NaN, as in the reference).
 * dsg_eval_bbox_prep: once per set, into `prep` (device, dsg_eval_bbox_prep_bytes(S, N, W) bytes); the same weights as the F1 call.
 * dsg_eval_bbox_f1: out[x - x0][y - y0][w] (float64, contiguous [x1-x0, y1-y0, W]) for generated scenes [x0, x1) x reference
 *   scenes [y0, y1); iou_thresholds: HOST array of n_iou (1..16) float64 thresholds (the reference's np.linspace(0.05, 0.5, 10)).
 *   N <= 255, n_classes <= 192. */
size_t dsg_eval_bbox_prep_bytes(int32_t S, int32_t N, int32_t W);
int dsg_eval_bbox_prep(int32_t S, int32_t N, int32_t n_classes, const float *boxes, const int32_t *classes, const uint8_t *flags,
                       int32_t W, const double *weights, void *prep, void *stream);
int dsg_eval_bbox_f1(const void *gen_prep, int32_t X, const void *ref_prep, int32_t Y, int32_t N, int32_t n_classes, int32_t W,
                     const double *weights, int32_t n_iou, const double *iou_thresholds, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                     double *out, void *stream);
/* Histograms for the Gaussian MMDs, written feature-major: hist[k * ld + b] (ld >= B), normalised by their sums as compute_mmd
 * does (mmd.py:152-153; a zero sum leaves the zeros), and sums[b] = the raw count.
 * dsg_eval_type_hist, edges = 0: node types 0..K-1 of the flagged nodes, types [B, N] (_get_node_type_hist, bbox_metrics.py:181-195),
 *   K rows.  edges = 1: edge types 1..K-1 over flagged x flagged entries (diagonal included), types [B, N, N]
 *   (_get_edge_type_hist, :197-216), K-1 rows; the caller drops graphs whose sum is 0.  A type equal to K counts as K-1
 *   (torch.histogram's closed last bin).  The float32 counts are normalised in float32, as the reference's are.  K <= 1024.
 * dsg_eval_degree_hist: adj [B, N, N] fp32; edge where adj[i,j] != 0 or adj[j,i] != 0, i != j; isolated nodes dropped, a graph
 *   without edges is one node of degree 0 (adjs_to_graphs + nx.degree_histogram, stats.py:23-60, 180-194); N rows (zero padding
 *   beyond the largest degree changes no distance).  N <= 1024.
 * dsg_eval_hist_mmd: Gaussian kernel exp(-|a-b|^2 / 2) in float64 (mmd.py:70-84): out[0] = disc(ref,ref) + disc(gen,gen)
 *   - 2 disc(ref,gen), out[1..3] = the three discs (means of the kernel over all pairs); ref [L][ld_ref], gen [L][ld_gen]
 *   (n_ref, n_gen >= 1, L <= 1024); ws: device scratch of 2 * n_ref + n_gen doubles. */
int dsg_eval_type_hist(int32_t B, int32_t N, int32_t K, int32_t edges, const int32_t *types, const uint8_t *flags, double *hist,
                       int32_t ld, double *sums, void *stream);
int dsg_eval_degree_hist(int32_t B, int32_t N, const float *adj, double *hist, int32_t ld, double *sums, void *stream);
int dsg_eval_hist_mmd(int32_t n_ref, const double *ref, int32_t ld_ref, int32_t n_gen, const double *gen, int32_t ld_gen, int32_t L,
                      double *ws, double *out, void *stream);

/* ---- Scene-graph statistics (no handle): what is left of the evaluation block of sg_go_sampling
 * (R/runner/sampler/sampler_node_adj.py:445-552) after the pairwise metrics above -- the triplet histogram of
 * compute_triplet_tv_dist, the per-layout metrics of compute_bbox_ioa and the row statistics the F1 matrix is reduced to.
 * Kernels: csrc/sgstat_kernels.hip; Python: diffusesg_amd/evaluate.py (SceneGraphEvaluatorHipFull, evaluate_samples); pinned by
 * tests/golden/eval_full.npz.  Device pointers, caller's stream, DSG_ERR_INVALID for a bad argument instead of a launch.  Integer
 * counts use integer atomics, float64 sums run in a fixed order: repeated calls are bit-identical.
 *
 * Triplet counts (_get_triplet_type_hist, bbox_metrics.py:215-268, summed over the graphs): edge_types [B, N, N] and node_types
 *   [B, N] int32.  Every entry with edge_types[b,i,j] != 0 is the triplet (node_types[b,i], node_types[b,j], edge_types[b,i,j]).
 *   QUIRKS kept from the reference: node flags are not consulted (it ignores its node_flags argument) and a diagonal entry counts.
 *   sorted_keys: the n_keys allowed triplets packed as subject << 42 | object << 21 | predicate (21 bits each), ascending;
 *   key_pos[k]: position of sorted key k in the caller's (dictionary) order.  counts [n_keys] int64 in that order and novel [1]
 *   int64 (triplets not in the table) are zeroed on the stream and then filled.  A value outside [0, 2^21) never matches a key
 *   (the Python wrapper refuses it beforehand).  n_keys may be 0 (everything is novel).
 * Layout metrics (R/evaluation/blt_utils.py through compute_bbox_ioa, bbox_metrics.py:443-483): boxes [B, N, 4] fp32 x1 y1 x2 y2,
 *   flags [B, N] uint8, canvas_size 1..64 (the reference passes 32), N <= 255.  values [4][B] float64 and valid [4][B] uint8
 *   (0 where the reference returns None; the value is 0 then), metric order: 0 IoU (mean of the positive pair IoUs; the IoU is 0
 *   where |union| <= 1e-8), 1 perceptual IoU (pixels covered more than once / pixels covered on the canvas, coordinates scaled
 *   in float32 and rounded half to even), 2 overlap (sum of the positive intersection areas), 3 alignment (sum over the boxes of
 *   the smallest left / centre / right distance to another box).  Pair terms are float32 op by op as in NumPy, summed in float64
 *   (the reference sums IoU and overlap in float32).
 * F1 row statistics: blk [rows, Y, W] float64 as the bbox F1 entry writes it; row_max, row_mean, row_median [rows, W] float64 and
 *   row_argmax [rows, W] int32 over the Y axis: the exact median (np.median), the first index of the maximum (np.argmax); a row
 *   holding a NaN gives NaN three times and the index of its first NaN.  Y <= 16384 (one row in LDS), W <= 8. */
int dsg_sgstat_triplet_counts(int32_t B, int32_t N, const int32_t *edge_types, const int32_t *node_types, int32_t n_keys,
                              const int64_t *sorted_keys, const int32_t *key_pos, int64_t *counts, int64_t *novel, void *stream);
int dsg_sgstat_layout(int32_t B, int32_t N, const float *boxes, const uint8_t *flags, int32_t canvas_size, double *values,
                      uint8_t *valid, void *stream);
int dsg_sgstat_f1_rowstats(int32_t rows, int32_t Y, int32_t W, const double *blk, double *row_max, double *row_mean,
                           double *row_median, int32_t *row_argmax, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DSG_H */
