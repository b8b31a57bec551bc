// guide_kernels.hip -- box guidance "through the skip path" inside the reverse loop (include/dsg.h: dsg_sample_guided).
//
// Per preconditioned call the loop shifts the denoised estimate D against the gradient of a box loss L(D),
//     D~ = D - f_b * c_i * g,      g = dL/dD_node,      c_i = w_i t^2 c_skip(t),
// where the network's Jacobian is dropped from dD/dx_hat = c_skip I + c_out dF/dx_hat.  The three losses are those of
// diffusesg_amd/guide.py (box_overlap_loss, box_region_loss with one rectangle per node, box_alignment_loss), always with the node
// flags, and their gradients are closed forms with torch autograd's conventions at the kinks: relu passes where its argument is > 0,
// minimum / maximum split a tie evenly.
//
// One block per graph, N <= 64.  Boxes, lines and flags sit in LDS; the loss terms are evaluated in float64 and rounded once, so the
// float32 gradient is the correctly rounded one up to the last bit.  Padded nodes are chosen by a select on the flags: a NaN in a
// padded row never reaches a sum.  Every reduction has one fixed order and uses no atomics; nothing depends on B or on the graph's
// position in the batch.
//
// The relation term (dsg_sample_guided_rel) is a compile-time variant of the same body: a pairwise squared hinge on
// box pairs whose kinds are given or decoded from the adjacency estimate of the call.  A guide without relations runs the kernel
// without it.
#include "kernels_common.hip.h"

#include <float.h>

namespace dsg {

// ||x_hat_b - D_b||^2 over the graph's live entries (adjacency and node), float64, t_graph_dot_kernel's order: thread t adds its
// entries j = t, t + 1024, ... ascending, adjacency before node, then a halving tree
constexpr int GNORM_T = 1024;
__global__ __launch_bounds__(GNORM_T) void graph_diff_norm_kernel(CStatePtrs a, CStatePtrs b, const uint8_t *__restrict__ flags, double *out, int N,
                                                                 int Ca, int Cn) {
    __shared__ double part[GNORM_T];
    __shared__ uint8_t fl[GUIDE_MAX_N];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid < N) fl[tid] = flags[(size_t)g * N + tid];
    __syncthreads();
    const size_t na = (size_t)Ca * N * N, nn = (size_t)N * Cn;
    const float *pa = a.adj + (size_t)g * na, *pb = b.adj + (size_t)g * na, *qa = a.node + (size_t)g * nn, *qb = b.node + (size_t)g * nn;
    double acc = 0.0;
    for (size_t j = tid; j < na; j += GNORM_T) {
        const int k = (int)(j % N), i = (int)((j / N) % N);
        if (fl[i] && fl[k]) { const double v = (double)pa[j] - (double)pb[j]; acc += v * v; }
    }
    for (size_t j = tid; j < nn; j += GNORM_T)
        if (fl[j / Cn]) { const double v = (double)qa[j] - (double)qb[j]; acc += v * v; }
    part[tid] = acc;
    __syncthreads();
    for (int w = GNORM_T / 2; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[g] = part[0];
}
bool launch_graph_diff_norm(CStatePtrs a, CStatePtrs b, const uint8_t *flags, double *out, Dims d, hipStream_t s) {
    if (d.B < 1 || d.N < 1 || d.N > GUIDE_MAX_N || d.Ca < 1 || d.Cn < 1) return false;
    hipLaunchKernelGGL(graph_diff_norm_kernel, dim3((unsigned)d.B), dim3(GNORM_T), 0, s, a, b, flags, out, d.N, d.Ca, d.Cn);
    return true;
}

// the derivative of minimum(a, b) / maximum(a, b) with respect to a as torch autograd defines it: a tie is split evenly
__device__ __forceinline__ double dmin_da(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double dmax_da(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }
__device__ __forceinline__ double relu_d(double v) { return v > 0.0 ? v : 0.0; }

// Lines of a box, in guide.py's order: 0 left, 1 centre x, 2 right, 3 top, 4 centre y, 5 bottom.  Work item (q, k) = line q of node
// k owns dL/d line_q(k) and the part of L that is attributed to it; a thread takes items tid, tid + GUIDE_T, ...
constexpr int GUIDE_T = 512, GUIDE_LINES = 6;   // 6 x 64 items: one round, two waves per SIMD to hide the float64 exp chains

// ---- the relation term: a squared hinge per ordered pair (subject s, object o) and kind ----
// The graph's kinds in LDS, one byte per ordered pair, 64 bytes per subject row.  An item reads its node's column (lanes = consecutive
// objects: consecutive bytes) and its node's row (lanes = consecutive subjects: 64 bytes apart, every fourth lane on one bank); the
// word of a row is XORed with the row's low bits, which spreads a row walk over 16 banks instead of 4 and leaves a column walk alone
__device__ __forceinline__ int kind_at(int s, int o) { return s * GUIDE_MAX_N + ((((o >> 2) ^ (s & 15)) << 2) | (o & 3)); }
// What pair (s, o) of kind `kind` adds to dL/d line_q of its subject (subj) or of its object, and, on the subject's side, the part of
// the pair's loss that is attributed to line q -- every elementary term is counted once, at the subject's line in it.  m: the margin
__device__ __forceinline__ void rel_pair(int q, int kind, bool subj, const double (*ln)[GUIDE_MAX_N], int s, int o, double m, double &grad,
                                         double &loss) {
    if (kind >= 1 && kind <= 4) {   // left of / right of (centre x), above / below (centre y; y grows downwards)
        const int ax = kind <= 2 ? 1 : 4;
        if (q != ax) return;
        const double sg = (kind & 1) ? 1.0 : -1.0;   // h(sg (c_s - c_o) + m)
        const double r = relu_d(sg * (ln[ax][s] - ln[ax][o]) + m);
        grad += (subj ? sg : -sg) * 2.0 * r;
        if (subj) loss += r * r;
    } else if (kind == 5 || kind == 6) {   // inside: the subject within the object; contains: the object within the subject
        if (q == 1 || q == 4) return;
        const int in = kind == 5 ? s : o, out = kind == 5 ? o : s;
        const bool low = q == 0 || q == 3;   // h(outer - inner) at the low sides, h(inner - outer) at the high ones
        const double r = relu_d(low ? ln[q][out] - ln[q][in] : ln[q][in] - ln[q][out]);
        const double d_in = low ? -2.0 * r : 2.0 * r;
        grad += (subj == (kind == 5)) ? d_in : -d_in;
        if (subj) loss += r * r;
    } else if (kind == 7) {   // on: (bottom_s - top_o)^2, not hinged, + the subject's centre x within the object's extent
        if (q == 5 && subj) { const double d = ln[5][s] - ln[3][o]; grad += 2.0 * d; loss += d * d; }
        else if (q == 3 && !subj) grad -= 2.0 * (ln[5][s] - ln[3][o]);
        else if (q == 1 && subj) {
            const double a = relu_d(ln[0][o] - ln[1][s]), b = relu_d(ln[1][s] - ln[2][o]);
            grad += 2.0 * (b - a); loss += a * a + b * b;
        } else if (q == 0 && !subj) grad += 2.0 * relu_d(ln[0][o] - ln[1][s]);
        else if (q == 2 && !subj) grad -= 2.0 * relu_d(ln[1][s] - ln[2][o]);
    }
}

// REL: the variant with the relation term; without it the body is the kernel as it was, and D_adj / Ca / kinds_out are not read
template <bool REL, bool DECODED>
__device__ __forceinline__ void box_guide_body(const GuideParams *__restrict__ P, const StepRow *tab, const RunCtl *ctl, float coef_direct,
                                               const float *__restrict__ D_node, const uint8_t *__restrict__ flags,
                                               const double *__restrict__ ref_norm2, int stage1, BoxGuideOut o, int N, int Cn,
                                               const float *__restrict__ D_adj, int Ca, uint8_t *kinds_out) {
    __shared__ double ln[GUIDE_LINES][GUIDE_MAX_N];    // the six lines of every node's box
    __shared__ double am[GUIDE_LINES][GUIDE_MAX_N];    // alignment: row maximum of -d^2 / tau
    __shared__ double as[GUIDE_LINES][GUIDE_MAX_N];    //            sum of exp(z - maximum)
    __shared__ double ai[GUIDE_LINES][GUIDE_MAX_N];    //            and its inverse
    __shared__ double gl[GUIDE_LINES][GUIDE_MAX_N];    // dL / d line
    __shared__ double lp[GUIDE_LINES][GUIDE_MAX_N];    // the item's share of L
    __shared__ float sh[GUIDE_MAX_N][4];               // c * g, zero at known entries
    __shared__ uint8_t fl[GUIDE_MAX_N];
    __shared__ float fac;
    __shared__ double pl[GUIDE_MAX_N], ps[GUIDE_MAX_N];   // per node: its six shares of L, its four squared shift entries
    const int g = blockIdx.x, tid = threadIdx.x;
    const GuideParams p = *P;
    const int items = GUIDE_LINES * N;
    if (tid < N) {
        const bool v = flags[(size_t)g * N + tid] != 0;
        fl[tid] = v;
        const float *src = D_node + ((size_t)g * N + tid) * Cn + (Cn - 4);
        // b = D * 0.5 + 0.5 (io.decode); a padded row is never read
        const double cx = v ? (double)src[0] * 0.5 + 0.5 : 0.0, cy = v ? (double)src[1] * 0.5 + 0.5 : 0.0;
        const double bw = v ? (double)src[2] * 0.5 + 0.5 : 0.0, bh = v ? (double)src[3] * 0.5 + 0.5 : 0.0;
        ln[0][tid] = cx - 0.5 * bw; ln[1][tid] = cx; ln[2][tid] = cx + 0.5 * bw;
        ln[3][tid] = cy - 0.5 * bh; ln[4][tid] = cy; ln[5][tid] = cy + 0.5 * bh;
    }
    __syncthreads();
    uint8_t *kd = nullptr;
    if constexpr (REL) {
        __shared__ uint8_t kd_s[GUIDE_MAX_N * GUIDE_MAX_N];   // kind_at(subject, object): 4 KB
        kd = kd_s;
        // every thread walks the N^2 ordered pairs, the object index fastest: a wave reads consecutive floats of each channel plane.
        // A pair that is not live (a padded row or column, the diagonal) is selected away before anything of it is read
        const size_t nn = (size_t)N * N;
        for (int e = tid; e < (int)nn; e += GUIDE_T) {
            const int i = e / N, j = e % N;
            int kind = 0;
            if (fl[i] && fl[j] && i != j) {
                if constexpr (DECODED) {
                    const int pr = decode_attr(D_adj + (size_t)g * Ca * nn + e, nn, Ca, p.rel_enc, p.rel_ntype);
                    kind = (pr >= 0 && pr < p.rel_ntype) ? p.pred_kind[pr] : 0;   // a NaN under ddpm decodes to -1: none
                } else kind = p.kinds[(size_t)g * nn + e];
                if (kind >= REL_KINDS) kind = 0;
            }
            kd[kind_at(i, j)] = (uint8_t)kind;
            if (kinds_out) kinds_out[(size_t)g * nn + e] = (uint8_t)kind;
        }
        __syncthreads();
    }
    int n_valid = 0;
    for (int j = 0; j < N; j++) n_valid += fl[j] ? 1 : 0;
    const bool align = p.a_a != 0.f && n_valid >= 2;
    const double tau = (double)p.tau;
    // alignment, pass 1: per (line, node) the maximum and the sum of the soft minimum over the other valid nodes
    if (align)
        for (int it = tid; it < items; it += GUIDE_T) {
            const int q = it / N, k = it % N;
            if (!fl[k]) continue;
            const double lk = ln[q][k];
            double m = -DBL_MAX;
            for (int j = 0; j < N; j++)
                if (j != k && fl[j]) { const double dd = lk - ln[q][j]; const double z = -(dd * dd) / tau; m = z > m ? z : m; }
            double sum = 0.0;
            for (int j = 0; j < N; j++)
                if (j != k && fl[j]) { const double dd = lk - ln[q][j]; sum += exp(-(dd * dd) / tau - m); }
            am[q][k] = m; as[q][k] = sum; ai[q][k] = 1.0 / sum;
        }
    __syncthreads();
    for (int it = tid; it < items; it += GUIDE_T) {
        const int q = it / N, k = it % N;
        double grad = 0.0, loss = 0.0;
        if (fl[k]) {
            const double lk = ln[q][k];
            if (align) {   // soft_k = -tau (m + log sum) + tau log(n - 1); d/d line_k collects row k and column k of the softmax
                loss += (double)p.a_a * (-tau * (am[q][k] + log(as[q][k])) + tau * log((double)(n_valid - 1)));
                double ga = 0.0;
                for (int j = 0; j < N; j++)
                    if (j != k && fl[j]) {
                        const double dd = lk - ln[q][j], z = -(dd * dd) / tau;
                        ga += 2.0 * dd * (exp(z - am[q][k]) * ai[q][k] + exp(z - am[q][j]) * ai[q][j]);
                    }
                grad += (double)p.a_a * ga;
            }
            if (p.a_o != 0.f && q != 1 && q != 4) {   // overlap: sum over unordered valid pairs of relu(iw) relu(ih)
                const bool horiz = q < 3, low = (q == 0 || q == 3);   // this line bounds the width / is the lower bound of its extent
                double go = 0.0, lo = 0.0;
                for (int j = 0; j < N; j++)
                    if (j != k && fl[j]) {
                        const double iw = fmin(ln[2][k], ln[2][j]) - fmax(ln[0][k], ln[0][j]);
                        const double ih = fmin(ln[5][k], ln[5][j]) - fmax(ln[3][k], ln[3][j]);
                        const double mine = horiz ? iw : ih, other = relu_d(horiz ? ih : iw);
                        if (mine > 0.0) go += low ? -other * dmax_da(lk, ln[q][j]) : other * dmin_da(lk, ln[q][j]);
                        if (q == 0 && j > k) lo += relu_d(iw) * relu_d(ih);
                    }
                grad += (double)p.a_o * go;
                loss += (double)p.a_o * lo;
            }
            if (p.a_r != 0.f && q != 1 && q != 4 && p.sel[(size_t)g * N + k]) {   // region: squared hinge of the four overshoots
                const float *rc = p.region + ((size_t)g * N + k) * 4;
                const double over = q == 0 ? relu_d((double)rc[0] - lk) : q == 3 ? relu_d((double)rc[1] - lk)
                                  : q == 2 ? relu_d(lk - (double)rc[2]) : relu_d(lk - (double)rc[3]);
                grad += (double)p.a_r * ((q == 0 || q == 3) ? -2.0 * over : 2.0 * over);
                loss += (double)p.a_r * over * over;
            }
            if constexpr (REL) {   // relations: node k's row (k the subject) and column (k the object), the partner ascending
                const double m = (double)p.rel_margin;
                double gr = 0.0, lr = 0.0;
                for (int j = 0; j < N; j++)
                    if (j != k && fl[j]) {
                        const int ks = kd[kind_at(k, j)], ko = kd[kind_at(j, k)];
                        if (ks) rel_pair(q, ks, true, ln, k, j, m, gr, lr);
                        if (ko) rel_pair(q, ko, false, ln, j, k, m, gr, lr);
                    }
                grad += (double)p.a_rel * gr;
                loss += (double)p.a_rel * lr;
            }
        }
        gl[q][k] = grad; lp[q][k] = loss;
    }
    __syncthreads();
    const float c = tab ? p.coef[tab[ctl->step].sched] : coef_direct;
    if (tid < N) {
        const bool v = fl[tid];
        // lines -> (cx, cy, w, h) -> D: the 0.5 of * 0.5 + 0.5
        const double gb[4] = {gl[0][tid] + gl[1][tid] + gl[2][tid], gl[3][tid] + gl[4][tid] + gl[5][tid],
                              0.5 * (gl[2][tid] - gl[0][tid]), 0.5 * (gl[5][tid] - gl[3][tid])};
        const size_t row = (size_t)g * N + tid;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float gd = v ? (float)(0.5 * gb[k]) : 0.f;
            const bool known = p.mask_node && p.mask_node[row * Cn + (Cn - 4) + k] != 0;
            sh[tid][k] = (known || !v) ? 0.f : __fmul_rn(c, gd);   // known entries win
            if (o.grad) o.grad[row * 4 + k] = gd;
        }
        // the two per-graph sums in a fixed order: per node here (lines / entries ascending), over the nodes ascending by thread 0
        double l6 = 0.0, s4 = 0.0;
        for (int q = 0; q < GUIDE_LINES; q++) l6 += lp[q][tid];
        for (int k = 0; k < 4; k++) s4 += (double)sh[tid][k] * (double)sh[tid][k];
        pl[tid] = l6; ps[tid] = s4;
    }
    __syncthreads();
    if (tid == 0) {
        double loss = 0.0, s2 = 0.0;
        for (int k = 0; k < N; k++) { loss += pl[k]; s2 += ps[k]; }
        const float sn = (float)sqrt(s2);
        float f = 1.f, rn = 0.f;
        if (ref_norm2) {   // guide.clip_factor, float32 operation by operation
            rn = (float)sqrt(ref_norm2[g]);
            const float bound = __fmul_rn(p.clip_ratio, rn);
            f = sn > bound ? __fdiv_rn(bound, fmaxf(sn, FLT_MIN)) : 1.f;
        }
        fac = f;
        if (o.loss) o.loss[g] = (float)loss;
        if (o.factor) o.factor[g] = f;
        if (o.norms) { o.norms[2 * g] = sn; o.norms[2 * g + 1] = rn; }
        if (stage1 && tab && p.trace) p.trace[(size_t)ctl->step * gridDim.x + g] = (float)loss;
    }
    __syncthreads();
    if (tid < N * 4) o.shift[(size_t)g * N * 4 + tid] = __fmul_rn(fac, sh[tid / 4][tid % 4]);
}
__global__ __launch_bounds__(GUIDE_T) void box_guide_kernel(const GuideParams *__restrict__ P, const StepRow *tab, const RunCtl *ctl, float coef_direct,
                                                           const float *__restrict__ D_node, const uint8_t *__restrict__ flags,
                                                           const double *__restrict__ ref_norm2, int stage1, BoxGuideOut o, int N, int Cn) {
    box_guide_body<false, false>(P, tab, ctl, coef_direct, D_node, flags, ref_norm2, stage1, o, N, Cn, nullptr, 0, nullptr);
}
template <bool DECODED>
__global__ __launch_bounds__(GUIDE_T) void box_guide_rel_kernel(const GuideParams *__restrict__ P, const StepRow *tab, const RunCtl *ctl, float coef_direct,
                                                               const float *__restrict__ D_adj, const float *__restrict__ D_node,
                                                               const uint8_t *__restrict__ flags, const double *__restrict__ ref_norm2, int stage1,
                                                               BoxGuideOut o, uint8_t *kinds_out, int N, int Ca, int Cn) {
    box_guide_body<true, DECODED>(P, tab, ctl, coef_direct, D_node, flags, ref_norm2, stage1, o, N, Cn, D_adj, Ca, kinds_out);
}
bool launch_box_guide_rel(const GuideParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_adj, const float *D_node,
                          const uint8_t *flags, const double *ref_norm2, bool stage1, BoxGuideOut o, uint8_t *kinds_out, bool decoded, Dims d,
                          hipStream_t s) {
    if (d.B < 1 || d.N < 1 || d.N > GUIDE_MAX_N || d.Cn < 4 || !o.shift || (decoded && (!D_adj || d.Ca < 1))) return false;
    if (decoded)
        hipLaunchKernelGGL(box_guide_rel_kernel<true>, dim3((unsigned)d.B), dim3(GUIDE_T), 0, s, P, tab, ctl, coef_direct, D_adj, D_node, flags,
                           ref_norm2, (int)stage1, o, kinds_out, d.N, d.Ca, d.Cn);
    else
        hipLaunchKernelGGL(box_guide_rel_kernel<false>, dim3((unsigned)d.B), dim3(GUIDE_T), 0, s, P, tab, ctl, coef_direct, D_adj, D_node, flags,
                           ref_norm2, (int)stage1, o, kinds_out, d.N, d.Ca, d.Cn);
    return true;
}
bool launch_box_guide(const GuideParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_node, const uint8_t *flags,
                      const double *ref_norm2, bool stage1, BoxGuideOut o, Dims d, hipStream_t s) {
    if (d.B < 1 || d.N < 1 || d.N > GUIDE_MAX_N || d.Cn < 4 || !o.shift) return false;
    hipLaunchKernelGGL(box_guide_kernel, dim3((unsigned)d.B), dim3(GUIDE_T), 0, s, P, tab, ctl, coef_direct, D_node, flags, ref_norm2,
                       (int)stage1, o, d.N, d.Cn);
    return true;
}

// D~_node = valid ? D_node - shift at the box channels : 0, on its own (dsg_debug_box_guide; the loop subtracts inside its update kernels)
__global__ void box_apply_kernel(const float *__restrict__ D_node, const float *__restrict__ shift, const uint8_t *__restrict__ flags, float *out,
                                 size_t n, int Cn) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / Cn;
    const int c = (int)(i % Cn) - (Cn - 4);
    out[i] = !flags[row] ? 0.f : (c >= 0 ? __fsub_rn(D_node[i], shift[row * 4 + c]) : D_node[i]);
}
void launch_box_apply(const float *D_node, const float *shift, const uint8_t *flags, float *out, Dims d, hipStream_t s) {
    const size_t n = (size_t)d.B * d.N * d.Cn;
    hipLaunchKernelGGL(box_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, D_node, shift, flags, out, n, d.Cn);
}

}  // namespace dsg
