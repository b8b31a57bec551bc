// guide_content_kernels.hip -- content guidance inside the reverse loop (include/dsg.h: dsg_sample_guided_content).
//
// "Samples that contain subject - predicate - object": per graph K items, each three target vectors in value space (subject label
// s_k [Cl], object label o_k [Cl], predicate p_k [Ca]) and three weights (a_s, a_o, a_p).  Over the live ordered pairs (i, j), i != j,
// both nodes valid, P of them,
//     d_k(i,j) = a_s |Dn[i,:Cl] - s_k|^2 + a_o |Dn[j,:Cl] - o_k|^2 + a_p |Da[:,i,j] - p_k|^2
//     L_k      = -tau log((1/P) sum exp(-d_k / tau)) = min d_k - tau log(S_k / P),   S_k = sum exp(-(d_k - min d_k) / tau)
//     pi_k     = exp(-(d_k - min d_k) / tau) / S_k
//     g_adj[c,i,j] = sum_k pi_k(i,j) 2 a_p (Da[c,i,j] - p_k[c])
//     g_node[i,c]  = sum_k (sum_j pi_k(i,j)) 2 a_s (Dn[i,c] - s_k[c]) + (sum_j pi_k(j,i)) 2 a_o (Dn[i,c] - o_k[c])        (c < Cl)
// and the shift is f_b * fmul(c_i w, g), zero at known entries, at padded rows and columns, on the diagonal and at node channels >= Cl.
//
// 512-thread blocks, N <= 64, any Ca and Cl: a graph's adjacency estimate is never assumed to fit on chip.  The phases run in one block
// per graph, or -- by default -- as a grid: (item, graph) blocks for phase A, (round, graph) blocks for phase B, one block per graph for
// the rest (the modes of content_guide_kernel below).
//   phase A, item after item: the per-node label distances, the item's d_k tile (N^2 doubles of LDS), its minimum with the lowest flat
//            index (the `best` pair), exp in place, S_k, and the row and column sums of pi_k;
//   phase B, pair-major: a thread recomputes d_k of its pairs for all items at once from the minima and sums of phase A (the same
//            operations in the same order: the same bits), forms pi_k and walks the channels, so that every entry of g_adj is one float64
//            sum over k ascending, rounded once;
//   phase C: the label channels from the row and column sums; then the shift's norm, the clip factor and the scaled store.
// Everything is float64 from the float32 inputs and rounded once; pairs that are not live and rows that are padded are chosen by
// selects and never read.  Every sum has one fixed order, nothing is atomic, nothing depends on B or on the graph's position.
#include "kernels_common.hip.h"

#include <float.h>
#include <limits.h>
#include <stdlib.h>

namespace dsg {

constexpr int CG_T = 512;
constexpr int CG_K = CONTENT_MAX_ITEMS;

// sum_c (row[c] - tgt[c])^2, c ascending
__device__ __forceinline__ double label_dist(const float *__restrict__ row, const float *__restrict__ tgt, int n) {
    double acc = 0.0;
    for (int c = 0; c < n; c++) { const double dd = (double)row[c] - (double)tgt[c]; acc += dd * dd; }
    return acc;
}
// d_k of one pair from its three squared distances
__device__ __forceinline__ double item_dist(double a_s, double a_o, double a_p, double ds, double dob, double pe) {
    return (a_s * ds + a_o * dob) + a_p * pe;
}

// Two forms of the same arithmetic.  CG_WHOLE: one block per graph runs everything.  The grid form is three launches:
//   CG_ITEMS   block (k, g): phase A of item k of graph g; leaves the item's minimum, sum, loss, the row and column sums of pi_k and
//              the per-node label distances in `stats` (CG_STAT doubles per item);
//   CG_PAIRS   block (r, g): phase B for the pairs e = tid + r CG_T of graph g -- the pairs that thread tid of the whole form takes in
//              its round r -- storing the unclipped shift and, per pair, its share of |shift|^2 (`part`, N^2 doubles per graph);
//   CG_FINISH  one block per graph: phase C, the norm (thread tid adds the shares of its rounds r ascending, then its label entries,
//              then the halving tree: the whole form's order), the clip factor and the scaled store.
// Every value is computed by the same code in the same order in both forms: the same bits.
constexpr int CG_WHOLE = 0, CG_ITEMS = 1, CG_FINISH = 2, CG_PAIRS = 3;
constexpr int CG_R = GUIDE_MAX_N * GUIDE_MAX_N / CG_T;   // rounds of the pair-major loop
constexpr int CG_STAT = CONTENT_STAT_DOUBLES;   // m, S, L_k, pad, rs[64], cs[64], subject label distances [64], object label distances [64]
template <int MODE>
__global__ __launch_bounds__(CG_T) void content_guide_kernel(const ContentParams *__restrict__ P, const StepRow *tab, const RunCtl *ctl,
                                                            float coef_direct, const float *__restrict__ D_adj,
                                                            const float *__restrict__ D_node, const uint8_t *__restrict__ flags,
                                                            const double *__restrict__ ref_norm2, int stage1, ContentOut o, int N, int Ca,
                                                            int Cn, double *stats) {
    __shared__ double big[GUIDE_MAX_N * GUIDE_MAX_N];   // phase A: the item's tile; phase B: the label distances of every item
    __shared__ double rs[CG_K][GUIDE_MAX_N];            // sum_j pi_k(i, j)
    __shared__ double cs[CG_K][GUIDE_MAX_N];            // sum_i pi_k(i, j)
    __shared__ double red[CG_T];
    __shared__ int redi[CG_T];
    __shared__ double dsn[GUIDE_MAX_N], don[GUIDE_MAX_N];
    __shared__ double mn[CG_K], sm[CG_K], lk[CG_K];
    __shared__ float wa[CG_K][3];
    __shared__ uint8_t fl[GUIDE_MAX_N];
    __shared__ float fac;
    const int g = (MODE == CG_ITEMS || MODE == CG_PAIRS) ? blockIdx.y : blockIdx.x, tid = threadIdx.x;
    const int n_graphs = (MODE == CG_ITEMS || MODE == CG_PAIRS) ? gridDim.y : gridDim.x;
    double *part = stats ? stats + (size_t)n_graphs * CG_K * CG_STAT + (size_t)g * GUIDE_MAX_N * GUIDE_MAX_N : nullptr;
    const ContentParams p = *P;
    const int K = p.K, Cl = p.Cl, NN = N * N;
    const int k_lo = MODE == CG_ITEMS ? (int)blockIdx.x : 0, k_hi = MODE == CG_ITEMS ? k_lo + 1 : (MODE == CG_WHOLE ? K : 0);
    const size_t adj0 = (size_t)g * Ca * NN, node0 = (size_t)g * N * Cn, lab0 = (size_t)g * N * Cl;
    if (tid < N) fl[tid] = flags[(size_t)g * N + tid] != 0;
    if (tid < K * 3) wa[tid / 3][tid % 3] = p.w_spo[(size_t)g * K * 3 + tid];
    __syncthreads();
    int n_valid = 0;
    for (int j = 0; j < N; j++) n_valid += fl[j] ? 1 : 0;
    const int n_pairs = n_valid * (n_valid - 1);
    const float c = tab ? p.coef[tab[ctl->step].sched] : coef_direct;
    const float cw = __fmul_rn(c, p.w);
    if (n_pairs == 0 && MODE == CG_PAIRS) return;   // the finishing launch writes the zeros
    if (n_pairs == 0 && MODE == CG_ITEMS) {   // the finishing launch does not read the statistics of such a graph
        if (tid == 0) {
            if (o.item_loss) o.item_loss[(size_t)g * K + k_lo] = 0.f;
            if (o.best) { o.best[((size_t)g * K + k_lo) * 2] = -1; o.best[((size_t)g * K + k_lo) * 2 + 1] = -1; }
        }
        return;
    }
    if (n_pairs == 0) {   // nothing to choose from: exactly 0, and nothing of the estimate is read
        for (size_t e = tid; e < (size_t)Ca * NN; e += CG_T) {
            o.shift_adj[adj0 + e] = 0.f;
            if (o.grad_adj) o.grad_adj[adj0 + e] = 0.f;
        }
        for (int e = tid; e < N * Cl; e += CG_T) {
            o.shift_label[lab0 + e] = 0.f;
            if (o.grad_label) o.grad_label[lab0 + e] = 0.f;
        }
        if (tid < K) {
            if (o.item_loss) o.item_loss[(size_t)g * K + tid] = 0.f;
            if (o.best) { o.best[((size_t)g * K + tid) * 2] = -1; o.best[((size_t)g * K + tid) * 2 + 1] = -1; }
        }
        if (tid == 0) {
            if (o.loss) o.loss[g] = 0.f;
            if (o.factor) o.factor[g] = 1.f;
            if (o.norms) { o.norms[2 * g] = 0.f; o.norms[2 * g + 1] = ref_norm2 ? (float)sqrt(ref_norm2[g]) : 0.f; }
            if (stage1 && tab && p.trace) p.trace[(size_t)ctl->step * gridDim.x + g] = 0.f;
        }
        return;
    }
    const double tau = (double)p.tau;
    // ---- phase A: item after item ----
    for (int k = k_lo; k < k_hi; k++) {
        const double a_s = (double)wa[k][0], a_o = (double)wa[k][1], a_p = (double)wa[k][2];
        const bool active = a_s != 0.0 || a_o != 0.0 || a_p != 0.0;
        const float *sk = p.subj + ((size_t)g * K + k) * Cl, *ok = p.obj + ((size_t)g * K + k) * Cl, *pk = p.pred + ((size_t)g * K + k) * Ca;
        if (!active) {   // uniform over the block
            if (tid < N) { rs[k][tid] = 0.0; cs[k][tid] = 0.0; }
            if (tid == 0) {
                mn[k] = 0.0; sm[k] = 1.0; lk[k] = 0.0;
                if (o.item_loss) o.item_loss[(size_t)g * K + k] = 0.f;
                if (o.best) { o.best[((size_t)g * K + k) * 2] = -1; o.best[((size_t)g * K + k) * 2 + 1] = -1; }
            }
            continue;
        }
        if (tid < 2 * N) {
            const int i = tid % N;
            const bool subj = tid < N;
            double v = 0.0;
            if (fl[i] && (subj ? a_s : a_o) != 0.0) v = label_dist(D_node + node0 + (size_t)i * Cn, subj ? sk : ok, Cl);
            (subj ? dsn : don)[i] = v;
        }
        __syncthreads();
        double best_d = DBL_MAX;
        int best_e = INT_MAX;
        for (int e = tid; e < NN; e += CG_T) {
            const int i = e / N, j = e % N;
            double d = DBL_MAX;
            if (fl[i] && fl[j] && i != j) {
                double pe = 0.0;
                if (a_p != 0.0)
                    for (int ch = 0; ch < Ca; ch++) { const double dd = (double)D_adj[adj0 + (size_t)ch * NN + e] - (double)pk[ch]; pe += dd * dd; }
                d = item_dist(a_s, a_o, a_p, dsn[i], don[j], pe);
                if (d < best_d) { best_d = d; best_e = e; }
            }
            big[e] = d;
        }
        red[tid] = best_d; redi[tid] = best_e;
        __syncthreads();
        for (int w = CG_T / 2; w > 0; w >>= 1) {   // the minimum, the lowest flat index among equals
            if (tid < w) {
                const double a = red[tid + w];
                const int ia = redi[tid + w];
                if (a < red[tid] || (a == red[tid] && ia < redi[tid])) { red[tid] = a; redi[tid] = ia; }
            }
            __syncthreads();
        }
        const double m = red[0];
        const int be = redi[0];
        __syncthreads();
        double esum = 0.0;
        for (int e = tid; e < NN; e += CG_T) {
            const int i = e / N, j = e % N;
            double ex = 0.0;
            if (fl[i] && fl[j] && i != j) { ex = exp(-(big[e] - m) / tau); esum += ex; }
            big[e] = ex;
        }
        red[tid] = esum;
        __syncthreads();
        for (int w = CG_T / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        const double S = red[0];
        if (tid < 2 * N) {   // row sums (the node as subject) and column sums (the node as object) of pi_k, the partner ascending
            const int i = tid % N;
            const bool row = tid < N;
            double acc = 0.0;
            if (fl[i])
                for (int j = 0; j < N; j++) acc += row ? big[i * N + j] : big[j * N + i];
            (row ? rs : cs)[k][i] = acc / S;
        }
        if (tid == 0) {
            const double l = m - tau * log(S / (double)n_pairs);
            mn[k] = m; sm[k] = S; lk[k] = l;
            if (o.item_loss) o.item_loss[(size_t)g * K + k] = (float)l;
            if (o.best) { o.best[((size_t)g * K + k) * 2] = be / N; o.best[((size_t)g * K + k) * 2 + 1] = be % N; }
        }
        __syncthreads();
    }
    __syncthreads();
    if constexpr (MODE == CG_ITEMS) {   // the item's statistics, for the finishing launch
        double *st = stats + ((size_t)g * K + k_lo) * CG_STAT;
        if (tid < N) {
            st[4 + tid] = rs[k_lo][tid]; st[4 + GUIDE_MAX_N + tid] = cs[k_lo][tid];
            st[4 + 2 * GUIDE_MAX_N + tid] = dsn[tid]; st[4 + 3 * GUIDE_MAX_N + tid] = don[tid];   // (unread where the item's weight is 0)
        }
        if (tid == 0) { st[0] = mn[k_lo]; st[1] = sm[k_lo]; st[2] = lk[k_lo]; }
        return;
    }
    if constexpr (MODE == CG_FINISH || MODE == CG_PAIRS) {
        for (int it = tid; it < K * N; it += CG_T) {
            const int k = it / N, i = it % N;
            const double *st = stats + ((size_t)g * K + k) * CG_STAT;
            rs[k][i] = st[4 + i]; cs[k][i] = st[4 + GUIDE_MAX_N + i];
            if constexpr (MODE == CG_PAIRS) { big[(k * 2) * N + i] = st[4 + 2 * GUIDE_MAX_N + i]; big[(k * 2 + 1) * N + i] = st[4 + 3 * GUIDE_MAX_N + i]; }
        }
        if (tid < K) { const double *st = stats + ((size_t)g * K + tid) * CG_STAT; mn[tid] = st[0]; sm[tid] = st[1]; lk[tid] = st[2]; }
        __syncthreads();
    }
    // ---- phase B: the adjacency gradient, pair-major.  big = [K][2][N] label distances, recomputed as phase A computed them ----
    for (int it = tid; MODE == CG_WHOLE && it < K * 2 * N; it += CG_T) {
        const int k = it / (2 * N), r = it % (2 * N), i = r % N;
        const bool subj = r < N;
        const double a = (double)wa[k][subj ? 0 : 1];
        double v = 0.0;
        if (fl[i] && a != 0.0)
            v = label_dist(D_node + node0 + (size_t)i * Cn, (subj ? p.subj : p.obj) + ((size_t)g * K + k) * Cl, Cl);
        big[it] = v;
    }
    __syncthreads();
    double s2 = 0.0;   // this thread's share of |shift|^2 before the clip: pair after pair (each pair's channels summed first), then labels
    const int r_lo = MODE == CG_PAIRS ? (int)blockIdx.x : 0, r_hi = MODE == CG_PAIRS ? r_lo + 1 : (MODE == CG_WHOLE ? CG_R : 0);
    for (int r = r_lo; r < r_hi; r++) {
        const int e = tid + r * CG_T;
        if (e >= NN) break;
        const int i = e / N, j = e % N;
        if constexpr (MODE == CG_PAIRS) part[e] = 0.0;
        if (!(fl[i] && fl[j] && i != j)) {
            for (int ch = 0; ch < Ca; ch++) {
                o.shift_adj[adj0 + (size_t)ch * NN + e] = 0.f;
                if (o.grad_adj) o.grad_adj[adj0 + (size_t)ch * NN + e] = 0.f;
            }
            continue;
        }
        double q[CG_K];
#pragma unroll
        for (int k = 0; k < CG_K; k++) q[k] = 0.0;
        for (int ch = 0; ch < Ca; ch++) {
            const double v = (double)D_adj[adj0 + (size_t)ch * NN + e];
#pragma unroll
            for (int k = 0; k < CG_K; k++)
                if (k < K && wa[k][2] != 0.f) { const double dd = v - (double)p.pred[((size_t)g * K + k) * Ca + ch]; q[k] += dd * dd; }
        }
#pragma unroll
        for (int k = 0; k < CG_K; k++) {   // q: the pair term -> pi_k 2 a_p
            double v = 0.0;
            if (k < K && wa[k][2] != 0.f) {
                const double a_s = (double)wa[k][0], a_o = (double)wa[k][1], a_p = (double)wa[k][2];
                const double d = item_dist(a_s, a_o, a_p, big[(k * 2) * N + i], big[(k * 2 + 1) * N + j], q[k]);
                v = exp(-(d - mn[k]) / tau) / sm[k] * (2.0 * a_p);
            }
            q[k] = v;
        }
        double pair2 = 0.0;
        for (int ch = 0; ch < Ca; ch++) {
            const size_t idx = adj0 + (size_t)ch * NN + e;
            const double v = (double)D_adj[idx];
            double gs = 0.0;
#pragma unroll
            for (int k = 0; k < CG_K; k++)
                if (k < K && wa[k][2] != 0.f) gs += q[k] * (v - (double)p.pred[((size_t)g * K + k) * Ca + ch]);
            const float gd = (float)gs;
            const bool known = p.mask_adj && p.mask_adj[idx] != 0;
            const float sh = known ? 0.f : __fmul_rn(cw, gd);   // known entries win
            o.shift_adj[idx] = sh;
            if (o.grad_adj) o.grad_adj[idx] = gd;
            pair2 += (double)sh * (double)sh;
        }
        s2 += pair2;
        if constexpr (MODE == CG_PAIRS) part[e] = pair2;
    }
    if constexpr (MODE == CG_PAIRS) return;
    if constexpr (MODE == CG_FINISH)
        for (int r = 0; r < CG_R; r++) { const int e = tid + r * CG_T; if (e < NN) s2 += part[e]; }
    // ---- phase C: the label channels ----
    for (int it = tid; it < N * Cl; it += CG_T) {
        const int i = it / Cl, ch = it % Cl;
        float gd = 0.f, sh = 0.f;
        if (fl[i]) {
            const double v = (double)D_node[node0 + (size_t)i * Cn + ch];
            double gs = 0.0;
            for (int k = 0; k < K; k++) {
                const double a_s = (double)wa[k][0], a_o = (double)wa[k][1];
                if (a_s != 0.0) gs += rs[k][i] * (2.0 * a_s) * (v - (double)p.subj[((size_t)g * K + k) * Cl + ch]);
                if (a_o != 0.0) gs += cs[k][i] * (2.0 * a_o) * (v - (double)p.obj[((size_t)g * K + k) * Cl + ch]);
            }
            gd = (float)gs;
            const bool known = p.mask_node && p.mask_node[node0 + (size_t)i * Cn + ch] != 0;
            sh = known ? 0.f : __fmul_rn(cw, gd);
        }
        o.shift_label[lab0 + it] = sh;
        if (o.grad_label) o.grad_label[lab0 + it] = gd;
        s2 += (double)sh * (double)sh;
    }
    red[tid] = s2;
    __syncthreads();
    for (int w = CG_T / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        double loss = 0.0;
        for (int k = 0; k < K; k++) loss += lk[k];
        const float sn = (float)sqrt(red[0]);
        float f = 1.f, rn = 0.f;
        if (ref_norm2) {   // guide.clip_factor, float32 operation by operation: the content shift's own factor
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
    const float f = fac;
    if (f == 1.f) return;
    // the clipped graph: every thread scales the entries it stored itself
    for (int e = tid; e < NN; e += CG_T) {
        const int i = e / N, j = e % N;
        if (!(fl[i] && fl[j] && i != j)) continue;
        for (int ch = 0; ch < Ca; ch++) { const size_t idx = adj0 + (size_t)ch * NN + e; o.shift_adj[idx] = __fmul_rn(f, o.shift_adj[idx]); }
    }
    for (int it = tid; it < N * Cl; it += CG_T) o.shift_label[lab0 + it] = __fmul_rn(f, o.shift_label[lab0 + it]);
}

bool launch_content_guide(const ContentParams *P, const StepRow *tab, const RunCtl *ctl, float coef_direct, const float *D_adj, const float *D_node,
                          const uint8_t *flags, const double *ref_norm2, bool stage1, ContentOut o, int grid_items, double *stats, Dims d,
                          hipStream_t s) {
    if (d.B < 1 || d.N < 1 || d.N > GUIDE_MAX_N || d.Ca < 1 || d.Cn < 5 || !D_adj || !D_node || !o.shift_adj || !o.shift_label) return false;
    if (grid_items < 0 || grid_items > CONTENT_MAX_ITEMS || (grid_items > 0 && !stats)) return false;
    if (grid_items == 0) {
        hipLaunchKernelGGL(content_guide_kernel<CG_WHOLE>, dim3((unsigned)d.B), dim3(CG_T), 0, s, P, tab, ctl, coef_direct, D_adj, D_node, flags,
                           ref_norm2, (int)stage1, o, d.N, d.Ca, d.Cn, nullptr);
        return true;
    }
    hipLaunchKernelGGL(content_guide_kernel<CG_ITEMS>, dim3((unsigned)grid_items, (unsigned)d.B), dim3(CG_T), 0, s, P, tab, ctl, coef_direct, D_adj,
                       D_node, flags, ref_norm2, (int)stage1, o, d.N, d.Ca, d.Cn, stats);
    hipLaunchKernelGGL(content_guide_kernel<CG_PAIRS>, dim3((unsigned)((d.N * d.N + CG_T - 1) / CG_T), (unsigned)d.B), dim3(CG_T), 0, s, P, tab, ctl,
                       coef_direct, D_adj, D_node, flags, ref_norm2, (int)stage1, o, d.N, d.Ca, d.Cn, stats);
    hipLaunchKernelGGL(content_guide_kernel<CG_FINISH>, dim3((unsigned)d.B), dim3(CG_T), 0, s, P, tab, ctl, coef_direct, D_adj, D_node, flags,
                       ref_norm2, (int)stage1, o, d.N, d.Ca, d.Cn, stats);
    return true;
}
// The form a run with K items per graph takes: the grid, always (CONTENT_GRID_MIN_ITEMS = 1) -- it is the faster form at every K measured
// (profiles/guide_content_bench.md).  The one-block form exists FOR MEASUREMENT AND FOR THE BIT-EQUALITY TEST ONLY: nothing in the
// product selects it.  DSG_CONTENT_GRID = 0 in the environment forces it, = 1 forces the grid; the variable is read when a run is
// planned, so it is a measurement switch, not an option of the handle.
int content_grid_items(int K) {
    const char *e = getenv("DSG_CONTENT_GRID");
    const bool grid = e && *e ? *e != '0' : K >= CONTENT_GRID_MIN_ITEMS;
    return grid ? K : 0;
}

// D~ on its own (dsg_debug_content_guide; the loop subtracts inside its update kernels): valid ? D - shift : 0, the node part at the
// label channels only
__global__ void content_apply_kernel(const float *__restrict__ D_adj, const float *__restrict__ D_node, const float *__restrict__ sh_adj,
                                     const float *__restrict__ sh_label, const uint8_t *__restrict__ flags, float *out_adj, float *out_node,
                                     Dims d, int Cl) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t na = (size_t)d.B * d.Ca * d.N * d.N, nn = (size_t)d.B * d.N * d.Cn;
    if (idx < na) {
        if (!out_adj) return;
        const int j = (int)(idx % d.N), i = (int)((idx / d.N) % d.N);
        const size_t b = idx / ((size_t)d.Ca * d.N * d.N);
        const bool v = flags[b * d.N + i] && flags[b * d.N + j];
        out_adj[idx] = v ? __fsub_rn(D_adj[idx], sh_adj[idx]) : 0.f;
    } else if (idx < na + nn) {
        if (!out_node) return;
        const size_t k = idx - na, row = k / d.Cn;
        const int ch = (int)(k % d.Cn);
        out_node[k] = !flags[row] ? 0.f : (ch < Cl ? __fsub_rn(D_node[k], sh_label[row * Cl + ch]) : D_node[k]);
    }
}
void launch_content_apply(const float *D_adj, const float *D_node, const float *sh_adj, const float *sh_label, const uint8_t *flags,
                          float *out_adj, float *out_node, int Cl, Dims d, hipStream_t s) {
    const size_t n = (size_t)d.B * ((size_t)d.Ca * d.N * d.N + (size_t)d.N * d.Cn);
    hipLaunchKernelGGL(content_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, D_adj, D_node, sh_adj, sh_label, flags, out_adj,
                       out_node, d, Cl);
}

}  // namespace dsg
