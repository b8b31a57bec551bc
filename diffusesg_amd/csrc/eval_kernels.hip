// eval_kernels.hip -- sample evaluation on the MI355X: the bounding-box F1 matrix and the histogram MMDs of the reference's
// SceneGraphEvaluator (R/evaluation/bbox_metrics.py), which runs them on the CPU after sampling.
//
// Built with -ffp-contract=off: the Pascal-VOC IoU of R/evaluation/bbox_utils.py:703-747 is float32 op by op under NumPy 2
// (np.float32 boxes, Python-int "+1", `interArea / float(union)` stays float32), and a fused multiply-add in the areas would
// change which side of an IoU threshold a box lands on.
//
// F1 of one (generated, reference) scene pair, measure_two_sets_of_bboxes (bbox_metrics.py:64-115) with GetPascalVOCMetrics
// (bbox_utils.py:338-460) read for what it does here:
//   - imageName = str(node index): the detection of node i can only meet the ground truth of node i, and only in its own class;
//     one box per image and class, so a match is a TP exactly when iou > 0 and iou >= threshold.
//   - every confidence is 1.0 and the sort is stable, so detections of a class are scored in node order: with ndet detections,
//     npos ground truths and TP ranks r_k,  mean(precision) = sum_k (H(ndet) - H(r_k)) / ndet,
//                                           mean(recall)    = sum_k (ndet - r_k) / (ndet * npos).
//   - F1 = 2PR / max(P + R, 1e-6), 0 for a class without TP (AP == 0 exactly then); classes are the union of both scenes;
//     weights are normalised over that union; no common class -> 0.  Mean over the IoU thresholds.
//   - the generated boxes went through BoundingBoxes.clone() (XYX2Y2 -> XYWH -> XYX2Y2): x2' = x1 + (x2 - x1) in float32.
// The pair kernel walks the generated scene's boxes in (class, node) order, so a class's sums are finished when its run ends and no
// per-class arrays are needed.  Sums are float64 in a fixed order; no atomics on floats anywhere in this file.
#include "eval_kernels.h"

#include <math.h>

namespace dsg {

// ---------------------------------------------------------------------------------------------------------------------------
// per-scene prep: one block per scene, one thread per node
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_bbox_prep_kernel(int S, int N, int C, const float4 *__restrict__ boxes,
                                                             const int32_t *__restrict__ classes, const uint8_t *__restrict__ flags,
                                                             int W, const double *__restrict__ weights, uint8_t *__restrict__ prep) {
    const int s = blockIdx.x, i = threadIdx.x;
    const EvalPrepLayout L = eval_prep_layout(S, N, W);
    __shared__ int cl[256];
    __shared__ int cnt[kEvalMaxClasses];
    __shared__ double harm[kEvalMaxNodes + 1];

    int c = -1;
    if (i < N) {
        const size_t k = (size_t)s * N + i;
        const float4 b = boxes[k];
        const int t = classes[k];
        // collect_bounding_box_per_scene (bbox_metrics.py:32-34): flag set and x >= 0, y >= 0, "w" = x2 > 0, "h" = y2 > 0
        if (flags[k] != 0 && b.x >= 0.f && b.y >= 0.f && b.z > 0.f && b.w > 0.f && t >= 0 && t < C) c = t;
        reinterpret_cast<float4 *>(prep + L.box)[(size_t)i * S + s] = b;
        reinterpret_cast<int32_t *>(prep + L.cls)[(size_t)i * S + s] = c;
    }
    cl[i] = c;
    if (i == 0) {
        harm[0] = 0.0;
        for (int k = 1; k <= N; k++) harm[k] = harm[k - 1] + 1.0 / k;
    }
    __syncthreads();

    if (c >= 0) {
        int rank = 0, ndet = 0, pos = 0;
        for (int j = 0; j < N; j++) {
            const int cj = cl[j];
            if (cj < 0) continue;
            ndet += cj == c;
            rank += cj == c && j < i;
            pos += cj < c || (cj == c && j < i);
        }
        const size_t e = (size_t)s * N + pos;
        reinterpret_cast<uint32_t *>(prep + L.ent)[e] = (uint32_t)i | (uint32_t)c << 8 | (uint32_t)rank << 16 | (uint32_t)ndet << 24;
        reinterpret_cast<double *>(prep + L.ep)[e] = (harm[ndet] - harm[rank]) / ndet;
        reinterpret_cast<double *>(prep + L.er)[e] = (double)(ndet - rank) / ndet;
    }
    for (int k = i; k < kEvalMaxClasses; k += blockDim.x) {
        int n = 0;
        for (int j = 0; j < N; j++) n += cl[j] == k;
        cnt[k] = n;
        prep[L.cnt + (size_t)k * S + s] = (uint8_t)n;
    }
    __syncthreads();
    if (i < kEvalMaskWords) {
        uint32_t m = 0;
        for (int b = 0; b < 32; b++) m |= (cnt[32 * i + b] > 0 ? 1u : 0u) << b;
        reinterpret_cast<uint32_t *>(prep + L.mask)[(size_t)i * S + s] = m;
    }
    if (i < W) {
        double sw = 0.0;   // ascending class order
        for (int k = 0; k < C; k++)
            if (cnt[k] > 0) sw += weights ? weights[(size_t)i * C + k] : 1.0;
        reinterpret_cast<double *>(prep + L.sw)[(size_t)s * W + i] = sw;
    }
    if (i == 0) {
        int n = 0;
        for (int k = 0; k < C; k++) n += cnt[k];
        reinterpret_cast<int32_t *>(prep + L.nval)[s] = n;
    }
}

// Evaluator.iou (bbox_utils.py:703-747) on float32, A = detection (generated), B = ground truth (reference)
__device__ inline float pascal_iou(float4 a, float4 b) {
    if (a.x > b.z || b.x > a.z || a.w < b.y || a.y > b.w) return 0.f;   // _boxesIntersect: strict comparisons
    const float xA = fmaxf(a.x, b.x), yA = fmaxf(a.y, b.y), xB = fminf(a.z, b.z), yB = fminf(a.w, b.w);
    const float inter = (xB - xA + 1.f) * (yB - yA + 1.f);
    const float areaA = (a.z - a.x + 1.f) * (a.w - a.y + 1.f);
    const float areaB = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
    const float uni = areaA + areaB - inter;
    return inter / uni;
}

// ---------------------------------------------------------------------------------------------------------------------------
// pair kernel: block = 4 generated scenes (one per wave, so a wave's loop is uniform) x 64 reference scenes (one per lane)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_bbox_f1_kernel(const uint8_t *__restrict__ gp, int X, const uint8_t *__restrict__ rp, int Y,
                                                           int N, int C, int W, const double *__restrict__ weights, EvalIou iou,
                                                           int x0, int x1, int y0, int y1, double *__restrict__ out) {
    const int x = __builtin_amdgcn_readfirstlane(x0 + (int)blockIdx.y * 4 + (int)threadIdx.y);
    if (x >= x1) return;
    const int y = y0 + (int)blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = y < y1;
    const int yr = live ? y : y1 - 1;
    const EvalPrepLayout G = eval_prep_layout(X, N, W), R = eval_prep_layout(Y, N, W);
    const float4 *gbox = reinterpret_cast<const float4 *>(gp + G.box);
    const uint32_t *gent = reinterpret_cast<const uint32_t *>(gp + G.ent) + (size_t)x * N;
    const double *gep = reinterpret_cast<const double *>(gp + G.ep) + (size_t)x * N;
    const double *ger = reinterpret_cast<const double *>(gp + G.er) + (size_t)x * N;
    const float4 *rbox = reinterpret_cast<const float4 *>(rp + R.box);
    const int32_t *rcls = reinterpret_cast<const int32_t *>(rp + R.cls);
    const uint32_t *rmask = reinterpret_cast<const uint32_t *>(rp + R.mask);
    const uint8_t *rcnt = rp + R.cnt;
    const int nv = reinterpret_cast<const int32_t *>(gp + G.nval)[x];

    double sP[kEvalMaxIou], sR[kEvalMaxIou], acc[kEvalMaxWeights], sint[kEvalMaxWeights];
#pragma unroll
    for (int t = 0; t < kEvalMaxIou; t++) sP[t] = sR[t] = 0.0;
#pragma unroll
    for (int v = 0; v < kEvalMaxWeights; v++) acc[v] = sint[v] = 0.0;
    bool tp = false, common = false;

    uint32_t en = nv > 0 ? gent[0] : 0u;
    for (int e = 0; e < nv; e++) {
        const uint32_t nx = e + 1 < nv ? gent[e + 1] : 0xffffffffu;
        const int i = en & 0xff, c = (en >> 8) & 0xff;
        if (rcls[(size_t)i * Y + yr] == c) {
            float4 a = gbox[(size_t)i * X + x];
            a.z = a.x + (a.z - a.x);   // BoundingBox.clone() round trip of the detections
            a.w = a.y + (a.w - a.y);
            const float q = pascal_iou(a, rbox[(size_t)i * Y + yr]);
            if (q > 0.f) {   // `iou > iouMax` with iouMax = sys.float_info.min
                const double dq = q, ep = gep[e], er = ger[e];
#pragma unroll
                for (int t = 0; t < kEvalMaxIou; t++)
                    if (t < iou.n && dq >= iou.thr[t]) { sP[t] += ep; sR[t] += er; tp = true; }
            }
        }
        if (((nx >> 8) & 0xff) != (uint32_t)c || e + 1 == nv) {   // last detection of class c (wave-uniform)
            if ((rmask[(size_t)(c >> 5) * Y + yr] >> (c & 31)) & 1u) {
                common = true;
#pragma unroll
                for (int v = 0; v < kEvalMaxWeights; v++)
                    if (v < W) sint[v] += weights ? weights[(size_t)v * C + c] : 1.0;
            }
            if (tp) {
                const double npos = rcnt[(size_t)c * Y + yr];
                double g = 0.0;
#pragma unroll
                for (int t = 0; t < kEvalMaxIou; t++) {
                    if (t < iou.n && sR[t] > 0.0) {
                        const double P = sP[t], Rc = sR[t] / npos;
                        g += 2.0 * P * Rc / fmax(P + Rc, 1e-6);
                    }
                    sP[t] = sR[t] = 0.0;
                }
#pragma unroll
                for (int v = 0; v < kEvalMaxWeights; v++)
                    if (v < W) acc[v] += (weights ? weights[(size_t)v * C + c] : 1.0) * g;
                tp = false;
            }
        }
        en = nx;
    }
    if (!live) return;
    const double *gsw = reinterpret_cast<const double *>(gp + G.sw) + (size_t)x * W;
    const double *rsw = reinterpret_cast<const double *>(rp + R.sw) + (size_t)yr * W;
    double *o = out + ((size_t)(x - x0) * (y1 - y0) + (y - y0)) * W;
#pragma unroll
    for (int v = 0; v < kEvalMaxWeights; v++)
        if (v < W) o[v] = common ? acc[v] / (gsw[v] + rsw[v] - sint[v]) / iou.n : 0.0;   // weight sum over the class union
}

// ---------------------------------------------------------------------------------------------------------------------------
// histograms: one block per graph; integer counts in LDS, normalised as the reference does (compute_mmd, mmd.py:152-153)
// ---------------------------------------------------------------------------------------------------------------------------
// _get_node_type_hist / _get_edge_type_hist (bbox_metrics.py:181-216): torch.histogram over [-1, K] with K+1 unit bins of the
// masked types; a type equal to K lands in the closed last bin.  The float32 histogram is normalised in float32.
__global__ __launch_bounds__(256) void eval_type_hist_kernel(int B, int N, int K, int edges, const int32_t *__restrict__ types,
                                                             const uint8_t *__restrict__ flags, double *__restrict__ hist, int ld,
                                                             double *__restrict__ sums) {
    __shared__ int cnt[kEvalMaxTypes];
    __shared__ int total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = edges ? K - 1 : K;
    for (int k = tid; k < nb; k += blockDim.x) cnt[k] = 0;
    __syncthreads();
    const uint8_t *f = flags + (size_t)b * N;
    if (!edges) {
        for (int i = tid; i < N; i += blockDim.x) {
            if (!f[i]) continue;
            const int t = types[(size_t)b * N + i];
            if (t >= 0 && t <= K) atomicAdd(&cnt[t < K ? t : K - 1], 1);
        }
    } else {
        const int32_t *tb = types + (size_t)b * N * N;
        for (int idx = tid; idx < N * N; idx += blockDim.x) {
            if (!f[idx / N] || !f[idx % N]) continue;
            const int t = tb[idx];
            if (t >= 1 && t <= K) atomicAdd(&cnt[t < K ? t - 1 : K - 2], 1);   // types 1..K-1 (0 = no edge)
        }
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < nb; k++) n += cnt[k];
        total = n;
        sums[b] = n;
    }
    __syncthreads();
    const int n = total;
    for (int k = tid; k < nb; k += blockDim.x)
        hist[(size_t)k * ld + b] = n ? (double)((float)cnt[k] / (float)n) : (double)cnt[k];
}

// adjs_to_graphs + nx.degree_histogram (stats.py:23-60, 180-194): an undirected edge wherever adj[i,j] or adj[j,i] is non-zero,
// i != j; isolated nodes removed; a graph left empty is one node of degree 0.  Integer histogram, normalised in float64.
__global__ __launch_bounds__(256) void eval_degree_hist_kernel(int B, int N, const float *__restrict__ adj, double *__restrict__ hist,
                                                               int ld, double *__restrict__ sums) {
    __shared__ int cnt[kEvalMaxTypes];
    __shared__ int total;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < N; k += blockDim.x) cnt[k] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    const float *A = adj + (size_t)b * N * N;
    for (int i = tid; i < N; i += blockDim.x) {
        int d = 0;
        for (int j = 0; j < N; j++) d += j != i && (A[(size_t)i * N + j] != 0.f || A[(size_t)j * N + i] != 0.f);
        if (d > 0) {
            atomicAdd(&cnt[d], 1);
            atomicAdd(&total, 1);
        }
    }
    __syncthreads();
    if (tid == 0 && total == 0) { cnt[0] = 1; total = 1; }
    __syncthreads();
    const int n = total;
    if (tid == 0) sums[b] = n;
    for (int k = tid; k < N; k += blockDim.x) hist[(size_t)k * ld + b] = (double)cnt[k] / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Gaussian-kernel Gram sums: disc(P, Q) = mean_ij exp(-|p_i - q_j|^2 / 2) (mmd.py:70-84, 110-161), histograms [L][n]
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kGramRows = 4;

// One block = kGramRows rows of one of the three products (ref x ref, gen x gen, ref x gen); writes each row's sum over Q.
__global__ __launch_bounds__(256) void eval_gram_rows_kernel(int nR, const double *__restrict__ Rh, int ldR, int nG,
                                                             const double *__restrict__ Gh, int ldG, int L, double *__restrict__ ws) {
    extern __shared__ double pv[];   // [kGramRows][L]
    __shared__ double red[kGramRows][256];
    const int bR = (nR + kGramRows - 1) / kGramRows, bG = (nG + kGramRows - 1) / kGramRows;
    int blk = blockIdx.x, seg;
    if (blk < bR) seg = 0;
    else if (blk < bR + bG) { seg = 1; blk -= bR; }
    else { seg = 2; blk -= bR + bG; }
    const double *P = seg == 1 ? Gh : Rh, *Q = seg == 0 ? Rh : Gh;
    const int ldP = seg == 1 ? ldG : ldR, ldQ = seg == 0 ? ldR : ldG;
    const int nP = seg == 1 ? nG : nR, nQ = seg == 0 ? nR : nG;
    const int r0 = blk * kGramRows, tid = threadIdx.x;
    for (int idx = tid; idx < kGramRows * L; idx += blockDim.x) {
        const int r = idx / L, k = idx % L;
        pv[idx] = r0 + r < nP ? P[(size_t)k * ldP + r0 + r] : 0.0;
    }
    __syncthreads();
    double acc[kGramRows];
#pragma unroll
    for (int r = 0; r < kGramRows; r++) acc[r] = 0.0;
    for (int j = tid; j < nQ; j += blockDim.x) {
        double s[kGramRows];
#pragma unroll
        for (int r = 0; r < kGramRows; r++) s[r] = 0.0;
        for (int k = 0; k < L; k++) {
            const double q = Q[(size_t)k * ldQ + j];
#pragma unroll
            for (int r = 0; r < kGramRows; r++) {
                const double d = pv[r * L + k] - q;
                s[r] += d * d;
            }
        }
#pragma unroll
        for (int r = 0; r < kGramRows; r++) {
            const double dist = sqrt(s[r]);   // np.linalg.norm, then dist * dist as gaussian() does
            acc[r] += exp(-dist * dist / 2.0);
        }
    }
#pragma unroll
    for (int r = 0; r < kGramRows; r++) red[r][tid] = acc[r];
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int r = 0; r < kGramRows; r++) red[r][tid] += red[r][tid + w];
        __syncthreads();
    }
    if (tid < kGramRows && r0 + tid < nP) {
        const size_t off = seg == 0 ? 0 : seg == 1 ? (size_t)nR : (size_t)nR + nG;
        ws[off + r0 + tid] = red[tid][0];
    }
}

// out = {mmd, disc(ref, ref), disc(gen, gen), disc(ref, gen)}: compute_mmd's disc(s1,s1) + disc(s2,s2) - 2 disc(s1,s2), s1 = ref
__global__ __launch_bounds__(256) void eval_mmd_final_kernel(int nR, int nG, const double *__restrict__ ws, double *__restrict__ out) {
    __shared__ double red[256];
    __shared__ double disc[3];
    const int tid = threadIdx.x;
    for (int seg = 0; seg < 3; seg++) {
        const size_t off = seg == 0 ? 0 : seg == 1 ? (size_t)nR : (size_t)nR + nG;
        const int n = seg == 1 ? nG : nR;
        double a = 0.0;
        for (int i = tid; i < n; i += blockDim.x) a += ws[off + i];
        red[tid] = a;
        __syncthreads();
        for (int w = blockDim.x / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            const double n1 = seg == 1 ? nG : nR, n2 = seg == 0 ? nR : nG;
            disc[seg] = red[0] / (n1 * n2);
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = disc[0] + disc[1] - 2.0 * disc[2];
        out[1] = disc[0];
        out[2] = disc[1];
        out[3] = disc[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// launchers (arguments are validated by eval_api.cpp)
// ---------------------------------------------------------------------------------------------------------------------------
void launch_eval_bbox_prep(int S, int N, int C, const float *boxes, const int32_t *classes, const uint8_t *flags, int W,
                           const double *weights, void *prep, hipStream_t s) {
    hipLaunchKernelGGL(eval_bbox_prep_kernel, dim3(S), dim3(256), 0, s, S, N, C, reinterpret_cast<const float4 *>(boxes), classes, flags,
                       W, weights, static_cast<uint8_t *>(prep));
}

void launch_eval_bbox_f1(const void *gen_prep, int X, const void *ref_prep, int Y, int N, int C, int W, const double *weights,
                         const EvalIou &iou, int x0, int x1, int y0, int y1, double *out, hipStream_t s) {
    const dim3 grid((unsigned)((y1 - y0 + 63) / 64), (unsigned)((x1 - x0 + 3) / 4));
    hipLaunchKernelGGL(eval_bbox_f1_kernel, grid, dim3(64, 4), 0, s, static_cast<const uint8_t *>(gen_prep), X,
                       static_cast<const uint8_t *>(ref_prep), Y, N, C, W, weights, iou, x0, x1, y0, y1, out);
}

void launch_eval_type_hist(int B, int N, int K, int edges, const int32_t *types, const uint8_t *flags, double *hist, int ld,
                           double *sums, hipStream_t s) {
    hipLaunchKernelGGL(eval_type_hist_kernel, dim3(B), dim3(256), 0, s, B, N, K, edges, types, flags, hist, ld, sums);
}

void launch_eval_degree_hist(int B, int N, const float *adj, double *hist, int ld, double *sums, hipStream_t s) {
    hipLaunchKernelGGL(eval_degree_hist_kernel, dim3(B), dim3(256), 0, s, B, N, adj, hist, ld, sums);
}

void launch_eval_hist_mmd(int n_ref, const double *ref, int ld_ref, int n_gen, const double *gen, int ld_gen, int L, double *ws,
                          double *out, hipStream_t s) {
    const int blocks = 2 * ((n_ref + kGramRows - 1) / kGramRows) + (n_gen + kGramRows - 1) / kGramRows;
    hipLaunchKernelGGL(eval_gram_rows_kernel, dim3(blocks), dim3(256), sizeof(double) * kGramRows * L, s, n_ref, ref, ld_ref, n_gen, gen,
                       ld_gen, L, ws);
    hipLaunchKernelGGL(eval_mmd_final_kernel, dim3(1), dim3(256), 0, s, n_ref, n_gen, ws, out);
}

}  // namespace dsg
