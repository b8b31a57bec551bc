// sgstat_kernels.hip -- the rest of the reference's after-sampling evaluation on the MI355X: the triplet histogram behind
// compute_triplet_tv_dist, the four per-layout metrics of compute_bbox_ioa (R/evaluation/blt_utils.py) and the row statistics
// of the F1 matrix (max, mean, median, arg-max) that sg_go_sampling reduces it to.
//
// Built with -ffp-contract=off: the box arithmetic of blt_utils.py is float32 op by op under NumPy and torch, and a fused
// multiply-add in `area_i + area_j - inter` would change the IoU of a pair.
//
// Determinism: integer counts use atomicAdd (the result does not depend on arrival order); every float64 sum is a per-thread
// sum in index order followed by a fixed tree over the block.  No atomics on floats.
#include "sgstat_kernels.h"

#include <limits.h>
#include <math.h>

namespace dsg {

// sum over the block of one value per thread, fixed tree; every thread gets the result.  `red` is reused: barrier on both sides.
template <typename T>
__device__ inline T block_sum256(T *red, T v) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// triplet counts: _get_triplet_type_hist (bbox_metrics.py:215-268) summed over the graphs
// ---------------------------------------------------------------------------------------------------------------------------
// Every non-zero entry of edge_types is a triplet (node_types[b,i], node_types[b,j], edge_types[b,i,j]); node flags are not
// consulted and the diagonal counts, as in the reference.  A value outside [0, 2^21) cannot be a key and counts as novel.
__global__ __launch_bounds__(256) void sgstat_triplet_kernel(size_t total, int N, const int32_t *__restrict__ edge,
                                                             const int32_t *__restrict__ node, int n_keys,
                                                             const int64_t *__restrict__ keys, const int32_t *__restrict__ pos,
                                                             unsigned long long *__restrict__ counts,
                                                             unsigned long long *__restrict__ novel) {
    __shared__ unsigned int blk_novel;
    if (threadIdx.x == 0) blk_novel = 0;
    __syncthreads();
    const size_t nn = (size_t)N * N;
    unsigned int mine = 0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int e = edge[idx];
        if (e == 0) continue;
        const size_t b = idx / nn;
        const int r = (int)(idx - b * nn), i = r / N, j = r - i * N;
        const int s = node[b * N + i], o = node[b * N + j];
        int hit = -1;
        if ((((uint32_t)s | (uint32_t)o | (uint32_t)e) >> kSgstatKeyBits) == 0) {
            const int64_t key = (int64_t)s << (2 * kSgstatKeyBits) | (int64_t)o << kSgstatKeyBits | (int64_t)e;
            int lo = 0, hi = n_keys;   // first index with keys[index] >= key
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n_keys && keys[lo] == key) hit = pos[lo];
        }
        if (hit >= 0) atomicAdd(&counts[hit], 1ull);
        else mine++;
    }
    if (mine) atomicAdd(&blk_novel, mine);
    __syncthreads();
    if (threadIdx.x == 0 && blk_novel) atomicAdd(novel, (unsigned long long)blk_novel);
}

// ---------------------------------------------------------------------------------------------------------------------------
// layout metrics: one block per layout, the flagged boxes compacted into LDS in node order
// ---------------------------------------------------------------------------------------------------------------------------
// _get_area (blt_utils.py:176-182): max(0., x1 - x0) * max(0., y1 - y0) in float32
__device__ inline float blt_area(float x0, float y0, float x1, float y1) { return fmaxf(0.f, x1 - x0) * fmaxf(0.f, y1 - y0); }

__global__ __launch_bounds__(256) void sgstat_layout_kernel(int B, int N, int canvas, const float4 *__restrict__ boxes,
                                                            const uint8_t *__restrict__ flags, double *__restrict__ values,
                                                            uint8_t *__restrict__ valid) {
    __shared__ float4 bx[256];
    __shared__ int4 px[256];
    __shared__ uint8_t fl[256];
    __shared__ double redd[256];
    __shared__ int redi[256];
    __shared__ int n_sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    fl[tid] = tid < N ? (uint8_t)(flags[(size_t)b * N + tid] != 0) : (uint8_t)0;
    __syncthreads();
    if (tid < N && fl[tid]) {
        int p = 0;
        for (int k = 0; k < tid; k++) p += fl[k];
        const float4 v = boxes[(size_t)b * N + tid];
        bx[p] = v;
        // get_perceptual_iou: layout *= canvas_size in float32, np.round (half to even), astype(int)
        const float c = (float)canvas;
        px[p] = make_int4((int)rintf(v.x * c), (int)rintf(v.y * c), (int)rintf(v.z * c), (int)rintf(v.w * c));
    }
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < N; k++) n += fl[k];
        n_sh = n;
    }
    __syncthreads();
    const int n = n_sh;

    // get_average_iou / get_overlap_index: pairs i < j; the pair terms are float32, their sums float64
    double s_iou = 0.0, s_ov = 0.0;
    int c_iou = 0, c_ov = 0;
    for (int p = tid; p < n * n; p += 256) {
        const int i = p / n, j = p - i * n;
        if (i >= j) continue;
        const float4 a = bx[i], q = bx[j];
        const float inter = blt_area(fmaxf(a.x, q.x), fmaxf(a.y, q.y), fminf(a.z, q.z), fminf(a.w, q.w));
        const float uni = blt_area(a.x, a.y, a.z, a.w) + blt_area(q.x, q.y, q.z, q.w) - inter;
        const float iou = fabs((double)uni) <= 1e-8 ? 0.f : inter / uni;   // np.isclose(union, 0.): float64 |union| <= atol
        if (iou > 0.f) { s_iou += (double)iou; c_iou++; }
        if (inter > 0.f) { s_ov += (double)inter; c_ov++; }
    }
    s_iou = block_sum256(redd, s_iou);
    s_ov = block_sum256(redd, s_ov);
    c_iou = block_sum256(redi, c_iou);
    c_ov = block_sum256(redi, c_ov);

    // get_perceptual_iou: pixel (x, y) is covered by a box when min_x <= x < max_x and min_y <= y < max_y
    int over = 0, cov = 0;
    for (int p = tid; p < canvas * canvas; p += 256) {
        const int x = p / canvas, y = p - x * canvas;
        int c = 0;
        for (int k = 0; k < n && c < 2; k++) {
            const int4 r = px[k];
            c += r.x <= x && x < r.z && r.y <= y && y < r.w;
        }
        cov += c > 0;
        over += c > 1;
    }
    over = block_sum256(redi, over);
    cov = block_sum256(redi, cov);

    // get_alignment_loss: per box the smallest of the left / centre / right distances to any other box (float32 means of two
    // absolute differences), summed in float64
    double al = 0.0;
    if (tid < n && n >= 2) {
        const float4 a = bx[tid];
        const float acx = (a.x + a.z) / 2.f, acy = (a.y + a.w) / 2.f;
        float m = INFINITY;
        for (int k = 0; k < n; k++) {
            if (k == tid) continue;
            const float4 q = bx[k];
            const float left = (fabsf(a.x - q.x) + fabsf(a.y - q.y)) / 2.f;
            const float centre = (fabsf(acx - (q.x + q.z) / 2.f) + fabsf(acy - (q.y + q.w) / 2.f)) / 2.f;
            const float right = (fabsf(a.z - q.z) + fabsf(a.w - q.w)) / 2.f;
            m = fminf(m, fminf(left, fminf(centre, right)));
        }
        al = (double)m;
    }
    al = block_sum256(redd, al);

    if (tid == 0) {
        const size_t sB = (size_t)B;
        values[0 * sB + b] = c_iou > 0 ? s_iou / (double)c_iou : 0.0;
        valid[0 * sB + b] = c_iou > 0;
        values[1 * sB + b] = (n >= 2 && cov > 0) ? (double)over / (double)cov : 0.0;
        valid[1 * sB + b] = n >= 2 && cov > 0;
        values[2 * sB + b] = c_ov > 0 ? s_ov : 0.0;
        valid[2 * sB + b] = c_ov > 0;
        values[3 * sB + b] = n >= 2 ? al : 0.0;
        valid[3 * sB + b] = n >= 2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// F1 row statistics: one block per (row, weight); the row sits in LDS, the median is an exact radix select
// ---------------------------------------------------------------------------------------------------------------------------
// order-preserving map of a non-NaN double onto uint64
__device__ inline uint64_t f64_key(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double f64_unkey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(256) void sgstat_rowstats_kernel(int Y, int W, const double *__restrict__ blk, double *__restrict__ omax,
                                                              double *__restrict__ omean, double *__restrict__ omed,
                                                              int32_t *__restrict__ oarg) {
    extern __shared__ double row[];   // [Y]
    __shared__ double redd[256];
    __shared__ int redi[256];
    __shared__ uint64_t redk[256];
    __shared__ unsigned int hist[256];
    __shared__ uint64_t prefix_sh;
    __shared__ int k_sh;
    const int tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * W + blockIdx.y;
    const double *src = blk + (size_t)blockIdx.x * Y * W + blockIdx.y;

    double sum = 0.0, mx = -INFINITY;
    int arg = INT_MAX, nan_at = INT_MAX;
    for (int y = tid; y < Y; y += 256) {
        const double v = src[(size_t)y * W];
        row[y] = v;
        sum += v;
        if (v != v) { if (nan_at == INT_MAX) nan_at = y; }
        else if (arg == INT_MAX || v > mx) { mx = v; arg = y; }
    }
    // first NaN of the row (np.max / np.mean / np.median give NaN then, np.argmax its index)
    __syncthreads();
    redi[tid] = nan_at;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) redi[tid] = min(redi[tid], redi[tid + w]);
        __syncthreads();
    }
    nan_at = redi[0];
    if (nan_at != INT_MAX) {   // block-uniform
        if (tid == 0) {
            omax[o] = omean[o] = omed[o] = NAN;
            oarg[o] = nan_at;
        }
        return;
    }
    sum = block_sum256(redd, sum);
    // maximum and its first index
    __syncthreads();
    redd[tid] = mx;
    redi[tid] = arg;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const double v = redd[tid + w];
            const int a = redi[tid + w];
            if (v > redd[tid] || (v == redd[tid] && a < redi[tid])) { redd[tid] = v; redi[tid] = a; }
        }
        __syncthreads();
    }
    mx = redd[0];
    arg = redi[0];

    // k-th smallest (k = (Y - 1) / 2) by an 8-bit radix select from the top byte down
    const int k_lo = (Y - 1) / 2, k_hi = Y / 2;
    uint64_t prefix = 0;
    int k = k_lo;
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 56 - 8 * pass;
        __syncthreads();
        hist[tid] = 0;
        __syncthreads();
        for (int y = tid; y < Y; y += 256) {
            const uint64_t u = f64_key(row[y]);
            if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(u >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int c = 0, d = 0;
            for (; d < 255; d++) {
                if (k < c + (int)hist[d]) break;
                c += (int)hist[d];
            }
            k_sh = k - c;
            prefix_sh = prefix | (uint64_t)d << shift;
        }
        __syncthreads();
        k = k_sh;
        prefix = prefix_sh;
    }
    const double v_lo = f64_unkey(prefix);
    double v_hi = v_lo;
    if (k_hi != k_lo) {
        // the next order statistic: v_lo again when enough elements are <= v_lo, else the smallest element above it
        int le = 0;
        uint64_t nxt = ~0ull;
        for (int y = tid; y < Y; y += 256) {
            const uint64_t u = f64_key(row[y]);
            if (u <= prefix) le++;
            else if (u < nxt) nxt = u;
        }
        le = block_sum256(redi, le);
        __syncthreads();
        redk[tid] = nxt;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w && redk[tid + w] < redk[tid]) redk[tid] = redk[tid + w];
            __syncthreads();
        }
        if (le < k_hi + 1) v_hi = f64_unkey(redk[0]);
    }
    if (tid == 0) {
        omax[o] = mx;
        omean[o] = sum / (double)Y;
        omed[o] = k_hi != k_lo ? (v_lo + v_hi) / 2.0 : v_lo;
        oarg[o] = arg;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// launchers (arguments are validated by sgstat_api.cpp)
// ---------------------------------------------------------------------------------------------------------------------------
void launch_sgstat_triplet_counts(int B, int N, const int32_t *edge_types, const int32_t *node_types, int n_keys,
                                  const int64_t *sorted_keys, const int32_t *key_pos, int64_t *counts, int64_t *novel, hipStream_t s) {
    const size_t total = (size_t)B * N * N;
    const size_t want = (total + 255) / 256;
    const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(sgstat_triplet_kernel, dim3(blocks), dim3(256), 0, s, total, N, edge_types, node_types, n_keys, sorted_keys,
                       key_pos, reinterpret_cast<unsigned long long *>(counts), reinterpret_cast<unsigned long long *>(novel));
}

void launch_sgstat_layout(int B, int N, const float *boxes, const uint8_t *flags, int canvas, double *values, uint8_t *valid,
                          hipStream_t s) {
    hipLaunchKernelGGL(sgstat_layout_kernel, dim3(B), dim3(256), 0, s, B, N, canvas, reinterpret_cast<const float4 *>(boxes), flags,
                       values, valid);
}

bool launch_sgstat_f1_rowstats(int rows, int Y, int W, const double *blk, double *row_max, double *row_mean, double *row_median,
                               int32_t *row_argmax, hipStream_t s) {
    const size_t lds = sizeof(double) * (size_t)Y;
    // rows beyond the default 64 KiB of dynamic LDS
    if (lds > 32768 && hipFuncSetAttribute((const void *)sgstat_rowstats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(double) * kSgstatMaxRow)) != hipSuccess)
        return false;
    hipLaunchKernelGGL(sgstat_rowstats_kernel, dim3(rows, W), dim3(256), lds, s, Y, W, blk, row_max, row_mean, row_median, row_argmax);
    return true;
}

}  // namespace dsg
