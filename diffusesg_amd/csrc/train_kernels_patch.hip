// train_kernels_patch.hip -- the edges of the training form at patch_size p > 1 (dsg_train_enable_patch).
//
// The blocks, PatchMerging and PatchBreakup of the training core run on a token resolution R = N / p as they are; what assumes one
// pixel per token is the way in (assembly, PatchEmbed's strided convolution) and the way out (read_out.0's transposed convolution, the
// masked adjacency store, the node pooling) and, for input gradients, the assembly's backward.  Token t = ti R + tj covers the pixels
// (I, J) = (p ti + a, p tj + b); rows of the read-out chain are in (token, a, b) order, m = (b_graph R^2 + t) p^2 + a p + b, as on the
// sampling path (kernels_patch.hip).  The raw weights are read in place in the reference's layouts and packed per call into weight
// images the existing t_gemm takes; their gradients are unpacked from images of the same layout.  Every mask is a select on the
// pixel's flags.  No atomics; every sum has one fixed order.  Launchers return false on refused arguments.
#include "kernels_common.hip.h"

namespace dsg {

static inline unsigned tp_blocks(size_t n) { return (unsigned)((n + 255) / 256); }
static inline bool tp_patch_ok(int N, int p) { return (p == 1 || p == 2 || p == 4) && N >= p && N % p == 0; }
static inline bool tp_grid_ok(size_t n) { return n >= 1 && (n + 255) / 256 <= 0x7fffffffull; }

// ---- PatchEmbed: patch_embed.proj.weight [E, Cin, p, p] <-> weight image [E, Kp], column (a p + b) Cin + c (launch_assemble_patch's
// order), zero from p^2 Cin up to Kp.  unpack reads the live columns only: whatever the pad columns of the gradient image hold stays there
__global__ void t_pe_pack_kernel(const float *__restrict__ W, float *__restrict__ img, int E, int Cin, int p, int Kp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)E * Kp) return;
    const int e = (int)(i / Kp), k = (int)(i % Kp);
    float v = 0.f;
    if (k < p * p * Cin) {
        const int sub = k / Cin, c = k % Cin;
        v = W[(((size_t)e * Cin + c) * p + sub / p) * p + sub % p];
    }
    img[i] = v;
}
__global__ void t_pe_unpack_kernel(const float *__restrict__ img, float *__restrict__ dW, int E, int Cin, int p, int Kp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)E * Cin * p * p) return;
    const int b = (int)(i % p), a = (int)((i / p) % p), c = (int)((i / ((size_t)p * p)) % Cin), e = (int)(i / ((size_t)p * p * Cin));
    dW[i] = img[(size_t)e * Kp + (a * p + b) * Cin + c];
}
int t_pe_image_width(int Cin, int p) { return (p * p * Cin + 31) / 32 * 32; }
bool t_pe_pack(const float *W, float *img, int E, int Cin, int p, int Kp, hipStream_t s) {
    if (!W || !img || E < 1 || Cin < 1 || (p != 1 && p != 2 && p != 4) || Kp < p * p * Cin || !tp_grid_ok((size_t)E * Kp)) return false;
    hipLaunchKernelGGL(t_pe_pack_kernel, dim3(tp_blocks((size_t)E * Kp)), dim3(256), 0, s, W, img, E, Cin, p, Kp);
    return true;
}
bool t_pe_unpack(const float *img, float *dW, int E, int Cin, int p, int Kp, hipStream_t s) {
    if (!img || !dW || E < 1 || Cin < 1 || (p != 1 && p != 2 && p != 4) || Kp < p * p * Cin || !tp_grid_ok((size_t)E * Kp)) return false;
    hipLaunchKernelGGL(t_pe_unpack_kernel, dim3(tp_blocks((size_t)E * Cin * p * p)), dim3(256), 0, s, img, dW, E, Cin, p, Kp);
    return true;
}

// ---- read_out.0: ConvTranspose2d weight [in, out, p, p] <-> weight image [in, p^2 out], column (a p + b) out + o, so that one product
// fy [B R^2, in] img writes the p^2 pixels of a token side by side; bias_rep [p^2 out] repeats the bias per sub-pixel (pack only)
__global__ void t_ro0_pack_kernel(const float *__restrict__ W, const float *__restrict__ bias, float *__restrict__ img,
                                  float *__restrict__ bias_rep, int Ei, int Eo, int p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int pp = p * p;
    if (i >= (size_t)Ei * pp * Eo) return;
    const int col = (int)(i % ((size_t)pp * Eo)), in = (int)(i / ((size_t)pp * Eo));
    const int sub = col / Eo, o = col % Eo;
    img[i] = W[(((size_t)in * Eo + o) * p + sub / p) * p + sub % p];
    if (in == 0 && bias_rep) bias_rep[col] = bias ? bias[o] : 0.f;
}
__global__ void t_ro0_unpack_kernel(const float *__restrict__ img, float *__restrict__ dW, int Ei, int Eo, int p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int pp = p * p;
    if (i >= (size_t)Ei * Eo * pp) return;
    const int b = (int)(i % p), a = (int)((i / p) % p), o = (int)((i / pp) % Eo), in = (int)(i / ((size_t)pp * Eo));
    dW[i] = img[(size_t)in * pp * Eo + (size_t)(a * p + b) * Eo + o];
}
bool t_ro0_pack(const float *W, const float *bias, float *img, float *bias_rep, int Ei, int Eo, int p, hipStream_t s) {
    if (!W || !img || Ei < 1 || Eo < 1 || (p != 1 && p != 2 && p != 4) || !tp_grid_ok((size_t)Ei * Eo * p * p)) return false;
    hipLaunchKernelGGL(t_ro0_pack_kernel, dim3(tp_blocks((size_t)Ei * Eo * p * p)), dim3(256), 0, s, W, bias, img, bias_rep, Ei, Eo, p);
    return true;
}
bool t_ro0_unpack(const float *img, float *dW, int Ei, int Eo, int p, hipStream_t s) {
    if (!img || !dW || Ei < 1 || Eo < 1 || (p != 1 && p != 2 && p != 4) || !tp_grid_ok((size_t)Ei * Eo * p * p)) return false;
    hipLaunchKernelGGL(t_ro0_unpack_kernel, dim3(tp_blocks((size_t)Ei * Eo * p * p)), dim3(256), 0, s, img, dW, Ei, Eo, p);
    return true;
}

// pixel (i, j) and graph b of row m in (token, a, b) order
__device__ __forceinline__ void tp_row_pixel(size_t m, int N, int p, int &b, int &i, int &j) {
    const int R = N / p, pp = p * p;
    const int sub = (int)(m % pp);
    const size_t tokg = m / pp;
    const int t = (int)(tokg % ((size_t)R * R));
    b = (int)(tokg / ((size_t)R * R));
    i = p * (t / R) + sub / p; j = p * (t % R) + sub % p;
}

// ---- adjacency head tail over rows in (token, a, b) order: F[b, c, I, J] = valid(I, J) ? oa[m][c] : 0, and its transpose
// d_oa[m][c] = valid(I, J) ? dF[b, c, I, J] : 0 (the p > 1 form of t_adj_out_kernel)
__global__ void t_adj_out_patch_kernel(const float *oa, const uint8_t *flags, float *F, const float *dF, float *d_oa, int N, int p, int Ca, size_t n,
                                       int bwd) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % Ca);
    int b, i, j;
    tp_row_pixel(idx / Ca, N, p, b, i, j);
    const bool ok = flags[(size_t)b * N + i] && flags[(size_t)b * N + j];
    const size_t k = (((size_t)b * Ca + c) * N + i) * N + j;
    if (bwd) d_oa[idx] = ok ? dF[k] : 0.f; else F[k] = ok ? oa[idx] : 0.f;
}
bool t_adj_out_patch(const float *oa, const uint8_t *flags, float *F, const float *dF, float *d_oa, int B, int N, int p, int Ca, bool bwd,
                     hipStream_t s) {
    if (B < 1 || Ca < 1 || !tp_patch_ok(N, p) || !flags || (bwd ? (!dF || !d_oa) : (!oa || !F))) return false;
    const size_t n = (size_t)B * N * N * Ca;
    if (!tp_grid_ok(n)) return false;
    hipLaunchKernelGGL(t_adj_out_patch_kernel, dim3(tp_blocks(n)), dim3(256), 0, s, oa, flags, F, dF, d_oa, N, p, Ca, n, (int)bwd);
    return true;
}

// ---- node pooling backward over rows in (token, a, b) order: d_rep[m][e] += valid(I, J) d_pool[(b, I)][e] / N -- the mean is over the
// N pixels of the row (forward: launch_pool_patch); accumulates into what the adjacency head's backward left
__global__ void t_pool_bwd_patch_kernel(const float *d_pool, const uint8_t *flags, float *d_rep_acc, int N, int p, int E, size_t n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int e = (int)(idx % E);
    int b, i, j;
    tp_row_pixel(idx / E, N, p, b, i, j);
    if (flags[(size_t)b * N + i] && flags[(size_t)b * N + j]) d_rep_acc[idx] += d_pool[((size_t)b * N + i) * E + e] / (float)N;
}
bool t_pool_bwd_patch(const float *d_pool, const uint8_t *flags, float *d_rep_acc, int B, int N, int p, int E, hipStream_t s) {
    if (B < 1 || E < 1 || !tp_patch_ok(N, p) || !d_pool || !flags || !d_rep_acc) return false;
    const size_t n = (size_t)B * N * N * E;
    if (!tp_grid_ok(n)) return false;
    hipLaunchKernelGGL(t_pool_bwd_patch_kernel, dim3(tp_blocks(n)), dim3(256), 0, s, d_pool, flags, d_rep_acc, N, p, E, n);
    return true;
}

// ---- input gradients: the live columns of PatchEmbed's weight image.  Per sub-pixel group g = a p + b the slots that multiply the
// CURRENT values (adj | node of the row | node of the column), G = Ca + 2 Cn wide: img [E][Np], column g G + slot, zero from p^2 G up to
// Np (a multiple of 32), so that d_tok = d_pe_lin img has p^2 groups per token (the p > 1 form of t_live_cols_kernel)
__global__ void t_live_cols_patch_kernel(const float *__restrict__ W, int Cin, int p, float *__restrict__ img, int E, int Np, int Ca, int Cn,
                                         int self_cond) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)E * Np) return;
    const int e = (int)(i / Np), col = (int)(i % Np), G = Ca + 2 * Cn, nsc = self_cond ? 2 : 1, sc = self_cond ? 1 : 0;
    float v = 0.f;
    if (col < p * p * G) {
        const int g = col / G, c = col % G;
        int src;
        if (c < Ca) src = sc * Ca + c;
        else if (c < Ca + Cn) src = nsc * Ca + sc * Cn + (c - Ca);
        else src = nsc * Ca + nsc * Cn + sc * Cn + (c - Ca - Cn);
        v = W[(((size_t)e * Cin + src) * p + g / p) * p + g % p];
    }
    img[i] = v;
}
int t_live_cols_patch_width(int Ca, int Cn, int p) { return (p * p * (Ca + 2 * Cn) + 31) / 32 * 32; }
bool t_live_cols_patch(const float *W, int Cin, int p, float *img, int E, int Ca, int Cn, bool self_cond, hipStream_t s) {
    if (!W || !img || E < 1 || Ca < 1 || Cn < 1 || (p != 1 && p != 2 && p != 4) || Cin != (self_cond ? 2 : 1) * (Ca + 2 * Cn)) return false;
    const int Np = t_live_cols_patch_width(Ca, Cn, p);
    hipLaunchKernelGGL(t_live_cols_patch_kernel, dim3(tp_blocks((size_t)E * Np)), dim3(256), 0, s, W, Cin, p, img, E, Np, Ca, Cn, (int)self_cond);
    return true;
}

// ---- the backward of assemble_patch_kernel fused with the preconditioning chain (the p > 1 form of t_assemble_bwd_kernel).
// d_tok [B R^2, ld] holds per token the p^2 groups of t_live_cols_patch; pixel (I, J) reads group (I mod p) p + J mod p of token
// (I / p, J / p).  With m the flags and g = dL/dD
//   out_adj[b,c,I,J] = c_skip_b m_I m_J g_adj[b,c,I,J] + c_in_b d_tok[pixel (I, J)][c]                  (the adjacency input is not masked)
//   out_node[b,I,c]  = m_I (c_skip_b g_node[b,I,c] + c_in_b (sum_J m_J d_tok[pixel (I, J)][Ca + c] + sum_J m_J d_tok[pixel (J, I)][Ca + Cn + c]))
// One block per (b, I).  Adjacency: 32 channels x 64 pixel columns go through an LDS tile, read channel-fastest and written
// column-fastest.  Node: work item (q, r), q one of the 2 Cn row / column slots, r one of PSUM_G interleaved groups of J; a thread adds
// its J ascending, the partials are added in order, the row sum before the column sum.  out_* may alias g_*.
constexpr int PASM_TC = 32, PASM_TJ = 64, PSUM_G = 8;
__global__ __launch_bounds__(256) void t_assemble_bwd_patch_kernel(const float *__restrict__ d_tok, int ld, const uint8_t *__restrict__ flags,
                                                                   const float *__restrict__ c_skip, const float *__restrict__ c_in,
                                                                   const float *g_adj, const float *g_node, float *out_adj, float *out_node,
                                                                   int N, int p, int Ca, int Cn) {
    extern __shared__ __attribute__((aligned(16))) float pasm_lds[];
    float *tile = pasm_lds;                           // [PASM_TC][PASM_TJ + 1]
    float *part = pasm_lds + PASM_TC * (PASM_TJ + 1); // [PSUM_G][2 Cn]
    const int b = blockIdx.x / N, i = blockIdx.x % N, tid = threadIdx.x;
    const int R = N / p, G = Ca + 2 * Cn, ti = i / p, a = i % p;
    const uint8_t *fl = flags + (size_t)b * N;
    const bool mi = fl[i] != 0;
    const float cs = c_skip[b], ci = c_in[b];
    const float *img = d_tok + (size_t)b * R * R * ld;           // the graph's tokens
    const float *row = img + (size_t)ti * R * ld + a * p * G;    // pixel (i, j): row[(j / p) ld + (j mod p) G + slot]
    const float *col = img + (size_t)ti * ld + a * G;            // pixel (j, i): col[(j / p) R ld + (j mod p) p G + slot]
    // ---- node sums: partials ----
    const int nq = 2 * Cn;
    for (int w = tid; w < nq * PSUM_G; w += 256) {
        const int q = w % nq, r = w / nq;
        float acc = 0.f;
        if (mi) {
            if (q < Cn) { for (int j = r; j < N; j += PSUM_G) if (fl[j]) acc += row[(size_t)(j / p) * ld + (j % p) * G + Ca + q]; }
            else { for (int j = r; j < N; j += PSUM_G) if (fl[j]) acc += col[(size_t)(j / p) * R * ld + (j % p) * p * G + Ca + q]; }
        }
        part[w] = acc;
    }
    // ---- adjacency: transpose through LDS ----
    for (int c0 = 0; c0 < Ca; c0 += PASM_TC)
        for (int j0 = 0; j0 < N; j0 += PASM_TJ) {
            __syncthreads();   // the previous tile has been read (and, the first time, nothing is pending)
            for (int k = tid; k < PASM_TC * PASM_TJ; k += 256) {
                const int c = k % PASM_TC, j = j0 + k / PASM_TC;
                if (c0 + c < Ca && j < N) tile[c * (PASM_TJ + 1) + k / PASM_TC] = row[(size_t)(j / p) * ld + (j % p) * G + c0 + c];
            }
            __syncthreads();
            for (int k = tid; k < PASM_TC * PASM_TJ; k += 256) {
                const int j = k % PASM_TJ, c = k / PASM_TJ;
                if (c0 + c < Ca && j0 + j < N) {
                    const size_t o = (((size_t)b * Ca + c0 + c) * N + i) * N + j0 + j;
                    const float skip = (mi && fl[j0 + j]) ? cs * g_adj[o] : 0.f;
                    out_adj[o] = skip + ci * tile[c * (PASM_TJ + 1) + j];
                }
            }
        }
    __syncthreads();   // part[] is complete
    for (int c = tid; c < Cn; c += 256) {
        const size_t o = ((size_t)b * N + i) * Cn + c;
        float srow = 0.f, scol = 0.f;
#pragma unroll
        for (int r = 0; r < PSUM_G; r++) { srow += part[r * nq + c]; scol += part[r * nq + Cn + c]; }
        out_node[o] = mi ? cs * g_node[o] + ci * (srow + scol) : 0.f;
    }
}
bool t_assemble_bwd_patch_ok(int Cn) { return Cn >= 1 && sizeof(float) * ((size_t)PASM_TC * (PASM_TJ + 1) + (size_t)PSUM_G * 2 * Cn) <= 64 * 1024; }
bool t_assemble_bwd_patch(const float *d_tok, int ld, const uint8_t *flags, const float *c_skip, const float *c_in, const float *g_adj,
                          const float *g_node, float *out_adj, float *out_node, int B, int N, int p, int Ca, int Cn, hipStream_t s) {
    if (B < 1 || Ca < 1 || !tp_patch_ok(N, p) || !t_assemble_bwd_patch_ok(Cn) || ld < p * p * (Ca + 2 * Cn) || (size_t)B * N > 0x7fffffffu) return false;
    if (!d_tok || !flags || !c_skip || !c_in || !g_adj || !g_node || !out_adj || !out_node) return false;
    const size_t lds = sizeof(float) * ((size_t)PASM_TC * (PASM_TJ + 1) + (size_t)PSUM_G * 2 * Cn);
    hipLaunchKernelGGL(t_assemble_bwd_patch_kernel, dim3((unsigned)(B * N)), dim3(256), lds, s, d_tok, ld, flags, c_skip, c_in, g_adj, g_node,
                       out_adj, out_node, N, p, Ca, Cn);
    return true;
}

}  // namespace dsg
