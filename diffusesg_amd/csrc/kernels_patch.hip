// kernels_patch.hip -- the edge kernels of the patch_size > 1 forward (include/dsg.h: dsg_create_patch).
//
// With p = patch_size the U-Net runs on R x R tokens, R = N / p; token t = ti R + tj covers the pixels (I, J) = (p ti + a, p tj + b).
// PatchEmbed's strided convolution becomes one GEMM over rows that hold the p^2 sub-pixels' channels side by side
// (assemble_patch_kernel), the read-out's transposed convolution one GEMM with p^2 E output columns, whose [B R^2, p^2 E] result is
// read as rows in (token, a, b) order: row m = (b R^2 + t) p^2 + a p + b.  The per-pixel 1 x 1 products behind it do not care about
// the row order; only the masked adjacency store (head_adj_patch_kernel) and the node pooling (pool_patch_kernel) carry the
// (token, a, b) -> (I, J) map.  Every mask is a select on the PIXEL's flags (flag_I && flag_J), never a product.
#include "kernels_common.hip.h"

namespace dsg {

// Input assembly at patch_size p: out [B R^2, Kp], k = (a p + b) Cin + c with c in assemble_kernel's channel order
// [sc_adj, adj, sc_node(i), node(i), sc_node(j), node(j)] of pixel (p ti + a, p tj + b); zero from p^2 Cin up to Kp.
__global__ void assemble_patch_kernel(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                                      const uint8_t *flags, float *out, int B, int N, int p, int Ca, int Cn, int self_cond, int Kp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int R = N / p;
    const size_t total = (size_t)B * R * R * Kp;
    if (idx >= total) return;
    const int k = idx % Kp;
    const size_t tokg = idx / Kp;
    const int tj = tokg % R, ti = (tokg / R) % R, b = tokg / ((size_t)R * R);
    const bool sc_on = self_cond && (has_sc == nullptr || *has_sc != 0) && sc_adj != nullptr;
    const int nsc = self_cond ? 2 : 1, Cin = nsc * (Ca + 2 * Cn);
    float v = 0.f;
    if (k < p * p * Cin) {
        const int sub = k / Cin, c = k % Cin;
        const int i = p * ti + sub / p, j = p * tj + sub % p;
        if (c < nsc * Ca) {
            const int which = self_cond ? c / Ca : 1, a = c % Ca;  // 0 = self-cond copy, 1 = current
            const float *src = (which == 0) ? (sc_on ? sc_adj : nullptr) : adj;
            if (src) v = src[(((size_t)b * Ca + a) * N + i) * N + j];
        } else {
            const int cc = c - nsc * Ca;
            const int colpart = cc / (nsc * Cn);  // 0: node_mat (row index i), 1: node_mat_t (column index j)
            const int c2 = cc % (nsc * Cn);
            const int which = self_cond ? c2 / Cn : 1, a = c2 % Cn;
            const int nodei = colpart ? j : i;
            const float *src = (which == 0) ? (sc_on ? sc_node : nullptr) : node;
            const bool m = flags[(size_t)b * N + i] && flags[(size_t)b * N + j];
            if (src && m) v = src[((size_t)b * N + nodei) * Cn + a];
        }
    }
    out[idx] = v;
}
bool launch_assemble_patch(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                           const uint8_t *flags, float *out, int B, int N, int p, int Ca, int Cn, int self_cond, int Kp, hipStream_t s) {
    if (B < 1 || p < 1 || N < p || N % p != 0 || Ca < 1 || Cn < 1 || Kp < p * p * (self_cond ? 2 : 1) * (Ca + 2 * Cn)) return false;
    const size_t total = (size_t)B * (N / p) * (N / p) * Kp;
    if ((total + 255) / 256 > 0x7fffffffull) return false;
    DSG_LAUNCH(assemble_patch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, adj, node, sc_adj, sc_node, has_sc, flags, out,
               B, N, p, Ca, Cn, self_cond, Kp);
    return true;
}

// Adjacency head tail over rows in (token, a, b) order: out[b][c][I][J] = valid(I, J) ? h[m] . W[c] + bias[c] : 0
// one wave per row: lanes split the E-long dot product
__global__ __launch_bounds__(256) void head_adj_patch_kernel(const float *h, const float *W, const float *bias, const uint8_t *flags,
                                                             float *out, int N, int p, int E, int Ca, int M) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int R = N / p, pp = p * p;
    const int sub = m % pp, tokg = m / pp, t = tokg % (R * R), b = tokg / (R * R);
    const int i = p * (t / R) + sub / p, j = p * (t % R) + sub % p;
    const bool ok = flags[(size_t)b * N + i] && flags[(size_t)b * N + j];
    const float *hr = h + (size_t)m * E;
    for (int c = 0; c < Ca; c++) {
        float acc = 0.f;
        if (ok)
            for (int e = lane; e < E; e += 64) acc += hr[e] * W[(size_t)c * E + e];
        acc = wave_sum(acc);
        if (lane == 0) out[(((size_t)b * Ca + c) * N + i) * N + j] = ok ? acc + bias[c] : 0.f;
    }
}
bool launch_head_adj_patch(const float *h, const float *W, const float *bias, const uint8_t *flags, float *out, int B, int N, int p, int E,
                           int Ca, hipStream_t s) {
    if (B < 1 || p < 1 || N < p || N % p != 0 || E < 1 || Ca < 1 || (size_t)B * N * N > 0x7fffffffull) return false;
    const int M = B * N * N;
    DSG_LAUNCH(head_adj_patch_kernel, dim3((M + 3) / 4), dim3(256), 0, s, h, W, bias, flags, out, N, p, E, Ca, M);
    return true;
}

// Padding-aware pooling over rows in (token, a, b) order: pool[b][I][e] = (1/N) sum_J valid(I, J) rep[row(I, J)][e] -- the mean is over
// the N pixels of the row, the mask per pixel; J ascending, the order of pool_kernel
__global__ void pool_patch_kernel(const float *rep, const uint8_t *flags, float *pool, int B, int N, int p, int E) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * N * E) return;
    const int e = idx % E, i = (idx / E) % N, b = idx / (E * N);
    const int R = N / p, pp = p * p;
    float acc = 0.f;
    if (flags[(size_t)b * N + i])
        for (int j = 0; j < N; j++)
            if (flags[(size_t)b * N + j]) {
                const size_t m = ((size_t)b * R * R + (size_t)(i / p) * R + j / p) * pp + (i % p) * p + j % p;
                acc += rep[m * E + e];
            }
    pool[idx] = acc / (float)N;
}
bool launch_pool_patch(const float *rep, const uint8_t *flags, float *pool, int B, int N, int p, int E, hipStream_t s) {
    if (B < 1 || p < 1 || N < p || N % p != 0 || E < 1 || (size_t)B * N * E > 0x7fffffffull) return false;
    const int n = B * N * E;
    DSG_LAUNCH(pool_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rep, flags, pool, B, N, p, E);
    return true;
}


// =================================================================================================
// The fused forms for E = 96, p = 2 (the hot case): the p = 1 kernels' structure (kernels.hip: fused_patch_embed96_kernel,
// fused_readout96_kernel) with one wave per 32 TOKENS of the R x R grid, lane = token, consecutive lanes = consecutive tj.
// =================================================================================================
constexpr int P96_LD = 100;                       // floats per padded row of a wave's [32, 96] LDS tile
constexpr int P96_FLOATS = 32 * P96_LD;
__device__ __forceinline__ void p96_put(float *tile, int lrow, int e4, f32x4 v) { *reinterpret_cast<f32x4 *>(tile + lrow * P96_LD + 4 * e4) = v; }
// the wave's tile -> `rows` consecutive rows of a [*, 96] tensor, 16 bytes per lane and coalesced
__device__ __forceinline__ void p96_store_rows(const float *tile, float *g, int rows, int lane) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const int q = 64 * k + lane, r = q / 24, c = q - 24 * r;
        if (r < rows) *reinterpret_cast<f32x4 *>(g + (size_t)r * 96 + 4 * c) = *reinterpret_cast<const f32x4 *>(tile + r * P96_LD + 4 * c);
    }
}

// Fused PatchEmbed, p = 2: the wave's 32 tokens accumulate the four sub-pixel gathers -- each the p = 1 kernel's input vector
// [sc_adj, adj, sc_node(i), node(i), sc_node(j), node(j)] of pixel (2 ti + a, 2 tj + b), node parts selected by THAT pixel's flags,
// KP = in_chans rounded up to 32 -- into the same MFMA accumulators, one K-chunk of KP per sub-pixel with its own weight fragments
// Wp [4][3][KP / 8][64] float4 (sub = 2 a + b); then the p = 1 epilogue: LayerNorm_96, modulate + SiLU, optionally the first block's.
template <int KP>
__global__ __launch_bounds__(256, 2) void fused_patch_embed96_p2_kernel(const float *__restrict__ adj, const float *__restrict__ node,
                                                                       const float *__restrict__ sc_adj, const float *__restrict__ sc_node,
                                                                       const int *__restrict__ has_sc, const uint8_t *__restrict__ flags,
                                                                       const float *__restrict__ Wp, const float *__restrict__ bias,
                                                                       const float *__restrict__ gam, const float *__restrict__ bet,
                                                                       const float *__restrict__ aff, int aff_ld, int aff_off, int aff_off2,
                                                                       float *__restrict__ x, int B, int N, int Ca, int Cn, int self_cond) {
    constexpr int C = 96, S = KP / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int R = N >> 1, T = R * R, M = B * T;
    const int m = (blockIdx.x * 4 + wave) * 32 + lrow;
    const bool ok = m < M;
    const int mc = ok ? m : M - 1;
    const int b = mc / T, ti = (mc / R) % R, tj = mc % R;
    const bool sc_on = self_cond && sc_adj != nullptr && (has_sc == nullptr || *has_sc != 0);
    const int nsc = self_cond ? 2 : 1;
    f32x16 acc[3];
#pragma unroll
    for (int nt = 0; nt < 3; nt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 32 * nt + 8 * g + 4 * lhalf);
#pragma unroll
            for (int t = 0; t < 4; t++) acc[nt][4 * g + t] = bv[t];
        }
#pragma unroll 1
    for (int sub = 0; sub < 4; sub++) {
        const int i = 2 * ti + (sub >> 1), j = 2 * tj + (sub & 1);
        const bool mask = flags[(size_t)b * N + i] && flags[(size_t)b * N + j];
        const f32x4 *w = reinterpret_cast<const f32x4 *>(Wp) + (size_t)sub * 3 * S * 64 + lane;
#pragma unroll 1
        for (int s0 = 0; s0 < S; s0 += 4) {   // 32 channels at a time: the gather's registers stay next to the 48 accumulators
        f32x4 in[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int c = 8 * (s0 + s) + 4 * lhalf + t;
                float v = 0.f;
                if (c < nsc * Ca) {
                    const int which = self_cond ? c / Ca : 1, a = c % Ca;
                    const float *src = (which == 0) ? (sc_on ? sc_adj : nullptr) : adj;
                    if (src) v = src[(((size_t)b * Ca + a) * N + i) * N + j];
                } else if (c < nsc * (Ca + 2 * Cn)) {
                    const int cc = c - nsc * Ca;
                    const int colpart = cc / (nsc * Cn), c2 = cc % (nsc * Cn);
                    const int which = self_cond ? c2 / Cn : 1, a = c2 % Cn;
                    const float *src = (which == 0) ? (sc_on ? sc_node : nullptr) : node;
                    if (src && mask) v = src[((size_t)b * N + (colpart ? j : i)) * Cn + a];
                }
                in[s][t] = v;
            }
#pragma unroll
        for (int nt = 0; nt < 3; nt++)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const f32x4 a = w[((size_t)nt * S + s0 + s) * 64];
#pragma unroll
                for (int t = 0; t < 4; t++) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], in[s][t], acc[nt], 0, 0, 0);
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 3; nt++)
#pragma unroll
        for (int r = 0; r < 16; r++) sum += acc[nt][r];
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / C);
    float var = 0.f;
#pragma unroll
    for (int nt = 0; nt < 3; nt++)
#pragma unroll
        for (int r = 0; r < 16; r++) { const float d = acc[nt][r] - mean; var = fmaf(d, d, var); }
    var += __shfl_xor(var, 32, 64);
    const float rstd = fast_rsqrt(var * (1.0f / C) + LN_EPS);
    __shared__ __attribute__((aligned(16))) float tiles[4 * P96_FLOATS];
    float *tile = tiles + wave * P96_FLOATS;
    const int m_w = (blockIdx.x * 4 + wave) * 32, rows_w = min(32, M - m_w);   // this wave's rows (<= 0: a padding wave)
    const float *scale = aff + (size_t)b * aff_ld + aff_off + 4 * lhalf, *shift = scale + C;
#pragma unroll
    for (int nt = 0; nt < 3; nt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int e = 32 * nt + 8 * g;
            const f32x4 gg = *reinterpret_cast<const f32x4 *>(gam + e + 4 * lhalf);
            const f32x4 bb = *reinterpret_cast<const f32x4 *>(bet + e + 4 * lhalf);
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(scale + e);
            const f32x4 sh = *reinterpret_cast<const f32x4 *>(shift + e);
            f32x4 o;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const float n = (acc[nt][4 * g + t] - mean) * rstd * gg[t] + bb[t];
                o[t] = silu_exact(sh[t] + n * (sc[t] + 1.0f));
            }
            if (aff_off2 >= 0) {   // the first Swin block's modulate+SiLU on top (it then takes its input pre-modulated)
                const float *scale2 = aff + (size_t)b * aff_ld + aff_off2 + 4 * lhalf;
                const f32x4 sc2 = *reinterpret_cast<const f32x4 *>(scale2 + e), sh2 = *reinterpret_cast<const f32x4 *>(scale2 + C + e);
#pragma unroll
                for (int t = 0; t < 4; t++) o[t] = silu_exact(sh2[t] + o[t] * (sc2[t] + 1.0f));
            }
            p96_put(tile, lrow, (e >> 2) + lhalf, o);
        }
    if (rows_w > 0) p96_store_rows(tile, x + (size_t)m_w * C, rows_w, lane);   // (each wave reads back its own tile only: no barrier)
}

bool launch_fused_patch_embed96_p2(const float *adj, const float *node, const float *sc_adj, const float *sc_node, const int *has_sc,
                                   const uint8_t *flags, const float *Wp, const float *bias, const float *gam, const float *bet,
                                   const float *aff, int aff_ld, int aff_off, int aff_off2, float *x, int B, int N, int Ca, int Cn,
                                   int self_cond, int Kps, hipStream_t s) {
    if (B < 1 || N < 2 || N % 2 != 0 || Ca < 1 || Cn < 1 || (self_cond ? 2 : 1) * (Ca + 2 * Cn) > Kps) return false;
    if ((size_t)B * N * N / 4 > 0x7fffffffull) return false;
    const int M = B * (N / 2) * (N / 2);
    const dim3 grid((M + 127) / 128), block(256);
#define PE2_ARGS adj, node, sc_adj, sc_node, has_sc, flags, Wp, bias, gam, bet, aff, aff_ld, aff_off, aff_off2, x, B, N, Ca, Cn, self_cond
    if (Kps == 32) DSG_LAUNCH(fused_patch_embed96_p2_kernel<32>, grid, block, 0, s, PE2_ARGS);
    else if (Kps == 64) DSG_LAUNCH(fused_patch_embed96_p2_kernel<64>, grid, block, 0, s, PE2_ARGS);
    else return false;
#undef PE2_ARGS
    return true;
}

// Fused read-out, p = 2: LN(x) of the wave's 32 tokens is formed once and held in registers; the folded chain
// F2 gelu(Fa[a, b] LN(x) + fa) + f2 runs once per sub-pixel on its own fragments Wfp [4][3][12][64] float4 (sub = 2 a + b; fa is the
// same for the four: the biases do not depend on the sub-pixel), each followed by the store to pixel (2 ti + a, 2 tj + b) of
// out_adj [B, Ca, N, N], selected by that pixel's flags.  The node head's pooling commutes with the chain: per token row (b, ti) and
// column parity q the wave leaves the partial of s[ti, q] = (1/N) sum_tj flag_{2 tj + q} LN(x)[ti, tj] in slot (tile - first tile of
// the row) of pool_part [B R][nseg][2][96]; pool_finish_p2_kernel adds a row's slots in slot order: no atomics, a fixed order.
// A token none of whose pixels is valid takes part with an exact-zero LN row (a select), whatever its row of x holds.
__global__ __launch_bounds__(256, 2) void fused_readout96_p2_kernel(const float *__restrict__ x, const float *__restrict__ gam,
                                                                    const float *__restrict__ bet, const float *__restrict__ Wfp,
                                                                    const float *__restrict__ fa, const float *__restrict__ W2p,
                                                                    const float *__restrict__ f2, const uint8_t *__restrict__ flags,
                                                                    float *__restrict__ out_adj, float *__restrict__ pool_part, int nseg,
                                                                    int B, int N, int Ca) {
    constexpr int C = 96, S = 12;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int R = N >> 1, T = R * R, M = B * T;
    const int tile = blockIdx.x * 4 + wave;
    const int m = tile * 32 + lrow;
    const bool ok = m < M;
    const int mc = ok ? m : M - 1;
    const int b = mc / T, ti = (mc / R) % R, tj = mc % R;
    const uint8_t *fb = flags + (size_t)b * N;
    const bool fi0 = fb[2 * ti] != 0, fi1 = fb[2 * ti + 1] != 0, fj0 = fb[2 * tj] != 0, fj1 = fb[2 * tj + 1] != 0;
    const bool tokvalid = ok && (fi0 || fi1) && (fj0 || fj1);
    const int rowid = ok ? b * R + ti : -1;
    const int r_first = __shfl(rowid, 0, 64);
    int r_last = __shfl(rowid, 31, 64);
    if (r_last < 0) r_last = (M - 1) / R;   // partially filled last tile
    if (r_first < 0) r_last = -2;           // a tile entirely beyond M (padding wave of the last block) owns no row
    if (__ballot(tokvalid) == 0) {
        // no valid pixel under the wave's 32 tokens: exact zeros for the outputs and the pooling partials, x is not read
        for (int r = r_first; r <= r_last; r++) {
            float *dst = pool_part + ((size_t)r * nseg + (tile - (r * R) / 32)) * 2 * C;
            if (lrow < 2 * S) *reinterpret_cast<f32x4 *>(dst + 8 * lrow + 4 * lhalf) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (ok) {
#pragma unroll 1
            for (int sub = 0; sub < 4; sub++) {
                const int i = 2 * ti + (sub >> 1), j = 2 * tj + (sub & 1);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int c = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    if (c < Ca) out_adj[(((size_t)b * Ca + c) * N + i) * N + j] = 0.f;
                }
            }
        }
        return;
    }
    const float *xr = x + (size_t)mc * C + 4 * lhalf;
    f32x4 xn[S];
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < S; s++) {
        xn[s] = *reinterpret_cast<const f32x4 *>(xr + 8 * s);
        sum += (xn[s][0] + xn[s][1]) + (xn[s][2] + xn[s][3]);
    }
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / C);
    float var = 0.f;
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int t = 0; t < 4; t++) { const float d = xn[s][t] - mean; var = fmaf(d, d, var); }
    var += __shfl_xor(var, 32, 64);
    const float rstd = fast_rsqrt(var * (1.0f / C) + LN_EPS);
#pragma unroll
    for (int s = 0; s < S; s++) {
        const f32x4 gg = *reinterpret_cast<const f32x4 *>(gam + 8 * s + 4 * lhalf);
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(bet + 8 * s + 4 * lhalf);
        xn[s] = (xn[s] - mean) * rstd * gg + bb;
    }
#pragma unroll
    for (int s = 0; s < S; s++)
        if (!tokvalid) xn[s] = (f32x4){0.f, 0.f, 0.f, 0.f};   // a select: nothing of such a row travels through the products with 0

    // pooled LN(x) per (token row, column parity): segmented sums over the tokens of this wave that share a row (b, ti)
    {
        const float inv = 1.0f / (float)N;
        const float w0 = (tokvalid && fj0) ? inv : 0.f, w1 = (tokvalid && fj1) ? inv : 0.f;
        for (int r = r_first; r <= r_last; r++) {
            float *dst = pool_part + ((size_t)r * nseg + (tile - (r * R) / 32)) * 2 * C;
#pragma unroll 1
            for (int q = 0; q < 2; q++) {
                const float sel = (rowid == r) ? (q ? w1 : w0) : 0.f;
#pragma unroll
                for (int s = 0; s < S; s++)
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        float v = sel * xn[s][t];
#pragma unroll
                        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                        if (lrow == 0) dst[q * C + 8 * s + 4 * lhalf + t] = v;
                    }
            }
        }
    }

    const f32x4 *w2 = reinterpret_cast<const f32x4 *>(W2p) + lane;
#pragma unroll 1
    for (int sub = 0; sub < 4; sub++) {
        const int i = 2 * ti + (sub >> 1), j = 2 * tj + (sub & 1);
        const bool valid = ok && ((sub >> 1) ? fi1 : fi0) && ((sub & 1) ? fj1 : fj0);
        const f32x4 *w1 = reinterpret_cast<const f32x4 *>(Wfp) + (size_t)sub * 3 * S * 64 + lane;
        f32x16 oacc;
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[r] = 0.f;
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            f32x16 hacc;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(fa + 32 * nt + 8 * g + 4 * lhalf);
#pragma unroll
                for (int t = 0; t < 4; t++) hacc[4 * g + t] = bv[t];
            }
#pragma unroll
            for (int s = 0; s < S; s++) {
                const f32x4 a = w1[((size_t)nt * S + s) * 64];
#pragma unroll
                for (int t = 0; t < 4; t++) hacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], xn[s][t], hacc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) { const f32x2_t gg = gelu_f2(hacc[r], hacc[r + 1]); hacc[r] = gg[0]; hacc[r + 1] = gg[1]; }
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x4 a = w2[((size_t)nt * 4 + g) * 64];
#pragma unroll
                for (int t = 0; t < 4; t++) oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], hacc[4 * g + t], oacc, 0, 0, 0);
            }
        }
        if (ok) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int c = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                if (c < Ca) out_adj[(((size_t)b * Ca + c) * N + i) * N + j] = valid ? oacc[r] + f2[c] : 0.f;
            }
        }
    }
}

// pool_ext [B N, 256] of node row (b, I = 2 ti + a): columns 0 .. 95 = s[ti, 0], 96 .. 191 = s[ti, 1] (the token row's partials added in
// slot order), column 192 + q = flag_I * (#valid pixel columns of parity q) / N (the factors of the folded constant term), rest zero
__global__ void pool_finish_p2_kernel(const uint8_t *flags, const float *pool_part, int nseg, float *pool_ext, int B, int N) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * N * 256) return;
    const int col = idx & 255, row = idx >> 8, b = row / N, I = row - b * N, R = N >> 1;
    float v = 0.f;
    if (col < 192) {
        const int q = col / 96, c = col - 96 * q, trow = b * R + (I >> 1);
        const int segs = (trow * R + R - 1) / 32 - (trow * R) / 32 + 1;
        for (int sg = 0; sg < segs; sg++) v += pool_part[(((size_t)trow * nseg + sg) * 2 + q) * 96 + c];
    } else if (col < 194 && flags[row]) {
        int cnt = 0;
        for (int jj = col - 192; jj < N; jj += 2) cnt += flags[(size_t)b * N + jj] ? 1 : 0;
        v = (float)cnt / (float)N;
    }
    pool_ext[idx] = v;
}

int readout_pool_segments_p2(int N) { return (N / 2 + 30) / 32 + 1; }   // most 32-token tiles a row of N / 2 tokens can touch

bool launch_fused_readout96_p2(const float *x, const float *gam, const float *bet, const float *Wfp, const float *fa, const float *W2p,
                               const float *f2, const uint8_t *flags, float *out_adj, float *pool_part, float *pool_ext, int B, int N,
                               int Ca, hipStream_t s) {
    if (B < 1 || N < 2 || N % 2 != 0 || Ca < 1 || Ca > 32 || (size_t)B * N * 256 > 0x7fffffffull) return false;
    const int M = B * (N / 2) * (N / 2), nseg = readout_pool_segments_p2(N);
    DSG_LAUNCH(fused_readout96_p2_kernel, dim3((M + 127) / 128), dim3(256), 0, s, x, gam, bet, Wfp, fa, W2p, f2, flags, out_adj, pool_part,
               nseg, B, N, Ca);
    const int n = B * N * 256;
    DSG_LAUNCH(pool_finish_p2_kernel, dim3((n + 255) / 256), dim3(256), 0, s, flags, pool_part, nseg, pool_ext, B, N);
    return true;
}

}  // namespace dsg
