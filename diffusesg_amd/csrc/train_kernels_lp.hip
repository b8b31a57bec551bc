// train_kernels_lp.hip -- the bf16 mode of the training products (opt-in: dsg_train_set_precision; kernels.h: TrainLp).
//
// A covered product runs with both operands rounded to bf16 (round to nearest even), products accumulated in fp32 on
// v_mfma_f32_32x32x16_bf16, and an fp32 result.  y = x W^T and dx = dy W go through the sampling path's bf16 GEMM (kernels_lp.hip:
// launch_gemm_lp, which rounds the fp32 activation on its way into LDS) on a bf16 plane of the weight that t_cast_lp builds once per
// entry call; dW = dy^T x is this file's gemm_tn_bf16_kernel.  Master weights, saved activations, gradients and db stay fp32.
//
// Compiled like kernels_lp.hip: -fno-slp-vectorize, and the build fails on a packed-f32 VALU instruction or v_cvt_pk_bf16_f32 in the
// ISA (see the header of kernels_lp.hip for why those must not sit next to in-flight bf16 MFMAs).
#include "kernels_common.hip.h"

#include <algorithm>

namespace dsg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// (hi & 0xffff0000) | (lo >> 16): two bf16_rne_hi results into one dword, `lo` in the low half (the lower k)
__device__ __forceinline__ unsigned tlp_pack(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradients on the bf16 matrix pipe:  C[M,N] = sum_k bf16(A[k][m]) bf16(B[k][n])  (dW = dy^T x: A = dy [tokens, out], B = x
// [tokens, in], both token-major fp32 as the forward and backward left them, K = tokens), the contract of gemm_tn_f32_kernel:
// split-K slices in one launch (slice z writes its partial product to Cp + z M N, t_splitk_reduce adds them in slice order: no
// atomics, deterministic), rows past the slice and columns past M / N read as zero through the buffer descriptors, and with CS the
// block column tn == 0 leaves cs_part[z][m] = sum_k A[k][m] of its slice -- from the UNROUNDED fp32 values, in fp32.
//
// The contraction axis is the slow one in memory and v_mfma_f32_32x32x16_bf16 wants eight consecutive k per lane, so the tile is
// transposed on its way into LDS.  Block tile 128 (m) x 96 (n), k chunks of 32 tokens.  A chunk is 4 k-octets x (32 + 24) column
// quads = 224 tasks, one per thread (threads 224..255 stage nothing): a task loads eight token rows of one quad -- 16-byte loads, 512
// contiguous bytes per row across a wave's lanes -- rounds, packs the eight k of each of its four channels into one register quad
// (k-pairs per dword, the lower k in the low half) and writes four 16-byte rows:
//     LDS  As[m][k], Bs[n][k]  bf16, channel pitch 40 elements (80 B: 32 k + 8 padding)
// so that a fragment is one ds_read_b128 of the lane's eight k (k = 16 step + 8 (lane >> 5) + 0..7) of channel lane & 31.  With the
// 80-byte pitch the eight lanes of a b128 read phase hit eight different 16-byte bank groups (20 dwords x 8 lanes = 0, 20, 40, .. mod
// 64: no overlap), the same layout and read pattern as gemm_bf16_kernel; the 16-byte writes (pitch 4 channels = 80 dwords) are two-way.
// Register-staged double buffer, one barrier per chunk, wave tile 32 x 96 (3 accumulators), as the fp32 kernel.
// ---------------------------------------------------------------------------------------------------------------------
template <bool CS>
__global__ __launch_bounds__(256, 2) void gemm_tn_bf16_kernel(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                                              float *__restrict__ Cp, int M, int N, int K, int kslice, int tiles_m, int tiles_n,
                                                              float *__restrict__ cs_part) {
    constexpr int BM = 128, BN = 96, BK = 32, LDP = BK + 8;
    constexpr int BUF = (BM + BN) * LDP;
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BUF];
    const int tiles = tiles_m * tiles_n;
    const int z = blockIdx.x / tiles, t = blockIdx.x % tiles, tm = t / tiles_n, tn = t % tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kb = z * kslice, ke = min(K, kb + kslice);
    const int nk = (ke - kb + BK - 1) / BK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lhalf = lane >> 5;
    // the staging task of this thread: operand (A: tid < 128, B: 128 <= tid < 224), k-octet ko, column quad c4
    const bool isA = tid < 128, isB = !isA && tid < 224;
    const int tb_ = tid - 128;
    const int ko = isA ? tid >> 5 : tb_ / 24, c4 = isA ? tid & 31 : tb_ % 24;
    const int ld = isA ? lda : ldb, c0 = isA ? m0 : n0, lim = isA ? M : N;
    // rows [kb, ke) of the task's operand; rows past the slice and columns past M / N read as zero
    const float *base = isA ? A : B;
    const rsrc_t rs = make_rsrc(base + (size_t)kb * ld, (unsigned)(ke - kb) * ld * 4u);
    const unsigned voff = ((isA || isB) && c0 + 4 * c4 < lim) ? ((unsigned)(8 * ko) * ld + (unsigned)(c0 + 4 * c4)) * 4u : 0x7fffffffu;
    __bf16 *const wdst = lds + (isA ? 0 : BM * LDP) + (4 * c4) * LDP + 8 * ko;   // + buffer offset, + t LDP for the task's channel t

    f32x4 st[8];
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    auto issue = [&](int kc) {
#pragma unroll
        for (int r = 0; r < 8; r++) st[r] = buf_load4(rs, voff + (unsigned)r * ld * 4u, (unsigned)kc * BK * ld * 4u);
    };
    auto write = [&](int buf) {
        if (!(isA || isB)) return;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            u32x4 q;
#pragma unroll
            for (int p = 0; p < 4; p++) q[p] = tlp_pack(bf16_rne_hi(st[2 * p][c]), bf16_rne_hi(st[2 * p + 1][c]));
            *reinterpret_cast<u32x4 *>(wdst + buf * BUF + c * LDP) = q;
            if (CS) {
#pragma unroll
                for (int r = 0; r < 8; r++) cs[c] += st[r][c];
            }
        }
    };
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
    if (nk > 0) {
        issue(0);
        write(0);
        __syncthreads();
    }
    for (int kc = 0; kc < nk; kc++) {
        const int cur = kc & 1;
        if (kc + 1 < nk) issue(kc + 1);
        const __bf16 *As = lds + cur * BUF + (wave * 32 + lrow) * LDP + 8 * lhalf, *Bs = lds + cur * BUF + BM * LDP + lrow * LDP + 8 * lhalf;
#pragma unroll
        for (int s2 = 0; s2 < BK / 16; s2++) {   // MFMA k-steps of 16; lane (row, half) holds k = 16 s2 + 8 half + 0..7
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(As + 16 * s2);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const bf16x8 b = *reinterpret_cast<const bf16x8 *>(Bs + 32 * j * LDP + 16 * s2);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
            }
        }
        if (kc + 1 < nk) write(1 - cur);
        __syncthreads();
    }
    // partial product of this slice: rows m0 + 32 wave + (r&3) + 8 (r>>2) + 4 half, columns n0 + 32 j + lrow
    float *Cz = Cp + (size_t)z * M * N;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int n = n0 + 32 * j + lrow;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
            if (m < M && n < N) Cz[(size_t)m * N + n] = acc[j][r];
        }
    }
    if (CS && tn == 0) {   // (block-uniform) the four k-octets' sums of a channel, added in octet order; the tiles are dead after the loop's last barrier
        float *red = reinterpret_cast<float *>(lds);   // [4 octets][128 channels]
        if (isA) {
#pragma unroll
            for (int c = 0; c < 4; c++) red[ko * BM + 4 * c4 + c] = cs[c];
        }
        __syncthreads();
        if (tid < BM && m0 + tid < M) cs_part[(size_t)z * M + m0 + tid] = ((red[tid] + red[BM + tid]) + red[2 * BM + tid]) + red[3 * BM + tid];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight planes: W [R, Cc] fp32 -> nk [R, Cc] and kn [Cc, R] bf16 (RNE; the rounding of launch_f32_to_bf16), one 32 x 32 tile per block,
// every weight of a group in one launch.  The transposed plane goes straight to bf16: no fp32 transposed copy in between.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void t_cast_lp_kernel(TCastGroup g) {
    __shared__ unsigned short tile[32][33];
    int e = 0;
    while (e + 1 < g.n && (int)blockIdx.x >= g.j[e + 1].tile0) e++;   // block-uniform
    const TCastJob &jb = g.j[e];
    const int tl = blockIdx.x - jb.tile0, tc = (jb.Cc + 31) / 32;
    const int r0 = (tl / tc) * 32, c0 = (tl % tc) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    unsigned short *nk = static_cast<unsigned short *>(jb.nk), *kn = static_cast<unsigned short *>(jb.kn);
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        unsigned short v = 0;
        if (r < jb.R && c < jb.Cc) {
            v = (unsigned short)(bf16_rne_hi(jb.src[(size_t)r * jb.Cc + c]) >> 16);
            if (nk) nk[(size_t)r * jb.Cc + c] = v;
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    if (!kn) return;
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < jb.Cc && r0 + tx < jb.R) kn[(size_t)(c0 + i) * jb.R + r0 + tx] = tile[tx][i];
}
void t_cast_lp_add(TCastGroup &g, const float *src, void *nk, void *kn, int R, int Cc) {
    g.j[g.n++] = TCastJob{src, nk, kn, R, Cc, g.tiles};
    g.tiles += ((R + 31) / 32) * ((Cc + 31) / 32);
}
void t_cast_lp(const TCastGroup &g, hipStream_t s) {
    if (g.n < 1 || g.tiles < 1) return;
    hipLaunchKernelGGL(t_cast_lp_kernel, dim3((unsigned)g.tiles), dim3(256), 0, s, g);
}

bool t_gemm_lp(TrainLp &lp, bool ta, bool tb, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc, int M, int N,
               int K, bool accumulate, hipStream_t s, float *a_colsum, const float *res, int act, float *c2, int *route) {
    if (!ta) {
        // y = x W^T (tb) / dx = dy W: the bf16 GEMM on the weight's plane, [N, K] either way
        if (!t_lp_rule(lp.any_rows ? 512 : (size_t)M, N, K) || lda != K || ldb != (tb ? K : N) || a_colsum) return false;
        if (act != ACT_NONE && (act != ACT_GELU_KEEP || !c2) && (act != ACT_DGELU || !res)) return false;
        if (act != ACT_NONE && (ldc != N || accumulate)) return false;   // (the elementwise pass behind the product walks M N contiguous values)
        const auto it = lp.planes.find(B);
        const void *Wb = it == lp.planes.end() ? nullptr : (tb ? it->second.nk : it->second.kn);
        if (!Wb) return false;
        GemmArgs g;
        g.A = A; g.lda = K; g.K1 = K; g.K = K; g.M = M; g.N = N; g.Wb = Wb; g.bias = bias; g.ldc = ldc;
        g.C = act == ACT_GELU_KEEP ? c2 : C;
        if (act == ACT_NONE) {
            if (res) { g.res = res; g.ldres = ldc; }
            else if (accumulate) { g.res = C; g.ldres = ldc; }
        }
        if (!launch_gemm_lp(g, s)) { t_scratch_mark_failed(s); return true; }   // (a form launch_gemm_lp builds; reported by the entry point)
        if (act == ACT_GELU_KEEP) t_gelu(c2, nullptr, C, (size_t)M * N, false, s);
        else if (act == ACT_DGELU) t_gelu(res, C, C, (size_t)M * N, true, s);
        if (route) { route[0] = 5; route[1] = 1; }
        return true;
    }
    // dW [M = out, N = in] = dy^T x, K = tokens
    if (tb || bias || res || act != ACT_NONE || !t_lp_rule(lp.any_rows ? 512 : (size_t)K, M, N)) return false;
    const int tiles_m = (M + 127) / 128, tiles_n = (N + 95) / 96;
    int S = std::max(1, std::min(256, 1024 / (tiles_m * tiles_n)));   // ~1024 blocks, slices of >= 512 rows: gemm_tn_f32_kernel's rule
    S = std::max(1, std::min(S, K / 512));
    const int kslice = ((K + S - 1) / S + 31) / 32 * 32;
    S = (K + kslice - 1) / kslice;
    const size_t nC = (size_t)S * M * N, nS = a_colsum ? (size_t)S * M : 0;
    float *buf = t_scratch_sk(s, nC + nS);
    if (!buf) return true;   // (out of memory: marked on the stream)
    const dim3 grid((unsigned)(tiles_m * tiles_n * S));
    if (a_colsum) hipLaunchKernelGGL((gemm_tn_bf16_kernel<true>), grid, dim3(256), 0, s, A, lda, B, ldb, buf, M, N, K, kslice, tiles_m, tiles_n, buf + nC);
    else hipLaunchKernelGGL((gemm_tn_bf16_kernel<false>), grid, dim3(256), 0, s, A, lda, B, ldb, buf, M, N, K, kslice, tiles_m, tiles_n, nullptr);
    t_splitk_reduce(buf, C, ldc, M, N, S, accumulate, buf + nC, a_colsum, s);
    if (route) { route[0] = 6; route[1] = S; }
    return true;
}

}  // namespace dsg
