// kernels_lp.hip -- the bf16-MFMA GEMMs of libdsg (both opt-in): "gemm_split" (fp32-accurate, six bf16 partial
// products of hi/mid/lo operand splits) and "gemm_bf16" (operands rounded to bf16).
//
// This file is compiled with -fno-slp-vectorize and the build fails if its ISA contains a packed-f32 VALU instruction
// (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32) or v_cvt_pk_bf16_f32: on MI355X those, issued next to in-flight bf16 MFMAs
// of the same wave, produced rare wrong lanes (one 16-lane group in ~1e3 wave tiles; found and bisected with
// tools/gemm_bench's full-matrix diff against the fp32 kernel -- the scalar-op forms of the same code are clean).  The
// f32-MFMA kernels in kernels.hip do not co-issue VALU work with the matrix pipe and are unaffected.
#include "kernels_common.hip.h"

namespace dsg {

// -------------------------------------------------------------------------------------------------
// bf16 GEMM (opt-in precision mode, BASELINE config 5): same interface and epilogue as gemm4, operands rounded to
// bf16 (RNE) -- A on the way into LDS (after the fp32 LayerNorm FMA), W pre-converted at pack time -- products on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Activations stay fp32 in HBM, so at these shapes the kernel is
// bound by HBM/L2 streaming, not by the matrix pipe (16x the f32 rate): 128x96 tile, K step 64, register-staged.
// -------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// fp32 -> bf16 on the integer pipe.  The gfx950 v_cvt_pk_bf16_f32 instruction is deliberately not used: in these kernels
// (conversion results feeding ds_write while bf16 MFMAs of the same wave are in flight) it produced rare wrong values in
// lanes 48..63 (about one 16-lane group in 1e5; found with tools/gemm_bench's full-matrix diff, gone with this code).
// (bf16_rne_hi lives in kernels_common.hip.h)
__device__ __forceinline__ unsigned pack_hi16(unsigned lo, unsigned hi) {   // (hi & 0xffff0000) | (lo >> 16)
    return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}
// hi + mid + lo == a to 24 bits, each term exactly representable in bf16 (truncating split; the terms share a's sign)
__device__ __forceinline__ void split3_bits(float a, unsigned &h, unsigned &m, unsigned &l) {
    h = __float_as_uint(a) & 0xffff0000u;
    const float r1 = a - __uint_as_float(h);
    m = __float_as_uint(r1) & 0xffff0000u;
    l = __float_as_uint(r1 - __uint_as_float(m));   // bits [31:16] are used
}
constexpr int HBK = 64;  // k per chunk of the 128x96 tile; K1 of a two-source GEMM must be a multiple of it

// EPI: the same epilogue extensions as gemm4_f32_kernel (kernels.hip): 1 row-statistics partials, 2 / 3 the next block's
// modulate+SiLU (batch-uniform / per-sample) + partials; LN statistics may come from a producer's partials (g.ln_part).
// ABF / CBF ("bf16 activations between kernels"): the A tensor is already bf16 (staged into LDS as is: no conversion, half the
// bytes) / the result is stored as bf16.  Used where the consumer is this kernel and would round the fp32 value to bf16 on its way
// into LDS anyway (fc1 -> fc2's hidden tensor, attention output -> proj): results are bit-identical to the fp32-tensor path.
// RB (round 2, late): 32-row blocks per wave.  RB = 1: 128x96 block tile, K step 64.  RB = 2: 256x96 block tile (a wave owns 64 rows),
// K step 32: every W fragment read from LDS feeds two MFMAs instead of one -- the 32x96 wave tile asks the LDS for ~340 B/clk per CU
// (it has 128), the 64x96 one for ~210 -- and the A tile is re-read from L2 by half as many column-tile blocks per row.
template <bool LN, int ACT, bool RES, int EPI = 0, bool ABF = false, bool CBF = false, int RB = 1>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(GemmArgs g, int tiles_m, int tiles_n) {
    static_assert(!(ABF && LN), "a bf16 A tensor carries no LayerNorm");
    constexpr int TM = GBM * RB;                 // block rows
    constexpr int KB = RB == 1 ? 64 : 32;        // k per chunk
    constexpr int LDP = KB + 8;                  // LDS row stride in bf16 elements (16-B aligned, conflict-free b128 reads)
    constexpr int TA = KB / 4, RPA = 256 / TA;   // fp32 A staging: threads per row (float4 each), rows per pass; TM / RPA == 8 passes
    constexpr int TW = KB / 8, RPW = 256 / TW;   // bf16 staging (W, and A when ABF): threads per row (8 bf16 each), rows per pass
    constexpr int PW = (GBN + RPW - 1) / RPW;    // W passes (3 or 2; rows >= 96 of the last pass are masked)
    constexpr int PAB = TM / RPW;                // bf16-A passes (4)
    static_assert(TM / RPA == 8 && PAB == 4, "staging layout");
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * (TM + GBN) * LDP];
    constexpr int BUF = (TM + GBN) * LDP;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, seq = bid >> 3;
    const int tm = (seq / tiles_n) * 8 + xcd, tn = seq % tiles_n;
    if (tm >= tiles_m) return;
    const int m0 = tm * TM, n0 = tn * GBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows_m = min(TM, g.M - m0), rows_n = min(GBN, g.N - n0);
    const rsrc_t rsA1 = ABF ? make_rsrc(reinterpret_cast<const __bf16 *>(g.A) + (size_t)m0 * g.lda, (unsigned)rows_m * g.lda * 2u)
                            : make_rsrc(g.A + (size_t)m0 * g.lda, (unsigned)rows_m * g.lda * 4u);
    const rsrc_t rsA2 = make_rsrc(g.A2 ? g.A2 + (size_t)m0 * g.lda2 : g.A, g.A2 ? (unsigned)rows_m * g.lda2 * 4u : 0u);
    const rsrc_t rsW = make_rsrc(static_cast<const __bf16 *>(g.Wb) + (size_t)n0 * g.K, (unsigned)rows_n * g.K * 2u);
    const int ca = tid % TA, ra = tid / TA, cw = tid % TW, rw = tid / TW;
    unsigned voffA1[8], voffA2[8], voffW[PW];
    float a_rstd[8], a_nmr[8];
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const int r = ra + RPA * p;
        voffA1[p] = ((unsigned)r * g.lda + 4u * ca) * 4u;
        voffA2[p] = ((unsigned)r * g.lda2 + 4u * ca) * 4u;
        if (LN) {
            const int m = min(m0 + r, g.M - 1);
            float mean, rstd;
            if (g.ln_part) {   // [M][nparts][2] partial (sum, sumsq) pairs of the producing GEMM, added in tile order
                const float *pp = g.ln_part + (size_t)m * g.ln_nparts * 2;
                float sm = 0.f, sq = 0.f;
                if (g.ln_nparts == 2) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(pp);
                    sm = a[0] + a[2]; sq = a[1] + a[3];
                } else if (g.ln_nparts == 4) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(pp), b = *reinterpret_cast<const f32x4 *>(pp + 4);
                    sm = (a[0] + a[2]) + (b[0] + b[2]); sq = (a[1] + a[3]) + (b[1] + b[3]);
                } else {
                    for (int t = 0; t < g.ln_nparts; t++) { sm += pp[2 * t]; sq += pp[2 * t + 1]; }
                }
                const float invk = 1.0f / (float)g.K;
                mean = sm * invk;
                rstd = fast_rsqrt(fmaxf(fmaf(-mean, mean, sq * invk), 0.f) + LN_EPS);
            } else {
                mean = g.ln_stats[2 * m]; rstd = g.ln_stats[2 * m + 1];
            }
            a_rstd[p] = rstd; a_nmr[p] = -mean * rstd;
        }
    }
#pragma unroll
    for (int p = 0; p < PW; p++) voffW[p] = (rw + RPW * p < GBN) ? ((unsigned)(rw + RPW * p) * g.K + 8u * cw) * 2u : 0x7fffffffu;
    unsigned voffAb[PAB];   // ABF: TW threads per row (8 bf16 each), rows rw + RPW p
#pragma unroll
    for (int p = 0; p < PAB; p++) voffAb[p] = ((unsigned)(rw + RPW * p) * g.lda + 8u * cw) * 2u;
    // K may be a multiple of 32 only (e.g. 96): with KB = 64 the last chunk is then half valid; the descriptor zero-fills the rest
    // of the row only at the buffer end, so clamp explicitly
    const int nk = (g.K + KB - 1) / KB;
    const int K1 = g.A2 ? g.K1 : g.K;

    f32x4 sa[8];
    bf16x8 sw[PW], sab[PAB];
    auto issue = [&](int kc) {
        const int k0 = kc * KB, k = k0 + 4 * ca;
        if (ABF) {
#pragma unroll
            for (int p = 0; p < PAB; p++) {
                bf16x8 v = {};
                if (k0 + 8 * cw < g.K) v = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsA1, voffAb[p], (unsigned)k0 * 2u, 0));
                sab[p] = v;
            }
        }
#pragma unroll
        for (int p = 0; p < (ABF ? 0 : 8); p++) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < g.K) v = (k >= K1) ? buf_load4(rsA2, voffA2[p], (unsigned)(k0 - K1) * 4u) : buf_load4(rsA1, voffA1[p], (unsigned)k0 * 4u);
            sa[p] = v;
        }
#pragma unroll
        for (int p = 0; p < PW; p++) {
            bf16x8 v = {};
            if (k0 + 8 * cw < g.K) v = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsW, voffW[p], (unsigned)k0 * 2u, 0));
            sw[p] = v;
        }
    };
    auto write = [&](int buf, int kc) {
        __bf16 *As = lds + buf * BUF, *Ws = As + TM * LDP;
        const bool kvalid = kc * KB + 4 * ca < g.K;
        if (ABF) {
#pragma unroll
            for (int p = 0; p < PAB; p++) *reinterpret_cast<bf16x8 *>(As + (rw + RPW * p) * LDP + 8 * cw) = sab[p];
        }
#pragma unroll
        for (int p = 0; p < (ABF ? 0 : 8); p++) {
            f32x4 v = sa[p];
            if (LN && kvalid) {
#pragma unroll
                for (int t = 0; t < 4; t++) v[t] = fmaf(v[t], a_rstd[p], a_nmr[p]);
            }
            u32x2 b;
            b[0] = pack_hi16(bf16_rne_hi(v[0]), bf16_rne_hi(v[1]));
            b[1] = pack_hi16(bf16_rne_hi(v[2]), bf16_rne_hi(v[3]));
            *reinterpret_cast<u32x2 *>(As + (ra + RPA * p) * LDP + 4 * ca) = b;
        }
#pragma unroll
        for (int p = 0; p < PW; p++)
            if (rw + RPW * p < GBN) *reinterpret_cast<bf16x8 *>(Ws + (rw + RPW * p) * LDP + 8 * cw) = sw[p];
    };
    const int lrow = lane & 31, lhalf = lane >> 5;
    f32x16 acc[RB][3];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rb][j][r] = 0.f;
    issue(0);
    write(0, 0);
    __syncthreads();
    for (int kc = 0; kc < nk; kc++) {
        const int cur = kc & 1;
        if (kc + 1 < nk) issue(kc + 1);
        const __bf16 *As = lds + cur * BUF, *Ws = As + TM * LDP;
#pragma unroll
        for (int s = 0; s < KB / 16; s++) {  // MFMA k-steps of 16; lane (row, half) holds k = 16s + 8*half + 0..7
            bf16x8 b[3];
#pragma unroll
            for (int j = 0; j < 3; j++) b[j] = *reinterpret_cast<const bf16x8 *>(Ws + (32 * j + lrow) * LDP + 16 * s + 8 * lhalf);
#pragma unroll
            for (int rb = 0; rb < RB; rb++) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(As + (wave * 32 * RB + 32 * rb + lrow) * LDP + 16 * s + 8 * lhalf);
#pragma unroll
                for (int j = 0; j < 3; j++) acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[j], acc[rb][j], 0, 0, 0);
            }
        }
        if (kc + 1 < nk) write(1 - cur, kc + 1);
        __syncthreads();
    }
    const rsrc_t rsC = CBF ? make_rsrc(reinterpret_cast<unsigned short *>(g.C) + (size_t)m0 * g.ldc, (unsigned)rows_m * g.ldc * 2u)
                           : make_rsrc(g.C + (size_t)m0 * g.ldc, (unsigned)rows_m * g.ldc * 4u);
    const rsrc_t rsC2 = make_rsrc(g.C2 ? g.C2 + (size_t)m0 * g.ldc2 : g.C, g.C2 ? (unsigned)rows_m * g.ldc2 * 4u : 0u);
    const rsrc_t rsR = make_rsrc(RES ? g.res + (size_t)m0 * g.ldres : g.C, RES ? (unsigned)rows_m * g.ldres * 4u : 0u);
    const unsigned OOB = 0x7fffffffu;
    float *ldsf = reinterpret_cast<float *>(lds);   // the K loop's tiles are dead after its last barrier
    int *bt = reinterpret_cast<int *>(ldsf) + 4 * 2304;   // EPI == 3: row -> sample table behind the four per-wave reduction slabs
    if (EPI == 3) {   // per-sample (scale,shift): row -> sample through a TM-entry LDS table
        for (int t = tid; t < TM; t += 256) bt[t] = min(m0 + t, g.M - 1) / g.mod_T;
        __syncthreads();
    }
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
        const unsigned rowl = (unsigned)(wave * 32 * RB + 32 * rb + 4 * lhalf);
        float st_s[16], st_q[16];
        int brow[16];
        if (EPI >= 1) {
#pragma unroll
            for (int r = 0; r < 16; r++) { st_s[r] = 0.f; st_q[r] = 0.f; }
        }
        if (EPI == 3) {
#pragma unroll
            for (int r = 0; r < 16; r++) brow[r] = bt[rowl + (r & 3) + 8 * (r >> 2)];
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int n = n0 + 32 * j + lrow;
            const bool nok = n < g.N;
            const float bias = (g.bias && nok) ? g.bias[n] : 0.f;
            const unsigned vC = nok ? (rowl * g.ldc + (unsigned)n) * 4u : OOB;
            const unsigned vC2 = nok ? (rowl * g.ldc2 + (unsigned)n) * 4u : OOB;
            const unsigned vR = nok ? (rowl * g.ldres + (unsigned)n) * 4u : OOB;
            float msc = 0.f, msh = 0.f;
            if (EPI == 2 && nok) { msc = g.mod_aff[g.mod_off + n] + 1.0f; msh = g.mod_aff[g.mod_off + g.N + n]; }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const unsigned rr = (unsigned)((r & 3) + 8 * (r >> 2));
                float v = acc[rb][j][r] + bias;
                if (ACT == ACT_GELU) v = gelu_f(v);
                else if (ACT == ACT_SILU) v = silu_exact(v);
                if (RES) v += buf_load1(rsR, vR, rr * g.ldres * 4u);
                if (g.C2) buf_store1(v, rsC2, vC2, rr * g.ldc2 * 4u);
                if (EPI == 3 && nok) {
                    const float *ar = g.mod_aff + (size_t)brow[r] * g.mod_ld + g.mod_off + n;
                    msc = ar[0] + 1.0f; msh = ar[g.N];
                }
                if (EPI >= 2) v = silu_exact(fmaf(v, msc, msh));
                if (EPI >= 1 && nok) { st_s[r] += v; st_q[r] = fmaf(v, v, st_q[r]); }
                if (CBF) buf_store_bf16(v, rsC, nok ? vC >> 1 : OOB, rr * g.ldc * 2u);
                else buf_store1(v, rsC, vC, rr * g.ldc * 4u);
            }
        }
        if (EPI >= 1) {   // row statistics of the stored tile: per-wave LDS transpose, fixed-order sums (see gemm4_f32_kernel)
            float *red = ldsf + wave * 2304;   // [2 quantities][32 rows][36]
            __builtin_amdgcn_wave_barrier();   // (RB = 2: the slab is reused by the wave's second row block)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                red[row * GLD + lrow] = st_s[r];
                red[(32 + row) * GLD + lrow] = st_q[r];
            }
            __builtin_amdgcn_wave_barrier();
            const float *src = red + (lhalf * 32 + lrow) * GLD;
            float tot = 0.f;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const f32x4 q4 = *reinterpret_cast<const f32x4 *>(src + 4 * i);
                tot += (q4[0] + q4[1]) + (q4[2] + q4[3]);
            }
            const rsrc_t rsP = make_rsrc(g.stats_out + (size_t)m0 * tiles_n * 2, (unsigned)(rows_m * tiles_n) * 8u);   // [M][tiles_n][2]
            buf_store1(tot, rsP, (unsigned)(((wave * 32 * RB + 32 * rb + lrow) * tiles_n + tn) * 2 + lhalf) * 4u, 0u);
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Split-bf16 GEMM (opt-in "gemm_split" mode): fp32-accurate products on the bf16 matrix pipe.
// Every fp32 operand is written as hi + mid + lo with three bf16 values (8 + 8 + 8 = 24 mantissa bits, bf16 has the
// fp32 exponent range so nothing can overflow or flush); a.w is accumulated in fp32 from the six partial products
// hh, hm, mh, hl, lh, mm (the dropped ml, lm, ll terms are <= 2^-24 relative -- fp32 rounding level).  Six
// v_mfma_f32_32x32x16_bf16 (192 cycles per 32x32x16) replace eight v_mfma_f32_32x32x2_f32 (512 cycles), and unlike the
// f32 MFMA the bf16 MFMA overlaps with VALU work.  A is split while it is staged into LDS (after the fp32 LayerNorm
// FMA, by truncation on the integer pipe: and / sub / and / sub / perm); weights are pre-split at pack time ([3][N][K] bf16).
// -------------------------------------------------------------------------------------------------
constexpr int SBK = 32, SLD = 40;  // k per chunk; LDS row stride in bf16 elements (80 B: 16-B aligned, conflict-free b128 reads)

// The A operand never touches LDS.  A wave owns 64 rows x all 96 columns of the block
// tile, so its A fragments are private: each lane loads the 16 k-values of its row half straight from global memory
// (64 contiguous bytes per lane and chunk; the MFMA k index is a free permutation as long as the W fragment uses the
// same one), splits them into the three bf16 planes on the integer pipe, and feeds the MFMAs.  Only the pre-split W
// tile (shared by the block's waves) is staged through a double-buffered LDS tile: one barrier per 32-k chunk.
// NW waves per block -> block tile (64 NW) x 96.
template <bool LN, int ACT, bool RES, int NW>
__global__ __launch_bounds__(64 * NW, 2) void gemm_split2_kernel(GemmArgs g, int tiles_m, int tiles_n) {
    constexpr int TM = 64 * NW, WROWS = 128, WPL = WROWS * SLD;   // W tile padded to 128 rows: staging is branch-free
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * 3 * WPL];   // [buf][plane][128][SLD]
    const int bid = blockIdx.x;
    const int xcd = bid & 7, seq = bid >> 3;
    const int tm = (seq / tiles_n) * 8 + xcd, tn = seq % tiles_n;
    if (tm >= tiles_m) return;
    const int m0 = tm * TM, n0 = tn * GBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int rows_m = min(TM, g.M - m0), rows_n = min(GBN, g.N - n0);
    const rsrc_t rsA1 = make_rsrc(g.A + (size_t)m0 * g.lda, (unsigned)rows_m * g.lda * 4u);
    const rsrc_t rsA2 = make_rsrc(g.A2 ? g.A2 + (size_t)m0 * g.lda2 : g.A, g.A2 ? (unsigned)rows_m * g.lda2 * 4u : 0u);
    const __bf16 *Ws = static_cast<const __bf16 *>(g.Ws3);
    const size_t plane = (size_t)g.N * g.K;
    rsrc_t rsW[3];
#pragma unroll
    for (int q = 0; q < 3; q++) rsW[q] = make_rsrc(Ws + q * plane + (size_t)n0 * g.K, (unsigned)rows_n * g.K * 2u);
    unsigned voffA1[2], voffA2[2];
    float a_rstd[2], a_nmr[2];
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
        const int r = wave * 64 + rb * 32 + lrow;
        const int rl = min(r, rows_m - 1);   // rows past M re-read the last valid row (never stored); see the note below
        voffA1[rb] = ((unsigned)rl * g.lda + 16u * lhalf) * 4u;
        voffA2[rb] = ((unsigned)rl * g.lda2 + 16u * lhalf) * 4u;
        if (LN) {
            const int m = min(m0 + r, g.M - 1);
            const float mean = g.ln_stats[2 * m], rstd = g.ln_stats[2 * m + 1];
            a_rstd[rb] = rstd; a_nmr[rb] = -mean * rstd;
        }
    }
    constexpr int RP = 16 * NW, NP = WROWS / RP;   // W staging: RP rows per pass, 4 x 16 B per row and plane; rows >= rows_n
                                                   // duplicate the last valid row (their columns are never stored)
    const int wr = tid >> 2, wc = tid & 3;
    unsigned voffW[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) voffW[i] = ((unsigned)min(wr + RP * i, rows_n - 1) * g.K + 8u * wc) * 2u;
    const int nk = g.K / SBK;
    const int nk1 = g.A2 ? g.K1 / SBK : nk;

    f32x4 sw[NP][3];
    f32x4 araw[2][4];
    auto issueW = [&](int kc) {
        const unsigned soff = (unsigned)kc * (SBK * 2u);
#pragma unroll
        for (int i = 0; i < NP; i++)
#pragma unroll
            for (int q = 0; q < 3; q++) sw[i][q] = buf_load4(rsW[q], voffW[i], soff);
    };
    auto writeW = [&](int buf) {
        __bf16 *Wp = lds + buf * 3 * WPL;
#pragma unroll
        for (int i = 0; i < NP; i++)
#pragma unroll
            for (int q = 0; q < 3; q++) *reinterpret_cast<f32x4 *>(Wp + q * WPL + (wr + RP * i) * SLD + 8 * wc) = sw[i][q];
    };
    // raw fp32 of (row block rb, k-step s) of chunk kc -> araw[rb][2s], araw[rb][2s+1]
    auto loadA = [&](int kc, int rb, int s2) {
        const bool second = kc >= nk1;
        const unsigned soff = (unsigned)(second ? kc - nk1 : kc) * (SBK * 4u);
#pragma unroll
        for (int t = 2 * s2; t < 2 * s2 + 2; t++)
            araw[rb][t] = second ? buf_load4(rsA2, voffA2[rb] + 16u * t, soff) : buf_load4(rsA1, voffA1[rb] + 16u * t, soff);
    };
    // araw[rb][2s], araw[rb][2s+1] -> the three bf16 planes of the lane's 8 k-values (packed math: 5 VALU per element)
    // araw[rb][2s], araw[rb][2s+1] -> dwords [e0, e1) of the three bf16 planes of the lane's 8 k-values (2 k per dword).
    // Scalar fp32 ops on purpose: packed-f32 VALU ops (v_pk_fma_f32 / v_pk_add_f32) next to bf16 MFMAs produced rare
    // wrong lanes on this part (see tools/gemm_bench's full-matrix diff), so nothing here may be SLP-vectorised.
    struct Frag { u32x4 p[3]; };   // p[0] = hi, p[1] = mid, p[2] = lo
    auto build = [&](int rb, int s2, Frag &F, int e0, int e1) {
#pragma unroll
        for (int e = e0; e < e1; e++) {
            const f32x4 src = araw[rb][2 * s2 + (e >> 1)];
            float v0 = src[2 * (e & 1)], v1 = src[2 * (e & 1) + 1];
            if (LN) { v0 = fmaf(v0, a_rstd[rb], a_nmr[rb]); v1 = fmaf(v1, a_rstd[rb], a_nmr[rb]); }
            unsigned h0, m0_, l0, h1, m1, l1;
            split3_bits(v0, h0, m0_, l0);
            split3_bits(v1, h1, m1, l1);
            F.p[0][e] = pack_hi16(h0, h1);
            F.p[1][e] = pack_hi16(m0_, m1);
            F.p[2][e] = pack_hi16(l0, l1);
        }
    };
    f32x16 acc[2][3];
#pragma unroll
    for (int rb = 0; rb < 2; rb++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rb][j][r] = 0.f;
    // W fragments of one k-step: three register groups of three column tiles; which group holds which plane rotates
    // (see the chunk loop) so that a plane's registers are refilled for the next k-step as soon as its last product of
    // the current one has been issued -- one group set instead of two, and every LDS read is ~200+ cycles ahead of its use.
    struct WGroup { bf16x8 t[3]; };
    auto ldW = [&](const __bf16 *Wp, int plane, int s2, WGroup &G) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            G.t[j] = *reinterpret_cast<const bf16x8 *>(Wp + plane * WPL + (32 * j + lrow) * SLD + 16 * lhalf + 8 * s2);
    };
    // one product = 3 MFMAs (the three column tiles): consecutive MFMAs never share an accumulator
    auto prod = [&](int rb, const u32x4 &a, const WGroup &G) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), G.t[j], acc[rb][j], 0, 0, 0);
    };
#define SPLIT_MIX(nmfma)                                                                                                   \
    _Pragma("unroll") for (int i_ = 0; i_ < (nmfma); i_++) {                                                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                 \
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                                                 \
    }                                                                                                                      \
    __builtin_amdgcn_sched_barrier(0)
    // First unit of a k-step (its W planes arrive lo, mid, hi): products lo.. first.  F = this unit's A fragment,
    // (nrb, ns, NF) = the fragment built meanwhile for the next unit.
#define SPLIT_UNIT_FIRST(rb, F, LO, MID, HI, nrb, ns, NF)                                                                  \
    prod(rb, F.p[0], LO); prod(rb, F.p[1], MID); prod(rb, F.p[0], MID); build(nrb, ns, NF, 0, 2); SPLIT_MIX(9);            \
    prod(rb, F.p[2], HI); prod(rb, F.p[1], HI); build(nrb, ns, NF, 2, 3); SPLIT_MIX(6);                                   \
    prod(rb, F.p[0], HI); build(nrb, ns, NF, 3, 4); SPLIT_MIX(3)
    // Second unit (same W fragments, other row block): hi products first, so the planes free up hi, mid, lo and are
    // refilled with the NEXT k-step's lo, mid, hi planes from Wsrc.
#define SPLIT_UNIT_SECOND(rb, F, LO, MID, HI, nrb, ns, NF, Wsrc, ws)                                                       \
    prod(rb, F.p[2], HI); prod(rb, F.p[1], HI); prod(rb, F.p[0], HI); build(nrb, ns, NF, 0, 2); SPLIT_MIX(9);              \
    ldW(Wsrc, 2, ws, HI); __builtin_amdgcn_sched_barrier(0);                                                               \
    prod(rb, F.p[1], MID); prod(rb, F.p[0], MID); build(nrb, ns, NF, 2, 3); SPLIT_MIX(6);                                 \
    ldW(Wsrc, 1, ws, MID); __builtin_amdgcn_sched_barrier(0);                                                              \
    prod(rb, F.p[0], LO); build(nrb, ns, NF, 3, 4); SPLIT_MIX(3);                                                          \
    ldW(Wsrc, 0, ws, LO); __builtin_amdgcn_sched_barrier(0)
#ifdef DSG_CLOCK_DIAG
    unsigned long long diag_t0 = 0, diag_r0 = 0;
    if (tid == 0) { diag_t0 = __builtin_amdgcn_s_memtime(); diag_r0 = __builtin_amdgcn_s_memrealtime(); }
#endif
    Frag F0, F1;
    WGroup G0, G1, G2;
    issueW(0);
    loadA(0, 0, 0); loadA(0, 1, 0); loadA(0, 0, 1); loadA(0, 1, 1);
    writeW(0);
    build(0, 0, F0, 0, 4);
    loadA(min(1, nk - 1), 0, 0);
    __syncthreads();
    ldW(lds, 2, 0, G0); ldW(lds, 1, 0, G1); ldW(lds, 0, 0, G2);   // k-step 0 of chunk 0: lo -> G0, mid -> G1, hi -> G2
    // Every prefetch is unconditional and in range: past the last chunk it re-reads the last chunk (never consumed), so
    // there are no branches and the scheduler sees straight-line code per chunk.
    for (int kc = 0; kc < nk; kc++) {
        const int cur = kc & 1;
        const __bf16 *Wc = lds + cur * 3 * WPL, *Wn = lds + (cur ^ 1) * 3 * WPL;
        const int kn = min(kc + 1, nk - 1), kn2 = min(kc + 2, nk - 1);
        issueW(kn);
        SPLIT_UNIT_FIRST(0, F0, G0, G1, G2, 1, 0, F1);
        loadA(kn, 1, 0);
        SPLIT_UNIT_SECOND(1, F1, G0, G1, G2, 0, 1, F0, Wc, 1);      // refills: lo -> G2, mid -> G1, hi -> G0 (k-step 1)
        loadA(kn, 0, 1);
        SPLIT_UNIT_FIRST(0, F0, G2, G1, G0, 1, 1, F1);
        loadA(kn, 1, 1);
        writeW(cur ^ 1);
        __syncthreads();   // the next chunk's W tile is complete; everybody is done reading this chunk's tile
        SPLIT_UNIT_SECOND(1, F1, G2, G1, G0, 0, 0, F0, Wn, 0);      // refills: lo -> G0, mid -> G1, hi -> G2 (next chunk)
        loadA(kn2, 0, 0);
    }
#ifdef DSG_CLOCK_DIAG
    if (tid == 0 && g_diag_buf) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        g_diag_buf[2 * bid] = t1 - diag_t0;
        g_diag_buf[2 * bid + 1] = r1 - diag_r0;
    }
#endif
#undef SPLIT_UNIT_FIRST
#undef SPLIT_UNIT_SECOND
#undef SPLIT_MIX
    __syncthreads();
    const float *gtab = reinterpret_cast<const float *>(lds);   // the W tiles are dead: reuse the LDS for the GELU table
    if (ACT == ACT_GELU && g.gelu_tab) {
        gelu_tab_to_lds(reinterpret_cast<float *>(lds), g.gelu_tab, tid, 64 * NW);
        __syncthreads();
    }
    const rsrc_t rsC = make_rsrc(g.C + (size_t)m0 * g.ldc, (unsigned)rows_m * g.ldc * 4u);
    const rsrc_t rsC2 = make_rsrc(g.C2 ? g.C2 + (size_t)m0 * g.ldc2 : g.C, g.C2 ? (unsigned)rows_m * g.ldc2 * 4u : 0u);
    const rsrc_t rsR = make_rsrc(RES ? g.res + (size_t)m0 * g.ldres : g.C, RES ? (unsigned)rows_m * g.ldres * 4u : 0u);
    const unsigned OOB = 0x7fffffffu;
#pragma unroll
    for (int rb = 0; rb < 2; rb++) {
        const unsigned rowl = (unsigned)(wave * 64 + rb * 32 + 4 * lhalf);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int n = n0 + 32 * j + lrow;
            const bool nok = n < g.N;
            const float bias = (g.bias && nok) ? g.bias[n] : 0.f;
            const unsigned vC = nok ? (rowl * g.ldc + (unsigned)n) * 4u : OOB;
            const unsigned vC2 = nok ? (rowl * g.ldc2 + (unsigned)n) * 4u : OOB;
            const unsigned vR = nok ? (rowl * g.ldres + (unsigned)n) * 4u : OOB;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const unsigned rr = (unsigned)((r & 3) + 8 * (r >> 2));
                float v = acc[rb][j][r] + bias;
                if (ACT == ACT_GELU) v = g.gelu_tab ? gelu_lut(v, gtab) : gelu_f(v);
                else if (ACT == ACT_SILU) v = silu_exact(v);
                if (RES) v += buf_load1(rsR, vR, rr * g.ldres * 4u);
                buf_store1(v, rsC, vC, rr * g.ldc * 4u);
                if (g.C2) buf_store1(v, rsC2, vC2, rr * g.ldc2 * 4u);
            }
        }
    }
}

// fp32 [n] -> three bf16 planes [3][n] with hi + mid + lo == value to 24 bits (pack time)
__global__ void f32_split3_kernel(const float *src, __bf16 *dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        unsigned h, m, l; split3_bits(src[i], h, m, l);
        unsigned short *d = reinterpret_cast<unsigned short *>(dst);
        d[i] = (unsigned short)(h >> 16); d[n + i] = (unsigned short)(m >> 16); d[2 * n + i] = (unsigned short)(l >> 16);
    }
}
void launch_f32_split3(const float *src, void *dst, size_t n, hipStream_t s) {
    DSG_LAUNCH(f32_split3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (__bf16 *)dst, n);
}

// fp32 [n] -> bf16 [n] (RNE), used once per weight at pack time
__global__ void f32_to_bf16_kernel(const float *src, __bf16 *dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) reinterpret_cast<unsigned short *>(dst)[i] = (unsigned short)(bf16_rne_hi(src[i]) >> 16);
}
void launch_f32_to_bf16(const float *src, void *dst, size_t n, hipStream_t s) {
    DSG_LAUNCH(f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (__bf16 *)dst, n);
}


__global__ void bf16_to_f32_kernel(const unsigned short *src, float *dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = __uint_as_float((unsigned)src[i] << 16);
}
void launch_bf16_to_f32(const void *src, float *dst, size_t n, hipStream_t s) {   // test / debug entries only
    DSG_LAUNCH(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned short *)src, dst, n);
}

static int round_up8(int x) { return (x + 7) / 8 * 8; }

thread_local int g_lp_tile_hook = 0;
thread_local int g_lp_tile_rows = 0;

bool launch_gemm_lp(const GemmArgs &g_in, hipStream_t s) {
    g_lp_tile_rows = 0;
    if (!g_in.Ws3 && !(g_in.Wb && (!g_in.A2 || g_in.K1 % HBK == 0))) return false;
    // the split kernel switches sources at chunk K1 / SBK: a K1 inside a chunk would read the wrong columns of both (no caller has one:
    // the forward's concat widths are multiples of 96)
    if (g_in.Ws3 && g_in.A2 && g_in.K1 % SBK != 0) return false;
    GemmArgs g = g_in;
    g.gelu_tab = gelu_table();
    const int tiles_n = (g.N + GBN - 1) / GBN;
    const bool split = g.Ws3 != nullptr;
    // bf16 kernel: the 256x96 tile (RB = 2, a wave owns 64 rows) wherever there are enough rows to fill the chip with it
    static const bool narrow_only = getenv("DSG_BF16_NARROW") != nullptr;   // dev knob: A/B against the 128x96 tile
    static const bool force_wide = getenv("DSG_BF16_WIDE") != nullptr;      // tests: the wide tile at every size
    // (g_fixed_tiles, option "batch_invariant": the choice below depends on M, i.e. on the batch size -- the 128x96 tile at every size)
    const bool rule_wide = !narrow_only && !g_fixed_tiles && (force_wide ? g.M >= 256 : (size_t)((g.M + 255) / 256) * tiles_n >= 512);
    const bool wide = !split && (g_lp_tile_hook ? g_lp_tile_hook == 2 : rule_wide);   // (the test hook of kernels.h comes first; 0: the rule)
    const int tile_m = split ? 256 : (wide ? 2 * GBM : GBM);
    const int tiles_m = (g.M + tile_m - 1) / tile_m;
    g_lp_tile_rows = tile_m;
    const dim3 grid(round_up8(tiles_m) * tiles_n), block(256);
#define LAUNCH_BF16(L, A, R, E, AB, CB)                                                                                           \
    do {                                                                                                                          \
        if (wide) DSG_LAUNCH((gemm_bf16_kernel<L, A, R, E, AB, CB, 2>), grid, block, 0, s, g, tiles_m, tiles_n);          \
        else DSG_LAUNCH((gemm_bf16_kernel<L, A, R, E, AB, CB, 1>), grid, block, 0, s, g, tiles_m, tiles_n);               \
    } while (0)
    const bool ln = g.ln_stats != nullptr || g.ln_part != nullptr, res = g.res != nullptr;
    if (g.a4_res > 0 || g.attn_bias) return false;               // fp32-kernel-only features
    if (g.a_bf16 || g.c_bf16) {   // bf16 tensors between kernels: only the shapes the forward uses; anything else is a caller bug
        const bool a_ok = g.a_bf16 && !g.c_bf16 && !split && !ln && g.act == ACT_NONE && res && !g.A2 && g.K % HBK == 0;
        const bool c_ok = g.c_bf16 && !g.a_bf16 && !split && ln && (g.act == ACT_GELU || g.act == ACT_NONE) && !res && !g.stats_out && !g.C2;
        if (!a_ok && !c_ok) return false;   // not built: launch_gemm reports it to the caller (nothing launched)
        if (c_ok) {
            if (g.act == ACT_GELU) LAUNCH_BF16(true, ACT_GELU, false, 0, false, true);
            else LAUNCH_BF16(true, ACT_NONE, false, 0, false, true);
            return true;
        }
        const int epi = !g.stats_out ? 0 : !g.mod_aff ? 1 : (g.mod_ld == 0 ? 2 : 3);
#define LP_ABF(E) LAUNCH_BF16(false, ACT_NONE, true, E, true, false)
        if (epi == 0) LP_ABF(0); else if (epi == 1) LP_ABF(1); else if (epi == 2) LP_ABF(2); else LP_ABF(3);
#undef LP_ABF
        return true;
    }
    if (split && (g.stats_out || g.ln_part)) return false;       // the split kernel has no epilogue extensions
    if (g.stats_out) {
        if (ln || g.act != ACT_NONE) return false;
        const int epi = !g.mod_aff ? 1 : (g.mod_ld == 0 ? 2 : 3);
#define LP_EPI(R, E) LAUNCH_BF16(false, ACT_NONE, R, E, false, false)
        if (res) { if (epi == 1) LP_EPI(true, 1); else if (epi == 2) LP_EPI(true, 2); else LP_EPI(true, 3); }
        else { if (epi == 1) LP_EPI(false, 1); else if (epi == 2) LP_EPI(false, 2); else LP_EPI(false, 3); }
#undef LP_EPI
        return true;
    }
#define GEMM_CASE(L, A, R)                                                                                     \
    do {                                                                                                       \
        if (split) DSG_LAUNCH((gemm_split2_kernel<L, A, R, 4>), grid, block, 0, s, g, tiles_m, tiles_n); \
        else LAUNCH_BF16(L, A, R, 0, false, false);                                                                \
    } while (0)
    if (ln && g.act == ACT_NONE && !res) GEMM_CASE(true, ACT_NONE, false);
    else if (ln && g.act == ACT_GELU && !res) GEMM_CASE(true, ACT_GELU, false);
    else if (!ln && g.act == ACT_NONE && res) GEMM_CASE(false, ACT_NONE, true);
    else if (!ln && g.act == ACT_NONE && !res) GEMM_CASE(false, ACT_NONE, false);
    else if (!ln && g.act == ACT_GELU && !res) GEMM_CASE(false, ACT_GELU, false);
    else if (!ln && g.act == ACT_SILU && !res) GEMM_CASE(false, ACT_SILU, false);
    else if (ln && g.act == ACT_NONE && res) GEMM_CASE(true, ACT_NONE, true);
    else if (ln && g.act == ACT_GELU && res) GEMM_CASE(true, ACT_GELU, true);
    else if (ln && g.act == ACT_SILU && !res) GEMM_CASE(true, ACT_SILU, false);
    else if (ln && g.act == ACT_SILU && res) GEMM_CASE(true, ACT_SILU, true);
    else if (!ln && g.act == ACT_GELU && res) GEMM_CASE(false, ACT_GELU, true);
    else GEMM_CASE(false, ACT_SILU, true);
#undef GEMM_CASE
    return true;
}

}  // namespace dsg
