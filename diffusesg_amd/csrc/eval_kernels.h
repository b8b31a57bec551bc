// eval_kernels.h -- launch wrappers of the sample-evaluation kernels (eval_kernels.hip), used by eval_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dsg {

constexpr int kEvalMaxNodes = 255;     // node index, rank and per-class count are packed as bytes
constexpr int kEvalMaxClasses = 192;   // class bitmask: 6 dwords
constexpr int kEvalMaskWords = kEvalMaxClasses / 32;
constexpr int kEvalMaxWeights = 8;
constexpr int kEvalMaxIou = 16;
constexpr int kEvalMaxTypes = 1024;    // histogram bins of one LDS block

// Byte offsets of the arrays of one prepared scene set (dsg_eval_bbox_prep) inside the caller's buffer.  S scenes of N nodes:
//   box  float4 [N][S]   (x1, y1, x2, y2) as given; node-major so that consecutive scenes of one node are adjacent
//   ep   double [S][N]   per detection, in (class, node) order: (H(ndet) - H(rank)) / ndet   (its share of mean precision)
//   er   double [S][N]   (ndet - rank) / ndet                                               (its share of mean recall * npos)
//   sw   double [S][W]   sum of the class weights over the classes present
//   cls  int32  [N][S]   class of a valid box, -1 otherwise
//   ent  uint32 [S][N]   valid boxes sorted by (class, node): node | class << 8 | rank << 16 | ndet << 24
//   nval int32  [S]      number of valid boxes
//   mask uint32 [6][S]   classes present
//   cnt  uint8  [192][S] valid boxes per class
struct EvalPrepLayout {
    size_t box, ep, er, sw, cls, ent, nval, mask, cnt, total;
};

__host__ __device__ inline size_t eval_align256(size_t b) { return (b + 255) / 256 * 256; }

__host__ __device__ inline EvalPrepLayout eval_prep_layout(int S, int N, int W) {
    EvalPrepLayout L;
    size_t o = 0, s = (size_t)S, n = (size_t)N;
    L.box = o;  o += eval_align256(16 * n * s);
    L.ep = o;   o += eval_align256(8 * n * s);
    L.er = o;   o += eval_align256(8 * n * s);
    L.sw = o;   o += eval_align256(8 * (size_t)W * s);
    L.cls = o;  o += eval_align256(4 * n * s);
    L.ent = o;  o += eval_align256(4 * n * s);
    L.nval = o; o += eval_align256(4 * s);
    L.mask = o; o += eval_align256(4 * (size_t)kEvalMaskWords * s);
    L.cnt = o;  o += eval_align256((size_t)kEvalMaxClasses * s);
    L.total = o;
    return L;
}

struct EvalIou {
    double thr[kEvalMaxIou];
    int n;
};

void launch_eval_bbox_prep(int S, int N, int C, const float *boxes, const int32_t *classes, const uint8_t *flags, int W,
                           const double *weights, void *prep, hipStream_t s);
void launch_eval_bbox_f1(const void *gen_prep, int X, const void *ref_prep, int Y, int N, int C, int W, const double *weights,
                         const EvalIou &iou, int x0, int x1, int y0, int y1, double *out, hipStream_t s);
void launch_eval_type_hist(int B, int N, int K, int edges, const int32_t *types, const uint8_t *flags, double *hist, int ld,
                           double *sums, hipStream_t s);
void launch_eval_degree_hist(int B, int N, const float *adj, double *hist, int ld, double *sums, hipStream_t s);
void launch_eval_hist_mmd(int n_ref, const double *ref, int ld_ref, int n_gen, const double *gen, int ld_gen, int L, double *ws,
                          double *out, hipStream_t s);

}  // namespace dsg
