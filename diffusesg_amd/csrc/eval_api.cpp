// eval_api.cpp -- C ABI of the sample-evaluation kernels (include/dsg.h, "Sample evaluation"): argument checks and launches.
#include "../../include/dsg.h"
#include "eval_kernels.h"

#include <hip/hip_runtime.h>

using namespace dsg;

static int launched() { return hipGetLastError() == hipSuccess ? DSG_OK : DSG_ERR_HIP; }

extern "C" {

size_t dsg_eval_bbox_prep_bytes(int32_t S, int32_t N, int32_t W) {
    if (S < 1 || N < 1 || W < 1) return 0;
    return eval_prep_layout(S, N, W).total;
}

int dsg_eval_bbox_prep(int32_t S, int32_t N, int32_t n_classes, const float *boxes, const int32_t *classes, const uint8_t *flags,
                       int32_t W, const double *weights, void *prep, void *stream) {
    if (S < 1 || N < 1 || N > kEvalMaxNodes || n_classes < 1 || n_classes > kEvalMaxClasses || W < 1 || W > kEvalMaxWeights ||
        (!weights && W != 1) || !boxes || !classes || !flags || !prep)
        return DSG_ERR_INVALID;
    launch_eval_bbox_prep(S, N, n_classes, boxes, classes, flags, W, weights, prep, (hipStream_t)stream);
    return launched();
}

int dsg_eval_bbox_f1(const void *gen_prep, int32_t X, const void *ref_prep, int32_t Y, int32_t N, int32_t n_classes, int32_t W,
                     const double *weights, int32_t n_iou, const double *iou_thresholds, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                     double *out, void *stream) {
    if (!gen_prep || !ref_prep || !out || !iou_thresholds || X < 1 || Y < 1 || N < 1 || N > kEvalMaxNodes || n_classes < 1 ||
        n_classes > kEvalMaxClasses || W < 1 || W > kEvalMaxWeights || (!weights && W != 1) || n_iou < 1 || n_iou > kEvalMaxIou ||
        x0 < 0 || x1 > X || x0 >= x1 || y0 < 0 || y1 > Y || y0 >= y1)
        return DSG_ERR_INVALID;
    EvalIou iou{};
    iou.n = n_iou;
    for (int t = 0; t < n_iou; t++) iou.thr[t] = iou_thresholds[t];
    launch_eval_bbox_f1(gen_prep, X, ref_prep, Y, N, n_classes, W, weights, iou, x0, x1, y0, y1, out, (hipStream_t)stream);
    return launched();
}

int dsg_eval_type_hist(int32_t B, int32_t N, int32_t K, int32_t edges, const int32_t *types, const uint8_t *flags, double *hist,
                       int32_t ld, double *sums, void *stream) {
    if (B < 1 || N < 1 || K < (edges ? 2 : 1) || K > kEvalMaxTypes || (edges != 0 && edges != 1) || ld < B || !types || !flags ||
        !hist || !sums)
        return DSG_ERR_INVALID;
    launch_eval_type_hist(B, N, K, edges, types, flags, hist, ld, sums, (hipStream_t)stream);
    return launched();
}

int dsg_eval_degree_hist(int32_t B, int32_t N, const float *adj, double *hist, int32_t ld, double *sums, void *stream) {
    if (B < 1 || N < 1 || N > kEvalMaxTypes || ld < B || !adj || !hist || !sums) return DSG_ERR_INVALID;
    launch_eval_degree_hist(B, N, adj, hist, ld, sums, (hipStream_t)stream);
    return launched();
}

int dsg_eval_hist_mmd(int32_t n_ref, const double *ref, int32_t ld_ref, int32_t n_gen, const double *gen, int32_t ld_gen, int32_t L,
                      double *ws, double *out, void *stream) {
    if (n_ref < 1 || n_gen < 1 || L < 1 || L > kEvalMaxTypes || ld_ref < n_ref || ld_gen < n_gen || !ref || !gen || !ws || !out)
        return DSG_ERR_INVALID;
    launch_eval_hist_mmd(n_ref, ref, ld_ref, n_gen, gen, ld_gen, L, ws, out, (hipStream_t)stream);
    return launched();
}

}  // extern "C"
