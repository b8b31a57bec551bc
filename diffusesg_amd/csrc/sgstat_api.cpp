// sgstat_api.cpp -- C ABI of the scene-graph statistics kernels (include/dsg.h, "Scene-graph statistics"): argument checks and
// launches.
#include "../../include/dsg.h"
#include "sgstat_kernels.h"

#include <hip/hip_runtime.h>

using namespace dsg;

static int launched() { return hipGetLastError() == hipSuccess ? DSG_OK : DSG_ERR_HIP; }

extern "C" {

int dsg_sgstat_triplet_counts(int32_t B, int32_t N, const int32_t *edge_types, const int32_t *node_types, int32_t n_keys,
                              const int64_t *sorted_keys, const int32_t *key_pos, int64_t *counts, int64_t *novel, void *stream) {
    if (B < 1 || N < 1 || n_keys < 0 || !edge_types || !node_types || !novel || (n_keys > 0 && (!sorted_keys || !key_pos || !counts)))
        return DSG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_keys > 0 && hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)n_keys, s) != hipSuccess) return DSG_ERR_HIP;
    if (hipMemsetAsync(novel, 0, sizeof(int64_t), s) != hipSuccess) return DSG_ERR_HIP;
    launch_sgstat_triplet_counts(B, N, edge_types, node_types, n_keys, sorted_keys, key_pos, counts, novel, s);
    return launched();
}

int dsg_sgstat_layout(int32_t B, int32_t N, const float *boxes, const uint8_t *flags, int32_t canvas_size, double *values,
                      uint8_t *valid, void *stream) {
    if (B < 1 || N < 1 || N > kSgstatMaxNodes || canvas_size < 1 || canvas_size > kSgstatMaxCanvas || !boxes || !flags || !values ||
        !valid)
        return DSG_ERR_INVALID;
    launch_sgstat_layout(B, N, boxes, flags, canvas_size, values, valid, (hipStream_t)stream);
    return launched();
}

int dsg_sgstat_f1_rowstats(int32_t rows, int32_t Y, int32_t W, const double *blk, double *row_max, double *row_mean,
                           double *row_median, int32_t *row_argmax, void *stream) {
    if (rows < 1 || Y < 1 || Y > kSgstatMaxRow || W < 1 || W > kSgstatMaxWeights || !blk || !row_max || !row_mean || !row_median ||
        !row_argmax)
        return DSG_ERR_INVALID;
    if (!launch_sgstat_f1_rowstats(rows, Y, W, blk, row_max, row_mean, row_median, row_argmax, (hipStream_t)stream)) return DSG_ERR_HIP;
    return launched();
}

}  // extern "C"
