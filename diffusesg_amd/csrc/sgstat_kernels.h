// sgstat_kernels.h -- launch wrappers of the scene-graph statistics kernels (sgstat_kernels.hip), used by sgstat_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dsg {

constexpr int kSgstatMaxNodes = 255;      // one thread per box in the layout kernel (as the F1 kernel's bound)
constexpr int kSgstatMaxCanvas = 64;      // perceptual-IoU canvas side
constexpr int kSgstatMaxRow = 16384;      // an F1 row of float64 held in LDS: 128 KiB of the CU's 160
constexpr int kSgstatMaxWeights = 8;
constexpr int kSgstatKeyBits = 21;        // (subject type, object type, predicate) packed into one int64 key

void launch_sgstat_triplet_counts(int B, int N, const int32_t *edge_types, const int32_t *node_types, int n_keys,
                                  const int64_t *sorted_keys, const int32_t *key_pos, int64_t *counts, int64_t *novel, hipStream_t s);
void launch_sgstat_layout(int B, int N, const float *boxes, const uint8_t *flags, int canvas, double *values, uint8_t *valid,
                          hipStream_t s);
bool launch_sgstat_f1_rowstats(int rows, int Y, int W, const double *blk, double *row_max, double *row_mean, double *row_median,
                               int32_t *row_argmax, hipStream_t s);

}  // namespace dsg
