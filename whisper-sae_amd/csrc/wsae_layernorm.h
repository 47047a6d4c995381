// Row LayerNorm pieces shared by the kernels that apply it (wsae_ring.hip: ring_push_ln_kernel, which also serves
// wsae_layernorm_rows) and the one that inverts it (wsae_intervene.hip): one wave per row, lane l owns columns
// l, l + 64, ..  Both sides take the row statistics from these functions, so the mean and the variance an intervention
// undoes are the ones the encoder's input was normalised with, operation for operation.
#pragma once

#include "wsae_common.h"

#ifdef __HIPCC__

// v[i] = row r, column lane + 64 i (0 beyond dim); returns the lane's partial sum in column order
template <int SRC, int VPL>
__device__ __forceinline__ float ln_row_load(const void* __restrict__ src, int64_t r, int dim, int lane, float (&v)[VPL]) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int d = lane + 64 * i;
        v[i] = 0.f;
        if (d < dim) v[i] = SRC == WSAE_DT_F32 ? ((const float*)src)[r * dim + d] : (float)((const bf16_t*)src)[r * dim + d];
        sum += v[i];
    }
    return sum;
}

// mean and (biased variance + eps) of the row by wave reductions, two passes over the registers
template <int VPL>
__device__ __forceinline__ void ln_row_stats(const float (&v)[VPL], float sum, int dim, int lane, float eps, float& mean,
                                             float& var_eps) {
    mean = wave_sum(sum) / (float)dim;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const float c = lane + 64 * i < dim ? v[i] - mean : 0.f;
        sq = fmaf(c, c, sq);
    }
    var_eps = wave_sum(sq) / (float)dim + eps;  // biased variance, as torch.nn.LayerNorm
}

#endif  // __HIPCC__
