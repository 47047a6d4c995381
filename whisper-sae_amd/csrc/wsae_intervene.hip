// Causal feature interventions (row N5): the edited compact code of a layer's activations written back into the
// layer's output.  The reference has no code for this (its whisper_sae.causal package is a docstring); the arithmetic
// is include/wsae.h's, section "causal feature interventions".
//
// One wave per row.  The row's code sits one entry per lane (two for k > 64), the weight every entry contributes with
// (act' - act when the reconstruction error stays in the stream, act' when the reconstruction replaces it) is computed
// there, and a ballot of the non-zero weights is all the wave needs to decide what to do: nothing at all (an
// unedited row of an in-place call reads 8 k bytes and returns), a copy, or a gather of exactly the decoder rows
// that matter - usually one or two, not k.  The ballot is wave-uniform, so that loop does not diverge.  Lanes own
// columns lane, lane + 64, .. as in the LayerNorm kernel, and mean / variance come from the functions that kernel
// uses (wsae_layernorm.h), so the sigma that scales the edit back is the one the encoder's input was divided by.
// Sums are fp32 fmaf chains in a fixed order (entries ascending, then the forced features in list order): there
// are no float atomics and two launches give the same bits.
#include "wsae_common.h"
#include "wsae_layernorm.h"

template <typename WT>
__device__ __forceinline__ float load_w(const WT* __restrict__ w, int64_t i) { return (float)w[i]; }

template <int DT>
__device__ __forceinline__ void store_act(void* __restrict__ p, int64_t i, float v) {
    if (DT == WSAE_DT_BF16) ((bf16_t*)p)[i] = (bf16_t)v;
    else ((float*)p)[i] = v;
}

template <int HDT, int ODT, typename WT, int VPL>
__global__ void __launch_bounds__(256) intervene_kernel(
    const WT* __restrict__ WdT, const float* __restrict__ bd, const float* __restrict__ bpre, const void* h,
    int64_t n_rows, int dim, int H, int K, const float* __restrict__ vals, const int32_t* __restrict__ idx,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, const float* __restrict__ scale,
    const int32_t* __restrict__ force_idx, const float* __restrict__ force_val, int n_force,
    const uint8_t* __restrict__ row_mask, int mode, void* out, int32_t* __restrict__ changed_rows) {
    __shared__ int wave_changed[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in_place = (const void*)out == h;
    int changed = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_rows; r += (int64_t)gridDim.x * 4) {
        const bool selected = !row_mask || row_mask[r] != 0;
        // the row's code, entry j = lane + 64 s in slot s, and the weight it enters the sum with
        float w[2];
        int ix[2];
        bool valid[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = lane + 64 * s;
            valid[s] = j < K;
            ix[s] = valid[s] ? idx[r * K + j] : -1;
            valid[s] = valid[s] && (unsigned)ix[s] < (unsigned)H;
            const float act = valid[s] ? fmaxf(vals[r * K + j], 0.f) : 0.f;
            float edited = act;
            if (selected && valid[s] && scale) edited = scale[ix[s]] * act;
            w[s] = mode == WSAE_IV_REPLACE ? edited : edited - act;
        }
        // forced features: the entry that holds one takes its value; one that no entry holds is a term of its own
        unsigned long long outside = 0ull;
        if (selected) {
            for (int f = 0; f < n_force; ++f) {
                const int fi = force_idx[f];
                const float cf = force_val[f];
                if ((unsigned)fi >= (unsigned)H) continue;
                bool hit = false;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (valid[s] && ix[s] == fi) {
                        const float act = fmaxf(vals[r * K + lane + 64 * s], 0.f);
                        w[s] = mode == WSAE_IV_REPLACE ? cf : cf - act;
                        hit = true;
                    }
                }
                if (__ballot(hit) == 0ull && cf != 0.f) outside |= 1ull << f;
            }
        }
        unsigned long long m[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) m[s] = __ballot(valid[s] && w[s] != 0.f);
        const bool edit = mode == WSAE_IV_REPLACE || (m[0] | m[1] | outside) != 0ull;
        if (!edit) {  // bit-identical row: nothing to store in place, a copy otherwise
            if (!in_place) {
#pragma unroll
                for (int i = 0; i < VPL; ++i) {
                    const int d = lane + 64 * i;
                    if (d < dim) store_act<ODT>(out, r * dim + d, load_act<HDT>(h, r * dim + d));
                }
            }
            continue;
        }
        ++changed;
        float v[VPL];
        const float sum = ln_row_load<HDT, VPL>(h, r, dim, lane, v);
        float mean = 0.f, sigma = 1.f;
        if (gamma) {
            float var_eps;
            ln_row_stats<VPL>(v, sum, dim, lane, eps, mean, var_eps);
            sigma = __fsqrt_rn(var_eps);
        }
        float acc[VPL];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int d = lane + 64 * i;
            acc[i] = (mode == WSAE_IV_REPLACE && d < dim) ? bd[d] + bpre[d] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned long long bits = m[s];
            while (bits) {
                const int j = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const float wj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(w[s]), j));
                const int ij = __builtin_amdgcn_readlane(ix[s], j);
                const WT* row = WdT + (int64_t)ij * dim;
#pragma unroll
                for (int i = 0; i < VPL; ++i) {
                    const int d = lane + 64 * i;
                    if (d < dim) acc[i] = fmaf(wj, load_w(row, d), acc[i]);
                }
            }
        }
        while (outside) {
            const int f = __ffsll((long long)outside) - 1;
            outside &= outside - 1;
            const float cf = force_val[f];
            const WT* row = WdT + (int64_t)force_idx[f] * dim;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int d = lane + 64 * i;
                if (d < dim) acc[i] = fmaf(cf, load_w(row, d), acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int d = lane + 64 * i;
            if (d >= dim) continue;
            float y;
            if (mode == WSAE_IV_REPLACE) y = gamma ? mean + __fdiv_rn(sigma * (acc[i] - beta[d]), gamma[d]) : acc[i];
            else y = v[i] + (gamma ? __fdiv_rn(sigma * acc[i], gamma[d]) : acc[i]);
            store_act<ODT>(out, r * dim + d, y);
        }
    }
    if (!changed_rows) return;
    if (lane == 0) wave_changed[wave] = changed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = wave_changed[0] + wave_changed[1] + wave_changed[2] + wave_changed[3];
        if (n) atomicAdd(changed_rows, n);
    }
}

extern "C" int wsae_intervene(wsae_ctx* ctx, const float* params, const void* h, int32_t h_dtype, int64_t n_rows,
                              const float* vals, const int32_t* idx, const float* gamma, const float* beta, float eps,
                              const float* scale, const int32_t* force_idx, const float* force_val, int32_t n_force,
                              const uint8_t* row_mask, int32_t mode, void* out, int32_t out_dtype, int32_t* changed_rows,
                              void* stream) {
    WSAE_REQUIRE(ctx && params && h && vals && idx && out && n_rows >= 0, "wsae_intervene: bad argument");
    WSAE_REQUIRE(h_dtype == WSAE_DT_F32 || h_dtype == WSAE_DT_BF16, "wsae_intervene: unknown input dtype %d", h_dtype);
    WSAE_REQUIRE(out_dtype == WSAE_DT_F32 || out_dtype == WSAE_DT_BF16, "wsae_intervene: unknown output dtype %d", out_dtype);
    WSAE_REQUIRE(mode == WSAE_IV_KEEP_ERROR || mode == WSAE_IV_REPLACE, "wsae_intervene: unknown mode %d", mode);
    WSAE_REQUIRE(n_force >= 0 && n_force <= WSAE_IV_MAX_FORCE, "wsae_intervene: %d forced features (at most %d)", n_force,
                 WSAE_IV_MAX_FORCE);
    WSAE_REQUIRE(n_force == 0 || (force_idx && force_val), "wsae_intervene: forced features without their tables");
    WSAE_REQUIRE(!gamma || beta, "wsae_intervene: gamma without beta");
    WSAE_REQUIRE(out != h || out_dtype == h_dtype, "wsae_intervene: an in-place call cannot change the dtype");
    WSAE_REQUIRE(ctx->D <= 2048 && ctx->K <= 128, "wsae_intervene: input_dim %d / k %d outside the kernel's range", ctx->D, ctx->K);
    hipStream_t st = (hipStream_t)stream;
    if (changed_rows) WSAE_HIP_CHECK(hipMemsetAsync(changed_rows, 0, sizeof(int32_t), st));
    if (n_rows == 0) return WSAE_OK;
    const float* bd = params + ctx->off[3];
    const float* bpre = params + ctx->off[4];
    // (columns beyond the row add exact zeros to a lane's partial sum, so the registers per lane may differ from the
    // LayerNorm kernel's without changing the statistics)
    // a few rows per wave once the grid fills the chip: one counter update per block, not per row
    const unsigned nb = (unsigned)min(ceil_div64(n_rows, 4), (int64_t)8 * ctx->cus);
#define IV_LAUNCH(HD, OD, WT, W, V)                                                                                   \
    intervene_kernel<HD, OD, WT, V><<<nb, 256, 0, st>>>(W, bd, bpre, h, n_rows, ctx->D, ctx->H, ctx->K, vals, idx, gamma, \
                                                        beta, eps, scale, force_idx, force_val, n_force, row_mask,    \
                                                        mode, out, changed_rows)
#define IV_WIDTH(HD, OD, WT, W)                                \
    do {                                                       \
        if (ctx->D <= 512) IV_LAUNCH(HD, OD, WT, W, 8);        \
        else if (ctx->D <= 1024) IV_LAUNCH(HD, OD, WT, W, 16); \
        else IV_LAUNCH(HD, OD, WT, W, 32);                     \
    } while (0)
#define IV_DTYPES(WT, W)                                                                                   \
    do {                                                                                                   \
        if (h_dtype == WSAE_DT_F32 && out_dtype == WSAE_DT_F32) IV_WIDTH(WSAE_DT_F32, WSAE_DT_F32, WT, W);  \
        else if (h_dtype == WSAE_DT_F32) IV_WIDTH(WSAE_DT_F32, WSAE_DT_BF16, WT, W);                       \
        else if (out_dtype == WSAE_DT_F32) IV_WIDTH(WSAE_DT_BF16, WSAE_DT_F32, WT, W);                     \
        else IV_WIDTH(WSAE_DT_BF16, WSAE_DT_BF16, WT, W);                                                  \
    } while (0)
    // the decoder rows the ctx's decode reads: the bf16 shadow in BF16 mode, the pack's fp32 rows in FP32 mode
    if (ctx->prec == WSAE_PREC_BF16) IV_DTYPES(bf16_t, (const bf16_t*)ctx->WdT_bf16);
    else IV_DTYPES(float, params + ctx->off[1]);
#undef IV_DTYPES
#undef IV_WIDTH
#undef IV_LAUNCH
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
