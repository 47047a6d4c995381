// Gradient-based feature attribution (attribution patching): the first-order effect on a scalar
// metric of the edit wsae_intervene applies in WSAE_IV_KEEP_ERROR mode, for every (row, code entry) pair and summed
// per feature, from one gradient G = dm/dh' of the clean run.  The arithmetic is include/wsae.h's, section "feature
// attribution".  It is the exact first-order term of the intervention, whose mean and sigma are frozen - not of a
// differentiated LayerNorm.
//
// Launches on the caller's stream: a memset node over the workspace, then
//   attribute_kernel    attr[r, j] = sigma_r * w_j * sum_d (G[r,d] / gamma_d) W_dT[i_j, d], and the call's max |attr|
//   attr_sum_kernel     every entry with w_j != 0 adds rint(attr / q) (and of |attr|) to its feature's int64 sums
//   attr_finish_kernel  feat_sum / feat_abs = float(sum * q), rounded once; feat_rows
// (the last two only when a per-feature output is asked for).
//
// attribute_kernel has the shape of intervene_kernel: one wave per row (a few rows per wave once the grid fills the
// chip), lanes own columns lane, lane + 64, .., u_d = G_d / gamma_d and sigma stay in registers, and a wave-uniform
// ballot of w_j != 0 drives the gather over exactly the decoder rows that matter; an entry with w_j == 0 stores 0.0f
// and its decoder row is never read.  Unlike an ablation of a few features the default edit touches every active
// entry, so up to k dot products per row have to be reduced across the wave.  The lanes keep their partial sums of 16
// entries (8 and 4 for wide rows, below) (fp32 fmaf chains in column order) and fold them together in a transposing butterfly on the lane
// exchanges of wsae_common.h: the steps over lane distance 1, 2, 4 and 8 each halve the entries a lane still
// carries (it keeps one half and hands the other to its partner), the steps over 16 and 32 finish the one that is
// left: 17 exchanges per 16 entries instead of 96, and lane l ends with the sum of entry bitrev4(l & 15).  One
// ds_bpermute per group hands every entry's sum to the lane that owns the entry.  Every entry is reduced by the same
// tree whatever its place in the group, the row's result depends on nothing but the row, and there are no float
// atomics: two launches, any grid and any order of the rows give the same attr bits.
//
// Per-feature sums are exact fixed point, so they do not depend on the order of the adds either: with A = max |attr|
// of the call (an atomic max on the bits of non-negative floats, which order like the floats), A < 2^e and
// q = 2^(e - 36), every entry adds the integer rint(attr / q), |.| < 2^36, with 64-bit integer atomics; n_rows * k
// <= 2^26 entries (more is rejected) stay below 2^62.  The quantisation error is at most q / 2 = 2^(e - 37) per
// entry.  A == 0 gives zeros.
//
// Non-finite values: an Inf or NaN attr (an Inf gradient, an overflow) makes the call's maximum Inf; no integer is then
// added, and feat_sum / feat_abs are NaN for every feature of the call.  attr itself carries the non-finite entries and
// feat_rows stays exact.
//
// Wide rows (D > 512).  Per-lane guards `column < dim` on 16 or 32 column slots, the same in every row, are exec masks the
// compiler computes once and keeps in scalar registers for the whole kernel: more than there are (2 spilled at D <= 1024,
// 47 at D <= 2048 with the guards written as at D <= 512).  Those two instantiations therefore read h, G, gamma and the
// decoder rows through buffer descriptors that cover exactly one row each, so the hardware range check returns the zeros
// beyond the row and no guard exists, take dim through an opaque per-row copy, and fold groups of 8 and 4 entries
// (10 exchanges per 8, 7 per 4).  The values and the order of every sum are those of the D <= 512 form.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; VGPRs / SGPRs / scratch bytes /
// SGPR spills / VGPR spills / waves per SIMD), attribute_kernel<h dtype, G dtype, decoder row type, registers per lane,
// group>, the worst of the four h / G dtype pairs of each:
//   VPL  8, group 16 (D <=  512):  bf16 rows  56 / 92 / 0 / 0 / 0 / 8,  fp32 rows  55 / 92 / 0 / 0 / 0 / 8
//   VPL 16, group  8 (D <= 1024):  bf16 rows 127 / 88 / 0 / 0 / 0 / 4,  fp32 rows 128 / 88 / 0 / 0 / 0 / 4
//   VPL 32, group  4 (D <= 2048):  bf16 rows 167 / 88 / 0 / 0 / 0 / 3,  fp32 rows 168 / 88 / 0 / 0 / 0 / 3
// attr_sum_kernel 21 / 56 / 0 / 0 / 0 / 8, attr_finish_kernel 7 / 16 / 0 / 0 / 0 / 8.  No instantiation spills a scalar
// or a vector register.
#include "wsae_common.h"
#include "wsae_layernorm.h"

#define AT_FLT_MAX 3.4028234663852886e38f
#define AT_FRAC_BITS 36      // q = 2^(e - AT_FRAC_BITS)
#define AT_MAX_ENTRIES (1ll << 26)
#define AT_HEAD_BYTES 16     // workspace: the bits of max |attr|, padded; then int64 sum[H], int64 abs[H], int32 rows[H]

template <typename WT>
__device__ __forceinline__ float at_load_w(const WT* __restrict__ w, int64_t i) { return (float)w[i]; }

// element at byte offset `off` of the row behind `rs`, 0 beyond its end
template <typename WT>
__device__ __forceinline__ float at_load_row(__amdgpu_buffer_rsrc_t rs, int off) {
    if constexpr (sizeof(WT) == 2) return (float)__builtin_bit_cast(bf16_t, __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
    else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}

template <int DT>
__device__ __forceinline__ constexpr int at_bytes() { return DT == WSAE_DT_BF16 ? 2 : 4; }
// element `i` of the activation row behind `rs` as float, 0 beyond its end
template <int DT>
__device__ __forceinline__ float at_load_act(__amdgpu_buffer_rsrc_t rs, int i) {
    if constexpr (DT == WSAE_DT_BF16) return (float)__builtin_bit_cast(bf16_t, __builtin_amdgcn_raw_buffer_load_b16(rs, i * 2, 0, 0));
    else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, i * 4, 0, 0));
}

// the weight an entry enters with: (scale - 1) * act on a selected row, -act without a scale table
__device__ __forceinline__ float at_weight(float val, int ix, int H, bool selected, const float* __restrict__ scale) {
    if (!selected || (unsigned)ix >= (unsigned)H) return 0.f;
    const float act = fmaxf(val, 0.f);
    return scale ? (scale[ix] - 1.f) * act : -act;
}

// one step of the transposing butterfly: N entries before it, N / 2 after it.  A lane whose bit M is clear keeps the
// lower half of its entries and hands the upper half to lane ^ M, the other way round where the bit is set.
template <int M, int N, int GRP>
__device__ __forceinline__ void at_fold(float (&p)[GRP], int lane) {
    const bool hi = (lane & M) != 0;
#pragma unroll
    for (int e = 0; e < N / 2; ++e) {
        const float keep = hi ? p[e + N / 2] : p[e];
        const float send = hi ? p[e] : p[e + N / 2];
        p[e] = keep + __uint_as_float(lane_xor_u32<M>(__float_as_uint(send), lane));
    }
}

template <int M>
__device__ __forceinline__ float at_add_xor(float t, int lane) {
    return t + __uint_as_float(lane_xor_u32<M>(__float_as_uint(t), lane));
}

// the whole butterfly over a group of GRP (2, 4, 8 or 16) entries: halving steps at lane distance 1 .. GRP / 2, plain
// steps at GRP .. 32.  Lane l returns the sum of entry at_bitrev<GRP>(l & (GRP - 1)).
template <int GRP>
__device__ __forceinline__ float at_butterfly(float (&p)[GRP], int lane) {
    at_fold<1, GRP, GRP>(p, lane);
    if constexpr (GRP >= 4) at_fold<2, GRP / 2, GRP>(p, lane);
    if constexpr (GRP >= 8) at_fold<4, GRP / 4, GRP>(p, lane);
    if constexpr (GRP >= 16) at_fold<8, GRP / 8, GRP>(p, lane);
    float t = p[0];
    if constexpr (GRP <= 2) t = at_add_xor<2>(t, lane);
    if constexpr (GRP <= 4) t = at_add_xor<4>(t, lane);
    if constexpr (GRP <= 8) t = at_add_xor<8>(t, lane);
    t = at_add_xor<16>(t, lane);
    return at_add_xor<32>(t, lane);
}

// x < GRP with its log2(GRP) bits reversed
template <int GRP>
__device__ __forceinline__ int at_bitrev(int x) {
    int y = 0;
#pragma unroll
    for (int b = 1, t = GRP >> 1; b < GRP; b <<= 1, t >>= 1)
        if (x & b) y |= t;
    return y;
}

template <int HDT, int GDT, typename WT, int VPL, int GRP>
__global__ void __launch_bounds__(256) attribute_kernel(
    const WT* __restrict__ WdT, const void* __restrict__ h, const void* __restrict__ grad, int64_t n_rows, int dim, int H,
    int K, const float* __restrict__ vals, const int32_t* __restrict__ idx, const float* __restrict__ gamma, float eps,
    const float* __restrict__ scale, const uint8_t* __restrict__ row_mask, float* __restrict__ attr,
    uint32_t* __restrict__ amax_bits) {
    __shared__ float wave_amax[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float amax = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_rows; r += (int64_t)gridDim.x * 4) {
        const bool selected = !row_mask || row_mask[r] != 0;
        // (the column guards d < dim below do not change from row to row; left to itself the compiler computes all VPL of
        // them once, before this loop, and keeps VPL exec masks in scalar registers for the whole kernel - more than there
        // are at VPL 16 and 32.  An opaque copy of dim per row makes them values of the row that die after its loads.)
        int dim_r = dim;
        if constexpr (VPL > 8) asm volatile("" : "+s"(dim_r));
        float w[2];
        int ix[2];
        bool valid[2];
        unsigned long long m[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = lane + 64 * s;
            valid[s] = j < K;
            ix[s] = valid[s] ? idx[r * K + j] : -1;
            w[s] = valid[s] ? at_weight(vals[r * K + j], ix[s], H, selected, scale) : 0.f;
            m[s] = __ballot(w[s] != 0.f);
        }
        float out[2] = {0.f, 0.f};
        if ((m[0] | m[1]) != 0ull) {
            // u_d = G_d / gamma_d and sigma of the row
            float u[VPL];
            float sigma = 1.f;
            if constexpr (VPL <= 8) {
                if (gamma) {
                    const float sum = ln_row_load<HDT, VPL>(h, r, dim_r, lane, u);
                    float mean, var_eps;
                    ln_row_stats<VPL>(u, sum, dim_r, lane, eps, mean, var_eps);
                    sigma = __fsqrt_rn(var_eps);
                }
#pragma unroll
                for (int i = 0; i < VPL; ++i) {
                    const int d = lane + 64 * i;
                    u[i] = 0.f;
                    if (d < dim_r) {
                        const float g = load_act<GDT>(grad, r * dim_r + d);
                        u[i] = gamma ? __fdiv_rn(g, gamma[d]) : g;
                    }
                }
            } else {
                // wide rows: the rows of h and G through range-checked descriptors as well (what ln_row_load does, with the
                // hardware returning the zeros beyond the row: the same values summed in the same order)
                if (gamma) {
                    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
                        (char*)h + r * dim_r * at_bytes<HDT>(), 0, dim_r * at_bytes<HDT>(), 0x00020000);
                    float sum = 0.f;
#pragma unroll
                    for (int i = 0; i < VPL; ++i) {
                        u[i] = at_load_act<HDT>(rh, lane + 64 * i);
                        sum += u[i];
                    }
                    float mean, var_eps;
                    ln_row_stats<VPL>(u, sum, dim_r, lane, eps, mean, var_eps);
                    sigma = __fsqrt_rn(var_eps);
                }
                const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
                    (char*)grad + r * dim_r * at_bytes<GDT>(), 0, dim_r * at_bytes<GDT>(), 0x00020000);
                const __amdgpu_buffer_rsrc_t rgam =
                    __builtin_amdgcn_make_buffer_rsrc((void*)gamma, 0, gamma ? dim_r * 4 : 0, 0x00020000);
#pragma unroll
                for (int i = 0; i < VPL; ++i) {
                    const int d = lane + 64 * i;
                    const float g = at_load_act<GDT>(rg, d);
                    u[i] = g;
                    if (gamma) {
                        const float q = __fdiv_rn(g, at_load_act<WSAE_DT_F32>(rgam, d));
                        u[i] = d < dim_r ? q : 0.f;  // (0 / 0 beyond the row)
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                unsigned long long bits = m[s];
                // place of the lane's own entry among the slot's non-zero ones; the bit reversal of it within its group is the
                // lane that ends the butterfly with the entry's sum
                const int rank = __popcll(m[s] & ((1ull << lane) - 1ull));
                const int src = at_bitrev<GRP>(rank & (GRP - 1));
                float s_mine = 0.f;
                for (int group = 0; bits; ++group) {
                    float p[GRP];
#pragma unroll
                    for (int g = 0; g < GRP; ++g) {
                        p[g] = 0.f;
                        if (bits) {  // wave-uniform
                            const int j = __ffsll((long long)bits) - 1;
                            bits &= bits - 1;
                            const int ij = __builtin_amdgcn_readlane(ix[s], j);
                            const WT* row = WdT + (int64_t)ij * dim;
                            if constexpr (VPL <= 8) {
#pragma unroll
                                for (int i = 0; i < VPL; ++i) {
                                    const int d = lane + 64 * i;
                                    if (d < dim) p[g] = fmaf(u[i], at_load_w(row, d), p[g]);
                                }
                            } else {
                                // wide rows: a per-lane guard per column slot keeps VPL exec masks alive in scalar registers
                                // (and spills them).  A buffer descriptor over exactly this decoder row lets the hardware
                                // range check do it: columns beyond the row read as 0, and u is 0 there as well
                                const __amdgpu_buffer_rsrc_t rs =
                                    __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, dim * (int)sizeof(WT), 0x00020000);
#pragma unroll
                                for (int i = 0; i < VPL; ++i)
                                    p[g] = fmaf(u[i], at_load_row<WT>(rs, (lane + 64 * i) * (int)sizeof(WT)), p[g]);
                            }
                        }
                    }
                    const float t = at_butterfly<GRP>(p, lane);
                    const float got = __shfl(t, src);
                    if (rank / GRP == group) s_mine = got;
                }
                if (w[s] != 0.f) out[s] = (sigma * w[s]) * s_mine;
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = lane + 64 * s;
            if (j < K) attr[r * K + j] = out[s];
            const float a = fabsf(out[s]);
            amax = a <= AT_FLT_MAX ? fmaxf(amax, a) : __uint_as_float(0x7f800000u);  // Inf or NaN: the call's maximum is Inf
        }
    }
    if (!amax_bits) return;
    amax = wave_max(amax);
    if (lane == 0) wave_amax[wave] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a = fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3]));
        if (a > 0.f) atomicMax(amax_bits, __float_as_uint(a));
    }
}

// binary exponent e of A > 0 with A < 2^e (A = f 2^e, 0.5 <= f < 1)
__device__ __forceinline__ int at_exponent(float a) {
    int e;
    (void)frexpf(a, &e);
    return e;
}

__global__ void __launch_bounds__(256) attr_sum_kernel(
    const float* __restrict__ attr, const float* __restrict__ vals, const int32_t* __restrict__ idx, int64_t n_entries, int H,
    int K, const float* __restrict__ scale, const uint8_t* __restrict__ row_mask, const uint32_t* __restrict__ amax_bits,
    unsigned long long* __restrict__ acc_sum, unsigned long long* __restrict__ acc_abs, int32_t* __restrict__ acc_rows) {
    const float a_max = __uint_as_float(*amax_bits);
    // attr / q = attr * 2^(36 - e): exact in double, |.| < 2^36
    // (a non-finite attr somewhere in the call: no sums, attr_finish_kernel writes NaN)
    const double inv_q = a_max > 0.f && a_max <= AT_FLT_MAX ? ldexp(1.0, AT_FRAC_BITS - at_exponent(a_max)) : 0.0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_entries; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / K;
        const int f = idx[t];
        const bool selected = !row_mask || row_mask[r] != 0;
        if (at_weight(vals[t], f, H, selected, scale) == 0.f) continue;
        atomicAdd(acc_rows + f, 1);
        if (inv_q == 0.0) continue;
        const long long qv = (long long)rint((double)attr[t] * inv_q);
        if (qv == 0) continue;
        atomicAdd(acc_sum + f, (unsigned long long)qv);
        atomicAdd(acc_abs + f, (unsigned long long)(qv < 0 ? -qv : qv));
    }
}

__global__ void __launch_bounds__(256) attr_finish_kernel(
    int H, const uint32_t* __restrict__ amax_bits, const long long* __restrict__ acc_sum, const long long* __restrict__ acc_abs,
    const int32_t* __restrict__ acc_rows, float* __restrict__ feat_sum, float* __restrict__ feat_abs,
    int32_t* __restrict__ feat_rows) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= H) return;
    const float a_max = __uint_as_float(*amax_bits);
    const bool finite = a_max <= AT_FLT_MAX;
    const int shift = a_max > 0.f && finite ? at_exponent(a_max) - AT_FRAC_BITS : 0;
    const float nan = __uint_as_float(0x7fc00000u);
    // one rounding: int64 -> fp32 to nearest, then a power of two
    if (feat_sum) feat_sum[f] = finite ? ldexpf(__ll2float_rn(acc_sum[f]), shift) : nan;
    if (feat_abs) feat_abs[f] = finite ? ldexpf(__ll2float_rn(acc_abs[f]), shift) : nan;
    if (feat_rows) feat_rows[f] = acc_rows[f];
}

extern "C" int64_t wsae_attribute_workspace_bytes(int32_t hidden_dim) {
    if (hidden_dim <= 0) return 0;
    return AT_HEAD_BYTES + (int64_t)hidden_dim * (2 * sizeof(long long) + sizeof(int32_t));
}

extern "C" int wsae_attribute(wsae_ctx* ctx, const float* params, const void* h, int32_t h_dtype, const void* grad_h,
                              int32_t grad_dtype, int64_t n_rows, const float* vals, const int32_t* idx, const float* gamma,
                              float eps, const float* scale, const uint8_t* row_mask, float* attr, float* feat_sum,
                              float* feat_abs, int32_t* feat_rows, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(ctx && params && h && grad_h && vals && idx && attr && n_rows >= 0, "wsae_attribute: bad argument");
    WSAE_REQUIRE(h_dtype == WSAE_DT_F32 || h_dtype == WSAE_DT_BF16, "wsae_attribute: unknown input dtype %d", h_dtype);
    WSAE_REQUIRE(grad_dtype == WSAE_DT_F32 || grad_dtype == WSAE_DT_BF16, "wsae_attribute: unknown gradient dtype %d", grad_dtype);
    WSAE_REQUIRE(ctx->D <= 2048 && ctx->K <= 128, "wsae_attribute: input_dim %d / k %d outside the kernel's range", ctx->D, ctx->K);
    WSAE_REQUIRE(n_rows * ctx->K <= AT_MAX_ENTRIES, "wsae_attribute: %lld rows of %d entries (at most 2^26 entries per call)",
                 (long long)n_rows, ctx->K);
    const bool per_feature = feat_sum || feat_abs || feat_rows;
    WSAE_REQUIRE(!per_feature || (workspace && workspace_bytes >= wsae_attribute_workspace_bytes(ctx->H)),
                 "wsae_attribute: workspace of %lld bytes (needs %lld)", (long long)(workspace ? workspace_bytes : 0),
                 (long long)wsae_attribute_workspace_bytes(ctx->H));
    WSAE_REQUIRE(!per_feature || ((uintptr_t)workspace & 7) == 0, "wsae_attribute: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int H = ctx->H, K = ctx->K;
    uint32_t* amax_bits = nullptr;
    long long *acc_sum = nullptr, *acc_abs = nullptr;
    int32_t* acc_rows = nullptr;
    if (per_feature) {
        WSAE_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)wsae_attribute_workspace_bytes(H), st));
        amax_bits = (uint32_t*)workspace;
        acc_sum = (long long*)((char*)workspace + AT_HEAD_BYTES);
        acc_abs = acc_sum + H;
        acc_rows = (int32_t*)(acc_abs + H);
    }
    if (n_rows > 0) {
        const unsigned nb = (unsigned)min(ceil_div64(n_rows, 4), (int64_t)8 * ctx->cus);
#define AT_LAUNCH(HD, GD, WT, W, V, G)                                                                                  \
    attribute_kernel<HD, GD, WT, V, G><<<nb, 256, 0, st>>>(W, h, grad_h, n_rows, ctx->D, H, K, vals, idx, gamma, eps, scale, \
                                                        row_mask, attr, amax_bits)
#define AT_WIDTH(HD, GD, WT, W)                                \
    do {                                                       \
        if (ctx->D <= 512) AT_LAUNCH(HD, GD, WT, W, 8, 16);        \
        else if (ctx->D <= 1024) AT_LAUNCH(HD, GD, WT, W, 16, 8); \
        else AT_LAUNCH(HD, GD, WT, W, 32, 4);                     \
    } while (0)
#define AT_DTYPES(WT, W)                                                                                    \
    do {                                                                                                    \
        if (h_dtype == WSAE_DT_F32 && grad_dtype == WSAE_DT_F32) AT_WIDTH(WSAE_DT_F32, WSAE_DT_F32, WT, W);  \
        else if (h_dtype == WSAE_DT_F32) AT_WIDTH(WSAE_DT_F32, WSAE_DT_BF16, WT, W);                        \
        else if (grad_dtype == WSAE_DT_F32) AT_WIDTH(WSAE_DT_BF16, WSAE_DT_F32, WT, W);                     \
        else AT_WIDTH(WSAE_DT_BF16, WSAE_DT_BF16, WT, W);                                                   \
    } while (0)
        // the decoder rows the ctx's decode reads: the bf16 shadow in BF16 mode, the pack's fp32 rows in FP32 mode
        if (ctx->prec == WSAE_PREC_BF16) AT_DTYPES(bf16_t, (const bf16_t*)ctx->WdT_bf16);
        else AT_DTYPES(float, params + ctx->off[1]);
#undef AT_DTYPES
#undef AT_WIDTH
#undef AT_LAUNCH
        WSAE_LAUNCH_CHECK();
    }
    if (!per_feature) return WSAE_OK;
    if (n_rows > 0) {
        const int64_t n_entries = n_rows * K;
        const unsigned nb = (unsigned)min(ceil_div64(n_entries, 256), (int64_t)16 * ctx->cus);
        attr_sum_kernel<<<nb, 256, 0, st>>>(attr, vals, idx, n_entries, H, K, scale, row_mask, amax_bits,
                                            (unsigned long long*)acc_sum, (unsigned long long*)acc_abs, acc_rows);
        WSAE_LAUNCH_CHECK();
    }
    attr_finish_kernel<<<ceil_div(H, 256), 256, 0, st>>>(H, amax_bits, acc_sum, acc_abs, acc_rows, feat_sum, feat_abs, feat_rows);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
