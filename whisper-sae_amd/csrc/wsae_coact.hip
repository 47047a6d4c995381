// Co-activation statistics: over a stream of rows of two compact codes, how often feature i of
// code A and feature j of code B fire on the same row, and per feature of A its strongest partners under a normalised
// score.  All state is integer, so every result is independent of launch geometry, row order and call split.
//
//   update  one wave per row (grid-stride): the row's active entries of A (those inside the window) and of B are
//           compacted into the wave's LDS lists by ballot; the na * nb pairs are then dealt to the lanes, consecutive
//           lanes walking B under one A entry, and each pair is one no-return integer atomic on its table cell.  The
//           marginals take one atomic per active entry, the row total one 64-bit atomic per workgroup.
//   top     one workgroup per table row: the threads sweep the row's columns (16 bytes per lane where the table's
//           alignment allows), score the candidates in fp64 from the integers, keep a sorted list each in registers
//           (wsae_toplist.h, the list of wsae_match.hip) and fold the 256 lists pairwise through LDS.
#include <limits.h>
#include <math.h>

#include "wsae_codewalk.h"
#include "wsae_toplist.h"

namespace {

constexpr int CO_MAX_BLOCKS = 2048;  // update: grid-stride beyond 8192 rows in flight (8 workgroups per CU on 256 CUs)

// the row's active entries -> list[0 .. returned count): idx - lo for the entries with lo <= idx < lo + span; every
// active entry (0 <= idx < hidden, v > 0), inside the window or not, bumps fire[idx] when fire is given
__device__ __forceinline__ int co_compact(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k, int hidden,
                                          int lo, int span, int32_t* __restrict__ fire, int* list, int lane) {
    int n = 0;
    for (int e0 = 0; e0 < k; e0 += 64) {
        const int e = e0 + lane;
        bool act = false;
        int i = 0;
        if (e < k) {
            i = idx[e];
            act = vals[e] > 0.f && i >= 0 && i < hidden;
        }
        if (act && fire) atomicAdd(fire + i, 1);
        const bool in = act && i >= lo && i - lo < span;
        const unsigned long long bal = __ballot(in);
        if (in) list[n + __popcll(bal & ((1ull << lane) - 1ull))] = i - lo;
        n += __popcll(bal);
    }
    return n;
}

__global__ __launch_bounds__(256) void coact_update_kernel(const float* __restrict__ va, const int32_t* __restrict__ ia, int ka,
                                                           int ha, const float* __restrict__ vb, const int32_t* __restrict__ ib,
                                                           int kb, int hb, int64_t n_rows, const uint8_t* __restrict__ row_mask,
                                                           int a_lo, int a_rows, int32_t* __restrict__ counts, int64_t ldc,
                                                           int32_t* __restrict__ fire_a, int32_t* __restrict__ fire_b,
                                                           unsigned long long* __restrict__ total_rows) {
    __shared__ int la[4][WSAE_COACT_MAX_K], lb[4][WSAE_COACT_MAX_K];
    __shared__ int done[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int mine = 0;  // contributing rows of this wave
    for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < n_rows; row += (int64_t)gridDim.x * 4) {
        if (row_mask && row_mask[row] == 0) continue;  // (wave-uniform)
        ++mine;
        const int na = co_compact(va + row * ka, ia + row * ka, ka, ha, a_lo, a_rows, fire_a, la[w], lane);
        const int nb = co_compact(vb + row * kb, ib + row * kb, kb, hb, 0, hb, fire_b, lb[w], lane);
        __builtin_amdgcn_wave_barrier();  // the lists are read by other lanes than wrote them (one wave: LDS keeps its order)
        const int np = na * nb;
        for (int p = lane; p < np; p += 64) {
            const int a = p / nb, b = p - a * nb;
            atomicAdd(counts + (int64_t)la[w][a] * ldc + lb[w][b], 1);
        }
        __builtin_amdgcn_wave_barrier();  // ... and rewritten by the next row
    }
    if (lane == 0) done[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int all = done[0] + done[1] + done[2] + done[3];
        if (all) atomicAdd(total_rows, (unsigned long long)all);
    }
}

// fp64 from the integers, rounded once to fp32.  n = fire_a[i], m = fire_b[j], N = total rows, c = counts[i][j];
// phi_a = sqrt(double(n (N - n))) of the row, 0 where the product is 0.
__device__ __forceinline__ float co_score(int metric, int64_t c, int64_t n, int64_t m, int64_t N, double phi_a) {
    double s = 0.0;
    if (metric == WSAE_COACT_COUNT) {
        s = (double)c;
    } else if (metric == WSAE_COACT_COND) {
        if (n != 0) s = (double)c / (double)n;
    } else if (metric == WSAE_COACT_JACCARD) {
        const int64_t d = n + m - c;
        if (d != 0) s = (double)c / (double)d;
    } else {
        const int64_t pb = m * (N - m);
        if (phi_a != 0.0 && pb != 0) s = (double)(N * c - n * m) / (phi_a * sqrt((double)pb));
    }
    return (float)s;
}

// block = one table row; VEC = 4: counts 16-byte aligned and ldc a multiple of 4
template <int NB, int VEC>
__global__ __launch_bounds__(256) void coact_top_kernel(const int32_t* __restrict__ counts, int64_t ldc, int a_lo, int hidden_b,
                                                        const int32_t* __restrict__ fire_a, const int32_t* __restrict__ fire_b,
                                                        const int64_t* __restrict__ total_rows, int metric, int min_count,
                                                        int exclude_self, int top_n, float* __restrict__ out_val,
                                                        int32_t* __restrict__ out_idx, int32_t* __restrict__ out_cnt) {
    __shared__ float sv[NB * 256];
    __shared__ int si[NB * 256];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int i = a_lo + (int)r;
    const int32_t* row = counts + r * ldc;
    const int64_t n = fire_a[i], N = *total_rows;
    const bool need_m = metric == WSAE_COACT_JACCARD || metric == WSAE_COACT_PHI;
    double phi_a = 0.0;
    if (metric == WSAE_COACT_PHI) {
        const int64_t pa = n * (N - n);
        if (pa != 0) phi_a = sqrt((double)pa);
    }
    float lv[NB];
    int li[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        lv[p] = -INFINITY;
        li[p] = MT_EMPTY;
    }
    const int nchunk = (hidden_b + VEC - 1) / VEC;
    for (int ch = tid; ch < nchunk; ch += 256) {
        const int c0 = ch * VEC;
        int cv[VEC];
        bool whole = false;
        if constexpr (VEC == 4) {
            whole = c0 + 4 <= hidden_b;
            if (whole) {
                const int4 q = *(const int4*)(row + c0);
                cv[0] = q.x; cv[1] = q.y; cv[2] = q.z; cv[3] = q.w;
            }
        }
        if (!whole) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) cv[e] = c0 + e < hidden_b ? row[c0 + e] : -1;  // (-1 is below every min_count)
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int j = c0 + e, c = cv[e];
            if (c < min_count || (exclude_self && j == i)) continue;
            const float s = co_score(metric, c, n, need_m ? fire_b[j] : 0, N, phi_a);
            if (s >= lv[NB - 1]) mt_insert<NB>(lv, li, s, j);
        }
    }
    // 256 lists -> one, pairwise: thread t takes the list of thread t + s
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < 2 * s) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                sv[p * 256 + tid] = lv[p];
                si[p * 256 + tid] = li[p];
            }
        }
        __syncthreads();  // (a round reads slots >= s and the next one writes slots < s: one barrier per round)
        bool go = tid < s;  // the partner's list is sorted: the first element that does not enter ends it
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            if (go) {
                const int ix = si[p * 256 + tid + s];
                const float v = sv[p * 256 + tid + s];
                go = ix != MT_EMPTY && (v > lv[NB - 1] || (v == lv[NB - 1] && ix < li[NB - 1]));
                if (go) mt_insert<NB>(lv, li, v, ix);
            }
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int p = 0; p < NB; ++p)
            if (p < top_n) {
                const bool used = li[p] != MT_EMPTY;
                out_val[r * top_n + p] = lv[p];
                out_idx[r * top_n + p] = used ? li[p] : -1;
                if (out_cnt) out_cnt[r * top_n + p] = used ? row[li[p]] : 0;
            }
    }
}

bool co_update_args_ok(int64_t n_rows, int k_a, int hidden_a, int k_b, int hidden_b, int64_t a_lo, int64_t a_rows) {
    return code_args_ok(n_rows, k_a, WSAE_COACT_MAX_K, hidden_a, a_lo, a_rows) &&
           code_args_ok(n_rows, k_b, WSAE_COACT_MAX_K, hidden_b, 0, hidden_b);  // (all of B's features)
}

bool co_top_args_ok(int64_t a_lo, int64_t a_rows, int hidden_b, int top_n) {
    return a_lo >= 0 && a_rows >= 1 && a_lo + a_rows <= INT_MAX && hidden_b >= 1 && hidden_b <= INT_MAX - 1024 && top_n >= 1 && top_n <= WSAE_MATCH_MAX_N;
}

}  // namespace

extern "C" int64_t wsae_coact_workspace_bytes(int64_t n_rows, int32_t k_a, int32_t hidden_a, int32_t k_b, int32_t hidden_b,
                                              int32_t a_lo, int32_t a_rows) {
    return co_update_args_ok(n_rows, k_a, hidden_a, k_b, hidden_b, a_lo, a_rows) ? 0 : -1;  // the atomics need no scratch
}

extern "C" int wsae_coact_update(const float* vals_a, const int32_t* idx_a, int32_t k_a, int32_t hidden_a, const float* vals_b,
                                 const int32_t* idx_b, int32_t k_b, int32_t hidden_b, int64_t n_rows, const uint8_t* row_mask,
                                 int32_t a_lo, int32_t a_rows, int32_t* counts, int64_t ldc, int32_t* fire_a, int32_t* fire_b,
                                 int64_t* total_rows, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)workspace;
    WSAE_REQUIRE(vals_a && idx_a && vals_b && idx_b && counts && fire_a && total_rows, "wsae_coact_update: null pointer");
    WSAE_REQUIRE(k_a >= 1 && k_a <= WSAE_COACT_MAX_K && k_b >= 1 && k_b <= WSAE_COACT_MAX_K,
                 "wsae_coact_update: need 1 <= k_a, k_b <= %d (got %d, %d)", WSAE_COACT_MAX_K, k_a, k_b);
    WSAE_REQUIRE(hidden_a >= 1 && hidden_b >= 1, "wsae_coact_update: hidden_a, hidden_b must be positive (got %d, %d)", hidden_a,
                 hidden_b);
    CW_REQUIRE_ROWS("wsae_coact_update", n_rows);
    CW_REQUIRE_WINDOW("wsae_coact_update", a_lo, a_rows, hidden_a);
    WSAE_REQUIRE(ldc >= hidden_b, "wsae_coact_update: ldc %lld < hidden_b %d", (long long)ldc, hidden_b);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_coact_update: workspace too small (%lld < 0)", (long long)workspace_bytes);
    if (n_rows == 0) return WSAE_OK;
    const int64_t want = ceil_div64(n_rows, 4);
    const int grid = (int)(want < CO_MAX_BLOCKS ? want : CO_MAX_BLOCKS);
    coact_update_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(vals_a, idx_a, k_a, hidden_a, vals_b, idx_b, k_b, hidden_b, n_rows,
                                                               row_mask, a_lo, a_rows, counts, ldc, fire_a, fire_b,
                                                               (unsigned long long*)total_rows);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_coact_top_workspace_bytes(int32_t a_lo, int32_t a_rows, int32_t hidden_b, int32_t top_n) {
    return co_top_args_ok(a_lo, a_rows, hidden_b, top_n) ? 0 : -1;  // one workgroup owns a row: nothing to hand over
}

extern "C" int wsae_coact_top(const int32_t* counts, int64_t ldc, int32_t a_lo, int32_t a_rows, int32_t hidden_b,
                              const int32_t* fire_a, const int32_t* fire_b, const int64_t* total_rows, int32_t metric,
                              int32_t min_count, int32_t exclude_self, int32_t top_n, float* out_val, int32_t* out_idx,
                              int32_t* out_cnt, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)workspace;
    WSAE_REQUIRE(counts && fire_a && total_rows && out_val && out_idx, "wsae_coact_top: null pointer");
    WSAE_REQUIRE(metric == WSAE_COACT_COUNT || metric == WSAE_COACT_COND || metric == WSAE_COACT_JACCARD ||
                     metric == WSAE_COACT_PHI,
                 "wsae_coact_top: unknown metric %d", metric);
    WSAE_REQUIRE(fire_b || metric == WSAE_COACT_COUNT || metric == WSAE_COACT_COND,
                 "wsae_coact_top: the jaccard and phi metrics need fire_b");
    WSAE_REQUIRE(top_n >= 1 && top_n <= WSAE_MATCH_MAX_N, "wsae_coact_top: need 1 <= top_n <= %d (got %d)", WSAE_MATCH_MAX_N,
                 top_n);
    WSAE_REQUIRE(hidden_b >= 1 && hidden_b <= INT_MAX - 1024, "wsae_coact_top: need 1 <= hidden_b <= 2^31 - 1025 (got %d)", hidden_b);
    WSAE_REQUIRE(a_lo >= 0 && a_rows >= 1 && (int64_t)a_lo + a_rows <= INT_MAX,
                 "wsae_coact_top: the window [%d, %d + %d) is not a range of features", a_lo, a_lo, a_rows);
    WSAE_REQUIRE(ldc >= hidden_b, "wsae_coact_top: ldc %lld < hidden_b %d", (long long)ldc, hidden_b);
    WSAE_REQUIRE(min_count >= 0, "wsae_coact_top: min_count must not be negative (got %d)", min_count);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_coact_top: workspace too small (%lld < 0)", (long long)workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (uintptr_t)counts % 16 == 0 && ldc % 4 == 0;
#define CO_LAUNCH(NB_, VEC_)                                                                                               \
    coact_top_kernel<NB_, VEC_><<<a_rows, 256, 0, st>>>(counts, ldc, a_lo, hidden_b, fire_a, fire_b, total_rows, metric,       \
                                                         min_count, exclude_self, top_n, out_val, out_idx, out_cnt)
    if (top_n <= 4) {
        if (vec) CO_LAUNCH(4, 4); else CO_LAUNCH(4, 1);
    } else if (top_n <= 8) {
        if (vec) CO_LAUNCH(8, 4); else CO_LAUNCH(8, 1);
    } else {
        if (vec) CO_LAUNCH(16, 4); else CO_LAUNCH(16, 1);
    }
#undef CO_LAUNCH
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
