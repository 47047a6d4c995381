// Code clustering: the two halves of a Lloyd iteration of k-means over the compact code, without
// the dense [frames, H] matrix, without a [frames, n_clusters] product and without float atomics.
//
// wsae_cluster_assign: one wave per row, lanes as clusters (CT tiles of 64 per lane), the front end and the entry loop of
// wsae_probe_forward.  A score is ONE chain: bias (or 0), then per entry an fp32 multiply and an fp32 add (not fused:
// contraction is off in this file), in ascending entry position.  The squared norm of the row is one fp64 chain over the
// same entries, which every lane carries (the values reach the lanes by v_readlane, so the chain is wave-uniform).  The
// winner, the runner-up and their scores come from the fixed butterfly over per-lane partials taken in ascending tile and
// from a read of the owning lane, so what is written for a row depends on that row alone.  The state is integer: a
// workgroup keeps counts, quantised scores, the totals and (where n_clusters x n_classes cells fit) the contingency table
// in LDS and adds every touched cell to the caller's state once, with a global integer atomic, when it ends.  A table too
// large for LDS takes one global integer atomic per labelled row.
//
// wsae_cluster_accumulate: S_q[p][assign[r]] += the quantised value of every entry (r, value) of column p of the
// transposed plan.  Integer sums do not depend on order, so the entry lists are cut into pieces of CL_CHUNK consecutive
// entries regardless of the columns: a workgroup owns a piece, finds the column of its first entry by bisection of col_ptr
// and walks the stretches of the piece that belong to one column each.  Per stretch the lanes add into an LDS table of
// n_clusters int64 cells keyed by the gathered assign, and the non-zero cells go to S_q with one global integer atomic
// each.  A feature that fires on every frame is cut into as many pieces as any other stretch of that length.
#include "wsae_codewalk.h"

// every fp32 multiply and add below rounds on its own, as the numpy mirror of the tests does
#pragma clang fp contract(off)

namespace {

constexpr int CL_BLOCK = 256;          // four waves, a row each
constexpr int CL_MAX_BLOCKS = 2048;    // more rows than CL_MAX_BLOCKS * 4: the grid-stride loop
constexpr int CL_FB = 8;               // entries of a row whose centroid rows are loaded before the first of them is added
constexpr int CL_LDS_CELLS = 8192;     // contingency cells a workgroup keeps in LDS (int32: a workgroup sees < 2^31 rows)
constexpr int CL_CHUNK = 4096;         // entries of the plan per accumulate job
constexpr int CL_ACC_MAX_BLOCKS = 1 << 20;
constexpr float CL_Q_SCALE = 1048576.f;  // 2^20
constexpr float CL_Q_CLIP = 4096.f;

struct AssignArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;
    const int32_t* col_of;
    const float* Ct;
    const float* bias;
    const int32_t* labels;
    int64_t n_rows, ldc;
    int k, hidden, C, n_classes, normalize, cont_in_lds;
    int32_t* assign;
    float* best;
    float* second;
    float* inv_norm;
    unsigned long long* count;
    unsigned long long* best_q;
    unsigned long long* contingency;
    unsigned long long* totals;
};

// the entries of `mask` (bits of the lanes whose col is a column), CL_FB at a time, in ascending position
template <int CT>
__device__ __forceinline__ void cl_add_entries(unsigned long long mask, float v, int col, const AssignArgs& a, int lane,
                                               float (&score)[CT], double& norm) {
    const int vb = __float_as_int(v);
    while (mask) {
        float ev[CL_FB];
        int ec[CL_FB];
#pragma unroll
        for (int u = 0; u < CL_FB; ++u) {
            ev[u] = 0.f;
            ec[u] = -1;
            if (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                ev[u] = __int_as_float(__builtin_amdgcn_readlane(vb, j));
                ec[u] = __builtin_amdgcn_readlane(col, j);
            }
        }
        float w[CL_FB][CT];
#pragma unroll
        for (int u = 0; u < CL_FB; ++u)
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int c = t * 64 + lane;
                w[u][t] = (ec[u] >= 0 && c < a.C) ? a.Ct[(int64_t)ec[u] * a.ldc + c] : 0.f;
            }
#pragma unroll
        for (int u = 0; u < CL_FB; ++u) {
            if (ec[u] < 0) continue;  // (wave-uniform)
            norm = norm + (double)ev[u] * (double)ev[u];  // (the square is exact in fp64)
#pragma unroll
            for (int t = 0; t < CT; ++t) score[t] = score[t] + ev[u] * w[u][t];  // (two roundings: contraction is off)
        }
    }
}

// the lowest cluster != skip at the maximum of the scores over the clusters != skip, and its score; -1 and -inf when
// there is none (all wave-uniform)
template <int CT>
__device__ __forceinline__ void cl_arg_max(const float (&score)[CT], int C, int skip, int lane, int& arg, float& top) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int c = t * 64 + lane;
        if (c < C && c != skip) mx = fmaxf(mx, score[t]);
    }
    mx = wave_max(mx);
    int am = INT_MAX;
#pragma unroll
    for (int t = CT - 1; t >= 0; --t) {
        const int c = t * 64 + lane;
        if (c < C && c != skip && score[t] == mx) am = c;
    }
    am = __builtin_amdgcn_readfirstlane(wave_min_i(am));
    arg = -1;
    top = -INFINITY;
    if (am == INT_MAX) return;  // (no cluster but skip; wave-uniform)
    float mine = 0.f;
#pragma unroll
    for (int t = 0; t < CT; ++t)
        if (t == (am >> 6)) mine = score[t];
    arg = am;
    top = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), am & 63));  // (the bits of the owner, -0 included)
}

// dynamic LDS: best_q uint64 [C], count uint32 [C], totals uint32 [4], contingency uint32 [C n_classes] where it fits
template <int CT>
__global__ __launch_bounds__(CL_BLOCK) void cluster_assign_kernel(AssignArgs a) {
    extern __shared__ unsigned long long cl_smem[];
    unsigned long long* s_bq = cl_smem;
    unsigned int* s_cnt = (unsigned int*)(s_bq + a.C);
    unsigned int* s_tot = s_cnt + a.C;
    unsigned int* s_cont = s_tot + 4;
    const int n_cells = a.cont_in_lds ? a.C * a.n_classes : 0;
    for (int c = threadIdx.x; c < a.C; c += CL_BLOCK) {
        s_bq[c] = 0ull;
        s_cnt[c] = 0u;
    }
    if (threadIdx.x < 4) s_tot[threadIdx.x] = 0u;
    for (int c = threadIdx.x; c < n_cells; c += CL_BLOCK) s_cont[c] = 0u;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (CL_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (CL_BLOCK / 64);
    // the segment, the label and the entries of a wave's next row are requested before it works on the current one
    float nv0 = 0.f, nv1 = 0.f;
    int nf0 = -1, nf1 = -1, nsg = -1, ny = -1;
    auto request = [&](int64_t r) {
        nsg = a.seg ? a.seg[r] : 0;
        ny = a.labels ? a.labels[r] : -1;
        probe_load_row(a.vals, a.idx, a.k, r, lane, nv0, nf0, nv1, nf1);
    };
    if (wave < a.n_rows) request(wave);
    for (int64_t r = wave; r < a.n_rows; r += n_waves) {
        const int sg = __builtin_amdgcn_readfirstlane(nsg);
        const int y = __builtin_amdgcn_readfirstlane(ny);
        const float v0 = nv0, v1 = nv1;
        const int f0 = nf0, f1 = nf1;
        if (r + n_waves < a.n_rows) request(r + n_waves);
        int col0 = -1, col1 = -1;
        if (sg >= 0) probe_row_columns(v0, f0, v1, f1, a.k, a.hidden, a.col_of, lane, col0, col1);
        const unsigned long long m0 = __ballot(col0 >= 0), m1 = __ballot(col1 >= 0);
        if ((m0 | m1) == 0ull) {  // padding, or no entry with a column: -1 and exact zeros
            if (lane == 0) {
                if (a.assign) a.assign[r] = -1;
                if (a.best) a.best[r] = 0.f;
                if (a.second) a.second[r] = 0.f;
                if (a.inv_norm) a.inv_norm[r] = 0.f;
                if (sg >= 0) atomicAdd(s_tot + 1, 1u);
            }
            continue;
        }
        float score[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) score[t] = (a.bias && t * 64 + lane < a.C) ? a.bias[t * 64 + lane] : 0.f;
        double norm = 0.0;
        cl_add_entries<CT>(m0, v0, col0, a, lane, score, norm);
        if (a.k > 64) cl_add_entries<CT>(m1, v1, col1, a, lane, score, norm);
        int am, a2;
        float top, sec;
        cl_arg_max<CT>(score, a.C, -1, lane, am, top);
        if (am < 0) continue;  // (NaN scores alone: finite Ct and bias are the caller's duty; nothing is written)
        cl_arg_max<CT>(score, a.C, am, lane, a2, sec);
        const float inv = (float)(1.0 / sqrt(norm));
        const float b = a.normalize ? top * inv : top;
        if (lane == 0) {
            if (a.assign) a.assign[r] = am;
            if (a.best) a.best[r] = top;
            if (a.second) a.second[r] = sec;
            if (a.inv_norm) a.inv_norm[r] = inv;
            const long long q = llrintf(fminf(fmaxf(b, -CL_Q_CLIP), CL_Q_CLIP) * CL_Q_SCALE);
            atomicAdd(s_cnt + am, 1u);
            atomicAdd(s_bq + am, (unsigned long long)q);
            atomicAdd(s_tot + 0, 1u);
            if (y >= 0 && y < a.n_classes) {
                atomicAdd(s_tot + 2, 1u);
                if (a.contingency) {
                    if (a.cont_in_lds) atomicAdd(s_cont + am * a.n_classes + y, 1u);
                    else atomicAdd(a.contingency + (int64_t)am * a.n_classes + y, 1ull);
                }
            }
        }
    }
    __syncthreads();
    // one global integer atomic per touched cell
    for (int c = threadIdx.x; c < a.C; c += CL_BLOCK) {
        const unsigned int n = s_cnt[c];
        if (n == 0u) continue;
        if (a.count) atomicAdd(a.count + c, (unsigned long long)n);
        if (a.best_q && s_bq[c]) atomicAdd(a.best_q + c, s_bq[c]);
    }
    if (a.totals && threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(a.totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
    if (a.contingency)
        for (int c = threadIdx.x; c < n_cells; c += CL_BLOCK)
            if (s_cont[c]) atomicAdd(a.contingency + c, (unsigned long long)s_cont[c]);
}

int64_t assign_lds_bytes(int C, int cells_in_lds) { return 8 * (int64_t)C + 4 * (int64_t)C + 16 + 4 * (int64_t)cells_in_lds; }

// ---- the centroid sums ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CL_BLOCK) void cluster_accumulate_kernel(const int64_t* __restrict__ col_ptr,
                                                                      const int32_t* __restrict__ t_row,
                                                                      const float* __restrict__ t_val, int64_t cap, int P,
                                                                      const int32_t* __restrict__ assign,
                                                                      const float* __restrict__ row_weight, int64_t n_rows, int C,
                                                                      unsigned long long* __restrict__ S_q, int64_t lds) {
    __shared__ unsigned long long tab[WSAE_CLUSTER_MAX];
    for (int c = threadIdx.x; c < C; c += CL_BLOCK) tab[c] = 0ull;
    __syncthreads();
    const int64_t total = min64(col_ptr[P], cap);  // the entries the lists hold
    const int64_t n_jobs = (total + CL_CHUNK - 1) / CL_CHUNK;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int64_t end = min64((job + 1) * CL_CHUNK, total);
        int64_t cur = job * CL_CHUNK;
        while (cur < end) {  // (block-uniform: every value below comes from col_ptr)
            int lo = 0, hi = P;  // the column of entry cur: the last p with col_ptr[p] <= cur
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (col_ptr[mid] <= cur) lo = mid; else hi = mid;
            }
            const int p = lo;
            int64_t stop = min64(col_ptr[p + 1], end);
            if (stop <= cur) stop = end;  // (col_ptr is not ascending: the caller's error; the walk still ends)
            for (int64_t i = cur + threadIdx.x; i < stop; i += CL_BLOCK) {
                const int r = t_row[i];
                float x = t_val[i];
                if (r < 0 || r >= n_rows) continue;
                const int c = assign[r];
                if (c < 0 || c >= C) continue;
                if (row_weight) x = x * row_weight[r];
                if (!(x > 0.f)) continue;  // (NaN is not)
                atomicAdd(tab + c, (unsigned long long)llrintf(fminf(x, CL_Q_CLIP) * CL_Q_SCALE));
            }
            __syncthreads();
            for (int c = threadIdx.x; c < C; c += CL_BLOCK) {
                const unsigned long long s = tab[c];
                if (s) {
                    atomicAdd(S_q + (int64_t)p * lds + c, s);
                    tab[c] = 0ull;
                }
            }
            __syncthreads();
            cur = stop;
        }
    }
}

#define CL_REQUIRE_CLUSTERS(FN, C)                                                                                        \
    WSAE_REQUIRE((C) >= 1 && (C) <= WSAE_CLUSTER_MAX, FN ": need 1 <= n_clusters <= %d (got %d)", WSAE_CLUSTER_MAX, C)

}  // namespace

extern "C" int64_t wsae_cluster_assign_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols,
                                                       int32_t n_clusters) {
    const bool ok = column_code_ok(n_rows, k, hidden, n_cols) && k <= WSAE_CLUSTER_MAX_K && n_clusters >= 1 &&
                    n_clusters <= WSAE_CLUSTER_MAX;
    return ok ? 0 : -1;
}

extern "C" int wsae_cluster_assign(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                   int64_t n_rows, const int32_t* col_of, int32_t n_cols, const float* Ct, int64_t ldc,
                                   const float* bias, int32_t n_clusters, int32_t normalize, const int32_t* labels,
                                   int32_t n_classes, int32_t* assign, float* best, float* second, float* inv_norm,
                                   int64_t* count, int64_t* best_q, int64_t* contingency, int64_t* totals, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && Ct, "wsae_cluster_assign: null pointer");
    CW_REQUIRE_K("wsae_cluster_assign", k, WSAE_CLUSTER_MAX_K);
    CW_REQUIRE_COLUMN_CODE("wsae_cluster_assign", k, hidden, n_rows, col_of, n_cols);
    CL_REQUIRE_CLUSTERS("wsae_cluster_assign", n_clusters);
    WSAE_REQUIRE(ldc >= n_clusters, "wsae_cluster_assign: ldc %lld is smaller than the %d clusters", (long long)ldc, n_clusters);
    WSAE_REQUIRE(!normalize || !bias, "wsae_cluster_assign: normalize needs bias == NULL (cosine scores carry no bias)");
    WSAE_REQUIRE(!labels || (n_classes >= 1 && n_classes <= WSAE_CLUSTER_MAX),
                 "wsae_cluster_assign: labels need 1 <= n_classes <= %d (got %d)", WSAE_CLUSTER_MAX, n_classes);
    WSAE_REQUIRE(!contingency || labels, "wsae_cluster_assign: a contingency table needs labels");
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_cluster_assign: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    (void)workspace;  // (wsae_cluster_assign_workspace_bytes is 0: one launch that keeps nothing)
    if (n_rows == 0) return WSAE_OK;
    const int classes = labels ? n_classes : 0;
    const int in_lds = contingency && (int64_t)n_clusters * classes <= CL_LDS_CELLS;
    AssignArgs a = {vals, idx, seg, col_of, Ct, bias, labels, n_rows, ldc, k, hidden, n_clusters, classes, normalize != 0, in_lds,
                    assign, best, second, inv_norm, (unsigned long long*)count, (unsigned long long*)best_q,
                    (unsigned long long*)contingency, (unsigned long long*)totals};
    const int64_t blocks = ceil_div64(n_rows, CL_BLOCK / 64);
    const int grid = (int)(blocks < CL_MAX_BLOCKS ? blocks : CL_MAX_BLOCKS);
    const size_t smem = (size_t)assign_lds_bytes(n_clusters, in_lds ? n_clusters * classes : 0);
    hipStream_t st = (hipStream_t)stream;
    if (n_clusters <= 64) cluster_assign_kernel<1><<<grid, CL_BLOCK, smem, st>>>(a);
    else if (n_clusters <= 128) cluster_assign_kernel<2><<<grid, CL_BLOCK, smem, st>>>(a);
    else if (n_clusters <= 256) cluster_assign_kernel<4><<<grid, CL_BLOCK, smem, st>>>(a);
    else if (n_clusters <= 512) cluster_assign_kernel<8><<<grid, CL_BLOCK, smem, st>>>(a);
    else cluster_assign_kernel<16><<<grid, CL_BLOCK, smem, st>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_cluster_accumulate_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_clusters, int64_t cap) {
    return n_rows >= 0 && n_rows <= INT_MAX && n_cols >= 1 && n_clusters >= 1 && n_clusters <= WSAE_CLUSTER_MAX && cap >= 0 ? 0 : -1;
}

extern "C" int wsae_cluster_accumulate(const int64_t* col_ptr, const int32_t* t_row, const float* t_val, int64_t cap,
                                       int32_t n_cols, const int32_t* assign, const float* row_weight, int64_t n_rows,
                                       int32_t n_clusters, int64_t* S_q, int64_t lds, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
    WSAE_REQUIRE(col_ptr && assign && S_q, "wsae_cluster_accumulate: null pointer");
    CW_REQUIRE_ROWS("wsae_cluster_accumulate", n_rows);
    WSAE_REQUIRE(n_cols >= 1, "wsae_cluster_accumulate: n_cols must be positive (got %d)", n_cols);
    CL_REQUIRE_CLUSTERS("wsae_cluster_accumulate", n_clusters);
    CW_REQUIRE_LISTS("wsae_cluster_accumulate", cap, t_row, t_val);
    WSAE_REQUIRE(lds >= n_clusters, "wsae_cluster_accumulate: lds %lld is smaller than the %d clusters", (long long)lds,
                 n_clusters);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_cluster_accumulate: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    (void)workspace;  // (wsae_cluster_accumulate_workspace_bytes is 0: one launch that keeps nothing)
    if (n_rows == 0 || cap == 0) return WSAE_OK;
    const int64_t jobs = ceil_div64(cap, CL_CHUNK);
    const int grid = (int)(jobs < CL_ACC_MAX_BLOCKS ? jobs : CL_ACC_MAX_BLOCKS);
    cluster_accumulate_kernel<<<grid, CL_BLOCK, 0, (hipStream_t)stream>>>(col_ptr, t_row, t_val, cap, n_cols, assign, row_weight,
                                                                           n_rows, n_clusters, (unsigned long long*)S_q, lds);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
