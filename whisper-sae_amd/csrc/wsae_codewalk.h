// What the analysis kernels that walk a compact (values, indices) code share.  Device side: the LDS
// pointer types, the per-segment row bounds of a call, the entry-per-thread walk (CodeArgs, pf_first_active) and the
// wave-per-row front end (probe_row_columns, probe_load_row).  Host side: the predicates behind the *_workspace_bytes
// queries (code_args_ok for a code with a feature window, column_code_ok for one with a column map) and the CW_REQUIRE_*
// checks of the entry points: k, rows, window, hidden, the column code, a single lag, the entry lists of a transposed plan,
// the size of the workspace and its alignment.  Included by wsae_groupstats.hip (pooling), wsae_runs.hip, wsae_labels.hip
// (the entry-per-thread walk), wsae_regress.hip, wsae_cluster.hip (the wave-per-row front end, the column code),
// wsae_dyn_canon.h (the same front end, for wsae_dynamics.hip and wsae_abx.hip), for the checks alone wsae_coact.hip,
// wsae_pairs.hip and wsae_align.hip, and through wsae_lists.h - the plumbing of the analyses that build per-key lists -
// by wsae_sta.hip, wsae_probe.hip, wsae_profile.hip and wsae_feature_topk.hip.  (align256, min64 and the wave helpers
// live in wsae_common.h: wsae_match.hip needs them and walks no code.)
#pragma once
#include <limits.h>

#include "wsae_common.h"

namespace {

// LDS is accessed through volatile pointers: the cells are read by other lanes than wrote them, and one wave's LDS
// instructions execute in order.  (The pointers name the LDS address space themselves: address-space inference leaves
// volatile accesses alone, and they would be flat.)
typedef __attribute__((address_space(3))) volatile float lds_f32;
typedef __attribute__((address_space(3))) volatile int lds_i32;
typedef __attribute__((address_space(3))) volatile uint8_t lds_u8;
typedef __attribute__((address_space(3))) volatile unsigned long long lds_u64;
typedef __attribute__((address_space(3))) volatile double lds_f64;

__global__ __launch_bounds__(256) void seg_reset_kernel(int32_t* __restrict__ first, int32_t* __restrict__ last, int n_seg) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_seg) {
        first[s] = INT_MAX;
        last[s] = -1;
    }
}

// first / last row of every segment of this call; a run of equal ids costs two atomics, whatever its length
__global__ __launch_bounds__(256) void seg_bounds_kernel(const int32_t* __restrict__ seg, int n_rows, int n_seg,
                                                         int32_t* __restrict__ first, int32_t* __restrict__ last) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int s = seg[r];
    if (s < 0 || s >= n_seg) return;
    if (r == 0 || seg[r - 1] != s) atomicMin(first + s, (int)r);
    if (r == n_rows - 1 || seg[r + 1] != s) atomicMax(last + s, (int)r);
}

// first[s] > last[s] afterwards: segment s has no row in this call
inline void seg_bounds(const int32_t* seg, int64_t n_rows, int n_seg, int32_t* first, int32_t* last, hipStream_t st) {
    seg_reset_kernel<<<ceil_div(n_seg, 256), 256, 0, st>>>(first, last, n_seg);
    seg_bounds_kernel<<<(int)ceil_div64(n_rows, 256), 256, 0, st>>>(seg, (int)n_rows, n_seg, first, last);
}

// ---- the entry-per-thread walk of wsae_profile.hip and wsae_labels.hip --------------------------------------------------
struct CodeArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;  // nullable
    int64_t n;           // n_rows * k
    int k, f_lo, f_cols;
};

// One block pass over the entries base .. base + 255 of the flat code (thread = entry); called by all threads of the
// block together.  true: the thread's entry is the first active entry of its (row, feature) on a non-padding row and the
// feature lies in the window (which lies in [0, hidden): the host checked).  v, f, r: its value, feature and row;
// row_head: the entry is column 0 of a non-padding row.
__device__ __forceinline__ bool pf_first_active(const CodeArgs& a, int64_t base, int* s_idx, float& v, int& f, int64_t& r,
                                                bool& row_head) {
    const int t = threadIdx.x;
    const int64_t e = base + t;
    const int64_t r0 = base / a.k;  // (block-uniform)
    const int j0 = (int)(base - r0 * a.k) + t;
    r = r0 + j0 / a.k;
    const int j = j0 % a.k;
    v = 0.f;
    f = -1;
    bool live = false;
    if (e < a.n) {
        v = a.vals[e];
        f = a.idx[e];
        live = a.seg == nullptr || a.seg[r] >= 0;
    }
    row_head = live && j == 0;
    const bool pos = v > 0.f;  // (NaN is not)
    __syncthreads();           // the previous pass has been read
    s_idx[t] = pos ? f : -1;
    __syncthreads();
    bool act = live && pos && f >= a.f_lo && f - a.f_lo < a.f_cols;
    if (act) {
        for (int d = 1; d <= j; ++d) {  // the row's earlier entries: entries e - 1 .. e - j
            const int prev = t - d >= 0 ? s_idx[t - d] : (a.vals[e - d] > 0.f ? a.idx[e - d] : -1);
            if (prev == f) {
                act = false;
                break;
            }
        }
    }
    return act;
}

// ---- the wave-per-row front end of wsae_probe.hip and wsae_regress.hip: one lane per entry, two for k > 64 ----------------
// The entries lane and lane + 64 of one row.  col0 / col1: the probe column where the entry is the first active entry of
// its feature on the row and the feature has a column, else -1.  Called by the whole wave; the row is not padding.
__device__ __forceinline__ void probe_row_columns(float v0, int f0, float v1, int f1, int k, int hidden,
                                                  const int32_t* __restrict__ col_of, int lane, int& col0, int& col1) {
    const int p0 = v0 > 0.f ? f0 : -1;  // (NaN is not; an absent entry carries v = 0)
    const int p1 = v1 > 0.f ? f1 : -1;
    bool dup0 = false, dup1 = false;
    const int k0 = k < 64 ? k : 64;
    for (int d = 0; d < k0; ++d) {  // (wave-uniform)
        const int g = __builtin_amdgcn_readlane(p0, d);
        dup0 |= d < lane && g == p0;
        dup1 |= g == p1;
    }
    for (int d = 64; d < k; ++d) {
        const int g = __builtin_amdgcn_readlane(p1, d - 64);
        dup1 |= d - 64 < lane && g == p1;
    }
    col0 = -1;
    col1 = -1;
    if (p0 >= 0 && p0 < hidden && !dup0) col0 = col_of ? col_of[p0] : p0;
    if (p1 >= 0 && p1 < hidden && !dup1) col1 = col_of ? col_of[p1] : p1;
}

__device__ __forceinline__ void probe_load_row(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k, int64_t r,
                                               int lane, float& v0, int& f0, float& v1, int& f1) {
    v0 = 0.f, v1 = 0.f, f0 = -1, f1 = -1;
    if (lane < k) {
        v0 = vals[r * k + lane];
        f0 = idx[r * k + lane];
    }
    if (lane + 64 < k) {
        v1 = vals[r * k + lane + 64];
        f1 = idx[r * k + lane + 64];
    }
}

// ---- host side: the checks every entry point makes on a code and its feature window ------------------------------------
inline bool code_args_ok(int64_t n_rows, int k, int max_k, int hidden, int64_t f_lo, int64_t f_cols) {
    return n_rows >= 0 && n_rows <= INT_MAX && k >= 1 && k <= max_k && hidden >= 1 && f_lo >= 0 && f_cols >= 1 &&
           f_lo + f_cols <= hidden;
}

// the same for a code read through a column map (col_of, or the identity) of P columns
inline bool column_code_ok(int64_t n_rows, int k, int hidden, int64_t P) {
    return n_rows >= 0 && n_rows <= INT_MAX && k >= 1 && k <= WSAE_PROBE_MAX_K && hidden >= 1 && P >= 1 && P <= hidden;
}

inline bool lag_ok(int lag) { return lag >= -1024 && lag <= 1024; }

// FN: the entry point's name, a string literal.  One macro per requirement, not one per entry point: every entry point
// has checks of its own between them, and the order of the checks decides which message a caller with two mistakes gets.
#define CW_REQUIRE_K(FN, k, max_k) WSAE_REQUIRE((k) >= 1 && (k) <= (max_k), FN ": need 1 <= k <= %d (got %d)", max_k, k)
#define CW_REQUIRE_ROWS(FN, n_rows)                                                                                       \
    WSAE_REQUIRE((n_rows) >= 0 && (n_rows) <= INT_MAX, FN ": need 0 <= n_rows <= 2^31 - 1 (got %lld)", (long long)(n_rows))
#define CW_REQUIRE_WINDOW(FN, f_lo, f_cols, hidden)                                                                       \
    WSAE_REQUIRE((f_lo) >= 0 && (f_cols) >= 1 && (int64_t)(f_lo) + (f_cols) <= (hidden),                                  \
                 FN ": the window [%d, %d + %d) is outside [0, %d)", f_lo, f_lo, f_cols, hidden)
#define CW_REQUIRE_HIDDEN(FN, hidden) WSAE_REQUIRE((hidden) >= 1, FN ": hidden must be positive (got %d)", hidden)
#define CW_REQUIRE_COLUMN_CODE(FN, k, hidden, n_rows, col_of, n_cols)                                                     \
    CW_REQUIRE_K(FN, k, WSAE_PROBE_MAX_K);                                                                                \
    CW_REQUIRE_HIDDEN(FN, hidden);                                                                                        \
    CW_REQUIRE_ROWS(FN, n_rows);                                                                                          \
    WSAE_REQUIRE((n_cols) >= 1 && (n_cols) <= (hidden), FN ": need 1 <= n_cols <= hidden = %d (got %d)", hidden, n_cols); \
    WSAE_REQUIRE((col_of) || (n_cols) == (hidden), FN ": without col_of the columns are the %d features (got n_cols %d)", \
                 hidden, n_cols)
#define CW_REQUIRE_LAG(FN, lag) WSAE_REQUIRE(lag_ok(lag), FN ": need -1024 <= lag <= 1024 (got %d)", lag)
// the entry lists of a transposed plan (wsae_probe_plan): cap entries of t_row and t_val
#define CW_REQUIRE_LISTS(FN, cap, t_row, t_val)                                                                           \
    WSAE_REQUIRE((cap) >= 0 && (((t_row) && (t_val)) || (cap) == 0), FN ": cap %lld entries need t_row and t_val",        \
                 (long long)(cap))
// (the workspace's size and alignment: WSAE_REQUIRE_WORKSPACE and WSAE_REQUIRE_WORKSPACE_ALIGNED, wsae_common.h)

}  // namespace
