// Label association: which feature detects which class of a per-frame label (phoneme, word
// position, speaker, language token), at which activation threshold and how many frames early or late?
//
// wsae_label_update: per feature of the window, lag, class and value stratum the number of frames on which the feature
// was active in that stratum while the frame `lag` rows further on carried that class (cnt), and per lag and class the
// number of such frame pairs whatever the features did (pair_rows).  One pass, one thread per entry of the flat code, the
// walk of wsae_profile.hip (pf_first_active); every field is an integer sum updated with integer atomics, so the state
// does not depend on the launch geometry, the order of the calls or the grouping of whole utterances into calls.
//
// cnt takes one global atomic per (first-active entry in the window, lag).  pair_rows would take one per (row, lag) on a
// few dozen addresses - labels are piecewise constant - so where its L n_classes cells fit LB_LDS_CELLS a block sums them
// in LDS and adds what is not zero to the state once, at its end (the way profile_kernel<true> treats fires).  The k
// threads of a row read the same seg and labels words for every lag; they are not staged in LDS: a wave reads at most
// ceil(64 / k) + 1 distinct words per lag, which the vector cache serves as broadcasts.  The form that combines equal
// cells of neighbouring rows in an LDS table before the global atomics did not ship: profiles/experiments/README.md.
#include "wsae_codewalk.h"

namespace {

constexpr int LB_BLOCK = 256;
constexpr int LB_MAX_BLOCKS = 2048;  // eight blocks per CU; more entries than LB_MAX_BLOCKS * LB_BLOCK: the grid-stride loop
constexpr int LB_LDS_CELLS = 4096;   // the largest pair_rows table (L * n_classes cells, 16 KB) a block sums in LDS

struct LabelArgs {
    const int32_t* labels;  // [n_rows]
    const float* edges;     // [f_cols, S - 1], nullable when S == 1
    int64_t n_rows;
    int C, S, lag_lo, L;
    int32_t* cnt;                   // [f_cols, L, C, S]
    unsigned long long* pair_rows;  // [L, C]
};

// The class of the pair (r, lag index l), or -1 where it is no pair.  seg_r: seg[r] (unused without seg); the caller has
// checked that row r is not padding.
__device__ __forceinline__ int lb_pair_class(const CodeArgs& a, const LabelArgs& g, int64_t r, int seg_r, int l) {
    const int64_t q = r + g.lag_lo + l;
    if (q < 0 || q >= g.n_rows) return -1;
    if (a.seg != nullptr && a.seg[q] != seg_r) return -1;
    const int c = g.labels[q];
    return c >= 0 && c < g.C ? c : -1;
}

// LDS_PAIRS: the block keeps pair_rows in LDS (L * C <= LB_LDS_CELLS counters; a cell takes at most one count per row,
// so 32 bits hold a call's 2^31 - 1 rows) and adds it to the state once, at its end.
template <bool LDS_PAIRS>
__global__ __launch_bounds__(LB_BLOCK) void label_kernel(CodeArgs a, LabelArgs g) {
    __shared__ int s_idx[LB_BLOCK];
    extern __shared__ unsigned int lb_pairs[];  // (LDS_PAIRS) [L, C]
    const int cells = g.L * g.C;
    if (LDS_PAIRS) {
        for (int i = threadIdx.x; i < cells; i += LB_BLOCK) lb_pairs[i] = 0u;
        // (the first barrier of pf_first_active orders this before the first add)
    }
    for (int64_t base = (int64_t)blockIdx.x * LB_BLOCK; base < a.n; base += (int64_t)gridDim.x * LB_BLOCK) {
        float v;
        int f;
        int64_t r;
        bool head;
        const bool act = pf_first_active(a, base, s_idx, v, f, r, head);
        if (!head && !act) continue;
        const int seg_r = a.seg != nullptr ? a.seg[r] : 0;
        int32_t* mine = nullptr;  // (act) the feature's cells of the value's stratum, at lag 0 and class 0
        if (act) {
            const int col = f - a.f_lo;
            int stratum = 0;  // the number of the feature's edges that are <= v (a NaN edge never is)
            const float* ed = g.edges + (int64_t)col * (g.S - 1);
            for (int t = 0; t < g.S - 1; ++t) stratum += ed[t] <= v;
            mine = g.cnt + (int64_t)col * g.L * g.C * g.S + stratum;
        }
        for (int l = 0; l < g.L; ++l) {  // the pair test once per lag, for the row's pair count and the feature's cell
            const int c = lb_pair_class(a, g, r, seg_r, l);
            if (c < 0) continue;
            if (head) {  // column 0 of a non-padding row counts the row's pairs
                if (LDS_PAIRS) {
                    atomicAdd(lb_pairs + l * g.C + c, 1u);
                } else {
                    atomicAdd(g.pair_rows + l * g.C + c, 1ull);
                }
            }
            if (act) atomicAdd(mine + ((int64_t)l * g.C + c) * g.S, 1);
        }
    }
    if (LDS_PAIRS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += LB_BLOCK) {
            const unsigned int n = lb_pairs[i];
            if (n) atomicAdd(g.pair_rows + i, (unsigned long long)n);
        }
    }
}

inline bool label_args_ok(int64_t n_rows, int k, int hidden, int64_t f_lo, int64_t f_cols, int C, int64_t lag_lo,
                          int64_t lag_hi, int S) {
    return code_args_ok(n_rows, k, WSAE_LABEL_MAX_K, hidden, f_lo, f_cols) && C >= 1 && C <= WSAE_LABEL_MAX_CLASSES &&
           lag_lo >= -1024 && lag_lo <= lag_hi && lag_hi <= 1024 && lag_hi - lag_lo + 1 <= WSAE_LABEL_MAX_LAGS && S >= 1 &&
           S <= WSAE_LABEL_MAX_STRATA;
}

}  // namespace

extern "C" int64_t wsae_label_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols,
                                              int32_t n_classes, int32_t lag_lo, int32_t lag_hi, int32_t n_strata) {
    return label_args_ok(n_rows, k, hidden, f_lo, f_cols, n_classes, lag_lo, lag_hi, n_strata) ? 0 : -1;
}

extern "C" int wsae_label_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                 const int32_t* labels, int64_t n_rows, int32_t n_classes, int32_t lag_lo, int32_t lag_hi,
                                 int32_t f_lo, int32_t f_cols, const float* edges, int32_t n_strata, int32_t* cnt,
                                 int64_t* pair_rows, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && labels && cnt && pair_rows, "wsae_label_update: null pointer");
    CW_REQUIRE_K("wsae_label_update", k, WSAE_LABEL_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_label_update", hidden);
    CW_REQUIRE_ROWS("wsae_label_update", n_rows);
    CW_REQUIRE_WINDOW("wsae_label_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(n_classes >= 1 && n_classes <= WSAE_LABEL_MAX_CLASSES, "wsae_label_update: need 1 <= n_classes <= %d (got %d)",
                 WSAE_LABEL_MAX_CLASSES, n_classes);
    WSAE_REQUIRE(lag_lo >= -1024 && lag_lo <= lag_hi && lag_hi <= 1024 &&
                     (int64_t)lag_hi - lag_lo + 1 <= WSAE_LABEL_MAX_LAGS,
                 "wsae_label_update: need -1024 <= lag_lo <= lag_hi <= 1024 and at most %d lags (got %d .. %d)",
                 WSAE_LABEL_MAX_LAGS, lag_lo, lag_hi);
    WSAE_REQUIRE(n_strata >= 1 && n_strata <= WSAE_LABEL_MAX_STRATA, "wsae_label_update: need 1 <= n_strata <= %d (got %d)",
                 WSAE_LABEL_MAX_STRATA, n_strata);
    WSAE_REQUIRE(edges || n_strata == 1, "wsae_label_update: %d strata need edges (null pointer)", n_strata);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_label_update: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    (void)workspace;  // (wsae_label_workspace_bytes is 0: one launch that keeps nothing)
    if (n_rows == 0) return WSAE_OK;
    const int L = lag_hi - lag_lo + 1;
    CodeArgs a = {vals, idx, seg, n_rows * k, k, f_lo, f_cols};
    LabelArgs g = {labels, edges, n_rows, n_classes, n_strata, lag_lo, L, cnt, (unsigned long long*)pair_rows};
    const int64_t blocks = ceil_div64(a.n, LB_BLOCK);
    const int grid = (int)(blocks < LB_MAX_BLOCKS ? blocks : LB_MAX_BLOCKS);
    if (L * n_classes <= LB_LDS_CELLS) {
        label_kernel<true><<<grid, LB_BLOCK, sizeof(unsigned int) * L * n_classes, (hipStream_t)stream>>>(a, g);
    } else {
        label_kernel<false><<<grid, LB_BLOCK, 0, (hipStream_t)stream>>>(a, g);
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
