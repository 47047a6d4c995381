// Activation profiles: what does the distribution of a feature's activations look like, and what
// does the feature do when it is not at its maximum?
//
// wsae_profile_update: per feature of the window a histogram of its active values over 192 bins read off the float's
// bits (eight per octave over [2^-12, 2^12)), the count, the minimum and maximum as bit patterns, the count of values
// >= 4096 and a 64-bit fixed-point sum.  One pass, one thread per entry of the flat code; every field is an integer
// sum, minimum or maximum updated with integer atomics, so the state does not depend on the launch geometry, the order
// of the calls or the batching.  The minimum and maximum are looked at with a plain load first: they settle after a few
// rows, a stale value only costs an atomic that changes nothing, and two of the five atomics per entry go away.  Where
// the window is at most 4096 features and at least half of `hidden`, a block keeps fires and sum_q of the window in LDS and
// adds them to the state once, which leaves one global atomic per entry (profiles/activation_profile_note.md has the A/B).
//
// wsae_sample_update: per (feature, value stratum) the m activations with the smallest keys ever offered, the key
// being a hash of (ordinal, feature, seed) above the ordinal: a bottom-m sketch, i.e. a uniform sample without
// replacement that does not depend on call order or batching and merges exactly.  The four launches of
// wsae_feature_topk.hip - count, scan (count_scan_kernel and the workspace head of wsae_lists.h, shared with that file),
// scatter by list, one wave per list merging - with a pre-filter in the first pass:
// an entry whose key is not below the last key of its list as the list stands when the call begins can never enter
// (lists only tighten), so its `seen` is counted and it goes no further.
//
// Both walk the code the same way (pf_first_active in wsae_codewalk.h, shared with wsae_labels.hip): an index repeated
// within a row counts once, with the value of its first active entry, which needs the row's earlier entries only - they
// are the thread's left neighbours in the block's LDS, or, for a row that began in the previous 256 entries, a few
// global loads.
#include <limits.h>

#include "wsae_lists.h"

namespace {

constexpr int PF_BLOCK = 256;
constexpr int PF_MAX_BLOCKS = 8192;
constexpr int PF_BINS = WSAE_PROFILE_BINS;
constexpr int PF_LDS_COLS = 4096;   // the widest window whose fires and sum_q a block keeps in LDS (48 KB)
constexpr int PF_LDS_BLOCKS = 768;  // ... three such blocks per CU; a block ends with at most 2 f_cols global atomics
constexpr unsigned long long SM_EMPTY = ~0ull;  // an unused slot of a list: no key reaches it (ordinals stay below 2^31)

// ---- the value histogram and moments ------------------------------------------------------------------------------------
struct ProfileOut {
    int32_t* fires;
    int32_t* hist;
    int32_t* max_bits;
    int32_t* min_bits;
    int32_t* over;
    unsigned long long* sum_q;
    unsigned long long* total_rows;
};

// LDS_SUMS: the block keeps fires and sum_q of the whole window in LDS (12 bytes per feature, f_cols <= PF_LDS_COLS) and
// adds them to the state once, at its end: two of the three global atomics per entry become LDS atomics.
template <bool LDS_SUMS>
__global__ __launch_bounds__(PF_BLOCK) void profile_kernel(CodeArgs a, ProfileOut o) {
    __shared__ int s_idx[PF_BLOCK];
    extern __shared__ unsigned long long pf_sums[];  // (LDS_SUMS) sum_q [f_cols], then fires [f_cols]
    int* l_fires = (int*)(pf_sums + a.f_cols);
    if (LDS_SUMS) {
        for (int c = threadIdx.x; c < a.f_cols; c += PF_BLOCK) {
            pf_sums[c] = 0ull;
            l_fires[c] = 0;
        }
        // (the first barrier of pf_first_active orders this before the first add)
    }
    unsigned long long rows_here = 0;
    for (int64_t base = (int64_t)blockIdx.x * PF_BLOCK; base < a.n; base += (int64_t)gridDim.x * PF_BLOCK) {
        float v;
        int f;
        int64_t r;
        bool head;
        const bool act = pf_first_active(a, base, s_idx, v, f, r, head);
        rows_here += head;
        if (!act) continue;
        const int c = f - a.f_lo;
        const int b = __float_as_int(v);
        int bin = (b >> 20) - 920;
        bin = bin < 0 ? 0 : (bin > PF_BINS - 1 ? PF_BINS - 1 : bin);
        atomicAdd(o.hist + (int64_t)c * PF_BINS + bin, 1);
        // rint(min(v, 4096) * 2^20): the product is exact in fp32, the conversion rounds to nearest even
        const unsigned long long q = (unsigned long long)__float2ll_rn(fminf(v, 4096.f) * 1048576.f);
        if (LDS_SUMS) {
            atomicAdd(l_fires + c, 1);
            atomicAdd(pf_sums + c, q);
        } else {
            atomicAdd(o.fires + c, 1);
            atomicAdd(o.sum_q + c, q);
        }
        if (b > o.max_bits[c]) atomicMax(o.max_bits + c, b);
        if (b < o.min_bits[c]) atomicMin(o.min_bits + c, b);
        if (v >= 4096.f) atomicAdd(o.over + c, 1);
    }
    if (LDS_SUMS) {
        __syncthreads();
        for (int c = threadIdx.x; c < a.f_cols; c += PF_BLOCK) {
            const int n = l_fires[c];
            if (n) {
                atomicAdd(o.fires + c, n);
                atomicAdd(o.sum_q + c, pf_sums[c]);
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) rows_here += __shfl_xor(rows_here, s, 64);
    if ((threadIdx.x & 63) == 0 && rows_here) atomicAdd(o.total_rows, rows_here);
}

// ---- the bottom-m sample per (feature, stratum) ----------------------------------------------------------------------------
struct SampleArgs {
    const float* edges;  // [f_cols, S - 1], nullable when S == 1
    int S, m;
    uint32_t seed;
    int64_t ord_base;
    const unsigned long long* keys;  // [f_cols, S, m] as the lists stand when the call begins
    int32_t* seen;                   // [f_cols, S]
};

__device__ __forceinline__ unsigned long long sm_key(uint32_t ordinal, uint32_t f, uint32_t seed) {
    uint32_t x = ordinal * 0x9E3779B1u ^ f * 0x85EBCA77u ^ seed;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return ((unsigned long long)x << 32) | ordinal;
}

// SCATTER false: counts `seen` and, per list, the entries that pass the pre-filter (slot = cnt); true: the same entries
// take their places behind the list's offset (slot = cursor).  Both passes read the lists as the call found them.
template <bool SCATTER>
__global__ __launch_bounds__(PF_BLOCK) void sample_pass_kernel(CodeArgs a, SampleArgs sa, int32_t* __restrict__ slot,
                                                               unsigned long long* __restrict__ ent_key,
                                                               float* __restrict__ ent_val) {
    __shared__ int s_idx[PF_BLOCK];
    for (int64_t base = (int64_t)blockIdx.x * PF_BLOCK; base < a.n; base += (int64_t)gridDim.x * PF_BLOCK) {
        float v;
        int f;
        int64_t r;
        bool head;
        if (!pf_first_active(a, base, s_idx, v, f, r, head)) continue;
        const int c = f - a.f_lo;
        int stratum = 0;  // the number of the feature's edges that are <= v
        const float* ed = sa.edges + (int64_t)c * (sa.S - 1);
        for (int t = 0; t < sa.S - 1; ++t) stratum += ed[t] <= v;
        const int64_t list = (int64_t)c * sa.S + stratum;
        const unsigned long long key = sm_key((uint32_t)(sa.ord_base + r), (uint32_t)f, sa.seed);
        if (!SCATTER) atomicAdd(sa.seen + list, 1);
        if (key < sa.keys[list * sa.m + sa.m - 1]) {
            const int p = atomicAdd(slot + list, 1);
            if (SCATTER) {
                ent_key[p] = key;
                ent_val[p] = v;
            }
        }
    }
}

// one wave per list; lane l holds list element l (m <= 64), ascending by key; lanes from m on hold SM_EMPTY
__global__ __launch_bounds__(PF_BLOCK) void sample_merge_kernel(const int32_t* __restrict__ offs,
                                                                const unsigned long long* __restrict__ ent_key,
                                                                const float* __restrict__ ent_val, int n_lists, int m,
                                                                unsigned long long* __restrict__ keys, float* __restrict__ svals) {
    const int lane = threadIdx.x & 63;
    const int list = blockIdx.x * (PF_BLOCK / 64) + (threadIdx.x >> 6);
    if (list >= n_lists) return;
    const int beg = offs[list], end = offs[list + 1];
    if (beg == end) return;
    unsigned long long lk = SM_EMPTY;
    float lv = 0.f;
    if (lane < m) {
        lk = keys[(int64_t)list * m + lane];
        lv = svals[(int64_t)list * m + lane];
    }
    for (int s = beg; s < end; s += 64) {
        unsigned long long ck = SM_EMPTY;
        float cv = 0.f;
        if (s + lane < end) {
            ck = ent_key[s + lane];
            cv = ent_val[s + lane];
        }
        const unsigned long long last = __shfl(lk, m - 1, 64);
        unsigned long long todo = __ballot(ck < last);  // (the list may have tightened since the pre-filter)
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned long long key = __shfl(ck, j, 64);
            const float val = __shfl(cv, j, 64);
            const int p = __popcll(__ballot(lk < key));  // the list elements that stay ahead: lanes 0 .. p - 1
            if (p >= m) continue;
            const unsigned long long uk = __shfl_up(lk, 1, 64);
            const float uv = __shfl_up(lv, 1, 64);
            if (lane > p) {
                lk = uk;
                lv = uv;
            } else if (lane == p) {
                lk = key;
                lv = val;
            }
            if (lane >= m) {
                lk = SM_EMPTY;
                lv = 0.f;
            }
        }
    }
    if (lane < m) {
        keys[(int64_t)list * m + lane] = lk;
        svals[(int64_t)list * m + lane] = lv;
    }
}

inline bool sample_args_ok(int64_t n_rows, int k, int hidden, int64_t f_lo, int64_t f_cols, int S, int m) {
    return code_args_ok(n_rows, k, WSAE_PROFILE_MAX_K, hidden, f_lo, f_cols) && n_rows * k <= INT_MAX && S >= 1 &&
           S <= WSAE_SAMPLE_MAX_STRATA && m >= 1 && m <= WSAE_SAMPLE_MAX_KEEP && f_cols * S < INT_MAX;
}

inline int pf_grid(int64_t n) { return (int)(ceil_div64(n, PF_BLOCK) < PF_MAX_BLOCKS ? ceil_div64(n, PF_BLOCK) : PF_MAX_BLOCKS); }

}  // namespace

extern "C" int64_t wsae_profile_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols) {
    return code_args_ok(n_rows, k, WSAE_PROFILE_MAX_K, hidden, f_lo, f_cols) ? 0 : -1;
}

extern "C" int wsae_profile_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                   int64_t n_rows, int32_t f_lo, int32_t f_cols, int32_t* fires, int32_t* hist,
                                   int32_t* max_bits, int32_t* min_bits, int32_t* over, int64_t* sum_q, int64_t* total_rows,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && fires && hist && max_bits && min_bits && over && sum_q && total_rows,
                 "wsae_profile_update: null pointer");
    CW_REQUIRE_K("wsae_profile_update", k, WSAE_PROFILE_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_profile_update", hidden);
    CW_REQUIRE_ROWS("wsae_profile_update", n_rows);
    CW_REQUIRE_WINDOW("wsae_profile_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_profile_update: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    (void)workspace;  // (wsae_profile_workspace_bytes is 0: this form keeps nothing between its launches)
    if (n_rows == 0) return WSAE_OK;
    CodeArgs a = {vals, idx, seg, n_rows * k, k, f_lo, f_cols};
    ProfileOut o = {fires, hist, max_bits, min_bits, over, (unsigned long long*)sum_q, (unsigned long long*)total_rows};
    // the LDS form where most entries land in the window (measured: 5.8 against 18.6 ms whole width at H = 3072, but 2.05
    // against 1.81 ms through a tenth of H = 40960, where the walk and not the atomics sets the time)
    if (f_cols <= PF_LDS_COLS && 2 * (int64_t)f_cols >= hidden) {
        const int64_t blocks = ceil_div64(a.n, PF_BLOCK);
        profile_kernel<true><<<(int)(blocks < PF_LDS_BLOCKS ? blocks : PF_LDS_BLOCKS), PF_BLOCK, (size_t)f_cols * 12,
                               (hipStream_t)stream>>>(a, o);
    } else {
        profile_kernel<false><<<pf_grid(a.n), PF_BLOCK, 0, (hipStream_t)stream>>>(a, o);
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_sample_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols,
                                               int32_t n_strata, int32_t keep) {
    if (!sample_args_ok(n_rows, k, hidden, f_lo, f_cols, n_strata, keep)) return -1;
    // the head of f_cols n_strata lists | ent_key [n_rows k] uint64 | ent_val [n_rows k] fp32
    return list_head(nullptr, (int64_t)f_cols * n_strata).bytes + 12 * n_rows * k;
}

extern "C" int wsae_sample_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                  int64_t n_rows, int64_t ord_base, int32_t f_lo, int32_t f_cols, const float* edges,
                                  int32_t n_strata, int32_t keep, uint32_t seed, uint64_t* keys, float* svals, int32_t* seen,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && keys && svals && seen, "wsae_sample_update: null pointer");
    CW_REQUIRE_K("wsae_sample_update", k, WSAE_PROFILE_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_sample_update", hidden);
    CW_REQUIRE_ROWS("wsae_sample_update", n_rows);
    WSAE_REQUIRE(n_rows * k <= INT_MAX, "wsae_sample_update: at most 2^31 - 1 entries per call (got %lld rows of %d)",
                 (long long)n_rows, k);
    CW_REQUIRE_WINDOW("wsae_sample_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(n_strata >= 1 && n_strata <= WSAE_SAMPLE_MAX_STRATA && keep >= 1 && keep <= WSAE_SAMPLE_MAX_KEEP,
                 "wsae_sample_update: need 1 <= n_strata <= %d and 1 <= keep <= %d (got %d, %d)", WSAE_SAMPLE_MAX_STRATA,
                 WSAE_SAMPLE_MAX_KEEP, n_strata, keep);
    WSAE_REQUIRE((int64_t)f_cols * n_strata < INT_MAX, "wsae_sample_update: %d features of %d strata are more than 2^31 - 2 lists",
                 f_cols, n_strata);
    WSAE_REQUIRE(edges || n_strata == 1, "wsae_sample_update: %d strata need edges (null pointer)", n_strata);
    WSAE_REQUIRE(ord_base >= 0 && ord_base + n_rows <= (1ll << 31),
                 "wsae_sample_update: the ordinals %lld + [0, %lld) leave [0, 2^31)", (long long)ord_base, (long long)n_rows);
    const int64_t n = n_rows * k, n_lists = (int64_t)f_cols * n_strata;
    const ListHead h = list_head(workspace, n_lists);
    WSAE_REQUIRE_WORKSPACE("wsae_sample_update", workspace, workspace_bytes, h.bytes + 12 * n, n_rows);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* ent_key = (unsigned long long*)((char*)workspace + h.bytes);
    float* ent_val = (float*)(ent_key + n);
    CodeArgs a = {vals, idx, seg, n, k, f_lo, f_cols};
    SampleArgs sa = {edges, n_strata, keep, seed, ord_base, (const unsigned long long*)keys, seen};
    WSAE_HIP_CHECK(hipMemsetAsync(h.cnt, 0, sizeof(int32_t) * n_lists, st));
    sample_pass_kernel<false><<<pf_grid(n), PF_BLOCK, 0, st>>>(a, sa, h.cnt, ent_key, ent_val);
    WSAE_LAUNCH_CHECK();
    count_scan_kernel<1024><<<1, 1024, 0, st>>>(h.cnt, h.offs, h.cursor, (int)n_lists);
    WSAE_LAUNCH_CHECK();
    sample_pass_kernel<true><<<pf_grid(n), PF_BLOCK, 0, st>>>(a, sa, h.cursor, ent_key, ent_val);
    WSAE_LAUNCH_CHECK();
    sample_merge_kernel<<<(int)ceil_div64(n_lists, PF_BLOCK / 64), PF_BLOCK, 0, st>>>(h.offs, ent_key, ent_val, (int)n_lists, keep,
                                                                                     (unsigned long long*)keys, svals);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
