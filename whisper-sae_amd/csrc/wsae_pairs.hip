// Token association: exact integer statistics of every (feature, token) pair that occurs, for
// vocabularies far beyond the dense table of wsae_labels.hip, in an open-addressing hash table in device memory that many
// workgroups insert into at once.
//
// wsae_pair_update: one pass, one thread per entry of the flat code, the walk of wsae_labels.hip (pf_first_active).  A first
// active entry on a row that forms a pair adds (1, fixed-point value) under its key; the three marginals are reduced in the
// block before they touch global memory where that pays: pair_rows takes one atomic per block, feat_rows is summed in LDS
// where the dictionary fits PR_LDS_FEATS counters, tok_rows takes one atomic per maximal run of rows with one token inside
// a block pass (token runs last 5 to 25 frames; a vocabulary does not fit LDS).
// Insertion: splitmix64 finaliser, linear probing with wrap-around, a read and at most one 64-bit compare-and-swap per
// probe; no lock, no waiting on another thread; the probe loop is the only loop and runs at most cap times.  A slot goes
// from empty to one key once and never changes again, so a key read from a slot is final, whatever cache served the
// read; only "empty" can be stale, and then the compare-and-swap decides.
// wsae_pair_merge: the same insertion for every occupied slot of a source table or list.
// wsae_pair_top: count the occupied slots per group, hand every group a segment of the slot list (one atomic cursor: the
// order of the segments matters as little as the order inside one), scatter the slot numbers, then one wave per group
// walks its segment with a register top list per lane and merges the 64 lists.  The order (score descending, id
// ascending) is total, so neither the slot layout nor the segment order reaches the result.
#include <math.h>

#include "wsae_codewalk.h"

namespace {

constexpr int PR_BLOCK = 256;
constexpr int PR_MAX_BLOCKS = 2048;  // eight blocks per CU; more entries than PR_MAX_BLOCKS * PR_BLOCK: the grid-stride loop
constexpr int PR_LDS_FEATS = 8192;   // the widest dictionary whose feat_rows a block sums in LDS (32 KB)
constexpr unsigned long long PR_EMPTY = ~0ull;
constexpr int PR_INT_MAX = 0x7fffffff;  // id of an unused list slot (score -inf); no feature or token reaches it

struct PairTable {
    unsigned long long* keys;  // [cap]
    int32_t* cnt;              // [cap]
    unsigned long long* sum_q; // [cap]
    unsigned long long mask;   // cap - 1
    unsigned long long* status;  // {occupied slots, dropped contributions}
};

struct PairArgs {
    const int32_t* tokens;  // [n_rows]
    int64_t n_rows;
    int n_tokens, lag, hidden;
    unsigned long long* feat_rows;  // [hidden]
    unsigned long long* tok_rows;   // [n_tokens]
    unsigned long long* pair_rows;  // [1]
};

__host__ __device__ __forceinline__ unsigned long long pr_hash(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// (c, q) under `key`.  claimed: the thread took an empty slot; the return value: it found a slot at all.
__device__ __forceinline__ bool pr_insert(const PairTable& tb, unsigned long long key, int c, unsigned long long q,
                                          bool& claimed) {
    unsigned long long slot = pr_hash(key) & tb.mask;
    claimed = false;
    for (unsigned long long probe = 0; probe <= tb.mask; ++probe) {  // (at most cap probes: a full table ends the loop)
        unsigned long long cur = __hip_atomic_load(tb.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PR_EMPTY) {
            cur = atomicCAS(tb.keys + slot, PR_EMPTY, key);
            if (cur == PR_EMPTY) {
                claimed = true;
                cur = key;
            }
        }
        if (cur == key) {
            atomicAdd(tb.cnt + slot, c);
            atomicAdd(tb.sum_q + slot, q);
            return true;
        }
        slot = (slot + 1) & tb.mask;
    }
    return false;
}

// status += the wave's claimed slots and dropped contributions: one atomic each per wave; called by whole waves
__device__ __forceinline__ void pr_count_status(const PairTable& tb, bool claimed, bool dropped) {
    const int n_claimed = __popcll(__ballot(claimed)), n_dropped = __popcll(__ballot(dropped));
    if ((threadIdx.x & 63) == 0) {
        if (n_claimed) atomicAdd(tb.status, (unsigned long long)n_claimed);
        if (n_dropped) atomicAdd(tb.status + 1, (unsigned long long)n_dropped);
    }
}

// The token of the pair of row r, or -1 where it forms none.  The caller has checked that row r is not padding.
__device__ __forceinline__ int pr_pair_token(const CodeArgs& a, const PairArgs& g, int64_t r) {
    const int64_t q = r + g.lag;
    if (q < 0 || q >= g.n_rows) return -1;
    if (a.seg != nullptr && a.seg[q] != a.seg[r]) return -1;
    const int t = g.tokens[q];
    return t >= 0 && t < g.n_tokens ? t : -1;
}

// LDS_FEATS: the block keeps feat_rows in LDS (hidden <= PR_LDS_FEATS counters; a cell takes at most one count per row,
// so 32 bits hold a call's 2^31 - 1 rows) and adds what is not zero to the state once, at its end.
template <bool LDS_FEATS>
__global__ __launch_bounds__(PR_BLOCK) void pair_update_kernel(CodeArgs a, PairArgs g, PairTable tb) {
    __shared__ int s_idx[PR_BLOCK];
    __shared__ unsigned int s_pairs;
    extern __shared__ unsigned int pr_feats[];  // (LDS_FEATS) [hidden]
    if (LDS_FEATS) {
        for (int i = threadIdx.x; i < g.hidden; i += PR_BLOCK) pr_feats[i] = 0u;
    }
    if (threadIdx.x == 0) s_pairs = 0u;
    // (the first barrier of pf_first_active orders this before the first add)
    unsigned int my_pairs = 0;  // the pairs of the rows whose column 0 this thread walked
    for (int64_t base = (int64_t)blockIdx.x * PR_BLOCK; base < a.n; base += (int64_t)gridDim.x * PR_BLOCK) {
        float v;
        int f;
        int64_t r;
        bool head;
        const bool act = pf_first_active(a, base, s_idx, v, f, r, head);
        bool claimed = false, dropped = false;
        if (head || act) {
            const int t = pr_pair_token(a, g, r);
            if (t >= 0) {
                if (head) {
                    ++my_pairs;
                    // tok_rows: the first row of a run of rows with this token inside the pass counts the run.  A run
                    // ends at the pass's last row, at a padding row or at a row with another token (or none).
                    const int64_t pass_first = (base + a.k - 1) / a.k;  // the first row whose column 0 lies in the pass
                    bool leads = r == pass_first;
                    if (!leads) leads = (a.seg != nullptr && a.seg[r - 1] < 0) || pr_pair_token(a, g, r - 1) != t;
                    if (leads) {
                        const int64_t pass_end = min64((base + PR_BLOCK - 1) / a.k, g.n_rows - 1);  // the last such row
                        unsigned long long run = 1;
                        for (int64_t s = r + 1; s <= pass_end; ++s) {
                            if ((a.seg != nullptr && a.seg[s] < 0) || pr_pair_token(a, g, s) != t) break;
                            ++run;
                        }
                        atomicAdd(g.tok_rows + t, run);
                    }
                }
                if (act) {
                    if (LDS_FEATS) {
                        atomicAdd(pr_feats + f, 1u);
                    } else {
                        atomicAdd(g.feat_rows + f, 1ull);
                    }
                    // rint(min(v, 4096) * 2^20): the product is exact in fp32, the conversion rounds to nearest even
                    const unsigned long long q = (unsigned long long)__float2ll_rn(fminf(v, 4096.f) * 1048576.f);
                    dropped = !pr_insert(tb, (unsigned long long)(unsigned int)f << 32 | (unsigned int)t, 1, q, claimed);
                }
            }
        }
        pr_count_status(tb, claimed, dropped);
    }
    const unsigned int wave_pairs = (unsigned int)wave_sum_i((int)my_pairs);
    if ((threadIdx.x & 63) == 0 && wave_pairs) atomicAdd(&s_pairs, wave_pairs);
    __syncthreads();
    if (threadIdx.x == 0 && s_pairs) atomicAdd(g.pair_rows, (unsigned long long)s_pairs);
    if (LDS_FEATS) {
        for (int i = threadIdx.x; i < g.hidden; i += PR_BLOCK) {
            const unsigned int n = pr_feats[i];
            if (n) atomicAdd(g.feat_rows + i, (unsigned long long)n);
        }
    }
}

__global__ __launch_bounds__(PR_BLOCK) void pair_merge_kernel(const unsigned long long* __restrict__ src_keys,
                                                              const int32_t* __restrict__ src_cnt,
                                                              const unsigned long long* __restrict__ src_sum_q, int64_t src_cap,
                                                              PairTable tb) {
    // (whole waves reach pr_count_status: the trip count is block-uniform)
    for (int64_t base = (int64_t)blockIdx.x * PR_BLOCK; base < src_cap; base += (int64_t)gridDim.x * PR_BLOCK) {
        const int64_t s = base + threadIdx.x;
        bool claimed = false, dropped = false;
        if (s < src_cap) {
            const unsigned long long key = src_keys[s];
            if (key != PR_EMPTY) dropped = !pr_insert(tb, key, src_cnt[s], src_sum_q[s], claimed);
        }
        pr_count_status(tb, claimed, dropped);
    }
}

// ---- wsae_pair_top ---------------------------------------------------------------------------------------------------------
struct TopArgs {
    const unsigned long long* keys;
    const int32_t* cnt;
    const long long* sum_q;
    int64_t cap;
    const long long* feat_rows;
    const long long* tok_rows;
    const long long* pair_rows;
    int hidden, n_tokens, by, n_groups, score, min_count, n;
};

// The group of the key in slot s (its feature or its token), or -1 where the slot is empty or the key out of range.
__device__ __forceinline__ int top_group(const TopArgs& g, int64_t s) {
    const unsigned long long key = g.keys[s];
    if (key == PR_EMPTY) return -1;
    const unsigned int f = (unsigned int)(key >> 32), t = (unsigned int)key;
    if (f >= (unsigned int)g.hidden || t >= (unsigned int)g.n_tokens) return -1;
    return (int)(g.by == WSAE_PAIR_BY_FEATURE ? f : t);
}

__global__ __launch_bounds__(PR_BLOCK) void top_count_kernel(TopArgs g, unsigned int* __restrict__ count) {
    for (int64_t s = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x; s < g.cap; s += (int64_t)gridDim.x * PR_BLOCK) {
        const int grp = top_group(g, s);
        if (grp >= 0) atomicAdd(count + grp, 1u);
    }
}

// next[grp] = the start of the group's segment; cursor[0] counts the slots handed out
__global__ __launch_bounds__(PR_BLOCK) void top_segments_kernel(int n_groups, const unsigned int* __restrict__ count,
                                                                unsigned int* __restrict__ next, unsigned int* cursor) {
    const int grp = blockIdx.x * PR_BLOCK + threadIdx.x;
    if (grp >= n_groups) return;
    const unsigned int c = count[grp];
    next[grp] = c ? atomicAdd(cursor, c) : 0u;
}

// slots[segment of grp] = the group's slot numbers, in any order; next[grp] ends up at the segment's end
__global__ __launch_bounds__(PR_BLOCK) void top_scatter_kernel(TopArgs g, unsigned int* __restrict__ next,
                                                               unsigned int* __restrict__ slots) {
    for (int64_t s = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x; s < g.cap; s += (int64_t)gridDim.x * PR_BLOCK) {
        const int grp = top_group(g, s);
        if (grp >= 0) slots[atomicAdd(next + grp, 1u)] = (unsigned int)s;
    }
}

__device__ __forceinline__ double top_score(const TopArgs& g, unsigned long long key, int cnt, long long sum_q) {
    const double c = (double)cnt;
    if (g.score == WSAE_PAIR_COUNT) return c;
    if (g.score == WSAE_PAIR_MEAN) return ((double)sum_q * (1.0 / 1048576.0)) / c;
    const double a = (double)g.feat_rows[key >> 32], b = (double)g.tok_rows[(unsigned int)key];
    switch (g.score) {
        case WSAE_PAIR_PRECISION: return c / a;
        case WSAE_PAIR_RECALL: return c / b;
        case WSAE_PAIR_F1: return (2.0 * c) / (a + b);
        case WSAE_PAIR_JACCARD: return c / ((a + b) - c);
        default: return (c * (double)g.pair_rows[0]) / (a * b);  // WSAE_PAIR_LIFT
    }
}

__device__ __forceinline__ bool top_before(double v, int i, double w, int j) { return v > w || (v == w && i < j); }

// One wave per group.  Every lane keeps the NB best of the pairs it walked, sorted; the 64 lists are merged by n rounds of
// "the best head of all lanes wins and leaves its list".
template <int NB>
__global__ __launch_bounds__(PR_BLOCK) void top_select_kernel(TopArgs g, const unsigned int* __restrict__ count,
                                                              const unsigned int* __restrict__ next,
                                                              const unsigned int* __restrict__ slots, int32_t* __restrict__ ids,
                                                              double* __restrict__ scores, int32_t* __restrict__ counts,
                                                              long long* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const int grp = blockIdx.x * (PR_BLOCK / 64) + (threadIdx.x >> 6);
    if (grp >= g.n_groups) return;  // (wave-uniform)
    double lv[NB];
    int li[NB];
    unsigned int ls[NB];  // the slot beside the id: the winner reads cnt and sum_q from it
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        lv[p] = -INFINITY;
        li[p] = PR_INT_MAX;
        ls[p] = 0u;
    }
    const unsigned int end = next[grp], begin = end - count[grp];
    for (unsigned int e = begin + lane; e < end; e += 64) {
        unsigned int s = slots[e];
        const int c = g.cnt[s];
        if (c < g.min_count) continue;
        const unsigned long long key = g.keys[s];
        double v = top_score(g, key, c, g.sum_q[s]);
        int i = (int)(g.by == WSAE_PAIR_BY_FEATURE ? (unsigned int)key : (unsigned int)(key >> 32));
        if (!top_before(v, i, lv[NB - 1], li[NB - 1])) continue;  // (also every NaN score)
#pragma unroll
        for (int p = 0; p < NB; ++p) {  // static indexing: the list stays in registers
            const bool b = top_before(v, i, lv[p], li[p]);
            const double tv = lv[p];
            const int ti = li[p];
            const unsigned int ts = ls[p];
            lv[p] = b ? v : tv;
            li[p] = b ? i : ti;
            ls[p] = b ? s : ts;
            v = b ? tv : v;
            i = b ? ti : i;
            s = b ? ts : s;
        }
    }
    const int64_t out = (int64_t)grp * g.n;
    for (int j = 0; j < g.n; ++j) {
        double bv = lv[0];
        int bi = li[0];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (top_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == PR_INT_MAX) {  // (wave-uniform) every list is used up: the tail
            if (lane == 0) {
                ids[out + j] = -1;
                scores[out + j] = -INFINITY;
                counts[out + j] = 0;
                sums[out + j] = 0;
            }
            continue;
        }
        if (li[0] == bi) {  // (ids are unique within a group: one lane)
            ids[out + j] = bi;
            scores[out + j] = bv;
            counts[out + j] = g.cnt[ls[0]];
            sums[out + j] = g.sum_q[ls[0]];
#pragma unroll
            for (int p = 0; p + 1 < NB; ++p) {
                lv[p] = lv[p + 1];
                li[p] = li[p + 1];
                ls[p] = ls[p + 1];
            }
            lv[NB - 1] = -INFINITY;
            li[NB - 1] = PR_INT_MAX;
        }
    }
}

inline bool cap_ok(int64_t cap) { return cap >= (1ll << 10) && cap <= (1ll << 31) && (cap & (cap - 1)) == 0; }

inline int pr_grid(int64_t items) {
    const int64_t blocks = ceil_div64(items, PR_BLOCK);
    return (int)(blocks < PR_MAX_BLOCKS ? blocks : PR_MAX_BLOCKS);
}

// the workspace of wsae_pair_top: count [n_groups], next [n_groups], cursor (one word in a section of its own), slots [cap]
inline int64_t top_groups_bytes(int n_groups) { return align256((int64_t)sizeof(unsigned int) * n_groups); }

#define PR_REQUIRE_CAP(FN, cap) \
    WSAE_REQUIRE(cap_ok(cap), FN ": cap must be a power of two in 2^10 .. 2^31 (got %lld)", (long long)(cap))

}  // namespace

extern "C" int wsae_pair_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                const int32_t* tokens, int64_t n_rows, int32_t n_tokens, int32_t lag, uint64_t* keys,
                                int32_t* cnt, int64_t* sum_q, int64_t cap, int64_t* status, int64_t* feat_rows,
                                int64_t* tok_rows, int64_t* pair_rows, void* stream) {
    WSAE_REQUIRE(vals && idx && tokens && keys && cnt && sum_q && status && feat_rows && tok_rows && pair_rows,
                 "wsae_pair_update: null pointer");
    CW_REQUIRE_K("wsae_pair_update", k, WSAE_PAIR_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_pair_update", hidden);
    CW_REQUIRE_ROWS("wsae_pair_update", n_rows);
    WSAE_REQUIRE(n_tokens >= 1 && n_tokens <= WSAE_PAIR_MAX_TOKENS, "wsae_pair_update: need 1 <= n_tokens <= %d (got %d)",
                 WSAE_PAIR_MAX_TOKENS, n_tokens);
    CW_REQUIRE_LAG("wsae_pair_update", lag);
    PR_REQUIRE_CAP("wsae_pair_update", cap);
    if (n_rows == 0) return WSAE_OK;
    CodeArgs a = {vals, idx, seg, n_rows * k, k, 0, hidden};
    PairArgs g = {tokens, n_rows, n_tokens, lag, hidden, (unsigned long long*)feat_rows, (unsigned long long*)tok_rows,
                  (unsigned long long*)pair_rows};
    PairTable tb = {(unsigned long long*)keys, cnt, (unsigned long long*)sum_q, (unsigned long long)cap - 1,
                    (unsigned long long*)status};
    const int grid = pr_grid(a.n);
    if (hidden <= PR_LDS_FEATS) {
        pair_update_kernel<true><<<grid, PR_BLOCK, sizeof(unsigned int) * hidden, (hipStream_t)stream>>>(a, g, tb);
    } else {
        pair_update_kernel<false><<<grid, PR_BLOCK, 0, (hipStream_t)stream>>>(a, g, tb);
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int wsae_pair_merge(const uint64_t* src_keys, const int32_t* src_cnt, const int64_t* src_sum_q, int64_t src_cap,
                               uint64_t* keys, int32_t* cnt, int64_t* sum_q, int64_t cap, int64_t* status, void* stream) {
    WSAE_REQUIRE(src_keys && src_cnt && src_sum_q && keys && cnt && sum_q && status, "wsae_pair_merge: null pointer");
    WSAE_REQUIRE(src_cap >= 1 && src_cap <= (1ll << 31), "wsae_pair_merge: need 1 <= src_cap <= 2^31 (got %lld)",
                 (long long)src_cap);
    PR_REQUIRE_CAP("wsae_pair_merge", cap);
    WSAE_REQUIRE(src_keys != keys && src_cnt != cnt && src_sum_q != sum_q,
                 "wsae_pair_merge: the source and the destination are the same memory");
    PairTable tb = {(unsigned long long*)keys, cnt, (unsigned long long*)sum_q, (unsigned long long)cap - 1,
                    (unsigned long long*)status};
    pair_merge_kernel<<<pr_grid(src_cap), PR_BLOCK, 0, (hipStream_t)stream>>>(
        (const unsigned long long*)src_keys, src_cnt, (const unsigned long long*)src_sum_q, src_cap, tb);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_pair_top_workspace_bytes(int64_t cap, int32_t n_groups) {
    if (!cap_ok(cap) || n_groups < 1) return -1;
    return 2 * top_groups_bytes(n_groups) + 256 + align256((int64_t)sizeof(unsigned int) * cap);
}

extern "C" int wsae_pair_top(const uint64_t* keys, const int32_t* cnt, const int64_t* sum_q, int64_t cap,
                             const int64_t* feat_rows, const int64_t* tok_rows, const int64_t* pair_rows, int32_t hidden,
                             int32_t n_tokens, int32_t by, int32_t n_groups, int32_t score, int32_t min_count, int32_t n,
                             int32_t* ids, double* scores, int32_t* counts, int64_t* sums, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(keys && cnt && sum_q && feat_rows && tok_rows && pair_rows && ids && scores && counts && sums,
                 "wsae_pair_top: null pointer");
    PR_REQUIRE_CAP("wsae_pair_top", cap);
    CW_REQUIRE_HIDDEN("wsae_pair_top", hidden);
    WSAE_REQUIRE(n_tokens >= 1 && n_tokens <= WSAE_PAIR_MAX_TOKENS, "wsae_pair_top: need 1 <= n_tokens <= %d (got %d)",
                 WSAE_PAIR_MAX_TOKENS, n_tokens);
    WSAE_REQUIRE(by == WSAE_PAIR_BY_FEATURE || by == WSAE_PAIR_BY_TOKEN, "wsae_pair_top: unknown direction %d", by);
    WSAE_REQUIRE(n_groups == (by == WSAE_PAIR_BY_FEATURE ? hidden : n_tokens),
                 "wsae_pair_top: n_groups must be %s = %d (got %d)", by == WSAE_PAIR_BY_FEATURE ? "hidden" : "n_tokens",
                 by == WSAE_PAIR_BY_FEATURE ? hidden : n_tokens, n_groups);
    WSAE_REQUIRE(score >= WSAE_PAIR_COUNT && score <= WSAE_PAIR_MEAN, "wsae_pair_top: unknown score %d", score);
    WSAE_REQUIRE(n >= 1 && n <= WSAE_PAIR_MAX_N, "wsae_pair_top: need 1 <= n <= %d (got %d)", WSAE_PAIR_MAX_N, n);
    const int64_t need = wsae_pair_top_workspace_bytes(cap, n_groups);
    WSAE_REQUIRE_WORKSPACE("wsae_pair_top", workspace, workspace_bytes, need, 1);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_pair_top", workspace, 8);
    hipStream_t st = (hipStream_t)stream;
    const int64_t gb = top_groups_bytes(n_groups);
    unsigned int* count = (unsigned int*)workspace;
    unsigned int* next = (unsigned int*)((char*)workspace + gb);
    unsigned int* cursor = (unsigned int*)((char*)workspace + 2 * gb);
    unsigned int* slots = (unsigned int*)((char*)workspace + 2 * gb + 256);
    TopArgs g = {(const unsigned long long*)keys, cnt, (const long long*)sum_q, cap, (const long long*)feat_rows,
                 (const long long*)tok_rows, (const long long*)pair_rows, hidden, n_tokens, by, n_groups, score, min_count, n};
    WSAE_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)gb, st));
    WSAE_HIP_CHECK(hipMemsetAsync(cursor, 0, sizeof(unsigned int), st));
    top_count_kernel<<<pr_grid(cap), PR_BLOCK, 0, st>>>(g, count);
    top_segments_kernel<<<ceil_div(n_groups, PR_BLOCK), PR_BLOCK, 0, st>>>(n_groups, count, next, cursor);
    top_scatter_kernel<<<pr_grid(cap), PR_BLOCK, 0, st>>>(g, next, slots);
    const int grid = ceil_div(n_groups, PR_BLOCK / 64);
    if (n <= 8) {
        top_select_kernel<8><<<grid, PR_BLOCK, 0, st>>>(g, count, next, slots, ids, scores, counts, (long long*)sums);
    } else if (n <= 16) {
        top_select_kernel<16><<<grid, PR_BLOCK, 0, st>>>(g, count, next, slots, ids, scores, counts, (long long*)sums);
    } else {
        top_select_kernel<32><<<grid, PR_BLOCK, 0, st>>>(g, count, next, slots, ids, scores, counts, (long long*)sums);
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
