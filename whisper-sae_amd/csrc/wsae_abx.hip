// ABX phone discrimination: DTW distances between segments of a compact code, and the count of
// the triples (a, b, x) in which x lies closer to a, an item of its own category, than to b, an item of another.
//
// wsae_dtw_matrix: two launches.  dyn_canon_kernel (wsae_dyn_canon.h) writes the canonical code of every row.
// dtw_kernel gives a workgroup one a-item and a group of DT_GROUP consecutive b-items.  The a-item is walked in tiles
// of DT_TILE frames: the active entries (f, frame, u) of a tile go into an LDS hash table keyed by feature, chained
// through the entry list (the entry of position e of the tile is slot e: no counter, and the order of a chain does not
// matter since a frame holds a feature once).  Then every lane owns one b-frame - the frames of the group's items are
// packed side by side into passes of DT_BLOCK lanes, an item never split - walks the k canonical entries of its own row
// in ascending position and probes the table; a hit adds the exact fp64 product to the accumulator of the a-frame that
// holds the feature, an unrolled select over DT_TILE registers.  That is the chain wsae.h states: per (a-frame,
// b-frame) one chain in the order of the b-frame's entries.  The sums become costs in an LDS tile, and one lane per
// (a, b) pair advances the dynamic program by the DT_TILE rows of the tile: the row above lives in LDS per b-frame
// (D fp64, L int32) and is overwritten in place, the diagonal and the left neighbour travel in registers.
//
// wsae_abx_count: a workgroup per X row.  Pass 1 appends the items admissible as `a` for this x to a list in the
// workspace.  Pass 2 gives every lane one candidate b; the a-list is read 64 entries at a time (index, distance and
// speaker per lane) and broadcast entry by entry (readlane), so a triple costs a few VALU operations and no memory
// access, and a lane's cell (cat[x], cat[b]) is fixed: its counts stay in registers until the list is through, go to
// per-block counters in LDS, and to the tables with one global integer atomic per touched cell at the end of the block.
#include <math.h>

#include "wsae_dyn_canon.h"

namespace {

constexpr int DT_BLOCK = 128;  // lanes of a pass: b-frames side by side (>= WSAE_DTW_MAX_LEN: an item fits a pass)
constexpr int DT_TILE = 16;    // a-frames whose accumulators a lane keeps in registers
constexpr int DT_GROUP = 16;   // b-items of a workgroup
constexpr int DT_MAX_Y = 32768;
constexpr int DT_FRAMES = DT_GROUP * WSAE_DTW_MAX_LEN;  // the b-frames of a group at most
static_assert(DT_BLOCK >= WSAE_DTW_MAX_LEN && DT_BLOCK % DT_GROUP == 0, "an item fits a pass; a DP lane per item");

struct DtwArgs {
    const float* cu;
    const int32_t* cf;
    const double* nrm;
    const int32_t* act;
    int64_t n_rows;
    const int32_t *a_start, *a_len, *b_start, *b_len;
    int n_a, n_b, k, buckets, normalize;
    float* dist;
    int32_t* steps;  // nullable
    int64_t ldd;
};

// buckets of the table of a tile: a power of two, at least the entries of a tile
inline int dtw_buckets(int k) {
    int b = 64;
    while (b < DT_TILE * k) b *= 2;
    return b;
}
// dynamic LDS of dtw_kernel: D, L, the cost tile, n_r and a_r of the tile, the table (heads; f, u, link per entry)
inline size_t dtw_lds_bytes(int k) {
    return (size_t)8 * DT_FRAMES + 4 * DT_FRAMES + 8 * DT_TILE * DT_BLOCK + 8 * DT_TILE + 4 * DT_TILE + 4 * (size_t)dtw_buckets(k) +
           12 * (size_t)DT_TILE * k;
}

__device__ __forceinline__ bool dtw_item_ok(int start, int len, int64_t n_rows) {
    return len >= 1 && len <= WSAE_DTW_MAX_LEN && start >= 0 && (int64_t)start + len <= n_rows;
}

template <bool JAC>
__global__ __launch_bounds__(DT_BLOCK) void dtw_kernel(DtwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* s_D = (double*)smem;                          // [DT_FRAMES] the DP row above, per b-frame of the group
    int* s_L = (int*)(s_D + DT_FRAMES);                   // [DT_FRAMES]
    int* s_c = s_L + DT_FRAMES;                           // [DT_TILE, DT_BLOCK, 2] the sums, then the costs of a pass
    double* s_an = (double*)(s_c + 2 * DT_TILE * DT_BLOCK);   // [DT_TILE] n_r of the tile's frames
    int* s_aa = (int*)(s_an + DT_TILE);                   // [DT_TILE] a_r
    int* s_head = s_aa + DT_TILE;                         // [buckets] entry + 1, 0 = empty
    int* s_ef = s_head + a.buckets;                       // [DT_TILE k] feature
    float* s_eu = (float*)(s_ef + DT_TILE * a.k);         // [DT_TILE k] u
    int* s_en = (int*)(s_eu + DT_TILE * a.k);             // [DT_TILE k] (next entry + 1) << 4 | frame of the tile
    __shared__ int s_bstart[DT_GROUP], s_blen[DT_GROUP], s_boff[DT_GROUP], s_bpass[DT_GROUP], s_bslot[DT_GROUP], s_npass;

    const int tid = threadIdx.x;
    const int k = a.k, mask = a.buckets - 1;
    const int64_t b0 = (int64_t)blockIdx.x * DT_GROUP;
    const int nb = (int)min64(DT_GROUP, a.n_b - b0);
    if (tid < DT_GROUP) {
        int st = 0, ln = 0;
        if (tid < nb) {
            st = a.b_start[b0 + tid], ln = a.b_len[b0 + tid];
            if (!dtw_item_ok(st, ln, a.n_rows)) ln = 0;  // (an invalid item takes no lane)
        }
        s_bstart[tid] = st, s_blen[tid] = ln;
    }
    __syncthreads();
    if (tid == 0) {  // the passes: items side by side while they fit DT_BLOCK lanes
        int off = 0, pass = 0, slot = 0;
        for (int j = 0; j < DT_GROUP; ++j) {
            const int ln = s_blen[j];
            if (slot + ln > DT_BLOCK) ++pass, slot = 0;
            s_boff[j] = off, s_bpass[j] = pass, s_bslot[j] = slot;
            off += ln, slot += ln;
        }
        s_npass = pass + 1;
    }
    __syncthreads();
    const int n_pass = s_npass;
    // the DP lane of item j is lane j * (DT_BLOCK / DT_GROUP): the pairs spread over the waves
    const int dp_item = tid % (DT_BLOCK / DT_GROUP) == 0 ? tid / (DT_BLOCK / DT_GROUP) : DT_GROUP;
    const int dp_m = dp_item < nb ? s_blen[dp_item] : 0;
    const int dp_off = dp_item < nb ? s_boff[dp_item] : 0, dp_slot = dp_item < nb ? s_bslot[dp_item] : 0;
    const int dp_pass = dp_item < nb ? s_bpass[dp_item] : -1;
    const float nanf_ = __int_as_float(0x7fc00000);

    for (int ai = blockIdx.y; ai < a.n_a; ai += gridDim.y) {
        const int ast = a.a_start[ai], an = a.a_len[ai];
        float* out = a.dist + (int64_t)ai * a.ldd + b0;
        int32_t* out_l = a.steps != nullptr ? a.steps + (int64_t)ai * a.ldd + b0 : nullptr;
        if (!dtw_item_ok(ast, an, a.n_rows)) {  // (block-uniform)
            if (tid < nb) {
                out[tid] = nanf_;
                if (out_l != nullptr) out_l[tid] = 0;
            }
            continue;
        }
        for (int i0 = 0; i0 < an; i0 += DT_TILE) {
            const int ta = an - i0 < DT_TILE ? an - i0 : DT_TILE;
            __syncthreads();  // the table and the tile of the previous round have been read
            for (int h = tid; h < a.buckets; h += DT_BLOCK) s_head[h] = 0;
            if (tid < ta) {
                s_an[tid] = a.nrm[ast + i0 + tid];
                s_aa[tid] = a.act[ast + i0 + tid];
            }
            __syncthreads();
            for (int e = tid; e < ta * k; e += DT_BLOCK) {
                const int64_t at = (int64_t)(ast + i0) * k + e;  // (the rows of the tile are consecutive)
                const int f = a.cf[at];
                if (f >= 0) {
                    s_ef[e] = f;
                    s_eu[e] = a.cu[at];
                    const int prev = atomicExch(&s_head[f & mask], e + 1);
                    s_en[e] = (prev << 4) | (e / k);
                }
            }
            __syncthreads();
            for (int pass = 0; pass < n_pass; ++pass) {
                int jb = -1;
                for (int j = 0; j < nb; ++j) {
                    if (s_bpass[j] == pass && tid >= s_bslot[j] && tid < s_bslot[j] + s_blen[j]) jb = j;
                }
                if (jb >= 0) {
                    const int64_t row = (int64_t)s_bstart[jb] + (tid - s_bslot[jb]);
                    double acc[DT_TILE];
                    int cnt[DT_TILE];
#pragma unroll
                    for (int t = 0; t < DT_TILE; ++t) acc[t] = 0.0, cnt[t] = 0;
                    for (int p = 0; p < k; ++p) {
                        const int f = a.cf[row * k + p];
                        if (f < 0) continue;
                        const double uq = (double)a.cu[row * k + p];
                        for (int e1 = s_head[f & mask]; e1 != 0;) {
                            const int e = e1 - 1;
                            const int link = s_en[e];
                            if (s_ef[e] == f) {
                                const int i = link & 15;
                                if (JAC) {
#pragma unroll
                                    for (int t = 0; t < DT_TILE; ++t) cnt[t] += t == i ? 1 : 0;
                                } else {
                                    const double prod = uq * (double)s_eu[e];  // (exact: two fp32 factors)
#pragma unroll
                                    for (int t = 0; t < DT_TILE; ++t) acc[t] = t == i ? acc[t] + prod : acc[t];
                                }
                            }
                            e1 = link >> 4;
                        }
                    }
                    // the sums go through the lane's own cells of the tile: the costs are made in a rolled loop (one
                    // copy of the fp64 root and quotient, not DT_TILE interleaved ones)
#pragma unroll
                    for (int t = 0; t < DT_TILE; ++t) {
                        int* cell = s_c + 2 * (t * DT_BLOCK + tid);
                        if (JAC) {
                            cell[0] = cnt[t];
                        } else {
                            cell[0] = __double2loint(acc[t]), cell[1] = __double2hiint(acc[t]);
                        }
                    }
                    const double n_q = JAC ? 0.0 : a.nrm[row];
                    const int a_q = JAC ? a.act[row] : 0;
                    for (int t = 0; t < ta; ++t) {
                        int* cell = s_c + 2 * (t * DT_BLOCK + tid);
                        double c = 0.0;
                        if (JAC) {
                            const int inter = cell[0], uni = s_aa[t] + a_q - inter;
                            if (uni != 0) c = (double)inter / (double)uni;
                        } else {
                            const double n_r = s_an[t];
                            if (n_r != 0.0 && n_q != 0.0) {
                                c = __hiloint2double(cell[1], cell[0]) / sqrt(n_r * n_q);
                                if (!(c <= 1.0)) c = 1.0;
                            }
                        }
                        cell[0] = __float_as_int((float)(1.0 - c));
                    }
                }
                __syncthreads();
                if (dp_pass == pass && dp_m > 0) {
                    for (int t = 0; t < ta; ++t) {
                        const bool top = i0 + t == 0;
                        double dD = 0.0, lD = 0.0;
                        int dL = 0, lL = 0;
                        for (int j = 0; j < dp_m; ++j) {
                            const double e = (double)__int_as_float(s_c[2 * (t * DT_BLOCK + dp_slot + j)]);
                            double uD = 0.0, bD = 0.0;
                            int uL = 0, bL = 0;
                            if (!top) uD = s_D[dp_off + j], uL = s_L[dp_off + j];
                            if (top) {
                                if (j > 0) bD = lD, bL = lL;
                            } else if (j == 0) {
                                bD = uD, bL = uL;
                            } else {  // diagonal, above, left: the smallest, ties to the earlier
                                bD = dD, bL = dL;
                                if (uD < bD) bD = uD, bL = uL;
                                if (lD < bD) bD = lD, bL = lL;
                            }
                            const double nD = e + bD;
                            const int nL = bL + 1;
                            dD = uD, dL = uL, lD = nD, lL = nL;
                            s_D[dp_off + j] = nD, s_L[dp_off + j] = nL;
                        }
                    }
                }
                __syncthreads();  // the cost tile is free for the next pass
            }
        }
        if (dp_item < nb) {
            float d = nanf_;
            int l = 0;
            if (dp_m > 0) {
                const double D = s_D[dp_off + dp_m - 1];
                l = s_L[dp_off + dp_m - 1];
                d = a.normalize ? (float)(D / (double)l) : (float)D;
            }
            out[dp_item] = d;
            if (out_l != nullptr) out_l[dp_item] = l;
        }
    }
}

// ---- the triple count -------------------------------------------------------------------------------------------------------
constexpr int AX_BLOCK = 256;

struct AbxArgs {
    const float* dist;
    int64_t ldd;
    int x_lo, n_x, n_items, n_cats, mode;
    const int32_t *cat, *ctx, *spk;  // ctx nullable; spk nullable with WSAE_ABX_ANY
    unsigned long long *wins2, *total, *skipped;
    int32_t* list;  // [n_x, n_items] the items admissible as a, per x
};

__global__ __launch_bounds__(AX_BLOCK) void abx_count_kernel(AbxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* s_tot = (unsigned long long*)smem;  // [n_cats] by cat[b]
    unsigned long long* s_win = s_tot + a.n_cats;
    __shared__ unsigned long long s_skip;
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int x = blockIdx.x, xi = a.x_lo + x;
    const int mode = a.mode;
    const int cx = a.cat[xi];
    const int tx = a.ctx != nullptr ? a.ctx[xi] : 0;
    const int sx = mode != WSAE_ABX_ANY ? a.spk[xi] : 0;
    if (cx < 0 || cx >= a.n_cats || tx < 0 || sx < 0) return;  // (block-uniform: x takes no part)
    for (int c = tid; c < a.n_cats; c += AX_BLOCK) s_tot[c] = 0ull, s_win[c] = 0ull;
    if (tid == 0) s_n = 0, s_skip = 0ull;
    __syncthreads();
    int32_t* list = a.list + (int64_t)x * a.n_items;
    const float* drow = a.dist + (int64_t)x * a.ldd;
    for (int i = tid; i < a.n_items; i += AX_BLOCK) {
        bool ok = i != xi && a.cat[i] == cx && (a.ctx == nullptr || a.ctx[i] == tx);
        if (ok && mode != WSAE_ABX_ANY) {
            const int s = a.spk[i];
            ok = mode == WSAE_ABX_WITHIN ? s == sx : (s >= 0 && s != sx);
        }
        if (ok) list[atomicAdd(&s_n, 1)] = i;
    }
    __syncthreads();  // (the list is read by other waves of this block)
    const int na = s_n;
    if (na == 0) return;
    for (int base_b = 0; base_b < a.n_items; base_b += AX_BLOCK) {
        const int b = base_b + tid;
        bool okb = false;
        int cb = 0, sb = 0;
        float db = 0.f;
        if (b < a.n_items) {
            cb = a.cat[b];
            okb = cb >= 0 && cb < a.n_cats && cb != cx && (a.ctx == nullptr || a.ctx[b] == tx);
            if (okb && mode != WSAE_ABX_ANY) {
                sb = a.spk[b];
                okb = mode == WSAE_ABX_WITHIN ? sb == sx : (sb >= 0 && sb != sx);
            }
            if (okb) db = drow[b];
        }
        if (__ballot(okb) == 0ull) continue;  // (wave-uniform)
        const bool nan_b = db != db;
        unsigned int tot = 0u, win = 0u, skip = 0u;
        for (int base = 0; base < na; base += 64) {
            const int n = na - base < 64 ? na - base : 64;
            float da = 0.f;
            int sa = 0;
            if (lane < n) {
                const int ia = list[base + lane];
                da = drow[ia];
                if (mode == WSAE_ABX_ACROSS) sa = a.spk[ia];
            }
            for (int j = 0; j < n; ++j) {
                const float dj = lane_f32(da, j);
                const bool adm = okb && (mode != WSAE_ABX_ACROSS || __builtin_amdgcn_readlane(sa, j) == sb);
                const bool bad = nan_b || dj != dj;
                skip += adm && bad ? 1u : 0u;
                tot += adm && !bad ? 1u : 0u;
                win += adm && !bad ? (dj < db ? 2u : (dj == db ? 1u : 0u)) : 0u;
            }
        }
        if (tot) {
            atomicAdd(&s_tot[cb], (unsigned long long)tot);
            if (win) atomicAdd(&s_win[cb], (unsigned long long)win);
        }
        if (skip) atomicAdd(&s_skip, (unsigned long long)skip);
    }
    __syncthreads();
    for (int c = tid; c < a.n_cats; c += AX_BLOCK) {
        if (s_tot[c]) atomicAdd(a.total + (int64_t)cx * a.n_cats + c, s_tot[c]);
        if (s_win[c]) atomicAdd(a.wins2 + (int64_t)cx * a.n_cats + c, s_win[c]);
    }
    if (tid == 0 && s_skip) atomicAdd(a.skipped, s_skip);
}

inline bool dtw_args_ok(int64_t n_rows, int k, int hidden, int n_a, int n_b) {
    return n_rows >= 0 && n_rows <= INT_MAX && k >= 1 && k <= WSAE_DTW_MAX_K && hidden >= 1 && n_a >= 0 && n_b >= 0;
}

inline bool abx_args_ok(int n_items, int n_x, int n_cats) {
    return n_items >= 0 && n_x >= 0 && n_x <= n_items && n_cats >= 1 && n_cats <= WSAE_ABX_MAX_CATS;
}

}  // namespace

extern "C" int64_t wsae_dtw_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_a, int32_t n_b) {
    return dtw_args_ok(n_rows, k, hidden, n_a, n_b) ? dyn_layout(n_rows, k).total : -1;
}

extern "C" int wsae_dtw_matrix(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                               const float* weight, int64_t n_rows, const int32_t* a_start, const int32_t* a_len, int32_t n_a,
                               const int32_t* b_start, const int32_t* b_len, int32_t n_b, int32_t metric, int32_t normalize,
                               float* dist, int32_t* steps, int64_t ldd, void* workspace, int64_t workspace_bytes,
                               void* stream) {
    CW_REQUIRE_K("wsae_dtw_matrix", k, WSAE_DTW_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_dtw_matrix", hidden);
    CW_REQUIRE_ROWS("wsae_dtw_matrix", n_rows);
    WSAE_REQUIRE(n_a >= 0 && n_b >= 0, "wsae_dtw_matrix: need n_a >= 0 and n_b >= 0 (got %d and %d)", n_a, n_b);
    WSAE_REQUIRE(metric == WSAE_DTW_COSINE || metric == WSAE_DTW_JACCARD, "wsae_dtw_matrix: unknown metric %d", metric);
    WSAE_REQUIRE(ldd >= n_b, "wsae_dtw_matrix: need ldd >= n_b = %d (got %lld)", n_b, (long long)ldd);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_dtw_matrix: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    if (n_a == 0 || n_b == 0 || n_rows == 0) return WSAE_OK;
    WSAE_REQUIRE(vals && idx && a_start && a_len && b_start && b_len && dist, "wsae_dtw_matrix: null pointer");
    const DynLayout w = dyn_layout(n_rows, k);
    WSAE_REQUIRE_WORKSPACE("wsae_dtw_matrix", workspace, workspace_bytes, w.total, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_dtw_matrix", workspace, 8);
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    DynArgs c = {};
    c.vals = vals, c.idx = idx, c.seg = seg, c.weight = weight;
    c.n_rows = n_rows, c.k = k, c.hidden = hidden;
    c.cu = (float*)(ws + w.cu), c.cf = (int32_t*)(ws + w.cf), c.nrm = (double*)(ws + w.nrm), c.act = (int32_t*)(ws + w.act);
    dyn_canon_kernel<<<dyn_canon_grid(n_rows), DY_BLOCK, 0, st>>>(c);
    WSAE_LAUNCH_CHECK();
    DtwArgs a = {};
    a.cu = c.cu, a.cf = c.cf, a.nrm = c.nrm, a.act = c.act, a.n_rows = n_rows;
    a.a_start = a_start, a.a_len = a_len, a.b_start = b_start, a.b_len = b_len;
    a.n_a = n_a, a.n_b = n_b, a.k = k, a.buckets = dtw_buckets(k), a.normalize = normalize != 0;
    a.dist = dist, a.steps = steps, a.ldd = ldd;
    const dim3 grid((unsigned)ceil_div(n_b, DT_GROUP), (unsigned)(n_a < DT_MAX_Y ? n_a : DT_MAX_Y));
    const size_t lds = dtw_lds_bytes(k);  // (sized by k: 36 KiB at k = 32, 60 KiB at k = 128)
    if (metric == WSAE_DTW_JACCARD) {
        dtw_kernel<true><<<grid, DT_BLOCK, lds, st>>>(a);
    } else {
        dtw_kernel<false><<<grid, DT_BLOCK, lds, st>>>(a);
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_abx_workspace_bytes(int32_t n_items, int32_t n_x, int32_t n_cats) {
    return abx_args_ok(n_items, n_x, n_cats) ? align256(4 * (int64_t)n_items * n_x) : -1;
}

extern "C" int wsae_abx_count(const float* dist, int64_t ldd, int32_t x_lo, int32_t n_x, int32_t n_items, const int32_t* cat,
                              const int32_t* ctx, const int32_t* spk, int32_t n_cats, int32_t mode, int64_t* wins2,
                              int64_t* total, int64_t* skipped, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(n_items >= 0 && n_x >= 0 && x_lo >= 0 && (int64_t)x_lo + n_x <= n_items,
                 "wsae_abx_count: the window [%d, %d + %d) is outside the %d items", x_lo, x_lo, n_x, n_items);
    WSAE_REQUIRE(n_cats >= 1 && n_cats <= WSAE_ABX_MAX_CATS, "wsae_abx_count: need 1 <= n_cats <= %d (got %d)",
                 WSAE_ABX_MAX_CATS, n_cats);
    WSAE_REQUIRE(mode == WSAE_ABX_ANY || mode == WSAE_ABX_WITHIN || mode == WSAE_ABX_ACROSS, "wsae_abx_count: unknown mode %d",
                 mode);
    WSAE_REQUIRE(ldd >= n_items, "wsae_abx_count: need ldd >= n_items = %d (got %lld)", n_items, (long long)ldd);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_abx_count: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    if (n_x == 0) return WSAE_OK;
    WSAE_REQUIRE(dist && cat && wins2 && total && skipped, "wsae_abx_count: null pointer");
    WSAE_REQUIRE(spk || mode == WSAE_ABX_ANY, "wsae_abx_count: WSAE_ABX_WITHIN and WSAE_ABX_ACROSS need spk (null pointer)");
    const int64_t need = align256(4 * (int64_t)n_items * n_x);
    WSAE_REQUIRE_WORKSPACE("wsae_abx_count", workspace, workspace_bytes, need, n_x);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_abx_count", workspace, 8);
    AbxArgs a = {};
    a.dist = dist, a.ldd = ldd, a.x_lo = x_lo, a.n_x = n_x, a.n_items = n_items, a.n_cats = n_cats, a.mode = mode;
    a.cat = cat, a.ctx = ctx, a.spk = mode == WSAE_ABX_ANY ? nullptr : spk;
    a.wins2 = (unsigned long long*)wins2, a.total = (unsigned long long*)total, a.skipped = (unsigned long long*)skipped;
    a.list = (int32_t*)workspace;
    abx_count_kernel<<<n_x, AX_BLOCK, 16 * (size_t)n_cats, (hipStream_t)stream>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
