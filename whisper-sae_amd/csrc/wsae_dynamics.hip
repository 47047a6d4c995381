// Code dynamics: how the code of a frame as a whole moves through time.
//
// wsae_dyn_update: the similarity (cosine, dot, Jaccard) of the codes of rows r and r + lag for up to 16 lags, as a
// [rows, lags] matrix and / or as integer statistics per (lag, label class).  Two launches.  dyn_canon_kernel
// (wsae_dyn_canon.h, shared with wsae_abx.hip), one wave
// per row on the front end of wsae_codewalk.h (one lane per entry, two for k > 64, the first active entry of a feature
// wins), writes the canonical code into the workspace: per entry u = v weight[f] and f, or -1 where the entry is not
// active, per row the norm and the number of active features.  dyn_sim_kernel, one wave per row r, keeps the canonical
// entries of r in its lanes and for every lag loads those of row q = r + lag the same way (re-reads that L2 serves); the
// entries of r are broadcast in ascending position (readlane), the lane of q that holds the same feature answers a
// ballot and its value is broadcast back, so every lane carries the one fp64 chain wsae.h states and no reduction tree
// is involved.  The statistics are integer sums, added up in LDS per workgroup first and handed to the state with one
// global atomic per touched cell at the end of the block.
//
// wsae_boundary_score: the precision / recall counts of a per-frame boundary curve against reference boundaries at up
// to 256 thresholds.  bd_flag_kernel (one thread per row) writes a flag byte per row - peak, reference, last row of its
// stretch - and appends the first row of every stretch to a list.  bd_walk_kernel gives a wave one stretch and 64
// thresholds, one per lane; all lanes walk the rows of the stretch together (64 rows per coalesced load, then a readlane
// per row) and each lane runs the greedy match for its own threshold as a stream: the items seen and not yet consumed
// are all predictions or all references, and only those of the last tol rows can still be hit, so they are a 64-bit
// mask of row ages plus one bit for their kind.  An item of the other kind hits the oldest of them.
#include <math.h>

#include "wsae_dyn_canon.h"

namespace {

constexpr int DY_CLASSES = 3;
constexpr int DY_CELLS = WSAE_DYN_MAX_LAGS * DY_CLASSES;

// One step of the chain: the entry (f, u) of row r, f >= 0 and the same in every lane, against the lanes of row q.
__device__ __forceinline__ void dyn_match(int f, float u, float qu0, int qf0, float qu1, int qf1, bool wide, double& s,
                                          int& inter) {
    const unsigned long long m0 = __ballot(qf0 == f);
    if (m0) {  // (row q holds a feature once: one bit)
        s += (double)u * (double)lane_f32(qu0, __builtin_ctzll(m0));
        ++inter;
        return;
    }
    if (!wide) return;
    const unsigned long long m1 = __ballot(qf1 == f);
    if (m1) {
        s += (double)u * (double)lane_f32(qu1, __builtin_ctzll(m1));
        ++inter;
    }
}

__global__ __launch_bounds__(DY_BLOCK) void dyn_sim_kernel(DynArgs a) {
    __shared__ unsigned int s_pairs[DY_CELLS];
    __shared__ unsigned long long s_simq[DY_CELLS];
    __shared__ unsigned long long s_sq[DY_CELLS];
    __shared__ unsigned int s_hist[DY_CELLS * WSAE_DYN_BINS];
    __shared__ unsigned int s_rows;
    const bool state = a.pairs != nullptr;
    const int cells = a.L * DY_CLASSES;
    if (state) {
        for (int i = threadIdx.x; i < cells; i += DY_BLOCK) s_pairs[i] = 0u, s_simq[i] = 0ull, s_sq[i] = 0ull;
        for (int i = threadIdx.x; i < cells * WSAE_DYN_BINS; i += DY_BLOCK) s_hist[i] = 0u;
        if (threadIdx.x == 0) s_rows = 0u;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (DY_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (DY_BLOCK / 64);
    const int k = a.k, k0 = k < 64 ? k : 64;
    const bool wide = k > 64;
    for (int64_t r = wave; r < a.n_rows; r += n_waves) {
        const int seg_r = a.seg != nullptr ? a.seg[r] : 0;
        const bool live = seg_r >= 0;
        float mine = __int_as_float(0x7fc00000);  // lane l: the similarity at lag l (NaN: no pair)
        if (live) {
            if (state && lane == 0) atomicAdd(&s_rows, 1u);
            float u0, u1;
            int f0, f1;
            dyn_load_canon(a, r, lane, u0, f0, u1, f1);
            const double n_r = a.nrm[r];
            const int a_r = a.act[r];
            const int lab_r = a.label != nullptr ? a.label[r] : -1;
            for (int l = 0; l < a.L; ++l) {
                const int64_t q = r + a.lag[l];
                if (q >= a.n_rows) break;  // (the lags ascend)
                if (a.seg != nullptr && a.seg[q] != seg_r) continue;
                float qu0, qu1;
                int qf0, qf1;
                dyn_load_canon(a, q, lane, qu0, qf0, qu1, qf1);
                double s = 0.0;
                int inter = 0;
                for (int d = 0; d < k0; ++d) {
                    const int f = __builtin_amdgcn_readlane(f0, d);
                    if (f >= 0) dyn_match(f, lane_f32(u0, d), qu0, qf0, qu1, qf1, wide, s, inter);
                }
                for (int d = 64; d < k; ++d) {
                    const int f = __builtin_amdgcn_readlane(f1, d - 64);
                    if (f >= 0) dyn_match(f, lane_f32(u1, d - 64), qu0, qf0, qu1, qf1, wide, s, inter);
                }
                double c;
                if (a.metric == WSAE_DYN_DOT) {
                    c = s;
                } else if (a.metric == WSAE_DYN_COSINE) {
                    const double n_q = a.nrm[q];
                    c = 0.0;
                    if (n_r != 0.0 && n_q != 0.0) {
                        c = s / sqrt(n_r * n_q);
                        if (!(c <= 1.0)) c = 1.0;
                    }
                } else {
                    const int uni = a_r + a.act[q] - inter;
                    c = uni != 0 ? (double)inter / (double)uni : 0.0;
                }
                const float res = (float)c;
                if (lane == l) mine = res;
                if (state && lane == 0) {
                    int cls = 2;
                    if (lab_r >= 0) {
                        const int lab_q = a.label[q];
                        if (lab_q >= 0) cls = lab_q == lab_r ? 0 : 1;
                    }
                    const long long x = llrint((double)res * 1073741824.0);
                    const int cell = l * DY_CLASSES + cls;
                    const long long bin = x >> 24;
                    atomicAdd(&s_pairs[cell], 1u);
                    atomicAdd(&s_simq[cell], (unsigned long long)x);
                    atomicAdd(&s_sq[cell], (unsigned long long)((x >> 15) * (x >> 15)));
                    atomicAdd(&s_hist[cell * WSAE_DYN_BINS + (int)(bin < 63 ? bin : 63)], 1u);
                }
            }
        }
        if (a.sim != nullptr && lane < a.L) a.sim[r * a.L + lane] = mine;
    }
    if (state) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += DY_BLOCK) {
            const unsigned int n = s_pairs[i];
            if (n) {
                atomicAdd(a.pairs + i, (unsigned long long)n);
                atomicAdd(a.sim_q + i, s_simq[i]);
                atomicAdd(a.sq_q + i, s_sq[i]);
            }
        }
        for (int i = threadIdx.x; i < cells * WSAE_DYN_BINS; i += DY_BLOCK) {
            const unsigned int n = s_hist[i];
            if (n) atomicAdd(a.hist + i, (unsigned long long)n);
        }
        if (threadIdx.x == 0 && s_rows) atomicAdd(a.total_rows, (unsigned long long)s_rows);
    }
}

inline bool dyn_args_ok(int64_t n_rows, int k, int hidden, int n_lags) {
    return n_rows >= 0 && n_rows <= INT_MAX && k >= 1 && k <= WSAE_DYN_MAX_K && hidden >= 1 && n_lags >= 1 &&
           n_lags <= WSAE_DYN_MAX_LAGS;
}

// ---- boundary scoring ------------------------------------------------------------------------------------------------------
constexpr int BD_BLOCK = 256;
constexpr int BD_MAX_BLOCKS = 2048;
constexpr int BD_WALK_BLOCKS = 512;  // at most 2048 waves per group of 64 thresholds walk the stretches
constexpr int BD_PEAK = 1, BD_REF = 2, BD_LAST = 4;

__global__ __launch_bounds__(BD_BLOCK) void bd_flag_kernel(const float* __restrict__ nov, const int32_t* __restrict__ seg,
                                                           const uint8_t* __restrict__ ref, int64_t n_rows,
                                                           uint8_t* __restrict__ code, int32_t* __restrict__ heads,
                                                           unsigned int* __restrict__ n_heads, uint8_t* __restrict__ peaks,
                                                           unsigned long long* n_ref, unsigned long long* n_peaks) {
    __shared__ unsigned int s_ref, s_peak;
    if (threadIdx.x == 0) s_ref = 0u, s_peak = 0u;
    __syncthreads();
    unsigned int my_ref = 0u, my_peak = 0u;
    for (int64_t r = (int64_t)blockIdx.x * BD_BLOCK + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * BD_BLOCK) {
        const int s = seg != nullptr ? seg[r] : 0;
        int c = 0;
        if (s >= 0) {
            const bool has_l = r > 0 && (seg == nullptr || seg[r - 1] == s);
            const bool has_r = r + 1 < n_rows && (seg == nullptr || seg[r + 1] == s);
            const float x = nov[r];
            float left = has_l ? nov[r - 1] : -INFINITY, right = has_r ? nov[r + 1] : -INFINITY;
            if (left != left) left = -INFINITY;
            if (right != right) right = -INFINITY;
            const bool peak = x > left && x >= right;  // (false for a NaN x)
            const bool is_ref = ref != nullptr && ref[r] != 0;
            c = (peak ? BD_PEAK : 0) | (is_ref ? BD_REF : 0) | (has_r ? 0 : BD_LAST);
            my_ref += is_ref;
            my_peak += peak;
            if (!has_l) heads[atomicAdd(n_heads, 1u)] = (int32_t)r;  // (at most one head per row: the list holds n_rows)
        }
        code[r] = (uint8_t)c;
        if (peaks != nullptr) peaks[r] = (uint8_t)(c & BD_PEAK);
    }
    if (my_ref) atomicAdd(&s_ref, my_ref);
    if (my_peak) atomicAdd(&s_peak, my_peak);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_ref) atomicAdd(n_ref, (unsigned long long)s_ref);
        if (s_peak) atomicAdd(n_peaks, (unsigned long long)s_peak);
    }
}

__global__ __launch_bounds__(BD_BLOCK) void bd_walk_kernel(const float* __restrict__ nov, const uint8_t* __restrict__ code,
                                                           const int32_t* __restrict__ heads,
                                                           const unsigned int* __restrict__ n_heads, int64_t n_rows,
                                                           const float* __restrict__ thr, int n_thr, int tol,
                                                           unsigned long long* n_pred, unsigned long long* n_hit) {
    __shared__ unsigned long long s_pred[64], s_hit[64];
    if (threadIdx.x < 64) s_pred[threadIdx.x] = 0ull, s_hit[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (BD_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (BD_BLOCK / 64);
    const int ti = blockIdx.y * 64 + lane;
    const float th = ti < n_thr ? thr[ti] : __int_as_float(0x7fc00000);  // (NaN: predicts nothing)
    const unsigned long long tol_mask = tol == 0 ? 0ull : (tol >= 64 ? ~0ull : (1ull << tol) - 1ull);  // ages 1 .. tol
    const int64_t nh = (int64_t)*n_heads;
    unsigned long long pred = 0ull, hit = 0ull;
    for (int64_t h = wave; h < nh; h += n_waves) {
        // pend: bit i = an item seen i + 1 rows ago waits for a partner; kind: 0 = the waiting items are predictions,
        // 1 = references; fresh: an item of this row waits (it enters pend with the next row)
        unsigned long long pend = 0ull;
        bool fresh = false;
        int kind = 0;
        bool done = false;
        for (int64_t base = heads[h]; !done; base += 64) {
            const int64_t rr = base + lane;
            const int c = rr < n_rows ? code[rr] : BD_LAST;  // (a stretch ends inside the call: never walked past it)
            const float x = rr < n_rows ? nov[rr] : 0.f;
            for (int j = 0; j < 64; ++j) {
                const int cj = __builtin_amdgcn_readlane(c, j);
                const float xj = lane_f32(x, j);
                pend = ((pend << 1) | (fresh ? 1ull : 0ull)) & tol_mask;
                const bool P = (cj & BD_PEAK) && xj >= th;
                const bool R = (cj & BD_REF) != 0;
                const bool both = P && R, any = P || R;
                const int y = R ? 1 : 0;  // (one item: its kind)
                const bool match = pend != 0ull && (both || (any && kind != y));  // the oldest waiting item is hit
                if (match) pend &= ~(1ull << (63 - __builtin_clzll(pend)));
                hit += (match || (both && !match)) ? 1ull : 0ull;  // (both, nothing waiting: they hit each other)
                fresh = both ? match : (any && !match);            // (both, after a hit: the item of the waiting kind stays)
                if (!both && any && !match) kind = y;
                pred += P ? 1ull : 0ull;
                if (cj & BD_LAST) {
                    done = true;
                    break;
                }
            }
        }
    }
    if (pred) atomicAdd(&s_pred[lane], pred);
    if (hit) atomicAdd(&s_hit[lane], hit);
    __syncthreads();
    if (threadIdx.x < 64 && ti < n_thr) {
        if (s_pred[lane]) atomicAdd(n_pred + ti, s_pred[lane]);
        if (s_hit[lane]) atomicAdd(n_hit + ti, s_hit[lane]);
    }
}

inline bool boundary_args_ok(int64_t n_rows, int n_thr, int tol) {
    return n_rows >= 0 && n_rows <= INT_MAX && n_thr >= 1 && n_thr <= WSAE_BOUNDARY_MAX_THR && tol >= 0 &&
           tol <= WSAE_BOUNDARY_MAX_TOL;
}

// the sections of the workspace of wsae_boundary_score: the counter, the flag bytes, the stretch list
struct BoundaryLayout {
    int64_t count, code, heads, total;
};
inline BoundaryLayout boundary_layout(int64_t n_rows) {
    BoundaryLayout w;
    w.count = 0;
    w.code = 256;
    w.heads = w.code + align256(n_rows);
    w.total = n_rows ? w.heads + align256(4 * n_rows) : 0;  // (no rows need none)
    return w;
}

}  // namespace

extern "C" int64_t wsae_dyn_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_lags) {
    return dyn_args_ok(n_rows, k, hidden, n_lags) ? dyn_layout(n_rows, k).total : -1;
}

extern "C" int wsae_dyn_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                               const float* weight, const int32_t* label, int64_t n_rows, const int32_t* lags, int32_t n_lags,
                               int32_t metric, float* sim, int64_t* pairs, int64_t* sim_q, int64_t* sq_q, int64_t* hist,
                               int64_t* total_rows, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && lags, "wsae_dyn_update: null pointer");
    CW_REQUIRE_K("wsae_dyn_update", k, WSAE_DYN_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_dyn_update", hidden);
    CW_REQUIRE_ROWS("wsae_dyn_update", n_rows);
    WSAE_REQUIRE(n_lags >= 1 && n_lags <= WSAE_DYN_MAX_LAGS, "wsae_dyn_update: need 1 <= n_lags <= %d (got %d)",
                 WSAE_DYN_MAX_LAGS, n_lags);
    for (int l = 0; l < n_lags; ++l) {
        WSAE_REQUIRE(lags[l] >= 1 && lags[l] <= WSAE_DYN_MAX_LAG && (l == 0 || lags[l] > lags[l - 1]),
                     "wsae_dyn_update: the lags must ascend within 1..%d (lag %d is %d)", WSAE_DYN_MAX_LAG, l, lags[l]);
    }
    WSAE_REQUIRE(metric == WSAE_DYN_COSINE || metric == WSAE_DYN_DOT || metric == WSAE_DYN_JACCARD,
                 "wsae_dyn_update: unknown metric %d", metric);
    const bool any_state = pairs || sim_q || sq_q || hist || total_rows;
    WSAE_REQUIRE(!any_state || (pairs && sim_q && sq_q && hist && total_rows),
                 "wsae_dyn_update: the state needs pairs, sim_q, sq_q, hist and total_rows (null pointer)");
    WSAE_REQUIRE(!any_state || metric != WSAE_DYN_DOT,
                 "wsae_dyn_update: the state holds similarities in [0, 1]: WSAE_DYN_DOT has none");
    WSAE_REQUIRE(sim || any_state, "wsae_dyn_update: neither sim nor a state to write");
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_dyn_update: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    const DynLayout w = dyn_layout(n_rows, k);
    WSAE_REQUIRE_WORKSPACE("wsae_dyn_update", workspace, workspace_bytes, w.total, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_dyn_update", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    char* ws = (char*)workspace;
    DynArgs a = {};
    a.vals = vals, a.idx = idx, a.seg = seg, a.weight = weight, a.label = label;
    a.n_rows = n_rows, a.k = k, a.hidden = hidden, a.L = n_lags, a.metric = metric;
    for (int l = 0; l < n_lags; ++l) a.lag[l] = lags[l];
    a.cu = (float*)(ws + w.cu), a.cf = (int32_t*)(ws + w.cf), a.nrm = (double*)(ws + w.nrm), a.act = (int32_t*)(ws + w.act);
    a.sim = sim;
    a.pairs = (unsigned long long*)pairs, a.sim_q = (unsigned long long*)sim_q, a.sq_q = (unsigned long long*)sq_q;
    a.hist = (unsigned long long*)hist, a.total_rows = (unsigned long long*)total_rows;
    const int grid = dyn_canon_grid(n_rows);
    dyn_canon_kernel<<<grid, DY_BLOCK, 0, (hipStream_t)stream>>>(a);
    WSAE_LAUNCH_CHECK();
    dyn_sim_kernel<<<grid, DY_BLOCK, 0, (hipStream_t)stream>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_boundary_workspace_bytes(int64_t n_rows, int32_t n_thr, int32_t tol) {
    return boundary_args_ok(n_rows, n_thr, tol) ? boundary_layout(n_rows).total : -1;
}

extern "C" int wsae_boundary_score(const float* nov, const int32_t* seg, const uint8_t* ref, int64_t n_rows, const float* thr,
                                   int32_t n_thr, int32_t tol, int64_t* n_pred, int64_t* n_hit, int64_t* n_ref,
                                   int64_t* n_peaks, uint8_t* peaks, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(nov && thr && n_pred && n_hit && n_ref && n_peaks, "wsae_boundary_score: null pointer");
    CW_REQUIRE_ROWS("wsae_boundary_score", n_rows);
    WSAE_REQUIRE(n_thr >= 1 && n_thr <= WSAE_BOUNDARY_MAX_THR, "wsae_boundary_score: need 1 <= n_thr <= %d (got %d)",
                 WSAE_BOUNDARY_MAX_THR, n_thr);
    WSAE_REQUIRE(tol >= 0 && tol <= WSAE_BOUNDARY_MAX_TOL, "wsae_boundary_score: need 0 <= tol <= %d (got %d)",
                 WSAE_BOUNDARY_MAX_TOL, tol);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_boundary_score: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    const BoundaryLayout w = boundary_layout(n_rows);
    WSAE_REQUIRE_WORKSPACE("wsae_boundary_score", workspace, workspace_bytes, w.total, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_boundary_score", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    char* ws = (char*)workspace;
    unsigned int* count = (unsigned int*)(ws + w.count);
    uint8_t* code = (uint8_t*)(ws + w.code);
    int32_t* heads = (int32_t*)(ws + w.heads);
    hipStream_t st = (hipStream_t)stream;
    WSAE_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned int), st));
    const int64_t blocks = ceil_div64(n_rows, BD_BLOCK);
    bd_flag_kernel<<<(int)(blocks < BD_MAX_BLOCKS ? blocks : BD_MAX_BLOCKS), BD_BLOCK, 0, st>>>(
        nov, seg, ref, n_rows, code, heads, count, peaks, (unsigned long long*)n_ref, (unsigned long long*)n_peaks);
    WSAE_LAUNCH_CHECK();
    // a wave per stretch: no more waves than 64-row pieces, which bounds the stretches worth a wave of their own
    const int64_t want = ceil_div64(ceil_div64(n_rows, 64), BD_BLOCK / 64);
    const dim3 grid((unsigned)(want < BD_WALK_BLOCKS ? want : BD_WALK_BLOCKS), (unsigned)ceil_div(n_thr, 64));
    bd_walk_kernel<<<grid, BD_BLOCK, 0, st>>>(nov, code, heads, count, n_rows, thr, n_thr, tol, (unsigned long long*)n_pred,
                                              (unsigned long long*)n_hit);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
