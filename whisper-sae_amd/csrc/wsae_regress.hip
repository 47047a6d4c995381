// Sparse ridge regression: the sufficient statistics of a linear regression of a continuous
// per-frame target on the compact code, and the forward product that applies a fitted map.  The dense [frames, H] code
// never exists and no float is added with an atomic.
//
// wsae_gram_update: G[p][c] += sum over the rows on which columns p and c are both active of the product of their values,
// for c >= p.  gram_rows_kernel first writes, once per call, the column (or -1) and the value of every entry of the code
// into the workspace: the first-active test (probe_row_columns) and col_of are paid once per row, not once per visit -
// a row is visited once per active column.  The rows of column p come from the transposed plan of wsae_probe_plan; a
// workgroup owns column p, each of its GR_WAVES waves takes another chunk of WSAE_PROBE_CHUNK entries of p's list and walks
// its rows IN LIST ORDER: the row's (column, value) pairs are loaded one lane per entry, and every lane adds its product to
// the cell of its column in the wave's own LDS row of fp64 accumulators.  The columns of one row are distinct, so the lanes never meet in a cell, and the LDS operations of one
// wave execute in order, so a cell is ONE chain of additions in list order.  After a round of GR_WAVES chunks all threads add
// the waves' rows to their running cells in chunk order; a cell is read from G once and written once.  More columns than
// an LDS row holds: the columns are tiled and the list is walked once per tile from the one that holds p.
//
// wsae_regress_forward: a wave owns WSAE_PROBE_CHUNK consecutive rows and 64 targets (lanes as targets) and walks the rows in
// order.  pred = bias, then per first-active entry with a column, in ascending position, an fp64 multiply and an fp64
// add (not fused: contraction is off in this file).  The five sums of a used row go into five fp64 chains kept in
// registers; the chunk's partials are stored, and regress_stats_sum_kernel adds them to the stored value in chunk order.
#include "wsae_codewalk.h"

// every fp64 multiply and add below rounds on its own, as the numpy loops of the tests do
#pragma clang fp contract(off)

namespace {

constexpr int GR_WAVES = 8;               // waves of a Gram workgroup: chunks of one column in flight
constexpr int GR_BLOCK = GR_WAVES * 64;
constexpr int GR_TILE_WIDE = 2048;        // columns of an LDS row: 8 waves x 2048 x 8 B = 128 KB of the CU's 160 KB
constexpr int GR_TILE_MID = 1024;         // n_cols <= 1024: 64 KB, two workgroups per CU
constexpr int GR_TILE_NARROW = 512;       // n_cols <= 512: 32 KB, four workgroups per CU
constexpr int GR_MAX_BLOCKS = 2048;       // more columns in the window: the grid-stride loop
constexpr int GR_CANON_BLOCK = 256;       // the row front end: four waves, a row each
constexpr int GR_CANON_MAX_BLOCKS = 4096;
constexpr int GR_ROWS = 8;                // rows of the code whose loads are issued before the first of them is added
constexpr int RF_FB = 8;                  // entries of a row whose weight rows are loaded before the first of them is added
constexpr int RF_MAX_BLOCKS = 1 << 20;
constexpr int RG_CHUNK = WSAE_PROBE_CHUNK;
constexpr int RF_STATS = 5;

static_assert(GR_TILE_WIDE % GR_BLOCK == 0 && GR_TILE_MID % GR_BLOCK == 0 && GR_TILE_NARROW % GR_BLOCK == 0,
              "a tile is a whole number of block passes");

// ---- the Gram matrix --------------------------------------------------------------------------------------------------------
struct GramArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;
    const int32_t* col_of;
    const int64_t* col_ptr;
    const int32_t* t_row;
    const float* t_val;
    double* G;
    int32_t* ccol;  // workspace [n_rows, k]: the column of every entry, -1 where it has none (gram_rows_kernel)
    float* cval;    // workspace [n_rows, k]: its value
    int64_t n_rows, cap, ldg;
    int k, hidden, n_cols, p_lo, p_rows;
};

// One chunk [b, e) of column p's list into the wave's LDS row: the cells of the columns lo .. hi - 1 (lo >= p), cell of
// column c at acc[c - c_lo].  Called by a whole wave.
__device__ __forceinline__ void gram_walk_chunk(const GramArgs& a, int p, int64_t b, int64_t e, int c_lo, int lo, int hi,
                                                lds_f64* acc, int lane) {
    for (int64_t i0 = b; i0 < e; i0 += 64) {
        int er = -1, ev = 0;  // 64 entries of the list, one per lane
        if (i0 + lane < e) {
            er = a.t_row[i0 + lane];
            ev = __float_as_int(a.t_val[i0 + lane]);
        }
        const int n = (int)min64(64, e - i0);
        for (int u0 = 0; u0 < n; u0 += GR_ROWS) {
            float v0[GR_ROWS], v1[GR_ROWS];
            int c0[GR_ROWS], c1[GR_ROWS];
#pragma unroll
            for (int u = 0; u < GR_ROWS; ++u) {
                const int r = u0 + u < n ? __builtin_amdgcn_readlane(er, (u0 + u) & 63) : -1;
                const bool have = r >= 0 && r < a.n_rows;  // (a row outside the call is skipped, never read)
                v0[u] = 0.f, v1[u] = 0.f, c0[u] = -1, c1[u] = -1;
                if (have) probe_load_row(a.cval, a.ccol, a.k, r, lane, v0[u], c0[u], v1[u], c1[u]);
            }
#pragma unroll
            for (int u = 0; u < GR_ROWS; ++u) {
                if (u0 + u >= n) break;  // (wave-uniform)
                const int col0 = c0[u], col1 = c1[u];  // (-1 on a padding row and where the entry has no column)
                const double x = (double)__int_as_float(__builtin_amdgcn_readlane(ev, (u0 + u) & 63));
                if (col0 >= lo && col0 < hi) {  // (on the diagonal the row's value is the list's own)
                    const double y = col0 == p ? x : (double)v0[u];
                    acc[col0 - c_lo] = acc[col0 - c_lo] + x * y;  // (the product is exact in fp64)
                }
                if (col1 >= lo && col1 < hi) {
                    const double y = col1 == p ? x : (double)v1[u];
                    acc[col1 - c_lo] = acc[col1 - c_lo] + x * y;
                }
            }
        }
    }
}

// The row front end, once per call: the column of every entry where it is the first active entry of its feature on a
// non-padding row and the feature has a column (else -1), and its value.  A row is visited once per active column by the
// walk below, which then needs neither the first-active test nor col_of.
__global__ __launch_bounds__(GR_CANON_BLOCK) void gram_rows_kernel(GramArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (GR_CANON_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (GR_CANON_BLOCK / 64);
    for (int64_t r = wave; r < a.n_rows; r += n_waves) {
        const int sg = __builtin_amdgcn_readfirstlane(a.seg ? a.seg[r] : 0);
        float v0, v1;
        int f0, f1, col0 = -1, col1 = -1;
        probe_load_row(a.vals, a.idx, a.k, r, lane, v0, f0, v1, f1);
        if (sg >= 0) probe_row_columns(v0, f0, v1, f1, a.k, a.hidden, a.col_of, lane, col0, col1);  // (wave-uniform)
        if (lane < a.k) {
            a.ccol[r * a.k + lane] = col0;
            a.cval[r * a.k + lane] = v0;
        }
        if (lane + 64 < a.k) {
            a.ccol[r * a.k + lane + 64] = col1;
            a.cval[r * a.k + lane + 64] = v1;
        }
    }
}

template <int TILE>
__global__ __launch_bounds__(GR_BLOCK) void gram_kernel(GramArgs a) {
    __shared__ double gr_smem[GR_WAVES * TILE];
    lds_f64* all = (lds_f64*)gr_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    lds_f64* acc = all + wave * TILE;
    constexpr int PER = TILE / GR_BLOCK;  // cells of a tile per thread
    for (int pp = blockIdx.x; pp < a.p_rows; pp += gridDim.x) {
        const int p = a.p_lo + pp;
        const int64_t beg = min64(a.col_ptr[p], a.cap), end = min64(a.col_ptr[p + 1], a.cap);
        if (end <= beg) continue;  // a column without entries touches nothing (block-uniform)
        const int64_t n_chunks = (end - beg + RG_CHUNK - 1) / RG_CHUNK;
        double* grow = a.G + (int64_t)pp * a.ldg;
        for (int c_lo = (p / TILE) * TILE; c_lo < a.n_cols; c_lo += TILE) {
            const int hi = c_lo + TILE < a.n_cols ? c_lo + TILE : a.n_cols;
            const int lo = p > c_lo ? p : c_lo;
            double run[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int c = c_lo + j * GR_BLOCK + tid;
                run[j] = (c >= lo && c < hi) ? grow[c] : 0.0;
            }
            for (int64_t q0 = 0; q0 < n_chunks; q0 += GR_WAVES) {
                const int64_t q = q0 + wave;
                if (q < n_chunks) {  // (wave-uniform)
                    for (int c = lo - c_lo + lane; c < hi - c_lo; c += 64) acc[c] = 0.0;
                    const int64_t b = beg + q * RG_CHUNK;
                    gram_walk_chunk(a, p, b, min64(b + RG_CHUNK, end), c_lo, lo, hi, acc, lane);
                }
                __syncthreads();
                const int nw = (int)min64(GR_WAVES, n_chunks - q0);
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int c = c_lo + j * GR_BLOCK + tid;
                    if (c >= lo && c < hi)
                        for (int w = 0; w < nw; ++w) run[j] = run[j] + all[w * TILE + (c - c_lo)];  // chunk order
                }
                __syncthreads();  // the rows are read before the next round clears them
            }
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int c = c_lo + j * GR_BLOCK + tid;
                if (c >= lo && c < hi) grow[c] = run[j];
            }
        }
    }
}

// ---- the forward product ----------------------------------------------------------------------------------------------------
struct RfArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;
    const float* Y;
    const int32_t* col_of;
    const double* W;
    const double* bias;
    float* pred;
    unsigned long long* n_used;
    int64_t n_rows, ldy, ldw, ldp;
    int k, hidden, lag, C;
};

// the entries of `mask` (bits of the lanes whose col is a column), RF_FB at a time, in ascending position
__device__ __forceinline__ double regress_add_entries(unsigned long long mask, float v, int col, const RfArgs& a, int c, bool has_c,
                                                      double pr) {
    const int vb = __float_as_int(v);
    while (mask) {
        float ev[RF_FB];
        int ec[RF_FB];
#pragma unroll
        for (int u = 0; u < RF_FB; ++u) {
            ev[u] = 0.f;
            ec[u] = -1;
            if (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                ev[u] = __int_as_float(__builtin_amdgcn_readlane(vb, j));
                ec[u] = __builtin_amdgcn_readlane(col, j);
            }
        }
        double w[RF_FB];
#pragma unroll
        for (int u = 0; u < RF_FB; ++u) w[u] = (ec[u] >= 0 && has_c) ? a.W[(int64_t)ec[u] * a.ldw + c] : 0.0;
#pragma unroll
        for (int u = 0; u < RF_FB; ++u) {
            if (ec[u] < 0) continue;  // (wave-uniform)
            pr = pr + (double)ev[u] * w[u];  // (two roundings: contraction is off in this file)
        }
    }
    return pr;
}

__device__ __forceinline__ bool rf_finite(float x) { return (__float_as_int(x) & 0x7f800000) != 0x7f800000; }

// part [row chunks][RF_STATS][C]: the chains of a chunk's used rows, started at 0
__global__ __launch_bounds__(64) void regress_forward_kernel(RfArgs a, int c_tiles, int64_t n_chunks, double* __restrict__ part) {
    const int lane = threadIdx.x;
    const int64_t n_jobs = n_chunks * c_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int64_t ch = job / c_tiles;
        const int tile = (int)(job - ch * c_tiles);
        const int c = tile * 64 + lane;
        const bool has_c = c < a.C;
        const double b = has_c ? a.bias[c] : 0.0;
        const int64_t r_lo = ch * RG_CHUNK, r_hi = min64(r_lo + RG_CHUNK, a.n_rows);
        double s_y = 0.0, s_yy = 0.0, s_p = 0.0, s_pp = 0.0, s_e = 0.0;
        unsigned long long used = 0;
        // the segment and the entries of the next row are requested before the wave works on the current one
        float nv0, nv1;
        int nf0, nf1;
        int nseg = a.seg ? a.seg[r_lo] : 0;  // (made scalar where it is used: the request is not waited for here)
        probe_load_row(a.vals, a.idx, a.k, r_lo, lane, nv0, nf0, nv1, nf1);
        for (int64_t r = r_lo; r < r_hi; ++r) {
            const int seg_r = __builtin_amdgcn_readfirstlane(nseg);
            const float v0 = nv0, v1 = nv1;
            const int f0 = nf0, f1 = nf1;
            if (r + 1 < r_hi) {
                nseg = a.seg ? a.seg[r + 1] : 0;
                probe_load_row(a.vals, a.idx, a.k, r + 1, lane, nv0, nf0, nv1, nf1);
            }
            // the row's target and its segment are requested before the weight rows
            const int64_t q = r + a.lag;
            const bool q_in = a.Y && seg_r >= 0 && q >= 0 && q < a.n_rows;  // (wave-uniform)
            int seg_q = seg_r;
            float y32 = 0.f;
            if (q_in) {
                if (a.seg) seg_q = a.seg[q];
                if (has_c) y32 = a.Y[q * a.ldy + c];
            }
            if (seg_r < 0) {  // padding: exact zeros, and it counts nowhere
                if (a.pred && has_c) a.pred[r * a.ldp + c] = 0.f;
                continue;
            }
            int col0, col1;
            probe_row_columns(v0, f0, v1, f1, a.k, a.hidden, a.col_of, lane, col0, col1);
            double pr = regress_add_entries(__ballot(col0 >= 0), v0, col0, a, c, has_c, b);
            if (a.k > 64) pr = regress_add_entries(__ballot(col1 >= 0), v1, col1, a, c, has_c, pr);
            if (a.pred && has_c) a.pred[r * a.ldp + c] = (float)pr;
            if (!q_in || __builtin_amdgcn_readfirstlane(seg_q) != seg_r) continue;  // (wave-uniform)
            bool bad = !rf_finite(y32);  // all the targets of the row are finite, not only this tile's
            for (int t = 0; t < c_tiles; ++t) {
                const int ct = t * 64 + lane;
                if (t != tile && ct < a.C) bad |= !rf_finite(a.Y[q * a.ldy + ct]);
            }
            if (__ballot(bad)) continue;
            const double y = (double)y32, d = y - pr;
            s_y = s_y + y;
            s_yy = s_yy + y * y;
            s_p = s_p + pr;
            s_pp = s_pp + pr * pr;
            s_e = s_e + d * d;
            used += 1;
        }
        if (a.Y) {
            if (has_c) {
                double* out = part + ch * RF_STATS * a.C + c;
                out[0] = s_y;
                out[(int64_t)a.C] = s_yy;
                out[2 * (int64_t)a.C] = s_p;
                out[3 * (int64_t)a.C] = s_pp;
                out[4 * (int64_t)a.C] = s_e;
            }
            if (tile == 0 && lane == 0 && used) atomicAdd(a.n_used, used);
        }
    }
}

// stats[s][c] = ((stored + partial_0) + partial_1) + ...
__global__ __launch_bounds__(64) void regress_stats_sum_kernel(const double* __restrict__ part, int C, int64_t n_chunks,
                                                               double* __restrict__ stats) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= RF_STATS * C) return;
    double x = stats[i];
#pragma unroll 8
    for (int64_t ch = 0; ch < n_chunks; ++ch) x = x + part[ch * RF_STATS * C + i];
    stats[i] = x;
}

int64_t gram_ws_half(int64_t n_rows, int k) { return align256(4 * n_rows * k); }  // ccol, then cval

int64_t forward_ws_bytes(int64_t n_rows, int C) { return align256(8 * ceil_div64(n_rows, RG_CHUNK) * RF_STATS * C); }

}  // namespace

extern "C" int64_t wsae_gram_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols, int32_t p_rows,
                                             int64_t cap) {
    return column_code_ok(n_rows, k, hidden, n_cols) && n_cols <= WSAE_GRAM_MAX_COLS && p_rows >= 1 && p_rows <= n_cols &&
                   cap >= 0
               ? 2 * gram_ws_half(n_rows, k)
               : -1;
}

extern "C" int wsae_gram_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                int64_t n_rows, const int32_t* col_of, int32_t n_cols, const int64_t* col_ptr,
                                const int32_t* t_row, const float* t_val, int64_t cap, int32_t p_lo, int32_t p_rows, double* G,
                                int64_t ldg, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && col_ptr && G, "wsae_gram_update: null pointer");
    CW_REQUIRE_COLUMN_CODE("wsae_gram_update", k, hidden, n_rows, col_of, n_cols);
    WSAE_REQUIRE(n_cols <= WSAE_GRAM_MAX_COLS, "wsae_gram_update: need n_cols <= %d (got %d)", WSAE_GRAM_MAX_COLS, n_cols);
    CW_REQUIRE_LISTS("wsae_gram_update", cap, t_row, t_val);
    WSAE_REQUIRE(p_lo >= 0 && p_rows >= 1 && (int64_t)p_lo + p_rows <= n_cols,
                 "wsae_gram_update: the row window [%d, %d + %d) is outside [0, %d)", p_lo, p_lo, p_rows, n_cols);
    WSAE_REQUIRE(ldg >= n_cols, "wsae_gram_update: ldg %lld is smaller than the %d columns", (long long)ldg, n_cols);
    const int64_t half = gram_ws_half(n_rows, k);
    WSAE_REQUIRE_WORKSPACE("wsae_gram_update", workspace, workspace_bytes, 2 * half, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_gram_update", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    GramArgs a = {vals, idx, seg, col_of, col_ptr, t_row, t_val, G, (int32_t*)workspace, (float*)((char*)workspace + half),
                  n_rows, cap, ldg, k, hidden, n_cols, p_lo, p_rows};
    const int grid = p_rows < GR_MAX_BLOCKS ? p_rows : GR_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    const int64_t row_blocks = ceil_div64(n_rows, GR_CANON_BLOCK / 64);
    gram_rows_kernel<<<(int)(row_blocks < GR_CANON_MAX_BLOCKS ? row_blocks : GR_CANON_MAX_BLOCKS), GR_CANON_BLOCK, 0, st>>>(a);
    if (n_cols <= GR_TILE_NARROW) gram_kernel<GR_TILE_NARROW><<<grid, GR_BLOCK, 0, st>>>(a);
    else if (n_cols <= GR_TILE_MID) gram_kernel<GR_TILE_MID><<<grid, GR_BLOCK, 0, st>>>(a);
    else gram_kernel<GR_TILE_WIDE><<<grid, GR_BLOCK, 0, st>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_regress_forward_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols,
                                                        int32_t n_targets, int32_t lag) {
    return column_code_ok(n_rows, k, hidden, n_cols) && n_targets >= 1 && n_targets <= WSAE_PROBE_MAX_CLASSES && lag_ok(lag)
               ? forward_ws_bytes(n_rows, n_targets)
               : -1;
}

extern "C" int wsae_regress_forward(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                    const float* Y, int64_t ldy, int64_t n_rows, int32_t lag, int32_t n_targets,
                                    const int32_t* col_of, int32_t n_cols, const double* W, int64_t ldw, const double* bias,
                                    float* pred, int64_t ldp, int64_t* n_used, double* stats, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && W && bias, "wsae_regress_forward: null pointer");
    CW_REQUIRE_COLUMN_CODE("wsae_regress_forward", k, hidden, n_rows, col_of, n_cols);
    WSAE_REQUIRE(n_targets >= 1 && n_targets <= WSAE_PROBE_MAX_CLASSES, "wsae_regress_forward: need 1 <= n_targets <= %d (got %d)",
                 WSAE_PROBE_MAX_CLASSES, n_targets);
    CW_REQUIRE_LAG("wsae_regress_forward", lag);
    WSAE_REQUIRE(ldw >= n_targets, "wsae_regress_forward: ldw %lld is smaller than the %d targets", (long long)ldw, n_targets);
    WSAE_REQUIRE(!pred || ldp >= n_targets, "wsae_regress_forward: ldp %lld is smaller than the %d targets", (long long)ldp,
                 n_targets);
    WSAE_REQUIRE(Y || pred, "wsae_regress_forward: without Y and without pred there is nothing to compute");
    WSAE_REQUIRE(!Y || (ldy >= n_targets && n_used && stats),
                 "wsae_regress_forward: Y needs ldy >= the %d targets (got %lld), n_used and stats", n_targets, (long long)ldy);
    const int64_t need = Y ? forward_ws_bytes(n_rows, n_targets) : 0;
    WSAE_REQUIRE(workspace_bytes >= need && (workspace || need == 0 || n_rows == 0),
                 "wsae_regress_forward: workspace too small (%lld < %lld)", (long long)(workspace ? workspace_bytes : 0),
                 (long long)need);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_regress_forward", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    RfArgs a = {vals, idx, seg, Y, col_of, W, bias, pred, (unsigned long long*)n_used, n_rows, ldy, ldw, ldp, k, hidden, lag,
                n_targets};
    const int c_tiles = ceil_div(n_targets, 64);
    const int64_t n_chunks = ceil_div64(n_rows, RG_CHUNK);
    const int64_t jobs = n_chunks * c_tiles;
    hipStream_t st = (hipStream_t)stream;
    regress_forward_kernel<<<(int)(jobs < RF_MAX_BLOCKS ? jobs : RF_MAX_BLOCKS), 64, 0, st>>>(a, c_tiles, n_chunks,
                                                                                              (double*)workspace);
    if (Y) regress_stats_sum_kernel<<<ceil_div(RF_STATS * n_targets, 64), 64, 0, st>>>((const double*)workspace, n_targets,
                                                                                       n_chunks, stats);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
