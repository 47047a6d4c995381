// Feature-triggered averages of a per-frame signal: what is in the input when a feature fires?
//
// For every trigger (row r, feature f, weight w) and every lag l of the call, acc[f][l][c] += w * y[r + l][c] in fp64,
// wsum[f][l] += w and cnt[f][l] += 1, where row r + l exists and belongs to the segment of r.  Each of these cells is one
// chain of fp64 additions in ascending trigger row, so nothing here adds with atomics and nothing splits a chain.
// Four launches.
//   1. sta_walk_kernel<false>: a single-wave workgroup owns (chunk of consecutive rows, tile of features), walks its rows
//      in order, one lane per entry, and counts the triggers of each tile feature in LDS; the counts become one row of the
//      [chunks, f_cols] table.  The per-feature "last seen on row" cell gives both "an index repeated within a row counts
//      once" and the onset rule (a chunk first looks at the row in front of it, without counting).
//   2. chunk_scan_kernel (wsae_lists.h): per feature the exclusive prefix over the chunks (feature-major, chunk-minor)
//      and its total.  sta_offsets_kernel (one workgroup, list_offsets of wsae_lists.h with the policy StaOffsets): the
//      exclusive prefix of the totals, and the features ordered by the length of their lists, long ones first (33 classes
//      by the position of the leading bit; the order inside a class is free and changes no result).
//   3. sta_walk_kernel<true>: the same walk, now taking slots from LDS cursors that start at the scanned positions: the
//      list of a feature holds (row, weight) in ascending row.  A stable counting sort; the trigger rules are applied here.
//   4. sta_accum_kernel: a single-wave workgroup owns (feature, tile of 64 channels); lane = channel, the L accumulators
//      of the lane stay in registers.  It walks the SIGNAL rows the feature's triggers reach, eight at a time (their loads
//      issued together): a row is loaded once and applied to every lag that has a trigger at row - lag.  The triggers of
//      the last L rows sit in a 128-slot LDS ring (row, weight, segment); lane j looks at the slot of lag j, a ballot gives
//      the lags that have a term, and the weight of lag j reaches the other lanes by v_readlane.  wsum and cnt of lag j
//      are kept by lane j of the feature's first channel tile.
// The chunking of the rows, the scan and the body of the offsets kernel are shared with wsae_probe.hip (wsae_lists.h); the
// walk and its trigger rules are this file's.
#include <limits.h>

#include "wsae_lists.h"

namespace {

constexpr int ST_TILE = 4096;        // features per walk job: 16 KB of rows + 4 KB of tags + 16 / 32 KB of counts / cursors
constexpr int ST_MAX_BLOCKS = 1 << 20;
constexpr int ST_ROWS = 4;           // rows of the code whose loads are issued before the first of them is processed
constexpr int ST_RB = 8;             // signal rows per block of the accumulation
constexpr int ST_RING = 128;         // slots of the trigger ring (>= WSAE_STA_MAX_LAGS + ST_RB)
constexpr int ST_NEVER = INT_MIN + 1000;  // a ring slot that holds no trigger

struct StaWalk {
    lds_i32* seen;  // the row the feature was last seen on, -2 = not yet
    lds_i32* cnt;   // (count) triggers of the chunk
    lds_u64* cur;   // (scatter) the next slot of the feature's list
    lds_u8* tag;
    int32_t* ent_row;
    float* ent_w;
    bool onset, one;
};

// one entry (column c of the tile, value v) on row r; prev_same: row r - 1 exists and has the segment of r
template <bool SCATTER>
__device__ __forceinline__ void sta_entry(bool act, int c, float v, int r, bool prev_same, bool counting, const StaWalk& t) {
    if (!act) return;
    const int ls = t.seen[c];
    if (ls == r) return;  // an earlier entry of this row named the feature: it counts once, the first value stands
    t.seen[c] = r;
    if (!counting || (t.onset && ls == r - 1 && prev_same)) return;
    if (SCATTER) {
        const unsigned long long slot = t.cur[c];
        t.cur[c] = slot + 1ull;
        t.ent_row[slot] = r;
        t.ent_w[slot] = t.one ? 1.f : v;
    } else {
        t.cnt[c] = t.cnt[c] + 1;
    }
}

// one pass of at most 64 entries (lane = entry) of row r; two entries of a pass that name one column are replayed in
// entry order (a TopK code never has them)
template <bool SCATTER>
__device__ __forceinline__ void sta_pass(bool in, int c, float v, int r, bool prev_same, bool counting, const StaWalk& t,
                                         int lane) {
    if (in) t.tag[c] = (uint8_t)lane;
    const bool lost = in && t.tag[c] != (uint8_t)lane;
    if (__ballot(lost) == 0ull) {
        sta_entry<SCATTER>(in, c, v, r, prev_same, counting, t);
    } else {
        for (unsigned long long m = __ballot(in); m; m &= m - 1ull)
            sta_entry<SCATTER>(in && lane == __builtin_ctzll(m), c, v, r, prev_same, counting, t);
    }
}

// NP: passes of 64 entries per row (k <= 64 * NP).  table [n_chunks][f_cols]: written by the count, read (after the scan)
// by the scatter; base [f_cols]: the first slot of every feature's list.
template <bool SCATTER, int NP>
__global__ __launch_bounds__(64) void sta_walk_kernel(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k,
                                                      const int32_t* __restrict__ seg, int64_t n_rows, int64_t chunk_rows,
                                                      int n_chunks, int f_lo, int f_cols, int n_tiles, int onset, int one,
                                                      int32_t* __restrict__ table, const int64_t* __restrict__ base,
                                                      int32_t* __restrict__ ent_row, float* __restrict__ ent_w) {
    extern __shared__ float st_smem[];
    StaWalk t;
    t.seen = (lds_i32*)st_smem;
    t.tag = (lds_u8*)(st_smem + ST_TILE);
    t.cnt = (lds_i32*)(st_smem + ST_TILE + ST_TILE / 4);
    t.cur = (lds_u64*)(st_smem + ST_TILE + ST_TILE / 4);  // (8-byte aligned: 20480 bytes in)
    t.ent_row = ent_row;
    t.ent_w = ent_w;
    t.onset = onset != 0;
    t.one = one != 0;
    const int lane = threadIdx.x;
    const int64_t n_jobs = (int64_t)n_chunks * n_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int ch = (int)(job / n_tiles), tl = (int)(job - (int64_t)ch * n_tiles);
        const int c_lo = tl * ST_TILE;
        const int width = f_cols - c_lo < ST_TILE ? f_cols - c_lo : ST_TILE;
        const int t_lo = f_lo + c_lo;
        const int64_t r_lo = (int64_t)ch * chunk_rows;
        const int64_t r_hi = r_lo + chunk_rows < n_rows ? r_lo + chunk_rows : n_rows;  // exclusive
        int32_t* trow = table + (int64_t)ch * f_cols + c_lo;
        for (int c = lane; c < width; c += 64) {
            t.seen[c] = -2;
            if (SCATTER) t.cur[c] = (unsigned long long)(base[c_lo + c] + (int64_t)trow[c]);
            else t.cnt[c] = 0;
        }
        // with the onset rule the chunk first looks at the row in front of it: who was active there?
        const int64_t r_first = (t.onset && r_lo > 0) ? r_lo - 1 : r_lo;
        for (int64_t row = r_first; row < r_hi; row += ST_ROWS) {
            float v[ST_ROWS][NP];
            int ix[ST_ROWS][NP];
            int sg[ST_ROWS], sp[ST_ROWS];
#pragma unroll
            for (int u = 0; u < ST_ROWS; ++u) {
                const bool have = row + u < r_hi;
                const int64_t rr = have ? row + u : r_hi - 1;
                sg[u] = __builtin_amdgcn_readfirstlane(have ? (seg ? seg[rr] : 0) : -1);
                sp[u] = __builtin_amdgcn_readfirstlane(rr > 0 ? (seg ? seg[rr - 1] : 0) : -1);
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int e = p * 64 + lane;
                    v[u][p] = 0.f;
                    ix[u][p] = -1;
                    if (e < k) {
                        v[u][p] = vals[rr * k + e];
                        ix[u][p] = idx[rr * k + e];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < ST_ROWS; ++u) {
                if (sg[u] < 0) continue;  // a padding row (wave-uniform)
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int i = ix[u][p];
                    const bool in = v[u][p] > 0.f && i >= t_lo && i - t_lo < width;  // (t_lo + width <= hidden)
                    sta_pass<SCATTER>(in, in ? i - t_lo : 0, v[u][p], (int)(row + u), sp[u] == sg[u], row + u >= r_lo, t, lane);
                }
            }
        }
        if (!SCATTER)
            for (int c = lane; c < width; c += 64) trow[c] = t.cnt[c];
    }
}

__device__ __forceinline__ int sta_class(int len) { return len > 0 ? 32 - __clz(len) : 0; }  // 0 (empty) .. 31

// list_offsets for the trigger lists: out = base [n] (no element n: the total goes nowhere); order = the features by class
// of length, long ones first
struct StaOffsets {
    static constexpr bool CLASSES = true, TOTAL = false;
    const int32_t* lens;
    int n;
    int64_t* out;
    int32_t* order;
    __device__ long long len(int f) const { return lens[f]; }
    __device__ void count(int* cls, int f) const { atomicAdd(&cls[sta_class(lens[f])], 1); }
    __device__ void place(int* cls, int f) const { order[atomicAdd(&cls[sta_class(lens[f])], 1)] = f; }
};

__global__ __launch_bounds__(1024) void sta_offsets_kernel(const int32_t* __restrict__ lens, int f_cols, int64_t* __restrict__ base,
                                                           int32_t* __restrict__ order) {
    list_offsets(StaOffsets{lens, f_cols, base, order});
}

// LP: lags the lane's registers hold (L <= LP); DT: the signal's type
template <int LP, int DT>
__global__ __launch_bounds__(64) void sta_accum_kernel(const int32_t* __restrict__ ent_row, const float* __restrict__ ent_w,
                                                       const int64_t* __restrict__ base, const int32_t* __restrict__ lens,
                                                       const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                       int64_t n_rows, const void* __restrict__ y, int C, int64_t ldy,
                                                       int lag_lo, int L, int f_cols, int c_tiles,
                                                       double* __restrict__ acc, double* __restrict__ wsum,
                                                       long long* __restrict__ cnt) {
    __shared__ int st_ring[3 * ST_RING];
    lds_i32* rrow = (lds_i32*)st_ring;
    lds_i32* rseg = (lds_i32*)(st_ring + ST_RING);
    lds_f32* rw = (lds_f32*)(st_ring + 2 * ST_RING);
    const int lane = threadIdx.x;
    const int64_t n_jobs = (int64_t)f_cols * c_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int jf = (int)(job / c_tiles), ct = (int)(job - (int64_t)jf * c_tiles);
        const int f = __builtin_amdgcn_readfirstlane(order[jf]);
        const int len = __builtin_amdgcn_readfirstlane(lens[f]);
        if (len == 0) continue;  // (wave-uniform) nothing to add: the state is not touched
        const int64_t b0 = base[f];
        const int32_t* e = ent_row + b0;
        const float* w = ent_w + b0;
        const int c = ct * 64 + lane;
        const bool has_c = c < C;
        double a[LP];
#pragma unroll
        for (int j = 0; j < LP; ++j) a[j] = (j < L && has_c) ? acc[((int64_t)f * L + j) * C + c] : 0.0;
        const bool keeps = ct == 0 && lane < L;  // lane j of the first channel tile keeps wsum and cnt of lag j
        double ws = keeps ? wsum[(int64_t)f * L + lane] : 0.0;
        long long n = keeps ? cnt[(int64_t)f * L + lane] : 0;
        rrow[lane] = ST_NEVER;
        rrow[lane + 64] = ST_NEVER;
        int next = 0;
        long long last = -(1ll << 40);  // the row of the newest trigger in the ring
        long long p0 = 0;               // p = signal row - lag_lo: the row whose trigger enters the ring at this step
        for (;;) {
            if (p0 - last > L - 1) {  // no trigger reaches the signal rows from here on: go to the next one
                if (next >= len) break;
                p0 = __builtin_amdgcn_readfirstlane(e[next]);
            }
            int tr = -1, sp = -1, sr = -1;
            int tw = 0;  // (the bits of the weight)
            if (lane < ST_RB) {
                if (next + lane < len) {
                    tr = e[next + lane];
                    tw = __float_as_int(w[next + lane]);
                }
                const long long pr = p0 + lane, rr = pr + lag_lo;
                if (pr < n_rows) sp = seg ? seg[pr] : 0;
                if (rr >= 0 && rr < n_rows) sr = seg ? seg[rr] : 0;  // negative: no such row, or padding
            }
            float yv[ST_RB];
#pragma unroll
            for (int i = 0; i < ST_RB; ++i) {
                yv[i] = 0.f;
                if (__builtin_amdgcn_readlane(sr, i) >= 0 && has_c) yv[i] = load_act<DT>(y, (p0 + i + lag_lo) * ldy + c);
            }
            int used = 0;
#pragma unroll
            for (int i = 0; i < ST_RB; ++i) {
                const int pi = (int)(p0 + i);
                if (__builtin_amdgcn_readlane(tr, used) == pi) {  // (at most one trigger per row and feature)
                    const float wn = __int_as_float(__builtin_amdgcn_readlane(tw, used));
                    const int sn = __builtin_amdgcn_readlane(sp, i);
                    if (lane == 0) {
                        rrow[pi & (ST_RING - 1)] = pi;
                        rw[pi & (ST_RING - 1)] = wn;
                        rseg[pi & (ST_RING - 1)] = sn;
                    }
                    ++used;
                    last = p0 + i;
                }
                const int s_i = __builtin_amdgcn_readlane(sr, i);
                if (s_i < 0) continue;  // (wave-uniform)
                const int q = pi - lane;  // the trigger row of lag lag_lo + lane
                const int slot = q & (ST_RING - 1);
                const bool valid = lane < L && rrow[slot] == q && rseg[slot] == s_i;
                const float wl = rw[slot];
                const unsigned long long m = __ballot(valid);
                if (m == 0ull) continue;
                const double wd = valid ? (double)wl : 0.0;
                if (valid) {
                    ws += wd;
                    n += 1;
                }
                const double yd = (double)yv[i];
                // (wave-uniform tests, first per group of four lags: a row that an isolated trigger reaches has one term)
#pragma unroll
                for (int g = 0; g < LP; g += 4) {
                    if (((m >> g) & 15ull) == 0ull) continue;
#pragma unroll
                    for (int j = g; j < g + 4 && j < LP; ++j)
                        if ((m >> j) & 1ull) a[j] = fma(lane_f64(wd, j), yd, a[j]);  // (the product is exact in fp64)
                }
            }
            next += used;
            p0 += ST_RB;
        }
#pragma unroll
        for (int j = 0; j < LP; ++j)
            if (j < L && has_c) acc[((int64_t)f * L + j) * C + c] = a[j];
        if (keeps) {
            wsum[(int64_t)f * L + lane] = ws;
            cnt[(int64_t)f * L + lane] = n;
        }
    }
}

struct StaPlan {
    ChunkPlan c;
    int64_t off_row, off_w, off_table, off_lens, off_base, off_order, bytes;
};

StaPlan sta_plan(int64_t n_rows, int k, int f_cols) {
    StaPlan p;
    p.c = chunk_plan(n_rows);
    const int64_t entries = n_rows * k;
    p.off_row = 0;
    p.off_w = p.off_row + align256(4 * entries);
    p.off_table = p.off_w + align256(4 * entries);
    p.off_lens = p.off_table + align256(4 * (int64_t)p.c.n_chunks * f_cols);
    p.off_base = p.off_lens + align256(4 * (int64_t)f_cols);
    p.off_order = p.off_base + align256(8 * (int64_t)f_cols);
    p.bytes = p.off_order + align256(4 * (int64_t)f_cols);
    return p;
}

}  // namespace

extern "C" int64_t wsae_sta_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t f_lo, int32_t f_cols) {
    return code_args_ok(n_rows, k, WSAE_STA_MAX_K, hidden, f_lo, f_cols) ? sta_plan(n_rows, k, f_cols).bytes : -1;
}

extern "C" int wsae_sta_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                               int64_t n_rows, const void* y, int32_t y_dtype, int32_t channels, int64_t ldy, int32_t lag_lo,
                               int32_t lag_hi, int32_t f_lo, int32_t f_cols, int32_t trigger, int32_t weight, double* acc,
                               double* wsum, int64_t* cnt, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && y && acc && wsum && cnt, "wsae_sta_update: null pointer");
    CW_REQUIRE_K("wsae_sta_update", k, WSAE_STA_MAX_K);
    CW_REQUIRE_HIDDEN("wsae_sta_update", hidden);
    CW_REQUIRE_ROWS("wsae_sta_update", n_rows);
    WSAE_REQUIRE(y_dtype == WSAE_DT_F32 || y_dtype == WSAE_DT_BF16, "wsae_sta_update: y_dtype must be WSAE_DT_F32 or WSAE_DT_BF16 (got %d)",
                 y_dtype);
    WSAE_REQUIRE(channels >= 1 && channels <= WSAE_STA_MAX_CH, "wsae_sta_update: need 1 <= channels <= %d (got %d)",
                 WSAE_STA_MAX_CH, channels);
    WSAE_REQUIRE(ldy >= channels, "wsae_sta_update: ldy %lld is smaller than the %d channels", (long long)ldy, channels);
    WSAE_REQUIRE(lag_lo <= lag_hi && lag_lo >= -1024 && lag_hi <= 1024 && lag_hi - lag_lo + 1 <= WSAE_STA_MAX_LAGS,
                 "wsae_sta_update: need -1024 <= lag_lo <= lag_hi <= 1024 and at most %d lags (got %d .. %d)", WSAE_STA_MAX_LAGS,
                 lag_lo, lag_hi);
    CW_REQUIRE_WINDOW("wsae_sta_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(trigger == WSAE_STA_TRIGGER_ALL || trigger == WSAE_STA_TRIGGER_ONSET,
                 "wsae_sta_update: trigger must be WSAE_STA_TRIGGER_ALL or WSAE_STA_TRIGGER_ONSET (got %d)", trigger);
    WSAE_REQUIRE(weight == WSAE_STA_WEIGHT_VALUE || weight == WSAE_STA_WEIGHT_ONE,
                 "wsae_sta_update: weight must be WSAE_STA_WEIGHT_VALUE or WSAE_STA_WEIGHT_ONE (got %d)", weight);
    const StaPlan p = sta_plan(n_rows, k, f_cols);
    WSAE_REQUIRE_WORKSPACE("wsae_sta_update", workspace, workspace_bytes, p.bytes, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_sta_update", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* ent_row = (int32_t*)(ws + p.off_row);
    float* ent_w = (float*)(ws + p.off_w);
    int32_t* table = (int32_t*)(ws + p.off_table);
    int32_t* lens = (int32_t*)(ws + p.off_lens);
    int64_t* base = (int64_t*)(ws + p.off_base);
    int32_t* order = (int32_t*)(ws + p.off_order);
    const int n_tiles = ceil_div(f_cols, ST_TILE);
    const int64_t walk_jobs = (int64_t)p.c.n_chunks * n_tiles;
    const int walk_grid = (int)(walk_jobs < ST_MAX_BLOCKS ? walk_jobs : ST_MAX_BLOCKS);
    const int onset = trigger == WSAE_STA_TRIGGER_ONSET, one = weight == WSAE_STA_WEIGHT_ONE;
    const size_t lds_count = ST_TILE * 9, lds_scatter = ST_TILE * 13;
#define ST_WALK(SC_, NP_, LDS_)                                                                                           \
    sta_walk_kernel<SC_, NP_><<<walk_grid, 64, LDS_, st>>>(vals, idx, k, seg, n_rows, p.c.chunk_rows, p.c.n_chunks, f_lo, f_cols, \
                                                           n_tiles, onset, one, table, base, ent_row, ent_w)
    if (k <= 64) ST_WALK(false, 1, lds_count); else ST_WALK(false, 2, lds_count);
    chunk_scan_kernel<256><<<ceil_div(f_cols, 256), 256, 0, st>>>(table, p.c.n_chunks, f_cols, lens);
    sta_offsets_kernel<<<1, 1024, 0, st>>>(lens, f_cols, base, order);
    if (k <= 64) ST_WALK(true, 1, lds_scatter); else ST_WALK(true, 2, lds_scatter);
#undef ST_WALK
    const int L = lag_hi - lag_lo + 1;
    const int c_tiles = ceil_div(channels, 64);
    const int64_t acc_jobs = (int64_t)f_cols * c_tiles;
    const int acc_grid = (int)(acc_jobs < ST_MAX_BLOCKS ? acc_jobs : ST_MAX_BLOCKS);
#define ST_ACCUM(LP_, DT_)                                                                                                 \
    sta_accum_kernel<LP_, DT_><<<acc_grid, 64, 0, st>>>(ent_row, ent_w, base, lens, order, seg, n_rows, y, channels, ldy, lag_lo, \
                                                        L, f_cols, c_tiles, acc, wsum, (long long*)cnt)
#define ST_ACCUM_L(DT_)                                                                                                   \
    do {                                                                                                                  \
        if (L <= 8) ST_ACCUM(8, DT_); else if (L <= 17) ST_ACCUM(17, DT_); else if (L <= 32) ST_ACCUM(32, DT_); else ST_ACCUM(64, DT_); \
    } while (0)
    if (y_dtype == WSAE_DT_BF16) ST_ACCUM_L(WSAE_DT_BF16); else ST_ACCUM_L(WSAE_DT_F32);
#undef ST_ACCUM_L
#undef ST_ACCUM
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
