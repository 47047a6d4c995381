// Temporal run statistics: how long does a feature stay on, how long does it stay away, and where
// are its activations in the utterance?
//
// A run of feature f in segment (utterance) s is a maximal stretch of consecutive rows of the call, all of segment s, on
// which f is active.  Three launches.  The workspace's per-segment row bounds are reset and found with integer atomics
// (one pair per stretch of equal ids: seg_bounds of wsae_codewalk.h).  Then a single-wave workgroup
// owns a (segment, tile of features) job and walks the segment's rows in ascending order (four rows of loads
// in flight), one lane per entry.  Per tile feature LDS holds the row it was last seen on and the first row of its open
// run (with events also the run's fp32 sum, in row order, and its peak).  An entry seen on row r continues the run when
// the feature was seen on r - 1; otherwise it closes the feature's previous run, which also yields the gap, and opens a
// new one; a sweep over the tile after the last row closes what is still open.  Closing a run is a handful of global
// integer atomics (counts, the two histogram cells, the 64-bit sum of squares, the maximum) and, with events, a record
// staged in the wave's LDS; the cursor is a single address for the whole chip, so a wave takes the slots of 65 to 128
// staged records with one atomic on it.  One owner per (segment, feature) and one order: no float atomics; every
// statistic is an integer sum or maximum, so the state does not depend on the launch geometry, the order of the batches
// or the grouping of whole utterances into calls.  A one-byte LDS tag per column tells whether two entries of one pass
// name the same column (a TopK code never does); only then the pass is replayed lane by lane, and an entry whose feature
// was already seen on this row is skipped: an index repeated within a row counts once, with the value of its first
// active entry.
#include <limits.h>

#include "wsae_codewalk.h"

namespace {

constexpr int RN_TILE = 3072;        // features per job without events: 24 KB of rows + 3 KB of tags per wave
constexpr int RN_TILE_EV = 1536;     // ... with events: 24 KB of rows, sums, peaks + 1.5 KB of tags + 3 KB of stage = 29184 B
constexpr int RN_STAGE = 128;        // event records a wave stages in LDS before it takes their slots (24 bytes each)
constexpr int RN_MAX_BLOCKS = 2560;  // five resident single-wave workgroups per CU by LDS; more jobs than that: grid-stride
constexpr int RN_ROWS = 4;           // rows whose loads are issued before the first of them is processed
constexpr int RN_BINS = WSAE_RUNS_BINS;

struct RunsOut {
    int32_t* frames;
    int32_t* runs;
    int32_t* dur_max;
    unsigned long long* dur_sq;
    int32_t* dur_hist;
    int32_t* gap_hist;  // nullable
    unsigned long long* total_rows;
    int32_t* ev_int;  // [ev_cap][4]
    float* ev_flt;    // [ev_cap][2]
    unsigned long long* ev_count;
    unsigned long long ev_cap;
    int ev_min_len;
    int seg_base;
};

// the tile's rows in LDS
struct RunsTile {
    lds_i32* seen;  // the row the feature was last seen on, -2 = not yet
    lds_i32* open;  // the first row of its open run
    lds_f32* sum;   // (events) the run's values added in row order
    lds_f32* peak;  // (events) ... and their maximum
    lds_u8* tag;
    lds_i32* stage;  // (events) [RN_STAGE][6]: feature, segment, start, length, the bits of total and peak
};

struct RunsClosed {
    bool yes;
    int a, b;  // first and last row of the run
    float total, peak;
};

// exact up to 32, then one bin per octave: bin 32 + j holds (2^(5+j), 2^(6+j)], the last bin everything above 2^20
__device__ __forceinline__ int runs_bin(int d) {
    if (d <= 32) return d - 1;
    const int b = 32 + (31 - __clz(d - 1)) - 5;
    return b < RN_BINS - 1 ? b : RN_BINS - 1;
}

// one entry (column c of the tile, value v) on row r; `cl` receives the run this entry closes, if any
template <bool EV>
__device__ __forceinline__ void runs_entry(bool act, int c, float v, int r, const RunsTile& t, RunsClosed& cl) {
    cl.yes = false;
    if (!act) return;
    const int ls = t.seen[c];
    if (ls == r) return;  // an earlier entry of this row named the feature: it counts once, the first value stands
    if (ls == r - 1) {
        t.seen[c] = r;
        if (EV) {
            t.sum[c] = t.sum[c] + v;
            t.peak[c] = fmaxf(t.peak[c], v);
        }
        return;
    }
    if (ls >= 0) {
        cl.yes = true;
        cl.a = t.open[c];
        cl.b = ls;
        if (EV) {
            cl.total = t.sum[c];
            cl.peak = t.peak[c];
        }
    }
    t.open[c] = r;
    t.seen[c] = r;
    if (EV) {
        t.sum[c] = v;
        t.peak[c] = v;
    }
}

// the staged event records take their slots: one bump of the cursor, then a record per lane.  Past the capacity the
// cursor keeps counting and the records are dropped.  Called by all 64 lanes together; n_staged is wave-uniform.
__device__ __forceinline__ void runs_flush(const RunsTile& t, int& n_staged, const RunsOut& o, int lane) {
    if (n_staged == 0) return;
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(o.ev_count, (unsigned long long)n_staged);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
    base = ((unsigned long long)hi << 32) | lo;
    for (int i = lane; i < n_staged; i += 64) {
        const unsigned long long slot = base + (unsigned long long)i;
        if (slot < o.ev_cap) {
            lds_i32* e = t.stage + 6 * i;
            int32_t* g = o.ev_int + 4 * slot;
            g[0] = e[0];
            g[1] = e[1];
            g[2] = e[2];
            g[3] = e[3];
            o.ev_flt[2 * slot] = __int_as_float(e[4]);
            o.ev_flt[2 * slot + 1] = __int_as_float(e[5]);
        }
    }
    n_staged = 0;
}

// the statistics of the closed runs of the wave's lanes (wc: the column in the window); called by all 64 lanes together.
// next_row >= 0: the row on which the feature was seen again, i.e. the closed run is followed by a gap.
template <bool EV>
__device__ __forceinline__ void runs_emit(const RunsClosed& cl, int next_row, int wc, int feature, int s, int r0,
                                          const RunsTile& t, int& n_staged, const RunsOut& o, int lane) {
    bool ev = false;
    int d = 0;
    if (cl.yes) {
        d = cl.b - cl.a + 1;
        atomicAdd(o.runs + wc, 1);
        atomicAdd(o.frames + wc, d);
        atomicMax(o.dur_max + wc, d);
        atomicAdd(o.dur_sq + wc, (unsigned long long)d * (unsigned long long)d);
        atomicAdd(o.dur_hist + (int64_t)wc * RN_BINS + runs_bin(d), 1);
        if (next_row >= 0 && o.gap_hist) atomicAdd(o.gap_hist + (int64_t)wc * RN_BINS + runs_bin(next_row - cl.b - 1), 1);
        ev = EV && d >= o.ev_min_len;
    }
    if (EV) {
        const unsigned long long m = __ballot(ev);
        if (m == 0ull) return;  // (wave-uniform)
        const int cnt = __popcll(m);
        if (n_staged + cnt > RN_STAGE) runs_flush(t, n_staged, o, lane);
        if (ev) {
            lds_i32* e = t.stage + 6 * (n_staged + __popcll(m & ((1ull << lane) - 1ull)));
            e[0] = feature;
            e[1] = o.seg_base + s;
            e[2] = cl.a - r0;
            e[3] = d;
            e[4] = __float_as_int(cl.total);
            e[5] = __float_as_int(cl.peak);
        }
        n_staged += cnt;
    }
}

// one pass of at most 64 entries (lane = entry) of row r into the wave's tile
template <bool EV>
__device__ __forceinline__ void runs_pass(bool in, int c, float v, int r, const RunsTile& t, int c_lo, int f_lo, int s, int r0,
                                          int& n_staged, const RunsOut& o, int lane) {
    if (in) t.tag[c] = (uint8_t)lane;
    const bool lost = in && t.tag[c] != (uint8_t)lane;  // another entry of this pass names the same column
    RunsClosed cl;
    if (__ballot(lost) == 0ull) {
        runs_entry<EV>(in, c, v, r, t, cl);
        runs_emit<EV>(cl, r, c_lo + c, f_lo + c_lo + c, s, r0, t, n_staged, o, lane);
    } else {
        for (unsigned long long m = __ballot(in); m; m &= m - 1ull) {  // in entry order
            runs_entry<EV>(in && lane == __builtin_ctzll(m), c, v, r, t, cl);
            runs_emit<EV>(cl, r, c_lo + c, f_lo + c_lo + c, s, r0, t, n_staged, o, lane);
        }
    }
}

// NP: passes of 64 entries per row (k <= 64 * NP)
template <bool EV, int NP>
__global__ __launch_bounds__(64) void runs_walk_kernel(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k,
                                                       const int32_t* __restrict__ seg, int n_seg, int f_lo, int f_cols,
                                                       int n_tiles, const int32_t* __restrict__ first,
                                                       const int32_t* __restrict__ last, RunsOut o) {
    constexpr int W = EV ? RN_TILE_EV : RN_TILE;
    extern __shared__ float rn_smem[];
    RunsTile t;
    t.seen = (lds_i32*)rn_smem;
    t.open = (lds_i32*)(rn_smem + W);
    t.tag = (lds_u8*)(rn_smem + (EV ? 4 : 2) * W);
    t.sum = t.peak = nullptr;
    t.stage = nullptr;
    if (EV) {  // (without events the tile is seen, open and the tags: 9 W bytes)
        t.sum = (lds_f32*)(rn_smem + 2 * W);
        t.peak = (lds_f32*)(rn_smem + 3 * W);
        t.stage = (lds_i32*)(rn_smem + 4 * W + W / 4);  // behind the W bytes of tags
    }
    int n_staged = 0;
    const int lane = threadIdx.x;
    const int64_t n_jobs = (int64_t)n_seg * n_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int s = (int)(job / n_tiles), tl = (int)(job - (int64_t)s * n_tiles);
        const int r0 = first[s], r1 = last[s];
        if (r0 > r1) continue;  // the segment has no row in this call (wave-uniform)
        const int c_lo = tl * W;
        const int width = f_cols - c_lo < W ? f_cols - c_lo : W;
        const int t_lo = f_lo + c_lo;
        for (int c = lane; c < width; c += 64) t.seen[c] = -2;
        int rows_here = 0;
        for (int64_t row = r0; row <= r1; row += RN_ROWS) {
            float v[RN_ROWS][NP];
            int ix[RN_ROWS][NP];
            int sg[RN_ROWS];
#pragma unroll
            for (int u = 0; u < RN_ROWS; ++u) {
                const bool have = row <= r1 - u;
                const int64_t rr = have ? row + u : r1;
                sg[u] = __builtin_amdgcn_readfirstlane(have ? seg[rr] : -1);
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
            for (int u = 0; u < RN_ROWS; ++u) {
                if (sg[u] != s) continue;  // a padding row, or a row of another segment, inside the range (wave-uniform)
                ++rows_here;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int i = ix[u][p];
                    const bool in = v[u][p] > 0.f && i >= t_lo && i - t_lo < width;  // (t_lo + width <= hidden)
                    runs_pass<EV>(in, in ? i - t_lo : 0, v[u][p], (int)row + u, t, c_lo, f_lo, s, r0, n_staged, o, lane);
                }
            }
        }
        for (int c0 = 0; c0 < width; c0 += 64) {  // what is still open ends with the segment (all lanes stay together)
            const int c = c0 + lane;
            RunsClosed cl;
            cl.yes = c < width && t.seen[c] >= 0;
            if (cl.yes) {
                cl.a = t.open[c];
                cl.b = t.seen[c];
                if (EV) {
                    cl.total = t.sum[c];
                    cl.peak = t.peak[c];
                }
            }
            runs_emit<EV>(cl, -1, c_lo + c, t_lo + c, s, r0, t, n_staged, o, lane);
        }
        if (tl == 0 && lane == 0) atomicAdd(o.total_rows, (unsigned long long)rows_here);
    }
    if (EV) runs_flush(t, n_staged, o, lane);
}

}  // namespace

extern "C" int64_t wsae_runs_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_seg, int32_t f_lo,
                                             int32_t f_cols) {
    const bool ok = code_args_ok(n_rows, k, WSAE_RUNS_MAX_K, hidden, f_lo, f_cols) && n_seg >= 1;
    return ok ? 8 * (int64_t)n_seg : -1;  // first and last row per segment
}

extern "C" int wsae_runs_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                int64_t n_rows, int32_t n_seg, int32_t seg_base, int32_t f_lo, int32_t f_cols, int32_t* frames,
                                int32_t* runs, int32_t* dur_max, int64_t* dur_sq, int32_t* dur_hist, int32_t* gap_hist,
                                int64_t* total_rows, int32_t* ev_int, float* ev_flt, int64_t ev_cap, int32_t ev_min_len,
                                int64_t* ev_count, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && seg && frames && runs && dur_max && dur_sq && dur_hist && total_rows,
                 "wsae_runs_update: null pointer");
    CW_REQUIRE_K("wsae_runs_update", k, WSAE_RUNS_MAX_K);
    WSAE_REQUIRE(hidden >= 1 && n_seg >= 1, "wsae_runs_update: hidden and n_seg must be positive (got %d, %d)", hidden, n_seg);
    CW_REQUIRE_ROWS("wsae_runs_update", n_rows);
    CW_REQUIRE_WINDOW("wsae_runs_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(seg_base >= 0 && (int64_t)seg_base + n_seg <= INT_MAX,
                 "wsae_runs_update: seg_base %d with %d segments leaves the int32 range", seg_base, n_seg);
    WSAE_REQUIRE(ev_cap >= 0, "wsae_runs_update: ev_cap must not be negative (got %lld)", (long long)ev_cap);
    WSAE_REQUIRE(ev_cap == 0 || (ev_int && ev_flt && ev_count),
                 "wsae_runs_update: ev_cap %lld needs the event buffers and the cursor (null pointer)", (long long)ev_cap);
    WSAE_REQUIRE(ev_min_len >= 1, "wsae_runs_update: ev_min_len must be at least 1 (got %d)", ev_min_len);
    const int64_t need = 8 * (int64_t)n_seg;
    WSAE_REQUIRE_WORKSPACE("wsae_runs_update", workspace, workspace_bytes, need, n_rows);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t* first = (int32_t*)workspace;
    int32_t* last = first + n_seg;
    seg_bounds(seg, n_rows, n_seg, first, last, st);
    const bool ev = ev_count != nullptr;  // (with ev_cap == 0 the cursor counts the records a buffer would need)
    RunsOut o;
    o.frames = frames;
    o.runs = runs;
    o.dur_max = dur_max;
    o.dur_sq = (unsigned long long*)dur_sq;
    o.dur_hist = dur_hist;
    o.gap_hist = gap_hist;
    o.total_rows = (unsigned long long*)total_rows;
    o.ev_int = ev_int;
    o.ev_flt = ev_flt;
    o.ev_count = (unsigned long long*)ev_count;
    o.ev_cap = (unsigned long long)ev_cap;
    o.ev_min_len = ev_min_len;
    o.seg_base = seg_base;
    const int tile = ev ? RN_TILE_EV : RN_TILE;
    const int n_tiles = ceil_div(f_cols, tile);
    const int64_t n_jobs = (int64_t)n_seg * n_tiles;
    const int grid = (int)(n_jobs < RN_MAX_BLOCKS ? n_jobs : RN_MAX_BLOCKS);
    const size_t lds = (size_t)tile * (ev ? 17 : 9) + (ev ? RN_STAGE * 24 : 0);
#define RN_LAUNCH(EV_, NP_)                                                                                               \
    runs_walk_kernel<EV_, NP_><<<grid, 64, lds, st>>>(vals, idx, k, seg, n_seg, f_lo, f_cols, n_tiles, first, last, o)
    if (ev) {
        if (k <= 64) RN_LAUNCH(true, 1); else RN_LAUNCH(true, 2);
    } else {
        if (k <= 64) RN_LAUNCH(false, 1); else RN_LAUNCH(false, 2);
    }
#undef RN_LAUNCH
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
