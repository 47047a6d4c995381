// Sparse linear probes: softmax regression of a per-frame label on the compact code, without the
// dense [frames, H] matrix and without float atomics.  An iteration of the fit is two sparse products over the code.
//
// wsae_probe_plan transposes the code once (it depends on the code, seg and col_of only).  A stable counting sort in
// four launches, the scheme of wsae_sta_update - with its chunking of the rows, its scan and the body of its offsets
// kernel, all in wsae_lists.h - and a walk of its own for this entry list (every first-active entry that has a column, no
// lags, no onset rule):
//   1. probe_walk_kernel<false>: a single-wave workgroup owns (chunk of consecutive rows, tile of PB_TILE columns), walks
//      its rows in order, one lane per entry, and counts the entries of each column in LDS: one row of [chunks, P].
//   2. chunk_scan_kernel: per column the exclusive prefix over the chunks and its total; probe_offsets_kernel<false> (one
//      workgroup, list_offsets with the policy ProbeOffsets): the exclusive prefix of the totals - col_ptr - and nnz.
//   3. probe_walk_kernel<true>: the same walk, taking slots from LDS cursors that start at the scanned positions, so a
//      column's list is in ascending row.  Slots from cap on are not written.
// The entries of one row name distinct columns (first-active entries name distinct features, col_of maps them to
// distinct columns), so the lanes of a pass never meet in a counter or a cursor.
//
// wsae_probe_forward: one wave per row, lanes as classes (CT tiles of 64 per lane).  The row's first-active entries are
// found in registers, their (value, column) reach the lanes by v_readlane, and the weight rows of PB_FB entries are
// loaded before the first of them is added; the label and the entries of the wave's next row are requested before that.  A logit is ONE chain: bias, then per entry an fp32 multiply and an fp32 add
// (not fused: contraction is off in this file), in ascending entry position.  The reductions over the classes are the fixed
// butterfly of wave_max / wave_sum over per-lane partials taken in ascending tile, so what is written for a row depends
// on that row alone.  The counters are integer sums kept per wave and added once at its end.
//
// wsae_probe_backward: gW[p][c] = stored + partial_0 + partial_1 + ..., partial_q one fp64 chain over the entries
// q CHUNK .. of column p.  probe_offsets_kernel<true> numbers the (column, chunk) jobs on the device (no host synchronisation),
// probe_partial_kernel gives a job and 64 classes to a wave (lanes as classes, eight error rows in flight, the job's
// column found by bisection of the job numbers) and stores the partial, probe_sum_kernel adds a column's partials in
// order.  gb the same way over chunks of WSAE_PROBE_CHUNK consecutive rows.
#include "wsae_lists.h"

// every fp32 multiply and add below rounds on its own, as the numpy mirror of the tests does
#pragma clang fp contract(off)

namespace {

constexpr int PB_TILE = 4096;        // columns per walk job: 16 KB of counts, or 32 KB of cursors
constexpr int PB_ROWS = 4;           // rows of the code whose loads are issued before the first of them is processed
constexpr int PB_MAX_BLOCKS = 1 << 20;
constexpr int PB_FWD_BLOCK = 256;        // four waves, a row each
constexpr int PB_FWD_MAX_BLOCKS = 2048;  // more rows than PB_FWD_MAX_BLOCKS * 4: the grid-stride loop
constexpr int PB_FB = 8;                 // entries of a row whose weight rows are loaded before the first of them is added
constexpr int PB_RB = 8;                 // error rows in flight in the backward chains
constexpr int PB_CHUNK = WSAE_PROBE_CHUNK;

static_assert((PB_CHUNK & (PB_CHUNK - 1)) == 0 && PB_CHUNK >= 64, "WSAE_PROBE_CHUNK must be a power of two >= 64");

// (probe_load_row and probe_row_columns, the row front end shared with wsae_regress.hip, are in wsae_codewalk.h)

// ---- the plan ---------------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__device__ __forceinline__ void probe_take(int col, float v, int r, int c_lo, int width, lds_i32* cnt, lds_u64* cur,
                                           int32_t* __restrict__ t_row, float* __restrict__ t_val, int64_t cap) {
    const int c = col - c_lo;
    if (col < 0 || c < 0 || c >= width) return;
    if (SCATTER) {
        const unsigned long long slot = cur[c];
        cur[c] = slot + 1ull;
        if ((int64_t)slot < cap) {
            t_row[slot] = r;
            t_val[slot] = v;
        }
    } else {
        cnt[c] = cnt[c] + 1;
    }
}

// table [n_chunks][P]: written by the count, read (after the scan) by the scatter
template <bool SCATTER>
__global__ __launch_bounds__(64) void probe_walk_kernel(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k,
                                                        int hidden, const int32_t* __restrict__ seg, int64_t n_rows,
                                                        int64_t chunk_rows, int n_chunks, const int32_t* __restrict__ col_of,
                                                        int P, int n_tiles, int32_t* __restrict__ table,
                                                        const int64_t* __restrict__ col_ptr, int32_t* __restrict__ t_row,
                                                        float* __restrict__ t_val, int64_t cap) {
    __shared__ unsigned long long pb_smem[PB_TILE];  // (count) int32 [PB_TILE]; (scatter) uint64 [PB_TILE]
    lds_i32* cnt = (lds_i32*)pb_smem;
    lds_u64* cur = (lds_u64*)pb_smem;
    const int lane = threadIdx.x;
    const int64_t n_jobs = (int64_t)n_chunks * n_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int ch = (int)(job / n_tiles), tl = (int)(job - (int64_t)ch * n_tiles);
        const int c_lo = tl * PB_TILE;
        const int width = P - c_lo < PB_TILE ? P - c_lo : PB_TILE;
        const int64_t r_lo = (int64_t)ch * chunk_rows;
        const int64_t r_hi = r_lo + chunk_rows < n_rows ? r_lo + chunk_rows : n_rows;  // exclusive
        int32_t* trow = table + (int64_t)ch * P + c_lo;
        for (int c = lane; c < width; c += 64) {
            if (SCATTER) cur[c] = (unsigned long long)(col_ptr[c_lo + c] + (int64_t)trow[c]);
            else cnt[c] = 0;
        }
        for (int64_t row = r_lo; row < r_hi; row += PB_ROWS) {
            float v0[PB_ROWS], v1[PB_ROWS];
            int f0[PB_ROWS], f1[PB_ROWS], sg[PB_ROWS];
#pragma unroll
            for (int u = 0; u < PB_ROWS; ++u) {
                const bool have = row + u < r_hi;
                const int64_t rr = have ? row + u : r_hi - 1;
                sg[u] = __builtin_amdgcn_readfirstlane(have ? (seg ? seg[rr] : 0) : -1);
                probe_load_row(vals, idx, k, rr, lane, v0[u], f0[u], v1[u], f1[u]);
            }
#pragma unroll
            for (int u = 0; u < PB_ROWS; ++u) {
                if (sg[u] < 0) continue;  // a padding row, or past the chunk (wave-uniform)
                int col0, col1;
                probe_row_columns(v0[u], f0[u], v1[u], f1[u], k, hidden, col_of, lane, col0, col1);
                probe_take<SCATTER>(col0, v0[u], (int)(row + u), c_lo, width, cnt, cur, t_row, t_val, cap);
                probe_take<SCATTER>(col1, v1[u], (int)(row + u), c_lo, width, cnt, cur, t_row, t_val, cap);
            }
        }
        if (!SCATTER)
            for (int c = lane; c < width; c += 64) trow[c] = cnt[c];
    }
}

// list_offsets for the plan: out [n + 1], out[n] = the total (also to *total when given).  CHUNKED: a length is the number
// of WSAE_PROBE_CHUNK pieces of column p's list clipped to cap (in: col_ptr); otherwise in is the lengths.
template <bool CHUNKED>
struct ProbeOffsets {
    static constexpr bool CLASSES = false, TOTAL = true;
    const void* in;
    int n;
    int64_t cap;
    int64_t* out;
    int64_t* total;
    __device__ long long len(int p) const {
        if (!CHUNKED) return ((const int32_t*)in)[p];
        const int64_t* cp = (const int64_t*)in;
        const int64_t a = cp[p] < cap ? cp[p] : cap, b = cp[p + 1] < cap ? cp[p + 1] : cap;
        return b > a ? (b - a + PB_CHUNK - 1) / PB_CHUNK : 0;
    }
};

template <bool CHUNKED>
__global__ __launch_bounds__(1024) void probe_offsets_kernel(const void* __restrict__ in, int P, int64_t cap,
                                                             int64_t* __restrict__ out, int64_t* __restrict__ total) {
    list_offsets(ProbeOffsets<CHUNKED>{in, P, cap, out, total});
}

struct PlanWs {
    ChunkPlan c;
    int64_t off_table, off_lens, bytes;
};

PlanWs plan_ws(int64_t n_rows, int P) {
    PlanWs w;
    w.c = chunk_plan(n_rows);
    w.off_table = 0;
    w.off_lens = w.off_table + align256(4 * (int64_t)w.c.n_chunks * P);
    w.bytes = w.off_lens + align256(4 * (int64_t)P);
    return w;
}

#define PB_REQUIRE_CLASSES(FN, C)                                                                                         \
    WSAE_REQUIRE((C) >= 1 && (C) <= WSAE_PROBE_MAX_CLASSES, FN ": need 1 <= n_classes <= %d (got %d)",                    \
                 WSAE_PROBE_MAX_CLASSES, C)

// ---- the forward product ----------------------------------------------------------------------------------------------------
struct FwdArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;
    const int32_t* labels;
    const int32_t* col_of;
    const float* W;
    const float* bias;
    const float* class_weight;
    int64_t n_rows, ldw, lde;
    int k, hidden, lag, C;
    float* err;
    float* row_loss;
    unsigned long long* n_used;
    unsigned long long* n_correct;
    unsigned long long* loss_q;
    unsigned long long* confusion;
};

// the entries of `mask` (bits of the lanes whose col is a column), PB_FB at a time, in ascending position
template <int CT>
__device__ __forceinline__ void probe_add_entries(unsigned long long mask, float v, int col, const FwdArgs& a, int lane,
                                                  float (&logit)[CT]) {
    const int vb = __float_as_int(v);
    while (mask) {
        float ev[PB_FB];
        int ec[PB_FB];
#pragma unroll
        for (int u = 0; u < PB_FB; ++u) {
            ev[u] = 0.f;
            ec[u] = -1;
            if (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                ev[u] = __int_as_float(__builtin_amdgcn_readlane(vb, j));
                ec[u] = __builtin_amdgcn_readlane(col, j);
            }
        }
        float w[PB_FB][CT];
#pragma unroll
        for (int u = 0; u < PB_FB; ++u)
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int c = t * 64 + lane;
                w[u][t] = (ec[u] >= 0 && c < a.C) ? a.W[(int64_t)ec[u] * a.ldw + c] : 0.f;
            }
#pragma unroll
        for (int u = 0; u < PB_FB; ++u) {
            if (ec[u] < 0) continue;  // (wave-uniform)
#pragma unroll
            for (int t = 0; t < CT; ++t) logit[t] = logit[t] + ev[u] * w[u][t];  // (two roundings: contraction is off in this file)
        }
    }
}

// CT: class tiles of 64 per lane (C <= 64 CT)
template <int CT>
__global__ __launch_bounds__(PB_FWD_BLOCK) void probe_forward_kernel(FwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (PB_FWD_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (PB_FWD_BLOCK / 64);
    unsigned long long used = 0, correct = 0;
    long long lq = 0;
    // the label of row r, -1 where the row is dropped (all wave-uniform)
    auto label_of = [&](int64_t r) -> int {
        const int seg_r = a.seg ? a.seg[r] : 0;
        const int64_t q = r + a.lag;
        int y = -1;
        if (seg_r >= 0 && q >= 0 && q < a.n_rows && (a.seg == nullptr || a.seg[q] == seg_r)) y = a.labels[q];
        return y >= 0 && y < a.C ? y : -1;
    };
    // the label and the entries of a wave's next row are requested before it works on the current one
    float nv0 = 0.f, nv1 = 0.f;
    int nf0 = -1, nf1 = -1, ny = -1;
    if (wave < a.n_rows) {
        ny = label_of(wave);
        probe_load_row(a.vals, a.idx, a.k, wave, lane, nv0, nf0, nv1, nf1);
    }
    for (int64_t r = wave; r < a.n_rows; r += n_waves) {
        const int y = __builtin_amdgcn_readfirstlane(ny);
        const float v0 = nv0, v1 = nv1;
        const int f0 = nf0, f1 = nf1;
        if (r + n_waves < a.n_rows) {
            ny = label_of(r + n_waves);
            probe_load_row(a.vals, a.idx, a.k, r + n_waves, lane, nv0, nf0, nv1, nf1);
        }
        if (y < 0) {  // dropped: exact zeros, and it counts nowhere
            if (a.err) {
#pragma unroll
                for (int t = 0; t < CT; ++t)
                    if (t * 64 + lane < a.C) a.err[r * a.lde + t * 64 + lane] = 0.f;
            }
            if (a.row_loss && lane == 0) a.row_loss[r] = 0.f;
            continue;
        }
        int col0, col1;
        probe_row_columns(v0, f0, v1, f1, a.k, a.hidden, a.col_of, lane, col0, col1);
        float logit[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) logit[t] = t * 64 + lane < a.C ? a.bias[t * 64 + lane] : 0.f;
        probe_add_entries<CT>(__ballot(col0 >= 0), v0, col0, a, lane, logit);
        if (a.k > 64) probe_add_entries<CT>(__ballot(col1 >= 0), v1, col1, a, lane, logit);
        // max-subtracted softmax: per-lane partials in ascending tile, then the fixed butterfly
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < CT; ++t)
            if (t * 64 + lane < a.C) mx = fmaxf(mx, logit[t]);
        mx = wave_max(mx);
        float e[CT], s = 0.f;
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            e[t] = t * 64 + lane < a.C ? expf(logit[t] - mx) : 0.f;
            s = s + e[t];
        }
        s = wave_sum(s);
        int am = INT_MAX;  // the lowest class at the maximum
        float ly = 0.f;
#pragma unroll
        for (int t = CT - 1; t >= 0; --t) {
            if (t * 64 + lane < a.C && logit[t] == mx) am = t * 64 + lane;
            if (t == (y >> 6)) ly = logit[t];
        }
        am = wave_min_i(am);
        ly = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ly), y & 63));
        const float wy = a.class_weight ? a.class_weight[y] : 1.f;
        const float loss = wy * ((logf(s) + mx) - ly);
        if (a.err) {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int c = t * 64 + lane;
                if (c < a.C) a.err[r * a.lde + c] = wy * (e[t] / s - (c == y ? 1.f : 0.f));
            }
        }
        if (a.row_loss && lane == 0) a.row_loss[r] = loss;
        used += 1;
        correct += am == y;
        lq += llrintf(fminf(loss, 1024.f) * 1048576.f);
        if (a.confusion && lane == 0 && am < a.C) atomicAdd(a.confusion + (int64_t)y * a.C + am, 1ull);
    }
    if (lane == 0 && used) {
        atomicAdd(a.n_used, used);
        if (correct) atomicAdd(a.n_correct, correct);
        if (lq) atomicAdd(a.loss_q, (unsigned long long)lq);
    }
}

// ---- the backward product ---------------------------------------------------------------------------------------------------
// job_ptr [P + 1]: the (column, chunk) jobs before column p.  part [jobs][C]: the chain of job (p, q) over the entries
// q CHUNK .. of column p, started at 0.
__global__ __launch_bounds__(64) void probe_partial_kernel(const int64_t* __restrict__ col_ptr, const int32_t* __restrict__ t_row,
                                                           const float* __restrict__ t_val, int64_t cap, int P,
                                                           const int64_t* __restrict__ job_ptr, const float* __restrict__ err,
                                                           int64_t lde, int C, int64_t n_rows, int c_tiles,
                                                           double* __restrict__ part) {
    const int lane = threadIdx.x;
    const int64_t n_jobs = job_ptr[P] * c_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int64_t jb = job / c_tiles;
        const int c = (int)(job - jb * c_tiles) * 64 + lane;
        const bool has_c = c < C;
        int lo = 0, hi = P;  // the column of job jb: the last p with job_ptr[p] <= jb (wave-uniform)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (job_ptr[mid] <= jb) lo = mid; else hi = mid;
        }
        const int p = lo;
        const int64_t end_p = min64(col_ptr[p + 1], cap);
        const int64_t beg = min64(col_ptr[p], cap) + (jb - job_ptr[p]) * PB_CHUNK;
        const int64_t end = min64(beg + PB_CHUNK, end_p);
        double acc = 0.0;
        for (int64_t i0 = beg; i0 < end; i0 += 64) {
            int er = -1, ev = 0;  // 64 entries of the list, one per lane
            if (i0 + lane < end) {
                er = t_row[i0 + lane];
                ev = __float_as_int(t_val[i0 + lane]);
            }
            const int n = (int)min64(64, end - i0);
#pragma unroll
            for (int u0 = 0; u0 < 64; u0 += PB_RB) {
                if (u0 >= n) break;  // (wave-uniform)
                float x[PB_RB];
#pragma unroll
                for (int u = 0; u < PB_RB; ++u) {
                    const int r = __builtin_amdgcn_readlane(er, u0 + u);
                    x[u] = (has_c && r >= 0 && r < n_rows) ? err[(int64_t)r * lde + c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < PB_RB; ++u) {
                    if (u0 + u >= n) break;
                    const float v = __int_as_float(__builtin_amdgcn_readlane(ev, u0 + u));
                    acc = fma((double)v, (double)x[u], acc);  // (the product is exact in fp64)
                }
            }
        }
        if (has_c) part[jb * C + c] = acc;
    }
}

// gW[p][c] = ((stored + partial_0) + partial_1) + ...; a column without entries is not touched
__global__ __launch_bounds__(256) void probe_sum_kernel(const int64_t* __restrict__ job_ptr, int P, int C,
                                                        const double* __restrict__ part, double* __restrict__ gW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)P * C) return;
    const int p = (int)(i / C), c = (int)(i - (int64_t)p * C);
    const int64_t j0 = job_ptr[p], j1 = job_ptr[p + 1];
    if (j0 == j1) return;
    double x = gW[i];
    for (int64_t j = j0; j < j1; ++j) x += part[j * C + c];
    gW[i] = x;
}

// bpart [row chunks][C]: the chain over the rows q CHUNK .. of the call, started at 0
__global__ __launch_bounds__(64) void probe_bias_partial_kernel(const float* __restrict__ err, int64_t lde, int C, int64_t n_rows,
                                                                int c_tiles, int64_t n_chunks, double* __restrict__ bpart) {
    const int lane = threadIdx.x;
    const int64_t n_jobs = n_chunks * c_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int64_t ch = job / c_tiles;
        const int c = (int)(job - ch * c_tiles) * 64 + lane;
        if (c >= C) continue;
        const int64_t r_lo = ch * PB_CHUNK, r_hi = min64(r_lo + PB_CHUNK, n_rows);
        double acc = 0.0;
        for (int64_t r0 = r_lo; r0 < r_hi; r0 += PB_RB) {
            float x[PB_RB];
#pragma unroll
            for (int u = 0; u < PB_RB; ++u) x[u] = r0 + u < r_hi ? err[(r0 + u) * lde + c] : 0.f;
#pragma unroll
            for (int u = 0; u < PB_RB; ++u)
                if (r0 + u < r_hi) acc += (double)x[u];
        }
        bpart[ch * C + c] = acc;
    }
}

__global__ __launch_bounds__(64) void probe_bias_sum_kernel(const double* __restrict__ bpart, int C, int64_t n_chunks,
                                                            double* __restrict__ gb) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double x = gb[c];
#pragma unroll 8
    for (int64_t ch = 0; ch < n_chunks; ++ch) x += bpart[ch * C + c];
    gb[c] = x;
}

struct BwdWs {
    int64_t max_jobs, row_chunks, off_jobs, off_part, off_bpart, bytes;
};

BwdWs bwd_ws(int64_t n_rows, int P, int C, int64_t cap) {
    BwdWs w;
    w.max_jobs = (int64_t)P + cap / PB_CHUNK;  // every column one ragged piece at most, and the full pieces
    w.row_chunks = ceil_div64(n_rows, PB_CHUNK);
    w.off_jobs = 0;
    w.off_part = w.off_jobs + align256(8 * ((int64_t)P + 1));
    w.off_bpart = w.off_part + align256(8 * w.max_jobs * C);
    w.bytes = w.off_bpart + align256(8 * w.row_chunks * C);
    return w;
}

}  // namespace

extern "C" int64_t wsae_probe_plan_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols) {
    return column_code_ok(n_rows, k, hidden, n_cols) ? plan_ws(n_rows, n_cols).bytes : -1;
}

extern "C" int wsae_probe_plan(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                               int64_t n_rows, const int32_t* col_of, int32_t n_cols, int64_t* col_ptr, int32_t* t_row,
                               float* t_val, int64_t cap, int64_t* nnz, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && col_ptr && nnz, "wsae_probe_plan: null pointer");
    CW_REQUIRE_COLUMN_CODE("wsae_probe_plan", k, hidden, n_rows, col_of, n_cols);
    CW_REQUIRE_LISTS("wsae_probe_plan", cap, t_row, t_val);
    const PlanWs w = plan_ws(n_rows, n_cols);
    WSAE_REQUIRE_WORKSPACE("wsae_probe_plan", workspace, workspace_bytes, w.bytes, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_probe_plan", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t* table = (int32_t*)((char*)workspace + w.off_table);
    int32_t* lens = (int32_t*)((char*)workspace + w.off_lens);
    const int n_tiles = ceil_div(n_cols, PB_TILE);
    const int64_t jobs = (int64_t)w.c.n_chunks * n_tiles;
    const int grid = (int)(jobs < PB_MAX_BLOCKS ? jobs : PB_MAX_BLOCKS);
    probe_walk_kernel<false><<<grid, 64, 0, st>>>(vals, idx, k, hidden, seg, n_rows, w.c.chunk_rows, w.c.n_chunks, col_of, n_cols,
                                                  n_tiles, table, col_ptr, t_row, t_val, cap);
    chunk_scan_kernel<256><<<ceil_div(n_cols, 256), 256, 0, st>>>(table, w.c.n_chunks, n_cols, lens);
    probe_offsets_kernel<false><<<1, 1024, 0, st>>>(lens, n_cols, 0, col_ptr, nnz);
    probe_walk_kernel<true><<<grid, 64, 0, st>>>(vals, idx, k, hidden, seg, n_rows, w.c.chunk_rows, w.c.n_chunks, col_of, n_cols,
                                                 n_tiles, table, col_ptr, t_row, t_val, cap);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_probe_forward_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_cols,
                                                      int32_t n_classes, int32_t lag) {
    const bool ok =
        column_code_ok(n_rows, k, hidden, n_cols) && n_classes >= 1 && n_classes <= WSAE_PROBE_MAX_CLASSES && lag_ok(lag);
    return ok ? 0 : -1;
}

extern "C" int wsae_probe_forward(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                  const int32_t* labels, int64_t n_rows, int32_t lag, int32_t n_classes, const int32_t* col_of,
                                  int32_t n_cols, const float* W, int64_t ldw, const float* bias, const float* class_weight,
                                  float* err, int64_t lde, float* row_loss, int64_t* n_used, int64_t* n_correct, int64_t* loss_q,
                                  int64_t* confusion, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(vals && idx && labels && W && bias && n_used && n_correct && loss_q, "wsae_probe_forward: null pointer");
    CW_REQUIRE_COLUMN_CODE("wsae_probe_forward", k, hidden, n_rows, col_of, n_cols);
    PB_REQUIRE_CLASSES("wsae_probe_forward", n_classes);
    CW_REQUIRE_LAG("wsae_probe_forward", lag);
    WSAE_REQUIRE(ldw >= n_classes, "wsae_probe_forward: ldw %lld is smaller than the %d classes", (long long)ldw, n_classes);
    WSAE_REQUIRE(!err || lde >= n_classes, "wsae_probe_forward: lde %lld is smaller than the %d classes", (long long)lde,
                 n_classes);
    WSAE_REQUIRE(workspace_bytes >= 0, "wsae_probe_forward: workspace_bytes must not be negative (got %lld)",
                 (long long)workspace_bytes);
    (void)workspace;  // (wsae_probe_forward_workspace_bytes is 0: one launch that keeps nothing)
    if (n_rows == 0) return WSAE_OK;
    FwdArgs a = {vals, idx, seg, labels, col_of, W, bias, class_weight, n_rows, ldw, lde, k, hidden, lag, n_classes, err,
                 row_loss, (unsigned long long*)n_used, (unsigned long long*)n_correct, (unsigned long long*)loss_q,
                 (unsigned long long*)confusion};
    const int64_t blocks = ceil_div64(n_rows, PB_FWD_BLOCK / 64);
    const int grid = (int)(blocks < PB_FWD_MAX_BLOCKS ? blocks : PB_FWD_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    if (n_classes <= 64) probe_forward_kernel<1><<<grid, PB_FWD_BLOCK, 0, st>>>(a);
    else if (n_classes <= 128) probe_forward_kernel<2><<<grid, PB_FWD_BLOCK, 0, st>>>(a);
    else if (n_classes <= 256) probe_forward_kernel<4><<<grid, PB_FWD_BLOCK, 0, st>>>(a);
    else probe_forward_kernel<16><<<grid, PB_FWD_BLOCK, 0, st>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_probe_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_classes, int64_t cap) {
    return n_rows >= 0 && n_rows <= INT_MAX && n_cols >= 1 && n_classes >= 1 && n_classes <= WSAE_PROBE_MAX_CLASSES && cap >= 0
               ? bwd_ws(n_rows, n_cols, n_classes, cap).bytes
               : -1;
}

extern "C" int wsae_probe_backward(const int64_t* col_ptr, const int32_t* t_row, const float* t_val, int64_t cap, int32_t n_cols,
                                   const float* err, int64_t lde, int32_t n_classes, int64_t n_rows, double* gW, double* gb,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(col_ptr && err && gW && gb, "wsae_probe_backward: null pointer");
    CW_REQUIRE_ROWS("wsae_probe_backward", n_rows);
    WSAE_REQUIRE(n_cols >= 1, "wsae_probe_backward: n_cols must be positive (got %d)", n_cols);
    PB_REQUIRE_CLASSES("wsae_probe_backward", n_classes);
    CW_REQUIRE_LISTS("wsae_probe_backward", cap, t_row, t_val);
    WSAE_REQUIRE(lde >= n_classes, "wsae_probe_backward: lde %lld is smaller than the %d classes", (long long)lde, n_classes);
    const BwdWs w = bwd_ws(n_rows, n_cols, n_classes, cap);
    WSAE_REQUIRE_WORKSPACE("wsae_probe_backward", workspace, workspace_bytes, w.bytes, n_rows);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_probe_backward", workspace, 8);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    int64_t* job_ptr = (int64_t*)((char*)workspace + w.off_jobs);
    double* part = (double*)((char*)workspace + w.off_part);
    double* bpart = (double*)((char*)workspace + w.off_bpart);
    const int c_tiles = ceil_div(n_classes, 64);
    probe_offsets_kernel<true><<<1, 1024, 0, st>>>(col_ptr, n_cols, cap, job_ptr, nullptr);
    const int64_t jobs = w.max_jobs * c_tiles;
    probe_partial_kernel<<<(int)(jobs < PB_MAX_BLOCKS ? jobs : PB_MAX_BLOCKS), 64, 0, st>>>(
        col_ptr, t_row, t_val, cap, n_cols, job_ptr, err, lde, n_classes, n_rows, c_tiles, part);
    probe_sum_kernel<<<(int)ceil_div64((int64_t)n_cols * n_classes, 256), 256, 0, st>>>(job_ptr, n_cols, n_classes, part, gW);
    const int64_t bjobs = w.row_chunks * c_tiles;
    probe_bias_partial_kernel<<<(int)(bjobs < PB_MAX_BLOCKS ? bjobs : PB_MAX_BLOCKS), 64, 0, st>>>(err, lde, n_classes, n_rows,
                                                                                                 c_tiles, w.row_chunks, bpart);
    probe_bias_sum_kernel<<<c_tiles, 64, 0, st>>>(bpart, n_classes, w.row_chunks, gb);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
