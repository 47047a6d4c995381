// The cold plumbing of the analyses that regroup a compact code into per-key lists: count, scan,
// offsets, scatter, merge.  Two schemes use it.
//   Chunked (wsae_sta.hip, wsae_probe.hip): the rows are cut into chunks (chunk_plan), a walk counts per (chunk, column),
//   chunk_scan_kernel turns every column of that table into its exclusive prefix over the chunks and the list lengths,
//   list_offsets turns the lengths into int64 list offsets, and a second walk scatters.  The walks, their row loops and
//   their entry rules stay in their files.
//   Flat (wsae_feature_topk.hip, wsae_profile.hip): a histogram per list in the head of the workspace (list_head),
//   count_scan_kernel for int32 offsets and cursors, a scatter with atomic cursors, and one wave per list that merges
//   the new entries into a sorted list held one element per lane.  The merges keep their own text: a shared insertion
//   step changed the instructions of both (profiles/list_plumbing_note.md).
// The two kernels are templates, so a file emits only the ones it launches.
#pragma once
#include "wsae_codewalk.h"

namespace {

// ---- chunked -------------------------------------------------------------------------------------------------------------
constexpr int CHUNKS_AT_MOST = 1024;     // rows of the count table
constexpr int CHUNK_ROWS_AT_LEAST = 64;  // a chunk is no shorter

struct ChunkPlan {
    int64_t chunk_rows;
    int n_chunks;
};

inline ChunkPlan chunk_plan(int64_t n_rows) {
    ChunkPlan c;
    c.chunk_rows = ceil_div64(n_rows, CHUNKS_AT_MOST);
    if (c.chunk_rows < CHUNK_ROWS_AT_LEAST) c.chunk_rows = CHUNK_ROWS_AT_LEAST;
    c.n_chunks = (int)ceil_div64(n_rows, c.chunk_rows);
    if (c.n_chunks < 1) c.n_chunks = 1;
    return c;
}

// table[ch][c] := the entries of column c in the chunks before ch; lens[c] := all of them
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void chunk_scan_kernel(int32_t* __restrict__ table, int n_chunks, int n_cols,
                                                           int32_t* __restrict__ lens) {
    const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n_cols) return;
    int run = 0;
#pragma unroll 8
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int n = table[(int64_t)ch * n_cols + c];
        table[(int64_t)ch * n_cols + c] = run;
        run += n;
    }
    lens[c] = run;
}

// The body of an offsets kernel, one workgroup of 1024 threads: a.out[p] = the sum of a.len(p') over p' < p, for the a.n
// lists of the policy A, which says what a length is.  A::TOTAL: out has an element n for the sum of all lengths, which
// also goes to *a.total when given.  A::CLASSES: the lists are ordered by the class of their length too (a.count(cls, p)
// before the class offsets are taken, a.place(cls, p) after).  The __global__ function around it stays in its file, three
// lines: it gives the pointers their __restrict__, which a struct's fields do not carry.
template <class A>
__device__ __forceinline__ void list_offsets(const A& a) {
    __shared__ long long part[1024];
    __shared__ int cls[33];  // (A::CLASSES)
    const int tid = threadIdx.x;
    const int per = (a.n + 1023) / 1024;
    const int64_t lo64 = (int64_t)tid * per;
    const int lo = lo64 < a.n ? (int)lo64 : a.n;
    const int hi = lo64 + per < a.n ? (int)(lo64 + per) : a.n;
    if constexpr (A::CLASSES) {
        if (tid < 33) cls[tid] = 0;
        __syncthreads();
    }
    long long sum = 0;
    for (int p = lo; p < hi; ++p) {
        sum += a.len(p);
        if constexpr (A::CLASSES) a.count(cls, p);
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int i = 0; i < 1024; ++i) {
            const long long s = part[i];
            part[i] = run;
            run += s;
        }
        if constexpr (A::TOTAL) {
            a.out[a.n] = run;
            if (a.total) a.total[0] = run;
        }
        if constexpr (A::CLASSES) {  // long lists first
            int at = 0;
            for (int b = 32; b >= 0; --b) {
                const int n = cls[b];
                cls[b] = at;
                at += n;
            }
        }
    }
    __syncthreads();
    long long run = part[tid];
    for (int p = lo; p < hi; ++p) {
        const long long n = a.len(p);  // (read before out[p] is written: in and out never alias)
        a.out[p] = run;
        run += n;
        if constexpr (A::CLASSES) a.place(cls, p);
    }
}

// ---- flat ----------------------------------------------------------------------------------------------------------------
// the head of the workspace: cnt [n_lists] | offs [n_lists + 1] | cursor [n_lists], int32, rounded up to 256 B
struct ListHead {
    int32_t* cnt;
    int32_t* offs;
    int32_t* cursor;
    int64_t bytes;
};

inline ListHead list_head(void* workspace, int64_t n_lists) {
    ListHead h;
    h.cnt = (int32_t*)workspace;
    h.offs = h.cnt + n_lists;
    h.cursor = h.offs + n_lists + 1;
    h.bytes = align256((3 * n_lists + 1) * 4);
    return h;
}

// one block: offs[i] = sum of cnt[< i], offs[n] the total; cursor[i] = offs[i]
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void count_scan_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ offs,
                                                           int32_t* __restrict__ cursor, int n) {
    __shared__ int32_t wsum[BLOCK / 64];
    __shared__ int32_t carry;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += BLOCK) {
        const int i = base + t;
        const int32_t c = i < n ? cnt[i] : 0;
        int32_t s = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t u = __shfl_up(s, o, 64);
            if (lane >= o) s += u;
        }
        if (lane == 63) wsum[w] = s;
        __syncthreads();
        int32_t before = carry;
        for (int q = 0; q < w; ++q) before += wsum[q];
        if (i < n) {
            offs[i] = before + s - c;
            cursor[i] = before + s - c;
        }
        __syncthreads();
        if (t == BLOCK - 1) carry = before + s;
        __syncthreads();
    }
    if (t == 0) offs[n] = carry;
}

}  // namespace
