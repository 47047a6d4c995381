// Group effect sizes: which features separate two groups of utterances, and how surely.
//
//   pool    segment (utterance) pooling of a compact code: per (segment, feature) the fp32 sum of the active values in
//           ascending row order, starting from the stored value, plus optional firing counts and the rows per segment.
//           Three launches: the per-segment row bounds of the call (seg_bounds of wsae_codewalk.h: reset, then found
//           with integer atomics, one per run of equal segment ids), and then one wave owns a (segment, tile of
//           PL_TILE features) job: the tile's sums sit
//           in LDS, the wave walks the segment's rows in order (four rows of loads in flight), one lane per entry.  A
//           one-byte LDS tag per column tells whether two entries of one pass name the same column (a TopK code never
//           does); only then the pass is replayed lane by lane, i.e. in entry order.  One owner per cell and one order:
//           no float atomics, and the same bits for any grid, any split of a segment over calls.
//   effect  Cohen's d / Hedges' g of two groups of segments in fp64, with bootstrap percentile intervals.  Launches:
//           the per-segment selector and the group sizes; (with replicates) the clamped weights transposed to
//           [segment][replicate] and the replicate totals N; the two-pass point statistics (16 columns x 16 segment
//           slices per workgroup, slices combined in a fixed order); the bootstrap: a workgroup of 512 threads owns
//           four features and ALL replicates, a thread RJ replicates x 4 features x 2 groups x (S1, S2) in registers,
//           walks the segments in ascending order (z and z^2 staged in LDS 64 segments at a time, the thread's weights
//           read straight from the transposed copy, eight segments of loads in flight), forms d* per replicate, sorts
//           the four columns in LDS (bitonic, dropped replicates = +inf at the end) and writes the quantiles and the
//           standard error.  The [R, H] replicate matrix is never written.  Every (r, f) sum runs over the segments in
//           one order with explicit fma, so a column's result does not depend on its tile, its neighbours or ld.
#include <limits.h>
#include <math.h>

#include "wsae_codewalk.h"

namespace {

// ---- pooling ------------------------------------------------------------------------------------------------------------
constexpr int PL_TILE = 3072;         // features per job: 12 KB of sums (+ 12 KB of counts) + 3 KB of tags per wave
constexpr int PL_MAX_BLOCKS = 2560;   // ten resident single-wave workgroups per CU by LDS; more jobs than that: grid-stride
constexpr int PL_ROWS = 4;            // rows whose loads are issued before the first of them is accumulated

// one pass of at most 64 entries (lane = entry) into the wave's tile
template <bool CNT>
__device__ __forceinline__ void pool_pass(bool in, int c, float v, lds_f32* acc, lds_i32* cn, lds_u8* tag, int lane) {
    if (in) tag[c] = (uint8_t)lane;
    const bool lost = in && tag[c] != (uint8_t)lane;  // another entry of this pass names the same column
    if (__ballot(lost) == 0ull) {
        if (in) {
            acc[c] = acc[c] + v;
            if (CNT) cn[c] = cn[c] + 1;
        }
    } else {
        for (unsigned long long m = __ballot(in); m; m &= m - 1ull) {  // in entry order
            if (lane == __builtin_ctzll(m)) {
                acc[c] = acc[c] + v;
                if (CNT) cn[c] = cn[c] + 1;
            }
        }
    }
}

// NP: passes of 64 entries per row (k <= 64 * NP)
template <bool CNT, int NP>
__global__ __launch_bounds__(64) void pool_accum_kernel(const float* __restrict__ vals, const int32_t* __restrict__ idx, int k,
                                                        const int32_t* __restrict__ seg, int n_seg, int f_lo, int f_cols,
                                                        int n_tiles, const int32_t* __restrict__ first,
                                                        const int32_t* __restrict__ last, float* __restrict__ sum,
                                                        int32_t* __restrict__ cnt, int64_t ld, int32_t* __restrict__ seg_rows) {
    extern __shared__ float pl_smem[];
    lds_f32* acc = (lds_f32*)pl_smem;
    lds_i32* cn = (lds_i32*)(pl_smem + PL_TILE);
    lds_u8* tag = (lds_u8*)(pl_smem + (CNT ? 2 : 1) * PL_TILE);
    const int lane = threadIdx.x;
    const int64_t n_jobs = (int64_t)n_seg * n_tiles;
    for (int64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const int s = (int)(job / n_tiles), t = (int)(job - (int64_t)s * n_tiles);
        const int r0 = first[s], r1 = last[s];
        if (r0 > r1) continue;  // the segment has no row in this call (wave-uniform)
        const int c_lo = t * PL_TILE;
        const int width = f_cols - c_lo < PL_TILE ? f_cols - c_lo : PL_TILE;
        const int t_lo = f_lo + c_lo;
        float* gs = sum + (int64_t)s * ld + c_lo;
        int32_t* gc = CNT ? cnt + (int64_t)s * ld + c_lo : nullptr;
        for (int c = lane; c < width; c += 64) {
            acc[c] = gs[c];
            if (CNT) cn[c] = gc[c];
        }
        int rows_here = 0;
        for (int64_t row = r0; row <= r1; row += PL_ROWS) {
            float v[PL_ROWS][NP];
            int ix[PL_ROWS][NP];
            int sg[PL_ROWS];
#pragma unroll
            for (int u = 0; u < PL_ROWS; ++u) {
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
            for (int u = 0; u < PL_ROWS; ++u) {
                if (sg[u] != s) continue;  // a padding frame inside the segment's range (wave-uniform)
                ++rows_here;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int i = ix[u][p];
                    const bool in = v[u][p] > 0.f && i >= t_lo && i - t_lo < width;  // (t_lo + width <= hidden)
                    pool_pass<CNT>(in, in ? i - t_lo : 0, v[u][p], acc, cn, tag, lane);
                }
            }
        }
        for (int c = lane; c < width; c += 64) {
            gs[c] = acc[c];
            if (CNT) gc[c] = cn[c];
        }
        if (t == 0 && lane == 0) seg_rows[s] += rows_here;
    }
}

// ---- effect sizes -------------------------------------------------------------------------------------------------------
constexpr int GE_FT = 4;         // features per workgroup of the bootstrap
constexpr int GE_THREADS = 512;  // ... and its threads: RJ replicates each, RJ = 1, 2 or 4
constexpr int GE_CHUNK = 64;     // segments staged in LDS at a time
constexpr int GE_AHEAD = 8;      // segments whose weights are in flight
constexpr int GE_MAX_SEG = 1 << 20;

__device__ __forceinline__ double ge_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// sel[s] = 0 / 1 for the included members of group a / b, -1 otherwise (and for the padding up to s_pad); the group sizes
__global__ __launch_bounds__(256) void ge_prep_kernel(const int32_t* __restrict__ div, const int32_t* __restrict__ group,
                                                      int n_seg, int s_pad, int32_t* __restrict__ sel,
                                                      int32_t* __restrict__ record) {
    __shared__ int sa[256], sb[256];
    int na = 0, nb = 0;
    for (int s = threadIdx.x; s < s_pad; s += 256) {
        int g = -1;
        if (s < n_seg && (!div || div[s] > 0)) {
            const int l = group[s];
            if (l == 0 || l == 1) g = l;
        }
        sel[s] = g;
        na += g == 0;
        nb += g == 1;
    }
    sa[threadIdx.x] = na;
    sb[threadIdx.x] = nb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i) {
            na += sa[i];
            nb += sb[i];
        }
        record[0] = na;
        record[1] = nb;
        record[2] = 0;
    }
}

// boot [R][n_seg] -> wT [s_pad][r_pad], negative weights and the padding as 0
__global__ __launch_bounds__(256) void ge_transpose_kernel(const int16_t* __restrict__ boot, int R, int n_seg,
                                                           int16_t* __restrict__ wT, int r_pad) {
    __shared__ int16_t tile[32][33];
    const int s0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, s = s0 + threadIdx.x;
        int16_t w = 0;
        if (r < R && s < n_seg) w = boot[(int64_t)r * n_seg + s];
        tile[i][threadIdx.x] = w < 0 ? (int16_t)0 : w;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) wT[(int64_t)(s0 + i) * r_pad + r0 + threadIdx.x] = tile[threadIdx.x][i];
}

// N of replicate r in each group (integer sums, exact as doubles): nab[r], nab[r_pad + r]; 0 for the padding replicates
__global__ __launch_bounds__(256) void ge_totals_kernel(const int16_t* __restrict__ boot, int R, int n_seg,
                                                        const int32_t* __restrict__ sel, double* __restrict__ nab, int r_pad) {
    __shared__ long long sa[256], sb[256];
    const int r = blockIdx.x;
    long long na = 0, nb = 0;
    if (r < R)
        for (int s = threadIdx.x; s < n_seg; s += 256) {
            const int w = boot[(int64_t)r * n_seg + s], g = sel[s];
            if (w > 0) {
                na += g == 0 ? w : 0;
                nb += g == 1 ? w : 0;
            }
        }
    sa[threadIdx.x] = na;
    sb[threadIdx.x] = nb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i) {
            na += sa[i];
            nb += sb[i];
        }
        nab[r] = (double)na;
        nab[r_pad + r] = (double)nb;
    }
}

__device__ __forceinline__ double ge_value(const float* __restrict__ X, int64_t ld, const int32_t* __restrict__ div, int s, int f) {
    const double x = (double)X[(int64_t)s * ld + f];
    return div ? x / (double)div[s] : x;
}

__device__ __forceinline__ double ge_cohen_d(double ma, double va, double na, double mb, double vb, double nb) {
    const double sp = sqrt(((na - 1.0) * va + (nb - 1.0) * vb) / (na + nb - 2.0));
    return sp == 0.0 ? 0.0 : (ma - mb) / sp;
}

// point statistics, two passes.  Thread (c, j): column 16 * block + c, segments j, j + 16, ...; the 16 slices of a column
// are combined in the order of j.
__global__ __launch_bounds__(256) void ge_point_kernel(const float* __restrict__ X, int64_t ld, const int32_t* __restrict__ div,
                                                       const int32_t* __restrict__ sel, int n_seg, int f_cols, int R,
                                                       const int32_t* __restrict__ record, double* __restrict__ mean_a,
                                                       double* __restrict__ mean_b, double* __restrict__ out_d,
                                                       double* __restrict__ out_g, double* __restrict__ ci_lo,
                                                       double* __restrict__ ci_hi, double* __restrict__ se) {
    __shared__ double pa[16][16], pb[16][16];
    __shared__ double ma_s[16], mb_s[16];
    const int c = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int f = blockIdx.x * 16 + c;
    const bool live = f < f_cols;
    const int n_a = record[0], n_b = record[1];
    if (n_a < 2 || n_b < 2) {  // (uniform over the grid)
        if (j == 0 && live) {
            const double q = ge_nan();
            mean_a[f] = q; mean_b[f] = q; out_d[f] = q; out_g[f] = q; ci_lo[f] = q; ci_hi[f] = q; se[f] = q;
        }
        return;
    }
    const double na = (double)n_a, nb = (double)n_b;
    double a = 0.0, b = 0.0;
    if (live)
        for (int s = j; s < n_seg; s += 16) {
            const int g = sel[s];
            if (g < 0) continue;
            const double x = ge_value(X, ld, div, s, f);
            if (g == 0) a += x; else b += x;
        }
    pa[j][c] = a;
    pb[j][c] = b;
    __syncthreads();
    if (j == 0) {
        for (int i = 1; i < 16; ++i) {
            a += pa[i][c];
            b += pb[i][c];
        }
        ma_s[c] = a / na;
        mb_s[c] = b / nb;
    }
    __syncthreads();
    const double ma = ma_s[c], mb = mb_s[c];
    a = 0.0;
    b = 0.0;
    if (live)
        for (int s = j; s < n_seg; s += 16) {
            const int g = sel[s];
            if (g < 0) continue;
            const double x = ge_value(X, ld, div, s, f);
            if (g == 0) a = fma(x - ma, x - ma, a); else b = fma(x - mb, x - mb, b);
        }
    pa[j][c] = a;
    pb[j][c] = b;
    __syncthreads();
    if (j == 0 && live) {
        for (int i = 1; i < 16; ++i) {
            a += pa[i][c];
            b += pb[i][c];
        }
        const double d = ge_cohen_d(ma, a / (na - 1.0), na, mb, b / (nb - 1.0), nb);
        mean_a[f] = ma;
        mean_b[f] = mb;
        out_d[f] = d;
        out_g[f] = d * (1.0 - 3.0 / (4.0 * (na + nb) - 9.0));
        if (R == 0) {
            ci_lo[f] = ge_nan();
            ci_hi[f] = ge_nan();
            se[f] = ge_nan();
        }
    }
}

// the q quantile of the ascending x[0 .. n), n >= 1: linear interpolation at (n - 1) q, in numpy's form
__device__ __forceinline__ double ge_quantile(const double* x, int n, double q) {
    const double pos = (double)(n - 1) * q;
    int lo = (int)floor(pos);
    if (lo > n - 1) lo = n - 1;
    const int hi = lo + 1 < n ? lo + 1 : n - 1;
    const double t = pos - (double)lo, a = x[lo], b = x[hi], diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

template <int RJ>
struct GeWeights;
template <>
struct GeWeights<1> { typedef int16_t type; };
template <>
struct GeWeights<2> { typedef short2 type; };
template <>
struct GeWeights<4> { typedef short4 type; };

template <int RJ>
__device__ __forceinline__ void ge_accumulate(double (&s1)[RJ][GE_FT], double (&s2)[RJ][GE_FT], const int16_t (&w)[RJ],
                                              const double* __restrict__ z) {
    double zz[2 * GE_FT];
#pragma unroll
    for (int i = 0; i < 2 * GE_FT; ++i) zz[i] = z[i];
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
        const double wd = (double)w[j];
#pragma unroll
        for (int f = 0; f < GE_FT; ++f) {
            s1[j][f] = fma(wd, zz[f], s1[j][f]);
            s2[j][f] = fma(wd, zz[GE_FT + f], s2[j][f]);
        }
    }
}

// LDS (doubles): max(GE_FT * rp2, GE_FT * GE_THREADS) - rp2 = R rounded up to a power of two.  Three uses in turn: the
// staging area of the contraction (z, z^2 [GE_CHUNK][2 GE_FT] and the selectors), the tree of the standard error
// [GE_FT][GE_THREADS], the sort buffer [GE_FT][rp2].
template <int RJ>
__global__ __launch_bounds__(GE_THREADS) void ge_boot_kernel(const float* __restrict__ X, int64_t ld,
                                                             const int32_t* __restrict__ div, const int32_t* __restrict__ sel,
                                                             int n_seg, int f_cols, const int16_t* __restrict__ wT,
                                                             const double* __restrict__ nab, int R, int rp2, double alpha,
                                                             const double* __restrict__ mean_a, const double* __restrict__ mean_b,
                                                             double* __restrict__ ci_lo, double* __restrict__ ci_hi,
                                                             double* __restrict__ se, int32_t* __restrict__ record) {
    extern __shared__ double ge_smem[];
    constexpr int r_pad = RJ * GE_THREADS;
    double* zs = ge_smem;                                // [GE_CHUNK][2 * GE_FT]
    int* gsel = (int*)(ge_smem + GE_CHUNK * 2 * GE_FT);  // [GE_CHUNK]
    double* part = ge_smem;                              // [GE_FT][GE_THREADS]
    double* buf = ge_smem;                               // [GE_FT][rp2]
    const int tid = threadIdx.x;
    const int f0 = blockIdx.x * GE_FT;
    // A group with fewer than two members (uniform over the grid): every output is NaN, and ge_point_kernel, launched
    // before this kernel on the same stream, has written them - ci_lo, ci_hi and se included.  That launch order, the
    // means it leaves in mean_a / mean_b and record[0 .. 1] from ge_prep_kernel are all this kernel takes from the others.
    if (record[0] < 2 || record[1] < 2) return;

    double a1[RJ][GE_FT], a2[RJ][GE_FT], b1[RJ][GE_FT], b2[RJ][GE_FT];
#pragma unroll
    for (int j = 0; j < RJ; ++j)
#pragma unroll
        for (int f = 0; f < GE_FT; ++f) a1[j][f] = a2[j][f] = b1[j][f] = b2[j][f] = 0.0;

    typedef typename GeWeights<RJ>::type wvec;
    const wvec* wrow = (const wvec*)wT + tid;  // replicates RJ tid .. RJ tid + RJ - 1 of segment 0
    const int s_pad = (n_seg + GE_CHUNK - 1) / GE_CHUNK * GE_CHUNK;
    for (int s0 = 0; s0 < s_pad; s0 += GE_CHUNK) {
        __syncthreads();
        if (tid < GE_CHUNK * GE_FT) {
            const int ss = tid / GE_FT, ff = tid % GE_FT;
            const int s = s0 + ss, f = f0 + ff;
            const int g = sel[s];  // (sel is padded to s_pad with -1)
            double z = 0.0;
            if (g >= 0 && f < f_cols) z = ge_value(X, ld, div, s, f) - (g == 0 ? mean_a[f] : mean_b[f]);
            zs[ss * 2 * GE_FT + ff] = z;
            zs[ss * 2 * GE_FT + GE_FT + ff] = z * z;
            if (ff == 0) gsel[ss] = g;
        }
        __syncthreads();
        for (int ss = 0; ss < GE_CHUNK; ss += GE_AHEAD) {
            wvec wv[GE_AHEAD];
#pragma unroll
            for (int u = 0; u < GE_AHEAD; ++u) wv[u] = wrow[(int64_t)(s0 + ss + u) * GE_THREADS];
#pragma unroll
            for (int u = 0; u < GE_AHEAD; ++u) {
                const int g = __builtin_amdgcn_readfirstlane(gsel[ss + u]);
                if (g < 0) continue;
                int16_t w[RJ];
                __builtin_memcpy(w, &wv[u], sizeof(w));
                if (g == 0) ge_accumulate<RJ>(a1, a2, w, zs + (ss + u) * 2 * GE_FT);
                else ge_accumulate<RJ>(b1, b2, w, zs + (ss + u) * 2 * GE_FT);
            }
        }
    }

    // d* of the thread's replicates (0 where the replicate is dropped: no term of the sums below)
    double dv[RJ][GE_FT];
    bool ok[RJ];
    int kept = 0;
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
        const int r = tid * RJ + j;
        const double na = nab[r], nb = nab[r_pad + r];
        ok[j] = r < R && na >= 2.0 && nb >= 2.0;
        kept += ok[j];
#pragma unroll
        for (int f = 0; f < GE_FT; ++f) {
            dv[j][f] = 0.0;
            if (ok[j]) {
                const double ma = mean_a[f0 + f < f_cols ? f0 + f : 0], mb = mean_b[f0 + f < f_cols ? f0 + f : 0];
                const double va = fmax(a2[j][f] - a1[j][f] * a1[j][f] / na, 0.0) / (na - 1.0);
                const double vb = fmax(b2[j][f] - b1[j][f] * b1[j][f] / nb, 0.0) / (nb - 1.0);
                dv[j][f] = ge_cohen_d(ma + a1[j][f] / na, va, na, mb + b1[j][f] / nb, vb, nb);
            }
        }
    }
    int* kept_s = (int*)ge_smem;  // [GE_THREADS]: the kept replicates, counted over the threads
    __syncthreads();              // (the last read of the staging area is behind every thread)
    kept_s[tid] = kept;
    __syncthreads();
    for (int s = GE_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) kept_s[tid] += kept_s[tid + s];
        __syncthreads();
    }
    kept = kept_s[0];
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) record[2] = kept;

    // standard error over the kept replicates: mean, then centred squares; a thread's replicates in order, then a tree
    // of fixed shape over the threads
    double mean[GE_FT], sq[GE_FT];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int f = 0; f < GE_FT; ++f) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < RJ; ++j)
                if (ok[j]) acc = pass == 0 ? acc + dv[j][f] : fma(dv[j][f] - mean[f], dv[j][f] - mean[f], acc);
            part[f * GE_THREADS + tid] = acc;
        }
        __syncthreads();
        for (int s = GE_THREADS / 2; s >= 1; s >>= 1) {
            if (tid < s)
#pragma unroll
                for (int f = 0; f < GE_FT; ++f) part[f * GE_THREADS + tid] += part[f * GE_THREADS + tid + s];
            __syncthreads();
        }
#pragma unroll
        for (int f = 0; f < GE_FT; ++f) {
            if (pass == 0) mean[f] = kept ? part[f * GE_THREADS] / (double)kept : 0.0;  // (no replicate kept: se is NaN below)
            else sq[f] = part[f * GE_THREADS];
        }
        __syncthreads();
    }

    // the sort buffer: a dropped replicate and the padding up to rp2 sort to the end
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
        const int r = tid * RJ + j;
        if (r < rp2)
#pragma unroll
            for (int f = 0; f < GE_FT; ++f) buf[f * rp2 + r] = ok[j] ? dv[j][f] : INFINITY;
    }
    __syncthreads();
    const int half = GE_FT * rp2 / 2;
    for (int size = 2; size <= rp2; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            for (int p = tid; p < half; p += GE_THREADS) {
                const int f = p / (rp2 / 2), q = p - f * (rp2 / 2);
                const int i = 2 * stride * (q / stride) + (q % stride), l = i + stride;
                const bool up = (i & size) == 0;
                double* col = buf + f * rp2;
                const double x = col[i], y = col[l];
                if ((x > y) == up) {
                    col[i] = y;
                    col[l] = x;
                }
            }
            __syncthreads();
        }
#pragma unroll
    for (int f = 0; f < GE_FT; ++f)
        if (tid == f && f0 + f < f_cols) {
            const double* col = buf + f * rp2;
            const int o = f0 + f;
            ci_lo[o] = kept >= 1 ? ge_quantile(col, kept, 0.5 * alpha) : ge_nan();
            ci_hi[o] = kept >= 1 ? ge_quantile(col, kept, 1.0 - 0.5 * alpha) : ge_nan();
            se[o] = kept >= 2 ? sqrt(sq[f] / (double)(kept - 1)) : ge_nan();
        }
}

bool ge_args_ok(int n_seg, int f_cols, int n_boot) {
    return n_seg >= 1 && n_seg <= GE_MAX_SEG && f_cols >= 1 && (n_boot == 0 || (n_boot >= 2 && n_boot <= WSAE_BOOT_MAX_R));
}

int ge_rj(int n_boot) { return n_boot <= GE_THREADS ? 1 : n_boot <= 2 * GE_THREADS ? 2 : 4; }

struct GeLayout {
    int s_pad, r_pad;
    int64_t off_nab, off_wt, bytes;
};

GeLayout ge_layout(int n_seg, int n_boot) {
    GeLayout l;
    l.s_pad = (n_seg + GE_CHUNK - 1) / GE_CHUNK * GE_CHUNK;
    l.r_pad = n_boot ? ge_rj(n_boot) * GE_THREADS : 0;
    l.off_nab = (int64_t)l.s_pad * 4;  // (a multiple of 256 bytes)
    l.off_wt = l.off_nab + 2 * (int64_t)l.r_pad * 8;
    l.bytes = l.off_wt + (int64_t)l.s_pad * l.r_pad * 2;
    return l;
}

}  // namespace

extern "C" int64_t wsae_pool_workspace_bytes(int64_t n_rows, int32_t k, int32_t hidden, int32_t n_seg, int32_t f_lo,
                                             int32_t f_cols) {
    const bool ok = code_args_ok(n_rows, k, WSAE_POOL_MAX_K, hidden, f_lo, f_cols) && n_seg >= 1;
    return ok ? 8 * (int64_t)n_seg : -1;  // first and last row per segment
}

extern "C" int wsae_pool_update(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                int64_t n_rows, int32_t n_seg, int32_t f_lo, int32_t f_cols, float* pooled_sum,
                                int32_t* pooled_cnt, int64_t ld, int32_t* seg_rows, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    WSAE_REQUIRE(vals && idx && seg && pooled_sum && seg_rows, "wsae_pool_update: null pointer");
    CW_REQUIRE_K("wsae_pool_update", k, WSAE_POOL_MAX_K);
    WSAE_REQUIRE(hidden >= 1 && n_seg >= 1, "wsae_pool_update: hidden and n_seg must be positive (got %d, %d)", hidden, n_seg);
    CW_REQUIRE_ROWS("wsae_pool_update", n_rows);
    CW_REQUIRE_WINDOW("wsae_pool_update", f_lo, f_cols, hidden);
    WSAE_REQUIRE(ld >= f_cols, "wsae_pool_update: ld %lld < f_cols %d", (long long)ld, f_cols);
    const int64_t need = 8 * (int64_t)n_seg;
    WSAE_REQUIRE_WORKSPACE("wsae_pool_update", workspace, workspace_bytes, need, n_rows);
    if (n_rows == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t* first = (int32_t*)workspace;
    int32_t* last = first + n_seg;
    seg_bounds(seg, n_rows, n_seg, first, last, st);
    const int n_tiles = ceil_div(f_cols, PL_TILE);
    const int64_t n_jobs = (int64_t)n_seg * n_tiles;
    const int grid = (int)(n_jobs < PL_MAX_BLOCKS ? n_jobs : PL_MAX_BLOCKS);
    const size_t lds = (size_t)PL_TILE * (pooled_cnt ? 9 : 5);
#define PL_LAUNCH(CNT_, NP_)                                                                                              \
    pool_accum_kernel<CNT_, NP_><<<grid, 64, lds, st>>>(vals, idx, k, seg, n_seg, f_lo, f_cols, n_tiles, first, last,      \
                                                        pooled_sum, pooled_cnt, ld, seg_rows)
    if (pooled_cnt) {
        if (k <= 64) PL_LAUNCH(true, 1); else PL_LAUNCH(true, 2);
    } else {
        if (k <= 64) PL_LAUNCH(false, 1); else PL_LAUNCH(false, 2);
    }
#undef PL_LAUNCH
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_group_effect_workspace_bytes(int32_t n_seg, int32_t f_cols, int32_t n_boot) {
    return ge_args_ok(n_seg, f_cols, n_boot) ? ge_layout(n_seg, n_boot).bytes : -1;
}

extern "C" int wsae_group_effect(const float* X, int64_t ld, const int32_t* div, const int32_t* group, int32_t n_seg,
                                 int32_t f_cols, const int16_t* boot, int32_t n_boot, double alpha, double* mean_a,
                                 double* mean_b, double* d, double* g, double* ci_lo, double* ci_hi, double* se,
                                 int32_t* record, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(X && group && mean_a && mean_b && d && g && ci_lo && ci_hi && se && record,
                 "wsae_group_effect: null pointer");
    WSAE_REQUIRE(n_seg >= 1 && n_seg <= GE_MAX_SEG, "wsae_group_effect: need 1 <= n_seg <= %d (got %d)", GE_MAX_SEG, n_seg);
    WSAE_REQUIRE(f_cols >= 1, "wsae_group_effect: f_cols must be positive (got %d)", f_cols);
    WSAE_REQUIRE(ld >= f_cols, "wsae_group_effect: ld %lld < f_cols %d", (long long)ld, f_cols);
    WSAE_REQUIRE(boot ? n_boot >= 2 && n_boot <= WSAE_BOOT_MAX_R : n_boot == 0,
                 "wsae_group_effect: need 2 <= replicates <= %d with boot, 0 without (got %d)", WSAE_BOOT_MAX_R, n_boot);
    WSAE_REQUIRE(alpha > 0.0 && alpha < 1.0, "wsae_group_effect: alpha must lie in (0, 1) (got %g)", alpha);
    const GeLayout lay = ge_layout(n_seg, n_boot);
    WSAE_REQUIRE(workspace && workspace_bytes >= lay.bytes, "wsae_group_effect: workspace too small (%lld < %lld)",
                 (long long)(workspace ? workspace_bytes : 0), (long long)lay.bytes);
    WSAE_REQUIRE((uintptr_t)workspace % 16 == 0, "wsae_group_effect: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* sel = (int32_t*)workspace;
    double* nab = (double*)((char*)workspace + lay.off_nab);
    int16_t* wT = (int16_t*)((char*)workspace + lay.off_wt);
    ge_prep_kernel<<<1, 256, 0, st>>>(div, group, n_seg, lay.s_pad, sel, record);
    if (n_boot) {
        ge_transpose_kernel<<<dim3(lay.s_pad / 32, lay.r_pad / 32), dim3(32, 8), 0, st>>>(boot, n_boot, n_seg, wT, lay.r_pad);
        ge_totals_kernel<<<lay.r_pad, 256, 0, st>>>(boot, n_boot, n_seg, sel, nab, lay.r_pad);
    }
    ge_point_kernel<<<ceil_div(f_cols, 16), 256, 0, st>>>(X, ld, div, sel, n_seg, f_cols, n_boot, record, mean_a, mean_b, d, g,
                                                          ci_lo, ci_hi, se);
    if (n_boot) {
        int rp2 = 2;
        while (rp2 < n_boot) rp2 <<= 1;
        const size_t lds = (size_t)GE_FT * (rp2 > GE_THREADS ? rp2 : GE_THREADS) * sizeof(double);  // (at most 64 KB)
        const int grid = ceil_div(f_cols, GE_FT);
#define GE_LAUNCH(RJ_)                                                                                                    \
    ge_boot_kernel<RJ_><<<grid, GE_THREADS, lds, st>>>(X, ld, div, sel, n_seg, f_cols, wT, nab, n_boot, rp2, alpha, mean_a,  \
                                                       mean_b, ci_lo, ci_hi, se, record)
        const int rj = ge_rj(n_boot);
        if (rj == 1) GE_LAUNCH(1); else if (rj == 2) GE_LAUNCH(2); else GE_LAUNCH(4);
#undef GE_LAUNCH
    }
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
