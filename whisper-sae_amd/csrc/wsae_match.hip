// Dictionary comparison: for every row of A the top_n most similar rows of B, as a GEMM whose
// epilogue is the selection - the [rows_a][rows_b] similarity matrix never exists in memory.
//
// Three launches on the caller's stream:
//   stage   one wave per row: (cosine) 1 / max(|row|, 1e-12) in fp32, scale, (BF16 mode) round once to bf16; the staged
//           copies have rows rounded up to 128 and K rounded up to the MFMA slab, both with zeros, so the contraction
//           needs no predicate on its loads
//   gemm    workgroup = 128 rows of A x one split of B's 128-row tiles.  The product is computed TRANSPOSED (B rows are
//           the MFMA rows, A rows the MFMA columns): in the 32 x 32 C layout a lane then owns ONE row of A per column
//           tile of the wave (two per wave tile), and keeps that row's running top-n sorted in registers over all of the
//           split's tiles.  A column tile first costs one max over the lane's 32 values per list; only where some lane's
//           maximum reaches its current n-th value are the values spilled to LDS and inserted.  A row's four partial lists
//           (two waves x two half-waves) are merged through LDS at the end of the block.
//   merge   one thread per row of A folds the splits' lists and writes the first top_n entries
// Order everywhere: value descending, then index ascending.  It is total, so what is kept never depends on which tile,
// split or lane saw a candidate first.
#include <limits.h>
#include <math.h>

#include "wsae_mfma.h"
#include "wsae_toplist.h"

namespace {

constexpr int MT_TARGET_BLOCKS = 512;     // column splits are added until the grid has about two blocks per CU

struct MatchPlan {
    int64_t rows_a_pad, rows_b_pad;
    int ldw;             // leading dimension of the staged operands (elements)
    int nb;              // list length: top_n rounded up to 4, 8 or 16
    int rtiles, ctiles;  // 128-row tiles of A and of B
    int tps, nsplit;     // column tiles per split, splits
    int64_t off_a, off_b, off_cv, off_ci, total;
};

// false: arguments outside the documented range (no message: the callers word their own)
bool mt_plan(int64_t rows_a, int64_t rows_b, int dim, int top_n, int precision, MatchPlan* p) {
    if (rows_a < 1 || rows_b < 1 || rows_a > INT_MAX - 256 || rows_b > INT_MAX - 256) return false;
    if (dim < 32 || dim > 2048 || dim % 32) return false;
    if (top_n < 1 || top_n > WSAE_MATCH_MAX_N) return false;
    if (precision != WSAE_PREC_BF16 && precision != WSAE_PREC_FP32) return false;
    p->rows_a_pad = (rows_a + 127) / 128 * 128;
    p->rows_b_pad = (rows_b + 127) / 128 * 128;
    const int esz = precision == WSAE_PREC_BF16 ? 2 : 4;
    p->ldw = precision == WSAE_PREC_BF16 ? (dim + 63) / 64 * 64 : dim;
    p->nb = top_n <= 4 ? 4 : top_n <= 8 ? 8 : 16;
    p->rtiles = (int)(p->rows_a_pad / 128);
    p->ctiles = (int)(p->rows_b_pad / 128);
    int want = (MT_TARGET_BLOCKS + p->rtiles - 1) / p->rtiles;
    if (want > p->ctiles) want = p->ctiles;
    p->tps = (p->ctiles + want - 1) / want;
    p->nsplit = (p->ctiles + p->tps - 1) / p->tps;
    p->off_a = 0;
    p->off_b = align256(p->off_a + p->rows_a_pad * p->ldw * esz);
    p->off_cv = align256(p->off_b + p->rows_b_pad * p->ldw * esz);
    p->off_ci = align256(p->off_cv + p->rows_a_pad * p->nsplit * p->nb * 4);
    p->total = align256(p->off_ci + p->rows_a_pad * p->nsplit * p->nb * 4);
    return true;
}

__device__ __forceinline__ void mt_store4(float* d, float4 v) { *(float4*)d = v; }
__device__ __forceinline__ void mt_store4(bf16_t* d, float4 v) {
    bf16x4 o;
    o[0] = (bf16_t)v.x; o[1] = (bf16_t)v.y; o[2] = (bf16_t)v.z; o[3] = (bf16_t)v.w;  // round to nearest even
    *(bf16x4*)d = o;
}

// dst [rows_pad][ldw]: row r < rows = src row r (COSINE: times 1 / max(|row|, 1e-12)), everything else zero
template <typename T, bool COSINE>
__global__ __launch_bounds__(256) void match_stage_kernel(const float* __restrict__ src, int64_t ld, int rows, int64_t rows_pad,
                                                          int dim, int ldw, T* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_pad) return;  // (wave-uniform)
    T* d = dst + row * ldw;
    const int nc = dim >> 2, ncw = ldw >> 2;
    if (row >= rows) {
        for (int c = lane; c < ncw; c += 64) mt_store4(d + 4 * c, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    const float4* s = (const float4*)(src + row * ld);
    float inv = 1.0f;
    if (COSINE) {
        float ss = 0.f;
        for (int c = lane; c < nc; c += 64) {
            const float4 v = s[c];
            ss = fmaf(v.x, v.x, ss);
            ss = fmaf(v.y, v.y, ss);
            ss = fmaf(v.z, v.z, ss);
            ss = fmaf(v.w, v.w, ss);
        }
        ss = wave_sum(ss);
        inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    for (int c = lane; c < ncw; c += 64) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < nc) {
            v = s[c];
            if (COSINE) {
                v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
            }
        }
        mt_store4(d + 4 * c, v);
    }
}

// As [rows_a_pad][ldw], Bs [rows_b_pad][ldw] staged operands; block = (row tile, column split), blockIdx.x = rt * nsplit + sp.
// cand_val / cand_idx [rows_a_pad][nsplit][NB]: this split's sorted list of every row of the tile.
template <typename T, int NB>
__global__ __launch_bounds__(256) void match_gemm_topn_kernel(const T* __restrict__ As, const T* __restrict__ Bs, int ldw,
                                                              int rows_b, int tps, int ctiles, int nsplit, int exclude_self,
                                                              float* __restrict__ cand_val, int32_t* __restrict__ cand_idx) {
    constexpr int KT = Mfma<T>::KT;
    __shared__ __attribute__((aligned(16))) char lds[2 * TILE_LDS_BYTES];
    static_assert(NB * 2 * 128 * 8 <= 2 * TILE_LDS_BYTES && 4 * 32 * 64 * 4 <= 2 * TILE_LDS_BYTES, "epilogue scratch must fit");
    char* Lb = lds;                   // image of B's tile: the MFMA rows
    char* La = lds + TILE_LDS_BYTES;  // image of A's tile: the MFMA columns
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, r = lane & 31, h = lane >> 5;
    const int rt = blockIdx.x / nsplit, sp = blockIdx.x - rt * nsplit;
    const int ct0 = sp * tps, ct1 = min(ct0 + tps, ctiles);
    const int nk = ldw / KT;

    float lv[2][NB];
    int li[2][NB];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            lv[ni][p] = -INFINITY;
            li[ni][p] = MT_EMPTY;
        }
    const int arl0 = wn * 64 + r;  // this lane's row inside the tile, list 0 (list 1: + 32)
    float* dump = (float*)lds + w * (32 * 64) + lane;  // [site 0..31][lane], private to the wave

    SlabRegs<T> ra, rb;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mi][ni][q] = 0.f;

    const int iters = (ct1 - ct0) * nk;
    int ct = ct0, kk = 0;
    slab_load_fast<T>(ra, As, ldw, rt * 128, INT_MAX, 0, tid);
    slab_load_fast<T>(rb, Bs, ldw, ct0 * 128, INT_MAX, 0, tid);
    for (int it = 0; it < iters; ++it) {
        slab_store<T>(ra, La, tid);
        slab_store<T>(rb, Lb, tid);
        __syncthreads();
        int nkk = kk + 1, nct = ct;
        if (nkk == nk) {
            nkk = 0;
            ++nct;
        }
        if (it + 1 < iters) {  // the next slab travels underneath this one's MFMAs (and the tile's epilogue)
            slab_load_fast<T>(ra, As, ldw, rt * 128, INT_MAX, nkk * KT, tid);
            slab_load_fast<T>(rb, Bs, ldw, nct * 128, INT_MAX, nkk * KT, tid);
        }
        Mfma<T>::slab(Lb, La, wm * 64, wn * 64, lane, acc);
        __syncthreads();
        if (kk == nk - 1) {
            // acc[mi][ni][q] = sim(row rt*128 + arl0 + 32 ni of A, column cbase + 32 mi + (q&3) + 8 (q>>2) of B)
            const int cbase = ct * 128 + wm * 64 + 4 * h;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                float m = acc[0][ni][0];
#pragma unroll
                for (int s = 1; s < 32; ++s) m = fmaxf(m, acc[s >> 4][ni][s & 15]);
                if (__ballot(m >= lv[ni][NB - 1]) != 0ull) {
                    const int arow = rt * 128 + arl0 + 32 * ni;
                    uint32_t mask = 0;
#pragma unroll
                    for (int s = 0; s < 32; ++s) {
                        const float v = acc[s >> 4][ni][s & 15];
                        const int col = cbase + 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2);
                        const bool ok = col < rows_b && !(exclude_self && col == arow) && v >= lv[ni][NB - 1];
                        mask |= (ok ? 1u : 0u) << s;
                        dump[s * 64] = v;
                    }
                    while (mask) {
                        const int s = __ffs((int)mask) - 1;
                        mask &= mask - 1;
                        const int col = cbase + 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2);
                        mt_insert<NB>(lv[ni], li[ni], dump[s * 64], col);
                    }
                }
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[mi][ni][q] = 0.f;
            __syncthreads();  // the dump used the operand images
        }
        kk = nkk;
        ct = nct;
    }

    // a row's four lists (wm x h) -> one: [p][src][row of the tile], first the wm = 1 waves' into the wm = 0 waves',
    // then the upper half-wave's into the lower one's
    float* mv = (float*)lds;
    int* mx = (int*)(lds + NB * 2 * 128 * 4);
    if (wm == 1) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                mv[(p * 2 + h) * 128 + arl0 + 32 * ni] = lv[ni][p];
                mx[(p * 2 + h) * 128 + arl0 + 32 * ni] = li[ni][p];
            }
    }
    __syncthreads();
    if (wm == 0) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            for (int p = 0; p < NB; ++p) {
                const int ix = mx[(p * 2 + h) * 128 + arl0 + 32 * ni];
                if (ix != MT_EMPTY) mt_insert<NB>(lv[ni], li[ni], mv[(p * 2 + h) * 128 + arl0 + 32 * ni], ix);
            }
    }
    __syncthreads();
    if (wm == 0 && h == 1) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                mv[(p * 2) * 128 + arl0 + 32 * ni] = lv[ni][p];
                mx[(p * 2) * 128 + arl0 + 32 * ni] = li[ni][p];
            }
    }
    __syncthreads();
    if (wm == 0 && h == 0) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            for (int p = 0; p < NB; ++p) {
                const int ix = mx[(p * 2) * 128 + arl0 + 32 * ni];
                if (ix != MT_EMPTY) mt_insert<NB>(lv[ni], li[ni], mv[(p * 2) * 128 + arl0 + 32 * ni], ix);
            }
            const int64_t o = (((int64_t)rt * 128 + arl0 + 32 * ni) * nsplit + sp) * NB;  // (padded rows exist in the workspace)
#pragma unroll
            for (int p = 0; p < NB; p += 4) {
                *(float4*)(cand_val + o + p) = make_float4(lv[ni][p], lv[ni][p + 1], lv[ni][p + 2], lv[ni][p + 3]);
                *(int4*)(cand_idx + o + p) = make_int4(li[ni][p], li[ni][p + 1], li[ni][p + 2], li[ni][p + 3]);
            }
        }
    }
}

// one thread per row of A: the splits' lists -> out_val / out_idx [rows_a][top_n]; unused slots leave as (-inf, -1)
template <int NB>
__global__ __launch_bounds__(64) void match_merge_kernel(const float* __restrict__ cand_val, const int32_t* __restrict__ cand_idx,
                                                         int rows_a, int nsplit, int top_n, float* __restrict__ out_val,
                                                         int32_t* __restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= rows_a) return;
    float lv[NB];
    int li[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        lv[p] = -INFINITY;
        li[p] = MT_EMPTY;
    }
    const float4* cv = (const float4*)(cand_val + i * nsplit * NB);
    const int4* ci = (const int4*)(cand_idx + i * nsplit * NB);
    for (int c = 0; c < nsplit * (NB / 4); ++c) {
        const float4 v = cv[c];
        const int4 x = ci[c];
        if (x.x != MT_EMPTY && v.x >= lv[NB - 1]) mt_insert<NB>(lv, li, v.x, x.x);
        if (x.y != MT_EMPTY && v.y >= lv[NB - 1]) mt_insert<NB>(lv, li, v.y, x.y);
        if (x.z != MT_EMPTY && v.z >= lv[NB - 1]) mt_insert<NB>(lv, li, v.z, x.z);
        if (x.w != MT_EMPTY && v.w >= lv[NB - 1]) mt_insert<NB>(lv, li, v.w, x.w);
    }
#pragma unroll
    for (int p = 0; p < NB; ++p)
        if (p < top_n) {
            out_val[i * top_n + p] = lv[p];
            out_idx[i * top_n + p] = li[p] == MT_EMPTY ? -1 : li[p];
        }
}

template <typename T>
int mt_run(const float* A, int rows_a, int64_t lda, const float* B, int rows_b, int64_t ldb, int dim, int metric, int top_n,
           int exclude_self, float* out_val, int32_t* out_idx, char* ws, const MatchPlan& p, hipStream_t st) {
    T* As = (T*)(ws + p.off_a);
    T* Bs = (T*)(ws + p.off_b);
    float* cv = (float*)(ws + p.off_cv);
    int32_t* ci = (int32_t*)(ws + p.off_ci);
    const int ga = (int)(p.rows_a_pad / 4), gb = (int)(p.rows_b_pad / 4);
    if (metric == WSAE_MATCH_COSINE) {
        match_stage_kernel<T, true><<<ga, 256, 0, st>>>(A, lda, rows_a, p.rows_a_pad, dim, p.ldw, As);
        match_stage_kernel<T, true><<<gb, 256, 0, st>>>(B, ldb, rows_b, p.rows_b_pad, dim, p.ldw, Bs);
    } else {
        match_stage_kernel<T, false><<<ga, 256, 0, st>>>(A, lda, rows_a, p.rows_a_pad, dim, p.ldw, As);
        match_stage_kernel<T, false><<<gb, 256, 0, st>>>(B, ldb, rows_b, p.rows_b_pad, dim, p.ldw, Bs);
    }
    WSAE_LAUNCH_CHECK();
    const int grid = p.rtiles * p.nsplit, gm = ceil_div(rows_a, 64);
#define MT_LAUNCH(NB_)                                                                                                     \
    match_gemm_topn_kernel<T, NB_><<<grid, 256, 0, st>>>(As, Bs, p.ldw, rows_b, p.tps, p.ctiles, p.nsplit, exclude_self, cv, ci); \
    WSAE_LAUNCH_CHECK();                                                                                                   \
    match_merge_kernel<NB_><<<gm, 64, 0, st>>>(cv, ci, rows_a, p.nsplit, top_n, out_val, out_idx)
    if (p.nb == 4) {
        MT_LAUNCH(4);
    } else if (p.nb == 8) {
        MT_LAUNCH(8);
    } else {
        MT_LAUNCH(16);
    }
#undef MT_LAUNCH
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

}  // namespace

extern "C" int64_t wsae_match_workspace_bytes(int32_t rows_a, int32_t rows_b, int32_t dim, int32_t top_n, int32_t precision) {
    MatchPlan p;
    return mt_plan(rows_a, rows_b, dim, top_n, precision, &p) ? p.total : -1;
}

extern "C" int wsae_match_rows(const float* A, int32_t rows_a, int64_t lda, const float* B, int32_t rows_b, int64_t ldb,
                               int32_t dim, int32_t metric, int32_t precision, int32_t top_n, int32_t exclude_self,
                               float* out_val, int32_t* out_idx, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(A && B && out_val && out_idx && workspace, "wsae_match_rows: null pointer");
    WSAE_REQUIRE(rows_a >= 1 && rows_b >= 1 && rows_a <= INT_MAX - 256 && rows_b <= INT_MAX - 256,
                 "wsae_match_rows: need 1 <= rows_a, rows_b <= 2^31 - 257 (got %d, %d)", rows_a, rows_b);
    WSAE_REQUIRE(dim >= 32 && dim <= 2048 && dim % 32 == 0, "wsae_match_rows: dim must be a multiple of 32, at most 2048 (got %d)",
                 dim);
    WSAE_REQUIRE(top_n >= 1 && top_n <= WSAE_MATCH_MAX_N, "wsae_match_rows: need 1 <= top_n <= %d (got %d)", WSAE_MATCH_MAX_N,
                 top_n);
    WSAE_REQUIRE(metric == WSAE_MATCH_COSINE || metric == WSAE_MATCH_DOT, "wsae_match_rows: unknown metric %d", metric);
    WSAE_REQUIRE(precision == WSAE_PREC_BF16 || precision == WSAE_PREC_FP32, "wsae_match_rows: unknown precision %d", precision);
    WSAE_REQUIRE(lda >= dim && ldb >= dim && lda % 4 == 0 && ldb % 4 == 0,
                 "wsae_match_rows: lda, ldb must be multiples of 4 and >= dim (got %lld, %lld, dim %d)", (long long)lda,
                 (long long)ldb, dim);
    WSAE_REQUIRE(((uintptr_t)A | (uintptr_t)B | (uintptr_t)workspace) % 16 == 0,
                 "wsae_match_rows: A, B and the workspace must be 16-byte aligned");
    MatchPlan p;
    WSAE_REQUIRE(mt_plan(rows_a, rows_b, dim, top_n, precision, &p), "wsae_match_rows: unsupported shape");
    WSAE_REQUIRE(workspace_bytes >= p.total, "wsae_match_rows: workspace too small (%lld < %lld)", (long long)workspace_bytes,
                 (long long)p.total);
    hipStream_t st = (hipStream_t)stream;
    if (precision == WSAE_PREC_BF16)
        return mt_run<bf16_t>(A, rows_a, lda, B, rows_b, ldb, dim, metric, top_n, exclude_self, out_val, out_idx,
                              (char*)workspace, p, st);
    return mt_run<float>(A, rows_a, lda, B, rows_b, ldb, dim, metric, top_n, exclude_self, out_val, out_idx, (char*)workspace,
                         p, st);
}
