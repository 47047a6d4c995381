// Token alignment: Whisper's word-timestamp recipe - z-score the cross-attention weights of the
// alignment heads over the tokens, median-filter along time, average the heads, negate, dynamic time warping - as two
// kernels whose every bit a sequential loop reproduces (tests/align_oracle.py).
//
// align_cost_kernel: a workgroup owns one utterance and AC_TILE frames plus a halo of p = width / 2 on each side; lanes are
// frames, so the reads along ld_f are coalesced.  Phase 1 builds mean and sd of every (head, column) of the tile in LDS
// (two fp64 each, one sequential chain over the token rows per entry).  Phase 2 walks the token rows, four at a time (one
// per wave), heads innermost: a lane z-scores the value of its column into the wave's row of LDS, takes the `width`
// neighbours back and selects their median with an odd-even transposition network on registers (static indexing), and
// adds it to the fp64 chain of the heads.  z and the medians never reach global memory.  Non-finite values are counted
// per utterance (integer atomics); align_cost_finish_kernel then overwrites the cost of such an utterance with the fill.
//
// align_dtw_kernel: one workgroup per utterance, a wave per strip of 64 token rows, a lane per row.  A wave sweeps the
// frames skewed - at its local step t lane l is at column t - l - so D[i-1][.] comes from the lane above by one DPP
// wave shift, and D[i][j-1] and the diagonal stay in registers.  Time runs in sub-phases of AD_SUB steps with one
// __syncthreads() each: a wave fetches the costs of its next AD_SUB steps coalesced, one sub-phase ahead (the steps hide
// the latency), passes them through LDS, already skewed ([row][step]), and reads them back a lane per row before the
// first step.  Lane 63 leaves the strip's bottom row in a ring in LDS; the strip below runs AD_LAG sub-phases behind,
// which is what puts a barrier between every write of the ring and its read (and between every read and the write that
// reuses the slot).  Nothing waits on another wave anywhere else.  The choice of every cell (2 bits) goes to the
// caller's workspace, 16 cells a word.  Wave 0 then walks the path back - the lanes hold the trace words of 64 rows at
// the current word column, so a step is one cross-lane read - and the block writes the tables.
#include <math.h>

#include "wsae_codewalk.h"

// every product and sum below is an IEEE operation of its own: the oracle has no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int AC_BLOCK = 256, AC_WAVES = AC_BLOCK / 64;
constexpr int AC_TILE = 64;  // frames a workgroup owns
constexpr int AC_MAX_CL = AC_TILE + WSAE_ALIGN_MAX_WIDTH - 1;

constexpr int AD_BLOCK = WSAE_ALIGN_MAX_TOK;  // a lane per row, a wave per strip of 64 rows
constexpr int AD_WAVES = AD_BLOCK / 64;
constexpr int AD_SUB = 16;    // steps between two barriers
constexpr int AD_LAG = 5;     // sub-phases a strip runs behind the one above: (AD_LAG - 1) * AD_SUB >= 63
constexpr int AD_RING = 128;  // columns of a strip's bottom row kept in LDS
static_assert(AD_SUB == 16, "a fetch is four rows of 16 columns per load: lane >> 4 and lane & 15");
static_assert((AD_LAG - 1) * AD_SUB >= 63, "a strip must be a whole barrier behind the bottom row it reads");
static_assert((AD_RING + 63) / AD_SUB - 1 > AD_LAG && (AD_RING & (AD_RING - 1)) == 0, "the ring is reused too early");

struct CostArgs {
    const void* w;
    int n_heads;
    int64_t ld_t, ld_f;
    const int32_t* n_tok;
    const int32_t* n_frames;
    float* cost;
    int32_t* n_bad;
};

template <int DT>
__device__ __forceinline__ float load_w(const void* p, int64_t i) {
    if (DT == WSAE_DT_BF16) return (float)((const bf16_t*)p)[i];
    if (DT == WSAE_DT_F16) return (float)((const _Float16*)p)[i];
    return ((const float*)p)[i];
}

__device__ __forceinline__ int reflect(int q, int n) { return q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q); }

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }  // (false for NaN)

template <int DT, int W>
__global__ __launch_bounds__(AC_BLOCK) void align_cost_kernel(CostArgs a, int tiles) {
    constexpr int P = W / 2, CL = AC_TILE + 2 * P;  // the columns a tile reads: P, the AC_TILE it owns, P
    extern __shared__ double ac_stats[];            // mean [n_heads][CL], then sd [n_heads][CL]
    __shared__ float s_z[AC_WAVES][AC_MAX_CL + 2];
    const int u = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * AC_TILE;
    const int nt = a.n_tok[u], nf = a.n_frames[u];
    float* cu = a.cost + (int64_t)u * a.ld_t * a.ld_f;
    const bool ok = nt >= 1 && nt <= min64(a.ld_t, WSAE_ALIGN_MAX_TOK) && nf > P && nf <= min64(a.ld_f, WSAE_ALIGN_MAX_FRAMES);
    // what phase 2 does not compute: rows from nt on, frames from nf on, every cell of an utterance of invalid sizes
    for (int64_t e = threadIdx.x; e < a.ld_t * AC_TILE; e += AC_BLOCK) {
        const int64_t i = e / AC_TILE, j = j0 + e % AC_TILE;
        if (j < a.ld_f && (!ok || i >= nt || j >= nf)) cu[i * a.ld_f + j] = WSAE_ALIGN_FILL;
    }
    if (!ok) {
        if (j0 == 0 && threadIdx.x == 0) a.n_bad[u] = -1;  // (no block of this utterance adds to it)
        return;
    }
    if (j0 >= nf) return;  // (block-uniform, like every condition above)
    const int64_t head_stride = a.ld_t * a.ld_f;
    const int64_t wu = (int64_t)u * a.n_heads * head_stride;  // (in elements)
    double* s_mean = ac_stats;
    double* s_sd = ac_stats + a.n_heads * CL;
    const double inv_n = (double)nt;
    // phase 1: column c of the tile is frame j0 - P + c, reflected; frames beyond nf - 1 + P serve no output
    for (int item = threadIdx.x; item < a.n_heads * CL; item += AC_BLOCK) {
        const int h = item / CL, c = item % CL, q = j0 - P + c;
        double mean = 0.0, sd = 0.0;
        if (q <= nf - 1 + P) {
            const int64_t base = wu + h * head_stride + reflect(q, nf);
            double s = 0.0;
            for (int i = 0; i < nt; ++i) s = __dadd_rn(s, (double)load_w<DT>(a.w, base + i * a.ld_f));
            mean = __ddiv_rn(s, inv_n);
            double v = 0.0;
            for (int i = 0; i < nt; ++i) {
                const double d = __dsub_rn((double)load_w<DT>(a.w, base + i * a.ld_f), mean);
                v = __dadd_rn(v, __dmul_rn(d, d));
            }
            sd = __dsqrt_rn(__ddiv_rn(v, inv_n));
        }
        s_mean[item] = mean;
        s_sd[item] = sd;
    }
    __syncthreads();
    // phase 2: a token row per wave, heads innermost
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* zb = s_z[wave];
    int bad = 0;
    for (int i0 = 0; i0 < nt; i0 += AC_WAVES) {  // (block-uniform trip counts: the barrier below is reached by all)
        const int i = i0 + wave;
        const bool row_on = i < nt;
        double S = 0.0;
        for (int h = 0; h < a.n_heads; ++h) {
            if (row_on) {
#pragma unroll
                for (int part = 0; part < 2; ++part) {  // columns lane and, on the first 2 P lanes, AC_TILE + lane
                    const int c = lane + AC_TILE * part;
                    if (part == 1 && lane >= 2 * P) break;
                    const int q = j0 - P + c;
                    float z = 0.f;
                    if (q <= nf - 1 + P) {
                        const float x = load_w<DT>(a.w, wu + h * head_stride + i * a.ld_f + reflect(q, nf));
                        if (c >= P && c < P + AC_TILE && q < nf && !finite_f(x)) ++bad;  // (an owned column: counted once)
                        const double sd = s_sd[h * CL + c];
                        if (sd != 0.0) z = (float)__ddiv_rn(__dsub_rn((double)x, s_mean[h * CL + c]), sd) + 0.0f;
                    }
                    zb[c] = z;
                }
            }
            __syncthreads();  // (the row of LDS is the wave's own: the barrier orders its lanes' writes and reads)
            if (row_on) {
                float v[W];
#pragma unroll
                for (int k = 0; k < W; ++k) v[k] = zb[lane + k];  // frames j - P .. j + P of the frame j = j0 + lane
#pragma unroll
                for (int pass = 0; pass < W; ++pass) {
#pragma unroll
                    for (int k = pass & 1; k + 1 < W; k += 2) {
                        const float lo = fminf(v[k], v[k + 1]), hi = fmaxf(v[k], v[k + 1]);
                        v[k] = lo;
                        v[k + 1] = hi;
                    }
                }
                S = __dadd_rn(S, (double)v[P]);
            }
            __syncthreads();  // (the reads are done before the next head overwrites the row)
        }
        if (row_on && j0 + lane < nf) cu[i * a.ld_f + j0 + lane] = (float)__dsub_rn(0.0, __ddiv_rn(S, (double)a.n_heads));
    }
    bad = wave_sum_i(bad);
    if (lane == 0 && bad) atomicAdd(a.n_bad + u, bad);
}

// An utterance with a non-finite value: its cost becomes the fill.  status += {invalid utterances, non-finite values}.
__global__ __launch_bounds__(AC_BLOCK) void align_cost_finish_kernel(CostArgs a, int tiles, unsigned long long* status) {
    const int u = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * AC_TILE;
    const int nb = a.n_bad[u];
    if (nb == 0) return;
    if (nb > 0) {
        float* cu = a.cost + (int64_t)u * a.ld_t * a.ld_f;
        for (int64_t e = threadIdx.x; e < a.ld_t * AC_TILE; e += AC_BLOCK) {
            const int64_t i = e / AC_TILE, j = j0 + e % AC_TILE;
            if (j < a.ld_f) cu[i * a.ld_f + j] = WSAE_ALIGN_FILL;
        }
    }
    if (j0 == 0 && threadIdx.x == 0) {
        atomicAdd(status, 1ull);
        if (nb > 0) atomicAdd(status + 1, (unsigned long long)nb);
    }
}

// ---- wsae_align_dtw -----------------------------------------------------------------------------------------------------------
struct DtwArgs {
    const float* cost;
    int64_t ld_t, ld_f;
    const int32_t* row_first;
    const int32_t* row_count;
    const int32_t* n_frames;
    const int32_t* n_bad;
    int32_t* frame_pos;
    int32_t* tok_start;
    int32_t* tok_end;
    float* path_cost;
    int32_t* path_len;
    unsigned long long* status;
    uint32_t* trace;
};

// the outputs of an invalid utterance; called by the whole block
__device__ __forceinline__ void dtw_invalid(const DtwArgs& a, int u, int n_bad_costs) {
    for (int64_t j = threadIdx.x; j < a.ld_f; j += AD_BLOCK) a.frame_pos[u * a.ld_f + j] = -1;
    for (int64_t r = threadIdx.x; r < a.ld_t; r += AD_BLOCK) {
        a.tok_start[u * a.ld_t + r] = -1;
        a.tok_end[u * a.ld_t + r] = -1;
    }
    if (threadIdx.x == 0) {
        a.path_cost[u] = WSAE_ALIGN_FILL;
        a.path_len[u] = 0;
        atomicAdd(a.status, 1ull);
        if (n_bad_costs) atomicAdd(a.status + 1, (unsigned long long)n_bad_costs);
    }
}

// The value of lane l - 1 (lane 0 keeps its own) by the DPP wave shift: a VALU move, where __shfl_up is a round trip
// through the LDS crossbar on the chain from step to step.  Called with all lanes active.
__device__ __forceinline__ float lane_above(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x138, 0xF, 0xF, false));  // wave_shr:1
}

__global__ __launch_bounds__(AD_BLOCK) void align_dtw_kernel(DtwArgs a) {
    __shared__ float s_tile[AD_WAVES][64][AD_SUB + 1];  // [row of the strip][step of the sub-phase]
    __shared__ float s_ring[AD_WAVES][AD_RING];         // the bottom row of every strip, by column & (AD_RING - 1)
    __shared__ int s_start[WSAE_ALIGN_MAX_TOK];
    __shared__ int s_fpos[WSAE_ALIGN_MAX_FRAMES];
    __shared__ int s_bad, s_len;
    __shared__ float s_final;
    const int64_t u = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int first = a.row_first[u], n = a.row_count[u], k = a.n_frames[u];
    const bool ok = (a.n_bad == nullptr || a.n_bad[u] == 0) && first >= 0 && n >= 1 && n <= WSAE_ALIGN_MAX_TOK &&
                    (int64_t)first + n <= a.ld_t && k >= 1 && k <= min64(a.ld_f, WSAE_ALIGN_MAX_FRAMES);
    if (!ok) {  // (block-uniform)
        dtw_invalid(a, u, 0);
        return;
    }
    if (threadIdx.x == 0) s_bad = 0;  // (the first barrier of the sweep orders this before the adds)
    const float* cu = a.cost + u * a.ld_t * a.ld_f + (int64_t)first * a.ld_f;
    const int64_t wpr = (a.ld_f + 15) >> 4;  // trace words per row
    uint32_t* tr = a.trace + u * a.ld_t * wpr;
    const int nstrips = (n + 63) >> 6;
    const int i = wave * 64 + lane;  // the lane's row
    const bool row_ok = i < n;
    float left = INFINITY;                 // D[i][j-1]
    float diag = i == 0 ? 0.f : INFINITY;  // D[i-1][j-1]
    uint32_t tword = 0;
    int bad = 0;
    const int n_sub = (k + 63 + AD_SUB - 1) / AD_SUB + AD_LAG * (nstrips - 1);
    // the costs of a sub-phase: four rows of AD_SUB consecutive columns per load, fetched one sub-phase ahead so that the
    // steps hide the memory latency, and kept in registers meanwhile (the wave has read its tile before it issues them)
    float pre[16];
    auto fetch = [&](int g) {
        const int t0 = (g - AD_LAG * wave) * AD_SUB;
        const bool on = wave < nstrips && t0 + AD_SUB > 0 && t0 < k + 63;
#pragma unroll
        for (int rr = 0; rr < 64; rr += 4) {
            const int r = rr + (lane >> 4), col = t0 + (lane & 15) - r;
            pre[rr >> 2] = on && wave * 64 + r < n && col >= 0 && col < k ? cu[(int64_t)(wave * 64 + r) * a.ld_f + col] : 0.f;
        }
    };
    fetch(0);
    for (int g = 0; g < n_sub; ++g) {
        const int t0 = (g - AD_LAG * wave) * AD_SUB;  // the wave's first local step of this sub-phase
        const bool wave_on = wave < nstrips && t0 + AD_SUB > 0 && t0 < k + 63;  // (wave-uniform)
        if (wave_on) {
#pragma unroll
            for (int rr = 0; rr < 64; rr += 4) s_tile[wave][rr + (lane >> 4)][lane & 15] = pre[rr >> 2];
        }
        __syncthreads();
        // everything the steps read from LDS, up front: only the lane shift stays on the chain from step to step
        float cs[AD_SUB];
        float above = INFINITY;
        if (wave_on) {
#pragma unroll
            for (int s = 0; s < AD_SUB; ++s) cs[s] = s_tile[wave][lane][s];
            // lane s: column t0 + s of the bottom row of the strip above, which lane 0 meets at step s
            if (wave > 0) above = s_ring[wave - 1][(t0 + (lane & (AD_SUB - 1))) & (AD_RING - 1)];
        }
        fetch(g + 1);  // (a wave that starts in the next sub-phase fetches too; off for every wave once g + 1 == n_sub)
        if (wave_on) {
#pragma unroll
            for (int s = 0; s < AD_SUB; ++s) {
                const int j = t0 + s - lane;
                float up = lane_above(left);  // D[i-1][j]: what the lane above computed one step ago
                const float up0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(above), s));
                if (lane == 0) up = up0;
                if (row_ok && j >= 0 && j < k) {
                    const float c = cs[s];
                    if (!finite_f(c)) ++bad;
                    float from;
                    uint32_t t;
                    if (diag < up && diag < left) {
                        from = diag;
                        t = 0u;
                    } else if (up < diag && up < left) {
                        from = up;
                        t = 1u;
                    } else {
                        from = left;
                        t = 2u;
                    }
                    const float d = c + from;
                    tword |= t << (2 * (j & 15));
                    if ((j & 15) == 15 || j == k - 1) {
                        tr[i * wpr + (j >> 4)] = tword;
                        tword = 0;
                    }
                    diag = up;
                    left = d;
                    if (lane == 63) s_ring[wave][j & (AD_RING - 1)] = d;
                }
            }
        }
    }
    if (bad) atomicAdd(&s_bad, bad);
    if (i == n - 1) s_final = left;
    __syncthreads();
    const int n_bad_costs = s_bad;
    if (n_bad_costs) {  // (block-uniform)
        dtw_invalid(a, u, n_bad_costs);
        return;
    }
    // the walk back: wave 0, every lane with the same (ci, cj); lane l holds the trace word of row top - l at word column wc
    if (wave == 0) {
        int ci = n - 1, cj = k - 1, len = 0, top = -1, wc = -1;
        uint32_t word = 0;
        bool new_col = true;
        for (int step = 0; step < n + k && ci >= 0 && cj >= 0; ++step) {
            if ((cj >> 4) != wc || ci < top - 63) {
                top = ci;
                wc = cj >> 4;
                word = top - lane >= 0 ? tr[(top - lane) * wpr + wc] : 0u;
            }
            // (ci, cj, top and wc are wave-uniform: a scalar lane select, no trip through LDS)
            const int from_lane = __builtin_amdgcn_readfirstlane(top - ci);
            int t = (int)((uint32_t)__builtin_amdgcn_readlane((int)word, from_lane) >> (2 * (cj & 15))) & 3;
            if (ci == 0) t = cj == 0 ? 0 : 2;  // row 0 goes left,
            else if (cj == 0) t = 1;           // column 0 goes up
            if (lane == 0) {
                if (new_col) s_fpos[cj] = first + ci;  // the walk reaches a frame at its largest row
                if (t != 2) s_start[ci] = cj;          // and leaves a row at its first frame
            }
            ++len;
            new_col = t != 1;
            if (t != 2) --ci;
            if (t != 1) --cj;
        }
        if (lane == 0) s_len = len;
    }
    __syncthreads();
    for (int64_t j = threadIdx.x; j < a.ld_f; j += AD_BLOCK) a.frame_pos[u * a.ld_f + j] = j < k ? s_fpos[j] : -1;
    for (int64_t r = threadIdx.x; r < a.ld_t; r += AD_BLOCK) {
        const int64_t li = r - first;
        const bool in = li >= 0 && li < n;
        a.tok_start[u * a.ld_t + r] = in ? s_start[li] : -1;
        a.tok_end[u * a.ld_t + r] = in ? (li == n - 1 ? k : s_start[li + 1]) : -1;
    }
    if (threadIdx.x == 0) {
        a.path_cost[u] = s_final;
        a.path_len[u] = s_len;
    }
}

constexpr int64_t AL_MAX_LD = 1 << 16;   // ld_t, ld_f
constexpr int AL_MAX_UTT = 1 << 16;

inline bool ld_ok(int64_t ld) { return ld >= 1 && ld <= AL_MAX_LD; }

template <int DT>
void launch_cost(int width, int grid, size_t lds, hipStream_t st, const CostArgs& a, int tiles) {
    switch (width) {
        case 1: align_cost_kernel<DT, 1><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 3: align_cost_kernel<DT, 3><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 5: align_cost_kernel<DT, 5><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 7: align_cost_kernel<DT, 7><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 9: align_cost_kernel<DT, 9><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 11: align_cost_kernel<DT, 11><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        case 13: align_cost_kernel<DT, 13><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
        default: align_cost_kernel<DT, 15><<<grid, AC_BLOCK, lds, st>>>(a, tiles); break;
    }
}

}  // namespace

extern "C" int wsae_align_cost(const void* w, int32_t w_dtype, int32_t n_utt, int32_t n_heads, int64_t ld_t, int64_t ld_f,
                               const int32_t* n_tok, const int32_t* n_frames, int32_t width, float* cost, int32_t* n_bad,
                               int64_t* status, void* stream) {
    WSAE_REQUIRE(w && n_tok && n_frames && cost && n_bad && status, "wsae_align_cost: null pointer");
    WSAE_REQUIRE(w_dtype == WSAE_DT_F32 || w_dtype == WSAE_DT_BF16 || w_dtype == WSAE_DT_F16,
                 "wsae_align_cost: unknown w_dtype %d", w_dtype);
    WSAE_REQUIRE(n_utt >= 0 && n_utt <= AL_MAX_UTT, "wsae_align_cost: need 0 <= n_utt <= %d (got %d)", AL_MAX_UTT, n_utt);
    WSAE_REQUIRE(n_heads >= 1 && n_heads <= WSAE_ALIGN_MAX_HEADS, "wsae_align_cost: need 1 <= n_heads <= %d (got %d)",
                 WSAE_ALIGN_MAX_HEADS, n_heads);
    WSAE_REQUIRE(ld_ok(ld_t) && ld_ok(ld_f), "wsae_align_cost: need 1 <= ld_t, ld_f <= %lld (got %lld, %lld)",
                 (long long)AL_MAX_LD, (long long)ld_t, (long long)ld_f);
    WSAE_REQUIRE(width >= 1 && width <= WSAE_ALIGN_MAX_WIDTH && (width & 1), "wsae_align_cost: width must be odd in 1 .. %d (got %d)",
                 WSAE_ALIGN_MAX_WIDTH, width);
    if (n_utt == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (int)ceil_div64(ld_f, AC_TILE);
    const int64_t blocks = (int64_t)n_utt * tiles;
    WSAE_REQUIRE(blocks <= 0x7fffffffll, "wsae_align_cost: n_utt * ld_f is too large for one launch");
    CostArgs a = {w, n_heads, ld_t, ld_f, n_tok, n_frames, cost, n_bad};
    WSAE_HIP_CHECK(hipMemsetAsync(n_bad, 0, sizeof(int32_t) * (size_t)n_utt, st));
    const size_t lds = sizeof(double) * 2 * (size_t)n_heads * (AC_TILE + width - 1);
    if (w_dtype == WSAE_DT_F32) launch_cost<WSAE_DT_F32>(width, (int)blocks, lds, st, a, tiles);
    else if (w_dtype == WSAE_DT_BF16) launch_cost<WSAE_DT_BF16>(width, (int)blocks, lds, st, a, tiles);
    else launch_cost<WSAE_DT_F16>(width, (int)blocks, lds, st, a, tiles);
    align_cost_finish_kernel<<<(int)blocks, AC_BLOCK, 0, st>>>(a, tiles, (unsigned long long*)status);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

extern "C" int64_t wsae_align_workspace_bytes(int32_t n_utt, int64_t max_tok, int64_t max_frames) {
    if (n_utt < 0 || n_utt > AL_MAX_UTT || !ld_ok(max_tok) || !ld_ok(max_frames)) return -1;
    return align256((int64_t)sizeof(uint32_t) * n_utt * max_tok * ((max_frames + 15) >> 4));
}

extern "C" int wsae_align_dtw(const float* cost, int32_t n_utt, int64_t ld_t, int64_t ld_f, const int32_t* row_first,
                              const int32_t* row_count, const int32_t* n_frames, const int32_t* n_bad, int32_t* frame_pos,
                              int32_t* tok_start, int32_t* tok_end, float* path_cost, int32_t* path_len, int64_t* status,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(cost && row_first && row_count && n_frames && frame_pos && tok_start && tok_end && path_cost && path_len && status,
                 "wsae_align_dtw: null pointer");
    WSAE_REQUIRE(n_utt >= 0 && n_utt <= AL_MAX_UTT, "wsae_align_dtw: need 0 <= n_utt <= %d (got %d)", AL_MAX_UTT, n_utt);
    WSAE_REQUIRE(ld_ok(ld_t) && ld_ok(ld_f), "wsae_align_dtw: need 1 <= ld_t, ld_f <= %lld (got %lld, %lld)", (long long)AL_MAX_LD,
                 (long long)ld_t, (long long)ld_f);
    const int64_t need = wsae_align_workspace_bytes(n_utt, ld_t, ld_f);
    WSAE_REQUIRE_WORKSPACE("wsae_align_dtw", workspace, workspace_bytes, need, n_utt);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_align_dtw", workspace, 8);
    if (n_utt == 0) return WSAE_OK;
    DtwArgs a = {cost,      ld_t,    ld_f,      row_first, row_count, n_frames, n_bad, frame_pos, tok_start,
                 tok_end,   path_cost, path_len, (unsigned long long*)status, (uint32_t*)workspace};
    align_dtw_kernel<<<n_utt, AD_BLOCK, 0, (hipStream_t)stream>>>(a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
