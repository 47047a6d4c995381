// BatchTopK selection (Bussmann, Leask & Nanda 2024) over the compact code of the per-row TopK: keep the B * k_batch
// largest POSITIVE candidates of the whole batch (at most k_max = ctx->K per row, the width of the code), zero the rest.
// An exact k-th-largest selection on the device, with no host sync:
//
//   positive floats order like their bit patterns, so the 31 significant bits are split 11 / 10 / 10 and each level is
//   one histogram launch over vals [B][K] (LDS histogram per block, then integer agent-scope atomics into a global
//   histogram: deterministic).  The LAST-ARRIVING block of a launch (agent-scope release fence + arrival ticket in
//   every block, agent-scope acquire fence in the last one) resolves the bin that
//   holds the target rank and leaves the key prefix and the rank left inside that bin for the next launch.  A final
//   launch zeroes the dropped candidates, counts the kept and saturated entries, and its last block writes t and updates
//   the threshold EMA.  No block ever waits on another: the levels hand over through launch boundaries.
//
// Counters and histograms live in ctx->btk_ws and are zeroed by one hipMemsetAsync ahead of the first launch.
#include "wsae_common.h"

namespace {

constexpr int BTK_THREADS = 256;
constexpr int BTK_MAX_BLOCKS = 128;     // arrivals per ticket / per hot histogram bin (fan-in cost grows with it)
constexpr int BTK_MIN_PER_BLOCK = 8192;  // entries below which one more block is not worth its arrival
constexpr int BTK_UNROLL = 8;            // float4 loads in flight per thread: a block's whole share in one or two round trips

// word layout of ctx->btk_ws (int32 words)
constexpr int W_H1 = 0;            // 2048 bins: key bits 30..20
constexpr int W_H2 = 2048;         // 1024 bins: key bits 19..10 (inside the level-1 bin)
constexpr int W_H3 = 3072;         // 1024 bins: key bits 9..0  (inside the level-2 prefix)
constexpr int W_CTL = 4096;
constexpr int C_PREFIX = 0;        // key prefix resolved so far (level 1: 11 bits, level 2: 21 bits, level 3: the whole key)
constexpr int C_NEED = 1;          // rank (1-based, from the top) still to find inside that prefix
constexpr int C_STATE = 2;         // 0: selecting; 1: threshold mode (eval with theta >= 0); 2: no positive candidate
constexpr int C_KEPT = 3;
constexpr int C_SAT = 4;
constexpr int C_TICKET = 8;        // one arrival counter per launch (4 launches)
constexpr int BTK_WS_WORDS = W_CTL + 16;

__device__ __forceinline__ int* ctl(int* ws) { return ws + W_CTL; }

// Arrival of one block (call with every thread): the block's global atomics are complete and released, then lane 0
// draws a ticket.  Returns true in every thread of the last-arriving block, after its acquire.
__device__ __forceinline__ bool btk_arrive(int* ticket, int* flag_lds) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int prev = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == (int)gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag_lds = last;
    }
    __syncthreads();
    return *flag_lds != 0;
}

// f(e, v) for the entries [lo, hi) of this block's share of vals[0, n): 16-byte loads, BTK_UNROLL of them issued before
// any is used (the share is a multiple of 4 entries; block 0 also takes the n % 4 tail)
template <typename F>
__device__ __forceinline__ void btk_for_each(const float* vals, int64_t n, F&& f) {
    const int64_t n4 = n >> 2;
    const int64_t per = (n4 + gridDim.x - 1) / gridDim.x;
    const int64_t lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
    const float4* v4 = (const float4*)vals;
    for (int64_t base = lo + threadIdx.x; base < hi; base += (int64_t)BTK_THREADS * BTK_UNROLL) {
        float4 r[BTK_UNROLL];
#pragma unroll
        for (int u = 0; u < BTK_UNROLL; ++u) {
            const int64_t i = base + (int64_t)u * BTK_THREADS;
            r[u] = i < hi ? v4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < BTK_UNROLL; ++u) {
            const int64_t i = base + (int64_t)u * BTK_THREADS;
            if (i < hi) {
                f(4 * i, r[u].x);
                f(4 * i + 1, r[u].y);
                f(4 * i + 2, r[u].z);
                f(4 * i + 3, r[u].w);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t e = 4 * n4 + threadIdx.x;
        f(e, vals[e]);
    }
}

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Last block of a histogram launch: find the bin b (counted from the top) where the running count reaches
// min(need, total of the histogram).  Writes *bin_out = b and *rest_out = that rank - (count of the bins above b), or
// *bin_out = -1 when the histogram is empty.  `need` >= 1.
template <int NB>
__device__ void btk_find(const int* hist, int64_t need64, int* lds, int* bin_out, int* rest_out) {
    constexpr int PER = NB / BTK_THREADS;
    const int t = threadIdx.x;
    int c[PER];
    int s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {  // thread t holds bins NB-1-(t*PER+i): thread 0 the top ones
        c[i] = ld_agent(hist + (NB - 1 - (t * PER + i)));
        s += c[i];
    }
    lds[t] = s;
    __syncthreads();
    // inclusive scan over the 256 thread sums (Hillis-Steele in LDS: this runs in one block of the grid)
    for (int off = 1; off < BTK_THREADS; off <<= 1) {
        const int v = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += v;
        __syncthreads();
    }
    const int total = lds[BTK_THREADS - 1];
    const int need = (int)(need64 < total ? need64 : total);  // fewer positives than B k: keep them all
    if (total == 0 && t == 0) *bin_out = -1;
    const int incl = lds[t], excl = incl - s;
    if (need > 0 && excl < need && need <= incl) {
        int run = excl;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (run < need && need <= run + c[i]) {
                *bin_out = NB - 1 - (t * PER + i);
                *rest_out = need - run;
            }
            run += c[i];
        }
    }
}

// One level of the radix select.  LEVEL 1: every positive entry, bin = key >> 20.  LEVEL 2: entries with key >> 20 ==
// prefix, bin = (key >> 10) & 1023.  LEVEL 3: entries with key >> 10 == prefix, bin = key & 1023.
template <int LEVEL>
__global__ void __launch_bounds__(BTK_THREADS) btk_hist_kernel(const float* __restrict__ vals, int64_t n, int64_t target,
                                                              int mode, const wsae_batch_topk_state* __restrict__ state,
                                                              int* __restrict__ ws) {
    constexpr int NB = LEVEL == 1 ? 2048 : 1024;
    constexpr int SHIFT = LEVEL == 1 ? 20 : (LEVEL == 2 ? 10 : 0);
    __shared__ int lds[NB + 2];
    int* c = ctl(ws);
    // whole-launch early outs (uniform): eval mode with a trained threshold needs no selection; no positive candidate
    if (LEVEL == 1) {
        if (mode == WSAE_BTK_EVAL && state->threshold >= 0.f) {
            if (blockIdx.x == 0 && threadIdx.x == 0) c[C_STATE] = 1;
            return;
        }
    } else if (c[C_STATE] != 0) {
        return;
    }
    const uint32_t prefix = LEVEL == 1 ? 0u : (uint32_t)c[C_PREFIX];
    for (int i = threadIdx.x; i < NB; i += BTK_THREADS) lds[i] = 0;
    __syncthreads();
    btk_for_each(vals, n, [&](int64_t, float v) {
        if (!(v > 0.f)) return;
        const uint32_t u = __float_as_uint(v);
        if (LEVEL == 2 && (u >> 20) != prefix) return;
        if (LEVEL == 3 && (u >> 10) != prefix) return;
        atomicAdd(&lds[(u >> SHIFT) & (NB - 1)], 1);
    });
    __syncthreads();
    int* hist = ws + (LEVEL == 1 ? W_H1 : (LEVEL == 2 ? W_H2 : W_H3));
    for (int i = threadIdx.x; i < NB; i += BTK_THREADS) {
        const int v = lds[i];
        if (v) __hip_atomic_fetch_add(hist + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!btk_arrive(c + C_TICKET + LEVEL - 1, &lds[NB])) return;
    // ---- last block: resolve this level's bin ----
    btk_find<NB>(hist, LEVEL == 1 ? target : (int64_t)c[C_NEED], lds, &lds[NB], &lds[NB + 1]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int bin = lds[NB];
        if (bin < 0) {  // (level 1 only: no positive candidate in the batch)
            c[C_STATE] = 2;
        } else {
            c[C_PREFIX] = (int)(LEVEL == 1 ? (uint32_t)bin : (prefix << 10) | (uint32_t)bin);
            c[C_NEED] = lds[NB + 1];
        }
    }
}

// Zero the dropped candidates; count kept entries and saturated rows; the last block writes the record and the EMA.
__global__ void __launch_bounds__(BTK_THREADS) btk_mask_kernel(float* __restrict__ vals, int64_t n, int K, int H, int mode,
                                                              wsae_batch_topk_state* __restrict__ state, int* __restrict__ ws) {
    __shared__ int lds[2 * (BTK_THREADS / 64) + 1];
    int* c = ctl(ws);
    const int how = c[C_STATE];  // 0: v >= t, 1: v > theta, 2: nothing positive
    const float theta = state->threshold;
    const float t = how == 0 ? __uint_as_float((uint32_t)c[C_PREFIX]) : theta;
    auto keep = [&](float v) { return v > 0.f && (how == 0 ? v >= t : (how == 1 && v > t)); };
    int kept = 0, sat = 0;
    btk_for_each(vals, n, [&](int64_t e, float v) {
        if (keep(v)) ++kept;
        else if (v != 0.f) vals[e] = 0.f;
    });
    // saturated rows: the last candidate kept.  Kept entries are never written and a dropped one reads as dropped
    // before or after another block zeroes it, so this needs no ordering against the pass above.
    if (K < H) {
        const int64_t B = n / K;
        for (int64_t r = (int64_t)blockIdx.x * BTK_THREADS + threadIdx.x; r < B; r += (int64_t)gridDim.x * BTK_THREADS)
            sat += keep(vals[r * K + K - 1]) ? 1 : 0;
    }
    kept = wave_sum_i(kept);
    sat = wave_sum_i(sat);
    if ((threadIdx.x & 63) == 0) {
        lds[threadIdx.x >> 6] = kept;
        lds[BTK_THREADS / 64 + (threadIdx.x >> 6)] = sat;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int bk = 0, bs = 0;
        for (int w = 0; w < BTK_THREADS / 64; ++w) {
            bk += lds[w];
            bs += lds[BTK_THREADS / 64 + w];
        }
        if (bk) __hip_atomic_fetch_add(c + C_KEPT, bk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bs) __hip_atomic_fetch_add(c + C_SAT, bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!btk_arrive(c + C_TICKET + 3, &lds[2 * (BTK_THREADS / 64)])) return;
    if (threadIdx.x != 0) return;
    const int tk = ld_agent(c + C_KEPT), ts = ld_agent(c + C_SAT);
    state->kept = tk;
    state->saturated_rows = ts;
    state->last_t = how == 2 ? -1.f : t;
    if (mode == WSAE_BTK_TRAIN && how == 0 && tk > 0) {
        // theta <- t on the first selection, then beta theta + (1 - beta) t, each operation rounded once (no contraction)
        const float beta = state->beta;
        state->threshold = theta < 0.f ? t : __fadd_rn(__fmul_rn(beta, theta), __fmul_rn(__fsub_rn(1.f, beta), t));
    }
}

}  // namespace

size_t wsae_internal_batch_topk_ws_bytes() { return (size_t)BTK_WS_WORDS * 4; }

int wsae_internal_batch_topk(wsae_ctx* ctx, float* vals, int B, int k_batch, int mode, wsae_batch_topk_state* state,
                             hipStream_t st) {
    WSAE_REQUIRE(((uintptr_t)vals & 15) == 0, "batch_topk: the code values must be 16-byte aligned");
    const int64_t n = (int64_t)B * ctx->K;
    const int64_t target = (int64_t)B * k_batch;
    int nblk = (int)ceil_div64(n, BTK_MIN_PER_BLOCK);
    nblk = nblk < 1 ? 1 : (nblk > BTK_MAX_BLOCKS ? BTK_MAX_BLOCKS : nblk);
    int* ws = ctx->btk_ws;
    WSAE_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)BTK_WS_WORDS * 4, st));
    btk_hist_kernel<1><<<nblk, BTK_THREADS, 0, st>>>(vals, n, target, mode, state, ws);
    btk_hist_kernel<2><<<nblk, BTK_THREADS, 0, st>>>(vals, n, target, mode, state, ws);
    btk_hist_kernel<3><<<nblk, BTK_THREADS, 0, st>>>(vals, n, target, mode, state, ws);
    btk_mask_kernel<<<nblk, BTK_THREADS, 0, st>>>(vals, n, ctx->K, ctx->H, mode, state, ws);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}

static int check_btk(const wsae_ctx* ctx, int k_batch, int mode, const void* state, const char* who) {
    WSAE_REQUIRE(ctx, "%s: null ctx", who);
    WSAE_REQUIRE(k_batch >= 0 && k_batch <= ctx->K, "%s: k_batch %d outside [0, k = %d] (k of the ctx is the per-row cap)",
                 who, k_batch, ctx->K);
    WSAE_REQUIRE(mode == WSAE_BTK_TRAIN || mode == WSAE_BTK_EVAL || mode == WSAE_BTK_SELECT, "%s: unknown mode %d", who, mode);
    WSAE_REQUIRE(k_batch == 0 || state, "%s: null state", who);
    return WSAE_OK;
}

extern "C" int wsae_batch_topk_select(wsae_ctx* ctx, float* vals, int32_t B, int32_t k_batch, int32_t mode,
                                      wsae_batch_topk_state* state, void* stream) {
    int rc = check_btk(ctx, k_batch, mode, state, "wsae_batch_topk_select");
    if (rc) return rc;
    WSAE_REQUIRE(vals && k_batch >= 1, "wsae_batch_topk_select: null vals or k_batch 0");
    WSAE_REQUIRE(B >= 1 && B <= ctx->maxB, "wsae_batch_topk_select: batch %d outside [1, max_batch=%d]", B, ctx->maxB);
    return wsae_internal_batch_topk(ctx, vals, B, k_batch, mode, state, (hipStream_t)stream);
}

extern "C" int wsae_ctx_set_batch_topk(wsae_ctx* ctx, int32_t k_batch, int32_t mode, wsae_batch_topk_state* state) {
    int rc = check_btk(ctx, k_batch, mode, state, "wsae_ctx_set_batch_topk");
    if (rc) return rc;
    ctx->btk_k = k_batch;
    ctx->btk_mode = mode;
    ctx->btk_state = k_batch ? state : nullptr;
    return WSAE_OK;
}
