// Experiment, not part of libwsae_hip.so (profiles/experiments/README.md, "Label association: combining equal cells in
// LDS"): wsae_label_update with the cnt atomics combined per block.  A block walks a CONTIGUOUS stretch of the flat code
// and adds every (feature, lag, class, stratum) cell it meets to an open-addressed LDS table key -> count; the table goes
// to the state - one global atomic per distinct cell - whenever it is half full, and at the block's end.  A cell that
// finds no slot within CB_PROBES probes takes the direct global atomic, so the integers are those of the direct form.
// Built against the library's wsae_codewalk.h (the walk) with an entry point of its own and the signature of
// wsae_label_update; the arguments are taken as already checked (profiles/label_association_timing.py calls the library
// with the same arguments first).
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared -std=c++17 -Iinclude -Iwhisper-sae_amd/csrc \
//         profiles/experiments/wsae_labels_combine.hip -o profiles/tools/build/libwsae_labels_combine.so
#include "wsae_codewalk.h"

namespace {

constexpr int CB_BLOCK = 256;
constexpr int CB_MAX_BLOCKS = 2048;
constexpr int CB_SLOTS = 4096;  // 32 KB of keys and counts
constexpr int CB_PROBES = 8;
constexpr int CB_LDS_CELLS = 4096;
constexpr unsigned int CB_EMPTY = 0xFFFFFFFFu;

struct CombineArgs {
    const int32_t* labels;
    const float* edges;
    int64_t n_rows, per_block;  // per_block: entries per block, a multiple of CB_BLOCK
    int C, S, lag_lo, L;
    int32_t* cnt;
    unsigned long long* pair_rows;
};

__device__ __forceinline__ int cb_pair_class(const CodeArgs& a, const CombineArgs& g, int64_t r, int seg_r, int l) {
    const int64_t q = r + g.lag_lo + l;
    if (q < 0 || q >= g.n_rows) return -1;
    if (a.seg != nullptr && a.seg[q] != seg_r) return -1;
    const int c = g.labels[q];
    return c >= 0 && c < g.C ? c : -1;
}

__global__ __launch_bounds__(CB_BLOCK) void label_combine_kernel(CodeArgs a, CombineArgs g) {
    __shared__ int s_idx[CB_BLOCK];
    __shared__ unsigned int s_key[CB_SLOTS];
    __shared__ unsigned int s_cnt[CB_SLOTS];
    __shared__ int s_used;
    extern __shared__ unsigned int cb_pairs[];  // [L, C]
    const int cells = g.L * g.C;
    for (int i = threadIdx.x; i < cells; i += CB_BLOCK) cb_pairs[i] = 0u;
    for (int i = threadIdx.x; i < CB_SLOTS; i += CB_BLOCK) {
        s_key[i] = CB_EMPTY;
        s_cnt[i] = 0u;
    }
    if (threadIdx.x == 0) s_used = 0;
    const int64_t begin = (int64_t)blockIdx.x * g.per_block;
    const int64_t end = begin + g.per_block < a.n ? begin + g.per_block : a.n;
    for (int64_t base = begin; base < end; base += CB_BLOCK) {
        float v;
        int f;
        int64_t r;
        bool head;
        const bool act = pf_first_active(a, base, s_idx, v, f, r, head);
        if (head || act) {
            const int seg_r = a.seg != nullptr ? a.seg[r] : 0;
            int col = 0, stratum = 0;
            if (act) {
                col = f - a.f_lo;
                const float* ed = g.edges + (int64_t)col * (g.S - 1);
                for (int t = 0; t < g.S - 1; ++t) stratum += ed[t] <= v;
            }
            for (int l = 0; l < g.L; ++l) {
                const int c = cb_pair_class(a, g, r, seg_r, l);
                if (c < 0) continue;
                if (head) atomicAdd(cb_pairs + l * g.C + c, 1u);
                if (!act) continue;
                const unsigned int cell = (unsigned int)((((int64_t)col * g.L + l) * g.C + c) * g.S + stratum);
                unsigned int h = (cell * 2654435761u) >> 20;  // 12 bits
                bool done = false;
                for (int p = 0; p < CB_PROBES && !done; ++p) {
                    const unsigned int prev = atomicCAS(s_key + h, CB_EMPTY, cell);
                    if (prev == CB_EMPTY) atomicAdd(&s_used, 1);
                    if (prev == CB_EMPTY || prev == cell) {
                        atomicAdd(s_cnt + h, 1u);
                        done = true;
                    }
                    h = (h + 1) & (CB_SLOTS - 1);
                }
                if (!done) atomicAdd(g.cnt + cell, 1);
            }
        }
        __syncthreads();
        const bool last = base + CB_BLOCK >= end;
        if (s_used > CB_SLOTS / 2 || last) {  // (block-uniform: read behind the barrier)
            for (int i = threadIdx.x; i < CB_SLOTS; i += CB_BLOCK) {
                const unsigned int key = s_key[i];
                if (key != CB_EMPTY) {
                    atomicAdd(g.cnt + key, (int)s_cnt[i]);
                    s_key[i] = CB_EMPTY;
                    s_cnt[i] = 0u;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) s_used = 0;
            // (the first barrier of the next pf_first_active orders this before the next insert)
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += CB_BLOCK) {
        const unsigned int n = cb_pairs[i];
        if (n) atomicAdd(g.pair_rows + i, (unsigned long long)n);
    }
}

}  // namespace

extern "C" int wsae_label_update_combine(const float* vals, const int32_t* idx, int32_t k, int32_t hidden, const int32_t* seg,
                                         const int32_t* labels, int64_t n_rows, int32_t n_classes, int32_t lag_lo,
                                         int32_t lag_hi, int32_t f_lo, int32_t f_cols, const float* edges, int32_t n_strata,
                                         int32_t* cnt, int64_t* pair_rows, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
    (void)hidden;
    (void)workspace;
    (void)workspace_bytes;
    const int L = lag_hi - lag_lo + 1;
    if (n_rows <= 0 || L * n_classes > CB_LDS_CELLS || (int64_t)f_cols * L * n_classes * n_strata >= 0xFFFFFFFFll) return -1;
    CodeArgs a = {vals, idx, seg, n_rows * k, k, f_lo, f_cols};
    const int64_t passes = ceil_div64(a.n, CB_BLOCK);
    const int grid = (int)(passes < CB_MAX_BLOCKS ? passes : CB_MAX_BLOCKS);
    const int64_t per_block = ceil_div64(passes, grid) * CB_BLOCK;
    CombineArgs g = {labels, edges, n_rows, per_block, n_classes, n_strata, lag_lo, L, cnt, (unsigned long long*)pair_rows};
    label_combine_kernel<<<grid, CB_BLOCK, sizeof(unsigned int) * L * n_classes, (hipStream_t)stream>>>(a, g);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
