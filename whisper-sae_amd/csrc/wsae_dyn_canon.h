// The canonical pass of the analyses that compare whole frames of a compact code (DESIGN.md sections 23 and 26):
// dyn_canon_kernel, one wave per row on the front end of wsae_codewalk.h, writes per entry u = v weight[f] and f (or -1
// where the entry is not active) and per row the norm n_r and the number of active features a_r into the workspace
// sections of dyn_layout; dyn_load_canon reads them back a lane per entry.  Included by wsae_dynamics.hip (frame against
// frame at a lag) and wsae_abx.hip (segment against segment).
#pragma once
#include "wsae_codewalk.h"

namespace {

constexpr int DY_BLOCK = 256;        // four waves, one row each per pass
constexpr int DY_MAX_BLOCKS = 4096;  // more rows than DY_MAX_BLOCKS * 4: the grid-stride loop

struct DynArgs {
    const float* vals;
    const int32_t* idx;
    const int32_t* seg;     // nullable
    const float* weight;    // nullable
    const int32_t* label;   // nullable
    int64_t n_rows;
    int k, hidden, L, metric;
    int lag[WSAE_DYN_MAX_LAGS];
    float* cu;      // [n_rows, k] canonical values (0 where inactive)
    int32_t* cf;    // [n_rows, k] canonical features (-1 where inactive)
    double* nrm;    // [n_rows]
    int32_t* act;   // [n_rows]
    float* sim;     // [n_rows, L], nullable
    unsigned long long* pairs;  // the state, nullable as a whole
    unsigned long long* sim_q;
    unsigned long long* sq_q;
    unsigned long long* hist;
    unsigned long long* total_rows;
};

__global__ __launch_bounds__(DY_BLOCK) void dyn_canon_kernel(DynArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (DY_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (DY_BLOCK / 64);
    const int k = a.k, k0 = k < 64 ? k : 64;
    for (int64_t r = wave; r < a.n_rows; r += n_waves) {
        float v0, v1;
        int f0, f1, c0, c1;
        probe_load_row(a.vals, a.idx, k, r, lane, v0, f0, v1, f1);
        probe_row_columns(v0, f0, v1, f1, k, a.hidden, nullptr, lane, c0, c1);
        if (a.seg != nullptr && a.seg[r] < 0) c0 = -1, c1 = -1;  // (padding: nothing is active)
        float u0 = 0.f, u1 = 0.f;
        if (c0 >= 0) {
            u0 = v0;
            if (a.weight != nullptr) {
                const float w = a.weight[c0];
                u0 = v0 * w;
                if (!(w > 0.f)) c0 = -1, u0 = 0.f;
            }
        }
        if (c1 >= 0) {
            u1 = v1;
            if (a.weight != nullptr) {
                const float w = a.weight[c1];
                u1 = v1 * w;
                if (!(w > 0.f)) c1 = -1, u1 = 0.f;
            }
        }
        double n = 0.0;  // one chain in ascending entry position, the same in every lane
        for (int d = 0; d < k0; ++d) {
            const double x = (double)lane_f32(u0, d);
            if (__builtin_amdgcn_readlane(c0, d) >= 0) n += x * x;
        }
        for (int d = 64; d < k; ++d) {
            const double x = (double)lane_f32(u1, d - 64);
            if (__builtin_amdgcn_readlane(c1, d - 64) >= 0) n += x * x;
        }
        const int active = __popcll(__ballot(c0 >= 0)) + __popcll(__ballot(c1 >= 0));
        if (lane < k) {
            a.cu[r * k + lane] = u0;
            a.cf[r * k + lane] = c0;
        }
        if (lane + 64 < k) {
            a.cu[r * k + lane + 64] = u1;
            a.cf[r * k + lane + 64] = c1;
        }
        if (lane == 0) {
            a.nrm[r] = n;
            a.act[r] = active;
        }
    }
}

// the canonical entries lane and lane + 64 of row r (f = -1 beyond k)
__device__ __forceinline__ void dyn_load_canon(const DynArgs& a, int64_t r, int lane, float& u0, int& f0, float& u1, int& f1) {
    u0 = 0.f, u1 = 0.f, f0 = -1, f1 = -1;
    if (lane < a.k) {
        u0 = a.cu[r * a.k + lane];
        f0 = a.cf[r * a.k + lane];
    }
    if (lane + 64 < a.k) {
        u1 = a.cu[r * a.k + lane + 64];
        f1 = a.cf[r * a.k + lane + 64];
    }
}

// the sections of the workspace the canonical pass fills: cu, cf, nrm, act
struct DynLayout {
    int64_t cu, cf, nrm, act, total;
};
inline DynLayout dyn_layout(int64_t n_rows, int k) {
    DynLayout w;
    w.cu = 0;
    w.cf = w.cu + align256(4 * n_rows * k);
    w.nrm = w.cf + align256(4 * n_rows * k);
    w.act = w.nrm + align256(8 * n_rows);
    w.total = w.act + align256(4 * n_rows);
    return w;
}

// the launch of the canonical pass over the n_rows of a (cu, cf, nrm, act set)
inline int dyn_canon_grid(int64_t n_rows) {
    const int64_t blocks = ceil_div64(n_rows, DY_BLOCK / 64);
    return (int)(blocks < DY_MAX_BLOCKS ? blocks : DY_MAX_BLOCKS);
}

}  // namespace
