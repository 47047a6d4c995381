// How much of a short streaming kernel is the write-back of the dirty L2 lines it leaves behind?
// The XCD L2s are write-back: plain and nt stores keep the line dirty until the agent-scope release at the kernel's end,
// write-through stores (aux bit 4 of the buffer store = sc1; 18 = sc1 + nt) send it on at once and drop the line.
// Two patterns, every launch preceded by the 400 MB fill of probe_update_stream.hip:
//   upd   the 71 MB read-modify-write of update_rows (k_once<2> of probe_update_stream.hip): p / m / v stored plain, aux 16 or
//         aux 18; the bf16 copy as 8-byte stores or widened to 16 bytes per lane (a lane takes two adjacent float4);
//   slab  the store side of w2_epilogue: 256 workgroups of 8 waves, 36 float4 stores per wave in 384-byte row pieces of the
//         [row][slot][D] slab (75.5 MB), behind `spin` dependent FMAs per wave - as ONE burst at the end, or spread (spin / 36
//         FMAs in front of each store).
// Each variant is timed with events twice: alone, and followed by a dependent one-block kernel in the same stream.
//   hipcc --offload-arch=gfx950 -O3 -o probe_dirty_tail probe_dirty_tail.hip && ./probe_dirty_tail
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#define AUX_PLAIN 0
#define AUX_NT 2
#define AUX_WT 16     // write-through (sc1)
#define AUX_WT_NT 18  // both

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(void* p, long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)bytes, 0x00020000);
}
template <int AUX>
__device__ __forceinline__ void st16(const __amdgpu_buffer_rsrc_t& r, long byte_off, const float4& a) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, a), r, (int)byte_off, 0, AUX);
}

__device__ __forceinline__ float4 upd(float4 p, float4 g, float4& m, float4& v) {
    m.x += (g.x - m.x) * 0.1f; m.y += (g.y - m.y) * 0.1f; m.z += (g.z - m.z) * 0.1f; m.w += (g.w - m.w) * 0.1f;
    v.x = 0.999f * v.x + 0.001f * g.x * g.x; v.y = 0.999f * v.y + 0.001f * g.y * g.y;
    v.z = 0.999f * v.z + 0.001f * g.z * g.z; v.w = 0.999f * v.w + 0.001f * g.w * g.w;
    p.x -= 1e-4f * m.x * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v.x) + 1e-8f);
    p.y -= 1e-4f * m.y * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v.y) + 1e-8f);
    p.z -= 1e-4f * m.z * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v.z) + 1e-8f);
    p.w -= 1e-4f * m.w * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v.w) + 1e-8f);
    return p;
}

// k_once<2> with buffer stores.  WIDE = 0: float4 i and i + 256 per thread, bf16 copy as two 8-byte stores (aux 0);
// WIDE = 1: float4 2 t and 2 t + 1 per thread, bf16 copy as ONE 16-byte store with policy AUX_S.
template <int AUX, int WIDE, int AUX_S>
__global__ void __launch_bounds__(256) k_upd(float4* P, const float4* G, float4* M, float4* V, __bf16* S, long n4) {
    const __amdgpu_buffer_rsrc_t rp = rsrc_of(P, n4 * 16), rm = rsrc_of(M, n4 * 16), rv = rsrc_of(V, n4 * 16), rs = rsrc_of(S, n4 * 8);
    const long base = (long)blockIdx.x * 512 + (WIDE ? 2 * threadIdx.x : threadIdx.x);
    constexpr int STEP = WIDE ? 1 : 256;
    float4 p[2], g[2], m[2], v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long i = min(base + (long)STEP * u, n4 - 1);
        p[u] = P[i]; g[u] = G[i]; m[u] = M[i]; v[u] = V[i];
    }
    float4 q[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long i = base + (long)STEP * u;
        if (i >= n4) continue;
        q[u] = upd(p[u], g[u], m[u], v[u]);
        st16<AUX>(rp, i * 16, q[u]); st16<AUX>(rm, i * 16, m[u]); st16<AUX>(rv, i * 16, v[u]);
        if (!WIDE) {
            bf16x4 s; s[0] = (__bf16)q[u].x; s[1] = (__bf16)q[u].y; s[2] = (__bf16)q[u].z; s[3] = (__bf16)q[u].w;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(i32x2, s), rs, (int)(i * 8), 0, AUX_PLAIN);
        }
    }
    if (WIDE && base + 1 < n4) {  // (n4 is even: a lane's two float4 are inside together)
        bf16x8 s;
        s[0] = (__bf16)q[0].x; s[1] = (__bf16)q[0].y; s[2] = (__bf16)q[0].z; s[3] = (__bf16)q[0].w;
        s[4] = (__bf16)q[1].x; s[5] = (__bf16)q[1].y; s[6] = (__bf16)q[1].z; s[7] = (__bf16)q[1].w;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, s), rs, (int)(base * 8), 0, AUX_S);
    }
}

// the store side of w2_epilogue: workgroup = tile * 8 + split, tile = (matrix, 192-row feature tile); wave (wm, wn) owns 96 rows
// x 96 columns and stores them as 3 patches of 32 x 96: 12 float4 per lane and patch, a wave instruction = 64 / 24 row pieces
#define SL_H 3072
#define SL_D 384
#define SL_NS 8
template <int AUX, int SPREAD>
__global__ void __launch_bounds__(512) k_slab(float* out, long bytes, int spin, int do_store) {
    const __amdgpu_buffer_rsrc_t ro = rsrc_of(out, bytes);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 2, wn = wave & 3;
    const int split = blockIdx.x % SL_NS, tile = blockIdx.x / SL_NS;  // tiles: 2 matrices x 16 feature tiles
    const long rstr = (long)SL_NS * SL_D;
    const long row0 = (long)tile * 192 + wm * 96;
    float a = (float)lane * 1e-3f + 1.f;
    const int per = SPREAD ? spin / 36 : spin;
    if (!SPREAD)
        for (int s = 0; s < per; ++s) a = fmaf(a, 0.999999f, 1e-7f);
#pragma unroll 1
    for (int mi = 0; mi < 3; ++mi) {
#pragma unroll 1
        for (int i = 0; i < 12; ++i) {
            if (SPREAD)
                for (int s = 0; s < per; ++s) a = fmaf(a, 0.999999f, 1e-7f);
            const int idx = lane + 64 * i;
            const int row = idx / 24, c4 = idx - row * 24;
            const long o = ((row0 + mi * 32 + row) * rstr + (long)split * SL_D + wn * 96 + c4 * 4) * 4;
            if (do_store) st16<AUX>(ro, o, make_float4(a, a + 1.f, a + 2.f, a + 3.f));
        }
    }
    if (!do_store && a == 123.456f) out[0] = a;  // (keeps the spin alive in the store-less form)
}

__global__ void k_fill(float4* X, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) X[i] = make_float4(1.f, 2.f, 3.f, 4.f);
}
// the dependent successor: one block, reads one word of what the predecessor wrote
__global__ void k_dep(const float* src, float* sink) {
    if (threadIdx.x == 0) sink[0] = src[0] + 1.f;
}

int main() {
    const long P = 2363136, n4 = P / 4;
    float4 *p, *g, *m, *v, *junk;
    __bf16* s;
    float *slab, *sink;
    const long jn4 = 400L * 1024 * 1024 / 16;
    const long slab_bytes = 2L * SL_H * SL_NS * SL_D * 4;  // 75.5 MB
    CK(hipMalloc(&p, P * 4)); CK(hipMalloc(&g, P * 4)); CK(hipMalloc(&m, P * 4)); CK(hipMalloc(&v, P * 4));
    CK(hipMalloc(&s, P * 2)); CK(hipMalloc(&junk, jn4 * 16)); CK(hipMalloc(&slab, slab_bytes)); CK(hipMalloc(&sink, 256));
    CK(hipMemset(p, 0, P * 4)); CK(hipMemset(g, 0, P * 4)); CK(hipMemset(m, 0, P * 4)); CK(hipMemset(v, 0, P * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto time = [&](auto launch, const float* dep, float& avg, float& best) {
        best = 1e9f;
        float sum = 0.f;
        const int reps = 30;
        for (int r = 0; r < reps + 3; ++r) {
            k_fill<<<2048, 256>>>(junk, jn4);
            CK(hipEventRecord(e0));
            launch();
            if (dep) k_dep<<<1, 64>>>(dep, sink);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 3) { sum += ms; best = ms < best ? ms : best; }
        }
        avg = sum / reps;
    };
    auto run = [&](const char* name, double bytes, const float* dep, auto launch) {
        float a0, b0, a1, b1;
        time(launch, nullptr, a0, b0);
        time(launch, dep, a1, b1);
        printf("%-44s alone avg %6.2f best %6.2f us (%5.2f TB/s)   + dependent avg %6.2f best %6.2f us   delta %5.2f\n", name,
               a0 * 1e3, b0 * 1e3, bytes / (a0 * 1e-3) / 1e12, a1 * 1e3, b1 * 1e3, (a1 - a0) * 1e3);
        fflush(stdout);
    };
    {   // what the boundary itself costs: a trivial predecessor
        float a0, b0, a1, b1;
        time([&] { k_dep<<<1, 64>>>(sink + 8, sink + 16); }, nullptr, a0, b0);
        time([&] { k_dep<<<1, 64>>>(sink + 8, sink + 16); }, sink + 16, a1, b1);
        printf("%-44s alone avg %6.2f best %6.2f us                + dependent avg %6.2f best %6.2f us   delta %5.2f\n",
               "trivial one-block kernel", a0 * 1e3, b0 * 1e3, a1 * 1e3, b1 * 1e3, (a1 - a0) * 1e3);
    }
    const double ub = 7.0 * P * 4 + 2.0 * P;
    const int nb = (int)((n4 + 511) / 512);
#define UPD(NAME, AUX, WIDE, AUX_S) \
    run(NAME, ub, (const float*)p, [&] { k_upd<AUX, WIDE, AUX_S><<<nb, 256>>>(p, g, m, v, s, n4); })
    printf("-- upd: 71 MB read-modify-write, k_once<2> (%d blocks)\n", nb);
    UPD("upd pmv plain   | bf16 8 B plain", AUX_PLAIN, 0, AUX_PLAIN);
    UPD("upd pmv aux 16  | bf16 8 B plain", AUX_WT, 0, AUX_PLAIN);
    UPD("upd pmv aux 18  | bf16 8 B plain", AUX_WT_NT, 0, AUX_PLAIN);
    UPD("upd pmv plain   | bf16 16 B plain", AUX_PLAIN, 1, AUX_PLAIN);
    UPD("upd pmv plain   | bf16 16 B aux 16", AUX_PLAIN, 1, AUX_WT);
    UPD("upd pmv plain   | bf16 16 B aux 18", AUX_PLAIN, 1, AUX_WT_NT);
    UPD("upd pmv aux 16  | bf16 16 B plain", AUX_WT, 1, AUX_PLAIN);
    UPD("upd pmv aux 16  | bf16 16 B aux 16", AUX_WT, 1, AUX_WT);
    UPD("upd pmv aux 18  | bf16 16 B aux 18", AUX_WT_NT, 1, AUX_WT_NT);
    UPD("upd pmv plain   | bf16 8 B plain (again)", AUX_PLAIN, 0, AUX_PLAIN);
#undef UPD
    const int spin = 2412;  // dependent FMAs per wave: the order of the contraction in front of the real epilogue
#define SLAB(NAME, AUX, SPREAD, SPIN, ST) \
    run(NAME, (ST) ? (double)slab_bytes : 0.0, slab, [&] { k_slab<AUX, SPREAD><<<256, 512>>>(slab, slab_bytes, SPIN, ST); })
    printf("-- slab: 75.5 MB of 16-byte stores from 256 workgroups, spin = %d FMAs per wave\n", spin);
    SLAB("slab spin only, no stores", AUX_PLAIN, 0, spin, 0);
    SLAB("slab stores only      plain", AUX_PLAIN, 0, 0, 1);
    SLAB("slab stores only      aux 16", AUX_WT, 0, 0, 1);
    SLAB("slab stores only      aux 18", AUX_WT_NT, 0, 0, 1);
    SLAB("slab spin, then burst plain", AUX_PLAIN, 0, spin, 1);
    SLAB("slab spin, then burst aux 16", AUX_WT, 0, spin, 1);
    SLAB("slab spin, then burst aux 18", AUX_WT_NT, 0, spin, 1);
    SLAB("slab spread           plain", AUX_PLAIN, 1, spin, 1);
    SLAB("slab spread           aux 16", AUX_WT, 1, spin, 1);
    SLAB("slab spread           aux 18", AUX_WT_NT, 1, spin, 1);
    SLAB("slab spin, then burst plain (again)", AUX_PLAIN, 0, spin, 1);
#undef SLAB
    CK(hipDeviceSynchronize());
    return 0;
}
