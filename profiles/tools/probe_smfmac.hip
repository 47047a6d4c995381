// What does v_smfmac_f32_32x32x32_bf16 (2:4 structured-sparse A operand) compute on gfx950, can its B operand be taken
// from wgrad2's row-major LDS image, how fast does it issue, and does it round like the dense 32x32x16 form?
//   (a) operand semantics, found from one-hot runs and then checked exactly on small integers against a host product:
//       which B element each (lane half, A slot, 2-bit index) multiplies, which bits of the index register belong to which
//       slot, which half of the register ABID selects, what a zero-valued slot may carry as its index;
//   (b) the B fragment as four ds_read_b64_tr_b16 from the [64 batch rows][128 bytes] image with wgrad2's rm_swz swizzle;
//   (c) issue rate against v_mfma_f32_32x32x16_bf16: back to back, four independent accumulators per wave, two waves per
//       SIMD on every CU (the set-up of probe_mfma_loop.hip, MODE 0);
//   (d) bit equality with the dense form on a 1 %-dense A over a 2048-row contraction.
// hipcc --offload-arch=gfx950 -O3 probe_smfmac.hip -o probe_smfmac && ./probe_smfmac
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef __bf16 bf16_t;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);       \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

// ---- one instruction per wave: block c runs config c (A [64][8], B [64][16], idx [64], C/D [64][16]) ----
template <int ABID>
__global__ void __launch_bounds__(64) one_kernel(const bf16_t* A, const bf16_t* Bm, const int* idx, const float* C, float* D) {
    const int64_t c = blockIdx.x, l = threadIdx.x;
    const bf16x8 a = *(const bf16x8*)(A + (c * 64 + l) * 8);
    const bf16x16 b = *(const bf16x16*)(Bm + (c * 64 + l) * 16);
    f32x16 acc = *(const f32x16*)(C + (c * 64 + l) * 16);
    acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a, b, acc, idx[c * 64 + l], 0, ABID);
    *(f32x16*)(D + (c * 64 + l) * 16) = acc;
}

// ---- a chain of n K = 32 steps per wave (block c = problem c): sparse form and dense form ----
__global__ void __launch_bounds__(64) chain_sparse(const bf16_t* A, const bf16_t* Bm, const int* idx, float* D, int n) {
    const int64_t c = blockIdx.x, l = threadIdx.x;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int t = 0; t < n; ++t) {
        const int64_t o = (c * n + t) * 64 + l;
        acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(*(const bf16x8*)(A + o * 8), *(const bf16x16*)(Bm + o * 16), acc, idx[o], 0, 0);
    }
    *(f32x16*)(D + (c * 64 + l) * 16) = acc;
}
__global__ void __launch_bounds__(64) chain_dense(const bf16_t* A, const bf16_t* Bm, float* D, int n) {  // n K = 16 steps
    const int64_t c = blockIdx.x, l = threadIdx.x;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int t = 0; t < n; ++t) {
        const int64_t o = (c * n + t) * 64 + l;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(A + o * 8), *(const bf16x8*)(Bm + o * 8), acc, 0, 0, 0);
    }
    *(f32x16*)(D + (c * 64 + l) * 16) = acc;
}

// ---- (b): the B fragment from the row-major image.  img: [64 batch rows][64 columns] bf16, plain row-major in global;
// the kernel lays it out as wgrad2 does (16-byte chunk c of row r at slot c ^ rm_swz(r)) and multiplies the 32 x 64
// compressed A (two K = 32 steps: A [2][64][8], idx [2][64]) into D [2 column tiles][64][16]
__device__ __forceinline__ int rm_swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
__global__ void __launch_bounds__(64) trread_kernel(const bf16_t* img, const bf16_t* A, const int* idx, float* D) {
    __shared__ __attribute__((aligned(16))) char sm[64 * 128];
    const int lane = threadIdx.x;
    for (int ch = lane; ch < 64 * 8; ch += 64) {
        const int r = ch >> 3, c = ch & 7;
        *(uint4*)(sm + r * 128 + ((c ^ rm_swz(r)) << 4)) = *(const uint4*)(img + r * 64 + c * 8);
    }
    __syncthreads();
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;
    const int h = lane >> 5, i = lane & 15, g1 = (lane >> 4) & 1;
    for (int ni = 0; ni < 2; ++ni) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int t = 0; t < 2; ++t) {
            bf16x4 q[4];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int c0 = ni * 32 + g1 * 16 + 4 * (i & 3);     // first of this lane's 4 address columns
                const int row = 32 * t + 16 * h + 4 * q4 + (i >> 2);  // the 4-row block q4 of this half's 16 batch rows
                q[q4] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (lds_bf16x4_t*)(sm + row * 128 + (((c0 >> 3) ^ rm_swz(row)) << 4) + 8 * (i & 1)));
            }
            const bf16x8 lo = __builtin_shufflevector(q[0], q[1], 0, 1, 2, 3, 4, 5, 6, 7);
            const bf16x8 hi = __builtin_shufflevector(q[2], q[3], 0, 1, 2, 3, 4, 5, 6, 7);
            const bf16x16 b = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
            acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(*(const bf16x8*)(A + (t * 64 + lane) * 8), b, acc, idx[t * 64 + lane], 0, 0);
        }
        *(f32x16*)(D + (ni * 64 + lane) * 16) = acc;
    }
}

// ---- (c): issue rate.  24 instructions per trip on four independent accumulators, operands in registers ----
template <int SPARSE>
__global__ void __launch_bounds__(256, 2) rate_kernel(const bf16_t* src, float* out, int trips) {
    const int l = threadIdx.x;
    bf16x8 a[4];
    bf16x16 b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = *(const bf16x8*)(src + (l * 4 + j) * 8);
        b[j] = *(const bf16x16*)(src + 8192 + (l * 4 + j) * 16);
    }
    const int ix = ((const int*)(src + 24576))[l];
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int t = 0; t < trips; ++t) {
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            if constexpr (SPARSE)
                acc[u & 3] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a[u & 3], b[(u >> 2) & 3], acc[u & 3], ix, 0, 0);
            else
                acc[u & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u & 3], __builtin_shufflevector(b[(u >> 2) & 3], b[(u >> 2) & 3], 0, 1, 2, 3, 4, 5, 6, 7), acc[u & 3], 0, 0, 0);
        }
    }
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) v += acc[j][r];
    if (v == 12345.f) out[l] = v;
}

// ================================================ host ================================================
static uint16_t f2bf(float f) {  // round to nearest even
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf2f(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static float rnd_normal() {  // sum of 4 uniforms, good enough for a magnitude spread
    float s = 0.f;
    for (int i = 0; i < 4; ++i) s += (float)(rnd() & 0xFFFF) / 65536.f - 0.5f;
    return s * 1.7f;
}
template <typename T>
static T* to_dev(const std::vector<T>& v) {
    T* d;
    CHECK(hipMalloc(&d, v.size() * sizeof(T) + 64));
    CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
// C/D register r of lane l is element [row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][column l & 31] (as the dense 32x32 forms)
static int d_row(int l, int r) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }

// the model part (a) finds: slot s of a lane of half h owns bit field fld[h][s] (2 bits at 2 * fld) of the index register
// and, with index v there, multiplies B element sel_e[h][s][v] of the lanes of half sel_h[h][s][v]
static int fld[2][8], sel_h[2][8][4], sel_e[2][8][4];
static int klog(int h, int s, int v) { return 16 * sel_h[h][s][v] + sel_e[h][s][v]; }  // logical k = 16 * (B half) + (B element)

struct OneRun {
    std::vector<uint16_t> A, B;
    std::vector<int> idx;
    std::vector<float> C, D;
    int n = 0;
    int add() {
        A.resize((n + 1) * 64 * 8, 0);
        B.resize((n + 1) * 64 * 16, 0);
        idx.resize((n + 1) * 64, 0);
        C.resize((n + 1) * 64 * 16, 0.f);
        return n++;
    }
    void run(int abid) {
        D.assign((size_t)n * 64 * 16, -1.f);
        uint16_t *dA = to_dev(A), *dB = to_dev(B);
        int* di = to_dev(idx);
        float *dC = to_dev(C), *dD = to_dev(D);
        if (abid == 0) one_kernel<0><<<n, 64>>>((bf16_t*)dA, (bf16_t*)dB, di, dC, dD);
        else one_kernel<1><<<n, 64>>>((bf16_t*)dA, (bf16_t*)dB, di, dC, dD);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
        hipFree(dA); hipFree(dB); hipFree(di); hipFree(dC); hipFree(dD);
    }
};

// one-hot: A = 1 in slot s of the lanes of half h, index register = reg in every lane, B element e of half h' = 1 + e + 16 h'
// -> every output element = 1 + (logical k selected); returns -1 where the 1024 outputs are not all that one value
static void onehot_cfg(OneRun& R, int h, int s, uint32_t reg) {
    const int c = R.add();
    for (int l = 0; l < 64; ++l) {
        if ((l >> 5) == h) R.A[(c * 64 + l) * 8 + s] = f2bf(1.f);
        R.idx[c * 64 + l] = (int)reg;
        for (int e = 0; e < 16; ++e) R.B[(c * 64 + l) * 16 + e] = f2bf((float)(1 + e + 16 * (l >> 5)));
    }
}
static int onehot_read(const OneRun& R, int c) {
    const float v = R.D[(size_t)c * 1024];
    for (int i = 1; i < 1024; ++i)
        if (R.D[(size_t)c * 1024 + i] != v) return -1;
    return (int)v - 1;
}

static bool part_a_discover() {
    printf("== (a) operand semantics of v_smfmac_f32_32x32x32_bf16 ==\n");
    OneRun R;
    for (int h = 0; h < 2; ++h)
        for (int s = 0; s < 8; ++s)
            for (int p = 0; p < 16; ++p)
                for (int v = 0; v < 4; ++v) onehot_cfg(R, h, s, (uint32_t)v << (2 * p));
    R.run(0);
    bool ok = true, standard = true;
    printf("one-hot runs, CBSZ = 0, ABID = 0 (k is named by the B operand: k = 16 * (lane >> 5) + element):\n");
    for (int h = 0; h < 2; ++h)
        for (int s = 0; s < 8; ++s) {
            int nf = 0;
            fld[h][s] = -1;
            for (int p = 0; p < 16; ++p) {
                int k[4];
                for (int v = 0; v < 4; ++v) k[v] = onehot_read(R, ((h * 8 + s) * 16 + p) * 4 + v);
                const bool varies = k[0] != k[1] || k[0] != k[2] || k[0] != k[3];
                if (varies) {
                    ++nf;
                    fld[h][s] = p;
                    for (int v = 0; v < 4; ++v) {
                        if (k[v] < 0 || k[v] > 31) { ok = false; k[v] = 0; }
                        sel_h[h][s][v] = k[v] >> 4;
                        sel_e[h][s][v] = k[v] & 15;
                    }
                }
            }
            if (nf != 1) { ok = false; printf("  half %d slot %d: %d index fields change the result\n", h, s, nf); continue; }
            printf("  half %d slot %d: index bits [%2d:%2d]; index 0,1,2,3 -> k = %2d %2d %2d %2d\n", h, s, 2 * fld[h][s] + 1,
                   2 * fld[h][s], klog(h, s, 0), klog(h, s, 1), klog(h, s, 2), klog(h, s, 3));
            for (int v = 0; v < 4; ++v)
                if (fld[h][s] != s || klog(h, s, v) != 16 * h + 4 * (s >> 1) + v) standard = false;
        }
    printf("model complete: %s;  equals \"slot s: bits [2s+1:2s], k = 16 (lane>>5) + 4 (s>>1) + index\": %s\n", ok ? "yes" : "NO",
           ok && standard ? "yes" : "NO");
    return ok;
}

static void part_a_abid() {
    // the same one-hot runs with the index in the low / high 16 bits (the other half holds the complemented index) under
    // ABID = 0 and ABID = 1: which half is read
    for (int abid = 0; abid < 2; ++abid) {
        OneRun R;
        for (int hi = 0; hi < 2; ++hi)
            for (int h = 0; h < 2; ++h)
                for (int s = 0; s < 8; ++s)
                    for (int v = 0; v < 4; ++v) {
                        const uint32_t good = (uint32_t)v << (2 * fld[h][s]), bad = (uint32_t)(v ^ 3) << (2 * fld[h][s]);
                        onehot_cfg(R, h, s, hi ? (good << 16) | bad : (bad << 16) | good);
                    }
        R.run(abid);
        for (int hi = 0; hi < 2; ++hi) {
            int match = 0, c = hi * 64;
            for (int h = 0; h < 2; ++h)
                for (int s = 0; s < 8; ++s)
                    for (int v = 0; v < 4; ++v) match += onehot_read(R, c++) == klog(h, s, v);
            printf("ABID = %d, index in bits [%s]: %d of 64 one-hot runs select the expected k\n", abid, hi ? "31:16" : "15:0", match);
        }
    }
}

// Random 2:4 A (small integers) in the model's encoding.  mode 0: up to two non-zeros per group in ascending index order,
// an unused slot holds value 0 and index 0 | 1: unused slots carry a random index | 2: two non-zeros in DESCENDING order |
// 3: two non-zeros with the SAME index (host: both count).  Returns the number of wrong output elements.
static void part_a_exact() {
    // groups: the slots whose four selectable k are the same aligned group must come in pairs
    const char* names[4] = {"<= 2 non-zeros ascending, unused slot: value 0, index 0", "unused slot: value 0, random index",
                            "two non-zeros, descending index order", "two non-zeros, the same index (host counts both)"};
    for (int mode = 0; mode < 4; ++mode) {
        OneRun R;
        const int N = 64;
        std::vector<double> ref((size_t)N * 32 * 32);
        for (int c = 0; c < N; ++c) {
            R.add();
            double Al[32][32] = {}, Bl[32][32];
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 16; ++e) {
                    const int v = (int)(rnd() % 17) - 8;
                    R.B[(c * 64 + l) * 16 + e] = f2bf((float)v);
                    Bl[16 * (l >> 5) + e][l & 31] = v;
                }
            for (int l = 0; l < 64; ++l) {
                const int h = l >> 5, row = l & 31;
                uint32_t reg = rnd() << 16;  // (ABID = 0: the high half is noise)
                for (int s0 = 0; s0 < 8; s0 += 2) {
                    int nz = mode >= 2 ? 2 : (int)(rnd() % 3);
                    int i0 = rnd() & 3, i1 = rnd() & 3;
                    if (mode == 3) i1 = i0;
                    else {
                        while (i1 == i0) i1 = rnd() & 3;
                        if ((i0 > i1) != (mode == 2)) { const int t = i0; i0 = i1; i1 = t; }
                    }
                    int v0 = (int)(rnd() % 7) + 1, v1 = (int)(rnd() % 7) + 1;
                    if (rnd() & 1) v0 = -v0;
                    if (rnd() & 1) v1 = -v1;
                    if (nz < 2) { v1 = 0; i1 = mode == 1 ? (int)(rnd() & 3) : 0; }
                    if (nz < 1) { v0 = 0; i0 = mode == 1 ? (int)(rnd() & 3) : 0; }
                    if (nz == 1 && (rnd() & 1)) { int t = v0; v0 = v1; v1 = t; t = i0; i0 = i1; i1 = t; }  // the value in either slot
                    R.A[(c * 64 + l) * 8 + s0] = f2bf((float)v0);
                    R.A[(c * 64 + l) * 8 + s0 + 1] = f2bf((float)v1);
                    reg |= (uint32_t)i0 << (2 * fld[h][s0]) | (uint32_t)i1 << (2 * fld[h][s0 + 1]);
                    Al[row][klog(h, s0, i0)] += v0;
                    Al[row][klog(h, s0 + 1, i1)] += v1;
                }
                R.idx[c * 64 + l] = (int)reg;
                for (int r = 0; r < 16; ++r) R.C[(c * 64 + l) * 16 + r] = (float)((int)(rnd() % 9) - 4);
            }
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    double s = 0;
                    for (int k = 0; k < 32; ++k) s += Al[i][k] * Bl[k][j];
                    ref[((size_t)c * 32 + i) * 32 + j] = s;
                }
        }
        R.run(0);
        long bad = 0;
        for (int c = 0; c < N; ++c)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 16; ++r) {
                    const double want = ref[((size_t)c * 32 + d_row(l, r)) * 32 + (l & 31)] + R.C[(c * 64 + l) * 16 + r];
                    bad += (double)R.D[((size_t)c * 64 + l) * 16 + r] != want;
                }
        printf("exact against the host product, %d random 32x32x32 problems, %s: %ld of %d elements differ\n", N, names[mode], bad,
               N * 1024);
    }
}

// encode a logical 32 x 32 block row of A (at most two non-zeros per aligned group of four k) into one step's lane operands;
// slot = rank in ascending k order.  a: [32][32] floats (bf16-exact).  Returns false if a group has more than two non-zeros.
static bool encode_step(const float* a, int lda, uint16_t* Aout, int* idx_out) {
    // inverse of the model: for logical k, the (half, slot pair) that can select it
    for (int l = 0; l < 64; ++l) {
        const int h = l >> 5, row = l & 31;
        uint32_t reg = 0;
        for (int s0 = 0; s0 < 8; s0 += 2) {
            int n = 0;
            for (int v = 0; v < 4; ++v) {
                const float x = a[row * lda + klog(h, s0, v)];
                if (x == 0.f) continue;
                if (n == 2) return false;
                Aout[l * 8 + s0 + n] = f2bf(x);
                reg |= (uint32_t)v << (2 * fld[h][s0 + n]);
                ++n;
            }
        }
        idx_out[l] = (int)reg;
    }
    return true;
}

static void part_b() {
    printf("== (b) B fragment by four ds_read_b64_tr_b16 from the row-major image (rm_swz swizzle) ==\n");
    std::vector<uint16_t> img(64 * 64), A(2 * 64 * 8, 0);
    std::vector<int> idx(2 * 64, 0);
    std::vector<float> Al(32 * 64, 0.f), Bl(64 * 64), D(2 * 64 * 16, -1.f);
    for (int i = 0; i < 64 * 64; ++i) {
        Bl[i] = (float)((int)(rnd() % 17) - 8);
        img[i] = f2bf(Bl[i]);
    }
    for (int i = 0; i < 32; ++i)
        for (int g = 0; g < 16; ++g) {
            const int nz = rnd() % 3;
            int k0 = rnd() & 3, k1 = rnd() & 3;
            while (k1 == k0) k1 = rnd() & 3;
            if (nz >= 1) Al[i * 64 + 4 * g + k0] = (float)((int)(rnd() % 7) + 1);
            if (nz >= 2) Al[i * 64 + 4 * g + k1] = -(float)((int)(rnd() % 7) + 1);
        }
    for (int t = 0; t < 2; ++t) encode_step(Al.data() + 32 * t, 64, A.data() + t * 512, idx.data() + t * 64);
    uint16_t *dimg = to_dev(img), *dA = to_dev(A);
    int* di = to_dev(idx);
    float* dD = to_dev(D);
    trread_kernel<<<1, 64>>>((bf16_t*)dimg, (bf16_t*)dA, di, dD);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int ni = 0; ni < 2; ++ni)
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 16; ++r) {
                double s = 0;
                for (int k = 0; k < 64; ++k) s += (double)Al[d_row(l, r) * 64 + k] * Bl[k * 64 + ni * 32 + (l & 31)];
                bad += (double)D[(ni * 64 + l) * 16 + r] != s;
            }
    printf("A [32 x 64 batch rows] x image [64 batch rows x 64 columns], two K = 32 steps, group = 4 consecutive batch rows:\n"
           "  %d of 2048 elements differ from the host product\n", bad);
}

static void part_c() {
    printf("== (c) issue rate, 512 workgroups x 4 waves, 2 waves per SIMD, 4 independent accumulators, 24 per trip ==\n");
    std::vector<uint16_t> src(8192 + 16384 + 512);
    for (auto& v : src) v = f2bf((float)((int)(rnd() % 5) - 2));
    for (int l = 0; l < 256; ++l) { src[24576 + 2 * l] = (uint16_t)(rnd() & 0xFFFF); src[24576 + 2 * l + 1] = 0; }  // index words
    uint16_t* d = to_dev(src);
    float* out;
    CHECK(hipMalloc(&out, 4096));
    const int trips = 4000, blocks = 512;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float ms[2][3];
    for (int rep = 0; rep < 3; ++rep)
        for (int sp = 0; sp < 2; ++sp) {
            if (sp) rate_kernel<1><<<blocks, 256>>>((bf16_t*)d, out, 50); else rate_kernel<0><<<blocks, 256>>>((bf16_t*)d, out, 50);
            hipEventRecord(e0);
            if (sp) rate_kernel<1><<<blocks, 256>>>((bf16_t*)d, out, trips); else rate_kernel<0><<<blocks, 256>>>((bf16_t*)d, out, trips);
            hipEventRecord(e1);
            CHECK(hipEventSynchronize(e1));
            hipEventElapsedTime(&ms[sp][rep], e0, e1);
        }
    for (int sp = 0; sp < 2; ++sp)
        for (int rep = 0; rep < 3; ++rep) {
            const double per = ms[sp][rep] * 1e6 / ((double)trips * 24 * 2);  // a SIMD runs two waves' instructions
            const double inst = (double)blocks * 4 * trips * 24;
            printf("  %-28s run %d: %.3f ms, %.2f ns per instruction and SIMD, %.0f TFLOP/s %s\n",
                   sp ? "v_smfmac_f32_32x32x32_bf16" : "v_mfma_f32_32x32x16_bf16", rep, ms[sp][rep], per,
                   inst * (sp ? 65536.0 : 32768.0) / (ms[sp][rep] * 1e-3) / 1e12, sp ? "(dense-equivalent, K = 32)" : "");
        }
    double bs = ms[1][0], bd = ms[0][0];
    for (int rep = 1; rep < 3; ++rep) { bs = ms[1][rep] < bs ? ms[1][rep] : bs; bd = ms[0][rep] < bd ? ms[0][rep] : bd; }
    printf("  cycles_sparse / cycles_dense = %.3f (best of 3 each); one sparse instruction replaces two dense ones, so the\n"
           "  matrix-pipe time of a K = 32 step changes by the factor %.3f\n", bs / bd, bs / (2 * bd));
}

static void part_d() {
    printf("== (d) bit equality with the dense form: 1 %%-dense A, B = 2048 batch rows, 64 tiles of 32 x 32 ==\n");
    const int N = 64, K = 2048, NS = K / 32, ND = K / 16;
    std::vector<uint16_t> As((size_t)N * NS * 512, 0), Bs((size_t)N * NS * 1024), Ad((size_t)N * ND * 512, 0), Bd((size_t)N * ND * 512);
    std::vector<int> idx((size_t)N * NS * 64, 0);
    std::vector<float> Al(32 * K), Bl((size_t)K * 32);
    long nnz = 0, dropped = 0;
    for (int c = 0; c < N; ++c) {
        for (auto& v : Al) v = 0.f;
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < K; ++k)
                if (rnd() % 100 == 0) {
                    float x = bf2f(f2bf(rnd_normal() * ((rnd() & 3) == 0 ? 8.f : 1.f)));
                    Al[i * K + k] = x == 0.f ? 1.f : x;
                }
        // (keep the 2:4 pattern: a third entry of a group is dropped - the kernel would put it into a second layer)
        for (int i = 0; i < 32; ++i)
            for (int g = 0; g < K / 4; ++g) {
                int n = 0;
                for (int v = 0; v < 4; ++v)
                    if (Al[i * K + 4 * g + v] != 0.f) {
                        if (++n > 2) { Al[i * K + 4 * g + v] = 0.f; ++dropped; } else ++nnz;
                    }
            }
        for (auto& v : Bl) v = bf2f(f2bf(rnd_normal()));
        for (int t = 0; t < NS; ++t) {
            const size_t o = (size_t)c * NS + t;
            encode_step(Al.data() + 32 * t, K, As.data() + o * 512, idx.data() + o * 64);
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 16; ++e) Bs[o * 1024 + l * 16 + e] = f2bf(Bl[(size_t)(32 * t + 16 * (l >> 5) + e) * 32 + (l & 31)]);
        }
        for (int u = 0; u < ND; ++u) {
            const size_t o = (size_t)c * ND + u;
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * u + 8 * (l >> 5) + j;
                    Ad[o * 512 + l * 8 + j] = f2bf(Al[(l & 31) * K + k]);
                    Bd[o * 512 + l * 8 + j] = f2bf(Bl[(size_t)k * 32 + (l & 31)]);
                }
        }
    }
    uint16_t *dAs = to_dev(As), *dBs = to_dev(Bs), *dAd = to_dev(Ad), *dBd = to_dev(Bd);
    int* di = to_dev(idx);
    std::vector<float> Ds((size_t)N * 1024, -1.f), Dd((size_t)N * 1024, -2.f);
    float *dDs = to_dev(Ds), *dDd = to_dev(Dd);
    chain_sparse<<<N, 64>>>((bf16_t*)dAs, (bf16_t*)dBs, di, dDs, NS);
    chain_dense<<<N, 64>>>((bf16_t*)dAd, (bf16_t*)dBd, dDd, ND);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(Ds.data(), dDs, Ds.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(Dd.data(), dDd, Dd.size() * 4, hipMemcpyDeviceToHost));
    long eq = 0, nonzero = 0;
    double maxrel = 0;
    for (size_t i = 0; i < Ds.size(); ++i) {
        eq += memcmp(&Ds[i], &Dd[i], 4) == 0;
        nonzero += Dd[i] != 0.f;
        if (Dd[i] != 0.f) { const double r = fabs((double)Ds[i] - Dd[i]) / fabs((double)Dd[i]); maxrel = r > maxrel ? r : maxrel; }
    }
    printf("  %.1f non-zero terms per output element on average (%ld third entries of a group dropped), %ld of %zu outputs non-zero\n",
           (double)nnz / (N * 32), dropped, nonzero, Ds.size());
    printf("  sparse == dense bit for bit: %ld of %zu elements (%.4f %%), largest relative difference %.3g\n", eq, Ds.size(),
           100.0 * eq / Ds.size(), maxrel);
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("device: %s (%s), %d CUs\n", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    if (!part_a_discover()) {
        printf("the one-hot runs do not give a complete operand model: stopping before the parts that need it\n");
        return 1;
    }
    part_a_abid();
    part_a_exact();
    part_b();
    part_c();
    part_d();
    return 0;
}
