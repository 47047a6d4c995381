// Log-mel front end: waveforms in, Whisper's input_features out - framing with the reflected
// borders, the windowed DFT, the power spectrum, the mel filter bank, log10 and the per-utterance clamp - as two kernels.
// The contract, operation by operation, is in include/wsae.h; tests/logmel_oracle.py restates it.
//
// logmel_kernel: a workgroup owns LM_TILE = 64 frames of one utterance, a wave 16 of them.
//   Staging.  The tile's sample span (63 * 160 + 400 = 10480 samples) goes to LDS once: reflection around n_samples, zeros
//   from length[u] on and the int16 scaling happen here, with non-temporal loads (a sample is read by at most two tiles).
//   Frames overlap, so the A operand of frame i at sample n is s_x[160 i + n]: nothing is framed in memory.
//   DFT.  64 x 416 outputs = 4 x 26 tiles of v_mfma_f32_16x16x4_f32; a wave holds the 26 tiles of its 16 frames (104
//   accumulator registers).  The basis streams from L2 in slabs of LM_KS = 8 rows: a slab is fetched into registers
//   under the MFMAs of the slab before it and goes to LDS between two barriers.  The slab's row stride (432 words) puts
//   the four k rows of a B fragment on disjoint banks.  Every (frame, column) is ONE accumulator chain over n = 0 .. 399
//   in ascending order, whatever the tile or the wave.
//   The suggested shape (32x32x2, a double-buffered 16-row slab) needs 97 KB of LDS and one workgroup per CU; this one
//   stays under the 64 KB a static allocation may take (55 744 B) so that two workgroups share a CU and one's MFMAs
//   cover the other's barriers.  The n / 400 - n fold is not used: it would double the A fragments and halve nothing of
//   the staging.
//   Tail.  re (column k) and im (column 208 + k) of a bin are tiles ct and ct + 13 of the SAME lane and register, so the
//   power needs no exchange.  It goes to a [frame][bin] tile in LDS (over the dead samples and slab; stride 212 words:
//   conflict-free both ways), which is the A operand of the mel contraction (52 k steps over the 208 padded bins); the B
//   operand is the caller's filter bank, read from L1/L2 (100 KB at most, shared by every workgroup).  A lane ends with
//   four consecutive frames of one mel row: one 16-byte store along t, 64-byte pieces per wave.
// logmel_finish_kernel reduces an utterance's tile maxima (a float maximum: any order gives the same bits) and applies
// max(v, M - 8) and (v + 4) / 4 in place.
#include <math.h>

#include "wsae_common.h"
#include "wsae_pcm.h"

// re * re + im * im is two products and one sum, each rounded: the oracle has no fused multiply-add there
#pragma clang fp contract(off)

namespace {

constexpr int LM_BLOCK = 256, LM_WAVES = LM_BLOCK / 64;
constexpr int LM_TILE = 64;                                          // frames a workgroup owns (16 per wave)
constexpr int LM_N = WSAE_LOGMEL_NFFT, LM_HOP = WSAE_LOGMEL_HOP;     // 400, 160
constexpr int LM_SPAN = (LM_TILE - 1) * LM_HOP + LM_N;               // samples behind a tile
constexpr int LM_COLS = WSAE_LOGMEL_COLS, LM_CT = LM_COLS / 16;      // 416 basis columns = 26 tiles of 16
constexpr int LM_IM = WSAE_LOGMEL_SIN_COL / 16;                      // the sine column of bin k is 13 tiles after its cosine
constexpr int LM_KS = 8;                                             // basis rows per slab
constexpr int LM_BSTRIDE = 432;                                      // words between two rows of the slab in LDS
constexpr int LM_SLAB4 = LM_KS * LM_COLS / 4;                        // float4 of a slab (832)
constexpr int LM_PRE = (LM_SLAB4 + LM_BLOCK - 1) / LM_BLOCK;         // float4 a thread prefetches (4; the last partly)
constexpr int LM_KB = LM_IM * 16;                                    // 208: the bins, padded to the k step
constexpr int LM_PSTRIDE = 212;                                      // words between two frames of the power tile
constexpr int LM_LDS = LM_SPAN + LM_KS * LM_BSTRIDE;                 // floats
constexpr int LM_FIN_FRAMES = 4 * LM_BLOCK;                          // frames a workgroup of the finish kernel owns
static_assert(LM_N % LM_KS == 0 && LM_KS % 4 == 0 && LM_COLS % 16 == 0 && LM_CT == 2 * LM_IM, "tiling");
static_assert(LM_BSTRIDE >= LM_COLS && LM_BSTRIDE % 4 == 0 && LM_BSTRIDE % 64 == 48, "slab rows: 16-byte aligned, k rows on disjoint banks");
static_assert(LM_SPAN % 4 == 0, "the slab starts on a 16-byte boundary");
static_assert(LM_WAVES * 16 * LM_PSTRIDE <= LM_LDS && LM_PSTRIDE >= LM_KB && LM_PSTRIDE % 64 == 20, "power tile");
static_assert(LM_LDS * 4 <= 64 * 1024, "static LDS");

struct LogmelArgs {
    const void* x;
    int64_t ld_x;
    const int32_t* length;
    int32_t max_length;
    int32_t P, T, tiles;
    const float* basis;
    const float* filt;
    float* out;
    float* mel_power;
    int64_t ld_m, ld_u;
    float* tile_max;
    int vec;  // 1: 16-byte stores are aligned (out, mel_power, ld_m, ld_u)
    int wt;   // 1: and a wave's 64-byte pieces are whole lines' parts, so the bulk outputs go write-through
};

__device__ __forceinline__ void store4(float* base, int64_t off, const float4& v, bool wt) {
    if (wt) wt_store4(wt_rsrc(base), off * 4, v);
    else *(float4*)(base + off) = v;
}

template <int DT, int NM>
__global__ __launch_bounds__(LM_BLOCK, 2) void logmel_kernel(LogmelArgs a) {
    constexpr int MT = NM / 16;
    __shared__ __attribute__((aligned(16))) float s_mem[LM_LDS];
    __shared__ float s_red[LM_WAVES];
    float* s_x = s_mem;
    float* s_b = s_mem + LM_SPAN;
    const int u = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles, t0 = tile * LM_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int len = min(max(a.length[u], 0), a.max_length);

    // the first slab is on its way while the samples are staged
    const float4* b4 = (const float4*)a.basis;
    float4 pre[LM_PRE];
#pragma unroll
    for (int p = 0; p < LM_PRE; ++p) {
        const int i = threadIdx.x + p * LM_BLOCK;
        pre[p] = i < LM_SLAB4 ? b4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    {
        const int64_t xu = (int64_t)u * a.ld_x;
        const int q0 = t0 * LM_HOP - LM_N / 2;  // signal index of the span's first sample
        for (int j = threadIdx.x; j < LM_SPAN; j += LM_BLOCK) {
            int s = q0 + j;
            if (s < 0) s = -s;                          // (at most 200 < P)
            else if (s >= a.P) s = 2 * (a.P - 1) - s;   // negative for the frames of a ragged tile that do not exist
            s_x[j] = s >= 0 && s < len ? pcm_load<DT, true>(a.x, xu + s) : 0.f;
        }
    }

    f32x4 acc[LM_CT];
#pragma unroll
    for (int c = 0; c < LM_CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xa = s_x + (wave * 16 + li) * LM_HOP + lk;
    const float* ba = s_b + lk * LM_BSTRIDE + li;
    for (int s = 0; s < LM_N / LM_KS; ++s) {
        __syncthreads();  // the slab before this one has been read (first pass: nothing to wait for but harmless)
#pragma unroll
        for (int p = 0; p < LM_PRE; ++p) {
            const int i = threadIdx.x + p * LM_BLOCK;
            if (i < LM_SLAB4) *(float4*)(s_b + (i / (LM_COLS / 4)) * LM_BSTRIDE + 4 * (i % (LM_COLS / 4))) = pre[p];
        }
        __syncthreads();  // (first pass: the samples are staged too)
        if (s + 1 < LM_N / LM_KS) {
#pragma unroll
            for (int p = 0; p < LM_PRE; ++p) {
                const int i = threadIdx.x + p * LM_BLOCK;
                if (i < LM_SLAB4) pre[p] = b4[(s + 1) * LM_SLAB4 + i];
            }
        }
#pragma unroll
        for (int kk = 0; kk < LM_KS / 4; ++kk) {
            const float av = xa[s * LM_KS + 4 * kk];
#pragma unroll
            for (int c = 0; c < LM_CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ba[4 * kk * LM_BSTRIDE + 16 * c], acc[c], 0, 0, 0);
        }
    }
    __syncthreads();  // samples and slab are dead: the power tile goes over them

    // power: lane (li, lk), register r = frame 4 lk + r of the wave, bin 16 ct + li
    float* s_p = s_mem + wave * 16 * LM_PSTRIDE;
#pragma unroll
    for (int c = 0; c < LM_IM; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float re = acc[c][r], im = acc[c + LM_IM][r];
            s_p[(4 * lk + r) * LM_PSTRIDE + 16 * c + li] = re * re + im * im;
        }
    }
    __syncthreads();

    // mel: A = power [frame li][bin 4 ks + lk], B = filt [bin][mel 16 mt + li]; bins 201 .. 207 are padding
    f32x4 mel[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) mel[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < LM_KB / 4; ++ks) {
        const int k = 4 * ks + lk;
        const float av = s_p[li * LM_PSTRIDE + k];
        const float* fk = a.filt + (k < WSAE_LOGMEL_BINS ? k : 0) * NM + li;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float bv = k < WSAE_LOGMEL_BINS ? fk[16 * m] : 0.f;
            mel[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, mel[m], 0, 0, 0);
        }
    }

    // lane (li, lk), register r = mel row 16 mt + li, frame t0 + 16 wave + 4 lk + r
    const int t = t0 + wave * 16 + 4 * lk;
    float* ou = a.out + (int64_t)u * a.ld_u;
    float* pu = a.mel_power ? a.mel_power + (int64_t)u * a.ld_u : nullptr;
    const bool full = a.vec && t + 3 < a.T;
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int64_t off = (int64_t)(16 * m + li) * a.ld_m + t;
        float lg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            lg[r] = mel[m][r] > WSAE_LOGMEL_FLOOR ? log10f(mel[m][r]) : -10.0f;
            if (t + r < a.T) mx = fmaxf(mx, lg[r]);
        }
        if (full) {
            store4(ou, off, make_float4(lg[0], lg[1], lg[2], lg[3]), false);  // (the finish kernel reads it again)
            if (pu) store4(pu, off, make_float4(mel[m][0], mel[m][1], mel[m][2], mel[m][3]), a.wt);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (t + r < a.T) {
                    ou[off + r] = lg[r];
                    if (pu) pu[off + r] = mel[m][r];
                }
            }
        }
    }
    mx = block_max(mx, s_red);
    if (threadIdx.x == 0) a.tile_max[(int64_t)u * a.tiles + tile] = mx;
}

template <int NM>
__global__ __launch_bounds__(LM_BLOCK) void logmel_finish_kernel(LogmelArgs a, int chunks) {
    __shared__ float s_red[LM_WAVES];
    const int u = blockIdx.x / chunks, t = (blockIdx.x % chunks) * LM_FIN_FRAMES + 4 * threadIdx.x;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < a.tiles; i += LM_BLOCK) mx = fmaxf(mx, a.tile_max[(int64_t)u * a.tiles + i]);
    const float thr = block_max(mx, s_red) - 8.0f;
    if (t >= a.T) return;
    float* ou = a.out + (int64_t)u * a.ld_u;
    const bool full = a.vec && t + 3 < a.T;
    for (int m = 0; m < NM; ++m) {
        const int64_t off = (int64_t)m * a.ld_m + t;
        if (full) {
            float4 v = *(const float4*)(ou + off);
            v.x = (fmaxf(v.x, thr) + 4.0f) / 4.0f;
            v.y = (fmaxf(v.y, thr) + 4.0f) / 4.0f;
            v.z = (fmaxf(v.z, thr) + 4.0f) / 4.0f;
            v.w = (fmaxf(v.w, thr) + 4.0f) / 4.0f;
            store4(ou, off, v, a.wt);
        } else {
            for (int r = 0; r < 4 && t + r < a.T; ++r) ou[off + r] = (fmaxf(ou[off + r], thr) + 4.0f) / 4.0f;
        }
    }
}

constexpr int LM_MAX_UTT = 1 << 16;
constexpr int64_t LM_MAX_SAMPLES = 1 << 28;
constexpr int64_t LM_MAX_LD_M = 1 << 21;  // 128 rows of it stay below the 2^31 bytes a buffer store addresses

inline bool samples_ok(int64_t P) { return P >= 3 * LM_HOP && P <= LM_MAX_SAMPLES && P % LM_HOP == 0; }
inline bool mels_ok(int n_mels) { return n_mels == 80 || n_mels == 128; }

template <int DT>
void launch_logmel(int n_mels, int grid, hipStream_t st, const LogmelArgs& a) {
    if (n_mels == 80) logmel_kernel<DT, 80><<<grid, LM_BLOCK, 0, st>>>(a);
    else logmel_kernel<DT, 128><<<grid, LM_BLOCK, 0, st>>>(a);
}

}  // namespace

extern "C" int64_t wsae_logmel_workspace_bytes(int32_t n_utt, int64_t n_samples, int32_t n_mels) {
    if (n_utt < 0 || n_utt > LM_MAX_UTT || !samples_ok(n_samples) || !mels_ok(n_mels)) return -1;
    return align256((int64_t)sizeof(float) * n_utt * ceil_div64(n_samples / LM_HOP, LM_TILE));
}

extern "C" int wsae_logmel(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, const int32_t* length, int64_t max_length,
                           int64_t n_samples, const float* basis, const float* filt, int32_t n_mels, float* out, int64_t ld_m,
                           int64_t ld_u, float* mel_power, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(x && length && basis && filt && out, "wsae_logmel: null pointer");
    PCM_REQUIRE_DTYPE("wsae_logmel", x_dtype);
    WSAE_REQUIRE(n_utt >= 0 && n_utt <= LM_MAX_UTT, "wsae_logmel: need 0 <= n_utt <= %d (got %d)", LM_MAX_UTT, n_utt);
    WSAE_REQUIRE(samples_ok(n_samples), "wsae_logmel: n_samples must be a multiple of %d in %d .. %lld (got %lld)", LM_HOP, 3 * LM_HOP,
                 (long long)LM_MAX_SAMPLES, (long long)n_samples);
    WSAE_REQUIRE(mels_ok(n_mels), "wsae_logmel: n_mels must be 80 or 128 (got %d)", n_mels);
    WSAE_REQUIRE(max_length >= 0 && max_length <= n_samples, "wsae_logmel: need 0 <= max_length <= n_samples = %lld (got %lld)",
                 (long long)n_samples, (long long)max_length);
    WSAE_REQUIRE(ld_x >= max_length && ld_x >= 1, "wsae_logmel: ld_x %lld is below max_length %lld", (long long)ld_x, (long long)max_length);
    const int64_t T = n_samples / LM_HOP;
    WSAE_REQUIRE(ld_m >= T && ld_m <= LM_MAX_LD_M, "wsae_logmel: need %lld frames <= ld_m <= %lld (got %lld)", (long long)T,
                 (long long)LM_MAX_LD_M, (long long)ld_m);
    WSAE_REQUIRE(ld_u >= n_mels * ld_m, "wsae_logmel: ld_u %lld is below n_mels * ld_m = %lld", (long long)ld_u, (long long)(n_mels * ld_m));
    PCM_REQUIRE_ELEMENTS_ALIGNED("wsae_logmel", x, x_dtype, out, WSAE_DT_F32);
    WSAE_REQUIRE(((uintptr_t)basis & 15) == 0 && ((uintptr_t)filt & 3) == 0, "wsae_logmel: basis must be 16-byte aligned, filt 4-byte");
    const int64_t need = wsae_logmel_workspace_bytes(n_utt, n_samples, n_mels);
    WSAE_REQUIRE_WORKSPACE("wsae_logmel", workspace, workspace_bytes, need, n_utt);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_logmel", workspace, 4);
    if (n_utt == 0) return WSAE_OK;
    const int tiles = (int)ceil_div64(T, LM_TILE), chunks = (int)ceil_div64(T, LM_FIN_FRAMES);
    WSAE_REQUIRE((int64_t)n_utt * tiles <= 0x7fffffffll, "wsae_logmel: n_utt * n_samples is too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    LogmelArgs a = {x, ld_x, length, (int32_t)max_length, (int32_t)n_samples, (int32_t)T, tiles, basis, filt, out, mel_power, ld_m, ld_u,
                    (float*)workspace, 0, 0};
    a.vec = ((uintptr_t)out & 15) == 0 && ((uintptr_t)mel_power & 15) == 0 && ld_m % 4 == 0 && ld_u % 4 == 0;
    a.wt = a.vec && ((uintptr_t)out & 63) == 0 && ((uintptr_t)mel_power & 63) == 0 && ld_m % 16 == 0 && ld_u % 16 == 0;
    if (x_dtype == WSAE_DT_F32) launch_logmel<WSAE_DT_F32>(n_mels, n_utt * tiles, st, a);
    else launch_logmel<WSAE_DT_I16>(n_mels, n_utt * tiles, st, a);
    WSAE_LAUNCH_CHECK();
    if (n_mels == 80) logmel_finish_kernel<80><<<n_utt * chunks, LM_BLOCK, 0, st>>>(a, chunks);
    else logmel_finish_kernel<128><<<n_utt * chunks, LM_BLOCK, 0, st>>>(a, chunks);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
