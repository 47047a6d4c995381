// What the audio kernels share (wsae_logmel.hip, wsae_clips.hip, wsae_resample.hip).
// Host side: the checks on a bank of waveforms, one macro per requirement (PCM_REQUIRE_*).
// Input side: one sample as float (PcmIn, pcm_load) and the walk over a span of frames that begins at an arbitrary element:
// scalar loads up to the first 16-byte boundary, 16-byte loads from there, scalar loads behind the last whole vector
// (pcm_for_span).
// Output side (wsae_clips.hip, wsae_resample.hip): the float32 -> PCM conversion and the store of a tile of outputs that
// sits in LDS to a destination of arbitrary alignment (DESIGN.md sections 30 and 31).
//
// The tile's cells are staged in LDS shifted by the cells that lead up to the destination's first 64-byte boundary, so that
// from that boundary on a lane stores 16 aligned bytes and a wave instruction whole 64-byte pieces: those go write-through
// (DESIGN.md 4.1), the at most three vectors behind the last whole piece plain, the ragged ends elementwise.  The same
// values whatever the alignment.
#pragma once

#include "wsae_common.h"

// ---- host side: the checks on a bank of waveforms ----------------------------------------------------------------------
// FN: the entry point's name, a string literal.  One macro per requirement: every entry point has checks of its own between
// them, and the order of the checks decides which message a caller with two mistakes gets.
inline bool pcm_dtype_ok(int dt) { return dt == WSAE_DT_F32 || dt == WSAE_DT_I16; }
inline uintptr_t pcm_elem_mask(int dt) { return dt == WSAE_DT_I16 ? 1 : 3; }
template <class... P>
inline uintptr_t ptr_bits(P... p) { return (uintptr_t(0) | ... | (uintptr_t)p); }

#define PCM_REQUIRE_DTYPE(FN, dt) WSAE_REQUIRE(pcm_dtype_ok(dt), FN ": unknown " #dt " %d (float32 or int16)", dt)
#define PCM_REQUIRE_N_UTT(FN, n_utt) WSAE_REQUIRE((n_utt) >= 0, FN ": n_utt must not be negative (got %d)", n_utt)
#define PCM_REQUIRE_MAX_LENGTH(FN, max_length)                                                                        \
    WSAE_REQUIRE((max_length) >= 0 && (max_length) <= 0x7fffffffll, FN ": need 0 <= max_length < 2^31 (got %lld)",    \
                 (long long)(max_length))
// a row holds `need` elements, which the message calls WHAT ("max_length", "max_length * channels =")
#define PCM_REQUIRE_LD_X(FN, ld_x, need, WHAT) \
    WSAE_REQUIRE((ld_x) >= (need), FN ": ld_x %lld is below " WHAT " %lld", (long long)(ld_x), (long long)(need))
#define PCM_REQUIRE_ELEMENTS_ALIGNED(FN, x, x_dtype, out, out_dtype)                                           \
    WSAE_REQUIRE(((uintptr_t)(x) & pcm_elem_mask(x_dtype)) == 0 && ((uintptr_t)(out) & pcm_elem_mask(out_dtype)) == 0, \
                 FN ": x and out must be aligned to their elements")
// bits4, bits8: ptr_bits() of the tables that need 4- and 8-byte alignment; TEXT names them
#define PCM_REQUIRE_TABLES_ALIGNED(FN, bits4, bits8, TEXT) \
    WSAE_REQUIRE(((bits4) & 3) == 0 && ((bits8) & 7) == 0, FN ": " TEXT)

#ifdef __HIPCC__

// ---- input side --------------------------------------------------------------------------------------------------------
// A sample type: its element, the 16-byte vector of VE of them, and the element as float (int16 is scaled by 2^-15, exact).
template <int DT> struct PcmIn;
template <> struct PcmIn<WSAE_DT_F32> {
    typedef float elem;
    typedef f32x4 vec;
    static constexpr int VE = 4;
    static __device__ __forceinline__ float to_f32(float v) { return v; }
};
template <> struct PcmIn<WSAE_DT_I16> {
    typedef int16_t elem;
    typedef short vec __attribute__((ext_vector_type(8)));
    static constexpr int VE = 8;
    static __device__ __forceinline__ float to_f32(int16_t v) { return (float)v * 0x1p-15f; }
};

// element i of p as float; NT: with the non-temporal hint
template <int DT, bool NT = false>
__device__ __forceinline__ float pcm_load(const void* p, int64_t i) {
    const typename PcmIn<DT>::elem* e = (const typename PcmIn<DT>::elem*)p + i;
    if constexpr (NT) return PcmIn<DT>::to_f32(__builtin_nontemporal_load(e));
    else return PcmIn<DT>::to_f32(*e);
}

// f(k, mono_k) exactly once for every frame k in [0, n) of the CH interleaved channels at p (aligned to a frame), by the
// BLOCK threads of the workgroup; mono_k is the sample, for CH == 2 (s0 + s1) / 2.0f.  Scalar loads up to the first 16-byte
// boundary, then 16-byte loads in batches of PER per thread - all loads of a batch issue before the first use -, scalar
// loads behind the last whole vector.  Nothing outside the n frames is read.
template <int DT, int CH, int BLOCK, int PER, class F>
__device__ __forceinline__ void pcm_for_span(const void* p, int n, F&& f) {
    typedef PcmIn<DT> In;
    static_assert(CH == 1 || CH == 2, "mono or stereo");
    constexpr int FB = CH * (int)sizeof(typename In::elem), FV = 16 / FB;  // bytes per frame, frames per vector
    const int tid = threadIdx.x;
    const int lead = min((int)(((16 - ((uintptr_t)p & 15)) & 15) / FB), n);
    const int nvec = (n - lead) / FV, done = lead + nvec * FV;
    auto frame = [&](int k) -> float {
        const float s = pcm_load<DT>(p, (int64_t)k * CH);
        if constexpr (CH == 2) return (s + pcm_load<DT>(p, (int64_t)k * CH + 1)) / 2.0f;
        else return s;
    };
    if (tid < lead) f(tid, frame(tid));
    const typename In::vec* pv = (const typename In::vec*)((const char*)p + lead * FB);
    for (int v0 = tid; v0 < nvec; v0 += PER * BLOCK) {
        typename In::vec q[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (v0 + k * BLOCK < nvec) q[k] = pv[v0 + k * BLOCK];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int v = v0 + k * BLOCK;
            if (v < nvec) {
#pragma unroll
                for (int i = 0; i < FV; ++i) {
                    const float s = In::to_f32(q[k][CH * i]);
                    if constexpr (CH == 2) f(lead + v * FV + i, (s + In::to_f32(q[k][CH * i + 1])) / 2.0f);
                    else f(lead + v * FV + i, s);
                }
            }
        }
    }
    if (done + tid < n) f(done + tid, frame(done + tid));  // (fewer than FV of them)
}

// ---- output side -------------------------------------------------------------------------------------------------------
template <int OT> struct PcmOut { typedef float type; };
template <> struct PcmOut<WSAE_DT_I16> { typedef int16_t type; };

// WSAE_DT_I16: clamp(rintf(fl(y * scale)), -32768, 32767), round half to even; WSAE_DT_F32: y
template <int OT>
__device__ __forceinline__ typename PcmOut<OT>::type pcm_convert(float y, float scale) {
    if constexpr (OT == WSAE_DT_I16) return (int16_t)(int)fminf(fmaxf(rintf(y * scale), -32768.0f), 32767.0f);
    else return y;
}

// A tile of mlen <= TILE cells that goes to po: cell j is staged at s_y[j + shift] (s_y: 64-byte aligned, TILE + 64 /
// sizeof(T) cells), so that the cell on po's first 64-byte boundary sits at s_y[0] or s_y[64 / sizeof(T)].
template <class T, int TILE, int BLOCK>
struct PcmTileStore {
    static constexpr int VE = 16 / (int)sizeof(T), PIECE = 64 / (int)sizeof(T), PER = (TILE / VE + BLOCK - 1) / BLOCK;
    static_assert(TILE % PIECE == 0, "a tile is a whole number of 64-byte pieces");
    T* po;
    int mlen, lead, shift;

    __device__ __forceinline__ PcmTileStore(T* po_, int mlen_) : po(po_), mlen(mlen_) {
        lead = min((int)(((64 - ((uintptr_t)po & 63)) & 63) / sizeof(T)), mlen);  // the cells in front of that boundary
        shift = (PIECE - lead) % PIECE;
    }

    // after the barrier behind the staging
    __device__ __forceinline__ void store(const T* s_y) const {
        const int tid = threadIdx.x;
        if (tid < lead) po[tid] = s_y[tid + shift];
        const int nvec = (mlen - lead) / VE, whole = nvec & ~3;  // whole: the vectors that make up whole 64-byte pieces
        const float4* sv = (const float4*)(s_y + lead + shift);
        T* pb = po + lead;
        const __amdgpu_buffer_rsrc_t rs = wt_rsrc(pb);  // (based at the tile: the 32-bit offsets below stay under 16 KB)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int v = tid + k * BLOCK;
            if (v < whole) wt_store4(rs, (int64_t)v * 16, sv[v]);
            else if (v < nvec) *(float4*)(pb + v * VE) = sv[v];
        }
        const int done = lead + nvec * VE;
        if (done + tid < mlen) po[done + tid] = s_y[done + tid + shift];
    }
};

#endif  // __HIPCC__
