// The output side the audio kernels share (wsae_clips.hip, wsae_resample.hip): the float32 -> PCM conversion and the store of
// a tile of outputs that sits in LDS to a destination of arbitrary alignment (DESIGN.md sections 30 and 31).
//
// The tile's cells are staged in LDS shifted by the cells that lead up to the destination's first 64-byte boundary, so that
// from that boundary on a lane stores 16 aligned bytes and a wave instruction whole 64-byte pieces: those go write-through
// (DESIGN.md 4.1), the at most three vectors behind the last whole piece plain, the ragged ends elementwise.  The same
// values whatever the alignment.
#pragma once

#include "wsae_common.h"

#ifdef __HIPCC__

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
