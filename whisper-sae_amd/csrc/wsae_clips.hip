// Audio clip export: cut n_clips ragged sample ranges out of a device-resident bank of waveforms, find
// each clip's peak, apply the gain and the linear fades, convert to float32 or 16-bit PCM and store every clip at its own
// offset of one output buffer - two kernels on the caller's stream.  The contract, operation by operation, is in
// include/wsae.h; tests/clip_oracle.py restates it.
//
// Both kernels run one workgroup of 256 threads per (clip, tile of WSAE_CLIP_TILE = 4096 samples), flattened into gridDim.x;
// a tile at or beyond the clip's n samples exits after the clip's bounds are resolved (a handful of scalar loads), which is
// what balances ragged event clips.
// clip_peak_kernel reduces |x| over its tile (DPP wave maximum, then LDS) into one workspace float per (clip, tile).
// clip_write_kernel reduces the clip's tile maxima (a float maximum: any order gives the same bits), reads its tile again
//   (from L2 / Infinity Cache: the peak kernel has just read it), computes the output values and stages them in LDS, then
//   stores them.  The staging is what decouples the two alignments: a clip starts at an arbitrary sample, so the source is
//   read as scalars up to the first 16-byte boundary, 16 bytes per lane from there, scalars behind the last whole vector
//   (for_tile); the output begins at an arbitrary clip_off, so the image sits in LDS shifted by the elements that lead up to
//   the output's first 64-byte boundary, and from that boundary on a lane stores 16 aligned bytes, a wave instruction whole
//   64-byte pieces: those go write-through, the at most three vectors behind the last whole piece plain,
//   the ragged ends elementwise (PcmTileStore, wsae_pcm.h: wsae_resample.hip stores the same way).  The same values
//   whatever the alignment.  The LDS writes of the staging are scalar (the
//   shift is arbitrary) and conflict 4- or 8-way; at 16 KB per tile that is a few hundred cycles against the thousands the
//   tile's bytes take at the memory rate.
// When neither the gain nor out_peak needs the peak (WSAE_CLIP_GAIN_NONE, out_peak null) the peak kernel is not launched.
#include <math.h>

#include "wsae_common.h"
#include "wsae_pcm.h"

// (x / m) * target * r is a division and two products, each rounded
#pragma clang fp contract(off)

namespace {

constexpr int CL_BLOCK = 256, CL_WAVES = CL_BLOCK / 64;
constexpr int CL_TILE = WSAE_CLIP_TILE;
constexpr int64_t CL_MAX_COUNT = 1ll << 30;  // tile offsets and n stay inside an int
static_assert(CL_TILE % (8 * CL_BLOCK) == 0, "a tile is a whole number of 16-byte vectors per thread, int16 and float32");

struct ClipArgs {
    const void* x;
    int64_t ld_x;
    const int32_t* length;
    int32_t n_utt, max_length;
    const int32_t* clip_utt;
    const int64_t* clip_start;
    const int32_t* clip_count;
    const int64_t* clip_off;
    int32_t max_count, tiles;  // tiles: per clip in the grid and in the workspace (at least one)
    int32_t gain_mode, fade, need_peak;
    float target, scale;       // scale: float -> int16 (32767; 32768 for the plain int16 copy, which is then exact)
    void* out;
    int64_t out_elems;
    int32_t* out_len;
    float* out_peak;
    float* tile_max;
};

struct ClipSpan {
    int64_t src, off;  // first sample in x (elements), first cell in out
    int n;             // samples
    bool valid;
};

// every value here is workgroup-uniform: c comes from blockIdx
__device__ __forceinline__ ClipSpan clip_span(const ClipArgs& a, int c) {
    ClipSpan s;
    const int u = a.clip_utt[c];
    const int64_t s0 = a.clip_start[c] > 0 ? a.clip_start[c] : 0;
    const int cnt = min(max(a.clip_count[c], 0), a.max_count);
    const bool in = u >= 0 && u < a.n_utt;
    const int len = in ? min(max(a.length[u], 0), a.max_length) : 0;
    s.n = s0 < len ? (int)min64(cnt, len - s0) : 0;
    s.off = a.clip_off[c];
    s.valid = in && s.off >= 0 && s.off <= a.out_elems - s.n;
    s.src = (int64_t)u * a.ld_x + s0;
    return s;
}

// f(j, x_j) for every j in [0, m) exactly once, x_j = element first + j of x as float (pcm_for_span, wsae_pcm.h: nothing
// outside [first, first + m) is read).  m <= CL_TILE, so its batch of 16-byte loads is the only one.
template <int DT, class F>
__device__ __forceinline__ void for_tile(const void* x, int64_t first, int m, F&& f) {
    typedef PcmIn<DT> In;
    pcm_for_span<DT, 1, CL_BLOCK, CL_TILE / In::VE / CL_BLOCK>((const typename In::elem*)x + first, m, f);
}

template <int DT>
__global__ __launch_bounds__(CL_BLOCK) void clip_peak_kernel(ClipArgs a) {
    __shared__ float s_red[CL_WAVES];
    const int c = blockIdx.x / a.tiles, t = blockIdx.x % a.tiles, j0 = t * CL_TILE;
    const ClipSpan s = clip_span(a, c);
    if (!s.valid || j0 >= s.n) return;
    float mx = 0.f;
    for_tile<DT>(a.x, s.src + j0, min(CL_TILE, s.n - j0), [&](int, float x) { mx = fmaxf(mx, fabsf(x)); });
    mx = block_max(mx, s_red);
    if (threadIdx.x == 0) a.tile_max[(int64_t)c * a.tiles + t] = mx;
}

template <int DT, int OT>
__global__ __launch_bounds__(CL_BLOCK) void clip_write_kernel(ClipArgs a) {
    typedef typename PcmOut<OT>::type T;
    typedef PcmTileStore<T, CL_TILE, CL_BLOCK> Store;
    __shared__ __attribute__((aligned(64))) T s_y[CL_TILE + Store::PIECE];
    __shared__ float s_red[CL_WAVES];
    const int c = blockIdx.x / a.tiles, t = blockIdx.x % a.tiles, j0 = t * CL_TILE, tid = threadIdx.x;
    const ClipSpan s = clip_span(a, c);
    const int tiles = s.valid ? (s.n + CL_TILE - 1) / CL_TILE : 0;
    if (t != 0 && t >= tiles) return;
    float m = 0.f;
    if (a.need_peak) {
        for (int i = tid; i < tiles; i += CL_BLOCK) m = fmaxf(m, a.tile_max[(int64_t)c * a.tiles + i]);
        m = block_max(m, s_red);
    }
    if (t == 0 && tid == 0) {  // the clip's first workgroup reports, also where the clip is empty or invalid
        a.out_len[c] = s.valid ? s.n : -1;
        if (a.out_peak) a.out_peak[c] = m;
    }
    if (t >= tiles) return;

    const int mlen = min(CL_TILE, s.n - j0);
    const Store st((T*)a.out + s.off + j0, mlen);  // (wsae_pcm.h: cell j of the tile sits at s_y[j + shift])
    const int shift = st.shift;
    const bool gain = a.gain_mode == WSAE_CLIP_GAIN_PEAK && m > 0.f;
    const float target = a.target, scale = a.scale, flen = (float)a.fade;
    const int fade = a.fade, last = s.n - 1;
    for_tile<DT>(a.x, s.src + j0, mlen, [&](int jl, float x) {
        float y = gain ? (x / m) * target : x;
        if (fade > 0) {
            const int j = j0 + jl;
            y = y * ((float)min(min(j, last - j) + 1, fade) / flen);
        }
        s_y[jl + shift] = pcm_convert<OT>(y, scale);
    });
    __syncthreads();

    st.store(s_y);
}

inline int64_t clip_tiles(int64_t max_count) { return max_count > CL_TILE ? ceil_div64(max_count, CL_TILE) : 1; }

template <int DT>
void launch_write(int out_dtype, unsigned grid, hipStream_t st, const ClipArgs& a) {
    if (out_dtype == WSAE_DT_I16) clip_write_kernel<DT, WSAE_DT_I16><<<grid, CL_BLOCK, 0, st>>>(a);
    else clip_write_kernel<DT, WSAE_DT_F32><<<grid, CL_BLOCK, 0, st>>>(a);
}

}  // namespace

extern "C" int64_t wsae_clip_workspace_bytes(int32_t n_clips, int64_t max_count) {
    if (n_clips < 0 || max_count < 0 || max_count > CL_MAX_COUNT) return -1;
    return align256((int64_t)sizeof(float) * n_clips * clip_tiles(max_count));
}

extern "C" int wsae_clip_extract(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, const int32_t* length,
                                 int64_t max_length, int32_t n_clips, const int32_t* clip_utt, const int64_t* clip_start,
                                 const int32_t* clip_count, int64_t max_count, const int64_t* clip_off, int32_t gain_mode,
                                 float target, int32_t fade, void* out, int32_t out_dtype, int64_t out_elems, int32_t* out_len,
                                 float* out_peak, void* workspace, int64_t workspace_bytes, void* stream) {
    WSAE_REQUIRE(x && length && clip_utt && clip_start && clip_count && clip_off && out && out_len, "wsae_clip_extract: null pointer");
    PCM_REQUIRE_DTYPE("wsae_clip_extract", x_dtype);
    PCM_REQUIRE_DTYPE("wsae_clip_extract", out_dtype);
    PCM_REQUIRE_N_UTT("wsae_clip_extract", n_utt);
    WSAE_REQUIRE(n_clips >= 0, "wsae_clip_extract: n_clips must not be negative (got %d)", n_clips);
    WSAE_REQUIRE(max_count >= 0 && max_count <= CL_MAX_COUNT, "wsae_clip_extract: need 0 <= max_count <= %lld (got %lld)",
                 (long long)CL_MAX_COUNT, (long long)max_count);
    PCM_REQUIRE_MAX_LENGTH("wsae_clip_extract", max_length);
    PCM_REQUIRE_LD_X("wsae_clip_extract", ld_x, max_length, "max_length");
    WSAE_REQUIRE(out_elems >= 0, "wsae_clip_extract: out_elems must not be negative (got %lld)", (long long)out_elems);
    WSAE_REQUIRE(gain_mode == WSAE_CLIP_GAIN_NONE || gain_mode == WSAE_CLIP_GAIN_PEAK, "wsae_clip_extract: unknown gain_mode %d",
                 gain_mode);
    WSAE_REQUIRE(isfinite(target), "wsae_clip_extract: target must be finite");
    WSAE_REQUIRE(fade >= 0, "wsae_clip_extract: fade must not be negative (got %d)", fade);
    PCM_REQUIRE_ELEMENTS_ALIGNED("wsae_clip_extract", x, x_dtype, out, out_dtype);
    PCM_REQUIRE_TABLES_ALIGNED("wsae_clip_extract", ptr_bits(length, clip_utt, clip_count, out_len, out_peak), ptr_bits(clip_start, clip_off),
                               "the int32 / float tables must be 4-byte aligned, clip_start and clip_off 8-byte");
    const int64_t need = wsae_clip_workspace_bytes(n_clips, max_count);
    WSAE_REQUIRE_WORKSPACE("wsae_clip_extract", workspace, workspace_bytes, need, n_clips);
    WSAE_REQUIRE_WORKSPACE_ALIGNED("wsae_clip_extract", workspace, 4);
    const int64_t tiles = clip_tiles(max_count);
    WSAE_REQUIRE((int64_t)n_clips * tiles <= 0x7fffffffll, "wsae_clip_extract: n_clips * tiles of max_count is too large for one launch");
    if (n_clips == 0) return WSAE_OK;
    hipStream_t st = (hipStream_t)stream;
    ClipArgs a;
    a.x = x; a.ld_x = ld_x; a.length = length; a.n_utt = n_utt; a.max_length = (int32_t)max_length;
    a.clip_utt = clip_utt; a.clip_start = clip_start; a.clip_count = clip_count; a.clip_off = clip_off;
    a.max_count = (int32_t)max_count; a.tiles = (int32_t)tiles;
    a.gain_mode = gain_mode; a.fade = fade; a.need_peak = gain_mode == WSAE_CLIP_GAIN_PEAK || out_peak != nullptr;
    a.target = target;
    a.scale = gain_mode == WSAE_CLIP_GAIN_NONE && fade == 0 && x_dtype == WSAE_DT_I16 ? 32768.0f : 32767.0f;
    a.out = out; a.out_elems = out_elems; a.out_len = out_len; a.out_peak = out_peak; a.tile_max = (float*)workspace;
    const unsigned grid = (unsigned)(n_clips * tiles);
    if (a.need_peak) {
        if (x_dtype == WSAE_DT_I16) clip_peak_kernel<WSAE_DT_I16><<<grid, CL_BLOCK, 0, st>>>(a);
        else clip_peak_kernel<WSAE_DT_F32><<<grid, CL_BLOCK, 0, st>>>(a);
        WSAE_LAUNCH_CHECK();
    }
    if (x_dtype == WSAE_DT_I16) launch_write<WSAE_DT_I16>(out_dtype, grid, st, a);
    else launch_write<WSAE_DT_F32>(out_dtype, grid, st, a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
