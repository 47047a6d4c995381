// Resampling: interleaved multi-channel waveforms at any rate in, mono waveforms at the new rate
// out - downmix, polyphase FIR, lengths and the PCM conversion as one kernel on the caller's stream.  The contract,
// operation by operation, is in include/wsae.h; tests/resample_oracle.py restates it.
//
// resample_kernel: a workgroup of 256 threads owns `tile` (WSAE_RESAMPLE_TILE = 1024, fewer where the span would not fit)
// consecutive outputs j0 .. of one utterance, which belong to the blocks i0 = j0 / new_ .. (a block: orig input frames in,
// new_ outputs out).
//   Staging.  The frames [i0 orig - halo, i_end orig + halo) go to LDS once as float32 mono: the int16 scaling and the
//   downmix happen here, zeros stand outside [0, L_u).  Mono and stereo rows whose frames fall on 16-byte boundaries are
//   read 16 bytes per lane from the first such boundary on, four loads in flight per thread, the ends by element; every
//   other channel count or alignment by element (LOAD_ANY).  The LDS writes are scalar and conflict like those of
//   wsae_clips.hip: a few hundred cycles a tile.
//   Taps.  The table goes to LDS transposed, [n_taps][new_ | 1]: lanes on consecutive phases read consecutive words, and
//   the odd row stride keeps the transposing writes off one bank (TAPS_LDS).  new_ == 1 has one phase, so one broadcast
//   read serves the four chains of a thread (TAPS_ONE).  A table that does not fit beside the span is read in place
//   through the cache (TAPS_GLOBAL).
//   FIR.  Thread tid owns the outputs j0 + tid + 256 r, r = 0 .. 3, and runs their four chains side by side through one
//   loop over the taps: four independent LDS reads and fmaf's per step hide the LDS latency that one chain alone would
//   wait out at every tap.  Each y[j] is ONE chain over w = 0 .. n_taps - 1 whatever the tile, the thread or the route.
//   Neighbouring lanes read words orig / new_ apart; the conflicts per ratio are counted in DESIGN.md.
//   Store.  The converted outputs are staged in LDS and leave through PcmTileStore (wsae_pcm.h), zeros from out_len[u] to
//   out_cols included.
#include <math.h>

#include "wsae_common.h"
#include "wsae_pcm.h"

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_TILE = WSAE_RESAMPLE_TILE;
constexpr int RS_PER = RS_TILE / RS_BLOCK;  // chains per thread
constexpr int RS_YBYTES = (RS_TILE + 16) * 4;  // the output stage: a tile and one 64-byte piece, float32 or int16
enum { LOAD_ANY = 0, LOAD_VEC1 = 1, LOAD_VEC2 = 2 };    // LOAD_VECc: c channels, 16-byte loads where the row allows
enum { TAPS_LDS = 0, TAPS_ONE = 1, TAPS_GLOBAL = 2 };
static_assert(RS_TILE % RS_BLOCK == 0, "a tile is a whole number of outputs per thread");
static_assert(RS_YBYTES % 16 == 0, "the span behind the output stage is 16-byte aligned");

struct ResampleArgs {
    const void* x;
    int64_t ld_x;
    const int32_t* length;
    int32_t max_length, channels;
    int32_t orig, new_, n_taps, halo;
    const float* taps;
    const int32_t* first;
    void* out;
    int64_t ld_y;
    int32_t out_cols;
    int32_t* out_len;
    int32_t tile, tiles, span;  // span: floats of LDS behind the staged frames of a tile
};

// frame m of a row: the channels summed in their order, then one IEEE division
template <int DT>
__device__ __forceinline__ float mono_frame(const void* row, int64_t m, int C) {
    float s = pcm_load<DT>(row, m * C);
    if (C == 1) return s;
    for (int c = 1; c < C; ++c) s = s + pcm_load<DT>(row, m * C + c);
    return s / (float)C;
}

// s_x[k] = mono[m_lo + k] for k in [0, span): zeros outside [0, len).  row: element 0 of the utterance.
template <int DT, int LOAD>
__device__ __forceinline__ void stage_span(const void* row, int64_t m_lo, int span, int len, int C, float* s_x) {
    const int tid = threadIdx.x;
    const int ka = (int)min64(max(-m_lo, (int64_t)0), span);          // [ka, kb): the cells with a frame behind them
    const int kb = (int)min64(max((int64_t)len - m_lo, (int64_t)ka), span);
    for (int k = tid; k < ka; k += RS_BLOCK) s_x[k] = 0.f;
    for (int k = kb + tid; k < span; k += RS_BLOCK) s_x[k] = 0.f;
    const int n = kb - ka;
    if (n <= 0) return;
    const int64_t ma = m_lo + ka;
    if constexpr (LOAD == LOAD_ANY) {
        for (int k = tid; k < n; k += RS_BLOCK) s_x[ka + k] = mono_frame<DT>(row, ma + k, C);
    } else {
        // (the host chose this route: the row's frames meet the 16-byte boundaries)
        constexpr int CH = LOAD == LOAD_VEC2 ? 2 : 1;
        float* sv = s_x + ka;
        pcm_for_span<DT, CH, RS_BLOCK, 4>((const typename PcmIn<DT>::elem*)row + ma * CH, n, [&](int k, float s) { sv[k] = s; });
    }
}

template <int DT, int LOAD, int OT, int TAPS>
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(ResampleArgs a) {
    typedef typename PcmOut<OT>::type T;
    typedef PcmTileStore<T, RS_TILE, RS_BLOCK> Store;
    extern __shared__ __attribute__((aligned(64))) char s_mem[];
    T* s_y = (T*)s_mem;
    float* s_x = (float*)(s_mem + RS_YBYTES);
    float* s_t = s_x + a.span;
    const int u = blockIdx.x / a.tiles, t = blockIdx.x % a.tiles, tid = threadIdx.x;
    const int orig = a.orig, new_ = a.new_, n_taps = a.n_taps, halo = a.halo;
    const int ts = new_ | 1;  // words between two taps of a phase in LDS: odd, so that the banks differ along w as along p
    const int len = min(max(a.length[u], 0), a.max_length);
    const int olen = (int)(((int64_t)new_ * len + orig - 1) / orig);  // (at most out_cols: the host checked max_length)
    if (t == 0 && tid == 0) a.out_len[u] = olen;
    const int j0 = t * a.tile;  // (tiles * tile < 2^31 + tile: the host checked)
    const int mlen = min(a.tile, a.out_cols - j0);  // cells this workgroup writes
    if (mlen <= 0) return;                          // (out_cols == 0: the one workgroup that reports the length)
    const int nval = min(mlen, olen - j0);          // of which carry a value; the rest are zeros
    const Store st((T*)a.out + (int64_t)u * a.ld_y + j0, mlen);

    float acc[RS_PER];
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) acc[r] = 0.f;
    if (nval > 0) {
        const int i0 = j0 / new_, i_end = (int)(((int64_t)j0 + nval + new_ - 1) / new_);
        const int span = (i_end - i0) * orig + 2 * halo;  // (at most a.span: the host sized it for any j0)
        const char* row = (const char*)a.x + (int64_t)u * a.ld_x * (DT == WSAE_DT_I16 ? 2 : 4);
        stage_span<DT, LOAD>(row, (int64_t)i0 * orig - halo, span, len, a.channels, s_x);
        if constexpr (TAPS != TAPS_GLOBAL) {
            for (int e = tid; e < n_taps * new_; e += RS_BLOCK) {  // (coalesced read; the odd stride spreads the transposing write)
                const int p = e / n_taps, w = e - p * n_taps;
                s_t[w * ts + p] = a.taps[e];
            }
        }
        __syncthreads();
        int kx[RS_PER], kt[RS_PER];  // where a chain's first sample and first tap are; a chain without a cell runs chain 0's
#pragma unroll
        for (int r = 0; r < RS_PER; ++r) {
            const int jl = tid + r * RS_BLOCK, j = j0 + (jl < nval ? jl : 0);
            const int i = j / new_, p = j - i * new_;
            const int f = min(max(a.first[p], -halo), orig + halo - n_taps);  // a broken promise stays inside the span
            kx[r] = (i - i0) * orig + f + halo;
            kt[r] = TAPS == TAPS_GLOBAL ? p * n_taps : TAPS == TAPS_ONE ? 0 : p;
        }
        auto tap = [&](int r, int w) -> float {
            if constexpr (TAPS == TAPS_GLOBAL) return a.taps[kt[r] + w];
            else if constexpr (TAPS == TAPS_ONE) return s_t[w];
            else return s_t[kt[r] + w * ts];
        };
        for (int w = 0; w < n_taps; ++w) {
#pragma unroll
            for (int r = 0; r < RS_PER; ++r) acc[r] = __builtin_fmaf(s_x[kx[r] + w], tap(r, w), acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
        const int jl = tid + r * RS_BLOCK;
        if (jl < mlen) s_y[jl + st.shift] = pcm_convert<OT>(jl < nval ? acc[r] : 0.f, 32768.0f);
    }
    __syncthreads();
    st.store(s_y);
}

// the most blocks a run of `tile` outputs touches, whatever its first output
inline int64_t blocks_of(int64_t tile, int64_t new_) { return tile % new_ == 0 ? tile / new_ : (tile + 2 * new_ - 2) / new_; }

template <int DT, int LOAD, int OT>
void launch_taps(int taps, unsigned grid, size_t lds, hipStream_t st, const ResampleArgs& a) {
    if (taps == TAPS_LDS) resample_kernel<DT, LOAD, OT, TAPS_LDS><<<grid, RS_BLOCK, lds, st>>>(a);
    else if (taps == TAPS_ONE) resample_kernel<DT, LOAD, OT, TAPS_ONE><<<grid, RS_BLOCK, lds, st>>>(a);
    else resample_kernel<DT, LOAD, OT, TAPS_GLOBAL><<<grid, RS_BLOCK, lds, st>>>(a);
}

template <int DT, int LOAD>
void launch_out(int out_dtype, int taps, unsigned grid, size_t lds, hipStream_t st, const ResampleArgs& a) {
    if (out_dtype == WSAE_DT_I16) launch_taps<DT, LOAD, WSAE_DT_I16>(taps, grid, lds, st, a);
    else launch_taps<DT, LOAD, WSAE_DT_F32>(taps, grid, lds, st, a);
}

template <int DT>
void launch_load(int load, int out_dtype, int taps, unsigned grid, size_t lds, hipStream_t st, const ResampleArgs& a) {
    if (load == LOAD_VEC1) launch_out<DT, LOAD_VEC1>(out_dtype, taps, grid, lds, st, a);
    else if (load == LOAD_VEC2) launch_out<DT, LOAD_VEC2>(out_dtype, taps, grid, lds, st, a);
    else launch_out<DT, LOAD_ANY>(out_dtype, taps, grid, lds, st, a);
}

int gcd_of(int a, int b) {
    while (b) { const int r = a % b; a = b; b = r; }
    return a;
}

}  // namespace

extern "C" int wsae_resample(const void* x, int32_t x_dtype, int32_t n_utt, int64_t ld_x, int32_t channels, const int32_t* length,
                             int64_t max_length, int32_t orig, int32_t new_, const float* taps, const int32_t* first,
                             int32_t n_taps, int32_t halo, void* out, int32_t out_dtype, int64_t ld_y, int64_t out_cols,
                             int32_t* out_len, void* stream) {
    WSAE_REQUIRE(x && length && taps && first && out && out_len, "wsae_resample: null pointer");
    PCM_REQUIRE_DTYPE("wsae_resample", x_dtype);
    PCM_REQUIRE_DTYPE("wsae_resample", out_dtype);
    PCM_REQUIRE_N_UTT("wsae_resample", n_utt);
    WSAE_REQUIRE(channels >= 1 && channels <= WSAE_RESAMPLE_MAX_CHANNELS, "wsae_resample: need 1 <= channels <= %d (got %d)",
                 WSAE_RESAMPLE_MAX_CHANNELS, channels);
    WSAE_REQUIRE(orig >= 1 && orig <= WSAE_RESAMPLE_MAX_RATE, "wsae_resample: need 1 <= orig <= %d (got %d)", WSAE_RESAMPLE_MAX_RATE, orig);
    WSAE_REQUIRE(new_ >= 1 && new_ <= WSAE_RESAMPLE_MAX_RATE, "wsae_resample: need 1 <= new_ <= %d (got %d)", WSAE_RESAMPLE_MAX_RATE, new_);
    WSAE_REQUIRE(gcd_of(orig, new_) == 1, "wsae_resample: orig %d and new_ %d must be coprime (divide both by %d)", orig, new_,
                 gcd_of(orig, new_));
    WSAE_REQUIRE(n_taps >= 1 && n_taps <= WSAE_RESAMPLE_MAX_TAPS, "wsae_resample: need 1 <= n_taps <= %d (got %d)",
                 WSAE_RESAMPLE_MAX_TAPS, n_taps);
    WSAE_REQUIRE(halo >= 0 && halo <= WSAE_RESAMPLE_MAX_HALO, "wsae_resample: need 0 <= halo <= %d (got %d)", WSAE_RESAMPLE_MAX_HALO, halo);
    WSAE_REQUIRE(n_taps <= orig + 2 * halo, "wsae_resample: n_taps %d does not fit the staged span of a block, orig + 2 halo = %d",
                 n_taps, orig + 2 * halo);
    PCM_REQUIRE_MAX_LENGTH("wsae_resample", max_length);
    PCM_REQUIRE_LD_X("wsae_resample", ld_x, max_length * channels, "max_length * channels =");
    const int64_t need_cols = ceil_div64((int64_t)new_ * max_length, orig);
    WSAE_REQUIRE(out_cols >= need_cols && out_cols <= 0x7fffffffll,
                 "wsae_resample: need ceil(new_ * max_length / orig) = %lld <= out_cols < 2^31 (got %lld)", (long long)need_cols,
                 (long long)out_cols);
    WSAE_REQUIRE(out_cols <= ld_y, "wsae_resample: out_cols %lld is above ld_y %lld", (long long)out_cols, (long long)ld_y);
    PCM_REQUIRE_ELEMENTS_ALIGNED("wsae_resample", x, x_dtype, out, out_dtype);
    PCM_REQUIRE_TABLES_ALIGNED("wsae_resample", ptr_bits(length, taps, first, out_len), 0, "length, taps, first and out_len must be 4-byte aligned");

    // the route: the largest tile whose span fits beside the output stage, and the table beside that where it fits too
    int64_t tile = RS_TILE, span;
    for (;; tile /= 2) {
        span = blocks_of(tile, new_) * orig + 2 * halo;
        if (RS_YBYTES + 4 * span <= WSAE_RESAMPLE_LDS_BYTES || tile == 1) break;
    }
    WSAE_REQUIRE(RS_YBYTES + 4 * span <= WSAE_RESAMPLE_LDS_BYTES, "wsae_resample: one block of orig %d with halo %d does not fit %d bytes of LDS",
                 orig, halo, WSAE_RESAMPLE_LDS_BYTES);
    const int64_t table = (int64_t)n_taps * (new_ | 1);  // (rows of odd stride: the kernel's ts)
    const bool table_fits = RS_YBYTES + 4 * (span + table) <= WSAE_RESAMPLE_LDS_BYTES;
    const int route = !table_fits ? TAPS_GLOBAL : new_ == 1 ? TAPS_ONE : TAPS_LDS;
    const int64_t tiles = out_cols > tile ? ceil_div64(out_cols, tile) : 1;
    WSAE_REQUIRE((int64_t)n_utt * tiles <= 0x7fffffffll, "wsae_resample: n_utt * tiles of out_cols is too large for one launch");
    if (n_utt == 0) return WSAE_OK;

    // 16-byte loads: mono or stereo, and every row's frames meet the 16-byte boundaries
    const int fb = channels * (x_dtype == WSAE_DT_I16 ? 2 : 4);
    const bool vec = channels <= 2 && (uintptr_t)x % fb == 0 && (n_utt == 1 || (ld_x * (fb / channels)) % fb == 0);
    const int load = !vec ? LOAD_ANY : channels == 2 ? LOAD_VEC2 : LOAD_VEC1;

    ResampleArgs a;
    a.x = x; a.ld_x = ld_x; a.length = length; a.max_length = (int32_t)max_length; a.channels = channels;
    a.orig = orig; a.new_ = new_; a.n_taps = n_taps; a.halo = halo; a.taps = taps; a.first = first;
    a.out = out; a.ld_y = ld_y; a.out_cols = (int32_t)out_cols; a.out_len = out_len;
    a.tile = (int32_t)tile; a.tiles = (int32_t)tiles; a.span = (int32_t)span;
    const size_t lds = (size_t)(RS_YBYTES + 4 * (span + (table_fits ? table : 0)));
    const unsigned grid = (unsigned)(n_utt * tiles);
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == WSAE_DT_I16) launch_load<WSAE_DT_I16>(load, out_dtype, route, grid, lds, st, a);
    else launch_load<WSAE_DT_F32>(load, out_dtype, route, grid, lds, st, a);
    WSAE_LAUNCH_CHECK();
    return WSAE_OK;
}
