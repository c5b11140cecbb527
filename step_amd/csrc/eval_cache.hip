// Evaluation cache of the frozen branch (include/step_hip.h, "evaluation cache"): what a forward reads of the TSFormer + kNN prior
// of one window -- the last patch's hidden state [N, 96] f32 and the prior graph [N, N] in {0, 1} -- is kept in HBM, the graph as
// one bit per edge, and handed back on later passes over the same windows.  Two streaming kernels, one launch each.
#include "common.h"

namespace {

constexpr int EC_THREADS = 256;          // four waves per workgroup
constexpr int EC_WAVES = EC_THREADS / 64;

struct CacheArgs {
    float* last;              // [B][N][96]   (store: read, load: written)
    float* adj;               // [B][N][N]    (store: read, load: written)
    const long* slot;         // [B] device
    float* cache_last;        // [capacity][N][96]
    uint32_t* cache_bits;     // [capacity][N][W]
    int N, W, chunks;         // W = ceil(N / 32) words per row, chunks = ceil(N / 64) waves per row
    long pack_waves;          // N * chunks
    int pack_blocks;          // workgroups of the bit part; the ones behind them copy the rows
    long row_vec4;            // N * 24 16-byte pieces of one window's [N, 96] rows
};

// grid (pack_blocks + copy_blocks, B).  Bit part: one wave per 64 consecutive columns of one row; the wave's 64-bit ballot is two
// words of the row, written by lanes 0 and 1 with ordinary vector stores (store) -- or read back by the two half-waves (load).
// Columns >= N vote 0, so the tail bits of a row's last word are 0.  Row part: 16-byte copies of the flat [N * 96] block (a window's
// block starts at a multiple of 384 bytes; the [N, N] rows are NOT 16-byte aligned for odd N and are moved 4 bytes per lane).
template <bool STORE>
__global__ __launch_bounds__(EC_THREADS) void frozen_cache_kernel(CacheArgs a) {
    const int b = blockIdx.y;
    const long s = a.slot[b];
    if (s < 0) return;                   // this sample is not moved (uniform over the workgroup)
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x < a.pack_blocks) {
        const long w = (long)blockIdx.x * EC_WAVES + (threadIdx.x >> 6);
        if (w >= a.pack_waves) return;   // uniform over the wave: every lane of a voting wave is active
        const int row = (int)(w / a.chunks), c = (int)(w % a.chunks);
        const int col = c * 64 + lane;
        float* src = a.adj + ((long)b * a.N + row) * a.N;
        uint32_t* words = a.cache_bits + ((long)s * a.N + row) * a.W;
        if (STORE) {
            const bool on = col < a.N && src[col] != 0.f;
            const unsigned long long m = __ballot(on);
            const int word = 2 * c + lane;
            if (lane < 2 && word < a.W) words[word] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
        } else if (col < a.N) {
            const uint32_t v = words[2 * c + (lane >> 5)];
            src[col] = ((v >> (lane & 31)) & 1u) ? 1.0f : 0.0f;
        }
        return;
    }
    const long i = (long)((int)blockIdx.x - a.pack_blocks) * EC_THREADS + threadIdx.x;
    if (i >= a.row_vec4) return;
    f32x4* mine = reinterpret_cast<f32x4*>(a.last) + (long)b * a.row_vec4 + i;
    f32x4* kept = reinterpret_cast<f32x4*>(a.cache_last) + s * a.row_vec4 + i;
    if (STORE) *kept = *mine; else *mine = *kept;
}

template <bool STORE>
int launch(const char* what, float* last, float* adj, int B, int N, const long* slot, long capacity, float* cache_last,
           uint32_t* cache_bits, void* stream) {
    STEP_REQUIRE(last && adj && slot && cache_last && cache_bits && B > 0 && N > 0 && capacity > 0,
                 "%s: bad arguments (NULL buffer, or B = %d, N = %d, capacity = %ld not all positive)", what, B, N, capacity);
    STEP_REQUIRE(B <= 65535, "%s: B = %d exceeds the 65535 samples of one launch", what, B);
    STEP_REQUIRE(((uintptr_t)last & 15) == 0 && ((uintptr_t)cache_last & 15) == 0, "%s: last / cache_last must be 16-byte aligned", what);
    CacheArgs a;
    a.last = last; a.adj = adj; a.slot = slot; a.cache_last = cache_last; a.cache_bits = cache_bits;
    a.N = N; a.W = (N + 31) / 32; a.chunks = (N + 63) / 64;
    a.pack_waves = (long)N * a.chunks;
    a.pack_blocks = cdiv(a.pack_waves, EC_WAVES);
    a.row_vec4 = (long)N * 24;
    const int copy_blocks = cdiv(a.row_vec4, EC_THREADS);
    frozen_cache_kernel<STORE><<<dim3(a.pack_blocks + copy_blocks, B), EC_THREADS, 0, (hipStream_t)stream>>>(a);
    STEP_LAUNCH_CHECK(what);
    return STEP_OK;
}

}  // namespace

extern "C" int step_frozen_cache_store(const float* last, const float* adj, int B, int N, const long* slot, long capacity,
                                       float* cache_last, uint32_t* cache_bits, void* stream) {
    return launch<true>("frozen_cache_store", const_cast<float*>(last), const_cast<float*>(adj), B, N, slot, capacity, cache_last,
                        cache_bits, stream);
}

extern "C" int step_frozen_cache_load(const float* cache_last, const uint32_t* cache_bits, long capacity, const long* slot, int B, int N,
                                      float* last, float* adj, void* stream) {
    return launch<false>("frozen_cache_load", last, adj, B, N, slot, capacity, const_cast<float*>(cache_last),
                         const_cast<uint32_t*>(cache_bits), stream);
}
