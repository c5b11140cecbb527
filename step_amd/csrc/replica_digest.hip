// Replica check of data-parallel training (include/step_hip.h, "replica digest"): a position-dependent 128-bit digest of a flat f32
// buffer, read once, so that the ranks of a data-parallel run can compare their parameter buffers with one 32-byte collective instead
// of moving the parameters.  It stands in for the guarantee DistributedDataParallel gives the reference (easytorch wraps the model when
// CFG.GPU_NUM > 1, step/STEP_PEMS04.py:30): the wrapper broadcasts rank 0's state once and every rank then applies the same reduced
// gradient.  Here nothing re-broadcasts, so the property is checked.
//
// Element i with bit pattern b (the 32 bits as stored: -0.0 differs from +0.0, a NaN keeps its payload) contributes
//     m = mix64(((uint64)i << 32) | b)
// with mix64 the finaliser of splitmix64:
//     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;
//     z ^= z >> 27;  z *= 0x94D049BB133111EB;
//     z ^= z >> 31;
// out2[0] = sum of all m mod 2^64, out2[1] = xor of all m.  Both reductions are commutative and exact: the words do not depend on the
// grid, on the order of the atomics or on the alignment split below.  mix64 is a bijection, so one changed bit changes m, hence both words.
//
// The body is read as 16-byte vectors from the first 16-byte aligned element on; the up to three elements in front of it and the up to
// three behind the last whole vector are read one by one by the first workgroup.  Per thread: a grid-stride loop over the vectors;
// per wave: a shuffle reduction; per workgroup: four partial pairs through LDS, then ONE 64-bit atomicAdd and ONE atomicXor.
#include "common.h"

namespace {

constexpr int RD_THREADS = 256, RD_WAVES = RD_THREADS / 64, RD_MAX_BLOCKS = 1024;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ uint64_t term(uint32_t i, uint32_t bits) { return mix64(((uint64_t)i << 32) | bits); }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int lane_mask) {
    const uint32_t lo = __shfl_xor((uint32_t)v, lane_mask, 64), hi = __shfl_xor((uint32_t)(v >> 32), lane_mask, 64);
    return ((uint64_t)hi << 32) | lo;
}

// bits: the buffer as 32-bit words; head: scalar elements in front of the first aligned vector; nvec: whole vectors; n: all elements
__global__ __launch_bounds__(RD_THREADS) void replica_digest_kernel(const uint32_t* __restrict__ bits, uint32_t head, uint32_t nvec,
                                                                   uint32_t n, unsigned long long* __restrict__ out2) {
    __shared__ uint64_t red[RD_WAVES][2];
    uint64_t s = 0, x = 0;
    const u32x4* body = reinterpret_cast<const u32x4*>(bits + head);
    const uint32_t stride = gridDim.x * RD_THREADS;
    for (uint64_t v = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x; v < nvec; v += stride) {      // (64-bit: v + stride may pass 2^32)
        const u32x4 w = body[v];
        const uint32_t i0 = head + 4u * (uint32_t)v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t m = term(i0 + c, w[c]);
            s += m; x ^= m;
        }
    }
    if (blockIdx.x == 0) {
        const uint32_t t = threadIdx.x, tail0 = head + 4u * nvec;
        if (t < head) { const uint64_t m = term(t, bits[t]); s += m; x ^= m; }
        // (64-bit comparison: no wrap-around next to 2^32)
        if (t >= 64 && (uint64_t)tail0 + (t - 64) < n) { const uint64_t m = term(tail0 + (t - 64), bits[tail0 + (t - 64)]); s += m; x ^= m; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += shfl_xor64(s, o); x ^= shfl_xor64(x, o); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = s; red[wave][1] = x; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < RD_WAVES; ++w) { s += red[w][0]; x ^= red[w][1]; }
        atomicAdd(out2, (unsigned long long)s);
        atomicXor(out2 + 1, (unsigned long long)x);
    }
}

}  // namespace

extern "C" int step_replica_digest(const float* flat, long n, unsigned long long* out2, void* stream) {
    STEP_REQUIRE(flat && out2, "replica_digest: NULL buffer");
    STEP_REQUIRE(n > 0 && n < (1L << 32), "replica_digest: need 0 < n < 2^32 elements (n = %ld): the element index is 32 bits of the hashed word", n);
    STEP_REQUIRE(((uintptr_t)flat & 3) == 0 && ((uintptr_t)out2 & 7) == 0, "replica_digest: flat must be 4-byte and out2 8-byte aligned");
    long head = (long)(((16 - ((uintptr_t)flat & 15)) & 15) >> 2);
    if (head > n) head = n;
    const long nvec = (n - head) / 4;
    hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(unsigned long long), (hipStream_t)stream);
    if (e != hipSuccess) {
        step_set_error("replica_digest: clearing the output failed: %s", hipGetErrorString(e));
        return STEP_ERR_HIP;
    }
    // four vectors (64 bytes) per thread where there are that many, at most RD_MAX_BLOCKS workgroups = that many atomics per word
    int blocks = cdiv(nvec, 4 * RD_THREADS);
    blocks = blocks < 1 ? 1 : (blocks > RD_MAX_BLOCKS ? RD_MAX_BLOCKS : blocks);
    replica_digest_kernel<<<blocks, RD_THREADS, 0, (hipStream_t)stream>>>(reinterpret_cast<const uint32_t*>(flat), (uint32_t)head,
                                                                          (uint32_t)nvec, (uint32_t)n, out2);
    STEP_LAUNCH_CHECK("replica_digest");
    return STEP_OK;
}
