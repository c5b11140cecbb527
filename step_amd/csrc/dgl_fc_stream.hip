// Streaming kernels for the three fc products of the graph learner, which all have one short side (100 outputs) over a2h, the
// channels-last bf16 conv2 activation [N][16 (T - 18)] (133 MB at PEMS04):
//   forward          gpre[N][100]  += a2h[N][K] . wp[100][K]^T
//   weight gradient  G[100][K]      = bf16(dgpre)^T[100][N] . a2h[N][K]
//   input gradient   dz2h[N][K]     = BatchNorm2 backward and ReLU mask (x = a2h) of bf16(dgpre)[N][100] . wp[100][K]
// The staged GEMM keeps one k step of loads in flight per workgroup and re-reads the short operand per 128-row tile; both products ran at a
// third of the memory system's rate.  Here a2h goes global -> LDS by DMA (lds_dma.h) through a ring of stages: a workgroup keeps two (forward)
// or three (weight gradient) stages of loads in flight while it multiplies another, waits with a counted s_waitcnt vmcnt(n) and a raw
// s_barrier (a __syncthreads() would drain the ring: it waits for vmcnt(0)), and reads every byte of a2h once.
// STEP_DGL_FC_STREAM=0 (dgl.hip) keeps the staged GEMM; measurements in profiles/dgl_fc_stream_{before,after}.md and
// profiles/dgl_fc_dgrad_{before,after}.md.
#include "common.h"
#include "step_internal.h"
#include "lds_dma.h"
#include <stdlib.h>

namespace {

template <int N>
__device__ __forceinline__ void fs_wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if constexpr (N == 40) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
    else if constexpr (N == 53) asm volatile("s_waitcnt vmcnt(53)" ::: "memory");
    else static_assert(N == 0, "add the case");
}
__device__ __forceinline__ void fs_barrier() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Forward.  One workgroup of 10 waves owns ALL rows of a row tile (FS_TM = 320: PEMS04's 307 nodes are one tile) and all outputs for a
// contiguous range of k steps: wp is read once per row tile, not once per 128 rows.  A stage is one k step of FS_KS = 64 bf16 (128 bytes
// per row) of the 320 a2h rows and of the 100 (104 staged) wp rows: 53 DMA instructions of 1 KB (8 rows), 5 or 6 per wave, two stages
// ahead of the matrix work (FS_RING = 3 stages of 54,272 bytes = 159 KB of LDS, 106 KB in flight).  A row's 8 pieces of 16 bytes are stored
// XOR-swizzled (piece c of row r in slot c ^ (r & 7)) through the lanes' SOURCE addresses, and read through the same XOR: the 16-byte
// fragment reads of 8 consecutive rows hit all banks.  Wave w multiplies rows 64 (w % 5) .. + 63 by outputs 64 (w / 5) .. + 63 (2 x 2 tiles of
// 32 x 32, four fragment reads for four products).  Rows past N repeat row N - 1 and outputs past O repeat row O - 1 of wp: they only
// feed results that are never stored.  K is a multiple of 16 (one time step), so the last k step holds 1 .. 4 whole 16-wide products; the
// pieces past K are loaded from the row's first piece of the step and never multiplied.
// The partial tile of a k range goes to the split-K workspace [range][N][O] (summed by fc_stream_reduce_kernel), or -- one range, no
// workspace -- straight into gpre with atomics.
constexpr int FS_TM = 320, FS_KS = 64, FS_ROWB = FS_KS * 2, FS_WROWS = 104, FS_RING = 3, FS_WAVES = 10;
constexpr int FS_STAGE = (FS_TM + FS_WROWS) * FS_ROWB;
static_assert(FS_RING * FS_STAGE <= 160 * 1024, "forward ring");
static_assert(FS_TM / 8 == 4 * FS_WAVES, "four a2h row groups per wave");

__global__ __launch_bounds__(FS_WAVES * 64) void fc_stream_fwd_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ W, int N, int O,
                                                                       long K, int per, float* __restrict__ out, long range_stride, int atomic) {
    extern __shared__ __attribute__((aligned(16))) char fs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = blockIdx.x, row0 = blockIdx.y * FS_TM;
    const int ksteps = (int)((K + FS_KS - 1) / FS_KS);
    const int step0 = s * per;
    const int nstep = min(ksteps - step0, per);
    const int rp = wave % 5, cp = wave / 5;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)fs_lds;
    // this wave's DMA instructions of a stage: a2h row groups 4 wave .. + 3, wp row group wave, and (waves 0 .. 2) wp row group 10 + wave
    const int pc = (lane & 7) ^ (lane >> 3);                  // the piece this lane fetches: slot lane & 7 of row (lane >> 3) of an 8-row group
    const uint16_t* src[6];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = min(row0 + (wave * 4 + j) * 8 + (lane >> 3), N - 1);
        src[j] = A + (long)row * K;
    }
    src[4] = W + (long)min(wave * 8 + (lane >> 3), O - 1) * K;
    src[5] = W + (long)min((10 + wave) * 8 + (lane >> 3), O - 1) * K;
    const bool six = wave < 3;
    auto issue = [&](int step, int buf) {
        const long k0 = (long)(step0 + step) * FS_KS;
        const long off = k0 + (k0 + pc * 8 < K ? pc * 8 : 0);
        const uint32_t base = lds0 + (uint32_t)(buf * FS_STAGE);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_dma_1k(src[j] + off, base + (uint32_t)((wave * 4 + j) * 1024));
        lds_dma_1k(src[4] + off, base + (uint32_t)(FS_TM * FS_ROWB + wave * 1024));
        if (six) lds_dma_1k(src[5] + off, base + (uint32_t)(FS_TM * FS_ROWB + (10 + wave) * 1024));
    };
    if (nstep > 0) {
        const int r = lane & 31, h = lane >> 5;
        const int wr0 = min(cp * 64 + r, O - 1), wr1 = min(cp * 64 + 32 + r, O - 1);
        const int offa0 = (rp * 64 + r) * FS_ROWB, offa1 = offa0 + 32 * FS_ROWB;
        const int offb0 = (FS_TM + wr0) * FS_ROWB, offb1 = (FS_TM + wr1) * FS_ROWB;
        const int xa = r & 7, xb0 = wr0 & 7, xb1 = wr1 & 7;
        issue(0, 0);
        if (nstep > 1) issue(1, 1);
        for (int i = 0; i < nstep; ++i) {
            // stage i has landed when at most this wave's DMAs of stage i + 1 are still in flight
            if (i + 1 < nstep) {
                if (six) fs_wait_vm<6>(); else fs_wait_vm<5>();
            } else {
                fs_wait_vm<0>();
            }
            fs_barrier();                                      // everybody's pieces of stage i are there; everybody is done with stage i - 1
            if (i + 2 < nstep) issue(i + 2, (i + 2) % FS_RING);      // ... whose buffer is refilled
            const char* buf = fs_lds + (i % FS_RING) * FS_STAGE;
            const long left = K - (long)(step0 + i) * FS_KS;
            const int kv = left >= FS_KS ? FS_KS / 16 : (int)(left / 16);
#pragma unroll
            for (int ks = 0; ks < FS_KS / 16; ++ks) {
                if (ks < kv) {
                    const int c = ks * 2 + h;
                    const bf16x8 a0 = *(const bf16x8*)(buf + offa0 + ((c ^ xa) << 4)), a1 = *(const bf16x8*)(buf + offa1 + ((c ^ xa) << 4));
                    const bf16x8 b0 = *(const bf16x8*)(buf + offb0 + ((c ^ xb0) << 4)), b1 = *(const bf16x8*)(buf + offb1 + ((c ^ xb1) << 4));
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[3], 0, 0, 0);
                }
            }
        }
    }
    // accumulator element (e, lane) of a 32 x 32 product: row 8 (e >> 2) + (e & 3) + 4 (lane >> 5), column lane & 31
    float* o = out + (long)s * range_stride;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = cp * 64 + (t & 1) * 32 + (lane & 31);
        const int rb = row0 + rp * 64 + (t >> 1) * 32 + 4 * (lane >> 5);
        if (atomic) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = rb + 8 * (e >> 2) + (e & 3);
                if (row < N && col < O) atomicAdd(o + (long)row * O + col, acc[t][e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = rb + 8 * (e >> 2) + (e & 3);
                if (row < N && col < O) o[(long)row * O + col] = acc[t][e];
            }
        }
    }
}

// C[e] += sum over the k ranges of ws[range][e] -- `chunk` ranges per workgroup row, as the staged GEMM's split-K reduction does
__global__ __launch_bounds__(256) void fc_stream_reduce_kernel(const float* __restrict__ ws, int ranges, int chunk, long total, float* __restrict__ C) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int z0 = blockIdx.y * chunk, z1 = z0 + chunk < ranges ? z0 + chunk : ranges;
    float s = 0.f;
#pragma unroll 8
    for (int z = z0; z < z1; ++z) s += ws[(long)z * total + e];
    atomicAdd(C + e, s);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient, N <= WG_TN nodes.  The contraction runs over the node index.  A workgroup converts bf16(dgpre)^T [O][N] (rounded to
// nearest even like the staged GEMM's f32 loader; zero past N) into LDS once, as k-contiguous rows of WG_DPITCH bytes (656: the 16-byte
// fragment reads of 16 consecutive rows cover all 64 banks once); math wave w (of 4) then holds its outputs 32 w .. + 31 (past O: row
// O - 1 again, not stored) as 20 fragments in registers for the life of the workgroup.  Column tiles of WG_CT = 32 bf16 (64 bytes per row)
// of ALL rows of a2h stream through a ring of WG_RING = 4 stages of 20 KB, 20 DMA instructions of 1 KB (16 rows) each, three stages
// (60 KB) ahead of the matrix work.  The stage is the plain row-major image [n][32]; the matrix operand wants 8 consecutive n of one column
// per lane, which ds_read_b64_tr_b16 delivers from it: per 16-lane group a block of 4 rows x 16 columns, lane 4 q + p supplying the address
// of row q, columns 4 p .. 4 p + 3, every address a multiple of 8 bytes.  The 32 lanes of a half read 4 whole rows = 256 contiguous bytes,
// so the image needs no swizzle.  Rows past N repeat row N - 1 (finite data against zeros of dgpre^T); the pieces past K are loaded from
// the row's first piece of the tile and feed columns that are never stored.  A stage is 20 products of 32 x 32 x 16 per math wave, into two
// accumulators.
// A FIFTH wave issues all the loads and does the counted waits: stores count in vmcnt together with loads and may complete out of order
// with them, so a wave that both loads and stores can only wait for "at most n LOADS in flight" by waiting for its stores as well -- the
// first version (every wave five loads per stage and its 16 stores per tile) ran the ring one stage deep, 95 us against the staged GEMM's
// 78; with the loading wave 59 - 64.  The math waves meet it at the barrier and never wait on vmcnt.
constexpr int WG_TN = 320, WG_CT = 32, WG_ROWB = WG_CT * 2, WG_RING = 4, WG_OROWS = 100, WG_DPITCH = WG_TN * 2 + 16;
constexpr int WG_STAGE = WG_TN * WG_ROWB, WG_DBYTES = WG_OROWS * WG_DPITCH, WG_MATH_WAVES = 4, WG_THREADS = (WG_MATH_WAVES + 1) * 64;
static_assert(WG_DBYTES % 16 == 0 && WG_DBYTES + WG_RING * WG_STAGE <= 160 * 1024, "weight-gradient LDS");

__device__ __forceinline__ u32x2 fs_read_tr(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s16x4;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
    return __builtin_bit_cast(u32x2, v);
}

__global__ __launch_bounds__(WG_THREADS) void fc_stream_wgrad_kernel(const uint16_t* __restrict__ A, const float* __restrict__ dT, int N, int O,
                                                                     long K, int per, float* __restrict__ G) {
    extern __shared__ __attribute__((aligned(16))) char fs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = (int)((K + WG_CT - 1) / WG_CT);
    const int tile0 = blockIdx.x * per;
    const int ntile = min(tiles - tile0, per);
    if (ntile <= 0) return;
    char* dlds = fs_lds;
    char* ring = fs_lds + WG_DBYTES;
    const uint32_t ring0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)ring;
    const bool producer = wave == WG_MATH_WAVES;
    // the loading wave's 20 DMA instructions of a stage: row group j of 16 rows, lane -> row lane >> 2, piece lane & 3
    const int pc = lane & 3;
    auto issue = [&](int tile, int buf) {
        const long c0 = (long)(tile0 + tile) * WG_CT;
        const long off = c0 + (c0 + pc * 8 < K ? pc * 8 : 0);
#pragma unroll
        for (int j = 0; j < WG_TN / 16; ++j)
            lds_dma_1k(A + (long)min(j * 16 + (lane >> 2), N - 1) * K + off, ring0 + (uint32_t)(buf * WG_STAGE + j * 1024));
    };
    if (producer) {
        issue(0, 0);
        if (ntile > 1) issue(1, 1);
        if (ntile > 2) issue(2, 2);
    }
    // dgpre^T -> bf16 rows [o][n], two nodes per 4-byte store; 25 pairs of loads per thread in flight together (clamped, not guarded)
    constexpr int PAIRS = WG_OROWS * (WG_TN / 2), PER = PAIRS / WG_THREADS / 2;
    static_assert(2 * PER * WG_THREADS == PAIRS, "pairs per thread");
    for (int c = 0; c < 2; ++c) {
        float v0[PER], v1[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + (c * PER + j) * WG_THREADS;
            const int o = min(i / (WG_TN / 2), O - 1), n = (i % (WG_TN / 2)) * 2;
            v0[j] = dT[(long)o * N + min(n, N - 1)];
            v1[j] = dT[(long)o * N + min(n + 1, N - 1)];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + (c * PER + j) * WG_THREADS;
            const int o = i / (WG_TN / 2), n = (i % (WG_TN / 2)) * 2;
            *(uint32_t*)(dlds + o * WG_DPITCH + n * 2) = pack_bf16x2((o < O && n < N) ? v0[j] : 0.f, (o < O && n + 1 < N) ? v1[j] : 0.f);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fs_barrier();
    if (producer) {
        for (int i = 0; i < ntile; ++i) {
            // stage i has landed when at most the loads of stages i + 1 and i + 2 are still in flight
            if (i + 2 < ntile) fs_wait_vm<2 * (WG_TN / 16)>();
            else if (i + 1 < ntile) fs_wait_vm<WG_TN / 16>();
            else fs_wait_vm<0>();
            fs_barrier();                                              // stage i is there; the math waves are done with stage i - 1
            if (i + 3 < ntile) issue(i + 3, (i + 3) % WG_RING);        // ... whose buffer is refilled
        }
        return;
    }
    const int r = lane & 31, h = lane >> 5;
    const int orow = min(wave * 32 + r, O - 1);
    const char* pa = dlds + orow * WG_DPITCH + h * 16;
    // transposed read: 16-lane group g = lane >> 4 covers columns 16 (g & 1) .. + 15, rows 8 (g >> 1) + q (+ 4 for the second read)
    const int troff = (8 * h + ((lane & 15) >> 2)) * WG_ROWB + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    // this wave's 32 rows of dgpre^T stay in registers from here on: 20 fragments of 16 nodes
    bf16x8 afr[WG_TN / 16];
#pragma unroll
    for (int kb = 0; kb < WG_TN / 16; ++kb) afr[kb] = *(const bf16x8*)(pa + kb * 32);
    f32x16 acc0, acc1;
    for (int i = 0; i < ntile; ++i) {
        fs_barrier();
        const char* pb = ring + (i % WG_RING) * WG_STAGE + troff;
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
        // all 20 blocks of 16 nodes: blocks past N multiply clamped (finite) rows by zeros
#pragma unroll
        for (int kb2 = 0; kb2 < WG_TN / 32; ++kb2) {
            const char* q0 = pb + kb2 * 32 * WG_ROWB;
            const u32x2 l0 = fs_read_tr(q0), h0 = fs_read_tr(q0 + 4 * WG_ROWB);
            const u32x2 l1 = fs_read_tr(q0 + 16 * WG_ROWB), h1 = fs_read_tr(q0 + 20 * WG_ROWB);
            const u32x4 b0 = {l0[0], l0[1], h0[0], h0[1]}, b1 = {l1[0], l1[1], h1[0], h1[1]};
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[2 * kb2], __builtin_bit_cast(bf16x8, b0), acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[2 * kb2 + 1], __builtin_bit_cast(bf16x8, b1), acc1, 0, 0, 0);
        }
        const long col = (long)(tile0 + i) * WG_CT + r;
        const int ob = wave * 32 + 4 * h;
        if (col < K) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = ob + 8 * (e >> 2) + (e & 3);
                if (o < O) G[(long)o * K + col] = acc0[e] + acc1[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Input gradient with BatchNorm2's backward and conv2's ReLU mask: dz2h[n][k'] = x > 0 ? v - km1 - (x - mu) km2 : 0 with
// v = bf16(dgpre)[n][.] . wp[.][k'], x = a2h[n][k'] and the per-channel km1 / km2 / mu of the staged GEMM's interleaved epilogue
// (gemm_bf16.hip, GEMM_FUSED_INTERLEAVED): the contraction is the short side (100 outputs, 7 products of 16), the launch is an epilogue
// over a2h / dz2h with a small product in front of it.  A workgroup owns one row tile of DG_TM = 320 nodes and a contiguous range of
// column tiles of 64 bf16; math wave w (of 5) owns rows 64 w .. + 63 and keeps bf16(dgpre) of them (round to nearest even, zero past
// O) as 14 fragments in registers for the life of the workgroup.  A stage is the forward kernel's: 320 a2h rows + 104 wp rows of 128
// bytes, 53 DMA instructions, through a ring of three.  The SIXTH wave issues every DMA and does the counted waits (see the weight
// gradient: a wave's stores share vmcnt with its loads).  vmcnt counts to 63, so of the two stages the ring runs ahead about 63 KB per
// unit are in flight at a time -- several times what one unit's share of the memory rate needs.
//   wp    : the matrix operand wants 8 consecutive o of one column per lane: ds_read_b64_tr_b16 from the row-major image [o][64].  At a
//           128-byte pitch rows q and q + 2 of the 4 rows x 64 bytes that 32 lanes read share their banks: the two 64-byte halves of rows
//           2, 3 (mod 4) are exchanged (piece c in slot c ^ 4 ((o >> 1) & 1), through the source addresses), and the four rows cover all
//           64 banks once.  The seventh product's upper half (o = 104 .. 111) reads rows 96 .. 103 again: finite values against zeros.
//   a2h   : is not a matrix operand but the epilogue's x, swizzled like the forward's (piece c of row r in slot c ^ (r & 7): an
//           accumulator register's 32 columns x 2 rows, four rows apart, hit 32 different banks).  A lane reads x at its accumulator
//           coordinates and writes the bf16 result IN PLACE; a wave's 64 rows are its own, so without a workgroup barrier it then moves
//           them out as whole 16-byte pieces, 128-byte runs per row.  The stage is refilled after the next barrier: its data has left LDS
//           by then (the stores take their data from registers).
// The products are those of the staged GEMM (the same instruction, dgpre as its first operand, o ascending) and the epilogue is its
// expression: the result is bit-identical to it.  Rows past N repeat row N - 1, pieces past K the row's first piece of the tile; neither
// is stored.
constexpr int DG_TM = FS_TM, DG_CT = FS_KS, DG_ROWB = FS_ROWB, DG_WROWS = FS_WROWS, DG_RING = FS_RING, DG_STAGE = FS_STAGE;
constexpr int DG_MATH_WAVES = DG_TM / 64, DG_THREADS = (DG_MATH_WAVES + 1) * 64, DG_OMAX = 100, DG_KB = (DG_OMAX + 15) / 16;
constexpr int DG_LOADS = (DG_TM + DG_WROWS) / 8;
static_assert(DG_LOADS <= 63 && DG_WROWS % 8 == 0 && DG_WROWS >= 16 * (DG_KB - 1) + 8 && DG_RING * DG_STAGE <= 160 * 1024, "input-gradient stage");

__global__ __launch_bounds__(DG_THREADS) void fc_stream_dgrad_kernel(const float* __restrict__ D, const uint16_t* __restrict__ W,
                                                                     const uint16_t* __restrict__ A, const float* __restrict__ coef,
                                                                     const float* __restrict__ st2, int N, int O, long K, int per, int rtiles,
                                                                     uint16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char fs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = blockIdx.x % rtiles, s = blockIdx.x / rtiles;      // the row tiles of a column range are neighbours: they share its wp
    const int row0 = rt * DG_TM;
    const int tiles = (int)((K + DG_CT - 1) / DG_CT);
    const int tile0 = s * per;
    const int ntile = min(tiles - tile0, per);
    if (ntile <= 0) return;
    if (wave == DG_MATH_WAVES) {
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)fs_lds;
        // lane -> row lane >> 3 of an 8-row group, slot lane & 7; the piece that belongs there (see above)
        const int pca = (lane & 7) ^ (lane >> 3), pcw = (lane & 7) ^ (((lane >> 4) & 1) << 2);
        auto issue = [&](int tile, int buf) {
            const long c0 = (long)(tile0 + tile) * DG_CT;
            const long offa = c0 + (c0 + pca * 8 < K ? pca * 8 : 0), offw = c0 + (c0 + pcw * 8 < K ? pcw * 8 : 0);
            const uint32_t base = lds0 + (uint32_t)(buf * DG_STAGE);
#pragma unroll
            for (int j = 0; j < DG_TM / 8; ++j)
                lds_dma_1k(A + (long)min(row0 + j * 8 + (lane >> 3), N - 1) * K + offa, base + (uint32_t)(j * 1024));
#pragma unroll
            for (int j = 0; j < DG_WROWS / 8; ++j)
                lds_dma_1k(W + (long)min(j * 8 + (lane >> 3), O - 1) * K + offw, base + (uint32_t)(DG_TM * DG_ROWB + j * 1024));
        };
        issue(0, 0);
        if (ntile > 1) issue(1, 1);
        for (int i = 0; i < ntile; ++i) {
            // stage i has landed when at most the loads of stage i + 1 are still in flight
            if (i + 1 < ntile) fs_wait_vm<DG_LOADS>(); else fs_wait_vm<0>();
            fs_barrier();                                              // stage i is there; the math waves have moved stage i - 1 out
            if (i + 2 < ntile) issue(i + 2, (i + 2) % DG_RING);        // ... whose buffer is refilled
        }
        return;
    }
    const int r = lane & 31, h = lane >> 5;
    // this wave's 64 rows of bf16(dgpre) stay in registers: 2 x 7 fragments of 16 outputs
    bf16x8 afr[2][DG_KB];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        const float* d = D + (long)min(row0 + wave * 64 + t2 * 32 + r, N - 1) * O;
#pragma unroll
        for (int kb = 0; kb < DG_KB; ++kb) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int o = kb * 16 + 8 * h + j;
                const float x = d[min(o, O - 1)];
                v[j] = o < O ? x : 0.f;
            }
            afr[t2][kb] = pack8(v);
        }
    }
    const int c = lane & 15;                                           // a column tile starts at a multiple of 64: one channel per lane
    const float km1 = coef[32 + c] * coef[c], km2 = coef[32 + c] * coef[16 + c] * st2[48 + c], mu = st2[32 + c];
    // transposed reads of wp: 16-lane group g covers columns 16 (g & 1) .. + 15, lane 4 q + p of it row q, columns 4 p .. + 3
    const int q = (lane & 15) >> 2, qb = (q >> 1) & 1;
    int trw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) trw[j] = DG_TM * DG_ROWB + q * DG_ROWB + (j ^ qb) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
    // x / result of accumulator register e: row 8 (e >> 2) + (e & 3) + 4 h of a 32 x 32 tile, column lane & 31
    int xoff[4][2];
#pragma unroll
    for (int e3 = 0; e3 < 4; ++e3)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r7 = e3 + 4 * h;
            xoff[e3][j] = (wave * 64 + r7) * DG_ROWB + (((j * 4 + (r >> 3)) ^ r7) << 4) + (r & 7) * 2;
        }
    const int pc = (lane & 7) ^ (lane >> 3);                           // the piece in slot lane & 7 of row lane >> 3 (mod 8)
    for (int i = 0; i < ntile; ++i) {
        fs_barrier();
        char* buf = fs_lds + (i % DG_RING) * DG_STAGE;
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
        for (int kb = 0; kb < DG_KB; ++kb) {
            const int rowb = 16 * kb + 8 * h < DG_WROWS ? 16 * kb + 8 * h : 16 * kb;
            bf16x8 b[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const char* p = buf + rowb * DG_ROWB + trw[j];
                const u32x2 lo = fs_read_tr(p), hi = fs_read_tr(p + 4 * DG_ROWB);
                const u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                b[j] = __builtin_bit_cast(bf16x8, t);
            }
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[0][kb], b[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[0][kb], b[1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[1][kb], b[0], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[1][kb], b[1], acc[3], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // all 16 reads of a tile before its first write: the compiler cannot reorder a read over a write that may alias it
            uint16_t xb[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) xb[e] = *(const uint16_t*)(buf + ((t >> 1) * 32 + 8 * (e >> 2)) * DG_ROWB + xoff[e & 3][t & 1]);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float x = __uint_as_float((uint32_t)xb[e] << 16);
                const float v = acc[t][e];
                const float o = x > 0.f ? v - km1 - (x - mu) * km2 : 0.f;
                *(uint16_t*)(buf + ((t >> 1) * 32 + 8 * (e >> 2)) * DG_ROWB + xoff[e & 3][t & 1]) = __builtin_bit_cast(uint16_t, (__bf16)o);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the wave's own rows: LDS serves a wave in order
        const long col = (long)(tile0 + i) * DG_CT + pc * 8;
        uint4 piece[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) piece[it] = *(const uint4*)(buf + (wave * 64 + it * 8 + (lane >> 3)) * DG_ROWB + (lane & 7) * 16);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = row0 + wave * 64 + it * 8 + (lane >> 3);
            if (row < N && col < K) *(uint4*)(out + (long)row * K + col) = piece[it];
        }
    }
}

int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && e[0] ? atoi(e) : dflt;
}

}  // namespace

bool dgl_fc_stream_wgrad_ok(int N) { return N <= WG_TN; }

// gpre [N][O] += a2h [N][K] . wp [O][K]^T (both bf16, K a multiple of 16).  ws: split-K workspace of ws_floats floats (16-byte aligned, may
// be null): the product runs over as many k ranges as it holds partial results for, at most FS_RANGES.
// FS_RANGES: inside the training step the encoder's persistent launch leaves 96 of the 256 units and one workgroup fills a unit; in the
// step 96 ranges take 85 - 88 us, 128 (a second round of 32) 124, 192 92 - 94, 256 110.  STEP_DGL_FC_STREAM_RANGES (read on every call)
// overrides it for measurements.
constexpr int FS_RANGES = 96;
int dgl_fc_stream_fwd(const void* a2h, const void* wp, int N, int O, long K, float* gpre, float* ws, long ws_floats, hipStream_t st) {
    STEP_REQUIRE(a2h && wp && gpre && N > 0 && O > 0 && O <= FS_WROWS && K > 0 && K % 16 == 0, "dgl_fc_stream_fwd: bad arguments");
    const int ksteps = (int)((K + FS_KS - 1) / FS_KS);
    const long mn = (long)N * O;
    long ranges = (ws && (((uintptr_t)ws) & 15) == 0) ? ws_floats / mn : 1;
    const int want = env_int("STEP_DGL_FC_STREAM_RANGES", FS_RANGES);
    if (ranges > want) ranges = want;
    if (ranges > ksteps) ranges = ksteps;
    if (ranges < 1) ranges = 1;
    const int per = (ksteps + (int)ranges - 1) / (int)ranges;
    const int used = (ksteps + per - 1) / per;                         // ranges that hold at least one k step
    STEP_TRY(step_raise_lds_once((const void*)fc_stream_fwd_kernel, 160 * 1024, "dgl_fc_stream_fwd"));
    const dim3 grid(used, cdiv(N, FS_TM));
    const bool direct = used == 1;
    fc_stream_fwd_kernel<<<grid, FS_WAVES * 64, FS_RING * FS_STAGE, st>>>((const uint16_t*)a2h, (const uint16_t*)wp, N, O, K, per, direct ? gpre : ws,
                                                                         direct ? 0 : mn, direct ? 1 : 0);
    STEP_LAUNCH_CHECK("dgl_fc_stream_fwd");
    if (!direct) {
        const int chunk = 16;
        fc_stream_reduce_kernel<<<dim3((unsigned)((mn + 255) / 256), (unsigned)cdiv(used, chunk)), 256, 0, st>>>(ws, used, chunk, mn, gpre);
        STEP_LAUNCH_CHECK("dgl_fc_stream_fwd(reduce)");
    }
    return STEP_OK;
}

// G [O][K] = bf16(dgpreT)[O][N] . a2h [N][K] (dgpreT f32 with the node index contiguous, a2h bf16), N <= 320 (dgl_fc_stream_wgrad_ok)
int dgl_fc_stream_wgrad(const void* a2h, const float* dgpreT, int N, int O, long K, float* G, hipStream_t st) {
    STEP_REQUIRE(a2h && dgpreT && G && N > 0 && N <= WG_TN && O > 0 && O <= WG_OROWS && K > 0 && K % 16 == 0, "dgl_fc_stream_wgrad: bad arguments");
    const int tiles = (int)((K + WG_CT - 1) / WG_CT);
    int groups = env_int("STEP_DGL_FC_STREAM_WGROUPS", 256);           // one workgroup per unit (read on every call: measurements)
    if (groups > tiles) groups = tiles;
    if (groups < 1) groups = 1;
    const int per = (tiles + groups - 1) / groups;
    STEP_TRY(step_raise_lds_once((const void*)fc_stream_wgrad_kernel, 160 * 1024, "dgl_fc_stream_wgrad"));
    fc_stream_wgrad_kernel<<<(tiles + per - 1) / per, WG_THREADS, WG_DBYTES + WG_RING * WG_STAGE, st>>>((const uint16_t*)a2h, dgpreT, N, O, K, per, G);
    STEP_LAUNCH_CHECK("dgl_fc_stream_wgrad");
    return STEP_OK;
}

// Up to three row tiles (STEP_PEMS07's 883 nodes) the step is faster on the kernel; at 4096 nodes (13 row tiles) the launch takes what the
// staged GEMM takes (1366 against 1375 us) and the step measured slower, so larger graphs keep the staged GEMM
// (profiles/dgl_fc_dgrad_after.md; nothing between 883 and 4096 nodes was measured).
constexpr int DG_MAX_RTILES = 3;
bool dgl_fc_stream_dgrad_ok(int N, long K) { return N > 0 && N <= DG_MAX_RTILES * DG_TM && K > 0; }

// dz2h [N][K] (bf16) = BatchNorm2 backward + conv2 ReLU mask of bf16(dgpre)[N][O] . wp[O][K] (wp, a2h bf16; K a multiple of 16): what the
// staged GEMM's GEMM_FUSED_INTERLEAVED epilogue stores, bit for bit.  At most one workgroup per unit: DG_GROUPS column ranges spread over
// the row tiles.  (STEP_PEMS07 queues the next batch's encoder late, so it runs next to the backward on 128 units; 128 workgroups were
// measured there against 256 and are within the run-to-run range: 5.106 / 5.184 / 5.187 against 5.151 / 5.159 / 5.122 ms per step.)
// STEP_DGL_FC_STREAM_DGROUPS (read on every call) overrides it for measurements.
constexpr int DG_GROUPS = 256;
int dgl_fc_stream_dgrad(const float* dgpre, const void* wp, const void* a2h, const float* coef, const float* st2, int N, int O, long K,
                        void* dz2h, hipStream_t st) {
    STEP_REQUIRE(dgpre && wp && a2h && coef && st2 && dz2h && N > 0 && O > 0 && O <= DG_OMAX && K > 0 && K % 16 == 0,
                 "dgl_fc_stream_dgrad: bad arguments");
    STEP_REQUIRE(((((uintptr_t)wp) | ((uintptr_t)a2h) | ((uintptr_t)dz2h)) & 15) == 0, "dgl_fc_stream_dgrad: wp, a2h and dz2h must be 16-byte aligned");
    const int tiles = (int)((K + DG_CT - 1) / DG_CT), rtiles = cdiv(N, DG_TM);
    int ranges = env_int("STEP_DGL_FC_STREAM_DGROUPS", DG_GROUPS) / rtiles;
    if (ranges > tiles) ranges = tiles;
    if (ranges < 1) ranges = 1;
    const int per = (tiles + ranges - 1) / ranges;
    const int used = (tiles + per - 1) / per;                          // ranges that hold at least one tile
    STEP_TRY(step_raise_lds_once((const void*)fc_stream_dgrad_kernel, 160 * 1024, "dgl_fc_stream_dgrad"));
    fc_stream_dgrad_kernel<<<used * rtiles, DG_THREADS, DG_RING * DG_STAGE, st>>>(dgpre, (const uint16_t*)wp, (const uint16_t*)a2h, coef, st2, N, O, K, per,
                                                                                 rtiles, (uint16_t*)dz2h);
    STEP_LAUNCH_CHECK("dgl_fc_stream_dgrad");
    return STEP_OK;
}
