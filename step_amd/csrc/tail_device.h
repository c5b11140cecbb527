// Device helpers shared by the iteration tails (csrc/train_tail.hip, csrc/pretrain_tail.hip): the rescaled element and its mask, the
// masked-error terms of basicts/metrics/{mae,rmse,mape}.py, the workgroup reduction, and the two-half work buffer.
//
// Work buffer (f64, zeroed by the caller ONCE, then owned by the calls of one stream):
//   [0, 6)    sums of the even calls   {S_abs, S_sq, cnt, S_ape, cnt0, S_bce}
//   [6, 12)   sums of the odd calls
//   12        index of the NEXT call (an unsigned 64-bit integer in the slot): written by a finish launch, read by the next reduce launch
//   13        index of the CURRENT call: written by a reduce launch, read by its finish launch
// Call n adds into half n & 1; its finish launch reads that half and clears the other one for call n + 1, so no memset is queued.
// Inside a launch the workgroups meet only in the atomic adds; whatever reads a sum or an index does so in a LATER launch of the same
// stream, and no word is both written and read inside one launch.
#pragma once
#include "common.h"

constexpr int TT_THREADS = 256;          // four waves per workgroup
constexpr int TT_WAVES = TT_THREADS / 64;
constexpr int TT_SUMS = 6;
constexpr int TT_NEXT = 2 * TT_SUMS, TT_CUR = 2 * TT_SUMS + 1;
constexpr long TT_WORK_DOUBLES = 2 * TT_SUMS + 2;

// The rescaling must round twice, like torch's `x * std + mean`: a label ONE float32 step across the 5e-5 / 1e-4 thresholds changes its
// mask (csrc/eval_metrics.hip has the whole story).  Contraction is off in every function that rescales, and the arithmetic is written
// with plain operators.
struct TailElem { float p, y; bool m; };
__device__ __forceinline__ TailElem tail_rescale(float p, float y, float scale, float shift, float null_val) {
#pragma clang fp contract(off)
    TailElem e;
    e.p = p * scale + shift;
    e.y = y * scale + shift;
    e.m = !(fabsf(e.y - null_val) <= 5e-5f);          // mae.py:17-21: ~isclose(y, null, atol = 5e-5, rtol = 0); a NaN label counts
    return e;
}

// The tails' own rescale.  NAN_NULL = false is tail_rescale itself; true is the reference's default null_val = NaN (mae.py:17-18): only a
// NaN label is masked.  A template parameter, not a branch: the loss kernels of csrc/optim.hip call tail_rescale and stay as they are.
template <bool NAN_NULL>
__device__ __forceinline__ TailElem tail_rescale_null(float p, float y, float scale, float shift, float null_val) {
#pragma clang fp contract(off)
    if constexpr (!NAN_NULL) {
        return tail_rescale(p, y, scale, shift, null_val);
    } else {
        TailElem e;
        e.p = p * scale + shift;
        e.y = y * scale + shift;
        e.m = !isnan(e.y);
        return e;
    }
}

// f32 terms as the reference computes them, added to the lane's f64 sums s[0..4]
__device__ __forceinline__ void tail_accumulate(const TailElem& e, double* s) {
#pragma clang fp contract(off)
    if (e.m) {
        const float d = e.p - e.y, ad = fabsf(d), sq = d * d;
        if (!isnan(ad)) s[0] += (double)ad;          // where(isnan(loss), 0, loss), mae.py:27: the element still counts
        if (!isnan(sq)) s[1] += (double)sq;
        s[2] += 1.0;
    }
    // mape.py:20-35: labels below 1e-4 become 0, the null value is 0 whatever the caller's
    const float y0 = fabsf(e.y) < 1e-4f ? 0.f : e.y;
    if (!(fabsf(y0) <= 5e-5f)) {
        const float t = fabsf(fabsf(e.p - y0) / y0);
        if (!isnan(t)) s[3] += (double)t;
        s[4] += 1.0;
    }
}

// d |p - y| / d p times g; a NaN difference compares false twice: gradient 0
__device__ __forceinline__ float tail_sign_grad(const TailElem& e, float g) {
#pragma clang fp contract(off)
    const float d = e.p - e.y;
    return e.m ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 0.f;
}

// The lane sums of a workgroup of TT_THREADS: over the wave by shuffles, over the four waves through LDS (red), then one atomic add per
// sum per workgroup into the half of call `call`; block 0 records the call index for the finish launch.  Every thread must arrive.
__device__ __forceinline__ void tail_block_add(double* s, double (*red)[TT_SUMS], double* work, unsigned long long call) {
#pragma unroll
    for (int j = 0; j < TT_SUMS; ++j)
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < TT_SUMS; ++j) red[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
    if (threadIdx.x < TT_SUMS) {
        const int j = threadIdx.x;
        atomicAdd(work + (call & 1) * TT_SUMS + j, red[0][j] + red[1][j] + red[2][j] + red[3][j]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(work)[TT_CUR] = call;
}

// One thread of the finish launch: MAE / RMSE / MAPE from the finished half `sum`, the other half cleared, the call index advanced.
// -> the MAE (the loss's error term)
__device__ __forceinline__ float tail_finish_values(const double* sum, double* work, unsigned long long call, float* metrics) {
    const double cnt = sum[2], cnt0 = sum[4];
    const float mae = cnt > 0.0 ? (float)(sum[0] / cnt) : 0.f;
    metrics[0] = mae;
    metrics[1] = cnt > 0.0 ? (float)sqrt(sum[1] / cnt) : 0.f;
    metrics[2] = cnt0 > 0.0 ? (float)(sum[3] / cnt0) : 0.f;
    double* other = work + ((call + 1) & 1) * TT_SUMS;
    for (int j = 0; j < TT_SUMS; ++j) other[j] = 0.0;
    reinterpret_cast<unsigned long long*>(work)[TT_NEXT] = call + 1;
    return mae;
}
