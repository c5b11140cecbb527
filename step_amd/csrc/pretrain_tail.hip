// The tail of one TSFormer pre-training iteration (include/step_hip.h, "pre-training tail"): masked MAE on the RESCALED reconstruction
// of the masked tokens and their labels, its gradient in the layout of the decoder's output, and the three training meters, in two
// launches that read the decoder's output r [S, P, 12] and the packed series [S, P * 12] in place -- what the reference does with a
// slice + reshape of r, an advanced-index gather of the series (step/step_arch/tsformer/tsformer.py:152-158), two rescales, masked_mae,
// three metric functions and their autograd nodes (basicts/runners/base_tsf_runner.py:237-254, basicts/metrics/{mae,rmse,mape}.py).
//
// A masked token is 12 floats = three 16-byte vectors, contiguous in both tensors.  The work item is one such vector: vector v of
// sequence s is token v / 3, quarter v % 3, so consecutive lanes read consecutive addresses of r (the masked rows of a sequence are
// adjacent) and 48-byte runs of the series.  The work buffer and the device helpers are those of csrc/tail_device.h.
#include "tail_device.h"
#include <limits.h>
#include <cmath>

namespace {

struct PretrainTailArgs {
    const float* r; const float* series; const int* mk;
    int S, P, Pm;
    float scale, shift, null_val;
    double* work;
};

__device__ __forceinline__ f32x4 load4(const float* base, long vec) { return *reinterpret_cast<const f32x4*>(base + 4 * vec); }

// the label vector that belongs to vector `rem` (= 3 * token + quarter) of the masked rows of sequence s
__device__ __forceinline__ f32x4 label4(const PretrainTailArgs& a, unsigned s, unsigned rem) {
    const unsigned j = rem / 3u, q = rem - 3u * j;
    return load4(a.series, ((long)s * a.P + a.mk[j]) * 3 + q);
}

// Launch 1.  Grid-stride over the S * Pm * 3 vectors of the masked tokens; f32 terms as the reference computes them, summed in f64.
// NAN_NULL: the mask of a NaN null_val (tail_rescale_null), an instantiation of its own.
template <bool NAN_NULL>
__global__ __launch_bounds__(TT_THREADS) void pretrain_tail_reduce_kernel(PretrainTailArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[TT_WAVES][TT_SUMS];
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_NEXT];
    double s[TT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned m3 = 3u * a.Pm, p3 = 3u * a.P, u3 = p3 - m3;          // (S * P * 12 < 2^31: 32-bit divisions)
    const long n = (long)a.S * m3;
    for (long i = first; i < n; i += stride) {
        const unsigned sq = (unsigned)i / m3, rem = (unsigned)i - sq * m3;
        const f32x4 p = load4(a.r, (long)sq * p3 + u3 + rem), y = label4(a, sq, rem);
#pragma unroll
        for (int c = 0; c < 4; ++c) tail_accumulate(tail_rescale_null<NAN_NULL>(p[c], y[c], a.scale, a.shift, a.null_val), s);
    }
    tail_block_add(s, red, a.work, call);
}

// Launch 2.  Every workgroup reads the finished sums; block 0 writes the loss and the metrics, clears the other half and advances the call
// index; all of them write dr over the FULL [S, P, 12] as 16-byte vectors (exact zeros in the unmasked rows, at masked labels and at NaN
// differences).  dr == NULL: one workgroup, values only.
template <bool NAN_NULL>
__global__ __launch_bounds__(TT_THREADS) void pretrain_tail_finish_kernel(PretrainTailArgs a, float* __restrict__ loss,
                                                                          float* __restrict__ metrics, float* __restrict__ dr) {
#pragma clang fp contract(off)
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_CUR];
    const double* sum = a.work + (call & 1) * TT_SUMS;
    const double cnt = sum[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss = tail_finish_values(sum, a.work, call, metrics);
    if (!dr) return;
    const float g = cnt > 0.0 ? (float)(1.0 / cnt) * a.scale : 0.f;      // d/d r of the mean on r * scale + shift
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned m3 = 3u * a.Pm, p3 = 3u * a.P, u3 = p3 - m3;
    const long n_all = (long)a.S * p3;
    for (long i = first; i < n_all; i += stride) {
        const unsigned sq = (unsigned)i / p3, row3 = (unsigned)i - sq * p3;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row3 >= u3) {
            const f32x4 p = load4(a.r, i), y = label4(a, sq, row3 - u3);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = tail_sign_grad(tail_rescale_null<NAN_NULL>(p[c], y[c], a.scale, a.shift, a.null_val), g);
        }
        *reinterpret_cast<f32x4*>(dr + 4 * i) = v;
    }
}

}  // namespace

extern "C" long step_pretrain_tail_work_doubles(void) { return TT_WORK_DOUBLES; }

extern "C" int step_pretrain_tail(const float* r, const float* series, const int* mk, int S, int P, int Pm, float scale, float shift,
                                  float null_val, double* work, float* loss, float* metrics, float* dr, void* stream) {
    STEP_REQUIRE(r && series && mk && work && loss && metrics, "pretrain_tail: NULL buffer");
    STEP_REQUIRE(S > 0 && P > 0 && Pm >= 1 && Pm <= P, "pretrain_tail: need S > 0 and 1 <= Pm <= P (S = %d, P = %d, Pm = %d)", S, P, Pm);
    STEP_REQUIRE((long)S * P * 12 <= INT_MAX, "pretrain_tail: S * P * 12 = %ld exceeds the %d elements of one call", (long)S * P * 12, INT_MAX);
    STEP_REQUIRE(!std::isinf(null_val), "pretrain_tail: null_val must be finite or NaN");
    STEP_REQUIRE(((uintptr_t)r & 15) == 0 && ((uintptr_t)series & 15) == 0 && ((uintptr_t)dr & 15) == 0,
                 "pretrain_tail: r, series and dr are read and written as 16-byte vectors and must be 16-byte aligned");
    PretrainTailArgs a;
    a.r = r; a.series = series; a.mk = mk;
    a.S = S; a.P = P; a.Pm = Pm;
    a.scale = scale; a.shift = shift; a.null_val = null_val;
    a.work = work;
    const long n_inc = (long)S * Pm * 3, n_all = (long)S * P * 3;
    // six f64 atomics per workgroup onto six addresses (the graph term's adds 0): at least four vectors (16 elements) per thread where there are that many
    int rblocks = (int)(n_inc / (4 * TT_THREADS));
    rblocks = rblocks < 1 ? 1 : (rblocks > 256 ? 256 : rblocks);
    int fblocks = dr ? cdiv(n_all, TT_THREADS) : 1;
    if (fblocks > 2048) fblocks = 2048;
    const hipStream_t st = (hipStream_t)stream;
    if (null_val != null_val) {
        pretrain_tail_reduce_kernel<true><<<rblocks, TT_THREADS, 0, st>>>(a);
        STEP_LAUNCH_CHECK("pretrain_tail_reduce");
        pretrain_tail_finish_kernel<true><<<fblocks, TT_THREADS, 0, st>>>(a, loss, metrics, dr);
    } else {
        pretrain_tail_reduce_kernel<false><<<rblocks, TT_THREADS, 0, st>>>(a);
        STEP_LAUNCH_CHECK("pretrain_tail_reduce");
        pretrain_tail_finish_kernel<false><<<fblocks, TT_THREADS, 0, st>>>(a, loss, metrics, dr);
    }
    STEP_LAUNCH_CHECK("pretrain_tail_finish");
    return STEP_OK;
}
