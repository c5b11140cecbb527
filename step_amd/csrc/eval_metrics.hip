// Evaluation metrics of a whole validation / test pass (include/step_hip.h, "evaluation metrics"): the reference's masked MAE / RMSE /
// MAPE (basicts/metrics/{mae,rmse,mape}.py) per horizon, over everything and as the mean of the per-batch values, accumulated on the
// device over any number of batches and read back once.  One launch per batch, one tiny launch per pass.
//
// Accumulator (f64, zeroed by the caller once per pass; A = 5 sums {S_abs, S_sq, cnt, S_ape, cnt0}):
//   [0, 5H)            the sums of horizon h at 5 h
//   [5H, 5H + 5)       the sums of the CURRENT call (all horizons); zero between calls
//   [5H + 5, 5H + 8)   sum over calls of the call's own MAE, RMSE, MAPE
//   5H + 8             number of calls
//   5H + 9             ticket counter of the current call (its low 32 bits as an unsigned int); zero between calls
// Calls on one accumulator must be ordered by their stream: the per-call slots belong to one launch at a time.
#include "common.h"
#include <limits.h>
#include <type_traits>

namespace {

constexpr int EM_THREADS = 256;          // four waves per workgroup
constexpr int EM_WAVES = EM_THREADS / 64;
constexpr int EM_MAX_H = 64;
constexpr int EM_SUMS = 5;
constexpr int EM_GRID_TARGET = 384;      // workgroups of one launch: H * chunks stays near this

__host__ __device__ inline long em_acc_doubles(int H) { return (long)EM_SUMS * H + EM_SUMS + 3 + 1 + 1; }

// NODES = false: one scale and one shift (float); true: f32 [N] of each on the device, read at the element's node -- two instantiations
// of the kernel, nothing is chosen per element
template <bool NODES>
struct MetricArgs {
    using Scaler = std::conditional_t<NODES, const float*, float>;
    const float* pred; long p_sb, p_sh, p_sn;
    const float* real; long r_sb, r_sh, r_sn;
    int B, H, N;
    unsigned per_h;            // B * N elements of one horizon
    Scaler scale, shift;
    float null_val;
    int null_is_nan;
    double* acc;
};

__device__ __forceinline__ double metric_of(double sum, double cnt) { return cnt > 0.0 ? sum / cnt : 0.0; }

// The value an accumulator slot holds at the device's coherence point (the adds of the other workgroups are atomics there).
__device__ __forceinline__ double slot_value(double* p) { return atomicAdd(p, 0.0); }

// grid (chunks, H).  Workgroup (c, h) walks the B * N elements of horizon h from c * 256 in steps of chunks * 256: consecutive lanes
// read consecutive n (the prediction's rows are contiguous, the label is one channel of [.., N, C]), a wave straddles a row's end at most
// once per step.  f32 terms as the reference computes them, summed in f64: per lane, over the wave by shuffles, over the four waves
// through LDS; lanes 0..4 then add the workgroup's five sums to the horizon's slots and to the call's.  Those ten atomics RETURN their old
// values into LDS, so they have been performed when the barrier behind them is passed and the ticket is drawn; the workgroup that draws
// the last ticket turns the call's sums into the call's three metrics and clears the per-call slots for the next launch.
template <bool NODES>
__global__ __launch_bounds__(EM_THREADS) void eval_metrics_kernel(MetricArgs<NODES> a) {
    // The rescaling must round twice, like torch's `x * std + mean`: a label ONE float32 step across the 5e-5 / 1e-4 thresholds changes its
    // mask, and its MAPE term by tens of percent.  hipcc contracts a * b + c into one fma by default -- also through __fmul_rn / __fadd_rn,
    // which are plain `*` / `+` carrying the header's contraction flag -- so the arithmetic below is written with operators and
    // contraction is off for this whole body (the assembly has v_mul_f32 + v_add_f32 here).
#pragma clang fp contract(off)
    __shared__ double red[EM_WAVES][EM_SUMS];
    __shared__ volatile double performed[2 * EM_SUMS];
    __shared__ bool last;
    const int h = blockIdx.y;
    const float* pred = a.pred + (long)h * a.p_sh;
    const float* real = a.real + (long)h * a.r_sh;
    double s[EM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const unsigned step = gridDim.x * EM_THREADS;
    for (unsigned i = blockIdx.x * EM_THREADS + threadIdx.x; i < a.per_h; i += step) {
        const unsigned b = i / (unsigned)a.N, n = i - b * (unsigned)a.N;
        float scale, shift;
        if constexpr (NODES) { scale = a.scale[n]; shift = a.shift[n]; } else { scale = a.scale; shift = a.shift; }
        const float p = pred[(long)b * a.p_sb + (long)n * a.p_sn] * scale + shift;
        const float y = real[(long)b * a.r_sb + (long)n * a.r_sn] * scale + shift;
        // mae.py:17-21 / rmse.py:17-21: ~isnan(y), or ~isclose(y, null, atol = 5e-5, rtol = 0) -- a NaN label is not close to a finite null
        const bool m = a.null_is_nan ? !isnan(y) : !(fabsf(y - a.null_val) <= 5e-5f);
        if (m) {
            const float d = p - y, ad = fabsf(d), sq = d * d;
            if (!isnan(ad)) s[0] += (double)ad;          // where(isnan(loss), 0, loss): the element still counts
            if (!isnan(sq)) s[1] += (double)sq;
            s[2] += 1.0;
        }
        // mape.py:21-35: labels below 1e-4 become 0, the null value is 0 whatever the caller's
        const float y0 = fabsf(y) < 1e-4f ? 0.f : y;
        if (!(fabsf(y0) <= 5e-5f)) {
            const float t = fabsf(fabsf(p - y0) / y0);
            if (!isnan(t)) s[3] += (double)t;
            s[4] += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < EM_SUMS; ++k)
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < EM_SUMS; ++k) red[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    double* call = a.acc + (long)EM_SUMS * a.H;
    if (threadIdx.x < EM_SUMS) {
        const int k = threadIdx.x;
        const double v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        performed[k] = atomicAdd(a.acc + (long)EM_SUMS * h + k, v);
        performed[EM_SUMS + k] = atomicAdd(call + k, v);
    }
    __threadfence();
    __syncthreads();
    unsigned int* ticket = reinterpret_cast<unsigned int*>(call + EM_SUMS + 3 + 1);
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x * gridDim.y - 1;
    __syncthreads();
    if (last && threadIdx.x == 0) {
        __threadfence();
        double c[EM_SUMS];
        for (int k = 0; k < EM_SUMS; ++k) c[k] = slot_value(call + k);
        double* mean = call + EM_SUMS;
        mean[0] += metric_of(c[0], c[2]);                // the only writer of these four slots in this launch
        mean[1] += sqrt(metric_of(c[1], c[2]));
        mean[2] += metric_of(c[3], c[4]);
        mean[3] += 1.0;
        for (int k = 0; k < EM_SUMS; ++k) call[k] = 0.0;
        *ticket = 0u;
    }
}

// one workgroup: thread h < H the three metrics of horizon h, thread H those of all horizons, thread H + 1 the mean over the calls
__global__ __launch_bounds__(128) void eval_metrics_finish_kernel(const double* __restrict__ acc, int H, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t > H + 1) return;
    double* o = out + 3 * t;
    if (t == H + 1) {
        const double* mean = acc + (long)EM_SUMS * H + EM_SUMS;
        for (int k = 0; k < 3; ++k) o[k] = metric_of(mean[k], mean[3]);
        return;
    }
    double c[EM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int h = (t < H ? t : 0); h < (t < H ? t + 1 : H); ++h)
        for (int k = 0; k < EM_SUMS; ++k) c[k] += acc[EM_SUMS * h + k];
    o[0] = metric_of(c[0], c[2]);
    o[1] = sqrt(metric_of(c[1], c[2]));
    o[2] = metric_of(c[3], c[4]);
}

}  // namespace

extern "C" long step_eval_metrics_acc_doubles(int H) { return H < 1 || H > EM_MAX_H ? 0 : em_acc_doubles(H); }

namespace {

template <bool NODES>
int eval_metrics_launch(const char* op, const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn,
                        int B, int H, int N, typename MetricArgs<NODES>::Scaler scale, typename MetricArgs<NODES>::Scaler shift, float null_val,
                        double* acc, void* stream) {
    STEP_REQUIRE(pred && real && acc, "%s: NULL pred, real or acc", op);
    if constexpr (NODES) STEP_REQUIRE(scale && shift, "%s: NULL scale_n or shift_n", op);
    STEP_REQUIRE(B > 0 && H > 0 && N > 0, "%s: B = %d, H = %d, N = %d must all be positive", op, B, H, N);
    STEP_REQUIRE(H <= EM_MAX_H, "%s: H = %d exceeds the %d horizons of one accumulator", op, H, EM_MAX_H);
    STEP_REQUIRE(p_sb > 0 && p_sh > 0 && p_sn > 0 && r_sb > 0 && r_sh > 0 && r_sn > 0,
                 "%s: element strides must be positive (pred %ld, %ld, %ld; real %ld, %ld, %ld)", op, p_sb, p_sh, p_sn, r_sb, r_sh, r_sn);
    STEP_REQUIRE((long)B * N <= INT_MAX, "%s: B * N = %ld exceeds the %d elements per horizon of one launch", op, (long)B * N, INT_MAX);
    MetricArgs<NODES> a;
    a.pred = pred; a.p_sb = p_sb; a.p_sh = p_sh; a.p_sn = p_sn;
    a.real = real; a.r_sb = r_sb; a.r_sh = r_sh; a.r_sn = r_sn;
    a.B = B; a.H = H; a.N = N; a.per_h = (unsigned)((long)B * N);
    a.scale = scale; a.shift = shift; a.null_val = null_val; a.null_is_nan = null_val != null_val;
    a.acc = acc;
    // at least four elements per lane where there are that many, H * chunks near EM_GRID_TARGET at most
    int chunks = cdiv(a.per_h, 4 * EM_THREADS);
    const int most = EM_GRID_TARGET / H > 1 ? EM_GRID_TARGET / H : 1;
    chunks = chunks < 1 ? 1 : (chunks > most ? most : chunks);
    eval_metrics_kernel<NODES><<<dim3(chunks, H), EM_THREADS, 0, (hipStream_t)stream>>>(a);
    STEP_LAUNCH_CHECK("eval_metrics_accumulate");
    return STEP_OK;
}

}  // namespace

extern "C" int step_eval_metrics_accumulate(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh,
                                            long r_sn, int B, int H, int N, float scale, float shift, float null_val, double* acc,
                                            void* stream) {
    return eval_metrics_launch<false>("eval_metrics_accumulate", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, scale, shift, null_val,
                                      acc, stream);
}

extern "C" int step_eval_metrics_accumulate_nodes(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh,
                                                  long r_sn, int B, int H, int N, const float* scale_n, const float* shift_n, float null_val,
                                                  double* acc, void* stream) {
    return eval_metrics_launch<true>("eval_metrics_accumulate_nodes", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, scale_n, shift_n,
                                     null_val, acc, stream);
}

extern "C" int step_eval_metrics_finish(const double* acc, int H, double* out, void* stream) {
    STEP_REQUIRE(acc && out, "eval_metrics_finish: NULL acc or out");
    STEP_REQUIRE(H > 0 && H <= EM_MAX_H, "eval_metrics_finish: H = %d is not in 1..%d", H, EM_MAX_H);
    eval_metrics_finish_kernel<<<1, 128, 0, (hipStream_t)stream>>>(acc, H, out);
    STEP_LAUNCH_CHECK("eval_metrics_finish");
    return STEP_OK;
}
