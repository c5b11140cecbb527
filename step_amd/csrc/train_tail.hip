// The tail of one training iteration (include/step_hip.h, "training tail"): step_loss on the first k horizon steps of the RESCALED
// prediction and label, both of its gradients, and the three training meters (masked MAE / RMSE / MAPE), in two launches straight from
// the model's NORMALISED [B, H, N] prediction and channel 0 of the batch's [B, H, N, C] future tensor -- what the reference's runner
// does with two rescales, two [:, :k] slices, step_loss, three metric functions and their autograd nodes
// (basicts/runners/base_tsf_runner.py:237-254 with curriculum learning, :170-190; step/step_loss/step_loss.py:5-16;
// basicts/metrics/{mae,rmse,mape}.py).
//
// Work buffer (f64, zeroed by the caller ONCE, then owned by the calls of one stream):
//   [0, 6)    sums of the even calls   {S_abs, S_sq, cnt, S_ape, cnt0, S_bce}
//   [6, 12)   sums of the odd calls
//   12        index of the NEXT call (an unsigned 64-bit integer in the slot): written by a finish launch, read by the next reduce launch
//   13        index of the CURRENT call: written by a reduce launch, read by its finish launch
// Call n adds into half n & 1; its finish launch reads that half and clears the other one for call n + 1, so no memset is queued.
// Inside a launch the workgroups meet only in the atomic adds; whatever reads a sum or an index does so in a LATER launch of the same
// stream, and no word is both written and read inside one launch.
#include "common.h"
#include <limits.h>

namespace {

constexpr int TT_THREADS = 256;          // four waves per workgroup
constexpr int TT_WAVES = TT_THREADS / 64;
constexpr int TT_MAX_H = 64;
constexpr int TT_SUMS = 6;
constexpr int TT_NEXT = 2 * TT_SUMS, TT_CUR = 2 * TT_SUMS + 1;
constexpr long TT_WORK_DOUBLES = 2 * TT_SUMS + 2;

struct TailArgs {
    const float* pred; long p_sb, p_sh, p_sn;
    const float* real; long r_sb, r_sh, r_sn;
    int B, H, N, k;
    float scale, shift, null_val;
    const float* theta; const float* prior; long n_adj;
    double* work;
};

// The rescaling must round twice, like torch's `x * std + mean`: a label ONE float32 step across the 5e-5 / 1e-4 thresholds changes its
// mask (csrc/eval_metrics.hip has the whole story).  Contraction is off in every function that rescales, and the arithmetic is written
// with plain operators.
struct TailElem { float p, y; bool m; };
__device__ __forceinline__ TailElem tail_elem(const TailArgs& a, long b, long h, long n) {
#pragma clang fp contract(off)
    TailElem e;
    e.p = a.pred[b * a.p_sb + h * a.p_sh + n * a.p_sn] * a.scale + a.shift;
    e.y = a.real[b * a.r_sb + h * a.r_sh + n * a.r_sn] * a.scale + a.shift;
    e.m = !(fabsf(e.y - a.null_val) <= 5e-5f);          // mae.py:17-21: ~isclose(y, null, atol = 5e-5, rtol = 0); a NaN label counts
    return e;
}

// Launch 1.  Grid-stride over the B * k * N included elements (consecutive lanes read consecutive n) and over the n_adj edges; f32 terms
// as the reference computes them, summed in f64: per lane, over the wave by shuffles, over the four waves through LDS, then one atomic
// add per sum per workgroup.
__global__ __launch_bounds__(TT_THREADS) void train_tail_reduce_kernel(TailArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[TT_WAVES][TT_SUMS];
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_NEXT];
    double s[TT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned kn = (unsigned)a.k * a.N;          // (B * H * N < 2^31: 32-bit divisions)
    const long n1 = (long)a.B * kn;
    for (long i = first; i < n1; i += stride) {
        const unsigned b = (unsigned)i / kn, r = (unsigned)i - b * kn, h = r / (unsigned)a.N, n = r - h * (unsigned)a.N;
        const TailElem e = tail_elem(a, b, h, n);
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
    for (long i = first; i < a.n_adj; i += stride) {
        const float t = a.theta[i], y = a.prior[i];
        const float l1 = fmaxf(logf(t), -100.f), l0 = fmaxf(logf(1.f - t), -100.f);      // torch's BCELoss clamps the logs at -100
        s[5] -= (double)(y * l1 + (1.f - y) * l0);
    }
#pragma unroll
    for (int j = 0; j < TT_SUMS; ++j)
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < TT_SUMS; ++j) red[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
    if (threadIdx.x < TT_SUMS) {
        const int j = threadIdx.x;
        atomicAdd(a.work + (call & 1) * TT_SUMS + j, red[0][j] + red[1][j] + red[2][j] + red[3][j]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(a.work)[TT_CUR] = call;
}

// Launch 2.  Every workgroup reads the finished sums; block 0 writes the loss and the metrics, clears the other half and advances the call
// index; all of them write dpred over the FULL [B, H, N] (exact zeros on excluded horizons, masked labels and NaN terms) and dtheta.
__global__ __launch_bounds__(TT_THREADS) void train_tail_finish_kernel(TailArgs a, float coef, float* __restrict__ loss,
                                                                       float* __restrict__ metrics, float* __restrict__ dpred,
                                                                       float* __restrict__ dtheta) {
#pragma clang fp contract(off)
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_CUR];
    const double* sum = a.work + (call & 1) * TT_SUMS;
    const double cnt = sum[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double cnt0 = sum[4];
        const float mae = cnt > 0.0 ? (float)(sum[0] / cnt) : 0.f;
        *loss = mae + coef * (float)(sum[5] / (double)a.n_adj);
        metrics[0] = mae;
        metrics[1] = cnt > 0.0 ? (float)sqrt(sum[1] / cnt) : 0.f;
        metrics[2] = cnt0 > 0.0 ? (float)(sum[3] / cnt0) : 0.f;
        double* other = a.work + ((call + 1) & 1) * TT_SUMS;
        for (int j = 0; j < TT_SUMS; ++j) other[j] = 0.0;
        reinterpret_cast<unsigned long long*>(a.work)[TT_NEXT] = call + 1;
    }
    const float g = cnt > 0.0 ? (float)(1.0 / cnt) * a.scale : 0.f;      // d/d pred of the mean on pred * scale + shift
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned hn = (unsigned)a.H * a.N;
    const long n_all = (long)a.B * hn;
    for (long i = first; i < n_all; i += stride) {
        const unsigned b = (unsigned)i / hn, r = (unsigned)i - b * hn, h = r / (unsigned)a.N, n = r - h * (unsigned)a.N;
        float v = 0.f;
        if (h < (unsigned)a.k) {
            const TailElem e = tail_elem(a, b, h, n);
            const float d = e.p - e.y;                                   // a NaN difference compares false twice: gradient 0
            if (e.m) v = d > 0.f ? g : (d < 0.f ? -g : 0.f);
        }
        dpred[i] = v;
    }
    const float sc = coef / (float)a.n_adj;
    for (long i = first; i < a.n_adj; i += stride) {
        const float t = a.theta[i], y = a.prior[i];
        dtheta[i] = sc * (t - y) / fmaxf(t * (1.f - t), 1e-12f);         // d/dt of -(y log t + (1 - y) log(1 - t)), torch's denominator floor
    }
}

}  // namespace

extern "C" long step_train_tail_work_doubles(void) { return TT_WORK_DOUBLES; }

extern "C" int step_train_tail(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn, int B,
                               int H, int N, int k, float scale, float shift, float null_val, const float* theta, const float* prior,
                               long n_adj, float coef, double* work, float* loss, float* metrics, float* dpred, float* dtheta,
                               void* stream) {
    STEP_REQUIRE(pred && real && theta && prior && work && loss && metrics && dpred && dtheta, "train_tail: NULL buffer");
    STEP_REQUIRE(B > 0 && N > 0 && n_adj > 0, "train_tail: B = %d, N = %d, n_adj = %ld must all be positive", B, N, n_adj);
    STEP_REQUIRE(k >= 1 && k <= H && H <= TT_MAX_H, "train_tail: need 1 <= k <= H <= %d (k = %d, H = %d)", TT_MAX_H, k, H);
    STEP_REQUIRE(p_sb > 0 && p_sh > 0 && p_sn > 0 && r_sb > 0 && r_sh > 0 && r_sn > 0,
                 "train_tail: element strides must be positive (pred %ld, %ld, %ld; real %ld, %ld, %ld)", p_sb, p_sh, p_sn, r_sb, r_sh, r_sn);
    STEP_REQUIRE((long)B * H * N <= INT_MAX, "train_tail: B * H * N = %ld exceeds the %d elements of one call", (long)B * H * N, INT_MAX);
    STEP_REQUIRE(null_val == null_val, "train_tail: null_val must be finite");
    TailArgs a;
    a.pred = pred; a.p_sb = p_sb; a.p_sh = p_sh; a.p_sn = p_sn;
    a.real = real; a.r_sb = r_sb; a.r_sh = r_sh; a.r_sn = r_sn;
    a.B = B; a.H = H; a.N = N; a.k = k;
    a.scale = scale; a.shift = shift; a.null_val = null_val;
    a.theta = theta; a.prior = prior; a.n_adj = n_adj;
    a.work = work;
    const long n_inc = (long)B * k * N, n_all = (long)B * H * N;
    // six f64 atomics per workgroup onto six addresses: at least four elements per thread where there are that many
    const long rmax = n_inc > n_adj ? n_inc : n_adj;
    int rblocks = (int)(rmax / (4 * TT_THREADS));
    rblocks = rblocks < 1 ? 1 : (rblocks > 256 ? 256 : rblocks);
    const long fmax = n_all > n_adj ? n_all : n_adj;
    int fblocks = cdiv(fmax, TT_THREADS);
    if (fblocks > 1024) fblocks = 1024;
    train_tail_reduce_kernel<<<rblocks, TT_THREADS, 0, (hipStream_t)stream>>>(a);
    STEP_LAUNCH_CHECK("train_tail_reduce");
    train_tail_finish_kernel<<<fblocks, TT_THREADS, 0, (hipStream_t)stream>>>(a, coef, loss, metrics, dpred, dtheta);
    STEP_LAUNCH_CHECK("train_tail_finish");
    return STEP_OK;
}
