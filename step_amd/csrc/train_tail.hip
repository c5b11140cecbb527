// The tail of one training iteration (include/step_hip.h, "training tail"): step_loss on the first k horizon steps of the RESCALED
// prediction and label, both of its gradients, and the three training meters (masked MAE / RMSE / MAPE), in two launches straight from
// the model's NORMALISED [B, H, N] prediction and channel 0 of the batch's [B, H, N, C] future tensor -- what the reference's runner
// does with two rescales, two [:, :k] slices, step_loss, three metric functions and their autograd nodes
// (basicts/runners/base_tsf_runner.py:237-254 with curriculum learning, :170-190; step/step_loss/step_loss.py:5-16;
// basicts/metrics/{mae,rmse,mape}.py).
//
// The work buffer and the device helpers are those of csrc/tail_device.h.
#include "tail_device.h"
#include <limits.h>
#include <cmath>
#include <type_traits>

namespace {

constexpr int TT_MAX_H = 64;

// NODES = false: one scale and one shift (float); true: f32 [N] of each on the device, read at the element's node.  The two forms are
// separate instantiations of the kernels below, and so are a finite and a NaN null_val (NAN_NULL): nothing is chosen per element.
template <bool NODES>
struct TailArgs {
    using Scaler = std::conditional_t<NODES, const float*, float>;
    const float* pred; long p_sb, p_sh, p_sn;
    const float* real; long r_sb, r_sh, r_sn;
    int B, H, N, k;
    Scaler scale, shift;
    float null_val;
    const float* theta; const float* prior; long n_adj;
    double* work;
};

template <bool NODES>
__device__ __forceinline__ float scale_at(const TailArgs<NODES>& a, long n) {
    if constexpr (NODES) return a.scale[n]; else return a.scale;
}

template <bool NODES, bool NAN_NULL>
__device__ __forceinline__ TailElem tail_elem(const TailArgs<NODES>& a, long b, long h, long n) {
    float shift;
    if constexpr (NODES) shift = a.shift[n]; else shift = a.shift;
    return tail_rescale_null<NAN_NULL>(a.pred[b * a.p_sb + h * a.p_sh + n * a.p_sn], a.real[b * a.r_sb + h * a.r_sh + n * a.r_sn],
                                       scale_at(a, n), shift, a.null_val);
}

// Launch 1.  Grid-stride over the B * k * N included elements (consecutive lanes read consecutive n) and over the n_adj edges; f32 terms
// as the reference computes them, summed in f64: per lane, over the wave by shuffles, over the four waves through LDS, then one atomic
// add per sum per workgroup.
template <bool NODES, bool NAN_NULL>
__global__ __launch_bounds__(TT_THREADS) void train_tail_reduce_kernel(TailArgs<NODES> a) {
#pragma clang fp contract(off)
    __shared__ double red[TT_WAVES][TT_SUMS];
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_NEXT];
    double s[TT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned kn = (unsigned)a.k * a.N;          // (B * H * N < 2^31: 32-bit divisions)
    const long n1 = (long)a.B * kn;
    for (long i = first; i < n1; i += stride) {
        const unsigned b = (unsigned)i / kn, r = (unsigned)i - b * kn, h = r / (unsigned)a.N, n = r - h * (unsigned)a.N;
        tail_accumulate(tail_elem<NODES, NAN_NULL>(a, b, h, n), s);
    }
    for (long i = first; i < a.n_adj; i += stride) {
        const float t = a.theta[i], y = a.prior[i];
        const float l1 = fmaxf(logf(t), -100.f), l0 = fmaxf(logf(1.f - t), -100.f);      // torch's BCELoss clamps the logs at -100
        s[5] -= (double)(y * l1 + (1.f - y) * l0);
    }
    tail_block_add(s, red, a.work, call);
}

// Launch 2.  Every workgroup reads the finished sums; block 0 writes the loss and the metrics, clears the other half and advances the call
// index; all of them write dpred over the FULL [B, H, N] (exact zeros on excluded horizons, masked labels and NaN terms) and dtheta.
template <bool NODES, bool NAN_NULL>
__global__ __launch_bounds__(TT_THREADS) void train_tail_finish_kernel(TailArgs<NODES> a, float coef, float* __restrict__ loss,
                                                                       float* __restrict__ metrics, float* __restrict__ dpred,
                                                                       float* __restrict__ dtheta) {
#pragma clang fp contract(off)
    const unsigned long long call = reinterpret_cast<const unsigned long long*>(a.work)[TT_CUR];
    const double* sum = a.work + (call & 1) * TT_SUMS;
    const double cnt = sum[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *loss = tail_finish_values(sum, a.work, call, metrics) + coef * (float)(sum[5] / (double)a.n_adj);
    }
    // d/d pred of the mean on pred * scale + shift: (float)(1 / cnt) * scale, per node the same product with the node's scale
    float g;
    if constexpr (NODES) g = cnt > 0.0 ? (float)(1.0 / cnt) : 0.f;
    else g = cnt > 0.0 ? (float)(1.0 / cnt) * a.scale : 0.f;
    const long stride = (long)gridDim.x * TT_THREADS, first = (long)blockIdx.x * TT_THREADS + threadIdx.x;
    const unsigned hn = (unsigned)a.H * a.N;
    const long n_all = (long)a.B * hn;
    for (long i = first; i < n_all; i += stride) {
        const unsigned b = (unsigned)i / hn, r = (unsigned)i - b * hn, h = r / (unsigned)a.N, n = r - h * (unsigned)a.N;
        float v = 0.f;
        if (h < (unsigned)a.k) {
            if constexpr (NODES) v = tail_sign_grad(tail_elem<NODES, NAN_NULL>(a, b, h, n), g * a.scale[n]);
            else v = tail_sign_grad(tail_elem<NODES, NAN_NULL>(a, b, h, n), g);
        }
        dpred[i] = v;
    }
    const float sc = coef / (float)a.n_adj;
    for (long i = first; i < a.n_adj; i += stride) {
        const float t = a.theta[i], y = a.prior[i];
        dtheta[i] = sc * (t - y) / fmaxf(t * (1.f - t), 1e-12f);         // d/dt of -(y log t + (1 - y) log(1 - t)), torch's denominator floor
    }
}

template <bool NODES>
int train_tail_launch(const char* op, const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn, int B,
                      int H, int N, int k, typename TailArgs<NODES>::Scaler scale, typename TailArgs<NODES>::Scaler shift, float null_val,
                      const float* theta, const float* prior, long n_adj, float coef, double* work, float* loss, float* metrics, float* dpred,
                      float* dtheta, void* stream) {
    STEP_REQUIRE(pred && real && theta && prior && work && loss && metrics && dpred && dtheta, "%s: NULL buffer", op);
    if constexpr (NODES) STEP_REQUIRE(scale && shift, "%s: NULL scale_n or shift_n", op);
    STEP_REQUIRE(B > 0 && N > 0 && n_adj > 0, "%s: B = %d, N = %d, n_adj = %ld must all be positive", op, B, N, n_adj);
    STEP_REQUIRE(k >= 1 && k <= H && H <= TT_MAX_H, "%s: need 1 <= k <= H <= %d (k = %d, H = %d)", op, TT_MAX_H, k, H);
    STEP_REQUIRE(p_sb > 0 && p_sh > 0 && p_sn > 0 && r_sb > 0 && r_sh > 0 && r_sn > 0,
                 "%s: element strides must be positive (pred %ld, %ld, %ld; real %ld, %ld, %ld)", op, p_sb, p_sh, p_sn, r_sb, r_sh, r_sn);
    STEP_REQUIRE((long)B * H * N <= INT_MAX, "%s: B * H * N = %ld exceeds the %d elements of one call", op, (long)B * H * N, INT_MAX);
    STEP_REQUIRE(!std::isinf(null_val), "%s: null_val must be finite or NaN", op);
    TailArgs<NODES> a;
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
    const hipStream_t st = (hipStream_t)stream;
    if (null_val != null_val) {
        train_tail_reduce_kernel<NODES, true><<<rblocks, TT_THREADS, 0, st>>>(a);
        STEP_LAUNCH_CHECK("train_tail_reduce");
        train_tail_finish_kernel<NODES, true><<<fblocks, TT_THREADS, 0, st>>>(a, coef, loss, metrics, dpred, dtheta);
    } else {
        train_tail_reduce_kernel<NODES, false><<<rblocks, TT_THREADS, 0, st>>>(a);
        STEP_LAUNCH_CHECK("train_tail_reduce");
        train_tail_finish_kernel<NODES, false><<<fblocks, TT_THREADS, 0, st>>>(a, coef, loss, metrics, dpred, dtheta);
    }
    STEP_LAUNCH_CHECK("train_tail_finish");
    return STEP_OK;
}

}  // namespace

extern "C" long step_train_tail_work_doubles(void) { return TT_WORK_DOUBLES; }

extern "C" int step_train_tail(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn, int B,
                               int H, int N, int k, float scale, float shift, float null_val, const float* theta, const float* prior,
                               long n_adj, float coef, double* work, float* loss, float* metrics, float* dpred, float* dtheta,
                               void* stream) {
    return train_tail_launch<false>("train_tail", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, k, scale, shift, null_val, theta, prior,
                                    n_adj, coef, work, loss, metrics, dpred, dtheta, stream);
}

extern "C" int step_train_tail_nodes(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn,
                                     int B, int H, int N, int k, const float* scale_n, const float* shift_n, float null_val,
                                     const float* theta, const float* prior, long n_adj, float coef, double* work, float* loss,
                                     float* metrics, float* dpred, float* dtheta, void* stream) {
    return train_tail_launch<true>("train_tail_nodes", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, k, scale_n, shift_n, null_val, theta,
                                   prior, n_adj, coef, work, loss, metrics, dpred, dtheta, stream);
}
