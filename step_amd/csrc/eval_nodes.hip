// Per-sensor tables of a validation / test pass and its predictions in data units (include/step_hip.h, "per-node evaluation
// metrics"): the five sums of csrc/eval_metrics.hip kept per (horizon, node) instead of per horizon, and the rescaled prediction of
// every element stored next to them.  One launch per batch beside step_eval_metrics_accumulate, one small launch per pass.
//
// Table (f64 [5, H, N], zeroed by the caller once per pass): sum k of {S_abs, S_sq, cnt, S_ape, cnt0} of (h, n) at (k * H + h) * N + n,
// so that the lanes of a wave (consecutive n) touch consecutive doubles of each of the five planes.
// A slot is written by ONE thread of a launch (plain load, add, store: no atomics), so launches on one table must be ordered by their
// stream -- the contract csrc/eval_metrics.hip already has -- and the sums do not depend on the grid or on timing.
#include "common.h"
#include <limits.h>
#include <math.h>
#include <type_traits>

namespace {

constexpr int EN_THREADS = 256;          // four waves per workgroup
constexpr int EN_MAX_H = 64;
constexpr int EN_SUMS = 5;
constexpr int EN_FLIGHT = 8;             // windows whose loads are issued before the first of them is used

// NODES = false: one scale and one shift (float); true: f32 [N] of each on the device, read once per thread at its node
template <bool NODES>
struct NodeArgs {
    using Scaler = std::conditional_t<NODES, const float*, float>;
    const float* pred; long p_sb, p_sh, p_sn;
    const float* real; long r_sb, r_sh, r_sn;
    int B, H, N;
    Scaler scale, shift;
    float null_val;
    int null_is_nan;
    double* table;          // may be NULL: the export alone (real is then not read)
    float* out;             // may be NULL: the sums alone
};

__device__ __forceinline__ double metric_of(double sum, double cnt) { return cnt > 0.0 ? sum / cnt : 0.0; }

// grid (cdiv(N, 256), H).  Thread n of workgroup (c, h) owns element column (h, c * 256 + n) and walks its B windows: consecutive lanes
// read consecutive n of a prediction row (the label is one channel of [.., N, C]).  The walk is a chain of dependent load latencies
// B = 8..64 long and nothing else, so the loads of EN_FLIGHT windows are issued before the first term is taken (rows behind the last
// window re-read the last one and are not used).  The terms are eval_metrics_kernel's, restated: f32 as the reference computes them,
// summed in f64 per thread.
template <bool NODES>
__global__ __launch_bounds__(EN_THREADS) void eval_node_metrics_kernel(NodeArgs<NODES> a) {
    // two roundings in the rescaling, like torch's `x * std + mean`: see eval_metrics_kernel (csrc/eval_metrics.hip) -- a label one
    // float32 step across the 5e-5 / 1e-4 thresholds changes its mask, and the export is compared with torch bit for bit
#pragma clang fp contract(off)
    const int n = blockIdx.x * EN_THREADS + threadIdx.x, h = blockIdx.y;
    if (n >= a.N) return;
    float scale, shift;
    if constexpr (NODES) { scale = a.scale[n]; shift = a.shift[n]; } else { scale = a.scale; shift = a.shift; }
    const bool sums = a.table != nullptr;          // (the same in every thread of the launch)
    const float* pred = a.pred + (long)h * a.p_sh + (long)n * a.p_sn;
    const float* real = sums ? a.real + (long)h * a.r_sh + (long)n * a.r_sn : nullptr;
    float* out = a.out ? a.out + (long)h * a.N + n : nullptr;
    const long out_sb = (long)a.H * a.N;
    double s[EN_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b0 = 0; b0 < a.B; b0 += EN_FLIGHT) {
        float pv[EN_FLIGHT], yv[EN_FLIGHT];
#pragma unroll
        for (int j = 0; j < EN_FLIGHT; ++j) {
            const int b = b0 + j < a.B ? b0 + j : a.B - 1;
            pv[j] = pred[(long)b * a.p_sb];
            yv[j] = sums ? real[(long)b * a.r_sb] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < EN_FLIGHT; ++j) {
            if (b0 + j >= a.B) break;
            const float p = pv[j] * scale + shift;
            if (out) out[(long)(b0 + j) * out_sb] = p;
            if (!sums) continue;
            const float y = yv[j] * scale + shift;
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
    }
    if (!sums) return;
    double* slot = a.table + (long)h * a.N + n;          // the only writer of these five slots in this launch
    const long plane = (long)a.H * a.N;
#pragma unroll
    for (int k = 0; k < EN_SUMS; ++k) slot[k * plane] += s[k];
}

// grid cdiv(N, 256): thread n the three metrics of node n at every horizon (rows 0 .. H - 1 of out [H + 1, N, 3]) and, from its sums
// added over the horizons, over all of them (row H)
__global__ __launch_bounds__(EN_THREADS) void eval_node_metrics_finish_kernel(const double* __restrict__ table, int H, int N,
                                                                              double* __restrict__ out) {
    const int n = blockIdx.x * EN_THREADS + threadIdx.x;
    if (n >= N) return;
    const long plane = (long)H * N;
    double all[EN_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int h = 0; h <= H; ++h) {
        double c[EN_SUMS];
        for (int k = 0; k < EN_SUMS; ++k) {
            c[k] = h < H ? table[k * plane + (long)h * N + n] : all[k];
            all[k] += h < H ? c[k] : 0.0;
        }
        double* o = out + ((long)h * N + n) * 3;
        o[0] = metric_of(c[0], c[2]);
        o[1] = sqrt(metric_of(c[1], c[2]));
        o[2] = metric_of(c[3], c[4]);
    }
}

template <bool NODES>
int eval_nodes_launch(const char* op, const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh, long r_sn,
                      int B, int H, int N, typename NodeArgs<NODES>::Scaler scale, typename NodeArgs<NODES>::Scaler shift, float null_val,
                      double* table, float* out, void* stream) {
    STEP_REQUIRE(pred && real, "%s: NULL pred or real", op);
    STEP_REQUIRE(table || out, "%s: NULL table and NULL out: nothing to do", op);
    if constexpr (NODES) STEP_REQUIRE(scale && shift, "%s: NULL scale_n or shift_n", op);
    STEP_REQUIRE(B > 0 && H > 0 && N > 0, "%s: B = %d, H = %d, N = %d must all be positive", op, B, H, N);
    STEP_REQUIRE(H <= EN_MAX_H, "%s: H = %d exceeds the %d horizons of one table", op, H, EN_MAX_H);
    STEP_REQUIRE(p_sb > 0 && p_sh > 0 && p_sn > 0 && r_sb > 0 && r_sh > 0 && r_sn > 0,
                 "%s: element strides must be positive (pred %ld, %ld, %ld; real %ld, %ld, %ld)", op, p_sb, p_sh, p_sn, r_sb, r_sh, r_sn);
    STEP_REQUIRE((long)B * N <= INT_MAX, "%s: B * N = %ld exceeds the %d elements per horizon of one launch", op, (long)B * N, INT_MAX);
    STEP_REQUIRE(!isinf(null_val), "%s: null_val must not be infinite", op);
    NodeArgs<NODES> a;
    a.pred = pred; a.p_sb = p_sb; a.p_sh = p_sh; a.p_sn = p_sn;
    a.real = real; a.r_sb = r_sb; a.r_sh = r_sh; a.r_sn = r_sn;
    a.B = B; a.H = H; a.N = N;
    a.scale = scale; a.shift = shift; a.null_val = null_val; a.null_is_nan = null_val != null_val;
    a.table = table; a.out = out;
    eval_node_metrics_kernel<NODES><<<dim3(cdiv(N, EN_THREADS), H), EN_THREADS, 0, (hipStream_t)stream>>>(a);
    STEP_LAUNCH_CHECK(op);
    return STEP_OK;
}

}  // namespace

extern "C" long step_eval_node_table_doubles(int H, int N) { return H < 1 || H > EN_MAX_H || N < 1 ? 0 : (long)EN_SUMS * H * N; }

extern "C" int step_eval_node_metrics_accumulate(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb, long r_sh,
                                                 long r_sn, int B, int H, int N, float scale, float shift, float null_val, double* table,
                                                 float* out, void* stream) {
    return eval_nodes_launch<false>("eval_node_metrics_accumulate", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, scale, shift,
                                    null_val, table, out, stream);
}

extern "C" int step_eval_node_metrics_accumulate_nodes(const float* pred, long p_sb, long p_sh, long p_sn, const float* real, long r_sb,
                                                       long r_sh, long r_sn, int B, int H, int N, const float* scale_n, const float* shift_n,
                                                       float null_val, double* table, float* out, void* stream) {
    return eval_nodes_launch<true>("eval_node_metrics_accumulate_nodes", pred, p_sb, p_sh, p_sn, real, r_sb, r_sh, r_sn, B, H, N, scale_n,
                                   shift_n, null_val, table, out, stream);
}

extern "C" int step_eval_node_metrics_finish(const double* table, int H, int N, double* out, void* stream) {
    STEP_REQUIRE(table && out, "eval_node_metrics_finish: NULL table or out");
    STEP_REQUIRE(H > 0 && H <= EN_MAX_H && N > 0, "eval_node_metrics_finish: H = %d is not in 1..%d or N = %d is not positive", H, EN_MAX_H, N);
    eval_node_metrics_finish_kernel<<<cdiv(N, EN_THREADS), EN_THREADS, 0, (hipStream_t)stream>>>(table, H, N, out);
    STEP_LAUNCH_CHECK("eval_node_metrics_finish");
    return STEP_OK;
}
