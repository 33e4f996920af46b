// The pooled step-size recursion of MCMC.model_mh / gp_mh(chains=M, adapt=) (include/cesx.h, cesx_mh_adapt_*): one launch
// of one workgroup behind every accept of an armed handle.  The ADAPT instantiation of hm_accept_kernel (kernels_hmc.hip) has
// left alpha[j], chain j's acceptance probability of adaptation step t; here
//     abar_t        = (1 / M) sum_j alpha[j]                       fp64, a fixed order, no atomics:
//                     thread k sums alpha[k], alpha[k + T], ... ascending (AD_BATCH loads in flight, added in their order),
//                     the T partials go through LDS, thread g < AD_GROUPS adds the partials g T / AD_GROUPS .. in thread
//                     order and thread 0 the AD_GROUPS group sums in order
//     log e_{t+1}   = log e_t + (gain / sqrt(t)) (abar_t - target)
//     log ebar_t    = t^-kappa log e_{t+1} + (1 - t^-kappa) log ebar_{t-1},      log ebar_0 = 0
// state = {e, log e, log ebar, t}: the next step's kernels read e = state[0] (stream order hands it over; nothing crosses to
// the host before cesx_mh_adapt_read).  hist row t - 1 = (e_t, abar_t): the multiplier step t ran with and what it accepted.
// A launch past the last row (t > n_steps) writes nothing; the entry points refuse it before it is made.
// One workgroup is latency-bound, not bandwidth-bound: 65 536 chains are 64 values per thread, 8 rounds of 8 loads.
#include "cesx_internal.h"

namespace cesx {

constexpr int AD_THREADS = 1024;
constexpr int AD_GROUPS = 32;                       // the second level: 32 threads add 32 partials each
constexpr int AD_BATCH = 8;

__global__ __launch_bounds__(AD_THREADS)
void ad_update_kernel(const double* __restrict__ alpha, long long M, double* __restrict__ state, double* __restrict__ hist,
                      int n_steps, double target, double gain, double kappa) {
    __shared__ double part[AD_THREADS];
    __shared__ double group[AD_GROUPS];
    const int k = threadIdx.x;
    double acc = 0.0;
    long long j = k;
    for (; j + (long long)(AD_BATCH - 1) * AD_THREADS < M; j += (long long)AD_BATCH * AD_THREADS) {
        double v[AD_BATCH];
#pragma unroll
        for (int b = 0; b < AD_BATCH; ++b) v[b] = alpha[j + (long long)b * AD_THREADS];
#pragma unroll
        for (int b = 0; b < AD_BATCH; ++b) acc += v[b];
    }
    for (; j < M; j += AD_THREADS) acc += alpha[j];
    part[k] = acc;
    __syncthreads();
    if (k < AD_GROUPS) {
        double g = 0.0;
        for (int i = 0; i < AD_THREADS / AD_GROUPS; ++i) g += part[k * (AD_THREADS / AD_GROUPS) + i];
        group[k] = g;
    }
    __syncthreads();
    if (k != 0) return;
    const int t = (int)state[3] + 1;
    if (t > n_steps) return;
    double sum = 0.0;
    for (int i = 0; i < AD_GROUPS; ++i) sum += group[i];
    const double abar = sum / (double)M;
    const double e = state[0];
    const double loge = state[1] + gain / sqrt((double)t) * (abar - target);
    const double w = pow((double)t, -kappa);
    hist[2 * (size_t)(t - 1)] = e;
    hist[2 * (size_t)(t - 1) + 1] = abar;
    state[0] = exp(loge);
    state[1] = loge;
    state[2] = w * loge + (1.0 - w) * state[2];
    state[3] = (double)t;
}

// the recursion of the step whose accept has just been launched on s (mh.ad_alpha is that launch's)
int launch_adapt_update(Engine& e, hipStream_t s) {
    hipLaunchKernelGGL(ad_update_kernel, dim3(1), dim3(AD_THREADS), 0, s, (const double*)e.mh.ad_alpha.get(), (long long)e.J,
                       e.mh.ad_state.get(), e.mh.ad_hist.get(), e.mh.ad_n, e.mh.ad_target, e.mh.ad_gain, e.mh.ad_kappa);
    CESX_HIP(hipGetLastError());
    return CESX_OK;
}

}  // namespace cesx
