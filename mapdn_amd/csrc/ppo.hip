// ppo.hip — the PPO half of MAPPO / IPPO's update (learning_algorithms/ppo.py:39-70), gfx950 (MI355X).
//
// The reference computes the generalised advantage estimate with a Python loop over the rows of the batch (ppo.py:46-54) and both
// clipped losses as ~40 one-line elementwise launches over [rows, n] (ppo.py:39, 56-70).  Here:
//   k_ppo_gae          the recurrence  adv[i] = delta[i] + gamma lambda mask[i] adv[succ(i)]  over chains of stride S (succ(i) = i + S: with
//                      the replay ring's (step, env) row order and S = the env count a chain is ONE env's time series; S = 1 is the
//                      reference's row-by-row walk).  One thread per (chain, agent) column walks its chain newest to oldest with the
//                      running advantage in a register; the threads of a wavefront read consecutive floats of one row at every step.
//   k_ppo_policy_loss  -sum w min(rho A, clamp(rho, 1 -/+ eps) A) and d/d mean of it, rho = exp(log_prob_new - log_prob_old);
//   k_ppo_value_loss   coef sum w max((V - R)^2, (V_clip - R)^2) and d/d V of it, R = r + gamma (1 - done) V(next);
//   k_ppo_loss_finish  the per-workgroup partial sums of either loss added in a fixed order by one workgroup (no floating-point atomics:
//                      the same input gives the same bits), times the weight normalisation.
// Each kernel writes out the f32 operations of the PyTorch expressions in their order without contraction, so that the only differences
// to the PyTorch route are expf / logf and the order of the loss sum.  The gradients are those autograd gives, ties included:
// torch.min / torch.max hand half of the incoming gradient to either operand where they are equal, clamp passes it on its bounds.
// All of it is bandwidth- and latency-bound f32 streaming: no LDS beyond the four partial sums of a workgroup, no matrix cores.
// Compiled inside capi.hip (which holds the C entry points and their argument checks); a file of its own, so that the kernel sets the
// tests parse from rollout.hip, critic*.hip and policy*.hip are what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mapdn.h"

namespace mapdn {

constexpr int PPO_NT = 256;                // threads of every launch here: four wavefronts
constexpr int PPO_BLOCKS_PER_CU = 8;       // 8 x 256 threads = the 32 wavefronts a CU holds

// sum over the 256 threads of a workgroup in a fixed order: shuffles within each 64-lane wavefront, then the four wavefront sums
// through LDS, (0 + 1) + (2 + 3); every thread returns the total
__device__ __forceinline__ float ppo_block_sum(float v, float* s4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// column j = c n + i (chain c < min(S, rows), agent i): rows c, c + S, c + 2 S, ... newest first.  mask = 1 - done on a last_step row,
// 1 elsewhere (ppo.py:48-51); delta = r + gamma V' mask - V (ppo.py:52); adv = delta + gamma lambda adv_next mask (ppo.py:53).
__global__ void __launch_bounds__(PPO_NT)
k_ppo_gae(const float* __restrict__ reward, const float* __restrict__ value, const float* __restrict__ next_value,
          const float* __restrict__ done, const float* __restrict__ last_step, float* __restrict__ adv, long rows, int n, long S, long cols,
          float gamma, float gl) {
#pragma clang fp contract(off)      // every PyTorch op of the recurrence rounds on its own (see k_explore, csrc/rollout.hip)
  const long T = (rows + S - 1) / S;
  for (long j = (long)blockIdx.x * PPO_NT + threadIdx.x; j < cols; j += (long)gridDim.x * PPO_NT) {
    const long c = j / n;
    float last = 0.0f;
    for (long t = T - 1; t >= 0; --t) {
      const long row = t * S + c;
      if (row >= rows) continue;                     // the ragged end: this chain is one row shorter
      const long idx = t * S * n + j;                // == row * n + i
      const float mask = last_step[row] != 0.0f ? 1.0f - done[row] : 1.0f;
      const float gv = gamma * next_value[idx];
      const float gvm = gv * mask;
      const float rg = reward[idx] + gvm;
      const float delta = rg - value[idx];
      const float ga = gl * last;
      const float gam = ga * mask;
      last = delta + gam;
      adv[idx] = last;
    }
  }
}

// partial[blockIdx.x] = sum over this workgroup's elements of w min(rho A, clamp(rho) A);  dmean[e] = d loss / d mean[e] with
// loss = -scale[0] * (sum of all partials).  log_prob of the action under N(mean, exp(log_std)) as torch.distributions.Normal writes it.
__global__ void __launch_bounds__(PPO_NT)
k_ppo_policy_loss(const float* __restrict__ action, const float* __restrict__ mean, const float* __restrict__ log_std,
                  const float* __restrict__ avail, const float* __restrict__ old_lp, const float* __restrict__ adv,
                  const float* __restrict__ valid, const float* __restrict__ scale, float lo, float hi, float* __restrict__ dmean,
                  float* __restrict__ partial, long elems, int n) {
#pragma clang fp contract(off)
  __shared__ float s4[4];
  const float sc = scale[0];
  float acc = 0.0f;
  for (long e = (long)blockIdx.x * PPO_NT + threadIdx.x; e < elems; e += (long)gridDim.x * PPO_NT) {
    const float w = valid ? valid[e / n] : 1.0f;
    const float sd = expf(log_std[e]);
    const float var = sd * sd;
    const float d = action[e] - mean[e];
    const float q = (d * d) / (2.0f * var);
    const float lp = (-q - logf(sd)) - 0.91893853320467274f;                  // log(sqrt(2 pi))
    const float m = (avail && avail[e] == 0.0f) ? 0.0f : 1.0f;               // restore mask (ppo.py:31-33)
    const float rho = expf(m * lp - m * old_lp[e]);
    const float A = adv[e];
    const float s1 = rho * A;
    const float rc = rho < lo ? lo : (rho > hi ? hi : rho);
    const float s2 = rc * A;
    const float term = (s1 < s2 || s1 != s1) ? s1 : s2;                       // torch.min (a NaN wins)
    acc += w * term;
    const float g1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);               // torch.min's backward: the smaller operand, halves at a tie
    const float g2 = s2 < s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float pass = (rho >= lo && rho <= hi) ? 1.0f : 0.0f;                // clamp's backward: bounds included
    const float dterm = g1 * A + (g2 * pass) * A;                             // d term / d rho
    const float dlp = dterm * rho * m;                                        // d term / d log_prob_new
    dmean[e] = -(sc * w) * (dlp * (d / var));
  }
  const float tot = ppo_block_sum(acc, s4);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// partial[blockIdx.x] = sum over this workgroup's elements of w max((V - R)^2, (V_clip - R)^2);  dv[e] = d loss / d V[e] with
// loss = coef * scale[0] * (sum of all partials); R = r + gamma (1 - done) V_next (ppo.py:56), V_clip = V_old + clamp(V - V_old, -/+ eps)
__global__ void __launch_bounds__(PPO_NT)
k_ppo_value_loss(const float* __restrict__ v, const float* __restrict__ v_old, const float* __restrict__ reward,
                 const float* __restrict__ v_next, const float* __restrict__ done, const float* __restrict__ valid,
                 const float* __restrict__ scale, float gamma, float eps, float coef, float* __restrict__ dv, float* __restrict__ partial,
                 long elems, int n) {
#pragma clang fp contract(off)
  __shared__ float s4[4];
  const float sc = scale[0];
  float acc = 0.0f;
  for (long e = (long)blockIdx.x * PPO_NT + threadIdx.x; e < elems; e += (long)gridDim.x * PPO_NT) {
    const long row = e / n;
    const float w = valid ? valid[row] : 1.0f;
    const float gnd = gamma * (1.0f - done[row]);
    const float R = reward[e] + gnd * v_next[e];
    const float V = v[e], Vo = v_old[e];
    const float df = V - Vo;
    const float cl = df < -eps ? -eps : (df > eps ? eps : df);
    const float Vc = Vo + cl;
    const float e1 = V - R, e2 = Vc - R;
    const float s1 = e1 * e1, s2 = e2 * e2;
    const float term = (s1 > s2 || s1 != s1) ? s1 : s2;                       // torch.max (a NaN wins)
    acc += w * term;
    const float g1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float g2 = s2 > s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float pass = (df >= -eps && df <= eps) ? 1.0f : 0.0f;
    const float dterm = g1 * (2.0f * e1) + (g2 * pass) * (2.0f * e2);
    dv[e] = (coef * sc * w) * dterm;
  }
  const float tot = ppo_block_sum(acc, s4);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// loss[0] = mult * scale[0] * sum_b partial[b]: thread t adds partial[t], partial[t + 256], ... in that order, then the workgroup sum
__global__ void __launch_bounds__(PPO_NT)
k_ppo_loss_finish(const float* __restrict__ partial, int nb, const float* __restrict__ scale, float mult, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ float s4[4];
  float acc = 0.0f;
  for (int b = threadIdx.x; b < nb; b += PPO_NT) acc += partial[b];
  const float tot = ppo_block_sum(acc, s4);
  if (threadIdx.x == 0) loss[0] = mult * (tot * scale[0]);
}

static int ppo_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus > 0 ? cus : 256;
}

// workgroups of a launch over `units` threads' worth of work: one thread each up to a full machine (8 workgroups per CU), grid-stride beyond
static int ppo_blocks(int64_t units, int cus) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((units + PPO_NT - 1) / PPO_NT, (int64_t)(cus ? cus : ppo_cus()) * PPO_BLOCKS_PER_CU));
}

// workgroups (= per-workgroup partial sums) of a loss launch over `elems` elements; cus = 0: the current device's CU count
static int ppo_loss_blocks(int64_t elems, int cus = 0) { return ppo_blocks(elems, cus); }

// the launchers return MAPDN_OK / MAPDN_E_HIP; the arguments were checked by the entry points (capi.hip)

static int launch_ppo_gae(const float* reward, const float* value, const float* next_value, const float* done, const float* last_step, float* adv,
                   int64_t rows, int32_t n, int64_t stride, float gamma, float gamma_lambda, hipStream_t st) {
  const int64_t cols = std::min<int64_t>(stride, rows) * n;          // chains c >= rows have no row
  const int blocks = ppo_blocks(cols, 0);
  hipLaunchKernelGGL(k_ppo_gae, dim3(blocks), dim3(PPO_NT), 0, st, reward, value, next_value, done, last_step, adv, (long)rows, (int)n, (long)stride,
                     (long)cols, gamma, gamma_lambda);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

static int launch_ppo_policy_loss(const float* action, const float* mean, const float* log_std, const float* avail, const float* old_log_prob,
                           const float* adv, const float* valid, const float* scale, float clip_lo, float clip_hi, float* loss, float* dmean,
                           float* partial, int64_t rows, int32_t n, hipStream_t st) {
  const int64_t elems = rows * n;
  const int blocks = ppo_blocks(elems, 0);
  hipLaunchKernelGGL(k_ppo_policy_loss, dim3(blocks), dim3(PPO_NT), 0, st, action, mean, log_std, avail, old_log_prob, adv, valid, scale, clip_lo,
                     clip_hi, dmean, partial, (long)elems, (int)n);
  hipLaunchKernelGGL(k_ppo_loss_finish, dim3(1), dim3(PPO_NT), 0, st, partial, blocks, scale, -1.0f, loss);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

static int launch_ppo_value_loss(const float* v, const float* v_old, const float* reward, const float* v_next, const float* done, const float* valid,
                          const float* scale, float gamma, float eps, float coef, float* loss, float* dv, float* partial, int64_t rows,
                          int32_t n, hipStream_t st) {
  const int64_t elems = rows * n;
  const int blocks = ppo_blocks(elems, 0);
  hipLaunchKernelGGL(k_ppo_value_loss, dim3(blocks), dim3(PPO_NT), 0, st, v, v_old, reward, v_next, done, valid, scale, gamma, eps, coef, dv, partial,
                     (long)elems, (int)n);
  hipLaunchKernelGGL(k_ppo_loss_finish, dim3(1), dim3(PPO_NT), 0, st, partial, blocks, scale, coef, loss);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

}  // namespace mapdn
