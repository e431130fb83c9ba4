// critic_cf.hip — COMA's counterfactual baseline as ONE launch, gfx950 (MI355X).  Compiled inside critic.hip (its layouts and load_row; the
// head itself is head_value of headtile.hpp: this file has the sampled rows and the mean over them).
//
// Reference: models/coma.py:139-151 — for every transition and agent i the critic is valued sample_size more times with agent i's
// action replaced by a draw from N(mean_i, std), on a [S b, n, (n + 1) o + n + n a] input, and the S values are averaged.  The first
// layer is linear in the actions, so with one action per agent a sampled row is the taken row plus a rank-1 term:
//     x_s[row] = x[row] + delta[s][row] * act_col[row % n]        (delta = sampled - taken action, act_col[i] = fc1's column of action i)
//     baseline[row] = 1/S sum_s head(x_s[row]),   head(x) = relu( relu(LayerNorm(x)) W2^T + b2 ) . w3 + b3
// A wavefront reads a 16-row tile of x and the rows' act_col once and runs the head of k_head_fwd S times on it (S + 1 with v0 = head(x),
// the `values` of coma.py:152), the W2 operand in registers throughout: HBM sees x once, S floats of delta per row and one or two
// floats out, where S separate forwards on formed rows read and write S x [rows][64].  Forward only: the advantage is detached
// (coma.py:182).  The sum over the samples runs in the order s = 0 .. S - 1 in one lane: deterministic.

namespace mapdn {

__global__ void __launch_bounds__(256)
k_cf_baseline(HeadArgs p, const float* __restrict__ act_col, const float* __restrict__ delta, int S, float* __restrict__ baseline,
              float* __restrict__ v0, long rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  f4 wop[4][4];
  load_w2_operand(p.w2, j, g, wop);
  const HeadParams<false> par(p, g);
  const float b3 = p.b3[0];
  const long n_tiles = (rows + 15) >> 4;
  for (long T = (long)blockIdx.x * 4 + wave; T < n_tiles; T += (long)gridDim.x * 4) {
    const long row = T * 16 + j, rc = row < rows ? row : rows - 1;       // (lanes past the end work on the last row and store nothing)
    f4 xb[4], col[4];
    load_row<false>(p, rc, g, xb);
    const float* pc = act_col + (size_t)((unsigned)rc % (unsigned)p.n) * 64 + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) col[c] = *(const f4*)(pc + 16 * c);
    const float* pd = delta + rc;
    float dnext = pd[0], sum = 0.0f;         // the next sample's delta is requested while the current one is in the matrix cores
    for (int s = v0 ? -1 : 0; s < S; ++s) {  // s == -1: the taken row itself
      f4 xa[4];
      if (s < 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) xa[c] = xb[c];
      } else {
        const float d = dnext;
        if (s + 1 < S) dnext = pd[(size_t)(s + 1) * (size_t)rows];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int q = 0; q < 4; ++q) xa[c][q] = fmaf(d, col[c][q], xb[c][q]);
      }
      const float v = head_value(xa, p.eps, wop, par) + b3;
      if (s < 0) { if (g == 0 && row < rows) v0[row] = v; }
      else sum += v;
    }
    if (g == 0 && row < rows) baseline[row] = sum / (float)S;
  }
}

}  // namespace mapdn

extern "C" int mapdn_critic_head_counterfactual(const float* x, int32_t n, const float* act_col, const float* delta, int32_t S,
                                                const float* gamma, const float* beta, float eps, const float* w2, const float* b2,
                                                const float* w3, const float* b3, float* baseline, float* v0, int64_t rows, void* stream) {
  using namespace mapdn;
  if (!head_args_ok(x, nullptr, 1, gamma, beta, w2, b2, w3, b3, rows) || !act_col || !delta || !baseline || n < 1 || S < 1 || S > 64)
    return MAPDN_E_INVALID;
  const HeadArgs a{x, nullptr, n, gamma, beta, eps, w2, b2, w3, b3};
  const int64_t tiles = (rows + 15) / 16;      // (head_fwd_blocks(rows), spelt out: tests/test_cf_kernel_matrix_cpu.py reads the launch shape here)
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, (int64_t)head_cus() * 2));
  hipLaunchKernelGGL(k_cf_baseline, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, act_col, delta, (int)S, baseline, v0, (long)rows);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}
