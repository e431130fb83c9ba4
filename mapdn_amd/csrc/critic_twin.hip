// critic_twin.hip — MATD3's twin critic head as ONE launch, gfx950 (MI355X).  Compiled inside critic.hip (its layouts and load_row; the
// trunk's steps are those of headtile.hpp: this file has what the twin adds — the second row, min(v1, v2), the two heads' dx summed;
// k_twin_mse spells one step out itself, its LayerNorm backward, see there).
//
// Reference: models/matd3.py:35-86 — ONE MLPCritic values the MADDPG input twice, with one more input column that is 0 (values1) or 1
// (values2).  Behind the first layer that is the single head of critic.hip on two rows that differ by a constant:
//     x1[row] = base[row / n] + per_n[row % n]            x2[row] = x1[row] + flag_col          (flag_col = fc1.weight[:, -1], [64])
//     v_h     = relu( relu(LayerNorm(x_h)) W2^T + b2 ) . w3 + b3
// A wavefront forms the 16-row tile once and runs the two heads one after the other on it with the W2 operand kept (registers in the
// forward, LDS in the loss kernel): one read of base / per_n, one operand load, and what leaves the kernel is already combined —
// min(v1, v2) for the target (matd3.py:141-142), dbase / dper_n / the parameter gradients summed over both heads for the loss
// (matd3.py:143-150), d flag_col = the second head's dx summed over all rows.  Layouts, tiles, the per-wavefront [n][64] LDS
// accumulator, the partial-and-reduce scheme and the pad rule are those of k_head_fwd / k_head_bwd<true, 3, 256>: the same calls but for that one step.

namespace mapdn {

constexpr int TP = HP + 64;            // floats of a twin partial / grads block ahead of dper_n: the head's HP | d flag_col [64]

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: v1, v2, vmin = min(v1, v2) per formed row; each output may be null
__global__ void __launch_bounds__(256)
k_twin_fwd(HeadArgs p, const float* __restrict__ flag, float* __restrict__ v1, float* __restrict__ v2, float* __restrict__ vmin, long rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  f4 wop[4][4], flg[4];
  load_w2_operand(p.w2, j, g, wop);
  const HeadParams<false> par(p, g);
#pragma unroll
  for (int c = 0; c < 4; ++c) flg[c] = *(const f4*)(flag + 16 * c + 4 * g);
  const float b3 = p.b3[0];
  const long n_tiles = (rows + 15) >> 4;
  for (long T = (long)blockIdx.x * 4 + wave; T < n_tiles; T += (long)gridDim.x * 4) {
    const long row = T * 16 + j;
    f4 xb[4];
    load_row<true>(p, row < rows ? row : rows - 1, g, xb);
    float vh[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f4 xa[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) xa[c] = h ? xb[c] + flg[c] : xb[c];
      vh[h] = head_value(xa, p.eps, wop, par) + b3;
    }
    if (g == 0 && row < rows) {
      if (v1) v1[row] = vh[0];
      if (v2) v2[row] = vh[1];
      if (vmin) vmin[row] = vh[1] < vh[0] || vh[1] != vh[1] ? vh[1] : vh[0];          // torch.min: NaN wins
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// loss = scale[0] sum_rows wrow[row / n] 1/2 [(ret - v1)^2 + (ret - v2)^2] and every gradient of it (k_head_bwd<true, 3, 256> on both
// heads of a tile, the dx of the two summed in registers before the one hand-over to dbase / dper_n).  partial (per workgroup):
// the head's [0, HW) | pad | [HP, HP + 64) d flag_col | [TP, TP + n * 64) dper_n.
__global__ void __launch_bounds__(256)
k_twin_mse(HeadArgs p, const float* __restrict__ flag, const float* __restrict__ ret, float* __restrict__ dx, float* __restrict__ partial,
           int pstride, long rows, const float* __restrict__ wrow, const float* __restrict__ scale) {
  constexpr int NT = 256, NW = NT / 64, TILES = 2;          // one wavefront per SIMD; two staging tiles per wavefront
  extern __shared__ float sm[];
  const HeadLds L(sm);                      // then, as k_head_bwd: staging tiles, [n][64] accumulators
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
  float* stage = L.rest + (size_t)wave * TILES * 16 * HS;
  float* accn0 = L.rest + (size_t)NW * TILES * 16 * HS, *accn = accn0 + (size_t)wave * p.n * 64;
  L.fill(p, tid, NT);
  for (int i = lane; i < p.n * 64; i += 64) accn[i] = 0.0f;
  const HeadParams<false> par(p, g);
  f4 flg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) flg[c] = *(const f4*)(flag + 16 * c + 4 * g);
  __syncthreads();
  // this wavefront's range of rows [r0, r1): whole groups of n
  const long W = (long)gridDim.x * NW, w = (long)blockIdx.x * NW + wave;
  const long G = rows / p.n, r0 = (G * w / W) * p.n, r1 = (G * (w + 1) / W) * p.n;
  HeadAcc A;                                // both heads
  f4 af[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};      // d flag_col in A layout: the second head's dx
  float carry = 0.0f;
  const float b3 = p.b3[0], lscale = 0.5f * scale[0];
  f4 xnext[4];
  float rtnext = 0.0f;
  if (r0 < r1) {
    const long row = r0 + j;
    load_row<true>(p, row < r1 ? row : r1 - 1, g, xnext);
    rtnext = row < r1 ? ret[row] : 0.0f;
  }
  for (long row0 = r0; row0 < r1; row0 += 16) {
    const long row = row0 + j;
    const bool valid = row < r1;
    f4 xb[4];
    float rt;
#pragma unroll
    for (int c = 0; c < 4; ++c) xb[c] = xnext[c];
    rt = rtnext;
    if (row0 + 16 < r1) {                    // the next tile is requested while this one is in the matrix cores
      const long rn = row + 16;
      load_row<true>(p, rn < r1 ? rn : r1 - 1, g, xnext);
      rtnext = rn < r1 ? ret[rn] : 0.0f;
    }
    float wgt = lscale;                      // w = 1/2 scale wrow for both heads
    if (wrow) wgt *= wrow[(unsigned)(valid ? row : r1 - 1) / (unsigned)p.n];
    f4 dxs[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};      // dx of the tile's rows, summed over the two heads
#pragma nounroll
    for (int h = 0; h < 2; ++h) {         // one head after the other: a real loop, so that the two never compete for registers
      f4 xh[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) xh[c] = h ? xb[c] + flg[c] : xb[c];
      const float rs = ln_stats(xh, p.eps);
      f4 xn[4], acc[4], dxn[4];
      ln_affine_relu(xh, par, xn);
      mm64_lds(L.sW, lane, xn, acc);         // pre^T = W2 xn^T
      const float dvr = mse_dv(acc, par, b3, rt, wgt, valid, g, A.aloss);      // v_h against the shared returns
      dpre_step<true>(acc, dvr, par, g, A);
      mm64_lds(L.sWT, lane, acc, dxn);       // dxn^T = W2^T dpre^T
      dw2_step<false>(stage, j, g, acc, xn, A.accW);
      wave_release();                        // (the staging tiles are free for the second head / the hand-over)
      // ---- LayerNorm backward, spelt out: through ln_backward() the compiler scalarises it into the dW2 products (6.89 ms against 6.70)
      float s1a = 0.0f, s2a = 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 d;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = xn[c][q] > 0.0f ? dxn[c][q] : 0.0f;
        A.ag[c] += d * xh[c]; A.ab[c] += d;
        const f4 a = d * par.gamma(c);
        s1a += hsum(a); s2a += hsum(a * xh[c]);
        dxn[c] = a;
      }
      const float m1 = sum_g(s1a) * (1.0f / 64.0f), m2 = sum_g(s2a) * (1.0f / 64.0f);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f4 d = (dxn[c] - m1 - xh[c] * m2) * rs;
        if (h) af[c] += d;
        dxs[c] += d;
      }
    }
    formed_handover<16>(stage, accn, dx, dxs, carry, p.n, r0, r1, row0, lane, j, g);
  }
  // ---- one partial block per workgroup (as k_head_bwd, TP floats per wavefront in LDS)
  float* pp = partial + (size_t)blockIdx.x * pstride;
  wave_blocks_sum<NT>(accn0, (size_t)p.n * 64, p.n * 64, pp + TP, tid);
  head_partials<NT, TP>(sm, pp, A, af, tid);
}

}  // namespace mapdn

// launch shape of k_twin_mse: workgroups as k_head_bwd<true, 3, 256> (one per CU, never more wavefronts than groups), 256 threads = one
// wavefront per SIMD.  A 512-thread form (two wavefronts per SIMD within 256 registers each, what the single head takes at large batches)
// was tried and needs 272 bytes of scratch per lane for the second head's state: not kept.
constexpr int TWIN_MSE_THREADS = 256;
static size_t twin_mse_lds(int32_t n) {
  return std::max(head_bwd_lds(TWIN_MSE_THREADS, n, true), (size_t)(TWIN_MSE_THREADS / 64) * mapdn::TP * 4);
}
static bool twin_args_ok(const float* base, const float* per_n, int32_t n, const float* flag, const float* gamma, const float* beta, const float* w2,
                         const float* b2, const float* w3, const float* b3, int64_t rows) {
  return head_args_ok(base, per_n, n, gamma, beta, w2, b2, w3, b3, rows) && per_n && flag;
}

extern "C" int mapdn_critic_twin_forward(const float* base, const float* per_n, int32_t n, const float* flag_col, const float* gamma,
                                         const float* beta, float eps, const float* w2, const float* b2, const float* w3, const float* b3,
                                         float* v1, float* v2, float* vmin, int64_t rows, void* stream) {
  using namespace mapdn;
  if (!twin_args_ok(base, per_n, n, flag_col, gamma, beta, w2, b2, w3, b3, rows) || (!v1 && !v2 && !vmin)) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(base, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  const int blocks = head_fwd_blocks(rows);
  hipLaunchKernelGGL(k_twin_fwd, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, flag_col, v1, v2, vmin, (long)rows);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

extern "C" int64_t mapdn_critic_twin_scratch_floats(int64_t rows, int32_t n) {
  if (rows < 1 || n < 1 || rows % n) return 0;
  return (int64_t)head_bwd_blocks(rows, n, true, TWIN_MSE_THREADS / 64) * (mapdn::TP + (int64_t)n * 64);
}

extern "C" int mapdn_critic_twin_geometry(int64_t rows, int32_t n, int32_t cus, int32_t* threads, int32_t* blocks, int32_t* lds_bytes) {
  if (rows < 1 || rows > 0x7fffffff || cus < 0 || n < 1 || n > 256 || rows % n) return MAPDN_E_INVALID;
  const int c = cus ? cus : head_cus();
  const int nt = TWIN_MSE_THREADS;
  const size_t lds = twin_mse_lds(n);
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;        // (what the launch refuses)
  if (threads) *threads = nt;
  if (blocks) *blocks = head_bwd_blocks(rows, n, true, nt / 64, c);
  if (lds_bytes) *lds_bytes = (int32_t)lds;
  return MAPDN_OK;
}

extern "C" int mapdn_critic_twin_mse(const float* ret, const float* wrow, const float* scale, const float* base, const float* per_n, int32_t n,
                                     const float* flag_col, const float* gamma, const float* beta, float eps, const float* w2, const float* b2,
                                     const float* w3, const float* b3, float* dbase, float* grads, float* scratch, int64_t rows, void* stream) {
  using namespace mapdn;
  if (!twin_args_ok(base, per_n, n, flag_col, gamma, beta, w2, b2, w3, b3, rows) || !ret || !scale || !dbase || !grads || !scratch)
    return MAPDN_E_INVALID;
  const HeadArgs a = head_args(base, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  hipStream_t st = (hipStream_t)stream;
  const int blocks = head_bwd_blocks(rows, n, true, TWIN_MSE_THREADS / 64), pstride = TP + n * 64;
  const size_t lds = twin_mse_lds(n);
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;
  if (hipFuncSetAttribute((const void*)k_twin_mse, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL(k_twin_mse, dim3(blocks), dim3(TWIN_MSE_THREADS), lds, st, a, flag_col, ret, dbase, scratch, pstride, (long)rows, wrow, scale);
  hipLaunchKernelGGL(k_head_reduce, dim3((HP + 63) / 64), dim3(256), 0, st, scratch, blocks, pstride, 0, HP, HW, grads);
  hipLaunchKernelGGL(k_head_reduce, dim3(1 + n), dim3(256), 0, st, scratch, blocks, pstride, HP, TP + n * 64, TP + n * 64, grads);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}
