// critic_twin.hip — MATD3's twin critic head as ONE launch, gfx950 (MI355X).  Compiled inside critic.hip (its helpers and layouts).
//
// Reference: models/matd3.py:35-86 — ONE MLPCritic values the MADDPG input twice, with one more input column that is 0 (values1) or 1
// (values2).  Behind the first layer that is the single head of critic.hip on two rows that differ by a constant:
//     x1[row] = base[row / n] + per_n[row % n]            x2[row] = x1[row] + flag_col          (flag_col = fc1.weight[:, -1], [64])
//     v_h     = relu( relu(LayerNorm(x_h)) W2^T + b2 ) . w3 + b3
// A wavefront forms the 16-row tile once and runs the two heads one after the other on it with the W2 operand kept (registers in the
// forward, LDS in the loss kernel): one read of base / per_n, one operand load, and what leaves the kernel is already combined —
// min(v1, v2) for the target (matd3.py:141-142), dbase / dper_n / the parameter gradients summed over both heads for the loss
// (matd3.py:143-150), d flag_col = the second head's dx summed over all rows.  Layouts, tiles, the per-wavefront [n][64] LDS
// accumulator, the partial-and-reduce scheme and the pad rule are those of k_head_fwd / k_head_bwd<true, 3, 256>.

namespace mapdn {

constexpr int TP = HP + 64;            // floats of a twin partial / grads block ahead of dper_n: the head's HP | d flag_col [64]

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: v1, v2, vmin = min(v1, v2) per formed row; each output may be null
__global__ void __launch_bounds__(256)
k_twin_fwd(HeadArgs p, const float* __restrict__ flag, float* __restrict__ v1, float* __restrict__ v2, float* __restrict__ vmin, long rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  f4 wop[4][4], gam[4], bet[4], b2v[4], w3v[4], flg[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
    for (int c = 0; c < 4; ++c) wop[nt][c] = *(const f4*)(p.w2 + (size_t)(16 * nt + j) * 64 + 16 * c + 4 * g);
    gam[nt] = *(const f4*)(p.gamma + 16 * nt + 4 * g); bet[nt] = *(const f4*)(p.beta + 16 * nt + 4 * g);
    b2v[nt] = *(const f4*)(p.b2 + 16 * nt + 4 * g); w3v[nt] = *(const f4*)(p.w3 + 16 * nt + 4 * g);
    flg[nt] = *(const f4*)(flag + 16 * nt + 4 * g);
  }
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
      ln_stats(xa, p.eps);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f4 y = xa[c] * gam[c] + bet[c];
        xa[c] = f4{relu_nan(y.x), relu_nan(y.y), relu_nan(y.z), relu_nan(y.w)};
      }
      f4 acc[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wop[nt][c][q], xa[c][q], acc[nt], 0, 0, 0);
      float dot = 0.0f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dot = fmaf(relu_nan(acc[nt][r] + b2v[nt][r]), w3v[nt][r], dot);
      vh[h] = sum_g(dot) + b3;
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
  f4* sW = (f4*)sm;                         // as k_head_bwd: W2 / W2^T operands, gamma | beta | b2 | w3, staging tiles, [n][64] accumulators
  f4* sWT = sW + 1024;
  float* sP = (float*)(sWT + 1024);
  float* stage = sP + 256 + (size_t)(threadIdx.x >> 6) * TILES * 16 * HS;
  float* accn = sP + 256 + (size_t)NW * TILES * 16 * HS + (size_t)(threadIdx.x >> 6) * p.n * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
  if (tid < 64) { sP[tid] = p.gamma[tid]; sP[64 + tid] = p.beta[tid]; sP[128 + tid] = p.b2[tid]; sP[192 + tid] = p.w3[tid]; }
  for (int i = tid; i < 1024; i += NT) {
    const int l = i & 63, c = (i >> 6) & 3, nt = i >> 8, lj = l & 15, lg = l >> 4;
    sW[i] = *(const f4*)(p.w2 + (size_t)(16 * nt + lj) * 64 + 16 * c + 4 * lg);
    f4 t;
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = p.w2[(size_t)(16 * c + 4 * lg + q) * 64 + 16 * nt + lj];
    sWT[i] = t;
  }
  for (int i = lane; i < p.n * 64; i += 64) accn[i] = 0.0f;
  f4 gam[4], bet[4], b2v[4], w3v[4], flg[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    gam[nt] = *(const f4*)(p.gamma + 16 * nt + 4 * g); bet[nt] = *(const f4*)(p.beta + 16 * nt + 4 * g);
    b2v[nt] = *(const f4*)(p.b2 + 16 * nt + 4 * g); w3v[nt] = *(const f4*)(p.w3 + 16 * nt + 4 * g);
    flg[nt] = *(const f4*)(flag + 16 * nt + 4 * g);
  }
  __syncthreads();

  // this wavefront's range of rows [r0, r1): whole groups of n
  const long W = (long)gridDim.x * NW, w = (long)blockIdx.x * NW + wave;
  const long G = rows / p.n, r0 = (G * w / W) * p.n, r1 = (G * (w + 1) / W) * p.n;

  f4 accW[4][4];                            // dW2[16 ntu + 4 g + r][16 ntk + j], both heads
  f4 ag[4], ab[4], aw3[4], ab2[4], af[4];   // column sums in A layout: dgamma, dbeta, dw3, db2 (both heads), d flag_col (second head's dx)
  float ab3 = 0.0f, carry = 0.0f, aloss = 0.0f;
  const float b3 = p.b3[0], lscale = 0.5f * scale[0];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) accW[a][b] = f4{0, 0, 0, 0};
    ag[a] = ab[a] = aw3[a] = ab2[a] = af[a] = f4{0, 0, 0, 0};
  }

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
    float wgt = lscale;
    if (wrow) wgt *= wrow[(unsigned)(valid ? row : r1 - 1) / (unsigned)p.n];
    f4 dxs[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};      // dx of the tile's rows, summed over the two heads
#pragma nounroll
    for (int h = 0; h < 2; ++h) {         // one head after the other: a real loop, so that the two never compete for registers
      f4 xh[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) xh[c] = h ? xb[c] + flg[c] : xb[c];
      const float rs = ln_stats(xh, p.eps);
      f4 xn[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f4 y = xh[c] * gam[c] + bet[c];
        xn[c] = f4{relu_nan(y.x), relu_nan(y.y), relu_nan(y.z), relu_nan(y.w)};
      }
      // ---- pre^T = W2 xn^T
      f4 acc[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 wv[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wv[nt] = sW[(nt * 4 + c) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][q], xn[c][q], acc[nt], 0, 0, 0);
      }
      // ---- v_h, its error against the shared returns, dv_h = -2 w (ret - v_h) with w = 1/2 scale wrow
      float dot = 0.0f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f4 bb = b2v[nt], ww = w3v[nt];
#pragma unroll
        for (int r = 0; r < 4; ++r) dot = fmaf(relu_nan(acc[nt][r] + bb[r]), ww[r], dot);
      }
      const float err = rt - (sum_g(dot) + b3);
      const float dvr = valid ? -2.0f * wgt * err : 0.0f;
      if (valid && g == 0) aloss = fmaf(wgt * err, err, aloss);
      // ---- dpre = [pre > 0] dv w3 (in place of acc); dw3 += relu(pre) dv; db2 += dpre; db3 += dv
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f4 bb = b2v[nt], ww = w3v[nt];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pre = acc[nt][r] + bb[r];
          const bool pos = pre > 0.0f;
          const float dp = pos ? dvr * ww[r] : 0.0f;
          aw3[nt][r] = fmaf(pos ? pre : 0.0f, dvr, aw3[nt][r]); ab2[nt][r] += dp;
          acc[nt][r] = dp;
        }
      }
      if (g == 0) ab3 += dvr;
      // ---- dxn^T = W2^T dpre^T
      f4 dxn[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 wv[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wv[nt] = sWT[(nt * 4 + c) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dxn[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][q], acc[c][q], dxn[nt], 0, 0, 0);
      }
      // ---- dW2 += dpre^T xn: both operands through LDS into C layout (rows on the contraction axis)
      {
        float* s0 = stage; float* s1 = stage + 16 * HS;
#pragma unroll
        for (int c = 0; c < 4; ++c) *(f4*)(s0 + j * HS + 16 * c + 4 * g) = acc[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) *(f4*)(s1 + j * HS + 16 * c + 4 * g) = xn[c];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float dC[4], xC[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) { dC[nt] = s0[(4 * g + s) * HS + 16 * nt + j]; xC[nt] = s1[(4 * g + s) * HS + 16 * nt + j]; }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) accW[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(dC[a], xC[b], accW[a][b], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();          // (the staging tiles are free for the second head / the hand-over)
      }
      // ---- LayerNorm backward on the lane's row
      float s1a = 0.0f, s2a = 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 d;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = xn[c][q] > 0.0f ? dxn[c][q] : 0.0f;
        ag[c] += d * xh[c]; ab[c] += d;
        const f4 a = d * gam[c];
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
    // ---- hand the summed dx over: dbase[group] = sum over the group's n rows, dper_n[i] += dx — lane = column, the tile's rows in order
    {
      float* s0 = stage;
#pragma unroll
      for (int c = 0; c < 4; ++c) *(f4*)(s0 + j * HS + 16 * c + 4 * g) = dxs[c];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int cnt = (int)(r1 - row0 < 16 ? r1 - row0 : 16);
      const unsigned rel = (unsigned)(row0 - r0);
      unsigned grp = rel / (unsigned)p.n, i = rel - grp * (unsigned)p.n;
      float* pbase = dx + ((size_t)(r0 / p.n) + grp) * 64 + lane;
      if (p.n >= 16) {
        unsigned i2 = i;
        constexpr int H = 16;      // rows in flight: the tile's rows belong to different agents, their slots are independent
#pragma unroll
        for (int h0 = 0; h0 < 16; h0 += H) {
          float val[H], cur[H];
#pragma unroll
          for (int rr = 0; rr < H; ++rr) {
            unsigned ii = i + h0 + rr; if (ii >= (unsigned)p.n) ii -= p.n;
            val[rr] = h0 + rr < cnt ? s0[(h0 + rr) * HS + lane] : 0.0f;
            cur[rr] = accn[ii * 64 + lane];
          }
#pragma unroll
          for (int rr = 0; rr < H; ++rr) {
            unsigned ii = i + h0 + rr; if (ii >= (unsigned)p.n) ii -= p.n;
            accn[ii * 64 + lane] = cur[rr] + val[rr];
          }
#pragma unroll
          for (int rr = 0; rr < H; ++rr)
            if (h0 + rr < cnt) {
              carry += val[rr];
              if (++i2 == (unsigned)p.n) { *pbase = carry; carry = 0.0f; i2 = 0; pbase += 64; }
            }
        }
      } else {
        for (int rr = 0; rr < cnt; ++rr) {
          const float val = s0[rr * HS + lane];
          carry += val;
          accn[i * 64 + lane] += val;
          if (++i == (unsigned)p.n) { *pbase = carry; carry = 0.0f; i = 0; pbase += 64; }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // ---- partial sums of the workgroup, through LDS in a fixed order (as k_head_bwd; TP floats per wavefront)
  float* pp = partial + (size_t)blockIdx.x * pstride;
  __syncthreads();
  {
    const float* a0 = sP + 256 + (size_t)NW * TILES * 16 * HS;
    for (int i = tid; i < p.n * 64; i += NT) {
      float t = a0[i];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) t += a0[(size_t)ww * p.n * 64 + i];
      pp[TP + i] = t;
    }
  }
  __syncthreads();
  float* red = sm + (size_t)wave * TP;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(16 * a + 4 * g + r) * 64 + 16 * b + j] = accW[a][b][r];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float tg = sum_j(ag[c][q]), tb = sum_j(ab[c][q]), t2 = sum_j(ab2[c][q]), t3 = sum_j(aw3[c][q]), tf = sum_j(af[c][q]);
      if (j == 0) {
        const int col = 16 * c + 4 * g + q;
        red[4096 + col] = tg; red[4160 + col] = tb; red[4224 + col] = t2; red[4288 + col] = t3; red[HP + col] = tf;
      }
    }
  const float t = sum_j(ab3), tl = sum_j(aloss);
  if (lane == 0) { red[4352] = t; red[4353] = tl; }
  __syncthreads();
  for (int col = tid; col < TP; col += NT) {
    if (col >= HW && col < HP) continue;      // pad: neither read nor written
    float v = sm[col];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) v += sm[(size_t)ww * TP + col];
    pp[col] = v;
  }
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
  const HeadArgs a{base, per_n, n, gamma, beta, eps, w2, b2, w3, b3};
  const int64_t tiles = (rows + 15) / 16;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, (int64_t)head_cus() * 2));
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
  const HeadArgs a{base, per_n, n, gamma, beta, eps, w2, b2, w3, b3};
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
