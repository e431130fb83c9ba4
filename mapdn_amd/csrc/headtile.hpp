// headtile.hpp — the critic head's trunk on one tile of 16 rows of 64 as the steps that the kernels of critic.hip, critic_twin.hip,
// critic_cf.hip and critic_shap.hip are put together from (layouts: the header of critic.hip; lane helpers: rowtile.hpp).  Two places
// still spell a step out beside it and change with it: k_twin_mse its LayerNorm backward (measured slower through ln_backward), and
// critic_shap.hip its four MFMA products (its CPU test reads them in the file's text).
//     v = relu( relu(LayerNorm(x)) W2^T + b2 ) . w3 + b3
// forward   load_w2_operand, HeadParams, head_value (= ln_stats, ln_affine_relu, mm64_reg, head_dot)
// backward  HeadLds (W2 / W2^T operands and the parameters in LDS), mm64_lds (pre^T and dxn^T), mse_dv, dpre_step, dw2_step, ln_backward,
//           dx_dot / formed_handover (where dx goes), HeadAcc + wave_blocks_sum / head_partials (a workgroup's partial block)
// A kernel keeps what is particular to it: how a row is formed, what dv is, where dx goes.  Every step does the operations of the
// kernels it was lifted from in their order (fmaf where they had fmaf, a * b + c where they had that, the same summation order): the
// results are theirs bit for bit.
#pragma once
#include "rowtile.hpp"

namespace mapdn {

// the lane's gamma | beta | b2 | w3 slices in A layout (features 16 c + 4 g + q).  LDS = false: 16 registers; LDS = true (the 512-thread
// k_head_bwd, 256 registers per wavefront): read from HeadLds::sP where used
template <bool LDS> struct HeadParams;
template <> struct HeadParams<false> {
  f4 gam[4], bet[4], b2v[4], w3v[4];
  __device__ __forceinline__ HeadParams(const HeadArgs& p, int g, const float* = nullptr) {      // (one spelling for k_head_bwd's HeadParams<SLIM>)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gam[c] = *(const f4*)(p.gamma + 16 * c + 4 * g); bet[c] = *(const f4*)(p.beta + 16 * c + 4 * g);
      b2v[c] = *(const f4*)(p.b2 + 16 * c + 4 * g); w3v[c] = *(const f4*)(p.w3 + 16 * c + 4 * g);
    }
  }
  __device__ __forceinline__ f4 gamma(int c) const { return gam[c]; }
  __device__ __forceinline__ f4 beta(int c) const { return bet[c]; }
  __device__ __forceinline__ f4 b2(int c) const { return b2v[c]; }
  __device__ __forceinline__ f4 w3(int c) const { return w3v[c]; }
};
template <> struct HeadParams<true> {
  const float* s;
  __device__ __forceinline__ HeadParams(const HeadArgs&, int g, const float* sP) : s(sP + 4 * g) {}
  __device__ __forceinline__ f4 gamma(int c) const { return *(const f4*)(s + 16 * c); }
  __device__ __forceinline__ f4 beta(int c) const { return *(const f4*)(s + 64 + 16 * c); }
  __device__ __forceinline__ f4 b2(int c) const { return *(const f4*)(s + 128 + 16 * c); }
  __device__ __forceinline__ f4 w3(int c) const { return *(const f4*)(s + 192 + 16 * c); }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// forward

// W2 as the register A operand of pre^T = W2 xn^T: wop[nt][c] = W2[16 nt + j][16 c + 4 g ..] (64 VGPRs)
__device__ __forceinline__ void load_w2_operand(const float* w2, int j, int g, f4 (&wop)[4][4]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int c = 0; c < 4; ++c) wop[nt][c] = *(const f4*)(w2 + (size_t)(16 * nt + j) * 64 + 16 * c + 4 * g);
}

// xn = relu(xhat gamma + beta) (xn may be xh itself)
template <class P>
__device__ __forceinline__ void ln_affine_relu(const f4 (&xh)[4], const P& par, f4 (&xn)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f4 y = xh[c] * par.gamma(c) + par.beta(c);
    xn[c] = f4{relu_nan(y.x), relu_nan(y.y), relu_nan(y.z), relu_nan(y.w)};
  }
}

// d^T = Op x^T, a 64 x 64 product as 64 MFMAs, x and d in A layout.  The weight operand in registers ...
__device__ __forceinline__ void mm64_reg(const f4 (&wop)[4][4], const f4 (&x)[4], f4 (&d)[4]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) d[nt] = f4{0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wop[nt][c][q], x[c][q], d[nt], 0, 0, 0);
}
// ... or in LDS ([4 nt][4 c][64 lanes] float4: HeadLds::sW for pre^T = W2 xn^T, HeadLds::sWT for dxn^T = W2^T dpre^T)
__device__ __forceinline__ void mm64_lds(const f4* sOp, int lane, const f4 (&x)[4], f4 (&d)[4]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) d[nt] = f4{0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f4 wv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) wv[nt] = sOp[(nt * 4 + c) * 64 + lane];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][q], x[c][q], d[nt], 0, 0, 0);
  }
}

// relu(pre + b2) . w3 of the lane's row, every lane of the row receiving it (acc = pre^T without the bias)
template <class P>
__device__ __forceinline__ float head_dot(const f4 (&acc)[4], const P& par) {
  float dot = 0.0f;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const f4 bb = par.b2(nt), ww = par.w3(nt);
#pragma unroll
    for (int r = 0; r < 4; ++r) dot = fmaf(relu_nan(acc[nt][r] + bb[r]), ww[r], dot);
  }
  return sum_g(dot);
}

// the forward of one tile: x in A layout (destroyed) -> v - b3 of the lane's row
__device__ __forceinline__ float head_value(f4 (&xa)[4], float eps, const f4 (&wop)[4][4], const HeadParams<false>& par) {
  ln_stats(xa, eps);
  ln_affine_relu(xa, par, xa);
  f4 acc[4];
  mm64_reg(wop, xa, acc);
  return head_dot(acc, par);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward

// the start of a backward kernel's LDS; what follows (staging tiles, accumulators) is per wavefront and the kernel's own, from `rest`
struct HeadLds {
  f4* sW;                                   // [4 nt][4 c][64]: W2[16 nt + j][16 c + 4 g + q]       A operand of pre^T = W2 xn^T
  f4* sWT;                                  // [4 nt][4 c][64]: W2[16 c + 4 g + q][16 nt + j]       A operand of dxn^T = W2^T dpre^T
  float* sP;                                // gamma | beta | b2 | w3 [4][64]
  float* rest;
  __device__ __forceinline__ HeadLds(float* sm) : sW((f4*)sm), sWT(sW + 1024), sP((float*)(sWT + 1024)), rest(sP + 256) {}
  // by the nt threads of the workgroup; a __syncthreads() before the first read.  fill_w2: sW and sWT alone (k_shap_bwd never reads sP)
  __device__ __forceinline__ void fill(const HeadArgs& p, int tid, int nt_threads) const {
    if (tid < 64) { sP[tid] = p.gamma[tid]; sP[64 + tid] = p.beta[tid]; sP[128 + tid] = p.b2[tid]; sP[192 + tid] = p.w3[tid]; }
    fill_w2(p, tid, nt_threads);
  }
  __device__ __forceinline__ void fill_w2(const HeadArgs& p, int tid, int nt_threads) const {
    for (int i = tid; i < 1024; i += nt_threads) {
      const int l = i & 63, c = (i >> 6) & 3, nt = i >> 8, lj = l & 15, lg = l >> 4;
      sW[i] = *(const f4*)(p.w2 + (size_t)(16 * nt + lj) * 64 + 16 * c + 4 * lg);
      f4 t;
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = p.w2[(size_t)(16 * c + 4 * lg + q) * 64 + 16 * nt + lj];
      sWT[i] = t;
    }
  }
};

// a wavefront's parameter-gradient accumulators over its rows
struct HeadAcc {
  f4 accW[4][4];                            // dW2[16 ntu + 4 g + r][16 ntk + j]
  f4 ag[4], ab[4], aw3[4], ab2[4];          // column sums in A layout (this lane's row j only): dgamma, dbeta, dw3, db2
  float ab3, aloss;                         // db3, the fused value loss (lanes with g == 0)
  __device__ __forceinline__ HeadAcc() : ab3(0.0f), aloss(0.0f) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) accW[a][b] = f4{0, 0, 0, 0};
      ag[a] = ab[a] = aw3[a] = ab2[a] = f4{0, 0, 0, 0};
    }
  }
};

// the fused value loss: v from acc = pre^T, err = ret - v, loss += wgt err^2; returns dv = -2 wgt err (0 for a lane past the end)
template <class P>
__device__ __forceinline__ float mse_dv(const f4 (&acc)[4], const P& par, float b3, float ret, float wgt, bool valid, int g, float& aloss) {
  const float err = ret - (head_dot(acc, par) + b3);
  if (valid && g == 0) aloss = fmaf(wgt * err, err, aloss);
  return valid ? -2.0f * wgt * err : 0.0f;
}

// dpre = [pre > 0] dv w3 in place of acc = pre^T; PG: dw3 += relu(pre) dv; db2 += dpre; db3 += dv
template <bool PG, class P>
__device__ __forceinline__ void dpre_step(f4 (&acc)[4], float dvr, const P& par, int g, HeadAcc& A) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const f4 bb = par.b2(nt), ww = par.w3(nt);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pre = acc[nt][r] + bb[r];
      const bool pos = pre > 0.0f;
      const float dp = pos ? dvr * ww[r] : 0.0f;
      if (PG) { A.aw3[nt][r] = fmaf(pos ? pre : 0.0f, dvr, A.aw3[nt][r]); A.ab2[nt][r] += dp; }
      acc[nt][r] = dp;
    }
  }
  if (PG && g == 0) A.ab3 += dvr;
}

// a tile in A layout into a 16 x HS staging tile
__device__ __forceinline__ void stage_store(float* s, int j, int g, const f4 (&t)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) *(f4*)(s + j * HS + 16 * c + 4 * g) = t[c];
}

// dW2 += dpre^T xn: both operands through the wavefront's staging tiles into C layout (rows on the contraction axis).  ONE_TILE (the
// 512-thread k_head_bwd): dpre is read back in C layout for all four steps before the one tile is reused for xn.  The reads of the tiles
// are not fenced off from what the caller stores there next.
template <bool ONE_TILE>
__device__ __forceinline__ void dw2_step(float* stage, int j, int g, const f4 (&dpre)[4], const f4 (&xn)[4], f4 (&accW)[4][4]) {
  float* s0 = stage; float* s1 = ONE_TILE ? stage : stage + 16 * HS;
  stage_store(s0, j, g, dpre);
  if (!ONE_TILE) stage_store(s1, j, g, xn);
  wave_sync();
  float dCs[4][4];
  if (ONE_TILE) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) dCs[s][nt] = s0[(4 * g + s) * HS + 16 * nt + j];
    wave_release();
    stage_store(s1, j, g, xn);
    wave_sync();
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float dC[4], xC[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { dC[nt] = ONE_TILE ? dCs[s][nt] : s0[(4 * g + s) * HS + 16 * nt + j]; xC[nt] = s1[(4 * g + s) * HS + 16 * nt + j]; }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) accW[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(dC[a], xC[b], accW[a][b], 0, 0, 0);
  }
}

// LayerNorm backward on the lane's row: d = [xn > 0] dxn, a = d gamma, dx = rstd (a - mean(a) - xhat mean(a xhat)) in place of dxn;
// PG: dgamma += d xhat, dbeta += d
template <bool PG, class P>
__device__ __forceinline__ void ln_backward(const f4 (&xn)[4], const f4 (&xh)[4], float rs, const P& par, f4 (&dxn)[4], HeadAcc& A) {
  float s1a = 0.0f, s2a = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f4 d;
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = xn[c][q] > 0.0f ? dxn[c][q] : 0.0f;
    if (PG) { A.ag[c] += d * xh[c]; A.ab[c] += d; }
    const f4 a = d * par.gamma(c);
    s1a += hsum(a); s2a += hsum(a * xh[c]);
    dxn[c] = a;
  }
  const float m1 = sum_g(s1a) * (1.0f / 64.0f), m2 = sum_g(s2a) * (1.0f / 64.0f);
#pragma unroll
  for (int c = 0; c < 4; ++c) dxn[c] = (dxn[c] - m1 - xh[c] * m2) * rs;
}

// dx . w of the lane's row, every lane of the row receiving it (pw = w + 4 g)
__device__ __forceinline__ float dx_dot(const f4 (&dx)[4], const float* pw) {
  float d = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) d += hsum(dx[c] * *(const f4*)(pw + 16 * c));
  return sum_g(d);
}

// formed rows: dbase[group] = sum of dx over the group's n rows, dper_n[i] += dx (accn, the wavefront's [n][64] in LDS), for the tile
// of rows row0 .. of the wavefront's range [r0, r1) — through the staging tile s0, lane = column, the tile's rows in order.  carry: the
// running sum over the rows of the current group.  H rows in flight where the tile's rows belong to different agents (n >= 16).
template <int H>
__device__ __forceinline__ void formed_handover(float* s0, float* accn, float* dbase, const f4 (&dx)[4], float& carry, int n, long r0, long r1,
                                                long row0, int lane, int j, int g) {
  stage_store(s0, j, g, dx);
  wave_sync();
  const int cnt = (int)(r1 - row0 < 16 ? r1 - row0 : 16);
  const unsigned rel = (unsigned)(row0 - r0);
  unsigned grp = rel / (unsigned)n, i = rel - grp * (unsigned)n;
  float* pbase = dbase + ((size_t)(r0 / n) + grp) * 64 + lane;
  if (n >= 16) {
    unsigned i2 = i;                      // (i stays the tile's first agent index for the slot addresses)
    // the tile's 16 rows belong to 16 DIFFERENT agents: their dper_n slots are independent — H reads, H adds, H writes in flight
    // instead of 16 dependent LDS round trips
#pragma unroll
    for (int h0 = 0; h0 < 16; h0 += H) {
      float val[H], cur[H];
#pragma unroll
      for (int rr = 0; rr < H; ++rr) {
        unsigned ii = i + h0 + rr; if (ii >= (unsigned)n) ii -= n;
        val[rr] = h0 + rr < cnt ? s0[(h0 + rr) * HS + lane] : 0.0f;
        cur[rr] = accn[ii * 64 + lane];
      }
#pragma unroll
      for (int rr = 0; rr < H; ++rr) {
        unsigned ii = i + h0 + rr; if (ii >= (unsigned)n) ii -= n;
        accn[ii * 64 + lane] = cur[rr] + val[rr];
      }
#pragma unroll
      for (int rr = 0; rr < H; ++rr)
        if (h0 + rr < cnt) {
          carry += val[rr];
          if (++i2 == (unsigned)n) { *pbase = carry; carry = 0.0f; i2 = 0; pbase += 64; }
        }
    }
  } else {
    for (int rr = 0; rr < cnt; ++rr) {
      const float val = s0[rr * HS + lane];
      carry += val;
      accn[i * 64 + lane] += val;
      if (++i == (unsigned)n) { *pbase = carry; carry = 0.0f; i = 0; pbase += 64; }
    }
  }
  wave_release();
}

// ---- the end of a backward kernel: the wavefronts of a workgroup are summed through LDS, in a fixed order, so that the second launch
// (k_head_reduce) reads one partial per workgroup instead of one per wavefront.  Both are called by every thread of the workgroup.

// out[i] = sum over the NT / 64 wavefronts, in order, of their LDS accumulators a0[w * wstride + i], i < count
template <int NT>
__device__ __forceinline__ void wave_blocks_sum(const float* a0, size_t wstride, int count, float* out, int tid) {
  __syncthreads();                          // every wavefront is out of its tile loop
  for (int i = tid; i < count; i += NT) {
    float t = a0[i];
#pragma unroll
    for (int ww = 1; ww < NT / 64; ++ww) t += a0[ww * wstride + i];
    out[i] = t;
  }
}

// pp[0, HW) = the sum over the wavefronts of A in the HP layout (dW2 4096 | dgamma | dbeta | db2 | dw3 | db3 | loss), through
// [NT / 64][STRIDE] floats from the start of LDS (the weights, staging tiles and accumulators there are dead: the launch sizes LDS for
// it).  STRIDE = HP: af is not used.  STRIDE = HP + 64 (k_twin_mse): 64 more column sums af in A layout -> pp[HP, HP + 64).  The pad
// [HW, HP) is neither read nor written.
template <int NT, int STRIDE>
__device__ __forceinline__ void head_partials(float* sm, float* pp, const HeadAcc& A, const f4* af, int tid) {
  static_assert(STRIDE == HP || STRIDE == HP + 64, "a partial block is the head's HP floats, or those and 64 more column sums");
  constexpr bool EXTRA = STRIDE > HP;
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
  __syncthreads();                          // every wavefront is done with the LDS that red overwrites
  float* red = sm + (size_t)wave * STRIDE;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(16 * a + 4 * g + r) * 64 + 16 * b + j] = A.accW[a][b][r];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float tg = sum_j(A.ag[c][q]), tb = sum_j(A.ab[c][q]), t2 = sum_j(A.ab2[c][q]), t3 = sum_j(A.aw3[c][q]);
      const float tf = EXTRA ? sum_j(af[c][q]) : 0.0f;
      if (j == 0) {
        const int col = 16 * c + 4 * g + q;
        red[4096 + col] = tg; red[4160 + col] = tb; red[4224 + col] = t2; red[4288 + col] = t3;
        if (EXTRA) red[HP + col] = tf;
      }
    }
  const float t = sum_j(A.ab3), tl = sum_j(A.aloss);           // (lanes with g != 0 hold 0)
  if (lane == 0) { red[4352] = t; red[4353] = tl; }
  __syncthreads();
  for (int col = tid; col < (EXTRA ? STRIDE : HW); col += NT) {
    if (EXTRA && col >= HW && col < HP) continue;
    float v = sm[col];
#pragma unroll
    for (int ww = 1; ww < NT / 64; ++ww) v += sm[(size_t)ww * STRIDE + col];
    pp[col] = v;
  }
}

}  // namespace mapdn
