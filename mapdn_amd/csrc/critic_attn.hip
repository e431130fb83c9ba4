// critic_attn.hip — the core of MAAC's attention critic as ONE forward and ONE backward launch, gfx950 (MI355X).  Compiled inside
// critic.hip (f4, k_head_reduce, head_cus).
//
// Reference: critics/maac_critic.py:116-136 — for every head h and agent i a stack / permute / matmul / softmax / sum chain over the keys
// and values of the OTHER agents.  Here, for sample b, agent i, head h (columns h d .. (h + 1) d of the 64, d = 64 / H):
//     logit_ij = sel_i . key_j   (j != i),    p_ij = softmax_j(logit_ij / sqrt(d))   (row maximum subtracted),    out_i = sum_j p_ij val_j,
//     logit_sq[i][h] = sum_b sum_{j != i} logit_ij^2            (the attention regulariser of maac_critic.py:156-157 on the unscaled logits).
// A workgroup of 256 threads takes one sample at a time (grid stride): the three [n][64] operands go to LDS once (row stride 68 floats: a
// 16-lane group reading 16 consecutive rows with 128-bit loads touches 16 distinct bank slots), the [H][n][n] scores live in LDS, HBM
// sees the operands once and the outputs once — no [b, d, n - 1] stack, no [b, H, n, n] tensor.  Products are f32 fmaf chains over k in
// ascending order on the vector ALU (each thread a 1 x 4 strip of scores, or one float4 of an output row); the coupled shape (n rows of
// 64 per sample, n^2 scores) is far from the 16-row tiles of the MFMA kernels and the launch is LDS- and HBM-bound, see DESIGN section 13.
// The diagonal (j == i) is never read: every loop over the other agents skips it, so there are no pad columns and no -inf fill.
// Row work (maximum, exp, sum, normalisation, sum of squares) is one thread per (h, i): H n <= 192 threads.
// logit_sq: thread (h, i) adds its row's sum of squares sample after sample in a register (the order of the samples a workgroup takes is
// fixed by the grid), writes one partial per workgroup, and k_head_reduce sums the workgroups in a fixed order: deterministic, no atomics,
// no pad (the partial stride is exactly n H).
// Backward: recomputes the scaled logits and the probabilities from the operands (nothing but the operands is saved), then
//     dP_ij = dout_i . val_j,   dlogit_ij = p_ij (dP_ij - sum_j p_ij dP_ij) / sqrt(d) + 2 logit_ij dlogit_sq[i][h],
//     dsel_i = sum_j dlogit_ij key_j,   dkey_j = sum_i dlogit_ij sel_i,   dval_j = sum_i p_ij dout_i          (all sums over the other agents).

namespace mapdn {

constexpr int AT_MAX_N = 48;           // agents per sample: the backward's four operands + two score arrays at H = 4 fit a CU's 160 KB of LDS
constexpr int AT_RS = 68;              // operand row stride in LDS (floats)
constexpr int AT_NT = 256;

// dst[r][0 .. 64) (row stride AT_RS) = src[r][0 .. 64) for r < n, as float4
__device__ __forceinline__ void at_load(float* __restrict__ dst, const float* __restrict__ src, int n, int tid) {
  for (int it = tid; it < n * 16; it += AT_NT) {
    const int r = it >> 4, c = (it & 15) * 4;
    *(f4*)(dst + r * AT_RS + c) = *(const f4*)(src + (size_t)r * 64 + c);
  }
}

// scaled[(h n + i) n + j] = (a_i . b_j over head h's columns) / div, raw[...] = the same undivided (raw may be null), for every h, i, j
// (the diagonal included: nobody reads it).  A thread takes j = jb, jb + JB, jb + 2 JB, jb + 3 JB: consecutive lanes read consecutive rows.
__device__ __forceinline__ void at_dots(const float* __restrict__ sA, const float* __restrict__ sB, float* __restrict__ raw,
                                        float* __restrict__ scaled, int n, int H, int d, float div, int tid) {
  const int JB = (n + 3) >> 2, items = H * n * JB;
  for (int it = tid; it < items; it += AT_NT) {
    const int jb = it % JB, hi = it / JB, i = hi % n, h = hi / n;
    const float* a = sA + i * AT_RS + h * d;
    const float* b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int j = jb + q * JB; b[q] = sB + (j < n ? j : n - 1) * AT_RS + h * d; }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < d; k += 4) {
      const f4 av = *(const f4*)(a + k);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 bv = *(const f4*)(b[q] + k);
        acc[q] = fmaf(av.w, bv.w, fmaf(av.z, bv.z, fmaf(av.y, bv.y, fmaf(av.x, bv.x, acc[q]))));
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = jb + q * JB;
      if (j < n) {
        const int o = (h * n + i) * n + j;
        if (raw) raw[o] = acc[q];
        scaled[o] = acc[q] / div;
      }
    }
  }
}

__global__ void __launch_bounds__(AT_NT)
k_attn_fwd(const float* __restrict__ sel, const float* __restrict__ key, const float* __restrict__ val, int B, int n, int H,
           float* __restrict__ out, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float at_sm[];
  float* sS = at_sm;                       // [n][AT_RS] each
  float* sK = sS + n * AT_RS;
  float* sV = sK + n * AT_RS;
  float* L = sV + n * AT_RS;               // [H][n][n] unscaled logits
  float* P = L + H * n * n;                // [H][n][n] scaled logits -> probabilities
  const int tid = threadIdx.x, d = 64 / H, R = H * n;
  const float div = sqrtf((float)d);
  float lsq = 0.0f;                        // thread (h, i) = tid: sum over this workgroup's samples of the row's sum of squares
  for (int s = blockIdx.x; s < B; s += gridDim.x) {
    const size_t base = (size_t)s * n * 64;
    at_load(sS, sel + base, n, tid); at_load(sK, key + base, n, tid); at_load(sV, val + base, n, tid);
    __syncthreads();
    at_dots(sS, sK, L, P, n, H, d, div, tid);
    __syncthreads();
    if (tid < R) {
      const int i = tid % n;
      float* x = P + tid * n;
      const float* l = L + tid * n;
      float m = -INFINITY, q = 0.0f, sum = 0.0f;
      for (int j = 0; j < n; ++j) if (j != i) { m = fmaxf(m, x[j]); q = fmaf(l[j], l[j], q); }
      for (int j = 0; j < n; ++j) if (j != i) { const float e = expf(x[j] - m); x[j] = e; sum += e; }
      for (int j = 0; j < n; ++j) if (j != i) x[j] = x[j] / sum;
      lsq += q;
    }
    __syncthreads();
    for (int it = tid; it < n * 16; it += AT_NT) {
      const int i = it >> 4, c = (it & 15) * 4, h = c / d;
      const float* p = P + (h * n + i) * n;
      f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int j = 0; j < n; ++j) if (j != i) {
        const float w = p[j];
        const f4 v = *(const f4*)(sV + j * AT_RS + c);
        acc = f4{fmaf(w, v.x, acc.x), fmaf(w, v.y, acc.y), fmaf(w, v.z, acc.z), fmaf(w, v.w, acc.w)};
      }
      *(f4*)(out + base + (size_t)i * 64 + c) = acc;
    }
    __syncthreads();                       // the next sample's loads overwrite the operands
  }
  if (tid < R) partial[(size_t)blockIdx.x * R + (tid % n) * H + tid / n] = lsq;           // logit_sq is [n][H]
}

__global__ void __launch_bounds__(AT_NT)
k_attn_bwd(const float* __restrict__ dout, const float* __restrict__ dlsq, const float* __restrict__ sel, const float* __restrict__ key,
           const float* __restrict__ val, int B, int n, int H, float* __restrict__ dsel, float* __restrict__ dkey, float* __restrict__ dval) {
  extern __shared__ __attribute__((aligned(16))) float at_sm[];
  float* sS = at_sm;
  float* sK = sS + n * AT_RS;
  float* sV = sK + n * AT_RS;
  float* sG = sV + n * AT_RS;              // dout
  float* P = sG + n * AT_RS;               // [H][n][n] scaled logits -> probabilities
  float* D = P + H * n * n;                // [H][n][n] dP -> dlogit
  const int tid = threadIdx.x, d = 64 / H, R = H * n;
  const float div = sqrtf((float)d);
  const float g2 = tid < R ? 2.0f * dlsq[(tid % n) * H + tid / n] : 0.0f;
  for (int s = blockIdx.x; s < B; s += gridDim.x) {
    const size_t base = (size_t)s * n * 64;
    at_load(sS, sel + base, n, tid); at_load(sK, key + base, n, tid); at_load(sV, val + base, n, tid); at_load(sG, dout + base, n, tid);
    __syncthreads();
    at_dots(sS, sK, nullptr, P, n, H, d, div, tid);
    at_dots(sG, sV, nullptr, D, n, H, d, 1.0f, tid);
    __syncthreads();
    if (tid < R) {
      const int i = tid % n;
      float* x = P + tid * n;
      float* dp = D + tid * n;
      float m = -INFINITY, sum = 0.0f, t = 0.0f;
      for (int j = 0; j < n; ++j) if (j != i) m = fmaxf(m, x[j]);
      for (int j = 0; j < n; ++j) if (j != i) sum += expf(x[j] - m);
      for (int j = 0; j < n; ++j) if (j != i) t = fmaf(expf(x[j] - m) / sum, dp[j], t);
      for (int j = 0; j < n; ++j) if (j != i) {
        const float p = expf(x[j] - m) / sum;                    // (the forward's probability, bit for bit)
        dp[j] = fmaf(g2, x[j] * div, p * (dp[j] - t) / div);     // unscaled logit = scaled * sqrt(d): exact for d = 16 and 64
        x[j] = p;
      }
    }
    __syncthreads();
    for (int it = tid; it < n * 16; it += AT_NT) {
      const int r = it >> 4, c = (it & 15) * 4, h = c / d;
      const float* prow = P + h * n * n;
      const float* drow = D + h * n * n;
      f4 as = f4{0.0f, 0.0f, 0.0f, 0.0f}, ak = as, av = as;
      for (int o = 0; o < n; ++o) if (o != r) {
        const float a = drow[r * n + o], b = drow[o * n + r], w = prow[o * n + r];
        const f4 kv = *(const f4*)(sK + o * AT_RS + c), sv = *(const f4*)(sS + o * AT_RS + c), gv = *(const f4*)(sG + o * AT_RS + c);
        as = f4{fmaf(a, kv.x, as.x), fmaf(a, kv.y, as.y), fmaf(a, kv.z, as.z), fmaf(a, kv.w, as.w)};
        ak = f4{fmaf(b, sv.x, ak.x), fmaf(b, sv.y, ak.y), fmaf(b, sv.z, ak.z), fmaf(b, sv.w, ak.w)};
        av = f4{fmaf(w, gv.x, av.x), fmaf(w, gv.y, av.y), fmaf(w, gv.z, av.z), fmaf(w, gv.w, av.w)};
      }
      const size_t off = base + (size_t)r * 64 + c;
      *(f4*)(dsel + off) = as; *(f4*)(dkey + off) = ak; *(f4*)(dval + off) = av;
    }
    __syncthreads();
  }
}

}  // namespace mapdn

static bool attn_shape_ok(int64_t B, int32_t n, int32_t H) {
  return B >= 1 && n >= 2 && n <= mapdn::AT_MAX_N && (H == 1 || H == 2 || H == 4) && B * n * 64 <= 0x7fffffff;
}
static bool attn_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
static int attn_blocks(int64_t B) { return (int)std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)head_cus() * 4)); }
static size_t attn_lds(int32_t n, int32_t H, int operands) { return ((size_t)operands * n * mapdn::AT_RS + (size_t)2 * H * n * n) * 4; }

extern "C" int32_t mapdn_attention_max_agents(void) { return mapdn::AT_MAX_N; }

extern "C" int64_t mapdn_attention_scratch_floats(int64_t B, int32_t n, int32_t H) {
  return attn_shape_ok(B, n, H) ? (int64_t)attn_blocks(B) * n * H : 0;
}

extern "C" int mapdn_attention_forward(const float* sel, const float* key, const float* val, int64_t B, int32_t n, int32_t H, float* out,
                                       float* logit_sq, float* scratch, void* stream) {
  using namespace mapdn;
  if (!attn_shape_ok(B, n, H) || !attn_aligned(sel) || !attn_aligned(key) || !attn_aligned(val) || !attn_aligned(out) || !logit_sq || !scratch)
    return MAPDN_E_INVALID;
  const int blocks = attn_blocks(B);
  const size_t lds = attn_lds(n, H, 3);
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;
  if (hipFuncSetAttribute((const void*)k_attn_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL(k_attn_fwd, dim3(blocks), dim3(AT_NT), lds, (hipStream_t)stream, sel, key, val, (int)B, (int)n, (int)H, out, scratch);
  const int R = n * H;
  hipLaunchKernelGGL(k_head_reduce, dim3((R + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, blocks, R, 0, R, R, logit_sq);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

extern "C" int mapdn_attention_backward(const float* dout, const float* dlogit_sq, const float* sel, const float* key, const float* val,
                                        int64_t B, int32_t n, int32_t H, float* dsel, float* dkey, float* dval, void* stream) {
  using namespace mapdn;
  if (!attn_shape_ok(B, n, H) || !attn_aligned(dout) || !dlogit_sq || !attn_aligned(sel) || !attn_aligned(key) || !attn_aligned(val) ||
      !attn_aligned(dsel) || !attn_aligned(dkey) || !attn_aligned(dval))
    return MAPDN_E_INVALID;
  const size_t lds = attn_lds(n, H, 4);
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;
  if (hipFuncSetAttribute((const void*)k_attn_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL(k_attn_bwd, dim3(attn_blocks(B)), dim3(AT_NT), lds, (hipStream_t)stream, dout, dlogit_sq, sel, key, val, (int)B, (int)n,
                     (int)H, dsel, dkey, dval);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}
