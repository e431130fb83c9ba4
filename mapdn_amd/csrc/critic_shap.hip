// critic_shap.hip — SQDDPG's Shapley coalition critic (models/sqddpg.py:37-106) on rows that are FORMED in the kernel, gfx950.
// Included at the end of critic.hip (HeadArgs, k_head_reduce, head_cus, the row-tile helpers of rowtile.hpp and the trunk's steps of
// headtile.hpp are in scope: this file has the coalition rows — the prefix P, the walks over a group — and where their dx goes; its
// four MFMA products stay spelt out here, see k_shap_fwd).
//
// The reference evaluates its critic on b x S x n rows of width n o + n a + n: sample b, coalition draw s, agent i.  With a = 1 and
// pos[b][s][i] = the position of agent i in draw s's order (gc = argsort(pos) = the agent at each position), the first layer of row
// (b, s, i) is
//     x[b][s][i] = base[b] + id_cols[i] + P[b][s][pos_i],      P[b][s][p] = sum_{q <= p} act[b][gc[q]] act_cols[q]
// (base = W_obs obs_all + b1, id_cols / act_cols = the id / action columns of fc1, transposed to [n][64]): the action slots are filled by
// POSITION, the slots behind the own one are zero, and only the own slot carries a gradient back to the action.  A wavefront owns
// whole samples (S n rows) and walks them in chunks of whole (b, s) groups: the chunk's prefix P is built once in LDS by a running sum
// (lane = column), then the chunk's rows go through the trunk (headtile.hpp, as k_head_fwd / k_head_bwd) in tiles of 16, straddling groups.  Backward,
// row (b, s, i) writes its dx over P[pos_i] — the slot that it alone read — so that after the chunk's tiles the same LDS rows hold dx in
// POSITION order and
//     dact_cols[q] += act[b][gc[q]] sum_{p >= q} dx[gc[p]]   (a suffix sum),   did_cols[gc[p]] += dx,   dbase[b] = sum over the sample
// are one walk per group.  dact[b][i] = sum_s dx[b][s][i] . act_cols[pos_i] is a dot in the row's registers, summed over s in order.
// Every sum has one writer and a fixed order: no atomics, two runs give identical bits.
// pos is int32 (a draw of torch.multinomial narrowed once by the caller; n is not bounded by 255).  A value outside [0, n) is clamped,
// so that a pos row that is no permutation (a broken precondition) gives wrong numbers, never an access outside the buffers.

namespace mapdn {

struct ShapArgs {
  const float* id_cols; const float* act_cols; const float* act; const int32_t* pos;
  int S, CG;                           // draws per sample; groups per chunk
  long b;
};

// floats of per-wavefront LDS behind the staging tiles: P [CR][64] | pos [CR] | gc [CR] | act by slot [CR] | per-row value [CR] |
// per-agent running sum [n] (| did_cols [n][64] | dact_cols [n][64]), CR = CG n; rounded to 4 floats (P is read as float4)
__host__ __device__ inline int shap_wave_floats(int n, int CG, bool acc) {
  const int CR = CG * n;
  return ((CR * 68 + n + (acc ? 2 * n * 64 : 0)) + 3) & ~3;
}

struct ShapWave {
  float* P; int* posS; int* gcS; float* actS; float* valS; float* facc; float* accI; float* accA;
  __device__ ShapWave(float* w, int n, int CG) {
    const int CR = CG * n;
    P = w; posS = (int*)(w + CR * 64); gcS = posS + CR; actS = (float*)(gcS + CR); valS = actS + CR; facc = valS + CR;
    accI = facc + n; accA = accI + n * 64;
  }
};

// the chunk's groups gq .. gq + ng: pos, gc, the action of every slot, and the prefix P
__device__ __forceinline__ void shap_chunk_setup(const HeadArgs& p, const ShapArgs& q, const ShapWave& L, long gq, int ng, int lane) {
  const int n = p.n, nr = ng * n;
  for (int r = lane; r < nr; r += 64) {
    int ps = q.pos[(size_t)gq * n + r];
    ps = ps < 0 ? 0 : (ps >= n ? n - 1 : ps);
    L.posS[r] = ps;
    L.gcS[r] = 0;
  }
  wave_sync();
  for (int r = lane; r < nr; r += 64) { const int grp = r / n; L.gcS[grp * n + L.posS[r]] = r - grp * n; }
  wave_sync();
  for (int r = lane; r < nr; r += 64) {
    const int grp = r / n;
    L.actS[r] = q.act[(size_t)((gq + grp) / q.S) * n + L.gcS[r]];
  }
  wave_sync();
  for (int grp = 0; grp < ng; ++grp) {
    float run = 0.0f;
    float* Pg = L.P + (size_t)grp * n * 64 + lane;
    const float* ag = L.actS + grp * n;
#pragma unroll 4
    for (int s = 0; s < n; ++s) { run = fmaf(ag[s], q.act_cols[(size_t)s * 64 + lane], run); Pg[s * 64] = run; }
  }
  wave_sync();
}

// row r of the chunk in A layout: base[b] + id_cols[i] + P[group][pos_i]; returns the row's P slot
__device__ __forceinline__ int shap_load_row(const HeadArgs& p, const ShapArgs& q, const ShapWave& L, long gq, int r, int g, f4 (&xa)[4]) {
  const int n = p.n, grp = r / n, i = r - grp * n, slot = grp * n + L.posS[r];
  const float* pb = p.x + (size_t)((gq + grp) / q.S) * 64 + 4 * g;
  const float* pn = p.per_n + (size_t)i * 64 + 4 * g;
  const float* pp = L.P + (size_t)slot * 64 + 4 * g;
#pragma unroll
  for (int c = 0; c < 4; ++c) xa[c] = (*(const f4*)(pb + 16 * c) + *(const f4*)(pn + 16 * c)) + *(const f4*)(pp + 16 * c);
  return slot;
}

// out[(b, i)] = sum over the sample's draws, in the order s = 0 .. S - 1, of the chunk's per-row values (times scale at the end)
__device__ __forceinline__ void shap_sum_draws(const ShapArgs& q, const ShapWave& L, int n, long gq, int ng, int lane, float scale, float* out) {
  for (int i = lane; i < n; i += 64) {
    float a = L.facc[i];
    for (int grp = 0; grp < ng; ++grp) {
      a += L.valS[grp * n + i];
      const long G = gq + grp;
      if ((G + 1) % q.S == 0) { out[(size_t)(G / q.S) * n + i] = a * scale; a = 0.0f; }
    }
    L.facc[i] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: v[b][s][i] and, with phi != nullptr, phi[b][i] = (sum_s v[b][s][i]) / S.  HeadArgs: x = base, per_n = id_cols.
__global__ void __launch_bounds__(256)
k_shap_fwd(HeadArgs p, ShapArgs q, float* __restrict__ v, float* __restrict__ phi) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15, n = p.n;
  const ShapWave L(sm + (size_t)wave * shap_wave_floats(n, q.CG, false), n, q.CG);
  f4 wop[4][4];
  load_w2_operand(p.w2, j, g, wop);
  const HeadParams<false> par(p, g);
  const float b3 = p.b3[0], inv_s = 1.0f / (float)q.S;
  const long W = (long)gridDim.x * 4, w = (long)blockIdx.x * 4 + wave;
  const long g0 = (q.b * w / W) * q.S, g1 = (q.b * (w + 1) / W) * q.S;      // whole samples: phi[b] has one writer
  if (phi) for (int i = lane; i < n; i += 64) L.facc[i] = 0.0f;
  for (long gq = g0; gq < g1; gq += q.CG) {
    const int ng = (int)(g1 - gq < q.CG ? g1 - gq : q.CG), nr = ng * n;
    shap_chunk_setup(p, q, L, gq, ng, lane);
    for (int t0 = 0; t0 < nr; t0 += 16) {
      const int r = t0 + j;
      const bool valid = r < nr;
      f4 xa[4];
      shap_load_row(p, q, L, gq, valid ? r : nr - 1, g, xa);
      // head_value() spelt out, and the three products of the backward below: tests/test_shap_kernel_matrix_cpu.py counts the MFMA
      // products in this file's text and looks for its relu
      ln_stats(xa, p.eps);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f4 y = xa[c] * par.gamma(c) + par.beta(c);
        xa[c] = f4{relu_nan(y.x), relu_nan(y.y), relu_nan(y.z), relu_nan(y.w)};
      }
      f4 acc[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wop[nt][c][qq], xa[c][qq], acc[nt], 0, 0, 0);
      const float dot = head_dot(acc, par) + b3;
      if (g == 0 && valid) { v[(size_t)gq * n + r] = dot; L.valS[r] = dot; }
    }
    wave_sync();
    if (phi) shap_sum_draws(q, L, n, gq, ng, lane, inv_s, phi);
    wave_sync();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward (recomputes the forward).  PG = true: dbase, the trunk's parameter gradients (HP layout) and did_cols / dact_cols as one
// partial per workgroup [HP | n 64 | n 64], dact when dact != nullptr.  PG = false: dact only (the policy update: the parameters do not
// require grad and the observations carry none).  NT = 256 / 192 / 128 threads: as many wavefronts as the per-wavefront LDS admits.
template <bool PG, int NT>
__global__ void __launch_bounds__(NT)
k_shap_bwd(HeadArgs p, ShapArgs q, const float* __restrict__ dv, float* __restrict__ dbase, float* __restrict__ dact,
           float* __restrict__ partial, int pstride) {
  constexpr int NW = NT / 64;
  extern __shared__ float sm[];
  const HeadLds H(sm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15, n = p.n;
  const int wfl = 2 * 16 * HS + shap_wave_floats(n, q.CG, PG);     // per wavefront: two staging tiles, then the ShapWave block
  float* stage = H.rest + (size_t)wave * wfl;
  const ShapWave L(stage + 2 * 16 * HS, n, q.CG);
  H.fill_w2(p, tid, NT);
  if (PG) for (int i = lane; i < 2 * n * 64; i += 64) L.accI[i] = 0.0f;      // (accA follows accI)
  if (dact) for (int i = lane; i < n; i += 64) L.facc[i] = 0.0f;
  const HeadParams<false> par(p, g);
  __syncthreads();

  const long W = (long)gridDim.x * NW, w = (long)blockIdx.x * NW + wave;
  const long g0 = (q.b * w / W) * q.S, g1 = (q.b * (w + 1) / W) * q.S;      // whole samples: dbase[b] and dact[b] have one writer

  HeadAcc A;
  float carry = 0.0f;

  for (long gq = g0; gq < g1; gq += q.CG) {
    const int ng = (int)(g1 - gq < q.CG ? g1 - gq : q.CG), nr = ng * n;
    shap_chunk_setup(p, q, L, gq, ng, lane);
    for (int t0 = 0; t0 < nr; t0 += 16) {
      const int r = t0 + j;
      const bool valid = r < nr;
      f4 xh[4];
      const int slot = shap_load_row(p, q, L, gq, valid ? r : nr - 1, g, xh);
      const float dvr = valid ? dv[(size_t)gq * n + r] : 0.0f;
      const float rs = ln_stats(xh, p.eps);
      f4 xn[4];
      ln_affine_relu(xh, par, xn);
      // ---- pre^T = W2 xn^T (mm64_lds)
      f4 acc[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 wv[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wv[nt] = H.sW[(nt * 4 + c) * 64 + lane];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][qq], xn[c][qq], acc[nt], 0, 0, 0);
      }
      dpre_step<PG>(acc, dvr, par, g, A);
      // ---- dxn^T = W2^T dpre^T (mm64_lds)
      f4 dxn[4] = {f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}, f4{0, 0, 0, 0}};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        f4 wv[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wv[nt] = H.sWT[(nt * 4 + c) * 64 + lane];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dxn[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[nt][qq], acc[c][qq], dxn[nt], 0, 0, 0);
      }
      // ---- dW2 += dpre^T xn: both operands through LDS into C layout (dw2_step<false>)
      if (PG) {
        float* s0 = stage; float* s1 = stage + 16 * HS;
        stage_store(s0, j, g, acc);
        stage_store(s1, j, g, xn);
        wave_sync();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float dC[4], xC[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) { dC[nt] = s0[(4 * g + s) * HS + 16 * nt + j]; xC[nt] = s1[(4 * g + s) * HS + 16 * nt + j]; }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) A.accW[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(dC[a], xC[b], A.accW[a][b], 0, 0, 0);
        }
        wave_sync();                         // (the next tile's staging writes come after these reads)
      }
      ln_backward<PG>(xn, xh, rs, par, dxn, A);
      // ---- hand dx over: the own-slot dot for dact; dx over the row's own P slot (position order) for the group walks
      if (dact) {
        const float d = dx_dot(dxn, q.act_cols + (size_t)L.posS[valid ? r : nr - 1] * 64 + 4 * g);
        if (g == 0 && valid) L.valS[r] = d;
      }
      if (PG && valid) {
        float* pp = L.P + (size_t)slot * 64 + 4 * g;
#pragma unroll
        for (int c = 0; c < 4; ++c) *(f4*)(pp + 16 * c) = dxn[c];
      }
    }
    wave_sync();
    if (PG) {
      // lane = column; positions from the last to the first: suffix sum for dact_cols, did_cols by agent, dbase over the sample
      for (int grp = 0; grp < ng; ++grp) {
        const float* Dg = L.P + (size_t)grp * n * 64 + lane;
        const float* agp = L.actS + grp * n;
        const int* gcp = L.gcS + grp * n;
        float run = 0.0f;
        for (int s = n - 1; s >= 0; --s) {
          const float d = Dg[s * 64];
          unsigned ai = (unsigned)gcp[s]; ai = ai < (unsigned)n ? ai : 0u;
          run += d;
          L.accA[s * 64 + lane] = fmaf(agp[s], run, L.accA[s * 64 + lane]);
          L.accI[ai * 64 + lane] += d;
        }
        carry += run;
        const long G = gq + grp;
        if ((G + 1) % q.S == 0) { dbase[(size_t)(G / q.S) * 64 + lane] = carry; carry = 0.0f; }
      }
    }
    if (dact) shap_sum_draws(q, L, n, gq, ng, lane, 1.0f, dact);
    wave_sync();
  }

  // ---- one partial block per workgroup: [0, HW) the trunk's parameter gradients | pad | [HP, ..) did_cols | dact_cols
  if (PG) {
    float* pp = partial + (size_t)blockIdx.x * pstride;
    const float* a0 = H.rest + 2 * 16 * HS + (size_t)(q.CG * n) * 68 + n;       // wavefront 0's accI
    wave_blocks_sum<NT>(a0, (size_t)wfl, 2 * n * 64, pp + HP, tid);
    head_partials<NT, HP>(sm, pp, A, nullptr, tid);
  }
}

}  // namespace mapdn

static constexpr size_t SHAP_LDS_BUDGET = (size_t)160 * 1024;
static int shap_cg(int32_t n) { return n >= 64 ? 1 : 64 / n; }           // groups per chunk: about 64 rows (four tiles), whole groups
static size_t shap_fwd_lds(int32_t n) { return (size_t)4 * mapdn::shap_wave_floats(n, shap_cg(n), false) * 4; }
static size_t shap_bwd_lds(int32_t n, bool pg, int nt) {
  const size_t nw = nt / 64;
  size_t lds = (size_t)2 * 1024 * 16 + 256 * 4 + nw * ((size_t)2 * 16 * mapdn::HS + mapdn::shap_wave_floats(n, shap_cg(n), pg)) * 4;
  if (pg) lds = std::max(lds, nw * mapdn::HP * 4);
  return lds;
}
// threads of the backward launch: the most wavefronts (4, 3, 2) whose LDS fits a CU; 0: n is too large
static int shap_bwd_threads(int32_t n, bool pg) {
  for (int nt = 256; nt >= 128; nt -= 64) if (shap_bwd_lds(n, pg, nt) <= SHAP_LDS_BUDGET) return nt;
  return 0;
}
static int32_t shap_max_n() {
  static int32_t m = 0;
  if (!m) { int32_t n = 1; while (shap_bwd_threads(n + 1, true) && shap_fwd_lds(n + 1) <= SHAP_LDS_BUDGET) ++n; m = n; }
  return m;
}
static bool shap_shape_ok(int64_t b, int32_t S, int32_t n) {
  return b >= 1 && S >= 1 && n >= 1 && n <= shap_max_n() && b <= 0x7fffffff / ((int64_t)S * n) && b * S * n < 0x7fffffffLL;
}
static bool shap_al16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
static bool shap_al4(const void* p) { return p && ((uintptr_t)p & 3) == 0; }
static int shap_blocks(int64_t b, int nw, int per_cu, int cus = 0) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((b + nw - 1) / nw, (int64_t)(cus ? cus : head_cus()) * per_cu));
}
// pos on the host (pinned or plain memory): every row of n must be a permutation of 0 .. n - 1; plain host memory is refused either way
// (the kernels cannot read it).  Device memory: a documented precondition.  true: go on.
static bool shap_pos_ok(const int32_t* pos, int64_t groups, int32_t n) {
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, pos);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return true;
  if (at.type != hipMemoryTypeHost) return false;
  unsigned char* seen = (unsigned char*)malloc((size_t)n);
  if (!seen) return false;
  bool ok = true;
  for (int64_t gi = 0; gi < groups && ok; ++gi) {
    for (int32_t i = 0; i < n; ++i) seen[i] = 0;
    for (int32_t i = 0; i < n && ok; ++i) {
      const int32_t v = pos[gi * n + i];
      if (v < 0 || v >= n || seen[v]) ok = false; else seen[v] = 1;
    }
  }
  free(seen);
  return ok;
}
static bool shap_operands_ok(const float* base, const float* id_cols, const float* act_cols, const float* act, const int32_t* pos,
                             const float* gamma, const float* beta, const float* w2, const float* b2, const float* w3, const float* b3) {
  return shap_al16(base) && shap_al16(id_cols) && shap_al16(act_cols) && shap_al4(act) && shap_al4(pos) && shap_al16(gamma) && shap_al16(beta) &&
         shap_al16(w2) && shap_al16(b2) && shap_al16(w3) && shap_al4(b3);
}

extern "C" int64_t mapdn_critic_shapley_scratch_floats(int64_t b, int32_t S, int32_t n) {
  if (!shap_shape_ok(b, S, n)) return 0;
  return (int64_t)shap_blocks(b, 2, 1) * (mapdn::HP + 2 * (int64_t)n * 64);      // (no launch shape has more workgroups than the 2-wavefront one)
}

// mode 0: forward; 1: backward with parameter gradients; 2: backward, dact only.  lds_budget / max_n are reported whatever the shape.
extern "C" int mapdn_critic_shapley_geometry(int64_t b, int32_t S, int32_t n, int32_t mode, int32_t cus, int32_t* threads, int32_t* blocks,
                                             int32_t* lds_bytes, int32_t* lds_budget, int32_t* max_n) {
  if (lds_budget) *lds_budget = (int32_t)SHAP_LDS_BUDGET;
  if (max_n) *max_n = shap_max_n();
  if (!shap_shape_ok(b, S, n) || mode < 0 || mode > 2 || cus < 0) return MAPDN_E_INVALID;
  const int nt = mode == 0 ? 256 : shap_bwd_threads(n, mode == 1);
  if (!nt) return MAPDN_E_INVALID;
  if (threads) *threads = nt;
  if (blocks) *blocks = mode == 0 ? shap_blocks(b, 4, 2, cus) : shap_blocks(b, nt / 64, 1, cus);
  if (lds_bytes) *lds_bytes = (int32_t)(mode == 0 ? shap_fwd_lds(n) : shap_bwd_lds(n, mode == 1, nt));
  return MAPDN_OK;
}

extern "C" int mapdn_critic_shapley_forward(const float* base, const float* id_cols, const float* act_cols, const float* act, const int32_t* pos,
                                            int64_t b, int32_t S, int32_t n, const float* gamma, const float* beta, float eps, const float* w2,
                                            const float* b2, const float* w3, const float* b3, float* v, float* phi, void* stream) {
  using namespace mapdn;
  if (!shap_shape_ok(b, S, n) || !shap_operands_ok(base, id_cols, act_cols, act, pos, gamma, beta, w2, b2, w3, b3) || !shap_al4(v) ||
      (phi && !shap_al4(phi)))
    return MAPDN_E_INVALID;
  const size_t lds = shap_fwd_lds(n);
  if (lds > SHAP_LDS_BUDGET || !shap_pos_ok(pos, b * S, n)) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(base, id_cols, n, gamma, beta, eps, w2, b2, w3, b3);
  const ShapArgs q{id_cols, act_cols, act, pos, S, shap_cg(n), (long)b};
  if (hipFuncSetAttribute((const void*)k_shap_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SHAP_LDS_BUDGET) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL(k_shap_fwd, dim3(shap_blocks(b, 4, 2)), dim3(256), lds, (hipStream_t)stream, a, q, v, phi);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

template <bool PG, int NT>
static int shap_bwd_launch(const mapdn::HeadArgs& a, const mapdn::ShapArgs& q, const float* dv, float* dbase, float* dact, float* scratch,
                           float* grads, hipStream_t st) {
  using namespace mapdn;
  const int blocks = shap_blocks(q.b, NT / 64, 1), pstride = HP + 2 * a.n * 64;
  const size_t lds = shap_bwd_lds(a.n, PG, NT);
  const void* fn = (const void*)k_shap_bwd<PG, NT>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SHAP_LDS_BUDGET) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL((k_shap_bwd<PG, NT>), dim3(blocks), dim3(NT), lds, st, a, q, dv, dbase, dact, scratch, pstride);
  if (PG) {
    hipLaunchKernelGGL(k_head_reduce, dim3((HP + 63) / 64), dim3(256), 0, st, (const float*)scratch, blocks, pstride, 0, HP, HW, grads);
    hipLaunchKernelGGL(k_head_reduce, dim3(2 * a.n), dim3(256), 0, st, (const float*)scratch, blocks, pstride, HP, pstride, pstride, grads);
  }
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

extern "C" int mapdn_critic_shapley_backward(const float* dv, const float* base, const float* id_cols, const float* act_cols, const float* act,
                                             const int32_t* pos, int64_t b, int32_t S, int32_t n, const float* gamma, const float* beta, float eps,
                                             const float* w2, const float* b2, const float* w3, const float* b3, float* dbase, float* grads,
                                             float* scratch, float* dact, int32_t param_grads, void* stream) {
  using namespace mapdn;
  if (!shap_shape_ok(b, S, n) || !shap_operands_ok(base, id_cols, act_cols, act, pos, gamma, beta, w2, b2, w3, b3) || !shap_al4(dv) ||
      (dact && !shap_al4(dact)))
    return MAPDN_E_INVALID;
  if (param_grads ? (!shap_al16(dbase) || !shap_al4(grads) || !shap_al4(scratch)) : !dact) return MAPDN_E_INVALID;
  const int nt = shap_bwd_threads(n, param_grads != 0);
  if (!nt || !shap_pos_ok(pos, b * S, n)) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(base, id_cols, n, gamma, beta, eps, w2, b2, w3, b3);
  const ShapArgs q{id_cols, act_cols, act, pos, S, shap_cg(n), (long)b};
  hipStream_t st = (hipStream_t)stream;
  if (param_grads) {
    if (nt == 256) return shap_bwd_launch<true, 256>(a, q, dv, dbase, dact, scratch, grads, st);
    if (nt == 192) return shap_bwd_launch<true, 192>(a, q, dv, dbase, dact, scratch, grads, st);
    return shap_bwd_launch<true, 128>(a, q, dv, dbase, dact, scratch, grads, st);
  }
  if (nt != 256) return MAPDN_E_INVALID;      // (without the accumulators four wavefronts fit for every n that shap_max_n admits)
  return shap_bwd_launch<false, 256>(a, q, dv, nullptr, dact, nullptr, nullptr, st);
}
