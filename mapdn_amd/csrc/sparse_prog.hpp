// sparse_prog.hpp — what every kernel that runs the handle's elimination program (plan.cpp::sparse_program) shares, once: the wave frame
// (SpWave), the block assembly ring (sp_assemble), the interpreter (sp_run_program), and on the host the list of compiled lane counts
// with its prepare and launch helpers.  k_nr_sparse (sparse.hip), k_action_grad_sparse (grad_sparse.hip) and k_opf_sens_sparse
// (opf_sparse.hip) include it and supply three lambdas to the ring.  Device code; not for g++.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "grad_sparse.hpp"   // gs_a
#include "nr_common.hpp"     // kernels.hpp (Dev), d2, u32x4, rcp_nr

namespace mapdn {

// the lane counts L (envs per one-wave workgroup) every such kernel is compiled for; tests/kernel_matrix.py reads the list from here
#define SP_FOR_EACH(X) X(16) X(8) X(4) X(2)

// A stage that reads what other lanes of the wave wrote to LDS waits for those writes (a wait, no barrier — there is one wavefront).
__device__ __forceinline__ void gs_handoff() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// ---- the frame.  A workgroup is ONE wavefront serving L envs with S = 64 / L sub-lanes each (lane = sub * L + env).  Dynamic LDS
// (nr_sparse_lds_bytes): [n + 2] voltages, then the blocks [slot][env][2x2], then the solver's epilogue scratch.
template <int L>
struct SpWave {
  static constexpr unsigned S = 64u / L;
  unsigned s, el, e;                             // sub-lane, env of the workgroup, env (< Bp: every per-env array has a row for it)
  int n, NPH;
  d2* sV;                                        // sV[k * L] = (e, f); k = n slack, n + 1 trash (the node of the padding entries)
  d2* sB;                                        // block b: sB[b * 2L], sB[b * 2L + 1] = rows (a00 a01), (a10 a11)
  __amdgpu_buffer_rsrc_t rsO;                    // the operation records; voO: this sub-lane's op of phase p at voO + p * S * 16
  unsigned voO;
  __device__ __forceinline__ SpWave(const Dev& d, d2* lds2)
      : s(threadIdx.x / L), el(threadIdx.x % L), e(blockIdx.x * L + el), n(d.n), NPH(d.sp_phases), sV(lds2 + el),
        sB(lds2 + (size_t)(d.n + 2) * L + 2u * el),
        rsO(__builtin_amdgcn_make_buffer_rsrc(const_cast<SpOp*>(d.sp_ops), 0, d.sp_ops_bytes, 0x00020000)), voO(s * 16u) {}
  __device__ __forceinline__ d2* blk(unsigned b) const { return sB + (size_t)b * (2u * L); }
};

// blocks that exist only as fill start from zero
template <int L>
__device__ __forceinline__ void sp_zero_fill(const SpWave<L>& w, const Dev& d) {
  for (unsigned q = w.s; q < (unsigned)d.sp_fill; q += w.S) {
    d2* f = w.blk((unsigned)d.sp_fill_slots[q]);
    f[0] = d2{0.0, 0.0}; f[1] = d2{0.0, 0.0};
  }
}

// the converged voltage of the env (the frame's Vout rows, the slack's included) and the trash node
template <int L>
__device__ __forceinline__ void sp_load_voltages(const SpWave<L>& w, const Dev& d) {
  const size_t Bp = (size_t)d.Bp;
  const double* vo = d.nrbuf + (size_t)d.r_vout * Bp + w.e;
  for (unsigned p = w.s; p < (unsigned)w.n + 2u; p += w.S)
    w.sV[(size_t)p * L] = p <= (unsigned)w.n ? d2{vo[((size_t)VOF * p + VO_E) * Bp], vo[((size_t)VOF * p + VO_F) * Bp]} : d2{0.0, 0.0};
}

// ---- the assembly stream: per sub-lane rps rows of mnz records of REC bytes each (row r of sub-lane s is node r * S + s; rows are
// padded to mnz records with Y = 0 at the trash node).  REC = 32: SpNz (Dev::sp_nz); REC = 48: GsNz, which carries Y_ji as well.
template <unsigned REC>
struct SpStream { __amdgpu_buffer_rsrc_t rs; int rps, mnz; };
template <class Rec>
__device__ __forceinline__ SpStream<sizeof(Rec)> sp_stream(const Rec* table, uint32_t bytes, int rows_per_sub, int max_nnz) {
  return {__builtin_amdgcn_make_buffer_rsrc(const_cast<Rec*>(table), 0, bytes, 0x00020000), rows_per_sub, max_nnz};
}

template <unsigned REC> struct SpRec;
template <> struct SpRec<32u> {
  u32x4 a; u32x2 t;                              // col, slot, Re Y_ij | Im Y_ij
  __device__ __forceinline__ double yr() const { return __hiloint2double((int)a.w, (int)a.z); }
  __device__ __forceinline__ double yi() const { return __hiloint2double((int)t.y, (int)t.x); }
  __device__ __forceinline__ unsigned col() const { return a.x & ~SP_COL_GEN; }      // (bit 31: the column's node is a gen bus)
};
template <> struct SpRec<48u> {
  u32x4 a, b; u32x2 t;                           // col, slot, Re Y_ij | Im Y_ij, Re Y_ji | Im Y_ji
  __device__ __forceinline__ double yr() const { return __hiloint2double((int)a.w, (int)a.z); }
  __device__ __forceinline__ double yi() const { return __hiloint2double((int)b.y, (int)b.x); }
  __device__ __forceinline__ double ytr() const { return __hiloint2double((int)b.w, (int)b.z); }
  __device__ __forceinline__ double yti() const { return __hiloint2double((int)t.y, (int)t.x); }
  __device__ __forceinline__ unsigned col() const { return a.x; }
};

// ---- the ring.  Every sub-lane walks its stream row by row and forms A_ij = V_i conj(Y_ij V_j), the row sum S_i and A_ii; the kernel
// stores what it makes of them:  row_begin(i, live) before the first record of a row,  entry(z, slot, vi, vj, ar, ai) for every record
// with a block slot,  row_end(i, live, vi, sr, si, aii_r, aii_i) after its last (live: i is a node, not padding).  The records are read
// through a ring that runs PF entries ahead of the arithmetic: the table is a constant in L2, but a global round trip per entry would
// otherwise be the whole cost of the assembly.  Control flow is wave-uniform.
template <int L, unsigned REC, class RowBegin, class Entry, class RowEnd>
__device__ __forceinline__ void sp_assemble(const SpWave<L>& w, const SpStream<REC>& zs, const RowBegin& row_begin, const Entry& entry,
                                            const RowEnd& row_end) {
  constexpr unsigned S = 64u / L;
  constexpr int PF = 8;
  const int RPS = zs.rps, MNZ = zs.mnz, T = RPS * MNZ;
  const unsigned n = (unsigned)w.n;
  const unsigned voZ = w.s * (unsigned)RPS * (unsigned)MNZ * REC;  // the records of this sub-lane's rows
  auto zload = [&](int t) {
    const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)min(t, T - 1) * REC);
    SpRec<REC> z;
    z.a = __builtin_amdgcn_raw_buffer_load_b128(zs.rs, voZ, so, 0);
    if constexpr (REC == 48u) z.b = __builtin_amdgcn_raw_buffer_load_b128(zs.rs, voZ + 16u, so, 0);
    z.t = __builtin_amdgcn_raw_buffer_load_b64(zs.rs, voZ + (REC - 16u), so, 0);
    return z;
  };
  SpRec<REC> zq[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) zq[u] = zload(u);
  int r = 0, q = 0;
  unsigned i = w.s;
  bool live = i < n;
  row_begin(i, live);
  d2 vi = w.sV[(size_t)(live ? i : n + 1u) * L];
  double sr = 0.0, si = 0.0, aii_r = 0.0, aii_i = 0.0;
  for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int t = t0 + u;
      if (t < T) {                               // (uniform; no `break`: the loop must unroll for the ring to stay in registers)
      const SpRec<REC> z = zq[u];
      zq[u] = zload(t + PF);
      const unsigned col = z.col();
      const int slot = (int)z.a.y;
      const d2 vj = w.sV[(size_t)col * L];
      double ar, ai;
      gs_a(vi.x, vi.y, z.yr(), z.yi(), vj.x, vj.y, &ar, &ai);
      sr += ar; si += ai;
      if (col == i) { aii_r = ar; aii_i = ai; }
      if (slot >= 0) entry(z, (unsigned)slot, vi, vj, ar, ai);
      if (++q == MNZ) {                          // (uniform) end of the row; next row
        row_end(i, live, vi, sr, si, aii_r, aii_i);
        q = 0; ++r;
        i = (unsigned)r * S + w.s;
        live = i < n && r < RPS;
        row_begin(i, live);
        vi = w.sV[(size_t)(live ? i : n + 1u) * L];
        sr = si = aii_r = aii_i = 0.0;
      }
      }
    }
  }
}

// ---- the interpreter: all phases of the program on the blocks of w — sub-lane s executes operation s of every phase for its L envs
// (S records per phase, w.NPH phases).  skip: this lane's env takes no more writes (the solver's per-env `done`).  Control flow is
// wave-uniform.  Plain `inline`, not __forceinline__: every kernel calls it from one or two places and the inliner takes it whole either
// way, but forced inlining happens before the body is simplified and schedules k_nr_sparse 2 % slower.
template <int L>
__device__ inline void sp_run_program(const SpWave<L>& w, const bool skip = false) {
  constexpr unsigned S = 64u / L;
  constexpr int PF = 8;                          // operation records run PF phases ahead (constant table in L2)
  const int NPH = w.NPH;
  u32x4 oq[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) oq[u] = __builtin_amdgcn_raw_buffer_load_b128(w.rsO, w.voO, __builtin_amdgcn_readfirstlane((unsigned)min(u, NPH - 1) * S * 16u), 0);
  for (int p0 = 0; p0 < NPH; p0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int p = p0 + u;
      if (p < NPH) {                             // (uniform)
      const u32x4 op = oq[u];
      oq[u] = __builtin_amdgcn_raw_buffer_load_b128(w.rsO, w.voO, __builtin_amdgcn_readfirstlane((unsigned)min(p + PF, NPH - 1) * S * 16u), 0);
      const unsigned type = op.x & 255u;
      const unsigned hint = __builtin_amdgcn_readfirstlane(op.x);     // bits 8 / 9: the phase holds an INV / an UPD (wave-uniform)
      const d2* A = w.blk(op.z); const d2* B = w.blk(op.w); d2* C = w.blk(op.y);
      const d2 a0 = A[0], a1 = A[1], b0 = B[0], b1 = B[1];
      d2 c0 = d2{0.0, 0.0}, c1 = d2{0.0, 0.0};
      if (hint & 512u) { c0 = C[0]; c1 = C[1]; }
      const double p00 = a0.x * b0.x + a0.y * b1.x, p01 = a0.x * b0.y + a0.y * b1.y;
      const double p10 = a1.x * b0.x + a1.y * b1.x, p11 = a1.x * b0.y + a1.y * b1.y;
      d2 n0, n1;
      if (type == 2u) { n0 = d2{p00, p01}; n1 = d2{p10, p11}; }
      else { n0 = d2{c0.x - p00, c0.y - p01}; n1 = d2{c1.x - p10, c1.y - p11}; }
      if (hint & 256u) {
        const double idet = rcp_nr(a0.x * a1.y - a0.y * a1.x);
        if (type == 1u) { n0 = d2{a1.y * idet, -a0.y * idet}; n1 = d2{-a1.x * idet, a0.x * idet}; }
      }
      if (type != 0u && !skip) { C[0] = n0; C[1] = n1; }
      }
    }
  }
}

// ---- host: one kernel of a template per lane count of SP_FOR_EACH.  `kernel` maps std::integral_constant<int, l> to the pointer of
// the instantiation for l, e.g. [](auto l) { return k_opf_sens_sparse<decltype(l)::value>; }.
template <class F>
inline bool sp_for_lanes(int L, F f) {
#define X(l) if (L == l) { f(std::integral_constant<int, l>{}); return true; }
  SP_FOR_EACH(X)
#undef X
  return false;
}
// the dynamic-LDS limit of the instantiation for L: 0, -1 when the runtime refuses, -2 for an L that is not instantiated
template <class K>
inline int sp_prepare(int L, K kernel) {
  int rc = -2;
  sp_for_lanes(L, [&](auto l) {
    rc = hipFuncSetAttribute((const void*)kernel(l), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess ? 0 : -1;
  });
  return rc;
}
// the instantiation for d.sp_lanes on one one-wave workgroup per sp_lanes of `envs`, with the handle's LDS
template <class K, class... A>
inline void sp_launch(const Dev& d, int envs, hipStream_t st, K kernel, const A&... a) {
  const size_t lds = nr_sparse_lds_bytes(d.n, d.sp_blocks, d.sp_lanes);
  sp_for_lanes(d.sp_lanes, [&](auto l) {
    hipLaunchKernelGGL(kernel(l), dim3((envs + decltype(l)::value - 1) / decltype(l)::value), dim3(64), lds, st, a...);
  });
}

}  // namespace mapdn
