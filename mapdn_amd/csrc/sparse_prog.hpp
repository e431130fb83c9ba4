// sparse_prog.hpp — the interpreter of the handle's elimination program (plan.cpp::sparse_program) for the kernels that run it outside
// the power flow: k_action_grad_sparse (grad_sparse.hip) and k_opf_sens_sparse (opf_sparse.hip).  k_nr_sparse keeps its own copy, which
// carries a per-env `done` mask.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nr_common.hpp"

namespace mapdn {

// A stage that reads what other lanes of the wave wrote to LDS waits for those writes (a wait, no barrier — there is one wavefront).
__device__ __forceinline__ void gs_handoff() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// All phases of the program on the blocks [slot][env][2x2] at sB (this lane's env: block b at sB + b * 2L, rows (a00 a01), (a10 a11)):
// sub-lane s executes operation s of every phase for its L envs.  rsO: the operation records, voO = s * 16 this sub-lane's record of a
// phase, S = 64 / L records per phase, NPH phases.  Control flow is wave-uniform.
template <int L>
__device__ __forceinline__ void sp_run_program(d2* sB, const __amdgpu_buffer_rsrc_t rsO, const unsigned voO, const int NPH) {
  constexpr unsigned S = 64u / L;
  constexpr int PF = 8;                          // operation records run PF phases ahead (constant table in L2)
  auto blk = [&](unsigned b) { return sB + (size_t)b * (2u * L); };
  u32x4 oq[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) oq[u] = __builtin_amdgcn_raw_buffer_load_b128(rsO, voO, __builtin_amdgcn_readfirstlane((unsigned)min(u, NPH - 1) * S * 16u), 0);
  for (int p0 = 0; p0 < NPH; p0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int p = p0 + u;
      if (p < NPH) {                             // (uniform)
      const u32x4 op = oq[u];
      oq[u] = __builtin_amdgcn_raw_buffer_load_b128(rsO, voO, __builtin_amdgcn_readfirstlane((unsigned)min(p + PF, NPH - 1) * S * 16u), 0);
      const unsigned type = op.x & 255u;
      const unsigned hint = __builtin_amdgcn_readfirstlane(op.x);     // bits 8 / 9: the phase holds an INV / an UPD (wave-uniform)
      const d2* A = blk(op.z); const d2* B = blk(op.w); d2* C = blk(op.y);
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
      if (type != 0u) { C[0] = n0; C[1] = n1; }
      }
    }
  }
}

}  // namespace mapdn
