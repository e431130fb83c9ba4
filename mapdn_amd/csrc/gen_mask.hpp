// gen_mask.hpp — the 2x2 pivot block of a GEN BUS (a bus with an in-service net.gen row: |V| held at the gen's vm_pu, P given, Q free;
// pypower's "PV" type — in this code base "PV bus" means a photovoltaic sgen's bus, so the voltage-controlled kind is a gen bus).
//
// The solvers work on z = [dtheta, d|V|/|V|] in 2x2 blocks per node.  newtonpf drops the Q equation and the |V| unknown of a gen bus;
// in block form that is the same block with its Q row and its |V| column struck out and a 1 left on the diagonal, so that the block
// stays regular and the eliminated unknown comes out as exactly 0:
//   after the children's Schur terms:  D1 = D2 = 0, D3 = 1, r1 = 0
//   row 2 of U = J'(k, parent) is 0 and column 2 of L = J'(parent, k) is 0
//   hence  D^-1 = [[1 / D0, 0], [0, 1]],  h1 = 0,  G2 = G3 = 0,  z_m(k) = 0
// (L's column 2 only ever multiplies G2, G3 and h1, which are 0: nothing else needs a mask.  A gen PARENT needs no mask in its children
// either: what they add to its D1, D2, D3 and r1 is overwritten here, and its z_m = 0 meets their G1, G3.)
// The fill-free tree elimination and the sparse program are therefore untouched.  Written once, as selects (the flag differs from lane to
// lane), for plan.cpp (host: flat-start factorisation), nr_tree.hpp and sparse.hip; plain C++, so that g++ can check it.
#pragma once

#if defined(__HIP__)     // (the compiler's own macro: set for every HIP translation unit, with or without the runtime's headers)
#define MAPDN_GEN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define MAPDN_GEN_HD inline
#endif

namespace mapdn {

// the pivot D = [[D0, D1], [D2, D3]] and the second right-hand side entry of a node, masked when the node is a gen bus
MAPDN_GEN_HD void gen_mask_pivot(bool gen, double& D1, double& D2, double& D3, double& r1) {
  D1 = gen ? 0.0 : D1; D2 = gen ? 0.0 : D2; D3 = gen ? 1.0 : D3; r1 = gen ? 0.0 : r1;
}
// I = D^-1 from idet = 1 / (D0 D3 - D1 D2); for a (masked) gen bus idet = 1 / D0 and I = [[1 / D0, 0], [0, 1]] exactly
MAPDN_GEN_HD void gen_pivot_inverse(bool gen, double D0, double D1, double D2, double D3, double idet, double& I0, double& I1, double& I2,
                                    double& I3) {
  I0 = D3 * idet; I1 = -D1 * idet; I2 = -D2 * idet; I3 = gen ? 1.0 : D0 * idet;
}
// second row of G = I U: row 2 of U = J'(k, parent) of a gen bus is zero
MAPDN_GEN_HD void gen_mask_factor(bool gen, double& G2, double& G3) { G2 = gen ? 0.0 : G2; G3 = gen ? 0.0 : G3; }
// the Q mismatch of a gen bus is not an equation: it neither enters ||F||inf nor the right-hand side
MAPDN_GEN_HD double gen_mask_fq(bool gen, double Fq) { return gen ? 0.0 : Fq; }

}  // namespace mapdn
