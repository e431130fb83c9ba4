"""The compiled Shapley coalition-critic kernels (csrc/critic_shap.hip, compiled inside critic.hip) and the rows that reach them: test
infrastructure of tests/test_shap_kernel_matrix_cpu.py (the rows cover the compiled set; the launch sites and the host refusals) and
tests/test_shap_kernel_matrix_gpu.py (every row, forward and backward, against the literal construction in float64), and the literal
construction itself (also used by tests/test_sqddpg.py).

The compiled set is parsed from the launch sites of the source (comments stripped), not restated.  A kernel is a tuple:
    ("shap_fwd",)                     k_shap_fwd
    ("shap_bwd", PG, NT)              k_shap_bwd<PG, NT>: PG = with parameter gradients (else dact only), NT threads per workgroup
k_shap_bwd is launched from one templated site, shap_bwd_launch<PG, NT>; its instantiations are that helper's call sites.  Which NT a
row reaches follows from n alone (the per-wavefront LDS); mapdn_critic_shapley_geometry reports it and the tests ask it."""
import ctypes
import os
import re
from typing import NamedTuple

import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests build the rows for (an MI355X); the GPU tests take the device's


def _src(name="critic_shap.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def compiled_kernels():
    """every k_shap_* instantiation the library holds (a list, so that one launched from two sites shows)"""
    src = _src()
    named = set(re.findall(r"\bk_shap_[a-z0-9_]+", src))
    assert named == {"k_shap_fwd", "k_shap_bwd"}, named                    # a third k_shap_* kernel needs a parser and rows here
    sites = re.findall(r"hipLaunchKernelGGL\(\(?(k_shap_[a-z0-9_]+)(<[^>]*>)?\)?,", src)
    assert sorted(sites) == [("k_shap_bwd", "<PG, NT>"), ("k_shap_fwd", "")], sites
    out = [("shap_fwd",)]
    out += [("shap_bwd", pg == "true", int(nt)) for pg, nt in re.findall(r"shap_bwd_launch<(true|false), (\d+)>\(", src)]
    assert len(out) > 1, "critic_shap.hip: shap_bwd_launch call sites not found"
    return out


def geometry(b, S, n, mode, cus=CUS):
    """(code, threads, blocks, lds_bytes, lds_budget, max_n) of mapdn_critic_shapley_geometry (host only with cus > 0)"""
    from mapdn_amd import _lib
    o = [ctypes.c_int32(0) for _ in range(5)]
    code = _lib.load().mapdn_critic_shapley_geometry(b, S, n, mode, cus, *[ctypes.byref(x) for x in o])
    return (code,) + tuple(x.value for x in o)


def max_agents():
    return geometry(1, 1, 1, 0)[5]


class Row(NamedTuple):
    shape: dict         # b, n, S
    label: str
    special: str        # "" | "ident" | "reversed" | "zero-act" | "hot": how pos / the actions are made

    def kernels(self, cus=CUS):
        """the kernels this row reaches: the forward, the backward with parameter gradients, the dact-only backward"""
        b, n, S = self.shape["b"], self.shape["n"], self.shape["S"]
        return (("shap_fwd",), ("shap_bwd", True, geometry(b, S, n, 1, cus)[1]), ("shap_bwd", False, geometry(b, S, n, 2, cus)[1]))


def big_samples(cus):
    """more samples than the wavefronts of 4 x `cus` workgroups of four, + 11: every wavefront of the widest launch (the forward's 2 per CU,
    the backward's 1 per CU) has several samples, no split is even, and the cross-workgroup reduce sums over every workgroup"""
    return cus * 4 * 4 + 11


def rows_for(cus=CUS):
    shapes = [(5, 1, 1, "n1", ""),                  # one agent: one slot, P = act * act_cols[0]
              (5, 2, 1, "n2", ""),                  # two orders only
              (1, 3, 3, "n3-s3", ""),               # a single sample: one wavefront has work, the others an empty range
              (7, 17, 2, "n17", ""),                # groups straddle the 16-row tiles (three groups of 17 per chunk)
              (3, 38, 10, "n38", ""),               # the feeder's shape: one group per chunk, tiles of 16 + 16 + 6, the 192-thread backward
              (2, max_agents(), 1, "nmax", ""),     # the largest n the LDS budget admits: the 128-thread backward
              (big_samples(cus), 3, 2, "big", ""),
              (5, 6, 2, "ident", "ident"),          # pos = identity for every draw: slot p holds agent p
              (5, 6, 2, "reversed", "reversed"),    # ... and its reverse
              (6, 5, 3, "zero-act", "zero-act"),    # all actions 0: P = 0, the values are mapdn_critic_head_forward's on base, id_cols
              (6, 5, 3, "hot", "hot")]              # actions x 100: the LayerNorm inputs are large
    return [Row(dict(b=b, n=n, S=S), tag, sp) for b, n, S, tag, sp in shapes]


ROWS = rows_for(CUS)


def literal_critic_input(obs_all, act, pos):
    """models/sqddpg.py:37-90 step by step on given positions: obs_all [b, K] (every agent's observation, concatenated), act [b, n],
    pos [b, S, n] -> [b, S, n, K + n + n].  The one-hot of the own position; its product with the lower triangle (the slots up to the own
    position); the agent at each position, by scattering; the joint action gathered into slot order in a five-dimensional expansion;
    the slots before the own one detached, those behind it zeroed; and [all obs | slots | one-hot id] concatenated."""
    b, S, n = pos.shape
    K, dt, dev = obs_all.shape[-1], obs_all.dtype, obs_all.device
    pos = pos.long()
    own = torch.zeros(b, S, n, n, dtype=dt, device=dev).scatter_(3, pos.unsqueeze(-1), 1.0)
    upto = torch.matmul(own, torch.tril(torch.ones(n, n, dtype=dt, device=dev)))
    order = torch.zeros(b, S, n, dtype=torch.long, device=dev)
    for i in range(n):
        order.scatter_(2, pos[:, :, i:i + 1], torch.full((b, S, 1), i, dtype=torch.long, device=dev))
    order5 = order.view(b, S, 1, n, 1).expand(b, S, n, n, 1)
    slots = act.view(b, 1, 1, n, 1).expand(b, S, n, n, 1).gather(3, order5)
    slots = (slots * (upto - own).unsqueeze(-1)).detach() + slots * own.unsqueeze(-1)
    obs5 = obs_all.view(b, 1, 1, K).expand(b, S, n, K)
    ids = torch.eye(n, dtype=dt, device=dev).view(1, 1, n, n).expand(b, S, n, n)
    return torch.cat((obs5, slots.reshape(b, S, n, n), ids), dim=-1)
