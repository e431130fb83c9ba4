"""The compiled attention-core kernels (csrc/critic_attn.hip, compiled inside critic.hip) and the rows that reach them: test
infrastructure of tests/test_attn_kernel_matrix_cpu.py (the rows cover the compiled set; the launch sites and the argument limits) and
tests/test_attn_kernel_matrix_gpu.py (every row, forward and backward, against the literal per-head, per-agent loop in float64).

The compiled set is parsed from the launch sites of the source (comments stripped), not restated.  A kernel is a tuple:
    ("attn_fwd",)   k_attn_fwd        ("attn_bwd",)   k_attn_bwd
Neither is templated: n and H are run-time arguments, so the rows vary them.  Launch: 256 threads, min(B, 4 per CU) workgroups, one
sample per workgroup per grid-stride turn."""
import os
import re
from typing import NamedTuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests build the rows for (an MI355X); the GPU tests take the device's
BLOCKS_PER_CU = 4


def _src(name="critic_attn.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def max_agents():
    return int(re.search(r"constexpr int AT_MAX_N = (\d+);", _src()).group(1))


def compiled_kernels():
    """every k_attn_* instantiation the library holds (a list, so that one launched from two sites shows)"""
    src = _src()
    out = [(name[2:],) for name in re.findall(r"hipLaunchKernelGGL\((k_attn_[a-z0-9_]+),", src)]
    assert not re.search(r"k_attn_[a-z0-9_]+\s*<", src), "a templated k_attn_* kernel needs its instantiations parsed here"
    named = set(re.findall(r"\bk_attn_[a-z0-9_]+", src))
    assert named == {"k_attn_fwd", "k_attn_bwd"}, named                    # a third k_attn_* kernel needs a parser and rows here
    assert out, "critic_attn.hip: launch sites not found"
    return out


class Row(NamedTuple):
    kernels: tuple      # the kernels this row must reach (forward and backward entries)
    shape: dict         # B, n, H
    label: str
    special: str        # "" | "diag" | "hot": how the operands are made


def big_samples(cus):
    """more samples than `cus` x 4 workgroups, + 11: the grid-stride turn, and a cross-workgroup sum of logit_sq over every workgroup"""
    return cus * BLOCKS_PER_CU + 11


def rows_for(cus=CUS):
    shapes = [(5, 2, 1, "n2", ""),                  # one other agent: out_i == val_j bit for bit; dsel / dkey from the regulariser alone
              (1, 3, 4, "n3-h4", ""),               # smallest head width, a single sample
              (67, 17, 2, "n17", ""),               # n one past 16; B a prime
              (27, 38, 1, "n38-h1", ""),            # the feeder's shape
              (27, 38, 4, "n38-h4", ""),
              (big_samples(cus), 38, 1, "big", ""),
              (5, 6, 1, "diag", "diag"),            # key_i = 50 sel_i / |sel_i|^2: an unmasked diagonal would take all the weight
              (5, 6, 1, "hot", "hot")]              # scaled logits reach +-100: without the max subtraction exp overflows
    both = (("attn_fwd",), ("attn_bwd",))
    return [Row(both, dict(B=B, n=n, H=H), tag, sp) for B, n, H, tag, sp in shapes]


ROWS = rows_for(CUS)
