"""The compiled counterfactual-baseline kernels (csrc/critic_cf.hip, compiled inside critic.hip) and the rows that reach them: test
infrastructure of tests/test_cf_kernel_matrix_cpu.py (the rows cover the compiled set; the one launch site and its argument limits) and
tests/test_cf_kernel_matrix_gpu.py (every row against the float64 modules evaluated S times).

The compiled set is parsed from the launch sites of the source (comments stripped), not restated.  A kernel is a tuple:
    ("cf_baseline",)       k_cf_baseline             (whether v0 is written is a run-time choice: every row runs with and without)
The launch has no chooser (256 threads, min(ceil(tiles / 4), 2 CUs' worth) workgroups, no LDS), hence no geometry query."""
import os
import re
from typing import NamedTuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests build the rows for (an MI355X); the GPU tests take the device's
S_MAX = 64


def _src(name="critic_cf.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def compiled_kernels():
    """every k_cf_* instantiation the library holds (a list, so that one launched from two sites shows)"""
    src = _src()
    out = [("cf_baseline",) for _ in re.findall(r"hipLaunchKernelGGL\(k_cf_baseline,", src)]
    assert not re.search(r"k_cf_[a-z0-9_]+\s*<", src), "a templated k_cf_* kernel needs its instantiations parsed here"
    named = set(re.findall(r"\bk_cf_[a-z0-9_]+", src))
    assert named == {"k_cf_baseline"}, named                               # a second k_cf_* kernel needs a parser and rows here
    assert out, "critic_cf.hip: launch sites not found"
    return out


class Row(NamedTuple):
    kernel: tuple       # the kernel this row must reach
    entry: str          # the C entry point that launches it
    shape: dict         # n, rows, S
    label: str


def big_groups(cus):
    """groups of 38 rows such that there are more 16-row tiles than `cus` x 2 workgroups have wavefronts, + 11: the grid-stride turn"""
    return cus * 2 * 4 + 11


def rows_for(cus=CUS):
    shapes = [(1, 203, 1, "n1-tail"),             # rows not a multiple of 16
              (6, 3 * 6, 10, "idle"),             # fewer rows than one workgroup's wavefronts have tiles
              (38, 27 * 38, 10, "n38"),           # the default case
              (38, 27 * 38, 2, "n38-s2"),         # small S
              (6, 5 * 6, S_MAX, "smax"),          # the S limit
              (38, big_groups(cus) * 38, 10, "big")]
    return [Row(("cf_baseline",), "mapdn_critic_head_counterfactual", dict(n=n, rows=rows, S=S), tag) for n, rows, S, tag in shapes]


ROWS = rows_for(CUS)
