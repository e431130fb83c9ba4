"""The compiled twin-critic kernels (csrc/critic_twin.hip, compiled inside critic.hip) and the rows that reach them: test infrastructure of
tests/test_twin_kernel_matrix_cpu.py (the rows cover the compiled set, the geometry query reports each row's kernel) and
tests/test_twin_kernel_matrix_gpu.py (every row against autograd through the float64 modules, the critic evaluated twice: flag 0 and 1).

The compiled set is parsed from the launch sites of the source (comments stripped), not restated.  A kernel is a tuple:
    ("twin_fwd",)          k_twin_fwd                (which of v1 / v2 / vmin it writes is a run-time choice: a row names its outputs)
    ("twin_mse",)          k_twin_mse                (256 threads)"""
import os
import re
from typing import NamedTuple

from mapdn_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests ask the geometry query for (an MI355X); the GPU tests take the device's
HP, HW, TP = 4416, 4354, 4480     # the head's grads block / its documented part; the twin's block ahead of dper_n (HP | d flag_col [64])
LDS_MAX = 160 * 1024
MAX_N = 88


def _src(name="critic_twin.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def compiled_kernels():
    """every k_twin_* instantiation the library holds (a list, so that one launched from two sites shows)"""
    src = _src()
    out = [("twin_fwd",) for _ in re.findall(r"hipLaunchKernelGGL\(k_twin_fwd,", src)]
    out += [("twin_mse",) for _ in re.findall(r"hipLaunchKernelGGL\(k_twin_mse,", src)]
    assert not re.search(r"k_twin_[a-z0-9_]+\s*<", src), "a templated k_twin_* kernel needs its instantiations parsed here"
    named = set(re.findall(r"\bk_twin_[a-z0-9_]+", src))
    assert named == {"k_twin_fwd", "k_twin_mse"}, named                    # a third k_twin_* kernel needs a parser and rows here
    assert out, "critic_twin.hip: launch sites not found"
    return out


class Row(NamedTuple):
    kernel: tuple       # the kernel this row must reach
    entry: str          # the C entry point that launches it
    shape: dict         # nb, n (rows = nb * n)
    opts: dict          # twin_fwd: outputs (names out of v1, v2, vmin); twin_mse: wrow (bool)
    label: str


def big_groups(cus, nt):
    """more groups than `cus` workgroups of nt threads have wavefronts, not a multiple of the wavefront count"""
    return cus * (nt // 64) + 53


def rows_for(cus=CUS):
    """n in {1, 6, 38, 88}; fewer groups than wavefronts (idle waves), group counts that are not a multiple of the wavefront count, more
    workgroups' worth of groups than CUs; wrow null and given; each nullable output null and not"""
    out = []
    shapes = [(203, 1, "n1"), (3, 6, "idle"), (333, 6, "n6"), (27, 38, "n38"), (35, 88, "n88"), (big_groups(cus, 256), 6, "big")]
    for nb, n, tag in shapes:
        for wrow in (False, True):
            out.append(Row(("twin_mse",), "mapdn_critic_twin_mse", dict(nb=nb, n=n), dict(wrow=wrow), f"mse-{tag}-{'w' if wrow else 'now'}"))
    outs = [("v1", "v2", "vmin"), ("vmin",), ("v1",), ("v2",), ("v1", "v2")]
    fwd_shapes = [(5, 6, "tail"), (203, 1, "n1"), (27, 38, "n38"), (35, 88, "n88"), (cus * 2 * 4 + 11, 38, "big")]
    for k, (nb, n, tag) in enumerate(fwd_shapes):
        for o in (outs if tag in ("tail", "big") else [outs[0], outs[1 + k % 4]]):
            out.append(Row(("twin_fwd",), "mapdn_critic_twin_forward", dict(nb=nb, n=n), dict(outputs=o), f"fwd-{tag}-{'+'.join(o)}"))
    return out


ROWS = rows_for(CUS)


def reported_kernel(row, cus=CUS):
    """the kernel the library launches for a row; for the loss kernel None when the geometry query refuses the shape, and its thread
    count must be the compiled 256"""
    if row.kernel[0] == "twin_fwd":
        return row.kernel
    g = _lib.critic_twin_geometry(row.shape["nb"] * row.shape["n"], row.shape["n"], cus)
    return None if g is None or g[0] != 256 else ("twin_mse",)
