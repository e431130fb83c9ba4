"""The compiled learner kernels (csrc/policy.hip, csrc/policy_bwd.hip, csrc/critic.hip) and the rows that reach them: test infrastructure of
tests/test_learner_kernel_matrix_cpu.py (the rows cover the compiled set, every row's geometry query reports its kernel) and
tests/test_learner_kernel_matrix_gpu.py (every row against the PyTorch modules in float64).

The compiled set is parsed from the launch sites of the sources (comments stripped), not restated.  A kernel is a tuple:
    ("policy_fwd", P)  ("policy_fwd2", P)           k_policy_fwd<P> / k_policy_fwd2<P>, P threads per workgroup
    ("head_fwd", BC)   ("head_bwd", BC, MODE, NT)   k_head_fwd<BC> / k_head_bwd<BC, MODE, NT>
    ("policy_bwd",)    ("ln64_fwd", RELU, BC)  ("ln64_bwd", RELU, BC)  ("relu_dot64_fwd",)  ("relu_dot64_bwd",)
The policy forward decides two more things at run time that change the path through the kernel — whether the id columns of fc1 sit in
LDS (ids_lds) and, in k_policy_fwd2, the load path of an odd observation width — so its rows are cells
("policy_fwd2", P, ids_lds, odd) and cover every combination; compiled_of() gives the compiled kernel of a cell."""
import os
import re
from typing import NamedTuple

from mapdn_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests ask the geometry queries for (an MI355X); the GPU tests take the device's
HP, HW = 4416, 4354          # floats per head partial / grads block, and how many of them are documented (the rest is pad)
PBP, PBW = 512, 449          # the same for mapdn_policy_backward's `small` and its partials
LDS_MAX = 160 * 1024


# ---- the compiled set ----------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def _b(s):
    return int(s == "true")


def policy_fwd_kernels():
    src = _src("policy.hip")
    out = [("policy_fwd2" if k.endswith("2") else "policy_fwd", int(p)) for k, p in re.findall(r"MAPDN_POLICY_LAUNCH\((k_policy_fwd2?),\s*(\d+)\)", src)]
    assert out, "no MAPDN_POLICY_LAUNCH(k_policy_fwd..., P) in policy.hip"
    return out


def ln64_kernels():
    src = _src("policy.hip")
    out = [("ln64_" + d, _b(r), _b(bc)) for d, r, bc in re.findall(r"hipLaunchKernelGGL\(\(k_ln64_(fwd|bwd)<(true|false),\s*(true|false)>\)", src)]
    out += [("relu_dot64_" + d,) for d in re.findall(r"hipLaunchKernelGGL\(k_relu_dot64_(fwd|bwd),", src)]
    assert out, "no k_ln64_* / k_relu_dot64_* launch in policy.hip"
    return out


def head_kernels():
    src = _src("critic.hip")
    fwd = [("head_fwd", _b(bc)) for bc in re.findall(r"hipLaunchKernelGGL\(k_head_fwd<(true|false)>", src)]
    nts = [int(x) for x in re.findall(r"head_bwd_launch_nt<BC,\s*MODE,\s*(\d+)>\(", src)]            # what head_bwd_launch dispatches to
    modes = [(_b(bc), int(m)) for bc, m in re.findall(r"head_bwd_launch<(true|false),\s*(\d+)>\(", src)]  # what the entry points ask for
    assert fwd and nts and modes, "critic.hip: launch sites not found"
    return fwd + [("head_bwd", bc, m, nt) for bc, m in modes for nt in nts]


def policy_bwd_kernels():
    n = len(re.findall(r"hipLaunchKernelGGL\(k_policy_bwd,", _src("policy_bwd.hip")))
    assert n, "no k_policy_bwd launch in policy_bwd.hip"
    return [("policy_bwd",)] * n


def compiled_kernels():
    """every learner kernel instantiation the library holds (a list, so that one listed twice in the sources shows)"""
    return policy_fwd_kernels() + ln64_kernels() + head_kernels() + policy_bwd_kernels()


def compiled_of(kernel):
    """the compiled instantiation a row's cell runs (policy forward: ids_lds and the parity of the width are run-time)"""
    return kernel[:2] if kernel[0] in ("policy_fwd", "policy_fwd2") else kernel


# ---- the rows ------------------------------------------------------------------------------------------------------------------
class Row(NamedTuple):
    kernel: tuple       # the cell this row must reach
    entry: str          # the C entry point that launches it
    shape: dict         # obs_dim, id_dim (policy forward) | rows (read rows) | nb, n (formed rows: rows = nb * n)
    env: dict           # switches: MAPDN_POLICY_FWD_V1, MAPDN_HEAD_BWD_THREADS ({} = the library's own choice)
    label: str


def big_rows(cus, nt=512):
    """read rows with more 16-row tiles than `cus` workgroups of nt threads have wavefronts, not a multiple of 16"""
    return cus * (nt // 64) * 16 + 16 * 37 + 5


def big_groups(cus, nt=512):
    """formed rows: more groups than `cus` workgroups of nt threads have wavefronts, not a multiple of the wavefront count"""
    return cus * (nt // 64) + 53


# observation widths of the policy forward: (obs_dim, id_dim) -> what policy_geometry must answer.  Per geometry: widths of one k chunk
# (1, 7, 16), ragged and full last chunks (o % 16 in {0, 1, 15}), o % 4 != 0, and the last width that fits.  With an id the row count
# cycles through id_dim agents.
POLICY_WIDTHS = {
    (512, 1, 0): [(16, 6), (26, 6), (58, 22), (58, 0), (80, 22), (64, 38), (96, 0)],
    (512, 1, 1): [(1, 6), (7, 6), (17, 22), (31, 38), (63, 38), (95, 0)],
    (512, 0, 0): [(66, 38), (82, 38), (96, 38)],
    (512, 0, 1): [(65, 38), (81, 38), (95, 38)],
    (256, 1, 0): [(98, 38), (112, 22), (128, 38), (144, 22), (176, 0)],
    (256, 1, 1): [(97, 0), (97, 38), (111, 22), (113, 38), (175, 0)],
    (256, 0, 0): [(130, 38), (160, 38), (176, 38)],
    (256, 0, 1): [(129, 38), (143, 38), (161, 38), (175, 38)],
}
POLICY_REFUSED = [(177, 38), (177, 0), (192, 0), (400, 38)]       # no launch shape: the caller keeps the PyTorch modules
POLICY_ENTRIES = ("mapdn_policy_forward", "mapdn_policy_forward_train")


def policy_rows():
    out = []
    for form, env in (("policy_fwd2", {}), ("policy_fwd", {"MAPDN_POLICY_FWD_V1": "1"})):
        for (pt, il, odd), widths in POLICY_WIDTHS.items():
            for o, ids in widths:
                out.append(Row((form, pt, il, odd), "mapdn_policy_forward", dict(obs_dim=o, id_dim=ids), dict(env), f"{form}-{pt}-lds{il}-{o}+{ids}"))
    return out


HEAD_ENTRY = {0: "mapdn_critic_head_backward", 1: "mapdn_critic_head_backward", 2: "mapdn_critic_head_backward_dot", 3: "mapdn_critic_head_mse"}


def head_rows(cus=CUS):
    """every k_head_bwd<BC, MODE, NT> forced with MAPDN_HEAD_BWD_THREADS: read rows with rows % 16 != 0, fewer tiles than wavefronts
    (one workgroup, idle waves) and more workgroups' worth than CUs; formed rows with n in {1, 6, 38, 88} (88 where the [n][64]
    accumulators of NT / 64 wavefronts fit LDS) and a group count that is not a multiple of the wavefront count; plus rows that leave the
    choice to the library (env {}) on either side of its threshold of 8 units per CU"""
    out = []
    for nt in (256, 512):
        env = {"MAPDN_HEAD_BWD_THREADS": str(nt)}
        for mode in (0, 1, 2, 3):
            for rows, tag in ((40, "idle"), (4101, "ragged"), (big_rows(cus, nt), "big")):
                out.append(Row(("head_bwd", 0, mode, nt), HEAD_ENTRY[mode], dict(rows=rows), env, f"read-m{mode}-{nt}-{tag}"))
            formed = [(203, 1, "n1"), (3, 6, "idle"), (333, 6, "n6"), (27, 38, "n38"), (big_groups(cus, nt), 6, "big")]
            if nt == 256 or mode == 2:
                formed.append((35, 88, "n88"))
            for nb, n, tag in formed:
                out.append(Row(("head_bwd", 1, mode, nt), HEAD_ENTRY[mode], dict(nb=nb, n=n), env, f"formed-m{mode}-{nt}-{tag}"))
    for mode in (0, 2):
        out.append(Row(("head_bwd", 0, mode, 256), HEAD_ENTRY[mode], dict(rows=cus * 8 * 16 - 16), {}, f"read-m{mode}-auto256"))
        out.append(Row(("head_bwd", 0, mode, 512), HEAD_ENTRY[mode], dict(rows=cus * 8 * 16 - 15), {}, f"read-m{mode}-auto512"))
        out.append(Row(("head_bwd", 1, mode, 256), HEAD_ENTRY[mode], dict(nb=cus * 8 - 1, n=6), {}, f"formed-m{mode}-auto256"))
        out.append(Row(("head_bwd", 1, mode, 512), HEAD_ENTRY[mode], dict(nb=cus * 8, n=6), {}, f"formed-m{mode}-auto512"))
    return out


def other_rows(cus=CUS):
    out = []
    for bc in (0, 1):
        for shape, tag in (((dict(rows=17), "tail"), (dict(rows=cus * 2 * 4 * 16 + 16 * 9 + 3), "big")) if not bc else
                           ((dict(nb=5, n=6), "tail"), (dict(nb=cus * 2 * 4 + 11, n=38), "big"))):
            out.append(Row(("head_fwd", bc), "mapdn_critic_head_forward", shape, {}, f"head_fwd-{bc}-{tag}"))
    for rows, tag in ((1, "one"), (4101, "ragged"), (cus * 4 * 16 + 16 * 21 + 7, "big")):
        out.append(Row(("policy_bwd",), "mapdn_policy_backward", dict(rows=rows), {}, f"policy_bwd-{tag}"))
    for d in ("fwd", "bwd"):
        for relu in (0, 1):
            e = "mapdn_layernorm64_" + ("forward" if d == "fwd" else "backward")
            out.append(Row(("ln64_" + d, relu, 0), e, dict(rows=4101), {}, f"ln64_{d}-relu{relu}-read"))
            out.append(Row(("ln64_" + d, relu, 0), e, dict(rows=cus * 8 * 16 + 77), {}, f"ln64_{d}-relu{relu}-read-big"))
            e = "mapdn_layernorm64_bc_" + ("forward" if d == "fwd" else "backward")
            out.append(Row(("ln64_" + d, relu, 1), e, dict(nb=107, n=38), {}, f"ln64_{d}-relu{relu}-formed"))
        out.append(Row(("relu_dot64_" + d,), "mapdn_relu_dot64_" + ("forward" if d == "fwd" else "backward"), dict(rows=4101), {}, f"relu_dot64_{d}"))
        out.append(Row(("relu_dot64_" + d,), "mapdn_relu_dot64_" + ("forward" if d == "fwd" else "backward"), dict(rows=cus * 8 * 16 + 77), {},
                       f"relu_dot64_{d}-big"))
    return out


def rows_for(cus=CUS):
    """the rows with their CU-dependent shapes sized for `cus`; same order and labels for every cus"""
    return policy_rows() + head_rows(cus) + other_rows(cus)


ROWS = rows_for(CUS)


def total_rows(shape):
    return shape["rows"] if "rows" in shape else shape["nb"] * shape["n"]


# ---- what the library reports for a row ------------------------------------------------------------------------------------------
def reported_kernel(row, cus=CUS, environ=None):
    """the cell the library's geometry queries report for a row under the row's switches (None: refused).  environ: the mapping the
    switches are set in (os.environ by default — the library reads them with getenv at every call)"""
    env = os.environ if environ is None else environ
    saved = {k: env.get(k) for k in ("MAPDN_POLICY_FWD_V1", "MAPDN_HEAD_BWD_THREADS")}
    try:
        for k in saved:
            env.pop(k, None)
        env.update(row.env)
        kind = row.kernel[0]
        if kind in ("policy_fwd", "policy_fwd2"):
            g = _lib.policy_forward_geometry(row.shape["obs_dim"], row.shape["id_dim"])
            if g is None:
                return None
            form = "policy_fwd" if row.env.get("MAPDN_POLICY_FWD_V1", "0") not in ("", "0") else "policy_fwd2"
            return (form, g[0], g[1], row.shape["obs_dim"] & 1)
        if kind == "head_bwd":
            formed = "nb" in row.shape
            g = _lib.critic_head_backward_geometry(total_rows(row.shape), row.shape.get("n", 1), formed, row.kernel[2], cus)
            return None if g is None else ("head_bwd", int(formed), row.kernel[2], g[0])
        if kind == "head_fwd" or kind.startswith("ln64_"):
            return row.kernel[:-1] + (int("nb" in row.shape),)             # the entry point's per_n argument decides BC
        return row.kernel
    finally:
        for k, v in saved.items():
            env.pop(k, None)
            if v is not None:
                env[k] = v
