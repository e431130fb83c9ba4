"""The compiled PPO kernels (mapdn_amd/csrc/ppo.hip) and the rows that reach them: test infrastructure of
tests/test_ppo_kernel_matrix_cpu.py (the rows cover the compiled set; the launch sites and argument limits; the float32 PyTorch fallback
against the float64 restatements below, which is where the bars come from) and tests/test_ppo_kernel_matrix_gpu.py (every row through the
C ABI against the same restatements).

The compiled set is parsed from the source (comments stripped), not restated: the `__global__` kernels named k_ppo_* and their launch
sites.  Rows:
    GAE rows (rows, n, S): one row; a short chain; a long chain with three live lanes; S > rows (every chain one row long); ragged with
    S n no multiple of 64; S n a small odd number past what the grid holds in one turn (cus x 8 workgroups x 256 threads).  done /
    last_step hold all four combinations in every row with at least four rows (the one-row case holds done + last_step), drawn so that
    chains pass through each.
    Loss rows rows x n in {1, 63, 65, 27 x 38, one past the grid's capacity}, each run with valid absent, all ones, mixed and all zeros
    (the loss and the gradient are then 0, not NaN), with planted ties: A = 0, masked actions, log_prob_new == old, V == V_old,
    |V - V_old| == eps exactly, and a run with eps_clip = 0, where rho == 1 sits on BOTH clip bounds at once.
Inputs are O(1) in magnitude: a wrong mask, stride or tie rule moves a result by ~0.1 of its scale or more.

Error measure: max |got - ref| over the output divided by max |ref| (for a loss: by the weighted mean of |term|, which a loss near 0 by
cancellation does not shrink).  Where the reference is exactly 0 (valid all zeros) the output must be exactly 0.

Bars.  The float32 PyTorch fallback (mapdn_amd.learner.ppo_gae_torch, ppo_policy_loss_torch, ppo_value_loss_torch with autograd) deviates
from the float64 restatements over these rows (256 CUs) by MEASURED below — GAE 2.04e-7, policy loss 8.89e-8, policy gradient 6.00e-7,
value loss 1.23e-7, value gradient 1.06e-7 —, measured on the CPU (tests/test_ppo_kernel_matrix_cpu.py::
test_the_float32_fallback_defines_the_bars re-measures and holds the recorded figures to it); the kernels' bar is BAR = 4 x that — 8.16e-7,
3.56e-7, 2.40e-6, 4.92e-7, 4.24e-7 —: contraction and another expf can each move a rounding, a logic error moves ~0.1."""
import math
import os
import re
from typing import NamedTuple

import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
CUS = 256                    # the CU count the CPU tests build the rows for (an MI355X); the GPU tests take the device's
THREADS, BLOCKS_PER_CU = 256, 8
GAMMA, LAMBDA, EPS_CLIP, COEF = 0.99, 0.95, 0.6, 2.0
EPS_EXACT = 0.5              # the value-loss rows: |V - V_old| == eps is planted with numbers both precisions hold exactly
KERNELS = {"k_ppo_gae", "k_ppo_policy_loss", "k_ppo_value_loss", "k_ppo_loss_finish"}

# largest deviation of the float32 PyTorch fallback from the float64 restatement over ROWS (CPU, measured): the kernels' bars are 4 x these
MEASURED = dict(gae=2.04e-7, policy_loss=8.89e-8, policy_grad=6.00e-7, value_loss=1.23e-7, value_grad=1.06e-7)
BAR = {k: 4.0 * v for k, v in MEASURED.items()}


def _src(name="ppo.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def compiled_kernels():
    """every k_ppo_* kernel the library holds, as the list of its launch sites' kernel names (one launched from two sites shows twice)"""
    src = _src()
    defined = set(re.findall(r"__global__[^;{]*?\b(k_ppo_[a-z0-9_]+)\s*\(", src))
    assert not re.search(r"k_ppo_[a-z0-9_]+\s*<", src), "a templated k_ppo_* kernel needs its instantiations parsed here"
    launched = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(k_ppo_[a-z0-9_]+)", src)
    named = set(re.findall(r"\bk_ppo_[a-z0-9_]+", src))
    assert named == defined, (named, defined)                              # every name is a kernel defined here
    assert set(launched) == defined, (launched, defined)                   # ... and is launched
    return launched


def capacity(cus=CUS):
    """threads of a full grid: what one turn of the grid-stride loops covers"""
    return cus * BLOCKS_PER_CU * THREADS


class GaeRow(NamedTuple):
    rows: int
    n: int
    S: int
    label: str
    kernels: tuple = ("k_ppo_gae",)
    entry: str = "mapdn_ppo_gae"


class LossRow(NamedTuple):
    kind: str            # "policy" | "value"
    rows: int
    n: int
    label: str

    @property
    def kernels(self):
        return (f"k_ppo_{self.kind}_loss", "k_ppo_loss_finish")

    @property
    def entry(self):
        return f"mapdn_ppo_{self.kind}_loss"


def big_stride(cus):
    """S (odd) with S x 3 a small odd number past the grid's capacity"""
    S = capacity(cus) // 3 + 1
    return S if S % 2 else S + 1


def big_loss_shape(cus):
    """(rows, n) with rows x n == capacity + 1"""
    e = capacity(cus) + 1
    n = next(k for k in (3, 5, 7, 1) if e % k == 0)
    return e // n, n


def gae_rows(cus=CUS):
    S = big_stride(cus)
    return [GaeRow(1, 1, 1, "one"), GaeRow(9, 3, 1, "short"), GaeRow(240, 3, 1, "long"), GaeRow(7, 3, 16, "s-gt-rows"),
            GaeRow(37, 38, 8, "ragged"), GaeRow(2 * S + S // 2, 3, S, "big")]


def loss_rows(cus=CUS):
    br, bn = big_loss_shape(cus)
    shapes = [(1, 1, "e1"), (21, 3, "e63"), (13, 5, "e65"), (27, 38, "n38"), (br, bn, "big")]
    return [LossRow(kind, r, n, f"{kind}-{tag}") for kind in ("policy", "value") for r, n, tag in shapes]


GAE_ROWS, LOSS_ROWS = gae_rows(CUS), loss_rows(CUS)
VALID_MODES = ("none", "ones", "mixed", "zeros")


# ---- inputs (float32, on the CPU generator: the same numbers on every device) -----------------------------------------------------
def flags(rows, g):
    """(done, last_step) [rows] f32 with all four combinations (rows >= 4): (0,0) mostly, so that chains run on through the others"""
    combo = torch.multinomial(torch.tensor([0.55, 0.15, 0.15, 0.15]), rows, replacement=True, generator=g)    # 0 none, 1 timeout, 2 done only, 3 both
    first = torch.randperm(4, generator=g)[:min(rows, 4)]
    combo[:first.numel()] = first if rows >= 4 else torch.tensor([3, 1, 2][:rows])
    done = ((combo == 2) | (combo == 3)).float()
    last = ((combo == 1) | (combo == 3)).float()
    return done, last


def gae_inputs(row, seed, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda: torch.randn(row.rows, row.n, generator=g)      # noqa: E731
    reward, value, next_value = r(), r(), r()
    done, last = flags(row.rows, g)
    return {k: v.to(device) for k, v in dict(reward=reward, value=value, next_value=next_value, done=done, last_step=last).items()}


def valid_of(mode, rows, g):
    if mode == "none":
        return None
    if mode == "ones":
        return torch.ones(rows)
    if mode == "zeros":
        return torch.zeros(rows)
    v = (torch.rand(rows, generator=g) < 0.6).float()
    v[0] = 1.0
    return v


def policy_inputs(row, seed, device="cpu"):
    """action / mean / log_std / avail / old / adv [rows, n] with planted ties by element index e: e % 7 == 0: A = 0; e % 11 == 3: the
    action is masked out; e % 5 == 1: log_std = 0 and old = the float32 log_prob_new (rho == 1 exactly; `tie` marks them); e % 13 == 5 /
    == 6: rho far above / below the clip range"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows, n = row.rows, row.n
    E = rows * n
    r = lambda: torch.randn(E, generator=g)      # noqa: E731
    action, mean, adv = torch.tanh(r()), 0.5 * r(), r()
    log_std = 0.2 * r()
    idx = torch.arange(E)
    far_up, far_down = idx % 13 == 5, idx % 13 == 6
    tie = (idx % 5 == 1) & ~far_up & ~far_down
    log_std[tie] = 0.0
    std = log_std.exp()
    lp = -((action - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))       # float32, as the fallback forms it
    old = lp + 0.3 * r()
    old[tie] = lp[tie]
    old[far_up] -= 2.0
    old[far_down] += 2.0
    adv[idx % 7 == 0] = 0.0
    avail = torch.ones(E)
    avail[idx % 11 == 3] = 0.0
    out = dict(action=action, mean=mean, log_std=log_std, avail=avail, old=old, adv=adv)
    out = {k: v.view(rows, n).to(device) for k, v in out.items()}
    out["tie"] = (tie & (avail != 0)).view(rows, n).to(device)
    return out


def value_inputs(row, seed, device="cpu"):
    """v / v_old / reward / v_next [rows, n], done [rows]; v and v_old are multiples of 1/8 so that the planted cases are exact in both
    precisions: e % 5 == 1: V == V_old; e % 7 == 2 / == 3: V - V_old == +/- EPS_EXACT; e % 11 == 4: far outside the clip range"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows, n = row.rows, row.n
    E = rows * n
    r = lambda: torch.randn(E, generator=g)      # noqa: E731
    v_old = torch.round(8 * r()) / 8
    v = v_old + torch.round(8 * 0.4 * r()) / 8
    idx = torch.arange(E)
    v[idx % 5 == 1] = v_old[idx % 5 == 1]
    v[idx % 7 == 2] = v_old[idx % 7 == 2] + EPS_EXACT
    v[idx % 7 == 3] = v_old[idx % 7 == 3] - EPS_EXACT
    v[idx % 11 == 4] = v_old[idx % 11 == 4] + 2.0
    reward, v_next = r(), r()
    done = (torch.rand(rows, generator=g) < 0.3).float()
    out = dict(v=v.view(rows, n), v_old=v_old.view(rows, n), reward=reward.view(rows, n), v_next=v_next.view(rows, n), done=done)
    return {k: t.to(device) for k, t in out.items()}


# ---- float64 restatements ---------------------------------------------------------------------------------------------------------
def gae_rowloop64(inp, S, gamma=GAMMA, lam=LAMBDA):
    """learning_algorithms/ppo.py:46-54 as written — a loop over the rows, newest first — with `last_advantages` kept per chain (row
    index modulo S); float64.  Small rows only."""
    rw, v, nv, done, last = (inp[k].double().cpu() for k in ("reward", "value", "next_value", "done", "last_step"))
    rows, n = rw.shape
    adv = torch.zeros(rows, n, dtype=torch.float64)
    last_adv = [torch.zeros(n, dtype=torch.float64) for _ in range(S)]
    for i in reversed(range(rows)):
        mask = 1.0 - done[i] if last[i] else 1.0
        delta = rw[i] + gamma * nv[i] * mask - v[i]
        last_adv[i % S] = delta + gamma * lam * last_adv[i % S] * mask
        adv[i] = last_adv[i % S]
    return adv


def gae_padded64(inp, S, gamma=GAMMA, lam=LAMBDA):
    """the same on rows padded to whole steps and viewed [T, S, n] (a padded row has delta 0 and comes last in its chain): float64, any size"""
    rw, v, nv, done, last = (inp[k].double() for k in ("reward", "value", "next_value", "done", "last_step"))
    rows, n = rw.shape
    T = -(-rows // S)
    pad = T * S - rows
    mask = torch.where(last != 0, 1.0 - done, torch.ones_like(done))
    delta = rw + gamma * nv * mask.unsqueeze(1) - v
    delta = torch.cat((delta, delta.new_zeros(pad, n))).view(T, S, n)
    mask = torch.cat((mask, mask.new_ones(pad))).view(T, S, 1)
    out = torch.zeros_like(delta)
    run = delta.new_zeros(S, n)
    for t in reversed(range(T)):
        run = delta[t] + gamma * lam * run * mask[t]
        out[t] = run
    return out.view(T * S, n)[:rows]


def _weights64(valid, rows, n, device):
    if valid is None:
        return torch.ones(rows, 1, dtype=torch.float64, device=device), 1.0 / (rows * n)
    vf = valid.double().view(rows, 1)
    return vf, 1.0 / (float(vf.sum().clamp(min=1.0)) * n)


def policy_ref64(inp, valid, eps_clip=EPS_CLIP, exact_ties=False):
    """(loss, d loss / d mean, scale of the loss) in float64 with autograd.  exact_ties: the planted log_prob_new == old elements take the
    float64 log_prob as their old one, so that rho == 1 exactly here as it is in float32 there (the eps_clip = 0 runs, where 1 is both bounds)"""
    a, ls, av, old, adv = (inp[k].double() for k in ("action", "log_std", "avail", "old", "adv"))
    mean = inp["mean"].double().requires_grad_(True)
    rows, n = a.shape
    std = ls.exp()
    lp = -((a - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))
    if exact_ties:
        old = torch.where(inp["tie"], lp.detach(), old)
    m = 1.0 - (av == 0).double()
    rho = torch.exp(m * lp - m * old)
    term = torch.min(rho * adv, torch.clamp(rho, 1 - eps_clip, 1 + eps_clip) * adv)
    w, sc = _weights64(valid, rows, n, a.device)
    loss = -(w * term).sum() * sc
    (grad,) = torch.autograd.grad(loss, mean)
    return loss.detach(), grad, float((w * term.detach().abs()).sum() * sc)


def value_ref64(inp, valid, gamma=GAMMA, eps_clip=EPS_EXACT, coef=COEF):
    """(loss, d loss / d V, scale of the loss) in float64 with autograd"""
    vo, rw, vn, done = (inp[k].double() for k in ("v_old", "reward", "v_next", "done"))
    v = inp["v"].double().requires_grad_(True)
    rows, n = vo.shape
    ret = rw + gamma * (1 - done.view(rows, 1)) * vn
    vc = vo + torch.clamp(v - vo, -eps_clip, eps_clip)
    term = torch.max((v - ret).pow(2), (vc - ret).pow(2))
    w, sc = _weights64(valid, rows, n, vo.device)
    loss = coef * (w * term).sum() * sc
    (grad,) = torch.autograd.grad(loss, v)
    return loss.detach(), grad, float(coef * (w * term.detach()).sum() * sc)


def rel_err(got, ref, scale=None):
    """max |got - ref| / max |ref| (or / scale); a reference that is exactly zero demands exactly zero"""
    got, ref = got.double(), ref.double()
    s = float(ref.abs().max()) if scale is None else float(scale)
    if s == 0.0:
        assert float(got.abs().max()) == 0.0, "the reference is exactly 0 and the output is not"
        return 0.0
    return float((got - ref).abs().max()) / s
