"""What a traditional baseline (droop_actions, opf_actions, opf_probe) must leave alone, shared by the GPU tests of both: the env's state,
its counters and its next step().  Test infrastructure only; the baseline's call is an argument."""
import numpy as np
import torch


def env_state(env):
    """(load_p, load_q, sgen_p, s_max) of every env: what the next step() solves with"""
    lp, lq = env.loads()
    pv = env.results(("sgen_p",))["sgen_p"]
    return lp.cpu().numpy(), lq.cpu().numpy(), pv.cpu().numpy(), env.profile_stats()[1]


def snapshot(env):
    torch.cuda.synchronize()
    out = dict(obs=env.get_obs().clone(), state=env.get_state().clone(), returns=env.episode_returns().clone(),
               starts=env.start_rows().clone(), stats=env.stats(), loads=torch.cat(env.loads(), 1).clone())
    out.update({k: v.clone() for k, v in env.results().items()})
    return out


def same(x, y):
    for k in x:
        if isinstance(x[k], torch.Tensor):
            assert torch.equal(x[k], y[k]), k
        else:
            assert x[k] == y[k], k


def check_state_untouched_and_step_agrees(make_env, baseline, after_solve, B=24):
    """make_env(B): a fresh env; baseline(env) -> (actions, status, vm_pu) as torch tensors.  From noisy resets and two random-action
    steps (and, after_solve, a solve() that leaves Sbus stale): the call changes nothing a twin env T does not have, step() with its
    actions gives the twin's bits, and the committed |V| of the envs it solved are the |V| it returned."""
    A, T = make_env(B), make_env(B)
    try:
        A.reset(); T.reset()
        rng = np.random.default_rng(3)
        for _ in range(2):
            act = torch.as_tensor(rng.uniform(-0.8, 0.8, (B, A.n_sgen)), device=A.device)
            A.step(act); T.step(act)
        if after_solve:
            lp, lq, pv, _ = env_state(A)
            for env in (A, T):
                env.solve(lp * 1.3, lq, pv, np.zeros_like(pv))
        before = snapshot(A)
        a, st, vm = baseline(A)
        same(before, snapshot(A))
        same(before, snapshot(T))
        r1, t1, i1 = [x.clone() for x in A.step(a)]
        r2, t2, i2 = [x.clone() for x in T.step(a)]
        assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(i1, i2)
        assert torch.equal(A.get_obs(), T.get_obs())
        ok = st <= 1
        assert ok.any()
        committed = A.results(("vm_pu",))["vm_pu"]
        assert float((committed[ok] - vm[ok]).abs().max()) < 1e-12
        r1, _, i1 = [x.clone() for x in A.step(a)]
        r2, _, i2 = [x.clone() for x in T.step(a)]
        assert torch.equal(r1, r2) and torch.equal(i1, i2)
    finally:
        A.close(); T.close()
