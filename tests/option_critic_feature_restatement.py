"""Restatement of what csrc/oc_mlp.hip and OptionCriticAgent's cart-pole device path compute (TEST INFRASTRUCTURE ONLY): the
OptionCriticNet forward (network_heads.py:105-127 over a two-layer FCBody, network_bodies.py:50-73), the rollout with the option
and action draws made by inverse CDF of given uniforms (OptionCritic_agent.py:29-93) over envs.CartPole, which is imported, not
restated, and one update (OptionCritic_agent.py:95-119 with torch.optim.RMSprop's step, its running average carried from update
to update).  fp64 by default; dtype=torch.float32 runs the same arithmetic in fp32 (the decision-margin test).
tests/test_option_critic_feature_host.py pins it to the reference's own run (tests/golden/option_critic_feature/) before a GPU test
leans on it.  Parameters are dicts keyed like OptionCriticNet.state_dict()."""
import numpy as np
import torch

from nstep_feature_restatement import returns, rmsprop_step, to_t      # noqa: F401  (the same scan, optimiser step, conversion)

F64 = torch.float64
_GATES = {"relu": torch.relu, "tanh": torch.tanh}
# in the order of dra_oc_mlp_net's offsets: w1 b1 w2 b2 wq bq wp bp wb bb
KEYS = ("body.layers.0.weight", "body.layers.0.bias", "body.layers.1.weight", "body.layers.1.bias", "fc_q.weight", "fc_q.bias",
        "fc_pi.weight", "fc_pi.bias", "fc_beta.weight", "fc_beta.bias")
N_ACTIONS = 2


def init_params(hidden, seed, n_options, state_dim=4, n_actions=N_ACTIONS):
    """float32 numpy parameters, O(0.3) scale: option values, terminations and policies that differ between rows."""
    rs = np.random.RandomState(seed)
    mk = lambda *shape, scale=0.3: (rs.randn(*shape) * scale).astype(np.float32)
    return {"body.layers.0.weight": mk(hidden, state_dim, scale=0.8), "body.layers.0.bias": mk(hidden, scale=0.1),
            "body.layers.1.weight": mk(hidden, hidden, scale=0.25), "body.layers.1.bias": mk(hidden, scale=0.1),
            "fc_q.weight": mk(n_options, hidden, scale=0.3), "fc_q.bias": mk(n_options, scale=0.05),
            "fc_pi.weight": mk(n_options * n_actions, hidden, scale=0.5), "fc_pi.bias": mk(n_options * n_actions, scale=0.1),
            "fc_beta.weight": mk(n_options, hidden, scale=0.5), "fc_beta.bias": mk(n_options, scale=0.1)}


def forward(p, obs, gate="relu", keep=None):
    """(q [n, O], beta [n, O], intra-option logits [n, O, A]) in the dtype of the parameters; `keep` (a dict) receives the two
    layers' pre-activations."""
    dt = p["fc_q.weight"].dtype
    g = _GATES[gate]
    lin = torch.nn.functional.linear
    x = torch.as_tensor(np.asarray(obs), dtype=dt)
    z1 = lin(x, p["body.layers.0.weight"], p["body.layers.0.bias"])
    z2 = lin(g(z1), p["body.layers.1.weight"], p["body.layers.1.bias"])
    if keep is not None:
        keep["z1"], keep["z2"] = z1.detach(), z2.detach()
    phi = g(z2)
    n_opt = p["fc_q.weight"].shape[0]
    return (lin(phi, p["fc_q.weight"], p["fc_q.bias"]), torch.sigmoid(lin(phi, p["fc_beta.weight"], p["fc_beta.bias"])),
            lin(phi, p["fc_pi.weight"], p["fc_pi.bias"]).view(-1, n_opt, N_ACTIONS))


def _seq_sum(x):
    return np.cumsum(x)[-1]        # (index order, one rounding per addition in x's dtype)


def inv_cdf(p, u):
    """Categorical(probs=p) by inverse CDF at u: the row divided by its sum (index order), then the first k whose running sum
    exceeds u, the last index when none does.  -> (k, the normalised row, the smallest |boundary - u| over the inner boundaries)."""
    p = p / _seq_sum(p)
    cum = np.cumsum(p)
    hit = np.nonzero(cum > u)[0]
    k = int(hit[0]) if hit.size else p.size - 1
    gap = float(np.abs(cum[:-1].astype(np.float64) - float(u)).min()) if p.size > 1 else float("inf")
    return k, p, gap


def categorical(x, u):
    """Categorical(logits=x): the inverse-CDF draw at u, log pi of it, the entropy.  -> (action, log_pi_a, entropy, gap)."""
    ft = x.dtype.type
    m = x.max()
    lse = m + np.log(_seq_sum(np.exp(x - m)))
    lp = (x - lse).astype(ft)
    p = np.exp(lp).astype(ft)
    ent = -_seq_sum(p * lp)
    cum = np.cumsum(p)
    hit = np.nonzero(cum > u)[0]
    a = int(hit[0]) if hit.size else x.size - 1
    return a, lp[a], ent, float(np.abs(cum[:-1].astype(np.float64) - float(u)).min())


def midpoint(probs, k):
    """The uniform in the middle of category k's interval of the normalised row `probs`: what makes inv_cdf return k."""
    cum = np.concatenate([[0.0], np.cumsum(np.asarray(probs, dtype=np.float64))])
    return np.float32(0.5 * (cum[k] + cum[k + 1]))


def rollout(params, target_params, envs, raw_states, t_len, eps, uniform, prev_option, is_initial, gate="relu", step0=0,
            reward_coef=1.0, dtype=F64, force_option=None):
    """OptionCritic_agent.py:55-93 over envs.CartPole objects (stepped with DummyVecEnv's auto reset) with eps [T] and uniform
    [T, N, 3] (fresh option, continued option, action) given.  Returns float32 state [T, N, 4]; q / beta [T, N, O], the chosen
    option's logits [T, N, A], log_pi_a / entropy [T, N] (fp64 arrays of the run's dtype values); int64 option / prev_option /
    action [T, N]; float32 init / reward / mask [T, N]; bootstrap [N] from the TARGET parameters; `events` (step counter,
    environment, episodic return) in (step, environment) order; `raw_states`; the carried state after the rollout
    (`prev_option_out`, `is_initial_out`); `margin`: the smallest gap between a uniform that decided something and a boundary of
    its CDF; `q_gap`: the smallest gap between the two largest option values of a row.  `force_option` (a test input, not a
    feature): every row takes this option whatever was drawn."""
    ft = np.float64 if dtype is F64 else np.float32
    p, pt = to_t(params, dtype), to_t(target_params, dtype)
    n = len(envs)
    n_opt = int(np.asarray(params["fc_q.weight"]).shape[0])
    keys = ("state", "q", "beta", "logits", "option", "prev_option", "action", "init", "log_pi_a", "entropy", "reward", "mask")
    out = {k: [] for k in keys}
    events, margin, q_gap = [], float("inf"), float("inf")
    raw = np.asarray(raw_states, dtype=np.float64)
    prev, init = np.asarray(prev_option, dtype=np.int64).copy(), np.asarray(is_initial).astype(bool).copy()
    eps, uniform = np.asarray(eps, dtype=np.float32), np.asarray(uniform, dtype=np.float32)
    one = ft(1.0)
    with torch.no_grad():
        for t in range(t_len):
            x = raw.astype(np.float32)
            q, beta, logits = [v.numpy() for v in forward(p, x, gate)]
            e = ft(eps[t])
            base, top = e / ft(n_opt), one - e + e / ft(n_opt)
            row = {k: [] for k in ("logits", "option", "action", "log_pi_a", "entropy")}
            for i in range(n):
                g = int(np.argmax(q[i]))
                top2 = np.sort(q[i].astype(np.float64))[-2:]
                q_gap = min(q_gap, float(top2[1] - top2[0]))
                pi_opt = np.full(n_opt, base, dtype=ft)
                pi_opt[g] = top
                keep = np.zeros(n_opt, dtype=ft)
                keep[prev[i]] = one
                pi_hat = ((one - beta[i]) * keep + beta[i] * pi_opt).astype(ft)
                fresh, _, gap_f = inv_cdf(pi_opt, ft(uniform[t, i, 0]))
                cont, _, gap_c = inv_cdf(pi_hat, ft(uniform[t, i, 1]))
                o = fresh if init[i] else cont
                if force_option is not None:
                    o, gap_f, gap_c = int(force_option), float("inf"), float("inf")
                a, lp, ent, gap_a = categorical(logits[i, o].astype(ft), ft(uniform[t, i, 2]))
                margin = min(margin, gap_f if init[i] else gap_c, gap_a)
                row["logits"].append(logits[i, o]); row["option"].append(o); row["action"].append(a)
                row["log_pi_a"].append(lp); row["entropy"].append(ent)
            acts = np.asarray(row["action"], dtype=np.int64)
            nxt, done = [], []
            for i, env in enumerate(envs):
                s, _, d, info = env.step(int(acts[i]))
                if d:
                    events.append((step0 + t, i, float(info['episodic_return'])))
                    s = env.reset()
                nxt.append(s)
                done.append(d)
            out["state"].append(x)
            out["q"].append(q.astype(np.float64)); out["beta"].append(beta.astype(np.float64))
            out["logits"].append(np.asarray(row["logits"], dtype=np.float64))
            out["option"].append(np.asarray(row["option"], dtype=np.int64)); out["prev_option"].append(prev.copy())
            out["action"].append(acts); out["init"].append(init.astype(np.float32))
            out["log_pi_a"].append(np.asarray(row["log_pi_a"], dtype=np.float64))
            out["entropy"].append(np.asarray(row["entropy"], dtype=np.float64))
            out["reward"].append(np.full(n, np.float32(1.0 * reward_coef), dtype=np.float32))
            out["mask"].append(1.0 - np.asarray(done, dtype=np.float32))
            prev, init = np.asarray(row["option"], dtype=np.int64), np.asarray(done, dtype=bool)
            raw = np.stack(nxt)
        qt, bt, _ = [v.to(F64).numpy() for v in forward(pt, raw.astype(np.float32), gate)]
        w = np.arange(n)
        boot = (1.0 - bt[w, prev]) * qt[w, prev] + bt[w, prev] * qt.max(axis=1)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(events=events, raw_states=raw, margin=margin, q_gap=q_gap, bootstrap=boot, bootstrap_state=raw.astype(np.float32),
               prev_option_out=prev, is_initial_out=init, eps=eps.copy())
    return res


def detached_terms(q, option, prev_option, ret, eps, term_reg):
    """OptionCritic_agent.py:99-105 in fp64 from the STORED q [T, N, O]: (advantage, beta_advantage) [T, N]."""
    q = np.asarray(q, dtype=np.float64)
    pick = lambda idx: np.take_along_axis(q, np.asarray(idx, dtype=np.int64)[..., None], axis=-1)[..., 0]
    e = np.asarray(eps, dtype=np.float64).reshape(-1, 1)
    v = q.max(axis=-1) * (1.0 - e) + q.mean(axis=-1) * e
    return ret - pick(option), pick(prev_option) - v + term_reg


def loss_and_grads(params, inp, eps, discount, term_reg, ent_w, gate="relu"):
    """fp64: `inp` holds what a rollout leaves (state [T, N, 4], q [T, N, O], option / prev_option / action / init / reward / mask
    [T, N], bootstrap [N]) -> dict(ret, adv, beta_adv [T, N], loss [4] = (total, q_loss, pi_loss, beta_loss), grads {name:
    gradient of pi_loss + q_loss + beta_loss}, z1, z2).  The detached terms come from the stored q, the graph from a forward of
    the stored states: what the reference's storage held."""
    p = to_t(params, requires_grad=True)
    t_len, n = np.asarray(inp["reward"]).shape
    rows = t_len * n
    ret = returns(inp["reward"], inp["mask"], inp["bootstrap"], discount)
    adv, badv = detached_terms(inp["q"], inp["option"], inp["prev_option"], ret, eps, term_reg)
    keep = {}
    q, beta, logits = forward(p, np.asarray(inp["state"], dtype=np.float64).reshape(rows, -1), gate, keep)
    col = lambda k: torch.as_tensor(np.asarray(inp[k]), dtype=torch.int64).reshape(rows, 1)
    f = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(rows, 1)
    option, prev, action = col("option"), col("prev_option"), col("action")
    lg = logits[torch.arange(rows), option.view(-1)]
    log_pi, pi = torch.log_softmax(lg, dim=-1), torch.softmax(lg, dim=-1)
    entropy = -(pi * log_pi).sum(-1, keepdim=True)
    q_loss = (q.gather(1, option) - f(ret)).pow(2).mul(0.5).mean()
    pi_loss = (-(log_pi.gather(1, action) * f(adv)) - ent_w * entropy).mean()
    beta_loss = (beta.gather(1, prev) * f(badv) * (1 - f(inp["init"]))).mean()
    total = pi_loss + q_loss + beta_loss
    names = list(p)
    grads = torch.autograd.grad(total, [p[k] for k in names])
    return dict(ret=ret, adv=adv, beta_adv=badv, loss=np.asarray([float(v.detach()) for v in (total, q_loss, pi_loss, beta_loss)]),
                grads={k: g.numpy() for k, g in zip(names, grads)}, z1=keep["z1"].numpy(), z2=keep["z2"].numpy())


def oc_update(params, roll, discount, term_reg, ent_w, gradient_clip, lr, gate="relu", square_avg=None):
    """One OptionCriticAgent.step's update on a rollout of this module -> (new parameters, dict of the losses' terms and the
    optimiser's running averages)."""
    inp = dict(roll, bootstrap=roll["bootstrap"])
    out = loss_and_grads(params, inp, roll["eps"], discount, term_reg, ent_w, gate)
    new, sq = rmsprop_step(params, out["grads"], gradient_clip, lr, square_avg=square_avg)
    out["square_avg"] = sq
    return new, out
