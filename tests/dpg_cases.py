"""What tests/test_dpg_update_host.py and tests/test_gpu_dpg_update.py share: the recorded reference updates
(tests/golden/ddpg_td3/ddpg_td3_update.npz, written by tests/golden/make_golden_ddpg_td3_update.py) as restatement states, and
random cases for the kernel-level comparisons."""
import os

import numpy as np
import torch

import dpg_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ddpg_td3", "ddpg_td3_update.npz")
# case -> (n_critics, policy step)
FIXTURE_CASES = {"b8_ddpg": (1, True), "b8_td3_policy": (2, True), "b8_td3_critic": (2, False),
                 "b20_ddpg": (1, True), "b20_td3_policy": (2, True), "b20_td3_critic": (2, False)}
GATE_RELU, GATE_TANH = 1, 2


def fixture_hyper(g):
    discount, mix, lr, noise, clip, delay = [float(x) for x in g["hyper"]]
    return dict(discount=discount, target_network_mix=mix, lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, td3_noise=noise,
                td3_noise_clip=clip, action_low=-1.0, action_high=1.0), int(delay)


def _sub(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def fixture_case(g, case):
    """(State before, batch, noise or None, dict of the reference's tensors after) of one recorded update."""
    nc, _ = FIXTURE_CASES[case]
    pre = case + "_before_"
    st = R.State(R.canonical(_sub(g, pre + "online_"), nc), R.canonical(_sub(g, pre + "target_"), nc), nc, GATE_RELU,
                 exp_avg=R.canonical(_sub(g, pre + "m_"), nc), exp_avg_sq=R.canonical(_sub(g, pre + "v_"), nc))
    st.t_actor, st.t_critic = int(g[pre + "t_actor"]), int(g[pre + "t_critic"])
    batch = {k: g["%s_batch_%s" % (case, k)] for k in ("state", "action", "reward", "next_state", "mask")}
    noise = g[case + "_noise"] if nc == 2 else None
    post = case + "_after_"
    after = dict(online=R.canonical(_sub(g, post + "online_"), nc), target=R.canonical(_sub(g, post + "target_"), nc),
                 m=R.canonical(_sub(g, post + "m_"), nc), v=R.canonical(_sub(g, post + "v_"), nc),
                 t_actor=int(g[post + "t_actor"]), t_critic=int(g[post + "t_critic"]))
    return st, batch, noise, after


def random_case(dims, n_critics, seed, head_scale=1.0):
    """(online, target) canonical fp64 parameter dicts with fp32-representable values, a batch with terminal rows, hyper."""
    b, s, a, h1, h2 = dims
    rs = np.random.RandomState(seed)

    def net():
        p = {}
        for role, k_in, n_out in [("a", s, a)] + [("c%d" % c, s + a, 1) for c in range(n_critics)]:
            for lay, shp, fan in (("w1", (h1, k_in), k_in), ("b1", (h1,), k_in), ("w2", (h2, h1), h1), ("b2", (h2,), h1),
                                  ("w3", (n_out, h2), h2), ("b3", (n_out,), h2)):
                v = rs.uniform(-1.0, 1.0, size=shp) * (1.5 / np.sqrt(fan)) * (head_scale if lay == "w3" else 1.0)
                p["%s.%s" % (role, lay)] = torch.as_tensor(v.astype(np.float32).astype(np.float64))
        return p

    online = net()
    target = {k: torch.as_tensor((v.numpy() + 0.05 * rs.randn(*v.shape) / np.sqrt(max(v.shape[-1], 1))).astype(np.float32)
                                 .astype(np.float64)) for k, v in online.items()}
    batch = dict(state=rs.randn(b, s).astype(np.float32), action=rs.uniform(-1, 1, size=(b, a)).astype(np.float32),
                 reward=rs.randn(b).astype(np.float32), next_state=rs.randn(b, s).astype(np.float32),
                 mask=(rs.rand(b) > 0.3).astype(np.float32))
    batch["mask"][0] = 0.0
    batch["mask"][-1] = 1.0 if b > 1 else 0.0
    hyper = dict(discount=0.99, target_network_mix=5e-3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, td3_noise=0.2,
                 td3_noise_clip=0.3, action_low=-1.0, action_high=1.0)
    return online, target, batch, hyper
