"""The pieces deeprl_amd/mlp_rollout.py shares between a2c_mlp, cat_mlp, ppo_mlp and dpg_mlp: the ONE two-layer-FCBody check gives
the verdicts each module's own copy of it gave, and the shared why_not names a reason wherever a2c_mlp.eligible (which is silent)
returns None.  No GPU: shapes and decisions only."""
import pytest
import torch
import torch.nn.functional as F

from test_a2c_continuous_host import _Agent, _Fused, _net as _gauss_net


CASES = {      # name -> (FCBody arguments, what fc_body must return behind the input width); the cases of the four modules' host tests
    "two-layer relu": (dict(hidden_units=(64, 64), gate=F.relu), (64, 64, 1)),
    "two-layer tanh": (dict(hidden_units=(32, 32), gate=torch.tanh), (32, 32, 2)),
    "unequal widths": (dict(hidden_units=(400, 300), gate=torch.relu), (400, 300, 1)),
    "three-layer": (dict(hidden_units=(64, 64, 64)), None),
    "one-layer": (dict(hidden_units=(64,)), None),
    "noisy": (dict(hidden_units=(64, 64), noisy_linear=True), None),
    "sigmoid gate": (dict(hidden_units=(64, 64), gate=torch.sigmoid), None),
    "missing bias": (dict(hidden_units=(64, 64)), None),
}


def _body(d, case, in_dim=17):
    body = d.FCBody(in_dim, **CASES[case][0])
    if case == "missing bias":
        body.layers[1].bias = None
    return body


def _old_check(d, body, equal_widths, tanh_only):
    """The condition as a2c_mlp.shape, cat_mlp.shape, ppo_mlp._mlp_shape (equal widths; ppo: tanh alone) and dpg_mlp._mlp_dims
    (any two widths) each wrote it out before they shared it."""
    gates = {F.relu: 1, torch.relu: 1, torch.tanh: 2, F.tanh: 2}
    gate_ok = body.gate is torch.tanh if tanh_only else body.gate in gates
    if type(body) is not d.FCBody or body.noisy_linear or not gate_ok or len(body.layers) != 2:
        return False
    if any(type(layer) is not d.nets.Linear or layer.bias is None for layer in body.layers):
        return False
    w1, w2 = body.layers[0].weight, body.layers[1].weight
    return w2.shape[1] == w1.shape[0] and (not equal_widths or w2.shape[0] == w1.shape[0])


@pytest.mark.parametrize("case", list(CASES))
def test_one_fc_body_check_gives_the_four_old_verdicts(case):
    import deeprl_amd as d
    from deeprl_amd import a2c_mlp, cat_mlp, dpg_mlp, mlp_rollout, ppo_mlp
    d.select_device(-1)
    body, tail = _body(d, case), CASES[case][1]
    want = None if tail is None else (17,) + tail
    assert mlp_rollout.fc_body(body) == want
    any_widths, one_width, one_width_tanh = (_old_check(d, body, *flags) for flags in ((False, False), (True, False), (True, True)))
    assert any_widths == (want is not None) and one_width == (any_widths and want[1] == want[2])
    assert one_width_tanh == (one_width and want[3] == 2)
    adam = lambda p: torch.optim.Adam(p, lr=1e-3)
    ddpg = d.DeterministicActorCriticNet(17, 6, actor_opt_fn=adam, critic_opt_fn=adam, actor_body=body, critic_body=_body(d, case, 23))
    assert (dpg_mlp.shape(ddpg) is not None) == any_widths
    gauss = d.GaussianActorCriticNet(17, 6, actor_body=body, critic_body=_body(d, case))
    assert (a2c_mlp.shape(gauss) is not None) == one_width
    assert (ppo_mlp._mlp_shape(gauss) is not None) == one_width_tanh
    assert (cat_mlp.shape(d.CategoricalActorCriticNet(17, 2, _body(d, case))) is not None) == one_width


def test_heads_must_be_plain_biased_linear_layers():
    import deeprl_amd as d
    from deeprl_amd import mlp_rollout
    d.select_device(-1)
    net = _gauss_net(d)
    assert mlp_rollout.head_out(net.fc_action, 64) == 6 and mlp_rollout.head_out(net.fc_critic, 64) == 1
    assert mlp_rollout.head_out(net.fc_action, 32) is None
    net.fc_critic.bias = None
    assert mlp_rollout.head_out(net.fc_critic, 64) is None
    assert mlp_rollout.head_out(torch.nn.Linear(64, 1), 64) is None


def test_shared_why_not_names_a_reason_wherever_the_gaussian_path_is_refused():
    """a2c_mlp.eligible returns None without a word; mlp_rollout.why_not(a2c_mlp.Rollout, agent) says which condition failed."""
    import deeprl_amd as d
    from deeprl_amd import a2c_mlp, mlp_rollout
    d.select_device(-1)
    why = lambda agent: mlp_rollout.why_not(a2c_mlp.Rollout, agent)
    good = _Agent(d, _gauss_net(d))
    assert a2c_mlp.eligible(good) == (17, 6, 64, 1) and why(good) is None
    hooked, parallel, partial = _Agent(d, _gauss_net(d)), _Agent(d, _gauss_net(d)), _Agent(d, _gauss_net(d))
    hooked.grad_hook = lambda g: None
    parallel.dp = type("Dp", (), {"active": True})()
    partial._fused = _Fused(list(partial.network.parameters())[1:])
    refused = [(_Agent(d, _gauss_net(d), fused_a2c_mlp=False), "fused_a2c_mlp"),
               (_Agent(d, _gauss_net(d, actor=(64, 32), critic=(64, 32))), "network"),
               (_Agent(d, _gauss_net(d, gates=(torch.tanh, torch.relu))), "network"),
               (_Agent(d, _gauss_net(d, actor=(48, 48), critic=(48, 48))), "not built for"),
               (_Agent(d, _gauss_net(d), num_workers=65), "not built for"),
               (hooked, "grad_hook"), (parallel, "data parallel"), (partial, "optimiser")]
    for agent, word in refused:
        assert a2c_mlp.eligible(agent) is None and word in why(agent), word
