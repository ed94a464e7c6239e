"""The pieces deeprl_amd/mlp_rollout.py shares between a2c_mlp, cat_mlp, ppo_mlp and dpg_mlp: the ONE two-layer-FCBody check gives
the verdicts each module's own copy of it gave, and the shared why_not names a reason wherever a2c_mlp.eligible (which is silent)
returns None; and what the cart-pole feature entries' host sides share: the net-struct filler, the target network's conditions, the
agents' pickled side file.  No GPU: shapes and decisions only."""
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


# ------------------------------------------------------------------------------------------ what the feature entries' host sides share
class _Flat:
    """A FlatParams as fill_net and target_why_not read it: one buffer, the parameters at stated offsets."""

    def __init__(self, params, offsets):
        self.params, self.offsets = list(params), list(offsets)
        self.flat = torch.zeros(max(self.offsets) + 8)

    def offset_of(self, p):
        return next(o for q, o in zip(self.params, self.offsets) if q is p)


@pytest.mark.parametrize("module, dims, shp", [
    ("q_mlp", ("state_dim", "n_actions", "hidden", "gate"), (4, 2, 64, 1)),
    ("oc_mlp", ("state_dim", "n_actions", "hidden", "gate", "n_options"), (4, 2, 32, 2, 3)),
    ("dist_mlp", ("state_dim", "n_actions", "hidden", "gate", "head", "n_atoms"), (4, 2, 16, 1, 2, 20)),
    ("cat_mlp", ("state_dim", "n_actions", "hidden", "gate"), (4, 2, 64, 2))])
def test_fill_net_writes_every_offset_and_dim(module, dims, shp):
    """With a target (q_mlp.Net, oc_mlp.Net, dist_mlp.Net) and without one (cat_mlp.Net has no such field): both pointers, every
    offset field at its parameter's offset and every dim; nothing else of the struct is touched."""
    import importlib
    from deeprl_amd import mlp_rollout
    Net = importlib.import_module("deeprl_amd." + module).Net
    names = [f[0] for f in Net._fields_]
    has_target = "target" in names
    offset_fields = [n for n in names if n not in dims and n not in ("param", "target", "v_min", "v_max")]
    params = [torch.zeros(1) for _ in offset_fields]
    offsets = [3 + 7 * i for i in range(len(params))]
    flat, target = _Flat(params, offsets), _Flat(params, [0] * len(params))
    n = mlp_rollout.fill_net(Net(), flat, list(zip(offset_fields, params)), dims, shp, target if has_target else None)
    assert type(n) is Net and n.param == flat.flat.data_ptr()
    if has_target:
        assert n.target == target.flat.data_ptr() != n.param
    assert [getattr(n, f) for f in offset_fields] == offsets
    assert tuple(getattr(n, f) for f in dims) == shp
    assert all(getattr(n, f) == 0.0 for f in names if f in ("v_min", "v_max"))
    if not has_target:
        with pytest.raises(AttributeError):
            Net().target


def test_target_why_not_returns_each_reason_and_none():
    from deeprl_amd import mlp_rollout
    online, target = [torch.zeros(2), torch.zeros(3)], [torch.zeros(2), torch.zeros(3)]
    fields = lambda net: list(zip(("w", "b"), net.p))
    shape = lambda net: net.shp
    net = lambda p, shp: type("N", (), {"p": p, "shp": shp})()

    def agent(target_shp, target_offsets):
        a = type("A", (), {})()
        a.network, a.target_network = net(online, (4, 2, 64, 1)), net(target, target_shp)
        a._fused = _Fused(online)
        a._fused.flat = _Flat(online, [0, 8])
        a._target_flat = _Flat(target, target_offsets)
        return a
    why = lambda a: mlp_rollout.target_why_not(a, shape, fields, (4, 2, 64, 1), "the caller's words")
    assert why(agent((4, 2, 64, 1), [0, 8])) is None
    assert why(agent((4, 2, 32, 1), [0, 8])) == "the caller's words"
    assert why(agent(None, [0, 8])) == "the caller's words"
    assert why(agent((4, 2, 64, 1), [0, 4])) == "the online and the target parameters are laid out differently in their flat buffers"
    assert why(agent((4, 2, 32, 1), [0, 4])) == "the caller's words"          # the shape is asked first
    # the ownership condition, next to it: every parameter the kernel reads is one the optimiser's flat buffer holds
    a = agent((4, 2, 64, 1), [0, 8])
    assert mlp_rollout.unowned(a, fields) is None
    a._fused.flat.params = online[:1]
    assert mlp_rollout.unowned(a, fields) == "one optimiser does not own every parameter the kernel reads"


def test_side_file_round_trips_and_is_none_when_absent(tmp_path):
    import numpy as np
    from deeprl_amd import agents
    name = str(tmp_path / "checkpoint")
    assert agents._read_side(name, ".envs") is None
    state = dict(step=41, seed=7, ring=np.arange(6, dtype=np.float64).reshape(2, 3), nested=dict(a=[1, 2]))
    agents._write_side(name, ".envs", state)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["checkpoint.envs"]
    got = agents._read_side(name, ".envs")
    assert set(got) == set(state) and got["step"] == 41 and got["seed"] == 7 and got["nested"] == dict(a=[1, 2])
    assert got["ring"].dtype == np.float64 and np.array_equal(got["ring"], state["ring"])
    assert agents._read_side(name, ".sampler") is None                       # (another suffix is another file)
